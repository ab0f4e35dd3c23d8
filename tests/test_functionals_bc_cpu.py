"""Host side of the force functionals with time-varying Dirichlet values
(`fem.functionals`: `cab`, `cmb`, `evaluate(..., dbc=, dbc_prev=)`,
`boundary_torque`) and the table rows `_ImexLoop.run_slice` hands the
functionals' log.

Shapes: `scenarios.toy_problem()` (NV = 1286, NP = 207, 348 cells, 240
Dirichlet dofs; the obstacle has 15 nodes).  Tolerance against the
un-condensed balance: `1e-12 * T_k`, `T_k` the sum of the absolute values of
every product of functional k (`evaluate(..., return_scale=True)`, which
counts the products of `cab` and `cmb` too): both sides are fp64 sums of a few
thousand products, as in `tests/test_functionals_cpu.py`.
"""
import numpy as np
import pytest
import scipy.sparse as sps

TOL = 1e-12
CENTER = (0.2, 0.2)


def obstacle_nodes(th, dbcinds, dbcvals):
    """the P2 nodes of the obstacle: boundary nodes away from the channel's
    walls, inflow and outflow"""
    nodes, xy = th.boundary_nodes()
    x, y = xy[:, 0], xy[:, 1]
    inner = (x > 1e-9) & (x < 2.2 - 1e-9) & (y > 1e-9) & (y < 0.41 - 1e-9)
    return nodes[inner]


def rotating_split(prob):
    """`(statinds, statvals, cntinds, xy of the controlled nodes)`: the
    obstacle's dofs controlled, every other Dirichlet dof static; the
    controlled dofs node by node, x then y"""
    th = prob['th']
    dbcinds = np.asarray(prob['dbcinds'], dtype=np.int64)
    dbcvals = np.asarray(prob['dbcvals'], dtype=np.float64)
    nodes = obstacle_nodes(th, dbcinds, dbcvals)
    cnt = np.stack([2*nodes, 2*nodes + 1], axis=1).reshape(-1)
    assert np.all(np.isin(cnt, dbcinds))
    stat = ~np.isin(dbcinds, cnt)
    return dbcinds[stat], dbcvals[stat], cnt, nodes


def rotation(th, nodes, omega):
    """`omega * (-(y - yc), x - xc)` on `nodes`, node by node, x then y"""
    xy = th.nodecoords[nodes]
    return omega*np.stack([-(xy[:, 1] - CENTER[1]), xy[:, 0] - CENTER[0]],
                          axis=1).reshape(-1)


def moving_femp(prob, statinds, cntinds, statvals, cntvals):
    """the problem dict of functionals whose Dirichlet dofs are ordered
    static first, controlled behind them"""
    return dict(invinds=prob['invinds'], nu=prob['nu'],
                dbcinds=np.concatenate([statinds, cntinds]),
                dbcvals=np.concatenate([statvals, cntvals]))


def bump(th, radius, center):
    xy = th.nodecoords
    r2 = ((xy - np.asarray(center)[None, :])**2).sum(axis=1)/radius**2
    b = np.where(r2 < 1., (1. - np.minimum(r2, 1.))**2, 0.)
    phi = np.zeros(th.vdim)
    phi[0::2] = b
    phi[1::2] = -.5*b
    return phi


@pytest.fixture(scope='module')
def setup(toy_prob):
    from dolfin_navier_scipy_amd import fem
    prob, th = toy_prob, toy_prob['th']
    statinds, statvals, cntinds, nodes = rotating_split(prob)
    assert nodes.size == 15 and statinds.size == 210
    femp = moving_femp(prob, statinds, cntinds, statvals,
                       np.zeros(cntinds.size))
    phib = bump(th, 0.3, (0., 0.2))
    fn = (fem.boundary_forces(th, femp, nodes=nodes)
          + fem.boundary_torque(th, femp, nodes=nodes, center=CENTER)
          + fem.MomentumFunctionals(th, femp, phib.reshape((-1, 1)),
                                    names=['bump'])
          + fem.pressure_difference(th, (0.15, 0.2), (0.3, 0.2)))
    phis = np.zeros((th.vdim, 4))
    phis[2*nodes, 0] = 1.
    phis[2*nodes + 1, 1] = 1.
    xy = th.nodecoords[nodes]
    phis[2*nodes, 2] = -(xy[:, 1] - CENTER[1])
    phis[2*nodes + 1, 2] = xy[:, 0] - CENTER[0]
    phis[:, 3] = phib
    rng = np.random.default_rng(5)
    u, up = rng.standard_normal(th.vdim), rng.standard_normal(th.vdim)
    # (the static dofs keep their values, the controlled ones differ)
    u[statinds] = up[statinds] = statvals
    NP = prob['smc']['J'].shape[0]
    return dict(prob=prob, th=th, fn=fn, femp=femp, phis=phis, u=u, up=up,
                p=rng.standard_normal(NP), dt=1./128, nodes=nodes,
                dbi=femp['dbcinds'], inv=np.asarray(prob['invinds']))


def test_shapes_of_the_toy_problem(setup):
    th, fn, prob = setup['th'], setup['fn'], setup['prob']
    NP, NV = prob['smc']['J'].shape
    assert (NV, NP, th.mesh.ncells, setup['dbi'].size) == (1286, 207, 348, 240)
    assert fn.names == ['fx', 'fy', 'torque', 'bump', 'dp'] and fn.nF == 5
    assert [c.size for c in fn.cells] == [28, 28, 28, 44, 0]
    assert fn.cab.shape == fn.cmb.shape == (5, 240)
    # the bump reaches Dirichlet dofs, the pressure difference none
    assert fn.cab[3].nnz > 0 and fn.cmb[3].nnz > 0
    assert fn.cab[4].nnz == 0 and fn.cmb[4].nnz == 0


def test_against_the_uncondensed_balance(setup):
    s, fn, th = setup, setup['fn'], setup['th']
    st = s['prob']['stms']
    u, up, p, dt = s['u'], s['up'], s['p'], s['dt']
    v, vp = u[s['inv']], up[s['inv']]
    g, gp = u[s['dbi']], up[s['dbi']]
    assert np.abs(g - gp).max() > 0.1
    y, T = fn.evaluate(v, vp, p, dt, return_scale=True, dbc=g, dbc_prev=gp)
    res = st['M'] @ ((u - up)/dt) + st['A'] @ u \
        + th.convection_vec(u)[:, 0] - st['J'].T @ p
    for k in range(4):
        ref = -float(s['phis'][:, k] @ res)
        print(fn.names[k], y[k], ref, abs(y[k] - ref)/T[k])
        assert abs(y[k] - ref) <= TOL*T[k], (k, y[k], ref, T[k])
    assert y[4] == fn.cp[4] @ p
    assert np.all(T >= np.abs(y))
    # the `cmb` term counts (where the functional reaches Dirichlet dofs)
    y2 = fn.evaluate(v, vp, p, dt, dbc=g, dbc_prev=g)
    assert np.all(np.abs(y2 - y)[:4] > 1e-6*T[:4])
    assert np.array_equal(y2, fn.evaluate(v, vp, p, dt, dbc=g))
    # and so do the values themselves
    y3 = fn.evaluate(v, vp, p, dt)
    assert np.all(np.abs(y3 - y)[:4] > 1e-6*T[:4])
    with pytest.raises(ValueError):
        fn.evaluate(v, vp, p, dt, dbc=g[:-1])
    with pytest.raises(ValueError):
        fn.evaluate(v, vp, p, dt, dbc_prev=g)


def test_constant_values_give_the_static_functional(setup):
    s, fn = setup, setup['fn']
    v, vp = s['u'][s['inv']], s['up'][s['inv']]
    g0 = np.asarray(s['femp']['dbcvals'])
    y0, T0 = fn.evaluate(v, vp, s['p'], s['dt'], return_scale=True)
    y1, T1 = fn.evaluate(v, vp, s['p'], s['dt'], return_scale=True, dbc=g0,
                         dbc_prev=g0)
    assert np.all(np.abs(y1 - y0) <= 1e-13*T1)
    # ... with the problem's own (non-zero: the inflow) values
    from dolfin_navier_scipy_amd import fem
    prob = s['prob']
    femp = dict(invinds=prob['invinds'], nu=prob['nu'],
                dbcinds=prob['dbcinds'], dbcvals=prob['dbcvals'])
    fb = fem.MomentumFunctionals(s['th'], femp, s['phis'][:, 3:4])
    gv = np.asarray(prob['dbcvals'], dtype=np.float64)
    assert np.abs(fb.c0).max() > 0 and np.all(fb.c0b == 0)
    y0, T0 = fb.evaluate(v, vp, s['p'], s['dt'], return_scale=True)
    y1, T1 = fb.evaluate(v, vp, s['p'], s['dt'], return_scale=True, dbc=gv,
                         dbc_prev=gv)
    assert np.all(np.abs(y1 - y0) <= 1e-13*T1) and np.all(T1 >= T0)


def test_stacking_and_device_layout(setup):
    from dolfin_navier_scipy_amd import fem
    s, fn, th = setup, setup['fn'], setup['th']
    forces = fem.boundary_forces(th, s['femp'], nodes=s['nodes'])
    dp = fem.pressure_difference(th, (0.15, 0.2), (0.3, 0.2))
    assert dp.cab.shape == (1, 0)
    for both in (forces + dp, dp + forces):
        assert both.cab.shape == both.cmb.shape == (3, 240)
        assert both.c0b.shape == (3,)
    assert np.array_equal((forces + dp).cab.toarray()[:2],
                          forces.cab.toarray())
    assert np.array_equal((dp + forces).cmb.toarray()[1:],
                          forces.cmb.toarray())
    sc = forces.scaled([2., 3.])
    assert sc.cab is forces.cab and sc.cmb is forces.cmb
    assert np.array_equal(sc.scale, [-2., -3.])
    wr = forces.without_rate()
    assert wr.cmb.nnz == 0 and wr.cmb.shape == forces.cmb.shape
    assert wr.cm.nnz == 0 and np.array_equal(wr.cab.toarray(),
                                             forces.cab.toarray())
    v, vp = s['u'][s['inv']], s['up'][s['inv']]
    g, gp = s['u'][s['dbi']], s['up'][s['dbi']]
    assert np.array_equal(
        wr.evaluate(v, vp, s['p'], s['dt'], dbc=g, dbc_prev=gp),
        forces.evaluate(v, v, s['p'], s['dt'], dbc=g, dbc_prev=g))
    # rows given by the caller: no boundary terms, the constant stays
    rows = fem.MomentumFunctionals.from_rows(
        th, s['femp'], ca=sps.csr_matrix(np.ones((1, v.size))), c0=[.25])
    assert rows.cab.shape == (1, 240) and rows.cab.nnz == 0
    assert rows.c0b[0] == .25
    assert rows.evaluate(v, vp, s['p'], s['dt'], dbc=g, dbc_prev=gp)[0] == \
        rows.evaluate(v, vp, s['p'], s['dt'])[0]
    # functionals of other Dirichlet dofs do not stack
    other = dict(s['femp'], dbcinds=s['femp']['dbcinds'][::-1],
                 dbcvals=s['femp']['dbcvals'][::-1])
    with pytest.raises(ValueError):
        forces + fem.boundary_forces(th, other, nodes=s['nodes'])
    # the device layouts
    args = fn.device_args(moving=True)
    assert args['cab'].shape == args['cmb'].shape == (5, 240)
    assert args['ca'].shape == (5, 1286) and args['cp'].shape == (5, 207)
    assert np.array_equal(args['c0'], np.zeros(5))
    assert args['cell_ptr'].tolist() == [0, 28, 56, 84, 128, 128]
    assert args['cell_w'].size == 12*128
    old = fn.device_args()
    assert set(old) == {'ca', 'cm', 'cp', 'c0', 'scale', 'cell_ptr',
                        'cell_idx', 'cell_w'}
    assert np.array_equal(old['c0'], fn.c0)


def test_torque_is_the_hand_built_test_vector(setup):
    from dolfin_navier_scipy_amd import fem
    s, th = setup, setup['th']
    tq = fem.boundary_torque(th, s['femp'], nodes=s['nodes'], center=CENTER)
    by_hand = fem.MomentumFunctionals(th, s['femp'], s['phis'][:, 2:3])
    assert tq.names == ['torque']
    for name in ('ca', 'cm', 'cp', 'cab', 'cmb'):
        assert np.array_equal(getattr(tq, name).toarray(),
                              getattr(by_hand, name).toarray())
    assert np.array_equal(tq.cells[0], by_hand.cells[0])
    assert np.array_equal(tq.weights[0], by_hand.weights[0])


class _StubStepper(object):
    """records what the slices upload; hands back zeros"""

    class _Sys(object):
        NV, NP = 3, 2

    def __init__(self):
        self.sys = self._Sys()
        self.armed, self.runs = [], []

    def set_convection(self, conv, scale=1.):
        pass

    def set_rhs_table(self, gv, gp):
        pass

    def set_rhs(self, gv, gp):
        pass

    def set_functionals(self, fn, nrows, dt, dbc_table=None):
        self.armed.append((nrows, None if dbc_table is None
                           else np.array(dbc_table)))

    def get_functionals(self, first, count):
        return np.zeros((count, 1))

    def set_recorder(self, n, cv_mat=None, snap_slots=None):
        self.nkept = int((np.asarray(snap_slots) >= 0).sum())

    def record_snapshots(self, first, count):
        return np.zeros((count, 3)), np.zeros((count, 2))

    def run(self, n, cf, opts):
        self.runs.append(n)

    def get_state(self):
        return np.zeros((3, 1)), np.zeros((2, 1))


class _StubConv(object):
    def __init__(self):
        self.tables = []

    def set_dbcvals(self, vals):
        pass

    def set_dbc_table(self, tab):
        self.tables.append(np.array(tab))


class _StubFn(object):
    nF, names, inv = 1, ['f'], np.zeros(3)
    cab = sps.csr_matrix((1, 3))


@pytest.mark.parametrize('record', [False, True])
def test_table_rows_for_slices_and_chunks_that_do_not_divide(record):
    """the functionals of the steps `a .. b` of a slice are armed with the
    rows `dbt[a .. b]` of the slice's table -- the values of the state before
    each step -- and the row behind it: `dbt[b]`, or the values at the slice's
    last time behind its last step; `n + 1` rows for `n` steps"""
    from dolfin_navier_scipy_amd import time_int_utils as tiu
    trange = np.linspace(0., 0.23, 24)
    dt, slices = tiu._inittimegrid(trange, ntimeslices=5)
    stat = [7.]

    def bcs(t):            # two controlled values, functions of the time
        return [float(t), float(-2*t)]
    stepper, conv = _StubStepper(), _StubConv()
    cur = tiu._Terms(bcs(trange[1]), 0., 0., 0., 0.)
    # (chunks: at most two snapshots each, so the slices of 4 steps, which
    # keep their last two, split unevenly)
    rsd = dict(bcs_time_only=True, static_dbcvals=stat, functionals=_StubFn(),
               record=record, record_bytes=2*8*64, savevp_times=())
    # (SBDF2 keeps the state before a slice's last step; its row is 0. here)
    rs = tiu._ImexLoop(
        tiu._SBDF2, stepper, None, None, dt, rsd, conv, bcs(trange[0]), False,
        prev=tiu._Terms(None, None, 0., None, None), cur=cur,
        getbcs=lambda t, v, p, mode=None: bcs(t),
        applybcs=lambda b: (0., 0., 0.), appndbcs=lambda v, b: v,
        f_tdp=lambda t: 0., g_tdp=lambda t: 0.,
        savevp=lambda v, p, time=None: None)
    assert rs.on_device and (rs.drec is not None) == record
    rs.attach(None, False, trange[1])
    tprev = trange[1]
    for ctrange in slices:
        if not len(ctrange):
            continue
        stepper.armed, conv.tables = [], []
        rs.run_slice(ctrange)
        times = [tprev] + list(ctrange)      # the states before / after
        want = np.array([stat + bcs(t) for t in times])
        assert sum(n for n, _ in stepper.armed) == len(ctrange)
        assert len(stepper.armed) == len(conv.tables)
        if not record:
            assert len(stepper.armed) == 1
        a = 0
        for (n, tab), ctab in zip(stepper.armed, conv.tables):
            assert tab.shape == (n + 1, 3)
            assert np.array_equal(tab, want[a:a + n + 1])
            # the operator's own table: the same rows without the last
            assert np.array_equal(ctab, want[a:a + n])
            a += n
        tprev = ctrange[-1]
    if record:
        assert max(len(c) for c in slices) > 2     # chunks did split
    # a functional built for another number of Dirichlet dofs is refused
    bad = dict(rsd, functionals=type('F', (_StubFn,),
                                     dict(cab=sps.csr_matrix((1, 4))))())
    rs2 = tiu._ImexLoop(
        tiu._SBDF2, stepper, None, None, dt, bad, conv, bcs(0.), False,
        prev=tiu._Terms(None, None, 0., None, None), cur=cur)
    with pytest.raises(ValueError):
        rs2.attach(None, False, trange[1])
