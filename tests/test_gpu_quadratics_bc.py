"""Device-resident quadratic functionals with moving Dirichlet values (the
moving-boundary instance of `k_quadratic_step`, `dns_imex_set_quadratics_bc` /
`_live`, `ImexStepper.set_quadratics(..., dbc_table=)`, `resident=dict(
quadratics=)` of `cnab` / `sbdftwo` with controlled boundaries): every row of
the device's log against the NumPy statement
`fem.QuadraticFunctionals.evaluate(..., dbc=, dbc_prev=)` on the states the
recorder wrote down in the same run and the table rows that belong to them.

Shapes: `scenarios.toy_problem()` (NV = 1286, NP = 207, 240 Dirichlet dofs, 30
of them on the obstacle), the stepper and the rotating obstacle of
`test_gpu_functionals_bc.py`.  The raw setter takes seeded general matrices over
`NV + ndbc` with `ndbc` in {1, 15, 240}: widths 1287, 1301, 1526, a last pass
of 7, 5 and 6 live rows of 16; among ordinary rows (about 20 entries) one of
130 entries that straddles column `NV` (more than two rounds of 16 lanes x 4),
an empty row, the last boundary row and an inner row with boundary columns
only; all four operand pairs on the first matrix, one form on a second, `qa` /
`qw` rows that reach into the boundary part; a table that varies per row.

Tolerance: `|row - evaluate| <= n_k 2^-52 T_k`, `T_k` the sum of the absolute
values of the `n_k` products of form k, boundary products included (in
`np.longdouble`): the a-priori bound of a sum of fp64 products in ANY order --
derived, not measured (`tests/test_gpu_quadratics.py`).  Measured on the
MI355X: worst 1.0e-4 of the bound with the raw setter, 2.3e-4 through the time
loops (`profiles/r18_closed_loop_budget/README.md`).
"""
import numpy as np
import pytest
import scipy.sparse as sps

import scenarios
from test_gpu_functionals_bc import DT, Loop, _loop_kw, gtiu, rot  # noqa: F401

pytestmark = pytest.mark.gpu

EPS = 2.**-52
NV = 1286


def _general(ndbc, seed):
    """non-symmetric over `NV + ndbc`, about 20 entries a row, with the rows
    the module's docstring lists"""
    n = NV + ndbc
    rng = np.random.default_rng(seed)
    R = sps.random(n, n, density=20./n, format='lil', random_state=rng)
    nb = min(ndbc, 65)
    odd = dict(straddle=(40, np.arange(NV + nb - 130, NV + nb)),
               empty=(41, np.zeros(0, dtype=np.int64)),
               inner_to_boundary=(900, NV + np.arange(ndbc)[:9]),
               boundary_to_boundary=(n - 1, NV + np.arange(ndbc)[-7:]))
    for row, cols in odd.values():
        R.rows[row] = cols.tolist()
        R.data[row] = rng.standard_normal(cols.size).tolist()
    R = sps.csr_matrix(R)
    R.sort_indices()
    lens = np.diff(R.indptr)
    assert lens[40] == 130 and lens[41] == 0
    assert R[40].indices.min() < NV <= R[40].indices.max()
    assert R[900].indices.min() >= NV and R[n - 1].indices.min() >= NV
    assert abs(R - R.T).max() > 0.1
    return R


def _forms(ndbc, seed=7):
    from dolfin_navier_scipy_amd import fem
    n = NV + ndbc
    rng = np.random.default_rng(seed)
    R, R2 = _general(ndbc, seed), _general(ndbc, seed + 1)

    def row(k):             # 40 entries anywhere, the boundary part for sure
        r = sps.random(1, n, density=40./n, format='lil', random_state=rng)
        r[0, NV + np.arange(ndbc)[::max(1, ndbc//8)]] = 1. + k
        return sps.csr_matrix(r)
    empty = sps.csr_matrix((1, n))
    qa = sps.vstack([row(0), empty, empty, row(1), empty]).tocsr()
    qw = sps.vstack([empty, row(2), empty, row(3), empty]).tocsr()
    qf = fem.QuadraticFunctionals.from_matrices(
        NV, [R, R2], [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0)],
        qa=qa, qw=qw, c0=[.3, 0., -.2, 0., 1.], scale=[.7, 1., 1., -2., 1.],
        names=['uRu', 'uRd', 'dRu', 'dRd', 'uR2u'], ndbc=ndbc)
    assert (qf.nM, qf.nQ, qf.N) == (2, 5, n)
    assert qf.qa[:, NV:].nnz > 0 and qf.qw[:, NV:].nnz > 0
    return qf


def _table(ndbc, nst, seed):
    """`(nst + 1, ndbc)`, another row for every state"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nst + 1, ndbc)) \
        + np.linspace(0., 1., nst + 1)[:, None]


def _check_rows(qf, rows, vs, v_first, tab, dt, what):
    """every row against `.evaluate` of the recorded states and the table
    rows that belong to them; returns the worst error in units of the bound"""
    assert rows.shape == (vs.shape[0], qf.nQ)
    assert tab.shape == (rows.shape[0] + 1, qf.ndbc)
    assert np.isfinite(rows).all()
    worst = np.zeros(qf.nQ)
    for r in range(rows.shape[0]):
        vprev = vs[r - 1] if r else np.asarray(v_first).reshape(-1)
        y, T, n = qf.evaluate(vs[r], vprev, dt, return_scale=True,
                              dbc=tab[r + 1], dbc_prev=tab[r])
        assert np.all(T > 0)
        worst = np.maximum(worst, np.abs(rows[r] - y)/(n*EPS*T))
    print(what, ': worst |row - evaluate| in units of n 2^-52 T per form',
          dict(zip(qf.names, worst)))
    assert np.all(worst <= 1.), (what, worst)
    return worst


def _recorded(lp, qf, tab, nst, how='run', max_grid=None, parts=None):
    """`nst` steps of `Loop` with recorder and quadratics on their own table:
    `(rows, vs, v before the first step)`"""
    v_first = lp.stp.get_state()[0][:, 0]
    lp.arm(None, nst)
    lp.stp.set_quadratics(qf, nst, lp.dt, max_grid=max_grid, dbc_table=tab)
    if how == 'run':
        for n in (parts or [nst]):
            lp.stp.run(n, lp.cf, lp.opts)
    else:
        for _ in range(nst):
            lp.stp.step(lp.cf, opts=lp.opts)
    vs, _ = lp.stp.record_snapshots()
    return lp.stp.get_quadratics(), vs, v_first


# ---- 1. the raw setter on its own table -------------------------------------------

@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
@pytest.mark.parametrize('ndbc', [1, 15, 240])
def test_rows_match_the_host_statement(gtiu, rot, scheme, ndbc):
    """8 steps, launched (`step`) and replayed (`run`), with the default grid
    (one pass per workgroup), `max_grid=3` (a workgroup's passes change
    matrix) and `max_grid=1`; re-armed each time, the matrices stay.  With
    `ndbc` = 240 the convection operator of the rotating obstacle is attached
    (its width), with 1 and 15 none is (the convection history stays
    frozen): the kernel reads the quadratics' own table either way"""
    nst = 8
    qf = _forms(ndbc)
    assert (NV + ndbc) % 16 == {1: 7, 15: 5, 240: 6}[ndbc]
    lp = Loop(rot, scheme)
    worst = np.zeros(qf.nQ)
    try:
        if ndbc != 240:
            lp.stp.set_convection(None)
        k = 0
        for how in ('step', 'run'):
            for grid in (None, 3, 1):
                tab = _table(ndbc, nst, seed=10*ndbc + k)
                rows, vs, v_first = _recorded(lp, qf, tab, nst, how, grid)
                want = {None: min(2*-(-(NV + ndbc)//16), 256), 3: 3, 1: 1}
                assert lp.stp.quadratics_grid() == want[grid]
                assert np.abs(vs[-1] - v_first).max() > 1e-6    # (it moves)
                worst = np.maximum(worst, _check_rows(
                    qf, rows, vs, v_first, tab, DT,
                    '{0} ndbc={1} {2} grid {3}'.format(scheme, ndbc, how,
                                                       grid)))
                # the table counts: other rows, another log
                y = qf.evaluate(vs[0], v_first, DT, dbc=tab[1], dbc_prev=tab[1])
                assert np.all(np.abs(rows[0] - y)[1:4] > 0)
                k += 1
    finally:
        lp.close()
    print(scheme, 'ndbc', ndbc, ': worst fraction of the bound', worst.max())


# ---- 2. deterministic ---------------------------------------------------------------

def test_logs_are_deterministic(gtiu, rot):
    qf, tab = _forms(240), _table(240, 8, seed=5)
    out = []
    for parts in (None, None, [3, 5]):
        lp = Loop(rot)
        try:
            out.append(_recorded(lp, qf, tab, 8, parts=parts))
        finally:
            lp.close()
    (r0, v0, _), (r1, v1, _), (r2, v2, f2) = out
    assert np.array_equal(v0, v1)
    assert np.array_equal(r0, r1)
    # one call against two: the same bits wherever the states are the same bits
    same = [r for r in range(8) if np.array_equal(v0[r], v2[r])
            and (r == 0 or np.array_equal(v0[r - 1], v2[r - 1]))]
    print('run(8) vs run(3) + run(5): states identical in', len(same), 'of 8')
    assert len(same) >= 1
    assert np.array_equal(r0[same], r2[same])
    if len(same) < 8:
        _check_rows(qf, r2, v2, f2, tab, DT, 'run(3) + run(5)')


# ---- 3. through the drop-ins ----------------------------------------------------------

@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_through_the_time_loops(gtiu, rot, scheme):
    """`bcs_time_only` on the rotating obstacle, 32 time steps over the
    slices of `ntimeslices=3`, the device recording: every row against
    `evaluate` of the states `savevp` saw with the boundary values it was
    handed; the trajectory is the one of the same loop without quadratics, bit
    for bit"""
    from dolfin_navier_scipy_amd import convection, fem
    inv, dbi = rot['inv'], rot['dbi']
    qf = fem.energy_budget(rot['th'], rot['femp'], moving=True)
    assert (qf.NV, qf.ndbc) == (NV, 240)
    integ = gtiu.cnab if scheme == 'cnab' else gtiu.sbdftwo
    got = {}
    for mode in ('with', 'without'):
        rec = scenarios.Recorder()
        kw = _loop_kw(rot, rec)
        kw.pop('f_vdp')
        cvop = convection.ConvectionP2.from_taylor_hood(
            rot['th'], inv, dbi, rot['femp']['dbcvals'])
        resident = dict(static_dbcvals=rot['statvals'].tolist(),
                        bcs_time_only=True, record=True)
        if mode == 'with':
            resident.update(quadratics=qf)
        try:
            v, p, ff = integ(resident=resident, device_convection=cvop,
                             invinds=inv, **kw)
        finally:
            cvop.close()
        assert ff == 0
        got[mode] = (dict(gtiu.LAST_RUN), rec.arrays(), v, p)
    lr, (times, vels, prss), v, p = got['with']
    assert lr['quadratics_on'] == 'device' and lr['record'] == 'device'
    assert lr['run_calls'] == 4 and times.size == 33
    assert lr['quadratics'].shape == (31, 4)
    assert lr['quadratics_names'] == ['ekin', 'dissipation', 'ekin_rate',
                                      'rate_norm']
    vs = np.array([vf[inv] for vf in vels[2:]])
    tab = np.array([vf[dbi] for vf in vels[1:]])
    assert np.abs(np.diff(tab, axis=0)).max() > 1e-3
    _check_rows(qf, lr['quadratics'], vs, vels[1][inv], tab, DT,
                scheme + ' bcs_time_only')
    rows = lr['quadratics']
    assert rows[:, 0].min() > 1e-2 and rows[:, 1].min() > 0.
    assert rows[:, 3].min() > 0.
    _, (_, vels0, prss0), v0, p0 = got['without']
    assert 'quadratics' not in got['without'][0]
    assert np.array_equal(vels, vels0) and np.array_equal(prss, prss0)
    assert np.array_equal(v, v0) and np.array_equal(p, p0)
    # forms that carry the values as constants are still refused here
    with pytest.raises(ValueError) as exc:
        integ(resident=dict(static_dbcvals=rot['statvals'].tolist(),
                            quadratics=fem.energy_budget(rot['th'],
                                                         rot['femp'])),
              **_loop_kw(rot, scenarios.Recorder()))
    assert 'moving Dirichlet' in str(exc.value)


# ---- 4. refusals -------------------------------------------------------------------------

def test_refusals(gtiu, rot):
    from dolfin_navier_scipy_amd import _capi
    qf, qf15, fn = _forms(240), _forms(15), rot['fn']
    lp = Loop(rot)
    try:
        stp = lp.stp
        lp.arm(None, 4)
        tab, tab15 = _table(240, 4, 1), _table(15, 4, 2)
        stp.set_quadratics(qf, 4, DT, dbc_table=tab)
        stp.run(2, lp.cf, lp.opts)
        rows = stp.get_quadratics()

        def refused(go, *words):
            with pytest.raises((_capi.DnsError, ValueError)) as exc:
                go()
            if isinstance(exc.value, _capi.DnsError):
                assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
            for word in words:
                assert word in str(exc.value), (word, str(exc.value))
        # another width than the attached operator's, at the setter (own
        # table and the operator's)
        refused(lambda: stp.set_quadratics(qf15, 4, DT, dbc_table=tab15),
                'ndbc = 15', '240')
        refused(lambda: stp.set_quadratics(qf15, 4, DT, dbc_table='operator'),
                'ndbc = 15', '240')
        # the operator's table: `lp.arm` gave it 4 rows, 4 steps need 5
        refused(lambda: stp.set_quadratics(qf, 4, DT, dbc_table='operator'),
                'quadratics', '4 rows', 'need 5')
        refused(lambda: stp.set_functionals(fn, 4, DT, dbc_table='operator'),
                'functionals', '4 rows', 'need 5')
        # what the Python layer sees itself
        refused(lambda: stp.set_quadratics(qf, 4, DT), 'dbc_table')
        refused(lambda: stp.set_quadratics(qf, 4, DT, dbc_table=tab[:4]),
                'dbc_table')
        refused(lambda: stp.set_quadratics(qf, 4, DT, dbc_table='table'),
                'operator')
        # a refused call leaves what was set
        assert np.array_equal(stp.get_quadratics(), rows)
        stp.run(2, lp.cf, lp.opts)
        # no operator at all
        stp.set_convection(None)
        refused(lambda: stp.set_quadratics(qf, 4, DT, dbc_table='operator'),
                'quadratics', 'no device convection operator')
        refused(lambda: stp.set_functionals(fn, 4, DT, dbc_table='operator'),
                'functionals', 'no device convection operator')
        # another width at the step: set without an operator, one attached
        stp.set_quadratics(qf15, 4, DT, dbc_table=tab15)
        stp.set_convection(lp.cvop, scale=-1.0)
        for go in (lambda: stp.run(1, lp.cf, lp.opts),
                   lambda: stp.step(lp.cf, opts=lp.opts)):
            refused(go, 'dns_imex_set_quadratics_bc', '15', '240')
        # the operator's table shortened behind the setter's back
        lp.cvop.set_dbc_table(np.tile(tab[0], (5, 1)))
        stp.set_quadratics(qf, 4, DT, dbc_table='operator')
        lp.cvop.set_dbc_table(np.tile(tab[0], (3, 1)))
        refused(lambda: stp.run(1, lp.cf, lp.opts), '3 rows', 'need 5')
    finally:
        lp.close()


def test_row_partitioned_stepper_is_refused(gtiu, rot):
    from dolfin_navier_scipy_amd import saddle, _capi, comm as dcomm
    M, A, J = rot['M'], rot['A'], rot['J']
    qf = _forms(15)
    cm = dcomm.Comm.rccl(0, 1, 0, dcomm.rccl_unique_id())
    system = saddle.SaddleSystem((M + .5*DT*A).tocsr(), J)
    stp = None
    try:
        system.set_comm(cm)
        system.setup_precond(cheb_degree=6, schur='dense', fhat='explicit')
        stp = saddle.ImexStepper(system, (M - .5*DT*A).tocsr())
        for table in (_table(15, 4, 3), 'operator'):
            with pytest.raises(_capi.DnsError) as exc:
                stp.set_quadratics(qf, 4, DT, dbc_table=table)
            assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
            assert 'partitioned' in str(exc.value)
    finally:
        if stp is not None:
            stp.close()
        system.set_comm(None)
        system.close()
        cm.close()
