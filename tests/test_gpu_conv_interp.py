"""Linear interpolation between the stored rows of a base trajectory on the
device: `ConvectionP2.set_base_rows(rows, weights)`, `set_base_row(row,
weight)`, `BaseTrajectory(interpolate=True)`, `ensemble_to_base(...,
interpolate=True)` (the interpolating instances of `k_conv_lin_cells<ADJ>` and
`k_conv_lin_cells_lane<ADJ>`):

 1. bit for bit: cell values and `apply` about row `r` with weight `theta`, both
    modes, both element kernels, against a second operator with
    `set_base_flow((V0 + th*(V1 - V0), Vd0 + th*(Vd1 - Vd0)))` formed in NumPy
    -- the contract of the three-operation formula, no tolerance; `theta` in
    {0.5, 0.25, 1/3, 2^-60, 1 - 2^-53} and 0 on every row, the last included;
    with `sel` lists, full vectors and a padded leading dimension,
 2. the same values inside `conv_lin_model.lin_model`'s counted bound about
    the NumPy-interpolated base (the count of the constant base: the
    interpolated vector is the model's exact input); `theta = 0.5` outside the
    bound of either end row,
 3. weight 0 is the hold: an all-zero weight table gives the bits of
    `set_base_rows` without weights, cell values and 12 `cnab` / `sbdf2` steps
    on the N=2 wake,
 4. index and weight tables in a stepper (ascending, descending, clamped past
    their end), both schemes, both modes, 12 steps against
    `imex_host_model.HostStepper` evaluating
    `linearised_convection_vec(V0 + th*(V1 - V0), w)` (1e-8, v in the M-norm
    and p),
 5. no stale graph: the weights alone, then the rows alone changed between
    `run` calls,
 6. `cnab` / `sbdftwo` with a `BaseTrajectory(interpolate=True)` stored every
    fourth step, forward over two slices, adjoint with a `time_map`, Heun start
    included, against the host loop; `ensemble_to_base(interpolate=True)` from
    an ensemble kept every fourth step, bit equal to an upload of the slots,
 7. every refusal by its message, the operator evaluating what it did before.

Largest error / bound measured on the MI355X (the report test prints them with
`pytest -s`): cell values forward 0.061, adjoint 0.078; `apply` forward 0.029,
adjoint 0.043 (of the counted bounds); against the host model, of 1e-8: weight
tables v 6.0e-13, p 2.0e-11; weights and rows changed between runs v 4.6e-13,
p 6.4e-11; the loops v 1.6e-11, p 1.7e-9.  61 tests, 32 s.
"""
import numpy as np
import pytest

import conv_lin_model as clm
import conv_model as cm
import imex_host_model as ihm
import scenarios
import test_gpu_conv_lin as tcl
import test_gpu_conv_traj as tct

pytestmark = pytest.mark.gpu

LD = cm.LD
VTOL, PTOL = tcl.VTOL, tcl.PTOL
MODES = tcl.MODES
MESHES = ['rect-1', 'rect-33', 'fan-40', 'rect-257']
NROWS = tct.NROWS
THETAS = [0.5, 0.25, 1./3, 2.0**-60, 1 - 2.0**-53]
WORST = {}
_cache = {}


def _note(path, r):
    WORST[path] = max(WORST.get(path, 0.0), r)
    return r


@pytest.fixture(scope='module')
def gtiu():
    from dolfin_navier_scipy_amd import time_int_utils, _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    return time_int_utils


@pytest.fixture(scope='module')
def wake(gtiu):
    return tcl.wake_setup()


def _lerp(v0, v1, th):
    """the NumPy statement: three separately rounded operations"""
    return v0 + th*(v1 - v0)


class LerpCase(tct.TrajCase):
    """`test_gpu_conv_traj.TrajCase` with rows free of -0.0 (`V_r + 0*d` turns
    a -0.0 into +0.0: the one value at which weight 0 is not the hold)"""

    def __init__(self, name):
        tct.TrajCase.__init__(self, name)
        assert NROWS == 5
        self.V, self.Vd = self.V + 0.0, self.Vd + 0.0
        assert not np.any(np.signbit(self.V) & (self.V == 0))
        assert not np.any(np.signbit(self.Vd) & (self.Vd == 0))

    def base_lerp(self, kind, r, th):
        p = min(r + 1, NROWS - 1)
        V0, D0 = self.base_of(kind, r)
        V1, D1 = self.base_of(kind, p)
        return _lerp(V0, V1, th), _lerp(D0, D1, th)

    def set_const_lerp(self, mode, kind, r, th):
        adj = mode == 'adjoint'
        base = self.base_lerp(kind, r, th)
        for cv in (self.k8, self.k1):
            cv.clear_base_flow()
            cv.set_dbcvals(self.wdbc(adj))
            cv.set_base_flow(base, adjoint=adj)
            assert cv.base_trajectory_rows == 0 and not cv.interpolates
        return base

    def model_lerp(self, mode, kind, r, th):
        key = ('lerp', mode, kind if self.ndbc else 'one', r, th)
        if key not in self._models:
            adj = mode == 'adjoint'
            V, Vd = self.base_lerp(kind, r, th)
            self._models[key] = clm.lin_model(self.sp, V, Vd, self.w,
                                              self.wdbc(adj), adj)
        return self._models[key]


def case(name):
    if name not in _cache:
        _cache[name] = LerpCase(name)
    return _cache[name]


def _arm(tv, r, th, table):
    """row `r` with weight `th` on a trajectory operator: as the host-named
    pair or as a table of one entry (outside a stepper: its first entry)"""
    if table:
        tv.set_base_rows([r, r], [th, th])
    else:
        tv.set_base_row(r, th)
    assert tv.interpolates == (table or th != 0.0)


# ---- 1. bit for bit -------------------------------------------------------------

@pytest.mark.parametrize('kind', ['rows', 'one'])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', MESHES)
def test_bits_of_the_numpy_interpolated_base(name, mode, kind):
    c = case(name)
    c.set_traj(mode, kind)
    nc = c.c.mesh.ncells
    rng = np.random.default_rng(nc)
    sels = [rng.permutation(nc)[:n].astype(np.int32)
            for n in sorted(set([1, max(1, nc//2), max(1, nc - 1)]))]
    fill = -3.5
    pairs = [(r, th) for r in range(NROWS - 1) for th in THETAS] \
        + [(r, 0.0) for r in range(NROWS)]
    for n, (r, th) in enumerate(pairs):
        base = c.set_const_lerp(mode, kind, r, th)
        if th == 0.0:
            assert np.array_equal(base[0], c.V[r])
        elif c.nv > 4 and th in (0.5, 0.25, 1./3):
            assert not np.array_equal(base[0], c.V[r])
            assert not np.array_equal(base[0], c.V[r + 1])
        for tv, kv in ((c.t8, c.k8), (c.t1, c.k1)):
            # (weight 0 through the interpolating instance: as a table)
            _arm(tv, r, th, table=(th == 0.0 or n % 2 == 1))
            want, _ = kv.cell_values(c.w)
            have, _ = tv.cell_values(c.w)
            assert np.array_equal(have, want), (r, th)
            assert np.array_equal(tv.apply(c.w, scale=-1.0),
                                  kv.apply(c.w, scale=-1.0)), (r, th)
            if th in (1./3, 0.0) and r in (1, NROWS - 1):
                for sel in sels:
                    a, _ = tv.cell_values(c.w, sel=sel, fill=fill)
                    b, _ = kv.cell_values(c.w, sel=sel, fill=fill)
                    assert np.array_equal(a, b)
                    rest = np.ones(nc, dtype=bool)
                    rest[sel] = False
                    assert np.all(a[:, rest] == fill)


def test_some_mesh_has_a_padded_leading_dimension():
    """(`ldv` is `nv` rounded up to 64: the partner row is `ldv` further on,
    not `nv`)"""
    assert any(case(n).nv % 64 for n in MESHES)
    assert any(case(n).nv > 64 for n in MESHES)


def test_full_vectors_and_the_setters_without_weights_take_them_off():
    from dolfin_navier_scipy_amd import convection
    c = case('fan-40')
    m = c.c.mesh
    full = np.zeros((NROWS, m.vdim))
    full[:, c.c.inv], full[:, c.c.dbc] = c.V, c.Vd
    cv = c.t8
    cv.clear_base_flow()
    cv.set_dbcvals(c.wd)
    cv.set_base_flow(convection.BaseTrajectory(np.arange(NROWS), full,
                                               interpolate=True))
    assert cv.base_trajectory_rows == NROWS and not cv.interpolates
    for rows, wts in (([3], [0.25]), ([2, 0, 3], [1./3, 0.5, 0.75]),
                      ([4, 1], [0.0, 0.5])):
        cv.set_base_rows(rows, wts)
        assert cv.interpolates and cv._base_info() == (NROWS, len(rows))
        c.set_const_lerp('forward', 'rows', rows[0], wts[0])
        assert np.array_equal(cv.apply(c.w), c.k8.apply(c.w))
    # the zero-order setters keep their meaning and take the weights off
    cv.set_base_rows([2, 0, 3])
    assert not cv.interpolates
    c.set_const('forward', 'rows', 2)
    assert np.array_equal(cv.apply(c.w), c.k8.apply(c.w))
    cv.set_base_row(1, 0.5)
    assert cv.interpolates and cv._base_info() == (NROWS, 0)
    cv.set_base_row(1)
    assert not cv.interpolates
    c.set_const('forward', 'rows', 1)
    assert np.array_equal(cv.apply(c.w), c.k8.apply(c.w))
    # a new base flow of any kind starts without weights
    cv.set_base_row(1, 0.5)
    cv.set_base_flow(c.traj('rows'))
    assert not cv.interpolates
    cv.set_base_row(1, 0.5)
    cv.set_base_flow(c.base_of('rows', 1))
    assert not cv.interpolates and cv.base_trajectory_rows == 0
    cv.clear_base_flow()
    assert not cv.interpolates


# ---- 2. against the long double model -------------------------------------------

@pytest.mark.parametrize('kind', ['rows', 'one'])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', MESHES)
def test_cells_and_apply_within_the_counted_bound(name, mode, kind):
    c = case(name)
    c.set_traj(mode, kind)
    worst_c = worst_a = 0.0
    for r, th in [(0, 0.5), (1, 0.25), (2, 1./3), (3, 0.5), (3, 1 - 2.0**-53),
                  (0, 2.0**-60), (NROWS - 1, 0.0)]:
        ref = c.model_lerp(mode, kind, r, th)
        got = None
        for tv in (c.t8, c.t1):
            _arm(tv, r, th, table=(th == 0.0))
            cells, pos = tv.cell_values(c.w)
            worst_c = max(worst_c, cm.ratio(cells[:, pos].T, *ref['cells']))
            val, bnd = ref['vec']
            for scale in (1.0, -0.37):
                got = tv.apply(c.w, scale=scale).reshape(-1)
                worst_a = max(worst_a, cm.ratio(got, LD(scale)*val,
                                                abs(LD(scale))*bnd))
        if th == 0.5 and c.nv > 4:
            # (the test can fail: the midpoint is outside the bound of either
            # end row)
            got = c.t8.apply(c.w).reshape(-1)
            for q in (r, r + 1):
                assert cm.ratio(got, *c.model(mode, kind, q)['vec']) > 1.0, \
                    (r, q)
    _note('cells ' + mode, worst_c)
    _note('apply ' + mode, worst_a)
    print('%s %s %s: cells %.3f apply %.3f' % (name, mode, kind, worst_c,
                                               worst_a))
    assert worst_c <= 1.0 and worst_a <= 1.0


# ---- 3. weight 0 is the hold ------------------------------------------------------

@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', MESHES)
def test_zero_weights_give_the_bits_of_the_hold(name, mode):
    c = case(name)
    c.set_traj(mode, 'rows')
    for r in range(NROWS):
        for tv in (c.t8, c.t1):
            tv.set_base_rows([r, (r + 1) % NROWS])
            assert not tv.interpolates
            want, app = tv.cell_values(c.w)[0], tv.apply(c.w)
            tv.set_base_rows([r, (r + 1) % NROWS], [0.0, 0.0])
            assert tv.interpolates
            assert np.array_equal(tv.cell_values(c.w)[0], want)
            assert np.array_equal(tv.apply(c.w), app)


def _wake_rows(wake, nrows, seed=11):
    return tct._wake_rows(wake, nrows, seed=seed) + 0.0


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_zero_weights_give_the_bits_of_the_held_run(gtiu, wake, scheme):
    w0 = tct._w0(wake)
    rows = _wake_rows(wake, 4)
    assert not np.any(np.signbit(rows) & (rows == 0))
    table = [k//3 for k in range(12)]
    la, lb = tcl.LinLoop(wake, scheme=scheme), tcl.LinLoop(wake, scheme=scheme)
    try:
        for lp, wts in ((la, None), (lb, np.zeros(12))):
            lp.cvop.set_base_flow(tct._traj_of(rows))
            lp.cvop.set_base_rows(table, wts)
            lp.start(w0)
            lp.stp.set_recorder(12, snap_slots='all')
            lp.stp.run(12, lp.cf, lp.opts)
        assert lb.cvop.interpolates and not la.cvop.interpolates
        for a, b in zip(la.stp.get_state(), lb.stp.get_state()):
            assert np.array_equal(a, b)
        va, vb = la.stp.record_snapshots()[0], lb.stp.record_snapshots()[0]
        assert np.array_equal(va, vb)
        # (the rows matter: the last state is not the one about row 0 alone)
        la.cvop.set_base_rows([0])
        la.start(w0)
        la.stp.set_recorder(12, snap_slots='all')
        la.stp.run(12, la.cf, la.opts)
        assert not np.array_equal(la.stp.get_state()[0], lb.stp.get_state()[0])
    finally:
        la.close()
        lb.close()


# ---- 4. index and weight tables in a stepper ------------------------------------

WROWS = tct.WROWS


class LerpRun(tct.TableRun):
    """`test_gpu_conv_traj.TableRun` with a weight beside every table entry:
    the host evaluates `-linearised_convection_vec(V0 + th*(V1 - V0), w)`"""

    weights = None

    def eval(self, v, row):
        s = min(row, len(self.table) - 1)
        k, th = self.table[s], self.weights[s]
        V = _lerp(self.rows[k], self.rows[min(k + 1, len(self.rows) - 1)], th)
        f = tcl._host_conv(self.wake, V, self.adj, self.adj)
        return f(tcl._full(self.wake, v, zero_dbc=self.adj))

    def arm(self, rows=None, table=None, weights=None):
        cv = self.lp.cvop
        if rows is not None:
            self.rows = rows
            cv.set_base_flow(tct._traj_of(rows), adjoint=self.adj)
            if table is None:               # (a new trajectory: arm it again)
                table, weights = self.table, self.weights
        if table is not None:
            self.table = list(table)
            self.weights = [0.0]*len(self.table) if weights is None \
                else list(weights)
            cv.set_base_rows(self.table, self.weights)
            assert cv.interpolates


def _walk(x0, dx, n=12):
    """positions `x0 + k dx` in units of the storage interval: rows, weights"""
    x = x0 + dx*np.arange(n)
    r = np.floor(x).astype(int)
    return r.tolist(), (x - r).tolist()


TABLES = dict(ascending=_walk(0.0, 0.75), descending=_walk(10.5, -0.75),
              clamped=([3, 7, 1], [0.5, 0.25, 1./3]))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_weight_tables_follow_the_host_model(gtiu, wake, scheme, mode):
    rows, w0 = _wake_rows(wake, WROWS), tct._w0(wake)
    tr = LerpRun(wake, scheme, mode)
    ends = {}
    try:
        tr.arm(rows=rows, table=[0])
        for name, (table, wts) in TABLES.items():
            assert max(table) < WROWS - 1 and 0 <= min(wts) and max(wts) < 1
            tr.arm(table=table, weights=wts)
            tr.start(w0)
            ev, ep = tr.run(12)
            print('%s %s %s: v %.2e p %.2e' % (scheme, mode, name, ev, ep))
            _note('table v ' + mode, ev/VTOL)
            _note('table p ' + mode, ep/PTOL)
            assert ev <= VTOL and ep <= PTOL
            ends[name] = tr.lp.stp.get_state()[0]
        # (not vacuous: held, the same tables end elsewhere)
        for name in ('ascending', 'clamped'):
            tr.lp.cvop.set_base_rows(TABLES[name][0])
            tr.start(w0)
            tr.lp.stp.set_recorder(12, snap_slots='all')
            tr.lp.stp.run(12, tr.lp.cf, tr.lp.opts)
            v0 = tr.lp.stp.get_state()[0]
            assert tcl._mnorm(tr.M, ends[name] - v0) \
                > 1e3*VTOL*tcl._mnorm(tr.M, v0), name
    finally:
        tr.close()


def test_a_new_weight_table_counts_from_the_step_that_follows(gtiu, wake):
    """no other table on the stepper, nothing else rewinds its counter: a new
    weight table is read from its first entry"""
    tr = LerpRun(wake, 'cnab', 'forward')
    try:
        tr.arm(rows=_wake_rows(wake, WROWS), table=[0])
        tr.start(tct._w0(wake))
        for table, wts in (_walk(0.0, 0.5, 6), _walk(10.75, -0.75, 6),
                           ([6, 2], [0.125, 0.875])):
            tr.arm(table=table, weights=wts)
            ev, ep = tr.run(6, record=False)
            print('table %s: v %.2e p %.2e' % (table, ev, ep))
            assert ev <= VTOL and ep <= PTOL, table
    finally:
        tr.close()


# ---- 5. no stale graph -------------------------------------------------------------

@pytest.mark.parametrize('mode', MODES)
def test_weights_then_rows_changed_between_runs(gtiu, wake, mode):
    """16 steps each: a pair of tables, other weights under the same rows,
    other rows under those weights, the first pair again -- every call against
    the host model"""
    rows = _wake_rows(wake, 8, seed=21)
    tab1, wts1 = _walk(0.0, 0.25, 16)
    wts2 = [0.75 - w for w in wts1]
    tab2 = [6 - r for r in tab1]
    tr = LerpRun(wake, 'cnab', mode)
    try:
        tr.arm(rows=rows, table=tab1, weights=wts1)
        tr.start(tct._w0(wake, 5))
        for what, kw in (('first', {}),
                         ('weights', dict(table=tab1, weights=wts2)),
                         ('rows', dict(table=tab2, weights=wts2)),
                         ('first again', dict(table=tab1, weights=wts1))):
            tr.arm(**kw)
            ev, ep = tr.run(16)
            print('%s, %s: v %.2e p %.2e' % (mode, what, ev, ep))
            _note('changed v ' + mode, ev/VTOL)
            _note('changed p ' + mode, ep/PTOL)
            assert ev <= VTOL and ep <= PTOL, what
        vh = tr.lp.host.get_state()[0]
        # (the changes matter: the first pair throughout ends elsewhere)
        tr.arm(table=tab1, weights=wts1)
        tr.start(tct._w0(wake, 5))
        for _ in range(4):
            tr.lp.stp.set_recorder(16, snap_slots='all')
            tr.lp.stp.run(16, tr.lp.cf, tr.lp.opts)
        assert tcl._mnorm(tr.M, tr.lp.stp.get_state()[0] - vh) \
            > 1e3*VTOL*tcl._mnorm(tr.M, vh)
    finally:
        tr.close()


# ---- 6. the loops -------------------------------------------------------------------

@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_loops_about_a_trajectory_stored_every_fourth_step(gtiu, wake, scheme,
                                                           mode):
    from dolfin_navier_scipy_amd import convection
    femp, M = wake['femp'], wake['M']
    th, inv, dbcinds, dbcvals = (femp['V'], femp['invinds'], femp['dbcinds'],
                                 femp['dbcvals'])
    adj = mode == 'adjoint'
    wdbc = np.zeros(dbcvals.size) if adj else dbcvals
    nts = 12
    rows = _wake_rows(wake, nts//4 + 1, seed=31)
    w0 = tct._w0(wake).reshape((-1, 1))

    def appnd(vvec, bcs):
        full = np.full((th.vdim, 1), np.nan)
        full[inv] = vvec
        full[dbcinds, 0] = wdbc
        return full
    trange = wake['make_kw'](None, nts=nts)['trange']
    T = trange[-1]
    traj = convection.BaseTrajectory(
        trange[::4], rows, time_map=(lambda t: T - t) if adj else None,
        interpolate=True)
    # the host loop evaluates f_vdp at the Heun start's three states and then
    # at the state every step starts from: the times in that order
    seq = [trange[0], trange[1], trange[1]] + list(trange[1:-1])
    calls = []

    def f_vdp(vfull):
        t = seq[len(calls)]
        r, wt = traj.weights_at([t])
        calls.append((int(r[0]), float(wt[0])))
        # (the NumPy statement: `linearised_convection_vec` about the vector
        # `flow_at` forms, V0 + th*(V1 - V0))
        V = traj.flow_at(t)
        assert np.array_equal(V, _lerp(rows[r[0]], rows[min(r[0] + 1, 3)],
                                       wt[0]))
        return tcl._host_conv(wake, V, adj, adj)(vfull)

    def kwargs(rec):
        kw = wake['make_kw'](rec, nts=nts)
        kw.update(inivel=w0, appndbcs=appnd, ntimeslices=2)
        return kw
    hrec = scenarios.Recorder()
    with pytest.MonkeyPatch.context() as mp:
        htiu = ihm.install(mp)
        hinteg = htiu.cnab if scheme == 'cnab' else htiu.sbdftwo
        kw = kwargs(hrec)
        kw['f_vdp'] = f_vdp
        vh, ph, ffh = hinteg(**kw)
    assert len(calls) == len(seq)
    want = [((nts - k)//4, ((nts - k) % 4)/4.) for k in range(1, nts)] if adj \
        else [(k//4, (k % 4)/4.) for k in range(1, nts)]
    assert [r for r, _ in calls[3:]] == [r for r, _ in want]
    for (_, got_w), (_, want_w) in zip(calls[3:], want):
        # (a stored time has weight exactly 0; the grid is a linspace)
        assert got_w == want_w if want_w == 0 else abs(got_w - want_w) < 1e-9
    cvop = convection.ConvectionP2.from_taylor_hood(th, inv, dbcinds, wdbc)
    grec = scenarios.Recorder()
    kw = kwargs(grec)
    kw.pop('f_vdp')
    try:
        cvop.set_base_flow(traj, adjoint=adj)
        integ = gtiu.cnab if scheme == 'cnab' else gtiu.sbdftwo
        vg, pg, ffg = integ(device_convection=cvop, invinds=inv,
                            resident=dict(record=True, savevp_times=None),
                            **kw)
        assert cvop.linearised == mode and cvop.interpolates
        assert cvop.base_trajectory_rows == nts//4 + 1
    finally:
        cvop.close()
    assert ffg == ffh == 0
    assert gtiu.LAST_RUN['record'] == 'device'
    tg, vgs, pgs = grec.arrays()
    thh, vhs, phs = hrec.arrays()
    assert tg.size == nts + 1 and np.array_equal(tg, thh)
    worst_v = worst_p = 0.0
    for k in range(tg.size):
        worst_v = max(worst_v, tcl._mnorm(M, vgs[k][inv] - vhs[k][inv])
                      / tcl._mnorm(M, vhs[k][inv]))
        if k >= 1:
            worst_p = max(worst_p, np.linalg.norm(pgs[k] - phs[k])
                          / np.linalg.norm(phs[k]))
    print('%s %s: worst v %.2e p %.2e' % (scheme, mode, worst_v, worst_p))
    _note('loop v ' + mode, worst_v/VTOL)
    _note('loop p ' + mode, worst_p/PTOL)
    assert worst_v <= VTOL and worst_p <= PTOL
    assert np.array_equal(vg[:, 0], vgs[-1][inv])
    assert np.array_equal(pg[:, 0], pgs[-1])


def test_ensemble_kept_every_fourth_step_becomes_an_interpolating_base(
        gtiu, wake):
    from dolfin_navier_scipy_amd import convection
    femp = wake['femp']
    th, inv, dbi, dbv = (femp['V'], femp['invinds'], femp['dbcinds'],
                         femp['dbcvals'])
    fwd = tcl.LinLoop(wake)                     # the nonlinear run
    cva = convection.ConvectionP2.from_taylor_hood(th, inv, dbi, dbv)
    cvu = convection.ConvectionP2.from_taylor_hood(th, inv, dbi, dbv)
    cvk = convection.ConvectionP2.from_taylor_hood(th, inv, dbi, dbv)
    try:
        fwd.start(wake['inivel'][:, 0])
        slots = [k//4 if k % 4 == 3 else -1 for k in range(12)]   # every=4
        fwd.stp.set_ensemble(slots, nslots=3)
        fwd.stp.run(12, fwd.cf, fwd.opts)
        E = fwd.stp.ensemble()
        assert E.shape == (3, inv.size)
        assert np.linalg.norm(E[2] - E[0]) > 1e-6*np.linalg.norm(E[0])
        times = 4*fwd.dt*np.arange(1, 4)
        w = tct._w0(wake, 9)
        fwd.stp.ensemble_to_base(cva, times=times, dbcvals=dbv,
                                 interpolate=True)
        assert cva.base_trajectory.interpolate and cva.base_trajectory_rows == 3
        assert not cva.interpolates               # (until weights are armed)
        cvu.set_base_flow(convection.BaseTrajectory(times, E, dbv,
                                                    interpolate=True))
        for k in range(4, 13):
            t = k*fwd.dt
            r, wt = cva.base_trajectory.weights_at([t])
            assert (int(r[0]), float(wt[0])) == (k//4 - 1, (k % 4)/4.)
            # armed the way the loops arm it
            gtiu._arm_base_row(cva, cva.base_trajectory, t)
            gtiu._arm_base_rows(cvu, cvu.base_trajectory, [t, t])
            assert cva.interpolates == (k % 4 != 0) and cvu.interpolates
            cvk.set_base_flow((_lerp(E[r[0]], E[min(r[0] + 1, 2)], wt[0]),
                               dbv))
            want = cvk.apply(w)
            assert np.array_equal(cva.apply(w), want), k
            assert np.array_equal(cvu.apply(w), want), k
        # without the flag the trajectory the loops see is held
        fwd.stp.ensemble_to_base(cva, times=times, dbcvals=dbv)
        assert not cva.base_trajectory.interpolate
    finally:
        fwd.close()
        cva.close()
        cvu.close()
        cvk.close()


# ---- 7. refusals --------------------------------------------------------------------

def _state(cv):
    return (cv.linearised, cv._base_info(), cv.interpolates)


def test_refusals_of_the_operator(gtiu):
    c = case('rect-33')
    cv = c.t8
    c.set_traj('forward', 'rows')
    cv.set_base_rows([3, 2, 1], [0.5, 0.25, 0.0])
    before, want = _state(cv), cv.apply(c.w)
    assert before == ('forward', (NROWS, 3), True)

    def same():
        assert _state(cv) == before
        assert np.array_equal(cv.apply(c.w), want)
    try:
        # weights outside [0, 1) or not finite
        for bad, word in (([0.5, 1.0], 'entry 1 has the interpolation weight 1'),
                          ([-0.25, 0.5], 'entry 0 has the interpolation '
                           'weight -0.25'),
                          ([0.5, np.nan], 'entry 1 has'),
                          ([np.inf, 0.5], 'entry 0 has'),
                          ([0.0, 1.0 + 2.0**-52], 'entry 1 has')):
            tcl._refused(lambda: cv.set_base_rows([0, 1], bad), 'base rows',
                         word, 'outside [0, 1)')
            same()
        for bad in (1.0, -0.5, np.nan, -np.inf, 7.0):
            tcl._refused(lambda: cv.set_base_row(1, bad),
                         'base row 1 has the interpolation weight',
                         'outside [0, 1)')
            same()
        # a non-zero weight on the last row
        tcl._refused(lambda: cv.set_base_rows([0, NROWS - 1, 1],
                                              [0.5, 2.0**-60, 0.5]),
                     'base rows: entry 1:', 'on row %d, the last of the %d '
                     'rows' % (NROWS - 1, NROWS))
        same()
        tcl._refused(lambda: cv.set_base_row(NROWS - 1, 0.5),
                     'base row %d:' % (NROWS - 1), 'the last of the')
        same()
        # the rows themselves, as without weights
        tcl._refused(lambda: cv.set_base_rows([0, NROWS], [0.5, 0.0]),
                     'entry 1 is %d' % NROWS, 'outside 0..%d' % (NROWS - 1))
        tcl._refused(lambda: cv.set_base_row(NROWS, 0.5),
                     'base row %d' % NROWS)
        tcl._refused(lambda: cv.set_base_rows([], []), 'a table of 0 entries')
        same()
        # weights of another length than the rows
        for rows, wts in (([0, 1], [0.5]), ([0], [0.5, 0.5]), ([0, 1], [])):
            with pytest.raises(ValueError) as exc:
                cv.set_base_rows(rows, wts)
            assert '%d interpolation weights for %d base rows' % (
                len(wts), len(rows)) in str(exc.value)
            same()
        # weights without a trajectory
        k = c.k8
        c.set_const('forward', 'rows', 0)
        kwant = k.apply(c.w)
        tcl._refused(lambda: k.set_base_rows([0], [0.0]),
                     'without a base trajectory')
        tcl._refused(lambda: k.set_base_row(0, 0.5),
                     'without a base trajectory')
        assert _state(k) == ('forward', (0, 0), False)
        assert np.array_equal(k.apply(c.w), kwant)
        k.clear_base_flow()
        tcl._refused(lambda: k.set_base_rows([0], [0.5]),
                     'without a base trajectory')
        # the adjoint with non-zero values of the perturbation, with a table:
        # refused as it was, whatever the trajectory's flag
        from dolfin_navier_scipy_amd import convection
        lerp = convection.BaseTrajectory(0.25*np.arange(NROWS), c.V, c.Vd,
                                         interpolate=True)
        tcl._refused(lambda: cv.set_base_flow(lerp, adjoint=True),
                     'linearised convection, adjoint mode', 'Dirichlet value')
        same()
        cv.set_dbc_table(np.tile(c.wd, (3, 1)))
        tcl._refused(lambda: cv.set_base_flow(lerp, adjoint=True),
                     'adjoint mode', 'dns_conv_set_dbc_table')
        assert _state(cv) == before
        cv.set_dbcvals(c.wd)
        same()
        # the entry points that form the nonlinear matrices and tensors
        cv.bind_pattern(cv.connectivity())
        tcl._refused(lambda: cv.assemble(c.w), 'linearised convection '
                     'operator', 'dns_conv_assemble')
        tcl._refused(lambda: cv.project_tensor(
            np.ones((2, c.nv + c.nv % 2))), 'dns_conv_project_tensor')
        same()
    finally:
        cv.clear_base_flow()
        cv.set_dbcvals(c.wd)


def test_refusals_of_the_loop(gtiu, wake):
    """a loop time behind the last stored time (no hold when interpolating)
    and `rom`: `ValueError` by name before anything is armed"""
    from dolfin_navier_scipy_amd import convection
    femp = wake['femp']
    cvop = convection.ConvectionP2.from_taylor_hood(
        femp['V'], femp['invinds'], femp['dbcinds'], femp['dbcvals'])
    kw = wake['make_kw'](scenarios.Recorder(), nts=8)
    kw.pop('f_vdp')
    trange = kw['trange']
    rows = _wake_rows(wake, 3)

    def traj(times, **kwt):
        return convection.BaseTrajectory(times, rows, interpolate=True, **kwt)
    try:
        T = trange[-1]
        for tr, word, t_bad in (
                (traj(trange[0:5:2]), 'behind the last stored time',
                 trange[5]),
                (traj(trange[2:7:2]), 'before the first stored time',
                 trange[0]),
                (traj(trange[0:5:2], time_map=lambda t: T - t),
                 'behind the last stored time', trange[0])):
            cvop.set_base_flow(tr)
            cvop.set_base_row(1, 0.5)
            state, want = _state(cvop), cvop.apply(tct._w0(wake))
            with pytest.raises(ValueError) as exc:
                gtiu.cnab(device_convection=cvop, invinds=femp['invinds'],
                          resident=dict(record=True), **kw)
            assert 'base trajectory: time {0!r}'.format(float(t_bad)) \
                in str(exc.value)
            assert word in str(exc.value)
            assert _state(cvop) == state
            assert np.array_equal(cvop.apply(tct._w0(wake)), want)
        # (held, the first of them is covered: one interval behind the last)
        convection.BaseTrajectory(trange[0:5:2], rows).rows_at(trange[:6])
        cvop.set_base_flow(traj(trange[::4]))
        with pytest.raises(ValueError) as exc:
            gtiu.cnab(device_convection=cvop, invinds=femp['invinds'],
                      resident=dict(pod=object(), rom=object()), **kw)
        assert 'linearised convection operator' in str(exc.value)
        assert '`rom`' in str(exc.value)
        assert cvop.base_trajectory_rows == 3
    finally:
        cvop.close()


def test_refusals_of_the_steppers(gtiu, toy_prob):
    """the trapezoidal stepper and a row-partitioned stepper refuse the
    operator with weights armed as they refuse it without"""
    from dolfin_navier_scipy_amd import (saddle, convection, comm as dcomm,
                                         newton_picard as dnp)
    M, A, J = (toy_prob['smc'][k] for k in 'MAJ')
    dt = 5e-3
    cvop = convection.ConvectionP2.from_taylor_hood(
        toy_prob['th'], toy_prob['invinds'], toy_prob['dbcinds'],
        toy_prob['dbcvals'])
    rows = np.zeros((2, toy_prob['th'].vdim))
    rows[:, toy_prob['dbcinds']] = toy_prob['dbcvals']
    traj = convection.BaseTrajectory(np.arange(2), rows, interpolate=True)
    cvop.set_base_flow(traj)
    cvop.set_base_row(0, 0.5)
    tcl._refused(lambda: dnp.TrapezoidalStepper(M, A, J, cvop, 4, dt,
                                                precond=False),
                 'linearised convection operator', 'the trapezoidal stepper')
    cmm = dcomm.Comm.rccl(0, 1, 0, dcomm.rccl_unique_id())
    system = saddle.SaddleSystem((M + .5*dt*A).tocsr(), J)
    stp = None
    try:
        system.set_comm(cmm)
        system.setup_precond(cheb_degree=6, schur='dense', fhat='explicit')
        stp = saddle.ImexStepper(system, (M - .5*dt*A).tocsr())
        tcl._refused(lambda: stp.set_convection(cvop, scale=-1.0),
                     'linearised convection operator on a row-partitioned '
                     'stepper', 'N(v)v')
        cvop.clear_base_flow()
        stp.set_convection(cvop, scale=-1.0)
        cvop.set_base_flow(traj)
        cvop.set_base_rows([1, 0], [0.0, 0.5])
        stp.set_state(np.zeros(J.shape[1]))
        cf = saddle.ImexStepper.coeffs(a_c=1., cn_c=1.5*dt, cn_o=-.5*dt,
                                       pscale=-1./dt, extrapolate=4)
        tcl._refused(lambda: stp.run(1, cf, saddle.solve_opts(method='gmres')),
                     'linearised convection operator on a row-partitioned '
                     'stepper')
        assert _state(cvop) == ('forward', (2, 2), True)
    finally:
        if stp is not None:
            stp.set_convection(None)
            stp.close()
        system.set_comm(None)
        system.close()
        cmm.close()
        cvop.close()


def test_functionals_with_cells_are_refused(gtiu, wake):
    from dolfin_navier_scipy_amd import fem
    femp = wake['femp']
    fn = fem.boundary_forces(femp['V'], femp)
    assert fn.cells[0].size > 0
    lp = tcl.LinLoop(wake)
    try:
        lp.start(0.1*wake['inivel'][:, 0])
        lp.stp.set_functionals(fn, 8, lp.dt)
        lp.stp.run(1, lp.cf, lp.opts)
        lp.cvop.set_base_flow(tct._traj_of(_wake_rows(wake, 2)))
        lp.cvop.set_base_rows([1, 0], [0.0, 0.5])
        for go in (lambda: lp.stp.run(1, lp.cf, lp.opts),
                   lambda: lp.stp.step(lp.cf, opts=lp.opts)):
            tcl._refused(go, 'linearised convection operator with '
                         'functionals with cells')
        assert _state(lp.cvop) == ('forward', (2, 2), True)
        lp.cvop.clear_base_flow()
        lp.stp.run(1, lp.cf, lp.opts)
    finally:
        lp.close()


# ---- 8. report ----------------------------------------------------------------------

def test_zz_report_and_close():
    """prints the largest error / bound per path (the module's docstring holds
    the figures measured on the MI355X)"""
    print('largest error / bound per path: '
          + '  '.join('%s %.3g' % kv for kv in sorted(WORST.items())))
    for c in _cache.values():
        c.close()
    _cache.clear()
