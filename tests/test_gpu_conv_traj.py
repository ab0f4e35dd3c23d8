"""Linearised and adjoint convection about a TIME-VARYING base flow on the
device: `ConvectionP2.set_base_flow(BaseTrajectory)`, `set_base_rows`,
`set_base_row`, `ImexStepper.ensemble_to_base` (the trajectory instances of
`k_conv_lin_cells<ADJ>` and `k_conv_lin_cells_lane<ADJ>`):

 1. cell values and `apply` about every row of a trajectory of five rows
    (Dirichlet values per row and as one set), both modes, both element
    kernels, PER ENTRY against `conv_lin_model.lin_model` of that row within
    its counted bound -- zero-order hold adds no rounding, the count is the one
    of the constant base; the two kernels bit equal; a row is outside the
    bound of any other row,
 2. bit for bit what an operator with `set_base_flow((V_r, Vd_r))` gives, with
    `sel` lists, with one row, with a padded leading dimension,
 3. the per-step index table in a stepper on the N=2 wake: all rows equal
    gives the bits of the constant-base run; ascending, descending, repeated
    and clamped tables, `cnab` and `sbdf2`, both modes, 12 steps against
    `imex_host_model.HostStepper` (1e-8, v in the M-norm and p),
 4. no stale graph: the index table, then the trajectory changed between
    `run` calls,
 5. the device-to-device adoption of ensemble slots, bit equal to an upload of
    the downloaded slots, and an adjoint run backwards over them,
 6. `cnab` / `sbdftwo` with a `BaseTrajectory` stored every second step, with
    a `time_map` in the adjoint case, over slices, Heun start included, against
    the host loop,
 7. every refusal by its message, the operator left as it was.

Largest error / bound measured on the MI355X (the report test prints them with
`pytest -s`): cell values forward 0.061, adjoint 0.078; `apply` forward 0.034,
adjoint 0.041 (of the counted bounds); against the host model, of 1e-8: index
tables v 6.7e-13, p 4.1e-11; table and trajectory changed between runs v
4.5e-13, p 3.2e-11; the adjoint run over the adopted slots v 2.9e-13, p
2.3e-12; the loops v 1.5e-11, p 1.0e-9.  72 tests, 34 s.
"""
import os
import types

import numpy as np
import pytest

import conv_lin_model as clm
import conv_model as cm
import imex_host_model as ihm
import scenarios
import test_gpu_conv_lin as tcl

pytestmark = pytest.mark.gpu

LD = cm.LD
VTOL, PTOL = tcl.VTOL, tcl.PTOL
MODES = tcl.MODES
MESHES = ['rect-1', 'rect-33', 'rect-33-nobc', 'fan-40', 'rect-257',
          'rect-1000']
NROWS = 5
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


class TrajCase(object):
    """mesh, space and perturbation of `test_gpu_conv_lin.Case`; `t8` / `t1`:
    the eight-lane and the one-lane operator that get the trajectory, `k8` /
    `k1`: the two that get one row as a constant base flow.  `V (m, nv)`,
    `Vd (m, ndbc)`: the rows"""

    def __init__(self, name):
        c = self.c = tcl.Case(name)
        self.t8, self.t1, self.k8 = c.cv8, c.cv1, c.cv0
        old = os.environ.get('DNS_CONV_LANE_MIN')
        os.environ['DNS_CONV_LANE_MIN'] = '1'
        try:
            from dolfin_navier_scipy_amd import convection
            m = c.mesh
            self.k1 = convection.ConvectionP2(m.cell_vdofs, m.glam, m.area,
                                              m.vdim, c.inv, c.dbc, c.wd)
        finally:
            if old is None:
                del os.environ['DNS_CONV_LANE_MIN']
            else:
                os.environ['DNS_CONV_LANE_MIN'] = old
        rng = np.random.default_rng(500 + c.mesh.ncells)
        self.V = tcl._grid(rng, (NROWS, c.inv.size))
        self.Vd = tcl._grid(rng, (NROWS, c.dbc.size))
        self.sp, self.w, self.wd = c.sp, c.w, c.wd
        self.nv, self.ndbc = c.inv.size, c.dbc.size
        self._models = {}

    def wdbc(self, adj):
        return np.zeros(self.ndbc) if adj else self.wd

    def traj(self, kind, rows=None):
        """`kind`: 'rows' -- Dirichlet values per row --, 'one' -- row 0's for
        every row"""
        from dolfin_navier_scipy_amd import convection
        rows = np.arange(NROWS) if rows is None else np.asarray(rows)
        return convection.BaseTrajectory(
            0.25*np.arange(rows.size), self.V[rows],
            self.Vd[rows] if kind == 'rows' else self.Vd[0])

    def base_of(self, kind, r):
        return self.V[r], self.Vd[r if kind == 'rows' else 0]

    def set_traj(self, mode, kind, rows=None):
        adj = mode == 'adjoint'
        for cv in (self.t8, self.t1):
            cv.clear_base_flow()
            cv.set_dbcvals(self.wdbc(adj))
            cv.set_base_flow(self.traj(kind, rows), adjoint=adj)
            assert cv.linearised == mode
            assert cv.base_trajectory_rows == (NROWS if rows is None
                                               else len(rows))
        return adj

    def set_const(self, mode, kind, r):
        adj = mode == 'adjoint'
        for cv in (self.k8, self.k1):
            cv.clear_base_flow()
            cv.set_dbcvals(self.wdbc(adj))
            cv.set_base_flow(self.base_of(kind, r), adjoint=adj)
            assert cv.base_trajectory_rows == 0

    def model(self, mode, kind, r):
        key = (mode, kind if self.ndbc else 'one', r)
        if key not in self._models:
            adj = mode == 'adjoint'
            V, Vd = self.base_of(kind, r)
            self._models[key] = clm.lin_model(self.sp, V, Vd, self.w,
                                              self.wdbc(adj), adj)
        return self._models[key]

    def close(self):
        self.k1.close()
        self.c.close()


def case(name):
    if name not in _cache:
        _cache[name] = TrajCase(name)
    return _cache[name]


# ---- 1. cells and apply per row against the model -----------------------------

@pytest.mark.parametrize('kind', ['rows', 'one'])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', MESHES)
def test_cells_and_apply_about_every_row(name, mode, kind):
    c = case(name)
    c.set_traj(mode, kind)
    worst_c = worst_a = 0.0
    got = {}
    for r in range(NROWS):
        for cv in (c.t8, c.t1):
            cv.set_base_row(r)
        ref = c.model(mode, kind, r)
        cells8, pos8 = c.t8.cell_values(c.w)
        cells1, pos1 = c.t1.cell_values(c.w)
        assert np.array_equal(pos8, pos1)
        assert np.array_equal(cells8, cells1)            # bit for bit
        worst_c = max(worst_c, cm.ratio(cells8[:, pos8].T, *ref['cells']))
        val, bnd = ref['vec']
        for scale in (1.0, -0.37):
            got8 = c.t8.apply(c.w, scale=scale).reshape(-1)
            got1 = c.t1.apply(c.w, scale=scale).reshape(-1)
            assert np.array_equal(got8, got1)
            worst_a = max(worst_a, cm.ratio(got8, LD(scale)*val,
                                            abs(LD(scale))*bnd))
            if scale == 1.0:
                got[r] = got8
    _note('cells ' + mode, worst_c)
    _note('apply ' + mode, worst_a)
    print('%s %s %s: cells %.3f apply %.3f' % (name, mode, kind, worst_c,
                                               worst_a))
    assert worst_c <= 1.0 and worst_a <= 1.0
    if c.nv > 4:
        # (not vacuous: row r is not within the bound of any other row)
        for r in range(NROWS):
            for q in range(NROWS):
                if q != r:
                    assert cm.ratio(got[r], *c.model(mode, kind, q)['vec']) \
                        > 1.0, (r, q)


# ---- 2. bit for bit the constant base -----------------------------------------

@pytest.mark.parametrize('kind', ['rows', 'one'])
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', MESHES)
def test_every_row_gives_the_bits_of_the_constant_base(name, mode, kind):
    c = case(name)
    c.set_traj(mode, kind)
    nc = c.c.mesh.ncells
    rng = np.random.default_rng(nc)
    sels = [rng.permutation(nc)[:n].astype(np.int32)
            for n in sorted(set([1, max(1, nc//2), max(1, nc - 1)]))]
    fill = -3.5
    for r in range(NROWS):
        c.set_const(mode, kind, r)
        for tv, kv in ((c.t8, c.k8), (c.t1, c.k1)):
            tv.set_base_row(r)
            want, _ = kv.cell_values(c.w)
            have, _ = tv.cell_values(c.w)
            assert np.array_equal(have, want)
            assert np.array_equal(tv.apply(c.w, scale=-1.0),
                                  kv.apply(c.w, scale=-1.0))
            for sel in sels:
                a, _ = tv.cell_values(c.w, sel=sel, fill=fill)
                b, _ = kv.cell_values(c.w, sel=sel, fill=fill)
                assert np.array_equal(a, b)
                rest = np.ones(nc, dtype=bool)
                rest[sel] = False
                assert np.all(a[:, rest] == fill)
    # (the constant operators have a base flow of their own kind)
    assert c.k8.linearised == mode and c.k8.base_trajectory_rows == 0


def test_some_mesh_has_a_padded_leading_dimension():
    """(`ldv` is `nv` rounded up to 64: the meshes above must not all fit)"""
    assert any(case(n).nv % 64 for n in MESHES)
    assert any(case(n).nv > 64 for n in MESHES)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['rect-33', 'rect-1000'])
def test_a_trajectory_of_one_row(name, mode):
    c = case(name)
    for r in (0, NROWS - 1):
        c.set_traj(mode, 'rows', rows=[r])
        c.set_const(mode, 'rows', r)
        for tv, kv in ((c.t8, c.k8), (c.t1, c.k1)):
            assert np.array_equal(tv.apply(c.w), kv.apply(c.w))
            tv.set_base_rows([0, 0, 0])
            assert np.array_equal(tv.cell_values(c.w)[0],
                                  kv.cell_values(c.w)[0])


def test_full_vectors_and_the_index_table_outside_a_stepper():
    """`v_rows` as full velocity vectors; outside a stepper an index table
    evaluates about its first entry; `set_base_flow` of a constant base and
    `clear_base_flow` release the trajectory"""
    from dolfin_navier_scipy_amd import convection
    c = case('fan-40')
    m = c.c.mesh
    full = np.zeros((NROWS, m.vdim))
    full[:, c.c.inv], full[:, c.c.dbc] = c.V, c.Vd
    cv = c.t8
    cv.clear_base_flow()
    cv.set_dbcvals(c.wd)
    cv.set_base_flow(convection.BaseTrajectory(np.arange(NROWS), full))
    assert cv.base_trajectory_rows == NROWS and cv.linearised == 'forward'
    for rows in ([3], [2, 0, 4], [4, 4]):
        cv.set_base_rows(rows)
        c.set_const('forward', 'rows', rows[0])
        assert np.array_equal(cv.apply(c.w), c.k8.apply(c.w))
    cv.set_base_flow(c.base_of('rows', 1))
    assert cv.base_trajectory_rows == 0 and cv.base_trajectory is None
    c.set_const('forward', 'rows', 1)
    assert np.array_equal(cv.apply(c.w), c.k8.apply(c.w))
    cv.set_base_flow(c.traj('rows'))
    cv.clear_base_flow()
    assert cv.base_trajectory_rows == 0 and cv.linearised is False


# ---- 3. the index table in a stepper --------------------------------------------

WROWS = 12


def _wake_rows(wake, nrows=WROWS, seed=11):
    """`nrows` distinct base flows on the N=2 wake, as full vectors (their
    Dirichlet values differ from row to row)"""
    femp = wake['femp']
    rng = np.random.default_rng(seed)
    v0 = wake['inivel'][:, 0]
    rows = np.zeros((nrows, femp['V'].vdim))
    for k in range(nrows):
        a = 0.5 + 0.5*np.cos(0.7*k)
        rows[k, femp['invinds']] = a*v0 + 2e-2*rng.standard_normal(v0.size)
        rows[k, femp['dbcinds']] = (0.8 + 0.04*k)*femp['dbcvals']
    return rows


def _traj_of(rows, times=None, time_map=None):
    from dolfin_navier_scipy_amd import convection
    return convection.BaseTrajectory(
        np.arange(rows.shape[0]) if times is None else times, rows,
        time_map=time_map)


def _w0(wake, seed=3):
    rng = np.random.default_rng(seed)
    return 0.1*wake['inivel'][:, 0] \
        + 1e-3*rng.standard_normal(wake['inivel'].shape[0])


class TableRun(object):
    """a `LinLoop` with its host model, the host evaluating
    `-linearised_convection_vec(V[table[min(step, len - 1)]], w)`"""

    def __init__(self, wake, scheme, mode):
        self.wake, self.adj = wake, mode == 'adjoint'
        self.lp = tcl.LinLoop(wake, scheme=scheme, zero_dbc=self.adj,
                              make_host=True)
        self.rows = self.table = None
        self.lp.host.set_convection(types.SimpleNamespace(eval=self.eval))
        self.M = wake['M']

    def eval(self, v, row):
        k = self.table[min(row, len(self.table) - 1)]
        f = tcl._host_conv(self.wake, self.rows[k], self.adj, self.adj)
        return f(tcl._full(self.wake, v, zero_dbc=self.adj))

    def arm(self, rows=None, table=None):
        cv = self.lp.cvop
        if rows is not None:
            self.rows = rows
            cv.set_base_flow(_traj_of(rows), adjoint=self.adj)
        if table is not None:
            self.table = list(table)
            cv.set_base_rows(self.table)

    def start(self, w0):
        # (`apply` outside the stepper: about the table's first row, which is
        # the row of the state both histories start from)
        self.lp.start(w0)

    def run(self, n, record=True):
        """`n` steps on both; returns the errors v (M-norm), p"""
        lp = self.lp
        if record:
            lp.stp.set_recorder(n, snap_slots='all')   # (rewinds the counter)
        lp.host.set_rhs_table(np.tile(np.ravel(lp.g), (n, 1)),
                              np.tile(np.ravel(lp.gp), (n, 1)))
        lp.stp.run(n, lp.cf, lp.opts)
        lp.host.run(n, lp.hcf)
        vg, pg = lp.stp.get_state()
        vh, ph = lp.host.get_state()
        if record:
            vs, ps = lp.stp.record_snapshots()
            assert np.array_equal(vs[-1], vg[:, 0])
            assert np.array_equal(ps[-1], pg[:, 0])
        return (tcl._mnorm(self.M, vg - vh)/tcl._mnorm(self.M, vh),
                np.linalg.norm(pg - ph)/np.linalg.norm(ph))

    def close(self):
        self.lp.close()


def test_equal_rows_give_the_bits_of_the_constant_base_run(gtiu, wake):
    w0 = _w0(wake)
    rows = np.tile(_wake_rows(wake, 1), (4, 1))
    la, lb = tcl.LinLoop(wake), tcl.LinLoop(wake)
    try:
        la.cvop.set_base_flow(rows[0])
        la.start(w0)
        la.stp.set_recorder(8, snap_slots='all')
        la.stp.run(8, la.cf, la.opts)
        lb.cvop.set_base_flow(_traj_of(rows))
        lb.cvop.set_base_rows([0, 1, 2, 3, 2, 1, 0, 3])
        lb.start(w0)
        lb.stp.set_recorder(8, snap_slots='all')
        lb.stp.run(8, lb.cf, lb.opts)
        for a, b in zip(la.stp.get_state(), lb.stp.get_state()):
            assert np.array_equal(a, b)
        assert la.cvop.base_trajectory_rows == 0
        assert lb.cvop.base_trajectory_rows == 4
    finally:
        la.close()
        lb.close()


TABLES = dict(ascending=list(range(WROWS)),
              descending=list(range(WROWS - 1, -1, -1)),
              repeats=[k//2 for k in range(WROWS)],
              clamped=[3, 7, 1])


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_index_tables_follow_the_host_model(gtiu, wake, scheme, mode):
    rows, w0 = _wake_rows(wake), _w0(wake)
    tr = TableRun(wake, scheme, mode)
    ends = {}
    try:
        tr.arm(rows=rows)
        for name, table in TABLES.items():
            tr.arm(table=table)
            tr.start(w0)
            ev, ep = tr.run(12)
            print('%s %s %s: v %.2e p %.2e' % (scheme, mode, name, ev, ep))
            _note('table v ' + mode, ev/VTOL)
            _note('table p ' + mode, ep/PTOL)
            assert ev <= VTOL and ep <= PTOL
            ends[name] = tr.lp.stp.get_state()[0]
        # (not vacuous: about row 0 alone the state is elsewhere)
        tr.arm(table=[0])
        tr.start(w0)
        tr.lp.stp.set_recorder(12, snap_slots='all')
        tr.lp.stp.run(12, tr.lp.cf, tr.lp.opts)
        v0 = tr.lp.stp.get_state()[0]
        for name in ('ascending', 'repeats'):
            assert tcl._mnorm(tr.M, ends[name] - v0) \
                > 1e3*VTOL*tcl._mnorm(tr.M, v0), name
    finally:
        tr.close()


def test_a_new_table_counts_from_the_step_that_follows(gtiu, wake):
    """no other table on the stepper, nothing else rewinds its counter: the
    second table is read from its first entry, not from entry 6"""
    tr = TableRun(wake, 'cnab', 'forward')
    try:
        tr.arm(rows=_wake_rows(wake), table=[0, 1, 2, 3, 4, 5])
        tr.start(_w0(wake))
        for table in ([0, 1, 2, 3, 4, 5], [11, 10, 9, 8, 7, 6], [6, 2]):
            tr.arm(table=table)
            ev, ep = tr.run(6, record=False)
            print('table %s: v %.2e p %.2e' % (table, ev, ep))
            assert ev <= VTOL and ep <= PTOL, table
    finally:
        tr.close()


# ---- 4. no stale graph ------------------------------------------------------------

@pytest.mark.parametrize('mode', MODES)
def test_table_then_trajectory_changed_between_runs(gtiu, wake, mode):
    """16 steps each: a table, another table, another trajectory under that
    table, the first pair again -- every call against the host model"""
    rows1 = _wake_rows(wake, 8, seed=21)
    rows2 = _wake_rows(wake, 8, seed=22)[::-1].copy()
    tab1 = [k//2 for k in range(16)]
    tab2 = [7 - k//2 for k in range(16)]
    tr = TableRun(wake, 'cnab', mode)
    try:
        tr.arm(rows=rows1, table=tab1)
        tr.start(_w0(wake, 5))
        for what, kw in (('first', {}), ('table', dict(table=tab2)),
                         ('trajectory', dict(rows=rows2, table=tab2)),
                         ('first again', dict(rows=rows1, table=tab1))):
            tr.arm(**kw)
            ev, ep = tr.run(16)
            print('%s, %s: v %.2e p %.2e' % (mode, what, ev, ep))
            _note('changed v ' + mode, ev/VTOL)
            _note('changed p ' + mode, ep/PTOL)
            assert ev <= VTOL and ep <= PTOL, what
        vh = tr.lp.host.get_state()[0]
        # (the changes matter: the first pair throughout ends elsewhere)
        tr.arm(rows=rows1, table=tab1)
        tr.start(_w0(wake, 5))
        for _ in range(4):
            tr.lp.stp.set_recorder(16, snap_slots='all')
            tr.lp.stp.run(16, tr.lp.cf, tr.lp.opts)
        assert tcl._mnorm(tr.M, tr.lp.stp.get_state()[0] - vh) \
            > 1e3*VTOL*tcl._mnorm(tr.M, vh)
    finally:
        tr.close()


# ---- 5. adoption from the ensemble, device to device ---------------------------

def test_ensemble_slots_become_the_base_trajectory(gtiu, wake):
    from dolfin_navier_scipy_amd import convection
    femp = wake['femp']
    th, inv, dbi, dbv = (femp['V'], femp['invinds'], femp['dbcinds'],
                         femp['dbcvals'])
    fwd = tcl.LinLoop(wake)                     # the nonlinear run
    cva = convection.ConvectionP2.from_taylor_hood(th, inv, dbi, dbv)
    cvk = convection.ConvectionP2.from_taylor_hood(th, inv, dbi, dbv)
    tr = None
    try:
        fwd.start(wake['inivel'][:, 0])
        slots = [k//2 if k % 2 else -1 for k in range(12)]
        fwd.stp.set_ensemble(slots, nslots=6)
        fwd.stp.run(12, fwd.cf, fwd.opts)
        E = fwd.stp.ensemble()
        assert E.shape == (6, inv.size)
        assert np.linalg.norm(E[5] - E[0]) > 1e-6*np.linalg.norm(E[0])
        w = _w0(wake, 9)
        fwd.stp.ensemble_to_base(cva, dbcvals=dbv)
        assert cva.base_trajectory_rows == 6 and cva.linearised == 'forward'
        for r in range(6):
            cva.set_base_row(r)
            cvk.set_base_flow((E[r], dbv))
            assert np.array_equal(cva.apply(w), cvk.apply(w)), r
        # a part of the slots
        fwd.stp.ensemble_to_base(cva, first=2, count=3, dbcvals=dbv)
        assert cva.base_trajectory_rows == 3
        cva.set_base_row(2)
        cvk.set_base_flow((E[4], dbv))
        assert np.array_equal(cva.apply(w), cvk.apply(w))
        # the adjoint run backwards over the slots, two steps a slot
        tr = TableRun(wake, 'cnab', 'adjoint')
        fwd.stp.ensemble_to_base(tr.lp.cvop, dbcvals=dbv, adjoint=True)
        assert tr.lp.cvop.linearised == 'adjoint'
        full = np.zeros((6, th.vdim))
        full[:, inv], full[:, dbi] = E, dbv
        tr.rows = full
        tr.arm(table=[5 - k//2 for k in range(12)])
        tr.start(w)
        ev, ep = tr.run(12)
        print('adjoint over the adopted slots: v %.2e p %.2e' % (ev, ep))
        _note('adopted v', ev/VTOL)
        _note('adopted p', ep/PTOL)
        assert ev <= VTOL and ep <= PTOL
    finally:
        if tr is not None:
            tr.close()
        fwd.close()
        cva.close()
        cvk.close()


# ---- 6. the loops -----------------------------------------------------------------

@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_loops_about_a_trajectory_stored_every_second_step(gtiu, wake, scheme,
                                                           mode):
    from dolfin_navier_scipy_amd import convection
    femp, M = wake['femp'], wake['M']
    th, inv, dbcinds, dbcvals = (femp['V'], femp['invinds'], femp['dbcinds'],
                                 femp['dbcvals'])
    adj = mode == 'adjoint'
    wdbc = np.zeros(dbcvals.size) if adj else dbcvals
    nts = 12
    rows = _wake_rows(wake, nts//2 + 1, seed=31)
    w0 = _w0(wake).reshape((-1, 1))

    def appnd(vvec, bcs):
        full = np.full((th.vdim, 1), np.nan)
        full[inv] = vvec
        full[dbcinds, 0] = wdbc
        return full
    trange = wake['make_kw'](None, nts=nts)['trange']
    T = trange[-1]
    traj = _traj_of(rows, times=trange[::2],
                    time_map=(lambda t: T - t) if adj else None)
    # the host loop evaluates f_vdp at the Heun start's three states and then
    # at the state every step starts from: the times in that order
    seq = [trange[0], trange[1], trange[1]] + list(trange[1:-1])
    calls = []

    def f_vdp(vfull):
        k = traj.row_at(seq[len(calls)])
        calls.append(k)
        return tcl._host_conv(wake, rows[k], adj, adj)(vfull)

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
    assert calls[3:] == ([6 - (k + 1)//2 for k in range(1, nts)] if adj
                         else [k//2 for k in range(1, nts)])
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
        assert cvop.linearised == mode
        assert cvop.base_trajectory_rows == nts//2 + 1
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


# ---- 7. refusals ------------------------------------------------------------------

def _state(cv):
    return (cv.linearised, cv._base_info())


def test_refusals_of_the_operator(gtiu):
    c = case('rect-33')
    cv = c.t8
    c.set_traj('forward', 'rows')
    cv.set_base_rows([4, 3, 2])
    before, want = _state(cv), cv.apply(c.w)
    assert before == ('forward', (NROWS, 3))
    try:
        # the index table: every entry a row
        for bad, word in (([0, NROWS], 'entry 1 is %d' % NROWS),
                          ([-1], 'entry 0 is -1'),
                          ([0, 1, 2, 3, 4, 7], 'entry 5 is 7')):
            tcl._refused(lambda: cv.set_base_rows(bad), 'base rows', word,
                         'outside 0..%d' % (NROWS - 1))
        tcl._refused(lambda: cv.set_base_row(NROWS), 'base row %d' % NROWS)
        tcl._refused(lambda: cv.set_base_row(-1), 'base row -1')
        # shapes
        with pytest.raises(ValueError):
            cv.set_base_flow(_traj_of(np.zeros((3, c.nv + 1))))
        from dolfin_navier_scipy_amd import convection
        with pytest.raises(ValueError):
            cv.set_base_flow(convection.BaseTrajectory(
                np.arange(3), c.V[:3], np.zeros((2, c.ndbc))))
        # the adjoint with non-zero values of the perturbation, with a table
        tcl._refused(lambda: cv.set_base_flow(c.traj('rows'), adjoint=True),
                     'linearised convection, adjoint mode', 'Dirichlet value')
        assert _state(cv) == before
        assert np.array_equal(cv.apply(c.w), want)
        cv.set_dbc_table(np.tile(c.wd, (3, 1)))
        tcl._refused(lambda: cv.set_base_flow(c.traj('one'), adjoint=True),
                     'adjoint mode', 'dns_conv_set_dbc_table')
        assert _state(cv) == before
        cv.set_dbcvals(c.wd)
        assert np.array_equal(cv.apply(c.w), want)
        # without a trajectory there are no rows to name
        k = c.k8
        c.set_const('forward', 'rows', 0)
        tcl._refused(lambda: k.set_base_rows([0]), 'without a base trajectory')
        tcl._refused(lambda: k.set_base_row(0), 'without a base trajectory')
        # an adjoint trajectory refuses values and tables like any adjoint
        c.set_traj('adjoint', 'rows')
        tcl._refused(lambda: cv.set_dbcvals(c.wd), 'adjoint mode')
        tcl._refused(lambda: cv.set_dbc_table(np.zeros((3, c.ndbc))),
                     'adjoint mode', 'table')
        # the entry points that form the nonlinear matrices and tensors
        cv.bind_pattern(cv.connectivity())
        tcl._refused(lambda: cv.assemble(c.w), 'linearised convection '
                     'operator', 'dns_conv_assemble')
        tcl._refused(lambda: cv.project_tensor(
            np.ones((2, c.nv + c.nv % 2))), 'dns_conv_project_tensor')
    finally:
        cv.clear_base_flow()
        cv.set_dbcvals(c.wd)


def test_refusals_of_the_loop(gtiu, wake):
    """times not covered and `rom`: `ValueError` by name before anything is
    armed"""
    from dolfin_navier_scipy_amd import convection
    femp = wake['femp']
    cvop = convection.ConvectionP2.from_taylor_hood(
        femp['V'], femp['invinds'], femp['dbcinds'], femp['dbcvals'])
    kw = wake['make_kw'](scenarios.Recorder(), nts=8)
    kw.pop('f_vdp')
    trange = kw['trange']
    rows = _wake_rows(wake, 3)
    try:
        for times, word in ((trange[2:5], 'before the first stored time'),
                            (trange[0:3], 'more than one storage interval')):
            cvop.set_base_flow(_traj_of(rows, times=times))
            state = _state(cvop)
            with pytest.raises(ValueError) as exc:
                gtiu.cnab(device_convection=cvop, invinds=femp['invinds'],
                          resident=dict(record=True), **kw)
            assert 'base trajectory: time' in str(exc.value)
            assert word in str(exc.value)
            assert _state(cvop) == state
        cvop.set_base_flow(_traj_of(rows, times=trange[::4]))
        with pytest.raises(ValueError) as exc:
            gtiu.cnab(device_convection=cvop, invinds=femp['invinds'],
                      resident=dict(pod=object(), rom=object()), **kw)
        assert 'linearised convection operator' in str(exc.value)
        assert '`rom`' in str(exc.value)
        assert cvop.base_trajectory_rows == 3
    finally:
        cvop.close()


def test_refusals_of_the_steppers(gtiu, toy_prob):
    from dolfin_navier_scipy_amd import (saddle, convection, comm as dcomm,
                                         newton_picard as dnp)
    M, A, J = (toy_prob['smc'][k] for k in 'MAJ')
    dt = 5e-3
    cvop = convection.ConvectionP2.from_taylor_hood(
        toy_prob['th'], toy_prob['invinds'], toy_prob['dbcinds'],
        toy_prob['dbcvals'])
    rows = np.zeros((2, toy_prob['th'].vdim))
    rows[:, toy_prob['dbcinds']] = toy_prob['dbcvals']
    traj = _traj_of(rows)
    cvop.set_base_flow(traj)
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
        cvop.set_base_rows([1, 0])
        stp.set_state(np.zeros(J.shape[1]))
        cf = saddle.ImexStepper.coeffs(a_c=1., cn_c=1.5*dt, cn_o=-.5*dt,
                                       pscale=-1./dt, extrapolate=4)
        tcl._refused(lambda: stp.run(1, cf, saddle.solve_opts(method='gmres')),
                     'linearised convection operator on a row-partitioned '
                     'stepper')
        assert _state(cvop) == ('forward', (2, 2))
    finally:
        if stp is not None:
            stp.set_convection(None)
            stp.close()
        system.set_comm(None)
        system.close()
        cmm.close()
        cvop.close()


def test_functionals_with_cells_and_adoption_are_refused(gtiu, wake, toy_prob):
    from dolfin_navier_scipy_amd import fem, convection
    femp = wake['femp']
    fn = fem.boundary_forces(femp['V'], femp)
    assert fn.cells[0].size > 0
    lp = tcl.LinLoop(wake)
    toy = convection.ConvectionP2.from_taylor_hood(
        toy_prob['th'], toy_prob['invinds'], toy_prob['dbcinds'],
        toy_prob['dbcvals'])
    try:
        w0 = 0.1*wake['inivel'][:, 0]
        lp.start(w0)
        # no ensemble: nothing to adopt
        tcl._refused(lambda: lp.stp.ensemble_to_base(
            lp.cvop, dbcvals=femp['dbcvals']), 'base trajectory from the '
            'ensemble', 'no ensemble is set')
        assert _state(lp.cvop) == (False, (0, 0))
        lp.stp.set_ensemble([0, 1], nslots=2)
        lp.stp.run(2, lp.cf, lp.opts)
        # an operator of another space; slots out of range
        tcl._refused(lambda: lp.stp.ensemble_to_base(
            toy, dbcvals=toy_prob['dbcvals']), 'base trajectory from the '
            'ensemble', 'inner dofs')
        assert _state(toy) == (False, (0, 0))
        tcl._refused(lambda: lp.stp.ensemble_to_base(
            lp.cvop, first=1, count=2, dbcvals=femp['dbcvals']),
            'slots 1 .. 2 outside 0..1')
        assert _state(lp.cvop) == (False, (0, 0))
        lp.stp.clear_ensemble()
        # functionals with cells
        lp.stp.set_functionals(fn, 8, lp.dt)
        lp.stp.run(1, lp.cf, lp.opts)
        lp.cvop.set_base_flow(_traj_of(_wake_rows(wake, 2)))
        lp.cvop.set_base_rows([1, 0])
        for go in (lambda: lp.stp.run(1, lp.cf, lp.opts),
                   lambda: lp.stp.step(lp.cf, opts=lp.opts)):
            tcl._refused(go, 'linearised convection operator with '
                         'functionals with cells')
        lp.cvop.clear_base_flow()
        lp.stp.run(1, lp.cf, lp.opts)
    finally:
        lp.close()
        toy.close()


# ---- 8. report --------------------------------------------------------------------

def test_zz_report_and_close():
    """prints the largest error / bound per path (the module's docstring holds
    the figures measured on the MI355X)"""
    print('largest error / bound per path: '
          + '  '.join('%s %.3g' % kv for kv in sorted(WORST.items())))
    for c in _cache.values():
        c.close()
    _cache.clear()
