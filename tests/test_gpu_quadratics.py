"""Device-resident quadratic functionals of the explicit loops -- the energy
budget (`k_quadratic_step`, `dns_imex_set_quadratics`, `resident=dict(
quadratics=...)` of `cnab` / `sbdftwo`, `solve_nse(quadratics=...)`): every row
of the device's log against the NumPy statement
`fem.QuadraticFunctionals.evaluate` on the states the recorder wrote down in
the same run.

Shapes (those of `test_gpu_functionals.py`): the reference's `cylinder_1` mesh,
NV = 5812, NP = 806, dense Schur block, dt = 1/512, from the Stokes state.
5812 rows are 363 passes of 16 rows and a quarter of one; three matrices are
1092 passes -- more than the 256 workgroups of the default grid (the stride),
and with `max_grid=3` an uneven partition in which a workgroup's passes change
matrix.  The forms: the four builders (`M` shared by three of them) and two
forms, `(0, 0)` and `(1, 0)`, on a seeded, non-symmetric `R` whose rows hold
0, 1, 17 and 300 entries among ordinary ones (a row shorter than its 16 lanes,
one that fills them once, one that takes five rounds), with a `qa` row, a `qw`
row, `c0` and scale 0.7: nM = 3, nQ = 6.

Tolerance: `|row - evaluate| <= n_k 2^-52 T_k`, `T_k` the sum of the absolute
values of the `n_k` products of form k (in `np.longdouble`): the a-priori
bound of a sum of fp64 products in ANY order -- derived, not measured.  One
dropped or misplaced product of ~3e5 moves the sum by ~`T_k / n_k`, four
orders above it.  Measured on the MI355X: worst 1.2e-4 of the bound over every
test of this file (`profiles/r14_quadratics/README.md`).
"""
import numpy as np
import pytest
import scipy.sparse as sps

import feedback_setup as fs
import scenarios
from oracle import saddle_oracle

pytestmark = pytest.mark.gpu

EPS = 2.**-52
DT = 1./512
ODD_ROWS = {5: 0, 6: 1, 7: 17, 100: 300, 5811: 300, 5810: 0}


@pytest.fixture(scope='module')
def gtiu():
    from dolfin_navier_scipy_amd import time_int_utils, _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    return time_int_utils


def _general_matrix(NV, seed=11):
    """non-symmetric, about 30 entries a row, the rows of ODD_ROWS with the
    lengths given there"""
    rng = np.random.default_rng(seed)
    R = sps.random(NV, NV, density=30./NV, format='lil', random_state=rng)
    for row, n in ODD_ROWS.items():
        cols = np.sort(rng.choice(NV, size=n, replace=False))
        R.rows[row] = cols.tolist()
        R.data[row] = rng.standard_normal(n).tolist()
    R = sps.csr_matrix(R)
    R.sort_indices()
    lens = np.diff(R.indptr)
    assert [int(lens[r]) for r in ODD_ROWS] == list(ODD_ROWS.values())
    assert abs(R - R.T).max() > 0.1
    return R


def _forms(th, femp, NV):
    from dolfin_navier_scipy_amd import fem
    rng = np.random.default_rng(3)
    R = _general_matrix(NV)
    qa = sps.vstack([sps.random(1, NV, density=300./NV, format='csr',
                                random_state=rng),
                     sps.csr_matrix((1, NV))]).tocsr()
    qw = sps.vstack([sps.csr_matrix((1, NV)),
                     sps.random(1, NV, density=40./NV, format='csr',
                                random_state=rng)]).tocsr()
    onR = fem.QuadraticFunctionals.from_matrices(
        NV, [R], [(0, 0, 0), (0, 1, 0)], qa=qa, qw=qw, c0=[.3, -.2],
        scale=[.7, .7], names=['vRv', 'wRv'])
    qf = fem.energy_budget(th, femp) + onR
    assert (qf.nM, qf.nQ) == (3, 6)
    return qf


def _problem(N):
    from dolfin_navier_scipy_amd import fem
    femp, sm, rhsd = fem.get_sysmats(problem='cylinderwake', N=N, Re=100)
    th, inv = femp['V'], femp['invinds']
    M, A, J = sm['M'].tocsr(), sm['A'].tocsr(), sm['J'].tocsr()
    NP, NV = J.shape
    vp0 = saddle_oracle.solve_sadpnt_smw(amat=A, jmat=J, rhsv=rhsd['fv'],
                                         rhsp=rhsd['fp'])
    return dict(femp=femp, th=th, inv=inv, M=M, A=A, J=J, rhsd=rhsd, NV=NV,
                NP=NP, v0=vp0[:NV], p0=-vp0[NV:], qf=_forms(th, femp, NV))


@pytest.fixture(scope='module')
def c1(gtiu):
    c = _problem(1)
    assert (c['NV'], c['NP'], c['th'].mesh.ncells) == (5812, 806, 1501)
    return c


class Loop1(object):
    """CNAB / SBDF2 coefficients on `cylinder_1` from the Stokes state"""

    def __init__(self, c, scheme='cnab', use_graph=True):
        from dolfin_navier_scipy_amd import saddle, convection
        M, A, J, rhsd = c['M'], c['A'], c['J'], c['rhsd']
        dt = self.dt = DT
        femp = c['femp']
        self.cvop = convection.ConvectionP2.from_taylor_hood(
            femp['V'], femp['invinds'], femp['dbcinds'], femp['dbcvals'])
        if scheme == 'cnab':
            F, R1, g = M + .5*dt*A, M - .5*dt*A, dt*rhsd['fv']
            self.cf = saddle.ImexStepper.coeffs(
                a_c=1., cn_c=1.5*dt, cn_o=-.5*dt, pscale=-1./dt, extrapolate=4)
        else:
            F, R1, g = M + 2./3*dt*A, M, 2./3*dt*rhsd['fv']
            self.cf = saddle.ImexStepper.coeffs(
                a_c=4./3, a_p=-1./3, cn_c=4./3*dt, cn_o=-2./3*dt,
                pscale=-1./dt, extrapolate=4)
        self.system = saddle.SaddleSystem(F.tocsr(), J)
        self.system.setup_precond(cheb_degree=6, schur='dense', drop_tol=1e-3,
                                  factorization='full')
        self.stp = saddle.ImexStepper(self.system, R1.tocsr())
        nfc = self.cvop.apply(c['v0'], scale=-1.0)
        self.stp.set_state(c['v0'], v_p=c['v0'], nfc_c=nfc, nfc_o=nfc)
        self.stp.set_rhs(g, rhsd['fp'])
        self.stp.set_convection(self.cvop, scale=-1.0)
        self.opts = saddle.solve_opts(method='gmres', rtol=1e-10, maxiter=400,
                                      restart=60, check_every=2,
                                      use_graph=use_graph, reorth=2)

    def recorded(self, qf, nst, how='run', max_grid=None, parts=None):
        """`nst` steps with recorder and quadratics: `(rows, vs)`; `parts`:
        the `run` calls the steps are split into"""
        self.stp.set_recorder(nst, snap_slots='all')
        if qf is not None:
            self.stp.set_quadratics(qf, nst, self.dt, max_grid=max_grid)
        if how == 'run':
            for n in (parts or [nst]):
                self.stp.run(n, self.cf, self.opts)
        else:
            for _ in range(nst):
                self.stp.step(self.cf, opts=self.opts)
        vs, ps = self.stp.record_snapshots()
        rows = None if qf is None else self.stp.get_quadratics()
        return rows, vs

    def close(self):
        self.stp.close()
        self.cvop.close()
        self.system.close()


def _bounds(qf, vs, v_first, dt):
    """`(y, bound)` per row: `.evaluate` of the recorded states"""
    ys, bs = [], []
    for r in range(vs.shape[0]):
        vprev = vs[r - 1] if r else np.asarray(v_first).reshape(-1)
        y, T, n = qf.evaluate(vs[r], vprev, dt, return_scale=True)
        ys.append(y)
        bs.append(n*EPS*T)
    return np.array(ys), np.array(bs)


def _check_rows(qf, rows, vs, v_first, dt, what):
    """every row against `.evaluate` of the recorded states; returns the
    worst error in units of the bound"""
    assert rows.shape == (vs.shape[0], qf.nQ)
    assert np.isfinite(rows).all()
    ys, bs = _bounds(qf, vs, v_first, dt)
    assert np.all(bs > 0)
    worst = (np.abs(rows - ys)/bs).max(axis=0)
    print(what, ': worst |row - evaluate| in units of n 2^-52 T per form',
          dict(zip(qf.names, worst)))
    assert np.all(worst <= 1.), (what, worst)
    return worst


def _check_identity(qf, rows, vs, v_first, dt, what):
    """E_r - E_{r-1} = dt rate_r - dt^2/2 rate_norm_r on the device's rows, to
    the sum of the forms' bounds (the energy at its two rows)"""
    k = {n: i for i, n in enumerate(qf.names)}
    e, ra, rn = k['ekin'], k['ekin_rate'], k['rate_norm']
    _, bs = _bounds(qf, vs, v_first, dt)
    lhs = rows[1:, e] - rows[:-1, e]
    rhs = dt*rows[1:, ra] - .5*dt*dt*rows[1:, rn]
    bound = bs[1:, e] + bs[:-1, e] + dt*bs[1:, ra] + .5*dt*dt*bs[1:, rn]
    print(what, ': energy identity, worst defect in units of the bound',
          (np.abs(lhs - rhs)/bound).max())
    assert np.all(np.abs(lhs - rhs) <= bound)


# ---- 1. rows match the host statement, every step ----------------------------

@pytest.mark.parametrize('scheme,step6,how',
                         [('cnab', '1', 'run'), ('sbdf2', '1', 'run'),
                          ('cnab', '0', 'run'), ('cnab', '1', 'step')])
def test_rows_match_the_host_statement(gtiu, c1, monkeypatch, scheme, step6,
                                       how):
    """48 steps (`step`: 6) from the Stokes state with the default grid (256
    workgroups striding over 1092 passes), then as many with `max_grid=3`
    (re-armed: the matrices stay) -- a snapshot of every step in the same
    run.  `DNS_STEP6=0`: the fused form of the step; `step`: the synchronous
    step, one launch behind each"""
    monkeypatch.setenv('DNS_STEP6', step6)
    nst = 48 if how == 'run' else 6
    qf = c1['qf']
    lp = Loop1(c1, scheme)
    try:
        rows, vs = lp.recorded(qf, nst, how)
        last = dict(lp.stp.last_run) if how == 'run' else None
        vl = lp.stp.get_state()[0]
        rows3, vs3 = lp.recorded(qf, nst, how, max_grid=3)
    finally:
        lp.close()
    assert np.array_equal(vs[-1], vl[:, 0])
    if how == 'run':
        six = last['lazy_steps'] + last['eager_steps']
        assert (six > 0) if step6 == '1' else (six == 0), last
    what = '{0} step6={1} {2}'.format(scheme, step6, how)
    _check_rows(qf, rows, vs, c1['v0'], DT, what + ' default grid')
    _check_rows(qf, rows3, vs3, vs[-1], DT, what + ' max_grid=3')
    # the kinetic energy stays far from zero, the dissipation is positive and
    # the flow moves
    for r in (rows, rows3):
        assert r[:, 0].min() > 1e-2 and r[:, 1].min() > 0.
        assert r[:, 3].min() >= 0.
    assert np.abs(rows[:, 2]).max() > 0.
    _check_identity(qf, rows, vs, c1['v0'], DT, what + ' default grid')
    _check_identity(qf, rows3, vs3, vs[-1], DT, what + ' max_grid=3')


# ---- 2. read-only ---------------------------------------------------------------

def test_quadratics_leave_the_trajectory_alone(gtiu, c1):
    la, lb = Loop1(c1), Loop1(c1)
    try:
        la.stp.set_quadratics(c1['qf'], 64, DT)
        la.stp.run(64, la.cf, la.opts)
        lb.stp.run(64, lb.cf, lb.opts)
        va, pa = la.stp.get_state()
        vb, pb = lb.stp.get_state()
        assert np.array_equal(va, vb) and np.array_equal(pa, pb)
        for k in ('lazy_steps', 'eager_steps', 'unconverged', 'replayed'):
            assert la.stp.last_run[k] == lb.stp.last_run[k], k
        assert la.stp.get_quadratics().shape == (64, 6)
        # ... and a stepper that cleared them steps like one that never had any
        la.stp.clear_quadratics()
        assert la.stp.table_position() == (64, -1)
        la.stp.run(8, la.cf, la.opts)
        lb.stp.run(8, lb.cf, lb.opts)
        assert np.array_equal(la.stp.get_state()[0], lb.stp.get_state()[0])
    finally:
        la.close()
        lb.close()


# ---- 3. deterministic ------------------------------------------------------------

def test_logs_are_deterministic(gtiu, c1):
    qf = c1['qf']
    out = []
    for use_graph, parts in ((True, None), (True, None), (False, None),
                             (True, [7, 17])):
        lp = Loop1(c1, use_graph=use_graph)
        try:
            out.append(lp.recorded(qf, 24, parts=parts))
        finally:
            lp.close()
    (r0, v0), (r1, v1), (r2, v2), (r3, v3) = out
    assert np.array_equal(v0, v1)
    assert np.array_equal(r0, r1)
    # replayed graphs against plain launches, one call against two: the same
    # bits wherever the states are the same bits
    for what, (rx, vx) in (('plain launches', (r2, v2)),
                           ('run(7) + run(17)', (r3, v3))):
        same = [r for r in range(24) if np.array_equal(v0[r], vx[r])
                and (r == 0 or np.array_equal(v0[r - 1], vx[r - 1]))]
        print('graph run(24) vs', what, ': states identical in', len(same),
              'of 24')
        assert np.array_equal(r0[same], rx[same])
        if len(same) < 24:
            _check_rows(qf, rx, vx, c1['v0'], DT, what)


# ---- 4. a restored batch ------------------------------------------------------------

def test_a_restored_batch_overwrites_its_own_rows(gtiu):
    """the recipe of `test_gpu_record.py::test_a_restored_batch_overwrites_its_
    own_rows` (N = 2, the tabulated forcing jumps at step 128, the batch
    around it is restored and repeated) with the quadratics on: the log is
    not part of the checkpoint, the repeated batch writes its rows again --
    every row is the form of the state the recorder kept for it"""
    from dolfin_navier_scipy_amd import fem
    from test_gpu_feedback import WakeLoop, wake_setup
    wake = wake_setup()
    femp = wake['femp']
    qf = fem.energy_budget(femp['V'], femp)
    nst = 256
    lp = WakeLoop(wake, nst, feedback=False)
    try:
        lp.stp.set_recorder(nst, snap_slots='all')
        lp.stp.set_quadratics(qf, nst, 1./512)
        lp.run(nst)
        vs, ps = lp.stp.record_snapshots()
        rows = lp.stp.get_quadratics()
        record = dict(lp.record)
    finally:
        lp.close()
    print('recorded run:', record)
    assert record['unconverged'] == 0
    assert record['replayed'] > 0, record
    _check_rows(qf, rows, vs, wake['inivel'], 1./512, 'restored batch')


# ---- 5. with the other attachments ----------------------------------------------------

def test_rows_with_the_other_attachments(gtiu, c1):
    """feedback, recorder, functionals, statistics, quadratics: five nodes in
    front of the step; the other four say what they say without the fifth"""
    from dolfin_navier_scipy_amd import fem
    nst = 32
    qf, th, femp = c1['qf'], c1['th'], c1['femp']
    C, B = fs.sensors_actuators(th, c1['inv'], c1['M'])
    obs = fs.observer(7, C.shape[0], B.shape[1])
    fn = fem.boundary_forces(th, femp) \
        + fem.pressure_difference(th, (0.15, 0.2), (0.25, 0.2))
    pairs = fem.component_pairs(th, c1['inv'])[:50]
    got = []
    for with_q in (True, False):
        lp = Loop1(c1)
        try:
            stp = lp.stp
            stp.set_feedback(C, B, obs['ha'], obs['hb'], obs['hc'], c_n=.5,
                             c_c=.5, dt=DT)
            stp.set_feedback_state(obs['inihx'], np.zeros(12),
                                   obs['hc'] @ obs['inihx'])
            stp.set_feedback_table(nst, None)
            stp.set_functionals(fn, nst, DT)
            stp.set_statistics(np.zeros(nst, dtype=np.int32), nbins=1,
                               pairs=pairs, reset=True)
            rows, vs = lp.recorded(qf if with_q else None, nst)
            _, ps = stp.record_snapshots()
            got.append(dict(rows=rows, vs=vs, ps=ps, fb=stp.feedback_log(),
                            fn=stp.get_functionals(), st=stp.statistics()))
        finally:
            lp.close()
    a, b = got
    assert np.abs(a['fb'][1]).max() > 0
    _check_rows(qf, a['rows'], a['vs'], c1['v0'], DT, 'five attachments')
    assert np.array_equal(a['vs'], b['vs']) and np.array_equal(a['ps'], b['ps'])
    assert np.array_equal(a['fb'][0], b['fb'][0])
    assert np.array_equal(a['fb'][1], b['fb'][1])
    assert np.array_equal(a['fn'], b['fn'])
    assert a['st']['counts'].tolist() == [nst]
    for k in a['st']:
        assert np.array_equal(a['st'][k], b['st'][k]), k


# ---- 6. edges ---------------------------------------------------------------------------

def _raw_set(stp, mats, mat, lop, rop, qa=None, qw=None, nrows=4, dt=DT,
             max_grid=0, nM=None, nQ=None, spoil=None):
    """`dns_imex_set_quadratics` as it stands, past the checks of the Python
    layers; `spoil(views)`: edit the CSR views before the call"""
    from dolfin_navier_scipy_amd import _capi as C
    views = [C.CsrView(m.copy()) for m in mats]      # (`spoil` edits them)
    lin = [None if m is None else C.CsrView(m) for m in (qa, qw)]
    if spoil is not None:
        spoil(views)
    structs = (C.dns_csr*max(len(views), 1))(*[v.struct for v in views])
    arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (mat, lop, rop)]
    return stp.lib.dns_imex_set_quadratics(
        stp._h, len(views) if nM is None else nM, structs,
        len(mat) if nQ is None else nQ,
        *[a.ctypes.data_as(C.c_int32_p) for a in arrs],
        *[None if v is None else v.byref() for v in lin], None, None,
        float(dt), int(nrows), int(max_grid))


def test_edges_and_refusals(gtiu, c1):
    from dolfin_navier_scipy_amd import _capi, fem
    qf, femp, NV = c1['qf'], c1['femp'], c1['NV']
    lp = Loop1(c1)
    try:
        stp = lp.stp
        # rows used up
        stp.set_quadratics(qf, 4, DT)
        assert stp.table_position() == (0, 4)
        stp.run(4, lp.cf, lp.opts)
        for go in (lambda: stp.run(1, lp.cf, lp.opts),
                   lambda: stp.step(lp.cf, opts=lp.opts)):
            with pytest.raises(_capi.DnsError) as exc:
                go()
            assert exc.value.status == _capi.DNS_ERR_NOT_READY
            assert 'dns_imex_set_quadratics' in str(exc.value)
        # getter ranges
        assert stp.get_quadratics(1, 3).shape == (3, 6)
        assert stp.get_quadratics(4, 0).shape == (0, 6)
        for first, count in ((2, 3), (-1, 2), (5, 0)):
            with pytest.raises(_capi.DnsError) as exc:
                stp.get_quadratics(first, count)
            assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        # re-arming with the same matrices keeps the buffers and with them
        # the graphs: nothing is captured in the second of two equal slices
        stp.set_quadratics(qf, 24, DT)
        stp.run(24, lp.cf, lp.opts)
        caps = []
        for _ in range(2):
            stp.set_quadratics(qf, 24, DT)
            stp.run(24, lp.cf, lp.opts)
            caps.append(stp.last_run['captures'])
        print('captures of two equal slices:', caps)
        assert caps[1] == 0, caps
        v_keep = stp.get_state()[0][:, 0]
        # every limit; a refused call leaves what was set: the forms go on
        # through the refusals, checked below
        stp.set_recorder(12, snap_slots='all')
        stp.set_quadratics(qf, 12, DT)
        stp.run(4, lp.cf, lp.opts)
        eye = sps.identity(NV, format='csr')
        one = ([eye], [0], [0], [0])

        def bad_column(views):
            views[0].indices[3] = NV

        def negative_column(views):
            views[0].indices[0] = -1
        wide = sps.csr_matrix((1, NV + 1))
        refused = [
            ('nM = 0', dict(nM=0)), ('nM = 5', dict(nM=5)),
            ('nQ = 0', dict(nQ=0)), ('nQ = 9', dict(nQ=9)),
            ('nrows', dict(nrows=0)), ('max_grid', dict(max_grid=-1)),
            ('dt', dict(dt=0.)), ('2^31', dict(nrows=(1 << 31)//256 + 1)),
            ('column index', dict(spoil=bad_column)),
            ('column index', dict(spoil=negative_column)),
            ('qa must be', dict(qa=wide)), ('qw must be', dict(qw=wide)),
            ('qa must be', dict(qa=sps.csr_matrix((2, NV))))]
        for word, kw in refused:
            assert _raw_set(stp, *one, **kw) == _capi.DNS_ERR_BAD_ARGUMENT, word
            assert word.encode() in stp.lib.dns_last_error(), \
                (word, stp.lib.dns_last_error())
        for mats, word in (([sps.identity(NV - 1, format='csr')], 'NV x NV'),
                           ([sps.csr_matrix((NV, NV + 1))], 'NV x NV')):
            assert _raw_set(stp, mats, [0], [0], [0]) \
                == _capi.DNS_ERR_BAD_ARGUMENT
            assert word.encode() in stp.lib.dns_last_error()
        for forms, word in ((([1], [0], [0]), 'mat['), (([-1], [0], [0]), 'mat['),
                            (([0], [2], [0]), 'operands'),
                            (([0], [0], [-1]), 'operands')):
            assert _raw_set(stp, [eye], *forms) == _capi.DNS_ERR_BAD_ARGUMENT
            assert word.encode() in stp.lib.dns_last_error()
        # the same through the Python layers: five matrices, nine forms
        five = fem.QuadraticFunctionals.from_matrices(
            NV, [eye.copy() for _ in range(5)], [(4, 0, 0)])
        nine = fem.QuadraticFunctionals.from_matrices(NV, [eye], [(0, 0, 0)]*9)
        for q, word in ((five, 'nM = 5'), (nine, 'nQ = 9')):
            with pytest.raises(_capi.DnsError) as exc:
                stp.set_quadratics(q, 4, DT)
            assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
            assert word in str(exc.value)
        # an operator with a per-step Dirichlet table: at the setter ...
        # (a table as long as the log: the rows are not what is missing)
        lp.cvop.set_dbc_table(np.tile(np.asarray(femp['dbcvals']), (12, 1)))
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_quadratics(qf, 4, DT)
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        assert 'Dirichlet table' in str(exc.value)
        # ... and at the step
        for go in (lambda: stp.run(1, lp.cf, lp.opts),
                   lambda: stp.step(lp.cf, opts=lp.opts)):
            with pytest.raises(_capi.DnsError) as exc:
                go()
            assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
            assert 'Dirichlet table' in str(exc.value)
        lp.cvop.set_dbcvals(femp['dbcvals'])
        assert stp.table_position()[0] == 4
        stp.run(8, lp.cf, lp.opts)
        rows = stp.get_quadratics()
        vs, _ = stp.record_snapshots()
        _check_rows(qf, rows, vs, v_keep, DT, 'through the refusals')
        v_keep = vs[-1]
        # the limits themselves are fine: four matrices and eight forms, one
        # matrix and one form whose matrix has no entry at all
        four = fem.QuadraticFunctionals.from_matrices(
            NV, [qf.mats[0], qf.mats[1], qf.mats[2], qf.mats[2].T.tocsr()],
            [(3, 1, 1), (0, 0, 0), (1, 0, 1), (2, 1, 0), (3, 0, 0), (0, 1, 1),
             (2, 0, 0), (1, 1, 0)])
        none = fem.QuadraticFunctionals.from_matrices(
            NV, [sps.csr_matrix((NV, NV))], [(0, 0, 1)], c0=[2.], scale=[3.])
        for few, grid in ((four, None), (four, 5), (none, 1)):
            assert (few.nM, few.nQ) in ((4, 8), (1, 1))
            r, vs = lp.recorded(few, 6, max_grid=grid)
            if few is none:
                assert np.array_equal(r, np.full((6, 1), 6.))
            else:
                _check_rows(few, r, vs, v_keep, DT,
                            'nM = 4, nQ = 8, grid %s' % grid)
            v_keep = vs[-1]
        # get after clear
        stp.clear_quadratics()
        with pytest.raises(ValueError):
            stp.get_quadratics()
        out = np.zeros(6)
        assert stp.lib.dns_imex_get_quadratics(
            stp._h, 0, 1, _capi.dptr(out)) == _capi.DNS_ERR_NOT_READY
        assert b'dns_imex_set_quadratics' in stp.lib.dns_last_error()
        stp.clear_quadratics()                       # (twice is fine)
    finally:
        lp.close()


def test_row_partitioned_stepper_is_refused(gtiu, c1):
    from dolfin_navier_scipy_amd import saddle, _capi, comm as dcomm
    M, A, J = c1['M'], c1['A'], c1['J']
    cm = dcomm.Comm.rccl(0, 1, 0, dcomm.rccl_unique_id())
    system = saddle.SaddleSystem((M + .5*DT*A).tocsr(), J)
    stp = None
    try:
        system.set_comm(cm)
        system.setup_precond(cheb_degree=6, schur='dense', fhat='explicit')
        stp = saddle.ImexStepper(system, (M - .5*DT*A).tocsr())
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_quadratics(c1['qf'], 4, DT)
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        assert 'partitioned' in str(exc.value)
    finally:
        if stp is not None:
            stp.close()
        system.set_comm(None)
        system.close()
        cm.close()


# ---- 7. through the drop-ins -------------------------------------------------------------

def _loop_kw(c, rec, nts=32):
    th, inv, femp, rhsd = c['th'], c['inv'], c['femp'], c['rhsd']

    def appnd(vvec, bcs):
        full = np.full((th.vdim, 1), np.nan)
        full[inv] = vvec
        full[femp['dbcinds'], 0] = femp['dbcvals']
        return full

    def f_vdp(vf):
        return -th.convection_vec(vf)[inv, :]
    return dict(trange=np.linspace(0, nts*DT, nts + 1), inivel=c['v0'],
                inip=c['p0'], bcs_ini=[], M=c['M'], A=c['A'], J=c['J'],
                f_vdp=f_vdp, f_tdp=lambda t: rhsd['fv'],
                g_tdp=lambda t: rhsd['fp'], scalep=-1.,
                getbcs=lambda t, v, p, mode=None: [],
                applybcs=lambda b: (0., 0., 0.), appndbcs=appnd, savevp=rec,
                check_ff_maxv=1e8, verbose=False, ntimeslices=3)


def _state_shift(qf, va, vpa, vb, vpb, dt):
    """how far the exact values of the forms at the states `(va, vpa)` and
    `(vb, vpb)` can lie apart, per form: with the operands `a = (va, va - vpa)`,
    `b = (vb, vb - vpb)` and `d = |a - b|`
        a_l^T Q a_r - b_l^T Q b_r = (a_l - b_l)^T Q a_r + b_l^T Q (a_r - b_r)
    (an identity), so
        |y(a) - y(b)| <= |scale| ( dt^-(l+r) (d_l^T |Q| |a_r| + |b_l|^T |Q| d_r)
                                   + |qa| . d_0 + |qw| . d_1 / dt )
    summed in `np.longdouble` like `T_k`"""
    ld = np.longdouble
    a = (va, va - vpa)
    b = (vb, vb - vpb)
    d = tuple(np.abs(x - y).astype(ld) for x, y in zip(a, b))
    out = np.zeros(qf.nQ)
    for k in range(qf.nQ):
        m, lo, ro = int(qf.mat[k]), int(qf.lop[k]), int(qf.rop[k])
        absq = abs(qf.mats[m]).astype(ld)
        t = (d[lo] @ (absq @ np.abs(a[ro]).astype(ld))
             + np.abs(b[lo]).astype(ld) @ (absq @ d[ro]))/ld(dt)**(lo + ro)
        qa, qw = qf.qa[k], qf.qw[k]
        t += (np.abs(qa.data).astype(ld)*d[0][qa.indices]).sum(dtype=ld)
        t += (np.abs(qw.data).astype(ld)*d[1][qw.indices]).sum(dtype=ld)/ld(dt)
        out[k] = float(ld(abs(qf.scale[k]))*t)
    return out


# states `savevp` sees where the loop runs resident WITHOUT the recorder:
# those behind rows 4, 19 and 30 (a row in the first slice, the last row of
# the second, the one-step slice) and the states before them
PLAIN_ROWS = (4, 19, 30)


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_through_the_time_loops(gtiu, c1, scheme):
    """the loop resident, with the recorder (`record`) and without (`plain`:
    ONE `run` per slice and stop, what a user runs), and one step at a time on
    the host.

    Every row of `record` and `host`, and the rows PLAIN_ROWS of `plain`,
    against `evaluate` of the states `savevp` saw on that path, within the
    bound.  Device against host path, EVERY row: the two paths take their own
    trajectories (the convection of the stepwise path is the host's, the
    solves end at `rtol`; no two states were the same bits when this was
    written), so the rows may differ by the summed bounds of the two PLUS
    what the difference of the states moves the exact value by -- bounded by
    `_state_shift`, an identity and the triangle inequality, no first-order
    term dropped.  The same for `plain` against `record` at PLAIN_ROWS.  That
    the tolerance still sees a wrong row is asserted with it: it stays below
    `T_k / n_k`, what ONE dropped product of average size moves a form by.
    Measured on the MI355X: the paths 9.6e-11 (CNAB) and 1.1e-10 (SBDF2)
    apart, device against host at most 0.13 of the tolerance, the tolerance
    at most 7.5e-4 of `T_k / n_k`"""
    from dolfin_navier_scipy_amd import convection
    qf, inv, femp = c1['qf'], c1['inv'], c1['femp']
    integ = gtiu.cnab if scheme == 'cnab' else gtiu.sbdftwo
    got = {}
    for mode in ('plain', 'record', 'host'):
        rec = scenarios.Recorder()
        kw = _loop_kw(c1, rec)
        trange = kw['trange']
        resident = dict(quadratics=qf)
        cvop = None
        if mode != 'host':
            kw.pop('f_vdp')
            cvop = convection.ConvectionP2.from_taylor_hood(
                femp['V'], inv, femp['dbcinds'], femp['dbcvals'])
            kw.update(device_convection=cvop, invinds=inv)
            keep = [float(trange[r + q]) for r in PLAIN_ROWS for q in (1, 2)]
            resident.update(savevp_times=keep if mode == 'plain' else None,
                            record=(mode == 'record'))
        try:
            v, p, ff = integ(resident=resident, **kw)
        finally:
            if cvop is not None:
                cvop.close()
        assert ff == 0
        lr = dict(gtiu.LAST_RUN)
        assert lr['quadratics'].shape == (31, 6)
        assert np.array_equal(lr['quadratics_t'], np.asarray(trange[2:]))
        assert lr['quadratics_names'] == qf.names
        times, vels, _ = rec.arrays()
        got[mode] = (lr, {float(t): vf[inv] for t, vf in zip(times, vels)})
    for mode in ('plain', 'record'):
        assert got[mode][0]['quadratics_on'] == 'device'
        assert got[mode][0]['run_calls'] > 0
    # (one `run` per slice and stop; SBDF2 keeps the state before a slice's
    # last step as a stop of its own)
    assert got['plain'][0]['run_calls'] <= 2*4 + len(PLAIN_ROWS)*2
    assert got['host'][0]['quadratics_on'] == 'host'
    assert got['host'][0]['run_calls'] == 0

    def at(mode, r):
        """the states behind row r of that path: `(v, v_prev)`"""
        seen = got[mode][1]
        return seen[float(trange[r + 2])], seen[float(trange[r + 1])]

    def own(mode, rows):
        """the rows against `evaluate` of the path's own states: the bounds"""
        out = {}
        worst = np.zeros(qf.nQ)
        for r in rows:
            y, T, n = qf.evaluate(*at(mode, r), DT, return_scale=True)
            out[r] = (n*EPS*T, T/n)
            worst = np.maximum(
                worst, np.abs(got[mode][0]['quadratics'][r] - y)/out[r][0])
        print(scheme, mode, ': worst |row - evaluate| in units of n 2^-52 T',
              dict(zip(qf.names, worst)))
        assert np.all(worst <= 1.), (mode, worst)
        return out
    bnd = dict(record=own('record', range(31)), host=own('host', range(31)),
               plain=own('plain', PLAIN_ROWS))

    def across(ma, mb, rows):
        ra, rb = got[ma][0]['quadratics'], got[mb][0]['quadratics']
        worst, power, moved = np.zeros(qf.nQ), np.zeros(qf.nQ), 0.
        for r in rows:
            (va, vpa), (vb, vpb) = at(ma, r), at(mb, r)
            moved = max(moved, np.abs(va - vb).max()/np.abs(vb).max())
            # (the shift itself is a longdouble sum of positive terms)
            tol = bnd[ma][r][0] + bnd[mb][r][0] \
                + (1. + 1e-9)*_state_shift(qf, va, vpa, vb, vpb, DT)
            worst = np.maximum(worst, np.abs(ra[r] - rb[r])/tol)
            power = np.maximum(power, tol/bnd[mb][r][1])
        print(scheme, ma, 'against', mb, ': states apart by', moved,
              '(max norm, relative); worst |row - row| in units of the '
              'tolerance', dict(zip(qf.names, worst)),
              '; tolerance in units of T / n', dict(zip(qf.names, power)))
        assert np.all(worst <= 1.), (ma, mb, worst)
        assert np.all(power < 1.), (ma, mb, power)
    across('record', 'host', range(31))
    across('plain', 'record', PLAIN_ROWS)
    across('plain', 'host', PLAIN_ROWS)
    # without the recorder the same rows, where the states seen are the same
    if all(np.array_equal(a, b) for r in PLAIN_ROWS
           for a, b in zip(at('plain', r), at('record', r))):
        assert np.array_equal(got['plain'][0]['quadratics'][list(PLAIN_ROWS)],
                              got['record'][0]['quadratics'][list(PLAIN_ROWS)])


def test_through_solve_nse(gtiu, c1):
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    qf, inv, femp, th = c1['qf'], c1['inv'], c1['femp'], c1['th']
    iniv = np.zeros((th.vdim, 1))
    iniv[inv] = c1['v0']
    iniv[femp['dbcinds'], 0] = femp['dbcvals']
    trange = np.linspace(0, 32*DT, 33)
    skw = dict(A=c1['A'], M=c1['M'], J=c1['J'], fv=c1['rhsd']['fv'],
               fp=c1['rhsd']['fp'], iniv=iniv, inip=c1['p0'], trange=trange,
               V=th, invinds=inv, dbcinds=femp['dbcinds'],
               dbcvals=femp['dbcvals'])
    try:
        vd, pd = snu.solve_nse(quadratics=qf, record_on_device=True,
                               return_dictofvelstrs=True,
                               return_dictofpstrs=True, **skw)
    finally:
        snu.clear_cache()
    lr = gtiu.LAST_RUN
    assert lr['quadratics_on'] == 'device' and lr['record'] == 'device'
    assert lr['quadratics'].shape == (31, 6)
    assert np.array_equal(lr['quadratics_t'], trange[2:])
    vs = np.array([vd[t][inv, 0] for t in trange[2:]])
    _check_rows(qf, lr['quadratics'], vs, vd[trange[1]][inv, 0], DT,
                'solve_nse')
    with pytest.raises(NotImplementedError):
        snu.solve_nse(quadratics=qf, treat_nonl_explicit=False, **skw)
