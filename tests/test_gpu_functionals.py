"""Device-resident force functionals of the explicit loops (`k_functional_step`,
`dns_imex_set_functionals`, `resident=dict(functionals=...)` of `cnab` /
`sbdftwo`, `solve_nse(functionals=...)`): every row of the device's log against
the NumPy statement `fem.MomentumFunctionals.evaluate` on the states the
recorder wrote down in the same run.

Shapes: the reference's `cylinder_1` mesh (NV = 5812, NP = 806, 1501 cells,
dense Schur block: the six-node step).  The cylinder has 39 cells -- more than
the 32 of one workgroup pass, no multiple of 8 -- and the bump about it a few
hundred: the stride, the partial pass and the sum over workgroups.

Tolerance `1e-11 * T_k`, `T_k` the sum of the absolute values of every product
of functional k: a functional sums at most a few thousand products, each cell
sum about a hundred flops, so fp64 rounding is about `5e3 * 1.1e-16 = 6e-13`
relative to `T_k`; the bound is 20x that.  Anything larger is a wrong index.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sps

import feedback_setup as fs
import scenarios
from oracle import saddle_oracle

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..', 'scripts'))

TOL = 1e-11
DT = 1./512


@pytest.fixture(scope='module')
def gtiu():
    from dolfin_navier_scipy_amd import time_int_utils, _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    return time_int_utils


def _bump(th, radius=0.12, center=(0.2, 0.2)):
    xy = th.nodecoords
    r2 = ((xy - np.asarray(center)[None, :])**2).sum(axis=1)/radius**2
    b = np.where(r2 < 1., (1. - np.minimum(r2, 1.))**2, 0.)
    phi = np.zeros((th.vdim, 1))
    phi[0::2, 0] = b
    phi[1::2, 0] = -.5*b
    return phi


def _problem(N):
    from dolfin_navier_scipy_amd import fem
    femp, sm, rhsd = fem.get_sysmats(problem='cylinderwake', N=N, Re=100)
    th, inv = femp['V'], femp['invinds']
    M, A, J = sm['M'].tocsr(), sm['A'].tocsr(), sm['J'].tocsr()
    NP, NV = J.shape
    vp0 = saddle_oracle.solve_sadpnt_smw(amat=A, jmat=J, rhsv=rhsd['fv'],
                                         rhsp=rhsd['fp'])
    rng = np.random.default_rng(3)
    row = sps.random(1, NV, density=300./NV, format='csr', random_state=rng)
    fn = fem.boundary_forces(th, femp) \
        + fem.pressure_difference(th, (0.15, 0.2), (0.25, 0.2)) \
        + fem.MomentumFunctionals.from_rows(th, femp, ca=row, c0=[0.3],
                                            scale=[0.7], names=['row']) \
        + fem.MomentumFunctionals(th, femp, _bump(th), names=['bump'])
    return dict(femp=femp, th=th, inv=inv, M=M, A=A, J=J, rhsd=rhsd, NV=NV,
                NP=NP, v0=vp0[:NV], p0=-vp0[NV:], fn=fn)


@pytest.fixture(scope='module')
def c1(gtiu):
    c = _problem(1)
    assert (c['NV'], c['NP'], c['th'].mesh.ncells) == (5812, 806, 1501)
    assert c['fn'].cells[0].size == 39 and c['fn'].cells[4].size > 100
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

    def recorded(self, fn, nst, how='run'):
        """`nst` steps with recorder and functionals: `(rows, vs, ps)`"""
        self.stp.set_recorder(nst, snap_slots='all')
        if fn is not None:
            self.stp.set_functionals(fn, nst, self.dt)
        if how == 'run':
            self.stp.run(nst, self.cf, self.opts)
        else:
            for _ in range(nst):
                self.stp.step(self.cf, opts=self.opts)
        vs, ps = self.stp.record_snapshots()
        rows = None if fn is None else self.stp.get_functionals()
        return rows, vs, ps

    def close(self):
        self.stp.close()
        self.cvop.close()
        self.system.close()


def _check_rows(fn, rows, vs, ps, v_first, dt, what):
    """every row against `.evaluate` of the recorded states; returns the
    worst error in units of `T_k`"""
    assert rows.shape == (vs.shape[0], fn.nF)
    assert np.isfinite(rows).all()
    worst = np.zeros(fn.nF)
    for r in range(rows.shape[0]):
        vprev = vs[r - 1] if r else np.asarray(v_first).reshape(-1)
        y, T = fn.evaluate(vs[r], vprev, ps[r], dt, return_scale=True)
        err = np.abs(rows[r] - y)/T
        worst = np.maximum(worst, err)
    print(what, ': worst |row - evaluate| / T per functional',
          dict(zip(fn.names, worst)))
    assert np.all(worst <= TOL), (what, worst)
    return worst


# ---- 1. rows match the host statement, every step ----------------------------

@pytest.mark.parametrize('scheme,step6,how',
                         [('cnab', '1', 'run'), ('sbdf2', '1', 'run'),
                          ('cnab', '0', 'run'), ('cnab', '1', 'step')])
def test_rows_match_the_host_statement(gtiu, c1, monkeypatch, scheme, step6,
                                       how):
    """48 steps from the Stokes state, a snapshot of every step in the same
    run: drag, lift, dp, a cell-free `ca` row and a smooth bump (general
    weights, a few hundred cells).  `DNS_STEP6=0`: the fused form of the
    step; `step`: the synchronous step, one launch behind each"""
    monkeypatch.setenv('DNS_STEP6', step6)
    nst = 48 if how == 'run' else 6
    lp = Loop1(c1, scheme)
    try:
        rows, vs, ps = lp.recorded(c1['fn'], nst, how)
        last = dict(lp.stp.last_run) if how == 'run' else None
        vl, pl = lp.stp.get_state()
    finally:
        lp.close()
    assert np.array_equal(vs[-1], vl[:, 0]) and np.array_equal(ps[-1], pl[:, 0])
    if how == 'run':
        six = last['lazy_steps'] + last['eager_steps']
        assert (six > 0) if step6 == '1' else (six == 0), last
    _check_rows(c1['fn'], rows, vs, ps, c1['v0'], DT,
                '{0} step6={1} {2}'.format(scheme, step6, how))
    # the values move and every term counts: drag far from zero, dp = p_a - p_b
    assert np.abs(rows[:, 0]).min() > 1e-3
    cp = c1['fn'].cp[2].toarray()[0]
    a, b = int(np.argmax(cp)), int(np.argmin(cp))
    assert np.all(np.abs(rows[:, 2] - (ps[:, a] - ps[:, b]))
                  <= 1e-13*(np.abs(ps[:, a]) + np.abs(ps[:, b])))


# ---- 2. read-only ---------------------------------------------------------------

def test_functionals_leave_the_trajectory_alone(gtiu, c1):
    la, lb = Loop1(c1), Loop1(c1)
    try:
        la.stp.set_functionals(c1['fn'], 64, DT)
        la.stp.run(64, la.cf, la.opts)
        lb.stp.run(64, lb.cf, lb.opts)
        va, pa = la.stp.get_state()
        vb, pb = lb.stp.get_state()
        assert np.array_equal(va, vb) and np.array_equal(pa, pb)
        for k in ('lazy_steps', 'eager_steps', 'unconverged', 'replayed'):
            assert la.stp.last_run[k] == lb.stp.last_run[k], k
        assert la.stp.get_functionals().shape == (64, 5)
        # ... and a stepper that cleared them steps like one that never had any
        la.stp.clear_functionals()
        assert la.stp.table_position() == (64, -1)
        la.stp.run(8, la.cf, la.opts)
        lb.stp.run(8, lb.cf, lb.opts)
        assert np.array_equal(la.stp.get_state()[0], lb.stp.get_state()[0])
    finally:
        la.close()
        lb.close()


# ---- 3. deterministic ------------------------------------------------------------

def test_logs_are_deterministic(gtiu, c1):
    out = []
    for use_graph in (True, True, False):
        lp = Loop1(c1, use_graph=use_graph)
        try:
            out.append(lp.recorded(c1['fn'], 32))
        finally:
            lp.close()
    (r0, v0, p0), (r1, v1, p1), (r2, v2, p2) = out
    assert np.array_equal(v0, v1) and np.array_equal(p0, p1)
    assert np.array_equal(r0, r1)
    # replayed graphs against plain launches: the same bits wherever the
    # states are the same bits
    same = [r for r in range(32)
            if np.array_equal(v0[r], v2[r]) and np.array_equal(p0[r], p2[r])
            and (r == 0 or np.array_equal(v0[r - 1], v2[r - 1]))]
    print('graph vs plain launches: states identical in', len(same), 'of 32')
    assert np.array_equal(r0[same], r2[same])
    if len(same) < 32:
        _check_rows(c1['fn'], r2, v2, p2, c1['v0'], DT, 'plain launches')


# ---- 4. a restored batch ------------------------------------------------------------

def test_a_restored_batch_overwrites_its_own_rows(gtiu):
    """the recipe of `test_gpu_record.py::test_a_restored_batch_overwrites_its_
    own_rows` (N = 2, the tabulated forcing jumps at step 128, the batch
    around it is restored and repeated) with the functionals on: the log is
    not part of the checkpoint, the repeated batch writes its rows again --
    every row is the functional of the state the recorder kept for it (which
    that test compares with single steps)"""
    from dolfin_navier_scipy_amd import fem
    from test_gpu_feedback import WakeLoop, wake_setup
    wake = wake_setup()
    femp = wake['femp']
    th = femp['V']
    fn = fem.boundary_forces(th, femp) \
        + fem.pressure_difference(th, (0.15, 0.2), (0.25, 0.2))
    assert fn.cells[0].size == 62
    nst = 256
    lp = WakeLoop(wake, nst, feedback=False)
    try:
        lp.stp.set_recorder(nst, snap_slots='all')
        lp.stp.set_functionals(fn, nst, 1./512)
        lp.run(nst)
        vs, ps = lp.stp.record_snapshots()
        rows = lp.stp.get_functionals()
        record = dict(lp.record)
    finally:
        lp.close()
    print('recorded run:', record)
    assert record['unconverged'] == 0
    assert record['replayed'] > 0, record
    _check_rows(fn, rows, vs, ps, wake['inivel'], 1./512, 'restored batch')


# ---- 5. with observer feedback -------------------------------------------------------

def test_rows_with_observer_feedback(gtiu, c1):
    """feedback, recorder, functionals: three nodes in front of the step"""
    nst = 32
    C, B = fs.sensors_actuators(c1['th'], c1['inv'], c1['M'])
    obs = fs.observer(7, C.shape[0], B.shape[1])
    lp, lo = Loop1(c1), Loop1(c1)
    try:
        lp.stp.set_feedback(C, B, obs['ha'], obs['hb'], obs['hc'], c_n=.5,
                            c_c=.5, dt=DT)
        lp.stp.set_feedback_state(obs['inihx'], np.zeros(12),
                                  obs['hc'] @ obs['inihx'])
        lp.stp.set_feedback_table(nst, None)
        rows, vs, ps = lp.recorded(c1['fn'], nst)
        ylog, ulog = lp.stp.feedback_log()
        ro, vo, po = lo.recorded(c1['fn'], nst)
    finally:
        lp.close()
        lo.close()
    assert np.abs(ulog).max() > 0
    assert np.abs(vs[-1] - vo[-1]).max() > 1e-9*np.abs(vo[-1]).max()
    _check_rows(c1['fn'], rows, vs, ps, c1['v0'], DT, 'closed loop')
    # the observer saw the states the functionals were taken of
    assert np.abs(ylog[1:] - (C @ vs[:-1].T).T).max() <= \
        1e-12*np.abs(ylog).max()


# ---- 6. edges ---------------------------------------------------------------------------

def test_edges_and_refusals(gtiu, c1):
    from dolfin_navier_scipy_amd import _capi, fem
    fn, th, femp = c1['fn'], c1['th'], c1['femp']
    lp = Loop1(c1)
    try:
        stp = lp.stp
        # rows used up
        stp.set_functionals(fn, 4, DT)
        assert stp.table_position() == (0, 4)
        stp.run(4, lp.cf, lp.opts)
        for go in (lambda: stp.run(1, lp.cf, lp.opts),
                   lambda: stp.step(lp.cf, opts=lp.opts)):
            with pytest.raises(_capi.DnsError) as exc:
                go()
            assert exc.value.status == _capi.DNS_ERR_NOT_READY
            assert 'dns_imex_set_functionals' in str(exc.value)
        with pytest.raises(_capi.DnsError):
            stp.get_functionals(2, 3)
        # re-arming with the same shapes keeps the buffers and with them the
        # graphs: nothing is captured in the second of two equal slices (24
        # steps: a multiple of the ring's six vectors and of the groups)
        stp.set_functionals(fn, 24, DT)
        stp.run(24, lp.cf, lp.opts)
        caps = []
        for _ in range(2):
            stp.set_functionals(fn, 24, DT)
            stp.run(24, lp.cf, lp.opts)
            caps.append(stp.last_run['captures'])
        print('captures of two equal slices:', caps)
        assert caps[1] == 0, caps
        rows = stp.get_functionals()
        assert rows.shape == (24, 5) and np.abs(rows[:, 0]).min() > 1e-3
        v_keep = stp.get_state()[0]
        # refusals leave what was set
        lp.cvop.set_dbc_table(np.tile(np.asarray(femp['dbcvals']), (4, 1)))
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_functionals(fn, 4, DT)
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        assert 'Dirichlet table' in str(exc.value)
        lp.cvop.set_dbcvals(femp['dbcvals'])
        dp = fem.pressure_difference(th, 3, 5)
        many = dp
        for _ in range(16):
            many = many + dp
        assert many.nF == 17
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_functionals(many, 4, DT)
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        assert 'nF = 17' in str(exc.value)
        bad = fem.boundary_forces(th, femp)
        bad.cells[1] = bad.cells[1].copy()
        bad.cells[1][-1] = th.mesh.ncells
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_functionals(bad, 4, DT)
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        assert 'cell index' in str(exc.value)
        assert np.array_equal(stp.get_functionals(), rows)
        assert np.array_equal(stp.get_state()[0], v_keep)
        # nF = 1 without cells (and without velocity rows), nF = 16
        for few in (dp, fn + fn + fn + dp):
            assert few.nF in (1, 16)
            r, vs, ps = lp.recorded(few, 8)
            _check_rows(few, r, vs, ps, v_keep, DT, 'nF = %d' % few.nF)
            v_keep = vs[-1]
        # cells without a convection operator
        stp.set_convection(None)
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_functionals(fn, 4, DT)
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        assert 'convection' in str(exc.value)
    finally:
        lp.close()


def test_another_convection_operator_needs_the_functionals_set_again(gtiu,
                                                                     c1):
    """the listed cells are positions in the cell order of the operator that
    was attached when they were set: a step with another one is refused (its
    cell arrays may be shorter), attaching the first one again or setting the
    functionals again is fine"""
    from dolfin_navier_scipy_amd import _capi, convection
    fn, femp = c1['fn'], c1['femp']
    lp = Loop1(c1)
    other = convection.ConvectionP2.from_taylor_hood(
        femp['V'], femp['invinds'], femp['dbcinds'], femp['dbcvals'])
    try:
        stp = lp.stp
        stp.set_functionals(fn, 8, DT)
        stp.run(2, lp.cf, lp.opts)
        stp.set_convection(other, scale=-1.0)
        for go in (lambda: stp.run(1, lp.cf, lp.opts),
                   lambda: stp.step(lp.cf, opts=lp.opts)):
            with pytest.raises(_capi.DnsError) as exc:
                go()
            assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
            assert 'another convection operator' in str(exc.value)
        stp.set_convection(lp.cvop, scale=-1.0)
        stp.run(2, lp.cf, lp.opts)
        assert np.abs(stp.get_functionals()[:, 0]).min() > 1e-3
        stp.set_convection(other, scale=-1.0)
        v_first = stp.get_state()[0][:, 0]
        rows, vs, ps = lp.recorded(fn, 4)
        _check_rows(fn, rows, vs, ps, v_first, DT, 'other operator')
    finally:
        lp.stp.set_convection(None)
        other.close()
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
            stp.set_functionals(c1['fn'], 4, DT)
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


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_through_the_time_loops(gtiu, c1, scheme):
    from dolfin_navier_scipy_amd import convection
    fn, inv, femp = c1['fn'], c1['inv'], c1['femp']
    integ = gtiu.cnab if scheme == 'cnab' else gtiu.sbdftwo
    got = {}
    for mode in ('plain', 'record', 'host'):
        rec = scenarios.Recorder()
        kw = _loop_kw(c1, rec)
        resident = dict(functionals=fn)
        cvop = None
        if mode != 'host':
            kw.pop('f_vdp')
            cvop = convection.ConvectionP2.from_taylor_hood(
                femp['V'], inv, femp['dbcinds'], femp['dbcvals'])
            kw.update(device_convection=cvop, invinds=inv)
            resident.update(savevp_times=() if mode == 'plain' else None,
                            record=(mode == 'record'))
        try:
            v, p, ff = integ(resident=resident, **kw)
        finally:
            if cvop is not None:
                cvop.close()
        assert ff == 0
        lr = dict(gtiu.LAST_RUN)
        assert lr['functionals'].shape == (31, 5)
        assert np.allclose(lr['functionals_t'], kw['trange'][2:], rtol=0,
                           atol=1e-15)
        assert lr['functionals_names'] == fn.names
        got[mode] = (lr, rec.arrays(), v, p)
    slices = [c for c in gtiu._inittimegrid(kw['trange'], 3)[1] if c]
    assert [len(c) for c in slices] == [10, 10, 10, 1]
    # one `run` per slice (SBDF2 without the recorder: one more per slice for
    # the velocity before the last step, which its blow-up guard looks at)
    calls = dict(record=4, plain=4 if scheme == 'cnab' else 7)
    for mode in ('plain', 'record'):
        assert got[mode][0]['functionals_on'] == 'device'
        assert got[mode][0]['run_calls'] == calls[mode], \
            (mode, got[mode][0]['run_calls'])
    assert got['host'][0]['functionals_on'] == 'host'
    assert got['host'][0]['run_calls'] == 0
    # the rows are the functionals of the states `savevp` saw
    for mode in ('record', 'host'):
        lr, (times, vels, prss), _, _ = got[mode]
        assert times.size == 33
        vs = np.array([vf[inv] for vf in vels[2:]])
        _check_rows(fn, lr['functionals'], vs, np.array(prss[2:]),
                    vels[1][inv], DT, scheme + ' ' + mode)
    # without the recorder the same rows, where the end states are the same
    if np.array_equal(got['plain'][2], got['record'][2]):
        assert np.array_equal(got['plain'][0]['functionals'],
                              got['record'][0]['functionals'])
    last = got['plain'][0]['functionals'][-1]
    ref = got['record'][0]['functionals'][-1]
    assert np.abs(last - ref).max() <= 1e-6*np.abs(ref).max()


def test_through_solve_nse(gtiu, c1):
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    fn, inv, femp, th = c1['fn'], c1['inv'], c1['femp'], c1['th']
    iniv = np.zeros((th.vdim, 1))
    iniv[inv] = c1['v0']
    iniv[femp['dbcinds'], 0] = femp['dbcvals']
    trange = np.linspace(0, 32*DT, 33)
    skw = dict(A=c1['A'], M=c1['M'], J=c1['J'], fv=c1['rhsd']['fv'],
               fp=c1['rhsd']['fp'], iniv=iniv, inip=c1['p0'], trange=trange,
               V=th, invinds=inv, dbcinds=femp['dbcinds'],
               dbcvals=femp['dbcvals'])
    try:
        vd, pd = snu.solve_nse(functionals=fn, record_on_device=True,
                               return_dictofvelstrs=True,
                               return_dictofpstrs=True, **skw)
    finally:
        snu.clear_cache()
    lr = gtiu.LAST_RUN
    assert lr['functionals_on'] == 'device' and lr['record'] == 'device'
    assert lr['run_calls'] == sum(
        1 for c in gtiu._inittimegrid(trange, 10)[1] if c)
    assert lr['functionals'].shape == (31, 5)
    assert np.allclose(lr['functionals_t'], trange[2:], rtol=0, atol=1e-15)
    vs = np.array([vd[t][inv, 0] for t in trange[2:]])
    ps = np.array([pd[t][:, 0] for t in trange[2:]])
    _check_rows(fn, lr['functionals'], vs, ps, vd[trange[1]][inv, 0], DT,
                'solve_nse')
    with pytest.raises(NotImplementedError):
        snu.solve_nse(functionals=fn, treat_nonl_explicit=False, **skw)


# ---- 8. physical ---------------------------------------------------------------------------

def test_schaefer_turek_forces_from_the_device_log(gtiu):
    """Schaefer-Turek 2D-1 at level 2: the last row of the device's log gives
    the `c_D`, `c_L` the script evaluates on the host for the same final
    state, at 1e-9 relative -- the functionals of the unsteady force, with
    the `M dv/dt` term in (`c?_device_dvdt`), and the steady ones without it
    (`c?_device`), which are the script's own formula.

    At the steady state `dv/dt` is the noise every step's solve leaves in `v`,
    divided by `dt` = 1/512, and `c_L` = 0.0088 is a small number next to the
    forces of size `c_D` = 5.55 that cancel in it.  So the march runs with the
    solves ended at `rtol` = 1e-13, not the script's default 1e-10.  Measured on
    the MI355X at t = 10, relative to the host value, with the term in:
        rtol 1e-10:  c_D 6.3e-12   c_L 4.0e-9   (c_L misses the bound)
        rtol 1e-12:  c_D 5.1e-13   c_L 7.2e-10
        rtol 1e-13:  c_D 5.6e-14   c_L 5.6e-11
    and without it 0 .. 2.5e-14 for both, whatever `rtol`."""
    import schaefer_turek as st
    out = st.run(N=2, refine=0, nts=512, tend=10.0, verbose=False,
                 device_forces=True, rtol=1e-13)
    assert out['last_change'] < 1e-7
    err = {}
    for k in ('cD', 'cL'):
        for sfx in ('_device', '_device_dvdt'):
            err[k + sfx] = abs(out[k + sfx]/out[k] - 1)
            print(k, 'host', out[k], k + sfx, out[k + sfx], 'rel',
                  err[k + sfx])
    assert max(err.values()) <= 1e-9, err
    ref = out['reference']
    assert abs(out['cD_device_dvdt']/ref['cD'] - 1) <= 0.01
