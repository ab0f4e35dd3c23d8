"""Device-resident observer feedback of the explicit loops (`k_lti_step`,
`dns_imex_set_feedback*`, `time_int_utils.LinearFeedback`): against the golden
vectors of the reference's own `cnab` / `sbdftwo` with the reference's own
observer, against the kernel's definition in NumPy, through batches and a
restored batch, at full size against the CPU oracle, and through `solve_nse`.

Tolerances: velocities and pressures 1e-8 relative (`VTOL` / `PTOL` of
`test_gpu_imex.py`); kernels against NumPy 1e-13 relative to the
sum of the absolute terms.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sps

import feedback_setup as fs
import scenarios
from oracle import imex_oracle, saddle_oracle

pytestmark = pytest.mark.gpu

VTOL, PTOL = 1e-8, 1e-8
KTOL = 1e-13
# test 6: the tabulated forcing jumps by JUMP_G times an actuator bump at step
# 128 and the observer is switched to the drift level JUMP_D there
JUMP_AT, JUMP_G, JUMP_D = 128, 5.0, 5.0


@pytest.fixture(scope='module')
def gtiu():
    from dolfin_navier_scipy_amd import time_int_utils, _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    return time_int_utils


def _golden(gtiu, golden_dir, scheme):
    gold = np.load(os.path.join(
        golden_dir, 'imex_{0}_feedback_s5.npz'.format(scheme)))
    fb = gtiu.LinearFeedback(fs.csr_unpack(gold, 'C'),
                             fs.csr_unpack(gold, 'B'), gold['ha'], gold['hb'],
                             gold['hc'], gold['inihx'],
                             drift=fs.drift_of(gold['dvec']))
    return gold, fb


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max()/np.abs(b).max()


# ---- 4. golden, resident ----------------------------------------------------

@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_resident_feedback_matches_reference_golden(gtiu, golden_dir, toy_prob,
                                                    scheme):
    """the drop-in loops with the golden's `LinearFeedback`, device convection
    and `resident=`: all 49 saved time points, the logs and the final memory
    against what the reference computed; the AB2 steps never call back"""
    from dolfin_navier_scipy_amd import convection
    gold, fb = _golden(gtiu, golden_dir, scheme)
    kw, rec, _ = scenarios.build(variant='plain', seed=5, Nts=48, tE=0.24,
                                 prob=toy_prob)
    kw.pop('f_vdp')
    cvop = convection.ConvectionP2.from_taylor_hood(
        toy_prob['th'], toy_prob['invinds'], toy_prob['dbcinds'],
        toy_prob['dbcvals'])
    mem = {}
    integ = gtiu.cnab if scheme == 'cnab' else gtiu.sbdftwo
    try:
        v, p, ff = integ(dynamic_rhs=fb, dynamic_rhs_memory=mem,
                         device_convection=cvop,
                         invinds=toy_prob['invinds'],
                         resident=dict(savevp_times=None), **kw)
    finally:
        cvop.close()
    assert ff == 0
    assert gtiu.LAST_RUN['feedback'] == 'resident'
    assert fb.calls == dict(init=1, heunpred=1, heuncorr=1, abtwo=0), fb.calls
    times, vels, prss = rec.arrays()
    assert times.size == gold['times'].size == 49
    assert np.allclose(times, gold['times'], rtol=0, atol=1e-15)
    worst_v = worst_p = 0.
    for k in range(49):
        ev = np.linalg.norm(vels[k] - gold['vels'][k]) / \
            np.linalg.norm(gold['vels'][k])
        dp = np.linalg.norm(prss[k] - gold['prss'][k])
        npk = np.linalg.norm(gold['prss'][k])
        worst_v = max(worst_v, ev)
        worst_p = max(worst_p, dp/npk if npk > 0 else dp)
        assert ev <= VTOL, (k, ev)
        assert dp <= PTOL*npk, (k, dp, npk)
    print(scheme, 'golden, resident: worst v', worst_v, 'p', worst_p)
    # logs of the 47 AB2 steps against the reference's callback record
    ab = gold['cb_mode'] == 3
    ylog, ulog = gtiu.LAST_RUN['feedback_y'], gtiu.LAST_RUN['feedback_u']
    assert ylog.shape == (47, 3) and ulog.shape == (47, 2)
    print(scheme, 'logs: y', _rel(ylog, gold['cb_y'][ab]), 'u',
          _rel(ulog, gold['cb_u'][ab]))
    assert _rel(ylog, gold['cb_y'][ab]) <= 1e-8
    assert _rel(ulog, gold['cb_u'][ab]) <= 1e-8
    # the final observer memory
    assert abs(mem['lastt'] - float(gold['mem_lastt'])) <= 1e-14
    assert abs(mem['lastdt'] - float(gold['mem_lastdt'])) <= 1e-14
    print(scheme, 'memory: hx', _rel(mem['lasthx'], gold['mem_lasthx']),
          'rhs', _rel(mem['lastrhs'], gold['mem_lastrhs']))
    assert _rel(mem['lasthx'], gold['mem_lasthx']) <= 1e-8
    assert _rel(mem['lastrhs'], gold['mem_lastrhs']) <= 1e-8


def test_other_dynamic_rhs_keeps_the_host_path(gtiu, toy_prob):
    """an arbitrary closure (the `forced` scenario) is called every step, and
    so is a `LinearFeedback` without `resident=`"""
    kw, rec, _ = scenarios.build(variant='forced', seed=1, Nts=6, tE=0.03,
                                 prob=toy_prob)
    gtiu.cnab(**kw)
    assert gtiu.LAST_RUN['feedback'] == 'host'
    kw, rec, _ = scenarios.build(variant='plain', seed=1, Nts=6, tE=0.03,
                                 prob=toy_prob)
    gtiu.cnab(**kw)
    assert gtiu.LAST_RUN['feedback'] is None


# ---- toy stepper for the kernel-level tests ---------------------------------

class ToyLoop(object):
    def __init__(self, prob, dt=5e-3, seed=11, hN=12, rows_only=False):
        from dolfin_navier_scipy_amd import saddle, convection
        M, A, J = (prob['smc'][k] for k in 'MAJ')
        self.M, self.dt = M, dt
        NP, NV = J.shape
        self.system = saddle.SaddleSystem((M + .5*dt*A).tocsr(), J)
        self.system.setup_precond(cheb_degree=6, schur='dense')
        self.stp = saddle.ImexStepper(self.system, (M - .5*dt*A).tocsr())
        self.cvop = convection.ConvectionP2.from_taylor_hood(
            prob['th'], prob['invinds'], prob['dbcinds'], prob['dbcvals'])
        rng = np.random.default_rng(seed)
        self.v0 = 1e-1*rng.standard_normal((NV, 1))
        self.stp.set_state(self.v0)
        self.stp.set_rhs(dt*prob['rhsd']['fv'], prob['rhsd']['fp'])
        self.stp.set_convection(self.cvop, scale=-1.0)
        self.cf = saddle.ImexStepper.coeffs(a_c=1., cn_c=1.5*dt, cn_o=-.5*dt,
                                            pscale=-1./dt, extrapolate=4)
        self.opts = saddle.solve_opts(method='gmres', rtol=1e-12, maxiter=400,
                                      restart=60, check_every=2,
                                      use_graph=True, reorth=2)
        self.C, self.B = fs.sensors_actuators(prob['th'], prob['invinds'], M)
        self.obs = fs.observer(seed, 3, 2, hN=hN)

    def close(self):
        self.stp.close()
        self.cvop.close()
        self.system.close()


# ---- 5. the kernel against its definition -----------------------------------

@pytest.mark.parametrize('hN', [12, 128])
def test_lti_kernel_against_its_definition(gtiu, toy_prob, hN):
    """32 steps, one `run(1)` each: the logged `y` against `C v_k` row by row
    at 1e-13 (|C| |v_k|); `u` and the observer state against the NumPy
    recurrence fed with the logged `y`, at 1e-13 relative to the sum of the
    absolute terms (hN = 12: the matrices staged in LDS; 128: the limit, read
    in place, the state longer than a workgroup)"""
    lp = ToyLoop(toy_prob, hN=hN)
    try:
        stp, obs, dt = lp.stp, lp.obs, lp.dt
        ha, hb, hc = obs['ha'], obs['hb'], obs['hc']
        nst = 32
        rng = np.random.default_rng(5)
        drift = rng.standard_normal((nst, hN))
        hx = obs['inihx'][:, 0].copy()
        fl = rng.standard_normal(hN)
        uc = hc @ hx
        stp.set_feedback(lp.C, lp.B, ha, hb, hc, c_n=.5, c_c=.5, dt=dt)
        stp.set_feedback_state(hx, fl, uc)
        stp.set_feedback_table(nst, drift)
        got = stp.feedback_state()
        assert all(np.array_equal(a, b) for a, b in zip(got, (hx, fl, uc)))
        absC = abs(lp.C)
        vs = [stp.get_state()[0]]
        for k in range(nst):
            stp.run(1, lp.cf, lp.opts)
            vs.append(stp.get_state()[0])
            ghx, gfl, guc = stp.feedback_state()
            ylog, ulog = stp.feedback_log(k, 1)
            y = ylog[0]
            bound = KTOL*(absC @ np.abs(vs[k]))[:, 0]
            assert np.all(np.abs(y - (lp.C @ vs[k])[:, 0]) <= bound), k
            f = ha @ hx + hb @ y + drift[k]
            fabs = np.abs(ha) @ np.abs(hx) + np.abs(hb) @ np.abs(y) \
                + np.abs(drift[k])
            assert np.all(np.abs(gfl - f) <= KTOL*fabs), k
            hxn = hx + 1.5*dt*f - .5*dt*fl
            hxabs = np.abs(hx) + 1.5*dt*fabs + .5*dt*np.abs(fl)
            assert np.all(np.abs(ghx - hxn) <= KTOL*hxabs), k
            un = hc @ hxn
            assert np.all(np.abs(guc - un) <= KTOL*(np.abs(hc) @ hxabs)), k
            assert np.array_equal(ulog[0], guc)
            # (the next step starts from the device's own values)
            hx, fl, uc = ghx, gfl, guc
        # the whole log at once, and the effect on the velocity: the same
        # steps without feedback end elsewhere
        ylog, ulog = stp.feedback_log()
        assert ylog.shape == (nst, 3) and ulog.shape == (nst, 2)
        assert stp.table_position() == (nst, 0)
        with pytest.raises(Exception):          # the table is used up
            stp.run(1, lp.cf, lp.opts)
    finally:
        lp.close()


def test_closed_loop_steps_match_the_host_recurrence(gtiu, toy_prob):
    """40 resident steps (batches) against the same steps taken with the
    right-hand side formed on the host from the logged inputs: the term
    enters the step with the coefficients and the timing of tiu:125-128"""
    lp, lh = ToyLoop(toy_prob), ToyLoop(toy_prob)
    try:
        obs, dt, nst = lp.obs, lp.dt, 40
        hx, fl = obs['inihx'][:, 0], np.zeros(12)
        uc0 = obs['hc'] @ hx
        lp.stp.set_feedback(lp.C, lp.B, obs['ha'], obs['hb'], obs['hc'],
                            c_n=.5, c_c=.5, dt=dt)
        lp.stp.set_feedback_state(hx, fl, uc0)
        lp.stp.set_feedback_table(nst, None)
        lp.stp.run(nst, lp.cf, lp.opts)
        vd, pd = lp.stp.get_state()
        ylog, ulog = lp.stp.feedback_log()
        # host: g_s = dt fv + dt/2 B (u_n + u_c) per step, as a table
        us = np.vstack([uc0.reshape((1, -1)), ulog])
        g0 = dt*toy_prob['rhsd']['fv'][:, 0]
        gtab = np.array([g0 + .5*dt*(lp.B @ (us[s + 1] + us[s]))
                         for s in range(nst)])
        lh.stp.set_rhs_table(gtab, None)
        lh.stp.run(nst, lh.cf, lh.opts)
        vh, ph = lh.stp.get_state()
        ev = fs.mnorm(lp.M, vd - vh)/fs.mnorm(lp.M, vh)
        ep = np.linalg.norm(pd - ph)/np.linalg.norm(ph)
        print('resident feedback vs tabulated on the host: v', ev, 'p', ep)
        assert ev <= VTOL and ep <= PTOL
        # and the feedback acts
        lo = ToyLoop(toy_prob)
        try:
            lo.stp.run(nst, lo.cf, lo.opts)
            vo, _ = lo.stp.get_state()
        finally:
            lo.close()
        assert fs.mnorm(lp.M, vd - vo) >= 1e-5*fs.mnorm(lp.M, vo)
    finally:
        lp.close()
        lh.close()


# ---- 9. loud errors -----------------------------------------------------------

def test_set_feedback_limits_are_loud(gtiu, toy_prob):
    from dolfin_navier_scipy_amd import _capi
    lp = ToyLoop(toy_prob)
    try:
        stp, obs, dt = lp.stp, lp.obs, lp.dt
        NV = lp.C.shape[1]
        big = fs.observer(1, 3, 2, hN=129)
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_feedback(lp.C, lp.B, big['ha'], big['hb'], big['hc'],
                             c_n=.5, c_c=.5, dt=dt)
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        assert 'hN = 129' in str(exc.value)
        dense = sps.csr_matrix(np.ones((14, NV)))          # 18004 > 16384
        wide = fs.observer(1, 14, 2)
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_feedback(dense, lp.B, wide['ha'], wide['hb'], wide['hc'],
                             c_n=.5, c_c=.5, dt=dt)
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        assert 'non-zeros' in str(exc.value)
        for Ny, Nu in ((33, 2), (3, 33)):
            o = fs.observer(1, Ny, Nu)
            Cm = sps.csr_matrix((np.ones(Ny), (np.arange(Ny), np.arange(Ny))),
                                shape=(Ny, NV))
            Bm = sps.csr_matrix((np.ones(Nu), (np.arange(Nu), np.arange(Nu))),
                                shape=(NV, Nu))
            with pytest.raises(_capi.DnsError):
                stp.set_feedback(Cm, Bm, o['ha'], o['hb'], o['hc'], c_n=.5,
                                 c_c=.5, dt=dt)
        # no feedback set: its state cannot be asked for
        stp._fb_shape = (12, 3, 2)
        with pytest.raises(_capi.DnsError):
            stp.feedback_state()
        # ... and the stepper is still usable open loop, like an untouched one
        stp.run(12, lp.cf, lp.opts)
        lo = ToyLoop(toy_prob)
        try:
            lo.stp.run(12, lo.cf, lo.opts)
            assert np.array_equal(stp.get_state()[0], lo.stp.get_state()[0])
        finally:
            lo.close()
        # clear_feedback returns to the open loop as well
        stp.set_feedback(lp.C, lp.B, obs['ha'], obs['hb'], obs['hc'], c_n=.5,
                         c_c=.5, dt=dt)
        with pytest.raises(_capi.DnsError):       # no table yet
            stp.run(1, lp.cf, lp.opts)
        stp.clear_feedback()
        stp.run(3, lp.cf, lp.opts)
    finally:
        lp.close()


def test_set_feedback_on_a_row_partitioned_stepper_is_refused(gtiu, toy_prob):
    from dolfin_navier_scipy_amd import saddle, _capi, comm as dcomm
    M, A, J = (toy_prob['smc'][k] for k in 'MAJ')
    dt = 5e-3
    cm = dcomm.Comm.rccl(0, 1, 0, dcomm.rccl_unique_id())
    system = saddle.SaddleSystem((M + .5*dt*A).tocsr(), J)
    stp = None
    try:
        system.set_comm(cm)
        system.setup_precond(cheb_degree=6, schur='dense', fhat='explicit')
        stp = saddle.ImexStepper(system, (M - .5*dt*A).tocsr())
        C, B = fs.sensors_actuators(toy_prob['th'], toy_prob['invinds'], M)
        obs = fs.observer(1, 3, 2)
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_feedback(C, B, obs['ha'], obs['hb'], obs['hc'], c_n=.5,
                             c_c=.5, dt=dt)
        assert 'partitioned' in str(exc.value)
    finally:
        if stp is not None:
            stp.close()
        system.set_comm(None)
        system.close()
        cm.close()


# ---- full size: wake N=2, Re=100, dt=1/512 ----------------------------------

def wake_setup():
    from dolfin_navier_scipy_amd.fem import get_sysmats
    femp, sm, rhsd = get_sysmats(problem='cylinderwake', N=2, Re=100)
    th, inv = femp['V'], femp['invinds']
    M, A, J = sm['M'].tocsr(), sm['A'].tocsr(), sm['J'].tocsr()
    NP, NV = J.shape
    vp0 = saddle_oracle.solve_sadpnt_smw(amat=A, jmat=J, rhsv=rhsd['fv'],
                                         rhsp=rhsd['fp'])     # snu:903-907
    inivel, inip = vp0[:NV], -vp0[NV:]
    dbcinds, dbcvals = femp['dbcinds'], femp['dbcvals']

    def appnd(vvec, bcs):
        full = np.full((th.vdim, 1), np.nan)
        full[inv] = vvec
        full[dbcinds, 0] = dbcvals
        return full

    def f_vdp(vf):
        return -th.convection_vec(vf)[inv, :]

    def make_kw(rec, nts=256):
        return dict(trange=np.linspace(0, nts/512., nts + 1), inivel=inivel,
                    inip=inip, bcs_ini=[], M=M, A=A, J=J, f_vdp=f_vdp,
                    f_tdp=lambda t: rhsd['fv'], g_tdp=lambda t: rhsd['fp'],
                    scalep=-1., getbcs=lambda t, v, p, mode=None: [],
                    applybcs=lambda b: (0., 0., 0.), appndbcs=appnd,
                    savevp=rec, check_ff_maxv=1e8, verbose=False)
    C, B = fs.sensors_actuators(th, inv, M)
    obs = fs.observer(7, 3, 2, gain=1.0)
    return dict(femp=femp, M=M, A=A, J=J, rhsd=rhsd, inivel=inivel,
                make_kw=make_kw, f_vdp=f_vdp, appnd=appnd, C=C, B=B, obs=obs)


@pytest.fixture(scope='module')
def wake(gtiu):
    return wake_setup()


# ---- 7. full size against the oracle ----------------------------------------

def test_full_size_closed_loop_against_the_oracle(gtiu, wake):
    """256 steps from the Stokes state, resident, against `imex_oracle.cnab`
    with the host `LinearFeedback`; gain 1 (observer seed 7): `ffflag` 0 and
    the closed loop ends 6.8e-3 (v) / 2.0e-2 (p) away from the open loop on
    the CPU"""
    from dolfin_navier_scipy_amd import convection
    femp, M, obs = wake['femp'], wake['M'], wake['obs']

    def feedback():
        return gtiu.LinearFeedback(wake['C'], wake['B'], obs['ha'], obs['hb'],
                                   obs['hc'], obs['inihx'],
                                   drift=fs.drift_of(obs['dvec']))
    vopen, popen, ffo = imex_oracle.cnab(
        **wake['make_kw'](scenarios.Recorder()))
    fbo, memo = feedback(), {}
    vo, po, ffc = imex_oracle.cnab(dynamic_rhs=fbo, dynamic_rhs_memory=memo,
                                   **wake['make_kw'](scenarios.Recorder()))
    assert ffo == 0 and ffc == 0
    acts = fs.mnorm(M, vo - vopen)/fs.mnorm(M, vopen)
    print('closed vs open loop (oracle): v', acts)
    assert acts >= 1e-6
    cvop = convection.ConvectionP2.from_taylor_hood(
        femp['V'], femp['invinds'], femp['dbcinds'], femp['dbcvals'])
    fbg, memg = feedback(), {}
    kw = wake['make_kw'](scenarios.Recorder())
    kw.pop('f_vdp')
    try:
        vg, pg, ff = gtiu.cnab(dynamic_rhs=fbg, dynamic_rhs_memory=memg,
                               device_convection=cvop,
                               invinds=femp['invinds'],
                               resident=dict(savevp_times=[]), **kw)
    finally:
        cvop.close()
    assert ff == 0
    assert gtiu.LAST_RUN['feedback'] == 'resident'
    assert fbg.calls['abtwo'] == 0
    ev = fs.mnorm(M, vg - vo)/fs.mnorm(M, vo)
    ep = np.linalg.norm(pg - po)/np.linalg.norm(po)
    print('full size, resident vs oracle: v', ev, 'p', ep)
    assert ev <= VTOL, ev
    assert ep <= PTOL, ep
    assert _rel(memg['lasthx'], memo['lasthx']) <= 1e-8
    uo = np.array([h[3] for h in fbo.history if h[1] == 'abtwo'])
    assert _rel(gtiu.LAST_RUN['feedback_u'], uo) <= 1e-8


# ---- 6. batches and replay ----------------------------------------------------

class WakeLoop(object):
    """the bench configuration (bench.py's solver defaults) with feedback, a
    tabulated forcing that jumps at step JUMP_AT and a drift table that jumps
    there too"""

    def __init__(self, wake, nst=256, feedback=True):
        import bench
        from dolfin_navier_scipy_amd import saddle, convection
        femp, M, A, J, rhsd = (wake['femp'], wake['M'], wake['A'], wake['J'],
                               wake['rhsd'])
        dt = 1./512
        dflt = bench.DEFAULTS
        self.system = saddle.SaddleSystem((M + .5*dt*A).tocsr(), J)
        self.system.setup_precond(cheb_degree=dflt['cheb'], schur='dense',
                                  fp32_store=bool(dflt['fp32']),
                                  drop_tol=dflt['drop'],
                                  factorization=dflt['fact'])
        self.stp = saddle.ImexStepper(self.system, (M - .5*dt*A).tocsr())
        self.cvop = convection.ConvectionP2.from_taylor_hood(
            femp['V'], femp['invinds'], femp['dbcinds'], femp['dbcvals'])
        v0 = wake['inivel']
        nfc0 = wake['f_vdp'](wake['appnd'](v0, []))
        self.stp.set_state(v0, nfc_c=nfc0, nfc_o=nfc0)
        self.stp.set_convection(self.cvop, scale=-1.0)
        self.cf = saddle.ImexStepper.coeffs(
            a_c=1., cn_c=1.5*dt, cn_o=-.5*dt, pscale=-1./dt,
            extrapolate=dflt['extrap'], carry_residual=True)
        self.opts = saddle.solve_opts(method='gmres', rtol=dflt['rtol'],
                                      maxiter=400, restart=60, check_every=2,
                                      use_graph=True, reorth=dflt['reorth'])
        g0 = dt*rhsd['fv'][:, 0]
        bump = np.asarray(wake['B'][:, [0]].todense())[:, 0]
        gtab = np.tile(g0, (nst, 1))
        gtab[JUMP_AT:] += dt*JUMP_G*bump
        gptab = np.tile(rhsd['fp'][:, 0], (nst, 1))
        self.stp.set_rhs_table(gtab, gptab)
        if feedback:
            obs = wake['obs']
            drift = np.zeros((nst, 12))
            drift[JUMP_AT:] = JUMP_D*obs['dvec'][:, 0]
            self.stp.set_feedback(wake['C'], wake['B'], obs['ha'], obs['hb'],
                                  obs['hc'], c_n=.5, c_c=.5, dt=dt)
            self.stp.set_feedback_state(obs['inihx'], np.zeros(12),
                                        obs['hc'] @ obs['inihx'])
            self.stp.set_feedback_table(nst, drift)
        self.record = dict(unconverged=0, replayed=0, lazy_steps=0,
                           eager_steps=0)

    def run(self, n):
        self.stp.run(n, self.cf, self.opts)
        for k in self.record:
            self.record[k] += int(self.stp.last_run[k])

    def close(self):
        self.stp.close()
        self.cvop.close()
        self.system.close()


def test_batches_and_a_restored_batch_reproduce_the_single_steps(gtiu, wake):
    """256 closed-loop steps on the bench system as ONE `run(256)` and as 256
    `run(1)`; at step 128 the tabulated forcing and the drift level jump, the
    warm start of that step is poor, the predicted cycle too short, and
    `dns_imex_run` restores the batch from its checkpoint and repeats it:
    observer state, slot parity and log rows come back with it.

    Observed on the MI355X when the jump was sized: without a jump nothing is
    replayed (closed and open loop); JUMP_G = 5, JUMP_D = 5 -- `replayed` 32,
    the batch of 32 steps that starts at step 124 ("attempt 1: c=3"), |v| stays
    at 56.3; the same jump of the forcing alone replays the same batch of the
    open loop (32), and so does the drift jump alone (32).  JUMP_G = 50 also
    replays (128) but drives the flow to a breakdown by step ~220, where
    trajectories stop being comparable -- not used.  `replayed` of the batched
    run is asserted, so the test cannot pass without a restore."""
    M = wake['M']
    nst = 256
    runs = []
    for mode in ('batched', 'batched', 'single'):
        lp = WakeLoop(wake, nst)
        try:
            if mode == 'batched':
                lp.run(nst)
            else:
                for _ in range(nst):
                    lp.run(1)
            v, p = lp.stp.get_state()
            ylog, ulog = lp.stp.feedback_log()
            runs.append(dict(v=v, p=p, y=ylog, u=ulog,
                             state=lp.stp.feedback_state(),
                             record=dict(lp.record)))
        finally:
            lp.close()
    a, a2, b = runs
    print('batched run:', a['record'], ' single steps:', b['record'])
    assert a['record']['unconverged'] == 0
    assert a['record']['replayed'] >= 1, a['record']
    ev = fs.mnorm(M, a['v'] - b['v'])/fs.mnorm(M, b['v'])
    ep = np.linalg.norm(a['p'] - b['p'])/np.linalg.norm(b['p'])
    print('batched vs single steps: v', ev, 'p', ep, 'y',
          _rel(a['y'], b['y']), 'u', _rel(a['u'], b['u']))
    assert ev <= 1e-8 and ep <= 1e-8
    assert a['y'].shape == (nst, 3) and a['u'].shape == (nst, 2)
    assert _rel(a['y'], b['y']) <= 1e-8
    assert _rel(a['u'], b['u']) <= 1e-8
    for x, y in zip(a['state'], b['state']):
        assert _rel(x, y) <= 1e-8
    # the jump arrives in the logs where it was put
    assert np.abs(a['u'][JUMP_AT + 4] - a['u'][JUMP_AT - 1]).max() > \
        10*np.abs(a['u'][JUMP_AT - 1] - a['u'][JUMP_AT - 5]).max()
    # the same run twice: fixed summation orders, the same kernels
    assert a2['record'] == a['record']
    assert np.array_equal(a['y'], a2['y'])
    assert np.array_equal(a['u'], a2['u'])
    for x, y in zip(a['state'], a2['state']):
        assert np.array_equal(x, y)
    assert np.array_equal(a['v'], a2['v'])


# ---- 8. solve_nse -------------------------------------------------------------

def test_solve_nse_with_dynamic_feedback_runs_resident(gtiu):
    """`solve_nse(closed_loop=True, dynamic_feedback=True, dyn_fb_disc='AB2')`
    on `karman2D-rotcyl_lvl1` (set up as `test_gpu_snu.py` does): the list of
    outputs against `imex_oracle.cnab` with the closures written out here and
    the host `LinearFeedback`"""
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    from dolfin_navier_scipy_amd.fem import get_sysmats
    femp, sm, rhsd = get_sysmats(
        problem='gen_bccont', nu=1e-3, charvel=0.2, bccontrol=False,
        meshparams=dict(meshname='karman2D-rotcyl_lvl1',
                        geodata='karman2D-rotcyl-bm_geo_cntrlbc'))
    M, A, J = sm['M'].tocsr(), sm['A'].tocsr(), sm['J'].tocsr()
    NP, NV = J.shape
    fv, fp = rhsd['fv'], rhsd['fp']
    th, inv = femp['V'], femp['invinds']
    dbcinds, dbcvals = femp['dbcinds'], femp['dbcvals']
    C, B = fs.sensors_actuators(th, inv, M)
    assert C.nnz <= 16384
    obs = fs.observer(9, 3, 2, gain=1.0)
    drift = fs.drift_of(obs['dvec'])
    t0, tE, Nts = 0.0, 0.05, 24
    trange = np.linspace(t0, tE, Nts + 1)

    # the oracle: Stokes start (snu:903-907), static boundary values
    vp0 = saddle_oracle.solve_sadpnt_smw(amat=A, jmat=J, rhsv=fv, rhsp=fp)
    iniv = vp0[:NV]

    def appnd(vvec, bcs):
        full = np.full((th.vdim, 1), np.nan)
        full[inv] = vvec
        full[dbcinds, 0] = dbcvals
        return full
    ylist_o = []

    def save(vfull, pvec, time=None):
        ylist_o.append(C @ vfull[inv])
    fbo = gtiu.LinearFeedback(C, B, obs['ha'], obs['hb'], obs['hc'],
                              obs['inihx'], drift=drift)
    kwo = dict(trange=trange, inivel=iniv, inip=np.zeros((NP, 1)), bcs_ini=[],
               M=M, A=A, J=J,
               f_vdp=lambda vf: -th.convection_vec(vf)[inv, :],
               f_tdp=lambda t: fv, g_tdp=lambda t: fp, scalep=-1.,
               getbcs=lambda t, v, p, mode=None: [],
               applybcs=lambda b: (0., 0., 0.), appndbcs=appnd, savevp=save,
               check_ff_maxv=1e8, verbose=False)
    vo, po, ffo = imex_oracle.cnab(dynamic_rhs=fbo, dynamic_rhs_memory={},
                                   **kwo)
    yopen = []
    kwo.update(savevp=lambda vfull, pvec, time=None: yopen.append(
        C @ vfull[inv]))
    imex_oracle.cnab(**kwo)
    assert ffo == 0
    ylist = snu.solve_nse(
        A=A, M=M, J=J, fv=fv, fp=fp, V=th, invinds=inv,
        dbcinds=dbcinds.tolist(), dbcvals=dbcvals.tolist(), trange=trange,
        treat_nonl_explicit=True, start_ssstokes=True,
        closed_loop=True, dynamic_feedback=True, dyn_fb_disc='AB2',
        dyn_fb_dict=dict(ha=obs['ha'], hb=obs['hb'], hc=obs['hc'],
                         inihx=obs['inihx'], drift=drift),
        b_mat=B, cv_mat=C, return_y_list=True, solver=dict(rtol=1e-13))
    assert gtiu.LAST_RUN['feedback'] == 'resident'
    assert len(ylist) == len(ylist_o) == Nts + 1
    scale = max(np.abs(y).max() for y in ylist_o)
    worst = max(np.abs(g - o).max() for g, o in zip(ylist, ylist_o))/scale
    acts = max(np.abs(c - o).max() for c, o in zip(ylist_o, yopen))/scale
    print('solve_nse, dynamic feedback: outputs', worst,
          '(closed vs open loop:', acts, ')')
    assert acts >= 1e-6
    for k, (g, o) in enumerate(zip(ylist, ylist_o)):
        assert np.abs(g - o).max() <= 1e-8*np.abs(o).max(), k
