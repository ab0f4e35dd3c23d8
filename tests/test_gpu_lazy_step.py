"""The lazy one-column cycle of the six-node resident step (`step6_lazy`,
DESIGN section 4): the head scales nothing and reduces nothing, the tail forms
the minimal-residual step from <r, K z>, <K z, K z> and ||r||^2.

Configuration and tolerances are those of `test_gpu_long_horizon.py`: cylinder
wake N=2, Re=80, Nts=512, velocities in the M-norm and pressures 1e-8 against
the CPU oracle's factor-once CNAB loop; the resident loop is driven as
`bench.py` drives it (its solver defaults, residual carry-over on).
"""
import numpy as np
import pytest

import scenarios
from oracle import imex_oracle, saddle_oracle

pytestmark = pytest.mark.gpu

VTOL, PTOL = 1e-8, 1e-8
NTS = 512
EPS = np.finfo(np.float64).eps
# The residual norm behind the one column is rho sqrt(d), d = 1 - cos^2, in
# both kinds of cycle (eager: Pythagoras on <w,w> - h^2), and both refuse a
# d <= GUARD (k_arn_tail6, pythagoras_norm).  An absolute rounding error
# gamma in d is a relative error gamma / (2 d) in the norm.  gamma: the three
# sums of 1e4 terms are formed in different orders by the two cycles (block
# and wave trees over short serial runs: at most 28 eps each relative, 2 x 3 of
# them enter cos^2 <= 1) plus the four operations of the formula on each side.
GUARD = 1e-8
GAMMA = 2*(3*28 + 4)*EPS
RELRES_BOUND = GAMMA/(2*GUARD)


@pytest.fixture(scope='module')
def wake():
    from dolfin_navier_scipy_amd.fem import get_sysmats
    from dolfin_navier_scipy_amd import _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    femp, sm, rhsd = get_sysmats(problem='cylinderwake', N=2, Re=80)
    th, inv = femp['V'], femp['invinds']
    M, A, J = sm['M'], sm['A'], sm['J']
    NP, NV = J.shape
    vp0 = saddle_oracle.solve_sadpnt_smw(amat=A, jmat=J, rhsv=rhsd['fv'],
                                         rhsp=rhsd['fp'])
    inivel, inip = vp0[:NV], -vp0[NV:]
    dbcinds, dbcvals = femp['dbcinds'], femp['dbcvals']

    def appnd(vvec, bcs):
        full = np.full((th.vdim, 1), np.nan)
        full[inv] = vvec
        full[dbcinds, 0] = dbcvals
        return full

    def f_vdp(vf):
        return -th.convection_vec(vf)[inv, :]

    kw = dict(trange=np.linspace(0, 1., NTS + 1), inivel=inivel, inip=inip,
              bcs_ini=[], M=M, A=A, J=J, f_vdp=f_vdp,
              f_tdp=lambda t: rhsd['fv'], g_tdp=lambda t: rhsd['fp'],
              scalep=-1., getbcs=lambda t, v, p, mode=None: [],
              applybcs=lambda b: (0., 0., 0.), appndbcs=appnd,
              check_ff_maxv=1e8, verbose=False)
    ro = scenarios.Recorder()
    vo, po, _ = imex_oracle.cnab(savevp=ro, **kw)
    dt = 1./NTS
    # the Heun start of the oracle (one step): the resident steps follow it
    (v1, p1, _, _, _, _, _, nfc0, _, _, _) = imex_oracle.heun_start(
        vc=inivel, pc=inip, tc=0., tn=dt, M=M, A=A, J=J, scalep=-1., dfv_c=0.,
        dynamic_rhs=lambda t, vc=None, memory={}, mode=None: (
            np.zeros_like(inivel), memory), drm={}, bcs_c=[],
        applybcs=kw['applybcs'], appndbcs=appnd, getbcs=kw['getbcs'],
        f_tdp=kw['f_tdp'], f_vdp=f_vdp, g_tdp=kw['g_tdp'])
    _, vso, pso = ro.arrays()
    return dict(femp=femp, sm=sm, rhsd=rhsd, vo=vo, po=po, vso=vso, pso=pso,
                v1=v1, p1=p1, nfc0=nfc0, dt=dt)


def _mnorm(M, x):
    x = np.asarray(x).reshape((-1, 1))
    return float(np.sqrt((x.T @ (M @ x)).item()))


class Resident(object):
    """system + stepper behind the oracle's Heun step, bench.py's settings"""

    def __init__(self, wake, lazy, restart=60, zero=False):
        import bench
        from dolfin_navier_scipy_amd import saddle, convection
        femp, sm, rhsd, dt = wake['femp'], wake['sm'], wake['rhsd'], wake['dt']
        M, A, J = sm['M'], sm['A'], sm['J']
        dflt = bench.DEFAULTS
        self.system = saddle.SaddleSystem((M + .5*dt*A).tocsr(), J)
        self.system.set_option('step6_lazy', int(lazy))
        self.system.setup_precond(cheb_degree=dflt['cheb'], schur='dense',
                                  fp32_store=bool(dflt['fp32']),
                                  drop_tol=dflt['drop'],
                                  factorization=dflt['fact'])
        self.stp = saddle.ImexStepper(self.system, (M - .5*dt*A).tocsr())
        self.cvop = None
        NP, NV = J.shape
        if zero:
            self.stp.set_state(np.zeros((NV, 1)), ptilde_c=np.zeros((NP, 1)),
                               nfc_c=np.zeros((NV, 1)))
            self.stp.set_rhs(np.zeros((NV, 1)), np.zeros((NP, 1)))
        else:
            self.stp.set_state(wake['v1'], ptilde_c=-dt*wake['p1'],
                               nfc_c=wake['nfc0'])
            self.stp.set_rhs(dt*rhsd['fv'], rhsd['fp'])
            self.cvop = convection.ConvectionP2.from_taylor_hood(
                femp['V'], femp['invinds'], femp['dbcinds'], femp['dbcvals'])
            self.stp.set_convection(self.cvop, scale=-1.0)
        self.cf = saddle.ImexStepper.coeffs(
            a_c=1., cn_c=1.5*dt, cn_o=-.5*dt, pscale=-1./dt,
            extrapolate=dflt['extrap'], carry_residual=True)
        self.opts = saddle.solve_opts(method='gmres', rtol=dflt['rtol'],
                                      maxiter=400, restart=restart,
                                      check_every=2, use_graph=True,
                                      reorth=dflt['reorth'])
        self.iters = 0
        self.record = dict(unconverged=0, replayed=0, lazy_steps=0,
                           eager_steps=0)

    def run(self, n):
        _, its, last = self.stp.run(n, self.cf, self.opts)
        self.iters += int(its)
        for k in self.record:
            self.record[k] += int(self.stp.last_run[k])
        return last

    def state(self):
        return self.stp.get_state()

    def close(self):
        self.stp.close()
        if self.cvop is not None:
            self.cvop.close()
        self.system.close()


def _errors(wake, vg, pg, k=NTS):
    M, inv = wake['sm']['M'], wake['femp']['invinds']
    vref = wake['vso'][k][inv].reshape((-1, 1))
    pref = wake['pso'][k].reshape((-1, 1))
    ev = _mnorm(M, np.asarray(vg).reshape((-1, 1)) - vref)/_mnorm(M, vref)
    ep = (np.linalg.norm(np.asarray(pg).reshape((-1, 1)) - pref) /
          np.linalg.norm(pref))
    return ev, ep


@pytest.fixture(scope='module')
def runs(wake):
    """the 511 resident steps behind the Heun step, switch on and off"""
    out = {}
    for lazy in (1, 0):
        r = Resident(wake, lazy)
        for n in (5, 20, NTS - 1 - 25):
            r.run(n)
        vg, pg = r.state()
        out[lazy] = dict(v=vg, p=pg, iters=r.iters, record=dict(r.record))
        r.close()
        print('switch', lazy, 'iters', r.iters, r.record)
    return out


def test_lazy_512_steps_against_oracle(wake, runs):
    ev, ep = _errors(wake, runs[1]['v'], runs[1]['p'])
    print('lazy 512 steps: v', ev, 'p', ep, runs[1]['record'])
    assert runs[1]['record']['lazy_steps'] > 0, runs[1]['record']
    assert ev <= VTOL, ev
    assert ep <= PTOL, ep


def test_switch_off_same_counts(wake, runs):
    ev, ep = _errors(wake, runs[0]['v'], runs[0]['p'])
    print('eager 512 steps: v', ev, 'p', ep, runs[0]['record'])
    assert ev <= VTOL, ev
    assert ep <= PTOL, ep
    assert runs[0]['record']['lazy_steps'] == 0, runs[0]['record']
    assert runs[0]['iters'] == runs[1]['iters'], (runs[0]['iters'],
                                                  runs[1]['iters'])
    for k in ('replayed', 'unconverged'):
        assert runs[0]['record'][k] == runs[1]['record'][k], (k, runs)


def test_impulsive_start_runs_both_kinds_of_cycle(wake):
    """right behind the impulsive start the solves need two columns: the
    batches run the general cycle and come back to the lazy one"""
    nres = 95
    r = Resident(wake, 1)
    r.run(nres)
    vg, pg = r.state()
    rec = dict(r.record)
    r.close()
    ev, ep = _errors(wake, vg, pg, k=nres + 1)
    print('impulsive start,', nres, 'steps: v', ev, 'p', ep, rec)
    assert rec['eager_steps'] > 0 and rec['lazy_steps'] > 0, rec
    assert ev <= VTOL, ev
    assert ep <= PTOL, ep


def test_zero_rhs_zero_state(wake):
    """r = 0 (and with it w = 0) takes no step and is converged, not NaN"""
    r = Resident(wake, 1, restart=1, zero=True)   # (restart 1: cycles of one)
    last = r.run(24)
    vg, pg = r.state()
    rec = dict(r.record)
    r.close()
    print('zero problem:', last, rec)
    assert rec['lazy_steps'] > 0, rec
    assert rec['unconverged'] == 0 and last['status'] == 0, (rec, last)
    assert np.all(np.isfinite(vg)) and np.all(np.isfinite(pg))
    assert not np.any(vg) and not np.any(pg)
    assert np.isfinite(last['est_relres']) and last['iters'] == 0, last


def test_stats_of_a_lazy_step_match_the_eager_step(wake):
    """one step from the SAME state (64 identical steps with the switch off
    in front), lazy and eager: `bnorm` and the iteration count are equal,
    `est_relres` agrees within the bound of the cancellation guard"""
    last = {}
    for lazy in (1, 0):
        r = Resident(wake, 0)
        r.run(64)
        r.system.set_option('step6_lazy', lazy)
        r.record = dict.fromkeys(r.record, 0)
        last[lazy] = dict(r.run(1))
        last[lazy]['record'] = dict(r.record)
        r.close()
    print('one step, lazy:', last[1], 'eager:', last[0])
    assert last[1]['record']['lazy_steps'] == 1, last[1]
    assert last[0]['record']['eager_steps'] == 1, last[0]
    assert last[1]['iters'] == last[0]['iters'] == 1, last
    assert last[1]['status'] == last[0]['status'] == 0, last
    # (||b||: the same 42 partials of the same kernel, summed by the same
    # tree in both tails)
    assert last[1]['bnorm'] == last[0]['bnorm'], last
    rel = abs(last[1]['est_relres'] - last[0]['est_relres']) / \
        last[0]['est_relres']
    print('est_relres: relative difference', rel, 'bound', RELRES_BOUND)
    assert rel <= RELRES_BOUND, (rel, RELRES_BOUND)


def test_lazy_runs_are_bitwise_reproducible(wake):
    states = []
    for _ in range(2):
        r = Resident(wake, 1)
        r.run(5)
        r.run(123)
        states.append(r.state())
        assert r.record['lazy_steps'] > 0, r.record
        r.close()
    assert np.array_equal(states[0][0], states[1][0])
    assert np.array_equal(states[0][1], states[1][1])
