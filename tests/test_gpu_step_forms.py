"""The forms of the resident CNAB step (`dns_imex::plan`)
agree: six-node lazy and eager, seven-node with the front kernel in MODE 2
(residual carry-over) and MODE 1, synchronous steps, the streamed right-hand
side -- each against the CPU oracle's CNAB loop.

Problem: `scenarios.toy_problem()` at its defaults, the Heun step of the oracle
and 24 resident steps behind it (start-up steps, then pipelined batches with a
full ring).  Solver options and tolerances are those of
`test_gpu_imex.py::test_pipelined_run_warm_start_orders` (full factorisation:
the six-node step needs J Fh^-1).  The knobs are read once, when the system
and the stepper are created.

No leg may replay a batch: a replay is the batch policy's answer to solves that
need more Krylov steps than the ones before them, i.e. to a transient.  So the
run starts, like that test, from the steady Stokes state (smooth, discretely
divergence free) and takes steps of dt = 2e-4, short enough for the quartic
warm start to stand within a column or two of the tolerance from the first
batch on; then the six-node leg also runs the lazy one-column cycle.
"""
import numpy as np
import pytest

import scenarios
from oracle import imex_oracle, saddle_oracle

pytestmark = pytest.mark.gpu

VTOL, PTOL = 1e-8, 1e-8
NRES = 24                      # resident steps behind the Heun step
DT = 2e-4


@pytest.fixture(scope='module')
def toy(toy_prob):
    """the oracle's trajectory (computed once) and the state behind its Heun
    step, from which the resident steps go on"""
    from dolfin_navier_scipy_amd import _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    kw, rec, aux = scenarios.build(variant='plain', Nts=NRES + 1,
                                   tE=DT*(NRES + 1), prob=toy_prob)
    NP, NV = kw['J'].shape
    vp0 = saddle_oracle.solve_sadpnt_smw(amat=kw['A'], jmat=kw['J'],
                                         rhsv=aux['cfv'], rhsp=aux['cfp'])
    kw['inivel'], kw['inip'] = vp0[:NV], -vp0[NV:]
    imex_oracle.cnab(**kw)
    _, vso, pso = rec.arrays()
    dt = kw['trange'][1] - kw['trange'][0]
    (v1, p1, _, _, _, _, _, nfc0, _, _, _) = imex_oracle.heun_start(
        vc=kw['inivel'], pc=kw['inip'], tc=0., tn=dt, M=kw['M'], A=kw['A'],
        J=kw['J'], scalep=-1., dfv_c=0.,
        dynamic_rhs=lambda t, vc=None, memory={}, mode=None: (
            np.zeros_like(kw['inivel']), memory), drm={}, bcs_c=[],
        applybcs=kw['applybcs'], appndbcs=kw['appndbcs'], getbcs=kw['getbcs'],
        f_tdp=kw['f_tdp'], f_vdp=kw['f_vdp'], g_tdp=kw['g_tdp'])
    inv = toy_prob['invinds']
    return dict(prob=toy_prob, kw=kw, dt=dt, v1=v1, p1=p1, nfc0=nfc0,
                vref=vso[NRES + 1][inv].reshape((-1, 1)),
                pref=pso[NRES + 1].reshape((-1, 1)))


def _run(toy, carry=True, lazy=None, graph=True):
    """24 resident steps; returns the errors against the oracle and the
    record of the run calls"""
    from dolfin_navier_scipy_amd import saddle, convection
    prob, kw, dt = toy['prob'], toy['kw'], toy['dt']
    M, A, J = kw['M'], kw['A'], kw['J']
    system = saddle.SaddleSystem((M + .5*dt*A).tocsr(), J)
    if lazy is not None:
        system.set_option('step6_lazy', int(lazy))
    system.setup_precond(cheb_degree=4, schur='dense', factorization='full')
    stp = saddle.ImexStepper(system, (M - .5*dt*A).tocsr())
    stp.set_state(toy['v1'], ptilde_c=-dt*toy['p1'], nfc_c=toy['nfc0'])
    stp.set_rhs(dt*kw['f_tdp'](0.), kw['g_tdp'](0.))
    cvop = convection.ConvectionP2.from_taylor_hood(
        prob['th'], prob['invinds'], prob['dbcinds'], prob['dbcvals'])
    stp.set_convection(cvop, scale=-1.0)
    cf = saddle.ImexStepper.coeffs(a_c=1., cn_c=1.5*dt, cn_o=-.5*dt,
                                   pscale=-1./dt, extrapolate=4,
                                   carry_residual=carry)
    opts = saddle.solve_opts(rtol=1e-12, maxiter=300, restart=60,
                             use_graph=graph, reorth=2)
    record = dict(unconverged=0, replayed=0, lazy_steps=0, eager_steps=0)
    for n in (8, NRES - 8):
        _, _, last = stp.run(n, cf, opts)
        assert last['status'] == 0, last
        for k in record:
            record[k] += int(stp.last_run[k])
    vg, pg = stp.get_state()
    stp.close()
    cvop.close()
    system.close()
    mnorm = lambda x: np.sqrt((x.T @ (M @ x)).item())
    ev = mnorm(np.asarray(vg).reshape((-1, 1)) - toy['vref'])/mnorm(toy['vref'])
    ep = (np.linalg.norm(np.asarray(pg).reshape((-1, 1)) - toy['pref']) /
          np.linalg.norm(toy['pref']))
    return ev, ep, record


def _check(name, ev, ep, record):
    print(name, 'v', ev, 'p', ep, record)
    assert record['unconverged'] == 0 and record['replayed'] == 0, record
    assert ev <= VTOL, ev
    assert ep <= PTOL, ep


def test_six_node_lazy_step(toy):
    ev, ep, rec = _run(toy)
    _check('six-node', ev, ep, rec)
    assert rec['lazy_steps'] + rec['eager_steps'] > 0, rec


def test_six_node_eager_step(toy):
    ev, ep, rec = _run(toy, lazy=0)
    _check('six-node eager', ev, ep, rec)
    assert rec['lazy_steps'] == 0 and rec['eager_steps'] > 0, rec


@pytest.mark.parametrize('carry', [True, False])
def test_seven_node_step(toy, monkeypatch, carry):
    """DNS_STEP6=0: the front kernel in MODE 2 (carry) / MODE 1"""
    monkeypatch.setenv('DNS_STEP6', '0')
    ev, ep, rec = _run(toy, carry=carry)
    _check('seven-node, carry %d' % carry, ev, ep, rec)
    assert rec['lazy_steps'] == 0 and rec['eager_steps'] == 0, rec


def test_synchronous_steps(toy):
    ev, ep, rec = _run(toy, graph=False)
    _check('synchronous', ev, ep, rec)
    assert rec['lazy_steps'] == 0 and rec['eager_steps'] == 0, rec


def test_streamed_rhs(toy, monkeypatch):
    monkeypatch.setenv('DNS_STREAM_NNZ', '1')
    ev, ep, rec = _run(toy)
    _check('streamed right-hand side', ev, ep, rec)
