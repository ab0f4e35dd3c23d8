"""`SaddleSystem.probe` (`dns_saddle_probe`) launches the nodes of the Krylov
cycle through the launchers the solve uses (`csrc/cycle_nodes.inc`), with
arguments of its own: column 3, scratch vectors, a control header in which
nothing converges.  Nothing else in the suite runs that path.

Per form of `krylov_ld_model.FORMS` (the toy problem, NV 1286, NP 207; one
Schur kind each: SK 0, 1, 2, 3), on a fresh handle since the probe overwrites
the control header: every name of `SaddleSystem.PROBES` and the pair code
`1000 + 10*0 + 2` (head, then K apply with the dots) returns a finite, positive
time per launch -- no time is asserted --, and a plain solve on the same handle
behind them converges to what `test_gpu_saddle.py` asks of that Schur block
(`rtol` 1e-12 and a true residual of 5e-12; multigrid: 1e-11 and 2e-11).
"""
import numpy as np
import pytest

import krylov_ld_model as kl
from test_gpu_precond_forms import make_system

pytestmark = pytest.mark.gpu

PAIR_HEAD_KAPPLY = 1000 + 10*0 + 2


@pytest.fixture(scope='module')
def bench(toy_prob):
    from dolfin_navier_scipy_amd import _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    return kl.toy_bench(toy_prob)


@pytest.mark.parametrize('form', list(kl.FORMS))
def test_probes_then_solve(bench, form):
    from dolfin_navier_scipy_amd import saddle
    system = make_system(saddle, bench,
                         dict(kl.FORMS[form], **kl.REGIMES['latency']))
    for which in saddle.SaddleSystem.PROBES + (PAIR_HEAD_KAPPLY,):
        us = system.probe(which, chain=2, reps=2)
        print('%-4s %-16s %.2f us' % (form, which, us))
        assert np.isfinite(us) and us > 0., (which, us)
    b = kl.right_hand_sides(bench)['time-step']
    mg = kl.FORMS[form]['schur'] == 'mg'
    kw = dict(rtol=1e-11, maxiter=400) if mg else dict(rtol=1e-12, maxiter=3000)
    x = system.solve(b[:bench.NV], b[bench.NV:], **kw)
    st = system.last_stats
    assert np.isfinite(x).all()
    assert st['status'] == 0, st
    assert st['true_relres'] <= (2e-11 if mg else 5e-12), st
    system.close()
