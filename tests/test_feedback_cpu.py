"""Observer feedback (`time_int_utils.LinearFeedback`), host side: the
restatement of the reference's `get_heunab_lti` (tiu:148-196) composed with
`cv_mat` / `b_mat` as in snu:1243-1247 reproduces what the REFERENCE's own
`cnab` / `sbdftwo` computed with the reference's own observer
(`tests/golden/make_golden_feedback.py`), the keywords of `solve_nse`, and
the C-ABI of the device form."""
import os
import re

import numpy as np
import pytest

import feedback_setup as fs
import scenarios
from oracle import imex_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ('init', 'heunpred', 'heuncorr', 'abtwo')
NEW_SYMBOLS = ('dns_imex_set_feedback', 'dns_imex_set_feedback_state',
               'dns_imex_get_feedback_state', 'dns_imex_set_feedback_table',
               'dns_imex_get_feedback_log', 'dns_imex_clear_feedback')


def golden_feedback(golden_dir, scheme):
    from dolfin_navier_scipy_amd import time_int_utils as gtiu
    gold = np.load(os.path.join(
        golden_dir, 'imex_{0}_feedback_s5.npz'.format(scheme)))
    fb = gtiu.LinearFeedback(fs.csr_unpack(gold, 'C'),
                             fs.csr_unpack(gold, 'B'), gold['ha'], gold['hb'],
                             gold['hc'], gold['inihx'],
                             drift=fs.drift_of(gold['dvec']))
    return gold, fb


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max()/np.abs(b).max()


@pytest.mark.parametrize('scheme', ('cnab', 'sbdf2'))
def test_linear_feedback_reproduces_the_reference(golden_dir, toy_prob,
                                                  scheme):
    """trajectories, the `(t, mode, y)` / `u` sequence of the callback and the
    final observer memory to 1e-10 relative (the bound of
    `test_oracle_golden.py`)"""
    gold, fb = golden_feedback(golden_dir, scheme)
    kw, rec, _ = scenarios.build(variant='plain', seed=5, Nts=48, tE=0.24,
                                 prob=toy_prob)
    assert np.array_equal(kw['inivel'], gold['inivel'])
    # the fixture's matrices are the builder's
    cv_mat, b_mat = fs.sensors_actuators(toy_prob['th'], toy_prob['invinds'],
                                         toy_prob['smc']['M'])
    assert abs(cv_mat - fb.cv_mat).max() < 1e-15
    assert abs(b_mat - fb.b_mat).max() < 1e-15
    # the recorded drift rows are the drift the test hands over
    assert np.array_equal(
        gold['drift_rows'],
        np.array([fb.drift(t)[:, 0] for t in gold['trange']]))
    mem = {}
    kw.update(dynamic_rhs=fb, dynamic_rhs_memory=mem)
    integ = imex_oracle.cnab if scheme == 'cnab' else imex_oracle.sbdftwo
    v, p, ff = integ(**kw)
    times, vels, prss = rec.arrays()
    assert ff == int(gold['ffflag']) == 0
    assert times.size == 49
    assert np.allclose(times, gold['times'], rtol=0, atol=1e-15)
    for got, want in ((vels, gold['vels']), (prss, gold['prss']),
                      (v, gold['vfinal']), (p, gold['pfinal'])):
        assert rel(got, want) <= 1e-10, rel(got, want)
    # what the callback saw and returned, call by call
    assert len(fb.history) == gold['cb_t'].size == 50
    assert fb.calls == dict(init=1, heunpred=1, heuncorr=1, abtwo=47)
    assert [MODES.index(h[1]) for h in fb.history] == gold['cb_mode'].tolist()
    assert np.allclose([h[0] for h in fb.history], gold['cb_t'], rtol=0,
                       atol=1e-15)
    ys = np.array([h[2] for h in fb.history[1:]])
    us = np.array([h[3] for h in fb.history])
    assert rel(ys, gold['cb_y'][1:]) <= 1e-10
    assert rel(us, gold['cb_u']) <= 1e-10
    # the final observer memory
    assert abs(mem['lastt'] - float(gold['mem_lastt'])) <= 1e-15
    assert abs(mem['lastdt'] - float(gold['mem_lastdt'])) <= 1e-15
    assert rel(mem['lasthx'], gold['mem_lasthx']) <= 1e-10
    assert rel(mem['lastrhs'], gold['mem_lastrhs']) <= 1e-10
    # and the feedback acts: far above every tolerance of the GPU tests
    assert float(gold['open_relv']) >= 1e-5


def test_solve_nse_dynamic_feedback_discretisations():
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    with pytest.raises(NotImplementedError):
        snu.solve_nse(dynamic_feedback=True, dyn_fb_disc='linear_implicit')
    with pytest.raises(NotImplementedError) as exc:
        snu.solve_nse(dynamic_feedback=True, dyn_fb_disc='trapezoidal')
    msg = str(exc.value)
    assert 'implicit_dynamic_rhs' in msg
    assert 'snu:1231-1235' in msg and '1267-1272' in msg
    with pytest.raises(NotImplementedError) as exc:      # the default
        snu.solve_nse(dynamic_feedback=True)
    assert 'snu:1231-1235' in str(exc.value)
    # AB2 needs its ingredients
    with pytest.raises(ValueError):
        snu.solve_nse(closed_loop=True, dynamic_feedback=True,
                      dyn_fb_disc='AB2')


def test_header_declares_and_capi_binds_the_feedback_entry_points():
    from dolfin_navier_scipy_amd import _capi
    hdr = open(os.path.join(ROOT, 'include', 'dns_amd.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(dns_[a-z0-9_]+)\s*\(', hdr))
    lib = _capi.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    # null handles fail cleanly, with a message
    assert lib.dns_imex_set_feedback(None, None, None, None, None, None, 1, 1,
                                     1, .5, .5, 1e-2) \
        == _capi.DNS_ERR_BAD_ARGUMENT
    assert b'null' in lib.dns_last_error()
    assert lib.dns_imex_clear_feedback(None) == _capi.DNS_ERR_BAD_ARGUMENT


def test_linear_feedback_modes_and_shapes():
    """the four modes of the reference's signature on a tiny system, against
    the equations written out"""
    from dolfin_navier_scipy_amd import time_int_utils as gtiu
    rng = np.random.default_rng(3)
    NV, Ny, Nu, hN = 7, 2, 3, 4
    C, B = rng.standard_normal((Ny, NV)), rng.standard_normal((NV, Nu))
    ha, hb, hc = (rng.standard_normal((hN, hN)), rng.standard_normal((hN, Ny)),
                  rng.standard_normal((Nu, hN)))
    x0, d = rng.standard_normal((hN, 1)), rng.standard_normal((hN, 1))
    fb = gtiu.LinearFeedback(C, B, ha, hb, hc, x0, drift=lambda t: t*d)
    v = [rng.standard_normal((NV, 1)) for _ in range(4)]
    dt = 0.1
    out, mem = fb(0., vc=v[0], memory={}, mode='init')
    assert out.shape == (NV, 1) and np.allclose(out, B @ hc @ x0)
    out, mem = fb(dt, vc=v[0], memory=mem, mode='heunpred')
    f0 = ha @ x0 + hb @ C @ v[0]
    assert np.allclose(out, B @ hc @ (x0 + dt*f0))
    out, mem = fb(dt, vc=v[1], memory=mem, mode='heuncorr')
    f1 = ha @ (x0 + dt*f0) + hb @ C @ v[1] + dt*d
    x1 = x0 + .5*dt*(f0 + f1)
    assert np.allclose(out, B @ hc @ x1)
    out, mem = fb(2*dt, vc=v[2], memory=mem, mode='abtwo')
    f2 = ha @ x1 + hb @ C @ v[2] + dt*d
    x2 = x1 + 1.5*dt*f2 - .5*dt*f0          # (lastrhs: the predictor's)
    assert np.allclose(out, B @ hc @ x2)
    out, mem = fb(3*dt, vc=v[3], memory=mem, mode='abtwo')
    f3 = ha @ x2 + hb @ C @ v[3] + 2*dt*d
    assert np.allclose(out, B @ hc @ (x2 + 1.5*dt*f3 - .5*dt*f2))
    assert fb.calls == dict(init=1, heunpred=1, heuncorr=1, abtwo=2)
