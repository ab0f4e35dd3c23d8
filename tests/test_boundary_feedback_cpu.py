"""`time_int_utils.BoundaryFeedback`, host side: the protocol (`getbcs` face
and `controls()` face) against a NumPy recurrence written out here, the
refusals, the linearity the device form rests on (`applybcs` of the unit
controls, the schemes' weights against their `row` formula), and the host loop
of the CPU oracle with the object as `getbcs`."""
import numpy as np
import pytest
import scipy.sparse as sps

import boundary_feedback_setup as bs
import feedback_setup as fs
from oracle import imex_oracle


@pytest.fixture(scope='module')
def tiu():
    from dolfin_navier_scipy_amd import time_int_utils
    return time_int_utils


def _states(prob, n, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((prob['th'].vdim, 1)) for _ in range(n)]


@pytest.mark.parametrize('Nu', [1, 2])
def test_protocol_against_a_numpy_recurrence(tiu, toy_prob, Nu):
    """`init`, `heunpred`, `heuncorr`, then AB2 steps: `b = base + S u` of
    every call, `history`, `calls` and the memory keys"""
    fb, obs = bs.make_feedback(tiu, toy_prob, seed=4, Nu=Nu)
    ha, hb, hc, x0, dv = (obs[k] for k in ('ha', 'hb', 'hc', 'inihx',
                                           'dvec'))
    inv = toy_prob['invinds']
    C = bs.full_sensors(toy_prob)[:, inv]
    S, base = fb.s_mat.toarray(), fb.base
    dt, vs = 5e-3, _states(toy_prob, 5)

    def drift(t):
        return np.sin(7*t)*dv

    def close(b, u):
        want = base + S @ u.reshape(-1)
        assert np.allclose(b, want, rtol=1e-14, atol=1e-16)
    b = fb(0., None, None, mode='init')
    assert isinstance(b, list) and len(b) == base.size
    close(b, hc @ x0)
    y = C @ vs[0][inv]
    f0 = ha @ x0 + hb @ y + drift(0.)
    xp = x0 + dt*f0
    close(fb(dt, vs[0], None, mode='heunpred'), hc @ xp)
    y = C @ vs[1][inv]
    f1 = ha @ xp + hb @ y + drift(dt)
    x = x0 + .5*dt*(f1 + f0)
    close(fb(dt, vs[1], None, mode='heuncorr'), hc @ x)
    flast, t = f0, dt               # (the PREDICTOR's right-hand side)
    for k in range(2, 5):
        y = C @ vs[k][inv]
        f = ha @ x + hb @ y + drift(t)
        x, flast, t = x + 1.5*dt*f - .5*dt*flast, f, t + dt
        close(fb(t, vs[k], None, mode='abtwo'), hc @ x)
        assert np.allclose(fb.history[-1][2], y[:, 0], rtol=1e-14)
        assert np.allclose(fb.history[-1][3], (hc @ x)[:, 0], rtol=1e-13,
                           atol=1e-16)
    assert fb.calls == dict(init=1, heunpred=1, heuncorr=1, abtwo=3)
    assert set(fb.memory) == {'lastt', 'lasthx', 'lastrhs', 'lastdt', 'hphx'}
    assert np.allclose(fb.memory['lasthx'], x, rtol=1e-13)
    assert np.allclose(fb.memory['lastrhs'], flast, rtol=1e-13)
    with pytest.raises(ValueError):
        fb(t, vs[0], None, mode='nonsense')


def test_controls_share_one_observer(tiu, toy_prob):
    """`Nu` callables: the first call for a `(time, mode)` advances the
    observer, whichever control it is; the values are those of the `getbcs`
    face"""
    fa, _ = bs.make_feedback(tiu, toy_prob, seed=4, Nu=2)
    fc, _ = bs.make_feedback(tiu, toy_prob, seed=4, Nu=2)
    funcs = fc.controls()
    assert len(funcs) == 2
    vs, dt = _states(toy_prob, 4, seed=1), 5e-3
    calls = [(0., None, 'stokes'), (dt, vs[0], 'heunpred'),
             (dt, vs[1], 'heuncorr'), (2*dt, vs[2], 'abtwo'),
             (3*dt, vs[3], 'abtwo')]
    for n, (t, v, mode) in enumerate(calls):
        fa(t, v, None, mode='init' if mode == 'stokes' else mode)
        want = fa.history[-1][3]
        order = (1, 0, 1) if n % 2 else (0, 1, 0)
        for k in order:
            mem = object()
            got, back = funcs[k](t, vel=v, p=None, mode=mode, memory=mem)
            assert back is mem
            assert got == want[k]
        assert len(fc.history) == n + 1
    assert fc.calls == dict(init=1, heunpred=1, heuncorr=1, abtwo=2)
    assert all(f.boundary_feedback is fc for f in funcs)
    assert tiu._boundary_feedback_of(fc) is fc
    assert tiu._boundary_feedback_of(lambda *a, **k: []) is None


def test_refusals(tiu, toy_prob):
    _, _, cntinds, cntbase = bs.split(toy_prob)
    obs = fs.observer(1, 3, 2)
    Cf = bs.full_sensors(toy_prob)
    S = bs.shape_matrix(cntbase, 2)
    args = (obs['ha'], obs['hb'], obs['hc'], obs['inihx'])
    # a sensor on a Dirichlet column
    bad = Cf.tolil()
    bad[1, cntinds[2]] = 1.
    with pytest.raises(ValueError) as exc:
        tiu.BoundaryFeedback(bad.tocsr(), S, *args,
                             invinds=toy_prob['invinds'])
    assert 'Dirichlet column' in str(exc.value)
    assert str(int(cntinds[2])) in str(exc.value)
    # widths
    with pytest.raises(ValueError):
        tiu.BoundaryFeedback(Cf, bs.shape_matrix(cntbase, 3), *args,
                             invinds=toy_prob['invinds'])
    with pytest.raises(ValueError):
        tiu.BoundaryFeedback(Cf[:2], S, *args, invinds=toy_prob['invinds'])
    with pytest.raises(ValueError):
        tiu.BoundaryFeedback(Cf, S, *args, invinds=toy_prob['invinds'],
                             base=np.ones(cntbase.size + 1))
    ok = tiu.BoundaryFeedback(Cf, S, *args, invinds=toy_prob['invinds'])
    assert np.array_equal(ok.base, np.zeros(cntbase.size))


@pytest.mark.parametrize('Nu', [1, 2])
def test_unit_calls_of_applybcs_reproduce_it(tiu, toy_prob, Nu):
    """`Ba u`, `Bm u`, `Bj u` from `Nu` calls with `S e_k` against
    `applybcs(S u)` for random `u`, at 1e-13 of the sums of absolute
    products; the literal closure has no terms"""
    kw, _, fb = bs.build(tiu, toy_prob, Nu=Nu)
    NP, NV = kw['J'].shape
    Ba, Bm, Bj = fb.boundary_terms(kw['applybcs'], NV, NP)
    assert Ba.shape == Bm.shape == (NV, Nu) and Bj.shape == (NP, Nu)
    assert Ba.nnz > 0 and Bm.nnz > 0 and Bj.nnz > 0
    rng = np.random.default_rng(8)
    for _ in range(3):
        u = rng.standard_normal(Nu)
        bfv, bfp, mbc = kw['applybcs']((fb.s_mat @ u).tolist())
        for B, want in ((Ba, bfv), (Bm, mbc), (Bj, bfp)):
            bound = 1e-13*(abs(B) @ np.abs(u)) + 1e-300
            assert np.all(np.abs(B @ u - want[:, 0]) <= bound)
    assert fb.boundary_terms(bs.literal_applybcs(NV, NP), NV, NP) is None
    assert fb.boundary_terms(lambda b: (0., 0., 0.), NV, NP) is None


@pytest.mark.parametrize('scheme', ['_CNAB', '_SBDF2'])
def test_scheme_weights_are_those_of_its_row_formula(tiu, scheme):
    """`row(terms(u)) - row(terms(0)) = sum_j (wm_j Bm + wa_j Ba) u_j`"""
    sch = getattr(tiu, scheme)
    rng = np.random.default_rng(2)
    n, Nu, dt = 7, 2, 1e-2
    Ba, Bm = rng.standard_normal((n, Nu)), rng.standard_normal((n, Nu))
    fv = [rng.standard_normal((n, 1)) for _ in range(3)]
    us = [rng.standard_normal((Nu, 1)) for _ in range(3)]       # n, c, p

    def terms(scale):
        return [tiu._Terms(None, scale*(Ba @ u), scale*(Bm @ u), f, 0.)
                for u, f in zip(us, fv)]
    tn, tc, tp = terms(1.)
    zn, zc, zp = terms(0.)
    diff = sch.row(dt, tp, tc, tn) - sch.row(dt, zp, zc, zn)
    wm, wa = sch.bc_weights(dt)
    want = sum(wm[j]*(Bm @ us[j]) + wa[j]*(Ba @ us[j]) for j in range(3))
    assert np.allclose(diff, want, rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_oracle_loop_takes_the_object_as_getbcs(tiu, toy_prob, scheme):
    """the CPU oracle calls it every step; the saved velocities carry `base +
    S u` of the step's observer output on the controlled dofs, and the
    feedback acts (another gain ends elsewhere)"""
    _, _, cntinds, _ = bs.split(toy_prob)
    integ = imex_oracle.cnab if scheme == 'cnab' else imex_oracle.sbdftwo
    ends = []
    for gain in (.5, 1.):
        kw, rec, fb = bs.build(tiu, toy_prob, Nts=6, tE=0.03, gain=gain)
        v, p, ff = integ(**kw)
        assert ff == 0
        assert fb.calls == dict(init=1, heunpred=1, heuncorr=1, abtwo=5)
        times, vels, _ = rec.arrays()
        rows = [h for h in fb.history if h[1] in ('init', 'heuncorr',
                                                  'abtwo')]
        assert len(rows) == times.size == 7
        for k, h in enumerate(rows):
            assert np.array_equal(vels[k][cntinds], fb.values(h[3]))
        ends.append(v)
    M = toy_prob['smc']['M']
    assert fs.mnorm(M, ends[0] - ends[1]) >= 1e-6*fs.mnorm(M, ends[1])
