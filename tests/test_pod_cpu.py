"""POD by the method of snapshots, host side: `fem.SnapshotPOD` (the model
`evaluate` against an SVD, `plan`, the bounds), the entry points of the
library, the host-only parts of `csrc/ensemble_host.hpp` under the sanitizers,
`solve_nse(pod=)` and `_PodEnsemble` through the host loop of `cnab` /
`sbdftwo` with `tests/imex_host_model.py` behind it.  No device."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sps

import imex_host_model
import pod_model
import scenarios

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NEW_SYMBOLS = ('dns_imex_set_ensemble', 'dns_imex_get_ensemble',
               'dns_imex_ensemble_gram', 'dns_imex_ensemble_combine',
               'dns_imex_clear_ensemble', 'dns_ensemble_gram',
               'dns_ensemble_combine')


# ---- entry points -----------------------------------------------------------------

def test_header_declares_and_capi_binds_the_ensemble_entry_points():
    from dolfin_navier_scipy_amd import _capi
    hdr = open(os.path.join(ROOT, 'include', 'dns_amd.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(dns_[a-z0-9_]+)\s*\(', hdr))
    lib = _capi.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    calls = ((lib.dns_imex_set_ensemble, (None, 4, None, 2, 0)),
             (lib.dns_imex_get_ensemble, (None, 0, 1, None)),
             (lib.dns_imex_ensemble_gram, (None, None, 2, None)),
             (lib.dns_imex_ensemble_combine, (None, 2, 1, None, None)),
             (lib.dns_imex_clear_ensemble, (None,)),
             (lib.dns_ensemble_gram, (0, 2, 4, 4, None, None, None)),
             (lib.dns_ensemble_combine, (0, 2, 4, 4, None, 1, None, None)))
    for fn, args in calls:
        assert fn(*args) == _capi.DNS_ERR_BAD_ARGUMENT
        assert b'null' in lib.dns_last_error()


def test_stateless_entries_check_their_shapes_before_the_device():
    from dolfin_navier_scipy_amd import _capi
    lib = _capi.load_library()
    e, g = np.zeros(2*6), np.zeros(4)
    d = _capi.dptr
    # an odd row stride, rows shorter than nv, nothing to do, W of another size
    for m, nv, ld in ((2, 5, 5), (2, 6, 4), (0, 4, 4), (2, 0, 4)):
        assert lib.dns_ensemble_gram(0, m, nv, ld, d(e), None, d(g)) \
            == _capi.DNS_ERR_BAD_ARGUMENT, (m, nv, ld)
        assert b'ensemble' in lib.dns_last_error()
    w = _capi.CsrView(sps.identity(5, format='csr'))
    assert lib.dns_ensemble_gram(0, 2, 4, 6, d(e), w.byref(), d(g)) \
        == _capi.DNS_ERR_BAD_ARGUMENT
    assert b'NV x NV' in lib.dns_last_error()
    assert lib.dns_ensemble_combine(0, 2, 4, 6, d(e), 0, d(g), d(g)) \
        == _capi.DNS_ERR_BAD_ARGUMENT


def test_ensemble_kernels_are_a_dependency_of_the_build():
    from dolfin_navier_scipy_amd import build
    names = [os.path.basename(p) for p in build.dependencies()]
    assert 'ensemble.hpp' in names and 'ensemble_host.hpp' in names
    text = open(os.path.join(ROOT, 'dolfin_navier_scipy_amd', 'csrc',
                             'imex.hpp')).read()
    assert '#include "ensemble.hpp"' in text


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_host_parts_under_asan_and_ubsan(tmp_path):
    """table checks, layout arithmetic and the coefficient packing, compiled
    without HIP into a program of their own"""
    exe = str(tmp_path / 'pod_host_sanitize')
    build = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror',
         '-I' + os.path.join(ROOT, 'include'),
         os.path.join(HERE, 'pod_host_sanitize.cpp'), '-o', exe],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert build.returncode == 0, build.stdout.decode()[-4000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0',
               UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=600)
    out = run.stdout.decode()
    assert run.returncode == 0, out[-4000:]
    assert 'all checks passed' in out
    assert 'runtime error' not in out and 'AddressSanitizer' not in out, out


# ---- the host model -----------------------------------------------------------------

@pytest.mark.parametrize('center', [True, False])
def test_evaluate_against_an_svd(center):
    """`W = L^T L`: the singular values of `L S_c^T` are `sigma`, and the
    kept modes are `W`-orthonormal (tolerances: `pod_model`, measured here
    and printed, margin 10)"""
    from dolfin_navier_scipy_amd.fem import SnapshotPOD
    NV, m = 60, 9
    W, L = pod_model.seeded_spd(NV, seed=3)
    rng = np.random.default_rng(4)
    S = rng.standard_normal((m, NV)) + 2.*rng.standard_normal(NV)
    pod = SnapshotPOD(W, center=center)
    ev = pod.evaluate(S)
    Sc = S - S.mean(axis=0) if center else S
    sv = np.linalg.svd(L @ Sc.T, compute_uv=False)
    r = ev['modes'].shape[0]
    assert r == (m - 1 if center else m)
    assert ev['sigma'].shape == (r,) and ev['coeffs'].shape == (r, m)
    err_s = np.abs(ev['sigma'] - sv[:r]).max()/sv[0]
    orth = ev['modes'] @ (W @ ev['modes'].T)
    err_o = np.abs(orth - np.eye(r)).max()
    print('center', center, ': sigma error / sigma_1', err_s,
          ', |modes W modes^T - I|', err_o)
    assert err_s <= pod_model.SIGMA_TOL
    assert err_o <= pod_model.ORTHO_TOL
    # the pieces fit together: snapshots = mean + coeffs^T modes
    back = ev['coeffs'].T @ ev['modes'] + (ev['mean'] if center else 0.)
    assert np.abs(back - S).max() <= 1e-12*np.abs(S).max()
    if center:
        assert np.abs(ev['mean'] - S.mean(axis=0)).max() <= 1e-14
        assert ev['coef'].shape == (r + 1, m)
    else:
        assert ev['mean'] is None and ev['coef'].shape == (r, m)
    assert np.array_equal(ev['gram'], S @ (W @ S.T))


def test_truncation_by_count_energy_and_rank():
    from dolfin_navier_scipy_amd.fem import SnapshotPOD
    NV, m = 60, 9
    W, _ = pod_model.seeded_spd(NV, seed=3)
    rng = np.random.default_rng(5)
    S = rng.standard_normal((m, NV))*(2.**-np.arange(m))[:, None]
    full = SnapshotPOD(W, center=False).evaluate(S)
    lam = full['sigma']**2
    assert SnapshotPOD(W, center=False, nmodes=3).evaluate(S)['modes'] \
        .shape[0] == 3
    want = int(np.searchsorted(np.cumsum(lam)/lam.sum(), .99)) + 1
    got = SnapshotPOD(W, center=False, energy=.99).evaluate(S)
    assert got['modes'].shape[0] == want < m
    assert SnapshotPOD(W, center=False, energy=1.).evaluate(S)['modes'] \
        .shape[0] == m
    # a repeated snapshot adds no mode
    S2 = np.vstack([S[:4], S[:4]])
    assert SnapshotPOD(W, center=False).evaluate(S2)['modes'].shape[0] == 4
    with pytest.raises(ValueError):
        SnapshotPOD(W, energy=0.)
    with pytest.raises(ValueError):
        SnapshotPOD(W, every=0)
    with pytest.raises(ValueError):
        SnapshotPOD(sps.csr_matrix((3, 4)))
    with pytest.raises(ValueError):
        SnapshotPOD(W).evaluate(np.zeros((3, NV + 1)))


def test_bounds_are_the_stated_expressions():
    from dolfin_navier_scipy_amd.fem import SnapshotPOD, pod as podmod
    NV, m = 60, 9
    W, _ = pod_model.seeded_spd(NV, seed=3)
    rng = np.random.default_rng(6)
    S, coef = rng.standard_normal((m, NV)), rng.standard_normal((4, m))
    pod = SnapshotPOD(W)
    u = 2.**-53
    bg = pod.bound_gram(S)
    want = 1.01*(NV + NV + 2)*u*(np.abs(S) @ (abs(W) @ np.abs(S).T))
    assert np.allclose(bg, want, rtol=1e-14, atol=0.)
    bc = pod.bound_combine(S, coef)
    assert np.allclose(bc, 1.01*(m + 1)*u*(np.abs(coef) @ np.abs(S)),
                       rtol=1e-14, atol=0.)
    bi = podmod.gram_bound(S, None)
    assert np.allclose(bi, 1.01*(NV + 3)*u*(np.abs(S) @ np.abs(S).T),
                       rtol=1e-14, atol=0.)
    # float64 NumPy itself lies inside them against the extended references
    G = S @ (W @ S.T)
    assert np.all(np.abs(G - pod_model.gram_longdouble(S, W)) <= bg)
    assert np.all(np.abs(coef @ S - pod_model.combine_longdouble(S, coef))
                  <= bc)


# ---- plan ------------------------------------------------------------------------------

def test_plan_every_times_cap_and_off_grid():
    from dolfin_navier_scipy_amd.fem import SnapshotPOD
    W = sps.identity(70, format='csr')
    trange = np.linspace(0., .06, 13)
    pod = SnapshotPOD(W, every=1)
    kept, slots = pod.plan(trange)
    assert kept.tolist() == list(range(2, 13))          # not the Heun start
    assert slots.tolist() == list(range(11)) and pod.m == 11
    pod = SnapshotPOD(W, every=3)
    kept, slots = pod.plan(trange)
    assert kept.tolist() == [3, 6, 9, 12] and slots.tolist() == [0, 1, 2, 3]
    # over the slices of the loop: global slots, -1 elsewhere
    from dolfin_navier_scipy_amd import time_int_utils as tiu
    _, slices = tiu._inittimegrid(trange, 3)
    tabs = [pod.slots_for(s).tolist() for s in slices if s]
    assert [len(t) for t in tabs] == [len(s) for s in slices if s]
    flat = sum(tabs, [])
    assert flat == [-1, 0, -1, -1, 1, -1, -1, 2, -1, -1, 3]
    # explicit times, in any order, repeated
    pod = SnapshotPOD(W, times=[trange[7], trange[2], trange[7], trange[12]])
    kept, slots = pod.plan(trange)
    assert kept.tolist() == [2, 7, 12] and slots.tolist() == [0, 1, 2]
    assert pod.slots_for(trange[5:9]).tolist() == [-1, -1, 1, -1]
    # a kept time off the grid, the Heun start, nothing kept
    for bad in ([.5*(trange[3] + trange[4])], [trange[1]], [trange[0]]):
        with pytest.raises(ValueError) as exc:
            SnapshotPOD(W, times=bad).plan(trange)
        assert 'step times' in str(exc.value)
        assert ('Heun start' in str(exc.value)) == (bad[0] == trange[1])
    with pytest.raises(ValueError):
        SnapshotPOD(W, every=20).plan(trange)
    # the cap: m * ldv * 8 bytes, ldv = 128 here
    assert SnapshotPOD(W, max_bytes=11*128*8).plan(trange)[0].size == 11
    with pytest.raises(ValueError) as exc:
        SnapshotPOD(W, max_bytes=11*128*8 - 1).plan(trange)
    assert 'm = 11' in str(exc.value) and str(11*128*8 - 1) in str(exc.value)


# ---- through the loops ------------------------------------------------------------------

def test_solve_nse_passes_it_on_and_refuses_non_explicit_schemes():
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    from dolfin_navier_scipy_amd.fem import SnapshotPOD
    pod = SnapshotPOD(sps.identity(8, format='csr'))
    sig = inspect.signature(snu.solve_nse)
    assert sig.parameters['pod'].default is None
    with pytest.raises(NotImplementedError) as exc:
        snu.solve_nse(pod=pod, lin_vel_point=[np.zeros((8, 1))])
    assert '`pod`' in str(exc.value)
    with pytest.raises(NotImplementedError):
        snu.solve_nse(pod=pod, treat_nonl_explicit=False)


@pytest.fixture
def tiu(monkeypatch):
    mod = imex_host_model.install(monkeypatch)
    monkeypatch.setattr(mod, 'ImexStepper', pod_model.PodStepper)
    return mod


def _run(tiu, scheme, kw):
    return (tiu.sbdftwo if scheme == 'sbdf2' else tiu.cnab)(**dict(kw))


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_pod_through_the_host_loop(tiu, toy_prob, scheme):
    """stepwise: the states are stored on the host, `pod_on == 'host'` and
    `gram` is the Gram matrix of the `Recorder`'s velocities at the kept
    times; resident (the stepper's model): armed once per slice, reset only
    the first time, the same snapshots"""
    from dolfin_navier_scipy_amd.fem import SnapshotPOD
    inv = toy_prob['invinds']
    M = sps.csr_matrix(toy_prob['smc']['M'])
    got = {}
    for path in ('stepwise', 'resident'):
        pod = SnapshotPOD(M, every=2, nmodes=3)
        kw, rec, _ = scenarios.build(variant='plain', seed=0, prob=toy_prob)
        if path == 'resident':
            conv = imex_host_model.StubConvection(kw.pop('f_vdp'),
                                                  kw['appndbcs'])
            kw.update(device_convection=conv, invinds=inv,
                      resident=dict(pod=pod))
        else:
            kw.update(resident=dict(pod=pod))
        _, _, ff = _run(tiu, scheme, kw)
        assert ff == 0
        got[path] = (dict(tiu.LAST_RUN), rec.arrays(), kw['trange'])
    for path, where in (('stepwise', 'host'), ('resident', 'device')):
        lr, (times, vels, prss), trange = got[path]
        assert lr['pod_on'] == where
        res = lr['pod']
        kept = [k for k in range(2, len(trange)) if k % 2 == 0]
        assert np.array_equal(res['times'], np.asarray(trange)[kept])
        S = vels[kept][:, inv]
        assert np.array_equal(res['gram'], S @ (M @ S.T)), path
        assert res['modes'].shape == (3, inv.size)
        assert res['mean'].shape == (inv.size,)
        assert res['sigma'].shape == (3,) and res['coeffs'].shape == (3, 6)
        assert np.all(pod_model.ortho_error(res, M)
                      <= pod_model.ortho_bound(res['gram'], res['sigma']))
        assert (lr['run_calls'] > 0) == (path == 'resident')
    stepper = imex_host_model.HostStepper.made[-1]
    slices = [s for s in tiu._inittimegrid(got['resident'][2], 10)[1] if s]
    assert stepper.ens_armed == len(slices) and stepper.ens_resets == 1
    assert stepper.ens_cleared


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_orthonormality_follows_the_derived_law(tiu, toy_prob, scheme):
    """where `pod_model.ORTHO_C` comes from: `|modes W modes^T - I|_kl
    sqrt(lambda_k lambda_l) / (m u |G|_2)` of EVERY kept mode (none
    truncated) on the host model, 6 and 13 snapshots of the toy wake, with
    and without centring, and on the seeded data of the SVD test; printed,
    and within the constant that is 10 times the largest seen (1.67)"""
    from dolfin_navier_scipy_amd.fem import SnapshotPOD
    inv = toy_prob['invinds']
    M = sps.csr_matrix(toy_prob['smc']['M'])
    worst = 0.

    def ratio(res, W):
        unit = pod_model.ortho_bound(res['gram'], res['sigma']) \
            / pod_model.ORTHO_C
        return float((pod_model.ortho_error(res, W)/unit).max())
    for nts, tE in ((12, .06), (26, .13)):
        for center in (True, False):
            pod = SnapshotPOD(M, every=2, center=center)
            kw, rec, _ = scenarios.build(variant='plain', seed=0,
                                         prob=toy_prob, Nts=nts, tE=tE)
            conv = imex_host_model.StubConvection(kw.pop('f_vdp'),
                                                  kw['appndbcs'])
            kw.update(device_convection=conv, invinds=inv,
                      resident=dict(pod=pod))
            _run(tiu, scheme, kw)
            res = tiu.LAST_RUN['pod']
            assert res['modes'].shape[0] >= 5
            c = ratio(res, M)
            print(scheme, nts, 'center', center, 'modes',
                  res['modes'].shape[0], ': c =', c)
            worst = max(worst, c)
    W, _ = pod_model.seeded_spd(60, seed=3)
    rng = np.random.default_rng(4)
    S = rng.standard_normal((9, 60)) + 2.*rng.standard_normal(60)
    for center in (True, False):
        c = ratio(SnapshotPOD(W, center=center).evaluate(S), W)
        print('seeded, center', center, ': c =', c)
        worst = max(worst, c)
    assert worst <= pod_model.ORTHO_C/10.*1.001


def test_a_loop_that_breaks_off_reports_no_pod(tiu, toy_prob):
    """the blow-up guard ends the loop: `ffflag = 1` comes back, nothing is
    decomposed (slots are unfilled), on both paths"""
    from dolfin_navier_scipy_amd.fem import SnapshotPOD
    M = sps.csr_matrix(toy_prob['smc']['M'])
    for path in ('stepwise', 'resident'):
        kw, rec, _ = scenarios.build(variant='plain', seed=0, prob=toy_prob)
        kw.update(check_ff_maxv=1e-3, ntimeslices=3)
        rsd = dict(pod=SnapshotPOD(M, every=2))
        if path == 'resident':
            conv = imex_host_model.StubConvection(kw.pop('f_vdp'),
                                                  kw['appndbcs'])
            kw.update(device_convection=conv, invinds=toy_prob['invinds'])
        kw.update(resident=rsd)
        _, _, ff = tiu.cnab(**kw)
        assert ff == 1
        assert tiu.LAST_RUN['pod'] is None
        assert 'pod_on' in tiu.LAST_RUN


def test_last_run_has_no_pod_keys_without_it(tiu, toy_prob):
    kw, rec, _ = scenarios.build(variant='plain', seed=0, prob=toy_prob)
    tiu.cnab(**kw)
    assert not [k for k in tiu.LAST_RUN if k.startswith('pod')]


def test_pod_of_another_size_is_refused(tiu, toy_prob):
    from dolfin_navier_scipy_amd.fem import SnapshotPOD
    kw, rec, _ = scenarios.build(variant='plain', seed=0, prob=toy_prob)
    kw.update(resident=dict(pod=SnapshotPOD(sps.identity(5, format='csr'))))
    with pytest.raises(ValueError) as exc:
        tiu.cnab(**kw)
    assert 'NV' in str(exc.value)
