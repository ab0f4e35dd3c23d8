"""POD-Galerkin projection, host side: `fem.GalerkinROM` (the fp64 model
`project(device=False)` against the long double model `rom_model`, against the
host assembler and against the full operators), `integrate`, the refusals, the
entry points of the library, the host-only parts of `csrc/galerkin_host.hpp`
under the sanitizers, and `resident=dict(pod=, rom=)` through the host loop of
`cnab` / `sbdftwo`.  No device."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.linalg as spla
import scipy.sparse as sps

import conv_meshes
import conv_model
import imex_host_model
import pod_model
import rom_model
import scenarios

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LD = np.longdouble
U = 2.0**-53

NEW_SYMBOLS = ('dns_ensemble_project', 'dns_conv_project_tensor')


# ---- entry points and constants ----------------------------------------------------

def test_header_declares_and_capi_binds_the_new_entry_points():
    from dolfin_navier_scipy_amd import _capi
    hdr = open(os.path.join(ROOT, 'include', 'dns_amd.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(dns_[a-z0-9_]+)\s*\(', hdr))
    lib = _capi.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.dns_ensemble_project(0, 2, 2, 4, 4, None, None, None, None) \
        == _capi.DNS_ERR_BAD_ARGUMENT
    assert b'null' in lib.dns_last_error()
    assert lib.dns_conv_project_tensor(None, 2, 2, 4, None, None, None) \
        == _capi.DNS_ERR_BAD_ARGUMENT
    assert b'null' in lib.dns_last_error()
    # shapes are checked before the device is touched
    x, p = np.zeros(2*6), np.zeros(4)
    d = _capi.dptr
    for mx, my, nv, ld in ((2, 2, 5, 5), (2, 2, 6, 4), (0, 2, 4, 4),
                           (2, 0, 4, 4), (2, 2, 0, 4)):
        assert lib.dns_ensemble_project(0, mx, my, nv, ld, d(x), d(x), None,
                                        d(p)) == _capi.DNS_ERR_BAD_ARGUMENT
        assert b'ensemble' in lib.dns_last_error()
    w = _capi.CsrView(sps.identity(5, format='csr'))
    assert lib.dns_ensemble_project(0, 2, 2, 4, 6, d(x), None, w.byref(),
                                    d(p)) == _capi.DNS_ERR_BAD_ARGUMENT
    assert b'NV x NV' in lib.dns_last_error()


def test_header_constants_are_the_ones_the_package_mirrors():
    from dolfin_navier_scipy_amd.fem import rom
    from dolfin_navier_scipy_amd import convection
    text = open(os.path.join(ROOT, 'dolfin_navier_scipy_amd', 'csrc',
                             'galerkin_host.hpp')).read()
    chunk = int(re.search(r'constexpr int kRomCellChunk = (\d+);', text).group(1))
    nbmax = int(re.search(r'constexpr int kRomMaxBasis = (\d+);', text).group(1))
    assert chunk == rom.ROM_CELL_CHUNK
    assert nbmax == rom.ROM_MAX_BASIS == convection.ROM_MAX_BASIS == 33
    # the counts of the bound are the model's
    assert rom.K_TEN == rom_model.K_TEN and rom.T_TAB == conv_model.T_TAB
    # the new kernels are a dependency of the build, outside the step
    from dolfin_navier_scipy_amd import build
    names = [os.path.basename(p) for p in build.dependencies()]
    assert 'galerkin.hpp' in names and 'galerkin_host.hpp' in names
    csrc = os.path.join(ROOT, 'dolfin_navier_scipy_amd', 'csrc')
    for f in ('imex.hpp', 'step_kernels.hpp', 'solver.hpp'):
        assert 'galerkin' not in open(os.path.join(csrc, f)).read()
    assert 'galerkin' not in open(os.path.join(ROOT, 'bench.py')).read()


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_host_parts_under_asan_and_ubsan(tmp_path):
    """tile and column index maps, partial-buffer sizes at the limits and the
    shape checks, compiled without HIP into a program of their own"""
    exe = str(tmp_path / 'rom_host_sanitize')
    build = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror',
         '-I' + os.path.join(ROOT, 'include'),
         os.path.join(HERE, 'rom_host_sanitize.cpp'), '-o', exe],
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


# ---- the host model against the long double model ------------------------------------

def _mesh_cases():
    yield 'fan', conv_meshes.fan(40, seed=5)
    yield 'rectangle33', conv_meshes.rectangle(33, seed=3)


SPLITS = (dict(dirichlet='boundary'), dict(dirichlet='none'),
          dict(dirichlet=0.3, full_cells=2))


def test_host_tensor_lies_inside_the_bound_of_the_model(toy_prob):
    from dolfin_navier_scipy_amd.fem import rom
    worst = 0.
    cases = []
    th = toy_prob['th']
    cases.append(('toy wake', rom_model.HostConv.from_taylor_hood(
        th, toy_prob['invinds'], toy_prob['dbcinds'])))
    for name, mesh in _mesh_cases():
        for k, split in enumerate(SPLITS):
            inv, dbc = mesh.split(seed=k, **split)
            cases.append(('%s %s' % (name, split['dirichlet']),
                          rom_model.HostConv.from_mesh(mesh, inv, dbc)))
    for k, (name, hc) in enumerate(cases):
        B, D = rom_model.seeded_basis(6, hc.nv, hc.ndbc, seed=10 + k)
        for nt, dbc_rows in ((6, D), (4, D), (6, None)):
            got = rom.tensor_host(hc, B, dbc_rows, ntest=nt)
            sp = hc.space()
            want = rom_model.tensor_longdouble(sp, B, dbc_rows, nt)
            bound = rom_model.bound_longdouble(sp, B, dbc_rows, nt)
            r = conv_model.ratio(got, want, bound)
            print(name, 'nt', nt, 'D', dbc_rows is not None,
                  ': error / bound', r)
            worst = max(worst, r)
            assert r <= 1.
            # the package's own bound is the model's (fp64 magnitude sums,
            # 1 % on top)
            mine = rom.bound_tensor(hc, B, dbc_rows, ntest=nt)
            assert np.all(mine >= bound.astype(np.float64))
            assert np.all(mine <= 1.02*bound.astype(np.float64))
    print('worst error / bound of tensor_host:', worst)


def _full(th, inv, dbi, row, dvals):
    f = np.zeros((th.vdim, 1))
    f[inv, 0] = row
    f[dbi, 0] = dvals
    return f


def test_the_three_identities_of_the_host_assembler(toy_prob):
    """the tensor against `convection_vec(u_k, utwo=u_j)`, its contraction
    against `convection_vec(u)`, and `c` / `L` / `H` against their
    definitions -- within the sum of the bounds involved (the assembler's:
    `conv_model`'s `K_VEC` count per row, contracted with `|phi_i|`)"""
    from dolfin_navier_scipy_amd.fem import rom, GalerkinROM
    th, inv, dbi = toy_prob['th'], toy_prob['invinds'], toy_prob['dbcinds']
    hc = rom_model.HostConv.from_taylor_hood(th, inv, dbi, toy_prob['dbcvals'])
    sp = hc.space()
    nb, nt = 5, 4
    B, D = rom_model.seeded_basis(nb, hc.nv, hc.ndbc, seed=21)
    T = rom.tensor_host(hc, B, D, ntest=nt)
    BT = rom.bound_tensor(hc, B, D, ntest=nt)
    Ta = rom.tensor_host(hc, B, D, ntest=nt, absval=True)
    g_vec = float(conv_model.gamma(conv_model.K_VEC + sp.row_len.max()))
    worst = 0.
    for j in range(nb):
        for k in range(nb):
            v = th.convection_vec(_full(th, inv, dbi, B[k], D[k]),
                                  utwo=_full(th, inv, dbi, B[j], D[j]))[inv, 0]
            tol = BT[:, j, k] + 1.01*(g_vec + (hc.nv + 1)*U)*Ta[:, j, k]
            err = np.abs(B[:nt] @ v - T[:, j, k])
            worst = max(worst, float((err/tol).max()))
            assert np.all(err <= tol)
            assert np.all(err <= 1e-14*np.abs(T).max())
    a = np.random.default_rng(22).standard_normal(nb)
    u, du = a @ B, a @ D
    v = th.convection_vec(_full(th, inv, dbi, u, du))[inv, 0]
    got = np.einsum('ijk,j,k->i', T, a, a)
    aa = np.abs(a)
    mag = np.einsum('ijk,j,k->i', Ta, aa, aa)
    tol = np.einsum('ijk,j,k->i', BT, aa, aa) \
        + 1.01*(g_vec + (hc.nv + 2*nb + 6)*U)*mag
    err = np.abs(B[:nt] @ v - got)
    print('tensor vs assembler, worst error / tolerance:', worst,
          '; contraction:', float((err/tol).max()))
    assert np.all(err <= tol)
    assert np.all(err <= 2e-14*np.abs(got).max())
    # c, L, H of `project` are the slices they are defined as
    prob = toy_prob
    M, A = (sps.csr_matrix(prob['smc'][k]) for k in ('M', 'A'))
    r = nb - 1
    gr = GalerkinROM(A, prob['rhsd']['fv'], M=M, J=prob['smc']['J'])
    ops = gr.project(B[:r], B[r], hc, D[r], device=False)
    Dm = np.zeros_like(D)
    Dm[r] = D[r]
    Tm = rom.tensor_host(hc, B, Dm, ntest=r)
    assert np.array_equal(ops['c'], Tm[:, r, r])
    assert np.array_equal(ops['H'], Tm[:, :r, :r])
    assert np.array_equal(ops['L'], Tm[:, r, :r] + Tm[:, :r, r])
    assert ops['L'][1, 2] == Tm[1, r, 2] + Tm[1, 2, r]
    assert np.array_equal(ops['Mr'], B[:r] @ (M @ B[:r].T))
    bo = gr.bound_ops(B[:r], B[r], hc, D[r])
    assert np.all(np.abs(ops['Ar'] - B[:r] @ (A @ B[:r].T)) <= 2*bo['Ar'])
    fv = np.asarray(prob['rhsd']['fv']).reshape(-1)
    assert np.all(np.abs(ops['b0'] - B[:r] @ (A @ B[r] - fv)) <= 2*bo['b0'])
    assert ops['div'] == np.abs(prob['smc']['J'] @ B[:r].T).max()
    # `mean is None`: a zero row carries the Dirichlet values
    ops0 = gr.project(B[:r], None, hc, D[r], device=False)
    Bz = np.vstack([B[:r], np.zeros((1, hc.nv))])
    T0 = rom.tensor_host(hc, Bz, Dm, ntest=r)
    assert np.array_equal(ops0['c'], T0[:, r, r])
    assert np.array_equal(ops0['b0'], -(B[:r] @ fv[:, None])[:, 0])


# ---- "the ROM is the Galerkin projection" ----------------------------------------------

def _spmv_ld(A, x):
    A = sps.csr_matrix(A)
    return conv_model._spmv(A.indptr, A.indices, A.data.astype(LD), x)


def _projection_identity(gr, hc, dbcvals, a):
    """`(error, tolerance)` of `rhs(a)` against `-Phi (A u + N(u)u - fv)`, `u
    = lift(a)`, the right side from the full operators in long double; the
    tolerance: `bound_ops` contracted with `|a|`, and the r x r contraction's
    own roundings"""
    sp = hc.space()
    modes, mean = gr.modes.astype(LD), gr.mean.astype(LD)
    aL = np.asarray(a, dtype=np.float64).astype(LD)
    uL = mean + aL @ modes
    full = np.zeros(hc._vdim, dtype=LD)
    full[hc._invinds] = uL
    if hc.ndbc:
        full[hc._dbcinds] = np.asarray(dbcvals, dtype=np.float64)
    ul = full[hc._cell_vdofs].reshape(hc.ncells, 6, 2)
    vec, _, _ = conv_model.cell_quantities(sp.glam, sp.area, ul, LD)
    nuu = sp.gather_rows(vec)
    want = -(modes @ (_spmv_ld(gr.A, uL) + nuu - gr.fv.astype(LD)))
    bo = gr.bound_ops(gr.modes, gr.mean, hc, dbcvals)
    o = gr.ops
    aa = np.abs(np.asarray(a, dtype=np.float64))
    r = aa.size
    mag = np.abs(o['Ar']) @ aa + np.abs(o['b0']) + np.abs(o['c']) \
        + np.abs(o['L']) @ aa + (np.abs(o['H']) @ aa) @ aa
    tol = bo['Ar'] @ aa + bo['b0'] + bo['c'] + bo['L'] @ aa \
        + (bo['H'] @ aa) @ aa + 1.01*(r*r + r + 6)*U*mag
    return np.abs(gr.rhs(a).astype(LD) - want).astype(np.float64), tol


def test_rhs_is_the_galerkin_projection_of_the_full_operators(toy_prob):
    from dolfin_navier_scipy_amd.fem import GalerkinROM
    prob = toy_prob
    th, inv, dbi = prob['th'], prob['invinds'], prob['dbcinds']
    hc = rom_model.HostConv.from_taylor_hood(th, inv, dbi, prob['dbcvals'])
    M, A = (sps.csr_matrix(prob['smc'][k]) for k in ('M', 'A'))
    rng = np.random.default_rng(31)
    r = 6
    modes = rng.standard_normal((r, hc.nv))
    mean = rng.standard_normal(hc.nv)
    gr = GalerkinROM(A, prob['rhsd']['fv'], M=M)
    gr.project(modes, mean, hc, prob['dbcvals'], device=False)
    worst = 0.
    for k in range(4):
        a = rng.standard_normal(r)*10.**(k - 2)
        err, tol = _projection_identity(gr, hc, prob['dbcvals'], a)
        worst = max(worst, float((err/tol).max()))
        assert np.all(err <= tol), (k, err, tol)
    print('seeded a: worst error / tolerance', worst)


# ---- integrate ---------------------------------------------------------------------------

def test_integrate_is_of_second_order():
    """a 3 x 3 linear system, `H = 0`: halving `dt` divides the error against
    `scipy.linalg.expm` by 3.5 to 4.5"""
    from dolfin_navier_scipy_amd.fem import GalerkinROM
    rng = np.random.default_rng(41)
    r = 3
    Mr = np.eye(r) + .1*rng.standard_normal((r, r))
    Mr = Mr @ Mr.T
    Ar = np.array([[1., 2., 0.], [-2., 1., .3], [0., -.3, .5]])
    L = .4*rng.standard_normal((r, r))
    b0, c = rng.standard_normal(r), rng.standard_normal(r)
    gr = GalerkinROM(sps.identity(4, format='csr'), np.zeros(4))
    gr.ops = dict(Mr=Mr, Ar=Ar, b0=b0, c=c, L=L, H=np.zeros((r, r, r)))
    a0 = rng.standard_normal(r)
    K = -np.linalg.solve(Mr, Ar + L)
    g = -np.linalg.solve(Mr, b0 + c)
    aug = np.zeros((r + 1, r + 1))
    aug[:r, :r], aug[:r, r] = K, g
    tE = 1.
    exact = (spla.expm(tE*aug) @ np.append(a0, 1.))[:r]
    errs = []
    for n in (40, 80, 160):
        traj = gr.integrate(a0, np.linspace(0., tE, n + 1))
        assert traj.shape == (n + 1, r) and np.array_equal(traj[0], a0)
        errs.append(np.linalg.norm(traj[-1] - exact))
    print('errors', errs, 'ratios', errs[0]/errs[1], errs[1]/errs[2])
    for e0, e1 in zip(errs[:-1], errs[1:]):
        assert 3.5 <= e0/e1 <= 4.5
    with pytest.raises(ValueError):
        gr.integrate(a0, [0., .1, .3])
    # rhs and lift
    a = rng.standard_normal(r)
    assert np.allclose(gr.rhs(a), -(Ar @ a + b0 + c + L @ a), rtol=1e-14)
    gr.modes, gr.mean = rng.standard_normal((r, 4)), rng.standard_normal(4)
    assert np.allclose(gr.lift(a), gr.mean + a @ gr.modes, rtol=1e-15)
    assert gr.lift(np.stack([a, 2*a], axis=1)).shape == (2, 4)


# ---- refusals --------------------------------------------------------------------------------

def test_refusals_by_name_before_any_device_call(toy_prob):
    from dolfin_navier_scipy_amd.fem import rom, GalerkinROM
    from dolfin_navier_scipy_amd import convection
    prob = toy_prob
    hc = rom_model.HostConv.from_taylor_hood(
        prob['th'], prob['invinds'], prob['dbcinds'], prob['dbcvals'])
    nv, nd = hc.nv, hc.ndbc
    for fun in (lambda *a, **k: rom.tensor_host(hc, *a, **k),
                lambda *a, **k: convection.check_basis(nv, nd, *a, **k),
                lambda *a, **k: convection.ConvectionP2.check_basis(
                    hc, *a, **k)):
        with pytest.raises(ValueError) as exc:
            fun(np.zeros((34, nv)))
        assert 'nb = 34' in str(exc.value)
        with pytest.raises(ValueError) as exc:
            fun(np.zeros((5, nv)), ntest=6)
        assert '`ntest` = 6' in str(exc.value)
        with pytest.raises(ValueError) as exc:
            fun(np.zeros((5, nv)), ntest=0)
        assert '`ntest`' in str(exc.value)
        for wrong in ((5, nv - 1), (5, nv + 3), (nv,)):
            with pytest.raises(ValueError) as exc:
                fun(np.zeros(wrong))
            assert '`basis`' in str(exc.value)
        with pytest.raises(ValueError) as exc:
            fun(np.zeros((5, nv)), np.zeros((4, nd)))
        assert '`dbc_rows`' in str(exc.value)
        with pytest.raises(ValueError) as exc:
            fun(np.zeros((5, nv)), np.zeros((5, nd + 1)))
        assert '`dbc_rows`' in str(exc.value)
    M, A = (sps.csr_matrix(prob['smc'][k]) for k in ('M', 'A'))
    gr = GalerkinROM(A, prob['rhsd']['fv'], M=M)
    for device in (True, False):        # (refused before the device route)
        with pytest.raises(ValueError) as exc:
            gr.project(np.zeros((33, nv)), None, hc, prob['dbcvals'],
                       device=device)
        assert 'nb = r + 1 = 34' in str(exc.value)
        with pytest.raises(ValueError) as exc:
            gr.project(np.zeros((3, nv + 2)), None, hc, prob['dbcvals'],
                       device=device)
        assert '`modes`' in str(exc.value)
        with pytest.raises(ValueError) as exc:
            gr.project(np.zeros((3, nv)), np.zeros(nv - 1), hc,
                       prob['dbcvals'], device=device)
        assert '`mean`' in str(exc.value)
        with pytest.raises(ValueError) as exc:
            gr.project(np.zeros((3, nv)), None, hc, prob['dbcvals'][:-1],
                       device=device)
        assert '`dbcvals`' in str(exc.value)
        hc.dbc_table_rows = 4
        with pytest.raises(ValueError) as exc:
            gr.project(np.zeros((3, nv)), None, hc, prob['dbcvals'],
                       device=device)
        assert 'constant boundary values only' in str(exc.value)
        hc.dbc_table_rows = 0
    with pytest.raises(ValueError) as exc:
        GalerkinROM(A, prob['rhsd']['fv']).project(
            np.zeros((3, nv)), None, hc, prob['dbcvals'], device=False)
    assert 'mass matrix' in str(exc.value)
    with pytest.raises(ValueError):
        GalerkinROM(A, np.zeros(nv + 1))
    with pytest.raises(ValueError):
        GalerkinROM(A, np.zeros(nv), M=sps.identity(nv + 1))
    with pytest.raises(ValueError):
        GalerkinROM(A, np.zeros(nv)).rhs(np.zeros(3))


def test_solve_nse_passes_it_on_and_refuses_non_explicit_schemes():
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    from dolfin_navier_scipy_amd.fem import SnapshotPOD, GalerkinROM
    W = sps.identity(8, format='csr')
    pod, gr = SnapshotPOD(W), GalerkinROM(W, np.zeros(8))
    sig = inspect.signature(snu.solve_nse)
    assert sig.parameters['rom'].default is None
    with pytest.raises(ValueError) as exc:
        snu.solve_nse(rom=gr)
    assert '`rom` without `pod`' in str(exc.value)
    with pytest.raises(NotImplementedError) as exc:
        snu.solve_nse(pod=pod, rom=gr, lin_vel_point=[np.zeros((8, 1))])
    assert '`rom`' in str(exc.value)
    with pytest.raises(NotImplementedError):
        snu.solve_nse(pod=pod, rom=gr, treat_nonl_explicit=False)
    src = inspect.getsource(snu.solve_nse)
    assert "update(rom=rom)" in src


# ---- through the loops ---------------------------------------------------------------------

@pytest.fixture
def tiu(monkeypatch):
    mod = imex_host_model.install(monkeypatch)
    monkeypatch.setattr(mod, 'ImexStepper', pod_model.PodStepper)
    return mod


def _no_feedback(t, vc=None, memory={}, mode=None):
    """a `dynamic_rhs` that adds nothing: the loop takes one step at a time"""
    return 0., memory


def _stepwise_kw(toy_prob, rsd, **over):
    kw, rec, _ = scenarios.build(variant='plain', seed=0, prob=toy_prob)
    conv = rom_model.StubRomConvection(
        kw.pop('f_vdp'), kw['appndbcs'], toy_prob['th'], toy_prob['invinds'],
        toy_prob['dbcinds'], toy_prob['dbcvals'])
    kw.update(device_convection=conv, invinds=toy_prob['invinds'],
              resident=rsd, dynamic_rhs=_no_feedback, dynamic_rhs_memory={})
    kw.update(over)
    return kw, conv


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_rom_through_the_host_loop(tiu, toy_prob, scheme):
    """one step at a time: `rom_on == 'host'`, `Mr` the identity within
    `pod_model.ortho_bound`, and `rhs` the projection of the full operators
    for the columns of `coeffs`"""
    from dolfin_navier_scipy_amd.fem import SnapshotPOD, GalerkinROM
    prob = toy_prob
    M, A = (sps.csr_matrix(prob['smc'][k]) for k in ('M', 'A'))
    pod = SnapshotPOD(M, every=2, nmodes=3)
    gr = GalerkinROM(A, prob['rhsd']['fv'], J=prob['smc']['J'])
    kw, conv = _stepwise_kw(prob, dict(pod=pod, rom=gr))
    run = tiu.sbdftwo if scheme == 'sbdf2' else tiu.cnab
    _, _, ff = run(**kw)
    assert ff == 0
    lr = tiu.LAST_RUN
    assert lr['pod_on'] == 'host' and lr['rom_on'] == 'host'
    assert lr['run_calls'] == 0
    ops, res = lr['rom'], lr['pod']
    assert sorted(ops) == ['Ar', 'H', 'L', 'Mr', 'b0', 'c', 'div']
    assert ops['Mr'].shape == (3, 3) and ops['H'].shape == (3, 3, 3)
    assert gr.M is pod.W                 # (the POD's weight matrix)
    assert np.all(np.abs(ops['Mr'] - np.eye(3))
                  <= pod_model.ortho_bound(res['gram'], res['sigma']))
    assert ops['div'] >= 0.
    worst = 0.
    for s in range(res['coeffs'].shape[1]):
        err, tol = _projection_identity(gr, conv, prob['dbcvals'],
                                        res['coeffs'][:, s])
        worst = max(worst, float((err/tol).max()))
        assert np.all(err <= tol), s
    print(scheme, 'coeffs columns: worst error / tolerance', worst)
    # the snapshots are the lifts of their coefficients (POD, all modes kept
    # would make it exact; here: the projection error is what is left)
    assert gr.lift(res['coeffs']).shape == (res['coeffs'].shape[1], M.shape[0])


def test_rom_is_refused_without_pod_and_without_a_device_operator(tiu, toy_prob):
    from dolfin_navier_scipy_amd.fem import SnapshotPOD, GalerkinROM
    prob = toy_prob
    M, A = (sps.csr_matrix(prob['smc'][k]) for k in ('M', 'A'))
    gr = GalerkinROM(A, prob['rhsd']['fv'])
    kw, _ = _stepwise_kw(prob, dict(rom=gr))
    with pytest.raises(ValueError) as exc:
        tiu.cnab(**kw)
    assert '`rom` without `pod`' in str(exc.value)
    # a host `f_vdp`: no element data
    kw, rec, _ = scenarios.build(variant='plain', seed=0, prob=prob)
    kw.update(resident=dict(pod=SnapshotPOD(M, every=2), rom=gr))
    with pytest.raises(ValueError) as exc:
        tiu.sbdftwo(**kw)
    assert '`rom`' in str(exc.value) and 'device_convection' in str(exc.value)


def test_a_loop_that_breaks_off_reports_no_rom_and_no_keys_without_it(
        tiu, toy_prob):
    from dolfin_navier_scipy_amd.fem import SnapshotPOD, GalerkinROM
    prob = toy_prob
    M, A = (sps.csr_matrix(prob['smc'][k]) for k in ('M', 'A'))
    gr = GalerkinROM(A, prob['rhsd']['fv'])
    kw, _ = _stepwise_kw(prob, dict(pod=SnapshotPOD(M, every=2), rom=gr),
                         check_ff_maxv=1e-3, ntimeslices=3)
    _, _, ff = tiu.cnab(**kw)
    assert ff == 1
    assert tiu.LAST_RUN['rom'] is None and tiu.LAST_RUN['pod'] is None
    assert 'rom_on' in tiu.LAST_RUN
    kw, _ = _stepwise_kw(prob, dict(pod=SnapshotPOD(M, every=2)))
    tiu.cnab(**kw)
    assert not [k for k in tiu.LAST_RUN if k.startswith('rom')]
    assert tiu.LAST_RUN['pod'] is not None
