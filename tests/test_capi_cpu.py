"""CPU-side checks of the boundary: the library builds for gfx950, loads, and
exports every symbol `include/dns_amd.h` declares; host-only argument checks."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def capi():
    from dolfin_navier_scipy_amd.build import build_library
    build_library(verbose=False)
    from dolfin_navier_scipy_amd import _capi
    _capi.load_library()
    return _capi


def test_header_symbols_all_exported(capi):
    hdr = open(os.path.join(ROOT, 'include', 'dns_amd.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(dns_[a-z0-9_]+)\s*\(', hdr))
    assert declared, 'no declarations parsed'
    assert declared == set(capi.SIGNATURES.keys())
    lib = capi.load_library()
    for name in declared:
        assert hasattr(lib, name), name


def test_status_strings_and_defaults(capi):
    lib = capi.load_library()
    assert lib.dns_version() >= 100
    assert lib.dns_status_string(0) == b'ok'
    assert lib.dns_status_string(1) == b'not converged'
    import ctypes as ct
    o = capi.dns_solve_opts()
    lib.dns_default_solve_opts(ct.byref(o))
    assert o.restart <= 64 and o.rtol > 0 and o.maxiter > 0
    p = capi.dns_precond_opts()
    lib.dns_default_precond_opts(ct.byref(p))
    assert p.cheb_degree >= 1


def test_struct_layout_matches_header(capi):
    import ctypes as ct
    assert ct.sizeof(capi.dns_csr) == 40
    assert ct.sizeof(capi.dns_precond_opts) == 64
    assert ct.sizeof(capi.dns_solve_opts) == 40
    assert ct.sizeof(capi.dns_solve_stats) == 48
    assert ct.sizeof(capi.dns_imex_coeffs) == 48
    assert ct.sizeof(capi.dns_spmv_epi) == 176


def test_null_and_bad_arguments_fail_cleanly(capi):
    import ctypes as ct
    lib = capi.load_library()
    assert lib.dns_saddle_solve(None, None, None, None, None, None, None) \
        == capi.DNS_ERR_BAD_ARGUMENT
    assert b'null' in lib.dns_last_error()
    assert lib.dns_saddle_setup_precond(None, None) == capi.DNS_ERR_BAD_ARGUMENT
    out = ct.c_void_p()
    assert lib.dns_saddle_create(0, None, None, None, ct.byref(out)) \
        == capi.DNS_ERR_BAD_ARGUMENT
    # malformed CSR is rejected on the host before any device work
    A = sps.identity(4, format='csr')
    view = capi.CsrView(A)
    view.indices[2] = 9
    x = np.ones(4)
    y = np.zeros(4)
    st = lib.dns_spmv(0, view.byref(), capi.dptr(x), capi.dptr(y), 1.0, 0.0, 0)
    assert st == capi.DNS_ERR_BAD_ARGUMENT
    # the epilogue entry: null arguments, a malformed matrix, and combinations
    # the chosen kernel does not implement
    assert lib.dns_spmv_epilogue(0, None, None, None, None, None, None, None,
                                 None) == capi.DNS_ERR_BAD_ARGUMENT
    good = capi.CsrView(A)
    npb, nbl = ct.c_int32(0), ct.c_int32(0)

    def epi(v=good, **kw):
        e = capi.dns_spmv_epi(ny=4, grid_cap=8, nvl=-1, alpha=1.0)
        for k, val in kw.items():
            setattr(e, k, val)
        return lib.dns_spmv_epilogue(0, v.byref(), ct.byref(e), capi.dptr(x),
                                     capi.dptr(y), None, None, ct.byref(npb),
                                     ct.byref(nbl))
    d = capi.dptr(np.ones(4))
    for bad in (dict(v=view), dict(kernel=2), dict(mode=3), dict(grid_cap=0),
                dict(ny=5), dict(nvec=1), dict(with_bb=1), dict(beta=1.0),
                dict(mode=1), dict(mode=1, dinv=d, b=d, beta=1.0),
                dict(mode=2, dinv=d, b=d, xin=d), dict(x2=d, nsplit=4),
                dict(map_on=1, row0=2, len1=4),
                dict(kernel=1, nv=2, mode=1, dinv=d, b=d),
                dict(kernel=1, nv=2, x2=d, nsplit=2),
                dict(kernel=1, nv=2, fp32_vals=1),
                dict(kernel=1, nv=2, map_on=1, len1=4),
                dict(kernel=1, nv=2, nvl=2, v0=2, p0=0)):
        assert epi(**bad) == capi.DNS_ERR_BAD_ARGUMENT, bad


def test_assembly_probe_checks_its_arguments_on_the_host(capi):
    import ctypes as ct
    lib = capi.load_library()
    pr = capi.dns_trap_probe()
    assert ct.sizeof(pr) == 96
    assert lib.dns_trap_assembly_probe(None, 1e-3, 0, 0, 0, None,
                                       ct.byref(pr)) \
        == capi.DNS_ERR_BAD_ARGUMENT
    assert lib.dns_trap_assembly_probe(None, 1e-3, 0, 0, 0, None, None) \
        == capi.DNS_ERR_BAD_ARGUMENT


def test_front_probe_checks_its_arguments_on_the_host(capi):
    import ctypes as ct
    lib = capi.load_library()
    pr = capi.dns_imex_probe()
    # (18 pointers, 14 words; appended: 2 pointers, rowmap[4], 4 words -- the
    # offsets from before keep their place)
    assert ct.sizeof(pr) == 248
    assert type(pr).parts_cap.offset == 144 and type(pr).pad.offset == 196
    assert type(pr).r_in.offset == 200 and type(pr).x0copy.offset == 208
    assert type(pr).rowmap.offset == 216 and type(pr).dcarry.offset == 232
    assert type(pr).nsel.offset == 244
    cf = capi.dns_imex_coeffs(a_c=1.)
    assert lib.dns_imex_front_probe(None, ct.byref(cf), None, 0, None,
                                    ct.byref(pr)) == capi.DNS_ERR_BAD_ARGUMENT
    assert lib.dns_imex_front_probe(None, None, None, 0, None, None) \
        == capi.DNS_ERR_BAD_ARGUMENT


def test_no_device_is_loud(capi):
    """without a GPU the product path must raise, never fall back"""
    if capi.device_count() > 0:
        pytest.skip('a GPU is present')
    from dolfin_navier_scipy_amd import saddle
    A = sps.identity(4, format='csr')
    J = sps.csr_matrix(np.ones((1, 4)))
    with pytest.raises(capi.DnsError):
        saddle.SaddleSystem(A, J)
    from dolfin_navier_scipy_amd import lin_alg_utils as lau
    with pytest.raises(capi.DnsError):
        lau.solve_sadpnt_smw(amat=A, jmat=J, rhsv=np.ones((4, 1)))


def test_install_as_lau():
    import sys
    import dolfin_navier_scipy_amd as pkg
    mod = pkg.install_as_lau()
    import sadptprj_riclyap_adi.lin_alg_utils as lau
    assert lau is mod
    for name in ('solve_sadpnt_smw', 'app_prj_via_sadpnt',
                 'SpslaKrylovCounter', 'apply_massinv'):
        assert hasattr(lau, name)
    sys.modules.pop('sadptprj_riclyap_adi.lin_alg_utils')
    sys.modules.pop('sadptprj_riclyap_adi')


def test_product_does_not_import_oracle():
    pkgdir = os.path.join(ROOT, 'dolfin_navier_scipy_amd')
    for dirpath, _, files in os.walk(pkgdir):
        for fn in files:
            if fn.endswith('.py'):
                src = open(os.path.join(dirpath, fn)).read()
                assert 'import oracle' not in src and 'from oracle' not in src
                assert 'krylov_model' not in src


def test_pattern_helpers_of_the_newton_picard_module():
    """host logic of `newton_picard`: union pattern with explicit zeros kept,
    values laid out in a super-pattern"""
    import scipy.sparse as sps
    from dolfin_navier_scipy_amd import newton_picard as dnp
    rng = np.random.default_rng(0)
    A = sps.random(40, 40, density=0.1, format='csr', random_state=rng)
    B = sps.random(40, 40, density=0.1, format='csr', random_state=rng)
    B.data[::3] = 0.                      # explicit zeros must stay
    P = dnp.union_pattern(A, B)
    assert P.has_canonical_format and np.all(P.data == 1.)
    want = set(zip(*A.nonzero())) | set(
        zip(np.repeat(np.arange(40), np.diff(B.indptr)), B.indices))
    got = set(zip(np.repeat(np.arange(40), np.diff(P.indptr)), P.indices))
    assert got == want
    va, vb = dnp.values_in_pattern(A, P), dnp.values_in_pattern(B, P)
    rebuilt = sps.csr_matrix((va + 2*vb, P.indices, P.indptr), shape=P.shape)
    assert abs(rebuilt - (A + 2*B)).max() <= 1e-15
    with pytest.raises(ValueError):
        dnp.values_in_pattern(sps.identity(40, format='csr') + A,
                              dnp.union_pattern(A))


def test_pressure_prolongations_of_a_refined_mesh():
    """input of the multigrid Schur block: P1 prolongations between nested
    pressure spaces in the spaces' own (RCM) dof numbering"""
    from dolfin_navier_scipy_amd.fem import (
        channel_cylinder_mesh, refine_uniform, TaylorHood,
        pressure_prolongations)
    coarse = channel_cylinder_mesh()
    mid, par1 = refine_uniform(coarse)
    fine, par2 = refine_uniform(mid)
    spaces = [TaylorHood(fine), TaylorHood(mid), TaylorHood(coarse)]
    prols = pressure_prolongations(spaces, [par2, par1, None])
    assert [p.shape for p in prols] == [(fine.nverts, mid.nverts),
                                        (mid.nverts, coarse.nverts)]
    for l, P in enumerate(prols):
        assert np.abs(np.asarray(P.sum(axis=1)).ravel() - 1.).max() < 1e-15
        assert P.data.min() >= 0.5 - 1e-15 and P.data.max() <= 1. + 1e-15
        # affine functions are reproduced (straight edges: exactly)
        fs, cs = spaces[l], spaces[l + 1]
        xc = np.empty(cs.pdim)
        xc[cs.vert_pdof] = 2*cs.mesh.verts[:, 0] - cs.mesh.verts[:, 1] + 3
        xf = np.empty(fs.pdim)
        xf[fs.vert_pdof] = 2*fs.mesh.verts[:, 0] - fs.mesh.verts[:, 1] + 3
        assert np.abs(P @ xc - xf).max() < 1e-12


def test_build_dependencies_cover_every_include():
    """`needs_build()` must see every file the translation unit includes
    (a hand-kept list once missed trap.hpp / trap_capi.inc)"""
    from dolfin_navier_scipy_amd import build
    deps = set(os.path.realpath(p) for p in build.dependencies())
    seen, todo = set(), [os.path.join(build.CSRC, s) for s in build.SOURCES]
    while todo:
        path = os.path.realpath(todo.pop())
        if path in seen:
            continue
        seen.add(path)
        for inc in re.findall(r'#include\s+"([^"]+)"', open(path).read()):
            todo.append(os.path.join(os.path.dirname(path), inc))
    assert len(seen) > 10
    missing = seen - deps
    assert not missing, missing


def test_spawn_retry_only_for_rendezvous_errors():
    import spawn_util
    assert spawn_util.is_rendezvous_error(
        RuntimeError('The server socket has failed to bind to [::]:29500 '
                     '(errno: 98 - Address already in use)'))
    assert not spawn_util.is_rendezvous_error(
        RuntimeError('process 1 terminated with signal SIGABRT'))
    assert not spawn_util.is_rendezvous_error(AssertionError('1e-3 > 1e-9'))


def test_every_host_copy_goes_through_common_hpp():
    """The DMA engine never sees a caller's or a stack's pageable memory:
    outside `common.hpp` (the staged and pinned copies) no `hipMemcpy*` call
    moves bytes between host and device, nothing pins host memory in place,
    and the removed enqueue-only upload is not back"""
    csrc = os.path.join(ROOT, 'dolfin_navier_scipy_amd', 'csrc')
    paths = sorted(os.path.join(csrc, f) for f in os.listdir(csrc)
                   if f.endswith(('.hip', '.inc', '.hpp')))
    assert len(paths) > 10
    bad = []
    for path in paths:
        name = os.path.basename(path)
        text = open(path).read()
        for word in ('hipHostRegister', 'upload_async', 'SyncOnExit'):
            if word in text:
                bad.append('%s: %s' % (name, word))
        if name == 'common.hpp':
            continue
        code = re.sub(r'//[^\n]*|/\*.*?\*/', ' ', text, flags=re.S)
        for m in re.finditer(r'\b(hipMemcpy\w*)\s*\(', code):
            depth, end = 0, m.end() - 1
            while True:                  # through to the closing parenthesis
                depth += {'(': 1, ')': -1}.get(code[end], 0)
                if depth == 0:
                    break
                end += 1
            call = code[m.start():end + 1]
            fn = m.group(1)
            if (re.search(r'hipMemcpy(HostToDevice|DeviceToHost|Default)\b',
                          call) or re.search(r'(To|From)Symbol|HtoD|DtoH', fn)):
                line = code.count('\n', 0, m.start()) + 1
                bad.append('%s:%d: %s' % (name, line, ' '.join(call.split())))
    assert not bad, '\n'.join(bad)


def _csrc_code():
    """{file name: text without comments} of every source file of the library"""
    csrc = os.path.join(ROOT, 'dolfin_navier_scipy_amd', 'csrc')
    return {f: re.sub(r'//[^\n]*|/\*.*?\*/', ' ',
                      open(os.path.join(csrc, f)).read(), flags=re.S)
            for f in sorted(os.listdir(csrc))
            if f.endswith(('.hip', '.inc', '.hpp'))}


def test_every_status_export_is_an_exception_barrier():
    """`DNS_ERR_HOST`: no C++ exception crosses the boundary.  Every export
    that returns a status is a function-try-block closed by DNS_CAPI_CATCH
    (status.hpp), with its body in place: no `_impl` twin behind a forwarding
    wrapper, no `dns::guarded` lambda"""
    import ctypes as ct
    from dolfin_navier_scipy_amd import _capi
    code = _csrc_code()
    assert len(code) > 10
    names = [n for n, (restype, _) in _capi.SIGNATURES.items()
             if restype is ct.c_int and n != 'dns_version']
    assert len(names) > 90
    bad = []
    for name in names:
        found = [(f, m) for f, text in code.items()
                 for m in re.finditer(r'^int %s\(' % name, text, flags=re.M)]
        if len(found) != 1:
            bad.append('%s: %d definitions' % (name, len(found)))
            continue
        f, m = found[0]
        text = code[f]
        brace = text.index('{', m.start())
        if not re.search(r'\)\s*try\s*$', text[m.start():brace]):
            bad.append('%s (%s): no function-try-block' % (name, f))
            continue
        # the body ends at the first brace in column 0
        close = re.compile(r'^\}.*$', flags=re.M).search(text, brace)
        if close.group(0).split() != ['}', 'DNS_CAPI_CATCH']:
            bad.append('%s (%s): closed by %r' % (name, f, close.group(0)))
    for f, text in code.items():
        for m in re.finditer(r'\bdns_\w+_impl\b|\bdns::guarded\b|'
                             r'\bint guarded\s*\(', text):
            bad.append('%s:%d: %s' % (f, text.count('\n', 0, m.start()) + 1,
                                      m.group(0)))
    assert not bad, '\n'.join(bad)


def test_create_functions_own_their_handle():
    """A handle is held in a `std::unique_ptr` from `std::make_unique` until it
    is released into `*out`: an exception on the way (it arrives as
    DNS_ERR_HOST) does not leak it.  No raw `new` of a handle type is left
    where the create functions live"""
    code = _csrc_code()
    handles = ('dns_saddle', 'dns_imex', 'dns_trap', 'dns_conv', 'dns_conv_mat',
               'dns_op', 'dns_bcmap', 'dns_comm')
    files = [f for f in code if f.endswith('_capi.inc')] \
        + ['rank_local.inc', 'dns_amd.hip']
    assert len(files) == 7
    bad, made = [], set()
    for f in files:
        text = code[f]
        for m in re.finditer(r'\bnew\b\s*(\(\s*std::nothrow\s*\))?\s*([\w:]+)',
                             text):
            if m.group(2) in handles + ('T',):
                bad.append('%s:%d: %s' % (f, text.count('\n', 0, m.start()) + 1,
                                          m.group(0)))
        made.update(re.findall(r'std::make_unique<(\w+)>\(\)', text))
        # inside a create function: no `new` at all
        for m in re.finditer(r'^(?:static )?int (\w*create\w*)\(', text,
                             flags=re.M):
            end = re.compile(r'^\}', flags=re.M).search(text, m.end()).start()
            if re.search(r'\bnew\b', text[m.end():end]):
                bad.append('%s: new in %s' % (f, m.group(1)))
    assert not bad, '\n'.join(bad)
    assert made == set(handles), made
