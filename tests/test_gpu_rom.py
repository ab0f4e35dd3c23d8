"""POD-Galerkin projection on the device: `saddle.ensemble_project` (`X W Y^T`,
the non-mirroring form of the Gram kernels), `ConvectionP2.project_tensor`
(`k_rom_tensor` / `k_rom_reduce`) against the long double model `rom_model`
at the tile, chunk and padding edges, and `resident=dict(pod=, rom=)` through
`cnab` / `sbdftwo` on the toy wake.

Worst error / bound of the tensor against the model (printed with `pytest
-s`): see profiles/r16_rom/README.md."""
import numpy as np
import pytest
import scipy.sparse as sps

import conv_meshes
import conv_model
import pod_model
import rom_model
import scenarios

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0**-53
CHUNK = 1024                    # kEnsChunk of csrc/ensemble_host.hpp
NV_CHUNKS = 2*CHUNK + 37        # three k-chunks, a ragged last one
C = 512                         # kRomCellChunk of csrc/galerkin_host.hpp
NST, EVERY = 24, 2


@pytest.fixture(scope='module')
def gtiu():
    from dolfin_navier_scipy_amd import time_int_utils, _capi
    from dolfin_navier_scipy_amd.fem import rom
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    assert rom.ROM_CELL_CHUNK == C
    return time_int_utils


# ---- 1. X W Y^T --------------------------------------------------------------------

def _padded(S, ld):
    E = np.full((S.shape[0], ld), np.nan)
    E[:, :S.shape[1]] = S
    return E


def _ld_for(nv):
    return nv + 2 + (nv % 2)                # even, > nv


def _int_weights(nv, rng):
    """small-integer NON-symmetric CSR with an empty row"""
    dens = min(1., 6./nv)
    A = sps.random(nv, nv, density=dens, random_state=rng,
                   data_rvs=lambda k: rng.integers(-2, 3, size=k).astype(
                       np.float64))
    W = sps.lil_matrix((A + sps.diags(rng.integers(1, 4, size=nv))
                        ).astype(np.float64))
    if nv > 1:
        W[nv//2, :] = 0.
        W[0, nv - 1] = 2.                   # (never symmetric)
        W[nv - 1, 0] = 0. if nv//2 == nv - 1 else -1.
    W = sps.csr_matrix(W)
    W.eliminate_zeros()
    assert nv == 1 or (np.diff(W.indptr).min() == 0 and abs(W - W.T).nnz > 0)
    return W


@pytest.mark.parametrize('nv', [1, 3, 63, 64, 65, NV_CHUNKS])
def test_project_is_exact_on_integer_data(gtiu, nv):
    from dolfin_navier_scipy_amd import saddle
    rng = np.random.default_rng(500 + nv)
    W = _int_weights(nv, rng)
    sizes = (1, 15, 16, 17, 33)
    rows = {m: rng.integers(-3, 4, size=(m, nv)).astype(np.float64)
            for m in sizes}
    ld = _ld_for(nv)
    for mx in sizes:
        X = rows[mx]
        for my in sizes:
            Y = rows[my][::-1].copy()
            for what, Wk in (('W = I', None), ('W', W)):
                P = saddle.ensemble_project(_padded(X, ld), _padded(Y, ld),
                                            Wk, nv=nv)
                want = X @ Y.T if Wk is None else X @ (Wk @ Y.T)
                assert P.shape == (mx, my)
                assert np.isfinite(P).all(), (what, 'the padding was read')
                assert np.array_equal(P, want), (mx, my, what)
        P = saddle.ensemble_project(_padded(X, ld), None, W, nv=nv)
        assert np.array_equal(P, X @ (W @ X.T)), mx


def test_project_holds_the_bits_of_the_gram_matrix(gtiu):
    """`X = Y`, `W` symmetric: every entry of a tile with `ib <= jb` (of the
    diagonal tiles the upper triangle) is `ensemble_gram`'s, bit for bit"""
    from dolfin_navier_scipy_amd import saddle
    m, nv = 33, NV_CHUNKS
    rng = np.random.default_rng(77)
    S = rng.standard_normal((m, nv))*np.exp(rng.standard_normal((m, 1)))
    A = sps.random(nv, nv, density=8./nv, random_state=rng,
                   data_rvs=rng.standard_normal)
    W = sps.csr_matrix(A + A.T + 4.*sps.identity(nv))
    E = _padded(S, _ld_for(nv))
    for Wk in (None, W):
        G = saddle.ensemble_gram(E, Wk, nv=nv)
        P = saddle.ensemble_project(E, None, Wk, nv=nv)
        P2 = saddle.ensemble_project(E, E.copy(), Wk, nv=nv)
        assert np.array_equal(P, P2)
        i, j = np.triu_indices(m)
        assert np.array_equal(P[i, j], G[i, j])
        # (below the diagonal blocks the project kernel sums the other
        # operand order: equal within the bound, not asserted bit for bit)


@pytest.mark.parametrize('mx,my,nv', [(17, 33, 65), (33, 16, NV_CHUNKS)])
def test_project_within_its_bound_on_real_data(gtiu, mx, my, nv):
    from dolfin_navier_scipy_amd import saddle
    from dolfin_navier_scipy_amd.fem import rom
    rng = np.random.default_rng(9 + nv)
    X = rng.standard_normal((mx, nv))*np.exp(rng.standard_normal((mx, 1)))
    Y = rng.standard_normal((my, nv))*np.exp(rng.standard_normal((my, 1)))
    W = sps.csr_matrix(sps.random(nv, nv, density=min(1., 8./nv),
                                  random_state=rng,
                                  data_rvs=rng.standard_normal)
                       + 4.*sps.identity(nv))
    ld = _ld_for(nv)
    worst = {}
    for what, Wk in (('W = I', None), ('W', W)):
        P = saddle.ensemble_project(_padded(X, ld), _padded(Y, ld), Wk, nv=nv)
        assert np.array_equal(P, saddle.ensemble_project(
            _padded(X, ld), _padded(Y, ld), Wk, nv=nv)), what
        Wd = np.eye(nv) if Wk is None else Wk.toarray()
        want = X.astype(LD) @ (Wd.astype(LD) @ Y.astype(LD).T)
        err = np.abs(P.astype(LD) - want)
        bound = rom.bound_project(X, Y, Wk)
        worst[what] = float((err/bound).max())
        assert np.all(err <= bound), (what, worst[what])
    print('mx', mx, 'my', my, 'nv', nv, ': worst error / bound', worst)


# ---- 2. the tensor against the model ----------------------------------------------------

SPLITS = dict(boundary=dict(dirichlet='boundary'), none=dict(dirichlet='none'),
              mixed=dict(dirichlet=0.3, full_cells=2))
# (mesh, split, rows of the model): the chunk edges with every cell live
# (`none`), the cells without an inner dof (`mixed`); the long double model of
# 33 rows takes 2.3 s at 1025 cells, once per case
CASES = (('rect', 1, 'none', 33), ('rect', 2, 'boundary', 33),
         ('rect', 2, 'none', 33), ('rect', C - 1, 'none', 33),
         ('rect', C, 'none', 33), ('rect', C + 1, 'none', 33),
         ('rect', C + 1, 'boundary', 33), ('rect', 2*C + 1, 'none', 33),
         ('rect', 2*C + 1, 'mixed', 33), ('fan', 40, 'boundary', 33),
         ('fan', 40, 'none', 33), ('fan', 40, 'mixed', 33))
SHAPES = ((1, 1), (2, 1), (2, 2), (15, 1), (15, 15), (16, 1), (16, 16),
          (17, 1), (17, 17), (33, 1), (33, 17), (33, 33))


def _device_conv(mesh, inv, dbc, dbcvals=None):
    from dolfin_navier_scipy_amd import convection
    return convection.ConvectionP2(
        mesh.cell_vdofs, mesh.glam, mesh.area, mesh.vdim, inv, dbc,
        np.zeros(dbc.size) if dbcvals is None else dbcvals)


_MODELS = {}


def _model(case):
    """mesh, split, device operator data and the long double tensor of `rows`
    seeded rows, computed once per case"""
    if case not in _MODELS:
        kind, nc, split, rows = case
        mesh = conv_meshes.rectangle(nc, seed=3) if kind == 'rect' \
            else conv_meshes.fan(nc, seed=5)
        k = CASES.index(case)
        inv, dbc = mesh.split(seed=k, **SPLITS[split])
        hc = rom_model.HostConv.from_mesh(mesh, inv, dbc)
        B, D = rom_model.seeded_basis(rows, hc.nv, hc.ndbc,
                                      seed=100 + k)
        T = rom_model.tensor_longdouble(hc.space(), B, D)
        _MODELS[case] = (mesh, inv, dbc, hc, B, D, T)
    return _MODELS[case]


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%s%d-%s' % c[:3])
def test_tensor_against_the_long_double_model(gtiu, case):
    """every `(nb, nt)` the case's rows allow: the leading rows of one seeded
    basis, whose tensor is the leading block of the model's"""
    from dolfin_navier_scipy_amd.fem import rom
    mesh, inv, dbc, hc, B, D, T = _model(case)
    conv = _device_conv(mesh, inv, dbc)
    worst = 0.
    try:
        bound_all = rom.bound_tensor(hc, B, D)
        for nb, nt in SHAPES:
            if nb > B.shape[0]:
                continue
            got = conv.project_tensor(B[:nb], D[:nb], ntest=nt)
            assert got.shape == (nt, nb, nb)
            r = conv_model.ratio(got, T[:nt, :nb, :nb],
                                 bound_all[:nt, :nb, :nb])
            worst = max(worst, r)
            assert r <= 1., (nb, nt, r)
        # no Dirichlet rows: zeros
        nb = min(5, B.shape[0])
        got = conv.project_tensor(B[:nb], None)
        want = rom_model.tensor_longdouble(hc.space(), B[:nb], None)
        r = conv_model.ratio(got, want, rom.bound_tensor(hc, B[:nb], None))
        worst = max(worst, r)
        assert r <= 1., r
    finally:
        conv.close()
    print(case, ': worst error / bound', worst)


def _far_apart_cells(mesh, count):
    """cells no two of which touch a common cell (or each other)"""
    inc = sps.csr_matrix((np.ones(mesh.cellnodes.size),
                          (np.repeat(np.arange(mesh.ncells), 6),
                           mesh.cellnodes.ravel())),
                         shape=(mesh.ncells, mesh.nnodes))
    adj = (inc @ inc.T).tocsr()
    two = (adj @ adj).tocsr()
    chosen, blocked = [], np.zeros(mesh.ncells, dtype=bool)
    for c in range(mesh.ncells):
        if not blocked[c]:
            chosen.append(c)
            blocked[two[c].indices] = True
            if len(chosen) == count:
                return chosen
    raise AssertionError('mesh too small')


def test_index_placement_with_disjoint_supports(gtiu):
    """rows 2p and 2p + 1 live on the dofs of one cell `c_p`, the cells far
    apart: `T[i, j, k]` is non-zero only where i, j, k belong to one pair, and
    there every wrong placement or `j <-> k` swap is off by orders of
    magnitude of the bound; the zeros are exact zeros"""
    from dolfin_navier_scipy_amd.fem import rom
    mesh = conv_meshes.rectangle(2*C + 1, seed=3)
    inv, dbc = mesh.split(dirichlet='none', seed=1)
    hc = rom_model.HostConv.from_mesh(mesh, inv, dbc)
    nb = 33
    cells = _far_apart_cells(mesh, 17)
    code = np.full(mesh.vdim, -1, dtype=np.int64)
    code[inv] = np.arange(inv.size)
    rng = np.random.default_rng(5)
    B = np.zeros((nb, hc.nv))
    for b in range(nb):
        dofs = code[mesh.cell_vdofs[cells[b//2]].ravel()]
        B[b, dofs] = rng.standard_normal(12) + (1. if b % 2 else -1.)
    conv = _device_conv(mesh, inv, dbc)
    try:
        for nt in (nb, 17):
            T = conv.project_tensor(B, None, ntest=nt)
            want = rom_model.tensor_longdouble(hc.space(), B, None, nt)
            bound = rom.bound_tensor(hc, B, None, ntest=nt)
            pair = np.arange(nb)//2
            same = (pair[:nt, None, None] == pair[None, :, None]) \
                & (pair[None, :, None] == pair[None, None, :])
            assert np.all(T[~same] == 0.)
            assert np.all(want[~same] == 0.) and np.all(bound[~same] == 0.)
            assert np.all(T[same] != 0.)
            assert conv_model.ratio(T, want, bound) <= 1.
            # a swap of j and k (where they differ) is far outside the bound
            swapped = np.abs(T.transpose(0, 2, 1).astype(LD) - want)
            offd = same & (np.arange(nb)[None, :, None]
                           != np.arange(nb)[None, None, :])
            assert offd.sum() >= 2*(nt - 1)     # (two per row of a pair)
            assert np.median(swapped[offd]/bound[offd]) > 1e3
    finally:
        conv.close()


def test_contraction_against_the_operators_own_convection(gtiu):
    """`sum_jk a_j a_k T[i, j, k]` against `B[i] . conv.apply(u)`, `u = a^T
    B` with the Dirichlet values `a^T D` (coefficients and entries on a grid
    of 2^-20: `u` is exact), within `bound_tensor` contracted plus
    `conv_model`'s `K_VEC` bound of `N(u)u` contracted with `|B[i]|` and the
    dot products' own roundings"""
    from dolfin_navier_scipy_amd.fem import rom
    mesh, inv, dbc, hc, B, D, _ = _model(('fan', 40, 'mixed', 33))
    nb, nt = 17, 17
    B = np.round(B[:nb]*2.**20)/2.**20
    D = np.round(D[:nb]*2.**20)/2.**20
    a = np.random.default_rng(8).choice([-2., -1., -.5, .5, 1., 2.], size=nb)
    u, du = a @ B, a @ D
    assert np.array_equal(u.astype(LD), a.astype(LD) @ B.astype(LD))
    conv = _device_conv(mesh, inv, dbc)
    try:
        T = conv.project_tensor(B, D, ntest=nt)
        conv.set_dbcvals(du)
        nuu = conv.apply(u)[:, 0]
    finally:
        conv.close()
    got = np.einsum('ijk,j,k->i', T, a, a)
    aa = np.abs(a)
    BT = rom.bound_tensor(hc, B, D, ntest=nt)
    Ta = rom.tensor_host(hc, B, D, ntest=nt, absval=True)
    vec, vbound = conv_model.conv_model(hc.space(), u, du)['vec']
    tol = np.einsum('ijk,j,k->i', BT, aa, aa) \
        + 1.01*(nb*nb + 4)*U*np.einsum('ijk,j,k->i', Ta, aa, aa) \
        + np.abs(B[:nt]) @ (vbound.astype(np.float64)
                            + 1.01*(hc.nv + 2)*U*np.abs(nuu))
    err = np.abs(B[:nt] @ nuu - got)
    print('contraction: worst error / tolerance', float((err/tol).max()))
    assert np.all(err <= tol)
    assert np.abs(got).min() > 0.


def test_the_same_call_gives_the_same_bits(gtiu):
    mesh, inv, dbc, hc, B, D, _ = _model(('rect', 2*C + 1, 'mixed', 33))
    conv = _device_conv(mesh, inv, dbc)
    other = _device_conv(mesh, inv, dbc, dbcvals=np.ones(dbc.size))
    try:
        B, D = B[:17], D[:17]
        T1 = conv.project_tensor(B, D, ntest=16)
        T2 = conv.project_tensor(B, D, ntest=16)
        T3 = other.project_tensor(B, D, ntest=16)
        assert np.array_equal(T1, T2) and np.array_equal(T1, T3)
        # refusals are host-side argument checks: the operator goes on as
        # before
        from dolfin_navier_scipy_amd import _capi as Cm
        lib = conv.lib
        Bp = np.ascontiguousarray(np.hstack([B, np.zeros((17, hc.nv % 2))]))
        out = np.zeros(17**3)
        for nb, nt, ld in ((34, 1, Bp.shape[1]), (17, 18, Bp.shape[1]),
                           (17, 0, Bp.shape[1]), (17, 17, hc.nv - 2)):
            assert lib.dns_conv_project_tensor(
                conv._h, nb, nt, ld, Cm.dptr(Bp.reshape(-1)), None,
                Cm.dptr(out)) == Cm.DNS_ERR_BAD_ARGUMENT
            assert b'galerkin' in lib.dns_last_error()
        with pytest.raises(ValueError):
            conv.project_tensor(np.zeros((34, hc.nv)))
        with pytest.raises(ValueError):
            conv.project_tensor(B, D[:, :-1])
        assert np.array_equal(T1, conv.project_tensor(B, D, ntest=16))
    finally:
        conv.close()
        other.close()


# ---- 3. through the loops ----------------------------------------------------------------

def _toy_cvop(prob):
    from dolfin_navier_scipy_amd import convection
    return convection.ConvectionP2.from_taylor_hood(
        prob['th'], prob['invinds'], prob['dbcinds'], prob['dbcvals'])


def _femp(prob):
    return dict(V=prob['th'], invinds=prob['invinds'],
                dbcinds=prob['dbcinds'], dbcvals=prob['dbcvals'],
                nu=prob['nu'])


def _projection_identity(gr, hc, dbcvals, a, bo):
    """as tests/test_rom_cpu.py: `rhs(a)` against the full operators in long
    double, within the contracted bounds"""
    sp = hc.space()
    modes, mean = gr.modes.astype(LD), gr.mean.astype(LD)
    uL = mean + np.asarray(a, dtype=np.float64).astype(LD) @ modes
    full = np.zeros(hc._vdim, dtype=LD)
    full[hc._invinds] = uL
    full[hc._dbcinds] = np.asarray(dbcvals, dtype=np.float64)
    ul = full[hc._cell_vdofs].reshape(hc.ncells, 6, 2)
    vec, _, _ = conv_model.cell_quantities(sp.glam, sp.area, ul, LD)
    A = gr.A
    Au = conv_model._spmv(A.indptr, A.indices, A.data.astype(LD), uL)
    want = -(modes @ (Au + sp.gather_rows(vec) - gr.fv.astype(LD)))
    o, aa = gr.ops, np.abs(np.asarray(a, dtype=np.float64))
    r = aa.size
    mag = np.abs(o['Ar']) @ aa + np.abs(o['b0']) + np.abs(o['c']) \
        + np.abs(o['L']) @ aa + (np.abs(o['H']) @ aa) @ aa
    tol = bo['Ar'] @ aa + bo['b0'] + bo['c'] + bo['L'] @ aa \
        + (bo['H'] @ aa) @ aa + 1.01*(r*r + r + 6)*U*mag
    return np.abs(gr.rhs(a).astype(LD) - want).astype(np.float64), tol


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_rom_through_the_time_loops(gtiu, toy_prob, scheme):
    """24 steps of the toy wake with the device convection: the projection
    runs on the device, every array inside its bound of the host model on the
    same modes; functionals, quadratics and statistics beside it say what
    they say without it, and so does the final state"""
    from dolfin_navier_scipy_amd import fem
    integ = gtiu.cnab if scheme == 'cnab' else gtiu.sbdftwo
    prob = toy_prob
    th, inv = prob['th'], prob['invinds']
    M, A = (sps.csr_matrix(prob['smc'][k]) for k in ('M', 'A'))
    fv = prob['rhsd']['fv']
    runs = {}
    for mode in ('rom', 'pod'):
        kw, rec, _ = scenarios.build(variant='plain', seed=0, prob=prob,
                                     Nts=NST + 1, tE=0.005*(NST + 1))
        kw.pop('f_vdp')
        pod = fem.SnapshotPOD(M, every=EVERY, nmodes=3)
        gr = fem.GalerkinROM(A, fv, J=prob['smc']['J'])
        qf = fem.kinetic_energy(th, _femp(prob)) \
            + fem.dissipation(th, _femp(prob))
        fn = fem.pressure_difference(th, 3, 5)
        fs = fem.FlowStatistics(pairs=fem.component_pairs(th, inv), nbins=1)
        rsd = dict(savevp_times=(), pod=pod, functionals=fn, quadratics=qf,
                   statistics=fs)
        if mode == 'rom':
            rsd.update(rom=gr)
        cvop = _toy_cvop(prob)
        try:
            v, p, ff = integ(ntimeslices=3, resident=rsd, device_convection=cvop,
                             invinds=inv, **kw)
        finally:
            cvop.close()
        assert ff == 0
        runs[mode] = (dict(gtiu.LAST_RUN), v, p, gr, pod)
    lr, v, p, gr, pod = runs['rom']
    lp, vp, pp = runs['pod'][:3]
    assert lr['pod_on'] == 'device' and lr['rom_on'] == 'device'
    assert not [k for k in lp if k.startswith('rom')]
    assert np.array_equal(v, vp) and np.array_equal(p, pp)
    assert lr['run_calls'] == lp['run_calls'] > 0
    for key in ('functionals', 'quadratics'):
        assert lr[key].shape[0] == NST and np.array_equal(lr[key], lp[key])
    for k in lr['statistics']:
        a, b = lr['statistics'][k], lp['statistics'][k]
        assert (a is None and b is None) or np.array_equal(a, b), k
    assert np.array_equal(lr['pod']['gram'], lp['pod']['gram'])
    ops, res = lr['rom'], lr['pod']
    r = res['modes'].shape[0]
    assert r == 3 and sorted(ops) == ['Ar', 'H', 'L', 'Mr', 'b0', 'c', 'div']
    # the host model on the same modes and mean
    hc = rom_model.HostConv.from_taylor_hood(th, inv, prob['dbcinds'],
                                             prob['dbcvals'])
    host = fem.GalerkinROM(A, fv, M=M, J=prob['smc']['J'])
    hops = host.project(res['modes'], res['mean'], hc, prob['dbcvals'],
                        device=False)
    bo = host.bound_ops(res['modes'], res['mean'], hc, prob['dbcvals'])
    worst = {}
    for key in ('Mr', 'Ar', 'b0', 'c', 'L', 'H'):
        err = np.abs(ops[key] - hops[key])
        worst[key] = float((err/(2*bo[key])).max())
        assert np.all(err <= 2*bo[key]), (key, worst[key])
    assert ops['div'] == hops['div']
    assert np.all(np.abs(ops['Mr'] - np.eye(r))
                  <= pod_model.ortho_bound(res['gram'], res['sigma']))
    print(scheme, ': device against host model, worst error / (2 bound)',
          worst)
    # the projection identity for the columns of `coeffs`
    w = 0.
    for s in range(res['coeffs'].shape[1]):
        err, tol = _projection_identity(gr, hc, prob['dbcvals'],
                                        res['coeffs'][:, s], bo)
        w = max(w, float((err/tol).max()))
        assert np.all(err <= tol), s
    print(scheme, ': rhs(coeffs) against the full operators, worst error / '
          'tolerance', w)


def test_a_loop_cut_by_the_guard_reports_no_rom(gtiu, toy_prob):
    from dolfin_navier_scipy_amd import fem
    prob = toy_prob
    M, A = (sps.csr_matrix(prob['smc'][k]) for k in ('M', 'A'))
    kw, rec, _ = scenarios.build(variant='plain', seed=0, prob=prob)
    kw.pop('f_vdp')
    kw.update(check_ff_maxv=1e-3)
    cvop = _toy_cvop(prob)
    try:
        _, _, ff = gtiu.cnab(
            ntimeslices=3, device_convection=cvop, invinds=prob['invinds'],
            resident=dict(pod=fem.SnapshotPOD(M, every=EVERY),
                          rom=fem.GalerkinROM(A, prob['rhsd']['fv'])), **kw)
        assert ff == 1
        assert gtiu.LAST_RUN['rom'] is None and gtiu.LAST_RUN['pod'] is None
        assert 'rom_on' in gtiu.LAST_RUN
        # refused by name, nothing launched: no `pod`
        kw2, _, _ = scenarios.build(variant='plain', seed=0, prob=prob)
        kw2.pop('f_vdp')
        with pytest.raises(ValueError) as exc:
            gtiu.cnab(device_convection=cvop, invinds=prob['invinds'],
                      resident=dict(rom=fem.GalerkinROM(
                          A, prob['rhsd']['fv'])), **kw2)
        assert '`rom` without `pod`' in str(exc.value)
    finally:
        cvop.close()
