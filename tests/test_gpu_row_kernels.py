"""The row kernels of the lazy six-node step in isolation
(`saddle.row_kernel_probe`, `dns_row_kernel_probe`): synthetic operators whose
row lengths sit at the edges of the kernels' load chunks -- 0, 1, LPR - 1, LPR,
LPR + 1, NCH LPR - 1, NCH LPR, NCH LPR + 1 (the last one enters the loop that
continues a long row) -- with an empty row between two full ones and the
longest row last, so that it ends exactly at nnz.

Reference: the fp64 product of SciPy.  Bound, per row:

    |y - A x| <= (len + 2) 2^-53 (|A| |x|)

the bound of a recursive sum with fma; the 2 allows for the reduction tree
over the lanes.  Operators with fp32 values are generated in fp32 and converted
exactly.  Where a kernel's output is not the bare product, the test either
feeds it data for which it is (tau with b_p = kx_p; the step's right-hand side
with all its other terms switched off) or adds the one further rounding to
the bound and says so."""
import numpy as np
import pytest
import scipy.sparse as sps

pytestmark = pytest.mark.gpu

U = 2.0**-53


def edge_lengths(lpr, nch, nrows, rng):
    """row lengths: [full, empty, full], the eight edges, random filling, the
    longest row (nch*lpr + 1) last"""
    full = nch*lpr
    head = [full, 0, full, 0, 1, 1, lpr - 1, lpr, lpr + 1, full - 1, full,
            full + 1]
    nfill = nrows - len(head) - 1
    assert nfill >= 0
    fill = list(rng.integers(0, full + 2, size=nfill))
    return np.array(head + fill + [full + 1], dtype=np.int64)


def csr_with_lengths(lens, ncols, rng, fp32=False, split=None):
    """canonical CSR with the given row lengths and random columns; `split`:
    every row of two or more entries has columns on both sides of it"""
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.empty(indptr[-1], dtype=np.int32)
    for i, ln in enumerate(lens):
        if split is not None and ln >= 2:
            k1 = min((ln + 1)//2, split)
            cols = np.concatenate([
                rng.choice(split, size=k1, replace=False),
                split + rng.choice(ncols - split, size=ln - k1,
                                   replace=False)])
        elif split is not None and ln == 1:
            # (the two rows of length one: one on either side)
            cols = np.array([0 if i % 2 == 0 else ncols - 1])
        else:
            cols = rng.choice(ncols, size=ln, replace=False)
        indices[indptr[i]:indptr[i + 1]] = np.sort(cols)
    data = rng.standard_normal(indptr[-1])
    if fp32:
        data = data.astype(np.float32).astype(np.float64)
    A = sps.csr_matrix((data, indices, indptr), shape=(len(lens), ncols))
    assert A.has_canonical_format and A.indptr[-1] == A.nnz
    assert np.array_equal(np.diff(A.indptr), lens)
    return A


def assert_rows(name, y, A, x, extra=None):
    """the bound of the module docstring (`extra`: a further term per row)"""
    ref = A @ x
    lens = np.diff(A.indptr)
    bound = (lens + 2)*U*(abs(A) @ np.abs(x))
    if extra is not None:
        bound = bound + extra
    err = np.abs(y - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(bound > 0, err/bound, np.where(err > 0, np.inf, 0.))
    worst = int(np.argmax(ratio))
    print('%s: max err/bound %.3f at row %d (len %d)'
          % (name, ratio[worst], worst, lens[worst]))
    assert np.all(np.isfinite(y)), name
    assert np.all(err <= bound), (name, worst, err[worst], bound[worst])


@pytest.fixture(scope='module')
def probe():
    from dolfin_navier_scipy_amd import saddle
    return saddle.row_kernel_probe


@pytest.fixture(scope='module')
def ksys():
    """K (n x n), R1 (nv x nv) and a cell list (nv x ncell) for 32 lanes per
    row and two chunks, with the vectors that go with them; n = 3 k + 1, so
    the last pass of three rows per sub-wave is a partial one"""
    rng = np.random.default_rng(7)
    n, nv, ncell, lpr, nch = 151, 120, 400, 32, 2
    K = csr_with_lengths(edge_lengths(lpr, nch, n, rng), n, rng)
    lr = edge_lengths(lpr, nch, nv, rng)
    lc = edge_lengths(lpr, nch, nv, rng)
    # (both lists full, one of them empty, both empty: rows 0 .. 3)
    lr[:4] = [nch*lpr, 0, nch*lpr, 0]
    lc[:4] = [nch*lpr, nch*lpr, 0, 0]
    R1 = csr_with_lengths(lr, nv, rng)
    cells = csr_with_lengths(lc, ncell, rng)
    cells.data[:] = 1.
    vec = {k: rng.standard_normal(n) for k in ('x0', 'v_c', 'v_p', 'z', 'r')}
    vec['cellvals'] = rng.standard_normal(ncell)
    return dict(n=n, nv=nv, lpr=lpr, K=K, R1=R1, cells=cells, **vec)


@pytest.mark.parametrize('lpr,fp32', [(64, True), (64, False), (32, True)])
def test_gc_rows(probe, lpr, fp32):
    """k_spmv_gc_lazy: four chunks per lane, columns on both sides of nv"""
    rng = np.random.default_rng(11 + lpr + fp32)
    nv, ncols = 300, 2000
    lens = edge_lengths(lpr, 4, nv, rng)
    A = csr_with_lengths(lens, ncols, rng, fp32=fp32, split=nv)
    below = np.add.reduceat((A.indices < nv).astype(int),
                            A.indptr[:-1][lens > 0])
    assert np.all((below > 0) | (lens[lens > 0] < 2))
    x = rng.standard_normal(ncols)
    out = probe('gc', A, x[:nv], lpr=lpr, fp32_vals=fp32, x2=x[nv:])
    assert_rows('gc lpr=%d fp32=%d' % (lpr, fp32), out['y'], A, x)


def test_tau_rows(probe):
    """k_tau_first, Schur rows (128 lanes per row, four chunks): with
    b_p = kx_p the output is the bare product, -J (b - kx)_v; with a pressure
    part it is (b - kx)_p - s, ONE further rounding of a difference whose terms
    are bounded by |r_p| and (1 + (len + 2) u) |A| |x|"""
    rng = np.random.default_rng(3)
    np_, nv = 41, 1500
    A = csr_with_lengths(edge_lengths(128, 4, np_, rng), nv, rng)
    lens = np.diff(A.indptr)
    b, kx = rng.standard_normal(nv + np_), rng.standard_normal(nv + np_)
    xd = (b - kx)[:nv]
    b0 = b.copy()
    b0[nv:] = kx[nv:]
    out = probe('tau', A, b0, x2=kx)
    assert np.array_equal(out['r'], b0 - kx)
    assert_rows('tau, r_p = 0', -out['y'], A, xd)
    out = probe('tau', A, b, x2=kx)
    assert np.array_equal(out['r'], b - kx)
    rp = (b - kx)[nv:]
    ax = abs(A) @ np.abs(xd)
    extra = U*(np.abs(rp) + (1 + (lens + 2)*U)*ax)
    assert_rows('tau', rp - out['y'], A, xd, extra=extra)


@pytest.mark.parametrize('a_p', [0., .5])
def test_step_front_both_families(probe, ksys, a_p):
    """k_step_one2: kx = K x0 (K family); b_v = R1 (v_c + a_p v_p) and the
    gathered cell values (b family), every other term of b switched off.  With
    a_c = 1 and a_p a power of two, fma(a_p, v_p, a_c v_c) is the one rounding
    NumPy's v_c + a_p v_p has"""
    s = ksys
    out = probe('step', s['K'], s['x0'], lpr=s['lpr'], x2=s['v_c'],
                R1=s['R1'], cells=s['cells'], v_p=s['v_p'],
                cellvals=s['cellvals'], a_c=1., a_p=a_p)
    nv = s['nv']
    assert_rows('step kx', out['kx'], s['K'], s['x0'])
    v = (s['v_c'] + a_p*s['v_p'])[:nv]
    assert_rows('step b_v (a_p=%g)' % a_p, out['b'][:nv], s['R1'], v)
    assert np.all(out['b'][nv:] == 0.)
    assert_rows('step cells', out['nfc'], s['cells'], s['cellvals'])


def test_spmv_rw_rows_and_partial_sums(probe, ksys):
    """k_spmv_rw: w = K z, three rows per sub-wave and pass, and the partials
    of <r, w> and <w, w> (recursive sums of n products: (n + 2) u sum |.|)"""
    s = ksys
    out = probe('rw', s['K'], s['z'], lpr=s['lpr'], x2=s['r'])
    w, n = out['y'], s['n']
    assert_rows('rw w', w, s['K'], s['z'])
    assert out['wr'].size == out['ww'].size == -(-n//(3*(512//s['lpr'])))
    for name, parts, a in (('<r,w>', out['wr'], s['r']), ('<w,w>', out['ww'], w)):
        ref, bound = np.dot(a, w), (n + 2)*U*np.dot(np.abs(a), np.abs(w))
        err = abs(parts.sum() - ref)
        print('rw %s: err/bound %.3f' % (name, err/bound))
        assert err <= bound, (name, err, bound)


def test_spmv_rw_other_widths(probe):
    """the same kernel with 16 and 64 lanes per row"""
    for lpr in (16, 64):
        rng = np.random.default_rng(lpr)
        n = 160 if lpr == 16 else 130
        K = csr_with_lengths(edge_lengths(lpr, 2, n, rng), n, rng)
        z, r = rng.standard_normal(n), rng.standard_normal(n)
        out = probe('rw', K, z, lpr=lpr, x2=r)
        assert_rows('rw lpr=%d' % lpr, out['y'], K, z)


@pytest.fixture(scope='module')
def dense():
    rng = np.random.default_rng(5)
    S = rng.standard_normal((1289, 1289)).astype(np.float32).astype(np.float64)
    return S, rng.standard_normal(1289)


@pytest.mark.parametrize('npr', [1, 255, 256, 257, 1289])
def test_dense_head_rows(probe, dense, npr):
    """k_arn_head_lazy, padded fp32 rows: zp = -S tau"""
    S, tau = dense[0][:npr, :npr], dense[1][:npr]
    out = probe('head', x=tau, x2=S)
    ref = S @ tau
    bound = (npr + 2)*U*(np.abs(S) @ np.abs(tau))
    err = np.abs(-out['y'] - ref)
    print('head np=%d: max err/bound %.3f' % (npr, (err/bound).max()))
    assert np.all(err <= bound), (npr, err.max())
