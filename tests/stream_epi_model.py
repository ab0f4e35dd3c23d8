"""Reference model of the epilogues of `k_spmv_stream16x` (kernels.hpp) and
`k_spmv_pair16x` (pair.hpp): the same operations in `np.longdouble` (64-bit
mantissa), the modulus sums their rounding-error bounds are made of, the bounds
themselves, and the matrices of the case list.

Row results (`reference`), with `s = A x` of one row and `L` its stored length:

    plain     y = alpha s + beta b           m = |alpha| |A||x| + |beta b|
    sweep     y = alpha (xin + omega dinv (b - s))
                                             m = |alpha| (|xin| + |omega dinv|
                                                          (|b| + |A||x|))
    add_cb    y = alpha s + omega dinv b     m = |alpha| |A||x| + |omega dinv b|

    |y_dev - y_ref| <= gamma(2 L + 8) m,     gamma(k) = k u / (1 - k u), u = 2^-53

(a sum of L products in any order is within gamma(L) of its modulus sum; the
factor 2 pays for the two roundings of a 2x2 block product in the pair format,
the 8 for the few operations of the epilogue).

Dots (`dot_references`) are formed from the DEVICE's `y`, which keeps their
error apart from the product's: over the `rows` of the launch

    |sum of partials - sum V_i[r] y_dev[r]| <= gamma(rows + 8) sum |V_i[r] y_dev[r]|

and the same for `<y, y>` and `<b, b>`; the caller sums the partials in
extended precision (`ldsum`).

With `fp32_vals` the model takes the values rounded to float and widened
again: exactly what the device holds.
"""
import numpy as np
import scipy.sparse as sps

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, 'the model needs an extended long double'
U = 2.0**-53

TILE, ROWCAP = 2048, 256          # row blocks of the streaming kernel


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k*U/(1. - k*U)


def ldsum(a):
    """sum in extended precision (error 2^-11 of a double's unit per term)"""
    return np.sum(np.asarray(a, dtype=LD), dtype=LD)


def device_values(A, fp32_vals=False):
    data = np.asarray(A.data, dtype=np.float64)
    if fp32_vals:
        data = data.astype(np.float32).astype(np.float64)
    return data


def row_sums(indptr, terms):
    """per-row sums of `terms` (one per stored entry), empty rows give 0"""
    out = np.zeros(indptr.size - 1, dtype=terms.dtype)
    rows = np.flatnonzero(np.diff(indptr) > 0)
    if rows.size:
        out[rows] = np.add.reduceat(terms, indptr[rows])
    return out


def product(A, x, fp32_vals=False):
    """(A x, |A||x|, stored row lengths), the first two in long double"""
    A = sps.csr_matrix(A)
    data = device_values(A, fp32_vals).astype(LD)
    terms = data*np.asarray(x, dtype=np.float64).astype(LD)[A.indices]
    return (row_sums(A.indptr, terms), row_sums(A.indptr, np.abs(terms)),
            np.diff(A.indptr))


def epilogue(s, sabs, mode, alpha, beta, b, dinv, xin, omega, dtype=LD):
    """(y, m) of one mode from the row products `s` and their modulus sums
    `sabs`, evaluated in `dtype`; b, dinv, xin: the rows' entries or None"""
    c = lambda v: None if v is None else np.asarray(v, np.float64).astype(dtype)
    s, b, dinv, xin = s.astype(dtype), c(b), c(dinv), c(xin)
    alpha, beta, omega = dtype(alpha), dtype(beta), dtype(omega)
    sabs = sabs.astype(LD)
    aa = abs(LD(alpha))
    L = lambda v: np.abs(v.astype(LD))
    if mode == 'plain':
        if b is None:
            return alpha*s, aa*sabs
        return alpha*s + beta*b, aa*sabs + L(beta*b)
    if mode == 'sweep':
        xi = np.zeros_like(s) if xin is None else xin
        return (alpha*(xi + omega*dinv*(b - s)),
                aa*(L(xi) + L(omega*dinv)*(L(b) + sabs)))
    assert mode == 'add_cb'
    return alpha*s + omega*dinv*b, aa*sabs + L(omega*dinv*b)


def reference(A, x, mode='plain', alpha=1., beta=0., b=None, dinv=None,
              xin=None, omega=1., fp32_vals=False, rows=None):
    """(y_ref, tol) per row of `A`, y_ref in long double, tol = gamma(2L+8) m.
    `x`: every column ([x ; x2] of a split input); b, dinv, xin are indexed by
    global row, `rows` are the global rows of A's rows (None: 0 .. nrows-1)"""
    s, sabs, L = product(A, x, fp32_vals)
    pick = lambda v: None if v is None else \
        np.asarray(v, np.float64)[slice(None) if rows is None else rows]
    y, m = epilogue(s, sabs, mode, alpha, beta, pick(b), pick(dinv), pick(xin),
                    omega)
    return y, (gamma(2*L + 8).astype(LD)*m).astype(np.float64)


def dot_references(y_dev, V, nvec, b=None, rows=None):
    """references and tolerances of the fused dots over `rows` from the
    device's y: dict(vy, vy_tol (nvec each), ww, ww_tol, bb, bb_tol)"""
    sel = slice(0, len(y_dev)) if rows is None else rows
    y = np.asarray(y_dev, np.float64)[sel].astype(LD)
    g = LD(gamma(y.size + 8))
    out = dict(vy=np.zeros(nvec, LD), vy_tol=np.zeros(nvec))
    for i in range(nvec):
        t = np.asarray(V[i], np.float64)[sel].astype(LD)*y
        out['vy'][i] = ldsum(t)
        out['vy_tol'][i] = float(g*ldsum(np.abs(t)))
    out['ww'] = ldsum(y*y)
    out['ww_tol'] = float(g*out['ww'])
    if b is not None:
        bb = np.asarray(b, np.float64)[sel].astype(LD)
        out['bb'] = ldsum(bb*bb)
        out['bb_tol'] = float(g*out['bb'])
    return out


# ---- the streaming kernel's row blocks (CsrDev::upload), restated ----------
def stream_rowblocks(A):
    """[(r0, r1)]: consecutive rows with at most TILE entries and at most
    ROWCAP rows; a longer row stands alone"""
    lens = np.diff(A.indptr)
    blocks, start, n = [], 0, lens.size
    while start < n:
        end, acc = start, 0
        while end < n and end - start < ROWCAP and acc + lens[end] <= TILE:
            acc += lens[end]
            end += 1
        if end == start:
            end = start + 1
        blocks.append((start, end))
        start = end
    return blocks


def stream_block_kinds(A):
    """per row block: 'empty', 'single' (one row longer than the tile), 'one'
    / 'two' (16-bit windows in use) or 'raw' (32-bit indices)"""
    kinds = []
    for r0, r1 in stream_rowblocks(A):
        cols = A.indices[A.indptr[r0]:A.indptr[r1]]
        if cols.size == 0:
            kinds.append('empty')
        elif cols.size > TILE:
            kinds.append('single')
        else:
            lo, mx = int(cols.min()), int(cols.max())
            far = cols[cols - lo > 32767]
            if far.size == 0:
                kinds.append('one')
            elif mx - int(far.min()) > 32767:
                kinds.append('raw')
            else:
                kinds.append('two')
    return kinds


def stream_g_class(A):
    """the G instantiation `launch_stream16x` picks"""
    avg = A.nnz/float(A.shape[0])
    return 1 if avg <= 6 else 2 if avg <= 12 else 4 if avg <= 192 else 16


# ---- matrices of the case list ----------------------------------------------
def _ragged(rng, nrows, ncols, mean, colfun=None):
    """rows of uneven length (0 .. 2 mean, a tenth of them empty)"""
    lens = rng.integers(1, 2*mean, nrows)
    lens[rng.random(nrows) < 0.1] = 0
    rows = np.repeat(np.arange(nrows), lens)
    cols = rng.integers(0, ncols, rows.size) if colfun is None \
        else colfun(rows)
    A = sps.csr_matrix((rng.uniform(-1, 1, rows.size), (rows, cols)),
                       shape=(nrows, ncols))
    A.sum_duplicates()
    A.sort_indices()
    return A


def stream_matrix(name):
    """the matrices of the streaming kernel's cases, by name (seeded)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == 'g1':
        return _ragged(rng, 4000, 4000, 4)
    if name == 'g2':
        return _ragged(rng, 3000, 3000, 9)
    if name == 'g4':
        return _ragged(rng, 1200, 1500, 60)
    if name == 'g16':
        return _ragged(rng, 300, 3000, 400)
    if name == 'longrow':        # one row beyond the tile stands alone
        A = _ragged(rng, 40, 6000, 30).tolil()
        cols = np.sort(rng.choice(6000, 3001, replace=False))
        A[17, cols] = rng.uniform(-1, 1, cols.size)
        A = A.tocsr()
        A.sort_indices()
        return A
    if name == 'rowcap':         # blocks closed by the 256-row cap
        return _ragged(rng, 700, 700, 2)
    if name == 'window2':        # far columns behind the second base
        def cols(rows):
            near = (10*rows + rng.integers(0, 3000, rows.size)) % 30000
            far = 100000 + (rows + rng.integers(0, 9000, rows.size)) % 20000
            return np.where(rng.random(rows.size) < 0.7, near, far)
        return _ragged(rng, 600, 120000, 8, cols)
    if name == 'raw':            # columns over more than two windows
        return _ragged(rng, 500, 120000, 20)
    raise KeyError(name)


STREAM_G = ('g1', 'g2', 'g4', 'g16')
STREAM_SPECIAL = ('longrow', 'rowcap', 'window2', 'raw')
PAIR_CASES = ((3000, 400, True), (3000, 400, False), (700, 0, True),
              (5, 3, False))


def pair_matrix(nodes, npres, coupled):
    """(K, nv) of the pair kernel's cases: `_pair_k` of test_gpu_kernels with
    that test's seeds and densities"""
    from test_gpu_kernels import _pair_k
    rng = np.random.default_rng(nodes + npres)
    return _pair_k(rng, nodes, npres, dens=min(0.5, 12./nodes), coupled=coupled)


def check_stream_matrix(name, A):
    """the properties the case list asks of a matrix"""
    blocks, kinds = stream_rowblocks(A), stream_block_kinds(A)
    lens = np.diff(A.indptr)
    if name in STREAM_G:
        assert stream_g_class(A) == int(name[1:])
        assert len(blocks) >= 12
        assert len(set(r1 - r0 for r0, r1 in blocks)) > 1
        assert (lens == 0).any()
        assert any(A.indptr[r0] & 1 for r0, _ in blocks)
    elif name == 'longrow':
        assert kinds.count('single') == 1 and lens.max() > TILE
    elif name == 'rowcap':
        assert any(r1 - r0 == ROWCAP for r0, r1 in blocks)
    elif name == 'window2':
        assert 'two' in kinds and 'raw' not in kinds
    elif name == 'raw':
        assert 'raw' in kinds
