"""A NumPy `longdouble` model of the FRONT of a resident IMEX step -- what
every form of the step hands the Krylov solver (`dns_imex::front_fused`,
`front_six`, `front_rows`, `front_stream`, and the tails that leave the next
warm start) -- written from the closed formulas, not from the kernels:

    x0  = sum_i e_i x_{-i}                      (warm start)
    b_v = R1 (a_c v_c + a_p v_p) + cn_c nfc_c + cn_o nfc_o + g [+ carry]
    b_p = gp
    kx  = K x0,   r0 = b - K x0,   sum r0^2,   sum b^2
    carry (MODE 2) = a_c r_c + a_p r_old,  r_c = (b_prev - K x_c)_v,
                     kx = e_c K x_c + sum_{i>0} e_i (K x_{-i} as kept)
    carry (Six)    = a_c rc6[current] + a_p rc6[previous]

The data are the fp64 values `dns_imex_front_probe` copies out before the
front runs and the matrices K, R1.  Every quantity comes with its MODULI: the
same sum with every term replaced by its absolute value.  Tolerances:

    entry-wise      16 u x moduli of the entry,      u = 2^-53
    sums of squares 16 u x the sum
    moduli 0        the values are equal

The coefficients e_i are DERIVED here (`extrap_table`): the interpolating sets
are the Lagrange weights at t = 1 through t = 0, -1, ...; order 13 is the value
at t = 1 of the cubic least-squares fit through five points; while the
history is filling the lower order is taken (and order 13 means 3).  In exact
rationals this gives (2,-1), (3,-3,1), (4,-6,4,-1), (5,-10,10,-5,1) and
(16/5, -14/5, -4/5, 11/5, -4/5).

Exceptions of single forms, pinned as they are (not reconciled):
  * a negative order is x0 = x_c on the fused path, the LINEAR start where the
    warm start is a kernel of its own (Plain, StreamRhs): `order_for`
  * order 13 where the warm start is a kernel of its own is the interpolating
    cubic even with a full ring; `prime_six` launches the QUARTIC.

Measured on the CPU (tests/test_imex_front_model_cpu.py prints them with
`pytest -s`): largest |fp64 evaluation - long double| / tolerance over
row-serial sums and sub-wave trees of 2 .. 64 lanes, each with and without
fused multiply-add, toy system, rough data, nsol 1 .. 5, order 4 and 13, CNAB
and SBDF2 (sums of squares: the raw partials of 32 rows each, added in long
double, against the long double sum over the same fp64 vector):
    x0 0.154  b 0.073  kx 0.218  r0 0.185  sum r0^2 0.018  sum b^2 0.022
    MODE 2: b 0.115  kx (linearity) 0.195  r0 0.158  K x_c 0.191  rcarry 0.122
            sum r0^2 0.022  sum b^2 0.028
    Six carry: b 0.108  kx 0.196  r0 0.175  sum r0^2 0.026  sum b^2 0.015
  (all <= 0.25)
c6, the allowance of the six-node step's residual by linearity
(r0 - sum y_j W_j against b - K x_new, units u (|b_prev| + |K| (|x0_prev| +
|x_c|))): largest ratio 0.953 with one and two columns -> 4 x, rounded up to a
power of two, at least 16:                                        c6 = 16
Mutations, smallest over the cases (order 4 and 13, CNAB and SBDF2) of the
largest |mutant - model| / tolerance (all >= 100):
    ring slots swapped (0,1) 1.1e15 (1,2) 7.8e14 (2,3) 1.2e15 (3,4) 1.1e15
    coefficient set of nsol - 1 3.9e14   cn_c <-> cn_o 8.0e14
    a_p at nsol = 1 3.4e13   g of the neighbouring row 5.6e16
    carry dropped 4.8e4 (a previous solve converged to 1e-10)
    x0 of the step before 1.7e15

By rows (`footprint`, `front_model_rows`: the row-partitioned forms DistFront,
Rows, StreamRows; tests/test_gpu_zz_dist_front.py): the same formulas on a
rank's own rows of the row-sliced K / R1, from the ring as that rank holds it,
every entry outside the rank's footprint (own rows, columns of its rows of K
and R1, dofs of the convection cells that touch an own row) set to NaN first.
On the CPU, 2 and 3 ranks, CNAB and SBDF2, in the order of `k_dist_front`
(32 lanes, fused): x0 0.154  b 0.073  kx 0.164  r 0.127, with the carried
residuals b 0.145  r 0.163 (all <= 0.25).  Mutations, smallest miss /
tolerance: row2 off by one 5.8e15, len1 one short 8.5e12, one halo entry of
the previous ring slot x0 4.1e14 (r 1.3e11 where K's own rows hold a non-zero
there), rcc <-> rcp 1.3e5, carry dropped 9.3e4, a_p at nsol = 1 9.1e12, a cell
never evaluated nfc_c 1.9e12 (b 9.2e9).

Measured on an MI355X (tests/test_gpu_imex_front.py prints them with
`pytest -s`), largest error / tolerance over all of its cases:
    x0 0.136  b 0.252  kx (Six) 0.032  r0 0.139  sum partR 0.016
    sum partB 0.024  K x_c 0.149  rcarry 0.085  nfc_c 0.055
    six-node carried residual 0.075 (of c6 u ...)
"""
from fractions import Fraction

import numpy as np
import scipy.sparse as sps

LD = np.longdouble
U = LD(2.0)**-53
TOL = 16*U
FIT35 = 13


# ---- the coefficient table ---------------------------------------------------

def lagrange_at_one(m):
    """weights at t = 1 of the interpolant through t = 0, -1, .., -(m - 1)"""
    t = [Fraction(-i) for i in range(m)]
    w = []
    for i in range(m):
        num = den = Fraction(1)
        for j in range(m):
            if j != i:
                num *= 1 - t[j]
                den *= t[i] - t[j]
        w.append(num/den)
    return w


def lsq_at_one(m, deg):
    """weights at t = 1 of the least-squares polynomial of degree `deg`
    through t = 0, -1, .., -(m - 1): p(1)^T (V^T V)^-1 V^T, in rationals"""
    t = [Fraction(-i) for i in range(m)]
    V = [[ti**k for k in range(deg + 1)] for ti in t]
    nq = deg + 1
    # solve (V^T V) c = p(1) (symmetric: the weights are V c)
    A = [[sum(V[r][i]*V[r][j] for r in range(m)) for j in range(nq)]
         + [Fraction(1)] for i in range(nq)]
    for i in range(nq):
        piv = next(r for r in range(i, nq) if A[r][i] != 0)
        A[i], A[piv] = A[piv], A[i]
        A[i] = [a/A[i][i] for a in A[i]]
        for r in range(nq):
            if r != i and A[r][i] != 0:
                A[r] = [a - A[r][i]*b for a, b in zip(A[r], A[i])]
    c = [A[i][nq] for i in range(nq)]
    return [sum(V[r][k]*c[k] for k in range(nq)) for r in range(m)]


def extrap_table(nsol, order):
    """the five coefficients (fp64) of the warm start from `nsol` solutions;
    history still filling: the lower order"""
    nsol = min(int(nsol), 5)
    if order == FIT35 and nsol >= 5:
        w = lsq_at_one(5, 3)
    else:
        if order == FIT35:
            order = 3
        m = max(1, min(nsol, order + 1, 5))
        w = lagrange_at_one(m)
    return np.array([float(x) for x in w] + [0.]*(5 - len(w)))


def order_for(order, form, primed_six=False):
    """the order a FORM makes of `extrapolate_x0` (today's behaviour, pinned):
    fused fronts and every tail take it as it is (negative: x0 = x_c); the
    warm-start kernel of Plain / StreamRhs takes the cubic for 13 and the
    linear start for a negative one; `prime_six` the quartic for 13"""
    if primed_six:
        return 4 if order == FIT35 else order
    if form in ('Plain', 'StreamRhs'):
        return 3 if order == FIT35 else 1 if order < 0 else order
    return order


# ---- long double sums --------------------------------------------------------

def _ld(x):
    return np.asarray(x, dtype=np.float64).astype(LD)


def spmv(A, x, absval=False):
    """rows of `A x` in long double (`absval`: |A| |x|)"""
    A = sps.csr_matrix(A)
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    d, xx = _ld(A.data), np.asarray(x, dtype=LD)
    if absval:
        d, xx = np.abs(d), np.abs(xx)
    out = np.zeros(A.shape[0], dtype=LD)
    np.add.at(out, rows, d*xx[A.indices])
    return out


def front_model(K, R1, ring, e, a_c, a_p, cn_c, cn_o, nfc, g, gp, carry=None):
    """dict of `(value, moduli)` pairs: `x0`, `b`, `kx`, `r`.  `ring (5, n)` in ring order (slots the coefficients
    `e (5,)` / `a_p` do not touch are not read), `nfc (2, nv)` = nfc_c, nfc_o.
    `carry`: None, or
      dict(kind='mode2', b_prev (n), kxs (4, n), r_old (nv)) -- adds `kxc` =
        K x_c, `rcarry` = (b_prev - K x_c)_v; kx is formed by linearity
      dict(kind='six', rc (2, nv)) -- rc6[current], rc6[previous]"""
    n, nv = K.shape[0], R1.shape[0]
    ring = _ld(ring)
    e = [LD(float(x)) for x in e]
    a_c, a_p, cn_c, cn_o = (LD(float(x)) for x in (a_c, a_p, cn_c, cn_o))
    x0 = np.zeros(n, dtype=LD)
    x0a = np.zeros(n, dtype=LD)
    for i in range(5):
        if e[i] != 0:
            x0 = x0 + e[i]*ring[i]
            x0a = x0a + abs(e[i])*np.abs(ring[i])
    w = a_c*ring[0, :nv]
    wa = abs(a_c)*np.abs(ring[0, :nv])
    if a_p != 0:
        w = w + a_p*ring[1, :nv]
        wa = wa + abs(a_p)*np.abs(ring[1, :nv])
    nfc, g, gp = _ld(nfc), _ld(g), _ld(gp)
    bv = spmv(R1, w) + cn_c*nfc[0] + cn_o*nfc[1] + g
    bva = (spmv(np.abs(R1), wa) + abs(cn_c)*np.abs(nfc[0])
           + abs(cn_o)*np.abs(nfc[1]) + np.abs(g))
    out = {}
    kx, kxa = spmv(K, x0), spmv(np.abs(K), x0a)
    if carry is not None and carry['kind'] == 'mode2':
        bp, kxs, ro = _ld(carry['b_prev']), _ld(carry['kxs']), \
            _ld(carry['r_old'])
        kxc, kxca = spmv(K, ring[0]), spmv(K, ring[0], absval=True)
        rc, rca = (bp - kxc)[:nv], (np.abs(bp) + kxca)[:nv]
        out['kxc'], out['rcarry'] = (kxc, kxca), (rc, rca)
        bv = bv + a_c*rc + a_p*ro
        bva = bva + abs(a_c)*rca + abs(a_p)*np.abs(ro)
        kx, kxa = e[0]*kxc, abs(e[0])*kxca
        for i in range(1, 5):
            if e[i] != 0:
                kx = kx + e[i]*kxs[i - 1]
                kxa = kxa + abs(e[i])*np.abs(kxs[i - 1])
    elif carry is not None and carry['kind'] == 'six':
        rc = _ld(carry['rc'])
        bv = bv + a_c*rc[0] + a_p*rc[1]
        bva = bva + abs(a_c)*np.abs(rc[0]) + abs(a_p)*np.abs(rc[1])
    b, ba = np.concatenate([bv, gp]), np.concatenate([bva, np.abs(gp)])
    out.update(x0=(x0, x0a), b=(b, ba), kx=(kx, kxa), r=(b - kx, ba + kxa))
    return out


# ---- the front by rows (row-partitioned forms) -------------------------------

def own_rows(st_v, st_p, rank, nv):
    """this rank's global rows of K: its velocity rows, then its pressure
    rows (`RowMap {st_v[r], len1, nv + st_p[r], len2}`)"""
    return np.r_[np.arange(st_v[rank], st_v[rank + 1]),
                 nv + np.arange(st_p[rank], st_p[rank + 1])]


def selected_cells(conv_space, st_v, rank):
    """the cells with a test function on one of the rank's velocity rows
    (`conv_space.code (nc, 12)`: inner row of the slot, negative: Dirichlet)"""
    code = conv_space.code
    return np.flatnonzero(((code >= st_v[rank])
                           & (code < st_v[rank + 1])).any(axis=1))


def footprint(K, R1, st_v, st_p, rank, conv_space=None):
    """the sorted global entries of a solution vector rank `rank` may read:
    its own velocity and pressure rows, the columns of those rows of K, the
    columns of its own rows of R1 and, with a convection, every dof of every
    cell that has a test function on an own row"""
    K, R1 = sps.csr_matrix(K), sps.csr_matrix(R1)
    nv = R1.shape[0]
    own = own_rows(st_v, st_p, rank, nv)
    mark = np.zeros(K.shape[0], dtype=bool)
    mark[own] = True
    mark[K[own].indices] = True
    mark[R1[st_v[rank]:st_v[rank + 1]].indices] = True
    if conv_space is not None:
        d = conv_space.code[selected_cells(conv_space, st_v, rank)]
        mark[d[d >= 0]] = True
    return np.flatnonzero(mark)


def _only(x, keep):
    """`x` in long double, NaN wherever the last index is not in `keep`"""
    x = _ld(x)
    y = np.full(x.shape, np.nan, dtype=LD)
    y[..., keep] = x[..., keep]
    return y


def front_model_rows(K, R1, st_v, st_p, rank, ring, e, a_c, a_p, cn_c, cn_o,
                     nfc, g, gp, carry=None, conv_space=None):
    """`front_model` on the own rows of the row-sliced K / R1, from the ring
    AS THAT RANK DOWNLOADED IT: every entry outside the footprint (and of
    `nfc`, `g`, `gp`, `carry['rc']` outside the own rows) is overwritten with
    NaN before use, so nothing else is read.  Returns `(value, moduli)` for
    `x0` on the footprint, `b`, `kx`, `r` on the own rows (velocity rows, then
    pressure rows) and, with `carry = dict(rc=(2, nv))` (the carried residuals
    of the current and the previous solve), the term `a_c rcc + a_p rcp` on the
    own velocity rows as `carry`; `own`, `fp`: the index sets"""
    K, R1 = sps.csr_matrix(K), sps.csr_matrix(R1)
    n, nv = K.shape[0], R1.shape[0]
    ov = np.arange(st_v[rank], st_v[rank + 1])
    op = np.arange(st_p[rank], st_p[rank + 1])
    own = own_rows(st_v, st_p, rank, nv)
    fp = footprint(K, R1, st_v, st_p, rank, conv_space)
    ring = _only(ring, fp)
    nfc, g, gp = _only(nfc, ov), _only(g, ov), _only(gp, op)
    Kr, Rr = K[own], R1[ov]
    e = [LD(float(x)) for x in e]
    a_c, a_p, cn_c, cn_o = (LD(float(x)) for x in (a_c, a_p, cn_c, cn_o))
    x0 = np.zeros(n, dtype=LD)
    x0a = np.zeros(n, dtype=LD)
    for i in range(5):
        if e[i] != 0:
            x0 = x0 + e[i]*ring[i]
            x0a = x0a + abs(e[i])*np.abs(ring[i])
    w = a_c*ring[0, :nv]
    wa = abs(a_c)*np.abs(ring[0, :nv])
    if a_p != 0:
        w = w + a_p*ring[1, :nv]
        wa = wa + abs(a_p)*np.abs(ring[1, :nv])
    bv = spmv(Rr, w) + cn_c*nfc[0, ov] + cn_o*nfc[1, ov] + g[ov]
    bva = (spmv(np.abs(Rr), wa) + abs(cn_c)*np.abs(nfc[0, ov])
           + abs(cn_o)*np.abs(nfc[1, ov]) + np.abs(g[ov]))
    out = dict(own=own, fp=fp)
    if carry is not None:
        rc = _only(carry['rc'], ov)
        t, ta = a_c*rc[0, ov], abs(a_c)*np.abs(rc[0, ov])
        if a_p != 0:
            t, ta = t + a_p*rc[1, ov], ta + abs(a_p)*np.abs(rc[1, ov])
        out['carry'] = (t, ta)
        bv, bva = bv + t, bva + ta
    b, ba = np.concatenate([bv, gp[op]]), np.concatenate([bva, np.abs(gp[op])])
    kx, kxa = spmv(Kr, x0), spmv(np.abs(Kr), x0a)
    out.update(x0=(x0[fp], x0a[fp]), b=(b, ba), kx=(kx, kxa),
               r=(b - kx, ba + kxa))
    return out


def dist_front_eval64(K, R1, st_v, st_p, rank, ring, e, a_c, a_p, cn_c, cn_o,
                      nfc, g, gp, carry=None, lanes=32, fused=True):
    """`x0` (all entries), `b`, `kx`, `r` (own rows) in fp64 in the order of
    `k_dist_front`: the row sums over sub-waves of `lanes`, `s + cn_c nc +
    cn_o nfc_o + g`, the two `fma` of the carry, `bv - sk`"""
    f8 = lambda x: np.asarray(x, dtype=np.float64)
    K, R1 = sps.csr_matrix(K), sps.csr_matrix(R1)
    n, nv = K.shape[0], R1.shape[0]
    ov = np.arange(st_v[rank], st_v[rank + 1])
    op = np.arange(st_p[rank], st_p[rank + 1])
    own = own_rows(st_v, st_p, rank, nv)
    ring, nfc, g, gp = f8(ring), f8(nfc), f8(g), f8(gp)
    x0 = e[0]*ring[0]
    for i in range(1, 5):
        if e[i] != 0:
            x0 = _fma(np.full(n, float(e[i])), ring[i], x0, fused)
    if a_p != 0:
        w = _fma(np.full(nv, float(a_c)), ring[0, :nv], a_p*ring[1, :nv], fused)
    else:
        w = a_c*ring[0, :nv]
    sk = spmv64(K[own], x0, lanes, fused)
    bv = spmv64(R1[ov], w, lanes, fused) + cn_c*nfc[0, ov] + cn_o*nfc[1, ov] \
        + g[ov]
    if carry is not None:
        rc = f8(carry['rc'])
        bv = _fma(np.full(ov.size, float(a_c)), rc[0, ov], bv, fused)
        if a_p != 0:
            bv = _fma(np.full(ov.size, float(a_p)), rc[1, ov], bv, fused)
    b = np.concatenate([bv, gp[op]])
    return dict(x0=x0, b=b, kx=sk, r=b - sk)


def sumsq(v):
    """`(sum v_i^2, the same)` of an fp64 vector in long double: what the raw
    partials of a norm add up to, with its moduli"""
    s = np.sum(_ld(v)**2)
    return s, s


def six_residual_bound(K, b_prev, x0_prev, x_c):
    """the unit of c6 per entry: u (|b_prev| + |K| (|x0_prev| + |x_c|))"""
    return U*(np.abs(_ld(b_prev)) + spmv(K, np.abs(_ld(x0_prev))
                                         + np.abs(_ld(x_c)), absval=True))


C6 = 16


def ratio(got, value, moduli, tol=TOL):
    """largest |got - value| / (tol moduli); entries with moduli 0 must be
    equal"""
    err = np.abs(np.asarray(got).reshape(-1).astype(LD)
                 - np.asarray(value, dtype=LD).reshape(-1))
    bound = tol*np.asarray(moduli, dtype=LD).reshape(-1)
    z = bound == 0
    if np.any(err[z] != 0) or not np.all(np.isfinite(err)):
        return np.inf
    if np.all(z):
        return 0.0
    return float(np.max(err[~z]/bound[~z]))


# ---- fp64 evaluations in the orders a kernel may choose ----------------------

def _fma(a, b, c, fused):
    if fused:       # (one rounding, up to the 64-bit significand in between)
        return (a.astype(LD)*b.astype(LD) + c.astype(LD)).astype(np.float64)
    return a*b + c


def spmv64(A, x, lanes=1, fused=True):
    """fp64 rows of `A x`: lane l of `lanes` takes the entries l, l + lanes,
    .. of a row one after the other, then a tree over the lanes"""
    A = sps.csr_matrix(A)
    lens = np.diff(A.indptr)
    nch = int(-(-max(1, lens.max())//lanes))
    val = np.zeros((A.shape[0], nch*lanes))
    xv = np.zeros_like(val)
    rows = np.repeat(np.arange(A.shape[0]), lens)
    pos = np.arange(A.nnz) - A.indptr[rows]
    val[rows, pos] = A.data
    xv[rows, pos] = np.asarray(x, dtype=np.float64)[A.indices]
    acc = val[:, :lanes]*xv[:, :lanes]
    for j in range(1, nch):
        sl = slice(j*lanes, (j + 1)*lanes)
        acc = _fma(val[:, sl], xv[:, sl], acc, fused)
    w = lanes
    while w > 1:
        w //= 2
        acc = acc[:, :w] + acc[:, w:2*w]
    return acc[:, 0]


def front_eval64(K, R1, ring, e, a_c, a_p, cn_c, cn_o, nfc, g, gp, carry=None,
                 lanes=1, fused=True):
    """the quantities of `front_model` in fp64, the sums in one of the orders;
    `rr`, `bb`: the raw partials of the sums of squares"""
    f8 = lambda x: np.asarray(x, dtype=np.float64)
    n, nv = K.shape[0], R1.shape[0]
    ring, nfc, g, gp = f8(ring), f8(nfc), f8(g), f8(gp)
    one = lambda s: np.full(n, float(s))
    x0 = e[0]*ring[0]
    for i in range(1, 5):
        if e[i] != 0:
            x0 = _fma(one(e[i]), ring[i], x0, fused)
    w = a_c*ring[0, :nv]
    if a_p != 0:
        w = _fma(np.full(nv, float(a_p)), ring[1, :nv], w, fused)
    bv = spmv64(R1, w, lanes, fused) + cn_c*nfc[0] + cn_o*nfc[1] + g
    out = {}
    kx = spmv64(K, x0, lanes, fused)
    if carry is not None and carry['kind'] == 'mode2':
        kxc = spmv64(K, ring[0], lanes, fused)
        rc = (f8(carry['b_prev']) - kxc)[:nv]
        out['kxc'], out['rcarry'] = kxc, rc
        bv = bv + _fma(np.full(nv, float(a_c)), rc, a_p*f8(carry['r_old']),
                       fused)
        kx = e[0]*kxc
        for i in range(1, 5):
            kx = _fma(one(e[i]), f8(carry['kxs'])[i - 1], kx, fused)
    elif carry is not None and carry['kind'] == 'six':
        rc = f8(carry['rc'])
        bv = bv + _fma(np.full(nv, float(a_p)), rc[1], a_c*rc[0], fused)
    b = np.concatenate([bv, gp])
    r = b - kx
    out.update(x0=x0, b=b, kx=kx, r=r)

    def sumsq(v):
        # one partial per 32 rows (a workgroup of k_step_back), its squares
        # added lane after lane or by a tree; the partials are the result
        m = -(-v.size//32)*32
        p = np.zeros(m)
        p[:v.size] = v
        p = p.reshape(-1, 32 // min(lanes, 32), min(lanes, 32))
        acc = np.zeros((p.shape[0], p.shape[2]))
        for j in range(p.shape[1]):
            acc = _fma(p[:, j], p[:, j], acc, fused)
        w_ = acc.shape[1]
        while w_ > 1:
            w_ //= 2
            acc = acc[:, :w_] + acc[:, w_:2*w_]
        return acc[:, 0]
    out['rr'], out['bb'] = sumsq(r), sumsq(b)
    return out


def six_route64(K, b, x0, zs, ys):
    """the six-node step's residual by linearity in fp64: `fl(b - K x0)`,
    `x_new = fl(x0 + sum y_j z_j)`, `W_j = fl(K z_j)`, `fl(r0 - sum y_j W_j)`;
    returns `(x_new, r_new)`"""
    r = np.asarray(b, dtype=np.float64) - spmv64(K, x0, 8, True)
    x = np.array(x0, dtype=np.float64)
    for y, z in zip(ys, zs):
        x = _fma(np.full(x.size, float(y)), np.asarray(z, dtype=np.float64), x,
                 True)
        r = _fma(np.full(x.size, -float(y)), spmv64(K, z, 8, True), r, True)
    return x, r


# ---- the inputs of the GPU cases (shared with the CPU test) ------------------

DT = 5e-3


def toy_system(prob, dt=DT, scheme='cnab'):
    """`(F, J, K, R1, cf)` of the toy problem: CNAB (R1 = M - dt/2 A) or SBDF2
    (R1 = M, F = M + 2/3 dt A)"""
    M, A, J = (sps.csr_matrix(prob['smc'][k]) for k in 'MAJ')
    if scheme == 'cnab':
        F, R1 = (M + .5*dt*A).tocsr(), (M - .5*dt*A).tocsr()
        cf = dict(a_c=1., a_p=0., cn_c=1.5*dt, cn_o=-.5*dt)
    else:
        F, R1 = (M + 2./3*dt*A).tocsr(), M.tocsr()
        cf = dict(a_c=4./3, a_p=-1./3, cn_c=4./3*dt, cn_o=-2./3*dt)
    for X in (F, R1, J):
        X.sort_indices()
    K = sps.bmat([[F, J.T], [J, None]], format='csr')
    K.sort_indices()
    return F, J, K, R1, cf


def rough(seed, *shape):
    """standard normal, fixed seed: successive states differ at O(1)"""
    return np.random.default_rng(seed).standard_normal(shape)


def rough_inputs(nv, npr, seed=0):
    """the data of a case: `v_c`, `v_p`, `pt`, `nfc (2, nv)`, `g`, `gp`, the
    per-step convection vectors `nfc_new (8, nv)` and a table `gtab (4, nv)`,
    `gptab (4, np)`"""
    return dict(v_c=rough(seed + 1, nv), v_p=rough(seed + 2, nv),
                pt=rough(seed + 3, npr), nfc=rough(seed + 4, 2, nv),
                g=rough(seed + 5, nv), gp=rough(seed + 6, npr),
                nfc_new=rough(seed + 7, 8, nv), gtab=rough(seed + 8, 4, nv),
                gptab=rough(seed + 9, 4, npr))
