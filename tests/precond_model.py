"""NumPy/SciPy model of `z = P^-1 r` as the DEVICE defines it (test
infrastructure, HIP-free; nothing in the package imports it).

Read off the set-up code (`csrc/dns_amd.hip`: `setup_precond`,
`build_explicit`, `mg_prepare`, `build_mg_levels`, `upload_mg_ops`,
`schur_to_f32`; `csrc/hostcsr.hpp`: `host_cheb_poly`; `csrc/mg_host.hpp`), not
off the kernels.  `F` is symmetric here (the `pc_sym` branch of a
convection-dominated `F` is not modelled).

The operators
-------------
* `G = p(D^-1 F) D^-1`, the Chebyshev polynomial of `krylov_model.ChebJacobi`
  with the bounds the handle reports (`cheb_bounds()`), formed as the sparse
  matrix recurrence `X += Dm; R -= Dm DF; Dm = c1 Dm + c2 R` from `R = I`,
  `Dm = I/theta`, `G = (X + Dm) D^-1`.  `drop_tol`: `host_cheb_poly` drops ONCE,
  at the end of a row's recurrence, the entries `|g_ij| < tol max_j |g_ij|`
  and keeps the diagonal; so does `explicit_poly`.
* `Gc = [G, -G J^T]`, `JG = J G`, `S0 = J G J^T` -- NOT symmetrised.
  `fhat='cheb'` (recurrence form): `z_v` by the vector recurrence; the dense
  Schur matrix the device fills row `c` with `J Fh^-1 J^T e_c`, i.e. it
  inverts `S0^T`; the multigrid block works on `J D^-1 J^T`.
* Schur block: dense inverse; Jacobi `1/((J o J) D^-1)`; multigrid: Galerkin
  `S_{l+1} = P^T (S_l P)`, `dinv` as `mg_diagonals`, `lmax` by the 20 power
  iterations of `mg_jacobi_lmax`, `omega, omega2` as `mg_damping`, the first
  level `<= max(mg_dense_max, min(mg_dense_half_max, 16384))` dense.  One plain
  recursive V(nu, nu) from zero; two cycles `x1 = a1 V(b)`,
  `x2 = x1 + a2 V(b - S0 x1)` (`schur_mg_apply_fused`: fused V(2,2) with
  `mg_cycles = 2` only -- every other form runs one cycle whatever the option).
* Blocks: `z_p = -Sh^-1 r_p` (triangular), `z_p = -Sh^-1 (r_p - JG r_v)`
  (full), `z_v = Gc [r_v; z_p]`.

The store map (`store_map`)
---------------------------
Which operators the device holds in fp32 / half; the model rounds exactly
those (`astype(float32)`), everything else is fp64.

=========  ==========================================================
`Gc`       fp32 iff `fp32_store` and the explicit form (`gc32`; the
           sub-wave AND the streaming kernel read it)
`sinv`     fp32 iff `fp32_store` and `schur='dense'` (`sinv32`, rows
           padded to `sld = (NP + 3) & ~3`; the padding is never read).
           The Jacobi diagonal stays fp64
`JG`       fp64 in `apply_precond` and in front of the dense and Jacobi
           blocks (`k_tau_guard` reads `JG.vals`); fp32 in the GMRES
           cycle iff `fp32_store`, `streams(JG)` and `schur='mg'`
`cinv`     the coarsest level's inverse: half iff `mg_dense_max < n <=
           mg_dense_half_max` (`k_to_half_rows`: entries / (max|a|/1024)
           rounded to fp32, then to fp16; `k_gemv_half` stages `x` as
           fp32), else fp32 iff `fp32_store`, else fp64
`Apre`,    fp32 iff `fp32_store`, the level runs a fused cycle and the
`Rr`,      operator is streamed (`streams_mg`: `nnz >= min(stream_nnz,
`Qq`, `S`  mg_stream_nnz)`; `S` = the fused V(2,2)'s last sweep only --
           the residual between two cycles reads the fp64 values, and
           the fused V(1,1) never applies `S`).  The plain cycle keeps
           `S`, `P`, `P^T` in fp64 always
=========  ==========================================================

A fused operator in fp32 is a rounded `Apre/Rr/Qq`, not a rounded `S`: for
those forms -- and only those -- the model runs the cycle on the fused
operators (`cycle='fused22' | 'fused11'`, transcribed from `mg_fused22_ops`,
`mg_fused11_ops`).  Everywhere else it runs the plain cycle, and that the
device's fused operators give the same map is what the tests check.

Yardsticks
----------
`Precond.apply_abs_chain(r)`: the same chain with every entry, inverse and
vector replaced by its modulus and every subtraction by an addition.
`Precond.yardsticks(rs)`: `a >= |z|`, the same with the true linear map behind
every stage in the place of the product of the moduli behind it (never larger,
see there), and the part of it that passed through a half-precision level
(`a_half`).  The reference of `rho_ref`: the same model in `np.longdouble` on
dense arrays (`ld=True`; stored operators are data: it takes the rounded arrays
of the fp64 model, and the pattern of a dropped `G`).  `Bench` ties them
together for the tests; `python tests/precond_model.py` prints `WAKE_RHO`.
"""
import numpy as np
import scipy.sparse as sps

import krylov_model as km

U64 = 2.0**-53
U32 = 2.0**-24
LD = np.longdouble

STORE_KEYS = ('Gc', 'sinv', 'JG', 'cinv', 'Apre', 'Rr', 'Qq', 'S')


def store_map(fp32_store=False, fhat='explicit', schur='dense', half=False,
              cycle='plain', streaming=False, entry='apply'):
    """which operators are held in what precision (module docstring)"""
    st = dict((k, 'f64') for k in STORE_KEYS)
    if fp32_store:
        if fhat == 'explicit':
            st['Gc'] = 'f32'
            if streaming and entry == 'gmres' and schur == 'mg':
                st['JG'] = 'f32'
        if schur == 'dense':
            st['sinv'] = 'f32'
        if schur == 'mg':
            st['cinv'] = 'f32'
            if streaming and cycle == 'fused22':
                st.update(Apre='f32', Rr='f32', Qq='f32', S='f32')
            if streaming and cycle == 'fused11':
                st.update(Rr='f32', Qq='f32')
    if schur == 'mg' and half:
        st['cinv'] = 'f16'
    return st


def device_cycle(nu, fused=True, cycles_knob=0, levels=2, entry='apply'):
    """`(form, cycles)` the device runs for `set_schur_mg(.., nu)`, the options
    `mg_fused`, `mg_cycles` on one GPU below 1.5e6 unknowns (`setup_precond`:
    knob 0 means two cycles there; `mg_prepare`; `mg_two_for`): the fused
    V(1,1) exists for one cycle only, two cycles run on the fused V(2,2) only,
    and outside a one-column Krylov cycle only when the option says 2"""
    mg_cycles = cycles_knob if cycles_knob > 0 else 2
    form = 'plain'
    if levels > 1 and fused and nu == 2:
        form = 'fused22'
    elif levels > 1 and fused and nu == 1 and mg_cycles < 2:
        form = 'fused11'
    two = form == 'fused22' and mg_cycles >= 2 and \
        (cycles_knob == 2 or entry == 'gmres')
    return form, (2 if two else 1)


# ---- small algebra that works on CSR/float64 and on dense/longdouble --------
def _is_ld(A):
    return isinstance(A, np.ndarray)


def _rows(d, A):
    """diag(d) A"""
    return d[:, None]*A if _is_ld(A) else (sps.diags(d) @ A).tocsr()


def _cols(A, d):
    """A diag(d)"""
    return A*d[None, :] if _is_ld(A) else (A @ sps.diags(d)).tocsr()


def _hstack(A, B):
    return np.hstack([A, B]) if _is_ld(A) else sps.hstack([A, B], format='csr')


def _eye(n, like):
    return np.eye(n, dtype=LD) if _is_ld(like) else sps.identity(n, format='csr')


def _T(A):
    return np.ascontiguousarray(A.T) if _is_ld(A) else A.T.tocsr()


def _dense(A):
    return A if _is_ld(A) else np.asarray(A.todense())


def _round(A, kind):
    """the values of a stored operator as the device holds them"""
    if kind == 'f64':
        return A
    assert kind == 'f32', kind
    if _is_ld(A):
        return A.astype(np.float32).astype(A.dtype)
    A = sps.csr_matrix(A, copy=True)
    A.data = A.data.astype(np.float32).astype(np.float64)
    return A


def spmm_ld(A, X, chunk=96):
    """`A @ X`, `A` CSR (float64 entries, exact in longdouble), `X` dense
    longdouble: products and sums in longdouble"""
    A = sps.csr_matrix(A)
    A.sort_indices()
    X = np.asarray(X, dtype=LD)
    one = X.ndim == 1
    if one:
        X = X[:, None]
    out = np.zeros((A.shape[0], X.shape[1]), dtype=LD)
    lens = np.diff(A.indptr)
    rows = np.flatnonzero(lens > 0)
    if rows.size:
        vals = A.data.astype(LD)[:, None]
        for c0 in range(0, X.shape[1], chunk):
            prod = vals*X[A.indices, c0:c0 + chunk]
            out[rows, c0:c0 + chunk] = np.add.reduceat(
                prod, A.indptr[rows], axis=0)
    return out[:, 0] if one else out


def inv_ld(A):
    """Gauss-Jordan inverse with partial pivoting in longdouble"""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    W = np.hstack([A, np.eye(n, dtype=LD)])
    for k in range(n):
        p = k + int(np.argmax(np.abs(W[k:, k])))
        if p != k:
            W[[k, p]] = W[[p, k]]
        W[k] = W[k]/W[k, k]
        col = W[:, k].copy()
        col[k] = 0
        W -= col[:, None]*W[k][None, :]
    return W[:, n:]


def f32_slack(X, S):
    """what the fp32 copy of a COMPUTED inverse `X ~= S^-1` may differ by from
    `X.astype(float32)`.  Two fp64 inverses of one matrix differ in their last
    digits, and where that carries an entry across an fp32 rounding boundary
    either float is a correct content of the store.  The measure is taken
    from the model: `E = |X - inv_LAPACK(S)|` (5e-14 of `max |X|` on the 1289
    rows of the wake, nearly relative entry by entry), allowed four times and
    nowhere less than its median relative size, `d = 4 max(E, med(E/|X|) |X|)`.
    Returns the sparse matrix of `|float32(X + d) - float32(X - d)|`: zero
    except at a fraction `2 d / (2^-23 |x|)` of the entries -- none of 207 x
    207, 18 of 1289 x 1289 on the wake (tests/test_precond_model_cpu.py
    counts them).  Each reaches one pressure entry of `z` and the velocity
    entries its row of `G J^T` touches: 27 % of `z` on the wake carry a slack
    above the tolerance (1e-8 of `|z|` at most), the rest the tolerance
    alone"""
    aX = np.abs(X)
    E = np.abs(X - np.linalg.inv(S))
    rel = np.median(E[aX > 0]/aX[aX > 0])
    d = 4*np.maximum(E, rel*aX)
    lo = (X - d).astype(np.float32).astype(np.float64)
    hi = (X + d).astype(np.float32).astype(np.float64)
    return sps.csr_matrix(hi - lo)


GJ_MAX = 2048


def inv_gj(A):
    """the device's inverse (`k_gj_pivot`, `k_gj_update`): Gauss-Jordan in
    place, pivots on the diagonal as they come"""
    a = np.array(A, dtype=np.float64)
    for k in range(a.shape[0]):
        p = 1.0/a[k, k]
        prow, pcol = a[k, :]*p, a[:, k].copy()
        a -= np.outer(pcol, prow)
        a[k, :] = prow
        a[:, k] = -pcol*p
        a[k, k] = p
    return a


def _inv(A):
    """longdouble: the reference; float64: the device's algorithm up to
    `GJ_MAX` rows -- against LAPACK's inverse its own rounding uses up to 0.9
    of the tolerance on the 207-row Schur complement of degree 2 -- and
    LAPACK beyond, where the sweep over the whole matrix per row takes NumPy
    too long for a test (5 s at 1289 rows, 40 s at 2592: the one level of
    that size here is stored in half precision)"""
    if A.dtype == LD:
        return inv_ld(A)
    return inv_gj(A) if A.shape[0] <= GJ_MAX else np.linalg.inv(A)


# ---- the explicit polynomial -------------------------------------------------
def diag_inv(F):
    """`1 / diag(F)` (1 where the diagonal is zero) as the set-up forms it"""
    d = sps.csr_matrix(F).diagonal()
    return 1.0/np.where(d != 0.0, d, 1.0)


def _drop_mask(G, tol):
    """`host_cheb_poly`: keep `|g_ij| >= tol max_j |g_ij|` and the diagonal"""
    G = sps.csr_matrix(G)
    G.sort_indices()
    rowmax = np.maximum.reduceat(np.abs(G.data), G.indptr[:-1])
    rows = np.repeat(np.arange(G.shape[0]), np.diff(G.indptr))
    return (np.abs(G.data) >= tol*rowmax[rows]) | (G.indices == rows)


def explicit_poly(F, lo, hi, degree, drop_tol=0., ld=False, pattern=None):
    """`G` (CSR float64, or dense longdouble restricted to `pattern`)"""
    F = sps.csr_matrix(F)
    n = F.shape[0]
    cheb = km.ChebJacobi(F, degree=degree, lmin=lo, lmax=hi)
    dv = diag_inv(F)
    DF = (sps.diags(dv) @ F).tocsr()
    if ld:
        # transposed iterates: (Dm DF)^T = DF^T Dm^T, a sparse-left product
        lo_, hi_ = LD(lo), LD(hi)
        theta, delta = (hi_ + lo_)/2, (hi_ - lo_)/2
        dvl = 1/np.where(F.diagonal() != 0, F.diagonal().astype(LD), LD(1))
        DFT = F.T.tocsr()       # (diag(dv) F)^T X = F^T (dv * X)
        X = np.zeros((n, n), dtype=LD)
        R = np.eye(n, dtype=LD)
        Dm = R/theta
        sigma1 = theta/delta
        rho = 1/sigma1
        for _ in range(degree - 1):
            rho_new = 1/(2*sigma1 - rho)
            X += Dm
            R -= spmm_ld(DFT, dvl[:, None]*Dm)
            Dm = (rho_new*rho)*Dm + (2*rho_new/delta)*R
            rho = rho_new
        G = ((X + Dm).T)*dvl[None, :]
        if pattern is not None:
            mask = np.zeros((n, n), dtype=bool)
            P = sps.coo_matrix(pattern)
            mask[P.row, P.col] = True
            G = np.where(mask, G, LD(0))
        return np.ascontiguousarray(G)
    eye = sps.identity(n, format='csr')
    X = sps.csr_matrix((n, n))
    R = eye
    Dm = (eye/cheb.theta).tocsr()
    for c1, c2 in cheb.coeffs():
        X = X + Dm
        R = R - Dm @ DF
        Dm = c1*Dm + c2*R
    G = ((X + Dm) @ sps.diags(dv)).tocsr()
    G.sort_indices()
    if drop_tol > 0.:
        keep = _drop_mask(G, drop_tol)
        rows = np.repeat(np.arange(n), np.diff(G.indptr))
        G = sps.csr_matrix((G.data[keep], (rows[keep], G.indices[keep])),
                           shape=(n, n))
        G.sort_indices()
    return G


# ---- the multigrid Schur block ------------------------------------------------
def mg_level_count(sizes, dense_max=2000, half_max=0):
    """`mg_prepare`: `sizes` = rows of S_0 and columns of every prolongation"""
    lim = max(dense_max, min(half_max, 16384))
    L = len(sizes)
    for l in range(L - 1):
        if sizes[l] <= lim:
            return l + 1
    return L


def mg_jacobi_lmax(S, dj, iters=20):
    n = S.shape[0]
    ld = _is_ld(S)
    i = np.arange(n, dtype=np.float64)
    x = 1.0 + 0.5*np.sin(0.37*i + 1.0)
    if ld:
        x = x.astype(LD)
    lam = 1.0
    for _ in range(iters):
        y = dj*(S @ x)
        nx, ny = x @ x, y @ y
        lam = np.sqrt(ny/nx)
        x = y/np.sqrt(ny)
    return lam


def mg_damping(lmax, cheb, alpha):
    lmax = max(1e-300, lmax)
    om = om2 = 4/(3*lmax)
    if cheb:
        hi, lo = 1.05*lmax, lmax/alpha
        mid, rad = (hi + lo)/2, (hi - lo)/2
        c = type(lmax)(0.70710678118654752)     # (the device's constant)
        om, om2 = 1/(mid + rad*c), 1/(mid - rad*c)
    return om, om2


class Level(object):
    pass


def half_rows(C):
    """`k_to_half_rows`: `(H, scale, W)`, `H` the float16 entries of
    `C / scale` rounded to fp32 and then to fp16, as the kernel writes it down.
    A compiler may fold the two conversions into one (gfx950 code of this
    library does): `W` is what the product with `scale H` may differ by then,
    `scale |H1 - H|` with `H1` the entries rounded once -- zero except where
    the fp32 value is a tie of two halves, 6e-5 of the entries"""
    C = np.asarray(C, dtype=np.float64)
    m = np.abs(C).max()
    scale = m/1024.0 if m > 0 else 1.0
    X = C*(1.0/scale)
    H = X.astype(np.float32).astype(np.float16)
    H1 = X.astype(np.float16)
    W = sps.csr_matrix(scale*np.abs(H1.astype(np.float64) -
                                    H.astype(np.float64)))
    return H, scale, W


# ---- straight-line programs ---------------------------------------------------
class Prog(object):
    """the pressure part of `z = P^-1 r` as a list of stages
    `out = sum_k d_k o (A_k v[in_k])` (`d_k`: None, a scalar or a vector;
    `A_k`: None or a matrix; a stage of kind `'half'` reads its inputs rounded
    to fp32).  One list serves the value, the modulus chain and the tail
    operators."""

    def __init__(self, inputs):
        self.inputs = tuple(inputs)
        self.stages = []
        self.slack = {}     # stage -> (W, input): entries either way right

    def add(self, base, terms, kind='f64'):
        name = '%s.%d' % (base, len(self.stages))
        self.stages.append((name, terms, kind))
        return name

    def run(self, inputs, mode='value'):
        """`mode='value'`: `(v, g)`, the value of every stage and its LOCAL
        modulus `g = sum_k |d_k| (|A_k| |v[in_k]|)` on the actual inputs;
        `mode='chain'`: `(v, None)` with every entry and vector replaced by
        its modulus along the whole chain"""
        chain = mode == 'chain'
        v = dict((k, np.abs(x) if chain else x) for k, x in inputs.items())
        g = {}
        absm = {}

        def mabs(A):
            if id(A) not in absm:
                absm[id(A)] = abs(A)
            return absm[id(A)]

        def term(d, A, y, mod):
            if mod:
                y = np.abs(y)
                A = None if A is None else mabs(A)
                d = None if d is None else np.abs(d)
            if A is not None:
                y = A @ y
            return y if d is None else d*y
        for name, terms, kind in self.stages:
            val, loc = 0, 0
            for d, A, inp in terms:
                y = v[inp]
                if kind == 'half':
                    y = y.astype(np.float32).astype(y.dtype)
                val = val + term(d, A, y, chain)
                if not chain and y.dtype != LD:
                    loc = loc + term(d, A, y, True)
            v[name], g[name] = val, loc
        return v, (None if chain else g)

    def tails(self, final, n, visit):
        """`visit(name, kind, T_i)` per stage that `final` (of length `n`)
        depends on, `T_i = d v[final] / d v[out_i]` dense, last stage first"""
        B = {final: np.eye(n)}
        for name, terms, kind in reversed(self.stages):
            Bo = B.pop(name, None)
            if Bo is None:
                continue
            visit(name, kind, Bo)
            for d, A, inp in terms:
                if inp in self.inputs:
                    continue
                C = Bo
                if d is not None:
                    C = Bo*(np.asarray(d, dtype=np.float64)[None, :]
                            if np.ndim(d) else float(d))
                if A is not None:
                    C = np.asarray(C @ A)
                B[inp] = B[inp] + C if inp in B else C


class MgSchur(object):
    """the hierarchy on `S0` and one or two V(nu, nu) cycles"""

    def __init__(self, S0, prols, nu=2, dense_max=2000, half_max=0, cheb=True,
                 alpha=3.0, cycles=1, rho=0.3, store=None, cycle='plain',
                 stored=None):
        ld = _is_ld(S0)
        self.ld = ld
        self.nu, self.cycle, self.rho = nu, cycle, rho
        self.store = store_map() if store is None else store
        sizes = [S0.shape[0]] + [P.shape[1] for P in prols]
        L = mg_level_count(sizes, dense_max, half_max)
        # (`cycles`: what RUNS -- `device_cycle` -- not what the option says)
        self.two = cycles >= 2 and L > 1
        self.levels = []
        Sl = S0
        for l in range(L):
            lv = Level()
            lv.n = Sl.shape[0]
            lv.S = Sl
            self.levels.append(lv)
            if l == L - 1:
                break
            P = sps.csr_matrix(prols[l])
            P.sort_indices()
            lv.P = P.toarray().astype(LD) if ld else P
            lv.PT = _T(lv.P)
            d = Sl.diagonal() if not ld else np.diagonal(Sl)
            one = LD(1) if ld else 1.0
            lv.dinv = one/np.where(d != 0, d, one)
            lmax = mg_jacobi_lmax(Sl, lv.dinv)
            lv.lmax = lmax
            lv.omega, lv.omega2 = mg_damping(lmax, cheb and nu == 2,
                                             LD(alpha) if ld else alpha)
            SP = Sl @ lv.P
            if cycle != 'plain':
                self._fused_ops(lv, SP, l, stored)
            Sl = lv.PT @ SP
            if not ld:
                Sl = sps.csr_matrix(Sl)
        self.sizes = [lv.n for lv in self.levels]
        kind = self.store['cinv']
        self.half = kind == 'f16'
        if stored is not None and kind != 'f64':
            # (stored operators are data)
            self.cinv = stored.cinv.astype(LD)
            self.cscale = stored.cscale
        else:
            C = _inv(_dense(self.levels[-1].S))
            self.cscale = None
            if kind == 'f16':
                H, self.cscale, self.cslack = half_rows(C)
                C = H.astype(np.float64)
            elif kind == 'f32':
                C = C.astype(np.float32).astype(C.dtype)
            self.cinv = C

    def _fused_ops(self, lv, SP, l, stored):
        """`mg_fused22_ops` / `mg_fused11_ops`, rounded where stored in fp32"""
        S, P, PT, dv = lv.S, lv.P, lv.PT, lv.dinv
        eye = _eye(lv.n, S)
        w1, w2 = lv.omega, lv.omega2
        WS = _rows(w1*dv, S)
        PW = P - _rows(w1*dv, SP)
        if self.cycle == 'fused22':
            ops = dict(Apre=_cols((w1 + w2)*eye - w2*WS, dv),
                       Rr=_hstack(PT, -(PT @ S)),
                       Qq=_hstack(eye - WS, PW), S=S)
        else:
            Ap = _cols(2.0*eye - WS, w1*dv)
            ops = dict(Rr=PT - _cols(PT @ S, w1*dv), Qq=_hstack(Ap, PW))
            if l == 0:
                ops['Qq'] = -ops['Qq']
        lv.ops = {}
        for k, A in ops.items():
            kind = self.store[k]
            if stored is not None and kind != 'f64':
                A = _dense(stored.levels[l].ops[k]).astype(LD)
            else:
                A = _round(A, kind)
            lv.ops[k] = A

    # -- the cycles as stages ---------------------------------------------------
    def _coarse(self, pg, b):
        name = pg.add('xc', [(self.cscale, self.cinv, b)],
                      'half' if self.half else 'f64')
        if getattr(self, 'cslack', None) is not None and self.cslack.nnz:
            pg.slack[name] = (self.cslack, b)
        return name

    def _sweeps(self, pg, lv, b, x):
        om = (lv.omega, lv.omega2)
        for s in range(self.nu):
            wd = om[s & 1]*lv.dinv
            if x is None:
                x = pg.add('x', [(wd, None, b)])
            else:
                x = pg.add('x', [(None, None, x), (wd, None, b),
                                 (-wd, lv.S, x)])
        return x

    def _plain(self, pg, l, b):
        if l == len(self.levels) - 1:
            return self._coarse(pg, b)
        lv = self.levels[l]
        x = self._sweeps(pg, lv, b, None)
        r = pg.add('r', [(None, None, b), (-1.0, lv.S, x)])
        e = self._plain(pg, l + 1, pg.add('b', [(None, lv.PT, r)]))
        x = pg.add('x', [(None, None, x), (None, lv.P, e)])
        return self._sweeps(pg, lv, b, x)

    def _fused22(self, pg, l, b):
        if l == len(self.levels) - 1:
            return self._coarse(pg, b)
        lv = self.levels[l]
        o, n = lv.ops, lv.n
        x = pg.add('x', [(None, o['Apre'], b)])
        bc = pg.add('b', [(None, o['Rr'][:, :n], b), (None, o['Rr'][:, n:], x)])
        e = self._fused22(pg, l + 1, bc)
        x2 = pg.add('x', [(None, o['Qq'][:, :n], x), (None, o['Qq'][:, n:], e),
                          (lv.omega*lv.dinv, None, b)])
        wd = lv.omega2*lv.dinv
        return pg.add('x', [(None, None, x2), (wd, None, b), (-wd, o['S'], x2)])

    def _fused11(self, pg, l, b):
        """(the finest level's `Qq` is negated: level 0 returns `-V(b)`)"""
        if l == len(self.levels) - 1:
            return self._coarse(pg, b)
        o, n = self.levels[l].ops, self.levels[l].n
        e = self._fused11(pg, l + 1, pg.add('b', [(None, o['Rr'], b)]))
        return pg.add('x', [(None, o['Qq'][:, :n], b),
                            (None, o['Qq'][:, n:], e)])

    def V(self, pg, b):
        if len(self.levels) == 1:
            return self._coarse(pg, b)
        if self.cycle == 'plain':
            return self._plain(pg, 0, b)
        if self.cycle == 'fused22':
            return self._fused22(pg, 0, b)
        return pg.add('x', [(-1.0, None, self._fused11(pg, 0, b))])

    def weights(self):
        rho = LD(self.rho) if self.ld else self.rho
        mid, rad = 1 - rho/2, rho/2
        c = type(mid)(0.70710678118654752)
        return 1/(mid + rad*c), 1/(mid - rad*c)

    def solve(self, pg, b):
        """stages of `x ~= S0^-1 b` (the device returns `z_p = -x`)"""
        if not self.two:
            return self.V(pg, b)
        a1, a2 = self.weights()
        x1 = pg.add('x', [(a1, None, self.V(pg, b))])
        r2 = pg.add('r', [(None, None, b), (-1.0, self.levels[0].S, x1)])
        return pg.add('x', [(None, None, x1), (a2, None, self.V(pg, r2))])


# ---- the block preconditioner ------------------------------------------------
class Precond(object):
    """`z = P^-1 r`.  `lo, hi`: the handle's `cheb_bounds()`; `mg`: keywords of
    `MgSchur`; `store`: `store_map(...)`; `stored`: the float64 model whose
    rounded operators (and drop pattern) a longdouble model (`ld=True`) takes
    over as data; `symmetrise`: the WRONG `0.5 (S0 + S0^T)` (a mutation of the
    tests); `cache`: a dict that keeps `G`, `G J^T`, `J G`, `S0` between
    models of the same polynomial"""

    def __init__(self, F, J, lo, hi, degree=4, schur='dense',
                 fact='triangular', fhat='explicit', drop_tol=0., prols=None,
                 mg=None, store=None, ld=False, stored=None, symmetrise=False,
                 cache=None):
        self.F, self.J = sps.csr_matrix(F), sps.csr_matrix(J)
        self.NP, self.NV = self.J.shape
        self.schur, self.fact, self.fhat, self.ld = schur, fact, fhat, ld
        self.store = store_map() if store is None else dict(store)
        self.cheb = km.ChebJacobi(self.F, degree=degree, lmin=lo, lmax=hi)
        self.degree = degree
        explicit = fhat == 'explicit'
        assert explicit or fact == 'triangular'
        key = (float(lo), float(hi), degree, float(drop_tol) if explicit
               else 0., ld)
        ops = None if cache is None else cache.get(key)
        if ops is None:
            ops = self._form(lo, hi, degree, drop_tol if explicit else 0., ld,
                             stored)
            if cache is not None:
                cache[key] = ops
        G, GJT, JG, S0 = ops
        self.G, self.GJT = G, GJT
        dvF = diag_inv(self.F)
        if ld:
            dvF = 1/np.where(self.F.diagonal() != 0,
                             self.F.diagonal().astype(LD), LD(1))
        self.dvF = dvF

        def take(name, make):
            kind = self.store[name]
            if stored is not None and kind != 'f64':
                return _dense(getattr(stored, name)).astype(LD)
            return _round(make(), kind)
        if explicit:
            self.Gc = take('Gc', lambda: _hstack(G, -GJT))
            if fact == 'full':
                self.JG = take('JG', lambda: JG)
        if symmetrise:
            S0 = (S0 + S0.T)/2
            if not ld:
                S0 = sps.csr_matrix(S0)
        self.S0 = S0
        if schur == 'dense':
            # (recurrence form: the device fills ROW c with S0 e_c)
            Sd = _dense(S0) if explicit else _dense(S0).T

            def inverse():
                ikey = ('inv', key, explicit, symmetrise)
                if cache is None:
                    return _inv(np.ascontiguousarray(Sd))
                if ikey not in cache:
                    cache[ikey] = _inv(np.ascontiguousarray(Sd))
                return cache[ikey]
            self.sinv = take('sinv', inverse)
            self.sinv_slack = None
            if self.store['sinv'] == 'f32' and not ld:
                self.sinv_slack = f32_slack(inverse(), Sd)
        elif schur == 'jacobi':
            JJ = self.J.multiply(self.J).tocsr()
            self.sdiag = 1/(spmm_ld(JJ, dvF) if ld else JJ @ dvF)
        else:
            if not explicit:
                if ld:
                    JT = self.J.T.tocsr()
                    S0 = np.hstack([spmm_ld(self.J, dvF[:, None]*JT[
                        :, c:c + 96].toarray().astype(LD))
                        for c in range(0, self.NP, 96)])
                else:
                    S0 = (self.J @ (sps.diags(dvF) @ self.J.T)).tocsr()
                self.S0 = S0
            kw = dict(mg or {})
            self.mg = MgSchur(S0, prols, store=self.store,
                              stored=None if stored is None else stored.mg,
                              **kw)

    def _form(self, lo, hi, degree, drop_tol, ld, stored):
        J = self.J
        if ld and self.fhat != 'explicit' and self.schur != 'dense':
            return None, None, None, None   # (nothing here reads the matrix)
        if ld:
            pat = None if stored is None else stored.G
            G = explicit_poly(self.F, lo, hi, degree, ld=True, pattern=pat)
            GJT = _T(spmm_ld(J, _T(G)))             # G J^T = (J G^T)^T
            return G, GJT, spmm_ld(J, G), spmm_ld(J, GJT)
        G = explicit_poly(self.F, lo, hi, degree, drop_tol)
        GJT = (G @ J.T).tocsr()
        return G, GJT, (J @ G).tocsr(), (J @ GJT).tocsr()

    # -- pieces -----------------------------------------------------------------
    def _fhat_vec(self, b):
        """the Chebyshev vector recurrence (`fhat='cheb'`)"""
        if not self.ld:
            return self.cheb.apply(b)
        lo, hi = LD(self.cheb.lmin), LD(self.cheb.lmax)
        theta, delta = (hi + lo)/2, (hi - lo)/2
        r = self.dvF*b
        d = r/theta
        x = np.zeros_like(b)
        sigma1 = theta/delta
        rho = 1/sigma1
        for _ in range(self.degree - 1):
            rho_new = 1/(2*sigma1 - rho)
            x = x + d
            r = r - self.dvF*spmm_ld(self.F, d)
            d = (rho_new*rho)*d + (2*rho_new/delta)*r
            rho = rho_new
        return x + d

    def _fhat_abs(self, b):
        """modulus of the recurrence: every term of the polynomial added"""
        aF = abs(self.F)
        dv = np.abs(self.dvF)
        r = dv*b
        d = r/self.cheb.theta
        x = np.zeros_like(b)
        for c1, c2 in self.cheb.coeffs():
            x = x + d
            r = r + dv*(aF @ d)
            d = abs(c1)*d + abs(c2)*r
        return x + d

    def program(self):
        """`(stages, name of the last one)`: `z_p` of `r = [rv; rp]`"""
        pg = Prog(('rv', 'rp'))
        t = 'rp'
        if self.fact == 'full':
            t = pg.add('t', [(None, None, 'rp'), (-1.0, self.JG, 'rv')])
        if self.schur == 'dense':
            x = pg.add('x', [(None, self.sinv, t)])
        elif self.schur == 'jacobi':
            x = pg.add('x', [(self.sdiag, None, t)])
        else:
            x = self.mg.solve(pg, t)
        return pg, pg.add('zp', [(-1.0, None, x)])

    def apply(self, r):
        r = np.asarray(r, dtype=LD if self.ld else np.float64)
        rv, rp = r[:self.NV], r[self.NV:]
        pg, last = self.program()
        zp = pg.run(dict(rv=rv, rp=rp))[0][last]
        if self.fhat == 'explicit':
            zv = self.Gc @ np.concatenate([rv, zp])
        else:
            JT = self.J.T.tocsr()
            zv = self._fhat_vec(rv - (spmm_ld(JT, zp) if self.ld else JT @ zp))
        return np.concatenate([zv, zp])

    def yardsticks(self, rs):
        """`[(a, a_half), ..]` per right-hand side, the yardstick of the
        forward error: with the stages `y_i = A_i(y_j, ..)` of `program()`,
        `g_i` = the modulus of stage `i` on its ACTUAL inputs and `T_i` = the
        linear map from `y_i` to the result,

            a = max_i |T_i| g_i   >=  |z|      (the last stage has T = I)

        -- a rounding error of relative size `u` in stage `i` moves `z` by at
        most `u |T_i| g_i`.  The velocity block of the explicit form takes
        `T_i` through `z_v = Gc [r_v; z_p]`, the recurrence form through the
        `-G J^T` it realises, with the modulus of the recurrence as its own
        stage.
        `a_half`: the terms of a half-precision coarsest level alone (its
        sums are fp32).  Entry by entry `a <= apply_abs_chain(r)`, the product
        of the moduli along the whole chain: the same yardstick wherever no
        stage cancels, and the only usable one through a multigrid cycle,
        whose chain of moduli exceeds `|z|` by 7e3 (one V(2,2)) to 1e11 (two
        cycles) on the 207 / 47 / 11 hierarchy of the tests."""
        assert not self.ld
        NV, NP = self.NV, self.NP
        explicit = self.fhat == 'explicit'
        pg, last = self.program()
        runs = []
        for r in rs:
            r = np.asarray(r, dtype=np.float64)
            v, g = pg.run(dict(rv=r[:NV], rp=r[NV:]))
            runs.append((r, v, g, np.zeros(NV), np.zeros(NP), np.zeros(NV),
                         np.zeros(NP)))
        self.yard_slack = [np.zeros(NV + NP) for _ in rs]
        # (the recurrence form: G J^T is the linear map it realises)
        GJ = self.Gc[:, NV:] if explicit else self.GJT

        def visit(name, kind, Bo):
            Tp, Tv = np.abs(Bo), np.abs(GJ @ Bo)
            if name in pg.slack:
                # (entries of a half-precision store that are right either
                # way, `half_rows`: what they multiply, through the rest)
                W, inp = pg.slack[name]
                for (r, v), sl in zip([q[:2] for q in runs], self.yard_slack):
                    e = W @ np.abs(v[inp].astype(np.float32).astype(float))
                    sl += np.concatenate([Tv @ e, Tp @ e])
            for r, v, g, av, ap, avh, aph in runs:
                for T, a, ah in ((Tp, ap, aph), (Tv, av, avh)):
                    t = T @ g[name]
                    np.maximum(a, t, out=a)
                    if kind == 'half':
                        ah += t
        pg.tails(last, NP, visit)
        out = []
        for r, v, g, av, ap, avh, aph in runs:
            arv, azp = np.abs(r[:NV]), np.abs(v[last])
            if explicit:
                gv = abs(self.Gc) @ np.concatenate([arv, azp])
            else:
                gv = self._fhat_abs(arv + abs(self.J.T.tocsr()) @ azp)
            out.append((np.concatenate([np.maximum(av, gv), ap]),
                        np.concatenate([avh, aph])))
        return out

    def slack(self, r):
        """entry by entry, what `z` may differ by beyond rounding (beside
        `yard_slack`, the same for a half-precision level, which
        `yardsticks` leaves): the
        ambiguous entries of an fp32 dense Schur inverse (`f32_slack`) times
        what they multiply, through `z_v = -G J^T z_p`; zero otherwise"""
        W = getattr(self, 'sinv_slack', None)
        if W is None or W.nnz == 0:
            return np.zeros(self.NV + self.NP)
        r = np.asarray(r, dtype=np.float64)
        t = r[self.NV:]
        if self.fact == 'full':
            t = t - self.JG @ r[:self.NV]
        e = W @ np.abs(t)
        GJ = self.Gc[:, self.NV:] if self.fhat == 'explicit' else self.GJT
        return np.concatenate([abs(GJ) @ e, e])

    def apply_abs_chain(self, r):
        """the same chain with every entry, inverse and vector replaced by its
        modulus and every subtraction by an addition"""
        r = np.abs(np.asarray(r, dtype=np.float64))
        rv, rp = r[:self.NV], r[self.NV:]
        pg, last = self.program()
        ap = pg.run(dict(rv=rv, rp=rp), mode='chain')[0][last]
        if self.fhat == 'explicit':
            av = abs(self.Gc) @ np.concatenate([rv, ap])
        else:
            av = self._fhat_abs(rv + abs(self.J.T.tocsr()) @ ap)
        return np.concatenate([av, ap])


# ---- the yardstick --------------------------------------------------------------
def blocks(v, NV):
    return v[:NV], v[NV:]


def rho_ref(model, ref, rs, yard=None):
    """`rho = ||z64 - z_ld|| / (2^-53 ||a||)` per right-hand side and block
    (inf norms): a list of pairs"""
    yard = model.yardsticks(rs) if yard is None else yard
    out = []
    for r, (a, _) in zip(rs, yard):
        z, zl = model.apply(r), ref.apply(r)
        pair = [0., 0.]
        for k in (0, 1):
            d = np.abs(blocks(z.astype(LD) - zl, model.NV)[k]).max()
            ak = blocks(a, model.NV)[k].max()
            if ak > 0.:         # (else the block is zero by construction)
                pair[k] = round(float(d/(U64*ak)), 3)
        out.append(tuple(pair))
    return out


def rho_max(rhos):
    """the largest `rho_ref` of each block over the right-hand sides"""
    return tuple(max(p[k] for p in rhos) for k in (0, 1))


def tolerance(model, yard, rho):
    """`16 max(rho, 1) (2^-53 ||a|| + 2^-24 ||a_half||)` per block; `yard`:
    one `(a, a_half)` of `yardsticks`; `rho`: its pair of `rho_ref`"""
    a, ah = yard
    return tuple(16*max(rho[k], 1.)*(U64*blocks(a, model.NV)[k].max() +
                                     U32*blocks(ah, model.NV)[k].max())
                 for k in (0, 1))


def right_hand_sides(M, NP, seed=3, rp_scale=1e-3):
    """`[r_v; r_p] = [M w; rp_scale q]` with random `w`, `q` (1e-3: the scaling
    of a time step's right-hand side), the same with `r_p = 0` (the
    warm-started time step) and with `r_v = 0`"""
    rng = np.random.default_rng(seed)
    NV = M.shape[0]
    r = np.concatenate([M @ rng.standard_normal(NV),
                        rp_scale*rng.standard_normal(NP)])
    r1, r2 = r.copy(), r.copy()
    r1[NV:] = 0.
    r2[:NV] = 0.
    return [r, r1, r2]


# ---- from the device's options to the model -------------------------------------
FORM_DEFAULTS = dict(schur='dense', fact='triangular', fhat='explicit', fp32=0,
                     drop=0., degree=4, nu=2, fused=1, cheb=1, cycles=1,
                     streaming=0, pair=1, dense_max=20, half_max=0)


def form_of(**kw):
    f = dict(FORM_DEFAULTS)
    assert set(kw) <= set(f), kw
    f.update(kw)
    return f


def form_id(f):
    d = FORM_DEFAULTS
    return '-'.join([f['schur'], f['fact'][:3], f['fhat'][:4], 'd%d' % f['degree']]
                    + ['%s%g' % (k, f[k]) for k in
                       ('fp32', 'drop', 'nu', 'fused', 'cheb', 'cycles',
                        'streaming', 'pair', 'dense_max', 'half_max')
                       if f[k] != d[k]])


def mg_sizes(J, prols):
    return [J.shape[0]] + [P.shape[1] for P in (prols or [])]


def build(F, J, lo, hi, f, prols=None, entry='apply', cache=None, ld=False,
          stored=None, **kw):
    """the model of the form `f` (`form_of`): the device's options mapped to
    what runs (`device_cycle`) and what is stored how (`store_map`)"""
    mg, cycle, half = None, 'plain', False
    if f['schur'] == 'mg':
        sizes = mg_sizes(J, prols)
        L = mg_level_count(sizes, f['dense_max'], f['half_max'])
        cycle, cyc = device_cycle(f['nu'], f['fused'], f['cycles'], L, entry)
        half = f['dense_max'] < sizes[L - 1] <= f['half_max']
        mg = dict(nu=f['nu'], dense_max=f['dense_max'], half_max=f['half_max'],
                  cheb=bool(f['cheb']), cycles=cyc)
    store = store_map(bool(f['fp32']), f['fhat'], f['schur'], half, cycle,
                      bool(f['streaming']), entry)
    if mg is not None:
        # (the fused operators only where they are what is rounded)
        mg['cycle'] = cycle if store['Rr'] == 'f32' else 'plain'
    args = dict(degree=f['degree'], schur=f['schur'], fact=f['fact'],
                fhat=f['fhat'], drop_tol=f['drop'], prols=prols, mg=mg,
                store=store, cache=cache, ld=ld, stored=stored)
    args.update(kw)
    return Precond(F, J, lo, hi, **args)


# every value of every knob at least once, and every pair that meets in one
# launch (tests/test_gpu_precond_forms.py)
TOY_FORMS = [
    form_of(fhat='cheb', degree=1),
    form_of(fhat='cheb', fp32=1),
    form_of(degree=1),
    form_of(fact='full', degree=6, drop=1e-3, fp32=1),
    form_of(schur='jacobi'),
    form_of(schur='jacobi', fact='full', fp32=1, drop=1e-3),
    form_of(fact='full', streaming=1),
    form_of(fact='full', streaming=1, fp32=1, pair=0),
    # multigrid, 207 / 47 / 11
    form_of(schur='mg', fact='full', fused=0),
    form_of(schur='mg', fused=0, nu=1, cheb=0, fp32=1),
    form_of(schur='mg', fact='full'),
    form_of(schur='mg', cycles=2, cheb=0, fp32=1, drop=1e-3, degree=6),
    form_of(schur='mg', fact='full', nu=1),
    form_of(schur='mg', fused=0, streaming=1),
    form_of(schur='mg', fact='full', streaming=1, fp32=1),
    form_of(schur='mg', nu=1, streaming=1, fp32=1, pair=0),
    form_of(schur='mg', fact='full', cycles=2, streaming=1),
    form_of(schur='mg', fhat='cheb', cycles=0),
    # the 47-row level dense in half precision (ldh = 48)
    form_of(schur='mg', fact='full', half_max=64),
    form_of(schur='mg', fused=0, half_max=64, fp32=1),
]

# cylinder wake N = 2 (NV 9356, NP 1289; 1289 / 296 / 66 with `coarsest=100`):
# dense rows of more than 256 columns, row lengths across the kernels'
# lanes-per-row instantiations
WAKE_FORMS = [
    form_of(fact='full', fp32=1, drop=1e-3),
    form_of(fact='full', drop=1e-3),
    form_of(schur='mg', fact='full', drop=1e-3, dense_max=100),
    form_of(schur='mg', fused=0, fp32=1, drop=1e-3, dense_max=300),
    form_of(schur='mg', streaming=1, fp32=1, drop=1e-3, dense_max=100),
]


# `rho_ref` of WAKE_FORMS per right-hand side (velocity, pressure block): the
# dense longdouble polynomial of 9356 x 9356 takes four minutes, so these are
# computed once (`python tests/precond_model.py`) -- from the model alone,
# Chebyshev bounds by `krylov_model.power_bounds`
WAKE_RHO = {
    'dense-ful-expl-d4-fp321-drop0.001':
        [(0.318, 0.674), (0.367, 0.296), (0.263, 0.786)],
    'dense-ful-expl-d4-drop0.001':
        [(0.324, 14.124), (0.338, 0.788), (0.291, 14.924)],
    'mg-ful-expl-d4-drop0.001-dense_max100':
        [(0.346, 0.233), (0.265, 0.193), (1.034, 0.904)],
    'mg-tri-expl-d4-fp321-drop0.001-fused0-dense_max300':
        [(0.972, 0.048), (2.639, 0.0), (0.757, 0.048)],
    'mg-tri-expl-d4-fp321-drop0.001-streaming1-dense_max100':
        [(0.907, 0.1), (2.639, 0.0), (0.441, 0.1)],
}

# ... and of the one case on the N = 3 cylinder (NP 2592 as one dense level in
# half precision, recurrence form, triangular): 12 s in longdouble, recomputed
# by tests/test_precond_model_cpu.py
HALF_RHO = [(0.012, 0.008), (0.173, 0.0), (0.013, 0.008)]


class Bench(object):
    """a system, its hierarchy and right-hand sides, and per form the model,
    its yardsticks, `rho_ref` and the tolerances of the three right-hand
    sides (`form`)"""

    def __init__(self, M, F, J, prols=None, lo=None, hi=None, rp_scale=1e-3):
        self.M, self.F, self.J = (sps.csr_matrix(X) for X in (M, F, J))
        self.NP, self.NV = self.J.shape
        self.prols = prols
        if lo is None:
            lo, hi = km.power_bounds(self.F, 1/self.F.diagonal())
            lo, hi = 0.9*lo, 1.05*hi
        self.lo, self.hi = lo, hi
        self.rs = right_hand_sides(self.M, self.NP, rp_scale=rp_scale)
        self.c64, self.cld, self.done = {}, {}, {}

    def model(self, f, lo=None, hi=None, entry='apply', **kw):
        return build(self.F, self.J, self.lo if lo is None else lo,
                     self.hi if hi is None else hi, f, self.prols, entry=entry,
                     cache=self.c64, **kw)

    def form(self, f, lo=None, hi=None, entry='apply', rho=None):
        """`(model, yardsticks, rho_ref, tolerances, slacks)`, the last three
        per right-hand side; `rho`: a `rho_ref` known already (no longdouble
        model then)"""
        lo = self.lo if lo is None else lo
        hi = self.hi if hi is None else hi
        m = self.model(f, lo, hi, entry)
        key = (form_id(f), lo, hi, tuple(sorted(m.store.items())),
               m.schur == 'mg' and (m.mg.cycle, m.mg.two))
        if key not in self.done:
            yard = m.yardsticks(self.rs)
            if rho is None:
                ref = build(self.F, self.J, lo, hi, f, self.prols, entry=entry,
                            cache=self.cld, ld=True, stored=m)
                rho = rho_ref(m, ref, self.rs, yard)
            rho = [tuple(p) for p in rho]
            assert len(rho) == len(self.rs)
            tols = [tolerance(m, y, p) for y, p in zip(yard, rho)]
            self.done[key] = (m, yard, rho, tols,
                              [m.slack(r) + ys for r, ys in
                               zip(self.rs, m.yard_slack)])
        return self.done[key]

    def excess(self, done, zs, detail=None):
        """largest `|zs[i] - z_model(rs[i])| / tolerance` over the blocks and
        right-hand sides, `done = form(..)`; `detail`: a list that takes the
        ratio of every right-hand side and block"""
        m, tols, slacks = done[0], done[3], done[4]
        worst = 0.
        for r, z, tol, sl in zip(self.rs, zs, tols, slacks):
            d = np.abs(z - m.apply(r))
            for k in (0, 1):
                dk = blocks(d, self.NV)[k]
                if tol[k] > 0.:
                    # (entry by entry: `slack` is zero on most of them)
                    q = float((dk/(tol[k] + blocks(sl, self.NV)[k])).max())
                    worst = max(worst, q)
                    if detail is not None:
                        detail.append(round(q, 3))
                else:           # (a block that is zero by construction)
                    assert dk.max() == 0.
        return worst

    def apply_excess(self, system, f, rho=None, detail=None):
        """Entry A on a handle that is set up as the form `f` says: the
        largest `error / tolerance` of `apply_precond` over the right-hand
        sides; a second call must return the same bits (stale level buffers,
        first-use allocations)"""
        lo, hi = system.cheb_bounds()
        done = self.form(f, lo, hi, rho=rho)
        zs = [system.apply_precond(r) for r in self.rs]
        for r, z in zip(self.rs, zs):
            assert np.array_equal(z, system.apply_precond(r)), \
                'a second apply returns other bits'
        return self.excess(done, zs, detail), done


class Wake(object):
    """the N = 2 cylinder wake of WAKE_FORMS (dt = 1/512, `coarsest=100`).
    Two sets of right-hand sides: behind the full factorisation with
    `r_p = 1e-3 q` the dense block sees `-J G r_v` alone, which leaves `|z_p|`
    at 5e-4 of its yardstick, and with the 6e4 condition of the 1289-row
    Schur complement the fp64 dense form's tolerance comes to 6e-11 `|z|`: a
    badly scaled input for that block.  The dense forms take `r_p = q`."""

    def __init__(self):
        from dolfin_navier_scipy_amd import amg
        from dolfin_navier_scipy_amd.fem import get_sysmats
        _, sm, _ = get_sysmats(problem='cylinderwake', N=2, Re=100)
        F = (sm['M'] + sm['A']/1024.).tocsr()
        prols = amg.algebraic_prolongations(F, sm['J'], coarsest=100)
        self.mg = Bench(sm['M'], F, sm['J'], prols)
        self.dense = Bench(sm['M'], F, sm['J'], prols, self.mg.lo, self.mg.hi,
                           rp_scale=1.0)
        self.dense.c64 = self.mg.c64        # (one polynomial)
        self.dense.cld = self.mg.cld

    def bench(self, f):
        return self.dense if f['schur'] == 'dense' else self.mg


def _wake_table():
    w = Wake()
    for f in WAKE_FORMS:
        print(repr(form_id(f)) + ':', w.bench(f).form(f)[2], flush=True)


if __name__ == '__main__':
    _wake_table()
