"""A NumPy `longdouble` model of the P2 convection forms and of the assembly
pair of a trapezoidal step, written from the mathematics:

    N(u)u [(a,i)]       = int phi_a (u . grad) u_i
    N1(u) [(a,i),(b,k)] = delta_ik int phi_a (u . grad phi_b)         (Picard)
    N2(u) [(a,i),(b,k)] = int phi_a phi_b d_k u_i                    (+ Newton)

on the raw element data of the C API (`cell_vdofs (nc,6,2)`, `glam (nc,3,2)`,
`area (nc,)`, `invinds`, `dbcinds`, Dirichlet values), with the 7-point
degree-5 rule; rule and shape functions come from their closed forms with
`sqrt(15)` in long double.  The fp64 inputs are the exact data of the model.

Every quantity has a MAGNITUDE TWIN: the same sum with every factor replaced
by its absolute value, `sum |terms|`.  The bound of an entry is

    sum over its groups of terms of  gamma_k * (magnitude of the group),
    gamma_k = k u / (1 - k u),  u = 2^-53,

`k` the largest number of roundings a term of the group passes through in the
device kernels, counted from their operation chains (a fused multiply-add is
one rounding; adding an exact zero is none; a sum of `len` numbers in ANY
order and bracketing -- serial, sixteen lanes and a shuffle tree -- puts a
term through at most `len - 1` additions):

  T, the fp64 tables: a term holds one weight, two shape functions and one
     gradient; each table's distance from the long double one is MEASURED
     here in units of u (`table_ulps`), T = ulp(qw) + 2 ulp(phi) + ulp(dphi)
  cell values of N(u)u (both element kernels, `conv_point`):
     gx/gy 3, g 6, uq 6, cv 3, weight 1, product 1, tree over the points 3
                                                       K_VEC    = 23 + T
  local matrices: grad phi_b 3, uq 6, u . grad phi_b 2, w |T| phi_a 2, seven
     accumulations 7 (N1: 20); N2: g 9, w |T| phi_a phi_b 3, 7 (19); the sum
     N1 + N2 of a Newton entry 1                       K_MAT    = 21 + T
  N(v)v as N1_cell u_cell (Newton, matrix family): N1 20, six fma
                                                       K_CLIN   = 26 + T
  L_cell x0_cell: 20 and up to eighteen fma            K_CX0    = 38 + T
  gathers: + len - 1 (sums), + len (fma sums: the product is in it);
     `scale`: + 1
  F = M + hdt (A + N): N + 3, A 3, M 1   (hdt = dt/2 is data, taken as it is)
  trapezoidal rows: fvn = fv - s + rc: + 2;  fc = fv_c - cc: + 1;
     (M - hdt A) v_c: 2 + len_row;  b = acc + hdt (fn + fc): + 3;
     K x0 per lane: the row (1 + len_row), hdt nx (+ 1), the row of J^T
     (+ len_jt), the tree -- every group of r gets len_row + len_jt + 6 on top
     of its own count, and 1 for r = b - K x0
  pressure rows: r_p = fp - J x0: len_j + 1;  b_p = fp exactly
  norm sums: 2 sum |r_i| e_i + gamma_(n+2) sum r_i^2

Margins measured on the CPU (tests/test_conv_model_cpu.py prints them with
`pytest -s`), largest error / bound per quantity.  The tables are 2 u (qw),
10 u (phi) and 11 u (dphi) away from the long double ones: T = 33.
  fp64 evaluation, summation orders shuffled (toy mesh, fan, rectangles with
  and without Dirichlet dofs; Picard and Newton):
     cell values 0.164  N1 0.176  N1+N2 0.179  N(u)u 0.154  N Picard 0.173
     N Newton 0.169  rhsbc 0.156  F 0.985  fvn 0.450  b 0.336  r 0.277
     ||r||^2 0.005  ||b||^2 0.004
  host assembler `fem.TaylorHood` (toy mesh and fan, full space):
     vector 0.038 (2.26 u x magnitude sum at the worst row), N1 0.114,
     N2 0.098
  (F: the last rounding of an entry that M dominates is half an ulp of the
  entry against gamma_1 |M|: a margin near 1 is what the count gives.)
"""
import numpy as np

LD = np.longdouble
U = LD(2.0)**-53
EDGE_OF = ((1, 2), (0, 2), (0, 1))


def gamma(k):
    k = np.asarray(k, dtype=LD)
    return k*U/(1 - k*U)


def tables(dtype=LD):
    """`(qw (7,), phi (7,6), dphi (7,6,3))` in `dtype`, by the closed forms"""
    one = dtype(1)
    s15 = np.sqrt(dtype(15))
    t1, t2 = (6 - s15)/21, (6 + s15)/21
    w1, w2 = (155 - s15)/1200, (155 + s15)/1200
    third = one/3
    qp = np.array([[third, third, third],
                   [1 - 2*t1, t1, t1], [t1, 1 - 2*t1, t1], [t1, t1, 1 - 2*t1],
                   [1 - 2*t2, t2, t2], [t2, 1 - 2*t2, t2], [t2, t2, 1 - 2*t2]],
                  dtype=dtype)
    qw = np.array([dtype(9)/40, w1, w1, w1, w2, w2, w2], dtype=dtype)
    phi = np.zeros((7, 6), dtype=dtype)
    dphi = np.zeros((7, 6, 3), dtype=dtype)
    for k in range(3):
        phi[:, k] = qp[:, k]*(2*qp[:, k] - 1)
        dphi[:, k, k] = 4*qp[:, k] - 1
        i, j = EDGE_OF[k]
        phi[:, 3 + k] = 4*qp[:, i]*qp[:, j]
        dphi[:, 3 + k, i] = 4*qp[:, j]
        dphi[:, 3 + k, j] = 4*qp[:, i]
    return qw, phi, dphi


def table_ulps():
    """distance of the fp64 tables from the long double ones, in units of u
    per entry, rounded up: `(qw, phi, dphi)`"""
    out = []
    for t64, tld in zip(tables(np.float64), tables(LD)):
        nz = tld != 0
        assert np.all(t64[~nz] == 0)
        rel = np.abs(t64[nz].astype(LD) - tld[nz])/np.abs(tld[nz])/U
        out.append(int(np.ceil(float(rel.max()))))
    return tuple(out)


_TU = table_ulps()
T_TAB = _TU[0] + 2*_TU[1] + _TU[2]
K_VEC = 23 + T_TAB
K_MAT = 21 + T_TAB
K_CLIN = 26 + T_TAB
K_CX0 = 38 + T_TAB


def cell_quantities(glam, area, ul, dtype=LD, absval=False, rng=None):
    """per cell: `vec (nc,12)` the cell values of N(u)u, `n1`, `n12 (nc,12,12)`
    the local matrices of N1(u) and N1(u) + N2(u); slot = 2 * node + component.
    `ul (nc,6,2)` the twelve local velocity values.  `absval`: the magnitude
    twin.  `dtype=float64` with `rng`: an evaluation in working precision with
    the sums over points and nodes taken in a random order."""
    qw, phi, dphi = tables(dtype)
    glam, area, ul = (np.asarray(x).astype(dtype) for x in (glam, area, ul))
    if absval:
        qw, phi, dphi, glam, area, ul = (np.abs(x) for x in
                                         (qw, phi, dphi, glam, area, ul))
    nc = area.size
    qo = np.arange(7) if rng is None else rng.permutation(7)
    ao = np.arange(6) if rng is None else rng.permutation(6)

    def ssum(terms):            # sum of a list in the list's order
        s = terms[0]
        for t in terms[1:]:
            s = s + t
        return s
    vec = []
    n1t, n2t = [], []
    for q in qo:
        gphi = ssum([dphi[q][None, :, k, None]*glam[:, None, k, :]
                     for k in (range(3) if rng is None else rng.permutation(3))])
        uq = ssum([phi[q, a]*ul[:, a, :] for a in ao])              # (nc,2)
        g = ssum([gphi[:, a, None, :]*ul[:, a, :, None] for a in ao])  # c,i,d
        w = qw[q]*area                                               # (nc,)
        cv = w[:, None]*(g[:, :, 0]*uq[:, None, 0] + g[:, :, 1]*uq[:, None, 1])
        vec.append(phi[q][None, :, None]*cv[:, None, :])            # c,a,i
        ugp = gphi[:, :, 0]*uq[:, None, 0] + gphi[:, :, 1]*uq[:, None, 1]
        wa = w[:, None]*phi[q][None, :]                             # c,a
        n1t.append(wa[:, :, None]*ugp[:, None, :])                  # c,a,b
        wab = wa[:, :, None]*phi[q][None, None, :]                  # c,a,b
        n2t.append(wab[:, :, :, None, None]*g[:, None, None, :, :])  # c,a,b,i,k
    vec = ssum(vec).reshape(nc, 12)
    n1s, n2 = ssum(n1t), ssum(n2t)
    n1 = np.zeros((nc, 6, 2, 6, 2), dtype=dtype)
    for i in range(2):
        n1[:, :, i, :, i] = n1s
    n12 = n1 + n2.transpose(0, 1, 3, 2, 4)
    return vec, n1.reshape(nc, 12, 12), n12.reshape(nc, 12, 12)


class Space(object):
    """the condensed space: which dof is inner row r, which the k-th Dirichlet
    value (`code`: r >= 0 or -(k+1), as the C API numbers them)"""

    def __init__(self, cell_vdofs, glam, area, vdim, invinds, dbcinds):
        self.vd = np.asarray(cell_vdofs).reshape(-1, 12).astype(np.int64)
        self.glam = np.asarray(glam, dtype=np.float64).reshape(-1, 3, 2)
        self.area = np.asarray(area, dtype=np.float64).reshape(-1)
        self.nc, self.vdim = self.area.size, int(vdim)
        self.inv = np.asarray(invinds, dtype=np.int64)
        self.dbc = np.asarray(dbcinds, dtype=np.int64)
        self.nv = self.inv.size
        code = np.full(self.vdim, np.iinfo(np.int64).min, dtype=np.int64)
        code[self.dbc] = -(np.arange(self.dbc.size) + 1)
        code[self.inv] = np.arange(self.nv)
        self.code = code[self.vd]                                  # (nc,12)
        assert self.code.min() > np.iinfo(np.int64).min
        self.row_len = np.bincount(self.code[self.code >= 0], minlength=self.nv)
        # Dirichlet pairs of a row: (row slot inner) x (column slot Dirichlet)
        ninn = (self.code >= 0).sum(axis=1)
        self.bc_len = np.bincount(
            self.code[self.code >= 0],
            weights=np.repeat(12 - ninn, 12).reshape(-1, 12)[self.code >= 0],
            minlength=self.nv).astype(np.int64)

    def local(self, v_inner, dbcvals):
        full = np.zeros(self.vdim)
        full[self.inv] = np.asarray(v_inner, dtype=np.float64).reshape(-1)
        if self.dbc.size:
            full[self.dbc] = np.asarray(dbcvals, dtype=np.float64).reshape(-1)
        return full[self.vd].reshape(self.nc, 6, 2)

    def pattern_keys(self, indptr, indices):
        rows = np.repeat(np.arange(self.nv), np.diff(indptr))
        keys = rows*np.int64(self.nv) + np.asarray(indices, dtype=np.int64)
        assert np.all(np.diff(keys) > 0), 'pattern rows must be sorted'
        return keys

    def gather_rows(self, cellvals, rng=None):
        """sum of the cell values `(nc,12)` over the slots of every inner row"""
        m = self.code >= 0
        r, v = self.code[m], cellvals[m]
        if rng is not None:
            p = rng.permutation(r.size)
            r, v = r[p], v[p]
        out = np.zeros(self.nv, dtype=cellvals.dtype)
        np.add.at(out, r, v)
        return out

    def gather_mat(self, L, keys, rng=None):
        """`(values in the pattern, contributions per non-zero)`"""
        rr = np.broadcast_to(self.code[:, :, None], L.shape)
        cc = np.broadcast_to(self.code[:, None, :], L.shape)
        m = (rr >= 0) & (cc >= 0)
        k = rr[m]*np.int64(self.nv) + cc[m]
        z = np.searchsorted(keys, k)
        assert np.all(keys[np.minimum(z, keys.size - 1)] == k), \
            'pattern lacks an entry'
        v = L[m]
        if rng is not None:
            p = rng.permutation(z.size)
            z, v = z[p], v[p]
        out = np.zeros(keys.size, dtype=L.dtype)
        np.add.at(out, z, v)
        return out, np.bincount(z, minlength=keys.size)

    def gather_bc(self, L, bcvals, rng=None):
        """`sum_k L[row, bc_k] bcvals_k` per inner row (rhsbc = minus this)"""
        out = np.zeros(self.nv, dtype=L.dtype)
        if not self.dbc.size:
            return out
        rr = np.broadcast_to(self.code[:, :, None], L.shape)
        cc = np.broadcast_to(self.code[:, None, :], L.shape)
        m = (rr >= 0) & (cc < 0)
        v = L[m]*np.asarray(bcvals).astype(L.dtype).reshape(-1)[-cc[m] - 1]
        r = rr[m]
        if rng is not None:
            p = rng.permutation(r.size)
            r, v = r[p], v[p]
        np.add.at(out, r, v)
        return out


def _both(fun):
    """value and magnitude twin of `fun(absval)`"""
    return fun(False), fun(True)


def conv_model(sp, v_inner, dbcvals, pattern=None, newton=False,
               dbcvals_rhs=None, dtype=LD, rng=None):
    """dict of `(value, bound)` pairs (bound: None for fp64 evaluations):
    `cells`, `n1`, `n12` per cell, `vec` = N(u)u[inner], and with `pattern
    (indptr, indices)`: `N` in the pattern, `rhsbc` with the values
    `dbcvals_rhs` (default: the field's own), `mat_len` contributions per
    non-zero"""
    ul = sp.local(v_inner, dbcvals)
    bcr = dbcvals if dbcvals_rhs is None else dbcvals_rhs
    cv, n1, n12 = cell_quantities(sp.glam, sp.area, ul, dtype, False, rng)
    out = dict(cells=cv, n1=n1, n12=n12, vec=sp.gather_rows(cv, rng))
    L = n12 if newton else n1
    if pattern is not None:
        keys = sp.pattern_keys(*pattern)
        out['N'], out['mat_len'] = sp.gather_mat(L, keys, rng)
        out['rhsbc'] = -sp.gather_bc(L, bcr, rng)
    if dtype is not LD:
        return out
    cva, n1a, n12a = cell_quantities(sp.glam, sp.area, ul, LD, True)
    La = n12a if newton else n1a
    res = dict(cells=(cv, gamma(K_VEC)*cva), n1=(n1, gamma(K_MAT)*n1a),
               n12=(n12, gamma(K_MAT)*n12a),
               vec=(out['vec'], gamma(K_VEC + sp.row_len)*sp.gather_rows(cva)),
               mag=dict(cells=cva, L=La))
    if pattern is not None:
        Na, ml = sp.gather_mat(La, keys)
        res['N'] = (out['N'], gamma(K_MAT + np.maximum(ml, 1) - 1)*Na)
        res['rhsbc'] = (out['rhsbc'], gamma(K_MAT + sp.bc_len) *
                        sp.gather_bc(La, np.abs(np.asarray(bcr, dtype=LD))))
        res['mat_len'] = ml
    return res


def csr_rows(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def _spmv(indptr, indices, vals, x, rng=None):
    r = csr_rows(indptr)
    t = vals*x[np.asarray(indices)]
    if rng is not None:
        p = rng.permutation(r.size)
        r, t = r[p], t[p]
    out = np.zeros(len(indptr) - 1, dtype=t.dtype)
    np.add.at(out, r, t)
    return out


def trap_assembly_model(sp, pattern, mvals, avals, J, hdt, v_lin, dbc_lin, v_c,
                        dbc_c, fv_n, fv_c, fp, x0, newton, dtype=LD, rng=None):
    """one trapezoidal step with `hdt = dt/2` about `v_lin` (Dirichlet values
    `dbc_lin`, the new time instance) from the current velocity `v_c` (its own
    `dbc_c`); `J` a SciPy CSR (np x nv); `x0 (nv + np)`.  dict of `(value,
    bound)` pairs (`dtype=LD`) or of values (fp64 evaluation): `N`, `F`,
    `rhsbc`, `fvn`, `b`, `r`, `rr` = ||r||^2, `bb` = ||b||^2"""
    indptr, indices = pattern
    nv, npr = sp.nv, J.shape[0]
    c = lambda x: np.asarray(x, dtype=np.float64).reshape(-1).astype(dtype)
    mv, av, fvn_, fvc_, fp_, x0_, vc_ = (c(x) for x in (mvals, avals, fv_n,
                                                        fv_c, fp, x0, v_c))
    hd = dtype(hdt)
    jp, ji, jd = J.indptr, J.indices, c(J.data)
    JT = J.T.tocsr()
    tp, ti, td = JT.indptr, JT.indices, c(JT.data)
    keys = sp.pattern_keys(indptr, indices)
    rows = csr_rows(indptr)

    def run(absval):
        a = np.abs if absval else (lambda x: x)
        ull = sp.local(v_lin, dbc_lin)
        ulc = sp.local(v_c, dbc_c)
        r_ = None if absval else rng
        cl, n1, n12 = cell_quantities(sp.glam, sp.area, ull, dtype, absval, r_)
        cc, _, _ = cell_quantities(sp.glam, sp.area, ulc, dtype, absval, r_)
        L = n12 if newton else n1
        N, ml = sp.gather_mat(L, keys, r_)
        g = dict(ml=ml, N=N)
        g['F_m'], g['F_a'], g['F_n'] = a(mv), hd*a(av), hd*N
        g['s'] = sp.gather_bc(L, a(c(dbc_lin)) if sp.dbc.size else None, r_)
        g['rc'] = sp.gather_rows(cl, r_) if newton else np.zeros(nv, dtype)
        g['cc'] = sp.gather_rows(cc, r_)
        g['mvc'] = _spmv(indptr, indices, a(mv), a(vc_), r_)
        g['avc'] = hd*_spmv(indptr, indices, a(av), a(vc_), r_)
        xv, xp = a(x0_[:nv]), a(x0_[nv:])
        g['mx'] = _spmv(indptr, indices, a(mv), xv, r_)
        g['ax'] = hd*_spmv(indptr, indices, a(av), xv, r_)
        g['nx'] = hd*_spmv(indptr, indices, N, xv, r_)
        g['jtx'] = _spmv(tp, ti, a(td), xp, r_) if npr else np.zeros(nv, dtype)
        g['jx'] = _spmv(jp, ji, a(jd), xv, r_)
        g['fvn'], g['fvc'], g['fp'] = a(fvn_), a(fvc_), a(fp_)
        return g
    v = run(False)
    val = dict(N=v['N'], F=mv + hd*(av + v['N']), rhsbc=-v['s'])
    val['fvn'] = v['fvn'] - v['s'] + v['rc']
    bv = v['mvc'] - v['avc'] + hd*(val['fvn'] + (v['fvc'] - v['cc']))
    val['b'] = np.concatenate([bv, v['fp']])
    kx = v['mx'] + v['ax'] + v['nx'] + v['jtx']
    val['r'] = np.concatenate([bv - kx, v['fp'] - v['jx']])
    val['rr'], val['bb'] = np.sum(val['r']**2), np.sum(val['b']**2)
    if dtype is not LD:
        return val
    m = run(True)
    ml = np.maximum(m['ml'], 1)
    lf, lj = np.diff(indptr), np.diff(tp)
    lg, lb = sp.row_len, sp.bc_len
    G = gamma
    e = dict(N=G(K_MAT + ml - 1)*m['N'])
    e['F'] = G(K_MAT + ml - 1 + 3)*m['F_n'] + G(3)*m['F_a'] + G(1)*m['F_m']
    k_s = K_MAT + lb
    k_rc = K_CLIN + lg - 1
    e['rhsbc'] = G(k_s)*m['s']
    e['fvn'] = G(2)*m['fvn'] + G(k_s + 2)*m['s'] + G(k_rc + 2)*m['rc']

    def bgroups(extra):
        return (G(2 + lf + 1 + extra)*(m['mvc'] + m['avc'])
                + hd*(G(2 + 3 + extra)*m['fvn'] + G(k_s + 5 + extra)*m['s']
                      + G(k_rc + 5 + extra)*m['rc']
                      + G(1 + 3 + extra)*m['fvc']
                      + G(K_VEC + lg - 1 + 4 + extra)*m['cc']))
    zero_p = np.zeros(npr, dtype=LD)
    e['b'] = np.concatenate([bgroups(0), zero_p])
    # the kernel takes N x0 as hdt * gather of L_cell x0_cell: magnitude
    # sum |L| |x0| per row = the twin product with the assembled twin of N
    xtra = lf + lj + 6
    er = bgroups(1) + G(1 + xtra + 1)*(m['mx'] + m['ax']) \
        + G(K_CX0 + lg - 1 + xtra + 1)*m['nx'] + G(xtra + 1)*m['jtx']
    erp = G(np.diff(jp) + 1)*m['jx'] + G(1)*m['fp']
    e['r'] = np.concatenate([er, erp])
    n = nv + npr
    for key, vec in (('rr', 'r'), ('bb', 'b')):
        e[key] = 2*np.sum(np.abs(val[vec])*e[vec]) + G(n + 2)*val[key]
    res = dict((k, (val[k], e[k])) for k in e)
    res['lens'] = dict(row=lf, jt=lj, cells=lg, bc=lb, mat=m['ml'],
                       j=np.diff(jp))
    return res


def ratio(got, value, bound):
    """largest |got - value| / bound; entries with bound 0 must be exact"""
    err = np.abs(np.asarray(got).reshape(-1).astype(LD)
                 - np.asarray(value).reshape(-1))
    bound = np.asarray(bound).reshape(-1)
    z = bound == 0
    if np.any(err[z] != 0):
        return np.inf
    if np.all(z):
        return 0.0
    return float(np.max(err[~z]/bound[~z]))
