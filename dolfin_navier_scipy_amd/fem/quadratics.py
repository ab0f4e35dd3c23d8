"""Quadratic functionals of a Taylor-Hood velocity -- the energy budget:
kinetic energy `1/2 u^T M u`, dissipation rate `u^T A u` (`nu/2 int |grad u +
grad u^T|^2` for the symmetric-gradient `A` of `TaylorHood.stokes_mats`), the
rate `u^T M du/dt` and the M-norm of `du/dt` (the steady-state criterion and
the blow-up indicator of a run).

Over `nM` sparse matrices `Q_0 .. Q_{nM-1}` on the inner velocity dofs
(`NV x NV`, general: not assumed symmetric) stand `nQ` forms.  With the inner
velocity `v`, the one before it `v_prev`, `w = v - v_prev` and the operands
`a_0 = v`, `a_1 = w`

    y_k = scale_k * ( dt^-(l_k + r_k) * a_{l_k}^T Q_{m_k} a_{r_k}
                      + qa_k . v + (qw_k . w)/dt + c0_k )

-- the form `ImexStepper.set_quadratics` evaluates on the device after every
step of a resident loop (`dns_imex_set_quadratics`, `csrc/quadratic.hpp`).
`evaluate` is the NumPy statement of the same sum.  The sparse rows `qa`, `qw`
and `c0` carry constant Dirichlet values `g`: with `u = E v + g` on the full
space

    u^T Q u = v^T Q_ii v + (g^T (Q_bi + Q_ib^T)) v + g^T Q_bb g

and the difference of two states has no boundary part.  Forms that share a
matrix (the same object) share it on the device: `1/2 v^T M v`, `v^T M w` and
`w^T M w` read `M` once per step.

Moving Dirichlet values (`ndbc > 0`): the forms stand on the full space.  Every
matrix is `(NV + ndbc) x (NV + ndbc)` in the order `[inner dofs; Dirichlet
dofs]` -- the Dirichlet dofs in the loop's order, `static_dbcvals` then the
controlled ones, the convention of `MomentumFunctionals.cab` --, the rows
`qa`, `qw` are `nQ x (NV + ndbc)`, and the operands are `a_0 = u = [v; g]`,
`a_1 = d = [v - v_prev; g - g_prev]` with the Dirichlet values `g`, `g_prev` of
the two states: nothing of `g` is folded into constants (the builders'
`moving=True`; `ImexStepper.set_quadratics(..., dbc_table=)`,
`dns_imex_set_quadratics_bc`).
"""
import weakref

import numpy as np
import scipy.sparse as sps

__all__ = ['QuadraticFunctionals', 'kinetic_energy', 'dissipation',
           'kinetic_energy_rate', 'rate_norm', 'energy_budget']


def _canonical(mat, shape, what):
    mat = sps.csr_matrix(mat)
    if mat.shape != shape:
        raise ValueError('{0} must be {1} x {2}, it is {3}'.format(
            what, shape[0], shape[1], mat.shape))
    if not mat.has_canonical_format:
        mat = mat.copy()
        mat.sum_duplicates()
    return mat


class QuadraticFunctionals(object):
    """`nQ` forms over `nM` matrices; made by `from_matrices` or the builders
    of this module, stacked with `+` (instances of one problem; a matrix that
    is the same object in both is kept once), `scaled(factors)` multiplies the
    scales.  The device takes at most 8 forms over at most 4 matrices."""

    def __init__(self, NV, ndbc=0):
        self.NV = int(NV)
        self.ndbc = int(ndbc)
        if self.ndbc < 0:
            raise ValueError('`ndbc` must not be negative')
        self.mats = []
        self.mat = np.zeros(0, dtype=np.int32)
        self.lop = np.zeros(0, dtype=np.int32)
        self.rop = np.zeros(0, dtype=np.int32)
        self.qa = sps.csr_matrix((0, self.N))
        self.qw = sps.csr_matrix((0, self.N))
        self.c0, self.scale = np.zeros(0), np.zeros(0)
        self.names = []

    @classmethod
    def from_matrices(cls, NV, mats, forms, qa=None, qw=None, c0=None,
                      scale=None, names=None, ndbc=0):
        """`mats`: the matrices (`NV x NV`), `forms`: a list of `(mat, lop,
        rop)` -- index into `mats`, left and right operand (0: `v`, 1:
        `v - v_prev`); `qa`, `qw`: `nQ x NV` sparse rows (None: no such
        term), `c0`, `scale`: `nQ` values (None: 0 / 1).  With `ndbc > 0`
        (moving Dirichlet values) matrices and rows are `NV + ndbc` wide,
        `[inner dofs; Dirichlet dofs]`"""
        new = cls(NV, ndbc)
        NV = new.N      # (the width of every matrix and row)
        mats = list(mats)
        forms = [tuple(int(i) for i in f) for f in forms]
        nQ = len(forms)
        if not mats or not forms:
            raise ValueError('at least one matrix and one form')
        new.mats = [_canonical(m, (NV, NV), 'matrix {0}'.format(k))
                    if not (sps.isspmatrix_csr(m) and m.shape == (NV, NV)
                            and m.has_canonical_format) else m
                    for k, m in enumerate(mats)]
        for k, f in enumerate(forms):
            if len(f) != 3:
                raise ValueError('form {0}: (mat, lop, rop) expected'.format(k))
            if not 0 <= f[0] < len(mats):
                raise ValueError('form {0}: matrix {1} outside 0..{2}'.format(
                    k, f[0], len(mats) - 1))
            if f[1] not in (0, 1) or f[2] not in (0, 1):
                raise ValueError('form {0}: operands are 0 (v) or 1 '
                                 '(v - v_prev)'.format(k))
        new.mat, new.lop, new.rop = (
            np.array([f[i] for f in forms], dtype=np.int32) for i in range(3))
        new.qa = _canonical((nQ, NV) if qa is None else qa, (nQ, NV), 'qa')
        new.qw = _canonical((nQ, NV) if qw is None else qw, (nQ, NV), 'qw')
        new.c0 = np.zeros(nQ) if c0 is None else \
            np.array(c0, dtype=np.float64).reshape(nQ)
        new.scale = np.ones(nQ) if scale is None else \
            np.array(scale, dtype=np.float64).reshape(nQ)
        new.names = list(names) if names is not None else \
            ['q{0}'.format(k) for k in range(nQ)]
        if len(new.names) != nQ:
            raise ValueError('`names` must have one entry per form')
        return new

    @property
    def N(self):
        """the width of the matrices and rows: `NV + ndbc`"""
        return self.NV + self.ndbc

    @property
    def nQ(self):
        return self.scale.size

    @property
    def nM(self):
        return len(self.mats)

    def __add__(self, other):
        if other.NV != self.NV:
            raise ValueError('quadratics of different problems')
        if other.ndbc != self.ndbc:
            raise ValueError(
                'quadratics of different `ndbc` ({0} and {1}): forms with '
                'constant and with moving Dirichlet values do not '
                'stack'.format(self.ndbc, other.ndbc))
        mats = list(self.mats)
        where = []
        for m in other.mats:
            hit = [k for k, mine in enumerate(mats) if mine is m]
            if hit:
                where.append(hit[0])
            else:
                where.append(len(mats))
                mats.append(m)
        new = QuadraticFunctionals(self.NV, self.ndbc)
        new.mats = mats
        new.mat = np.concatenate(
            [self.mat, np.array(where, dtype=np.int32)[other.mat]]
        ).astype(np.int32)
        new.lop = np.concatenate([self.lop, other.lop]).astype(np.int32)
        new.rop = np.concatenate([self.rop, other.rop]).astype(np.int32)
        new.qa = sps.vstack([self.qa, other.qa]).tocsr()
        new.qw = sps.vstack([self.qw, other.qw]).tocsr()
        new.c0 = np.concatenate([self.c0, other.c0])
        new.scale = np.concatenate([self.scale, other.scale])
        new.names = list(self.names) + list(other.names)
        return new

    def scaled(self, factors):
        """a copy whose scales are multiplied by `factors` (a number or one
        per form); the matrices are shared"""
        new = QuadraticFunctionals(self.NV, self.ndbc)
        new.mats = self.mats
        new.mat, new.lop, new.rop = self.mat, self.lop, self.rop
        new.qa, new.qw, new.c0 = self.qa, self.qw, self.c0
        new.names = list(self.names)
        new.scale = self.scale*np.asarray(factors, dtype=np.float64)
        if new.scale.shape != self.scale.shape:
            raise ValueError('`factors`: a number or one per form')
        return new

    # -- what the device is handed ---------------------------------------
    def device_args(self):
        """`dict(mats, mat, lop, rop, qa, qw, c0, scale)` in the layout of
        `dns_imex_set_quadratics`: the list of CSR matrices, three int32
        arrays of `nQ` entries, the sparse rows `nQ x NV` and two float64
        arrays of `nQ` entries.  With moving Dirichlet values also `ndbc`
        (> 0), the number of Dirichlet dofs behind the inner ones: matrices
        and rows are `NV + ndbc` wide (`dns_imex_set_quadratics_bc`)"""
        args = self._device_args()
        if self.ndbc > 0:
            args['ndbc'] = self.ndbc
        return args

    def _device_args(self):
        return dict(mats=list(self.mats),
                    mat=np.ascontiguousarray(self.mat, dtype=np.int32),
                    lop=np.ascontiguousarray(self.lop, dtype=np.int32),
                    rop=np.ascontiguousarray(self.rop, dtype=np.int32),
                    qa=self.qa, qw=self.qw,
                    c0=np.ascontiguousarray(self.c0, dtype=np.float64),
                    scale=np.ascontiguousarray(self.scale, dtype=np.float64))

    # -- the NumPy statement ----------------------------------------------
    def evaluate(self, v, v_prev, dt, return_scale=False, dbc=None,
                 dbc_prev=None):
        """`y (nQ,)` for inner velocities `v`, `v_prev` (`ndbc > 0`: and the
        Dirichlet values `dbc`, `dbc_prev` of the two states, which the
        operands go on with -- the boundary products count in `T_k`, `n_k`
        like any other); with `return_scale`
        also `T_k`, the sum of the absolute values of every product of form
        k as it enters `y_k` (the matrix entries `|a_i Q_ij b_j|`, the rows'
        `|qa_j v_j|`, `|qw_j w_j|` and `|c0_k|`, with the powers of `dt` and
        `|scale_k|`; summed in `np.longdouble`), and `n_k`, their number:
        rounding in fp64 moves a sum of `n_k` products, in whatever order, by
        at most `n_k 2^-52 T_k`"""
        NV = self.NV
        v = np.asarray(v, dtype=np.float64).reshape(-1)[:NV]
        w = v - np.asarray(v_prev, dtype=np.float64).reshape(-1)[:NV]
        if self.ndbc > 0:
            if dbc is None or dbc_prev is None:
                raise ValueError(
                    'quadratics with moving Dirichlet values (ndbc = {0}) '
                    'need `dbc` and `dbc_prev`'.format(self.ndbc))
            g, gp = (np.asarray(x, dtype=np.float64).reshape(-1)
                     for x in (dbc, dbc_prev))
            if g.size != self.ndbc or gp.size != self.ndbc:
                raise ValueError(
                    '`dbc`, `dbc_prev`: {0} and {1} values, the forms were '
                    'built for {2}'.format(g.size, gp.size, self.ndbc))
            v, w = np.concatenate([v, g]), np.concatenate([w, g - gp])
            NV = self.N
        ops = (v, w)
        prod = {}
        y = np.zeros(self.nQ)
        for k in range(self.nQ):
            m, lo, ro = int(self.mat[k]), int(self.lop[k]), int(self.rop[k])
            if (m, ro) not in prod:
                prod[(m, ro)] = self.mats[m] @ ops[ro]
            q = float(ops[lo] @ prod[(m, ro)])
            for _ in range(lo + ro):
                q = q/dt
            lin = float(self.qa[k].toarray().reshape(-1) @ v) \
                + float(self.qw[k].toarray().reshape(-1) @ w)/dt
            y[k] = self.scale[k]*(q + lin + self.c0[k])
        if not return_scale:
            return y
        ld = np.longdouble
        absops = (np.abs(v).astype(ld), np.abs(w).astype(ld))
        T, n = np.zeros(self.nQ), np.zeros(self.nQ, dtype=np.int64)
        aprod = {}
        for k in range(self.nQ):
            m, lo, ro = int(self.mat[k]), int(self.lop[k]), int(self.rop[k])
            mat = self.mats[m]
            if (m, ro) not in aprod:
                rows = np.repeat(np.arange(NV), np.diff(mat.indptr))
                terms = np.abs(mat.data).astype(ld)*absops[ro][mat.indices]
                aprod[(m, ro)] = (rows, terms)
            rows, terms = aprod[(m, ro)]
            t = (terms*absops[lo][rows]).sum(dtype=ld)/ld(dt)**(lo + ro)
            qa, qw = self.qa[k], self.qw[k]
            t += (np.abs(qa.data).astype(ld)*absops[0][qa.indices]).sum(
                dtype=ld)
            t += (np.abs(qw.data).astype(ld)*absops[1][qw.indices]).sum(
                dtype=ld)/ld(dt)
            t += ld(abs(self.c0[k]))
            T[k] = float(ld(abs(self.scale[k]))*t)
            n[k] = mat.nnz + qa.nnz + qw.nnz + 1
        return y, T, n


# -- builders on the full-space matrices of a Taylor-Hood problem ------------

def _inner_blocks(Q, femp):
    """`(Q_ii, g^T Q_bi, Q_ib g, g^T Q_bb g)` of a full-space matrix"""
    inv = np.asarray(femp['invinds'], dtype=np.int64)
    dbi = np.asarray(femp['dbcinds'], dtype=np.int64)
    g = np.asarray(femp['dbcvals'], dtype=np.float64).reshape(-1)
    Q = sps.csr_matrix(Q)
    Qii = sps.csr_matrix(Q[inv, :][:, inv])
    Qii.sum_duplicates()
    Qii.sort_indices()
    left = np.asarray(Q[dbi, :][:, inv].T @ g).reshape(-1)
    right = np.asarray(Q[inv, :][:, dbi] @ g).reshape(-1)
    return Qii, left, right, float(g @ (Q[dbi, :][:, dbi] @ g))


_blocks = weakref.WeakKeyDictionary()


def _problem_mats(th, femp):
    """the inner blocks of `M` and `A` of a problem, built once per space,
    viscosity and Dirichlet data (the builders share them: the same objects
    stack to ONE matrix each)"""
    key = (float(femp['nu']),
           np.asarray(femp['invinds'], dtype=np.int64).tobytes(),
           np.asarray(femp['dbcinds'], dtype=np.int64).tobytes(),
           np.asarray(femp['dbcvals'], dtype=np.float64).tobytes())
    cache = _blocks.setdefault(th, {})
    if key not in cache:
        stms = th.stokes_mats(nu=femp['nu'])
        cache[key] = dict(M=_inner_blocks(stms['M'], femp),
                          A=_inner_blocks(stms['A'], femp))
    return cache[key]


def _full_mats(th, femp):
    """`M` and `A` of a problem on `[inner dofs; Dirichlet dofs]`, the
    Dirichlet dofs in the order of `femp['dbcinds']`: `Q[perm][:, perm]` with
    `perm = invinds ++ dbcinds`, built once per space, viscosity and index
    sets (the moving builders share them: the same objects stack to ONE matrix
    each)"""
    inv = np.asarray(femp['invinds'], dtype=np.int64)
    dbi = np.asarray(femp['dbcinds'], dtype=np.int64)
    key = ('full', float(femp['nu']), inv.tobytes(), dbi.tobytes())
    cache = _blocks.setdefault(th, {})
    if key not in cache:
        stms = th.stokes_mats(nu=femp['nu'])
        perm = np.concatenate([inv, dbi])

        def full(Q):
            Q = sps.csr_matrix(sps.csr_matrix(Q)[perm, :][:, perm])
            Q.sum_duplicates()
            Q.sort_indices()
            return Q
        cache[key] = dict(M=full(stms['M']), A=full(stms['A']), NV=inv.size,
                          ndbc=dbi.size)
    return cache[key]


def _moving(th, femp, which, form, name, scale=None):
    blk = _full_mats(th, femp)
    return QuadraticFunctionals.from_matrices(
        blk['NV'], [blk[which]], [form], scale=scale, names=[name],
        ndbc=blk['ndbc'])


def _row(vec):
    return sps.csr_matrix(np.asarray(vec, dtype=np.float64).reshape((1, -1)))


def kinetic_energy(th, femp, name='ekin', moving=False):
    """`1/2 u^T M u` of the full velocity `u` (Dirichlet values included);
    `moving`: on the full space, the Dirichlet values come with the state"""
    if moving:
        return _moving(th, femp, 'M', (0, 0, 0), name, scale=[.5])
    Mii, left, right, const = _problem_mats(th, femp)['M']
    return QuadraticFunctionals.from_matrices(
        Mii.shape[0], [Mii], [(0, 0, 0)], qa=_row(left + right), c0=[const],
        scale=[.5], names=[name])


def dissipation(th, femp, name='dissipation', moving=False):
    """`u^T A u`: `nu/2 int |grad u + grad u^T|^2` with the symmetric-gradient
    `A` of `TaylorHood.stokes_mats`; `moving`: on the full space"""
    if moving:
        return _moving(th, femp, 'A', (0, 0, 0), name)
    Aii, left, right, const = _problem_mats(th, femp)['A']
    return QuadraticFunctionals.from_matrices(
        Aii.shape[0], [Aii], [(0, 0, 0)], qa=_row(left + right), c0=[const],
        names=[name])


def kinetic_energy_rate(th, femp, name='ekin_rate', moving=False):
    """`u^T M (u - u_prev)/dt`; where the boundary values do not move `u -
    u_prev` lives on the inner dofs: `(v^T M_ii w + g^T M_bi w)/dt`; `moving`:
    on the full space, `u - u_prev` includes `g - g_prev`"""
    if moving:
        return _moving(th, femp, 'M', (0, 0, 1), name)
    Mii, left, _, _ = _problem_mats(th, femp)['M']
    return QuadraticFunctionals.from_matrices(
        Mii.shape[0], [Mii], [(0, 0, 1)], qw=_row(left), names=[name])


def rate_norm(th, femp, name='rate_norm', moving=False):
    """`d^T M d` with `d = (u - u_prev)/dt`: the squared M-norm of the
    discrete time derivative; `moving`: `d` includes `(g - g_prev)/dt`"""
    if moving:
        return _moving(th, femp, 'M', (0, 1, 1), name)
    Mii = _problem_mats(th, femp)['M'][0]
    return QuadraticFunctionals.from_matrices(
        Mii.shape[0], [Mii], [(0, 1, 1)], names=[name])


def energy_budget(th, femp, moving=False):
    """the four together: `ekin`, `dissipation`, `ekin_rate`, `rate_norm`
    over two matrices; `moving`: with moving Dirichlet values (`ndbc =
    len(femp['dbcinds'])`)"""
    return kinetic_energy(th, femp, moving=moving) \
        + dissipation(th, femp, moving=moving) \
        + kinetic_energy_rate(th, femp, moving=moving) \
        + rate_norm(th, femp, moving=moving)
