"""POD-Galerkin reduced-order model of the semi-discrete Navier-Stokes system

    M v' + A v + N(v) v + J^T p = fv,   J v = fp,

on modes `phi_k` (r x NV, `SnapshotPOD`'s, `M`-orthonormal) about a mean flow
`vbar`: with `v = vbar + sum_k a_k phi_k` and the rows of `Phi` as test
functions

    Mr a' = -(Ar a + b0 + c + L a + H : a a),
    Mr = Phi M Phi^T,  Ar = Phi A Phi^T,  b0 = Phi (A vbar - fv),
    T[i, j, k] = int phi_i . (u_j . grad) u_k,   basis u = [modes; vbar],
    c = T[:, r, r],  L[i, k] = T[i, r, k] + T[i, k, r],  H = T[:, :r, :r].

The mean flow comes last in the basis (the layout of `SnapshotPOD.decompose` /
`split`) and carries the Dirichlet values; the modes vanish on the Dirichlet
dofs, and so do the test functions.  The pressure term `Phi J^T p` is dropped
(`div = max |J Phi^T|` says how much of it there is).

What is large runs on the device: the three linear projections through
`saddle.ensemble_project` (fp64 matrix cores, `X W Y^T`), the tensor through
`ConvectionP2.project_tensor`.  `device=False` is the fp64 NumPy statement of
the same thing from the operator's element data.  What is `r x r` -- `rhs`,
`integrate`, `lift` -- runs here.
"""
import numpy as np
import scipy.sparse as sps

from .. import convection as _conv

__all__ = ['GalerkinROM', 'tensor_host', 'bound_tensor', 'bound_project']

_U = 2.0**-53
ROM_MAX_BASIS = _conv.ROM_MAX_BASIS     # kRomMaxBasis (csrc/galerkin_host.hpp)
ROM_CELL_CHUNK = 512                    # kRomCellChunk
# Roundings a term  w_q |cell| phi_i,d u_j,e d_e u_k,d  of the tensor passes
# through in `k_rom_tensor`, counted from its operation chain (a fused
# multiply-add is one rounding):
#   test side   phi_i,d(x_q): six fma over the nodes 6, w_q |cell| 1, their
#               product 1                                                  8
#   field side  grad phi_n: a product and two fma 3, d_e u_k,d: six fma 6,
#               u_j,e(x_q) 6, the product and the fma over e 2            17
#   matrix core every product-accumulate counted as two roundings,
#               whatever the unit does inside: the product, and one beside
#               the additions counted below                                2
# K_TEN = 27, + the tables' T_TAB (one weight, two shape functions and one
# gradient: 2 + 2*10 + 11 units of u, measured by tests/conv_model.py), + 14
# ncells - 1 additions of a sum of 14 ncells terms in any order (zeros add
# nothing).
K_TEN = 27
T_TAB = 33


def _gamma(k):
    return k*_U/(1. - k*_U)


def _tables():
    """`(qw (7,), phi (7,6), dphi (7,6,3))` of the 7-point degree-5 rule and
    the P2 shape functions, by the closed forms the library uses"""
    s15 = np.sqrt(15.)
    t1, t2 = (6. - s15)/21., (6. + s15)/21.
    w1, w2 = (155. - s15)/1200., (155. + s15)/1200.
    qp = np.array([[1/3., 1/3., 1/3.],
                   [1 - 2*t1, t1, t1], [t1, 1 - 2*t1, t1], [t1, t1, 1 - 2*t1],
                   [1 - 2*t2, t2, t2], [t2, 1 - 2*t2, t2], [t2, t2, 1 - 2*t2]])
    qw = np.array([9/40., w1, w1, w1, w2, w2, w2])
    phi, dphi = np.zeros((7, 6)), np.zeros((7, 6, 3))
    for k, (i, j) in enumerate(((1, 2), (0, 2), (0, 1))):
        phi[:, k] = qp[:, k]*(2*qp[:, k] - 1)
        dphi[:, k, k] = 4*qp[:, k] - 1
        phi[:, 3 + k] = 4*qp[:, i]*qp[:, j]
        dphi[:, 3 + k, i] = 4*qp[:, j]
        dphi[:, 3 + k, j] = 4*qp[:, i]
    return qw, phi, dphi


def _local(conv, rows, dbc_rows):
    """`(nb, nc, 6, 2)`: the twelve local values of every row per cell"""
    rows = np.asarray(rows, dtype=np.float64)
    full = np.zeros((rows.shape[0], conv._vdim))
    full[:, conv._invinds] = rows[:, :conv.nv]
    if dbc_rows is not None and conv.ndbc:
        full[:, conv._dbcinds] = dbc_rows
    return full[:, conv._cell_vdofs].reshape(rows.shape[0], -1, 6, 2)


def tensor_host(conv, basis, dbc_rows=None, ntest=None, absval=False):
    """the tensor of `ConvectionP2.project_tensor` in fp64 NumPy from the
    operator's element data (`conv.glam`, `.area`, the cell dofs); `absval`:
    its magnitude twin, every factor replaced by its absolute value"""
    B, D, nt = _conv.check_basis(conv.nv, conv.ndbc, basis, dbc_rows, ntest)
    nb = B.shape[0]
    qw, phi, dphi = _tables()
    glam, area = np.asarray(conv.glam), np.asarray(conv.area)
    ul, tl = _local(conv, B, D), _local(conv, B[:nt], None)
    if absval:
        qw, phi, dphi, glam, area, ul, tl = (
            np.abs(x) for x in (qw, phi, dphi, glam, area, ul, tl))
    gphi = np.einsum('qnv,cve->cqne', dphi, glam)
    U = np.einsum('qn,bcne->bcqe', phi, ul)
    G = np.einsum('cqne,bcnd->bcqde', gphi, ul)             # d_e u_b,d
    w = qw[None, :]*area[:, None]
    P = np.einsum('cq,qn,icnd->icqd', w, phi, tl).reshape(nt, -1)
    T = np.empty((nt, nb, nb))
    for j in range(nb):
        Cj = np.einsum('cqe,kcqde->kcqd', U[j], G).reshape(nb, -1)
        T[:, j, :] = P @ Cj.T
    return T


def bound_tensor(conv, basis, dbc_rows=None, ntest=None):
    """`|T_computed - T| <= 1.01 gamma_K x (magnitude twin)`, `K = K_TEN +
    T_TAB + 14 ncells - 1`: for the device kernel and for `tensor_host`, any
    order of the sum over cells and points (`ntest x nb x nb`)"""
    K = K_TEN + T_TAB + 14*int(conv.ncells) - 1
    return 1.01*_gamma(K)*tensor_host(conv, basis, dbc_rows, ntest,
                                      absval=True)


def bound_project(X, Y=None, W=None):
    """`|P_computed - X W Y^T|_ij <= 1.01 (NV + maxrownnz(W) + 2) u sum_k
    |X_ik| (|W| |Y_j|)_k`, `u = 2^-53`: any summation order, with or without
    fma (`mx x my`) -- `pod.gram_bound` for two row sets"""
    X = np.abs(np.atleast_2d(np.asarray(X, dtype=np.float64)))
    Y = X if Y is None else np.abs(np.atleast_2d(np.asarray(Y,
                                                            dtype=np.float64)))
    nv = X.shape[1]
    if W is None:
        Wa, rownnz = sps.identity(nv, format='csr'), 1
    else:
        Wa = abs(sps.csr_matrix(W))
        rownnz = int(np.diff(Wa.indptr).max()) if nv else 0
    return 1.01*(nv + rownnz + 2)*_U*(X @ (Wa @ Y.T))


class GalerkinROM(object):
    """the condensed full-order operators `A` (NV x NV), `fv` (NV), the mass
    matrix `M` (None: the POD's weight matrix, which the loops hand over) and,
    for the divergence diagnostic, `J`"""

    def __init__(self, A, fv, M=None, J=None):
        self.A = sps.csr_matrix(A)
        self.NV = self.A.shape[0]
        if self.A.shape != (self.NV, self.NV):
            raise ValueError('`A` must be square, it is {0}'.format(
                self.A.shape))
        self.fv = np.asarray(fv, dtype=np.float64).reshape(-1)
        if self.fv.size != self.NV:
            raise ValueError('`fv` must have NV = {0} entries, it has '
                             '{1}'.format(self.NV, self.fv.size))
        self.M = None if M is None else sps.csr_matrix(M)
        self.J = None if J is None else sps.csr_matrix(J)
        for name, mat, shp in (('M', self.M, (self.NV, self.NV)),
                               ('J', self.J, (None, self.NV))):
            if mat is not None and (mat.shape[1] != shp[1] or (
                    shp[0] is not None and mat.shape[0] != shp[0])):
                raise ValueError('`{0}` does not fit NV = {1}: {2}'.format(
                    name, self.NV, mat.shape))
        self.ops = self.modes = self.mean = None

    bound_tensor = staticmethod(bound_tensor)
    bound_project = staticmethod(bound_project)

    # ---- the projection -------------------------------------------------------
    def basis(self, modes, mean, conv, dbcvals):
        """`(modes (r, NV), vbar (NV,), basis [modes; vbar], D)`, every shape
        checked by name: the mean comes last and carries `dbcvals`"""
        modes = np.atleast_2d(np.asarray(modes, dtype=np.float64))
        if modes.shape[1] != self.NV or conv.nv != self.NV:
            raise ValueError(
                '`modes` must be r x NV = r x {0} and the convection operator '
                'over the same inner dofs, they are {1} and {2}'.format(
                    self.NV, modes.shape, conv.nv))
        r = modes.shape[0]
        if r + 1 > ROM_MAX_BASIS:
            raise ValueError(
                'nb = r + 1 = {0} basis rows, the tensor kernel takes at most '
                '{1} (32 modes and a mean flow)'.format(r + 1, ROM_MAX_BASIS))
        if getattr(conv, 'dbc_table_rows', 0) > 0:
            raise ValueError(
                'the convection operator carries a time-varying Dirichlet '
                'table: constant boundary values only')
        vbar = np.zeros(self.NV) if mean is None else \
            np.asarray(mean, dtype=np.float64).reshape(-1)
        if vbar.size != self.NV:
            raise ValueError('`mean` must have NV = {0} entries, it has '
                             '{1}'.format(self.NV, vbar.size))
        dbv = np.zeros(0) if dbcvals is None else \
            np.asarray(dbcvals, dtype=np.float64).reshape(-1)
        if dbv.size != conv.ndbc:
            raise ValueError('`dbcvals` must have ndbc = {0} entries, it has '
                             '{1}'.format(conv.ndbc, dbv.size))
        D = np.zeros((r + 1, conv.ndbc))
        D[r] = dbv
        return modes, vbar, np.vstack([modes, vbar[None, :]]), D

    def _weights(self):
        if self.M is None:
            raise ValueError('no mass matrix: pass `M` (the loops hand over '
                             'the POD\'s weight matrix)')
        return self.M

    def project(self, modes, mean, conv, dbcvals, device=True):
        """the reduced operators as a dict `Mr`, `Ar` (r x r), `b0`, `c` (r),
        `L` (r x r), `H` (r x r x r) and, with `J`, `div`; kept in `self.ops`
        for `rhs` / `integrate` / `lift`"""
        modes, vbar, basis, D = self.basis(modes, mean, conv, dbcvals)
        M = self._weights()
        r = modes.shape[0]
        if device:
            from ..saddle import ensemble_project
            ld = -(-self.NV//2)*2
            pad = lambda X: np.ascontiguousarray(
                np.hstack([X, np.zeros((X.shape[0], ld - self.NV))]))
            Phi = pad(modes)
            Mr = ensemble_project(Phi, None, M, nv=self.NV)
            PA = ensemble_project(Phi, pad(basis), self.A, nv=self.NV)
            Pf = ensemble_project(Phi, pad(self.fv[None, :]), None,
                                  nv=self.NV)
            T = conv.project_tensor(basis, D, ntest=r)
        else:
            Mr = modes @ (M @ modes.T)
            PA = modes @ (self.A @ basis.T)
            Pf = modes @ self.fv[:, None]
            T = tensor_host(conv, basis, D, ntest=r)
        ops = dict(Mr=Mr, Ar=np.ascontiguousarray(PA[:, :r]),
                   b0=PA[:, r] - Pf[:, 0], c=T[:, r, r].copy(),
                   L=T[:, r, :r] + T[:, :r, r],
                   H=np.ascontiguousarray(T[:, :r, :r]))
        if self.J is not None:
            ops['div'] = float(np.abs(self.J @ modes.T).max()) if r else 0.
        self.ops, self.modes, self.mean = ops, modes, vbar
        return ops

    def bound_ops(self, modes, mean, conv, dbcvals):
        """a-priori bounds of `project`'s arrays against the exact reduced
        operators, the same keys: `bound_project` / `bound_tensor` of what each
        is made of, and one rounding for a sum of two of them"""
        modes, vbar, basis, D = self.basis(modes, mean, conv, dbcvals)
        r = modes.shape[0]
        BA = bound_project(modes, basis, self.A)
        Bf = bound_project(modes, self.fv[None, :], None)
        BT = bound_tensor(conv, basis, D, ntest=r)
        Ta = tensor_host(conv, basis, D, ntest=r, absval=True)
        mag_b0 = np.abs(modes) @ (abs(self.A) @ np.abs(vbar)) \
            + np.abs(modes) @ np.abs(self.fv)
        return dict(Mr=bound_project(modes, None, self._weights()),
                    Ar=BA[:, :r], b0=BA[:, r] + Bf[:, 0] + 1.01*_U*mag_b0,
                    c=BT[:, r, r], H=BT[:, :r, :r],
                    L=BT[:, r, :r] + BT[:, :r, r]
                    + 1.01*_U*(Ta[:, r, :r] + Ta[:, :r, r]))

    # ---- the model --------------------------------------------------------------
    def _need(self):
        if self.ops is None:
            raise ValueError('no reduced operators: call `project` first')
        return self.ops

    def nonlinear(self, a):
        """`c + L a + H : a a`"""
        o = self._need()
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        return o['c'] + o['L'] @ a + (o['H'] @ a) @ a

    def rhs(self, a):
        """`-(Ar a + b0 + c + L a + H : a a)`, the right-hand side of `Mr a' =
        rhs(a)`"""
        o = self._need()
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        return -(o['Ar'] @ a + o['b0'] + self.nonlinear(a))

    def integrate(self, a0, trange):
        """CNAB on `Mr a' = rhs(a)` over the uniform grid `trange`, dense: the
        linear part by the trapezoidal rule, `c + L a + H : a a` by
        Adams-Bashforth 2 behind a Heun start; `len(trange) x r`"""
        o = self._need()
        t = np.asarray(trange, dtype=np.float64)
        if t.size < 2 or not np.allclose(np.diff(t), t[1] - t[0], rtol=1e-10,
                                         atol=0.):
            raise ValueError('`trange` must be a uniform grid of at least two '
                             'points')
        dt = t[1] - t[0]
        Mr, Ar, b0 = o['Mr'], o['Ar'], o['b0']
        lhs, rmat = Mr + .5*dt*Ar, Mr - .5*dt*Ar
        a = np.asarray(a0, dtype=np.float64).reshape(-1)
        out = np.empty((t.size, a.size))
        out[0] = a
        n_c = self.nonlinear(a)
        pred = np.linalg.solve(lhs, rmat @ a - dt*(b0 + n_c))
        a_n = np.linalg.solve(
            lhs, rmat @ a - dt*(b0 + .5*(n_c + self.nonlinear(pred))))
        out[1] = a_n
        for k in range(2, t.size):
            n_o, n_c = n_c, self.nonlinear(a_n)
            a_n = np.linalg.solve(
                lhs, rmat @ a_n - dt*(b0 + 1.5*n_c - .5*n_o))
            out[k] = a_n
        return out

    def lift(self, a):
        """`mean + a^T modes`: `a` of length r gives NV entries, `a` r x n (a
        column per state, as `coeffs`) gives n x NV"""
        self._need()
        return np.asarray(a, dtype=np.float64).T @ self.modes + self.mean
