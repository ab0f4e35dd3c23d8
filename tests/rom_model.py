"""A NumPy `longdouble` model of the convection tensor of a Galerkin projection,
written from the formula

    T[i, j, k] = sum_cells sum_q w_q |cell| sum_d phi_i,d(x_q)
                 sum_e u_j,e(x_q) d_e u_k,d(x_q),

`u_b` row `b` of the basis on the inner dofs and row `b` of `D` on the Dirichlet
dofs, `phi_i` row `i < nt` on the inner dofs and zero on the Dirichlet dofs; the
7-point rule and the P2 shape functions from `conv_model.tables` in long double.
The fp64 inputs are the exact data of the model.  `j` convects, `k` is
convected.

It has a MAGNITUDE TWIN (`absval=True`): the same sum with every factor replaced
by its absolute value.  The bound of an entry is `gamma_K` times its twin,

    K = K_TEN + T_TAB + 14 ncells - 1,

`K_TEN = 27` counted from the operation chain of `k_rom_tensor` in
`fem/rom.py` (test side 8, field side 17, every product-accumulate of the
matrix core 2), `T_TAB` the tables' distance from the long double ones
(`conv_model`), and `14 ncells - 1` additions for a sum of that many terms in
any order.

Margins measured on the CPU (tests/test_rom_cpu.py prints them with `pytest
-s`), largest error / bound:
  `fem.rom.tensor_host` (fp64 einsum) against this model, toy wake, fan and
  rectangle(33) with the three Dirichlet splits:              0.0020
     (fan, boundary split, no Dirichlet rows; toy wake 8.5e-5: the bound
     grows with 14 ncells, the error of a sum of mixed signs does not)
  the host assembler `TaylorHood.convection_vec(u_k, utwo=u_j)` against
  `tensor_host` (toy wake, sum of both bounds): 3.3e-5; the contraction
  against `convection_vec(u)`: 2.4e-6
  `rhs(a)` against the full operators in long double, contracted bounds:
  seeded `a` 2.1e-5, the `coeffs` columns of a toy-wake POD 1.4e-4
"""
import numpy as np

import conv_model
import imex_host_model

LD = np.longdouble
K_TEN = 27


def k_total(ncells):
    return K_TEN + conv_model.T_TAB + 14*int(ncells) - 1


def _locals(sp, rows, dbc_rows):
    nd = sp.dbc.size
    return np.stack([
        sp.local(r[:sp.nv], np.zeros(nd) if dbc_rows is None else dbc_rows[b])
        for b, r in enumerate(rows)])


def tensor_longdouble(sp, basis, dbc_rows=None, ntest=None, absval=False):
    """`sp` a `conv_model.Space`; `(nt, nb, nb)` in long double"""
    B = np.asarray(basis, dtype=np.float64)
    nb = B.shape[0]
    nt = nb if ntest is None else int(ntest)
    qw, phi, dphi = conv_model.tables(LD)
    glam, area = sp.glam.astype(LD), sp.area.astype(LD)
    ul = _locals(sp, B, dbc_rows).astype(LD)               # (nb, nc, 6, 2)
    tl = _locals(sp, B[:nt], None).astype(LD)
    if absval:
        qw, phi, dphi, glam, area, ul, tl = (
            np.abs(x) for x in (qw, phi, dphi, glam, area, ul, tl))
    T = np.zeros((nt, nb, nb), dtype=LD)
    for q in range(7):
        gphi = sum(dphi[q][None, :, v, None]*glam[:, None, v, :]
                   for v in range(3))                       # (nc, 6, 2): n, e
        U = sum(phi[q, n]*ul[:, :, n, :] for n in range(6))        # b, c, e
        G = sum(gphi[None, :, n, None, :]*ul[:, :, n, :, None]
                for n in range(6))                          # b, c, d, e
        Pq = (qw[q]*area)[None, :, None] * \
            sum(phi[q, n]*tl[:, :, n, :] for n in range(6))        # i, c, d
        for j in range(nb):
            # ((u_j . grad) u_k)_d = sum_e u_j,e d_e u_k,d
            Cj = G[:, :, :, 0]*U[j][None, :, 0, None] \
                + G[:, :, :, 1]*U[j][None, :, 1, None]      # k, c, d
            T[:, j, :] += Pq.reshape(nt, -1) @ Cj.reshape(nb, -1).T
    return T


def bound_longdouble(sp, basis, dbc_rows=None, ntest=None):
    return conv_model.gamma(k_total(sp.nc)) * \
        tensor_longdouble(sp, basis, dbc_rows, ntest, absval=True)


def seeded_basis(nb, nv, ndbc, seed):
    """`(B (nb, nv), D (nb, ndbc))`, every row of both non-zero"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nb, nv)),
            rng.standard_normal((nb, ndbc)) + 0.25)


class HostConv(object):
    """the element data of a `convection.ConvectionP2` without the device:
    what `fem.rom.tensor_host` and `GalerkinROM.project(device=False)` read"""

    def __init__(self, cell_vdofs, glam, area, vdim, invinds, dbcinds,
                 dbcvals=None):
        self._cell_vdofs = np.asarray(cell_vdofs).reshape(-1, 12)
        self.glam = np.asarray(glam, dtype=np.float64).reshape(-1, 3, 2)
        self.area = np.asarray(area, dtype=np.float64).reshape(-1)
        self.ncells, self._vdim = self.area.size, int(vdim)
        self._invinds, self._dbcinds = np.asarray(invinds), np.asarray(dbcinds)
        self.nv, self.ndbc = self._invinds.size, self._dbcinds.size
        self.dbcvals = None if dbcvals is None else np.asarray(dbcvals)
        self.dbc_table_rows = 0

    @classmethod
    def from_mesh(cls, mesh, invinds, dbcinds, dbcvals=None):
        return cls(mesh.cell_vdofs, mesh.glam, mesh.area, mesh.vdim, invinds,
                   dbcinds, dbcvals)

    @classmethod
    def from_taylor_hood(cls, th, invinds, dbcinds, dbcvals=None):
        return cls(th._vdofs(), th.glam, th.area, th.vdim, invinds, dbcinds,
                   dbcvals)

    def space(self):
        return conv_model.Space(self._cell_vdofs, self.glam, self.area,
                                self._vdim, self._invinds, self._dbcinds)


class StubRomConvection(imex_host_model.StubConvection, HostConv):
    """`StubConvection` of the host loop with the element data beside it"""

    def __init__(self, f_vdp, appndbcs, th, invinds, dbcinds, dbcvals):
        imex_host_model.StubConvection.__init__(self, f_vdp, appndbcs)
        HostConv.__init__(self, th._vdofs(), th.glam, th.area, th.vdim,
                          invinds, dbcinds, dbcvals)
