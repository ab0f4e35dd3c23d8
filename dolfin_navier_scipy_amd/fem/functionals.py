"""Momentum-balance functionals of a Taylor-Hood state: consistent nodal
forces (drag, lift, torque), pressure differences, patch averages.

For a test vector `phi` on the full velocity space the consistent force is

    F = -phi^T (M dv/dt + A v + N(v) v - J^T p)

with the un-condensed operators and `v` carrying its Dirichlet values: only
the dofs where `phi` is non-zero and the cells around them contribute.  In
the inner dofs `v`, the state before it `v_prev` and the pressure `p` this is

    y_k = scale_k * ( ca_k . v + cm_k . (v - v_prev)/dt + cp_k . p
                      + sum_{c in cells_k} sum_{sl<12} w_k[c][sl] N_loc(c; v)[sl]
                      + c0_k )

(`dv/dt` by the backward difference, constant Dirichlet values: they drop out
of the `M` term and enter `A` through `c0` and `N` through the cells) -- the
form `ImexStepper.set_functionals` evaluates on the device after every step
of a resident loop (`dns_imex_set_functionals`).  `evaluate` is the NumPy
statement of the same sum.

With Dirichlet values `g` that change from step to step (controlled
boundaries: a rotating body, a modulated inflow; `g` in the order of
`femp['dbcinds']`) they stay where they are in the balance:

    y_k = scale_k * ( ca_k . v + cm_k . (v - v_prev)/dt + cp_k . p
                      + cab_k . g + cmb_k . (g - g_prev)/dt
                      + sum_{c in cells_k} sum_{sl<12} w_k[c][sl] N_loc(c; v, g)[sl]
                      + c0b_k )

with `cab`, `cmb` the Dirichlet columns of `phi^T A`, `phi^T M` and `c0b` the
constants that are no boundary terms (zero for test vectors, the caller's for
`from_rows`) -- `evaluate(..., dbc=g, dbc_prev=g_prev)`, on the device
`set_functionals(..., dbc_table=)` (`dns_imex_set_functionals_bc`).  With
constant `g` it is the first form: `cab . g` is its `c0`, the `cmb` term zero.
"""
import numpy as np
import scipy.sparse as sps

from . import taylor_hood as thm

__all__ = ['MomentumFunctionals', 'boundary_forces', 'boundary_torque',
           'pressure_difference', 'cylinder_nodes']


class MomentumFunctionals(object):
    """`phis`: `(vdim, nF)` test vectors on the full velocity space (dense or
    sparse), `femp`: the problem dict of `get_sysmats` (`invinds`, `dbcinds`,
    `dbcvals`, `nu`).  Each column gives one functional with `scale = -1`
    (the force ON the body where `phi = 1` on its dofs).  Instances of one
    problem are stacked with `+`; `scaled(factors)` multiplies the scales
    (force coefficients)."""

    def __init__(self, th, femp=None, phis=None, names=None):
        self.th = th
        if femp is None:
            # (pressure-only rows: the velocity space is taken over from the
            # instance they are stacked with)
            if phis is not None:
                raise ValueError('test vectors need the problem dict `femp`')
            self.inv, self.bcs, self.NV = None, None, 0
            self.dbi = None
        else:
            self.inv = np.asarray(femp['invinds'])
            self.bcs = np.zeros(th.vdim)
            self.bcs[np.asarray(femp['dbcinds'], dtype=np.int64)] = \
                np.asarray(femp['dbcvals'], dtype=np.float64).reshape(-1)
            self.NV = self.inv.size
            # (the Dirichlet dofs, in the order their values come in)
            self.dbi = np.asarray(femp['dbcinds'], dtype=np.int64)
        self.NP = th.pdim
        self.ndbc = 0 if self.dbi is None else self.dbi.size
        self.ca = sps.csr_matrix((0, self.NV))
        self.cm = sps.csr_matrix((0, self.NV))
        self.cp = sps.csr_matrix((0, self.NP))
        self.cab = sps.csr_matrix((0, self.ndbc))
        self.cmb = sps.csr_matrix((0, self.ndbc))
        self.c0, self.scale = np.zeros(0), np.zeros(0)
        self.c0b = np.zeros(0)
        self.cells, self.weights, self.names = [], [], []
        if phis is None:
            return
        phis = sps.csc_matrix(phis)
        if phis.shape[0] != th.vdim:
            raise ValueError('`phis` must have vdim = {0} rows'.format(th.vdim))
        nF = phis.shape[1]
        stms = th.stokes_mats(nu=femp['nu'])
        arows = sps.csr_matrix((stms['A'].T @ phis).T)            # nF x vdim
        mrows = sps.csr_matrix((stms['M'].T @ phis).T)
        jrows = sps.csr_matrix((stms['J'] @ phis).T)              # nF x pdim
        self.ca = sps.csr_matrix(arows[:, self.inv])
        self.cm = sps.csr_matrix(mrows[:, self.inv])
        self.cp = sps.csr_matrix(-jrows)
        self.cab = sps.csr_matrix(arows[:, self.dbi])
        self.cmb = sps.csr_matrix(mrows[:, self.dbi])
        self.c0 = np.asarray(arows @ self.bcs).reshape(-1)
        self.c0b = np.zeros(nF)
        self.scale = -np.ones(nF)
        vd = th._vdofs().reshape((-1, 12))        # slot = 2*node + component
        for k in range(nF):
            phi = np.asarray(phis[:, k].todense()).reshape(-1)
            wloc = phi[vd]                                        # (nc, 12)
            cells = np.where((wloc != 0.).any(axis=1))[0]
            self.cells.append(cells.astype(np.int32))
            self.weights.append(np.ascontiguousarray(wloc[cells]))
        self.names = list(names) if names is not None else \
            ['f{0}'.format(k) for k in range(nF)]
        if len(self.names) != nF:
            raise ValueError('`names` must have one entry per functional')
        self._tidy()

    def _tidy(self):
        for name in ('ca', 'cm', 'cp', 'cab', 'cmb'):
            mat = sps.csr_matrix(getattr(self, name))
            mat.sum_duplicates()
            mat.sort_indices()
            setattr(self, name, mat)

    @property
    def nF(self):
        return self.scale.size

    def _empty_like(self):
        new = MomentumFunctionals.__new__(MomentumFunctionals)
        new.th, new.inv, new.bcs = self.th, self.inv, self.bcs
        new.NV, new.NP = self.NV, self.NP
        new.dbi, new.ndbc = self.dbi, self.ndbc
        return new

    @classmethod
    def from_rows(cls, th, femp=None, ca=None, cm=None, cp=None, c0=None,
                  scale=None, names=None):
        """functionals without cells, given by their sparse rows (`nF x NV`,
        `nF x NV`, `nF x NP`; None: no such term); without `femp` only
        pressure rows"""
        new = cls(th, femp)
        if femp is None and (ca is not None or cm is not None):
            raise ValueError('velocity rows need the problem dict `femp`')
        given = [m for m in (ca, cm, cp) if m is not None]
        if not given:
            raise ValueError('no rows at all')
        nF = sps.csr_matrix(given[0]).shape[0]
        new.ca = sps.csr_matrix((nF, new.NV) if ca is None else ca)
        new.cm = sps.csr_matrix((nF, new.NV) if cm is None else cm)
        new.cp = sps.csr_matrix((nF, new.NP) if cp is None else cp)
        for mat, ncol in ((new.ca, new.NV), (new.cm, new.NV),
                          (new.cp, new.NP)):
            if mat.shape != (nF, ncol):
                raise ValueError('rows of shape {0}, expected {1}'.format(
                    mat.shape, (nF, ncol)))
        new.c0 = np.zeros(nF) if c0 is None else \
            np.asarray(c0, dtype=np.float64).reshape(nF)
        # (rows have no boundary terms: the constant is the caller's)
        new.cab = sps.csr_matrix((nF, new.ndbc))
        new.cmb = sps.csr_matrix((nF, new.ndbc))
        new.c0b = new.c0.copy()
        new.scale = np.ones(nF) if scale is None else \
            np.asarray(scale, dtype=np.float64).reshape(nF)
        new.cells = [np.zeros(0, dtype=np.int32) for _ in range(nF)]
        new.weights = [np.zeros((0, 12)) for _ in range(nF)]
        new.names = list(names) if names is not None else \
            ['f{0}'.format(k) for k in range(nF)]
        new._tidy()
        return new

    def __add__(self, other):
        if other.th is not self.th or (
                self.inv is not None and other.inv is not None
                and other.NV != self.NV):
            raise ValueError('functionals of different problems')
        new = (self if self.inv is not None else other)._empty_like()

        def wide(fn, mat):      # (pressure-only rows in the velocity space)
            return mat if fn.inv is not None or new.inv is None \
                else sps.csr_matrix((fn.nF, new.NV))

        def wideb(fn, mat):
            return mat if fn.inv is not None or new.inv is None \
                else sps.csr_matrix((fn.nF, new.ndbc))
        if self.inv is not None and other.inv is not None and not \
                np.array_equal(self.dbi, other.dbi):
            raise ValueError('functionals with different Dirichlet dofs')
        new.ca = sps.vstack([wide(self, self.ca),
                             wide(other, other.ca)]).tocsr()
        new.cm = sps.vstack([wide(self, self.cm),
                             wide(other, other.cm)]).tocsr()
        new.cp = sps.vstack([self.cp, other.cp]).tocsr()
        new.cab = sps.vstack([wideb(self, self.cab),
                              wideb(other, other.cab)]).tocsr()
        new.cmb = sps.vstack([wideb(self, self.cmb),
                              wideb(other, other.cmb)]).tocsr()
        new.c0 = np.concatenate([self.c0, other.c0])
        new.c0b = np.concatenate([self.c0b, other.c0b])
        new.scale = np.concatenate([self.scale, other.scale])
        new.cells = list(self.cells) + list(other.cells)
        new.weights = list(self.weights) + list(other.weights)
        new.names = list(self.names) + list(other.names)
        new._tidy()
        return new

    def scaled(self, factors):
        """a copy whose scales are multiplied by `factors` (a number or one
        per functional): force coefficients `2 F/(Ubar^2 D)`"""
        new = self._empty_like()
        new.ca, new.cm, new.cp = self.ca, self.cm, self.cp
        new.cab, new.cmb, new.c0b = self.cab, self.cmb, self.c0b
        new.c0, new.cells, new.weights = self.c0, self.cells, self.weights
        new.names = list(self.names)
        new.scale = self.scale*np.asarray(factors, dtype=np.float64)
        return new

    def without_rate(self, names=None):
        """a copy without the `M dv/dt` term: the force of a steady state,
        `-phi^T (A v + N(v) v - J^T p)`"""
        new = self.scaled(1.)
        new.cm = sps.csr_matrix(self.cm.shape)
        new.cmb = sps.csr_matrix(self.cmb.shape)
        if names is not None:
            new.names = list(names)
        return new

    # -- what the device is handed ---------------------------------------
    def device_args(self, moving=False):
        """`dict(ca, cm, cp, c0, scale, cell_ptr, cell_idx, cell_w)` in the
        layout of `dns_imex_set_functionals`; `moving`: with `cab`, `cmb`
        (`nF x ndbc`) and the boundary-free constant for `c0`, the layout of
        `dns_imex_set_functionals_bc`"""
        cell_ptr = np.zeros(self.nF + 1, dtype=np.int32)
        cell_ptr[1:] = np.cumsum([c.size for c in self.cells])
        cell_idx = np.concatenate(self.cells).astype(np.int32) \
            if self.nF else np.zeros(0, dtype=np.int32)
        cell_w = np.vstack(self.weights).reshape(-1) if self.nF \
            else np.zeros(0)
        args = dict(ca=self.ca, cm=self.cm, cp=self.cp,
                    c0=np.ascontiguousarray(self.c0),
                    scale=np.ascontiguousarray(self.scale),
                    cell_ptr=cell_ptr, cell_idx=cell_idx,
                    cell_w=np.ascontiguousarray(cell_w, dtype=np.float64))
        if moving:
            args.update(cab=self.cab, cmb=self.cmb,
                        c0=np.ascontiguousarray(self.c0b))
        return args

    # -- the NumPy statement ----------------------------------------------
    def _cell_sums(self, v, dbc=None):
        """`(N_loc, |N_loc|)` of the listed cells of every functional:
        `(k, 12)` local convection sums and the sums of the absolute values
        of their quadrature products; `dbc`: Dirichlet values other than the
        problem's"""
        th = self.th
        out = []
        if self.inv is not None:
            full = self.bcs.copy()
            if dbc is not None:
                full[self.dbi] = dbc
            full[self.inv] = v
        for cells in self.cells:
            if cells.size == 0:
                out.append((np.zeros((0, 12)), np.zeros((0, 12))))
                continue
            uloc = full[th._vdofs()[cells]]                       # (k, 6, 2)
            gphi = th._gphi[cells]
            w = thm._QW[None, :]*th.area[cells][:, None]
            uq = np.einsum('qa,cai->cqi', th._phi, uloc)
            guq = np.einsum('cqaj,cai->cqij', gphi, uloc)
            conv = np.einsum('cqij,cqj->cqi', guq, uq)
            floc = np.einsum('cq,qa,cqi->cai', w, th._phi, conv)
            fabs = np.einsum('cq,qa,cqi->cai', w, np.abs(th._phi),
                             np.abs(conv))
            out.append((floc.reshape((-1, 12)), fabs.reshape((-1, 12))))
        return out

    def evaluate(self, v, v_prev, p, dt, return_scale=False, dbc=None,
                 dbc_prev=None):
        """`y (nF,)` for inner velocities `v`, `v_prev` and the pressure `p`;
        with `return_scale` also `T_k = |scale_k| (sum of the absolute values
        of every product + |c0_k|)`, the size rounding errors are relative
        to (for the cells: of the products of the quadrature sums).  `dbc`,
        `dbc_prev` (`ndbc` values in the order of `dbcinds`; `dbc_prev`
        defaults to `dbc`): the Dirichlet values that belong to `v` and to
        `v_prev` where they change with time -- the second form of the module
        docstring; `T_k` then counts the products of `cab`, `cmb` too"""
        v = np.asarray(v, dtype=np.float64).reshape(-1)[:self.ca.shape[1]]
        vp = np.asarray(v_prev,
                        dtype=np.float64).reshape(-1)[:self.ca.shape[1]]
        p = np.asarray(p, dtype=np.float64).reshape(-1)
        vdot = (v - vp)/dt
        lin = self.ca @ v + self.cm @ vdot + self.cp @ p
        big = abs(self.ca) @ np.abs(v) + abs(self.cm) @ np.abs(vdot) \
            + abs(self.cp) @ np.abs(p)
        const = self.c0
        if dbc is not None and self.inv is None:
            const = self.c0b         # (pressure-only rows: no boundary terms)
        elif dbc is not None:
            g = np.asarray(dbc, dtype=np.float64).reshape(-1)
            gp = g if dbc_prev is None else \
                np.asarray(dbc_prev, dtype=np.float64).reshape(-1)
            if g.size != self.ndbc or gp.size != self.ndbc:
                raise ValueError('`dbc` must hold {0} values'.format(
                    self.ndbc))
            gdot = (g - gp)/dt
            lin = lin + self.cab @ g + self.cmb @ gdot
            big = big + abs(self.cab) @ np.abs(g) \
                + abs(self.cmb) @ np.abs(gdot)
            const = self.c0b
        elif dbc_prev is not None:
            raise ValueError('`dbc_prev` without `dbc`')
        nl, nlbig = np.zeros(self.nF), np.zeros(self.nF)
        for k, (floc, fabs) in enumerate(self._cell_sums(v, dbc)):
            nl[k] = float((self.weights[k]*floc).sum())
            nlbig[k] = float((np.abs(self.weights[k])*fabs).sum())
        y = self.scale*(lin + nl + const)
        if return_scale:
            return y, np.abs(self.scale)*(big + nlbig + np.abs(const))
        return y


def cylinder_nodes(th, center=(0.2, 0.2), radius=0.05, margin=1e-3):
    """the P2 nodes on the cylinder of the wake meshes"""
    nodes, xy = th.boundary_nodes()
    r = np.sqrt((xy[:, 0] - center[0])**2 + (xy[:, 1] - center[1])**2)
    return nodes[r < radius + margin]


def boundary_forces(th, femp, nodes=None, names=('fx', 'fy')):
    """drag and lift: `phi = 1` on the x (y) dofs of `nodes` (default: the
    cylinder of the wake meshes), the force the fluid exerts on them"""
    nodes = cylinder_nodes(th) if nodes is None else \
        np.asarray(nodes, dtype=np.int64)
    n = nodes.size
    phis = sps.csc_matrix(
        (np.ones(2*n), (np.concatenate([2*nodes, 2*nodes + 1]),
                        np.repeat([0, 1], n))), shape=(th.vdim, 2))
    return MomentumFunctionals(th, femp, phis, names=names)


def boundary_torque(th, femp, nodes=None, center=(0.2, 0.2), name='torque'):
    """the moment about `center` the fluid exerts on `nodes` (default: the
    cylinder of the wake meshes): `phi = (-(y - yc), x - xc)` on them -- what
    a rotating body needs"""
    nodes = cylinder_nodes(th) if nodes is None else \
        np.asarray(nodes, dtype=np.int64)
    xy = th.nodecoords[nodes]
    n = nodes.size
    vals = np.concatenate([-(xy[:, 1] - center[1]), xy[:, 0] - center[0]])
    phis = sps.csc_matrix(
        (vals, (np.concatenate([2*nodes, 2*nodes + 1]),
                np.zeros(2*n, dtype=np.int64))),
        shape=(th.vdim, 1))
    return MomentumFunctionals(th, femp, phis, names=[name])


def _pressure_dof(th, where):
    if np.ndim(where) == 0:
        return int(where)
    xy = np.asarray(where, dtype=np.float64).reshape(2)
    verts = th.mesh.verts
    return int(th.vert_pdof[np.argmin(((verts - xy[None, :])**2).sum(axis=1))])


def pressure_difference(th, node_a, node_b, femp=None, name='dp'):
    """`p[a] - p[b]`: `node_a`, `node_b` are pressure dofs or points `(x, y)`
    (the nearest vertex is taken); stack it with the functionals of the
    problem (`+`), or give `femp` to use it on its own"""
    a, b = _pressure_dof(th, node_a), _pressure_dof(th, node_b)
    cp = sps.csr_matrix(([1., -1.], ([0, 0], [a, b])), shape=(1, th.pdim))
    return MomentumFunctionals.from_rows(th, femp, cp=cp, names=[name])
