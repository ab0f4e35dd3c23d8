"""Device convection `N(u)u` for P2 velocities on triangles (`dns_conv_*`).

Replaces the per-step host callback `f_vdp` of the reference
(`stokes_navier_utils.py:1136-1140` -> `dolfin_to_sparrays.get_convvec`,
dts:427-472): with an operator attached (`ImexStepper.set_convection`) the
CNAB/SBDF2 loop needs no host round trip at all.
"""
import ctypes as ct

import numpy as np

from . import _capi as C

__all__ = ['ConvectionP2', 'BaseTrajectory', 'lerp_rows']

ROM_MAX_BASIS = 33          # kRomMaxBasis of csrc/galerkin_host.hpp


def _i32(arr):
    return np.ascontiguousarray(arr, dtype=np.int32)


def check_basis(nv, ndbc, basis, dbc_rows=None, ntest=None):
    """the shapes `project_tensor` takes, refused by name on the host:
    returns `(basis (nb, ld) padded to an even `ld`, dbc_rows (nb, ndbc) or
    None, ntest)`"""
    B = np.asarray(basis, dtype=np.float64)
    if B.ndim != 2 or B.shape[1] < nv or B.shape[1] > nv + 64 \
            or (B.shape[1] != nv and B.shape[1] % 2):
        raise ValueError(
            '`basis` must be nb x {0} (the inner dofs; or padded to an '
            'even width), it is {1}'.format(nv, B.shape))
    nb = B.shape[0]
    if not 1 <= nb <= ROM_MAX_BASIS:
        raise ValueError(
            '`basis` has nb = {0} rows, the tensor kernel takes 1..{1} '
            '(32 modes and a mean flow)'.format(nb, ROM_MAX_BASIS))
    nt = nb if ntest is None else int(ntest)
    if not 1 <= nt <= nb:
        raise ValueError('`ntest` = {0} outside 1..nb = {1}'.format(nt, nb))
    D = None
    if dbc_rows is not None:
        D = np.ascontiguousarray(dbc_rows, dtype=np.float64)
        if D.shape != (nb, ndbc):
            raise ValueError(
                '`dbc_rows` must be nb x ndbc = {0} x {1}, it is {2}'
                .format(nb, ndbc, D.shape))
    if B.shape[1] % 2:
        B = np.hstack([B, np.zeros((nb, 1))])
    return np.ascontiguousarray(B), D, nt


# what `time_int_utils._checkuniformgrid` takes for "the same time":
# `np.allclose(., 0)`, its absolute tolerance
TIME_ATOL = 1e-8


def lerp_rows(v0, v1, theta):
    """`v0 + theta*(v1 - v0)`, each operation rounded once: the base flow an
    interpolating operator evaluates about, bit for bit (the device does the
    same three operations, uncontracted)"""
    v0 = np.asarray(v0, dtype=np.float64)
    return v0 + np.float64(theta)*(np.asarray(v1, dtype=np.float64) - v0)


class BaseTrajectory(object):
    """A time-varying base flow for `ConvectionP2.set_base_flow`: `m` stored
    flows and their times, held piecewise constant (zero-order hold) or, with
    `interpolate=True`, interpolated linearly between the stored times
    (`weights_at`; the loops of `time_int_utils` then arm weights beside the
    rows).

    `times`: `m` ascending stored times.  `v_rows`: `(m, nv)` inner values or
    `(m, vdim)` full velocity vectors (`None`: the rows are on the device
    already, `ImexStepper.ensemble_to_base`).  `dbcvals`: the base flow's
    Dirichlet values, `(ndbc,)` for every row or `(m, ndbc)` (`None` with full
    vectors: taken from them).  `time_map`: loop time -> stored time, the
    identity by default; `lambda t: T - t` makes an adjoint run walk a stored
    forward run backwards.  `interpolate`: a flow stored every k-th step is
    a second-order representation of `V(t)` instead of a first-order one, at
    the price of a second gather in the element kernels."""

    def __init__(self, times, v_rows, dbcvals=None, time_map=None,
                 interpolate=False):
        t = np.array(times, dtype=np.float64).reshape(-1)
        if t.size < 1 or not np.all(np.isfinite(t)) \
                or np.any(np.diff(t) <= TIME_ATOL):
            raise ValueError('`times` must be ascending stored times, at '
                             'least one: {0}'.format(t.tolist()[:8]))
        self.times, self.time_map = t, time_map
        self.v_rows = None if v_rows is None else \
            np.asarray(v_rows, dtype=np.float64)
        if self.v_rows is not None and (
                self.v_rows.ndim != 2 or self.v_rows.shape[0] != t.size):
            raise ValueError('`v_rows` must be {0} rows, one per stored time: '
                             '{1}'.format(t.size, self.v_rows.shape))
        self.dbcvals = None if dbcvals is None else \
            np.asarray(dbcvals, dtype=np.float64)
        # one stored flow holds for good; else a row holds for one interval
        self.hold = np.inf if t.size == 1 else t[-1] - t[-2]
        self.interpolate = bool(interpolate)

    @property
    def nrows(self):
        return self.times.size

    def _stored_time(self, t):
        """`(time_map(t), how the refusals name the time)`"""
        tm = float(t) if self.time_map is None \
            else float(self.time_map(float(t)))
        what = 'time {0!r}'.format(float(t)) + (
            '' if self.time_map is None
            else ' (stored time {0!r})'.format(tm))
        return tm, what

    def weights_at(self, ts):
        """`(rows, theta)` for linear interpolation: `rows` as `rows_at`,
        `theta = (tm - t_r)/(t_{r+1} - t_r)` in `[0, 1)` with `tm =
        time_map(t)` -- exactly 0.0 within `TIME_ATOL` of a stored time (a
        time that close to the NEXT stored time is that row with weight 0).
        No extrapolation: `ValueError`, by the time, before the first stored
        time and more than `TIME_ATOL` behind the last (the one-interval hold
        of `rows_at` does not apply)"""
        rows = np.empty(len(ts), dtype=np.int32)
        theta = np.zeros(len(ts))
        times = self.times
        for k, t in enumerate(ts):
            tm, what = self._stored_time(t)
            r = int(np.searchsorted(times, tm + TIME_ATOL, side='right')) - 1
            if r < 0 or not np.isfinite(tm):
                raise ValueError(
                    'base trajectory: {0} lies before the first stored time '
                    '{1!r}'.format(what, float(times[0])))
            rows[k] = r
            if abs(tm - times[r]) <= TIME_ATOL:
                continue
            if r + 1 >= times.size:
                raise ValueError(
                    'base trajectory: {0} lies behind the last stored time '
                    '{1!r}: interpolation between stored rows does not '
                    'extrapolate'.format(what, float(times[-1])))
            th = (tm - times[r])/(times[r + 1] - times[r])
            theta[k] = min(max(th, 0.0), np.nextafter(1.0, 0.0))
        return rows, theta

    def flow_at(self, time):
        """the row of `v_rows` the operator evaluates about at loop time
        `time` -- held, or with `interpolate` `lerp_rows` of the two rows: the
        host statement of a step is `fem.TaylorHood.linearised_convection_vec`
        about this vector"""
        if not self.interpolate:
            return self.v_rows[self.row_at(time)]
        rows, th = self.weights_at([time])
        r = int(rows[0])
        return lerp_rows(self.v_rows[r],
                         self.v_rows[min(r + 1, self.nrows - 1)], th[0])

    def row_at(self, time):
        return int(self.rows_at([time])[0])

    def rows_at(self, ts):
        """for each loop time the index of the last stored time `<=
        time_map(t)` (within `TIME_ATOL`).  `ValueError`, by the time, before
        the first stored time and more than one storage interval behind the
        last"""
        rows = np.empty(len(ts), dtype=np.int32)
        for k, t in enumerate(ts):
            tm = float(t) if self.time_map is None \
                else float(self.time_map(float(t)))
            r = int(np.searchsorted(self.times, tm + TIME_ATOL,
                                    side='right')) - 1
            what = 'time {0!r}'.format(float(t)) + (
                '' if self.time_map is None
                else ' (stored time {0!r})'.format(tm))
            if r < 0 or not np.isfinite(tm):
                raise ValueError(
                    'base trajectory: {0} lies before the first stored time '
                    '{1!r}'.format(what, float(self.times[0])))
            if tm - self.times[-1] > self.hold + TIME_ATOL:
                raise ValueError(
                    'base trajectory: {0} lies more than one storage interval '
                    '({1!r}) behind the last stored time {2!r}'.format(
                        what, float(self.hold), float(self.times[-1])))
            rows[k] = r
        return rows

    def resolve_dbcvals(self, ndbc, full=None, dbcinds=None):
        """the Dirichlet values as the library takes them: `(sets, flat)`"""
        D = self.dbcvals
        if D is None and ndbc == 0:
            D = np.zeros((1, 0))
        if D is None:
            if full is None:
                raise ValueError('base trajectory: `dbcvals`, the base '
                                 'flow\'s Dirichlet values, are needed')
            D = full[:, dbcinds]
        D = np.ascontiguousarray(D, dtype=np.float64)
        if D.ndim <= 1 or (D.ndim == 2 and D.shape[0] == 1
                           and self.nrows != 1):
            D = D.reshape((1, -1))
        if D.shape not in ((1, ndbc), (self.nrows, ndbc)):
            raise ValueError(
                'base trajectory: `dbcvals` must be ({0},) or ({1}, {0}), it '
                'is {2}'.format(ndbc, self.nrows, D.shape))
        flat = D.reshape(-1) if D.size else np.zeros(1)
        return D.shape[0], np.ascontiguousarray(flat)


class ConvectionP2(object):
    def __init__(self, cell_vdofs, glam, area, vdim, invinds, dbcinds,
                 dbcvals, device=0):
        """`cell_vdofs (nc, 6, 2)`, `glam (nc, 3, 2)`, `area (nc,)` -- the
        element data any P2 FE library has (see include/dns_amd.h)"""
        self.lib = C.load_library()
        cv = _i32(np.asarray(cell_vdofs).reshape(-1))
        gl = np.ascontiguousarray(np.asarray(glam, dtype=np.float64).reshape(-1))
        ar = C.as_f64(area)
        self.ncells = ar.size
        self._cell_vdofs = cv.reshape((-1, 12))
        # (the element data stays here as well: `fem.GalerkinROM`'s host model
        # works from the same object)
        self.glam, self.area = gl.reshape((-1, 3, 2)), ar
        self._dbcinds = None
        self.dbc_table_rows = 0     # > 0: a time-varying Dirichlet table is set
        self.base_trajectory = None     # the `BaseTrajectory` that is set
        self._vdim = int(vdim)
        inv, dbi = _i32(invinds), _i32(dbcinds)
        self._invinds = inv
        dbv = C.as_f64(dbcvals, size=dbi.size)
        self._dbcinds = dbi
        self.dbcvals = np.array(dbv)    # the constant set (None: a table)
        self.ndbc = int(dbi.size)
        self.nv = inv.size
        self._h = ct.c_void_p()
        C.check(self.lib.dns_conv_create_p2(
            device, self.ncells, cv.ctypes.data_as(C.c_int32_p), C.dptr(gl),
            C.dptr(ar), int(vdim), inv.size, inv.ctypes.data_as(C.c_int32_p),
            dbi.size, dbi.ctypes.data_as(C.c_int32_p), C.dptr(dbv),
            ct.byref(self._h)))

    @classmethod
    def from_taylor_hood(cls, th, invinds, dbcinds, dbcvals, device=0):
        """element data of the scaffolding assembler (`fem.TaylorHood`)"""
        return cls(th._vdofs(), th.glam, th.area, th.vdim, invinds, dbcinds,
                   dbcvals, device=device)

    def set_dbcvals(self, dbcvals):
        """one constant set of Dirichlet values (drops a value table)"""
        dbv = C.as_f64(dbcvals, size=self.ndbc)
        C.check(self.lib.dns_conv_set_dbcvals(self._h, C.dptr(dbv)))
        self.dbc_table_rows = 0
        self.dbcvals = np.array(dbv)

    def set_dbc_table(self, table):
        """`(nrows, ndbc)` Dirichlet values per step (IMEX stepper: row s for
        the s-th step after the stepper's tables were set) or per trajectory
        slot (trapezoidal sweeps)"""
        tab = np.ascontiguousarray(table, dtype=np.float64).reshape(
            (-1, max(self.ndbc, 1)) if self.ndbc else (len(table), 0))
        nrows = tab.shape[0]
        flat = C.as_f64(tab) if tab.size else np.zeros(1)
        C.check(self.lib.dns_conv_set_dbc_table(self._h, int(nrows),
                                                C.dptr(flat)))
        self.dbc_table_rows = int(nrows)
        self.dbcvals = None

    def set_dbc_row(self, row):
        C.check(self.lib.dns_conv_set_dbc_row(self._h, int(row)))

    # -- linearised / adjoint convection about a base flow --------------------
    def set_base_flow(self, base, adjoint=False):
        """From here on the operator evaluates, for the perturbation `w` it
        is handed (`apply`, an attached `cnab` / `sbdftwo` loop),
        `L(V)w = N(V)w + N(w)V` -- or with `adjoint` the transpose
        `(N1(V) + N2(V))_II^T w` -- instead of `N(w)w`.  `base`: the full
        velocity vector `V` (`vdim` entries) or the pair `(v_inner, dbcvals)`.
        The perturbation's own Dirichlet values stay the operator's; the
        adjoint takes zero values and no table (`ValueError` otherwise).

        `base` may be a `BaseTrajectory`: a time-varying base flow, uploaded
        once.  `set_base_rows` then names the row of every step of an attached
        loop, `set_base_row` the row for `apply`; `cnab` / `sbdftwo` arm both
        from the trajectory's times -- with the weights towards the next row
        when the trajectory was made with `interpolate=True`"""
        if isinstance(base, BaseTrajectory):
            return self._set_base_trajectory(base, adjoint)
        if isinstance(base, (tuple, list)) and len(base) == 2:
            vin = C.as_f64(base[0], size=self.nv)
            dbv = C.as_f64(base[1], size=self.ndbc)
        else:
            full = C.as_f64(base, size=self._vdim)
            vin = np.ascontiguousarray(full[self._invinds])
            dbv = np.ascontiguousarray(full[self._dbcinds])
        if dbv.size == 0:
            dbv = np.zeros(1)
        C.check(self.lib.dns_conv_set_base_flow(
            self._h, C.dptr(vin), C.dptr(dbv), int(bool(adjoint))))
        self.base_trajectory = None

    def _set_base_trajectory(self, traj, adjoint):
        R = traj.v_rows
        if R is None or R.shape[1] not in (self.nv, self._vdim):
            raise ValueError(
                'base trajectory: `v_rows` must be ({0}, {1}) inner values or '
                '({0}, {2}) full vectors, it is {3}'.format(
                    traj.nrows, self.nv, self._vdim,
                    None if R is None else R.shape))
        full = R if (R.shape[1] == self._vdim and self._vdim != self.nv) \
            else None
        sets, dflat = traj.resolve_dbcvals(self.ndbc, full, self._dbcinds)
        rows = np.ascontiguousarray(R if full is None
                                    else full[:, self._invinds])
        C.check(self.lib.dns_conv_set_base_trajectory(
            self._h, traj.nrows,
            C.dptr(rows.reshape(-1) if rows.size else np.zeros(1)),
            int(rows.shape[1]), int(sets), C.dptr(dflat), int(bool(adjoint))))
        self.base_trajectory = traj

    def set_base_rows(self, rows, weights=None):
        """the per-step index table of a base trajectory: the `s`-th step of
        the chunk an attached stepper runs next evaluates about row
        `rows[min(s, len(rows) - 1)]` (descending: a reversed adjoint run;
        repeats: a trajectory stored every k-th step).  `weights`: one
        `theta` in `[0, 1)` per entry, the step evaluates about `V_r +
        theta*(V_{r+1} - V_r)` (`lerp_rows`, bit for bit); `None`: the
        zero-order hold, which also takes weights off that were set.
        `ValueError`, the operator as it was: weights outside `[0, 1)` or not
        finite, a non-zero weight on the last row, another length than
        `rows`"""
        r = _i32(np.asarray(rows).reshape(-1))
        if weights is None:
            C.check(self.lib.dns_conv_set_base_rows(
                self._h, int(r.size), r.ctypes.data_as(C.c_int32_p)))
            return
        w = np.ascontiguousarray(
            np.asarray(weights, dtype=np.float64).reshape(-1))
        if w.size != r.size:
            raise ValueError(
                'base trajectory: {0} interpolation weights for {1} base '
                'rows, one per entry'.format(w.size, r.size))
        C.check(self.lib.dns_conv_set_base_rows_lerp(
            self._h, int(r.size), r.ctypes.data_as(C.c_int32_p),
            C.dptr(w if w.size else np.zeros(1))))

    def set_base_row(self, row, weight=0.0):
        """the row of the base trajectory `apply`, `cell_values` and
        `host_callback` evaluate about (takes the index table off); with a
        non-zero `weight` in `(0, 1)`, between that row and the next.  Weight
        0.0 is the row itself: the zero-order entry point, which takes the
        weights off"""
        if weight == 0.0:
            C.check(self.lib.dns_conv_set_base_row(self._h, int(row)))
        else:
            C.check(self.lib.dns_conv_set_base_row_lerp(
                self._h, int(row), float(weight)))

    @property
    def interpolates(self):
        """True while interpolation weights are armed (`set_base_rows` with
        `weights`, `set_base_row` with a non-zero `weight`)"""
        lerp = ct.c_int32(0)
        C.check(self.lib.dns_conv_get_base_lerp(self._h, ct.byref(lerp)))
        return bool(lerp.value)

    @property
    def base_trajectory_rows(self):
        """rows of the base trajectory on the device; 0: a constant base flow
        or none"""
        return self._base_info()[0]

    def _base_info(self):
        nrows, nbrow = ct.c_int32(0), ct.c_int32(0)
        C.check(self.lib.dns_conv_get_base_info(self._h, ct.byref(nrows),
                                                ct.byref(nbrow)))
        return nrows.value, nbrow.value

    def clear_base_flow(self):
        """back to `N(v)v`"""
        C.check(self.lib.dns_conv_clear_base_flow(self._h))
        self.base_trajectory = None

    @property
    def linearised(self):
        """False, 'forward' or 'adjoint'"""
        mode = ct.c_int32(0)
        C.check(self.lib.dns_conv_get_mode(self._h, ct.byref(mode)))
        return {0: False, 1: 'forward', 2: 'adjoint'}[mode.value]

    def cell_values(self, v_inner, sel=None, fill=0.0):
        """TEST ONLY: `(cells (12, ncells), pos)` -- what the element launch
        leaves for `v_inner` in the current mode, in the operator's internal
        cell order, and the caller's cell -> internal cell.  `sel`: internal
        cells to evaluate, every other entry is `fill`"""
        v = C.as_f64(v_inner, size=self.nv)
        out = np.empty((12, self.ncells))
        pos = np.empty(self.ncells, dtype=np.int32)
        s = None if sel is None else _i32(sel)
        C.check(self.lib.dns_conv_cells_probe(
            self._h, C.dptr(v),
            None if s is None or s.size == 0
            else s.ctypes.data_as(C.c_int32_p),
            -1 if s is None else int(s.size), float(fill),
            C.dptr(out.reshape(-1)), pos.ctypes.data_as(C.c_int32_p)))
        return out, pos

    def apply(self, v_inner, scale=1.0):
        """`scale*N(v)v` on the inner dofs -- with a base flow set,
        `scale*L(V)v` or its transpose"""
        v = C.as_f64(v_inner, size=self.nv)
        out = np.empty(self.nv)
        C.check(self.lib.dns_conv_apply(self._h, C.dptr(v), float(scale),
                                        C.dptr(out)))
        return out.reshape((-1, 1))

    # -- the convection tensor of a Galerkin projection ----------------------
    def check_basis(self, basis, dbc_rows=None, ntest=None):
        return check_basis(self.nv, self.ndbc, basis, dbc_rows, ntest)

    def project_tensor(self, basis, dbc_rows=None, ntest=None):
        """`T[i, j, k] = int phi_i . (u_j . grad) u_k` (`ntest x nb x nb`; `j`
        convects, `k` is convected) on the device, `dns_conv_project_tensor`:
        `u_b` is row `b` of `basis` on the inner dofs and row `b` of `dbc_rows`
        (None: zeros) on the Dirichlet dofs, the test functions `phi_i` are the
        rows `i < ntest` on the inner dofs and vanish on the Dirichlet dofs.
        The operator's own Dirichlet values play no part"""
        B, D, nt = self.check_basis(basis, dbc_rows, ntest)
        nb, ld = B.shape
        out = np.empty((nt, nb, nb))
        C.check(self.lib.dns_conv_project_tensor(
            self._h, nb, nt, ld, C.dptr(B.reshape(-1)),
            None if (D is None or D.size == 0) else C.dptr(D.reshape(-1)),
            C.dptr(out.reshape(-1))))
        return out

    # -- linearised convection matrices (Newton/Picard sweeps) ---------------
    def connectivity(self):
        """CSR of ones: all pairs of inner velocity dofs sharing a cell -- the
        pattern of the condensed `N1(u) + N2(u)` for any `u`"""
        import scipy.sparse as sps
        code = np.full(self._vdim, -1, dtype=np.int64)
        code[self._invinds] = np.arange(self.nv)
        loc = code[self._cell_vdofs]                      # (nc, 12)
        rows = np.repeat(loc[:, :, None], 12, axis=2).reshape(-1)
        cols = np.repeat(loc[:, None, :], 12, axis=1).reshape(-1)
        keep = (rows >= 0) & (cols >= 0)
        pat = sps.coo_matrix((np.ones(int(keep.sum())),
                              (rows[keep], cols[keep])),
                             shape=(self.nv, self.nv)).tocsr()
        pat.sum_duplicates()
        pat.sort_indices()
        pat.data[:] = 1.
        return pat

    def bind_pattern(self, pattern):
        """the CSR pattern `assemble` (and the trapezoidal stepper) fill; it
        must contain `connectivity()`"""
        view = C.CsrView(pattern)
        C.check(self.lib.dns_conv_bind_pattern(self._h, view.byref()))
        self._pattern = view

    def assemble(self, u_inner, newton=False, dbcvals_lin=None,
                 dbcvals_rhs=None):
        """`(N, rhsbc, rhscon)`: `N1(u)` (Picard) or `N1(u) + N2(u)` (Newton)
        condensed, in the bound pattern; `-N[:, bc] bcvals`; `N(u)u`
        (reference `get_v_conv_conts`, snu:109-133).  `dbcvals_lin` /
        `dbcvals_rhs`: Dirichlet values of the linearisation field / the ones
        that go to `rhsbc` (default: the operator's own set)"""
        import scipy.sparse as sps
        u = C.as_f64(u_inner, size=self.nv)
        pv = self._pattern
        nvals = np.empty(pv.data.size)
        rhsbc, rhscon = np.empty(self.nv), np.empty(self.nv)
        if dbcvals_lin is None:
            C.check(self.lib.dns_conv_assemble(
                self._h, C.dptr(u), int(bool(newton)), C.dptr(nvals),
                C.dptr(rhsbc), C.dptr(rhscon)))
        else:
            dl = C.as_f64(dbcvals_lin, size=self.ndbc) if self.ndbc else \
                np.zeros(1)
            dr = None if dbcvals_rhs is None else (
                C.as_f64(dbcvals_rhs, size=self.ndbc) if self.ndbc
                else np.zeros(1))
            C.check(self.lib.dns_conv_assemble2(
                self._h, C.dptr(u), C.dptr(dl), C.dptr(dr), int(bool(newton)),
                C.dptr(nvals), C.dptr(rhsbc), C.dptr(rhscon)))
        N = sps.csr_matrix((nvals, pv.indices, pv.indptr), shape=pv.shape)
        return N, rhsbc.reshape((-1, 1)), rhscon.reshape((-1, 1))

    def host_callback(self, invinds, scale=-1.0):
        """an `f_vdp(vfull)` callable (reference tiu:113) backed by this
        operator: the inner part of `vfull` in, `scale*N(v)v` out (with a
        base flow set: what `apply` gives then)"""
        inv = np.asarray(invinds)

        def f_vdp(vfull):
            return self.apply(np.asarray(vfull).reshape(-1)[inv], scale=scale)
        return f_vdp

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self.lib.dns_conv_destroy(self._h)
            self._h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
