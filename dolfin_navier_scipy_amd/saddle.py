"""Python handles on the device objects of `include/dns_amd.h`."""
import ctypes as ct

import numpy as np
import scipy.sparse as sps

from . import _capi as C

__all__ = ['streaming_precond_defaults', 'choose_schur', 'SaddleSystem', 'ImexStepper', 'spmv', 'dot', 'axpy', 'gemv',
           'dense_inverse', 'spmv_bench', 'spmv_pair', 'spmv_epilogue', 'solve_opts', 'precond_opts',
           'ensemble_gram', 'ensemble_combine', 'ensemble_project']

_METHODS = {'gmres': C.DNS_METHOD_GMRES, 'bicgstab': C.DNS_METHOD_BICGSTAB}
_SCHUR = {'dense': C.DNS_SCHUR_DENSE, 'jacobi': C.DNS_SCHUR_JACOBI, 'mg': 2}
_VARIANTS = {'vector': C.DNS_SPMV_VECTOR, 'stream': C.DNS_SPMV_STREAM,
             'stream16': 2}
_FHAT = {'cheb': C.DNS_FHAT_CHEB, 'explicit': C.DNS_FHAT_EXPLICIT,
         'auto': C.DNS_FHAT_AUTO}


def solve_opts(method='gmres', restart=60, maxiter=400, reorth=True,
               rtol=1e-10, atol=0., check_every=4, use_graph=False):
    """`reorth`: True / 1 classical Gram-Schmidt twice, False / 0 once, 2 once
    and fused into the head kernel.  On a row-partitioned handle (`set_comm`,
    `from_rows`) `reorth = 1` is ONE pass as well: its explicit branch runs
    `k_orth<0>` alone, a second pass would cost two more all-reduces per
    column (pinned by `tests/test_gpu_zz_dist_krylov.py`)."""
    o = C.dns_solve_opts()
    C.load_library().dns_default_solve_opts(ct.byref(o))
    o.method = _METHODS[method.lower()] if isinstance(method, str) else method
    o.restart, o.maxiter = int(restart), int(maxiter)
    # True/1: CGS2, False/0: CGS once, 2: CGS once fused into the head kernel
    o.reorth = 2 if (reorth == 2 and reorth is not True) else (1 if reorth else 0)
    o.rtol, o.atol = float(rtol), float(atol)
    o.check_every = int(check_every)
    o.use_graph = 1 if use_graph else 0
    return o


def precond_opts(cheb_degree=4, schur='dense', fhat='auto', eig_lo=0.,
                 eig_hi=0., eig_lo_safety=0.9, eig_hi_safety=1.05,
                 fp32_store=None, drop_tol=None, factorization='triangular'):
    o = C.dns_precond_opts()
    C.load_library().dns_default_precond_opts(ct.byref(o))
    if fp32_store is not None:
        o.fp32_store = 1 if fp32_store else 0
    if drop_tol is not None:
        o.drop_tol = float(drop_tol)
    o.factorization = {'triangular': 0, 'full': 1}[factorization] \
        if isinstance(factorization, str) else int(factorization)
    o.cheb_degree = int(cheb_degree)
    o.schur = _SCHUR[schur] if isinstance(schur, str) else schur
    o.fhat = _FHAT[fhat] if isinstance(fhat, str) else fhat
    o.eig_lo, o.eig_hi = float(eig_lo), float(eig_hi)
    o.eig_lo_safety, o.eig_hi_safety = float(eig_lo_safety), \
        float(eig_hi_safety)
    return o


class SaddleSystem(object):
    """`[[F, JT], [J, 0]]` resident in HBM with its block preconditioner"""

    def __init__(self, F, J, JT=None, device=0):
        self.lib = C.load_library()
        self._f = C.CsrView(F)
        self._j = C.CsrView(J)
        self._jt = C.CsrView(JT) if JT is not None else None
        self.NP, self.NV = self._j.shape
        self.n = self.NV + self.NP
        self.device = device
        self._h = ct.c_void_p()
        C.check(self.lib.dns_saddle_create(
            device, self._f.byref(), self._j.byref(),
            self._jt.byref() if self._jt is not None else None,
            ct.byref(self._h)))
        self.last_stats = None
        self.precond_ready = False

    @classmethod
    def from_rows(cls, F_rows, JT_rows, J_rows, NV, NP, comm, device=0):
        """rank-local construction (`dns_saddle_create_rows`): this rank's rows
        of `F` and `J^T` -- rows `comm.partition_range(NV)` -- and of `J` --
        rows `partition_range(NP)` -- with global column indices; no rank
        holds a whole matrix.  Collective over `comm`."""
        self = cls.__new__(cls)
        self.lib = C.load_library()
        self._f = C.CsrView(F_rows)
        self._jt = C.CsrView(JT_rows)
        self._j = C.CsrView(J_rows)
        self.NP, self.NV = int(NP), int(NV)
        self.n = self.NV + self.NP
        self.device = device
        self._comm = comm
        self._h = ct.c_void_p()
        C.check(self.lib.dns_saddle_create_rows(
            device, comm._h, self.NV, self.NP, self._f.byref(),
            self._jt.byref(), self._j.byref(), ct.byref(self._h)))
        self.last_stats = None
        self.precond_ready = False
        self.from_rows_handle = True
        return self

    @classmethod
    def from_rows_of(cls, F, J, comm, device=0):
        """`from_rows` with the rows cut out of whole SciPy matrices (tests,
        the bench: a distributed assembler hands its rows over directly)"""
        import scipy.sparse as sps
        from .comm import partition_range
        NP, NV = J.shape
        v0, v1 = partition_range(NV, comm.nranks, comm.rank)
        p0, p1 = partition_range(NP, comm.nranks, comm.rank)
        F, J = sps.csr_matrix(F), sps.csr_matrix(J)
        JT = sps.csr_matrix(J[:, v0:v1].T)
        return cls.from_rows(F[v0:v1, :], JT, J[p0:p1, :], NV, NP, comm,
                             device=device)

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self.lib.dns_saddle_destroy(self._h)
            self._h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_comm(self, comm):
        """attach a `comm.Comm` (row-partitioned solve); call before
        `setup_precond`; `None` detaches"""
        C.check(self.lib.dns_saddle_set_comm(
            self._h, comm._h if comm is not None else None))
        # (only once the library has taken it: a handle created from rows
        # refuses another communicator and keeps the one it has)
        self._comm = comm
        self.precond_ready = False

    def device_matrix_bytes(self):
        """bytes of HBM this rank's matrices occupy (`dns_saddle_device_bytes`)
        -- shrinks with the number of ranks of a row-partitioned handle"""
        out = ct.c_int64(0)
        C.check(self.lib.dns_saddle_device_bytes(self._h, ct.byref(out)))
        return out.value

    def host_matrix_bytes(self):
        """`(kept, setup)` bytes of host matrices (`dns_saddle_host_bytes`):
        what the handle keeps, and what its last partitioned set-up held"""
        a, b = ct.c_int64(0), ct.c_int64(0)
        C.check(self.lib.dns_saddle_host_bytes(self._h, ct.byref(a),
                                               ct.byref(b)))
        return a.value, b.value

    def set_schur_mg(self, prolongations, smooth_steps=2):
        """nested pressure spaces for `schur='mg'`: `prolongations[l]` maps
        level `l+1` (coarser) to level `l`, finest first; the coarsest level
        gets a dense inverse"""
        views = [C.CsrView(p) for p in prolongations]
        arr = (C.dns_csr*max(len(views), 1))(*[v.struct for v in views])
        C.check(self.lib.dns_saddle_set_schur_mg(self._h, len(views), arr,
                                                 int(smooth_steps)))
        self.precond_ready = False

    def update_values(self, fdata):
        fdata = C.as_f64(fdata, size=self._f.data.size)
        C.check(self.lib.dns_saddle_update_values(self._h, C.dptr(fdata)))

    def setup_precond(self, **kw):
        o = precond_opts(**kw)
        C.check(self.lib.dns_saddle_setup_precond(self._h, ct.byref(o)))
        self.precond_ready = True

    def cheb_bounds(self):
        lo, hi = ct.c_double(), ct.c_double()
        C.check(self.lib.dns_saddle_cheb_bounds(self._h, ct.byref(lo),
                                                ct.byref(hi)))
        return lo.value, hi.value

    def set_option(self, name, value):
        """a tuning knob of this handle (`dns_saddle_set_option`: `stream_nnz`,
        `pair`, `mg_dense_max`, `mg_dense_half_max`, `mg_part_min`,
        `mg_fused`, `mg_cheb`, `mg_cheb_alpha`, `mg_cycles`, `mg_rho`, `dist_graph`, `oversolve`,
        `oversolve_cmin`); before
        `setup_precond`"""
        C.check(self.lib.dns_saddle_set_option(self._h, name.encode(),
                                               float(value)))
        return self

    def precond_info(self):
        """sizes of the resident preconditioner (bench.py's byte counts)"""
        buf = (ct.c_int64*64)()
        cnt = ct.c_int32(0)
        C.check(self.lib.dns_saddle_precond_info(self._h, 64, buf,
                                                 ct.byref(cnt)))
        v = list(buf[:cnt.value])
        out = dict(nnz_K=v[0], nnz_Gc=v[1], nnz_JG=v[2], NP=v[3],
                   fp32_store=bool(v[4]), cheb_degree=v[5],
                   schur={0: 'dense', 1: 'jacobi', 2: 'mg'}[v[6]],
                   NV=self.NV, nnz_F=int(self._f.data.size),
                   nnz_J=int(self._j.data.size), mg_nu=v[8], mg_levels=[])
        for l in range(v[7]):
            n, nnzs, nnzp = v[9 + 3*l:12 + 3*l]
            out['mg_levels'].append(dict(n=n, nnz_S=nnzs, nnz_P=nnzp))
        tail = 9 + 3*v[7]
        out['pair_format_bytes'] = v[tail] if len(v) > tail else 0
        out['mg_coarse_val_bytes'] = v[tail + 1] if len(v) > tail + 1 else 8
        out['mg_cycles'] = max(1, v[tail + 2]) if len(v) > tail + 2 else 1
        out['mg_two_cycle_maxc'] = v[tail + 3] if len(v) > tail + 3 else 0
        return out

    def solve(self, rhsv, rhsp=None, x0=None, raise_on_fail=True, **kw):
        """returns `[v; p~]` as a 1-D array of length NV+NP"""
        o = kw.pop('opts', None)
        o = solve_opts(**kw) if o is None else o
        rv = C.as_f64(rhsv, size=self.NV)
        rp = None if rhsp is None else C.as_f64(rhsp, size=self.NP)
        xi = None if x0 is None else C.as_f64(x0, size=self.n)
        out = np.empty(self.n)
        st = C.dns_solve_stats()
        C.check(self.lib.dns_saddle_solve(self._h, C.dptr(rv), C.dptr(rp),
                                          C.dptr(xi), C.dptr(out),
                                          ct.byref(o), ct.byref(st)))
        self.last_stats = st.asdict()
        if raise_on_fail and st.status != C.DNS_OK:
            cls = C.NotConverged if st.status == C.DNS_NOT_CONVERGED \
                else C.Breakdown
            raise cls(st.status, 'Krylov solve stopped after {0} iterations '
                      'at relative residual {1:.3e}'.format(st.iters,
                                                            st.est_relres))
        return out

    PROBES = ('head', 'fhat', 'kapply_dots', 'orth', 'resid_norm', 'tail',
              'combine', 'precond', 'arnoldi_step_seq')

    def probe(self, which, chain=64, reps=20):
        """microseconds per launch of one cycle kernel in a replayed graph"""
        idx = self.PROBES.index(which) if isinstance(which, str) else which
        out = ct.c_double(0.)
        C.check(self.lib.dns_saddle_probe(self._h, idx, chain, reps,
                                          ct.byref(out)))
        return out.value

    def solve_multi(self, rhsv, rhsp=None, x0=None, raise_on_fail=True, **kw):
        """`k` right-hand sides in one call (`dns_saddle_solve_multi`): `rhsv`
        `(NV, k)`, `rhsp` `(NP, k)` or None, `x0` `(NV+NP, 1 or k)` or None;
        returns the `(NV+NP, k)` solutions; `last_stats_cols` holds one
        record per column, `last_stats` the last column's"""
        o = kw.pop('opts', None)
        o = solve_opts(**kw) if o is None else o
        rv = np.asarray(rhsv, dtype=np.float64).reshape((self.NV, -1))
        k = rv.shape[1]
        rvf = np.ascontiguousarray(rv.T).reshape(-1)          # column by column
        rpf = None
        if rhsp is not None:
            rpf = np.ascontiguousarray(np.asarray(
                rhsp, dtype=np.float64).reshape((self.NP, k)).T).reshape(-1)
        x0f, x0c = None, 0
        if x0 is not None:
            xa = np.asarray(x0, dtype=np.float64).reshape((self.n, -1))
            x0c = xa.shape[1]
            if x0c not in (1, k):
                raise ValueError('`x0` must have 1 or {0} columns'.format(k))
            x0f = np.ascontiguousarray(xa.T).reshape(-1)
        out = np.empty(k*self.n)
        sts = (C.dns_solve_stats*k)()
        C.check(self.lib.dns_saddle_solve_multi(
            self._h, k, C.dptr(rvf), C.dptr(rpf), C.dptr(x0f), x0c,
            C.dptr(out), ct.byref(o), sts))
        self.last_stats_cols = [st.asdict() for st in sts]
        self.last_stats = self.last_stats_cols[-1]
        if raise_on_fail:
            for c, st in enumerate(sts):
                if st.status != C.DNS_OK:
                    cls = C.NotConverged if st.status == C.DNS_NOT_CONVERGED \
                        else C.Breakdown
                    raise cls(st.status, 'column {0}: Krylov solve stopped '
                              'after {1} iterations at relative residual '
                              '{2:.3e}'.format(c, st.iters, st.est_relres))
        return out.reshape((k, self.n)).T.copy()

    def residual_history_col(self, col):
        cnt = ct.c_int32(0)
        C.check(self.lib.dns_saddle_residual_history_col(
            self._h, int(col), None, 0, ct.byref(cnt)))
        out = np.zeros(max(cnt.value, 1))
        C.check(self.lib.dns_saddle_residual_history_col(
            self._h, int(col), C.dptr(out), cnt.value, ct.byref(cnt)))
        return out[:cnt.value]

    def residual_history(self):
        cnt = ct.c_int32(0)
        C.check(self.lib.dns_saddle_residual_history(self._h, None, 0,
                                                     ct.byref(cnt)))
        out = np.zeros(max(cnt.value, 1))
        C.check(self.lib.dns_saddle_residual_history(
            self._h, C.dptr(out), cnt.value, ct.byref(cnt)))
        return out[:cnt.value]

    def apply(self, x):
        x = C.as_f64(x, size=self.n)
        y = np.empty(self.n)
        C.check(self.lib.dns_saddle_apply(self._h, C.dptr(x), C.dptr(y)))
        return y

    def apply_precond(self, r):
        r = C.as_f64(r, size=self.n)
        z = np.empty(self.n)
        C.check(self.lib.dns_saddle_apply_precond(self._h, C.dptr(r),
                                                  C.dptr(z)))
        return z


class ImexStepper(object):
    """device-resident CNAB/SBDF2 state (`dns_imex_*`)"""

    def __init__(self, system, R1, rows=None):
        """`rows=True` (default on a system created from rows): `R1` holds
        this rank's rows only, or is cut down to them here when it is whole
        (`dns_imex_create_rows`)"""
        self.sys = system
        self.lib = system.lib
        if rows is None:
            rows = getattr(system, 'from_rows_handle', False)
        self._h = ct.c_void_p()
        if rows:
            from .comm import partition_range
            cm = system._comm
            v0, v1 = partition_range(system.NV, cm.nranks, cm.rank)
            if R1.shape[0] == system.NV and (v1 - v0) != system.NV:
                import scipy.sparse as sps
                R1 = sps.csr_matrix(R1)[v0:v1, :]
            self._r1 = C.CsrView(R1)
            C.check(self.lib.dns_imex_create_rows(
                system._h, self._r1.byref(), ct.byref(self._h)))
        else:
            self._r1 = C.CsrView(R1)
            C.check(self.lib.dns_imex_create(system._h, self._r1.byref(),
                                             ct.byref(self._h)))
        self.last_stats = None
        # time steps and Krylov steps since the stepper exists
        self.total_steps, self.total_iters = 0, 0
        self.run_calls = 0          # `run` calls since the stepper exists

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            self.lib.dns_imex_destroy(self._h)
            self._h = ct.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_state(self, v_c, v_p=None, ptilde_c=None, nfc_c=None, nfc_o=None):
        NV, NP = self.sys.NV, self.sys.NP
        args = [C.as_f64(v_c, NV),
                None if v_p is None else C.as_f64(v_p, NV),
                None if ptilde_c is None else C.as_f64(ptilde_c, NP),
                None if nfc_c is None else C.as_f64(nfc_c, NV),
                None if nfc_o is None else C.as_f64(nfc_o, NV)]
        C.check(self.lib.dns_imex_set_state(self._h, *[C.dptr(a)
                                                       for a in args]))

    def set_convection(self, conv, scale=-1.0):
        """attach a `convection.ConvectionP2`: every step then evaluates
        `nfc_c = scale*N(v_c)v_c` on the device (`None` detaches)"""
        self._conv = conv
        C.check(self.lib.dns_imex_set_convection(
            self._h, conv._h if conv is not None else None, float(scale)))

    def set_rhs(self, gvec=None, rhsp=None):
        g = None if gvec is None else C.as_f64(gvec, self.sys.NV)
        gp = None if rhsp is None else C.as_f64(rhsp, self.sys.NP)
        C.check(self.lib.dns_imex_set_rhs(self._h, C.dptr(g), C.dptr(gp)))

    def set_rhs_table(self, gv=None, gp=None):
        """per-step right-hand sides known in advance: row s of `gv`
        `(nsteps, NV)` / `gp` `(nsteps, NP)` is used by the s-th step from now
        on (`dns_imex_set_rhs_table`); `set_rhs` returns to constant vectors"""
        NV, NP = self.sys.NV, self.sys.NP
        tv = None if gv is None else \
            np.ascontiguousarray(gv, dtype=np.float64).reshape((-1, NV))
        tp = None if gp is None else \
            np.ascontiguousarray(gp, dtype=np.float64).reshape((-1, NP))
        nsteps = (tv if tv is not None else tp).shape[0]
        if tv is not None and tp is not None and tp.shape[0] != nsteps:
            raise ValueError('tables of different length')
        C.check(self.lib.dns_imex_set_rhs_table(
            self._h, int(nsteps), C.dptr(None if tv is None else tv.reshape(-1)),
            C.dptr(None if tp is None else tp.reshape(-1))))

    def table_position(self):
        pos, left = ct.c_int32(0), ct.c_int32(0)
        C.check(self.lib.dns_imex_table_position(self._h, ct.byref(pos),
                                                 ct.byref(left)))
        return pos.value, left.value

    @staticmethod
    def coeffs(a_c=1., a_p=0., cn_c=0., cn_o=0., pscale=1., extrapolate=True,
               carry_residual=True):
        """`carry_residual`: the velocity residual of a step's inexact solve
        goes into the next step's right-hand side (include/dns_amd.h): the
        distance to the direct-solve trajectory stays at the size of ONE
        solve's error instead of adding up step after step"""
        return C.dns_imex_coeffs(a_c=a_c, a_p=a_p, cn_c=cn_c, cn_o=cn_o,
                                 pscale=pscale,
                                 extrapolate_x0=int(extrapolate),
                                 carry_residual=int(bool(carry_residual)))

    def step(self, cf, nfc_new=None, opts=None, raise_on_fail=True):
        o = solve_opts() if opts is None else opts
        nf = None if nfc_new is None else C.as_f64(nfc_new, self.sys.NV)
        st = C.dns_solve_stats()
        C.check(self.lib.dns_imex_step(self._h, C.dptr(nf), ct.byref(cf),
                                       ct.byref(o), ct.byref(st)))
        self.last_stats = st.asdict()
        self.total_steps += 1
        self.total_iters += int(st.iters)
        if raise_on_fail and st.status != C.DNS_OK:
            raise C.NotConverged(st.status, 'time step solve failed: '
                                 '{0}'.format(self.last_stats))
        return self.last_stats

    def run(self, nsteps, cf, opts=None, raise_on_fail=True):
        """`nsteps` steps without host callbacks (device convection if
        attached, else the convection history stays frozen); returns
        `(device_seconds, total_iters, last_stats)`.  `last_run` then holds the
        record of the call: time steps whose solve ended at `maxiter`
        (`unconverged`, `first_bad`), steps repeated after a mispredicted
        batch (`replayed`), graphs captured inside the call (`captures`) and
        the six-node steps by the kind of their cycle (`lazy_steps`,
        `eager_steps`).
        Raises `NotConverged` if any step did not converge, like `step()`."""
        o = solve_opts() if opts is None else opts
        st = C.dns_solve_stats()
        secs = ct.c_double(0.)
        its = ct.c_int64(0)
        status = self.lib.dns_imex_run(self._h, int(nsteps), ct.byref(cf),
                                       ct.byref(o), ct.byref(st),
                                       ct.byref(secs), ct.byref(its))
        if status != C.DNS_NOT_CONVERGED:
            C.check(status)
        self.run_calls += 1
        self.last_stats = st.asdict()
        self.total_steps += int(nsteps)
        self.total_iters += int(its.value)
        vals = [ct.c_int32(0) for _ in range(4)]
        C.check(self.lib.dns_imex_run_info(self._h,
                                           *[ct.byref(v) for v in vals]))
        self.last_run = dict(zip(('unconverged', 'first_bad', 'replayed',
                                  'captures'), [v.value for v in vals]))
        kinds = (ct.c_int64*2)()
        C.check(self.lib.dns_imex_run_cycles(self._h, kinds))
        self.last_run['lazy_steps'] = int(kinds[0])
        self.last_run['eager_steps'] = int(kinds[1])
        if status == C.DNS_NOT_CONVERGED and raise_on_fail:
            C.check(status)
        return secs.value, its.value, self.last_stats

    PROBE_FORMS = {0: 'Plain', 1: 'Six', 2: 'Fused', 3: 'DistFront',
                   4: 'Rows', 5: 'StreamRhs', 6: 'StreamRows'}

    def front_probe(self, cf, opts=None, cycle_len=0, nfc_new=None):
        """TEST ONLY (`dns_imex_front_probe`): the front of one step without
        its solve, as a dict -- what the front reads (`nsol`, `ring` `(5, n)`
        in ring order, `nfc_in` `(2, NV)`, `g_in`, `gp_in`, `b_prev`, `r_in`,
        `tab_row`; for a carry plan `kxs_in` `(4, n)`, `rcarry_in`; for a
        six-node plan or a partitioned one with `dcarry` `rc6_in` `(2, NV)`,
        `x0_other`) and what it has left (`x0`, `b`, `nfc_out`; `kx`
        six-node; `r`, `partR`, `partB` where the front forms them;
        `kxs_cur`, `rcarry_out` in mode 2; `x0copy` with `dtail`), with the
        plan (`form` by name, `mode`, `use_pre`, `carry`, `dcarry`, `dtail`,
        `have_cells`), `rowmap` (`row0, len1, row2, len2` of this rank's rows,
        zeros when un-partitioned), `nsel` and `k_lpr`, `r1_lpr`, `r1_pair`
        (R1 is held in the pair format).
        What a plan does not have is None.  On a row-partitioned system every
        rank calls it together.  The stepper is consumed: `set_state` before
        it steps again."""
        NV, NP = self.sys.NV, self.sys.NP
        n, cap = NV + NP, 4096
        o = solve_opts() if opts is None else opts
        nan = lambda *shape: np.full(shape, np.nan)
        res = dict(ring=nan(5, n), nfc_in=nan(2, NV), g_in=nan(NV),
                   gp_in=nan(NP), b_prev=nan(n), kxs_in=nan(4, n),
                   rcarry_in=nan(NV), rc6_in=nan(2, NV), x0_other=nan(n),
                   x0=nan(n), b=nan(n), nfc_out=nan(NV), kx=nan(n), r=nan(n),
                   partR=nan(cap), partB=nan(cap), kxs_cur=nan(n),
                   rcarry_out=nan(NV), r_in=nan(n), x0copy=nan(n))
        pr = C.dns_imex_probe(parts_cap=cap)
        for k, arr in res.items():
            setattr(pr, k, C.dptr(arr.reshape(-1)))
        nf = None if nfc_new is None else C.as_f64(nfc_new, NV)
        C.check(self.lib.dns_imex_front_probe(
            self._h, ct.byref(cf), ct.byref(o), int(cycle_len), C.dptr(nf),
            ct.byref(pr)))
        for k in ('nsol', 'tab_row', 'mode', 'k_lpr', 'r1_lpr', 'nparts',
                  'nsel'):
            res[k] = int(getattr(pr, k))
        res['form'] = self.PROBE_FORMS[int(pr.form)]
        for k in ('use_pre', 'carry', 'r1_pair', 'dcarry', 'dtail',
                  'have_cells'):
            res[k] = bool(getattr(pr, k))
        res['rowmap'] = tuple(int(v) for v in pr.rowmap)
        res['partR'] = res['partR'][:pr.nparts]
        res['partB'] = res['partB'][:pr.nparts]
        if not pr.has_carry:
            res['kxs_in'] = res['rcarry_in'] = None
        if not pr.has_six:
            res['kx'] = None
        if not (pr.has_six or pr.dcarry):
            res['rc6_in'] = res['x0_other'] = None
        if pr.nparts == 0:
            res['r'] = res['partR'] = res['partB'] = None
        if pr.mode != 2:
            res['kxs_cur'] = res['rcarry_out'] = None
        if not pr.dtail:
            res['x0copy'] = None
        return res

    def step_counters(self):
        """`(built, tail_cells, cells_reused)` of the row-partitioned step
        (`dns_imex_step_counters`)"""
        buf = (ct.c_int64*3)()
        C.check(self.lib.dns_imex_step_counters(self._h, buf))
        return tuple(int(b) for b in buf)

    # ---- observer feedback (`dns_imex_set_feedback*`) ----------------------
    def set_feedback(self, cv_mat, b_mat, ha, hb, hc, c_n, c_c, dt):
        """closed loop with a linear observer on the device: before every step
        `y = cv_mat v_c`, `hx' = ha hx + hb y + drift` (AB2), `u = hc hx` and
        `dt*(c_n b_mat u_n + c_c b_mat u_c)` added to the right-hand side
        (`include/dns_amd.h`; CNAB `c_n = c_c = 1/2`, SBDF2 `2/3, 0`).  The
        observer state and the drift / log table follow through
        `set_feedback_state` and `set_feedback_table`."""
        ha = np.ascontiguousarray(ha, dtype=np.float64)
        hN = ha.shape[0]
        hb = np.ascontiguousarray(np.asarray(hb, dtype=np.float64)
                                  .reshape((hN, -1)))
        hc = np.ascontiguousarray(np.asarray(hc, dtype=np.float64)
                                  .reshape((-1, hN)))
        Ny, Nu = hb.shape[1], hc.shape[0]
        if ha.shape != (hN, hN):
            raise ValueError('ha must be square')
        cview, bview = C.CsrView(cv_mat), C.CsrView(b_mat)
        if cview.shape != (Ny, self.sys.NV) or bview.shape != (self.sys.NV, Nu):
            raise ValueError('cv_mat must be Ny x NV and b_mat NV x Nu')
        C.check(self.lib.dns_imex_set_feedback(
            self._h, cview.byref(), bview.byref(), C.dptr(ha.reshape(-1)),
            C.dptr(hb.reshape(-1)), C.dptr(hc.reshape(-1)), hN, Ny, Nu,
            float(c_n), float(c_c), float(dt)))
        self._fb_shape = (hN, Ny, Nu)

    def clear_feedback(self):
        C.check(self.lib.dns_imex_clear_feedback(self._h))
        self._fb_shape = None

    def set_feedback_state(self, hx, f_last, u_c):
        hN, _, Nu = self._fb_shape
        args = [C.as_f64(hx, hN), C.as_f64(f_last, hN), C.as_f64(u_c, Nu)]
        C.check(self.lib.dns_imex_set_feedback_state(
            self._h, *[C.dptr(a) for a in args]))

    def feedback_state(self):
        """`(hx, f_last, u_c)` of the current time"""
        hN, _, Nu = self._fb_shape
        hx, fl, uc = np.empty(hN), np.empty(hN), np.empty(Nu)
        C.check(self.lib.dns_imex_get_feedback_state(
            self._h, C.dptr(hx), C.dptr(fl), C.dptr(uc)))
        return hx, fl, uc

    def set_feedback_table(self, nsteps, drift=None):
        """room for `nsteps` steps: their drift rows `(nsteps, hN)` (None: no
        drift) and as many rows of the `y` / `u` logs; resets the step counter
        like `set_rhs_table` (call it after that one)"""
        hN = self._fb_shape[0]
        tab = None if drift is None else np.ascontiguousarray(
            drift, dtype=np.float64).reshape((int(nsteps), hN))
        C.check(self.lib.dns_imex_set_feedback_table(
            self._h, int(nsteps), C.dptr(None if tab is None
                                         else tab.reshape(-1))))

    def feedback_log(self, first=0, count=None):
        """`(y, u)`: rows `first .. first + count` of the logs -- what the
        steps since `set_feedback_table` measured and actuated (default: all
        steps taken since)"""
        _, Ny, Nu = self._fb_shape
        if count is None:
            count = self.table_position()[0] - first
        y, u = np.empty((count, Ny)), np.empty((count, Nu))
        C.check(self.lib.dns_imex_get_feedback_log(
            self._h, int(first), int(count), C.dptr(y.reshape(-1)),
            C.dptr(u.reshape(-1))))
        return y, u

    # ---- boundary feedback (`dns_imex_set_feedback_boundary`) ---------------
    def set_feedback_boundary(self, s_mat, base=None, col0=0, Ba=None,
                              Bm=None, Bj=None, wm=(0., 0., 0.),
                              wa=(0., 0., 0.)):
        """behind `set_feedback` (whose `b_mat` may be empty): the observer's
        output drives the controlled Dirichlet values, `b = base + s_mat u`
        (`s_mat`: `nc x Nu`), written by the device into the columns `col0 ..
        col0 + nc` of the NEXT row of the Dirichlet table of the attached
        convection operator (`ConvectionP2.set_dbc_table`, one row more than
        steps: row 0 holds the values of the current state).  `Ba`, `Bm` (`NV
        x Nu`), `Bj` (`NP x Nu`): what `applybcs` makes of the unit controls
        (all None: the literal zero); `wm`, `wa`: the scheme's weights of
        `Bm u_j`, `Ba u_j` for `j = n, c, p` (`include/dns_amd.h`).  State
        and table follow: `set_feedback_state(.., u_p=)`,
        `set_feedback_table`."""
        _, _, Nu = self._fb_shape
        sview = C.CsrView(s_mat)
        if sview.shape[1] != Nu:
            raise ValueError('s_mat must be nc x Nu')
        nc = sview.shape[0]
        mats = (Ba, Bm, Bj)
        if any(m is None for m in mats) and not all(m is None for m in mats):
            raise ValueError('Ba, Bm and Bj come together')
        views = [None if m is None else C.CsrView(m) for m in mats]
        base = None if base is None else C.as_f64(base, nc)
        wm, wa = C.as_f64(wm, 3), C.as_f64(wa, 3)
        C.check(self.lib.dns_imex_set_feedback_boundary(
            self._h, sview.byref(), C.dptr(base), int(col0),
            *[None if v is None else v.byref() for v in views],
            C.dptr(wm), C.dptr(wa)))
        self._fb_nc = nc

    def set_feedback_state_bc(self, hx, f_last, u_c, u_p):
        hN, _, Nu = self._fb_shape
        args = [C.as_f64(hx, hN), C.as_f64(f_last, hN), C.as_f64(u_c, Nu),
                C.as_f64(u_p, Nu)]
        C.check(self.lib.dns_imex_set_feedback_state_bc(
            self._h, *[C.dptr(a) for a in args]))

    def feedback_state_bc(self):
        """`(hx, f_last, u_c, u_p)` of the current time"""
        hN, _, Nu = self._fb_shape
        out = np.empty(hN), np.empty(hN), np.empty(Nu), np.empty(Nu)
        C.check(self.lib.dns_imex_get_feedback_state_bc(
            self._h, *[C.dptr(a) for a in out]))
        return out

    def feedback_bcs(self, first=0, count=None):
        """rows `first .. first + count` of the controlled columns of the
        Dirichlet table as the device filled them (`count x nc`; default: row
        0 up to the row of the current state).  Row `s + 1` holds the values
        of the state step `s` left"""
        if count is None:
            count = self.table_position()[0] + 1 - first
        out = np.empty((int(count), self._fb_nc))
        C.check(self.lib.dns_imex_get_feedback_bcs(
            self._h, int(first), int(count), C.dptr(out.reshape(-1))))
        return out

    def feedback_rhs(self, velocity=True, pressure=True):
        """`(geff, gpeff)` the last step read (None where not asked for)"""
        geff = np.empty(self.sys.NV) if velocity else None
        gpeff = np.empty(self.sys.NP) if pressure else None
        C.check(self.lib.dns_imex_get_feedback_rhs(self._h, C.dptr(geff),
                                                   C.dptr(gpeff)))
        return geff, gpeff

    # ---- trajectory recorder (`dns_imex_set_recorder`) ----------------------
    def set_recorder(self, nrows, cv_mat=None, snap_slots=None):
        """the next `nrows` steps (`step` and `run` alike) write themselves
        down on the device: the outputs `y = cv_mat v` of every step
        (`cv_mat`: `Ny x NV`, None: no outputs) and / or the state `[v; p]` of
        the steps `s` with `snap_slots[s] >= 0` into that slot of a snapshot
        buffer (`snap_slots`: `nrows` integers, `-1`: not kept, None: no
        snapshots; `'all'`: every step, slot `s`).  Row `s` is what `get_state`
        would have returned after the `(s+1)`-th step from now.  Resets the
        step counter like `set_rhs_table` (call it after that one, and collect
        with `record_outputs` / `record_snapshots` before the next tables)."""
        nrows = int(nrows)
        if nrows < 1:
            raise ValueError('`nrows` must be positive')
        if cv_mat is None and snap_slots is None:
            raise ValueError('neither `cv_mat` nor `snap_slots`: nothing to '
                             'record')
        cview = None
        if cv_mat is not None:
            cview = C.CsrView(cv_mat)
            if len(cview.shape) != 2 or cview.shape[1] != self.sys.NV \
                    or cview.shape[0] < 1:
                raise ValueError('cv_mat must be Ny x NV (NV = {0}), it is '
                                 '{1}'.format(self.sys.NV, cview.shape))
        slots, nslots = None, 0
        if snap_slots is not None:
            if isinstance(snap_slots, str):
                if snap_slots != 'all':
                    raise ValueError("snap_slots: an array or 'all'")
                snap_slots = np.arange(nrows)
            slots = np.ascontiguousarray(snap_slots, dtype=np.int32).reshape(-1)
            if slots.size != nrows:
                raise ValueError('snap_slots must have `nrows` entries')
            if slots.min() < -1:
                raise ValueError('snap_slots: entries are slots or -1')
            nslots = int(slots.max()) + 1
            if nslots < 1:
                raise ValueError('snap_slots keeps no step at all')
        C.check(self.lib.dns_imex_set_recorder(
            self._h, None if cview is None else cview.byref(), nrows,
            None if slots is None else slots.ctypes.data_as(C.c_int32_p),
            nslots))
        self._rec_shape = (nrows, 0 if cview is None else cview.shape[0],
                           nslots)

    def clear_recorder(self):
        C.check(self.lib.dns_imex_clear_recorder(self._h))
        self._rec_shape = None

    def _rec_need(self):
        shape = getattr(self, '_rec_shape', None)
        if shape is None:
            raise ValueError('no recorder is set (`set_recorder`)')
        return shape

    def record_outputs(self, first=0, count=None):
        """rows `first .. first + count` of `y = cv_mat v` (default: of all
        steps taken since `set_recorder`), `(count, Ny)`"""
        _, Ny, _ = self._rec_need()
        if count is None:
            count = self.table_position()[0] - first
        y = np.empty((int(count), Ny))
        C.check(self.lib.dns_imex_get_record_outputs(
            self._h, int(first), int(count), C.dptr(y.reshape(-1))))
        return y

    def record_snapshots(self, first=0, count=None):
        """slots `first .. first + count` of the snapshot buffer (default: all
        slots): `(v (count, NV), p (count, NP))`"""
        _, _, nslots = self._rec_need()
        if count is None:
            count = nslots - first
        v = np.empty((int(count), self.sys.NV))
        p = np.empty((int(count), self.sys.NP))
        C.check(self.lib.dns_imex_get_record_snapshots(
            self._h, int(first), int(count), C.dptr(v.reshape(-1)),
            C.dptr(p.reshape(-1))))
        return v, p

    # ---- what functionals and quadratics share ------------------------------
    @staticmethod
    def _dbc_source(dbc_table, nrows, ndbc=None):
        """`(live, table)` of a `dbc_table` argument: None (constant values),
        `'operator'` (live: the convection operator's table) or the rows,
        `nrows + 1` of them (`ndbc` wide where it is given)"""
        if dbc_table is None:
            return False, None
        if isinstance(dbc_table, str):
            if dbc_table != 'operator':
                raise ValueError('`dbc_table`: a table or the string '
                                 '\'operator\', not {0!r}'.format(dbc_table))
            return True, None
        tab = np.ascontiguousarray(dbc_table, dtype=np.float64)
        if ndbc is None and (tab.ndim != 2 or tab.shape[0] != nrows + 1):
            raise ValueError('`dbc_table` must have nrows + 1 = {0} rows, '
                             'it is {1}'.format(nrows + 1, tab.shape))
        if ndbc is not None and tab.shape != (nrows + 1, ndbc):
            raise ValueError(
                '`dbc_table` must be (nrows + 1) x ndbc = {0} x {1}, it '
                'is {2}'.format(nrows + 1, ndbc, tab.shape))
        return False, tab

    def _set_log(self, setter, head, live, tab, ndbc):
        """the export `setter` for constant values, or its `_bc` / `_live`
        form (`_dbc_source`), on the arguments `head` all three share"""
        if live:
            C.check(getattr(self.lib, setter + '_live')(*head, ndbc))
        elif tab is not None:
            C.check(getattr(self.lib, setter + '_bc')(
                *head, ndbc, C.dptr(tab.reshape(-1))))
        else:
            C.check(getattr(self.lib, setter)(*head))

    def _log_rows(self, shape_attr, unset, getter, first, count):
        """rows `first .. first + count` of a log `(nrows, n)` through the
        export `getter` (default: of all steps taken since it was set)"""
        shape = getattr(self, shape_attr, None)
        if shape is None:
            raise ValueError(unset)
        if count is None:
            count = self.table_position()[0] - first
        out = np.empty((int(count), shape[1]))
        C.check(getattr(self.lib, getter)(
            self._h, int(first), int(count),
            C.dptr(out.reshape(-1) if out.size else np.zeros(1))))
        return out

    # ---- force functionals (`dns_imex_set_functionals`) ---------------------
    def set_functionals(self, fn, nrows, dt, dbc_table=None):
        """the next `nrows` steps (`step` and `run` alike) evaluate the
        momentum-balance functionals `fn` (`fem.MomentumFunctionals`: drag,
        lift, pressure differences, ...; at most 16) of the state they leave,
        on the device, into a log of `nrows` rows; `dt`: the time step of the
        backward difference `(v - v_prev)/dt`.  Row `s` is `fn.evaluate` of
        what `get_state` would have returned after the `(s+1)`-th step from
        now and the state before it.  Resets the step counter like
        `set_rhs_table` (call it after that one, and collect with
        `get_functionals` before the next tables).  Functionals with cells
        need the convection operator attached (`set_convection`) with
        constant Dirichlet values; their cells refer to that operator, so
        after attaching another one they are set again.

        `dbc_table` (`(nrows + 1, ndbc)`): Dirichlet values that change from
        step to step, in the order of the operator's `dbcinds` (static first,
        controlled behind them).  Row `j` holds the values of the state
        BEFORE the `j`-th step from now, row `nrows` those of the state after
        the last one; row `s` of the log is then `fn.evaluate(..., dbc=
        dbc_table[s + 1], dbc_prev=dbc_table[s])`
        (`dns_imex_set_functionals_bc`).  The table is the functionals' own:
        the operator's (`set_dbc_table`) keeps its meaning and length.

        `dbc_table='operator'`: no table of their own -- the values are read
        from the table of the attached convection operator (`conv.
        set_dbc_table`, at least `nrows + 1` rows of the functionals' width,
        the same row convention), which a resident `BoundaryFeedback` writes
        step by step (`dns_imex_set_functionals_live`)."""
        nrows = int(nrows)
        if nrows < 1:
            raise ValueError('`nrows` must be positive')
        moving = dbc_table is not None
        live, tab = self._dbc_source(dbc_table, nrows)
        args = fn.device_args(moving=True) if moving else fn.device_args()
        nF = int(args['scale'].size)
        terms = [('ca', self.sys.NV), ('cm', self.sys.NV), ('cp', self.sys.NP)]
        if moving:
            ndbc = int(args['cab'].shape[1] if live else tab.shape[1])
            terms += [('cab', ndbc), ('cmb', ndbc)]
        views = []
        for name, ncol in terms:
            mat = args[name]
            if mat.nnz == 0 and mat.shape[1] != ncol:
                views.append(None)           # (pressure-only functionals)
                continue
            if mat.shape != (nF, ncol):
                raise ValueError('{0} must be {1} x {2}, it is {3}'.format(
                    name, nF, ncol, mat.shape))
            views.append(C.CsrView(mat))
        cptr = np.ascontiguousarray(args['cell_ptr'], dtype=np.int32)
        cidx = np.ascontiguousarray(args['cell_idx'], dtype=np.int32)
        cw = C.as_f64(args['cell_w']) if args['cell_w'].size else np.zeros(1)
        if cidx.size == 0:
            cidx = np.zeros(1, dtype=np.int32)
        c0, scale = C.as_f64(args['c0'], nF), C.as_f64(args['scale'], nF)
        refs = [None if v is None else v.byref() for v in views]
        tail = (C.dptr(c0), C.dptr(scale), cptr.ctypes.data_as(C.c_int32_p),
                cidx.ctypes.data_as(C.c_int32_p), C.dptr(cw), float(dt), nrows)
        self._set_log('dns_imex_set_functionals', (self._h, nF, *refs, *tail),
                      live, tab, ndbc if moving else 0)
        self._fn_shape = (nrows, nF)

    def clear_functionals(self):
        C.check(self.lib.dns_imex_clear_functionals(self._h))
        self._fn_shape = None

    def get_functionals(self, first=0, count=None):
        """rows `first .. first + count` of the functionals' log (default: of
        all steps taken since `set_functionals`), `(count, nF)`"""
        return self._log_rows('_fn_shape', 'no functionals are set '
                              '(`set_functionals`)',
                              'dns_imex_get_functionals', first, count)

    # ---- flow statistics (`dns_imex_set_stats`) ------------------------------
    def set_statistics(self, bins, nbins=None, pairs=None, reset=False):
        """the next `len(bins)` steps (`step` and `run` alike) add the state
        `x = [v; p]` they leave to running sums on the device: the step `s`
        from now goes into bin `bins[s]` (`-1`: skipped; `nbins`: at most 256,
        default `max(bins) + 1`), `N += 1`, `S1 += x`, `S2 += x**2` and, for
        the index pairs `pairs` (`(npairs, 2)` into `[0, NV + NP)`),
        `SX += x[i]*x[j]` (`fem.FlowStatistics` makes means, variances and
        covariances of them).  The sums go on across calls with the same
        `nbins` and `pairs` unless `reset`: the slices of a time loop set
        their bins and keep summing; collect with `statistics()`.  Resets the
        step counter like `set_rhs_table` (call it after that one)."""
        bins = np.asarray(bins)
        if bins.ndim != 1 or bins.size < 1:
            raise ValueError('`bins`: one entry per step, at least one')
        if not np.issubdtype(bins.dtype, np.integer):
            raise ValueError('`bins` must be integers')
        if nbins is None:
            nbins = max(int(bins.max()) + 1, 1)
        nbins = int(nbins)
        if not 1 <= nbins <= 256:
            raise ValueError('`nbins` = {0} outside 1..256'.format(nbins))
        if bins.min() < -1 or bins.max() >= nbins:
            raise ValueError('`bins`: entries are bins below `nbins` = {0} '
                             'or -1'.format(nbins))
        bins = np.ascontiguousarray(bins, dtype=np.int32)
        n = self.sys.NV + self.sys.NP
        pr = np.zeros((0, 2), dtype=np.int32) if pairs is None else \
            np.asarray(pairs)
        if pr.size and not np.issubdtype(pr.dtype, np.integer):
            raise ValueError('`pairs` must be integers')
        if pr.size == 0:
            pr = np.zeros((0, 2), dtype=np.int32)
        if pr.ndim != 2 or pr.shape[1] != 2:
            raise ValueError('`pairs` must be npairs x 2, it is {0}'.format(
                pr.shape))
        if pr.size and (pr.min() < 0 or pr.max() >= n):
            raise ValueError('`pairs`: indices into [0, NV + NP) = [0, {0})'
                             .format(n))
        pi = np.ascontiguousarray(pr[:, 0], dtype=np.int32)
        pj = np.ascontiguousarray(pr[:, 1], dtype=np.int32)
        npairs = int(pi.size)
        C.check(self.lib.dns_imex_set_stats(
            self._h, int(bins.size), bins.ctypes.data_as(C.c_int32_p), nbins,
            npairs, pi.ctypes.data_as(C.c_int32_p) if npairs else None,
            pj.ctypes.data_as(C.c_int32_p) if npairs else None,
            int(bool(reset))))
        self._st_shape = (nbins, npairs)

    def clear_statistics(self):
        C.check(self.lib.dns_imex_clear_stats(self._h))
        self._st_shape = None

    def statistics(self):
        """the sums since they were last zeroed, a dict: `counts` `(nbins,)`
        (integers), `s1_v`, `s2_v` `(nbins, NV)`, `s1_p`, `s2_p` `(nbins, NP)`
        and `sx` `(nbins, npairs)`"""
        shape = getattr(self, '_st_shape', None)
        if shape is None:
            raise ValueError('no statistics are set (`set_statistics`)')
        nbins, npairs = shape
        NV, NP = self.sys.NV, self.sys.NP
        cnt = np.empty(nbins)
        s1, s2 = np.empty((nbins, NV + NP)), np.empty((nbins, NV + NP))
        sx = np.empty((nbins, npairs))
        C.check(self.lib.dns_imex_get_stats(
            self._h, 0, nbins, C.dptr(cnt), C.dptr(s1.reshape(-1)),
            C.dptr(s2.reshape(-1)),
            C.dptr(sx.reshape(-1)) if npairs else None))
        return dict(counts=np.rint(cnt).astype(np.int64),
                    s1_v=s1[:, :NV].copy(), s1_p=s1[:, NV:].copy(),
                    s2_v=s2[:, :NV].copy(), s2_p=s2[:, NV:].copy(), sx=sx)

    # ---- quadratic functionals (`dns_imex_set_quadratics`) ------------------
    def set_quadratics(self, qf, nrows, dt, max_grid=None, dbc_table=None):
        """the next `nrows` steps (`step` and `run` alike) evaluate the
        quadratic forms `qf` (`fem.QuadraticFunctionals`: kinetic energy,
        dissipation rate, `u^T M du/dt`, the M-norm of `du/dt`, ...; at most 8
        forms over at most 4 matrices) of the state they leave, on the device,
        into a log of `nrows` rows; `dt`: the time step of the difference
        `w = v - v_prev`.  Row `s` is `qf.evaluate` of what `get_state` would
        have returned after the `(s+1)`-th step from now and the state before
        it.  Resets the step counter like `set_rhs_table` (call it after that
        one, and collect with `get_quadratics` before the next tables).  The
        log takes `nrows x G x nQ` doubles, `G` the workgroups of the kernel
        (at most 256): `max_grid` caps it lower.  Matrices the device holds
        already are not uploaded again.

        Forms with moving Dirichlet values (`qf.ndbc > 0`: the builders'
        `moving=True`) need `dbc_table` (`(nrows + 1, ndbc)`): row `j` holds
        the values of the state BEFORE the `j`-th step from now, row `nrows`
        those of the state after the last one; row `s` of the log is then
        `qf.evaluate(..., dbc=dbc_table[s + 1], dbc_prev=dbc_table[s])`
        (`dns_imex_set_quadratics_bc`; the table is the quadratics' own).
        `dbc_table='operator'`: the values are read from the table of the
        attached convection operator instead, which a resident
        `BoundaryFeedback` writes step by step
        (`dns_imex_set_quadratics_live`)."""
        nrows = int(nrows)
        if nrows < 1:
            raise ValueError('`nrows` must be positive')
        args = qf.device_args()
        ndbc = int(args.get('ndbc', 0))
        if ndbc > 0 and dbc_table is None:
            raise ValueError(
                'quadratics with moving Dirichlet values (ndbc = {0}) need '
                '`dbc_table`: the rows of values or \'operator\''.format(ndbc))
        if ndbc == 0 and dbc_table is not None:
            raise ValueError(
                '`dbc_table` with quadratics that carry constant Dirichlet '
                'values (ndbc = 0): build them with `moving=True`')
        live, tab = self._dbc_source(dbc_table, nrows, ndbc)
        NV = self.sys.NV + ndbc
        nQ = int(args['scale'].size)
        mats = args['mats']
        for m, mat in enumerate(mats):
            if mat.shape != (NV, NV):
                raise ValueError('matrix {0} must be NV x NV (NV = {1}), it '
                                 'is {2}'.format(m, NV, mat.shape))
        views = [C.CsrView(mat) for mat in mats]
        structs = (C.dns_csr*len(views))(*[v.struct for v in views])
        lin = []
        for name in ('qa', 'qw'):
            mat = args[name]
            if mat is None or mat.nnz == 0:
                lin.append(None)
                continue
            if mat.shape != (nQ, NV):
                raise ValueError('{0} must be nQ x NV = {1} x {2}, it is '
                                 '{3}'.format(name, nQ, NV, mat.shape))
            lin.append(C.CsrView(mat))
        forms = [np.ascontiguousarray(args[k], dtype=np.int32)
                 for k in ('mat', 'lop', 'rop')]
        c0, scale = C.as_f64(args['c0'], nQ), C.as_f64(args['scale'], nQ)
        head = (self._h, len(views), structs, nQ,
                *[f.ctypes.data_as(C.c_int32_p) for f in forms],
                *[None if v is None else v.byref() for v in lin],
                C.dptr(c0), C.dptr(scale), float(dt), nrows,
                0 if max_grid is None else int(max_grid))
        self._set_log('dns_imex_set_quadratics', head, live, tab, ndbc)
        self._qd_shape = (nrows, nQ)

    def clear_quadratics(self):
        C.check(self.lib.dns_imex_clear_quadratics(self._h))
        self._qd_shape = None

    def quadratics_grid(self):
        """`G`, the workgroups of the kernel: the log on the device holds
        `nrows x G x nQ` doubles"""
        g = ct.c_int32(0)
        C.check(self.lib.dns_imex_quadratics_grid(self._h, ct.byref(g)))
        return g.value

    def get_quadratics(self, first=0, count=None):
        """rows `first .. first + count` of the quadratics' log (default: of
        all steps taken since `set_quadratics`), `(count, nQ)`"""
        return self._log_rows('_qd_shape', 'no quadratics are set '
                              '(`set_quadratics`)',
                              'dns_imex_get_quadratics', first, count)

    # ---- snapshot ensemble (`dns_imex_set_ensemble`) -------------------------
    def set_ensemble(self, slots, nslots=None, reset=False):
        """the next `len(slots)` steps (`step` and `run` alike) copy the
        velocity they leave into slot `slots[s]` of an ensemble of `nslots`
        snapshots on the device (`-1`: the step is not kept; default `nslots`:
        `max(slots) + 1`) -- the snapshots of a POD (`fem.SnapshotPOD`).  The
        ensemble is kept across calls with the same `nslots` unless `reset`:
        the slices of a time loop set their slot tables and go on filling;
        `ensemble_gram` and `ensemble_combine` work on it behind the loop.
        Resets the step counter like `set_rhs_table` (call it after that
        one)."""
        slots = np.asarray(slots)
        if slots.ndim != 1 or slots.size < 1:
            raise ValueError('`slots`: one entry per step, at least one')
        if not np.issubdtype(slots.dtype, np.integer):
            raise ValueError('`slots` must be integers')
        if nslots is None:
            nslots = max(int(slots.max()) + 1, 1)
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        C.check(self.lib.dns_imex_set_ensemble(
            self._h, int(slots.size), slots.ctypes.data_as(C.c_int32_p),
            int(nslots), int(bool(reset))))
        self._ens_slots = int(nslots)

    def clear_ensemble(self):
        C.check(self.lib.dns_imex_clear_ensemble(self._h))
        self._ens_slots = None

    def _ens_m(self, m):
        nslots = getattr(self, '_ens_slots', None)
        if nslots is None:
            raise ValueError('no ensemble is set (`set_ensemble`)')
        return nslots if m is None else int(m)

    def ensemble(self, first=0, count=None):
        """slots `first .. first + count` of the ensemble (default: all),
        `(count, NV)`"""
        count = self._ens_m(None) - first if count is None else int(count)
        out = np.empty((count, self.sys.NV))
        C.check(self.lib.dns_imex_get_ensemble(
            self._h, int(first), count,
            C.dptr(out.reshape(-1) if out.size else np.zeros(1))))
        return out

    def ensemble_to_base(self, conv, times=None, first=0, count=None,
                         dbcvals=None, adjoint=False, time_map=None,
                         interpolate=False):
        """slots `first .. first + count` of the ensemble (default: all from
        `first` on) become the base trajectory of the linearised operator
        `conv` (`ConvectionP2.set_base_flow` of a `BaseTrajectory`), device to
        device: the forward run that filled the slots and the linearised or
        adjoint run about them never meet on the host.  `dbcvals`: the base
        flow's Dirichlet values, `(ndbc,)` or `(count, ndbc)` -- the only
        thing that crosses the bus.  With `times` (one per slot, ascending;
        `time_map` as in `BaseTrajectory`) the operator gets the trajectory's
        clock as well, so that `cnab` / `sbdftwo` arm its rows; without, name
        them with `conv.set_base_rows` / `set_base_row`.  `interpolate`: as in
        `BaseTrajectory`, the loops arm weights beside the rows (slots kept
        `every=k` then stand for a flow that moves every step).  Refused by name
        (`ValueError`): no ensemble, slots out of range, another device,
        another number of inner dofs"""
        from .convection import BaseTrajectory
        nslots = getattr(self, '_ens_slots', None)
        if count is None:
            count = (nslots if nslots is not None else 0) - int(first)
        count = int(count)
        traj = BaseTrajectory(np.arange(count) if times is None else times,
                              None, dbcvals, time_map=time_map,
                              interpolate=interpolate) \
            if count >= 1 else None
        if traj is not None and traj.nrows != count:
            raise ValueError('base trajectory: {0} `times` for {1} slots'
                             .format(traj.nrows, count))
        sets, dflat = (1, np.zeros(1)) if traj is None else \
            traj.resolve_dbcvals(conv.ndbc)
        C.check(self.lib.dns_imex_ensemble_to_base(
            self._h, int(first), count, conv._h, int(sets), C.dptr(dflat),
            int(bool(adjoint))))
        conv.base_trajectory = traj if times is not None else None

    def ensemble_gram(self, W=None, m=None):
        """`G = E W E^T` of the first `m` slots (default: all), `(m, m)`,
        exactly symmetric; `W`: symmetric NV x NV (None: the identity).  Runs
        on the device (fp64 matrix cores), `m^2` doubles come back."""
        m = self._ens_m(m)
        view = None if W is None else C.CsrView(W)
        out = np.empty((m, m))
        C.check(self.lib.dns_imex_ensemble_gram(
            self._h, None if view is None else view.byref(), m,
            C.dptr(out.reshape(-1))))
        return out

    def ensemble_combine(self, coef, m=None):
        """`coef @ E` for the first `m` slots: `coef` `(r, m)`, returns `(r,
        NV)` -- per entry `acc = fma(coef[q, s], E[s, k], acc)`, `s`
        ascending"""
        coef = np.ascontiguousarray(np.atleast_2d(coef), dtype=np.float64)
        m = self._ens_m(coef.shape[1] if m is None else m)
        if coef.shape[1] != m or coef.shape[0] < 1:
            raise ValueError('`coef` must be r x m = r x {0}, it is {1}'
                             .format(m, coef.shape))
        out = np.empty((coef.shape[0], self.sys.NV))
        C.check(self.lib.dns_imex_ensemble_combine(
            self._h, m, coef.shape[0], C.dptr(coef.reshape(-1)),
            C.dptr(out.reshape(-1))))
        return out

    def get_state(self):
        v = np.empty(self.sys.NV)
        p = np.empty(self.sys.NP)
        C.check(self.lib.dns_imex_get_state(self._h, C.dptr(v), C.dptr(p)))
        return v.reshape((-1, 1)), p.reshape((-1, 1))

    def vnorm(self):
        out = ct.c_double(0.)
        C.check(self.lib.dns_imex_vnorm(self._h, ct.byref(out)))
        return out.value


def choose_schur(system, F, J, schur='auto', prolongations=None,
                 dense_max=6000):
    """the Schur block of a drop-in's system: `'auto'` = the dense inverse up
    to `dense_max` pressure dofs, beyond it the multigrid block -- on the
    caller's nested pressure spaces (`prolongations`) or, for a mesh that
    comes with none, on a hierarchy built from `F` and `J` alone
    (`amg.algebraic_prolongations`; `'amg'` asks for it by name).  Returns
    the `schur=` keyword for `setup_precond` (the prolongations are attached
    here); what was built is left in `system.schur_hierarchy`."""
    NP = J.shape[0]
    system.schur_hierarchy = None
    if prolongations is not None and schur in ('auto', 'mg'):
        system.set_schur_mg(prolongations)
        system.schur_hierarchy = dict(kind='geometric',
                                      levels=[NP] + [P.shape[1]
                                                     for P in prolongations])
        return 'mg'
    if schur == 'auto' and NP <= dense_max:
        return 'dense'
    if schur in ('auto', 'amg'):
        from . import amg
        info = dict(kind='algebraic')
        prols = amg.algebraic_prolongations(F, J, info=info,
                                            coarsest=min(1500, dense_max))
        if not prols:
            return 'dense' if NP <= 4*dense_max else 'jacobi'
        system.set_schur_mg(prols)
        system.schur_hierarchy = info
        return 'mg'
    return schur


def streaming_precond_defaults(n):
    """degree and drop tolerance of the explicit polynomial `Fh^-1` for a
    system of `n` unknowns.  Where the step is bandwidth bound the polynomial
    matrix `Gc` is the largest stream of a Krylov step (3.6 x the non-zeros of
    `K` at degree 8, drop 1e-3): a HIGHER degree with a LARGER drop tolerance
    keeps the Krylov-step count and cuts the stream -- measured on the refined
    wake (profiles/r04_gc_pareto/table.txt): n = 173k 3651 -> 4039 steps/s,
    n = 693k 1301 -> 1595, n = 2.78M 308 -> 431.  At the reference sizes (cache
    resident, ONE Krylov step per time step) degree 6 / 1e-3 stays.

    `extrapolate`: order of the warm start.  With the multigrid Schur block a
    solve runs the two columns of its cycle whatever its residual (oversolve,
    `solver.hpp`); what the next start residual then consists of is the final
    residuals of the last solves times the warm start's coefficients, and the
    cubic's (sum |c| = 15) keep a two-column cycle contracting where the
    quartic's (31) do not: n = 173k 4175 -> 4490 steps/s, n = 693k 1434 ->
    1870, n = 2.78M 465 -> 604 (profiles/r05_oversolve/)."""
    if n >= 100000:
        return dict(cheb_degree=8, drop_tol=7e-3, extrapolate=3)
    return dict(cheb_degree=6, drop_tol=1e-3, extrapolate=4)


# ---- standalone kernels ---------------------------------------------------
def spmv(A, x, y=None, alpha=1., beta=0., variant='vector', device=0):
    lib = C.load_library()
    view = C.CsrView(A)
    x = C.as_f64(x, size=view.shape[1])
    out = np.zeros(view.shape[0]) if y is None else C.as_f64(y).copy()
    C.check(lib.dns_spmv(device, view.byref(), C.dptr(x), C.dptr(out),
                         float(alpha), float(beta),
                         _VARIANTS.get(variant, variant)))
    return out


def ensemble_gram(E, W=None, nv=None, device=0):
    """`G = E[:, :nv] W E[:, :nv]^T` through `dns_ensemble_gram` (the kernels
    of `ImexStepper.ensemble_gram` alone): `E` is `m x ld`, `ld` even, its
    columns from `nv` on are never read"""
    lib = C.load_library()
    E = np.ascontiguousarray(E, dtype=np.float64)
    m, ld = E.shape
    nv = ld if nv is None else int(nv)
    view = None if W is None else C.CsrView(W)
    out = np.empty((m, m))
    C.check(lib.dns_ensemble_gram(device, m, nv, ld, C.dptr(E.reshape(-1)),
                                  None if view is None else view.byref(),
                                  C.dptr(out.reshape(-1))))
    return out


def ensemble_project(X, Y=None, W=None, nv=None, device=0):
    """`P = X[:, :nv] W Y[:, :nv]^T`, `P[i, j] = x_i . (W y_j)`, through
    `dns_ensemble_project`: `X` is `mx x ld`, `Y` `my x ld` (`None`: `Y = X`),
    `ld` even, `W` any `nv x nv` matrix or `None` for the identity"""
    lib = C.load_library()
    X = np.ascontiguousarray(np.atleast_2d(X), dtype=np.float64)
    mx, ld = X.shape
    if Y is not None:
        Y = np.ascontiguousarray(np.atleast_2d(Y), dtype=np.float64)
        if Y.shape[1] != ld:
            raise ValueError('`Y` must have the {0} columns of `X`, it is '
                             '{1}'.format(ld, Y.shape))
    my = mx if Y is None else Y.shape[0]
    nv = ld if nv is None else int(nv)
    view = None if W is None else C.CsrView(W)
    out = np.empty((mx, my))
    C.check(lib.dns_ensemble_project(
        device, mx, my, nv, ld, C.dptr(X.reshape(-1)),
        None if Y is None else C.dptr(Y.reshape(-1)),
        None if view is None else view.byref(), C.dptr(out.reshape(-1))))
    return out


def ensemble_combine(E, coef, nv=None, device=0):
    """`coef @ E[:, :nv]` through `dns_ensemble_combine`: `coef` is `r x m`"""
    lib = C.load_library()
    E = np.ascontiguousarray(E, dtype=np.float64)
    coef = np.ascontiguousarray(np.atleast_2d(coef), dtype=np.float64)
    m, ld = E.shape
    nv = ld if nv is None else int(nv)
    if coef.shape[1] != m:
        raise ValueError('`coef` must be r x {0}, it is {1}'.format(
            m, coef.shape))
    out = np.empty((coef.shape[0], nv))
    C.check(lib.dns_ensemble_combine(device, m, nv, ld, C.dptr(E.reshape(-1)),
                                     coef.shape[0], C.dptr(coef.reshape(-1)),
                                     C.dptr(out.reshape(-1))))
    return out


def spmv_pair(K, nv, x, reps=0, warmup=1, device=0):
    """`y = K x` through the pair format (`dns_spmv_pair`); with `reps > 0`
    returns `(y, seconds_per_launch, format_bytes)`"""
    lib = C.load_library()
    view = C.CsrView(K)
    x = C.as_f64(x, size=view.shape[1])
    out = np.zeros(view.shape[0])
    secs, fb = ct.c_double(0.), ct.c_int64(0)
    C.check(lib.dns_spmv_pair(device, view.byref(), int(nv), C.dptr(x),
                              C.dptr(out), int(reps), int(warmup),
                              ct.byref(secs), ct.byref(fb)))
    if reps > 0:
        return out, secs.value, fb.value
    return out


def spmv_epilogue(A, x, y0, kernel='stream', nv=0, fp32_vals=False,
                  alpha=1., beta=0., b=None, x2=None, nsplit=0, mode='plain',
                  dinv=None, xin=None, omega=1., V=None, nvec=0, ld=None,
                  with_ww=False, with_bb=False, part=None, part_bb=None,
                  rowmap=None, pair_block=None, grid_cap=65535, guard=None,
                  device=0):
    """ONE launch of the streaming kernel with epilogues (`kernel='stream'`)
    or of the pair kernel (`'pair'`, `nv` velocity dofs) through
    `dns_spmv_epilogue` -- tests of the epilogues in isolation.

    `y0`: initial contents of `y` (global length); `part` / `part_bb`: the
    caller's pre-filled partials arrays (`part` turns the fused dots on), both
    returned as the device left them.  `V`: `nvec` rows of `ld` entries;
    `rowmap = (row0, len1, row2, len2)`; `pair_block = (nvl, v0, p0)`;
    `guard`: value of a device flag (None: no flag).  Returns
    `dict(y, part, part_bb, nparts, nblocks)`."""
    lib = C.load_library()
    view = C.CsrView(A)
    f64 = lambda v: None if v is None else C.as_f64(v)
    split = x2 is not None
    x = C.as_f64(x, size=int(nsplit) if split else view.shape[1])
    x2 = None if not split else C.as_f64(x2, size=view.shape[1] - int(nsplit))
    y = C.as_f64(y0).copy()
    ny = y.size
    b, dinv, xin = f64(b), f64(dinv), f64(xin)
    for v in (b, dinv, xin):
        if v is not None and v.size != ny:
            raise ValueError('b, dinv and xin hold one entry per row of y')
    e = C.dns_spmv_epi()
    e.kernel = {'stream': 0, 'pair': 1}[kernel]
    e.nv = int(nv)
    e.fp32_vals = int(bool(fp32_vals))
    e.mode = {'plain': 0, 'sweep': 1, 'add_cb': 2}[mode]
    e.alpha, e.beta, e.omega = float(alpha), float(beta), float(omega)
    e.b, e.x2, e.dinv, e.xin = C.dptr(b), C.dptr(x2), C.dptr(dinv), C.dptr(xin)
    e.nsplit = int(nsplit)
    e.nvec = int(nvec)
    e.ld = ny if ld is None else int(ld)
    if V is not None:
        V = C.as_f64(V)
        if V.size != e.ld * e.nvec:
            raise ValueError('V holds nvec rows of ld entries')
    e.V = C.dptr(V)
    e.ny = ny
    e.with_ww, e.with_bb = int(bool(with_ww)), int(bool(with_bb))
    part = None if part is None else C.as_f64(part).copy()
    part_bb = None if part_bb is None else C.as_f64(part_bb).copy()
    e.part_len = 0 if part is None else part.size
    e.part_bb_len = 0 if part_bb is None else part_bb.size
    if rowmap is not None:
        e.map_on = 1
        e.row0, e.len1, e.row2, e.len2 = [int(v) for v in rowmap]
    e.nvl = -1
    if pair_block is not None:
        e.nvl, e.v0, e.p0 = [int(v) for v in pair_block]
    e.grid_cap = int(grid_cap)
    e.use_guard = int(guard is not None)
    e.guard = int(guard or 0)
    nparts, nblocks = ct.c_int32(0), ct.c_int32(0)
    C.check(lib.dns_spmv_epilogue(device, view.byref(), ct.byref(e), C.dptr(x),
                                  C.dptr(y), C.dptr(part), C.dptr(part_bb),
                                  ct.byref(nparts), ct.byref(nblocks)))
    return dict(y=y, part=part, part_bb=part_bb, nparts=nparts.value,
                nblocks=nblocks.value)


def row_kernel_probe(kernel, A=None, x=None, lpr=32, fp32_vals=False, x2=None,
                     R1=None, cells=None, v_p=None, cellvals=None, a_c=1.,
                     a_p=0., device=0):
    """TEST ONLY (`dns_row_kernel_probe`): ONE launch of a row kernel of the
    lazy six-node step on the caller's operators.

    `'gc'`: `A` nv x (nv + np), `x` = r_v, `x2` = z_p -> `dict(y)`;
    `'tau'`: `A` np x nv, `x` = b, `x2` = kx -> `dict(y, r)`;
    `'step'`: `A` = K, `R1`, `cells` (nv x ncell pattern), `x` = x0, `x2` = v_c,
    `v_p`, `cellvals` -> `dict(kx, b, nfc)`;
    `'rw'`: `A` = K, `x` = z, `x2` = r -> `dict(y, wr, ww)` (partials);
    `'head'`: `x2` = the dense np x np rows, `x` = tau -> `dict(y)`."""
    lib = C.load_library()
    code = {'gc': 0, 'tau': 1, 'step': 2, 'rw': 3, 'head': 4}[kernel]
    p = C.dns_row_probe()
    p.kernel, p.lpr, p.fp32_vals = code, int(lpr), int(bool(fp32_vals))
    p.a_c, p.a_p = float(a_c), float(a_p)
    keep = []
    if kernel == 'head':
        S = np.ascontiguousarray(x2, dtype=np.float64)
        npr = S.shape[0]
        if S.shape != (npr, npr):
            raise ValueError('head: a square dense matrix')
        x = C.as_f64(x, size=npr)
        p.nsplit = npr
        p.x2 = C.dptr(S)
        y = np.empty(npr)
        C.check(lib.dns_row_kernel_probe(device, None, ct.byref(p), C.dptr(x),
                                         C.dptr(y)))
        return dict(y=y)
    view = C.CsrView(A)
    nr, nc = view.shape
    out = {}
    if kernel == 'gc':
        x = C.as_f64(x, size=nr)
        x2 = C.as_f64(x2, size=nc - nr)
        p.nsplit = nr
        y = np.empty(nr)
    elif kernel == 'tau':
        x = C.as_f64(x, size=nr + nc)
        x2 = C.as_f64(x2, size=nr + nc)
        y = np.empty(nr)
        out['r'] = np.empty(nr + nc)
        p.y2 = C.dptr(out['r'])
    elif kernel == 'step':
        v2, v3 = C.CsrView(R1), C.CsrView(cells)
        keep += [v2, v3]
        nv = v2.shape[0]
        x = C.as_f64(x, size=nr)
        x2 = C.as_f64(x2, size=nr)
        v_p = C.as_f64(v_p, size=nr)
        cellvals = C.as_f64(cellvals, size=v3.shape[1])
        p.a2, p.a3 = ct.pointer(v2.struct), ct.pointer(v3.struct)
        p.x3, p.x4 = C.dptr(v_p), C.dptr(cellvals)
        y = np.empty(nr)
        out['b'], out['nfc'] = np.empty(nr), np.empty(nv)
        p.y2, p.y3 = C.dptr(out['b']), C.dptr(out['nfc'])
    else:
        x = C.as_f64(x, size=nr)
        x2 = C.as_f64(x2, size=nr)
        y = np.empty(nr)
        parts = np.zeros(512)
        p.y2 = C.dptr(parts)
    p.x2 = C.dptr(x2)
    C.check(lib.dns_row_kernel_probe(device, view.byref(), ct.byref(p),
                                     C.dptr(x), C.dptr(y)))
    if kernel == 'step':
        out['kx'] = y
        return out
    out['y'] = y
    if kernel == 'rw':
        out['wr'] = parts[:p.nparts].copy()
        out['ww'] = parts[p.nparts:2*p.nparts].copy()
    return out


def dot(x, y, device=0):
    x, y = C.as_f64(x), C.as_f64(y)
    out = ct.c_double(0.)
    C.check(C.load_library().dns_dot(device, x.size, C.dptr(x), C.dptr(y),
                                     ct.byref(out)))
    return out.value


def axpy(a, x, y, device=0):
    x = C.as_f64(x)
    out = C.as_f64(y).copy()
    C.check(C.load_library().dns_axpy(device, x.size, float(a), C.dptr(x),
                                      C.dptr(out)))
    return out


def gemv(A, x, alpha=1., device=0):
    A = np.ascontiguousarray(A, dtype=np.float64)
    x = C.as_f64(x, size=A.shape[0])
    y = np.empty(A.shape[0])
    C.check(C.load_library().dns_gemv(device, A.shape[0], C.dptr(A),
                                      C.dptr(x), C.dptr(y), float(alpha)))
    return y


def dense_inverse(A, device=0):
    out = np.array(A, dtype=np.float64, order='C', copy=True)
    C.check(C.load_library().dns_dense_inverse(device, out.shape[0],
                                               C.dptr(out)))
    return out


def spmv_bench(A, variant='stream', reps=50, warmup=5, device=0):
    """average seconds per `y = A x` on resident data, and `||y||^2`"""
    view = C.CsrView(sps.csr_matrix(A))
    secs, chk = ct.c_double(0.), ct.c_double(0.)
    vid = _VARIANTS[variant] if isinstance(variant, str) else int(variant)
    C.check(C.load_library().dns_spmv_bench(
        device, view.byref(), vid, int(reps), int(warmup),
        ct.byref(secs), ct.byref(chk)))
    return secs.value, chk.value


def hbm_probe(nbytes=2 << 30, kind='read', reps=20, device=0):
    """attainable HBM bandwidth [GB/s] of plain streaming kernels over
    `nbytes` (`kind`: 'read' | 'copy' | 'triad')"""
    out = ct.c_double(0.)
    C.check(C.load_library().dns_hbm_probe(
        int(device), int(nbytes),
        {'read': 0, 'copy': 1, 'triad': 2, 'read8a': 3, 'read8b': 4,
         'read8c': 5, 'read_b64': 6, 'read_tiles8': 7,
         'read_tiles1': 8}[kind],
        int(reps), ct.byref(out)))
    return out.value
