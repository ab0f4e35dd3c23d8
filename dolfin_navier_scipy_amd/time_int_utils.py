"""MI355X drop-in for the semi-explicit integrators of the reference
(`dolfin_navier_scipy/time_int_utils.py`): same names, same keyword
interfaces, same callbacks, same return values -- but the constant system
`[[M + theta*dt*A, J^T], [J, 0]]`, the velocity/pressure iterates and the
convection history live in HBM, the right-hand side of every step is built by
a fused HIP SpMV kernel and the saddle-point solve is the block-preconditioned
Krylov iteration of `csrc/` (instead of `spsla.factorized`, tiu:89-91,134).

 * `cnab`                (tiu:23-145)   Heun start + CN / AB2
 * `sbdftwo`             (tiu:260-355)  Heun start + SBDF2
 * `semi_implicit_euler` (tiu:566-635)
 * `_onestepheun`        (tiu:366-477)  two boundary solves via `lin_alg_utils`
 * `_inittimegrid`       (tiu:480-489)
 * `LinearFeedback`      (tiu:148-196 composed as in snu:1243-1247) observer
                         feedback as a `dynamic_rhs` the loops can run resident
 * `BoundaryFeedback`    the same observer driving the controlled Dirichlet
                         values (`getbcs` / `diricontfuncs`), resident as well

Per step the host still evaluates the reference's callbacks (`f_vdp`, `getbcs`,
`applybcs`, `f_tdp`, `g_tdp`, `dynamic_rhs`, `savevp`) because they are the
caller's Python code; everything between them is on the device.  A
`dynamic_rhs` that is a `LinearFeedback` is no such callback: its arithmetic is
known, and `cnab` / `sbdftwo` hand it to the device with the rest of the step.
"""
import collections
import logging

import numpy as np
import scipy.sparse as sps

from . import lin_alg_utils as lau
from .saddle import SaddleSystem, ImexStepper, solve_opts, choose_schur

__all__ = ['cnab', 'sbdftwo', 'semi_implicit_euler', 'SOLVER',
           'LinearFeedback', 'BoundaryFeedback']

# solver settings of the time loops; `rtol` is relative to ||rhs||.  `None`:
# `lin_alg_utils.default_rtol` of the system at hand -- 1e-12, and 1e-13 where
# penalised rows inflate ||rhs|| (BASELINE config 5: Robin penalty 1/alpha =
# 1e5; its pressure meets 1e-8 against the direct solve at 1e-13 (1.7e-10), not
# at 1e-12 (1e-8) -- tests/test_gpu_config5.py)
SOLVER = dict(method='gmres', rtol=None, maxiter=400, restart=60,
              cheb_degree=6, drop_tol=1e-3, factorization='full', reorth=2,
              schur='auto', extrapolate='auto', device=0, check_every=2,
              use_graph=True, carry_residual=True)


# record of the last time loop that ran (diagnostics / tests): which Schur
# block its system got, the algebraic or geometric hierarchy behind it, time
# steps and Krylov steps of the loop
LAST_RUN = {}


def _record_run(name, system, stepper, reports=()):
    """`reports`: what rode along with the loop (`_Attachment`s, a
    `_DeviceRecord` or None); the keys of their `report()` go on top of those
    of an open loop whose trajectory the host collected"""
    LAST_RUN.clear()
    try:        # (runs in a `finally`: never in the way of the real error)
        LAST_RUN.update(
            record='host', run_calls=getattr(stepper, 'run_calls', 0),
            record_y=None, record_t=None,
            integrator=name, time_steps=stepper.total_steps,
            krylov_steps=stepper.total_iters,
            schur_hierarchy=getattr(system, 'schur_hierarchy', None),
            precond=system.precond_info(), feedback=None,
            feedback_y=None, feedback_u=None)
        for rep in reports:
            LAST_RUN.update({} if rep is None else rep.report())
    except Exception:
        pass


class _Attachment(object):
    """What rides along with the loop of `cnab` / `sbdftwo`.  The loop calls
    every attachment at the same places and never names one; each overrides
    what it needs"""

    def start(self, v, p, time):
        """the state after the Heun start"""

    def arm(self, times, tables):
        """behind `set_rhs_table`, for the steps towards `times` of a slice
        (or chunk) that runs on the device; `tables`: what the slice
        tabulated beside the right-hand sides (`_Tables`)"""

    def collect(self, times):
        """after these steps have run on the device"""

    def host_row(self, step):
        """after a step with a host round trip (`_Step`)"""

    def finish(self, drm):
        """behind the last slice; `drm`: the memory dict of `dynamic_rhs`"""

    def report(self):
        """the keys it contributes to `LAST_RUN`"""
        return {}


# `dbc*`: where the boundary moves (else None), the Dirichlet values -- of the
# state before each step and behind the last (`arm`), of the two states
_Tables = collections.namedtuple('_Tables', 'dbc')
_Step = collections.namedtuple('_Step', 'v v_prev p time dbc dbc_prev')


class LinearFeedback(object):
    """Output feedback through a linear observer as a `dynamic_rhs`

        y = cv_mat v,   hx' = ha hx + hb y + drift(t),   u = hc hx,
        returns b_mat u

    with the Heun / Adams-Bashforth-2 discretisation of the reference's
    `get_heunab_lti` (tiu:148-196), composed with `cv_mat` and `b_mat` as
    `solve_nse` does (snu:1243-1247).  Signature and modes (`init`,
    `heunpred`, `heuncorr`, `abtwo`) and the keys of `memory` (`lastt`,
    `lasthx`, `lastrhs`, `lastdt`, `hphx`) are the reference's, so any loop
    that takes a `dynamic_rhs` can call it.

    `cnab` / `sbdftwo` recognise an instance: with `device_convection` and
    `resident=` the AB2 steps are not called back but evaluated on the device
    (`ImexStepper.set_feedback`), with the constant step `dt` of the grid where
    the reference recomputes `t - lastt` (a difference of rounding only).

    `calls` counts the calls by mode; `history` lists `(t, mode, y, u)` of
    every call that was made on the host."""

    def __init__(self, cv_mat, b_mat, ha, hb, hc, inihx, drift=None):
        self.cv_mat = sps.csr_matrix(cv_mat)
        self.b_mat = sps.csr_matrix(b_mat)
        self.ha = np.array(ha, dtype=np.float64)
        hN = self.ha.shape[0]
        self.hb = np.array(hb, dtype=np.float64).reshape((hN, -1))
        self.hc = np.array(hc, dtype=np.float64).reshape((-1, hN))
        self.inihx = np.array(inihx, dtype=np.float64).reshape((hN, 1))
        self.hN, self.Ny, self.Nu = hN, self.hb.shape[1], self.hc.shape[0]
        if self.cv_mat.shape[0] != self.Ny or self.b_mat.shape[1] != self.Nu:
            raise ValueError('cv_mat / b_mat do not fit hb / hc')
        self._drift = drift
        self.calls = dict(init=0, heunpred=0, heuncorr=0, abtwo=0)
        self.history = []

    def drift(self, t):
        if self._drift is None:
            return np.zeros((self.hN, 1))
        return np.asarray(self._drift(t), dtype=np.float64).reshape(
            (self.hN, 1))

    def _out(self, t, mode, y, chx, memory):
        u = self.hc @ chx
        self.history.append((t, mode, None if y is None else y.reshape(-1),
                             u.reshape(-1)))
        return self.b_mat @ u, memory

    def __call__(self, t, vc=None, memory={}, mode='abtwo'):
        self.calls[mode] += 1
        ha, hb, inihx = self.ha, self.hb, self.inihx
        if mode == 'init':
            memory.update(dict(lastt=t, lasthx=inihx))
            return self._out(t, mode, None, inihx, memory)
        y = self.cv_mat @ np.asarray(vc).reshape((-1, 1))
        curdt = t - memory['lastt']
        if mode == 'heunpred':
            currhs = ha @ inihx + hb @ y + self.drift(memory['lastt'])
            chx = inihx + curdt*currhs
            memory.update(dict(lastrhs=currhs, hphx=chx))
        elif mode == 'heuncorr':
            currhs = ha @ memory['hphx'] + hb @ y + self.drift(t)
            chx = inihx + .5*curdt*(currhs + memory['lastrhs'])
            memory.update(dict(lastt=t, lasthx=chx, lastdt=curdt))
        elif mode == 'abtwo':
            currhs = ha @ memory['lasthx'] + hb @ y \
                + self.drift(memory['lastt'])
            chx = memory['lasthx'] + 1.5*curdt*currhs \
                - .5*memory['lastdt']*memory['lastrhs']
            memory.update(dict(lastt=t, lasthx=chx, lastrhs=currhs,
                               lastdt=curdt))
        else:
            raise ValueError('unknown mode {0}'.format(mode))
        return self._out(t, mode, y, chx, memory)


class _ResidentFeedback(_Attachment):
    """the device side of a `LinearFeedback` inside `cnab` / `sbdftwo`: takes
    the observer over from the Heun start, tabulates the drift per slice,
    collects the logs and hands the final state back to the memory dict"""

    def __init__(self, fb, stepper, drm, c_n, c_c, dt, tstart):
        self.fb, self.stepper, self.dt = fb, stepper, dt
        self.tlast = tstart
        self.ylog, self.ulog = [], []
        stepper.set_feedback(fb.cv_mat, fb.b_mat, fb.ha, fb.hb, fb.hc,
                             c_n=c_n, c_c=c_c, dt=dt)
        # corrector state, the PREDICTOR's right-hand side (tiu:171-174)
        stepper.set_feedback_state(drm['lasthx'], drm['lastrhs'],
                                   fb.hc @ drm['lasthx'])

    def arm(self, ctrange, tables):
        """the drift the step towards `ctrange[s]` sees is the one at the
        time before it (tiu:187-188)"""
        befores = [self.tlast] + list(ctrange[:-1])
        drift = None if self.fb._drift is None else \
            np.array([self.fb.drift(t)[:, 0] for t in befores])
        self.stepper.set_feedback_table(len(ctrange), drift)
        self.tlast = ctrange[-1]

    def collect(self, ctrange):
        y, u = self.stepper.feedback_log()
        self.ylog.append(y)
        self.ulog.append(u)

    def finish(self, drm):
        hx, flast, _ = self.stepper.feedback_state()
        drm.update(dict(lastt=self.tlast, lasthx=hx.reshape((-1, 1)),
                        lastrhs=flast.reshape((-1, 1)), lastdt=self.dt))

    def report(self):
        y = np.vstack(self.ylog) if self.ylog else np.zeros((0, self.fb.Ny))
        u = np.vstack(self.ulog) if self.ulog else np.zeros((0, self.fb.Nu))
        return dict(feedback='resident', feedback_y=y, feedback_u=u)


class _HostFeedback(_Attachment):
    """a `dynamic_rhs` (or `f_tvdp`) the loop calls back every step: reports
    only -- for a `LinearFeedback` `lti` the `(y, u)` rows of its AB2 steps"""

    def __init__(self, lti):
        self.lti = lti

    def report(self):
        fb = self.lti
        if fb is None:
            return dict(feedback='host')
        rows = [h for h in fb.history if h[1] == 'abtwo']
        y, u = ([h[k] for h in rows] for k in (2, 3))
        return dict(feedback='host',
                    feedback_y=np.array(y).reshape((-1, fb.Ny)),
                    feedback_u=np.array(u).reshape((-1, fb.Nu)))


class BoundaryFeedback(object):
    """Output feedback through a linear observer whose output drives the
    controlled Dirichlet values (rotating cylinders, a modulated inflow)

        y = cv_mat v_inner,   hx' = ha hx + hb y + drift(t),   u = hc hx,
        b(t) = base + s_mat u(t)

    `b`: the `nc` values of the controlled dofs in the order `getbcs` returns
    them, `s_mat`: `nc x Nu`, `base`: `nc` values (default 0).  The
    discretisation, the modes (`init`, `heunpred`, `heuncorr`, `abtwo`) and
    the keys of `memory` are `LinearFeedback`'s.  `cv_mat` is given over the
    FULL velocity dofs together with `invinds`; an entry in a Dirichlet column
    is refused: sensors live in the flow.

    Two faces of one object:
     * a `getbcs` of `cnab` / `sbdftwo`: `fb(time, vvec, pvec, mode=)` returns
       the list `b`; `vvec` is the full vector.  `bcs_ini` is what
       `fb(trange[0], mode='init')` returns.  With `device_convection` and
       `resident=` the AB2 / BDF2 steps are not called back: the device
       advances the observer and writes the values into the convection
       operator's Dirichlet table (`ImexStepper.set_feedback_boundary`)
     * `diricontfuncs` of `solve_nse`: `fb.controls()` returns `Nu` callables
       `func(time, vel=, p=, mode=, memory=)` that share the observer -- the
       first call for a `(time, mode)` advances it, the others read it; or
       the instance itself, `diricontfuncs=fb` (`s_mat` may be None then:
       `solve_nse` builds it from `diricontbcvals`, one column per boundary)

    `memory` is the object's own (`getbcs` has none to pass); `calls` counts
    the calls by mode; `history` lists `(t, mode, y, u)` of every observer
    step that was made on the host."""

    def __init__(self, cv_mat, s_mat, ha, hb, hc, inihx, invinds=None,
                 base=None, drift=None):
        self.ha = np.array(ha, dtype=np.float64)
        hN = self.ha.shape[0]
        self.hb = np.array(hb, dtype=np.float64).reshape((hN, -1))
        self.hc = np.array(hc, dtype=np.float64).reshape((-1, hN))
        self.inihx = np.array(inihx, dtype=np.float64).reshape((hN, 1))
        self.hN, self.Ny, self.Nu = hN, self.hb.shape[1], self.hc.shape[0]
        self.cv_mat = sps.csr_matrix(cv_mat)
        if self.cv_mat.shape[0] != self.Ny:
            raise ValueError('cv_mat has {0} rows, hb takes {1} outputs'
                             .format(self.cv_mat.shape[0], self.Ny))
        self.s_mat = self.base = self.invinds = self.cv_inner = None
        self._base = base
        if invinds is not None:
            self.bind_inner(invinds)
        if s_mat is not None:
            self.bind_boundary(s_mat)
        self._drift = drift
        self.memory = {}
        self.calls = dict(init=0, heunpred=0, heuncorr=0, abtwo=0)
        self.history = []
        self._seen = None           # `((time, mode), u)` of the last step

    def bind_inner(self, invinds):
        """the inner dofs of the full vector `cv_mat` is given over"""
        inv = np.asarray(invinds, dtype=np.int64).reshape(-1)
        outside = np.ones(self.cv_mat.shape[1], dtype=bool)
        outside[inv] = False
        cols = self.cv_mat.tocoo().col
        if np.any(outside[cols]):
            raise ValueError(
                'cv_mat has an entry in a Dirichlet column (dof {0}): sensors '
                'live in the flow'.format(int(cols[outside[cols]][0])))
        self.invinds = inv
        self.cv_inner = self.cv_mat[:, inv].tocsr()
        self.cv_inner.sort_indices()

    def bind_boundary(self, s_mat):
        s_mat = sps.csr_matrix(s_mat)
        if s_mat.shape[1] != self.Nu:
            raise ValueError('s_mat has {0} columns, hc gives {1} inputs'
                             .format(s_mat.shape[1], self.Nu))
        s_mat.sort_indices()
        nc = s_mat.shape[0]
        base = np.zeros(nc) if self._base is None else \
            np.array(self._base, dtype=np.float64).reshape(-1)
        if base.size != nc:
            raise ValueError('base has {0} entries, s_mat {1} rows'
                             .format(base.size, nc))
        self.s_mat, self.base = s_mat, base

    def drift(self, t):
        if self._drift is None:
            return np.zeros((self.hN, 1))
        return np.asarray(self._drift(t), dtype=np.float64).reshape(
            (self.hN, 1))

    def values(self, u):
        """`b = base + s_mat u`"""
        return self.base + self.s_mat @ np.asarray(u).reshape(-1)

    def observe(self, t, vvec=None, mode='abtwo'):
        """one observer step (`LinearFeedback.__call__` without `b_mat`);
        `vvec`: the full velocity vector.  Returns `u` (Nu)"""
        mode = 'init' if mode == 'stokes' else \
            'abtwo' if mode is None else mode
        if mode not in self.calls:
            raise ValueError('unknown mode {0}'.format(mode))
        self.calls[mode] += 1
        ha, hb, inihx, memory = self.ha, self.hb, self.inihx, self.memory
        if mode == 'init':
            memory.clear()
            memory.update(dict(lastt=t, lasthx=inihx))
            y, chx = None, inihx
        else:
            if self.cv_inner is None:
                raise ValueError('no inner dofs given (`invinds`)')
            vin = np.asarray(vvec, dtype=np.float64).reshape(-1)[self.invinds]
            y = self.cv_inner @ vin.reshape((-1, 1))
            curdt = t - memory['lastt']
            if mode == 'heunpred':
                currhs = ha @ inihx + hb @ y + self.drift(memory['lastt'])
                chx = inihx + curdt*currhs
                memory.update(dict(lastrhs=currhs, hphx=chx))
            elif mode == 'heuncorr':
                currhs = ha @ memory['hphx'] + hb @ y + self.drift(t)
                chx = inihx + .5*curdt*(currhs + memory['lastrhs'])
                memory.update(dict(lastt=t, lasthx=chx, lastdt=curdt))
            else:
                currhs = ha @ memory['lasthx'] + hb @ y \
                    + self.drift(memory['lastt'])
                chx = memory['lasthx'] + 1.5*curdt*currhs \
                    - .5*memory['lastdt']*memory['lastrhs']
                memory.update(dict(lastt=t, lasthx=chx, lastrhs=currhs,
                                   lastdt=curdt))
        u = (self.hc @ chx).reshape(-1)
        self.history.append((t, mode, None if y is None else y.reshape(-1),
                             u))
        return u

    def __call__(self, time, vvec=None, pvec=None, mode='abtwo'):
        return self.values(self.observe(time, vvec, mode)).tolist()

    def controls(self):
        """`Nu` control functions of one observer for `diricontfuncs`"""
        def control(k):
            def func(time, vel=None, p=None, mode=None, memory=None):
                key = (time, mode)
                if self._seen is None or self._seen[0] != key:
                    self._seen = (key, self.observe(time, vel, mode))
                return float(self._seen[1][k]), memory
            func.boundary_feedback = self
            return func
        return [control(k) for k in range(self.Nu)]

    def boundary_terms(self, applybcs, NV, NP):
        """`(Ba, Bm, Bj)`: `bfv`, `mbc` (NV x Nu) and `bfp` (NP x Nu) of the
        unit controls `s_mat e_k` -- `applybcs` is linear --, or None where it
        returns zero for all of them (the literal closure)"""
        cols = []
        for k in range(self.Nu):
            e = np.zeros(self.Nu)
            e[k] = 1.
            bfv, bfp, mbc = applybcs((self.s_mat @ e).tolist())
            cols.append((_col(bfv, NV), _col(mbc, NV), _col(bfp, NP)))
        if not any(np.any(c) for col in cols for c in col):
            return None
        return tuple(sps.csr_matrix(np.hstack([col[q] for col in cols]))
                     for q in range(3))


def _boundary_feedback_of(getbcs):
    """the `BoundaryFeedback` behind a `getbcs`, if any: the instance itself
    or a closure that carries it (`solve_nse`)"""
    if isinstance(getbcs, BoundaryFeedback):
        return getbcs
    fb = getattr(getbcs, 'boundary_feedback', None)
    return fb if isinstance(fb, BoundaryFeedback) else None


class _ResidentBoundaryFeedback(_Attachment):
    """the device side of a `BoundaryFeedback` inside `cnab` / `sbdftwo`:
    takes the observer over from the Heun start, leaves the loop the terms of
    `u = 0` to tabulate, arms drift rows and logs per slice, collects `y`,
    `u` and the boundary values the device wrote and hands the final state
    back to the object's memory"""

    def __init__(self, fb, loop, tstart):
        stepper = loop.stepper
        NV, NP = stepper.sys.NV, stepper.sys.NP
        self.fb, self.stepper, self.dt = fb, stepper, loop.dt
        self.tlast = tstart
        self.ylog, self.ulog, self.blog = [], [], []
        self.slice_bcs = []
        mem = fb.memory
        u_c = (fb.hc @ mem['lasthx']).reshape(-1)
        u_p = (fb.hc @ fb.inihx).reshape(-1)
        # (what the device continues must be what the host started)
        for name, got, u in (('bcs_ini', loop.bcs_ini, u_p),
                             ('the Heun start', loop.cur.bcs, u_c)):
            want = fb.values(u)
            if len(got) != want.size or not np.allclose(
                    np.asarray(got, dtype=np.float64), want, rtol=1e-12,
                    atol=1e-14):
                raise ValueError(
                    'boundary feedback: the boundary values of {0} are not '
                    '`base + s_mat u` of the observer (`bcs_ini` must be '
                    '`fb(trange[0], mode=\'init\')`)'.format(name))
        terms = fb.boundary_terms(loop.applybcs, NV, NP)
        Ba, Bm, Bj = (None, None, None) if terms is None else terms
        wm, wa = loop.scheme.bc_weights(loop.dt)
        stepper.set_feedback(fb.cv_inner, sps.csr_matrix((NV, fb.Nu)), fb.ha,
                             fb.hb, fb.hc, c_n=0., c_c=0., dt=loop.dt)
        stepper.set_feedback_boundary(fb.s_mat, fb.base,
                                      col0=len(loop.statvals), Ba=Ba, Bm=Bm,
                                      Bj=Bj, wm=wm, wa=wa)
        # corrector state, the PREDICTOR's right-hand side (tiu:171-174)
        stepper.set_feedback_state_bc(mem['lasthx'], mem['lastrhs'], u_c, u_p)
        # the values of the current state (row 0 of the next table); the loop
        # tabulates with `u = 0`
        self.current = np.array(loop.cur.bcs, dtype=np.float64)
        self.base_bcs = fb.base.tolist()
        bfv0, _, mbc0 = loop.applybcs(self.base_bcs)
        loop.prev = loop.prev._replace(mbc=mbc0)
        loop.cur = loop.cur._replace(bcs=self.base_bcs, bfv=bfv0, mbc=mbc0)

    def arm(self, ctrange, tables):
        befores = [self.tlast] + list(ctrange[:-1])
        drift = None if self.fb._drift is None else \
            np.array([self.fb.drift(t)[:, 0] for t in befores])
        self.stepper.set_feedback_table(len(ctrange), drift)
        self.tlast = ctrange[-1]

    def collect(self, ctrange):
        y, u = self.stepper.feedback_log()
        rows = self.stepper.feedback_bcs(0, len(ctrange) + 1)
        self.ylog.append(y)
        self.ulog.append(u)
        self.blog.append(rows[1:])
        self.slice_bcs.extend(rows[1:])
        self.current = rows[-1].copy()

    def finish(self, drm):
        hx, flast, _, _ = self.stepper.feedback_state_bc()
        self.fb.memory.update(dict(
            lastt=self.tlast, lasthx=hx.reshape((-1, 1)),
            lastrhs=flast.reshape((-1, 1)), lastdt=self.dt))

    def report(self):
        fb = self.fb
        y = np.vstack(self.ylog) if self.ylog else np.zeros((0, fb.Ny))
        u = np.vstack(self.ulog) if self.ulog else np.zeros((0, fb.Nu))
        b = np.vstack(self.blog) if self.blog else \
            np.zeros((0, fb.base.size))
        return dict(feedback='resident-boundary', feedback_y=y, feedback_u=u,
                    feedback_bcs=b)


RECORD_BYTES = 1 << 30      # default cap of a slice's snapshot buffer


def stop_steps(ctrange, savetimes, keep_prev=False):
    """Steps of a resident time slice whose state the host gets to see: those
    whose time is in `savetimes` (None: every step), the last step of the
    slice always (the loop goes on from it), and with `keep_prev` the step
    before it; in time order"""
    ns = len(ctrange)
    return [s for s, t in enumerate(ctrange)
            if savetimes is None or t in savetimes
            or s >= ns - 1 - bool(keep_prev)]


def plan_record(ctrange, savetimes, snap_bytes, record_bytes=RECORD_BYTES,
                keep_prev=False):
    """Slots and chunks of a recorded time slice (`resident=dict(record=True)`)

    Kept are the `stop_steps` of the slice.  A snapshot takes `snap_bytes`; a chunk keeps at most `record_bytes //
    snap_bytes` of them, so a slice that keeps more is cut into chunks, each
    ending with a kept step.  Returns the chunks in time order as dicts
    `first`, `nsteps` (steps `first .. first + nsteps` of the slice), `slots`
    (int32, `nsteps` entries: slot of the step or -1) and `kept` (list of
    `(step of the slice, slot)`); an empty slice has none."""
    ns = len(ctrange)
    cap = int(record_bytes) // int(snap_bytes)
    if cap < 1:
        raise ValueError('record_bytes = {0} is below one snapshot ({1} '
                         'bytes)'.format(record_bytes, snap_bytes))
    keep = set(stop_steps(ctrange, savetimes, keep_prev))
    chunks, first = [], 0
    while first < ns:
        slots, kept, s = [], [], first
        while s < ns:
            if s in keep:
                slots.append(len(kept))
                kept.append((s, len(kept)))
            else:
                slots.append(-1)
            s += 1
            if len(kept) == cap:
                break
        chunks.append(dict(first=first, nsteps=s - first,
                           slots=np.array(slots, dtype=np.int32), kept=kept))
        first = s
    return chunks


class _DeviceRecord(object):
    """`resident=dict(record=True)` of `cnab` / `sbdftwo`: runs a slice as one
    `stepper.run` per chunk of `plan_record` with the recorder on and hands
    back the kept states; collects `y = outputs v` of every step"""

    def __init__(self, stepper, rsd, NV, NP):
        self.stepper = stepper
        out = rsd.get('outputs', None)
        self.outputs = None if out is None else sps.csr_matrix(out)
        self.record_bytes = int(rsd.get('record_bytes', RECORD_BYTES))
        # (a slot is a ring vector: NV + NP padded to 64 entries)
        self.snap_bytes = 8*(-(-(NV + NP)//64)*64)
        self.ys, self.ts = [], []
        self.run_calls = 0

    def run_slice(self, cf, opts, ctrange, savetimes, upload, keep_prev=False,
                  after_chunk=None):
        """`upload(a, b)`: set the tables of the steps `a .. b` of the slice;
        returns `{step of the slice: (v, p)}` of the kept steps"""
        states = {}
        for ch in plan_record(ctrange, savetimes, self.snap_bytes,
                              self.record_bytes, keep_prev=keep_prev):
            a, n = ch['first'], ch['nsteps']
            upload(a, a + n)
            self.stepper.set_recorder(n, cv_mat=self.outputs,
                                      snap_slots=ch['slots'])
            self.stepper.run(n, cf, opts)
            self.run_calls += 1
            vs, ps = self.stepper.record_snapshots(0, len(ch['kept']))
            for s, slot in ch['kept']:
                states[s] = (vs[slot].reshape((-1, 1)),
                             ps[slot].reshape((-1, 1)))
            if self.outputs is not None:
                self.ys.append(self.stepper.record_outputs(0, n))
                self.ts.extend(ctrange[a:a + n])
            if after_chunk is not None:
                after_chunk()
        # (the recorder stays set: the next slice takes its buffers over, and
        # with them the graphs that were captured for them)
        return states

    def result(self):
        if self.outputs is None:
            return None, None
        ny = self.outputs.shape[0]
        y = np.vstack(self.ys) if self.ys else np.zeros((0, ny))
        return y, np.array(self.ts, dtype=np.float64)

    def report(self):
        rec_y, rec_t = self.result()
        return dict(record='device', record_y=rec_y, record_t=rec_t)


class _RowLog(_Attachment):
    """What `_FunctionalLog` and `_QuadraticLog` share: one row per step, from
    the device's log per slice (or chunk) or, where the loop takes one step
    at a time, from the host.  With controlled (moving) Dirichlet values `arm`
    takes their rows from `tables` -- one more than steps -- or, `live`
    (beside a resident `BoundaryFeedback`, which makes them on the device),
    points at the operator's table; `host_row` gets those of the two states.
    A subclass has `_set(nrows, dbc_table)`, `_get(count)`, `_evaluate(step)`,
    `key` (the prefix of its `LAST_RUN` keys), `width` (entries of a row),
    `moving` (False: constant values, no rows are handed on) and `need_rows`
    (moving values cannot do without them)."""
    key, width, moving, need_rows = None, 0, True, False

    def __init__(self, stepper, dt, live, names):
        self.stepper, self.dt, self.live = stepper, dt, live
        self.ys, self.ts = [], []
        self.where = None
        self.names = names

    def arm(self, times, tables):
        if not self.moving:
            return self._set(len(times), None)
        dbc_rows = 'operator' if self.live else tables.dbc
        short = self.need_rows if dbc_rows is None else \
            (not self.live and len(dbc_rows) != len(times) + 1)
        if short:
            raise ValueError('{0} steps need {1} rows of Dirichlet values, '
                             'got {2}'.format(
                                 len(times), len(times) + 1,
                                 None if dbc_rows is None else len(dbc_rows)))
        self._set(len(times), dbc_rows)

    def collect(self, times):
        self.add(self._get(len(times)), times)
        self.where = 'device'

    def add(self, rows, times):
        self.ys.append(np.asarray(rows, dtype=np.float64))
        self.ts.extend(times)

    def host_row(self, step):
        self.add(self._evaluate(step).reshape((1, -1)), [step.time])
        self.where = 'host'

    def result(self):
        y = np.vstack(self.ys) if self.ys else np.zeros((0, self.width))
        return y, np.array(self.ts, dtype=np.float64)

    def report(self):
        y, t = self.result()
        return {self.key: y, self.key + '_t': t, self.key + '_on': self.where,
                self.key + '_names': self.names}


class _FunctionalLog(_RowLog):
    """`resident=dict(functionals=fn)` of `cnab` / `sbdftwo`: arms the
    stepper's functionals next to the tables and collects their rows
    (`_RowLog`).  With controlled (moving) Dirichlet values the loop has
    `ndbc` of them, static ones included, and the functionals' boundary rows
    `cab`, `cmb` must be as wide, in that order"""
    key = 'functionals'

    def __init__(self, stepper, fn, dt, ndbc=None, live=False):
        if ndbc is not None and fn.inv is not None and fn.cab.shape[1] != ndbc:
            raise ValueError(
                '`functionals` with controlled (moving) Dirichlet values: '
                'they were built for {0} Dirichlet dofs, the loop has {1} '
                '(`static_dbcvals` then the controlled ones: build them with '
                '`dbcinds` in that order)'.format(fn.cab.shape[1], ndbc))
        _RowLog.__init__(self, stepper, dt, live,
                         None if fn is None else list(fn.names))
        self.fn = fn
        self.width = 0 if fn is None else fn.nF

    def _set(self, nrows, dbc_table):
        self.stepper.set_functionals(self.fn, nrows, self.dt,
                                     dbc_table=dbc_table)

    def _get(self, count):
        return self.stepper.get_functionals(0, count)

    def _evaluate(self, step):
        return self.fn.evaluate(step.v, step.v_prev, step.p, self.dt,
                                dbc=step.dbc, dbc_prev=step.dbc_prev)


class _QuadraticLog(_RowLog):
    """`resident=dict(quadratics=qf)` of `cnab` / `sbdftwo`, `qf` a
    `fem.QuadraticFunctionals` (the energy budget): arms the stepper's
    quadratics next to the tables -- the matrices stay on the device from
    slice to slice -- and collects their rows (`_RowLog`).  Forms that carry
    CONSTANT Dirichlet values (`qf.ndbc == 0`) are for loops without moving
    ones (`ndbc` None).  With controlled (moving) Dirichlet values the loop
    has `ndbc` of them, static ones included, and the forms must stand on
    `NV + ndbc` dofs, the Dirichlet dofs in that order"""
    key, need_rows = 'quadratics', True

    def __init__(self, stepper, qf, dt, max_grid=None, ndbc=None,
                 live=False):
        if ndbc is not None and qf.ndbc == 0:
            raise ValueError(
                '`quadratics` with moving Dirichlet values: the forms carry '
                'the boundary values as constants (build them with '
                '`moving=True`)')
        if (ndbc or 0) != qf.ndbc:
            raise ValueError(
                '`quadratics` with controlled (moving) Dirichlet values: '
                'they were built for {0} Dirichlet dofs, the loop has {1} '
                '(`static_dbcvals` then the controlled ones: build them with '
                '`dbcinds` in that order)'.format(qf.ndbc, ndbc or 0))
        _RowLog.__init__(self, stepper, dt, live, list(qf.names))
        self.qf, self.max_grid = qf, max_grid
        self.width, self.moving = qf.nQ, qf.ndbc > 0

    def _set(self, nrows, dbc_table):
        kw = {} if dbc_table is None else dict(dbc_table=dbc_table)
        self.stepper.set_quadratics(self.qf, nrows, self.dt,
                                    max_grid=self.max_grid, **kw)

    def _get(self, count):
        return self.stepper.get_quadratics(0, count)

    def _evaluate(self, step):
        return self.qf.evaluate(step.v, step.v_prev, self.dt, dbc=step.dbc,
                                dbc_prev=step.dbc_prev)


class _PodEnsemble(_Attachment):
    """`resident=dict(pod=pod)` of `cnab` / `sbdftwo`, `pod` a
    `fem.SnapshotPOD`: plans the kept steps of the whole loop once, arms the
    stepper's snapshot ensemble per slice (or chunk) next to the tables -- a
    slot table each, the ensemble stays and fills up --, and when the loop ends
    forms the Gram matrix on the device, decomposes it on the host (`m x m`)
    and has the device combine the modes and the mean flow: `m^2` and `(r + 1)
    NV` doubles come back, the snapshots never do.  Where the loop takes one
    step at a time the kept states are stored on the host and go through
    `pod.evaluate`.  The snapshots are the inner velocity dofs: controlled
    Dirichlet values are not in them.  With `rom` (a `fem.GalerkinROM`) the
    modes and the mean flow go on into `rom.project` with the loop's convection
    operator `conv` -- on the device where the POD was formed there, through
    the host model otherwise"""

    def __init__(self, stepper, pod, trange, keep_snapshots=False, rom=None,
                 conv=None):
        NV = stepper.sys.NV
        if pod.NV != NV:
            raise ValueError('`pod`: its weight matrix is {0} x {0}, the loop '
                             'has NV = {1}'.format(pod.NV, NV))
        self.stepper, self.pod = stepper, pod
        kept, _ = pod.plan(trange)
        self.times = np.array([float(trange[k]) for k in kept])
        self.m = len(kept)
        self.where, self.armed = None, False
        self.keep_snapshots = keep_snapshots
        self.host = {}
        self.filled = 0             # kept steps that have run
        self.res = None
        self.rom, self.conv, self.rom_res = rom, conv, None

    def arm(self, times, tables):
        self.stepper.set_ensemble(self.pod.slots_for(times), nslots=self.m,
                                  reset=not self.armed)
        self.armed = True

    def collect(self, times):
        self.filled += int(np.sum(self.pod.slots_for(times) >= 0))

    def host_row(self, step):
        slot = int(self.pod.slots_for([step.time])[0])
        if slot >= 0:
            self.host[slot] = np.array(step.v, dtype=np.float64).reshape(-1)
            self.filled += 1

    def finish(self, drm):
        pod, stepper = self.pod, self.stepper
        if self.filled < self.m:
            # the loop broke off (blow-up guard): slots are unfilled or hold
            # what blew up -- no decomposition, the caller gets its `ffflag`
            self.res = None
            self.where = self.where or ('device' if self.armed else 'host')
            if self.armed:
                stepper.clear_ensemble()
                self.armed = False
            return
        if self.armed and not self.host:
            gram = stepper.ensemble_gram(pod.W)
            dec = pod.decompose(gram)
            modes, mean = pod.split(dec, stepper.ensemble_combine(dec['coef']))
            self.res = dict(gram=gram, sigma=dec['sigma'], modes=modes,
                            mean=mean, coeffs=dec['coeffs'], coef=dec['coef'])
            if self.keep_snapshots:
                self.res['snapshots'] = stepper.ensemble()
            self.where = 'device'
        else:
            S = stepper.ensemble() if self.armed else \
                np.zeros((self.m, pod.NV))
            for slot, v in self.host.items():
                S[slot] = v
            self.res = pod.evaluate(S)
            if self.keep_snapshots:
                self.res['snapshots'] = S
            self.where = 'host'
        self.res['times'] = self.times
        if self.armed:
            stepper.clear_ensemble()
            self.armed = False
        if self.rom is not None:
            if self.rom.M is None:
                self.rom.M = pod.W
            self.rom_res = self.rom.project(
                self.res['modes'], self.res['mean'], self.conv,
                self.conv.dbcvals, device=self.where == 'device')

    def report(self):
        out = dict(pod=self.res, pod_on=self.where)
        if self.rom is not None:
            out.update(rom=self.rom_res, rom_on=self.where)
        return out


class _StatisticsSums(_Attachment):
    """`resident=dict(statistics=fs)` of `cnab` / `sbdftwo`, `fs` a
    `fem.FlowStatistics`: arms the stepper's statistics per slice (or chunk)
    next to the tables -- a bin table each, the sums go on -- and downloads
    them ONCE, when the loop ends, into `fs`; where the loop takes one step at
    a time the same states go through `fs.add` on the host.  The Heun start is
    a host step on both paths (`start`): both count the same states"""

    def __init__(self, stepper, fs):
        self.stepper, self.fs = stepper, fs
        self.where = None
        self.armed = False

    def start(self, v, p, time):
        self.fs.add(v, p, time)

    def arm(self, times, tables):
        self.stepper.set_statistics(self.fs.bins(times), nbins=self.fs.nbins,
                                    pairs=self.fs.pairs, reset=False)
        self.armed = True
        self.where = 'device'

    def host_row(self, step):
        self.fs.add(step.v, step.p, step.time)
        self.where = 'host'

    def finish(self, drm):
        if self.armed:
            self.fs.add_sums(self.stepper.statistics())
            self.armed = False

    def report(self):
        sums = {k: (None if a is None else np.array(a))
                for k, a in self.fs.sums().items()}
        return dict(statistics=sums, statistics_on=self.where)


# boundary values, the terms `applybcs` makes of them, the forcing and what
# `dynamic_rhs` returned at one time; `dfv` is the float 0. where the loop runs
# resident: there the actuation, if any, is added on the device
_Terms = collections.namedtuple('_Terms', 'bcs bfv mbc fv dfv')

# What tells the schemes apart, as data: the system is `M + theta*dt*A`;
# `r1(M, A, dt)`; `coeffs(dt)`: `a_c, a_p, cn_c, cn_o` of `dns_imex_coeffs`;
# `fb_weights`: `(c_n, c_c)` of a resident `LinearFeedback`; `row(dt, prev,
# cur, nxt)`: the scheme's ONE formula of a step's `gvec` -- everything that is
# not `R1 v` or convection -- from the `_Terms` at the two times before it and
# at its own; `keep_prev`: the state before a slice's last step is a stop;
# `state_v_p`: `set_state` gets the velocity before the Heun start;
# `guard_prev`: the blow-up guard looks at the velocity BEFORE the last step
# and logs nothing (reference quirk, tiu:311), else at `stepper.vnorm()`
# `bc_weights(dt)`: `(wm, wa)`, what `row` multiplies `mbc` and `bfv` of the
# times `n, c, p` with -- a resident `BoundaryFeedback` adds `(wm_j Bm + wa_j
# Ba) u_j` on the device
_Scheme = collections.namedtuple(
    '_Scheme', 'name theta r1 coeffs fb_weights row keep_prev state_v_p '
    'guard_prev bc_weights')

_CNAB = _Scheme(
    name='cnab', theta=.5, r1=lambda M, A, dt: (M - .5*dt*A).tocsr(),
    coeffs=lambda dt: dict(a_c=1., a_p=0., cn_c=1.5*dt, cn_o=-.5*dt),
    fb_weights=(.5, .5),
    bc_weights=lambda dt: ((-1., 1., 0.), (.5*dt, .5*dt, 0.)),
    row=lambda dt, p, c, n: (-(n.mbc - c.mbc)
                             + .5*dt*(c.fv + n.fv + n.bfv + c.bfv
                                      + n.dfv + c.dfv)),
    keep_prev=False, state_v_p=False, guard_prev=False)

_SBDF2 = _Scheme(
    name='sbdftwo', theta=2./3, r1=lambda M, A, dt: M,
    coeffs=lambda dt: dict(a_c=4./3, a_p=-1./3, cn_c=4./3*dt, cn_o=-2./3*dt),
    fb_weights=(2./3, 0.),
    bc_weights=lambda dt: ((-1., 4/3, -1/3), (2/3*dt, 0., 0.)),
    row=lambda dt, p, c, n: (-(n.mbc - 4/3*c.mbc + 1/3*p.mbc)
                             + 2/3*dt*n.bfv + 2/3*dt*(n.fv + n.dfv)),
    keep_prev=True, state_v_p=True, guard_prev=True)


# A base trajectory (`convection.BaseTrajectory`) names the row of every time
# convection is evaluated at -- with `interpolate`, the row and the weight
# towards the next one.  The three places that arm it: the coverage check
# before the loop, a chunk's table, and a single time (Heun start, host step).
def _base_rows_at(traj, ts):
    """`(rows, weights or None)`; `ValueError` by the time not covered"""
    if getattr(traj, 'interpolate', False):
        return traj.weights_at(ts)
    return traj.rows_at(ts), None


def _arm_base_rows(conv, traj, ts):
    rows, weights = _base_rows_at(traj, ts)
    if weights is None:
        conv.set_base_rows(rows)
    else:
        conv.set_base_rows(rows, weights)


def _arm_base_row(conv, traj, time):
    rows, weights = _base_rows_at(traj, [time])
    if weights is None:
        conv.set_base_row(int(rows[0]))
    else:
        conv.set_base_row(int(rows[0]), float(weights[0]))


class _ImexLoop(object):
    """The AB2 / BDF2 steps of `cnab` and `sbdftwo` behind the Heun start: how
    `resident=` is read, the terms of the last two times (`prev`, `cur`) and
    the last two states, a time slice on the device as tabulate / upload /
    replay / collect (`run_slice`), a step with a host round trip (`step`),
    and the slices one after the other (`march`).  What differs between the
    schemes is in `scheme`; what rides along is in `attachments`"""

    def __init__(self, scheme, stepper, cf, opts, dt, resident, conv, bcs_ini,
                 state_dependent, prev=None, cur=None, v_c=None, v_n=None,
                 p_n=None, drm=None, getbcs=None, applybcs=None,
                 appndbcs=None, f_tdp=None, g_tdp=None, f_vdp=None,
                 dynamic_rhs=None, savevp=None, bfb=None):
        # (`bfb`: the `BoundaryFeedback` behind `getbcs` where the loop can
        # run it resident -- the only state-dependent `getbcs` that may)
        self.bfb, self.bfb_att, self.bcs_ini = bfb, None, bcs_ini
        if bfb is not None and (conv is None or resident is None
                                or state_dependent):
            raise ValueError('a resident `BoundaryFeedback` needs '
                             '`device_convection` and `resident=`')
        self.scheme, self.stepper, self.cf = scheme, stepper, cf
        self.opts = opts
        self.dt, self.conv, self.state_dependent = dt, conv, state_dependent
        # (`v_c`: the velocity before the last step, `v_n`, `p_n`: the state)
        self.v_c, self.v_n, self.p_n, self.drm = v_c, v_n, p_n, drm
        self.getbcs, self.applybcs, self.appndbcs = getbcs, applybcs, appndbcs
        self.f_tdp, self.g_tdp, self.f_vdp = f_tdp, g_tdp, f_vdp
        self.dynamic_rhs, self.savevp = dynamic_rhs, savevp
        self.rsd = rsd = dict(resident or {})
        self.statvals = list(rsd.get('static_dbcvals', []) or [])
        self.moving = len(bcs_ini) > 0
        if conv is not None:
            stepper.set_convection(conv, scale=-1.0)
            if self.moving or self.statvals:
                conv.set_dbcvals(self.statvals + list(cur.bcs))
        self.on_device = (conv is not None and resident is not None
                          and not state_dependent
                          and (not self.moving or bfb is not None
                               or rsd.get('bcs_time_only', False)))
        self.prev = prev
        self.cur = cur._replace(dfv=0.) if self.on_device else cur
        savetimes = rsd.get('savevp_times', None)
        self.savetimes = None if savetimes is None else set(savetimes)
        # `record=True`: the device writes the trajectory down (where the loop
        # runs resident at all)
        self.drec = _DeviceRecord(stepper, rsd, stepper.sys.NV,
                                  stepper.sys.NP) \
            if (self.on_device and rsd.get('record', False)) else None
        self.attachments = []
        # a linearised operator about a time-varying base flow
        # (`convection.BaseTrajectory`): every evaluation names the row of the
        # time of its operand; `t_n`: the time of the state `v_n` (`march`)
        self.traj = getattr(conv, 'base_trajectory', None)
        self.t_n = None

    def attach(self, lti, fb_dev, tstart, trange=None):
        """the functionals, the statistics, the quadratics, the POD ensemble
        (it plans over the loop's `trange`) and the feedback -- a
        `LinearFeedback` `lti` that can run resident (`fb_dev`) as the
        observer on the device -- in the order they are armed in (inside the
        loop's `try`: they may refuse)"""
        resident_fb = fb_dev and self.on_device
        if not resident_fb and (lti is not None or self.state_dependent):
            self.attachments.append(_HostFeedback(lti))
        host_bfb = _boundary_feedback_of(self.getbcs)
        if self.bfb is None and host_bfb is not None and lti is None \
                and not self.state_dependent:
            # called back every step: its `(y, u)` rows for the report
            self.attachments.append(_HostFeedback(host_bfb))
        ndbc = len(self._dbc(self.cur)) if self.moving else None
        fn = self.rsd.get('functionals', None)
        qf = self.rsd.get('quadratics', None)
        live = self.bfb is not None
        if live:
            # The boundary values exist on the device only: functionals and
            # quadratics read the operator's table, which the observer kernel
            # writes; nothing host-made can stand in for it.
            if self.rsd.get('rom', None) is not None:
                raise ValueError(
                    '`rom` together with a resident `BoundaryFeedback`: '
                    'constant boundary values only, the mean flow carries '
                    'them')
            for key, att, wide in (
                    ('functionals', fn, lambda a: a.inv is not None
                     and a.cab.shape[1]),
                    ('quadratics', qf, lambda a: a.ndbc)):
                if att is None:
                    continue
                try:
                    have = wide(att)
                except AttributeError:
                    have = None
                if have != ndbc:
                    raise ValueError(
                        '`{0}` together with a resident `BoundaryFeedback`: '
                        'the boundary values exist on the device only, so '
                        'the {0} must be built for the loop\'s {1} moving '
                        'Dirichlet values (`static_dbcvals` then the '
                        'controlled ones{2})'.format(
                            key, ndbc,
                            '; `moving=True`' if key == 'quadratics'
                            else '; `dbcinds` in that order'))
            self.bfb_att = _ResidentBoundaryFeedback(self.bfb, self, tstart)
            self.attachments.append(self.bfb_att)
        flog = None if fn is None else _FunctionalLog(
            self.stepper, fn, self.dt, ndbc=ndbc, live=live)
        if resident_fb:
            self.attachments.append(_ResidentFeedback(
                lti, self.stepper, self.drm, *self.scheme.fb_weights,
                dt=self.dt, tstart=tstart))
        fs = self.rsd.get('statistics', None)
        pod = self.rsd.get('pod', None)
        rom = self.rsd.get('rom', None)
        if rom is not None:
            if pod is None:
                raise ValueError('`rom` without `pod`: the reduced operators '
                                 'are projections onto the POD\'s modes')
            if self.conv is None:
                raise ValueError(
                    '`rom` needs the loop\'s device convection operator '
                    '(`device_convection`) for the tensor: a host `f_vdp` '
                    'has no element data')
            if self.moving:
                raise ValueError(
                    '`rom` with moving Dirichlet values: constant boundary '
                    'values only, the mean flow carries them')
            if getattr(self.conv, 'linearised', False):
                raise ValueError(
                    'linearised convection operator (`set_base_flow`) with '
                    '`rom`: the tensor is the projection of the nonlinear '
                    'form N(u)u (`clear_base_flow` first)')
        self.attachments += [a for a in (
            flog, None if fs is None else _StatisticsSums(self.stepper, fs),
            None if qf is None else _QuadraticLog(
                self.stepper, qf, self.dt,
                max_grid=self.rsd.get('quadratics_max_grid', None),
                ndbc=ndbc, live=live),
            None if pod is None else _PodEnsemble(
                self.stepper, pod, trange,
                keep_snapshots=self.rsd.get('pod_snapshots', False),
                rom=rom, conv=self.conv))
            if a is not None]

    def _terms_at(self, ctime, v_c=None, p_c=None):
        """the callbacks of the step towards `ctime` behind `f_vdp`, in the
        reference's order (tiu:114-120, 330-336); with the state the step
        starts from `dynamic_rhs` as well, without it (a slice is tabulated
        ahead of its states) `getbcs` sees `None, None`.  Returns the `_Terms`
        and the lower right-hand side"""
        vfull = None if v_c is None else self.appndbcs(v_c, self.cur.bcs)
        # (a resident `BoundaryFeedback` is not called: the slice is tabulated
        # for `u = 0`, the device adds what is linear in `u`)
        bcs_n = self.bfb_att.base_bcs if self.bfb_att is not None else \
            self.getbcs(ctime, vfull, p_c, mode='abtwo')
        bfv_n, bfp_n, mbc_n = self.applybcs(bcs_n)
        fv_n, fp_n = self.f_tdp(ctime), self.g_tdp(ctime)
        dfv_n = 0.
        if v_c is not None:
            dfv_n, self.drm = self.dynamic_rhs(ctime, vc=v_c, memory=self.drm,
                                               mode='abtwo')
        return (_Terms(bcs_n, bfv_n, mbc_n, fv_n, dfv_n),
                _col(fp_n + bfp_n, self.stepper.sys.NP))

    def _dbc(self, terms):
        return self.statvals + list(terms.bcs)

    def run_slice(self, ctrange):
        """the whole slice on the device: tabulate what the callbacks return,
        upload, replay; the host sees the `stop_steps` only, `savevp` the save
        times"""
        stepper, moving = self.stepper, self.moving
        NV, NP = stepper.sys.NV, stepper.sys.NP
        ns = len(ctrange)
        gvt, gpt = np.empty((ns, NV)), np.empty((ns, NP))
        # (the functionals see the values of the state a step LEAVES: one row
        # more, the values behind the slice's last step)
        dbt = np.empty((ns + 1, len(self._dbc(self.cur)))) if moving else None
        for s, ctime in enumerate(ctrange):
            nxt, gp = self._terms_at(ctime)
            gvt[s] = _col(self.scheme.row(self.dt, self.prev, self.cur, nxt),
                          NV)[:, 0]
            gpt[s] = gp[:, 0]
            if moving:       # N(v_c) sees the CURRENT boundary values
                dbt[s] = self._dbc(self.cur)
            self.prev, self.cur = self.cur, nxt
        bcs_n = self.cur.bcs
        if moving:
            dbt[ns] = self._dbc(self.cur)
        span = [0, 0]
        # (`t_cur[s]`: the time of the state step `s` starts from -- the
        # convention of `dbt[s]`)
        t_cur = [self.t_n] + list(ctrange[:-1])
        bfa, nstat = self.bfb_att, len(self.statvals)
        if bfa is not None:
            bfa.slice_bcs = []

        def upload(a, b):
            stepper.set_rhs_table(gvt[a:b], gpt[a:b])
            if bfa is not None:
                # one row more: the device writes row `s + 1` in step `s`;
                # row 0 holds the values of the state the chunk starts from
                tab = dbt[a:b + 1].copy()
                tab[0, nstat:] = bfa.current
                self.conv.set_dbc_table(tab)
            elif moving:
                self.conv.set_dbc_table(dbt[a:b])
            if self.traj is not None:
                _arm_base_rows(self.conv, self.traj, t_cur[a:b])
            tables = _Tables(dbt[a:b + 1] if moving else None)
            for att in self.attachments:
                att.arm(ctrange[a:b], tables)
            span[:] = [a, b]

        def after_chunk():
            for att in self.attachments:
                att.collect(ctrange[span[0]:span[1]])
        if self.drec is not None:
            # the device writes the slice down; the host collects it
            states = self.drec.run_slice(
                self.cf, self.opts, ctrange, self.savetimes, upload,
                keep_prev=self.scheme.keep_prev, after_chunk=after_chunk)
        else:
            upload(0, ns)
            states, done = {}, 0
            for s in stop_steps(ctrange, self.savetimes,
                                self.scheme.keep_prev):
                stepper.run(s + 1 - done, self.cf, self.opts)
                done = s + 1
                states[s] = stepper.get_state()
            after_chunk()
        if bfa is not None:
            # the values every state carries are the device's
            self.cur = self.cur._replace(bcs=bfa.current.tolist())
        for s, ctime in enumerate(ctrange):
            if self.savetimes is None or ctime in self.savetimes:
                bcs_at = bfa.slice_bcs[s].tolist() if bfa is not None \
                    else dbt[s + 1][len(self.statvals):].tolist() \
                    if (moving and s + 1 < ns) else bcs_n
                self.savevp(self.appndbcs(states[s][0], bcs_at),
                            states[s][1], time=ctime)
        if moving:
            self.conv.set_dbcvals(self._dbc(self.cur))
        stepper.set_rhs(_col(0., NV), _col(0., NP))
        if self.scheme.keep_prev:
            self.v_c = states[ns - 2][0] if ns > 1 else self.v_n
        self.v_n, self.p_n = states[ns - 1]
        self.t_n = ctrange[-1]

    def step(self, ctime):
        """one step with a host round trip: each callback of the reference's
        step, in its order (tiu:104-143, 320-353)"""
        stepper, conv, cur = self.stepper, self.conv, self.cur
        v_c, p_c = self.v_n, self.p_n
        if conv is not None and (self.moving or self.statvals):
            conv.set_dbcvals(self._dbc(cur))
        if conv is not None and self.traj is not None:
            _arm_base_row(conv, self.traj, self.t_n)
        nfc_new = None if conv is not None \
            else self.f_vdp(self.appndbcs(v_c, cur.bcs))
        nxt, gp = self._terms_at(ctime, v_c, p_c)
        gvec = self.scheme.row(self.dt, self.prev, cur, nxt)
        stepper.set_rhs(_col(gvec, stepper.sys.NV), gp)
        stepper.step(self.cf, nfc_new=nfc_new, opts=self.opts)
        v_n, p_n = stepper.get_state()
        row = _Step(v_n, v_c, p_n, ctime,
                    self._dbc(nxt) if self.moving else None,
                    self._dbc(cur) if self.moving else None)
        for att in self.attachments:
            att.host_row(row)
        self.savevp(self.appndbcs(v_n, nxt.bcs), p_n, time=ctime)
        self.prev, self.cur = cur, nxt
        self.v_c, self.v_n, self.p_n = v_c, v_n, p_n
        self.t_n = ctime

    def _blown_up(self, kck, ntimeslices, check_ff_maxv, verbose):
        """the blow-up guard at a slice's start"""
        quiet = self.scheme.guard_prev
        nrmvc = np.linalg.norm(self.v_c) if quiet else self.stepper.vnorm()
        if verbose and not quiet:
            logging.info('time {0}/{1} -- |v| {2:.2e}'.format(
                kck, ntimeslices, nrmvc))
        blown = nrmvc > check_ff_maxv or np.isnan(nrmvc)
        if blown and not quiet:
            logging.warning('BREAK: |v| is `NaN` or |v| > threshhold')
        return blown

    def march(self, tstart, listofts, ntimeslices, check_ff_maxv, verbose):
        """all slices; returns `ffflag`"""
        ffflag = 0
        self.t_n = tstart
        for att in self.attachments:
            att.start(self.v_n, self.p_n, tstart)
        for kck, ctrange in enumerate(listofts):
            if self._blown_up(kck, ntimeslices, check_ff_maxv, verbose):
                ffflag = 1
                break
            if self.on_device and len(ctrange) > 0:
                self.run_slice(ctrange)
            else:
                for ctime in ctrange:
                    self.step(ctime)
        for att in self.attachments:
            att.finish(self.drm)
        return ffflag


def _checkuniformgrid(trange):
    steps = np.diff(np.asarray(trange, dtype=np.float64))
    if not np.allclose(np.linalg.norm(np.diff(steps)), 0):
        raise NotImplementedError()


def _inittimegrid(trange, ntimeslices=10):
    _checkuniformgrid(trange)
    dt = trange[1] - trange[0]
    rest = np.array(trange[2:])
    chunk = np.floor(rest.size/ntimeslices).astype(np.int32)
    slices = [rest[k*chunk:(k+1)*chunk].tolist() for k in range(ntimeslices)]
    slices.append(rest[ntimeslices*chunk:].tolist())
    return dt, slices


def _col(vec, n):
    """callbacks may return scalars (`applybcs -> 0., 0., 0.`, snu:1104)"""
    arr = np.asarray(vec, dtype=np.float64)
    if arr.ndim == 0 or arr.size == 1:
        return np.full((n, 1), float(arr.reshape(-1)[0]) if arr.size else 0.)
    return arr.reshape((n, 1))


def _wrap_callbacks(NV, dynamic_rhs, f_tvdp, f_vdp):
    zerorhs = np.zeros((NV, 1))
    if dynamic_rhs is None:
        def dynamic_rhs(t, vc=None, memory={}, mode=None):
            return zerorhs, memory
    if f_tvdp is not None:
        inner = dynamic_rhs

        def dynamic_rhs(t, vc=None, memory={}, mode=None):
            val, mem = inner(t, vc=vc, memory=memory, mode=mode)
            return val + f_tvdp(t, vc), mem
    if f_vdp is None:
        def f_vdp(vvec):
            return zerorhs
    return dynamic_rhs, f_vdp


def _solver_settings(solver):
    prm = dict(SOLVER)
    prm.update(solver or {})
    return prm


def _device_system(fmat, J, prm):
    NP = J.shape[0]
    system = SaddleSystem(fmat, J, device=prm['device'])
    # dense inverse up to `schur_dense_max` pressure dofs; beyond it the
    # multigrid block, on nested pressure spaces if the caller has them
    # (`prolongations`: refined meshes), else on an algebraic hierarchy
    schur = choose_schur(system, fmat, J, schur=prm['schur'],
                         prolongations=prm.get('prolongations'),
                         dense_max=lau.DEFAULTS['schur_dense_max'])
    if prm['extrapolate'] == 'auto':
        # warm start: quartic where one Krylov step per time step does it
        # (dense Schur block); cubic with the multigrid block, whose solves
        # run their cycle's two columns (`saddle.streaming_precond_defaults`)
        prm['extrapolate'] = 3 if schur == 'mg' else 4
    # the full block factorisation needs the explicit polynomial matrix
    fact = prm['factorization']
    if fmat.shape[0] > 1000000 or not 2 <= prm['cheb_degree'] <= 12:
        fact = 'triangular'
    system.setup_precond(cheb_degree=prm['cheb_degree'], schur=schur,
                         drop_tol=prm['drop_tol'], factorization=fact)
    rtol = prm['rtol'] if prm['rtol'] is not None else lau.default_rtol(fmat)
    opts = solve_opts(method=prm['method'], rtol=rtol,
                      maxiter=prm['maxiter'], restart=prm['restart'],
                      check_every=prm['check_every'],
                      use_graph=prm['use_graph'], reorth=prm['reorth'])
    return system, opts


def _onestepheun(vc=None, pc=None, tc=None, tn=None, M=None, A=None, J=None,
                 scalep=1., dfv_c=None, dynamic_rhs=None, drm={},
                 bcs_c=None, applybcs=None, appndbcs=None, getbcs=None,
                 f_tdp=None, f_vdp=None, g_tdp=None, krylov=None,
                 krpslvprms={}, base_row=None):
    """IMEX-Euler predictor / trapezoidal corrector (tiu:366-477); both
    saddle solves go through `lin_alg_utils.solve_sadpnt_smw` on the GPU.
    The corrector keeps the reference's `amat=M` (tiu:466).  `base_row(t)`: a
    device convection about a base trajectory is told the time of the state
    `f_vdp` is about to see"""
    NP, NV = J.shape
    if base_row is None:
        def base_row(time):
            pass
    dt = tn - tc
    JT = sps.csr_matrix(J.T)
    bfv_c, _, mbc_c = applybcs(bcs_c)
    fv_c = f_tdp(tc)
    base_row(tc)
    nfc_c = f_vdp(appndbcs(vc, bcs_c))
    tdfv_n, drm = dynamic_rhs(tn, vc=vc, memory=drm, mode='heunpred')
    tbcs = getbcs(tn, appndbcs(vc, bcs_c), pc, mode='heunpred')
    tbfv_n, tbfp_n, tmbc_n = applybcs(tbcs)
    fv_n, fp_n = f_tdp(tn), g_tdp(tn)
    tfv = M @ vc + dt*(fv_n + tbfv_n + tdfv_n) + dt*nfc_c - (tmbc_n - mbc_c)
    tvp_n = lau.solve_sadpnt_smw(amat=M + dt*A, jmat=J, jmatT=JT, rhsv=tfv,
                                 rhsp=_col(fp_n + tbfp_n, NP), krylov=krylov,
                                 krpslvprms=krpslvprms)
    tv_n = tvp_n[:NV, :]
    tp_n = 1./dt*scalep*tvp_n[NV:, :]
    dfv_n, drm = dynamic_rhs(tn, vc=tv_n, memory=drm, mode='heuncorr')
    base_row(tn)
    tnfc_n = f_vdp(appndbcs(tv_n, tbcs))
    bcs_n = getbcs(tn, appndbcs(tv_n, tbcs), tp_n, mode='heuncorr')
    bfv_n, bfp_n, mbc_n = applybcs(bcs_n)
    rhs_n = M @ vc - (mbc_n - mbc_c) - .5*dt*(A @ (vc + tv_n)) \
        + .5*dt*(fv_c + fv_n + bfv_n + bfv_c + dfv_n + dfv_c + nfc_c + tnfc_n)
    vp_n = lau.solve_sadpnt_smw(amat=M, jmat=J, jmatT=JT, rhsv=rhs_n,
                                rhsp=_col(fp_n + bfp_n, NP), krylov=krylov,
                                krpslvprms=krpslvprms)
    v_n = vp_n[:NV].reshape((NV, 1))
    p_n = 1./dt*scalep*vp_n[NV:].reshape((NP, 1))
    base_row(tn)
    nfc_n = f_vdp(appndbcs(v_n, bcs_n))
    return (v_n, p_n, bcs_n, bfv_n, mbc_c, mbc_n, fv_n, nfc_c, nfc_n, dfv_n,
            drm)


def _imex_loop(scheme, trange, inivel, inip, bcs_ini, M, A, J, f_vdp, f_tdp,
               g_tdp, scalep, getbcs, applybcs, appndbcs, savevp, dynamic_rhs,
               dynamic_rhs_memory, check_ff_maxv, ntimeslices, verbose, solver,
               device_convection, invinds, resident, f_tvdp=None):
    """`cnab` / `sbdftwo` with their keywords (`scheme`: `_CNAB` / `_SBDF2`):
    the Heun start on the host, the constant system and the stepper on the
    device, then the slices of `_ImexLoop`"""
    prm = _solver_settings(solver)
    # a `LinearFeedback` is evaluated on the device with the step itself
    lti = dynamic_rhs if isinstance(dynamic_rhs, LinearFeedback) else None
    fb_dev = (lti is not None and f_tvdp is None
              and device_convection is not None and resident is not None)
    state_dependent = (dynamic_rhs is not None and not fb_dev) \
        or f_tvdp is not None
    # a `BoundaryFeedback` behind `getbcs` runs on the device as well (beside
    # an open loop: the step has ONE observer node)
    bfb = _boundary_feedback_of(getbcs)
    if not (bfb is not None and dynamic_rhs is None and f_tvdp is None
            and device_convection is not None and resident is not None
            and len(bcs_ini) > 0):
        bfb = None
    dt, listofts = _inittimegrid(trange, ntimeslices=ntimeslices)
    NP, NV = J.shape
    # a base trajectory on the operator must cover the time of every state
    # convection is evaluated at (all but the last): refused by the time,
    # before anything is armed
    traj = getattr(device_convection, 'base_trajectory', None)
    base_row = None
    if traj is not None:
        _base_rows_at(traj, trange[:-1])

        def base_row(time):
            _arm_base_row(device_convection, traj, time)
    if device_convection is not None and f_vdp is None:
        f_vdp = device_convection.host_callback(invinds)   # Heun start only
    dynamic_rhs, f_vdp = _wrap_callbacks(NV, dynamic_rhs, f_tvdp, f_vdp)
    dfv_c, drm = dynamic_rhs(trange[0], vc=inivel, memory=dynamic_rhs_memory,
                             mode='init')
    savevp(appndbcs(inivel, bcs_ini), inip, time=trange[0])
    (v_n, p_n, bcs_n, bfv_n, mbc_c, mbc_n, fv_n, nfc_c, nfc_n, dfv_n,
     drm) = _onestepheun(vc=inivel, pc=inip, tc=trange[0], tn=trange[1],
                         M=M, A=A, J=J, scalep=scalep, dfv_c=dfv_c,
                         dynamic_rhs=dynamic_rhs, drm=drm, bcs_c=bcs_ini,
                         applybcs=applybcs, appndbcs=appndbcs, getbcs=getbcs,
                         f_tdp=f_tdp, f_vdp=f_vdp, g_tdp=g_tdp,
                         base_row=base_row)
    savevp(appndbcs(v_n, bcs_n), p_n, time=trange[1])

    # the constant system of the loop, factor-once in the reference (tiu:89-91)
    M, A = sps.csr_matrix(M), sps.csr_matrix(A)
    system, opts = _device_system((M + scheme.theta*dt*A).tocsr(), J, prm)
    stepper = ImexStepper(system, scheme.r1(M, A, dt))
    cf = ImexStepper.coeffs(pscale=scalep/dt, extrapolate=prm['extrapolate'],
                            carry_residual=prm['carry_residual'],
                            **scheme.coeffs(dt))
    stepper.set_state(v_n, v_p=inivel if scheme.state_v_p else None,
                      ptilde_c=p_n*dt/scalep, nfc_c=nfc_c)
    loop = _ImexLoop(
        scheme, stepper, cf, opts, dt, resident, device_convection, bcs_ini,
        state_dependent, prev=_Terms(None, None, mbc_c, None, None),
        cur=_Terms(bcs_n, bfv_n, mbc_n, fv_n, dfv_n), v_c=inivel, v_n=v_n,
        p_n=p_n, drm=drm, getbcs=getbcs, applybcs=applybcs,
        appndbcs=appndbcs, f_tdp=f_tdp, g_tdp=g_tdp, f_vdp=f_vdp,
        dynamic_rhs=dynamic_rhs, savevp=savevp, bfb=bfb)
    try:
        loop.attach(lti, fb_dev, trange[1], trange=trange)
        ffflag = loop.march(trange[1], listofts, ntimeslices, check_ff_maxv,
                            verbose)
    finally:
        _record_run(scheme.name, system, stepper,
                    [loop.drec] + loop.attachments)
        stepper.close()
        system.close()
    return loop.v_n, loop.p_n, ffflag


def cnab(trange=None, inivel=None, inip=None, bcs_ini=[],
         M=None, A=None, J=None, f_vdp=None, f_tdp=None, g_tdp=None,
         f_tvdp=None, scalep=-1., getbcs=None, applybcs=None, appndbcs=None,
         savevp=None, dynamic_rhs=None, dynamic_rhs_memory={},
         check_ff_maxv=None, ntimeslices=10, verbose=True, solver=None,
         device_convection=None, invinds=None, resident=None):
    """Crank-Nicolson / Adams-Bashforth-2 on the GPU (reference tiu:23-145)

    `solver`: optional dict overriding `SOLVER` (method, rtol, cheb_degree...).
    `device_convection`: a `convection.ConvectionP2` (with `invinds`, the inner
    dofs of the full velocity vector) -- the loop then evaluates `-N(v)v` on
    the device and `f_vdp` is not called per step.
    `resident`: dict, with `device_convection` only -- what the caller
    guarantees about its callbacks so that whole time slices run on the device
    without a host round trip per step:
      `bcs_time_only`   `getbcs(t, v, p)` ignores `v` and `p` (prescribed
                        boundary motion); static boundaries need no flag
      `static_dbcvals`  values of the operator's leading (static) Dirichlet
                        dofs; the controlled values `bcs` follow them
      `savevp_times`    the only times `savevp` has to see (None: all)
      `record`          True: the device writes the states of these times down
                        while it replays the slice (`ImexStepper.set_recorder`)
                        and `savevp` is called afterwards, in time order, with
                        the arguments it gets otherwise -- ONE `stepper.run`
                        per slice instead of one per saved time
      `outputs`         with `record`: a sparse `C` (Ny x NV); `y = C v` of
                        every step of the loop ends up in
                        `LAST_RUN['record_y']`, its times in `['record_t']`
      `record_bytes`    with `record`: cap of a slice's snapshot buffer
                        (default 1 GiB); a slice that keeps more runs in
                        chunks (`plan_record`)
      `functionals`     a `fem.MomentumFunctionals` (drag, lift, torque,
                        pressure differences, ...): evaluated
                        on the device after every step of a slice
                        (`ImexStepper.set_functionals`), with and without
                        `record`; `LAST_RUN['functionals']` is `nsteps x nF`,
                        `['functionals_t']` its times.  The rows cover the
                        AB2 / BDF2 steps of the loop, `trange[2:]`: the Heun
                        start runs on the host and has no row.  Where the
                        loop does not run resident the same rows come from
                        `fn.evaluate` on the host;
                        `LAST_RUN['functionals_on']` says 'device' or
                        'host'.  With controlled Dirichlet values (`bcs_ini`
                        not empty) the functionals must be built with
                        `dbcinds` = the static dofs then the controlled ones
                        (the order of `static_dbcvals + bcs`; `ValueError`
                        otherwise): the boundary terms `cab . g + cmb .
                        (g - g_prev)/dt` go by the values of each state, on
                        the device with `bcs_time_only` (a table of their own
                        per slice), on the host otherwise
      `statistics`      a `fem.FlowStatistics`: running sums (mean, second
                        moments, products of listed pairs, by bins) of the
                        state `[v; p]` after the Heun start and after every
                        AB2 / BDF2 step, `trange[1:]`, added on the device
                        where the loop runs resident
                        (`ImexStepper.set_statistics`: a bin table per slice,
                        ONE download when the loop ends), through `fs.add` on
                        the host otherwise; the sums end up in the object
                        itself (on top of what it held) and, as a dict, in
                        `LAST_RUN['statistics']`; `['statistics_on']` says
                        'device' or 'host'
      `quadratics`      a `fem.QuadraticFunctionals` (the energy budget:
                        kinetic energy, dissipation rate, `u^T M du/dt`, the
                        M-norm of `du/dt`; any forms `a^T Q b` over sparse
                        matrices): evaluated on the device after every step
                        of a slice (`ImexStepper.set_quadratics`; the
                        matrices are uploaded once), rows and times as for
                        `functionals`: `LAST_RUN['quadratics']` is `nsteps x
                        nQ`, `['quadratics_t']` its times, `['quadratics_on']`
                        'device' or 'host' (`qf.evaluate` per step),
                        `['quadratics_names']` the forms' names.  With
                        controlled Dirichlet values (`bcs_ini` not empty) the
                        forms must stand on the full space (the builders'
                        `moving=True` with `dbcinds` = the static dofs then
                        the controlled ones, `qf.ndbc` = their number): the
                        operands `[v; g]`, `[v - v_prev; g - g_prev]` go by
                        the values of each state, on the device with
                        `bcs_time_only` (a table of their own per slice), on
                        the host otherwise; forms that carry the boundary
                        values as constants (`qf.ndbc == 0`) are a
                        `ValueError` there.  `quadratics_max_grid` caps the workgroups of
                        the kernel and with them the log (`nsteps x G x nQ`
                        doubles per slice)
      `pod`             a `fem.SnapshotPOD` (weight matrix, which times are
                        kept, truncation): the velocities of the kept AB2 /
                        BDF2 steps (`trange[2:]`; the Heun start is not a
                        snapshot) are copied into an ensemble on the device
                        that lasts over the slices
                        (`ImexStepper.set_ensemble`: one copy node per step);
                        when the loop ends the Gram matrix `S W S^T` is formed
                        on the device (fp64 matrix cores), decomposed on the
                        host (`m x m`) and the modes and the mean flow are
                        combined on the device: `m^2 + (r + 1) NV` doubles
                        come back.  `LAST_RUN['pod']` is a dict `gram`,
                        `sigma`, `modes` (r x NV), `mean`, `coeffs` (r x m),
                        `coef`, `times`; `['pod_on']` says 'device' or 'host'
                        (`pod.evaluate` of the states stored per step); a
                        loop that breaks off on the blow-up guard leaves
                        `['pod']` None.  The
                        snapshots are the inner dofs `v`: with controlled
                        Dirichlet values the boundary values are not part of
                        the POD.  `ValueError` when the ensemble would exceed
                        `pod.max_bytes`.  `pod_snapshots=True` downloads the
                        snapshots as well (`['pod']['snapshots']`, m x NV:
                        diagnostics)
      `rom`             with `pod`: a `fem.GalerkinROM` (the condensed `A`,
                        `fv`; `M` defaults to the POD's weight matrix).  When
                        the modes exist they are projected with the loop's
                        convection operator (`rom.project`): the reduced mass
                        and stiffness matrices and the constant term through
                        `X W Y^T` on the fp64 matrix cores, the cubic
                        convection tensor `int phi_i . (u_j . grad) u_k`
                        through `ConvectionP2.project_tensor` -- on the device
                        where the POD was formed there, by the fp64 host model
                        otherwise.  `LAST_RUN['rom']` is the dict `Mr`, `Ar`,
                        `b0`, `c`, `L`, `H` (`div` with `J`), None where the
                        loop broke off; `['rom_on']` says 'device' or 'host'.
                        Constant Dirichlet values only; `ValueError` without
                        `pod`, without `device_convection`, or with `bcs_ini`
                        not empty
    `LAST_RUN['record']` says 'device' or 'host', `LAST_RUN['run_calls']`
    counts the `stepper.run` calls of the loop.
    The per-step data the callbacks return (`f_tdp`, `g_tdp`, `applybcs`) are
    tabulated per slice and uploaded (`dns_imex_set_rhs_table`,
    `dns_conv_set_dbc_table`); the blow-up guard stays at the slice starts.
    Not possible (falls back to one host round trip per step) with a
    `dynamic_rhs` or `f_tvdp`, which depend on the state -- except a
    `dynamic_rhs` that is a `LinearFeedback` (without `f_tvdp`): the Heun start
    calls it on the host, then the observer state is handed to the stepper,
    the drift is tabulated per slice next to the right-hand sides, and after
    the loop the final observer state is written back into the memory dict;
    `LAST_RUN['feedback']` says 'resident' then and `LAST_RUN['feedback_y']`,
    `['feedback_u']` hold the outputs and inputs of the AB2 steps.
    A `getbcs` that reads the state keeps the per-step path as well -- except
    a `BoundaryFeedback` (without `dynamic_rhs` / `f_tvdp`, with `bcs_ini`
    from its `init` call): the device advances its observer and writes the
    controlled values into the convection operator's Dirichlet table, the
    slices are tabulated for `u = 0`; `LAST_RUN['feedback']` says
    'resident-boundary' and `['feedback_bcs']` holds the values of every
    step.  `functionals` and `quadratics` beside it run on the device too:
    they read the operator's table, where the observer kernel writes the
    values (no host-made copy could hold them), and must be built for the
    loop's moving Dirichlet values (`ValueError` otherwise); `rom` beside it
    is a `ValueError`.
    Returns `v_n, p_n, ffflag` like the reference.
    """
    return _imex_loop(_CNAB, **locals())


def sbdftwo(trange=None, inivel=None, inip=None, bcs_ini=[],
            M=None, A=None, J=None, f_vdp=None, f_tdp=None, g_tdp=None,
            check_ff=False, check_ff_maxv=None, scalep=-1.,
            getbcs=None, applybcs=None, appndbcs=None, savevp=None,
            dynamic_rhs=None, dynamic_rhs_memory={},
            ntimeslices=10, verbose=True, solver=None,
            device_convection=None, invinds=None, resident=None):
    """SBDF2 on the GPU (reference tiu:260-355, quirks kept: pressure scaled
    by `1/dt`, blow-up guard on the previous velocity)

    `device_convection`, `invinds`, `resident`: as in `cnab` -- `-N(v)v` from
    the device operator, and whole time slices without a host round trip per
    step when the callbacks depend on the time only (rhs / boundary-value
    tables)."""
    kw = locals()
    del kw['check_ff']          # (unused, as in the reference)
    return _imex_loop(_SBDF2, **kw)


def semi_implicit_euler(iniv=None, jmat=None, mmat=None, amat=None, rhsv=None,
                        trange=None, data_trange=None, fp=None, solver=None,
                        device_convection=None, constant_rhs=None):
    """`M v' + A v + J^T p = rhs(t, v)`, `J v = fp` with the linear part
    implicit (reference tiu:566-635); list of velocities at `data_trange`

    `device_convection` (a `convection.ConvectionP2` over the inner dofs) with
    `constant_rhs` (NV x 1 or None): the right-hand side is
    `rhs(t, v) = constant_rhs - N(v)v`, evaluated on the device -- `rhsv` is
    not called and the loop runs resident between the data points."""
    prm = _solver_settings(solver)
    record = list(np.copy(trange if data_trange is None else data_trange))
    record.pop(0)
    NP, NV = jmat.shape
    fpz = np.zeros((NP, 1)) if fp is None else fp
    dt = trange[1] - trange[0]
    mmat, amat = sps.csr_matrix(mmat), sps.csr_matrix(amat)
    system, opts = _device_system((mmat + dt*amat).tocsr(), jmat, prm)
    stepper = ImexStepper(system, mmat)
    cf = ImexStepper.coeffs(a_c=1., a_p=0., cn_c=dt, cn_o=0., pscale=1.,
                            extrapolate=prm['extrapolate'],
                            carry_residual=prm['carry_residual'])
    stepper.set_state(iniv)
    stepper.set_rhs(np.zeros((NV, 1)), fpz)
    out = [iniv]
    cv = iniv
    try:
        if device_convection is not None:
            stepper.set_convection(device_convection, scale=-1.0)
            if constant_rhs is not None:
                stepper.set_rhs(dt*_col(constant_rhs, NV), fpz)
            todo = 0
            for ct in trange[1:]:
                todo += 1
                if len(record) > 0 and ct == record[0]:
                    stepper.run(todo, cf, opts)
                    todo = 0
                    out.append(stepper.get_state()[0])
                    record.pop(0)
            if todo:
                stepper.run(todo, cf, opts)
            return out
        for ct in trange[1:]:
            # b_v = M v + dt*rhs(t, v): `rhs` plays the role of the convection
            stepper.step(cf, nfc_new=rhsv(ct, cv), opts=opts)
            cv, _ = stepper.get_state()
            if len(record) > 0 and ct == record[0]:
                out.append(cv)
                record.pop(0)
    finally:
        _record_run('semi_implicit_euler', system, stepper)
        stepper.close()
        system.close()
    return out
