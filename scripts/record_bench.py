"""What it costs to SEE the trajectory of the explicit loop: stepping rates with
the device-resident recorder against one host round trip per step, on the
bench configuration (cylinder wake N=2, Re=100, dt=1/512, bench.py's solver
defaults, start from the Stokes state).

One command per leg (profiles/r08_recorder/README.md):

  --leg stepwise  `run(1)` + `get_state()` per step: what `cnab` does today
                  when `savevp` wants every step (no API newer than
                  `ImexStepper.run`, so the parent tree runs it too)
  --leg open      `run(steps)` after the spin-up, nothing recorded
  --leg snap      `run(steps)` with a snapshot of every step, then ONE download
  --leg outputs   `run(steps)` with `y = C v` of every step (the three box
                  means of scripts/feedback_bench.py, nnz(C) = 977)
  --leg forces    `run(steps)` with drag, lift and dp of every step evaluated
                  on the device (`ImexStepper.set_functionals`), then ONE
                  download of the rows; `--with-outputs`: the recorder's `y`
                  log on as well
  --leg forces_stepwise  `run(1)` + `get_state()` + the same functionals
                  evaluated on the host (`MomentumFunctionals.evaluate`) per
                  step: what scripts/schaefer_turek_unsteady.py does without
                  the device log
  --refine R      the same legs on the mesh refined R times (multigrid Schur
                  block, dt = 1/(512 2^R), start from rest, as refined_bench.py)

Timing: HIP events around `stp.run` (the `device_seconds` it returns), as
bench.py does; the download of leg `snap` / `outputs` by the host clock, stated
apart (`download_seconds`) and included in `steps_per_s_with_download`; leg
`stepwise`, which has no long `run`, by the host clock around the loop, whose
every step ends in a synchronise.  Each leg is repeated `--repeats` times from
a fresh system; one JSON line per leg.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


class RefinedSetup(object):
    """the stepper of refined_bench.py (start from rest)"""

    def __init__(self, refine):
        from dolfin_navier_scipy_amd.fem import (
            get_sysmats, cylinder_mesh_hierarchy, pressure_prolongations,
            TaylorHood)
        import feedback_bench as fbb
        self.femp, sm, self.rhsd = get_sysmats(problem='cylinderwake', N=2,
                                               refine=refine, Re=100.)
        self.M, self.A, self.J = (sm[k].tocsr() for k in 'MAJ')
        self.dt = 1./(512*2**refine)
        hier = cylinder_mesh_hierarchy(N=2, refine=refine)
        spaces = [TaylorHood(m) for m, _ in hier][::-1]
        self.prols = pressure_prolongations(spaces, [p for _, p in hier][::-1])
        self.C, _ = fbb.sensors_actuators(self.femp['V'],
                                          self.femp['invinds'], self.M)

    def stepper(self):
        from dolfin_navier_scipy_amd import saddle, convection
        M, A, J, dt, femp = self.M, self.A, self.J, self.dt, self.femp
        NP, NV = J.shape
        system = saddle.SaddleSystem((M + .5*dt*A).tocsr(), J)
        system.set_schur_mg(self.prols, smooth_steps=2)
        dflt = saddle.streaming_precond_defaults(NV + NP)
        system.setup_precond(cheb_degree=dflt['cheb_degree'], schur='mg',
                             drop_tol=dflt['drop_tol'], fhat='explicit',
                             factorization='full')
        stp = saddle.ImexStepper(system, (M - .5*dt*A).tocsr())
        cvop = convection.ConvectionP2.from_taylor_hood(
            femp['V'], femp['invinds'], femp['dbcinds'], femp['dbcvals'])
        v0 = np.zeros((NV, 1))
        nfc0 = cvop.apply(v0, scale=-1.0)
        stp.set_state(v0, nfc_c=nfc0, nfc_o=nfc0)
        stp.set_rhs(dt*self.rhsd['fv'], self.rhsd['fp'])
        stp.set_convection(cvop, scale=-1.0)
        cf = saddle.ImexStepper.coeffs(a_c=1., cn_c=1.5*dt, cn_o=-.5*dt,
                                       pscale=-1./dt,
                                       extrapolate=dflt['extrapolate'])
        opts = saddle.solve_opts(rtol=1e-10, maxiter=400, use_graph=True,
                                 reorth=2)

        def close():
            stp.close()
            cvop.close()
            system.close()
        return stp, cf, opts, close


def _record(stp, steps, secs, its):
    return dict(seconds=secs, steps_per_s=steps/secs, iters=int(its),
                run=dict(stp.last_run), step_counters=stp.step_counters(),
                vnorm=stp.vnorm())


def _timed_window(stp, cf, opts, steps, attempts=3):
    """`run(steps)`; a window in which graphs had to be captured (the predicted
    cycle length moved: a one-time cost like the set-up) is repeated, as
    refined_bench.py does; returns `(seconds, iters, windows run)`"""
    for n in range(1, attempts + 1):
        secs, its, _ = stp.run(steps, cf, opts)
        if stp.last_run['captures'] == 0:
            break
    return secs, its, n


def leg_open(su, steps, spin):
    stp, cf, opts, close = su.stepper()
    try:
        stp.run(spin, cf, opts)
        secs, its, n = _timed_window(stp, cf, opts, steps)
        out = _record(stp, steps, secs, its)
        out['windows'] = n
    finally:
        close()
    return out


def leg_stepwise(su, steps, spin):
    stp, cf, opts, close = su.stepper()
    try:
        stp.run(spin, cf, opts)
        t0 = time.perf_counter()
        for _ in range(steps):
            stp.run(1, cf, opts)
            v, p = stp.get_state()
        secs = time.perf_counter() - t0
        out = dict(seconds=secs, steps_per_s=steps/secs, vnorm=stp.vnorm(),
                   v_last_norm=float(np.linalg.norm(v)))
    finally:
        close()
    return out


def _leg_recorded(su, steps, spin, snaps, outputs):
    stp, cf, opts, close = su.stepper()
    try:
        # (set before the spin-up, like the tables of feedback_bench.py: the
        # graphs of the recorded step are captured there, the timed call
        # replays)
        # (rows for up to three windows: see _timed_window; the last one is
        # downloaded)
        stp.set_recorder(spin + 3*steps, cv_mat=su.C if outputs else None,
                         snap_slots='all' if snaps else None)
        stp.run(spin, cf, opts)
        secs, its, n = _timed_window(stp, cf, opts, steps)
        out = _record(stp, steps, secs, its)
        out['windows'] = n
        spin += (n - 1)*steps
        t0 = time.perf_counter()
        nbytes = 0
        if snaps:
            v, p = stp.record_snapshots(spin, steps)
            nbytes += v.nbytes + p.nbytes
            vl, pl = stp.get_state()
            out['last_row_is_state'] = bool(
                np.array_equal(v[-1], vl[:, 0])
                and np.array_equal(p[-1], pl[:, 0]))
        if outputs:
            y = stp.record_outputs(spin, steps)
            nbytes += y.nbytes
            out['y_last'] = y[-1].tolist()
        dl = time.perf_counter() - t0
        out.update(download_seconds=dl, download_bytes=int(nbytes),
                   steps_per_s_with_download=steps/(secs + dl))
    finally:
        close()
    return out


def leg_snap(su, steps, spin):
    return _leg_recorded(su, steps, spin, True, False)


def leg_outputs(su, steps, spin):
    return _leg_recorded(su, steps, spin, False, True)


def _functionals(su):
    """drag and lift coefficients and the pressure difference"""
    from dolfin_navier_scipy_amd import fem
    femp = su.femp
    th = femp['V']
    return fem.boundary_forces(th, femp, names=('cD', 'cL')).scaled(
        2./((2./3)**2*0.1)) \
        + fem.pressure_difference(th, (0.15, 0.2), (0.25, 0.2))


def leg_forces(su, steps, spin, with_outputs=False):
    stp, cf, opts, close = su.stepper()
    try:
        fn = _functionals(su)
        dt = getattr(su, 'dt', 1./512)
        # (set before the spin-up, rows for up to three windows: as
        # _leg_recorded)
        if with_outputs:
            stp.set_recorder(spin + 3*steps, cv_mat=su.C)
        stp.set_functionals(fn, spin + 3*steps, dt)
        stp.run(spin, cf, opts)
        secs, its, n = _timed_window(stp, cf, opts, steps)
        out = _record(stp, steps, secs, its)
        out['windows'] = n
        spin += (n - 1)*steps
        t0 = time.perf_counter()
        rows = stp.get_functionals(spin, steps)
        # (what crosses the bus: every workgroup's share of every row; the
        # getter sums them; `functional_grid` of csrc/functional.hpp)
        ncl = sum(int(c.size) for c in fn.cells)
        grid = max(1, min(64, max(-(-3*fn.nF//4), -(-ncl//32))))
        nbytes = steps*grid*fn.nF*8
        if with_outputs:
            y = stp.record_outputs(spin, steps)
            nbytes += y.nbytes
        dl = time.perf_counter() - t0
        out.update(download_seconds=dl, download_bytes=int(nbytes),
                   steps_per_s_with_download=steps/(secs + dl),
                   rows_bytes=int(rows.nbytes), workgroups=grid,
                   names=fn.names, row_last=rows[-1].tolist(),
                   body_cells=int(fn.cells[0].size))
    finally:
        close()
    return out


def leg_forces_outputs(su, steps, spin):
    return leg_forces(su, steps, spin, with_outputs=True)


def leg_forces_stepwise(su, steps, spin):
    stp, cf, opts, close = su.stepper()
    try:
        fn = _functionals(su)
        dt = getattr(su, 'dt', 1./512)
        stp.run(spin, cf, opts)
        vprev = stp.get_state()[0][:, 0]
        rows = np.empty((steps, fn.nF))
        t0 = time.perf_counter()
        for k in range(steps):
            stp.run(1, cf, opts)
            v, p = stp.get_state()
            rows[k] = fn.evaluate(v[:, 0], vprev, p[:, 0], dt)
            vprev = v[:, 0]
        secs = time.perf_counter() - t0
        out = dict(seconds=secs, steps_per_s=steps/secs, vnorm=stp.vnorm(),
                   names=fn.names, row_last=rows[-1].tolist())
    finally:
        close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=('stepwise', 'open', 'snap', 'outputs',
                                      'forces', 'forces_stepwise'),
                    required=True)
    ap.add_argument('--with-outputs', action='store_true',
                    help="leg forces: the recorder's y log on as well")
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--spin', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--refine', type=int, default=0)
    ap.add_argument('--label', default='')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from dolfin_navier_scipy_amd import _capi
    if _capi.device_count() < 1:
        raise SystemExit('no HIP device: nothing is measured without one')
    if args.refine > 0:
        su = RefinedSetup(args.refine)
    else:
        import feedback_bench as fbb
        su = fbb.Setup()
    fn = dict(stepwise=leg_stepwise, open=leg_open, snap=leg_snap,
              outputs=leg_outputs, forces_stepwise=leg_forces_stepwise,
              forces=(leg_forces_outputs if args.with_outputs
                      else leg_forces))[args.leg]
    reps = [fn(su, args.steps, args.spin) for _ in range(args.repeats)]
    key = 'steps_per_s_with_download' \
        if args.leg in ('snap', 'outputs', 'forces') \
        else 'steps_per_s'
    rates = [r['steps_per_s'] for r in reps]
    out = dict(leg=args.leg, label=args.label, steps=args.steps,
               spin=args.spin, refine=args.refine,
               unknowns=int(su.J.shape[0] + su.J.shape[1]),
               device=_capi.device_name(0), steps_per_s=rates,
               best=max(rates), worst=min(rates),
               spread_rel=(max(rates) - min(rates))/max(rates),
               with_download=[r[key] for r in reps], repeats=reps)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
