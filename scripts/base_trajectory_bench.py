"""Stepping rates of the explicit CNAB loop with a linearised / adjoint
convection operator about a TIME-VARYING base flow
(`ConvectionP2.set_base_flow(BaseTrajectory)`, `ImexStepper.ensemble_to_base`),
on the bench configuration (cylinder wake N=2, Re=100, dt=1/512, bench.py's
solver defaults) and, `--refine R`, on the mesh refined R times (the stepper of
refined_bench.py: multigrid Schur block, dt = 1/(512 2^R)).

Per repeat: a nonlinear stepper runs `--spin` steps, then `--steps` steps that
leave every velocity in its snapshot ensemble -- the stored forward run.  A
second stepper then steps the perturbation, per `--modes` (forward, adjoint;
the adjoint walks the slots backwards), in these variants, their order
rotating with the repeat:

  a<k>  the resident loop about the trajectory: the slots adopted device to
        device, one index table for the whole window, `run(steps)`; the table
        names every k-th slot and holds it for k steps (`--strides`, k = 1:
        a base flow that moves with every step; k > 1: a trajectory stored
        every k-th step, the base flow jumps every k steps; k = 0: every
        entry names the row of variant c -- the run of c, bit for bit, through
        the trajectory instance of the element kernel: what that instance
        costs in the loop)
  h<k>  (`--lerp k`) the resident loop about a trajectory STORED every k-th
        step (every k-th slot, uploaded), the row of the last stored time held
        -- a<k> with the trajectory a user who stores every k-th step has
  i<k>  the same trajectory interpolated linearly between its rows (weights
        beside the index table): a base flow that moves a little every step
  z<k>  the tables of h<k> with all-zero weights: the run of h<k> bit for bit
        through the interpolating instance of the element kernel (two gathers
        of V) -- what that instance costs in the loop
  b     what had to be done before: one `set_base_flow` per step (the slot's
        row from a host copy of the ensemble) and `run(1)`, `--steps-b` steps,
        wall clock; with the loops' solver options (captured graphs: every
        new base flow is a new graph key)
  b0    the same without graphs (`use_graph=0`)
  c     the constant-base loop: `set_base_flow` once, `run(steps)`

a and c: HIP events around `stp.run` (the `device_seconds` it returns), as
bench.py does; a window in which graphs were captured is repeated.  Beside
them the adoption itself: `ensemble_to_base` against `set_base_flow` of a
`BaseTrajectory` made of the downloaded slots (the same rows; wall clock, both
complete on return, best of three).  One JSON line per variant, mode and
repeat.
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


def _best(call, n=3):
    best = None
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def run_repeat(su, args, rep):
    import record_bench as rb
    from dolfin_navier_scipy_amd import convection
    femp = su.femp
    dbv = np.asarray(femp['dbcvals'], dtype=np.float64)
    NV = su.J.shape[1]
    steps = args.steps
    nslots = steps
    out = []
    fwd, cf, opts, close_fwd = su.stepper()
    lin, lcf, lopts, close_lin = su.stepper()
    try:
        # ---- the stored forward run
        fwd.run(args.spin, cf, opts)
        fwd.set_ensemble(list(range(steps)), nslots=nslots)
        secs, its, _ = fwd.run(steps, cf, opts)
        out.append(dict(variant='store', mode='nonlinear',
                        **rb._record(fwd, steps, secs, its)))
        E = fwd.ensemble()
        cv = lin._conv
        rng = np.random.default_rng(rep)
        w0 = 0.1*E[0] + 1e-3*rng.standard_normal(NV)
        for mode in args.modes.split(','):
            adj = mode == 'adjoint'
            cv.clear_base_flow()
            cv.set_dbcvals(np.zeros(dbv.size) if adj else dbv)

            def slot_of(k, stride=1):
                j = ((k//stride)*stride) % nslots if stride > 0 else 0
                return nslots - 1 - j if adj else j
            # ---- the adoption: device to device against the same rows uploaded
            t_d2d = _best(lambda: fwd.ensemble_to_base(cv, dbcvals=dbv,
                                                       adjoint=adj))
            traj = convection.BaseTrajectory(np.arange(nslots), E, dbv)
            t_h2d = _best(lambda: cv.set_base_flow(traj, adjoint=adj))
            out.append(dict(variant='adopt', mode=mode, nslots=nslots,
                            bytes=int(E.nbytes), d2d_seconds=t_d2d,
                            upload_seconds=t_h2d))
            order = ['a%d' % k for k in args.strides] + ['b', 'b0', 'c'] \
                + ['%s%d' % (v, k) for k in args.lerp for v in 'hiz']
            order = order[rep % len(order):] + order[:rep % len(order)]
            nograph = type(lopts).from_buffer_copy(lopts)
            nograph.use_graph = 0
            order = [v for v in order if v not in args.skip.split(',')]
            for variant in order:
                def restart(base):
                    cv.set_base_flow(base, adjoint=adj)
                    nfc0 = cv.apply(w0, scale=-1.0)
                    lin.set_state(w0, nfc_c=nfc0, nfc_o=nfc0)
                if variant[0] in 'hiz':
                    # every k-th slot stored (uploaded: the ensemble's slots
                    # are contiguous), the position moving with every step
                    k = int(variant[1:])
                    Ek = E[::k]
                    span = k*(Ek.shape[0] - 1)
                    cv.set_base_flow(convection.BaseTrajectory(
                        np.arange(Ek.shape[0]), Ek, dbv), adjoint=adj)
                    pos = [(span - n % span) if adj else n % span
                           for n in range(args.spin + 3*steps)]
                    rows = [p//k for p in pos]
                    wts = None if variant[0] == 'h' else \
                        [((p % k)/float(k) if variant[0] == 'i' else 0.0)
                         for p in pos]
                    cv.set_base_row(rows[0], 0.0 if wts is None else wts[0])
                    nfc0 = cv.apply(w0, scale=-1.0)
                    lin.set_state(w0, nfc_c=nfc0, nfc_o=nfc0)
                    cv.set_base_rows(rows, wts)
                    lin.run(args.spin, lcf, lopts)
                    secs, its, n = rb._timed_window(lin, lcf, lopts, steps)
                    rec = rb._record(lin, steps, secs, its)
                    rec.update(windows=n, stored_every=k,
                               interpolates=bool(cv.interpolates))
                elif variant.startswith('a'):
                    stride = int(variant[1:])
                    fwd.ensemble_to_base(cv, dbcvals=dbv, adjoint=adj)
                    cv.set_base_row(slot_of(0))
                    nfc0 = cv.apply(w0, scale=-1.0)
                    lin.set_state(w0, nfc_c=nfc0, nfc_o=nfc0)
                    # (one table for the spin-up and every window a capture
                    # may repeat)
                    cv.set_base_rows([slot_of(k, stride)
                                      for k in range(args.spin + 3*steps)])
                    lin.run(args.spin, lcf, lopts)
                    secs, its, n = rb._timed_window(lin, lcf, lopts, steps)
                    rec = rb._record(lin, steps, secs, its)
                    rec.update(windows=n, hold=stride)
                elif variant == 'c':
                    restart((E[slot_of(0)], dbv))
                    lin.run(args.spin, lcf, lopts)
                    secs, its, n = rb._timed_window(lin, lcf, lopts, steps)
                    rec = rb._record(lin, steps, secs, its)
                    rec.update(windows=n)
                else:
                    bopts = lopts if variant == 'b' else nograph
                    restart((E[slot_of(0)], dbv))
                    for k in range(args.spin):
                        cv.set_base_flow((E[slot_of(k)], dbv), adjoint=adj)
                        lin.run(1, lcf, bopts)
                    its = 0
                    t0 = time.perf_counter()
                    for k in range(args.steps_b):
                        cv.set_base_flow((E[slot_of(args.spin + k)], dbv),
                                         adjoint=adj)
                        its += lin.run(1, lcf, bopts)[1]
                    lin.vnorm()
                    secs = time.perf_counter() - t0
                    rec = dict(seconds=secs, steps_per_s=args.steps_b/secs,
                               iters=int(its), vnorm=lin.vnorm(),
                               steps_timed=args.steps_b)
                rec.update(variant=variant, mode=mode,
                           base_rows=cv.base_trajectory_rows)
                out.append(rec)
    finally:
        close_lin()
        close_fwd()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--modes', default='forward,adjoint')
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--steps-b', type=int, default=100)
    ap.add_argument('--strides', default='0,1,4')
    ap.add_argument('--lerp', default='',
                    help='storage strides k of the variants h<k>, i<k>, z<k>, '
                         'e.g. 4')
    ap.add_argument('--spin', type=int, default=64)
    ap.add_argument('--skip', default='',
                    help='variants to leave out, e.g. b,b0')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--refine', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    args.strides = [int(k) for k in args.strides.split(',') if k]
    args.lerp = [int(k) for k in args.lerp.split(',') if k]
    import record_bench as rb
    if args.refine > 0:
        su = rb.RefinedSetup(args.refine)
    else:
        import feedback_bench as fbb
        su = fbb.Setup()
    NP, NV = su.J.shape
    lines = []
    for rep in range(args.repeats):
        for rec in run_repeat(su, args, rep):
            rec.update(repeat=rep, refine=args.refine, NV=int(NV), NP=int(NP),
                       ncells=int(su.femp['V'].mesh.ncells), steps=args.steps,
                       spin=args.spin)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
