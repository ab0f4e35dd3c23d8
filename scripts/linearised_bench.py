"""Stepping rates of the explicit CNAB loop with a linearised / adjoint
convection operator (`ConvectionP2.set_base_flow`) beside the nonlinear loop,
on the bench configuration (cylinder wake N=2, Re=100, dt=1/512, bench.py's
solver defaults) and, `--refine R`, on the mesh refined R times (the stepper of
refined_bench.py: multigrid Schur block, dt = 1/(512 2^R)).

  --legs nonlinear,forward,adjoint   (default: all three, alternating)

  nonlinear   `run(steps)` after the spin-up, N(v)v: the loop as it was (no API
              newer than `ImexStepper.run`, so the parent tree runs it too)
  forward     the same stepper, the operator linearised about the base flow:
              L(V)w by `k_conv_lin_cells<false>` in a launch of its own in
              front of the step (no six-node step)
  adjoint     the transposed cell statements, `k_conv_lin_cells<true>`; the
              operator's own Dirichlet values are zero

The base flow is the state the nonlinear leg starts from with the problem's
Dirichlet values (N=2: the Stokes state; refined: rest inside), the
perturbation starts from a tenth of it plus 1e-3 x a seeded normal field.
Timing: HIP events around `stp.run` (the `device_seconds` it returns), as
bench.py does; a window in which graphs were captured is repeated.  Each leg
is repeated `--repeats` times from a fresh system, the legs alternating; one
JSON line per repeat.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))


def run_leg(su, leg, steps, spin, seed=0):
    import record_bench as rb
    stp, cf, opts, close = su.stepper()
    try:
        cvop, femp = stp._conv, su.femp
        NV = su.J.shape[1]
        v0 = getattr(su, 'v0', None)
        v0 = np.zeros(NV) if v0 is None else np.asarray(v0).reshape(-1)
        if leg != 'nonlinear':
            adj = leg == 'adjoint'
            if adj:
                cvop.set_dbcvals(np.zeros(femp['dbcvals'].size))
            cvop.set_base_flow((v0, femp['dbcvals']), adjoint=adj)
            rng = np.random.default_rng(seed)
            w0 = 0.1*v0 + 1e-3*rng.standard_normal(NV)
            nfc0 = cvop.apply(w0, scale=-1.0)
            stp.set_state(w0, nfc_c=nfc0, nfc_o=nfc0)
        stp.run(spin, cf, opts)
        secs, its, n = rb._timed_window(stp, cf, opts, steps)
        out = rb._record(stp, steps, secs, its)
        out.update(windows=n, mode=str(cvop.linearised))
    finally:
        close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='nonlinear,forward,adjoint')
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--spin', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--refine', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import record_bench as rb
    if args.refine > 0:
        su = rb.RefinedSetup(args.refine)
    else:
        import feedback_bench as fbb
        su = fbb.Setup()
    NP, NV = su.J.shape
    lines = []
    for rep in range(args.repeats):
        for leg in args.legs.split(','):
            rec = run_leg(su, leg, args.steps, args.spin, seed=rep)
            rec.update(leg=leg, repeat=rep, refine=args.refine, NV=int(NV),
                       NP=int(NP), ncells=int(su.femp['V'].mesh.ncells),
                       steps=args.steps, spin=args.spin)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
