"""What a POD of the trajectory costs: the device-resident snapshot ensemble
(`ImexStepper.set_ensemble`, `.ensemble_gram`, `.ensemble_combine`) against the
way there was before it -- the recorder keeping the same steps, ONE download of
the `m x (NV + NP)` buffer, then the method of snapshots on the host -- on the
bench configuration (cylinder wake N=2, Re=100, dt=1/512, bench.py's solver
defaults, start from the Stokes state) and on the refined meshes
(`--refine R`, as scripts/record_bench.py).

One command per leg (profiles/r15_pod/README.md); `m = --steps`, every step of
the timed window is kept:

  --leg open    `run(m)` after the spin-up, nothing attached
  --leg pod     `run(m)` with the ensemble set (the copy node in every step),
                then `G = E M E^T` on the device (`m^2` doubles come back; the
                first call uploads `M`, a second one is timed as well),
                `SnapshotPOD.decompose` on the host and `coef @ E` on the
                device (`(r + 1) NV` doubles come back)
  --leg record  `run(m)` with a recorder snapshot of every step, ONE download,
                `G = S M S^T` by SciPy, `decompose`, `coef @ S` by NumPy: the
                same result by the route of the parent tree

Timing: HIP events around `stp.run` (the `device_seconds` it returns), as
bench.py does; everything behind the loop by the host clock, each piece stated
apart.  `gram_tflops` is the work of the tiles that are computed (`j >= i`: 2 x
256 x NV flops per tile) over the WALL time of the second `ensemble_gram` call,
SpMM, reduction and the download of `G` included: a lower bound of the rate of
`k_ens_gram` itself (its device time: a kernel trace of this leg).  Each leg is
repeated `--repeats` times from a fresh system; one JSON line per leg.
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

import record_bench as rb          # noqa: E402


def _pod(su, nmodes):
    from dolfin_navier_scipy_amd.fem import SnapshotPOD
    return SnapshotPOD(su.M, nmodes=nmodes)


def leg_open(su, m, spin, nmodes):
    return rb.leg_open(su, m, spin)


def leg_pod(su, m, spin, nmodes):
    stp, cf, opts, close = su.stepper()
    try:
        pod = _pod(su, nmodes)
        # (set before the spin-up: the graphs of the step with the copy node
        # are captured there; rows for up to three windows, see
        # record_bench._timed_window -- every window fills the same m slots)
        rows = spin + 3*m
        slots = np.array([-1]*spin + list(range(m))*3, dtype=np.int32)
        stp.set_ensemble(slots[:rows], nslots=m)
        stp.run(spin, cf, opts)
        secs, its, n = rb._timed_window(stp, cf, opts, m)
        out = rb._record(stp, m, secs, its)
        out['windows'] = n
        NV = su.J.shape[1]
        t0 = time.perf_counter()
        G = stp.ensemble_gram(pod.W)
        t1 = time.perf_counter()
        G2 = stp.ensemble_gram(pod.W)
        t2 = time.perf_counter()
        dec = pod.decompose(G)
        t3 = time.perf_counter()
        full = stp.ensemble_combine(dec['coef'])
        t4 = time.perf_counter()
        ntiles = (-(-m//16))*(-(-m//16) + 1)//2
        flops = 2.*256*NV*ntiles
        vl, _ = stp.get_state()
        out.update(
            gram_first_seconds=t1 - t0, gram_seconds=t2 - t1,
            decompose_seconds=t3 - t2, combine_seconds=t4 - t3,
            post_seconds=(t2 - t1) + (t3 - t2) + (t4 - t3),
            gram_tiles=ntiles, gram_flops=flops,
            gram_tflops=flops/(t2 - t1)/1e12,
            download_bytes=int(G.nbytes + full.nbytes),
            modes=int(dec['nmodes']), sigma=dec['sigma'][:4].tolist(),
            same_bits=bool(np.array_equal(G, G2)),
            symmetric=bool(np.array_equal(G, G.T)),
            last_slot_is_state=bool(np.array_equal(
                stp.ensemble(m - 1, 1)[0], vl[:, 0])),
            steps_per_s_with_post=m/(secs + (t2 - t1) + (t3 - t2)
                                     + (t4 - t3)))
    finally:
        close()
    return out


def leg_record(su, m, spin, nmodes):
    stp, cf, opts, close = su.stepper()
    try:
        pod = _pod(su, nmodes)
        stp.set_recorder(spin + 3*m, snap_slots='all')
        stp.run(spin, cf, opts)
        secs, its, n = rb._timed_window(stp, cf, opts, m)
        out = rb._record(stp, m, secs, its)
        out['windows'] = n
        first = spin + (n - 1)*m
        t0 = time.perf_counter()
        S, P = stp.record_snapshots(first, m)
        t1 = time.perf_counter()
        G = S @ (pod.W @ S.T)
        t2 = time.perf_counter()
        dec = pod.decompose(G)
        t3 = time.perf_counter()
        full = dec['coef'] @ S
        t4 = time.perf_counter()
        out.update(
            download_seconds=t1 - t0, gram_seconds=t2 - t1,
            decompose_seconds=t3 - t2, combine_seconds=t4 - t3,
            post_seconds=t4 - t0, download_bytes=int(S.nbytes + P.nbytes),
            modes=int(dec['nmodes']), sigma=dec['sigma'][:4].tolist(),
            full_norm=float(np.linalg.norm(full)),
            steps_per_s_with_post=m/(secs + t4 - t0))
    finally:
        close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=('open', 'pod', 'record'), required=True)
    ap.add_argument('--steps', type=int, default=400,
                    help='m: the steps of the timed window, all kept')
    ap.add_argument('--spin', type=int, default=64)
    ap.add_argument('--nmodes', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--refine', type=int, default=0)
    ap.add_argument('--label', default='')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from dolfin_navier_scipy_amd import _capi
    if _capi.device_count() < 1:
        raise SystemExit('no HIP device: nothing is measured without one')
    if args.refine > 0:
        su = rb.RefinedSetup(args.refine)
    else:
        import feedback_bench as fbb
        su = fbb.Setup()
    fn = dict(open=leg_open, pod=leg_pod, record=leg_record)[args.leg]
    reps = [fn(su, args.steps, args.spin, args.nmodes)
            for _ in range(args.repeats)]
    rates = [r['steps_per_s'] for r in reps]
    out = dict(leg=args.leg, label=args.label, m=args.steps, spin=args.spin,
               refine=args.refine, NV=int(su.J.shape[1]),
               unknowns=int(su.J.shape[0] + su.J.shape[1]),
               device=_capi.device_name(0), steps_per_s=rates,
               best=max(rates), worst=min(rates),
               spread_rel=(max(rates) - min(rates))/max(rates),
               with_post=[r.get('steps_per_s_with_post') for r in reps],
               post_seconds=[r.get('post_seconds') for r in reps],
               repeats=reps)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
