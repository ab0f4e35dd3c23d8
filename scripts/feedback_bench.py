"""Closed-loop (observer feedback) against open-loop stepping rates on the
bench configuration: cylinder wake N=2, Re=100, dt=1/512, bench.py's solver
defaults, start from the Stokes state.

One command per leg (profiles/r07_feedback/README.md):

  --leg host      closed loop through a plain Python `dynamic_rhs`-style
                  closure: per step `get_state`, NumPy observer, `set_rhs`,
                  synchronous `step` -- what a code base without the device
                  observer can do (no API newer than `ImexStepper.step`)
  --leg open      open-loop resident headline: `run(steps)` after the spin-up
  --leg resident  closed loop with the observer on the device
                  (`ImexStepper.set_feedback`): `run(steps)` after the spin-up

Timing: HIP events around `stp.run` (the `device_seconds` it returns), as
bench.py does; the host leg, which has no `run`, by the host clock around the
loop, whose every step ends in a synchronise.  Each leg is repeated
`--repeats` times from the same start; one JSON line per leg.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOXES = ((0.55, 0.10), (0.55, 0.20), (0.55, 0.30))
BOX_HALF = (0.12, 0.055)
BUMPS = ((0.32, 0.14), (0.32, 0.26))
SIGMA, RADIUS = 0.03, 0.085


def sensors_actuators(th, invinds, M):
    """box means of the vertical velocity in the wake / `M`-weighted Gaussian
    bumps behind the obstacle (as tests/feedback_setup.py)"""
    invinds = np.asarray(invinds)
    node, comp = invinds//2, invinds % 2
    xy = th.nodecoords[node]
    rows, cols, vals = [], [], []
    for k, (cx, cy) in enumerate(BOXES):
        idx = np.flatnonzero((comp == 1)
                             & (np.abs(xy[:, 0] - cx) <= BOX_HALF[0])
                             & (np.abs(xy[:, 1] - cy) <= BOX_HALF[1]))
        rows += [k]*idx.size
        cols += idx.tolist()
        vals += [1./idx.size]*idx.size
    C = sps.csr_matrix((vals, (rows, cols)), shape=(len(BOXES), invinds.size))
    gcols = []
    for (cx, cy) in BUMPS:
        d2 = (xy[:, 0] - cx)**2 + (xy[:, 1] - cy)**2
        g = np.where((comp == 1) & (d2 <= RADIUS**2),
                     np.exp(-d2/(2*SIGMA**2)), 0.)
        gcols.append(sps.csr_matrix(g.reshape((-1, 1))))
    B = sps.csr_matrix(sps.csr_matrix(M) @ sps.hstack(gcols).tocsr())
    B.eliminate_zeros()
    return C, B


def observer(hN=12, Ny=3, Nu=2, seed=107):
    rng = np.random.default_rng(seed)
    return dict(ha=-5.*np.eye(hN) + rng.standard_normal((hN, hN)),
                hb=rng.standard_normal((hN, Ny)),
                hc=rng.standard_normal((Nu, hN)),
                inihx=0.1*rng.standard_normal(hN),
                dvec=rng.standard_normal(hN))


class Setup(object):
    def __init__(self):
        import bench
        from dolfin_navier_scipy_amd import saddle
        self.femp, sm, self.rhsd = bench.build_problem(N=2, Re=100.)
        self.M, self.A, self.J = (sm[k].tocsr() for k in 'MAJ')
        self.dt = 1./512
        self.dflt = bench.DEFAULTS
        self.v0, _, _ = bench.initial_state(
            sm, self.rhsd, lambda F, Jm: saddle.SaddleSystem(F, Jm))
        self.C, self.B = sensors_actuators(self.femp['V'],
                                           self.femp['invinds'], self.M)
        self.obs = observer()

    def stepper(self):
        from dolfin_navier_scipy_amd import saddle, convection
        M, A, J, dt, dflt = self.M, self.A, self.J, self.dt, self.dflt
        femp = self.femp
        system = saddle.SaddleSystem((M + .5*dt*A).tocsr(), J)
        system.setup_precond(cheb_degree=dflt['cheb'], schur='dense',
                             fp32_store=bool(dflt['fp32']),
                             drop_tol=dflt['drop'],
                             factorization=dflt['fact'])
        stp = saddle.ImexStepper(system, (M - .5*dt*A).tocsr())
        cvop = convection.ConvectionP2.from_taylor_hood(
            femp['V'], femp['invinds'], femp['dbcinds'], femp['dbcvals'])
        nfc0 = cvop.apply(self.v0, scale=-1.0)
        stp.set_state(self.v0, nfc_c=nfc0, nfc_o=nfc0)
        stp.set_rhs(dt*self.rhsd['fv'], self.rhsd['fp'])
        stp.set_convection(cvop, scale=-1.0)
        cf = saddle.ImexStepper.coeffs(a_c=1., cn_c=1.5*dt, cn_o=-.5*dt,
                                       pscale=-1./dt,
                                       extrapolate=dflt['extrap'])
        opts = saddle.solve_opts(method='gmres', rtol=dflt['rtol'],
                                 maxiter=400, restart=60, check_every=2,
                                 use_graph=True, reorth=dflt['reorth'])

        def close():
            stp.close()
            cvop.close()
            system.close()
        return stp, cf, opts, close


def leg_open(su, steps, spin):
    stp, cf, opts, close = su.stepper()
    try:
        stp.run(spin, cf, opts)
        secs, its, _ = stp.run(steps, cf, opts)
        rec = dict(stp.last_run)
        counters = stp.step_counters()
        vn = stp.vnorm()
    finally:
        close()
    return dict(seconds=secs, steps_per_s=steps/secs, iters=int(its),
                run=rec, step_counters=counters, vnorm=vn)


def leg_resident(su, steps, spin):
    stp, cf, opts, close = su.stepper()
    o, dt = su.obs, su.dt
    try:
        stp.set_feedback(su.C, su.B, o['ha'], o['hb'], o['hc'], c_n=.5,
                         c_c=.5, dt=dt)
        stp.set_feedback_state(o['inihx'], np.zeros(12), o['hc'] @ o['inihx'])
        times = dt*np.arange(spin + steps)
        stp.set_feedback_table(spin + steps,
                               np.sin(7*times)[:, None]*o['dvec'][None, :])
        stp.run(spin, cf, opts)
        secs, its, _ = stp.run(steps, cf, opts)
        rec = dict(stp.last_run)
        counters = stp.step_counters()
        vn = stp.vnorm()
        _, ulog = stp.feedback_log()
    finally:
        close()
    return dict(seconds=secs, steps_per_s=steps/secs, iters=int(its),
                run=rec, step_counters=counters, vnorm=vn,
                u_last=ulog[-1].tolist())


def leg_host(su, steps, spin):
    """the same closed loop with the observer in a Python closure"""
    stp, cf, opts, close = su.stepper()
    o, dt, C, B = su.obs, su.dt, su.C, su.B
    g0 = dt*su.rhsd['fv']
    mem = dict(hx=o['inihx'].copy(), flast=np.zeros(12), k=0)
    mem['u'] = o['hc'] @ mem['hx']

    def dynamic_rhs(vc):
        y = C @ vc[:, 0]
        f = o['ha'] @ mem['hx'] + o['hb'] @ y \
            + np.sin(7*dt*mem['k'])*o['dvec']
        hxn = mem['hx'] + 1.5*dt*f - .5*dt*mem['flast']
        un = o['hc'] @ hxn
        out = .5*dt*(B @ (un + mem['u']))
        mem.update(hx=hxn, flast=f, u=un, k=mem['k'] + 1)
        return out.reshape((-1, 1))

    def step():
        v, _ = stp.get_state()
        stp.set_rhs(g0 + dynamic_rhs(v), None)
        stp.step(cf, opts=opts)
    try:
        for _ in range(spin):
            step()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        stp.get_state()
        secs = time.perf_counter() - t0
        vn = stp.vnorm()
    finally:
        close()
    return dict(seconds=secs, steps_per_s=steps/secs, vnorm=vn,
                u_last=mem['u'].tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=('host', 'open', 'resident'),
                    required=True)
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--spin', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--label', default='')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from dolfin_navier_scipy_amd import _capi
    if _capi.device_count() < 1:
        raise SystemExit('no HIP device: nothing is measured without one')
    su = Setup()
    fn = dict(host=leg_host, open=leg_open, resident=leg_resident)[args.leg]
    reps = [fn(su, args.steps, args.spin) for _ in range(args.repeats)]
    rates = [r['steps_per_s'] for r in reps]
    out = dict(leg=args.leg, label=args.label, steps=args.steps,
               spin=args.spin, device=_capi.device_name(0),
               steps_per_s=rates, best=max(rates), worst=min(rates),
               spread_rel=(max(rates) - min(rates))/max(rates),
               repeats=reps)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
