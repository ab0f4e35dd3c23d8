"""Boundary feedback (an observer whose output is the rotation rate of the
cylinder) through the three routes of `time_int_utils.cnab`, on the bench
configuration: cylinder wake N=2, Re=100, dt=1/512, bench.py's solver
defaults, start from the Stokes state.  An observer of 12 states, one sensor
row (the mean vertical velocity in a box in the wake), one input: the rotation
of the cylinder (`b = s_mat u`, the tangential unit velocity on its dofs; the
literal `applybcs`, as `solve_nse` has it by default).

One command per leg (profiles/r17_boundary_feedback/README.md), one fresh
process each:

  --leg resident  `getbcs` is the `BoundaryFeedback`: whole slices on the
                  device (`k_lti_bc_step` in front of every step)
  --leg host      the same law as a plain closure: `getbcs` reads the state,
                  every step is a host round trip -- the only route before
  --leg open      `bcs_time_only`: a prescribed rotation, tabulated ahead

`--attach budget` (profiles/r18_closed_loop_budget/README.md) adds drag, lift
and torque of the cylinder (`functionals`) and the energy budget with moving
Dirichlet values (`quadratics`, `energy_budget(moving=True)`) to any leg: on
the device beside the resident feedback (they read the operator's Dirichlet
table) and in the `open` leg (tables of their own), through `evaluate` on the
host in the `host` leg.

Timing: the host clock between two `savevp` calls of ONE `cnab` run over
`warmup + steps` loop steps, cut into slices of `warmup` steps: the call behind
the first slice and the call behind the last one (a resident slice hands the
states over when it is through, the host path after every step; both have
synchronised by then).  So the rate covers all a slice costs -- tabulation,
upload, replay, collection --, not the set-up and not the Heun start.  Each
leg is repeated `--repeats` times; one JSON line per leg.
"""
import argparse
import json
import os
import sys
import time as _time

import numpy as np
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOX, BOX_HALF = (0.55, 0.20), (0.12, 0.055)
GAIN = 0.5


class Setup(object):
    def __init__(self, refine=0):
        import bench
        from dolfin_navier_scipy_amd import saddle, fem
        self.femp, sm, self.rhsd = bench.build_problem(N=2, Re=100.,
                                                       refine=refine)
        self.M, self.A, self.J = (sm[k].tocsr() for k in 'MAJ')
        self.dt = 1./512
        self.v0, self.p0, _ = bench.initial_state(
            sm, self.rhsd, lambda F, Jm: saddle.SaddleSystem(F, Jm))
        th = self.th = self.femp['V']
        self.inv = np.asarray(self.femp['invinds'])
        dbcinds = np.asarray(self.femp['dbcinds'])
        dbcvals = np.asarray(self.femp['dbcvals'], dtype=np.float64)
        # the cylinder's dofs are the controlled ones: tangential unit velocity
        nodes = fem.cylinder_nodes(th)
        oncyl = np.isin(dbcinds//2, nodes)
        assert oncyl.sum() == 2*nodes.size
        self.statinds, self.statvals = dbcinds[~oncyl], dbcvals[~oncyl]
        self.cntinds = dbcinds[oncyl]
        xy = th.nodecoords[self.cntinds//2] - np.array([0.2, 0.2])
        r = np.linalg.norm(xy, axis=1)
        self.shape = np.where(self.cntinds % 2 == 0, -xy[:, 1], xy[:, 0])/r
        # one sensor row over the FULL dofs
        node, comp = self.inv//2, self.inv % 2
        nxy = th.nodecoords[node]
        idx = np.flatnonzero((comp == 1)
                             & (np.abs(nxy[:, 0] - BOX[0]) <= BOX_HALF[0])
                             & (np.abs(nxy[:, 1] - BOX[1]) <= BOX_HALF[1]))
        self.C = sps.csr_matrix((np.full(idx.size, 1./idx.size),
                                 (np.zeros(idx.size, dtype=int),
                                  self.inv[idx])), shape=(1, th.vdim))
        rng = np.random.default_rng(117)
        self.obs = dict(ha=-5.*np.eye(12) + rng.standard_normal((12, 12)),
                        hb=rng.standard_normal((12, 1)),
                        hc=GAIN*rng.standard_normal((1, 12)),
                        inihx=0.1*rng.standard_normal((12, 1)),
                        dvec=rng.standard_normal((12, 1)))

    def feedback(self):
        from dolfin_navier_scipy_amd import time_int_utils as tiu
        o = self.obs
        return tiu.BoundaryFeedback(
            self.C, sps.csr_matrix(self.shape.reshape((-1, 1))), o['ha'],
            o['hb'], o['hc'], o['inihx'], invinds=self.inv,
            drift=lambda t: np.sin(7*t)*o['dvec'])

    def appndbcs(self, vvec, bcs):
        full = np.full((self.th.vdim, 1), np.nan)
        full[self.inv] = vvec
        full[self.statinds, 0] = self.statvals
        full[self.cntinds, 0] = bcs
        return full

    def attachments(self):
        """drag, lift, torque of the cylinder and the moving energy budget,
        built for the loop's Dirichlet dofs (static, then the cylinder's)"""
        from dolfin_navier_scipy_amd import fem
        femp = dict(invinds=self.inv, nu=self.femp['nu'],
                    dbcinds=np.concatenate([self.statinds, self.cntinds]),
                    dbcvals=np.concatenate([self.statvals, 0.*self.shape]))
        fn = fem.boundary_forces(self.th, femp) \
            + fem.boundary_torque(self.th, femp)
        return dict(functionals=fn,
                    quadratics=fem.energy_budget(self.th, femp, moving=True))

    def run(self, leg, warmup, steps, attach='none'):
        """one `cnab` call; the host seconds of the `steps` loop steps behind
        the first `warmup`"""
        from dolfin_navier_scipy_amd import time_int_utils as tiu
        from dolfin_navier_scipy_amd import convection
        import bench
        dflt = bench.DEFAULTS
        NP, NV = self.J.shape
        zv, zp = np.zeros((NV, 1)), np.zeros((NP, 1))
        fb = self.feedback()
        if steps % warmup:
            raise SystemExit('--steps must be a multiple of --warmup')
        nts = warmup + steps + 2
        trange = self.dt*np.arange(nts + 1)
        marks = {float(trange[warmup + 1]): None, float(trange[-1]): None}
        resident = dict(static_dbcvals=self.statvals.tolist(),
                        savevp_times=list(marks))

        if attach == 'budget':
            resident.update(self.attachments())

        def savevp(vvec, pvec, time=None):
            if time in marks:
                marks[time] = _time.perf_counter()
        if leg == 'resident':
            getbcs = fb
        elif leg == 'host':
            def getbcs(time, vvec, pvec, mode='abtwo'):
                return fb(time, vvec, pvec, mode=mode)
        else:
            u0 = float((self.obs['hc'] @ self.obs['inihx'])[0, 0])
            resident.update(bcs_time_only=True)

            def getbcs(time, vvec, pvec, mode=None):
                return (u0*np.cos(7*time)*self.shape).tolist()
        cvop = convection.ConvectionP2.from_taylor_hood(
            self.th, self.inv, np.concatenate([self.statinds, self.cntinds]),
            np.concatenate([self.statvals, 0.*self.shape]))
        dbi = np.concatenate([self.statinds, self.cntinds])

        def f_vdp(vfull):           # (the Heun start: values from the vector)
            ve = np.asarray(vfull).reshape(-1)
            cvop.set_dbcvals(ve[dbi])
            return cvop.apply(ve[self.inv], scale=-1.0)
        kw = dict(trange=trange, inivel=self.v0,
                  ntimeslices=(warmup + steps)//warmup,
                  f_vdp=f_vdp,
                  inip=-self.p0, M=self.M, A=self.A, J=self.J,
                  bcs_ini=getbcs(0., None, None, mode='init'),
                  f_tdp=lambda t: self.rhsd['fv'],
                  g_tdp=lambda t: self.rhsd['fp'], scalep=-1., getbcs=getbcs,
                  applybcs=lambda b: (-zv, -zp, zv.copy()),
                  appndbcs=self.appndbcs, savevp=savevp,
                  check_ff_maxv=1e8, verbose=False,
                  solver=dict(rtol=dflt['rtol'], cheb_degree=dflt['cheb'],
                              extrapolate=dflt['extrap'],
                              drop_tol=dflt['drop'],
                              factorization=dflt['fact'],
                              reorth=dflt['reorth']),
                  device_convection=cvop, invinds=self.inv,
                  resident=resident)
        try:
            v, p, ff = tiu.cnab(**kw)
        finally:
            cvop.close()
        last = tiu.LAST_RUN
        u = last.get('feedback_u')
        t_a, t_b = (marks[k] for k in sorted(marks))
        rows = {k: (None if last.get(k) is None
                    else np.asarray(last[k])[-1].tolist())
                for k in ('functionals', 'quadratics')}
        return dict(seconds=t_b - t_a, steps_per_s=steps/(t_b - t_a),
                    ffflag=int(ff), feedback=last['feedback'],
                    functionals_on=last.get('functionals_on'),
                    quadratics_on=last.get('quadratics_on'),
                    functionals_last=rows['functionals'],
                    quadratics_last=rows['quadratics'],
                    run_calls=last['run_calls'],
                    krylov_steps=int(last['krylov_steps']),
                    vnorm=float(np.linalg.norm(v)),
                    u_last=None if u is None or not len(u)
                    else np.asarray(u)[-1].tolist())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=('resident', 'host', 'open'),
                    required=True)
    ap.add_argument('--attach', choices=('none', 'budget'), default='none')
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--warmup', type=int, default=40)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--refine', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from dolfin_navier_scipy_amd import _capi
    if _capi.device_count() < 1:
        raise SystemExit('no HIP device: nothing is measured without one')
    su = Setup(refine=args.refine)
    reps = []
    for _ in range(args.repeats):
        reps.append(su.run(args.leg, args.warmup, args.steps, args.attach))
    rates = [r['steps_per_s'] for r in reps]
    out = dict(leg=args.leg, attach=args.attach, steps=args.steps, warmup=args.warmup,
               refine=args.refine, device=_capi.device_name(0),
               unknowns=int(sum(su.J.shape)), steps_per_s=rates,
               best=max(rates), worst=min(rates), repeats=reps)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
