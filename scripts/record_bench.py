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
  --leg moving_open    the cylinder rotates, `omega(t)` tabulated: rhs table
                  and Dirichlet table of the convection operator as
                  `cnab(resident=dict(bcs_time_only=True))` sets them, nothing
                  else attached (no API newer than `set_dbc_table`, so the
                  parent tree runs it too)
  --leg moving_forces  the same with drag, lift, torque and dp of every step on
                  the device (`set_functionals(..., dbc_table=)`), then ONE
                  download of the rows
  --leg moving_host    what there is without the moving-boundary functionals: a
                  device snapshot of every step, ONE download, then
                  `MomentumFunctionals.evaluate(..., dbc=, dbc_prev=)` per
                  step on the host (profiles/r12_functionals_bc/README.md)
  --leg stats     `run(steps)` with the flow statistics on the device (one bin,
                  `fem.component_pairs` of the whole mesh:
                  `ImexStepper.set_statistics`), then ONE download of the sums
  --leg stats_by_record  what there is without them: a device snapshot of
                  every step, ONE download, the same sums by NumPy
  --leg stats_stepwise   `run(1)` + `get_state()` + `FlowStatistics.add` per
                  step (profiles/r13_statistics/README.md)
  --leg quad      `run(steps)` with the energy budget of every step on the device
                  (kinetic energy, dissipation rate, its rate and the M-norm of
                  dv/dt: `fem.energy_budget`, `ImexStepper.set_quadratics`),
                  then ONE download of the rows
  --leg quad_by_record  what there is without it: a device snapshot of every
                  step, ONE download, `QuadraticFunctionals.evaluate` per step
  --leg quad_stepwise   `run(1)` + `get_state()` + `evaluate` per step
                  (profiles/r14_quadratics/README.md)
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


class _Rotation(object):
    """the cylinder's dofs carry `omega(t) (-(y - yc), x - xc)`: the tables of
    `rows` steps from t = 0 (right-hand sides as `cnab` forms them, Dirichlet
    values of the operator's order with one row more: the values behind the
    last step) and a convection operator of the leg's own to carry them"""

    def __init__(self, su, stp, rows):
        from dolfin_navier_scipy_amd import fem, convection
        femp, dt = su.femp, getattr(su, 'dt', 1./512)
        th, inv = femp['V'], np.asarray(femp['invinds'])
        self.dbi = np.asarray(femp['dbcinds'], dtype=np.int64)
        nodes = fem.cylinder_nodes(th)
        pos = {int(d): k for k, d in enumerate(self.dbi)}
        cyl = np.array([[pos[2*n], pos[2*n + 1]] for n in nodes]).reshape(-1)
        xy = th.nodecoords[nodes]
        shape = np.stack([-(xy[:, 1] - 0.2), xy[:, 0] - 0.2],
                         axis=1).reshape(-1)
        base = np.asarray(femp['dbcvals'], dtype=np.float64).reshape(-1)
        times = dt*np.arange(rows + 1)
        self.tab = np.tile(base, (rows + 1, 1))
        self.tab[:, cyl] = np.outer(2.*np.sin(2*np.pi*times/0.25), shape)
        st = th.stokes_mats(nu=femp['nu'])
        aux = np.zeros((th.vdim, rows + 1))
        aux[self.dbi[cyl], :] = self.tab[:, cyl].T
        bfv = -(st['A'] @ aux)[inv, :].T                  # (rows + 1, NV)
        mbc = (st['M'] @ aux)[inv, :].T
        bfp = -(st['J'] @ aux).T
        fv, fp = su.rhsd['fv'][:, 0], su.rhsd['fp'][:, 0]
        gv = dt*fv[None, :] - (mbc[1:] - mbc[:-1]) + .5*dt*(bfv[1:] + bfv[:-1])
        gp = fp[None, :] + bfp[1:]
        self.cvop = convection.ConvectionP2.from_taylor_hood(
            th, inv, self.dbi, base)
        stp.set_convection(self.cvop, scale=-1.0)
        stp.set_rhs_table(gv, gp)
        self.cvop.set_dbc_table(self.tab[:rows])
        self.nodes, self.rows = nodes, rows

    def functionals(self, su):
        from dolfin_navier_scipy_amd import fem
        th, femp = su.femp['V'], su.femp
        return fem.boundary_forces(th, femp, nodes=self.nodes) \
            + fem.boundary_torque(th, femp, nodes=self.nodes) \
            + fem.pressure_difference(th, (0.15, 0.2), (0.25, 0.2))

    def close(self, stp):
        stp.set_convection(None)
        self.cvop.close()


def _leg_moving(su, steps, spin, what):
    stp, cf, opts, close = su.stepper()
    rot = None
    try:
        dt = getattr(su, 'dt', 1./512)
        rows = spin + 3*steps
        rot = _Rotation(su, stp, rows)
        fn = rot.functionals(su) if what != 'open' else None
        if what == 'host':
            stp.set_recorder(rows, snap_slots='all')
        if what == 'forces':
            stp.set_functionals(fn, rows, dt, dbc_table=rot.tab)
        stp.run(spin, cf, opts)
        secs, its, n = _timed_window(stp, cf, opts, steps)
        out = _record(stp, steps, secs, its)
        out['windows'] = n
        spin += (n - 1)*steps
        if what == 'forces':
            t0 = time.perf_counter()
            got = stp.get_functionals(spin, steps)
            dl = time.perf_counter() - t0
            out.update(download_seconds=dl,
                       steps_per_s_with_download=steps/(secs + dl),
                       names=fn.names, row_last=got[-1].tolist(),
                       body_cells=int(fn.cells[0].size))
        if what == 'host':
            t0 = time.perf_counter()
            v, p = stp.record_snapshots(spin - 1, steps + 1)
            dl = time.perf_counter() - t0
            got = np.empty((steps, fn.nF))
            for k in range(steps):
                r = spin + k
                got[k] = fn.evaluate(v[k + 1], v[k], p[k + 1], dt,
                                     dbc=rot.tab[r + 1], dbc_prev=rot.tab[r])
            ev = time.perf_counter() - t0 - dl
            out.update(download_seconds=dl, evaluate_seconds=ev,
                       steps_per_s_with_download=steps/(secs + dl + ev),
                       names=fn.names, row_last=got[-1].tolist())
    finally:
        if rot is not None:
            rot.close(stp)
        close()
    return out


def leg_moving_open(su, steps, spin):
    return _leg_moving(su, steps, spin, 'open')


def leg_moving_forces(su, steps, spin):
    return _leg_moving(su, steps, spin, 'forces')


def leg_moving_host(su, steps, spin):
    return _leg_moving(su, steps, spin, 'host')


def _flow_statistics(su):
    from dolfin_navier_scipy_amd import fem
    return fem.FlowStatistics(pairs=fem.component_pairs(
        su.femp['V'], su.femp['invinds']))


def leg_stats(su, steps, spin):
    stp, cf, opts, close = su.stepper()
    try:
        fs = _flow_statistics(su)
        # (set before the spin-up, rows for up to three windows: as
        # _leg_recorded; the spin-up and repeated windows go into no bin)
        rows = spin + 3*steps
        stp.set_statistics(-np.ones(rows, dtype=np.int32), nbins=1,
                           pairs=fs.pairs)
        stp.run(spin, cf, opts)
        for n in range(1, 4):
            bins = -np.ones(rows, dtype=np.int32)
            bins[:steps] = 0
            # (the same buffers: the graphs of the spin-up are replayed)
            stp.set_statistics(bins, nbins=1, pairs=fs.pairs, reset=True)
            secs, its, _ = stp.run(steps, cf, opts)
            if stp.last_run['captures'] == 0:
                break
        out = _record(stp, steps, secs, its)
        out['windows'] = n
        t0 = time.perf_counter()
        sums = stp.statistics()
        dl = time.perf_counter() - t0
        fs.add_sums(sums)
        nbytes = sum(int(a.nbytes) for a in sums.values())
        out.update(download_seconds=dl, download_bytes=nbytes,
                   steps_per_s_with_download=steps/(secs + dl),
                   counts=fs.counts.tolist(), npairs=int(fs.pairs.shape[0]),
                   mean_v_max=float(np.abs(fs.mean()[0]).max()),
                   cov_max=float(np.abs(fs.covariance()).max()))
    finally:
        close()
    return out


def leg_stats_by_record(su, steps, spin):
    stp, cf, opts, close = su.stepper()
    try:
        fs = _flow_statistics(su)
        stp.set_recorder(spin + 3*steps, snap_slots='all')
        stp.run(spin, cf, opts)
        secs, its, n = _timed_window(stp, cf, opts, steps)
        out = _record(stp, steps, secs, its)
        out['windows'] = n
        spin += (n - 1)*steps
        t0 = time.perf_counter()
        v, p = stp.record_snapshots(spin, steps)
        dl = time.perf_counter() - t0
        x = np.hstack([v, p])
        fs.add_sums(dict(
            counts=[steps], s1_v=v.sum(axis=0)[None, :],
            s1_p=p.sum(axis=0)[None, :], s2_v=(v*v).sum(axis=0)[None, :],
            s2_p=(p*p).sum(axis=0)[None, :],
            sx=(x[:, fs.pairs[:, 0]]*x[:, fs.pairs[:, 1]]).sum(axis=0)[None, :]))
        ev = time.perf_counter() - t0 - dl
        out.update(download_seconds=dl, evaluate_seconds=ev,
                   download_bytes=int(v.nbytes + p.nbytes),
                   steps_per_s_with_download=steps/(secs + dl + ev),
                   counts=fs.counts.tolist(),
                   mean_v_max=float(np.abs(fs.mean()[0]).max()),
                   cov_max=float(np.abs(fs.covariance()).max()))
    finally:
        close()
    return out


def leg_stats_stepwise(su, steps, spin):
    stp, cf, opts, close = su.stepper()
    try:
        fs = _flow_statistics(su)
        stp.run(spin, cf, opts)
        t0 = time.perf_counter()
        for k in range(steps):
            stp.run(1, cf, opts)
            v, p = stp.get_state()
            fs.add(v, p, float(k))
        secs = time.perf_counter() - t0
        out = dict(seconds=secs, steps_per_s=steps/secs, vnorm=stp.vnorm(),
                   counts=fs.counts.tolist(),
                   mean_v_max=float(np.abs(fs.mean()[0]).max()),
                   cov_max=float(np.abs(fs.covariance()).max()))
    finally:
        close()
    return out


def leg_quad(su, steps, spin):
    from dolfin_navier_scipy_amd import fem
    stp, cf, opts, close = su.stepper()
    try:
        qf = fem.energy_budget(su.femp['V'], su.femp)
        dt = getattr(su, 'dt', 1./512)
        # (set before the spin-up, rows for up to three windows: as
        # _leg_recorded)
        stp.set_quadratics(qf, spin + 3*steps, dt)
        stp.run(spin, cf, opts)
        secs, its, n = _timed_window(stp, cf, opts, steps)
        out = _record(stp, steps, secs, its)
        out['windows'] = n
        spin += (n - 1)*steps
        t0 = time.perf_counter()
        rows = stp.get_quadratics(spin, steps)
        dl = time.perf_counter() - t0
        # (what crosses the bus: every workgroup's share of every row, the
        # getter sums them.  What the kernel must read per step: the matrices
        # -- 12 bytes per non-zero, 4 per row -- and the two velocities)
        NV = qf.NV
        grid = stp.quadratics_grid()
        nnz = sum(int(m.nnz) for m in qf.mats)
        out.update(download_seconds=dl,
                   download_bytes=int(steps*grid*qf.nQ*8),
                   steps_per_s_with_download=steps/(secs + dl),
                   rows_bytes=int(rows.nbytes), workgroups=grid,
                   kernel_bytes_per_step=int(12*nnz + 4*qf.nM*(NV + 1)
                                             + 16*NV),
                   nnz=nnz, names=qf.names, row_last=rows[-1].tolist())
    finally:
        close()
    return out


def leg_quad_by_record(su, steps, spin):
    from dolfin_navier_scipy_amd import fem
    stp, cf, opts, close = su.stepper()
    try:
        qf = fem.energy_budget(su.femp['V'], su.femp)
        dt = getattr(su, 'dt', 1./512)
        stp.set_recorder(spin + 3*steps, snap_slots='all')
        stp.run(spin, cf, opts)
        secs, its, n = _timed_window(stp, cf, opts, steps)
        out = _record(stp, steps, secs, its)
        out['windows'] = n
        spin += (n - 1)*steps
        t0 = time.perf_counter()
        # (one snapshot more: the state before the first step of the window)
        v, p = stp.record_snapshots(spin - 1, steps + 1)
        dl = time.perf_counter() - t0
        rows = np.array([qf.evaluate(v[k + 1], v[k], dt)
                         for k in range(steps)])
        ev = time.perf_counter() - t0 - dl
        out.update(download_seconds=dl, evaluate_seconds=ev,
                   download_bytes=int(v.nbytes + p.nbytes),
                   steps_per_s_with_download=steps/(secs + dl + ev),
                   names=qf.names, row_last=rows[-1].tolist())
    finally:
        close()
    return out


def leg_quad_stepwise(su, steps, spin):
    from dolfin_navier_scipy_amd import fem
    stp, cf, opts, close = su.stepper()
    try:
        qf = fem.energy_budget(su.femp['V'], su.femp)
        dt = getattr(su, 'dt', 1./512)
        stp.run(spin, cf, opts)
        vprev = stp.get_state()[0][:, 0]
        rows = np.empty((steps, qf.nQ))
        t0 = time.perf_counter()
        for k in range(steps):
            stp.run(1, cf, opts)
            v, p = stp.get_state()
            rows[k] = qf.evaluate(v[:, 0], vprev, dt)
            vprev = v[:, 0]
        secs = time.perf_counter() - t0
        out = dict(seconds=secs, steps_per_s=steps/secs, vnorm=stp.vnorm(),
                   names=qf.names, row_last=rows[-1].tolist())
    finally:
        close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', choices=('stepwise', 'open', 'snap', 'outputs',
                                      'forces', 'forces_stepwise',
                                      'moving_open', 'moving_forces',
                                      'moving_host', 'stats',
                                      'stats_by_record', 'stats_stepwise',
                                      'quad', 'quad_by_record',
                                      'quad_stepwise'),
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
    fn = dict(moving_open=leg_moving_open, moving_forces=leg_moving_forces,
              moving_host=leg_moving_host, stats=leg_stats,
              stats_by_record=leg_stats_by_record,
              stats_stepwise=leg_stats_stepwise, quad=leg_quad,
              quad_by_record=leg_quad_by_record,
              quad_stepwise=leg_quad_stepwise,
              stepwise=leg_stepwise, open=leg_open, snap=leg_snap,
              outputs=leg_outputs, forces_stepwise=leg_forces_stepwise,
              forces=(leg_forces_outputs if args.with_outputs
                      else leg_forces))[args.leg]
    reps = [fn(su, args.steps, args.spin) for _ in range(args.repeats)]
    key = 'steps_per_s_with_download' \
        if args.leg in ('snap', 'outputs', 'forces', 'moving_forces',
                        'moving_host', 'stats', 'stats_by_record', 'quad',
                        'quad_by_record') \
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
