"""What a base trajectory stored every k-th step costs a tangent run in
accuracy, held (`BaseTrajectory`, zero-order) and interpolated
(`interpolate=True`), on the host alone: the NumPy statement
`fem.TaylorHood.linearised_convection_vec` about `flow_at(t)` behind the host
model of the CNAB step (`tests/imex_host_model.HostStepper`).  No device.

A smooth analytic base flow on the toy channel (`tests/scenarios.toy_problem`),

    V(t) = (1 + 0.5 sin(w t)) Va + cos(w t) Vb,

`Va` the parabolic inflow profile everywhere, `Vb` a divergence-free looking
standing wave; the perturbation vanishes on the Dirichlet dofs.  Three runs
over `[0, T]` from the same start: about `V(t_n)` at every step (the
reference), about the trajectory stored every `--every`-th step held, and the
same trajectory interpolated.  The distance of the two from the reference at
`T` (M-norm, relative) at `dt = T/steps` and at `dt/2` (twice the steps, the
storage interval halves with `dt`): a held base is a first-order
representation of `V(t)` -- the error halves --, an interpolated one a
second-order representation -- it falls to a quarter.  One JSON line.
"""
import argparse
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def base_flow(prob, omega):
    th = prob['th']
    x, y = th.nodecoords[:, 0], th.nodecoords[:, 1]
    ly = y.max() - y.min()
    s = (y - y.min())/ly
    lx = x.max() - x.min()
    Va, Vb = np.zeros(th.vdim), np.zeros(th.vdim)
    Va[0::2] = 4*s*(1 - s)
    kx = 2*np.pi/lx
    Vb[0::2] = 0.3*np.sin(kx*x)*np.cos(np.pi*s)*np.pi/ly
    Vb[1::2] = -0.3*kx*np.cos(kx*x)*np.sin(np.pi*s)

    def V(t):
        return (1 + 0.5*np.sin(omega*t))*Va + np.cos(omega*t)*Vb
    return V


def tangent_run(prob, flow_of_step, nsteps, dt, w0):
    """`nsteps` CNAB steps of the tangent problem about `flow_of_step(n)`, the
    base flow at the state step `n` starts from; returns the last velocity"""
    import imex_host_model as ihm
    th, inv = prob['th'], prob['invinds']
    M, A, J = (prob['smc'][k] for k in 'MAJ')
    NP, NV = J.shape

    def conv(n, v):
        full = np.zeros(th.vdim)
        full[inv] = np.asarray(v).reshape(-1)
        return -th.linearised_convection_vec(flow_of_step(n), full)[inv, :]
    stp = ihm.HostStepper(ihm.HostSystem((M + .5*dt*A).tocsr(), J),
                          (M - .5*dt*A).tocsr())
    stp.set_convection(types.SimpleNamespace(eval=lambda v, row: conv(row, v)))
    zero = np.zeros((nsteps, NV))
    stp.set_rhs_table(zero, np.zeros((nsteps, NP)))
    nfc0 = conv(0, w0)
    stp.set_state(w0.reshape((-1, 1)), v_p=w0.reshape((-1, 1)), nfc_c=nfc0,
                  nfc_o=nfc0)
    cf = types.SimpleNamespace(a_c=1., a_p=0., cn_c=1.5*dt, cn_o=-.5*dt,
                               pscale=-1./dt)
    stp.run(nsteps, cf)
    return stp.get_state()[0].reshape(-1)


def measure(prob, steps=64, T=1.0, every=4, omega=np.pi):
    """`{dt: (held, interpolated)}` for `dt = T/steps` and `dt/2`, and the
    two ratios error(dt)/error(dt/2)"""
    from dolfin_navier_scipy_amd import convection
    M = prob['smc']['M']
    V = base_flow(prob, omega)
    rng = np.random.default_rng(0)
    NV = M.shape[0]
    w0 = 0.1*V(0.)[prob['invinds']] + 1e-3*rng.standard_normal(NV)

    def mnorm(v):
        return float(np.sqrt(v @ (M @ v)))
    out = {}
    for n in (steps, 2*steps):
        dt = T/n
        stored = dt*np.arange(0, n + 1, every)
        rows = np.array([V(t) for t in stored])
        ref = tangent_run(prob, lambda k: V(k*dt), n, dt, w0)
        errs = []
        for lerp in (False, True):
            traj = convection.BaseTrajectory(stored, rows, interpolate=lerp)
            got = tangent_run(prob, lambda k: traj.flow_at(k*dt), n, dt, w0)
            errs.append(mnorm(got - ref)/mnorm(ref))
        out[n] = tuple(errs)
    (h1, i1), (h2, i2) = out[steps], out[2*steps]
    return dict(steps=steps, T=T, every=every, omega=float(omega),
                held=[h1, h2], interpolated=[i1, i2], ratio_held=h1/h2,
                ratio_interpolated=i1/i2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=64)
    ap.add_argument('--every', type=int, default=4)
    ap.add_argument('--T', type=float, default=1.0)
    ap.add_argument('--nx', type=int, default=11)
    ap.add_argument('--ny', type=int, default=4)
    args = ap.parse_args()
    import scenarios
    prob = scenarios.toy_problem(nx=args.nx, ny=args.ny)
    rec = measure(prob, steps=args.steps, T=args.T, every=args.every)
    rec.update(NV=int(prob['smc']['M'].shape[0]))
    print(json.dumps(rec))


if __name__ == '__main__':
    main()
