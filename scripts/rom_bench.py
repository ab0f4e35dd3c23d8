"""What the Galerkin projection onto POD modes costs: `GalerkinROM.project` on
the device (`saddle.ensemble_project` for the three linear projections,
`ConvectionP2.project_tensor` for the cubic convection tensor) against the
fp64 NumPy statement of the same thing, `project(device=False)` -- the only
route there was before it, which runs none of the new kernels -- on the cylinder
wake N=2 and on its refined meshes (`--refine R`, as scripts/record_bench.py).

One command per leg, each a fresh process (profiles/r16_rom/README.md):

  --route device   the three `ensemble_project` calls and `project_tensor`,
                   each by the host clock, uploads and downloads included,
                   and the whole `project`
  --route host     the same pieces by NumPy / SciPy from the operator's element
                   data (`fem.rom.tensor_host`)

`--modes r`: the basis is `r` modes and a mean flow, `nb = r + 1`.  What is
timed does not depend on the values: the modes are seeded smooth fields made
`M`-orthonormal, not a POD of a flow (no time loop runs here).  A warm-up call
of every piece comes first; then `--repeats` timed calls, all reported.
`tensor_gflops` is `2 x 16 x nt x nb^2` flop per cell with an inner dof (the
matrix-core work, padding included) over the WALL time of `project_tensor`,
upload of the basis and download of the tensor included: a lower bound of the
rate of `k_rom_tensor` itself (its device time: a kernel trace of this leg).
One JSON line per leg.
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


def problem(refine):
    """`(femp, M, A, J, fv)` of the cylinder wake N=2, Re=100"""
    if refine > 0:
        from dolfin_navier_scipy_amd.fem import get_sysmats
        femp, sm, rhsd = get_sysmats(problem='cylinderwake', N=2,
                                     refine=refine, Re=100.)
    else:
        import bench
        femp, sm, rhsd = bench.build_problem(N=2, Re=100.)
    M, A, J = (sm[k].tocsr() for k in 'MAJ')
    return femp, M, A, J, np.asarray(rhsd['fv']).reshape(-1)


def seeded_modes(femp, M, r, seed=0):
    """`r` smooth seeded fields on the inner dofs, `M`-orthonormal, and a
    parabolic mean flow"""
    th, inv = femp['V'], np.asarray(femp['invinds'])
    xy = th.nodecoords
    rng = np.random.default_rng(seed)
    full = np.zeros((r + 1, th.vdim))
    for b in range(r):
        k = rng.uniform(1., 6., size=(2, 2))
        ph = rng.uniform(0., 2*np.pi, size=(2, 2))
        for d in range(2):
            full[b, d::2] = np.sin(k[d, 0]*xy[:, 0] + ph[d, 0]) \
                * np.cos(k[d, 1]*xy[:, 1]*5. + ph[d, 1])
    full[r, 0::2] = 4*xy[:, 1]*(0.41 - xy[:, 1])/0.41**2
    S = full[:, inv]
    G = S[:r] @ (M @ S[:r].T)
    Linv = np.linalg.inv(np.linalg.cholesky(G))
    return Linv @ S[:r], S[r]


class ElementData(object):
    """what the host model reads of a `ConvectionP2`, without the device"""

    def __init__(self, th, invinds, dbcinds, dbcvals):
        self._cell_vdofs = np.asarray(th._vdofs()).reshape(-1, 12)
        self.glam, self.area = np.asarray(th.glam), np.asarray(th.area)
        self.ncells, self._vdim = self.area.size, th.vdim
        self._invinds, self._dbcinds = np.asarray(invinds), np.asarray(dbcinds)
        self.nv, self.ndbc = self._invinds.size, self._dbcinds.size
        self.dbc_table_rows, self.dbcvals = 0, dbcvals


def timed(fun, repeats):
    fun()                                   # warm-up
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = fun()
        out.append(time.perf_counter() - t0)
    return out, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--route', choices=('device', 'host'), required=True)
    ap.add_argument('--modes', type=int, default=16)
    ap.add_argument('--refine', type=int, default=0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--label', default='')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from dolfin_navier_scipy_amd import _capi, convection, saddle
    from dolfin_navier_scipy_amd.fem import GalerkinROM, rom
    device = args.route == 'device'
    if device and _capi.device_count() < 1:
        raise SystemExit('no HIP device: nothing is measured without one')
    femp, M, A, J, fv = problem(args.refine)
    r, nb = args.modes, args.modes + 1
    modes, mean = seeded_modes(femp, M, r)
    NV = M.shape[0]
    dbcvals = np.asarray(femp['dbcvals'], dtype=np.float64)
    th = femp['V']
    if device:
        conv = convection.ConvectionP2.from_taylor_hood(
            th, femp['invinds'], femp['dbcinds'], dbcvals)
    else:
        conv = ElementData(th, femp['invinds'], femp['dbcinds'], dbcvals)
    gr = GalerkinROM(A, fv, M=M)
    _, _, basis, D = gr.basis(modes, mean, conv, dbcvals)
    ld = -(-NV//2)*2
    pad = lambda X: np.ascontiguousarray(
        np.hstack([X, np.zeros((X.shape[0], ld - NV))]))
    Phi, Bp, fp = pad(modes), pad(basis), pad(fv[None, :])
    if device:
        pieces = dict(
            Mr=lambda: saddle.ensemble_project(Phi, None, M, nv=NV),
            Ar_b0=lambda: saddle.ensemble_project(Phi, Bp, A, nv=NV),
            fv=lambda: saddle.ensemble_project(Phi, fp, None, nv=NV),
            tensor=lambda: conv.project_tensor(basis, D, ntest=r))
    else:
        pieces = dict(
            Mr=lambda: modes @ (M @ modes.T),
            Ar_b0=lambda: modes @ (A @ basis.T),
            fv=lambda: modes @ fv[:, None],
            tensor=lambda: rom.tensor_host(conv, basis, D, ntest=r))
    secs, res = {}, {}
    for name, fun in pieces.items():
        secs[name], res[name] = timed(fun, args.repeats)
    secs['project'], ops = timed(
        lambda: gr.project(modes, mean, conv, dbcvals, device=device),
        args.repeats)
    code = np.full(th.vdim, -1, dtype=np.int64)
    code[np.asarray(femp['invinds'])] = 1
    live = int((code[conv._cell_vdofs] >= 0).any(axis=1).sum())
    flops = 2.*16*r*nb*nb*live
    nch = -(-live//rom.ROM_CELL_CHUNK)
    out = dict(
        route=args.route, label=args.label, refine=args.refine, modes=r,
        nb=nb, NV=int(NV), ncells=int(conv.ncells), live_cells=live,
        device=_capi.device_name(0) if device else 'host',
        ms={k: [1e3*s for s in v] for k, v in secs.items()},
        linear_ms=[1e3*(a + b + c) for a, b, c in
                   zip(secs['Mr'], secs['Ar_b0'], secs['fv'])],
        tensor_flops=flops,
        tensor_gflops=[flops/s/1e9 for s in secs['tensor']],
        partial_tile_bytes=int(nch*(-(-r//16))*(-(-nb*nb//16))*2048),
        basis_upload_bytes=int(Bp.nbytes),
        mr_minus_identity=float(np.abs(ops['Mr'] - np.eye(r)).max()),
        tensor_norm=float(np.linalg.norm(res['tensor'])),
        c_norm=float(np.linalg.norm(ops['c'])))
    if device:
        conv.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
