"""Bit-level record of what the Krylov cycle computes, to compare two builds of
the library on the same card (a refactor of the host code that enqueues the
cycle must not change one bit: `profiles/r21_cycle_nodes/`).

    python scripts/cycle_digest.py --out digest.json [--lib libdnsamd.so]
    python scripts/cycle_digest.py --eager 2000 [--reps 5] [--lib ...]

Digest: one line of JSON per run, the configuration and the SHA-256 of the
bytes of the result and of the residual history.

* GMRES with `restart = check_every = maxiter = k`, `rtol = 1e-300` (exactly `k`
  columns, `tests/test_gpu_krylov_steps.py`) on the handles of
  `krylov_ld_model.FORMS` (toy problem, NV 1286, NP 207) in the three regimes
  of that test, `k` in 1, 3, 9, 12, `reorth` 0, 1, 2, eager and as a graph, from
  the first right-hand side and start of `krylov_ld_model.CASES`;
* 24 resident CNAB steps of `tests/test_gpu_step_forms.py`'s set-up in the
  six-node lazy, six-node eager and seven-node form: `v`, `p` and the last
  solve's history.

The identical call repeated gives identical bits (leg 5 of the Krylov pin), so
a line that differs between two builds is a launch that differs.  The digests
belong to one compiler and one card: a record, not a test.

`--eager N`: seconds for `N` solves with `use_graph = 0`, `k = 1`, D4f, latency
regime -- the one path on which the host's launch code is on the clock --
`--reps` times, one line of JSON.

`--lib`: load this build of the library instead of the tree's own.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

KS, NRES, DT = (1, 3, 9, 12), 24, 2e-4


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def gmres_lines(bench):
    import krylov_ld_model as kl
    from dolfin_navier_scipy_amd import saddle
    from test_gpu_precond_forms import make_system
    rhs, start = kl.CASES[0]
    b, x0 = kl.right_hand_sides(bench)[rhs], kl.starts(bench)[start]
    for form in kl.FORMS:
        for regime in kl.REGIMES:
            system = make_system(saddle, bench,
                                 dict(kl.FORMS[form], **kl.REGIMES[regime]))
            for k in KS:
                for reorth in kl.REORTHS:
                    for graph in (0, 1):
                        x = system.solve(
                            b[:bench.NV], b[bench.NV:], x0=x0,
                            raise_on_fail=False, restart=k, check_every=k,
                            maxiter=k, rtol=1e-300, reorth=reorth,
                            use_graph=bool(graph))
                        yield dict(run='gmres', form=form, regime=regime, k=k,
                                   reorth=reorth, graph=graph, x=sha(x),
                                   hist=sha(system.residual_history()),
                                   restarts=system.last_stats['restarts'])
            system.close()


def step_lines(prob):
    """(the set-up of `test_gpu_step_forms.py`: steady Stokes state, the
    oracle's Heun step, then the resident steps)"""
    import scenarios
    from oracle import imex_oracle, saddle_oracle
    from dolfin_navier_scipy_amd import saddle, convection
    kw, _, aux = scenarios.build(variant='plain', Nts=NRES + 1,
                                 tE=DT*(NRES + 1), prob=prob)
    M, A, J = kw['M'], kw['A'], kw['J']
    NV = J.shape[1]
    vp0 = saddle_oracle.solve_sadpnt_smw(amat=A, jmat=J, rhsv=aux['cfv'],
                                         rhsp=aux['cfp'])
    dt = kw['trange'][1] - kw['trange'][0]
    heun = imex_oracle.heun_start(
        vc=vp0[:NV], pc=-vp0[NV:], tc=0., tn=dt, M=M, A=A, J=J, scalep=-1.,
        dfv_c=0.,
        dynamic_rhs=lambda t, vc=None, memory={}, mode=None: (
            np.zeros_like(vp0[:NV]), memory), drm={}, bcs_c=[],
        applybcs=kw['applybcs'], appndbcs=kw['appndbcs'], getbcs=kw['getbcs'],
        f_tdp=kw['f_tdp'], f_vdp=kw['f_vdp'], g_tdp=kw['g_tdp'])
    v1, p1, nfc0 = heun[0], heun[1], heun[7]
    for name, lazy, step6 in (('six-node lazy', None, None),
                              ('six-node eager', 0, None),
                              ('seven-node', None, '0')):
        if step6 is not None:
            os.environ['DNS_STEP6'] = step6
        system = saddle.SaddleSystem((M + .5*dt*A).tocsr(), J)
        if lazy is not None:
            system.set_option('step6_lazy', lazy)
        system.setup_precond(cheb_degree=4, schur='dense',
                             factorization='full')
        stp = saddle.ImexStepper(system, (M - .5*dt*A).tocsr())
        os.environ.pop('DNS_STEP6', None)
        stp.set_state(v1, ptilde_c=-dt*p1, nfc_c=nfc0)
        stp.set_rhs(dt*kw['f_tdp'](0.), kw['g_tdp'](0.))
        cvop = convection.ConvectionP2.from_taylor_hood(
            prob['th'], prob['invinds'], prob['dbcinds'], prob['dbcvals'])
        stp.set_convection(cvop, scale=-1.0)
        cf = saddle.ImexStepper.coeffs(a_c=1., cn_c=1.5*dt, cn_o=-.5*dt,
                                       pscale=-1./dt, extrapolate=4,
                                       carry_residual=True)
        opts = saddle.solve_opts(rtol=1e-12, maxiter=300, restart=60,
                                 use_graph=True, reorth=2)
        kinds = [0, 0]
        for n in (8, NRES - 8):
            stp.run(n, cf, opts)
            kinds[0] += int(stp.last_run['lazy_steps'])
            kinds[1] += int(stp.last_run['eager_steps'])
        v, p = stp.get_state()
        yield dict(run='cnab', form=name, steps=NRES, lazy_steps=kinds[0],
                   eager_steps=kinds[1], v=sha(v), p=sha(p),
                   hist=sha(system.residual_history()))
        stp.close()
        cvop.close()
        system.close()


def eager_seconds(bench, nsolves, reps):
    import krylov_ld_model as kl
    from dolfin_navier_scipy_amd import saddle
    from test_gpu_precond_forms import make_system
    system = make_system(saddle, bench,
                         dict(kl.FORMS['D4f'], **kl.REGIMES['latency']))
    b = kl.right_hand_sides(bench)['time-step']
    kw = dict(raise_on_fail=False, restart=1, check_every=1, maxiter=1,
              rtol=1e-300, reorth=2, use_graph=False)
    out = []
    for rep in range(reps + 1):          # (the first repetition warms up)
        t0 = time.perf_counter()
        for _ in range(nsolves):
            system.solve(b[:bench.NV], b[bench.NV:], **kw)
        out.append(time.perf_counter() - t0)
    system.close()
    return out[1:]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--out')
    ap.add_argument('--lib')
    ap.add_argument('--eager', type=int, default=0)
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    from dolfin_navier_scipy_amd import _capi
    if args.lib:
        _capi.load_library(os.path.abspath(args.lib))
    import scenarios
    import krylov_ld_model as kl
    prob = scenarios.toy_problem()
    bench = kl.toy_bench(prob)
    if args.eager:
        secs = eager_seconds(bench, args.eager, args.reps)
        print(json.dumps(dict(run='eager', solves=args.eager, seconds=secs,
                              median=float(np.median(secs)))))
        return
    with open(args.out, 'w') as f:
        for gen in (gmres_lines(bench), step_lines(prob)):
            for line in gen:
                f.write(json.dumps(line, sort_keys=True) + '\n')
                f.flush()
    print('wrote', args.out)


if __name__ == '__main__':
    main()
