"""A FIXED number of GMRES columns through `SaddleSystem.solve` on a
ROW-PARTITIONED handle (`enqueue_cycle_dist`) against the longdouble model of
`tests/krylov_ld_model.py`, entry by entry, at the tolerances
`tests/test_krylov_model_cpu.py` fixes from the model alone
(`tests/golden/krylov_steps_tol.npz` for D4, D4f, MG;
`tests/golden/krylov_dist_tol.npz` for D4t and the `1+5` runs).  The model,
its noise and its tolerances do not depend on how the rows are split: the noise
is what fp64 arithmetic may do to every dot and every preconditioner output in
ANY order of summation.  `tests/test_gpu_zz_dist.py` runs this path to
convergence only, which corrects a wrong Givens entry, a dropped column of
`Z y` or a stale halo entry with a few more iterations; `x_k` after exactly `k`
columns does not.

Ways (as `tests/test_gpu_zz_dist_front.py`): ONE RCCL rank in this process
(graph-capable, trivial partition; every handle, regime and leg), one spawn of
2 and one of 3 gloo-staged ranks sharing the GPU (4 processes with the GPU
open at most).  Partitions (`comm.partition_range`, asserted): [0, 644, 1286] /
[0, 104, 207] and [0, 430, 860, 1286] / [0, 70, 140, 207].  Every rank runs the
same solves in the same order and writes one .npz, the parent evaluates the
model.

Handles (toy problem NV 1286, NP 207, `F = M + 0.5 5e-3 A`, levels
207 / 47 / 11; Chebyshev bounds from the handle, held to the host's as in
`tests/test_gpu_krylov_steps.py`), each in the regimes latency / streamed /
pair of `krylov_ld_model.REGIMES`:

    D4      dense Schur by columns (`schur_cols`), `J Fh^-1`: own entries of
            `tau`, NP-long all-reduce of `zp_j`, with `reorth = 2` the fold
            `- sum h_i zp_i` added by rank 0 alone
    D4f     the same stored in fp32
    D4t     triangular: no `J Fh^-1`, the Schur block reads the pressure
            part of the basis vector itself (model: `DIST_FORMS['D4t']`)
    D4rows  D4 from `SaddleSystem.from_rows_of` (no rank holds a matrix)
    MG      multigrid Schur block, replicated (default `mg_part_min`)
    MGp     `mg_part_min = 0`: levels 207 and 47 row-partitioned (on three
            ranks 16 / 15 / 16 rows of the 47), 11 dense on every rank

(J2 cannot exist: a partitioned handle needs the explicit `Fh^-1`.)  The
schur kind, `nnz_JG > 0` iff full, the level sizes, ONE V-cycle
(`mg_cycles_eff`) and the storage of the coarse inverse are asserted against
the form and the model: the block MG / MGp report is the fused V(2,2) in one
cycle the model `FORMS['MG']` was built for (a world of one rank runs the
replicated levels, `mg_fused && P > 1`).

Legs, `rtol = 1e-300` and `cycle_first` set on EVERY solve (on a
host-callback communicator `gmres()` takes a one-column first cycle whenever
the previous solve needed at most one iteration, whatever `restart` says):

1. exactly `k` columns, `cycle_first = restart = check_every = maxiter = k`,
   `k` in 1, 2, 3, 5, 9, 12, `reorth` 0, 1, 2 (`k = 1`: `dist_lazy1 = 0`, the
   general one-column cycle);
2. `maxiter = k` inside a cycle enqueued 12 long, `k` in 1, 4, 9;
3. `restart = 5`, `maxiter = 13`: cycles 5, 5, 3, the later ones from an `x`
   whose halo entries the tail wrote; once more with `dist_x0_exchange = 1`:
   IDENTICAL BITS (x, history, statistics) in every solve of every way -- the
   claim of DESIGN section 6 holds;
4. the lazy one-step cycle (`reorth = 2`, `cycle_first = 1`): `maxiter = 1`
   against row 1 of the model's `1+5` run, lazy and (`dist_lazy1 = 0`)
   general; `restart = 5`, `maxiter = 6`: cycles 1, 5, `restarts == 1`, seven
   history entries; the guard `rho > 1e-3 tol` of `k_arn_tail_lazy1` from
   `x0 = fl(x_k)` of the model (`guard_k`: residual down by 1e-7): with
   `rtol = 30 res / ||b||` ONE step is taken although the start is inside the
   tolerance (`iters == 1`, OK, `x != x0` -- the general cycle would return
   `x0`, so this is also what shows that the lazy cycle ran), with
   `rtol = 1e5 res / ||b||` none (`x0` back bit for bit, `iters == 0`, OK);
5. stop on `rtol` between `h_k` and `h_{k+1}`, `k` in 2, 6, wherever
   `stop_between()` allows: `iters == k + 1` on every rank;
6. the identical call repeated: identical bits;
7. graphs: on the RCCL rank legs 1 and 4 once more with `use_graph = True`;
   on the gloo ranks one such solve, which is the eager one bit for bit.

The spawned worlds run all of it on D4 / latency and MGp / latency, elsewhere
leg 1 at `k` in 1, 3, 12, legs 3, 4, 6, 7 and the two cases from zero.

Per solve: `x` on all NV + NP entries and every history entry at its own
tolerance (`listed()` decides what is a test; a dropped `k` with a finite
tolerance is held to it; behind a printed Gram-Schmidt fallback nothing more
is compared), `iters`, the length of the history, `restarts`, the status,
`est_relres`, `bnorm`, no NaN, never a breakdown; ACROSS RANKS x, history and
statistics bit for bit; `true_relres` against `||b - K x|| / ||b||` in
longdouble from the returned `x`, within `16u || |b| + |K| |x| || / ||b||`.

Named exception, `...-reorth1-is-one-pass-exception`: the explicit branch of
`enqueue_cycle_dist` launches `k_orth<0>` alone, so `reorth = 1` on a
partitioned handle is classical Gram-Schmidt ONCE.  It is held to the
`reorth = 0` model and tolerances.  In longdouble the models of one and of
two passes are one iterate; they are nowhere further apart than their
tolerances together (0 of the 867 listed cases on the RCCL rank), so no case
here could tell which of the two ran -- the pin is the reading of the code,
the test holds the device to the (wider) history tolerances of one pass.

The handle remembers: `gs_fallbacks` counts the solves IN A ROW whose fused
Gram-Schmidt fell back, and from the eighth on every `reorth = 2` of that
handle runs as `reorth = 0`, silently and for good (no set-up resets it).  A
first version of this module lost the fused form that way before it reached
leg 4 (the guard solve returned `iters == 0`: the general cycle).  `forgive()`
runs one clean fused column behind every fallback.

Largest `error / tol` measured on the MI355X (listed | dropped with a finite
tolerance), the worst regime and `reorth`:

                 1 RCCL rank     2 gloo ranks    3 gloo ranks
    D4     leg 1  0.005 | 0.004   0.006 | 0.004   0.004 | 0.003
           leg 2  0.005 | 0.004   0.004 | 0.003   0.004 | 0.003
           leg 3  0.006 | 0.004   0.004 | 0.004   0.003 | 0.003
           leg 4  0.004 | 0.003   0.003 | 0.003   0.004 | 0.002
           leg 5  0.005 | 0.004   0.003 | 0.003   0.004 | 0.003
    D4f    leg 1  0.007 | 0.004   0.003 | 0.003   0.005 | 0.003
           leg 3  0.004 | 0.004   0.003 | 0.003   0.003 | 0.003
           leg 4  0.004 | 0.004   0.003 | 0.003   0.004 | 0.004
    D4t    leg 1  0.037 | 0.005   0.004 | 0.003   0.003 | 0.004
           leg 3  0.005 |   --    0.008 |   --    0.004 |   --
           leg 4  0.037 | 0.005   0.004 | 0.005   0.005 | 0.005
    D4rows leg 1  0.005 | 0.004   0.006 | 0.004   0.004 | 0.003
           leg 3  0.006 | 0.004   0.003 | 0.004   0.003 | 0.003
           leg 4  0.004 | 0.003   0.003 | 0.003   0.004 | 0.000
    MG     leg 1  0.006 | 0.004   0.004 | 0.004   0.005 | 0.003
           leg 3  0.004 |   --    0.004 |   --    0.003 |   --
           leg 4  0.004 | 0.002   0.003 |   --    0.004 |   --
    MGp    leg 1  0.006 | 0.004   0.004 | 0.004   0.005 | 0.003
           leg 2  0.004 | 0.004   0.003 | 0.003   0.004 | 0.003
           leg 3  0.004 |   --    0.004 |   --    0.003 |   --
           leg 4  0.004 | 0.002   0.003 | 0.002   0.004 | 0.002
           leg 5  0.004 |   --    0.005 |   --    0.003 |   --
    (one rank, legs 2 and 5 of D4f / D4rows / D4t / MG: 0.006 / 0.005 /
    0.037 / 0.004 at most)
    true_relres, error / its tolerance: 0.053 at most (D4t)
    (the columns of the spawned worlds were measured with the three regimes
    of `SPAWN_CUT` still in them)

The lazy and the general one-column cycle differ in bits in every one of the
108 + 38 + 38 pairs and are both within 0.037 of the model's tolerance of
`x_1` (4e-12 .. 7e-11 of `||x_1||`).  Gram-Schmidt fallbacks, all in dropped
cases with `reorth = 2`: D4 / D4f / D4rows at `k = 5, 9, 12`, in leg 2 at
`k = 9` and in the cycle of five behind the lazy step; D4t, MG, MGp at
`k = 12` (which of them varies with the regime and the way); none in a listed
case.

What this says about the open finding of `tests/test_gpu_zz_dist_front.py`
(start residuals of 5-18 x tol on the partitioned path): the Krylov cycle is
cleared as well.  Every iterate, Givens estimate and true residual of the
partitioned cycle is the model's to 0.04 of a tolerance, on every rank the
same bits, with and without the exchange of `x`; front, warm start and cycle
compute what they say.  What is left is what the numbers mean: the one-step
cycle takes its step whenever `rho > 1e-3 tol` and reports the residual
BEHIND the step, so a start residual above `tol` is no error of the path.

Seconds on the MI355X: the 54 cases on one RCCL rank 19.8 in all (6.6 of them
the module's fixtures: the library, the toy problem, the guard starts); the
spawn of 2 ranks 16.2, of 3 ranks 24.0 (`test_gpu_zz_dist_front.py`: 7.8, 6.8,
6.7).
The spawns are more than twice their siblings, so by the rule of the issue the
`pair` regime of D4f and D4t and the `streamed` regime of MG are left to the
RCCL rank there (`SPAWN_CUT`; 19.6 s and 25.8 s with them).  Most of what
remains is D4 / latency and MGp / latency, which run every leg (2.0 s and
4.1 s on two ranks, 2.6 s and 6.0 s on three: a partitioned V-cycle is some
sixteen host-synchronising collectives per column), and 4 s to start the
ranks.
"""
import os
import sys
import time

import numpy as np
import pytest

import krylov_ld_model as kl

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LD = np.longdouble
BIG = float(2**40)
NV, NP = 1286, 207
PARTS = {1: ([0, 1286], [0, 207]),
         2: ([0, 644, 1286], [0, 104, 207]),
         3: ([0, 430, 860, 1286], [0, 70, 140, 207])}
# handle -> (form of the model, how it is made)
HANDLES = {'D4': 'D4', 'D4f': 'D4f', 'D4t': 'D4t', 'D4rows': 'D4', 'MG': 'MG',
           'MGp': 'MG'}
GRID = [(h, r) for h in HANDLES for r in kl.REGIMES]
# the spawned worlds run every leg on these, the reduced grid elsewhere ...
FULL = (('D4', 'latency'), ('MGp', 'latency'))
# ... and leave these to the one RCCL rank (the seconds: module docstring)
SPAWN_CUT = (('D4f', 'pair'), ('D4t', 'pair'), ('MG', 'streamed'))
SPAWN_GRID = [g for g in GRID if g not in SPAWN_CUT]
REDUCED_CASES = (('time-step', 'zero'), ('rough', 'zero'))
REDUCED_K = (1, 3, 12)
ONE_PASS = '-reorth1-is-one-pass-exception'
# what the explicit branch of the partitioned cycle runs for `reorth = 1`:
# `k_orth<0>` alone, classical Gram-Schmidt ONCE -- the `reorth = 0` model
MODEL_REORTH = {0: 0, 1: 0, 2: 2}
GUARD_GO, GUARD_STOP = 30., 1e5


def tag(reorth):
    return 'r%d%s' % (reorth, ONE_PASS if reorth == 1 else '')


# ---- the solves of one handle and regime, the same list on every rank -----------

def plan(name, regime, full, graph, reorths=kl.REORTHS, tab=None):
    """the solves of the handle `name` in `regime`, grouped by the options
    that cost a set-up (`cycle_first`, `dist_lazy1`, `dist_x0_exchange`).
    `graph`: the communicator can capture (one RCCL rank: legs 1 and 4 once
    more as graphs); else ONE solve with `use_graph = True`, which must be
    the eager bits.  Every entry: `sid`, the option state, the arguments of
    `solve`, and what it is judged by"""
    form = HANDLES[name]
    cases = kl.CASES if full else REDUCED_CASES
    out = []

    def add(sid, leg, rhs, start, state, kw, **how):
        kw = dict(dict(rtol=1e-300, use_graph=False), **kw)
        out.append(dict(sid='%s/%s/%s' % (name, regime, sid), leg=leg, rhs=rhs,
                        start=start, state=state, kw=kw, form=form, **how))
        return out[-1]['sid']

    graphs = (False, True) if graph else (False,)
    # legs 2, 5 and column 12 of leg 1: a first cycle of 12
    for reorth in reorths:
        mr = MODEL_REORTH[reorth]
        for rhs, start in cases:
            cs = '%s-%s-%s' % (rhs, start, tag(reorth))
            for g in graphs:
                add('leg1-k12-%s%s' % (cs, '-graph' if g else ''), 'leg1', rhs,
                    start, (12, 1, 0), dict(restart=12, check_every=12,
                                            maxiter=12, reorth=reorth,
                                            use_graph=g),
                    reorth=mr, cycles=kl.LONG, k=12)
            if not full:
                continue
            for k in kl.LEG2_K:
                add('leg2-k%d-%s' % (k, cs), 'leg2', rhs, start, (12, 1, 0),
                    dict(restart=12, check_every=12, maxiter=k, reorth=reorth),
                    reorth=mr, cycles=kl.LONG, k=k)
            bn = float(kl.norm_ld(RHS[rhs]))
            for k in kl.LEG4_K:
                key = kl.gmres_key(form, rhs, start, mr, kl.LONG)
                stop = kl.stop_between(tab, key, k)
                if stop is None:
                    continue
                add('leg5-k%d-%s' % (k, cs), 'leg5', rhs, start, (12, 1, 0),
                    dict(restart=12, check_every=12, maxiter=12, reorth=reorth,
                         rtol=stop/bn),
                    reorth=mr, cycles=kl.LONG, k=k + 1, stop=stop)
    def one_column(lazy):
        # (leg 4: the lazy cycle and, held to the same model, the general
        # one-column cycle)
        for rhs, start in cases:
            for g in graphs:
                add('leg4-%s-one-%s-%s%s' % (
                    'lazy' if lazy else 'general', rhs, start,
                    '-graph' if g else ''), 'leg4', rhs, start, (1, lazy, 0),
                    dict(restart=5, check_every=1, maxiter=1, reorth=2,
                         use_graph=g), reorth=2, cycles=kl.LAZY, k=1)

    # leg 1, the other lengths (k = 1: the general one-column cycle)
    for k in (kl.LEG1_K if full else REDUCED_K):
        if k == 12:
            continue
        if k == 1 and 2 in reorths:
            one_column(0)
        for reorth in reorths:
            for ci, (rhs, start) in enumerate(cases):
                cs = '%s-%s-%s' % (rhs, start, tag(reorth))
                st = (k, 0 if k == 1 else 1, 0)
                kw = dict(restart=k, check_every=k, maxiter=k, reorth=reorth)
                for g in graphs:
                    first = add('leg1-k%d-%s%s' % (k, cs,
                                                   '-graph' if g else ''),
                                'leg1', rhs, start, st, dict(kw, use_graph=g),
                                reorth=MODEL_REORTH[reorth], cycles=kl.LONG,
                                k=k)
                # leg 6: the identical call once more; leg 7 on a communicator
                # that cannot capture: `use_graph` changes nothing
                if ci == 0 and k == (5 if full else 3):
                    add('leg6-k%d-%s' % (k, cs), 'leg6', rhs, start, st, kw,
                        same_as=first)
                    if not graph and reorth == 2:
                        add('leg7-k%d-%s' % (k, cs), 'leg7', rhs, start, st,
                            dict(kw, use_graph=True), same_as=first)
    # leg 3: cycles of 5, 5, 3, with and without the exchange of `x`
    for reorth in reorths:
        for rhs, start in cases:
            cs = '%s-%s-%s' % (rhs, start, tag(reorth))
            kw = dict(restart=5, check_every=5, maxiter=13, reorth=reorth)
            add('leg3-%s' % cs, 'leg3', rhs, start, (5, 1, 0), kw,
                reorth=MODEL_REORTH[reorth], cycles=kl.RESTARTED, k=13,
                restarts=2)
    for reorth in reorths:
        for rhs, start in cases:
            cs = '%s-%s-%s' % (rhs, start, tag(reorth))
            kw = dict(restart=5, check_every=5, maxiter=13, reorth=reorth)
            add('leg3-x0-exchange-%s' % cs, 'leg3', rhs, start, (5, 1, 1), kw,
                restarts=2, same_as='%s/%s/leg3-%s' % (name, regime, cs))
    # leg 4: the one-step cycle
    if 2 in reorths:
        one_column(1)
        for rhs, start in cases:
            for g in graphs:
                add('leg4-lazy-1+5-%s-%s%s' % (rhs, start,
                                               '-graph' if g else ''), 'leg4',
                    rhs, start, (1, 1, 0),
                    dict(restart=5, check_every=5, maxiter=6, reorth=2,
                         use_graph=g), reorth=2, cycles=kl.LAZY, k=6,
                    restarts=1)
        # the guards of `k_arn_tail_lazy1` (`rho > 1e-3 tol`), from the
        # model's `x_k` rounded to fp64: `INPUTS[form]` = (x0, res, ||b||)
        x0, res, bn = INPUTS[form]
        for how, fac in (('go', GUARD_GO), ('stop', GUARD_STOP)):
            assert fac*res/bn < 1.
            add('leg4-guard-%s' % how, 'leg4', 'time-step', 'guard',
                (1, 1, 0), dict(restart=5, check_every=1, maxiter=6, reorth=2,
                                rtol=fac*res/bn), guard=how)
    return out


# (filled by `prepare`, in the parent and in every worker alike)
RHS, START, INPUTS = {}, {}, {}


def guard_k(form):
    """the column whose `x_k` starts the guard solves: the time step from
    zero has come down by 1e-7 (model, module `krylov_ld_model`), so that
    `1e5 res / ||b|| < 1`"""
    return {'D4': 5, 'D4f': 5, 'D4t': 11, 'MG': 9}[form]


def make_inputs(bench):
    """`{form: (x0, ||b - K x0||, ||b||)}` with `x0 = fl(x_k)` of the model
    with the host's Chebyshev bounds (a start vector: any would do)"""
    out = {}
    b = kl.right_hand_sides(bench)['time-step']
    for form in sorted(set(HANDLES.values())):
        prob = kl.Problem(bench, kl.ALL_FORMS[form])
        xs = kl.gmres_cycles(prob, b, None, (guard_k(form),), 1)[0]
        x0 = xs[-1].astype(np.float64)
        res = float(kl.norm_ld(b.astype(LD) - prob.mv(x0.astype(LD))))
        out[form] = (x0, res, float(kl.norm_ld(b)))
    return out


def prepare(bench, inputs):
    RHS.update(kl.right_hand_sides(bench))
    START.update(kl.starts(bench))
    INPUTS.update(inputs)


def load_tab(golden_dir):
    tab = dict(np.load(os.path.join(golden_dir, kl.GOLDEN)))
    tab.update(np.load(os.path.join(golden_dir, kl.GOLDEN_DIST)))
    return tab


# ---- running them (this process or a worker) ----------------------------------------

class Handle(object):
    """one partitioned handle; `state()` sets the three options that are part
    of a solve here and sets the preconditioner up again (any option does
    away with it)"""

    def __init__(self, sad, bench, comm, name, regime):
        form = HANDLES[name]
        self.f = f = dict(kl.ALL_FORMS[form], **kl.REGIMES[regime])
        self.name, self.comm = name, comm
        if name == 'D4rows':
            system = sad.SaddleSystem.from_rows_of(bench.F, bench.J, comm)
        else:
            system = sad.SaddleSystem(bench.F, bench.J)
        thr = 1. if f['streaming'] else BIG
        system.set_option('stream_nnz', thr).set_option('mg_stream_nnz', thr)
        system.set_option('pair', f['pair'])
        if name == 'MGp':
            system.set_option('mg_part_min', 0)
        if name != 'D4rows':
            system.set_comm(comm)
        if f['schur'] == 'mg':
            system.set_schur_mg(bench.prols, smooth_steps=f['nu'])
            for k in ('dense_max', 'dense_half_max', 'fused', 'cheb',
                      'cycles'):
                system.set_option('mg_' + k,
                                  f[k.replace('dense_half', 'half')])
        self.system, self.now, self.bounds, self.setups = system, None, None, 0
        self.forgiven = 0
        self.bench = bench

    def state(self, st):
        if st == self.now:
            return
        s, f = self.system, self.f
        s.set_option('cycle_first', st[0]).set_option('dist_lazy1', st[1])
        s.set_option('dist_x0_exchange', st[2])
        s.setup_precond(cheb_degree=f['degree'], schur=f['schur'],
                        fhat=f['fhat'], fp32_store=bool(f['fp32']),
                        drop_tol=f['drop'], factorization=f['fact'])
        self.setups += 1
        bounds = s.cheb_bounds()
        if self.bounds is None:
            lo, hi = self.bounds = bounds
            # (as in tests/test_gpu_krylov_steps.py)
            assert abs(hi - self.bench.hi) <= 1e-6*self.bench.hi
            assert abs(lo - self.bench.lo) <= 1e-3*self.bench.lo
            self.info = info = s.precond_info()
            assert info['schur'] == f['schur']
            assert info['cheb_degree'] == f['degree']
            assert info['fp32_store'] == bool(f['fp32'])
            assert info['nnz_Gc'] > 0
            assert (info['nnz_JG'] > 0) == (f['fact'] == 'full')
            assert [lv['n'] for lv in info['mg_levels']] == \
                ([207, 47, 11] if f['schur'] == 'mg' else [])
            if f['schur'] == 'mg':
                # a partitioned handle runs ONE V-cycle (`mg_cycles_eff`)
                assert info['mg_nu'] == 2 and info['mg_cycles'] == 1
        # the same set-up every time
        assert bounds == self.bounds
        self.now = st

    def forgive(self):
        """the handle counts the solves IN A ROW whose fused Gram-Schmidt
        fell back, and from the eighth on runs every `reorth = 2` as
        `reorth = 0` for good (`gs_fallbacks`, which no set-up resets): a
        clean fused solve of one column behind every fallback keeps the count
        at zero, so that `reorth = 2` below means the fused form"""
        b = RHS['time-step']
        self.system.solve(b[:NV], b[NV:], x0=None, raise_on_fail=False,
                          restart=1, check_every=1, maxiter=1, rtol=1e-300,
                          reorth=2)
        assert self.system.last_stats['restarts'] == 0
        assert self.system.last_stats['iters'] == 1
        self.forgiven += 1

    def solve(self, spec):
        self.state(spec['state'])
        b = RHS[spec['rhs']]
        x0 = INPUTS[spec['form']][0] if spec['start'] == 'guard' \
            else START[spec['start']]
        x = self.system.solve(b[:NV], b[NV:], x0=x0, raise_on_fail=False,
                              **spec['kw'])
        st = self.system.last_stats
        out = dict(x=x, h=self.system.residual_history().copy(),
                   st=np.array([st['iters'], st['restarts'], st['status'],
                                st['bnorm'], st['est_relres'],
                                st['true_relres']]))
        if spec['kw']['reorth'] == 2 and \
                st['restarts'] > spec.get('restarts', 0):
            self.forgive()
        return out


def run_rank(sad, bench, comm, grid, full_on, graph, tab, reorths=kl.REORTHS):
    """every solve of `grid` on this rank: `{sid + '__x' / '__h' / '__st'}`,
    the bounds and the seconds of every handle"""
    res = {}
    for name, regime in grid:
        t0 = time.time()
        h = Handle(sad, bench, comm, name, regime)
        try:
            full = full_on is None or (name, regime) in full_on
            for spec in plan(name, regime, full, graph, reorths, tab):
                for k, v in h.solve(spec).items():
                    res['%s__%s' % (spec['sid'], k)] = v
            res['%s/%s__bounds' % (name, regime)] = np.array(h.bounds)
            res['%s/%s__info' % (name, regime)] = np.array(
                [h.info['mg_coarse_val_bytes'], h.setups, h.forgiven])
        finally:
            h.system.close()
        res['%s/%s__seconds' % (name, regime)] = np.array(time.time() - t0)
    return res


# ---- the checks -------------------------------------------------------------------

def _same(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return a.shape == b.shape and bool(np.all(a == b))


class Judge(object):
    """the models (with the Chebyshev bounds the handles report) and their
    clean runs, computed once per module"""

    def __init__(self, bench, tab, share=None):
        self.bench, self.tab = bench, tab
        # (the references are computed once and shared by the three ways)
        self.probs, self.runs = ({}, {}) if share is None else \
            (share.probs, share.runs)
        self.worst, self.fallbacks, self.count = {}, {}, {}
        self.lazy_bits = [0, 0]

    def prob(self, form, bounds):
        at = (form,) + tuple(bounds)
        if at not in self.probs:
            self.probs[at] = kl.Problem(self.bench, kl.ALL_FORMS[form],
                                        *bounds)
        return self.probs[at]

    def run(self, form, bounds, rhs, start, reorth, cycles):
        key = kl.gmres_key(form, rhs, start, reorth, cycles)
        at = (key,) + tuple(bounds)
        if at not in self.runs:
            self.runs[at] = kl.gmres_cycles(
                self.prob(form, bounds), RHS[rhs], START[start], cycles,
                reorth)
        return key, self.runs[at]

    def true_relres(self, form, bounds, rhs, x, got):
        """`||b - K x|| / ||b||` from the RETURNED `x`, within
        `16u || |b| + |K| |x| || / ||b||`"""
        prob = self.prob(form, bounds)
        b = RHS[rhs].astype(LD)
        ref = kl.norm_ld(b - prob.mv(x.astype(LD)))/kl.norm_ld(b)
        tol = 16*kl.U64*kl.norm_ld(np.abs(b) + kl.pm.spmm_ld(
            prob.aK, np.abs(x.astype(LD))))/kl.norm_ld(b)
        assert abs(LD(got) - ref) <= tol, (got, float(ref), float(tol))
        return float(abs(LD(got) - ref)/tol)

    def excess(self, key, run, k, x, hist):
        tx, th = self.tab[key + '/tx'][k - 1], self.tab[key + '/th'][:k + 1]
        ex = None
        if np.isfinite(tx).all():
            d = np.abs(x.astype(LD) - run[0][k - 1])
            ex = max(float(d[:NV].max()/tx[0]), float(d[NV:].max()/tx[1]))
        fin = np.isfinite(th)
        dh = np.abs(hist.astype(LD) - run[1][:k + 1])[fin]
        return ex, float((dh/th[fin]).max()) if fin.any() else 0.

    def check(self, spec, outs, bounds, by_sid):
        """one solve: the ranks against each other, then the model"""
        from dolfin_navier_scipy_amd import _capi as C
        sid, form, rhs = spec['sid'], spec['form'], spec['rhs']
        x, hist, st = outs[0]['x'], outs[0]['h'], outs[0]['st']
        for r, o in enumerate(outs[1:]):
            # all-reduced inputs, the velocity gathered from the owners: a
            # difference means a rank took another path
            assert _same(o['x'], x), (sid, r + 1, 'x')
            assert _same(o['h'], hist), (sid, r + 1, 'history')
            assert _same(o['st'], st), (sid, r + 1, o['st'], st)
        iters, restarts, status = (int(v) for v in st[:3])
        bnorm, est, true = st[3:]
        assert x.shape == (NV + NP,) and np.isfinite(x).all(), sid
        assert np.isfinite(hist).all() and status != C.DNS_BREAKDOWN, sid
        bn = kl.norm_ld(RHS[rhs])
        assert abs(bnorm - bn) <= 16*kl.U64*bn, sid
        assert est == hist[-1]/bnorm, sid
        group = (spec['leg'], sid.split('/')[0])
        w = self.worst.setdefault(group, [0., 0., 0.])
        w[2] = max(w[2], self.true_relres(form, bounds, rhs, x, true))
        if 'same_as' in spec:
            ref = by_sid[spec['same_as']]
            assert _same(x, ref['x']) and _same(hist, ref['h']), sid
            assert _same(st[:5], ref['st'][:5]), sid
            return
        if 'guard' in spec:
            x0 = INPUTS[form][0]
            assert status == C.DNS_OK and restarts == 0, (sid, st)
            if spec['guard'] == 'go':
                assert iters == 1 and hist.size == 2, (sid, st)
                assert not np.array_equal(x, x0) and hist[1] < hist[0], sid
            else:
                assert iters == 0 and hist.size == 1, (sid, st)
                assert _same(x, x0), sid
            res = INPUTS[form][1]
            assert abs(hist[0] - res) <= 1e-6*res, (sid, hist[0], res)
            return
        k = spec['k']
        assert iters == k and hist.size == k + 1, (sid, st, hist.size)
        if 'stop' in spec:
            assert status == C.DNS_OK, (sid, st)
            assert hist[-1] <= spec['stop'] < hist[-2], sid
        else:
            assert status == C.DNS_NOT_CONVERGED, (sid, st)
        want = spec.get('restarts', 0)
        key, run = self.run(form, bounds, rhs, spec['start'], spec['reorth'],
                            spec['cycles'])
        listed = kl.listed(self.tab, key, k)
        n = self.count.setdefault(group, [0, 0])
        n[0 if listed else 1] += 1
        if listed:
            assert restarts == want, (sid, st)
        elif restarts != want:
            self.fallbacks.setdefault(group, set()).add(sid.split('/', 1)[1])
            return
        ex, eh = self.excess(key, run, k, x, hist)
        assert not listed or ex is not None
        both = max(eh, 0. if ex is None else ex)
        w[0 if listed else 1] = max(w[0 if listed else 1], both)
        assert both <= 1., (sid, key, k, ex, eh)
        if ONE_PASS in sid and listed:
            # where the models of one and of two passes are further apart
            # than their tolerances together, the device is on the side of
            # ONE pass (just asserted); counted, so that the report says how
            # often the two could be told apart at all
            key1, run1 = self.run(form, bounds, rhs, spec['start'], 1,
                                  spec['cycles'])
            d = np.abs(run1[0][k - 1] - run[0][k - 1])
            tx = self.tab[key + '/tx'][k - 1] + self.tab[key1 + '/tx'][k - 1]
            dh = np.abs(run1[1][:k + 1] - run[1][:k + 1])
            th = self.tab[key + '/th'][:k + 1] + self.tab[key1 + '/th'][:k + 1]
            apart = d[:NV].max() > tx[0] or d[NV:].max() > tx[1] or \
                bool(np.any(dh > th))
            a = self.count.setdefault(('apart',) + group[1:], [0, 0])
            a[0 if apart else 1] += 1

    def check_grid(self, outs, grid, full_on, graph, reorths=kl.REORTHS):
        """`outs`: one dict per rank as `run_rank` returns it"""
        for name, regime in grid:
            pre = '%s/%s' % (name, regime)
            bounds = tuple(float(v) for v in outs[0][pre + '__bounds'])
            for o in outs[1:]:
                assert _same(o[pre + '__bounds'], outs[0][pre + '__bounds'])
            m = self.prob(HANDLES[name], bounds).m64
            if m.schur == 'mg':
                # the block the handle reports is the block of the model:
                # levels 207 / 47 / 11 (asserted on the rank), the fused
                # V(2,2) in ONE cycle, the coarse inverse as stored
                assert m.mg.sizes == [207, 47, 11] and not m.mg.two
                assert int(outs[0][pre + '__info'][0]) == \
                    {'f64': 8, 'f32': 4, 'f16': 2}[m.store['cinv']]
            full = full_on is None or (name, regime) in full_on
            by_sid = {}
            for spec in plan(name, regime, full, graph, reorths, self.tab):
                sid = spec['sid']
                ranks = [dict((k, o['%s__%s' % (sid, k)])
                              for k in ('x', 'h', 'st')) for o in outs]
                by_sid[sid] = ranks[0]
                self.check(spec, ranks, bounds, by_sid)
            # the two one-column cycles: the same model, maybe other bits
            for spec in plan(name, regime, full, graph, reorths, self.tab):
                sid = spec['sid']
                if '/leg4-lazy-one-' in sid:
                    other = by_sid[sid.replace('-lazy-one-', '-general-one-')]
                    self.lazy_bits[_same(by_sid[sid]['x'], other['x'])] += 1

    def report(self, what):
        print('%s: %d models, %d clean runs' % (what, len(self.probs),
                                                len(self.runs)))
        for group in sorted(self.worst):
            if group[0] == 'apart':
                continue
            w, n = self.worst[group], self.count.get(group, [0, 0])
            print('  %-5s %-7s error / tol %.3f | %.3f  (%d listed, %d '
                  'dropped)  true_relres %.3f' % (group + (w[0], w[1], n[0],
                                                           n[1], w[2])))
            fb = sorted(self.fallbacks.get(group, ()))
            if fb:
                print('      Gram-Schmidt fallback in dropped cases: '
                      + ', '.join(fb))
        for group in sorted(self.count):
            if group[0] == 'apart':
                print('  reorth = 1, %-7s one- and two-pass models apart in %d '
                      'listed cases, not in %d' % (group[1], *self.count[group]))
        print('  one-step cycle, lazy against general: other bits in %d '
              'solves, the same in %d' % tuple(self.lazy_bits))


@pytest.fixture(scope='module')
def env(toy_prob, golden_dir):
    from dolfin_navier_scipy_amd import _capi, comm as dcomm
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    for P in (1, 2, 3):
        for r in range(P):
            assert dcomm.partition_range(NV, P, r) == \
                tuple(PARTS[P][0][r:r + 2])
            assert dcomm.partition_range(NP, P, r) == \
                tuple(PARTS[P][1][r:r + 2])
    bench = kl.toy_bench(toy_prob)
    inputs = make_inputs(bench)
    prepare(bench, inputs)
    return dict(bench=bench, inputs=inputs, tab=load_tab(golden_dir),
                golden_dir=golden_dir)


@pytest.fixture(scope='module')
def judge(env):
    return Judge(env['bench'], env['tab'])


# ---- one RCCL rank in this process ------------------------------------------------

@pytest.fixture(scope='module')
def rccl(env):
    from dolfin_navier_scipy_amd import comm as dcomm
    cm1 = dcomm.Comm.rccl(0, 1, 0, dcomm.rccl_unique_id())
    yield cm1
    cm1.close()


ONE_RANK = [(h, r, q) for h, r in GRID for q in kl.REORTHS]
ONE_RANK_RAN = {}


@pytest.mark.parametrize('name,regime,reorth', ONE_RANK, ids=[
    '%s-%s-reorth%d%s' % (h, r, q, ONE_PASS[8:] if q == 1 else '')
    for h, r, q in ONE_RANK])
def test_one_rccl_rank(env, judge, rccl, name, regime, reorth):
    """every leg, eager and as a graph (RCCL calls are captured with the
    kernels), trivial partition"""
    from dolfin_navier_scipy_amd import saddle
    grid = [(name, regime)]
    # (the solves of the three `reorth` of a handle run together, grouped by
    # the options that cost a set-up; each case judges its own)
    if (name, regime) not in ONE_RANK_RAN:
        ONE_RANK_RAN.clear()
        ONE_RANK_RAN[name, regime] = run_rank(saddle, env['bench'], rccl,
                                              grid, None, True, env['tab'])
        print('%s/%s: %.2f s, %d set-ups, %d fallbacks' % (
            (name, regime, ONE_RANK_RAN[name, regime][
                '%s/%s__seconds' % (name, regime)]) + tuple(
                ONE_RANK_RAN[name, regime]['%s/%s__info' % (name, regime)][1:])))
    out = ONE_RANK_RAN[name, regime]
    judge.check_grid([out], grid, None, True, (reorth,))
    if (name, regime, reorth) == ONE_RANK[-1]:
        judge.report('one RCCL rank')


# ---- gloo-staged ranks sharing the GPU ---------------------------------------------

def _worker(rank, world, port, outdir, golden_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      RANK=str(rank), WORLD_SIZE=str(world),
                      GLOO_SOCKET_IFNAME='lo')   # loopback, deterministically
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import datetime
    import faulthandler
    import torch.distributed as dist
    faulthandler.dump_traceback_later(100, exit=True)   # never hang a GPU box
    dist.init_process_group('gloo', rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    import scenarios
    from dolfin_navier_scipy_amd import saddle, comm as dcomm
    cmg = dcomm.Comm.gloo(0)
    assert (cmg.rank, cmg.nranks) == (rank, world)
    bench = kl.toy_bench(scenarios.toy_problem())
    inp = np.load(os.path.join(outdir, 'inputs.npz'))
    prepare(bench, dict((f, (inp[f + '__x0'], float(inp[f + '__res']),
                             float(inp[f + '__bn'])))
                        for f in set(HANDLES.values())))
    # (every rank: the same solves in the same order with the same arguments)
    res = run_rank(saddle, bench, cmg, SPAWN_GRID, FULL, False,
                   load_tab(golden_dir))
    np.savez(os.path.join(outdir, 'krylov_rank{0}.npz'.format(rank)), **res)
    cmg.close()
    dist.destroy_process_group()


def _spawned(env, shared, tmp_path, world):
    from spawn_util import spawn_ranks
    inp = {}
    for f, (x0, res, bn) in env['inputs'].items():
        inp.update({f + '__x0': x0, f + '__res': res, f + '__bn': bn})
    np.savez(tmp_path / 'inputs.npz', **inp)
    t0 = time.time()
    spawn_ranks(_worker, world, str(tmp_path), env['golden_dir'])
    t1 = time.time()
    outs = [dict(np.load(tmp_path / 'krylov_rank{0}.npz'.format(r)))
            for r in range(world)]
    judge = Judge(env['bench'], env['tab'], share=shared)
    judge.check_grid(outs, SPAWN_GRID, FULL, False)
    judge.report('%d gloo ranks (%.1f s in the ranks, %.1f s of models)'
                 % (world, t1 - t0, time.time() - t1))
    print('  seconds per handle on rank 0: ' + ' '.join(
        '%s/%s %.2f (%d set-ups, %d fallbacks)' % (
            (h, r, outs[0]['%s/%s__seconds' % (h, r)])
            + tuple(outs[0]['%s/%s__info' % (h, r)][1:]))
        for h, r in SPAWN_GRID))


def test_two_gloo_ranks(env, judge, tmp_path):
    _spawned(env, judge, tmp_path, 2)


def test_three_gloo_ranks_middle_rank_has_two_neighbours(env, judge, tmp_path):
    assert PARTS[3][0][1] == 430 and PARTS[3][1][1] == 70
    _spawned(env, judge, tmp_path, 3)
