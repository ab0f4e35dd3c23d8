"""A FIXED number of GMRES columns / BiCGStab iterations through
`SaddleSystem.solve` against the longdouble model of
`tests/krylov_ld_model.py`, entry by entry, at the tolerance
`tests/test_krylov_model_cpu.py` fixes from the model alone
(`tests/golden/krylov_steps_tol.npz`): the iterate `x_k` per block, every entry
of the residual history, and the solve's statistics.  A converged solve
corrects a wrong Givens entry, a dropped column of `Z y` or a stale `zp_i` with
a few more iterations; `x_k` after exactly `k` columns does not.

Why `restart = check_every = k` fixes the cycle length: `dns_saddle::gmres`
starts with `c = last_iters + 1` (16 on a fresh handle), rounds it UP to a
multiple of `check_every` and caps it at `min(restart, 64)` -- with both equal
to `k` that is `k` whatever the previous solve on the handle left in
`last_iters`; a restarted solve goes on with `min(m, max(2 c, 8))`, which is
`m` again for `m = 5`.  `rtol = 1e-300`: nothing converges, `maxiter` (counted
in `givens_close`) or the end of the cycle stops the solve.

Forms (`krylov_ld_model.FORMS`; the toy problem NV 1286, NP 207,
`F = M + 0.5 5e-3 A`, levels 207 / 47 / 11), one handle per form and regime:

    J2   Jacobi Schur, Chebyshev recurrence of degree 2, triangular  (SK 0)
    D4   dense Schur, explicit degree 4, full factorisation, fp64    (SK 1)
    D4f  the same stored in fp32                                     (SK 2)
    MG   multigrid V(2,2) Schur, explicit, full                      (SK 3)

    latency   stream_nnz = mg_stream_nnz = 2^40
    streamed  thresholds 1, pair = 0
    pair      thresholds 1, pair = 1

GMRES legs, each for `reorth` 0, 1, 2, eager and as a graph, the right-hand
sides / starts of `krylov_ld_model.CASES`:

1. exactly `k` columns, `k` in 1, 2, 3, 5, 9, 12 (`maxiter = k`); column 9 is
   the first whose dots no longer fit the streaming epilogue (`kStreamDots`);
2. `maxiter = k` inside a cycle enqueued 12 long, `k` in 1, 4, 9;
3. `restart = 5`, `maxiter = 13`: cycles of 5, 5, 3, on every form (the CPU
   table has `x_13` of D4 within the condition for `reorth` 0 and 1).  The
   history of the third cycle is held to its own tolerance, which on D4 and
   MG -- at rounding level by then -- is 1e-5 of the entry to the entry
   itself: `x_13`, `restarts == 2` and the 14 entries are what is pinned;
4. stop on `rtol` (and once `atol`) between `h_k` and `h_{k+1}`, `k` in 2, 6:
   `iters == k + 1` exactly;
5. the identical call repeated: identical bits.

Which `(run, k)` count as tests is the CPU module's `listed()`: the tolerance
of `x_k` at most 1e-10 of its block, nothing else.  On those `error / tol <= 1`
for `x` and for EVERY history entry at its own tolerance, `restarts` (0, or 2
in leg 3: no Gram-Schmidt fallback), the status and `est_relres` are asserted.
Leg 4 runs wherever the model's tolerances separate the stop from `h_0..h_k`
and `h_{k+1}` (`stop_between()`), whether `x_{k+1}` is listed or not.  A dropped
`k` is still run and held to what the code promises in any case (`iters`, the
length of the history, no NaN, never a breakdown).  Without a fallback it is
compared like a listed one wherever the model has a finite tolerance.  With a
fallback (printed, not an error: the CPU module's docstring says why fused
Gram-Schmidt gives up early behind the dense block) NOTHING more is compared,
the iterate behind a fallback is not the model's.  So the fold
`- sum h_i zp_i` of `k_arn_head_f<1, 2>` (D4, D4f with `reorth = 2`) is held to
the model at `k = 1` (listed) and `k = 2, 3` (tolerance 2e-10) only: from
`k = 5` on those runs are uncompared, and the fold never crosses `kStreamDots`
on the dense block; it does on J2 (`k = 9, 12`, tolerance 1e-10).

BiCGStab (J2, D4; latency regime only: the method runs `k_spmv_dot2` and
`apply_precond`, never the streaming epilogues): `k` in 1, 2, 3 from zero and
1, 2 from the rough start -- iteration 3 reads `BicgCtl::sc[0]` as iteration 1
wrote it, so both parity slots are read after being written.  `k_bicg_p`
stops at `it >= maxiter` with the last update applied: `iters == k`,
`hist[0..k]`.  A start at the converged solution returns it bit for bit.

Stagnation (D4, latency, `reorth = 2`, one cycle of 40): by column 5 the
residual is down by 1e-8, `kappa^2 u` is one, the basis of classical
Gram-Schmidt once is no longer orthogonal and `<w, w> - sum h_i^2` falls below
`1e-8 <w, w>`: `pythagoras_norm` returns -1, `k_arn_head_f` raises
`kGsFallback`, the driver counts a restart and goes on with `reorth = 0` from
the iterate it has.  Either way: no NaN, no breakdown, `iters <= 40`, and the
true residual within 32 times the smallest one the longdouble model reaches
in 40 columns (1.6e-10: its fused run ends at column 7).

Largest `error / tol` measured on the MI355X (listed cases | dropped cases
with a finite tolerance), per form, the worst regime and `reorth`:

             J2             D4             D4f            MG
    leg 1    0.031 | 0.006  0.005 | 0.004  0.007 | 0.004  0.005 | 0.004
    leg 2    0.031 | 0.006  0.005 | 0.004  0.007 | 0.004  0.005 | 0.004
    leg 3    0.010 | 0.006  0.005 | 0.004  0.004 | 0.004  0.004
    leg 4    0.010 | 0.004  0.004 | 0.004  0.006 | 0.004  0.006
    BiCGStab 0.004          0.003

Leg 4 runs all 54 solves of a form and regime (3 `reorth` x 3 cases x eager /
graph x `k = 2`, `k = 6`, `k = 2` with `atol`) on J2 and MG, 48 on D4 and D4f
(`krylov_ld_model.LEG4_NOT_RUN`: fused, `k = 6`, NaN tolerances), the stop at
least 43 tolerances from the entries.  Stagnation: the fused norm gave up
(`restarts == 1`), 40 iterations, true residual 9.6e-17 against 32 x 1.6e-10.
Gram-Schmidt fallbacks, all in dropped cases of legs 1 and 2 with
`reorth = 2`: D4 / D4f at `k = 5, 9, 12`, MG at `k = 12` (which of them varies
with the regime); none in a listed case.  The module takes 9 s.
"""
import os

import numpy as np
import pytest

import krylov_ld_model as kl
from test_gpu_precond_forms import make_system, check_info

pytestmark = pytest.mark.gpu

LD = np.longdouble
GRID = [(f, r) for f in kl.FORMS for r in kl.REGIMES]
GRID_IDS = ['%s-%s' % fr for fr in GRID]


class Ctx(object):
    """the handles, the models (with the Chebyshev bounds the handles report)
    and their clean runs, computed once"""

    def __init__(self, sad, bench, golden):
        self.sad, self.bench, self.tab = sad, bench, golden
        self.NV, self.n = bench.NV, bench.NV + bench.NP
        self.rhs, self.start = kl.right_hand_sides(bench), kl.starts(bench)
        self.handles, self.probs, self.runs, self.bounds = {}, {}, {}, {}
        self.worst, self.fallbacks = {}, {}

    def handle(self, form, regime):
        if (form, regime) not in self.handles:
            f = dict(kl.FORMS[form], **kl.REGIMES[regime])
            system = make_system(self.sad, self.bench, f)
            self.handles[form, regime] = system
            lo, hi = self.bounds[form, regime] = system.cheb_bounds()
            # the tolerances were worked out with the host's bounds, the
            # model of `x_k` takes the handle's: the same polynomial to a
            # part in a thousand (the smaller bound comes from a shifted
            # power iteration that has not settled further), which moves
            # 32 x a largest deviation of eight noisy runs by as little
            assert abs(hi - self.bench.hi) <= 1e-6*self.bench.hi
            assert abs(lo - self.bench.lo) <= 1e-3*self.bench.lo
            check_info(system, f, self.prob(form, regime).m64)
        return self.handles[form, regime]

    def prob(self, form, regime):
        """(one model for the three regimes if they report the same bounds)"""
        lo, hi = self.bounds[form, regime]
        if (form, lo, hi) not in self.probs:
            self.probs[form, lo, hi] = kl.Problem(self.bench, kl.FORMS[form],
                                                  lo, hi)
        return self.probs[form, lo, hi]

    def gmres(self, form, regime, rhs, start, reorth, cycles):
        key = kl.gmres_key(form, rhs, start, reorth, cycles)
        at = (key,) + self.bounds[form, regime]
        if at not in self.runs:
            self.runs[at] = kl.gmres_cycles(
                self.prob(form, regime), self.rhs[rhs], self.start[start],
                cycles, reorth)
        return key, self.runs[at]

    def bicg(self, form, regime, rhs, start):
        key = kl.bicg_key(form, rhs, start)
        at = (key,) + self.bounds[form, regime]
        if at not in self.runs:
            self.runs[at] = kl.bicgstab_steps(
                self.prob(form, regime), self.rhs[rhs], self.start[start],
                kl.BICG_K[start])
        return key, self.runs[at]

    def close(self):
        for system in self.handles.values():
            system.close()

    # -- one solve against the model -------------------------------------------
    def solve(self, system, rhs, start, **kw):
        b = self.rhs[rhs]
        x = system.solve(b[:self.NV], b[self.NV:], x0=self.start[start],
                         raise_on_fail=False, **kw)
        return x, system.residual_history().copy(), dict(system.last_stats)

    def excess(self, key, run, k, x, hist):
        """`error / tol` of `x` against `x_k` and of every entry of `hist`
        against `hist[0..k]`, each at its own tolerance; an entry (or `x`)
        without a finite tolerance is not compared: `(ex_x, ex_h)`, None for
        `x` then"""
        tx, th = self.tab[key + '/tx'][k - 1], self.tab[key + '/th'][:k + 1]
        ex = None
        if np.isfinite(tx).all():
            d = np.abs(x.astype(LD) - run[0][k - 1])
            ex = max(float(d[:self.NV].max()/tx[0]),
                     float(d[self.NV:].max()/tx[1]))
        fin = np.isfinite(th)
        dh = np.abs(hist.astype(LD) - run[1][:k + 1])[fin]
        return ex, float((dh/th[fin]).max()) if fin.any() else 0.

    def common(self, rhs, st, hist, k):
        """what holds for every solve that ran `k` steps"""
        from dolfin_navier_scipy_amd import _capi as C
        assert st['iters'] == k and hist.size == k + 1
        assert np.isfinite(hist).all()
        assert st['status'] != C.DNS_BREAKDOWN
        bn = kl.norm_ld(self.rhs[rhs])
        assert abs(st['bnorm'] - bn) <= 16*kl.U64*bn
        assert st['est_relres'] == hist[-1]/st['bnorm']

    def judge(self, group, key, run, k, x, hist, st, restarts=0):
        """a listed `x_k`: the number of restarts (no Gram-Schmidt fallback),
        `x` and every history entry within tolerance.  A dropped one: a
        fallback is recorded and nothing compared (the iterate behind a
        fallback is not the model's); else whatever has a finite tolerance"""
        assert np.isfinite(x).all()
        w = self.worst.setdefault(group, [0., 0.])
        listed = kl.listed(self.tab, key, k)
        if listed:
            assert st['restarts'] == restarts, (key, k, st)
        elif st['restarts'] != restarts:
            self.fallbacks.setdefault(group, set()).add(
                '%s k=%d' % (key.split('/', 2)[2], k))
            return
        ex, eh = self.excess(key, run, k, x, hist)
        assert not listed or ex is not None
        both = max(eh, 0. if ex is None else ex)
        w[0 if listed else 1] = max(w[0 if listed else 1], both)
        assert both <= 1., (key, k, ex, eh)


@pytest.fixture(scope='module')
def ctx(toy_prob, golden_dir):
    from dolfin_navier_scipy_amd import saddle, _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    c = Ctx(saddle, kl.toy_bench(toy_prob),
            dict(np.load(os.path.join(golden_dir, kl.GOLDEN))))
    yield c
    c.close()


def report(ctx, leg, form, regime):
    w = ctx.worst.get((leg, form, regime), [0., 0.])
    print('%s %-4s %-8s error / tol %.3f | %.3f' % (leg, form, regime, *w))
    fb = sorted(ctx.fallbacks.get((leg, form, regime), ()))
    if fb:
        print('    Gram-Schmidt fallback in dropped cases: ' + ', '.join(fb))


def variants():
    for reorth in kl.REORTHS:
        for graph in (False, True):
            for rhs, start in kl.CASES:
                yield reorth, graph, rhs, start


def not_converged():
    from dolfin_navier_scipy_amd import _capi as C
    return C.DNS_NOT_CONVERGED


@pytest.mark.parametrize('form,regime', GRID, ids=GRID_IDS)
def test_exactly_k_columns(ctx, form, regime):
    """legs 1 and 5"""
    system = ctx.handle(form, regime)
    for reorth, graph, rhs, start in variants():
        key, run = ctx.gmres(form, regime, rhs, start, reorth, kl.LONG)
        for k in kl.LEG1_K:
            kw = dict(restart=k, check_every=k, maxiter=k, rtol=1e-300,
                      reorth=reorth, use_graph=graph)
            x, hist, st = ctx.solve(system, rhs, start, **kw)
            ctx.common(rhs, st, hist, k)
            assert st['status'] == not_converged()
            ctx.judge(('leg1', form, regime), key, run, k, x, hist, st)
            if k == 5:
                x2, hist2, st2 = ctx.solve(system, rhs, start, **kw)
                assert np.array_equal(x, x2) and np.array_equal(hist, hist2)
                assert st2['iters'] == st['iters']
    report(ctx, 'leg1', form, regime)


@pytest.mark.parametrize('form,regime', GRID, ids=GRID_IDS)
def test_stop_inside_a_longer_cycle(ctx, form, regime):
    """leg 2: the tails run with `jdone < c`, no column is open"""
    system = ctx.handle(form, regime)
    for reorth, graph, rhs, start in variants():
        key, run = ctx.gmres(form, regime, rhs, start, reorth, kl.LONG)
        for k in kl.LEG2_K:
            x, hist, st = ctx.solve(system, rhs, start, restart=12,
                                    check_every=12, maxiter=k, rtol=1e-300,
                                    reorth=reorth, use_graph=graph)
            ctx.common(rhs, st, hist, k)
            assert st['status'] == not_converged()
            ctx.judge(('leg2', form, regime), key, run, k, x, hist, st)
    report(ctx, 'leg2', form, regime)


@pytest.mark.parametrize('form,regime', [g for g in GRID
                                         if g[0] in kl.LEG3_FORMS],
                         ids=[i for i, g in zip(GRID_IDS, GRID)
                              if g[0] in kl.LEG3_FORMS])
def test_restart_and_stop_in_the_third_cycle(ctx, form, regime):
    """leg 3: cycles of 5, 5 and 3 columns, two restarts, 14 history entries
    (the `beta` of the second and third cycle is not appended)"""
    system = ctx.handle(form, regime)
    k = sum(kl.RESTARTED)
    for reorth, graph, rhs, start in variants():
        key, run = ctx.gmres(form, regime, rhs, start, reorth, kl.RESTARTED)
        x, hist, st = ctx.solve(system, rhs, start, restart=5, check_every=5,
                                maxiter=k, rtol=1e-300, reorth=reorth,
                                use_graph=graph)
        ctx.common(rhs, st, hist, k)
        assert hist.size == 14 and st['status'] == not_converged()
        ctx.judge(('leg3', form, regime), key, run, k, x, hist, st,
                  restarts=2)
    report(ctx, 'leg3', form, regime)


@pytest.mark.parametrize('form,regime', GRID, ids=GRID_IDS)
def test_stop_on_the_tolerance(ctx, form, regime):
    """leg 4: `rtol ||b||` (once `atol`) halfway, in the logarithm, between
    the model's `h_k` and `h_{k+1}`: the solve takes `k + 1` columns, not one
    more or less, and says it converged"""
    from dolfin_navier_scipy_amd import _capi as C
    system = ctx.handle(form, regime)
    ran = []
    for reorth, graph, rhs, start in variants():
        key, run = ctx.gmres(form, regime, rhs, start, reorth, kl.LONG)
        bn = kl.norm_ld(ctx.rhs[rhs])
        for k, how in [(2, 'rtol'), (6, 'rtol'), (2, 'atol')]:
            # wherever the model's tolerances separate the stop from the
            # entries (else which column stops is not determined), `x_{k+1}`
            # listed or not
            if kl.stop_between(ctx.tab, key, k) is None:
                continue
            stop = np.sqrt(run[1][k]*run[1][k + 1])
            tol = dict(rtol=float(stop/bn)) if how == 'rtol' else \
                dict(rtol=0., atol=float(stop))
            x, hist, st = ctx.solve(system, rhs, start, restart=12,
                                    check_every=12, maxiter=12, reorth=reorth,
                                    use_graph=graph, **tol)
            ctx.common(rhs, st, hist, k + 1)
            assert st['status'] == C.DNS_OK
            assert hist[-1] <= float(stop) < hist[-2]
            ctx.judge(('leg4', form, regime), key, run, k + 1, x, hist, st)
            ran.append((reorth, rhs, start, k))
    print('leg4 %-4s %-8s %d solves' % (form, regime, len(ran)))
    # every Gram-Schmidt form, right-hand side, start and `k` but the ones
    # spelled out in `LEG4_NOT_RUN`
    want = [(r, rhs, start, k) for r in kl.REORTHS for rhs, start in kl.CASES
            for k in kl.LEG4_K
            if (r, rhs, start, k) not in kl.LEG4_NOT_RUN[form]]
    assert sorted(set(ran)) == sorted(want)
    report(ctx, 'leg4', form, regime)


def test_stagnation(ctx):
    from dolfin_navier_scipy_amd import _capi as C
    system = ctx.handle('D4', 'latency')
    b = ctx.rhs['time-step']
    x, hist, st = ctx.solve(system, 'time-step', 'zero', restart=40,
                            check_every=40, maxiter=40, rtol=1e-300, reorth=2)
    _, floor, _, bn = ctx.tab['stagnation']
    K = ctx.prob('D4', 'latency')
    res = float(kl.norm_ld(b.astype(LD) - K.mv(x.astype(LD))))
    print('stagnation: %s, iters %d, restarts %d, true residual %.2e '
          '(%.3f of 32 x the model\'s floor %.2e), last estimate %.2e'
          % ('Gram-Schmidt fallback' if st['restarts'] else
             'the fused norm survived', st['iters'], st['restarts'], res,
             res/(32*floor), floor, hist[-1]))
    assert st['status'] != C.DNS_BREAKDOWN
    assert 1 <= st['iters'] <= 40 and hist.size == st['iters'] + 1
    assert np.isfinite(hist).all() and np.isfinite(x).all()
    assert res <= 32*floor


@pytest.mark.parametrize('form', kl.BICG_FORMS)
def test_bicgstab_steps(ctx, form):
    system = ctx.handle(form, 'latency')
    group = ('bicg', form, 'latency')
    for rhs in ctx.rhs:
        for start, kmax in kl.BICG_K.items():
            key, run = ctx.bicg(form, 'latency', rhs, start)
            for k in range(1, kmax + 1):
                kw = dict(method='bicgstab', maxiter=k, rtol=1e-300)
                x, hist, st = ctx.solve(system, rhs, start, **kw)
                ctx.common(rhs, st, hist, k)
                assert st['status'] == not_converged()
                ctx.judge(group, key, run, k, x, hist, st)
                x2, hist2, _ = ctx.solve(system, rhs, start, **kw)
                assert np.array_equal(x, x2) and np.array_equal(hist, hist2)
    report(ctx, 'bicg', form, 'latency')


@pytest.mark.parametrize('form', kl.BICG_FORMS)
def test_bicgstab_from_the_solution(ctx, form):
    """`k_bicg_start` finds the start converged: no iteration, and `x` comes
    back bit for bit"""
    from dolfin_navier_scipy_amd import _capi as C
    system = ctx.handle(form, 'latency')
    import scipy.sparse.linalg as spla
    b = ctx.rhs['time-step']
    xs = spla.spsolve(ctx.prob(form, 'latency').K.tocsc(), b)
    x = system.solve(b[:ctx.NV], b[ctx.NV:], x0=xs, method='bicgstab',
                     rtol=1e-6, maxiter=3)
    st, hist = system.last_stats, system.residual_history()
    assert st['iters'] == 0 and st['status'] == C.DNS_OK
    assert hist.size == 1 and hist[0] <= 1e-6*st['bnorm']
    assert np.array_equal(x, xs)
