"""The longdouble model of a fixed number of Krylov steps
(`tests/krylov_ld_model.py`) checked against itself: no GPU, no library.  It
fixes the tolerance `tests/test_gpu_krylov_steps.py` asserts with -- from the
model alone:

    tol = 32 max over 8 noise seeds of ||x_k(noisy) - x_k||_inf,block
          (nowhere below 16u ||x_k||_inf,block)

per run (form, right-hand side, start, `reorth`, cycle lengths), step count `k`
and block, the entries of the history likewise.  The noise (`Noise`) is what
fp64 arithmetic may do: every preconditioner output moved, entry by entry, by
the tolerance `precond_model` gives for that input (`16 max(rho_ref, 1)
(2^-53 a_i + 2^-24 a_half,i)`, `a` its yardstick, plus the entry-wise slack;
never below `16u |z_i|`), every dot product -- rows of `K z` included -- by
`16u` times the sum of the moduli of its terms.  32 ~ sqrt(1493): a random
pattern of `n` roundings falls short of an aligned one by about that.

What is a test: `tol <= 1e-10 ||x_k||_inf,block` for both blocks (`X_COND`,
`listed()`); a `k` that fails is dropped, as are the columns behind a noisy run
whose `hn^2 = <w, w> - sum h_i^2` came out `<= 0` (NaN below).  Nothing else is
dropped.  Every history entry is compared at its own tolerance, however wide
(under classical Gram-Schmidt once it reaches the size of the entry when the
residual has come down by 1e-8: those estimates are no longer determined,
the iterate still is); the GPU test also compares the dropped `k` that have a
finite tolerance at that tolerance.  Leg 4 (stop on the tolerance) runs
wherever `sqrt(h_k h_{k+1})` lies four tolerances from the entries
(`stop_between()`, `SEPARATION`): everywhere but D4 / D4f with `reorth = 2`
at `k = 6`, whose tolerances are NaN by then (at least 43 tolerances where it
runs).

The tolerances take five minutes to compute, so they are kept in
`tests/golden/krylov_steps_tol.npz` (`python tests/test_krylov_model_cpu.py`
writes it and prints the table); `test_golden_tolerances_are_the_models`
recomputes the `time-step / zero` runs of every form, every BiCGStab run and
the stagnation floor, and compares; `test_clean_runs_of_the_golden_file`
recomputes the noise-free part (norms and histories) of EVERY run.

Form / right-hand side / start / `reorth`, which `k = 1 .. 12` of ONE cycle
are listed (`x`), and `tol / ||x_k||` (the larger block) at `k` = 1, 2, 3, 5,
9, 12 (NV 1286, NP 207, `F = M + 0.5 5e-3 A`; `test_print_the_table` prints
every `k`, and the `5+5+3` runs; of those `x_13` is listed on every form for
`reorth = 0, 1`, from zero also for `reorth = 2` on J2 and MG):

    D4/rough/zero/r0       xxxxxxxxxxxx  6e-11 6e-12 4e-12 4e-12 4e-12 4e-12
    D4/rough/zero/r1       xxxxxxxxxxxx  6e-11 5e-12 4e-12 4e-12 4e-12 4e-12
    D4/rough/zero/r2       x...........  6e-11 1e-10 2e-10 nan nan nan
    D4/time-step/rough/r0  .xxxxxxxxxxx  4e-09 9e-11 6e-12 6e-12 7e-12 7e-12
    D4/time-step/rough/r1  .xxxxxxxxxxx  4e-09 9e-11 7e-12 5e-12 5e-12 5e-12
    D4/time-step/rough/r2  ............  4e-09 7e-09 7e-09 nan nan nan
    D4/time-step/zero/r0   xxxxxxxxxxxx  7e-11 5e-12 3e-12 3e-12 3e-12 3e-12
    D4/time-step/zero/r1   xxxxxxxxxxxx  7e-11 4e-12 3e-12 3e-12 3e-12 3e-12
    D4/time-step/zero/r2   x...........  7e-11 2e-10 2e-10 nan nan nan
    D4f/rough/zero/r0      xxxxxxxxxxxx  6e-11 6e-12 4e-12 4e-12 4e-12 4e-12
    D4f/rough/zero/r1      xxxxxxxxxxxx  6e-11 5e-12 4e-12 4e-12 4e-12 4e-12
    D4f/rough/zero/r2      x...........  6e-11 1e-10 2e-10 nan nan nan
    D4f/time-step/rough/r0 .xxxxxxxxxxx  4e-09 9e-11 6e-12 6e-12 7e-12 7e-12
    D4f/time-step/rough/r1 .xxxxxxxxxxx  4e-09 9e-11 7e-12 5e-12 5e-12 5e-12
    D4f/time-step/rough/r2 ............  4e-09 7e-09 7e-09 nan nan nan
    D4f/time-step/zero/r0  xxxxxxxxxxxx  7e-11 5e-12 3e-12 3e-12 3e-12 3e-12
    D4f/time-step/zero/r1  xxxxxxxxxxxx  7e-11 4e-12 3e-12 3e-12 3e-12 3e-12
    D4f/time-step/zero/r2  x...........  7e-11 2e-10 2e-10 nan nan nan
    J2/rough/zero/r0       xxxxxxxxxxxx  3e-13 1e-12 1e-12 9e-13 2e-12 3e-12
    J2/rough/zero/r1       xxxxxxxxxxxx  3e-13 1e-12 5e-13 5e-13 8e-13 9e-13
    J2/rough/zero/r2       xxxxxxxx....  3e-13 1e-12 6e-12 5e-11 1e-10 1e-10
    J2/time-step/rough/r0  xxxxxx......  3e-14 3e-13 2e-12 2e-11 3e-10 6e-10
    J2/time-step/rough/r1  xxxxxxxxxxxx  4e-14 2e-13 1e-12 1e-11 2e-11 3e-11
    J2/time-step/rough/r2  xxx.........  3e-14 5e-13 3e-11 8e-10 2e-08 5e-08
    J2/time-step/zero/r0   xxxxxxxxxxxx  7e-13 5e-13 9e-13 1e-12 4e-12 5e-12
    J2/time-step/zero/r1   xxxxxxxxxxxx  7e-13 3e-13 3e-13 4e-13 6e-13 6e-13
    J2/time-step/zero/r2   xxxxxxxx....  7e-13 2e-12 8e-12 4e-11 1e-10 1e-10
    MG/rough/zero/r0       xxxxxxxxxxxx  4e-11 1e-11 6e-12 4e-12 4e-12 4e-12
    MG/rough/zero/r1       xxxxxxxxxxxx  4e-11 1e-11 6e-12 4e-12 4e-12 4e-12
    MG/rough/zero/r2       xxxxxxxx....  4e-11 1e-11 6e-12 4e-12 nan nan
    MG/time-step/rough/r0  ..xxxxxxxxxx  1e-10 3e-10 7e-11 1e-11 8e-12 8e-12
    MG/time-step/rough/r1  ..xxxxxxxxxx  1e-10 3e-10 6e-11 8e-12 6e-12 6e-12
    MG/time-step/rough/r2  ..xxxxxx....  1e-10 3e-10 7e-11 9e-12 nan nan
    MG/time-step/zero/r0   xxxxxxxxxxxx  4e-11 2e-11 3e-12 3e-12 3e-12 3e-12
    MG/time-step/zero/r1   xxxxxxxxxxxx  4e-11 2e-11 3e-12 3e-12 3e-12 3e-12
    MG/time-step/zero/r2   xxxxxxxx....  4e-11 2e-11 3e-12 3e-12 nan nan

    bicg/D4/rough/rough          xx 6e-12 4e-12
    bicg/D4/rough/zero           xxx 6e-12 4e-12 4e-12
    bicg/D4/time-step/rough      x. 9e-11 5e-12
    bicg/D4/time-step/zero       xxx 5e-12 3e-12 3e-12
    bicg/J2/rough/rough          xx 3e-13 1e-11
    bicg/J2/rough/zero           xxx 3e-13 1e-11 2e-12
    bicg/J2/time-step/rough      xx 3e-12 1e-11
    bicg/J2/time-step/zero       xxx 3e-13 2e-11 1e-12

The runs the row-partitioned cycle adds (`tests/test_gpu_zz_dist_krylov.py`)
are in a second file, `tests/golden/krylov_dist_tol.npz` (`--dist` writes it,
two minutes; same recipe, same `listed()`): the form D4t (dense Schur,
TRIANGULAR, explicit degree 4: no `J Fh^-1`), one cycle of twelve and
`5+5+3`, and the cycle lists `1+5` (`cycle_first = 1`, `restart = 5`,
`maxiter = 6`, `reorth = 2`: the one-step cycle of a partitioned solve is
column 1 of GMRES, its `x_1`, `hist[0]`, `hist[1]` need no second model) on
D4, D4f, D4t, MG.  30 runs, 192 listed `(run, k)`; of leg 1 on D4t (`k` in 1,
2, 3, 5, 9, 12, three cases) 12, 12 and 6 of 18 for `reorth` 0, 1, 2, every
`k` among them from zero for 0 and 1; `x_1` of every `1+5` run from zero.
`test_golden_tolerances_of_the_second_file_are_the_models` recomputes the
`time-step / zero` runs of D4t and of every `1+5`, `test_clean_runs_of_the_
second_file` the noise-free part of all 30.  D4t, one cycle of twelve (as
above), and all six `k` of the `1+5` runs:

    D4t/rough/zero/r0       xxxxxxxxxxxx  4e-12 7e-11 6e-11 4e-12 4e-12 4e-12
    D4t/rough/zero/r1       xxxxxxxxxxxx  4e-12 8e-11 7e-11 3e-12 3e-12 3e-12
    D4t/rough/zero/r2       xx.xxxxxx...  4e-12 7e-11 1e-10 5e-11 5e-11 nan
    D4t/time-step/rough/r0  x...........  1e-13 1e-09 2e-09 3e-09 2e-09 2e-09
    D4t/time-step/rough/r1  x...........  1e-13 2e-09 2e-09 5e-10 2e-10 2e-10
    D4t/time-step/rough/r2  x...........  1e-13 2e-09 6e-08 8e-08 nan nan
    D4t/time-step/zero/r0   x.xxxxxxxxxx  4e-12 2e-10 8e-11 5e-12 5e-12 5e-12
    D4t/time-step/zero/r1   x.xxxxxxxxxx  4e-12 2e-10 8e-11 4e-12 4e-12 4e-12
    D4t/time-step/zero/r2   x...........  4e-12 2e-10 2e-10 2e-10 nan nan

    D4/rough/zero/r2/1+5        xxxxx.  6e-11 7e-12 7e-12 7e-12 7e-12 nan
    D4/time-step/rough/r2/1+5   .xxxx.  4e-09 9e-11 8e-12 5e-12 5e-12 nan
    D4/time-step/zero/r2/1+5    xxxxx.  7e-11 5e-12 4e-12 4e-12 4e-12 nan
    D4f/rough/zero/r2/1+5       xxxxx.  6e-11 7e-12 7e-12 7e-12 7e-12 nan
    D4f/time-step/rough/r2/1+5  .xxxx.  4e-09 9e-11 8e-12 8e-12 8e-12 nan
    D4f/time-step/zero/r2/1+5   xxxxx.  7e-11 5e-12 4e-12 4e-12 4e-12 nan
    D4t/rough/zero/r2/1+5       xx....  4e-12 4e-12 3e-10 2e-10 2e-10 2e-10
    D4t/time-step/rough/r2/1+5  xx....  1e-13 1e-13 2e-09 2e-08 3e-08 3e-08
    D4t/time-step/zero/r2/1+5   xx....  4e-12 4e-12 3e-10 3e-10 4e-10 4e-10
    MG/rough/zero/r2/1+5        xxxxxx  4e-11 2e-11 9e-12 6e-12 6e-12 6e-12
    MG/time-step/rough/r2/1+5   ....xx  1e-10 3e-10 3e-10 1e-10 3e-11 9e-12
    MG/time-step/zero/r2/1+5    xxxxxx  4e-11 3e-11 2e-11 8e-12 5e-12 4e-12

(`5+5+3` on D4t: `x_13` listed in all nine runs.  The triangular form takes
the time step's right-hand side slowly -- the residual is still 1.0 of
`||b||` after one column, 4.5e-9 after twelve -- and from the rough start every
`x_k` past the first is a small difference of large vectors.  The restart
behind the one-step cycle gives the fused form a fresh basis: D4 lists `x_2` ..
`x_5` of `1+5`, of one cycle of twelve `x_1` alone.)

What the table says about the device algorithm (each a consequence of the
code, none an error):

* explicit Gram-Schmidt (`reorth = 0, 1`) from a zero start is pinned through
  all twelve columns on every form, from the rough start from column 3 at the
  latest (J2 with `reorth = 0`: up to column 6).
* Classical Gram-Schmidt once (`reorth = 0, 2`) loses the orthogonality of the
  basis like `kappa^2 u`: once the residual has come down by 1e-4 or so
  (D4: 35 per column) the tolerance of a Givens estimate passes 1e-8 of the
  estimate, and the fused norm `<w, w> - sum h_i^2` comes out negative in noisy
  runs shortly after: that is `pythagoras_norm` returning -1 on the device.
* behind a dense or Jacobi Schur block `reorth = 2` forms
  `zp_j = (-Sh^-1 tau(w) - sum h_i zp_i) / hn` from the STORED `zp_i`: what
  those carry of rounding is multiplied by `h_i / hn` column after column
  (35 per column on D4).  The iterate stays a valid flexible-GMRES iterate
  (`x += Z y` with the same `Z`), but which one is not determined to 1e-10
  beyond `k = 1` (D4), `k = 8` (J2).
* a rough start leaves `x_1`, `x_2` of D4 / MG a small difference of large
  vectors: not determined to 1e-10 either.

Stagnation (D4, one fused cycle of 40 columns from zero, `||b|| = 3.6e-2`):
the smallest true residual norm the model reaches is 1.6e-10 -- the fused
longdouble run ends at column 7, where `hn^2 <= 0` -- and the same for its
iterates rounded to fp64; the GPU test allows 32 times that.  (With the noise
hook: 7.5e-09, the largest of the eight seeds.)

Mutations (each must leave the tolerance of at least one listed case by a
factor 100; the largest `error / tol` over the listed cases):

    drop_last_z    the last column left out of `Z y`               3.7e+12
    no_x0          `x0` not added                                  5.6e+14
    givens_prev    rotation j-1 with (c, s) of column j-2          3.1e+12
    backsub_T      `R[k, i]` for `R[i, k]` in the back substitution 4.4e+12
    no_fold_corr   `- sum h_i zp_i` dropped from `zp_j`            2.8e+11
    hist_shift     the history shifted by one                      4.2e+13
    beta_plain     BiCGStab: `beta` without `alpha / omega`        4.2e+11
    parity         BiCGStab: the scalars of the other parity slot  1.9e+12
    omega_ss       BiCGStab: `omega = (t.s) / (s.s)`               1.0e+12
    lazy_no_norm   one-step cycle: `alpha = <w, r>`, not `/ <w, w>` 2.8e+15
"""
import os
import sys
import warnings

import numpy as np
import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import krylov_model as km
import krylov_ld_model as kl

warnings.filterwarnings('ignore', 'invalid value encountered')


@pytest.fixture(scope='module')
def bench(toy_prob):
    return kl.toy_bench(toy_prob)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, kl.GOLDEN)))


@pytest.fixture(scope='module')
def golden_dist(golden_dir):
    return dict(np.load(os.path.join(golden_dir, kl.GOLDEN_DIST)))


@pytest.fixture(scope='module')
def probs(bench):
    return dict((name, kl.Problem(bench, f)) for name, f in kl.FORMS.items())


def runs_of(tab, kind):
    return sorted(k[:-3] for k in tab if k.startswith(kind) and
                  k.endswith('/tx'))


def table_lines(tab):
    out = []
    for key in runs_of(tab, 'gmres') + runs_of(tab, 'bicg'):
        tx, nx = tab[key + '/tx'], tab[key + '/nx']
        rel = (tx/nx).max(axis=1)
        marks = ''.join('x' if kl.listed(tab, key, k + 1) else '.'
                        for k in range(len(rel)))
        out.append('    %-36s %s  %s' % (
            key, marks, ' '.join('%.0e' % q for q in rel)))
    return out


def test_print_the_table(golden):
    print()
    for line in table_lines(golden):
        print(line)
    print('    stagnation: noisy %.2e  clean %.2e  clean, rounded to fp64 '
          '%.2e  ||b|| %.2e' % tuple(golden['stagnation']))


def test_every_run_is_in_the_golden_file(golden):
    want = []
    for form in kl.FORMS:
        for rhs, start, cycles in kl.gmres_runs(form):
            want += [kl.gmres_key(form, rhs, start, r, cycles)
                     for r in kl.REORTHS]
    assert sorted(want) == runs_of(golden, 'gmres')
    want = [kl.bicg_key(form, rhs, start) for form in kl.BICG_FORMS
            for rhs in ('time-step', 'rough') for start in kl.BICG_K]
    assert sorted(want) == runs_of(golden, 'bicg')
    for key in runs_of(golden, 'gmres'):
        n = sum(int(c) for c in key.split('/')[-1].split('+'))
        assert golden[key + '/tx'].shape == (n, 2)
        assert golden[key + '/th'].shape == (n + 1,)


def test_golden_tolerances_are_the_models(bench, golden):
    """recomputed: the `time-step / zero` cycle of twelve of every form, all
    of BiCGStab, the stagnation floor"""
    tab = kl.tolerance_table(bench, cases=(('time-step', 'zero'),), leg3=())
    assert len(tab) == 4*12 + 2*16 + 1
    # the clean runs are longdouble arithmetic alone: the same everywhere.
    # The noisy ones take their amplitudes from fp64 products (the
    # yardsticks), whose last digit may depend on the BLAS at hand: what is
    # listed is well conditioned and must agree, what is not listed amplifies
    # such a digit by up to 35 per column and is only required to stay
    # unlisted (and to separate the same stops of leg 4)
    for key in runs_of(tab, 'gmres') + runs_of(tab, 'bicg'):
        for s in ('/nx', '/h'):
            assert np.allclose(tab[key + s], golden[key + s], rtol=1e-9,
                               atol=0., equal_nan=True), key
        for k in range(1, len(tab[key + '/tx']) + 1):
            assert kl.listed(tab, key, k) == kl.listed(golden, key, k), key
            if kl.listed(tab, key, k):
                assert np.allclose(tab[key + '/tx'][k - 1],
                                   golden[key + '/tx'][k - 1], rtol=1e-2)
                # (history entries: where the noise leaves six digits)
                th, h = golden[key + '/th'][:k + 1], golden[key + '/h'][:k + 1]
                ok = th <= 1e-6*h
                assert np.allclose(tab[key + '/th'][:k + 1][ok], th[ok],
                                   rtol=1e-2)
        if key.endswith('/12'):
            for k in kl.LEG4_K:
                assert (kl.stop_between(tab, key, k) is None) == \
                    (kl.stop_between(golden, key, k) is None), (key, k)
    noisy, clean, rounded, bnorm = tab['stagnation']
    assert 0.5 <= noisy/golden['stagnation'][0] <= 2.
    assert np.allclose([clean, rounded, bnorm], golden['stagnation'][1:],
                       rtol=1e-6)


def test_golden_tolerances_of_the_second_file_are_the_models(bench,
                                                             golden_dist):
    """the same comparison for `krylov_dist_tol.npz`: the `time-step / zero`
    runs of D4t (12, 5+5+3, all three `reorth`) and the `1+5` run of every
    form of `LAZY_FORMS` from `time-step / zero`"""
    tab = kl.dist_tolerance_table(bench, runs=kl.dist_runs(
        cases=(('time-step', 'zero'),), lazy_cases=(('time-step', 'zero'),)))
    assert len(tab) == 4*(2*3 + 4)
    for key in runs_of(tab, 'gmres'):
        for s in ('/nx', '/h'):
            assert np.allclose(tab[key + s], golden_dist[key + s], rtol=1e-9,
                               atol=0., equal_nan=True), key
        for k in range(1, len(tab[key + '/tx']) + 1):
            assert kl.listed(tab, key, k) == kl.listed(golden_dist, key, k), \
                (key, k)
            if kl.listed(tab, key, k):
                assert np.allclose(tab[key + '/tx'][k - 1],
                                   golden_dist[key + '/tx'][k - 1], rtol=1e-2)
                th = golden_dist[key + '/th'][:k + 1]
                h = golden_dist[key + '/h'][:k + 1]
                ok = th <= 1e-6*h
                assert np.allclose(tab[key + '/th'][:k + 1][ok], th[ok],
                                   rtol=1e-2)
        if key.endswith('/12'):
            for k in kl.LEG4_K:
                assert (kl.stop_between(tab, key, k) is None) == \
                    (kl.stop_between(golden_dist, key, k) is None), (key, k)


def test_clean_runs_of_the_second_file(bench, golden_dist):
    """the noise-free arrays of EVERY run in `krylov_dist_tol.npz`"""
    tab = kl.dist_clean_table(bench)
    assert sorted(tab) == sorted(k for k in golden_dist
                                 if k.endswith(('/nx', '/h')))
    for key, val in tab.items():
        assert np.allclose(val, golden_dist[key], rtol=1e-9, atol=0.,
                           equal_nan=True), key


def test_print_the_second_table(golden_dist):
    print()
    for line in table_lines(golden_dist):
        print(line)


def test_what_is_listed_in_the_second_file(golden, golden_dist):
    """the runs, the shapes and the listed set of `krylov_dist_tol.npz` are
    what the module docstring says; no key of the first file is repeated"""
    want = []
    for form, rhs, start, cycles, reorths in kl.dist_runs():
        want += [kl.gmres_key(form, rhs, start, r, cycles) for r in reorths]
    assert sorted(want) == runs_of(golden_dist, 'gmres')
    assert len(want) == 18 + 12 and not set(golden_dist) & set(golden)
    assert runs_of(golden_dist, 'bicg') == []

    def ks(form, rhs, start, reorth, cycles=kl.LONG):
        key = kl.gmres_key(form, rhs, start, reorth, cycles)
        return [k for k in range(1, sum(cycles) + 1)
                if kl.listed(golden_dist, key, k)]
    count = 0
    for key in want:
        n = sum(int(c) for c in key.split('/')[-1].split('+'))
        tx, th, nx = (golden_dist[key + s] for s in ('/tx', '/th', '/nx'))
        assert tx.shape == (n, 2) and th.shape == (n + 1,)
        for k in range(1, n + 1):
            if kl.listed(golden_dist, key, k):
                count += 1
                assert (tx[k - 1] <= 1e-10*nx[k - 1]).all()
                assert (tx[k - 1] >= 16*kl.U64*nx[k - 1]).all()
                assert np.isfinite(th[:k + 1]).all()
    assert count == 192
    every = list(range(1, 13))
    for r in (0, 1):
        # D4t, explicit Gram-Schmidt: the rough right-hand side from zero
        # through all twelve columns (every `k` of leg 1), the time step's
        # all but `x_2` (2e-10); from the rough start `x_1` alone in one
        # cycle and `x_13` of the restarted run
        assert ks('D4t', 'rough', 'zero', r) == every
        assert ks('D4t', 'time-step', 'zero', r) == [1] + every[2:]
        assert ks('D4t', 'time-step', 'rough', r) == [1]
        for rhs, start in kl.CASES:
            assert 13 in ks('D4t', rhs, start, r, kl.RESTARTED)
    # fused: the first column everywhere
    for rhs, start in kl.CASES:
        assert 1 in ks('D4t', rhs, start, 2)
    # leg 1 (`LEG1_K` of the three cases): 12, 12 and 6 of 18
    for r, n in ((0, 12), (1, 12), (2, 6)):
        assert sum(k in ks('D4t', rhs, start, r) for rhs, start in kl.CASES
                   for k in kl.LEG1_K) == n
    # the one-step cycle and the cycle of five behind it: `x_1` from zero on
    # every form; `x_6` on MG alone (dense block: NaN by the fifth fused
    # column, D4t: 3e-10 from the third)
    for form in kl.LAZY_FORMS:
        for rhs in ('time-step', 'rough'):
            assert 1 in ks(form, rhs, 'zero', 2, kl.LAZY)
        assert (6 in ks(form, 'time-step', 'zero', 2, kl.LAZY)) == \
            (form == 'MG')
    assert ks('D4', 'time-step', 'zero', 2, kl.LAZY) == [1, 2, 3, 4, 5]
    assert ks('D4t', 'time-step', 'zero', 2, kl.LAZY) == [1, 2]


def test_clean_runs_of_the_golden_file(bench, golden):
    """the noise-free arrays of every run in the file, recomputed"""
    tab = kl.clean_table(bench)
    assert sorted(tab) == sorted(k for k in golden if k.endswith(('/nx', '/h')))
    for key, val in tab.items():
        assert np.allclose(val, golden[key], rtol=1e-9, atol=0.,
                           equal_nan=True), key


def test_what_is_listed(golden):
    """the condition holds on everything listed (by construction of `listed`:
    spelled out here once more), and the listed set is what the module
    docstring says it is"""
    def ks(form, rhs, start, reorth, cycles=kl.LONG):
        key = kl.gmres_key(form, rhs, start, reorth, cycles)
        return [k for k in range(1, sum(cycles) + 1)
                if kl.listed(golden, key, k)]
    for key in runs_of(golden, 'gmres') + runs_of(golden, 'bicg'):
        tx, th, nx = (golden[key + s] for s in ('/tx', '/th', '/nx'))
        for k in range(1, len(tx) + 1):
            if kl.listed(golden, key, k):
                assert (tx[k - 1] <= 1e-10*nx[k - 1]).all()
                assert (tx[k - 1] >= 16*kl.U64*nx[k - 1]).all()
                assert np.isfinite(th[:k + 1]).all()
    every = list(range(1, 13))
    for form in kl.FORMS:
        for rhs in ('time-step', 'rough'):
            # explicit Gram-Schmidt, once or twice, from zero: all twelve
            # columns on every form; the first column of the fused form
            for r in (0, 1):
                assert ks(form, rhs, 'zero', r) == every
            assert 1 in ks(form, rhs, 'zero', 2)
        # the rough start: from column 3 at the latest
        assert ks(form, 'time-step', 'rough', 1)[-10:] == every[2:]
        # fused, from zero: D4 one column, J2 and MG eight
        want = [1] if form.startswith('D4') else every[:8]
        assert ks(form, 'time-step', 'zero', 2) == want
    # the restarted run (leg 3), `x_13`: every form with explicit
    # Gram-Schmidt, every case; fused from zero on J2 and MG (D4: NaN from
    # the second column)
    for form in kl.LEG3_FORMS:
        for rhs, start in kl.CASES:
            for r in (0, 1):
                assert 13 in ks(form, rhs, start, r, kl.RESTARTED)
        assert (13 in ks(form, 'time-step', 'zero', 2, kl.RESTARTED)) == \
            (not form.startswith('D4'))
    # BiCGStab: three steps from zero, two from the rough start (the issue's
    # bound on the step count), one case short of it
    for form in kl.BICG_FORMS:
        for rhs in ('time-step', 'rough'):
            for start, k in kl.BICG_K.items():
                key = kl.bicg_key(form, rhs, start)
                got = [kl.listed(golden, key, i) for i in range(1, k + 1)]
                assert all(got) or key == 'bicg/D4/time-step/rough', key


def test_stop_on_the_tolerance_falls_between_two_entries(golden):
    """leg 4: where it runs, `rtol ||b|| = sqrt(h_k h_{k+1})` lies
    `SEPARATION` tolerances below `h_0 .. h_k` and above `h_{k+1}`
    (`stop_between`), and a factor of two from both wherever the
    preconditioner converges at all (J2: 12 columns leave 0.37 of the
    residual, its entries are 3 to 20 % apart).  It runs for every form,
    Gram-Schmidt form, right-hand side, start and `k` but `LEG4_NOT_RUN`"""
    for form in kl.FORMS:
        ran = kl.leg4_runs(golden, form)
        every = [(r, rhs, start, k) for r in kl.REORTHS
                 for rhs, start in kl.CASES for k in kl.LEG4_K]
        assert [c for c in every if c not in ran] == kl.LEG4_NOT_RUN[form]
        worst = np.inf
        for r, rhs, start, k in ran:
            key = kl.gmres_key(form, rhs, start, r, kl.LONG)
            h, th = golden[key + '/h'], golden[key + '/th']
            stop = np.sqrt(h[k]*h[k + 1])
            worst = min(worst, ((h[:k + 1] - stop)/th[:k + 1]).min(),
                        (stop - h[k + 1])/th[k + 1])
            if form != 'J2':
                assert h[k]/h[k + 1] >= 2., (key, k, h[k]/h[k + 1])
        print('    leg 4 %-3s: %d of 18 (reorth, case, k), the stop at least '
              '%.0f tolerances from the entries' % (form, len(ran), worst))
        assert worst >= kl.SEPARATION


def test_stagnation_floor(golden):
    noisy, clean, rounded, bnorm = golden['stagnation']
    # (the yardstick of the GPU test is the clean model's, which its iterates
    # rounded to fp64 reach as well)
    assert clean <= rounded*(1 + 1e-6) and rounded <= noisy
    assert clean <= 1e-8*bnorm


# ---- the longdouble model against the fp64 one -----------------------------------
@pytest.mark.parametrize('form', list(kl.FORMS))
def test_gmres_agrees_with_the_fp64_model(bench, probs, golden, form):
    """`krylov_model.gmres` (CGS twice, `x += P^-1 (V y)`) on the fp64
    preconditioner model: the same iterate in exact arithmetic, so within the
    tolerance of the GPU test in fp64"""
    prob = probs[form]
    b = kl.right_hand_sides(bench)['time-step']
    xs, hist, res = kl.gmres_cycles(prob, b, None, kl.LONG, 1)
    key = kl.gmres_key(form, 'time-step', 'zero', 1, kl.LONG)
    for k in kl.LEG1_K:
        x, h, its = km.gmres(prob.K, b, prob.m64, rtol=0., restart=k,
                             maxiter=k, reorth=True)
        assert its == k and len(h) == k + 2    # (km: beta of the next cycle)
        d = np.abs(x - xs[k - 1])
        ex = max(float(d[:prob.NV].max()/golden[key + '/tx'][k - 1, 0]),
                 float(d[prob.NV:].max()/golden[key + '/tx'][k - 1, 1]))
        eh = float((np.abs(h[:k + 1] - hist[:k + 1]) /
                    golden[key + '/th'][:k + 1]).max())
        print('%s k=%2d fp64 model: error / tol %.3f (x) %.3f (history)'
              % (form, k, ex, eh))
        assert ex <= 1. and eh <= 1.
        # the true residual the model reports is the one of its iterate
        # (while fp64 can tell: above 1e-8 of the first one)
        if res[k - 1] >= 1e-8*hist[0]:
            assert abs(h[k + 1] - res[k - 1]) <= 1e-6*res[k - 1]


@pytest.mark.parametrize('form', kl.BICG_FORMS)
def test_bicgstab_agrees_with_the_fp64_model(bench, probs, golden, form):
    prob = probs[form]
    b = kl.right_hand_sides(bench)['time-step']
    xs, hist = kl.bicgstab_steps(prob, b, None, 3)
    key = kl.bicg_key(form, 'time-step', 'zero')
    for k in (1, 2, 3):
        x, h, its = km.bicgstab(prob.K, b, prob.m64, rtol=0., maxiter=k)
        assert its == k
        d = np.abs(x - xs[k - 1])
        ex = max(float(d[:prob.NV].max()/golden[key + '/tx'][k - 1, 0]),
                 float(d[prob.NV:].max()/golden[key + '/tx'][k - 1, 1]))
        eh = float((np.abs(h - hist[:k + 1])/golden[key + '/th'][:k + 1]).max())
        print('%s k=%d fp64 model: error / tol %.3f (x) %.3f (history)'
              % (form, k, ex, eh))
        assert ex <= 1. and eh <= 1.


def test_the_three_gram_schmidt_forms_are_one_iterate(bench, probs):
    """in longdouble the three `reorth` give the same `x_k` (they differ in
    how the noise gets in, which is what the tolerances show)"""
    prob = probs['J2']
    b = kl.right_hand_sides(bench)['time-step']
    ref = kl.gmres_cycles(prob, b, None, kl.LONG, 1)[0]
    for reorth in (0, 2):
        xs = kl.gmres_cycles(prob, b, None, kl.LONG, reorth)[0]
        assert np.abs(xs - ref).max() <= 1e-15*np.abs(ref).max()


# ---- mutations -------------------------------------------------------------------
def excess(tab, key, out, clean, NV, ks):
    """largest `error / tol` of a (wrong) run over the listed `k` of `ks`"""
    worst = 0.
    for k in ks:
        if not kl.listed(tab, key, k):
            continue
        d = np.abs(out[0][k - 1] - clean[0][k - 1])
        worst = max(worst, float(d[:NV].max()/tab[key + '/tx'][k - 1, 0]),
                    float(d[NV:].max()/tab[key + '/tx'][k - 1, 1]),
                    float((np.abs(out[1][:k + 1] - clean[1][:k + 1]) /
                           tab[key + '/th'][:k + 1]).max()))
    return worst


def mutation_excess(bench, probs, golden, mut):
    rhs_of, start_of = kl.right_hand_sides(bench), kl.starts(bench)
    worst = 0.
    if mut in kl.GMRES_MUTATIONS:
        for form in ('J2', 'D4'):
            prob = probs[form]
            for rhs, start in kl.CASES[:2]:
                for reorth in (1, 2):
                    args = (prob, rhs_of[rhs], start_of[start], kl.LONG,
                            reorth)
                    key = kl.gmres_key(form, rhs, start, reorth, kl.LONG)
                    worst = max(worst, excess(
                        golden, key, kl.gmres_cycles(*args, mut=mut),
                        kl.gmres_cycles(*args), prob.NV, kl.LEG1_K))
    else:
        for form in kl.BICG_FORMS:
            prob = probs[form]
            for start, k in kl.BICG_K.items():
                args = (prob, rhs_of['rough'], start_of[start], k)
                key = kl.bicg_key(form, 'rough', start)
                worst = max(worst, excess(
                    golden, key, kl.bicgstab_steps(*args, mut=mut),
                    kl.bicgstab_steps(*args), prob.NV, range(1, k + 1)))
    return worst


@pytest.mark.parametrize('mut', kl.GMRES_MUTATIONS + kl.BICG_MUTATIONS)
def test_mutation_is_caught(bench, probs, golden, mut):
    ex = mutation_excess(bench, probs, golden, mut)
    print('    %-14s error / tol %.1e' % (mut, ex))
    assert ex >= 100.


@pytest.mark.parametrize('mut', kl.LAZY_MUTATIONS)
def test_mutation_of_the_one_step_cycle_is_caught(bench, probs, golden_dist,
                                                  mut):
    """`x_1` and the rows behind it of the `1+5` runs (D4 and D4t, the two
    starts of the time step's right-hand side)"""
    rhs_of, start_of = kl.right_hand_sides(bench), kl.starts(bench)
    worst = 0.
    for form in ('D4', 'D4t'):
        prob = probs[form] if form in probs else \
            kl.Problem(bench, kl.ALL_FORMS[form])
        for rhs, start in kl.CASES[:2]:
            args = (prob, rhs_of[rhs], start_of[start], kl.LAZY, 2)
            key = kl.gmres_key(form, rhs, start, 2, kl.LAZY)
            worst = max(worst, excess(
                golden_dist, key, kl.gmres_cycles(*args, mut=mut),
                kl.gmres_cycles(*args), prob.NV, range(1, 7)))
    print('    %-14s error / tol %.1e' % (mut, worst))
    assert worst >= 100.


if __name__ == '__main__':
    # no argument: write the golden file and print the table (five minutes);
    # `--check`: recompute ALL of it and compare with the file instead
    # `--dist`: the second file (`krylov_dist_tol.npz`, two minutes) alone
    import scenarios
    bench_ = kl.toy_bench(scenarios.toy_problem())
    here = os.path.dirname(os.path.abspath(__file__))
    if '--dist' in sys.argv:
        tab_ = kl.dist_tolerance_table(bench_,
                                       log=lambda k: print(k, flush=True))
        np.savez_compressed(os.path.join(here, 'golden', kl.GOLDEN_DIST),
                            **tab_)
        for line_ in table_lines(tab_):
            print(line_)
        sys.exit(0)
    tab_ = kl.tolerance_table(bench_, log=lambda k: print(k, flush=True))
    path_ = os.path.join(here, 'golden', kl.GOLDEN)
    if '--check' in sys.argv:
        old_ = dict(np.load(path_))
        assert sorted(old_) == sorted(tab_)
        for key_ in runs_of(tab_, 'gmres') + runs_of(tab_, 'bicg'):
            for k_ in range(1, len(tab_[key_ + '/tx']) + 1):
                assert kl.listed(tab_, key_, k_) == kl.listed(old_, key_, k_)
                if kl.listed(tab_, key_, k_):
                    assert np.allclose(tab_[key_ + '/tx'][k_ - 1],
                                       old_[key_ + '/tx'][k_ - 1], rtol=1e-2)
        print('the golden file is the model\'s')
        sys.exit(0)
    np.savez_compressed(path_, **tab_)
    for line_ in table_lines(tab_):
        print(line_)
    print(tab_['stagnation'])
