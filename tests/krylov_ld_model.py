"""`np.longdouble` model of a FIXED number of Krylov steps as the device takes
them (test infrastructure, HIP-free; nothing in the package imports it).

`gmres_cycles` and `bicgstab_steps` mirror the ALGORITHM of `dns_saddle::gmres`
/ `enqueue_cycle` / `gmres_kernels.hpp` and of `dns_saddle::bicgstab` /
`bicgstab_kernels.hpp`, not their rounding:

* right preconditioning with the preconditioned vectors kept, `x += Z y`
  (`k_arn_tail_acc`, `k_basis_combine_acc`), never `P^-1 (V y)`;
* a cycle starts from a freshly computed residual `b - K x`;
* `reorth = 0`: classical Gram-Schmidt once, `hn = ||w - V h||`;
  `reorth = 1`: twice, `h` the sum of both passes (`k_orth<1>`, `k_orth<0>`);
  `reorth = 2`: once, `hn^2 = <w, w> - sum h_i^2` (`pythagoras_norm`) and,
  behind a dense or Jacobi Schur block, the pressure part of `z_j` by
  linearity,
  `zp_j = (-Sh^-1 tau(w) - sum h_i zp_i) / hn` (`k_arn_head_f`); the multigrid
  block is applied to `V_j` itself;
* Givens rotations and the back substitution of `givens_close` / `k_arn_tail`;
* the history as the device appends it: `beta_0`, then one Givens estimate per
  column, the first entry (`beta`) of every later cycle skipped;
* BiCGStab with the scalars `(rho, alpha, omega)` double buffered by the parity
  of the iteration (`BicgCtl::sc[par]`: iteration `it` reads slot `it & 1` and
  writes the other one).

Matrix products run in longdouble (`precond_model.spmm_ld`), the preconditioner
is the longdouble model of `precond_model.build(.., ld=True)` (`Problem`).

The noise hook (`Noise`) is the model of what fp64 arithmetic may do to these
steps: every preconditioner output is moved entry by entry by
`max(t_i, 16u |z_i|) U(-1, 1)`, `t` the tolerance of `precond_model` for THAT
input taken entry by entry -- `16 max(rho_ref, 1) (2^-53 a_i + 2^-24 a_half,i)`
with the yardstick `a` of `Precond.yardsticks` and the `rho_ref` of the input's
block, plus the entry-wise `slack` (`Problem.tol_entry`; the tests of the
apply use the largest entry of a block for all of it) -- and every dot
product, the rows of `K z` among them, by `16u` times the sum of the moduli of
its terms times `U(-1, 1)`.  Seeds are fixed.  `tolerances()` turns eight noisy
runs into the tolerance of the GPU test (`tests/test_krylov_model_cpu.py` says
how and checks it).

`mut`: deliberately WRONG variants, the mutations of the CPU test.
"""
import numpy as np

import krylov_model as km
import precond_model as pm

LD = np.longdouble
U64 = pm.U64
SEEDS = tuple(range(101, 109))          # the eight noise seeds
FACTOR = 32                             # ~ sqrt(1493), see the CPU test

GMRES_MUTATIONS = ('drop_last_z', 'no_x0', 'givens_prev', 'backsub_T',
                   'no_fold_corr', 'hist_shift')
# (of the one-step cycle of the row-partitioned solve, `k_arn_tail_lazy1`)
LAZY_MUTATIONS = ('lazy_no_norm',)
BICG_MUTATIONS = ('beta_plain', 'parity', 'omega_ss')


def norm_ld(v):
    v = np.asarray(v, dtype=LD)
    return np.sqrt(v @ v)


class Problem(object):
    """`K = [[F, J^T], [J, 0]]`, the fp64 model of the form `f` (the source of
    the preconditioner's tolerance) and its longdouble twin (the
    preconditioner of the Krylov model)"""

    def __init__(self, bench, f, lo=None, hi=None, entry='gmres'):
        lo = bench.lo if lo is None else lo
        hi = bench.hi if hi is None else hi
        self.NV, self.NP = bench.NV, bench.NP
        self.n = self.NV + self.NP
        self.K = km.saddle(bench.F, bench.J).tocsr()
        self.aK = abs(self.K).tocsr()
        self.m64 = bench.model(f, lo, hi, entry)
        self.P = pm.build(bench.F, bench.J, lo, hi, f, bench.prols,
                          entry=entry, cache=bench.cld, ld=True,
                          stored=self.m64)
        # `k_arn_head_f<0..2>` folds the Gram-Schmidt update into `zp_j`,
        # `<3>` leaves the multigrid block to the kernels behind it
        self.fold = f['schur'] != 'mg'

    def mv(self, x):
        return pm.spmm_ld(self.K, x)

    def apply(self, r):
        return self.P.apply(r)

    def schur_part(self, r):
        """`z_p` of `r` alone (`-Sh^-1 tau(r)`)"""
        r = np.asarray(r, dtype=LD)
        pg, last = self.P.program()
        return pg.run(dict(rv=r[:self.NV], rp=r[self.NV:]))[0][last]

    def vel_part(self, rv, zp):
        """`z_v = Fh^-1 (r_v - J^T z_p)` as `Precond.apply` forms it"""
        P = self.P
        if P.fhat == 'explicit':
            return P.Gc @ np.concatenate([rv, zp])
        return P._fhat_vec(rv - pm.spmm_ld(P.J.T.tocsr(), zp))

    def tol_entry(self, v):
        """the entry-wise tolerance of `P^-1 v` (`precond_model`)"""
        v = np.asarray(v, dtype=np.float64)
        yard = self.m64.yardsticks([v])
        rho = pm.rho_ref(self.m64, self.P, [v], yard)[0]
        a, ah = yard[0]
        fac = np.concatenate([np.full(self.NV, 16*max(rho[0], 1.)),
                              np.full(self.NP, 16*max(rho[1], 1.))])
        return fac*(U64*a + pm.U32*ah) + self.m64.slack(v) \
            + self.m64.yard_slack[0]


class Noise(object):
    """the noise hook (module docstring).  `tols`: a list shared by the runs
    of one case -- the tolerance of the preconditioner's `i`-th input is
    worked out by the first run that gets there (the inputs of two runs of
    one case differ by the noise alone)"""

    def __init__(self, prob, seed, tols):
        self.prob = prob
        self.rng = np.random.default_rng(seed)
        self.tols = tols
        self.count = 0

    def _u(self, shape=None):
        return self.rng.uniform(-1.0, 1.0, shape).astype(LD) \
            if shape is not None else LD(self.rng.uniform(-1.0, 1.0))

    def precond(self, z, v):
        if self.count == len(self.tols):
            self.tols.append(self.prob.tol_entry(v))
        t = np.maximum(self.tols[self.count].astype(LD), 16*U64*np.abs(z))
        self.count += 1
        return z + t*self._u(z.shape)

    def mv(self, w, z):
        return w + 16*U64*pm.spmm_ld(self.prob.aK, np.abs(z))*self._u(w.shape)

    def dot(self, s, a, b):
        return s + 16*U64*(np.abs(a) @ np.abs(b))*self._u()

    def dots(self, h, V, w):
        return h + 16*U64*(np.abs(V) @ np.abs(w))*self._u(h.shape)


class _Quiet(object):
    """no noise"""

    def precond(self, z, v):
        return z

    def mv(self, w, z):
        return w

    def dot(self, s, a, b):
        return s

    def dots(self, h, V, w):
        return h


def gmres_cycles(prob, b, x0, cycles, reorth, noise=None, mut=None):
    """`(xs, hist, res)`: `x` after every column (an array of
    `sum(cycles)` rows), the history as the device lays it out, the true
    residual norm of every `x_k` (no noise in that one).  `prob`: a `Problem`
    (`K` and `P`)"""
    nz = _Quiet() if noise is None else noise
    NV = prob.NV
    b = np.asarray(b, dtype=LD)
    xstart = np.zeros(prob.n, dtype=LD) if x0 is None \
        else np.asarray(x0, dtype=LD)
    x = xstart.copy()
    xs, hist, res = [], [], []
    for cyc, c in enumerate(cycles):
        r = b - nz.mv(prob.mv(x), x)
        beta = np.sqrt(nz.dot(r @ r, r, r))
        if cyc == 0:
            hist.append(beta)
        V = np.zeros((c + 1, prob.n), dtype=LD)
        Z = np.zeros((c, prob.n), dtype=LD)
        R = np.zeros((c + 1, c), dtype=LD)
        cs, sn, g = np.zeros(c, LD), np.zeros(c, LD), np.zeros(c + 1, LD)
        V[0] = r/beta
        g[0] = beta
        h = hn = wraw = None
        for j in range(c):
            if j > 0 and reorth == 2 and prob.fold:
                zp = prob.schur_part(wraw)
                if mut != 'no_fold_corr':
                    zp = zp - Z[:j, NV:].T @ h
                zp = zp/hn
                z = np.concatenate([prob.vel_part(V[j, :NV], zp), zp])
            else:
                z = prob.apply(V[j])
            Z[j] = z = nz.precond(z, V[j])
            w = nz.mv(prob.mv(z), z)
            if j == 0:
                w0 = w
            Vj = V[:j + 1]
            h = nz.dots(Vj @ w, Vj, w)
            if reorth == 2:
                ww = nz.dot(w @ w, w, w)
                with np.errstate(invalid='ignore'):
                    hn = np.sqrt(ww - h @ h)        # (NaN: see below)
                wraw = w
                w = w - Vj.T @ h
            else:
                w = w - Vj.T @ h
                if reorth == 1:
                    h2 = nz.dots(Vj @ w, Vj, w)
                    w = w - Vj.T @ h2
                    h = h + h2
                hn = np.sqrt(nz.dot(w @ w, w, w))
            if not hn > 0:
                # (`hn^2 <= 0`: the space is exhausted to the last digit; no
                # further column means anything)
                nan = np.full(prob.n, np.nan, dtype=LD)
                left = sum(cycles) - len(xs)
                return (np.array(xs + [nan]*left),
                        np.array(hist + [LD(np.nan)]*left),
                        np.array(res + [LD(np.nan)]*left))
            V[j + 1] = w/hn
            # givens_close
            col = np.concatenate([h, [hn]])
            for i in range(j):
                ci, si = cs[i], sn[i]
                if mut == 'givens_prev' and i == j - 1 and i >= 1:
                    ci, si = cs[i - 1], sn[i - 1]
                t = ci*col[i] + si*col[i + 1]
                col[i + 1] = -si*col[i] + ci*col[i + 1]
                col[i] = t
            den = np.hypot(col[j], col[j + 1])
            cs[j], sn[j] = col[j]/den, col[j + 1]/den
            col[j], col[j + 1] = den, 0
            R[:j + 2, j] = col
            g[j + 1] = -sn[j]*g[j]
            g[j] = cs[j]*g[j]
            hist.append(abs(g[j + 1]))
            # the tail behind column j: y = R^-1 g, x += Z y
            jc = j + 1
            y = np.zeros(jc, dtype=LD)
            for i in range(jc - 1, -1, -1):
                s = g[i]
                for k in range(i + 1, jc):
                    s = s - (R[k, i] if mut == 'backsub_T' else R[i, k])*y[k]
                y[i] = s/R[i, i]
            if mut == 'drop_last_z':
                y[jc - 1] = 0
            xk = x + Z[:jc].T @ y
            if mut == 'lazy_no_norm' and cyc == 0 and c == 1:
                # the one-step cycle on the un-normalised `V_0 = r`:
                # `x += (<w, r> / <w, w>) z`, here without the division
                zr, wr = beta*Z[0], beta*w0
                xk = x + (wr @ r)*zr
            xs.append(xk - xstart if mut == 'no_x0' else xk)
            res.append(norm_ld(b - prob.mv(xk)))
        x = xk
    hist = np.array(hist, dtype=LD)
    if mut == 'hist_shift':
        hist = np.concatenate([hist[1:], hist[-1:]])
    return np.array(xs), hist, np.array(res, dtype=LD)


def bicgstab_steps(prob, b, x0, k, noise=None, mut=None):
    """`(xs, hist)`: `x` after each of `k` iterations and `hist[0..k]`, by the
    recurrences of `k_bicg_start / p / s / x`"""
    nz = _Quiet() if noise is None else noise
    b = np.asarray(b, dtype=LD)
    x = np.zeros(prob.n, dtype=LD) if x0 is None else np.asarray(x0, dtype=LD)
    r = b - nz.mv(prob.mv(x), x)
    rhat = r.copy()
    p, v = np.zeros(prob.n, dtype=LD), np.zeros(prob.n, dtype=LD)
    one = LD(1)
    sc = [(one, one, one), (one, one, one)]
    rr = nn = nz.dot(r @ r, r, r)   # (`partR` serves as both at the start)
    hist, xs = [np.sqrt(nn)], []
    for it in range(k):
        par = it & 1
        rho, alpha_o, omega_o = sc[par ^ 1 if mut == 'parity' else par]
        rho_new = rr
        beta = rho_new/rho
        if mut != 'beta_plain':
            beta = beta*(alpha_o/omega_o)
        p = r + beta*(p - omega_o*v)
        y = nz.precond(prob.apply(p), p)
        v = nz.mv(prob.mv(y), y)
        alpha = rho_new/nz.dot(rhat @ v, rhat, v)
        s = r - alpha*v
        z = nz.precond(prob.apply(s), s)
        t = nz.mv(prob.mv(z), z)
        ts = nz.dot(t @ s, t, s)
        omega = ts/(nz.dot(s @ s, s, s) if mut == 'omega_ss'
                    else nz.dot(t @ t, t, t))
        x = x + alpha*y + omega*z
        r = s - omega*t
        rr = nz.dot(rhat @ r, rhat, r)
        nn = nz.dot(r @ r, r, r)
        sc[par ^ 1] = (rho_new, alpha, omega)
        hist.append(np.sqrt(nn))
        xs.append(x)
    return np.array(xs), np.array(hist, dtype=LD)


def tolerances(run, prob, seeds=SEEDS, tols=None):
    """`run(noise) -> (xs, hist, ..)`; `tols`: the list of `Noise`, to share
    between runs with the same preconditioner inputs (the three `reorth` of
    one case).  Returns `(clean, tol_x, tol_h)`:
    `tol_x[k] = (velocity, pressure)`,

        32 max over the seeds ||x_k(noisy) - x_k||_inf,block,
        nowhere below 16u ||x_k||_inf,block

    and `tol_h` the same for the entries of the history"""
    clean = run(None)
    xs, hist = clean[0], clean[1]
    NV = prob.NV
    dx = np.zeros((len(xs), 2), dtype=LD)
    dh = np.zeros(len(hist), dtype=LD)
    tols = [] if tols is None else tols
    for seed in seeds:
        out = run(Noise(prob, seed, tols))
        d = np.abs(out[0] - xs)
        dx = np.maximum(dx, np.stack([d[:, :NV].max(axis=1),
                                      d[:, NV:].max(axis=1)], axis=1))
        dh = np.maximum(dh, np.abs(out[1] - hist))
    ax = np.abs(xs)
    floor = 16*U64*np.stack([ax[:, :NV].max(axis=1), ax[:, NV:].max(axis=1)],
                            axis=1)
    tol_x = np.maximum(FACTOR*dx, floor).astype(np.float64)
    tol_h = np.maximum(FACTOR*dh, 16*U64*np.abs(hist)).astype(np.float64)
    return clean, tol_x, tol_h


def block_norms(xs, NV):
    """`||x_k||_inf` per block, one row per `k`"""
    ax = np.abs(np.asarray(xs))
    return np.stack([ax[:, :NV].max(axis=1), ax[:, NV:].max(axis=1)],
                    axis=1).astype(np.float64)


# ---- the cases of tests/test_gpu_krylov_steps.py ---------------------------------
FORMS = {
    'J2': pm.form_of(schur='jacobi', fhat='cheb', degree=2),
    'D4': pm.form_of(fact='full'),
    'D4f': pm.form_of(fact='full', fp32=1),
    'MG': pm.form_of(schur='mg', fact='full'),
}
REGIMES = {'latency': dict(streaming=0, pair=0),
           'streamed': dict(streaming=1, pair=0),
           'pair': dict(streaming=1, pair=1)}
REORTHS = (0, 1, 2)
LONG = (12,)                # legs 1, 2, 4: x_1 .. x_12 of ONE cycle
RESTARTED = (5, 5, 3)       # leg 3
STAG_COLS = 40


def toy_bench(toy_prob):
    from dolfin_navier_scipy_amd import amg
    M, A, J = (toy_prob['smc'][k] for k in 'MAJ')
    F = (M + .5*5e-3*A).tocsr()
    b = pm.Bench(M, F, J, amg.algebraic_prolongations(F, J, coarsest=40))
    assert (b.NV, b.NP) == (1286, 207)
    assert pm.mg_sizes(b.J, b.prols) == [207, 47, 11]
    return b


def right_hand_sides(bench):
    """`Bench.rs[0]` and a rough one"""
    rough = np.random.default_rng(11).standard_normal(bench.NV + bench.NP)
    return {'time-step': bench.rs[0], 'rough': rough}


def starts(bench):
    return {'zero': None,
            'rough': np.random.default_rng(12).standard_normal(
                bench.NV + bench.NP)}


# (right-hand side, start): both right-hand sides from zero, the first one
# from a rough start as well
CASES = (('time-step', 'zero'), ('time-step', 'rough'), ('rough', 'zero'))
LEG1_K = (1, 2, 3, 5, 9, 12)
LEG2_K = (1, 4, 9)
LEG4_K = (2, 6)
LEG3_FORMS = ('J2', 'D4', 'D4f', 'MG')
BICG_FORMS = ('J2', 'D4')
BICG_K = {'zero': 3, 'rough': 2}
X_COND = 1e-10      # tol_x <= X_COND ||x_k||_inf,block, else "not a test"
# leg 4: the GPU test holds every history entry to ONE tolerance of the
# model's, so a stop more than one tolerance below h_0 .. h_k and above
# h_{k+1} fixes which column stops; four leaves a margin for the stop's own
# rounding (`rtol ||b||` with the device's `||b||`)
SEPARATION = 4
GOLDEN = 'krylov_steps_tol.npz'


def gmres_key(form, rhs, start, reorth, cycles):
    return 'gmres/%s/%s/%s/r%d/%s' % (form, rhs, start, reorth,
                                      '+'.join(str(c) for c in cycles))


def bicg_key(form, rhs, start):
    return 'bicg/%s/%s/%s' % (form, rhs, start)


def pack(tab, key, clean, tol_x, tol_h, NV):
    tab[key + '/tx'] = tol_x
    tab[key + '/th'] = tol_h
    tab[key + '/nx'] = block_norms(clean[0], NV)
    tab[key + '/h'] = np.asarray(clean[1], dtype=np.float64)


def listed(tab, key, k):
    """is `x_k` of the run `key` a test: `X_COND` on both blocks, the one
    reason to drop a case (a NaN -- a noisy run whose basis gave out before
    column `k` -- fails it)"""
    tx, nx = tab[key + '/tx'], tab[key + '/nx']
    with np.errstate(invalid='ignore'):
        return bool(np.all(tx[k - 1] <= X_COND*nx[k - 1]))


def stop_between(tab, key, k):
    """leg 4: `sqrt(h_k h_{k+1})`, or None unless it lies `SEPARATION`
    tolerances below every entry up to `h_k` and above `h_{k+1}` (a NaN
    tolerance separates nothing)"""
    h, th = tab[key + '/h'], tab[key + '/th']
    stop = np.sqrt(h[k]*h[k + 1])
    with np.errstate(invalid='ignore'):
        ok = np.all(h[:k + 1] - stop >= SEPARATION*th[:k + 1]) and \
            stop - h[k + 1] >= SEPARATION*th[k + 1]
    return float(stop) if ok else None


def leg4_runs(tab, form):
    """the `(reorth, rhs, start, k)` of leg 4 on `form`"""
    return [(r, rhs, start, k) for r in REORTHS for rhs, start in CASES
            for k in LEG4_K
            if stop_between(tab, gmres_key(form, rhs, start, r, LONG), k)
            is not None]


# what `leg4_runs` comes to on the golden file, spelled out (the CPU test
# holds the file to it, the GPU test what ran): all but these
LEG4_NOT_RUN = {
    'J2': [],
    # (fused Gram-Schmidt behind the dense block: NaN tolerances by h_6)
    'D4': [(2, 'time-step', 'zero', 6), (2, 'time-step', 'rough', 6),
           (2, 'rough', 'zero', 6)],
    'MG': [],
}
LEG4_NOT_RUN['D4f'] = LEG4_NOT_RUN['D4']


def gmres_runs(form, cases=CASES, leg3=LEG3_FORMS):
    for rhs, start in cases:
        for cycles in (LONG, RESTARTED):
            if cycles == LONG or form in leg3:
                yield rhs, start, cycles


def clean_table(bench):
    """`/h` and `/nx` of every run (no noise: longdouble arithmetic alone)"""
    tab = {}
    rhs_of, start_of = right_hand_sides(bench), starts(bench)
    for form in FORMS:
        prob = Problem(bench, FORMS[form])
        for rhs, start, cycles in gmres_runs(form):
            for reorth in REORTHS:
                out = gmres_cycles(prob, rhs_of[rhs], start_of[start], cycles,
                                   reorth)
                key = gmres_key(form, rhs, start, reorth, cycles)
                tab[key + '/nx'] = block_norms(out[0], prob.NV)
                tab[key + '/h'] = np.asarray(out[1], dtype=np.float64)
        if form in BICG_FORMS:
            for rhs in rhs_of:
                for start, k in BICG_K.items():
                    out = bicgstab_steps(prob, rhs_of[rhs], start_of[start], k)
                    key = bicg_key(form, rhs, start)
                    tab[key + '/nx'] = block_norms(out[0], prob.NV)
                    tab[key + '/h'] = np.asarray(out[1], dtype=np.float64)
    return tab


def tolerance_table(bench, forms=None, stagnation=True, log=None,
                    cases=CASES, leg3=LEG3_FORMS):
    """every tolerance of tests/test_gpu_krylov_steps.py as a dict of arrays
    (what `tests/golden/krylov_steps_tol.npz` holds)"""
    tab = {}
    rhs_of, start_of = right_hand_sides(bench), starts(bench)
    for form in (FORMS if forms is None else forms):
        prob = Problem(bench, FORMS[form])
        for rhs, start, cycles in gmres_runs(form, cases, leg3):
            tols = []
            for reorth in REORTHS:
                def run(nz):
                    return gmres_cycles(prob, rhs_of[rhs], start_of[start],
                                        cycles, reorth, nz)
                key = gmres_key(form, rhs, start, reorth, cycles)
                pack(tab, key, *tolerances(run, prob, tols=tols), prob.NV)
                if log:
                    log(key)
        if form in BICG_FORMS:
            for rhs in rhs_of:
                for start, k in BICG_K.items():
                    def run(nz):
                        return bicgstab_steps(prob, rhs_of[rhs],
                                              start_of[start], k, nz)
                    pack(tab, bicg_key(form, rhs, start),
                         *tolerances(run, prob), prob.NV)
        if form == 'D4' and stagnation:
            tab['stagnation'] = stagnation_floor(prob, rhs_of['time-step'])
    return tab


def stagnation_floor(prob, b):
    """`[noisy, clean, rounded, ||b||]`: the smallest true residual norm in
    `STAG_COLS` columns of one fused cycle (`reorth = 2`) from zero -- of the
    model with the noise hook (the largest of the eight seeds: what fp64
    arithmetic can be held to), of the model without it (longdouble rounding
    level, out of reach for a vector of doubles), and of the latter's
    iterates rounded to fp64.  A run ends where `hn^2 <= 0`."""
    def best(res):
        res = np.asarray(res, dtype=np.float64)
        return float(np.nanmin(res))
    xs, _, res = gmres_cycles(prob, b, None, (STAG_COLS,), 2)
    rounded = [float(norm_ld(np.asarray(b, dtype=LD) - prob.mv(
        x.astype(np.float64).astype(LD)))) for x in xs
        if np.isfinite(x[0])]
    tols, noisy = [], 0.
    for seed in SEEDS:
        noisy = max(noisy, best(gmres_cycles(
            prob, b, None, (STAG_COLS,), 2, Noise(prob, seed, tols))[2]))
    return np.array([noisy, best(res), min(rounded), float(norm_ld(b))])


# ---- the runs tests/test_gpu_zz_dist_krylov.py adds -------------------------------
# (a second golden file; `FORMS` and `GOLDEN` above stay what they are)
DIST_FORMS = {
    # dense Schur, explicit degree 4, TRIANGULAR: no `J Fh^-1`, the Schur block
    # of a row-partitioned head reads the pressure part itself
    'D4t': pm.form_of(),
}
ALL_FORMS = dict(FORMS, **DIST_FORMS)
# `cycle_first = 1`, `restart = 5`, `maxiter = 6`: the one-step cycle (lazy or
# general: column 1 of GMRES either way), then `min(m, max(2 c, 8)) = 5`
LAZY = (1, 5)
LAZY_FORMS = ('D4', 'D4f', 'D4t', 'MG')
GOLDEN_DIST = 'krylov_dist_tol.npz'


def dist_runs(cases=CASES, lazy_cases=CASES, leg3=True):
    """`(form, rhs, start, cycles, reorths)` of the second golden file: the
    `LONG` and `RESTARTED` runs of `DIST_FORMS`, the `LAZY` runs (`reorth = 2`
    alone: nothing else takes the one-step cycle) of `LAZY_FORMS`"""
    for form in DIST_FORMS:
        for rhs, start in cases:
            for cycles in (LONG, RESTARTED) if leg3 else (LONG,):
                yield form, rhs, start, cycles, REORTHS
    for form in LAZY_FORMS:
        for rhs, start in lazy_cases:
            yield form, rhs, start, LAZY, (2,)


def dist_clean_table(bench):
    """`/h` and `/nx` of every run of `dist_runs()`"""
    tab, probs = {}, {}
    rhs_of, start_of = right_hand_sides(bench), starts(bench)
    for form, rhs, start, cycles, reorths in dist_runs():
        if form not in probs:
            probs[form] = Problem(bench, ALL_FORMS[form])
        for reorth in reorths:
            out = gmres_cycles(probs[form], rhs_of[rhs], start_of[start],
                               cycles, reorth)
            key = gmres_key(form, rhs, start, reorth, cycles)
            tab[key + '/nx'] = block_norms(out[0], bench.NV)
            tab[key + '/h'] = np.asarray(out[1], dtype=np.float64)
    return tab


def dist_tolerance_table(bench, runs=None, log=None):
    """every tolerance `tests/golden/krylov_dist_tol.npz` holds, by the recipe
    of `tolerance_table` (`tolerances()`)"""
    tab, probs = {}, {}
    rhs_of, start_of = right_hand_sides(bench), starts(bench)
    for form, rhs, start, cycles, reorths in (dist_runs() if runs is None
                                              else runs):
        if form not in probs:
            probs[form] = Problem(bench, ALL_FORMS[form])
        prob, tols = probs[form], []
        for reorth in reorths:
            def run(nz):
                return gmres_cycles(prob, rhs_of[rhs], start_of[start], cycles,
                                    reorth, nz)
            key = gmres_key(form, rhs, start, reorth, cycles)
            pack(tab, key, *tolerances(run, prob, tols=tols), prob.NV)
            if log:
                log(key)
    return tab
