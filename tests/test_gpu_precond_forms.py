"""Every form of the preconditioner apply against the fp64 model of
`tests/precond_model.py`, at the tolerance `tests/test_precond_model_cpu.py`
fixes from the model alone:

    16 max(rho_ref, 1) (2^-53 ||a||_inf + 2^-24 ||a_half||_inf)    per block

Entry A, `apply_precond(r)`: three right-hand sides (random, `r_p = 0`,
`r_v = 0`), and a second call on the same handle must return the same bits.

Entry B, the path a GMRES cycle takes (`k_arn_head`, `k_tau_guard`, the guarded
multigrid cycle, the streamed `J Fh^-1`): ONE column from `x0 = 0`.  With
`z = P^-1 b`, `w = K z` the iterate is `x1 = alpha z`, `alpha = (w.b)/(w.w)`.
The device's `z` is within the tolerance `t` (a vector: `t_v` on the velocity
entries, `t_p` on the pressure entries, plus the entry-wise slack of
`Bench.form`) of the model's, so its `w` within `|K| t`, and its two dots are sums of `n` products in fp64 in an order of its
own (error at most `16 u` times the sum of the moduli, the same allowance as
everywhere here).  To first order

    |d alpha| <= [ |b|.(|K| t) + 16u |w|.|b|
                   + |alpha| (2 |w|.(|K| t) + 16u |w|.|w|) ] / (w.w)
    |x1 - alpha z|_block <= |alpha| t_block + |d alpha| ||z_block||_inf .

`F` is symmetric throughout (the polynomial of the symmetric part of a
convection-dominated `F` is not modelled), one GPU, whole matrices.  Every test
prints its largest `error / tolerance` (run with `-s`).
"""
import numpy as np
import pytest

import krylov_model as km
import precond_model as pm

pytestmark = pytest.mark.gpu

BIG = float(2**40)      # a threshold no operator here reaches: latency regime


@pytest.fixture(scope='module')
def sad():
    from dolfin_navier_scipy_amd import saddle, _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    return saddle


@pytest.fixture(scope='module')
def toy(toy_prob):
    from dolfin_navier_scipy_amd import amg
    M, A, J = (toy_prob['smc'][k] for k in 'MAJ')
    F = (M + .5*5e-3*A).tocsr()
    b = pm.Bench(M, F, J, amg.algebraic_prolongations(F, J, coarsest=40))
    assert pm.mg_sizes(b.J, b.prols) == [207, 47, 11]
    return b


def _cylinder(N, coarsest):
    from dolfin_navier_scipy_amd import amg
    from dolfin_navier_scipy_amd.fem import get_sysmats
    _, sm, _ = get_sysmats(problem='cylinderwake', N=N, Re=100)
    F = (sm['M'] + sm['A']/1024.).tocsr()           # dt = 1/512
    prols = [] if coarsest is None else \
        amg.algebraic_prolongations(F, sm['J'], coarsest=coarsest)
    return pm.Bench(sm['M'], F, sm['J'], prols)


@pytest.fixture(scope='module')
def wake():
    w = pm.Wake()
    assert pm.mg_sizes(w.mg.J, w.mg.prols) == [1289, 296, 66]
    assert w.mg.NV == 9356
    return w


def make_system(sad, b, f):
    """a handle with every knob of the form pinned, set up"""
    system = sad.SaddleSystem(b.F, b.J)
    thr = 1. if f['streaming'] else BIG
    system.set_option('stream_nnz', thr).set_option('mg_stream_nnz', thr)
    system.set_option('pair', f['pair'])
    if f['schur'] == 'mg':
        system.set_schur_mg(b.prols, smooth_steps=f['nu'])
        for k in ('dense_max', 'dense_half_max', 'fused', 'cheb', 'cycles'):
            system.set_option('mg_' + k, f[k.replace('dense_half', 'half')])
    system.setup_precond(cheb_degree=f['degree'], schur=f['schur'],
                         fhat=f['fhat'], fp32_store=bool(f['fp32']),
                         drop_tol=f['drop'], factorization=f['fact'])
    return system


def check_info(system, f, m):
    """the form that was asked for is the form that runs -- as far as
    `precond_info()` tells: it reports neither whether the fused operators
    nor whether the streaming kernels ran.  The fp32 x streaming forms are
    tied to their path by what is rounded; an fp64 form that fell back to the
    sub-wave or the plain kernels would compute the same map and pass"""
    info = system.precond_info()
    assert info['schur'] == f['schur'] and info['cheb_degree'] == f['degree']
    assert info['fp32_store'] == bool(f['fp32'])
    assert (info['nnz_Gc'] > 0) == (f['fhat'] == 'explicit')
    assert (info['nnz_JG'] > 0) == (f['fact'] == 'full')
    if not f['pair']:
        assert info['pair_format_bytes'] == 0
    if f['schur'] != 'mg':
        assert info['mg_levels'] == []
        return
    assert [lv['n'] for lv in info['mg_levels']] == m.mg.sizes
    assert info['mg_nu'] == f['nu']
    assert info['mg_coarse_val_bytes'] == \
        {'f64': 8, 'f32': 4, 'f16': 2}[m.store['cinv']]
    # two cycles in every application iff the option says 2 (and then only
    # on the fused V(2,2): `precond_model.device_cycle`)
    assert (info['mg_cycles'] >= 2 and info['mg_two_cycle_maxc'] >= 1000) == \
        (f['cycles'] == 2)


def run_entry_a(sad, b, f, rho=None):
    system = make_system(sad, b, f)
    try:
        detail = []
        ex, done = b.apply_excess(system, f, rho, detail)
        check_info(system, f, done[0])
    finally:
        system.close()
    print('apply  %-52s error / tolerance %.3f  (rho_ref %.1f %.1f) %s'
          % (pm.form_id(f), ex, *pm.rho_max(done[2]), detail))
    assert ex <= 1.0


def one_column(b, done, r):
    """`(x1, tolerance per block)` of the model (module docstring)"""
    m, tols, slacks = done[0], done[3], done[4]
    K = km.saddle(b.F, b.J).tocsr()
    aK = abs(K)
    i = [k for k, q in enumerate(b.rs) if q is r][0]
    z = m.apply(r)
    w = K @ z
    ww = w @ w
    alpha = (w @ r)/ww
    # (entry by entry: the slack of an fp32 inverse sits on a few entries)
    t = np.concatenate([np.full(b.NV, tols[i][0]),
                        np.full(b.NP, tols[i][1])]) + slacks[i]
    Kt = aK @ t
    u16 = 16*pm.U64
    dalpha = (np.abs(r) @ Kt + u16*(np.abs(w) @ np.abs(r)) +
              abs(alpha)*(2*(np.abs(w) @ Kt) + u16*ww))/ww
    tol = [abs(alpha)*pm.blocks(t, b.NV)[k] +
           dalpha*np.abs(pm.blocks(z, b.NV)[k]).max() for k in (0, 1)]
    return alpha*z, tol


def run_entry_b(sad, b, f, rho=None):
    system = make_system(sad, b, f)
    worst = 0.
    try:
        lo, hi = system.cheb_bounds()
        done = b.form(f, lo, hi, entry='gmres', rho=rho)
        for r in b.rs[:2]:
            x1, tol = one_column(b, done, r)
            for reorth in (1, 2):
                for graph in (False, True):
                    x = system.solve(r[:b.NV], r[b.NV:], x0=None, maxiter=1,
                                     restart=1, rtol=1e-300, reorth=reorth,
                                     use_graph=graph, raise_on_fail=False)
                    assert system.last_stats['iters'] == 1
                    for k in (0, 1):
                        d = np.abs(pm.blocks(x - x1, b.NV)[k])
                        ok = tol[k] > 0.    # (else zero by construction)
                        assert not d[~ok].any()
                        if ok.any():
                            worst = max(worst, float((d[ok]/tol[k][ok]).max()))
    finally:
        system.close()
    print('gmres  %-52s error / tolerance %.3f' % (pm.form_id(f), worst))
    assert worst <= 1.0


@pytest.mark.parametrize('f', pm.TOY_FORMS, ids=pm.form_id)
def test_apply_precond_matches_the_model(sad, toy, f):
    run_entry_a(sad, toy, f)


@pytest.mark.parametrize('f', pm.TOY_FORMS, ids=pm.form_id)
def test_one_gmres_column_matches_the_model(sad, toy, f):
    run_entry_b(sad, toy, f)


@pytest.mark.parametrize('f', pm.WAKE_FORMS, ids=pm.form_id)
def test_apply_precond_on_the_wake(sad, wake, f):
    """dense rows of more than 256 columns in fp32 and in fp64 (1289, and the
    296-row coarsest level of `dense_max=300`), `sld = 1292 != 1289`, row
    lengths across the lanes-per-row instantiations"""
    run_entry_a(sad, wake.bench(f), f, rho=pm.WAKE_RHO[pm.form_id(f)])


@pytest.mark.parametrize('f', pm.WAKE_FORMS[:3], ids=pm.form_id)
def test_one_gmres_column_on_the_wake(sad, wake, f):
    run_entry_b(sad, wake.bench(f), f, rho=pm.WAKE_RHO[pm.form_id(f)])


def test_half_level_beyond_the_unrolled_loop(sad):
    """`k_gemv_half`'s four-loads loop runs only past 1536 rows: the smallest
    pressure space of the meshes beyond that, N = 3 (NP 2592, `ldh / 8 = 324`
    packets a row: every lane takes the four-loads pass once, the remainder
    pass at packet `256 + lane`, and lanes 0..3 a second one at `320 + lane`
    too), as ONE dense level in half precision.  390 of its 6.7e6 entries
    are ties of two halves once rounded to fp32 (`precond_model.half_rows`):
    those, and only those, may come out one half-precision step apart"""
    b = _cylinder(3, None)
    assert b.NP == 2592
    f = pm.form_of(schur='mg', fhat='cheb', half_max=4096)
    run_entry_a(sad, b, f, rho=pm.HALF_RHO)
