"""The fp64 model of the preconditioner apply (`tests/precond_model.py`) checked
against itself: no GPU, no library.  It fixes the yardstick the GPU parity
tests (`tests/test_gpu_precond_forms.py`) assert with.

* the explicit polynomial `G` is the Chebyshev vector recurrence, and the drop
  rule is `host_cheb_poly`'s;
* the plain V-cycle is the cycle on the fused operators of `mg_fused22_ops` /
  `mg_fused11_ops`, and swapping `omega` and `omega2` changes nothing;
* `rho_ref = ||z64 - z_ld||_inf / (2^-53 ||a||_inf)` per block and form, `z_ld`
  the same model in `np.longdouble` on dense arrays, `a` the yardstick of
  `Precond.yardsticks`;
* the GPU tolerance `16 max(rho_ref, 1) (2^-53 ||a|| + 2^-24 ||a_half||)` stays
  below `1e-11 ||z||` per block for every form that sums in fp64;
* every mutation the GPU tests are there to catch leaves that tolerance by a
  factor of at least 100.

`rho_ref` on the toy problem (NV 1286, NP 207, levels 207 / 47 / 11), the
largest of the three right-hand sides (each has its own in the tolerance), velocity / pressure block; `tol/|z|` the
largest tolerance relative to its block (printed by `test_rho_ref_table`, run
with `-s`):

    form                                               rho_v  rho_p  tol/|z|
    dense-tri-cheb-d1                                    1.0   38.6   8e-13
    dense-tri-cheb-d4-fp321                              0.1    0.8   2e-12
    dense-tri-expl-d1                                    1.6   37.9   8e-13
    dense-ful-expl-d6-fp321-drop0.001                    0.3    0.7   1e-12
    jacobi-tri-expl-d4                                   4.4    1.2   2e-14
    jacobi-ful-expl-d4-fp321-drop0.001                   2.4    4.8   1e-14
    dense-ful-expl-d4-streaming1                         0.5    4.8   6e-12
    dense-ful-expl-d4-fp321-streaming1-pair0             0.3    0.8   1e-12
    mg-ful-expl-d4-fused0                                0.6    0.8   1e-12
    mg-tri-expl-d4-fp321-nu1-fused0-cheb0                3.6    0.3   5e-13
    mg-ful-expl-d4                                       0.5    0.3   1e-12
    mg-tri-expl-d6-fp321-drop0.001-cheb0-cycles2         2.3    0.1   4e-12
    mg-ful-expl-d4-nu1                                   0.7    1.0   1e-12
    mg-tri-expl-d4-fused0-streaming1                     4.5    0.8   9e-13
    mg-ful-expl-d4-fp321-streaming1                      0.6    0.2   1e-12
    mg-tri-expl-d4-fp321-nu1-streaming1-pair0            3.0    0.4   2e-13
    mg-ful-expl-d4-cycles2-streaming1                    0.2    0.1   3e-12
    mg-tri-cheb-d4-cycles0                               0.1    0.7   8e-13
    mg-ful-expl-d4-half_max64       (fp32 sums)          0.6    0.1   2e-05
    mg-tri-expl-d4-fp321-fused0-half_max64  (fp32 sums)  3.2    0.1   7e-05

(`rho_ref` above one: the Gauss-Jordan inverse of `S0`, condition 2e3 to 4e3,
formed as the device forms it -- `precond_model.inv_gj`.)  The chain of moduli
of the issue (`apply_abs_chain`) is `a` itself for the dense and Jacobi blocks; through a
multigrid cycle it is 20 to 7e3 times `a`, through two cycles 1e8 to 1e11
times, which would put the tolerance at 1e-7 to 1e-1 of `|z|`: `a` takes the
true linear map behind every stage instead of the product of moduli.  It is
never larger (asserted below), so the tolerance never wider.
"""
import numpy as np
import pytest

import krylov_model as km
import precond_model as pm


@pytest.fixture(scope='module')
def toy(toy_prob):
    from dolfin_navier_scipy_amd import amg
    M, A, J = (toy_prob['smc'][k] for k in 'MAJ')
    F = (M + .5*5e-3*A).tocsr()
    b = pm.Bench(M, F, J, amg.algebraic_prolongations(F, J, coarsest=40))
    assert pm.mg_sizes(b.J, b.prols) == [207, 47, 11]
    return b


# ---- the model against itself ----------------------------------------------------
@pytest.mark.parametrize('degree', [1, 2, 4, 6])
def test_explicit_poly_is_the_vector_recurrence(toy, degree):
    """`G b` and the recurrence are two fp64 evaluations of one polynomial:
    they differ by the rounding of either, bounded by the modulus of the
    recurrence (every term added)"""
    m = toy.model(pm.form_of(degree=degree))
    for r in toy.rs[:2]:
        b = r[:toy.NV]
        bound = 16*pm.U64*m._fhat_abs(np.abs(b)).max()
        err = np.abs(m.G @ b - m.cheb.apply(b)).max()
        print('degree %d: |G b - recurrence| = %.1e (bound %.1e, |G b| %.1e)'
              % (degree, err, bound, np.abs(m.G @ b).max()))
        assert err <= bound
        assert bound <= 1e-11*np.abs(m.G @ b).max()    # (and says something)


def test_explicit_poly_on_the_cylinder_wake():
    from dolfin_navier_scipy_amd.fem import get_sysmats
    _, sm, _ = get_sysmats(problem='cylinderwake', N=2, Re=100)
    F = (sm['M'] + sm['A']/1024.).tocsr()
    lo, hi = km.power_bounds(F, 1/F.diagonal())
    cheb = km.ChebJacobi(F, degree=4, lmin=.9*lo, lmax=1.05*hi)
    G = pm.explicit_poly(F, cheb.lmin, cheb.lmax, 4)
    b = sm['M'] @ np.random.default_rng(0).standard_normal(F.shape[0])
    err = np.abs(G @ b - cheb.apply(b)).max()/np.abs(G @ b).max()
    print('N=2 wake, degree 4: |G b - recurrence| / |G b| = %.1e' % err)
    assert err <= 64*pm.U64


def test_drop_rule_is_host_cheb_polys(toy):
    """dropped once, at the end: what stays is the undropped entry, what goes
    is below `tol` times its row's largest modulus, the diagonal stays"""
    G0 = pm.explicit_poly(toy.F, toy.lo, toy.hi, 6).tocsr()
    tol = 1e-3
    G = pm.explicit_poly(toy.F, toy.lo, toy.hi, 6, tol).tocsr()
    assert toy.NV < G.nnz < 0.5*G0.nnz
    D0, D = G0.toarray(), G.toarray()
    kept = D != 0
    assert (D[kept] == D0[kept]).all()
    thr = tol*np.abs(D0).max(axis=1)[:, None]
    gone = (~kept) & (D0 != 0)
    assert (np.abs(D0) < thr)[gone].all()
    assert not ((np.abs(D0) >= thr) & ~kept).any()
    assert (np.diag(D) == np.diag(D0)).all() and np.diag(D).all()
    # ... and with it G is no longer symmetric, so neither is S0 = J G J^T
    S0 = (toy.J @ G @ toy.J.T).toarray()
    assert np.abs(S0 - S0.T).max() > 1e-6*np.abs(S0).max()


@pytest.mark.parametrize('cycle,kw', [
    ('fused22', dict(fact='full')), ('fused22', dict(cheb=0)),
    ('fused22', dict(cycles=2, fact='full')), ('fused11', dict(nu=1))])
def test_plain_cycle_is_the_fused_cycle(toy, cycle, kw):
    """`Apre / Rr / Qq` of `mg_fused22_ops`, `mg_fused11_ops` transcribed: the
    same map as the plain V(nu, nu), to the tolerance of the GPU tests"""
    f = pm.form_of(schur='mg', **kw)
    m, rho = toy.form(f)[0], pm.rho_max(toy.form(f)[2])
    assert m.mg.cycle == 'plain'
    assert pm.device_cycle(f['nu'], 1, f['cycles'], 3)[0] == cycle
    mg = dict(nu=f['nu'], dense_max=20, cheb=bool(f['cheb']),
              cycles=f['cycles'], cycle=cycle)
    fused = toy.model(f, mg=mg)
    assert fused.mg.cycle == cycle and fused.mg.two == (f['cycles'] == 2)
    ex = toy.excess(toy.form(f), [fused.apply(r) for r in toy.rs])
    print('%s vs plain: %.2f of the tolerance (rho_ref %.1f, %.1f)'
          % (cycle, ex, rho[0], rho[1]))
    assert ex <= 1.0


def test_the_two_sweeps_commute(toy):
    f = pm.form_of(schur='mg', fact='full', fused=0)
    other = toy.model(f)
    for lv in other.mg.levels[:-1]:
        assert lv.omega2 > 1.5*lv.omega
        lv.omega, lv.omega2 = lv.omega2, lv.omega
    ex = toy.excess(toy.form(f), [other.apply(r) for r in toy.rs])
    print('omega <-> omega2: %.2f of the tolerance' % ex)
    assert ex <= 1.0


# ---- the yardstick --------------------------------------------------------------
@pytest.mark.parametrize('f', pm.TOY_FORMS, ids=pm.form_id)
def test_rho_ref_table(toy, f):
    m, yard, rhos, tols, slacks = toy.form(f)
    rho = pm.rho_max(rhos)
    # (only the fp32 copy of a computed inverse is ambiguous, on few entries)
    if m.store['sinv'] != 'f32':
        assert not any(sl.any() for sl in slacks)
    else:
        print('entries of sinv32 on an fp32 rounding boundary: %d'
              % m.sinv_slack.nnz)
        assert m.sinv_slack.nnz == 0
    half = m.schur == 'mg' and m.mg.half
    worst = 0.
    for r, (a, ah), tol in zip(toy.rs, yard, tols):
        z = m.apply(r)
        chain = m.apply_abs_chain(r)
        assert (a >= np.abs(z)*(1 - 1e-12)).all()
        assert (a <= chain*(1 + 1e-12)).all()
        # (nothing passes a half-precision level unless there is one; with
        # one, everything that reaches the Schur block does)
        assert ah.any() == (half and bool(np.abs(z[toy.NV:]).max() > 0.))
        for k in (0, 1):
            zk = np.abs(pm.blocks(z, toy.NV)[k]).max()
            if zk > 0.:
                worst = max(worst, tol[k]/zk)
    print('%-50s rho_ref %5.1f %5.1f   tol/|z| %.0e'
          % (pm.form_id(f), rho[0], rho[1], worst))
    assert np.isfinite(rho).all()
    if not half:
        # (a wider tolerance than this means a badly scaled input)
        assert worst < 1e-11


# ---- what the GPU tests must be able to see ----------------------------------------
MG = dict(schur='mg', fact='full')


def _mutants(toy):
    """`(name, form, mutated model)`"""
    out = []
    for l in (0, 1):
        f = pm.form_of(**MG)
        mut = toy.model(f)
        mut.mg.levels[l].omega2 *= 1.01
        out.append(('omega2 of level %d off by 1 %%' % l, f, mut))
    f = pm.form_of(**MG)
    mut = toy.model(f)
    mut.mg.cinv = mut.mg.cinv.copy()
    mut.mg.cinv[-1, :] = 0.
    out.append(('last row of the coarsest inverse zeroed', f, mut))
    for l in (0, 1):
        mut = toy.model(f)
        P = mut.mg.levels[l].P.copy()
        i = P.shape[0]//2
        assert P.indptr[i + 1] - P.indptr[i] >= 2
        P.data[P.indptr[i + 1] - 1] = 0.
        mut.mg.levels[l].P = P
        out.append(('last entry of a row of P_%d dropped' % l, f, mut))
    # one operator in the other precision
    for name, fkw, op, kind in (
            ('Gc in fp32, the map says fp64', dict(fact='full'), 'Gc', 'f32'),
            ('sinv in fp32, the map says fp64', dict(fact='full'), 'sinv', 'f32'),
            ('JG in fp32, the map says fp64', dict(fact='full'), 'JG', 'f32'),
            ('Gc in fp64, the map says fp32', dict(fact='full', fp32=1), 'Gc', 'f64'),
            ('sinv in fp64, the map says fp32', dict(fact='full', fp32=1), 'sinv', 'f64'),
            ('cinv in fp32, the map says fp64', dict(**MG), 'cinv', 'f32'),
            ('cinv in fp64, the map says fp32', dict(fp32=1, **MG), 'cinv', 'f64'),
            ('Qq in fp64, the map says fp32',
             dict(fp32=1, streaming=1, **MG), 'Qq', 'f64'),
            ('Rr in fp32, the map says fp64', dict(streaming=1, **MG), 'Rr', 'f32')):
        f = pm.form_of(**fkw)
        base = toy.form(f)[0]
        store = dict(base.store)
        assert store[op] != kind
        store[op] = kind
        kw = dict(store=store)
        if op in ('Qq', 'Rr'):
            kw['mg'] = dict(nu=2, dense_max=20, cheb=True, cycles=1,
                            cycle='fused22')
        out.append((name, f, toy.model(f, **kw)))
    # the padding column of sinv32 read as data: rows of sld = 208 floats
    # read with the stride 207
    f = pm.form_of(fact='full', fp32=1)
    mut = toy.model(f)
    NP = toy.NP
    sld = (NP + 3) & ~3
    assert sld != NP
    pad = np.zeros((NP, sld))
    pad[:, :NP] = mut.sinv
    mut.sinv = pad.reshape(-1)[:NP*NP].reshape((NP, NP))
    out.append(('padding of sinv32 read as data', f, mut))
    for fkw in (dict(fact='full', drop=1e-3, degree=6),
                dict(drop=1e-3, degree=6, **MG)):
        f = pm.form_of(**fkw)
        out.append(('S0 symmetrised (%s, drop_tol 1e-3)' % f['schur'], f,
                    toy.model(f, symmetrise=True)))
    f = pm.form_of(cycles=2, **MG)
    assert toy.form(f)[0].mg.two
    out.append(('one cycle where two are asked for', f,
                toy.model(f, mg=dict(nu=2, dense_max=20, cheb=True, cycles=1))))
    return out


def test_mutations_leave_the_tolerance(toy):
    fails = []
    for name, f, mut in _mutants(toy):
        ex = toy.excess(toy.form(f), [mut.apply(r) for r in toy.rs])
        print('%-45s %9.2e x the tolerance  (%s)' % (name, ex, pm.form_id(f)))
        if not ex >= 100.:
            fails.append((name, ex))
    assert not fails, fails


# ---- the larger fixtures of the GPU tests ------------------------------------------
@pytest.fixture(scope='module')
def wake():
    return pm.Wake()


@pytest.mark.parametrize('f', pm.WAKE_FORMS, ids=pm.form_id)
def test_wake_tolerances(wake, f):
    """the condition of the toy forms on the wake, with the recorded
    `rho_ref` (`WAKE_RHO`), and how much the entry-wise slack of the fp32
    inverse adds: 18 of the 1.66e6 entries of the store are ambiguous; they
    reach 18 pressure entries of `z` and the 2.8e3 velocity entries the rows
    of `G J^T` spread them to.  Every other entry keeps the tolerance alone"""
    wake = wake.bench(f)
    m, yard, rho, tols, slacks = wake.form(f, rho=pm.WAKE_RHO[pm.form_id(f)])
    worst, over = 0., 0
    for r, tol, sl in zip(wake.rs, tols, slacks):
        z = m.apply(r)
        for k in (0, 1):
            zk = np.abs(pm.blocks(z, wake.NV)[k]).max()
            if zk > 0.:
                worst = max(worst, tol[k]/zk)
            over = max(over, int((pm.blocks(sl, wake.NV)[k] > tol[k]).sum()))
    amb = m.sinv_slack.nnz if getattr(m, 'sinv_slack', None) is not None else 0
    print('%-55s tol/|z| %.1e  ambiguous fp32 entries %d, entries of z whose '
          'slack exceeds the tolerance: %d' % (pm.form_id(f), worst, amb, over))
    assert worst < 1e-11
    if m.store['sinv'] != 'f32':
        assert amb == 0 and over == 0
    else:
        # (of 1289^2 entries; each reaches its pressure entry and the ~160
        # velocity entries its column of G J^T touches)
        assert amb <= 32 and over <= 32*200
        assert max(int((sl[wake.NV:] > 0).sum()) for sl in slacks) <= amb


def test_wake_sinv32_padding_mutation(wake):
    """rows of `sld = 1292` floats read with the stride 1289: seen through the
    tolerance of the wake's fp32 form, its slack included"""
    f = pm.WAKE_FORMS[0]
    assert f['fp32'] and f['schur'] == 'dense'
    wake = wake.bench(f)
    done = wake.form(f, rho=pm.WAKE_RHO[pm.form_id(f)])
    mut = wake.model(f)
    NP = wake.NP
    sld = (NP + 3) & ~3
    assert (NP, sld) == (1289, 1292)
    pad = np.zeros((NP, sld))
    pad[:, :NP] = mut.sinv
    mut.sinv = pad.reshape(-1)[:NP*NP].reshape((NP, NP))
    ex = wake.excess(done, [mut.apply(r) for r in wake.rs])
    print('padding of sinv32 read as data, wake: %.2e x the tolerance' % ex)
    assert ex >= 100.
    # ... and one entry of the store one fp32 step off, where that is NOT
    # within what two fp64 inverses differ by
    mut = wake.model(f)
    W = done[0].sinv_slack.toarray()
    i, j = [int(q[0]) for q in np.nonzero(W == 0)]
    assert W[i, j] == 0
    mut.sinv = mut.sinv.copy()
    mut.sinv[i, j] = np.nextafter(np.float32(mut.sinv[i, j]), np.float32(np.inf))
    ex = wake.excess(done, [mut.apply(r) for r in wake.rs])
    print('one unambiguous entry of sinv32 one step off: %.2e x the tolerance'
          % ex)
    assert ex >= 100.


def test_half_rho_is_current():
    """`HALF_RHO`, the recorded `rho_ref` of the 2592-row half-precision level
    of the GPU tests, recomputed"""
    from dolfin_navier_scipy_amd.fem import get_sysmats
    _, sm, _ = get_sysmats(problem='cylinderwake', N=3, Re=100)
    F = (sm['M'] + sm['A']/1024.).tocsr()
    b = pm.Bench(sm['M'], F, sm['J'], [])
    rho = b.form(pm.form_of(schur='mg', fhat='cheb', half_max=4096))[2]
    print('rho_ref of the 2592-row half level:', rho)
    for got, rec in zip(rho, pm.HALF_RHO):
        for k in (0, 1):
            assert abs(got[k] - rec[k]) <= 0.5*rec[k] + 0.01
