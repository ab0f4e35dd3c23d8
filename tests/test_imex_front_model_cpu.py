"""The long double model of the IMEX front (`imex_front_model.py`) on the CPU:
its coefficient table, its tolerance (fixed from the model alone: fp64
evaluations in the orders a kernel may choose stay within a quarter of it),
the allowance c6 of the six-node step's residual by linearity, and the proof
that the checks of `test_gpu_imex_front.py` can fail: every mutation misses
the model by at least 100 tolerances on the inputs of the GPU cases.
`pytest -s` prints the figures the model's docstring lists."""
import numpy as np
import pytest

import imex_front_model as fm
from imex_front_model import LD, U

LANES = (1, 2, 4, 8, 16, 32, 64)
SCHEMES = ('cnab', 'sbdf2')


@pytest.fixture(scope='module')
def toy(toy_prob):
    out = {}
    for sch in SCHEMES:
        F, J, K, R1, cf = fm.toy_system(toy_prob, scheme=sch)
        out[sch] = dict(K=K, R1=R1, cf=cf)
    NP, NV = J.shape
    out['nv'], out['np'], out['n'] = NV, NP, NV + NP
    out['inp'] = fm.rough_inputs(NV, NP)
    out['ring'] = fm.rough(100, 5, NV + NP)
    return out


def _args(toy, sch, nsol, order, ring=None, g=None, nfc=None, **cfkw):
    s, inp = toy[sch], toy['inp']
    cf = dict(s['cf'], **cfkw)
    if nsol < 2:
        cf['a_p'] = 0.
    return dict(K=s['K'], R1=s['R1'], ring=toy['ring'] if ring is None else ring,
                e=fm.extrap_table(nsol, order), a_c=cf['a_c'], a_p=cf['a_p'],
                cn_c=cf['cn_c'], cn_o=cf['cn_o'],
                nfc=inp['nfc'] if nfc is None else nfc,
                g=inp['g'] if g is None else g, gp=inp['gp'])


def _mode2(toy, sch, rel=1e-10):
    """a carry step's inputs: K x products in fp64, a previous right-hand side
    whose solve left a residual of `rel` (the size a converged solve leaves)"""
    K, ring, nv = toy[sch]['K'], toy['ring'], toy['nv']
    kx = np.array([fm.spmv64(K, ring[i], 8, True) for i in range(5)])
    mag = np.abs(K) @ np.abs(ring[0])
    return dict(kind='mode2', b_prev=kx[0] + rel*mag*fm.rough(7, toy['n']),
                kxs=kx[1:], r_old=rel*mag[:nv]*fm.rough(8, nv))


def test_coefficient_table_is_derived():
    exp = {(2, 1): (2, -1), (3, 2): (3, -3, 1), (4, 3): (4, -6, 4, -1),
           (5, 4): (5, -10, 10, -5, 1)}
    for (nsol, order), c in exp.items():
        assert [float(x) for x in fm.lagrange_at_one(nsol)] == list(c)
        assert tuple(fm.extrap_table(nsol, order)[:nsol]) == c
    assert tuple(fm.extrap_table(5, fm.FIT35)) == (3.2, -2.8, -0.8, 2.2, -0.8)
    # history still filling: the lower order; 13 means the cubic then
    assert tuple(fm.extrap_table(3, 4)) == (3, -3, 1, 0, 0)
    assert tuple(fm.extrap_table(4, fm.FIT35)) == (4, -6, 4, -1, 0)
    assert tuple(fm.extrap_table(2, fm.FIT35)) == (2, -1, 0, 0, 0)
    assert tuple(fm.extrap_table(5, 7)) == (5, -10, 10, -5, 1)
    for nsol in range(1, 6):
        assert tuple(fm.extrap_table(nsol, 0)) == (1, 0, 0, 0, 0)
        assert tuple(fm.extrap_table(nsol, -1)) == (1, 0, 0, 0, 0)
        assert tuple(fm.extrap_table(1, nsol)) == (1, 0, 0, 0, 0)
    # the exceptions of single forms
    assert fm.order_for(-1, 'Fused') == -1 and fm.order_for(-1, 'Plain') == 1
    assert fm.order_for(13, 'StreamRhs') == 3 and fm.order_for(13, 'Six') == 13
    assert fm.order_for(13, 'Six', primed_six=True) == 4


def test_fp64_reorders_stay_within_a_quarter_of_the_tolerance(toy):
    worst = {}
    for sch in SCHEMES:
        for nsol, order in ((1, 4), (2, 4), (3, 4), (4, 4), (5, 4),
                            (5, fm.FIT35)):
            for carry in (None, 'mode2', 'six'):
                if carry and nsol < 5:
                    continue
                a = _args(toy, sch, nsol, order)
                if carry == 'mode2':
                    a['carry'] = _mode2(toy, sch)
                elif carry == 'six':
                    a['carry'] = dict(kind='six',
                                      rc=1e-10*fm.rough(9, 2, toy['nv']))
                mod = fm.front_model(**a)
                for lanes in LANES:
                    for fused in (True, False):
                        got = fm.front_eval64(lanes=lanes, fused=fused, **a)
                        for k, v in got.items():
                            key = (carry or 'plain') + ' ' + k
                            # (a sum of squares: against the long double sum
                            # over the SAME fp64 vector, as on the GPU)
                            ref = fm.sumsq(got[k[0]]) if k in ('rr', 'bb') \
                                else mod[k]
                            if k in ('rr', 'bb'):
                                v = np.sum(fm._ld(v))
                            worst[key] = max(worst.get(key, 0.),
                                             fm.ratio(v, *ref))
    print('fp64 reorders, largest error / tolerance:',
          {k: float('%.3g' % v) for k, v in sorted(worst.items())})
    assert max(worst.values()) <= 0.25, worst


def test_c6_of_the_residual_by_linearity(toy):
    """the six-node route in fp64 against long double b - K x_new"""
    K, n = toy['cnab']['K'], toy['n']
    x0 = toy['ring'][0]
    worst = 0.
    for ncol in (1, 2):
        for seed in range(4):
            zs = fm.rough(200 + seed, ncol, n)
            ys = 1e-6*np.linalg.norm(x0)/np.linalg.norm(zs, axis=1)/ncol
            # a right-hand side whose solution is near x_new
            xn = x0 + sum(y*z for y, z in zip(ys, zs))
            b = fm.spmv64(K, xn, 8, True)
            x_new, r_new = fm.six_route64(K, b, x0, zs, ys)
            assert abs(np.linalg.norm(x_new - x0)/np.linalg.norm(x0)/1e-6
                       - 1) < .5
            ref = fm._ld(b) - fm.spmv(K, fm._ld(x_new))
            unit = fm.six_residual_bound(K, b, x0, x_new)
            worst = max(worst, fm.ratio(r_new, ref, unit/U, tol=U))
    c6 = max(16, int(2**np.ceil(np.log2(4*worst))))
    print('c6: largest ratio %.3g -> c6 = %d' % (worst, c6))
    assert c6 == fm.C6


def test_every_mutation_misses_the_model_by_100_tolerances(toy):
    inp, ring, nv = toy['inp'], toy['ring'], toy['nv']
    seen = {}

    def miss(name, base, mutant, keys=('x0', 'b', 'kx', 'r')):
        mb, mm = fm.front_model(**base), fm.front_model(**mutant)
        r = max(fm.ratio(mm[k][0], *mb[k]) for k in keys)
        seen[name] = min(seen.get(name, np.inf), r)

    for sch in SCHEMES:
        for order in (4, fm.FIT35):
            base = _args(toy, sch, 5, order)
            for i in range(4):
                sw = ring.copy()
                sw[[i, i + 1]] = sw[[i + 1, i]]
                miss('slots %d,%d' % (i, i + 1), base, dict(base, ring=sw))
            # the x0 of the step before: the same set one slot further back
            back = np.vstack([ring[1:], fm.rough(101, 1, toy['n'])])
            mut = fm.front_model(**dict(base, ring=back))
            mb = fm.front_model(**base)
            seen['x0 before'] = min(seen.get('x0 before', np.inf),
                                    fm.ratio(mut['x0'][0], *mb['x0']))
            miss('cn swapped', base, dict(base, cn_c=base['cn_o'],
                                          cn_o=base['cn_c']), ('b', 'r'))
            miss('g neighbour', dict(base, g=inp['gtab'][2]),
                 dict(base, g=inp['gtab'][1]), ('b', 'r'))
            miss('g neighbour', dict(base, g=inp['gtab'][3]),
                 dict(base, g=inp['gtab'][2]), ('b', 'r'))
            c2 = dict(base, carry=_mode2(toy, sch))
            miss('carry dropped', c2, base, ('b',))
        for nsol in (2, 3, 4, 5):
            for order in (4, fm.FIT35):
                base = _args(toy, sch, nsol, order)
                miss('set of nsol - 1', base,
                     dict(base, e=fm.extrap_table(nsol - 1, order)))
    # a_p at nsol = 1 (x_p = x_c, as the separate right-hand side kernel had it)
    base = _args(toy, 'sbdf2', 1, 4)
    r1 = ring.copy()
    r1[1] = r1[0]
    miss('a_p at nsol 1', base, dict(base, ring=r1,
                                     a_p=toy['sbdf2']['cf']['a_p']), ('b', 'r'))
    print('mutations, smallest miss / tolerance:',
          {k: float('%.2g' % v) for k, v in seen.items()})
    assert len(seen) == 10 and min(seen.values()) >= 100, seen


# ---- the front by rows (row-partitioned forms) -------------------------------

PARTS = {2: ([0, 644, 1286], [0, 104, 207]),
         3: ([0, 430, 860, 1286], [0, 70, 140, 207])}


def _conv_space(prob):
    import conv_model as cm
    th = prob['th']
    return cm.Space(th._vdofs(), th.glam, th.area, th.vdim, prob['invinds'],
                    prob['dbcinds'])


def _rows_args(toy, sch, P, rank, nsol, order, ring=None, carry=None, **cfkw):
    a = _args(toy, sch, nsol, order, ring=ring, **cfkw)
    st_v, st_p = PARTS[P]
    return dict(a, st_v=st_v, st_p=st_p, rank=rank, carry=carry)


@pytest.mark.parametrize('P', [2, 3])
def test_footprint_is_own_rows_plus_the_halo_lists(toy, toy_prob, P):
    """`footprint` minus the own rows == the union of `comm.halo_lists` (host
    only) over the blocks of K the rank's rows hold (F and J: velocity
    columns, J^T: pressure columns) and its rows of R1; the partition is the
    library's (`partition_range`)"""
    from dolfin_navier_scipy_amd.build import build_library
    build_library(verbose=False)
    from dolfin_navier_scipy_amd import comm
    K, R1 = toy['cnab']['K'], toy['cnab']['R1']
    nv, npr = toy['nv'], toy['np']
    st_v = [0] + [comm.partition_range(nv, P, r)[1] for r in range(P)]
    st_p = [0] + [comm.partition_range(npr, P, r)[1] for r in range(P)]
    assert (st_v, st_p) == PARTS[P]
    for r in range(P):
        assert comm.partition_range(nv, P, r) == (st_v[r], st_v[r + 1])
    F, JT, J = K[:nv, :nv].tocsr(), K[:nv, nv:].tocsr(), K[nv:, :nv].tocsr()
    sp = _conv_space(toy_prob)
    seen = np.zeros(nv + npr, dtype=int)
    for r in range(P):
        own = fm.own_rows(st_v, st_p, r, nv)
        seen[own] += 1
        fp = fm.footprint(K, R1, st_v, st_p, r)
        assert np.all(np.diff(fp) > 0)
        v0, v1, p0, p1 = st_v[r], st_v[r + 1], st_p[r], st_p[r + 1]
        halo = set()
        for A, r0, r1, cs, ncol, off in ((F, v0, v1, st_v, nv, 0),
                                         (J, p0, p1, st_v, nv, 0),
                                         (R1, v0, v1, st_v, nv, 0),
                                         (JT, v0, v1, st_p, npr, nv)):
            for q, lst in enumerate(comm.halo_lists(A, r0, r1, P, r, cs,
                                                    ncol)):
                assert q != r or lst.size == 0
                halo.update(int(c) + off for c in lst)
        assert set(fp) - set(own) == halo
        assert len(halo) > 0
        # with the convection: every inner dof of every selected cell, and no
        # other cell has a slot on an own row
        fpc = fm.footprint(K, R1, st_v, st_p, r, sp)
        sel = fm.selected_cells(sp, st_v, r)
        assert set(fp) <= set(fpc)
        d = sp.code[sel]
        assert set(d[d >= 0]) <= set(fpc)
        rest = np.delete(sp.code, sel, axis=0)
        assert not np.any((rest >= v0) & (rest < v1))
        assert 0 < sel.size < sp.nc
        print('P %d rank %d: own %d halo %d with cells %d, %d of %d cells' % (
            P, r, own.size, len(halo), fpc.size - own.size, sel.size, sp.nc))
    assert np.all(seen == 1)


def _rc(toy, rel=1e-10):
    """carried residuals of the size a converged solve leaves"""
    mag = (np.abs(toy['cnab']['K']) @ np.abs(toy['ring'][0]))[:toy['nv']]
    return dict(rc=rel*mag*fm.rough(9, 2, toy['nv']))


@pytest.mark.parametrize('P', [2, 3])
def test_fp64_by_rows_stays_within_a_quarter_of_the_tolerance(toy, P):
    worst = {}
    for sch in SCHEMES:
        for nsol, order, carry in ((1, 4, None), (2, 4, None), (5, 4, None),
                                   (5, fm.FIT35, None), (2, 4, _rc(toy)),
                                   (5, 4, _rc(toy))):
            for rank in range(P):
                a = _rows_args(toy, sch, P, rank, nsol, order, carry=carry)
                mod = fm.front_model_rows(**a)
                got = fm.dist_front_eval64(lanes=32, fused=True, **a)
                got['x0'] = got['x0'][mod['fp']]
                for k, v in got.items():
                    key = ('carry ' if carry else '') + k
                    worst[key] = max(worst.get(key, 0.), fm.ratio(v, *mod[k]))
    print('fp64 by rows, %d ranks, largest error / tolerance:' % P,
          {k: float('%.3g' % v) for k, v in sorted(worst.items())})
    assert max(worst.values()) <= 0.25, worst


def test_the_model_by_rows_reads_its_footprint_only_and_equals_the_whole(toy):
    """every entry outside the footprint may be anything; on the own rows the
    model by rows IS the un-partitioned model"""
    for P in (2, 3):
        for rank in range(P):
            a = _rows_args(toy, 'sbdf2', P, rank, 5, 4)
            mod = fm.front_model_rows(**a)
            junk = toy['ring'].copy()
            out = np.ones(toy['n'], dtype=bool)
            out[mod['fp']] = False
            junk[:, out] = 1e300
            mod2 = fm.front_model_rows(**dict(a, ring=junk))
            whole = fm.front_model(**_args(toy, 'sbdf2', 5, 4))
            for k in ('b', 'kx', 'r'):
                assert np.all(np.isfinite(mod[k][0].astype(np.float64)))
                assert np.array_equal(mod[k][0], mod2[k][0])
                assert np.array_equal(mod[k][0], whole[k][0][mod['own']]), k
                assert np.array_equal(mod[k][1], whole[k][1][mod['own']]), k
            assert np.array_equal(mod['x0'][0], whole['x0'][0][mod['fp']])


def test_every_mutation_by_rows_misses_the_model_by_100_tolerances(toy,
                                                                   toy_prob):
    import conv_model as cm
    nv, n = toy['nv'], toy['n']
    seen = {}

    def note(name, r):
        seen[name] = min(seen.get(name, np.inf), r)

    for P in (2, 3):
        st_v, st_p = PARTS[P]
        for sch in SCHEMES:
            cfd = toy[sch]['cf']
            for rank in range(P):
                base = _rows_args(toy, sch, P, rank, 5, 4)
                mb = fm.front_model_rows(**base)
                len1 = st_v[rank + 1] - st_v[rank]
                # row2 off by one: the pressure rows one further down (where
                # there is one)
                if rank + 1 < P:
                    sp1 = list(st_p)
                    sp1[rank], sp1[rank + 1] = sp1[rank] + 1, sp1[rank + 1] + 1
                    mm = fm.front_model_rows(**dict(base, st_p=sp1))
                    note('row2 + 1', max(fm.ratio(mm[k][0], *mb[k])
                                         for k in ('b', 'r')))
                # len1 one short: the last own velocity row is formed by the
                # pressure branch (b = gp of the first own pressure row, the K
                # row of that row)
                mut = {k: np.array(mb[k][0]) for k in ('b', 'kx')}
                mut['b'][len1 - 1] = mb['b'][0][len1]
                mut['kx'][len1 - 1] = mb['kx'][0][len1]
                note('len1 - 1', min(
                    fm.ratio(mut['b'], *mb['b']),
                    fm.ratio(mut['b'] - mut['kx'], *mb['r'])))
                # one halo entry of x0 from the previous ring slot
                halo = np.setdiff1d(mb['fp'], mb['own'])
                hv = halo[halo < nv]
                assert hv.size
                # (a column may be in the pattern with explicit zeros only,
                # the coupling of the two velocity components: the start
                # residual then cannot see the entry, the check of x0 on the
                # footprint does)
                colw = np.asarray(abs(toy[sch]['K'][mb['own']]).sum(axis=0))[0]
                for h in (hv[0], hv[-1]):
                    ring = toy['ring'].copy()
                    ring[:4, h] = toy['ring'][1:, h]
                    mm = fm.front_model_rows(**dict(base, ring=ring))
                    note('stale halo entry: x0',
                         fm.ratio(mm['x0'][0], *mb['x0']))
                    if colw[h] > 1e-8*colw.max():
                        note('stale halo entry: r',
                             fm.ratio(mm['r'][0], *mb['r']))
                # rcc <-> rcp
                rc = _rc(toy)
                cb = fm.front_model_rows(**dict(base, carry=rc))
                cm_ = fm.front_model_rows(
                    **dict(base, carry=dict(rc=rc['rc'][::-1])))
                note('rcc <-> rcp', min(fm.ratio(cm_['b'][0], *cb['b']),
                                        fm.ratio(cm_['carry'][0],
                                                 *cb['carry'])))
                note('carry dropped', fm.ratio(mb['b'][0], *cb['b']))
            # a_p at nsol = 1 (x_p = x_c)
            if cfd['a_p'] != 0:
                for rank in range(P):
                    base = _rows_args(toy, sch, P, rank, 1, 4)
                    r1 = toy['ring'].copy()
                    r1[1] = r1[0]
                    mm = fm.front_model_rows(
                        **dict(base, ring=r1, a_p=cfd['a_p']))
                    mb = fm.front_model_rows(**base)
                    note('a_p at nsol 1', fm.ratio(mm['b'][0], *mb['b']))
    # the gather of a non-selected cell: one cell that touches an own row keeps
    # the values of another velocity (its slot was never evaluated)
    sp = _conv_space(toy_prob)
    inp = toy['inp']
    res = cm.conv_model(sp, inp['v_c'], toy_prob['dbcvals'])
    stale = cm.conv_model(sp, inp['v_p'], toy_prob['dbcvals'])['cells'][0]
    val, bnd = res['vec']
    for P in (2, 3):
        st_v, st_p = PARTS[P]
        for rank in range(P):
            sel = fm.selected_cells(sp, st_v, rank)
            ov = np.arange(st_v[rank], st_v[rank + 1])
            for cell in (sel[0], sel[-1]):
                cv = np.array(res['cells'][0])
                cv[cell] = stale[cell]
                mut = sp.gather_rows(cv)
                note('non-selected cell: nfc_c',
                     cm.ratio(mut[ov], val[ov], bnd[ov]))
                base = _rows_args(toy, 'cnab', P, rank, 5, 4)
                nfc = np.array([-val, inp['nfc'][0]], dtype=np.float64)
                nfm = np.array([-mut, inp['nfc'][0]], dtype=np.float64)
                mb = fm.front_model_rows(**dict(base, nfc=nfc))
                mm = fm.front_model_rows(**dict(base, nfc=nfm))
                note('non-selected cell: b', fm.ratio(mm['b'][0], *mb['b']))
    print('mutations by rows, smallest miss / tolerance:',
          {k: float('%.2g' % v) for k, v in seen.items()})
    assert len(seen) == 9 and min(seen.values()) >= 100, seen
