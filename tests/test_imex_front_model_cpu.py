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
