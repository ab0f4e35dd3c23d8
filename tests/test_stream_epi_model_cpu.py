"""The reference of `tests/stream_epi_model.py` on its own (no library call):
it equals SciPy's product to rounding, and a plain fp64 evaluation of every
mode -- each row's terms summed in a shuffled order, as a kernel that sums a
tile through LDS and a sub-wave may -- stays inside the row bounds
`gamma(2L + 8) m` for every matrix of the case list, so the bounds hold with
margin before any device enters.  Prints the largest `error / bound` (`-s`).
"""
import numpy as np
import pytest

import stream_epi_model as sm

MATS = {}


def _mat(key):
    if key not in MATS:
        MATS[key] = sm.stream_matrix(key) if isinstance(key, str) \
            else sm.pair_matrix(*key)[0]
    return MATS[key]


ALL = list(sm.STREAM_G + sm.STREAM_SPECIAL) + list(sm.PAIR_CASES)
IDS = [k if isinstance(k, str) else 'pair%d_%d_%d' % k for k in ALL]


@pytest.mark.parametrize('name', sm.STREAM_G + sm.STREAM_SPECIAL)
def test_stream_matrices_reach_their_branches(name):
    sm.check_stream_matrix(name, _mat(name))


@pytest.mark.parametrize('key', ALL, ids=IDS)
def test_model_product_equals_scipy(key):
    A = _mat(key)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(A.shape[1])
    s, sabs, L = sm.product(A, x)
    err = np.abs(s - (A @ x).astype(sm.LD))
    bound = sm.gamma(L + 1).astype(sm.LD)*sabs
    assert (err <= bound).all()
    assert (np.abs(sabs - (abs(A) @ np.abs(x))) <= bound).all()
    # fp32 values: the rounded matrix, exactly
    A32 = A.copy()
    A32.data = A.data.astype(np.float32).astype(np.float64)
    s32 = sm.product(A, x, fp32_vals=True)[0]
    assert (np.abs(s32 - (A32 @ x).astype(sm.LD)) <= bound).all()
    if A.nnz:
        assert np.abs(s32 - s).max() > 0


def _shuffled_fp64(A, x, rng, fp32_vals):
    """fp64 row sums, every row's products added in a random order"""
    terms = sm.device_values(A, fp32_vals)*x[A.indices]
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    order = np.lexsort((rng.random(terms.size), rows))
    return sm.row_sums(A.indptr, terms[order])


@pytest.mark.parametrize('key', ALL, ids=IDS)
def test_fp64_evaluation_stays_inside_the_row_bounds(key):
    A = _mat(key)
    rng = np.random.default_rng(11)
    n, nc = A.shape
    x = rng.standard_normal(nc)
    b, xin = rng.standard_normal((2, n))
    dinv = rng.uniform(0.5, 2., n)*rng.choice([-1., 1.], n)
    worst = 0.
    for fp32 in (False, True):
        s64 = _shuffled_fp64(A, x, rng, fp32)
        sabs = sm.product(A, x, fp32)[1]
        for mode, kw in (('plain', dict(alpha=1., beta=-1.5, b=b)),
                         ('plain', dict(alpha=-1., beta=2., b=b)),
                         ('plain', dict(alpha=.37, beta=-.25, b=b)),
                         ('plain', dict(alpha=.37)),
                         ('sweep', dict(alpha=.8, b=b, dinv=dinv, xin=xin,
                                        omega=.7)),
                         ('sweep', dict(alpha=1., b=b, dinv=dinv, omega=.7)),
                         ('add_cb', dict(alpha=-.6, b=b, dinv=dinv,
                                         omega=1.3))):
            ref, tol = sm.reference(A, x, mode=mode, fp32_vals=fp32, **kw)
            full = dict(alpha=1., beta=0., b=None, dinv=None, xin=None,
                        omega=1.)
            full.update(kw)
            got, _ = sm.epilogue(s64, sabs, mode, dtype=np.float64, **full)
            assert got.dtype == np.float64
            err = np.abs(got.astype(sm.LD) - ref).astype(np.float64)
            assert (err <= tol).all(), (mode, kw.get('alpha'), fp32)
            nz = tol > 0
            if nz.any():
                worst = max(worst, float((err[nz]/tol[nz]).max()))
            assert (err[~nz] == 0).all()
    print('%s: largest fp64 error / bound %.3f' % (key, worst))
    assert 0 < worst < 1


def test_dot_references_and_bounds():
    """the dot references see the rows of the map only, and an fp64 dot in a
    shuffled order stays inside gamma(rows + 8) sum |V y|"""
    rng = np.random.default_rng(5)
    n, ld = 3000, 3011
    y = rng.standard_normal(n)
    b = rng.standard_normal(n)
    V = np.full((4, ld), np.nan)
    V[:, :n] = rng.standard_normal((4, n))
    rows = np.r_[100:900, 2000:2600]
    d = sm.dot_references(y, V, 4, b=b, rows=rows)
    worst = 0.
    for i in range(4):
        p = rng.permutation(rows)
        got = 0.
        for t in V[i, p]*y[p]:
            got += t
        err = abs(float(sm.LD(got) - d['vy'][i]))
        assert err <= d['vy_tol'][i]
        worst = max(worst, err/d['vy_tol'][i])
    assert abs(float(d['ww'] - sm.LD(y[rows] @ y[rows]))) <= d['ww_tol']
    assert abs(float(d['bb'] - sm.LD(b[rows] @ b[rows]))) <= d['bb_tol']
    full = sm.dot_references(y, V, 1)
    assert abs(float(full['vy'][0] - d['vy'][0])) > 1e3*d['vy_tol'][0]
    print('dots: largest fp64 error / bound %.2e' % worst)
    assert 0 < worst < 1
