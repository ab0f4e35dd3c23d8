"""Every epilogue of the two kernels behind the large operator applies,
`k_spmv_stream16x<G, VT, DOTS>` (kernels.hpp) and `k_spmv_pair16x<4, 0, DOTS,
ND>` (pair.hpp), ONE launch at a time through `saddle.spmv_epilogue` against
the long double model of `tests/stream_epi_model.py`:

    rows   |y - y_ref|          <= gamma(2 L + 8) m
    dots   |sum partials - ref| <= gamma(rows + 8) sum |V_i| |y_dev|

(`m`: the modulus sum of the row's mode, `L` its stored length, the dot
references formed from the device's own `y`; `test_stream_epi_model_cpu.py`
shows what margin the bounds leave).  `y` goes up with a sentinel per row and
the partials with NaN, so what a launch did not write is told apart bit for
bit.  Instantiations: the matrices g1 / g2 / g4 / g16 select `G`, `fp32` the
value type, `part` the DOTS instance, `nvec <= 3` / `nvec >= 4` the pair
kernel's ND = 3 / 8.  Every test prints its largest `error / tolerance` (`-s`).
"""
import numpy as np
import pytest
import scipy.sparse as sps

import stream_epi_model as sm

pytestmark = pytest.mark.gpu

CAPS = (1, 3, 7, 8, 9, 13)           # and nblocks, nblocks + 5
NVECS = (0, 1, 3, 4, 8)
ALPHAS = (1., -1., .37)
PAD = 5                              # ld = ny + PAD, the padding holds NaN
PAIR_IDS = ['pair%d_%d_%d' % c for c in sm.PAIR_CASES]


@pytest.fixture(scope='module')
def sad():
    from dolfin_navier_scipy_amd import saddle, _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    return saddle


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Case(object):
    """a matrix with its vectors; `rows`: global rows of the matrix's rows"""

    def __init__(self, name, A, kernel='stream', nv=0, ny=None, rows=None,
                 pair_block=None):
        self.name, self.A, self.kernel, self.nv = name, A, kernel, nv
        self.ny = A.shape[0] if ny is None else ny
        self.rows = np.arange(self.ny) if rows is None else rows
        self.mapped = rows is not None
        self.pair_block = pair_block
        rng = np.random.default_rng(self.ny + A.nnz)
        ny, nc = self.ny, A.shape[1]
        self.x = rng.standard_normal(nc)
        self.b, self.xin = rng.standard_normal((2, ny))
        self.dinv = rng.uniform(.5, 2., ny)*rng.choice([-1., 1.], ny)
        self.ld = ny + PAD
        self.V = np.full((9, self.ld), np.nan)
        self.V[:, :ny] = rng.standard_normal((9, ny))
        self.y0 = 1e30*(1. + np.arange(ny))
        self.nsplit = nc//2 + 3
        self.refs = {}
        self.worst = dict(rows=0., dots=0.)

    def share_vectors(self, whole):
        """a row block of `whole`: the global vectors are the same"""
        for k in ('x', 'b', 'xin', 'dinv', 'V', 'y0'):
            setattr(self, k, getattr(whole, k))

    def launch(self, sad, fp32=False, mode='plain', alpha=1., beta=0., b=False,
               split=False, xin=False, omega=1., nvec=None, ww=False,
               bb=False, cap=65535, guard=None):
        """one launch; `nvec=None`: the instance without dots"""
        dots = nvec is not None
        nv_ = nvec or 0
        kw = dict(kernel=self.kernel, nv=self.nv, fp32_vals=fp32, mode=mode,
                  alpha=alpha, beta=beta, omega=omega, grid_cap=cap,
                  guard=guard, pair_block=self.pair_block)
        needs_b = b or mode != 'plain'
        kw['b'] = self.b if needs_b else None
        if mode != 'plain':
            kw['dinv'] = self.dinv
            kw['xin'] = self.xin if xin else None
        if split:
            kw.update(x2=self.x[self.nsplit:], nsplit=self.nsplit)
        if self.mapped and self.kernel == 'stream':
            kw['rowmap'] = self.rowmap
        slots = min(cap, self.A.shape[0]) + 3
        if dots:
            kw.update(V=self.V[:nv_].copy() if nv_ else None, nvec=nv_,
                      ld=self.ld, with_ww=ww, with_bb=bb,
                      part=np.full((nv_ + 1)*slots + 7, np.nan),
                      part_bb=np.full(slots, np.nan) if bb else None)
        res = sad.spmv_epilogue(self.A, self.x[:self.nsplit] if split
                                else self.x, self.y0, **kw)
        res.update(nvec=nv_, ww=ww, bb=bb, dots=dots, needs_b=needs_b)
        key = (fp32, mode, alpha, beta, needs_b, xin, omega)
        if key not in self.refs:
            self.refs[key] = sm.reference(
                self.A, self.x, mode=mode, alpha=alpha, beta=beta,
                b=self.b if needs_b else None,
                dinv=self.dinv if mode != 'plain' else None,
                xin=self.xin if xin and mode != 'plain' else None,
                omega=omega, fp32_vals=fp32, rows=self.rows)
        res['ref'] = self.refs[key]
        return res

    def check_rows(self, res):
        """rows of the launch inside the bound, all others untouched"""
        ref, tol = res['ref']
        y = res['y']
        assert np.isfinite(y).all()
        err = np.abs(y[self.rows].astype(sm.LD) - ref).astype(np.float64)
        bad = np.flatnonzero(err > tol)
        assert bad.size == 0, (self.name, bad[:5], err[bad[:5]], tol[bad[:5]])
        nz = tol > 0
        if nz.any():
            self.worst['rows'] = max(self.worst['rows'],
                                     float((err[nz]/tol[nz]).max()))
        out = np.ones(self.ny, bool)
        out[self.rows] = False
        assert np.array_equal(bits(y[out]), bits(self.y0[out]))

    def check_dots(self, res):
        """requested slots finite and inside the dot bound, all other slots
        untouched"""
        n, nvec = res['nparts'], res['nvec']
        part = res['part']
        table = part[:(nvec + 1)*n].reshape(nvec + 1, n)
        want = nvec + (1 if res['ww'] else 0)
        assert np.isfinite(table[:want]).all()
        assert np.isnan(part[want*n:]).all()
        d = sm.dot_references(res['y'], self.V, nvec,
                              b=self.b if res['bb'] else None, rows=self.rows)
        pairs = [(sm.ldsum(table[i]), d['vy'][i], d['vy_tol'][i])
                 for i in range(nvec)]
        if res['ww']:
            pairs.append((sm.ldsum(table[nvec]), d['ww'], d['ww_tol']))
        if res['bb']:
            assert np.isfinite(res['part_bb'][:n]).all()
            assert np.isnan(res['part_bb'][n:]).all()
            pairs.append((sm.ldsum(res['part_bb'][:n]), d['bb'], d['bb_tol']))
        for i, (got, ref, tol) in enumerate(pairs):
            err = abs(float(got - ref))
            assert err <= tol, (self.name, i, err, tol)
            if tol > 0:
                self.worst['dots'] = max(self.worst['dots'], err/tol)

    def check(self, res):
        self.check_rows(res)
        if res['dots']:
            self.check_dots(res)
        return res

    def report(self, what, note=''):
        print('%s %s: largest error / tolerance rows %.3f dots %.1e %s'
              % (self.name, what, self.worst['rows'], self.worst['dots'],
                 note))
        assert self.worst['rows'] < 1 and self.worst['dots'] < 1
        self.worst = dict(rows=0., dots=0.)


def dots_vs_plain(case, with_dots, without):
    """the DOTS instance is another instantiation of the same row arithmetic:
    equal bits are not guaranteed by construction, the row bound is (both were
    checked against it); says which it was"""
    same = same_bits(with_dots['y'], without['y'])
    return 'y with dots vs without: %s' % (
        'bit-identical' if same else 'within the row bound')


CASES = {}


def stream_case(name):
    if name not in CASES:
        A = sm.stream_matrix(name)
        sm.check_stream_matrix(name, A)
        CASES[name] = Case(name, A)
    return CASES[name]


def stream_block_case(name):
    """rows [v0, v1) and [nv + p0, nv + p1) of the matrix as a rank's row
    block: global columns, global y / b / V / dinv / xin"""
    key = name + '/block'
    if key not in CASES:
        K = stream_case(name).A
        n = K.shape[0]
        nv = (6*n)//10
        v0, v1 = n//7 + 1, n//7 + 1 + (3*n)//10
        p0, p1 = n//20, n//20 + n//5 + 1
        assert 0 < v0 < v1 < nv and nv + p1 < n
        rows = np.r_[v0:v1, nv + p0:nv + p1]
        local = sps.vstack([K[v0:v1], K[nv + p0:nv + p1]], format='csr')
        local.sort_indices()
        assert sm.stream_g_class(local) == sm.stream_g_class(K)
        assert len(sm.stream_rowblocks(local)) >= 4
        c = Case(key, local, ny=n, rows=rows)
        c.rowmap = (v0, v1 - v0, nv + p0, p1 - p0)
        c.share_vectors(stream_case(name))
        CASES[key] = c
    return CASES[key]


def pair_case(nodes, npres, coupled):
    key = ('pair', nodes, npres, coupled)
    if key not in CASES:
        K, nv = sm.pair_matrix(nodes, npres, coupled)
        CASES[key] = Case('pair%d_%d_%d' % (nodes, npres, coupled), K,
                          kernel='pair', nv=nv)
    return CASES[key]


def pair_block_case(nodes, npres, coupled):
    key = ('pair/block', nodes, npres, coupled)
    if key not in CASES:
        K, nv = sm.pair_matrix(nodes, npres, coupled)
        v0, nvl = 2*max(1, nodes//3), 2*max(1, nodes//2)
        p0 = npres//8 + (1 if npres > 1 else 0)
        p1 = npres - npres//4
        assert v0 > 0 and v0 % 2 == 0 and v0 + nvl <= nv and p0 <= p1 <= npres
        rows = np.r_[v0:v0 + nvl, nv + p0:nv + p1]
        local = sps.vstack([K[v0:v0 + nvl], K[nv + p0:nv + p1]], format='csr')
        local.sort_indices()
        c = Case('pair%d_%d_%d/block' % (nodes, npres, coupled), local,
                 kernel='pair', nv=nv, ny=K.shape[0], rows=rows,
                 pair_block=(nvl, v0, p0))
        c.share_vectors(pair_case(nodes, npres, coupled))
        CASES[key] = c
    return CASES[key]


def check_nblocks(case, res):
    if case.kernel == 'stream':
        assert res['nblocks'] == len(sm.stream_rowblocks(case.A))
    elif case.A.shape[0] > 5000:      # the two large systems
        assert res['nblocks'] >= 12
    return res['nblocks']


STREAM = pytest.mark.parametrize('name', sm.STREAM_G)
FP32 = pytest.mark.parametrize('fp32', [False, True], ids=['f64', 'f32'])
PAIRS = pytest.mark.parametrize('pc', sm.PAIR_CASES, ids=PAIR_IDS)


# ---- 1. plain with beta ------------------------------------------------------
def plain_with_beta(sad, c, fp32, nvecs):
    note = ''
    for alpha in ALPHAS:
        plain = c.check(c.launch(sad, fp32, alpha=alpha, beta=-1.5, b=True))
        check_nblocks(c, plain)
        for nvec in nvecs:
            r = c.check(c.launch(sad, fp32, alpha=alpha, beta=-1.5, b=True,
                                 nvec=nvec, ww=True, bb=True))
            note = dots_vs_plain(c, r, plain)
    c.check(c.launch(sad, fp32, alpha=.37))
    c.check(c.launch(sad, fp32, alpha=.37, nvec=1, ww=True))
    c.report('plain with beta', note)


@STREAM
@FP32
def test_stream_plain_with_beta(sad, name, fp32):
    plain_with_beta(sad, stream_case(name), fp32, (2,))


@PAIRS
def test_pair_plain_with_beta(sad, pc):
    plain_with_beta(sad, pair_case(*pc), False, (2, 5))


# ---- 2. split input, sweep, add_cb (stream) ---------------------------------
@STREAM
@FP32
def test_stream_split_sweep_add_cb(sad, name, fp32):
    c = stream_case(name)
    # the split point lies inside the column window of some row block
    assert any(c.A.indices[c.A.indptr[r0]:c.A.indptr[r1]].min() < c.nsplit
               <= c.A.indices[c.A.indptr[r0]:c.A.indptr[r1]].max()
               for r0, r1 in sm.stream_rowblocks(c.A)
               if c.A.indptr[r1] > c.A.indptr[r0])
    for nvec in (None, 2):
        kw = dict(nvec=nvec, ww=nvec is not None, bb=nvec is not None)
        c.check(c.launch(sad, fp32, alpha=-1., beta=2., b=True, split=True,
                         **kw))
        c.check(c.launch(sad, fp32, mode='sweep', alpha=.8, omega=.7, xin=True,
                         **kw))
        c.check(c.launch(sad, fp32, mode='sweep', alpha=1., omega=.7,
                         split=True, **kw))
        c.check(c.launch(sad, fp32, mode='add_cb', alpha=-.6, omega=1.3,
                         split=True, **kw))
        c.check(c.launch(sad, fp32, mode='add_cb', alpha=-.6, omega=1.3,
                         **kw))
    c.report('split / sweep / add_cb')


# ---- 3. fused dots -----------------------------------------------------------
def fused_dots(sad, c, fp32, families):
    """`families`: nvec -> instantiation family (equal bits of y inside one)"""
    from dolfin_navier_scipy_amd import _capi
    plain = c.check(c.launch(sad, fp32, alpha=-1., beta=1., b=True))
    first, note = {}, ''
    for nvec in NVECS:
        for ww in (False, True):
            for bb in (False, True):
                r = c.check(c.launch(sad, fp32, alpha=-1., beta=1., b=True,
                                     nvec=nvec, ww=ww, bb=bb))
                ref = first.setdefault(families(nvec), r)
                assert same_bits(r['y'], ref['y']), (nvec, ww, bb)
                note = dots_vs_plain(c, r, plain)
    with pytest.raises(_capi.DnsError) as exc:
        c.launch(sad, fp32, alpha=-1., beta=1., b=True, nvec=9, ww=True)
    assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
    assert 'fused dots' in str(exc.value)
    c.report('fused dots', note)


@STREAM
@FP32
def test_stream_fused_dots(sad, name, fp32):
    fused_dots(sad, stream_case(name), fp32, lambda nvec: 0)


@PAIRS
def test_pair_fused_dots(sad, pc):
    fused_dots(sad, pair_case(*pc), False, lambda nvec: nvec <= 3)


# ---- 4. capped grids ---------------------------------------------------------
def capped_grids(sad, c, fp32, nvecs):
    nb = check_nblocks(c, c.launch(sad, fp32))
    caps = sorted(set(CAPS + (nb, nb + 5)))
    for nvec in nvecs:
        first = None
        for cap in caps:
            r = c.launch(sad, fp32, alpha=-1., beta=1., b=True, nvec=nvec,
                         ww=True, bb=True, cap=cap)
            assert r['nparts'] == min(cap, nb)
            if r['dots']:
                c.check_dots(r)
            first = first or c.check(r)
            assert same_bits(r['y'], first['y']), cap
    c.report('caps %s of %d row blocks' % (caps, nb))


@STREAM
@FP32
def test_stream_capped_grids(sad, name, fp32):
    capped_grids(sad, stream_case(name), fp32, (None, 3))


@PAIRS
def test_pair_capped_grids(sad, pc):
    capped_grids(sad, pair_case(*pc), False, (None, 3, 4))


# ---- 5. row blocks of a partitioned system ----------------------------------
@STREAM
@FP32
def test_stream_row_block(sad, name, fp32):
    c = stream_block_case(name)
    whole = stream_case(name)
    for nvec in (None, 3):
        kw = dict(nvec=nvec, ww=nvec is not None, bb=nvec is not None)
        r = c.check(c.launch(sad, fp32, alpha=-1., beta=1., b=True, **kw))
        c.check(c.launch(sad, fp32, alpha=.37, beta=-1.5, b=True, cap=3, **kw))
        c.check(c.launch(sad, fp32, mode='sweep', alpha=.8, omega=.7, xin=True,
                         split=True, **kw))
        c.check(c.launch(sad, fp32, mode='add_cb', alpha=-.6, omega=1.3, **kw))
    # the rows of the block are the rows of the whole system's product
    g = whole.launch(sad, fp32, alpha=-1., beta=1., b=True)
    r = c.check(c.launch(sad, fp32, alpha=-1., beta=1., b=True))
    tol = g['ref'][1][c.rows] + r['ref'][1]
    assert (np.abs(g['y'][c.rows] - r['y'][c.rows]) <= tol).all()
    c.report('row block %s' % (c.rowmap,))


@PAIRS
def test_pair_row_block(sad, pc):
    c = pair_block_case(*pc)
    whole = pair_case(*pc)
    g = whole.check(whole.launch(sad, alpha=-1., beta=1., b=True))
    for nvec in (None, 3, 4):
        kw = dict(nvec=nvec, ww=nvec is not None, bb=nvec is not None)
        r = c.check(c.launch(sad, alpha=-1., beta=1., b=True, **kw))
        c.check(c.launch(sad, alpha=.37, beta=-1.5, b=True, cap=3, **kw))
        tol = g['ref'][1][c.rows] + r['ref'][1]
        assert (np.abs(g['y'][c.rows] - r['y'][c.rows]) <= tol).all()
    c.report('row block %s' % (c.pair_block,))


# ---- 6. guard, 7. determinism -------------------------------------------------
def guard_and_determinism(sad, c, fp32, nvecs, modes):
    for nvec in nvecs:
        for mode in modes:
            kw = dict(mode=mode, alpha=-.6, omega=1.3, b=True, nvec=nvec,
                      ww=nvec is not None, bb=nvec is not None, cap=7)
            if mode == 'plain':
                kw['beta'] = 1.
            free = c.check(c.launch(sad, fp32, **kw))
            again = c.launch(sad, fp32, **kw)
            open_ = c.launch(sad, fp32, guard=0, **kw)
            shut = c.launch(sad, fp32, guard=1, **kw)
            assert same_bits(shut['y'], c.y0)
            for r in (again, open_):
                assert same_bits(r['y'], free['y'])
            if nvec is not None:
                assert np.isnan(shut['part']).all()
                assert np.isnan(shut['part_bb']).all()
                for r in (again, open_):
                    assert same_bits(r['part'], free['part'])
                    assert same_bits(r['part_bb'], free['part_bb'])
    c.report('guard / determinism')


@STREAM
@FP32
def test_stream_guard_and_determinism(sad, name, fp32):
    guard_and_determinism(sad, stream_case(name), fp32, (None, 3),
                          ('plain', 'sweep'))


@PAIRS
def test_pair_guard_and_determinism(sad, pc):
    guard_and_determinism(sad, pair_case(*pc), False, (None, 3, 4), ('plain',))


# ---- the block kinds of the streaming kernel ---------------------------------
@pytest.mark.parametrize('name', sm.STREAM_SPECIAL)
def test_stream_block_kinds(sad, name):
    """a single long row, the 256-row cap, the second 16-bit window, raw
    32-bit indices: every epilogue family on each"""
    c = stream_case(name)
    for fp32 in (False, True):
        for nvec in (None, 3):
            kw = dict(nvec=nvec, ww=nvec is not None, bb=nvec is not None)
            r = c.check(c.launch(sad, fp32, alpha=-1., beta=1., b=True, **kw))
            check_nblocks(c, r)
            c.check(c.launch(sad, fp32, alpha=.37, beta=-1.5, b=True,
                             split=True, cap=3, **kw))
            c.check(c.launch(sad, fp32, mode='sweep', alpha=.8, omega=.7,
                             xin=True, split=True, **kw))
            c.check(c.launch(sad, fp32, mode='add_cb', alpha=-.6, omega=1.3,
                             cap=2, **kw))
    c.report('block kinds %s' % sorted(set(sm.stream_block_kinds(c.A))))


# ---- what the pair kernel does not implement is refused ----------------------
def test_pair_refuses_what_it_does_not_implement(sad):
    from dolfin_navier_scipy_amd import _capi
    c = pair_case(5, 3, False)
    kw = dict(kernel='pair', nv=c.nv)
    for bad in (dict(x2=c.x[8:], nsplit=8, x=c.x[:8]),
                dict(mode='sweep', dinv=c.dinv, b=c.b),
                dict(mode='add_cb', dinv=c.dinv, b=c.b),
                dict(rowmap=(0, c.ny, 0, 0)), dict(fp32_vals=True),
                dict(with_bb=True, b=c.b, part_bb=np.zeros(8)),
                dict(nv=c.nv - 1)):
        args = dict(kw, x=c.x)
        args.update(bad)
        x = args.pop('x')
        with pytest.raises(_capi.DnsError) as exc:
            sad.spmv_epilogue(c.A, x, c.y0, **args)
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT, bad
