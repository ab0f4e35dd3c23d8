"""The device convection entry points (`ConvectionP2.apply`, `assemble`, the
Dirichlet tables) against the long double model of tests/conv_model.py, PER
ENTRY against its derived bound, on the synthetic meshes of
tests/conv_meshes.py: cell counts at the block edges of both element kernels,
a fan whose hub dofs lie in 40 cells, no Dirichlet dofs at all, cells without
an inner dof.

Largest error / bound per kernel path, measured on the MI355X (the last test
prints them with `pytest -s`): eight-lane 0.118, lane 0.118 (bit-equal to
each other at every size), matrix Picard 0.136, matrix Newton 0.163, bc gather
0.115.  77 cases, 1.9 s.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sps

import conv_meshes
import conv_model as cm

pytestmark = pytest.mark.gpu

WORST = {}


def _note(path, r):
    WORST[path] = max(WORST.get(path, 0.0), r)
    return r


def _mesh(name):
    kind, n = name.split('-')[0], int(name.split('-')[1])
    if kind == 'fan':
        return conv_meshes.fan(n, seed=n)
    return conv_meshes.rectangle(n, seed=n,
                                 decades=3.0 if 'spread' in name else 0.0)


CASES = ['rect-%d' % n for n in conv_meshes.SIZES] + \
    ['rect-33-nobc', 'fan-40', 'fan-40-nobc', 'rect-257-spread']
_cache = {}


class Case(object):
    def __init__(self, name):
        from dolfin_navier_scipy_amd import convection
        self.name = name
        mesh = self.mesh = _mesh(name)
        n = mesh.ncells
        if 'nobc' in name:
            inv, dbc = mesh.split('none')
        elif n <= 2:
            inv, dbc = mesh.split(0.4)
        else:
            inv, dbc = mesh.split('boundary', full_cells=2 if n >= 255 else 0)
        self.inv, self.dbc = inv, dbc
        rng = self.rng = np.random.default_rng(n)
        self.dbcvals = rng.standard_normal(dbc.size)
        self.v = rng.standard_normal(inv.size)
        if 'spread' in name:
            self.v *= 10.0**rng.integers(-6, 7, inv.size)
        self.sp = cm.Space(mesh.cell_vdofs, mesh.glam, mesh.area, mesh.vdim,
                           inv, dbc)

        def make():
            return convection.ConvectionP2(mesh.cell_vdofs, mesh.glam,
                                           mesh.area, mesh.vdim, inv, dbc,
                                           self.dbcvals)
        self.cv8 = make()
        # the one-lane-per-cell kernel: DNS_CONV_LANE_MIN is read at creation
        old = os.environ.get('DNS_CONV_LANE_MIN')
        os.environ['DNS_CONV_LANE_MIN'] = '1'
        try:
            self.cv1 = make()
        finally:
            if old is None:
                del os.environ['DNS_CONV_LANE_MIN']
            else:
                os.environ['DNS_CONV_LANE_MIN'] = old
        # a pattern larger than connectivity(): structural zeros on top
        con = self.cv8.connectivity()
        nv = inv.size
        extra = sps.random(nv, nv, density=min(1.0, 3.0/max(nv, 1)),
                           format='csr', random_state=np.random.RandomState(n))
        pat = (con + extra + sps.identity(nv, format='csr')).tocsr()
        pat.sort_indices()
        pat.data[:] = 1.0
        self.pat = pat
        self.structural = np.asarray(
            con[pat.nonzero()]).reshape(-1) == 0
        self.cv8.bind_pattern(pat)
        self._models = {}

    def model(self, newton, dbcvals=None, dbcvals_rhs=None, key=None):
        k = (newton, key)
        if k not in self._models:
            self._models[k] = cm.conv_model(
                self.sp, self.v,
                self.dbcvals if dbcvals is None else dbcvals,
                pattern=(self.pat.indptr, self.pat.indices), newton=newton,
                dbcvals_rhs=dbcvals_rhs)
        return self._models[k]


def case(name):
    if name not in _cache:
        _cache[name] = Case(name)
    return _cache[name]


@pytest.mark.parametrize('scale', [1.0, -1.0, 0.37])
@pytest.mark.parametrize('name', CASES)
def test_apply_both_element_kernels(name, scale):
    c = case(name)
    val, bnd = c.model(False)['vec']
    # (`scale` is one more rounding: the count K_VEC + len holds it)
    want = cm.LD(scale)*val
    wb = abs(cm.LD(scale))*bnd
    got8 = c.cv8.apply(c.v, scale=scale).reshape(-1)
    got1 = c.cv1.apply(c.v, scale=scale).reshape(-1)
    r8 = _note('eight-lane', cm.ratio(got8, want, wb))
    r1 = _note('lane', cm.ratio(got1, want, wb))
    print('%s scale %g: eight-lane %.3f lane %.3f' % (name, scale, r8, r1))
    assert r8 <= 1.0 and r1 <= 1.0
    assert np.array_equal(got8, got1)


def _check_assemble(c, got, ref, tag):
    N, rhsbc, rhscon = got
    assert np.array_equal(N.indices, c.pat.indices)
    assert np.all(N.data[c.structural] == 0.0)
    # (structural zeros exist unless connectivity() is already full)
    assert c.structural.sum() > 0 or c.pat.nnz == c.sp.nv**2
    r = dict(N=cm.ratio(N.data, *ref['N']),
             rhsbc=cm.ratio(rhsbc, *ref['rhsbc']),
             rhscon=cm.ratio(rhscon, *ref['vec']))
    print('%s %s: N %.3f rhsbc %.3f rhscon %.3f'
          % (c.name, tag, r['N'], r['rhsbc'], r['rhscon']))
    return r


@pytest.mark.parametrize('newton', [False, True])
@pytest.mark.parametrize('name', CASES)
def test_assemble_per_entry(name, newton):
    c = case(name)
    r = _check_assemble(c, c.cv8.assemble(c.v, newton=newton),
                        c.model(newton), 'newton' if newton else 'picard')
    _note('matrix Newton' if newton else 'matrix Picard', r['N'])
    _note('bc gather', r['rhsbc'])
    _note('eight-lane', r['rhscon'])
    assert max(r.values()) <= 1.0


@pytest.mark.parametrize('newton', [False, True])
@pytest.mark.parametrize('name', ['rect-33', 'fan-40', 'rect-257',
                                  'rect-33-nobc'])
def test_assemble_with_two_value_sets(name, newton):
    """`dbcvals_lin` for the linearisation field, `dbcvals_rhs` for rhsbc"""
    c = case(name)
    rng = np.random.default_rng(11)
    lin, rhs = rng.standard_normal(c.dbc.size), rng.standard_normal(c.dbc.size)
    ref = c.model(newton, dbcvals=lin, dbcvals_rhs=rhs, key='two')
    got = c.cv8.assemble(c.v, newton=newton, dbcvals_lin=lin, dbcvals_rhs=rhs)
    r = _check_assemble(c, got, ref, 'two sets')
    _note('matrix Newton' if newton else 'matrix Picard', r['N'])
    _note('bc gather', r['rhsbc'])
    assert max(r.values()) <= 1.0
    if c.dbc.size:
        # (the two sets do differ in what they give)
        one = c.model(newton, dbcvals=lin, key='one')
        assert cm.ratio(got[1], *one['rhsbc']) > 1.0


@pytest.mark.parametrize('name', ['rect-33', 'fan-40'])
def test_dirichlet_tables_rows_differ(name):
    c = case(name)
    rng = np.random.default_rng(12)
    tab = rng.standard_normal((5, c.dbc.size))
    try:
        for cv in (c.cv8, c.cv1):
            cv.set_dbc_table(tab)
        for row in (0, 2, 4):
            ref = c.model(True, dbcvals=tab[row], key=('row', row))
            for cv, path in ((c.cv8, 'eight-lane'), (c.cv1, 'lane')):
                cv.set_dbc_row(row)
                got = cv.apply(c.v).reshape(-1)
                assert _note(path, cm.ratio(got, *ref['vec'])) <= 1.0
            r = _check_assemble(c, c.cv8.assemble(c.v, newton=True), ref,
                                'table row %d' % row)
            assert max(r.values()) <= 1.0
            # (another row's values are not within the bounds)
            other = c.model(True, dbcvals=tab[(row + 1) % 5],
                            key=('row', (row + 1) % 5))
            assert cm.ratio(got, *other['vec']) > 1.0
        with pytest.raises(Exception):
            c.cv8.set_dbc_row(5)
        # a later set_dbcvals drops the table
        newv = rng.standard_normal(c.dbc.size)
        ref = c.model(False, dbcvals=newv, key='dropped')
        for cv in (c.cv8, c.cv1):
            cv.set_dbcvals(newv)
            cv.set_dbc_row(3)
            assert cm.ratio(cv.apply(c.v), *ref['vec']) <= 1.0
    finally:
        for cv in (c.cv8, c.cv1):
            cv.set_dbcvals(c.dbcvals)


def test_lists_the_cases_rely_on():
    c = case('fan-40')
    hub = np.flatnonzero(np.isin(c.inv, [2*c.mesh.hub_node,
                                         2*c.mesh.hub_node + 1]))
    assert hub.size == 2 and np.all(c.sp.row_len[hub] > 32)
    assert np.all(c.sp.bc_len[hub] > 200)
    assert case('rect-33-nobc').dbc.size == 0 and case('fan-40-nobc').dbc.size == 0
    c = case('rect-257')
    assert (c.sp.code < 0).all(axis=1).sum() >= 2     # cells without inner dof
    c = case('rect-257-spread')
    assert c.mesh.area.max()/c.mesh.area.min() >= 1e3
    assert np.abs(c.v).max()/np.abs(c.v).min() >= 1e10


def test_zz_report_and_close():
    print('largest error / bound per path: '
          + '  '.join('%s %.3f' % kv for kv in sorted(WORST.items())))
    for c in _cache.values():
        c.cv8.close()
        c.cv1.close()
    _cache.clear()
