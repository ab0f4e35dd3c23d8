"""The assembly pair of a trapezoidal step -- `k_conv_step_cells` and the row
part `trap_rows<HASG, WITHR, CELLS>` of `k_conv_mat_bc_gather` -- through the
test-only probe `TrapezoidalStepper.assembly_probe` (the launches a step
enqueues before its solve, by the member function the step calls), PER ENTRY
against `conv_model.trap_assembly_model` and its derived bounds.

M, A and J are random values on the bound pattern (the kernels treat them as
data; M has a dominant diagonal); J has rows of 0 to more than 16 entries.
The fan has a hub whose lists -- cells, Dirichlet pairs, matrix row -- are
longer than 32: every 16-lane loop behind the peeled first trips runs.

Largest error / bound per path, measured on the MI355X (the last test prints
them with `pytest -s`): trap_rows<HASG=0, WITHR=0> 0.465, <0, 1> 0.777,
<1, 0> 0.544, <1, 1> 0.777 (CELLS always on), ||r||^2 0.005, ||b||^2 0.008,
F 0.990 (an entry M dominates: half an ulp of it against gamma_1 |M|), N
through the step's element launch 0.119 (Picard) and 0.100 (Newton).
23 cases, 2.2 s.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sps

import conv_meshes
import conv_model as cm

pytestmark = pytest.mark.gpu

WORST = {}
DT = 3.7e-3
NSLOTS, LIN_SLOT = 4, 2


def _note(path, r):
    WORST[path] = max(WORST.get(path, 0.0), r)
    return r


class env(object):
    """an environment variable set (or unset: None) around a creation"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        if self.value is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


def _random_j(npr, nv, hot, rng):
    """np x nv, row lengths 0 .. > 16 (one row: > 16); the columns `hot`
    sit in every row that is not empty (long rows of J^T)"""
    lens = [37] if npr == 1 else [(0, 1, 2, 7, 16, 17, 18, 35)[i % 8]
                                  for i in range(npr)]
    rows, cols = [], []
    for i, ln in enumerate(lens):
        ln = min(ln, nv)
        if ln == 0:
            continue
        pick = list(hot[:ln])
        rest = np.setdiff1d(np.arange(nv), pick)
        pick += list(rng.permutation(rest)[:ln - len(pick)])
        rows += [i]*ln
        cols += pick
    J = sps.coo_matrix((rng.standard_normal(len(rows)), (rows, cols)),
                       shape=(npr, nv)).tocsr()
    J.sort_indices()
    return J


MESHES = {'fan40-np300': ('fan', 40, 300), 'fan40-np17': ('fan', 40, 17),
          'rect33-np1': ('rect', 33, 1), 'rect1000-np300': ('rect', 1000, 300),
          'nobc-np17': ('nobc', 33, 17)}
_setups = {}


def setup_of(name):
    if name in _setups:
        return _setups[name]
    kind, n, npr = MESHES[name]
    s = type('Setup', (), {})()
    mesh = s.mesh = (conv_meshes.fan(n, seed=n) if kind == 'fan'
                     else conv_meshes.rectangle(n, seed=n))
    s.inv, s.dbc = mesh.split('none' if kind == 'nobc' else 'boundary')
    s.sp = cm.Space(mesh.cell_vdofs, mesh.glam, mesh.area, mesh.vdim, s.inv,
                    s.dbc)
    nv, nd = s.inv.size, s.dbc.size
    rng = np.random.default_rng(100 + n + npr)
    s.dbc_tab = rng.standard_normal((NSLOTS, nd))
    s.fv_tab = rng.standard_normal((NSLOTS, nv))
    s.fp_tab = rng.standard_normal((NSLOTS, npr))
    s.v_lin, s.v_c = rng.standard_normal(nv), rng.standard_normal(nv)
    s.x0 = rng.standard_normal(nv + npr)
    hot = []
    if kind == 'fan':
        hot = list(np.flatnonzero(np.isin(s.inv, [2*mesh.hub_node,
                                                  2*mesh.hub_node + 1])))
    s.J = _random_j(npr, nv, hot, rng)
    s.hub = hot
    s.mats = None
    _setups[name] = s
    return s


def _make_stepper(s, fuse_env):
    from dolfin_navier_scipy_amd import convection, newton_picard
    mesh = s.mesh
    conv = convection.ConvectionP2(mesh.cell_vdofs, mesh.glam, mesh.area,
                                   mesh.vdim, s.inv, s.dbc, s.dbc_tab[0])
    if s.mats is None:
        pat = conv.connectivity()
        rng = np.random.default_rng(5)
        M = sps.csr_matrix((rng.standard_normal(pat.nnz), pat.indices,
                            pat.indptr), shape=pat.shape)
        M = (M + sps.diags(50.0 + rng.random(pat.shape[0]))).tocsr()
        A = sps.csr_matrix((30*rng.standard_normal(pat.nnz), pat.indices,
                            pat.indptr), shape=pat.shape)
        s.mats = (M, A)
    with env('DNS_TRAP_FUSE_R', fuse_env):
        st = newton_picard.TrapezoidalStepper(s.mats[0], s.mats[1], s.J, conv,
                                              NSLOTS, DT, precond=False)
    return conv, st


def _run(s, newton, table, fuse_env):
    conv, st = _make_stepper(s, fuse_env)
    try:
        if table:
            st.set_tables(fv_tab=s.fv_tab, fp_tab=s.fp_tab,
                          dbc_tab=s.dbc_tab if s.dbc.size else None)
        else:
            st.set_rhs(s.fv_tab[0], s.fp_tab[0])
        st.write_linpoint(0, LIN_SLOT, s.v_lin)
        st.start(s.v_c, newton)
        out = st.assembly_probe(DT, 0, LIN_SLOT, newton, x0=s.x0)
        dl = s.dbc_tab[LIN_SLOT if table else 0]
        out['assemble'] = conv.assemble(s.v_lin, newton=newton,
                                        dbcvals_lin=dl)[0].data.copy()
        out['pattern'] = (st.pattern.indptr.copy(), st.pattern.indices.copy())
        out['mvals'], out['avals'] = st.mvals.copy(), st.avals.copy()
    finally:
        st.close()
        conv.close()
    return out


@pytest.mark.parametrize('table', [False, True], ids=['const', 'table'])
@pytest.mark.parametrize('newton', [False, True], ids=['picard', 'newton'])
@pytest.mark.parametrize('name', sorted(MESHES))
def test_assembly_pair_per_entry(name, newton, table):
    s = setup_of(name)
    runs = dict((fe, _run(s, newton, table, fe)) for fe in (None, '0'))
    # a fused case cannot quietly run unfused
    assert runs[None]['fused'] is True and runs['0']['fused'] is False
    o = runs[None]
    lin, cur = (LIN_SLOT, 0) if table else (0, 0)
    ref = cm.trap_assembly_model(
        s.sp, o['pattern'], o['mvals'], o['avals'], s.J, 0.5*DT, s.v_lin,
        s.dbc_tab[lin], s.v_c, s.dbc_tab[cur], s.fv_tab[lin], s.fv_tab[cur],
        s.fp_tab[lin], s.x0, newton)
    nv = s.inv.size
    for fe, o in runs.items():
        withr = int(o['fused'])
        path = 'trap_rows<HASG=%d, WITHR=%d>' % (int(newton), withr)
        assert np.array_equal(o['x0'], s.x0)
        r = dict((k, cm.ratio(o[k], *ref[{'nvals': 'N', 'fvals': 'F'}.get(k, k)]))
                 for k in ('nvals', 'fvals', 'rhsbc', 'fvn', 'b'))
        if o['fused']:
            r['r'] = cm.ratio(o['r'], *ref['r'])
            assert o['partR'].size == o['partB'].size > 0
            r['rr'] = _note('||r||^2', cm.ratio(np.sum(o['partR'].astype(cm.LD)),
                                                *ref['rr']))
            r['bb'] = _note('||b||^2', cm.ratio(np.sum(o['partB'].astype(cm.LD)),
                                                *ref['bb']))
        print('%s %s %s %s: ' % (name, 'newton' if newton else 'picard',
                                 'table' if table else 'const', path)
              + '  '.join('%s %.3f' % kv for kv in sorted(r.items())))
        _note(path, max(r[k] for k in ('rhsbc', 'fvn', 'b')
                        + (('r',) if o['fused'] else ())))
        _note('matrix Newton' if newton else 'matrix Picard', r['nvals'])
        _note('F', r['fvals'])
        assert max(r.values()) <= 1.0, r
        # the pressure part of b is fp itself
        assert np.array_equal(o['b'][nv:], s.fp_tab[lin])
        # F sits in K as it sits in F; N is what `assemble` gives
        assert np.array_equal(o['kfvals'], o['fvals'])
        assert np.array_equal(o['nvals'], o['assemble'])
    for k in ('b', 'fvn', 'rhsbc', 'nvals', 'fvals'):
        assert np.array_equal(runs[None][k], runs['0'][k]), k
    if table and s.dbc.size:
        # the other row for N(v_c) v_c is not within the bound
        swapped = cm.trap_assembly_model(
            s.sp, o['pattern'], o['mvals'], o['avals'], s.J, 0.5*DT, s.v_lin,
            s.dbc_tab[lin], s.v_c, s.dbc_tab[lin], s.fv_tab[lin],
            s.fv_tab[cur], s.fp_tab[lin], s.x0, newton)
        assert cm.ratio(o['b'], *swapped['b']) > 1.0


def test_lists_the_cases_rely_on():
    s = setup_of('fan40-np300')
    ref_len = dict(cells=s.sp.row_len, bc=s.sp.bc_len)
    assert len(s.hub) == 2
    assert np.all(ref_len['cells'][s.hub] > 32)           # lists pg, pc
    assert np.all(ref_len['bc'][s.hub] > 200)             # list pb
    JT = s.J.T.tocsr()
    assert np.all(np.diff(JT.indptr)[s.hub] > 32)         # list pj
    code = s.sp.code
    cols = [np.unique(code[(code == h).any(axis=1)]) for h in s.hub]
    assert all((c >= 0).sum() > 32 for c in cols)         # matrix row, loop
    for name in MESHES:
        lens = np.diff(setup_of(name).J.indptr)
        assert lens.max() > 16 and (lens.min() == 0 or lens.size == 1)
    assert setup_of('nobc-np17').dbc.size == 0
    assert np.abs(s.x0[s.inv.size:]).min() > 0            # pressure part of x0
    assert not np.array_equal(s.v_c, s.v_lin)


def test_probe_refuses_a_pipelined_stepper():
    from dolfin_navier_scipy_amd import _capi
    s = setup_of('rect33-np1')
    conv, st = _make_stepper(s, None)
    try:
        st.set_rhs(s.fv_tab[0], s.fp_tab[0])
        st.write_linpoint(0, LIN_SLOT, s.v_lin)
        st.start(s.v_c, False)
        st.set_pipeline(3)
        with pytest.raises(_capi.DnsError) as ei:
            st.assembly_probe(DT, 0, LIN_SLOT, False, x0=s.x0)
        assert ei.value.status == _capi.DNS_ERR_NOT_READY
        st.set_pipeline(0)
        # without x0: the extrapolated warm start (first step: the state)
        out = st.assembly_probe(DT, 0, LIN_SLOT, False)
        assert np.array_equal(out['x0'][:s.inv.size], s.v_c)
    finally:
        st.close()
        conv.close()


def test_zz_report():
    print('largest error / bound per path: '
          + '  '.join('%s %.3f' % kv for kv in sorted(WORST.items())))
    _setups.clear()
