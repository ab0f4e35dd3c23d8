"""Quadratic functionals with moving Dirichlet values, host side: the
full-space instances of `fem.quadratics` (`ndbc > 0`, the builders'
`moving=True`, `evaluate(..., dbc=, dbc_prev=)`) against the dense statement on
the scattered full vectors, against the constant-value builders where the
values do not move, the class (`+`, `device_args`), the three new entry points
of the library, and `_QuadraticLog` through the host loop of `cnab` /
`sbdftwo` on the `movingbc` scenario.  No device.

Shapes: `scenarios.toy_problem()` (NV = 1286, NP = 207, 240 Dirichlet dofs, 30
of them on the obstacle); the Dirichlet dofs ordered static first, the
obstacle's behind them (`rotating_split`, `moving_femp` of
`tests/test_functionals_bc_cpu.py`).

Bound of a form's value: `n_k 2^-52 T_k`, `T_k` the sum of the absolute values
of its `n_k` products, boundary products included -- the a-priori bound of a
sum of fp64 products in any order (`evaluate(..., return_scale=True)`).  The
dense statement is formed in `np.longdouble`: its own rounding is 2^-11 of
that."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sps

import imex_host_model
import scenarios
from test_functionals_bc_cpu import moving_femp, rotating_split, rotation
from test_quadratics_cpu import QuadStepper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.**-52
LD = np.longdouble

NEW_SYMBOLS = ('dns_imex_set_quadratics_bc', 'dns_imex_set_quadratics_live',
               'dns_imex_set_functionals_live')
NAMES = ['ekin', 'dissipation', 'ekin_rate', 'rate_norm']


@pytest.fixture(scope='module')
def mov(toy_prob):
    from dolfin_navier_scipy_amd import fem
    prob, th = toy_prob, toy_prob['th']
    statinds, statvals, cntinds, nodes = rotating_split(prob)
    femp = moving_femp(prob, statinds, cntinds, statvals,
                       rotation(th, nodes, 1.))
    parts = [fem.kinetic_energy(th, femp, moving=True),
             fem.dissipation(th, femp, moving=True),
             fem.kinetic_energy_rate(th, femp, moving=True),
             fem.rate_norm(th, femp, moving=True)]
    inv = np.asarray(prob['invinds'])
    dbi = np.asarray(femp['dbcinds'])
    assert (inv.size, dbi.size, cntinds.size) == (1286, 240, 30)
    return dict(prob=prob, th=th, femp=femp, parts=parts,
                qf=parts[0] + parts[1] + parts[2] + parts[3], inv=inv,
                dbi=dbi, nodes=nodes, nstat=statinds.size)


def _states(mov, seed):
    """inner velocities and Dirichlet values of two states; the obstacle's
    values move, the static ones keep theirs"""
    rng = np.random.default_rng(seed)
    NV = mov['inv'].size
    v = rng.standard_normal(NV)
    vp = v + 1e-2*rng.standard_normal(NV)
    g = np.array(mov['femp']['dbcvals'], dtype=np.float64)
    gp = g.copy()
    g[mov['nstat']:] = rotation(mov['th'], mov['nodes'], 1.3)
    gp[mov['nstat']:] = rotation(mov['th'], mov['nodes'], 0.9)
    return v, vp, g, gp


def _scatter(mov, v, g):
    u = np.zeros(mov['th'].vdim)
    u[mov['inv']] = v
    u[mov['dbi']] = g
    return u


# ---- entry points -----------------------------------------------------------------

def test_header_declares_and_capi_binds_the_new_entry_points():
    from dolfin_navier_scipy_amd import _capi
    hdr = open(os.path.join(ROOT, 'include', 'dns_amd.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(dns_[a-z0-9_]+)\s*\(', hdr))
    lib = _capi.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    quad = (None, 1, None, 1, None, None, None, None, None, None, None, 1., 4,
            0)
    func = (None, 1, None, None, None, None, None, None, None, None, None,
            None, 1., 4)
    for fn, args in ((lib.dns_imex_set_quadratics_bc, quad + (3, None)),
                     (lib.dns_imex_set_quadratics_live, quad + (3,)),
                     (lib.dns_imex_set_functionals_live, func + (3,))):
        assert fn(*args) == _capi.DNS_ERR_BAD_ARGUMENT
        assert b'null' in lib.dns_last_error()


# ---- builders ----------------------------------------------------------------------

def test_moving_builders_against_the_dense_full_space_statement(mov):
    th, qf, parts = mov['th'], mov['qf'], mov['parts']
    stms = th.stokes_mats(nu=mov['prob']['nu'])
    M, A = (stms[k].toarray().astype(LD) for k in 'MA')
    dt = 1./64
    assert qf.names == NAMES and qf.ndbc == 240 and qf.NV == 1286
    assert qf.qa.nnz == 0 and qf.qw.nnz == 0 and not qf.c0.any()
    for seed in (0, 1):
        v, vp, g, gp = _states(mov, seed)
        u = _scatter(mov, v, g).astype(LD)
        up = _scatter(mov, vp, gp).astype(LD)
        d = (u - up)/LD(dt)
        want = np.array([LD(.5)*(u @ M @ u), u @ A @ u, u @ M @ d,
                         d @ M @ d])
        y, T, n = qf.evaluate(v, vp, dt, return_scale=True, dbc=g,
                              dbc_prev=gp)
        assert y.shape == T.shape == n.shape == (4,)
        bound = n*EPS*T
        frac = np.abs((y.astype(LD) - want).astype(np.float64))/bound
        print('moving builders: |evaluate - dense| / (n 2^-52 T)', frac)
        assert np.all(frac <= 1.)
        assert np.all(np.abs(want.astype(np.float64)) > 1e3*bound)
        # the boundary part counts: the inner blocks alone say something else
        inner = qf.evaluate(v, vp, dt, dbc=0*g, dbc_prev=0*gp)
        assert np.all(np.abs(inner - y) > 1e3*bound)
        # ... and so does `g - g_prev` in the two rates
        still = qf.evaluate(v, vp, dt, dbc=g, dbc_prev=g)
        assert np.all(np.abs(still - y)[2:] > 1e3*bound[2:])
        assert np.array_equal(still[:2], y[:2])
        for k, part in enumerate(parts):
            assert part.nQ == 1 and part.nM == 1 and part.ndbc == 240
            assert np.array_equal(
                part.evaluate(v, vp, dt, dbc=g, dbc_prev=gp), y[k:k + 1])
    # `T`, `n` count the boundary products
    nnz = [m.nnz for m in qf.mats]
    assert n.tolist() == [nnz[0] + 1, nnz[1] + 1, nnz[0] + 1, nnz[0] + 1]
    with pytest.raises(ValueError):
        qf.evaluate(v, vp, dt)
    with pytest.raises(ValueError):
        qf.evaluate(v, vp, dt, dbc=g[:-1], dbc_prev=gp[:-1])


def test_constant_values_give_the_constant_builders(mov):
    """`g == g_prev == femp['dbcvals']`: both instances state the same sums,
    each within its own bound of the exact value"""
    from dolfin_navier_scipy_amd import fem
    th, femp = mov['th'], mov['femp']
    const = fem.energy_budget(th, femp)
    assert const.ndbc == 0 and 'ndbc' not in const.device_args()
    g = np.asarray(femp['dbcvals'], dtype=np.float64)
    assert np.abs(g[mov['nstat']:]).max() > 1e-2      # (the obstacle turns)
    dt = 1./64
    for seed in (2, 3):
        v, vp, _, _ = _states(mov, seed)
        y0, T0, n0 = const.evaluate(v, vp, dt, return_scale=True)
        y1, T1, n1 = mov['qf'].evaluate(v, vp, dt, return_scale=True, dbc=g,
                                        dbc_prev=g)
        tol = n0*EPS*T0 + n1*EPS*T1
        print('moving against constant builders, in units of the two bounds',
              np.abs(y1 - y0)/tol)
        assert np.all(np.abs(y1 - y0) <= tol)
        assert np.all(np.abs(y0) > 1e3*tol)


# ---- the class ---------------------------------------------------------------------

def test_stacking_shares_matrices_and_refuses_mixed_widths(mov):
    from dolfin_navier_scipy_amd import fem
    th, femp, qf, parts = mov['th'], mov['femp'], mov['qf'], mov['parts']
    assert qf.nM == 2 and qf.nQ == 4 and qf.mat.tolist() == [0, 1, 0, 0]
    assert qf.mats[0] is parts[0].mats[0] is parts[2].mats[0] \
        is parts[3].mats[0]
    both = fem.energy_budget(th, femp, moving=True)
    assert both.nM == 2 and both.mats[0] is qf.mats[0] \
        and both.mats[1] is qf.mats[1]
    # (other values on the same dofs: the same matrices, nothing is folded in)
    other = fem.kinetic_energy(th, dict(femp, dbcvals=0*femp['dbcvals']),
                               moving=True)
    assert other.mats[0] is qf.mats[0]
    assert qf.mats[0].shape == (1526, 1526)
    perm = np.concatenate([mov['inv'], mov['dbi']])
    M = sps.csr_matrix(th.stokes_mats(nu=mov['prob']['nu'])['M'])
    assert abs(qf.mats[0] - M[perm][:, perm]).max() == 0.
    args = qf.device_args()
    assert args['ndbc'] == 240
    assert args['qa'].shape == args['qw'].shape == (4, 1526)
    assert qf.scaled(2.).ndbc == 240 and (qf + qf).ndbc == 240
    const = fem.energy_budget(th, femp)
    for a, b in ((qf, const), (const, qf), (parts[3], const.scaled(2.))):
        with pytest.raises(ValueError) as exc:
            a + b
        assert 'ndbc' in str(exc.value)
    make = fem.QuadraticFunctionals.from_matrices
    with pytest.raises(ValueError):                  # NV x NV with ndbc
        make(4, [sps.identity(4, format='csr')], [(0, 0, 0)], ndbc=2)
    with pytest.raises(ValueError):                  # rows not NV + ndbc wide
        make(4, [sps.identity(6, format='csr')], [(0, 0, 0)], ndbc=2,
             qa=sps.csr_matrix((1, 4)))
    small = make(4, [sps.identity(6, format='csr')], [(0, 0, 1)], ndbc=2,
                 qa=sps.csr_matrix(np.arange(6.).reshape((1, 6))))
    v, vp = np.arange(4.), np.ones(4)
    y = small.evaluate(v, vp, .5, dbc=[2., 3.], dbc_prev=[1., 5.])
    u, d = np.r_[v, 2., 3.], np.r_[v - vp, 1., -2.]
    assert y[0] == (u @ d)/.5 + np.arange(6.) @ u


# ---- through the host loop ---------------------------------------------------------

class QuadBcStepper(QuadStepper):
    """the host model's quadratics with a table of Dirichlet values: row `s`
    of the log is `qf.evaluate` with the rows `s + 1`, `s` of the table"""

    def set_quadratics(self, qf, nrows, dt, max_grid=None, dbc_table=None):
        QuadStepper.set_quadratics(self, qf, nrows, dt, max_grid=max_grid)
        self.qtab = None if dbc_table is None else np.array(dbc_table)
        if qf.ndbc > 0:
            assert self.qtab.shape == (nrows + 1, qf.ndbc)

    def step(self, cf, nfc_new=None, opts=None):
        imex_host_model.HostStepper.step(self, cf, nfc_new=nfc_new, opts=opts)
        if getattr(self, 'qd', None) is not None:
            qf, nrows, dt = self.qd
            r = len(self.qrows)
            assert r < nrows, 'stepped past the last row'
            kw = {} if self.qtab is None else dict(dbc=self.qtab[r + 1],
                                                   dbc_prev=self.qtab[r])
            self.qrows.append(qf.evaluate(self.v_c, self.v_p, dt, **kw))


@pytest.fixture
def tiu(monkeypatch):
    mod = imex_host_model.install(monkeypatch)
    monkeypatch.setattr(mod, 'ImexStepper', QuadBcStepper)
    return mod


def _run(tiu, scheme, kw):
    kw = dict(kw)
    if scheme == 'sbdf2':
        kw.pop('f_tvdp', None)
        return tiu.sbdftwo(**kw)
    return tiu.cnab(**kw)


def _inflow_budget(prob):
    """the moving energy budget of the `movingbc` scenario: its controlled
    dofs are the inflow's, the loop has no other Dirichlet values (the rest
    are zero and stay out)"""
    from dolfin_navier_scipy_amd import fem
    dbcinds, dbcvals = (np.asarray(prob[k]) for k in ('dbcinds', 'dbcvals'))
    cnt = dbcinds[np.abs(dbcvals) > 0]
    femp = dict(invinds=prob['invinds'], nu=prob['nu'], dbcinds=cnt,
                dbcvals=dbcvals[np.abs(dbcvals) > 0])
    return fem.energy_budget(prob['th'], femp, moving=True), cnt


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_moving_quadratic_log_through_the_host_loop(tiu, toy_prob, scheme):
    qf, cnt = _inflow_budget(toy_prob)
    inv = toy_prob['invinds']
    assert qf.ndbc == cnt.size > 0
    got = {}
    for path in ('stepwise', 'resident'):
        kw, rec, _ = scenarios.build(variant='movingbc', seed=2,
                                     prob=toy_prob)
        if path == 'resident':
            conv = imex_host_model.StubConvection(kw.pop('f_vdp'),
                                                  kw['appndbcs'])
            kw.update(device_convection=conv, invinds=inv,
                      resident=dict(bcs_time_only=True, quadratics=qf))
        else:
            kw.update(resident=dict(quadratics=qf))
        _, _, ff = _run(tiu, scheme, kw)
        assert ff == 0
        got[path] = (dict(tiu.LAST_RUN), rec.arrays(), kw['trange'])
    dt = got['stepwise'][2][1] - got['stepwise'][2][0]
    for path, where in (('stepwise', 'host'), ('resident', 'device')):
        lr, (times, vels, prss), trange = got[path]
        assert lr['quadratics_on'] == where
        assert lr['quadratics_names'] == NAMES
        assert lr['quadratics'].shape == (11, 4)
        assert np.array_equal(lr['quadratics_t'], np.asarray(trange[2:]))
        assert (lr['run_calls'] > 0) == (path == 'resident')
        # the rows are the forms of the states `savevp` saw, with the values
        # it was handed on the controlled dofs
        assert np.abs(vels[3][cnt] - vels[2][cnt]).max() > 1e-3
        for r in range(11):
            want = qf.evaluate(vels[r + 2][inv], vels[r + 1][inv], dt,
                               dbc=vels[r + 2][cnt], dbc_prev=vels[r + 1][cnt])
            assert np.array_equal(lr['quadratics'][r], want), (path, r)
    # the two paths: the same rows
    assert np.array_equal(got['stepwise'][1][1], got['resident'][1][1])
    assert np.array_equal(got['stepwise'][0]['quadratics'],
                          got['resident'][0]['quadratics'])


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_constant_instances_and_other_widths_are_still_refused(tiu, toy_prob,
                                                               scheme):
    from dolfin_navier_scipy_amd import fem
    prob = toy_prob
    const = fem.energy_budget(prob['th'], dict(
        invinds=prob['invinds'], nu=prob['nu'], dbcinds=prob['dbcinds'],
        dbcvals=prob['dbcvals']))
    qf, cnt = _inflow_budget(prob)
    narrow = fem.kinetic_energy(prob['th'], dict(
        invinds=prob['invinds'], nu=prob['nu'], dbcinds=cnt[:-1],
        dbcvals=np.zeros(cnt.size - 1)), moving=True)
    for bad, words in ((const, ('moving Dirichlet',)),
                       (narrow, ('`quadratics`', str(cnt.size - 1),
                                 str(cnt.size)))):
        for path in ('stepwise', 'resident'):
            kw, rec, _ = scenarios.build(variant='movingbc', seed=2,
                                         prob=prob)
            if path == 'resident':
                conv = imex_host_model.StubConvection(kw.pop('f_vdp'),
                                                      kw['appndbcs'])
                kw.update(device_convection=conv, invinds=prob['invinds'],
                          resident=dict(bcs_time_only=True, quadratics=bad))
            else:
                kw.update(resident=dict(quadratics=bad))
            with pytest.raises(ValueError) as exc:
                _run(tiu, scheme, kw)
            for word in words:
                assert word in str(exc.value), (word, str(exc.value))
    # a moving instance in a loop whose boundary values do not move
    kw, rec, _ = scenarios.build(variant='plain', seed=0, prob=prob)
    kw.update(resident=dict(quadratics=qf))
    with pytest.raises(ValueError) as exc:
        _run(tiu, scheme, kw)
    assert '`quadratics`' in str(exc.value)
