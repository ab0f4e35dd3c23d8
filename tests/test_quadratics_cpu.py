"""Quadratic functionals (the energy budget) of the explicit loops, host side:
the builders of `fem.quadratics` against the dense full-space statement, the
class (`+`, `scaled`, `device_args`, refusals), the entry points of the
library, and `_QuadraticLog` through the host loop of `cnab` / `sbdftwo` with
`tests/imex_host_model.py` behind it.  No device.

Bound of a form's value: `n_k 2^-52 T_k`, `T_k` the sum of the absolute values
of its `n_k` products -- the a-priori bound of a sum of fp64 products in any
order (`QuadraticFunctionals.evaluate(..., return_scale=True)`)."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import scipy.sparse as sps

import imex_host_model
import scenarios
from oracle import snu_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.**-52

NEW_SYMBOLS = ('dns_imex_set_quadratics', 'dns_imex_get_quadratics',
               'dns_imex_clear_quadratics', 'dns_imex_quadratics_grid')


def _femp(prob):
    return dict(V=prob['th'], invinds=prob['invinds'],
                dbcinds=prob['dbcinds'], dbcvals=prob['dbcvals'],
                nu=prob['nu'])


@pytest.fixture(scope='module')
def budget(toy_prob):
    from dolfin_navier_scipy_amd import fem
    femp = _femp(toy_prob)
    th = toy_prob['th']
    parts = [fem.kinetic_energy(th, femp), fem.dissipation(th, femp),
             fem.kinetic_energy_rate(th, femp), fem.rate_norm(th, femp)]
    return parts, parts[0] + parts[1] + parts[2] + parts[3]


def _states(prob, seed=0):
    rng = np.random.default_rng(seed)
    NV = np.asarray(prob['invinds']).size
    v = rng.standard_normal(NV)
    return v, v + 1e-2*rng.standard_normal(NV)


def _full(prob, v):
    return snu_oracle.append_bcs_vec(
        v, vdim=prob['th'].vdim, bcinds=prob['dbcinds'],
        bcvals=prob['dbcvals'], invinds=prob['invinds'])[:, 0]


# ---- entry points -----------------------------------------------------------------

def test_header_declares_and_capi_binds_the_quadratics_entry_points():
    from dolfin_navier_scipy_amd import _capi
    hdr = open(os.path.join(ROOT, 'include', 'dns_amd.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(dns_[a-z0-9_]+)\s*\(', hdr))
    lib = _capi.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    calls = ((lib.dns_imex_set_quadratics,
              (None, 1, None, 1, None, None, None, None, None, None, None,
               1., 4, 0)),
             (lib.dns_imex_get_quadratics, (None, 0, 1, None)),
             (lib.dns_imex_quadratics_grid, (None, None)),
             (lib.dns_imex_clear_quadratics, (None,)))
    for fn, args in calls:
        assert fn(*args) == _capi.DNS_ERR_BAD_ARGUMENT
        assert b'null' in lib.dns_last_error()


def test_quadratic_kernel_is_a_dependency_of_the_build():
    from dolfin_navier_scipy_amd import build
    names = [os.path.basename(p) for p in build.dependencies()]
    assert 'quadratic.hpp' in names
    text = open(os.path.join(ROOT, 'dolfin_navier_scipy_amd', 'csrc',
                             'imex.hpp')).read()
    assert '#include "quadratic.hpp"' in text


# ---- builders ----------------------------------------------------------------------

def test_builders_against_the_dense_full_space_statement(toy_prob, budget):
    parts, qf = budget
    th, nu = toy_prob['th'], toy_prob['nu']
    stms = th.stokes_mats(nu=nu)
    M, A = stms['M'].toarray(), stms['A'].toarray()
    dt = 1./64
    for seed in (0, 1):
        v, vp = _states(toy_prob, seed)
        u, up = _full(toy_prob, v), _full(toy_prob, vp)
        assert np.isfinite(u).all()
        d = (u - up)/dt
        want = np.array([.5*u @ M @ u, u @ A @ u, u @ M @ d, d @ M @ d])
        y, T, n = qf.evaluate(v, vp, dt, return_scale=True)
        assert y.shape == T.shape == n.shape == (4,)
        # the dense statement sums vdim^2 products of the same sizes; its own
        # rounding is inside the same bound with n = vdim^2
        bound = th.vdim**2*EPS*T
        print('builders: |evaluate - dense| / bound', np.abs(y - want)/bound)
        assert np.all(np.abs(y - want) <= bound)
        assert np.all(np.abs(want) > 1e3*bound)     # (the check means something)
        assert y[1] >= 0. and y[3] >= 0. and y[0] > 0.
        # each builder alone says what it says in the stack
        for k, part in enumerate(parts):
            assert part.nQ == 1 and part.nM == 1
            assert np.array_equal(part.evaluate(v, vp, dt), y[k:k + 1])
    assert qf.names == ['ekin', 'dissipation', 'ekin_rate', 'rate_norm']


def test_energy_identity(toy_prob, budget):
    """E(v) - E(v_prev) = dt rate - dt^2/2 rate_norm, exactly (M symmetric;
    the boundary values do not move): to the sum of the forms' bounds -- the
    energy at its two states, the rate and the norm with their factors"""
    _, qf = budget
    dt = 1./64
    v, vp = _states(toy_prob, 2)
    y, T, n = qf.evaluate(v, vp, dt, return_scale=True)
    yp, Tp, _ = qf.evaluate(vp, vp, dt, return_scale=True)
    b = n*EPS*T
    bound = b[0] + n[0]*EPS*Tp[0] + dt*b[2] + .5*dt*dt*b[3]
    lhs = y[0] - yp[0]
    rhs = dt*y[2] - .5*dt*dt*y[3]
    print('identity: |lhs - rhs| / bound', abs(lhs - rhs)/bound)
    assert abs(lhs - rhs) <= bound
    assert abs(lhs) > 1e3*bound
    assert yp[2] == 0. and yp[3] == 0.         # (w = 0: no rate)


# ---- the class ---------------------------------------------------------------------

def test_stacking_shares_a_matrix_that_is_the_same_object(toy_prob, budget):
    from dolfin_navier_scipy_amd import fem
    parts, qf = budget
    assert qf.nM == 2 and qf.nQ == 4
    assert qf.mat.tolist() == [0, 1, 0, 0]
    assert qf.lop.tolist() == [0, 0, 0, 1] and qf.rop.tolist() == [0, 0, 1, 1]
    assert qf.mats[0] is parts[0].mats[0] is parts[3].mats[0]
    both = fem.energy_budget(toy_prob['th'], _femp(toy_prob))
    assert both.nM == 2 and both.mats[0] is qf.mats[0]
    # an equal matrix that is another object is kept apart
    NV = qf.NV
    other = fem.QuadraticFunctionals.from_matrices(
        NV, [qf.mats[0].copy()], [(0, 0, 0)])
    assert (qf + other).nM == 3 and (qf + other).mat.tolist() == [0, 1, 0, 0, 2]
    with pytest.raises(ValueError):
        qf + fem.QuadraticFunctionals.from_matrices(
            3, [sps.identity(3, format='csr')], [(0, 0, 0)])


def test_device_args_layout_and_scaled(budget):
    _, qf = budget
    args = qf.device_args()
    assert set(args) == {'mats', 'mat', 'lop', 'rop', 'qa', 'qw', 'c0',
                         'scale'}
    NV = qf.NV
    assert len(args['mats']) == 2
    for m in args['mats']:
        assert sps.isspmatrix_csr(m) and m.shape == (NV, NV)
        assert m.has_canonical_format
    for k in ('mat', 'lop', 'rop'):
        assert args[k].dtype == np.int32 and args[k].shape == (4,)
        assert args[k].flags['C_CONTIGUOUS']
    assert args['qa'].shape == args['qw'].shape == (4, NV)
    assert args['qa'][0].nnz > 0 and args['qa'][2].nnz == 0
    assert args['qw'][2].nnz > 0 and args['qw'][0].nnz == 0
    assert args['c0'].dtype == args['scale'].dtype == np.float64
    assert args['scale'].tolist() == [.5, 1., 1., 1.]
    assert args['c0'][0] > 0. and args['c0'][2] == 0.
    sc = qf.scaled([2., 1., -1., 3.])
    assert sc.scale.tolist() == [1., 1., -1., 3.]
    assert sc.mats[0] is qf.mats[0] and qf.scale.tolist() == [.5, 1., 1., 1.]
    rng = np.random.default_rng(5)
    v, vp = rng.standard_normal(NV), rng.standard_normal(NV)
    y, T, n = qf.evaluate(v, vp, .5, return_scale=True)
    ys, Ts, ns = sc.evaluate(v, vp, .5, return_scale=True)
    assert np.array_equal(ys, np.array([2., 1., -1., 3.])*y)
    assert np.array_equal(Ts, np.array([2., 1., 1., 3.])*T)
    assert np.array_equal(ns, n)
    assert qf.scaled(2.).scale.tolist() == [1., 2., 2., 2.]
    with pytest.raises(ValueError):
        qf.scaled([1., 2.])


def test_evaluate_of_a_general_matrix_with_rows_and_constants():
    """a non-symmetric matrix, both operands, `qa`, `qw`, `c0`, `scale`: the
    formula, entry by entry"""
    from dolfin_navier_scipy_amd.fem import QuadraticFunctionals
    R = sps.csr_matrix(np.array([[1., 2., 0.], [0., 0., 0.], [-3., 0., 4.]]))
    qa = sps.csr_matrix(np.array([[1., 0., -1.], [0., 0., 0.]]))
    qw = sps.csr_matrix(np.array([[0., 0., 0.], [0., 2., 0.]]))
    qf = QuadraticFunctionals.from_matrices(
        3, [R], [(0, 0, 0), (0, 1, 0)], qa=qa, qw=qw, c0=[.25, -1.],
        scale=[.5, 2.], names=['a', 'b'])
    v, vp, dt = np.array([1., 2., 3.]), np.array([0., 4., 2.]), .5
    w = v - vp
    Rv = np.array([5., 0., 9.])
    want = [.5*(v @ Rv + (1. - 3.) + .25),
            2.*((w @ Rv)/dt + (2.*w[1])/dt - 1.)]
    y, T, n = qf.evaluate(v, vp, dt, return_scale=True)
    assert np.allclose(y, want, rtol=1e-15, atol=0)
    assert n.tolist() == [4 + 2 + 0 + 1, 4 + 0 + 1 + 1]
    absRv = np.array([1. + 4., 0., 3. + 12.])
    assert np.allclose(T, [.5*(np.abs(v) @ absRv + 1. + 3. + .25),
                           2.*((np.abs(w) @ absRv)/dt + 4./dt + 1.)],
                       rtol=1e-15, atol=0)
    # a state handed over as a column, longer than NV: the head counts
    assert np.array_equal(qf.evaluate(np.r_[v, 9.].reshape((-1, 1)), vp, dt),
                          y)


def test_shape_refusals_in_python():
    from dolfin_navier_scipy_amd import saddle
    from dolfin_navier_scipy_amd.fem import QuadraticFunctionals
    eye = sps.identity(4, format='csr')
    make = QuadraticFunctionals.from_matrices
    with pytest.raises(ValueError):                  # not NV x NV
        make(5, [eye], [(0, 0, 0)])
    with pytest.raises(ValueError):                  # no matrix / no form
        make(4, [], [(0, 0, 0)])
    with pytest.raises(ValueError):
        make(4, [eye], [])
    with pytest.raises(ValueError):                  # matrix index
        make(4, [eye], [(1, 0, 0)])
    with pytest.raises(ValueError):                  # operand
        make(4, [eye], [(0, 2, 0)])
    with pytest.raises(ValueError):                  # rows not NV wide
        make(4, [eye], [(0, 0, 0)], qa=sps.csr_matrix((1, 5)))
    with pytest.raises(ValueError):                  # one row per form
        make(4, [eye], [(0, 0, 0)], qw=sps.csr_matrix((2, 4)))
    with pytest.raises(ValueError):
        make(4, [eye], [(0, 0, 0)], c0=[1., 2.])
    with pytest.raises(ValueError):
        make(4, [eye], [(0, 0, 0)], names=['a', 'b'])
    # the stepper's own checks come before the library is called
    stp = saddle.ImexStepper.__new__(saddle.ImexStepper)
    stp.sys = types.SimpleNamespace(NV=7, NP=3)
    stp.lib = stp._h = None
    qf = make(4, [eye], [(0, 0, 0)])
    with pytest.raises(ValueError) as exc:
        stp.set_quadratics(qf, 4, .1)
    assert 'NV x NV' in str(exc.value)
    with pytest.raises(ValueError):
        stp.set_quadratics(qf, 0, .1)
    with pytest.raises(ValueError):                  # nothing was set
        stp.get_quadratics()


# ---- through the host loop ---------------------------------------------------------

class QuadStepper(imex_host_model.HostStepper):
    """the host model with the quadratics' log: a row per step after
    `set_quadratics`, `qf.evaluate` of the state the step leaves"""

    def set_quadratics(self, qf, nrows, dt, max_grid=None):
        self.qd = (qf, int(nrows), dt)
        self.qrows = []
        self.armed = getattr(self, 'armed', 0) + 1

    def step(self, cf, nfc_new=None, opts=None):
        imex_host_model.HostStepper.step(self, cf, nfc_new=nfc_new, opts=opts)
        if getattr(self, 'qd', None) is not None:
            qf, nrows, dt = self.qd
            assert len(self.qrows) < nrows, 'stepped past the last row'
            self.qrows.append(qf.evaluate(self.v_c, self.v_p, dt))

    def get_quadratics(self, first=0, count=None):
        rows = np.array(self.qrows).reshape((-1, self.qd[0].nQ))
        count = rows.shape[0] - first if count is None else count
        assert first + count <= rows.shape[0]
        return rows[first:first + count]


@pytest.fixture
def tiu(monkeypatch):
    mod = imex_host_model.install(monkeypatch)
    monkeypatch.setattr(mod, 'ImexStepper', QuadStepper)
    return mod


def _run(tiu, scheme, kw):
    kw = dict(kw)
    if scheme == 'sbdf2':
        kw.pop('f_tvdp', None)
        return tiu.sbdftwo(**kw)
    return tiu.cnab(**kw)


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_quadratic_log_through_the_host_loop(tiu, toy_prob, budget, scheme):
    _, qf = budget
    inv = toy_prob['invinds']
    got = {}
    for path in ('stepwise', 'resident'):
        kw, rec, _ = scenarios.build(variant='plain', seed=0, prob=toy_prob)
        if path == 'resident':
            conv = imex_host_model.StubConvection(kw.pop('f_vdp'),
                                                  kw['appndbcs'])
            kw.update(device_convection=conv, invinds=inv,
                      resident=dict(quadratics=qf))
        else:
            kw.update(resident=dict(quadratics=qf))
        _, _, ff = _run(tiu, scheme, kw)
        assert ff == 0
        got[path] = (dict(tiu.LAST_RUN), rec.arrays(), kw['trange'])
    dt = got['stepwise'][2][1] - got['stepwise'][2][0]
    for path, where in (('stepwise', 'host'), ('resident', 'device')):
        lr, (times, vels, prss), trange = got[path]
        assert lr['quadratics_on'] == where
        assert lr['quadratics_names'] == qf.names
        assert lr['quadratics'].shape == (11, 4)
        assert np.array_equal(lr['quadratics_t'], np.asarray(trange[2:]))
        assert (lr['run_calls'] > 0) == (path == 'resident')
        # the rows are the forms of the states `savevp` saw
        for r in range(11):
            want = qf.evaluate(vels[r + 2][inv], vels[r + 1][inv], dt)
            assert np.array_equal(lr['quadratics'][r], want), (path, r)
    # armed once per slice that has steps
    stepper = imex_host_model.HostStepper.made[-1]
    slices = [s for s in tiu._inittimegrid(got['resident'][2], 10)[1] if s]
    assert stepper.armed == len(slices)


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_moving_boundaries_are_refused_on_both_paths(tiu, toy_prob, budget,
                                                     scheme):
    _, qf = budget
    for path in ('stepwise', 'resident'):
        kw, rec, _ = scenarios.build(variant='movingbc', seed=2,
                                     prob=toy_prob)
        if path == 'resident':
            conv = imex_host_model.StubConvection(kw.pop('f_vdp'),
                                                  kw['appndbcs'])
            kw.update(device_convection=conv, invinds=toy_prob['invinds'],
                      resident=dict(bcs_time_only=True, quadratics=qf))
        else:
            kw.update(resident=dict(quadratics=qf))
        with pytest.raises(ValueError) as exc:
            _run(tiu, scheme, kw)
        assert 'moving Dirichlet' in str(exc.value)


def test_last_run_has_no_quadratics_keys_without_them(tiu, toy_prob):
    kw, rec, _ = scenarios.build(variant='plain', seed=0, prob=toy_prob)
    tiu.cnab(**kw)
    assert not [k for k in tiu.LAST_RUN if k.startswith('quadratics')]


def test_solve_nse_passes_it_on_and_refuses_non_explicit_schemes(toy_prob,
                                                                 budget):
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    _, qf = budget
    sig = inspect.signature(snu.solve_nse)
    assert sig.parameters['quadratics'].default is None
    with pytest.raises(NotImplementedError) as exc:
        snu.solve_nse(quadratics=qf, treat_nonl_explicit=False)
    assert 'quadratics' in str(exc.value)
