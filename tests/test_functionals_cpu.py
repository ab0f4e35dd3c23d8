"""Host side of the force functionals (`fem.functionals`): the NumPy statement
`MomentumFunctionals.evaluate` against the un-condensed momentum balance,
against the `CylinderForces` of `scripts/schaefer_turek_unsteady.py`, the
pressure difference, the cells a test vector reaches, and the time bookkeeping
of `LAST_RUN['functionals_t']`.

Shapes: the reference's `cylinder_1` mesh (NV = 5812, NP = 806, 1501 cells; the
cylinder has 36 nodes and 39 cells).  Tolerance: `1e-12 * T_k`, `T_k` the sum
of the absolute values of every product of functional k (`evaluate(...,
return_scale=True)`): both sides are fp64 sums of a few thousand products.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

TOL = 1e-12


@pytest.fixture(scope='module')
def cyl1():
    from dolfin_navier_scipy_amd import fem
    femp, sm, rhsd = fem.get_sysmats(problem='cylinderwake', N=1, Re=100.)
    th = femp['V']
    rng = np.random.default_rng(11)
    NP, NV = sm['J'].shape
    state = dict(v=rng.standard_normal(NV), vp=rng.standard_normal(NV),
                 p=rng.standard_normal(NP), dt=1./256)
    return dict(femp=femp, sm=sm, th=th, state=state, NV=NV, NP=NP,
                stms=th.stokes_mats(nu=femp['nu']))


def _full(c, v):
    femp, th = c['femp'], c['th']
    w = np.zeros(th.vdim)
    w[femp['dbcinds']] = np.asarray(femp['dbcvals']).reshape(-1)
    w[femp['invinds']] = v
    return w


def _direct(c, phi, v, vp, p, dt):
    """`-phi^T (M (w - w_prev)/dt + A w + N(w) w - JT p)`, un-condensed"""
    st, th = c['stms'], c['th']
    w, wp = _full(c, v), _full(c, vp)
    res = st['M'] @ ((w - wp)/dt) + st['A'] @ w \
        + th.convection_vec(w)[:, 0] - st['JT'] @ p
    return -float(phi @ res)


def _bump(th, radius=0.12, center=(0.2, 0.2)):
    """a smooth patch about the cylinder centre, both components"""
    xy = th.nodecoords
    r2 = ((xy - np.asarray(center)[None, :])**2).sum(axis=1)/radius**2
    b = np.where(r2 < 1., (1. - np.minimum(r2, 1.))**2, 0.)
    phi = np.zeros(th.vdim)
    phi[0::2] = b
    phi[1::2] = -.5*b
    return phi


def test_shapes_of_cylinder_1(cyl1):
    from dolfin_navier_scipy_amd import fem
    th = cyl1['th']
    assert (cyl1['NV'], cyl1['NP'], th.mesh.ncells) == (5812, 806, 1501)
    fn = fem.boundary_forces(th, cyl1['femp'])
    assert fem.cylinder_nodes(th).size == 36
    assert fn.cells[0].size == fn.cells[1].size == 39
    assert fn.nF == 2 and fn.names == ['fx', 'fy']


def test_evaluate_against_the_uncondensed_balance(cyl1):
    from dolfin_navier_scipy_amd import fem
    th, femp, s = cyl1['th'], cyl1['femp'], cyl1['state']
    nodes = fem.cylinder_nodes(th)
    phis = np.zeros((th.vdim, 4))
    phis[2*nodes, 0] = 1.
    phis[2*nodes + 1, 1] = 1.
    phis[:, 2] = _bump(th)
    # torque about the centre: phi = (-(y - yc), x - xc) on the body's nodes
    xy = th.nodecoords[nodes]
    phis[2*nodes, 3] = -(xy[:, 1] - 0.2)
    phis[2*nodes + 1, 3] = xy[:, 0] - 0.2
    fn = fem.MomentumFunctionals(th, femp, phis,
                                 names=['fx', 'fy', 'bump', 'torque'])
    assert fn.cells[2].size > 100
    y, T = fn.evaluate(s['v'], s['vp'], s['p'], s['dt'], return_scale=True)
    for k in range(4):
        ref = _direct(cyl1, phis[:, k], s['v'], s['vp'], s['p'], s['dt'])
        print(fn.names[k], y[k], ref, abs(y[k] - ref)/T[k])
        assert abs(y[k] - ref) <= TOL*T[k], (k, y[k], ref, T[k])
    assert np.all(T > np.abs(y))
    # the terms matter: each of them moves the value by more than the bound
    y2 = fn.evaluate(s['v'], s['v'], s['p'], s['dt'])
    y3 = fn.evaluate(s['v'], s['vp'], 0*s['p'], s['dt'])
    assert np.all(np.abs(y2 - y) > 1e-6*T) and np.all(np.abs(y3 - y) > 1e-6*T)


def test_reproduces_the_cylinder_forces_of_the_script(cyl1):
    from dolfin_navier_scipy_amd import fem
    import schaefer_turek_unsteady as stu
    th, femp, s = cyl1['th'], cyl1['femp'], cyl1['state']
    forces = stu.CylinderForces(femp, th)
    fx, fy = forces(s['v'], (s['v'] - s['vp'])/s['dt'], s['p'])
    fn = fem.boundary_forces(th, femp)
    y, T = fn.evaluate(s['v'], s['vp'], s['p'], s['dt'], return_scale=True)
    assert abs(y[0] - fx) <= TOL*T[0] and abs(y[1] - fy) <= TOL*T[1]
    assert np.array_equal(np.sort(fn.cells[0]), np.sort(forces.cells))
    # the steady force: no `M dv/dt`
    ys = fn.without_rate().evaluate(s['v'], s['vp'], s['p'], s['dt'])
    assert np.array_equal(ys, fn.evaluate(s['v'], s['v'], s['p'], s['dt']))
    # coefficients: the scale carries the factor
    cf = fn.scaled(2./((2./3)**2*0.1))
    assert np.allclose(cf.evaluate(s['v'], s['vp'], s['p'], s['dt']),
                       y*2./((2./3)**2*0.1), rtol=1e-15, atol=0)


def test_pressure_difference_and_stacking(cyl1):
    from dolfin_navier_scipy_amd import fem
    th, femp, s = cyl1['th'], cyl1['femp'], cyl1['state']
    dp = fem.pressure_difference(th, (0.15, 0.2), (0.25, 0.2))
    a = int(np.flatnonzero(dp.cp.toarray()[0] == 1.)[0])
    b = int(np.flatnonzero(dp.cp.toarray()[0] == -1.)[0])
    va = th.mesh.verts[np.flatnonzero(th.vert_pdof == a)[0]]
    vb = th.mesh.verts[np.flatnonzero(th.vert_pdof == b)[0]]
    assert np.allclose(va, (0.15, 0.2), atol=1e-12)
    assert np.allclose(vb, (0.25, 0.2), atol=1e-12)
    assert dp.evaluate(s['v'], s['vp'], s['p'], s['dt'])[0] == \
        s['p'][a] - s['p'][b]
    assert fem.pressure_difference(th, a, b).cp.nnz == 2
    fn = fem.boundary_forces(th, femp) + dp
    assert fn.nF == 3 and fn.names == ['fx', 'fy', 'dp']
    y = fn.evaluate(s['v'], s['vp'], s['p'], s['dt'])
    y2 = fem.boundary_forces(th, femp).evaluate(s['v'], s['vp'], s['p'],
                                                s['dt'])
    assert np.array_equal(y[:2], y2) and y[2] == s['p'][a] - s['p'][b]
    args = fn.device_args()
    assert args['cell_ptr'].tolist() == [0, 39, 78, 78]
    assert args['cell_w'].size == 12*78 and args['ca'].shape == (3, 5812)
    assert (dp + fem.boundary_forces(th, femp)).names == ['dp', 'fx', 'fy']


def test_a_single_dof_picks_out_its_cells(cyl1):
    from dolfin_navier_scipy_amd import fem
    th, femp = cyl1['th'], cyl1['femp']
    node = int(th.cellnodes[700, 4])
    phi = np.zeros((th.vdim, 1))
    phi[2*node + 1, 0] = 2.5
    fn = fem.MomentumFunctionals(th, femp, phi)
    want = np.where((th.cellnodes == node).any(axis=1))[0]
    assert np.array_equal(fn.cells[0], want) and want.size >= 1
    w = fn.weights[0]
    assert w.shape == (want.size, 12)
    assert np.all((w != 0).sum(axis=1) == 1) and np.all(w.sum(axis=1) == 2.5)
    for row, c in zip(w, want):
        a = int(np.flatnonzero(th.cellnodes[c] == node)[0])
        assert row[2*a + 1] == 2.5
    s = cyl1['state']
    y, T = fn.evaluate(s['v'], s['vp'], s['p'], s['dt'], return_scale=True)
    ref = _direct(cyl1, phi[:, 0], s['v'], s['vp'], s['p'], s['dt'])
    assert abs(y[0] - ref) <= TOL*T[0]


def test_times_of_the_rows_for_slices_that_do_not_divide():
    """the rows cover `trange[2:]` in order, whatever the slices.

    This drives `_FunctionalLog`, which `cnab` / `sbdftwo` fill slice by
    slice, with the slices of `_inittimegrid` by hand: the loops themselves
    need a device for their solves (also where the rows are evaluated on the
    host), so `LAST_RUN['functionals_t']` as they leave it is checked in
    `tests/test_gpu_functionals.py::test_through_the_time_loops`."""
    from dolfin_navier_scipy_amd import time_int_utils as tiu
    trange = np.linspace(0., 0.23, 24)
    for nsl in (1, 4, 5, 10, 30):
        _, slices = tiu._inittimegrid(trange, ntimeslices=nsl)
        log = tiu._FunctionalLog(None, None, 1.)
        for ctrange in slices:
            if len(ctrange):
                log.add(np.zeros((len(ctrange), 2)), ctrange)
        y, t = log.result()
        assert y.shape == (22, 2)
        assert np.array_equal(t, trange[2:])
    # nothing ran: empty, with the right width unknown -> zero columns
    y, t = tiu._FunctionalLog(None, None, 1.).result()
    assert y.shape[0] == 0 and t.size == 0
