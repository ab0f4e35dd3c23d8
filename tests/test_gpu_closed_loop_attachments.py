"""Forces and energy budget of a flow under boundary feedback, device resident:
`functionals` and `quadratics` beside a resident `BoundaryFeedback`
(`dns_imex_set_functionals_live` / `dns_imex_set_quadratics_live`: the two
kernels read the convection operator's Dirichlet table, where `k_lti_bc_step`
writes the controlled values), through `cnab` / `sbdftwo` and `solve_nse`.

The controlled toy problem of `test_gpu_boundary_feedback.py` (the 22 x 8
channel, NV = 1286, NP = 207, 240 Dirichlet dofs; its inflow dofs follow the
observer, the other Dirichlet dofs -- the obstacle's 30 among them -- are
static); the functionals are drag, lift and torque of the obstacle and a
momentum balance at the inflow (it reaches the controlled dofs), the
quadratics `energy_budget(moving=True)`.  24 loop steps (`Nts=25`) in three
slices of 8.

Every row against the NumPy statements on the states the device recorded and
the Dirichlet values it wrote (`LAST_RUN['feedback_bcs']`, the static values
in front): functionals within `1e-11 T_k` (the tolerance and reasoning of
`test_gpu_functionals_bc.py`), quadratics within `n_k 2^-52 T_k` (the a-priori
bound of `test_gpu_quadratics.py`).

Rows of runs that are cut into other `run` calls (one slice against three,
chunks of the recorder) are compared bit for bit wherever the two states of
the row are the same bits in both runs: the rows are functions of the states
and the table, and `test_one_slice_three_slices_and_the_same_call_twice`
documents that states of differently cut runs agree within 1e-8, not bit for
bit.  Every such row is still held to the bounds above on its own states.

Measured on the MI355X: functionals at most 5.0e-5 of `1e-11 T_k`, quadratics
at most 3.0e-4 of `n_k 2^-52 T_k`; with the Dirichlet values frozen at their
first row the same comparison is off by factors 1e6 - 1e9.  Three slices
against one: the states of 8 of the 24 rows are the same bits (the first
slice), against two chunks per slice 12 of 24; those rows are bit equal.
"""
import numpy as np
import pytest

import boundary_feedback_setup as bs
from test_functionals_bc_cpu import (CENTER, bump, moving_femp,
                                     rotating_split)
from test_gpu_boundary_feedback import _nse_setup, gtiu, run_resident  # noqa

pytestmark = pytest.mark.gpu

EPS = 2.**-52
FTOL = 1e-11
LOOP = dict(Nts=25, tE=0.125, Nu=2)


@pytest.fixture(scope='module')
def att(gtiu, toy_prob):
    """drag, lift, torque of the obstacle and the moving energy budget, built
    for the loop's Dirichlet dofs: the static ones, then the inflow's"""
    from dolfin_navier_scipy_amd import fem
    prob, th = toy_prob, toy_prob['th']
    statinds, statvals, cntinds, cntbase = bs.split(prob)
    nodes = rotating_split(prob)[3]
    femp = moving_femp(prob, statinds, cntinds, statvals, cntbase)
    fn = _forces(th, femp, nodes)
    qf = fem.energy_budget(th, femp, moving=True)
    assert fn.names == ['fx', 'fy', 'torque', 'bump']
    assert fn.cab.shape == (4, 240)
    # (the bump at the inflow reaches controlled dofs, the forces static ones)
    assert fn.cab[3][:, statinds.size:].nnz > 0 and fn.cab[0].nnz > 0
    assert (qf.NV, qf.ndbc, nodes.size) == (1286, 240, 15)
    return dict(fn=fn, qf=qf, inv=np.asarray(prob['invinds']),
                dbi=np.asarray(femp['dbcinds']), cntinds=cntinds,
                statvals=statvals, rsd=dict(functionals=fn, quadratics=qf))


def _forces(th, femp, nodes):
    """drag, lift and torque of the obstacle and the momentum balance tested
    with a bump at the inflow, which reaches the controlled dofs"""
    from dolfin_navier_scipy_amd import fem
    return fem.boundary_forces(th, femp, nodes=nodes) \
        + fem.boundary_torque(th, femp, nodes=nodes, center=CENTER) \
        + fem.MomentumFunctionals(th, femp,
                                  bump(th, 0.3, (0., 0.2)).reshape((-1, 1)),
                                  names=['bump'])


def _dbc_rows(att, run):
    """the Dirichlet values of the states 1 .. last: those the Heun start
    left, then the rows the device wrote, the static values in front"""
    bcs = np.vstack([run['v'][1][att['cntinds']][None, :],
                     run['last']['feedback_bcs']])
    return np.hstack([np.tile(att['statvals'], (bcs.shape[0], 1)), bcs])


def _check_rows(att, run, what, tab=None):
    """functional and quadratic rows against `evaluate` of the saved states;
    returns the worst errors in units of the two bounds"""
    fn, qf, inv = att['fn'], att['qf'], att['inv']
    lr, vs, ps = run['last'], run['v'], run['p']
    dt = run['t'][1] - run['t'][0]
    own = tab is None
    tab = _dbc_rows(att, run) if own else tab
    nrow = vs.shape[0] - 2
    assert lr['functionals'].shape == (nrow, fn.nF)
    assert lr['quadratics'].shape == (nrow, qf.nQ)
    assert tab.shape == (nrow + 1, 240)
    # (the saved states carry the table's values)
    assert not own or np.array_equal(tab, vs[1:][:, att['dbi']])
    wf, wq = np.zeros(fn.nF), np.zeros(qf.nQ)
    for r in range(nrow):
        v, vp = vs[r + 2][inv], vs[r + 1][inv]
        y, T = fn.evaluate(v, vp, ps[r + 2], dt, return_scale=True,
                           dbc=tab[r + 1], dbc_prev=tab[r])
        wf = np.maximum(wf, np.abs(lr['functionals'][r] - y)/(FTOL*T))
        y, T, n = qf.evaluate(v, vp, dt, return_scale=True, dbc=tab[r + 1],
                              dbc_prev=tab[r])
        wq = np.maximum(wq, np.abs(lr['quadratics'][r] - y)/(n*EPS*T))
    print(what, ': worst |row - evaluate|, functionals in units of 1e-11 T',
          dict(zip(fn.names, wf)), ', quadratics in units of n 2^-52 T',
          dict(zip(qf.names, wq)))
    assert np.all(wf <= 1.) and np.all(wq <= 1.), (what, wf, wq)
    return wf, wq


# ---- 1. the rows of the closed loop -------------------------------------------------

@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_rows_of_the_closed_loop(gtiu, toy_prob, att, scheme):
    a = run_resident(gtiu, toy_prob, scheme, ntimeslices=3,
                     resident=dict(att['rsd'], record=True), **LOOP)
    lr = a['last']
    assert lr['feedback'] == 'resident-boundary'
    assert lr['functionals_on'] == lr['quadratics_on'] == 'device'
    assert lr['run_calls'] == 3 and a['fb'].calls['abtwo'] == 0
    assert lr['functionals_names'] == att['fn'].names
    assert lr['quadratics_names'] == att['qf'].names
    assert np.array_equal(lr['functionals_t'], a['kw']['trange'][2:])
    assert np.array_equal(lr['quadratics_t'], a['kw']['trange'][2:])
    # the controlled values do move, and the forms see it
    assert np.ptp(lr['feedback_u']) > 1e-4
    assert np.ptp(lr['feedback_bcs'], axis=0).max() > 1e-4
    _check_rows(att, a, scheme + ' closed loop')
    tab = _dbc_rows(att, a)
    frozen = np.tile(tab[0], (tab.shape[0], 1))
    with pytest.raises(AssertionError):
        _check_rows(att, a, 'frozen values', tab=frozen)
    rows = lr['quadratics']
    assert rows[:, 0].min() > 1e-2 and rows[:, 1].min() > 0.
    assert rows[:, 3].min() > 0.


# ---- 2. zero gain: the table's owner is all that differs ----------------------------

@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_zero_gain_rows_equal_the_time_only_loops(gtiu, toy_prob, att,
                                                  scheme):
    """`hc = 0`: the operator's table holds `base` in every row, the
    `bcs_time_only` loop that prescribes `base` uploads the same values into
    tables of the attachments' own -- the same kernel instances on the same
    values: the same bits (the statement of
    `test_zero_gain_equals_the_time_only_loop`, for the logs)"""
    a = run_resident(gtiu, toy_prob, scheme, zero_gain=True, ntimeslices=3,
                     resident=dict(att['rsd']), **dict(LOOP, Nu=1))
    assert a['last']['feedback'] == 'resident-boundary'
    assert not np.any(a['last']['feedback_u'])
    base = a['fb'].base.tolist()
    b = run_resident(gtiu, toy_prob, scheme, ntimeslices=3,
                     getbcs=lambda t, v, p, mode=None: list(base),
                     resident=dict(att['rsd'], bcs_time_only=True),
                     **dict(LOOP, Nu=1))
    assert b['last']['feedback'] is None
    assert np.array_equal(a['v'], b['v']) and np.array_equal(a['p'], b['p'])
    for key in ('functionals', 'quadratics'):
        assert a['last'][key + '_on'] == b['last'][key + '_on'] == 'device'
        assert a['last'][key].shape[0] == 24
        assert np.abs(a['last'][key]).min(axis=0).max() > 0
        assert np.array_equal(a['last'][key], b['last'][key]), key


# ---- 3. slices and chunks -------------------------------------------------------------

def _same_rows(a, b):
    """rows whose two states are the same bits in both runs"""
    return [r for r in range(a['v'].shape[0] - 2)
            if all(np.array_equal(a[k][r + q], b[k][r + q])
                   for k in ('v', 'p') for q in (1, 2))]


def test_one_slice_three_slices_and_chunks(gtiu, toy_prob, att):
    """the operator's table is uploaded again per slice and per chunk of the
    recorder, row 0 with the current values: the live source works there
    unchanged"""
    rsd = dict(att['rsd'], record=True)
    # (a snapshot is NV + NP = 1493 doubles padded to 1536: four fit, so the
    # slices of 8 steps run as two chunks)
    snap = 8*1536
    one = run_resident(gtiu, toy_prob, 'cnab', ntimeslices=1, resident=rsd,
                       **LOOP)
    three = run_resident(gtiu, toy_prob, 'cnab', ntimeslices=3, resident=rsd,
                         **LOOP)
    chunks = run_resident(gtiu, toy_prob, 'cnab', ntimeslices=3,
                          resident=dict(rsd, record_bytes=4*snap), **LOOP)
    again = run_resident(gtiu, toy_prob, 'cnab', ntimeslices=3,
                         resident=dict(rsd, record_bytes=4*snap), **LOOP)
    assert [r['last']['run_calls'] for r in (one, three, chunks)] == [1, 3, 6]
    for what, run in (('one slice', one), ('three slices', three),
                      ('two chunks per slice', chunks)):
        _check_rows(att, run, what)
    # the same call twice: the same bits
    for key in ('functionals', 'quadratics', 'feedback_bcs'):
        assert np.array_equal(chunks['last'][key], again['last'][key])
    for what, other in (('one slice', one), ('chunks', chunks)):
        same = _same_rows(three, other)
        print('three slices against', what, ': states identical in',
              len(same), 'of 24 rows')
        assert len(same) >= 1
        for key in ('functionals', 'quadratics'):
            assert np.array_equal(three['last'][key][same],
                                  other['last'][key][same]), (what, key)
            rel = np.abs(three['last'][key] - other['last'][key]).max() \
                / np.abs(three['last'][key]).max()
            assert rel <= 1e-6, (what, key, rel)


# ---- 4. read-only -----------------------------------------------------------------------

@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_attachments_leave_the_closed_loop_alone(gtiu, toy_prob, att, scheme):
    a = run_resident(gtiu, toy_prob, scheme, ntimeslices=3,
                     resident=dict(att['rsd'], record=True), **LOOP)
    b = run_resident(gtiu, toy_prob, scheme, ntimeslices=3,
                     resident=dict(record=True), **LOOP)
    assert 'functionals' not in b['last'] or b['last']['functionals'] is None
    assert np.array_equal(a['v'], b['v']) and np.array_equal(a['p'], b['p'])
    assert np.array_equal(a['vend'], b['vend'])
    assert np.array_equal(a['pend'], b['pend'])
    for key in ('feedback_y', 'feedback_u', 'feedback_bcs'):
        assert np.array_equal(a['last'][key], b['last'][key]), key
    for k in ('lasthx', 'lastrhs'):
        assert np.array_equal(a['fb'].memory[k], b['fb'].memory[k])


# ---- 5. what is refused beside the feedback -----------------------------------------------

def test_attachments_built_for_other_values_are_refused(gtiu, toy_prob, att):
    from dolfin_navier_scipy_amd import fem
    prob, th = toy_prob, toy_prob['th']
    const_femp = dict(invinds=prob['invinds'], nu=prob['nu'],
                      dbcinds=prob['dbcinds'], dbcvals=prob['dbcvals'])
    short = dict(const_femp, dbcinds=att['dbi'][:-2],
                 dbcvals=np.zeros(att['dbi'].size - 2))
    for key, bad in (('quadratics', fem.energy_budget(th, const_femp)),
                     ('quadratics', fem.kinetic_energy(th, short,
                                                       moving=True)),
                     ('quadratics', object()), ('functionals', object()),
                     ('functionals', fem.pressure_difference(
                         th, (0.15, 0.2), (0.3, 0.2))),
                     ('rom', object())):
        with pytest.raises(ValueError) as exc:
            run_resident(gtiu, toy_prob, 'cnab', resident={key: bad})
        assert '`{0}`'.format(key) in str(exc.value), str(exc.value)
        assert 'BoundaryFeedback' in str(exc.value)


# ---- 6. through solve_nse -------------------------------------------------------------------

@pytest.mark.parametrize('funcs', ['fb', 'controls'])
def test_through_solve_nse(gtiu, toy_prob, funcs):
    from dolfin_navier_scipy_amd import fem
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    prob, th = toy_prob, toy_prob['th']
    kw, fb, cntinds, cntvals = _nse_setup(gtiu, prob, funcs)
    statinds = np.asarray(kw['dbcinds'], dtype=np.int64)
    inner = np.setdiff1d(kw['invinds'], cntinds)
    dbi = np.concatenate([statinds, cntinds])
    femp = dict(invinds=inner, nu=prob['nu'], dbcinds=dbi,
                dbcvals=np.concatenate([kw['dbcvals'],
                                        np.zeros(cntinds.size)]))
    nodes = rotating_split(prob)[3]
    fn = _forces(th, femp, nodes)
    qf = fem.energy_budget(th, femp, moving=True)
    trange = kw['trange']
    try:
        vd, pd = snu.solve_nse(functionals=fn, quadratics=qf,
                               record_on_device=True,
                               return_dictofpstrs=True, **kw)
        lr = dict(gtiu.LAST_RUN)
        for extra in (dict(rom=object(), pod=object()),
                      dict(functionals=object())):
            kw2 = _nse_setup(gtiu, prob, funcs)[0]
            with pytest.raises(ValueError) as exc:
                snu.solve_nse(**dict(kw2, **extra))
            assert '`{0}`'.format(list(extra)[0]) in str(exc.value)
            assert 'BoundaryFeedback' in str(exc.value)
    finally:
        snu.clear_cache()
    assert lr['feedback'] == 'resident-boundary' and lr['record'] == 'device'
    assert lr['functionals_on'] == lr['quadratics_on'] == 'device'
    assert lr['run_calls'] == 11 and fb.calls['abtwo'] == 0
    assert np.ptp(lr['feedback_u']) > 1e-4
    run = dict(t=trange, v=np.array([vd[t][:, 0] for t in trange]),
               p=np.array([pd[t][:, 0] for t in trange]), last=lr)
    a = dict(fn=fn, qf=qf, inv=inner, dbi=dbi, cntinds=cntinds,
             statvals=np.asarray(kw['dbcvals'], dtype=np.float64))
    _check_rows(a, run, 'solve_nse ' + funcs)
