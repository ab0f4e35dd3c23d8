"""The six attachments of the resident IMEX loop side by side: observer
feedback, recorder, functionals, statistics, quadratics and ensemble on one
stepper say, bit for bit, what each of the five says alone beside the feedback
(which stays on in every leg: it alters the right-hand side), and the shortest
of their tables is the one that ends a run.

`scenarios.toy_problem()` through the `Loop` of `test_gpu_pod.py` (NV = 1286,
NP = 207).  A leg is `run(4)`, one `step`, the tables set again, `run(3)`:
launches, a replayed graph and the closing node all write rows, and the
statistics' sums and the ensemble's slots are kept across the second arming
(no `reset`).
"""
import numpy as np
import pytest
import scipy.sparse as sps

import feedback_setup as fs
from test_gpu_pod import Loop, _femp, gtiu  # noqa: F401

pytestmark = pytest.mark.gpu

FIVE = ('rec', 'fn', 'st', 'qd', 'ens')
# (rows of the first and of the second arming: run(4) + step, run(3))
N1, N2 = 5, 3
BINS = (np.array([0, 1, 0, 1, 0], dtype=np.int32),
        np.array([1, 0, 1], dtype=np.int32))
SLOTS = (np.array([0, -1, 1, -1, 2], dtype=np.int32),
         np.array([3, -1, 4], dtype=np.int32))


@pytest.fixture(scope='module')
def parts(gtiu, toy_prob):
    from dolfin_navier_scipy_amd import fem
    th, femp = toy_prob['th'], _femp(toy_prob)
    NP, NV = toy_prob['smc']['J'].shape
    C, B = fs.sensors_actuators(th, toy_prob['invinds'],
                                sps.csr_matrix(toy_prob['smc']['M']))
    obs = fs.observer(7, C.shape[0], B.shape[1])
    return dict(C=C, B=B, obs=obs,
                fn=fem.pressure_difference(th, 3, 5),
                qf=fem.kinetic_energy(th, femp) + fem.dissipation(th, femp),
                pairs=np.array([(0, 1), (NV - 1, NV), (NV + NP - 1, 2)],
                               dtype=np.int32))


def _feedback(lp, parts):
    obs = parts['obs']
    lp.stp.set_feedback(parts['C'], parts['B'], obs['ha'], obs['hb'],
                        obs['hc'], c_n=.5, c_c=.5, dt=lp.dt)
    lp.stp.set_feedback_state(obs['inihx'], np.zeros(obs['ha'].shape[0]),
                              obs['hc'] @ obs['inihx'])


def _arm(lp, parts, on, half, rows=None):
    """the tables of `on` for the steps of arming `half` (`rows`: another
    length per attachment)"""
    stp, n = lp.stp, (N1, N2)[half]
    rows = dict.fromkeys(('fb',) + FIVE, n) if rows is None else rows
    pad = (lambda a, k: np.concatenate([a, np.full(k, -1, a.dtype)])[:k])
    stp.set_feedback_table(rows['fb'], None)
    if 'rec' in on:
        stp.set_recorder(rows['rec'], cv_mat=parts['C'], snap_slots='all')
    if 'fn' in on:
        stp.set_functionals(parts['fn'], rows['fn'], lp.dt)
    if 'st' in on:
        stp.set_statistics(pad(BINS[half], rows['st']), nbins=2,
                           pairs=parts['pairs'])
    if 'qd' in on:
        stp.set_quadratics(parts['qf'], rows['qd'], lp.dt)
    if 'ens' in on:
        stp.set_ensemble(pad(SLOTS[half], rows['ens']), nslots=5)


def _collect(stp, on):
    got = dict(fb=stp.feedback_log())
    if 'rec' in on:
        got['rec'] = (stp.record_outputs(),) + stp.record_snapshots()
    if 'fn' in on:
        got['fn'] = stp.get_functionals()
    if 'qd' in on:
        got['qd'] = stp.get_quadratics()
    return got


def _leg(toy_prob, parts, on, use_graph):
    from dolfin_navier_scipy_amd import saddle
    lp = Loop(toy_prob)
    lp.opts = saddle.solve_opts(method='gmres', rtol=1e-12, maxiter=400,
                                restart=60, check_every=2,
                                use_graph=use_graph, reorth=2)
    try:
        stp = lp.stp
        _feedback(lp, parts)
        _arm(lp, parts, on, 0)
        stp.run(4, lp.cf, lp.opts)
        stp.step(lp.cf, opts=lp.opts)
        assert stp.table_position() == (N1, 0)
        first = _collect(stp, on)
        _arm(lp, parts, on, 1)
        stp.run(3, lp.cf, lp.opts)
        assert stp.table_position() == (N2, 0)
        second = _collect(stp, on)
        if 'st' in on:
            second['st'] = stp.statistics()
        if 'ens' in on:
            second['ens'] = stp.ensemble()
        second['state'] = stp.get_state()
        return first, second
    finally:
        lp.close()


def _same(a, b, what):
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), what
        for k in a:
            _same(a[k], b[k], what + (k,))
    elif isinstance(a, tuple):
        assert len(a) == len(b), what
        for k, (x, y) in enumerate(zip(a, b)):
            _same(x, y, what + (k,))
    else:
        assert a.shape == b.shape and np.array_equal(a, b), what


@pytest.mark.parametrize('use_graph', [True, False])
def test_all_six_say_what_each_says_alone(gtiu, toy_prob, parts, use_graph):
    both = _leg(toy_prob, parts, FIVE, use_graph)
    # the legs do write: the loop is closed, every log is full and moves, the
    # sums and slots of the first arming are still there behind the second
    assert np.abs(both[0]['fb'][1]).max() > 0
    for half, n in ((0, N1), (1, N2)):
        assert both[half]['fn'].shape == (n, parts['fn'].nF)
        assert both[half]['qd'].shape == (n, parts['qf'].nQ)
        assert np.abs(both[half]['qd']).min() > 0
        assert np.ptp(both[half]['fn'], axis=0).min() > 0
        y, vs, ps = both[half]['rec']
        assert y.shape == (n, parts['C'].shape[0]) and vs.shape[0] == n
        assert np.abs(y - (parts['C'] @ vs.T).T).max() <= \
            1e-12*np.abs(y).max()
    last = both[1]
    assert last['st']['counts'].tolist() == [4, 4]
    assert np.array_equal(last['ens'][[0, 1, 2]], both[0]['rec'][1][[0, 2, 4]])
    assert np.array_equal(last['ens'][[3, 4]], last['rec'][1][[0, 2]])
    assert np.array_equal(last['state'][0][:, 0], last['rec'][1][-1])
    assert np.array_equal(last['state'][1][:, 0], last['rec'][2][-1])
    for one in FIVE:
        alone = _leg(toy_prob, parts, (one,), use_graph)
        for half in (0, 1):
            want = {k: both[half][k] for k in alone[half]}
            _same(alone[half], want, (one, half))


def test_the_shortest_table_ends_the_run(gtiu, toy_prob, parts):
    from dolfin_navier_scipy_amd import _capi
    rows = dict(fb=10, rec=6, fn=5, st=7, qd=8, ens=9)
    lp = Loop(toy_prob)
    try:
        stp = lp.stp
        _feedback(lp, parts)
        _arm(lp, parts, FIVE, 0, rows=rows)
        assert stp.table_position() == (0, 5)
        with pytest.raises(_capi.DnsError) as exc:
            stp.run(6, lp.cf, lp.opts)
        assert '6 steps asked for, the per-step tables hold 5 more' in \
            str(exc.value)
        assert stp.table_position() == (0, 5)
        stp.run(5, lp.cf, lp.opts)
        assert stp.table_position() == (5, 0)
        assert stp.get_functionals().shape == (5, parts['fn'].nF)
        assert stp.get_quadratics().shape == (5, parts['qf'].nQ)
        with pytest.raises(_capi.DnsError):
            stp.step(lp.cf, opts=lp.opts)
        # every attachment in turn is the shortest
        for short in ('fb',) + FIVE:
            _arm(lp, parts, FIVE, 0, rows=dict(rows, **{short: 4}))
            assert stp.table_position() == (0, 4), short
    finally:
        lp.close()
