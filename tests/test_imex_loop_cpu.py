"""The host loop of `time_int_utils.cnab` / `sbdftwo` without a device: the
loop itself is host Python, so with `tests/imex_host_model.py` behind it (a
direct solve where the device iterates) the golden vectors of the reference's
own `time_int_utils`, the order of the callbacks, the protocol of the loop's
attachments and the shape of `LAST_RUN` are checked on any machine."""
import os

import numpy as np
import pytest

import feedback_setup as fs
import imex_host_model
import scenarios
from oracle import imex_oracle

# a direct solve on both sides: measured 5.9e-14 (velocities) and 4.7e-13
# (pressures); 1e-10 leaves two orders of magnitude for another SciPy / LU
# build and stays two below the project's 1e-8
TOL = 1e-10
SCHEMES = ('cnab', 'sbdf2')


@pytest.fixture
def tiu(monkeypatch):
    return imex_host_model.install(monkeypatch)


def run_scheme(tiu, scheme, kw):
    kw = dict(kw)
    if scheme == 'sbdf2':
        kw.pop('f_tvdp', None)
        return tiu.sbdftwo(**kw)
    return tiu.cnab(**kw)


def resident_kw(kw, prob):
    """the same scenario with the stub operator for `f_vdp`, resident"""
    kw = dict(kw)
    conv = imex_host_model.StubConvection(kw.pop('f_vdp'), kw['appndbcs'])
    kw.update(device_convection=conv, invinds=prob['invinds'],
              resident=dict(bcs_time_only=True))
    return kw


def assert_golden(golden_dir, scheme, variant, seed, rec, ff):
    gold = np.load(os.path.join(
        golden_dir, 'imex_{0}_{1}_s{2}.npz'.format(scheme, variant, seed)))
    times, vels, prss = rec.arrays()
    assert ff == int(gold['ffflag'])
    assert np.allclose(times, gold['times'], rtol=0, atol=1e-15)
    for k in range(times.size):
        ev = np.linalg.norm(vels[k] - gold['vels'][k]) / \
            np.linalg.norm(gold['vels'][k])
        assert ev <= TOL, (k, ev)
        if k > 0:
            ep = np.linalg.norm(prss[k] - gold['prss'][k]) / \
                np.linalg.norm(gold['prss'][k])
            assert ep <= TOL, (k, ep)


@pytest.mark.parametrize('scheme', SCHEMES)
@pytest.mark.parametrize('seed,variant', list(enumerate(scenarios.VARIANTS)))
def test_host_loop_matches_reference_golden(tiu, golden_dir, toy_prob, scheme,
                                            seed, variant):
    kw, rec, _ = scenarios.build(variant=variant, seed=seed, prob=toy_prob)
    v, p, ff = run_scheme(tiu, scheme, kw)
    assert_golden(golden_dir, scheme, variant, seed, rec, ff)


@pytest.mark.parametrize('scheme', SCHEMES)
@pytest.mark.parametrize('seed,variant', [(0, 'plain'), (2, 'movingbc')])
def test_one_row_formula_on_both_paths(tiu, golden_dir, toy_prob, scheme,
                                       seed, variant):
    """the `g` a step solves with is the same array whether the loop takes one
    step at a time or tabulates whole slices"""
    kw, rec, _ = scenarios.build(variant=variant, seed=seed, prob=toy_prob)
    run_scheme(tiu, scheme, kw)
    assert tiu.LAST_RUN['run_calls'] == 0
    kw, rec, _ = scenarios.build(variant=variant, seed=seed, prob=toy_prob)
    v, p, ff = run_scheme(tiu, scheme, resident_kw(kw, toy_prob))
    assert tiu.LAST_RUN['run_calls'] > 0
    stepwise, resident = (s.glog for s in imex_host_model.HostStepper.made)
    assert len(stepwise) == len(resident) == 11
    for k, (gs, gr) in enumerate(zip(stepwise, resident)):
        assert np.array_equal(gs, gr), k
    assert_golden(golden_dir, scheme, variant, seed, rec, ff)


CALLBACKS = ('f_vdp', 'getbcs', 'applybcs', 'f_tdp', 'g_tdp', 'dynamic_rhs',
             'savevp')


def logged(kw):
    """`kw` with its callbacks wrapped: each call appends `(name, time or
    None, mode or None)` to the list that is returned with it"""
    calls, kw = [], dict(kw)

    def wrap(name, fun):
        def wrapped(*args, **kwargs):
            time = kwargs.get('time', None)
            if name in ('getbcs', 'f_tdp', 'g_tdp', 'dynamic_rhs'):
                time = args[0]
            calls.append((name, time, kwargs.get('mode', None)))
            return fun(*args, **kwargs)
        return wrapped
    for name in CALLBACKS:
        if kw.get(name, None) is not None:
            kw[name] = wrap(name, kw[name])
    return kw, calls


@pytest.mark.parametrize('scheme', SCHEMES)
@pytest.mark.parametrize('seed,variant', [(1, 'forced'), (2, 'movingbc')])
def test_callbacks_in_the_order_of_the_reference(tiu, toy_prob, scheme, seed,
                                                 variant):
    """callbacks have side effects (the memory of `dynamic_rhs`): the
    stepwise loop calls them like the restatement of tiu:104-143, 320-353"""
    integ = imex_oracle.cnab if scheme == 'cnab' else imex_oracle.sbdftwo
    kw, _, _ = scenarios.build(variant=variant, seed=seed, prob=toy_prob)
    kw, want = logged(kw)
    if scheme == 'sbdf2':
        kw.pop('f_tvdp', None)
    integ(**kw)
    kw, _, _ = scenarios.build(variant=variant, seed=seed, prob=toy_prob)
    kw, got = logged(kw)
    run_scheme(tiu, scheme, kw)
    assert len(want) > 11*len([c for c in CALLBACKS if c in kw])
    assert got == want


class Spy(object):
    """mixed into the loop's attachment base: logs what the loop calls"""

    def __init__(self):
        self.calls = []

    def start(self, v, p, time):
        self.calls.append(('start', time))

    def arm(self, times, tables):
        self.calls.append(('arm', list(times), np.array(tables.dbc)))

    def collect(self, times):
        self.calls.append(('collect', list(times)))

    def host_row(self, step):
        self.calls.append(('host_row', step))

    def finish(self, drm):
        self.calls.append(('finish',))

    def report(self):
        return dict(spy_calls=len(self.calls))


@pytest.mark.parametrize('scheme', SCHEMES)
def test_the_protocol_is_the_only_door(tiu, monkeypatch, toy_prob, scheme):
    """an attachment the loop has never heard of, appended to its list, is
    started, armed and collected per slice (with the slice's times and `n + 1`
    rows of Dirichlet values), or handed every stepwise step, finished, and
    reports into `LAST_RUN`"""
    spy = type('SpyAttachment', (Spy, tiu._Attachment), {})()
    attach = tiu._ImexLoop.attach

    def attach_and_append(self, *args, **kwargs):
        attach(self, *args, **kwargs)
        self.attachments.append(spy)
    monkeypatch.setattr(tiu._ImexLoop, 'attach', attach_and_append)
    kw, rec, _ = scenarios.build(variant='movingbc', seed=2, prob=toy_prob)
    trange, getbcs = kw['trange'], kw['getbcs']
    _, slices = tiu._inittimegrid(trange, ntimeslices=10)
    slices = [s for s in slices if len(s)]

    def vals(t):
        return getbcs(t, None, None)
    run_scheme(tiu, scheme, resident_kw(kw, toy_prob))
    assert tiu.LAST_RUN['spy_calls'] == len(spy.calls) == 2 + 2*len(slices)
    assert spy.calls[0] == ('start', trange[1])
    assert spy.calls[-1] == ('finish',)
    before = trange[1]
    for k, ctrange in enumerate(slices):
        name, times, rows = spy.calls[1 + 2*k]
        assert name == 'arm' and times == ctrange
        # the values of the state before each step and behind the last
        assert rows.shape[0] == len(ctrange) + 1
        assert np.array_equal(
            rows, np.array([vals(t) for t in [before] + ctrange]))
        assert spy.calls[2 + 2*k] == ('collect', ctrange)
        before = ctrange[-1]
    # one step at a time
    spy.calls = []
    kw, rec, _ = scenarios.build(variant='movingbc', seed=2, prob=toy_prob)
    run_scheme(tiu, scheme, kw)
    times, vels, prss = rec.arrays()
    inv = toy_prob['invinds']
    assert tiu.LAST_RUN['spy_calls'] == len(spy.calls) == 2 + 11
    assert spy.calls[0] == ('start', trange[1])
    assert spy.calls[-1] == ('finish',)
    for k, (name, step) in enumerate(spy.calls[1:-1], start=2):
        assert name == 'host_row' and step.time == trange[k]
        assert np.array_equal(step.v[:, 0], vels[k][inv])
        assert np.array_equal(step.v_prev[:, 0], vels[k - 1][inv])
        assert np.array_equal(step.p[:, 0], prss[k])
        assert step.dbc == vals(trange[k])
        assert step.dbc_prev == vals(trange[k - 1])


OPEN_LOOP_KEYS = {'record', 'run_calls', 'record_y', 'record_t', 'integrator',
                  'time_steps', 'krylov_steps', 'schur_hierarchy', 'precond',
                  'feedback', 'feedback_y', 'feedback_u'}


@pytest.mark.parametrize('scheme', SCHEMES)
def test_last_run_keeps_its_shape(tiu, toy_prob, scheme):
    kw, rec, _ = scenarios.build(variant='plain', seed=0, prob=toy_prob)
    run_scheme(tiu, scheme, kw)
    run = tiu.LAST_RUN
    assert set(run) == OPEN_LOOP_KEYS
    assert run['feedback'] is None and run['record'] == 'host'
    assert run['feedback_y'] is None and run['feedback_u'] is None
    assert run['record_y'] is None and run['record_t'] is None
    assert run['integrator'] == ('cnab' if scheme == 'cnab' else 'sbdftwo')
    assert run['time_steps'] == 11 and run['run_calls'] == 0
    # a `LinearFeedback` the host calls back: the rows of its AB2 steps
    cv_mat, b_mat = fs.sensors_actuators(toy_prob['th'], toy_prob['invinds'],
                                         toy_prob['smc']['M'])
    obs = fs.observer(5, cv_mat.shape[0], b_mat.shape[1])
    fb = tiu.LinearFeedback(cv_mat, b_mat, obs['ha'], obs['hb'], obs['hc'],
                            obs['inihx'], drift=fs.drift_of(obs['dvec']))
    kw, rec, _ = scenarios.build(variant='plain', seed=0, prob=toy_prob)
    kw.update(dynamic_rhs=fb, dynamic_rhs_memory={})
    run_scheme(tiu, scheme, kw)
    run = tiu.LAST_RUN
    assert set(run) == OPEN_LOOP_KEYS
    assert run['feedback'] == 'host' and run['record'] == 'host'
    assert fb.calls == dict(init=1, heunpred=1, heuncorr=1, abtwo=11)
    rows = [h for h in fb.history if h[1] == 'abtwo']
    assert np.array_equal(run['feedback_y'], np.array([h[2] for h in rows]))
    assert np.array_equal(run['feedback_u'], np.array([h[3] for h in rows]))
    assert run['feedback_y'].shape == (11, fb.Ny)
    assert run['feedback_u'].shape == (11, fb.Nu)
