"""`TrapezoidalStepper.sweep` without a device.  What a sweep decides -- batch
lengths, cycle lengths, replays, rebuilds of the preconditioner -- is host
arithmetic on the counters of `poll()`; `tests/trap_sweep_model.py` scripts
those counters, and `tests/golden/trap_sweep_calls.json` holds every call the
sweep made on the stepper and everything it returned at the commit before it
was split into a loop, `_CyclePolicy` and `_RefreshPolicy`.  The scenarios are
replayed on the tree's code and must give the same, the floats bit for bit;
the branches of the policies the golden file is there for are asserted on the
file itself; a few transitions of the two classes are written out by hand."""
import json
import os

import pytest

import trap_sweep_model as model
from dolfin_navier_scipy_amd import newton_picard as dnp

PARENT = 'e1342e3f2fa42371c266ac82fa5ea265c8a6508a'
BOUND = 3.0                            # `refresh_iters` of the model's default


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'trap_sweep_calls.json')) as fh:
        return json.load(fh)


def test_golden_file_was_made_before_the_split(golden, golden_dir):
    assert golden['commit'] == PARENT
    assert set(golden['scenarios']) == set(model.SCENARIOS)
    size = os.path.getsize(os.path.join(golden_dir, 'trap_sweep_calls.json'))
    assert size < 512*1024


@pytest.mark.parametrize('name', sorted(model.SCENARIOS))
def test_sweep_makes_the_pinned_calls(golden, name):
    got = json.loads(json.dumps(model.run_scenario(name)))
    want = golden['scenarios'][name]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w) == {'log', 'tot', 'norm', 'vtimes', 'ptimes',
                                    'refreshes'}
        assert set(g['tot']) == {'iters', 'device_seconds', 'refreshes',
                                 'replayed_batches', 'batches', 'cycle'}
        for key in ('tot', 'norm', 'vtimes', 'ptimes', 'refreshes'):
            assert g[key] == w[key], (name, k, key)
        for i, (ge, we) in enumerate(zip(g['log'], w['log'])):
            assert ge == we, (name, k, i)
        assert len(g['log']) == len(w['log'])


# ---- what the golden file is there for ---------------------------------
def batches(sweep):
    """the pipelined batches of a recorded sweep: cycle length, first slot,
    steps, the counters of its `poll`, whether it was replayed step by step
    and whether the preconditioner was rebuilt behind it"""
    out, log = [], sweep['log']
    for i, e in enumerate(log):
        if e[0] == 'checkpoint':
            assert log[i + 1][0] == 'set_pipeline' and log[i + 1][1] > 0
            out.append(dict(cycle=log[i + 1][1], count=0, slot0=None,
                            restored=False, refreshed=False))
        elif not out:
            continue
        elif e[0] == 'run':
            assert e[3] == out[-1]['cycle']
            out[-1].update(slot0=e[1], count=e[2])
        elif e[0] == 'step' and 'poll' not in out[-1]:
            if out[-1]['slot0'] is None:
                out[-1]['slot0'] = e[4]
            out[-1]['count'] += 1
        elif e[0] == 'poll':
            out[-1]['poll'] = e[1]
            assert log[i + 1] == ['set_pipeline', 0]
        elif e[0] == 'restore':
            out[-1]['restored'] = True
        elif e[0] == 'refresh_precond':
            out[-1]['refreshed'] = True
    assert len(out) == len(sweep['tot']['batches']) or not out
    return out


def need(third):
    return max(1, model._ceil3(third))


def test_cycle_rises_without_a_replay(golden):
    sw = golden['scenarios']['raise_without_replay'][0]
    bs = batches(sw)
    rises = [(a, b) for a, b in zip(bs, bs[1:])
             if a['poll']['maxrel'] > 0.9 and a['poll']['fails'] == 0]
    assert rises
    for a, b in rises:
        assert b['cycle'] == a['cycle'] + 1 and not a['restored']
    assert sw['tot']['replayed_batches'] == 0
    assert not any(e[0] == 'restore' for e in sw['log'])


def test_cycle_shrinks_to_the_columns_run(golden):
    bs = batches(golden['scenarios']['learn_shrink_hint'][0])
    shrunk = [(a, b) for a, b in zip(bs, bs[1:])
              if a['poll']['maxit'] < a['cycle']]
    assert shrunk and all(a['poll']['fails'] == 0 for a, _ in shrunk)
    for a, b in shrunk:
        assert b['cycle'] == a['poll']['maxit']


def trials(bs):
    """indices of the batches that try one column less than a batch which ran
    all of its columns"""
    return [i for i in range(1, len(bs))
            if bs[i]['cycle'] == bs[i - 1]['cycle'] - 1
            and bs[i - 1]['poll']['fails'] == 0
            and bs[i - 1]['poll']['maxit'] == bs[i - 1]['cycle']]


def test_a_trial_batch_is_short_and_holds(golden):
    # the Newton sweep with a hint: no learning, whole batches of 32
    bs = batches(golden['scenarios']['trial_holds'][2])
    (i,) = trials(bs)
    assert 0. < bs[i - 1]['poll']['maxprev'] < 0.25
    assert bs[i - 1]['count'] == 32 and bs[i]['count'] == 16
    assert bs[i]['poll']['fails'] == 0 and not bs[i]['restored']
    assert all(b['cycle'] == bs[i]['cycle'] and b['poll']['fails'] == 0
               for b in bs[i:])
    assert bs[i + 1]['count'] == 32


@pytest.mark.parametrize('name,wait', [('trial_fails_backoff', 9),
                                       ('trial_ends_at_tolerance', 8)])
def test_a_failed_trial_makes_the_next_one_wait(golden, name, wait):
    """the first trial comes behind the first whole batch; the one behind a
    trial that failed waits for `hold = backoff = 4 x 2` batches (a replayed
    batch does not count one down, a batch that went through does).  Without
    the back-off it would come behind 5 (`max(2, 4)` of a replay) or 2
    batches"""
    (sw,) = golden['scenarios'][name]
    bs = batches(sw)
    first, second = trials(bs)
    assert first == 1
    if name == 'trial_fails_backoff':
        assert bs[first]['poll']['fails'] > 0 and bs[first]['restored']
        assert sw['tot']['replayed_batches'] == 1
    else:
        assert bs[first]['poll']['fails'] == 0 and not bs[first]['restored']
        assert bs[first]['poll']['maxrel'] > 0.9
        assert sw['tot']['replayed_batches'] == 0
    between = bs[first + 1:second]
    assert len(between) == wait
    # every one of them stood where the first trial was taken from
    for b in between:
        assert b['cycle'] == bs[0]['cycle']
        assert b['poll'] == bs[0]['poll'] and b['count'] == 16
    assert bs[second]['poll']['fails'] == 0


@pytest.mark.parametrize('name', ['fallback_oversolve',
                                  'fallback_slack_column'])
def test_a_batch_falls_back_to_synchronous_steps(golden, name):
    over = name == 'fallback_oversolve'
    spike = need(11)
    for sw in golden['scenarios'][name]:
        bs = batches(sw)
        (i,) = [i for i, b in enumerate(bs) if b['restored']]
        assert bs[i]['poll']['fails'] == 1
        assert sw['tot']['replayed_batches'] == 1
        assert bs[i + 1]['cycle'] == (max(bs[i]['cycle'] + 1, spike) if over
                                      else max(2, spike + 1))
        # the replay: restore, then the batch's steps one by one
        at = sw['log'].index(['restore', sw['log'][0][2]])
        again = [e for e in sw['log'][at + 1:at + 1 + 2*bs[i]['count']]
                 if e[0] == 'step']
        assert [e[4] for e in again] == list(
            range(bs[i]['slot0'], bs[i]['slot0'] + 16))


def test_a_second_sweep_of_a_kind_starts_from_the_hint(golden):
    pic, nwt1, nwt2 = golden['scenarios']['learn_shrink_hint']
    startup = need(12)                  # of the third sweep's first steps
    hint = nwt1['tot']['cycle']
    assert batches(nwt2)[0]['cycle'] == min(startup, hint + 1) == hint + 1
    # the Picard sweep's cycle is no hint for a Newton sweep
    assert batches(nwt1)[0]['cycle'] == batches(pic)[0]['cycle'] == need(9)


def test_a_stepper_without_a_hint_learns_on_short_batches(golden):
    pic, nwt1, nwt2 = golden['scenarios']['learn_shrink_hint']
    for sw in (pic, nwt1):
        bs = batches(sw)
        moved = [a['cycle'] != b['cycle'] for a, b in zip(bs, bs[1:])]
        n = moved.index(False) + 1       # the first batch that kept its cycle
        assert n >= 2
        assert [b['count'] for b in bs[:n]] == [16]*n
        assert bs[n]['count'] == 32
    assert batches(nwt2)[0]['count'] == 32


def test_the_form_without_oversolve_keeps_a_slack_column(golden):
    for sw in golden['scenarios']['slack_column']:
        bs = batches(sw)
        assert bs[0]['cycle'] == max(2, need(9) + 1)
        assert bs[0]['count'] == 32      # (nothing to learn)
        for a, b in zip(bs, bs[1:]):
            assert a['poll']['fails'] == 0
            assert b['cycle'] == max(2, a['poll']['maxit'] + 1)
        assert {b['cycle'] for b in bs} == {2, 3, 4}
        assert sw['tot']['cycle'] == max(2, bs[-1]['poll']['maxit'] + 1)


def test_record_is_a_matter_of_the_host_only(golden):
    """`record=True` steps through `step` + `state` where `record=False` calls
    `run`: same batches, same cycle lengths, same statistics"""
    off, on = golden['scenarios']['slack_column']
    assert off['tot'] == on['tot']
    assert [(b['cycle'], b['count'], b['poll']) for b in batches(off)] == \
        [(b['cycle'], b['count'], b['poll']) for b in batches(on)]
    assert off['vtimes'] == [] and off['ptimes'] == []
    assert on['vtimes'] == model.grid(130).tolist()
    assert on['ptimes'] == model.grid(130).tolist()[1:]


def test_other_grids_and_closed_loops_run_step_by_step(golden):
    odd, loop, unpiped, short = golden['scenarios']['step_by_step']
    for sw, nt in ((odd, 40), (loop, 40), (unpiped, 40), (short, 8)):
        assert sw['tot']['cycle'] is None
        assert {e[0] for e in sw['log']} == {
            'start', 'write_linpoint', 'step', 'update_norm'}
        steps = [e for e in sw['log'] if e[0] == 'step']
        assert [e[4] for e in steps] == list(range(1, nt))
        assert all((e[9] is not None) == (sw is loop) for e in steps)
        assert len(sw['tot']['batches']) == -(-(nt - 1)//16)
    assert {e[1] for e in odd['log'] if e[0] == 'step'} == {model.DT,
                                                            2*model.DT}


def rebuilt(sw):
    return [i for i, b in enumerate(batches(sw)) if b['refreshed']]


def test_a_first_batch_above_the_bound_rebuilds_once(golden):
    for name in ('refresh_first_batch', 'refresh_slack_column'):
        sw = golden['scenarios'][name][0]
        assert sw['tot']['batches'][0] > BOUND
        assert rebuilt(sw) == [0]
        assert sw['tot']['refreshes'] == sw['refreshes'] == 1
        assert max(sw['tot']['batches'][1:]) < BOUND


def test_a_later_batch_a_fifth_above_its_level_rebuilds(golden):
    sw = golden['scenarios']['refresh_later_then_out_of_reach'][0]
    per = sw['tot']['batches']
    (i,) = rebuilt(sw)
    assert i > 0 and per[i] > BOUND and per[i] > 1.2*per[0]
    assert all(p <= BOUND for p in per[:i])


def test_a_bound_out_of_reach_does_not_rebuild_every_batch(golden):
    first, second, third = golden['scenarios'][
        'refresh_later_then_out_of_reach']
    (i,) = rebuilt(first)
    behind = first['tot']['batches'][i + 1:]
    assert len(behind) >= 4 and min(behind) > BOUND
    # nor in the next sweep: the level is kept from sweep to sweep ...
    assert min(second['tot']['batches']) > BOUND and rebuilt(second) == []
    assert second['tot']['refreshes'] == 0 and second['refreshes'] == 1
    # ... until a batch rises a fifth above it
    level, per = behind[0], third['tot']['batches']
    (j,) = rebuilt(third)
    assert per[j] > 1.2*level
    assert any(level < p <= 1.2*level for p in per[:j])
    assert third['refreshes'] == 2


def test_no_bound_no_rebuild(golden):
    for name in ('refresh_never', 'refresh_bound_zero'):
        for sw in golden['scenarios'][name]:
            assert max(sw['tot']['batches']) > BOUND
            assert sw['tot']['refreshes'] == sw['refreshes'] == 0
            assert ['refresh_precond'] not in sw['log']


def test_no_rebuild_behind_the_last_batch(golden):
    last, more = golden['scenarios']['refresh_not_behind_last_batch']
    per = last['tot']['batches']
    assert per[-1] > BOUND and per[-1] > 1.2*per[0]
    assert rebuilt(last) == [] and last['tot']['refreshes'] == 0
    assert len(per) == len(batches(last))        # (listed all the same)
    # the same batch with steps behind it
    assert more['tot']['batches'][:len(per)] == per
    assert rebuilt(more) == [len(per) - 1]


# ---- the two policies by hand ------------------------------------------
def cycle_state(p):
    return dict(cycle=p.cycle, hold=p.hold, backoff=p.backoff,
                lowered=p.lowered, learning=p.learning)


def cycle_policy(over=True, **state):
    p = dnp._CyclePolicy(over)
    for key, val in state.items():
        assert hasattr(p, key)
        setattr(p, key, val)
    return p


def test_cycle_policy_after_the_startup_steps():
    p = dnp._CyclePolicy(True)
    assert cycle_state(p) == dict(cycle=None, hold=0, backoff=2,
                                  lowered=False, learning=False)
    p.after_startup(3)
    assert cycle_state(p) == dict(cycle=3, hold=0, backoff=2, lowered=False,
                                  learning=True)
    assert p.short_batch() and p.hint() == 3
    p = dnp._CyclePolicy(True)
    p.after_startup(0)
    assert p.cycle == 1
    # a hint bounds from above, one column of head room for the transient
    for worst, hint, cycle in ((4, 1, 2), (3, 5, 3), (3, 2, 3)):
        p = dnp._CyclePolicy(True)
        p.after_startup(worst, hint)
        assert cycle_state(p) == dict(cycle=cycle, hold=0, backoff=2,
                                      lowered=False, learning=False)
        assert not p.short_batch()
    # without oversolve: a slack column, no hint, nothing to learn
    for worst, cycle in ((3, 4), (0, 2)):
        p = dnp._CyclePolicy(False)
        p.after_startup(worst, 1)
        assert cycle_state(p) == dict(cycle=cycle, hold=0, backoff=2,
                                      lowered=False, learning=False)


def test_cycle_policy_without_oversolve_follows_the_longest_solve():
    p = cycle_policy(False, cycle=4)
    p.after_batch(maxit=1, maxneed=1, maxrel=0.95, maxprev=0.1)
    assert cycle_state(p) == dict(cycle=2, hold=0, backoff=2, lowered=False,
                                  learning=False)
    p.after_batch(maxit=2, maxneed=2, maxrel=0.5, maxprev=4.)
    assert p.cycle == 3
    p.after_fallback(6)
    assert cycle_state(p) == dict(cycle=7, hold=0, backoff=2, lowered=False,
                                  learning=False)


def test_cycle_policy_raises_shrinks_and_tries():
    # close to the tolerance: one more column, and no trial for a batch
    p = cycle_policy(cycle=2)
    p.after_batch(maxit=2, maxneed=2, maxrel=0.95, maxprev=3.)
    assert cycle_state(p) == dict(cycle=3, hold=1, backoff=2, lowered=False,
                                  learning=False)
    p = cycle_policy(cycle=2)
    p.after_batch(maxit=2, maxneed=2, maxrel=0.9, maxprev=3.)     # (not >)
    assert p.cycle == 2
    # every solve at the floor early: what was run
    p = cycle_policy(cycle=4, hold=3)
    p.after_batch(maxit=2, maxneed=1, maxrel=1e-4, maxprev=1e-3)
    assert cycle_state(p) == dict(cycle=2, hold=2, backoff=2, lowered=False,
                                  learning=False)
    # a decade below the tolerance in front of the last column: a trial
    p = cycle_policy(cycle=3)
    p.after_batch(maxit=3, maxneed=2, maxrel=0.02, maxprev=0.2)
    assert cycle_state(p) == dict(cycle=2, hold=0, backoff=2, lowered=True,
                                  learning=False)
    assert p.short_batch()
    # ... which is not taken at 0.25, at 0 (nothing accumulated), from one
    # column, or while the hold lasts
    for state, maxprev in ((dict(cycle=3), 0.25), (dict(cycle=3), 0.),
                           (dict(cycle=1), 0.2),
                           (dict(cycle=3, hold=1), 0.2)):
        p = cycle_policy(**state)
        p.after_batch(maxit=state['cycle'], maxneed=1, maxrel=0.02,
                      maxprev=maxprev)
        assert cycle_state(p) == dict(cycle=state['cycle'], hold=0, backoff=2,
                                      lowered=False, learning=False)
    # the trial held: an ordinary batch again
    p = cycle_policy(cycle=2, lowered=True)
    p.after_batch(maxit=2, maxneed=2, maxrel=0.06, maxprev=0.5)
    assert cycle_state(p) == dict(cycle=2, hold=0, backoff=2, lowered=False,
                                  learning=False)


def test_cycle_policy_learns_until_a_batch_keeps_its_cycle():
    # no solve NEEDED the last column and it stood at half the tolerance
    p = cycle_policy(cycle=3, learning=True)
    p.after_batch(maxit=3, maxneed=2, maxrel=0.05, maxprev=0.4)
    assert cycle_state(p) == dict(cycle=2, hold=0, backoff=2, lowered=True,
                                  learning=True)
    p.after_batch(maxit=2, maxneed=2, maxrel=0.4, maxprev=3.)
    assert cycle_state(p) == dict(cycle=2, hold=0, backoff=2, lowered=False,
                                  learning=False)
    # the same batch on a stepper that has learnt: no trial
    p = cycle_policy(cycle=3)
    p.after_batch(maxit=3, maxneed=2, maxrel=0.05, maxprev=0.4)
    assert p.cycle == 3 and not p.lowered
    # and not when a solve needed the column or the margin is thinner
    for maxneed, maxprev in ((3, 0.4), (2, 0.5)):
        p = cycle_policy(cycle=3, learning=True)
        p.after_batch(maxit=3, maxneed=maxneed, maxrel=0.05, maxprev=maxprev)
        assert cycle_state(p) == dict(cycle=3, hold=0, backoff=2,
                                      lowered=False, learning=False)


def test_cycle_policy_backs_off_by_four_up_to_4096():
    p = cycle_policy(cycle=2, lowered=True)
    for k, backoff in enumerate((8, 32, 128, 512, 2048, 4096, 4096, 4096)):
        p.after_fallback(1)
        assert cycle_state(p) == dict(cycle=3 + k, hold=backoff,
                                      backoff=backoff, lowered=False,
                                      learning=False)
        p.lowered = True                 # (the next trial, failing again)
    # a trial that went through but ended at the tolerance backs off as well
    p = cycle_policy(cycle=2, lowered=True, backoff=8)
    p.after_batch(maxit=2, maxneed=2, maxrel=1., maxprev=8.)
    assert cycle_state(p) == dict(cycle=3, hold=31, backoff=32,
                                  lowered=False, learning=False)
    # an established cycle that fails: no back-off, four batches of hold, the
    # cycle up to what the synchronous steps took
    p = cycle_policy(cycle=2, learning=True)
    p.after_fallback(5)
    assert cycle_state(p) == dict(cycle=5, hold=4, backoff=2, lowered=False,
                                  learning=True)
    p = cycle_policy(cycle=2, backoff=32)
    p.after_fallback(2)
    assert cycle_state(p) == dict(cycle=3, hold=32, backoff=32,
                                  lowered=False, learning=False)


def refresh_state(p):
    return p.level, p.tried


def test_refresh_policy_by_hand():
    for bound in (None, 0, 0.):
        p = dnp._RefreshPolicy(bound)
        assert not p.rebuild(100., True)
        assert refresh_state(p) == (None, False)
    p = dnp._RefreshPolicy(3.0)
    # behind the last batch: nothing, not even the level
    assert not p.rebuild(5., False) and refresh_state(p) == (None, False)
    # the first batch behind the set-up of the start, above the bound
    assert p.rebuild(5., True) and refresh_state(p) == (None, True)
    # the first batch behind THAT set-up is its level, wherever it is
    assert not p.rebuild(4., True) and refresh_state(p) == (4., True)
    # above the bound, not a fifth above the level
    assert not p.rebuild(4.75, True) and refresh_state(p) == (4., True)
    assert not p.rebuild(1.2*4., True)
    assert not p.rebuild(6., False) and refresh_state(p) == (4., True)
    assert p.rebuild(5., True) and refresh_state(p) == (None, True)
    assert not p.rebuild(2.5, True) and refresh_state(p) == (2.5, True)
    # a fifth above the level, not above the bound
    assert not p.rebuild(3.0, True) and refresh_state(p) == (2.5, True)
    assert p.rebuild(3.125, True) and refresh_state(p) == (None, True)
    # a first batch below the bound: no rebuild, and `tried` stays open
    p = dnp._RefreshPolicy(3.0)
    assert not p.rebuild(2., True) and refresh_state(p) == (2., False)
    assert p.rebuild(3.5, True) and refresh_state(p) == (None, True)


def test_the_policies_persist_as_the_sweep_documents():
    """one refresh policy per stepper, a cycle policy per sweep, hints keyed
    by the kind of sweep and written by sweeps longer than two batches only"""
    stp = model.ModelStepper(120, batch=32)
    refresh = stp._refresh
    script = model.thirds(120, (7, 9), (120, -5))
    for picard, nt, hints in ((True, 120, {False: 1}),
                              (False, 64, {False: 1}),
                              (False, 65, {False: 1, True: 1})):
        stp.script(script)
        stp.sweep(model.grid(nt), [1., -1.], 0, picard, record=False)
        assert stp._cycle_hint == hints
        assert stp._refresh is refresh and refresh.level == 1.0
    stp = model.ModelStepper(120, batch=32, oversolve=0.)
    stp.script(script)
    stp.sweep(model.grid(120), [1., -1.], 0, True, record=False)
    assert stp._cycle_hint == {}
