"""A scripted stand-in for the device behind `TrapezoidalStepper.sweep`, so
that the sweep -- all of it host Python: the batches, their cycle lengths, the
replays and the rebuilds of the preconditioner -- runs without a device.

`ModelStepper` is a `TrapezoidalStepper` whose `__init__` opens no library and
which overrides the device-facing methods the sweep calls, nothing else:
`start`, `write_linpoint`, `step`, `run`, `state`, `checkpoint`,
`set_pipeline`, `poll`, `restore`, `refresh_precond`, `update_norm` (and
`close` / `__del__`).  Every call is appended to `log` with its arguments,
`run` as ONE entry.

THE RULE.  A sweep is scripted by `third` (`script()`): the start residual of
the solve of step `k` is `2**third[k]` x tolerance and every Krylov column
divides it by 8, so the solve NEEDS `need = max(1, ceil(third[k]/3))` columns
and stands at `rel(j) = 2**(third[k] - 3 j)` x tolerance behind column `j`
(powers of two: every figure below is exact in floating point).  Several
lists are the stages of the preconditioner: list `r` holds behind the `r`-th
`refresh_precond` since `script()` (the last one from then on).

 * a synchronous step (`set_pipeline(0)`) runs `need` columns and reports
   `iters = need`, `device_seconds = need/1024`;
 * under `set_pipeline(c)` a solve with `need > c` is a failure (`fails`, its
   `c` columns in `iters`, nothing else).  The others run `j = need` columns,
   or with oversolve on `j = min(c, max(need, ceil((third[k] + 10)/3)))`: on to
   the floor of 2**-10 x tolerance or to the end of the cycle.  `poll()`
   returns and clears `solves`, `fails`, `iters` (sum of `j`), `maxit` (max
   `j`), `maxneed`, `sumneed`, `maxrel = max rel(j)` and `maxprev = max
   rel(j - 1)`.

`SCENARIOS` are sequences of sweeps on one stepper; `run_scenario` returns
what `tests/golden/trap_sweep_calls.json` pins: per sweep the call log, the
returned statistics, the update norm, the recorded times and the stepper's
`refreshes`."""
import numpy as np

from dolfin_navier_scipy_amd import newton_picard as dnp

NV, NP = 2, 1
DT = 2.0**-7
FLOOR = 10                   # oversolve runs on to 2**-FLOOR x tolerance


def _ceil3(q):
    return -((-q)//3)


class ModelStepper(dnp.TrapezoidalStepper):

    def __init__(self, nslots, batch=64, refresh_iters=3.0, oversolve=1e-3):
        # the attributes the sweep reads, as `TrapezoidalStepper.__init__`
        # leaves them
        self.nslots, self.NV, self.NP = int(nslots), NV, NP
        self.batch = int(batch)
        self.refreshes = 0
        self.last_stats = None
        self._over = float(oversolve or 0.0) > 0.0
        self._cycle_hint = {}
        if hasattr(dnp, '_RefreshPolicy'):
            self._refresh = dnp._RefreshPolicy(refresh_iters)
        else:
            # (the commit the golden file was made at: the state of the
            # refresh policy as attributes of the stepper)
            self.refresh_iters = refresh_iters
            self._level, self._tried = None, False
        # the model's own
        self.log = []
        self.stages, self.stage = [[]], 0
        self.cycle, self.last_slot, self.sweeps = 0, 0, 0
        self._clear()

    def script(self, *stages):
        self.stages, self.stage = [list(s) for s in stages], 0

    def close(self):
        pass

    def __del__(self):
        pass

    def _clear(self):
        self.acc = dict(solves=0, fails=0, iters=0, maxit=0, maxneed=0,
                        sumneed=0, maxrel=0., maxprev=0.)

    def _solve(self, k):
        third = self.stages[min(self.stage, len(self.stages) - 1)][k]
        need = max(1, _ceil3(third))
        self.last_slot = k
        if self.cycle == 0:
            return dict(iters=need, device_seconds=need/1024., status=0)
        acc, c = self.acc, self.cycle
        acc['solves'] += 1
        if need > c:
            acc['fails'] += 1
            acc['iters'] += c
        else:
            j = min(c, max(need, _ceil3(third + FLOOR))) if self._over \
                else need
            acc['iters'] += j
            acc['maxit'] = max(acc['maxit'], j)
            acc['maxneed'] = max(acc['maxneed'], need)
            acc['sumneed'] += need
            acc['maxrel'] = max(acc['maxrel'], 2.0**(third - 3*j))
            acc['maxprev'] = max(acc['maxprev'], 2.0**(third - 3*(j - 1)))
        return dict(iters=0, device_seconds=0., status=0)

    # -- what the sweep calls --------------------------------------------
    def start(self, iniv, newton):
        self.sweeps += 1
        self.log.append(['start', np.asarray(iniv).reshape(-1).tolist(),
                         bool(newton)])

    def write_linpoint(self, which, slot, v):
        self.log.append(['write_linpoint', int(which), int(slot),
                         np.asarray(v).reshape(-1).tolist()])

    def step(self, dt, lin_which, lin_slot, out_slot, newton, opts=None,
             extrapolate=4, raise_on_fail=True, feedback=None):
        fb = None if feedback is None else [
            None if m is None else float(np.sum(m)) for m in feedback]
        self.log.append(['step', float(dt), int(lin_which), int(lin_slot),
                         int(out_slot), bool(newton), opts, int(extrapolate),
                         bool(raise_on_fail), fb])
        self.last_stats = self._solve(int(out_slot))
        return self.last_stats

    def run(self, dt, lin_which, slot0, count, newton, opts=None,
            extrapolate=4):
        self.log.append(['run', int(slot0), int(count), self.cycle, float(dt),
                         int(lin_which), bool(newton), opts,
                         int(extrapolate)])
        for k in range(int(slot0), int(slot0) + int(count)):
            self._solve(k)

    def state(self):
        self.log.append(['state'])
        return (np.full((NV, 1), float(self.last_slot)),
                np.full((NP, 1), -float(self.last_slot)))

    def checkpoint(self):
        self.log.append(['checkpoint'])

    def set_pipeline(self, cycle_len):
        self.log.append(['set_pipeline', int(cycle_len)])
        self.cycle = int(cycle_len)
        self._clear()

    def poll(self):
        acc = self.acc
        self._clear()
        self.log.append(['poll', dict(acc)])
        return acc

    def restore(self, newton):
        self.log.append(['restore', bool(newton)])

    def refresh_precond(self):
        self.log.append(['refresh_precond'])
        self.stage += 1
        self.refreshes += 1

    def update_norm(self):
        self.log.append(['update_norm'])
        return 2.0**-self.sweeps


def grid(nt, odd_step=None):
    """`nt` time instances `DT` apart; `odd_step`: that step takes `2 DT`"""
    steps = np.full(nt - 1, DT)
    if odd_step is not None:
        steps[odd_step] *= 2.
    return np.concatenate([[0.], np.cumsum(steps)])


def thirds(nt, *pieces):
    """the script of a sweep over `nt` instances: `pieces` are `(upto, third)`
    -- `third` holds for the steps below `upto` that no earlier piece took
    (entry 0 is no step: slot 0 holds the initial value)"""
    out, k = [], 0
    for upto, third in pieces:
        out += [third]*(min(upto, nt) - k)
        k = max(k, min(upto, nt))
    assert len(out) == nt, (len(out), nt)
    return out


def feedback(t):
    """a closed loop's low-rank terms: `umat` the same at every instance"""
    return np.ones((NV, 1)), np.full((1, NV), float(round(t/DT)))


# name -> (keywords of the stepper, sweeps); a sweep is (picard, nt, stages of
# thirds, keywords of `sweep` -- `record=False` unless given).  Picard, then
# Newton after Newton, as `newton_picard` runs them; what each scenario is
# there for is asserted on the golden file in `tests/test_trap_sweep_cpu.py`
def _scenarios():
    S = {}
    # start-up needs 3 columns, the run 2 with a margin: learning batches of
    # 16 on the first sweep of a kind, the floor reached early (shrink to
    # maxit), the second Newton sweep starts from the hint
    calm = [thirds(120, (7, 9), (120, -5))]
    S['learn_shrink_hint'] = (dict(batch=32), [
        (True, 120, calm, {}), (False, 120, calm, {}),
        (False, 120, [thirds(120, (7, 12), (120, -5))], {})])
    # a batch ends AT the tolerance (third = 3 c): one more column, no replay
    S['raise_without_replay'] = (dict(batch=16), [
        (True, 100, [thirds(100, (40, 3), (56, 6), (100, 3))], {}),
        (False, 100, [thirds(100, (40, 3), (56, 6), (100, 3))], {})])
    # three columns run, the residual in front of the last one a decade below
    # the tolerance: a trial batch of two columns, which holds
    S['trial_holds'] = (dict(batch=32), [
        (True, 140, [thirds(140, (7, 9), (140, 2))], {}),
        (False, 140, [thirds(140, (7, 9), (140, 2))], {}),
        (False, 140, [thirds(140, (7, 9), (140, 2))], {})])
    # the trial batch meets a step that needs the third column: replay, and
    # the next trial waits 8 batches instead of 1
    S['trial_fails_backoff'] = (dict(batch=16), [
        (False, 200, [thirds(200, (7, 9), (30, 2), (31, 7), (200, 2))], {})])
    # the trial batch goes through, but ends at the tolerance: back up, and
    # the wait is 8 batches as well
    S['trial_ends_at_tolerance'] = (dict(batch=16), [
        (False, 200, [thirds(200, (7, 9), (30, 2), (31, 6), (200, 2))], {})])
    # a step beyond the cycle in an established batch, oversolve on and off
    spike = [thirds(110, (50, 5), (51, 11), (110, 5))]
    S['fallback_oversolve'] = (dict(batch=16), [
        (True, 110, spike, {}), (False, 110, spike, dict(record=True))])
    S['fallback_slack_column'] = (dict(batch=16, oversolve=0.), [
        (True, 110, spike, {}), (False, 110, spike, {})])
    # the form without oversolve: max(2, maxit + 1), batches of `batch` from
    # the first one on, no hints
    S['slack_column'] = (dict(batch=32, oversolve=0.), [
        (True, 130, [thirds(130, (7, 9), (60, 1), (130, 5))], {}),
        (False, 130, [thirds(130, (7, 9), (60, 1), (130, 5))],
         dict(record=True))])
    # step by step: a non-uniform grid, a closed loop, `pipeline=False`, and a
    # grid too short to be called uniform
    S['step_by_step'] = (dict(batch=16), [
        (True, 40, [thirds(40, (40, 5))], dict(odd_step=20)),
        (False, 40, [thirds(40, (40, 5))], dict(feedback=feedback)),
        (False, 40, [thirds(40, (40, 5))], dict(pipeline=False)),
        (False, 8, [thirds(8, (8, 5))], {})])
    # the set-up of the start was made for another state: the first batch is
    # above the bound, ONE rebuild, the batches behind it are below
    stale = [thirds(100, (100, 11)), thirds(100, (100, 5))]
    S['refresh_first_batch'] = (dict(batch=16), [
        (True, 100, stale, {}), (False, 100, [thirds(100, (100, 5))], {})])
    # the flow moves away from the set-up: a later batch above the bound and a
    # fifth above the level rebuilds; what the rebuild gives stays above the
    # bound (tight tolerance) and must not rebuild batch after batch -- nor in
    # the next sweep, until it rises by a fifth again
    drift = [thirds(150, (60, 5), (150, 11)), thirds(150, (150, 10))]
    S['refresh_later_then_out_of_reach'] = (dict(batch=16), [
        (True, 150, drift, {}),
        (False, 150, [thirds(150, (150, 10))], {}),
        (False, 150, [thirds(150, (100, 10), (150, 14)),
                      thirds(150, (150, 11))], {})])
    # the same drift without a bound, and with a bound of 0
    S['refresh_never'] = (dict(batch=16, refresh_iters=None), [
        (True, 150, drift, {}), (False, 150, drift, {})])
    S['refresh_bound_zero'] = (dict(batch=16, refresh_iters=0), [
        (True, 150, drift, {})])
    # the LAST batch is the one above the bound: listed, not rebuilt; the same
    # batch with steps behind it is
    late = [thirds(119, (87, 5), (119, 11)), thirds(119, (119, 5))]
    S['refresh_not_behind_last_batch'] = (dict(batch=16), [
        (True, 103, [s[:103] for s in late], {}), (False, 119, late, {})])
    # the refresh policy without oversolve goes by the columns run
    S['refresh_slack_column'] = (dict(batch=16, oversolve=0.), [
        (True, 100, stale, {}),
        (False, 100, [thirds(100, (40, 5), (100, 11)),
                      thirds(100, (100, 5))], {})])
    return S


SCENARIOS = _scenarios()


def run_scenario(name, stepper_cls=ModelStepper):
    """the sweeps of a scenario on one stepper: per sweep a dict of the call
    log, `tot`, the update norm, the recorded times and `refreshes`"""
    skw, sweeps = SCENARIOS[name]
    nslots = max(nt for _, nt, _, _ in sweeps)
    stp = stepper_cls(nslots, **skw)
    out, which = [], 0
    for picard, nt, stages, kw in sweeps:
        kw = dict(dict(record=False), **kw)
        trange = grid(nt, kw.pop('odd_step', None))
        stp.script(*stages)
        stp.log = []
        vdict, pdict, norm, tot = stp.sweep(
            trange, np.array([1., -1.]), which, picard,
            opts='opts-{0}'.format(len(out)),
            extrapolate=3 + len(out), **kw)
        assert stp.last_stats is None or stp.last_stats['status'] == 0
        for k, t in enumerate(trange):       # (`state()` behind step k)
            assert t not in pdict or vdict[t][0, 0] == -pdict[t][0, 0] == k
        out.append(dict(log=stp.log, tot=tot, norm=norm,
                        vtimes=sorted(vdict), ptimes=sorted(pdict),
                        refreshes=stp.refreshes))
        which = 1 - which
    return out
