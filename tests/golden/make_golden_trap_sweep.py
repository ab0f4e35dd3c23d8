"""Record what `TrapezoidalStepper.sweep` does with the scripted stepper of
`tests/trap_sweep_model.py`: every call on the stepper, in order and with its
arguments, and what the sweep returns.

    python tests/golden/make_golden_trap_sweep.py

runs the `SCENARIOS` of the model through the `sweep` of the tree it is called
in and writes `tests/golden/trap_sweep_calls.json`: the commit it was made at
(the script refuses a tree whose `newton_picard.py` differs from that commit)
and per scenario, per sweep, `log`, `tot`, `norm`, `vtimes`, `ptimes` and
`refreshes` as `trap_sweep_model.run_scenario` returns them.  Floats are
written by `repr` (`json`), so they read back bit for bit.

The file pins the sweep as it stood BEFORE it was split into a loop, a cycle
policy and a refresh policy; `tests/test_trap_sweep_cpu.py` replays the
scenarios on the tree's code and asks for equality.  Run it again only to pin
a change of behaviour that is meant."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

MODULE = 'dolfin_navier_scipy_amd/newton_picard.py'


def git(*args):
    return subprocess.check_output(('git',) + args, cwd=ROOT).decode().strip()


def dumps(commit, scenarios):
    """one call of the log per line"""
    js = json.dumps
    out = ['{', ' "commit": {0},'.format(js(commit)), ' "scenarios": {']
    for i, (name, sweeps) in enumerate(scenarios.items()):
        out.append('  {0}: ['.format(js(name)))
        for j, sw in enumerate(sweeps):
            out.append('   {')
            for key in ('tot', 'norm', 'vtimes', 'ptimes', 'refreshes'):
                out.append('    {0}: {1},'.format(js(key), js(sw[key])))
            out.append('    "log": [')
            out.append(',\n'.join('     ' + js(e) for e in sw['log']))
            out.append('    ]')
            out.append('   }' + (',' if j + 1 < len(sweeps) else ''))
        out.append('  ]' + (',' if i + 1 < len(scenarios) else ''))
    out += [' }', '}', '']
    return '\n'.join(out)


def main():
    import trap_sweep_model as model
    if git('status', '--porcelain', '--', MODULE):
        raise SystemExit(MODULE + ' differs from the commit: not recorded')
    commit = git('rev-parse', 'HEAD')
    scenarios = {name: model.run_scenario(name) for name in model.SCENARIOS}
    text = dumps(commit, scenarios)
    assert json.loads(text)['scenarios'] == json.loads(json.dumps(scenarios))
    fn = os.path.join(HERE, 'trap_sweep_calls.json')
    with open(fn, 'w') as fh:
        fh.write(text)
    print(fn, len(text), 'bytes,', len(scenarios), 'scenarios,',
          sum(len(s) for s in scenarios.values()), 'sweeps, at', commit)


if __name__ == '__main__':
    main()
