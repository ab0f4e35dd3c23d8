"""`bench.py --gpus 1` without `--full`: the headline window alone, `--steps`
timed steps, and `--dump-outputs` writing the state the last timed step
leaves -- the same state from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(outdir, steps):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1',
           '--steps', str(steps), '--warmup', '4', '--spinup', '8',
           '--dump-outputs', str(outdir)]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    lines = [ln for ln in out.stdout.decode().splitlines()
             if ln.startswith('{')]
    assert len(lines) == 1, out.stdout.decode()[-2000:]
    return json.loads(lines[0])


def test_plain_line_and_dumped_state(tmp_path):
    rec = _plain_run(tmp_path / 'a', 24)
    assert rec['steps'] == 24 and rec['warmup'] == 4
    assert rec['unit'] == 'timesteps/s' and rec['higher_is_better'] is True
    assert rec['dtype'] == 'f64' and rec['ms_per_step'] > 0.
    assert abs(rec['value']*rec['ms_per_step'] - 1e3) <= 1e-3*1e3
    cfg = rec['config']
    # (the secondary legs are --full's)
    assert rec['cpu_baseline'] is None and rec['parity'] is None
    for key in ('window_400', 'early_transient', 'row_partitioned',
                'newton_picard_sweeps', 'refined_mesh'):
        assert cfg[key] is None, key
    assert cfg['timed_run_record']['unconverged'] == 0
    v = np.load(str(tmp_path / 'a' / 'v.npy'))
    p = np.load(str(tmp_path / 'a' / 'p.npy'))
    assert v.dtype == np.float64 and p.dtype == np.float64
    assert 'NV={0} NP={1}'.format(v.size, p.size) in cfg['workload']
    assert np.all(np.isfinite(v)) and np.all(np.isfinite(p))
    assert np.linalg.norm(v) > 0. and np.linalg.norm(p) > 0.
    # same arguments, same inputs: the same state up to the solver tolerance
    _plain_run(tmp_path / 'b', 24)
    v2 = np.load(str(tmp_path / 'b' / 'v.npy'))
    p2 = np.load(str(tmp_path / 'b' / 'p.npy'))
    assert np.linalg.norm(v2 - v) <= 1e-8*np.linalg.norm(v)
    assert np.linalg.norm(p2 - p) <= 1e-8*np.linalg.norm(p)
