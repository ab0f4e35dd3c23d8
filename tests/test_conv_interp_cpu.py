"""The host side of linear interpolation between the stored rows of a base
trajectory (`convection.BaseTrajectory(interpolate=True)`, `weights_at`,
`csrc/conv_host.hpp`), without a device:

 * `weights_at`: weight exactly 0 at and within `TIME_ATOL` of a stored time
   (on either side), midpoints, non-uniform stored times, a `time_map` walking
   backwards, accumulated loop times, and the `ValueError`s by the time they
   name -- no extrapolation, the one-interval hold of `rows_at` does not apply,
 * `lerp_rows` / `flow_at`: the three-operation formula,
 * how `time_int_utils` arms an operator from a trajectory of either kind,
 * the checks of the weights in the host header under AddressSanitizer + UBSan
   (`tests/conv_interp_host_sanitize.cpp`, a program of its own),
 * the new entry points refuse null handles cleanly, and the messages about
   weights arrive as `ValueError`.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope='module')
def conv():
    from dolfin_navier_scipy_amd import convection
    return convection


def _traj(conv, times, **kw):
    times = np.asarray(times, dtype=float)
    return conv.BaseTrajectory(times, np.zeros((times.size, 3)), np.zeros(2),
                               interpolate=True, **kw)


def test_stored_times_have_weight_exactly_zero(conv):
    tol = conv.TIME_ATOL
    t = _traj(conv, 0.5*np.arange(5))
    assert t.interpolate and not conv.BaseTrajectory(
        [0., 1.], np.zeros((2, 3)), np.zeros(2)).interpolate
    rows, th = t.weights_at([0., 0.5, 1.0, 1.5, 2.0])
    assert rows.dtype == np.int32 and th.dtype == np.float64
    assert rows.tolist() == [0, 1, 2, 3, 4]
    assert np.array_equal(th, np.zeros(5)) and not np.any(np.signbit(th))
    # within the tolerance, on either side: that row, weight 0 -- a time just
    # short of the NEXT stored time is the next row, not weight 1 - eps
    rows, th = t.weights_at([1.0 - 0.5*tol, 1.0 + 0.5*tol, -0.5*tol,
                             2.0 - 0.5*tol, 2.0 + 0.5*tol])
    assert rows.tolist() == [2, 2, 0, 4, 4]
    assert np.array_equal(th, np.zeros(5))
    # outside the tolerance the weight is the small (or nearly one) it is
    rows, th = t.weights_at([1.0 + 4*tol, 1.0 - 4*tol])
    assert rows.tolist() == [2, 1]
    assert th[0] == (1.0 + 4*tol - 1.0)/0.5 and 0 < th[0] < 1e-6
    assert 1 - 1e-6 < th[1] < 1.0
    e = t.weights_at([])
    assert e[0].size == 0 and e[1].size == 0
    # rows are those of `rows_at`
    ts = np.linspace(0., 2., 33)
    assert np.array_equal(t.weights_at(ts)[0], t.rows_at(ts))


def test_midpoints_and_non_uniform_stored_times(conv):
    t = _traj(conv, 0.5*np.arange(5))
    rows, th = t.weights_at([0.25, 0.125, 1.875, 0.5 + 1./6])
    assert rows.tolist() == [0, 0, 3, 1]
    assert th[:3].tolist() == [0.5, 0.25, 0.75]
    assert th[3] == (0.5 + 1./6 - 0.5)/0.5
    times = np.array([0., 0.1, 0.4, 1.0, 1.0625])
    t = _traj(conv, times)
    ts = [0.05, 0.1, 0.25, 0.7, 1.0, 1.03125, 1.0625]
    rows, th = t.weights_at(ts)
    assert rows.tolist() == [0, 1, 1, 2, 3, 3, 4]
    for k, (r, w) in enumerate(zip(rows, th)):
        if ts[k] in times:
            assert w == 0.0
        else:
            assert w == (ts[k] - times[r])/(times[r + 1] - times[r])
            assert 0.0 < w < 1.0
    assert th[5] == 0.5
    # accumulated times, as a loop makes them: stored every fourth step
    dt = 1./512
    t = _traj(conv, 4*dt*np.arange(4))
    acc, got = 0., []
    for _ in range(13):
        got.append(t.weights_at([acc]))
        acc += dt
    assert [int(g[0][0]) for g in got] == [k//4 for k in range(13)]
    assert [float(g[1][0]) for g in got] == [(k % 4)/4. for k in range(13)]


def test_time_map_walks_a_stored_run_backwards(conv):
    dt, T = 0.25, 2.0
    t = _traj(conv, 4*dt*np.arange(3), time_map=lambda s: T - s)
    rows, th = t.weights_at(dt*np.arange(9))
    assert rows.tolist() == [2, 1, 1, 1, 1, 0, 0, 0, 0]
    assert th.tolist() == [0., .75, .5, .25, 0., .75, .5, .25, 0.]
    # a non-zero weight never stands on the last row
    assert np.all(rows[th != 0] + 1 < t.nrows)
    with pytest.raises(ValueError) as exc:
        t.weights_at([0.5, 2.25])
    assert 'time 2.25' in str(exc.value) and '-0.25' in str(exc.value)
    assert 'before the first stored time 0.0' in str(exc.value)
    with pytest.raises(ValueError) as exc:
        t.weights_at([-0.125])
    assert 'time -0.125' in str(exc.value) and '2.125' in str(exc.value)
    assert 'behind the last stored time 2.0' in str(exc.value)


def test_no_extrapolation_behind_the_last_stored_time(conv):
    tol = conv.TIME_ATOL
    t = _traj(conv, [1., 1.5, 2.])
    # `rows_at` holds the last row for one interval, `weights_at` does not
    assert t.rows_at([2.25]).tolist() == [2]
    with pytest.raises(ValueError) as exc:
        t.weights_at([1.25, 2.25])
    assert 'base trajectory: time 2.25' in str(exc.value)
    assert 'behind the last stored time 2.0' in str(exc.value)
    assert 'does not extrapolate' in str(exc.value)
    with pytest.raises(ValueError) as exc:
        t.weights_at([2.0 + 4*tol])
    assert 'behind the last stored time' in str(exc.value)
    assert t.weights_at([2.0 + 0.5*tol])[1][0] == 0.0
    with pytest.raises(ValueError) as exc:
        t.weights_at([1., 0.75])
    assert 'time 0.75' in str(exc.value)
    assert 'before the first stored time 1.0' in str(exc.value)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            t.weights_at([bad])
    # one stored flow: its own time and nothing else
    one = _traj(conv, [3.])
    assert one.weights_at([3.])[0].tolist() == [0]
    assert one.rows_at([1e6]).tolist() == [0]
    with pytest.raises(ValueError):
        one.weights_at([3.5])
    # `rows_at` is what it was, whatever the flag
    assert t.rows_at([1., 1.25, 1.5, 2.4]).tolist() == [0, 0, 1, 2]


def test_lerp_rows_is_the_three_operation_formula(conv):
    rng = np.random.default_rng(7)
    v0, v1 = rng.standard_normal(200), rng.standard_normal(200)
    for th in (0.5, 0.25, 1./3, 2.0**-60, 1 - 2.0**-53, 0.0):
        got = conv.lerp_rows(v0, v1, th)
        want = np.array([a + th*(b - a) for a, b in zip(v0.tolist(),
                                                        v1.tolist())])
        assert np.array_equal(got, want)
    assert np.array_equal(conv.lerp_rows(v0, v1, 0.0), v0)
    times = np.array([0., 1., 3.])
    rows = rng.standard_normal((3, 6))
    t = conv.BaseTrajectory(times, rows, np.zeros(2), interpolate=True)
    assert np.array_equal(t.flow_at(1.0), rows[1])
    assert np.array_equal(t.flow_at(2.0), rows[1] + 0.5*(rows[2] - rows[1]))
    assert np.array_equal(t.flow_at(3.0), rows[2])
    held = conv.BaseTrajectory(times, rows, np.zeros(2))
    assert np.array_equal(held.flow_at(2.0), rows[1])


class _FakeConv(object):
    def __init__(self):
        self.calls = []

    def set_base_rows(self, *args):
        self.calls.append(('rows',) + tuple(np.asarray(a).tolist()
                                            for a in args))

    def set_base_row(self, *args):
        self.calls.append(('row',) + args)


def test_the_loops_arm_weights_only_for_an_interpolating_trajectory(conv):
    from dolfin_navier_scipy_amd import time_int_utils as tiu
    ts = [0., 0.25, 0.5, 0.75, 1.0]
    held = conv.BaseTrajectory([0., 1.], np.zeros((2, 3)), np.zeros(2))
    lerp = _traj(conv, [0., 1.])
    cv = _FakeConv()
    tiu._arm_base_rows(cv, held, ts)
    tiu._arm_base_row(cv, held, 0.5)
    tiu._arm_base_rows(cv, lerp, ts)
    tiu._arm_base_row(cv, lerp, 0.75)
    tiu._arm_base_row(cv, lerp, 1.0)
    assert cv.calls == [('rows', [0, 0, 0, 0, 1]), ('row', 0),
                        ('rows', [0, 0, 0, 0, 1], [0., .25, .5, .75, 0.]),
                        ('row', 0, 0.75), ('row', 1, 0.0)]
    # the coverage check before the loop: held one interval, never extrapolated
    assert tiu._base_rows_at(held, [1.5])[1] is None
    with pytest.raises(ValueError) as exc:
        tiu._base_rows_at(lerp, [0.5, 1.5])
    assert 'time 1.5' in str(exc.value)


def test_interpolated_base_gains_an_order_over_the_held_one():
    """`scripts/base_interp_accuracy.py` (host model only): a tangent run about
    a smooth analytic base flow stored every fourth step.  Measured: held
    0.120 -> 0.057 (ratio 2.10), interpolated 5.2e-3 -> 1.2e-3 (ratio 4.21)
    from dt = 1/64 to 1/128.  Asserted: no more than that the interpolated
    error falls by more than the held one"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import base_interp_accuracy as bia
    finally:
        sys.path.remove(os.path.join(ROOT, 'scripts'))
    import scenarios
    rec = bia.measure(scenarios.toy_problem(nx=11, ny=4))
    print(rec)
    assert rec['interpolated'][0] < rec['held'][0]
    assert rec['interpolated'][1] < rec['held'][1]
    assert rec['ratio_interpolated'] > rec['ratio_held'] > 1.0


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_weight_checks_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / 'conv_interp_host_sanitize')
    build = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror',
         '-I' + os.path.join(ROOT, 'include'),
         os.path.join(HERE, 'conv_interp_host_sanitize.cpp'), '-o', exe],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert build.returncode == 0, build.stdout.decode()[-4000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0',
               UBSAN_OPTIONS='print_stacktrace=1')
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=600)
    out = run.stdout.decode()
    assert run.returncode == 0, out[-4000:]
    assert 'all checks passed' in out
    assert 'runtime error' not in out and 'AddressSanitizer' not in out, out


def test_new_entry_points_refuse_null_handles():
    import ctypes as ct
    from dolfin_navier_scipy_amd.build import build_library
    build_library(verbose=False)
    from dolfin_navier_scipy_amd import _capi
    lib = _capi.load_library()
    r = np.zeros(2, dtype=np.int32)
    w = np.zeros(2)
    a = ct.c_int32(7)
    for status in (
            lib.dns_conv_set_base_rows_lerp(
                None, 2, r.ctypes.data_as(_capi.c_int32_p), _capi.dptr(w)),
            lib.dns_conv_set_base_row_lerp(None, 0, 0.5),
            lib.dns_conv_get_base_lerp(None, ct.byref(a))):
        assert status == _capi.DNS_ERR_BAD_ARGUMENT
        assert b'null' in lib.dns_last_error()
    assert a.value == 7


def test_messages_about_weights_are_value_errors():
    from dolfin_navier_scipy_amd import _capi
    assert issubclass(_capi.LinearisedRefusal, ValueError)
    src = open(os.path.join(ROOT, 'dolfin_navier_scipy_amd', 'csrc',
                            'conv_host.hpp')).read()
    body = src.split('inline int check_base_weight')[1].split(
        'inline int check_base_row_lerp')[0]
    msgs = body.split('fail(DNS_ERR_BAD_ARGUMENT,')[1:]
    assert len(msgs) == 3
    for m in msgs:
        assert m.lstrip().startswith('"linearised convection'), m[:80]
