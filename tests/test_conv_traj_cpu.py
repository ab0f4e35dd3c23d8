"""The host side of the base trajectory of a linearised convection operator
(`convection.BaseTrajectory`, `csrc/conv_host.hpp`), without a device:

 * `BaseTrajectory.rows_at`: zero-order hold, the tolerance of
   `time_int_utils._checkuniformgrid`, `time_map`, both ends, and the
   `ValueError`s that name the time,
 * the shapes `BaseTrajectory` takes,
 * the layout arithmetic, the packing and every check of the host header under
   AddressSanitizer + UBSan (`tests/conv_traj_host_sanitize.cpp`, a program of
   its own),
 * the new entry points of the C boundary refuse null handles cleanly, and the
   library's messages about a base trajectory arrive as `ValueError`.
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


def test_rows_at_holds_the_last_stored_time(conv):
    t = conv.BaseTrajectory(0.5*np.arange(5), np.zeros((5, 3)), np.zeros(2))
    assert t.nrows == 5
    rows = t.rows_at([0., 0.1, 0.49, 0.5, 0.75, 1.0, 1.99, 2.0, 2.3, 2.5])
    assert rows.dtype == np.int32
    assert rows.tolist() == [0, 0, 0, 1, 1, 2, 3, 4, 4, 4]
    assert t.row_at(1.5) == 3 and isinstance(t.row_at(1.5), int)
    assert t.rows_at([]).size == 0


def test_rows_at_uses_the_tolerance_of_the_uniform_grid_check(conv):
    from dolfin_navier_scipy_amd import time_int_utils as tiu
    tol = conv.TIME_ATOL
    # (the tolerance is the one `_checkuniformgrid` accepts a grid with)
    tiu._checkuniformgrid([0., 1., 2. + 0.5*tol])
    with pytest.raises(NotImplementedError):
        tiu._checkuniformgrid([0., 1., 2. + 4*tol])
    dt = 1./512
    times = dt*np.arange(0, 13, 2)                # stored every second step
    t = conv.BaseTrajectory(times, np.zeros((7, 3)), np.zeros(2))
    # a time a rounding short of a stored one belongs to it
    assert t.rows_at([2*dt - 0.5*tol, 2*dt - 2*tol, 2*dt + 0.5*tol]).tolist() \
        == [1, 0, 1]
    # accumulated times, as a loop makes them
    acc, got = 0., []
    for _ in range(13):
        got.append(t.row_at(acc))
        acc += dt
    assert got == [k//2 for k in range(13)]
    # both ends within the tolerance
    assert t.row_at(-0.5*tol) == 0
    assert t.row_at(times[-1] + 2*dt + 0.5*tol) == 6


def test_rows_at_names_the_time_it_refuses(conv):
    t = conv.BaseTrajectory([1., 1.5, 2.], np.zeros((3, 3)), np.zeros(2))
    with pytest.raises(ValueError) as exc:
        t.rows_at([1., 0.75, 1.25])
    assert 'time 0.75' in str(exc.value)
    assert 'before the first stored time 1.0' in str(exc.value)
    # one storage interval behind the last is held, more is not
    assert t.rows_at([2.5]).tolist() == [2]
    with pytest.raises(ValueError) as exc:
        t.rows_at([2.25, 2.625])
    assert 'time 2.625' in str(exc.value)
    assert 'more than one storage interval (0.5)' in str(exc.value)
    assert 'last stored time 2.0' in str(exc.value)
    with pytest.raises(ValueError):
        t.rows_at([np.nan])
    # one stored flow holds for good, from its time on
    one = conv.BaseTrajectory([3.], np.zeros((1, 3)), np.zeros(2))
    assert one.rows_at([3., 1e6]).tolist() == [0, 0]
    with pytest.raises(ValueError):
        one.rows_at([2.9])


def test_time_map_walks_a_stored_run_backwards(conv):
    dt, T = 0.25, 2.0
    t = conv.BaseTrajectory(dt*np.arange(9), np.zeros((9, 3)), np.zeros(2),
                            time_map=lambda s: T - s)
    assert t.rows_at(dt*np.arange(9)).tolist() == list(range(8, -1, -1))
    # stored every second step: each row twice, descending
    t2 = conv.BaseTrajectory(2*dt*np.arange(5), np.zeros((5, 3)), np.zeros(2),
                             time_map=lambda s: T - s)
    assert t2.rows_at(dt*np.arange(9)).tolist() == [4, 3, 3, 2, 2, 1, 1, 0, 0]
    with pytest.raises(ValueError) as exc:
        t2.rows_at([2.25])
    # (the loop's time and the stored time it maps to)
    assert 'time 2.25' in str(exc.value) and '-0.25' in str(exc.value)


def test_shapes_of_a_base_trajectory(conv):
    for times in ([], [0., 0.], [1., 0.5], [0., np.inf]):
        with pytest.raises(ValueError):
            conv.BaseTrajectory(times, None, None)
    with pytest.raises(ValueError):
        conv.BaseTrajectory([0., 1.], np.zeros((3, 4)), np.zeros(2))
    with pytest.raises(ValueError):
        conv.BaseTrajectory([0., 1.], np.zeros(4), np.zeros(2))
    t = conv.BaseTrajectory([0., 1., 2.], np.zeros((3, 4)), np.arange(2.))
    sets, flat = t.resolve_dbcvals(2)
    assert sets == 1 and flat.tolist() == [0., 1.]
    t = conv.BaseTrajectory([0., 1., 2.], np.zeros((3, 4)),
                            np.arange(6.).reshape((3, 2)))
    sets, flat = t.resolve_dbcvals(2)
    assert sets == 3 and flat.tolist() == list(range(6))
    with pytest.raises(ValueError) as exc:
        t.resolve_dbcvals(3)
    assert '(3,) or (3, 3)' in str(exc.value)
    # no Dirichlet dofs: nothing to give; from full vectors: their entries
    assert conv.BaseTrajectory([0.], None, None).resolve_dbcvals(0)[0] == 1
    with pytest.raises(ValueError):
        conv.BaseTrajectory([0.], None, None).resolve_dbcvals(2)
    full = np.arange(12.).reshape((2, 6))
    sets, flat = conv.BaseTrajectory([0., 1.], full, None).resolve_dbcvals(
        2, full, np.array([1, 4]))
    assert sets == 2 and flat.tolist() == [1., 4., 7., 10.]


@pytest.mark.skipif(shutil.which('g++') is None, reason='needs g++')
def test_host_header_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / 'conv_traj_host_sanitize')
    build = subprocess.run(
        ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all', '-Wall', '-Wextra', '-Werror',
         '-I' + os.path.join(ROOT, 'include'),
         os.path.join(HERE, 'conv_traj_host_sanitize.cpp'), '-o', exe],
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
    """(`tests/test_capi_cpu.py` loads the library without a device the same
    way; an operator needs one, so the checks behind the handle are the
    sanitized program's and the GPU tests')"""
    import ctypes as ct
    from dolfin_navier_scipy_amd.build import build_library
    build_library(verbose=False)
    from dolfin_navier_scipy_amd import _capi
    lib = _capi.load_library()
    v = np.zeros(4)
    r = np.zeros(2, dtype=np.int32)
    a, b = ct.c_int32(7), ct.c_int32(7)
    for status in (
            lib.dns_conv_set_base_trajectory(None, 1, _capi.dptr(v), 4, 1,
                                             _capi.dptr(v), 0),
            lib.dns_conv_set_base_rows(None, 2,
                                       r.ctypes.data_as(_capi.c_int32_p)),
            lib.dns_conv_set_base_row(None, 0),
            lib.dns_conv_get_base_info(None, ct.byref(a), ct.byref(b)),
            lib.dns_imex_ensemble_to_base(None, 0, 1, None, 1, _capi.dptr(v),
                                          0)):
        assert status == _capi.DNS_ERR_BAD_ARGUMENT
        assert b'null' in lib.dns_last_error()
    assert (a.value, b.value) == (7, 7)


def test_messages_about_a_base_trajectory_are_value_errors():
    from dolfin_navier_scipy_amd import _capi
    assert issubclass(_capi.LinearisedRefusal, ValueError)
    src = open(os.path.join(ROOT, 'dolfin_navier_scipy_amd', 'csrc',
                            'conv_host.hpp')).read()
    # every message of the header starts the way `_capi.check` looks for
    msgs = [m for m in src.split('fail(DNS_ERR_BAD_ARGUMENT,')[1:]]
    assert len(msgs) >= 12
    for m in msgs:
        assert m.lstrip().startswith('"linearised convection'), m[:80]
