"""Trajectory recorder of the explicit loops, host side: the entry points
(header, ctypes table, exports of the cross-compiled library, null handles),
the slot / chunk planner of `time_int_utils` and the argument checks that
`ImexStepper.set_recorder` makes in Python.  No device."""
import os
import re
import types

import numpy as np
import pytest
import scipy.sparse as sps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ('dns_imex_set_recorder', 'dns_imex_get_record_outputs',
               'dns_imex_get_record_snapshots', 'dns_imex_clear_recorder')


def test_header_declares_and_capi_binds_the_recorder_entry_points():
    from dolfin_navier_scipy_amd import _capi
    hdr = open(os.path.join(ROOT, 'include', 'dns_amd.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(dns_[a-z0-9_]+)\s*\(', hdr))
    lib = _capi.load_library()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _capi.SIGNATURES, name
        assert hasattr(lib, name), name
    # null handles fail cleanly, with a message
    calls = ((lib.dns_imex_set_recorder, (None, None, 4, None, 0)),
             (lib.dns_imex_get_record_outputs, (None, 0, 1, None)),
             (lib.dns_imex_get_record_snapshots, (None, 0, 1, None, None)),
             (lib.dns_imex_clear_recorder, (None,)))
    for fn, args in calls:
        assert fn(*args) == _capi.DNS_ERR_BAD_ARGUMENT
        assert b'null' in lib.dns_last_error()


def test_record_kernel_is_a_dependency_of_the_build():
    from dolfin_navier_scipy_amd import build
    names = [os.path.basename(p) for p in build.dependencies()]
    assert 'record.hpp' in names
    text = open(os.path.join(ROOT, 'dolfin_navier_scipy_amd', 'csrc',
                             'imex.hpp')).read()
    assert '#include "record.hpp"' in text


# ---- the planner --------------------------------------------------------------

def _check_plan(chunks, ns, kept_steps):
    """the chunks tile the slice, every chunk ends with a kept step, the slots
    of a chunk count up from 0, and the kept steps are the expected ones"""
    pos, kept = 0, []
    for ch in chunks:
        assert ch['first'] == pos and ch['nsteps'] >= 1
        assert ch['slots'].dtype == np.int32
        assert ch['slots'].shape == (ch['nsteps'],)
        local = [(ch['first'] + i, int(s))
                 for i, s in enumerate(ch['slots']) if s >= 0]
        assert local == ch['kept']
        assert [s for _, s in local] == list(range(len(local)))
        assert local and local[-1][0] == ch['first'] + ch['nsteps'] - 1
        assert set(ch['slots'][ch['slots'] < 0].tolist()) <= {-1}
        kept += [s for s, _ in local]
        pos += ch['nsteps']
    assert pos == ns
    assert kept == kept_steps


def test_plan_keeps_every_step_for_none():
    from dolfin_navier_scipy_amd.time_int_utils import plan_record
    t = (0.5 + 0.01*np.arange(9)).tolist()
    chunks = plan_record(t, None, snap_bytes=800)
    assert len(chunks) == 1
    _check_plan(chunks, 9, list(range(9)))


def test_plan_keeps_the_save_times_and_always_the_last_step():
    from dolfin_navier_scipy_amd.time_int_utils import plan_record
    t = (0.5 + 0.01*np.arange(10)).tolist()
    chunks = plan_record(t, {t[0], t[3], t[6], 17.0}, snap_bytes=800)
    assert len(chunks) == 1
    _check_plan(chunks, 10, [0, 3, 6, 9])
    # no time of the slice wanted: the last step still is (the loop goes on
    # from it), and for SBDF2 the one before it (blow-up guard)
    _check_plan(plan_record(t, set(), 800), 10, [9])
    _check_plan(plan_record(t, set(), 800, keep_prev=True), 10, [8, 9])
    _check_plan(plan_record(t[:1], set(), 800, keep_prev=True), 1, [0])
    # a wanted last step is not kept twice
    _check_plan(plan_record(t, {t[9]}, 800), 10, [9])


def test_stop_steps_of_a_slice():
    """step `s` of an `ns`-step slice is a stop iff `savetimes` is None, its
    time is in `savetimes`, or `s >= ns - 1 - keep_prev`; the expected sets are
    written out by hand"""
    from dolfin_navier_scipy_amd.time_int_utils import stop_steps
    t = (0.5 + 0.01*np.arange(5)).tolist()
    expected = {
        # (ns, keep_prev): the stops for `savetimes` None, empty, and a subset
        # that misses the last two steps: {17.0}, and for ns = 5 t[0], t[2] too
        (1, False): ([0], [0], [0]),
        (1, True): ([0], [0], [0]),
        (2, False): ([0, 1], [1], [1]),
        (2, True): ([0, 1], [0, 1], [0, 1]),
        (5, False): ([0, 1, 2, 3, 4], [4], [0, 2, 4]),
        (5, True): ([0, 1, 2, 3, 4], [3, 4], [0, 2, 3, 4]),
    }
    for (ns, keep_prev), wants in expected.items():
        subset = set(t[:max(ns - 2, 0):2]) | {17.0}
        assert not subset & set(t[:ns][-2:])
        for savetimes, want in zip((None, set(), subset), wants):
            got = stop_steps(t[:ns], savetimes, keep_prev)
            assert got == want, (ns, keep_prev, savetimes)
            assert got[-1] == ns - 1              # the loop goes on from it
            if keep_prev and ns > 1:
                assert got[-2] == ns - 2          # SBDF2's blow-up guard
    assert stop_steps([], None, True) == []


def test_plan_of_an_empty_slice_is_empty():
    from dolfin_navier_scipy_amd.time_int_utils import plan_record
    assert plan_record([], None, snap_bytes=800) == []
    assert plan_record([], {1.0}, snap_bytes=800, keep_prev=True) == []


def test_plan_chunks_under_a_small_record_bytes():
    from dolfin_navier_scipy_amd.time_int_utils import plan_record
    t = (0.01*np.arange(1, 13)).tolist()
    # room for 4 snapshots (and 799 bytes to spare): 12 kept steps, 3 chunks
    chunks = plan_record(t, None, snap_bytes=800, record_bytes=4*800 + 799)
    assert [c['nsteps'] for c in chunks] == [4, 4, 4]
    _check_plan(chunks, 12, list(range(12)))
    # every third time: 4 kept steps + the last, room for 2 per chunk
    want = {t[0], t[3], t[6], t[9]}
    chunks = plan_record(t, want, snap_bytes=800, record_bytes=1600)
    _check_plan(chunks, 12, [0, 3, 6, 9, 11])
    assert [(c['first'], c['nsteps']) for c in chunks] == [(0, 4), (4, 6),
                                                           (10, 2)]
    # one snapshot per chunk
    chunks = plan_record(t, want, snap_bytes=800, record_bytes=800)
    _check_plan(chunks, 12, [0, 3, 6, 9, 11])
    assert len(chunks) == 5


def test_plan_refuses_record_bytes_below_one_snapshot():
    from dolfin_navier_scipy_amd.time_int_utils import plan_record
    with pytest.raises(ValueError) as exc:
        plan_record([0.1, 0.2], None, snap_bytes=800, record_bytes=799)
    assert 'record_bytes' in str(exc.value)


def test_device_record_sizes_a_snapshot_like_a_ring_vector():
    from dolfin_navier_scipy_amd import time_int_utils as tiu
    rec = tiu._DeviceRecord(None, dict(record=True), 100, 27)
    assert rec.snap_bytes == 8*128          # NV + NP padded to 64 entries
    assert rec.record_bytes == tiu.RECORD_BYTES == 1 << 30
    assert rec.outputs is None and rec.result() == (None, None)
    rec = tiu._DeviceRecord(None, dict(outputs=np.ones((2, 100)),
                                       record_bytes=4096), 100, 28)
    assert rec.snap_bytes == 8*128 and rec.record_bytes == 4096
    y, t = rec.result()
    assert y.shape == (0, 2) and t.shape == (0,)


# ---- argument checks of `ImexStepper.set_recorder` ------------------------------

def _bare_stepper(NV=7, NP=3):
    """an `ImexStepper` without a device behind it: the checks below fail
    before the library is called"""
    from dolfin_navier_scipy_amd import saddle
    stp = saddle.ImexStepper.__new__(saddle.ImexStepper)
    stp.sys = types.SimpleNamespace(NV=NV, NP=NP)
    stp.lib = None
    stp._h = None
    return stp


def test_set_recorder_argument_checks():
    stp = _bare_stepper()
    C = sps.csr_matrix(np.ones((2, 7)))
    with pytest.raises(ValueError):                  # nothing to record
        stp.set_recorder(4)
    with pytest.raises(ValueError):                  # no rows
        stp.set_recorder(0, cv_mat=C)
    with pytest.raises(ValueError) as exc:           # columns of cv_mat
        stp.set_recorder(4, cv_mat=sps.csr_matrix(np.ones((2, 8))))
    assert 'NV' in str(exc.value)
    with pytest.raises(ValueError):                  # the transpose
        stp.set_recorder(4, cv_mat=sps.csr_matrix(np.ones((7, 2))))
    with pytest.raises(ValueError):                  # one slot entry per row
        stp.set_recorder(4, snap_slots=[0, 1, 2])
    with pytest.raises(ValueError):                  # below -1
        stp.set_recorder(4, snap_slots=[0, -2, 1, 2])
    with pytest.raises(ValueError):                  # keeps nothing
        stp.set_recorder(4, snap_slots=[-1, -1, -1, -1])
    with pytest.raises(ValueError):
        stp.set_recorder(4, snap_slots='some')
    # nothing was set: the downloads say so
    with pytest.raises(ValueError):
        stp.record_outputs()
    with pytest.raises(ValueError):
        stp.record_snapshots()


def test_solve_nse_has_the_keyword_off_by_default():
    import inspect
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    sig = inspect.signature(snu.solve_nse)
    assert sig.parameters['record_on_device'].default is False
