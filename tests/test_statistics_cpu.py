"""Flow statistics of the explicit loops, host side: the entry points (header,
ctypes table, exports of the cross-compiled library, null handles), the
argument checks `ImexStepper.set_statistics` makes in Python,
`fem.FlowStatistics` against hand-written cases and `fem.component_pairs` on a
small mesh.  No device."""
import inspect
import os
import re
import types
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ('dns_imex_set_stats', 'dns_imex_get_stats',
               'dns_imex_clear_stats')


def test_header_declares_and_capi_binds_the_statistics_entry_points():
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
    bins = np.zeros(4, dtype=np.int32)
    bp = bins.ctypes.data_as(_capi.c_int32_p)
    calls = ((lib.dns_imex_set_stats, (None, 4, bp, 1, 0, None, None, 0)),
             (lib.dns_imex_get_stats, (None, 0, 1, None, None, None, None)),
             (lib.dns_imex_clear_stats, (None,)))
    for fn, args in calls:
        assert fn(*args) == _capi.DNS_ERR_BAD_ARGUMENT
        assert b'null' in lib.dns_last_error()


def test_stats_kernel_is_a_dependency_of_the_build():
    from dolfin_navier_scipy_amd import build
    names = [os.path.basename(p) for p in build.dependencies()]
    assert 'stats.hpp' in names
    text = open(os.path.join(ROOT, 'dolfin_navier_scipy_amd', 'csrc',
                             'imex.hpp')).read()
    assert '#include "stats.hpp"' in text


# ---- argument checks of `ImexStepper.set_statistics` ---------------------------

def _bare_stepper(NV=7, NP=3):
    """an `ImexStepper` without a device behind it: the checks below fail
    before the library is called"""
    from dolfin_navier_scipy_amd import saddle
    stp = saddle.ImexStepper.__new__(saddle.ImexStepper)
    stp.sys = types.SimpleNamespace(NV=NV, NP=NP)
    stp.lib = None
    stp._h = None
    return stp


def test_set_statistics_argument_checks():
    stp = _bare_stepper()
    with pytest.raises(ValueError):                  # no rows
        stp.set_statistics([])
    with pytest.raises(ValueError):                  # one entry per step
        stp.set_statistics([[0, 0], [0, 0]])
    with pytest.raises(ValueError):                  # bins are integers
        stp.set_statistics([0., 1.])
    with pytest.raises(ValueError):                  # below -1
        stp.set_statistics([0, -2, 0])
    with pytest.raises(ValueError):                  # a bin >= nbins
        stp.set_statistics([0, 2, 1], nbins=2)
    with pytest.raises(ValueError) as exc:           # nbins outside 1..256
        stp.set_statistics([0, 1], nbins=257)
    assert '256' in str(exc.value)
    with pytest.raises(ValueError):
        stp.set_statistics([0, 1], nbins=0)
    with pytest.raises(ValueError):                  # pairs: npairs x 2
        stp.set_statistics([0, 0], pairs=[0, 1, 2])
    with pytest.raises(ValueError):
        stp.set_statistics([0, 0], pairs=[[0, 1, 2]])
    with pytest.raises(ValueError) as exc:           # an index >= NV + NP
        stp.set_statistics([0, 0], pairs=[[0, 1], [3, 10]])
    assert 'NV + NP' in str(exc.value)
    with pytest.raises(ValueError):
        stp.set_statistics([0, 0], pairs=[[-1, 1]])
    with pytest.raises(ValueError):                  # integer indices
        stp.set_statistics([0, 0], pairs=[[0.5, 1.]])
    # nothing was set: the download says so
    with pytest.raises(ValueError):
        stp.statistics()


# ---- `fem.FlowStatistics` ---------------------------------------------------------

def test_flow_statistics_against_hand_written_cases():
    from dolfin_navier_scipy_amd.fem import FlowStatistics
    # NV = 2, NP = 1; three bins by the time, bin 2 never hit, t = 9 skipped
    fs = FlowStatistics(pairs=[[0, 1], [1, 2], [2, 2]], nbins=3,
                        bin_of=lambda t: -1 if t == 9 else int(t) % 2)
    fs.add([1., 2.], [3.], 0)           # bin 0
    fs.add([10., 20.], [30.], 1)        # bin 1
    fs.add([3., 6.], [-1.], 2)          # bin 0
    fs.add([100., 100.], [100.], 9)     # skipped
    assert fs.counts.tolist() == [2, 1, 0]
    assert np.array_equal(fs.s1_v, [[4., 8.], [10., 20.], [0., 0.]])
    assert np.array_equal(fs.s1_p, [[2.], [30.], [0.]])
    assert np.array_equal(fs.s2_v, [[10., 40.], [100., 400.], [0., 0.]])
    assert np.array_equal(fs.s2_p, [[10.], [900.], [0.]])
    assert np.array_equal(fs.sx, [[2. + 18., 6. - 6., 9. + 1.],
                                  [200., 600., 900.], [0., 0., 0.]])
    with warnings.catch_warnings():
        warnings.simplefilter('error')             # an empty bin: no warning
        mv, mp = fs.mean()
        vv, vp = fs.variance()
        cov = fs.covariance()
    assert np.array_equal(mv[:2], [[2., 4.], [10., 20.]])
    assert np.array_equal(mp[:2], [[1.], [30.]])
    assert np.isnan(mv[2]).all() and np.isnan(mp[2]).all()
    # bin 0: v0 in {1, 3}: variance 1; v1 in {2, 6}: 4; p in {3, -1}: 4
    assert np.array_equal(vv[:2], [[1., 4.], [0., 0.]])
    assert np.array_equal(vp[:2], [[4.], [0.]])
    assert np.isnan(vv[2]).all() and np.isnan(vp[2]).all()
    # bin 0: cov(v0, v1) = 10 - 8 = 2, cov(v1, p) = 0 - 4 = -4, var p = 4
    assert np.array_equal(cov[:2], [[2., -4., 4.], [0., 0., 0.]])
    assert np.isnan(cov[2]).all()
    # sums formed elsewhere go on top
    fs.add_sums(dict(counts=[0, 0, 1], s1_v=np.ones((3, 2)),
                     s1_p=np.ones((3, 1)), s2_v=np.ones((3, 2)),
                     s2_p=np.ones((3, 1)), sx=np.ones((3, 3))))
    assert fs.counts.tolist() == [2, 1, 1]
    assert np.array_equal(fs.s1_v[0], [5., 9.])
    assert np.array_equal(fs.mean()[0][2], [1., 1.])


def test_flow_statistics_defaults_and_refusals():
    from dolfin_navier_scipy_amd.fem import FlowStatistics
    fs = FlowStatistics(t_start=0.5)
    assert fs.bins([0.25, 0.5, 0.75]).tolist() == [-1, 0, 0]
    assert fs.bins([0.25, 0.5]).dtype == np.int32
    assert FlowStatistics().bins([-3., 7.]).tolist() == [0, 0]
    with pytest.raises(ValueError):                 # nothing added yet
        fs.mean()
    fs.add(np.ones((4, 1)), np.ones((2, 1)), 0.25)
    assert fs.counts.tolist() == [0] and fs.sx.shape == (1, 0)
    assert np.isnan(fs.mean()[0]).all()
    fs.add(2*np.ones((4, 1)), np.ones((2, 1)), 0.5)
    assert fs.counts.tolist() == [1]
    assert np.array_equal(fs.mean()[0], 2*np.ones((1, 4)))
    with pytest.raises(ValueError):                 # a state of another size
        fs.add(np.ones(5), np.ones(2), 1.)
    with pytest.raises(ValueError):
        FlowStatistics(nbins=0)
    with pytest.raises(ValueError):
        FlowStatistics(nbins=257)
    with pytest.raises(ValueError):
        FlowStatistics(pairs=[0, 1, 2])
    with pytest.raises(ValueError):                 # bin_of outside its bins
        FlowStatistics(nbins=2, bin_of=lambda t: 2).bin_of(0.)
    with pytest.raises(ValueError):                 # a pair beyond NV + NP
        FlowStatistics(pairs=[[0, 6]]).add(np.ones(4), np.ones(2), 0.)


def test_component_pairs_on_a_small_mesh_with_a_dirichlet_node():
    from dolfin_navier_scipy_amd.fem import component_pairs
    # four nodes; node 1 is Dirichlet in x only, node 2 in both components
    th = types.SimpleNamespace(vdim=8)
    invinds = np.array([0, 1, 3, 6, 7])     # full dofs 2 (x of node 1), 4, 5 out
    pairs = component_pairs(th, invinds)
    assert pairs.dtype == np.int32
    # node 0: inner 0, 1; node 1: x fixed -> no pair; node 3: inner 3, 4
    assert pairs.tolist() == [[0, 1], [3, 4]]
    assert component_pairs(th, np.arange(8)).tolist() == \
        [[0, 1], [2, 3], [4, 5], [6, 7]]


def test_component_pairs_of_the_toy_problem(toy_prob):
    from dolfin_navier_scipy_amd.fem import component_pairs
    th, inv = toy_prob['th'], np.asarray(toy_prob['invinds'])
    pairs = component_pairs(th, inv)
    assert pairs.shape[1] == 2 and 0 < pairs.shape[0] <= inv.size//2
    # a pair is the two components of ONE node, x first
    assert np.array_equal(inv[pairs[:, 0]] + 1, inv[pairs[:, 1]])
    assert np.all(inv[pairs[:, 0]] % 2 == 0)
    # every free node with both components is there
    free = set(inv.tolist())
    want = sum(1 for n in range(th.vdim//2)
               if 2*n in free and 2*n + 1 in free)
    assert pairs.shape[0] == want


def test_solve_nse_has_the_keyword_off_by_default():
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    sig = inspect.signature(snu.solve_nse)
    assert sig.parameters['statistics'].default is None
