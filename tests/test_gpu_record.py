"""Device-resident trajectory recorder of the explicit loops (`k_record_step`,
`dns_imex_set_recorder`, `resident=dict(record=True)` of `cnab` / `sbdftwo`,
`solve_nse(record_on_device=True)`): against the golden vectors of the
reference's own `cnab` / `sbdftwo`, against the kernel's definition, with
selected save times and chunked snapshot buffers, through a restored batch, at
full size against the CPU oracle, together with observer feedback, through
`solve_nse`, and the refusals.

Tolerances: velocities and pressures 1e-8 relative (`VTOL` / `PTOL` of
`test_gpu_imex.py`); kernels against NumPy / SciPy 1e-13 relative to
the sum of the absolute terms.
"""
import os

import numpy as np
import pytest
import scipy.sparse as sps

import feedback_setup as fs
import scenarios
from oracle import imex_oracle
from oracle import snu_oracle as so
from test_gpu_feedback import ToyLoop, WakeLoop, wake_setup

pytestmark = pytest.mark.gpu

VTOL, PTOL = 1e-8, 1e-8
KTOL = 1e-13


@pytest.fixture(scope='module')
def gtiu():
    from dolfin_navier_scipy_amd import time_int_utils, _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    return time_int_utils


@pytest.fixture(scope='module')
def wake(gtiu):
    return wake_setup()


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max()/np.abs(b).max()


def _nslices(gtiu, trange, ntimeslices=10):
    """non-empty time slices of the loop"""
    return sum(1 for c in gtiu._inittimegrid(trange, ntimeslices)[1] if c)


def _toy_cvop(prob, variant='plain'):
    """the device convection of a scenario; `movingbc`: the static Dirichlet
    dofs first, the controlled ones behind them (`resident['static_dbcvals']`)
    """
    from dolfin_navier_scipy_amd import convection
    dbcinds, dbcvals = prob['dbcinds'], prob['dbcvals']
    statvals = []
    if variant == 'movingbc':
        cnt = np.abs(dbcvals) > 0
        statvals = dbcvals[~cnt].tolist()
        dbcinds = np.concatenate([dbcinds[~cnt], dbcinds[cnt]])
        dbcvals = np.concatenate([dbcvals[~cnt], dbcvals[cnt]])
    cvop = convection.ConvectionP2.from_taylor_hood(
        prob['th'], prob['invinds'], dbcinds, dbcvals)
    return cvop, statvals


def _against(times, vels, prss, gold_t, gold_v, gold_p, what, first_p=1):
    assert np.allclose(times, gold_t, rtol=0, atol=1e-15)
    worst_v = worst_p = 0.
    for k in range(len(times)):
        ev = np.linalg.norm(vels[k] - gold_v[k])/np.linalg.norm(gold_v[k])
        worst_v = max(worst_v, ev)
        assert ev <= VTOL, (what, k, ev)
        if k >= first_p:
            dp = np.linalg.norm(prss[k] - gold_p[k])
            npk = np.linalg.norm(gold_p[k])
            worst_p = max(worst_p, dp/npk if npk > 0 else dp)
            assert dp <= PTOL*npk, (what, k, dp, npk)
    print(what, ': worst v', worst_v, 'p', worst_p)


# ---- 1. against the reference's own recordings --------------------------------

@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
@pytest.mark.parametrize('seed,variant', [(0, 'plain'), (2, 'movingbc')])
def test_recorded_slices_match_reference_golden(gtiu, golden_dir, toy_prob,
                                                scheme, seed, variant):
    """all 13 `(time, v with boundary values, p)` triples of the golden runs,
    the 11 loop steps written down by the device: one `run` per time slice"""
    gold = np.load(os.path.join(
        golden_dir, 'imex_{0}_{1}_s{2}.npz'.format(scheme, variant, seed)))
    kw, rec, _ = scenarios.build(variant=variant, seed=seed, prob=toy_prob)
    if variant == 'plain':
        kw.pop('f_vdp')
    # (`movingbc` keeps the scenario's `f_vdp` for the Heun start: it reads the
    # boundary values of that start out of the full vector it is handed)
    cvop, statvals = _toy_cvop(toy_prob, variant)
    integ = gtiu.cnab if scheme == 'cnab' else gtiu.sbdftwo
    resident = dict(record=True, savevp_times=None)
    if variant == 'movingbc':
        resident.update(bcs_time_only=True, static_dbcvals=statvals)
    try:
        v, p, ff = integ(device_convection=cvop, invinds=toy_prob['invinds'],
                         resident=resident, **kw)
    finally:
        cvop.close()
    assert ff == int(gold['ffflag'])
    assert gtiu.LAST_RUN['record'] == 'device'
    assert gtiu.LAST_RUN['run_calls'] == _nslices(gtiu, kw['trange']) == 11
    times, vels, prss = rec.arrays()
    assert times.size == 13
    _against(times, vels, prss, gold['times'], gold['vels'], gold['prss'],
             '{0} {1}, recorded'.format(scheme, variant))
    # what the loop returns is the last row
    assert np.array_equal(p[:, 0], prss[-1])


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_state_dependent_callbacks_keep_the_host_path(gtiu, golden_dir,
                                                      toy_prob, scheme):
    """`forced` has a `dynamic_rhs` that reads the velocity: `record=True`
    changes nothing, the loop takes one step at a time"""
    gold = np.load(os.path.join(
        golden_dir, 'imex_{0}_forced_s1.npz'.format(scheme)))
    kw, rec, _ = scenarios.build(variant='forced', seed=1, prob=toy_prob)
    kw.pop('f_vdp')
    cvop, _ = _toy_cvop(toy_prob)
    try:
        if scheme == 'sbdf2':
            kw.pop('f_tvdp', None)
            gtiu.sbdftwo(device_convection=cvop, invinds=toy_prob['invinds'],
                         resident=dict(record=True, savevp_times=None), **kw)
        else:
            gtiu.cnab(device_convection=cvop, invinds=toy_prob['invinds'],
                      resident=dict(record=True, savevp_times=None), **kw)
    finally:
        cvop.close()
    assert gtiu.LAST_RUN['record'] == 'host'
    assert gtiu.LAST_RUN['run_calls'] == 0
    assert gtiu.LAST_RUN['record_y'] is None
    times, vels, prss = rec.arrays()
    _against(times, vels, prss, gold['times'], gold['vels'], gold['prss'],
             '{0} forced, host'.format(scheme))


# ---- 2. the kernel against its definition -------------------------------------

def _test_matrix(NV, seed=3):
    """a `C` with a one-entry row, an empty row, a full row and sparse rows"""
    rng = np.random.default_rng(seed)
    rows = [np.zeros(NV) for _ in range(6)]
    rows[0][NV//3] = 1.7                                   # one entry
    rows[2] = rng.standard_normal(NV)                      # full (row 1: empty)
    for r in (3, 4, 5):
        idx = rng.choice(NV, size=70 + 30*r, replace=False)
        rows[r][idx] = rng.standard_normal(idx.size)
    return sps.csr_matrix(np.array(rows))


@pytest.mark.parametrize('how', ['step', 'run'])
def test_record_kernel_against_its_definition(gtiu, toy_prob, how):
    """k steps by `dns_imex_step` / one `dns_imex_run`: the last row is
    `get_state()` bit for bit, `y` row s is `C @ v` of the recorded snapshot
    to 1e-13 of `|C| |v|`, a slot table with `-1` entries keeps the same
    bits, and a second identical run gives identical bits"""
    nst = 24

    def trajectory(slots, C):
        lp = ToyLoop(toy_prob)
        try:
            stp = lp.stp
            stp.set_recorder(nst, cv_mat=C, snap_slots=slots)
            assert stp.table_position() == (0, nst)
            states = []
            if how == 'step':
                for k in range(nst):
                    stp.step(lp.cf, opts=lp.opts)
                    if k in (0, 7, nst - 1):
                        states.append((k, stp.get_state()))
            else:
                stp.run(nst, lp.cf, lp.opts)
                states.append((nst - 1, stp.get_state()))
            assert stp.table_position() == (nst, 0)
            vs, ps = stp.record_snapshots()
            y = stp.record_outputs()
            return vs, ps, y, states
        finally:
            lp.close()

    NV = toy_prob['smc']['J'].shape[1]
    C = _test_matrix(NV)
    vs, ps, y, states = trajectory('all', C)
    assert vs.shape == (nst, NV) and y.shape == (nst, 6)
    for k, (v, p) in states:
        assert np.array_equal(vs[k], v[:, 0]), k
        assert np.array_equal(ps[k], p[:, 0]), k
    # the trajectory moves: rows differ from one another
    assert np.abs(vs[-1] - vs[0]).max() > 1e-6*np.abs(vs[0]).max()
    absC = abs(C)
    worst = 0.
    for s in range(nst):
        bound = KTOL*(absC @ np.abs(vs[s]))
        err = np.abs(y[s] - C @ vs[s])
        assert np.all(err <= bound), (s, err, bound)
        worst = max(worst, (err[bound > 0]/bound[bound > 0]).max()*KTOL)
    print(how, ': y against C v, worst error relative to |C||v|', worst)
    assert np.all(y[:, 1] == 0.)                           # the empty row
    assert np.array_equal(y[:, 0], 1.7*vs[:, NV//3])       # the one entry
    # every third step and the last one kept, in slots counted from 0
    slots = -np.ones(nst, dtype=np.int32)
    keep = sorted(set(range(2, nst, 3)) | {nst - 1})
    slots[keep] = np.arange(len(keep))
    vk, pk, yk, _ = trajectory(slots, C)
    assert vk.shape == (len(keep), NV)
    assert np.array_equal(vk, vs[keep]) and np.array_equal(pk, ps[keep])
    assert np.array_equal(yk, y)
    # the same run again
    v2, p2, y2, _ = trajectory('all', C)
    assert np.array_equal(v2, vs) and np.array_equal(p2, ps)
    assert np.array_equal(y2, y)
    # outputs only / snapshots only
    lp = ToyLoop(toy_prob)

    def advance(n):
        if how == 'run':
            lp.stp.run(n, lp.cf, lp.opts)
        else:
            for _ in range(n):
                lp.stp.step(lp.cf, opts=lp.opts)
    try:
        lp.stp.set_recorder(nst, cv_mat=C)
        advance(nst)
        assert np.array_equal(lp.stp.record_outputs(), y)
        lp.stp.set_recorder(4, snap_slots=[-1, 0, -1, 1])
        advance(4)
        v4, p4 = lp.stp.record_snapshots()
        vl, pl = lp.stp.get_state()
        assert np.array_equal(v4[1], vl[:, 0])
        assert np.array_equal(p4[1], pl[:, 0])
    finally:
        lp.close()


def test_recorder_off_leaves_the_step_as_it_was(gtiu, toy_prob):
    """a stepper that had a recorder and cleared it steps like one that never
    had one: the same bits, the same number of steps built"""
    la, lb = ToyLoop(toy_prob), ToyLoop(toy_prob)
    try:
        NV = toy_prob['smc']['J'].shape[1]
        la.stp.set_recorder(8, cv_mat=_test_matrix(NV), snap_slots='all')
        la.stp.clear_recorder()
        assert la.stp.table_position() == (0, -1)
        la.stp.run(20, la.cf, la.opts)
        lb.stp.run(20, lb.cf, lb.opts)
        assert np.array_equal(la.stp.get_state()[0], lb.stp.get_state()[0])
        assert np.array_equal(la.stp.get_state()[1], lb.stp.get_state()[1])
        assert la.stp.step_counters() == lb.stp.step_counters()
        assert la.stp.last_run == lb.stp.last_run
    finally:
        la.close()
        lb.close()


# ---- 3. selection and chunks ----------------------------------------------------

@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_selected_times_and_chunked_slices(gtiu, toy_prob, scheme):
    """every third time wanted, two slices of 23 steps (and one of one step),
    room for three snapshots: three chunks per slice.  The same `savevp`
    calls as the host path of the same tree, the same values, and both
    against the oracle"""
    Nts = 48
    integ = gtiu.cnab if scheme == 'cnab' else gtiu.sbdftwo
    orac = imex_oracle.cnab if scheme == 'cnab' else imex_oracle.sbdftwo
    kwo, reco, _ = scenarios.build(variant='plain', seed=4, Nts=Nts, tE=0.24,
                                   prob=toy_prob)
    orac(**kwo)
    to, vo, po = reco.arrays()
    want = kwo['trange'][::3].tolist()
    NP, NV = toy_prob['smc']['J'].shape
    snap = 8*(-(-(NV + NP)//64)*64)
    got = {}
    for mode in ('host', 'device'):
        kw, rec, _ = scenarios.build(variant='plain', seed=4, Nts=Nts,
                                     tE=0.24, prob=toy_prob)
        kw.pop('f_vdp')
        cvop, _ = _toy_cvop(toy_prob)
        resident = dict(savevp_times=want)
        if mode == 'device':
            resident.update(record=True, record_bytes=3*snap + 8)
        try:
            v, p, ff = integ(device_convection=cvop, ntimeslices=2,
                             invinds=toy_prob['invinds'], resident=resident,
                             **kw)
        finally:
            cvop.close()
        assert ff == 0
        assert gtiu.LAST_RUN['record'] == mode
        got[mode] = rec.arrays() + (v, p, gtiu.LAST_RUN['run_calls'])
    th, vh, ph, vhe, phe, calls_h = got['host']
    td, vd, pd, vde, pde, calls_d = got['device']
    print(scheme, 'run calls: host', calls_h, 'device', calls_d)
    assert calls_d == 7                  # 3 + 3 chunks and the one-step slice
    # the same calls, in the same order: t0, t1 (Heun start), then the wanted
    expect = [kwo['trange'][0], kwo['trange'][1]] + \
        [t for t in want if t > kwo['trange'][1]]
    assert th.tolist() == expect and td.tolist() == expect
    _against(td, vd, pd, th, vh, ph, scheme + ' chunks, device vs host')
    idx = [int(np.argmin(np.abs(to - t))) for t in expect]
    assert np.allclose(to[idx], expect, rtol=0, atol=1e-15)
    _against(td, vd, pd, to[idx], vo[idx], po[idx],
             scheme + ' chunks, device vs oracle')
    _against(th, vh, ph, to[idx], vo[idx], po[idx],
             scheme + ' chunks, host vs oracle')
    assert np.linalg.norm(vde - vhe) <= VTOL*np.linalg.norm(vhe)
    assert np.linalg.norm(pde - phe) <= PTOL*np.linalg.norm(phe)


# ---- 4. replayed batch -----------------------------------------------------------

def test_a_restored_batch_overwrites_its_own_rows(gtiu, wake):
    """the recipe of `test_batches_and_a_restored_batch_reproduce_the_single_
    steps` (open loop: the tabulated forcing jumps at step 128, the batch
    around it is restored and repeated) with the recorder on: every recorded
    row against the same 256 steps taken one at a time and read with
    `get_state`.  The record buffers are not part of the checkpoint: the
    repeated batch writes its rows again."""
    M, C = wake['M'], wake['C']
    nst = 256
    lp = WakeLoop(wake, nst, feedback=False)
    try:
        lp.stp.set_recorder(nst, cv_mat=C, snap_slots='all')
        lp.run(nst)
        vs, ps = lp.stp.record_snapshots()
        ys = lp.stp.record_outputs()
        vl, pl = lp.stp.get_state()
        record = dict(lp.record)
    finally:
        lp.close()
    print('recorded run:', record)
    assert record['unconverged'] == 0
    assert record['replayed'] > 0, record
    assert np.array_equal(vs[-1], vl[:, 0]) and np.array_equal(ps[-1], pl[:, 0])
    ls = WakeLoop(wake, nst, feedback=False)
    worst_v = worst_p = worst_y = 0.
    yscale = np.abs(ys).max()
    try:
        for s in range(nst):
            ls.run(1)
            v, p = ls.stp.get_state()
            ev = fs.mnorm(M, vs[s].reshape((-1, 1)) - v)/fs.mnorm(M, v)
            ep = np.linalg.norm(ps[s] - p[:, 0])/np.linalg.norm(p)
            ey = np.abs(ys[s] - (C @ v)[:, 0]).max()/yscale
            worst_v, worst_p = max(worst_v, ev), max(worst_p, ep)
            worst_y = max(worst_y, ey)
            assert ev <= 1e-8 and ep <= 1e-8, (s, ev, ep)
            assert ey <= 1e-8, (s, ey)
    finally:
        ls.close()
    print('recorded rows vs single steps: v', worst_v, 'p', worst_p, 'y',
          worst_y)


# ---- 5. full size against the oracle --------------------------------------------

def test_full_size_record_against_the_oracle(gtiu, wake):
    """wake N=2, Re=100, dt=1/512, 256 steps from the Stokes state: every
    recorded velocity and pressure and every `y = C v` against
    `imex_oracle.cnab`; one `run` per time slice"""
    from dolfin_navier_scipy_amd import convection
    femp, M, C = wake['femp'], wake['M'], wake['C']
    inv = femp['invinds']
    reco = scenarios.Recorder()
    vo, po, ffo = imex_oracle.cnab(**wake['make_kw'](reco))
    to, vso, pso = reco.arrays()
    assert ffo == 0 and to.size == 257
    cvop = convection.ConvectionP2.from_taylor_hood(
        femp['V'], inv, femp['dbcinds'], femp['dbcvals'])
    rec = scenarios.Recorder()
    kw = wake['make_kw'](rec)
    kw.pop('f_vdp')
    try:
        vg, pg, ff = gtiu.cnab(device_convection=cvop, invinds=inv,
                               resident=dict(record=True, outputs=C,
                                             savevp_times=None), **kw)
    finally:
        cvop.close()
    assert ff == 0
    assert gtiu.LAST_RUN['record'] == 'device'
    assert gtiu.LAST_RUN['run_calls'] == _nslices(gtiu, kw['trange']) == 11
    tg, vsg, psg = rec.arrays()
    assert tg.size == 257 and np.allclose(tg, to, rtol=0, atol=1e-15)
    worst_v = worst_p = 0.
    for k in range(257):
        ev = fs.mnorm(M, (vsg[k] - vso[k])[inv].reshape((-1, 1))) / \
            fs.mnorm(M, vso[k][inv].reshape((-1, 1)))
        worst_v = max(worst_v, ev)
        assert ev <= 1e-8, (k, ev)
        if k > 0:
            ep = np.linalg.norm(psg[k] - pso[k])/np.linalg.norm(pso[k])
            worst_p = max(worst_p, ep)
            assert ep <= 1e-8, (k, ep)
    ry, rt = gtiu.LAST_RUN['record_y'], gtiu.LAST_RUN['record_t']
    assert ry.shape == (255, C.shape[0])
    assert np.allclose(rt, to[2:], rtol=0, atol=1e-15)
    yo = np.array([C @ vso[k][inv] for k in range(2, 257)])
    ey = np.abs(ry - yo).max()/np.abs(yo).max()
    print('full size, recorded vs oracle: v', worst_v, 'p', worst_p, 'y', ey)
    assert ey <= 1e-8, ey


# ---- 6. with feedback --------------------------------------------------------------

@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_record_with_resident_feedback_matches_golden(gtiu, golden_dir,
                                                      toy_prob, scheme):
    """the golden closed loop (49 points) with the recorder on -- a step then
    has eight nodes: the assertions of `test_resident_feedback_matches_
    reference_golden`, and the recorder's `y` rows against the observer's own
    log, which is one row ahead (`feedback_y[s]` is what step s saw)"""
    gold = np.load(os.path.join(
        golden_dir, 'imex_{0}_feedback_s5.npz'.format(scheme)))
    fb = gtiu.LinearFeedback(fs.csr_unpack(gold, 'C'),
                             fs.csr_unpack(gold, 'B'), gold['ha'], gold['hb'],
                             gold['hc'], gold['inihx'],
                             drift=fs.drift_of(gold['dvec']))
    kw, rec, _ = scenarios.build(variant='plain', seed=5, Nts=48, tE=0.24,
                                 prob=toy_prob)
    kw.pop('f_vdp')
    cvop, _ = _toy_cvop(toy_prob)
    mem = {}
    integ = gtiu.cnab if scheme == 'cnab' else gtiu.sbdftwo
    try:
        v, p, ff = integ(dynamic_rhs=fb, dynamic_rhs_memory=mem,
                         device_convection=cvop, invinds=toy_prob['invinds'],
                         resident=dict(savevp_times=None, record=True,
                                       outputs=fb.cv_mat), **kw)
    finally:
        cvop.close()
    assert ff == 0
    assert gtiu.LAST_RUN['feedback'] == 'resident'
    assert gtiu.LAST_RUN['record'] == 'device'
    assert gtiu.LAST_RUN['run_calls'] == _nslices(gtiu, kw['trange'])
    assert fb.calls == dict(init=1, heunpred=1, heuncorr=1, abtwo=0), fb.calls
    times, vels, prss = rec.arrays()
    assert times.size == gold['times'].size == 49
    _against(times, vels, prss, gold['times'], gold['vels'], gold['prss'],
             scheme + ' golden feedback, recorded', first_p=0)
    ab = gold['cb_mode'] == 3
    ylog, ulog = gtiu.LAST_RUN['feedback_y'], gtiu.LAST_RUN['feedback_u']
    assert ylog.shape == (47, 3) and ulog.shape == (47, 2)
    assert _rel(ylog, gold['cb_y'][ab]) <= 1e-8
    assert _rel(ulog, gold['cb_u'][ab]) <= 1e-8
    assert abs(mem['lastt'] - float(gold['mem_lastt'])) <= 1e-14
    assert abs(mem['lastdt'] - float(gold['mem_lastdt'])) <= 1e-14
    assert _rel(mem['lasthx'], gold['mem_lasthx']) <= 1e-8
    assert _rel(mem['lastrhs'], gold['mem_lastrhs']) <= 1e-8
    ry = gtiu.LAST_RUN['record_y']
    assert ry.shape == (47, 3)
    shift = _rel(ry[:-1], ylog[1:])
    print(scheme, 'record_y[s-1] vs feedback_y[s]:', shift)
    assert shift <= 1e-13
    assert _rel(ry[-1], fb.cv_mat @ vels[-1][toy_prob['invinds']]) <= 1e-13


# ---- 7. solve_nse --------------------------------------------------------------------

def _static_kwargs(prob, kw):
    return dict(A=prob['smc']['A'], M=prob['smc']['M'], J=prob['smc']['J'],
                fv=prob['rhsd']['fv'], fp=prob['rhsd']['fp'],
                iniv=kw['appndbcs'](kw['inivel'], []), inip=kw['inip'],
                trange=kw['trange'], V=prob['th'], invinds=prob['invinds'],
                dbcinds=prob['dbcinds'], dbcvals=prob['dbcvals'])


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_solve_nse_y_list_from_the_device(gtiu, toy_prob, scheme):
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    kw, _, _ = scenarios.build(variant='plain', seed=2, Nts=24, tE=0.12,
                               prob=toy_prob)
    skw = _static_kwargs(toy_prob, kw)
    inv = toy_prob['invinds']
    C, _ = fs.sensors_actuators(toy_prob['th'], inv, toy_prob['smc']['M'])
    reco = scenarios.Recorder()
    so.solve_nse(time_int_scheme=scheme, savevp=reco, **skw)
    to, vso, _ = reco.arrays()
    try:
        yh = snu.solve_nse(time_int_scheme=scheme, return_y_list=True,
                           cv_mat=C, **skw)
        assert gtiu.LAST_RUN['record'] == 'host'
        calls_h = gtiu.LAST_RUN['run_calls']
        yd = snu.solve_nse(time_int_scheme=scheme, return_y_list=True,
                           cv_mat=C, record_on_device=True, **skw)
        assert gtiu.LAST_RUN['record'] == 'device'
        calls_d = gtiu.LAST_RUN['run_calls']
        # selected data points
        dtr = kw['trange'][[0, 5, 6, 24]].tolist()
        ysel = snu.solve_nse(time_int_scheme=scheme, return_y_list=True,
                             cv_mat=C, record_on_device=True,
                             datatrange=list(dtr), **skw)
    finally:
        snu.clear_cache()
    print(scheme, 'solve_nse run calls: host', calls_h, 'device', calls_d)
    assert calls_d == _nslices(gtiu, kw['trange']) < calls_h
    assert len(yh) == len(yd) == 25
    scale = max(np.abs(C @ vso[k][inv]).max() for k in range(25))
    for k in range(25):
        assert yd[k].shape == yh[k].shape == (C.shape[0], 1)
        assert np.abs(yd[k] - yh[k]).max() <= VTOL*scale, k
        assert np.abs(yd[k][:, 0] - C @ vso[k][inv]).max() <= VTOL*scale, k
    assert len(ysel) == 4
    for y, k in zip(ysel, (0, 5, 6, 24)):
        assert np.abs(y - yd[k]).max() <= VTOL*scale, k


def test_solve_nse_recorded_velocities_seed_the_sweeps(gtiu, toy_prob):
    """the explicit run that seeds the Newton / Picard sweeps hands them the
    same linearisation points whether the host or the device collected them"""
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    kw, _, _ = scenarios.build(variant='plain', seed=0, Nts=6, tE=0.03,
                               prob=toy_prob)
    skw = _static_kwargs(toy_prob, kw)
    inv = toy_prob['invinds']
    try:
        lin = {}
        for dev in (False, True):
            lin[dev] = snu.solve_nse(return_dictofvelstrs=True,
                                     record_on_device=dev, **skw)
            assert gtiu.LAST_RUN['record'] == ('device' if dev else 'host')
        swp = {}
        for dev in (False, True):
            swp[dev] = snu.solve_nse(
                treat_nonl_explicit=False, vel_pcrd_stps=1, vel_nwtn_stps=1,
                return_dictofvelstrs=True, return_dictofpstrs=True,
                record_on_device=dev, **skw)
    finally:
        snu.clear_cache()
    assert sorted(lin[True].keys()) == sorted(lin[False].keys()) \
        == sorted(kw['trange'].tolist())
    for t in kw['trange']:
        a, b = lin[True][t], lin[False][t]
        assert a.shape == b.shape and not np.isnan(a[inv]).any()
        assert np.linalg.norm(a[inv] - b[inv]) <= VTOL*np.linalg.norm(b[inv])
        assert np.array_equal(a[toy_prob['dbcinds']], b[toy_prob['dbcinds']])
    (vd, pd), (vh, ph) = swp[True], swp[False]
    for t in kw['trange'][1:]:
        assert np.linalg.norm(vd[t][inv] - vh[t][inv]) <= \
            VTOL*np.linalg.norm(vh[t][inv]), t
        assert np.linalg.norm(pd[t] - ph[t]) <= PTOL*np.linalg.norm(ph[t]), t


# ---- 8. refusals ----------------------------------------------------------------------

def test_set_recorder_refusals_leave_the_stepper_as_it_was(gtiu, toy_prob):
    from dolfin_navier_scipy_amd import _capi
    import ctypes as ct
    lp, lo = ToyLoop(toy_prob), ToyLoop(toy_prob)
    try:
        stp, lib = lp.stp, lp.stp.lib
        NV = toy_prob['smc']['J'].shape[1]
        C = _test_matrix(NV)
        stp.set_recorder(6, cv_mat=C, snap_slots='all')
        stp.run(2, lp.cf, lp.opts)
        # refused calls, straight at the C-ABI (Python would catch some first)
        cview = _capi.CsrView(C)
        wide = _capi.CsrView(sps.csr_matrix(np.ones((2, NV + 1))))
        slots = np.arange(6, dtype=np.int32)
        sp = slots.ctypes.data_as(_capi.c_int32_p)
        refused = (
            ('nrows', (cview.byref(), 0, None, 0)),
            ('snap_slot', (cview.byref(), 6, sp, 5)),         # entry 5 >= 5
            ('NV', (wide.byref(), 6, None, 0)),
            ('neither', (None, 6, None, 0)),
            ('nslots', (None, 6, sp, 0)),
        )
        for word, args in refused:
            rc = lib.dns_imex_set_recorder(stp._h, *args)
            assert rc == _capi.DNS_ERR_BAD_ARGUMENT, word
            assert word.encode() in lib.dns_last_error(), \
                (word, lib.dns_last_error())
        with pytest.raises(_capi.DnsError):                   # rows out of range
            stp.record_outputs(4, 3)
        with pytest.raises(_capi.DnsError):
            stp.record_snapshots(5, 2)
        # ... the recorder that was there still records, the counter went on
        assert stp.table_position() == (2, 4)
        stp.run(4, lp.cf, lp.opts)
        vs, ps = stp.record_snapshots()
        v, p = stp.get_state()
        assert np.array_equal(vs[5], v[:, 0]) and np.array_equal(ps[5], p[:, 0])
        lo.stp.run(6, lo.cf, lo.opts)
        assert np.array_equal(v, lo.stp.get_state()[0])
        # stepping past the rows
        with pytest.raises(_capi.DnsError) as exc:
            stp.run(1, lp.cf, lp.opts)
        assert exc.value.status == _capi.DNS_ERR_NOT_READY
        with pytest.raises(_capi.DnsError) as exc:
            stp.step(lp.cf, opts=lp.opts)
        assert exc.value.status == _capi.DNS_ERR_NOT_READY
        assert np.array_equal(stp.get_state()[0], v)
        # no recorder: nothing to download, and the stepper steps on
        stp.clear_recorder()
        y = np.empty(6)
        assert lib.dns_imex_get_record_outputs(
            stp._h, 0, 1, y.ctypes.data_as(ct.POINTER(ct.c_double))) \
            == _capi.DNS_ERR_NOT_READY
        stp.run(3, lp.cf, lp.opts)
        lo.stp.run(3, lo.cf, lo.opts)
        assert np.array_equal(stp.get_state()[0], lo.stp.get_state()[0])
    finally:
        lp.close()
        lo.close()


def test_set_recorder_on_a_row_partitioned_stepper_is_refused(gtiu, toy_prob):
    from dolfin_navier_scipy_amd import saddle, _capi, comm as dcomm
    M, A, J = (toy_prob['smc'][k] for k in 'MAJ')
    dt = 5e-3
    cm = dcomm.Comm.rccl(0, 1, 0, dcomm.rccl_unique_id())
    system = saddle.SaddleSystem((M + .5*dt*A).tocsr(), J)
    stp = None
    try:
        system.set_comm(cm)
        system.setup_precond(cheb_degree=6, schur='dense', fhat='explicit')
        stp = saddle.ImexStepper(system, (M - .5*dt*A).tocsr())
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_recorder(4, snap_slots='all')
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        assert 'partitioned' in str(exc.value)
    finally:
        if stp is not None:
            stp.close()
        system.set_comm(None)
        system.close()
        cm.close()
