"""Device-resident flow statistics of the explicit loops (`k_stats_step`,
`dns_imex_set_stats`, `resident=dict(statistics=fs)` of `cnab` / `sbdftwo`,
`solve_nse(statistics=)`): the kernel against its definition over the rows
the recorder wrote down in the same run, however the steps are split into
calls; re-arming; off is off; through a restored batch; through the
integrators against the golden vectors of the reference's own `cnab` /
`sbdftwo`; and the refusals.

Tolerances.  `S1` is plain additions in step order: bit-equal to the
sequential NumPy sum of the recorded rows.  `S2` and `SX` are sums of `n_b`
products by `fma`: recursive summation of `n` terms errs by at most
`(n + 1) u sum |terms|`, `u = 2^-53`; asserted is `n_b 2^-52 sum |terms|` per
entry, which leaves a factor of about 2 (the reference sum is formed in
extended precision).  A row counted twice is an error of the size of one
term.  Means through the integrators: 1e-8 of the maximum of the mean (`VTOL`
/ `PTOL` of `test_gpu_imex.py`).
"""
import os

import numpy as np
import pytest

import scenarios
from test_gpu_feedback import ToyLoop, WakeLoop, wake_setup

pytestmark = pytest.mark.gpu

VTOL, PTOL = 1e-8, 1e-8
NST = 24


@pytest.fixture(scope='module')
def gtiu():
    from dolfin_navier_scipy_amd import time_int_utils, _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    return time_int_utils


@pytest.fixture(scope='module')
def wake(gtiu):
    return wake_setup()


def _toy_bins(nst=NST):
    """three bins: bin 2 stays empty, every fifth step is skipped"""
    return np.array([-1 if s % 5 == 3 else s % 2 for s in range(nst)],
                    dtype=np.int32)


def _toy_pairs(NV, NP, seed=5):
    """an odd number of pairs, more than one workgroup's: `(i, i)`, a
    velocity-pressure pair, one that hits index `NV + NP - 1`"""
    n = NV + NP
    rng = np.random.default_rng(seed)
    pairs = [(3, 3), (5, NV + 2), (n - 1, 7), (NV - 1, NV), (n - 1, n - 1)]
    pairs += [tuple(rng.integers(0, n, size=2)) for _ in range(296)]
    pairs = np.array(pairs, dtype=np.int32)
    assert pairs.shape[0] % 2 == 1 and pairs.shape[0] > 256
    return pairs


def _expected(rows, bins, nbins, pairs):
    """the definition over the recorded rows `x_r`: counts, `S1` by sequential
    float64 additions; `S2`, `SX` in extended precision with the sums of the
    absolute terms"""
    n = rows.shape[1]
    cnt = np.zeros(nbins, dtype=np.int64)
    s1 = np.zeros((nbins, n))
    ld = np.longdouble
    s2, a2 = np.zeros((nbins, n), dtype=ld), np.zeros((nbins, n), dtype=ld)
    sx = np.zeros((nbins, pairs.shape[0]), dtype=ld)
    ax = np.zeros((nbins, pairs.shape[0]), dtype=ld)
    for r, b in enumerate(bins):
        if b < 0:
            continue
        x = rows[r]
        cnt[b] += 1
        s1[b] += x
        xl = x.astype(ld)
        s2[b] += xl*xl
        a2[b] += xl*xl
        pr = xl[pairs[:, 0]]*xl[pairs[:, 1]]
        sx[b] += pr
        ax[b] += np.abs(pr)
    return dict(counts=cnt, s1=s1, s2=s2, a2=a2, sx=sx, ax=ax)


def _check(got, exp, NV, what):
    """counts exact, `S1` bit-equal, `S2` / `SX` within the bound; returns
    the worst ratio error / bound"""
    assert got['counts'].tolist() == exp['counts'].tolist(), what
    s1 = np.hstack([got['s1_v'], got['s1_p']])
    s2 = np.hstack([got['s2_v'], got['s2_p']])
    assert np.array_equal(s1, exp['s1']), \
        (what, np.abs(s1 - exp['s1']).max())
    worst = 0.
    for b, nb in enumerate(exp['counts']):
        for have, ref, mag in ((s2[b], exp['s2'][b], exp['a2'][b]),
                               (got['sx'][b], exp['sx'][b], exp['ax'][b])):
            err = np.abs(have.astype(np.longdouble) - ref)
            bound = nb*2.**-52*mag
            assert np.all(err <= bound), (what, b, float(err.max()))
            if np.any(bound > 0):
                worst = max(worst, float((err[bound > 0]/bound[bound > 0])
                                         .max()))
    print(what, ': S2 / SX worst error / bound', worst)
    return worst


def _advance(lp, how, n):
    if how == 'step':
        for _ in range(n):
            lp.stp.step(lp.cf, opts=lp.opts)
    elif how == 'run':
        lp.stp.run(n, lp.cf, lp.opts)
    else:
        assert how == 'split' and n == NST
        lp.stp.run(7, lp.cf, lp.opts)
        lp.stp.run(17, lp.cf, lp.opts)


def _rows(stp):
    vs, ps = stp.record_snapshots()
    return np.hstack([vs, ps])


# ---- 1. the kernel against its definition -------------------------------------

@pytest.mark.parametrize('how', ['step', 'run', 'split'])
def test_stats_kernel_against_its_definition(gtiu, toy_prob, how):
    """24 steps by `dns_imex_step` (every row is launched for twice: by the
    step's closing node and by the next step's front node), one `dns_imex_run`,
    and `run(7)` then `run(17)` (the row behind the first call twice), with
    the recorder on in the same run"""
    NP, NV = toy_prob['smc']['J'].shape
    bins, pairs = _toy_bins(), _toy_pairs(NV, NP)

    def once():
        lp = ToyLoop(toy_prob)
        try:
            lp.stp.set_recorder(NST, snap_slots='all')
            lp.stp.set_statistics(bins, nbins=3, pairs=pairs)
            assert lp.stp.table_position() == (0, NST)
            _advance(lp, how, NST)
            assert lp.stp.table_position() == (NST, 0)
            return _rows(lp.stp), lp.stp.statistics()
        finally:
            lp.close()

    rows, got = once()
    assert rows.shape == (NST, NV + NP)
    # the trajectory moves: one term more or less is far outside the bound
    assert np.abs(rows[-1] - rows[0]).max() > 1e-6*np.abs(rows[0]).max()
    exp = _expected(rows, bins, 3, pairs)
    assert exp['counts'].tolist() == [10, 9, 0]
    worst = _check(got, exp, NV, how)
    assert worst <= 1.
    for key in ('s1_v', 's1_p', 's2_v', 's2_p', 'sx'):      # the empty bin
        assert np.all(got[key][2] == 0.), key
    assert got['s1_v'].shape == (3, NV) and got['s2_p'].shape == (3, NP)
    assert got['sx'].shape == (3, pairs.shape[0])
    # the same run again: the same bits
    rows2, got2 = once()
    assert np.array_equal(rows2, rows)
    for key in got:
        assert np.array_equal(got2[key], got[key]), key


# ---- 2. re-arming -----------------------------------------------------------------

@pytest.mark.parametrize('reset', [False, True])
def test_rearmed_statistics_go_on_summing_unless_reset(gtiu, toy_prob, reset):
    """bins for 10 rows and `run(10)`, then bins for 14 rows and `run(14)`:
    the sums over all 24 recorded rows (`reset=False`; `S1` as ONE sequential
    sum) or over the last 14 (`reset=True`).  The recorder is set again in
    between -- the counter is rewound once more -- and disturbs nothing"""
    NP, NV = toy_prob['smc']['J'].shape
    bins, pairs = _toy_bins(), _toy_pairs(NV, NP)
    lp = ToyLoop(toy_prob)
    try:
        stp = lp.stp
        stp.set_recorder(10, snap_slots='all')
        stp.set_statistics(bins[:10], nbins=3, pairs=pairs)
        stp.run(10, lp.cf, lp.opts)
        rows_a = _rows(stp)
        first = stp.statistics()
        stp.set_statistics(bins[10:], nbins=3, pairs=pairs, reset=reset)
        stp.set_recorder(14, snap_slots='all')
        assert stp.table_position() == (0, 14)
        stp.run(14, lp.cf, lp.opts)
        rows_b = _rows(stp)
        got = stp.statistics()
    finally:
        lp.close()
    _check(first, _expected(rows_a, bins[:10], 3, pairs), NV, 'first 10')
    if reset:
        exp = _expected(rows_b, bins[10:], 3, pairs)
    else:
        exp = _expected(np.vstack([rows_a, rows_b]), bins, 3, pairs)
    assert _check(got, exp, NV, 'reset={0}'.format(reset)) <= 1.


# ---- 3. off is off ------------------------------------------------------------------

def test_statistics_off_leave_the_step_as_it_was(gtiu, toy_prob):
    """a stepper that had statistics and cleared them steps like one that
    never had any: the same bits, the same number of steps built"""
    NP, NV = toy_prob['smc']['J'].shape
    la, lb = ToyLoop(toy_prob), ToyLoop(toy_prob)
    try:
        la.stp.set_statistics(_toy_bins(8), nbins=3, pairs=_toy_pairs(NV, NP))
        la.stp.clear_statistics()
        assert la.stp.table_position() == (0, -1)
        with pytest.raises(ValueError):
            la.stp.statistics()
        la.stp.run(20, la.cf, la.opts)
        lb.stp.run(20, lb.cf, lb.opts)
        assert np.array_equal(la.stp.get_state()[0], lb.stp.get_state()[0])
        assert np.array_equal(la.stp.get_state()[1], lb.stp.get_state()[1])
        assert la.stp.step_counters() == lb.stp.step_counters()
        assert la.stp.last_run == lb.stp.last_run
    finally:
        la.close()
        lb.close()


# ---- 4. restored batch ---------------------------------------------------------------

def test_a_restored_batch_adds_its_rows_once(gtiu, wake):
    """the recipe of `test_a_restored_batch_overwrites_its_own_rows` (the
    tabulated forcing jumps at step 128, the batch around it is restored and
    repeated) with statistics on: the accumulators and the marks come back
    with the checkpoint, so the sums are those of the recorder's 256 FINAL
    rows -- a batch counted twice would be off by 32 terms"""
    from dolfin_navier_scipy_amd.fem import component_pairs
    femp = wake['femp']
    NP, NV = wake['J'].shape
    nst = 256
    pairs = component_pairs(femp['V'], femp['invinds'])
    assert pairs.shape[0] > 1000
    bins = (np.arange(nst) % 2).astype(np.int32)
    bins[100:140:7] = -1
    lp = WakeLoop(wake, nst, feedback=False)
    try:
        lp.stp.set_recorder(nst, snap_slots='all')
        lp.stp.set_statistics(bins, nbins=2, pairs=pairs)
        lp.run(nst)
        rows = _rows(lp.stp)
        got = lp.stp.statistics()
        record = dict(lp.record)
    finally:
        lp.close()
    print('run with statistics:', record)
    assert record['unconverged'] == 0
    assert record['replayed'] > 0, record
    exp = _expected(rows, bins, 2, pairs)
    assert exp['counts'].sum() == nst - 6
    assert _check(got, exp, NV, 'restored batch') <= 1.


# ---- 5. through the integrators ---------------------------------------------------------

def _toy_cvop(prob):
    from dolfin_navier_scipy_amd import convection
    return convection.ConvectionP2.from_taylor_hood(
        prob['th'], prob['invinds'], prob['dbcinds'], prob['dbcvals'])


def _flow_statistics(prob, trange):
    """two bins by the parity of the step, the step towards `trange[4]`
    skipped; the pairs of the Reynolds shear stress"""
    from dolfin_navier_scipy_amd import fem
    dt = trange[1] - trange[0]

    def bin_of(t):
        k = int(round((t - trange[0])/dt))
        return -1 if k == 4 else k % 2
    return fem.FlowStatistics(
        pairs=fem.component_pairs(prob['th'], prob['invinds']), nbins=2,
        bin_of=bin_of)


def _means_close(fs, ref, what):
    assert fs.counts.tolist() == ref.counts.tolist(), what
    (mv, mp), (rv, rp) = fs.mean(), ref.mean()
    ev = np.abs(mv - rv).max(axis=1)/np.abs(rv).max(axis=1)
    ep = np.abs(mp - rp).max(axis=1)/np.abs(rp).max(axis=1)
    print(what, ': mean v', ev.max(), 'mean p', ep.max())
    assert np.all(ev <= VTOL), (what, ev)
    assert np.all(ep <= PTOL), (what, ep)


def _sums_of(prob, trange, times, vels, prss):
    """the same sums formed from a trajectory `(time, v with boundary values,
    p)`: every point but the initial one"""
    ref = _flow_statistics(prob, trange)
    assert np.allclose(times, trange, rtol=0, atol=1e-15)
    for k in range(1, len(trange)):
        ref.add(vels[k][prob['invinds']], prss[k], trange[k])
    return ref


@pytest.mark.parametrize('scheme,step6', [('cnab', '1'), ('sbdf2', '1'),
                                          ('cnab', '0')])
def test_statistics_through_the_integrators(gtiu, golden_dir, toy_prob,
                                            monkeypatch, scheme, step6):
    """`resident=dict(statistics=fs)` on the device (two slices of five steps
    and one of one) and on the host path of the same tree, against each other
    and against the sums over the golden trajectory of the reference's own
    integrator; `DNS_STEP6=0`: the fused form of the step"""
    monkeypatch.setenv('DNS_STEP6', step6)
    gold = np.load(os.path.join(
        golden_dir, 'imex_{0}_plain_s0.npz'.format(scheme)))
    integ = gtiu.cnab if scheme == 'cnab' else gtiu.sbdftwo
    inv = toy_prob['invinds']
    got = {}
    for mode in ('device', 'host'):
        kw, _, _ = scenarios.build(variant='plain', seed=0, prob=toy_prob)
        fs = _flow_statistics(toy_prob, kw['trange'])
        cvop = None
        if mode == 'device':
            kw.pop('f_vdp')
            cvop = _toy_cvop(toy_prob)
            kw.update(device_convection=cvop, invinds=inv)
        try:
            _, _, ff = integ(ntimeslices=2,
                             resident=dict(statistics=fs, savevp_times=()),
                             **kw)
        finally:
            if cvop is not None:
                cvop.close()
        assert ff == 0
        assert gtiu.LAST_RUN['statistics_on'] == mode
        last = gtiu.LAST_RUN['statistics']
        for key in fs.KEYS:
            assert np.array_equal(last[key], getattr(fs, key)), key
        got[mode] = fs
    trange = kw['trange']
    ref = _sums_of(toy_prob, trange, gold['times'], gold['vels'],
                   gold['prss'])
    assert ref.counts.tolist() == [5, 6]
    what = '{0} (DNS_STEP6={1})'.format(scheme, step6)
    _means_close(got['device'], got['host'], what + ' device vs host')
    _means_close(got['device'], ref, what + ' device vs golden')
    _means_close(got['host'], ref, what + ' host vs golden')
    # second moments: states within VTOL of their maximum have squares and
    # products within 2 VTOL of the maximum's square; asserted is twice that
    for key in ('s2_v', 's2_p', 'sx'):
        a, b = getattr(got['device'], key), getattr(got['host'], key)
        assert np.abs(b).max() > 0, key
        assert np.abs(a - b).max() <= 4*VTOL*np.abs(b).max(), key


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_solve_nse_statistics(gtiu, golden_dir, toy_prob, scheme):
    """`solve_nse(statistics=fs)` sets up the scenario `plain` (its CPU
    oracle reproduces the golden trajectory to 4e-13): the loop runs resident,
    the sums are those over the golden trajectory, the same numbers as
    through the integrator itself"""
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    kw, _, _ = scenarios.build(variant='plain', seed=0, prob=toy_prob)
    trange = kw['trange']
    skw = dict(A=toy_prob['smc']['A'], M=toy_prob['smc']['M'],
               J=toy_prob['smc']['J'], fv=toy_prob['rhsd']['fv'],
               fp=toy_prob['rhsd']['fp'],
               iniv=kw['appndbcs'](kw['inivel'], []), inip=kw['inip'],
               trange=trange, V=toy_prob['th'], invinds=toy_prob['invinds'],
               dbcinds=toy_prob['dbcinds'], dbcvals=toy_prob['dbcvals'])
    gold = np.load(os.path.join(
        golden_dir, 'imex_{0}_plain_s0.npz'.format(scheme)))
    ref = _sums_of(toy_prob, trange, gold['times'], gold['vels'],
                   gold['prss'])
    fs = _flow_statistics(toy_prob, trange)
    try:
        snu.solve_nse(time_int_scheme=scheme, statistics=fs,
                      return_dictofvelstrs=True, **skw)
    finally:
        snu.clear_cache()
    assert gtiu.LAST_RUN['statistics_on'] == 'device'
    _means_close(fs, ref, scheme + ' solve_nse vs golden')
    with pytest.raises(NotImplementedError):
        snu.solve_nse(time_int_scheme=scheme, statistics=fs,
                      treat_nonl_explicit=False, **skw)


# ---- 6. refusals ----------------------------------------------------------------------------

def test_set_stats_refusals_leave_the_statistics_as_they_were(gtiu, toy_prob):
    from dolfin_navier_scipy_amd import _capi
    NP, NV = toy_prob['smc']['J'].shape
    n = NV + NP
    bins, pairs = _toy_bins(), _toy_pairs(NV, NP)
    lp = ToyLoop(toy_prob)
    try:
        stp, lib = lp.stp, lp.stp.lib
        stp.set_recorder(NST, snap_slots='all')
        stp.set_statistics(bins, nbins=3, pairs=pairs)
        stp.run(9, lp.cf, lp.opts)
        # refused calls, straight at the C-ABI (Python would catch them first)
        ip = _capi.c_int32_p
        b6 = np.zeros(6, dtype=np.int32)
        bad_bin = np.array([0, 1, 3, 0, 0, 0], dtype=np.int32)
        low_bin = np.array([0, -2, 0, 0, 0, 0], dtype=np.int32)
        pi = np.array([0, n], dtype=np.int32)
        pj = np.array([1, 2], dtype=np.int32)
        neg = np.array([0, -1], dtype=np.int32)

        def p(a):
            return a.ctypes.data_as(ip)
        refused = (
            ('nbins', (6, p(b6), 0, 0, None, None, 0)),
            ('nbins', (6, p(b6), 257, 0, None, None, 0)),
            ('nrows', (0, p(b6), 3, 0, None, None, 0)),
            ('bin[2]', (6, p(bad_bin), 3, 0, None, None, 0)),
            ('bin[1]', (6, p(low_bin), 3, 0, None, None, 0)),
            ('pair 1', (6, p(b6), 3, 2, p(pi), p(pj), 0)),
            ('pair 1', (6, p(b6), 3, 2, p(pj), p(neg), 1)),
            # 256 bins x 2^23 products: 2^31 entries and more
            ('accumulator', (6, p(b6), 256, 1 << 23, p(pi), p(pj), 0)),
        )
        for word, args in refused:
            rc = lib.dns_imex_set_stats(stp._h, *args)
            assert rc == _capi.DNS_ERR_BAD_ARGUMENT, word
            assert word.encode() in lib.dns_last_error(), \
                (word, lib.dns_last_error())
        with pytest.raises(_capi.DnsError):                  # bins out of range
            lib_rc = lib.dns_imex_get_stats(stp._h, 2, 2, None, None, None,
                                            None)
            _capi.check(lib_rc)
        # ... the statistics that were there go on, and so did the counter
        assert stp.table_position() == (9, NST - 9)
        stp.run(NST - 9, lp.cf, lp.opts)
        exp = _expected(_rows(stp), bins, 3, pairs)
        assert _check(stp.statistics(), exp, NV, 'after the refusals') <= 1.
        # stepping past the rows
        with pytest.raises(_capi.DnsError) as exc:
            stp.run(1, lp.cf, lp.opts)
        assert exc.value.status == _capi.DNS_ERR_NOT_READY
        # no statistics: nothing to download
        stp.clear_statistics()
        assert lib.dns_imex_get_stats(stp._h, 0, 1, None, None, None, None) \
            == _capi.DNS_ERR_NOT_READY
    finally:
        lp.close()


def test_statistics_on_a_row_partitioned_stepper_are_refused(gtiu, toy_prob):
    """when they are set, and -- set before the stepper was partitioned -- by
    the step"""
    from dolfin_navier_scipy_amd import saddle, _capi, comm as dcomm
    M, A, J = (toy_prob['smc'][k] for k in 'MAJ')
    dt = 5e-3
    cm = dcomm.Comm.rccl(0, 1, 0, dcomm.rccl_unique_id())
    system = saddle.SaddleSystem((M + .5*dt*A).tocsr(), J)
    stp = None
    try:
        system.setup_precond(cheb_degree=6, schur='dense', fhat='explicit')
        stp = saddle.ImexStepper(system, (M - .5*dt*A).tocsr())
        stp.set_state(np.zeros((J.shape[1], 1)))
        stp.set_rhs(dt*toy_prob['rhsd']['fv'], toy_prob['rhsd']['fp'])
        stp.set_statistics(np.zeros(4, dtype=np.int32))
        system.set_comm(cm)
        # (the preconditioner is set up again on a communicator: from here on
        # the system is row-partitioned)
        system.setup_precond(cheb_degree=6, schur='dense', fhat='explicit')
        with pytest.raises(_capi.DnsError) as exc:            # by the setter
            stp.set_statistics(np.zeros(4, dtype=np.int32))
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        assert 'partitioned' in str(exc.value)
        cf = saddle.ImexStepper.coeffs(a_c=1., cn_c=1.5*dt, cn_o=-.5*dt,
                                       pscale=-1./dt)
        with pytest.raises(_capi.DnsError) as exc:            # by the step
            stp.step(cf, nfc_new=np.zeros(J.shape[1]),
                     opts=saddle.solve_opts(method='gmres', rtol=1e-10))
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        assert 'statistics on a row-partitioned' in str(exc.value)
    finally:
        if stp is not None:
            stp.close()
        system.set_comm(None)
        system.close()
        cm.close()
