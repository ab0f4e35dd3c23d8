"""Device-resident POD of the explicit loops: the snapshot ensemble
(`k_ensemble_step`, `dns_imex_set_ensemble`), the Gram matrix on the fp64
matrix cores (`k_ens_spmm`, `k_ens_gram`, `k_ens_gram_reduce`), the linear
combinations (`k_ens_combine`), `resident=dict(pod=...)` of `cnab` / `sbdftwo`.

Tolerances.  Integer data: every sum is exact in fp64, the device equals NumPy
bit for bit (the check of the MFMA lane maps).  Real data, `u = 2^-53`, any
summation order, with or without fma:
    |G_dev - G_ref|_ij   <= 1.01 (NV + maxrownnz(W) + 2) u sum_k |E_ik| (|W||E_j|)_k
    |out_dev - coef E|_qk <= 1.01 (m + 1) u sum_s |coef_qs| |E_sk|
with the references in `np.longdouble` (`pod_model`).  The copy node writes
the bits of the recorder's snapshot of `v`.  Orthonormality of the modes: the
tolerance fixed on the CPU (`pod_model.ORTHO_TOL`).  The method of snapshots
loses orthonormality like `u |G|_2 / lambda_k` (the centring cancels in an
`m x m` matrix of RAW snapshots): on the toy wake `|G|_2 = 6.3`, `lambda =
1.1e-2, 8e-4, 8e-5`; measured on the device for the leading 1, 2, 3 modes:
5.4e-14, 2.2e-13, 4.3e-12 (CNAB), 1.5e-14, 1.2e-12, 2.2e-12 (SBDF2), the host
model `evaluate` gives 1.3e-14, 4.2e-13, 4.2e-13 on its own trajectory.  So
every kept mode and every pair of them is asserted against the derived law
`ORTHO_C m u |G|_2 / sqrt(lambda_k lambda_l)` (`pod_model.ortho_bound`; the
constant is measured on the host model in the CPU test, margin 10), and the
leading mode, whose figure lies below it, at `ORTHO_TOL` as well.

Measured worst error / bound (MI355X): Gram 0.070 (W = I), 0.027 (W) on seeded
data and 0.011 through `cnab`; combine 0.16 on seeded data, 0.34 through
`cnab`.

The three ways to take the steps (one `run`, slices of 7 / 7 / 10,
`dns_imex_step`) fill the ensemble with the same bits where the TRAJECTORY does
not depend on the split: plain launches, a warm start of order <= 1, no
residual carry (`SETTINGS['plain']`).  With the defaults of the other tests
(graph replay, quartic warm start, residual carry) each way still equals its own
recorder bit for bit, but the trajectories differ in their last bits -- the
steps are iterative solves to `rtol = 1e-12` whose warm start and batch form
depend on how the steps are split into calls, and tables set again re-prime the
six-node step: max |run - slices| = 6.3e-13, |run - step| = 1.3e-14 (CNAB),
3.5e-14 and 3.4e-14 (SBDF2) at max |v| = 1.4; with graph replay and neither
extrapolation nor carry `run` and the slices agree to the last bit and
`dns_imex_step` differs by 2.6e-13 / 5.1e-13.
"""
import numpy as np
import pytest
import scipy.sparse as sps

import feedback_setup as fs
import pod_model
import scenarios

pytestmark = pytest.mark.gpu

NST, EVERY = 24, 2
CHUNK = 1024                    # kEnsChunk of csrc/ensemble_host.hpp
NV_CHUNKS = 2*CHUNK + 37        # three k-chunks, a ragged last one


@pytest.fixture(scope='module')
def gtiu():
    from dolfin_navier_scipy_amd import time_int_utils, _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    return time_int_utils


# ---- 1. / 2. the stateless kernels -------------------------------------------------

def _padded(S, ld):
    """`S` in rows of `ld` entries, NaN behind its columns"""
    E = np.full((S.shape[0], ld), np.nan)
    E[:, :S.shape[1]] = S
    return E


def _ld_for(nv):
    return nv + 2 + (nv % 2)                # even, > nv


def _int_weights(nv, rng):
    """small-integer symmetric CSR with an empty row (and column)"""
    dens = min(1., 6./nv)
    A = sps.random(nv, nv, density=dens, random_state=rng,
                   data_rvs=lambda k: rng.integers(-2, 3, size=k).astype(
                       np.float64))
    W = sps.lil_matrix((A + A.T + sps.diags(rng.integers(1, 4, size=nv))
                        ).astype(np.float64))
    if nv > 1:
        e = nv//2
        W[e, :] = 0.
        W[:, e] = 0.
    W = sps.csr_matrix(W)
    W.eliminate_zeros()
    assert abs(W - W.T).nnz == 0
    assert nv == 1 or np.diff(W.indptr).min() == 0
    return W


@pytest.mark.parametrize('nv', [1, 3, 63, 64, 65, NV_CHUNKS])
@pytest.mark.parametrize('m', [1, 15, 16, 17, 33])
def test_kernels_are_exact_on_integer_data(gtiu, m, nv):
    from dolfin_navier_scipy_amd import saddle
    rng = np.random.default_rng(1000*m + nv)
    S = rng.integers(-3, 4, size=(m, nv)).astype(np.float64)
    E = _padded(S, _ld_for(nv))
    W = _int_weights(nv, rng)
    for what, Wk in (('W = I', None), ('W', W)):
        G = saddle.ensemble_gram(E, Wk, nv=nv)
        want = S @ S.T if Wk is None else S @ (Wk @ S.T)
        assert np.isfinite(G).all(), (what, 'the padding was read')
        assert np.array_equal(G, want), (what, np.abs(G - want).max())
    for r in (1, 16, 17):
        coef = rng.integers(-3, 4, size=(r, m)).astype(np.float64)
        out = saddle.ensemble_combine(E, coef, nv=nv)
        assert out.shape == (r, nv)
        assert np.array_equal(out, coef @ S), (r, np.abs(out - coef @ S).max())


def test_gram_of_the_identity_weight_puts_rows_and_columns_right(gtiu):
    """`E = [I 0]`-like data with an ASYMMETRIC weight product: `G = E Y^T`
    with `Y = E W` is only symmetric because `W` is -- hand the kernels an
    ensemble whose rows are unit vectors, so `G = W[:m, :m]` entry by entry,
    with `W`'s entries all different"""
    from dolfin_navier_scipy_amd import saddle
    m, nv = 33, 40
    S = np.zeros((m, nv))
    S[np.arange(m), np.arange(m)] = 1.
    B = np.arange(1., nv*nv + 1.).reshape((nv, nv))
    W = sps.csr_matrix(np.triu(B) + np.triu(B, 1).T)     # symmetric, distinct
    G = saddle.ensemble_gram(_padded(S, _ld_for(nv)), W, nv=nv)
    assert np.array_equal(G, W.toarray()[:m, :m])


@pytest.mark.parametrize('m,nv', [(17, 65), (33, NV_CHUNKS)])
def test_kernels_within_their_bounds_on_real_data(gtiu, m, nv):
    from dolfin_navier_scipy_amd import saddle
    from dolfin_navier_scipy_amd.fem import pod as podmod
    rng = np.random.default_rng(7 + nv)
    S = rng.standard_normal((m, nv))*np.exp(rng.standard_normal((m, 1)))
    E = _padded(S, _ld_for(nv))
    A = sps.random(nv, nv, density=min(1., 8./nv), random_state=rng,
                   data_rvs=rng.standard_normal)
    W = sps.csr_matrix(A + A.T + 4.*sps.identity(nv))
    worst = {}
    for what, Wk in (('W = I', None), ('W', W)):
        G = saddle.ensemble_gram(E, Wk, nv=nv)
        assert np.array_equal(G, G.T), what
        assert np.array_equal(G, saddle.ensemble_gram(E, Wk, nv=nv)), what
        err = np.abs(G.astype(np.longdouble)
                     - pod_model.gram_longdouble(S, Wk))
        bound = podmod.gram_bound(S, Wk)
        worst[what] = float((err/bound).max())
        assert np.all(err <= bound), (what, worst[what])
    coef = rng.standard_normal((17, m))
    out = saddle.ensemble_combine(E, coef, nv=nv)
    assert np.array_equal(out, saddle.ensemble_combine(E, coef, nv=nv))
    err = np.abs(out.astype(np.longdouble)
                 - pod_model.combine_longdouble(S, coef))
    bound = podmod.combine_bound(S, coef)
    worst['combine'] = float((err/bound).max())
    assert np.all(err <= bound), worst
    # the stated order: acc = fma(c, e, acc), s ascending -- without fma in
    # NumPy the last bit may differ, so this is a bound check only
    print('m', m, 'nv', nv, ': worst error / bound', worst)


# ---- 3. the copy node ---------------------------------------------------------------

class Loop(object):
    """CNAB / SBDF2 coefficients on the toy problem from a seeded state"""

    def __init__(self, prob, scheme='cnab', dt=5e-3, seed=11):
        from dolfin_navier_scipy_amd import saddle, convection
        M, A, J = (prob['smc'][k] for k in 'MAJ')
        rhsd = prob['rhsd']
        self.M, self.dt = sps.csr_matrix(M), dt
        NP, NV = J.shape
        if scheme == 'cnab':
            F, R1, g = M + .5*dt*A, M - .5*dt*A, dt*rhsd['fv']
            self.cf = saddle.ImexStepper.coeffs(
                a_c=1., cn_c=1.5*dt, cn_o=-.5*dt, pscale=-1./dt, extrapolate=4)
        else:
            F, R1, g = M + 2./3*dt*A, M, 2./3*dt*rhsd['fv']
            self.cf = saddle.ImexStepper.coeffs(
                a_c=4./3, a_p=-1./3, cn_c=4./3*dt, cn_o=-2./3*dt,
                pscale=-1./dt, extrapolate=4)
        self.system = saddle.SaddleSystem(sps.csr_matrix(F), J)
        self.system.setup_precond(cheb_degree=6, schur='dense')
        self.stp = saddle.ImexStepper(self.system, sps.csr_matrix(R1))
        self.cvop = convection.ConvectionP2.from_taylor_hood(
            prob['th'], prob['invinds'], prob['dbcinds'], prob['dbcvals'])
        rng = np.random.default_rng(seed)
        self.v0 = 1e-1*rng.standard_normal((NV, 1))
        self.stp.set_state(self.v0, v_p=self.v0)
        self.stp.set_rhs(g, rhsd['fp'])
        self.stp.set_convection(self.cvop, scale=-1.0)
        self.opts = saddle.solve_opts(method='gmres', rtol=1e-12, maxiter=400,
                                      restart=60, check_every=2,
                                      use_graph=True, reorth=2)

    def close(self):
        self.stp.close()
        self.cvop.close()
        self.system.close()


def _slots(first, n, spare=0):
    """global slots of the steps `first .. first + n` of NST: every EVERY-th
    is kept"""
    return np.array([(s + 1)//EVERY - 1 + spare if (s + 1) % EVERY == 0
                     else -1 for s in range(first, first + n)],
                    dtype=np.int32)


def _fill(lp, how, nslots, spare=0):
    """NST steps with recorder and ensemble on together; returns the
    ensemble and the recorder's `v` of the kept steps, in slot order"""
    stp = lp.stp
    parts = {'run': [NST], 'slices': [7, 7, 10], 'step': [NST]}[how]
    first, recv = 0, []
    for n in parts:
        glob = _slots(first, n, spare)
        local = np.where(glob >= 0, np.cumsum(glob >= 0) - 1, -1)
        if local.max() >= 0:
            stp.set_recorder(n, snap_slots=local)
        stp.set_ensemble(glob, nslots=nslots, reset=(first == 0))
        if how == 'step':
            for _ in range(n):
                stp.step(lp.cf, opts=lp.opts)
        else:
            stp.run(n, lp.cf, lp.opts)
        if local.max() >= 0:
            recv.append(stp.record_snapshots()[0])
        first += n
    return stp.ensemble(), np.vstack(recv)


# (use_graph, order of the warm start, residual carry)
SETTINGS = {'replay': (True, 4, True),      # the defaults of the other tests
            'replay0': (True, 0, False),
            'plain': (False, 1, False)}


@pytest.fixture(scope='module')
def filled(gtiu, toy_prob):
    """{(settings, scheme, how): (ensemble, recorder's v)} of the three ways
    to take the NST steps, computed once"""
    m = NST//EVERY
    out = {}
    for name, (graph, extr, carry) in SETTINGS.items():
        for scheme in ('cnab', 'sbdf2'):
            for how in ('run', 'slices', 'step'):
                lp = Loop(toy_prob, scheme)
                try:
                    lp.cf.extrapolate_x0 = extr
                    lp.cf.carry_residual = int(carry)
                    lp.opts.use_graph = int(graph)
                    # (two spare slots in front, one behind: never written)
                    out[name, scheme, how] = _fill(lp, how, m + 3, spare=2)
                    assert lp.stp.table_position()[0] == \
                        {'slices': 10}.get(how, NST)
                finally:
                    lp.close()
    return out


@pytest.mark.parametrize('how', ['run', 'slices', 'step'])
@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
@pytest.mark.parametrize('settings', sorted(SETTINGS))
def test_copy_node_writes_the_recorders_bits(filled, settings, scheme, how):
    """one `run`, slices of 7 / 7 / 10 (the ensemble lasts, the recorder is
    planned anew) and `dns_imex_step` (every row launched for twice), with
    both attachments on together: the bits of the recorder's `v`; slots
    nobody is sent to stay 0"""
    m = NST//EVERY
    ens, recv = filled[settings, scheme, how]
    assert np.array_equal(ens[:2], np.zeros_like(ens[:2]))
    assert np.array_equal(ens[-1], np.zeros_like(ens[-1]))
    assert recv.shape == (m, ens.shape[1])
    assert np.abs(recv).max(axis=1).min() > 0
    assert np.array_equal(ens[2:2 + m], recv)
    # the snapshots differ from one another (the flow moves)
    assert np.abs(np.diff(recv, axis=0)).max(axis=1).min() > 0


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_ensemble_is_the_same_however_the_steps_are_taken(filled, scheme):
    """the ensembles of the three ways, bit for bit, where the trajectory
    does not depend on the split (module docstring); with graph replay and
    no extrapolation the re-armed slices against the one `run`; the
    differences under the defaults are printed"""
    def ways(name):
        return [filled[name, scheme, how][0]
                for how in ('run', 'slices', 'step')]
    run, sl, st = ways('plain')
    assert np.array_equal(run, sl)
    assert np.array_equal(run, st)
    run, sl, st = ways('replay0')
    assert np.array_equal(run, sl)
    print(scheme, 'replay0: max |run - step|', np.abs(run - st).max())
    run, sl, st = ways('replay')
    print(scheme, 'replay: max |run - slices|', np.abs(run - sl).max(),
          ', max |run - step|', np.abs(run - st).max(), ', max |v|',
          np.abs(run).max())


def test_ensemble_operations_of_the_stepper(gtiu, toy_prob):
    """`ensemble_gram` / `ensemble_combine` of the stepper against the
    stateless entries on the downloaded ensemble: the same launchers, the
    same bits; `m` below `nslots`; the weights handed over twice"""
    from dolfin_navier_scipy_amd import saddle
    m = NST//EVERY
    lp = Loop(toy_prob)
    try:
        ens, _ = _fill(lp, 'run', m)
        stp, M = lp.stp, lp.M
        NV = ens.shape[1]
        E = _padded(ens, -(-NV//64)*64)
        for Wk in (None, M):
            G = stp.ensemble_gram(Wk)
            assert np.array_equal(G, saddle.ensemble_gram(E, Wk, nv=NV))
            assert np.array_equal(G, stp.ensemble_gram(Wk))
            assert np.array_equal(stp.ensemble_gram(Wk, m=5), G[:5, :5])
        coef = np.random.default_rng(3).standard_normal((4, m))
        out = stp.ensemble_combine(coef)
        assert np.array_equal(out, saddle.ensemble_combine(E, coef, nv=NV))
        assert np.array_equal(stp.ensemble_combine(coef[:, :5], m=5),
                              saddle.ensemble_combine(E[:5], coef[:, :5],
                                                      nv=NV))
    finally:
        lp.close()


# ---- 4. end to end -------------------------------------------------------------------

def _toy_cvop(prob):
    from dolfin_navier_scipy_amd import convection
    return convection.ConvectionP2.from_taylor_hood(
        prob['th'], prob['invinds'], prob['dbcinds'], prob['dbcvals'])


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_pod_through_the_time_loops(gtiu, toy_prob, scheme):
    from dolfin_navier_scipy_amd.fem import SnapshotPOD
    integ = gtiu.cnab if scheme == 'cnab' else gtiu.sbdftwo
    inv = toy_prob['invinds']
    M = sps.csr_matrix(toy_prob['smc']['M'])
    res, calls = {}, {}
    for mode in ('device', 'plain', 'host'):
        kw, rec, _ = scenarios.build(variant='plain', seed=0, prob=toy_prob,
                                     Nts=26, tE=0.13)
        pod = SnapshotPOD(M, every=EVERY, nmodes=3)
        rsd = dict(savevp_times=())
        if mode != 'plain':
            rsd.update(pod=pod, pod_snapshots=True)
        cvop = None
        if mode != 'host':
            kw.pop('f_vdp')
            cvop = _toy_cvop(toy_prob)
            kw.update(device_convection=cvop, invinds=inv)
        try:
            _, _, ff = integ(ntimeslices=3, resident=rsd, **kw)
        finally:
            if cvop is not None:
                cvop.close()
        assert ff == 0
        calls[mode] = gtiu.LAST_RUN['run_calls']
        if mode != 'plain':
            assert gtiu.LAST_RUN['pod_on'] == mode
            res[mode] = gtiu.LAST_RUN['pod']
    assert calls['device'] == calls['plain'] > 0 and calls['host'] == 0
    dev, host = res['device'], res['host']
    trange = kw['trange']
    kept = [k for k in range(2, len(trange)) if k % EVERY == 0]
    m = len(kept)
    assert np.array_equal(dev['times'], np.asarray(trange)[kept])
    E = dev['snapshots']
    assert E.shape == (m, inv.size) and dev['gram'].shape == (m, m)
    # the Gram matrix against the model on the device's OWN snapshots
    ev = pod.evaluate(E)
    assert np.array_equal(dev['gram'], dev['gram'].T)
    gerr = np.abs(dev['gram'].astype(np.longdouble)
                  - pod_model.gram_longdouble(E, M))
    gb = pod.bound_gram(E)
    assert np.all(gerr <= gb), float((gerr/gb).max())
    # ... and against the host path of the same tree: the two bounds plus
    # what the states' difference moves the exact value by,
    # |dG| <= |dE| |W| |E|^T + |E| |W| |dE|^T + |dE| |W| |dE|^T
    dE = np.abs(E - host['snapshots'])
    Wa, Ea = abs(M), np.abs(E)
    shift = dE @ (Wa @ Ea.T) + Ea @ (Wa @ dE.T) + dE @ (Wa @ dE.T)
    assert np.all(np.abs(dev['gram'] - host['gram'])
                  <= gb + pod.bound_gram(host['snapshots']) + shift)
    print(scheme, ': |E_dev - E_host| max', dE.max(), ', gram error / bound',
          float((gerr/gb).max()))
    # modes and mean flow against coef @ E with the SAME coef
    r = dev['modes'].shape[0]
    assert r == 3 and dev['coef'].shape == (r + 1, m)
    full = np.vstack([dev['modes'], dev['mean'][None, :]])
    cerr = np.abs(full.astype(np.longdouble)
                  - pod_model.combine_longdouble(E, dev['coef']))
    cb = pod.bound_combine(E, dev['coef'])
    assert np.all(cerr <= cb), float((cerr/cb).max())
    print(scheme, ': combine error / bound', float((cerr/cb).max()))
    # the decomposition is the host's algebra on the device's Gram matrix
    dec = pod.decompose(dev['gram'])
    assert np.array_equal(dec['coef'], dev['coef'])
    assert np.array_equal(dec['sigma'], dev['sigma'])
    # (Weyl: eigenvalues move by at most |dG|_2 <= m max|dG|, the centring
    # is a projection; d sigma = d lambda / (sigma + sigma'))
    assert np.all(np.abs(dev['sigma'] - ev['sigma'])
                  <= 2*m*gb.max()/ev['sigma'])
    # orthonormality (module docstring): EVERY kept mode and every pair of
    # them within the derived bound whose constant the CPU test fixes, the
    # leading mode at the CPU test's tolerance for well-conditioned data
    orth = pod_model.ortho_error(dev, M)
    ob = pod_model.ortho_bound(dev['gram'], dev['sigma'])
    print(scheme, ': |modes W modes^T - I| of the leading 1, 2, 3 modes',
          [float(orth[:k, :k].max()) for k in (1, 2, 3)],
          ', worst entry / bound', float((orth/ob).max()))
    assert np.all(orth <= ob), float((orth/ob).max())
    assert orth[0, 0] <= pod_model.ORTHO_TOL


# ---- 5. coexistence and refusals -----------------------------------------------------

def _femp(prob):
    return dict(V=prob['th'], invinds=prob['invinds'],
                dbcinds=prob['dbcinds'], dbcvals=prob['dbcvals'],
                nu=prob['nu'])


def test_rows_of_the_other_attachments_with_the_ensemble(gtiu, toy_prob):
    """feedback, recorder, functionals, statistics, quadratics and the
    ensemble: six nodes in front of the step; the other five say what they
    say without the sixth"""
    from dolfin_navier_scipy_amd import fem
    nst = NST
    th, femp = toy_prob['th'], _femp(toy_prob)
    NP, NV = toy_prob['smc']['J'].shape
    M = sps.csr_matrix(toy_prob['smc']['M'])
    C, B = fs.sensors_actuators(th, toy_prob['invinds'], M)
    obs = fs.observer(7, C.shape[0], B.shape[1])
    hN = obs['ha'].shape[0]
    qf = fem.kinetic_energy(th, femp) + fem.dissipation(th, femp)
    fn = fem.pressure_difference(th, 3, 5)
    pairs = np.array([(0, 1), (NV - 1, NV), (NV + NP - 1, 2)], dtype=np.int32)
    got = []
    for with_e in (True, False):
        lp = Loop(toy_prob)
        try:
            stp = lp.stp
            stp.set_feedback(C, B, obs['ha'], obs['hb'], obs['hc'], c_n=.5,
                             c_c=.5, dt=lp.dt)
            stp.set_feedback_state(obs['inihx'], np.zeros(hN),
                                   obs['hc'] @ obs['inihx'])
            stp.set_feedback_table(nst, None)
            stp.set_recorder(nst, snap_slots='all')
            stp.set_functionals(fn, nst, lp.dt)
            stp.set_statistics(np.zeros(nst, dtype=np.int32), nbins=1,
                               pairs=pairs, reset=True)
            stp.set_quadratics(qf, nst, lp.dt)
            if with_e:
                stp.set_ensemble(_slots(0, nst), nslots=nst//EVERY)
            stp.run(9, lp.cf, lp.opts)
            stp.run(nst - 9, lp.cf, lp.opts)
            vs, ps = stp.record_snapshots()
            got.append(dict(vs=vs, ps=ps, fb=stp.feedback_log(),
                            fn=stp.get_functionals(), st=stp.statistics(),
                            qd=stp.get_quadratics(),
                            ens=stp.ensemble() if with_e else None))
        finally:
            lp.close()
    a, b = got
    assert np.abs(a['fb'][1]).max() > 0 and np.abs(a['qd']).min() > 0
    assert np.array_equal(a['ens'], a['vs'][EVERY - 1::EVERY])
    assert np.array_equal(a['vs'], b['vs']) and np.array_equal(a['ps'], b['ps'])
    assert np.array_equal(a['fb'][0], b['fb'][0])
    assert np.array_equal(a['fb'][1], b['fb'][1])
    assert np.array_equal(a['fn'], b['fn'])
    assert np.array_equal(a['qd'], b['qd'])
    assert a['st']['counts'].tolist() == [nst]
    for k in a['st']:
        assert np.array_equal(a['st'][k], b['st'][k]), k


def test_ensemble_off_leaves_the_step_as_it_was(gtiu, toy_prob):
    la, lb = Loop(toy_prob), Loop(toy_prob)
    try:
        la.stp.set_ensemble(_slots(0, 8), nslots=4)
        la.stp.run(4, la.cf, la.opts)
        la.stp.clear_ensemble()
        with pytest.raises(ValueError):
            la.stp.ensemble()
        lb.stp.run(4, lb.cf, lb.opts)
        la.stp.run(20, la.cf, la.opts)
        lb.stp.run(20, lb.cf, lb.opts)
        assert np.array_equal(la.stp.get_state()[0], lb.stp.get_state()[0])
        assert np.array_equal(la.stp.get_state()[1], lb.stp.get_state()[1])
        assert la.stp.last_run == lb.stp.last_run
    finally:
        la.close()
        lb.close()


def test_refusals_leave_the_ensemble_as_it_was(gtiu, toy_prob):
    from dolfin_navier_scipy_amd import _capi
    lp = Loop(toy_prob)
    try:
        stp = lp.stp
        lib, i32 = stp.lib, _capi.c_int32_p
        stp.set_ensemble(_slots(0, 8), nslots=4)
        stp.run(8, lp.cf, lp.opts)
        before = stp.ensemble()
        assert np.abs(before).max(axis=1).min() > 0
        bad = np.array([0, 4, -1, 1], dtype=np.int32)       # slot >= nslots
        for slots, nslots in ((bad, 4), (np.array([-2], dtype=np.int32), 4),
                              (np.zeros(2, dtype=np.int32), 0)):
            rc = lib.dns_imex_set_ensemble(
                stp._h, int(slots.size), slots.ctypes.data_as(i32), nslots, 1)
            assert rc == _capi.DNS_ERR_BAD_ARGUMENT, (slots, nslots)
            assert b'ensemble' in lib.dns_last_error()
        assert lib.dns_imex_set_ensemble(stp._h, 0, bad.ctypes.data_as(i32),
                                         4, 0) == _capi.DNS_ERR_BAD_ARGUMENT
        assert stp.table_position()[0] == 8         # (no rewind either)
        assert np.array_equal(stp.ensemble(), before)
        # out of range for the getters and the operations
        g = np.zeros(25)
        for m in (0, 5):
            assert lib.dns_imex_ensemble_gram(stp._h, None, m, _capi.dptr(g)) \
                == _capi.DNS_ERR_BAD_ARGUMENT
            assert lib.dns_imex_ensemble_combine(
                stp._h, m, 1, _capi.dptr(g), _capi.dptr(g)) \
                == _capi.DNS_ERR_BAD_ARGUMENT
        with pytest.raises(_capi.DnsError):
            stp.ensemble(3, 2)
        with pytest.raises(_capi.DnsError):
            stp.ensemble_gram(sps.identity(5, format='csr'))
        # stepping past the table
        with pytest.raises(_capi.DnsError) as exc:
            stp.run(1, lp.cf, lp.opts)
        assert exc.value.status == _capi.DNS_ERR_NOT_READY
        # a re-arm without reset keeps the snapshots, with reset zeroes them
        stp.set_ensemble(np.full(2, -1, dtype=np.int32), nslots=4)
        assert np.array_equal(stp.ensemble(), before)
        stp.set_ensemble(np.full(2, -1, dtype=np.int32), nslots=4, reset=True)
        assert not stp.ensemble().any()
        stp.clear_ensemble()
        assert lib.dns_imex_get_ensemble(stp._h, 0, 1, None) \
            == _capi.DNS_ERR_NOT_READY
    finally:
        lp.close()


def test_ensemble_on_a_row_partitioned_stepper_is_refused(gtiu, toy_prob):
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
            stp.set_ensemble(np.zeros(4, dtype=np.int32))
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        assert 'ensemble on a row-partitioned' in str(exc.value)
    finally:
        if stp is not None:
            stp.close()
        system.set_comm(None)
        system.close()
        cm.close()
