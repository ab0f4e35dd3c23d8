"""Device-resident boundary feedback (`k_lti_bc_step`,
`dns_imex_set_feedback_boundary`, `time_int_utils.BoundaryFeedback`): the
kernel against its definition, zero gain and replayed inputs against the
`bcs_time_only` loop, the resident loop against the per-step host path and the
CPU oracle, slices, batches, determinism, `solve_nse`, limits and refusals.

The 22 x 8 channel; its inflow dofs are the controlled boundary
(`boundary_feedback_setup`).  Tolerances: states 1e-8 relative (`VTOL` /
`PTOL`, `M`-norm / 2-norm as in `test_gpu_feedback.py`), logs and memory 1e-8
relative, the kernel 1e-13 of the sum of the absolute products (`KTOL`).

Not covered: a RESTORED batch.  `test_gpu_feedback`'s way of forcing one needs
the bench system and 256 steps (a jump at step 128); at the 24 steps of the toy
channel no batch is rejected.
"""
import numpy as np
import pytest
import scipy.sparse as sps

import boundary_feedback_setup as bs
import feedback_setup as fs
import scenarios
from oracle import imex_oracle

pytestmark = pytest.mark.gpu

VTOL, PTOL = 1e-8, 1e-8
KTOL = 1e-13
WEIGHTS = dict(cnab=lambda dt: ((-1., 1., 0.), (.5*dt, .5*dt, 0.)),
               sbdf2=lambda dt: ((-1., 4/3, -1/3), (2/3*dt, 0., 0.)))


@pytest.fixture(scope='module')
def gtiu():
    from dolfin_navier_scipy_amd import time_int_utils, _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    return time_int_utils


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max()/np.abs(b).max()


def _integ(mod, scheme):
    return mod.cnab if scheme == 'cnab' else mod.sbdftwo


def run_resident(gtiu, prob, scheme='cnab', resident=None, ntimeslices=10,
                 **kwb):
    """the drop-in loop with device convection and `resident=`; returns the
    recorder's arrays, the final state, a copy of `LAST_RUN` and the object"""
    kw, rec, fb = bs.build(gtiu, prob, **kwb)
    cvop, statvals = bs.toy_cvop(prob)
    rsd = dict(static_dbcvals=statvals, savevp_times=None)
    rsd.update(resident or {})
    try:
        v, p, ff = _integ(gtiu, scheme)(
            device_convection=cvop, invinds=prob['invinds'], resident=rsd,
            ntimeslices=ntimeslices, **kw)
    finally:
        cvop.close()
    assert ff == 0
    times, vels, prss = rec.arrays()
    return dict(t=times, v=vels, p=prss, vend=v, pend=p, fb=fb,
                last=dict(gtiu.LAST_RUN), kw=kw)


def _state_distance(prob, a, b):
    """worst relative `M`-norm (inner velocities) / 2-norm (pressures) over
    the saved steps"""
    M, inv = prob['smc']['M'], prob['invinds']
    assert np.array_equal(a['t'], b['t'])
    ev = max(fs.mnorm(M, x[inv] - y[inv])/fs.mnorm(M, y[inv])
             for x, y in zip(a['v'], b['v']))
    ep = max(np.linalg.norm(x - y)/np.linalg.norm(y)
             for x, y in zip(a['p'][1:], b['p'][1:]))
    return ev, ep


# ---- 1. the kernel against its definition -------------------------------------

class ToyBcLoop(object):
    """a CNAB stepper on the toy channel with boundary feedback set by hand:
    random right-hand-side tables, the Dirichlet table with `base`, the
    weights of either scheme"""

    def __init__(self, prob, hN=12, Nu=1, weights='cnab', literal=False,
                 with_b=False, nst=8, seed=11, dt=5e-3, setup=True):
        from dolfin_navier_scipy_amd import saddle
        M, A, J = (prob['smc'][k] for k in 'MAJ')
        self.M, self.dt, self.nst = M, dt, nst
        NP, NV = J.shape
        self.NV, self.NP = NV, NP
        self.system = saddle.SaddleSystem((M + .5*dt*A).tocsr(), J)
        self.system.setup_precond(cheb_degree=6, schur='dense')
        self.stp = saddle.ImexStepper(self.system, (M - .5*dt*A).tocsr())
        self.cvop, self.statvals = bs.toy_cvop(prob)
        rng = np.random.default_rng(seed)
        skw, _, aux = scenarios.build(variant='movingbc', seed=seed,
                                      prob=prob)
        self.stp.set_state(skw['inivel'])
        self.stp.set_convection(self.cvop, scale=-1.0)
        self.cf = saddle.ImexStepper.coeffs(a_c=1., cn_c=1.5*dt, cn_o=-.5*dt,
                                            pscale=-1./dt, extrapolate=4)
        self.opts = saddle.solve_opts(method='gmres', rtol=1e-12, maxiter=400,
                                      restart=60, check_every=2,
                                      use_graph=True, reorth=2)
        _, _, cntinds, cntbase = bs.split(prob)
        self.C = bs.full_sensors(prob)[:, prob['invinds']].tocsr()
        self.S, self.base = bs.shape_matrix(cntbase, Nu, scale=.3), cntbase
        self.obs = fs.observer(seed, 3, Nu, hN=hN, gain=.5)
        self.B = fs.sensors_actuators(prob['th'], prob['invinds'], M)[1] \
            if with_b else sps.csr_matrix((NV, Nu))
        assert self.B.shape == (NV, Nu)
        self.terms = None
        if not literal:
            stm, vdim, inv = prob['stms'], prob['th'].vdim, prob['invinds']
            E = sps.csr_matrix((np.ones(cntinds.size),
                                (cntinds, np.arange(cntinds.size))),
                               shape=(vdim, cntinds.size)) @ self.S
            self.terms = tuple(sps.csr_matrix(m) for m in (
                -(stm['A'] @ E)[inv, :], (stm['M'] @ E)[inv, :],
                -(stm['J'] @ E)))
        self.wm, self.wa = WEIGHTS[weights](dt)
        # the rows a host would tabulate for u = 0 (the lifting of `base`
        # among them), each step its own
        stm, lift = prob['stms'], np.zeros((prob['th'].vdim, 1))
        lift[cntinds, 0] = cntbase
        g0 = dt*(aux['cfv'] - (stm['A'] @ lift)[prob['invinds'], :])[:, 0]
        gp0 = (aux['cfp'] - stm['J'] @ lift)[:, 0]
        self.gtab = g0 + 1e-5*rng.standard_normal((nst, NV))
        self.gptab = gp0 + 1e-6*rng.standard_normal((nst, NP))
        self.drift = rng.standard_normal((nst, hN))
        self.hx = self.obs['inihx'][:, 0].copy()
        self.fl = rng.standard_normal(hN)
        self.uc = self.obs['hc'] @ self.hx
        self.up = rng.standard_normal(Nu)
        if setup:
            self.arm()

    def arm(self, table_rows=None):
        stp, obs = self.stp, self.obs
        Ba, Bm, Bj = (None,)*3 if self.terms is None else self.terms
        stp.set_feedback(self.C, self.B, obs['ha'], obs['hb'], obs['hc'],
                         c_n=.5, c_c=.5, dt=self.dt)
        stp.set_feedback_boundary(self.S, self.base,
                                  col0=len(self.statvals), Ba=Ba, Bm=Bm,
                                  Bj=Bj, wm=self.wm, wa=self.wa)
        stp.set_feedback_state_bc(self.hx, self.fl, self.uc, self.up)
        stp.set_rhs_table(self.gtab, self.gptab)
        rows = self.nst + 1 if table_rows is None else table_rows
        self.tab = np.tile(np.concatenate([self.statvals, self.base]),
                           (rows, 1))
        self.tab[0, len(self.statvals):] = self.base + self.S @ self.uc
        self.cvop.set_dbc_table(self.tab)
        stp.set_feedback_table(self.nst, self.drift)

    def run(self, n):
        self.stp.run(n, self.cf, self.opts)

    def close(self):
        self.stp.close()
        self.cvop.close()
        self.system.close()


@pytest.mark.parametrize('hN,Nu,weights,literal,with_b', [
    (1, 1, 'cnab', False, False), (12, 2, 'sbdf2', False, True),
    (128, 2, 'cnab', False, False), (12, 1, 'cnab', True, False),
    (128, 1, 'sbdf2', True, False)])
def test_bc_kernel_against_its_definition(gtiu, toy_prob, hN, Nu, weights,
                                          literal, with_b):
    """8 steps, one `run(1)` each, every quantity recomputed from the device's
    own previous state: `y`, `f`, `hx_n`, `u_n`, the slot (`u_c`, `u_p`), the
    Dirichlet row, `geff`, `gpeff`, each within KTOL of the sum of the absolute
    products; the rows the kernel must not touch yet (row 0, the row after the
    next) keep the host's bits"""
    lp = ToyBcLoop(toy_prob, hN=hN, Nu=Nu, weights=weights, literal=literal,
                   with_b=with_b)
    try:
        stp, obs, dt, nst = lp.stp, lp.obs, lp.dt, lp.nst
        ha, hb, hc = obs['ha'], obs['hb'], obs['hc']
        S, base, nstat = lp.S, lp.base, len(lp.statvals)
        got = stp.feedback_state_bc()
        want = (lp.hx, lp.fl, lp.uc, lp.up)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        hx, fl, uc, up = want
        absC = abs(lp.C)
        v = stp.get_state()[0]
        for k in range(nst):
            lp.run(1)
            ghx, gfl, guc, gup = stp.feedback_state_bc()
            ylog, ulog = stp.feedback_log(k, 1)
            y = ylog[0]
            bound = KTOL*(absC @ np.abs(v))[:, 0]
            assert np.all(np.abs(y - (lp.C @ v)[:, 0]) <= bound), k
            f = ha @ hx + hb @ y + lp.drift[k]
            fabs = np.abs(ha) @ np.abs(hx) + np.abs(hb) @ np.abs(y) \
                + np.abs(lp.drift[k])
            assert np.all(np.abs(gfl - f) <= KTOL*fabs), k
            hxn = hx + 1.5*dt*f - .5*dt*fl
            hxabs = np.abs(hx) + 1.5*dt*fabs + .5*dt*np.abs(fl)
            assert np.all(np.abs(ghx - hxn) <= KTOL*hxabs), k
            un = hc @ hxn
            assert np.all(np.abs(guc - un) <= KTOL*(np.abs(hc) @ hxabs)), k
            assert np.array_equal(ulog[0], guc)
            assert np.array_equal(gup, uc)          # u_p: the old u_c
            un = guc                # (the rest from the device's own u_n)
            # the Dirichlet row of the state this step leaves
            row = stp.feedback_bcs(k + 1, 1)[0]
            babs = np.abs(base) + abs(S) @ np.abs(un)
            assert np.all(np.abs(row - (base + S @ un)) <= KTOL*babs), k
            if k + 2 <= nst:        # (the next row is still the host's)
                assert np.array_equal(stp.feedback_bcs(k + 2, 1)[0], base)
            if literal and not with_b:
                with pytest.raises(Exception):      # the step reads g itself
                    stp.feedback_rhs()
            else:
                us = (un, uc, up)
                want_g, gabs = lp.gtab[k].copy(), np.abs(lp.gtab[k])
                want_p, pabs = lp.gptab[k].copy(), np.abs(lp.gptab[k])
                if lp.terms is not None:
                    Ba, Bm, Bj = lp.terms
                    for j in range(3):
                        want_g += lp.wm[j]*(Bm @ us[j]) + lp.wa[j]*(Ba @ us[j])
                        gabs += abs(lp.wm[j])*(abs(Bm) @ np.abs(us[j])) \
                            + abs(lp.wa[j])*(abs(Ba) @ np.abs(us[j]))
                    want_p += Bj @ un
                    pabs += abs(Bj) @ np.abs(un)
                if with_b:
                    want_g += dt*.5*(lp.B @ un + lp.B @ uc)
                    gabs += dt*.5*(abs(lp.B) @ (np.abs(un) + np.abs(uc)))
                geff, gpeff = stp.feedback_rhs(pressure=lp.terms is not None)
                assert np.all(np.abs(geff - want_g) <= KTOL*gabs), k
                if lp.terms is not None:
                    assert np.all(np.abs(gpeff - want_p) <= KTOL*pabs), k
            hx, fl, uc, up = ghx, gfl, guc, gup
            v = stp.get_state()[0]
        # row 0 keeps the host's bits
        rows = stp.feedback_bcs(0, nst + 1)
        assert np.array_equal(rows[0], lp.tab[0, nstat:])
        assert stp.table_position() == (nst, 0)
        with pytest.raises(Exception):              # the tables are used up
            lp.run(1)
    finally:
        lp.close()


@pytest.mark.parametrize('hN,Nu', [(1, 2), (13, 2), (128, 2)])
def test_bc_observer_step_has_the_plain_kernels_bits(gtiu, toy_prob, hN, Nu):
    """`k_lti_bc_step` and `k_lti_step` share one observer step: two steppers
    on one system, the same state, tables, sensors, observer and drift; the
    boundary mode literal, without `B`, with an `S` of zeros (every Dirichlet
    row it writes is `base`), the plain mode with an empty `B` and the same
    constant Dirichlet table.  Four steps, one `run(1)` each: `y`, `u`, `hx`,
    `f_last`, `u_c` are the same bits, `u_p` is the `u_c` of the step before.
    (hN = 1: one half of `ha hx` is empty; 13: odd, staged in LDS; 128: read
    in place, the slots 258 and 260 entries long)

    The velocities of the two loops are NOT bit equal throughout -- measured
    on the MI355X, before the two kernels shared their code as after: equal
    after the steps 0, 1, 2, different after step 3 in all three cases (why
    is not established: the one loop's steps read `g` from the table row, the
    other's the same values from `geff`).  So the observer quantities of the
    first step are
    always compared (`v` is the same by construction), those of a later step
    only while the `v` it read was bit equal; nothing is compared within a
    tolerance."""
    from dolfin_navier_scipy_amd import saddle
    bc = ToyBcLoop(toy_prob, hN=hN, Nu=Nu, literal=True, nst=4, setup=False)
    bc.S = sps.csr_matrix((np.zeros(bc.S.nnz), bc.S.indices, bc.S.indptr),
                          shape=bc.S.shape)
    M, A = (toy_prob['smc'][k] for k in 'MA')
    stp = saddle.ImexStepper(bc.system, (M - .5*bc.dt*A).tocsr())
    cvop, _ = bs.toy_cvop(toy_prob)
    try:
        obs = bc.obs
        assert bc.B.nnz == 0 and bc.terms is None and obs['hb'].shape[1] == 3
        stp.set_state(bc.stp.get_state()[0])
        stp.set_convection(cvop, scale=-1.0)
        bc.arm()
        stp.set_feedback(bc.C, sps.csr_matrix((bc.NV, Nu)), obs['ha'],
                         obs['hb'], obs['hc'], c_n=.5, c_c=.5, dt=bc.dt)
        stp.set_feedback_state(bc.hx, bc.fl, bc.uc)
        stp.set_rhs_table(bc.gtab, bc.gptab)
        assert np.array_equal(bc.tab[0], bc.tab[1])
        cvop.set_dbc_table(bc.tab)
        stp.set_feedback_table(bc.nst, bc.drift)
        uc, same_v = bc.uc, True
        for k in range(bc.nst):
            bc.run(1)
            stp.run(1, bc.cf, bc.opts)
            ghx, gfl, guc, gup = bc.stp.feedback_state_bc()
            assert np.array_equal(gup, uc), k
            uc = guc
            assert np.array_equal(bc.stp.feedback_bcs(k + 1, 1)[0], bc.base)
            if not same_v:
                continue
            for a, b in zip(bc.stp.feedback_log(k, 1), stp.feedback_log(k, 1)):
                assert np.array_equal(a, b), k
            for a, b in zip((ghx, gfl, guc), stp.feedback_state()):
                assert np.array_equal(a, b), k
            same_v = np.array_equal(bc.stp.get_state()[0], stp.get_state()[0])
            print(hN, 'step', k, 'observer bit equal; v after it:', same_v)
        assert np.abs(uc).max() > 0
    finally:
        stp.close()
        cvop.close()
        bc.close()


# ---- 2. zero gain ---------------------------------------------------------------

@pytest.mark.parametrize('scheme,literal', [('cnab', False), ('sbdf2', False),
                                            ('cnab', True)])
def test_zero_gain_equals_the_time_only_loop(gtiu, toy_prob, scheme, literal):
    """`hc = 0`: the closed loop IS the `bcs_time_only` run with the constant
    values `base`, bit for bit -- nothing but +0 is added anywhere"""
    a = run_resident(gtiu, toy_prob, scheme, literal=literal, zero_gain=True)
    assert a['last']['feedback'] == 'resident-boundary'
    assert a['fb'].calls['abtwo'] == 0
    assert not np.any(a['last']['feedback_u'])
    assert np.any(a['last']['feedback_y'])
    base = a['fb'].base.tolist()
    b = run_resident(gtiu, toy_prob, scheme, literal=literal,
                     getbcs=lambda t, v, p, mode=None: list(base),
                     resident=dict(bcs_time_only=True))
    assert b['last']['feedback'] is None
    assert a['t'].size == 13
    assert np.array_equal(a['v'], b['v'])
    assert np.array_equal(a['p'], b['p'])
    assert np.array_equal(a['vend'], b['vend'])
    assert np.array_equal(a['pend'], b['pend'])


# ---- 3. / 4. the logged inputs, replayed open loop --------------------------------

def _replay(gtiu, prob, scheme, literal, a):
    """`bcs_time_only` with control functions that return the `u` of the
    closed-loop run `a` by step (the Heun start: by mode), `gain * sv` per
    dof as `solve_nse` forms the values"""
    fb, trange = a['fb'], a['kw']['trange']
    S = fb.s_mat.tocsc()
    shapes = [S[:, k].toarray()[:, 0] for k in range(fb.Nu)]
    owner = S.tocsr().indices                       # one control per dof
    assert owner.size == S.shape[0]
    heun = {h[1]: h[3] for h in fb.history}
    ulog = a['last']['feedback_u']

    def getbcs(time, vvec, pvec, mode=None):
        step = int(np.argmin(np.abs(trange - time)))
        u = heun[mode] if step < 2 else ulog[step - 2]
        return [float(u[owner[i]])*shapes[owner[i]][i]
                for i in range(owner.size)]
    return run_resident(gtiu, prob, scheme, literal=literal, getbcs=getbcs,
                        resident=dict(bcs_time_only=True))


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_literal_mode_replay_is_bit_equal(gtiu, toy_prob, scheme):
    """`base = 0`, one control per dof, the literal `applybcs`: the control
    reaches the flow through `S u` against `gain * sv` only, one product
    each -- `v`, `p` of every saved step are the same bits"""
    a = run_resident(gtiu, toy_prob, scheme, literal=True, Nu=2, base=False,
                     gain=2.)
    assert a['last']['feedback'] == 'resident-boundary'
    assert np.abs(a['last']['feedback_u']).max() > 1e-3
    b = _replay(gtiu, toy_prob, scheme, True, a)
    assert np.array_equal(a['v'], b['v'])
    assert np.array_equal(a['p'], b['p'])


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_nonliteral_replay_within_the_parity_tolerances(gtiu, toy_prob,
                                                        scheme):
    """the same with `applybcs` writing the values: the device adds `(wm_j Bm
    + wa_j Ba) u_j` and `Bj u_n` to rows tabulated for `u = 0`, the replay
    tabulates `applybcs(b)`.  Measured on the MI355X (worst saved step):
    see profiles/r17_boundary_feedback/README.md"""
    a = run_resident(gtiu, toy_prob, scheme, literal=False, Nu=2, base=False,
                     gain=2.)
    b = _replay(gtiu, toy_prob, scheme, False, a)
    ev, ep = _state_distance(toy_prob, a, b)
    print(scheme, 'non-literal replay: v', ev, 'p', ep)
    assert ev <= VTOL and ep <= PTOL
    # ... and the boundary terms do matter: the literal run ends elsewhere
    c = run_resident(gtiu, toy_prob, scheme, literal=True, Nu=2, base=False,
                     gain=2.)
    assert _state_distance(toy_prob, c, a)[0] > 1e-6


# ---- 5. resident against the host path and the oracle -------------------------------

@pytest.mark.parametrize('scheme,Nu,hN,literal', [
    ('cnab', 1, 12, False), ('sbdf2', 2, 12, False), ('cnab', 2, 1, True),
    ('sbdf2', 1, 128, True)])
def test_resident_against_host_path_and_oracle(gtiu, toy_prob, scheme, Nu, hN,
                                               literal):
    fbkw = dict(literal=literal, Nu=Nu, hN=hN)
    a = run_resident(gtiu, toy_prob, scheme, **fbkw)
    assert a['last']['feedback'] == 'resident-boundary'
    assert a['fb'].calls == dict(init=1, heunpred=1, heuncorr=1, abtwo=0)
    runs = {}
    for name, mod in (('host', gtiu), ('oracle', imex_oracle)):
        kw, rec, fb = bs.build(gtiu, toy_prob, **fbkw)
        v, p, ff = _integ(mod, scheme)(**kw)
        assert ff == 0 and fb.calls['abtwo'] == 11
        t, vs, ps = rec.arrays()
        runs[name] = dict(t=t, v=vs, p=ps, fb=fb)
        if name == 'host':
            assert gtiu.LAST_RUN['feedback'] == 'host'
            assert gtiu.LAST_RUN['run_calls'] == 0
    _, _, cntinds, _ = bs.split(toy_prob)
    for name, b in runs.items():
        ev, ep = _state_distance(toy_prob, a, b)
        rows = [h for h in b['fb'].history if h[1] == 'abtwo']
        yb, ub = (np.array([h[k] for h in rows]) for k in (2, 3))
        ey = _rel(a['last']['feedback_y'], yb)
        eu = _rel(a['last']['feedback_u'], ub)
        mem_a, mem_b = a['fb'].memory, b['fb'].memory
        em = max(_rel(mem_a[k], mem_b[k]) for k in ('lasthx', 'lastrhs'))
        print(scheme, Nu, hN, literal, 'resident vs', name, ': v', ev, 'p',
              ep, 'y', ey, 'u', eu, 'memory', em)
        assert ev <= VTOL and ep <= PTOL
        assert ey <= 1e-8 and eu <= 1e-8 and em <= 1e-8
        assert abs(mem_a['lastt'] - mem_b['lastt']) <= 1e-14
        assert abs(mem_a['lastdt'] - mem_b['lastdt']) <= 1e-14
        # the boundary values the saved states carry
        eb = _rel(a['v'][:, cntinds], b['v'][:, cntinds])
        assert eb <= 1e-8, eb
    # ... which are the device's table: base + S u of the logged inputs
    want = a['fb'].base + a['last']['feedback_u'] @ a['fb'].s_mat.T.toarray()
    assert np.allclose(a['last']['feedback_bcs'], want, rtol=1e-13, atol=0)
    assert np.array_equal(a['v'][2:, cntinds], a['last']['feedback_bcs'])


# ---- 6. / 7. slices, batches, determinism --------------------------------------------

def test_one_slice_three_slices_and_the_same_call_twice(gtiu, toy_prob):
    """13 loop steps as one slice and as three agree within 1e-8; the same
    call twice gives the same bits: states, logs, table"""
    # (the device writes the states down: ONE `run` per slice)
    kwb = dict(Nts=14, tE=0.07, Nu=2, resident=dict(record=True))
    one = run_resident(gtiu, toy_prob, 'cnab', ntimeslices=1, **kwb)
    three = run_resident(gtiu, toy_prob, 'cnab', ntimeslices=3, **kwb)
    again = run_resident(gtiu, toy_prob, 'cnab', ntimeslices=3, **kwb)
    assert one['last']['feedback_u'].shape == (13, 2)
    nsl = [sum(1 for c in gtiu._inittimegrid(one['kw']['trange'], n)[1] if c)
           for n in (1, 3)]
    assert [one['last']['run_calls'], three['last']['run_calls']] == nsl
    assert nsl[0] == 1 and nsl[1] >= 3
    ev, ep = _state_distance(toy_prob, one, three)
    print('one slice vs three: v', ev, 'p', ep)
    assert ev <= 1e-8 and ep <= 1e-8
    for key in ('feedback_y', 'feedback_u', 'feedback_bcs'):
        assert _rel(one['last'][key], three['last'][key]) <= 1e-8
        assert np.array_equal(three['last'][key], again['last'][key])
    assert np.array_equal(three['v'], again['v'])
    assert np.array_equal(three['p'], again['p'])
    for k in ('lasthx', 'lastrhs'):
        assert np.array_equal(three['fb'].memory[k], again['fb'].memory[k])


def test_a_batch_against_single_steps(gtiu, toy_prob):
    """24 steps as ONE `run(24)` (twice) and as 24 `run(1)`: states, logs,
    observer state and table within 1e-8; the two batched runs bit equal"""
    runs = []
    for mode in ('batched', 'batched', 'single'):
        lp = ToyBcLoop(toy_prob, Nu=2, weights='sbdf2', with_b=True, nst=24)
        try:
            if mode == 'batched':
                lp.run(24)
            else:
                for _ in range(24):
                    lp.run(1)
            v, p = lp.stp.get_state()
            y, u = lp.stp.feedback_log()
            runs.append(dict(v=v, p=p, y=y, u=u, b=lp.stp.feedback_bcs(),
                             state=lp.stp.feedback_state_bc(),
                             unconverged=lp.stp.last_run['unconverged']))
        finally:
            lp.close()
    a, a2, b = runs
    assert a['unconverged'] == 0 and a['b'].shape[0] == 25
    ev = fs.mnorm(lp.M, a['v'] - b['v'])/fs.mnorm(lp.M, b['v'])
    ep = np.linalg.norm(a['p'] - b['p'])/np.linalg.norm(b['p'])
    print('batch vs single steps: v', ev, 'p', ep)
    assert ev <= 1e-8 and ep <= 1e-8
    for key in ('y', 'u', 'b'):
        assert _rel(a[key], b[key]) <= 1e-8
        assert np.array_equal(a[key], a2[key])
    for x, y, z in zip(a['state'], b['state'], a2['state']):
        assert _rel(x, y) <= 1e-8
        assert np.array_equal(x, z)
    assert np.array_equal(a['v'], a2['v']) and np.array_equal(a['p'], a2['p'])


# ---- 8. solve_nse ---------------------------------------------------------------------

def _nse_setup(gtiu, prob, funcs='fb'):
    from dolfin_navier_scipy_amd.fem import condense_sysmatsbybcs
    th, stms = prob['th'], prob['stms']
    statinds, statvals, cntinds, cntvals = bs.split(prob)
    smc, rhs, inv = condense_sysmatsbybcs(stms, statinds, statvals)
    obs = fs.observer(6, 3, 1, gain=2.)
    fb = gtiu.BoundaryFeedback(bs.full_sensors(prob), None, obs['ha'],
                               obs['hb'], obs['hc'], obs['inihx'],
                               drift=fs.drift_of(obs['dvec']))
    u0 = float((obs['hc'] @ obs['inihx'])[0, 0])
    rng = np.random.default_rng(6)
    full0 = np.zeros((th.vdim, 1))
    full0[0::2, 0] = u0
    full0[prob['invinds'], 0] += 1e-2*rng.standard_normal(
        prob['invinds'].size)
    full0[statinds, 0] = statvals
    full0[cntinds, 0] = cntvals*u0

    def plain(t, vel=None, p=None, mode=None, memory=None):
        y = 0. if vel is None else float(np.mean(vel[prob['invinds']]))
        return u0*(1. + 1e-2*y), memory
    kw = dict(A=smc['A'], M=smc['M'], J=smc['J'], fv=rhs['fv'], fp=rhs['fp'],
              iniv=full0, inip=np.zeros((smc['J'].shape[0], 1)),
              trange=np.linspace(0, 0.06, 13), V=th, invinds=inv,
              dbcinds=statinds.tolist(), dbcvals=statvals.tolist(),
              diricontbcinds=[cntinds.tolist()],
              diricontbcvals=[cntvals.tolist()],
              diricontfuncs=dict(fb=fb, controls=fb.controls(),
                                 plain=[plain])[funcs],
              diricontfuncmems=[None], treat_nonl_explicit=True,
              return_dictofvelstrs=True)
    return kw, fb, cntinds, cntvals


@pytest.mark.parametrize('funcs', ['fb', 'controls'])
def test_solve_nse_runs_the_feedback_resident(gtiu, toy_prob, funcs):
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    kw, fb, cntinds, cntvals = _nse_setup(gtiu, toy_prob, funcs)
    vels = snu.solve_nse(record_on_device=True, **kw)
    last = gtiu.LAST_RUN
    assert last['feedback'] == 'resident-boundary'
    assert last['record'] == 'device'
    nslices = sum(1 for c in gtiu._inittimegrid(kw['trange'], 10)[1] if c)
    assert last['run_calls'] == nslices == 11
    assert fb.calls == dict(init=1, heunpred=1, heuncorr=1, abtwo=0)
    # the returned velocities carry base + S u (here: u times the profile)
    heun = {h[1]: h[3] for h in fb.history}
    us = [heun['init'], heun['heuncorr']] + list(last['feedback_u'])
    assert len(vels) == len(us) == 13
    for t, u in zip(kw['trange'], us):
        assert np.array_equal(vels[t][cntinds, 0], float(u[0])*cntvals), t
    assert np.ptp([float(u[0]) for u in us]) > 1e-4      # and they move


def test_solve_nse_other_functions_and_functionals(gtiu, toy_prob):
    """a plain state-dependent control function keeps the per-step host path;
    `functionals=` beside the feedback is refused by name"""
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    kw, _, _, _ = _nse_setup(gtiu, toy_prob, 'plain')
    snu.solve_nse(**kw)
    assert gtiu.LAST_RUN['feedback'] is None
    assert gtiu.LAST_RUN['run_calls'] == 0
    kw, _, _, _ = _nse_setup(gtiu, toy_prob, 'fb')
    with pytest.raises(ValueError) as exc:
        snu.solve_nse(functionals=object(), **kw)
    assert '`functionals`' in str(exc.value)
    assert 'BoundaryFeedback' in str(exc.value)


# ---- 9. limits and refusals ---------------------------------------------------------------

def test_limits_and_refusals_are_loud(gtiu, toy_prob):
    from dolfin_navier_scipy_amd import _capi
    lp = ToyBcLoop(toy_prob, nst=6, setup=False)
    ref = ToyBcLoop(toy_prob, nst=6)
    try:
        stp, obs, NV = lp.stp, lp.obs, lp.NV
        # the limits are k_lti_step's
        big = fs.observer(1, 3, 1, hN=129)
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_feedback(lp.C, lp.B, big['ha'], big['hb'], big['hc'],
                             c_n=.5, c_c=.5, dt=lp.dt)
        assert 'hN = 129' in str(exc.value)
        wide = fs.observer(1, 3, 33)
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_feedback(lp.C, sps.csr_matrix((NV, 33)), wide['ha'],
                             wide['hb'], wide['hc'], c_n=.5, c_c=.5, dt=lp.dt)
        assert 'Nu = 33' in str(exc.value)
        # no feedback set
        stp._fb_shape = (12, 3, 1)
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_feedback_boundary(lp.S, lp.base, col0=len(lp.statvals))
        assert exc.value.status == _capi.DNS_ERR_NOT_READY
        # widths: columns past the operator's Dirichlet values, S against Nu
        stp.set_feedback(lp.C, lp.B, obs['ha'], obs['hb'], obs['hc'], c_n=.5,
                         c_c=.5, dt=lp.dt)
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_feedback_boundary(lp.S, lp.base,
                                      col0=len(lp.statvals) + 1)
        assert 'do not fit' in str(exc.value)
        with pytest.raises(ValueError):
            stp.set_feedback_boundary(sps.csr_matrix((lp.base.size, 2)))
        Ba, Bm, Bj = lp.terms
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_feedback_boundary(lp.S, lp.base, col0=len(lp.statvals),
                                      Ba=Ba, Bm=Bm, Bj=Bm)
        assert 'Bj must be' in str(exc.value)
        # no device convection
        stp.set_convection(None)
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_feedback_boundary(lp.S, lp.base, col0=len(lp.statvals))
        assert 'convection' in str(exc.value)
        stp.set_convection(lp.cvop, scale=-1.0)
        # a table with too few rows: the step refuses, by name
        lp.arm(table_rows=lp.nst)
        with pytest.raises(_capi.DnsError) as exc:
            lp.run(1)
        assert 'Dirichlet table has 6 rows' in str(exc.value)
        # ... and the handle is still good: the same steps as an untouched one
        # (the refused step has not run: its warm start may differ)
        lp.stp.set_state(ref.stp.get_state()[0])
        lp.arm()
        lp.run(6)
        ref.run(6)
        assert _rel(stp.get_state()[0], ref.stp.get_state()[0]) <= 1e-8
        assert _rel(stp.feedback_bcs(), ref.stp.feedback_bcs()) <= 1e-8
    finally:
        lp.close()
        ref.close()


def test_a_refused_boundary_leaves_the_plain_feedback_working(gtiu, toy_prob):
    """`dns_imex_set_feedback_boundary` refuses an `S` of the wrong width and
    `Ba` without `Bm` (both past the wrapper's own checks): the feedback stays
    as `set_feedback` left it -- the state that was set, and a step that runs"""
    from dolfin_navier_scipy_amd import _capi
    lp = ToyBcLoop(toy_prob, Nu=2, nst=2, with_b=True, setup=False)
    try:
        stp, obs = lp.stp, lp.obs
        stp.set_feedback(lp.C, lp.B, obs['ha'], obs['hb'], obs['hc'], c_n=.5,
                         c_c=.5, dt=lp.dt)
        stp.set_feedback_state(lp.hx, lp.fl, lp.uc)
        shape, col0 = stp._fb_shape, len(lp.statvals)
        stp._fb_shape = shape[:2] + (3,)            # (the wrapper lets it by)
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_feedback_boundary(bs.shape_matrix(lp.base, 3), lp.base,
                                      col0=col0)
        stp._fb_shape = shape
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        assert 'S must be nc x Nu' in str(exc.value)
        Ba = lp.terms[0]
        sview, aview = _capi.CsrView(lp.S), _capi.CsrView(Ba)
        w = _capi.as_f64((0., 0., 0.), 3)
        with pytest.raises(_capi.DnsError) as exc:
            _capi.check(stp.lib.dns_imex_set_feedback_boundary(
                stp._h, sview.byref(), _capi.dptr(lp.base), col0,
                aview.byref(), None, None, _capi.dptr(w), _capi.dptr(w)))
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        assert 'come together' in str(exc.value)
        # still the plain feedback: no boundary mode, the state as it was set
        with pytest.raises(_capi.DnsError) as exc:
            stp.feedback_state_bc()
        assert exc.value.status == _capi.DNS_ERR_NOT_READY
        want = (lp.hx, lp.fl, lp.uc)
        assert all(np.array_equal(a, b)
                   for a, b in zip(stp.feedback_state(), want))
        stp.set_rhs_table(lp.gtab, lp.gptab)
        stp.set_feedback_table(lp.nst, lp.drift)
        assert all(np.array_equal(a, b)
                   for a, b in zip(stp.feedback_state(), want))
        lp.run(1)
        assert stp.table_position()[0] == 1
        y, u = stp.feedback_log(0, 1)
        v = lp.stp.get_state()[0]
        assert np.all(np.isfinite(y)) and np.all(np.isfinite(u))
        assert np.all(np.isfinite(v))
        assert np.array_equal(stp.feedback_state()[2], u[0])
    finally:
        lp.close()


def test_a_row_partitioned_stepper_is_refused(gtiu, toy_prob):
    from dolfin_navier_scipy_amd import saddle, _capi, comm as dcomm
    M, A, J = (toy_prob['smc'][k] for k in 'MAJ')
    dt = 5e-3
    _, _, _, cntbase = bs.split(toy_prob)
    cm = dcomm.Comm.rccl(0, 1, 0, dcomm.rccl_unique_id())
    system = saddle.SaddleSystem((M + .5*dt*A).tocsr(), J)
    stp = None
    try:
        system.set_comm(cm)
        system.setup_precond(cheb_degree=6, schur='dense', fhat='explicit')
        stp = saddle.ImexStepper(system, (M - .5*dt*A).tocsr())
        stp._fb_shape = (12, 3, 1)
        with pytest.raises(_capi.DnsError) as exc:
            stp.set_feedback_boundary(bs.shape_matrix(cntbase, 1), cntbase)
        assert 'boundary feedback on a row-partitioned stepper' in \
            str(exc.value)
    finally:
        if stp is not None:
            stp.close()
        system.set_comm(None)
        system.close()
        cm.close()
