"""Device-resident force functionals with time-varying Dirichlet values (the
moving-boundary instance of `k_functional_step`, `dns_imex_set_functionals_bc`,
`ImexStepper.set_functionals(..., dbc_table=)`, `resident=dict(functionals=)`
of `cnab` / `sbdftwo` with controlled boundaries, `solve_nse(diricontfuncs=,
functionals=)`): every row of the device's log against the NumPy statement
`fem.MomentumFunctionals.evaluate(..., dbc=, dbc_prev=)` on the states the
recorder wrote down in the same run.

Shapes: `scenarios.toy_problem()` (NV = 1286, NP = 207, 348 cells, 240
Dirichlet dofs).  Rotating obstacle: its 15 nodes (30 dofs) carry `g(t) =
omega(t) (-(y - yc), x - xc)`, the other 210 Dirichlet dofs are static; `fx`,
`fy` and the torque list 28 cells each -- 84 listed cells, three passes of 32,
the last one partial and no multiple of 8 wide --, the inflow bump 44 more.

Tolerance `1e-11 * T_k`, `T_k` the sum of the absolute values of every product
of functional k, those of `cab` and `cmb` included: the bound of
`tests/test_gpu_functionals.py` (a few thousand fp64 products, 20x the
rounding estimate) carries over, because `T_k` counts the new products too.
"""
import numpy as np
import pytest
import scipy.sparse as sps

import scenarios
from test_functionals_bc_cpu import (CENTER, bump, moving_femp, rotating_split,
                                     rotation)

pytestmark = pytest.mark.gpu

TOL = 1e-11
DT = 1./512


def omega(t):
    return 1. + 2.*np.sin(40.*t)


@pytest.fixture(scope='module')
def gtiu():
    from dolfin_navier_scipy_amd import time_int_utils, _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    return time_int_utils


@pytest.fixture(scope='module')
def rot(gtiu, toy_prob):
    """the toy problem with the obstacle's dofs controlled (a rotation)"""
    from dolfin_navier_scipy_amd import fem
    prob, th = toy_prob, toy_prob['th']
    statinds, statvals, cntinds, nodes = rotating_split(prob)
    femp = moving_femp(prob, statinds, cntinds, statvals,
                       np.zeros(cntinds.size))
    inv = np.asarray(prob['invinds'])
    smc = prob['smc']
    M, A, J = smc['M'].tocsr(), smc['A'].tocsr(), smc['J'].tocsr()
    NP, NV = J.shape
    assert (NV, NP, th.mesh.ncells) == (1286, 207, 348)
    rng = np.random.default_rng(3)
    row = sps.random(1, NV, density=100./NV, format='csr', random_state=rng)
    fn = (fem.boundary_forces(th, femp, nodes=nodes)
          + fem.boundary_torque(th, femp, nodes=nodes, center=CENTER)
          + fem.pressure_difference(th, (0.15, 0.2), (0.3, 0.2))
          + fem.MomentumFunctionals.from_rows(th, femp, ca=row, c0=[0.3],
                                              scale=[0.7], names=['row'])
          + fem.MomentumFunctionals(th, femp,
                                    bump(th, 0.3, (0., 0.2)).reshape((-1, 1)),
                                    names=['bump']))
    assert [c.size for c in fn.cells] == [28, 28, 28, 0, 0, 44]
    stms = prob['stms']
    aux0 = np.zeros((th.vdim, 1))
    aux0[statinds, 0] = statvals
    cfv = -(stms['A'] @ aux0)[inv, :]
    cfp = -(stms['J'] @ aux0)

    def gvals(t):                      # the controlled values at time t
        return rotation(th, nodes, omega(t))

    def applybcs(bcs_n):
        caux = np.zeros((th.vdim, 1))
        caux[cntinds, 0] = bcs_n
        return (-(stms['A'] @ caux)[inv, :], -(stms['J'] @ caux),
                (stms['M'] @ caux)[inv, :])

    def appndbcs(vvec, bcs):
        full = np.full((th.vdim, 1), np.nan)
        full[inv] = vvec
        full[statinds, 0] = statvals
        full[cntinds, 0] = bcs
        return full
    xy = th.nodecoords
    ufull = np.zeros((th.vdim, 1))
    ufull[0::2, 0] = 4*xy[:, 1]*(0.41 - xy[:, 1])/0.41**2
    v0 = ufull[inv] + 1e-2*rng.standard_normal((NV, 1))
    return dict(prob=prob, th=th, fn=fn, femp=femp, inv=inv, M=M, A=A, J=J,
                NV=NV, NP=NP, statinds=statinds, statvals=statvals,
                cntinds=cntinds, nodes=nodes, dbi=femp['dbcinds'], cfv=cfv,
                cfp=cfp, gvals=gvals, applybcs=applybcs, appndbcs=appndbcs,
                v0=v0, touched=[0, 1, 2, 5])


def _table(c, nst, t0=0., amp=1.):
    """`(nst + 1, 240)`: the Dirichlet values at `t0 + j dt`"""
    return np.array([np.concatenate([c['statvals'],
                                     amp*c['gvals'](t0 + j*DT)])
                     for j in range(nst + 1)])


class Loop(object):
    """CNAB / SBDF2 on the toy problem with the rotating obstacle: rhs table,
    Dirichlet table of the convection operator, recorder, functionals"""

    def __init__(self, c, scheme='cnab', use_graph=True):
        from dolfin_navier_scipy_amd import saddle, convection
        M, A, J = c['M'], c['A'], c['J']
        dt = self.dt = DT
        self.c, self.scheme = c, scheme
        self.cvop = convection.ConvectionP2.from_taylor_hood(
            c['th'], c['inv'], c['dbi'], c['femp']['dbcvals'])
        if scheme == 'cnab':
            F, R1 = M + .5*dt*A, M - .5*dt*A
            self.cf = saddle.ImexStepper.coeffs(
                a_c=1., cn_c=1.5*dt, cn_o=-.5*dt, pscale=-1./dt, extrapolate=4)
        else:
            F, R1 = M + 2./3*dt*A, M
            self.cf = saddle.ImexStepper.coeffs(
                a_c=4./3, a_p=-1./3, cn_c=4./3*dt, cn_o=-2./3*dt,
                pscale=-1./dt, extrapolate=4)
        self.system = saddle.SaddleSystem(F.tocsr(), J)
        self.system.setup_precond(cheb_degree=6, schur='dense', drop_tol=1e-3,
                                  factorization='full')
        self.stp = saddle.ImexStepper(self.system, R1.tocsr())
        self.cvop.set_dbcvals(_table(c, 0)[0])
        nfc = self.cvop.apply(c['v0'], scale=-1.0)
        self.stp.set_state(c['v0'], v_p=c['v0'], nfc_c=nfc, nfc_o=nfc)
        self.stp.set_convection(self.cvop, scale=-1.0)
        self.opts = saddle.solve_opts(method='gmres', rtol=1e-10, maxiter=400,
                                      restart=60, check_every=2,
                                      use_graph=use_graph, reorth=2)
        self.t = 0.

    def arm(self, fn, nst, amp=1., recorder=True, moving=True):
        """tables of the next `nst` steps; returns the functionals' table"""
        c, dt = self.c, self.dt
        tab = _table(c, nst, self.t, amp)
        nst_c = len(c['statvals'])
        terms = [c['applybcs'](tab[j][nst_c:]) for j in range(nst + 1)]
        tm1 = c['applybcs'](amp*c['gvals'](self.t - dt))
        gv, gp = np.empty((nst, c['NV'])), np.empty((nst, c['NP']))
        for s in range(nst):
            (bfv_c, _, mbc_c), (bfv_n, bfp_n, mbc_n) = terms[s], terms[s + 1]
            mbc_p = terms[s - 1][2] if s else tm1[2]
            if self.scheme == 'cnab':
                g = -(mbc_n - mbc_c) + .5*dt*(2*c['cfv'] + bfv_n + bfv_c)
            else:
                g = -(mbc_n - 4./3*mbc_c + 1./3*mbc_p) \
                    + 2./3*dt*(bfv_n + c['cfv'])
            gv[s], gp[s] = g[:, 0], (c['cfp'] + bfp_n)[:, 0]
        self.stp.set_rhs_table(gv, gp)
        self.cvop.set_dbc_table(tab[:nst])
        if recorder:
            self.stp.set_recorder(nst, snap_slots='all')
        if fn is not None:
            self.stp.set_functionals(fn, nst, dt,
                                     dbc_table=tab if moving else None)
        self.t += nst*dt
        return tab

    def recorded(self, fn, nst, how='run', amp=1.):
        """`nst` steps with recorder and functionals: `(rows, vs, ps, tab)`"""
        tab = self.arm(fn, nst, amp)
        if how == 'run':
            self.stp.run(nst, self.cf, self.opts)
        else:
            for _ in range(nst):
                self.stp.step(self.cf, opts=self.opts)
        vs, ps = self.stp.record_snapshots()
        return self.stp.get_functionals(), vs, ps, tab

    def close(self):
        self.stp.close()
        self.cvop.close()
        self.system.close()


def _check_rows(fn, rows, vs, ps, v_first, tab, dt, what):
    """every row against `.evaluate` of the recorded states and the table
    rows that belong to them; returns `(worst error / T_k, T of the rows)`"""
    assert rows.shape == (vs.shape[0], fn.nF)
    assert tab.shape[0] == rows.shape[0] + 1
    assert np.isfinite(rows).all()
    worst, Ts = np.zeros(fn.nF), []
    for r in range(rows.shape[0]):
        vprev = vs[r - 1] if r else np.asarray(v_first).reshape(-1)
        y, T = fn.evaluate(vs[r], vprev, ps[r], dt, return_scale=True,
                           dbc=tab[r + 1], dbc_prev=tab[r])
        worst = np.maximum(worst, np.abs(rows[r] - y)/T)
        Ts.append(T)
    print(what, ': worst |row - evaluate| / T per functional',
          dict(zip(fn.names, worst)))
    assert np.all(worst <= TOL), (what, worst)
    return worst, np.array(Ts)


# ---- 1. rows match the host statement, every step ----------------------------

@pytest.mark.parametrize('scheme,step6,how',
                         [('cnab', '1', 'run'), ('sbdf2', '1', 'run'),
                          ('cnab', '0', 'run'), ('cnab', '1', 'step')])
def test_rows_match_the_host_statement(gtiu, rot, monkeypatch, scheme, step6,
                                       how):
    monkeypatch.setenv('DNS_STEP6', step6)
    nst = 48 if how == 'run' else 6
    fn = rot['fn']
    lp = Loop(rot, scheme)
    try:
        rows, vs, ps, tab = lp.recorded(fn, nst, how)
        vl, pl = lp.stp.get_state()
    finally:
        lp.close()
    assert np.array_equal(vs[-1], vl[:, 0]) and np.array_equal(ps[-1], pl[:, 0])
    _, Ts = _check_rows(fn, rows, vs, ps, rot['v0'], tab, DT,
                        '{0} step6={1} {2}'.format(scheme, step6, how))
    # the boundary terms count: against the static statement where the
    # functional reaches the obstacle, and against the one without `cmb .
    # (g - g_prev)/dt` -- there without `fy`: the mesh about the obstacle is
    # symmetric in x, so the acceleration of a rotation about its centre,
    # `omega' (-(y - yc), x - xc)`, has no y-momentum and `cmb_fy . g'` is a
    # sum of rounding errors
    k, km = rot['touched'], [0, 2, 5]
    for r in range(nst):
        vprev = vs[r - 1] if r else rot['v0'][:, 0]
        ys = fn.evaluate(vs[r], vprev, ps[r], DT)
        yc = fn.evaluate(vs[r], vprev, ps[r], DT, dbc=tab[r + 1],
                         dbc_prev=tab[r + 1])
        assert np.all(np.abs(rows[r] - ys)[k] > 1e-6*Ts[r][k]), r
        assert np.all(np.abs(rows[r] - yc)[km] > 1e-6*Ts[r][km]), r


# ---- 2. edges ---------------------------------------------------------------------

def test_edges_and_refusals(gtiu, rot):
    from dolfin_navier_scipy_amd import _capi, fem
    fn, th, femp = rot['fn'], rot['th'], rot['femp']
    lp = Loop(rot)
    try:
        stp = lp.stp
        v_keep = rot['v0'][:, 0]
        # one row: a table of two
        rows, vs, ps, tab = lp.recorded(fn, 1)
        assert tab.shape == (2, 240)
        _check_rows(fn, rows, vs, ps, v_keep, tab, DT, 'nrows = 1')
        v_keep = vs[-1]
        # rows used up
        for go in (lambda: stp.run(1, lp.cf, lp.opts),
                   lambda: stp.step(lp.cf, opts=lp.opts)):
            with pytest.raises(_capi.DnsError) as exc:
                go()
            assert exc.value.status == _capi.DNS_ERR_NOT_READY
        # nF = 16, five sparse rows each: 80 rows, the grid strides; nF = 1,
        # pressure only
        dp = fem.pressure_difference(th, 3, 5)
        for few in (fn + fn + dp + dp + dp + dp, dp):
            assert few.nF in (1, 16)
            rows, vs, ps, tab = lp.recorded(few, 8)
            _check_rows(few, rows, vs, ps, v_keep, tab, DT,
                        'nF = %d' % few.nF)
            v_keep = vs[-1]
        rows, vs, ps, tab = lp.recorded(fn, 8)
        v_keep, p_keep = stp.get_state()
        # refusals leave the log and the state as they were
        wrong = np.zeros((5, 239))
        bad_cols = fn.scaled(1.)
        bad_cols.cab = sps.csr_matrix(
            (np.ones(6), (np.arange(6), np.arange(6))), shape=(6, 241))
        for go, word in (
                (lambda: stp.set_functionals(fn, 4, DT,
                                             dbc_table=np.zeros((5, 241))),
                 'cab'),
                (lambda: stp.set_functionals(dp, 4, DT,
                                             dbc_table=np.zeros((5, 0))),
                 'ndbc'),
                (lambda: stp.set_functionals(fn, 4, DT), 'Dirichlet table')):
            with pytest.raises((_capi.DnsError, ValueError)) as exc:
                go()
            if isinstance(exc.value, _capi.DnsError):
                assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
            assert word in str(exc.value), str(exc.value)
        with pytest.raises(ValueError):
            stp.set_functionals(fn, 4, DT, dbc_table=wrong[:4])   # nrows + 1
        with pytest.raises(ValueError):
            stp.set_functionals(bad_cols, 4, DT, dbc_table=np.zeros((5, 240)))
        assert np.array_equal(stp.get_functionals(), rows)
        assert np.array_equal(stp.get_state()[0], v_keep)
        assert np.array_equal(stp.get_state()[1], p_keep)
    finally:
        lp.close()


def test_the_c_boundary_checks_the_widths(gtiu, rot):
    """past the Python layer: `ndbc` that is not the operator's, `cab` with
    another number of columns, a null table -- DNS_ERR_BAD_ARGUMENT, and the
    functionals that were set stay"""
    from dolfin_navier_scipy_amd import _capi as C
    fn = rot['fn']
    lp = Loop(rot)
    try:
        stp = lp.stp
        rows, vs, ps, tab = lp.recorded(fn, 4)
        args = fn.device_args(moving=True)
        nF = fn.nF
        views = {k: C.CsrView(args[k]) for k in ('ca', 'cm', 'cp', 'cab',
                                                 'cmb')}
        narrow = C.CsrView(sps.csr_matrix((nF, 239)))
        cptr = np.ascontiguousarray(args['cell_ptr'], dtype=np.int32)
        cidx = np.ascontiguousarray(args['cell_idx'], dtype=np.int32)
        cw, c0, sc = (C.as_f64(args['cell_w']), C.as_f64(args['c0']),
                      C.as_f64(args['scale']))
        t239, t240 = np.zeros(5*239), np.zeros(5*240)

        def call(cab, cmb, ndbc, table):
            return stp.lib.dns_imex_set_functionals_bc(
                stp._h, nF, views['ca'].byref(), views['cm'].byref(),
                views['cp'].byref(), cab.byref(), cmb.byref(),
                C.dptr(c0), C.dptr(sc), cptr.ctypes.data_as(C.c_int32_p),
                cidx.ctypes.data_as(C.c_int32_p), C.dptr(cw), DT, 4, ndbc,
                C.dptr(table))
        wide = views['cab'], views['cmb']
        for cab, cmb, ndbc, table, word in (
                (wide[0], wide[1], 239, t239, 'cab'),   # cab is nF x 240
                (narrow, wide[1], 239, t239, 'cmb'),    # cmb is nF x 240
                (narrow, wide[1], 240, t240, 'cab'),
                (wide[0], wide[1], 0, t240, 'ndbc'),
                (wide[0], wide[1], 240, None, 'table'),
                # (cells are listed: the operator has 240 values)
                (narrow, narrow, 239, t239, 'convection operator')):
            assert call(cab, cmb, ndbc, table) == C.DNS_ERR_BAD_ARGUMENT
            assert word in stp.lib.dns_last_error().decode(), word
        assert np.array_equal(stp.get_functionals(), rows)
        assert call(wide[0], wide[1], 240, t240) == C.DNS_OK
    finally:
        lp.close()


def test_another_number_of_dirichlet_values_at_the_step(gtiu, rot):
    """functionals without cells set for 3 values, then an operator with 240
    attached: the step refuses"""
    from dolfin_navier_scipy_amd import _capi, fem
    lp = Loop(rot)
    try:
        stp = lp.stp
        rows3 = fem.MomentumFunctionals.from_rows(
            rot['th'], dict(rot['femp'], dbcinds=rot['dbi'][:3],
                            dbcvals=rot['femp']['dbcvals'][:3]),
            ca=sps.csr_matrix(np.ones((1, rot['NV']))))
        assert rows3.cab.shape == (1, 3)
        stp.set_convection(None)
        stp.set_functionals(rows3, 4, DT, dbc_table=np.zeros((5, 3)))
        stp.set_convection(lp.cvop, scale=-1.0)
        with pytest.raises(_capi.DnsError) as exc:
            stp.run(1, lp.cf, lp.opts)
        assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
        assert 'dns_imex_set_functionals_bc' in str(exc.value)
    finally:
        lp.close()


# ---- 3. re-arming keeps the graphs ---------------------------------------------------

def test_rearming_keeps_the_graphs(gtiu, rot):
    fn = rot['fn']
    lp = Loop(rot)
    try:
        lp.recorded(fn, 24)
        caps, out = [], []
        for amp in (1., 1.1):
            v_first = lp.stp.get_state()[0][:, 0]
            out.append(lp.recorded(fn, 24, amp=amp) + (v_first,))
            caps.append(lp.stp.last_run['captures'])
        print('captures of two equal slices:', caps)
        assert caps[1] == 0, caps
        (_, _, _, tab1, _), (rows, vs, ps, tab2, v_first) = out
        assert np.abs(tab2 - tab1).max() > 1e-3
        _check_rows(fn, rows, vs, ps, v_first, tab2, DT, 'second slice')
    finally:
        lp.close()


# ---- 4. deterministic ------------------------------------------------------------------

def test_logs_are_deterministic(gtiu, rot):
    fn = rot['fn']
    out = []
    for use_graph in (True, True, False):
        lp = Loop(rot, use_graph=use_graph)
        try:
            out.append(lp.recorded(fn, 32))
        finally:
            lp.close()
    (r0, v0, p0, tab), (r1, v1, p1, _), (r2, v2, p2, _) = out
    assert np.array_equal(v0, v1) and np.array_equal(p0, p1)
    assert np.array_equal(r0, r1)
    same = [r for r in range(32)
            if np.array_equal(v0[r], v2[r]) and np.array_equal(p0[r], p2[r])
            and (r == 0 or np.array_equal(v0[r - 1], v2[r - 1]))]
    print('graph vs plain launches: states identical in', len(same), 'of 32')
    assert np.array_equal(r0[same], r2[same])
    _check_rows(fn, r2, v2, p2, rot['v0'], tab, DT, 'plain launches')


# ---- 5. a restored batch -----------------------------------------------------------------

def test_a_restored_batch_takes_the_rows_of_the_restored_counter(gtiu):
    """the recipe of `test_gpu_functionals.py::test_a_restored_batch_
    overwrites_its_own_rows` (N = 2, the tabulated forcing jumps at step 128,
    the batch around it is restored and repeated) with a rotation table on the
    cylinder's dofs: the repeated batch writes its rows again, with the table
    rows the restored counter selects"""
    from dolfin_navier_scipy_amd import fem
    from test_gpu_feedback import WakeLoop, wake_setup
    wake = wake_setup()
    femp = wake['femp']
    th = femp['V']
    nodes = fem.cylinder_nodes(th)
    fn = fem.boundary_forces(th, femp) + fem.boundary_torque(th, femp) \
        + fem.pressure_difference(th, (0.15, 0.2), (0.25, 0.2))
    assert fn.cells[0].size == 62
    dbi = np.asarray(femp['dbcinds'], dtype=np.int64)
    pos = {int(d): k for k, d in enumerate(dbi)}
    cyl = np.array([[pos[2*n], pos[2*n + 1]] for n in nodes]).reshape(-1)
    nst, dt = 256, 1./512
    tab = np.tile(np.asarray(femp['dbcvals'], dtype=np.float64), (nst + 1, 1))
    for j in range(nst + 1):
        tab[j, cyl] = rotation(th, nodes, 0.5*omega(j*dt))
    lp = WakeLoop(wake, nst, feedback=False)
    try:
        lp.cvop.set_dbc_table(tab[:nst])
        lp.stp.set_recorder(nst, snap_slots='all')
        lp.stp.set_functionals(fn, nst, dt, dbc_table=tab)
        lp.run(nst)
        vs, ps = lp.stp.record_snapshots()
        rows = lp.stp.get_functionals()
        record = dict(lp.record)
    finally:
        lp.close()
    print('recorded run:', record)
    assert record['unconverged'] == 0
    assert record['replayed'] > 0, record
    _check_rows(fn, rows, vs, ps, wake['inivel'], tab, dt, 'restored batch')


# ---- 6. through the drop-ins ---------------------------------------------------------------

def _loop_kw(c, rec, nts=32):
    th, inv = c['th'], c['inv']

    def f_vdp(vf):
        return -th.convection_vec(vf)[inv, :]
    trange = np.linspace(0, nts*DT, nts + 1)
    return dict(trange=trange, inivel=c['v0'], inip=np.zeros((c['NP'], 1)),
                bcs_ini=c['gvals'](0.).tolist(), M=c['M'], A=c['A'], J=c['J'],
                f_vdp=f_vdp, f_tdp=lambda t: c['cfv'],
                g_tdp=lambda t: c['cfp'], scalep=-1.,
                getbcs=lambda t, v, p, mode=None: c['gvals'](t).tolist(),
                applybcs=c['applybcs'], appndbcs=c['appndbcs'], savevp=rec,
                check_ff_maxv=1e8, verbose=False, ntimeslices=3)


@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_through_the_time_loops(gtiu, rot, scheme):
    from dolfin_navier_scipy_amd import convection
    fn, inv, dbi = rot['fn'], rot['inv'], rot['dbi']
    integ = gtiu.cnab if scheme == 'cnab' else gtiu.sbdftwo
    got = {}
    for mode in ('plain', 'record', 'host'):
        rec = scenarios.Recorder()
        kw = _loop_kw(rot, rec)
        resident = dict(functionals=fn,
                        static_dbcvals=rot['statvals'].tolist())
        cvop = None
        if mode != 'host':
            kw.pop('f_vdp')
            cvop = convection.ConvectionP2.from_taylor_hood(
                rot['th'], inv, dbi, rot['femp']['dbcvals'])
            kw.update(device_convection=cvop, invinds=inv)
            resident.update(bcs_time_only=True,
                            savevp_times=() if mode == 'plain' else None,
                            record=(mode == 'record'))
        try:
            v, p, ff = integ(resident=resident, **kw)
        finally:
            if cvop is not None:
                cvop.close()
        assert ff == 0
        lr = dict(gtiu.LAST_RUN)
        assert lr['functionals'].shape == (31, 6)
        assert np.allclose(lr['functionals_t'], kw['trange'][2:], rtol=0,
                           atol=1e-15)
        assert lr['functionals_names'] == fn.names
        got[mode] = (lr, rec.arrays(), v, p)
    calls = dict(record=4, plain=4 if scheme == 'cnab' else 7)
    for mode in ('plain', 'record'):
        assert got[mode][0]['functionals_on'] == 'device'
        assert got[mode][0]['run_calls'] == calls[mode], \
            (mode, got[mode][0]['run_calls'])
    assert got['host'][0]['functionals_on'] == 'host'
    assert got['host'][0]['run_calls'] == 0
    # the rows are the functionals of the states `savevp` saw, with the
    # boundary values it was handed
    for mode in ('record', 'host'):
        lr, (times, vels, prss), _, _ = got[mode]
        assert times.size == 33
        vs = np.array([vf[inv] for vf in vels[2:]])
        tab = np.array([vf[dbi] for vf in vels[1:]])
        assert np.abs(np.diff(tab, axis=0)).max() > 1e-3
        _check_rows(fn, lr['functionals'], vs, np.array(prss[2:]),
                    vels[1][inv], tab, DT, scheme + ' ' + mode)
    if np.array_equal(got['plain'][2], got['record'][2]):
        assert np.array_equal(got['plain'][0]['functionals'],
                              got['record'][0]['functionals'])
    last = got['plain'][0]['functionals'][-1]
    ref = got['record'][0]['functionals'][-1]
    assert np.abs(last - ref).max() <= 1e-6*np.abs(ref).max()
    # functionals built for other Dirichlet dofs are refused
    from dolfin_navier_scipy_amd import fem
    short = fem.boundary_forces(
        rot['th'], dict(rot['femp'], dbcinds=dbi[:-2],
                        dbcvals=rot['femp']['dbcvals'][:-2]),
        nodes=rot['nodes'][:3])
    with pytest.raises(ValueError):
        integ(resident=dict(functionals=short,
                            static_dbcvals=rot['statvals'].tolist()),
              **_loop_kw(rot, scenarios.Recorder()))


# ---- 7. through solve_nse ---------------------------------------------------------------------

def test_through_solve_nse(gtiu, toy_prob):
    from dolfin_navier_scipy_amd import fem
    from dolfin_navier_scipy_amd import stokes_navier_utils as snu
    from test_gpu_snu import _controlled_setup
    prob, th = toy_prob, toy_prob['th']
    skw = _controlled_setup(prob, amplitude=0.3)()
    statinds = np.asarray(skw['dbcinds'], dtype=np.int64)
    cntinds = np.asarray(skw['diricontbcinds'][0], dtype=np.int64)
    assert cntinds.size == 15
    inner = np.setdiff1d(skw['invinds'], cntinds)
    dbi = np.concatenate([statinds, cntinds])
    femp = dict(invinds=inner, nu=prob['nu'], dbcinds=dbi,
                dbcvals=np.concatenate([skw['dbcvals'],
                                        np.zeros(cntinds.size)]))
    fn = fem.MomentumFunctionals(th, femp,
                                 bump(th, 0.3, (0., 0.2)).reshape((-1, 1)),
                                 names=['bump']) \
        + fem.pressure_difference(th, (0.15, 0.2), (0.3, 0.2))
    # the bump touches all 15 controlled dofs
    assert np.all(np.abs(fn.cab[0].toarray()[0, statinds.size:]) > 0)
    trange = skw['trange']
    dt = trange[1] - trange[0]
    try:
        vd, pd = snu.solve_nse(functionals=fn, record_on_device=True,
                               bcs_time_only=True, return_dictofvelstrs=True,
                               return_dictofpstrs=True, **skw)
        lr = dict(gtiu.LAST_RUN)
        for bad in (dict(femp, dbcinds=np.concatenate([cntinds, statinds])),
                    dict(femp, dbcinds=dbi[:-1], dbcvals=femp['dbcvals'][:-1],
                         invinds=np.append(inner, dbi[-1]))):
            fbad = fem.MomentumFunctionals.from_rows(
                th, bad, ca=sps.csr_matrix(np.ones((1, len(bad['invinds'])))))
            with pytest.raises(ValueError):
                snu.solve_nse(functionals=fbad, bcs_time_only=True,
                              return_final_vp=True,
                              **_controlled_setup(prob, amplitude=0.3)())
    finally:
        snu.clear_cache()
    assert lr['functionals_on'] == 'device' and lr['record'] == 'device'
    assert lr['run_calls'] == sum(
        1 for c in gtiu._inittimegrid(trange, 10)[1] if c)
    assert lr['functionals'].shape == (11, 2)
    assert np.allclose(lr['functionals_t'], trange[2:], rtol=0, atol=1e-15)
    vs = np.array([vd[t][inner, 0] for t in trange[2:]])
    ps = np.array([pd[t][:, 0] for t in trange[2:]])
    tab = np.array([vd[t][dbi, 0] for t in trange[1:]])
    assert np.abs(np.diff(tab, axis=0)).max() > 1e-3
    _check_rows(fn, lr['functionals'], vs, ps, vd[trange[1]][inner, 0], tab,
                dt, 'solve_nse')
