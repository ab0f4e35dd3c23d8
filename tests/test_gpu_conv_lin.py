"""The linearised and adjoint convection of `ConvectionP2.set_base_flow`
(`k_conv_lin_cells<ADJ>`, `k_conv_lin_cells_lane<ADJ>`) on the device:

 * cell values and `apply` of both modes and both element kernels, PER ENTRY
   against the long double model of tests/conv_lin_model.py within its counted
   bound, on the meshes of tests/conv_meshes.py (block edges of both kernels,
   fan and rectangles, with and without Dirichlet dofs, cells without an inner
   dof, seeded numbering); the two kernels bit equal,
 * the polarisation identity N(V+w)(V+w) - N(V)V - N(w)w = L(V)w with the
   nonlinear kernels, the duality of the two modes, `sel` / `nsel`,
 * clearing the base flow gives back the bits of an operator that never had one
   (`apply`, and 8 CNAB steps on the N=2 wake),
 * 12 steps of `cnab` / `sbdftwo` on the N=2 wake against the host model of
   tests/imex_host_model.py driven by `TaylorHood.linearised_convection_vec`
   (1e-8, v in the M-norm and p), two `run` calls with the base flow changed
   in between, recorder rows against `get_state`,
 * every refusal by its message.

Largest error / bound measured on the MI355X (the report test prints them with
`pytest -s`): cell values forward 0.122, adjoint 0.119; `apply` forward 0.088,
adjoint 0.109; polarisation 0.009, duality 0.001; the loops against the host
model v 1.2e-11, p 1.1e-9 (of 1e-8).  76 cases, 17 s.
"""
import os
import types

import numpy as np
import pytest

import conv_lin_model as clm
import conv_meshes
import conv_model as cm
import imex_host_model as ihm
import scenarios
from test_gpu_feedback import wake_setup

pytestmark = pytest.mark.gpu

LD = cm.LD
VTOL, PTOL = 1e-8, 1e-8
WORST = {}
MODES = ('forward', 'adjoint')


def _note(path, r):
    WORST[path] = max(WORST.get(path, 0.0), r)
    return r


@pytest.fixture(scope='module')
def gtiu():
    from dolfin_navier_scipy_amd import time_int_utils, _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    return time_int_utils


def _mesh(name):
    kind, n = name.split('-')[0], int(name.split('-')[1])
    if kind == 'fan':
        return conv_meshes.fan(n, seed=n)
    return conv_meshes.rectangle(n, seed=n,
                                 decades=3.0 if 'spread' in name else 0.0)


CASES = ['rect-%d' % n for n in conv_meshes.SIZES] + \
    ['rect-33-nobc', 'fan-40', 'fan-40-nobc', 'rect-257-spread']
_cache = {}


def _grid(rng, n, scale=1.0):
    """random values on the grid 2^-20: sums of two of them are exact"""
    return np.round(scale*rng.standard_normal(n)*2.0**20)/2.0**20


class Case(object):
    """`cv8` / `cv1`: the eight-lane and the one-lane operator, `cv0`: one that
    never gets a base flow.  `w`, `wd`: the perturbation and its Dirichlet
    values (forward mode; the adjoint takes zeros), `V`, `Vd`: the base flow"""

    def __init__(self, name):
        from dolfin_navier_scipy_amd import convection
        self.name = name
        mesh = self.mesh = _mesh(name)
        n = mesh.ncells
        if 'nobc' in name:
            inv, dbc = mesh.split('none')
        elif n <= 2:
            inv, dbc = mesh.split(0.4)
        else:
            inv, dbc = mesh.split('boundary', full_cells=2 if n >= 255 else 0)
        self.inv, self.dbc = inv, dbc
        rng = np.random.default_rng(100 + n)
        self.V, self.Vd = _grid(rng, inv.size), _grid(rng, dbc.size)
        self.w, self.wd = _grid(rng, inv.size), _grid(rng, dbc.size)
        self.w2 = _grid(rng, inv.size)
        if 'spread' in name:
            self.w = self.w*10.0**rng.integers(-6, 7, inv.size)
            self.V = self.V*10.0**rng.integers(-3, 4, inv.size)
        self.sp = cm.Space(mesh.cell_vdofs, mesh.glam, mesh.area, mesh.vdim,
                           inv, dbc)

        def make():
            return convection.ConvectionP2(mesh.cell_vdofs, mesh.glam,
                                           mesh.area, mesh.vdim, inv, dbc,
                                           self.wd)
        self.cv8, self.cv0 = make(), make()
        old = os.environ.get('DNS_CONV_LANE_MIN')
        os.environ['DNS_CONV_LANE_MIN'] = '1'
        try:
            self.cv1 = make()
        finally:
            if old is None:
                del os.environ['DNS_CONV_LANE_MIN']
            else:
                os.environ['DNS_CONV_LANE_MIN'] = old
        self._models = {}

    def set_mode(self, mode, V=None, Vd=None):
        """both linearised operators into `mode` about `(V, Vd)`"""
        adj = mode == 'adjoint'
        for cv in (self.cv8, self.cv1):
            cv.clear_base_flow()
            cv.set_dbcvals(np.zeros(self.dbc.size) if adj else self.wd)
            cv.set_base_flow((self.V if V is None else V,
                              self.Vd if Vd is None else Vd), adjoint=adj)
            assert cv.linearised == mode
        return adj

    def model(self, mode, w=None):
        key = (mode, None if w is None else id(w))
        if key not in self._models:
            adj = mode == 'adjoint'
            self._models[key] = clm.lin_model(
                self.sp, self.V, self.Vd, self.w if w is None else w,
                np.zeros(self.dbc.size) if adj else self.wd, adj)
        return self._models[key]

    def close(self):
        for cv in (self.cv8, self.cv1, self.cv0):
            cv.close()


def case(name):
    if name not in _cache:
        _cache[name] = Case(name)
    return _cache[name]


# ---- 1. cell values and apply against the model ------------------------------

@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', CASES)
def test_cells_and_apply_both_element_kernels(name, mode):
    c = case(name)
    c.set_mode(mode)
    ref = c.model(mode)
    cells8, pos8 = c.cv8.cell_values(c.w)
    cells1, pos1 = c.cv1.cell_values(c.w)
    assert np.array_equal(pos8, pos1)
    assert sorted(pos8.tolist()) == list(range(c.mesh.ncells))
    assert np.array_equal(cells8, cells1)            # bit for bit
    rc = _note('cells ' + mode, cm.ratio(cells8[:, pos8].T, *ref['cells']))
    val, bnd = ref['vec']
    worst = 0.0
    for scale in (1.0, -1.0, 0.37):
        # (`scale` is one more rounding: the count K + len holds it)
        got8 = c.cv8.apply(c.w, scale=scale).reshape(-1)
        got1 = c.cv1.apply(c.w, scale=scale).reshape(-1)
        assert np.array_equal(got8, got1)
        worst = max(worst, cm.ratio(got8, LD(scale)*val, abs(LD(scale))*bnd))
    ra = _note('apply ' + mode, worst)
    print('%s %s: cells %.3f apply %.3f' % (name, mode, rc, ra))
    assert rc <= 1.0 and ra <= 1.0
    if mode == 'forward' and c.sp.nv > 4:
        # (not vacuous: the nonlinear form of w is not within the bounds)
        assert cm.ratio(c.cv0.apply(c.w), val, bnd) > 1.0


# ---- 2. polarisation: ties the new kernels to the old ones --------------------

@pytest.mark.parametrize('name', [n for n in CASES if 'spread' not in n])
def test_polarisation_identity_with_the_nonlinear_kernels(name):
    """N(V+w)(V+w) - N(V)V - N(w)w = L(V)w; V, w and their Dirichlet values
    lie on a grid where V + w is exact.  Within the sum of the three bounds of
    the nonlinear terms (conv_model.py)"""
    c = case(name)
    c.set_mode('forward')
    lin = c.cv8.apply(c.w).reshape(-1).astype(LD)
    s, sd = c.V + c.w, c.Vd + c.wd
    assert np.array_equal((s - c.V), c.w) and np.array_equal(sd - c.Vd, c.wd)
    try:
        total, bound = np.zeros(c.sp.nv, dtype=LD), np.zeros(c.sp.nv, dtype=LD)
        for v, d, sign in ((s, sd, 1), (c.V, c.Vd, -1), (c.w, c.wd, -1)):
            c.cv0.set_dbcvals(d)
            total = total + sign*c.cv0.apply(v).reshape(-1).astype(LD)
            bound = bound + cm.conv_model(c.sp, v, d)['vec'][1]
    finally:
        c.cv0.set_dbcvals(c.wd)
    r = _note('polarisation', cm.ratio(total - lin, np.zeros(c.sp.nv, LD),
                                       bound))
    print('%s: polarisation %.3f' % (name, r))
    assert r <= 1.0
    if c.sp.nv > 4:
        assert np.abs(lin).max() > 0


# ---- 3. duality ---------------------------------------------------------------

@pytest.mark.parametrize('name', CASES)
def test_duality_of_the_two_modes(name):
    """w2 . L(V) w1 = w1 . L(V)^T w2 for zero Dirichlet values of w1, w2,
    within the bounds of the two device vectors contracted with the other
    field (the dot products are taken in long double)"""
    c = case(name)
    z = np.zeros(c.dbc.size)
    w1, w2 = c.w, c.w2
    c.set_mode('adjoint')
    aw2 = c.cv8.apply(w2).reshape(-1)
    b_ad = clm.lin_model(c.sp, c.V, c.Vd, w2, z, True)['vec'][1]
    c.set_mode('forward')
    for cv in (c.cv8, c.cv1):
        cv.set_dbcvals(z)
    fw1 = c.cv8.apply(w1).reshape(-1)
    b_fw = clm.lin_model(c.sp, c.V, c.Vd, w1, z, False)['vec'][1]
    a = np.sum(w2.astype(LD)*fw1.astype(LD))
    b = np.sum(w1.astype(LD)*aw2.astype(LD))
    bound = np.sum(np.abs(w2)*b_fw) + np.sum(np.abs(w1)*b_ad)
    r = _note('duality', cm.ratio(np.array([a]), np.array([b]),
                                  np.array([bound])))
    print('%s: duality %.3f (%.3e against %.3e)' % (name, r, float(a - b),
                                                    float(bound)))
    assert r <= 1.0


# ---- 4. selection -------------------------------------------------------------

@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', ['rect-1', 'rect-33', 'rect-257', 'fan-40',
                                  'rect-1000'])
def test_selection_writes_only_the_listed_cells(name, mode):
    c = case(name)
    c.set_mode(mode)
    nc = c.mesh.ncells
    rng = np.random.default_rng(nc)
    fill = 777.25
    for cv in (c.cv8, c.cv1):
        full, _ = cv.cell_values(c.w)
        for nsel in sorted(set([1, max(1, nc//2), max(1, nc - 1)])):
            sel = rng.permutation(nc)[:nsel].astype(np.int32)
            part, _ = cv.cell_values(c.w, sel=sel, fill=fill)
            rest = np.ones(nc, dtype=bool)
            rest[sel] = False
            assert np.array_equal(part[:, sel], full[:, sel])
            assert np.all(part[:, rest] == fill)
        none, _ = cv.cell_values(c.w, sel=np.zeros(0, dtype=np.int32),
                                 fill=fill)
        assert np.all(none == fill)


# ---- 5. clearing restores the old bits ----------------------------------------

@pytest.mark.parametrize('name', ['rect-33', 'fan-40', 'rect-1000'])
def test_clearing_restores_the_bits_of_apply(name):
    c = case(name)
    want = c.cv0.apply(c.w)
    for mode in MODES:
        c.set_mode(mode)
        for cv in (c.cv8, c.cv1):
            assert not np.array_equal(cv.apply(c.w), want)
            cv.clear_base_flow()
            assert cv.linearised is False
            cv.set_dbcvals(c.wd)
            assert np.array_equal(cv.apply(c.w), want)


@pytest.fixture(scope='module')
def wake(gtiu):
    return wake_setup()


def _full(wake, v_inner, zero_dbc=False):
    femp = wake['femp']
    full = np.zeros(femp['V'].vdim)
    full[femp['invinds']] = np.asarray(v_inner).reshape(-1)
    if not zero_dbc:
        full[femp['dbcinds']] = femp['dbcvals']
    return full


class LinLoop(object):
    """CNAB / SBDF2 on the N=2 wake with a tight solve; `zero_dbc`: the
    operator's own Dirichlet values (those of the perturbation) are zero"""

    def __init__(self, wake, scheme='cnab', zero_dbc=False, make_host=False,
                 cvop=None):
        from dolfin_navier_scipy_amd import saddle, convection
        femp, M, A, J, rhsd = (wake['femp'], wake['M'], wake['A'], wake['J'],
                               wake['rhsd'])
        self.wake, self.zero_dbc = wake, zero_dbc
        dt = self.dt = 1./512
        if scheme == 'cnab':
            F, R1, g = M + .5*dt*A, M - .5*dt*A, dt*rhsd['fv']
            ckw = dict(a_c=1., a_p=0., cn_c=1.5*dt, cn_o=-.5*dt, pscale=-1./dt)
        else:
            F, R1, g = M + 2./3*dt*A, M, 2./3*dt*rhsd['fv']
            ckw = dict(a_c=4./3, a_p=-1./3, cn_c=4./3*dt, cn_o=-2./3*dt,
                       pscale=-1./dt)
        self.g, self.gp = g, rhsd['fp']
        self.cf = saddle.ImexStepper.coeffs(extrapolate=4, **ckw)
        self.hcf = types.SimpleNamespace(**ckw)
        self.system = saddle.SaddleSystem(F.tocsr(), J)
        self.system.setup_precond(cheb_degree=6, schur='dense')
        self.stp = saddle.ImexStepper(self.system, R1.tocsr())
        dbv = np.zeros(femp['dbcvals'].size) if zero_dbc else femp['dbcvals']
        self.own_cvop = cvop is None
        self.cvop = cvop if cvop is not None else \
            convection.ConvectionP2.from_taylor_hood(
                femp['V'], femp['invinds'], femp['dbcinds'], dbv)
        self.stp.set_rhs(g, rhsd['fp'])
        self.stp.set_convection(self.cvop, scale=-1.0)
        self.opts = saddle.solve_opts(method='gmres', rtol=1e-12, maxiter=400,
                                      restart=60, check_every=2,
                                      use_graph=True, reorth=2)
        self.host = None
        if make_host:
            self.host = ihm.HostStepper(ihm.HostSystem(F.tocsr(), J),
                                        R1.tocsr())
            self.host.set_rhs(g, rhsd['fp'])

    def start(self, w0):
        """both steppers from `w0` with the device's own convection history"""
        nfc = self.cvop.apply(w0, scale=-1.0)
        self.stp.set_state(w0, v_p=w0, nfc_c=nfc, nfc_o=nfc)
        if self.host is not None:
            self.host.set_state(w0.reshape((-1, 1)), v_p=w0.reshape((-1, 1)),
                                nfc_c=nfc, nfc_o=nfc)

    def close(self):
        self.stp.set_convection(None)
        self.stp.close()
        if self.own_cvop:
            self.cvop.close()
        self.system.close()


def test_clearing_restores_the_bits_of_eight_cnab_steps(gtiu, wake):
    """an operator that has stepped four linearised steps (on a stepper of
    its own) and is cleared steps the nonlinear problem, on a fresh stepper,
    to the bits of one that never had a base flow"""
    w0 = wake['inivel'][:, 0]
    Vfull = _full(wake, 0.9*w0)
    la, lb = LinLoop(wake), LinLoop(wake)
    lc = None
    try:
        la.start(w0)
        la.stp.run(8, la.cf, la.opts)
        va, pa = la.stp.get_state()
        lb.cvop.set_base_flow(Vfull)
        lb.start(w0)
        lb.stp.run(4, lb.cf, lb.opts)
        vlin = lb.stp.get_state()[0]
        lb.cvop.clear_base_flow()
        lc = LinLoop(wake, cvop=lb.cvop)
        lc.start(w0)
        lc.stp.run(8, lc.cf, lc.opts)
        vc, pc = lc.stp.get_state()
        assert np.array_equal(va, vc) and np.array_equal(pa, pc)
        # (the linearised steps were others)
        lb.start(w0)
        lb.stp.run(4, lb.cf, lb.opts)
        assert not np.array_equal(lb.stp.get_state()[0], vlin)
    finally:
        la.close()
        if lc is not None:
            lc.close()
        lb.close()


# ---- 6. stepper parity ----------------------------------------------------------

def _mnorm(M, v):
    v = np.asarray(v).reshape(-1)
    return np.sqrt(v @ (M @ v))


def _host_conv(wake, Vfull, adjoint, zero_dbc):
    """the NumPy statement as an `f_vdp(vfull)`: minus, it goes to the rhs"""
    th, inv = wake['femp']['V'], wake['femp']['invinds']

    def f_vdp(vfull):
        return -th.linearised_convection_vec(
            Vfull, np.asarray(vfull).reshape(-1), adjoint=adjoint)[inv, :]
    return f_vdp


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
def test_twelve_loop_steps_follow_the_host_model(gtiu, wake, scheme, mode):
    """`cnab` / `sbdftwo` with a linearised operator, recorded on the device,
    against the same loop over `imex_host_model.HostStepper` with
    `TaylorHood.linearised_convection_vec` for `f_vdp`"""
    from dolfin_navier_scipy_amd import convection
    femp, M = wake['femp'], wake['M']
    inv, dbcinds, dbcvals = femp['invinds'], femp['dbcinds'], femp['dbcvals']
    adj = mode == 'adjoint'
    # (forward: a boundary-actuated perturbation, the inflow values on its
    # Dirichlet dofs; adjoint: zeros)
    wdbc = np.zeros(dbcvals.size) if adj else dbcvals
    th = femp['V']

    def appnd(vvec, bcs):
        full = np.full((th.vdim, 1), np.nan)
        full[inv] = vvec
        full[dbcinds, 0] = wdbc
        return full
    Vfull = _full(wake, wake['inivel'])
    rng = np.random.default_rng(3)
    w0 = 0.1*wake['inivel'] + 1e-3*rng.standard_normal(wake['inivel'].shape)

    def kwargs(rec):
        kw = wake['make_kw'](rec, nts=12)
        kw.update(inivel=w0, appndbcs=appnd,
                  f_vdp=_host_conv(wake, Vfull, adj, adj))
        return kw
    hrec = scenarios.Recorder()
    with pytest.MonkeyPatch.context() as mp:
        htiu = ihm.install(mp)
        hinteg = htiu.cnab if scheme == 'cnab' else htiu.sbdftwo
        vh, ph, ffh = hinteg(**kwargs(hrec))
    cvop = convection.ConvectionP2.from_taylor_hood(th, inv, dbcinds, wdbc)
    grec = scenarios.Recorder()
    kw = kwargs(grec)
    kw.pop('f_vdp')
    try:
        cvop.set_base_flow(Vfull, adjoint=adj)
        integ = gtiu.cnab if scheme == 'cnab' else gtiu.sbdftwo
        vg, pg, ffg = integ(device_convection=cvop, invinds=inv,
                            resident=dict(record=True, savevp_times=None),
                            **kw)
        assert cvop.linearised == mode
    finally:
        cvop.close()
    assert ffg == ffh == 0
    assert gtiu.LAST_RUN['record'] == 'device'
    tg, vgs, pgs = grec.arrays()
    thh, vhs, phs = hrec.arrays()
    assert tg.size == 13 and np.array_equal(tg, thh)
    worst_v = worst_p = 0.0
    for k in range(tg.size):
        ev = _mnorm(M, vgs[k][inv] - vhs[k][inv])/_mnorm(M, vhs[k][inv])
        worst_v = max(worst_v, ev)
        if k >= 1:
            worst_p = max(worst_p, np.linalg.norm(pgs[k] - phs[k])
                          / np.linalg.norm(phs[k]))
    print('%s %s: worst v %.2e p %.2e' % (scheme, mode, worst_v, worst_p))
    _note('loop v ' + mode, worst_v/VTOL)
    _note('loop p ' + mode, worst_p/PTOL)
    assert worst_v <= VTOL and worst_p <= PTOL
    # the recorder's last row is the state the loop hands back, bit for bit
    assert np.array_equal(vg[:, 0], vgs[-1][inv])
    assert np.array_equal(pg[:, 0], pgs[-1])
    # (the run is not the nonlinear one)
    assert _mnorm(M, vgs[-1][inv] - w0[:, 0]) > 1e-6*_mnorm(M, w0[:, 0])


@pytest.mark.parametrize('mode', MODES)
def test_base_flow_changed_between_two_runs(gtiu, wake, mode):
    """16 + 16 steps in two `run` calls, the base flow changed between them;
    then the first base flow again: no stale graph.  The recorder's rows of the
    last call against `get_state`, bit for bit"""
    adj = mode == 'adjoint'
    M = wake['M']
    rng = np.random.default_rng(5)
    w0 = 0.1*wake['inivel'][:, 0] + 1e-3*rng.standard_normal(M.shape[0])
    V1 = _full(wake, wake['inivel'])
    V2 = _full(wake, 0.6*wake['inivel'][:, 0]
               + 1e-2*rng.standard_normal(M.shape[0]))
    lp = LinLoop(wake, zero_dbc=adj, make_host=True)
    wfull = lambda v: _full(wake, v, zero_dbc=adj)
    holder = dict(f=None)
    lp.host.set_convection(types.SimpleNamespace(
        eval=lambda v, row: holder['f'](wfull(v))))
    try:
        lp.cvop.set_base_flow(V1, adjoint=adj)
        holder['f'] = _host_conv(wake, V1, adj, adj)
        lp.start(w0)
        for Vk, n in ((V1, 16), (V2, 16), (V1, 16)):
            lp.cvop.set_base_flow(Vk, adjoint=adj)
            holder['f'] = _host_conv(wake, Vk, adj, adj)
            lp.stp.set_recorder(n, snap_slots='all')
            lp.stp.run(n, lp.cf, lp.opts)
            lp.host.run(n, lp.hcf)
            vg, pg = lp.stp.get_state()
            vh, ph = lp.host.get_state()
            ev = _mnorm(M, vg - vh)/_mnorm(M, vh)
            ep = np.linalg.norm(pg - ph)/np.linalg.norm(ph)
            print('%s after %d more steps: v %.2e p %.2e' % (mode, n, ev, ep))
            assert ev <= VTOL and ep <= PTOL
            vs, ps = lp.stp.record_snapshots()
            assert np.array_equal(vs[-1], vg[:, 0])
            assert np.array_equal(ps[-1], pg[:, 0])
        # (the change matters: with V1 throughout the state is elsewhere)
        lp.cvop.set_base_flow(V1, adjoint=adj)
        lp.start(w0)
        lp.stp.clear_recorder()
        lp.stp.run(48, lp.cf, lp.opts)
        assert _mnorm(M, lp.stp.get_state()[0] - vh) > 1e3*VTOL*_mnorm(M, vh)
    finally:
        lp.close()


# ---- 7. refusals ----------------------------------------------------------------

def _refused(call, *words):
    from dolfin_navier_scipy_amd import _capi
    with pytest.raises(ValueError) as exc:
        call()
    assert isinstance(exc.value, _capi.DnsError)
    assert exc.value.status == _capi.DNS_ERR_BAD_ARGUMENT
    for word in words:
        assert word in str(exc.value), str(exc.value)


def test_refusals_of_the_operator(gtiu):
    c = case('rect-33')
    cv = c.cv8
    cv.clear_base_flow()
    try:
        # the adjoint takes zero Dirichlet values and no table
        cv.set_dbcvals(c.wd)
        _refused(lambda: cv.set_base_flow((c.V, c.Vd), adjoint=True),
                 'linearised convection, adjoint mode', 'Dirichlet value')
        assert cv.linearised is False
        cv.set_dbc_table(np.zeros((3, c.dbc.size)))
        _refused(lambda: cv.set_base_flow((c.V, c.Vd), adjoint=True),
                 'adjoint mode', 'dns_conv_set_dbc_table')
        cv.set_dbcvals(np.zeros(c.dbc.size))
        cv.set_base_flow((c.V, c.Vd), adjoint=True)
        _refused(lambda: cv.set_dbcvals(c.wd), 'adjoint mode',
                 'Dirichlet value')
        _refused(lambda: cv.set_dbc_table(np.zeros((3, c.dbc.size))),
                 'adjoint mode', 'table')
        assert cv.linearised == 'adjoint'
        # (forward mode takes both)
        cv.set_base_flow((c.V, c.Vd))
        cv.set_dbc_table(np.tile(c.wd, (3, 1)))
        cv.set_dbc_row(1)
        assert cm.ratio(cv.apply(c.w), *c.model('forward')['vec']) <= 1.0
        cv.set_dbcvals(c.wd)
        # the entry points that form the nonlinear matrices and tensors
        cv.bind_pattern(cv.connectivity())
        for mode in MODES:
            c.set_mode(mode)
            _refused(lambda: cv.assemble(c.w), 'linearised convection operator',
                     mode + ' mode', 'dns_conv_assemble')
            _refused(lambda: cv.assemble(c.w, dbcvals_lin=c.wd),
                     'dns_conv_assemble2')
            _refused(lambda: cv.project_tensor(np.ones((2, c.sp.nv + c.sp.nv % 2))),
                     'dns_conv_project_tensor')
        # wrong sizes of the base flow are the caller's ValueError
        with pytest.raises(ValueError):
            cv.set_base_flow(np.zeros(c.mesh.vdim + 1))
        full = np.zeros(c.mesh.vdim)
        full[c.inv], full[c.dbc] = c.V, c.Vd
        # (the loop above has left the adjoint's zero values behind)
        cv.clear_base_flow()
        cv.set_dbcvals(c.wd)
        cv.set_base_flow(full)
        assert cm.ratio(cv.apply(c.w), *c.model('forward')['vec']) <= 1.0
    finally:
        cv.clear_base_flow()
        cv.set_dbcvals(c.wd)


def test_refusals_of_the_steppers(gtiu, toy_prob):
    from dolfin_navier_scipy_amd import (saddle, convection, comm as dcomm,
                                         newton_picard as dnp)
    M, A, J = (toy_prob['smc'][k] for k in 'MAJ')
    dt = 5e-3
    cvop = convection.ConvectionP2.from_taylor_hood(
        toy_prob['th'], toy_prob['invinds'], toy_prob['dbcinds'],
        toy_prob['dbcvals'])
    Vfull = np.zeros(toy_prob['th'].vdim)
    Vfull[toy_prob['dbcinds']] = toy_prob['dbcvals']
    cvop.set_base_flow(Vfull)
    # the trapezoidal stepper
    _refused(lambda: dnp.TrapezoidalStepper(M, A, J, cvop, 4, dt,
                                            precond=False),
             'linearised convection operator', 'the trapezoidal stepper')
    # a row-partitioned IMEX stepper
    cmm = dcomm.Comm.rccl(0, 1, 0, dcomm.rccl_unique_id())
    system = saddle.SaddleSystem((M + .5*dt*A).tocsr(), J)
    stp = None
    try:
        system.set_comm(cmm)
        system.setup_precond(cheb_degree=6, schur='dense', fhat='explicit')
        stp = saddle.ImexStepper(system, (M - .5*dt*A).tocsr())
        _refused(lambda: stp.set_convection(cvop, scale=-1.0),
                 'linearised convection operator on a row-partitioned stepper',
                 'N(v)v')
        # (attached before it was linearised: the step refuses)
        cvop.clear_base_flow()
        stp.set_convection(cvop, scale=-1.0)
        cvop.set_base_flow(Vfull)
        stp.set_state(np.zeros(J.shape[1]))
        cf = saddle.ImexStepper.coeffs(a_c=1., cn_c=1.5*dt, cn_o=-.5*dt,
                                       pscale=-1./dt, extrapolate=4)
        _refused(lambda: stp.run(1, cf, saddle.solve_opts(method='gmres')),
                 'linearised convection operator on a row-partitioned stepper')
    finally:
        if stp is not None:
            stp.set_convection(None)
            stp.close()
        system.set_comm(None)
        system.close()
        cmm.close()
        cvop.close()


def test_functionals_with_cells_are_refused(gtiu, wake):
    from dolfin_navier_scipy_amd import fem
    femp = wake['femp']
    fn = fem.boundary_forces(femp['V'], femp)
    assert fn.cells[0].size > 0
    lp = LinLoop(wake)
    try:
        w0 = 0.1*wake['inivel'][:, 0]
        lp.start(w0)
        lp.stp.set_functionals(fn, 8, lp.dt)
        lp.stp.run(1, lp.cf, lp.opts)
        lp.cvop.set_base_flow(_full(wake, wake['inivel']))
        for go in (lambda: lp.stp.run(1, lp.cf, lp.opts),
                   lambda: lp.stp.step(lp.cf, opts=lp.opts)):
            _refused(go, 'linearised convection operator with functionals '
                     'with cells')
        lp.cvop.clear_base_flow()
        lp.stp.run(1, lp.cf, lp.opts)
    finally:
        lp.close()


def test_rom_is_refused_by_the_loop(gtiu, wake):
    """`resident=dict(pod=..., rom=...)`: refused on the host, by name, before
    anything is armed"""
    from dolfin_navier_scipy_amd import convection
    femp = wake['femp']
    cvop = convection.ConvectionP2.from_taylor_hood(
        femp['V'], femp['invinds'], femp['dbcinds'], femp['dbcvals'])
    kw = wake['make_kw'](scenarios.Recorder(), nts=4)
    kw.pop('f_vdp')
    try:
        cvop.set_base_flow(_full(wake, wake['inivel']))
        with pytest.raises(ValueError) as exc:
            gtiu.cnab(device_convection=cvop, invinds=femp['invinds'],
                      resident=dict(pod=object(), rom=object()), **kw)
        assert 'linearised convection operator' in str(exc.value)
        assert '`rom`' in str(exc.value)
    finally:
        cvop.close()


def test_zz_report_and_close():
    """prints the largest error / bound per path (the module's docstring holds
    the figures measured on the MI355X)"""
    print('largest error / bound per path: '
          + '  '.join('%s %.3f' % kv for kv in sorted(WORST.items())))
    for c in _cache.values():
        c.close()
    _cache.clear()
