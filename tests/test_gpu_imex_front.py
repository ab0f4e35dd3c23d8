"""The front of every resident IMEX step form on one GPU against the long
double model `imex_front_model.py`, through the test-only probe
`ImexStepper.front_probe` (`dns_imex_front_probe`): the warm start `x0`, the
right-hand side `b`, `K x0`, the start residual and the raw partials of both
norms, as `k_step_front<L,0/1/2>` + `k_step_back`, `k_step_one2`, `k_imex_rhs`
+ `k_lincomb*` and `k_imex_bvec` + the streamed / pair product with R1 leave
them -- and the `x0` the TAIL of the step before wrote (`k_arn_tail_acc`,
`k_basis_combine_acc`, `k_arn_tail6`).  No Krylov arithmetic is modelled:
everything is a closed formula of what the probe copies out before the front
runs.  Every entry of every output is compared:

    entry-wise  |got - model| <= 16 u x (moduli of the entry's terms)
    sum partR   against sum r^2 of the downloaded r, 16 u x the sum (b alike)
    six-node carried residual against b_prev - K x_c,
                c6 u (|b_prev| + |K| (|x0_prev| + |x_c|)), c6 = 16

Toy problem (NV 1286, NP 207: no multiple of any lanes-per-row block), dt =
5e-3, rough data (standard normal, fixed seeds: successive solutions differ at
O(1), a wrong ring slot cannot hide in a smooth trajectory).

Pinned exceptions (ids `...-exception`): a negative order is x0 = x_c on the
fused path but the linear start for Plain / StreamRhs; order 13 with a full
ring is the interpolating cubic for Plain / StreamRhs and the quartic where
`prime_six` launches the warm start.

Largest error / tolerance measured on an MI355X (`pytest -s` prints every
case with its plan and the lanes-per-row instantiations that ran; K.lpr = 32
everywhere, R1.lpr = 32 for CNAB and 16 for SBDF2, on the toy and on the wake):
    Fused MODE 0 after set_state    0.139 (r0)   full ring, other signature 0.137
    Fused MODE 1, every tail        0.151 (b)    zero columns: x0 0.110
    Fused MODE 2                    0.149 (K x_c), rcarry 0.085, b 0.083
    Six                             0.234 (b), x0 0.041, kx 0.032, rc6 0.075
    Six, start of prime_six         0.163 (b), x0 0.038
    StreamRhs / Plain               0.116 / 0.108 (b), x0 0.089
    device convection               nfc_c 0.055 (Six 0.025), b 0.118
    per-step tables                 0.136
    cylinder wake N = 1             Fused 0.176, Six 0.252 (b), rc6 0.071
The wake runs the same lanes-per-row instantiations as the toy (32 / 32).

Not reachable from one process and therefore not exercised: the refusal of a
pending pipelined batch (`dns_imex_run` leaves none behind).  A row-partitioned
handle is probed too (a communicator attached to the system: form DistFront);
its forms are held entry by entry in `test_gpu_zz_dist_front.py`.  Of the six
attachments the force functionals are not attached here
(they need a problem's test vectors); the other five are, one by one.
"""
import contextlib

import numpy as np
import pytest
import scipy.sparse as sps

import conv_model as cm
import imex_front_model as fm
from imex_front_model import U

pytestmark = pytest.mark.gpu

DT = fm.DT
ORDERS = [-1, 0, 1, 2, 3, 4, 7, 13]


@pytest.fixture(scope='module')
def toy(toy_prob):
    from dolfin_navier_scipy_amd import _capi
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    out = dict(prob=toy_prob)
    for sch in ('cnab', 'sbdf2'):
        F, J, K, R1, cf = fm.toy_system(toy_prob, scheme=sch)
        out[sch] = dict(F=F, J=J, K=K, R1=R1, cf=cf)
    NP, NV = J.shape
    assert (NV, NP) == (1286, 207)
    out['nv'], out['np'] = NV, NP
    out['inp'] = fm.rough_inputs(NV, NP)
    return out


@contextlib.contextmanager
def _stepper(mats, options=(), conv_prob=None):
    """a system (dense Schur block, full factorisation: what the six-node
    step needs) and ONE stepper on it"""
    from dolfin_navier_scipy_amd import saddle, convection
    system = saddle.SaddleSystem(mats['F'], mats['J'])
    for k, v in options:
        system.set_option(k, v)
    system.setup_precond(cheb_degree=4, schur='dense', factorization='full')
    stp = saddle.ImexStepper(system, mats['R1'])
    cvop = None
    if conv_prob is not None:
        cvop = convection.ConvectionP2.from_taylor_hood(
            conv_prob['th'], conv_prob['invinds'], conv_prob['dbcinds'],
            conv_prob['dbcvals'])
        stp.set_convection(cvop, scale=-1.0)
    try:
        yield stp
    finally:
        stp.close()
        if cvop is not None:
            cvop.close()
        system.close()


def _coeffs(cfd, order, carry=False):
    from dolfin_navier_scipy_amd import saddle
    return saddle.ImexStepper.coeffs(pscale=-1./DT, extrapolate=order,
                                     carry_residual=carry, **cfd)


def _opts(**kw):
    from dolfin_navier_scipy_amd import saddle
    base = dict(rtol=1e-10, maxiter=300, restart=60, use_graph=False,
                reorth=2)
    base.update(kw)
    return saddle.solve_opts(**base)


def _start(stp, inp, nsol=1, table=False):
    stp.set_state(inp['v_c'], v_p=inp['v_p'] if nsol == 2 else None,
                  ptilde_c=inp['pt'], nfc_c=inp['nfc'][0], nfc_o=inp['nfc'][1])
    stp.set_rhs(inp['g'], inp['gp'])
    if table:
        stp.set_rhs_table(inp['gtab'], inp['gptab'])


def _conv_value(prob, v):
    """`(nfc_c, bound, magnitude)` of -N(v)v by the convection model"""
    sp = cm.Space(prob['th']._vdofs(), prob['th'].glam, prob['th'].area,
                  prob['th'].vdim, prob['invinds'], prob['dbcinds'])
    res = cm.conv_model(sp, v, prob['dbcvals'])
    val, bnd = res['vec']
    return -val, bnd, sp.gather_rows(res['mag']['cells'])


def check(name, out, mats, order, expect, conv_prob=None, g=None, gp=None,
          six_carry=False, primed_six=False):
    """every output of a probe against the model; returns the ratios.
    `primed_six`: the warm start is the one `prime_six` launched, not a
    tail's"""
    K, R1, cfd = mats['K'], mats['R1'], mats['cf']
    nv = R1.shape[0]
    form, nsol = out['form'], out['nsol']
    plan = (form, out['mode'], out['use_pre'], out['carry'])
    assert plan == expect, (name, plan, expect)
    # the coefficient set: the tails and the fused fronts take the order as it
    # is, the warm-start kernel of Plain / StreamRhs has its exceptions
    o_eff = fm.order_for(order, form, primed_six=True) if primed_six \
        else order if (out['use_pre'] or form == 'Six') \
        else fm.order_for(order, form)
    e = fm.extrap_table(nsol, o_eff)
    a_p = cfd['a_p'] if nsol >= 2 else 0.
    if g is not None:
        assert np.array_equal(out['g_in'], g), name
        assert np.array_equal(out['gp_in'], gp), name
    nfc = out['nfc_in'].copy()
    ratios = {}
    six = form == 'Six'
    if conv_prob is not None:
        val, bnd, mag = _conv_value(conv_prob, out['ring'][0, :nv])
        if six:
            # the cells saw x0 + sum y_j Z_j: the velocity to 4 u |v| per entry,
            # first order in a form quadratic in v: 8 u x magnitude
            bnd = bnd + 8*U*mag
        ratios['nfc_c'] = cm.ratio(out['nfc_out'], val, bnd)
        nfc[0] = out['nfc_out']
        # (b is held to the nfc_c the kernel itself formed and stored)
    else:
        assert np.array_equal(out['nfc_out'], out['nfc_in'][0]), name
    carry = None
    if out['mode'] == 2:
        carry = dict(kind='mode2', b_prev=out['b_prev'], kxs=out['kxs_in'],
                     r_old=out['rcarry_in'])
    elif six and six_carry:
        carry = dict(kind='six', rc=out['rc6_in'])
    mod = fm.front_model(K, R1, out['ring'], e, cfd['a_c'], a_p, cfd['cn_c'],
                         cfd['cn_o'], nfc, out['g_in'], out['gp_in'],
                         carry=carry)
    ratios['x0'] = fm.ratio(out['x0'], *mod['x0'])
    ratios['b'] = fm.ratio(out['b'], *mod['b'])
    assert np.array_equal(out['b'][nv:], out['gp_in']), name
    if six:
        ratios['kx'] = fm.ratio(out['kx'], *mod['kx'])
        assert out['nparts'] == 0 and out['r'] is None
    if form == 'Fused':
        ratios['r'] = fm.ratio(out['r'], *mod['r'])
        n = K.shape[0]
        assert out['nparts'] == max(1, min((n + 31)//32, 1024)), name
        assert out['partR'].size == out['nparts'] == out['partB'].size
        ratios['partR'] = fm.ratio(np.sum(fm._ld(out['partR'])),
                                   *fm.sumsq(out['r']))
        ratios['partB'] = fm.ratio(np.sum(fm._ld(out['partB'])),
                                   *fm.sumsq(out['b']))
    if out['mode'] == 2:
        # (rigorous: 16 u (|b_prev| + |K| |x_c|))
        ratios['kxs_cur'] = fm.ratio(out['kxs_cur'], *mod['kxc'])
        ratios['rcarry'] = fm.ratio(out['rcarry_out'], *mod['rcarry'])
    if carry is not None and carry['kind'] == 'six':
        ref = (fm._ld(out['b_prev']) - fm.spmv(K, fm._ld(out['ring'][0])))[:nv]
        unit = fm.six_residual_bound(K, out['b_prev'], out['x0_other'],
                                     out['ring'][0])[:nv]
        ratios['rc6'] = fm.ratio(out['rc6_in'][0], ref, unit/U, tol=fm.C6*U)
    worst = max(ratios.values())
    print('%s: %s nsol %d K.lpr %d R1.lpr %d  worst %.3f  %s' % (
        name, plan, nsol, out['k_lpr'], out['r1_lpr'], worst,
        ' '.join('%s %.3f' % kv for kv in sorted(ratios.items()))))
    assert worst <= 1.0, (name, ratios)
    return ratios


def _steps(stp, cf, inp, k, opts, first=0):
    """steps `first .. first + k`, each with its own rough convection vector"""
    for q in range(first, first + k):
        st = stp.step(cf, nfc_new=inp['nfc_new'][q % 8], opts=opts)
        assert st['status'] == 0, st


# ---- Fused, MODE 0 -----------------------------------------------------------

@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
@pytest.mark.parametrize('nsol', [1, 2])
@pytest.mark.parametrize('order', ORDERS, ids=lambda o: (
    'order%d' % o if o >= 0 else 'negative-order-is-x_c-exception'))
def test_fused_mode0_after_set_state(toy, scheme, nsol, order):
    inp, mats = toy['inp'], toy[scheme]
    with _stepper(mats) as stp:
        _start(stp, inp, nsol)
        out = stp.front_probe(_coeffs(mats['cf'], order), _opts(),
                              nfc_new=inp['nfc_new'][0])
    assert out['nsol'] == nsol
    assert np.array_equal(out['ring'][0], np.r_[inp['v_c'], inp['pt']])
    assert np.array_equal(out['nfc_in'], [inp['nfc_new'][0], inp['nfc'][0]])
    check('mode0 %s nsol%d order%d' % (scheme, nsol, order), out, mats, order,
          ('Fused', 0, False, False), g=inp['g'], gp=inp['gp'])


@pytest.mark.parametrize('k', [2, 3, 4, 5, 6])
def test_fused_mode0_full_ring_other_signature(toy, k):
    """k steps at order 4, probed at order 2: the tail's warm start carries
    the signature of order 4 and must not be used (nsol 3, 4, 5)"""
    inp, mats = toy['inp'], toy['sbdf2']
    with _stepper(mats) as stp:
        _start(stp, inp, 1)
        _steps(stp, _coeffs(mats['cf'], 4), inp, k, _opts())
        out = stp.front_probe(_coeffs(mats['cf'], 2), _opts(),
                              nfc_new=inp['nfc_new'][k])
    assert out['nsol'] == min(k + 1, 5)
    check('mode0 ring k%d' % k, out, mats, 2, ('Fused', 0, False, False),
          g=inp['g'], gp=inp['gp'])


# ---- Fused, MODE 1: x0 is what a tail wrote ----------------------------------

TAILS = {
    'reorth2': dict(reorth=2), 'reorth2-graph': dict(reorth=2, use_graph=True),
    'reorth1': dict(reorth=1), 'reorth1-graph': dict(reorth=1, use_graph=True),
    'restart3': dict(reorth=2, restart=3),
    'zero-columns': dict(reorth=2, atol=1e30),
}


@pytest.mark.parametrize('tail', sorted(TAILS))
@pytest.mark.parametrize('k,order', [(1, 1), (2, 2), (3, 3), (4, 4), (5, 13),
                                     (6, 4)])
def test_fused_mode1_warm_start_of_the_tail(toy, tail, k, order):
    inp, mats = toy['inp'], toy['sbdf2']
    opts = _opts(**TAILS[tail])
    cf = _coeffs(mats['cf'], order)
    with _stepper(mats) as stp:
        _start(stp, inp, 1)
        if tail == 'zero-columns':
            # (the steps before converge: the ring is rough, only the LAST
            # solve accepts its warm start as it is)
            _steps(stp, cf, inp, k - 1, _opts())
            _steps(stp, cf, inp, 1, opts, first=k - 1)
        else:
            _steps(stp, cf, inp, k, opts)
        if tail == 'restart3':
            assert stp.last_stats['restarts'] >= 1, stp.last_stats
        if tail == 'zero-columns':
            assert stp.last_stats['iters'] == 0, stp.last_stats
        out = stp.front_probe(cf, opts, nfc_new=inp['nfc_new'][k])
    assert out['nsol'] == min(k + 1, 5)
    if k > 1:
        # a rough ring: no two slots alike
        assert not np.array_equal(out['ring'][0], out['ring'][1])
    if tail == 'zero-columns':
        # (zero columns: the solution IS the warm start the step began with)
        assert k == 1 or not np.array_equal(out['ring'][1], out['ring'][2])
    check('mode1 %s k%d order%d' % (tail, k, order), out, mats, order,
          ('Fused', 1, True, False), g=inp['g'], gp=inp['gp'])


# ---- Fused, MODE 2: residual carry-over --------------------------------------

@pytest.mark.parametrize('scheme', ['cnab', 'sbdf2'])
@pytest.mark.parametrize('order', [4, 13])
def test_fused_mode2_carry(toy, scheme, order):
    inp, mats = toy['inp'], toy[scheme]
    cf = _coeffs(mats['cf'], order, carry=True)
    with _stepper(mats) as stp:
        _start(stp, inp, 1)
        _steps(stp, cf, inp, 7, _opts())
        out = stp.front_probe(cf, _opts(), nfc_new=inp['nfc_new'][7])
    r = check('mode2 %s order%d' % (scheme, order), out, mats, order,
              ('Fused', 2, True, True), g=inp['g'], gp=inp['gp'])
    assert set(r) >= {'kxs_cur', 'rcarry', 'r', 'b'}


# ---- Six ----------------------------------------------------------------------

@pytest.mark.parametrize('lazy', [1, 0])
@pytest.mark.parametrize('carry', [1, 0])
@pytest.mark.parametrize('order', [4, 13])
def test_six_node_front(toy, order, carry, lazy):
    inp, mats = toy['inp'], toy['cnab']
    cf = _coeffs(mats['cf'], order, carry=bool(carry))
    opts = _opts(use_graph=True)
    with _stepper(mats, options=(('step6_lazy', lazy),)) as stp:
        _start(stp, inp, 1)
        # 4 start-up steps, then batches of 8 and 16 six-node steps
        stp.run(28, cf, opts)
        rec = stp.last_run
        assert rec['unconverged'] == 0, rec
        assert rec['lazy_steps'] + rec['eager_steps'] >= 16, rec
        if not lazy:
            assert rec['lazy_steps'] == 0, rec
        out = stp.front_probe(cf, opts, cycle_len=1)
    assert out['nsol'] == 5
    r = check('six order%d carry%d lazy%d' % (order, carry, lazy), out, mats,
              order, ('Six', 0, False, False), g=inp['g'], gp=inp['gp'],
              six_carry=bool(carry))
    assert ('rc6' in r) == bool(carry)


def test_six_node_front_primed_order13_is_quartic_exception(toy):
    """the warm start `prime_six` launches: with order 13 the QUARTIC, not the
    least-squares fit the tails write (pinned as it is).  A primed start is
    in place when a run ends on the fallback of a batch that failed twice:
    with `restart=1` no cycle is longer than one column, the rough solves
    need more, both attempts of the batch fail, its 8 steps are taken one by
    one and `prime_six` runs behind them."""
    inp, mats = toy['inp'], toy['cnab']
    cf = _coeffs(mats['cf'], 13, carry=False)
    opts = _opts(use_graph=True, restart=1)
    with _stepper(mats) as stp:
        _start(stp, inp, 1)
        stp.run(12, cf, opts)               # 4 start-up steps, one batch of 8
        rec = stp.last_run
        assert rec['unconverged'] == 0, rec
        assert rec['replayed'] == 16, rec
        assert rec['lazy_steps'] + rec['eager_steps'] == 0, rec
        out = stp.front_probe(cf, opts, cycle_len=1)
    assert out['nsol'] == 5
    # (the plan notes the tail's warm start in the work buffer of the steps
    # taken one by one; the six-node front does not read it)
    check('six primed order13', out, mats, 13, ('Six', 0, True, False),
          g=inp['g'], gp=inp['gp'], primed_six=True)
    # ... and it is NOT the fit
    mod = fm.front_model(mats['K'], mats['R1'], out['ring'],
                         fm.extrap_table(5, 13), 1., 0., 0., 0.,
                         out['nfc_in'], out['g_in'], out['gp_in'])
    assert fm.ratio(out['x0'], *mod['x0']) > 100


# ---- StreamRhs and Plain ------------------------------------------------------

def _separate_options(form, mats, pair=1):
    if form == 'StreamRhs':
        return (('pair', pair), ('stream_nnz', 1))
    # Plain: K streams, R1 does not
    assert mats['R1'].nnz < mats['K'].nnz
    return (('pair', pair), ('stream_nnz', mats['R1'].nnz + 1))


SEPARATE = [
    # (id, steps before, order, what the warm start is)
    ('nsol1-order4', 0, 4), ('nsol2-order4', 0, 4), ('nsol5-order4', 4, 4),
    ('nsol1-a_p-dropped-order1', 0, 1),
    ('nsol2-negative-order-is-linear-exception', 0, -1),
    ('nsol5-order13-is-cubic-exception', 4, 13),
]


@pytest.mark.parametrize('form,pair', [('StreamRhs', 1), ('StreamRhs', 0),
                                       ('Plain', 1)])
@pytest.mark.parametrize('case', SEPARATE, ids=[c[0] for c in SEPARATE])
def test_stream_and_plain_fronts(toy, form, pair, case):
    """the steps before run at order 2: their tails' warm start carries another
    signature, the warm-start kernel of the form runs
    (`dns_imex::warm_start`)"""
    name, k, order = case
    inp, mats = toy['inp'], toy['sbdf2']
    cf = _coeffs(mats['cf'], order)
    with _stepper(mats, options=_separate_options(form, mats, pair)) as stp:
        _start(stp, inp, 2 if name.startswith('nsol2') else 1)
        _steps(stp, _coeffs(mats['cf'], 2), inp, k, _opts())
        out = stp.front_probe(cf, _opts(), nfc_new=inp['nfc_new'][k])
    assert out['nsol'] == int(name[4])
    # (the pair format of R1 really is what the streamed product took)
    assert out['r1_pair'] == (form == 'StreamRhs' and pair == 1)
    check('%s pair%d %s' % (form, pair, name), out, mats, order,
          (form, 0, False, False), g=inp['g'], gp=inp['gp'])


# ---- device convection ----------------------------------------------------------

@pytest.mark.parametrize('form', ['Fused', 'StreamRhs', 'Plain', 'Six'])
def test_device_convection(toy, form):
    inp, mats, prob = toy['inp'], toy['cnab'], toy['prob']
    options = () if form in ('Fused', 'Six') \
        else _separate_options(form, mats)
    cf = _coeffs(mats['cf'], 4, carry=False)
    opts = _opts(use_graph=form == 'Six')
    with _stepper(mats, options=options, conv_prob=prob) as stp:
        _start(stp, inp, 2)
        if form == 'Six':
            stp.run(27, cf, opts)
            assert stp.last_run['lazy_steps'] + stp.last_run['eager_steps'] \
                >= 16, stp.last_run
            out = stp.front_probe(cf, opts, cycle_len=1)
        else:
            # the refusal of the step's own preamble, nothing touched
            from dolfin_navier_scipy_amd import _capi
            with pytest.raises(_capi.DnsError, match='convection') as ei:
                stp.front_probe(cf, opts, nfc_new=inp['nfc_new'][0])
            assert ei.value.status == _capi.DNS_ERR_BAD_ARGUMENT
            out = stp.front_probe(cf, opts)
    # the swap of a device convection: the old nfc_c is nfc_o
    if form != 'Six':
        assert np.array_equal(out['nfc_in'][1], inp['nfc'][0])
    r = check('conv %s' % form, out, mats, 4,
              (form, 0, False, False), conv_prob=prob, g=inp['g'],
              gp=inp['gp'])
    assert 'nfc_c' in r


# ---- per-step tables ----------------------------------------------------------

@pytest.mark.parametrize('steps', [2, 3], ids=['position2', 'last-row'])
def test_rhs_table_row(toy, steps):
    inp, mats = toy['inp'], toy['sbdf2']
    cf = _coeffs(mats['cf'], 4)
    with _stepper(mats) as stp:
        _start(stp, inp, 1, table=True)
        _steps(stp, cf, inp, steps, _opts())
        assert stp.table_position() == (steps, 4 - steps)
        out = stp.front_probe(cf, _opts(), nfc_new=inp['nfc_new'][steps])
    assert out['tab_row'] == steps
    check('table row %d' % steps, out, mats, 4, ('Fused', 1, True, False),
          g=inp['gtab'][steps], gp=inp['gptab'][steps])


# ---- the probe's contract -------------------------------------------------------

def test_probe_refusals_and_consumed_stepper(toy):
    from dolfin_navier_scipy_amd import _capi
    inp, mats = toy['inp'], toy['sbdf2']
    cf = _coeffs(mats['cf'], 4)
    with _stepper(mats) as stp:
        _start(stp, inp, 1)
        # every attachment: refused by name, nothing touched
        from dolfin_navier_scipy_amd import fem
        nv = toy['nv']
        row = sps.csr_matrix(np.ones((1, nv)))
        one = np.ones((1, 1))
        qf = fem.QuadraticFunctionals.from_matrices(
            nv, [sps.identity(nv, format='csr')], [(0, 0, 0)])
        attach = [
            (lambda: stp.set_recorder(4, cv_mat=row), stp.clear_recorder),
            (lambda: stp.set_statistics([0, 0, 0, 0], nbins=1),
             stp.clear_statistics),
            (lambda: stp.set_quadratics(qf, 4, DT), stp.clear_quadratics),
            (lambda: stp.set_ensemble([0, 1, 2, 3]), stp.clear_ensemble),
            (lambda: stp.set_feedback(row, row.T.tocsr(), one, one, one, .5,
                                      .5, DT), stp.clear_feedback)]
        for on, off in attach:
            on()
            with pytest.raises(_capi.DnsError, match='attachments') as ei:
                stp.front_probe(cf, _opts())
            assert ei.value.status == _capi.DNS_ERR_BAD_ARGUMENT
            off()
        # a communicator on the system: a row-partitioned handle
        import ctypes as ct
        from dolfin_navier_scipy_amd.comm import Comm
        ar = _capi.ALLREDUCE_CB(lambda ctx, dev, count: 0)
        ag = _capi.ALLGATHERV_CB(lambda ctx, dev, starts, nr: 0)
        h = ct.c_void_p()
        _capi.check(stp.lib.dns_comm_create_callbacks(0, 1, 0, ar, ag, None,
                                                      ct.byref(h)))
        stp.sys.set_comm(Comm(h, 0, 1, keep=(ar, ag)))
        # (attaching has dropped the preconditioner: set up by rows, the probe
        # then runs the partitioned front; tests/test_gpu_zz_dist_front.py)
        stp.sys.setup_precond(cheb_degree=4, schur='dense', fhat='explicit',
                              factorization='full')
        out = stp.front_probe(cf, _opts(), nfc_new=inp['nfc_new'][0])
        assert out['form'] == 'DistFront'
        assert out['rowmap'] == (0, nv, nv, toy['np'])
        _start(stp, inp, 1)
        stp.sys.set_comm(None)
        stp.lib.dns_comm_destroy(h)
        # (detaching has dropped the preconditioner)
        with pytest.raises(_capi.DnsError, match='preconditioner') as ei:
            stp.front_probe(cf, _opts())
        assert ei.value.status == _capi.DNS_ERR_NOT_READY
        stp.sys.setup_precond(cheb_degree=4, schur='dense',
                              factorization='full')
        out = stp.front_probe(cf, _opts(), nfc_new=inp['nfc_new'][0])
        assert out['form'] == 'Fused'
        for call in (lambda: stp.step(cf, opts=_opts()),
                     lambda: stp.run(2, cf, _opts()),
                     lambda: stp.front_probe(cf, _opts())):
            with pytest.raises(_capi.DnsError,
                               match='dns_imex_front_probe') as ei:
                call()
            assert ei.value.status == _capi.DNS_ERR_NOT_READY
        stp.get_state()


def test_probed_stepper_after_set_state_equals_a_fresh_one(toy):
    """6 steps (carry on: the probe has overwritten K x_c, the carried
    residual, the convection slot and the work vector) bit for bit"""
    inp, mats = toy['inp'], toy['sbdf2']
    cf = _coeffs(mats['cf'], 4, carry=True)

    def trajectory(probe):
        with _stepper(mats) as stp:
            _start(stp, inp, 1)
            _steps(stp, cf, inp, 7, _opts())
            if probe:
                out = stp.front_probe(cf, _opts(), nfc_new=inp['nfc_new'][7])
                assert out['mode'] == 2
            _start(stp, inp, 2)
            _steps(stp, cf, inp, 6, _opts())
            return stp.get_state()
    (v0, p0), (v1, p1) = trajectory(False), trajectory(True)
    assert np.array_equal(v0, v1) and np.array_equal(p0, p1)


# ---- a second matrix -----------------------------------------------------------

@pytest.mark.parametrize('form', ['Fused', 'Six'])
def test_cylinder_wake(form):
    """the cylinder wake N = 1 (the system of
    `test_pipelined_run_warm_start_orders`), rough data: Fused MODE 1 and Six.
    It runs the same lanes-per-row instantiations as the toy (printed)."""
    from dolfin_navier_scipy_amd.fem import get_sysmats
    femp, sm, rhsd = get_sysmats(problem='cylinderwake', N=1, Re=60)
    M, A, J = (sps.csr_matrix(sm[k]) for k in 'MAJ')
    NP, NV = J.shape
    dt = 1./256
    F, R1 = (M + .5*dt*A).tocsr(), (M - .5*dt*A).tocsr()
    for X in (F, R1, J):
        X.sort_indices()
    K = sps.bmat([[F, J.T], [J, None]], format='csr')
    mats = dict(F=F, J=J, K=K, R1=R1,
                cf=dict(a_c=1., a_p=0., cn_c=1.5*dt, cn_o=-.5*dt))
    inp = fm.rough_inputs(NV, NP, seed=50)
    cf = _coeffs(mats['cf'], 4, carry=True)
    with _stepper(mats) as stp:
        _start(stp, inp, 1)
        if form == 'Six':
            opts = _opts(use_graph=True)
            stp.run(28, cf, opts)
            assert stp.last_run['lazy_steps'] + stp.last_run['eager_steps'] \
                >= 16, stp.last_run
            out = stp.front_probe(cf, opts, cycle_len=1)
            expect = ('Six', 0, False, False)
        else:
            _steps(stp, cf, inp, 3, _opts())
            out = stp.front_probe(cf, _opts(), nfc_new=inp['nfc_new'][3])
            expect = ('Fused', 1, True, False)
    check('wake %s' % form, out, mats, 4, expect, g=inp['g'], gp=inp['gp'],
          six_carry=form == 'Six')
