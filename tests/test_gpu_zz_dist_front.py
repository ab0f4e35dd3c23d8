"""The front of every ROW-PARTITIONED form of the resident IMEX step against
the long double model by rows (`imex_front_model.front_model_rows`), through
the test-only probe `ImexStepper.front_probe` on a partitioned handle:

    DistFront   `k_dist_front<L>` over a RowMap (one launch: convection
                gather, R1 product, b, r = b - K x0, both norms, the carried
                residuals, the copy of x0 for the lazy tail)
    Rows        `enqueue_rows`, `k_imex_rhs<L>` with row0 / prow0 / prow1
                (`DNS_DIST_FRONT=0` when the stepper is created)
    StreamRows  `k_imex_bvec`, then the mapped streamed product or the pair
                product with R1 (option `stream_nnz = 1`, `pair` 1 / 0)

and the warm start the partitioned tails leave over own rows AND halo
(`k_arn_tail_acc` / `k_basis_combine_acc` after general cycles,
`k_arn_tail_lazy1` after a one-step cycle, which also writes the carried
residual and, with a device convection, the cells of the new velocity).

Three ways: ONE RCCL rank in this process (every case, trivial RowMap
{0, NV, NV, NP}), one spawn of 2 and one of 3 gloo-staged ranks sharing the
GPU (every case again, each rank writes one .npz, the parent evaluates the
model).  Partitions (`comm.partition_range`, asserted against `rowmap`):
2 ranks [0, 644, 1286] / [0, 104, 207]; 3 ranks [0, 430, 860, 1286] /
[0, 70, 140, 207] (the middle rank has neighbours on both sides).

Toy problem NV 1286, NP 207, dt = 5e-3, CNAB and SBDF2, rough inputs.  Per
rank and case: the plan (form, use_pre, dcarry, dtail, have_cells), `x0` on
the footprint, `b` and `r` on the own rows (16 u x moduli), `b_p == gp` bit
for bit, the sums of the raw partials, `nparts`; b, r, nfc_c OUTSIDE the own
rows untouched bit for bit; across ranks x0 and the ring on a rank's footprint
equal the owner's entries bit for bit; the un-partitioned model on the rows of
every rank, which cover 0 .. n-1 exactly once.

Pinned exceptions (named in the case ids):
  * `negative-order-is-linear-exception`, `order13-is-cubic-exception`: the
    warm-start kernel of its own, as for Plain / StreamRhs on one GPU
  * `first-step-cuts-exception`: the step that cuts the stepper's row blocks
    neither trusts nor leaves a tail's warm start (use_pre false behind it)
  * StreamRows (`every-row-of-b` in the check): `k_imex_bvec` writes b on
    EVERY row, the streamed product adds R1 w on the own rows only.  The
    entries outside the own rows are read by nothing: the solver's kernels go
    through `dist_rowmap()` (`k_resid_norm`, `k_spmv_multidot`, `k_orth`, the
    true residual), the next front overwrites them; the checkpoint of a batch
    copies them along.  They are held to `cn_c nfc_c + cn_o nfc_o + g`, `gp`.

`LAZY_RTOL`: with `cycle_first = 1` every solve of the lazy cases must be ONE
Krylov step without a restart (asserted from every step's stats), so that the
tail is `k_arn_tail_lazy1` and not the general one.

Largest error / tolerance measured on an MI355X (`pytest -s` prints every
case; K.lpr / R1.lpr as printed: 32 / 32 CNAB, 32 / 16 SBDF2 on every rank,
the instantiations of the one-GPU test), per form over all of its cases:
                         1 RCCL rank   2 gloo ranks   3 gloo ranks
    DistFront  x0           0.159         0.148          0.160
               b            0.150         0.162          0.210
               r            0.184         0.173          0.173
               partR/partB  0.013/0.012   0.019/0.010    0.021/0.014
               rc6 (of c6)  0.069         0.058          0.057
               nfc_c        0.055         0.055          0.055
    Rows       x0 / b       0.062/0.100   0.084/0.125    0.087/0.107
    StreamRows x0 / b       0.062/0.118   0.062/0.118    0.069/0.118
               b, every row   --          0.073          0.073
    un-partitioned model on the rows of every rank: the same figures
All below the 0.25 of the one-GPU forms; no check found a wrong entry, a stale
halo entry or a wrong ring slot: the start residuals of 5-18 x tol of the
partitioned path are not explained by its front or its tails' warm start --
nor by its Krylov cycle, which `tests/test_gpu_zz_dist_krylov.py` holds to the
long double model column by column (0.04 of a tolerance at most, the same bits
on every rank, with and without the exchange of `x`).  The path computes what
it says; what is left is the stopping rule: a one-step cycle takes its step
whenever the start residual is above `1e-3 tol` and reports the residual
BEHIND the step, so a start residual of a few `tol` is by itself no error.

Seconds on the MI355X: the 98 cases on one RCCL rank 7.8 in all
(`test_gpu_imex_front.py`: 12.2 for its 114); the spawn of 2 ranks 6.8, of 3
ranks 6.7 (`test_construction_from_rows_over_three_ranks`: 7.7).
"""
import os
import sys

import numpy as np
import pytest

import conv_model as cm
import imex_front_model as fm
from imex_front_model import U

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DT = fm.DT
NV, NP = 1286, 207
PARTS = {1: ([0, 1286], [0, 207]),
         2: ([0, 644, 1286], [0, 104, 207]),
         3: ([0, 430, 860, 1286], [0, 70, 140, 207])}
FORM = {'dist': 'DistFront', 'rows': 'Rows', 'stream-pair': 'StreamRows',
        'stream-nopair': 'StreamRows'}
# one Krylov step must reach it from every warm start of the lazy cases, and
# the start residual must stay above 1e-3 of it (k_arn_tail_lazy1 takes no
# step below).  Measured on the MI355X over 6 lazy steps of every variant:
# the residual after the one step is 3.3e-4 .. 3.5e-2 of |b| (the start
# residual is no smaller), and the trajectory is the same for every rtol in
# 0.1 .. 10 since each solve is that one step.  0.1 leaves a factor 3 on
# either side.
LAZY_RTOL = 0.1


def _case(name, scheme='sbdf2', kind='dist', nsol=1, order=4, steps=0,
          step_order=None, carry=False, conv=False, table=False, lazy=False,
          fresh=False, expect=(False, False, False, False)):
    """`set_state` with `nsol` solutions, `steps` steps at `step_order`, one
    probe at `order`; `expect`: use_pre, dcarry, dtail, have_cells"""
    return dict(name=name, scheme=scheme, kind=kind, nsol=nsol, order=order,
                steps=steps,
                step_order=order if step_order is None else step_order,
                carry=carry, conv=conv, table=table, lazy=lazy, fresh=fresh,
                expect=(FORM[kind],) + tuple(expect))


def _cases():
    out = []
    # 1. after set_state
    for kind in ('dist', 'rows', 'stream-pair', 'stream-nopair'):
        for scheme in ('cnab', 'sbdf2'):
            for nsol in (1, 2):
                for order in (0, 2, 4, 13):
                    out.append(_case('start-%s-%s-nsol%d-order%d' % (
                        kind, scheme, nsol, order), scheme, kind, nsol, order))
        out.append(_case('start-%s-nsol2-negative-order-is-linear-exception'
                         % kind, 'sbdf2', kind, 2, -1))
        out.append(_case('ring-%s-nsol5-order13-is-cubic-exception' % kind,
                         'sbdf2', kind, 1, 13, steps=4, step_order=2))
    # 2. the warm start of the tails, own rows and halo
    out.append(_case('tail-general-k1-order1-first-step-cuts-exception',
                     order=1, steps=1, fresh=True))
    for k, order in ((1, 1), (2, 2), (3, 3), (4, 4), (5, 13), (6, 4)):
        out.append(_case('tail-general-k%d-order%d' % (k, order), order=order,
                         steps=k, expect=(True, False, False, False)))
        out.append(_case('tail-lazy1-k%d-order%d' % (k, order), order=order,
                         steps=k, lazy=True,
                         expect=(True, False, False, False)))
    # 3. carried residuals
    for scheme in ('cnab', 'sbdf2'):
        for k in (3, 4):
            out.append(_case('carry-lazy1-%s-k%d' % (scheme, k), scheme,
                             steps=k, carry=True, lazy=True,
                             expect=(True, True, False, False)))
        out.append(_case('carry-general-%s-k3-residual-is-zero' % scheme,
                         scheme, steps=3, carry=True,
                         expect=(True, True, False, False)))
    # 4. device convection
    for kind in ('dist', 'rows', 'stream-pair'):
        out.append(_case('conv-start-%s' % kind, 'cnab', kind, 2, conv=True))
    out.append(_case('conv-lazy1-dist-k2-cells-from-the-tail', 'cnab',
                     steps=2, conv=True, lazy=True,
                     expect=(True, False, True, True)))
    out.append(_case('conv-lazy1-dist-start-copies-x0', 'cnab', nsol=2,
                     conv=True, lazy=True,
                     expect=(False, False, True, False)))
    # 5. per-step tables
    out.append(_case('table-position2', steps=2, table=True,
                     expect=(True, False, False, False)))
    out.append(_case('table-last-row', steps=3, table=True,
                     expect=(True, False, False, False)))
    return out


CASES = _cases()


def _toy(prob):
    out = dict(prob=prob, inp=fm.rough_inputs(NV, NP))
    for sch in ('cnab', 'sbdf2'):
        F, J, K, R1, cf = fm.toy_system(prob, scheme=sch)
        out[sch] = dict(F=F, J=J, K=K, R1=R1, cf=cf)
    assert J.shape == (NP, NV)
    return out


# ---- running the cases (this process or a worker) ----------------------------

class Bench(object):
    """systems and steppers on ONE communicator, one per configuration; a
    cached stepper has run one probe, so its row blocks are cut"""

    def __init__(self, comm, toy):
        self.comm, self.toy, self.cache = comm, toy, {}

    def _make(self, case):
        from dolfin_navier_scipy_amd import saddle, convection
        mats, kind = self.toy[case['scheme']], case['kind']
        system = saddle.SaddleSystem(mats['F'], mats['J'])
        if kind.startswith('stream'):
            system.set_option('pair', 1 if kind == 'stream-pair' else 0)
            system.set_option('stream_nnz', 1)
        if case['lazy']:
            system.set_option('cycle_first', 1)
        system.set_comm(self.comm)
        system.setup_precond(cheb_degree=4, schur='dense', fhat='explicit',
                             factorization='full')
        if kind == 'rows':
            os.environ['DNS_DIST_FRONT'] = '0'
        try:
            stp = saddle.ImexStepper(system, mats['R1'])
        finally:
            os.environ.pop('DNS_DIST_FRONT', None)
        cvop = None
        if case['conv']:
            prob = self.toy['prob']
            cvop = convection.ConvectionP2.from_taylor_hood(
                prob['th'], prob['invinds'], prob['dbcinds'], prob['dbcvals'])
            stp.set_convection(cvop, scale=-1.0)
        return system, stp, cvop

    def get(self, case):
        if case['fresh']:
            return self._make(case), True
        key = (case['scheme'], case['kind'], case['conv'], case['lazy'])
        if key not in self.cache:
            made = self._make(case)
            _start(made[1], self.toy['inp'], 1)
            made[1].front_probe(
                _coeffs(self.toy[case['scheme']]['cf'], 4), _opts(),
                nfc_new=None if case['conv'] else self.toy['inp']['nfc_new'][0])
            self.cache[key] = made
        return self.cache[key], False

    def close(self, made=None):
        for system, stp, cvop in ([made] if made else self.cache.values()):
            stp.close()
            if cvop is not None:
                cvop.close()
            system.close()
        if made is None:
            self.cache = {}


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


def run_case(bench, case):
    """`set_state`, the steps, ONE probe; returns the probe's dict with the
    stats of every step (`step_iters`, `step_restarts`, `step_relres`)"""
    inp, cfd = bench.toy['inp'], bench.toy[case['scheme']]['cf']
    (system, stp, cvop), fresh = bench.get(case)
    try:
        opts = _opts(rtol=LAZY_RTOL) if case['lazy'] else _opts()
        _start(stp, inp, case['nsol'], case['table'])
        cfs = _coeffs(cfd, case['step_order'], case['carry'])
        its, rst, rel = [], [], []
        for q in range(case['steps']):
            st = stp.step(cfs, opts=opts, nfc_new=None if case['conv']
                          else inp['nfc_new'][q % 8])
            assert st['status'] == 0, (case['name'], q, st)
            its.append(st['iters'])
            rst.append(st['restarts'])
            rel.append(st['est_relres'])
        out = stp.front_probe(
            _coeffs(cfd, case['order'], case['carry']), opts,
            nfc_new=None if case['conv'] else inp['nfc_new'][case['steps'] % 8])
        out.update(step_iters=np.array(its, dtype=np.int64),
                   step_restarts=np.array(rst, dtype=np.int64),
                   step_relres=np.array(rel))
        return out
    finally:
        if fresh:
            bench.close((system, stp, cvop))


# ---- the checks ----------------------------------------------------------------

def _same(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float64).view(np.int64)
    return a.shape == b.shape and bool(np.all(a == b))


def _conv_space(prob):
    th = prob['th']
    return cm.Space(th._vdofs(), th.glam, th.area, th.vdim, prob['invinds'],
                    prob['dbcinds'])


def _nparts(nrows, lpr):
    g = max(1, min(-(-nrows//(256//lpr)), 4096))
    return max(1, min(g, 2048))


def check_rank(case, out, toy, P, rank, sp):
    """one rank's probe against the model by rows; returns the ratios"""
    name = '%s rank %d/%d' % (case['name'], rank, P)
    mats, inp = toy[case['scheme']], toy['inp']
    K, R1, cfd = mats['K'], mats['R1'], mats['cf']
    st_v, st_p = PARTS[P]
    v0, v1, p0, p1 = st_v[rank], st_v[rank + 1], st_p[rank], st_p[rank + 1]
    ov, op = np.arange(v0, v1), np.arange(p0, p1)
    n = NV + NP
    form = str(out['form'])
    plan = (form, bool(out['use_pre']), bool(out['dcarry']),
            bool(out['dtail']), bool(out['have_cells']))
    assert plan == case['expect'], (name, plan, case['expect'])
    assert tuple(int(v) for v in out['rowmap']) == (v0, v1 - v0, NV + p0,
                                                    p1 - p0), name
    nsol = int(out['nsol'])
    assert nsol == min(case['nsol'] + case['steps'], 5), name
    # the tails take the order as it is; the warm-start kernel of its own has
    # the exceptions of Plain / StreamRhs
    o_eff = case['order'] if plan[1] else fm.order_for(case['order'], 'Plain')
    e = fm.extrap_table(nsol, o_eff)
    a_p = cfd['a_p'] if nsol >= 2 else 0.
    step = case['steps']
    g, gp = (inp['gtab'][step], inp['gptab'][step]) if case['table'] \
        else (inp['g'], inp['gp'])
    assert np.array_equal(out['g_in'], g) and np.array_equal(out['gp_in'], gp)
    if case['table']:
        assert int(out['tab_row']) == step, name
    csp = sp if case['conv'] else None
    fp = fm.footprint(K, R1, st_v, st_p, rank, csp)
    own = fm.own_rows(st_v, st_p, rank, NV)
    rest = np.setdiff1d(np.arange(n), own)
    restv = rest[rest < NV]
    ratios = {}
    nfc = np.array(out['nfc_in'])
    if case['conv']:
        sel = fm.selected_cells(sp, st_v, rank)
        assert int(out['nsel']) == sel.size, (name, out['nsel'], sel.size)
        v = np.full(NV, np.nan)
        keep = fp[fp < NV]
        v[keep] = out['ring'][0, keep]
        with np.errstate(invalid='ignore'):
            res = cm.conv_model(sp, v, toy['prob']['dbcvals'])
            val, bnd = res['vec']
            mag = sp.gather_rows(res['mag']['cells'])
        val = -val
        assert np.all(np.isfinite(val[ov].astype(np.float64))), name
        if plan[4]:
            # the cells saw x0 + alpha z: 8 u x magnitude, as the six-node form
            bnd = bnd + 8*U*mag
        ratios['nfc_c'] = cm.ratio(out['nfc_out'][ov], val[ov], bnd[ov])
        nfc[0] = out['nfc_out']
    else:
        assert int(out['nsel']) == 0, name
        assert _same(out['nfc_out'], out['nfc_in'][0]), name
    assert _same(out['nfc_out'][restv], out['nfc_in'][0][restv]), name
    carry = dict(rc=out['rc6_in']) if plan[2] else None
    mod = fm.front_model_rows(K, R1, st_v, st_p, rank, out['ring'], e,
                              cfd['a_c'], a_p, cfd['cn_c'], cfd['cn_o'], nfc,
                              out['g_in'], out['gp_in'], carry=carry,
                              conv_space=csp)
    assert np.array_equal(mod['fp'], fp) and np.array_equal(mod['own'], own)
    ratios['x0'] = fm.ratio(out['x0'][fp], *mod['x0'])
    ratios['b'] = fm.ratio(out['b'][own], *mod['b'])
    assert _same(out['b'][NV + op], out['gp_in'][op]), name
    if form == 'DistFront':
        ratios['r'] = fm.ratio(out['r'][own], *mod['r'])
        assert int(out['nparts']) == _nparts(own.size, int(out['k_lpr'])), name
        assert out['partR'].size == out['nparts'] == out['partB'].size
        ratios['partR'] = fm.ratio(np.sum(fm._ld(out['partR'])),
                                   *fm.sumsq(out['r'][own]))
        ratios['partB'] = fm.ratio(np.sum(fm._ld(out['partB'])),
                                   *fm.sumsq(out['b'][own]))
        assert _same(out['r'][rest], out['r_in'][rest]), name
    else:
        assert int(out['nparts']) == 0 and out.get('r') is None, name
    # untouched outside the own rows
    if form == 'StreamRows':
        # every-row-of-b exception (module docstring): the vector part
        w = fm._ld
        cc, co = fm.LD(cfd['cn_c']), fm.LD(cfd['cn_o'])
        bv = cc*w(nfc[0]) + co*w(nfc[1]) + w(out['g_in'])
        bva = abs(cc)*np.abs(w(nfc[0])) + abs(co)*np.abs(w(nfc[1])) \
            + np.abs(w(out['g_in']))
        ratios['b every row'] = fm.ratio(out['b'][restv], bv[restv],
                                         bva[restv])
        assert _same(out['b'][rest[rest >= NV]],
                     out['gp_in'][rest[rest >= NV] - NV]), name
    else:
        assert _same(out['b'][rest], out['b_prev'][rest]), name
    if plan[3]:
        assert _same(out['x0copy'], out['x0']), name
    if case['lazy'] and case['steps']:
        assert list(out['step_iters']) == [1]*case['steps'], \
            (name, out['step_iters'], out['step_relres'])
        assert not np.any(out['step_restarts']), name
    if case['carry'] and case['steps']:
        rc = out['rc6_in'][0]
        if case['lazy']:
            # the residual k_arn_tail_lazy1 left behind the last solve
            ring = fm._only(out['ring'], fp)
            Kr = K[own]
            ep = fm.extrap_table(nsol - 1, case['order'])
            x0p = sum(fm.LD(ep[i])*ring[i + 1] for i in range(4) if ep[i])
            ref = (fm._ld(out['b_prev'])[own] - fm.spmv(Kr, ring[0]))[:ov.size]
            unit = (np.abs(fm._ld(out['b_prev'])[own])
                    + fm.spmv(Kr, np.abs(x0p) + np.abs(ring[0]),
                              absval=True))[:ov.size]
            assert np.any(rc[ov] != 0), name
            ratios['rc6'] = fm.ratio(rc[ov], ref, unit, tol=fm.C6*U)
        else:
            # a solve that ended in a general cycle carries none (the memset
            # behind enqueue_cycle_dist): the bits
            assert _same(rc, np.zeros(NV)), name
    worst = max(ratios.values())
    print('%s: %s nsol %d K.lpr %d R1.lpr %d pair %d  worst %.3f  %s%s' % (
        name, plan, nsol, out['k_lpr'], out['r1_lpr'], out['r1_pair'], worst,
        ' '.join('%s %.3f' % kv for kv in sorted(ratios.items())),
        '' if not case['steps'] else '  steps: iters %s res/|b| %s'
        % ([int(v) for v in out['step_iters']],
           ['%.2g' % v for v in out['step_relres']])))
    assert worst <= 1.0, (name, ratios)
    return ratios


def check_case(case, outs, toy, sp):
    """every rank's probe, the ranks against each other and against the
    un-partitioned model; returns the worst ratio per quantity"""
    P = len(outs)
    st_v, st_p = PARTS[P]
    mats = toy[case['scheme']]
    K, R1, cfd = mats['K'], mats['R1'], mats['cf']
    n = NV + NP
    if case['kind'] == 'stream-pair':
        assert all(bool(o['r1_pair']) for o in outs), case['name']
    elif case['kind'] == 'stream-nopair':
        assert not any(bool(o['r1_pair']) for o in outs), case['name']
    worst = {}
    seen = np.zeros(n, dtype=int)
    glob = dict(ring=np.full((5, n), np.nan), x0=np.full(n, np.nan),
                nfc_in=np.full((2, NV), np.nan), nfc_out=np.full(NV, np.nan),
                rc6=np.zeros((2, NV)))
    for r, out in enumerate(outs):
        for k, v in check_rank(case, out, toy, P, r, sp).items():
            worst[k] = max(worst.get(k, 0.), v)
        own = fm.own_rows(st_v, st_p, r, NV)
        ov = own[own < NV]
        seen[own] += 1
        glob['ring'][:, own] = out['ring'][:, own]
        glob['x0'][own] = out['x0'][own]
        glob['nfc_in'][:, ov] = out['nfc_in'][:, ov]
        glob['nfc_out'][ov] = out['nfc_out'][ov]
        if bool(out['dcarry']):
            glob['rc6'][:, ov] = out['rc6_in'][:, ov]
    # no row dropped or doubled
    assert np.all(seen == 1), case['name']
    # across ranks: the footprint holds the owners' entries, bit for bit
    csp = sp if case['conv'] else None
    for r, out in enumerate(outs):
        fp = fm.footprint(K, R1, st_v, st_p, r, csp)
        assert _same(out['x0'][fp], glob['x0'][fp]), (case['name'], r, 'x0')
        for q in range(5):
            assert _same(out['ring'][q, fp], glob['ring'][q, fp]), \
                (case['name'], r, 'ring slot %d' % q)
    # the un-partitioned model from the owners' entries, on every rank's rows
    o0 = outs[0]
    nsol, plan_pre = int(o0['nsol']), bool(o0['use_pre'])
    o_eff = case['order'] if plan_pre else fm.order_for(case['order'], 'Plain')
    nfc = np.array(glob['nfc_in'])
    if case['conv']:
        nfc[0] = glob['nfc_out']
    carry = dict(kind='six', rc=glob['rc6']) if bool(o0['dcarry']) else None
    whole = fm.front_model(K, R1, glob['ring'], fm.extrap_table(nsol, o_eff),
                           cfd['a_c'], cfd['a_p'] if nsol >= 2 else 0.,
                           cfd['cn_c'], cfd['cn_o'], nfc, o0['g_in'],
                           o0['gp_in'], carry=carry)
    for r, out in enumerate(outs):
        own = fm.own_rows(st_v, st_p, r, NV)
        keys = ('b', 'r') if str(out['form']) == 'DistFront' else ('b',)
        for k in keys:
            rt = fm.ratio(out[k][own], whole[k][0][own], whole[k][1][own])
            worst['whole ' + k] = max(worst.get('whole ' + k, 0.), rt)
            assert rt <= 1.0, (case['name'], r, k, rt)
    return worst


# ---- one RCCL rank in this process ---------------------------------------------

@pytest.fixture(scope='module')
def toy(toy_prob):
    from dolfin_navier_scipy_amd import _capi, comm as dcomm
    assert _capi.device_count() > 0, 'HIP device required for -m gpu tests'
    for P in (1, 2, 3):
        for r in range(P):
            assert dcomm.partition_range(NV, P, r) == tuple(PARTS[P][0][r:r + 2])
            assert dcomm.partition_range(NP, P, r) == tuple(PARTS[P][1][r:r + 2])
    out = _toy(toy_prob)
    out['sp'] = _conv_space(toy_prob)
    return out


@pytest.fixture(scope='module')
def bench(toy):
    from dolfin_navier_scipy_amd import comm as dcomm
    cm1 = dcomm.Comm.rccl(0, 1, 0, dcomm.rccl_unique_id())
    b = Bench(cm1, toy)
    yield b
    b.close()
    cm1.close()


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_one_rccl_rank(toy, bench, case):
    out = run_case(bench, case)
    check_case(case, [out], toy, toy['sp'])


# ---- gloo-staged ranks sharing the GPU ------------------------------------------

def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                      RANK=str(rank), WORLD_SIZE=str(world),
                      GLOO_SOCKET_IFNAME='lo')   # loopback, deterministically
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import datetime
    import faulthandler
    import torch.distributed as dist
    faulthandler.dump_traceback_later(100, exit=True)   # never hang a GPU box
    dist.init_process_group('gloo', rank=rank, world_size=world,
                            timeout=datetime.timedelta(seconds=60))
    import scenarios
    from dolfin_navier_scipy_amd import comm as dcomm
    cmg = dcomm.Comm.gloo(0)
    bench = Bench(cmg, _toy(scenarios.toy_problem()))
    res = {}
    # (every rank: the same cases in the same order with the same arguments)
    for case in CASES:
        for k, v in run_case(bench, case).items():
            if v is not None:
                res['%s__%s' % (case['name'], k)] = np.asarray(v)
    np.savez(os.path.join(outdir, 'front_rank{0}.npz'.format(rank)), **res)
    bench.close()
    cmg.close()
    dist.destroy_process_group()


def _spawned(toy, tmp_path, world):
    from spawn_util import spawn_ranks
    spawn_ranks(_worker, world, str(tmp_path))
    files = [np.load(tmp_path / 'front_rank{0}.npz'.format(r))
             for r in range(world)]
    worst = {}
    for case in CASES:
        pre = case['name'] + '__'
        outs = [{k[len(pre):]: f[k] for k in f.files if k.startswith(pre)}
                for f in files]
        for k, v in check_case(case, outs, toy, toy['sp']).items():
            key = '%s %s' % (case['expect'][0], k)
            worst[key] = max(worst.get(key, 0.), v)
    print('%d ranks, largest error / tolerance per form:' % world,
          {k: float('%.3f' % v) for k, v in sorted(worst.items())})


def test_two_gloo_ranks(toy, tmp_path):
    _spawned(toy, tmp_path, 2)


def test_three_gloo_ranks_middle_rank_has_two_neighbours(toy, tmp_path):
    assert PARTS[3][0][1] == 430 and NV + PARTS[3][1][1] == NV + 70
    _spawned(toy, tmp_path, 3)
