// extern "C" entry points of the device-resident IMEX loop (included by
// dns_amd.hip).

// The ring-independent part of everything a captured step depends on besides
// the solver options: coefficients, this stepper and its convection, tables,
// the primed-state flags and the attachments (feedback, recorder, functionals)
uint64_t dns_imex::config_key(const dns_imex_coeffs *cf) const {
    uint64_t k = mix64(
        0x1234, {kw(cf->a_c), kw(cf->a_p), kw(cf->cn_c), kw(cf->cn_o),
                 kw(conv_scale), kw(cf->extrapolate_x0), kw(this), kw(conv),
                 kw(tables() ? 1 + 2 * tab_v + 4 * tab_p : 0), kw(gtab.p),
                 kw(gptab.p), kw(tab_rows),
                 kw((cf->carry_residual != 0) + 2 * carry_ok + 4 * six_ok +
                    8 * dcells_ok)});
    if (conv) k = mix64(k, {kw(conv->dbc_rows), kw(conv->dbc_tab.p)});
    // (a linearised operator: mode and base flow; whatever sets, changes or
    // clears them bumps dbc_gen)
    if (conv && conv->linearised())
        k = mix64(k, {kw(conv->lin_mode), kw(conv->vbase.p),
                      kw(conv->dbc_gen)});
    // (about a base trajectory: its buffers, its rows, the index table and the
    // row the host names; they bump dbc_gen as well)
    if (conv && conv->linearised() && conv->bt_rows > 0)
        k = mix64(k, {kw(conv->btraj.p), kw(conv->btraj_dbc.p),
                      kw(conv->bt_rows + 2 * (conv->bt_dbc_rows > 1)),
                      kw(conv->brow.p), kw(conv->nbrow), kw(conv->bt_row)});
    // (interpolating between its rows: another instance of the element
    // kernels, with the weight table, its length and the host-named weight
    // among its arguments)
    if (conv && conv->linearised() && conv->bt_rows > 0 && conv->bt_lerp)
        k = mix64(k, {kw(1), kw(conv->bwgt.p), kw(conv->bwgt.n),
                      kw(conv->nbrow), kw(conv->bt_weight)});
    return attachments_key(k);
}

// ... and the ring as it stands
uint64_t dns_imex::step_key(const dns_imex_coeffs *cf) const {
    return mix64(config_key(cf), {kw(cur + 8 * prev + 64 * pprev + 512 * p3 +
                                     4096 * p4 + 32768 * work),
                                  kw(nc + 2 * std::min(nsol, 5))});
}

// R1 (or this rank's rows of it, starting at the even global row `v0`) in the
// pair format; silently absent where the format does not apply
int dns_imex::build_r1_pair(const dns::HostCsr &rows, int v0) {
    dns_saddle *h = sys;
    R1p.release_all();
    if (!h->pair_knob || !h->streams(R1)) return DNS_OK;
    dns::HostPair hp;
    const bool block = rows.nrows != h->nv;
    const bool ok = block ? dns::host_pair_from_k(rows, h->nv, hp, nullptr,
                                                  rows.nrows, v0, 0)
                          : dns::host_pair_from_k(rows, h->nv, hp);
    if (ok) DNS_TRY(R1p.upload(hp, h->stream));
    return DNS_OK;
}

// what the six-node step asks of the system, whatever the solve
bool dns_imex::six_capable() const {
    // (its tail evaluates N(v)v of the new velocity: not a linearised operator)
    return env_six && !(conv && conv->linearised()) && !sys->dist() &&
           !sys->streams(sys->K) && !sys->streams(R1) && sys->have_jg &&
           sys->popts.schur == DNS_SCHUR_DENSE;
}

// The form of the step about to be built (or replayed).  `cycle_len`: its
// sys->pipeline_c (0: a synchronous solve, first cycle sys->cycle_first long)
StepPlan dns_imex::plan(const dns_imex_coeffs *cf, const dns_solve_opts *o,
                        int cycle_len) const {
    const dns_saddle *h = sys;
    const bool gm = o->method == DNS_METHOD_GMRES, cr = cf->carry_residual != 0;
    const bool rows = h->dist() && part.on;
    const bool sk = h->streams(h->K), sr = h->streams(R1);
    StepPlan p;
    // one-launch prologue on one GPU while the system is latency bound (it
    // gathers K's columns from up to five history vectors; beyond ~4e5
    // unknowns forming x0 first and gathering once is cheaper)
    const bool fused = !h->dist() && !sk;
    // the tail before has left this step's warm start in the work buffer (same
    // coefficient set)?  (row-partitioned with the stepper's own halo plan: the
    // tails of the partitioned cycle extrapolate over own entries and halo)
    p.can_pre = !h->dist() || part.on;
    p.use_pre = p.can_pre && pre_ok &&
                pre_sig == dns::extrap_sig(nsol, cf->extrapolate_x0);
    // six-node step: pipelined, primed by prime_six or by the step before
    const bool six = six_capable() && six_ok && cycle_len > 0 && gm &&
                     o->reorth == 2 && nsol >= 5;
    // residual carry-over: a PRE step whose ring of K x products is current
    p.carry = !six && cr && fused && p.use_pre && carry_ok && b_valid && gm;
    // row-partitioned, latency regime: ONE front kernel (convection gather,
    // right-hand side, residual and its norms)
    const bool dfront = rows && env_dfront && !sr && !sk && gm;
    // (the residual of every one-step solve is carried into the next
    // right-hand side, as on one GPU: k_dist_front / k_arn_tail_lazy1)
    p.dcarry = dfront && cr && rc6[0].p && rc6[1].p && nsol >= 2;
    // ... whose cycle ends in k_arn_tail_lazy1 with the convection cells of
    // the new velocity (the conditions of `lazy` in enqueue_cycle_dist): a
    // pipelined one-step cycle, or a synchronous solve whose first cycle is one
    // step long (its cells count only if it was the whole solve: step_device)
    const bool one = cycle_len == 1 || (cycle_len == 0 && h->cycle_first == 1);
    p.dtail = dfront && env_dtail && conv && h->dist_lazy1 && o->reorth == 2 &&
              o->atol < 1.0 && o->maxiter > 0 && one && x0c.p != nullptr;
    p.have_cells = dfront && conv && dcells_ok && dcells_gen == conv->dbc_gen;
    // row-partitioned: the preconditioned vectors travel over THIS stepper's
    // halo (rows of K, of R1 and the convection cells): the new solution is
    // valid on it, the next step's front and warm start need no exchange
    p.zwide = rows;
    p.form = six      ? StepPlan::Six
             : fused  ? StepPlan::Fused
             : dfront ? StepPlan::DistFront
             : rows   ? (sr ? StepPlan::StreamRows : StepPlan::Rows)
             : sr && !h->dist() ? StepPlan::StreamRhs
                                : StepPlan::Plain;
    if (p.form == StepPlan::Fused) p.mode = p.carry ? 2 : p.use_pre ? 1 : 0;
    return p;
}

// the cell values of the current velocity by a plain launch (start of a
// pipelined phase, after a batch has been restored): the first step then
// already is the seven-kernel step the graphs were captured for
int dns_imex::prime_dcells(const dns_imex_coeffs *cf, const dns_solve_opts *o) {
    dns_saddle *h = sys;
    dcells_ok = false;
    // (asked before the batches set the cycle length: a one-step cycle?)
    if (!plan(cf, o, 1).dtail) return DNS_OK;
    conv->attach_counter(stepctr.p);
    DNS_TRY(conv->enqueue_cells(xs[cur].p, h->stream, part.conv_sel.p,
                                part.nsel));
    dcells_ok = true;
    dcells_gen = conv->dbc_gen;
    return DNS_OK;
}

// partials of ||r||^2, ||b||^2 the front leaves (0: no residual)
int dns_imex::front_nparts(const StepPlan &pl) const {
    const dns_saddle *h = sys;
    if (pl.form == StepPlan::Six) return h->gridD;
    if (pl.form == StepPlan::Fused)
        return std::max(1, std::min((h->n + 31) / 32, 1024));
    if (pl.form != StepPlan::DistFront) return 0;
    const dns::RowMap rm = h->dist_rowmap();
    return std::max(1, std::min(dns::grid_for_rows(rm.len1 + rm.len2, h->K.lpr),
                                2048));
}

// six-node step, ONE launch: K x0, R1 v, convection gather, b, r, norms
int dns_imex::front_six(const dns_imex_coeffs *cf, const StepPlan &) {
    dns_saddle *h = sys;
    const int par = work & 1;
    // (residuals that do not exist yet are zeros: prime_six)
    const double *rcc = cf->carry_residual ? rc6[par].p : nullptr;
    const double *rcp = cf->carry_residual ? rc6[1 - par].p : nullptr;
    // K x0 side by side with b; r = b - kx and the norms are formed by the
    // first tau kernel (gridD partials)
    const int gk = h->gridS, gb = dns::grid_for_rows(h->n, h->K.lpr);
    const ConvGather cg = conv_gather();
    DNS_LPR_SWITCH(
        h->K.lpr,
        hipLaunchKernelGGL(
            (dns::k_step_one2<L>), gk + gb, dns::kBlock, 0, h->stream, gk, h->n,
            h->nv, h->K.rowptr.p, h->K.colidx.p, h->K.vals.p, R1.rowptr.p,
            R1.colidx.p, R1.vals.p, x0buf[par].p, xs[cur].p, xs[prev].p,
            cf->a_c, (nsol >= 2) ? cf->a_p : 0.0, nfc[nc].p, nfc[no].p,
            cf->cn_c, cf->cn_o, g_ref(), gp_ref(), cg.gptr, cg.gidx,
            cg.cellvals, conv_scale, rcc, rcp, b.p, kx6.p));
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}

// front: convection cells || (x0, K x0, R1 v) -- one launch; back: convection
// gather, b, r = b - K x0, norms (step_kernels.hpp)
int dns_imex::front_fused(const dns_imex_coeffs *cf, const StepPlan &pl) {
    dns_saddle *h = sys;
    hipStream_t s = h->stream;
    const int n = h->n, nv = h->nv;
    double *x = xs[work].p;
    double e[5];
    dns::extrap_coeffs(nsol, cf->extrapolate_x0, e);
    // a linearised operator launches its own element kernel in front; the
    // front kernel then runs as it does without an operator (one launch more)
    const bool lin = conv && conv->linearised();
    if (lin) DNS_TRY(conv->enqueue_cells(xs[cur].p, s));
    const dns_conv *fc = lin ? nullptr : conv;
    const int nconv =
        fc ? (8 * fc->ncells + dns::kBlock - 1) / dns::kBlock : 0;
    const dns::CarryRef cr =
        pl.carry ? dns::CarryRef{kxs[cur].p,  kxs[prev].p, kxs[pprev].p,
                                 kxs[p3].p,   kxs[p4].p,   rcarry.p}
                 : dns::CarryRef{nullptr, nullptr, nullptr,
                                 nullptr, nullptr, nullptr};
#define DNS_FRONT(MODE)                                                        \
    DNS_LPR_SWITCH(                                                            \
        h->K.lpr,                                                              \
        hipLaunchKernelGGL(                                                    \
            (dns::k_step_front<L, MODE>), nconv + h->gridS, dns::kBlock, 0, s, \
            nconv, fc ? fc->ncells : 0,                                        \
            fc ? fc->cellmap.p : (const int *)nullptr,                         \
            fc ? fc->glam.p : (const double *)nullptr,                         \
            fc ? fc->area.p : (const double *)nullptr,                         \
            fc ? fc->dbc_ref() : dns::TabRef{nullptr, nullptr, 0, 1},          \
            fc ? fc->cellvals.p : (double *)nullptr, n, nv,                    \
            h->K.rowptr.p, h->K.colidx.p, h->K.vals.p, R1.rowptr.p,            \
            R1.colidx.p, R1.vals.p, xs[cur].p, xs[prev].p, xs[pprev].p,        \
            xs[p3].p, xs[p4].p, e[0], e[1], e[2], e[3], e[4], cf->a_c,         \
            (nsol >= 2) ? cf->a_p : 0.0, x, h->r.p, b.p, cr))
    switch (pl.mode) {
        case 2: DNS_FRONT(2); break;
        case 1: DNS_FRONT(1); break;
        default: DNS_FRONT(0);
    }
#undef DNS_FRONT
    const ConvGather cg = conv_gather();
    hipLaunchKernelGGL(dns::k_step_back<8>, front_nparts(pl), dns::kBlock, 0, s,
                       n, nv, nfc[nc].p, nfc[no].p, cf->cn_c, cf->cn_o, g_ref(),
                       gp_ref(), cg.gptr, cg.gidx, cg.cellvals, conv_scale, b.p,
                       h->r.p, h->partR.p, h->partB.p);
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}

// x0 by a kernel of its own, unless the tail before has left it in the work
// buffer.  (The kernels carry the interpolating coefficients: the least-squares
// fit, whose warm start the tail kernels write, falls back to the cubic here.
// A negative extrapolate_x0 gives the LINEAR start here but x0 = x_c on the
// fused path (extrap_coeffs): kept as it is, not yet reconciled)
int dns_imex::warm_start(const dns_imex_coeffs *cf, const StepPlan &pl) {
    if (pl.use_pre) return DNS_OK;
    const int ex = cf->extrapolate_x0;
    const int exq = ex == dns::kExtrapFit35 ? 3 : ex < 0 ? 1 : ex;
    double e[5];
    return dns::enqueue_extrap(dns::extrap_coeffs(nsol, exq, e), xs, *this,
                               xs[work].p, sys->n, sys->stream);
}

// row-partitioned, latency regime: cells (unless the tail before has left
// them: seven kernels instead of eight), warm start, ONE front kernel
int dns_imex::front_dist(const dns_imex_coeffs *cf, const StepPlan &pl) {
    dns_saddle *h = sys;
    hipStream_t s = h->stream;
    const int par = work & 1;
    if (conv && !pl.have_cells)
        DNS_TRY(conv->enqueue_cells(xs[cur].p, s, part.conv_sel.p, part.nsel));
    DNS_TRY(warm_start(cf, pl));
    const ConvGather cg = conv_gather();
    DNS_LPR_SWITCH(
        h->K.lpr,
        hipLaunchKernelGGL(
            (dns::k_dist_front<L>), front_nparts(pl), dns::kBlock, 0, s,
            h->dist_rowmap(), h->nv, h->K.rowptr.p, h->K.colidx.p, h->K.vals.p,
            xs[work].p, R1.rowptr.p, R1.colidx.p, R1.vals.p, xs[cur].p,
            (nsol >= 2) ? xs[prev].p : xs[cur].p, cf->a_c,
            (nsol >= 2) ? cf->a_p : 0.0, nfc[nc].p, nfc[no].p, cf->cn_c,
            cf->cn_o, g_ref(), gp_ref(), cg.gptr, cg.gidx, cg.cellvals,
            conv_scale, b.p, h->r.p, h->partR.p, h->partB.p,
            pl.dcarry ? rc6[par].p : (const double *)nullptr,
            pl.dcarry ? rc6[1 - par].p : (const double *)nullptr,
            pl.dtail ? x0c.p : (double *)nullptr, h->n));
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}

// convection and right-hand side by kernels of their own (Plain; Rows: this
// rank's rows), then the warm start
int dns_imex::front_rows(const dns_imex_coeffs *cf, const StepPlan &pl) {
    dns_saddle *h = sys;
    hipStream_t s = h->stream;
    const bool own = pl.form == StepPlan::Rows;
    const int rv0 = own ? h->dd->v0 : 0, rv1 = own ? h->dd->v1 : h->nv;
    const int rp0 = own ? h->dd->p0 : 0, rp1 = own ? h->dd->p1 : h->np;
    if (conv && own)
        DNS_TRY(conv->enqueue_rows(xs[cur].p, conv_scale, nfc[nc].p, rv0, rv1,
                                   part.conv_sel.p, part.nsel, s));
    else if (conv)
        DNS_TRY(conv->enqueue(xs[cur].p, conv_scale, nfc[nc].p, s));
    const int grid = dns::grid_for_rows(std::max(1, rv1 - rv0), R1.lpr);
    DNS_LPR_SWITCH(
        R1.lpr,
        hipLaunchKernelGGL(dns::k_imex_rhs<L>, grid, dns::kBlock, 0, s,
                           rv1 - rv0, h->np, R1.rowptr.p, R1.colidx.p,
                           R1.vals.p, xs[cur].p,
                           (nsol >= 2) ? xs[prev].p : xs[cur].p, cf->a_c,
                           (nsol >= 2) ? cf->a_p : 0.0, nfc[nc].p, nfc[no].p,
                           cf->cn_c, cf->cn_o, g_ref(), gp_ref(), b.p, rv0,
                           h->nv, rp0, rp1));
    return warm_start(cf, pl);
}

// bandwidth regime: vector part first (StreamRhs: with the convection gather),
// then b_v += R1 xin through the streaming kernel (xin in the solver's scratch
// vector u; StreamRows: this rank's rows, mapped to their global numbers)
int dns_imex::front_stream(const dns_imex_coeffs *cf, const StepPlan &pl) {
    dns_saddle *h = sys;
    hipStream_t s = h->stream;
    const bool own = pl.form == StepPlan::StreamRows;
    if (conv && own)
        DNS_TRY(conv->enqueue_rows(xs[cur].p, conv_scale, nfc[nc].p, h->dd->v0,
                                   h->dd->v1, part.conv_sel.p, part.nsel, s));
    else if (conv)
        DNS_TRY(conv->enqueue_cells(xs[cur].p, s));   // gather: in bvec
    const ConvGather cg = own ? ConvGather{} : conv_gather();
    hipLaunchKernelGGL(dns::k_imex_bvec, dns::grid_for_elems(h->n), dns::kBlock,
                       0, s, h->nv, h->np, xs[cur].p,
                       (nsol >= 2) ? xs[prev].p : xs[cur].p, cf->a_c,
                       (nsol >= 2) ? cf->a_p : 0.0, nfc[nc].p, nfc[no].p,
                       cf->cn_c, cf->cn_o, g_ref(), gp_ref(), b.p, h->u.p,
                       cg.gptr, cg.gidx, cg.cellvals, conv_scale);
    dns::StreamEpi ep = dns::stream_epi_plain(1.0, 1.0, b.p);
    if (R1p.ready) {
        // (the pair format knows its global rows: PairDev::aoff)
        DNS_TRY(dns::launch_pair16x(R1p, h->u.p, b.p, ep, s, nullptr));
    } else {
        if (own) {
            ep.map_on = 1;
            ep.rm = dns::RowMap{h->dd->v0, h->dd->v1 - h->dd->v0, 0, 0};
        }
        DNS_TRY(dns::launch_stream16x<double>(R1, R1.vals.p, h->u.p, b.p, ep, s,
                                              nullptr));
    }
    return warm_start(cf, pl);
}

// Right-hand side and warm start, enqueued in front of the first Krylov cycle
// so that a whole time step is ONE captured graph
int dns_imex::prologue(const dns_imex_coeffs *cf, const StepPlan &pl) {
    // the attachments: the first nodes of the step, whatever its form
    // (xs[cur] is complete: the state after the step before)
    DNS_TRY(launch_front_nodes(sys->stream));
    switch (pl.form) {
        case StepPlan::Six: return front_six(cf, pl);
        case StepPlan::Fused: return front_fused(cf, pl);
        case StepPlan::DistFront: return front_dist(cf, pl);
        case StepPlan::StreamRhs:
        case StepPlan::StreamRows: return front_stream(cf, pl);
        default: return front_rows(cf, pl);
    }
}

// what the solver is handed for the solve of this step
dns::StepHooks dns_imex::hooks(const dns_imex_coeffs *cf, const StepPlan &pl) {
    const int par = work & 1;
    dns::StepHooks hk;
    hk.prologue = [this, cf, pl]() -> int { return prologue(cf, pl); };
    hk.prologue_key = mix64(step_key(cf), {pl.key()});
    hk.resid_nparts = front_nparts(pl);
    hk.prologue_has_resid = hk.resid_nparts > 0;
    hk.stepctr = tables() ? stepctr.p : nullptr;
    // the tail kernels leave the NEXT step's warm start in its work buffer
    // (= this step's p4: not read after this step's front kernel)
    if (pl.can_pre) {
        double en[5];
        dns::extrap_coeffs(std::min(nsol + 1, 5), cf->extrapolate_x0, en);
        hk.tail_extrap = dns::TailExtrap{xs[cur].p, xs[prev].p, xs[pprev].p,
                                         xs[p3].p,  en[0], en[1], en[2],
                                         en[3],     en[4], xs[p4].p};
    }
    if (pl.form == StepPlan::Six) {
        // the cycle starts from x0buf[par], its tail writes the solution into
        // the work buffer, the next warm start into x0buf[1 - par], the new
        // residual into rc6[1 - par] (the next step's `current`)
        hk.tail_extrap.out = x0buf[1 - par].p;
        hk.step6.on = true;
        hk.step6.t6 = dns::Tail6{
            x0buf[par].p, xs[work].p, nullptr, nullptr,
            cf->carry_residual ? rc6[1 - par].p : (double *)nullptr, sys->nv};
        hk.step6.kx = kx6.p;
        if (conv)
            hk.step6.cells = dns::TailCells{
                conv->ncells,
                (8 * conv->ncells + dns::kBlock - 1) / dns::kBlock,
                conv->cellmap.p, conv->glam.p, conv->area.p, conv->dbc_ref(),
                conv->cellvals.p};
    }
    hk.z_plan = pl.zwide ? &part.planX : nullptr;
    hk.carry_rnew = pl.dcarry ? rc6[1 - par].p : nullptr;
    if (pl.dtail) {
        hk.dist_tail.on = true;
        hk.dist_tail.x0copy = x0c.p;
        hk.dist_tail.cells = dns::TailCells{
            conv->ncells, (8 * part.nsel + dns::kBlock - 1) / dns::kBlock,
            conv->cellmap.p, conv->glam.p, conv->area.p, conv->dbc_ref(),
            conv->cellvals.p, part.conv_sel.p, part.nsel};
    }
    return hk;
}

// device convection: the old nfc_c becomes nfc_o, the new one is evaluated
// from the current velocity inside the step's graph, with the Dirichlet row
// the device counter selects (step_device; dns_imex_front_probe)
void dns_imex::turn_convection() {
    if (!conv) return;
    std::swap(nc, no);
    conv->attach_counter(stepctr.p);
}

int dns_imex::step_device(const dns_imex_coeffs *cf, const dns_solve_opts *o,
                          dns_solve_stats *st, bool with_true_residual) {
    dns_saddle *h = sys;
    double *x = xs[work].p;
    turn_convection();
    if (!h->precond_ready)
        return dns::fail(DNS_ERR_NOT_READY, "preconditioner not set up");
    // (a step that has to cut the stepper's row blocks first neither trusts
    // nor leaves a tail's warm start: kept as it is)
    const bool cut = h->dist() && !part.on;
    DNS_TRY(ensure_partition());
    StepPlan pl = plan(cf, o, h->pipeline_c);
    if (cut) pl.can_pre = pl.use_pre = false;
    const bool six = pl.form == StepPlan::Six;
    DNS_TRY(check_attachments());
    if (tables()) {
        if (o->method != DNS_METHOD_GMRES)
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "per-step tables need the GMRES solver");
        if (rows_left() <= 0 && !preparing)
            return dns::fail(DNS_ERR_NOT_READY,
                             "the per-step tables are used up after %d steps: "
                             "upload the next ones (dns_imex_set_rhs_table / "
                             "dns_conv_set_dbc_table / "
                             "dns_imex_set_feedback_table / "
                             "dns_imex_set_recorder / "
                             "dns_imex_set_functionals / dns_imex_set_stats / "
                             "dns_imex_set_quadratics / "
                             "dns_imex_set_ensemble)",
                             tab_pos);
    }
    const int next_nsol = std::min(nsol + 1, 5);
    if (o->method == DNS_METHOD_GMRES) {
        const dns::StepHooks hk = hooks(cf, pl);
        const int grc = h->gmres(b.p, six ? x0buf[work & 1].p : x, o, st, &hk);
        // (the cell values on the device are those of the NEW velocity if
        // the cycle that was enqueued ended in the lazy tail)
        dcells_ok = pl.dtail && hk.dist_tail_ran &&
                    (h->pipeline_c > 0 ||
                     (st->restarts == 0 && st->status == DNS_OK));
        if (dcells_ok) dcells_gen = conv->dbc_gen;
        n_steps_built++;
        n_steps_tail_cells += dcells_ok ? 1 : 0;
        n_steps_cells_reused += pl.have_cells ? 1 : 0;
        if (env_debug) {
            static int said = 0;
            if (said < 6 && h->dist())
                fprintf(stderr, "[dns] partitioned step %d: form %d, cells by "
                        "the tail before %d, tail with cells %d of %d (cycle "
                        "%d)\n", said++, (int)pl.form, (int)pl.have_cells,
                        (int)dcells_ok, (int)pl.dtail, h->pipeline_c);
        }
        pre_ok = false;
        DNS_TRY(grc);
        if (pl.can_pre && !six) {
            pre_ok = true;
            pre_sig = dns::extrap_sig(next_nsol, cf->extrapolate_x0);
        }
        // row-partitioned: the next step's right-hand side, convection and
        // warm start read this rank's rows and their halo
        if (pl.zwide)
            part.state_full = false;
        else if (h->dist())
            DNS_TRY(h->comm->allgatherv(x, h->st_v, h->stream));
    } else {
        pre_ok = false;
        dcells_ok = false;
        DNS_TRY(prologue(cf, pl));
        DNS_TRY(h->bicgstab(b.p, x, o, st));
    }
    if (tables()) tab_pos++;
    if (with_true_residual) {
        double tr = 0.0;
        DNS_TRY(h->true_residual(b.p, x, &tr));
        st->true_relres = st->bnorm > 0 ? tr / st->bnorm : tr;
    }
    rotate();
    steps_enqueued++;
    last_pscale = cf->pscale;
    b_valid = true;
    // a carry step has left K x_c of ITS current solution in the ring: after
    // the rotation kxs[prev..p4] are current again; any other step breaks it
    carry_ok = pl.carry;
    // a six-node step has left the next warm start, the cell values of the new
    // velocity and the new residual behind
    six_ok = six;
    return DNS_OK;
}

// What a six-node step needs from the step before, for the ring as it stands:
// the warm start in x0buf[work & 1], the convection cell values of the current
// velocity, and no carried residual (the steps before converged to the
// tolerance themselves).  Plain launches: never inside a capture.
int dns_imex::prime_six(const dns_imex_coeffs *cf, bool keep_r) {
    dns_saddle *h = sys;
    six_ok = false;
    if (!six_capable() || nsol < 5) return DNS_OK;
    const size_t ld = h->ld;
    if (kx6.n < ld) DNS_TRY(kx6.alloc(ld));
    for (int q = 0; q < 2; ++q) {
        if (x0buf[q].n < ld) DNS_TRY(x0buf[q].alloc(ld));
        bool fresh = false;
        if (rc6[q].n < (size_t)h->nv) {
            DNS_TRY(rc6[q].alloc((size_t)h->nv));
            fresh = true;
        }
        if (!keep_r || fresh) DNS_TRY(rc6[q].zero(h->stream));
    }
    const int m = dns::kMaxRestart;
    if (h->Wcols.n < (size_t)m * ld) {
        DNS_HIP(hipStreamSynchronize(h->stream));
        h->drop_graphs();
        DNS_TRY(h->Wcols.alloc((size_t)m * ld));
    }
    // (nsol == 5 here.  With kExtrapFit35 this launches the QUARTIC, not the
    // least-squares fit the tails write: kept as it is, not yet reconciled)
    double e[5];
    const int order = cf->extrapolate_x0 == dns::kExtrapFit35
                          ? 4 : dns::extrap_coeffs(nsol, cf->extrapolate_x0, e);
    DNS_TRY(dns::enqueue_extrap(order, xs, *this, x0buf[work & 1].p, h->n,
                                h->stream));
    if (conv) {
        conv->attach_counter(stepctr.p);
        DNS_TRY(conv->enqueue_cells(xs[cur].p, h->stream));
        six_conv_gen = conv->dbc_gen;
    }
    six_ok = true;
    return DNS_OK;
}

// K xs[prev..p4] for the ring as it stands (and, `zero_r`, a zero previous
// residual): the next PRE step can then carry its predecessor's residual.
// Plain launches: never inside a capture.
int dns_imex::prime_carry(bool zero_r) {
    dns_saddle *h = sys;
    carry_ok = false;
    if (!b_valid || nsol < 2 || h->dist() || h->streams(h->K)) return DNS_OK;
    for (int q = 0; q < 6; ++q)
        if (kxs[q].n < h->ld) {
            DNS_TRY(kxs[q].alloc(h->ld));
            DNS_TRY(kxs[q].zero(h->stream));
        }
    if (rcarry.n < (size_t)h->nv) {
        DNS_TRY(rcarry.alloc((size_t)h->nv));
        zero_r = true;
    }
    if (zero_r) DNS_TRY(rcarry.zero(h->stream));
    // the step about to run computes K x_c of today's cur itself and reads
    // the products of today's prev, pprev, p3, p4
    const int need[4] = {prev, pprev, p3, p4};
    for (int q = 0; q < 4; ++q)
        DNS_TRY(dns::launch_spmv(h->K, xs[need[q]].p, kxs[need[q]].p, 1.0, 0.0,
                                 nullptr, 0, h->stream));
    carry_ok = true;
    return DNS_OK;
}

// (Re)cut this stepper's own operators when the system's slicing has changed:
// R1 by rows, the convection cells that touch this rank's rows, and the halo
// plan of a solution vector = footprint of the rows of K, of R1 and of those
// cells.  Every rank computes every rank's lists from the replicated host
// patterns (no set-up communication).
int dns_imex::ensure_partition() {
    dns_saddle *h = sys;
    const bool want = h->dist() && h->dist_sliced && h->dd;
    if (!want && r1_rows)
        return dns::fail(DNS_ERR_NOT_READY,
                         "a stepper created from rows of R1 runs on a system "
                         "whose preconditioner has been set up");
    if (!want) {
        if (part.on) {
            const dns_csr v = R1h.view();
            DNS_TRY(R1.upload(&v, h->stream));
            DNS_TRY(build_r1_pair(R1h, 0));
            DNS_HIP(hipStreamSynchronize(h->stream));
            part.on = false;
        }
        return DNS_OK;
    }
    if (part.on && part.gen == h->dist_generation && part.conv_for == conv)
        return DNS_OK;
    // the old halo lists end here: every rank's rows everywhere first (all
    // ranks take this branch together, the state of the handles is replicated)
    DNS_TRY(gather_state());
    const int P = h->comm->nranks, me = h->comm->rank, nv = h->nv;
    const std::vector<int> &stv = h->st_v;
    std::vector<std::vector<std::vector<int>>> need((size_t)P);
    const dns_csr rv = R1h.view();
    std::vector<int> mysel;
    for (int r = 0; r < P; ++r) {
        std::vector<std::vector<int>> a;
        need[r].assign((size_t)P, std::vector<int>());
        // (rows of R1 only: the own lists, exchanged below)
        if (r1_rows && r != me) continue;
        dns::halo_need(&rv, stv[r], stv[r + 1], P, r, stv.data(), nv, a);
        std::vector<std::vector<int>> c((size_t)P);
        if (conv) {
            // cells with a test function on one of the rows of rank r ...
            const int nc_all = conv->ncells;
            std::vector<unsigned char> cm((size_t)nc_all, 0), dm((size_t)nv, 0);
            for (int row = stv[r]; row < stv[r + 1]; ++row)
                for (int k = conv->gptr_host[row]; k < conv->gptr_host[row + 1];
                     ++k)
                    cm[conv->gidx_host[k] % nc_all] = 1;
            // ... read all their dofs
            for (int cl = 0; cl < nc_all; ++cl) {
                if (!cm[cl]) continue;
                if (r == me) mysel.push_back(cl);
                for (int k = 0; k < 12; ++k) {
                    const int m = conv->cmap_host[(size_t)k * nc_all + cl];
                    if (m >= 0) dm[m] = 1;
                }
            }
            for (int q = 0; q < P; ++q) {
                if (q == r) continue;
                for (int d = stv[q]; d < stv[q + 1]; ++d)
                    if (dm[d]) c[q].push_back(d);
            }
        }
        need[r].assign((size_t)P, std::vector<int>());
        for (int q = 0; q < P; ++q) {
            std::vector<int> m1, &out = need[r][q];
            const std::vector<int> &kq = h->dd->needK[r][q];
            std::set_union(a[q].begin(), a[q].end(), kq.begin(), kq.end(),
                           std::back_inserter(m1));
            std::set_union(m1.begin(), m1.end(), c[q].begin(), c[q].end(),
                           std::back_inserter(out));
        }
    }
    if (r1_rows) {
        const std::vector<std::vector<int>> mine = need[me];
        DNS_TRY(h->gather_need_lists(mine, need));
    }
    DNS_TRY(part.planX.build(need, me, P, h->stream));
    {
        const dns::HostCsr rl = host_row_slice(R1h, stv[me], stv[me + 1]);
        const dns_csr v = rl.view();
        DNS_TRY(R1.upload(&v, h->stream));
        DNS_TRY(build_r1_pair(rl, stv[me]));
    }
    for (int q = 0; q < 2; ++q)
        if (rc6[q].n < (size_t)nv) {
            DNS_TRY(rc6[q].alloc((size_t)nv));
            DNS_TRY(rc6[q].zero(h->stream));
        }
    if (x0c.n < h->ld) DNS_TRY(x0c.alloc(h->ld));
    dcells_ok = false;                  // (another selection of cells)
    part.nsel = (int)mysel.size();
    DNS_TRY(part.conv_sel.alloc((size_t)std::max(1, part.nsel)));
    if (part.nsel)
        DNS_TRY(part.conv_sel.upload(mysel.data(), mysel.size(), h->stream));
    DNS_HIP(hipStreamSynchronize(h->stream));
    part.on = true;
    part.gen = h->dist_generation;
    part.conv_for = conv;
    return DNS_OK;
}

// every rank's rows of the current solution on every rank (a collective: all
// ranks call it together -- dns_imex_get_state, dns_imex_vnorm do)
int dns_imex::gather_state() {
    dns_saddle *h = sys;
    if (part.state_full || !h->dist()) return DNS_OK;
    DNS_TRY(h->comm->allgatherv(xs[cur].p, h->st_v, h->stream));
    part.state_full = true;
    return DNS_OK;
}

int dns_imex::sync_counter() {
    return stepctr.upload(&tab_pos, 1, sys->stream);
}

// everything a captured group of `group` steps depends on
std::vector<uint64_t> dns_imex::group_key(const dns_imex_coeffs *cf,
                                          const dns_solve_opts *o,
                                          int group) const {
    const dns_saddle *h = sys;
    return {9u, step_key(cf), kw(h->pipeline_c), kw(o->reorth), kw(o->maxiter),
            kw(o->rtol), kw(o->atol), kw(h->popts.cheb_degree),
            kw(h->popts.schur), kw(h->fhat_explicit), kw(group),
            kw(o->restart), kw(h->step6_lazy)};
}

// `group` pipelined steps as ONE graph (sys->pipeline_c = cycle length must be
// set).  launch == false: capture + instantiate only; the host's view of the
// ring is advanced either way.
int dns_imex::enqueue_group(const dns_imex_coeffs *cf, const dns_solve_opts *o,
                            int group, bool launch) {
    dns_saddle *h = sys;
    dns_solve_stats dummy;
    const long before = steps_enqueued;
    DNS_TRY(h->run_cached(group_key(cf, o, group), true, [&]() -> int {
        for (int g = 0; g < group; ++g)
            DNS_TRY(step_device(cf, o, &dummy, false));
        return DNS_OK;
    }, launch));
    if (steps_enqueued == before) {
        // the graph existed: move the host's view of the ring along
        for (int g = 0; g < group; ++g) {
            if (conv) std::swap(nc, no);
            rotate();
        }
        // (replayed steps are fused GMRES steps: they leave a warm start)
        pre_ok = true;
        pre_sig = dns::extrap_sig(nsol, cf->extrapolate_x0);
        steps_enqueued += group;
        if (tables()) tab_pos += group;
        last_pscale = cf->pscale;
        b_valid = true;       // (carry_ok is part of the key: it stays as is)
        if (six_ok) pre_ok = false;   // (six-node steps leave x0 elsewhere)
        // (the tails of the replayed steps were the captured ones': they left
        // the cell values of the new velocity iff such a step would now)
        dcells_ok = plan(cf, o, h->pipeline_c).dtail;
        if (dcells_ok) dcells_gen = conv->dbc_gen;
        // (partitioned: a replayed step leaves own rows + halo, like a
        // launched one)
        if (sys->dist() && part.on) part.state_full = false;
    }
    return DNS_OK;
}

// Capture every graph the batches can ask for -- six ring states x (group of
// env_group steps, single step) x the cycle lengths around the prediction --
// BEFORE the batches start, so that no dns_imex_run ever captures inside its
// stepping loop.  Nothing is launched; the host state is restored.
int dns_imex::prepare_graphs(const dns_imex_coeffs *cf,
                             const dns_solve_opts *o) {
    dns_saddle *h = sys;
    DNS_TRY(h->ensure_solver_buffers(o));    // no allocation inside a capture
    // (the ring positions are not part of the signature: all six are captured)
    // (step6_lazy: the kind of the c = 1 cycle)
    uint64_t sig = mix64(config_key(cf),
                         {kw(h->graph_generation), kw(o->rtol), kw(o->atol),
                          kw(o->reorth), kw(o->maxiter), kw(o->restart),
                          kw(h->step6_lazy)});
    const int m = std::max(1, std::min(o->restart, dns::kMaxRestart));
    // (hysteresis: a prediction that moves between 3 and 4 Krylov steps -- the
    // bandwidth regime -- must not capture all ~80 graphs of a run again every
    // time it comes down by one; a prediction that has come down for good --
    // the long cycles of a start-up transient -- is followed, or the graphs of
    // cycle lengths nobody asks for any more crowd the cache)
    const int needed = std::min(m, std::max(4, policy.cpred + 1));
    if (needed > chi_hi)
        chi_hi = needed;
    else if (needed < chi_hi - 1)
        chi_hi = needed + 1;
    const int chi = chi_hi;
    sig = mix64(sig, {kw(chi)});
    if (sig == prepared_sig) return DNS_OK;
    prepare_attempted = true;
    const int big = group_for(1 << 30);
    const HostState s0 = host_state();
    // (on every exit: no cycle length set, the ring as it was)
    dns::ScopeExit reset([&] {
        h->pipeline_c = 0;
        set_host_state(s0);
        preparing = false;
    });
    preparing = true;          // (captures only: the tables are not consumed)
    for (int c = 1; c <= chi; ++c) {
        h->pipeline_c = c;
        set_host_state(s0);
        for (int r = 0; r < (s0.ring.pre_ok ? 6 : 7); ++r) {
            for (int gsz : {big, group_for(big / 2)}) {
                if (gsz <= 1) continue;
                const HostState sr = host_state();
                const int rc = enqueue_group(cf, o, gsz, false);
                set_host_state(sr);
                DNS_TRY(rc);
            }
            DNS_TRY(enqueue_group(cf, o, 1, false));   // advances by one
        }
    }
    prepared_sig = sig;
    return DNS_OK;
}

// one dns_imex_run call: what its pieces share
struct ImexRun {
    dns_imex *st;
    dns_saddle *h;
    const dns_imex_coeffs *cf;
    int nsteps;
    dns_solve_stats *sp;
    dns_solve_opts o, osync;       // batches / synchronous steps
    int k = 0;                     // steps done
    int64_t iters = 0;
    bool pipelined = false;
    bool fin_batch = false;        // the last batch carried the closing event
    int sync_steps(int count);
    int enter_pipeline();
    int run_batch();
    int finish_run(double *device_seconds, int64_t *total_iters);
};

// synchronous steps (plain launches, the host waits for every solve): the
// start-up steps that establish the extrapolation history and the iteration
// count, the non-pipelined configurations, and the last resort after a batch
// that failed twice
int ImexRun::sync_steps(int count) {
    for (int q = 0; q < count && k < nsteps; ++q, ++k) {
        DNS_TRY(st->step_device(cf, &osync, sp, false));
        iters += sp->iters;
        if (sp->status == DNS_NOT_CONVERGED) {
            if (st->run_unconverged++ == 0) st->run_first_bad = k;
        } else if (sp->status != DNS_OK) {
            return sp->status;
        }
    }
    return DNS_OK;
}

// from the start-up steps to the batches: what the captured steps expect to
// find primed, the partition, and every graph the batches can ask for
int ImexRun::enter_pipeline() {
    if (st->six_ok && st->conv && st->six_conv_gen != st->conv->dbc_gen)
        st->six_ok = false;       // boundary values changed in between
    if (!st->six_ok) DNS_TRY(st->prime_six(cf, false));
    if (!st->six_ok && cf->carry_residual && !st->carry_ok)
        DNS_TRY(st->prime_carry(true));
    DNS_HIP(hipEventRecord(st->e1, h->stream));
    // (the stepper's row blocks and halo plan: host work and collectives
    // that must not land inside a capture)
    DNS_TRY(st->ensure_partition());
    // (cell values a step of the run before has left are kept)
    if (!(st->dcells_ok && st->conv && st->dcells_gen == st->conv->dbc_gen))
        DNS_TRY(st->prime_dcells(cf, &o));
    st->prepare_attempted = false;
    int prc = st->prepare_graphs(cf, &o);
    if (h->dist() && st->prepare_attempted) {
        // a capture can fail on ONE rank only (instantiation out of memory,
        // an invalidated capture): replayed one-step cycles and plain
        // synchronous steps issue different collective sequences, so the
        // ranks agree on the branch before they take it -- whoever captured
        // asks (the signatures, hence the decision to capture, are the same
        // on every rank)
        bool any = false;
        DNS_TRY(h->all_ranks_any(prc != DNS_OK, &any));
        if (any && prc == DNS_OK)
            prc = dns::fail(DNS_ERR_COMM, "graph capture failed on another "
                            "rank");
    }
    if (prc == DNS_OK || !h->dist()) return prc;
    // a capture with collectives did not go through on this communicator:
    // plain launches from here on, on every rank
    if (st->env_debug)
        fprintf(stderr, "[dns] graph capture of the partitioned step failed "
                "(%s): plain launches\n", dns_last_error());
    h->dist_graph_ok = false;
    h->drop_graphs();
    pipelined = false;
    osync.use_graph = 0;
    return sync_steps(nsteps - k);
}

// pipelined batches: every group of steps is ONE graph launch and nobody
// waits; the device accumulates iteration counts and failures, the host
// looks once per batch.  A batch in which some solve needed more Krylov
// steps than predicted is restored from the checkpoint of the ring and
// repeated with a longer cycle (once), then synchronously.
int ImexRun::run_batch() {
    dns::BatchPolicy &pol = st->policy;
    const int nb = std::min(pol.batch_len, nsteps - k);
    const bool sixing = st->six_ok;
    // (partitioned stepper: its carried residuals live in the same buffers)
    const bool dcar = h->dist() && st->part.on && cf->carry_residual != 0 &&
                      st->rc6[0].p && st->rc6[1].p;
    const bool carrying = cf->carry_residual != 0 && st->carry_ok;
    dns::Checkpoint &ck = st->ck;        // (saved by the first attempt)
    ck.clear();
    for (int q : {st->cur, st->prev, st->pprev, st->p3, st->p4, st->work})
        DNS_TRY(ck.add(st->xs[q].p, h->ld));
    if (st->conv)
        for (int q = 0; q < 2; ++q) DNS_TRY(ck.add(st->nfc[q].p, h->nv));
    if ((sixing || dcar) && cf->carry_residual)
        for (int q = 0; q < 2; ++q) DNS_TRY(ck.add(st->rc6[q].p, h->nv));
    if (carrying) {
        DNS_TRY(ck.add(st->b.p, h->ld));
        DNS_TRY(ck.add(st->rcarry.p, h->nv));
    }
    // observer feedback: both slots of the state and the right-hand side it
    // left (the slot, the drift row and the log row come back with the step
    // counter; the log rows of a discarded batch are overwritten)
    if (st->fb) {
        DNS_TRY(ck.add(st->fb->state.p, (size_t)2 * st->fb->stride()));
        // (boundary feedback: gpeff lies behind geff)
        DNS_TRY(ck.add(st->fb->geff.p,
                       (size_t)h->nv + (st->fb->rhs_p() ? (size_t)h->np : 0)));
    }
    // flow statistics: the sums AND the workgroups' marks -- a restored batch
    // adds its rows again, to the sums the batch started from (a checkpoint
    // of their own: the list above can be full)
    dns::Checkpoint &cks = st->ck_st;
    cks.clear();
    if (st->stat)
        DNS_TRY(cks.add(st->stat->acc.p, st->stat->lay.total()));
    const dns_imex::HostState hs0 = st->host_state();
    // back to the checkpoint, then what derives from it: K x products of the
    // ring, device step counter, cell values (not in the ring), the six-node
    // warm start and cell values (the counter is back at the first step)
    auto restore = [&]() -> int {
        DNS_TRY(ck.restore(h->stream));
        if (st->stat) DNS_TRY(cks.restore(h->stream));
        st->set_host_state(hs0);
        if (carrying) DNS_TRY(st->prime_carry(false));
        if (st->tables()) DNS_TRY(st->sync_counter());
        DNS_TRY(st->prime_dcells(cf, &o));
        if (sixing) DNS_TRY(st->prime_six(cf, true));
        return DNS_OK;
    };
    // oversolve (see DnsCtl::stop_frac): general cycles with the multigrid
    // Schur block -- not the six-node step (its tail keeps no record of the
    // columns a solve needed; it runs one column anyway)
    const bool over = h->oversolve && !sixing;
    const int cmax = std::max(1, std::min(o.restart, dns::kMaxRestart));
    const int c_first = pol.cycle(over);
    int c = std::min(c_first, cmax);
    const dns::CtlHeaderAcc *ha = h->hdr_host.p;
    bool batch_ok = false, replayed = false;
    for (int attempt = 0; attempt < 2 && !batch_ok; ++attempt) {
        if (attempt == 1) {
            // restore the ring and try once more with a longer cycle
            DNS_TRY(restore());
            c = dns::BatchPolicy::longer(c, cmax);
            st->run_replayed += nb;
            replayed = true;
        }
        DNS_TRY(ck.save(h->stream, h->ctl.p, over ? h->oversolve_frac : 0.0,
                        attempt == 0));
        if (st->stat && attempt == 0) DNS_TRY(cks.save(h->stream));
        h->pipeline_c = c;
        for (int q = 0, g = 0; q < nb; q += g) {
            g = st->group_for(nb - q);
            DNS_TRY(st->enqueue_group(cf, &o, g, true));
        }
        h->pipeline_c = 0;
        // the call's last batch: the closing event and the true residual of
        // the last step (for the record) ride behind it, so that ONE
        // synchronisation -- the header's -- ends the call
        fin_batch = k + nb >= nsteps && !h->dist();
        if (fin_batch) {
            // (the last rows: nobody runs a prologue behind it)
            DNS_TRY(st->launch_closing_nodes(h->stream));
            DNS_HIP(hipEventRecord(st->e1, h->stream));
            DNS_TRY(h->resid_norm_csr(h->gridS, st->xs[st->cur].p, st->b.p,
                                      nullptr, dns::RowMap{0, h->n, 0, 0}));
            hipLaunchKernelGGL(dns::k_sum_partials, 1, dns::kBlock, 0,
                               h->stream, h->partR.p, h->gridS, h->scal.p);
            DNS_TRY(dns::d2h_pinned(h->scal_host.p, h->scal.p, 1, h->stream));
        }
        DNS_TRY(h->read_header());
        if (st->env_debug)
            fprintf(stderr,
                    "[dns] batch at step %d (%d steps, attempt %d): c=%d "
                    "solves=%d fail=%d iters=%d maxit=%d maxrel=%.2e "
                    "need=%d prev=%.2e r0(last)=%.2e status=%d\n",
                    k, nb, attempt, c, ha->acc_solves, ha->acc_fail,
                    ha->acc_iters, ha->acc_maxit, ha->acc_maxrel,
                    ha->acc_maxneed, ha->acc_maxprev,
                    ha->h.tol > 0 ? ha->h.beta / ha->h.tol : 0.0,
                    ha->h.status);
        if (ha->h.status == dns::kGsFallback) o.reorth = osync.reorth = 0;
        batch_ok = ha->acc_fail == 0 && ha->h.status == DNS_OK;
        if (!batch_ok) fin_batch = false;
    }
    if (!batch_ok) {
        // last resort: the batch step by step from the checkpoint
        if (over) DNS_TRY(h->set_stop_frac(0.0));
        DNS_TRY(restore());
        st->run_replayed += nb;
        const int rc = sync_steps(nb);
        if (rc == DNS_OK) DNS_TRY(st->prime_six(cf, false));
        if (!st->six_ok && cf->carry_residual && rc == DNS_OK)
            DNS_TRY(st->prime_carry(true));
        pol.after_fallback(h->last_iters);
        return rc;
    }
    k += nb;
    iters += ha->acc_iters;
    if (sixing)
        (h->step6_lazy_for(c) ? st->run_lazy_steps : st->run_eager_steps) += nb;
    pol.after_batch({over, c_first, c, replayed, ha->acc_maxit, ha->acc_maxrel,
                     ha->acc_maxprev},
                    {h->oversolve_cmin_eff(), h->oversolve_raise,
                     h->oversolve_lower, h->mg_two_for(1) && !h->mg_two_for(2),
                     st->env_slack_adapt, st->env_noslack_maxrel});
    h->last_iters = ha->h.total_it;
    sp->iters = ha->h.total_it;
    sp->status = ha->h.conv ? DNS_OK : DNS_NOT_CONVERGED;
    sp->bnorm = ha->h.bnorm;
    sp->est_relres =
        ha->h.bnorm > 0 ? ha->h.resnorm / ha->h.bnorm : ha->h.resnorm;
    return DNS_OK;
}

// the closing event, the true residual of the last step, the timing and the
// report of steps that ended unconverged
int ImexRun::finish_run(double *device_seconds, int64_t *total_iters) {
    if (fin_batch) {
        // (event and residual were enqueued behind the last batch and have
        // arrived with its header)
        const double tr = std::sqrt(h->scal_host.p[0]);
        sp->true_relres = sp->bnorm > 0 ? tr / sp->bnorm : tr;
        h->spmv_count++;
    } else {
        if (nsteps > 0) DNS_TRY(st->launch_closing_nodes(h->stream));
        DNS_HIP(hipEventRecord(st->e1, h->stream));
        // true residual of the last step for the record: behind the closing
        // event (not part of the stepping time), ONE synchronisation for both
        if (nsteps > 0) {
            double tr = 0.0;
            DNS_TRY(h->true_residual(st->b.p, st->xs[st->cur].p, &tr));
            sp->true_relres = sp->bnorm > 0 ? tr / sp->bnorm : tr;
        } else {
            DNS_HIP(hipEventSynchronize(st->e1));
        }
    }
    float ms = 0.f;
    DNS_HIP(hipEventElapsedTime(&ms, st->e0, st->e1));
    if (device_seconds) *device_seconds = 1e-3 * ms;
    if (total_iters) *total_iters = iters;
    if (st->run_unconverged > 0) {
        sp->status = DNS_NOT_CONVERGED;
        return dns::fail(DNS_NOT_CONVERGED,
                         "%d of %d time steps ended at maxiter without reaching "
                         "the tolerance (first: step %d of this run); the state "
                         "was advanced with the best iterates",
                         st->run_unconverged, nsteps, st->run_first_bad);
    }
    return DNS_OK;
}

int dns_imex::refuse_probed() const {
    if (!probed) return DNS_OK;
    return dns::fail(DNS_ERR_NOT_READY,
                     "dns_imex_front_probe has run the front of a step without "
                     "its solve: dns_imex_set_state before the stepper steps "
                     "again");
}

// what dns_imex_step refuses before anything is touched
int dns_imex::step_refusals(const double *nfc_new) const {
    if (nfc_new && conv)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "a device convection operator is attached: the "
                         "convection vector must not be supplied by the host");
    // (refused before the convection history is touched: the stepper stays
    // as it was)
    if (tables() && rows_left() < 1)
        return dns::fail(DNS_ERR_NOT_READY,
                         "the per-step tables are used up after %d steps: "
                         "upload the next ones (dns_imex_set_rhs_table / ... / "
                         "dns_imex_set_functionals / dns_imex_set_quadratics)",
                         tab_pos);
    return check_attachments();
}

int dns_imex::step_preamble(const double *nfc_new, const dns_imex_coeffs *cf,
                            const dns_solve_opts &o) {
    dns_saddle *h = sys;
    DNS_TRY(step_refusals(nfc_new));
    if (nfc_new) {
        std::swap(nc, no);
        DNS_TRY(nfc[nc].upload(nfc_new, (size_t)h->nv, h->stream));
    }
    if (cf->carry_residual && !carry_ok && pre_ok && nsol >= 5 &&
        o.method == DNS_METHOD_GMRES)
        DNS_TRY(prime_carry(true));
    return DNS_OK;
}

extern "C" {

// both creates: `r1` is all of R1, or with `by_rows` this rank's rows of it
static int build_imex(dns_saddle *sys, const dns_csr *r1, dns_imex **out,
                      bool by_rows) {
    if (!sys || !out) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    *out = nullptr;
    DNS_TRY(dns::check_csr(r1, "R1"));
    int row0 = 0;
    if (by_rows) {
        // this rank's rows of R1 (a system created from rows)
        if (!sys->rank_local || !sys->comm)
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "rows of R1 need a system created from rows");
        row0 = sys->st_v[sys->comm->rank];
        const int row1 = sys->st_v[sys->comm->rank + 1];
        if (r1->nrows != row1 - row0 || r1->ncols != sys->nv)
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "rank %d holds rows [%d, %d) of R1 (%d columns)",
                             sys->comm->rank, row0, row1, sys->nv);
    } else if (r1->nrows != sys->nv || r1->ncols != sys->nv)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "R1 must be NV x NV");
    DNS_HIP(hipSetDevice(sys->device));
    auto st = std::make_unique<dns_imex>();
    st->sys = sys;
    st->env_step_history = getenv("DNS_STEP_HISTORY") != nullptr;
    st->env_debug = getenv("DNS_DEBUG") != nullptr;
    if (const char *senv = getenv("DNS_SLACK_ADAPT"))
        st->env_slack_adapt = senv[0] != '0';
    if (const char *nenv = getenv("DNS_NOSLACK_MAXREL"))
        st->env_noslack_maxrel = atof(nenv);
    if (const char *senv = getenv("DNS_STEP6")) st->env_six = senv[0] != '0';
    if (const char *senv = getenv("DNS_DIST_FRONT"))
        st->env_dfront = senv[0] != '0';
    if (const char *senv = getenv("DNS_DIST_TAIL"))
        st->env_dtail = senv[0] != '0';
    if (const char *genv = getenv("DNS_STEP_GROUP"))
        st->env_group = std::max(1, atoi(genv));
    st->r1_rows = by_rows;
    if (by_rows) {
        // (uploaded by ensure_partition, as every row block is)
        st->R1h = dns::host_embed_rows(r1, row0, sys->nv);
    } else {
        DNS_TRY(st->R1.upload(r1, sys->stream));
        st->R1h = dns::host_copy(r1);
        DNS_TRY(st->build_r1_pair(st->R1h, 0));
    }
    for (int i = 0; i < 6; ++i) {
        DNS_TRY(st->xs[i].alloc(sys->ld));
        DNS_TRY(st->xs[i].zero(sys->stream));
    }
    for (int i = 0; i < 2; ++i) {
        DNS_TRY(st->nfc[i].alloc((size_t)sys->nv));
        DNS_TRY(st->nfc[i].zero(sys->stream));
    }
    DNS_TRY(st->g.alloc((size_t)sys->nv));
    DNS_TRY(st->gp.alloc((size_t)sys->np));
    DNS_TRY(st->b.alloc(sys->ld));
    DNS_TRY(st->stepctr.alloc(1));
    DNS_TRY(st->stepctr.zero(sys->stream));
    DNS_TRY(st->g.zero(sys->stream));
    DNS_TRY(st->gp.zero(sys->stream));
    if (hipEventCreate(&st->e0) != hipSuccess)
        return dns::fail(DNS_ERR_HIP, "hipEventCreate failed");
    if (hipEventCreate(&st->e1) != hipSuccess)
        return dns::fail(DNS_ERR_HIP, "hipEventCreate failed");
    if (hipStreamSynchronize(sys->stream) != hipSuccess)
        return dns::fail(DNS_ERR_HIP, "stream sync failed");
    *out = st.release();
    return DNS_OK;
}

int dns_imex_create(dns_saddle *sys, const dns_csr *r1, dns_imex **out) try {
    return build_imex(sys, r1, out, false);
} DNS_CAPI_CATCH

int dns_imex_create_rows(dns_saddle *sys, const dns_csr *r1_rows,
                         dns_imex **out) try {
    return build_imex(sys, r1_rows, out, true);
} DNS_CAPI_CATCH

void dns_imex_destroy(dns_imex *st) {
    if (!st) return;
    (void)hipSetDevice(st->sys->device);
    (void)hipStreamSynchronize(st->sys->stream);
    delete st;
}

int dns_imex_set_state(dns_imex *st, const double *v_c, const double *v_p,
                       const double *ptilde_c, const double *nfc_c,
                       const double *nfc_o) try {
    if (!st || !v_c) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = st->sys;
    DNS_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    st->reset(1);
    for (int i = 0; i < 6; ++i) DNS_TRY(st->xs[i].zero(s));
    DNS_TRY(st->xs[0].upload(v_c, (size_t)h->nv, s));
    if (ptilde_c)
        DNS_TRY(dns::upload_to(st->xs[0].p + h->nv, ptilde_c, (size_t)h->np,
                               s));
    for (int q = 0; q < 2; ++q)
        if (st->rc6[q].p) DNS_TRY(st->rc6[q].zero(s));   // a new trajectory
    st->b_valid = false;
    st->carry_ok = false;
    st->six_ok = false;
    st->dcells_ok = false;
    st->probed = false;
    st->part.state_full = true;
    if (v_p) {
        DNS_TRY(st->xs[1].upload(v_p, (size_t)h->nv, s));
        st->nsol = 2;
    }
    st->nc = 0;
    st->no = 1;
    if (nfc_c)
        DNS_TRY(st->nfc[0].upload(nfc_c, (size_t)h->nv, s));
    else
        DNS_TRY(st->nfc[0].zero(s));
    if (nfc_o)
        DNS_TRY(st->nfc[1].upload(nfc_o, (size_t)h->nv, s));
    else
        DNS_TRY(st->nfc[1].zero(s));
    DNS_HIP(hipStreamSynchronize(s));
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_imex_set_rhs(dns_imex *st, const double *gvec,
                     const double *rhs_p) try {
    if (!st) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = st->sys;
    DNS_HIP(hipSetDevice(h->device));
    if (gvec) DNS_TRY(st->g.upload(gvec, (size_t)h->nv, h->stream));
    if (rhs_p) DNS_TRY(st->gp.upload(rhs_p, (size_t)h->np, h->stream));
    DNS_HIP(hipStreamSynchronize(h->stream));
    st->tab_rows = 0;                 // constant vectors from here on
    st->tab_v = st->tab_p = false;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_imex_set_rhs_table(dns_imex *st, int32_t nsteps, const double *gv,
                           const double *gp) try {
    if (!st || nsteps < 1 || (!gv && !gp))
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    dns_saddle *h = st->sys;
    DNS_HIP(hipSetDevice(h->device));
    DNS_HIP(hipStreamSynchronize(h->stream));   // replays may still read it
    const size_t nv = (size_t)h->nv, np = (size_t)std::max(1, h->np);
    if (gv) {
        if (st->gtab.n < nv * nsteps) DNS_TRY(st->gtab.alloc(nv * nsteps));
        DNS_TRY(st->gtab.upload(gv, nv * nsteps, h->stream));
    }
    if (gp) {
        if (st->gptab.n < np * nsteps) DNS_TRY(st->gptab.alloc(np * nsteps));
        DNS_TRY(st->gptab.upload(gp, (size_t)h->np * nsteps, h->stream));
    }
    st->tab_v = gv != nullptr;
    st->tab_p = gp != nullptr;
    st->tab_rows = nsteps;
    return st->rewind_tables();
} DNS_CAPI_CATCH

int dns_imex_table_position(dns_imex *st, int32_t *pos, int32_t *left) try {
    if (!st) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    if (pos) *pos = st->tab_pos;
    if (left) *left = st->tables() ? st->rows_left() : -1;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_imex_step(dns_imex *st, const double *nfc_new,
                  const dns_imex_coeffs *cf, const dns_solve_opts *opts,
                  dns_solve_stats *stats) try {
    if (!st || !cf) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = st->sys;
    DNS_HIP(hipSetDevice(h->device));
    dns_solve_opts o;
    if (opts)
        o = *opts;
    else
        dns_default_solve_opts(&o);
    dns_solve_stats local;
    dns_solve_stats *sp = stats ? stats : &local;
    memset(sp, 0, sizeof(*sp));
    DNS_TRY(st->refuse_probed());
    DNS_TRY(st->adopt_base_rows());
    DNS_TRY(st->step_preamble(nfc_new, cf, o));
    // nobody reads the history per time step (scripts/extrap_probe.py does)
    h->want_history = st->env_step_history;
    const int src = st->step_device(cf, &o, sp, true);
    h->want_history = true;
    if (src != DNS_OK) return src;
    DNS_TRY(st->launch_closing_nodes(h->stream));       // the row of this step
    DNS_HIP(hipStreamSynchronize(h->stream));
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_imex_run(dns_imex *st, int32_t nsteps, const dns_imex_coeffs *cf,
                 const dns_solve_opts *opts, dns_solve_stats *last_stats,
                 double *device_seconds, int64_t *total_iters) try {
    if (!st || !cf || nsteps < 0)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    dns_saddle *h = st->sys;
    DNS_HIP(hipSetDevice(h->device));
    dns_solve_opts o;
    if (opts)
        o = *opts;
    else
        dns_default_solve_opts(&o);
    dns_solve_stats local;
    ImexRun r{st, h, cf, nsteps, last_stats ? last_stats : &local, o, o};
    memset(r.sp, 0, sizeof(*r.sp));
    DNS_TRY(st->refuse_probed());
    DNS_TRY(st->adopt_base_rows());
    if (st->tables() && st->rows_left() < nsteps)
        return dns::fail(DNS_ERR_NOT_READY,
                         "%d steps asked for, the per-step tables hold %d more "
                         "(dns_imex_set_rhs_table / ... / "
                         "dns_imex_set_functionals / dns_imex_set_quadratics)",
                         (int)nsteps, st->rows_left());
    // (what a step would refuse on behalf of its attachments, before anything
    // is touched or captured)
    DNS_TRY(st->check_attachments());
    // the run's settings of the system, undone on every exit (the status of
    // the oversolve reset is ignored: the first error is the one reported)
    bool over = false;
    dns::ScopeExit reset([&] {
        h->want_history = true;
        h->pipeline_c = 0;
        if (over) (void)h->set_stop_frac(0.0);
    });
    h->want_history = false;
    st->run_unconverged = 0;
    st->run_first_bad = -1;
    st->run_replayed = 0;
    st->run_lazy_steps = st->run_eager_steps = 0;
    const int64_t captures0 = h->graph_captures;
    r.pipelined = r.o.method == DNS_METHOD_GMRES && r.o.use_graph != 0 &&
                  h->graph_capable();
    if (r.pipelined) r.osync.use_graph = 0;
    int rc = DNS_OK;
    if (!r.pipelined) {
        rc = r.sync_steps(nsteps);
    } else {
        // a fresh stepper does its first steps one by one
        const int need = st->policy.startup_steps(st->nsol);
        if (need > 0) {
            rc = r.sync_steps(need);
            st->policy.after_startup(h->last_iters);
        }
        if (rc == DNS_OK && r.k < nsteps) rc = r.enter_pipeline();
    }
    over = h->oversolve && r.pipelined;
    if (rc == DNS_OK) DNS_HIP(hipEventRecord(st->e0, h->stream));
    while (rc == DNS_OK && r.pipelined && r.k < nsteps) rc = r.run_batch();
    st->run_captures = (int)(h->graph_captures - captures0);
    if (rc != DNS_OK && rc != DNS_NOT_CONVERGED) return rc;
    return r.finish_run(device_seconds, total_iters);
} DNS_CAPI_CATCH

int dns_imex_step_counters(dns_imex *st, int64_t *out3) try {
    if (!st || !out3) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    out3[0] = st->n_steps_built;
    out3[1] = st->n_steps_tail_cells;
    out3[2] = st->n_steps_cells_reused;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_imex_run_info(dns_imex *st, int32_t *unconverged, int32_t *first_bad,
                      int32_t *replayed, int32_t *captures) try {
    if (!st) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    if (unconverged) *unconverged = st->run_unconverged;
    if (first_bad) *first_bad = st->run_first_bad;
    if (replayed) *replayed = st->run_replayed;
    if (captures) *captures = st->run_captures;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_imex_run_cycles(dns_imex *st, int64_t *out2) try {
    if (!st || !out2) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    out2[0] = st->run_lazy_steps;
    out2[1] = st->run_eager_steps;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_imex_get_state(dns_imex *st, double *v, double *p) try {
    if (!st) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = st->sys;
    DNS_HIP(hipSetDevice(h->device));
    DNS_TRY(st->gather_state());
    if (v) DNS_TRY(st->xs[st->cur].download(v, (size_t)h->nv, h->stream));
    if (p)
        DNS_TRY(dns::download_from(p, st->xs[st->cur].p + h->nv,
                                   (size_t)h->np, h->stream));
    DNS_HIP(hipStreamSynchronize(h->stream));
    if (p)
        for (int i = 0; i < h->np; ++i) p[i] *= st->last_pscale;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_imex_vnorm(dns_imex *st, double *out) try {
    if (!st || !out) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = st->sys;
    DNS_HIP(hipSetDevice(h->device));
    double s2 = 0.0;
    DNS_TRY(st->gather_state());
    DNS_TRY(h->dot_host(h->nv, st->xs[st->cur].p, st->xs[st->cur].p, &s2));
    *out = std::sqrt(s2);
    return DNS_OK;
} DNS_CAPI_CATCH

// TEST ONLY: the front of a step -- what dns_imex_step does before
// step_device (step_preamble), then what step_device does before its solve
// (the stepper's row blocks, the turn of a device convection, the plan), then
// the member function prologue() would pick for the plan (front_six /
// front_fused / front_dist / front_rows / front_stream), without the
// attachments' nodes and without a solve -- with a copy out of what the front
// reads before it runs and of what it has left.  The stepper is consumed.  On a
// row-partitioned handle the call is COLLECTIVE (gather_state may all-gather).
int dns_imex_front_probe(dns_imex *st, const dns_imex_coeffs *cf,
                         const dns_solve_opts *opts, int32_t cycle_len,
                         const double *nfc_new, dns_imex_probe *out) try {
    if (!st || !cf || !out || cycle_len < 0 || out->parts_cap < 0)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    dns_saddle *h = st->sys;
    if (st->attachments().n > 0)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "the front probe takes a stepper without attachments "
                         "(feedback, recorder, functionals, statistics, "
                         "quadratics, ensemble)");
    if (h->pipeline_c > 0 || st->preparing)
        return dns::fail(DNS_ERR_NOT_READY,
                         "the front probe: a pipelined batch is pending");
    DNS_TRY(st->refuse_probed());
    if (!h->precond_ready)
        return dns::fail(DNS_ERR_NOT_READY, "preconditioner not set up");
    DNS_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    dns_solve_opts o;
    if (opts)
        o = *opts;
    else
        dns_default_solve_opts(&o);
    // (the refusals of the step itself; from the first touch on the stepper
    // counts as consumed, whatever fails behind)
    DNS_TRY(st->step_refusals(nfc_new));
    st->probed = true;
    DNS_TRY(st->step_preamble(nfc_new, cf, o));
    // (from here on as step_device: the stepper's own row blocks -- a step
    // that has to cut them first trusts no tail's warm start --, the turn of a
    // device convection, the plan)
    const bool cut = h->dist() && !st->part.on;
    DNS_TRY(st->ensure_partition());
    st->turn_convection();
    StepPlan pl = st->plan(cf, &o, cycle_len);
    if (cut) pl.can_pre = pl.use_pre = false;
    const bool six = pl.form == StepPlan::Six;
    const bool dfront = pl.form == StepPlan::DistFront;
    const size_t n = (size_t)h->n, nv = (size_t)h->nv, np = (size_t)h->np;
    const int par = st->work & 1;
    // ---- what the front will read
    out->nsol = st->nsol;
    out->has_carry = pl.carry ? 1 : 0;
    out->has_six = six ? 1 : 0;
    int ctr = 0;
    if (st->tables()) DNS_TRY(st->stepctr.download(&ctr, 1, s));
    DNS_HIP(hipStreamSynchronize(s));
    out->tab_row = ctr;
    auto row_of = [&](const dns::TabRef &t) {
        if (!t.ctr) return t.base;
        const int r = ctr < 0 ? 0 : (ctr >= t.rows ? t.rows - 1 : ctr);
        return t.base + (size_t)r * t.stride;
    };
    const int ring[5] = {st->cur, st->prev, st->pprev, st->p3, st->p4};
    if (out->ring)
        for (int q = 0; q < 5; ++q)
            DNS_TRY(st->xs[ring[q]].download(out->ring + q * n, n, s));
    if (out->nfc_in) {
        DNS_TRY(st->nfc[st->nc].download(out->nfc_in, nv, s));
        DNS_TRY(st->nfc[st->no].download(out->nfc_in + nv, nv, s));
    }
    if (out->g_in)
        DNS_TRY(dns::download_from(out->g_in, row_of(st->g_ref()), nv, s));
    if (out->gp_in && np)
        DNS_TRY(dns::download_from(out->gp_in, row_of(st->gp_ref()), np, s));
    if (out->b_prev) DNS_TRY(st->b.download(out->b_prev, n, s));
    if (out->r_in) DNS_TRY(dns::download_from(out->r_in, h->r.p, n, s));
    if (pl.carry) {
        if (out->kxs_in)
            for (int q = 1; q < 5; ++q)
                DNS_TRY(st->kxs[ring[q]].download(out->kxs_in + (q - 1) * n, n,
                                                  s));
        if (out->rcarry_in) DNS_TRY(st->rcarry.download(out->rcarry_in, nv, s));
    }
    if (six || pl.dcarry) {
        if (out->rc6_in) {
            DNS_TRY(st->rc6[par].download(out->rc6_in, nv, s));
            DNS_TRY(st->rc6[1 - par].download(out->rc6_in + nv, nv, s));
        }
        // (row-partitioned: the solve before has overwritten its warm start in
        // place; what is left of it is the copy its front made for a lazy
        // tail with cells, x0c -- stale unless that step's plan had dtail)
        if (out->x0_other)
            DNS_TRY((six ? st->x0buf[1 - par] : st->x0c)
                        .download(out->x0_other, n, s));
    }
    DNS_HIP(hipStreamSynchronize(s));
    // ---- the front, by its form (prologue() without launch_front_nodes)
    switch (pl.form) {
        case StepPlan::Six: DNS_TRY(st->front_six(cf, pl)); break;
        case StepPlan::Fused: DNS_TRY(st->front_fused(cf, pl)); break;
        case StepPlan::DistFront: DNS_TRY(st->front_dist(cf, pl)); break;
        case StepPlan::StreamRhs:
        case StepPlan::StreamRows: DNS_TRY(st->front_stream(cf, pl)); break;
        case StepPlan::Plain:
        case StepPlan::Rows: DNS_TRY(st->front_rows(cf, pl)); break;
    }
    DNS_HIP(hipStreamSynchronize(s));
    // ---- what it has left
    out->form = (int32_t)pl.form;
    out->mode = pl.mode;
    out->use_pre = pl.use_pre ? 1 : 0;
    out->carry = pl.carry ? 1 : 0;
    out->k_lpr = h->K.lpr;
    out->r1_lpr = st->R1.lpr;
    out->r1_pair = st->R1p.ready ? 1 : 0;
    out->pad = 0;
    const dns::RowMap rm = (h->dist() && h->dist_sliced && h->dd)
                               ? h->dist_rowmap() : dns::RowMap{0, 0, 0, 0};
    out->rowmap[0] = rm.row0;
    out->rowmap[1] = rm.len1;
    out->rowmap[2] = rm.row2;
    out->rowmap[3] = rm.len2;
    out->dcarry = pl.dcarry ? 1 : 0;
    out->dtail = pl.dtail ? 1 : 0;
    out->have_cells = pl.have_cells ? 1 : 0;
    out->nsel = st->part.on ? st->part.nsel : 0;
    const bool fused = pl.form == StepPlan::Fused;
    out->nparts = (fused || dfront) ? st->front_nparts(pl) : 0;
    if (out->x0)
        DNS_TRY((six ? st->x0buf[par] : st->xs[st->work]).download(out->x0, n,
                                                                   s));
    if (out->b) DNS_TRY(st->b.download(out->b, n, s));
    if (out->nfc_out) DNS_TRY(st->nfc[st->nc].download(out->nfc_out, nv, s));
    if (six && out->kx) DNS_TRY(st->kx6.download(out->kx, n, s));
    if (pl.dtail && out->x0copy) DNS_TRY(st->x0c.download(out->x0copy, n, s));
    if (fused || dfront) {
        if (out->nparts > out->parts_cap && (out->partR || out->partB))
            return dns::fail(DNS_ERR_BAD_ARGUMENT, "%d partials, room for %d",
                             out->nparts, out->parts_cap);
        if (out->r) DNS_TRY(dns::download_from(out->r, h->r.p, n, s));
        if (out->partR)
            DNS_TRY(dns::download_from(out->partR, h->partR.p,
                                       (size_t)out->nparts, s));
        if (out->partB)
            DNS_TRY(dns::download_from(out->partB, h->partB.p,
                                       (size_t)out->nparts, s));
    }
    if (pl.mode == 2) {
        if (out->kxs_cur) DNS_TRY(st->kxs[st->cur].download(out->kxs_cur, n, s));
        if (out->rcarry_out)
            DNS_TRY(st->rcarry.download(out->rcarry_out, nv, s));
    }
    DNS_HIP(hipStreamSynchronize(s));
    return DNS_OK;
} DNS_CAPI_CATCH

}  // extern "C"
