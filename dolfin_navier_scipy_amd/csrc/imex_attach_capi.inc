// The attachments of the resident IMEX loop -- observer feedback
// (feedback.hpp), trajectory recorder (record.hpp), force functionals
// (functional.hpp), flow statistics (stats.hpp), quadratic functionals
// (quadratic.hpp), snapshot ensemble (ensemble.hpp): one node each in front of
// every step -- and their extern "C" entry points (included by dns_amd.hip
// behind imex_capi.inc).  First each one's key and launch, then
// dns_imex::attachments(), the one list of them that everything else loops
// over; what functionals and quadratics share (the source of moving Dirichlet
// values, the log of the workgroups' shares) is MovingBc and ShareLog, and
// attach_host.hpp for what needs no device.

// "feedback on", its shape, its coefficients and every buffer k_lti_step is
// handed: a graph captured for another set must not be replayed
uint64_t dns_imex::fb_key() const {
    const Feedback &f = *fb;
    uint64_t k = mix64(0xfb, {kw(f.hN), kw(f.Ny), kw(f.Nu), kw(f.rows),
                              kw(f.has_drift), kw(f.dt), kw(f.c_n), kw(f.c_c),
                              kw(f.C.vals.p), kw(f.B.vals.p), kw(f.haT.p),
                              kw(f.drift.p), kw(f.state.p), kw(f.ylog.p),
                              kw(f.ulog.p), kw(f.geff.p), kw(g.p)});
    if (!f.bc) return k;
    // the boundary mode: its shape, weights and every further buffer
    // k_lti_bc_step is handed (the table itself is part of config_key)
    const Feedback::Boundary &b = *f.bc;
    k = mix64(k, {kw(0xbc), kw(b.nc), kw(b.col0), kw(b.rhs), kw(f.has_b()),
                  kw(b.S.vals.p), kw(b.base.p), kw(b.Ba.vals.p),
                  kw(b.Bm.vals.p), kw(b.Bj.vals.p), kw(f.gpeff(sys->nv)),
                  kw(gp.p)});
    return mix64(k, {kw(b.wm[0]), kw(b.wm[1]), kw(b.wm[2]), kw(b.wa[0]),
                     kw(b.wa[1]), kw(b.wa[2]), kw(conv ? conv->ndbc : 0)});
}

// "recorder on", its shape, every buffer k_record_step is handed and the
// pressure scale of the state it is about to write down
uint64_t dns_imex::rec_key() const {
    return mix64(0x7ec, {kw(rec->rows), kw(rec->Ny), kw(rec->nslots),
                         kw(last_pscale), kw(rec->C ? rec->C->vals.p : nullptr),
                         kw(rec->slot.p), kw(rec->snap.p), kw(rec->ylog.p)});
}

int dns_imex::rec_launch(hipStream_t s) {
    const Recorder &r = *rec;
    const bool snaps = r.nslots > 0, outs = r.Ny > 0;
    const dns::RecArgs a{stepctr.p, r.rows, xs[cur].p, sys->nv, sys->n,
                         (int)sys->ld, last_pscale, r.slot.p,
                         snaps ? r.snap.p : (double *)nullptr, r.nslots, r.Ny,
                         outs ? r.C->rowptr.p : (const int *)nullptr,
                         outs ? r.C->colidx.p : (const int *)nullptr,
                         outs ? r.C->vals.p : (const double *)nullptr,
                         outs ? r.ylog.p : (double *)nullptr};
    hipLaunchKernelGGL(dns::k_record_step,
                       dns::record_grid((int)sys->ld, snaps, r.Ny),
                       dns::kBlock, 0, s, a);
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}

// with moving values: that they are, how many, their source and the table in
// use -- their own or the operator's --, its stride and rows
uint64_t dns_imex::MovingBc::key(uint64_t k, const dns_imex &st,
                                 int rows) const {
    if (!moving()) return k;
    const Table t = table(st, rows);
    return mix64(k, {kw(0xbc), kw(ndbc), kw(live), kw(t.p), kw(t.stride),
                     kw(t.rows)});
}

// "functionals on", their shape and instance (constant or moving Dirichlet
// values), every buffer k_functional_step is handed (the ring vectors come
// with the step key) and the pressure scale
uint64_t dns_imex::fn_key() const {
    const Functionals &f = *fn;
    uint64_t k = mix64(0xf6, {kw(f.nF), kw(f.log.G), kw(f.log.rows), kw(f.ncl),
                              kw(f.dt), kw(last_pscale), kw(f.rp.p),
                              kw(f.ci.p), kw(f.va.p), kw(f.cptr.p)});
    k = f.bc.key(k, *this, f.log.rows);
    return mix64(k,
                 {kw(f.cidx.p), kw(f.cw.p), kw(f.scale.p), kw(f.c0.p),
                  kw(f.log.buf.p), kw(stepctr.p), kw(conv ? conv->ncells : 0),
                  kw(conv ? conv->cellmap.p : nullptr),
                  kw(conv ? conv->glam.p : nullptr),
                  kw(conv ? conv->area.p : nullptr),
                  kw(conv ? conv->dbcvals.p : nullptr)});
}

int dns_imex::fn_launch(hipStream_t s) {
    const Functionals &f = *fn;
    const bool cells = f.ncl > 0;
    const int G = f.log.G;
    const dns::FnArgs a{stepctr.p, f.log.rows, xs[cur].p, xs[prev].p, sys->nv,
                        last_pscale, f.dt, f.nF, G, f.rp.p, f.ci.p, f.va.p,
                        f.ncl, f.cptr.p, f.cidx.p, f.cw.p,
                        cells ? conv->ncells : 0,
                        cells ? conv->cellmap.p : (const int *)nullptr,
                        cells ? conv->glam.p : (const double *)nullptr,
                        cells ? conv->area.p : (const double *)nullptr,
                        cells ? conv->dbcvals.p : (const double *)nullptr,
                        f.scale.p, f.c0.p, f.log.buf.p};
    if (f.bc.moving()) {
        dns::FnBcArgs b;
        static_cast<dns::FnArgs &>(b) = a;
        // (a live table is as wide as the functionals' own -- its stride is
        // ndbc -- and has more than `rows` rows: check_attachments)
        b.gtab = f.bc.table(*this, f.log.rows).p;
        b.ndbc = f.bc.ndbc;
        hipLaunchKernelGGL(dns::k_functional_step<dns::FnBcArgs>, G,
                           dns::kBlock, 0, s, b);
    } else {
        hipLaunchKernelGGL(dns::k_functional_step<dns::FnArgs>, G,
                           dns::kBlock, 0, s, a);
    }
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}

// k_lti_step<STAGE> / k_lti_bc_step<STAGE> by the size of ha, hb, hc
template <typename Args>
static int lti_launch(void (*staged)(Args), void (*inplace)(Args),
                      const Args &a, const dns::LtiArgs &l, hipStream_t s) {
    hipLaunchKernelGGL(dns::lti_staged(l.hN, l.Ny, l.Nu) ? staged : inplace,
                       dns::lti_grid(l.nv), dns::kBlock, 0, s, a);
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}

int dns_imex::fb_launch(hipStream_t s) {
    const Feedback &f = *fb;
    if (f.rows < 1)
        return dns::fail(DNS_ERR_NOT_READY, "observer feedback without a "
                         "table (dns_imex_set_feedback_table)");
    const dns::LtiArgs a{stepctr.p, f.rows, f.hN, f.Ny, f.Nu, sys->nv,
                         f.C.rowptr.p, f.C.colidx.p, f.C.vals.p,
                         f.B.rowptr.p, f.B.colidx.p, f.B.vals.p,
                         f.haT.p, f.hbT.p, f.hc.p,
                         f.has_drift ? f.drift.p : (const double *)nullptr,
                         f.state.p, f.ylog.p, f.ulog.p, f.dt, f.c_n,
                         f.c_c, g_src(), xs[cur].p, f.geff.p};
    if (!f.bc)
        return lti_launch(dns::k_lti_step<true>, dns::k_lti_step<false>, a, a,
                          s);
    // (check_attachments has seen to the convection operator and its table;
    // Ba, Bm, Bj and gpeff are null without the boundary terms)
    const Feedback::Boundary &c = *f.bc;
    dns::LtiArgs l = a;
    if (!f.has_b()) l.brp = nullptr;
    if (!f.rhs_v()) l.geff = nullptr;
    const dns::LtiBcArgs b{
        l, sys->np, c.nc, c.S.rowptr.p, c.S.colidx.p, c.S.vals.p, c.base.p,
        conv->dbc_tab.p + c.col0, std::max(1, conv->ndbc), conv->dbc_rows,
        c.Ba.rowptr.p, c.Ba.colidx.p, c.Ba.vals.p, c.Bm.rowptr.p,
        c.Bm.colidx.p, c.Bm.vals.p, c.Bj.rowptr.p, c.Bj.colidx.p, c.Bj.vals.p,
        c.wm[0], c.wm[1], c.wm[2], c.wa[0], c.wa[1], c.wa[2], gp_src(),
        f.gpeff(sys->nv)};
    return lti_launch(dns::k_lti_bc_step<true>, dns::k_lti_bc_step<false>, b,
                      b.l, s);
}

// "statistics on", their shape and grid, every buffer k_stats_step is handed
// and the pressure scale of the state it is about to add
uint64_t dns_imex::st_key() const {
    const Statistics &t = *stat;
    return mix64(0x57a7, {kw(t.rows), kw(t.lay.nbins), kw(t.lay.npairs),
                          kw(t.lay.G), kw(last_pscale), kw(t.bin.p),
                          kw(t.pairs.p), kw(t.acc.p), kw(stepctr.p)});
}

int dns_imex::st_launch(hipStream_t s) {
    const Statistics &t = *stat;
    const dns::StArgs a{stepctr.p, t.rows, xs[cur].p, sys->nv, sys->n,
                        (int)sys->ld, last_pscale, t.bin.p, t.lay.nbins,
                        t.lay.npairs, t.pairs.p, t.acc.p, t.lay.G,
                        t.lay.head(), t.lay.npx()};
    hipLaunchKernelGGL(dns::k_stats_step, t.lay.G, dns::kBlock, 0, s, a);
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}

// "quadratics on", their shape, forms and grid, every buffer
// k_quadratic_step is handed (the ring vectors come with the step key) and,
// with moving Dirichlet values, the table in use, its stride and rows
uint64_t dns_imex::qd_key() const {
    const Quadratics &q = *qd;
    uint64_t k = mix64(0x9d, {kw(q.nM), kw(q.nQ), kw(q.log.G), kw(q.log.rows),
                              kw(q.dt), kw(q.rp.p), kw(q.ci.p), kw(q.va.p),
                              kw(q.lrp.p), kw(q.lci.p), kw(q.lva.p),
                              kw(q.scale.p), kw(q.c0.p), kw(q.log.buf.p),
                              kw(stepctr.p)});
    for (int m = 0; m < q.nM; ++m)
        k = mix64(k, {kw(q.nzbase[m]), kw(q.need[m])});
    for (int f = 0; f < q.nQ; ++f)
        k = mix64(k, {kw(q.mat[f]), kw(q.lop[f]), kw(q.rop[f])});
    return q.bc.key(k, *this, q.log.rows);
}

int dns_imex::qd_launch(hipStream_t s) {
    const Quadratics &q = *qd;
    dns::QdArgs a{};
    a.stepctr = stepctr.p;
    a.nrows = q.log.rows;
    a.x = xs[cur].p;
    a.xp = xs[prev].p;
    a.nv = sys->nv;
    a.dt = q.dt;
    a.nM = q.nM;
    a.nQ = q.nQ;
    a.G = q.log.G;
    a.rp = q.rp.p;
    a.ci = q.ci.p;
    a.va = q.va.p;
    for (int m = 0; m < dns::kQdMaxMats; ++m) {
        a.nzbase[m] = q.nzbase[m];
        a.need |= (unsigned)q.need[m] << (2 * m);
    }
    for (int f = 0; f < q.nQ; ++f)
        a.forms |= dns::quadratic_form_bits(q.mat[f], q.lop[f], q.rop[f])
                   << (4 * f);
    a.lrp = q.lrp.p;
    a.lci = q.lci.p;
    a.lva = q.lva.p;
    a.scale = q.scale.p;
    a.c0 = q.c0.p;
    a.log = q.log.buf.p;
    if (q.bc.moving()) {
        const MovingBc::Table t = q.bc.table(*this, q.log.rows);
        dns::QdBcArgs b;
        static_cast<dns::QdArgs &>(b) = a;
        b.gtab = t.p;
        b.ndbc = q.bc.ndbc;             // (== t.stride: check_attachments)
        b.trows = t.rows;
        hipLaunchKernelGGL(dns::k_quadratic_step<dns::QdBcArgs>, a.G,
                           dns::kBlock, 0, s, b);
    } else {
        hipLaunchKernelGGL(dns::k_quadratic_step<dns::QdArgs>, a.G,
                           dns::kBlock, 0, s, a);
    }
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}

// "ensemble on", its shape and every buffer k_ensemble_step is handed (E is
// kept from slice to slice, and with it the key)
uint64_t dns_imex::ens_key() const {
    const Ensemble &e = *ens;
    return mix64(0xe5b, {kw(e.rows), kw(e.nslots), kw((long long)e.ldv),
                         kw(e.slot.p), kw(e.E.p), kw(stepctr.p)});
}

int dns_imex::ens_launch(hipStream_t s) {
    const Ensemble &e = *ens;
    const dns::EnsStepArgs a{stepctr.p, e.rows, xs[cur].p, sys->nv, e.slot.p,
                             e.E.p, e.nslots, e.ldv};
    hipLaunchKernelGGL(dns::k_ensemble_step, dns::ensemble_step_grid(sys->nv),
                       dns::kBlock, 0, s, a);
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}

// ---- what the six have in common --------------------------------------------

// (why a row-partitioned / distributed stepper refuses each: refuse_partitioned)
static const char *const kFbPartitioned =
    "the outputs y = C v would need an all-reduce (multi-rank feedback is not "
    "supported)";
static const char *const kRecPartitioned =
    "the outputs y = C v would need an all-reduce, the snapshots a gather "
    "(multi-rank recording is not supported)";
static const char *const kFnPartitioned = "the sums would need an all-reduce",
                         *const kQdPartitioned = kFnPartitioned;
static const char *const kStPartitioned =
    "the sums are local to a rank, the getter would need a gather (multi-rank "
    "statistics are not supported)";
static const char *const kEnsPartitioned =
    "the slots would hold a rank's rows only, the Gram matrix would need an "
    "all-reduce (multi-rank ensembles are not supported)";

// Those present, in the order of their nodes in front of every step:
// k_lti_step leaves the right-hand side the front kernels read, the other
// five write down / add the row of the step before -- and run once more
// behind the last step of a call (`closing`).
//
// Functionals and quadratics that read the operator's LIVE Dirichlet table
// (boundary feedback) depend on this order: k_lti_bc_step, the FIRST front
// node of step s, writes row s + 1; row j thus holds the values of the state
// before step j -- the row convention of the attachments' own tables -- and
// rows s and s - 1, which the two nodes of step s read behind it on the same
// stream, were complete a step earlier (row 0 was uploaded).  The closing
// launch reads row `rows`, which the last step's observer node wrote.
dns_imex::Attachments dns_imex::attachments() const {
    Attachments l;
    if (fb)
        l.a[l.n++] = {"observer feedback", kFbPartitioned, fb->rows, false,
                      &dns_imex::fb_key, &dns_imex::fb_launch};
    if (rec)
        l.a[l.n++] = {"recorder", kRecPartitioned, rec->rows, true,
                      &dns_imex::rec_key, &dns_imex::rec_launch};
    if (fn)
        l.a[l.n++] = {"functionals", kFnPartitioned, fn->log.rows, true,
                      &dns_imex::fn_key, &dns_imex::fn_launch};
    if (stat)
        l.a[l.n++] = {"statistics", kStPartitioned, stat->rows, true,
                      &dns_imex::st_key, &dns_imex::st_launch};
    if (qd)
        l.a[l.n++] = {"quadratics", kQdPartitioned, qd->log.rows, true,
                      &dns_imex::qd_key, &dns_imex::qd_launch};
    if (ens)
        l.a[l.n++] = {"ensemble", kEnsPartitioned, ens->rows, true,
                      &dns_imex::ens_key, &dns_imex::ens_launch};
    return l;
}

int dns_imex::launch_front_nodes(hipStream_t s) {
    for (const Attachment &a : attachments()) DNS_TRY((this->*a.launch)(s));
    return DNS_OK;
}

// Behind the last step of a call: the rows nobody runs a prologue for.
int dns_imex::launch_closing_nodes(hipStream_t s) {
    for (const Attachment &a : attachments())
        if (a.closing) DNS_TRY((this->*a.launch)(s));
    return DNS_OK;
}

uint64_t dns_imex::attachments_key(uint64_t k) const {
    for (const Attachment &a : attachments()) k = mix64(k, {(this->*a.key)()});
    return k;
}

bool dns_imex::tables() const {
    return tab_rows > 0 || (conv && conv->dbc_rows > 0) ||
           (conv && conv->nbrow > 0) || attachments().n > 0;
}

int dns_imex::rows_left() const {
    int lim = 1 << 30;
    if (tab_rows > 0) lim = std::min(lim, tab_rows);
    for (const Attachment &a : attachments()) lim = std::min(lim, a.rows);
    if (conv && conv->dbc_rows > 0) lim = std::min(lim, conv->dbc_rows);
    return lim - tab_pos;
}

// New tables: the step counter, which selects the row of every table, the log
// rows and the slot of the observer state (`tab_pos & 1`, slot 0 from here
// on), goes back to 0 -- here and nowhere else; complete on return.  The marks
// of the statistics count rows since the rewind: they go back with it (the
// sums stay).
int dns_imex::rewind_tables() {
    if (stat)
        DNS_HIP(hipMemsetAsync(stat->acc.p, 0, stat->lay.G * sizeof(double),
                               sys->stream));
    if (fb && (tab_pos & 1)) {
        const size_t n = (size_t)fb->stride();
        DNS_HIP(hipMemcpyAsync(fb->state.p, fb->state.p + n, n * sizeof(double),
                               hipMemcpyDeviceToDevice, sys->stream));
    }
    tab_pos = 0;
    six_ok = false;          // (cell values belong to a row of the old tables)
    dcells_ok = false;
    if (conv && conv->dbc_rows > 0) conv->dbc_row = 0;
    DNS_TRY(sync_counter());
    DNS_HIP(hipStreamSynchronize(sys->stream));
    return DNS_OK;
}

// The per-step index table of a base trajectory lives on the operator, which
// does not know its stepper: the step that follows a new one (a step or a run)
// counts from 0 like after any table setter -- unless one of those has just
// rewound the counter, as the slices of a time loop do.
int dns_imex::adopt_base_rows() {
    if (!conv || conv->brow_gen == brow_gen_seen) return DNS_OK;
    brow_gen_seen = conv->brow_gen;
    return tab_pos != 0 ? rewind_tables() : DNS_OK;
}

// None of the six runs on a row-partitioned / distributed stepper: refused
// when it is set and, should the stepper be partitioned later, by the step.
int dns_imex::refuse_partitioned(const char *noun, const char *reason) const {
    if (!(r1_rows || part.on || sys->dist())) return DNS_OK;
    return dns::fail(DNS_ERR_BAD_ARGUMENT, "%s on a row-partitioned stepper: %s",
                     noun, reason);
}

static const char *const kLinPartitioned =
    "the tails of the partitioned step evaluate N(v)v";
// (constant Dirichlet values beside a per-step table on the operator: what
// the setters say, and what a step says later)
static const char *const kQdMovingBc =
    "quadratics with a per-step Dirichlet table on the convection operator "
    "(dns_conv_set_dbc_table): moving boundary values are not part of the "
    "constants";
static const char *const kFnMovingBcSet =
    "functionals with a per-step Dirichlet table on the convection operator "
    "(dns_conv_set_dbc_table): the moving-boundary terms are not part of the "
    "functional";
static const char *const kFnMovingBcStep =
    "functionals with a per-step Dirichlet table on the convection operator: "
    "the moving-boundary terms are not part of the functional";

// What reading the operator's live Dirichlet table takes: the operator, its
// width and `rows` + 1 rows (the setters and the step ask alike).
int dns_imex::check_live(const char *noun, int ndbc, int rows) const {
    if (!conv)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "%s on the operator's Dirichlet table: no device "
                         "convection operator is attached "
                         "(dns_imex_set_convection)", noun);
    if (conv->ndbc != ndbc)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "%s on the operator's Dirichlet table: ndbc = %d, "
                         "the convection operator has %d Dirichlet values",
                         noun, ndbc, conv->ndbc);
    if (conv->dbc_rows < rows + 1)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "%s on the operator's Dirichlet table: it has %d "
                         "rows, %d steps need %d (dns_conv_set_dbc_table; row "
                         "0: the values of the current state)", noun,
                         conv->dbc_rows, rows, rows + 1);
    return DNS_OK;
}

// what a step refuses on their behalf
int dns_imex::check_attachments() const {
    if (conv && conv->linearised()) {
        DNS_TRY(refuse_partitioned("linearised convection operator",
                                   kLinPartitioned));
        if (fn && fn->ncl > 0)
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "linearised convection operator with functionals "
                             "with cells: their kernel evaluates N(v)v on the "
                             "listed cells (dns_imex_set_functionals without "
                             "cells, or dns_conv_clear_base_flow)");
        if (conv->lin_mode == dns::kConvAdjoint)
            DNS_TRY(dns::check_adjoint_dbc(conv->dbc_host.data(), conv->ndbc,
                                           conv->dbc_rows));
    }
    for (const Attachment &a : attachments())
        DNS_TRY(refuse_partitioned(a.noun, a.partitioned));
    if (fb && fb->bc) {
        const Feedback::Boundary &b = *fb->bc;
        // k_lti_bc_step writes row `counter + 1` of the operator's table
        if (!conv)
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "boundary feedback needs the device convection "
                             "operator whose Dirichlet table it writes "
                             "(dns_imex_set_convection)");
        if (b.col0 + b.nc > conv->ndbc)
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "boundary feedback: the controlled columns "
                             "[%d, %d) do not fit the %d Dirichlet values of "
                             "the convection operator", b.col0,
                             b.col0 + b.nc, conv->ndbc);
        if (conv->dbc_rows < fb->rows + 1)
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "boundary feedback: the Dirichlet table has %d "
                             "rows, %d steps need %d (dns_conv_set_dbc_table; "
                             "row 0: the values of the current state)",
                             conv->dbc_rows, fb->rows, fb->rows + 1);
        // (the device makes the values: a host-made copy cannot hold them)
        if ((fn && !fn->bc.live) || (qd && !qd->bc.live))
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "boundary feedback with %s that do not read the "
                             "operator's live Dirichlet table: their Dirichlet "
                             "values are host-made copies (%s)",
                             fn && !fn->bc.live ? "functionals" : "quadratics",
                             fn && !fn->bc.live
                                 ? "dns_imex_set_functionals_live"
                                 : "dns_imex_set_quadratics_live");
    }
    if (qd)
        DNS_TRY(qd->bc.check_step(*this, qd->log.rows, "quadratics",
                                  "dns_imex_set_quadratics_bc", kQdMovingBc));
    if (!fn) return DNS_OK;
    if (fn->ncl > 0 && !conv)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "functionals with cells need the device convection "
                         "operator they were set with "
                         "(dns_imex_set_convection)");
    // (the listed cells are positions in that operator's cell order)
    if (fn->ncl > 0 && (conv != fn->conv || conv->ncells != fn->ncells ||
                        conv->cellmap.p != fn->cellmap))
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "functionals with cells were set with another "
                         "convection operator than the one attached now: "
                         "set them again (dns_imex_set_functionals)");
    return fn->bc.check_step(*this, fn->log.rows, "functionals",
                             "dns_imex_set_functionals_bc", kFnMovingBcStep);
}

// (the table rows are `ndbc` wide, and so are the cells' Dirichlet slots of
// the functionals and the columns behind nv of the quadratics: positions in
// the operator's values)
int dns_imex::MovingBc::check_step(const dns_imex &st, int rows,
                                   const char *noun, const char *setter,
                                   const char *const_refusal) const {
    const dns_conv *cv = st.conv;
    if (!moving() && cv && cv->dbc_rows > 0)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "%s", const_refusal);
    if (moving() && cv && cv->ndbc != ndbc)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "%s with moving Dirichlet values were set for %d "
                         "values, the convection operator attached now has "
                         "%d: set them again (%s)", noun, ndbc, cv->ndbc,
                         setter);
    return live ? st.check_live(noun, ndbc, rows) : DNS_OK;
}

int dns_imex::MovingBc::check_set(const dns_imex &st, const char *noun,
                                  const char *const_refusal, bool moving,
                                  bool live, int ndbc, int rows) {
    if (!moving && st.conv && st.conv->dbc_rows > 0)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "%s", const_refusal);
    return live ? st.check_live(noun, ndbc, rows) : DNS_OK;
}

// the handle, the attachment (`what`: "... is" / "... are") and the device
static int need(dns_imex *st, bool present, const char *what,
                const char *setter) {
    if (!st) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    if (!present)
        return dns::fail(DNS_ERR_NOT_READY, "no %s set (%s)", what, setter);
    return hipSetDevice(st->sys->device) == hipSuccess
               ? DNS_OK : dns::fail(DNS_ERR_HIP, "hipSetDevice failed");
}

// Rows [first, first + count) of a log of `rows` rows, `width` entries each
// (`ld` apart on the device), into `dst` (null: the range is checked only);
// complete on return.
static int download_log_rows(dns_imex *st, double *dst, const double *buf,
                             int first, int count, size_t width, int rows,
                             const char *what, const char *holder,
                             size_t ld = 0) {
    if (first < 0 || count < 0 || first + count > rows)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "%s [%d, %d) asked for, the %s holds %d", what, first,
                         first + count, holder, rows);
    if (ld == 0) ld = width;
    hipStream_t s = st->sys->stream;
    if (dst)
        DNS_TRY(dns::download_rows(dst, buf + (size_t)first * ld,
                                   (size_t)count, width, ld, s));
    DNS_HIP(hipStreamSynchronize(s));
    return DNS_OK;
}

// A buffer that is large enough is kept, and with it the graphs that were
// captured for it: the slices of a time loop set their attachments again and
// again.  `dst` gets room for `need` entries -- a fresh buffer now, unless
// `old` (which may be `dst` itself) holds one that will do: adopt() takes that
// one over, once nothing can be refused any more.
template <typename T>
static int keep_or_alloc(dns::DevBuf<T> &dst, const dns::DevBuf<T> &old,
                         size_t need) {
    if (old.p != nullptr && old.n >= need) return DNS_OK;
    return dst.alloc(need);
}

template <typename T>
static void adopt(dns::DevBuf<T> &dst, dns::DevBuf<T> &old) {
    if (dst.p != nullptr) return;
    std::swap(dst.p, old.p);
    std::swap(dst.n, old.n);
}

// a host vector into a buffer that is kept where it is large enough
template <typename T>
static int put(dns::DevBuf<T> &buf, const std::vector<T> &host, hipStream_t s) {
    DNS_TRY(keep_or_alloc(buf, buf, host.size()));
    if (!host.empty()) DNS_TRY(buf.upload(host.data(), host.size(), s));
    return DNS_OK;
}

int dns_imex::MovingBc::set(bool moving, bool live_, int ndbc_, int rows,
                            const double *dbc_table, hipStream_t s) {
    if (moving && !live_) {
        const size_t ng = ((size_t)rows + 1) * ndbc_;
        DNS_TRY(keep_or_alloc(gtab, gtab, ng));
        DNS_TRY(gtab.upload(dbc_table, ng, s));
    }
    ndbc = moving ? ndbc_ : 0;
    live = live_;
    return DNS_OK;
}

int dns_imex::ShareLog::ensure(int rows_, int G_, int n_, hipStream_t s) {
    DNS_TRY(keep_or_alloc(buf, buf, (size_t)rows_ * G_ * n_));
    DNS_TRY(buf.zero(s));
    rows = rows_;
    G = G_;
    n = n_;
    return DNS_OK;
}

// rows [first, first + count) of the log, the shares summed (`what`: the rows
// in a refusal); complete on return
int dns_imex::ShareLog::download_sums(dns_imex *st, int first, int count,
                                      double *out, const char *what) const {
    if (!out) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    const size_t per = (size_t)G * n;
    std::vector<double> part((size_t)std::min(std::max(count, 0), rows) * per);
    DNS_TRY(download_log_rows(st, part.data(), buf.p, first, count, per, rows,
                              what, "log"));
    dns::sum_shares(part.data(), count, G, n, out);
    return DNS_OK;
}

// Before an attachment is set again or taken off: replays may still use its
// buffers.  (The counter goes on counting for the other tables, if any.)
static int quiesce(dns_imex *st) {
    if (!st) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_HIP(hipSetDevice(st->sys->device));
    DNS_HIP(hipStreamSynchronize(st->sys->stream));
    return DNS_OK;
}

// the exports that clear an attachment
template <typename T>
static int take_off(dns_imex *st, std::unique_ptr<T> dns_imex::*which) {
    DNS_TRY(quiesce(st));
    (st->*which).reset();
    return DNS_OK;
}

// What dns_imex_set_functionals (`moving` false: constant Dirichlet values,
// three sparse rows per functional), dns_imex_set_functionals_bc (`moving`:
// five rows and a table of the values, (nrows + 1) x ndbc) and
// dns_imex_set_functionals_live (`moving` and `live`: no table, the attached
// convection operator's is read) share: every check first -- a refusal leaves the functionals that were there --, then the
// upload.  Called inside the exports' exception barrier.
static int set_functionals(dns_imex *st, int32_t nF, const dns_csr *ca,
                           const dns_csr *cm, const dns_csr *cp,
                           const dns_csr *cab, const dns_csr *cmb,
                           const double *c0, const double *scale,
                           const int32_t *cell_ptr, const int32_t *cell_idx,
                           const double *cell_w, double dt, int32_t nrows,
                           int32_t ndbc, const double *dbc_table,
                           bool moving, bool live = false) {
    if (!st) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = st->sys;
    DNS_TRY(st->refuse_partitioned("functionals", kFnPartitioned));
    const int nterms = moving ? 5 : 3;
    const dns_csr *terms[5] = {ca, cm, cp, cab, cmb};
    DNS_TRY(dns::check_functionals_args(nF, dns::kFnMax, nrows, dt, moving,
                                        live, ndbc, dbc_table, terms, h->nv,
                                        h->np, cell_ptr, cell_idx, cell_w));
    for (int t = 0; t < nterms; ++t)
        if (terms[t]) DNS_TRY(dns::check_csr(terms[t], dns::kFnTermNames[t]));
    DNS_TRY(dns_imex::MovingBc::check_set(*st, "functionals", kFnMovingBcSet,
                                          moving, live, ndbc, nrows));
    const int ncl = cell_ptr ? cell_ptr[nF] : 0;
    if (ncl > 0) {
        if (!st->conv)
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "functionals with cells need a device convection "
                             "operator (dns_imex_set_convection)");
        for (int j = 0; j < ncl; ++j)
            if (cell_idx[j] < 0 || cell_idx[j] >= st->conv->ncells)
                return dns::fail(DNS_ERR_BAD_ARGUMENT,
                                 "functionals: cell index %d at %d outside "
                                 "0..%d (ncells of the convection operator)",
                                 (int)cell_idx[j], j, st->conv->ncells - 1);
    }
    if (moving && ncl > 0 && st->conv->ndbc != ndbc)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "functionals: ndbc = %d, the convection operator of "
                         "the listed cells has %d Dirichlet values",
                         (int)ndbc, st->conv->ndbc);
    // the 3 nF (5 nF) sparse rows (k, term) in one CSR
    std::vector<int> rp, ci;
    std::vector<double> va, sc, cc;
    dns::stack_rows(terms, nterms, nF, rp, ci, va);
    std::vector<int> cptr(nF + 1, 0);
    if (cell_ptr) cptr.assign(cell_ptr, cell_ptr + nF + 1);
    dns::scale_c0(scale, c0, nF, sc, cc);
    DNS_TRY(quiesce(st));                       // replays may still write it
    hipStream_t s = h->stream;
    // In place (keep_or_alloc; everything was checked above: a failed
    // allocation leaves the stepper without functionals).
    std::unique_ptr<dns_imex::Functionals> f = std::move(st->fn);
    if (!f) f.reset(new (std::nothrow) dns_imex::Functionals());
    if (!f) return dns::fail(DNS_ERR_BAD_ARGUMENT, "out of host memory");
    DNS_TRY(put(f->rp, rp, s));
    DNS_TRY(put(f->ci, ci, s));
    DNS_TRY(put(f->va, va, s));
    DNS_TRY(put(f->cptr, cptr, s));
    DNS_TRY(put(f->scale, sc, s));
    DNS_TRY(put(f->c0, cc, s));
    DNS_TRY(keep_or_alloc(f->cidx, f->cidx, (size_t)ncl));
    DNS_TRY(keep_or_alloc(f->cw, f->cw, (size_t)12 * ncl));
    if (ncl > 0) {
        // (the operator keeps its cells in an order of its own)
        std::vector<int> cint((size_t)ncl);
        for (int j = 0; j < ncl; ++j)
            cint[j] = st->conv->cpos_host[cell_idx[j]];
        DNS_TRY(f->cidx.upload(cint.data(), (size_t)ncl, s));
        DNS_TRY(f->cw.upload(cell_w, (size_t)12 * ncl, s));
    }
    DNS_TRY(f->log.ensure(nrows, dns::functional_grid(nF, ncl, nterms), nF, s));
    DNS_TRY(f->bc.set(moving, live, ndbc, nrows, dbc_table, s));
    f->nF = nF;
    f->ncl = ncl;
    f->dt = dt;
    f->conv = ncl > 0 ? st->conv : nullptr;
    f->ncells = ncl > 0 ? st->conv->ncells : 0;
    f->cellmap = ncl > 0 ? st->conv->cellmap.p : nullptr;
    st->fn = std::move(f);
    return st->rewind_tables();
}

// The state slot of the current parity -- hx, f_last, u_c and (boundary mode)
// u_p -- from the host (`P` const double *) or to it (double *); a null
// pointer leaves its part out; complete on return.
template <typename P>
static int fb_state_copy(dns_imex *st, P hx, P f_last, P u_c, P u_p) {
    constexpr bool up = std::is_const<std::remove_pointer_t<P>>::value;
    const dns_imex::Feedback &f = *st->fb;
    hipStream_t s = st->sys->stream;
    if (up) DNS_HIP(hipStreamSynchronize(s));
    double *slot = f.state.p + (size_t)(st->tab_pos & 1) * f.stride();
    const P host[4] = {hx, f_last, u_c, u_p};
    const int len[4] = {f.hN, f.hN, f.Nu, f.Nu};
    for (int q = 0; q < 4; slot += len[q++]) {
        if (!host[q]) continue;
        if constexpr (up)
            DNS_TRY(dns::upload_to(slot, host[q], (size_t)len[q], s));
        else
            DNS_TRY(dns::download_from(host[q], slot, (size_t)len[q], s));
    }
    if (!up) DNS_HIP(hipStreamSynchronize(s));
    return DNS_OK;
}

extern "C" {

// ---- observer feedback (feedback.hpp) --------------------------------------

int dns_imex_set_feedback(dns_imex *st, const dns_csr *cmat, const dns_csr *bmat,
                          const double *ha, const double *hb, const double *hc,
                          int32_t hN, int32_t Ny, int32_t Nu, double c_n,
                          double c_c, double dt) try {
    if (!st || !cmat || !bmat || !ha || !hb || !hc)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = st->sys;
    DNS_TRY(st->refuse_partitioned("observer feedback", kFbPartitioned));
    if (hN < 1 || hN > dns::kFbMaxState || Ny < 1 || Ny > dns::kFbMaxOut ||
        Nu < 1 || Nu > dns::kFbMaxIn)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "observer feedback: hN = %d, Ny = %d, Nu = %d outside "
                         "the limits 1..%d, 1..%d, 1..%d of the one-launch "
                         "observer step", (int)hN, (int)Ny, (int)Nu,
                         dns::kFbMaxState, dns::kFbMaxOut, dns::kFbMaxIn);
    DNS_TRY(dns::check_csr(cmat, "C"));
    DNS_TRY(dns::check_csr(bmat, "B"));
    if (cmat->nrows != Ny || cmat->ncols != h->nv)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "C must be Ny x NV (%d x %d)",
                         (int)Ny, h->nv);
    if (bmat->nrows != h->nv || bmat->ncols != Nu)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "B must be NV x Nu (%d x %d)",
                         h->nv, (int)Nu);
    if (cmat->nnz > dns::kFbMaxNnzC)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "observer feedback: C has %lld non-zeros, the "
                         "one-launch observer step takes at most %d",
                         (long long)cmat->nnz, dns::kFbMaxNnzC);
    if (!(dt > 0.0))
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "observer feedback: dt <= 0");
    DNS_TRY(quiesce(st));                       // replays may still read it
    hipStream_t s = h->stream;
    // A fresh one (the plain mode: dns_imex_set_feedback_boundary follows),
    // moved in once nothing can fail any more; a `geff` that is large enough
    // is taken over from the one that was there.
    std::unique_ptr<dns_imex::Feedback> fp(new (std::nothrow)
                                               dns_imex::Feedback());
    if (!fp) return dns::fail(DNS_ERR_BAD_ARGUMENT, "out of host memory");
    dns_imex::Feedback &f = *fp;
    DNS_TRY(f.C.upload(cmat, s));
    DNS_TRY(f.B.upload(bmat, s));
    const size_t n = (size_t)hN;
    std::vector<double> haT(n * n), hbT(n * Ny);
    for (size_t i = 0; i < n; ++i) {
        for (size_t j = 0; j < n; ++j) haT[j * n + i] = ha[i * n + j];
        for (size_t k = 0; k < (size_t)Ny; ++k) hbT[k * n + i] = hb[i * Ny + k];
    }
    DNS_TRY(f.haT.alloc(n * n));
    DNS_TRY(f.haT.upload(haT.data(), n * n, s));
    DNS_TRY(f.hbT.alloc(n * Ny));
    DNS_TRY(f.hbT.upload(hbT.data(), n * Ny, s));
    DNS_TRY(f.hc.alloc(n * Nu));
    DNS_TRY(f.hc.upload(hc, n * Nu, s));
    f.hN = hN;
    f.Ny = Ny;
    f.Nu = Nu;
    f.dt = dt;
    f.c_n = c_n;
    f.c_c = c_c;
    DNS_TRY(f.state.alloc((size_t)2 * f.stride()));
    DNS_TRY(f.state.zero(s));
    dns::DevBuf<double> &old = st->fb ? st->fb->geff : f.geff;
    DNS_TRY(keep_or_alloc(f.geff, old, (size_t)h->nv));
    DNS_TRY((f.geff.p ? f.geff : old).zero(s));
    DNS_HIP(hipStreamSynchronize(s));
    adopt(f.geff, old);
    st->fb = std::move(fp);
    return DNS_OK;
} DNS_CAPI_CATCH

static int fb_need(dns_imex *st) {
    return need(st, st && st->fb, "observer feedback is",
                "dns_imex_set_feedback");
}

int dns_imex_set_feedback_state(dns_imex *st, const double *hx,
                                const double *f_last, const double *u_c) try {
    DNS_TRY(fb_need(st));
    if (!hx || !f_last || !u_c)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    return fb_state_copy(st, hx, f_last, u_c, (const double *)nullptr);
} DNS_CAPI_CATCH

int dns_imex_get_feedback_state(dns_imex *st, double *hx, double *f_last,
                                double *u_c) try {
    DNS_TRY(fb_need(st));
    return fb_state_copy(st, hx, f_last, u_c, (double *)nullptr);
} DNS_CAPI_CATCH

int dns_imex_set_feedback_table(dns_imex *st, int32_t nsteps,
                                const double *drift) try {
    DNS_TRY(fb_need(st));
    if (nsteps < 1) return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    dns_imex::Feedback &f = *st->fb;
    dns_saddle *h = st->sys;
    hipStream_t s = h->stream;
    DNS_HIP(hipStreamSynchronize(s));           // replays may still read it
    const size_t ns = (size_t)nsteps;
    if (drift) {
        if (f.drift.n < ns * f.hN) DNS_TRY(f.drift.alloc(ns * f.hN));
        DNS_TRY(f.drift.upload(drift, ns * f.hN, s));
    }
    if (f.ylog.n < ns * f.Ny) DNS_TRY(f.ylog.alloc(ns * f.Ny));
    if (f.ulog.n < ns * f.Nu) DNS_TRY(f.ulog.alloc(ns * f.Nu));
    DNS_TRY(f.ylog.zero(s));
    DNS_TRY(f.ulog.zero(s));
    f.has_drift = drift != nullptr;
    f.rows = nsteps;
    return st->rewind_tables();
} DNS_CAPI_CATCH

int dns_imex_get_feedback_log(dns_imex *st, int32_t first, int32_t count,
                              double *y, double *u) try {
    DNS_TRY(fb_need(st));
    const dns_imex::Feedback &f = *st->fb;
    DNS_TRY(download_log_rows(st, y, f.ylog.p, first, count, (size_t)f.Ny,
                              f.rows, "log rows", "table"));
    return download_log_rows(st, u, f.ulog.p, first, count, (size_t)f.Nu,
                             f.rows, "log rows", "table");
} DNS_CAPI_CATCH

int dns_imex_clear_feedback(dns_imex *st) try {
    return take_off(st, &dns_imex::fb);
} DNS_CAPI_CATCH

// ---- boundary feedback (k_lti_bc_step) -------------------------------------

static int fbc_need(dns_imex *st) {
    return need(st, st && st->fb && st->fb->bc, "boundary feedback is",
                "dns_imex_set_feedback_boundary");
}

int dns_imex_set_feedback_boundary(dns_imex *st, const dns_csr *smat,
                                   const double *base, int32_t col0,
                                   const dns_csr *ba, const dns_csr *bm,
                                   const dns_csr *bj, const double *wm,
                                   const double *wa) try {
    if (!st || !smat || !wm || !wa)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    // a refusal, or a failure, leaves the feedback as dns_imex_set_feedback
    // left it
    DNS_TRY(st->refuse_partitioned("boundary feedback", kFbPartitioned));
    DNS_TRY(fb_need(st));
    dns_saddle *h = st->sys;
    dns_imex::Feedback &f = *st->fb;
    if (!st->conv)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "boundary feedback needs a device convection operator: "
                         "it writes that operator's Dirichlet table "
                         "(dns_imex_set_convection)");
    DNS_TRY(dns::check_csr(smat, "S"));
    const int nc = smat->nrows;
    if (nc < 1 || smat->ncols != f.Nu)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "boundary feedback: S must be nc x Nu (%d columns), "
                         "it is %d x %d", f.Nu, (int)smat->nrows,
                         (int)smat->ncols);
    if (col0 < 0 || col0 + nc > st->conv->ndbc)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "boundary feedback: the controlled columns [%d, %d) "
                         "do not fit the %d Dirichlet values of the convection "
                         "operator", (int)col0, (int)col0 + nc,
                         st->conv->ndbc);
    const bool rhs = ba || bm || bj;
    if (rhs && !(ba && bm && bj))
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "boundary feedback: Ba, Bm and Bj come together (or "
                         "all NULL: no boundary terms)");
    if (rhs) {
        const dns_csr *mats[3] = {ba, bm, bj};
        const char *names[3] = {"Ba", "Bm", "Bj"};
        for (int t = 0; t < 3; ++t) {
            DNS_TRY(dns::check_csr(mats[t], names[t]));
            const int want = t == 2 ? h->np : h->nv;
            if (mats[t]->nrows != want || mats[t]->ncols != f.Nu)
                return dns::fail(DNS_ERR_BAD_ARGUMENT,
                                 "boundary feedback: %s must be %d x %d, it is "
                                 "%d x %d", names[t], want, f.Nu,
                                 (int)mats[t]->nrows, (int)mats[t]->ncols);
        }
    }
    DNS_TRY(quiesce(st));                       // replays may still read it
    hipStream_t s = h->stream;
    std::unique_ptr<dns_imex::Feedback::Boundary> b(
        new (std::nothrow) dns_imex::Feedback::Boundary());
    if (!b) return dns::fail(DNS_ERR_BAD_ARGUMENT, "out of host memory");
    DNS_TRY(b->S.upload(smat, s));
    std::vector<double> b0((size_t)nc, 0.0);
    if (base) b0.assign(base, base + nc);
    DNS_TRY(b->base.alloc((size_t)nc));
    DNS_TRY(b->base.upload(b0.data(), (size_t)nc, s));
    if (rhs) {
        DNS_TRY(b->Ba.upload(ba, s));
        DNS_TRY(b->Bm.upload(bm, s));
        DNS_TRY(b->Bj.upload(bj, s));
    }
    b->rhs = rhs;
    b->nc = nc;
    b->col0 = col0;
    for (int j = 0; j < 3; ++j) {
        b->wm[j] = wm[j];
        b->wa[j] = wa[j];
    }
    // geff and gpeff in one buffer; the slots get room for u_p: fresh
    // buffers, which take the others' place once nothing can fail any more
    dns::DevBuf<double> geff, state;
    DNS_TRY(keep_or_alloc(geff, f.geff,
                          (size_t)h->nv + (size_t)std::max(1, h->np)));
    DNS_TRY((geff.p ? geff : f.geff).zero(s));
    DNS_TRY(state.alloc((size_t)4 * (f.hN + f.Nu)));
    DNS_TRY(state.zero(s));
    DNS_HIP(hipStreamSynchronize(s));
    if (geff.p) f.geff.release();               // (else: kept)
    adopt(f.geff, geff);
    f.state.release();
    adopt(f.state, state);
    f.bc = std::move(b);
    f.rows = 0;                                 // the table follows
    f.has_drift = false;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_imex_set_feedback_state_bc(dns_imex *st, const double *hx,
                                   const double *f_last, const double *u_c,
                                   const double *u_p) try {
    DNS_TRY(fbc_need(st));
    if (!hx || !f_last || !u_c || !u_p)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    return fb_state_copy(st, hx, f_last, u_c, u_p);
} DNS_CAPI_CATCH

int dns_imex_get_feedback_state_bc(dns_imex *st, double *hx, double *f_last,
                                   double *u_c, double *u_p) try {
    DNS_TRY(fbc_need(st));
    return fb_state_copy(st, hx, f_last, u_c, u_p);
} DNS_CAPI_CATCH

int dns_imex_get_feedback_bcs(dns_imex *st, int32_t first, int32_t count,
                              double *bcs) try {
    DNS_TRY(fbc_need(st));
    const dns_imex::Feedback::Boundary &b = *st->fb->bc;
    const dns_conv *cv = st->conv;
    if (!bcs) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    if (!cv || cv->dbc_rows < 1 || b.col0 + b.nc > cv->ndbc)
        return dns::fail(DNS_ERR_NOT_READY,
                         "boundary feedback: no Dirichlet table of that width "
                         "on the convection operator (dns_conv_set_dbc_table)");
    return download_log_rows(st, bcs, cv->dbc_tab.p + b.col0, first, count,
                             (size_t)b.nc, cv->dbc_rows, "table rows",
                             "Dirichlet table", (size_t)std::max(1, cv->ndbc));
} DNS_CAPI_CATCH

int dns_imex_get_feedback_rhs(dns_imex *st, double *geff, double *gpeff) try {
    DNS_TRY(fbc_need(st));
    const dns_imex::Feedback &f = *st->fb;
    const dns_saddle *h = st->sys;
    if ((geff && !f.rhs_v()) || (gpeff && !f.rhs_p()))
        return dns::fail(DNS_ERR_NOT_READY,
                         "boundary feedback without terms of the right-hand "
                         "side: the step reads the tabulated rows");
    hipStream_t s = h->stream;
    if (geff) DNS_TRY(dns::download_from(geff, f.geff.p, (size_t)h->nv, s));
    if (gpeff)
        DNS_TRY(dns::download_from(gpeff, f.gpeff(h->nv), (size_t)h->np, s));
    DNS_HIP(hipStreamSynchronize(s));
    return DNS_OK;
} DNS_CAPI_CATCH

// ---- trajectory recorder (record.hpp) --------------------------------------

int dns_imex_set_recorder(dns_imex *st, const dns_csr *cmat, int32_t nrows,
                          const int32_t *snap_slot, int32_t nslots) try {
    if (!st) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = st->sys;
    DNS_TRY(st->refuse_partitioned("recorder", kRecPartitioned));
    if (!cmat && !snap_slot)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "recorder: neither outputs (cmat) nor snapshots "
                         "(snap_slot) asked for");
    if (nrows < 1)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "recorder: nrows = %d < 1",
                         (int)nrows);
    if (cmat) {
        DNS_TRY(dns::check_csr(cmat, "C"));
        if (cmat->nrows < 1 || cmat->ncols != h->nv)
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "recorder: C must be Ny x NV (%d columns), it is "
                             "%d x %d", h->nv, (int)cmat->nrows,
                             (int)cmat->ncols);
    }
    if (snap_slot) {
        if (nslots < 1)
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "recorder: a slot table with nslots = %d < 1",
                             (int)nslots);
        for (int r = 0; r < nrows; ++r)
            if (snap_slot[r] < -1 || snap_slot[r] >= nslots)
                return dns::fail(DNS_ERR_BAD_ARGUMENT,
                                 "recorder: snap_slot[%d] = %d outside -1..%d",
                                 r, (int)snap_slot[r], (int)nslots - 1);
    }
    DNS_TRY(quiesce(st));                       // replays may still write it
    hipStream_t s = h->stream;
    // Built aside: a refusal below leaves the recorder that was there.  What
    // that one holds is taken over where it is large enough (keep_or_alloc;
    // C where it is the same matrix).
    dns_imex::Recorder none;
    dns_imex::Recorder &old = st->rec ? *st->rec : none;
    std::unique_ptr<dns_imex::Recorder> r(new (std::nothrow)
                                              dns_imex::Recorder());
    if (!r) return dns::fail(DNS_ERR_BAD_ARGUMENT, "out of host memory");
    r->rows = nrows;
    bool keep_c = false;
    if (cmat) {
        r->Ny = cmat->nrows;
        const dns::HostCsr &oc = old.Ch;
        keep_c = old.C && oc.nrows == cmat->nrows && oc.nnz() == cmat->nnz &&
                 std::equal(oc.rowptr.begin(), oc.rowptr.end(), cmat->rowptr) &&
                 std::equal(oc.colidx.begin(), oc.colidx.end(), cmat->colidx) &&
                 std::equal(oc.vals.begin(), oc.vals.end(), cmat->vals);
        if (!keep_c) {
            r->C.reset(new (std::nothrow) dns::CsrDev());
            if (!r->C) return dns::fail(DNS_ERR_BAD_ARGUMENT, "out of host memory");
            DNS_TRY(r->C->upload(cmat, s));
            r->Ch = dns::host_copy(cmat);
        }
        DNS_TRY(keep_or_alloc(r->ylog, old.ylog, (size_t)nrows * cmat->nrows));
    }
    if (snap_slot) {
        r->nslots = nslots;
        DNS_TRY(keep_or_alloc(r->slot, old.slot, (size_t)nrows));
        DNS_TRY(keep_or_alloc(r->snap, old.snap, (size_t)nslots * h->ld));
    }
    // (nothing is refused from here on)
    if (keep_c) {
        r->C = std::move(old.C);
        r->Ch = std::move(old.Ch);
    }
    if (cmat) {
        adopt(r->ylog, old.ylog);
        DNS_TRY(r->ylog.zero(s));
    }
    if (snap_slot) {
        adopt(r->slot, old.slot);
        adopt(r->snap, old.snap);
        DNS_TRY(r->slot.upload(snap_slot, (size_t)nrows, s));
        DNS_TRY(r->snap.zero(s));
    }
    st->rec = std::move(r);
    return st->rewind_tables();
} DNS_CAPI_CATCH

static int rec_need(dns_imex *st) {
    return need(st, st && st->rec, "recorder is", "dns_imex_set_recorder");
}

int dns_imex_get_record_outputs(dns_imex *st, int32_t first, int32_t count,
                                double *y) try {
    DNS_TRY(rec_need(st));
    const dns_imex::Recorder &r = *st->rec;
    if (r.Ny < 1)
        return dns::fail(DNS_ERR_NOT_READY, "the recorder keeps no outputs");
    if (!y) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    return download_log_rows(st, y, r.ylog.p, first, count, (size_t)r.Ny,
                             r.rows, "output rows", "recorder");
} DNS_CAPI_CATCH

int dns_imex_get_record_snapshots(dns_imex *st, int32_t first_slot,
                                  int32_t count, double *v, double *p) try {
    DNS_TRY(rec_need(st));
    const dns_imex::Recorder &r = *st->rec;
    if (r.nslots < 1)
        return dns::fail(DNS_ERR_NOT_READY, "the recorder keeps no snapshots");
    const dns_saddle *h = st->sys;
    DNS_TRY(download_log_rows(st, v, r.snap.p, first_slot, count,
                              (size_t)h->nv, r.nslots, "slots", "recorder",
                              h->ld));
    return download_log_rows(st, p, r.snap.p + h->nv, first_slot, count,
                             (size_t)h->np, r.nslots, "slots", "recorder",
                             h->ld);
} DNS_CAPI_CATCH

int dns_imex_clear_recorder(dns_imex *st) try {
    return take_off(st, &dns_imex::rec);
} DNS_CAPI_CATCH

// ---- force functionals (functional.hpp) ------------------------------------

int dns_imex_set_functionals(dns_imex *st, int32_t nF, const dns_csr *ca,
                             const dns_csr *cm, const dns_csr *cp,
                             const double *c0, const double *scale,
                             const int32_t *cell_ptr, const int32_t *cell_idx,
                             const double *cell_w, double dt,
                             int32_t nrows) try {
    return set_functionals(st, nF, ca, cm, cp, nullptr, nullptr, c0, scale,
                           cell_ptr, cell_idx, cell_w, dt, nrows, 0, nullptr,
                           false);
} DNS_CAPI_CATCH

int dns_imex_set_functionals_bc(dns_imex *st, int32_t nF, const dns_csr *ca,
                                const dns_csr *cm, const dns_csr *cp,
                                const dns_csr *cab, const dns_csr *cmb,
                                const double *c0, const double *scale,
                                const int32_t *cell_ptr,
                                const int32_t *cell_idx, const double *cell_w,
                                double dt, int32_t nrows, int32_t ndbc,
                                const double *dbc_table) try {
    return set_functionals(st, nF, ca, cm, cp, cab, cmb, c0, scale, cell_ptr,
                           cell_idx, cell_w, dt, nrows, ndbc, dbc_table, true);
} DNS_CAPI_CATCH

int dns_imex_set_functionals_live(dns_imex *st, int32_t nF, const dns_csr *ca,
                                  const dns_csr *cm, const dns_csr *cp,
                                  const dns_csr *cab, const dns_csr *cmb,
                                  const double *c0, const double *scale,
                                  const int32_t *cell_ptr,
                                  const int32_t *cell_idx,
                                  const double *cell_w, double dt,
                                  int32_t nrows, int32_t ndbc) try {
    return set_functionals(st, nF, ca, cm, cp, cab, cmb, c0, scale, cell_ptr,
                           cell_idx, cell_w, dt, nrows, ndbc, nullptr, true,
                           true);
} DNS_CAPI_CATCH

int dns_imex_get_functionals(dns_imex *st, int32_t first, int32_t count,
                             double *out) try {
    DNS_TRY(need(st, st && st->fn, "functionals are",
                 "dns_imex_set_functionals"));
    return st->fn->log.download_sums(st, first, count, out, "functional rows");
} DNS_CAPI_CATCH

int dns_imex_clear_functionals(dns_imex *st) try {
    return take_off(st, &dns_imex::fn);
} DNS_CAPI_CATCH

// ---- flow statistics (stats.hpp) -------------------------------------------

int dns_imex_set_stats(dns_imex *st, int32_t nrows, const int32_t *bin,
                       int32_t nbins, int32_t npairs, const int32_t *pair_i,
                       const int32_t *pair_j, int32_t reset) try {
    if (!st || !bin) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = st->sys;
    DNS_TRY(st->refuse_partitioned("statistics", kStPartitioned));
    if (nbins < 1 || nbins > dns::kStMaxBins)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "statistics: nbins = %d outside 1..%d", (int)nbins,
                         dns::kStMaxBins);
    if (nrows < 1)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "statistics: nrows = %d < 1",
                         (int)nrows);
    if (npairs < 0 || (npairs > 0 && (!pair_i || !pair_j)))
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "statistics: npairs = %d without pair_i / pair_j",
                         (int)npairs);
    dns::StLayout lay;
    lay.G = dns::stats_grid((int)h->ld, npairs);
    lay.nbins = nbins;
    lay.ld = (int)h->ld;
    lay.npairs = npairs;
    // (the checkpoint of a batch counts in int)
    if (lay.total() >= ((size_t)1 << 31))
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "statistics: an accumulator of %zu entries (%d bins "
                         "x (2 x %d + %d)), the limit is 2^31 - 1",
                         lay.total(), (int)nbins, lay.ld, lay.npx());
    for (int r = 0; r < nrows; ++r)
        if (bin[r] < -1 || bin[r] >= nbins)
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "statistics: bin[%d] = %d outside -1..%d", r,
                             (int)bin[r], (int)nbins - 1);
    for (int q = 0; q < npairs; ++q)
        if (pair_i[q] < 0 || pair_i[q] >= h->n || pair_j[q] < 0 ||
            pair_j[q] >= h->n)
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "statistics: pair %d = (%d, %d) outside 0..%d "
                             "(NV + NP - 1)", q, (int)pair_i[q],
                             (int)pair_j[q], h->n - 1);
    DNS_TRY(quiesce(st));                       // replays may still add to it
    hipStream_t s = h->stream;
    // In place (keep_or_alloc; everything was checked above: a failed
    // allocation leaves the stepper without statistics).
    std::unique_ptr<dns_imex::Statistics> t = std::move(st->stat);
    if (!t) t.reset(new (std::nothrow) dns_imex::Statistics());
    if (!t) return dns::fail(DNS_ERR_BAD_ARGUMENT, "out of host memory");
    const bool keep = !reset && t->acc.p && t->lay.nbins == nbins &&
                      t->lay.ld == lay.ld && t->lay.npairs == npairs &&
                      std::equal(t->pi.begin(), t->pi.end(), pair_i) &&
                      std::equal(t->pj.begin(), t->pj.end(), pair_j);
    if (!keep) {
        DNS_TRY(keep_or_alloc(t->acc, t->acc, lay.total()));
        DNS_TRY(t->acc.zero(s));
        DNS_TRY(keep_or_alloc(t->pairs, t->pairs, (size_t)npairs));
        std::vector<int2> pq((size_t)npairs);
        for (int q = 0; q < npairs; ++q) pq[q] = make_int2(pair_i[q], pair_j[q]);
        if (npairs > 0) DNS_TRY(t->pairs.upload(pq.data(), pq.size(), s));
        t->pi.assign(pair_i, pair_i + npairs);
        t->pj.assign(pair_j, pair_j + npairs);
        t->lay = lay;
    }
    DNS_TRY(keep_or_alloc(t->bin, t->bin, (size_t)nrows));
    DNS_TRY(t->bin.upload(bin, (size_t)nrows, s));
    t->rows = nrows;
    st->stat = std::move(t);
    return st->rewind_tables();
} DNS_CAPI_CATCH

int dns_imex_get_stats(dns_imex *st, int32_t first_bin, int32_t count,
                       double *counts, double *s1, double *s2,
                       double *sx) try {
    DNS_TRY(need(st, st && st->stat, "statistics are", "dns_imex_set_stats"));
    const dns_imex::Statistics &t = *st->stat;
    const dns::StLayout &l = t.lay;
    const double *bins = t.acc.p + l.head();
    const size_t n = (size_t)st->sys->n, bs = l.bin_stride();
    DNS_TRY(download_log_rows(st, counts, t.acc.p + l.G, first_bin, count, 1,
                              l.nbins, "bins", "statistics"));
    DNS_TRY(download_log_rows(st, s1, bins, first_bin, count, n, l.nbins,
                              "bins", "statistics", bs));
    DNS_TRY(download_log_rows(st, s2, bins + l.ld, first_bin, count, n,
                              l.nbins, "bins", "statistics", bs));
    return download_log_rows(st, sx, bins + (size_t)2 * l.ld, first_bin,
                             count, (size_t)l.npairs, l.nbins, "bins",
                             "statistics", bs);
} DNS_CAPI_CATCH

int dns_imex_clear_stats(dns_imex *st) try {
    return take_off(st, &dns_imex::stat);
} DNS_CAPI_CATCH

// ---- quadratic functionals (quadratic.hpp) ---------------------------------

// What dns_imex_set_quadratics (`moving` false: constant Dirichlet values,
// NV x NV matrices), dns_imex_set_quadratics_bc (`moving`: matrices and rows
// NV + ndbc wide and a table of the values, (nrows + 1) x ndbc) and
// dns_imex_set_quadratics_live (`moving` and `live`: no table, the attached
// convection operator's is read) share.  Called inside the exports' exception
// barrier.
static int set_quadratics(dns_imex *st, int32_t nM, const dns_csr *mats,
                          int32_t nQ, const int32_t *mat, const int32_t *lop,
                          const int32_t *rop, const dns_csr *qa,
                          const dns_csr *qw, const double *c0,
                          const double *scale, double dt, int32_t nrows,
                          int32_t max_grid, int32_t ndbc,
                          const double *dbc_table, bool moving, bool live) {
    if (!st || !mats || !mat || !lop || !rop)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = st->sys;
    DNS_TRY(st->refuse_partitioned("quadratics", kQdPartitioned));
    // (`nv`: the width of every matrix and row, NV + ndbc with moving values)
    const int nv = h->nv + (moving ? ndbc : 0);
    const dns_csr *lin[2] = {qa, qw};
    DNS_TRY(dns::check_quadratics_args(nM, dns::kQdMaxMats, nQ,
                                       dns::kQdMaxForms, nrows, max_grid, dt,
                                       moving, live, ndbc, dbc_table, mats,
                                       mat, lop, rop, lin, nv));
    // (check_csr: every column index inside [0, ncols))
    for (int m = 0; m < nM; ++m)
        DNS_TRY(dns::check_csr(&mats[m], "quadratics: a matrix"));
    for (int t = 0; t < 2; ++t)
        if (lin[t]) DNS_TRY(dns::check_csr(lin[t], dns::kQdLinNames[t]));
    DNS_TRY(dns_imex::MovingBc::check_set(*st, "quadratics", kQdMovingBc,
                                          moving, live, ndbc, nrows));
    // (the columns behind NV are positions in the operator's values)
    if (moving && st->conv && st->conv->ndbc != ndbc)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "quadratics: ndbc = %d, the convection operator "
                         "attached has %d Dirichlet values", (int)ndbc,
                         st->conv->ndbc);
    const int G = dns::quadratic_grid(nM, nv, max_grid);
    DNS_TRY(dns::check_quadratics_log(nrows, G, nQ));
    // the same matrices as the device holds: as many, and each equal entry by
    // entry (row pointers, columns and the bytes of the values)
    dns_imex::Quadratics none;
    const dns_imex::Quadratics &old = st->qd ? *st->qd : none;
    bool same = old.rp.p && (int)old.Qh.size() == nM;
    for (int m = 0; same && m < nM; ++m) {
        const auto &o = old.Qh[m];
        const dns_csr &c = mats[m];
        same = o.rp.size() == (size_t)nv + 1 && (int64_t)o.ci.size() == c.nnz &&
               std::equal(o.rp.begin(), o.rp.end(), c.rowptr) &&
               std::equal(o.ci.begin(), o.ci.end(), c.colidx) &&
               (c.nnz == 0 ||
                memcmp(o.va.data(), c.vals, (size_t)c.nnz * sizeof(double)) == 0);
    }
    // the 2 nQ sparse rows (k, qa / qw) in one CSR
    std::vector<int> lrp, lci;
    std::vector<double> lva, sc, cc;
    dns::stack_rows(lin, 2, nQ, lrp, lci, lva);
    dns::scale_c0(scale, c0, nQ, sc, cc);
    DNS_TRY(quiesce(st));                       // replays may still write it
    hipStream_t s = h->stream;
    // In place (keep_or_alloc; everything was checked above: a failed
    // allocation leaves the stepper without quadratics).
    std::unique_ptr<dns_imex::Quadratics> q = std::move(st->qd);
    if (!q) q.reset(new (std::nothrow) dns_imex::Quadratics());
    if (!q) return dns::fail(DNS_ERR_BAD_ARGUMENT, "out of host memory");
    if (!same) {
        size_t total = 0;
        for (int m = 0; m < nM; ++m) total += (size_t)mats[m].nnz;
        q->Qh.clear();                  // (until the device holds the new ones)
        DNS_TRY(keep_or_alloc(q->rp, q->rp, (size_t)nM * (nv + 1)));
        DNS_TRY(keep_or_alloc(q->ci, q->ci, total));
        DNS_TRY(keep_or_alloc(q->va, q->va, total));
        std::vector<dns_imex::Quadratics::HostMat> held((size_t)nM);
        size_t base = 0;
        for (int m = 0; m < nM; ++m) {
            const dns_csr &c = mats[m];
            const size_t nz = (size_t)c.nnz;
            auto &o = held[m];
            o.rp.assign(c.rowptr, c.rowptr + nv + 1);
            o.ci.assign(c.colidx, c.colidx + nz);
            o.va.assign(c.vals, c.vals + nz);
            DNS_TRY(dns::upload_to(q->rp.p + (size_t)m * (nv + 1), c.rowptr,
                                   (size_t)nv + 1, s));
            if (nz > 0) {
                DNS_TRY(dns::upload_to(q->ci.p + base, c.colidx, nz, s));
                DNS_TRY(dns::upload_to(q->va.p + base, c.vals, nz, s));
            }
            q->nzbase[m] = (long long)base;
            base += nz;
        }
        for (int m = nM; m < dns::kQdMaxMats; ++m) q->nzbase[m] = 0;
        q->Qh = std::move(held);
    }
    DNS_TRY(put(q->lrp, lrp, s));
    DNS_TRY(put(q->lci, lci, s));
    DNS_TRY(put(q->lva, lva, s));
    DNS_TRY(put(q->scale, sc, s));
    DNS_TRY(put(q->c0, cc, s));
    DNS_TRY(q->log.ensure(nrows, G, nQ, s));
    DNS_TRY(q->bc.set(moving, live, ndbc, nrows, dbc_table, s));
    for (int m = 0; m < dns::kQdMaxMats; ++m) q->need[m] = 0;
    for (int k = 0; k < dns::kQdMaxForms; ++k) {
        q->mat[k] = k < nQ ? mat[k] : 0;
        q->lop[k] = k < nQ ? lop[k] : 0;
        q->rop[k] = k < nQ ? rop[k] : 0;
        if (k < nQ) q->need[mat[k]] |= rop[k] ? 2 : 1;
    }
    q->nM = nM;
    q->nQ = nQ;
    q->dt = dt;
    st->qd = std::move(q);
    return st->rewind_tables();
}

int dns_imex_set_quadratics(dns_imex *st, int32_t nM, const dns_csr *mats,
                            int32_t nQ, const int32_t *mat, const int32_t *lop,
                            const int32_t *rop, const dns_csr *qa,
                            const dns_csr *qw, const double *c0,
                            const double *scale, double dt, int32_t nrows,
                            int32_t max_grid) try {
    return set_quadratics(st, nM, mats, nQ, mat, lop, rop, qa, qw, c0, scale,
                          dt, nrows, max_grid, 0, nullptr, false, false);
} DNS_CAPI_CATCH

int dns_imex_set_quadratics_bc(dns_imex *st, int32_t nM, const dns_csr *mats,
                               int32_t nQ, const int32_t *mat,
                               const int32_t *lop, const int32_t *rop,
                               const dns_csr *qa, const dns_csr *qw,
                               const double *c0, const double *scale,
                               double dt, int32_t nrows, int32_t max_grid,
                               int32_t ndbc, const double *dbc_table) try {
    return set_quadratics(st, nM, mats, nQ, mat, lop, rop, qa, qw, c0, scale,
                          dt, nrows, max_grid, ndbc, dbc_table, true, false);
} DNS_CAPI_CATCH

int dns_imex_set_quadratics_live(dns_imex *st, int32_t nM, const dns_csr *mats,
                                 int32_t nQ, const int32_t *mat,
                                 const int32_t *lop, const int32_t *rop,
                                 const dns_csr *qa, const dns_csr *qw,
                                 const double *c0, const double *scale,
                                 double dt, int32_t nrows, int32_t max_grid,
                                 int32_t ndbc) try {
    return set_quadratics(st, nM, mats, nQ, mat, lop, rop, qa, qw, c0, scale,
                          dt, nrows, max_grid, ndbc, nullptr, true, true);
} DNS_CAPI_CATCH

int dns_imex_get_quadratics(dns_imex *st, int32_t first, int32_t count,
                            double *out) try {
    DNS_TRY(need(st, st && st->qd, "quadratics are",
                 "dns_imex_set_quadratics"));
    return st->qd->log.download_sums(st, first, count, out, "quadratic rows");
} DNS_CAPI_CATCH

int dns_imex_quadratics_grid(dns_imex *st, int32_t *grid) try {
    DNS_TRY(need(st, st && st->qd, "quadratics are",
                 "dns_imex_set_quadratics"));
    if (!grid) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    *grid = st->qd->log.G;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_imex_clear_quadratics(dns_imex *st) try {
    return take_off(st, &dns_imex::qd);
} DNS_CAPI_CATCH

// ---- snapshot ensemble (ensemble.hpp) --------------------------------------

int dns_imex_set_ensemble(dns_imex *st, int32_t nrows, const int32_t *slot,
                          int32_t nslots, int32_t reset) try {
    if (!st) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = st->sys;
    DNS_TRY(st->refuse_partitioned("ensemble", kEnsPartitioned));
    DNS_TRY(dns::check_slot_table(nrows, slot, nslots));
    const size_t ldv = dns::ens_ldv(h->nv);
    DNS_TRY(dns::check_ensemble_shape(nslots, h->nv, ldv));
    DNS_TRY(quiesce(st));                       // replays may still write it
    hipStream_t s = h->stream;
    // Built aside where it is not kept: a refusal (a failed allocation) leaves
    // the ensemble that was there.
    dns_imex::Ensemble none;
    dns_imex::Ensemble &old = st->ens ? *st->ens : none;
    const bool keep = !reset && old.E.p && old.nslots == nslots &&
                      old.ldv == ldv;
    dns::DevBuf<double> E;
    dns::DevBuf<int> tab;
    if (!keep) DNS_TRY(E.alloc((size_t)nslots * ldv));
    DNS_TRY(keep_or_alloc(tab, old.slot, (size_t)nrows));
    // (nothing is refused from here on)
    if (!st->ens) {
        st->ens.reset(new (std::nothrow) dns_imex::Ensemble());
        if (!st->ens) return dns::fail(DNS_ERR_BAD_ARGUMENT, "out of host memory");
    }
    dns_imex::Ensemble &e = *st->ens;
    if (!keep) {
        std::swap(e.E.p, E.p);
        std::swap(e.E.n, E.n);
        DNS_TRY(e.E.zero(s));
    }
    if (tab.p) {
        std::swap(e.slot.p, tab.p);
        std::swap(e.slot.n, tab.n);
    }
    DNS_TRY(e.slot.upload(slot, (size_t)nrows, s));
    e.rows = nrows;
    e.nslots = nslots;
    e.ldv = ldv;
    return st->rewind_tables();
} DNS_CAPI_CATCH

static int ens_need(dns_imex *st) {
    return need(st, st && st->ens, "ensemble is", "dns_imex_set_ensemble");
}

int dns_imex_get_ensemble(dns_imex *st, int32_t first_slot, int32_t count,
                          double *v) try {
    DNS_TRY(ens_need(st));
    const dns_imex::Ensemble &e = *st->ens;
    return download_log_rows(st, v, e.E.p, first_slot, count,
                             (size_t)st->sys->nv, e.nslots, "slots",
                             "ensemble", e.ldv);
} DNS_CAPI_CATCH

int dns_imex_ensemble_gram(dns_imex *st, const dns_csr *w, int32_t m,
                           double *g) try {
    DNS_TRY(ens_need(st));
    dns_imex::Ensemble &e = *st->ens;
    const int nv = st->sys->nv;
    if (!g) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    if (m < 1 || m > e.nslots)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "ensemble: m = %d outside 1..%d (nslots)", (int)m,
                         e.nslots);
    DNS_TRY(dns::check_ensemble_weights(w, nv));
    hipStream_t s = st->sys->stream;
    if (w) {
        // the same weights as the device holds are not uploaded again
        const dns::HostCsr &o = e.Wh;
        const bool same =
            e.W && o.nrows == w->nrows && o.nnz() == w->nnz &&
            std::equal(o.rowptr.begin(), o.rowptr.end(), w->rowptr) &&
            std::equal(o.colidx.begin(), o.colidx.end(), w->colidx) &&
            (w->nnz == 0 || memcmp(o.vals.data(), w->vals,
                                   (size_t)w->nnz * sizeof(double)) == 0);
        if (!same) {
            DNS_HIP(hipStreamSynchronize(s));
            auto W = std::make_unique<dns::EnsWeights>();
            DNS_TRY(W->upload(w, s));
            e.W = std::move(W);
            e.Wh = dns::host_copy(w);
        }
    }
    if (e.gm.n < (size_t)m * m) DNS_TRY(e.gm.alloc((size_t)m * m));
    DNS_TRY(dns::launch_ensemble_gram(e.E.p, m, nv, e.ldv,
                                      w ? e.W.get() : nullptr, e.y, e.part,
                                      e.gm.p, s));
    DNS_TRY(e.gm.download(g, (size_t)m * m, s));
    DNS_HIP(hipStreamSynchronize(s));
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_imex_ensemble_combine(dns_imex *st, int32_t m, int32_t r,
                              const double *coef, double *out) try {
    DNS_TRY(ens_need(st));
    dns_imex::Ensemble &e = *st->ens;
    const int nv = st->sys->nv;
    if (!coef || !out) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    if (m < 1 || m > e.nslots || r < 1)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "ensemble: m = %d outside 1..%d (nslots) or r = %d < "
                         "1", (int)m, e.nslots, (int)r);
    hipStream_t s = st->sys->stream;
    const std::vector<double> packed = dns::ens_pack_coef(coef, r, m);
    if (e.cf.n < packed.size()) DNS_TRY(e.cf.alloc(packed.size()));
    if (e.out.n < (size_t)r * e.ldv) DNS_TRY(e.out.alloc((size_t)r * e.ldv));
    DNS_TRY(e.cf.upload(packed.data(), packed.size(), s));
    DNS_TRY(dns::launch_ensemble_combine(e.E.p, m, nv, e.ldv, e.cf.p, r,
                                         e.out.p, e.ldv, s));
    DNS_TRY(dns::download_rows(out, (const double *)e.out.p, (size_t)r,
                               (size_t)nv, e.ldv, s));
    DNS_HIP(hipStreamSynchronize(s));
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_imex_clear_ensemble(dns_imex *st) try {
    return take_off(st, &dns_imex::ens);
} DNS_CAPI_CATCH

// Slots [first, first + count) of the ensemble become the base trajectory of
// the linearised operator `cv`, device to device on the stepper's stream (the
// slot layout is the trajectory's: one copy); only the base flow's Dirichlet
// values cross the bus.  The forward run that filled the slots and the
// linearised / adjoint run about them never meet on the host.
int dns_imex_ensemble_to_base(dns_imex *st, int32_t first, int32_t count,
                              dns_conv *cv, int32_t dbc_nrows,
                              const double *dbc_vals, int32_t adjoint) try {
    if (!st || !cv) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    static const char *const who =
        "linearised convection: base trajectory from the ensemble";
    if (!st->ens)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "%s: no ensemble is set (dns_imex_set_ensemble)", who);
    const dns_imex::Ensemble &e = *st->ens;
    dns_saddle *h = st->sys;
    DNS_TRY(dns::check_base_slots(first, count, e.nslots));
    if (cv->device != h->device)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "%s: the operator lives on device %d, the ensemble on "
                         "device %d", who, cv->device, h->device);
    if (cv->nv_inner != h->nv || dns::base_traj_ldv(cv->nv_inner) != e.ldv)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "%s: the operator has %d inner dofs, a slot holds %d",
                         who, cv->nv_inner, h->nv);
    // (the rows are on the device: only their number and the values are asked)
    DNS_TRY(dns::check_base_trajectory(count, 0, nullptr, 0, dbc_nrows,
                                       cv->ndbc, dbc_vals));
    if (adjoint)
        DNS_TRY(dns::check_adjoint_dbc(cv->dbc_host.data(), cv->ndbc,
                                       cv->dbc_rows));
    DNS_HIP(hipSetDevice(h->device));
    DNS_HIP(hipDeviceSynchronize());           // replays may still read it
    hipStream_t s = h->stream;
    const size_t len = dns::base_traj_offset(count, e.ldv);
    dns::DevBuf<double> T;
    DNS_TRY(T.alloc(len));
    DNS_HIP(hipMemcpyAsync(T.p, e.E.p + dns::base_traj_offset(first, e.ldv),
                           len * sizeof(double), hipMemcpyDeviceToDevice, s));
    return cv->adopt_base_trajectory(T, count, dbc_nrows, dbc_vals,
                                     adjoint != 0, s);
} DNS_CAPI_CATCH

// ---- the two dense operations alone (host pointers; tests) ------------------

int dns_ensemble_gram(int device, int32_t m, int32_t nv, int32_t ld,
                      const double *e, const dns_csr *w, double *g) try {
    if (!e || !g) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_TRY(dns::check_ensemble_shape(m, nv, ld < 0 ? 0 : (size_t)ld));
    DNS_TRY(dns::check_ensemble_weights(w, nv));
    DNS_HIP(hipSetDevice(device));
    ScopedStream ss;
    DNS_HIP(hipStreamCreate(&ss.s));
    dns::DevBuf<double> E, y, part, G;
    dns::EnsWeights W;
    DNS_TRY(E.alloc((size_t)m * ld));
    DNS_TRY(G.alloc((size_t)m * m));
    DNS_TRY(E.upload(e, (size_t)m * ld, ss.s));
    if (w) DNS_TRY(W.upload(w, ss.s));
    DNS_TRY(dns::launch_ensemble_gram(E.p, m, nv, (size_t)ld,
                                      w ? &W : nullptr, y, part, G.p, ss.s));
    DNS_TRY(G.download(g, (size_t)m * m, ss.s));
    DNS_HIP(hipStreamSynchronize(ss.s));
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_ensemble_project(int device, int32_t mx, int32_t my, int32_t nv,
                         int32_t ld, const double *x, const double *y,
                         const dns_csr *w, double *p) try {
    if (!x || !p) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_TRY(dns::check_ensemble_shape(mx, nv, ld < 0 ? 0 : (size_t)ld));
    DNS_TRY(dns::check_ensemble_shape(y ? my : mx, nv, (size_t)ld));
    DNS_TRY(dns::check_ensemble_weights(w, nv));
    if (!y) my = mx;
    DNS_HIP(hipSetDevice(device));
    ScopedStream ss;
    DNS_HIP(hipStreamCreate(&ss.s));
    dns::DevBuf<double> X, Y, scratch, part, P;
    dns::EnsWeights W;
    DNS_TRY(X.alloc((size_t)mx * ld));
    DNS_TRY(P.alloc((size_t)mx * my));
    DNS_TRY(X.upload(x, (size_t)mx * ld, ss.s));
    if (y) {
        DNS_TRY(Y.alloc((size_t)my * ld));
        DNS_TRY(Y.upload(y, (size_t)my * ld, ss.s));
    }
    if (w) DNS_TRY(W.upload(w, ss.s));
    DNS_TRY(dns::launch_ensemble_project(X.p, mx, (size_t)ld, y ? Y.p : X.p, my,
                                         (size_t)ld, nv, w ? &W : nullptr,
                                         scratch, part, P.p, ss.s));
    DNS_TRY(P.download(p, (size_t)mx * my, ss.s));
    DNS_HIP(hipStreamSynchronize(ss.s));
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_ensemble_combine(int device, int32_t m, int32_t nv, int32_t ld,
                         const double *e, int32_t r, const double *coef,
                         double *out) try {
    if (!e || !coef || !out)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_TRY(dns::check_ensemble_shape(m, nv, ld < 0 ? 0 : (size_t)ld));
    if (r < 1)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "ensemble: r = %d < 1", (int)r);
    DNS_HIP(hipSetDevice(device));
    ScopedStream ss;
    DNS_HIP(hipStreamCreate(&ss.s));
    dns::DevBuf<double> E, C, O;
    const size_t ldo = ((size_t)nv + 1) & ~(size_t)1;
    DNS_TRY(E.alloc((size_t)m * ld));
    const std::vector<double> packed = dns::ens_pack_coef(coef, r, m);
    DNS_TRY(C.alloc(packed.size()));
    DNS_TRY(O.alloc((size_t)r * ldo));
    DNS_TRY(E.upload(e, (size_t)m * ld, ss.s));
    DNS_TRY(C.upload(packed.data(), packed.size(), ss.s));
    DNS_TRY(dns::launch_ensemble_combine(E.p, m, nv, (size_t)ld, C.p, r, O.p,
                                         ldo, ss.s));
    DNS_TRY(dns::download_rows(out, (const double *)O.p, (size_t)r, (size_t)nv,
                               ldo, ss.s));
    DNS_HIP(hipStreamSynchronize(ss.s));
    return DNS_OK;
} DNS_CAPI_CATCH

}  // extern "C"
