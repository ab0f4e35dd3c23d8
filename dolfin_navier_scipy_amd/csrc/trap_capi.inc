// extern "C" entry points of the Newton/Picard trapezoidal stepper (included
// by dns_amd.hip)

// What a step's right-hand side needs of the CURRENT velocity (snu:1034-1035,
// 1529-1537): f_c - C_c v_c with C_c = A + N_c.  Its convection part is a VECTOR
// whatever the linearisation: with the boundary terms,
//   Picard:  -N1(u)[inner, :] u                  = -N(u)u
//   Newton:  -(N1 + N2)(u)[inner, :] u + N(u)u   = -N(u)u
// (u the velocity with its Dirichlet values; N1(u)u = N2(u)u = N(u)u is the
// reference's own known-answer test, tests/test_units_fenicsci.py:84-85).  So
// no matrix is assembled for it: the cell values of the convection vector of
// the current velocity are taken by extra workgroups of the step's element
// launch (k_conv_step_cells) and gathered by the rows that form the right-hand
// side (TrapRhs in k_conv_mat_bc_gather).

// The cells that touch this rank's rows, the non-zeros of its rows of F, and
// the halo plan of a velocity = footprint of its rows of K and of those cells
// (every rank computes every rank's lists from the replicated patterns, as
// dns_imex::ensure_partition does).  Off on an un-partitioned handle.
int dns_trap::ensure_partition() {
    dns_saddle *h = sys;
    const bool want = h->dist() && h->dist_sliced && h->dd && !h->rank_local;
    if (!want) {
        part.on = false;
        return DNS_OK;
    }
    if (part.on && part.gen == h->dist_generation) return DNS_OK;
    const int P = h->comm->nranks, me = h->comm->rank, nv = h->nv;
    const std::vector<int> &stv = h->st_v;
    const int nc_all = conv->ncells;
    std::vector<std::vector<std::vector<int>>> need((size_t)P);
    std::vector<int> mysel;
    for (int r = 0; r < P; ++r) {
        std::vector<unsigned char> cm((size_t)nc_all, 0), dm((size_t)nv, 0);
        for (int row = stv[r]; row < stv[r + 1]; ++row)
            for (int k = conv->gptr_host[row]; k < conv->gptr_host[row + 1]; ++k)
                cm[conv->gidx_host[k] % nc_all] = 1;
        for (int cl = 0; cl < nc_all; ++cl) {
            if (!cm[cl]) continue;
            if (r == me) mysel.push_back(cl);
            for (int k = 0; k < 12; ++k) {
                const int m = conv->cmap_host[(size_t)k * nc_all + cl];
                if (m >= 0) dm[m] = 1;
            }
        }
        need[r].assign((size_t)P, std::vector<int>());
        for (int q = 0; q < P; ++q) {
            if (q == r) continue;
            std::vector<int> c;
            for (int d = stv[q]; d < stv[q + 1]; ++d)
                if (dm[d]) c.push_back(d);
            const std::vector<int> &kq = h->dd->needK[r][q];
            std::set_union(c.begin(), c.end(), kq.begin(), kq.end(),
                           std::back_inserter(need[r][q]));
        }
    }
    DNS_TRY(part.planX.build(need, me, P, h->stream));
    part.nsel = (int)mysel.size();
    DNS_TRY(part.sel.alloc((size_t)std::max(1, part.nsel)));
    if (part.nsel)
        DNS_TRY(part.sel.upload(mysel.data(), mysel.size(), h->stream));
    part.v0 = stv[me];
    part.v1 = stv[me + 1];
    part.z0 = h->Fh.rowptr[part.v0];
    part.z1 = h->Fh.rowptr[part.v1];
    part.nhalo = part.planX.nrecv;
    DNS_HIP(hipStreamSynchronize(h->stream));
    part.on = true;
    part.gen = h->dist_generation;
    return DNS_OK;
}

// a trajectory slot holds a rank's rows and its halo: every rank's rows
// everywhere before somebody reads the whole (collective)
int dns_trap::gather_slot(int which, int slot) {
    dns_saddle *h = sys;
    if (!h->dist()) return DNS_OK;
    return h->comm->allgatherv(traj[which].p + (size_t)slot * h->nv, h->st_v,
                               h->stream);
}

// the partials a pipelined batch has left in the ring -> updnorm_dev
int dns_trap::flush_pending_upd() {
    if (!pend.on) return DNS_OK;
    pend.on = false;
    const dns::UpdJob &u = pend.job;
    DNS_LPR_SWITCH(u.lpr,
                   hipLaunchKernelGGL(dns::k_trap_updnorm<L>, u.nblk,
                                      dns::kBlock, 0, sys->stream, u.nv,
                                      u.rowptr, u.colidx, u.mvals, u.x, u.y,
                                      u.part, u.copy_out, 0, u.nv,
                                      (const int *)nullptr, 0, u.scale));
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}

int dns_trap::flush_updnorm() {
    DNS_TRY(flush_pending_upd());
    if (upd_slot == 0) return DNS_OK;
    hipLaunchKernelGGL(dns::k_trap_acc, 1, dns::kBlock, 0, sys->stream,
                       upd_ring.p, upd_slot * upd_stride, 1.0, updnorm_dev.p);
    DNS_HIP(hipGetLastError());
    upd_slot = 0;
    return DNS_OK;
}

// the part of the update norm still on the device, added to `updnorm`
// (synchronises the stream)
int dns_trap::collect_updnorm() {
    double dd = 0.0;
    DNS_TRY(flush_updnorm());
    DNS_TRY(updnorm_dev.download(&dd, 1, sys->stream));
    DNS_HIP(hipStreamSynchronize(sys->stream));
    updnorm += dd;
    return updnorm_dev.zero(sys->stream);
}

extern "C" {

int dns_trap_create(dns_saddle *sys, dns_conv *conv, const double *m_vals,
                    const double *a_vals, int32_t nslots, dns_trap **out) try {
    if (!sys || !conv || !m_vals || !a_vals || !out || nslots < 1)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    *out = nullptr;
    DNS_TRY(conv->refuse_linearised("the trapezoidal stepper"));
    DNS_HIP(hipSetDevice(sys->device));
    // row-partitioned handle: the assembly is REPLICATED (every rank forms all
    // of N(v_lin), F and the right-hand side: element work, a few SpMVs), the
    // solve -- the expensive part -- is partitioned; the solution is gathered
    // after every step.  F comes back to the device for that.
    DNS_TRY(sys->ensure_F_device());
    if (!conv->mat || conv->mat->nnz != (int)sys->F.nnz ||
        conv->nv_inner != sys->nv)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "bind the convection operator to the pattern of the "
                         "system's F block first (dns_conv_bind_pattern)");
    auto t = std::make_unique<dns_trap>();
    t->sys = sys;
    t->conv = conv;
    t->nslots = nslots;
    if (const char *fe = getenv("DNS_TRAP_FUSE_R")) t->env_fuse_r = fe[0] != '0';
    if (const char *ge = getenv("DNS_TRAP_GRAPH")) t->env_graph = ge[0] != '0';
    if (const char *ue = getenv("DNS_TRAP_UPD_RIDE"))
        t->env_upd_ride = ue[0] != '0';
    const size_t nnz = (size_t)sys->F.nnz, nv = (size_t)sys->nv;
    DNS_TRY(t->mvals.alloc(nnz));
    DNS_TRY(t->avals.alloc(nnz));
    DNS_TRY(t->nn_vals.alloc(nnz));
    for (int i = 0; i < 6; ++i) DNS_TRY(t->xs[i].alloc(sys->ld));
    DNS_TRY(t->fv.alloc(nv));
    DNS_TRY(t->fp.alloc((size_t)std::max(1, sys->np)));
    DNS_TRY(t->fvn_n.alloc(nv));
    DNS_TRY(t->rhsbc.alloc(nv));
    DNS_TRY(t->rhscon.alloc(nv));
    DNS_TRY(t->b.alloc(sys->ld));
    DNS_TRY(t->dtmp.alloc(nv));
    DNS_TRY(t->mtmp.alloc(nv));
    for (int w = 0; w < 2; ++w)
        DNS_TRY(t->traj[w].alloc((size_t)nslots * nv));
    DNS_TRY(t->updnorm_dev.alloc(1));
    DNS_TRY(t->mvals.upload(m_vals, nnz, sys->stream));
    DNS_TRY(t->avals.upload(a_vals, nnz, sys->stream));
    DNS_TRY(t->fv.zero(sys->stream));
    DNS_TRY(t->fp.zero(sys->stream));
    for (int w = 0; w < 2; ++w) DNS_TRY(t->traj[w].zero(sys->stream));
    DNS_TRY(t->updnorm_dev.zero(sys->stream));
    if (!sys->dist_sliced) {
        DNS_TRY(t->kpos.alloc(nnz));
        hipLaunchKernelGGL(dns::k_trap_kpos, dns::grid_for_rows(sys->nv, 8),
                           dns::kBlock, 0, sys->stream, sys->nv,
                           sys->F.rowptr.p, sys->K.rowptr.p, t->kpos.p);
    }
    if (hipStreamSynchronize(sys->stream) != hipSuccess)
        return dns::fail(DNS_ERR_HIP, "stream sync failed");
    *out = t.release();
    return DNS_OK;
} DNS_CAPI_CATCH

void dns_trap_destroy(dns_trap *t) {
    if (!t) return;
    (void)hipSetDevice(t->sys->device);
    (void)hipStreamSynchronize(t->sys->stream);
    // (exports nobody waited for are dropped: their arrays may be gone)
    {
        std::lock_guard<std::mutex> lock(t->exp_.mu);
        if (t->exp_.cstream) (void)hipStreamSynchronize(t->exp_.cstream);
        for (auto &j : t->exp_.jobs) (void)hipHostFree(j.stage);
        t->exp_.jobs.clear();
    }
    if (t->exp_.cstream) (void)hipStreamDestroy(t->exp_.cstream);
    if (t->exp_.ready) (void)hipEventDestroy(t->exp_.ready);
    for (int w = 0; w < 2; ++w)
        if (t->exp_.done[w]) (void)hipEventDestroy(t->exp_.done[w]);
    delete t;
}

// Queue the copy of slots [slot0, slot0 + count) of traj[which] (count * NV
// doubles; into a page-locked buffer of the library's, handed to `host` by
// dns_trap_traj_export_wait) on the copy stream, behind everything the
// solver's stream has been given so far.  Returns at once; the solver's stream goes on with the
// next sweep and only waits if it is about to overwrite traj[which].
int dns_trap_traj_export_async(dns_trap *t, int32_t which, int32_t slot0,
                               int32_t count, double *host) try {
    if (!t || !host || which < 0 || which > 1 || slot0 < 0 || count < 1 ||
        slot0 + count > t->nslots)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    dns_saddle *h = t->sys;
    DNS_HIP(hipSetDevice(h->device));
    std::lock_guard<std::mutex> lock(t->exp_.mu);
    dns_trap::Export &e = t->exp_;
    if (!e.cstream)
        DNS_HIP(hipStreamCreateWithFlags(&e.cstream, hipStreamNonBlocking));
    if (!e.ready)
        DNS_HIP(hipEventCreateWithFlags(&e.ready, hipEventDisableTiming));
    for (int w = 0; w < 2; ++w)
        if (!e.done[w])
            DNS_HIP(hipEventCreateWithFlags(&e.done[w],
                                            hipEventDisableTiming));
    const size_t bytes = (size_t)count * h->nv * sizeof(double);
    DNS_TRY(t->flush_pending_upd());
    // (partitioned assembly: a slot holds a rank's rows and its halo --
    // every rank's rows everywhere first; collective)
    if (t->part.on)
        for (int k = 0; k < count; ++k)
            DNS_TRY(t->gather_slot(which, slot0 + k));
    void *stage = nullptr;
    DNS_HIP(hipHostMalloc(&stage, bytes, hipHostMallocDefault));
    e.jobs.push_back({host, stage, bytes});
    dns::log_host_copy("export (at the wait)", host, t->traj[which].p, bytes);
    DNS_HIP(hipEventRecord(e.ready, h->stream));
    DNS_HIP(hipStreamWaitEvent(e.cstream, e.ready, 0));
    DNS_TRY(dns::d2h_pinned(static_cast<double *>(stage),
                            t->traj[which].p + (size_t)slot0 * h->nv,
                            (size_t)count * h->nv, e.cstream));
    DNS_HIP(hipEventRecord(e.done[which], e.cstream));
    e.pending[which] = true;
    return DNS_OK;
} DNS_CAPI_CATCH

// blocks until every queued export has arrived (any host thread may call it)
int dns_trap_traj_export_wait(dns_trap *t) try {
    if (!t) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_HIP(hipSetDevice(t->sys->device));
    std::lock_guard<std::mutex> lock(t->exp_.mu);
    dns_trap::Export &e = t->exp_;
    if (e.cstream) DNS_HIP(hipStreamSynchronize(e.cstream));
    for (auto &j : e.jobs) {
        memcpy(j.host, j.stage, j.bytes);
        (void)hipHostFree(j.stage);
    }
    e.jobs.clear();
    e.pending[0] = e.pending[1] = false;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_trap_set_rhs(dns_trap *t, const double *fv, const double *fp) try {
    if (!t) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = t->sys;
    DNS_HIP(hipSetDevice(h->device));
    if (fv)
        DNS_TRY(t->fv.upload(fv, (size_t)h->nv, h->stream));
    else
        DNS_TRY(t->fv.zero(h->stream));
    if (fp)
        DNS_TRY(t->fp.upload(fp, (size_t)h->np, h->stream));
    else
        DNS_TRY(t->fp.zero(h->stream));
    DNS_HIP(hipStreamSynchronize(h->stream));
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_trap_traj_write(dns_trap *t, int32_t which, int32_t slot,
                        const double *v) try {
    if (!t || !v || which < 0 || which > 1 || slot < 0 || slot >= t->nslots)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    dns_saddle *h = t->sys;
    DNS_HIP(hipSetDevice(h->device));
    DNS_TRY(t->flush_pending_upd());   // (it may store a slot of this buffer)
    DNS_TRY(t->export_fence(which));
    DNS_TRY(dns::upload_to(t->traj[which].p + (size_t)slot * h->nv, v,
                           (size_t)h->nv, h->stream));
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_trap_traj_read(dns_trap *t, int32_t which, int32_t slot,
                       double *v) try {
    if (!t || !v || which < 0 || which > 1 || slot < 0 || slot >= t->nslots)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    dns_saddle *h = t->sys;
    DNS_HIP(hipSetDevice(h->device));
    DNS_TRY(t->flush_pending_upd());
    if (t->part.on) DNS_TRY(t->gather_slot(which, slot));
    DNS_TRY(dns::download_from(v, t->traj[which].p + (size_t)slot * h->nv,
                               (size_t)h->nv, h->stream));
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_trap_start(dns_trap *t, const double *iniv, int32_t newton) try {
    if (!t || !iniv) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = t->sys;
    DNS_HIP(hipSetDevice(h->device));
    t->reset(1);
    for (int i = 0; i < 6; ++i) DNS_TRY(t->xs[i].zero(h->stream));
    DNS_TRY(t->xs[0].upload(iniv, (size_t)h->nv, h->stream));
    t->updnorm = 0.0;
    t->pipeline_c = 0;
    t->cur_slot = 0;
    t->conv->dbc_ctr = nullptr;
    t->conv->dbc_row = 0;
    DNS_TRY(t->updnorm_dev.zero(h->stream));
    t->upd_slot = 0;
    t->pend.on = false;
    (void)newton;            // (N_c, f_c: taken by the first step, snu:1351,1364)
    DNS_HIP(hipStreamSynchronize(h->stream));
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_trap_step(dns_trap *t, double dt, int32_t lin_which, int32_t lin_slot,
                  int32_t out_slot, int32_t newton, int32_t extrapolate_x0,
                  const dns_solve_opts *opts, dns_solve_stats *stats) try {
    if (!t) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    return t->step_impl(dt, lin_which, lin_slot, out_slot, newton,
                        extrapolate_x0, opts, stats, nullptr);
} DNS_CAPI_CATCH

// `count` pipelined steps of one step size in a row, slots slot0 ..
// slot0 + count - 1 (linearisation point and output slot of a step are its
// time instance, as the sweeps of the reference have it): the per-step trip
// through the caller's language (15-20 us in Python, a fifth of a step at
// N = 2) happens once per batch
int dns_trap_run(dns_trap *t, double dt, int32_t lin_which, int32_t slot0,
                 int32_t count, int32_t newton, int32_t extrapolate_x0,
                 const dns_solve_opts *opts) try {
    if (!t || count < 0 || slot0 < 0 || slot0 + count > t->nslots)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    if (t->pipeline_c <= 0)
        return dns::fail(DNS_ERR_NOT_READY,
                         "dns_trap_run: pipelined steps only "
                         "(dns_trap_set_pipeline)");
    dns_solve_stats st;
    for (int k = 0; k < count; ++k)
        DNS_TRY(t->step_impl(dt, lin_which, slot0 + k, slot0 + k, newton,
                             extrapolate_x0, opts, &st, nullptr));
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_trap_step_fb(dns_trap *t, double dt, int32_t lin_which,
                     int32_t lin_slot, int32_t out_slot, int32_t newton,
                     int32_t extrapolate_x0, const dns_solve_opts *opts,
                     dns_solve_stats *stats, int32_t r, const double *umat,
                     const double *vmat_c, const double *vmat_n) try {
    if (!t || r < 1 || r > 64 || !umat || !vmat_n)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    if (t->pipeline_c > 0)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "steps with low-rank feedback are synchronous");
    const dns_trap::Feedback fb = {r, umat, vmat_c, vmat_n};
    return t->step_impl(dt, lin_which, lin_slot, out_slot, newton,
                        extrapolate_x0, opts, stats, &fb);
} DNS_CAPI_CATCH

int dns_trap_set_tables(dns_trap *t, const double *fv_tab, const double *fp_tab,
                        const double *mbc_tab) try {
    if (!t) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = t->sys;
    DNS_HIP(hipSetDevice(h->device));
    DNS_HIP(hipStreamSynchronize(h->stream));
    const size_t nv = (size_t)h->nv, np = (size_t)std::max(1, h->np),
                 ns = (size_t)t->nslots;
    t->have_fv_tab = fv_tab != nullptr;
    t->have_fp_tab = fp_tab != nullptr;
    t->have_mbc_tab = mbc_tab != nullptr;
    if (fv_tab) {
        if (t->fv_tab.n < nv * ns) DNS_TRY(t->fv_tab.alloc(nv * ns));
        DNS_TRY(t->fv_tab.upload(fv_tab, nv * ns, h->stream));
    }
    if (fp_tab) {
        if (t->fp_tab.n < np * ns) DNS_TRY(t->fp_tab.alloc(np * ns));
        DNS_TRY(t->fp_tab.upload(fp_tab, (size_t)h->np * ns, h->stream));
    }
    if (mbc_tab) {
        if (t->mbc_tab.n < nv * ns) DNS_TRY(t->mbc_tab.alloc(nv * ns));
        DNS_TRY(t->mbc_tab.upload(mbc_tab, nv * ns, h->stream));
    }
    DNS_HIP(hipStreamSynchronize(h->stream));
    return DNS_OK;
} DNS_CAPI_CATCH

}  // extern "C"

// host-side solve of the r x r Sherman-Morrison-Woodbury system (partial
// pivoting); false: singular
static bool small_solve(int r, std::vector<double> &a, std::vector<double> &b) {
    for (int k = 0; k < r; ++k) {
        int piv = k;
        for (int i = k + 1; i < r; ++i)
            if (std::fabs(a[(size_t)i * r + k]) > std::fabs(a[(size_t)piv * r + k]))
                piv = i;
        if (a[(size_t)piv * r + k] == 0.0) return false;
        if (piv != k) {
            for (int j = 0; j < r; ++j)
                std::swap(a[(size_t)k * r + j], a[(size_t)piv * r + j]);
            std::swap(b[k], b[piv]);
        }
        for (int i = k + 1; i < r; ++i) {
            const double f = a[(size_t)i * r + k] / a[(size_t)k * r + k];
            for (int j = k; j < r; ++j)
                a[(size_t)i * r + j] -= f * a[(size_t)k * r + j];
            b[i] -= f * b[k];
        }
    }
    for (int k = r - 1; k >= 0; --k) {
        for (int j = k + 1; j < r; ++j) b[k] -= a[(size_t)k * r + j] * b[j];
        b[k] /= a[(size_t)k * r + k];
    }
    return true;
}

int dns_trap::export_fence(int which) {
    std::lock_guard<std::mutex> lock(exp_.mu);
    if (exp_.pending[which])
        DNS_HIP(hipStreamWaitEvent(sys->stream, exp_.done[which], 0));
    return DNS_OK;
}

// The front part of a step: everything it enqueues before its solve -- the
// warm start, the element launch (k_conv_step_cells) and the gather launch
// (k_conv_mat_bc_gather: N, F into the system, the right-hand side and, fused,
// the start residual with its norms).  `x_given`: the work buffer holds the
// warm start already (dns_trap_assembly_probe: the caller's).
int dns_trap::enqueue_front(double dt, int lin_which, int lin_slot, int newton,
                            int extrapolate_x0, const dns_solve_opts &o,
                            const Feedback *fb, bool x_given, Front *out) {
    dns_trap *t = this;
    dns_saddle *h = t->sys;
    dns_conv *cv = t->conv;
    hipStream_t s = h->stream;
    const int nv = h->nv, np = h->np, n = h->n;
    const int nw = newton ? 1 : 0;
    const double hdt = 0.5 * dt;
    DNS_TRY(cv->refuse_linearised("the trapezoidal stepper"));
    DNS_TRY(h->ensure_F_device());      // (a re-set-up slices the handle again)
    const double *vlin = t->traj[lin_which].p + (size_t)lin_slot * nv;
    // boundary values of the new time instance (controlled boundaries)
    cv->dbc_ctr = nullptr;
    cv->dbc_row = lin_slot;
    DNS_HIP(hipEventRecord(h->ev0, s));
    // N_n, F = M + dt/2 (A + N_n) straight into the system, f_n  (snu:1443-1459)
    // (Newton: N(v_lin) v_lin -- its cell values; the gather rides along in
    // the assembly kernel's boundary part)
    DNS_TRY(t->ensure_partition());
    const bool pon = t->part.on;
    const int rv0 = pon ? t->part.v0 : 0, rv1 = pon ? t->part.v1 : nv;
    if (fb && pon) {
        // (the low-rank terms take inner products with whole vectors)
        DNS_TRY(h->comm->allgatherv(t->xs[t->cur].p, h->st_v, s));
    }
    const int *csel = pon ? t->part.sel.p : (const int *)nullptr;
    const int ncsel = pon ? t->part.nsel : 0;
    // warm start (snu:1493-1503 `krylovini='upd'`, one order higher when the
    // history allows; p~ scales with dt, so only for an unchanged step size)
    double *x = t->xs[t->work].p;
    const bool same_dt = t->last_dt > 0.0 &&
                         std::fabs(dt - t->last_dt) <= 1e-12 * dt;
    // (the order is capped at the quartic: kExtrapFit35 runs as the quartic)
    const int ex = std::min(extrapolate_x0, 4);
    const bool use_pre = t->pre_ok &&
                         t->pre_sig == dns::extrap_sig(t->nsol, extrapolate_x0) &&
                         same_dt && std::fabs(dt - t->pre_dt) <= 1e-12 * dt;
    t->pre_ok = false;
    if (!use_pre && !x_given) {
        // (else the tail of the step before has left the warm start in `x`)
        double e[5];
        const int order = same_dt ? dns::extrap_coeffs(t->nsol, ex, e) : 0;
        DNS_TRY(dns::enqueue_extrap(order, t->xs, *t, x, n, s));
    }
    // ONE launch for the element work: local matrices about v_lin, the cell
    // values of the CURRENT velocity (f_c - N_c v_c, with the boundary values
    // of its own time instance) and -- Newton -- those of v_lin
    // (round 5) the start residual r = b - K x0 and the partials of both
    // norms come out of the gather launch -- no residual kernel in front of
    // the Krylov cycle -- where nothing touches b behind it (no boundary-mass
    // table, no low-rank terms) and the rows are all here
    // (workgroups of the gather launch's row part: sixteen lanes per
    // velocity row and -- with the residual -- per pressure row, the latter
    // in workgroups of their own at the end; one pair of norm partials each)
    const int gb_vel = std::max(1, std::min((16 * (rv1 - rv0) +
                                             dns::kBlock - 1) / dns::kBlock,
                                            2048));
    const int gb_prs_fused = std::max(1, std::min((16 * np + dns::kBlock - 1) /
                                                      dns::kBlock, 256));
    const bool fuse_r = t->env_fuse_r && !pon && !fb && !t->have_mbc_tab &&
                        o.method == DNS_METHOD_GMRES && !h->dist() &&
                        !h->streams(h->K) && h->JT.rowptr.p && h->J.rowptr.p &&
                        (size_t)(gb_vel + gb_prs_fused) <= h->partR.n;
    // (the update norm of the step before rides along, dns::UpdJob -- unless
    // this step reads the trajectory that job stores a slot of)
    if (t->pend.on && (t->pend.out_which == lin_which || pon))
        DNS_TRY(t->flush_pending_upd());
    const bool ride = t->pend.on;
    const dns::UpdJob job = t->pend.job;
    t->pend.on = false;
    DNS_TRY(cv->enqueue_step_cells(vlin, nw, t->xs[t->cur].p,
                                   t->cur_slot - lin_slot, s, csel, ncsel,
                                   fuse_r ? x : (const double *)nullptr,
                                   ride ? &job : (const dns::UpdJob *)nullptr));
    // (un-partitioned handle: the assembly kernel writes the new values into
    // the assembled K as well; a row block of K is re-valued from F)
    const bool kdirect = !h->dist_sliced && t->kpos.p != nullptr;
    const dns_conv::RowRange rr = {t->part.z0, t->part.z1, rv0, rv1};
    // (the right-hand side (snu:1034-1035), from N_c, f_c of the previous
    // step's end, is formed by the row part of the same launch)
    const int gb_prs = fuse_r ? gb_prs_fused : 0;
    const int gb_rows = gb_vel + gb_prs;
    dns::TrapRhs trhs = {h->F.rowptr.p, h->F.colidx.p, t->xs[t->cur].p,
                         (const double *)nullptr, t->fp_at(lin_slot),
                         t->b.p, nv, np,
                         cv->gptr.p, cv->gidx.p, cv->cellvals_c.p,
                         t->fv_at(t->cur_slot),
                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                         nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    if (fuse_r) {
        trhs.pblocks = gb_prs;
        trhs.x0 = x;
        trhs.cx0 = cv->cellvals_x0.p;
        trhs.jt_rp = h->JT.rowptr.p;
        trhs.jt_ci = h->JT.colidx.p;
        trhs.jt_v = h->JT.vals.p;
        trhs.j_rp = h->J.rowptr.p;
        trhs.j_ci = h->J.colidx.p;
        trhs.j_v = h->J.vals.p;
        trhs.r = h->r.p;
        trhs.partR = h->partR.p;
        trhs.partB = h->partB.p;
    }
    DNS_TRY(cv->enqueue_mat_bc_gather(
        t->nn_vals.p, t->mvals.p, t->avals.p, hdt, h->F.vals.p, t->rhsbc.p,
        t->fv_at(lin_slot), nw ? t->rhscon.p : (const double *)nullptr,
        t->fvn_n.p, s, kdirect ? t->kpos.p : (const int *)nullptr,
        kdirect ? h->K.vals.p : (double *)nullptr, nw != 0,
        pon ? &rr : (const dns_conv::RowRange *)nullptr, &trhs));
    DNS_TRY(h->device_values_changed(kdirect, pon));
    *out = Front{x, vlin, pon, fuse_r, rv0, rv1, ex, gb_rows};
    return DNS_OK;
}

int dns_trap::step_impl(double dt, int lin_which, int lin_slot, int out_slot,
                        int newton, int extrapolate_x0,
                        const dns_solve_opts *opts, dns_solve_stats *stats,
                        const Feedback *fb) {
    dns_trap *t = this;
    if (!(dt > 0.0) || lin_which < 0 || lin_which > 1 || lin_slot < 0 ||
        lin_slot >= t->nslots || out_slot >= t->nslots)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    dns_saddle *h = t->sys;
    if (!h->precond_ready)
        return dns::fail(DNS_ERR_NOT_READY, "preconditioner not set up");
    DNS_HIP(hipSetDevice(h->device));
    dns_solve_opts o;
    if (opts)
        o = *opts;
    else
        dns_default_solve_opts(&o);
    dns_solve_stats local;
    dns_solve_stats *st = stats ? stats : &local;
    memset(st, 0, sizeof(*st));
    hipStream_t s = h->stream;
    const int nv = h->nv, np = h->np, n = h->n;
    const double hdt = 0.5 * dt;
    // warm start, element launch, gather launch: N_n, F into the system, the
    // right-hand side and -- fused -- the start residual
    Front fr;
    DNS_TRY(t->enqueue_front(dt, lin_which, lin_slot, newton, extrapolate_x0, o,
                             fb, false, &fr));
    double *x = fr.x;
    const double *vlin = fr.vlin;
    const bool pon = fr.pon, fuse_r = fr.fuse_r;
    const int rv0 = fr.rv0, rv1 = fr.rv1, ex = fr.ex, gb_rows = fr.gb_rows;
    if (t->have_mbc_tab) {
        // rhs += mbcs_n - mbcs_c (snu:1044-1045)
        hipLaunchKernelGGL(dns::k_axpby, dns::grid_for_elems(nv), dns::kBlock,
                           0, s, (int64_t)nv, 1.0,
                           t->mbc_tab.p + (size_t)lin_slot * nv, 1.0, t->b.p);
        hipLaunchKernelGGL(dns::k_axpby, dns::grid_for_elems(nv), dns::kBlock,
                           0, s, (int64_t)nv, -1.0,
                           t->mbc_tab.p + (size_t)t->cur_slot * nv, 1.0,
                           t->b.p);
    }
    if (fb) {
        // rhs += dt/2 U (V_c v_c)   (snu:1040)
        const size_t nr = (size_t)fb->r * nv;
        if (t->fb_u.n < nr) {
            DNS_TRY(t->fb_u.alloc(nr));
            DNS_TRY(t->fb_vc.alloc(nr));
            DNS_TRY(t->fb_vn.alloc(nr));
        }
        if (t->fb_y.n < (size_t)fb->r * h->ld)
            DNS_TRY(t->fb_y.alloc((size_t)fb->r * h->ld));
        DNS_TRY(t->fb_u.upload(fb->umat, nr, s));
        DNS_TRY(t->fb_vn.upload(fb->vmat_n, nr, s));
        if (fb->vmat_c) {
            DNS_TRY(t->fb_vc.upload(fb->vmat_c, nr, s));
            for (int j = 0; j < fb->r; ++j) {
                double wj = 0.0;
                DNS_TRY(h->dot_host(nv, t->fb_vc.p + (size_t)j * nv,
                                    t->xs[t->cur].p, &wj));
                hipLaunchKernelGGL(dns::k_axpby, dns::grid_for_elems(nv),
                                   dns::kBlock, 0, s, (int64_t)nv, hdt * wj,
                                   t->fb_u.p + (size_t)j * nv, 1.0, t->b.p);
            }
        }
    }
    DNS_HIP(hipGetLastError());
    h->want_history = false;
    const bool async = t->pipeline_c > 0 && o.method == DNS_METHOD_GMRES;
    int rc;
    if (o.method == DNS_METHOD_GMRES) {
        // the tail kernel of the solve leaves the NEXT step's warm start in
        // the buffer that becomes its work buffer (today's oldest solution:
        // read by today's warm start only) -- one vector kernel per step less;
        // on a partitioned handle the solution is gathered behind the solve,
        // the warm start stays a kernel of its own there
        const int nn = std::min(t->nsol + 1, 5);
        double e[5];
        dns::StepHooks hk;
        if (!h->dist() && !fb && dns::extrap_coeffs(nn, ex, e) >= 1)
            hk.tail_extrap = dns::TailExtrap{
                t->xs[t->cur].p, t->xs[t->prev].p, t->xs[t->pprev].p,
                t->xs[t->p3].p,  e[0], e[1], e[2], e[3], e[4], t->xs[t->p4].p};
        // pipelined sweep: one cycle of the agreed length, nobody waits; the
        // device counts steps / failures for dns_trap_poll (as dns_imex_run)
        if (async) h->pipeline_c = t->pipeline_c;
        if (async && !h->dist() && !t->env_graph) o.use_graph = 0;
        // (partitioned assembly: the preconditioned vectors travel over the
        // stepper's halo, the new iterate is valid wherever this rank reads)
        hk.z_plan = pon ? &t->part.planX : nullptr;
        if (fuse_r) {
            // (the assembly launch has left r and the partials of both norms)
            hk.prologue_key = 0x7f05u;
            hk.prologue_has_resid = true;
            hk.resid_nparts = gb_rows;
        }
        rc = h->gmres(t->b.p, x, &o, st, &hk);
        h->pipeline_c = 0;
        if (hk.tail_extrap.out && rc == DNS_OK) {
            t->pre_ok = true;
            t->pre_sig = dns::extrap_sig(nn, extrapolate_x0);
            t->pre_dt = dt;
        }
    } else {
        rc = h->bicgstab(t->b.p, x, &o, st);
    }
    h->want_history = true;
    if (rc != DNS_OK) return rc;
    if (h->dist() && (!pon || fb || o.method != DNS_METHOD_GMRES)) {
        // replicated assembly (or low-rank terms): every rank works with the
        // whole velocity -- gather the row blocks of the new iterate
        DNS_TRY(h->comm->allgatherv(x, h->st_v, s));
        if (np > 0) DNS_TRY(h->comm->allgatherv(x + nv, h->st_p, s));
    }
    if (fb && st->status == DNS_OK) {
        // Sherman-Morrison-Woodbury with Ue = dt/2 [U; 0], Ve = [V_n, 0]:
        // x = x0 + Y (I - V_n Y_v)^-1 V_n x0_v,  K Y = Ue
        const int r = fb->r;
        for (int j = 0; j < r; ++j) {
            double *yj = t->fb_y.p + (size_t)j * h->ld;
            DNS_HIP(hipMemsetAsync(h->bdev.p, 0, h->ld * sizeof(double), s));
            hipLaunchKernelGGL(dns::k_axpby, dns::grid_for_elems(nv),
                               dns::kBlock, 0, s, (int64_t)nv, hdt,
                               t->fb_u.p + (size_t)j * nv, 0.0, h->bdev.p);
            DNS_HIP(hipMemsetAsync(yj, 0, h->ld * sizeof(double), s));
            dns_solve_stats sj;
            memset(&sj, 0, sizeof(sj));
            h->want_history = false;
            const int rj = h->gmres(h->bdev.p, yj, &o, &sj);
            h->want_history = true;
            if (rj != DNS_OK) return rj;
            if (h->dist()) {
                // (the small Woodbury system is formed redundantly by every
                // rank from whole vectors, like the assembly)
                DNS_TRY(h->comm->allgatherv(yj, h->st_v, s));
                if (np > 0) DNS_TRY(h->comm->allgatherv(yj + nv, h->st_p, s));
            }
            st->iters += sj.iters;
            if (sj.status != DNS_OK) st->status = sj.status;
        }
        std::vector<double> small((size_t)r * r), rhs((size_t)r);
        for (int i = 0; i < r; ++i) {
            DNS_TRY(h->dot_host(nv, t->fb_vn.p + (size_t)i * nv, x, &rhs[i]));
            for (int j = 0; j < r; ++j) {
                double d = 0.0;
                DNS_TRY(h->dot_host(nv, t->fb_vn.p + (size_t)i * nv,
                                    t->fb_y.p + (size_t)j * h->ld, &d));
                small[(size_t)i * r + j] = (i == j ? 1.0 : 0.0) - d;
            }
        }
        if (!small_solve(r, small, rhs))
            return dns::fail(DNS_BREAKDOWN,
                             "singular Sherman-Morrison-Woodbury system");
        for (int j = 0; j < r; ++j)
            hipLaunchKernelGGL(dns::k_axpby, dns::grid_for_elems(n),
                               dns::kBlock, 0, s, (int64_t)n, rhs[j],
                               t->fb_y.p + (size_t)j * h->ld, 1.0, x);
        DNS_HIP(hipGetLastError());
    }
    t->rotate();                       // the new solution is current
    t->last_dt = dt;
    t->cur_slot = lin_slot;
    // (N_c, f_c at the new velocity, snu:1529-1537: taken when the next step
    // forms its right-hand side -- k_conv_step_cells, TrapRhs)
    // dt ||v_n - v_lin||_M^2  (snu:1557-1560) and the new velocity into its
    // trajectory slot, in ONE walk over the rows of M
    double *slot_out = nullptr;
    if (out_slot >= 0) {
        DNS_TRY(t->export_fence(1 - lin_which));
        slot_out = t->traj[1 - lin_which].p + (size_t)out_slot * nv;
    }
    // (riding in the element launch: few enough workgroups to be resident
    // beside the element workgroups, which hold two or three waves per SIMD)
    const bool will_ride = async && !pon && t->env_upd_ride;
    const int gU = std::max(1, std::min(dns::grid_for_rows(
                                            std::max(1, rv1 - rv0), h->F.lpr),
                                        will_ride ? 256 : 1024));
    // pipelined sweep: this step's partials go to their place in the batch's
    // ring (times dt); one sum per poll instead of one launch per step
    if (async && t->upd_stride != gU) {
        DNS_TRY(t->flush_updnorm());
        DNS_TRY(t->upd_ring.alloc((size_t)dns_trap::kUpdSlots * gU));
        t->upd_stride = gU;
    }
    const bool ringed = async && t->upd_slot < dns_trap::kUpdSlots;
    double *upart = ringed ? t->upd_ring.p + (size_t)t->upd_slot * gU
                           : h->partC.p;
    if (ringed && will_ride) {
        // (launched by the element launch of the next step, or by whoever
        // asks for its results first)
        t->pend.on = true;
        t->pend.job = dns::UpdJob{h->F.rowptr.p, h->F.colidx.p, t->mvals.p,
                                  t->xs[t->cur].p, vlin, upart, slot_out,
                                  nv, gU, h->F.lpr, dt};
        t->pend.out_which = out_slot >= 0 ? 1 - lin_which : -1;
        t->upd_slot++;
        return DNS_OK;
    }
    DNS_LPR_SWITCH(h->F.lpr,
                   hipLaunchKernelGGL(dns::k_trap_updnorm<L>, gU, dns::kBlock,
                                      0, s, nv, h->F.rowptr.p, h->F.colidx.p,
                                      t->mvals.p, t->xs[t->cur].p, vlin,
                                      upart, slot_out, rv0, rv1,
                                      pon ? t->part.planX.ridx.p
                                          : (const int *)nullptr,
                                      pon ? t->part.nhalo : 0,
                                      ringed ? dt : 1.0));
    DNS_HIP(hipGetLastError());
    if (ringed) {
        t->upd_slot++;                 // (summed when the host polls)
    } else if (async) {
        hipLaunchKernelGGL(dns::k_trap_acc, 1, dns::kBlock, 0, s, h->partC.p,
                           gU, dt, t->updnorm_dev.p);
        DNS_HIP(hipGetLastError());
    } else {
        hipLaunchKernelGGL(dns::k_sum_partials, 1, dns::kBlock, 0, s,
                           h->partC.p, gU, h->scal.p);
        DNS_HIP(hipGetLastError());
        DNS_TRY(dns::d2h_pinned(h->scal_host.p, h->scal.p, 1, s));
        DNS_HIP(hipStreamSynchronize(s));
        t->updnorm += dt * h->scal_host.p[0];
    }
    if (async) return DNS_OK;            // (device time: see dns_trap_poll)
    DNS_HIP(hipEventRecord(h->ev1, s));
    DNS_HIP(hipEventSynchronize(h->ev1));
    float ms = 0.f;
    DNS_HIP(hipEventElapsedTime(&ms, h->ev0, h->ev1));
    st->device_seconds = 1e-3 * ms;
    return DNS_OK;
}

extern "C" {

int dns_trap_set_pipeline(dns_trap *t, int32_t cycle_len) try {
    if (!t || cycle_len < 0) return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    dns_saddle *h = t->sys;
    DNS_HIP(hipSetDevice(h->device));
    DNS_TRY(t->flush_pending_upd());
    t->pipeline_c = cycle_len;
    // batch accumulators of the control block start from zero; inside a
    // pipelined batch the solves may run their whole cycle (oversolve)
    return h->set_stop_frac(cycle_len > 0 ? t->over_frac : 0.0);
} DNS_CAPI_CATCH

// both polls: the batch accumulators of the control block (and, with `ext_i`,
// the extended ones), the update norm collected, the stop fraction re-armed
static int read_batch_accumulators(dns_trap *t, int32_t *solves,
                                   int32_t *fails, int32_t *iters,
                                   int32_t *maxit, int32_t *ext_i = nullptr,
                                   double *ext_d = nullptr) {
    if (!t) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = t->sys;
    DNS_HIP(hipSetDevice(h->device));
    DNS_TRY(h->read_header());                 // synchronises the stream
    const dns::CtlHeaderAcc *ha = h->hdr_host.p;
    if (solves) *solves = ha->acc_solves;
    if (fails) *fails = ha->acc_fail;
    if (iters) *iters = ha->acc_iters;
    if (maxit) *maxit = ha->acc_maxit;
    DNS_TRY(t->collect_updnorm());
    if (ext_i) {
        ext_i[0] = ha->acc_maxneed;
        ext_i[1] = ha->acc_sumneed;
        ext_d[0] = ha->acc_maxrel;
        ext_d[1] = ha->acc_maxprev;
    }
    DNS_TRY(h->set_stop_frac(t->pipeline_c > 0 ? t->over_frac : 0.0));
    DNS_HIP(hipStreamSynchronize(h->stream));
    return DNS_OK;
}

int dns_trap_poll(dns_trap *t, int32_t *solves, int32_t *fails, int32_t *iters,
                  int32_t *maxit) try {
    return read_batch_accumulators(t, solves, fails, iters, maxit);
} DNS_CAPI_CATCH

int dns_trap_poll_ext(dns_trap *t, int32_t *out6, double *out2) try {
    if (!out6 || !out2) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    return read_batch_accumulators(t, out6, out6 + 1, out6 + 2, out6 + 3,
                                   out6 + 4, out2);
} DNS_CAPI_CATCH

int dns_trap_set_oversolve(dns_trap *t, double stop_frac) try {
    if (!t || !(stop_frac >= 0.0) || stop_frac > 1.0)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    t->over_frac = stop_frac;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_trap_checkpoint(dns_trap *t) try {
    if (!t) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = t->sys;
    DNS_HIP(hipSetDevice(h->device));
    // (the work buffer is not part of it: restore clears pre_ok)
    t->ck.clear();
    for (int q : {t->cur, t->prev, t->pprev, t->p3, t->p4})
        DNS_TRY(t->ck.add(t->xs[q].p, h->ld));
    DNS_TRY(t->ck.save(h->stream));
    // (the part of the update norm still on the device belongs to the steps
    // before the checkpoint)
    DNS_TRY(t->collect_updnorm());
    t->ckh.valid = true;
    t->ckh.ring = *t;
    t->ckh.cur_slot = t->cur_slot;
    t->ckh.last_dt = t->last_dt;
    t->ckh.updnorm = t->updnorm;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_trap_restore(dns_trap *t, int32_t newton) try {
    if (!t) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    if (!t->ckh.valid)
        return dns::fail(DNS_ERR_NOT_READY, "no checkpoint to restore");
    dns_saddle *h = t->sys;
    DNS_HIP(hipSetDevice(h->device));
    DNS_HIP(hipStreamSynchronize(h->stream));
    // (the ring as it was: one of its six rotations, as a reset ring is)
    DNS_TRY(t->ck.restore(h->stream));
    static_cast<dns::Ring &>(*t) = t->ckh.ring;
    t->pre_ok = false;       // (the work buffer is not part of the checkpoint)
    t->cur_slot = t->ckh.cur_slot;
    t->last_dt = t->ckh.last_dt;
    t->updnorm = t->ckh.updnorm;
    t->pipeline_c = 0;
    DNS_TRY(t->updnorm_dev.zero(h->stream));
    t->upd_slot = 0;          // (partials of the steps behind the checkpoint)
    t->pend.on = false;
    DNS_TRY(h->set_stop_frac(0.0));      // (accumulators, oversolve off)
    t->conv->dbc_ctr = nullptr;
    t->conv->dbc_row = t->cur_slot;
    (void)newton;
    DNS_HIP(hipStreamSynchronize(h->stream));
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_trap_get_state(dns_trap *t, double *v, double *p) try {
    if (!t) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    dns_saddle *h = t->sys;
    DNS_HIP(hipSetDevice(h->device));
    if (h->dist() && t->part.on)
        DNS_TRY(h->comm->allgatherv(t->xs[t->cur].p, h->st_v, h->stream));
    if (v) DNS_TRY(t->xs[t->cur].download(v, (size_t)h->nv, h->stream));
    if (p) {
        DNS_TRY(dns::download_from(p, t->xs[t->cur].p + h->nv,
                                   (size_t)h->np, h->stream));
        const double sc = t->last_dt > 0.0 ? -1.0 / t->last_dt : 1.0;
        for (int i = 0; i < h->np; ++i) p[i] *= sc;          // snu:1542
    }
    DNS_HIP(hipStreamSynchronize(h->stream));
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_trap_update_norm(dns_trap *t, double *out) try {
    if (!t || !out) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    *out = t->updnorm;
    dns_saddle *h = t->sys;
    if (h->dist() && t->part.on) {
        // (partitioned assembly: every rank holds the share of its rows;
        // collective -- all ranks ask together)
        DNS_HIP(hipSetDevice(h->device));
        double v = t->updnorm;
        DNS_TRY(h->allreduce_host(&v, 1));
        *out = v;
    }
    return DNS_OK;
} DNS_CAPI_CATCH

// TEST ONLY: the front part of a step (dns_trap::enqueue_front, the member
// function step_impl calls) and a copy out of what it has left
int dns_trap_assembly_probe(dns_trap *t, double dt, int32_t lin_which,
                            int32_t lin_slot, int32_t newton,
                            const double *x0_in, dns_trap_probe *out) try {
    if (!t || !out || !(dt > 0.0) || lin_which < 0 || lin_which > 1 ||
        lin_slot < 0 || lin_slot >= t->nslots || out->parts_cap < 0)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    dns_saddle *h = t->sys;
    if (h->dist() || h->dist_sliced || h->rank_local)
        return dns::fail(DNS_ERR_BAD_ARGUMENT,
                         "the assembly probe takes an un-partitioned handle");
    if (t->pipeline_c > 0 || t->pend.on || t->upd_slot > 0)
        return dns::fail(DNS_ERR_NOT_READY,
                         "the assembly probe: a pipelined batch or an "
                         "update-norm job is pending");
    DNS_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t nv = (size_t)h->nv, n = (size_t)h->n, nnz = (size_t)h->F.nnz;
    dns_solve_opts o;
    dns_default_solve_opts(&o);
    if (x0_in) DNS_TRY(dns::upload_to(t->xs[t->work].p, x0_in, n, s));
    dns_trap::Front fr;
    DNS_TRY(t->enqueue_front(dt, lin_which, lin_slot, newton, 4, o, nullptr,
                             x0_in != nullptr, &fr));
    DNS_HIP(hipStreamSynchronize(s));
    out->fused = fr.fuse_r ? 1 : 0;
    out->nparts = fr.fuse_r ? fr.gb_rows : 0;
    if (out->nvals) DNS_TRY(t->nn_vals.download(out->nvals, nnz, s));
    if (out->fvals) DNS_TRY(dns::download_from(out->fvals, h->F.vals.p, nnz, s));
    if (out->kfvals) {
        if (!t->kpos.p)
            return dns::fail(DNS_ERR_NOT_READY, "no positions of F in K");
        std::vector<int> kp(nnz);
        std::vector<double> kv((size_t)h->K.nnz);
        DNS_TRY(t->kpos.download(kp.data(), nnz, s));
        DNS_TRY(dns::download_from(kv.data(), h->K.vals.p, kv.size(), s));
        DNS_HIP(hipStreamSynchronize(s));
        for (size_t z = 0; z < nnz; ++z) {
            if (kp[z] < 0 || (size_t)kp[z] >= kv.size())
                return dns::fail(DNS_ERR_HOST, "position %d outside K", kp[z]);
            out->kfvals[z] = kv[(size_t)kp[z]];
        }
    }
    if (out->rhsbc) DNS_TRY(t->rhsbc.download(out->rhsbc, nv, s));
    if (out->fvn) DNS_TRY(t->fvn_n.download(out->fvn, nv, s));
    if (out->b) DNS_TRY(t->b.download(out->b, n, s));
    if (out->x0) DNS_TRY(dns::download_from(out->x0, fr.x, n, s));
    if (fr.fuse_r) {
        if (fr.gb_rows > out->parts_cap && (out->partR || out->partB))
            return dns::fail(DNS_ERR_BAD_ARGUMENT,
                             "%d partials, room for %d", fr.gb_rows,
                             out->parts_cap);
        if (out->r) DNS_TRY(dns::download_from(out->r, h->r.p, n, s));
        if (out->partR)
            DNS_TRY(dns::download_from(out->partR, h->partR.p,
                                       (size_t)fr.gb_rows, s));
        if (out->partB)
            DNS_TRY(dns::download_from(out->partB, h->partB.p,
                                       (size_t)fr.gb_rows, s));
    }
    DNS_HIP(hipStreamSynchronize(s));
    return DNS_OK;
} DNS_CAPI_CATCH

}  // extern "C"
