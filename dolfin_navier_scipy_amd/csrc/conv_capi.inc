// extern "C" entry points of the device convection (included by dns_amd.hip)

namespace dns {

static int upload_conv_tables() {
    static bool done = false;
    if (done) return DNS_OK;
    ConvTables t;
    const double s15 = std::sqrt(15.0);
    const double t1 = (6.0 - s15) / 21.0, t2 = (6.0 + s15) / 21.0;
    const double w1 = (155.0 - s15) / 1200.0, w2 = (155.0 + s15) / 1200.0;
    const double qp[7][3] = {{1 / 3., 1 / 3., 1 / 3.},
                             {1 - 2 * t1, t1, t1}, {t1, 1 - 2 * t1, t1},
                             {t1, t1, 1 - 2 * t1}, {1 - 2 * t2, t2, t2},
                             {t2, 1 - 2 * t2, t2}, {t2, t2, 1 - 2 * t2}};
    const double qw[7] = {9 / 40., w1, w1, w1, w2, w2, w2};
    const int eo[3][2] = {{1, 2}, {0, 2}, {0, 1}};   // edge node k opposite vertex k
    for (int q = 0; q < 7; ++q) {
        t.qw[q] = qw[q];
        for (int a = 0; a < 6; ++a)
            for (int i = 0; i < 3; ++i) t.dphi[q][a][i] = 0.0;
        for (int k = 0; k < 3; ++k) {
            t.phi[q][k] = qp[q][k] * (2 * qp[q][k] - 1);
            t.dphi[q][k][k] = 4 * qp[q][k] - 1;
            const int i = eo[k][0], j = eo[k][1];
            t.phi[q][3 + k] = 4 * qp[q][i] * qp[q][j];
            t.dphi[q][3 + k][i] = 4 * qp[q][j];
            t.dphi[q][3 + k][j] = 4 * qp[q][i];
        }
    }
    void *dst = nullptr;
    DNS_HIP(hipGetSymbolAddress(&dst, HIP_SYMBOL(c_conv)));
    DNS_TRY(upload_to(static_cast<ConvTables *>(dst), &t, 1, nullptr));
    done = true;
    return DNS_OK;
}

}  // namespace dns

extern "C" {

int dns_conv_create_p2(int device, int32_t ncells, const int32_t *cell_vdofs,
                       const double *glam, const double *area, int32_t vdim,
                       int32_t nv_inner, const int32_t *invinds, int32_t ndbc,
                       const int32_t *dbcinds, const double *dbcvals,
                       dns_conv **out) try {
    if (!out || !cell_vdofs || !glam || !area || !invinds || ncells < 1 ||
        vdim < 1 || nv_inner < 0 || ndbc < 0 || (ndbc > 0 && (!dbcinds || !dbcvals)))
        return fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    *out = nullptr;
    // full dof -> inner index (>= 0) or -(k+1) for the k-th Dirichlet value
    std::vector<int> code((size_t)vdim, INT32_MIN);
    for (int k = 0; k < ndbc; ++k) {
        if (dbcinds[k] < 0 || dbcinds[k] >= vdim)
            return fail(DNS_ERR_BAD_ARGUMENT, "Dirichlet index out of range");
        code[dbcinds[k]] = -(k + 1);
    }
    for (int r = 0; r < nv_inner; ++r) {
        if (invinds[r] < 0 || invinds[r] >= vdim)
            return fail(DNS_ERR_BAD_ARGUMENT, "inner index out of range");
        code[invinds[r]] = r;
    }
    // INTERNAL cell order = cells sorted by their smallest inner dof (the dofs
    // are numbered along the mesh: neighbouring rows then gather their cell
    // contributions from neighbouring cells, and neighbouring cells gather
    // their twelve dof values from neighbouring lines).  A mesh refiner numbers
    // the children of a coarse cell consecutively, with no relation to the dof
    // numbering: at n = 2.8e6 the gather of the step's right-hand side read
    // ~8 x its algorithmic bytes.  Nothing per cell leaves the handle, so the
    // order is nobody's business but this file's.
    std::vector<int> order((size_t)ncells), key((size_t)ncells, INT32_MAX);
    for (int c = 0; c < ncells; ++c) {
        order[c] = c;
        for (int k = 0; k < 12; ++k) {
            const int d = cell_vdofs[(size_t)12 * c + k];
            if (d < 0 || d >= vdim || code[d] == INT32_MIN)
                return fail(DNS_ERR_BAD_ARGUMENT,
                            "cell %d: dof %d is neither inner nor Dirichlet", c,
                            d);
            if (code[d] >= 0) key[c] = std::min(key[c], code[d]);
        }
    }
    std::stable_sort(order.begin(), order.end(),
                     [&](int a, int b) { return key[a] < key[b]; });
    std::vector<int> cmap((size_t)12 * ncells), cnt((size_t)nv_inner + 1, 0);
    std::vector<double> gl((size_t)6 * ncells), ar((size_t)ncells);
    for (int c = 0; c < ncells; ++c) {
        const int src = order[c];
        for (int k = 0; k < 12; ++k) {
            const int d = cell_vdofs[(size_t)12 * src + k];
            cmap[(size_t)k * ncells + c] = code[d];
            if (code[d] >= 0) cnt[code[d] + 1]++;
        }
        for (int k = 0; k < 6; ++k)
            gl[(size_t)k * ncells + c] = glam[(size_t)6 * src + k];
        ar[c] = area[src];
    }
    for (int r = 0; r < nv_inner; ++r) cnt[r + 1] += cnt[r];
    std::vector<int> gidx((size_t)cnt[nv_inner]), pos(cnt.begin(), cnt.end() - 1);
    for (int k = 0; k < 12; ++k)          // fixed order -> reproducible sums
        for (int c = 0; c < ncells; ++c) {
            const int m = cmap[(size_t)k * ncells + c];
            if (m >= 0) gidx[pos[m]++] = k * ncells + c;
        }
    DNS_HIP(hipSetDevice(device));
    DNS_TRY(upload_conv_tables());
    auto cv = std::make_unique<dns_conv>();
    cv->device = device;
    if (const char *e = getenv("DNS_CONV_LANE_MIN")) cv->lane_min = atoi(e);
    cv->cmap_host = cmap;
    cv->cpos_host.resize((size_t)ncells);
    for (int c = 0; c < ncells; ++c) cv->cpos_host[order[c]] = c;
    cv->gptr_host = cnt;
    cv->gidx_host = gidx;
    cv->ncells = ncells;
    cv->nv_inner = nv_inner;
    cv->ndbc = ndbc;
    cv->dbc_host.assign(dbcvals, dbcvals + ndbc);
    DNS_TRY(cv->cellmap.alloc(cmap.size()));
    DNS_TRY(cv->gptr.alloc(cnt.size()));
    DNS_TRY(cv->gidx.alloc(gidx.size()));
    DNS_TRY(cv->glam.alloc(gl.size()));
    DNS_TRY(cv->area.alloc((size_t)ncells));
    DNS_TRY(cv->dbcvals.alloc((size_t)std::max(1, ndbc)));
    DNS_TRY(cv->cellvals.alloc((size_t)12 * ncells));
    DNS_TRY(cv->cellmap.upload(cmap.data(), cmap.size(), nullptr));
    DNS_TRY(cv->gptr.upload(cnt.data(), cnt.size(), nullptr));
    DNS_TRY(cv->gidx.upload(gidx.data(), gidx.size(), nullptr));
    DNS_TRY(cv->glam.upload(gl.data(), gl.size(), nullptr));
    DNS_TRY(cv->area.upload(ar.data(), (size_t)ncells, nullptr));
    if (ndbc > 0)
        DNS_TRY(cv->dbcvals.upload(dbcvals, (size_t)ndbc, nullptr));
    if (hipDeviceSynchronize() != hipSuccess)
        return fail(DNS_ERR_HIP, "device sync failed");
    *out = cv.release();
    return DNS_OK;
} DNS_CAPI_CATCH

void dns_conv_destroy(dns_conv *cv) {
    if (!cv) return;
    (void)hipSetDevice(cv->device);
    (void)hipDeviceSynchronize();
    delete cv;
}

int dns_conv_set_dbcvals(dns_conv *cv, const double *dbcvals) try {
    if (!cv || !dbcvals) return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    if (cv->lin_mode == dns::kConvAdjoint)
        DNS_TRY(dns::check_adjoint_dbc(dbcvals, cv->ndbc, 0));
    DNS_HIP(hipSetDevice(cv->device));
    if (cv->ndbc > 0)
        DNS_TRY(dns::upload_to(cv->dbcvals.p, dbcvals, (size_t)cv->ndbc,
                               nullptr));
    cv->dbc_host.assign(dbcvals, dbcvals + cv->ndbc);
    cv->dbc_rows = 0;                  // one constant value set from here on
    cv->dbc_gen++;
    cv->dbc_ctr = nullptr;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_conv_set_dbc_table(dns_conv *cv, int32_t nrows,
                           const double *vals) try {
    if (!cv || nrows < 1 || !vals)
        return fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    if (cv->lin_mode == dns::kConvAdjoint)
        DNS_TRY(dns::check_adjoint_dbc(nullptr, 0, nrows));
    DNS_HIP(hipSetDevice(cv->device));
    DNS_HIP(hipDeviceSynchronize());           // replays may still read it
    const size_t nd = (size_t)std::max(1, cv->ndbc);
    if (cv->dbc_tab.n < nd * nrows) DNS_TRY(cv->dbc_tab.alloc(nd * nrows));
    if (cv->ndbc > 0)
        DNS_TRY(dns::upload_to(cv->dbc_tab.p, vals,
                               (size_t)cv->ndbc * nrows, nullptr));
    cv->dbc_rows = nrows;
    cv->dbc_row = 0;
    cv->dbc_gen++;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_conv_set_dbc_row(dns_conv *cv, int32_t row) try {
    if (!cv || row < 0 || (cv->dbc_rows > 0 && row >= cv->dbc_rows))
        return fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    cv->dbc_row = row;
    cv->dbc_gen++;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_conv_set_base_flow(dns_conv *cv, const double *v_inner,
                           const double *dbcvals, int32_t adjoint) try {
    if (!cv) return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    if (adjoint)
        DNS_TRY(dns::check_adjoint_dbc(cv->dbc_host.data(), cv->ndbc,
                                       cv->dbc_rows));
    std::vector<double> vb;
    DNS_TRY(dns::expand_base_flow(cv->cmap_host.data(), cv->ncells,
                                  cv->nv_inner, cv->ndbc, v_inner, dbcvals,
                                  vb));
    DNS_HIP(hipSetDevice(cv->device));
    DNS_HIP(hipDeviceSynchronize());           // replays may still read it
    if (cv->vbase.n < vb.size()) DNS_TRY(cv->vbase.alloc(vb.size()));
    DNS_TRY(cv->vbase.upload(vb.data(), vb.size(), nullptr));
    DNS_HIP(hipDeviceSynchronize());
    cv->release_base_trajectory();             // a constant base from here on
    cv->lin_mode = adjoint ? dns::kConvAdjoint : dns::kConvForward;
    cv->dbc_gen++;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_conv_clear_base_flow(dns_conv *cv) try {
    if (!cv) return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_HIP(hipSetDevice(cv->device));
    DNS_HIP(hipDeviceSynchronize());           // replays may still read it
    cv->vbase.release();
    cv->release_base_trajectory();
    cv->lin_mode = dns::kConvNonlinear;
    cv->dbc_gen++;
    return DNS_OK;
} DNS_CAPI_CATCH

// A time-varying base flow: `nrows` rows of inner velocities (`ld_host` apart)
// and the base flow's Dirichlet values, one set or one per row.  One staged
// upload of the packed rows; row 0 and no index table until one is set.
int dns_conv_set_base_trajectory(dns_conv *cv, int32_t nrows,
                                 const double *v_rows, int32_t ld_host,
                                 int32_t dbc_nrows, const double *dbc_vals,
                                 int32_t adjoint) try {
    if (!cv) return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_TRY(dns::check_base_trajectory(nrows, cv->nv_inner, v_rows, ld_host,
                                       dbc_nrows, cv->ndbc, dbc_vals));
    if (adjoint)
        DNS_TRY(dns::check_adjoint_dbc(cv->dbc_host.data(), cv->ndbc,
                                       cv->dbc_rows));
    std::vector<double> rows;
    DNS_TRY(dns::pack_base_trajectory(nrows, cv->nv_inner, v_rows, ld_host,
                                      rows));
    DNS_HIP(hipSetDevice(cv->device));
    DNS_HIP(hipDeviceSynchronize());           // replays may still read it
    DevBuf<double> T;
    DNS_TRY(T.alloc(rows.size()));
    DNS_TRY(T.upload(rows.data(), rows.size(), nullptr));
    return cv->adopt_base_trajectory(T, nrows, dbc_nrows, dbc_vals,
                                     adjoint != 0, nullptr);
} DNS_CAPI_CATCH

// The per-step index table: step s of the chunk an attached stepper runs next
// (its counter) evaluates about row rows[min(s, n - 1)] -- with `weights`,
// between that row and the next.  The caller has checked the table.
static int set_base_table(dns_conv *cv, int32_t n, const int32_t *rows,
                          const double *weights) {
    DNS_HIP(hipSetDevice(cv->device));
    DNS_HIP(hipDeviceSynchronize());           // replays may still read it
    // (whatever can run out of memory comes before the first change)
    DevBuf<int> tab;
    DevBuf<double> wtab;
    if (cv->brow.n < (size_t)n) DNS_TRY(tab.alloc((size_t)n));
    if (weights && cv->bwgt.n < (size_t)n) DNS_TRY(wtab.alloc((size_t)n));
    if (tab.p) {
        std::swap(cv->brow.p, tab.p);
        std::swap(cv->brow.n, tab.n);
    }
    if (wtab.p) {
        std::swap(cv->bwgt.p, wtab.p);
        std::swap(cv->bwgt.n, wtab.n);
    }
    cv->nbrow = 0;                             // (until the table is there)
    cv->bt_ctr = nullptr;
    cv->bt_lerp = false;
    cv->bt_weight = 0.0;
    cv->dbc_gen++;
    DNS_TRY(cv->brow.upload(rows, (size_t)n, nullptr));
    if (weights) DNS_TRY(cv->bwgt.upload(weights, (size_t)n, nullptr));
    cv->nbrow = n;
    cv->bt_row = rows[0];
    if (weights) {
        cv->bt_lerp = true;
        cv->bt_weight = weights[0];
    }
    cv->brow_gen++;
    return DNS_OK;
}

int dns_conv_set_base_rows(dns_conv *cv, int32_t n, const int32_t *rows) try {
    if (!cv) return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_TRY(dns::check_base_rows(n, rows, cv->bt_rows));
    return set_base_table(cv, n, rows, nullptr);
} DNS_CAPI_CATCH

int dns_conv_set_base_rows_lerp(dns_conv *cv, int32_t n, const int32_t *rows,
                                const double *weights) try {
    if (!cv) return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_TRY(dns::check_base_rows_lerp(n, rows, weights, cv->bt_rows));
    return set_base_table(cv, n, rows, weights);
} DNS_CAPI_CATCH

// The row for dns_conv_apply and the probes outside a stepper -- and, since it
// takes the index table off, for the steps of an attached one
int dns_conv_set_base_row(dns_conv *cv, int32_t row) try {
    if (!cv) return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_TRY(dns::check_base_row(row, cv->bt_rows));
    cv->bt_row = row;
    cv->nbrow = 0;
    cv->bt_ctr = nullptr;
    cv->bt_lerp = false;
    cv->bt_weight = 0.0;
    cv->dbc_gen++;
    return DNS_OK;
} DNS_CAPI_CATCH

// ... between that row and the next: V_row + weight (V_{row+1} - V_row)
int dns_conv_set_base_row_lerp(dns_conv *cv, int32_t row, double weight) try {
    if (!cv) return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_TRY(dns::check_base_row_lerp(row, weight, cv->bt_rows));
    cv->bt_row = row;
    cv->nbrow = 0;
    cv->bt_ctr = nullptr;
    cv->bt_lerp = true;
    cv->bt_weight = weight;
    cv->dbc_gen++;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_conv_get_base_lerp(const dns_conv *cv, int32_t *lerp) try {
    if (!cv || !lerp) return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    *lerp = cv->bt_lerp ? 1 : 0;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_conv_get_base_info(const dns_conv *cv, int32_t *nrows,
                           int32_t *nbrow) try {
    if (!cv) return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    if (nrows) *nrows = cv->bt_rows;
    if (nbrow) *nbrow = cv->nbrow;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_conv_get_mode(const dns_conv *cv, int32_t *mode) try {
    if (!cv || !mode) return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    *mode = cv->lin_mode;
    return DNS_OK;
} DNS_CAPI_CATCH

// TEST ONLY: the cell values [12][ncells] (internal cell order) the element
// launch leaves for `v_inner`, all cells or -- nsel >= 0 -- the cells sel[0 ..
// nsel) of the internal order over a background of `fill`; with `cell_pos` the
// caller's cell -> internal cell
int dns_conv_cells_probe(dns_conv *cv, const double *v_inner,
                         const int32_t *sel, int32_t nsel, double fill,
                         double *cells_out, int32_t *cell_pos) try {
    if (!cv || !v_inner || !cells_out || (nsel > 0 && !sel))
        return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    for (int k = 0; k < nsel; ++k)
        if (sel[k] < 0 || sel[k] >= cv->ncells)
            return fail(DNS_ERR_BAD_ARGUMENT, "cell %d outside 0..%d", sel[k],
                        cv->ncells - 1);
    DNS_HIP(hipSetDevice(cv->device));
    const size_t nc12 = (size_t)12 * cv->ncells;
    DevBuf<double> dv;
    DevBuf<int> dsel;
    DNS_TRY(dv.alloc((size_t)std::max(1, cv->nv_inner)));
    DNS_TRY(dv.upload(v_inner, (size_t)cv->nv_inner, nullptr));
    std::vector<double> bg(nc12, fill);
    DNS_TRY(cv->cellvals.upload(bg.data(), nc12, nullptr));
    if (nsel >= 0) {
        DNS_TRY(dsel.alloc((size_t)std::max(1, nsel)));
        if (nsel > 0) DNS_TRY(dsel.upload(sel, (size_t)nsel, nullptr));
    }
    cv->bt_ctr = nullptr;      // (outside a stepper: the row the host names)
    DNS_TRY(cv->enqueue_cells(dv.p, nullptr, nsel >= 0 ? dsel.p : nullptr,
                              std::max(0, nsel)));
    DNS_TRY(cv->cellvals.download(cells_out, nc12, nullptr));
    DNS_HIP(hipDeviceSynchronize());
    if (cell_pos)
        for (int c = 0; c < cv->ncells; ++c) cell_pos[c] = cv->cpos_host[c];
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_conv_apply(dns_conv *cv, const double *v_inner, double scale,
                   double *outv) try {
    if (!cv || !v_inner || !outv)
        return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_HIP(hipSetDevice(cv->device));
    DevBuf<double> dv, dout;
    DNS_TRY(dv.alloc((size_t)cv->nv_inner));
    DNS_TRY(dout.alloc((size_t)cv->nv_inner));
    DNS_TRY(dv.upload(v_inner, (size_t)cv->nv_inner, nullptr));
    cv->bt_ctr = nullptr;      // (outside a stepper: the row the host names)
    DNS_TRY(cv->enqueue(dv.p, scale, dout.p, nullptr));
    DNS_TRY(dout.download(outv, (size_t)cv->nv_inner, nullptr));
    DNS_HIP(hipDeviceSynchronize());
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_conv_project_tensor(dns_conv *cv, int32_t nb, int32_t nt, int32_t ld,
                            const double *basis, const double *dbc_rows,
                            double *out) try {
    if (!cv || !basis || !out)
        return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_TRY(cv->refuse_linearised("dns_conv_project_tensor"));
    const int nlive = dns::rom_live_cells(cv->cmap_host.data(), cv->ncells);
    DNS_TRY(dns::check_rom_shape(nb, nt, cv->nv_inner, ld, nlive));
    DNS_HIP(hipSetDevice(cv->device));
    const bool with_d = dbc_rows && cv->ndbc > 0;
    DevBuf<double> B, D, part, T;
    DNS_TRY(B.alloc((size_t)nb * ld));
    DNS_TRY(T.alloc((size_t)nt * nb * nb));
    DNS_TRY(B.upload(basis, (size_t)nb * ld, nullptr));
    if (with_d) {
        DNS_TRY(D.alloc((size_t)nb * cv->ndbc));
        DNS_TRY(D.upload(dbc_rows, (size_t)nb * cv->ndbc, nullptr));
    }
    DNS_TRY(dns::launch_rom_tensor(*cv, nlive, B.p, (size_t)ld,
                                   with_d ? D.p : nullptr, nb, nt, part, T.p,
                                   nullptr));
    DNS_TRY(T.download(out, (size_t)nt * nb * nb, nullptr));
    DNS_HIP(hipDeviceSynchronize());
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_conv_bind_pattern(dns_conv *cv, const dns_csr *pat) try {
    if (!cv || !pat || !pat->rowptr || !pat->colidx)
        return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    if (pat->nrows != cv->nv_inner || pat->ncols != cv->nv_inner)
        return fail(DNS_ERR_BAD_ARGUMENT, "pattern must be NV x NV");
    DNS_HIP(hipSetDevice(cv->device));
    const int nc = cv->ncells, nv = cv->nv_inner;
    const int64_t nnz = pat->rowptr[nv];
    const std::vector<int> &cm = cv->cmap_host;
    // position of (row, col) in the pattern; columns of a row need not be sorted
    auto find = [&](int r, int c) -> int64_t {
        for (int64_t k = pat->rowptr[r]; k < pat->rowptr[r + 1]; ++k)
            if (pat->colidx[k] == c) return k;
        return -1;
    };
    // pass 1: count, pass 2: fill -- contributions in (slot, cell) order
    std::vector<int> mcnt((size_t)nnz + 1, 0), bcnt((size_t)nv + 1, 0);
    std::vector<int64_t> where((size_t)144 * nc, -2);   // >= 0 nnz, -1 bc, -2 none
    for (int rs = 0; rs < 12; ++rs)
        for (int cs = 0; cs < 12; ++cs)
            for (int c = 0; c < nc; ++c) {
                const int mr = cm[(size_t)rs * nc + c];
                const int mc = cm[(size_t)cs * nc + c];
                if (mr < 0) continue;               // Dirichlet row: dropped
                const size_t e = ((size_t)rs * 12 + cs) * nc + c;
                if (mc >= 0) {
                    const int64_t z = find(mr, mc);
                    if (z < 0)
                        return fail(DNS_ERR_BAD_ARGUMENT,
                                    "pattern lacks entry (%d, %d) of the "
                                    "convection matrix", mr, mc);
                    where[e] = z;
                    mcnt[z + 1]++;
                } else {
                    where[e] = -1;
                    bcnt[mr + 1]++;
                }
            }
    for (int64_t z = 0; z < nnz; ++z) mcnt[z + 1] += mcnt[z];
    for (int r = 0; r < nv; ++r) bcnt[r + 1] += bcnt[r];
    std::vector<int> midx((size_t)mcnt[nnz]), bidx((size_t)bcnt[nv]),
        bbc((size_t)bcnt[nv]);
    std::vector<int> mpos(mcnt.begin(), mcnt.end() - 1),
        bpos(bcnt.begin(), bcnt.end() - 1);
    for (int rs = 0; rs < 12; ++rs)
        for (int cs = 0; cs < 12; ++cs)
            for (int c = 0; c < nc; ++c) {
                const size_t e = ((size_t)rs * 12 + cs) * nc + c;
                // (device layout of the local matrices: cell-major, a cell's
                // 144 entries side by side -- the gathers of neighbouring
                // non-zeros of a row share cache lines)
                const int edev = c * 144 + rs * 12 + cs;
                if (where[e] >= 0) {
                    midx[mpos[where[e]]++] = edev;
                } else if (where[e] == -1) {
                    const int mr = cm[(size_t)rs * nc + c];
                    const int mc = cm[(size_t)cs * nc + c];
                    bidx[bpos[mr]] = edev;
                    bbc[bpos[mr]++] = -mc - 1;
                }
            }
    auto m = std::make_unique<dns_conv_mat>();
    m->nnz = (int)nnz;
    DNS_TRY(m->mptr.alloc(mcnt.size()));
    DNS_TRY(m->midx.alloc(std::max<size_t>(1, midx.size())));
    DNS_TRY(m->bptr.alloc(bcnt.size()));
    DNS_TRY(m->bidx.alloc(std::max<size_t>(1, bidx.size())));
    DNS_TRY(m->bbc.alloc(std::max<size_t>(1, bbc.size())));
    DNS_TRY(m->L.alloc((size_t)144 * nc));
    DNS_TRY(m->mptr.upload(mcnt.data(), mcnt.size(), nullptr));
    DNS_TRY(m->midx.upload(midx.data(), midx.size(), nullptr));
    DNS_TRY(m->bptr.upload(bcnt.data(), bcnt.size(), nullptr));
    DNS_TRY(m->bidx.upload(bidx.data(), bidx.size(), nullptr));
    DNS_TRY(m->bbc.upload(bbc.data(), bbc.size(), nullptr));
    if (hipDeviceSynchronize() != hipSuccess)
        return fail(DNS_ERR_HIP, "device sync failed");
    delete cv->mat;
    cv->mat = m.release();
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_conv_assemble(dns_conv *cv, const double *u_inner, int32_t newton,
                      double *nvals, double *rhsbc, double *rhscon) try {
    if (!cv || !u_inner || !nvals)
        return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_TRY(cv->refuse_linearised("dns_conv_assemble"));
    if (!cv->mat) return fail(DNS_ERR_NOT_READY, "no pattern bound");
    DNS_HIP(hipSetDevice(cv->device));
    const size_t nv = (size_t)cv->nv_inner;
    DevBuf<double> dv, dn, db, dc;
    DNS_TRY(dv.alloc(nv));
    DNS_TRY(dn.alloc((size_t)cv->mat->nnz));
    DNS_TRY(db.alloc(nv));
    DNS_TRY(dc.alloc(nv));
    DNS_TRY(dv.upload(u_inner, nv, nullptr));
    DNS_TRY(cv->enqueue_mat_cells(dv.p, newton ? 1 : 0, nullptr));
    DNS_TRY(cv->enqueue_mat_gather(dn.p, nullptr, nullptr, 0.0, nullptr,
                                   nullptr));
    DNS_TRY(dn.download(nvals, (size_t)cv->mat->nnz, nullptr));
    if (rhsbc) {
        DNS_TRY(cv->enqueue_bc_gather(db.p, nullptr));
        DNS_TRY(db.download(rhsbc, nv, nullptr));
    }
    if (rhscon) {
        DNS_TRY(cv->enqueue(dv.p, 1.0, dc.p, nullptr));
        DNS_TRY(dc.download(rhscon, nv, nullptr));
    }
    DNS_HIP(hipDeviceSynchronize());
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_conv_assemble2(dns_conv *cv, const double *u_inner,
                       const double *dbcvals_lin, const double *dbcvals_rhs,
                       int32_t newton, double *nvals, double *rhsbc,
                       double *rhscon) try {
    if (!cv || !u_inner || !nvals || !dbcvals_lin)
        return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_TRY(cv->refuse_linearised("dns_conv_assemble2"));
    if (!cv->mat) return fail(DNS_ERR_NOT_READY, "no pattern bound");
    DNS_HIP(hipSetDevice(cv->device));
    const size_t nv = (size_t)cv->nv_inner;
    const size_t nd = (size_t)std::max(1, cv->ndbc);
    // the two value sets: the linearisation field's own boundary values and
    // the ones that go to the right-hand side (snu:446-455: "use the old v-bcs
    // to compute the convection, apply the new v-bcs")
    DevBuf<double> dv, dn, db, dc, dlin, drhs;
    DNS_TRY(dv.alloc(nv));
    DNS_TRY(dn.alloc((size_t)cv->mat->nnz));
    DNS_TRY(db.alloc(nv));
    DNS_TRY(dc.alloc(nv));
    DNS_TRY(dlin.alloc(nd));
    DNS_TRY(drhs.alloc(nd));
    DNS_TRY(dv.upload(u_inner, nv, nullptr));
    if (cv->ndbc > 0) {
        DNS_TRY(dlin.upload(dbcvals_lin, (size_t)cv->ndbc, nullptr));
        DNS_TRY(drhs.upload(dbcvals_rhs ? dbcvals_rhs : dbcvals_lin,
                            (size_t)cv->ndbc, nullptr));
    }
    const int g8 = (8 * cv->ncells + kBlock - 1) / kBlock;
    const TabRef lin = {dlin.p, nullptr, 0, 1}, rhs = {drhs.p, nullptr, 0, 1};
    hipLaunchKernelGGL(k_conv_mat_cells, g8, kBlock, 0, nullptr, cv->ncells,
                       cv->cellmap.p, cv->glam.p, cv->area.p, dv.p, lin,
                       newton ? 1 : 0, cv->mat->L.p);
    DNS_TRY(cv->enqueue_mat_gather(dn.p, nullptr, nullptr, 0.0, nullptr,
                                   nullptr));
    DNS_TRY(dn.download(nvals, (size_t)cv->mat->nnz, nullptr));
    if (rhsbc) {
        const int gr = std::max(1, std::min((cv->nv_inner + kBlock - 1) /
                                                kBlock, 2048));
        hipLaunchKernelGGL(k_conv_bc_gather, gr, kBlock, 0, nullptr,
                           cv->nv_inner, cv->mat->bptr.p, cv->mat->bidx.p,
                           cv->mat->bbc.p, cv->mat->L.p, rhs, db.p);
        DNS_TRY(db.download(rhsbc, nv, nullptr));
    }
    if (rhscon) {
        hipLaunchKernelGGL(k_conv_cells, g8, kBlock, 0, nullptr, cv->ncells,
                           cv->cellmap.p, cv->glam.p, cv->area.p, dv.p, lin,
                           cv->cellvals.p, (const int *)nullptr, 0);
        const int g2 = std::max(1, std::min((cv->nv_inner + kBlock - 1) /
                                                kBlock, 2048));
        hipLaunchKernelGGL(k_conv_gather, g2, kBlock, 0, nullptr, 0,
                           cv->nv_inner, cv->gptr.p, cv->gidx.p,
                           cv->cellvals.p, 1.0, dc.p);
        DNS_TRY(dc.download(rhscon, nv, nullptr));
    }
    DNS_HIP(hipGetLastError());
    DNS_HIP(hipDeviceSynchronize());
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_imex_set_convection(dns_imex *st, dns_conv *cv, double scale) try {
    if (!st) return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    if (cv && cv->nv_inner != st->sys->nv)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "convection operator has %d inner dofs, system has %d",
                    cv->nv_inner, st->sys->nv);
    if (cv && cv->linearised())
        DNS_TRY(st->refuse_partitioned(
            "linearised convection operator", kLinPartitioned));
    st->sys->drop_graphs();
    st->conv = cv;
    st->conv_scale = scale;
    st->six_ok = false;        // (cell values of another operator / none)
    st->dcells_ok = false;
    return DNS_OK;
} DNS_CAPI_CATCH

}  // extern "C"
