// Rank-local construction of a row-partitioned handle (dns_saddle_create_rows):
// a rank hands over ITS rows of K = [[F, JT], [J, 0]] only -- rows [v0, v1) of
// F and of J^T, rows [p0, p1) of J, global column indices -- and never holds a
// whole matrix, neither on the host nor in HBM.
//
//  * host copies keep the global shape with the own rows populated
//    (hostcsr.hpp, host_embed_rows): the row-wise set-up algebra of the
//    partitioned set-up (dist_solve.inc, build_explicit_part) runs on them
//    unchanged;
//  * the rows of the polynomial G = p(D^-1 F) D^-1 a rank forms reach
//    `degree - 1` rings of the pattern of F beyond the rows themselves: the
//    rows of F (and of J^T, for G JT) on those rings are FETCHED from their
//    owners ring by ring (fetch_rows: the requests through two all-gathers, the
//    rows through two grouped send/receive exchanges) and dropped after the
//    set-up;
//  * the spectral bounds of D^-1 F come from the power iterations of
//    estimate_bounds with the product formed by rows: every rank multiplies its
//    rows (lanes per row of the WHOLE matrix: the same sums in the same order),
//    the iterate is all-gathered, its norms are taken on the whole vector by
//    the kernels the one-GPU set-up uses -- bounds equal bit for bit, hence the
//    preconditioner is the one a handle created from whole matrices builds;
//  * halo index lists come from the rank's own patterns and are exchanged
//    (gather_need_lists), as the partitioned set-up already does for Gc.
// Not rank-local: the Schur complement's multigrid hierarchy (the rows of S are
// all-gathered, the Galerkin products run on the whole, every rank keeps its
// row blocks of the levels: setup_dist_mg) and the dense Schur inverse.

// one double per rank -> the largest
int dns_saddle::all_ranks_max(double mine, double *out) {
    using namespace dns;
    const int P = comm->nranks, me = comm->rank;
    std::vector<double> v((size_t)P, 0.0);
    v[me] = mine;
    DevBuf<double> buf;
    DNS_TRY(buf.alloc((size_t)P));
    DNS_TRY(buf.upload(v.data(), v.size(), stream));
    std::vector<int> st((size_t)P + 1);
    for (int r = 0; r <= P; ++r) st[r] = r;
    DNS_TRY(comm->allgatherv(buf.p, st, stream));
    DNS_TRY(buf.download(v.data(), v.size(), stream));
    *out = *std::max_element(v.begin(), v.end());
    return DNS_OK;
}

// Rows of a row-partitioned matrix from their owners.  `A`: global shape, this
// rank's rows [starts[me], starts[me + 1]) populated; `want`: sorted global
// indices of rows of OTHER ranks; `out`: global shape, exactly the wanted rows
// populated.  A collective: every rank calls it (an empty list is fine).
int dns_saddle::fetch_rows(const dns::HostCsr &A, const std::vector<int> &starts,
                           const std::vector<int> &want, dns::HostCsr &out) {
    using namespace dns;
    const int P = comm->nranks, me = comm->rank;
    std::vector<std::vector<int>> mine((size_t)P);
    // (local verdicts are agreed on before anybody leaves: the exchanges
    // below are entered by all ranks or by none)
    int bad = DNS_OK;
    {
        int q = 0, last = -1;
        for (int r : want) {
            if (r <= last || r < 0 || r >= starts[P]) {
                bad = fail(DNS_ERR_BAD_ARGUMENT,
                           "fetch_rows: list not sorted or out of range");
                break;
            }
            last = r;
            while (q + 1 < P && r >= starts[q + 1]) ++q;
            if (q == me) {
                bad = fail(DNS_ERR_BAD_ARGUMENT, "fetch_rows: own row %d", r);
                break;
            }
            mine[q].push_back(r);
        }
    }
    DNS_TRY(agree(bad, "fetch_rows (request lists)"));
    // all[r][q] = the rows rank r wants from rank q
    std::vector<std::vector<std::vector<int>>> all;
    DNS_TRY(gather_need_lists(mine, all));
    std::vector<int> sc((size_t)P, 0), sd((size_t)P, 0), rc((size_t)P, 0),
        rd((size_t)P, 0);
    size_t ns = 0, nr = 0;
    for (int q = 0; q < P && bad == DNS_OK; ++q)
        for (int i : all[q][me])
            if (i < starts[me] || i >= starts[me + 1]) {
                bad = fail(DNS_ERR_COMM,
                           "fetch_rows: rank %d asks rank %d for row %d", q,
                           me, i);
                break;
            }
    DNS_TRY(agree(bad, "fetch_rows (served rows)"));
    for (int q = 0; q < P; ++q) {
        const std::vector<int> &serve = all[q][me];
        sc[q] = (int)serve.size();
        sd[q] = (int)ns;
        ns += serve.size();
        rc[q] = (int)mine[q].size();
        rd[q] = (int)nr;
        nr += mine[q].size();
    }
    // 1. the lengths of the rows
    std::vector<double> sb(std::max<size_t>(1, ns), 0.0),
        rb(std::max<size_t>(1, nr), 0.0);
    {
        size_t k = 0;
        for (int q = 0; q < P; ++q)
            for (int i : all[q][me])
                sb[k++] = (double)(A.rowptr[i + 1] - A.rowptr[i]);
    }
    DevBuf<double> ds, dr;
    DNS_TRY(ds.alloc(sb.size()));
    DNS_TRY(dr.alloc(rb.size()));
    DNS_TRY(ds.upload(sb.data(), sb.size(), stream));
    DNS_TRY(comm->alltoallv(ds.p, sc, sd, dr.p, rc, rd, stream));
    DNS_TRY(dr.download(rb.data(), rb.size(), stream));
    DNS_HIP(hipStreamSynchronize(stream));
    // 2. their entries as (column, value) pairs
    std::vector<int> sc2((size_t)P, 0), sd2((size_t)P, 0), rc2((size_t)P, 0),
        rd2((size_t)P, 0);
    int64_t ns2 = 0, nr2 = 0;
    for (int q = 0; q < P; ++q) {
        int64_t a = 0, b = 0;
        for (int i : all[q][me]) a += A.rowptr[i + 1] - A.rowptr[i];
        for (int k = 0; k < rc[q]; ++k) b += (int64_t)rb[(size_t)rd[q] + k];
        if (2 * (ns2 + a) > (int64_t)INT32_MAX ||
            2 * (nr2 + b) > (int64_t)INT32_MAX)
            return fail(DNS_ERR_BAD_ARGUMENT, "fetch_rows: too many entries");
        sc2[q] = (int)(2 * a);
        sd2[q] = (int)(2 * ns2);
        rc2[q] = (int)(2 * b);
        rd2[q] = (int)(2 * nr2);
        ns2 += a;
        nr2 += b;
    }
    std::vector<double> sb2((size_t)std::max<int64_t>(1, 2 * ns2), 0.0),
        rb2((size_t)std::max<int64_t>(1, 2 * nr2), 0.0);
    {
        size_t k = 0;
        for (int q = 0; q < P; ++q)
            for (int i : all[q][me])
                for (int e = A.rowptr[i]; e < A.rowptr[i + 1]; ++e) {
                    sb2[k++] = (double)A.colidx[e];
                    sb2[k++] = A.vals[e];
                }
    }
    DNS_TRY(ds.alloc(sb2.size()));
    DNS_TRY(dr.alloc(rb2.size()));
    DNS_TRY(ds.upload(sb2.data(), sb2.size(), stream));
    DNS_TRY(comm->alltoallv(ds.p, sc2, sd2, dr.p, rc2, rd2, stream));
    DNS_TRY(dr.download(rb2.data(), rb2.size(), stream));
    DNS_HIP(hipStreamSynchronize(stream));
    // 3. the wanted rows in global numbering (owners are consecutive blocks of
    // rows: the received order IS the order of `want`)
    out = HostCsr();
    out.nrows = A.nrows;
    out.ncols = A.ncols;
    out.rowptr.assign((size_t)A.nrows + 1, 0);
    for (size_t k = 0; k < want.size(); ++k)
        out.rowptr[(size_t)want[k] + 1] = (int)rb[k];
    for (int i = 0; i < A.nrows; ++i) out.rowptr[(size_t)i + 1] += out.rowptr[i];
    out.colidx.resize((size_t)nr2);
    out.vals.resize((size_t)nr2);
    for (int64_t k = 0; k < nr2; ++k) {
        const double c = rb2[(size_t)(2 * k)];
        if (!(c >= 0.0) || c >= (double)A.ncols)
            return fail(DNS_ERR_COMM, "fetch_rows: column index out of range");
        out.colidx[(size_t)k] = (int)c;
        out.vals[(size_t)k] = rb2[(size_t)(2 * k + 1)];
    }
    return DNS_OK;
}

int dns_saddle::init_rows(int dev, dns_comm *c, int nv_all, int np_all,
                          const dns_csr *f, const dns_csr *jt,
                          const dns_csr *j) {
    using namespace dns;
    if (!c) return fail(DNS_ERR_BAD_ARGUMENT, "null communicator");
    if (nv_all < 1 || np_all < 0)
        return fail(DNS_ERR_BAD_ARGUMENT, "bad sizes");
    st_v = partition_starts(nv_all, c->nranks);
    st_p = partition_starts(np_all, c->nranks);
    const int v0 = st_v[c->rank], v1 = st_v[c->rank + 1];
    const int p0 = st_p[c->rank], p1 = st_p[c->rank + 1];
    // what this rank was handed is judged by ALL ranks together (the creation
    // is collective: a rank that left on its own would leave the others waiting
    // in the first exchange)
    int bad = DNS_OK;
    if (check_csr(f, "F rows") != DNS_OK || check_csr(jt, "JT rows") != DNS_OK ||
        check_csr(j, "J rows") != DNS_OK)
        bad = DNS_ERR_BAD_ARGUMENT;
    else if (f->nrows != v1 - v0 || f->ncols != nv_all ||
             jt->nrows != v1 - v0 || jt->ncols != np_all ||
             j->nrows != p1 - p0 || j->ncols != nv_all)
        bad = fail(DNS_ERR_BAD_ARGUMENT,
                   "rank %d of %d holds rows [%d, %d) of F (%d columns) and "
                   "of JT (%d columns), rows [%d, %d) of J (dns_partition_"
                   "range): got %d x %d, %d x %d, %d x %d",
                   c->rank, c->nranks, v0, v1, nv_all, np_all, p0, p1,
                   f->nrows, f->ncols, jt->nrows, jt->ncols, j->nrows,
                   j->ncols);
    nv = nv_all;
    np = np_all;
    DNS_TRY(init_device(dev));
    comm = c;
    rank_local = true;
    dist_active = false;
    // sizes of the whole matrices (launch shapes follow the whole K and F, as
    // on a handle created from them)
    {
        double cnt[4] = {0.0, 0.0, 0.0, bad != DNS_OK ? 1.0 : 0.0};
        if (bad == DNS_OK) {
            cnt[0] = (double)f->nnz;
            cnt[1] = (double)jt->nnz;
            cnt[2] = (double)j->nnz;
        }
        DNS_TRY(allreduce_host(cnt, 4));
        if (bad != DNS_OK) return bad;
        if (cnt[3] > 0.0)
            return fail(DNS_ERR_BAD_ARGUMENT,
                        "another rank was handed rows that do not fit the "
                        "partition");
        if (cnt[1] != cnt[2])
            return fail(DNS_ERR_BAD_ARGUMENT,
                        "the rows of JT hold %.0f entries over all ranks, the "
                        "rows of J %.0f", cnt[1], cnt[2]);
        nnz_f_all = (int64_t)cnt[0];
        nnz_j_all = (int64_t)cnt[2];
        if (nnz_f_all + 2 * nnz_j_all > 0x7fffffffLL)
            return fail(DNS_ERR_BAD_ARGUMENT, "K exceeds int32 indexing");
    }
    Fh = host_embed_rows(f, v0, nv);
    JTh = host_embed_rows(jt, v0, nv);
    Jh = host_embed_rows(j, p0, np);
    K.lpr = pick_lpr((double)(nnz_f_all + 2 * nnz_j_all) / std::max(1, n));
    // 1 / diag(F) on the own rows (what the power iterations read)
    {
        std::vector<double> dv((size_t)nv, 1.0);
        for (int i = v0; i < v1; ++i) {
            double d = 0.0;
            for (int k = Fh.rowptr[i]; k < Fh.rowptr[i + 1]; ++k)
                if (Fh.colidx[k] == i) d += Fh.vals[k];
            dv[i] = (d != 0.0) ? 1.0 / d : 1.0;
        }
        DNS_TRY(dinv.alloc((size_t)nv));
        DNS_TRY(dinv.upload(dv.data(), dv.size(), stream));
    }
    return init_workspace();
}

// estimate_bounds with the product formed by rows (see the head of this file)
int dns_saddle::estimate_bounds_rows() {
    using namespace dns;
    const int v0 = st_v[comm->rank], v1 = st_v[comm->rank + 1];
    CsrDev Fl;
    {
        const HostCsr fl = host_row_slice(Fh, v0, v1);
        const dns_csr v = fl.view();
        DNS_TRY(Fl.upload(&v, stream));
    }
    Fl.lpr = pick_lpr((double)nnz_f_all / std::max(1, nv));
    // (dinv may be stale on the other ranks' rows: only the own rows are read)
    {
        std::vector<double> dv((size_t)std::max(1, v1 - v0), 1.0);
        for (int i = v0; i < v1; ++i) {
            double d = 0.0;
            for (int k = Fh.rowptr[i]; k < Fh.rowptr[i + 1]; ++k)
                if (Fh.colidx[k] == i) d += Fh.vals[k];
            dv[(size_t)(i - v0)] = (d != 0.0) ? 1.0 / d : 1.0;
        }
        if (v1 > v0) DNS_TRY(upload_to(dinv.p + v0, dv.data(), (size_t)(v1 - v0), stream));
    }
    double *x = cheb_d0.p, *y = cheb_d1.p;
    const int g = grid_for_elems(nv);
    const int gl = grid_for_elems(std::max(1, v1 - v0));
    auto product = [&]() -> int {
        // y = D^-1 F x: own rows, then every rank's rows everywhere
        if (v1 > v0) {
            DNS_TRY(launch_spmv(Fl, x, y + v0, 1.0, 0.0, nullptr,
                                DNS_SPMV_VECTOR, stream));
            hipLaunchKernelGGL(k_scale_by, gl, kBlock, 0, stream, v1 - v0,
                               dinv.p + v0, y + v0);
            DNS_HIP(hipGetLastError());
        }
        return comm->allgatherv(y, st_v, stream);
    };
    double lam = 0;
    hipLaunchKernelGGL(k_fill_wave, g, kBlock, 0, stream, nv, x, 0.37, 7.0, 0);
    for (int it = 0; it < 30; ++it) {
        DNS_TRY(product());
        double xx, yy;
        DNS_TRY(dot_host(nv, x, x, &xx));
        DNS_TRY(dot_host(nv, y, y, &yy));
        if (!(yy > 0.0) || !(xx > 0.0))
            return fail(DNS_BREAKDOWN, "power iteration broke down");
        lam = std::sqrt(yy / xx);
        hipLaunchKernelGGL(k_axpby, g, kBlock, 0, stream, (int64_t)nv,
                           1.0 / std::sqrt(yy), y, 0.0, x);
    }
    const double lmax = lam;
    const double shift = 1.05 * lmax;
    hipLaunchKernelGGL(k_fill_wave, g, kBlock, 0, stream, nv, x, 0.61, 7.0, 1);
    double mu = 0;
    for (int it = 0; it < 50; ++it) {
        DNS_TRY(product());
        hipLaunchKernelGGL(k_axpby, g, kBlock, 0, stream, (int64_t)nv, shift,
                           x, -1.0, y);
        double xx, yy;
        DNS_TRY(dot_host(nv, x, x, &xx));
        DNS_TRY(dot_host(nv, y, y, &yy));
        if (!(yy > 0.0) || !(xx > 0.0)) break;
        mu = std::sqrt(yy / xx);
        hipLaunchKernelGGL(k_axpby, g, kBlock, 0, stream, (int64_t)nv,
                           1.0 / std::sqrt(yy), y, 0.0, x);
    }
    DNS_HIP(hipStreamSynchronize(stream));
    double lmin = shift - mu;
    if (!(lmin > 0.0)) lmin = lmax / 100.0;
    lam_lo = popts.eig_lo_safety * lmin;
    lam_hi = popts.eig_hi_safety * lmax;
    return DNS_OK;
}

// The rows of F and J^T this rank's part of the set-up reads, fetched from
// their owners: R_0 = own velocity rows + the columns of the own rows of J,
// R_{s+1} = R_s + the columns of the rows R_s of F; the polynomial of degree
// k - 1 reads the rows R_{k-2} of F and the diagonal and the rows of J^T on
// R_{k-1}.  `Fx`, `JTx`: global shape, own + fetched rows; `dv`: 1 / diag(F) on
// R_{k-1} (1 elsewhere).
int dns_saddle::extend_rows_for_setup(dns::HostCsr &Fx, dns::HostCsr &JTx,
                                      std::vector<double> &dv) {
    using namespace dns;
    const int me = comm->rank;
    const int v0 = st_v[me], v1 = st_v[me + 1], p0 = st_p[me], p1 = st_p[me + 1];
    const int k = popts.cheb_degree;
    std::vector<char> inR((size_t)nv, 0);
    std::vector<int> fresh;            // R_s \ R_{s-1}, sorted
    for (int i = v0; i < v1; ++i) inR[i] = 1;
    for (int r = p0; r < p1; ++r)
        for (int e = Jh.rowptr[r]; e < Jh.rowptr[r + 1]; ++e)
            inR[Jh.colidx[e]] = 1;
    std::vector<int> ghost;            // all rows of other ranks, sorted at the end
    for (int i = 0; i < nv; ++i)
        if (inR[i]) fresh.push_back(i);
    Fx = Fh;
    for (int s = 0; s < k; ++s) {
        // rows of `fresh` that are not here yet (all but the own ones)
        std::vector<int> want;
        for (int i : fresh)
            if (i < v0 || i >= v1) want.push_back(i);
        HostCsr got;
        DNS_TRY(fetch_rows(Fh, st_v, want, got));
        if (!want.empty()) Fx = host_merge_rows(Fx, got);
        ghost.insert(ghost.end(), want.begin(), want.end());
        if (s + 1 == k) break;
        std::vector<int> next;
        for (int i : fresh)
            for (int e = Fx.rowptr[i]; e < Fx.rowptr[i + 1]; ++e) {
                const int c = Fx.colidx[e];
                if (!inR[c]) {
                    inR[c] = 1;
                    next.push_back(c);
                }
            }
        std::sort(next.begin(), next.end());
        fresh.swap(next);
    }
    std::sort(ghost.begin(), ghost.end());
    {
        HostCsr got;
        DNS_TRY(fetch_rows(JTh, st_v, ghost, got));
        JTx = ghost.empty() ? JTh : host_merge_rows(JTh, got);
    }
    dv.assign((size_t)nv, 1.0);
    for (int i = 0; i < nv; ++i) {
        if (!inR[i]) continue;
        double d = 0.0;
        for (int e = Fx.rowptr[i]; e < Fx.rowptr[i + 1]; ++e)
            if (Fx.colidx[e] == i) d += Fx.vals[e];
        dv[i] = (d != 0.0) ? 1.0 / d : 1.0;
    }
    if (getenv("DNS_DEBUG"))
        fprintf(stderr,
                "[dns] setup (rows of rank %d): %zu ghost rows of F and JT "
                "(%d own), %lld + %lld entries fetched\n",
                me, ghost.size(), v1 - v0,
                (long long)(Fx.nnz() - Fh.nnz()),
                (long long)(JTx.nnz() - JTh.nnz()));
    return DNS_OK;
}

// A bound of the skew radius (hostcsr.hpp, host_skew_radius) from the own rows
// and the first ring of ghost rows: the largest absolute row sum of
// D^-1/2 (F - F^T)/2 D^-1/2, which is >= its spectral radius; 0 for a matrix
// that is symmetric up to rounding.
int dns_saddle::skew_bound_rows(const dns::HostCsr &Fx, double *eta) {
    using namespace dns;
    const int me = comm->rank;
    const int v0 = st_v[me], v1 = st_v[me + 1];
    auto diag_of = [&](int i) {
        for (int e = Fx.rowptr[i]; e < Fx.rowptr[i + 1]; ++e)
            if (Fx.colidx[e] == i) return Fx.vals[e];
        return 0.0;
    };
    double mx = 0.0, amax = 0.0, rowsum = 0.0;
    for (int i = v0; i < v1; ++i) {
        const double di = diag_of(i);
        const double si = di > 0.0 ? 1.0 / std::sqrt(di) : 1.0;
        double s = 0.0;
        for (int e = Fx.rowptr[i]; e < Fx.rowptr[i + 1]; ++e) {
            const int j = Fx.colidx[e];
            const double a = Fx.vals[e];
            amax = std::max(amax, std::fabs(a));
            if (j == i) continue;
            double b = 0.0;                        // F(j, i)
            const int *lo = Fx.colidx.data() + Fx.rowptr[j];
            const int *hi = Fx.colidx.data() + Fx.rowptr[j + 1];
            const int *it = std::lower_bound(lo, hi, i);
            if (it != hi && *it == i) b = Fx.vals[(size_t)(it - Fx.colidx.data())];
            const double dj = diag_of(j);
            const double sj = dj > 0.0 ? 1.0 / std::sqrt(dj) : 1.0;
            const double kk = 0.5 * (a - b);
            mx = std::max(mx, std::fabs(kk));
            s += std::fabs(kk) * si * sj;
        }
        rowsum = std::max(rowsum, s);
    }
    double gmx = 0.0, gamax = 0.0, grow = 0.0;
    DNS_TRY(all_ranks_max(mx, &gmx));
    DNS_TRY(all_ranks_max(amax, &gamax));
    DNS_TRY(all_ranks_max(rowsum, &grow));
    *eta = (gmx > 1e-12 * gamax) ? grow : 0.0;
    return DNS_OK;
}

static int64_t host_csr_bytes(const dns::HostCsr &a) {
    return 4 * (int64_t)(a.rowptr.size() + a.colidx.size()) +
           8 * (int64_t)a.vals.size();
}

int dns_saddle_host_bytes(dns_saddle *h, int64_t *kept, int64_t *setup) try {
    if (!h) return fail(DNS_ERR_BAD_ARGUMENT, "null handle");
    int64_t b = host_csr_bytes(h->Fh) + host_csr_bytes(h->Jh) +
                host_csr_bytes(h->JTh) + host_csr_bytes(h->Fpc_h);
    for (const auto &pm : h->mg_prol_h) b += host_csr_bytes(pm);
    for (const auto &lv : h->mg)
        b += host_csr_bytes(lv.Sh) + host_csr_bytes(lv.Apreh) +
             host_csr_bytes(lv.Rrh) + host_csr_bytes(lv.Qqh);
    if (kept) *kept = b;
    if (setup) *setup = h->host_setup_bytes;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_saddle_create_rows(int device, dns_comm *comm, int32_t nv, int32_t np,
                           const dns_csr *f_rows, const dns_csr *jt_rows,
                           const dns_csr *j_rows, dns_saddle **out) try {
    if (!out) return fail(DNS_ERR_BAD_ARGUMENT, "null output handle");
    *out = nullptr;
    auto h = std::make_unique<dns_saddle>();
    DNS_TRY(h->init_rows(device, comm, nv, np, f_rows, jt_rows, j_rows));
    *out = h.release();
    return DNS_OK;
} DNS_CAPI_CATCH
