// The multigrid hierarchy of the Schur block formed BY ROWS (partitioned
// set-up): a level that runs row-partitioned (solver.hpp, MgLevel::part;
// schur_mg_apply_dist) is never put together as a whole matrix.  Per such level
// l, with this rank's rows [f0, f1) of S_l and its rows [c0, c1) of level l+1:
//   * 1 / diag(S_l) is all-gathered (one vector);
//   * the damping comes from the power iteration of host_jacobi_lmax with the
//     product formed by rows and the iterate all-gathered -- the same sums in
//     the same order, the same damping bit for bit;
//   * the rows of S_l the rank's rows of P^T reference beyond its own are
//     fetched from their owners (fetch_rows, one exchange per level); S_l P on
//     those rows is formed locally (P is replicated: it is the geometry);
//   * Apre, Qq (own fine rows), Rr = [P^T, -P^T S_l] and S_{l+1} = P^T S_l P
//     (own coarse rows) are row-wise products of these: equal, entry for entry,
//     to the rows build_mg_levels cuts out of the whole operators;
//   * halo lists from the own patterns, exchanged (gather_need_lists).
// The first level that runs replicated is all-gathered and the rest of the
// hierarchy built from it as on one GPU (build_mg_levels).

namespace dns {

// alpha on the diagonal of the rows [r0, r1) of an n x n matrix, other rows empty
inline HostCsr host_diag_range(int n, int r0, int r1, double alpha) {
    HostCsr h;
    h.nrows = h.ncols = n;
    h.rowptr.assign((size_t)n + 1, 0);
    h.colidx.resize((size_t)(r1 - r0));
    h.vals.assign((size_t)(r1 - r0), alpha);
    for (int i = r0; i < r1; ++i) {
        h.colidx[(size_t)(i - r0)] = i;
        h.rowptr[(size_t)i + 1] = i - r0 + 1;
    }
    for (int i = r1; i < n; ++i) h.rowptr[(size_t)i + 1] = r1 - r0;
    return h;
}

}  // namespace dns

// rows [st[me], st[me+1]) of a host vector -> every rank's rows everywhere
int dns_saddle::allgather_host(std::vector<double> &v,
                               const std::vector<int> &st) {
    using namespace dns;
    const int me = comm->rank;
    DevBuf<double> buf;
    DNS_TRY(buf.alloc(std::max<size_t>(1, v.size())));
    const int a = st[me], b = st[me + 1];
    if (b > a) DNS_TRY(upload_to(buf.p + a, v.data() + a, (size_t)(b - a), stream));
    DNS_TRY(comm->allgatherv(buf.p, st, stream));
    DNS_TRY(buf.download(v.data(), v.size(), stream));
    DNS_HIP(hipStreamSynchronize(stream));
    return DNS_OK;
}

int dns_saddle::build_mg_schur_rows(const dns::HostCsr &S0loc) {
    using namespace dns;
    const int P = comm->nranks, me = comm->rank;
    DNS_TRY(mg_prepare(np));
    const int L = (int)mg.size();
    // level sizes and how many levels run row-partitioned (setup_dist_mg's rule)
    std::vector<int> nl((size_t)L);
    nl[0] = np;
    for (int l = 1; l < L; ++l) nl[l] = mg_prol_h[(size_t)l - 1].ncols;
    int Lp = 0;
    if (mg_fused && P > 1 && mg_rows_knob)
        while (Lp + 1 < L && nl[Lp] >= mg_part_min) ++Lp;
    if (Lp == 0) {
        HostCsr S;
        DNS_TRY(gather_csr_rows(S0loc, st_p, np, S));
        return build_mg_levels(0, std::move(S));
    }
    for (int l = 0; l <= Lp; ++l) {
        MgLevel &lv = mg[l];
        if (l == 0) {
            lv.st = st_p;
        } else {
            lv.st.assign((size_t)P + 1, 0);
            for (int r = 0; r < P; ++r) {
                int a = 0, b = 0;
                dns_partition_range(nl[l], P, r, &a, &b);
                lv.st[r] = a;
                lv.st[r + 1] = b;
            }
        }
    }
    HostCsr Sloc = S0loc;                  // own rows of the level, compact
    for (int l = 0; l < Lp; ++l) {
        MgLevel &lv = mg[l];
        const int n = nl[l], nc = nl[l + 1];
        const std::vector<int> &st = lv.st, &stc = mg[l + 1].st;
        const int f0 = st[me], f1 = st[me + 1], c0 = stc[me], c1 = stc[me + 1];
        lv.n = n;
        DNS_TRY(lv.x.alloc((size_t)n));
        DNS_TRY(lv.b.alloc((size_t)n));
        DNS_TRY(lv.r.alloc((size_t)n));
        DNS_TRY(lv.x2.alloc((size_t)n));
        const HostCsr &Pm = mg_prol_h[l];
        if (Pm.nrows != n || Sloc.nrows != f1 - f0 || Sloc.ncols != n)
            return fail(DNS_ERR_BAD_ARGUMENT,
                        "prolongation %d has %d rows, level has %d", l, Pm.nrows,
                        n);
        const dns_csr slv = Sloc.view();
        const HostCsr Sg = host_embed_rows(&slv, f0, n);
        // 1 / diag (smoothing) and the diagonal as host_jacobi_lmax reads it
        std::vector<double> dv((size_t)n, 1.0), dj((size_t)n, 1.0);
        for (int i = f0; i < f1; ++i) {
            double d = 0.0;
            for (int k = Sg.rowptr[i]; k < Sg.rowptr[i + 1]; ++k)
                if (Sg.colidx[k] == i) {
                    d += Sg.vals[k];
                    if (Sg.vals[k] != 0.0) dj[i] = 1.0 / Sg.vals[k];
                }
            dv[i] = (d != 0.0) ? 1.0 / d : 1.0;
        }
        DNS_TRY(allgather_host(dv, st));
        // power iteration of host_jacobi_lmax, the product by rows
        double lmax = 1.0;
        {
            std::vector<double> x((size_t)n), y((size_t)n, 0.0);
            for (int i = 0; i < n; ++i) x[i] = 1.0 + 0.5 * std::sin(0.37 * i + 1.0);
            for (int it = 0; it < 20; ++it) {
                for (int i = f0; i < f1; ++i) {
                    double s = 0.0;
                    for (int k = Sg.rowptr[i]; k < Sg.rowptr[i + 1]; ++k)
                        s += Sg.vals[k] * x[Sg.colidx[k]];
                    y[i] = dj[i] * s;
                }
                DNS_TRY(allgather_host(y, st));
                double nx = 0.0, ny = 0.0;
                for (int i = 0; i < n; ++i) {
                    nx += x[i] * x[i];
                    ny += y[i] * y[i];
                }
                lmax = std::sqrt(ny / nx);
                const double sc = 1.0 / std::sqrt(ny);
                for (int i = 0; i < n; ++i) x[i] = y[i] * sc;
            }
            lmax = std::max(1e-300, lmax);
        }
        lv.omega = lv.omega2 = 4.0 / (3.0 * lmax);
        if (mg_cheb && mg_nu == 2) {
            const double hi = 1.05 * lmax, lo = lmax / mg_cheb_alpha;
            const double mid = 0.5 * (hi + lo), rad = 0.5 * (hi - lo);
            const double c = 0.70710678118654752;    // cos(pi / 4)
            lv.omega = 1.0 / (mid + rad * c);
            lv.omega2 = 1.0 / (mid - rad * c);
        }
        // the rows of S the own rows of P^T reference, from their owners
        const HostCsr PT = host_transpose(Pm);
        const HostCsr PTc = host_row_slice(PT, c0, c1);
        HostCsr Sx;
        {
            std::vector<char> mark((size_t)n, 0);
            for (int k : PTc.colidx) mark[k] = 1;
            std::vector<int> want;
            for (int i = 0; i < n; ++i)
                if (mark[i] && (i < f0 || i >= f1)) want.push_back(i);
            HostCsr got;
            DNS_TRY(fetch_rows(Sg, st, want, got));
            Sx = want.empty() ? Sg : host_merge_rows(Sg, got);
        }
        const HostCsr SPx = host_spgemm(Sx, Pm);           // own + fetched rows
        std::vector<double> wd((size_t)n, 0.0);
        for (int i = f0; i < f1; ++i) wd[i] = lv.omega * dv[i];
        const HostCsr I = host_diag_range(n, f0, f1, 1.0);
        HostCsr WS = Sg;
        host_scale_rows(wd, WS);                           // w1 D^-1 S, own rows
        const HostCsr T = host_add(1.0, I, -1.0, WS);
        HostCsr Ap = host_add(lv.omega + lv.omega2, I, -lv.omega2, WS);
        for (size_t k = 0; k < Ap.vals.size(); ++k)        // ... D^-1
            Ap.vals[k] *= dv[Ap.colidx[k]];
        HostCsr mPTS = host_spgemm(PTc, Sx);               // own coarse rows
        for (double &v : mPTS.vals) v = -v;
        const HostCsr Rr = host_hstack(PTc, mPTS);
        HostCsr WSP = host_row_slice(SPx, f0, f1);
        {
            const std::vector<double> wl(wd.begin() + f0, wd.begin() + f1);
            host_scale_rows(wl, WSP);
        }
        const HostCsr Qq = host_hstack(
            host_row_slice(T, f0, f1),
            host_add(1.0, host_row_slice(Pm, f0, f1), -1.0, WSP));
        const HostCsr Apl = host_row_slice(Ap, f0, f1);
        // halo lists from the own patterns
        lv.coarse_replicated = (l + 1 == Lp);
        {
            std::vector<unsigned char> mf((size_t)n, 0), mc((size_t)nc, 0);
            for (int c : Apl.colidx) mf[c] = 1;
            for (int c : Sloc.colidx) mf[c] = 1;
            for (int c : Qq.colidx) {
                if (c < n) mf[c] = 1;
                else mc[c - n] = 1;
            }
            for (int c : Rr.colidx) mf[c < n ? c : c - n] = 1;
            std::vector<std::vector<int>> mineF((size_t)P), mineC((size_t)P);
            for (int q = 0; q < P; ++q) {
                if (q == me) continue;
                for (int c = st[q]; c < st[q + 1]; ++c)
                    if (mf[c]) mineF[q].push_back(c);
                if (!lv.coarse_replicated)
                    for (int c = stc[q]; c < stc[q + 1]; ++c)
                        if (mc[c]) mineC[q].push_back(c);
            }
            std::vector<std::vector<std::vector<int>>> needF, needC;
            DNS_TRY(gather_need_lists(mineF, needF));
            DNS_TRY(gather_need_lists(mineC, needC));
            DNS_TRY(lv.planF.build(needF, me, P, stream));
            DNS_TRY(lv.planC.build(needC, me, P, stream));
        }
        // this rank's row blocks in HBM
        {
            const dns_csr av = Sloc.view(), bv = Apl.view(), cv = Rr.view(),
                          qv = Qq.view();
            DNS_TRY(lv.S.upload(&av, stream));
            DNS_TRY(lv.Apre.upload(&bv, stream));
            DNS_TRY(lv.Rr.upload(&cv, stream));
            DNS_TRY(lv.Qq.upload(&qv, stream));
            if (fp32_store)
                for (CsrDev *o : {&lv.Apre, &lv.Rr, &lv.Qq, &lv.S})
                    if (streams(*o))
                        DNS_TRY(to_f32(o->vals.p, o->vals32,
                                       (size_t)o->nnz + 2));
            DNS_TRY(lv.dinv.alloc((size_t)n));
            DNS_TRY(lv.dinv.upload(dv.data(), dv.size(), stream));
        }
        // sizes of the whole operators (byte counts of the roofline model)
        {
            double cnt = (double)Sloc.nnz();
            DNS_TRY(allreduce_host(&cnt, 1));
            lv.nnz_S = (int64_t)cnt;
            lv.nnz_P = Pm.nnz();
        }
        lv.part = true;
        host_setup_bytes +=
            4 * (int64_t)(Sx.rowptr.size() + Sx.colidx.size() +
                          SPx.rowptr.size() + SPx.colidx.size()) +
            8 * (int64_t)(Sx.vals.size() + SPx.vals.size());
        // own rows of the next level
        Sloc = host_spgemm(PTc, SPx);
    }
    mg_rows_parts = Lp;
    // the first replicated level, whole, and the rest of the hierarchy from it
    HostCsr S;
    DNS_TRY(gather_csr_rows(Sloc, mg[Lp].st, nl[Lp], S));
    return build_mg_levels(Lp, std::move(S));
}
