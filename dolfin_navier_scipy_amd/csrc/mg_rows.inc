// The multigrid hierarchy of the Schur block formed BY ROWS (partitioned
// set-up): a level that runs row-partitioned (solver.hpp, MgLevel::part;
// schur_mg_apply_dist) is never put together as a whole matrix.  The algebra
// is that of the whole hierarchy (mg_host.hpp) on the rank's rows [f0, f1) of
// S_l and its rows [c0, c1) of level l+1; what this file adds is the
// communication:
//   * 1 / diag(S_l) is all-gathered (one vector);
//   * the power iteration of the damping all-gathers its iterate after each
//     product -- the same sums in the same order, the same damping bit for bit;
//   * the rows of S_l the rank's rows of P^T reference beyond its own are
//     fetched from their owners (fetch_rows, one exchange per level); S_l P on
//     those rows is formed locally (P is replicated: it is the geometry);
//   * the halo lists of the own rows are exchanged (gather_need_lists).
// The first level that runs replicated is all-gathered and the rest of the
// hierarchy built from it as on one GPU (build_mg_levels).

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
    for (int l = 0; l <= Lp; ++l)
        mg[l].st = (l == 0) ? st_p : partition_starts(nl[l], P);
    HostCsr Sloc = S0loc;                  // own rows of the level, compact
    for (int l = 0; l < Lp; ++l) {
        MgLevel &lv = mg[l];
        const int n = nl[l];
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
        std::vector<double> dv, dj;
        mg_diagonals(Sg, f0, f1, dv, dj);
        DNS_TRY(allgather_host(dv, st));
        double lmax = 1.0;
        DNS_TRY(mg_jacobi_lmax(
            Sg, f0, f1, dj,
            [&](std::vector<double> &y) { return allgather_host(y, st); },
            &lmax));
        mg_damping(lmax, mg_cheb && mg_nu == 2, mg_cheb_alpha, &lv.omega,
                   &lv.omega2);
        // the rows of S the own rows of P^T reference, from their owners
        const HostCsr PTc = host_row_slice(host_transpose(Pm), c0, c1);
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
        const MgOps o = mg_fused22_ops(Sx, SPx, Pm, PTc, f0, f1, dv,
                                       lv.omega, lv.omega2);
        // halo lists from the own patterns
        lv.coarse_replicated = (l + 1 == Lp);
        {
            std::vector<std::vector<int>> mineF, mineC;
            mg_need_lists(Sloc, o.Apre, o.Qq, 0, f1 - f0, o.Rr, 0, c1 - c0, st,
                          stc, me, lv.coarse_replicated, mineF, mineC);
            std::vector<std::vector<std::vector<int>>> needF, needC;
            DNS_TRY(gather_need_lists(mineF, needF));
            DNS_TRY(gather_need_lists(mineC, needC));
            DNS_TRY(lv.planF.build(needF, me, P, stream));
            DNS_TRY(lv.planC.build(needC, me, P, stream));
        }
        // this rank's row blocks in HBM
        DNS_TRY(upload_mg_ops(lv, &Sloc, &o.Apre, &o.Rr, &o.Qq, false));
        DNS_TRY(lv.dinv.alloc((size_t)n));
        DNS_TRY(lv.dinv.upload(dv.data(), dv.size(), stream));
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
