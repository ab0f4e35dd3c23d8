// Row-partitioned solve over several GPUs (included by dns_amd.hip).
//
// Partition: rank r owns the velocity rows [v0, v1) and the pressure rows
// [p0, p1) (block partitions of the RCM-ordered dofs: both ranges describe
// the same slab of the mesh).  In HBM a rank keeps ONLY its rows of
//   K    = [[F, JT], [J, 0]]   (velocity rows, then pressure rows; RowMap)
//   Gc   = [G, -G JT]          explicit Fh^-1 (velocity rows)
//   J Fh^-1                    (pressure rows; full block factorisation)
// with global column indices.  Vectors stay full length on every rank; valid
// are a rank's own entries plus the halo entries it has received.  The Schur
// block: the dense fp32/fp64 inverse is held by COLUMNS (a rank forms its share
// of every row of zp = -Sinv tau from its own entries of tau; the shares are
// all-reduced: NP doubles, ONE collective); the multigrid Schur block runs
// replicated on the all-gathered tau (NP doubles as well) or, for levels of at
// least mg_part_min rows, row-partitioned (setup_dist_mg below).
//
// Per Arnoldi step (dense Schur block): halo(src_v) -> tau (own rows) -> head
// (V_j everywhere it is valid, this rank's share of zp_j) -> all-reduce(zp_j)
// -> zv = Gc_loc [V_j,v; zp_j] (own rows) -> halo(zv) -> w = K_loc z + dots
// over own rows -> ONE all-reduce of the j+2 scalars: four collectives.
//
// Gram-Schmidt: `reorth == 2` runs the fused form (norm by Pythagoras) -- one
// all-reduce per step; a cycle that trips the cancellation guard ends early
// and dns_saddle::gmres restarts from the current iterate in the explicit
// mode (`reorth != 2`: k_orth on the own rows and a SECOND all-reduce for
// ||w||^2), so the fallback cannot loop.

struct dns_dist_data {
    int v0 = 0, v1 = 0, p0 = 0, p1 = 0;
    dns::RowMap kmap = {0, 0, 0, 0};
    dns_halo_plan planK;      // velocity entries the rows of K_loc reference
    dns_halo_plan planU;      // ... the rows of Gc_loc and (J Fh^-1)_loc do
    bool schur_cols = false;  // dense Schur inverse held by columns [p0, p1)
    int schur_ld = 0;         // ... with this row stride
    // needK[r][q]: the velocity entries rank r needs from rank q for its rows
    // of K (kept for the attached time steppers: their halo is this plus the
    // footprint of their own operators)
    std::vector<std::vector<std::vector<int>>> needK;
};

// every rank's lists of what it needs from every other rank, from each rank's
// OWN lists (partitioned set-up: a rank knows the patterns of its rows only):
// counts, then the concatenated lists, through two all-gathers
int dns_saddle::gather_need_lists(
    const std::vector<std::vector<int>> &mine,
    std::vector<std::vector<std::vector<int>>> &all) {
    using namespace dns;
    const int P = comm->nranks, me = comm->rank;
    std::vector<double> cnt((size_t)P * P, 0.0);
    for (int q = 0; q < P; ++q) cnt[(size_t)me * P + q] = (double)mine[q].size();
    DevBuf<double> buf;
    DNS_TRY(buf.alloc((size_t)P * P));
    DNS_TRY(buf.upload(cnt.data(), cnt.size(), stream));
    std::vector<int> st((size_t)P + 1);
    for (int r = 0; r <= P; ++r) st[r] = r * P;
    DNS_TRY(comm->allgatherv(buf.p, st, stream));
    DNS_TRY(buf.download(cnt.data(), cnt.size(), stream));
    DNS_HIP(hipStreamSynchronize(stream));
    std::vector<int> off((size_t)P + 1, 0);
    for (int r = 0; r < P; ++r) {
        int64_t t = 0;
        for (int q = 0; q < P; ++q) t += (int64_t)cnt[(size_t)r * P + q];
        if ((int64_t)off[r] + t > (int64_t)INT32_MAX)
            return fail(DNS_ERR_BAD_ARGUMENT, "halo lists too long");
        off[r + 1] = off[r] + (int)t;
    }
    std::vector<double> flat((size_t)std::max(1, off[P]), 0.0);
    {
        size_t k = (size_t)off[me];
        for (int q = 0; q < P; ++q)
            for (int c : mine[q]) flat[k++] = (double)c;
    }
    DNS_TRY(buf.alloc(flat.size()));
    DNS_TRY(buf.upload(flat.data(), flat.size(), stream));
    DNS_TRY(comm->allgatherv(buf.p, off, stream));
    DNS_TRY(buf.download(flat.data(), flat.size(), stream));
    DNS_HIP(hipStreamSynchronize(stream));
    all.assign((size_t)P, std::vector<std::vector<int>>());
    for (int r = 0; r < P; ++r) {
        all[r].assign((size_t)P, std::vector<int>());
        size_t k = (size_t)off[r];
        for (int q = 0; q < P; ++q) {
            const int c = (int)cnt[(size_t)r * P + q];
            all[r][q].resize((size_t)c);
            for (int i = 0; i < c; ++i) all[r][q][i] = (int)flat[k++];
        }
    }
    return DNS_OK;
}

// the rows [starts[me], starts[me+1]) of a sparse matrix on every rank -> the
// whole matrix on every rank (row lengths, column indices and values through
// three all-gathers; the indices travel as doubles)
int dns_saddle::gather_csr_rows(const dns::HostCsr &loc,
                                const std::vector<int> &starts, int ncols,
                                dns::HostCsr &out) {
    using namespace dns;
    const int P = comm->nranks, me = comm->rank;
    const int nr = starts[P];
    std::vector<double> len((size_t)std::max(1, nr), 0.0);
    for (int i = 0; i < loc.nrows; ++i)
        len[(size_t)starts[me] + i] = (double)(loc.rowptr[i + 1] - loc.rowptr[i]);
    DevBuf<double> buf;
    DNS_TRY(buf.alloc(len.size()));
    DNS_TRY(buf.upload(len.data(), len.size(), stream));
    DNS_TRY(comm->allgatherv(buf.p, starts, stream));
    DNS_TRY(buf.download(len.data(), len.size(), stream));
    DNS_HIP(hipStreamSynchronize(stream));
    out = HostCsr();
    out.nrows = nr;
    out.ncols = ncols;
    out.rowptr.assign((size_t)nr + 1, 0);
    int64_t tot = 0;
    for (int i = 0; i < nr; ++i) {
        tot += (int64_t)len[i];
        if (tot > (int64_t)INT32_MAX)
            return fail(DNS_ERR_BAD_ARGUMENT,
                        "Schur complement too large to be gathered");
        out.rowptr[(size_t)i + 1] = (int)tot;
    }
    std::vector<int> off((size_t)P + 1);
    for (int r = 0; r <= P; ++r) off[r] = out.rowptr[starts[r]];
    std::vector<double> flat((size_t)std::max<int64_t>(1, tot), 0.0);
    DNS_TRY(buf.alloc(flat.size()));
    // (column indices first, then the values, through the same buffer)
    for (size_t k = 0; k < loc.colidx.size(); ++k)
        flat[(size_t)off[me] + k] = (double)loc.colidx[k];
    DNS_TRY(buf.upload(flat.data(), flat.size(), stream));
    DNS_TRY(comm->allgatherv(buf.p, off, stream));
    DNS_TRY(buf.download(flat.data(), flat.size(), stream));
    DNS_HIP(hipStreamSynchronize(stream));
    out.colidx.resize((size_t)tot);
    for (int64_t k = 0; k < tot; ++k) out.colidx[(size_t)k] = (int)flat[(size_t)k];
    for (size_t k = 0; k < loc.vals.size(); ++k)
        flat[(size_t)off[me] + k] = loc.vals[k];
    DNS_TRY(buf.upload(flat.data(), flat.size(), stream));
    DNS_TRY(comm->allgatherv(buf.p, off, stream));
    out.vals.resize((size_t)tot);
    DNS_TRY(buf.download(out.vals.data(), (size_t)tot, stream));
    DNS_HIP(hipStreamSynchronize(stream));
    return DNS_OK;
}

// The explicit preconditioner of a row-partitioned handle, every rank forming
// ITS rows only: rows of the polynomial G for its velocity rows and for the
// columns of its rows of J (row recurrences are independent of each other),
// from them its rows of Gc = [G, -G JT], of J G and of S = J G JT.  Only the
// Schur complement is put together on every rank (dense: all-gathered and
// inverted by every rank; multigrid: the sparse rows all-gathered, hierarchy
// from the whole).  The rows are the ones the replicated set-up forms, bit for
// bit: row-wise products do not depend on which other rows are formed.
int dns_saddle::build_explicit_part(bool dense_schur, const dns::HostCsr &DF,
                                    const std::vector<double> &dv,
                                    const dns::HostCsr &JTx) {
    using namespace dns;
    const bool dbg = getenv("DNS_DEBUG") != nullptr;
    double t0 = wall_now();
    auto lap = [&](const char *what) {
        if (!dbg) return;
        const double t1 = wall_now();
        fprintf(stderr, "[dns] setup (rows of rank %d) %-24s %8.1f ms\n",
                comm->rank, what, 1e3 * (t1 - t0));
        t0 = t1;
    };
    const int me = comm->rank;
    const int v0 = st_v[me], v1 = st_v[me + 1], p0 = st_p[me], p1 = st_p[me + 1];
    std::vector<int> rows;
    {
        std::vector<char> need((size_t)nv, 0);
        for (int i = v0; i < v1; ++i) need[i] = 1;
        for (int r = p0; r < p1; ++r)
            for (int k = Jh.rowptr[r]; k < Jh.rowptr[r + 1]; ++k)
                need[Jh.colidx[k]] = 1;
        for (int i = 0; i < nv; ++i)
            if (need[i]) rows.push_back(i);
    }
    // The index set the rows reach: R = `rows` and k - 1 rings of the pattern of
    // DF around them (k = degree).  Everything below runs on R renumbered
    // 0 .. |R| - 1 (monotone: sums keep their order, results their bits): the
    // scratch of the row recurrences and of the products is |R| long per host
    // thread instead of NV, and the work is spread over the rows that exist.
    std::vector<int> R, loc_of((size_t)nv, -1);
    {
        std::vector<char> in((size_t)nv, 0);
        std::vector<int> fresh = rows, next;
        for (int i : rows) in[i] = 1;
        R = rows;
        for (int s = 0; s + 1 < popts.cheb_degree; ++s) {
            next.clear();
            for (int i : fresh)
                for (int e = DF.rowptr[i]; e < DF.rowptr[i + 1]; ++e) {
                    const int c = DF.colidx[e];
                    if (!in[c]) {
                        in[c] = 1;
                        next.push_back(c);
                    }
                }
            R.insert(R.end(), next.begin(), next.end());
            fresh.swap(next);
        }
        std::sort(R.begin(), R.end());
        for (size_t q = 0; q < R.size(); ++q) loc_of[R[q]] = (int)q;
    }
    const int nloc = (int)R.size();
    HostCsr Gp;                            // rows `rows` of G on the index set R
    {
        const HostCsr DFc = host_compact_rows(DF, R, &loc_of);
        std::vector<double> dvc((size_t)nloc);
        for (int q = 0; q < nloc; ++q) dvc[q] = dv[R[q]];
        std::vector<int> rows_c(rows.size());
        for (size_t q = 0; q < rows.size(); ++q) rows_c[q] = loc_of[rows[q]];
        Gp = host_cheb_poly(DFc, dvc, theta, c1, c2, popts.drop_tol, &rows_c);
        host_setup_bytes = 4 * (int64_t)(DFc.rowptr.size() + DFc.colidx.size()) +
                           8 * (int64_t)(DFc.vals.size() + dvc.size());
    }
    lap("polynomial G");
    const HostCsr GJT = host_spgemm(Gp, host_compact_rows(JTx, R, nullptr));
    lap("G*JT");
    auto to_global = [&](HostCsr &A) {     // columns back to the numbering of NV
        for (int &c : A.colidx) c = R[c];
        A.ncols = nv;
    };
    {
        // (the own rows are consecutive in R as they are in NV)
        const int l0 = v1 > v0 ? loc_of[v0] : 0;
        HostCsr Gown = host_row_slice(Gp, l0, l0 + (v1 - v0));
        to_global(Gown);
        HostCsr mGJT = host_row_slice(GJT, l0, l0 + (v1 - v0));
        for (auto &v : mGJT.vals) v = -v;
        tmp_Gch = host_hstack(Gown, mGJT);
    }
    HostCsr Jloc = host_row_slice(Jh, p0, p1);      // ... on the index set R
    for (int &c : Jloc.colidx) c = loc_of[c];
    Jloc.ncols = nloc;
    tmp_JGh = HostCsr();
    if (popts.factorization == DNS_FACT_FULL) {
        tmp_JGh = host_spgemm(Jloc, Gp);
        to_global(tmp_JGh);
        DNS_TRY(tau.alloc((size_t)std::max(1, np)));
        have_jg = true;
        lap("J*G");
    }
    tmp_presliced = true;
    {
        auto hb = [](const HostCsr &a) {
            return 4 * (int64_t)(a.rowptr.size() + a.colidx.size()) +
                   8 * (int64_t)a.vals.size();
        };
        host_setup_bytes += hb(DF) + hb(Gp) + hb(GJT) + hb(tmp_Gch) +
                            hb(tmp_JGh) + hb(Jloc) + 8 * (int64_t)dv.size() +
                            4 * (int64_t)(R.size() + loc_of.size()) +
                            (&JTx != &JTh ? hb(JTx) : 0);
    }
    if (dense_schur) {
        if ((int64_t)np * np > (int64_t)INT32_MAX)
            return fail(DNS_ERR_BAD_ARGUMENT,
                        "dense Schur complement too large to be gathered");
        const HostCsr Sl = host_spgemm(Jloc, GJT);
        std::vector<double> sd((size_t)std::max(1, p1 - p0) * np, 0.0);
        for (int i = 0; i < p1 - p0; ++i)
            for (int k = Sl.rowptr[i]; k < Sl.rowptr[i + 1]; ++k)
                sd[(size_t)i * np + Sl.colidx[k]] = Sl.vals[k];
        DNS_TRY(sinv.alloc((size_t)np * np));
        if (p1 > p0)
            DNS_TRY(upload_to(sinv.p + (size_t)p0 * np, sd.data(),
                              (size_t)(p1 - p0) * np, stream));
        std::vector<int> st((size_t)comm->nranks + 1);
        for (int r = 0; r <= comm->nranks; ++r) st[r] = st_p[r] * np;
        DNS_TRY(comm->allgatherv(sinv.p, st, stream));
        DNS_HIP(hipStreamSynchronize(stream));
        lap("rows of S, all-gather");
        DNS_TRY(invert_dense(sinv.p, np));
        lap("Gauss-Jordan inverse");
    } else if (popts.schur == DNS_SCHUR_MG) {
        const HostCsr Sl = host_spgemm(Jloc, GJT);
        lap("rows of S");
        // (levels that run row-partitioned are formed by rows, mg_rows.inc)
        DNS_TRY(build_mg_schur_rows(Sl));
        lap("multigrid hierarchy");
    }
    return DNS_OK;
}

int dns_saddle::setup_dist(const dns::HostCsr &Gch, const dns::HostCsr *JGh,
                           bool presliced) {
    using namespace dns;
    const int P = comm->nranks, me = comm->rank;
    if (!dd) dd = new dns_dist_data();
    dd->v0 = st_v[me];
    dd->v1 = st_v[me + 1];
    dd->p0 = st_p[me];
    dd->p1 = st_p[me + 1];
    dd->kmap = {dd->v0, dd->v1 - dd->v0, nv + dd->p0, dd->p1 - dd->p0};
    // halo plans from the (replicated) host patterns: what every rank needs
    // from every other one
    std::vector<std::vector<std::vector<int>>> needK((size_t)P), needU((size_t)P);
    const dns_csr fv = Fh.view(), jv = Jh.view(), gv = Gch.view();
    dns_csr jgv;
    if (JGh) jgv = JGh->view();
    // (a handle created from rows knows its own patterns only)
    const bool own_only = rank_local;
    for (int r = 0; r < P; ++r) {
        std::vector<std::vector<int>> a, b;
        needK[r].assign((size_t)P, std::vector<int>());
        needU[r].assign((size_t)P, std::vector<int>());
        if (own_only && r != me) continue;
        // K rows of rank r: F rows (velocity columns) and J rows
        halo_need(&fv, st_v[r], st_v[r + 1], P, r, st_v.data(), nv, a);
        halo_need(&jv, st_p[r], st_p[r + 1], P, r, st_v.data(), nv, b);
        needK[r].assign((size_t)P, std::vector<int>());
        for (int q = 0; q < P; ++q) {
            std::vector<int> &m = needK[r][q];
            m.resize(a[q].size() + b[q].size());
            std::merge(a[q].begin(), a[q].end(), b[q].begin(), b[q].end(),
                       m.begin());
            m.erase(std::unique(m.begin(), m.end()), m.end());
        }
        // Gc rows (velocity columns only: zp is replicated) and J Fh^-1 rows
        // (partitioned set-up: the rank's own rows only, see below)
        if (presliced && r != me) continue;
        if (presliced) {
            halo_need(&gv, 0, gv.nrows, P, r, st_v.data(), nv, a);
            if (JGh) halo_need(&jgv, 0, jgv.nrows, P, r, st_v.data(), nv, b);
        } else {
            halo_need(&gv, st_v[r], st_v[r + 1], P, r, st_v.data(), nv, a);
            if (JGh)
                halo_need(&jgv, st_p[r], st_p[r + 1], P, r, st_v.data(), nv, b);
        }
        if (!JGh) b.assign((size_t)P, std::vector<int>());
        needU[r].assign((size_t)P, std::vector<int>());
        for (int q = 0; q < P; ++q) {
            std::vector<int> &m = needU[r][q];
            m.resize(a[q].size() + b[q].size());
            std::merge(a[q].begin(), a[q].end(), b[q].begin(), b[q].end(),
                       m.begin());
            m.erase(std::unique(m.begin(), m.end()), m.end());
        }
    }
    if (own_only) {
        const std::vector<std::vector<int>> mine = needK[me];
        DNS_TRY(gather_need_lists(mine, needK));
    }
    DNS_TRY(dd->planK.build(needK, me, P, stream));
    dd->needK = needK;
    if (presliced) {
        // what the others need from this rank: from their own lists
        const std::vector<std::vector<int>> mine = needU[me];
        DNS_TRY(gather_need_lists(mine, needU));
    }
    DNS_TRY(dd->planU.build(needU, me, P, stream));
    // this rank's row blocks replace the full matrices in HBM
    {
        const HostCsr kl = host_k_slice(Fh, JTh, Jh, nv, dd->v0, dd->v1, dd->p0,
                                        dd->p1);
        const dns_csr kv = kl.view();
        DNS_TRY(K.upload(&kv, stream));
        // bandwidth regime: the row block in the pair format (2x2 node
        // blocks), as on one GPU; silently absent when the block does not fit
        Kp.release_all();
        HostPair hp;
        if (pair_knob && streams(K) && !fh_stale &&
            host_pair_from_k(kl, nv, hp, nullptr, dd->v1 - dd->v0, dd->v0,
                             dd->p0))
            DNS_TRY(Kp.upload(hp, stream));
    }
    {
        const HostCsr gl =
            presliced ? HostCsr() : host_row_slice(Gch, dd->v0, dd->v1);
        const dns_csr v = presliced ? Gch.view() : gl.view();
        DNS_TRY(Gc.upload(&v, stream));
        if (fp32_store) DNS_TRY(to_f32(Gc.vals.p, gc32, (size_t)Gc.nnz));
    }
    if (JGh) {
        const HostCsr jl =
            presliced ? HostCsr() : host_row_slice(*JGh, dd->p0, dd->p1);
        const dns_csr v = presliced ? JGh->view() : jl.view();
        DNS_TRY(JG.upload(&v, stream));
        if (fp32_store && streams(JG))
            DNS_TRY(to_f32(JG.vals.p, JG.vals32, (size_t)JG.nnz + 2));
    }
    F.release_all();
    J.release_all();
    JT.release_all();
    if (popts.schur == DNS_SCHUR_DENSE && P > 1) {
        // the dense Schur inverse by COLUMNS: this rank keeps the columns of
        // its pressure block and forms its share of every row of
        // zp = -Sinv tau from its own entries of tau; the shares are
        // all-reduced (NP doubles) -- one collective instead of gathering tau
        // and zp
        const int ncl = dd->p1 - dd->p0;
        if (fp32_store) {
            const int sldc = std::max(4, (ncl + 3) & ~3);
            DevBuf<float> loc;
            DNS_TRY(loc.alloc((size_t)np * sldc));
            DNS_TRY(loc.zero(stream));
            if (ncl > 0)
                DNS_HIP(hipMemcpy2DAsync(loc.p, (size_t)sldc * sizeof(float),
                                         sinv32.p + dd->p0,
                                         (size_t)sld * sizeof(float),
                                         (size_t)ncl * sizeof(float), (size_t)np,
                                         hipMemcpyDeviceToDevice, stream));
            DNS_HIP(hipStreamSynchronize(stream));
            std::swap(loc.p, sinv32.p);
            std::swap(loc.n, sinv32.n);
            dd->schur_ld = sldc;
        } else {
            const int ldc = std::max(1, ncl);
            DevBuf<double> loc;
            DNS_TRY(loc.alloc((size_t)np * ldc));
            DNS_TRY(loc.zero(stream));
            if (ncl > 0)
                DNS_HIP(hipMemcpy2DAsync(loc.p, (size_t)ldc * sizeof(double),
                                         sinv.p + dd->p0,
                                         (size_t)np * sizeof(double),
                                         (size_t)ncl * sizeof(double),
                                         (size_t)np, hipMemcpyDeviceToDevice,
                                         stream));
            DNS_HIP(hipStreamSynchronize(stream));
            std::swap(loc.p, sinv.p);
            std::swap(loc.n, sinv.n);
            dd->schur_ld = ldc;
        }
        dd->schur_cols = true;
    } else {
        dd->schur_cols = false;
    }
    mg_nparts = 0;
    if (popts.schur == DNS_SCHUR_MG && mg_fused && P > 1) {
        if (mg_rows_parts > 0)
            mg_nparts = mg_rows_parts;       // (formed by rows: in place)
        else
            DNS_TRY(setup_dist_mg());
    }
    // (the whole level operators on the host have done their duty: every new
    // set-up builds the hierarchy afresh)
    for (auto &lv : mg)
        lv.Sh = lv.Apreh = lv.Rrh = lv.Qqh = HostCsr();
    if (!lazy_one.p) {
        static const double one_zero[2] = {1.0, 0.0};
        DNS_TRY(lazy_one.alloc(2));
        DNS_TRY(lazy_one.upload(one_zero, 2, stream));
    }
    DNS_HIP(hipStreamSynchronize(stream));
    dist_sliced = true;
    dist_generation++;
    return DNS_OK;
}

// the full matrices back in HBM (before a new set-up: its device parts -- power
// iterations, Schur assembly -- work on whole matrices)
int dns_saddle::restore_full_device() {
    using namespace dns;
    if (!dist_sliced) return DNS_OK;
    if (!rank_local) {
        const dns_csr fv = Fh.view(), jv = Jh.view(), tv = JTh.view();
        DNS_TRY(F.upload(&fv, stream));
        DNS_TRY(J.upload(&jv, stream));
        DNS_TRY(JT.upload(&tv, stream));
        const HostCsr kf = host_k_slice(Fh, JTh, Jh, nv, 0, nv, 0, np);
        const dns_csr kv = kf.view();
        DNS_TRY(K.upload(&kv, stream));
    }
    // (created from rows: there are no whole matrices to bring back -- the
    // set-up works by rows and the row block of K stays until setup_dist
    // replaces it)
    Kp.release_all();                // (the row block's)
    // (row-partitioned multigrid levels stay as they are: both callers leave
    // the preconditioner "not ready", and the next set-up builds the hierarchy
    // afresh)
    for (auto &lv : mg) lv.part = false;
    mg_nparts = 0;
    DNS_HIP(hipStreamSynchronize(stream));
    dist_sliced = false;
    dist_generation++;
    return DNS_OK;
}

// Row-partitioned multigrid levels (fused V(2,2) cycle): every level with at
// least mg_part_min rows keeps the rank's rows of S, Apre, Qq (and the rows of
// Rr that produce the rank's rows of the next level) only; vectors of a level
// stay full length, valid on the own rows and the halo.  Halo plans per level:
// planF = level-l entries the rank's rows of Apre / S / Qq / Rr reference,
// planC = entries of the next level's correction the rank's rows of Qq
// reference (not needed when the next level runs replicated).
int dns_saddle::setup_dist_mg() {
    using namespace dns;
    const int P = comm->nranks, me = comm->rank;
    const int L = (int)mg.size();
    int Lp = 0;
    while (Lp + 1 < L && mg[Lp].n >= mg_part_min && !mg[Lp].Sh.rowptr.empty())
        ++Lp;
    mg_nparts = Lp;
    if (Lp == 0) return DNS_OK;
    for (int l = 0; l <= Lp; ++l)
        mg[l].st = (l == 0) ? st_p : partition_starts(mg[l].n, P);
    for (int l = 0; l < Lp; ++l) {
        MgLevel &lv = mg[l];
        const std::vector<int> &st = lv.st, &stc = mg[l + 1].st;
        lv.coarse_replicated = (l + 1 == Lp);
        std::vector<std::vector<std::vector<int>>> needF((size_t)P),
            needC((size_t)P);
        for (int r = 0; r < P; ++r)
            mg_need_lists(lv.Sh, lv.Apreh, lv.Qqh, st[r], st[r + 1], lv.Rrh,
                          stc[r], stc[r + 1], st, stc, r, lv.coarse_replicated,
                          needF[r], needC[r]);
        DNS_TRY(lv.planF.build(needF, me, P, stream));
        DNS_TRY(lv.planC.build(needC, me, P, stream));
        // (row blocks that are streamed cross the HBM as fp32, like the whole
        // operators on one GPU)
        const HostCsr a = host_row_slice(lv.Sh, st[me], st[me + 1]);
        const HostCsr b = host_row_slice(lv.Apreh, st[me], st[me + 1]);
        const HostCsr c = host_row_slice(lv.Rrh, stc[me], stc[me + 1]);
        const HostCsr d = host_row_slice(lv.Qqh, st[me], st[me + 1]);
        DNS_TRY(upload_mg_ops(lv, &a, &b, &c, &d, false));
        lv.part = true;
    }
    DNS_HIP(hipStreamSynchronize(stream));
    return DNS_OK;
}

// zp = -MG(in) with the first mg_nparts levels row-partitioned.  `in` is valid
// on the rank's own pressure rows; zp comes back complete (all-gathered) on
// every rank.
int dns_saddle::schur_mg_apply_dist(const double *in, double *zp,
                                    const int *guard) {
    using namespace dns;
    const int L = (int)mg.size(), Lp = mg_nparts, me = comm->rank;
    auto op = [&](const CsrDev &A, const double *xa, int nsplit,
                  const double *xb, const MgLevel *add, const double *b,
                  double *out, int row0) -> int {
        if (A.nrows == 0) return DNS_OK;
        if (streams_mg(A)) {
            // bandwidth regime: the row block through the streaming kernel
            StreamEpi ep = stream_epi_plain(1.0, 0.0, nullptr);
            ep.x2 = xb;
            ep.nsplit = nsplit;
            if (add) {
                ep.dinv = add->dinv.p;
                ep.b = b;
                ep.omega = add->omega;
                ep.add_cb = 1;
            }
            ep.map_on = 1;
            ep.rm = RowMap{row0, A.nrows, 0, 0};
            if (A.vals32.p)
                return launch_stream16x<float>(A, A.vals32.p, xa, out, ep,
                                               stream, guard);
            return launch_stream16x<double>(A, A.vals.p, xa, out, ep, stream,
                                            guard);
        }
        DNS_LPR_SWITCH(
            A.lpr,
            hipLaunchKernelGGL(k_mg_split<L>, grid_for_rows(A.nrows, A.lpr),
                               kBlock, 0, stream, A.nrows, A.rowptr.p,
                               A.colidx.p, A.vals.p, xa, nsplit, xb,
                               add ? add->dinv.p : (const double *)nullptr, b,
                               add ? add->omega : 0.0, out, guard, row0));
        DNS_HIP(hipGetLastError());
        return DNS_OK;
    };
    // the last post-sweep of a level, out = osc (x2 + omega2 dinv (b - S x2))
    // for the rows [r0, r0 + nrows) the CSR arrays of S hold
    auto sweep = [&](MgLevel &lv, int nrows, int r0, const double *b,
                     double *out, double osc) -> int {
        if (streams_mg(lv.S)) {
            StreamEpi ep = stream_epi_plain(osc, 0.0, b);
            ep.dinv = lv.dinv.p;
            ep.xin = lv.x2.p;
            ep.omega = lv.omega2;
            ep.map_on = 1;
            ep.rm = RowMap{r0, nrows, 0, 0};
            if (lv.S.vals32.p)
                return launch_stream16x<float>(lv.S, lv.S.vals32.p, lv.x2.p,
                                               out, ep, stream, guard);
            return launch_stream16x<double>(lv.S, lv.S.vals.p, lv.x2.p, out,
                                            ep, stream, guard);
        }
        DNS_LPR_SWITCH(
            lv.S.lpr,
            hipLaunchKernelGGL(k_mg_sweep<L>, grid_for_rows(nrows, lv.S.lpr),
                               kBlock, 0, stream, nrows, lv.S.rowptr.p,
                               lv.S.colidx.p, lv.S.vals.p, lv.dinv.p, lv.omega2,
                               b, lv.x2.p, out, guard, osc, (double *)nullptr,
                               r0));
        DNS_HIP(hipGetLastError());
        return DNS_OK;
    };
    // level 0 works on a copy of `in` (the exchange writes halo entries)
    {
        const int a = mg[0].st[me], b = mg[0].st[me + 1];
        if (b > a)
            DNS_HIP(hipMemcpyAsync(mg[0].b.p + a, in + a,
                                   (size_t)(b - a) * sizeof(double),
                                   hipMemcpyDeviceToDevice, stream));
    }
    for (int l = 0; l < Lp; ++l) {
        MgLevel &lv = mg[l];
        double *b = lv.b.p;
        DNS_TRY(lv.planF.exchange(comm, b, stream));
        DNS_TRY(op(lv.Apre, b, lv.n, nullptr, nullptr, nullptr, lv.x.p,
                   lv.st[me]));
        DNS_TRY(lv.planF.exchange(comm, lv.x.p, stream));
        DNS_TRY(op(lv.Rr, b, lv.n, lv.x.p, nullptr, nullptr, mg[l + 1].b.p,
                   mg[l + 1].st[me]));
        if (lv.coarse_replicated)
            DNS_TRY(comm->allgatherv(mg[l + 1].b.p, mg[l + 1].st, stream));
    }
    // replicated levels Lp .. L-1 (every rank runs them in full)
    for (int l = Lp; l + 1 < L; ++l) {
        MgLevel &lv = mg[l];
        DNS_TRY(mg_op(lv.Apre, lv.b.p, lv.n, nullptr, nullptr, nullptr, lv.x.p,
                      guard));
        DNS_TRY(mg_op(lv.Rr, lv.b.p, lv.n, lv.x.p, nullptr, nullptr,
                      mg[l + 1].b.p, guard));
    }
    {
        MgLevel &lc = mg[L - 1];
        DNS_TRY(mg_coarse_apply(lc.b.p, lc.x.p, guard));
    }
    for (int l = L - 2; l >= Lp; --l) {
        MgLevel &lv = mg[l];
        DNS_TRY(mg_op(lv.Qq, lv.x.p, lv.n, mg[l + 1].x.p, &lv, lv.b.p, lv.x2.p,
                      guard));
        DNS_TRY(sweep(lv, lv.n, 0, lv.b.p, lv.x.p, 1.0));
    }
    for (int l = Lp - 1; l >= 0; --l) {
        MgLevel &lv = mg[l];
        const int r0 = lv.st[me], nloc = lv.st[me + 1] - lv.st[me];
        if (!lv.coarse_replicated)
            DNS_TRY(lv.planC.exchange(comm, mg[l + 1].x.p, stream));
        DNS_TRY(op(lv.Qq, lv.x.p, lv.n, mg[l + 1].x.p, &lv, lv.b.p, lv.x2.p,
                   r0));
        DNS_TRY(lv.planF.exchange(comm, lv.x2.p, stream));
        double *out = (l == 0) ? zp : lv.x.p;
        if (nloc > 0)
            DNS_TRY(sweep(lv, nloc, r0, lv.b.p, out, (l == 0) ? -1.0 : 1.0));
    }
    DNS_HIP(hipGetLastError());
    // every rank needs all of zp (Gc and K read it along their rows)
    DNS_TRY(comm->allgatherv(zp, st_p, stream));
    return DNS_OK;
}

int dns_saddle::all_ranks_any(bool mine, bool *any) {
    *any = mine;
    if (!dist()) return DNS_OK;
    double v = mine ? 1.0 : 0.0;
    DNS_TRY(allreduce_host(&v, 1));
    *any = v > 0.5;
    return DNS_OK;
}

int dns_saddle::allreduce_host(double *v, int count) {
    if (scal.n < 1) DNS_TRY(scal.alloc(16));
    DNS_TRY(scal.upload(v, (size_t)count, stream));   // (fails past scal.n)
    DNS_TRY(comm->allreduce(scal.p, count, stream));
    return scal.download(v, (size_t)count, stream);
}

int dns_saddle::agree(int rc_local, const char *where) {
    if (!comm || comm->nranks < 2) return rc_local;
    const std::string kept = dns::g_last_error;     // (the local message)
    double v = rc_local != DNS_OK ? 1.0 : 0.0;
    DNS_TRY(allreduce_host(&v, 1));
    if (rc_local != DNS_OK) {
        dns::g_last_error = kept;
        return rc_local;
    }
    if (v > 0.5)
        return dns::fail(DNS_ERR_COMM, "%s: failed on another rank", where);
    return DNS_OK;
}

int dns_saddle::dist_v0() const { return dd ? dd->v0 : 0; }
int dns_saddle::dist_v1() const { return dd ? dd->v1 : nv; }

// new values of F (same pattern) while the matrices are sliced
int dns_saddle::update_values_dist() {
    using namespace dns;
    const HostCsr kl = host_k_slice(Fh, JTh, Jh, nv, dd->v0, dd->v1, dd->p0,
                                    dd->p1);
    DNS_TRY(K.vals.upload(kl.vals.data(), kl.vals.size(), stream));
    DNS_HIP(hipStreamSynchronize(stream));
    Kp.release_all();                // copies of the values: next set-up
    return DNS_OK;
}

// the plan of a row-partitioned cycle: this rank's row blocks, and every
// reduction read as ONE all-reduced sum from `dsum`
// (lazy: "norms" 1 and 0 -- the head copies r, scales nothing, stops never)
CyclePlan dns_saddle::plan_cycle_dist(const dns_solve_opts *o, int first,
                                      const dns::StepHooks &hk,
                                      bool lazy) const {
    using namespace dns;
    const dns_dist_data *D = dd;
    CyclePlan P;
    P.v0 = D->v0, P.v1 = D->v1, P.p0 = D->p0, P.p1 = D->p1;
    P.q1 = np;
    P.map_on = 1;
    P.kmap = D->kmap;
    P.schur = schur_block();
    if (D->schur_cols) {
        // dense Schur inverse by columns: every rank forms its share of all NP
        // rows from its own entries of tau; the shares are all-reduced behind
        if (P.schur.kind == 1 || P.schur.kind == 2)
            P.schur.stride = D->schur_ld;
        P.schur.col0 = P.p0;
        P.schur.ncols = P.p1 - P.p0;
        P.schur.add_corr = comm->rank == 0 ? 1 : 0;
    }
    P.dense = popts.schur == DNS_SCHUR_DENSE;
    P.mgs = popts.schur == DNS_SCHUR_MG;
    // fused Gram-Schmidt (norm by Pythagoras: ONE all-reduce per step) unless
    // the caller asks for the explicit form or a cycle of this solve has
    // tripped the cancellation guard; the explicit form orthogonalises the
    // own rows and takes the norm with a second all-reduce
    P.fusedgs = o->reorth == 2;
    // bandwidth regime: the row blocks go through the streaming kernels too
    // (local CSR rows -> global rows through the RowMap of the epilogue)
    P.stream_k = P.stream_dots = streams(K);
    P.multidot_ww = 1;
    P.first = first;
    P.stepctr = first == 1 ? hk.stepctr : nullptr;
    P.rtol = o->rtol;
    P.atol = o->atol;
    P.maxiter = o->maxiter;
    P.gridA = head_grid();
    const int nloc = (P.v1 - P.v0) + (P.p1 - P.p0);
    P.gridKc = P.gridR =
        std::max(1, std::min(grid_for_rows(nloc, K.lpr), 2048));
    P.gridK = P.stream_k ? (Kp.ready ? pair_grid(Kp, sgrid)
                                     : stream_grid(K, sgrid))
                         : P.gridKc;
    P.rr_part = lazy ? lazy_one.p : dsum.p;
    P.bb_part = P.rr_part + 1;
    P.rr_np = P.bb_np = 1;
    P.hpart = dsum.p + 2;
    P.hsummed = true;
    P.npart = dsum.p + kMaxRestart + 4;
    P.nnp = 1;
    P.w = w.p;
    P.ld = ld;
    return P;
}

// zv (own rows) = Gc_loc [V_j,v ; zp]
int dns_saddle::node_fhat_dist(const CyclePlan &P, int j) {
    using namespace dns;
    const double *vj = V.p + (size_t)j * ld;
    double *zj = Z.p + (size_t)j * ld, *zp = zj + nv;
    if (P.stream_k && streams(Gc)) {
        StreamEpi ep = stream_epi_plain(1.0, 0.0, nullptr);
        ep.x2 = zp;
        ep.nsplit = nv;
        ep.map_on = 1;
        ep.rm = RowMap{P.v0, P.v1 - P.v0, 0, 0};
        if (fp32_store)
            return launch_stream16x<float>(Gc, gc32.p, vj, zj, ep, stream,
                                           done_ptr());
        return launch_stream16x<double>(Gc, Gc.vals.p, vj, zj, ep, stream,
                                        done_ptr());
    }
    const int *g_rp = Gc.rowptr.p - P.v0;    // row pointers by GLOBAL row
    const int g = grid_for_rows(P.v1 - P.v0, Gc.lpr);
    if (fp32_store) {
        DNS_LPR_SWITCH(
            Gc.lpr,
            hipLaunchKernelGGL((k_spmv_split<L, float>), g, kBlock, 0, stream,
                               nv, g_rp, Gc.colidx.p, gc32.p, vj, (size_t)0,
                               zero_ptr(), zp, zj, done_ptr(),
                               (double *)nullptr, P.v0, P.v1));
    } else {
        DNS_LPR_SWITCH(
            Gc.lpr,
            hipLaunchKernelGGL((k_spmv_split<L, double>), g, kBlock, 0, stream,
                               nv, g_rp, Gc.colidx.p, Gc.vals.p, vj, (size_t)0,
                               zero_ptr(), zp, zj, done_ptr(),
                               (double *)nullptr, P.v0, P.v1));
    }
    return DNS_OK;
}

// One restart cycle of the row-partitioned solve: the nodes of enqueue_cycle
// on this rank's rows, with the halo exchanges, the gathers and the all-reduced
// scalar sums between them
int dns_saddle::enqueue_cycle_dist(const double *b, double *x, int c,
                                   const dns_solve_opts *o, int first,
                                   bool have_resid, const dns::StepHooks &hk) {
    using namespace dns;
    dns_dist_data *D = dd;
    // one-step cycle (what a pipelined time step predicts once the warm start
    // is good): the first vector stays un-normalised and the norms of r and b
    // travel with the step's dots -- ONE all-reduce of scalars per time step
    // instead of two (k_arn_tail_lazy1)
    const bool lazy = dist_lazy1 && o->reorth == 2 && c == 1 && first == 1 &&
                      o->atol < 1.0 && o->maxiter > 0;
    const CyclePlan P = plan_cycle_dist(o, first, hk, lazy);
    const bool fused = P.fusedgs, scols = D->schur_cols;
    double *const hsum = P.hpart, *const dnorm = P.npart;
    // x is valid on the own entries AND on the halo the rows of K_loc
    // reference when a cycle starts: a caller's start vector is whole (solve,
    // trapezoidal stepper) or a combination of earlier solutions that are
    // (IMEX stepper), and the tail of a cycle updates the halo entries with the
    // same y_j and the exchanged Z_j the owner uses -- no exchange here
    // ("dist_x0_exchange" = 1 brings it back)
    if (dist_x0_exchange) DNS_TRY(D->planK.exchange(comm, x, stream));
    // the preconditioned vectors are exchanged over the caller's halo when it
    // has a wider one (IMEX stepper: rows of R1 and convection cells as well),
    // so that the new iterate needs no exchange of its own behind the solve
    const dns_halo_plan *zplan = hk.z_plan ? hk.z_plan : &D->planK;
    // (have_resid: the caller's prologue kernel has left r = b - K x and the
    // partials of both norms -- resid_nparts of them -- behind)
    const bool pre_r = have_resid && hk.resid_nparts > 0;
    const int gR = pre_r ? hk.resid_nparts : P.gridK;   // partials of ||r||, ||b||
    if (!pre_r) DNS_TRY(node_residual(P, b, x));
    if (lazy) {
        if (!lazy_one.p)
            return fail(DNS_ERR_NOT_READY, "lazy cycle without its constants");
    } else {
        hipLaunchKernelGGL(k_sum_partials2, 2, kBlock, 0, stream, partR.p,
                           partB.p, gR, P.rr_part);
        DNS_TRY(comm->allreduce(P.rr_part, 2, stream));
    }
    for (int j = 0; j < c; ++j) {
        double *zj = Z.p + (size_t)j * ld;
        double *zp = zj + nv;
        double *src = (j == 0) ? r.p : w.p;
        // velocity halo of the new (un-normalised) basis vector
        DNS_TRY(D->planU.exchange(comm, src, stream));
        const double *tin = nullptr;
        if (have_jg && !P.mgs) {
            DNS_TRY(node_tau(src, hsum, 1, fused ? j : (j > 0 ? -1 : 0), P.p0,
                             P.p1));
            // (column form of the dense inverse: own entries of tau suffice)
            if (!scols) DNS_TRY(comm->allgatherv(tau.p, st_p, stream));
            tin = tau.p;
        } else if (!scols && !have_jg) {
            // the Schur block reads the pressure part itself
            DNS_TRY(comm->allgatherv(src + nv, st_p, stream));
        }
        DNS_TRY(node_head(P, j, src, zp, tin));
        if (scols) DNS_TRY(comm->allreduce(zp, np, stream));
        // (replicated or partitioned V-cycle on tau(V_j) / V_j,p)
        if (P.mgs) DNS_TRY(node_schur_mg(P, j));
        DNS_TRY(node_fhat_dist(P, j));
        DNS_TRY(const_cast<dns_halo_plan *>(zplan)->exchange(comm, zj, stream));
        // w (own rows) = K_loc z and the step's dots over the own rows
        DNS_TRY(node_k_apply(P, j, zj));
        if (lazy) {
            hipLaunchKernelGGL(k_sum_lazy4, 1, kBlock, 0, stream, partA.p,
                               P.kparts(j), partR.p, partB.p, gR, hsum);
            DNS_TRY(comm->allreduce(hsum, 4, stream));
        } else {
            hipLaunchKernelGGL(k_sum_partials_n, 1, kBlock, 0, stream, partA.p,
                               P.kparts(j), j + 2, hsum);
            DNS_TRY(comm->allreduce(hsum, fused ? j + 2 : j + 1, stream));
        }
        if (!fused) {
            // explicit Gram-Schmidt on the own rows, norm by a second
            // all-reduce
            hipLaunchKernelGGL(k_orth<0>, gridD, kBlock, 0, stream, n, V.p, ld,
                               w.p, hsum, 1, j, 0, partN.p, gridD, ctl.p,
                               D->kmap);
            hipLaunchKernelGGL(k_sum_partials, 1, kBlock, 0, stream, partN.p,
                               gridD, dnorm);
            DNS_TRY(comm->allreduce(dnorm, 1, stream));
        }
    }
    if (lazy) {
        const bool cells = hk.dist_tail.on && hk.dist_tail.cells.nblocks > 0;
        hipLaunchKernelGGL(k_arn_tail_lazy1,
                           gridD + (cells ? hk.dist_tail.cells.nblocks : 0), kBlock,
                           0, stream, n, hsum, ctl.p, histdev.p, (int)hist_cap,
                           o->maxiter, o->rtol, o->atol, Z.p, x, hk.tail_extrap,
                           r.p, w.p, hk.carry_rnew, nv, gridD,
                           cells ? hk.dist_tail.x0copy : (const double *)nullptr,
                           cells ? hk.dist_tail.cells : TailCells{});
        if (cells) hk.dist_tail_ran = true;
    } else {
        DNS_TRY(node_tail(P, c, x, hk));
    }
    // (residual carry-over: only the one-step cycle knows the true residual
    // behind it; a solve that ends with a general cycle carries none)
    if (!lazy && hk.carry_rnew)
        DNS_HIP(hipMemsetAsync(hk.carry_rnew, 0, (size_t)nv * sizeof(double),
                               stream));
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}

extern "C" {

int dns_comm_set_alltoallv_cb(dns_comm *c, dns_alltoallv_cb cb) try {
    if (!c) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    c->a2a_cb = cb;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_comm_stats2(dns_comm *c, int64_t *out5) try {
    if (!c || !out5) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    out5[0] = c->n_allreduce;
    out5[1] = c->n_allgather;
    out5[2] = c->n_alltoall;
    out5[3] = c->bytes_alltoall;
    out5[4] = c->bytes_allgather;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_comm_set_timing(dns_comm *c, int on) try {
    if (!c) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_HIP(hipSetDevice(c->device));
    DNS_TRY(c->timing_collect());
    c->timing = on != 0;
    if (on)
        for (int k = 0; k < dns_comm::kKinds; ++k) {
            c->timed_ms[k] = 0.0;
            c->timed_calls[k] = 0;
        }
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_comm_timing(dns_comm *c, double *ms3, int64_t *calls3) try {
    if (!c || !ms3 || !calls3)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    DNS_HIP(hipSetDevice(c->device));
    DNS_TRY(c->timing_collect());
    for (int k = 0; k < dns_comm::kKinds; ++k) {
        ms3[k] = c->timed_ms[k];
        calls3[k] = c->timed_calls[k];
    }
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_halo_lists(const dns_csr *a, int32_t row0, int32_t row1,
                   int32_t nranks, int32_t rank, const int32_t *col_starts,
                   int32_t ncols_part, int32_t *counts, int32_t *lists,
                   int64_t cap, int64_t *total) try {
    DNS_TRY(dns::check_csr(a, "A"));
    if (!col_starts || !counts || !total || nranks < 1 || rank < 0 ||
        rank >= nranks || row0 < 0 || row1 > a->nrows || row0 > row1 ||
        ncols_part > a->ncols || col_starts[nranks] != ncols_part)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "bad argument");
    std::vector<std::vector<int>> need;
    dns::halo_need(a, row0, row1, nranks, rank, col_starts, ncols_part, need);
    int64_t pos = 0;
    for (int q = 0; q < nranks; ++q) {
        counts[q] = (int32_t)need[q].size();
        for (int c : need[q]) {
            if (lists && pos < cap) lists[pos] = c;
            ++pos;
        }
    }
    *total = pos;
    return DNS_OK;
} DNS_CAPI_CATCH

int dns_saddle_device_bytes(dns_saddle *h, int64_t *matrix_bytes) try {
    if (!h || !matrix_bytes)
        return dns::fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    auto csr = [](const dns::CsrDev &A) -> int64_t {
        return (int64_t)(A.rowptr.n * 4 + A.colidx.n * 4 + A.vals.n * 8 +
                         A.c16.n * 2 + A.c16base.n * 4 +
                         (A.rowblocks_t[0].n + A.rowblocks_t[1].n +
                          A.rowblocks_t[2].n) * 4);
    };
    int64_t b = csr(h->F) + csr(h->J) + csr(h->JT) + csr(h->K) + csr(h->Gc) +
                csr(h->JG);
    b += (int64_t)h->gc32.n * 4 + (int64_t)h->sinv.n * 8 +
         (int64_t)h->sinv32.n * 4;
    for (const auto &lv : h->mg)
        b += csr(lv.S) + csr(lv.P) + csr(lv.PT) + csr(lv.Apre) + csr(lv.Rr) +
             csr(lv.Qq);
    b += (int64_t)(h->mg_cinv.p ? h->mg_cinv.n : 0) * 8 +
         (int64_t)(h->mg_cinv32.p ? h->mg_cinv32.n : 0) * 4 +
         (int64_t)(h->mg_cinv16.p ? h->mg_cinv16.n : 0) * 2;
    *matrix_bytes = b;
    return DNS_OK;
} DNS_CAPI_CATCH

}  // extern "C"
