// The nodes of one restart cycle of right-preconditioned GMRES, one launcher
// each, and the plan they share (solver.hpp, CyclePlan).  enqueue_cycle (one
// GPU), enqueue_cycle_dist (row-partitioned) and dns_saddle_probe put them in
// sequence; a node that the two cycles launch with more than other values of
// the plan has a form of its own beside the partitioned cycle (dist_solve.inc).
// Every node only enqueues on `stream`: nothing here synchronises or allocates.

// workgroups of the head (dense Schur rows: one wave each, four per workgroup)
int dns_saddle::head_grid() const {
    return popts.schur == DNS_SCHUR_DENSE
               ? std::max(gridD, std::min((np + 3) / 4, 2048))
               : gridD;
}

// (one GPU; the partitioned plan sets the stride and the columns it holds)
SchurBlock dns_saddle::schur_block() const {
    SchurBlock S;
    if (popts.schur == DNS_SCHUR_MG) {
        S.kind = 3;
    } else if (popts.schur == DNS_SCHUR_DENSE && fp32_store) {
        S.kind = 2;
        S.inv = sinv32.p;
        S.stride = sld;
    } else {
        // (Jacobi: sinv is the DIAGONAL, np entries)
        S.kind = popts.schur == DNS_SCHUR_DENSE ? 1 : 0;
        S.inv = sinv.p;
    }
    return S;
}

CyclePlan dns_saddle::plan_cycle(int c, const dns_solve_opts *o, int first,
                                 bool have_resid, const StepHooks &hk) const {
    CyclePlan P;
    P.schur = schur_block();
    P.dense = popts.schur == DNS_SCHUR_DENSE;
    P.mgs = popts.schur == DNS_SCHUR_MG;
    P.stream_k = streams(K);
    P.fusedgs = o->reorth == 2 && (fuse_dots || P.stream_k);
    P.stream_dots = P.stream_k && P.fusedgs;
    P.multidot = fuse_dots || P.fusedgs;
    P.multidot_ww = P.fusedgs ? 1 : 0;
    P.first = first;
    P.stepctr = first == 1 ? hk.stepctr : nullptr;
    P.rtol = o->rtol;
    P.atol = o->atol;
    P.maxiter = o->maxiter;
    P.gridA = head_grid();
    P.gridKc = gridC;
    P.gridK = P.stream_k ? (Kp.ready ? pair_grid(Kp, sgrid)
                                     : stream_grid(K, sgrid))
                         : gridC;
    P.gridR = gridS;
    // (the caller's prologue kernel may have produced r and the partials)
    P.rr_part = partR.p;
    P.bb_part = partB.p;
    P.rr_np = (have_resid && hk.resid_nparts > 0)
                  ? hk.resid_nparts
                  : ((!have_resid && P.stream_k) ? P.gridK : gridS);
    P.bb_np = P.rr_np;
    P.hpart = partA.p;
    P.npart = partN.p;
    P.nnp = gridD;
    P.q1 = P.p1 = np;
    P.v1 = nv;
    P.kmap = RowMap{0, n, 0, 0};
    P.s6 = hk.step6.on && P.fusedgs && !P.stream_k && have_resid &&
           Wcols.n >= (size_t)c * ld;
    P.t6 = hk.step6.t6;
    P.t6.r0 = r.p;
    P.t6.W = Wcols.p;
    P.t6.nv = nv;
    P.w = w.p;
    P.wcols = Wcols.p;
    P.ld = ld;
    return P;
}

// r = b - K x by CSR rows (`rm`: the rows the arrays of K hold), `grid`
// partials of ||r||^2 in partR and (part_bb != null) of ||b||^2
int dns_saddle::resid_norm_csr(int grid, const double *x, const double *b,
                               double *part_bb, const RowMap &rm) {
    DNS_LPR_SWITCH(K.lpr,
                   hipLaunchKernelGGL(k_resid_norm<L>, grid, kBlock, 0, stream,
                                      n, K.rowptr.p, K.colidx.p, K.vals.p, x,
                                      b, r.p, partR.p, part_bb, rm));
    return DNS_OK;
}

// r = b - K x, ||r||^2, ||b||^2
int dns_saddle::node_residual(const CyclePlan &P, const double *b,
                              const double *x) {
    if (!P.stream_k) return resid_norm_csr(P.gridR, x, b, partB.p, P.kmap);
    // bandwidth regime: at the streaming rate with the partials of both norms
    // from the same launch
    StreamEpi ep = stream_epi_plain(-1.0, 1.0, b);
    ep.part = partR.p;
    ep.nvec = 0;
    ep.with_ww = 1;
    ep.nparts = P.gridK;
    ep.part_bb = partB.p;
    ep.map_on = P.map_on;
    if (P.map_on) ep.rm = P.kmap;
    if (Kp.ready) return launch_pair16x(Kp, x, r.p, ep, stream, nullptr, sgrid);
    return launch_stream16x<double>(K, K.vals.p, x, r.p, ep, stream, nullptr,
                                    sgrid);
}

// full block factorisation: tau = src_p - (J Fh^-1) src_v, rows [p0, p1), feeds
// the Schur block instead of src_p (`jt`, `part`: the guard of k_tau_guard)
int dns_saddle::node_tau(const double *src, const double *part, int nparts,
                         int jt, int p0, int p1) {
    const int *rp = JG.rowptr.p - p0;        // row pointers by GLOBAL row
    DNS_LPR_SWITCH(
        JG.lpr,
        hipLaunchKernelGGL(k_tau_guard<L>,
                           grid_for_rows(p1 - p0, JG.lpr == 64 ? 128 : JG.lpr),
                           kBlock, 0, stream, np, nv, rp, JG.colidx.p,
                           JG.vals.p, src, tau.p, part, nparts, jt, ctl.p, p0,
                           p1));
    return DNS_OK;
}

// six-node step: r = b - kx with its norms and tau(r) in ONE launch
int dns_saddle::node_tau_first(const double *b, const double *kx) {
    const int gt = std::max(1, std::min((np + 1) / 2, 4096));
    hipLaunchKernelGGL(k_tau_first, gt + gridD, kBlock, 0, stream, gt, n, np,
                       nv, JG.rowptr.p, JG.colidx.p, JG.vals.p, b, kx, tau.p,
                       r.p, partR.p, partB.p);
    return DNS_OK;
}

template <typename F>
static inline void with_schur_kind(int kind, F &&f) {
    switch (kind) {
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 1: f(std::integral_constant<int, 1>{}); break;
        default: f(std::integral_constant<int, 0>{}); break;
    }
}

// head of column j: closes column j - 1, normalises `src` (r, or K z_{j-1})
// into V_j -- with the Gram-Schmidt update when it is fused -- and applies the
// Schur block to its pressure part (or `tin`), zp_j
int dns_saddle::node_head(const CyclePlan &P, int j, const double *src,
                          double *zp, const double *tin) {
    const SchurBlock &S = P.schur;
    with_schur_kind(S.kind, [&](auto sk) {
        constexpr int SK = decltype(sk)::value;
        if (P.fusedgs && j > 0)
            hipLaunchKernelGGL(k_arn_head_f<SK>, P.gridA, kBlock, 0, stream, n,
                               nv, np, j, src, P.hpart, P.hparts(j - 1), V.p,
                               ld, Z.p, S.inv, ctl.p, P.maxiter, tin, P.q0,
                               P.q1, S.stride, S.col0, S.ncols, S.add_corr);
        else
            hipLaunchKernelGGL(k_arn_head<SK>, P.gridA, kBlock, 0, stream, n,
                               nv, np, j, src, j == 0 ? P.rr_part : P.npart,
                               j == 0 ? P.rr_np : P.nnp, V.p, ld, S.inv, zp,
                               ctl.p, P.rtol, P.atol, P.bb_part, P.bb_np,
                               P.maxiter, P.q0, P.q1, j == 0 ? P.first : 0,
                               tin, j == 0 ? P.stepctr : nullptr, S.stride,
                               S.col0, S.ncols);
    });
    return DNS_OK;
}

// Schur block = V-cycle on V_j,p, or on tau of the NORMALISED vector (own
// rows; a replicated cycle of the partitioned solve gathers them)
int dns_saddle::node_schur_mg(const CyclePlan &P, int j) {
    const double *vj = V.p + (size_t)j * ld;
    double *zp = Z.p + (size_t)j * ld + nv;
    const double *sin = vj + nv;
    if (have_jg) {
        if (streams(JG)) {
            // tau = V_j,p - JG V_j,v through the streaming kernel
            StreamEpi ep = stream_epi_plain(-1.0, 1.0, vj + nv);
            ep.map_on = P.map_on;
            if (P.map_on) ep.rm = RowMap{P.p0, P.p1 - P.p0, 0, 0};
            if (JG.vals32.p)
                DNS_TRY(launch_stream16x<float>(JG, JG.vals32.p, vj, tau.p, ep,
                                                stream, done_ptr()));
            else if (P.map_on)
                DNS_TRY(launch_stream16x<double>(JG, JG.vals.p, vj, tau.p, ep,
                                                 stream, done_ptr()));
            else
                DNS_TRY(launch_spmv(JG, vj, tau.p, -1.0, 1.0, vj + nv,
                                    DNS_SPMV_STREAM16, stream, done_ptr()));
        } else {
            DNS_TRY(node_tau(vj, nullptr, 0, -1, P.p0, P.p1));
        }
        // (a partitioned cycle starts from the own rows of tau)
        if (P.map_on && mg_nparts == 0)
            DNS_TRY(comm->allgatherv(tau.p, st_p, stream));
        sin = tau.p;
    }
    if (P.map_on && mg_nparts > 0)
        return schur_mg_apply_dist(sin, zp, done_ptr());
    return schur_mg_apply(sin, zp, nullptr, done_ptr());
}

// w_j (own rows) = K z_j with the step's dots <V_i, w>, i <= j (and <w, w>
// where the Gram-Schmidt update is fused)
int dns_saddle::node_k_apply(const CyclePlan &P, int j, const double *zj) {
    if (P.stream_dots && j + 1 <= kStreamDots) {
        StreamEpi ep = stream_epi_plain(1.0, 0.0, nullptr);
        ep.V = V.p;
        ep.ld = ld;
        ep.nvec = j + 1;
        ep.with_ww = 1;
        ep.part = partA.p;
        ep.nparts = P.gridK;
        ep.map_on = P.map_on;
        if (P.map_on) ep.rm = P.kmap;
        if (Kp.ready)
            return launch_pair16x(Kp, zj, w.p, ep, stream, done_ptr(), sgrid);
        return launch_stream16x<double>(K, K.vals.p, zj, w.p, ep, stream,
                                        done_ptr(), sgrid);
    }
    if (P.multidot) {
        DNS_LPR_SWITCH(
            K.lpr,
            hipLaunchKernelGGL(k_spmv_multidot<L>, P.gridKc, kBlock, 0, stream,
                               n, K.rowptr.p, K.colidx.p, K.vals.p, zj,
                               P.wcol(j), V.p, ld, j, partA.p, P.gridKc, ctl.p,
                               P.kmap, P.multidot_ww));
        return DNS_OK;
    }
    if (K.c16.p) {
        // bandwidth regime: the LDS-streaming kernel with 16-bit column
        // offsets (the roofline kernel of bench.py)
        DNS_TRY(launch_spmv(K, zj, w.p, 1.0, 0.0, nullptr, DNS_SPMV_STREAM16,
                            stream, done_ptr()));
    } else {
        DNS_LPR_SWITCH(
            K.lpr,
            hipLaunchKernelGGL(k_spmv_guard<L>, grid_for_rows(n, K.lpr), kBlock,
                               0, stream, n, K.rowptr.p, K.colidx.p, K.vals.p,
                               zj, w.p, ctl.p, 0, n));
    }
    hipLaunchKernelGGL(k_multidot, gridC, kBlock, 0, stream, n, V.p, ld, w.p,
                       partA.p, gridC, j, ctl.p);
    return DNS_OK;
}

// explicit Gram-Schmidt of w against V_0 .. V_j (one GPU; reorth == 1: twice)
int dns_saddle::node_orth(const CyclePlan &P, int j, int reorth) {
    if (reorth == 1) {
        hipLaunchKernelGGL(k_orth<1>, gridD, kBlock, 0, stream, n, V.p, ld, w.p,
                           P.hpart, P.gridKc, j, 0, partE.p, gridD, ctl.p);
        hipLaunchKernelGGL(k_orth<0>, gridD, kBlock, 0, stream, n, V.p, ld, w.p,
                           partE.p, gridD, j, 1, partN.p, gridD, ctl.p);
    } else {
        hipLaunchKernelGGL(k_orth<0>, gridD, kBlock, 0, stream, n, V.p, ld, w.p,
                           P.hpart, P.gridKc, j, 0, partN.p, gridD, ctl.p);
    }
    return DNS_OK;
}

// closes column c - 1 and takes the correction x += Z y
int dns_saddle::node_tail(const CyclePlan &P, int c, double *x,
                          const StepHooks &hk) {
    if (P.s6) {
        // six-node step: out-of-place tail + new residual + convection cells
        hipLaunchKernelGGL(k_arn_tail6<false>, gridD + hk.step6.cells.nblocks,
                           kBlock, 0, stream, c, n, gridD, P.hpart,
                           P.hparts(c - 1), ctl.p, histdev.p, (int)hist_cap,
                           P.maxiter, Z.p, ld, P.t6, hk.tail_extrap,
                           hk.step6.cells, TailLazy{});
    } else if (P.fusedgs) {
        // fused Gram-Schmidt: tail and correction in ONE launch
        hipLaunchKernelGGL(k_arn_tail_acc, gridD, kBlock, 0, stream, c, n,
                           P.hpart, P.hparts(c - 1), ctl.p, histdev.p,
                           (int)hist_cap, P.maxiter, Z.p, ld, x,
                           hk.tail_extrap);
    } else {
        hipLaunchKernelGGL(k_arn_tail, 1, kBlock, 0, stream, c, P.npart, P.nnp,
                           ctl.p, histdev.p, (int)hist_cap, P.maxiter, 0);
        hipLaunchKernelGGL(k_basis_combine_acc, gridD, kBlock, 0, stream, n,
                           Z.p, ld, ctl.p, x, hk.tail_extrap);
    }
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}
