// Device-resident snapshot ensemble of the explicit time loops and the two
// dense operations of the method of snapshots on it (POD):
//   E      nslots x ldv doubles, slot s = the velocity v of a kept step (ldv:
//          NV rounded up to 64; the pressure plays no part)
//   G      = E W E^T  (m x m, W a symmetric NV x NV CSR matrix or the identity)
//   out    = coef E   (r x NV: modes and mean flow from the m x m algebra)
//
// k_ensemble_step: ONE kernel in front of a time step's first kernel (behind
// the other front nodes, and once more behind the last step of a call) copies
// what the step before has left in xs[cur][0:NV] into slot `slot[row]`, row =
// (device step counter) - 1 -- the bits of k_record_step's snapshot of v.  A
// row launched for twice, or a restored batch, overwrites its own slot with
// the same bits: no marks, no checkpoint.
//
// The Gram matrix runs behind the loop as plain launches, one block column jb
// of 16 snapshots at a time:
//   k_ens_spmm         Y = E[16 jb .. 16 jb + 15, :] W   (skipped for W = I)
//   k_ens_gram         partial tiles (ib <= jb, jb) per chunk of kEnsChunk k
//   k_ens_gram_reduce  sums the partials in chunk order, writes G and mirrors
// P = X W Y^T for two row sets (launch_ensemble_project: the reduced operators
// of a Galerkin projection) runs the same three kernels, k_ens_gram and
// k_ens_gram_reduce in their non-mirroring form <false>: every tile (ib, jb),
// every entry written once.
// No atomics; the chunk length is a constant, so the bits are the same in
// every run and on every grid.  Extra memory beside E: Y, 16 x ldv doubles,
// and the partial tiles of one block column, ceil(m / 16) x ceil(NV / 1024) x
// 256 doubles (m = 400, NV = 150k: 19 MB + 7.5 MB), never a second ensemble.
#pragma once
#include "ensemble_host.hpp"
#include "kernels.hpp"

namespace dns {

struct EnsStepArgs {
    const int *stepctr;                 // device step counter
    int nrows;                          // rows of the slot table
    const double *x;                    // xs[cur]: v (nv) first
    int nv;
    const int *slot;                    // nrows entries, -1: step not kept
    double *E;                          // nslots x ldv
    int nslots;
    size_t ldv;
};

// The workgroups stride over the pairs of v with 16-byte loads and stores.  A
// chain of dependent loads (counter -> slot -> store address): the first pair
// of every thread is asked for before the counter is looked at.
__global__ void __launch_bounds__(kBlock) k_ensemble_step(EnsStepArgs a) {
    const int tid = threadIdx.x;
    // ---- loads that depend on nothing ----
    const int step = *a.stepctr;
    const int n2 = (a.nv + 1) >> 1;     // (nv odd: the ring is even and >= nv + 1)
    const int i_first = blockIdx.x * kBlock + tid;
    const double2 *__restrict__ src = reinterpret_cast<const double2 *>(a.x);
    double2 w_first = make_double2(0.0, 0.0);
    if (i_first < n2) w_first = src[i_first];
    const int row = step - 1;
    if (row < 0 || row >= a.nrows) return;      // (the same in every thread)
    // ---- loads that depend on the counter only ----
    const int sl = a.slot[row];
    if (sl < 0 || sl >= a.nslots) return;
    double2 *__restrict__ dst =
        reinterpret_cast<double2 *>(a.E + (size_t)sl * a.ldv);
    for (int i = i_first; i < n2; i += gridDim.x * kBlock) {
        double2 w = i == i_first ? w_first : src[i];
        if (2 * i + 1 >= a.nv) w.y = 0.0;       // (padding of the slot)
        dst[i] = w;
    }
}

// one pair per thread, capped (beyond it the workgroups stride)
inline int ensemble_step_grid(int nv) {
    return std::max(1, std::min(((nv + 1) / 2 + kBlock - 1) / kBlock, 256));
}

// ---- Y = E_block W -----------------------------------------------------------
struct EnsSpmmArgs {
    const double *E;                    // first snapshot of the block
    int ns;                             // snapshots of the block, 1..16
    int nv;
    size_t ld, ldy;
    const int *rp, *ci;                 // W (nv x nv, any)
    const double *va;
    double *Y;                          // 16 x ldy
};

// One wave per row r of W, the waves of the grid stride over the rows, lanes
// stride over the row's entries; (column, value) is loaded once and used for
// every snapshot of the block; wave_sum: a fixed order.  For any W
// Y[s, r] = sum_c W[r, c] E[s, c] = (W e_s)[r], so that the tiles behind it
// hold x_i . (W e_j); for a symmetric W that is (E W)[s, r] as well.
__global__ void __launch_bounds__(kBlock) k_ens_spmm(EnsSpmmArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wpg = kBlock / kWave;
    for (int r = blockIdx.x * wpg + wave; r < a.nv; r += gridDim.x * wpg) {
        const int k0 = a.rp[r], k1 = a.rp[r + 1];
        double acc[kEnsTile];
#pragma unroll
        for (int s = 0; s < kEnsTile; ++s) acc[s] = 0.0;
        for (int k = k0 + lane; k < k1; k += kWave) {
            const int c = a.ci[k];
            const double w = a.va[k];
            const double *__restrict__ e = a.E + c;
#pragma unroll
            for (int s = 0; s < kEnsTile; ++s)
                if (s < a.ns) acc[s] = fma(w, e[(size_t)s * a.ld], acc[s]);
        }
#pragma unroll
        for (int s = 0; s < kEnsTile; ++s) {
            const double y = wave_sum(acc[s]);
            if (lane == s && s < a.ns) a.Y[(size_t)s * a.ldy + r] = y;
        }
    }
}

// ---- partial tiles of G -------------------------------------------------------
typedef double ens_f64x4 __attribute__((ext_vector_type(4)));
constexpr int kEnsGramDepth = 4;    // 16-byte loads a lane has in flight per operand

struct EnsGramArgs {
    const double *E;                    // m x ld
    const double *B;                    // the 16 rows j of the block column:
                                        // Y, or E + 16 jb ld (W = I)
    int m, nv, jb, nchunks;
    size_t ld, ldb;
    double *part;                       // (jb + 1) x nchunks x 256
    int mj = 0;                         // <false>: rows of the other set (the
                                        // block column's side), part is
                                        // ens_blocks(m) x nchunks x 256
};

// entries k, k + 1 of a row (k even), nothing at or behind `kend`, nothing of
// a row that does not exist
__device__ __forceinline__ double2 ens_pair(const double *__restrict__ p, int k,
                                            int kend, bool row_ok) {
    double2 v = make_double2(0.0, 0.0);
    if (row_ok) {
        if (k + 1 < kend)
            v = *reinterpret_cast<const double2 *>(p + k);
        else if (k < kend)
            v.x = p[k];
    }
    return v;
}

// One wave = one 16 x 16 tile (ib, jb) over one chunk of k, the four waves of
// a workgroup take four block rows ib (they share the loads of B).
// v_mfma_f64_16x16x4_f64: lane l holds A[l & 15][kq] and B[kq][l & 15], kq =
// l >> 4, with A[i][k] = E[16 ib + i, k] and B[k][j] = Y[16 jb + j, k]: both
// operands are "row l & 15, entry kq" of their matrix.  A lane loads the pair
// k0 + 2 kq, k0 + 2 kq + 1 of its row with one 16-byte load and feeds the two
// to two MFMAs (a permutation of k, the same for A and B).  Result register g
// of lane l is row (l >> 4) + 4 g, column l & 15 (NOT the f32 map).
// SYM: G = E W E^T, the tiles ib <= jb only (the reduction mirrors); !SYM:
// every block row ib of E against the block column jb of another row set of
// `mj` rows.
template <bool SYM>
__global__ void __launch_bounds__(kBlock) k_ens_gram(EnsGramArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ib = blockIdx.y * (kBlock / kWave) + wave;
    if (SYM ? ib > a.jb : ib >= ens_blocks(a.m)) return;    // (a whole wave)
    const int chunk = blockIdx.x;
    const int kbeg = chunk * kEnsChunk;
    const int kend = min(a.nv, kbeg + kEnsChunk);
    const int row = lane & 15, kq = lane >> 4;
    const int i = ib * kEnsTile + row, j = a.jb * kEnsTile + row;
    const bool iok = i < a.m, jok = j < (SYM ? a.m : a.mj);
    const double *__restrict__ pa = a.E + (size_t)(iok ? i : 0) * a.ld;
    const double *__restrict__ pb = a.B + (size_t)(jok ? row : 0) * a.ldb;
    ens_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    // kEnsGramDepth steps of 8 entries at a time: their loads go out
    // together, then the MFMAs (behind `kend`: zeros, which add nothing)
    for (int k0 = kbeg; k0 < kend; k0 += 8 * kEnsGramDepth) {   // (uniform)
        double2 x[kEnsGramDepth], y[kEnsGramDepth];
#pragma unroll
        for (int u = 0; u < kEnsGramDepth; ++u) {
            const int k = k0 + 8 * u + 2 * kq;
            x[u] = ens_pair(pa, k, kend, iok);
            y[u] = ens_pair(pb, k, kend, jok);
        }
#pragma unroll
        for (int u = 0; u < kEnsGramDepth; ++u) {
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u].x, y[u].x, acc, 0,
                                                       0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x[u].y, y[u].y, acc, 0,
                                                       0, 0);
        }
    }
    double *__restrict__ out =
        a.part + ((size_t)ib * a.nchunks + chunk) * (kEnsTile * kEnsTile);
#pragma unroll
    for (int g = 0; g < 4; ++g) out[g * kWave + lane] = acc[g];
}

// Workgroup ib, thread e: entry e of tile (ib, jb), its partials added in
// chunk order; of a diagonal tile the upper triangle only; written to G[i, j]
// and G[j, i]: G is exactly symmetric.  !SYM: every entry of the tile, to
// G[i, j] of the m x mj result alone.
template <bool SYM>
__global__ void __launch_bounds__(kBlock)
k_ens_gram_reduce(const double *__restrict__ part, int nchunks, int jb, int m,
                  double *__restrict__ G, int mj) {
    const int ib = blockIdx.x, e = threadIdx.x;
    const double *__restrict__ p =
        part + (size_t)ib * nchunks * (kEnsTile * kEnsTile) + e;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += p[(size_t)c * (kEnsTile * kEnsTile)];
    const int i = ib * kEnsTile + ens_tile_row(e);
    const int j = jb * kEnsTile + ens_tile_col(e);
    if (SYM) {
        if (i < m && j < m && j >= i) {
            G[(size_t)i * m + j] = s;
            G[(size_t)j * m + i] = s;
        }
    } else if (i < m && j < mj) {
        G[(size_t)i * mj + j] = s;
    }
}

// ---- out = coef E ---------------------------------------------------------------
struct EnsCombArgs {
    const double *E;                    // m x ld
    int m, nv, r;
    size_t ld, ldo;
    const double *coef;                 // packed: ens_pack_coef
    double *out;                        // r x ldo
};

// A thread owns the columns k, k + 1 (one 16-byte load per snapshot) and the
// rows q0 .. q0 + 15 of `out`, q0 = 16 blockIdx.y: 32 accumulators, s ascends
// with fma -- acc = fma(coef[q, s], E[s, k], acc), the order of the host loop.
// The coefficients come packed (ens_pack_coef: the 16 of a pass and a snapshot
// side by side, zeros behind r) and are the same in every lane: scalar loads.
template <bool TWO>
__device__ __forceinline__ void ens_combine_cols(const EnsCombArgs &a, int k) {
    const int q0 = blockIdx.y * kEnsAcc;
    const int nq = min(kEnsAcc, a.r - q0);
    const double *__restrict__ e = a.E + k;
    const double *__restrict__ c =
        a.coef + (size_t)blockIdx.y * a.m * kEnsAcc;
    double2 acc[kEnsAcc];
#pragma unroll
    for (int q = 0; q < kEnsAcc; ++q) acc[q] = make_double2(0.0, 0.0);
#pragma unroll 1
    for (int s = 0; s < a.m; ++s) {
        double2 v = make_double2(0.0, 0.0);
        if (TWO)
            v = *reinterpret_cast<const double2 *>(e + (size_t)s * a.ld);
        else
            v.x = e[(size_t)s * a.ld];
#pragma unroll
        for (int q = 0; q < kEnsAcc; ++q) {
            const double cq = c[(size_t)s * kEnsAcc + q];
            acc[q].x = fma(cq, v.x, acc[q].x);
            if (TWO) acc[q].y = fma(cq, v.y, acc[q].y);
        }
    }
#pragma unroll
    for (int q = 0; q < kEnsAcc; ++q) {
        if (q < nq) {                   // (rows at and behind r: never stored)
            double *__restrict__ o = a.out + (size_t)(q0 + q) * a.ldo + k;
            if (TWO)
                *reinterpret_cast<double2 *>(o) = acc[q];
            else
                o[0] = acc[q].x;
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_ens_combine(EnsCombArgs a) {
    const int k = 2 * (blockIdx.x * kBlock + threadIdx.x);
    if (k + 1 < a.nv)
        ens_combine_cols<true>(a, k);
    else if (k < a.nv)                  // (nv odd: its last column)
        ens_combine_cols<false>(a, k);
}

// ---- launchers (the stepper's entries and the stateless ones alike) ------------

// W on the device (what k_ens_spmm reads)
struct EnsWeights {
    int nv = 0;
    DevBuf<int> rp, ci;
    DevBuf<double> va;
    int upload(const dns_csr *w, hipStream_t s) {
        nv = w->nrows;
        DNS_TRY(rp.alloc((size_t)w->nrows + 1));
        DNS_TRY(ci.alloc((size_t)w->nnz));
        DNS_TRY(va.alloc((size_t)w->nnz));
        DNS_TRY(rp.upload(w->rowptr, (size_t)w->nrows + 1, s));
        if (w->nnz > 0) {
            DNS_TRY(ci.upload(w->colidx, (size_t)w->nnz, s));
            DNS_TRY(va.upload(w->vals, (size_t)w->nnz, s));
        }
        return DNS_OK;
    }
};

inline int check_ensemble_weights(const dns_csr *w, int nv) {
    if (!w) return DNS_OK;
    DNS_TRY(check_csr(w, "W"));
    if (w->nrows != nv || w->ncols != nv)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "ensemble: W must be NV x NV (%d), it is %d x %d", nv,
                    (int)w->nrows, (int)w->ncols);
    return DNS_OK;
}

// G (device, m x m) = E W E^T for the m snapshots at E (ld apart); W null: I.
// `y` and `part` are scratch the caller keeps (grown here).  Enqueued on `s`.
inline int launch_ensemble_gram(const double *E, int m, int nv, size_t ld,
                                const EnsWeights *W, DevBuf<double> &y,
                                DevBuf<double> &part, double *G,
                                hipStream_t s) {
    DNS_TRY(check_ensemble_shape(m, nv, ld));
    const int nb = ens_blocks(m), nch = ens_chunks(nv);
    const size_t ldy = ens_ldv(nv);
    if (W && y.n < (size_t)kEnsTile * ldy) DNS_TRY(y.alloc((size_t)kEnsTile * ldy));
    if (part.n < ens_partials(m, nv)) DNS_TRY(part.alloc(ens_partials(m, nv)));
    const int wpg = kBlock / kWave;
    for (int jb = 0; jb < nb; ++jb) {
        const double *Ej = E + (size_t)jb * kEnsTile * ld;
        if (W) {
            const EnsSpmmArgs sa{Ej, std::min(kEnsTile, m - jb * kEnsTile), nv,
                                 ld, ldy, W->rp.p, W->ci.p, W->va.p, y.p};
            hipLaunchKernelGGL(k_ens_spmm,
                               std::max(1, std::min((nv + wpg - 1) / wpg, 4096)),
                               kBlock, 0, s, sa);
        }
        const EnsGramArgs ga{E, W ? y.p : Ej, m, nv, jb, nch, ld,
                             W ? ldy : ld, part.p};
        hipLaunchKernelGGL(k_ens_gram<true>, dim3(nch, (jb + wpg) / wpg),
                           kBlock, 0, s, ga);
        hipLaunchKernelGGL(k_ens_gram_reduce<true>, jb + 1, kBlock, 0, s,
                           part.p, nch, jb, m, G, m);
    }
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}

// P (device, mx x my) = X W Y^T, P[i, j] = x_i . (W y_j), for the mx rows at X
// (ldx apart) and the my rows at Y (ldy apart); W null: I.  The chunks and the
// order of their sums are those of the Gram matrix: with X = Y and a
// symmetric W the tiles ib <= jb hold its bits.  `y` and `part` are scratch
// the caller keeps (grown here).  Enqueued on `s`.
inline int launch_ensemble_project(const double *X, int mx, size_t ldx,
                                   const double *Y, int my, size_t ldy, int nv,
                                   const EnsWeights *W, DevBuf<double> &y,
                                   DevBuf<double> &part, double *P,
                                   hipStream_t s) {
    DNS_TRY(check_ensemble_shape(mx, nv, ldx));
    DNS_TRY(check_ensemble_shape(my, nv, ldy));
    const int nbx = ens_blocks(mx), nby = ens_blocks(my), nch = ens_chunks(nv);
    const size_t ldw = ens_ldv(nv);
    if (W && y.n < (size_t)kEnsTile * ldw) DNS_TRY(y.alloc((size_t)kEnsTile * ldw));
    if (part.n < ens_partials(mx, nv)) DNS_TRY(part.alloc(ens_partials(mx, nv)));
    const int wpg = kBlock / kWave;
    for (int jb = 0; jb < nby; ++jb) {
        const double *Yj = Y + (size_t)jb * kEnsTile * ldy;
        if (W) {
            const EnsSpmmArgs sa{Yj, std::min(kEnsTile, my - jb * kEnsTile), nv,
                                 ldy, ldw, W->rp.p, W->ci.p, W->va.p, y.p};
            hipLaunchKernelGGL(k_ens_spmm,
                               std::max(1, std::min((nv + wpg - 1) / wpg, 4096)),
                               kBlock, 0, s, sa);
        }
        const EnsGramArgs ga{X, W ? y.p : Yj, mx, nv, jb, nch, ldx,
                             W ? ldw : ldy, part.p, my};
        hipLaunchKernelGGL(k_ens_gram<false>, dim3(nch, (nbx + wpg - 1) / wpg),
                           kBlock, 0, s, ga);
        hipLaunchKernelGGL(k_ens_gram_reduce<false>, nbx, kBlock, 0, s, part.p,
                           nch, jb, mx, P, my);
    }
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}

// out (device, r x ldo, ldo even and >= nv) = coef E; coef on the device as
// ens_pack_coef has laid it out (ens_passes(r) x m x 16 doubles)
inline int launch_ensemble_combine(const double *E, int m, int nv, size_t ld,
                                   const double *coef, int r, double *out,
                                   size_t ldo, hipStream_t s) {
    DNS_TRY(check_ensemble_shape(m, nv, ld));
    if (r < 1 || ldo < (size_t)nv || (ldo & 1))
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "ensemble: r = %d < 1 or a bad output stride %zu", r, ldo);
    const EnsCombArgs a{E, m, nv, r, ld, ldo, coef, out};
    const int gx = ((nv + 1) / 2 + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_ens_combine, dim3(gx, ens_passes(r)), kBlock, 0, s, a);
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}

}  // namespace dns
