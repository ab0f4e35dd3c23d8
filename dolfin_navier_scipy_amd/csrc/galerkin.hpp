// The cubic convection tensor of a POD-Galerkin projection on the device:
//   T[i, j, k] = sum_cells sum_q w_q |cell| phi_i(x_q) . (u_j . grad) u_k (x_q)
// for a basis of nb rows over the inner dofs (row b carries its Dirichlet
// values in row b of D), phi_i = row i < nt on the inner dofs, zero on the
// Dirichlet dofs; the 7-point rule and the tables of conv_point.
//
// Per cell a small GEMM, T_cell = P C^T with K = (point, component), 14
// padded to 16 with zeros:
//   P[i, (q, d)]      = w_q |cell| phi_i,d(x_q)                     nt   x 16
//   C[(j, k), (q, d)] = sum_e u_j,e(x_q) d_e u_k,d(x_q)             nb^2 x 16
// the cells concatenate along K: four v_mfma_f64_16x16x4_f64 per cell and
// 16 x 16 tile.
//
//   k_rom_tensor  workgroup (chunk of kRomCellChunk cells) x (group of twelve
//                 column tiles).  kRomStage cells at a time it stages, for
//                 all nb rows, u_b(x_q), grad u_b(x_q) and w_q |cell| phi_b(x_q)
//                 in LDS (one thread per (cell, row, point), the eight of a
//                 (cell, row) share their loads by shuffles; the staging is
//                 recomputed per column group: ~1.5 % of the tile flops each).
//                 Wave w carries three column tiles against all (<= 3) row
//                 tiles, nine accumulators over the chunk's cells: the C
//                 operand of a column tile -- two LDS reads, a product and an
//                 fma per lane -- is formed once and fed to the MFMAs of every
//                 row tile.  Partial tiles go to HBM.
//   k_rom_reduce  adds the partial tiles in chunk order and writes T.
// No atomics; the chunk length is a constant: the same bits in every run, on
// every device and grid.  Cells without an inner dof (the operator sorts them
// to the end) are not visited: P vanishes on them.
#pragma once
#include "convection.hpp"
#include "ensemble.hpp"
#include "galerkin_host.hpp"

namespace dns {

struct RomTensorArgs {
    const int *cellmap;                 // [12][ncells]
    const double *glam, *area;          // [6][ncells], [ncells]
    int ncells, nlive;                  // cells 0 .. nlive - 1 are visited
    const double *B;                    // nb x ld
    size_t ld;
    const double *D;                    // nb x ndbc or null (zeros)
    int ndbc;
    int nb, nt, nrt, nct;
    double *part;                       // rom_partials(nlive, nb, nt)
};

// u_b, grad u_b and the weighted test function of row b at point q of cell c
// (q == 7 or a cell behind the chunk: zeros) into the LDS rows of (s, b).
// The eight lanes q of a (cell, row) ask the memory ONCE: lane q fetches dof
// slots q and q + 8 (map entry, then the value) and geometry entry q (six
// gradients, then the area); the group hands them round by shuffles, as
// conv_cells_block_to does.  (Every lane fetching everything was 31 load
// instructions per item.)  Whole groups of eight are in the caller's loop or
// out of it.  The operation chain is conv_point's: gx / gy by two fma behind
// a product, six fma per sum over the nodes.
__device__ __forceinline__ void
rom_stage_point(const RomTensorArgs &a, int c, bool live, int b, int q,
                int lane0, double *__restrict__ u, double *__restrict__ g,
                double *__restrict__ p) {
#pragma clang fp contract(off)
    int m_a = -1, m_b = -1;
    double v_a = 0.0, v_b = 0.0, g_q = 0.0;
    if (live) {                                     // (the same in the group)
        const double *__restrict__ row = a.B + (size_t)b * a.ld;
        const double *__restrict__ drow =
            a.D ? a.D + (size_t)b * a.ndbc : nullptr;
        m_a = a.cellmap[(size_t)q * a.ncells + c];
        v_a = m_a >= 0 ? row[m_a] : (drow ? drow[-m_a - 1] : 0.0);
        if (q < 4) {
            m_b = a.cellmap[(size_t)(q + 8) * a.ncells + c];
            v_b = m_b >= 0 ? row[m_b] : (drow ? drow[-m_b - 1] : 0.0);
        }
        if (q < 6) g_q = a.glam[(size_t)q * a.ncells + c];
        if (q == 6) g_q = a.area[c];
    }
    double ul[6][2], tl[6][2], gl[3][2];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const int src = lane0 + (k & 7);
        const int m = __shfl(k < 8 ? m_a : m_b, src, 64);
        const double v = __shfl(k < 8 ? v_a : v_b, src, 64);
        ul[k >> 1][k & 1] = v;
        tl[k >> 1][k & 1] = m >= 0 ? v : 0.0;       // test functions: inner
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) gl[k >> 1][k & 1] = __shfl(g_q, lane0 + k, 64);
    const double area = __shfl(g_q, lane0 + 6, 64);
    double uq[2] = {0.0, 0.0}, tq[2] = {0.0, 0.0};
    double gr[2][2] = {{0.0, 0.0}, {0.0, 0.0}};     // gr[d][e] = d_e u_d
    double wq = 0.0;
    if (live && q < 7) {
        wq = __dmul_rn(c_conv.qw[q], area);
#pragma unroll
        for (int n = 0; n < 6; ++n) {
            const double ph = c_conv.phi[q][n];
            const double d0 = c_conv.dphi[q][n][0], d1 = c_conv.dphi[q][n][1],
                         d2 = c_conv.dphi[q][n][2];
            const double gx =
                fma(d2, gl[2][0], fma(d1, gl[1][0], __dmul_rn(d0, gl[0][0])));
            const double gy =
                fma(d2, gl[2][1], fma(d1, gl[1][1], __dmul_rn(d0, gl[0][1])));
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                uq[d] = fma(ph, ul[n][d], uq[d]);
                tq[d] = fma(ph, tl[n][d], tq[d]);
                gr[d][0] = fma(gx, ul[n][d], gr[d][0]);
                gr[d][1] = fma(gy, ul[n][d], gr[d][1]);
            }
        }
    }
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        u[2 * q + d] = uq[d];
        p[2 * q + d] = __dmul_rn(wq, tq[d]);
        g[(2 * q + d) * 2 + 0] = gr[d][0];
        g[(2 * q + d) * 2 + 1] = gr[d][1];
    }
}

// MFMA operands as in k_ens_gram: lane l holds A[l & 15][kq] and B[kq][l &
// 15], kq = l >> 4; here A[i][kk] = P[16 rt + i, kk] and B[kk][n] = C[16 ct +
// n, kk], kk = 4 step + kq.  Result register r of lane l is row (l >> 4) + 4
// r, column l & 15.
__global__ void __launch_bounds__(kBlock) k_rom_tensor(RomTensorArgs a) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) double
        sU[kRomStage * kRomMaxBasis * kRomLdU];
    __shared__ __attribute__((aligned(16))) double
        sG[kRomStage * kRomMaxBasis * kRomLdG];
    __shared__ __attribute__((aligned(16))) double
        sP[kRomStage * kRomMaxBasis * kRomLdP];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int chunk = blockIdx.x, grp = blockIdx.y;
    const int c0 = chunk * kRomCellChunk;
    const int c1 = min(a.nlive, c0 + kRomCellChunk);
    const int r16 = lane & 15, kq = lane >> 4;
    const int nb = a.nb;
    int jrow[kRomTilesPerWave], krow[kRomTilesPerWave];
    bool cok[kRomTilesPerWave];
#pragma unroll
    for (int t = 0; t < kRomTilesPerWave; ++t) {
        const int col = rom_wave_tile(grp, wave, t) * kRomTile + r16;
        cok[t] = col < rom_cols(nb);
        jrow[t] = cok[t] ? rom_col_j(col, nb) : 0;
        krow[t] = cok[t] ? rom_col_k(col, nb) : 0;
    }
    ens_f64x4 acc[kRomTilesPerWave][3];
#pragma unroll
    for (int t = 0; t < kRomTilesPerWave; ++t)
#pragma unroll
        for (int rt = 0; rt < 3; ++rt) acc[t][rt] = {0.0, 0.0, 0.0, 0.0};
    for (int cb = c0; cb < c1; cb += kRomStage) {            // (uniform)
        __syncthreads();                // the cells before are consumed
        for (int idx = tid; idx < kRomStage * nb * 8; idx += kBlock) {
            const int q = idx & 7, sb = idx >> 3;           // sb = s nb + b
            const int s = sb / nb, b = sb - s * nb;
            rom_stage_point(a, cb + s, cb + s < c1, b, q, lane & ~7,
                            sU + sb * kRomLdU, sG + sb * kRomLdG,
                            sP + sb * kRomLdP);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kRomStage; ++s) {
            if (cb + s >= c1) break;                         // (uniform)
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const int kk = 4 * st + kq;
                double x[3];
#pragma unroll
                for (int rt = 0; rt < 3; ++rt) {
                    const int i = rt * kRomTile + r16;
                    x[rt] = i < a.nt ? sP[(s * nb + i) * kRomLdP + kk] : 0.0;
                }
#pragma unroll
                for (int t = 0; t < kRomTilesPerWave; ++t) {
                    if (rom_wave_tile(grp, wave, t) >= a.nct) break;  // (uniform)
                    const double2 u = *reinterpret_cast<const double2 *>(
                        sU + (s * nb + jrow[t]) * kRomLdU +
                        2 * rom_k_point(kk));
                    const double2 g = *reinterpret_cast<const double2 *>(
                        sG + (s * nb + krow[t]) * kRomLdG + 2 * kk);
                    const double y =
                        cok[t] ? fma(u.y, g.y, __dmul_rn(u.x, g.x)) : 0.0;
#pragma unroll
                    for (int rt = 0; rt < 3; ++rt)
                        if (rt < a.nrt)                      // (uniform)
                            acc[t][rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                                x[rt], y, acc[t][rt], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < kRomTilesPerWave; ++t) {
        const int ct = rom_wave_tile(grp, wave, t);
        if (ct >= a.nct) break;
#pragma unroll
        for (int rt = 0; rt < 3; ++rt) {
            if (rt >= a.nrt) break;
            double *__restrict__ out =
                a.part + rom_part_index(chunk, rt, ct, a.nrt, a.nct);
#pragma unroll
            for (int r = 0; r < 4; ++r) out[r * kWave + lane] = acc[t][rt][r];
        }
    }
}

// Workgroup = tile (rt, ct), thread e = its entry: the partials added in
// chunk order, written to T[i, j, k] (col = j nb + k)
__global__ void __launch_bounds__(kBlock)
k_rom_reduce(const double *__restrict__ part, int nchunks, int nrt, int nct,
             int nb, int nt, double *__restrict__ T) {
    const int rt = blockIdx.x / nct, ct = blockIdx.x - rt * nct;
    const int e = threadIdx.x;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c)
        s += part[rom_part_index(c, rt, ct, nrt, nct) + e];
    const int i = rt * kRomTile + ens_tile_row(e);
    const int col = ct * kRomTile + ens_tile_col(e);
    if (i < nt && col < rom_cols(nb)) T[(size_t)i * rom_cols(nb) + col] = s;
}

// T (device, nt x nb x nb) from the basis B (device, nb x ld) and its
// Dirichlet rows D (device, nb x ndbc, or null); `part` is scratch the caller
// keeps (grown here).  Enqueued on `s`.
inline int launch_rom_tensor(const dns_conv &cv, int nlive, const double *B,
                             size_t ld, const double *D, int nb, int nt,
                             DevBuf<double> &part, double *T, hipStream_t s) {
    DNS_TRY(check_rom_shape(nb, nt, cv.nv_inner, (long long)ld, nlive));
    if (nlive < 0 || nlive > cv.ncells)
        return fail(DNS_ERR_BAD_ARGUMENT, "galerkin: %d of %d cells", nlive,
                    cv.ncells);
    const int nch = rom_chunks(nlive), nrt = rom_row_tiles(nt),
              nct = rom_col_tiles(nb);
    const size_t np = rom_partials(nlive, nb, nt);
    if (part.n < np) DNS_TRY(part.alloc(np));
    if (nch > 0) {
        const RomTensorArgs a{cv.cellmap.p, cv.glam.p, cv.area.p, cv.ncells,
                              nlive, B, ld, D, cv.ndbc, nb, nt, nrt, nct,
                              part.p};
        hipLaunchKernelGGL(k_rom_tensor, dim3(nch, rom_col_groups(nb)), kBlock,
                           0, s, a);
    }
    hipLaunchKernelGGL(k_rom_reduce, nrt * nct, kBlock, 0, s, part.p, nch, nrt,
                       nct, nb, nt, T);
    DNS_HIP(hipGetLastError());
    return DNS_OK;
}

}  // namespace dns
