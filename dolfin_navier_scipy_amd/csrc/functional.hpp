// Device-resident momentum-balance functionals of the explicit time loops
// (drag, lift, pressure differences, torque, patch averages): ONE kernel in
// front of a time step's first kernel (behind k_lti_step and k_record_step,
// and once more behind the last step of a call) evaluates, for k < nF, with
// v = xs[cur][:nv], v_prev = xs[prev][:nv], p = pscale * xs[cur][nv:],
//   y_k = scale_k * ( ca_k . v + cm_k . (v - v_prev) / dt + cp_k . p
//                     + sum_{c in cells_k} sum_{sl < 12} w_k[c][sl] N_loc(c; v)[sl]
//                     + c0_k )
// (constant Dirichlet values: they are in c0 and in N_loc), or, where the
// Dirichlet values g move with the step (FnBcArgs: a table of their own, row j
// the values of the state before step j, one more row than the log),
//   y_k = scale_k * ( ... + cab_k . g + cmb_k . (g - g_prev) / dt
//                     + sum ... N_loc(c; v, g)[sl] + c0_k )
// with c0 the constants that are no boundary terms --
// and writes it into row `counter - 1` of a log in HBM: in the prologue of
// step s the counter still says s and xs[cur] / xs[prev] are the complete
// states after steps s - 1 / s - 2, so row r is the functional of what
// dns_imex_get_state would have returned after the (r+1)-th step.  N_loc are
// the twelve local convection sums of a cell, formed by the code k_conv_cells
// runs (convection.hpp, conv_cell_sums): the same bits.
//
// No workgroup waits for another and nothing is added atomically: workgroup g
// writes its share of y_k to log[row][g][k] in a fixed order, the getter sums
// g in index order -- the same bits in every run, launched or replayed.
#pragma once
#include <type_traits>

#include "convection.hpp"

namespace dns {

constexpr int kFnMax = 16;          // functionals of a stepper
constexpr int kFnMaxGrid = 64;      // workgroups (beyond it they stride)
constexpr int kFnUnroll = 8;        // entries of a row a lane has in flight
constexpr int kFnCells = kBlock / 8;   // cells of a workgroup per pass

struct FnArgs {
    const int *stepctr;                 // device step counter
    int nrows;                          // rows of the log
    const double *x, *xp;               // xs[cur], xs[prev]
    int nv;
    double pscale, dt;
    int nF, G;                          // G: the grid the log is laid out for
    // the sparse rows: row 3 k + t is term t (0: ca, 1: cm, 2: cp) of
    // functional k; columns of cp count from the first pressure dof
    const int *rp, *ci;
    const double *va;
    // the listed cells of functional k: [cptr[k], cptr[k + 1]); `cw`: twelve
    // weights per listed cell (slot = 2 * node + component)
    int ncl;
    const int *cptr, *cidx;
    const double *cw;
    // the convection operator's element data and constant Dirichlet values
    int ncells;
    const int *cellmap;
    const double *glam, *area, *dbcvals;
    const double *scale, *c0;
    double *log;                        // nrows x G x nF
};

// Moving Dirichlet values: the functionals' own table, (nrows + 1) x ndbc.  In
// the prologue of step s (counter s) the state is the one before step s: its
// values are row s, those of the state before it row s - 1; the closing launch
// reads row nrows.  The sparse rows are then five per functional: row
// 5 k + t, t = 3: cab over g, t = 4: cmb over g - g_prev (divided by dt).
// The kernel is instantiated per argument type, so the instance for constant
// values takes FnArgs as it stands.
struct FnBcArgs : FnArgs {
    const double *gtab;
    int ndbc;
};

// a cell's weighted sum, reduced over its eight lanes by xor shuffles, into
// the workgroup's LDS slot of the cell
struct FnWeighCells {
    const double *__restrict__ cw;      // twelve weights per listed cell
    double *cval;                       // LDS, one entry per cell of the pass
    __device__ __forceinline__ void operator()(bool live, int slot, int c,
                                               int q, double mine,
                                               double mine8) const {
        const double w_a = live ? cw[(size_t)slot * 12 + q] : 0.0;
        const double w_b = (live && q < 4) ? cw[(size_t)slot * 12 + q + 8] : 0.0;
        double s = fma(w_b, mine8, w_a * mine);
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        if (q == 0) cval[threadIdx.x >> 3] = s;
    }
};

// Sparse rows: one wave per (functional, term), the waves of the whole grid
// stride over the 3 nF (5 nF) rows, lanes stride over a row's entries,
// wave_sum (the order of k_record_step's y).  Element part: eight lanes per listed cell
// through conv_cells_block_to (the listed cells are its `sel`), the workgroups
// stride over the list; the cells of a pass are summed per functional in
// list order by ONE thread.
//
// Constant Dirichlet values (ARGS = FnArgs): NOTHING the kernel loads depends
// on the counter: it is asked for first and looked at last, where it gives the
// row to store to (or none: the launch in front of the first step after the
// functionals were set, whose sums are dropped).  Moving ones (FnBcArgs): the
// counter selects the two table rows, so their loads wait for it; the row
// indices are clamped to [0, nrows] (the launch in front of the first step
// takes row 0 twice and drops its sums).  Every address is valid whatever the
// counter says.
template <typename ARGS>
__global__ void __launch_bounds__(kBlock) k_functional_step(ARGS a) {
    constexpr bool kBc = std::is_same<ARGS, FnBcArgs>::value;
    constexpr int kTerms = kBc ? 5 : 3;
    __shared__ double rowsum[kTerms * kFnMax];
    __shared__ double cval[kFnCells];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g = blockIdx.x, G = a.G;
    constexpr int kWaves = kBlock / kWave;
    const int step = *a.stepctr;
    const double *gc = a.dbcvals, *gp = a.dbcvals;
    if constexpr (kBc) {
        const int r1 = min(max(step, 0), a.nrows);
        const int r0 = min(max(step - 1, 0), a.nrows);
        gc = a.gtab + (size_t)r1 * a.ndbc;
        gp = a.gtab + (size_t)r0 * a.ndbc;
    }
    const int nT = kTerms * a.nF;
    int cp0 = 0, cp1 = 0;
    double sc = 0.0, c0 = 0.0;
    if (tid < a.nF) {
        cp0 = a.cptr[tid];
        cp1 = a.cptr[tid + 1];
        sc = a.scale[tid];
        c0 = a.c0[tid];
    }
    // ---- sparse rows ----
    for (int t = g * kWaves + wave; t < nT; t += G * kWaves) {
        const int k0 = a.rp[t], k1 = a.rp[t + 1];
        const int term = t % kTerms;
        const double *__restrict__ pa = a.x + (term == 2 ? a.nv : 0);
        const double *__restrict__ pb = a.xp;
        if constexpr (kBc) {
            if (term >= 3) {
                pa = gc;
                pb = gp;
            }
        }
        // kFnUnroll entries of a lane at a time: their (column, value) loads
        // go out together, then the gathers, then the products in the order
        // of the plain loop
        double acc = 0.0;
        for (int k = k0 + lane; k < k1; k += kFnUnroll * kWave) {
            int c[kFnUnroll];
            double w[kFnUnroll], xv[kFnUnroll];
#pragma unroll
            for (int j = 0; j < kFnUnroll; ++j) {
                const int kk = k + j * kWave;
                c[j] = kk < k1 ? a.ci[kk] : 0;
                w[j] = kk < k1 ? a.va[kk] : 0.0;
            }
            if (term == 1 || (kBc && term == 4)) {
#pragma unroll
                for (int j = 0; j < kFnUnroll; ++j)
                    xv[j] = pa[c[j]] - pb[c[j]];
            } else {
#pragma unroll
                for (int j = 0; j < kFnUnroll; ++j) xv[j] = pa[c[j]];
            }
#pragma unroll
            for (int j = 0; j < kFnUnroll; ++j)
                acc = k + j * kWave < k1 ? fma(w[j], xv[j], acc) : acc;
        }
        acc = wave_sum(acc);
        if (lane == 0) rowsum[t] = acc;
    }
    // ---- element part ----
    double cacc = 0.0;      // thread k < nF: the cells of functional k here
    for (int pass = g; pass * kFnCells < a.ncl; pass += G) {
        const int base = pass * kFnCells;
        conv_cells_block_to(pass, a.ncells, a.cellmap, a.glam, a.area,
                            ConvFromVec{a.x}, TabRef{gc, nullptr, 0, 1},
                            FnWeighCells{a.cw, cval}, a.cidx, a.ncl);
        __syncthreads();
        if (tid < a.nF) {
            const int j0 = max(base, cp0);
            const int j1 = min(min(base + kFnCells, a.ncl), cp1);
            for (int jj = j0; jj < j1; ++jj) cacc += cval[jj - base];
        }
        __syncthreads();
    }
    __syncthreads();
    // ---- this workgroup's share of y_k ----
    const int row = step - 1;
    if (tid < a.nF && row >= 0 && row < a.nrows) {
        double tot = cacc;
        // (row t was summed here if the wave (t mod G * kWaves) is one of ours)
        const int t0 = kTerms * tid;
        if ((t0 / kWaves) % G == g) tot += rowsum[t0];
        if (((t0 + 1) / kWaves) % G == g) tot += rowsum[t0 + 1] / a.dt;
        if (((t0 + 2) / kWaves) % G == g) tot += a.pscale * rowsum[t0 + 2];
        if constexpr (kBc) {
            if (((t0 + 3) / kWaves) % G == g) tot += rowsum[t0 + 3];
            if (((t0 + 4) / kWaves) % G == g) tot += rowsum[t0 + 4] / a.dt;
        }
        if (g == 0) tot += c0;
        a.log[((size_t)row * G + g) * a.nF + tid] = sc * tot;
    }
}

// enough workgroups for one wave per sparse row (three per functional, five
// with moving Dirichlet values) / eight lanes per listed cell
inline int functional_grid(int nF, int ncl, int terms = 3) {
    const int g = std::max((terms * nF + kBlock / kWave - 1) / (kBlock / kWave),
                           (ncl + kFnCells - 1) / kFnCells);
    return std::max(1, std::min(g, kFnMaxGrid));
}

}  // namespace dns
