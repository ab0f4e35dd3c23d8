// Device-resident observer feedback of the explicit time loops (the
// reference's `dynamic_rhs` built from `get_heunab_lti`, tiu:148-196,
// snu:1237-1247): ONE kernel in front of a time step's first kernel
//   y    = C v_c                                  (C: Ny x NV CSR, sensors)
//   f    = ha hx + hb y + drift(step)             (observer, hN x hN dense)
//   hx_n = hx + 1.5 dt f - 0.5 dt f_last          (AB2)
//   u_n  = hc hx_n                                (Nu inputs)
//   geff = g(step) + dt (c_n B u_n + c_c B u_c)   (B: NV x Nu CSR, actuators)
// The front kernels of the step then read `geff` where they read `g`.
#pragma once
#include "kernels.hpp"

namespace dns {

// limits of the redundant one-launch form (checked by dns_imex_set_feedback)
constexpr int kFbMaxState = 128, kFbMaxOut = 32, kFbMaxIn = 32;
constexpr int kFbMaxNnzC = 16384;
static_assert(kBlock == 2 * kFbMaxState, "two threads per observer row");

struct LtiArgs {
    const int *stepctr;                 // device step counter (row, parity)
    int rows;                           // rows of the drift table / the logs
    int hN, Ny, Nu, nv;
    const int *crp, *cci;
    const double *cva;
    const int *brp, *bci;
    const double *bva;
    const double *haT, *hbT, *hc;       // ha, hb transposed; hc row major
    const double *drift;                // rows x hN, or nullptr (no drift)
    // observer state, double buffered by step parity: slot q at
    // state + q (2 hN + Nu) holds hx (hN), f_last (hN), u_c (Nu)
    double *state;
    double *ylog, *ulog;                // rows x Ny, rows x Nu
    double dt, c_n, c_c;
    TabRef g;                           // the right-hand side without feedback
    const double *v;                    // current solution (velocity first)
    double *geff;
};

// Every workgroup computes y, the observer update and u_n redundantly (fixed
// summation orders: all workgroups, and every run, get the same bits) from the
// state slot of the step's parity; only workgroup 0 writes the other slot and
// the log rows.  Nobody waits for another workgroup.  Then each workgroup
// writes its rows of geff.
//
// The kernel is a chain of dependent global loads (counter -> row pointers ->
// (col, val) -> v[col] -> ... -> B rows), each a round trip of about a
// microsecond, and little else.  So everything that does not depend on y is
// asked for BEFORE the first barrier: both state slots (the parity picks one
// afterwards), ha / hb / hc into LDS (STAGE: they fit kFbStage doubles; else
// they are read where they are used), the first row of B and of g of every
// thread.  What remains in sequence: counter and row pointers of C, its
// entries, the gather from v, LDS arithmetic, the stores.
constexpr int kFbStage = 4096;

template <bool STAGE>
__global__ void __launch_bounds__(kBlock) k_lti_step(LtiArgs a) {
    __shared__ double sy[kFbMaxOut], shx[kFbMaxState], sfl[kFbMaxState],
        sf[kFbMaxState], shn[kFbMaxState], sun[kFbMaxIn], suc[kFbMaxIn],
        spart[kBlock], smat[STAGE ? kFbStage : 1];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int hN = a.hN, Ny = a.Ny, Nu = a.Nu;
    const int stride = 2 * hN + Nu;
    // ---- loads that depend on nothing ----
    int step = *a.stepctr;
    double st0 = 0.0, st1 = 0.0;        // entry `tid` of the two state slots
    if (tid < stride) {
        st0 = a.state[tid];
        st1 = a.state[stride + tid];
    }
    const int r_first = blockIdx.x * kBlock + tid;
    int bk0 = 0, bk1 = 0;
    if (r_first < a.nv) {
        bk0 = a.brp[r_first];
        bk1 = a.brp[r_first + 1];
    }
    const double *__restrict__ mhaT = a.haT, *__restrict__ mhbT = a.hbT,
                               *__restrict__ mhc = a.hc;
    if (STAGE) {
        const int n1 = hN * hN, n2 = n1 + hN * Ny, n3 = n2 + Nu * hN;
        for (int k = tid; k < n3; k += kBlock)
            smat[k] = k < n1 ? a.haT[k] : k < n2 ? a.hbT[k - n1] : a.hc[k - n2];
        mhaT = smat;
        mhbT = smat + n1;
        mhc = smat + n2;
    }
    step = step < 0 ? 0 : step;
    const int row = step >= a.rows ? a.rows - 1 : step;
    const int par = step & 1;
    double *__restrict__ nw = a.state + (size_t)(1 - par) * stride;
    // ---- loads that depend on the counter only ----
    const double *__restrict__ g = tab_row(a.g);
    const double g_first = r_first < a.nv ? g[r_first] : 0.0;
    double dr = 0.0;
    if (a.drift && tid < hN) dr = a.drift[(size_t)row * hN + tid];
    {
        const double sv = par ? st1 : st0;
        if (tid < hN) shx[tid] = sv;
        else if (tid < 2 * hN) sfl[tid - hN] = sv;
        else if (tid < stride) suc[tid - 2 * hN] = sv;
        // (2 hN + Nu can pass the block size by up to Nu: inputs only)
        if (tid + kBlock < stride)
            suc[tid + kBlock - 2 * hN] =
                a.state[(size_t)par * stride + tid + kBlock];
    }
    // y = C v_c: one wave per sensor row, lanes stride over its entries
    for (int r = wave; r < Ny; r += kBlock / kWave) {
        double acc = 0.0;
        for (int k = a.crp[r] + lane; k < a.crp[r + 1]; k += kWave)
            acc = fma(a.cva[k], a.v[a.cci[k]], acc);
        acc = wave_sum(acc);
        if (lane == 0) sy[r] = acc;
    }
    __syncthreads();
    // f = ha hx + hb y + drift: two threads per row of ha, each over half of
    // the columns (ha transposed: neighbouring threads read neighbours)
    {
        const int i = tid & (kFbMaxState - 1), half = tid / kFbMaxState;
        const int jm = hN / 2;
        const int j0 = half ? jm : 0, j1 = half ? hN : jm;
        double acc = 0.0;
        if (i < hN)
            for (int j = j0; j < j1; ++j)
                acc = fma(mhaT[(size_t)j * hN + i], shx[j], acc);
        spart[tid] = acc;
    }
    __syncthreads();
    if (tid < hN) {
        double f = spart[tid] + spart[tid + kFbMaxState];
        for (int k = 0; k < Ny; ++k)
            f = fma(mhbT[(size_t)k * hN + tid], sy[k], f);
        if (a.drift) f += dr;
        sf[tid] = f;
        shn[tid] = shx[tid] + 1.5 * a.dt * f - 0.5 * a.dt * sfl[tid];
    }
    __syncthreads();
    // u_n = hc hx_n: one wave per input
    for (int m = wave; m < Nu; m += kBlock / kWave) {
        double acc = 0.0;
        for (int i = lane; i < hN; i += kWave)
            acc = fma(mhc[(size_t)m * hN + i], shn[i], acc);
        acc = wave_sum(acc);
        if (lane == 0) sun[m] = acc;
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        if (tid < hN) {
            nw[tid] = shn[tid];
            nw[hN + tid] = sf[tid];
        }
        if (tid < Nu) {
            nw[2 * hN + tid] = sun[tid];
            a.ulog[(size_t)row * Nu + tid] = sun[tid];
        }
        if (tid < Ny) a.ylog[(size_t)row * Ny + tid] = sy[tid];
    }
    // geff = g + dt (c_n B u_n + c_c B u_c); rows of B without entries copy
    for (int r = r_first; r < a.nv; r += gridDim.x * kBlock) {
        const bool first = r == r_first;
        const int k0 = first ? bk0 : a.brp[r], k1 = first ? bk1 : a.brp[r + 1];
        double sn = 0.0, sc = 0.0;
        for (int k = k0; k < k1; ++k) {
            const int c = a.bci[k];
            sn = fma(a.bva[k], sun[c], sn);
            sc = fma(a.bva[k], suc[c], sc);
        }
        a.geff[r] = (first ? g_first : g[r]) + a.dt * (a.c_n * sn + a.c_c * sc);
    }
}

// (ha, hb, hc fit the LDS stage?)
inline bool lti_staged(int hN, int Ny, int Nu) {
    return hN * hN + hN * Ny + Nu * hN <= kFbStage;
}

inline int lti_grid(int nv) {
    return std::max(1, std::min((nv + kBlock - 1) / kBlock, 64));
}

}  // namespace dns
