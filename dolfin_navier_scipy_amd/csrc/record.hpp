// Device-resident trajectory recorder of the explicit time loops: ONE kernel
// in front of a time step's first kernel (and once more behind the last step
// of a call) writes what the step before has left in xs[cur],
//   y    = C v                    (C: Ny x NV CSR) into row `row` of the y log
//   snap = [v; pscale * p~]       into slot `slot[row]` of the snapshot buffer
// where row = (device step counter) - 1: in the prologue of step s the counter
// still says s and xs[cur] is the complete state after step s - 1, so row r
// holds what dns_imex_get_state would have returned after the (r+1)-th step.
// Replayed graphs walk through the rows without the host; a restored batch
// puts the counter back and overwrites its own rows.
#pragma once
#include "kernels.hpp"

namespace dns {

constexpr int kRecUnroll = 8;       // entries of C a lane has in flight

struct RecArgs {
    const int *stepctr;                 // device step counter
    int nrows;                          // rows of the slot table / the y log
    const double *x;                    // xs[cur]: v (nv), p~ (n - nv), padding
    int nv, n, ld;                      // ld: even, >= n (ring padding)
    double pscale;                      // p = pscale * p~ (as get_state)
    const int *slot;                    // nrows entries, -1: step not kept
    double *snap;                       // nslots x ld, or nullptr (no snapshots)
    int nslots;
    int Ny;                             // rows of C
    const int *crp, *cci;
    const double *cva;
    double *ylog;                       // nrows x Ny, or nullptr (no outputs)
};

// Outputs: one wave per row of C, the waves of the whole grid stride over the
// rows, lanes stride over a row's entries, wave_sum: a fixed summation order
// (the same bits in every run, launched or replayed; the order of
// k_lti_step's y).  Snapshots: the workgroups stride over the ld / 2 pairs of
// the ring vector with 16-byte loads and stores.
//
// A short chain of dependent loads and little else (counter -> slot -> store
// address; counter -> store address for y), so everything that depends on
// nothing is asked for before the counter is looked at: the first pair of
// every thread, the row pointers of every wave's first row.
__global__ void __launch_bounds__(kBlock) k_record_step(RecArgs a) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    // ---- loads that depend on nothing ----
    const int step = *a.stepctr;
    const int n2 = a.ld >> 1;
    const int i_first = blockIdx.x * kBlock + tid;
    const double2 *__restrict__ src = reinterpret_cast<const double2 *>(a.x);
    double2 w_first = make_double2(0.0, 0.0);
    if (a.snap && i_first < n2) w_first = src[i_first];
    const int r_first = blockIdx.x * (kBlock / kWave) + wave;
    int k0_first = 0, k1_first = 0;
    if (a.ylog && r_first < a.Ny) {
        k0_first = a.crp[r_first];
        k1_first = a.crp[r_first + 1];
    }
    const int row = step - 1;
    if (row < 0 || row >= a.nrows) return;      // (the same in every thread)
    // ---- loads that depend on the counter only ----
    int sl = -1;
    if (a.snap) sl = a.slot[row];
    // y = C v
    if (a.ylog) {
        double *__restrict__ y = a.ylog + (size_t)row * a.Ny;
        for (int r = r_first; r < a.Ny; r += gridDim.x * (kBlock / kWave)) {
            const bool first = r == r_first;
            const int k0 = first ? k0_first : a.crp[r];
            const int k1 = first ? k1_first : a.crp[r + 1];
            // kRecUnroll entries of a lane at a time: their (column, value)
            // loads go out together, then the gathers, then the products in
            // the order of the plain loop (the same bits)
            double acc = 0.0;
            for (int k = k0 + lane; k < k1; k += kRecUnroll * kWave) {
                int c[kRecUnroll];
                double w[kRecUnroll], xv[kRecUnroll];
#pragma unroll
                for (int j = 0; j < kRecUnroll; ++j) {
                    const int kk = k + j * kWave;
                    c[j] = kk < k1 ? a.cci[kk] : 0;
                    w[j] = kk < k1 ? a.cva[kk] : 0.0;
                }
#pragma unroll
                for (int j = 0; j < kRecUnroll; ++j) xv[j] = a.x[c[j]];
#pragma unroll
                for (int j = 0; j < kRecUnroll; ++j)
                    acc = k + j * kWave < k1 ? fma(w[j], xv[j], acc) : acc;
            }
            acc = wave_sum(acc);
            if (lane == 0) y[r] = acc;
        }
    }
    // snapshot
    if (sl >= 0 && sl < a.nslots) {
        double2 *__restrict__ dst =
            reinterpret_cast<double2 *>(a.snap + (size_t)sl * a.ld);
        for (int i = i_first; i < n2; i += gridDim.x * kBlock) {
            double2 w = i == i_first ? w_first : src[i];
            const int e = 2 * i;
            if (e >= a.nv && e < a.n) w.x *= a.pscale;
            if (e + 1 >= a.nv && e + 1 < a.n) w.y *= a.pscale;
            dst[i] = w;
        }
    }
}

// enough workgroups for one pair per thread / one row of C per wave, capped at
// one per CU (beyond it they stride)
inline int record_grid(int ld, bool snaps, int Ny) {
    int g = 1;
    if (snaps) g = std::max(g, (ld / 2 + kBlock - 1) / kBlock);
    if (Ny > 0) g = std::max(g, (Ny + kBlock / kWave - 1) / (kBlock / kWave));
    return std::min(g, 256);
}

}  // namespace dns
