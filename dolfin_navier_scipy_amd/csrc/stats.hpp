// Device-resident flow statistics of the explicit time loops (mean flow, mean
// pressure, variances, Reynolds stresses; phase averages and batch means by
// bins): ONE kernel in front of a time step's first kernel (behind
// k_lti_step, k_record_step and k_functional_step, and once more behind the
// last step of a call) adds what the step before has left in xs[cur],
//   x = [v; pscale * p~]          (k_record_step's snapshot, bit for bit)
// into the sums of bin b = bin[row], row = (device step counter) - 1:
//   N_b += 1,  S1_b[i] += x[i],  S2_b[i] += x[i]^2   (i < n),
//   SX_b[q] += x[pi[q]] * x[pj[q]]                    (q < npairs)
// (b = -1: the step is skipped).  S1 is plain additions, S2 and SX are fma.
//
// Unlike the rows of the other attachments a sum must not see a row twice,
// and a row IS launched twice: by the closing node of a call and by the front
// node of the next call's first step (dns_imex_step: every step).  So
// workgroup g keeps a mark done[g], the number of rows it has added since the
// counter was last rewound, and adds row r only where done[g] == r.  It reads
// and writes its own mark only and owns a fixed set of entries: no workgroup
// waits for another, nothing is added atomically, and within a bin the rows
// are added in step order -- the same bits in every run, launched or
// replayed, however the steps are split into calls.  The marks are part of the
// accumulator buffer, which a batch checkpoints as a whole: a restored batch
// adds its rows again to the sums it started from.
#pragma once
#include "kernels.hpp"

namespace dns {

constexpr int kStMaxBins = 256;
constexpr int kStMaxGrid = 256;     // workgroups (beyond it they stride)

// The accumulator buffer, doubles:
//   done[G] | N[nbins] | (pad to even) | bin 0: S1[ld] S2[ld] SX[npx] | bin 1 ..
// ld: the ring's (even, >= n), npx: npairs rounded up to even -- every S1 / S2
// starts on a 16-byte boundary.
struct StLayout {
    int G = 1, nbins = 0, ld = 0, npairs = 0;
    int head() const { return (G + nbins + 1) & ~1; }
    int npx() const { return (npairs + 1) & ~1; }
    size_t bin_stride() const { return (size_t)2 * ld + npx(); }
    size_t total() const { return head() + (size_t)nbins * bin_stride(); }
};

struct StArgs {
    const int *stepctr;                 // device step counter
    int nrows;                          // rows of the bin table
    const double *x;                    // xs[cur]: v (nv), p~ (n - nv), padding
    int nv, n, ld;
    double pscale;                      // p = pscale * p~ (as get_state)
    const int *bin;                     // nrows entries in -1..nbins-1
    int nbins, npairs;
    const int2 *pairs;                  // (pi, pj), both in [0, n)
    double *acc;                        // StLayout
    int G, head, npx;
};

// Workgroup g owns the pairs i of the ring vector (entries 2 i, 2 i + 1) and
// the products q with i, q == g * kBlock + tid modulo G * kBlock; 16-byte
// loads and stores over x, S1 and S2.  A chain of dependent loads and little
// else (counter -> bin -> accumulator address), so what depends on nothing is
// asked for before the counter is looked at: the first pair of x, the first
// pair indices, the workgroup's mark.
__global__ void __launch_bounds__(kBlock) k_stats_step(StArgs a) {
    // (S1 is a sum of the recorder's entries: the scaling of the pressure
    // must not be contracted into the addition)
#pragma clang fp contract(off)
    const int tid = threadIdx.x, g = blockIdx.x;
    const int stride = a.G * kBlock;
    // ---- loads that depend on nothing ----
    const int step = *a.stepctr;
    const int n2 = a.ld >> 1;
    const int i_first = g * kBlock + tid;
    const double2 *__restrict__ src = reinterpret_cast<const double2 *>(a.x);
    double2 w_first = make_double2(0.0, 0.0);
    if (i_first < n2) w_first = src[i_first];
    int2 q_first = make_int2(0, 0);
    if (i_first < a.npairs) q_first = a.pairs[i_first];
    const double mark = a.acc[g];
    const int row = step - 1;
    if (row < 0 || row >= a.nrows) return;      // (the same in every thread)
    // ---- loads that depend on the counter only ----
    const int b = a.bin[row];
    __syncthreads();        // every thread has the mark before one rewrites it
    if (mark == (double)row && b >= 0 && b < a.nbins) {
        double *__restrict__ base =
            a.acc + a.head + (size_t)b * ((size_t)2 * a.ld + a.npx);
        double2 *__restrict__ s1 = reinterpret_cast<double2 *>(base);
        double2 *__restrict__ s2 = reinterpret_cast<double2 *>(base + a.ld);
        double *__restrict__ sx = base + (size_t)2 * a.ld;
        // (entries 2 i, 2 i + 1; the caller has i < n2)
        auto add_pair = [&](int i, double2 w) {
            const int e = 2 * i;
            if (e >= a.n) return;               // padding only
            double2 u = s1[i], t = s2[i];
            if (e >= a.nv) w.x *= a.pscale;
            if (e + 1 >= a.nv) w.y *= a.pscale;
            u.x += w.x;
            t.x = fma(w.x, w.x, t.x);
            if (e + 1 < a.n) {                  // (else: padding, stays 0)
                u.y += w.y;
                t.y = fma(w.y, w.y, t.y);
            }
            s1[i] = u;
            s2[i] = t;
        };
        if (i_first < n2) add_pair(i_first, w_first);
        for (int i = i_first + stride; i < n2; i += stride)
            add_pair(i, src[i]);
        for (int q = i_first; q < a.npairs; q += stride) {
            const int2 ij = q == i_first ? q_first : a.pairs[q];
            double xi = a.x[ij.x], xj = a.x[ij.y];
            if (ij.x >= a.nv) xi *= a.pscale;
            if (ij.y >= a.nv) xj *= a.pscale;
            sx[q] = fma(xi, xj, sx[q]);
        }
        if (g == 0 && tid == 0) a.acc[a.G + b] += 1.0;
    }
    __syncthreads();
    if (tid == 0) a.acc[g] = (double)(row + 1);
}

// one 16-byte pair (and one product) per thread, capped
inline int stats_grid(int ld, int npairs) {
    const int work = std::max(ld / 2, npairs);
    return std::max(1, std::min((work + kBlock - 1) / kBlock, kStMaxGrid));
}

}  // namespace dns
