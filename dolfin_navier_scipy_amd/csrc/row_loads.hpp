// Row loads of the latency-bound gather kernels of the lazy six-node step,
// written so that a LEVEL of loads stays one basic block.
//
// A load behind `cond ? p[i] : 0` cannot be speculated by the compiler: it
// lands in an exec-masked block of its own, closed by a wait for ALL loads in
// flight, and a kernel written "level by level" comes out with one memory
// round trip per load group instead of one per level.  Here every lane loads
// unconditionally from an index CLAMPED INTO ITS OWN ROW and the value is
// selected afterwards:
//
//   level 1  row pointers (with whatever else belongs to the row itself)
//   level 2  (col, val) of the first NCH chunks     row_chunks_load
//   level 3  the NCH gathers                        row_gather
//
// The clamp min(k, k1 - 1) needs a non-empty row [k0, k1): empty rows leave by
// a row-uniform branch in front of level 2 and nothing outside the row's own
// entries is ever read.  The accumulation follows, lane by lane, the order and
// the accumulators of the loop forms these helpers stand in for (RowPairs:
// csr_row_dot and the Schur rows of k_tau_first; RowQuads: k_spmv_split), with
// a per-lane SELECT of the sum -- s = on ? fma(v, x, s) : s -- never a product
// with a zeroed value (the sign of a zero, a non-finite x).  Rows longer than
// NCH * LPR go on in the loop form itself.
//
// NCH is the number of chunks an AVERAGE row fills: every chunk is loaded and
// gathered whether the lane has it or not, and chunks no row uses cost their
// issue slots (measured: profiles/HISTORY.md, the b family of k_step_one2).
#pragma once

namespace dns {

// (col, val) of chunks 0 .. NCH-1 of this lane, k = k0 + sublane, k0 < k1
template <int LPR, int NCH, typename VT>
__device__ __forceinline__ void row_chunks_load(const int *__restrict__ colidx,
                                                const VT *__restrict__ vals,
                                                int k, int k1, int (&c)[NCH],
                                                VT (&v)[NCH]) {
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
        const int kq = min(k + q * LPR, k1 - 1);
        c[q] = colidx[kq];
        v[q] = vals[kq];
    }
}

// the gathered value of every chunk: `at(c)` loads unconditionally (a split
// input selects the ADDRESS, not the loaded value: one load, no branch)
template <int NCH, typename At>
__device__ __forceinline__ void row_gather(const int (&c)[NCH], At at,
                                           double (&x)[NCH]) {
#pragma unroll
    for (int q = 0; q < NCH; ++q) x[q] = at(c[q]);
}

struct GatherVec {                      // x[c]
    const double *__restrict__ x;
    __device__ __forceinline__ double operator()(int c) const { return x[c]; }
};
struct GatherSplit {                    // c < nv ? a[c] : b[c - nv]
    const double *__restrict__ a, *__restrict__ b;
    int nv;
    __device__ __forceinline__ double operator()(int c) const {
        return *(c < nv ? a + c : b + (c - nv));
    }
};
struct GatherDiff {                     // b[c] - kx[c]
    const double *__restrict__ b, *__restrict__ kx;
    __device__ __forceinline__ double operator()(int c) const {
        return b[c] - kx[c];
    }
};

// two accumulators, chunk q into s[q & 1]: the order of
//   for (; k + LPR < k1; k += 2 LPR) { s0 <- k; s1 <- k + LPR; }
//   if (k < k1) s0 <- k;
struct RowPairs {};
// four accumulators while FOUR chunks are left to the lane, the lane's last
// (up to three) entries one after the other into s0: the order of
//   for (; k + 3 LPR < k1; k += 4 LPR) { s0 .. s3 <- k .. k + 3 LPR; }
//   for (; k < k1; k += LPR) s0 <- k;
struct RowQuads {};

// the lane's part of <A[row, :], x>, row = [k0, k1) NOT empty; the caller
// reduces over the LPR lanes
template <int LPR, int NCH, typename VT, typename At>
__device__ __forceinline__ double row_dot_flat(RowPairs,
                                               const int *__restrict__ colidx,
                                               const VT *__restrict__ vals,
                                               At at, int k0, int k1,
                                               int sublane) {
    static_assert(NCH % 2 == 0, "pairs of chunks");
    int k = k0 + sublane;
    int c[NCH];
    VT v[NCH];
    double x[NCH];
    row_chunks_load<LPR, NCH, VT>(colidx, vals, k, k1, c, v);
    row_gather<NCH>(c, at, x);
    double s[2] = {0.0, 0.0};
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
        const bool on = k + q * LPR < k1;
        const double t = fma((double)v[q], x[q], s[q & 1]);
        s[q & 1] = on ? t : s[q & 1];
    }
    for (k += NCH * LPR; k + LPR < k1; k += 2 * LPR) {
        const int c0 = colidx[k], c1 = colidx[k + LPR];
        const double v0 = (double)vals[k], v1 = (double)vals[k + LPR];
        s[0] = fma(v0, at(c0), s[0]);
        s[1] = fma(v1, at(c1), s[1]);
    }
    if (k < k1) s[0] = fma((double)vals[k], at(colidx[k]), s[0]);
    return s[0] + s[1];
}

template <int LPR, int NCH, typename VT, typename At>
__device__ __forceinline__ double row_dot_flat(RowQuads,
                                               const int *__restrict__ colidx,
                                               const VT *__restrict__ vals,
                                               At at, int k0, int k1,
                                               int sublane) {
    static_assert(NCH == 4, "one group of four chunks");
    int k = k0 + sublane;
    int c[4];
    VT v[4];
    double x[4];
    row_chunks_load<LPR, 4, VT>(colidx, vals, k, k1, c, v);
    row_gather<4>(c, at, x);
    // `full`: the lane enters the four-accumulator loop; otherwise its (up to
    // three) entries go into s0 one after the other
    const bool full = k + 3 * LPR < k1;
    const bool on0 = k < k1, on1 = k + LPR < k1, on2 = k + 2 * LPR < k1;
    const double a0 = fma((double)v[0], x[0], 0.0);
    double s0 = on0 ? a0 : 0.0;
    const double a1 = fma((double)v[1], x[1], full ? 0.0 : s0);
    double s1 = full ? a1 : 0.0;
    s0 = (!full && on1) ? a1 : s0;
    const double a2 = fma((double)v[2], x[2], full ? 0.0 : s0);
    double s2 = full ? a2 : 0.0;
    s0 = (!full && on2) ? a2 : s0;
    const double a3 = fma((double)v[3], x[3], 0.0);
    double s3 = full ? a3 : 0.0;
    // (a lane that was not full has no entry left)
    k = full ? k + 4 * LPR : k1;
    for (; k + 3 * LPR < k1; k += 4 * LPR) {
        const int c0 = colidx[k], c1 = colidx[k + LPR];
        const int c2 = colidx[k + 2 * LPR], c3 = colidx[k + 3 * LPR];
        const double v0 = (double)vals[k], v1 = (double)vals[k + LPR];
        const double v2 = (double)vals[k + 2 * LPR];
        const double v3 = (double)vals[k + 3 * LPR];
        s0 = fma(v0, at(c0), s0);
        s1 = fma(v1, at(c1), s1);
        s2 = fma(v2, at(c2), s2);
        s3 = fma(v3, at(c3), s3);
    }
    for (; k < k1; k += LPR)
        s0 = fma((double)vals[k], at(colidx[k]), s0);
    return (s0 + s1) + (s2 + s3);
}

}  // namespace dns
