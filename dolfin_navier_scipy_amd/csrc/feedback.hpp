// Device-resident observer feedback of the explicit time loops (the
// reference's `dynamic_rhs` built from `get_heunab_lti`, tiu:148-196,
// snu:1237-1247): ONE kernel in front of a time step's first kernel
//   y    = C v_c                                  (C: Ny x NV CSR, sensors)
//   f    = ha hx + hb y + drift(step)             (observer, hN x hN dense)
//   hx_n = hx + 1.5 dt f - 0.5 dt f_last          (AB2)
//   u_n  = hc hx_n                                (Nu inputs)
// -- the observer step, written once below (lti_issue, lti_stage, lti_select,
// lti_observe) -- and then what the inputs drive: k_lti_step
//   geff = g(step) + dt (c_n B u_n + c_c B u_c)   (B: NV x Nu CSR, actuators)
// or k_lti_bc_step, the controlled Dirichlet values (see there).  The front
// kernels of the step then read `geff` where they read `g`.
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
    // state + q stride holds hx (hN), f_last (hN), u_c (Nu) and, in the
    // boundary mode, u_p (Nu): stride = 2 hN + Nu or 2 hN + 2 Nu
    double *state;
    double *ylog, *ulog;                // rows x Ny, rows x Nu
    double dt, c_n, c_c;
    TabRef g;                           // the right-hand side without feedback
    const double *v;                    // current solution (velocity first)
    double *geff;
};

// ---- the observer step ------------------------------------------------------
// Every workgroup computes y, the observer update and u_n redundantly (fixed
// summation orders: all workgroups, and every run, get the same bits) from the
// state slot of the step's parity; only workgroup 0 writes the other slot and
// the log rows.  Nobody waits for another workgroup.  Then each workgroup
// writes its share of what the kernel makes of u_n.
//
// A kernel is a chain of dependent global loads (counter -> row pointers ->
// (col, val) -> v[col] -> ... -> B rows), each a round trip of about a
// microsecond, and little else.  So everything that does not depend on y is
// asked for BEFORE the first barrier, and what depends on nothing before
// anything waits for the counter: both state slots (the parity picks one
// afterwards), ha / hb / hc into LDS (STAGE: they fit kFbStage doubles; else
// they are read where they are used), and -- between lti_issue and lti_stage,
// in the kernel -- the first row pointers of every thread; behind lti_stage
// its first entries of g / gp.  What remains in sequence: counter and row
// pointers of C, its entries, the gather from v, LDS arithmetic, the stores.
constexpr int kFbStage = 4096;

// the LDS of the step (u_p: the boundary mode's), beside the staged matrices
struct LtiLds {
    double y[kFbMaxOut], hx[kFbMaxState], fl[kFbMaxState], f[kFbMaxState],
        hn[kFbMaxState], un[kFbMaxIn], uc[kFbMaxIn], up[kFbMaxIn],
        part[kBlock];
};

// what a thread carries from the early loads to the step
struct LtiRegs {
    int step, row, par;                 // counter (clamped), table row, parity
    double s0, s1, s0b, s1b;            // entries tid, tid + kBlock of the slots
    double dr;                          // drift entry
    const double *haT, *hbT, *hc;       // the matrices: LDS (STAGE) or global
};

// entry k of a state slot to its place in LDS
__device__ __forceinline__ void lti_put(int k, double v, int hN, int Nu,
                                        int stride, LtiLds &sh) {
    if (k < hN) sh.hx[k] = v;
    else if (k < 2 * hN) sh.fl[k - hN] = v;
    else if (k < 2 * hN + Nu) sh.uc[k - 2 * hN] = v;
    else if (k < stride) sh.up[k - 2 * hN - Nu] = v;
}

// sum_k A[r, k] u[k] over the entries [k0, k1) of a row, in storage order
__device__ __forceinline__ double lti_row_dot(const int *__restrict__ ci,
                                              const double *__restrict__ va,
                                              int k0, int k1, const double *u) {
    double acc = 0.0;
    for (int k = k0; k < k1; ++k) acc = fma(va[k], u[ci[k]], acc);
    return acc;
}

// loads that depend on nothing: the counter and both state slots (a slot can
// pass the block size: by up to Nu entries, in the boundary mode 2 Nu)
__device__ __forceinline__ LtiRegs lti_issue(const LtiArgs &a, int stride) {
    const int tid = threadIdx.x;
    LtiRegs o{};
    o.step = *a.stepctr;
    if (tid < stride) {
        o.s0 = a.state[tid];
        o.s1 = a.state[stride + tid];
    }
    if (tid + kBlock < stride) {
        o.s0b = a.state[tid + kBlock];
        o.s1b = a.state[stride + tid + kBlock];
    }
    return o;
}

// ... and ha, hb, hc into LDS
template <bool STAGE>
__device__ __forceinline__ void lti_stage(const LtiArgs &a, LtiRegs &o) {
    o.haT = a.haT;
    o.hbT = a.hbT;
    o.hc = a.hc;
    if constexpr (STAGE) {
        __shared__ double smat[kFbStage];
        const int hN = a.hN;
        const int n1 = hN * hN, n2 = n1 + hN * a.Ny, n3 = n2 + a.Nu * hN;
        for (int k = threadIdx.x; k < n3; k += kBlock)
            smat[k] = k < n1 ? a.haT[k] : k < n2 ? a.hbT[k - n1] : a.hc[k - n2];
        o.haT = smat;
        o.hbT = smat + n1;
        o.hc = smat + n2;
    }
}

// what depends on the counter only: row, parity, the drift entry, and the
// slot of that parity into LDS
__device__ __forceinline__ void lti_select(const LtiArgs &a, int stride,
                                           LtiLds &sh, LtiRegs &o) {
    const int tid = threadIdx.x;
    o.step = o.step < 0 ? 0 : o.step;
    o.row = o.step >= a.rows ? a.rows - 1 : o.step;
    o.par = o.step & 1;
    if (a.drift && tid < a.hN) o.dr = a.drift[(size_t)o.row * a.hN + tid];
    lti_put(tid, o.par ? o.s1 : o.s0, a.hN, a.Nu, stride, sh);
    lti_put(tid + kBlock, o.par ? o.s1b : o.s0b, a.hN, a.Nu, stride, sh);
}

// y, f, hx_n, u_n (left in sh.y, sh.f, sh.hn, sh.un behind the last barrier),
// and workgroup 0's stores of the new slot and the log rows
__device__ __forceinline__ void lti_observe(const LtiArgs &a, int stride,
                                            LtiLds &sh, const LtiRegs &o) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int hN = a.hN, Ny = a.Ny, Nu = a.Nu;
    const double *__restrict__ mhaT = o.haT, *__restrict__ mhbT = o.hbT,
                               *__restrict__ mhc = o.hc;
    // y = C v_c: one wave per sensor row, lanes stride over its entries
    for (int r = wave; r < Ny; r += kBlock / kWave) {
        double acc = 0.0;
        for (int k = a.crp[r] + lane; k < a.crp[r + 1]; k += kWave)
            acc = fma(a.cva[k], a.v[a.cci[k]], acc);
        acc = wave_sum(acc);
        if (lane == 0) sh.y[r] = acc;
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
                acc = fma(mhaT[(size_t)j * hN + i], sh.hx[j], acc);
        sh.part[tid] = acc;
    }
    __syncthreads();
    if (tid < hN) {
        double f = sh.part[tid] + sh.part[tid + kFbMaxState];
        for (int k = 0; k < Ny; ++k)
            f = fma(mhbT[(size_t)k * hN + tid], sh.y[k], f);
        if (a.drift) f += o.dr;
        sh.f[tid] = f;
        sh.hn[tid] = sh.hx[tid] + 1.5 * a.dt * f - 0.5 * a.dt * sh.fl[tid];
    }
    __syncthreads();
    // u_n = hc hx_n: one wave per input
    for (int m = wave; m < Nu; m += kBlock / kWave) {
        double acc = 0.0;
        for (int i = lane; i < hN; i += kWave)
            acc = fma(mhc[(size_t)m * hN + i], sh.hn[i], acc);
        acc = wave_sum(acc);
        if (lane == 0) sh.un[m] = acc;
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        double *__restrict__ nw = a.state + (size_t)(1 - o.par) * stride;
        if (tid < hN) {
            nw[tid] = sh.hn[tid];
            nw[hN + tid] = sh.f[tid];
        }
        if (tid < Nu) {
            nw[2 * hN + tid] = sh.un[tid];
            // (the boundary mode's slot: u_c becomes u_p)
            if (2 * hN + Nu + tid < stride) nw[2 * hN + Nu + tid] = sh.uc[tid];
            a.ulog[(size_t)o.row * Nu + tid] = sh.un[tid];
        }
        if (tid < Ny) a.ylog[(size_t)o.row * Ny + tid] = sh.y[tid];
    }
}

// ---- actuation through the right-hand side ----------------------------------
template <bool STAGE>
__global__ void __launch_bounds__(kBlock) k_lti_step(LtiArgs a) {
    __shared__ LtiLds sh;
    const int stride = 2 * a.hN + a.Nu;
    LtiRegs o = lti_issue(a, stride);
    const int r_first = blockIdx.x * kBlock + threadIdx.x;
    int bk0 = 0, bk1 = 0;
    if (r_first < a.nv) {
        bk0 = a.brp[r_first];
        bk1 = a.brp[r_first + 1];
    }
    lti_stage<STAGE>(a, o);
    const double *__restrict__ g = tab_row(a.g);
    const double g_first = r_first < a.nv ? g[r_first] : 0.0;
    lti_select(a, stride, sh, o);
    lti_observe(a, stride, sh, o);
    // geff = g + dt (c_n B u_n + c_c B u_c); rows of B without entries copy
    for (int r = r_first; r < a.nv; r += gridDim.x * kBlock) {
        const bool first = r == r_first;
        const int k0 = first ? bk0 : a.brp[r], k1 = first ? bk1 : a.brp[r + 1];
        const double sn = lti_row_dot(a.bci, a.bva, k0, k1, sh.un);
        const double sc = lti_row_dot(a.bci, a.bva, k0, k1, sh.uc);
        a.geff[r] = (first ? g_first : g[r]) + a.dt * (a.c_n * sn + a.c_c * sc);
    }
}

// ---- boundary actuation -----------------------------------------------------
// The observer's output drives the controlled Dirichlet values (the reference's
// `diricontfuncs` read the state): behind the same y, f, hx_n, u_n
//   b(s + 1) = base + S u_n                        (S: nc x Nu CSR)
// goes into the controlled columns of row s + 1 of the convection operator's
// Dirichlet table -- the front convection of this step reads row s, the tail's
// convection of the new state row s + 1, both later in the stream -- and what
// the boundary terms of the right-hand sides have that is linear in u is added
// to the rows the host tabulated with u = 0:
//   geff  = g(s) + sum_{j = n, c, p} (wm_j Bm + wa_j Ba) u_j
//                + dt (c_n B u_n + c_c B u_c)      (B optional)
//   gpeff = gp(s) + Bj u_n
// (Ba, Bm: NV x Nu, Bj: NP x Nu: `applybcs` of the unit controls; u_p, the
// output two times back, is SBDF2's.)  The state slot holds hx, f_last, u_c,
// u_p: 2 hN + 2 Nu entries.
struct LtiBcArgs {
    LtiArgs l;                          // brp null: no B; geff null: no
                                        // right-hand-side terms at all
    int np, nc;
    const int *srp, *sci;
    const double *sva, *base;
    double *dbc;                        // the table's controlled columns, row 0
    int dbc_stride, dbc_rows;
    const int *arp, *aci;               // Ba, Bm, Bj (all null: literal zero)
    const double *ava;
    const int *mrp, *mci;
    const double *mva;
    const int *jrp, *jci;
    const double *jva;
    double wm_n, wm_c, wm_p, wa_n, wa_c, wa_p;
    TabRef gp;
    double *gpeff;
};

// The observer step, then each workgroup writes its entries of the Dirichlet
// row and its rows of geff and gpeff.
template <bool STAGE>
__global__ void __launch_bounds__(kBlock) k_lti_bc_step(LtiBcArgs b) {
    const LtiArgs &a = b.l;
    __shared__ LtiLds sh;
    const int stride = 2 * a.hN + 2 * a.Nu;     // <= 2 kBlock
    LtiRegs o = lti_issue(a, stride);
    const int r_first = blockIdx.x * kBlock + threadIdx.x;
    const bool rhs_v = a.geff != nullptr, rhs_p = b.gpeff != nullptr;
    const bool has_b = a.brp != nullptr, has_m = b.mrp != nullptr;
    int bk0 = 0, bk1 = 0, mk0 = 0, mk1 = 0, ak0 = 0, ak1 = 0, jk0 = 0, jk1 = 0;
    if (rhs_v && r_first < a.nv) {
        if (has_b) {
            bk0 = a.brp[r_first];
            bk1 = a.brp[r_first + 1];
        }
        if (has_m) {
            mk0 = b.mrp[r_first];
            mk1 = b.mrp[r_first + 1];
            ak0 = b.arp[r_first];
            ak1 = b.arp[r_first + 1];
        }
    }
    if (rhs_p && r_first < b.np) {
        jk0 = b.jrp[r_first];
        jk1 = b.jrp[r_first + 1];
    }
    int sk0 = 0, sk1 = 0;
    if (r_first < b.nc) {
        sk0 = b.srp[r_first];
        sk1 = b.srp[r_first + 1];
    }
    lti_stage<STAGE>(a, o);
    const double *__restrict__ g = rhs_v ? tab_row(a.g) : nullptr;
    const double *__restrict__ gp = rhs_p ? tab_row(b.gp) : nullptr;
    const double g_first = rhs_v && r_first < a.nv ? g[r_first] : 0.0;
    const double gp_first = rhs_p && r_first < b.np ? gp[r_first] : 0.0;
    lti_select(a, stride, sh, o);
    lti_observe(a, stride, sh, o);
    const double *sun = sh.un, *suc = sh.uc, *sup = sh.up;
    // the Dirichlet values of the state this step leaves: row step + 1
    if (o.step + 1 < b.dbc_rows) {
        double *__restrict__ drow = b.dbc + (size_t)(o.step + 1) * b.dbc_stride;
        for (int i = r_first; i < b.nc; i += gridDim.x * kBlock) {
            const bool first = i == r_first;
            const int k0 = first ? sk0 : b.srp[i], k1 = first ? sk1 : b.srp[i + 1];
            drow[i] = b.base[i] + lti_row_dot(b.sci, b.sva, k0, k1, sun);
        }
    }
    // geff: rows without entries copy g
    if (rhs_v)
        for (int r = r_first; r < a.nv; r += gridDim.x * kBlock) {
            const bool first = r == r_first;
            double add = 0.0;
            if (has_m) {
                const int m0 = first ? mk0 : b.mrp[r];
                const int m1 = first ? mk1 : b.mrp[r + 1];
                const int a0 = first ? ak0 : b.arp[r];
                const int a1 = first ? ak1 : b.arp[r + 1];
                const double mn = lti_row_dot(b.mci, b.mva, m0, m1, sun);
                const double mc = lti_row_dot(b.mci, b.mva, m0, m1, suc);
                const double mp = lti_row_dot(b.mci, b.mva, m0, m1, sup);
                const double an = lti_row_dot(b.aci, b.ava, a0, a1, sun);
                const double ac = lti_row_dot(b.aci, b.ava, a0, a1, suc);
                const double ap = lti_row_dot(b.aci, b.ava, a0, a1, sup);
                add = b.wm_n * mn + b.wm_c * mc + b.wm_p * mp + b.wa_n * an +
                      b.wa_c * ac + b.wa_p * ap;
            }
            if (has_b) {
                const int k0 = first ? bk0 : a.brp[r];
                const int k1 = first ? bk1 : a.brp[r + 1];
                const double sn = lti_row_dot(a.bci, a.bva, k0, k1, sun);
                const double sc = lti_row_dot(a.bci, a.bva, k0, k1, suc);
                add += a.dt * (a.c_n * sn + a.c_c * sc);
            }
            a.geff[r] = (first ? g_first : g[r]) + add;
        }
    if (rhs_p)
        for (int r = r_first; r < b.np; r += gridDim.x * kBlock) {
            const bool first = r == r_first;
            const int k0 = first ? jk0 : b.jrp[r], k1 = first ? jk1 : b.jrp[r + 1];
            b.gpeff[r] = (first ? gp_first : gp[r]) +
                         lti_row_dot(b.jci, b.jva, k0, k1, sun);
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
