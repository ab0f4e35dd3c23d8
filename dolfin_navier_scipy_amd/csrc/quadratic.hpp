// Device-resident quadratic functionals of the explicit time loops (kinetic
// energy, dissipation rate, the rate u^T M du/dt, the M-norm of du/dt): ONE
// kernel in front of a time step's first kernel (the last of the front nodes,
// behind k_stats_step, and once more behind the last step of a call)
// evaluates, for k < nQ, with v = xs[cur][:nv], w = v - xs[prev][:nv] and the
// operands a_0 = v, a_1 = w,
//   y_k = scale_k * ( dt^-(l_k + r_k) * a_{l_k}^T Q_{m_k} a_{r_k}
//                     + qa_k . v + (qw_k . w) / dt + c0_k )
// over nM <= 4 general (not symmetric) sparse matrices Q_m, nv x nv, and
// writes it into row `counter - 1` of a log in HBM -- the row convention of
// k_functional_step: row r is the value of what dns_imex_get_state would have
// returned after the (r+1)-th step.  Forms that share a matrix share ONE pass
// over it: per matrix the products s0 = Q v and / or s1 = Q w are formed, as
// some form on it needs them.
//
// Moving Dirichlet values (QdBcArgs): the forms stand on the full space,
// n = nv + ndbc rows and columns per matrix in the order [inner dofs;
// Dirichlet dofs], the operands are a_0 = u = [v; g] and a_1 = d = [v - v_prev;
// g - g_prev] with g, g_prev rows `counter`, `counter - 1` of a table of the
// Dirichlet values (row j: the values of the state before step j, the row
// convention of FnBcArgs) -- the stepper's own copy or the convection
// operator's live table, which k_lti_bc_step writes.
//
// No workgroup waits for another and nothing is added atomically: workgroup g
// writes its share of y_k to log[row][g][k] in a fixed order, the getter sums
// g in index order -- the same bits in every run, launched or replayed.
#pragma once
#include <type_traits>

#include "kernels.hpp"

namespace dns {

constexpr int kQdMaxMats = 4;       // matrices of a stepper
constexpr int kQdMaxForms = 8;      // forms over them
constexpr int kQdMaxGrid = 256;     // workgroups (beyond it they stride)
constexpr int kQdLanes = 16;        // lanes of a row
constexpr int kQdUnroll = 4;        // entries of a row a lane has in flight
constexpr int kQdRows = kBlock / kQdLanes;   // rows of a workgroup per pass

struct QdArgs {
    const int *stepctr;                 // device step counter
    int nrows;                          // rows of the log
    const double *x, *xp;               // xs[cur], xs[prev]
    int nv;
    double dt;
    int nM, nQ, G;                      // G: the grid the log is laid out for
    // the matrices one behind the other: row pointers nM x (nv + 1), each
    // counting from its matrix's first entry, which is entry nzbase[m] of
    // ci / va
    const int *rp, *ci;
    const double *va;
    long long nzbase[kQdMaxMats];
    // two bits per matrix (m: bits 2 m, 2 m + 1): some form needs Q v / Q w
    unsigned need;
    // four bits per form (k: from bit 4 k): matrix (two bits), left operand,
    // right operand (0: v, 1: w)
    unsigned forms;
    // the sparse rows: row 2 k is qa_k (over v), row 2 k + 1 is qw_k (over w)
    const int *lrp, *lci;
    const double *lva;
    const double *scale, *c0;
    double *log;                        // nrows x G x nQ
};

// Moving Dirichlet values: `gtab` holds `trows` rows of `ndbc` values each
// (one behind the other); in the prologue of step s (counter s) the state is
// the one before step s: its values are row s, those of the state before it row
// s - 1; the closing launch reads row nrows (trows >= nrows + 1).  Matrices and
// sparse rows are nv + ndbc wide, the row pointers nM x (nv + ndbc + 1).  The
// kernel is instantiated per argument type, so the instance for constant
// values takes QdArgs as it stands.
struct QdBcArgs : QdArgs {
    const double *gtab;
    int ndbc;
    int trows;
};

// passes over one matrix: kQdRows rows each, so that a pass never holds rows
// of two matrices (what it forms is uniform over the workgroup)
inline unsigned quadratic_form_bits(int mat, int lop, int rop) {
    return (unsigned)mat | (unsigned)lop << 2 | (unsigned)rop << 3;
}

// (`n`: the rows of a matrix, nv or nv + ndbc)
inline int quadratic_passes(int n) { return (n + kQdRows - 1) / kQdRows; }

// enough workgroups for one pass each, capped (`max_grid` > 0: lower)
inline int quadratic_grid(int nM, int n, int max_grid) {
    int g = std::min(nM * quadratic_passes(n), kQdMaxGrid);
    if (max_grid > 0) g = std::min(g, max_grid);
    return std::max(1, g);
}

// Matrix part, matrix by matrix: kQdLanes lanes per row, the workgroups stride
// over the passes (kQdRows rows of ONE matrix, numbered through all of them);
// a lane has kQdUnroll entries in flight -- their (column, value) loads go out
// together, then the gathers, then the products in the order of the plain
// loop --, the lanes of a row are summed by xor shuffles and the row's first
// lane adds a_l[i] * s_r to the matrix's four accumulators (l, r).  Behind a
// matrix they are summed over the wave by xor shuffles and put down in LDS;
// ONE thread per form adds the four waves' sums of its (m, l, r) in wave
// order.  Sparse rows: one wave per row, the waves of the whole grid stride
// over the 2 nQ rows, wave_sum (k_functional_step's).
//
// Constant Dirichlet values (ARGS = QdArgs): NOTHING the kernel loads depends
// on the counter: it is asked for first and looked at last, where it gives the
// row to store to (or none: the launch in front of the first step after the
// forms were set, whose sums are dropped).  Moving ones (QdBcArgs): the counter
// selects the two table rows, clamped to [0, trows - 1] (the launch in front of
// the first step takes row 0 twice and drops its sums): every address is valid
// whatever the counter says.  Only the gathers from the table wait for it: a
// column c goes to x / xp with the index c < nv ? c : 0 -- a load that does not
// know the counter, issued as in the constant instance -- and, right behind
// it and without a branch, to the table with the index c < nv ? 0 : c - nv;
// the value is selected once both are there, so no column pays a second,
// dependent round trip.  The row pointers, the matrix stream and the inner
// left operands do not depend on the counter either.
// The divisions by dt happen once per form, on the workgroup's share.
template <typename ARGS>
__global__ void __launch_bounds__(kBlock) k_quadratic_step(ARGS a) {
    constexpr bool kBc = std::is_same<ARGS, QdBcArgs>::value;
    constexpr int kWaves = kBlock / kWave;
    __shared__ double rowsum[2 * kQdMaxForms];
    __shared__ double red[kQdMaxMats * 4 * kWaves];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int g = blockIdx.x, G = a.G;
    const int step = *a.stepctr;
    const int grp = tid / kQdLanes, sub = tid % kQdLanes;
    const int nv = a.nv;
    // (n: rows and columns of a matrix)
    int n = nv;
    const double *gc = nullptr, *gp = nullptr;
    if constexpr (kBc) {
        n = nv + a.ndbc;
        const int r1 = min(max(step, 0), a.trows - 1);
        const int r0 = min(max(step - 1, 0), a.trows - 1);
        gc = a.gtab + (size_t)r1 * a.ndbc;
        gp = a.gtab + (size_t)r0 * a.ndbc;
    }
    double sc = 0.0, c0 = 0.0;
    if (tid < a.nQ) {
        sc = a.scale[tid];
        c0 = a.c0[tid];
    }
    // ---- matrices ----
    const int ppm = (n + kQdRows - 1) / kQdRows;
    for (int m = 0; m < a.nM; ++m) {
        long long base = a.nzbase[0];
#pragma unroll
        for (int q = 1; q < kQdMaxMats; ++q)
            base = m == q ? a.nzbase[q] : base;
        const int *__restrict__ ci = a.ci + base;
        const double *__restrict__ va = a.va + base;
        const int *__restrict__ rpm = a.rp + (size_t)m * (n + 1);
        const unsigned need = a.need >> (2 * m);
        const bool n0 = need & 1, n1 = need & 2;
        // (pass j of matrix m is pass m * ppm + j of the grid's stride)
        const int first = ((g - m * ppm) % G + G) % G;
        double avv = 0.0, avw = 0.0, awv = 0.0, aww = 0.0;
        for (int pass = first; pass < ppm; pass += G) {
            const int i = pass * kQdRows + grp;
            const bool live = i < n;
            int k0 = 0, k1 = 0;
            double vi = 0.0, vpi = 0.0;
            if constexpr (kBc) {
                if (live) {
                    k0 = rpm[i];
                    k1 = rpm[i + 1];
                    if (i < nv) {
                        vi = a.x[i];
                        vpi = a.xp[i];
                    } else {
                        vi = gc[i - nv];
                        vpi = gp[i - nv];
                    }
                }
            } else if (live) {
                k0 = rpm[i];
                k1 = rpm[i + 1];
                vi = a.x[i];
                vpi = a.xp[i];
            }
            double s0 = 0.0, s1 = 0.0;
            for (int k = k0 + sub; k < k1; k += kQdUnroll * kQdLanes) {
                int c[kQdUnroll];
                double q[kQdUnroll], xv[kQdUnroll], xw[kQdUnroll];
#pragma unroll
                for (int j = 0; j < kQdUnroll; ++j) {
                    const int kk = k + j * kQdLanes;
                    c[j] = kk < k1 ? ci[kk] : 0;
                    q[j] = kk < k1 ? va[kk] : 0.0;
                }
                if constexpr (kBc) {
                    // inner part first (an index of its own for the boundary
                    // columns: no load of x / xp knows the table rows)
                    // (the table's values land in registers of their own:
                    // their loads go out behind the inner ones without
                    // waiting for them)
                    double xq[kQdUnroll], gv[kQdUnroll], gq[kQdUnroll];
#pragma unroll
                    for (int j = 0; j < kQdUnroll; ++j) {
                        const int cx = c[j] < nv ? c[j] : 0;
                        xv[j] = a.x[cx];
                        xq[j] = n1 ? a.xp[cx] : 0.0;
                    }
#pragma unroll
                    for (int j = 0; j < kQdUnroll; ++j) {
                        // (no branch: an inner column reads entry 0, one
                        // line for all of them)
                        const int cg = c[j] < nv ? 0 : c[j] - nv;
                        gv[j] = gc[cg];
                        gq[j] = n1 ? gp[cg] : 0.0;
                    }
#pragma unroll
                    for (int j = 0; j < kQdUnroll; ++j) {
                        const bool in = c[j] < nv;
                        xv[j] = in ? xv[j] : gv[j];
                        xw[j] = n1 ? xv[j] - (in ? xq[j] : gq[j]) : 0.0;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < kQdUnroll; ++j) {
                        xv[j] = a.x[c[j]];
                        xw[j] = n1 ? xv[j] - a.xp[c[j]] : 0.0;
                    }
                }
#pragma unroll
                for (int j = 0; j < kQdUnroll; ++j) {
                    const bool in = k + j * kQdLanes < k1;
                    if (n0) s0 = in ? fma(q[j], xv[j], s0) : s0;
                    if (n1) s1 = in ? fma(q[j], xw[j], s1) : s1;
                }
            }
            s0 = subwave_sum<kQdLanes>(s0);
            s1 = subwave_sum<kQdLanes>(s1);
            if (sub == 0 && live) {
                const double wi = vi - vpi;
                avv = fma(vi, s0, avv);
                avw = fma(vi, s1, avw);
                awv = fma(wi, s0, awv);
                aww = fma(wi, s1, aww);
            }
        }
        avv = wave_sum(avv);
        avw = wave_sum(avw);
        awv = wave_sum(awv);
        aww = wave_sum(aww);
        if (lane == 0) {
            // (l, r) at 2 l + r
            double *out = red + (size_t)m * 4 * kWaves + wave;
            out[0] = avv;
            out[kWaves] = avw;
            out[2 * kWaves] = awv;
            out[3 * kWaves] = aww;
        }
    }
    // ---- sparse rows ----
    const int nT = 2 * a.nQ;
    for (int t = g * kWaves + wave; t < nT; t += G * kWaves) {
        const int k0 = a.lrp[t], k1 = a.lrp[t + 1];
        const bool diff = t & 1;
        double s = 0.0;
        for (int k = k0 + lane; k < k1; k += kQdUnroll * kWave) {
            int c[kQdUnroll];
            double q[kQdUnroll], xv[kQdUnroll];
#pragma unroll
            for (int j = 0; j < kQdUnroll; ++j) {
                const int kk = k + j * kWave;
                c[j] = kk < k1 ? a.lci[kk] : 0;
                q[j] = kk < k1 ? a.lva[kk] : 0.0;
            }
            if constexpr (kBc) {
#pragma unroll
                for (int j = 0; j < kQdUnroll; ++j) {
                    // (as in the matrix part: x / xp with an index that does
                    // not know the table, the table's entry beside it)
                    const bool in = c[j] < nv;
                    const int cx = in ? c[j] : 0, cg = in ? 0 : c[j] - nv;
                    const double xi = diff ? a.x[cx] - a.xp[cx] : a.x[cx];
                    const double gi = diff ? gc[cg] - gp[cg] : gc[cg];
                    xv[j] = in ? xi : gi;
                }
            } else {
#pragma unroll
                for (int j = 0; j < kQdUnroll; ++j)
                    xv[j] = diff ? a.x[c[j]] - a.xp[c[j]] : a.x[c[j]];
            }
#pragma unroll
            for (int j = 0; j < kQdUnroll; ++j)
                s = k + j * kWave < k1 ? fma(q[j], xv[j], s) : s;
        }
        s = wave_sum(s);
        if (lane == 0) rowsum[t] = s;
    }
    __syncthreads();
    // ---- this workgroup's share of y_k ----
    const int row = step - 1;
    if (tid < a.nQ && row >= 0 && row < a.nrows) {
        const unsigned f = a.forms >> (4 * tid);
        const int lo = f >> 2 & 1, ro = f >> 3 & 1, p = lo + ro;
        const double *mine = red + ((f & 3) * 4 + 2 * lo + ro) * kWaves;
        double tot = 0.0;
        for (int w = 0; w < kWaves; ++w) tot += mine[w];
        if (p >= 1) tot /= a.dt;
        if (p == 2) tot /= a.dt;
        // (row t was summed here if the wave (t mod G * kWaves) is one of ours)
        const int t0 = 2 * tid;
        if ((t0 / kWaves) % G == g) tot += rowsum[t0];
        if (((t0 + 1) / kWaves) % G == g) tot += rowsum[t0 + 1] / a.dt;
        if (g == 0) tot += c0;
        a.log[((size_t)row * G + g) * a.nQ + tid] = sc * tot;
    }
}

}  // namespace dns
