// The front of a resident IMEX time step in the latency regime (n ~ 1e4), cut
// along its data dependencies instead of along its operations:
//
//   k_step_front : [convection element kernel]  ||  [x0 = extrapolation,
//                  kx = K x0, rs = R1 (a_c v_c + a_p v_p)]      -- ONE launch:
//                  the first workgroups evaluate the cells, the others walk
//                  the rows; neither half needs the other (both read v_c only)
//   k_step_back  : nfc_c = scale * gather(cell values);  b = rs + cn_c nfc_c +
//                  cn_o nfc_o + g;  r = b - kx;  partials of ||r||^2, ||b||^2
//
// Before (k_conv_cells -> one prologue kernel) the three gather chains of the
// prologue -- 12.2 us of the ~53 us step -- waited for the 5.8 us element
// kernel although only the (short) convection gather depends on it.
#pragma once
#include "convection.hpp"
#include "gmres_kernels.hpp"
#include "kernels.hpp"

namespace dns {

// MODE 0: x0 = extrapolation of up to five ring vectors, gathered per entry
// MODE 1 (PRE): the warm start x0 has been written into `x0` by the previous
//   step's tail kernel (TailExtrap): the K chain gathers that ONE vector (x0
//   is not stored again)
// MODE 2 (PRE + residual carry-over): the K chain gathers the CURRENT solution
//   x_c instead; K x_c is kept per ring slot (`cr.kx_c`), so that
//     K x0 = e_c K x_c + e_p K x_p + ...          (row-local, no gather) and
//     r_c  = b_prev - K x_c                       (the TRUE residual of the
//                                                  previous step's solve)
//   cost nothing beyond a few row-local loads.  The velocity part of r_c
//   (weighted like the state it belongs to: a_c r_c + a_p r_p) is added to
//   this step's right-hand side.  A Krylov solve stopped after one step leaves
//   an error delta = K^-1 r of the same sign step after step, which the next
//   step propagates as R1 delta_v = r_v - JT delta_p - theta dt A delta_v:
//   carrying r_v cancels the leading term, what is left of a step's error in
//   the NEXT state is K^-1 [theta dt A delta_v; 0] (small for the smooth
//   components that would add up) -- the distance to the direct-solve
//   trajectory stops growing with the number of steps
//   (scripts/carry_over_model.py: 10-20x at 800 steps of the wake at Re = 100).
struct CarryRef {
    double *kx_c;                       // out: K x_c (ring slot of x_c)
    const double *kx_p, *kx_pp, *kx_p3, *kx_p4;
    double *rprev;                      // in: r of the step before, out: r_c
};

template <int LPR, int MODE>
__global__ void __launch_bounds__(kBlock)
k_step_front(int nconv_blocks,
             // --- convection half
             int ncells, const int *__restrict__ cellmap,
             const double *__restrict__ glam, const double *__restrict__ area,
             TabRef dbctab, double *__restrict__ cellvals,
             // --- row half
             int n, int nv, const int *__restrict__ k_rowptr,
             const int *__restrict__ k_colidx,
             const double *__restrict__ k_vals,
             const int *__restrict__ r_rowptr,
             const int *__restrict__ r_colidx,
             const double *__restrict__ r_vals,
             const double *__restrict__ x_c, const double *__restrict__ x_p,
             const double *__restrict__ x_pp, const double *__restrict__ x_p3,
             const double *__restrict__ x_p4, double e_c, double e_p,
             double e_pp, double e_p3, double e_p4, double a_c, double a_p,
             double *x0, double *__restrict__ kx, double *rs, CarryRef cr) {
    constexpr bool PRE = MODE == 1;
    constexpr bool CARRY = MODE == 2;
    if ((int)blockIdx.x < nconv_blocks) {
        if (ncells > 0)
            conv_cells_block(blockIdx.x, ncells, cellmap, glam, area,
                             ConvFromVec{x_c}, dbctab, cellvals);
        return;
    }
    const int rb = blockIdx.x - nconv_blocks;
    const int nrb = gridDim.x - nconv_blocks;
    const int sub = (rb * kBlock + threadIdx.x) / LPR;
    const int sublane = threadIdx.x % LPR;
    const int nsub = nrb * (kBlock / LPR);
    for (int row = sub; row < n; row += nsub) {
        // two independent gather chains, first pass issued level by level
        const bool isv = row < nv;
        int kk = k_rowptr[row] + sublane;
        const int kend = k_rowptr[row + 1];
        int rk = 0, rend = 0;
        if (isv) {
            rk = r_rowptr[row] + sublane;
            rend = r_rowptr[row + 1];
        }
        const bool k_on = kk < kend, r_on = rk < rend;
        int kc = 0, rc = 0;
        double kval = 0.0, rval = 0.0;
        if (k_on) {
            kc = k_colidx[kk];
            kval = k_vals[kk];
        }
        if (r_on) {
            rc = r_colidx[rk];
            rval = r_vals[rk];
        }
        // carry-over: the row's own entries of the ring of K x products, of the
        // previous right-hand side and of the previous residual (none of them
        // depends on the gathers: they go out with the first pass)
        double h_p = 0.0, h_pp = 0.0, h_p3 = 0.0, h_p4 = 0.0, b_old = 0.0,
               r_old = 0.0;
        if (CARRY && sublane == 0) {
            if (e_p != 0.0) h_p = cr.kx_p[row];
            if (e_pp != 0.0) h_pp = cr.kx_pp[row];
            if (e_p3 != 0.0) h_p3 = cr.kx_p3[row];
            if (e_p4 != 0.0) h_p4 = cr.kx_p4[row];
            if (isv) b_old = rs[row];   // (the step before left its b here)
            if (isv && a_p != 0.0) r_old = cr.rprev[row];
        }
        double ks = 0.0, rsum = 0.0;
        if (k_on && PRE) {
            ks = kval * x0[kc];
        } else if (k_on && CARRY) {
            ks = kval * x_c[kc];
        } else if (k_on) {
            double xv = e_c * x_c[kc];
            if (e_p != 0.0) xv = fma(e_p, x_p[kc], xv);
            if (e_pp != 0.0) xv = fma(e_pp, x_pp[kc], xv);
            if (e_p3 != 0.0) xv = fma(e_p3, x_p3[kc], xv);
            if (e_p4 != 0.0) xv = fma(e_p4, x_p4[kc], xv);
            ks = kval * xv;
        }
        if (r_on) {
            double vv = a_c * x_c[rc];
            if (a_p != 0.0) vv = fma(a_p, x_p[rc], vv);
            rsum = rval * vv;
        }
        for (kk += LPR; kk < kend; kk += LPR) {
            const int c = k_colidx[kk];
            if (PRE) {
                ks = fma(k_vals[kk], x0[c], ks);
                continue;
            }
            if (CARRY) {
                ks = fma(k_vals[kk], x_c[c], ks);
                continue;
            }
            double xv = e_c * x_c[c];
            if (e_p != 0.0) xv = fma(e_p, x_p[c], xv);
            if (e_pp != 0.0) xv = fma(e_pp, x_pp[c], xv);
            if (e_p3 != 0.0) xv = fma(e_p3, x_p3[c], xv);
            if (e_p4 != 0.0) xv = fma(e_p4, x_p4[c], xv);
            ks = fma(k_vals[kk], xv, ks);
        }
        for (rk += LPR; rk < rend; rk += LPR) {
            const int c = r_colidx[rk];
            double vv = a_c * x_c[c];
            if (a_p != 0.0) vv = fma(a_p, x_p[c], vv);
            rsum = fma(r_vals[rk], vv, rsum);
        }
        ks = subwave_sum<LPR>(ks);
        rsum = subwave_sum<LPR>(rsum);
        if (sublane == 0) {
            if (MODE == 0) {
                double xv = e_c * x_c[row];
                if (e_p != 0.0) xv = fma(e_p, x_p[row], xv);
                if (e_pp != 0.0) xv = fma(e_pp, x_pp[row], xv);
                if (e_p3 != 0.0) xv = fma(e_p3, x_p3[row], xv);
                if (e_p4 != 0.0) xv = fma(e_p4, x_p4[row], xv);
                x0[row] = xv;
            }
            if (CARRY) {
                cr.kx_c[row] = ks;                   // K x_c, kept
                double k0 = e_c * ks;                // K x0 by linearity
                k0 = fma(e_p, h_p, k0);
                k0 = fma(e_pp, h_pp, k0);
                k0 = fma(e_p3, h_p3, k0);
                k0 = fma(e_p4, h_p4, k0);
                kx[row] = k0;
                if (isv) {
                    const double r_c = b_old - ks;   // true residual, step k-1
                    cr.rprev[row] = r_c;
                    rs[row] = rsum + fma(a_c, r_c, a_p * r_old);
                }
            } else {
                kx[row] = ks;
                if (isv) rs[row] = rsum;
            }
        }
    }
}

// LPR lanes per row (the convection list of a velocity dof has ~6-12 entries)
template <int LPR>
__global__ void __launch_bounds__(kBlock)
k_step_back(int n, int nv, double *__restrict__ nfc_c,
            const double *__restrict__ nfc_o, double cn_c, double cn_o,
            TabRef gtab, TabRef gptab, const int *__restrict__ gptr,
            const int *__restrict__ gidx, const double *__restrict__ cellvals,
            double conv_scale, double *__restrict__ b /* in: rs */,
            double *__restrict__ r /* in: kx */, double *__restrict__ part_rr,
            double *__restrict__ part_bb) {
    __shared__ double red[4];
    const double *__restrict__ g = tab_row(gtab);
    const double *__restrict__ gp = tab_row(gptab);
    const int sub = (blockIdx.x * kBlock + threadIdx.x) / LPR;
    const int sublane = threadIdx.x % LPR;
    const int nsub = gridDim.x * (kBlock / LPR);
    double arr = 0.0, abb = 0.0;
    for (int row = sub; row < n; row += nsub) {
        double cvs = 0.0;
        const bool isv = row < nv;
        // the row's own entries go out before the (three loads deep) gather
        // chain of the convection: none of them depends on it
        double b_in = 0.0, r_in = 0.0, no_in = 0.0, g_in = 0.0, nc_in = 0.0;
        if (sublane == 0) {
            r_in = r[row];
            if (isv) {
                b_in = b[row];
                no_in = nfc_o[row];
                g_in = g[row];
                if (!gptr) nc_in = nfc_c[row];
            } else {
                g_in = gp[row - nv];
            }
        }
        if (isv && gptr) {
            const int gend = gptr[row + 1];
            for (int k = gptr[row] + sublane; k < gend; k += LPR)
                cvs += cellvals[gidx[k]];
        }
        cvs = subwave_sum<LPR>(cvs);
        if (sublane == 0) {
            double bv;
            if (isv) {
                const double nc = gptr ? conv_scale * cvs : nc_in;
                if (gptr) nfc_c[row] = nc;
                bv = b_in + cn_c * nc + cn_o * no_in + g_in;
            } else {
                bv = g_in;
            }
            const double rv = bv - r_in;
            b[row] = bv;
            r[row] = rv;
            arr = fma(rv, rv, arr);
            abb = fma(bv, bv, abb);
        }
    }
    arr = block_sum(arr, red);
    abb = block_sum(abb, red);
    if (threadIdx.x == 0) {
        part_rr[blockIdx.x] = arr;
        part_bb[blockIdx.x] = abb;
    }
}

// ---------------------------------------------------------------------------
// The six-node step (round 3): front and back merged, the convection cells
// moved into the TAIL of the step before.
//
//   k_step_one  : per row THREE independent gather chains in one launch --
//                 kx = K x0 (x0: the warm start the previous tail left),
//                 rs = R1 (a_c v_c + a_p v_p), nfc_c = scale * gather of the
//                 cell values (computed by the previous step's tail) -- then
//                 b = rs + cn_c nfc_c + cn_o nfc_o + g [+ carried residuals],
//                 r = b - kx, partials of ||r||^2, ||b||^2.
//   k_arn_tail6 : k_arn_tail_acc (close the last column, y = R^-1 g,
//                 x_new = x0 + Z y OUT OF PLACE, next warm start) plus
//                 * the true residual of this solve by linearity,
//                   r_new = r0 - sum_j y_j W_j  (W_j = K z_j kept per column),
//                   velocity rows -> the carry-over buffer;
//                 * in extra workgroups the convection cells of the NEW
//                   velocity, each value taken from its definition
//                   x0[m] + sum_j y_j Z_j[m] (the new solution vector is being
//                   written by other workgroups of this launch: it is never
//                   read here, x0 and Z are not written).
//
// Everything a step needs from the step before is complete when the step's
// first kernel starts; nothing is recurred (K x0 and the W_j are exact gathers
// every step), so no rounding error builds up along the run.
// ---------------------------------------------------------------------------
template <int LPR>
__global__ void __launch_bounds__(kBlock)
k_step_one(int n, int nv, const int *__restrict__ k_rowptr,
           const int *__restrict__ k_colidx, const double *__restrict__ k_vals,
           const int *__restrict__ r_rowptr, const int *__restrict__ r_colidx,
           const double *__restrict__ r_vals, const double *__restrict__ x0,
           const double *__restrict__ x_c, const double *__restrict__ x_p,
           double a_c, double a_p, double *__restrict__ nfc_c,
           const double *__restrict__ nfc_o, double cn_c, double cn_o,
           TabRef gtab, TabRef gptab, const int *__restrict__ gptr,
           const int *__restrict__ gidx, const double *__restrict__ cellvals,
           double conv_scale, const double *__restrict__ rc_c,
           const double *__restrict__ rc_p, double *__restrict__ b,
           double *__restrict__ r, double *__restrict__ part_rr,
           double *__restrict__ part_bb) {
    __shared__ double red[4];
    const double *__restrict__ g = tab_row(gtab);
    const double *__restrict__ gp = tab_row(gptab);
    const int sub = (blockIdx.x * kBlock + threadIdx.x) / LPR;
    const int sublane = threadIdx.x % LPR;
    const int nsub = gridDim.x * (kBlock / LPR);
    double arr = 0.0, abb = 0.0;
    for (int row = sub; row < n; row += nsub) {
        const bool isv = row < nv;
        // first pass of the three chains, level by level
        int kk = k_rowptr[row] + sublane;
        const int kend = k_rowptr[row + 1];
        int rk = 0, rend = 0, ck = 0, cend = 0;
        if (isv) {
            rk = r_rowptr[row] + sublane;
            rend = r_rowptr[row + 1];
            if (gptr) {
                ck = gptr[row] + sublane;
                cend = gptr[row + 1];
            }
        }
        const bool k_on = kk < kend, r_on = rk < rend, c_on = ck < cend;
        int kc = 0, rc = 0, ci = 0;
        double kval = 0.0, rval = 0.0;
        if (k_on) {
            kc = k_colidx[kk];
            kval = k_vals[kk];
        }
        if (r_on) {
            rc = r_colidx[rk];
            rval = r_vals[rk];
        }
        if (c_on) ci = gidx[ck];
        // the row's own entries: none depends on the gathers
        double no_in = 0.0, g_in = 0.0, nc_in = 0.0, car = 0.0;
        if (sublane == 0) {
            if (isv) {
                no_in = nfc_o[row];
                g_in = g[row];
                if (!gptr) nc_in = nfc_c[row];
                if (rc_c) car = a_c * rc_c[row];
                if (rc_p && a_p != 0.0) car = fma(a_p, rc_p[row], car);
            } else {
                g_in = gp[row - nv];
            }
        }
        double ks = k_on ? kval * x0[kc] : 0.0;
        double rsum = 0.0, cvs = 0.0;
        if (r_on) {
            double vv = a_c * x_c[rc];
            if (a_p != 0.0) vv = fma(a_p, x_p[rc], vv);
            rsum = rval * vv;
        }
        if (c_on) cvs = cellvals[ci];
        for (kk += LPR; kk < kend; kk += LPR)
            ks = fma(k_vals[kk], x0[k_colidx[kk]], ks);
        for (rk += LPR; rk < rend; rk += LPR) {
            const int c = r_colidx[rk];
            double vv = a_c * x_c[c];
            if (a_p != 0.0) vv = fma(a_p, x_p[c], vv);
            rsum = fma(r_vals[rk], vv, rsum);
        }
        for (ck += LPR; ck < cend; ck += LPR) cvs += cellvals[gidx[ck]];
        ks = subwave_sum<LPR>(ks);
        rsum = subwave_sum<LPR>(rsum);
        cvs = subwave_sum<LPR>(cvs);
        if (sublane == 0) {
            double bv;
            if (isv) {
                const double nc = gptr ? conv_scale * cvs : nc_in;
                if (gptr) nfc_c[row] = nc;
                bv = rsum + cn_c * nc + cn_o * no_in + g_in + car;
            } else {
                bv = g_in;
            }
            const double rv = bv - ks;
            b[row] = bv;
            r[row] = rv;
            arr = fma(rv, rv, arr);
            abb = fma(bv, bv, abb);
        }
    }
    arr = block_sum(arr, red);
    abb = block_sum(abb, red);
    if (threadIdx.x == 0) {
        part_rr[blockIdx.x] = arr;
        part_bb[blockIdx.x] = abb;
    }
}

// The same cut ALONG the dependencies once more: three gather families that
// do not need each other run side by side in one launch --
//   workgroups [0, gk)   : kx = K x0                       (all rows)
//   workgroups [gk, ...) : b  = R1 (a_c v_c + a_p v_p) + cn_c nfc_c + cn_o nfc_o
//                               + g [+ carried residuals], nfc_c = gather of
//                               the cell values            (velocity rows);
//                          b_p = g_p                       (pressure rows)
// and what joins them -- r = b - kx with both norms -- is done by extra
// workgroups of the tau kernel behind (k_tau_first), whose row workgroups
// gather b - kx themselves.  (One kernel with all three chains per row took
// 8.9 us; the chains side by side take as long as the longest.)
template <int LPR>
__global__ void __launch_bounds__(kBlock)
k_step_one2(int gk, int n, int nv, const int *__restrict__ k_rowptr,
            const int *__restrict__ k_colidx, const double *__restrict__ k_vals,
            const int *__restrict__ r_rowptr, const int *__restrict__ r_colidx,
            const double *__restrict__ r_vals, const double *__restrict__ x0,
            const double *__restrict__ x_c, const double *__restrict__ x_p,
            double a_c, double a_p, double *__restrict__ nfc_c,
            const double *__restrict__ nfc_o, double cn_c, double cn_o,
            TabRef gtab, TabRef gptab, const int *__restrict__ gptr,
            const int *__restrict__ gidx, const double *__restrict__ cellvals,
            double conv_scale, const double *__restrict__ rc_c,
            const double *__restrict__ rc_p, double *__restrict__ b,
            double *__restrict__ kx) {
    const int sublane = threadIdx.x % LPR;
    if ((int)blockIdx.x < gk) {
        const int sub = (blockIdx.x * kBlock + threadIdx.x) / LPR;
        const int nsub = gk * (kBlock / LPR);
        for (int row = sub; row < n; row += nsub) {
            // (csr_row_dot's sums in three load levels: row_loads.hpp)
            const int k0 = k_rowptr[row], k1 = k_rowptr[row + 1];
            double s = 0.0;
            if (k0 < k1)
                s = row_dot_flat<LPR, 2, double>(RowPairs{}, k_colidx, k_vals,
                                                 GatherVec{x0}, k0, k1,
                                                 sublane);
            s = subwave_sum<LPR>(s);
            if (sublane == 0) kx[row] = s;
        }
        return;
    }
    const double *__restrict__ g = tab_row(gtab);
    const double *__restrict__ gp = tab_row(gptab);
    const int rb = blockIdx.x - gk, nrb = gridDim.x - gk;
    const int sub = (rb * kBlock + threadIdx.x) / LPR;
    const int nsub = nrb * (kBlock / LPR);
    for (int row = sub; row < n; row += nsub) {
        if (row >= nv) {
            if (sublane == 0) b[row] = gp[row - nv];
            continue;
        }
        int rk = r_rowptr[row] + sublane;
        const int rend = r_rowptr[row + 1];
        int ck = 0, cend = 0;
        if (gptr) {
            ck = gptr[row] + sublane;
            cend = gptr[row + 1];
        }
        const bool r_on = rk < rend, c_on = ck < cend;
        int rc = 0, ci = 0;
        double rval = 0.0;
        if (r_on) {
            rc = r_colidx[rk];
            rval = r_vals[rk];
        }
        if (c_on) ci = gidx[ck];
        double no_in = 0.0, g_in = 0.0, nc_in = 0.0, car = 0.0;
        if (sublane == 0) {
            no_in = nfc_o[row];
            g_in = g[row];
            if (!gptr) nc_in = nfc_c[row];
            if (rc_c) car = a_c * rc_c[row];
            if (rc_p && a_p != 0.0) car = fma(a_p, rc_p[row], car);
        }
        double rsum = 0.0, cvs = 0.0;
        if (r_on) {
            double vv = a_c * x_c[rc];
            if (a_p != 0.0) vv = fma(a_p, x_p[rc], vv);
            rsum = rval * vv;
        }
        if (c_on) cvs = cellvals[ci];
        for (rk += LPR; rk < rend; rk += LPR) {
            const int c = r_colidx[rk];
            double vv = a_c * x_c[c];
            if (a_p != 0.0) vv = fma(a_p, x_p[c], vv);
            rsum = fma(r_vals[rk], vv, rsum);
        }
        for (ck += LPR; ck < cend; ck += LPR) cvs += cellvals[gidx[ck]];
        rsum = subwave_sum<LPR>(rsum);
        cvs = subwave_sum<LPR>(cvs);
        if (sublane == 0) {
            const double nc = gptr ? conv_scale * cvs : nc_in;
            if (gptr) nfc_c[row] = nc;
            b[row] = rsum + cn_c * nc + cn_o * no_in + g_in + car;
        }
    }
}

// tau(r) for r = b - kx that nobody has formed yet: workgroups [0, gt) take
// the Schur rows, tau = r_p - (J Fh^-1) r_v with r gathered as b - kx;
// workgroups [gt, ...) form r itself with the partials of ||r||^2, ||b||^2
// (one per workgroup, read by the head kernel behind).  Rows of J Fh^-1 are
// long (~270 entries): 128 lanes per row.
__global__ void __launch_bounds__(kBlock)
k_tau_first(int gt, int n, int np, int nv, const int *__restrict__ rowptr,
            const int *__restrict__ colidx, const double *__restrict__ vals,
            const double *__restrict__ b, const double *__restrict__ kx,
            double *__restrict__ tau, double *__restrict__ r,
            double *__restrict__ part_rr, double *__restrict__ part_bb) {
    if ((int)blockIdx.x >= gt) {
        __shared__ double red[4];
        const int rb = blockIdx.x - gt, nrb = gridDim.x - gt;
        double arr = 0.0, abb = 0.0;
        for (int e = rb * kBlock + threadIdx.x; e < n; e += nrb * kBlock) {
            const double bv = b[e];
            const double rv = bv - kx[e];
            r[e] = rv;
            arr = fma(rv, rv, arr);
            abb = fma(bv, bv, abb);
        }
        arr = block_sum(arr, red);
        abb = block_sum(abb, red);
        if (threadIdx.x == 0) {
            part_rr[rb] = arr;
            part_bb[rb] = abb;
        }
        return;
    }
    __shared__ double half[kBlock / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int pair = threadIdx.x >> 7, l128 = threadIdx.x & 127;
    for (int base = blockIdx.x * 2; base < np; base += gt * 2) {
        const int row = base + pair;
        // level 1: the row's pointers WITH its own entries of b and kx (they
        // used to be asked for behind the two barriers); levels 2 and 3: four
        // chunks of 128 and their gathers (row_loads.hpp; an average row has
        // 270 entries, the fourth chunk repeats the row's last entry)
        const int rowc = min(row, np - 1);
        const int k0 = rowptr[rowc], k1 = rowptr[rowc + 1];
        const double bp = b[nv + rowc], kp = kx[nv + rowc];
        double sl = 0.0;
        if (row < np && k0 < k1)
            sl = row_dot_flat<128, 4, double>(RowPairs{}, colidx, vals,
                                              GatherDiff{b, kx}, k0, k1, l128);
        const double s = wave_sum(sl);
        __syncthreads();
        if (lane == 0) half[wave] = s;
        __syncthreads();
        if (l128 == 0 && row < np)
            tau[row] = (bp - kp) - (half[2 * pair] + half[2 * pair + 1]);
    }
}

// what the LAZY one-column tail reads beside the partials of the K apply:
// the partials of ||r||^2 and ||b||^2 (k_tau_first) and the tolerances
struct TailLazy {
    const double *part_rr, *part_bb;
    int nrb;                            // partials of each (<= kBlock)
    double rtol, atol;
};

// One block-wide reduction for the four sums of the lazy tail: every thread
// brings at most one partial of each, the result is valid in every thread and
// the same bits in every workgroup (fixed order); `red` holds 16 doubles
__device__ __forceinline__ void block_sum4(double &a, double &b, double &c,
                                           double &d, double *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
        c += __shfl_xor(c, o, 64);
        d += __shfl_xor(d, o, 64);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        red[4 * wave] = a;
        red[4 * wave + 1] = b;
        red[4 * wave + 2] = c;
        red[4 * wave + 3] = d;
    }
    __syncthreads();
    a = (red[0] + red[4]) + (red[8] + red[12]);
    b = (red[1] + red[5]) + (red[9] + red[13]);
    c = (red[2] + red[6]) + (red[10] + red[14]);
    d = (red[3] + red[7]) + (red[11] + red[15]);
}

// (the first `nrow_blocks` workgroups do the rows, the rest the cells; every
// workgroup repeats the tiny tail computation in its own LDS, workgroup 0
// alone commits the bookkeeping -- as k_arn_tail_acc)
// LAZY: the tail of the one-column cycle whose head scaled nothing
// (k_arn_head_lazy, k_spmv_rw): norm_part = [<r,w> | <w,w>], nparts <= kBlock
// partials each.  Every thread asks for its row or cell values and for one
// partial of each of the four sums at once, ONE reduction gives
//   alpha = <r,w> / <w,w>,   ||r - alpha w||^2 = ||r||^2 (1 - <r,w>^2 / (<w,w> ||r||^2))
// and the stores follow; no control-block entry is read in front of them.
// Workgroup 0 commits what k_arn_head (j = 0, first = 1) and the general tail
// leave in the control block AFTER its stores.  A start residual inside the
// tolerance takes no step (as the head would have stopped the cycle), r = 0
// among them; the six-node step never oversolves (stop_frac is not read).
template <bool LAZY>
__global__ void __launch_bounds__(kBlock)
k_arn_tail6(int c, int n, int nrow_blocks,
            const double *__restrict__ norm_part, int nparts, DnsCtl *ctl,
            double *__restrict__ histbuf, int hist_cap, int maxiter,
            const double *__restrict__ Z, size_t ld, Tail6 t6, TailExtrap te,
            TailCells tc, TailLazy tl) {
    __shared__ double sc[kMaxRestart + 2];
    __shared__ double yl[kMaxRestart];
    __shared__ int jl;
    if (LAZY) c = 1;
    const bool open_col = LAZY ? true : (!ctl->done && c > 0);
    const bool rowblk = (int)blockIdx.x < nrow_blocks;
    const int ef = blockIdx.x * kBlock + threadIdx.x;
    double pfx = 0.0, pz0 = 0.0, ph1 = 0.0, ph2 = 0.0, ph3 = 0.0, ph4 = 0.0,
           pr0 = 0.0, pw0 = 0.0;
    // cell workgroups: the twelve local values of x0 and of Z_0 are asked for
    // BEFORE the coefficients y exist (nothing of it depends on them)
    double u0[6][2], uz[6][2];
    int cmap[12];
    int cslot = 0, cq = 0, ccell = 0;
    bool clive = false;
    if (!rowblk && tc.nblocks > 0) {
        const double *__restrict__ dbcvals = tab_row(tc.dbctab);
        const int t = (blockIdx.x - nrow_blocks) * kBlock + threadIdx.x;
        cslot = t >> 3;
        cq = t & 7;
        clive = cslot < tc.ncells;
        ccell = clive ? cslot : 0;
        // one lane per slot asks the memory (lane q of the cell's eight: slots
        // q and q + 8), shuffles hand map entries and values round: 6 loads
        // per lane instead of 36 in front of the element arithmetic
        const int lane0 = (threadIdx.x & 63) & ~7;
        const int m_a = tc.cellmap[(size_t)cq * tc.ncells + ccell];
        const int m_b =
            (cq < 4) ? tc.cellmap[(size_t)(cq + 8) * tc.ncells + ccell] : -1;
        const double x_a = (m_a >= 0) ? t6.x0[m_a] : dbcvals[-m_a - 1];
        const double z_a = (m_a >= 0 && c > 0) ? Z[m_a] : 0.0;
        double x_b = 0.0, z_b = 0.0;
        if (cq < 4) {
            x_b = (m_b >= 0) ? t6.x0[m_b] : dbcvals[-m_b - 1];
            z_b = (m_b >= 0 && c > 0) ? Z[m_b] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            cmap[k] = __shfl(m_a, lane0 + k, 64);
            u0[k >> 1][k & 1] = __shfl(x_a, lane0 + k, 64);
            uz[k >> 1][k & 1] = __shfl(z_a, lane0 + k, 64);
        }
#pragma unroll
        for (int k = 8; k < 12; ++k) {
            cmap[k] = __shfl(m_b, lane0 + k - 8, 64);
            u0[k >> 1][k & 1] = __shfl(x_b, lane0 + k - 8, 64);
            uz[k >> 1][k & 1] = __shfl(z_b, lane0 + k - 8, 64);
        }
    }
    if (rowblk && ef < n) {
        pfx = t6.x0[ef];
        if (c > 0) pz0 = Z[ef];
        if (te.out) {
            if (te.e1 != 0.0) ph1 = te.h1[ef];
            if (te.e2 != 0.0) ph2 = te.h2[ef];
            if (te.e3 != 0.0) ph3 = te.h3[ef];
            if (te.e4 != 0.0) ph4 = te.h4[ef];
        }
        if (t6.rnew && ef < t6.nv) {
            pr0 = t6.r0[ef];
            if (c > 0) pw0 = t6.W[ef];
        }
    }
    // lazy cycle: what workgroup 0 commits behind its stores
    int lz_status = DNS_OK, lz_conv = 0, lz_tot = 0;
    double lz_rho = 0.0, lz_bn = 0.0, lz_tol = 0.0, lz_res = 0.0,
           lz_alpha = 0.0;
    if (LAZY) {
        const int t = threadIdx.x;
        double wr = t < nparts ? norm_part[t] : 0.0;
        double ww = t < nparts ? norm_part[nparts + t] : 0.0;
        double rr = t < tl.nrb ? tl.part_rr[t] : 0.0;
        double bb = t < tl.nrb ? tl.part_bb[t] : 0.0;
        block_sum4(wr, ww, rr, bb, sc);
        lz_rho = sqrt(rr);
        lz_bn = sqrt(bb);
        lz_tol = fmax(tl.rtol * lz_bn, tl.atol);
        lz_res = lz_rho;
        if (!(lz_rho > lz_tol)) {
            // nothing to do (or NaN): the head would have stopped the cycle
            lz_conv = lz_rho <= lz_tol;
            if (isnan(lz_rho) || isnan(lz_tol)) lz_status = DNS_BREAKDOWN;
        } else {
            // (ratios, not products: <w,w> ||r||^2 may leave the range)
            const double a = wr / ww;
            const double d = 1.0 - a * (wr / rr);
            if (!(d > 1e-8)) {
                // the guard of the fused Gram-Schmidt (pythagoras_norm): the
                // norm has lost its digits -- or w = 0, or NaN: no step
                lz_status = kGsFallback;
            } else {
                lz_alpha = a;
                lz_res = lz_rho * sqrt(d);
                lz_tot = 1;
                lz_conv = lz_res <= lz_tol;
            }
        }
    }
    if (!LAZY && open_col) reduce_partials(norm_part, nparts, nparts, c + 1, sc);
    if (!LAZY && threadIdx.x == 0) {
        // (the column being closed lives in LDS: as a local array indexed
        // at run time it went to scratch memory, 528 bytes per lane of every
        // wave of the launch for one thread's use)
        __shared__ double rcol[kMaxRestart + 1];
        double gl[2] = {0.0, 0.0};
        int jcols = ctl->jdone, status = DNS_OK, conv = 0, tot = ctl->total_it;
        double res = ctl->resnorm;
        bool closed = false;
        if (open_col) {
            const int j = c - 1;
            const double hn = pythagoras_norm(sc, c);
            if (hn < 0.0) {
                status = kGsFallback;
            } else {
                for (int i = 0; i <= j; ++i) rcol[i] = sc[i];
                for (int i = 0; i < j; ++i) {
                    const double t = ctl->cs[i] * rcol[i] +
                                     ctl->sn[i] * rcol[i + 1];
                    rcol[i + 1] = -ctl->sn[i] * rcol[i] +
                                  ctl->cs[i] * rcol[i + 1];
                    rcol[i] = t;
                }
                const double den = hypot(rcol[j], hn);
                double cc = 1.0, ss = 0.0;
                if (den > 0.0) {
                    cc = rcol[j] / den;
                    ss = hn / den;
                } else {
                    status = DNS_BREAKDOWN;
                }
                rcol[j] = den;
                gl[1] = -ss * ctl->g[j];
                gl[0] = cc * ctl->g[j];
                res = fabs(gl[1]);
                jcols = j + 1;
                tot += 1;
                conv = res <= ctl->tol;
                if (isnan(res)) status = DNS_BREAKDOWN;
                closed = true;
            }
        }
        for (int i = jcols - 1; i >= 0; --i) {
            double s = (closed && i == jcols - 1) ? gl[0] : ctl->g[i];
            for (int k = i + 1; k < jcols; ++k) {
                const double rik = (closed && k == jcols - 1)
                                       ? rcol[i]
                                       : ctl->R[(size_t)k * (kMaxRestart + 1) + i];
                s -= rik * yl[k];
            }
            const double d = (closed && i == jcols - 1)
                                 ? rcol[i]
                                 : ctl->R[(size_t)i * (kMaxRestart + 1) + i];
            yl[i] = (d != 0.0) ? s / d : 0.0;
        }
        jl = jcols;
        if (blockIdx.x == 0) {
            const int was_conv = ctl->conv;
            if (closed) {
                ctl->resnorm = res;
                ctl->hist[jcols] = res;
                ctl->total_it = tot;
                if (status != DNS_OK) ctl->status = status;
                if (conv) ctl->conv = 1;
            } else if (status != DNS_OK) {
                ctl->status = status;
            }
            const int nowconv = was_conv || conv;
            int hl = ctl->hist_len;
            for (int i = (hl > 0 ? 1 : 0); i <= jcols && hl < hist_cap; ++i)
                histbuf[hl++] = (closed && i == jcols) ? res : ctl->hist[i];
            ctl->hist_len = hl;
            ctl->acc_solves += 1;
            ctl->acc_iters += tot;
            if (tot > ctl->acc_maxit) ctl->acc_maxit = tot;
            if (nowconv && ctl->tol > 0.0) {
                const double rel = res / ctl->tol;
                if (rel > ctl->acc_maxrel) ctl->acc_maxrel = rel;
            }
            if (!nowconv) ctl->acc_fail += 1;
        }
    }
    if (!LAZY) __syncthreads();
    const int jcols = LAZY ? lz_tot : jl;
    const double y0 = LAZY ? lz_alpha : (jcols > 0 ? yl[0] : 0.0);
    if (!rowblk) {
        // convection cells of the new velocity x0 + Z y, from the values that
        // arrived meanwhile (further columns: rare, gathered now)
        if (tc.nblocks > 0) {
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    double v = fma(y0, uz[a][i], u0[a][i]);
                    const int m = cmap[2 * a + i];
                    if (!LAZY && m >= 0)
                        for (int j = 1; j < jcols; ++j)
                            v = fma(yl[j], Z[(size_t)j * ld + m], v);
                    u0[a][i] = v;
                }
            conv_cells_compute(u0, tc.ncells, ccell, cslot, cq, clive, tc.glam,
                               tc.area, tc.cellvals);
        }
        return;
    }
    const int stride = nrow_blocks * kBlock;
    for (int e = ef; e < n; e += stride) {
        const bool first = e == ef;
        double s = first ? pfx : t6.x0[e];
        if (jcols > 0) s = fma(y0, first ? pz0 : Z[e], s);
        if (!LAZY)
            for (int i = 1; i < jcols; ++i)
                s = fma(yl[i], Z[(size_t)i * ld + e], s);
        t6.xout[e] = s;
        if (te.out) {
            if (first) {
                double v = te.e0 * s;
                v = fma(te.e1, ph1, v);
                v = fma(te.e2, ph2, v);
                v = fma(te.e3, ph3, v);
                v = fma(te.e4, ph4, v);
                te.out[e] = v;
            } else {
                tail_extrapolate(te, e, s);
            }
        }
        if (t6.rnew && e < t6.nv) {
            double rr = first ? pr0 : t6.r0[e];
            if (jcols > 0) rr = fma(-y0, first ? pw0 : t6.W[e], rr);
            if (!LAZY)
                for (int i = 1; i < jcols; ++i)
                    rr = fma(-yl[i], t6.W[(size_t)i * ld + e], rr);
            t6.rnew[e] = rr;
        }
    }
    if (LAZY && blockIdx.x == 0 && threadIdx.x == 0) {
        // the solve's record, behind this workgroup's stores: what k_arn_head
        // (j = 0, first = 1) and the general tail above leave
        ctl->predone = 0;
        ctl->jdone = lz_tot;
        ctl->zero = 0;
        ctl->done = 1;
        ctl->status = lz_status;
        ctl->total_it = lz_tot;
        ctl->conv = lz_conv;
        ctl->need_it = lz_conv ? lz_tot : -1;
        ctl->beta = lz_rho;
        ctl->tol = lz_tol;
        ctl->resnorm = lz_res;
        ctl->bnorm = lz_bn;
        ctl->g[0] = lz_rho;
        ctl->hist[0] = lz_rho;
        ctl->hist[1] = lz_res;
        int hl = 0;
        if (hl < hist_cap) histbuf[hl++] = lz_rho;
        if (lz_tot > 0 && hl < hist_cap) histbuf[hl++] = lz_res;
        ctl->hist_len = hl;
        ctl->acc_solves += 1;
        ctl->acc_iters += lz_tot;
        if (lz_tot > ctl->acc_maxit) ctl->acc_maxit = lz_tot;
        if (lz_conv && lz_tol > 0.0) {
            const double rel = lz_res / lz_tol;
            if (rel > ctl->acc_maxrel) ctl->acc_maxrel = rel;
        }
        if (!lz_conv) ctl->acc_fail += 1;
    }
}

// Start of a pipelined batch in ONE launch: checkpoint of the ring (and of
// the convection history) and reset of the batch accumulators of the control
// block -- eight hipMemcpyAsync + two hipMemsetAsync cost the host ~50 us per
// batch, which a 20-step window sees.
struct CopyList {
    const double *src[12];
    double *dst[12];
    int n[12];
    int count;
};

__global__ void __launch_bounds__(kBlock)
k_batch_begin(CopyList cl, DnsCtl *ctl, double stop_frac) {
    for (int q = 0; q < cl.count; ++q) {
        const double *__restrict__ s = cl.src[q];
        double *__restrict__ d = cl.dst[q];
        for (int i = blockIdx.x * kBlock + threadIdx.x; i < cl.n[q];
             i += gridDim.x * kBlock)
            d[i] = s[i];
    }
    if (ctl && blockIdx.x == 0 && threadIdx.x == 0) {
        ctl->acc_solves = 0;
        ctl->acc_fail = 0;
        ctl->acc_iters = 0;
        ctl->acc_maxit = 0;
        ctl->acc_maxrel = 0.0;
        ctl->acc_maxprev = 0.0;
        ctl->acc_maxneed = 0;
        ctl->acc_sumneed = 0;
        ctl->stop_frac = stop_frac;
    }
}

// Checkpoint of a pipelined batch (dns_imex_run, dns_trap_checkpoint): `add`
// copies a live buffer into a buffer of the checkpoint's own (allocated when
// it grows: call it outside a stream capture) and records the pair in both
// directions.  save() is ONE k_batch_begin launch over the list (with `ctl`:
// and the reset of the batch accumulators; `copy` false: that alone),
// restore() the same launch with the list reversed and no control block.
struct Checkpoint {
    static constexpr int kMax = sizeof(CopyList::n) / sizeof(CopyList::n[0]);
    DevBuf<double> buf[kMax];
    CopyList fwd{}, back{};
    size_t nmax = 0;                   // (sizes the grid: the ring's ld)
    void clear() {
        fwd.count = back.count = 0;
        nmax = 0;
    }
    int add(double *live, size_t n) {
        const int q = fwd.count;
        if (q >= kMax) return fail(DNS_ERR_BAD_ARGUMENT, "checkpoint full");
        if (buf[q].n < n) DNS_TRY(buf[q].alloc(n));
        fwd.count = back.count = q + 1;
        fwd.src[q] = back.dst[q] = live;
        back.src[q] = fwd.dst[q] = buf[q].p;
        fwd.n[q] = back.n[q] = (int)n;
        nmax = std::max(nmax, n);
        return DNS_OK;
    }
    int save(hipStream_t s, DnsCtl *ctl = nullptr, double stop_frac = 0.0,
             bool copy = true) const {
        CopyList l = fwd;
        if (!copy) l.count = 0;
        return launch(l, s, ctl, stop_frac);
    }
    int restore(hipStream_t s) const { return launch(back, s, nullptr, 0.0); }

  private:
    int launch(const CopyList &l, hipStream_t s, DnsCtl *ctl,
               double stop_frac) const {
        const int g = (int)std::max<size_t>(
            128, std::min<size_t>(2048, nmax / 1024));
        hipLaunchKernelGGL(k_batch_begin, g, kBlock, 0, s, l, ctl, stop_frac);
        DNS_HIP(hipGetLastError());
        return DNS_OK;
    }
};

// ---------------------------------------------------------------------------
// Front of a ROW-PARTITIONED IMEX step in the latency regime: for this rank's
// rows of K (velocity rows, then pressure rows; RowMap) ONE launch forms
//   nfc_c = scale * (gathered convection cell values)       (gptr != nullptr)
//   b_v   = R1 (a_c v_c + a_p v_p) + cn_c nfc_c + cn_o nfc_o + g ,  b_p = gp
//   r     = b - K x0   and the partials of ||r||^2, ||b||^2
// (three launches before: convection gather, right-hand side, residual).  R1
// holds the rank's velocity rows (local row = local velocity row of K).
// ---------------------------------------------------------------------------
template <int LPR>
__global__ void __launch_bounds__(kBlock)
k_dist_front(RowMap rm, int nv_all, const int *__restrict__ krp,
             const int *__restrict__ kci, const double *__restrict__ kva,
             const double *__restrict__ x0, const int *__restrict__ rrp,
             const int *__restrict__ rci, const double *__restrict__ rva,
             const double *__restrict__ v_c, const double *__restrict__ v_p,
             double a_c, double a_p, double *__restrict__ nfc_c,
             const double *__restrict__ nfc_o, double cn_c, double cn_o,
             TabRef gtab, TabRef gptab, const int *__restrict__ gptr,
             const int *__restrict__ gidx, const double *__restrict__ cellvals,
             double conv_scale, double *__restrict__ b, double *__restrict__ r,
             double *__restrict__ part_rr, double *__restrict__ part_bb,
             const double *__restrict__ rcc, const double *__restrict__ rcp,
             double *__restrict__ x0copy = nullptr, int n_all = 0) {
    // rcc / rcp (residual carry-over, dns_imex_coeffs.carry_residual): the true
    // velocity residuals of the last two solves, added to the right-hand side
    // with the weights of the solutions they belong to
    // x0copy: the warm start as it stands, for the cell workgroups of this
    // step's tail (k_arn_tail_lazy1 overwrites x0 in place while they run)
    __shared__ double red[4];
    if (x0copy)
        for (int e = blockIdx.x * kBlock + threadIdx.x; e < n_all;
             e += gridDim.x * kBlock)
            x0copy[e] = x0[e];
    const double *__restrict__ g = tab_row(gtab);
    const double *__restrict__ gp = tab_row(gptab);
    const int sub = (blockIdx.x * kBlock + threadIdx.x) / LPR;
    const int sublane = threadIdx.x % LPR;
    const int nsub = gridDim.x * (kBlock / LPR);
    double arr = 0.0, abb = 0.0;
    for (int li = sub; li < rm.len1 + rm.len2; li += nsub) {
        const int row = map_row(rm, li);
        // K row first: its gathers are the long pole
        const double sk = csr_row_dot<LPR>(krp, kci, kva, x0, li, sublane);
        double bv;
        if (li < rm.len1) {
            double s = 0.0;
            const int k1 = rrp[li + 1];
            if (a_p != 0.0) {
                for (int k = rrp[li] + sublane; k < k1; k += LPR) {
                    const int c = rci[k];
                    s = fma(rva[k], fma(a_c, v_c[c], a_p * v_p[c]), s);
                }
            } else {
                for (int k = rrp[li] + sublane; k < k1; k += LPR)
                    s = fma(rva[k], a_c * v_c[rci[k]], s);
            }
            s = subwave_sum<LPR>(s);
            double nc;
            if (gptr) {
                double sg = 0.0;
                const int g1 = gptr[row + 1];
                for (int k = gptr[row] + sublane; k < g1; k += LPR)
                    sg += cellvals[gidx[k]];
                nc = conv_scale * subwave_sum<LPR>(sg);
                if (sublane == 0) nfc_c[row] = nc;
            } else {
                nc = nfc_c[row];
            }
            bv = s + cn_c * nc + cn_o * nfc_o[row] + g[row];
            if (rcc) {
                bv = fma(a_c, rcc[row], bv);
                if (a_p != 0.0) bv = fma(a_p, rcp[row], bv);
            }
        } else {
            bv = gp[row - nv_all];
        }
        if (sublane == 0) {
            const double v = bv - sk;
            b[row] = bv;
            r[row] = v;
            arr = fma(v, v, arr);
            abb = fma(bv, bv, abb);
        }
    }
    arr = block_sum(arr, red);
    abb = block_sum(abb, red);
    if (threadIdx.x == 0) {
        part_rr[blockIdx.x] = arr;
        part_bb[blockIdx.x] = abb;
    }
}

// Tail of that cycle: every workgroup forms the step length from the four
// all-reduced sums and updates its share of x; workgroup 0 commits the solve's
// bookkeeping -- everything k_arn_head (j = 0, first = 1) and k_arn_tail_acc
// would have left in the control block.  A solve whose start vector is inside
// the tolerance already takes no step.
__global__ void __launch_bounds__(kBlock)
k_arn_tail_lazy1(int n, const double *__restrict__ hs, DnsCtl *ctl,
                 double *__restrict__ histbuf, int hist_cap, int maxiter,
                 double rtol, double atol, const double *__restrict__ Z,
                 double *__restrict__ x, TailExtrap te,
                 const double *__restrict__ r0 = nullptr,
                 const double *__restrict__ w = nullptr,
                 double *__restrict__ rnew = nullptr, int nv = 0,
                 int nrow_blocks = 0, const double *__restrict__ x0copy = nullptr,
                 TailCells tc = TailCells{}) {
    // rnew (residual carry-over): the velocity part of the TRUE residual behind
    // the step, r0 - alpha w = b - K (x0 + alpha z), wherever r0 and w are
    // valid (the rank's own rows)
    // tc / x0copy (time stepper with device convection): workgroups beyond
    // `nrow_blocks` evaluate the convection cells of the NEW velocity from its
    // definition x0 + alpha z -- x is being overwritten by the row workgroups
    // of this very launch, so the warm start is read from the copy the front
    // kernel of the step has made (`x0copy`), never from x
    if (nrow_blocks <= 0) nrow_blocks = gridDim.x;
    const bool rowblk = (int)blockIdx.x < nrow_blocks;
    const int ef = blockIdx.x * kBlock + threadIdx.x;
    double pfx = 0.0, pz0 = 0.0;
    double u0[6][2], uz[6][2];
    int cslot = 0, cq = 0, ccell = 0;
    bool clive = false;
    if (!rowblk) {
        const double *__restrict__ dbcvals = tab_row(tc.dbctab);
        const int t = (blockIdx.x - nrow_blocks) * kBlock + threadIdx.x;
        cslot = t >> 3;
        cq = t & 7;
        clive = tc.sel ? cslot < tc.nsel : cslot < tc.ncells;
        ccell = clive ? (tc.sel ? tc.sel[cslot] : cslot) : 0;
        // (one lane per slot asks the memory, as in k_arn_tail6)
        const int lane0 = (threadIdx.x & 63) & ~7;
        const int m_a = tc.cellmap[(size_t)cq * tc.ncells + ccell];
        const int m_b =
            (cq < 4) ? tc.cellmap[(size_t)(cq + 8) * tc.ncells + ccell] : -1;
        const double x_a = (m_a >= 0) ? x0copy[m_a] : dbcvals[-m_a - 1];
        const double z_a = (m_a >= 0) ? Z[m_a] : 0.0;
        double x_b = 0.0, z_b = 0.0;
        if (cq < 4) {
            x_b = (m_b >= 0) ? x0copy[m_b] : dbcvals[-m_b - 1];
            z_b = (m_b >= 0) ? Z[m_b] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            u0[k >> 1][k & 1] = __shfl(x_a, lane0 + k, 64);
            uz[k >> 1][k & 1] = __shfl(z_a, lane0 + k, 64);
        }
#pragma unroll
        for (int k = 8; k < 12; ++k) {
            u0[k >> 1][k & 1] = __shfl(x_b, lane0 + k - 8, 64);
            uz[k >> 1][k & 1] = __shfl(z_b, lane0 + k - 8, 64);
        }
    } else if (ef < n) {
        pfx = x[ef];
        pz0 = Z[ef];
    }
    const double wr = hs[0], ww = hs[1], rr = hs[2], bb = hs[3];
    const double rho = sqrt(rr), bn = sqrt(bb);
    const double tol = fmax(rtol * bn, atol);
    int status = DNS_OK, conv = 0, tot = 0;
    double res = rho, alpha = 0.0;
    // The step is TAKEN even when the start residual is inside the tolerance
    // already: z and w of this cycle exist whatever rho was (the captured
    // kernels of a one-step cycle always run), so the correction is free --
    // and a time step that skipped it would keep the extrapolated pressure,
    // p = -p~/dt, with an error of tol/dt (level 3, dt = 1/1024: 1.3e-8 against
    // the reference with one step in nine skipped).  Only a residual at the
    // rounding level is left alone (the Pythagoras guard below would misread
    // it).
    const bool go = (rho > 1e-3 * tol) && !isnan(rho) && maxiter > 0;
    if (isnan(rho) || isnan(tol)) status = DNS_BREAKDOWN;
    if (go) {
        const double d = ww * rr - wr * wr;
        if (!(ww > 0.0) || isnan(ww)) {
            status = DNS_BREAKDOWN;
        } else if (!(d > 1e-8 * ww * rr)) {
            // (the guard of the fused Gram-Schmidt: the norm by Pythagoras has
            // lost its digits)
            status = kGsFallback;
        } else {
            alpha = wr / ww;
            res = rho * sqrt(d / (ww * rr));
            tot = 1;
            conv = res <= tol;
            if (isnan(res)) status = DNS_BREAKDOWN;
        }
    } else {
        conv = rho <= tol;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl->predone = 0;
        ctl->jdone = tot;
        ctl->zero = 0;
        ctl->done = 1;
        ctl->status = status;
        ctl->total_it = tot;
        ctl->conv = conv;
        ctl->beta = rho;
        ctl->tol = tol;
        ctl->resnorm = res;
        ctl->bnorm = bn;
        ctl->g[0] = rho;
        ctl->hist[0] = rho;
        ctl->hist[1] = res;
        ctl->y[0] = rho * alpha;
        int hl = 0;
        if (hl < hist_cap) histbuf[hl++] = rho;
        if (tot > 0 && hl < hist_cap) histbuf[hl++] = res;
        ctl->hist_len = hl;
        ctl->acc_solves += 1;
        ctl->acc_iters += tot;
        if (tot > ctl->acc_maxit) ctl->acc_maxit = tot;
        if (conv && tol > 0.0) {
            const double rel = res / tol;
            if (rel > ctl->acc_maxrel) ctl->acc_maxrel = rel;
        }
        if (!conv) ctl->acc_fail += 1;
    }
    if (!rowblk) {
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int i = 0; i < 2; ++i)
                u0[a][i] = fma(alpha, uz[a][i], u0[a][i]);
        conv_cells_compute(u0, tc.ncells, ccell, ccell, cq, clive, tc.glam,
                           tc.area, tc.cellvals);
        return;
    }
    const int stride = nrow_blocks * kBlock;
    if (rnew)
        for (int e = ef; e < nv; e += stride)
            rnew[e] = fma(-alpha, w[e], r0[e]);
    if (tot == 0 && !te.out) return;
    if (ef < n) {
        const double s = fma(alpha, pz0, pfx);
        if (tot > 0) x[ef] = s;
        if (te.out) tail_extrapolate(te, ef, s);
    }
    for (int e = ef + stride; e < n; e += stride) {
        const double s = fma(alpha, Z[e], x[e]);
        if (tot > 0) x[e] = s;
        if (te.out) tail_extrapolate(te, e, s);
    }
}

}  // namespace dns
