// Host-side algebra of the multigrid levels of the Schur block: smoothing
// diagonals, damping, the fused cycle operators and the halo lists of a
// row-partitioned level.  Plain C++, no HIP (see halo_host.hpp).
//
// Every piece is defined on the rows [f0, f1) of the level operator S: the
// whole hierarchy (build_mg_levels) passes [0, n), the partitioned set-up
// (mg_rows.inc) a rank's rows of a matrix that keeps the global shape with only
// the rows it holds populated (hostcsr.hpp, host_embed_rows).  Every product is
// row-wise, so the rows of a partitioned set-up are equal, entry for entry, to
// the same rows of the whole operators.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "halo_host.hpp"
#include "hostcsr.hpp"

namespace dns {

// 1 / diag(S) for smoothing (dv: duplicate diagonal entries summed, 1 where the
// sum is 0) and the diagonal of the power iteration (dj: 1 / the last non-zero
// diagonal entry) of the rows [f0, f1); 1 on the other rows
inline void mg_diagonals(const HostCsr &S, int f0, int f1,
                         std::vector<double> &dv, std::vector<double> &dj) {
    dv.assign((size_t)S.nrows, 1.0);
    dj.assign((size_t)S.nrows, 1.0);
    for (int i = f0; i < f1; ++i) {
        double d = 0.0;
        for (int k = S.rowptr[i]; k < S.rowptr[i + 1]; ++k)
            if (S.colidx[k] == i) {
                d += S.vals[k];
                if (S.vals[k] != 0.0) dj[i] = 1.0 / S.vals[k];
            }
        dv[i] = (d != 0.0) ? 1.0 / d : 1.0;
    }
}

// largest eigenvalue (in modulus) of D^-1 S by power iterations: the product on
// the rows [f0, f1), then exchange(y) completes y (an int status, 0 = fine: a
// no-op on the whole matrix, the all-gather by rows); the norms are taken on
// the whole vector in index order, so the result does not depend on the split
template <typename Exchange>
inline int mg_jacobi_lmax(const HostCsr &S, int f0, int f1,
                          const std::vector<double> &dj, Exchange &&exchange,
                          double *lmax, int iters = 20) {
    const int n = S.nrows;
    std::vector<double> x((size_t)n), y((size_t)n, 0.0);
    for (int i = 0; i < n; ++i) x[i] = 1.0 + 0.5 * std::sin(0.37 * i + 1.0);
    double lam = 1.0;
    for (int it = 0; it < iters; ++it) {
        for (int i = f0; i < f1; ++i) {
            double s = 0.0;
            for (int k = S.rowptr[i]; k < S.rowptr[i + 1]; ++k)
                s += S.vals[k] * x[S.colidx[k]];
            y[i] = dj[i] * s;
        }
        if (const int e = exchange(y)) return e;
        double nx = 0.0, ny = 0.0;
        for (int i = 0; i < n; ++i) {
            nx += x[i] * x[i];
            ny += y[i] * y[i];
        }
        lam = std::sqrt(ny / nx);
        const double sc = 1.0 / std::sqrt(ny);
        for (int i = 0; i < n; ++i) x[i] = y[i] * sc;
    }
    *lmax = lam;
    return 0;
}

// damping of the first / second sweep of a pair (solver.hpp, MgLevel::omega):
// 4 / (3 lmax) twice, or with `cheb` (two sweeps) the reciprocals of the
// Chebyshev roots of [lmax / alpha, 1.05 lmax]
inline void mg_damping(double lmax, bool cheb, double alpha, double *omega,
                       double *omega2) {
    lmax = std::max(1e-300, lmax);
    *omega = *omega2 = 4.0 / (3.0 * lmax);
    if (cheb) {
        const double hi = 1.05 * lmax, lo = lmax / alpha;
        const double mid = 0.5 * (hi + lo), rad = 0.5 * (hi - lo);
        const double c = 0.70710678118654752;    // cos(pi / 4)
        *omega = 1.0 / (mid + rad * c);
        *omega2 = 1.0 / (mid - rad * c);
    }
}

// operators of a fused cycle: rows [f0, f1) of Apre and Qq, the rows of Rr
// that the rows of P^T passed in give
struct MgOps {
    HostCsr Apre, Rr, Qq;
};

// what both fused cycles build on, rows [f0, f1): the identity, W S and
// P - W S P with W = w D^-1 (SP = S P on the rows of S held)
struct MgSweepRows {
    HostCsr I, WS, PW;
};

inline MgSweepRows mg_sweep_rows(const HostCsr &S, const HostCsr &SP,
                                 const HostCsr &P, int f0, int f1,
                                 const std::vector<double> &dv, double w) {
    std::vector<double> wd((size_t)(f1 - f0));
    for (int i = f0; i < f1; ++i) wd[(size_t)(i - f0)] = w * dv[i];
    MgSweepRows r;
    r.I.nrows = f1 - f0;
    r.I.ncols = S.ncols;
    r.I.vals.assign((size_t)(f1 - f0), 1.0);
    for (int i = f0; i <= f1; ++i) r.I.rowptr.push_back(i - f0);
    for (int i = f0; i < f1; ++i) r.I.colidx.push_back(i);
    r.WS = host_row_slice(S, f0, f1);
    host_scale_rows(wd, r.WS);
    HostCsr WSP = host_row_slice(SP, f0, f1);
    host_scale_rows(wd, WSP);
    r.PW = host_add(1.0, host_row_slice(P, f0, f1), -1.0, WSP);
    return r;
}

// fused V(2,2) (solver.hpp, MgLevel), T = I - w1 D^-1 S:
//   Apre = ((w1 + w2) I - w2 (w1 D^-1 S)) D^-1   (two sweeps from 0)
//   Rr   = [P^T, -P^T S]
//   Qq   = [T, T P]
// S holds the rows [f0, f1) and the rows the rows of PT reference
inline MgOps mg_fused22_ops(const HostCsr &S, const HostCsr &SP,
                            const HostCsr &P, const HostCsr &PT, int f0, int f1,
                            const std::vector<double> &dv, double w1,
                            double w2) {
    const MgSweepRows s = mg_sweep_rows(S, SP, P, f0, f1, dv, w1);
    MgOps o;
    o.Apre = host_add(w1 + w2, s.I, -w2, s.WS);
    for (size_t k = 0; k < o.Apre.vals.size(); ++k)
        o.Apre.vals[k] *= dv[o.Apre.colidx[k]];
    HostCsr mPTS = host_spgemm(PT, S);
    for (double &v : mPTS.vals) v = -v;
    o.Rr = host_hstack(PT, mPTS);
    o.Qq = host_hstack(host_add(1.0, s.I, -1.0, s.WS), s.PW);
    return o;
}

// fused V(1,1) (solver.hpp, mg_fused11), T = I - w D^-1 S:
//   Rr = Rd = P^T - (P^T S) w D^-1
//   Qq = U  = [(I + T) w D^-1, T P], negated on the finest level (zp = -x)
inline MgOps mg_fused11_ops(const HostCsr &S, const HostCsr &SP,
                            const HostCsr &P, const HostCsr &PT, int f0, int f1,
                            const std::vector<double> &dv, double w,
                            bool finest) {
    const MgSweepRows s = mg_sweep_rows(S, SP, P, f0, f1, dv, w);
    MgOps o;
    // (I + T) w D^-1 = (2 I - w D^-1 S) w D^-1
    HostCsr Ap = host_add(2.0, s.I, -1.0, s.WS);
    for (size_t k = 0; k < Ap.vals.size(); ++k)
        Ap.vals[k] *= w * dv[Ap.colidx[k]];
    HostCsr PTSw = host_spgemm(PT, S);
    for (size_t k = 0; k < PTSw.vals.size(); ++k)
        PTSw.vals[k] *= w * dv[PTSw.colidx[k]];
    o.Rr = host_add(1.0, PT, -1.0, PTSw);
    o.Qq = host_hstack(Ap, s.PW);
    if (finest)
        for (double &v : o.Qq.vals) v = -v;
    return o;
}

// halo lists of one rank on a row-partitioned level (starts st, next level
// stc): needF[q] the level-l entries in q's rows that the rows [f0, f1) of S,
// Apre, Qq and the rows [c0, c1) of Rr = [P^T, -P^T S] (both halves index
// level-l vectors) reference; needC[q] the next level's entries the second
// half of Qq references -- none when that level runs replicated
inline void mg_need_lists(const HostCsr &S, const HostCsr &Apre,
                          const HostCsr &Qq, int f0, int f1, const HostCsr &Rr,
                          int c0, int c1, const std::vector<int> &st,
                          const std::vector<int> &stc, int rank,
                          bool coarse_replicated,
                          std::vector<std::vector<int>> &needF,
                          std::vector<std::vector<int>> &needC) {
    const int nranks = (int)st.size() - 1, n = st.back(), nc = stc.back();
    std::vector<unsigned char> mf((size_t)n, 0), mc((size_t)nc, 0);
    mark_cols(S.view(), f0, f1, 0, n, 0, mf);
    mark_cols(Apre.view(), f0, f1, 0, n, 0, mf);
    mark_cols(Qq.view(), f0, f1, 0, n, 0, mf);
    mark_cols(Qq.view(), f0, f1, n, n + nc, n, mc);
    mark_cols(Rr.view(), c0, c1, 0, n, 0, mf);
    mark_cols(Rr.view(), c0, c1, n, 2 * n, n, mf);
    marked_need(mf, st.data(), nranks, rank, needF);
    if (coarse_replicated)
        needC.assign((size_t)nranks, std::vector<int>());
    else
        marked_need(mc, stc.data(), nranks, rank, needC);
}

}  // namespace dns
