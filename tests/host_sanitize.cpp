// CPU-only sanitizer target for the HOST logic of the library (no HIP, no GPU):
// hostcsr.hpp (SpGEMM, polynomial rows, transposes, slices), pair_host.hpp
// (pair-format builder), halo_host.hpp (partition, halo index lists),
// mg_host.hpp (multigrid level operators, damping, halo lists),
// batch_policy.hpp (cycle and batch length of the pipelined batches),
// ring.hpp (solution ring and warm-start coefficients of the resident time
// steppers) and status.hpp (the exception barrier of the C-ABI) are compiled
// as they are with
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover
// and driven over a small saddle-point system with the structure of the
// package's matrices (2x2 velocity node blocks, pressure rows on node
// patches), whole and in row blocks of 1..4 ranks, with the edge cases the
// set-up meets (empty blocks, odd sizes, rows without entries).  Every result
// is checked against a dense / scalar restatement, so a wrong index that stays
// inside its allocation is caught as well.  tests/test_host_sanitized.py
// builds and runs it.
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../dolfin_navier_scipy_amd/csrc/batch_policy.hpp"
#include "../dolfin_navier_scipy_amd/csrc/halo_host.hpp"
#include "../dolfin_navier_scipy_amd/csrc/hostcsr.hpp"
#include "../dolfin_navier_scipy_amd/csrc/mg_host.hpp"
#include "../dolfin_navier_scipy_amd/csrc/pair_host.hpp"
#include "../dolfin_navier_scipy_amd/csrc/ring.hpp"
#include "../dolfin_navier_scipy_amd/csrc/status.hpp"

using dns::HostCsr;

static int g_fail = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #cond, __FILE__,   \
                    __LINE__);                                               \
            ++g_fail;                                                        \
        }                                                                    \
    } while (0)

static HostCsr from_map(int nr, int nc,
                        const std::vector<std::map<int, double>> &rows) {
    HostCsr A;
    A.nrows = nr;
    A.ncols = nc;
    A.rowptr.assign(1, 0);
    for (int i = 0; i < nr; ++i) {
        for (const auto &kv : rows[i]) {
            A.colidx.push_back(kv.first);
            A.vals.push_back(kv.second);
        }
        A.rowptr.push_back((int)A.colidx.size());
    }
    return A;
}

static std::vector<double> dense(const HostCsr &A) {
    std::vector<double> d((size_t)A.nrows * A.ncols, 0.0);
    for (int i = 0; i < A.nrows; ++i)
        for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k)
            d[(size_t)i * A.ncols + A.colidx[k]] += A.vals[k];
    return d;
}

static double lcg(unsigned &s) {
    s = s * 1664525u + 1013904223u;
    return ((s >> 8) & 0xffff) / 65536.0 - 0.5;
}

// nodes on an nx x ny grid, two interleaved velocity dofs per node; F couples
// a node with its 4 neighbours through dense 2x2 blocks (diagonally dominant),
// J has one pressure row per grid cell over the 8 dofs of its corners
static void build_system(int nx, int ny, HostCsr &F, HostCsr &J) {
    const int nn = nx * ny, nv = 2 * nn, np = (nx - 1) * (ny - 1);
    unsigned seed = 12345u;
    std::vector<std::map<int, double>> fr((size_t)nv), jr((size_t)np);
    auto node = [&](int i, int j) { return j * nx + i; };
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            const int a = node(i, j);
            const int nb[5][2] = {{i, j}, {i - 1, j}, {i + 1, j}, {i, j - 1},
                                  {i, j + 1}};
            for (int q = 0; q < 5; ++q) {
                const int bi = nb[q][0], bj = nb[q][1];
                if (bi < 0 || bi >= nx || bj < 0 || bj >= ny) continue;
                const int b = node(bi, bj);
                for (int r = 0; r < 2; ++r)
                    for (int c = 0; c < 2; ++c) {
                        double v = 0.2 * lcg(seed);
                        if (q == 0 && r == c) v += 4.0;
                        fr[(size_t)2 * a + r][2 * b + c] = v;
                    }
            }
        }
    for (int j = 0; j + 1 < ny; ++j)
        for (int i = 0; i + 1 < nx; ++i) {
            const int p = j * (nx - 1) + i;
            const int cs[4] = {node(i, j), node(i + 1, j), node(i, j + 1),
                               node(i + 1, j + 1)};
            for (int q = 0; q < 4; ++q) {
                jr[(size_t)p][2 * cs[q]] = lcg(seed);
                // (some rows touch only the x dof of a corner: half-filled
                // (vx, vy) entries of the pair format)
                if ((p + q) % 3) jr[(size_t)p][2 * cs[q] + 1] = lcg(seed);
            }
        }
    F = from_map(nv, nv, fr);
    J = from_map(np, nv, jr);
}

// y = K x from the pair format, scalar restatement of k_spmv_pair16x's
// arithmetic incl. the 16-bit column decoding
static std::vector<double> pair_apply(const dns::HostPair &P,
                                      const std::vector<double> &x) {
    const int nblocks = (int)P.rowblocks.size() - 1;
    std::vector<double> y((size_t)2 * P.nvp + P.np, 0.0);
    auto col = [&](unsigned short c, int b, int which) {
        return P.base[(size_t)2 * b + which] + (int)c;
    };
    for (int b = 0; b < nblocks; ++b)
        for (int r = P.rowblocks[b]; r < P.rowblocks[b + 1]; ++r) {
            if (r < P.nvp) {
                double y0 = 0.0, y1 = 0.0;
                for (int k = P.rpA[r]; k < P.rpA[r + 1]; ++k) {
                    const int c = col(P.cA[k], b, 0);
                    CHECK(c == P.colA[k]);
                    const double x0 = x[(size_t)2 * c], x1 = x[(size_t)2 * c + 1];
                    y0 += P.vA[(size_t)4 * k] * x0 + P.vA[(size_t)4 * k + 1] * x1;
                    y1 += P.vA[(size_t)4 * k + 2] * x0 + P.vA[(size_t)4 * k + 3] * x1;
                }
                for (int k = P.rpB[r]; k < P.rpB[r + 1]; ++k) {
                    const int c = col(P.cB[k], b, 1);
                    CHECK(c == P.colB[k]);
                    y0 += P.vB[(size_t)2 * k] * x[(size_t)P.nv + c];
                    y1 += P.vB[(size_t)2 * k + 1] * x[(size_t)P.nv + c];
                }
                y[(size_t)2 * r] = y0;
                y[(size_t)2 * r + 1] = y1;
            } else {
                const int p = r - P.nvp;
                double yp = 0.0;
                for (int k = P.rpC[p]; k < P.rpC[p + 1]; ++k) {
                    const int c = col(P.cC[k], b, 0);
                    CHECK(c == P.colC[k]);
                    yp += P.vC[(size_t)2 * k] * x[(size_t)2 * c] +
                          P.vC[(size_t)2 * k + 1] * x[(size_t)2 * c + 1];
                }
                y[(size_t)2 * P.nvp + p] = yp;
            }
        }
    return y;
}

static void test_products_and_slices(const HostCsr &F, const HostCsr &J) {
    const int nv = F.nrows, np = J.nrows;
    const HostCsr JT = dns::host_transpose(J);
    CHECK(JT.nrows == nv && JT.ncols == np && JT.nnz() == J.nnz());
    const HostCsr JTT = dns::host_transpose(JT);
    CHECK(JTT.rowptr == J.rowptr && JTT.colidx == J.colidx && JTT.vals == J.vals);
    // S = J JT against the dense product
    const HostCsr S = dns::host_spgemm(J, JT);
    const std::vector<double> jd = dense(J), sd = dense(S);
    for (int i = 0; i < np; ++i)
        for (int j = 0; j < np; ++j) {
            double ref = 0.0;
            for (int k = 0; k < nv; ++k)
                ref += jd[(size_t)i * nv + k] * jd[(size_t)j * nv + k];
            CHECK(std::fabs(ref - sd[(size_t)i * np + j]) <= 1e-13);
        }
    // [F, JT] and K slices of every block partition
    const HostCsr FJ = dns::host_hstack(F, JT);
    CHECK(FJ.ncols == nv + np && FJ.nnz() == F.nnz() + JT.nnz());
    const HostCsr K = dns::host_k_slice(F, JT, J, nv, 0, nv, 0, np);
    CHECK(K.nrows == nv + np && K.nnz() == F.nnz() + 2 * J.nnz());
    for (int P = 1; P <= 4; ++P) {
        const std::vector<int> sv = dns::partition_starts(nv, P),
                               sp = dns::partition_starts(np, P);
        CHECK(sv[0] == 0 && sv[P] == nv && sp[0] == 0 && sp[P] == np);
        int64_t nnz = 0;
        for (int r = 0; r < P; ++r) {
            CHECK((sv[r] & 1) == 0 && sv[r] <= sv[r + 1]);
            const HostCsr Kl = dns::host_k_slice(F, JT, J, nv, sv[r], sv[r + 1],
                                                 sp[r], sp[r + 1]);
            nnz += Kl.nnz();
            const HostCsr Fl = host_row_slice(F, sv[r], sv[r + 1]);
            CHECK(Fl.nrows == sv[r + 1] - sv[r]);
            for (int i = 0; i < Fl.nrows; ++i)
                CHECK(Fl.rowptr[i + 1] - Fl.rowptr[i] ==
                      F.rowptr[sv[r] + i + 1] - F.rowptr[sv[r] + i]);
        }
        CHECK(nnz == K.nnz());
    }
}

static void test_polynomial_rows(const HostCsr &F) {
    // D^-1 F, a degree-3 polynomial; the rows of a subset equal the rows of
    // the full build bit for bit (the partitioned set-up rests on that)
    const int nv = F.nrows;
    std::vector<double> dv((size_t)nv);
    HostCsr DF = F;
    for (int i = 0; i < nv; ++i) {
        double d = 1.0;
        for (int k = F.rowptr[i]; k < F.rowptr[i + 1]; ++k)
            if (F.colidx[k] == i) d = F.vals[k];
        dv[i] = 1.0 / d;
        for (int k = F.rowptr[i]; k < F.rowptr[i + 1]; ++k) DF.vals[k] *= dv[i];
    }
    const std::vector<double> c1 = {0.1, 0.05, 0.02}, c2 = {0.9, 0.8, 0.7};
    for (double tol : {0.0, 1e-3}) {
        const HostCsr G = dns::host_cheb_poly(DF, dv, 1.0, c1, c2, tol);
        CHECK(G.nrows == nv && G.rowptr[nv] == (int)G.colidx.size());
        std::vector<int> rows;
        for (int i = 0; i < nv; i += 3) rows.push_back(i);
        rows.push_back(nv - 1);
        std::sort(rows.begin(), rows.end());
        rows.erase(std::unique(rows.begin(), rows.end()), rows.end());
        const HostCsr Gs = dns::host_cheb_poly(DF, dv, 1.0, c1, c2, tol, &rows);
        size_t q = 0;
        for (int i = 0; i < nv; ++i) {
            const bool in = q < rows.size() && rows[q] == i;
            if (in) ++q;
            const int len = Gs.rowptr[i + 1] - Gs.rowptr[i];
            CHECK(len == (in ? G.rowptr[i + 1] - G.rowptr[i] : 0));
            for (int k = 0; in && k < len; ++k) {
                CHECK(Gs.colidx[Gs.rowptr[i] + k] == G.colidx[G.rowptr[i] + k]);
                CHECK(Gs.vals[Gs.rowptr[i] + k] == G.vals[G.rowptr[i] + k]);
            }
        }
        // empty row list: an empty matrix, not a crash
        const std::vector<int> none;
        const HostCsr G0 = dns::host_cheb_poly(DF, dv, 1.0, c1, c2, tol, &none);
        CHECK(G0.nnz() == 0 && (int)G0.rowptr.size() == nv + 1);
    }
}

// Rank-local construction: a block of rows embedded in the global shape, ghost
// rows merged in ring by ring, the polynomial rows of the block formed on the
// renumbered index set they reach -- equal, bit for bit, to the rows of the
// polynomial of the whole matrix (dist_solve.inc, build_explicit_part;
// rank_local.inc, extend_rows_for_setup)
static void test_rows_on_their_reach(const HostCsr &F) {
    const int nv = F.nrows;
    std::vector<double> dv((size_t)nv);
    for (int i = 0; i < nv; ++i) {
        double d = 1.0;
        for (int k = F.rowptr[i]; k < F.rowptr[i + 1]; ++k)
            if (F.colidx[k] == i) d = F.vals[k];
        dv[i] = 1.0 / d;
    }
    const std::vector<double> c1 = {0.1, 0.05, 0.02}, c2 = {0.9, 0.8, 0.7};
    const int degree = (int)c1.size() + 1;
    HostCsr DFw = F;
    dns::host_scale_rows(dv, DFw);
    const HostCsr Gw = dns::host_cheb_poly(DFw, dv, 1.0, c1, c2, 1e-3);
    for (int nranks : {1, 2, 3}) {
        const std::vector<int> st = dns::partition_starts(nv, nranks);
        for (int me = 0; me < nranks; ++me) {
            const int v0 = st[me], v1 = st[me + 1];
            // the own rows in the global shape
            const HostCsr blk = host_row_slice(F, v0, v1);
            const dns_csr bv = blk.view();
            HostCsr Fx = dns::host_embed_rows(&bv, v0, nv);
            CHECK(Fx.nrows == nv && Fx.nnz() == blk.nnz());
            for (int i = 0; i < nv; ++i)
                CHECK(Fx.rowptr[i + 1] - Fx.rowptr[i] ==
                      ((i >= v0 && i < v1) ? F.rowptr[i + 1] - F.rowptr[i] : 0));
            // ghost rows ring by ring (here: cut out of the whole matrix)
            std::vector<char> in((size_t)nv, 0);
            std::vector<int> fresh, rows;
            for (int i = v0; i < v1; ++i) {
                in[i] = 1;
                fresh.push_back(i);
                rows.push_back(i);
            }
            for (int s = 0; s < degree; ++s) {
                std::vector<int> want;
                for (int i : fresh)
                    if (i < v0 || i >= v1) want.push_back(i);
                HostCsr got;
                got.nrows = nv;
                got.ncols = nv;
                got.rowptr.assign((size_t)nv + 1, 0);
                for (int i : want) got.rowptr[(size_t)i + 1] = F.rowptr[i + 1] - F.rowptr[i];
                for (int i = 0; i < nv; ++i) got.rowptr[(size_t)i + 1] += got.rowptr[i];
                for (int i : want)
                    for (int k = F.rowptr[i]; k < F.rowptr[i + 1]; ++k) {
                        got.colidx.push_back(F.colidx[k]);
                        got.vals.push_back(F.vals[k]);
                    }
                if (!want.empty()) Fx = dns::host_merge_rows(Fx, got);
                if (s + 1 == degree) break;
                std::vector<int> next;
                for (int i : fresh)
                    for (int k = Fx.rowptr[i]; k < Fx.rowptr[i + 1]; ++k)
                        if (!in[Fx.colidx[k]]) {
                            in[Fx.colidx[k]] = 1;
                            next.push_back(Fx.colidx[k]);
                        }
                std::sort(next.begin(), next.end());
                fresh.swap(next);
            }
            // the index set the rows reach, renumbered
            std::vector<int> R, loc_of((size_t)nv, -1);
            for (int i = 0; i < nv; ++i)
                if (in[i]) R.push_back(i);
            for (size_t q = 0; q < R.size(); ++q) loc_of[R[q]] = (int)q;
            HostCsr DFx = Fx;
            dns::host_scale_rows(dv, DFx);
            const HostCsr DFc = dns::host_compact_rows(DFx, R, &loc_of);
            CHECK(DFc.nrows == (int)R.size() && DFc.ncols == (int)R.size());
            std::vector<double> dvc(R.size());
            for (size_t q = 0; q < R.size(); ++q) dvc[q] = dv[R[q]];
            std::vector<int> rows_c;
            for (int i : rows) rows_c.push_back(loc_of[i]);
            const HostCsr Gc = dns::host_cheb_poly(DFc, dvc, 1.0, c1, c2, 1e-3,
                                                   &rows_c);
            for (int i = v0; i < v1; ++i) {
                const int q = loc_of[i];
                const int len = Gc.rowptr[q + 1] - Gc.rowptr[q];
                CHECK(len == Gw.rowptr[i + 1] - Gw.rowptr[i]);
                for (int k = 0; k < len && k < Gw.rowptr[i + 1] - Gw.rowptr[i]; ++k) {
                    CHECK(R[Gc.colidx[Gc.rowptr[q] + k]] ==
                          Gw.colidx[Gw.rowptr[i] + k]);
                    CHECK(Gc.vals[Gc.rowptr[q] + k] == Gw.vals[Gw.rowptr[i] + k]);
                }
            }
            // rows kept global when no map is given
            const HostCsr Fr = dns::host_compact_rows(Fx, R, nullptr);
            CHECK(Fr.ncols == nv && Fr.nnz() == Fx.nnz());
        }
    }
}

static void test_pair_format(const HostCsr &F, const HostCsr &J) {
    const int nv = F.nrows, np = J.nrows, n = nv + np;
    const HostCsr JT = dns::host_transpose(J);
    const HostCsr K = dns::host_k_slice(F, JT, J, nv, 0, nv, 0, np);
    std::vector<double> x((size_t)n), yref((size_t)n);
    unsigned seed = 99u;
    for (double &v : x) v = lcg(seed);
    dns::host_spmv(K, x, yref);
    dns::HostPair P;
    const char *why = nullptr;
    CHECK(dns::host_pair_from_k(K, nv, P, &why));
    const std::vector<double> y = pair_apply(P, x);
    for (int i = 0; i < n; ++i) CHECK(std::fabs(y[i] - yref[i]) <= 1e-13);
    // row blocks of 1..4 ranks: local rows, global columns
    for (int R = 2; R <= 4; ++R) {
        const std::vector<int> sv = dns::partition_starts(nv, R),
                               sp = dns::partition_starts(np, R);
        for (int r = 0; r < R; ++r) {
            const HostCsr Kl = dns::host_k_slice(F, JT, J, nv, sv[r], sv[r + 1],
                                                 sp[r], sp[r + 1]);
            dns::HostPair Pl;
            if (Kl.nrows == 0) continue;
            CHECK(dns::host_pair_from_k(Kl, nv, Pl, &why, sv[r + 1] - sv[r],
                                        sv[r], sp[r]));
            const std::vector<double> yl = pair_apply(Pl, x);
            for (int i = 0; i < sv[r + 1] - sv[r]; ++i)
                CHECK(std::fabs(yl[i] - yref[sv[r] + i]) <= 1e-13);
            for (int i = 0; i < sp[r + 1] - sp[r]; ++i)
                CHECK(std::fabs(yl[(size_t)(sv[r + 1] - sv[r]) + i] -
                                yref[(size_t)nv + sp[r] + i]) <= 1e-13);
        }
    }
    // refusals instead of out-of-range writes: odd velocity count, an entry in
    // the pressure-pressure block
    dns::HostPair Q;
    HostCsr Kodd = dns::host_k_slice(F, JT, J, nv, 0, nv, 0, np);
    CHECK(!dns::host_pair_from_k(Kodd, nv - 1, Q, &why));
    HostCsr Kpp = K;
    Kpp.colidx.back() = n - 1;          // last pressure row, last column
    CHECK(!dns::host_pair_from_k(Kpp, nv, Q, &why));
}

static void test_halo_lists(const HostCsr &F, const HostCsr &J) {
    const int nv = F.nrows, np = J.nrows;
    const dns_csr fv = F.view(), jv = J.view();
    for (int P = 1; P <= 4; ++P) {
        const std::vector<int> sv = dns::partition_starts(nv, P),
                               sp = dns::partition_starts(np, P);
        std::vector<std::vector<std::vector<int>>> need((size_t)P);
        for (int r = 0; r < P; ++r) {
            dns::halo_need(&fv, sv[r], sv[r + 1], P, r, sv.data(), nv, need[r]);
            CHECK(need[r][r].empty());
            std::vector<std::vector<int>> nj;
            dns::halo_need(&jv, sp[r], sp[r + 1], P, r, sv.data(), nv, nj);
            CHECK(nj[r].empty());
            // every off-rank column of the rank's rows is in exactly one list
            for (int i = sv[r]; i < sv[r + 1]; ++i)
                for (int k = F.rowptr[i]; k < F.rowptr[i + 1]; ++k) {
                    const int c = F.colidx[k];
                    if (c >= sv[r] && c < sv[r + 1]) continue;
                    int hits = 0;
                    for (int q = 0; q < P; ++q)
                        hits += (int)std::count(need[r][q].begin(),
                                                need[r][q].end(), c);
                    CHECK(hits == 1);
                }
            for (int q = 0; q < P; ++q)
                for (size_t k = 0; k < need[r][q].size(); ++k) {
                    CHECK(need[r][q][k] >= sv[q] && need[r][q][k] < sv[q + 1]);
                    CHECK(k == 0 || need[r][q][k - 1] < need[r][q][k]);
                }
        }
    }
    // more ranks than rows, no rows at all
    const std::vector<int> tiny = dns::partition_starts(3, 8);
    CHECK(tiny[0] == 0 && tiny[8] == 3);
    for (int r = 0; r < 8; ++r) CHECK(tiny[r] <= tiny[r + 1]);
    const std::vector<int> zero = dns::partition_starts(0, 4);
    for (int r = 0; r <= 4; ++r) CHECK(zero[r] == 0);
}

static void test_misc(const HostCsr &F) {
    HostCsr A = F;
    dns::host_drop_small(A, 0.03);
    CHECK(A.nnz() <= F.nnz() && A.rowptr.back() == (int)A.colidx.size());
    const HostCsr T = dns::host_transpose(F);
    const HostCsr sum = dns::host_add(1.0, F, -1.0, T);
    CHECK(sum.nrows == F.nrows);
    double lmin = 0.0, lmax = 0.0;
    dns::host_jacobi_bounds(F, &lmin, &lmax);
    CHECK(lmax >= lmin && lmax > 0.0);
    const double eta = dns::host_skew_radius(F, T);
    CHECK(eta >= 0.0 && std::isfinite(eta));
    std::vector<double> d((size_t)F.nrows, 2.0);
    const HostCsr D = dns::host_diag(d);
    const HostCsr DF = dns::host_spgemm(D, F);
    CHECK(DF.nnz() == F.nnz());
    for (int64_t k = 0; k < F.nnz(); ++k)
        CHECK(std::fabs(DF.vals[k] - 2.0 * F.vals[k]) <= 1e-15);
    // a matrix with empty rows and an empty matrix go through every routine
    HostCsr E;
    E.nrows = 5;
    E.ncols = 5;
    E.rowptr.assign(6, 0);
    const HostCsr ET = dns::host_transpose(E);
    CHECK(ET.nnz() == 0);
    const HostCsr EE = dns::host_spgemm(E, E);
    CHECK(EE.nnz() == 0 && (int)EE.rowptr.size() == 6);
    const HostCsr Es = host_row_slice(E, 2, 2);
    CHECK(Es.nrows == 0 && Es.nnz() == 0);
}

// ---- multigrid levels (mg_host.hpp) ----

// y = A x, dense restatement
static std::vector<double> matvec(const HostCsr &A, const std::vector<double> &x) {
    std::vector<double> y((size_t)A.nrows, 0.0);
    const std::vector<double> d = dense(A);
    for (int i = 0; i < A.nrows; ++i)
        for (int j = 0; j < A.ncols; ++j)
            y[i] += d[(size_t)i * A.ncols + j] * x[j];
    return y;
}

static std::vector<double> cat(const std::vector<double> &a,
                               const std::vector<double> &b) {
    std::vector<double> c = a;
    c.insert(c.end(), b.begin(), b.end());
    return c;
}

static bool close_to(const std::vector<double> &a, const std::vector<double> &b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (std::fabs(a[i] - b[i]) > 1e-12 * (1.0 + std::fabs(b[i])))
            return false;
    return true;
}

static bool same_csr(const HostCsr &a, const HostCsr &b) {
    return a.nrows == b.nrows && a.ncols == b.ncols && a.rowptr == b.rowptr &&
           a.colidx == b.colidx && a.vals == b.vals;
}

// the rows of `blk` below those of `acc`
static void append_rows(HostCsr &acc, const HostCsr &blk) {
    if (acc.rowptr.empty()) acc.rowptr.push_back(0);
    acc.ncols = blk.ncols;
    for (int i = 0; i < blk.nrows; ++i)
        acc.rowptr.push_back(acc.rowptr.back() + blk.rowptr[i + 1] -
                             blk.rowptr[i]);
    acc.nrows += blk.nrows;
    acc.colidx.insert(acc.colidx.end(), blk.colidx.begin(), blk.colidx.end());
    acc.vals.insert(acc.vals.end(), blk.vals.begin(), blk.vals.end());
}

// a pressure-like Schur operator S = J diag(F)^-1 J^T and an aggregation
// prolongation: aggregates of 3 (the last one shorter), weights around 1,
// column 1 an empty aggregate
static void build_level(const HostCsr &F, const HostCsr &J, HostCsr &S,
                        HostCsr &P) {
    std::vector<double> df((size_t)F.nrows, 1.0);
    for (int i = 0; i < F.nrows; ++i)
        for (int k = F.rowptr[i]; k < F.rowptr[i + 1]; ++k)
            if (F.colidx[k] == i) df[i] = 1.0 / F.vals[k];
    HostCsr JD = J;
    for (int64_t k = 0; k < JD.nnz(); ++k) JD.vals[k] *= df[JD.colidx[k]];
    S = dns::host_spgemm(JD, dns::host_transpose(J));
    const int n = S.nrows, nagg = (n + 2) / 3;
    unsigned seed = 777u;
    std::vector<std::map<int, double>> pr((size_t)n);
    for (int i = 0; i < n; ++i) {
        const int a = i / 3;
        pr[i][a < 1 ? a : a + 1] = 1.0 + 0.2 * lcg(seed);
    }
    P = from_map(n, nagg + 1, pr);
}

// all-gather of host vectors between threads that stand for ranks
struct HostAllgather {
    std::mutex m;
    std::condition_variable cv;
    int nranks = 1, arrived = 0, generation = 0;
    std::vector<double> buf;
    void barrier() {
        std::unique_lock<std::mutex> lk(m);
        const int g = generation;
        if (++arrived == nranks) {
            arrived = 0;
            ++generation;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return generation != g; });
        }
    }
    int operator()(std::vector<double> &v, const std::vector<int> &st, int me) {
        {
            std::lock_guard<std::mutex> lk(m);
            buf.resize(v.size());
            for (int i = st[me]; i < st[me + 1]; ++i) buf[i] = v[i];
        }
        barrier();
        {
            std::lock_guard<std::mutex> lk(m);
            v = buf;
        }
        barrier();
        return 0;
    }
};

static void test_mg_levels(const HostCsr &F, const HostCsr &J) {
    HostCsr S, P;
    build_level(F, J, S, P);
    const int n = S.nrows, nc = P.ncols;
    const HostCsr PT = dns::host_transpose(P), SP = dns::host_spgemm(S, P);
    // the whole level
    std::vector<double> dv, dj;
    dns::mg_diagonals(S, 0, n, dv, dj);
    double lmax = 0.0;
    CHECK(dns::mg_jacobi_lmax(S, 0, n, dj,
                              [](std::vector<double> &) { return 0; },
                              &lmax) == 0);
    double w1 = 0.0, w2 = 0.0, w = 0.0, wj = 0.0;
    dns::mg_damping(lmax, true, 3.0, &w1, &w2);
    dns::mg_damping(lmax, false, 3.0, &w, &wj);
    const dns::MgOps o = dns::mg_fused22_ops(S, SP, P, PT, 0, n, dv, w1, w2);
    const HostCsr Sc = dns::host_spgemm(PT, SP);
    // damping: the closed forms
    CHECK(lmax > 0.0 && w == 4.0 / (3.0 * lmax) && wj == w);
    {
        const double hi = 1.05 * lmax, lo = lmax / 3.0;
        const double mid = 0.5 * (hi + lo), rad = 0.5 * (hi - lo);
        // (1 - w1 t)(1 - w2 t) = T_2((mid - t) / rad) / T_2(mid / rad)
        for (double t : {lo, 0.5 * (lo + hi), hi, 0.1 * lmax}) {
            const double s = (mid - t) / rad, s0 = mid / rad;
            const double ref = (2 * s * s - 1) / (2 * s0 * s0 - 1);
            CHECK(std::fabs((1 - w1 * t) * (1 - w2 * t) - ref) <= 1e-12);
        }
        CHECK(w1 < w2 && w1 > 0.0);
        double a = 0.0, b = 0.0;
        dns::mg_damping(0.0, false, 3.0, &a, &b);
        CHECK(a == 4.0 / 3e-300 && b == a);
    }
    // the operators do what their comments say, against dense loops
    unsigned seed = 99u;
    std::vector<double> b((size_t)n), x((size_t)n), e((size_t)nc);
    for (double &v : b) v = lcg(seed);
    for (double &v : x) v = lcg(seed);
    for (double &v : e) v = lcg(seed);
    auto sweep = [&](const std::vector<double> &x0, double om) {
        const std::vector<double> sx = matvec(S, x0);
        std::vector<double> y = x0;
        for (int i = 0; i < n; ++i) y[i] += om * dv[i] * (b[i] - sx[i]);
        return y;
    };
    auto restrict_ = [&](const std::vector<double> &r) { return matvec(PT, r); };
    {
        // Apre b: two damped Jacobi sweeps from zero
        CHECK(close_to(matvec(o.Apre, b),
                   sweep(sweep(std::vector<double>((size_t)n, 0.0), w1), w2)));
        // Rr [b; x] = P^T (b - S x)
        std::vector<double> r = matvec(S, x);
        for (int i = 0; i < n; ++i) r[i] = b[i] - r[i];
        CHECK(close_to(matvec(o.Rr, cat(b, x)), restrict_(r)));
        // Qq [x; e] + w1 D^-1 b = one sweep on x + P e
        std::vector<double> q = matvec(o.Qq, cat(x, e));
        std::vector<double> xp = matvec(P, e);
        for (int i = 0; i < n; ++i) {
            q[i] += w1 * dv[i] * b[i];
            xp[i] += x[i];
        }
        CHECK(close_to(q, sweep(xp, w1)));
    }
    for (bool finest : {true, false}) {
        const dns::MgOps u =
            dns::mg_fused11_ops(S, SP, P, PT, 0, n, dv, w, finest);
        CHECK(u.Apre.nrows == 0);
        // Rd b = P^T (b - S w D^-1 b)
        std::vector<double> c((size_t)n);
        for (int i = 0; i < n; ++i) c[i] = w * dv[i] * b[i];
        std::vector<double> r = matvec(S, c);
        for (int i = 0; i < n; ++i) r[i] = b[i] - r[i];
        CHECK(close_to(matvec(u.Rr, b), restrict_(r)));
        // U [b; e] = (I + T) w D^-1 b + T P e, T = I - w D^-1 S
        std::vector<double> y = matvec(P, e);
        for (int i = 0; i < n; ++i) y[i] += c[i];
        const std::vector<double> sy = matvec(S, y);
        for (int i = 0; i < n; ++i) {
            y[i] += c[i] - w * dv[i] * sy[i];
            if (finest) y[i] = -y[i];
        }
        CHECK(close_to(matvec(u.Qq, cat(b, e)), y));
    }
    for (int R = 1; R <= 4; ++R) {
        const std::vector<int> st = dns::partition_starts(n, R),
                               stc = dns::partition_starts(nc, R);
        // rows equal whole: every rank's set-up as mg_rows.inc runs it, the
        // all-gathers between threads
        std::vector<dns::MgOps> ops((size_t)R);
        std::vector<HostCsr> next((size_t)R);
        std::vector<std::vector<double>> dvs((size_t)R);
        std::vector<double> lm((size_t)R, 0.0), om1((size_t)R), om2((size_t)R);
        HostAllgather ag;
        ag.nranks = R;
        auto rank = [&](int me) {
            const int f0 = st[me], f1 = st[me + 1];
            const HostCsr Sloc = host_row_slice(S, f0, f1);
            const dns_csr slv = Sloc.view();
            const HostCsr Sg = dns::host_embed_rows(&slv, f0, n);
            std::vector<double> djr;
            dns::mg_diagonals(Sg, f0, f1, dvs[me], djr);
            ag(dvs[me], st, me);
            auto ex = [&](std::vector<double> &y) { return ag(y, st, me); };
            CHECK(dns::mg_jacobi_lmax(Sg, f0, f1, djr, ex, &lm[me]) == 0);
            dns::mg_damping(lm[me], true, 3.0, &om1[me], &om2[me]);
            const HostCsr PTc = host_row_slice(PT, stc[me], stc[me + 1]);
            // own rows + the rows the own rows of P^T reference
            std::vector<char> keep((size_t)n, 0);
            for (int i = f0; i < f1; ++i) keep[i] = 1;
            for (int c : PTc.colidx) keep[c] = 1;
            HostCsr Sx = S;
            for (int i = 0, k = 0; i < n; ++i) {
                if (!keep[i]) {
                    const int len = Sx.rowptr[i + 1] - Sx.rowptr[i];
                    Sx.colidx.erase(Sx.colidx.begin() + k,
                                    Sx.colidx.begin() + k + len);
                    Sx.vals.erase(Sx.vals.begin() + k, Sx.vals.begin() + k + len);
                    for (int j = i + 1; j <= n; ++j) Sx.rowptr[j] -= len;
                }
                k = Sx.rowptr[i + 1];
            }
            const HostCsr SPx = dns::host_spgemm(Sx, P);
            ops[me] = dns::mg_fused22_ops(Sx, SPx, P, PTc, f0, f1, dvs[me],
                                          om1[me], om2[me]);
            next[me] = dns::host_spgemm(PTc, SPx);
        };
        std::vector<std::thread> th;
        for (int me = 0; me < R; ++me) th.emplace_back(rank, me);
        for (auto &t : th) t.join();
        HostCsr Ap, Rr, Qq, Sn;
        for (int me = 0; me < R; ++me) {
            CHECK(dvs[me] == dv && lm[me] == lmax);
            CHECK(om1[me] == w1 && om2[me] == w2);
            append_rows(Ap, ops[me].Apre);
            append_rows(Rr, ops[me].Rr);
            append_rows(Qq, ops[me].Qq);
            append_rows(Sn, next[me]);
        }
        CHECK(same_csr(Ap, o.Apre) && same_csr(Rr, o.Rr));
        CHECK(same_csr(Qq, o.Qq) && same_csr(Sn, Sc));
        // need lists: whole operators cut by ranges (setup_dist_mg) and the
        // rank's own blocks (mg_rows.inc) against a scan of every column
        for (bool crep : {true, false})
            for (int me = 0; me < R; ++me) {
                const int f0 = st[me], f1 = st[me + 1], c0 = stc[me],
                          c1 = stc[me + 1];
                std::vector<std::vector<int>> nf, ncl, nf2, ncl2;
                dns::mg_need_lists(S, o.Apre, o.Qq, f0, f1, o.Rr, c0, c1, st,
                                   stc, me, crep, nf, ncl);
                dns::mg_need_lists(host_row_slice(S, f0, f1), ops[me].Apre,
                                   ops[me].Qq, 0, f1 - f0, ops[me].Rr, 0,
                                   c1 - c0, st, stc, me, crep, nf2, ncl2);
                CHECK(nf == nf2 && ncl == ncl2);
                auto refs = [](const HostCsr &A, int r0, int r1, int c) {
                    for (int i = r0; i < r1; ++i)
                        for (int k = A.rowptr[i]; k < A.rowptr[i + 1]; ++k)
                            if (A.colidx[k] == c) return true;
                    return false;
                };
                for (int q = 0; q < R; ++q) {
                    std::vector<int> wf, wc;
                    for (int c = st[q]; q != me && c < st[q + 1]; ++c)
                        if (refs(S, f0, f1, c) || refs(o.Apre, f0, f1, c) ||
                            refs(o.Qq, f0, f1, c) || refs(o.Rr, c0, c1, c) ||
                            refs(o.Rr, c0, c1, n + c))
                            wf.push_back(c);
                    for (int c = stc[q]; !crep && q != me && c < stc[q + 1]; ++c)
                        if (refs(o.Qq, f0, f1, n + c)) wc.push_back(c);
                    CHECK((int)nf.size() == R && (int)ncl.size() == R);
                    CHECK(nf[q] == wf && ncl[q] == wc);
                }
            }
    }
}

// every branch of the batch policy: state before, a batch that went through
// (or the start-up / fallback), state after -- the expected values worked out
// from the arithmetic as dns_imex_run had it inline
static bool same(const dns::BatchPolicy &a, const dns::BatchPolicy &b) {
    return a.cpred == b.cpred && a.noslack == b.noslack &&
           a.noslack_hold == b.noslack_hold && a.lower_hold == b.lower_hold &&
           a.lower_backoff == b.lower_backoff &&
           a.lowered_last == b.lowered_last && a.spiked == b.spiked &&
           a.batch_len == b.batch_len;
}

static void test_batch_policy() {
    using dns::BatchPolicy;
    // {cpred, noslack, noslack_hold, lower_hold, lower_backoff, lowered_last,
    //  spiked, batch_len}
    const BatchPolicy fresh;
    CHECK(same(fresh, BatchPolicy{-1, false, 1, 0, 2, false, false, 8}));
    // {cmin, raise, lower, two_one, slack_adapt, noslack_maxrel}
    const dns::BatchParams P{1, 0.9, 0.25, false, true, 0.85};
    const dns::BatchParams P2{2, 0.9, 0.25, false, true, 0.85};
    const dns::BatchParams PT{1, 0.9, 0.25, true, true, 0.85};
    const dns::BatchParams PN{1, 0.9, 0.25, false, false, 0.85};
    const bool F = false, T = true;
    struct Case {
        const char *what;
        BatchPolicy before;
        dns::BatchOutcome r;   // {over, c_first, c, replayed, maxit, maxrel, maxprev}
        dns::BatchParams p;
        BatchPolicy after;
    };
    const Case cases[] = {
        // slack step (no oversolve)
        {"no slack: a margin below the bound", {4, F, 1, 0, 2, F, F, 8},
         {F, 4, 4, F, 3, 0.5, 0.0}, P, {4, T, 0, 0, 2, F, F, 16}},
        {"no slack: as many steps as the cycle", {4, F, 1, 0, 2, F, F, 8},
         {F, 4, 4, F, 4, 0.5, 0.0}, P, {5, T, 0, 0, 2, F, F, 16}},
        {"slack: batch maximum at the bound", {4, T, 0, 0, 2, F, F, 16},
         {F, 3, 3, F, 3, 0.85, 0.0}, P, {4, F, 0, 0, 2, F, F, 32}},
        {"slack: more steps than the cycle", {4, F, 0, 0, 2, F, F, 32},
         {F, 4, 4, F, 5, 0.5, 0.0}, P, {6, F, 0, 0, 2, F, F, 32}},
        {"slack: no residual recorded", {4, F, 0, 0, 2, F, F, 8},
         {F, 4, 4, F, 3, 0.0, 0.0}, P, {4, F, 0, 0, 2, F, F, 16}},
        {"slack: DNS_SLACK_ADAPT=0", {4, F, 0, 0, 2, F, F, 8},
         {F, 4, 4, F, 3, 0.5, 0.0}, PN, {4, F, 0, 0, 2, F, F, 16}},
        {"hold: a replayed batch keeps the slack step", {4, T, 0, 0, 2, F, F, 16},
         {F, 3, 5, T, 4, 0.5, 0.0}, P, {5, F, 3, 0, 2, F, F, 32}},
        {"hold: counts down", {5, F, 3, 0, 2, F, F, 32},
         {F, 5, 5, F, 4, 0.5, 0.0}, P, {5, F, 2, 0, 2, F, F, 32}},
        {"hold: runs out", {5, F, 1, 0, 2, F, F, 32},
         {F, 5, 5, F, 4, 0.5, 0.0}, P, {5, T, 0, 0, 2, F, F, 32}},
        // oversolve
        {"spike: the first replay keeps the cycle", {2, F, 0, 0, 2, F, F, 16},
         {T, 2, 4, T, 3, 0.5, 0.1}, P, {2, F, 3, 0, 2, F, T, 32}},
        {"spike twice: raise", {2, F, 3, 0, 2, F, T, 32},
         {T, 2, 4, T, 3, 0.5, 0.1}, P, {3, F, 3, 3, 2, F, F, 32}},
        {"spike: cleared by a batch without a replay", {2, F, 0, 0, 2, F, T, 16},
         {T, 2, 2, F, 2, 0.5, 0.3}, P, {2, F, 0, 0, 2, F, F, 32}},
        {"raise: ended close to the tolerance", {2, F, 0, 0, 2, F, F, 8},
         {T, 2, 2, F, 2, 0.95, 0.3}, P, {3, F, 0, 3, 2, F, F, 16}},
        {"floor: down to what was run", {4, F, 0, 0, 2, F, F, 8},
         {T, 4, 4, F, 2, 0.01, 0.001}, P, {2, F, 0, 0, 2, F, F, 16}},
        {"floor: not below cmin", {4, F, 0, 0, 2, F, F, 8},
         {T, 4, 4, F, 1, 0.01, 0.001}, P2, {2, F, 0, 0, 2, F, F, 16}},
        {"trial: a decade below in front of the last column",
         {3, F, 0, 0, 2, F, F, 32}, {T, 3, 3, F, 3, 0.5, 0.1}, P,
         {2, F, 0, 0, 2, T, F, 8}},
        {"trial, second form: two V-cycles in one column",
         {2, F, 0, 0, 2, F, F, 32}, {T, 2, 2, F, 2, 0.4, 0.5}, PT,
         {1, F, 0, 0, 2, T, F, 8}},
        {"second form: only with two V-cycles", {2, F, 0, 0, 2, F, F, 32},
         {T, 2, 2, F, 2, 0.4, 0.5}, P, {2, F, 0, 0, 2, F, F, 32}},
        {"second form: only with a margin", {2, F, 0, 0, 2, F, F, 32},
         {T, 2, 2, F, 2, 0.6, 0.5}, PT, {2, F, 0, 0, 2, F, F, 32}},
        {"no trial while held", {3, F, 0, 2, 2, F, F, 32},
         {T, 3, 3, F, 3, 0.5, 0.1}, P, {3, F, 0, 1, 2, F, F, 32}},
        {"no trial at cmin", {2, F, 0, 0, 2, F, F, 32},
         {T, 2, 2, F, 2, 0.5, 0.1}, P2, {2, F, 0, 0, 2, F, F, 32}},
        {"no trial without a residual in front", {3, F, 0, 0, 2, F, F, 32},
         {T, 3, 3, F, 3, 0.5, 0.0}, P, {3, F, 0, 0, 2, F, F, 32}},
        {"failed trial: the back-off doubles", {2, F, 0, 0, 2, T, F, 8},
         {T, 2, 4, T, 3, 0.5, 0.1}, P, {3, F, 3, 3, 4, F, F, 16}},
        {"trial ended close: the back-off doubles", {2, F, 0, 0, 2, T, F, 8},
         {T, 2, 2, F, 2, 0.95, 0.3}, P, {3, F, 0, 3, 4, F, F, 16}},
        {"back-off capped at 1024", {2, F, 0, 0, 600, T, F, 8},
         {T, 2, 4, T, 3, 0.5, 0.1}, P, {3, F, 3, 1023, 1024, F, F, 16}},
        {"back-off stays at 1024", {2, F, 0, 0, 1024, T, F, 8},
         {T, 2, 4, T, 3, 0.5, 0.1}, P, {3, F, 3, 1023, 1024, F, F, 16}},
    };
    for (const Case &c : cases) {
        BatchPolicy pol = c.before;
        pol.after_batch(c.r, c.p);
        if (!same(pol, c.after)) {
            fprintf(stderr, "batch policy: %s\n", c.what);
            ++g_fail;
        }
    }
    // start-up: a stepper without its history steps synchronously first
    CHECK(fresh.startup_steps(0) == 5 && fresh.startup_steps(3) == 2);
    CHECK(fresh.startup_steps(4) == 2 && fresh.startup_steps(5) == 2);
    BatchPolicy pol{3, T, 0, 5, 8, T, T, 32};
    CHECK(pol.startup_steps(5) == 0 && pol.startup_steps(4) == 2);
    pol.after_startup(3);
    CHECK(same(pol, BatchPolicy{4, F, 1, 5, 8, T, T, 8}));
    pol.after_startup(-1);
    CHECK(pol.cpred == 2);
    // fallback: a batch that failed twice and ran step by step
    pol = BatchPolicy{3, T, 0, 5, 8, T, T, 32};
    pol.after_fallback(5);
    CHECK(same(pol, BatchPolicy{7, F, 8, 5, 8, T, T, 8}));
    pol.after_fallback(0);
    CHECK(pol.cpred == 3);
    // first attempt's cycle (oversolve / no slack step / slack step) and the
    // second attempt's
    CHECK(fresh.cycle(true) == 1 && fresh.cycle(false) == 2);
    CHECK((BatchPolicy{3, F}.cycle(true) == 3));
    CHECK((BatchPolicy{3, F}.cycle(false) == 3));
    CHECK((BatchPolicy{4, T}.cycle(false) == 3));
    CHECK((BatchPolicy{1, T}.cycle(false) == 1));
    CHECK((BatchPolicy{4, T}.cycle(true) == 4));   // (no slack step to drop)
    CHECK(BatchPolicy::longer(3, 64) == 5 && BatchPolicy::longer(63, 64) == 64);
    CHECK(BatchPolicy::longer(1, 1) == 1);
    // batch length 8 -> 16 -> 32 while the predictions hold
    pol = fresh;
    pol.after_startup(2);
    const dns::BatchOutcome good{F, 3, 3, F, 2, 0.5, 0.0};
    for (int len : {16, 32, 32}) {
        pol.after_batch(good, P);
        CHECK(pol.batch_len == len);
    }
}

// the ring: every rotation moves each solution back by one and makes the
// oldest the work buffer; the indices stay a permutation of 0..5, nsol
// saturates at 5, and six rotations are the identity
static bool is_reset(const dns::Ring &r) {
    return r.cur == 0 && r.prev == 1 && r.pprev == 2 && r.p3 == 3 &&
           r.p4 == 4 && r.work == 5;
}

static void test_ring() {
    dns::Ring r;
    CHECK(is_reset(r) && r.nsol == 0 && !r.pre_ok);
    r.reset(1);
    CHECK(is_reset(r) && r.nsol == 1 && !r.pre_ok);
    for (int k = 1; k <= 13; ++k) {
        const dns::Ring b = r;
        r.rotate();
        CHECK(r.cur == b.work && r.prev == b.cur && r.pprev == b.prev &&
              r.p3 == b.pprev && r.p4 == b.p3 && r.work == b.p4);
        const int idx[6] = {r.cur, r.prev, r.pprev, r.p3, r.p4, r.work};
        int seen = 0;
        for (int i : idx) {
            CHECK(i >= 0 && i < 6);
            if (i >= 0 && i < 6) seen |= 1 << i;
        }
        CHECK(seen == 63);
        CHECK(r.nsol == std::min(1 + k, 5));
        CHECK(r.cur == (6 - k % 6) % 6);
        CHECK(is_reset(r) == (k % 6 == 0));
    }
    r.pre_ok = true;
    r.pre_sig = 7;
    r.reset(2);
    CHECK(is_reset(r) && r.nsol == 2 && !r.pre_ok);
    // one signature per (nsol, order up to 7); nsol saturates at 5 like the ring
    for (int n = 0; n <= 5; ++n)
        for (int x = 0; x <= 13; ++x) {
            CHECK(dns::extrap_sig(n, x) == 8 * n + std::min(x, 7));
            CHECK(dns::extrap_sig(n + 3, x) == dns::extrap_sig(std::min(n + 3, 5), x));
        }
}

// sum_i e_i q(-i) for q(t) = t^d: the solutions sit at t = 0, -1, .., -4 (cur
// first), the warm start is their value at t = 1
static double extrap_moment(const double e[5], int d) {
    double s = 0.0;
    for (int i = 0; i < 5; ++i) s += e[i] * std::pow(-(double)i, d);
    return s;
}

// the warm-start coefficients: they sum to one, order p reproduces degree p
// at the integer nodes exactly (the least-squares fit: a cubic), and capped
// at the quartic they are the ladder the trapezoidal stepper had on its own
static void test_extrap_coeffs() {
    // the trapezoidal ladder, order by [nsol - 1][extrapolate_x0 = 0..13]
    static const int kTrapOrder[5][14] = {
        {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0},
        {0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1},
        {0, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2},
        {0, 1, 2, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3},
        {0, 1, 2, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4},
    };
    // ... and its coefficients by order (0: a copy of x_c)
    static const double kTrapCoef[5][5] = {
        {1.0, 0.0, 0.0, 0.0, 0.0},
        {2.0, -1.0, 0.0, 0.0, 0.0},
        {3.0, -3.0, 1.0, 0.0, 0.0},
        {4.0, -6.0, 4.0, -1.0, 0.0},
        {5.0, -10.0, 10.0, -5.0, 1.0},
    };
    for (int n = 1; n <= 5; ++n)
        for (int x = -1; x <= 13; ++x) {
            double e[5];
            const int p = dns::extrap_coeffs(n, x, e);
            const bool fit = x == dns::kExtrapFit35 && n >= 5;
            const int want = x == dns::kExtrapFit35
                                 ? std::min(3, n - 1)
                                 : std::max(0, std::min({x, 4, n - 1}));
            CHECK(p == want);
            double sum = 0.0;
            for (int i = 0; i < 5; ++i) sum += e[i];
            CHECK(std::fabs(sum - 1.0) <= 1e-14);
            for (int d = 0; d <= p; ++d) {
                const double m = extrap_moment(e, d);
                if (fit)
                    CHECK(std::fabs(m - 1.0) <= 1e-12);
                else
                    CHECK(m == 1.0);
            }
            if (!fit) {
                // (interpolating: order p and no more, on the last p + 1)
                CHECK(extrap_moment(e, p + 1) != 1.0);
                for (int i = p + 1; i < 5; ++i) CHECK(e[i] == 0.0);
            }
            if (x < 0) continue;
            const int pt = dns::extrap_coeffs(n, std::min(x, 4), e);
            CHECK(pt == kTrapOrder[n - 1][x]);
            for (int i = 0; i < 5; ++i) CHECK(e[i] == kTrapCoef[pt][i]);
        }
}

// ---- the exception barrier (status.hpp) ----
// local functions written exactly like an export: a function-try-block with
// the body in place, closed by the macro

static int g_exits = 0;   // ScopeExit bodies that have run
static int g_live = 0;    // Counted objects alive

struct Counted {
    Counted() { ++g_live; }
    ~Counted() { --g_live; }
    std::vector<double> payload = std::vector<double>(64, 1.0);
};

extern "C" {

int barrier_throws(int what) try {
    dns::ScopeExit leave([] { ++g_exits; });
    if (what == 0) throw std::bad_alloc();
    if (what == 1) throw std::runtime_error("boom");
    if (what == 2) throw 5;
    if (what == 3) return (int)std::vector<int>(2).at(7);
    return DNS_OK;
} DNS_CAPI_CATCH

static int refuses() { return dns::fail(DNS_ERR_NOT_READY, "not set up"); }

int barrier_passes_status(int *after) try {
    dns::ScopeExit leave([] { ++g_exits; });
    DNS_TRY(refuses());
    *after = 1;
    return DNS_OK;
} DNS_CAPI_CATCH

// a create function: the handle is owned until it is handed out
int barrier_create(int fail_how, Counted **out) try {
    if (!out) return dns::fail(DNS_ERR_BAD_ARGUMENT, "null output handle");
    *out = nullptr;
    auto h = std::make_unique<Counted>();
    if (fail_how == 1) throw std::runtime_error("set-up thread failed");
    if (fail_how == 2) DNS_TRY(refuses());
    *out = h.release();
    return DNS_OK;
} DNS_CAPI_CATCH

}  // extern "C"

static void test_barrier() {
    // (dns::g_last_error is the string dns_last_error() hands out; the export
    // itself lives in the HIP translation unit and cannot be linked here)
    const struct {
        int what;
        const char *msg;
        bool whole;
    } throwers[] = {{0, "out of host memory", true},
                    {1, "boom", false},
                    {2, "host-side exception", true}};
    for (const auto &c : throwers) {
        dns::g_last_error.clear();
        g_exits = 0;
        CHECK(barrier_throws(c.what) == DNS_ERR_HOST);
        CHECK(g_exits == 1);
        if (c.whole)
            CHECK(dns::g_last_error == c.msg);
        else
            CHECK(dns::g_last_error.find(c.msg) != std::string::npos);
    }
    // a library exception (std::out_of_range) by its what()
    CHECK(barrier_throws(3) == DNS_ERR_HOST);
    CHECK(dns::g_last_error.find("host-side exception: ") == 0);
    g_exits = 0;
    CHECK(barrier_throws(4) == DNS_OK && g_exits == 1);
    // a failing status passes through unchanged, with its own message, and
    // the ScopeExit has run by the time it is returned
    int after = 0;
    g_exits = 0;
    CHECK(barrier_passes_status(&after) == DNS_ERR_NOT_READY);
    CHECK(after == 0 && g_exits == 1);
    CHECK(dns::g_last_error == "not set up");
    // an owned handle: freed on an exception and on a status, handed out once
    Counted *h = reinterpret_cast<Counted *>(&after);
    CHECK(barrier_create(1, &h) == DNS_ERR_HOST && h == nullptr);
    CHECK(g_live == 0);
    CHECK(dns::g_last_error.find("set-up thread failed") != std::string::npos);
    h = reinterpret_cast<Counted *>(&after);
    CHECK(barrier_create(2, &h) == DNS_ERR_NOT_READY && h == nullptr);
    CHECK(g_live == 0);
    CHECK(barrier_create(0, &h) == DNS_OK && h != nullptr && g_live == 1);
    delete h;
    CHECK(g_live == 0);
    CHECK(barrier_create(0, nullptr) == DNS_ERR_BAD_ARGUMENT);
}

int main() {
    test_barrier();
    test_ring();
    test_extrap_coeffs();
    test_batch_policy();
    for (const auto &dims : {std::pair<int, int>{7, 5}, {12, 9}, {3, 2}}) {
        HostCsr F, J;
        build_system(dims.first, dims.second, F, J);
        test_products_and_slices(F, J);
        test_polynomial_rows(F);
        test_rows_on_their_reach(F);
        test_pair_format(F, J);
        test_halo_lists(F, J);
        test_mg_levels(F, J);
        test_misc(F);
    }
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("host logic: all checks passed under the sanitizers\n");
    return 0;
}
