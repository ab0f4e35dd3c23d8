// What functionals and quadratics do on the host alone (csrc/attach_host.hpp:
// the stacked sparse rows, the sum of the workgroups' shares, the defaults of
// scale / c0 and the argument checks of the setters that need no device)
// WITHOUT HIP, under AddressSanitizer + UBSan:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover
//         -Iinclude tests/attach_host_sanitize.cpp -o attach_host_sanitize
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../dolfin_navier_scipy_amd/csrc/attach_host.hpp"

// (as the library defines it)
const char *dns_last_error(void) { return dns::g_last_error.c_str(); }

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

// a refusal with exactly this text
#define REFUSED(call, text)                                                  \
    do {                                                                     \
        dns::g_last_error.clear();                                           \
        const int s__ = (call);                                              \
        if (s__ != DNS_ERR_BAD_ARGUMENT ||                                   \
            strcmp(dns_last_error(), text) != 0) {                           \
            fprintf(stderr, "FAILED %s:%d: %s\n  status %d, message \"%s\"\n"\
                    "  expected \"%s\"\n", __FILE__, __LINE__, #call, s__,   \
                    dns_last_error(), text);                                 \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

namespace {

// a dense nrows x ncols matrix and its CSR (zeros are not stored)
struct Mat {
    int nrows, ncols;
    std::vector<double> dense;
    std::vector<int32_t> rp, ci;
    std::vector<double> va;
    dns_csr view() const {
        dns_csr v;
        v.nrows = nrows;
        v.ncols = ncols;
        v.nnz = (int64_t)va.size();
        v.rowptr = rp.data();
        v.colidx = ci.data();
        v.vals = va.data();
        return v;
    }
};

// entry (i, j) is non-zero where keep(i, j); distinct values
template <typename Keep>
Mat make(int nrows, int ncols, int seed, Keep keep) {
    Mat m;
    m.nrows = nrows;
    m.ncols = ncols;
    m.dense.assign((size_t)nrows * ncols, 0.0);
    m.rp.assign(1, 0);
    for (int i = 0; i < nrows; ++i) {
        for (int j = 0; j < ncols; ++j)
            if (keep(i, j)) {
                const double x = 1.0 + seed + 0.5 * i + 0.001 * j;
                m.dense[(size_t)i * ncols + j] = x;
                m.ci.push_back(j);
                m.va.push_back(x);
            }
        m.rp.push_back((int32_t)m.ci.size());
    }
    return m;
}

Mat shape(int nrows, int ncols) {
    return make(nrows, ncols, 0, [](int, int) { return false; });
}

// stack_rows against the dense statement: row nterms k + t of the result is
// row k of term t, an empty row where the term is null
void check_stack(const std::vector<const Mat *> &terms, int n) {
    const int nterms = (int)terms.size();
    std::vector<dns_csr> views((size_t)nterms);
    std::vector<const dns_csr *> ptr((size_t)nterms, nullptr);
    int width = 1;
    for (int t = 0; t < nterms; ++t)
        if (terms[t]) {
            views[t] = terms[t]->view();
            ptr[t] = &views[t];
            CHECK(terms[t]->nrows == n);
            width = std::max(width, terms[t]->ncols);
        }
    // (left over from another call: the vectors are written, not appended to)
    std::vector<int> rp(3, 7), ci(5, 9);
    std::vector<double> va(5, 9.0);
    dns::stack_rows(ptr.data(), nterms, n, rp, ci, va);
    CHECK(rp.size() == (size_t)nterms * n + 1 && rp[0] == 0);
    CHECK(ci.size() == va.size() && (size_t)rp.back() == ci.size());
    for (int k = 0; k < n; ++k)
        for (int t = 0; t < nterms; ++t) {
            const size_t r = (size_t)nterms * k + t;
            CHECK(rp[r + 1] >= rp[r]);
            std::vector<double> got((size_t)width, 0.0), want((size_t)width, 0.0);
            for (int z = rp[r]; z < rp[r + 1]; ++z) {
                CHECK(ci[z] >= 0 && ci[z] < width);
                CHECK(z == rp[r] || ci[z] > ci[z - 1]);  // the term's order
                got[(size_t)ci[z]] = va[z];
            }
            if (terms[t])
                for (int j = 0; j < terms[t]->ncols; ++j)
                    want[j] = terms[t]->dense[(size_t)k * terms[t]->ncols + j];
            CHECK(got == want);
        }
}

void test_stack_rows() {
    auto some = [](int i, int j) { return (i + 2 * j) % 3 == 0; };
    // (n, nterms) = (1, 3): the functionals' ca, cm, cp
    const Mat a1 = make(1, 7, 1, some), m1 = make(1, 7, 2, some),
              p1 = make(1, 3, 3, some);
    check_stack({&a1, &m1, &p1}, 1);
    check_stack({&a1, nullptr, &p1}, 1);
    // (16, 5): the limit, with the boundary terms
    const Mat a = make(16, 11, 1, some), m = make(16, 11, 2, some),
              p = make(16, 5, 3, some), ab = make(16, 4, 4, some),
              mb = make(16, 4, 5, some);
    check_stack({&a, &m, &p, &ab, &mb}, 16);
    check_stack({nullptr, &m, nullptr, &ab, nullptr}, 16);
    // (8, 2): the quadratics' qa, qw
    const Mat qa = make(8, 9, 1, some), qw = make(8, 9, 2, some);
    check_stack({&qa, &qw}, 8);
    check_stack({nullptr, &qw}, 8);
    // every term null
    check_stack({nullptr, nullptr, nullptr}, 1);
    check_stack({nullptr, nullptr, nullptr, nullptr, nullptr}, 16);
    check_stack({nullptr, nullptr}, 8);
    // a term with empty rows (every other one, the first among them), a term
    // whose last row is empty, a term without entries
    const Mat holes = make(8, 9, 6, [](int i, int) { return i % 2 == 1; });
    const Mat tail = make(8, 9, 7, [](int i, int j) { return i < 7 && j % 2; });
    const Mat none = shape(8, 9);
    check_stack({&holes, &tail}, 8);
    check_stack({&tail, &holes}, 8);
    check_stack({&none, &tail}, 8);
    check_stack({&holes, &none, &tail}, 8);
}

void test_sum_shares() {
    // shares whose sum depends on the order: 1e16, 1, -1e16 in turn (shifted
    // by row and column), left to right
    const double vals[3] = {1e16, 1.0, -1e16};
    for (int G : {1, 2, 256})
        for (int n : {1, 16})
            for (int count : {0, 1, 3}) {
                std::vector<double> part((size_t)count * G * n);
                for (int r = 0; r < count; ++r)
                    for (int g = 0; g < G; ++g)
                        for (int k = 0; k < n; ++k)
                            part[((size_t)r * G + g) * n + k] =
                                vals[(g + k + r) % 3] * (1 + k);
                std::vector<double> out((size_t)count * n + 1, -7.0);
                dns::sum_shares(part.data(), count, G, n, out.data());
                for (int r = 0; r < count; ++r)
                    for (int k = 0; k < n; ++k) {
                        volatile double y = 0.0;
                        for (int g = 0; g < G; ++g)
                            y = y + vals[(g + k + r) % 3] * (1 + k);
                        CHECK(out[(size_t)r * n + k] == y);
                    }
                CHECK(out.back() == -7.0);
            }
    // the order shows: 1e16 + 1 - 1e16 is 0 from the left, 1 is lost
    const double three[3] = {1e16, 1.0, -1e16};
    double y = -1.0;
    dns::sum_shares(three, 1, 3, 1, &y);
    CHECK(y == 0.0);
    const double other[3] = {1e16, -1e16, 1.0};
    dns::sum_shares(other, 1, 3, 1, &y);
    CHECK(y == 1.0);
}

void test_scale_c0() {
    std::vector<double> sc(9, 5.0), cc(1, 5.0);
    dns::scale_c0(nullptr, nullptr, 3, sc, cc);
    CHECK(sc == std::vector<double>(3, 1.0) && cc == std::vector<double>(3, 0.0));
    const double s[2] = {2.0, 3.0}, c[2] = {-1.0, 4.0};
    dns::scale_c0(s, nullptr, 2, sc, cc);
    CHECK(sc == std::vector<double>(s, s + 2) && cc == std::vector<double>(2, 0.0));
    dns::scale_c0(nullptr, c, 2, sc, cc);
    CHECK(sc == std::vector<double>(2, 1.0) && cc == std::vector<double>(c, c + 2));
}

// ---- the setters' checks: one accepted input per form, then inputs that
// violate exactly one condition each

struct FnIn {
    int nF = 2, nF_max = 16, nrows = 4;
    double dt = 0.5;
    bool moving = false, live = false;
    int ndbc = 0;
    const double *table = nullptr;
    int nv = 10, np = 4;
    const dns_csr *terms[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const int32_t *cell_ptr = nullptr, *cell_idx = nullptr;
    const double *cell_w = nullptr;
    int check() const {
        return dns::check_functionals_args(nF, nF_max, nrows, dt, moving, live,
                                           ndbc, table, terms, nv, np,
                                           cell_ptr, cell_idx, cell_w);
    }
};

void test_functionals_checks() {
    const Mat a = shape(2, 10), p = shape(2, 4), b = shape(2, 3);
    const dns_csr va = a.view(), vp = p.view(), vb = b.view();
    const double tab[15] = {};
    const int32_t cptr[3] = {0, 1, 3}, cidx[3] = {0, 1, 2};
    const double cw[36] = {};
    FnIn ok;                            // constant values, with cells
    ok.terms[0] = &va;
    ok.terms[1] = &va;
    ok.terms[2] = &vp;
    ok.cell_ptr = cptr;
    ok.cell_idx = cidx;
    ok.cell_w = cw;
    CHECK(ok.check() == DNS_OK);
    FnIn own = ok;                      // a table of their own
    own.moving = true;
    own.ndbc = 3;
    own.table = tab;
    own.terms[3] = &vb;
    own.terms[4] = &vb;
    CHECK(own.check() == DNS_OK);
    FnIn live = own;                    // the operator's table
    live.live = true;
    live.table = nullptr;
    CHECK(live.check() == DNS_OK);
    FnIn bare;                          // no term, no cells
    CHECK(bare.check() == DNS_OK);
    const int32_t nocells[3] = {0, 0, 0};
    FnIn empty = ok;                    // cell_ptr without a cell
    empty.cell_ptr = nocells;
    empty.cell_idx = nullptr;
    empty.cell_w = nullptr;
    CHECK(empty.check() == DNS_OK);

    FnIn x = ok;
    x.nF = 0;
    REFUSED(x.check(), "functionals: nF = 0 outside 1..16");
    x = ok;
    x.nF = 17;
    REFUSED(x.check(), "functionals: nF = 17 outside 1..16");
    x = ok;
    x.nrows = 0;
    REFUSED(x.check(), "functionals: nrows = 0 < 1");
    x = ok;
    x.dt = 0.0;
    REFUSED(x.check(), "functionals: dt must be positive");
    x = ok;
    x.dt = -1.0;
    REFUSED(x.check(), "functionals: dt must be positive");
    x = ok;
    x.dt = std::nan("");
    REFUSED(x.check(), "functionals: dt must be positive");
    x = own;
    x.ndbc = 0;
    x.terms[3] = x.terms[4] = nullptr;
    REFUSED(x.check(), "functionals: ndbc = 0 < 1 (constant Dirichlet values: "
                       "dns_imex_set_functionals)");
    x = own;
    x.table = nullptr;
    REFUSED(x.check(), "functionals: no table of the Dirichlet values");
    x = ok;
    x.terms[0] = &vp;                   // ca as wide as NP
    REFUSED(x.check(), "functionals: ca must be nF x 10, it is 2 x 4");
    x = ok;
    x.terms[1] = &vb;
    REFUSED(x.check(), "functionals: cm must be nF x 10, it is 2 x 3");
    x = ok;
    x.terms[2] = &va;
    REFUSED(x.check(), "functionals: cp must be nF x 4, it is 2 x 10");
    x = own;
    x.terms[3] = &vp;
    REFUSED(x.check(), "functionals: cab must be nF x 3, it is 2 x 4");
    x = own;
    x.terms[4] = &va;
    REFUSED(x.check(), "functionals: cmb must be nF x 3, it is 2 x 10");
    const Mat rows3 = shape(3, 10);
    const dns_csr v3 = rows3.view();
    x = ok;
    x.terms[0] = &v3;                   // another number of rows
    REFUSED(x.check(), "functionals: ca must be nF x 10, it is 3 x 10");
    const int32_t from1[3] = {1, 1, 3}, back[3] = {0, 2, 1};
    x = ok;
    x.cell_ptr = from1;
    REFUSED(x.check(), "functionals: cell_ptr[0] must be 0");
    x = ok;
    x.cell_ptr = back;
    REFUSED(x.check(), "functionals: cell_ptr not monotone");
    x = ok;
    x.cell_idx = nullptr;
    REFUSED(x.check(), "functionals: cells without cell_idx / cell_w");
    x = ok;
    x.cell_w = nullptr;
    REFUSED(x.check(), "functionals: cells without cell_idx / cell_w");
}

struct QdIn {
    int nM = 2, nM_max = 4, nQ = 3, nQ_max = 8, nrows = 4, max_grid = 0;
    double dt = 0.5;
    bool moving = false, live = false;
    int ndbc = 0;
    const double *table = nullptr;
    const dns_csr *mats = nullptr;
    const int32_t *mat = nullptr, *lop = nullptr, *rop = nullptr;
    const dns_csr *lin[2] = {nullptr, nullptr};
    int nv = 10;
    int check() const {
        return dns::check_quadratics_args(nM, nM_max, nQ, nQ_max, nrows,
                                          max_grid, dt, moving, live, ndbc,
                                          table, mats, mat, lop, rop, lin, nv);
    }
};

void test_quadratics_checks() {
    const Mat sq = shape(10, 10), wide = shape(13, 13), l = shape(3, 10),
              lw = shape(3, 13), odd = shape(10, 9);
    const dns_csr two[2] = {sq.view(), sq.view()},
                  twow[2] = {wide.view(), wide.view()},
                  bad[2] = {sq.view(), odd.view()};
    const dns_csr vl = l.view(), vlw = lw.view();
    const int32_t mat[3] = {0, 1, 1}, lop[3] = {0, 1, 0}, rop[3] = {0, 1, 1};
    const double tab[15] = {};
    QdIn ok;                            // constant values
    ok.mats = two;
    ok.mat = mat;
    ok.lop = lop;
    ok.rop = rop;
    ok.lin[0] = &vl;
    CHECK(ok.check() == DNS_OK);
    QdIn own = ok;                      // a table of their own, NV + ndbc wide
    own.moving = true;
    own.ndbc = 3;
    own.table = tab;
    own.nv = 13;
    own.mats = twow;
    own.lin[0] = nullptr;
    own.lin[1] = &vlw;
    CHECK(own.check() == DNS_OK);
    QdIn live = own;                    // the operator's table
    live.live = true;
    live.table = nullptr;
    CHECK(live.check() == DNS_OK);

    QdIn x = ok;
    x.nM = 0;
    REFUSED(x.check(), "quadratics: nM = 0 outside 1..4");
    x = ok;
    x.nM = 5;
    REFUSED(x.check(), "quadratics: nM = 5 outside 1..4");
    x = ok;
    x.nQ = 0;
    REFUSED(x.check(), "quadratics: nQ = 0 outside 1..8");
    x = ok;
    x.nQ = 9;
    REFUSED(x.check(), "quadratics: nQ = 9 outside 1..8");
    x = ok;
    x.nrows = 0;
    REFUSED(x.check(), "quadratics: nrows = 0 < 1");
    x = ok;
    x.max_grid = -1;
    REFUSED(x.check(), "quadratics: max_grid = -1 < 0");
    x = ok;
    x.dt = 0.0;
    REFUSED(x.check(), "quadratics: dt must be positive");
    x = own;
    x.ndbc = 0;
    x.nv = 10;
    x.mats = two;
    x.lin[1] = nullptr;
    REFUSED(x.check(), "quadratics: ndbc = 0 < 1 (constant Dirichlet values: "
                       "dns_imex_set_quadratics)");
    x = own;
    x.table = nullptr;
    REFUSED(x.check(), "quadratics: no table of the Dirichlet values");
    x = ok;
    x.mats = bad;
    REFUSED(x.check(),
            "quadratics: matrix 1 must be NV x NV (10), it is 10 x 9");
    x = own;
    x.mats = two;
    REFUSED(x.check(), "quadratics: matrix 0 must be (NV + ndbc) x (NV + ndbc) "
                       "(13), it is 10 x 10");
    x = ok;
    x.lin[0] = &vlw;
    REFUSED(x.check(),
            "quadratics: qa must be nQ x NV (3 x 10), it is 3 x 13");
    x = own;
    x.lin[1] = &vl;
    REFUSED(x.check(), "quadratics: qw must be nQ x (NV + ndbc) (3 x 13), it "
                       "is 3 x 10");
    const int32_t mat_hi[3] = {0, 2, 1}, mat_lo[3] = {0, 1, -1},
                  op2[3] = {0, 2, 0}, opm[3] = {-1, 1, 1};
    x = ok;
    x.mat = mat_hi;
    REFUSED(x.check(), "quadratics: mat[1] = 2 outside 0..1");
    x = ok;
    x.mat = mat_lo;
    REFUSED(x.check(), "quadratics: mat[2] = -1 outside 0..1");
    x = ok;
    x.lop = op2;
    REFUSED(x.check(), "quadratics: operands (2, 1) of form 1 are not 0 (v) or "
                       "1 (v - v_prev)");
    x = ok;
    x.rop = opm;
    REFUSED(x.check(), "quadratics: operands (0, -1) of form 0 are not 0 (v) "
                       "or 1 (v - v_prev)");
    // the log: rows x G x nQ below 2^31
    CHECK(dns::check_quadratics_log(1, 1, 1) == DNS_OK);
    CHECK(dns::check_quadratics_log(1048575, 256, 8) == DNS_OK);
    REFUSED(dns::check_quadratics_log(1048576, 256, 8),
            "quadratics: a log of 2147483648 entries (1048576 rows x 256 "
            "workgroups x 8 forms), the limit is 2^31 - 1: cap the grid "
            "(max_grid) or take shorter slices");
}

}  // namespace

int main() {
    test_stack_rows();
    test_sum_shares();
    test_scale_c0();
    test_functionals_checks();
    test_quadratics_checks();
    printf("all checks passed\n");
    return 0;
}
