// What the functionals and the quadratics of the resident IMEX loop
// (imex_attach_capi.inc) do on the host alone: the argument checks of their
// setters that need neither the stepper's device state nor the convection
// operator, the stacking of their sparse rows into one CSR and the sum of the
// workgroups' shares of a log.  No HIP in here (limits that live beside the
// kernels come in as arguments): tests/attach_host_sanitize.cpp runs it under
// the sanitizers on the host alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "status.hpp"

namespace dns {

static const char *const kFnTermNames[5] = {"ca", "cm", "cp", "cab", "cmb"};
static const char *const kQdLinNames[2] = {"qa", "qw"};

// The `nterms * n` sparse rows (k, term) in one CSR; a null term is an empty
// row.  (Functionals: 3 or 5 terms of nF rows; quadratics: qa / qw, nQ rows.)
inline void stack_rows(const dns_csr *const *terms, int nterms, int n,
                       std::vector<int> &rp, std::vector<int> &ci,
                       std::vector<double> &va) {
    rp.assign((size_t)nterms * n + 1, 0);
    ci.clear();
    va.clear();
    for (int k = 0; k < n; ++k)
        for (int t = 0; t < nterms; ++t) {
            if (terms[t])
                for (int64_t z = terms[t]->rowptr[k];
                     z < terms[t]->rowptr[k + 1]; ++z) {
                    ci.push_back(terms[t]->colidx[z]);
                    va.push_back(terms[t]->vals[z]);
                }
            rp[(size_t)nterms * k + t + 1] = (int)ci.size();
        }
}

// `count` rows of a log of G x n shares each: the workgroups' shares, in index
// order
inline void sum_shares(const double *part, int count, int G, int n,
                       double *out) {
    const size_t per = (size_t)G * n;
    for (int r = 0; r < count; ++r)
        for (int k = 0; k < n; ++k) {
            double y = 0.0;
            for (int g = 0; g < G; ++g)
                y += part[(size_t)r * per + (size_t)g * n + k];
            out[(size_t)r * n + k] = y;
        }
}

// defaults of the affine map of a row: scale 1, c0 0
inline void scale_c0(const double *scale, const double *c0, int n,
                     std::vector<double> &sc, std::vector<double> &cc) {
    sc.assign((size_t)n, 1.0);
    cc.assign((size_t)n, 0.0);
    if (scale) sc.assign(scale, scale + n);
    if (c0) cc.assign(c0, c0 + n);
}

// What both setters ask of the rows, the step and the source of the Dirichlet
// values (`moving`: `ndbc` of them per row -- `live`: read from the convection
// operator's table, else from `dbc_table`); `const_setter`: the export for
// constant values.
inline int check_log_args(const char *noun, const char *const_setter,
                          int nrows, double dt, bool moving, bool live,
                          int ndbc, const double *dbc_table) {
    if (nrows < 1)
        return fail(DNS_ERR_BAD_ARGUMENT, "%s: nrows = %d < 1", noun, nrows);
    if (!(dt > 0.0))
        return fail(DNS_ERR_BAD_ARGUMENT, "%s: dt must be positive", noun);
    if (moving && ndbc < 1)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "%s: ndbc = %d < 1 (constant Dirichlet values: %s)", noun,
                    ndbc, const_setter);
    if (moving && !live && !dbc_table)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "%s: no table of the Dirichlet values", noun);
    return DNS_OK;
}

// dns_imex_set_functionals / _bc / _live: `terms` ca, cm, cp (moving: and cab,
// cmb), null where absent; nv, np: the stepper's
inline int check_functionals_args(int nF, int nF_max, int nrows, double dt,
                                  bool moving, bool live, int ndbc,
                                  const double *dbc_table,
                                  const dns_csr *const *terms, int nv, int np,
                                  const int32_t *cell_ptr,
                                  const int32_t *cell_idx,
                                  const double *cell_w) {
    if (nF < 1 || nF > nF_max)
        return fail(DNS_ERR_BAD_ARGUMENT, "functionals: nF = %d outside 1..%d",
                    nF, nF_max);
    DNS_TRY(check_log_args("functionals", "dns_imex_set_functionals", nrows,
                           dt, moving, live, ndbc, dbc_table));
    for (int t = 0; t < (moving ? 5 : 3); ++t) {
        if (!terms[t]) continue;
        const int want = t == 2 ? np : (t > 2 ? ndbc : nv);
        if (terms[t]->nrows != nF || terms[t]->ncols != want)
            return fail(DNS_ERR_BAD_ARGUMENT,
                        "functionals: %s must be nF x %d, it is %d x %d",
                        kFnTermNames[t], want, (int)terms[t]->nrows,
                        (int)terms[t]->ncols);
    }
    if (!cell_ptr) return DNS_OK;
    if (cell_ptr[0] != 0)
        return fail(DNS_ERR_BAD_ARGUMENT, "functionals: cell_ptr[0] must be 0");
    for (int k = 0; k < nF; ++k)
        if (cell_ptr[k + 1] < cell_ptr[k])
            return fail(DNS_ERR_BAD_ARGUMENT,
                        "functionals: cell_ptr not monotone");
    if (cell_ptr[nF] > 0 && (!cell_idx || !cell_w))
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "functionals: cells without cell_idx / cell_w");
    return DNS_OK;
}

// dns_imex_set_quadratics / _bc / _live: `mats` nM matrices, `lin` qa / qw
// (null where absent), all `nv` wide -- the stepper's NV, with moving values
// NV + ndbc
inline int check_quadratics_args(int nM, int nM_max, int nQ, int nQ_max,
                                 int nrows, int max_grid, double dt,
                                 bool moving, bool live, int ndbc,
                                 const double *dbc_table, const dns_csr *mats,
                                 const int32_t *mat, const int32_t *lop,
                                 const int32_t *rop,
                                 const dns_csr *const *lin, int nv) {
    if (nM < 1 || nM > nM_max)
        return fail(DNS_ERR_BAD_ARGUMENT, "quadratics: nM = %d outside 1..%d",
                    nM, nM_max);
    if (nQ < 1 || nQ > nQ_max)
        return fail(DNS_ERR_BAD_ARGUMENT, "quadratics: nQ = %d outside 1..%d",
                    nQ, nQ_max);
    if (max_grid < 0)
        return fail(DNS_ERR_BAD_ARGUMENT, "quadratics: max_grid = %d < 0",
                    max_grid);
    DNS_TRY(check_log_args("quadratics", "dns_imex_set_quadratics", nrows, dt,
                           moving, live, ndbc, dbc_table));
    for (int m = 0; m < nM; ++m)
        if (mats[m].nrows != nv || mats[m].ncols != nv)
            return fail(DNS_ERR_BAD_ARGUMENT,
                        "quadratics: matrix %d must be %s (%d), it is %d x %d",
                        m, moving ? "(NV + ndbc) x (NV + ndbc)" : "NV x NV", nv,
                        (int)mats[m].nrows, (int)mats[m].ncols);
    for (int t = 0; t < 2; ++t)
        if (lin[t] && (lin[t]->nrows != nQ || lin[t]->ncols != nv))
            return fail(DNS_ERR_BAD_ARGUMENT,
                        "quadratics: %s must be nQ x %s (%d x %d), it is "
                        "%d x %d", kQdLinNames[t],
                        moving ? "(NV + ndbc)" : "NV", nQ, nv,
                        (int)lin[t]->nrows, (int)lin[t]->ncols);
    for (int k = 0; k < nQ; ++k) {
        if (mat[k] < 0 || mat[k] >= nM)
            return fail(DNS_ERR_BAD_ARGUMENT,
                        "quadratics: mat[%d] = %d outside 0..%d", k,
                        (int)mat[k], nM - 1);
        if (lop[k] < 0 || lop[k] > 1 || rop[k] < 0 || rop[k] > 1)
            return fail(DNS_ERR_BAD_ARGUMENT,
                        "quadratics: operands (%d, %d) of form %d are not 0 "
                        "(v) or 1 (v - v_prev)", (int)lop[k], (int)rop[k], k);
    }
    return DNS_OK;
}

// (the getter and the kernel count the entries of the log in int)
inline int check_quadratics_log(int nrows, int G, int nQ) {
    const size_t total = (size_t)nrows * G * nQ;
    if (total >= ((size_t)1 << 31))
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "quadratics: a log of %zu entries (%d rows x %d "
                    "workgroups x %d forms), the limit is 2^31 - 1: cap "
                    "the grid (max_grid) or take shorter slices", total,
                    nrows, G, nQ);
    return DNS_OK;
}

}  // namespace dns
