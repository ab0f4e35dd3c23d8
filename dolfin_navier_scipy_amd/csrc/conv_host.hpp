// Host side of the linearised convection operator (convection.hpp,
// conv_capi.inc): the expansion of a base flow into the twelve slots of every
// cell and what the adjoint mode asks of the Dirichlet values.  No HIP in
// here: tests/conv_lin_host_sanitize.cpp exercises it on the host alone.
#pragma once
#include <cstddef>
#include <vector>

#include "status.hpp"

namespace dns {

constexpr int kConvNonlinear = 0, kConvForward = 1, kConvAdjoint = 2;

// vbase[k * ncells + c] = V at slot k of cell c: inner dof m >= 0 of the map
// [12][ncells] from `v_inner`, Dirichlet value -(m + 1) from `dbcvals`
inline int expand_base_flow(const int *cmap, int ncells, int nv, int ndbc,
                            const double *v_inner, const double *dbcvals,
                            std::vector<double> &vbase) {
    if (!cmap || ncells < 1 || nv < 0 || ndbc < 0 || (nv > 0 && !v_inner) ||
        (ndbc > 0 && !dbcvals))
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "linearised convection: base flow needs the inner values "
                    "(%d) and the Dirichlet values (%d)", nv, ndbc);
    vbase.assign((size_t)12 * ncells, 0.0);
    for (int k = 0; k < 12; ++k)
        for (int c = 0; c < ncells; ++c) {
            const size_t e = (size_t)k * ncells + c;
            const int m = cmap[e];
            if (m >= 0) {
                if (m >= nv)
                    return fail(DNS_ERR_BAD_ARGUMENT,
                                "linearised convection: map entry %d of cell "
                                "%d outside the %d inner dofs", m, c, nv);
                vbase[e] = v_inner[m];
            } else {
                // (long: -(INT_MIN) does not exist)
                const long d = -(long)m - 1;
                if (d >= ndbc)
                    return fail(DNS_ERR_BAD_ARGUMENT,
                                "linearised convection: map entry %d of cell "
                                "%d outside the %d Dirichlet values", m, c,
                                ndbc);
                vbase[e] = dbcvals[d];
            }
        }
    return DNS_OK;
}

// Adjoint mode: the cell transposes gather to (L_II)^T w_I only if the
// perturbation vanishes on the Dirichlet dofs -- zero values, no table.
inline int check_adjoint_dbc(const double *dbc_host, int ndbc, int dbc_rows) {
    if (dbc_rows > 0)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "linearised convection, adjoint mode: a per-step "
                    "Dirichlet table is set (dns_conv_set_dbc_table); the "
                    "adjoint takes zero Dirichlet values and no table");
    for (int k = 0; k < ndbc; ++k)
        if (dbc_host[k] != 0.0)
            return fail(DNS_ERR_BAD_ARGUMENT,
                        "linearised convection, adjoint mode: Dirichlet value "
                        "%d is %g; the adjoint takes zero Dirichlet values "
                        "(dns_conv_set_dbcvals)", k, dbc_host[k]);
    return DNS_OK;
}

}  // namespace dns
