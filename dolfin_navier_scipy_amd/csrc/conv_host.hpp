// Host side of the linearised convection operator (convection.hpp,
// conv_capi.inc): the expansion of a base flow into the twelve slots of every
// cell, the layout and the index table of a base trajectory and what the
// adjoint mode asks of the Dirichlet values.  No HIP in here:
// tests/conv_lin_host_sanitize.cpp, tests/conv_traj_host_sanitize.cpp and
// tests/conv_interp_host_sanitize.cpp exercise it on the host alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
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

// ---- base trajectory (dns_conv_set_base_trajectory) -------------------------
// `nrows` rows of inner velocities, row r at `r * ldv` (ldv: nv rounded up to
// 64, the slot layout of the snapshot ensemble: a slot copies row for row), the
// base flow's Dirichlet values as one set or one per row, and an index table
// `brow` that names the row of every step of an armed chunk (zero-order hold:
// descending for a reversed run, repeated entries for a subsampled trajectory).
constexpr size_t base_traj_ldv(int nv) {
    return ((size_t)nv + 63) & ~(size_t)63;
}
constexpr size_t base_traj_offset(int row, size_t ldv) {
    return (size_t)row * ldv;
}
// entries between two sets of Dirichlet values: 0 for one set (every row
// reads set 0), max(1, ndbc) for a set per row
constexpr int base_traj_dbc_stride(int dbc_nrows, int ndbc) {
    return dbc_nrows > 1 ? (ndbc > 1 ? ndbc : 1) : 0;
}

inline int check_base_trajectory(int nrows, int nv, const double *v_rows,
                                 long ld_host, int dbc_nrows, int ndbc,
                                 const double *dbc_vals) {
    if (nrows < 1)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "linearised convection: base trajectory of %d rows", nrows);
    if (nv < 0 || ndbc < 0 || (nv > 0 && !v_rows) || (ndbc > 0 && !dbc_vals))
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "linearised convection: base trajectory needs the inner "
                    "values (%d per row) and the Dirichlet values (%d)", nv,
                    ndbc);
    if (ld_host < (long)nv)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "linearised convection: base trajectory rows %ld apart, "
                    "%d inner values each", ld_host, nv);
    if (dbc_nrows != 1 && dbc_nrows != nrows)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "linearised convection: base trajectory of %d rows with "
                    "%d sets of Dirichlet values (one set, or one per row)",
                    nrows, dbc_nrows);
    return DNS_OK;
}

// the rows as the device holds them: nrows x ldv, zeros behind nv
inline int pack_base_trajectory(int nrows, int nv, const double *v_rows,
                                long ld_host, std::vector<double> &out) {
    DNS_TRY(check_base_trajectory(nrows, nv, v_rows, ld_host, 1, 0, nullptr));
    const size_t ldv = base_traj_ldv(nv);
    out.assign((size_t)nrows * std::max<size_t>(ldv, 1), 0.0);
    for (int r = 0; r < nrows; ++r)
        for (int i = 0; i < nv; ++i)
            out[base_traj_offset(r, ldv) + (size_t)i] =
                v_rows[(size_t)r * (size_t)ld_host + (size_t)i];
    return DNS_OK;
}

// the per-step index table: every entry a row of the trajectory, refused by
// name before anything is uploaded
inline int check_base_rows(int n, const int32_t *rows, int nrows) {
    if (nrows < 1)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "linearised convection: base rows without a base "
                    "trajectory (dns_conv_set_base_trajectory)");
    if (n < 1 || !rows)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "linearised convection: base rows: a table of %d entries",
                    n);
    for (int s = 0; s < n; ++s)
        if (rows[s] < 0 || rows[s] >= nrows)
            return fail(DNS_ERR_BAD_ARGUMENT,
                        "linearised convection: base rows: entry %d is %d, "
                        "outside 0..%d (the rows of the base trajectory)", s,
                        (int)rows[s], nrows - 1);
    return DNS_OK;
}

inline int check_base_row(int row, int nrows) {
    if (nrows < 1)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "linearised convection: base row without a base "
                    "trajectory (dns_conv_set_base_trajectory)");
    if (row < 0 || row >= nrows)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "linearised convection: base row %d outside 0..%d (the "
                    "rows of the base trajectory)", row, nrows - 1);
    return DNS_OK;
}

// ---- linear interpolation between row r and row r + 1 -----------------------
// One weight beside every entry of the index table (or beside the named row):
// the element kernels evaluate about V_r + th (V_{r+1} - V_r).  A weight is
// finite and lies in [0, 1) -- th = 1 is row r + 1 with weight 0 --, and a
// non-zero weight needs the row behind its own.
inline int check_base_weight(int entry, int row, double weight, int nrows) {
    // (entry < 0: the single host-named row)
    char where[48];
    if (entry >= 0) snprintf(where, sizeof where, "base rows: entry %d", entry);
    else snprintf(where, sizeof where, "base row %d", row);
    if (!(weight >= 0.0 && weight < 1.0))    // (a NaN fails both comparisons)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "linearised convection: %s has the interpolation weight "
                    "%.17g, outside [0, 1)", where, weight);
    if (weight != 0.0 && (long)row + 1 >= (long)nrows)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "linearised convection: %s: the interpolation weight "
                    "%.17g on row %d, the last of the %d rows of the base "
                    "trajectory (no row %ld to interpolate towards)", where,
                    weight, row, nrows, (long)row + 1);
    return DNS_OK;
}

inline int check_base_rows_lerp(int n, const int32_t *rows,
                                const double *weights, int nrows) {
    DNS_TRY(check_base_rows(n, rows, nrows));
    if (!weights)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "linearised convection: base rows: %d entries without "
                    "their interpolation weights", n);
    for (int s = 0; s < n; ++s)
        DNS_TRY(check_base_weight(s, rows[s], weights[s], nrows));
    return DNS_OK;
}

inline int check_base_row_lerp(int row, double weight, int nrows) {
    DNS_TRY(check_base_row(row, nrows));
    return check_base_weight(-1, row, weight, nrows);
}

// slots [first, first + count) of an ensemble of `nslots` slots
inline int check_base_slots(int first, int count, int nslots) {
    if (first < 0 || count < 1 || first > nslots - count)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "linearised convection: base trajectory from the "
                    "ensemble: slots %d .. %ld outside 0..%d", first,
                    (long)first + count - 1, nslots - 1);
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
