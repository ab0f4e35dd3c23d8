// Layout arithmetic and table checks of the snapshot ensemble (ensemble.hpp).
// No HIP in here: tests/pod_host_sanitize.cpp exercises it on the host alone.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "status.hpp"

namespace dns {

constexpr int kEnsTile = 16;        // snapshots per tile edge / per block of Y
constexpr int kEnsChunk = 1024;     // entries k of one partial tile: a constant,
                                    // so the bits do not depend on the device
constexpr int kEnsAcc = 16;         // rows q of `out` a combine pass carries

// a slot: NV rounded up to 64 doubles (every slot starts on a 512-byte line)
constexpr size_t ens_ldv(int nv) { return ((size_t)nv + 63) & ~(size_t)63; }
constexpr int ens_blocks(int m) { return (m + kEnsTile - 1) / kEnsTile; }
constexpr int ens_chunks(int nv) { return (nv + kEnsChunk - 1) / kEnsChunk; }
constexpr int ens_passes(int r) { return (r + kEnsAcc - 1) / kEnsAcc; }
// the partial tiles of one block column of G: a tile per block row, chunk
// after chunk, 256 doubles each
constexpr size_t ens_partials(int m, int nv) {
    return (size_t)ens_blocks(m) * ens_chunks(nv) * kEnsTile * kEnsTile;
}
// entry e of a tile as the wave holds it: register e >> 6 of lane e & 63
// (v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 * register)
constexpr int ens_tile_row(int e) { return ((e & 63) >> 4) + 4 * (e >> 6); }
constexpr int ens_tile_col(int e) { return e & 15; }

// coef (r x m, row-major) as k_ens_combine reads it: for every pass of 16
// rows q and every snapshot s the 16 coefficients side by side, zeros behind r
inline std::vector<double> ens_pack_coef(const double *coef, int r, int m) {
    std::vector<double> c((size_t)ens_passes(r) * m * kEnsAcc, 0.0);
    for (int q = 0; q < r; ++q)
        for (int s = 0; s < m; ++s)
            c[((size_t)(q / kEnsAcc) * m + s) * kEnsAcc + q % kEnsAcc] =
                coef[(size_t)q * m + s];
    return c;
}

inline int check_slot_table(int nrows, const int32_t *slot, int nslots) {
    if (!slot) return fail(DNS_ERR_BAD_ARGUMENT, "null argument");
    if (nrows < 1)
        return fail(DNS_ERR_BAD_ARGUMENT, "ensemble: nrows = %d < 1", nrows);
    if (nslots < 1)
        return fail(DNS_ERR_BAD_ARGUMENT, "ensemble: nslots = %d < 1", nslots);
    for (int r = 0; r < nrows; ++r)
        if (slot[r] < -1 || slot[r] >= nslots)
            return fail(DNS_ERR_BAD_ARGUMENT,
                        "ensemble: slot[%d] = %d outside -1..%d", r,
                        (int)slot[r], nslots - 1);
    return DNS_OK;
}

// what the kernels index in int: the entries of the ensemble and of the
// partial tiles stay below 2^31 pairs / doubles per row block
inline int check_ensemble_shape(int m, int nv, size_t ld) {
    if (m < 1 || nv < 1)
        return fail(DNS_ERR_BAD_ARGUMENT, "ensemble: m = %d, nv = %d < 1", m, nv);
    if (ld < (size_t)nv || (ld & 1))
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "ensemble: ld = %zu must be even and >= nv = %d (16-byte "
                    "rows)", ld, nv);
    if (ens_partials(m, nv) >= ((size_t)1 << 31))
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "ensemble: %zu partial entries (m = %d, nv = %d), the "
                    "limit is 2^31 - 1", ens_partials(m, nv), m, nv);
    return DNS_OK;
}

}  // namespace dns
