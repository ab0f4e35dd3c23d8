// Tile plan, index maps and shape checks of the convection tensor of a
// Galerkin projection (galerkin.hpp).  No HIP in here:
// tests/rom_host_sanitize.cpp exercises it on the host alone.
//
//   T[i, (j, k)] = sum_cells P_cell C_cell^T,  P nt x 16, C nb^2 x 16 per cell
// (fourteen (point, component) pairs and two zeros).  Rows i in tiles of 16
// (at most 3), columns col = j nb + k in tiles of 16 (at most 69).  A
// workgroup is (chunk of kRomCellChunk cells) x (group of kRomGroupTiles
// column tiles); wave w of it carries the column tiles
//   group kRomGroupTiles + t kRomWaves + w,  t < kRomTilesPerWave,
// against every row tile.  The partial tiles of a chunk lie side by side,
//   part[((chunk nrt + rt) nct + ct) 256 + e],
// entry e of a tile as the wave holds it (ens_tile_row / ens_tile_col).
#pragma once
#include <cstddef>
#include <cstdint>

#include "ensemble_host.hpp"
#include "status.hpp"

namespace dns {

constexpr int kRomMaxBasis = 33;    // 32 modes and the mean flow
constexpr int kRomCellChunk = 512;  // cells of one partial tile: a constant,
                                    // so the bits do not depend on the device
constexpr int kRomTile = 16;
constexpr int kRomWaves = 4;        // waves of a workgroup
constexpr int kRomTilesPerWave = 3; // column tiles a wave carries
constexpr int kRomGroupTiles = kRomWaves * kRomTilesPerWave;
constexpr int kRomStage = 2;        // cells staged in LDS at a time
// LDS rows per (staged cell, basis row): u at the 8 point slots (2 entries
// each), grad u (4 each, two doubles of padding: rows 4 banks apart), the
// weighted test function (2 each, padded likewise)
constexpr int kRomLdU = 16, kRomLdG = 34, kRomLdP = 18;

constexpr int rom_row_tiles(int nt) { return (nt + kRomTile - 1) / kRomTile; }
constexpr int rom_cols(int nb) { return nb * nb; }
constexpr int rom_col_tiles(int nb) {
    return (rom_cols(nb) + kRomTile - 1) / kRomTile;
}
constexpr int rom_col_groups(int nb) {
    return (rom_col_tiles(nb) + kRomGroupTiles - 1) / kRomGroupTiles;
}
constexpr int rom_chunks(int ncells) {
    return (ncells + kRomCellChunk - 1) / kRomCellChunk;
}
// the column tile of pass t of wave w of group g (may lie behind the last)
constexpr int rom_wave_tile(int g, int w, int t) {
    return g * kRomGroupTiles + t * kRomWaves + w;
}
// column col = j nb + k: j the convecting, k the convected field
constexpr int rom_col_j(int col, int nb) { return col / nb; }
constexpr int rom_col_k(int col, int nb) { return col % nb; }
// K index kk < 16 of a cell: point kk >> 1 (7: the zero padding), component
// kk & 1
constexpr int rom_k_point(int kk) { return kk >> 1; }
constexpr int rom_k_comp(int kk) { return kk & 1; }

constexpr size_t rom_part_index(int chunk, int rt, int ct, int nrt, int nct) {
    return (((size_t)chunk * nrt + rt) * nct + ct) * (kRomTile * kRomTile);
}
// doubles of all partial tiles
constexpr size_t rom_partials(int ncells, int nb, int nt) {
    return (size_t)rom_chunks(ncells) * rom_row_tiles(nt) * rom_col_tiles(nb) *
           (kRomTile * kRomTile);
}
constexpr size_t rom_lds_doubles() {
    return (size_t)kRomStage * kRomMaxBasis * (kRomLdU + kRomLdG + kRomLdP);
}

// the cells that hold an inner dof, given the map [12][ncells] in the
// operator's internal order (cells without one come last)
inline int rom_live_cells(const int *cmap, int ncells) {
    int n = ncells;
    for (; n > 0; --n) {
        bool inner = false;
        for (int k = 0; k < 12; ++k)
            inner = inner || cmap[(size_t)k * ncells + (n - 1)] >= 0;
        if (inner) break;
    }
    return n;
}

inline int check_rom_shape(int nb, int nt, int nv, long long ld, int ncells) {
    if (nb < 1 || nb > kRomMaxBasis)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "galerkin: nb = %d basis rows outside 1..%d (32 modes and "
                    "a mean flow)", nb, kRomMaxBasis);
    if (nt < 1 || nt > nb)
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "galerkin: nt = %d test rows outside 1..nb = %d", nt, nb);
    if (ld < (long long)nv || (ld & 1))
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "galerkin: ld = %lld must be even and >= the %d inner "
                    "dofs", ld, nv);
    if (ncells < 0 || rom_partials(ncells, nb, nt) >= ((size_t)1 << 31))
        return fail(DNS_ERR_BAD_ARGUMENT,
                    "galerkin: %zu partial entries (%d cells, nb = %d), the "
                    "limit is 2^31 - 1", rom_partials(ncells, nb, nt), ncells,
                    nb);
    return DNS_OK;
}

}  // namespace dns
