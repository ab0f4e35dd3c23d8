// The host-only parts of the Galerkin projection (csrc/galerkin_host.hpp: the
// tile plan, the column and K index maps, the partial-buffer sizes at the
// limits, the live-cell count and the shape checks) WITHOUT HIP, under
// AddressSanitizer + UBSan:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover
//         -Iinclude tests/rom_host_sanitize.cpp -o rom_host_sanitize
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../dolfin_navier_scipy_amd/csrc/galerkin_host.hpp"

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

int main() {
    using namespace dns;
    CHECK(kRomMaxBasis == 33 && kRomCellChunk == 512);
    CHECK(kRomGroupTiles == kRomWaves * kRomTilesPerWave);
    // tiles
    CHECK(rom_row_tiles(1) == 1 && rom_row_tiles(16) == 1 &&
          rom_row_tiles(17) == 2 && rom_row_tiles(33) == 3);
    CHECK(rom_col_tiles(1) == 1 && rom_col_tiles(4) == 1 &&
          rom_col_tiles(5) == 2 && rom_col_tiles(33) == 69);
    CHECK(rom_col_groups(1) == 1 && rom_col_groups(13) == 1 &&
          rom_col_groups(14) == 2 && rom_col_groups(33) == 6);
    CHECK(rom_chunks(0) == 0 && rom_chunks(1) == 1 &&
          rom_chunks(kRomCellChunk) == 1 && rom_chunks(kRomCellChunk + 1) == 2);
    // every column tile belongs to exactly one (group, wave, pass); the
    // kernel's three row-tile accumulators cover the limit
    CHECK(rom_row_tiles(kRomMaxBasis) <= 3);
    for (int nb = 1; nb <= kRomMaxBasis; ++nb) {
        const int nct = rom_col_tiles(nb);
        std::vector<int> owner((size_t)nct, 0);
        for (int g = 0; g < rom_col_groups(nb); ++g)
            for (int w = 0; w < kRomWaves; ++w)
                for (int t = 0; t < kRomTilesPerWave; ++t) {
                    const int ct = rom_wave_tile(g, w, t);
                    CHECK(ct >= 0);
                    if (ct < nct) owner[(size_t)ct]++;
                }
        for (int ct = 0; ct < nct; ++ct) CHECK(owner[(size_t)ct] == 1);
        // columns <-> (j, k), a bijection onto nb x nb
        std::set<int> seen;
        for (int col = 0; col < rom_cols(nb); ++col) {
            const int j = rom_col_j(col, nb), k = rom_col_k(col, nb);
            CHECK(j >= 0 && j < nb && k >= 0 && k < nb && j * nb + k == col);
            seen.insert(j * nb + k);
        }
        CHECK((int)seen.size() == nb * nb);
        CHECK(nct * kRomTile >= rom_cols(nb) &&
              (nct - 1) * kRomTile < rom_cols(nb));
    }
    // K index: fourteen (point, component) pairs and the two zeros of point 7
    for (int kk = 0; kk < 16; ++kk) {
        CHECK(rom_k_point(kk) * 2 + rom_k_comp(kk) == kk);
        CHECK(rom_k_point(kk) <= 7 && (rom_k_point(kk) == 7) == (kk >= 14));
    }
    // LDS: the staged rows fit their strides and 64 KiB
    CHECK(kRomLdU >= 16 && kRomLdG >= 32 && kRomLdP >= 16);
    CHECK(kRomLdU % 2 == 0 && kRomLdG % 2 == 0);        // 16-byte reads
    CHECK(rom_lds_doubles() * sizeof(double) <= 64 * 1024);
    // partial tiles: a dense walk of the buffer, no index twice, none outside
    for (int nb : {1, 5, 33})
        for (int nt : {1, nb}) {
            const int ncells = 2 * kRomCellChunk + 1;
            const int nch = rom_chunks(ncells), nrt = rom_row_tiles(nt),
                      nct = rom_col_tiles(nb);
            const size_t np = rom_partials(ncells, nb, nt);
            std::vector<char> hit(np, 0);
            for (int c = 0; c < nch; ++c)
                for (int rt = 0; rt < nrt; ++rt)
                    for (int ct = 0; ct < nct; ++ct) {
                        const size_t at = rom_part_index(c, rt, ct, nrt, nct);
                        CHECK(at + 256 <= np);
                        for (int e = 0; e < 256; ++e) {
                            CHECK(!hit[at + e]);
                            hit[at + e] = 1;
                        }
                    }
            for (size_t i = 0; i < np; ++i) CHECK(hit[i]);
        }
    // the figure of the mesh refined twice (about 38k cells) at the limit
    CHECK(rom_partials(38400, 33, 33) * sizeof(double) ==
          (size_t)75 * 3 * 69 * 2048);
    CHECK(rom_partials(38400, 33, 33) * sizeof(double) < (size_t)64 << 20);
    // live cells: those without an inner dof come last
    {
        const int nc = 5;
        std::vector<int> cmap((size_t)12 * nc, -1);
        CHECK(rom_live_cells(cmap.data(), nc) == 0);
        cmap[(size_t)11 * nc + 2] = 7;          // cell 2, slot 11
        CHECK(rom_live_cells(cmap.data(), nc) == 3);
        cmap[(size_t)0 * nc + 4] = 0;
        CHECK(rom_live_cells(cmap.data(), nc) == 5);
        CHECK(rom_live_cells(cmap.data(), 0) == 0);
    }
    // shapes
    CHECK(check_rom_shape(33, 33, 60, 60, 1000) == DNS_OK);
    CHECK(check_rom_shape(33, 1, 60, 64, 0) == DNS_OK);
    CHECK(check_rom_shape(34, 1, 60, 60, 10) == DNS_ERR_BAD_ARGUMENT);
    CHECK(g_last_error.find("nb = 34") != std::string::npos);
    CHECK(check_rom_shape(0, 0, 60, 60, 10) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_rom_shape(5, 6, 60, 60, 10) == DNS_ERR_BAD_ARGUMENT);
    CHECK(g_last_error.find("nt = 6") != std::string::npos);
    CHECK(check_rom_shape(5, 0, 60, 60, 10) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_rom_shape(5, 5, 61, 61, 10) == DNS_ERR_BAD_ARGUMENT);  // odd
    CHECK(check_rom_shape(5, 5, 60, 58, 10) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_rom_shape(5, 5, 60, -2, 10) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_rom_shape(5, 5, 60, 60, -1) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_rom_shape(33, 33, 60, 60, 2000000000) ==
          DNS_ERR_BAD_ARGUMENT);                                 // partials
    CHECK(g_last_error.find("partial entries") != std::string::npos);
    printf("all checks passed\n");
    return 0;
}
