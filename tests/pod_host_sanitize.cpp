// The host-only parts of the snapshot ensemble (csrc/ensemble_host.hpp: layout
// arithmetic, the slot-table and shape checks, the packing of the combine
// coefficients) WITHOUT HIP, under AddressSanitizer + UBSan:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover
//         -Iinclude tests/pod_host_sanitize.cpp -o pod_host_sanitize
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../dolfin_navier_scipy_amd/csrc/ensemble_host.hpp"

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

int main() {
    using namespace dns;
    // layout
    CHECK(ens_ldv(1) == 64 && ens_ldv(64) == 64 && ens_ldv(65) == 128);
    CHECK(ens_blocks(1) == 1 && ens_blocks(16) == 1 && ens_blocks(17) == 2);
    CHECK(ens_chunks(1) == 1 && ens_chunks(kEnsChunk) == 1 &&
          ens_chunks(kEnsChunk + 1) == 2);
    CHECK(ens_passes(1) == 1 && ens_passes(16) == 1 && ens_passes(17) == 2);
    CHECK(ens_partials(33, 2 * kEnsChunk + 37) == (size_t)3 * 3 * 256);
    // the tile map is a bijection of 0..255 onto 16 x 16
    std::set<int> seen;
    for (int e = 0; e < 256; ++e) {
        const int r = ens_tile_row(e), c = ens_tile_col(e);
        CHECK(r >= 0 && r < 16 && c >= 0 && c < 16);
        seen.insert(16 * r + c);
    }
    CHECK(seen.size() == 256);
    // (lane 17, register 2: row (17 >> 4) + 4 * 2, column 17 & 15)
    CHECK(ens_tile_row(2 * 64 + 17) == 9 && ens_tile_col(2 * 64 + 17) == 1);
    // slot tables
    std::vector<int32_t> slot = {0, -1, 1, 2, -1, 3};
    CHECK(check_slot_table(6, slot.data(), 4) == DNS_OK);
    CHECK(check_slot_table(6, slot.data(), 3) == DNS_ERR_BAD_ARGUMENT);
    CHECK(g_last_error.find("slot[5] = 3") != std::string::npos);
    slot[1] = -2;
    CHECK(check_slot_table(6, slot.data(), 4) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_slot_table(0, slot.data(), 4) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_slot_table(6, slot.data(), 0) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_slot_table(6, nullptr, 4) == DNS_ERR_BAD_ARGUMENT);
    // shapes
    CHECK(check_ensemble_shape(9, 60, 64) == DNS_OK);
    CHECK(check_ensemble_shape(9, 60, 60) == DNS_OK);
    CHECK(check_ensemble_shape(9, 61, 61) == DNS_ERR_BAD_ARGUMENT);   // odd
    CHECK(check_ensemble_shape(9, 60, 58) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_ensemble_shape(0, 60, 64) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_ensemble_shape(9, 0, 64) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_ensemble_shape(1 << 20, 1 << 30, (size_t)1 << 30) ==
          DNS_ERR_BAD_ARGUMENT);                                 // partials
    // packing: every coefficient at its place, zeros behind r
    for (int r : {1, 16, 17, 35})
        for (int m : {1, 9, 33}) {
            std::vector<double> coef((size_t)r * m);
            for (size_t i = 0; i < coef.size(); ++i) coef[i] = 1.0 + (double)i;
            const std::vector<double> c = ens_pack_coef(coef.data(), r, m);
            CHECK(c.size() == (size_t)ens_passes(r) * m * kEnsAcc);
            size_t nonzero = 0;
            for (int p = 0; p < ens_passes(r); ++p)
                for (int s = 0; s < m; ++s)
                    for (int q = 0; q < kEnsAcc; ++q) {
                        const double v = c[((size_t)p * m + s) * kEnsAcc + q];
                        const int row = p * kEnsAcc + q;
                        if (row < r) {
                            CHECK(v == coef[(size_t)row * m + s]);
                            ++nonzero;
                        } else {
                            CHECK(v == 0.0);
                        }
                    }
            CHECK(nonzero == coef.size());
        }
    printf("all checks passed\n");
    return 0;
}
