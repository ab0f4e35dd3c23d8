// The host-only parts of the base trajectory of a linearised convection
// operator (csrc/conv_host.hpp: the layout arithmetic, the packing of the rows,
// the checks of the shapes, of the per-step index table, of a named row and of
// the ensemble slots) WITHOUT HIP, under AddressSanitizer + UBSan:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover
//         -Iinclude tests/conv_traj_host_sanitize.cpp -o conv_traj_host_sanitize
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../dolfin_navier_scipy_amd/csrc/conv_host.hpp"

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

static bool says(const char *word) {
    return dns::g_last_error.find(word) != std::string::npos;
}

int main() {
    using namespace dns;
    // ---- layout: ldv = nv rounded up to 64, offsets in size_t ---------------
    CHECK(base_traj_ldv(0) == 0 && base_traj_ldv(1) == 64);
    CHECK(base_traj_ldv(64) == 64 && base_traj_ldv(65) == 128);
    CHECK(base_traj_ldv(INT_MAX) == ((size_t)1 << 31));
    // (a row offset past 2^31 entries: no int arithmetic on the way)
    CHECK(base_traj_offset(INT_MAX, base_traj_ldv(INT_MAX)) ==
          (size_t)INT_MAX * ((size_t)1 << 31));
    CHECK(base_traj_offset(40000, base_traj_ldv(150001)) ==
          (size_t)40000 * 150016);
    CHECK(base_traj_dbc_stride(1, 7) == 0 && base_traj_dbc_stride(5, 7) == 7);
    CHECK(base_traj_dbc_stride(5, 0) == 1 && base_traj_dbc_stride(1, 0) == 0);

    // ---- packing: exact sizes, a read past either end is the sanitizer's ----
    for (int nv : {1, 5, 63, 64, 65, 130})
        for (int m : {1, 2, 5})
            for (int pad : {0, 3}) {
                const long ld = nv + pad;
                // (the last row ends at nv: nothing behind it belongs to us)
                std::vector<double> rows((size_t)(m - 1) * ld + nv), out;
                for (int r = 0; r < m; ++r)
                    for (int i = 0; i < nv; ++i)
                        rows[(size_t)r * ld + i] = 1000.0 * r + i + 0.5;
                CHECK(pack_base_trajectory(m, nv, rows.data(), ld, out) ==
                      DNS_OK);
                const size_t ldv = base_traj_ldv(nv);
                CHECK(out.size() == (size_t)m * ldv);
                for (int r = 0; r < m; ++r)
                    for (size_t i = 0; i < ldv; ++i)
                        CHECK(out[base_traj_offset(r, ldv) + i] ==
                              (i < (size_t)nv ? 1000.0 * r + i + 0.5 : 0.0));
            }
    {
        // no inner dof at all: nothing is read, one entry per row is kept
        std::vector<double> out;
        CHECK(pack_base_trajectory(3, 0, nullptr, 0, out) == DNS_OK);
        CHECK(out.size() == 3);
    }

    // ---- shapes ---------------------------------------------------------------
    {
        std::vector<double> v(10, 1.0), d(6, 2.0);
        CHECK(check_base_trajectory(2, 5, v.data(), 5, 1, 3, d.data()) ==
              DNS_OK);
        CHECK(check_base_trajectory(2, 5, v.data(), 5, 2, 3, d.data()) ==
              DNS_OK);
        CHECK(check_base_trajectory(1, 5, v.data(), 5, 1, 0, nullptr) ==
              DNS_OK);
        CHECK(check_base_trajectory(0, 5, v.data(), 5, 1, 3, d.data()) ==
              DNS_ERR_BAD_ARGUMENT);
        CHECK(says("base trajectory of 0 rows"));
        CHECK(check_base_trajectory(-3, 5, v.data(), 5, 1, 3, d.data()) ==
              DNS_ERR_BAD_ARGUMENT);
        CHECK(check_base_trajectory(2, 5, nullptr, 5, 1, 3, d.data()) ==
              DNS_ERR_BAD_ARGUMENT);
        CHECK(check_base_trajectory(2, 5, v.data(), 5, 1, 3, nullptr) ==
              DNS_ERR_BAD_ARGUMENT);
        CHECK(says("Dirichlet values (3)"));
        CHECK(check_base_trajectory(2, 5, v.data(), 4, 1, 3, d.data()) ==
              DNS_ERR_BAD_ARGUMENT);
        CHECK(says("rows 4 apart"));
        for (int sets : {0, 3, -1, INT_MAX}) {
            CHECK(check_base_trajectory(2, 5, v.data(), 5, sets, 3,
                                        d.data()) == DNS_ERR_BAD_ARGUMENT);
            CHECK(says("one set, or one per row"));
        }
        CHECK(g_last_error.find("linearised convection") == 0);
        // a refused shape packs nothing and leaves `out` alone
        std::vector<double> out(2, 7.0);
        CHECK(pack_base_trajectory(2, 5, v.data(), 4, out) ==
              DNS_ERR_BAD_ARGUMENT);
        CHECK(out.size() == 2 && out[0] == 7.0);
    }

    // ---- the per-step index table ----------------------------------------------
    {
        const int m = 5;
        std::vector<int32_t> up{0, 1, 2, 3, 4}, down{4, 3, 2, 1, 0},
            rep{0, 0, 1, 1, 2, 2}, one{4};
        for (const auto &t : {up, down, rep, one})
            CHECK(check_base_rows((int)t.size(), t.data(), m) == DNS_OK);
        // every position, one past either end, by name
        for (size_t k = 0; k < rep.size(); ++k)
            for (int32_t bad : {(int32_t)-1, (int32_t)m, (int32_t)INT_MIN,
                                (int32_t)INT_MAX}) {
                std::vector<int32_t> t = rep;
                t[k] = bad;
                CHECK(check_base_rows((int)t.size(), t.data(), m) ==
                      DNS_ERR_BAD_ARGUMENT);
                char want[64];
                snprintf(want, sizeof want, "entry %d is %d, outside 0..%d",
                         (int)k, (int)bad, m - 1);
                CHECK(says(want));
            }
        CHECK(check_base_rows(0, up.data(), m) == DNS_ERR_BAD_ARGUMENT);
        CHECK(check_base_rows(-1, up.data(), m) == DNS_ERR_BAD_ARGUMENT);
        CHECK(check_base_rows(5, nullptr, m) == DNS_ERR_BAD_ARGUMENT);
        CHECK(check_base_rows(5, up.data(), 0) == DNS_ERR_BAD_ARGUMENT);
        CHECK(says("without a base trajectory"));
    }

    // ---- a named row, the slots of an ensemble ---------------------------------
    CHECK(check_base_row(0, 1) == DNS_OK && check_base_row(4, 5) == DNS_OK);
    CHECK(check_base_row(5, 5) == DNS_ERR_BAD_ARGUMENT);
    CHECK(says("base row 5 outside 0..4"));
    CHECK(check_base_row(-1, 5) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_base_row(INT_MIN, 5) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_base_row(0, 0) == DNS_ERR_BAD_ARGUMENT);
    CHECK(says("without a base trajectory"));
    CHECK(check_base_slots(0, 6, 6) == DNS_OK);
    CHECK(check_base_slots(5, 1, 6) == DNS_OK);
    CHECK(check_base_slots(2, 4, 6) == DNS_OK);
    CHECK(check_base_slots(2, 5, 6) == DNS_ERR_BAD_ARGUMENT);
    CHECK(says("slots 2 .. 6 outside 0..5"));
    CHECK(check_base_slots(-1, 2, 6) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_base_slots(0, 0, 6) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_base_slots(6, 1, 6) == DNS_ERR_BAD_ARGUMENT);
    // (first + count does not exist in int)
    CHECK(check_base_slots(INT_MAX, INT_MAX, 6) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_base_slots(1, INT_MAX, INT_MAX) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_base_slots(0, INT_MAX, INT_MAX) == DNS_OK);
    printf("all checks passed\n");
    return 0;
}
