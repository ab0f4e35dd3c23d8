// The host-only checks of the interpolation weights of a base trajectory
// (csrc/conv_host.hpp: check_base_rows_lerp, check_base_row_lerp,
// check_base_weight) WITHOUT HIP, under AddressSanitizer + UBSan:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover
//         -Iinclude tests/conv_interp_host_sanitize.cpp
//         -o conv_interp_host_sanitize
// The tables live in vectors of their exact length: a read past either end is
// the sanitizer's.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
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
    const double inf = std::numeric_limits<double>::infinity();
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double below1 = std::nextafter(1.0, 0.0);       // 1 - 2^-53
    const double tiny = std::ldexp(1.0, -60);
    const double denorm = std::numeric_limits<double>::denorm_min();
    const int m = 5;

    // ---- good tables -----------------------------------------------------------
    {
        std::vector<int32_t> up{0, 1, 2, 3, 4}, down{4, 3, 2, 1, 0},
            rep{0, 0, 0, 0, 1, 1, 1, 1, 2}, one{3};
        std::vector<double> wup{0.5, 0.25, 1.0 / 3, below1, 0.0},
            wdown{0.0, below1, 0.75, tiny, denorm},
            wrep{0.0, 0.25, 0.5, 0.75, 0.0, 0.25, 0.5, 0.75, 0.0}, wone{0.125};
        CHECK(check_base_rows_lerp(5, up.data(), wup.data(), m) == DNS_OK);
        CHECK(check_base_rows_lerp(5, down.data(), wdown.data(), m) == DNS_OK);
        CHECK(check_base_rows_lerp(9, rep.data(), wrep.data(), m) == DNS_OK);
        CHECK(check_base_rows_lerp(1, one.data(), wone.data(), m) == DNS_OK);
        // all weights zero: every row, the last one too
        std::vector<double> zero(5, 0.0);
        CHECK(check_base_rows_lerp(5, up.data(), zero.data(), m) == DNS_OK);
        // (-0.0 is zero: in [0, 1), and allowed on the last row)
        std::vector<double> negz(5, -0.0);
        CHECK(check_base_rows_lerp(5, up.data(), negz.data(), m) == DNS_OK);
        // a trajectory of one row takes weight 0 only
        std::vector<int32_t> r0{0, 0};
        std::vector<double> w0{0.0, 0.0}, w1{0.0, 0.5};
        CHECK(check_base_rows_lerp(2, r0.data(), w0.data(), 1) == DNS_OK);
        CHECK(check_base_rows_lerp(2, r0.data(), w1.data(), 1) ==
              DNS_ERR_BAD_ARGUMENT);
        CHECK(says("entry 1") && says("on row 0, the last of the 1 rows"));
    }

    // ---- a bad weight at every position, by name -----------------------------
    {
        std::vector<int32_t> rows{0, 1, 2, 3, 3, 2};
        std::vector<double> good{0.5, 0.25, 0.0, 0.75, below1, tiny};
        CHECK(check_base_rows_lerp(6, rows.data(), good.data(), m) == DNS_OK);
        for (size_t k = 0; k < rows.size(); ++k)
            for (double bad : {1.0, -tiny, -1.0, 1.5, inf, -inf, nan,
                               std::nextafter(1.0, 2.0), -denorm}) {
                std::vector<double> w = good;
                w[k] = bad;
                CHECK(check_base_rows_lerp(6, rows.data(), w.data(), m) ==
                      DNS_ERR_BAD_ARGUMENT);
                char want[64];
                snprintf(want, sizeof want, "base rows: entry %d has", (int)k);
                CHECK(says(want));
                CHECK(says("outside [0, 1)"));
                CHECK(g_last_error.find("linearised convection") == 0);
            }
        // a non-zero weight on the last row, wherever it stands
        for (size_t k = 0; k < rows.size(); ++k) {
            std::vector<int32_t> r = rows;
            r[k] = m - 1;
            std::vector<double> w = good;
            w[k] = tiny;
            CHECK(check_base_rows_lerp(6, r.data(), w.data(), m) ==
                  DNS_ERR_BAD_ARGUMENT);
            char want[96];
            snprintf(want, sizeof want, "base rows: entry %d:", (int)k);
            CHECK(says(want));
            CHECK(says("on row 4, the last of the 5 rows"));
            CHECK(says("no row 5 to interpolate towards"));
            w[k] = 0.0;
            CHECK(check_base_rows_lerp(6, r.data(), w.data(), m) == DNS_OK);
        }
    }

    // ---- the rows are checked first, like check_base_rows ---------------------
    {
        std::vector<int32_t> rows{0, 5, 1};
        std::vector<double> w{0.5, nan, 0.5};
        CHECK(check_base_rows_lerp(3, rows.data(), w.data(), m) ==
              DNS_ERR_BAD_ARGUMENT);
        CHECK(says("entry 1 is 5, outside 0..4"));
        std::vector<int32_t> big{INT_MAX};
        std::vector<double> wb{0.5};
        CHECK(check_base_rows_lerp(1, big.data(), wb.data(), m) ==
              DNS_ERR_BAD_ARGUMENT);
        std::vector<int32_t> ok{0, 1};
        std::vector<double> wok{0.5, 0.5};
        CHECK(check_base_rows_lerp(2, ok.data(), nullptr, m) ==
              DNS_ERR_BAD_ARGUMENT);
        CHECK(says("2 entries without their interpolation weights"));
        CHECK(check_base_rows_lerp(2, nullptr, wok.data(), m) ==
              DNS_ERR_BAD_ARGUMENT);
        CHECK(check_base_rows_lerp(0, ok.data(), wok.data(), m) ==
              DNS_ERR_BAD_ARGUMENT);
        CHECK(check_base_rows_lerp(-1, ok.data(), wok.data(), m) ==
              DNS_ERR_BAD_ARGUMENT);
        // weights without a trajectory
        CHECK(check_base_rows_lerp(2, ok.data(), wok.data(), 0) ==
              DNS_ERR_BAD_ARGUMENT);
        CHECK(says("without a base trajectory"));
    }

    // ---- the single host-named row ----------------------------------------------
    CHECK(check_base_row_lerp(0, 0.5, m) == DNS_OK);
    CHECK(check_base_row_lerp(3, below1, m) == DNS_OK);
    CHECK(check_base_row_lerp(4, 0.0, m) == DNS_OK);
    CHECK(check_base_row_lerp(0, 0.0, 1) == DNS_OK);
    CHECK(check_base_row_lerp(4, 0.5, m) == DNS_ERR_BAD_ARGUMENT);
    CHECK(says("base row 4:") && says("the last of the 5 rows"));
    CHECK(check_base_row_lerp(2, 1.0, m) == DNS_ERR_BAD_ARGUMENT);
    CHECK(says("base row 2 has the interpolation weight 1, outside [0, 1)"));
    CHECK(check_base_row_lerp(2, nan, m) == DNS_ERR_BAD_ARGUMENT);
    CHECK(says("outside [0, 1)"));
    CHECK(check_base_row_lerp(2, -inf, m) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_base_row_lerp(5, 0.5, m) == DNS_ERR_BAD_ARGUMENT);
    CHECK(says("base row 5 outside 0..4"));
    CHECK(check_base_row_lerp(-1, 0.0, m) == DNS_ERR_BAD_ARGUMENT);
    CHECK(check_base_row_lerp(0, 0.5, 0) == DNS_ERR_BAD_ARGUMENT);
    CHECK(says("without a base trajectory"));
    // (row + 1 does not exist in int)
    CHECK(check_base_weight(-1, INT_MAX, 0.5, INT_MAX) ==
          DNS_ERR_BAD_ARGUMENT);
    CHECK(check_base_weight(0, INT_MAX - 1, 0.5, INT_MAX) ==
          DNS_ERR_BAD_ARGUMENT);
    CHECK(check_base_weight(0, INT_MAX - 2, 0.5, INT_MAX) == DNS_OK);
    printf("all checks passed\n");
    return 0;
}
