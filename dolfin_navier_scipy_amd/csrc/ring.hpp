// The solution ring of the resident time steppers (dns_imex, dns_trap) and
// the polynomial warm start drawn from it: host arithmetic only, no HIP
// (tests/host_sanitize.cpp).
#pragma once
#include <algorithm>

namespace dns {

// Six [v; p~] vectors used as a ring: the current solution, the four before
// it, and the work buffer the next solve writes.  `nsol`: how many of them
// are valid solutions (0..5).  `pre_ok`: the work buffer already holds this
// step's warm start (written by the previous step's tail kernel,
// dns::TailExtrap) for the coefficient set `pre_sig` = extrap_sig(nsol, order).
struct Ring {
    int cur = 0, prev = 1, pprev = 2, p3 = 3, p4 = 4, work = 5;
    int nsol = 0;
    bool pre_ok = false;
    int pre_sig = -1;

    void reset(int nsol_) {
        cur = 0;
        prev = 1;
        pprev = 2;
        p3 = 3;
        p4 = 4;
        work = 5;
        nsol = nsol_;
        pre_ok = false;
        pre_sig = -1;
    }
    void rotate() {           // p4 <- p3 <- pprev <- prev <- cur <- new
        const int old = p4;
        p4 = p3;
        p3 = pprev;
        pprev = prev;
        prev = cur;
        cur = work;
        work = old;
        if (nsol < 5) nsol++;
    }
};

// the warm start's coefficient set, for Ring::pre_sig
inline int extrap_sig(int nsol, int order) {
    return 8 * std::min(nsol, 5) + std::min(order, 7);
}

// coefficients of the polynomial warm start from `nsol_` solutions; returns
// the order used (0..4)
constexpr int kExtrapFit35 = 13;
inline int extrap_coeffs(int nsol_, int order, double e[5]) {
    e[0] = 1.0;
    e[1] = e[2] = e[3] = e[4] = 0.0;
    if (nsol_ >= 5 && order == kExtrapFit35) {
        // value at the new time of the CUBIC least-squares fit through the
        // last FIVE solutions.  A warm start multiplies the final
        // residuals of the solves it is built from by its coefficients:
        // sqrt(sum c^2) = 4.9 here against 15.8 for the interpolating
        // quartic (8.3 cubic), for 1.8 x the cubic's truncation error --
        // once the start residual consists of those residuals rather
        // than of the truncation error (dt <= 1e-3: scripts/
        // recycle_probe.py) that is the better trade
        e[0] = 3.2; e[1] = -2.8; e[2] = -0.8; e[3] = 2.2; e[4] = -0.8;
        return 3;
    }
    if (order == kExtrapFit35) order = 3;      // (history still filling)
    if (nsol_ >= 5 && order >= 4) {
        e[0] = 5.0; e[1] = -10.0; e[2] = 10.0; e[3] = -5.0; e[4] = 1.0;
        return 4;
    }
    if (nsol_ >= 4 && order >= 3) {
        e[0] = 4.0; e[1] = -6.0; e[2] = 4.0; e[3] = -1.0;
        return 3;
    }
    if (nsol_ >= 3 && order >= 2) {
        e[0] = 3.0; e[1] = -3.0; e[2] = 1.0;
        return 2;
    }
    if (nsol_ >= 2 && order >= 1) {
        e[0] = 2.0; e[1] = -1.0;
        return 1;
    }
    return 0;
}

}  // namespace dns
