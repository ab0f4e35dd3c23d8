// Cycle length and batch length of the pipelined batches of dns_imex_run
// (imex_capi.inc): host arithmetic only, no HIP (tests/host_sanitize.cpp).
// (The sweeps' counterpart, constants of its own: newton_picard._CyclePolicy)
#pragma once
#include <algorithm>

namespace dns {

// a batch that went through: its first attempt's cycle length (before the
// restart clamp), the cycle of the attempt that went through (the second:
// `replayed`) and what the control block accumulated (k_arn_tail_acc)
struct BatchOutcome {
    bool over;                // oversolve (DnsCtl::stop_frac)
    int c_first, c;
    bool replayed;
    int maxit;                // acc_maxit
    double maxrel, maxprev;   // acc_maxrel, acc_maxprev: largest residual /
                              // tol behind / in front of the last column
};

struct BatchParams {
    int cmin;                 // dns_saddle::oversolve_cmin_eff()
    double raise, lower;      // dns_saddle::oversolve_raise / _lower
    bool two_one;             // mg_two_for(1) && !mg_two_for(2)
    bool slack_adapt;         // DNS_SLACK_ADAPT
    double noslack_maxrel;    // DNS_NOSLACK_MAXREL: no slack step while the
                              // batch maximum of residual / tol stays below
};

// what the last batch learnt is kept across dns_imex_run calls (a run is then
// 100 % graph replays from its first step on -- the driver's 20-step window
// sees what a 400-step window sees)
struct BatchPolicy {
    int cpred = -1;                // predicted cycle length of a batch
    bool noslack = false;
    int noslack_hold = 1;
    // oversolve policy (multigrid Schur block, DnsCtl::stop_frac): `cpred` is
    // then the cycle length itself; it comes down only when every solve of a
    // batch stood a decade below the tolerance in FRONT of its last column
    // and goes up, without a replay, when a batch ended close to it
    int lower_hold = 0, lower_backoff = 2;
    bool lowered_last = false, spiked = false;
    int batch_len = 8;             // steps per batch: 8 -> 16 -> 32 while the
                                   // predictions hold

    // a stepper that has its history (five solutions for the quartic warm
    // start, the iteration count of the last solve) goes straight to the
    // batches; a fresh one does its first steps one by one
    int startup_steps(int nsol) const {
        return (nsol >= 5 && cpred > 0) ? 0 : std::max(2, 5 - nsol);
    }
    void after_startup(int last_iters) {
        cpred = std::max(1, last_iters) + 1;
        noslack = false;
        noslack_hold = 1;
        batch_len = 8;
    }
    // after a batch that failed twice and was run step by step
    void after_fallback(int last_iters) {
        cpred = std::max(1, last_iters) + 2;
        noslack = false;
        noslack_hold = 8;          // batches before it is tried again
        batch_len = 8;
    }
    // the first attempt's cycle: no slack step while every solve of the last
    // batch ended a factor four below the tolerance in as many steps as
    // predicted (noslack)
    int cycle(bool over) const {
        return over ? std::max(1, cpred)
               : noslack ? std::max(1, cpred - 1)
                         : std::max(2, cpred);
    }
    // the second attempt's
    static int longer(int c, int cmax) { return std::min(c + 2, cmax); }

    void after_batch(const BatchOutcome &r, const BatchParams &p) {
        cpred = r.maxit + 1;
        // (a batch that needed its second attempt: the slack step stays for a
        // few batches, so that a residual hovering at the tolerance does not
        // cost a replay every other batch)
        if (r.replayed) noslack_hold = 4;
        if (noslack_hold > 0) --noslack_hold;
        noslack = p.slack_adapt && noslack_hold == 0 && r.maxrel > 0.0 &&
                  r.maxrel < p.noslack_maxrel && r.maxit <= r.c;
        if (r.over) {
            int cnext = r.c_first;
            bool trial = false;
            if (r.replayed && !lowered_last && !spiked) {
                // an established cycle length whose batch had to be replayed
                // ONCE: a residual spike (one or two solves of a batch, then
                // none for hundreds of steps at n = 2.8M) -- the replay has
                // dealt with it, the cycle stays; twice in a row raises it
                spiked = true;
            } else if (r.replayed || r.maxrel > p.raise) {
                // the cycle was too short (replayed) or ended close to the
                // tolerance: one more column.  A cycle that had just been
                // shortened: the next attempt waits twice as long (one
                // column less is not a matter of margins: the warm start
                // multiplies the final residuals of the last solves by its
                // coefficients, and a cycle whose reduction does not beat
                // that factor lets the start residuals grow step by step)
                cnext = r.c_first + 1;
                spiked = false;
                if (lowered_last) {
                    lower_backoff = std::min(1024, 2 * lower_backoff);
                    lower_hold = lower_backoff;
                } else {
                    // (an established cycle length that failed once: a
                    // residual spike -- back soon, on a trial batch)
                    lower_hold = 4;
                }
            } else if (r.maxit < r.c_first) {
                // every solve reached the floor (stop_frac x tol) before the
                // end of the cycle: the columns behind that are no-ops
                cnext = std::max(p.cmin, r.maxit);
            } else if (r.c_first > p.cmin && lower_hold == 0 &&
                       r.maxprev > 0.0 &&
                       (r.maxprev < p.lower ||
                        (r.c_first == 2 && p.two_one && r.maxrel < 0.5))) {
                // (second form: the one-column cycle applies TWO V-cycles
                // where these two columns applied one each -- a different
                // cycle, not this one cut short: what its first column left
                // says little about it, so it is simply tried while the
                // batch ended with a margin; a failed trial costs a replay
                // of eight steps and doubles the wait for the next one)
                // a decade below the tolerance in FRONT of the last column:
                // try one column less, on a short batch (what a failed
                // attempt replays)
                cnext = r.c_first - 1;
                trial = true;
            }
            if (!r.replayed) spiked = false;
            lowered_last = trial;
            if (lower_hold > 0) --lower_hold;
            cpred = cnext;
            noslack = false;
            if (trial) batch_len = 4;     // (doubled below: 8 steps)
        }
        batch_len = std::min(32, 2 * batch_len);
    }
};

}  // namespace dns
