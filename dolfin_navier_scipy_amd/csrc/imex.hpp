// Device-resident IMEX stepper state (CNAB / SBDF2 inner loops).
#pragma once
#include "attach_host.hpp"
#include "batch_policy.hpp"
#include "convection.hpp"
#include "ensemble.hpp"
#include "feedback.hpp"
#include "functional.hpp"
#include "quadratic.hpp"
#include "record.hpp"
#include "ring.hpp"
#include "solver.hpp"
#include "stats.hpp"
#include "trap.hpp"
#include "step_kernels.hpp"
#include <memory>

// The form of one resident step, decided ONCE (dns_imex::plan): the front of
// the step, the hooks the solver is handed and the bookkeeping behind a
// replayed graph all read it.
struct StepPlan {
    // the front of the step: k_step_one2; k_step_front (MODE `mode`: 0 plain,
    // 1 PRE, 2 carry) + k_step_back; k_dist_front; kernels of their own
    enum Form { Plain, Six, Fused, DistFront, Rows, StreamRhs, StreamRows };
    Form form = Plain;
    int mode = 0;
    // (each flag is said where it is decided: dns_imex::plan)
    bool can_pre = false, use_pre = false, carry = false, dcarry = false,
         dtail = false, have_cells = false, zwide = false;
    // injective: three bits of form, two of mode, one per flag
    uint64_t key() const {
        return (uint64_t)form | (uint64_t)mode << 3 | (uint64_t)can_pre << 5 |
               (uint64_t)use_pre << 6 | (uint64_t)carry << 7 |
               (uint64_t)dcarry << 8 | (uint64_t)dtail << 9 |
               (uint64_t)have_cells << 10 | (uint64_t)zwide << 11;
    }
};

// (dns::Ring: the ring indices of xs, nsol, and whether the work buffer holds
// the warm start already)
struct dns_imex : dns::Ring {
    dns_saddle *sys = nullptr;
    dns::CsrDev R1;                // all rows, or this rank's (partitioned)
    dns::HostCsr R1h;              // host copy (row blocks are cut from it)
    bool r1_rows = false;          // R1h holds this rank's rows only
                                   // (dns_imex_create_rows)
    // pair format of R1 (2x2 node blocks, pair.hpp) for the streamed
    // right-hand-side product of the bandwidth regime: R1 = M - theta dt A has
    // the block structure of F (8.5 instead of 10 bytes per non-zero, a third
    // of the gather addresses); absent when R1 is not streamed or NV is odd
    dns::PairDev R1p;
    int build_r1_pair(const dns::HostCsr &rows, int v0);
    // row-partitioned system (dist_solve.inc): the right-hand side is formed
    // for this rank's rows only -- R1 by rows, the convection from the cells
    // that touch them -- and the solution's halo entries are exchanged by
    // index lists (footprints of K, R1 and those cells) instead of gathering
    // the whole vector
    struct Partition {
        bool on = false;
        uint64_t gen = 0;          // sys->dist_generation it was built for
        const dns_conv *conv_for = nullptr;
        dns_halo_plan planX;
        dns::DevBuf<int> conv_sel;
        int nsel = 0;
        bool state_full = true;    // xs[cur] holds every rank's rows
    } part;
    int ensure_partition();
    int gather_state();
    // current and the four solutions before it, work
    dns::DevBuf<double> xs[6];
    // checkpoint of a pipelined batch: the ring (the work buffer too: it
    // holds the warm start), the convection history and, when residuals are
    // carried, the last right-hand side and residual and the two residuals
    // of the six-node / partitioned step
    dns::Checkpoint ck;
    // residual carry-over (dns_imex_coeffs.carry_residual, k_step_front MODE 2):
    // K xs[i] per ring slot and the velocity residual of the previous solve;
    // `b_valid`: b holds the right-hand side whose solution is xs[cur];
    // `carry_ok`: kxs[prev..p4] are K times the ring as it stands (primed by
    // prime_carry or kept current by carry steps)
    dns::DevBuf<double> kxs[6], rcarry;
    bool b_valid = false, carry_ok = false;
    int prime_carry(bool zero_r);
    // six-node step (step_kernels.hpp): the warm start lives in x0buf[work & 1]
    // (the tail reads one and writes the other), the residuals of the last two
    // solves in rc6[.] (same parity), the convection cell values are produced
    // by the tail of the step before.  `six_ok`: x0buf / cell values / rc6 are
    // those of the ring as it stands (primed by prime_six or kept by six-node
    // steps); DNS_STEP6=0 keeps the seven-node step
    dns::DevBuf<double> x0buf[2], rc6[2], kx6;
    bool six_ok = false, env_six = true;
    bool env_dfront = true;   // DNS_DIST_FRONT: one-launch front of a partitioned step
    // row-partitioned step whose one-step cycle ends in k_arn_tail_lazy1: the
    // tail evaluates the convection cells of the new velocity (DNS_DIST_TAIL,
    // the step is 7 kernels instead of 8).  `dcells_ok`: the cell values on
    // the device are those of xs[cur] for the boundary values of generation
    // `dcells_gen` (left by such a tail or by prime_dcells)
    bool env_dtail = true, dcells_ok = false;
    uint64_t dcells_gen = 0;
    dns::DevBuf<double> x0c;       // the warm start, copied by the front
    // steps BUILT (launched or captured; a replayed graph is not counted), of
    // them: with the cells in the tail / with the cell kernel left out because
    // the tail before had run it (dns_imex_step_counters: tests)
    int64_t n_steps_built = 0, n_steps_tail_cells = 0, n_steps_cells_reused = 0;
    int prime_dcells(const dns_imex_coeffs *cf, const dns_solve_opts *o);
    uint64_t six_conv_gen = 0;     // conv->dbc_gen the cell values belong to
    bool six_capable() const;
    int prime_six(const dns_imex_coeffs *cf, bool keep_r);
    long steps_enqueued = 0;       // counts step_device calls (graph replay
                                   // must advance the host state itself)
    dns::DevBuf<double> nfc[2];
    int nc = 0, no = 1;
    dns::DevBuf<double> g, gp, b;
    // per-step right-hand sides known in advance (time-dependent forcing,
    // moving Dirichlet data: what the reference's `f_tdp`, `g_tdp`, `applybcs`
    // callbacks return, tiu:114-127): row s of the tables replaces g / gp in
    // step s after the upload; `stepctr` lives on the device so that replayed
    // graphs walk through the tables without the host
    dns::DevBuf<double> gtab, gptab;
    dns::DevBuf<int> stepctr;
    int tab_rows = 0;              // 0: no table, g / gp are used
    bool tab_v = false, tab_p = false;
    int tab_pos{0};                // host copy of the counter
    bool preparing = false;        // prepare_graphs is capturing (no launch)
    // the last prepare_graphs call went past its "already prepared" exit, i.e.
    // it captured (or tried to): the same on every rank of a partitioned run
    bool prepare_attempted = false;
    // observer feedback (feedback.hpp): k_lti_step runs in front of every
    // step and leaves the right-hand side with the actuation in `geff`, which
    // the front kernels then read through g_ref().  The state slot that holds
    // the current hx / f_last / u_c is `tab_pos & 1`: the step counter selects
    // the slot, the drift row and the log row alike, so a restored batch
    // (HostState::tab_pos, sync_counter) replays all three.  Present = on.
    struct Feedback {
        int hN = 0, Ny = 0, Nu = 0;
        int rows = 0;              // drift rows = log capacity (0: no table yet)
        bool has_drift = false;
        double dt = 0.0, c_n = 0.0, c_c = 0.0;
        dns::CsrDev C, B;
        // (geff: NV entries, in the boundary mode NV + NP -- gpeff lies behind
        // it in ONE buffer: one entry of a checkpoint)
        dns::DevBuf<double> haT, hbT, hc, drift, state, ylog, ulog, geff;
        // boundary actuation (dns_imex_set_feedback_boundary): k_lti_bc_step
        // in the place of k_lti_step.  It also writes the controlled columns
        // [col0, col0 + nc) of row `counter + 1` of the convection operator's
        // Dirichlet table, and the slot keeps u_p behind u_c.  `rhs`: the
        // boundary terms Ba, Bm, Bj were given (else they stay empty, their
        // pointers null).  Present = boundary mode.
        struct Boundary {
            bool rhs = false;
            int nc = 0, col0 = 0;
            dns::CsrDev S, Ba, Bm, Bj;
            dns::DevBuf<double> base;
            double wm[3] = {0, 0, 0}, wa[3] = {0, 0, 0};
        };
        std::unique_ptr<Boundary> bc;
        bool has_b() const { return B.nnz > 0; }
        int stride() const { return 2 * hN + Nu + (bc ? Nu : 0); }
        // does the step read geff / gpeff?
        bool rhs_v() const { return !bc || bc->rhs || has_b(); }
        bool rhs_p() const { return bc && bc->rhs; }
        double *gpeff(int nv) const { return rhs_p() ? geff.p + nv : nullptr; }
    };
    std::unique_ptr<Feedback> fb;
    int fb_launch(hipStream_t s);  // k_lti_step / k_lti_bc_step for the step
                                   // about to run
    uint64_t fb_key() const;
    // The other five (their place among the nodes: attachments()) run in
    // front of every step and once behind the last step of a call and work on
    // row `counter - 1`: a restored batch overwrites its own rows, so their
    // buffers need no checkpoint (the statistics ADD: see there).  Present = on.
    //
    // trajectory recorder (record.hpp): k_record_step.
    struct Recorder {
        int rows = 0;              // steps the slot table / the y log cover
        int Ny = 0, nslots = 0;    // 0: no outputs / no snapshots
        std::unique_ptr<dns::CsrDev> C;
        dns::HostCsr Ch;           // (what C holds: the same matrix set again
                                   // keeps the device copy)
        dns::DevBuf<int> slot;
        dns::DevBuf<double> snap, ylog;
    };
    std::unique_ptr<Recorder> rec;
    int rec_launch(hipStream_t s); // k_record_step for the state as it stands
    uint64_t rec_key() const;
    // The Dirichlet values of functionals and quadratics: constant (`ndbc` =
    // 0), a table of their own (`gtab`, `rows` + 1 rows of `ndbc`: the `_bc`
    // setters) or, `live`, the attached convection operator's table, which
    // boundary feedback writes (the `_live` setters).
    struct MovingBc {
        int ndbc = 0;
        dns::DevBuf<double> gtab;
        bool live = false;
        bool moving() const { return ndbc > 0; }
        // the table in use (check_step has seen to a live one's shape)
        struct Table {
            const double *p;
            int stride, rows;
        };
        Table table(const dns_imex &st, int rows) const {
            if (live && st.conv)
                return {st.conv->dbc_tab.p, std::max(1, st.conv->ndbc),
                        st.conv->dbc_rows};
            return {gtab.p, ndbc, rows + 1};
        }
        uint64_t key(uint64_t k, const dns_imex &st, int rows) const;
        // a setter's refusals (`const_refusal`: constant values beside a
        // per-step table on the operator), then its upload
        static int check_set(const dns_imex &st, const char *noun,
                             const char *const_refusal, bool moving, bool live,
                             int ndbc, int rows);
        int set(bool moving, bool live, int ndbc, int rows,
                const double *dbc_table, hipStream_t s);
        // a step's refusals: the operator may have changed since
        int check_step(const dns_imex &st, int rows, const char *noun,
                       const char *setter, const char *const_refusal) const;
    };
    // Their log: the share of each of `G` workgroups in each of `n` entries of
    // every row, zeroed when set, summed in index order by the getters.
    struct ShareLog {
        dns::DevBuf<double> buf;
        int G = 1, n = 0, rows = 0;
        int ensure(int rows, int G, int n, hipStream_t s);
        int download_sums(dns_imex *st, int first, int count, double *out,
                          const char *what) const;
    };
    // force functionals (functional.hpp): k_functional_step.
    struct Functionals {
        int nF = 0;
        int ncl = 0;               // listed cells (all functionals)
        double dt = 1.0;
        dns::DevBuf<int> rp, ci;   // the 3 nF (moving: 5 nF) sparse rows
        dns::DevBuf<double> va;    // (k, term)
        dns::DevBuf<int> cptr, cidx;
        dns::DevBuf<double> cw, scale, c0;
        ShareLog log;              // rows x G x nF
        MovingBc bc;               // (moving: the terms cab, cmb are there)
        // the convection operator whose cell order `cidx` refers to (a step
        // with another one attached is refused)
        const dns_conv *conv = nullptr;
        int ncells = 0;
        const int *cellmap = nullptr;
    };
    std::unique_ptr<Functionals> fn;
    int fn_launch(hipStream_t s);  // k_functional_step for the state as it stands
    uint64_t fn_key() const;
    // flow statistics (stats.hpp): k_stats_step ADDS its row to running sums,
    // so -- unlike the rows of the others -- a row must not be seen twice: the
    // workgroups' marks (the head of `acc`) drop the second launch for a row,
    // rewind_tables() zeroes them with the counter, and a batch checkpoints
    // `acc` as a whole (`ck_st`: `ck` can be full without it).
    struct Statistics {
        dns::StLayout lay;
        int rows = 0;              // steps the bin table covers
        std::vector<int> pi, pj;   // (the same pairs set again keep the sums)
        dns::DevBuf<int> bin;
        dns::DevBuf<int2> pairs;
        dns::DevBuf<double> acc;
    };
    std::unique_ptr<Statistics> stat;
    dns::Checkpoint ck_st;
    int st_launch(hipStream_t s);  // k_stats_step for the state as it stands
    uint64_t st_key() const;
    // quadratic functionals (quadratic.hpp): k_quadratic_step.  The matrices
    // stay on the device across calls that hand over the same ones (`Qh`:
    // what the device holds).
    struct Quadratics {
        int nM = 0, nQ = 0;
        double dt = 1.0;
        int mat[dns::kQdMaxForms] = {}, lop[dns::kQdMaxForms] = {},
            rop[dns::kQdMaxForms] = {};
        int need[dns::kQdMaxMats] = {};
        long long nzbase[dns::kQdMaxMats] = {};
        struct HostMat {
            std::vector<int> rp, ci;
            std::vector<double> va;
        };
        std::vector<HostMat> Qh;
        dns::DevBuf<int> rp, ci;   // the nM matrices, one behind the other
        dns::DevBuf<double> va;
        dns::DevBuf<int> lrp, lci; // the 2 nQ sparse rows (k, qa / qw)
        dns::DevBuf<double> lva, scale, c0;
        ShareLog log;              // rows x G x nQ
        MovingBc bc;               // (moving: matrices and sparse rows are
                                   // nv + ndbc wide)
    };
    std::unique_ptr<Quadratics> qd;
    int check_live(const char *noun, int ndbc, int rows) const;
    int qd_launch(hipStream_t s);  // k_quadratic_step for the state as it stands
    uint64_t qd_key() const;
    // snapshot ensemble (ensemble.hpp): k_ensemble_step copies v into slot
    // `slot[counter - 1]` of E, which the stepper owns ACROSS the slices of a
    // time loop (they re-arm the slot table only).  The Gram matrix and the
    // linear combinations run behind the loop as plain launches (`W`: the
    // weights as uploaded last, `Wh` what they are; `y`, `part`, `gm`, `cf`,
    // `out`: their scratch).
    struct Ensemble {
        int rows = 0, nslots = 0;
        size_t ldv = 0;
        dns::DevBuf<int> slot;
        dns::DevBuf<double> E;
        std::unique_ptr<dns::EnsWeights> W;
        dns::HostCsr Wh;
        dns::DevBuf<double> y, part, gm, cf, out;
    };
    std::unique_ptr<Ensemble> ens;
    int ens_launch(hipStream_t s); // k_ensemble_step for the state as it stands
    uint64_t ens_key() const;
    // What the six have in common (imex_attach_capi.inc): attachments() lists
    // those present, in launch order -- noun, why a row-partitioned stepper
    // refuses it, rows of its table, whether it runs behind the last step of
    // a call too, its part of a captured step's key, its launch.  Front and
    // closing nodes, key, refusals and the counter's limits loop over it.
    struct Attachment {
        const char *noun, *partitioned;
        int rows;
        bool closing;
        uint64_t (dns_imex::*key)() const;
        int (dns_imex::*launch)(hipStream_t);
    };
    struct Attachments {
        Attachment a[6];
        int n = 0;
        const Attachment *begin() const { return a; }
        const Attachment *end() const { return a + n; }
    };
    Attachments attachments() const;
    int launch_front_nodes(hipStream_t s);
    int launch_closing_nodes(hipStream_t s);
    uint64_t attachments_key(uint64_t k) const;
    int refuse_partitioned(const char *noun, const char *reason) const;
    int check_attachments() const;
    // a step counter is needed as soon as anything is tabulated
    bool tables() const;
    int rows_left() const;
    int rewind_tables();           // new tables: the counter back to 0
    // a new index table on the operator (dns_conv_set_base_rows) is a new
    // table: seen by the next dns_imex_step / dns_imex_run
    uint64_t brow_gen_seen = 0;
    int adopt_base_rows();
    dns::TabRef g_src() const {
        if (tab_rows > 0 && tab_v)
            return {gtab.p, stepctr.p, sys->nv, tab_rows};
        return {g.p, nullptr, 0, 1};
    }
    // (with feedback: what k_lti_step has made of g_src() for this step)
    dns::TabRef g_ref() const {
        if (fb && fb->rhs_v()) return {fb->geff.p, nullptr, 0, 1};
        return g_src();
    }
    dns::TabRef gp_src() const {
        if (tab_rows > 0 && tab_p)
            return {gptab.p, stepctr.p, std::max(1, sys->np), tab_rows};
        return {gp.p, nullptr, 0, 1};
    }
    // (with boundary feedback and its terms: what k_lti_bc_step has made of it)
    dns::TabRef gp_ref() const {
        if (fb && fb->rhs_p()) return {fb->gpeff(sys->nv), nullptr, 0, 1};
        return gp_src();
    }
    int sync_counter();            // device counter <- tab_pos
    double last_pscale = 1.0;
    dns_conv *conv = nullptr;      // device convection: nfc_c = scale*N(v_c)v_c
    double conv_scale = -1.0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    dns::BatchPolicy policy;       // cycle length and length of the batches
    uint64_t prepared_sig = 0;     // configuration the graphs were captured for
    int chi_hi = 0;                // longest cycle length they cover (with hysteresis)
    // record of the last dns_imex_run (dns_imex_run_info)
    int run_unconverged = 0, run_first_bad = -1, run_replayed = 0;
    // six-node steps of the accepted batches of the last run, by the kind of
    // their cycle (lazy one-column / general)
    int64_t run_lazy_steps = 0, run_eager_steps = 0;
    int run_captures = 0;          // graphs captured inside the last run
    // knobs read ONCE, when the stepper is created
    bool env_step_history = false, env_debug = false, env_slack_adapt = true;
    int env_group = 8;
    double env_noslack_maxrel = 0.85;   // DNS_NOSLACK_MAXREL (BatchParams)
    // steps in the next graph of a batch with `left` steps to go: groups of
    // env_group (at most 32), for the tail of a batch groups of half as many
    // (from 4 on: a 20-step call is 8 + 8 + 4 = three launches), single steps
    int group_for(int left) const {
        const int g = std::max(1, std::min(env_group, 32));
        return left >= g ? g : (g >= 4 && left >= g / 2) ? g / 2 : 1;
    }
    struct HostState {
        dns::Ring ring;
        int nc, no, tab_pos;
        long steps_enqueued;
        bool b_valid, carry_ok, six_ok, dcells_ok;
        double last_pscale;        // (the recorder scales the pressure by it)
    };
    HostState host_state() const {
        return {*this, nc, no, tab_pos, steps_enqueued, b_valid, carry_ok,
                six_ok, dcells_ok, last_pscale};
    }
    void set_host_state(const HostState &s) {
        static_cast<dns::Ring &>(*this) = s.ring;
        nc = s.nc;
        no = s.no;
        tab_pos = s.tab_pos;
        steps_enqueued = s.steps_enqueued;
        b_valid = s.b_valid;
        carry_ok = s.carry_ok;
        six_ok = s.six_ok;
        dcells_ok = s.dcells_ok;
        last_pscale = s.last_pscale;
    }
    std::vector<uint64_t> group_key(const dns_imex_coeffs *cf,
                                    const dns_solve_opts *o, int group) const;
    int enqueue_group(const dns_imex_coeffs *cf, const dns_solve_opts *o,
                      int group, bool launch);
    int prepare_graphs(const dns_imex_coeffs *cf, const dns_solve_opts *o);
    ~dns_imex() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
    uint64_t config_key(const dns_imex_coeffs *cf) const;
    uint64_t step_key(const dns_imex_coeffs *cf) const;
    // gather lists and cell values of the device convection (nulls: none)
    struct ConvGather {
        const int *gptr = nullptr, *gidx = nullptr;
        const double *cellvals = nullptr;
    };
    ConvGather conv_gather() const {
        if (!conv) return {};
        return {conv->gptr.p, conv->gidx.p, conv->cellvals.p};
    }
    StepPlan plan(const dns_imex_coeffs *cf, const dns_solve_opts *o,
                  int cycle_len) const;
    // the front of a step by its form, and what they share
    int front_nparts(const StepPlan &pl) const;
    int warm_start(const dns_imex_coeffs *cf, const StepPlan &pl);
    int front_six(const dns_imex_coeffs *cf, const StepPlan &pl);
    int front_fused(const dns_imex_coeffs *cf, const StepPlan &pl);
    int front_dist(const dns_imex_coeffs *cf, const StepPlan &pl);
    int front_rows(const dns_imex_coeffs *cf, const StepPlan &pl);
    int front_stream(const dns_imex_coeffs *cf, const StepPlan &pl);
    int prologue(const dns_imex_coeffs *cf, const StepPlan &pl);
    dns::StepHooks hooks(const dns_imex_coeffs *cf, const StepPlan &pl);
    int step_device(const dns_imex_coeffs *cf, const dns_solve_opts *o,
                    dns_solve_stats *st, bool with_true_residual);
    // what dns_imex_step does before step_device: its refusals, the upload of
    // the caller's convection vector, the products of a carry step
    int step_refusals(const double *nfc_new) const;
    int step_preamble(const double *nfc_new, const dns_imex_coeffs *cf,
                      const dns_solve_opts &o);
    void turn_convection();
    // dns_imex_front_probe (TEST ONLY) has run a front without its solve: the
    // convection slot and the carry buffers are those of a step that never
    // finished.  dns_imex_set_state starts over.
    bool probed = false;
    int refuse_probed() const;
};
