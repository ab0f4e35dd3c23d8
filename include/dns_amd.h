/*
 * dns_amd.h -- C-ABI of the MI355X (gfx950) saddle-point time-stepping path.
 *
 * Drop-in boundary for dolfin_navier_scipy's linear-algebra layer.  The
 * reference reaches its solver through the Python module
 * `sadptprj_riclyap_adi.lin_alg_utils` (un-vendored; call sites listed below)
 * and through `scipy.sparse.linalg.factorized`; the Python wrapper
 * `dolfin_navier_scipy_amd/lin_alg_utils.py` binds the entry points declared
 * here with `ctypes` and presents that same Python surface.
 *
 * Conventions
 *  - plain pointers and sizes only; all pointers are HOST pointers unless the
 *    name ends in `_dev`; buffers are borrowed for the duration of the call;
 *  - matrices are CSR with int32 indices and float64 values (what
 *    `dolfin_to_sparrays.mat_dolfin2sparse` produces, reference dts:67-81);
 *  - every function returns a status code (0 = ok); `dns_last_error()` gives
 *    the message of the last failure on the calling thread;
 *  - one host thread per handle, one HIP stream per handle.
 *
 * Saddle-point contract:
 *      [ F   JT ] [ v  ]   [ rhs_v ]
 *      [ J   0  ] [ p~ ] = [ rhs_p ]      F = M + theta*dt*(A [+ N(v_lin)])
 */
#ifndef DNS_AMD_H
#define DNS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DNS_OK               0
#define DNS_NOT_CONVERGED    1   /* maxiter reached, best iterate returned   */
#define DNS_BREAKDOWN        2   /* Krylov / factorisation breakdown         */
#define DNS_ERR_HIP          3   /* a HIP runtime call failed                */
#define DNS_ERR_BAD_ARGUMENT 4
#define DNS_ERR_NOT_READY    5   /* e.g. solve before the preconditioner     */
#define DNS_ERR_COMM         6   /* RCCL failure                             */
#define DNS_ERR_HOST         7   /* host-side failure inside the library (out
                                    of memory, a thread that cannot start):
                                    no C++ exception crosses this boundary   */

#define DNS_METHOD_GMRES     0
#define DNS_METHOD_BICGSTAB  1

#define DNS_SCHUR_DENSE      0   /* explicit inverse of J Fh^-1 JT (NP small) */
#define DNS_SCHUR_JACOBI     1   /* diag(J D^-1 JT)^-1  (always available)   */
#define DNS_SCHUR_MG         2   /* one multigrid V-cycle on the sparse Schur
                                    complement (dns_saddle_set_schur_mg)     */

#define DNS_SPMV_VECTOR      0   /* sub-wave per row, shuffle reduction      */
#define DNS_SPMV_STREAM      1   /* row blocks streamed through LDS          */
#define DNS_SPMV_STREAM16    2   /* the same, 16-bit column offsets per block */

typedef struct dns_saddle dns_saddle;   /* opaque: one saddle-point system  */
typedef struct dns_imex dns_imex;       /* opaque: device-resident stepper  */

typedef struct dns_csr {         /* host-side CSR view (borrowed)            */
    int32_t nrows, ncols;
    int64_t nnz;
    const int32_t *rowptr;       /* nrows+1 */
    const int32_t *colidx;       /* nnz     */
    const double  *vals;         /* nnz     */
} dns_csr;

#define DNS_FHAT_CHEB        0   /* Chebyshev recurrence: degree-1 SpMVs/apply */
#define DNS_FHAT_EXPLICIT    1   /* same polynomial as ONE explicit CSR matrix */
#define DNS_FHAT_AUTO        2   /* explicit while the system is launch-bound  */

/* block structure of the right preconditioner (both use the same Fh^-1 and the
 * same Sh = J Fh^-1 JT):
 *   TRIANGULAR  P = [[Fh, JT], [0, -Sh]]            one Fh^-1 apply
 *   FULL        P = [[Fh, JT], [J, 0]] exactly (block LDU):
 *               zp = -Sh^-1 (rp - J Fh^-1 rv),  zv = Fh^-1 (rv - JT zp)
 *               one more sparse product (J Fh^-1, formed explicitly) per
 *               apply; needs the explicit Fh^-1 and one GPU.  With a residual
 *               whose pressure part vanishes (warm-started time steps) the
 *               triangular form spends two Krylov steps before it starts to
 *               converge; the full form gains ~2 orders in its first step.  */
#define DNS_FACT_TRIANGULAR  0
#define DNS_FACT_FULL        1

typedef struct dns_precond_opts {
    int32_t cheb_degree;         /* terms of the Jacobi-Chebyshev F^-1 (>=1) */
    int32_t schur;               /* DNS_SCHUR_*                              */
    int32_t fhat;                /* DNS_FHAT_*                               */
    int32_t fp32_store;          /* 1: keep the explicit preconditioner
                                    matrices (Gc values, Schur inverse) in
                                    fp32 -- halves their bytes; the Krylov
                                    iteration itself stays fp64             */
    double  eig_lo_safety;       /* multiply the estimated lambda_min (0.9)  */
    double  eig_hi_safety;       /* multiply the estimated lambda_max (1.05) */
    double  eig_lo, eig_hi;      /* >0: use these bounds, skip the estimate  */
    double  drop_tol;            /* explicit Gc: drop |g_ij| < tol*max_j|g_ij| */
    int32_t factorization;       /* DNS_FACT_*                               */
    int32_t pad;
} dns_precond_opts;

typedef struct dns_solve_opts {
    int32_t method;              /* DNS_METHOD_*                             */
    int32_t restart;             /* GMRES cycle length (<= 64)               */
    int32_t maxiter;             /* total inner iterations                   */
    int32_t reorth;              /* 0: classical Gram-Schmidt once, 1: twice,
                                    2: once, folded into the next step's head
                                       kernel (norm by Pythagoras; one GPU) */
    double  rtol;                /* stop at ||r|| <= max(rtol*||b||, atol)   */
    double  atol;
    int32_t check_every;         /* host polls the device flag every k its   */
    int32_t use_graph;           /* replay hipGraph chunks instead of eager  */
} dns_solve_opts;

typedef struct dns_solve_stats {
    int32_t iters;               /* Krylov iterations performed              */
    int32_t status;              /* DNS_OK / DNS_NOT_CONVERGED / ...         */
    int32_t spmv_count;          /* K applies + F applies (preconditioner)   */
    int32_t restarts;
    double  bnorm;               /* ||[rhs_v; rhs_p]||_2                     */
    double  est_relres;          /* recurrence residual / ||b||              */
    double  true_relres;         /* ||b - K x|| / ||b|| recomputed at the end*/
    double  device_seconds;      /* HIP-event time of the solve on its stream*/
} dns_solve_stats;

/* ---- library ---------------------------------------------------------- */
int         dns_version(void);
const char *dns_status_string(int status);
const char *dns_last_error(void);
int         dns_device_count(int *count);
int         dns_device_name(int device, char *buf, size_t buflen);
/* block until all work queued on `device` has finished */
int         dns_device_synchronize(int device);

/* ---- saddle-point systems ---------------------------------------------
 * Replaces, per call site of `lau.solve_sadpnt_smw(amat=, jmat=, jmatT=,
 * rhsv=, rhsp=, krylov=, krpslvprms=, ...)`:
 *   stokes_navier_utils.py:401,458,497 (steady), :894,904 (initial Stokes),
 *   :1505-1512 (per time step), :1622,1629 (get_pfromv);
 *   time_int_utils.py:402,408,466 (Heun start), :605 (return_alu);
 * and `scipy.sparse.linalg.factorized(K)` + `coeffmatlu(rhs)` at
 *   time_int_utils.py:89-91,134 and :304-306,348.
 * `jt` may be NULL (the transpose of `j` is formed on the host, as
 * `jmatT=None -> jmat.T` at time_int_utils.py:605).
 */
int dns_saddle_create(int device, const dns_csr *f, const dns_csr *j,
                      const dns_csr *jt, dns_saddle **out);
void dns_saddle_destroy(dns_saddle *h);

/* same sparsity pattern, new values of F (Newton/Picard re-linearisation:
 * `solvmat = M + 0.5*dt*(A + N(v))`, stokes_navier_utils.py:1034,1484-1491) */
int dns_saddle_update_values(dns_saddle *h, const double *f_vals);

/* build / rebuild the block preconditioner  P = [[Fh, JT], [0, -Sh]] */
int dns_saddle_setup_precond(dns_saddle *h, const dns_precond_opts *opts);

/* out_vp = [v; p~] (NV+NP); x0 may be NULL (`krpslvprms['x0']`,
 * stokes_navier_utils.py:1493-1503); rhs_p may be NULL (zero,
 * stokes_navier_utils.py:1629-1632) */
int dns_saddle_solve(dns_saddle *h, const double *rhs_v, const double *rhs_p,
                     const double *x0, double *out_vp,
                     const dns_solve_opts *opts, dns_solve_stats *stats);

/* `ncols` right-hand sides in one call -- `lau.solve_sadpnt_smw` takes
 * `(NV, k)` blocks (`umat` / `vmat` feedback, stokes_navier_utils.py:1036-1042,
 * 1512; `apply_massinv`, tests/time_dep_nse_bigchannel.py:33): the blocks cross
 * the PCIe once, the solves run back to back on the resident system.
 * Column c of `rhs_v` at rhs_v + c NV, of `rhs_p` (may be NULL) at rhs_p + c NP,
 * of `out_vp` at out_vp + c (NV + NP); `x0`: `x0_cols` start vectors (0 none,
 * 1 shared, `ncols` one each); `stats` (may be NULL) holds `ncols` records.
 * A column that does not converge is reported in its record, like the single
 * solve; the residual histories per column: dns_saddle_residual_history_col */
int dns_saddle_solve_multi(dns_saddle *h, int32_t ncols, const double *rhs_v,
                           const double *rhs_p, const double *x0,
                           int32_t x0_cols, double *out_vp,
                           const dns_solve_opts *opts, dns_solve_stats *stats);
int dns_saddle_residual_history_col(dns_saddle *h, int32_t col, double *out,
                                    int32_t cap, int32_t *count);

/* residual history of the last solve (`krpslvprms['convstatsl']`,
 * tests/time_dep_nse_krylov.py:47); returns the number of entries written */
int dns_saddle_residual_history(dns_saddle *h, double *out, int32_t cap,
                                int32_t *count);

/* y = K x for the assembled K = [[F, JT],[J, 0]] (parity / residual checks) */
int dns_saddle_apply(dns_saddle *h, const double *x, double *y);
/* z = P^-1 r (parity checks of the preconditioner) */
int dns_saddle_apply_precond(dns_saddle *h, const double *r, double *z);
/* profiling aid: replay a hipGraph chain of `chain` identical launches of one
 * kernel of the GMRES cycle on the handle's resident data (which: 0 head,
 * 1 Fh^-1 part, 2 K apply + dots, 3 Gram-Schmidt update, 4 residual+norms,
 * 5 tail, 6 basis combine, 7 Schur block) and report microseconds per launch */
int dns_saddle_probe(dns_saddle *h, int32_t which, int32_t chain,
                     int32_t reps, double *us_per_launch);
/* eigenvalue bounds used by the Chebyshev iteration */
int dns_saddle_cheb_bounds(dns_saddle *h, double *lo, double *hi);
/* sizes of what the preconditioner keeps resident (for the published
 * per-step byte counts of bench.py): out[0..] = nnz(K), nnz(Gc) (0: recurrence
 * form), nnz(J Fh^-1) (0: triangular form), NP, fp32_store, cheb_degree,
 * schur kind, L = multigrid levels, smoothing steps, then per level l < L: n_l,
 * nnz(S_l), nnz(P_l) (0 on the coarsest).  `count` = entries available; at most `cap`
 * are written */
int dns_saddle_precond_info(dns_saddle *h, int32_t cap, int64_t *out,
                            int32_t *count);
void dns_default_precond_opts(dns_precond_opts *o);
void dns_default_solve_opts(dns_solve_opts *o);

/* ---- row-partitioned solve over several GPUs ------------------------------
 * One process per GPU.  Every rank creates the saddle system, attaches a
 * communicator and sets up the preconditioner; from then on it keeps in HBM
 * only ITS row block of every operator (K, the explicit Fh^-1, J Fh^-1) and
 * computes only those rows.  Per Arnoldi step: one halo exchange of the new
 * basis vector's velocity part (each neighbour gets exactly the entries its
 * rows reference: index lists from the column footprint), one all-gather of
 * the pressure-sized Schur input, one halo exchange of the preconditioned
 * velocity in front of the K apply, ONE all-reduce of the step's j+2 dot
 * products.  Production backend: RCCL over xGMI (grouped ncclSend/ncclRecv +
 * ncclAllReduce).  Test backend: host callbacks (torch.distributed/gloo, so
 * that two ranks can share one GPU).  Needs the explicit Fh^-1.  The
 * reference has no counterpart.
 */
typedef struct dns_comm dns_comm;
#define DNS_UNIQUE_ID_BYTES 128
/* in-place sum over ranks of `count` doubles at DEVICE pointer `dev` */
typedef int (*dns_allreduce_cb)(void *ctx, double *dev, int32_t count);
/* in-place: rank r owns dev[starts[r] .. starts[r+1]); afterwards every rank
 * holds every block; `starts` has nranks+1 entries */
typedef int (*dns_allgatherv_cb)(void *ctx, double *dev, const int32_t *starts,
                                 int32_t nranks);
/* halo exchange: send `sendcounts[q]` doubles at DEVICE `send + senddispls[q]`
 * to rank q, receive `recvcounts[q]` at DEVICE `recv + recvdispls[q]` */
typedef int (*dns_alltoallv_cb)(void *ctx, const double *send_dev,
                                const int32_t *sendcounts,
                                const int32_t *senddispls, double *recv_dev,
                                const int32_t *recvcounts,
                                const int32_t *recvdispls, int32_t nranks);
int dns_comm_unique_id(char *out_128_bytes);          /* call on rank 0     */
int dns_comm_create_rccl(int device, int32_t nranks, int32_t rank,
                         const char *unique_id_128_bytes, dns_comm **out);
int dns_comm_create_callbacks(int device, int32_t nranks, int32_t rank,
                              dns_allreduce_cb allreduce,
                              dns_allgatherv_cb allgatherv, void *ctx,
                              dns_comm **out);
/* the callback backend's halo exchange (RCCL: grouped ncclSend/ncclRecv) */
int dns_comm_set_alltoallv_cb(dns_comm *c, dns_alltoallv_cb alltoallv);
void dns_comm_destroy(dns_comm *c);
int dns_comm_stats(dns_comm *c, int64_t *n_allreduce, int64_t *n_allgather);
/* calls and bytes this rank sent: out[0..4] = all-reduce calls, all-gather-v
 * calls, halo exchanges, halo bytes, all-gather bytes */
int dns_comm_stats2(dns_comm *c, int64_t *out5);
/* Device time per collective.  While switched on, every collective that is
 * issued as a plain launch (not inside a captured graph) is bracketed by an
 * event pair on the launch stream; `dns_comm_timing` waits for the pairs and
 * returns the summed milliseconds and the number of timed calls since the
 * switch, in the order all-reduce, all-gather-v, halo exchange (the
 * ncclSend/Recv group alone, without its pack / unpack kernels).  The time
 * between the events includes the wait for the slowest peer. */
int dns_comm_set_timing(dns_comm *c, int on);
int dns_comm_timing(dns_comm *c, double *ms3, int64_t *calls3);
/* First-contact self-test, ONE primitive per call (so that a caller can say
 * which one did not come back): `which` 0 = all-reduce of `count` doubles, 1 =
 * one grouped ncclSend/ncclRecv exchange round the ring (the halo exchange's
 * call pattern), 2 = all-gather of unequal blocks (staged ncclAllGather), 3 =
 * all-gather of equal blocks (in-place ncclAllGather); `graph` 0 = plain
 * launches, 1 = captured in a hipGraph and replayed.  One call is checked
 * entry by entry (*ok), then `reps` calls are timed by an event pair on the
 * launch stream (*us_per_call).  Collective.  No reference counterpart. */
int dns_comm_selftest(dns_comm *c, int32_t which, int32_t graph, int32_t count,
                      int32_t reps, int32_t *ok, double *us_per_call);
/* out[0..2] = all-gathers issued as in-place ncclAllGather, staged
 * ncclAllGather (unequal blocks), group of ncclBroadcasts (fallback) */
int dns_comm_gather_forms(dns_comm *c, int64_t *out3);
/* 0 = in-place where the blocks are equal, staged otherwise (default); 1 = the
 * group of broadcasts; 2 = always staged (tests: one rank exercises the pack /
 * unpack path).  Environment DNS_COMM_ALLGATHER=bcast|staged sets it too. */
int dns_comm_set_gather_form(dns_comm *c, int32_t form);
/* The halo plan of a row partition, host only (no GPU needed): for the CSR
 * pattern `a` (n rows, columns < ncols_part partitioned by `col_starts`
 * [nranks+1]; columns >= ncols_part are ignored) and the rows [row0, row1) of
 * rank `rank`, the sorted distinct columns that rank references in every
 * other rank's range.  `counts` [nranks] receives the list lengths, `lists`
 * (capacity `cap`) the concatenated lists; returns the total in `*total`. */
int dns_halo_lists(const dns_csr *a, int32_t row0, int32_t row1,
                   int32_t nranks, int32_t rank, const int32_t *col_starts,
                   int32_t ncols_part, int32_t *counts, int32_t *lists,
                   int64_t cap, int64_t *total);
/* bytes of HBM the handle's matrices occupy on this rank (K, Fh^-1, J Fh^-1,
 * Schur block, F/J/JT copies): shrinks with the number of ranks */
int dns_saddle_device_bytes(dns_saddle *h, int64_t *matrix_bytes);
/* bytes of HOST memory: `kept` = the matrix copies the handle keeps (F, J, JT
 * -- whole, or the own rows of a handle created from rows --, prolongations,
 * level operators of a partitioned multigrid); `setup` = the matrices the last
 * partitioned explicit set-up had alive at its end (0 otherwise) */
int dns_saddle_host_bytes(dns_saddle *h, int64_t *kept, int64_t *setup);
/* attach before dns_saddle_setup_precond; NULL detaches */
int dns_saddle_set_comm(dns_saddle *h, dns_comm *c);
/* Rank-local construction of a row-partitioned handle: rank r of `comm` hands
 * over ITS rows of K = [[F, JT], [J, 0]] only -- `f_rows` = rows [v0, v1) of F
 * (v1 - v0 rows, `nv` columns, GLOBAL column indices), `jt_rows` = the same rows
 * of J^T (`np` columns), `j_rows` = rows [p0, p1) of J (`nv` columns), with
 * [v0, v1) = dns_partition_range(nv, ...) and [p0, p1) =
 * dns_partition_range(np, ...).  No rank ever holds a whole matrix, on the host
 * or in HBM: the rows of F and J^T a rank's part of the polynomial
 * preconditioner reaches beyond its own are fetched from their owners during
 * dns_saddle_setup_precond (degree - 1 rings of the pattern of F) and dropped
 * again; the spectral bounds come from power iterations whose product is formed
 * by rows.  The preconditioner, hence every iterate, equals bit for bit the one
 * of a handle created from whole matrices with the same communicator attached.
 * Collective (every rank of `comm` calls it).  Restrictions: explicit Fh^-1
 * (degree 2..12), dense or multigrid Schur block (its hierarchy is still built
 * from the all-gathered Schur complement); F close to symmetric (the
 * convection-dominated set-up of dns_saddle_setup_precond needs whole
 * matrices); dns_saddle_update_values takes the values of the own rows;
 * the communicator cannot be exchanged.  The reference has no counterpart (one
 * process: `lau.solve_sadpnt_smw(amat=, jmat=)`, stokes_navier_utils.py:1512);
 * this is the entry a distributed assembler binds. */
int dns_saddle_create_rows(int device, dns_comm *comm, int32_t nv, int32_t np,
                           const dns_csr *f_rows, const dns_csr *jt_rows,
                           const dns_csr *j_rows, dns_saddle **out);
/* the block partition used for n rows: [start, end) of `rank` (chunks of
 * ceil(n / nranks) rows rounded up to an even number: the two velocity dofs of
 * a node stay on one rank) */
int dns_partition_range(int32_t n, int32_t nranks, int32_t rank,
                        int32_t *start, int32_t *end);
/* raw device <-> host copies for the callback backend */
int dns_device_read(int device, const void *dev, void *host, size_t bytes);
int dns_device_write(int device, void *dev, const void *host, size_t bytes);

/* ---- device-resident IMEX time loop -------------------------------------
 * Replaces the inner loops of `time_int_utils.cnab` (tiu:104-143) and
 * `time_int_utils.sbdftwo` (tiu:320-353): the state (v, p, history) and the
 * constant system stay in HBM; per step the host supplies only what the
 * reference obtains from callbacks.
 *
 *   rhs_v = R1 (a_c v_c + a_p v_p) + cn_c*nfc_c + cn_o*nfc_o + gvec
 *   solve K [v_n; p~] = [rhs_v; rhs_p];   p_n = pscale * p~
 *
 *   CNAB : R1 = M - dt/2 A, a_c = 1,   a_p = 0,    cn_c = 3dt/2, cn_o = -dt/2
 *   SBDF2: R1 = M,          a_c = 4/3, a_p = -1/3, cn_c = 4dt/3, cn_o = -2dt/3
 */
typedef struct dns_imex_coeffs {
    double a_c, a_p;             /* weights of current / previous velocity   */
    double cn_c, cn_o;           /* weights of current / old convection      */
    double pscale;               /* p = pscale * p~  (scalep/dt, tiu:137)    */
    int32_t extrapolate_x0;      /* warm start: 0: x0 = x_c, 1: 2 x_c - x_p,
                                    2: 3 x_c - 3 x_p + x_pp (quadratic),
                                    3: 4 x_c - 6 x_p + 4 x_pp - x_ppp (cubic),
                                    4: 5, -10, 10, -5, 1 (quartic);
                                    13: cubic least-squares fit through the
                                    last five solutions (3.2, -2.8, -0.8, 2.2,
                                    -0.8: a third of the quartic's
                                    amplification of the solves' residuals) */
    int32_t carry_residual;      /* 1: the velocity residual b - K x of a step's
                                    (inexact) solve is added to the next
                                    step's right-hand side, so that the
                                    distance to the direct-solve trajectory
                                    does not grow with the number of steps
                                    (pipelined GMRES steps of dns_imex_run on
                                    one GPU below the streaming threshold;
                                    ignored elsewhere)                       */
} dns_imex_coeffs;

int dns_imex_create(dns_saddle *sys, const dns_csr *r1, dns_imex **out);
/* ... on a system created from rows (dns_saddle_create_rows): `r1_rows` = this
 * rank's rows of R1 -- rows dns_partition_range(NV, ...), NV columns, global
 * column indices; the halo lists of the stepper are exchanged instead of being
 * computed from a replicated pattern.  Collective at the first step. */
int dns_imex_create_rows(dns_saddle *sys, const dns_csr *r1_rows,
                         dns_imex **out);
void dns_imex_destroy(dns_imex *st);
/* set the state: current / previous velocity (v_p may be NULL), current p~
 * (may be NULL = 0; only seeds the warm start), the two convection history
 * vectors (NULL = 0) */
int dns_imex_set_state(dns_imex *st, const double *v_c, const double *v_p,
                       const double *ptilde_c, const double *nfc_c,
                       const double *nfc_o);
/* constant (or updated) parts of the right-hand side; NULL keeps the old */
int dns_imex_set_rhs(dns_imex *st, const double *gvec, const double *rhs_p);
/* Per-step right-hand sides known in advance -- what the reference's callbacks
 * `f_tdp(t)`, `g_tdp(t)`, `applybcs(getbcs(t))` return per step (tiu:114-127,
 * snu:1103-1126) when they depend on time only (time-dependent forcing,
 * prescribed moving-boundary data): row s of `gv` (nsteps x NV, may be NULL)
 * / `gp` (nsteps x NP, may be NULL) replaces gvec / rhs_p in the s-th step
 * after this call.  A step counter on the device selects the row, so
 * dns_imex_run replays its graphs through the whole table without the host.
 * Stepping past the last row fails with DNS_ERR_NOT_READY; dns_imex_set_rhs
 * returns to constant vectors. */
int dns_imex_set_rhs_table(dns_imex *st, int32_t nsteps, const double *gv,
                           const double *gp);
/* steps taken since the tables were uploaded / rows left (-1: no table) */
int dns_imex_table_position(dns_imex *st, int32_t *pos, int32_t *left);
/* one step; `nfc_new` (host, may be NULL) is the convection vector
 * f_vdp(v_c) evaluated by the caller at the current velocity -- it becomes
 * nfc_c, the old nfc_c becomes nfc_o (tiu:112-113).  NULL keeps both. */
int dns_imex_step(dns_imex *st, const double *nfc_new,
                  const dns_imex_coeffs *cf, const dns_solve_opts *opts,
                  dns_solve_stats *stats);
/* `nsteps` steps back to back without host callbacks (convection evaluated on
 * the device if an operator is attached, else its history stays frozen); HIP-
 * event time of the stepping loop on the handle's stream.  With GMRES and
 * `use_graph` the steps are pipelined: a fresh stepper first does up to four
 * synchronous steps (extrapolation history), then every graph the loop can ask
 * for is captured (six ring states x cycle lengths), then batches of steps are
 * replayed without host synchronisation; the ring, the predicted cycle length
 * and the graphs persist across calls, so a later call starts replaying at
 * once.  Returns DNS_NOT_CONVERGED (state advanced, outputs filled) if some
 * step ended at `maxiter`: see dns_imex_run_info. */
int dns_imex_run(dns_imex *st, int32_t nsteps, const dns_imex_coeffs *cf,
                 const dns_solve_opts *opts, dns_solve_stats *last_stats,
                 double *device_seconds, int64_t *total_iters);
/* record of the last dns_imex_run: steps that did not converge and the first
 * of them (index within the run, -1: none), steps that were repeated because
 * a batch mispredicted its cycle length, graphs captured inside the call */
int dns_imex_run_info(dns_imex *st, int32_t *unconverged, int32_t *first_bad,
                      int32_t *replayed, int32_t *captures);
/* diagnostics of the row-partitioned step (tests): out[0] = steps built
 * (launched or captured; graph replays are not counted), out[1] = of them the
 * steps whose one-step cycle evaluated the convection cells of the new
 * velocity in its tail, out[2] = the steps that left the cell kernel out
 * because the tail before had run it */
int dns_imex_step_counters(dns_imex *st, int64_t *out3);
/* six-node steps of the accepted batches of the last dns_imex_run by the kind
 * of their Krylov cycle: out[0] = lazy one-column cycles ("step6_lazy"),
 * out[1] = general cycles */
int dns_imex_run_cycles(dns_imex *st, int64_t *out2);
/* v (NV) and p = pscale*p~ (NP) of the current state */
int dns_imex_get_state(dns_imex *st, double *v, double *p);

/* TEST ONLY.  The front of ONE step: what `dns_imex_step` does before its
 * solve (the upload of `nfc_new` with its swap, the K x products of a carry
 * step; on a row-partitioned handle the stepper's own row blocks and halo
 * plan), then the plan for `cycle_len` (0: a synchronous solve; > 0: the cycle
 * length of a pipelined batch) and the launches that plan puts in front of the
 * first Krylov cycle -- by the member functions the step itself calls, without
 * the nodes of the attachments and without a solve -- then a synchronise.
 * `out` receives what the front READS, copied before it runs, and what it has
 * LEFT.  Every pointer of `out` may be NULL (n = NV + NP).  On a
 * row-partitioned handle the call is COLLECTIVE: every rank calls it, in the
 * same order with the same arguments (the current solution may be
 * all-gathered before the row blocks are cut); every vector is copied out in
 * full, valid on the rank's own rows and their halo.
 * DNS_ERR_BAD_ARGUMENT with an attachment (feedback, recorder, functionals,
 * statistics, quadratics, ensemble); DNS_ERR_NOT_READY with a pipelined batch
 * pending; nothing is touched then.
 * The stepper is CONSUMED: the convection slot, the carry buffers and the
 * work vector are those of a step that never finished.  dns_imex_step,
 * dns_imex_run and a second probe answer DNS_ERR_NOT_READY until
 * dns_imex_set_state starts over. */
typedef struct dns_imex_probe {
    /* --- read by the front */
    double *ring;          /* 5 n: cur, prev, pprev, p3, p4, raw [v; p~]       */
    double *nfc_in;        /* 2 NV: nfc_c, nfc_o as the front finds them       */
    double *g_in, *gp_in;  /* NV, NP: the rows of g / gp the counter selects   */
    double *b_prev;        /* n: the right-hand side of the step before        */
    double *kxs_in;        /* 4 n: K x of prev .. p4      (has_carry)          */
    double *rcarry_in;     /* NV: the carried residual    (has_carry)          */
    double *rc6_in;        /* 2 NV: current, previous     (has_six or dcarry)  */
    double *x0_other;      /* n: the warm start before    (has_six; dcarry:
                            * the copy the front before made, stale unless
                            * that step's plan had dtail)                      */
    /* --- left by the front */
    double *x0, *b;        /* n each                                           */
    double *nfc_out;       /* NV: nfc_c (written with a device convection)     */
    double *kx;            /* n: K x0                     (six-node form)      */
    double *r;             /* n: b - K x0                 (nparts > 0)         */
    double *partR, *partB; /* parts_cap each: raw partials (nparts > 0)        */
    double *kxs_cur;       /* n: K x_c                    (mode 2)             */
    double *rcarry_out;    /* NV: b_prev - K x_c          (mode 2)             */
    int32_t parts_cap;     /* in                                               */
    int32_t nsol, tab_row, has_carry, has_six;
    /* the plan: StepPlan::Form (0 Plain, 1 Six, 2 Fused, 3 DistFront, 4 Rows,
     * 5 StreamRhs, 6 StreamRows), the MODE of k_step_front, "the tail before
     * left the warm start", "residual carried"; the lanes-per-row
     * instantiations of K and R1; the partials; "R1 is held in the pair
     * format" (the streamed product then takes it) */
    int32_t form, mode, use_pre, carry, k_lpr, r1_lpr, nparts, r1_pair, pad;
    /* --- appended for the row-partitioned forms */
    double *r_in;          /* n: the solver's residual vector as the front
                            * finds it (read by no front: what it must leave
                            * untouched outside the own rows)                  */
    double *x0copy;        /* n: the copy of x0 left by the front (dtail)      */
    /* row0, len1, row2, len2 of this rank's rows of K (all zero when the
     * handle is not partitioned); the plan's "residuals of the one-step
     * solves carried", "lazy tail with the convection cells", "the tail
     * before left the cells"; the number of cells this rank evaluates */
    int32_t rowmap[4];
    int32_t dcarry, dtail, have_cells, nsel;
} dns_imex_probe;
int dns_imex_front_probe(dns_imex *st, const dns_imex_coeffs *cf,
                         const dns_solve_opts *opts, int32_t cycle_len,
                         const double *nfc_new, dns_imex_probe *out);
/* ---- observer feedback of the explicit loops ------------------------------
 * The reference's `dynamic_rhs` of a closed loop with a linear observer
 * (`get_heunab_lti`, tiu:148-196, composed as in snu:1243-1247), resident:
 *     y    = C v_c                          C: Ny x NV CSR (sensors)
 *     f    = ha hx + hb y + drift(t_c)      ha: hN x hN, hb: hN x Ny, row major
 *     hx_n = hx + 1.5 dt f - 0.5 dt f_last  (AB2)
 *     u_n  = hc hx_n                        hc: Nu x hN, row major
 *     g   += dt (c_n B u_n + c_c B u_c)     B: NV x Nu CSR (actuators)
 * evaluated by one kernel in front of every step (dns_imex_step and
 * dns_imex_run alike), so that closed-loop steps are replayed as graphs like
 * open-loop ones.  CNAB: c_n = c_c = 1/2; SBDF2: c_n = 2/3, c_c = 0.
 * Limits (DNS_ERR_BAD_ARGUMENT beyond them): hN <= 128, Ny <= 32, Nu <= 32,
 * nnz(C) <= 16384, one GPU (not on a row-partitioned stepper).  A call that
 * fails leaves the stepper as it was.  After this call the observer state is
 * zero and no table is set: dns_imex_set_feedback_table must follow. */
int dns_imex_set_feedback(dns_imex *st, const dns_csr *cmat, const dns_csr *bmat,
                          const double *ha, const double *hb, const double *hc,
                          int32_t hN, int32_t Ny, int32_t Nu, double c_n,
                          double c_c, double dt);
/* observer state of the current time: hx (hN), the last observer right-hand
 * side f_last (hN) and the current input u_c (Nu) -- the hand-over from a
 * start-up scheme on the host (Heun: `lasthx`, `lastrhs`, hc lasthx) */
int dns_imex_set_feedback_state(dns_imex *st, const double *hx,
                                const double *f_last, const double *u_c);
/* the same, read back (any pointer may be NULL) */
int dns_imex_get_feedback_state(dns_imex *st, double *hx, double *f_last,
                                double *u_c);
/* drift rows: row s of `drift` (nsteps x hN, NULL: no drift) enters the s-th
 * step after this call; `nsteps` is also the capacity of the logs.  Resets
 * the step counter like dns_imex_set_rhs_table (upload the tables of a slice
 * together); stepping past the last row fails with DNS_ERR_NOT_READY. */
int dns_imex_set_feedback_table(dns_imex *st, int32_t nsteps,
                                const double *drift);
/* rows [first, first + count) of the logs: y (count x Ny) = C v_c the s-th
 * step saw, u (count x Nu) = the input u_n it computed (either may be NULL) */
int dns_imex_get_feedback_log(dns_imex *st, int32_t first, int32_t count,
                              double *y, double *u);
/* back to open-loop steps */
int dns_imex_clear_feedback(dns_imex *st);
/* ---- boundary feedback: the observer drives controlled Dirichlet values ----
 * Behind dns_imex_set_feedback (whose `bmat` may be empty: no actuation
 * through the right-hand side): the same observer step, and
 *     b(s+1) = base + S u_n                  S: nc x Nu CSR, base: nc (NULL: 0)
 * written into the columns [col0, col0 + nc) of row s + 1 of the Dirichlet
 * table of the attached convection operator (dns_conv_set_dbc_table, which
 * needs nsteps + 1 rows: row 0 holds the values of the current state, the
 * other columns and rows are the host's).  The front convection of step s
 * reads row s, the convection of the new state row s + 1.
 * `ba`, `bm` (NV x Nu), `bj` (NP x Nu): what `applybcs` makes of the unit
 * controls S e_k (-A_bc, M_bc, -J_bc columns); all NULL: no boundary terms.
 * With them the rows the host tabulated for u = 0 get what is linear in u:
 *     geff  = g(s) + sum_{j = n, c, p} (wm[j] Bm + wa[j] Ba) u_j
 *                  + dt (c_n B u_n + c_c B u_c)
 *     gpeff = gp(s) + Bj u_n
 * `wm`, `wa`: three weights each for u_n, u_c, u_p (CNAB: wm = (-1, 1, 0),
 * wa = dt/2 (1, 1, 0); SBDF2: wm = (-1, 4/3, -1/3), wa = (2/3 dt, 0, 0)).
 * Limits as dns_imex_set_feedback; refused (DNS_ERR_BAD_ARGUMENT) on a
 * row-partitioned stepper, without a device convection operator, and for
 * widths that do not fit; a step refuses a table with fewer than nsteps + 1
 * rows, and functionals / quadratics beside it.  After this call the observer
 * state is zero and no table is set. */
int dns_imex_set_feedback_boundary(dns_imex *st, const dns_csr *smat,
                                   const double *base, int32_t col0,
                                   const dns_csr *ba, const dns_csr *bm,
                                   const dns_csr *bj, const double *wm,
                                   const double *wa);
/* the observer state with u_p (Nu), the input one time before u_c */
int dns_imex_set_feedback_state_bc(dns_imex *st, const double *hx,
                                   const double *f_last, const double *u_c,
                                   const double *u_p);
/* the same, read back (any pointer may be NULL) */
int dns_imex_get_feedback_state_bc(dns_imex *st, double *hx, double *f_last,
                                   double *u_c, double *u_p);
/* rows [first, first + count) of the controlled columns of the Dirichlet
 * table as they stand on the device (count x nc): row s + 1 is what step s
 * wrote */
int dns_imex_get_feedback_bcs(dns_imex *st, int32_t first, int32_t count,
                              double *bcs);
/* the right-hand sides the last step read: geff (NV), gpeff (NP); either may
 * be NULL; DNS_ERR_NOT_READY for one the step does not form */
int dns_imex_get_feedback_rhs(dns_imex *st, double *geff, double *gpeff);
/* ---- trajectory recorder of the explicit loops ----------------------------
 * While dns_imex_step / dns_imex_run step (and replay their graphs), one more
 * kernel per step writes down the trajectory on the device:
 *     y row r    = C v          C: Ny x NV CSR (`cmat`, NULL: no outputs)
 *     slot[r]    = [v; p]       `snap_slot` (nrows entries, NULL: no
 *                               snapshots): the slot (0 .. nslots-1) that keeps
 *                               the state of row r, -1: not kept
 * Row r holds what dns_imex_get_state would have returned after the (r+1)-th
 * step since the step counter was last reset (p = pscale*p~, the same bits).
 * `nrows` is a table length like the others: this call resets the step counter
 * like dns_imex_set_rhs_table (upload the tables of a slice together -- and
 * collect the rows before the next upload: any of those calls rewinds them),
 * stepping past the last row fails with DNS_ERR_NOT_READY.  Works with and
 * without observer feedback.  No limit on Ny, nnz(C), nrows or nslots other
 * than memory (nslots x (NV + NP, padded to 64) doubles).  One GPU: a
 * row-partitioned stepper refuses it.  A call that fails leaves the stepper
 * and an earlier recorder as they were. */
int dns_imex_set_recorder(dns_imex *st, const dns_csr *cmat, int32_t nrows,
                          const int32_t *snap_slot, int32_t nslots);
/* rows [first, first + count) of the outputs: y (count x Ny) */
int dns_imex_get_record_outputs(dns_imex *st, int32_t first, int32_t count,
                                double *y);
/* slots [first_slot, first_slot + count): v (count x NV) and p (count x NP),
 * either may be NULL */
int dns_imex_get_record_snapshots(dns_imex *st, int32_t first_slot,
                                  int32_t count, double *v, double *p);
/* recorder off (the step is what it was before dns_imex_set_recorder) */
int dns_imex_clear_recorder(dns_imex *st);
/* ---- force functionals of the explicit loops (drag, lift, dp, ...) --------
 * While dns_imex_step / dns_imex_run step (and replay their graphs), one more
 * kernel per step evaluates nF momentum-balance functionals of the state the
 * step has left, v = current velocity, v_prev = the one before, p = pressure
 * as dns_imex_get_state returns it:
 *     y_k = scale_k * ( ca_k . v + cm_k . (v - v_prev) / dt + cp_k . p
 *                       + sum_{c in cells_k} sum_{sl < 12} w_k[c][sl] N_loc(c; v)[sl]
 *                       + c0_k )
 * ca, cm: nF x NV, cp: nF x NP (host CSR, NULL: no such term).  The cells of
 * functional k are cell_idx[cell_ptr[k] .. cell_ptr[k+1]) (cells of the
 * attached convection operator, numbered as in the cell_vdofs it was created
 * with; NULL cell_ptr: none), cell_w holds twelve
 * weights per listed cell, slot = 2 * node + component; N_loc are the twelve
 * local sums of N(v)v on that cell with the operator's constant Dirichlet
 * values.  c0 / scale: nF values (NULL: 0 / 1).  With the rows of the test
 * vector phi in M, A, -J^T and phi's local values as weights, scale = -1
 * gives the consistent nodal force -phi^T (M dv/dt + A v + N(v)v - J^T p).
 * Row r of the log belongs to the (r+1)-th step after this call, which
 * resets the step counter like dns_imex_set_rhs_table (call it after that
 * one); stepping past the last row fails with DNS_ERR_NOT_READY.  Calling it
 * again re-arms it (buffers that are large enough are kept).
 * Limits (DNS_ERR_BAD_ARGUMENT beyond them): 1 <= nF <= 16; cell indices
 * below the operator's ncells; cells need an attached convection operator;
 * an operator with a per-step Dirichlet table (dns_conv_set_dbc_table: use
 * dns_imex_set_functionals_bc) and a row-partitioned stepper are refused.  Any nnz, any number of cells.
 * Works with and without observer feedback and the recorder. */
int dns_imex_set_functionals(dns_imex *st, int32_t nF, const dns_csr *ca,
                             const dns_csr *cm, const dns_csr *cp,
                             const double *c0, const double *scale,
                             const int32_t *cell_ptr, const int32_t *cell_idx,
                             const double *cell_w, double dt, int32_t nrows);
/* The same with Dirichlet values g that change from step to step (controlled
 * boundaries: a rotating body, a modulated inflow), ndbc of them in the order
 * of the convection operator's dbcinds:
 *     y_k = scale_k * ( ca_k . v + cm_k . (v - v_prev) / dt + cp_k . p
 *                       + cab_k . g + cmb_k . (g - g_prev) / dt
 *                       + sum_{c in cells_k} sum_{sl < 12} w_k[c][sl] N_loc(c; v, g)[sl]
 *                       + c0_k )
 * cab, cmb: nF x ndbc, the Dirichlet columns of phi^T A and phi^T M (host CSR,
 * NULL: no such term); c0 holds constants that are no boundary terms.
 * dbc_table: row-major (nrows + 1) x ndbc, row j the values of the state
 * BEFORE the j-th step after this call, row nrows those of the state after
 * the last one: log row r uses g = row r + 1, g_prev = row r.  It is a table
 * of the functionals' own; the operator's table (dns_conv_set_dbc_table) keeps
 * its meaning and length.  Further limits: ndbc >= 1, equal to the operator's
 * where cells are listed -- when it is set and when a step runs.  With
 * constant values the rows are those of dns_imex_set_functionals with
 * c0 + cab . g for c0. */
int dns_imex_set_functionals_bc(dns_imex *st, int32_t nF, const dns_csr *ca,
                                const dns_csr *cm, const dns_csr *cp,
                                const dns_csr *cab, const dns_csr *cmb,
                                const double *c0, const double *scale,
                                const int32_t *cell_ptr,
                                const int32_t *cell_idx, const double *cell_w,
                                double dt, int32_t nrows, int32_t ndbc,
                                const double *dbc_table);
/* dns_imex_set_functionals_bc without a table of their own: the Dirichlet
 * values are read from the table of the attached convection operator
 * (dns_conv_set_dbc_table) -- row j of it holds the values of the state before
 * the j-th step, the same convention -- which is what boundary feedback
 * (dns_imex_set_feedback_boundary) writes step by step: the functionals then
 * follow the values the observer makes on the device.  Needs, when it is set
 * and when a step runs (DNS_ERR_BAD_ARGUMENT otherwise, the message names what
 * is missing): an attached convection operator, its ndbc equal to `ndbc`, and
 * at least nrows + 1 rows in its table.  Beside boundary feedback only
 * functionals set this way are accepted. */
int dns_imex_set_functionals_live(dns_imex *st, int32_t nF, const dns_csr *ca,
                                  const dns_csr *cm, const dns_csr *cp,
                                  const dns_csr *cab, const dns_csr *cmb,
                                  const double *c0, const double *scale,
                                  const int32_t *cell_ptr,
                                  const int32_t *cell_idx,
                                  const double *cell_w, double dt,
                                  int32_t nrows, int32_t ndbc);
/* rows [first, first + count) of the log: out (count x nF) */
int dns_imex_get_functionals(dns_imex *st, int32_t first, int32_t count,
                             double *out);
/* functionals off (the step is what it was before) */
int dns_imex_clear_functionals(dns_imex *st);
/* Flow statistics (time averages, variances, Reynolds stresses; phase
 * averages and batch means by bins) as running sums on the device: the next
 * nrows steps (dns_imex_step and dns_imex_run alike) add the state they leave,
 * x_r = [v; pscale * p~] of row r -- what dns_imex_get_state returns after the
 * (r+1)-th step after this call --, to the sums of bin b = bin[r] (-1: the
 * step is skipped; nbins in 1..256):
 *     N_b += 1,  S1_b[i] += x_r[i],  S2_b[i] += x_r[i]^2     (i < NV + NP),
 *     SX_b[q] += x_r[pair_i[q]] * x_r[pair_j[q]]             (q < npairs)
 * with index pairs into [0, NV + NP) (npairs 0: none).  One kernel per step,
 * no atomics, the rows of a bin in step order: the same bits however the steps
 * are split into calls; S1 is plain additions.  A row is added once, whoever
 * launches for it a second time, and a batch dns_imex_run restores and repeats
 * adds to the sums it started from.  The sums are kept across calls with the
 * same nbins and pairs and reset == 0 (the slices of a time loop set a bin
 * table each and go on summing), zeroed otherwise.  Every check comes first: a
 * refused call leaves the statistics that were there.  Resets the step counter
 * like dns_imex_set_rhs_table.  Not on a row-partitioned stepper. */
int dns_imex_set_stats(dns_imex *st, int32_t nrows, const int32_t *bin,
                       int32_t nbins, int32_t npairs, const int32_t *pair_i,
                       const int32_t *pair_j, int32_t reset);
/* bins [first_bin, first_bin + count): counts (count), s1 and s2 (count x
 * (NV + NP), unpadded), sx (count x npairs); NULL outputs are skipped */
int dns_imex_get_stats(dns_imex *st, int32_t first_bin, int32_t count,
                       double *counts, double *s1, double *s2, double *sx);
/* statistics off (the step is what it was before) */
int dns_imex_clear_stats(dns_imex *st);
/* Quadratic functionals of the velocity (the energy budget: kinetic energy
 * 1/2 u^T M u, dissipation rate u^T A u, the rate u^T M du/dt, the M-norm of
 * du/dt) in a log on the device: while dns_imex_step / dns_imex_run step (and
 * replay their graphs), one more kernel per step evaluates nQ forms over nM
 * sparse matrices Q_0 .. Q_{nM-1} of the state the step has left.  With v =
 * current velocity, w = v - v_prev (the one before) and the operands a_0 = v,
 * a_1 = w:
 *     y_k = scale_k * ( dt^-(l_k + r_k) * a_{l_k}^T Q_{m_k} a_{r_k}
 *                       + qa_k . v + (qw_k . w) / dt + c0_k )
 * mats: nM host CSR matrices, each NV x NV, general (not assumed symmetric);
 * mat / lop / rop: nQ entries each, m_k in [0, nM), l_k and r_k 0 or 1; qa,
 * qw: nQ x NV (host CSR, NULL: no such term); c0 / scale: nQ values (NULL: 0 /
 * 1).  The sparse rows and c0 carry constant Dirichlet values g: for u = E v +
 * g, u^T Q u = v^T Q_ii v + (g^T (Q_bi + Q_ib^T)) v + g^T Q_bb g.  Forms that
 * share a matrix share one pass over it.
 * Row r of the log belongs to the (r+1)-th step after this call, which resets
 * the step counter like dns_imex_set_rhs_table (call it after that one);
 * stepping past the last row fails with DNS_ERR_NOT_READY.  The log is nrows x
 * G x nQ doubles, G the workgroups of the kernel (one per 16 rows of the
 * matrices, at most 256; max_grid > 0 caps it lower, 0: the default) -- the
 * getter sums G in index order, nothing is added atomically: the same bits
 * launched or replayed.  A batch dns_imex_run restores and repeats overwrites
 * its own rows.  Calling it again re-arms it: buffers that are large enough
 * are kept, and the same matrices are neither uploaded again nor change what a
 * captured step graph is keyed by -- "the same" means as many matrices as the
 * device holds, each equal to the one held entry by entry (row pointers,
 * columns and the bytes of the values; the library keeps a host copy to
 * compare with: 12 bytes per non-zero and 4 per row of host memory for as
 * long as the forms are set, and one pass over it per call).  Every check
 * comes first: a call refused for its arguments or for the stepper's state
 * leaves the forms that were there; a failed allocation or upload behind the
 * checks (DNS_ERR_HIP) leaves the stepper without quadratics.
 * Limits (DNS_ERR_BAD_ARGUMENT beyond them): 1 <= nM <= 4, 1 <= nQ <= 8,
 * nrows >= 1, a log below 2^31 entries; column indices inside [0, NV); any
 * number of non-zeros.  A row-partitioned stepper and a convection operator
 * with a per-step Dirichlet table (dns_conv_set_dbc_table: moving boundary
 * values are not part of the constants) are refused, here and by the step.
 * Works with and without the other attachments. */
int dns_imex_set_quadratics(dns_imex *st, int32_t nM, const dns_csr *mats,
                            int32_t nQ, const int32_t *mat, const int32_t *lop,
                            const int32_t *rop, const dns_csr *qa,
                            const dns_csr *qw, const double *c0,
                            const double *scale, double dt, int32_t nrows,
                            int32_t max_grid);
/* The same on the full space, with Dirichlet values g that change from step to
 * step, ndbc of them in the order of the convection operator's dbcinds: every
 * matrix is (NV + ndbc) x (NV + ndbc) in the order [inner dofs; Dirichlet
 * dofs], qa and qw are nQ x (NV + ndbc), and the operands are a_0 = u = [v; g]
 * and a_1 = d = [v - v_prev; g - g_prev]:
 *     y_k = scale_k * ( dt^-(l_k + r_k) * a_{l_k}^T Q_{m_k} a_{r_k}
 *                       + qa_k . u + (qw_k . d) / dt + c0_k )
 * Nothing of g is folded into qa, qw or c0.  dbc_table: row-major (nrows + 1) x
 * ndbc, row j the values of the state BEFORE the j-th step after this call,
 * row nrows those of the state after the last one: log row r uses g = row
 * r + 1, g_prev = row r (the convention of dns_imex_set_functionals_bc; a table
 * of the quadratics' own).  Further limits: ndbc >= 1, equal to the ndbc of an
 * attached convection operator -- when it is set and when a step runs.  The
 * same matrices are kept on the device as with dns_imex_set_quadratics. */
int dns_imex_set_quadratics_bc(dns_imex *st, int32_t nM, const dns_csr *mats,
                               int32_t nQ, const int32_t *mat,
                               const int32_t *lop, const int32_t *rop,
                               const dns_csr *qa, const dns_csr *qw,
                               const double *c0, const double *scale,
                               double dt, int32_t nrows, int32_t max_grid,
                               int32_t ndbc, const double *dbc_table);
/* dns_imex_set_quadratics_bc without a table of their own: the values are read
 * from the table of the attached convection operator, as with
 * dns_imex_set_functionals_live, with the same three requirements. */
int dns_imex_set_quadratics_live(dns_imex *st, int32_t nM, const dns_csr *mats,
                                 int32_t nQ, const int32_t *mat,
                                 const int32_t *lop, const int32_t *rop,
                                 const dns_csr *qa, const dns_csr *qw,
                                 const double *c0, const double *scale,
                                 double dt, int32_t nrows, int32_t max_grid,
                                 int32_t ndbc);
/* rows [first, first + count) of the log: out (count x nQ) */
int dns_imex_get_quadratics(dns_imex *st, int32_t first, int32_t count,
                            double *out);
/* G: the workgroups the log is laid out for (nrows x G x nQ doubles) */
int dns_imex_quadratics_grid(dns_imex *st, int32_t *grid);
/* quadratics off (the step is what it was before) */
int dns_imex_clear_quadratics(dns_imex *st);
/* Snapshot ensemble for a proper orthogonal decomposition (method of
 * snapshots) on the device: the stepper owns a buffer E of nslots slots, NV
 * doubles each (ldv = NV rounded up to 64 apart; velocities only), and the next
 * nrows steps (dns_imex_step and dns_imex_run alike) copy the velocity they
 * leave, v_r of row r -- what dns_imex_get_state returns after the (r+1)-th
 * step after this call, bit for bit --, into slot slot[r] (-1: the step is not
 * kept; slots in [0, nslots)).  One kernel per step; a row copied twice, or by
 * a batch dns_imex_run restores and repeats, has the same bits.  E is kept
 * across calls with the same nslots and reset == 0 (the slices of a time loop
 * set a slot table each and go on filling), reallocated and zeroed otherwise.
 * Every check comes first: a refused call leaves the ensemble that was there.
 * Resets the step counter like dns_imex_set_rhs_table.  Not on a
 * row-partitioned stepper.  Works with and without the other attachments. */
int dns_imex_set_ensemble(dns_imex *st, int32_t nrows, const int32_t *slot,
                          int32_t nslots, int32_t reset);
/* slots [first_slot, first_slot + count): v (count x NV, unpadded) */
int dns_imex_get_ensemble(dns_imex *st, int32_t first_slot, int32_t count,
                          double *v);
/* g (m x m, host) = E W E^T of the first m slots; w: symmetric NV x NV host
 * CSR (the mass matrix; the same matrix handed over again is not uploaded
 * again), NULL: the identity.  Plain launches behind the loop: Y = E W for 16
 * snapshots at a time, 16 x 16 tiles on the fp64 matrix cores over chunks of
 * 1024 entries, their partials added in chunk order.  No atomics: the same
 * bits in every run, on every device; g is exactly symmetric.  Extra device
 * memory: 16 x ldv + ceil(m / 16) x ceil(NV / 1024) x 256 doubles. */
int dns_imex_ensemble_gram(dns_imex *st, const dns_csr *w, int32_t m,
                           double *g);
/* out (r x NV, host) = coef (r x m, host) times the first m slots; per entry
 * acc = fma(coef[q, s], E[s, k], acc) for s = 0 .. m - 1: a fixed order */
int dns_imex_ensemble_combine(dns_imex *st, int32_t m, int32_t r,
                              const double *coef, double *out);
/* ensemble off and freed (the step is what it was before) */
int dns_imex_clear_ensemble(dns_imex *st);
/* ||v||_2 of the current velocity (blow-up guard, tiu:94-103) */
int dns_imex_vnorm(dns_imex *st, double *out);

/* ---- convection on the device --------------------------
 * N(u)u = inner(grad(u)*u, v)*dx for P2 velocities on triangles: replaces the
 * host callback `f_vdp` = `get_v_conv_conts(semi_explicit=True)` ->
 * `dolfin_to_sparrays.get_convvec` (stokes_navier_utils.py:1136-1140,103-107;
 * dolfin_to_sparrays.py:427-472) including its `append_bcs_vec`
 * (dolfin_to_sparrays.py:49-64).  Mesh data as the caller's FE library has it:
 *   cell_vdofs[12*c + 2*a + i] : FULL-space velocity dof of local node a,
 *        component i; local nodes 0..2 = vertices, 3..5 = midpoints of the
 *        edges opposite to vertex 0, 1, 2
 *   glam[6*c + 2*k + d]  : d-th component of grad(lambda_k) on cell c
 *   area[c]; invinds (inner dofs, order of the condensed vectors);
 *   dbcinds / dbcvals (Dirichlet dofs and values)
 */
typedef struct dns_conv dns_conv;
int dns_conv_create_p2(int device, int32_t ncells, const int32_t *cell_vdofs,
                       const double *glam, const double *area, int32_t vdim,
                       int32_t nv_inner, const int32_t *invinds, int32_t ndbc,
                       const int32_t *dbcinds, const double *dbcvals,
                       dns_conv **out);
void dns_conv_destroy(dns_conv *cv);
int dns_conv_set_dbcvals(dns_conv *cv, const double *dbcvals);
/* Dirichlet values that change from step to step (`append_bcs_vec` with
 * controlled boundary values, snu:1003-1006,1152-1157): `nrows` value sets
 * (nrows x ndbc).  Attached to an IMEX stepper, row s is used by the s-th step
 * after the stepper's tables were (re)set (the values at the step's CURRENT
 * time, where N(v_c)v_c is evaluated); in the trapezoidal sweeps the row is the
 * trajectory slot.  dns_conv_set_dbcvals returns to one constant set. */
int dns_conv_set_dbc_table(dns_conv *cv, int32_t nrows, const double *dbcvals);
/* the row the host-driven entry points (dns_conv_apply / _assemble) use */
int dns_conv_set_dbc_row(dns_conv *cv, int32_t row);
/* out = scale * N(u)u restricted to the inner dofs (host in/out; parity) */
int dns_conv_apply(dns_conv *cv, const double *v_inner, double scale,
                   double *out);
/* Linearised convection about a base flow V = [v_inner; dbcvals] (host
 * pointers, expanded into the cells and uploaded once).  From here on every
 * element launch of the operator -- dns_conv_apply, an attached CNAB / SBDF2
 * stepper -- evaluates, for the perturbation w it is handed,
 *   adjoint == 0:  L(V) w = int phi . ((w . grad) V + (V . grad) w)
 *   adjoint != 0:  the sum of the cell transposes (N1(V) + N2(V))^T_cell w_cell
 * instead of N(w)w, in the same cell-value layout.  The perturbation's own
 * Dirichlet values stay the operator's (dns_conv_set_dbcvals / _set_dbc_table);
 * the adjoint takes zero values and no table (then the sum is (L_II)^T w_I) and
 * refuses anything else.  A linearised operator is refused by
 * dns_conv_assemble*, dns_conv_project_tensor, the trapezoidal stepper, a
 * row-partitioned IMEX stepper and functionals with cells.  This base flow is
 * constant in time (dns_conv_set_base_trajectory: one that is not); the adjoint is the continuous one, stepped like any run */
#define DNS_CONV_NONLINEAR 0
#define DNS_CONV_FORWARD 1
#define DNS_CONV_ADJOINT 2
int dns_conv_set_base_flow(dns_conv *cv, const double *v_inner,
                           const double *dbcvals, int32_t adjoint);
int dns_conv_clear_base_flow(dns_conv *cv);
int dns_conv_get_mode(const dns_conv *cv, int32_t *mode);
/* Linearised convection about a TIME-VARYING base flow: a trajectory of nrows
 * base flows resident on the device -- the inner velocities (row r of v_rows,
 * ld_host >= nv_inner doubles apart on the host; on the device ldv = nv_inner
 * rounded up to 64 apart, the slot layout of the snapshot ensemble) and the
 * base flow's Dirichlet values, dbc_nrows == 1: one set for every row, or
 * dbc_nrows == nrows: row-major nrows x ndbc.  One upload; V is gathered
 * through the cell map as the perturbation is.  Modes, the perturbation's own
 * Dirichlet values and every refusal are those of dns_conv_set_base_flow.
 * Which row an element launch evaluates about (zero-order hold; the _lerp
 * forms below interpolate between two rows):
 *   dns_conv_set_base_rows  a per-step index table of n entries, each in
 *                           0..nrows-1 (anything else is refused by name before
 *                           anything is uploaded): the s-th step of the
 *                           attached CNAB / SBDF2 stepper after the call (its
 *                           step counter goes back to 0 as after any of its
 *                           own table setters) evaluates about row
 *                           rows[min(s, n - 1)].  Descending: an adjoint run
 *                           backwards over a stored forward run; repeated
 *                           entries: a trajectory stored every k-th step.
 *                           Outside a stepper (dns_conv_apply) row rows[0]
 *   dns_conv_set_base_row   one row the host names, for dns_conv_apply and for
 *                           the steps alike; it takes the index table off
 * Row 0 and no table until one of them is called.  dns_conv_set_base_flow and
 * dns_conv_clear_base_flow release the trajectory; dns_conv_get_base_info:
 * nrows (0: a constant base flow or none) and the length of the index table */
int dns_conv_set_base_trajectory(dns_conv *cv, int32_t nrows,
                                 const double *v_rows, int32_t ld_host,
                                 int32_t dbc_nrows, const double *dbc_vals,
                                 int32_t adjoint);
int dns_conv_set_base_rows(dns_conv *cv, int32_t n, const int32_t *rows);
int dns_conv_set_base_row(dns_conv *cv, int32_t row);
int dns_conv_get_base_info(const dns_conv *cv, int32_t *nrows, int32_t *nbrow);
/* Linear interpolation between the stored rows: with a weight th beside a row
 * r the element launches evaluate, for every dof they gather (inner values and
 * the base flow's Dirichlet values alike), about
 *   V = V_r + th * (V_p - V_r),   p = min(r + 1, nrows - 1),
 * three separately rounded fp64 operations (subtract, multiply, add; no
 * contraction) -- NumPy's V0 + th*(V1 - V0) bit for bit.
 *   dns_conv_set_base_rows_lerp  the index table of dns_conv_set_base_rows and
 *                           n weights beside it, read through the same clamped
 *                           step counter (rows[min(s, n - 1)] with
 *                           weights[min(s, n - 1)]); outside a stepper rows[0]
 *                           with weights[0].  The attached stepper counts from
 *                           0 again as after dns_conv_set_base_rows
 *   dns_conv_set_base_row_lerp   one row and one weight the host names; takes
 *                           the index table off
 * Refused by name before anything is uploaded, the operator left as it was: a
 * weight that is not finite or outside [0, 1) (th = 1 is row r + 1 with weight
 * 0), a non-zero weight on the last row, weights without a trajectory, a null
 * table.  All-zero weights give the bits of the zero-order hold.
 * dns_conv_set_base_rows / _set_base_row keep their meaning and take the
 * weights off; dns_conv_get_base_lerp: 1 while weights are armed, else 0 */
int dns_conv_set_base_rows_lerp(dns_conv *cv, int32_t n, const int32_t *rows,
                                const double *weights);
int dns_conv_set_base_row_lerp(dns_conv *cv, int32_t row, double weight);
int dns_conv_get_base_lerp(const dns_conv *cv, int32_t *lerp);
/* ... adopted from the snapshot ensemble of a stepper (dns_imex_set_ensemble):
 * slots first .. first + count - 1 become rows 0 .. count - 1, copied device to
 * device on the stepper's stream; only dbc_vals (as above, dbc_nrows 1 or
 * count) cross the bus.  Refused by name: no ensemble, slots out of range, the
 * operator on another device, another number of inner dofs */
int dns_imex_ensemble_to_base(dns_imex *st, int32_t first, int32_t count,
                              dns_conv *cv, int32_t dbc_nrows,
                              const double *dbc_vals, int32_t adjoint);
/* TEST ONLY: the cell values [12][ncells] (the operator's internal cell order)
 * the element launch leaves for v_inner in the current mode; nsel >= 0: only
 * the internal cells sel[0..nsel) are evaluated, every other entry is `fill`.
 * cell_pos (ncells, or NULL): the caller's cell -> internal cell */
int dns_conv_cells_probe(dns_conv *cv, const double *v_inner,
                         const int32_t *sel, int32_t nsel, double fill,
                         double *cells_out, int32_t *cell_pos);
/* the cubic convection tensor of a Galerkin projection (reduced-order models),
 *   out[i, j, k] = sum_cells sum_q w_q |cell| phi_i(x_q) . (u_j . grad) u_k (x_q),
 * nt x nb x nb, row-major, j the convecting and k the convected field, by the
 * 7-point rule of dns_conv_apply.  basis is nb x ld on the host (ld even, >=
 * the inner dofs; row b holds u_b on the inner dofs), dbc_rows nb x ndbc the
 * Dirichlet values row b carries (NULL: zeros); the test functions phi_i are
 * the rows i < nt on the inner dofs and zero on the Dirichlet dofs.  1 <= nt
 * <= nb <= 33 (32 modes and a mean flow).  Fixed chunks of 512 cells, fp64
 * matrix cores, partial tiles added in chunk order: no atomics, the same bits
 * in every run.  The operator's own Dirichlet values and tables play no part
 * and stay as they are */
int dns_conv_project_tensor(dns_conv *cv, int32_t nb, int32_t nt, int32_t ld,
                            const double *basis, const double *dbc_rows,
                            double *out);
/* let the stepper evaluate nfc_c = scale * N(v_c)v_c itself every step
 * (scale = -1: "goes to the rhs", stokes_navier_utils.py:1128-1140); NULL
 * detaches.  dns_imex_step then takes nfc_new = NULL and dns_imex_run
 * advances the convection history instead of freezing it */
int dns_imex_set_convection(dns_imex *st, dns_conv *cv, double scale);

/* ---- standalone kernels (parity tests, micro-benchmarks) -----------------
 * upload, run the same device kernels the solver uses, download */
int dns_spmv(int device, const dns_csr *a, const double *x, double *y,
             double alpha, double beta, int32_t variant);
int dns_dot(int device, int64_t n, const double *x, const double *y,
            double *out);
int dns_axpy(int device, int64_t n, double a, const double *x, double *y);
int dns_gemv(int device, int32_t n, const double *a_rowmajor, const double *x,
             double *y, double alpha);
/* dense in-place inverse by the device Gauss-Jordan used for the Schur block */
int dns_dense_inverse(int device, int32_t n, double *a_rowmajor);

/* the two dense operations of dns_imex_ensemble_gram / _combine alone, through
 * the same launchers: e is m x ld on the host (ld even, >= nv; entries at and
 * behind nv of a row are never read), w NV x NV or NULL, g m x m, coef r x m,
 * out r x nv */
int dns_ensemble_gram(int device, int32_t m, int32_t nv, int32_t ld,
                      const double *e, const dns_csr *w, double *g);
int dns_ensemble_combine(int device, int32_t m, int32_t nv, int32_t ld,
                         const double *e, int32_t r, const double *coef,
                         double *out);
/* p (mx x my, row-major) = X W Y^T, p[i, j] = x_i . (W y_j): the reduced
 * operators of a Galerkin projection.  x is mx x ld and y my x ld on the host
 * (ld even, >= nv, as above); y NULL: Y = X (my is ignored); w any NV x NV
 * matrix -- it need not be symmetric -- or NULL for the identity.  The kernels
 * are those of dns_ensemble_gram in their non-mirroring form: the same chunks
 * of 1024 entries summed in chunk order, no atomics, the same bits in every
 * run; with Y = X and a symmetric w the tiles on and above the block diagonal
 * hold dns_ensemble_gram's bits */
int dns_ensemble_project(int device, int32_t mx, int32_t my, int32_t nv,
                         int32_t ld, const double *x, const double *y,
                         const dns_csr *w, double *p);

/* repeat y = A x `reps` times on resident data; reports the average kernel
 * time (HIP events on the launch stream) -- the roofline measurement */
int dns_spmv_bench(int device, const dns_csr *a, int32_t variant, int32_t reps,
                   int32_t warmup, double *avg_seconds, double *checksum);
/* y = K x for K = [[F, JT],[J, 0]] (CSR, velocity rows/columns first, `nv` of
 * them) through the 2x2-blocked PAIR format: rows and columns are taken in
 * pairs (the two velocity dofs of a node; consecutive pressure dofs), an entry
 * is a 2x2 block = four values + one 16-bit column offset, served by one
 * 16-byte gather of x.  Holds any K with even nv and even size (explicit zeros
 * where a block is not full); DNS_ERR_BAD_ARGUMENT otherwise.  reps > 0 and
 * avg_seconds != NULL: seconds per launch by HIP events, as dns_spmv_bench;
 * format_bytes: device bytes of the format (may be NULL).  Inside a solver
 * the format carries the K applies of the bandwidth regime automatically
 * (DNS_PAIR=0 turns it off). */
int dns_spmv_pair(int device, const dns_csr *k, int32_t nv, const double *x,
                  double *y, int32_t reps, int32_t warmup, double *avg_seconds,
                  int64_t *format_bytes);

/* ONE launch of the streaming kernel with epilogues (k_spmv_stream16x) or of
 * the pair kernel (k_spmv_pair16x) with the epilogue described here -- what the
 * solver's large applies run, reachable in isolation (tests).  Vectors b, dinv,
 * xin and the rows of V are indexed by GLOBAL row and hold `ny` entries (V: `ld
 * >= ny` apart).  Any combination the chosen kernel does not implement is
 * refused with DNS_ERR_BAD_ARGUMENT. */
#define DNS_EPI_STREAM  0
#define DNS_EPI_PAIR    1
#define DNS_EPI_PLAIN   0   /* y = alpha A x + beta b                         */
#define DNS_EPI_SWEEP   1   /* y = alpha (xin + omega dinv .* (b - A x))       */
#define DNS_EPI_ADD_CB  2   /* y = alpha A x + omega dinv .* b                 */
typedef struct dns_spmv_epi {
    int32_t kernel;          /* DNS_EPI_STREAM / DNS_EPI_PAIR                  */
    int32_t nv;              /* pair: GLOBAL number of velocity dofs           */
    int32_t fp32_vals;       /* stream: values rounded to float on the device  */
    int32_t mode;            /* DNS_EPI_PLAIN / _SWEEP / _ADD_CB               */
    double alpha, beta, omega;
    const double *b;         /* may be NULL (plain)                            */
    const double *x2;        /* != NULL: x holds the columns < nsplit, x2 the  */
    const double *dinv;      /*          other ncols - nsplit                  */
    const double *xin;       /* sweep; NULL = 0                                */
    const double *V;         /* fused dots: nvec vectors, ld apart             */
    int64_t ld;
    int64_t ny;              /* entries of y (global length)                   */
    int64_t part_len;        /* doubles the caller's `part` / `part_bb` hold   */
    int64_t part_bb_len;
    int32_t nsplit;
    int32_t nvec, with_ww, with_bb;
    int32_t map_on;          /* stream: RowMap{row0, len1, row2, len2}         */
    int32_t row0, len1, row2, len2;
    int32_t nvl, v0, p0;     /* pair: nvl >= 0 = row block of nvl velocity rows
                              * from even global row v0, pressure rows from p0 */
    int32_t grid_cap;        /* at most this many workgroups (= partials)      */
    int32_t use_guard, guard;/* use_guard: launch with a device flag = guard   */
    int32_t pad;
} dns_spmv_epi;
/* `a`: the matrix (stream: its rows are the RowMap's; pair: K or a row block of
 * K with global columns).  y (ny entries), part and part_bb are uploaded with
 * the caller's contents, so what the launch did not write comes back as it
 * was.  part != NULL turns the fused dots on: row i < nvec of the
 * (nvec + 1) x *nparts table holds the partials of <V_i, y>, row nvec those of
 * <y, y> (with_ww); part_bb[*nparts] those of <b, b> (with_bb).  *nparts = the
 * grid that was launched, *nblocks = the row blocks of the format. */
int dns_spmv_epilogue(int device, const dns_csr *a, const dns_spmv_epi *e,
                      const double *x, double *y, double *part,
                      double *part_bb, int32_t *nparts, int32_t *nblocks);

/* TEST ONLY: ONE launch of a row kernel of the lazy six-node step on the
 * caller's operators, with the grid the step gives it (tests of the kernels in
 * isolation: row lengths at the edges of their load chunks).
 *   GC    a: nv x (nv + np), nsplit = nv; x = r_v (nv), x2 = z_p (np);
 *         y = a [x; x2] (nv).  fp32_vals: values rounded to float
 *   TAU   a: np x nv; x = b, x2 = kx (nv + np each); y (np) =
 *         (b - kx)[nv + i] - (a (b - kx)[:nv])[i]; y2 (optional) = b - kx
 *   STEP  a = K (n x n), a2 = R1 (nv x nv), a3 = the cell list (nv x ncell, its
 *         values are not read); x = x0, x2 = v_c, x3 = v_p (n each), x4 = cell
 *         values (ncell); y = K x0 (n), y2 = b (n): b_v = R1 (a_c v_c + a_p v_p)
 *         + 0 * (...), b_p = 0; y3 (nv) = sum of the listed cell values
 *   RW    a = K (n x n); x = z, x2 = r; y = w = K z, y2 = [<r, w> | <w, w>]
 *         partials, nparts of each (room for 2 x 256)
 *   HEAD  a unused; nsplit = np, x2 = np x np rows (row-major, rounded to
 *         float), x = tau; y = -x2 tau (k_arn_head_lazy, fp32 rows)          */
#define DNS_ROWK_GC    0
#define DNS_ROWK_TAU   1
#define DNS_ROWK_STEP  2
#define DNS_ROWK_RW    3
#define DNS_ROWK_HEAD  4
typedef struct dns_row_probe {
    int32_t kernel;          /* DNS_ROWK_*                                     */
    int32_t lpr;             /* lanes per row (GC, STEP, RW)                   */
    int32_t fp32_vals;       /* GC                                             */
    int32_t nsplit;          /* GC: nv; HEAD: np                               */
    const dns_csr *a2, *a3;
    const double *x2, *x3, *x4;
    double a_c, a_p;         /* STEP                                           */
    double *y2, *y3;
    int32_t nparts;          /* out (RW)                                       */
    int32_t pad;
} dns_row_probe;
int dns_row_kernel_probe(int device, const dns_csr *a, dns_row_probe *p,
                         const double *x, double *y);

/* Multigrid Schur block for pressure spaces too large for the dense inverse
 * (refined meshes).  `prol[l]` (CSR, n_l x n_{l+1}, l = 0 .. nprol-1) are the
 * prolongations of a nested hierarchy of pressure spaces, finest first (n_0 =
 * NP); the coarsest space gets a dense inverse, so keep n_nprol at a few
 * thousand.  At `dns_saddle_setup_precond(schur = DNS_SCHUR_MG)` the library
 * forms the sparse Schur complement S_0 = J Fh^-1 JT (explicit Fh^-1) or
 * J D^-1 JT (recurrence), the Galerkin operators S_{l+1} = P_l^T S_l P_l and
 * applies Sh^-1 ~ one V(nu,nu)-cycle with damped Jacobi smoothing (in the
 * row-partitioned solve every rank runs the whole cycle).
 * (Reference counterpart: none -- its direct solver does not need one.) */
int dns_saddle_set_schur_mg(dns_saddle *h, int32_t nprol, const dns_csr *prol,
                            int32_t smooth_steps);
/* Tuning knobs of ONE handle, to be set before dns_saddle_setup_precond (the
 * environment variables DNS_<NAME> give the defaults when the handle is
 * created; this call replaces process-global state in tests and drivers):
 *   "stream_nnz"    matrices with at least this many non-zeros take the
 *                   LDS-streaming kernels (bandwidth regime)
 *   "pair"          0/1: pair format of K in the bandwidth regime
 *   "mg_dense_max"  first multigrid level <= this gets the dense inverse
 *   "mg_dense_half_max"  ... and a level up to this size gets it in half
 *                   precision (one bandwidth-bound launch instead of the five
 *                   latency-bound launches of a sparse level); 0 = never
 *   "mg_part_min"   levels with at least this many rows are row-partitioned
 *   "mg_fused"      0/1: fused V(2,2) operators
 *   "mg_cheb"       0/1: Chebyshev pair of smoothing weights; "mg_cheb_alpha"
 *   "mg_cycles"     1 or 2 cycles per application; "mg_rho"
 *   "dist_graph"    0/1: hipGraph replay with captured RCCL calls
 *   "cycle_first"   > 0: Krylov steps in the first cycle of every solve
 *                   (default: what the previous solve needed, plus one)
 *   "dist_lazy1"    0/1: one-step cycles of a partitioned solve leave the
 *                   first basis vector un-normalised; ||r||, ||b|| travel with
 *                   the step's dots (one all-reduce per time step less)
 *   "step6_lazy"    0/1: one-column cycles of the six-node resident step
 *                   normalise nothing: the head is the Schur product alone,
 *                   the tail forms the step from <r,Kz>, <Kz,Kz>, ||r||^2
 *                   (default 1, DNS_STEP6_LAZY; longer cycles are general)
 *   "dist_x0_exchange"  0/1: halo exchange of the start vector at the head of
 *                   every cycle of a partitioned solve (default 0: it is valid)
 *   "part_setup"    0/1: with a communicator, every rank forms only the rows
 *                   of Fh^-1, J Fh^-1 and of the Schur complement its blocks
 *                   are made of (default 1; 0: every rank forms all rows)
 *   "mg_stream_nnz": operators of the multigrid cycle with at least this
 *                   many non-zeros run as fp32 streams through the
 *                   LDS-streaming kernels (default 600000; "stream_nnz",
 *                   1300000, is the threshold of K, Fh^-1 and J Fh^-1)
 *   "oversolve"   : 1 / 0 = the solves of a pipelined batch run the columns
 *                   of their cycle instead of stopping at the tolerance / stop
 *                   at it (slack-column policy); -1 = the default (on with the
 *                   multigrid Schur block below 1.5e6 unknowns)
 *   "oversolve_cmin": shortest cycle the oversolve policy tries (default 2
 *                   with the multigrid block, else 1)
 * Unknown names: DNS_ERR_BAD_ARGUMENT.  (No reference counterpart.) */
int dns_saddle_set_option(dns_saddle *h, const char *name, double value);

/* ---- linearised convection matrices + Newton/Picard trapezoidal sweeps ------
 * (reference: `get_v_conv_conts` snu:109-133 with `get_convmats` dts:325-376
 * and `condense_velmatsbybcs` dts:610-642; `_get_mats_rhs_ts` snu:1016-1047;
 * the time loop snu:1402-1566)
 *
 * dns_conv_bind_pattern: the CSR pattern (values ignored) the condensed
 *   N1(u) (+ N2(u)) are assembled into -- it must contain theirs, e.g. the
 *   pattern of A (symmetric-gradient form) or of M + A kept with its zeros.
 * dns_conv_assemble (host pointers; the parity-test entry): values of
 *   N1(u) [newton = 0] or N1(u) + N2(u) [newton = 1] in that pattern,
 *   rhsbc = -N[:, Dirichlet cols] * Dirichlet values (may be NULL) and
 *   rhscon = N(u)u (may be NULL).
 */
int dns_conv_bind_pattern(dns_conv *cv, const dns_csr *pattern);
int dns_conv_assemble(dns_conv *cv, const double *u_inner, int32_t newton,
                      double *nvals, double *rhsbc, double *rhscon);

/* the same with two sets of Dirichlet values: `dbcvals_lin` belong to the
 * linearisation field (they enter N1, N2 and N(u)u), `dbcvals_rhs` multiply
 * the Dirichlet columns in `rhsbc` (NULL: the same set) -- the steady Picard
 * iteration uses the old values for the field and the new ones for the rhs
 * (snu:446-455); the operator's own value set / table is not touched */
int dns_conv_assemble2(dns_conv *cv, const double *u_inner,
                       const double *dbcvals_lin, const double *dbcvals_rhs,
                       int32_t newton, double *nvals, double *rhsbc,
                       double *rhscon);

/* Trapezoidal stepper: M, A given as value arrays in the pattern of `sys`'s F
 * block (to which `conv` must be bound); two trajectory buffers of `nslots`
 * velocities each hold the linearisation points of the running sweep
 * (`which`) and the velocities it produces (`1 - which`).
 *   start : v_c = iniv, f_c - N_c v_c evaluated there, update norm reset
 *   step  : one step of size dt linearised about traj[lin_which][lin_slot];
 *           F = M + dt/2 (A + N_n) is formed on the device inside `sys`
 *           (same pattern, preconditioner kept); result -> traj[1-lin_which]
 *           [out_slot] (out_slot < 0: not stored).  `extrapolate_x0` = order
 *           of the warm start from the last solutions, 0 .. 4 as in
 *           dns_imex_coeffs (the reference's `krylovini='upd'` is order 1,
 *           snu:1493-1503).  The part of the right-hand side that depends on
 *           the current velocity through the convection, f_c - N_c v_c, is
 *           evaluated as fv - N(v_c)v_c (N1(u)u = N2(u)u = N(u)u): no second
 *           matrix assembly per step
 *   get_state: v_c and p = -p~/dt (snu:1542)
 *   update_norm: sum of dt ||v_n - v_lin||_M^2 since `start` (snu:1557-1560)
 */
typedef struct dns_trap dns_trap;
int dns_trap_create(dns_saddle *sys, dns_conv *conv, const double *m_vals,
                    const double *a_vals, int32_t nslots, dns_trap **out);
void dns_trap_destroy(dns_trap *t);
int dns_trap_set_rhs(dns_trap *t, const double *fv, const double *fp);
int dns_trap_traj_write(dns_trap *t, int32_t which, int32_t slot,
                        const double *v);
int dns_trap_traj_read(dns_trap *t, int32_t which, int32_t slot, double *v);
/* Asynchronous writer of the trajectory store (replaces the
 * blocking per-step `dou.save_npa`, reference snu:1012-1014, 1424-1431): the
 * copy of the slots [slot0, slot0+count) of traj[which] (count*NV doubles,
 * into a page-locked buffer of the library's) is queued on a copy stream of
 * its own
 * behind the work the solver's stream has been given so far; the call returns
 * at once and the next sweep runs while the data travels.  The solver's stream
 * waits for a pending export only before it overwrites traj[which].
 * dns_trap_traj_export_wait blocks until all exports have arrived and fills
 * the `host` arrays (which have to be alive until then); any host thread may
 * call it. */
int dns_trap_traj_export_async(dns_trap *t, int32_t which, int32_t slot0,
                               int32_t count, double *host);
int dns_trap_traj_export_wait(dns_trap *t);
int dns_trap_start(dns_trap *t, const double *iniv, int32_t newton);
int dns_trap_step(dns_trap *t, double dt, int32_t lin_which, int32_t lin_slot,
                  int32_t out_slot, int32_t newton, int32_t extrapolate_x0,
                  const dns_solve_opts *opts, dns_solve_stats *stats);
int dns_trap_get_state(dns_trap *t, double *v, double *p);
int dns_trap_update_norm(dns_trap *t, double *out);
/* On a row-partitioned system (dns_saddle_set_comm) the stepper's assembly is
 * partitioned like the solve and no solution is gathered per step: trajectory
 * slots and states hold a rank's rows and its halo.  dns_trap_traj_read,
 * dns_trap_traj_export_async, dns_trap_get_state and dns_trap_update_norm are
 * COLLECTIVE then (they gather / all-reduce first): every rank calls them. */
/* time-dependent data of the sweeps, one row per trajectory slot (= time
 * instance; nslots rows each, NULL = not time dependent): `fv_tab` replaces fv
 * (forcing `fvtd(t)` and the stiffness contribution of controlled boundary
 * values, snu:1466-1468), `fp_tab` replaces fp, `mbc_tab` = M[:, cnt] bcvals(t)
 * adds `mbcs_n - mbcs_c` to the rhs (snu:1044-1045, 1438-1441) */
int dns_trap_set_tables(dns_trap *t, const double *fv_tab, const double *fp_tab,
                        const double *mbc_tab);
/* one step with the low-rank feedback terms of `_get_mats_rhs_ts`
 * (snu:1036-1042, passed at snu:1505-1512): system matrix F - dt/2 U V_n
 * (Sherman-Morrison-Woodbury: r more solves with the same K), right-hand side
 * + dt/2 U (V_c v_c).  umat: NV x r column major; vmat_c (may be NULL),
 * vmat_n: r x NV row major; synchronous steps only */
int dns_trap_step_fb(dns_trap *t, double dt, int32_t lin_which,
                     int32_t lin_slot, int32_t out_slot, int32_t newton,
                     int32_t extrapolate_x0, const dns_solve_opts *opts,
                     dns_solve_stats *stats, int32_t r, const double *umat,
                     const double *vmat_c, const double *vmat_n);
/* pipelined sweeps: with cycle_len > 0 `dns_trap_step` only enqueues (one GMRES
 * cycle of that length, no host synchronisation, `stats` not filled); the
 * device counts solves / unconverged solves / Krylov steps and keeps the update
 * norm; `dns_trap_poll` synchronises, hands the counters back (and resets
 * them) and folds the device part of the update norm in.  A sweep with
 * `fails > 0` has to be repeated with cycle_len = 0. */
int dns_trap_set_pipeline(dns_trap *t, int32_t cycle_len);
/* `count` pipelined steps of step size dt in a row: step k has its
 * linearisation point in slot slot0 + k of traj[lin_which] and stores its
 * velocity in the same slot of the other buffer (the time loop of a sweep,
 * snu:1402-1566, without a trip through the caller per step).  Needs
 * dns_trap_set_pipeline(cycle_len > 0) */
int dns_trap_run(dns_trap *t, double dt, int32_t lin_which, int32_t slot0,
                 int32_t count, int32_t newton, int32_t extrapolate_x0,
                 const dns_solve_opts *opts);
int dns_trap_poll(dns_trap *t, int32_t *solves, int32_t *fails, int32_t *iters,
                  int32_t *maxit);
/* Oversolve of the pipelined batches: with stop_frac > 0 a solve does not stop
 * at the tolerance but runs the columns of its cycle (the nodes of a replayed
 * cycle are paid for either way) until its residual is below stop_frac x
 * tolerance; 0 (default) = stop at the tolerance.  dns_trap_poll_ext: the
 * counters of dns_trap_poll in out6[0..3], out6[4] = the largest number of
 * columns a solve NEEDED to meet the tolerance, out6[5] = the sum of those
 * numbers over the batch's solves, out2[0] = batch maximum of
 * final residual / tolerance, out2[1] = ... of the residual in front of the
 * last column / tolerance: what the host's choice of the next cycle length
 * goes by. */
int dns_trap_set_oversolve(dns_trap *t, double stop_frac);
int dns_trap_poll_ext(dns_trap *t, int32_t *out6, double *out2);
/* checkpoint / restore of the stepper's state between pipelined batches: a
 * batch in which a step did not converge within the agreed cycle length is
 * repeated from the checkpoint (call `dns_trap_checkpoint` behind a
 * `dns_trap_poll`; `dns_trap_restore` leaves the pipeline switched off and
 * re-assembles N_c / f_c at the restored velocity) */
int dns_trap_checkpoint(dns_trap *t);
int dns_trap_restore(dns_trap *t, int32_t newton);

/* TEST ONLY.  The launches a `dns_trap_step` (default options) enqueues BEFORE
 * its solve -- warm start, element launch, gather launch, by the same member
 * function the step calls -- then a synchronise and a copy out: the assembly
 * pair of a trapezoidal step reachable in isolation.  Every pointer of `out`
 * may be NULL.  x0_in != NULL: these NV + NP values are the warm start instead
 * of the extrapolated one.  Needs no preconditioner.  DNS_ERR_NOT_READY with a
 * pipelined batch or a pending update-norm job, DNS_ERR_BAD_ARGUMENT on a
 * row-partitioned handle.  The system matrix is re-valued and no solution
 * follows: call dns_trap_start before the stepper steps again. */
typedef struct dns_trap_probe {
    double *nvals, *fvals;   /* N(v_lin), F = M + dt/2 (A + N): nnz of pattern */
    double *kfvals;          /* the values of F as they sit in K (nnz)         */
    double *rhsbc, *fvn;     /* NV each                                        */
    double *b, *x0;          /* NV + NP each: right-hand side, warm start used */
    double *r;               /* NV + NP, written if *fused                     */
    double *partR, *partB;   /* parts_cap each: raw partials, if *fused        */
    int32_t parts_cap;
    int32_t nparts;          /* out: partials the launch wrote (0: not fused)  */
    int32_t fused;           /* out: the start residual came from the gather   */
    int32_t pad;
} dns_trap_probe;
int dns_trap_assembly_probe(dns_trap *t, double dt, int32_t lin_which,
                            int32_t lin_slot, int32_t newton,
                            const double *x0_in, dns_trap_probe *out);

/* ---- resident helpers of the caller side of the path -----------------------
 * A CSR matrix kept in HBM for repeated products with host vectors: what the
 * closures of `solve_nse` do per step with SciPy -- `applybcs` (snu:1111-1115:
 * -A[:, cnt] vals, -J[:, cnt] vals, M[:, cnt] vals),
 * `condense_velmatsbybcs(get_rhs_only=True)` (dts:610-630) -- and the J / J^T
 * products of the decoupled pressure solve (snu:1622-1628).
 *   y = alpha A x + beta y   (host vectors) */
typedef struct dns_op dns_op;
int dns_op_create(int device, const dns_csr *a, dns_op **out);
void dns_op_destroy(dns_op *op);
int dns_op_apply(dns_op *op, const double *x, double *y, double alpha,
                 double beta);
/* `append_bcs_vec` (dts:49-64): out = NaN everywhere, then out[invinds] =
 * v_inner, then out[bcinds] = bcvals (boundary values win; of a repeated index
 * the last occurrence wins, as in NumPy's fancy assignment) */
typedef struct dns_bcmap dns_bcmap;
int dns_bcmap_create(int device, int32_t vdim, int32_t ninv,
                     const int32_t *invinds, int32_t nbc, const int32_t *bcinds,
                     dns_bcmap **out);
void dns_bcmap_destroy(dns_bcmap *m);
int dns_bc_scatter(dns_bcmap *m, const double *v_inner, const double *bcvals,
                   double *out_full);

/* attainable HBM bandwidth of the device, measured with plain streaming
 * kernels over `bytes` of fp64 data (kind 0: read + reduce, 1: copy,
 * 2: triad a = b + s c); reports GB/s of the bytes the kernel moves.  The SpMV
 * roofline fraction is quoted against the 8 TB/s peak AND against this. */
int dns_hbm_probe(int device, int64_t bytes, int32_t kind, int32_t reps,
                  double *gbytes_per_s);

#ifdef __cplusplus
}
#endif
#endif /* DNS_AMD_H */
