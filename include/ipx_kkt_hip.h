/* ipx_kkt_hip.h -- C ABI of the MI355X (gfx950) implementation of IPX's
 * per-IPM-iteration KKT normal-equations solve.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.
 * Each entry point names the reference interface (file:line under the reference
 * root) it replaces; ipx_amd/host/ holds KKTSolver / LinearOperator subclasses
 * written against the reference's own headers that call nothing but this file
 * (see INTEGRATION.md for the three lines of lp_solver.cc that select them).
 *
 * Conventions
 *  - ipxint = int64_t (include/ipx_config.h:5); values are IEEE fp64.
 *  - Sparse matrices are CSC triples (colptr[ncol+1], rowidx[nnz], values[nnz])
 *    exactly as ipx::SparseMatrix stores them (src/sparse_matrix.h:59-65).
 *  - Vector arguments are host pointers by default (the reference's Vector is a
 *    std::valarray in host memory).  ipxk_set_pointer_mode(IPXK_POINTER_DEVICE)
 *    switches all *vector* arguments of the solve/apply calls to device
 *    pointers (resident inputs, what bench.py times); matrix/factor/permutation
 *    arguments are always host pointers (they are uploaded once per
 *    model / per Factorize).
 *  - Every function returns 0 on success or a negative IPXK_E_* code; the text
 *    of the last failure is available from ipxk_last_error().  Numerical
 *    outcomes use the reference's own channel: an `errflag` output holding 0 or
 *    an IPX_ERROR_* value of include/ipx_status.h:31-47.
 *  - A context is not thread safe; calls block until results are in the output
 *    arrays (the reference interface is blocking and single-threaded).
 */
#ifndef IPX_KKT_HIP_H_
#define IPX_KKT_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int64_t ipxint;
typedef struct ipxk_context ipxk_context;

#define IPXK_OK 0
#define IPXK_E_HIP (-1)        /* HIP runtime / RCCL failure  -> std::runtime_error */
#define IPXK_E_ALLOC (-2)      /* device or host allocation   -> std::bad_alloc     */
#define IPXK_E_ARGUMENT (-3)   /* invalid argument / state    -> std::logic_error   */
#define IPXK_E_UNSUPPORTED (-4)

#define IPXK_POINTER_HOST 0
#define IPXK_POINTER_DEVICE 1

/* basis statuses, values of ipx::Basis::BasicStatus (src/basis.h:64) */
#define IPXK_NONBASIC_FIXED (-2)
#define IPXK_NONBASIC (-1)
#define IPXK_BASIC 0
#define IPXK_BASIC_FREE 1

/* variable states, one byte per variable: Iterate::StateOf with the barrier state
 * split by Iterate::has_barrier_lb / has_barrier_ub (src/iterate.h:99-108,295-318) */
#define IPXK_STATE_FIXED 0
#define IPXK_STATE_FREE 1          /* FREE and IMPLIED_EQ (finite lb == ub) */
#define IPXK_STATE_BARRIER_LB 2
#define IPXK_STATE_BARRIER_UB 3
#define IPXK_STATE_BARRIER_BOXED 4
/* Iterate::make_implied_lb / make_implied_ub (src/iterate.cc:160-172), the result of DropPrimal: xl = xu = inf, zl and
 * zu keep their values, the IPM treats the variable as free; Postprocess puts it on its bound (:294-308) */
#define IPXK_STATE_IMPLIED_LB 5
#define IPXK_STATE_IMPLIED_UB 6

/* Wall-clock seconds accumulated by the last solve, measured with HIP events on
 * the context's stream; they feed ipx_info::time_cr1* / time_cr2*
 * (include/ipx_info.h:66-75, src/kkt_solver_diag.cc:100-105,
 * src/kkt_solver_basis.cc:151-156). */
typedef struct ipxk_times {
    double cr;        /* whole CR loop            -> time_cr1 / time_cr2      */
    double op;        /* operator C applications  -> time_cr1_AAt / _NNt      */
    double precond;   /* preconditioner P         -> time_cr1_pre             */
    double solve_B;   /* forward solves           -> time_cr2_B               */
    double solve_Bt;  /* backward solves          -> time_cr2_Bt              */
} ipxk_times;

/* What the reference prints through control_.Debug(3) when a CR run stops on an
 * error (src/conjugate_residuals.cc:53-56,140-152,198-202): the numbers of the
 * last CR run on this context, for the host classes to format. */
typedef struct ipxk_cr_diag {
    ipxint errflag, iter, maxiter;
    double resnorm, tol;            /* 201: residual at the last loop head, tolerance */
    double cdot;                    /* 202: rhs-dot-lhs of the last operator application */
    double infnorm_residual;        /* 202 */
    double infnorm_sresidual;       /* 202 (preconditioned CR; 0 for plain CR) */
    double rps_old, rps_new;        /* 204: resnorm_precond_system before / after the 5 iterations */
} ipxk_cr_diag;

const char* ipxk_last_error(void);
int ipxk_device_count(void);

/* ---- model upload (stand-alone, host arrays, computed on `device`) ---- */
/* Presolver::EquilibrateMatrix (src/presolver.cc:883-974): recursive row / column
 * equilibration of the m x n structural matrix by powers of two.  Ax is scaled in
 * place; colscale[n], rowscale[m] receive the accumulated factors (1 where none).
 * *rounds = number of rounds that rescaled the matrix, or -1 if every entry was in
 * range from the start (the reference then leaves its scaling vectors empty,
 * src/presolver.cc:912-924).  All arithmetic is exact: bit-identical results. */
int ipxk_equilibrate(ipxint m, ipxint n, const ipxint* Ap, const ipxint* Ai,
                     double* Ax, double* colscale, double* rowscale,
                     ipxint* rounds, int device);
/* Transpose (src/sparse_matrix.cc:120-151): row-wise copy of an m x n CSC matrix,
 * entries of a row in ascending source-column order (Model::AIt, src/model.h:61). */
int ipxk_transpose(ipxint m, ipxint n, const ipxint* Ap, const ipxint* Ai,
                   const double* Ax, ipxint* ATp, ipxint* ATi, double* ATx,
                   int device);

/* ---- context: the model's matrix, resident on one GPU -------------------- */
/* Replaces the role of ipx::Model::AI()/AIt() for the path (src/model.h:61):
 * uploads the n structural columns of AI = [A I] (the slack identity is never
 * stored) as a 32-bit-index CSC and builds the row-wise copy on the device
 * side's own index arithmetic (Transpose, src/sparse_matrix.cc:120-151 --
 * ascending source-column order within each row).  Also classifies dense
 * columns as Model::FindDenseColumns does (src/model.cc:34-56). */
int ipxk_create(ipxint m, ipxint n, const ipxint* Ap, const ipxint* Ai,
                const double* Ax, int device, ipxk_context** out);
void ipxk_destroy(ipxk_context* ctx);
int ipxk_set_pointer_mode(ipxk_context* ctx, int mode);
/* Use a caller-owned hipStream_t (e.g. torch's current stream); NULL restores
 * the context's own stream. */
int ipxk_set_stream(ipxk_context* ctx, void* hip_stream);
int ipxk_synchronize(ipxk_context* ctx);
/* on != 0: HIP events around every operator / preconditioner / triangular-solve application fill
 * ipxk_times::op, precond, solve_B, solve_Bt (the reference's per-object timers,
 * src/normal_matrix.cc:57,125, src/diagonal_precond.cc:126,158,
 * src/splitted_normal_matrix.cc:93-110).  Off by default: ~2 extra stream markers per call. */
int ipxk_set_profiling(ipxk_context* ctx, int on);
/* Control::InterruptCheck for the calls that take no callback of their own: ipxk_maxvolume and
 * ipxk_maxvolume_sequential poll it once per candidate column (src/maxvolume.cc:52,250); a nonzero
 * value ends the run with info->errflag = that value, the exchanges made so far kept.  NULL: none. */
int ipxk_set_interrupt(ipxk_context* ctx, ipxint (*interrupt)(void* user), void* interrupt_user);
/* A context handed from one solver object to the next (ipx_amd/host/hip_device.h keeps one per Model, as the
 * reference's solver objects share one Model, src/lp_solver.cc:375,386,457) starts like a new one: NormalMatrix /
 * DiagonalPrecond / KKTSolverDiag unprepared, no iterate, no operator of a basis, no LU factors, no interrupt
 * callback, host pointer mode, own stream; the pivot tolerance of Maxvolume's refactorizations -- tightened for good
 * after an unstable exchange, like Basis::TightenLuPivotTol (src/basis.cc:490-503) -- is set to lu_pivottol
 * (Control::lu_pivottol(), src/basis.cc:30; <= 0: 0.1).  The model and its layouts stay; workspaces stay allocated. */
int ipxk_reset_solver_state(ipxk_context* ctx, double lu_pivottol);
/* # dense columns of Model::FindDenseColumns (src/model.cc:34-56).  After ipxk_comm_init / ipxk_comm_init_columns:
 * of the WHOLE partitioned matrix, the same number on every rank (a rank of the column partition may own none). */
ipxint ipxk_num_dense_cols(const ipxk_context* ctx);
/* The locality-recovering renumbering of the model ("row/column reordering ... must stay a pure permutation").
 * ipxk_create looks for one -- breadth-first levels of the bipartite graph rows <-> columns from a pseudo-peripheral row, rows
 * and columns numbered by (level, index) -- builds a second copy of the matrix in that numbering with gather layouts of its own,
 * times NormalMatrix::Apply's two products on both copies and keeps the copy if it is at least 10 % faster.  Then the CR loop of
 * ipxk_kkt_diag_solve (src/kkt_solver_diag.cc:98-99) runs on the copy: right-hand side, weights, preconditioner and residual
 * scaling are permuted going in, y coming out; nothing else of the ABI sees the numbering.  Models with dense columns (the
 * Sherman-Morrison-Woodbury preconditioner), partitioned contexts and models of fewer than 2^20 entries keep the numbering as given;
 * a matrix without structure (half of its rows within 8 levels of any row) is recognised at once.  IPXK_REORDER=0: never, =1: always. */
typedef struct {
  ipxint active;             /* 1: the renumbered copy is in use */
  ipxint levels, components; /* of the breadth-first structure */
  double ms;                 /* cost inside ipxk_create */
  double us_original, us_reordered;   /* the two products of one Apply on either copy (0: not timed) */
} ipxk_reorder_info;
int ipxk_get_reorder_info(const ipxk_context* ctx, ipxk_reorder_info* info);
/* rowperm[m], colperm[n]: new index -> index as given (either may be NULL); fails if no renumbering was computed */
int ipxk_get_reordering(ipxk_context* ctx, ipxint* rowperm, ipxint* colperm);
/* Copies out the device-side row-wise matrix (for bit-exact index parity
 * tests against Transpose): ATp[m+1], ATi[nnz], ATx[nnz]; NULL skips. */
int ipxk_get_rowwise(const ipxk_context* ctx, ipxint* ATp, ipxint* ATi,
                     double* ATx);

/* ---- NormalMatrix (src/normal_matrix.h:18-43) ---------------------------- */
/* Prepare(W): W has n+m entries or is NULL (1 on structurals, 0 on slacks).
 * Unlike the reference (raw pointer kept, normal_matrix.h:24-28) W is copied
 * to the device here; in device pointer mode it is used in place. */
int ipxk_normal_prepare(ipxk_context* ctx, const double* W);
/* _Apply (src/normal_matrix.cc:45-126): lhs = AI*W*AI'*rhs, optional dot. */
int ipxk_normal_apply(ipxk_context* ctx, const double* rhs, double* lhs,
                      double* rhs_dot_lhs);

/* ---- DiagonalPrecond (src/diagonal_precond.h:25-57) ---------------------- */
/* Factorize (src/diagonal_precond.cc:17-111); *errflag = 0 or
 * IPX_ERROR_lapack_chol (401).  On a partitioned system the dense-column (Sherman-Morrison-Woodbury) form
 * factorizes the Schur complement of the whole matrix on every rank: all ranks hold the same k x k factor
 * bit for bit and return the same errflag.  Row partition: one all-reduce of k^2 doubles here and one of k
 * doubles per ipxk_diag_apply (lhs is this rank's slice; ipxk_diag_get returns the local diagonal and the
 * global factor).  Column partition: the dense columns of all ranks are gathered once per communicator and
 * the k dense weights per Factorize; Apply exchanges nothing (its vectors are replicated). */
int ipxk_diag_factorize(ipxk_context* ctx, const double* W,
                        int precond_dense_cols, ipxint* errflag);
/* _Apply (src/diagonal_precond.cc:121-159) */
int ipxk_diag_apply(ipxk_context* ctx, const double* rhs, double* lhs,
                    double* rhs_dot_lhs);
/* copies diagonal_[m] and the k x k column-major Cholesky factor; NULL skips */
int ipxk_diag_get(const ipxk_context* ctx, double* diagonal, double* chol);

/* ---- ConjugateResiduals (src/conjugate_residuals.h:20-70) ---------------- */
/* Preconditioned CR (src/conjugate_residuals.cc:90-213) with C = the prepared
 * NormalMatrix and P = the factorized DiagonalPrecond.  lhs: initial iterate in,
 * solution out.  resscale may be NULL.  maxiter < 0 means m+100.
 * interrupt (may be NULL) plays Control::InterruptCheck()
 * (src/control.cc:17-22): a nonzero return value stops the solve and becomes
 * *errflag.  Granularity: the reference polls after every iteration
 * (src/conjugate_residuals.cc:209); here the callback is polled once per 5
 * iterations that the host enqueues, first after the first five (a
 * system whose initial residual meets tol returns errflag 0 whatever the
 * callback says, like the reference).  What is in the queue is finished:
 * *iter is the number of iterations enqueued when the callback returned
 * nonzero.  On a partitioned system the host runs up to 2 cycles of 5
 * iterations ahead and the flag is reduced (max) over the ranks together
 * with the loop's `done` snapshot, so every rank leaves the loop in the
 * same cycle, up to 15 iterations after the callback first returned nonzero.
 * resnorm_hist (may be NULL): termination-test residual norm of each pass
 * through the loop head, at most hist_cap entries (always a host pointer). */
typedef ipxint (*ipxk_interrupt_fn)(void* user);
int ipxk_pcr_solve(ipxk_context* ctx, const double* rhs, double tol,
                   const double* resscale, ipxint maxiter, double* lhs,
                   ipxint* iter, ipxint* errflag, ipxk_interrupt_fn interrupt,
                   void* interrupt_user, double* resnorm_hist, ipxint hist_cap,
                   ipxk_times* times);

/* numbers of the last CR run (any of ipxk_pcr_solve, ipxk_cr_solve, the KKT solves) */
int ipxk_cr_diagnostics(ipxk_context* ctx, ipxk_cr_diag* out);
/* what the last CR run put into the queue, counted on the host: out[0] iterations enqueued, out[1] launches of the
 * loop's own kernels (control, direction, the diagonal preconditioner, initialisation and tail; the kernels of the
 * operator and of the dense-column preconditioner are not counted), out[2] launches that hand a snapshot of `done`
 * to the host, out[3] events recorded inside the loop.  On a single GPU the host follows a progress word the
 * direction kernel stores: out[2] = out[3] = 0 and out[0] <= *iter + 1 + R with R the run-ahead (3 iterations;
 * IPXK_CR_AHEAD).  IPXK_CR_PACE=cycles selects the driver that partitioned systems keep: cycles of 5 iterations,
 * one snapshot and one event each. */
int ipxk_cr_loop_stats(ipxk_context* ctx, ipxint out[4]);

/* ---- KKTSolverDiag (src/kkt_solver_diag.h:23-49) ------------------------- */
/* _Factorize (src/kkt_solver_diag.cc:18-65).  xl == NULL is Factorize(nullptr)
 * (W = 1).  mu = iterate->mu().  Builds W, resscale, prepares the normal matrix
 * and factorizes the preconditioner. */
int ipxk_kkt_diag_factorize(ipxk_context* ctx, const double* xl,
                            const double* xu, const double* zl,
                            const double* zu, double mu,
                            int precond_dense_cols, ipxint* errflag);
/* _Solve (src/kkt_solver_diag.cc:82-118): a[n+m], b[m] -> x[n+m], y[m]. */
int ipxk_kkt_diag_solve(ipxk_context* ctx, const double* a, const double* b,
                        double tol, ipxint maxiter, double* x, double* y,
                        ipxint* iter, ipxint* errflag,
                        ipxk_interrupt_fn interrupt, void* interrupt_user,
                        ipxk_times* times);
/* copies W_[n+m] and resscale_[m] (host pointers; NULL skips) */
int ipxk_kkt_diag_get(const ipxk_context* ctx, double* W, double* resscale);

/* ---- SplittedNormalMatrix (src/splitted_normal_matrix.h:25-67) ----------- */
/* Prepare (src/splitted_normal_matrix.cc:18-66).  The hand-off from
 * Basis::GetLuFactors (src/basis.cc:162-166) is explicit: L (strictly lower,
 * no diagonal), U (upper, diagonal last in each column), rowperm, colperm with
 * B[rowperm,colperm] = (L+I)*U (src/lu_update.h:43-60); basis[p] = variable at
 * position p; status[n+m] in IPXK_*; colscale[n+m].  Row indices inside a column
 * may come in any order as long as U's diagonal is last; a dense trailing block of
 * the factors is cut out of the sweeps (and applied as a blocked solve or an
 * explicit inverse) only when the columns of U that cross it are sorted, as
 * GetLuFactors returns them.
 *
 * Column-partitioned context (ipxk_comm_init_columns; a row-partitioned one gets
 * IPXK_E_ARGUMENT): the basis path is collective, and every rank obtains the same
 * m-vectors bit for bit.
 *  - Replicated arguments: L, U, rowperm, colperm -- the factors of the GLOBAL B,
 *    from the host -- and basis[m] in the global numbering 0..n_global+m, the same
 *    on every rank.
 *  - Local arguments: status, colscale (and a, x of ipxk_kkt_basis_solve) in the
 *    partition's local form [this rank's structural slice; all m slack entries].
 *  - Slabs are contiguous and in rank order (rank r holds the global columns
 *    c0_r .. c0_r + n_r - 1 with c0_r = n_0 + ... + n_{r-1}); the first Prepare
 *    after ipxk_comm_init_columns learns c0 and n_global by one all-gather of n.
 *  - The ranks fail or proceed together: the argument checks end in one
 *    all-reduce of each rank's verdict and a fingerprint of the replicated
 *    arguments (factors, permutations, basis, slack parts of status and
 *    colscale).  A failed check on any rank, or fingerprints that differ, make
 *    every rank return IPXK_E_ARGUMENT.
 *  - Prepare and ipxk_split_rescale form the status and scale of every basis
 *    position from the owners' contributions (one all-reduce of 2m); N holds this
 *    rank's nonbasic structural columns.
 *  - ipxk_split_apply: U' and L' sweeps, this rank's N_g N_g' partial (the slack
 *    term on rank 0), one all-reduce of m, L and U sweeps.  The triangular solves
 *    (ipxk_forward_solve, ipxk_backward_solve, ipxk_solve_dense) run replicated
 *    and exchange nothing; ipxk_cr_solve exchanges once per Apply plus the
 *    max-reduce of its loop flags once per 5 iterations.
 *  - ipxk_kkt_basis_solve: three all-reduces of m (a[basis], the right-hand
 *    side product, b - N x_N) plus one per CR Apply.  x receives the entries this
 *    rank holds: its nonbasic and basic structural columns and all slacks.
 * An operator prepared under another partition is refused until prepared again. */
int ipxk_split_prepare(ipxk_context* ctx, const ipxint* Lp, const ipxint* Li,
                       const double* Lx, const ipxint* Up, const ipxint* Ui,
                       const double* Ux, const ipxint* rowperm,
                       const ipxint* colperm, const ipxint* basis,
                       const ipxint* status, const double* colscale);
/* Prepare when ONLY the scaling factors changed: KKTSolverBasis::_Factorize
 * keeps the factorization when the basis was not updated
 * (src/kkt_solver_basis.cc:59-64), and then all that differs for the operator is
 * the scaling of U's columns and of N and the free positions
 * (src/splitted_normal_matrix.cc:30-64).  Reuses the level schedule and the
 * packed factors of the last ipxk_split_prepare (same L, U, permutations and
 * basis) and rebuilds only what depends on status / colscale; the result is
 * bit-identical to a full ipxk_split_prepare with the same arguments.  Column
 * partition: collective (status / colscale local, their slack parts replicated;
 * the ranks agree on the verdict as in ipxk_split_prepare). */
int ipxk_split_rescale(ipxk_context* ctx, const ipxint* status,
                       const double* colscale);
/* ---- basis LU factorization on the device ------------------
 * The LuFactorization contract, src/lu_factorization.h:21-58:
 *     B[rowperm,colperm] = (L+I)*U
 * with L strictly lower (no diagonal stored), U upper with the diagonal last in
 * each column, indices sorted; dependent columns are replaced by unit columns in
 * the product and their positions in colperm are listed.  Replaces the kernel
 * behind BasicLuKernel::_Factorize (src/basiclu_kernel.cc:31-82, BASICLU); call
 * sites ForrestTomlin::_Factorize (src/forrest_tomlin.cc:28-30) and, through
 * LuUpdate::Factorize, Basis::Factorize (src/basis.cc:116-156).  Method: rounds of
 * column / row singletons, then the remaining bump as a dense matrix with partial
 * pivoting (any pivottol in (0,1] is therefore met inside the bump; a row
 * singleton must pass |a| >= pivottol * max|active column|).  Absolute pivot
 * tolerance: kLuDependencyTol = 1e-3 (src/ipx_internal.h:26) if
 * strict_abs_pivottol, else 1e-14.  A bump of more than IPXK_LU_BUMP_MAX rows
 * (environment, default 8192) is torn first: whenever the rounds stall, the
 * active columns with the most active entries are set aside as spikes and the
 * rounds go on; the spikes are carried through the row singleton pivots by a
 * forward substitution and end in a dense block of one row per spike
 * (bump-and-spike ordering; ipxk_lu_info.spikes; the spikes may number up to
 * 16384, the largest dense block the panel kernels take).  If that block would
 * exceed 16384 rows, the factorization starts again and eliminates the bump sparsely:
 * rounds of pivots of low Markowitz cost that form a diagonal block, under the
 * same absolute and relative pivot thresholds, the fill-in entering the current
 * matrix (ipxk_lu_info.sparse_pivots / sparse_rounds; environment IPXK_LU_SPARSE
 * = 1: from the start, = 0: never); what is left is factorized densely.
 * IPXK_E_UNSUPPORTED is returned only if that rest still exceeds the limit or
 * the elimination fills the bump beyond IPXK_LU_SPARSE_FILL_MAX (8) x nnz(B).
 * Columns of B are Bi/Bx[Bbegin[j] .. Bend[j]-1] (4-array form, as Basis passes
 * AI's arrays); indices need not be sorted.  The factors stay on the device;
 * ipxk_lu_get_factors copies them out (array sizes from ipxk_lu_info; any
 * pointer may be NULL). */
typedef struct {
  ipxint lnz, unz;          /* entries of L (no diagonal) and of U (with it) */
  ipxint num_dependent;     /* columns replaced by unit columns */
  ipxint col_singletons, row_singletons, bump, rounds;
  double seconds_singletons, seconds_bump, seconds_assemble;
  ipxint spikes;            /* columns torn off a bump beyond the dense limit (0: the bump
                               was factorized as it stood); then bump == spikes */
  ipxint sparse_pivots, sparse_rounds; /* pivots and rounds of the sparse elimination of a bump
                               beyond the dense limit (0: none) */
  ipxint reused;            /* 1: nothing was computed -- the context already held the factors of exactly
                               this matrix (the basis ipxk_lu_factorize_basis / ipxk_maxvolume factorized
                               last, columns in any order, same tolerances: Basis::Load after Maxvolume
                               on the device, src/basis.cc:81-114) and hands them out again */
} ipxk_lu_info;
int ipxk_lu_factorize(ipxk_context* ctx, ipxint dim, const ipxint* Bbegin,
                      const ipxint* Bend, const ipxint* Bi, const double* Bx,
                      double pivottol, int strict_abs_pivottol,
                      ipxk_lu_info* info);
/* Number of LU factorizations this context has COMPUTED so far (a reused one does not count): a caller that
 * keeps track of which basis the resident factors belong to (KKTSolverBasisHip) sees with it whether
 * another factorization went through the context in between. */
ipxint ipxk_lu_generation(const ipxk_context* ctx);
int ipxk_lu_get_factors(ipxk_context* ctx, ipxint* Lp, ipxint* Li, double* Lx,
                        ipxint* Up, ipxint* Ui, double* Ux, ipxint* rowperm,
                        ipxint* colperm, ipxint* dependent_cols);
/* B = AI[:, basis[0..m-1]] taken from the matrix resident in the context (slack
 * columns j >= n are unit columns): Basis::Factorize (src/basis.cc:116-156)
 * without B crossing PCIe -- only the m basis indices do.  Refused
 * (IPXK_E_ARGUMENT) on a partitioned context, as are ipxk_split_prepare_lu,
 * ipxk_maxvolume and ipxk_maxvolume_sequential: replicated factors must be the
 * same bit for bit on every rank; pass host factors to ipxk_split_prepare. */
int ipxk_lu_factorize_basis(ipxk_context* ctx, const ipxint* basis,
                            double pivottol, int strict_abs_pivottol,
                            ipxk_lu_info* info);
/* SplittedNormalMatrix::Prepare (src/splitted_normal_matrix.cc:18-66) on the
 * factors of the last ipxk_lu_factorize_basis, which never leave the device:
 * the GetLuFactors hand-off of src/basis.cc:162-166 without a host round trip.
 * Fails (IPXK_E_ARGUMENT) when that factorization found dependent columns: the
 * reference repairs the basis first (Basis::AdaptToSingularFactorization). */
int ipxk_split_prepare_lu(ipxk_context* ctx, const ipxint* status,
                          const double* colscale);
/* ---- Maxvolume on the device -------------------------------
 * Maxvolume::RunHeuristic (src/maxvolume.cc:108-153 with Driver :202-320,
 * ScaleFtran :322-337, FindLargest :179-200) over the part of ipx::Basis it
 * drives (SolveDense, SolveForUpdate, TableauRow, ExchangeIfStable,
 * src/basis.cc:162-330), followed by the tail of KKTSolverBasis::_Factorize
 * (src/kkt_solver_basis.cc:46-61): the split operator of the final basis -- from
 * a fresh factorization, or from the earlier factors with the last exchanges
 * behind them (kept_etas below).  Precondition: ipxk_lu_factorize_basis +
 * ipxk_split_prepare_lu for the current basis.  status / colscale: n+m entries
 * as for ipxk_split_prepare (BASIC_FREE variables never leave, NONBASIC_FIXED
 * ones never enter).  The factorization is kept current by product-form etas on
 * the resident factors and refactorized after max_etas exchanges or when an
 * exchange fails the stability test (the pivot from the tableau row against the
 * one from the tableau column, relative 1e-8).  On return basis_out[m] /
 * status_out[n+m] hold the new basis (either may be NULL), the context the
 * operator for it (by a fresh factorization, src/kkt_solver_basis.cc:56-61, or -- when that would cost more than
 * carrying the last exchanges through the solves that follow, a fixed cost model -- by the earlier factors with the
 * exchanges as a product form behind them: info.kept_etas; IPXK_MAXVOL_KEEP_ETAS=0 in the environment: always fresh), exchange_log (may be NULL) the accepted exchanges as pairs
 * (leaving variable, entering variable), at most log_cap of them.
 * info.errflag: 0, or IPX_ERROR_basis_too_ill_conditioned (306). */
typedef struct {
  double volume_tol;        /* ipx_parameters.volume_tol, default 2.0 */
  ipxint maxskip_updates;   /* default 10 */
  ipxint rows_per_slice;    /* default 10000 */
  ipxint max_etas;          /* exchanges between refactorizations, default (0) 100; < 0: as many as pay -- a
                               refactorization when the etas since the last one have cost as much as it
                               costs (a fixed cost model, not the clock: the run stays reproducible),
                               at least 100, at most 1024 or what 2 GiB of dense etas hold */
} ipxk_maxvolume_params;
typedef struct {
  ipxint updates, skipped, slices;   /* Maxvolume::updates() / skipped() / slices() */
  ipxint refused;                    /* exchanges refused as unstable (then refactorized) */
  ipxint factorizations;             /* refactorizations, the final one (if any: kept_etas) included */
  ipxint errflag;
  double volinc;                     /* Maxvolume::volinc(): log2 of the volume gained */
  double seconds;
  ipxint kept_etas;                  /* > 0: no final refactorization -- the context holds the factors of an earlier basis and
                                        this many etas (product form) behind them, which every solve and operator application
                                        of the context applies, and the next ipxk_maxvolume goes on with; any factorization
                                        in the context (ipxk_lu_factorize*, ipxk_split_prepare*) ends that state */
} ipxk_maxvolume_info;
int ipxk_maxvolume(ipxk_context* ctx, const ipxint* status, const double* colscale,
                   const ipxk_maxvolume_params* params, ipxint* basis_out,
                   ipxint* status_out, ipxk_maxvolume_info* info,
                   ipxint* exchange_log, ipxint log_cap);
/* Maxvolume::RunSequential (src/maxvolume.cc:14-106), the variant KKTSolverBasis
 * selects for update_heuristic == 0 (src/kkt_solver_basis.cc:47-51): passes over
 * the NONBASIC columns in decreasing order of their scaling factor; per candidate
 * the tableau column (SolveForUpdate) and the largest scaled entry
 * |x_p| * invscale_basic[p] * colscale[j]; an exchange when it exceeds
 * max(volume_tol, 1), checked like ipxk_maxvolume's (the BTRAN of the leaving
 * variable that ExchangeIfStable computes for sys = -1 gives the pivot from the
 * row).  maxpasses < 0: until a pass brings no update (the reference's default).
 * Same preconditions, outputs and final refactorization + Prepare as
 * ipxk_maxvolume; info->slices reports the number of passes.  A candidate costs
 * two sweeps over all m unknowns on the device (the reference's solves are
 * hypersparse): meant for moderate sizes, the heuristic is the one for 1M rows. */
int ipxk_maxvolume_sequential(ipxk_context* ctx, const ipxint* status,
                              const double* colscale, double volume_tol,
                              ipxint maxpasses, ipxint max_etas, ipxint* basis_out,
                              ipxint* status_out, ipxk_maxvolume_info* info,
                              ipxint* exchange_log, ipxint log_cap);
/* _Apply (src/splitted_normal_matrix.cc:90-117); column partition: rhs, lhs
 * replicated m-vectors, one all-reduce of m (see ipxk_split_prepare) */
int ipxk_split_apply(ipxk_context* ctx, const double* rhs, double* lhs,
                     double* rhs_dot_lhs);
/* ForwardSolve / BackwardSolve with the prepared (scaled) factors, in place
 * (src/sparse_matrix.cc:303-311). */
int ipxk_forward_solve(ipxk_context* ctx, double* x);
int ipxk_backward_solve(ipxk_context* ctx, double* x);
/* Basis::SolveDense on the fresh unscaled factors (src/basis.cc:168-170) */
int ipxk_solve_dense(ipxk_context* ctx, const double* rhs, double* lhs,
                     char trans);
/* number of level sets of the four triangular sweeps (U', L', L, U) */
int ipxk_split_levels(const ipxk_context* ctx, ipxint levels[4]);
/* Plain CR (src/conjugate_residuals.cc:14-88) on the prepared split operator */
int ipxk_cr_solve(ipxk_context* ctx, const double* rhs, double tol,
                  const double* resscale, ipxint maxiter, double* lhs,
                  ipxint* iter, ipxint* errflag, ipxk_interrupt_fn interrupt,
                  void* interrupt_user, double* resnorm_hist, ipxint hist_cap,
                  ipxk_times* times);

/* ---- KKTSolverBasis::_Solve (src/kkt_solver_basis.cc:75-194) -------------
 * Column partition: a[n+m], x[n+m] local, b, y replicated (see ipxk_split_prepare);
 * also in the device-pointer (resident) form. */
int ipxk_kkt_basis_solve(ipxk_context* ctx, const double* a, const double* b,
                         double tol, ipxint maxiter, double* x, double* y,
                         ipxint* iter, ipxint* errflag,
                         ipxk_interrupt_fn interrupt, void* interrupt_user,
                         ipxk_times* times);

/* ---- IPM::SolveNewtonSystem (src/ipm.cc:532-645), SURVEY.md section 8f row 3 ----
 * Builds the KKT right-hand side from the residuals rb[m], rc/rl/ru[n+m] (any of
 * these four may be NULL = zero) and the complementarity targets sl/su[n+m],
 * solves with the factorized diag solver (use_basis = 0) or the prepared basis
 * solver (use_basis = 1) to tol, and recovers the Newton step dx, dxl, dxu, dzl,
 * dzu [n+m], dy [m].  xl, xu, zl, zu are the iterate's vectors, state[n+m] the
 * IPXK_STATE_* codes.  With device pointers nothing crosses PCIe.  On errflag != 0
 * the step vectors are undefined (ipm.cc:571-573 returns).
 * Column partition (ipxk_comm_init_columns): rb, dy replicated, every (n+m)-vector
 * local [this rank's structural slice; all m slack entries]; collectives are those
 * of the KKT solve only.  A row-partitioned context is refused (IPXK_E_ARGUMENT). */
int ipxk_newton_solve(ipxk_context* ctx, int use_basis, const double* rb,
                      const double* rc, const double* rl, const double* ru,
                      const double* sl, const double* su, const double* xl,
                      const double* xu, const double* zl, const double* zu,
                      const unsigned char* state, double tol, ipxint maxiter,
                      double* dx, double* dxl, double* dxu, double* dy,
                      double* dzl, double* dzu, ipxint* iter, ipxint* errflag,
                      ipxk_interrupt_fn interrupt, void* interrupt_user,
                      ipxk_times* times);

/* ---- the IPM iterate on the device -----------
 * Iterate::Initialize / accessors (src/iterate.cc:60-92): the six vectors
 * x, xl, xu, zl, zu [n+m], y [m] and one IPXK_STATE_* byte per variable are
 * copied into the context.
 * Column partition (ipxk_comm_init_columns): the (n+m)-vectors and state are
 * local [this rank's structural slice; all m slack entries], y is replicated.
 * The scalars of the calls below (residual norms, complementarity, objectives,
 * the step lengths and the driver's decisions) are global and bitwise the same
 * on every rank; with one rank they equal the unpartitioned context's.  Each rank
 * reduces its own entries, one all-gather carries the per-rank values, every rank
 * combines them in rank order; the slack terms and b'y count on rank 0 only.
 * ipxk_iterate_set is collective there: one all-reduce carries each rank's
 * verdict and a fingerprint of y and the slack parts of x, xl, xu, zl, zu and
 * state; if any rank's arguments are wrong or they differ, every rank fails
 * with IPXK_E_ARGUMENT.
 * A variable in IPXK_STATE_IMPLIED_LB / IMPLIED_UB must meet what Iterate::assert_consistency
 * (src/iterate.cc:500-513) asks of the iterate's own vectors: xl = xu = inf and zl, zu >= 0 (the bound it
 * is implied at must be finite; the call does not see the bounds).  Otherwise IPXK_E_ARGUMENT, the first
 * offending index in the message.  An iterate without those states is copied unchecked, as before. */
int ipxk_iterate_set(ipxk_context* ctx, const double* x, const double* xl,
                     const double* xu, const double* y, const double* zl,
                     const double* zu, const unsigned char* state);
/* copies out; NULL pointers are skipped */
int ipxk_iterate_get(ipxk_context* ctx, double* x, double* xl, double* xu,
                     double* y, double* zl, double* zu);
/* the IPXK_STATE_* byte of every variable, state[n+m] (host memory): what ipxk_iterate_set was given, as
 * ipxk_ipm_starting_basis and the drop procedures (ipxk_ipm_drop_degenerate) have changed it */
int ipxk_iterate_get_state(ipxk_context* ctx, unsigned char* state);
/* Iterate::Update (src/iterate.cc:94-139): x += sp*dx on non-fixed variables,
 * xl/xu += sp*d, zl/zu += sd*d on variables with that barrier term, truncated
 * at kBarrierMin = 1e-30; y += sd*dy.  NULL step components are skipped. */
int ipxk_iterate_update(ipxk_context* ctx, double sp, const double* dx,
                        const double* dxl, const double* dxu, double sd,
                        const double* dy, const double* dzl, const double* dzu);
/* Iterate::ComputeResiduals (src/iterate.cc:536-588) for the model vectors
 * b[m], c, lb, ub [n+m]: rb = b - AI x, rc = c - AI'y - zl + zu (0 on fixed
 * variables), rl = lb - x + xl, ru = ub - x - xu (0 without that barrier
 * term); presidual = max(|rb|,|rl|,|ru|)_inf, dresidual = |rc|_inf.
 * Column partition: b, rb replicated, c, lb, ub, rc, rl, ru local; one
 * all-reduce of m (rb) and one all-gather of 2 per rank.  Row partition: refused. */
int ipxk_iterate_residuals(ipxk_context* ctx, const double* b, const double* c,
                           const double* lb, const double* ub, double* rb,
                           double* rc, double* rl, double* ru,
                           double* presidual, double* dresidual);
/* Iterate::ComputeComplementarity (src/iterate.cc:642-670):
 * out4 = {complementarity, mu, mu_min, mu_max} (host memory).  Column partition:
 * global, one all-gather of 4 per rank (row partition: this rank's terms only). */
int ipxk_iterate_complementarity(ipxk_context* ctx, double out4[4]);
/* StepToBoundary (src/ipm.cc:320-339): largest alpha <= alpha0 with
 * x + alpha*dx >= 0, damped by 1 - eps at the blocking index (-1: none).
 * Parallel minimum over the candidates; equals the reference's sequential
 * scan except when alpha lands within one ulp factor of another candidate.
 * A generic vector primitive: rank-local on a partitioned context (no
 * collective; the index is local).  ipxk_ipm_step takes the global form. */
int ipxk_step_to_boundary(ipxk_context* ctx, const double* x, const double* dx,
                          ipxint len, double alpha0, double* alpha,
                          ipxint* blocking_index);

/* One predictor-corrector step on the resident iterate: IPM::Predictor,
 * AddCorrector, StepSizes and MakeStep (src/ipm.cc:340-530) with the factorized
 * diag solver (use_basis = 0) or the prepared basis solver (1); KKT tolerance
 * kkt_tol*sqrt(mu) (src/ipm.cc:572, ipx_parameters::kkt_tol = 0.3).  The caller
 * factorizes for the current iterate first, as IPM::Driver does
 * (ipxk_iterate_factorize_diag for the diag solver).  b[m], c, lb, ub [n+m]
 * are the model's vectors.  On errflag != 0 (from a KKT solve) the iterate is
 * left unchanged.
 * Column partition: b replicated, c, lb, ub local; use_basis = 1 after
 * ipxk_split_prepare with replicated host factors.  Every field of info is the
 * same on every rank.  Collectives besides the two KKT solves: one all-reduce of
 * m (rb), then all-gathers of per-rank rows: 6 (residual norms, complementarity),
 * 24 twice (the four step-to-boundary problems: alpha, global blocking index
 * c0 + j or n_global + i, and x, dx, z, dz there; the first gives the
 * lexicographic minimum of (alpha, index), the reference's first-index rule),
 * 1 twice (complementarity at the trial point), 4 (mu after the step); the first
 * call also learns the column offsets (one all-gather of 1).  Row partition:
 * refused. */
typedef struct ipxk_ipm_step_info {
    double step_primal, step_dual;   /* IPM::step_primal_, step_dual_ */
    double mu_before, mu_after;      /* Iterate::mu() before / after the update */
    double sigma;                    /* centering parameter of the corrector */
    double presidual, dresidual;     /* of the iterate the step started from */
    ipxint kktiter_predictor, kktiter_corrector;
    ipxint errflag;
} ipxk_ipm_step_info;
int ipxk_ipm_step(ipxk_context* ctx, int use_basis, const double* b,
                  const double* c, const double* lb, const double* ub,
                  double kkt_tol, ipxint maxiter, ipxk_ipm_step_info* info,
                  ipxk_interrupt_fn interrupt, void* interrupt_user);
/* KKTSolverDiag::_Factorize (src/kkt_solver_diag.cc:18-65) for the resident
 * iterate: nothing crosses PCIe. */
int ipxk_iterate_factorize_diag(ipxk_context* ctx, int precond_dense_cols,
                                ipxint* errflag);

/* Iterate::ComputeObjectives (src/iterate.cc:590-640) of the resident iterate for
 * the model vectors: out3 = {pobjective, dobjective, offset}; pobjective + offset
 * and dobjective + offset are the objectives after postprocessing (:203-211).
 * Variable states as in ipxk_iterate_set; a variable in IPXK_STATE_IMPLIED_LB / IMPLIED_UB
 * moves (zl - zu) x from pobjective to offset (:621-626).  On a postprocessed iterate
 * (ipxk_iterate_postprocess) it is the other branch (:599-609): pobjective = c'x,
 * dobjective = b'y + sum lb zl - sum ub zu over the finite bounds, offset = 0.
 * Column partition: global, one
 * all-gather of 4 per rank (offset and the fixed structural x_j A_j'y included).
 * Row partition: refused. */
int ipxk_iterate_objectives(ipxk_context* ctx, const double* b, const double* c,
                            const double* lb, const double* ub, double out3[3]);

/* IPM::Driver (src/ipm.cc:56-123) on the resident iterate with the diag solver:
 * loop of {termination test (Iterate::term_crit_reached, src/iterate.cc:221-249,
 * with the crossover_start of ipxk_ipm_set_crossover_start, 0 unless set: a positive
 * value adds the dropping residuals to the test, on a column partition with one more
 * all-gather of 2 at a feasible and optimal iterate), divergence / bad-iteration
 * test (:71-93), iteration
 * limit, InterruptCheck, KKTSolverDiag::Factorize, Predictor + AddCorrector +
 * MakeStep}.  status_ipm uses the values of include/ipx_status.h
 * (IPX_STATUS_optimal 1, primal_infeas 3, dual_infeas 4, time_limit 5,
 * iter_limit 6, no_progress 7, failed 8).  A CR failure of the diag solver ends
 * the loop with IPX_STATUS_failed and the CR errflag: that is where LpSolver
 * switches to the basis solver (src/lp_solver.cc:399-418), the caller's move.
 * Column partition: b replicated, c, lb, ub local (ipxk_iterate_set's forms).
 * At entry one all-reduce carries each rank's verdict and a fingerprint of b and
 * the slack parts of c, lb, ub (mismatch: IPXK_E_ARGUMENT on every rank).  Every
 * decision is taken from replicated scalars, and interrupt(user) is agreed once
 * per iteration (max over the ranks), so all ranks return the same info in the
 * same iteration.  Per iteration besides the KKT factorize and solves: one
 * all-reduce of m, all-gathers of 10, 24, 1, 24, 1, 4 doubles per rank and one
 * all-reduce (max) of 1.  Row partition: refused. */
typedef struct ipxk_ipm_params {
    double kkt_tol;            /* ipx_parameters::kkt_tol, 0.3 */
    double feasibility_tol;    /* ipm_feasibility_tol, 1e-6 */
    double optimality_tol;     /* ipm_optimality_tol, 1e-8 */
    ipxint kkt_maxiter;        /* CR iteration cap of the diag solver (src/lp_solver.cc:393) */
    ipxint ipm_maxiter;        /* ipm_maxiter, 300 */
    int precond_dense_cols;
} ipxk_ipm_params;
typedef struct ipxk_ipm_info {
    ipxint status_ipm, iter, errflag, kktiter;
    double pobjective, dobjective;       /* after postprocessing */
    double presidual, dresidual, complementarity, mu;
    double step_primal, step_dual;       /* of the last step */
    ipxint basis_updates;                /* ipxk_ipm_driver_basis: exchanges by Maxvolume (Info::updates_ipm) */
} ipxk_ipm_info;
int ipxk_ipm_driver(ipxk_context* ctx, const double* b, const double* c,
                    const double* lb, const double* ub,
                    const ipxk_ipm_params* params, ipxk_ipm_info* info,
                    ipxk_interrupt_fn interrupt, void* interrupt_user);

/* IPM::ComputeStartingPoint (src/ipm.cc:125-259) on the device, into the resident
 * iterate: KKTSolverDiag::Factorize(nullptr) (G = I); x = clamp(0, lb, ub) and the
 * first KKT solve (a = 0, rhs b - AI x, tol 0.1 |rb|_inf), x += dx; xl = x - lb,
 * xu = ub - x shifted by 1 + 1.5 xinfeas; if |c|_2 = 0, zl, zu = 1 or 0 by bound
 * finiteness, else the second solve (a = c, rhs 0, tol 0.1 |c|_inf), zl = c - AI'y,
 * zl += 0.05 c and y *= 0.95 if |zl|_2 < 0.05 |c|_2, the split into zl, zu by the
 * bounds shifted by 1 + 1.5 zinfeas; then the leveling shifts (:226-251).  The states
 * follow Iterate::Initialize (src/iterate.cc:76-88; lb == ub gives BARRIER_BOXED),
 * so ipxk_ipm_driver can be called right after.  b[m], c, lb, ub [n+m] in the forms of
 * ipxk_ipm_driver; of params only kkt_maxiter (-1: m + 100) and precond_dense_cols
 * are read.  NULL arguments, lb > ub, lb = +inf, ub = -inf and NaNs in b, c, lb, ub
 * are refused (IPXK_E_ARGUMENT, the first such index in the message).
 * info: status_ipm as ipm.cc:31-41 (errflag 999 from the interrupt: IPX_STATUS_time_limit
 * 5 and errflag 0; any other errflag: IPX_STATUS_failed 8 with the errflag; else
 * IPX_STATUS_not_run 0); kktiter = CR iterations of both solves; presidual,
 * dresidual, complementarity, mu, pobjective, dobjective of the resulting point; the
 * other fields 0.  An errflag from the factorization or a solve leaves the point of
 * the Iterate constructor (src/iterate.cc:31-57: x = 0, y = 0, xl / xu / zl / zu =
 * 1 / inf / 0 by bound kind), as LpSolver expects (src/lp_solver.cc:377-379).  The
 * interrupt is checked as in ipxk_kkt_diag_solve.  Every reduction is a fixed-order
 * sum of block partials: two calls on the same inputs give the same bits.
 * Column partition: collective.  One all-reduce carries each rank's verdict and the
 * fingerprint of b and the slack parts of c, lb, ub (as ipxk_ipm_driver; mismatch:
 * IPXK_E_ARGUMENT on every rank).  Besides the factorization, the two KKT solves and
 * the evaluation of the point (as one driver iteration's: one all-reduce of m and one
 * all-gather of 10): one all-reduce of m (rb), all-gathers of 3 (xinfeas, |c|^2,
 * |c|_inf), 1 (|zl|^2), 1 (zinfeas) and 3 (the leveling sums) doubles per rank (the
 * second and third are skipped when c = 0).  Slack terms count on rank 0 only, so one
 * rank reproduces the unpartitioned context bit for bit.  Row partition: refused. */
int ipxk_ipm_starting_point(ipxk_context* ctx, const double* b, const double* c,
                            const double* lb, const double* ub,
                            const ipxk_ipm_params* params, ipxk_ipm_info* info,
                            ipxk_interrupt_fn interrupt, void* interrupt_user);
/* IPM::LoadStartingPoint (src/ipm.cc:261-316): the caller's point x, xl, xu, zl, zu
 * [n+m], y [m] becomes the resident iterate after repair.  It must be valid, as the
 * reference asserts: at a finite bound xl (xu) and zl (zu) finite and nonnegative, at
 * an infinite one xl (xu) = inf and zl (zu) = 0; otherwise IPXK_E_ARGUMENT with the
 * first offending index.  mu = the mean of the products with both factors > 0 (1.0 if
 * there are none); a pair with both entries 0 becomes sqrt(mu), sqrt(mu), one zero
 * entry becomes mu over the other.  States as Iterate::Initialize.
 * Column partition: forms of ipxk_iterate_set; collective.  One all-reduce carries
 * each rank's verdict and a fingerprint of y and the slack parts of x, xl, xu, zl,
 * zu, lb, ub, one all-gather of 2 the sum and the count (slack pairs on rank 0). */
int ipxk_ipm_load_starting_point(ipxk_context* ctx, const double* x,
                                 const double* xl, const double* xu,
                                 const double* y, const double* zl,
                                 const double* zu, const double* lb,
                                 const double* ub);

/* The main IPM phase (LpSolver::RunMainIPM, src/lp_solver.cc:456-462): IPM::Driver around KKTSolverBasis.
 * Every iteration's KKTSolverBasis::_Factorize (src/kkt_solver_basis.cc:20-63) runs on the device: scaling
 * factors from the resident iterate (Iterate::ScalingFactor, src/iterate.cc:183-198),
 * DropPrimal / DropDual when a drop tolerance is positive (ipxk_ipm_set_drop_tolerances below; :36-43, off by
 * default), Maxvolume (ipxk_maxvolume), fresh factorization, Prepare; then the predictor-corrector step with the
 * basis-preconditioned solves.  The starting basis is the slack basis (ConstructBasisFromWeights with
 * crash_basis = 0, src/basis.cc:353-385).  Models whose
 * iterate holds free or fixed variables are refused (IPXK_E_UNSUPPORTED) when the phase has to build the slack
 * basis -- not when the context holds a live
 * starting basis (ipxk_ipm_starting_basis below): then the phase starts from that basis and its four-valued
 * statuses instead, BASIC_FREE and NONBASIC_FIXED persist through Maxvolume and Prepare, and the scaling
 * factors 0 / inf of fixed / free variables are taken as they are; nor in a later iteration, whose basis may
 * hold the variables the drop procedures have fixed or implied.  basis_out[m] / status_out[n+m]
 * (either may be NULL) return the final basis.  params->kkt_maxiter is ignored (KKTSolverBasis runs CR with
 * maxiter = -1).  The termination test is ipxk_ipm_driver's, crossover_start included; a postprocessed iterate is
 * refused by both drivers.  Limits of the refactorizations: see ipxk_lu_factorize (dense bump).  Refused on any partitioned
 * context (it needs the device LU and Maxvolume). */
int ipxk_ipm_driver_basis(ipxk_context* ctx, const double* b, const double* c,
                          const double* lb, const double* ub,
                          const ipxk_ipm_params* params, ipxk_ipm_info* info,
                          ipxint* basis_out, ipxint* status_out,
                          ipxk_interrupt_fn interrupt, void* interrupt_user);

/* StartingBasis (src/starting_basis.cc:128-185) for crash_basis = 0 on the resident iterate: what LpSolver
 * calls between the diag iterations and the main phase (src/lp_solver.cc:420-454).
 *   1. Weights: Iterate::ScalingFactor per variable (src/iterate.cc:183-198), 0 where lb == ub.  A free
 *      variable must have weight inf and every other one a finite weight, as the reference asserts
 *      (IPXK_E_ARGUMENT otherwise).
 *   2. Basis::ConstructBasisFromWeights (src/basis.cc:353-385) from the slack basis:
 *      PivotFreeVariablesIntoBasis (:676-781) and PivotFixedVariablesOutOfBasis (:783-930) with their
 *      stability swaps (> 4.0 against < 1.0), the dependency test (<= dependency_tol), the unbounded primal
 *      / dual ray tests that set cols_inconsistent / rows_inconsistent, the volume-maximizing choice among
 *      the stable pivots (>= 0.1 of the largest), and Basis::ExchangeIfStable (:286-321): an exchange whose
 *      pivot from the row and from the column differ by more than 1e-8 relative is refused, the pivot
 *      tolerance tightened (Basis::TightenLuPivotTol) and the basis refactorized.  Per candidate one
 *      tableau column and one tableau row (two sweeps each over all m unknowns); the exchanges are kept as
 *      product-form etas behind the factors (max_etas as in ipxk_maxvolume_sequential) and one block of
 *      scalars per candidate reaches the host.
 *   3. starting_basis.cc:153-173: basic variables of weight 0 / inf become BASIC_FREE, nonbasic ones
 *      NONBASIC_FIXED; a lb == ub variable that ended NONBASIC_FIXED is fixed in the iterate (x = lb,
 *      xl = xu = zl = zu = 0, IPXK_STATE_FIXED).
 *   4. PostprocessDependencies (:52-126): dependent free columns are fixed at 0 with the basic variables
 *      moved so that AI x is unchanged; the y_i of dependent equality rows go to 0 without altering AI'y
 *      and their slacks become implied (xl = xu = inf, zl = zu = 0, IPXK_STATE_FREE).
 * On return the context holds a fresh factorization of the starting basis and its operator, and
 * ipxk_ipm_driver_basis goes on from them ("live starting basis"); ipxk_iterate_set,
 * ipxk_ipm_starting_point, ipxk_ipm_load_starting_point and ipxk_reset_solver_state end that state.
 * b[m], c, lb, ub [n+m] in the forms of ipxk_ipm_driver.  params may be NULL (dependency_tol 1e-6,
 * include/ipx_parameters.h:68; max_etas 0 = 100).  basis_out[m], status_out[n+m] (IPXK_BASIC* / IPXK_NONBASIC*)
 * and exchange_log (pairs jb, jn of the first log_cap exchanges, info->updates_start of them) may be NULL.
 * What an inconsistent flag means is the caller's decision (src/lp_solver.cc:437-450).  info->errflag: 999
 * from the interrupt (polled once per candidate), 301 / 306 from a refactorization (singular / too ill
 * conditioned); then the iterate is unchanged and no starting basis is live.  Every reduction is a
 * fixed-order tree over block partials with ties to the lowest index: two calls from the same iterate
 * give the same bits.  Refused on any partitioned context (it needs the device LU). */
typedef struct {
    double dependency_tol;     /* dependency_tol, 1e-6; negative values count as 0 */
    ipxint max_etas;           /* as ipxk_maxvolume_sequential */
} ipxk_starting_basis_params;
typedef struct {
    ipxint errflag;
    ipxint dependent_rows, dependent_cols;         /* Info::dependent_rows / dependent_cols */
    ipxint rows_inconsistent, cols_inconsistent;   /* Info::rows_inconsistent / cols_inconsistent (0 / 1) */
    ipxint updates_start;                          /* Info::updates_start: exchanges */
    ipxint stability_pivots;                       /* of them: swaps of two free / two fixed variables */
    ipxint factorizations;                         /* the slack basis and the final basis included */
    double seconds;
} ipxk_starting_basis_info;
int ipxk_ipm_starting_basis(ipxk_context* ctx, const double* b, const double* c,
                            const double* lb, const double* ub,
                            const ipxk_starting_basis_params* params,
                            ipxk_starting_basis_info* info, ipxint* basis_out,
                            ipxint* status_out, ipxint* exchange_log, ipxint log_cap,
                            ipxk_interrupt_fn interrupt, void* interrupt_user);

/* ---- KKTSolverBasis::DropPrimal / DropDual (src/kkt_solver_basis.cc:36-43, 196-387) --------------------------
 * Control::ipm_drop_primal / ipm_drop_dual for ipxk_ipm_driver_basis, ipxk_ipm_solve and ipxk_lp_solve: with a
 * positive tolerance every Factorize of the main phase first takes nearly degenerate variables out of the barrier
 * problem (below).  0, 0 (the default, restored by ipxk_reset_solver_state): off, the phase runs as it did without
 * them.  Negative or non-finite values: IPXK_E_ARGUMENT.  (The reference's default is 1e-9 for both.) */
int ipxk_ipm_set_drop_tolerances(ipxk_context* ctx, double drop_primal, double drop_dual);
/* One DropPrimal + DropDual pass on the resident iterate and the context's live basis, with the tolerances set
 * above: what KKTSolverBasis::_Factorize does between the scaling factors and Maxvolume.
 *   Gate (:36): nothing happens unless pobjective >= dobjective (without the offset, as ipxk_iterate_objectives
 *     returns them); the model vectors b[m], c, lb, ub [n+m] are read for it alone.
 *   DropPrimal: the candidates are the BASIC variables whose distance xj to the nearer bound and its dual zj have
 *     xj < 0.01 zj and xj <= drop_primal, taken from the back of the list in position order.  Per candidate jb at
 *     position p: the tableau row r = AI' inverse(B') e_p over the NONBASIC columns and the arg max of
 *     |r_j| colscale_j / colscale_jb among |r_j| > 1e-7 (kPivotZeroTol) with a value > 2.0 (volume_tol), both strict,
 *     ties to the lowest j -- one fused pass over the matrix, the row is never stored.  A winner jmax is exchanged for
 *     jb (Basis::ExchangeIfStable with the pivot from the FTRAN of jmax; a refused exchange refactorizes and tries
 *     the candidate again); without one jb becomes implied at lb (zl/xl > zu/xu) or at ub (IPXK_STATE_IMPLIED_*,
 *     xl = xu = inf, zl, zu kept), BASIC_FREE, scaling factor inf.
 *   DropDual: the candidates are the NONBASIC variables whose larger dual zj and its xj have zj < 0.01 xj and
 *     zj <= drop_dual, from the back of the ascending list.  Per candidate jn: the tableau column and the arg max of
 *     |lhs_p| colscale_jn / colscale_basis[p] under the same two thresholds (a BASIC_FREE position never wins).  A
 *     winner is exchanged (pivot from the BTRAN against the one from the column); without one jn is fixed at its
 *     value (IPXK_STATE_FIXED, xl = xu = zl = zu = 0), NONBASIC_FIXED, scaling factor 0.
 * When a screening kernel finds no candidate, only its count reaches the host and nothing else is launched.  Every
 * reduction is a fixed-order tree with ties to the lowest index: two calls from the same state give the same bits.
 * Requires a live starting basis (ipxk_ipm_starting_basis) or the basis ipxk_ipm_driver_basis ended with, whose
 * factors are still the context's; otherwise IPXK_E_ARGUMENT.  Afterwards that basis is the one returned here, with
 * fresh factors and its operator.  basis_out[m], status_out[n+m] may be NULL; so may colscale_out[n+m] (host memory), which
 * receives the scaling factors Maxvolume would go on with: Iterate::ScalingFactor of every variable, read back from the device
 * after the pass, with the inf of the implied and the 0 of the fixed variables as the deciding kernels wrote them.  log receives triples {variable, action, partner} of
 * the first log_cap decisions (3 log_cap entries): action 0 exchanged (partner: the variable it was exchanged with), 1 implied at lb, 2 implied at ub,
 * 3 fixed (partner -1).  info->errflag: 301 / 306 from a refactorization, 999 (or the callback's value) from the
 * interrupt, polled once per candidate; variables already dropped stay dropped, as in the reference, and after an interrupt
 * the context holds the factors and the operator of the basis returned.  A call that ends with an errflag leaves no live
 * basis (the next one is refused until ipxk_ipm_starting_basis or ipxk_ipm_driver_basis has run again); so does an
 * ipxk_ipm_driver_basis that ends inside a Factorize.
 * Refused on any partitioned context and on a postprocessed iterate. */
typedef struct ipxk_drop_info {
    ipxint errflag;
    ipxint primal_candidates, dual_candidates;   /* of the two screenings */
    ipxint primal_dropped, dual_dropped;         /* Info::primal_dropped / dual_dropped of this pass */
    ipxint updates;                              /* exchanges (they count into Info::updates_ipm) */
    ipxint refused;                              /* exchanges refused as unstable */
    ipxint factorizations;
    double seconds;
} ipxk_drop_info;
int ipxk_ipm_drop_degenerate(ipxk_context* ctx, const double* b, const double* c, const double* lb, const double* ub,
                             ipxk_drop_info* info, ipxint* basis_out, ipxint* status_out, double* colscale_out,
                             ipxint* log, ipxint log_cap, ipxk_interrupt_fn interrupt, void* interrupt_user);
/* Sums over the Factorizes since the last ipxk_ipm_driver_basis / ipxk_ipm_solve / ipxk_lp_solve began
 * (Info::primal_dropped, Info::dual_dropped and the exchanges of the drop procedures, which ipxk_ipm_info::basis_updates
 * includes as Info::updates_ipm does).  Any pointer may be NULL. */
int ipxk_ipm_drop_counts(const ipxk_context* ctx, ipxint* primal_dropped, ipxint* dual_dropped, ipxint* drop_updates);

/* ---- the end of the solve (src/lp_solver.cc:305-332, src/iterate.cc:237-448) -------------------------------
 * Iterate::Postprocess (src/iterate.cc:250-313) on the resident iterate for the model vectors c, lb, ub [n+m].
 * The reference's StateDetail is derived from the device states and the bounds: IPXK_STATE_FIXED is FIXED;
 * IPXK_STATE_FREE with finite lb == ub is IMPLIED_EQ (the slacks of dependent equality rows after
 * ipxk_ipm_starting_basis); IPXK_STATE_FREE otherwise is FREE; IPXK_STATE_IMPLIED_LB / IMPLIED_UB are themselves.
 *   fixed:      xl = x - lb, xu = ub - x (inf at an infinite bound); if lb == ub, z = c_j - a_j'y goes to zl
 *               (z >= 0) or to zu as -z.
 *   implied eq: z goes to zl or zu by sign, the other one is 0; x = lb, xl = xu = 0.
 *   implied lb: zl = z, zu = 0, x = lb;  implied ub: zl = 0, zu = -z, x = ub;  then xl = x - lb, xu = ub - x
 *               (:294-308).
 * Only those variables are written; when a count on the device finds none, nothing else is launched and the
 * iterate keeps its bits.  The products a_j'y come from one pass over the column gather matrix.
 * Afterwards the iterate is "postprocessed" until ipxk_iterate_set, ipxk_ipm_starting_point,
 * ipxk_ipm_load_starting_point or ipxk_reset_solver_state: ipxk_iterate_residuals keeps rc on fixed variables
 * (:552-556), ipxk_iterate_objectives takes the postprocessed branch (:599-609), and every call that advances
 * the iterate (ipxk_iterate_update, ipxk_ipm_step, ipxk_ipm_driver, ipxk_ipm_driver_basis,
 * ipxk_ipm_starting_basis) is refused with IPXK_E_ARGUMENT.
 * Column partition: c, lb, ub local; no collective (every rule is column-local, y is replicated).  Row
 * partition: refused. */
int ipxk_iterate_postprocess(ipxk_context* ctx, const double* c, const double* lb,
                             const double* ub);
/* Iterate::ResidualsFromDropping (src/iterate.cc:393-448): out2 = {pres, dres} (host memory), the primal and
 * dual residuals that dropping every barrier variable to its bound or its dual to zero would introduce.  The
 * per-column max |a_ij| (1 for slack columns) is computed on the device at the first call and kept with the
 * context.  Fixed-order max over block partials.  Column partition: lb, ub local; one all-gather of 2 per rank
 * (max; slack terms on rank 0).  Row partition: refused. */
int ipxk_iterate_dropping_residuals(ipxk_context* ctx, const double* lb, const double* ub,
                                    double out2[2]);
/* Iterate::crossover_start_ for both drivers (ipx_parameters::crossover_start, 1e-8 in the reference when
 * crossover is on).  0 (the default, restored by ipxk_reset_solver_state): a feasible and optimal iterate ends
 * the loop.  Positive: it does so only if the dropping residuals are within value*(1 + norm_bounds) and
 * value*(1 + norm_c) (src/iterate.cc:237-248); they are evaluated only at such an iterate. */
int ipxk_ipm_set_crossover_start(ipxk_context* ctx, double value);
/* Iterate::DropToComplementarity (src/iterate.cc:315-391) of a postprocessed iterate (IPXK_E_ARGUMENT on any
 * other): x_out, z_out [n+m], y_out [m], the complementary point crossover starts from.  The outputs follow the
 * pointer mode.  Column partition: local forms, no collective. */
int ipxk_iterate_drop_to_complementarity(ipxk_context* ctx, const double* lb, const double* ub,
                                         double* x_out, double* y_out, double* z_out);

/* ---- crossover in solver form (src/crossover.cc, src/basis.cc:324-351, src/lp_solver.cc:464-537) ---------------
 * The two push phases, Basis::ComputeBasicSolution and the call that strings them together, on the device basis
 * (FTRAN, BTRAN, the eta file, Basis::ExchangeIfStable with the pivot-tolerance ladder).  The vertex stays in
 * solver form here; ipxk_lp_crossover below returns it in the user's terms (Presolver::PostsolveBasicSolution /
 * PostsolveBasis, UserModel::EvaluateBasicPoint).  Out of scope: partitioned contexts, on which all four calls are refused.
 * Conventions of all four:
 *   basis[m] (host) is given; crossover only distinguishes basic from nonbasic, so NONBASIC_FIXED counts as nonbasic
 *     and the tableau row is taken without ignore_fixed.  Each call factorizes the given basis at entry (unit scaling
 *     factors) and depends on no live basis.  On return basis holds the final basis and the context fresh factors of
 *     it (ipxk_solve_dense solves with it).
 *   x, z [n+m], y [m] are in/out and follow the pointer mode; lb, ub, b, c are in the forms of ipxk_ipm_driver.
 *     variables (host) lists the candidates in the order they are pushed; fixed_at_bound (host bytes, may be NULL).
 *   Per candidate one block of scalars reaches the host.  An exchange refused as unstable (refactorization, tighter
 *     pivot tolerance) tries the same candidate again, as crossover.cc:165-166, :291-292.
 *   The interrupt is polled once per candidate: 999 gives status_crossover 5 (time_limit) with errflag 0; 301 / 306
 *     from the basis give 8 (failed); otherwise 1.  What has been pushed stays pushed.
 *   The reference's logic_error checks are IPXK_E_ARGUMENT, counted on the device before any push: a listed variable of
 *     the wrong kind, x outside [lb, ub], a fixed-at-bound variable off its bounds, a z that violates its sign restriction
 *     (bit 1: x != ub, z >= 0; bit 2: x != lb, z <= 0).
 *   The ratio tests are order free.  The reference's first pass shrinks the step entry by entry; in exact arithmetic
 *     its result is the candidate ratio of least magnitude among the entries with |pivot| > 1e-5 (kPivotZeroTol,
 *     strict) that violate their bound by more than feastol at the FULL step: (z_j +- feastol) / row_j for the dual
 *     test, (lbbasic_p - xbasic_p - feastol) / pivot and (ubbasic_p - xbasic_p + feastol) / pivot for the primal one.
 *     That ratio is computed (lowest index among equal magnitudes), then the reference's second pass: the largest |pivot|
 *     among the entries that block within that step, lowest index among equals.  This equals the reference's loop
 *     wherever no two candidate ratios lie within rounding of each other, and exactly at exact ties.  Every reduction is a
 *     fixed-order tree: two calls from the same state give the same bits.
 * ipxk_crossover_push_dual (:229-357): per candidate jb with z[jb] != 0 the tableau row is formed in one gather pass
 *   with the first pass of the ratio test fused in and stored; blocked: jn enters, step = z[jn] / row[jn]; then
 *   y += step btran, z -= step row with the clamps, z[jb] -= step, z[jn] = 0.  x is read only.
 * ipxk_crossover_push_primal (:73-227): per candidate jn not at a bound (nor free at 0) move_to is the nearer finite
 *   bound (ties to lb), 0 for a free variable; blocked: the variable at pblock leaves, step from lbbasic / ubbasic (0
 *   when a fixed-at-bound variable blocks); x[jb] takes exactly its bound, an unblocked x[jn] exactly move_to.
 * ipxk_crossover_basic_solution (basis.cc:324-351): x_B = inverse(B)(b - N x_N), y = inverse(B')(c_B - z_B),
 *   z_j = c_j - a_j'y on the nonbasic j; x_N and z_B stay as given.
 * ipxk_crossover_run (lp_solver.cc:464-537) on the resident POSTPROCESSED iterate: DropToComplementarity; the order
 *   Sortperm(weights) -- weights[n+m] follows the pointer mode, NULL: Iterate::ScalingFactor of the resident iterate --
 *   ascending by (weight, index), a stable sort on the device; the dual superbasics (basic, z != 0) in ascending, the
 *   primal superbasics (nonbasic, off both bounds, not free at 0; screened after the dual phase) in descending order;
 *   the basic solution; basic_statuses[n+m] (host, may be NULL): IPX_basic 0, IPX_nonbasic_lb -1, IPX_nonbasic_ub -2,
 *   IPX_superbasic -3 by the rule at :499-512; primal_infeas / dual_infeas of the vertex (src/model.cc:69-97); status 2
 *   (imprecise) when the first exceeds primal_feastol or the second dual_feastol.  A push phase that does not end optimal
 *   ends the run there; x_out, y_out, z_out then hold no solution.
 * log receives the pairs {jb, jn} of the first log_cap pivots (2 log_cap entries). */
typedef struct ipxk_crossover_params {
    double primal_feastol;     /* 1e-7; for a dualized model the caller swaps the two (crossover.cc:83-84, :237-238) */
    double dual_feastol;       /* 1e-7 */
    ipxint max_etas;           /* 100 */
} ipxk_crossover_params;       /* NULL: the defaults */
typedef struct ipxk_crossover_info {
    ipxint errflag, status_crossover;
    ipxint dual_superbasics, primal_superbasics;    /* candidates listed */
    ipxint dual_pushes, dual_pivots, primal_pushes, primal_pivots;   /* Info::updates_crossover = the two pivot counts */
    ipxint refused;                                 /* exchanges refused as unstable */
    ipxint factorizations;
    double primal_infeas, dual_infeas;              /* ipxk_crossover_run: of the vertex */
    double seconds_dual, seconds_primal;
} ipxk_crossover_info;
int ipxk_crossover_push_dual(ipxk_context* ctx, const double* lb, const double* ub, const double* x, double* y, double* z,
                             const ipxint* variables, ipxint num_variables, ipxint* basis,
                             const ipxk_crossover_params* params, ipxk_crossover_info* info, ipxint* log, ipxint log_cap,
                             ipxk_interrupt_fn interrupt, void* interrupt_user);
int ipxk_crossover_push_primal(ipxk_context* ctx, const double* lb, const double* ub, double* x, const ipxint* variables,
                               ipxint num_variables, const unsigned char* fixed_at_bound, ipxint* basis,
                               const ipxk_crossover_params* params, ipxk_crossover_info* info, ipxint* log, ipxint log_cap,
                               ipxk_interrupt_fn interrupt, void* interrupt_user);
int ipxk_crossover_basic_solution(ipxk_context* ctx, const double* b, const double* c, const ipxint* basis, double* x,
                                  double* y, double* z);
int ipxk_crossover_run(ipxk_context* ctx, const double* b, const double* c, const double* lb, const double* ub,
                       const double* weights, ipxint* basis, const ipxk_crossover_params* params,
                       ipxk_crossover_info* info, double* x_out, double* y_out, double* z_out, ipxint* basic_statuses,
                       ipxint* log, ipxint log_cap, ipxk_interrupt_fn interrupt, void* interrupt_user);

/* LpSolver::InteriorPointSolve (src/lp_solver.cc:305-462) without presolve, postsolve and crossover (the crossover of
 * the solver-form result: ipxk_crossover_run), in one call:
 *   1. ipxk_ipm_starting_point (skipped with use_resident_point: the caller has called
 *      ipxk_ipm_load_starting_point, :337-343); a status other than not_run ends the run.
 *   2. RunInitialIPM (:384-420): ipxk_ipm_driver; switchiter < 0: CR cap min(500, 10 + m/20) and limit
 *      ipm_maxiter, otherwise limit min(switchiter, ipm_maxiter) and no CR cap.  optimal, no_progress, failed and
 *      "stopped at switchiter" go on; any other status ends the run.
 *   3. ipxk_ipm_starting_basis with BuildStartingBasis' mapping (:430-453): errflag 999 -> time_limit (errflag 0),
 *      any other errflag -> failed, rows_inconsistent -> primal_infeas, cols_inconsistent -> dual_infeas.
 *   4. ipxk_ipm_driver_basis with what is left of ipm_maxiter; iter, kktiter and basis_updates are sums over both
 *      phases.
 *   5. ipxk_iterate_postprocess, whatever the status.
 *   6. The postprocessed iterate's residuals, objectives, complementarity and dropping residuals.
 *   7. optimal becomes IPX_STATUS_imprecise (2) when |rel_objgap| > optimality_tol or a relative residual exceeds
 *      feasibility_tol (:326-330).
 * crossover_start holds for this call only (the context's own value is restored).  basis_out[m], status_out[n+m]
 * (either may be NULL) return the last basis if one was built.  Refused on any partitioned context, before any
 * work. */
typedef struct ipxk_solve_params {
    double kkt_tol;            /* 0.3 */
    double feasibility_tol;    /* ipm_feasibility_tol, 1e-6 */
    double optimality_tol;     /* ipm_optimality_tol, 1e-8 */
    double crossover_start;    /* 0: off (the reference with crossover = 0); its default with crossover: 1e-8 */
    double dependency_tol;     /* 1e-6 */
    ipxint ipm_maxiter;        /* 300 */
    ipxint switchiter;         /* -1: the reference's default */
    ipxint max_etas;           /* as ipxk_ipm_starting_basis */
    int precond_dense_cols;
    int use_resident_point;
} ipxk_solve_params;
typedef struct ipxk_solve_info {
    ipxint status_ipm, iter, errflag, kktiter;
    double pobjective, dobjective;       /* of the postprocessed iterate */
    double presidual, dresidual, complementarity, mu;
    double step_primal, step_dual;
    ipxint basis_updates;
    ipxint iter_initial, status_initial; /* the initial iterations and what ended them */
    ipxint dependent_rows, dependent_cols, rows_inconsistent, cols_inconsistent, updates_start;
    double abs_presidual, abs_dresidual; /* of the postprocessed iterate */
    double rel_presidual, rel_dresidual; /* over 1 + norm_bounds, 1 + norm_c */
    double rel_objgap;                   /* (pobj - dobj) / (1 + 0.5 |pobj + dobj|) */
    double pres_dropping, dres_dropping;
} ipxk_solve_info;
int ipxk_ipm_solve(ipxk_context* ctx, const double* b, const double* c, const double* lb,
                   const double* ub, const ipxk_solve_params* params, ipxk_solve_info* info,
                   ipxint* basis_out, ipxint* status_out, ipxk_interrupt_fn interrupt,
                   void* interrupt_user);

/* ---- user model: an LP as the user states it, presolved on the device (src/user_model.cc, src/presolver.cc) ----
 *   min obj'x   s.t.  A x {=,<,>} rhs,  lb <= x <= ub          (A: num_constr x num_var, CSC; bounds may be infinite)
 * ipxk_lp_create is UserModel::Load + Presolver::PresolveModel into a context the lp owns:
 *   - validation as UserModel::CopyInput, CheckVectors and CheckMatrix (src/user_model.cc:217-303): dimensions
 *     (num_constr >= 0, num_var > 0) and NULL arguments, then the reference's checks -1 rhs finite, -2 obj finite,
 *     -3 bounds finite or the correct infinity with lb <= ub, -4 constr_type one of "=<>", -5 Ap[0] == 0 and monotone,
 *     -6 values finite, -7 row indices in range, -8 no row index twice in a column (sorted or not).  A failure returns
 *     IPXK_E_ARGUMENT and ipxk_last_error() reads "... check <number> ... index <i>": the check the reference would
 *     have failed first, and the first index that fails it (of rhs / obj / the bounds / constr_type / Ap; the position in
 *     Ax / Ai for -6, -7, -8; for -8 the position of the second occurrence).  The checks run on the device; the first
 *     index is a minimum over block partials.
 *   - SparseMatrix::LoadFromArrays (src/sparse_matrix.cc:49-69), the end of CopyInput: explicit zeros are dropped and
 *     every column is sorted by row index, so ipxk_lp_info::nnz may be below Ap[num_var].
 *   - ComputeUserModelAttributes (src/presolver.cc:118-133), LoadPrimal (:135-180) or LoadDual (:182-264) --
 *     dualize < 0: when num_constr > 2 * num_var (:33-34) -- and ScaleModel (:266-292) with ipxk_equilibrate's kernels
 *     when scale >= 1.  All of it is sign flips, copies and powers of two: the solver form is the reference's bit for bit.
 *   - the context from the resident matrix as ipxk_create builds it (layouts, dense columns, renumbering).
 * Between the upload of the arguments and the downloads of the getters only scalars, counts and flag blocks cross
 * to the host -- and what the construction of any context brings there: the column pointers, the histogram of the
 * column counts and, below 2^16 entries, the entries for the host layout builders.  The context (ipxk_lp_context)
 * is owned by the lp and unpartitioned; every ipxk_* call works on it.
 * Out of scope: Presolver::PresolveIPMStartingPoint (a caller who has a starting point loads it in solver form with
 * ipxk_ipm_load_starting_point on the lp's context and sets use_resident_point), Presolver::PresolveStartingPoint (a
 * user-form basic starting point), and partitioned contexts (after ipxk_comm_init* on the lp's context ipxk_lp_solve
 * and ipxk_lp_crossover return what ipxk_ipm_solve and ipxk_crossover_run return on a partitioned context). */
typedef struct ipxk_lp ipxk_lp;
typedef struct ipxk_lp_params {
    ipxint dualize;            /* -1: num_constr > 2 * num_var, 0: never, 1: always (ipx_parameters::dualize) */
    ipxint scale;              /* 0: none, >= 1: EquilibrateMatrix (ipx_parameters::scale, :271-272) */
    int device;
} ipxk_lp_params;              /* NULL: -1, 1, 0 */
typedef struct ipxk_lp_info {
    ipxint m, n, nnz;          /* solver form; nnz of the n structural columns */
    ipxint dualized, num_boxed, num_flipped, num_free_var, num_eqconstr;
    ipxint scale_rounds;       /* as ipxk_equilibrate's *rounds (-1 also with scale == 0) */
    ipxint num_dense_cols;
    double seconds;
} ipxk_lp_info;
int ipxk_lp_create(ipxint num_constr, ipxint num_var, const ipxint* Ap, const ipxint* Ai,
                   const double* Ax, const double* rhs, const char* constr_type,
                   const double* obj, const double* lb, const double* ub,
                   const ipxk_lp_params* params, ipxk_lp_info* info, ipxk_lp** out);
void ipxk_lp_destroy(ipxk_lp* lp);
ipxk_context* ipxk_lp_context(ipxk_lp* lp);
/* The solver form (host arrays): the n structural columns of AI (Ap[n+1], Ai, Ax[nnz]), b[m], c, lb, ub [n+m],
 * colscale[n], rowscale[m] (1.0 where the reference's scaling vectors are empty).  Any may be NULL. */
int ipxk_lp_get_model(ipxk_lp* lp, ipxint* Ap, ipxint* Ai, double* Ax, double* b, double* c,
                      double* lb, double* ub, double* colscale, double* rowscale);
/* ipxk_ipm_solve on the lp's context with the resident b, c, lb, ub.  The last basis, if the solve built one, stays
 * with the lp (ipxk_lp_get_basis, ipxk_lp_crossover); a basic solution stored by an earlier ipxk_lp_crossover is
 * cleared. */
int ipxk_lp_solve(ipxk_lp* lp, const ipxk_solve_params* params, ipxk_solve_info* info,
                  ipxk_interrupt_fn interrupt, void* interrupt_user);
/* Presolver::PostsolveInteriorPoint (src/presolver.cc:618-793) of the context's resident iterate, postprocessed or
 * not: x, xl, xu, zl, zu [num_var], slack, y [num_constr]; any may be NULL.  A pure elementwise map with the
 * reference's operations on the reference's operands (one IEEE operation per entry).  The outputs follow the
 * context's pointer mode. */
int ipxk_lp_postsolve(ipxk_lp* lp, double* x, double* xl, double* xu, double* slack, double* y,
                      double* zl, double* zu);
/* UserModel::EvaluateInteriorPoint (src/user_model.cc:99-171) of the postsolved resident iterate, with the norms of
 * UserModel::ComputeNorms (:306-316).  Computed on the device; every sum and maximum is a fixed-order tree over
 * block partials: two calls give the same bits.  ipxk_lp_get_residuals copies out the two residual vectors of the
 * last evaluation, rb = rhs - slack - A x [num_constr] and rc = obj - zl + zu - A'y [num_var] (host arrays; either
 * may be NULL). */
typedef struct ipxk_lp_eval {
    double abs_presidual, abs_dresidual, rel_presidual, rel_dresidual;
    double pobjval, dobjval, rel_objgap, complementarity;
    double normx, normy, normz;
    double norm_obj, norm_rhs, norm_bounds;
} ipxk_lp_eval;
int ipxk_lp_evaluate(ipxk_lp* lp, ipxk_lp_eval* out);
int ipxk_lp_get_residuals(ipxk_lp* lp, double* rb, double* rc);
/* ---- basic solutions in user form (src/presolver.cc:92-116, 566-616, 795-867; src/user_model.cc:173-211) ----
 * ipxk_lp_postsolve_basic is Presolver::PostsolveBasicSolution of ANY solver-form point: PostsolveGeneralPoint,
 * PostsolveBasis and CorrectBasicSolution as one map from x_solver, z_solver [n+m], y_solver [m] and
 * basic_statuses[n+m] (IPX_basic 0, IPX_nonbasic_lb -1, IPX_nonbasic_ub -2, IPX_superbasic -3) to x, z [num_var],
 * slack, y [num_constr], vbasis[num_var] (the same four values) and cbasis[num_constr] (IPX_basic 0, IPX_nonbasic -1).
 * The double arrays follow the context's pointer mode, the status arrays are host memory; any output may be NULL.
 * Every entry is the reference's operation on the reference's operands; the correction writes exactly lb[j], ub[j]
 * of the user model or 0.0.  Statuses that violate the reference's asserts are refused with IPXK_E_ARGUMENT, found on
 * the device before anything is written (ipxk_last_error() names the first offending index): a slack variable that is
 * superbasic, and for a dualized model a boxed variable whose added column is basic while the variable's own slack
 * is basic too (:822: the variable would be nonbasic twice).  num_constr == 0 is served.
 *
 * ipxk_lp_crossover is the tail of LpSolver::Solve after the interior solve (src/lp_solver.cc:64-67, :464-537).  It
 * needs a preceding ipxk_lp_solve on this lp (IPXK_E_ARGUMENT otherwise).  If that solve did not end with status_ipm
 * 1 or 2 it returns 0 with status_crossover 0 and nothing else happens.  Otherwise ipxk_crossover_run's body runs on the
 * resident b, c, lb, ub from the basis the solve left, with the scaling factors of the resident iterate as weights.
 * params are in the USER's terms: for a dualized model the call swaps primal_feastol and dual_feastol itself
 * (src/crossover.cc:83-84, :237-238).  With status_crossover 1 the vertex is postsolved, kept in the lp and
 * evaluated (UserModel::EvaluateBasicPoint: primal_infeas, dual_infeas, objval = obj'x, fixed-order trees over block
 * partials: the same bits from the same vertex); status_crossover becomes 2 when primal_infeas exceeds the user's
 * primal_feastol or dual_infeas the dual one (:534-536).  crossover_info->primal_infeas / dual_infeas stay those of
 * the solver-form vertex.  A push phase that does not end optimal, or an interrupt (status_crossover 5, errflag 0),
 * leaves no basic solution; basic_eval (may be NULL) is zero then.  An lp with num_constr == 0 is refused with
 * IPXK_E_ARGUMENT (there is no basis to push on); so is a partitioned context.
 *
 * ipxk_lp_evaluate_basic is UserModel::EvaluateBasicPoint on its own, of any user-form point: x, z [num_var], slack, y
 * [num_constr] follow the pointer mode, vbasis[num_var] is host memory; none may be NULL (slack and y may with num_constr
 * == 0).  Two calls on the same point give the same bits.
 *
 * ipxk_lp_get_basic_solution copies out the stored vertex (IPXK_E_ARGUMENT when there is none, where
 * LpSolver::GetBasicSolution returns -1); ipxk_lp_get_basis is LpSolver::GetBasis: the vertex's statuses if one is
 * stored, else BuildBasicStatuses (:212-231) of the last solve's basis through PostsolveBasis, else IPXK_E_ARGUMENT.
 * Doubles follow the pointer mode, statuses are host arrays, any may be NULL. */
typedef struct ipxk_lp_basic_eval {
    double primal_infeas, dual_infeas, objval;
} ipxk_lp_basic_eval;
int ipxk_lp_postsolve_basic(ipxk_lp* lp, const double* x_solver, const double* y_solver, const double* z_solver,
                            const ipxint* basic_statuses, double* x, double* slack, double* y, double* z,
                            ipxint* cbasis, ipxint* vbasis);
int ipxk_lp_crossover(ipxk_lp* lp, const ipxk_crossover_params* params, ipxk_crossover_info* crossover_info,
                      ipxk_lp_basic_eval* basic_eval, ipxk_interrupt_fn interrupt, void* interrupt_user);
int ipxk_lp_evaluate_basic(ipxk_lp* lp, const double* x, const double* slack, const double* y, const double* z,
                           const ipxint* vbasis, ipxk_lp_basic_eval* out);
int ipxk_lp_get_basic_solution(ipxk_lp* lp, double* x, double* slack, double* y, double* z, ipxint* cbasis,
                               ipxint* vbasis);
int ipxk_lp_get_basis(ipxk_lp* lp, ipxint* cbasis, ipxint* vbasis);

/* ---- multi-GPU: rows of AI partitioned over ranks, one RCCL all-reduce per
 *      NormalMatrix apply ---------------------------- */
/* 128-byte RCCL unique id, created on rank 0 and broadcast by the launcher. */
int ipxk_comm_unique_id(void* id128);
/* The context must have been created from this rank's row slab (m = local
 * rows, all n columns, row indices local).  After this call dot products and
 * norms of the CR loop are global and ipxk_normal_apply all-reduces A_g' y_g.
 * Collective: the dense columns are classified once more from the column
 * counts of the whole matrix (one all-reduce of n), so that every rank treats
 * the same dense columns (ipxk_num_dense_cols, dense-column preconditioning). */
int ipxk_comm_init(ipxk_context* ctx, const void* id128, int rank, int nranks);
/* Alternative partition ("column partition"): the context
 * was created from this rank's slab of structural COLUMNS (all m rows, n =
 * local columns).  Vector arguments then are [local structural part; all m
 * slack entries] for (n+m)-vectors and full m-vectors; every m-vector and
 * every scalar of the CR loop is replicated, the one exchange step per
 * NormalMatrix::_Apply is the all-reduce of the m partial sums A_g t_g.
 * Collective: the dense columns are classified from a histogram of the column
 * counts of all ranks (an all-reduce of 1 and one of max count + 1 doubles);
 * each rank keeps the dense columns it owns, and the first Factorize with
 * dense-column preconditioning gathers those of every rank.  The basis path
 * (ipxk_split_prepare and what uses its operator) runs on this partition; see
 * ipxk_split_prepare for its conventions.  So does the device IPM (the iterate,
 * ipxk_newton_solve, ipxk_ipm_step, ipxk_ipm_driver, ipxk_ipm_starting_point,
 * ipxk_ipm_load_starting_point); see ipxk_iterate_set. */
int ipxk_comm_init_columns(ipxk_context* ctx, const void* id128, int rank, int nranks);
/* What the transport itself reports about the communicator of this context:
 * transport 0 = none, 1 = RCCL (nranks / rank from ncclCommCount /
 * ncclCommUserRank), 2 = the direct exchange (its rank table).  For the records
 * of a multi-GPU run (bench.py writes it into its JSON line). */
int ipxk_comm_info(const ipxk_context* ctx, int* transport, int* nranks, int* rank);

/* ---- measurement helpers (bench.py, section 8d) --------------------------- */
/* Runs `reps` NormalMatrix applies on resident device vectors and returns the
 * total elapsed milliseconds between HIP events on the context's stream. */
int ipxk_time_normal_apply(ipxk_context* ctx, const double* rhs_dev,
                           double* lhs_dev, int reps, double* ms_total);
/* algorithmic bytes of one NormalMatrix apply: 2*nnz*(4+8) + (n+m+2)*4 +
 * 8*(3n+4m) */
ipxint ipxk_normal_apply_bytes(const ipxk_context* ctx);
/* Which device layout the two sparse products of NormalMatrix::_Apply
 * (normal_matrix.cc:45-126) use on this model: layout[0] for t = W.*(A'y),
 * layout[1] for lhs = A t; 0 = phased (time-tiled), 1 = XCD-sliced tiles,
 * 2 = fused tiles (one slice, epilogue in the tile kernel), 3 = retired (it
 * was the sorted sub-tiles: the sliced layout's slices with the gathers of a
 * tile issued in address order; never returned), 4 = sorted fused tiles
 * (one slice, gathers in address order, epilogue in the tile kernel: bit-identical
 * to 0 and 2, for matrices whose gathers have locality), 5 = accumulated tiles
 * (the sliced layout's slices, a row block's sums kept in LDS, the entries of a
 * tile in address order and in batches that hold one entry per row; same partial
 * sums as 1 for rows stored with ascending indices; used whenever the sliced
 * layout is and IPXK_SPMV_ACC is not 0), 6 = plain rows (the matrix as it is, 8
 * lanes per row, sums in storage order: bit-identical to 0, 2 and 4; a candidate of
 * the timing for matrices of at most 4M entries), 7 = fused accumulated tiles (5
 * with one slice and the epilogue in the tile kernel, for matrices whose gathers have
 * locality and whose rows are stored sorted: bit-identical to 0, 2, 4, 6).  The sliced layouts are
 * chosen by a property of the matrix (x larger than an XCD's L2 and gathers that
 * spread over the slices): 5 when it can be built (the host builders do not
 * build it for a matrix with long rows), else 1, no timing takes part; otherwise a timing at ipxk_create picks among the
 * bit-identical 0, 2, 4, 6 and 7
 * (IPXK_SPMV_LAYOUT=phased|sliced|fused|sortedfused|acc|plain|accfused
 * overrides).  us[6] receives the measured microseconds {pass 1: phased, the layout
 * in use if it is 1 or 5 (else sliced), the layout in use if it is 2, 4, 6 or 7
 * (else fused); pass 2 likewise} (0 = not timed). */
int ipxk_spmv_layout(const ipxk_context* ctx, int layout[2], double us[6]);
/* The guard of the explicit inverses of SplittedNormalMatrix::Prepare's device
 * form (ipxk_split_prepare*): narrow first / last levels of a sweep and large
 * dense blocks of the factors are applied as inverse(T) * b; substitution is
 * backward stable whatever the condition of T, a product with a computed inverse
 * is not, and IPX's late bases are ill conditioned by construction (that is what
 * the stability loop of src/basis.cc:130-152 and the residual test of
 * src/lu_factorization.cc:87-127 are for).  Every inverse is therefore probed at
 * Prepare with two fixed vectors, || T (M z) - z ||_inf: the inverted levels of a
 * sweep must meet 1e-10, the inverse of a dense block of the factors 1e-8
 * (IPXK_INVERSE_TOL sets both).  A dense block's inverse from the matrix cores that
 * misses 1e-8 gets up to two refinement steps X += X (I - D X) first
 * (IPXK_DENSE_INVERSE_REFINE); one that still misses it but stays below 1e-5 is held
 * against the blocked solve it would replace, probed with the same two vectors, and
 * kept if it is within four times that solve's own residual (an ill-conditioned
 * block leaves neither at 1e-8).  A block that fails keeps its level-scheduled /
 * blocked solve.  Returns the number of probes, of rejected inverses and the worst
 * accepted residual seen since ipxk_create; ipxk_split_inverse_refined the number
 * of refinement steps taken. */
int ipxk_split_inverse_stats(const ipxk_context* ctx, ipxint* probes,
                             ipxint* rejected, double* worst_residual);
ipxint ipxk_split_inverse_refined(const ipxk_context* ctx);
/* Inspection of the device layouts (tests: the layouts built on the device by
 * radix sorts, layout_device.hip, against the host builders, array by array;
 * IPXK_LAYOUT_BUILD=host forces the host builders).  The reference's
 * NormalMatrix copies nothing (normal_matrix.h:20-27): what replaces its
 * "construct = store a reference" is one upload + transpose + layout build per
 * model, timed in create_ms {upload + transpose, A' layouts, A layouts, rest}.
 * which: 0 = the gather matrix of A'y (rows = columns of A), 1 = of A t.
 * info: {use_sliced, retired, use_sorted_fused, nlong, sliced.built, R,
 * nslices, nrb, nrows_pad, max_tile, bits of the fullest-slice share (double),
 * sorted.built, retired, retired, nrb, RB, nrows_pad, max_sub, retired, retired,
 * nnz, P, G, RT*1e6 + Q*1e3, use_acc, acc.built, nslices, nrb, RB, nrows_pad,
 * slice_elems, # batches, # entries that waited for a later batch, use_acc_fused,
 * accf.built, nrb, RB, # batches, use_plain, # steps of the accumulated tiles (runs
 * of batches the persistent kernel takes as one pipeline step), # 16-byte units of
 * their wide stream (0: not built, IPXK_ACC_WIDE=0), the launch grid their head
 * tables are built for (0: not built, the default; IPXK_ACC_HEAD=1 builds them); the rest of the 48 is 0}.
 * `sorted`: the sorted fused tiles.  The retired slots [1], [12], [13], [18], [19]
 * described the sorted sub-tiles (use_sorted, their slice and sub-slice counts, their
 * slice width, the fused flag) and are always 0.  use_sorted_fused, use_acc,
 * use_acc_fused and use_plain say whether that is the layout of ipxk_spmv_layout (at
 * most one of them is 1); use_sliced whether the sliced or fused tiles are built, which
 * masked products (the basis path) use whatever the layout. */
int ipxk_layout_info(const ipxk_context* ctx, int which, ipxint info[48],
                     double create_ms[4]);
/* array: 0 sliced tile_ptr (u32), 1 sliced cnt (u8), 2 sliced idx (i32), 3
 * sliced val (f64), 4-7 the sorted fused tiles: sub_ptr (u32), cnt (u8), pack
 * (u32), val (f64); 8 / 9 / 10 the row-wise copy of the model (Transpose,
 * sparse_matrix.cc:120-151) as the device holds it: ptr (i32), idx (i32), val
 * (f64); 11 acc tile_batch (u32), 12 acc bptr (u32), 13 acc pack (u32), 14 acc
 * val (f64); 15-19 the fused accumulated tiles: tile_batch, bptr, pack (u32), val
 * (f64), xmin (i32); 20 xmin of the sorted fused tiles (i32); 21 acc
 * tile_step (u32, first step of each tile), 22 acc step records (4 x u32 each: first
 * entry and three cuts; one more than there are steps); 23 the wide stream of the
 * accumulated tiles (u32; units of 16 bytes: per step of ne entries and Tp =
 * roundup64(ceil(ne / 4)) threads Tp units {entry words of positions t, Tp + t,
 * 2 Tp + t, 3 Tp + t}, Tp units {values of the first two}, Tp units {values of the
 * last two}, as bit patterns; positions >= ne are zero), 24 the first unit of each
 * step in it (u32, one per step record; the last is the total).  23 and 24 are empty
 * with IPXK_ACC_WIDE=0, which makes the persistent tile kernel read arrays 13 and 14
 * as it did before there was a wide stream.  25 the head of the accumulated tiles
 * (u32, 64 words per workgroup of the launch grid: the records {first entry, end,
 * three cuts, first unit of the wide stream, tile, 0} of the first six steps of the
 * workgroup's walk, tile = -1 past its last tile, then the walker's state {tile,
 * step in it, first step record of the tile, its steps}, then zeros), 26 the head of
 * the wide stream (u32; per workgroup, step 0-2 and plane 0-2 the 512 units of 16
 * bytes that threads 0-511 load for it); both empty unless IPXK_ACC_HEAD=1, 26 also
 * with IPXK_ACC_WIDE=0.  Copies min(cap, size) bytes into out;
 * *nbytes = the array's size. */
int ipxk_layout_array(ipxk_context* ctx, int which, int array, void* out,
                      ipxint cap, ipxint* nbytes);
/* plain device allocation helpers so that callers without torch can hold
 * resident vectors */
int ipxk_dev_alloc(ipxk_context* ctx, ipxint bytes, void** ptr);
int ipxk_dev_free(ipxk_context* ctx, void* ptr);
int ipxk_dev_upload(ipxk_context* ctx, void* dst_dev, const void* src_host,
                    ipxint bytes);
int ipxk_dev_download(ipxk_context* ctx, void* dst_host, const void* src_dev,
                      ipxint bytes);

#ifdef __cplusplus
}
#endif
#endif /* IPX_KKT_HIP_H_ */
