// The object behind ipxk_context: one model's matrix resident on one GPU plus
// every workspace of the KKT path (allocated once, reused by every solve).
#pragma once

#include "internal.hpp"
#include "device_utils.hpp"

struct ncclComm;

namespace ipxk {

constexpr int kPartialStride = kMaxPartials + 8;   // doubles per partial array

// indices of the per-workgroup partial arrays inside Context::partials
enum PartialSlot {
    kPartRes0 = 0,   // scaled residual norm (max), parity 0
    kPartRes1,       //                          , parity 1
    kPartPdot,       // Cstep' * P * Cstep  (or Cstep'*Cstep for plain CR)
    kPartCdot,       // dot from C.Apply
    kPartRsdot,      // residual' * P * residual (every 5th iteration)
    kPartScratch,
    kNumPartialSlots
};

// A second copy of the model with rows and columns renumbered for locality (reorder.hip, reorder_model): the loop of the
// preconditioned CR method of the diag path runs on it, in permuted numbering; everything else keeps the original numbering.
struct Reordered {
    bool active = false;                 // the copy exists and is the faster one
    int levels = 0;                      // depth of the breadth-first level structure the numbering comes from
    int components = 0;
    double ms = 0.0;                     // time of the analysis + the second copy inside ipxk_create
    float us_original = 0.f, us_reordered = 0.f;      // the two products of NormalMatrix::Apply, timed on both copies
    DevBuf<int> rowperm, rowinv, colperm, colinv;     // new -> old, old -> new
    DevBuf<int> Ap, Ai, Tp, Ti;          // the renumbered matrix: CSC and the row-wise copy
    DevBuf<double> Ax, Tx;
    GatherMatrix Acols, Arows;
    DevBuf<double> W, diagonal, resscale, rhs, y, tcols;       // the solver's vectors in the new numbering
    bool in_use = false;                 // set around the CR loop of kkt_diag_solve_dev: operator and preconditioner take the copy
};

struct SplitOperator;   // trisolve.hpp
struct PrepareHost;     // prepare_device.hip
struct LuState;         // lu.hip
struct MaxvolState;     // internal.hpp
struct NMatrix;         // nmatrix.hip

struct Context;
long lu_generation(const Context* c);   // lu.hip

// A basis and its statuses on the host, together with the factorization they belong to: another factorization in the context
// ends the state.
struct LiveBasis {
    bool live = false;
    long lu_generation = -1;
    std::vector<ipxint> basis, status;
    bool current(const Context* c) const { return live && lu_generation == ipxk::lu_generation(c); }
    void store(const Context* c, const std::vector<ipxint>& b, const std::vector<ipxint>& s) {
        basis = b;
        status = s;
        lu_generation = ipxk::lu_generation(c);
        live = true;
    }
    void clear() { live = false; }
};

struct Context {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    int pointer_mode = IPXK_POINTER_HOST;
    // optional per-operator timing (ipxk_set_profiling): HIP events around every operator /
    // preconditioner / triangular-solve application of a solve, summed into ipxk_times afterwards
    bool profile_ops = false;
    // host pointer mode: the device copies of one call's vector arguments, one slot per argument in the order the call declares
    // them (api.hip); grow-only.  kStageSlots: the most vector arguments any entry point has (ipxk_newton_solve, 10 in + 6 out)
    static constexpr int kStageSlots = 16;
    DevBuf<double> stage_slots[kStageSlots];
    DevBuf<unsigned char> stage_bytes;
    ipxint (*interrupt)(void*) = nullptr;   // ipxk_set_interrupt: Control::InterruptCheck for calls without a callback argument
    void* interrupt_user = nullptr;
    bool timing_active = false;
    std::vector<hipEvent_t> time_events;
    std::vector<int> time_kinds;        // per recorded event: kind (begin) or -1-kind (end)
    size_t time_used = 0;

    // ---- model ----
    int64_t m = 0, n = 0, nnz = 0;
    std::vector<ipxint> h_Ap;           // column pointers (host)
    // host copies of the entries and of the row-wise copy: filled on demand only (ensure_host_model) -- the model
    // lives on the device, the layouts are built there (model.hip, layout_device.hip)
    std::vector<ipxint> h_Ai;
    std::vector<double> h_Ax;
    std::vector<ipxint> h_ATp, h_ATi;
    std::vector<double> h_ATx;
    // the model on the device in plain form, 32-bit indices: CSC and the row-wise copy (Transpose,
    // src/sparse_matrix.cc:120-151).  Shared by the layout builders, N (nmatrix.hip) and the basis LU (lu.hip).
    DevBuf<int> pl_Ap, pl_Ai, pl_Tp, pl_Ti;
    DevBuf<double> pl_Ax, pl_Tx;
    bool have_plain = false;
    double create_ms[4] = {0, 0, 0, 0};   // ipxk_create: upload + transpose, Acols layouts, Arows layouts, the rest
    GatherMatrix Acols;                 // rows = columns of A  (computes A'y)
    GatherMatrix Arows;                 // rows = rows of A     (computes A t)
    Reordered reord;                    // the same matrix renumbered for locality, if that pays (reorder.hip)
    int64_t num_dense = 0, nz_dense = 0;
    std::vector<ipxint> dense_cols;

    // ---- NormalMatrix ----
    DevBuf<double> W_own;               // n+m
    const double* W = nullptr;          // device pointer in use (W_own or caller's)
    bool normal_prepared = false;
    DevBuf<double> tcols;               // n workspace: t = Ws .* (A'y)

    // ---- DiagonalPrecond ----
    DevBuf<double> diagonal;            // m
    bool diag_factorized = false;
    int64_t kdense = 0;                 // # dense columns treated by SMW (0: plain diagonal)
    GatherMatrix AdCols;                // k rows x m: computes Ad' u
    GatherMatrix AdRows;                // m rows x k: computes Ad w
    DevBuf<double> chol, chol_inv, smw_work, smw_u, Wnodense;   // chol_inv: inverted 64 x 64 diagonal blocks (k > 64)
    DevBuf<double> schur_panel, schur_part;     // blocked Schur assembly: dense copy of the dense columns, per-slab partial S
    DevBuf<int> schur_colptr;
    DevBuf<int> chol_info;
    DevBuf<unsigned char> dense_mask;   // n, 1 for dense columns
    // column partition: # dense columns of every rank (AdCols / AdRows then hold all of them, rank order, then local
    // order) and the gathered dense weights
    std::vector<int> dense_rank_k;
    DevBuf<double> dense_W, dense_Wsend, dense_Wrecv;
    DevBuf<int> dense_Widx;

    // ---- CR workspaces (m-vectors) ----
    DevBuf<double> v_rhs, v_lhs, v_residual, v_sresidual, v_step, v_Cstep, v_Cres, v_pCstep;
    DevBuf<double> partials;            // kNumPartialSlots * kPartialStride
    DevBuf<CrState> state;
    CrState* h_state = nullptr;         // pinned
    DevBuf<double> hist;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
    std::vector<hipEvent_t> ev_window;
    // what the last CR run enqueued (ipxk_cr_loop_stats): iterations, kernel launches of the loop's own kernels,
    // snapshot launches, events recorded inside the loop
    long long cr_loop_stats[4] = {0, 0, 0, 0};

    // ---- KKTSolverDiag ----
    DevBuf<double> resscale;            // m
    DevBuf<double> k_tmp;               // n+m scratch
    bool kkt_diag_factorized = false;

    // ---- IPM::SolveNewtonSystem (newton.hip) ----
    DevBuf<double> nw_rhs1, nw_rhs2;    // n+m, m

    // ---- the IPM iterate (iterate.hip) ----
    DevBuf<double> it_x, it_xl, it_xu, it_y, it_zl, it_zu, it_partials;
    DevBuf<double> it_row, it_bnd, it_table;   // column partition: this rank's row of scalars, step-to-boundary partials, gathered rows
    DevBuf<unsigned char> it_state;
    bool it_set = false;
    DevBuf<double> ipm[12];            // residuals, complementarity targets and the step of ipxk_ipm_step
    // the end of the solve (finish.hip): Iterate::postprocessed_ (residuals and objectives take the postprocessed branches, the
    // iterate no longer advances), Iterate::crossover_start_ (0: the drivers stop at feasible and optimal), and max |a_ij| of every
    // structural column for ResidualsFromDropping (computed at the first use, kept: the model never changes)
    bool postprocessed = false;
    double crossover_start = 0.0;
    DevBuf<double> colmax;
    bool have_colmax = false;

    // ---- basis path ----
    // guard of the explicit inverses (inverse_guard.hpp): # probes and # inverses rejected since the context was created, worst residual
    struct { long inverse_probes = 0, inverse_rejected = 0, inverse_refined = 0; double worst_probe = 0.0; } split_stats;
    SplitOperator* split = nullptr;
    SplitOperator* split_spare = nullptr;  // the operator's buffers after ipxk_reset_solver_state: reused by the next Prepare, never applied
    // LU pivot tolerance of Maxvolume's refactorizations: tightened after an unstable exchange and kept for the later calls of the SAME
    // solver object, like Basis::TightenLuPivotTol changes lu_->pivottol() for good (src/basis.cc:490-503); ipxk_reset_solver_state
    // sets it again (src/basis.cc:30: every Basis starts from control.lu_pivottol())
    double maxvol_pivottol = 0.1;
    PrepareHost* prepare_host = nullptr;   // host workspaces of split_prepare (prepare_device.hip)
    LuState* lu = nullptr;                 // factors of the last ipxk_lu_factorize* (lu.hip)
    DevBuf<double> dense_work;             // workspace of the dense block inverse (dense_inverse.hip), grow-only
    MaxvolState* maxvol = nullptr;         // workspaces of the basis exchanges (basis.hip, maxvolume.hip, starting_basis.hip)
    bool etas_live = false;                // the operator `split` stands for a LATER basis than its factors: Maxvolume's last exchanges are applied as etas behind them (basis.hip)
    NMatrix* nmat = nullptr;               // N of the split operator as a matrix of its own (nmatrix.hip)
    // the factors, the operator and these statuses are the result of ipxk_ipm_starting_basis (starting_basis.hip): the main phase
    // (ipm_driver_dev with use_basis) goes on from them instead of the slack basis
    LiveBasis sb;
    // DropPrimal / DropDual (drop.hip): Control::ipm_drop_primal / ipm_drop_dual (0, 0: off), the basis ipm_driver_dev ended with
    // when it did not start from a starting basis (what ipxk_ipm_drop_degenerate then works on), and Info::primal_dropped /
    // dual_dropped / the drop exchanges since the last driver began
    double drop_primal = 0.0, drop_dual = 0.0;
    LiveBasis drv;
    ipxint sum_primal_dropped = 0, sum_dual_dropped = 0, sum_drop_updates = 0;

    // ---- multi-GPU ----
    ncclComm* comm = nullptr;
    struct DirectComm* direct = nullptr;   // hand-written exchange over hipIpc-mapped peer buffers (IPXK_COMM=direct)
    int rank = 0, nranks = 1;
    int64_t m_global = 0;               // rows of the whole system (sum over ranks)
    bool force_comm = false;
    // false: rows of AI partitioned (m local, n global; scalars and A'y need exchange steps);
    // true: structural COLUMNS partitioned (m global, n local; every m-vector and every scalar of
    // the CR loop is replicated, the only exchange is the sum of the partial products A_g t_g)
    bool col_partition = false;
    // column partition: this rank's first structural column and the structural columns of all ranks (learn_col_offsets;
    // -1: not known yet)
    int64_t col_offset = -1, n_global = 0;
    DevBuf<double> comm_scalars;        // scratch scalars (single-value reductions)
    DevBuf<double> comm_send;           // kNumPartialSlots scalars of this rank
    DevBuf<double> comm_gather;         // nranks * kNumPartialSlots, rank-major
    int* h_cycle_done = nullptr;        // mapped pinned ring: `done` at the end of each cycle
    int* d_cycle_done = nullptr;

    Context() = default;
    ~Context();
    double* part(int slot) const { return partials.get() + (size_t)slot * kPartialStride; }
    void ensure_partials() { if (partials.size() == 0) partials.resize((size_t)kNumPartialSlots * kPartialStride); }
};

// ---- model.hip: the model on the device, its gather matrices, the dense-column classification ----
void build_model(Context* c, const ipxint* Ap, const ipxint* Ai, const double* Ax);
void upload_plain_model(Context* c, const ipxint* Ap, const ipxint* Ai, const double* Ax);
// a model whose plain CSC is on the device already: adopt_plain_model completes the plain copy (host column pointers, row-wise
// copy), build_model_resident builds everything else of the context (host arrays NULL: none to fall back on)
void adopt_plain_model(Context* c);
void build_model_resident(Context* c, const ipxint* Ap, const ipxint* Ai, const double* Ax);
void ensure_host_model(Context* c, bool rowwise);
void fetch_columns(Context* c, const std::vector<ipxint>& cols, std::vector<ipxint>& Cp, std::vector<ipxint>& Ci, std::vector<double>& Cx);
// partitioned contexts: dense-column classification of the whole matrix (comm_init); true if it changed
bool classify_dense_columns_global(Context* c);
struct LayoutScratch;                 // layout_scratch.hpp
struct Tmp;
int device_max_row_length(LayoutScratch& S, int nrows, const int* dptr, hipStream_t s);
// row of every entry of a row-wise matrix, and (pos != nullptr) the entry's own position; row pointers from the sorted rows of the entries
void device_row_of_entries(int nrows, const int* ptr, int* rowof, unsigned* pos, hipStream_t s);
void device_row_pointers(int64_t nrows, int64_t nz, const unsigned* sorted_rows, int* ptr, hipStream_t s);
void device_transpose(Tmp& T, DevBuf<int>& colof, int64_t n, int64_t m, int64_t nz, const int* Ap, const int* Ai, const double* Ax, int* Tp,
                      int* Ti, double* Tx, hipStream_t s);

// ---- layout_device.hip: the device builders (the host builders are members of GatherMatrix: layout_host.hip) ----
// rows of more than kMaxRowLen entries out of a row-wise matrix: fills G's long-row arrays, returns the matrix without them
bool device_strip_long_rows(LayoutScratch& S, GatherMatrix& G, int nrows, const int* dptr, const int* didx, const double* dval,
                            DevBuf<int>& sptr, DevBuf<int>& sidx, DevBuf<double>& sval, int64_t* nnz_short, hipStream_t s);
bool device_build_sliced(LayoutScratch& S, SlicedMatrix& out, int nrows, int ncols, int64_t nnz, const int* dptr, const int* didx,
                         const double* dval, hipStream_t s, int ns_request = 0);
bool device_build_sorted_fused(LayoutScratch& S, SortedMatrix& out, int nrows, int ncols, int64_t nnz, const int* dptr, const int* didx,
                               const double* dval, hipStream_t s);
bool device_build_acc_fused(LayoutScratch& S, AccMatrix& out, int nrows, int ncols, int64_t nnz, const int* dptr, const int* didx,
                            const double* dval, hipStream_t s);
bool device_build_acc(LayoutScratch& S, AccMatrix& out, const SlicedMatrix& sliced, int nrows, int ncols, int64_t nnz, const int* dptr,
                      const int* didx, const double* dval, hipStream_t s);
// the persistent tile kernel's step table from A.tile_batch / A.bptr on the device (internal.hpp); the tail of both builders
void acc_build_steps(AccMatrix& A, int64_t ntiles, int64_t nnz, bool wide, hipStream_t s);

// ---- reorder.hip: the locality-recovering renumbering (SURVEY section 7 / 8d "row/column reordering ... a pure permutation") ----
void reorder_model(Context* c);
void reorder_permute_rows(Context* c, const double* in_old, double* out_new);      // out_new[i'] = in_old[rowperm[i']]
void reorder_unpermute_rows(Context* c, const double* in_new, double* out_old);    // out_old[rowperm[i']] = in_new[i']
void reorder_permute_weights(Context* c, const double* W_old, double* W_new);      // n structural by colperm, m slack by rowperm

// dense_inverse.hip
void dense_lu_inverse(Context* c, int kb, const double* D, const double* invL, const double* invU, double* X, double* Xt, int refine = 0);

enum TimeKind { kTimeOp = 0, kTimePrecond = 1, kTimeB = 2, kTimeBt = 3, kNumTimeKinds = 4 };
void time_mark(Context* c, int kind, bool begin);      // no-op unless timing is active
void time_start(Context* c, ipxk_times* times);        // called by a solve before it enqueues work
void time_collect(Context* c, ipxk_times* times);      // after the solve's stream sync

// ---- spmv.hip ----
void normal_apply_dev(Context* c, const double* W, const double* rhs, double* lhs, int* ndot,
                      const int* done);
float time_normal_pair(Context* c, GatherMatrix& Ac, GatherMatrix& Ar);     // microseconds of the two products
void debug_single_pass(Context* c, int which, const double* x, double* out);

// ---- precond.hip ----
void prepare_dense_columns(Context* c);   // model-dependent part of the dense-column preconditioner (precond.hip)
void reset_dense_columns(Context* c);     // drops what was built from an earlier classification
void diag_factorize_dev(Context* c, const double* W, bool precond_dense_cols, ipxint* errflag);
// lhs = P rhs; partial dot rhs'lhs -> part(slot); returns # partials.  grid > 0: that many workgroups (hence partials) for
// the diagonal form, so that a caller's own kernels can produce the same partials (cr.hip); 0: vec_grid(m)
int diag_apply_dev(Context* c, const double* rhs, double* lhs, int slot, const int* done, int grid = 0);

// ---- cr.hip ----
struct CrResult { ipxint iter; ipxint errflag; };
CrResult pcr_solve_dev(Context* c, const double* rhs, double tol, const double* resscale,
                       ipxint maxiter, double* lhs, bool lhs_is_zero, ipxk_interrupt_fn interrupt,
                       void* user, double* hist_host, ipxint hist_cap, ipxk_times* times);
CrResult cr_solve_dev(Context* c, const double* rhs, double tol, const double* resscale,
                      ipxint maxiter, double* lhs, bool lhs_is_zero, ipxk_interrupt_fn interrupt,
                      void* user, double* hist_host, ipxint hist_cap, ipxk_times* times);
double reduce_partials_host(Context* c, int slot, int count, bool is_max);
void cr_diagnostics_dev(Context* c, ipxk_cr_diag* out);
void cr_loop_stats_dev(const Context* c, ipxint out[4]);
// partitioned runs: finalize this rank's partials of `slot`, all-gather, return the per-rank view
struct PartRef publish_scalar(Context* c, int slot, int count, int op);
// finalize this rank's partials of `slot`, all-reduce the scalar; returns a one-element view
struct PartRef allreduce_scalar(Context* c, int slot, int count, int op);

// ---- newton.hip ----
CrResult newton_solve_dev(Context* c, bool use_basis, const double* rb, const double* rc, const double* rl,
                          const double* ru, const double* sl, const double* su, const double* xl, const double* xu,
                          const double* zl, const double* zu, const unsigned char* state, double tol,
                          ipxint maxiter, double* dx, double* dxl, double* dxu, double* dy, double* dzl,
                          double* dzu, ipxk_interrupt_fn interrupt, void* user, ipxk_times* times);

// ---- iterate.hip ----
void iterate_update_dev(Context* c, double sp, const double* dx, const double* dxl, const double* dxu, double sd,
                        const double* dy, const double* dzl, const double* dzu);
void iterate_residuals_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub,
                           double* rb, double* rc, double* rl, double* ru, double* presidual, double* dresidual);
void iterate_complementarity_dev(Context* c, double out4[4], double* num_terms = nullptr);
// the scalars of the iterate at one point of the IPM, on a column-partitioned context from ONE all-gather
enum IterWhat : unsigned { kIterResiduals = 1, kIterComplementarity = 2, kIterObjectives = 4 };
struct IterScalars {
    double presidual = 0, dresidual = 0;
    double comp[4] = {0, 0, 0, 0};      // complementarity, mu, mu_min, mu_max
    double num_terms = 0;
    double obj[3] = {0, 0, 0};          // pobjective, dobjective, offset
};
void iterate_scalars_dev(Context* c, unsigned what, const double* b, const double* cc, const double* lb, const double* ub,
                         double* rb, double* rc, double* rl, double* ru, IterScalars* out);
// the step-to-boundary problems of xl, xu, zl, zu over all ranks of a column partition (iterate.hip)
struct BoundaryVectors { const double *xl, *dxl, *zl, *dzl, *xu, *dxu, *zu, *dzu; };
struct Boundary { double alpha, index, x, dx, z, dz; };   // index: global, -1 if nothing blocks
void steps_to_boundary(Context* c, const BoundaryVectors& V, double alpha0, Boundary out[4]);
// column partition: row[k] (this rank's values) <- their combination over the ranks, one all-gather (iterate.hip); no-op
// on any other context
enum CombineOp { kCombineSum, kCombineMax, kCombineMin };
void combine_over_ranks(Context* c, double* row, const CombineOp* ops, int k);
// whether this rank's (n+m)-vectors include the replicated slack entries in its reductions (rank 0 of a column partition)
bool with_replicated(const Context* c);
void iterate_objectives_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub, double out3[3]);
// rb = b - AI x for an (n+m)-vector x on the device (column partition: one all-reduce of m; rb replicated)
void residual_rb(Context* c, const double* b, const double* x, double* rb);
void model_norms_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub, double out2[2]);
double step_to_boundary_dev(Context* c, const double* x, const double* dx, int64_t len, double alpha0,
                            ipxint* blocking);

// ---- ipm_step.hip ----
// pre: residuals (in ipm[0..3]) and complementarity of the current iterate when the caller has them; comp_after: the
// complementarity after the step
void ipm_step_dev(Context* c, bool use_basis, const double* b, const double* cc, const double* lb, const double* ub,
                  double kkt_tol, ipxint maxiter, ipxk_ipm_step_info* info, ipxk_interrupt_fn interrupt, void* user,
                  const IterScalars* pre = nullptr, double* comp_after = nullptr);

void ipm_driver_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub,
                    const ipxk_ipm_params* prm, ipxk_ipm_info* info, ipxk_interrupt_fn interrupt, void* user,
                    bool use_basis = false, ipxint* basis_out = nullptr, ipxint* status_out = nullptr);

// column partition: fingerprint of b and the slack parts of c, lb, ub (device), what the ranks of the device IPM agree on
uint64_t model_fingerprint(Context* c, const double* b, const double* cc, const double* lb, const double* ub);

// ---- finish.hip ----
// before a new iterate is loaded: a live basis belongs to the iterate it was built from, and so does the postprocessing
inline void begin_new_iterate(Context* c) {
    c->sb.clear();
    c->drv.clear();
    c->postprocessed = false;
}
// every call that advances the iterate refuses a postprocessed one with this
constexpr const char* kPostprocessedRefusal =
    "the resident iterate has been postprocessed (ipxk_iterate_postprocess) and no longer advances: load an iterate again "
    "(ipxk_iterate_set, ipxk_ipm_starting_point or ipxk_ipm_load_starting_point)";
void iterate_postprocess_dev(Context* c, const double* cc, const double* lb, const double* ub);
// out2 = pres, dres of Iterate::ResidualsFromDropping, over all ranks of a column partition
void iterate_dropping_residuals_dev(Context* c, const double* lb, const double* ub, double out2[2]);
void iterate_drop_to_complementarity_dev(Context* c, const double* lb, const double* ub, double* x, double* y, double* z);
void ipm_solve_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub, const ipxk_solve_params* prm,
                   ipxk_solve_info* info, ipxint* basis_out, ipxint* status_out, ipxk_interrupt_fn interrupt, void* user);

// ---- starting_basis.hip ----
void ipm_starting_basis_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub,
                            const ipxk_starting_basis_params* prm, ipxk_starting_basis_info* info, ipxint* basis_out,
                            ipxint* status_out, ipxint* log, ipxint log_cap, ipxk_interrupt_fn interrupt, void* user);
// Iterate::ScalingFactor of every variable into d[n+m] (device); *nonbarrier (device) is set when a variable is fixed or free
void iterate_scaling_factors_dev(Context* c, double* d, int* nonbarrier);

// ---- drop.hip ----
// One DropPrimal + DropDual pass (src/kkt_solver_basis.cc:196-387) on the resident iterate and the basis (basis[m], status[n+m],
// colscale[n+m], host; updated in place) whose factors and operator the context holds -- fresh, or with Maxvolume's kept etas
// behind them.  The caller has taken the gate (:36).  On return the context holds the operator of the basis returned.
void ipm_drop_dev(Context* c, std::vector<ipxint>& basis, std::vector<ipxint>& status, std::vector<double>& colscale,
                  ipxk_drop_info* info, ipxint* log, ipxint log_cap, ipxk_interrupt_fn interrupt, void* user);
// ipxk_ipm_drop_degenerate: the gate, the scaling factors and the pass on the context's live basis
void ipm_drop_degenerate_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub, ipxk_drop_info* info,
                             ipxint* basis_out, ipxint* status_out, double* colscale_out, ipxint* log, ipxint log_cap,
                             ipxk_interrupt_fn interrupt, void* user);
// the first variable in IPXK_STATE_IMPLIED_* whose xl, xu, zl, zu break Iterate::assert_consistency, -1: none (ipxk_iterate_set)
int64_t iterate_check_implied_dev(Context* c);

// ---- crossover.hip ----
// Crossover::PushDual / PushPrimal, Basis::ComputeBasicSolution and LpSolver::RunCrossover in solver form.  Vectors on the device;
// basis (in/out), variables, fixed_at_bound, statuses_out and log on the host.  Each factorizes the given basis at entry and leaves
// fresh factors of the basis returned.
void crossover_push_dual_dev(Context* c, const double* lb, const double* ub, const double* x, double* y, double* z, const ipxint* variables,
                             ipxint num_variables, ipxint* basis, const ipxk_crossover_params* prm, ipxk_crossover_info* info, ipxint* log,
                             ipxint log_cap, ipxk_interrupt_fn interrupt, void* user);
void crossover_push_primal_dev(Context* c, const double* lb, const double* ub, double* x, const ipxint* variables, ipxint num_variables,
                               const unsigned char* fixed_at_bound, ipxint* basis, const ipxk_crossover_params* prm, ipxk_crossover_info* info,
                               ipxint* log, ipxint log_cap, ipxk_interrupt_fn interrupt, void* user);
void crossover_basic_solution_dev(Context* c, const double* b, const double* cc, const ipxint* basis, double* x, double* y, double* z);
void crossover_run_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub, const double* weights, ipxint* basis,
                       const ipxk_crossover_params* prm, ipxk_crossover_info* info, double* x, double* y, double* z, ipxint* statuses_out,
                       ipxint* log, ipxint log_cap, ipxk_interrupt_fn interrupt, void* user);

// ---- start.hip ----
// IPM::ComputeStartingPoint (the model vectors on the device; b, c, lb, ub checked) and IPM::LoadStartingPoint (the
// six iterate vectors already copied into it_*; lb, ub on the device)
void ipm_starting_point_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub,
                            const ipxk_ipm_params* prm, ipxk_ipm_info* info, ipxk_interrupt_fn interrupt, void* user);
void ipm_load_starting_point_dev(Context* c, const double* lb, const double* ub);

// ---- kkt_diag.hip ----
void kkt_diag_factorize_dev(Context* c, const double* xl, const double* xu, const double* zl,
                            const double* zu, double mu, bool precond_dense_cols, ipxint* errflag);
CrResult kkt_diag_solve_dev(Context* c, const double* a, const double* b, double tol,
                            ipxint maxiter, double* x, double* y, ipxk_interrupt_fn interrupt,
                            void* user, ipxk_times* times);

// ---- trisolve.hip (the operator), sweep.hip (forward_ / backward_solve_dev, split_levels, check_sweep_abort), kkt_basis.hip ----
void split_prepare_host(Context* c, const ipxint* Lp, const ipxint* Li, const double* Lx,
                        const ipxint* Up, const ipxint* Ui, const double* Ux, const ipxint* rowperm,
                        const ipxint* colperm, const ipxint* basis, const ipxint* status,
                        const double* colscale);
// lhs = C rhs (device vectors), dot partials -> part(kPartCdot); returns # partials
int split_apply_dev(Context* c, const double* rhs, double* lhs, const int* done);
void split_rescale_host(Context* c, const ipxint* status, const double* colscale);
// raises unless the split operator was prepared under the context's current partition (trisolve.hip)
void split_check_partition(const Context* c);
// the device LU, the Prepare from it and Maxvolume on a partitioned context
constexpr const char* kDeviceLuRefusal =
    "the device LU (and the Prepare and Maxvolume that use it) does not run on a partitioned system: factorize the basis "
    "identically for every rank and pass the factors to ipxk_split_prepare";
// the operator follows Maxvolume's exchanges without new factors (Context::etas_live): the basis by position (device), its statuses and scaling
void split_follow_basis(Context* c, const ipxint* basis_dev, const ipxint* status, const double* colscale);
// out = inverse(B) in / inverse(B') in on the (scaled) factors; in may be out
void forward_solve_dev(Context* c, const double* in, double* out, bool scaled, const int* done);
void backward_solve_dev(Context* c, const double* in, double* out, bool scaled, const int* done);
void solve_dense_dev(Context* c, const double* rhs, double* lhs, char trans);
CrResult kkt_basis_solve_dev(Context* c, const double* a, const double* b, double tol,
                             ipxint maxiter, double* x, double* y, ipxk_interrupt_fn interrupt,
                             void* user, ipxk_times* times);
void split_levels(const Context* c, ipxint levels[4]);
void check_sweep_abort(Context* c);
void destroy_split(SplitOperator*);
void destroy_prepare_host(PrepareHost*);

// ---- lu.hip ----
void lu_factorize_host(Context* c, int64_t dim, const ipxint* Bbegin, const ipxint* Bend, const ipxint* Bi,
                       const double* Bx, double pivottol, bool strict, ipxk_lu_info* info);
void lu_factorize_basis(Context* c, const ipxint* basis, double pivottol, bool strict, ipxk_lu_info* info);
void lu_get_factors(Context* c, ipxint* Lp, ipxint* Li, double* Lx, ipxint* Up, ipxint* Ui, double* Ux,
                    ipxint* rowperm, ipxint* colperm, ipxint* dependent);
void split_prepare_lu(Context* c, const ipxint* status, const double* colscale);
void destroy_lu(LuState*);
void lu_invalidate(Context* c);          // the factors of an earlier factorization are no longer handed out
// ---- maxvolume.hip ----
void maxvolume_dev(Context* c, const ipxint* status, const double* colscale, const ipxk_maxvolume_params* prm,
                   ipxint* basis_out, ipxint* status_out, ipxk_maxvolume_info* info, ipxint* log, ipxint log_cap);
void maxvolume_sequential_dev(Context* c, const ipxint* status, const double* colscale, double volume_tol, ipxint maxpasses,
                              ipxint max_etas, ipxint* basis_out, ipxint* status_out, ipxk_maxvolume_info* info, ipxint* log,
                              ipxint log_cap);
void destroy_maxvol(MaxvolState*);
// ---- basis.hip (EtaFile, DeviceBasis: internal.hpp) ----
bool tighten_pivottol(double& pivottol);                            // Basis::TightenLuPivotTol; false at the top of the ladder
void mv_scatter_column(Context* c, const MvScalars* S, double* rhs);       // rhs[m] = column S->jn of AI
void mv_unit_vector(Context* c, const MvScalars* S, double* v);            // v[m] = e_(S->pmax)
void mv_pivot_from_row(Context* c, const double* btran, MvScalars* S);     // S->pivot_row = btran' a_(S->jn)
void maxvol_apply_etas(Context* c, bool transposed, double* v);     // v (by basis position) <- inverse(E_K ... E_1) v  /  its transpose
const ipxint* maxvol_current_basis(Context* c);                     // device, by basis position: the basis factors + etas stand for
void maxvol_drop_etas(Context* c);                                  // a new factorization / operator: the eta file is history
void destroy_nmatrix(NMatrix*);
void nmatrix_invalidate(Context* c);
// N = the NONBASIC columns of A with nonzero weight as a pair of gather matrices built on the device (nmatrix.hip):
// prepare returns false when N is not used for this model; apply: work = W_I .* u + N (W_N .* (N' u))
bool nmatrix_prepare(Context* c, const double* W);
void nmatrix_apply(Context* c, const double* WI, const double* u, double* work, const int* done);
// ---- presolve.hip (the resident routine; stand-alone wrappers on host arrays, no context) ----
template <class P>
void equilibrate_resident(int64_t m, int64_t n, int64_t nz, const P* dAp, const int* dAi, double* dAx, double* cs, double* rs,
                          ipxint* rounds, hipStream_t s);
void equilibrate_device(int device, int64_t m, int64_t n, const ipxint* Ap, const ipxint* Ai, double* Ax,
                        double* colscale, double* rowscale, ipxint* rounds);
void transpose_device(int device, int64_t m, int64_t n, const ipxint* Ap, const ipxint* Ai, const double* Ax,
                      ipxint* Tp, ipxint* Ti, double* Tx);

// ---- user_model.hip: an LP in user form, presolved on the device into a context it owns ----
struct Lp;
Lp* lp_create(int64_t num_constr, int64_t num_var, const ipxint* Ap, const ipxint* Ai, const double* Ax, const double* rhs,
              const char* constr_type, const double* obj, const double* lb, const double* ub, const ipxk_lp_params* prm,
              ipxk_lp_info* info);
void lp_destroy(Lp* lp);
Context* lp_context(Lp* lp);
void lp_get_model(Lp* lp, ipxint* Ap, ipxint* Ai, double* Ax, double* b, double* c, double* lb, double* ub, double* colscale,
                  double* rowscale);
void lp_solve(Lp* lp, const ipxk_solve_params* prm, ipxk_solve_info* info, ipxk_interrupt_fn interrupt, void* user);
// the seven user-form vectors of the resident iterate, on the device: x, xl, xu [num_var], slack, y [num_constr], zl, zu [num_var]
void lp_postsolve_dev(Lp* lp, const double* out[7]);
void lp_dims(const Lp* lp, int64_t* num_constr, int64_t* num_var);
void lp_evaluate(Lp* lp, ipxk_lp_eval* out);
void lp_get_residuals(Lp* lp, double* rb, double* rc);
// Presolver::PostsolveBasicSolution of a solver-form point: doubles on the device, statuses on the host; outputs may be null
struct LpBasicPoint { double *x, *slack, *y, *z; ipxint *cbasis, *vbasis; };
void lp_postsolve_basic(Lp* lp, const double* x_solver, const double* y_solver, const double* z_solver, const ipxint* statuses,
                        const LpBasicPoint& out);
void lp_crossover(Lp* lp, const ipxk_crossover_params* prm, ipxk_crossover_info* info, ipxk_lp_basic_eval* eval,
                  ipxk_interrupt_fn interrupt, void* user);
// UserModel::EvaluateBasicPoint of a user-form point: doubles on the device, vbasis on the host
void lp_evaluate_basic(Lp* lp, const double* x, const double* slack, const double* y, const double* z, const ipxint* vbasis,
                       ipxk_lp_basic_eval* out);
// the stored vertex, on the device (x, slack, y, z) and on the host (cbasis, vbasis); throws when there is none
void lp_basic_solution(Lp* lp, const double* out[4], const ipxint** cbasis, const ipxint** vbasis);
void lp_get_basis(Lp* lp, ipxint* cbasis, ipxint* vbasis);

// ---- comm.hip ----
void comm_allreduce_sum(Context* c, double* buf, size_t count);
void comm_allreduce_max(Context* c, double* buf, size_t count);
void comm_allgather(Context* c, const double* send, double* recv, size_t count_per_rank);
bool comm_active(const Context* c);      // more than one rank (or forced for testing)
bool comm_rows(const Context* c);        // active communicator, row partition
bool comm_cols(const Context* c);        // active communicator, column partition
void comm_allreduce_min(Context* c, double* buf, size_t count);
void comm_destroy(Context* c);
void comm_check(Context* c);             // raises if a collective of the direct transport timed out
double* comm_stage(Context* c, size_t count);
void comm_allreduce_sum_staged(Context* c, double* dst, size_t count);
// dst = sum over the ranks of what produce(out) writes to out: the direct exchange's buffer where it offers one
template <class F>
void allreduce_product(Context* c, double* dst, size_t count, F produce) {
    double* stage = comm_stage(c, count);
    produce(stage ? stage : dst);
    if (stage) comm_allreduce_sum_staged(c, dst, count);
    else comm_allreduce_sum(c, dst, count);
}
// all-gather of one row of k doubles per rank (device); returns the nranks x k table, rank-major, on the host
std::vector<double> comm_gather_table(Context* c, const double* row_dev, size_t k);

// fingerprint of the arguments every rank must hold identically
struct Fingerprint {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    void mix(uint64_t w) { h ^= w; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; }
    template <class T> void add(const T* p, size_t count) {
        const size_t len = count * sizeof(T);
        const unsigned char* b = reinterpret_cast<const unsigned char*>(p);
        size_t i = 0;
        for (; i + 8 <= len; i += 8) { uint64_t w; memcpy(&w, b + i, 8); mix(w); }
        if (i < len) { uint64_t w = 0; memcpy(&w, b + i, len - i); mix(w); }
        mix((uint64_t)len);
    }
};
// The ranks fail or proceed together, so that no rank enters a later collective alone: this rank's verdict (err empty:
// accepted) and fingerprint h go through one all-reduce.  Throws IPXK_E_ARGUMENT on every rank if any rank refused or the
// fingerprints differ; `who` names the call, `what` the replicated arguments.
void agree_on_arguments(Context* c, const std::string& err, uint64_t h, const char* who, const char* what);
// column partition: this rank's first structural column and the structural columns of all ranks (Context::col_offset,
// n_global), one all-gather at the first call that needs them; 0 and n on any other context
void learn_col_offsets(Context* c);

}  // namespace ipxk

struct ipxk_context : ipxk::Context {};
