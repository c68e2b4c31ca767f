// An LP in user form on the device (include/ipx_kkt_hip.h, "user model"):
//   UserModel::CopyInput / CheckVectors / CheckMatrix     reference src/user_model.cc:217-303
//   SparseMatrix::LoadFromArrays                          src/sparse_matrix.cc:49-69
//   Presolver::ComputeUserModelAttributes                 src/presolver.cc:118-133
//   Presolver::LoadPrimal / LoadDual / ScaleModel         :135-180, :182-264, :266-292
//   Presolver::PostsolveInteriorPoint                     :618-793
//   UserModel::EvaluateInteriorPoint / ComputeNorms       src/user_model.cc:99-171, :306-316
//   Presolver::PostsolveBasicSolution / PostsolveBasis    src/presolver.cc:92-116, :566-616, :795-867
//   UserModel::EvaluateBasicPoint                         src/user_model.cc:173-211
//   LpSolver::RunCrossover's tail, GetBasis               src/lp_solver.cc:64-67, :212-244, :524-536
// The caller's arrays are uploaded once; validation, the attributes, the solver form, its scaling and the context's matrix
// are built from the resident copies, and only scalars, counts and the flag / result blocks come back to the host.  The
// solver form is sign flips, copies and powers of two, so it equals the reference's bit for bit; the postsolve applies
// the reference's operation to the reference's operands, entry by entry.
#include <climits>
#include <cmath>

#include "layout_scratch.hpp"

namespace ipxk {

struct Lp {
    ipxk_context* ctx = nullptr;
    int64_t num_constr = 0, num_var = 0;
    bool dualized = false;
    int64_t num_boxed = 0, num_flipped = 0;
    // the user model (unscaled): vectors, A as LoadFromArrays leaves it (no explicit zeros, a column's entries in ascending row
    // order) and by rows (Transpose: a row's entries in ascending column order)
    DevBuf<double> rhs, obj, lbu, ubu;
    DevBuf<unsigned char> ctype;
    DevBuf<int> uAp, uAi, uTp, uTi;
    DevBuf<double> uAx, uTx;
    DevBuf<int> boxed, flipped;                  // index lists, ascending
    // the solver form: b [m], c, lb, ub [n + m], scaling factors (1.0 where the reference's vectors are empty)
    DevBuf<double> b, c, lb, ub, colscale, rowscale;
    // the postsolved point (x, xl, xu, zl, zu [num_var]; slack, y [num_constr]) and the evaluation's residuals and partials
    DevBuf<double> px, pxl, pxu, pslack, py, pzl, pzu, rb, rc, part, result;
    bool evaluated = false;
    // the last ipxk_lp_solve: whether there was one, its status, and the basis it left (empty: none was built)
    bool solved = false;
    ipxint status_ipm = 0;
    std::vector<ipxint> basis;
    // the basic solution of the last ipxk_lp_crossover: x, z [num_var], slack, y [num_constr]; its statuses on the host
    DevBuf<double> vx, vslack, vy, vz;
    std::vector<ipxint> cbasis, vbasis;
    bool has_vertex = false;
    // work space of the basic postsolve: the solver-form statuses and the user-form ones, the first violations of the asserts
    DevBuf<ipxint> st_solver, st_cbasis, st_vbasis;
    DevBuf<long long> st_part, st_first;
    ~Lp() { if (ctx) { (void)hipSetDevice(ctx->device); (void)hipStreamSynchronize(ctx->stream); delete ctx; } }
};

namespace {

constexpr long long kNoIndex = LLONG_MAX;
constexpr int kFlagGrid = 1024;                  // partials per check: the grid of every checking kernel is at most this
constexpr int kNumChecks = 8;                    // the reference's checks -1 .. -8 are slots 0 .. 7
constexpr int kNumSlots = kNumChecks + 1;        // slot 8: the first entry that LoadFromArrays drops or moves
constexpr int kEvalGrid = 1024;
enum EvalSlot { kRowMaxRb, kRowMaxY, kRowMaxRhs, kRowRhsY, kRowYSlack, kVarMaxRc, kVarMaxBound, kVarMaxX, kVarMaxZ, kVarMaxObj,
                kVarMaxBounds, kVarObjX, kVarBoundZ, kVarComp, kNumEvalSlots };
__host__ __device__ constexpr bool eval_is_max(int slot) { return slot <= kRowMaxRhs || (slot >= kVarMaxRc && slot <= kVarMaxBounds); }

size_t atleast1(int64_t n) { return (size_t)std::max<int64_t>(n, 1); }

// the workgroup's smallest index (kNoIndex: none), wavefront trees and then the wavefronts in order; valid in thread 0.  A minimum
// of integers does not depend on the order it is taken in.
__device__ __forceinline__ long long block_first(long long v) {
    __shared__ long long sh[kBlock / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const long long o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
    __syncthreads();                             // sh may still be read by an earlier call
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < kBlock / 64; k++) v = sh[k] < v ? sh[k] : v;
    return v;
}
__device__ __forceinline__ void put_first(long long* part, int check, long long v) {
    v = block_first(v);
    if (threadIdx.x == 0) part[check * kFlagGrid + blockIdx.x] = v;
}
__device__ __forceinline__ void note(long long& first, int64_t i) { if (i < first) first = i; }

// CheckVectors (src/user_model.cc:217-238): checks -1 .. -4, and CheckMatrix's -5 on the column pointers (:243-247)
__global__ __launch_bounds__(kBlock) void check_vectors_kernel(int64_t nc, int64_t nv, const double* __restrict__ rhs,
                                                               const unsigned char* __restrict__ ctype, const double* __restrict__ obj,
                                                               const double* __restrict__ lb, const double* __restrict__ ub,
                                                               const ipxint* __restrict__ Ap, long long* part) {
    long long f1 = kNoIndex, f2 = kNoIndex, f3 = kNoIndex, f4 = kNoIndex, f5 = kNoIndex;
    IPXK_GRID_STRIDE(i, nc) {
        if (!isfinite(rhs[i])) note(f1, i);
        const unsigned char t = ctype[i];
        if (t != '=' && t != '<' && t != '>') note(f4, i);
    }
    IPXK_GRID_STRIDE(j, nv) {
        if (!isfinite(obj[j])) note(f2, j);
        const double l = lb[j], u = ub[j];
        if ((!isfinite(l) && l != -INFINITY) || (!isfinite(u) && u != INFINITY) || l > u) note(f3, j);
        if ((j == 0 && Ap[0] != 0) || Ap[j] > Ap[j + 1]) note(f5, j);
    }
    put_first(part, 0, f1); put_first(part, 1, f2); put_first(part, 2, f3); put_first(part, 3, f4); put_first(part, 4, f5);
}
// :248-250 and the range test of :256: checks -6 and -7 by position; the narrowed row index, an index out of range as
// row nc (a row of its own behind the matrix, so that the sort by row below stays defined)
__global__ __launch_bounds__(kBlock) void check_entries_kernel(int64_t nz, int64_t nc, const ipxint* __restrict__ Ai64,
                                                               const double* __restrict__ Ax, int* __restrict__ Ai, long long* part) {
    long long f6 = kNoIndex, f7 = kNoIndex;
    IPXK_GRID_STRIDE(p, nz) {
        if (!isfinite(Ax[p])) note(f6, p);
        const ipxint i = Ai64[p];
        const bool bad = i < 0 || i >= nc;
        if (bad) note(f7, p);
        Ai[p] = bad ? (int)nc : (int)i;
    }
    put_first(part, 5, f6); put_first(part, 6, f7);
}
// :258-260, whatever the order of a column's entries: in the row-wise copy (a row's entries in ascending column order, equal
// columns next to each other) two neighbours with the same column are a row index that occurs twice in that column; the
// reference stops at the second occurrence, which is looked up in the column.
__global__ __launch_bounds__(kBlock) void check_duplicates_kernel(int64_t nc, const int* __restrict__ Tp, const int* __restrict__ Ti,
                                                                  const int* __restrict__ Ap, const int* __restrict__ Ai, long long* part) {
    long long f8 = kNoIndex;
    IPXK_GRID_STRIDE(i, nc)
        for (int t = Tp[i] + 1; t < Tp[i + 1]; t++) {
            if (Ti[t] != Ti[t - 1]) continue;
            const int j = Ti[t];
            int seen = 0;
            for (int p = Ap[j]; p < Ap[j + 1]; p++)
                if (Ai[p] == (int)i && ++seen == 2) { note(f8, p); break; }
        }
    put_first(part, 7, f8);
}
// first[k] = the smallest partial of check k; one workgroup per check
__global__ __launch_bounds__(kBlock) void first_index_kernel(const long long* __restrict__ part, long long* first) {
    long long v = kNoIndex;
    for (int g = threadIdx.x; g < kFlagGrid; g += kBlock) { const long long o = part[blockIdx.x * kFlagGrid + g]; v = o < v ? o : v; }
    v = block_first(v);
    if (threadIdx.x == 0) first[blockIdx.x] = v;
}

// LoadFromArrays (src/sparse_matrix.cc:49-69) drops explicit zeros and sorts every column by row index.  Slot 8: the first
// entry that is an explicit zero or whose row index is below its predecessor's in the same column (none: nothing to do, the
// reference's IsSorted).
__global__ __launch_bounds__(kBlock) void check_loaded_kernel(int64_t nz, const int* __restrict__ colof, const int* __restrict__ Ai,
                                                              const double* __restrict__ Ax, long long* part) {
    long long f = kNoIndex;
    IPXK_GRID_STRIDE(p, nz)
        if (Ax[p] == 0.0 || (p > 0 && colof[p - 1] == colof[p] && Ai[p - 1] > Ai[p])) note(f, p);
    put_first(part, kNumChecks, f);
}
__global__ void nonzero_mask_kernel(int64_t nz, const double* __restrict__ Ax, int* __restrict__ mask) {
    IPXK_GRID_STRIDE(p, nz + 1) mask[p] = p < nz && Ax[p] != 0.0;
}
// the entries with mask 1 move to pos[] (the exclusive prefix sums of mask, nz + 1 of them), the column pointers follow
__global__ void compact_entries_kernel(int64_t nz, int64_t ncol, const int* __restrict__ mask, const int* __restrict__ pos,
                                       const int* __restrict__ Ai, const double* __restrict__ Ax, int* Ap, int* __restrict__ Ai_out,
                                       double* __restrict__ Ax_out) {
    IPXK_GRID_STRIDE(p, nz) if (mask[p]) { Ai_out[pos[p]] = Ai[p]; Ax_out[pos[p]] = Ax[p]; }
    IPXK_GRID_STRIDE(j, ncol + 1) Ap[j] = pos[Ap[j]];
}

// ComputeUserModelAttributes (:118-133) and the flipped variables of LoadDual (:195-201) as 0/1 masks
__global__ void attribute_masks_kernel(int64_t nc, int64_t nv, const unsigned char* __restrict__ ctype, const double* __restrict__ lb,
                                       const double* __restrict__ ub, int* __restrict__ is_eq, int* __restrict__ is_free,
                                       int* __restrict__ is_boxed, int* __restrict__ is_flipped) {
    IPXK_GRID_STRIDE(i, nc) is_eq[i] = ctype[i] == '=';
    IPXK_GRID_STRIDE(j, nv) {
        const bool has_lb = isfinite(lb[j]), has_ub = isfinite(ub[j]);
        is_free[j] = !has_lb && !has_ub;
        is_boxed[j] = has_lb && has_ub;
        is_flipped[j] = isinf(lb[j]) && has_ub;
    }
}
__global__ void mask_count_kernel(int64_t len, const int* __restrict__ mask, const int* __restrict__ pos, int* count) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = len > 0 ? pos[len - 1] + mask[len - 1] : 0;
}
__global__ void mask_list_kernel(int64_t len, const int* __restrict__ mask, const int* __restrict__ pos, int* __restrict__ list) {
    IPXK_GRID_STRIDE(j, len) if (mask[j]) list[pos[j]] = (int)j;
}

// LoadPrimal (:155-179): c, lb, ub of the nv structural and the nc slack variables (b is a copy of rhs)
__global__ void load_primal_kernel(int64_t nc, int64_t nv, const unsigned char* __restrict__ ctype, const double* __restrict__ obj,
                                   const double* __restrict__ lbu, const double* __restrict__ ubu, double* __restrict__ c,
                                   double* __restrict__ lb, double* __restrict__ ub) {
    IPXK_GRID_STRIDE(k, nv + nc) {
        if (k < nv) { c[k] = obj[k]; lb[k] = lbu[k]; ub[k] = ubu[k]; continue; }
        const unsigned char t = ctype[k - nv];
        c[k] = 0.0;
        lb[k] = t == '>' ? -INFINITY : 0.0;
        ub[k] = t == '<' ? INFINITY : 0.0;
    }
}
// LoadDual's matrix (:203-214): A' with the rows of flipped variables negated, then one column (j, -1.0) per boxed variable
__global__ void load_dual_matrix_kernel(int64_t nc, int64_t nb, int64_t nz, const int* __restrict__ Tp, const int* __restrict__ Ti,
                                        const double* __restrict__ Tx, const int* __restrict__ is_flipped, const int* __restrict__ boxed,
                                        int* __restrict__ Ap, int* __restrict__ Ai, double* __restrict__ Ax) {
    IPXK_GRID_STRIDE(t, nz) {
        const int j = Ti[t];
        Ai[t] = j;
        Ax[t] = is_flipped[j] ? Tx[t] * -1.0 : Tx[t];
    }
    IPXK_GRID_STRIDE(k, nb) { Ai[nz + k] = boxed[k]; Ax[nz + k] = -1.0; }
    IPXK_GRID_STRIDE(i, nc + nb + 1) Ap[i] = i <= nc ? Tp[i] : (int)(nz + (i - nc));
}
// LoadDual's vectors (:221-263); n = nc + nb structural columns, nv rows
__global__ void load_dual_vectors_kernel(int64_t nc, int64_t nb, int64_t nv, const unsigned char* __restrict__ ctype,
                                         const double* __restrict__ rhs, const double* __restrict__ obj, const double* __restrict__ lbu,
                                         const double* __restrict__ ubu, const int* __restrict__ is_flipped, const int* __restrict__ boxed,
                                         double* __restrict__ b, double* __restrict__ c, double* __restrict__ lb, double* __restrict__ ub) {
    const int64_t n = nc + nb;
    IPXK_GRID_STRIDE(k, n + nv) {
        if (k < nc) {
            const unsigned char t = ctype[k];
            c[k] = -rhs[k];
            lb[k] = t == '>' ? 0.0 : -INFINITY;
            ub[k] = t == '<' ? 0.0 : INFINITY;
        } else if (k < n) {
            c[k] = ubu[boxed[k - nc]];
            lb[k] = 0.0;
            ub[k] = INFINITY;
        } else {
            const int64_t j = k - n;
            const double l = is_flipped[j] ? -ubu[j] : lbu[j];
            b[j] = is_flipped[j] ? obj[j] * -1.0 : obj[j];
            c[k] = isfinite(l) ? -l : 0.0;
            lb[k] = 0.0;
            ub[k] = isfinite(l) ? INFINITY : 0.0;
        }
    }
}
// ScaleModel (:275-291)
__global__ void scale_vectors_kernel(int64_t m, int64_t n, const double* __restrict__ cs, const double* __restrict__ rs,
                                     double* __restrict__ b, double* __restrict__ c, double* __restrict__ lb, double* __restrict__ ub) {
    IPXK_GRID_STRIDE(k, n + m) {
        if (k < n) {
            c[k] *= cs[k]; lb[k] /= cs[k]; ub[k] /= cs[k];
        } else {
            const double r = rs[k - n];
            b[k - n] *= r; c[k] /= r; lb[k] *= r; ub[k] *= r;
        }
    }
}

// ---- PostsolveInteriorPoint (:618-793) ----
struct Point { const double *x, *xl, *xu, *y, *zl, *zu; };             // the solver's iterate
struct UserPoint { double *x, *xl, *xu, *slack, *y, *zl, *zu; };
// primal branch (:732-792): n = nv, m = nc
__global__ void postsolve_primal_kernel(int64_t nc, int64_t nv, Point s, const unsigned char* __restrict__ ctype,
                                        const double* __restrict__ cs, const double* __restrict__ rs, UserPoint u) {
    IPXK_GRID_STRIDE(j, nv) {
        u.x[j] = s.x[j] * cs[j];
        u.zl[j] = s.zl[j] / cs[j];
        u.zu[j] = s.zu[j] / cs[j];
        u.xl[j] = s.xl[j] * cs[j];
        u.xu[j] = s.xu[j] * cs[j];
    }
    IPXK_GRID_STRIDE(i, nc) {
        const unsigned char t = ctype[i];
        const int64_t k = nv + i;
        u.y[i] = t == '=' ? s.y[i] * rs[i] : t == '<' ? -s.zl[k] * rs[i] : s.zu[k] * rs[i];
        u.slack[i] = t == '=' ? 0.0 : t == '<' ? s.xl[k] / rs[i] : -s.xu[k] / rs[i];
    }
}
// dualized branch (:634-719) without the boxed and flipped variables: n = nc + nb, m = nv
__global__ void postsolve_dual_kernel(int64_t nc, int64_t nb, int64_t nv, Point s, const unsigned char* __restrict__ ctype,
                                      const double* __restrict__ lb, const double* __restrict__ ub, const double* __restrict__ cs,
                                      const double* __restrict__ rs, UserPoint u) {
    const int64_t n = nc + nb;
    IPXK_GRID_STRIDE(j, nv) {
        const bool fixed = lb[n + j] == ub[n + j];
        u.x[j] = -s.y[j] * rs[j];
        u.zl[j] = fixed ? 0.0 : s.xl[n + j] / rs[j];
        u.zu[j] = 0.0;
        u.xl[j] = fixed ? INFINITY : s.zl[n + j] * rs[j];
        u.xu[j] = INFINITY;
    }
    IPXK_GRID_STRIDE(i, nc) {
        const unsigned char t = ctype[i];
        u.y[i] = t == '=' ? s.x[i] * cs[i] : t == '<' ? -s.xu[i] * cs[i] : s.xl[i] * cs[i];
        u.slack[i] = t == '=' ? 0.0 : t == '<' ? s.zu[i] / cs[i] : -s.zl[i] / cs[i];
    }
}
// :680-685, :699-704: the columns added for boxed variables carry zu and xu
__global__ void postsolve_boxed_kernel(int64_t nc, int64_t nb, Point s, const int* __restrict__ boxed, const double* __restrict__ cs, UserPoint u) {
    IPXK_GRID_STRIDE(k, nb) {
        const int j = boxed[k];
        u.zu[j] = s.xl[nc + k] * cs[nc + k];
        u.xu[j] = s.zl[nc + k] / cs[nc + k];
    }
}
// :721-730 (after the boxed columns: a flipped variable is not boxed)
__global__ void postsolve_flipped_kernel(int64_t nf, const int* __restrict__ flipped, UserPoint u) {
    IPXK_GRID_STRIDE(f, nf) {
        const int j = flipped[f];
        u.x[j] *= -1.0;
        u.xu[j] = u.xl[j];
        u.xl[j] = INFINITY;
        u.zu[j] = u.zl[j];
        u.zl[j] = 0.0;
    }
}

// ---- EvaluateInteriorPoint (src/user_model.cc:99-171) ----
__device__ __forceinline__ void put_partial(double* part, int slot, double v, bool is_max, double* scratch) {
    v = is_max ? block_reduce<MaxOp>(v, scratch) : block_reduce<SumOp>(v, scratch);
    if (threadIdx.x == 0) part[slot * kEvalGrid + blockIdx.x] = v;
}
// rb = rhs - slack - A x, a row's products subtracted in ascending column order, rhs added last (:109-114)
__global__ __launch_bounds__(kBlock) void evaluate_rows_kernel(int64_t nc, const int* __restrict__ Tp, const int* __restrict__ Ti,
                                                               const double* __restrict__ Tx, const double* __restrict__ rhs,
                                                               const double* __restrict__ x, const double* __restrict__ slack,
                                                               const double* __restrict__ y, double* __restrict__ rb, double* part) {
    __shared__ double scratch[kBlock / 64 + 1];
    double max_rb = 0.0, max_y = 0.0, max_rhs = 0.0, rhs_y = 0.0, y_slack = 0.0;
    IPXK_GRID_STRIDE(i, nc) {
        double r = 0.0;
        for (int t = Tp[i]; t < Tp[i + 1]; t++) r -= Tx[t] * x[Ti[t]];
        r -= slack[i];
        r += rhs[i];
        rb[i] = r;
        max_rb = MaxOp::apply(max_rb, fabs(r));
        max_y = MaxOp::apply(max_y, fabs(y[i]));
        max_rhs = MaxOp::apply(max_rhs, fabs(rhs[i]));
        rhs_y += rhs[i] * y[i];
        y_slack += y[i] * slack[i];
    }
    put_partial(part, kRowMaxRb, max_rb, true, scratch);
    put_partial(part, kRowMaxY, max_y, true, scratch);
    put_partial(part, kRowMaxRhs, max_rhs, true, scratch);
    put_partial(part, kRowRhsY, rhs_y, false, scratch);
    put_partial(part, kRowYSlack, y_slack, false, scratch);
}
// rc = obj - zl + zu - A'y, obj added last (:116-121); the bound residuals (:127-136), the objective terms (:138-145), the
// complementarity products (:150-156) and the norms of ComputeNorms (:306-316)
__global__ __launch_bounds__(kBlock) void evaluate_columns_kernel(int64_t nv, const int* __restrict__ Ap, const int* __restrict__ Ai,
                                                                  const double* __restrict__ Ax, const double* __restrict__ obj,
                                                                  const double* __restrict__ lb, const double* __restrict__ ub, UserPoint u,
                                                                  double* __restrict__ rc, double* part) {
    __shared__ double scratch[kBlock / 64 + 1];
    double max_rc = 0.0, max_bound = 0.0, max_x = 0.0, max_z = 0.0, max_obj = 0.0, max_bounds = 0.0, obj_x = 0.0, bound_z = 0.0, comp = 0.0;
    IPXK_GRID_STRIDE(j, nv) {
        double r = 0.0;
        for (int p = Ap[j]; p < Ap[j + 1]; p++) r -= Ax[p] * u.y[Ai[p]];
        r -= u.zl[j] - u.zu[j];
        r += obj[j];
        rc[j] = r;
        max_rc = MaxOp::apply(max_rc, fabs(r));
        if (isfinite(lb[j])) {
            max_bound = MaxOp::apply(max_bound, fabs(lb[j] - u.x[j] + u.xl[j]));
            max_bounds = MaxOp::apply(max_bounds, fabs(lb[j]));
            bound_z += lb[j] * u.zl[j];
            comp += u.xl[j] * u.zl[j];
        }
        if (isfinite(ub[j])) {
            max_bound = MaxOp::apply(max_bound, fabs(ub[j] - u.x[j] - u.xu[j]));
            max_bounds = MaxOp::apply(max_bounds, fabs(ub[j]));
            bound_z -= ub[j] * u.zu[j];
            comp += u.xu[j] * u.zu[j];
        }
        max_x = MaxOp::apply(max_x, fabs(u.x[j]));
        max_z = MaxOp::apply(max_z, fmax(fabs(u.zl[j]), fabs(u.zu[j])));
        max_obj = MaxOp::apply(max_obj, fabs(obj[j]));
        obj_x += obj[j] * u.x[j];
    }
    put_partial(part, kVarMaxRc, max_rc, true, scratch);
    put_partial(part, kVarMaxBound, max_bound, true, scratch);
    put_partial(part, kVarMaxX, max_x, true, scratch);
    put_partial(part, kVarMaxZ, max_z, true, scratch);
    put_partial(part, kVarMaxObj, max_obj, true, scratch);
    put_partial(part, kVarMaxBounds, max_bounds, true, scratch);
    put_partial(part, kVarObjX, obj_x, false, scratch);
    put_partial(part, kVarBoundZ, bound_z, false, scratch);
    put_partial(part, kVarComp, comp, false, scratch);
}
// one workgroup: every slot's partials in fixed order
__global__ __launch_bounds__(kBlock) void evaluate_finish_kernel(int grid_rows, int grid_cols, const double* __restrict__ part, double* result) {
    __shared__ double scratch[kBlock / 64 + 1];
    for (int slot = 0; slot < kNumEvalSlots; slot++) {
        const PartRef ref{part + slot * kEvalGrid, slot < kVarMaxRc ? grid_rows : grid_cols, 1};
        const double v = eval_is_max(slot) ? reduce_partials<MaxOp>(ref, scratch) : reduce_partials<SumOp>(ref, scratch);
        if (threadIdx.x == 0) result[slot] = v;
    }
}

// ---- PostsolveBasicSolution (:92-101) = PostsolveGeneralPoint (:566-616) + PostsolveBasis (:795-845) + CorrectBasicSolution
// (:847-867) ----
constexpr ipxint kBasic = 0, kNonbasic = -1, kNonbasicLb = -1, kNonbasicUb = -2, kSuperbasic = -3;      // include/ipx_status.h
struct SolverPoint { const double *x, *y, *z; const ipxint* st; };      // x, z, st [n + m], y [m]
struct BasicPoint { double *x, *slack, *y, *z; ipxint *cbasis, *vbasis; };       // any of the four doubles may be null

// The asserts of PostsolveBasis, by first index.  Slot 0: a slack variable that is superbasic (:812, :836).  Slot 1 (dualized):
// a boxed variable, by its place in the list, whose added column is basic although its own slack is basic too, which has made
// it nonbasic already (:822).  (:826 cannot fail: a flipped variable is not boxed.)
__global__ __launch_bounds__(kBlock) void check_statuses_kernel(int64_t n, int64_t m, int64_t nc, int64_t nb, const ipxint* __restrict__ st,
                                                                const int* __restrict__ boxed, long long* part) {
    long long f0 = kNoIndex, f1 = kNoIndex;
    IPXK_GRID_STRIDE(i, m) if (st[n + i] == kSuperbasic) note(f0, i);
    IPXK_GRID_STRIDE(k, nb) if (st[nc + k] == kBasic && st[n + boxed[k]] == kBasic) note(f1, k);
    put_first(part, 0, f0); put_first(part, 1, f1);
}
// primal form: n = nv, m = nc; the three steps of an entry in one pass (the correction owns x where vbasis is -1 / -2, z where it
// is basic, slack where cbasis is nonbasic and y where it is basic)
__global__ void postsolve_basic_primal_kernel(int64_t nc, int64_t nv, SolverPoint s, const double* __restrict__ cs, const double* __restrict__ rs,
                                              const double* __restrict__ lbu, const double* __restrict__ ubu, BasicPoint u) {
    IPXK_GRID_STRIDE(j, nv) {
        const ipxint vb = s.st[j];
        if (u.x) u.x[j] = vb == kNonbasicLb ? lbu[j] : vb == kNonbasicUb ? ubu[j] : s.x[j] * cs[j];
        if (u.z) u.z[j] = vb == kBasic ? 0.0 : s.z[j] / cs[j];
        u.vbasis[j] = vb;
    }
    IPXK_GRID_STRIDE(i, nc) {
        const ipxint cb = s.st[nv + i] == kBasic ? kBasic : kNonbasic;
        if (u.slack) u.slack[i] = cb == kNonbasic ? 0.0 : s.x[nv + i] / rs[i];
        if (u.y) u.y[i] = cb == kBasic ? 0.0 : s.y[i] * rs[i];
        u.cbasis[i] = cb;
    }
}
// dualized form without the boxed and flipped variables: n = nc + nb, m = nv.  The rows are final here (cbasis depends on
// nothing else); x, z and vbasis of the variables wait for the two lists and are corrected after them.
__global__ void postsolve_basic_dual_kernel(int64_t nc, int64_t nb, int64_t nv, SolverPoint s, const double* __restrict__ lb,
                                            const double* __restrict__ ub, const double* __restrict__ cs, const double* __restrict__ rs,
                                            BasicPoint u) {
    const int64_t n = nc + nb;
    IPXK_GRID_STRIDE(j, nv) {
        if (u.x) u.x[j] = -s.y[j] * rs[j];
        if (u.z) u.z[j] = s.x[n + j] / rs[j];
        u.vbasis[j] = s.st[n + j] != kBasic ? kBasic : lb[n + j] != ub[n + j] ? kNonbasicLb : kSuperbasic;
    }
    IPXK_GRID_STRIDE(i, nc) {
        const ipxint cb = s.st[i] == kBasic ? kNonbasic : kBasic;
        if (u.slack) u.slack[i] = cb == kNonbasic ? 0.0 : -s.z[i] / cs[i];
        if (u.y) u.y[i] = cb == kBasic ? 0.0 : s.x[i] * cs[i];
        u.cbasis[i] = cb;
    }
}
// :587-591, :819-824.  colscale is a power of two, so the product is exact and a fused multiply-add, were this file built with
// contraction, would give the bits of the reference's multiply and subtract.
__global__ void postsolve_basic_boxed_kernel(int64_t nc, int64_t nb, SolverPoint s, const int* __restrict__ boxed, const double* __restrict__ cs,
                                             BasicPoint u) {
    IPXK_GRID_STRIDE(k, nb) {
        const int j = boxed[k];
        if (u.z) u.z[j] -= s.x[nc + k] * cs[nc + k];
        if (s.st[nc + k] == kBasic) u.vbasis[j] = kNonbasicUb;
    }
}
// :593-596, :825-829
__global__ void postsolve_basic_flipped_kernel(int64_t nf, const int* __restrict__ flipped, BasicPoint u) {
    IPXK_GRID_STRIDE(f, nf) {
        const int j = flipped[f];
        if (u.x) u.x[j] *= -1.0;
        if (u.z) u.z[j] *= -1.0;
        if (u.vbasis[j] == kNonbasicLb) u.vbasis[j] = kNonbasicUb;
    }
}
// CorrectBasicSolution's loop over the variables, once vbasis is final
__global__ void correct_basic_kernel(int64_t nv, const double* __restrict__ lbu, const double* __restrict__ ubu, BasicPoint u) {
    IPXK_GRID_STRIDE(j, nv) {
        const ipxint vb = u.vbasis[j];
        if (u.x && vb == kNonbasicLb) u.x[j] = lbu[j];
        if (u.x && vb == kNonbasicUb) u.x[j] = ubu[j];
        if (u.z && vb == kBasic) u.z[j] = 0.0;
    }
}
// BuildBasicStatuses (src/lp_solver.cc:212-231): the nonbasic statuses from the solver form's bounds, then the basis over them
__global__ void nonbasic_statuses_kernel(int64_t N, const double* __restrict__ lb, const double* __restrict__ ub, ipxint* __restrict__ st) {
    IPXK_GRID_STRIDE(k, N) st[k] = isfinite(lb[k]) ? kNonbasicLb : isfinite(ub[k]) ? kNonbasicUb : kSuperbasic;
}
__global__ void basic_statuses_kernel(int64_t m, const ipxint* __restrict__ basis, ipxint* __restrict__ st) {
    IPXK_GRID_STRIDE(p, m) st[basis[p]] = kBasic;
}

// ---- EvaluateBasicPoint (src/user_model.cc:173-211) ----
enum BasicSlot { kBasicPrimal, kBasicDual, kBasicObjX, kNumBasicSlots };
__device__ __forceinline__ double std_max(double a, double b) { return a < b ? b : a; }      // std::max: a NaN on the right is dropped
__global__ __launch_bounds__(kBlock) void evaluate_basic_kernel(int64_t nc, int64_t nv, const double* __restrict__ lbu, const double* __restrict__ ubu,
                                                                const double* __restrict__ obj, const unsigned char* __restrict__ ctype,
                                                                const double* __restrict__ x, const double* __restrict__ slack,
                                                                const double* __restrict__ y, const double* __restrict__ z,
                                                                const ipxint* __restrict__ vbasis, double* part) {
    __shared__ double scratch[kBlock / 64 + 1];
    double pinf = 0.0, dinf = 0.0, obj_x = 0.0;
    IPXK_GRID_STRIDE(j, nv) {
        pinf = std_max(pinf, lbu[j] - x[j]);
        pinf = std_max(pinf, x[j] - ubu[j]);
        if (vbasis[j] != kNonbasicLb) dinf = std_max(dinf, z[j]);
        if (vbasis[j] != kNonbasicUb) dinf = std_max(dinf, -z[j]);
        obj_x += obj[j] * x[j];
    }
    IPXK_GRID_STRIDE(i, nc) {
        const unsigned char t = ctype[i];
        if (t == '<') { pinf = std_max(pinf, -slack[i]); dinf = std_max(dinf, y[i]); }
        else if (t == '>') { pinf = std_max(pinf, slack[i]); dinf = std_max(dinf, -y[i]); }
        else pinf = std_max(pinf, fabs(slack[i]));
    }
    put_partial(part, kBasicPrimal, pinf, true, scratch);
    put_partial(part, kBasicDual, dinf, true, scratch);
    put_partial(part, kBasicObjX, obj_x, false, scratch);
}
// one workgroup: the three slots' partials in fixed order
__global__ __launch_bounds__(kBlock) void evaluate_basic_finish_kernel(int grid, const double* __restrict__ part, double* result) {
    __shared__ double scratch[kBlock / 64 + 1];
    for (int slot = 0; slot < kNumBasicSlots; slot++) {
        const PartRef ref{part + slot * kEvalGrid, grid, 1};
        const double v = slot == kBasicObjX ? reduce_partials<SumOp>(ref, scratch) : reduce_partials<MaxOp>(ref, scratch);
        if (threadIdx.x == 0) result[slot] = v;
    }
}

// exclusive prefix sums of a 0/1 mask, the number of ones into *count (device) and their indices, ascending, into list
void list_of_mask(Tmp& T, int64_t len, const int* mask, int* pos, int* count, int* list, hipStream_t s) {
    if (len > 0) scan_int(T, mask, pos, (size_t)len, s);
    hipLaunchKernelGGL(mask_count_kernel, dim3(1), dim3(64), 0, s, len, mask, pos, count);
    if (len > 0 && list) hipLaunchKernelGGL(mask_list_kernel, dim3(gridn(len)), dim3(kBlock), 0, s, len, mask, pos, list);
}

const char* const kCheckNames[kNumChecks] = {"rhs must be finite", "obj must be finite",
                                             "bounds must be finite or the correct infinity, with lb <= ub",
                                             "constr_type must be one of = < >", "Ap must start at 0 and be monotone",
                                             "matrix values must be finite", "row index out of range", "row index twice in a column"};

// the reference's verdict from the first failing index of every check: CheckVectors' four loops in order, then Ap, the values,
// and whichever of an index out of range or a repeated one its last loop meets first (:253-262; the range is tested first)
void throw_first_failure(const long long first[kNumChecks]) {
    int k = -1;
    for (int q = 0; q < 6 && k < 0; q++)
        if (first[q] != kNoIndex) k = q;
    if (k < 0 && (first[6] != kNoIndex || first[7] != kNoIndex)) k = first[6] <= first[7] ? 6 : 7;
    if (k < 0) return;
    char buf[256];
    snprintf(buf, sizeof buf, "ipxk_lp_create: invalid model, check %d (%s), first at index %lld", -(k + 1), kCheckNames[k], first[k]);
    throw Error(IPXK_E_ARGUMENT, buf);
}

}  // namespace

Lp* lp_create(int64_t nc, int64_t nv, const ipxint* Ap, const ipxint* Ai, const double* Ax, const double* rhs, const char* constr_type,
              const double* obj, const double* lbuser, const double* ubuser, const ipxk_lp_params* prm, ipxk_lp_info* info) {
    const double t_start = now_s();
    const ipxint dualize_prm = prm ? prm->dualize : -1, scale_prm = prm ? prm->scale : 1;
    const int device = prm ? prm->device : 0;
    // CopyInput (src/user_model.cc:272-287)
    IPXK_REQUIRE(nc >= 0 && nv > 0, "invalid dimension (num_constr >= 0 and num_var > 0)");
    IPXK_REQUIRE(nc < (int64_t(1) << 30) && nv < (int64_t(1) << 30), "dimension exceeds 32-bit device indices");
    IPXK_REQUIRE(Ap && obj && lbuser && ubuser && (nc == 0 || (rhs && constr_type)), "NULL argument");
    int ndev = 0;
    IPXK_HIP(hipGetDeviceCount(&ndev));
    if (ndev <= 0) throw Error(IPXK_E_HIP, "no HIP device available (the GPU path has no CPU fallback)");
    IPXK_REQUIRE(device >= 0 && device < ndev, "device ordinal out of range");

    std::unique_ptr<Lp> lp(new Lp);
    lp->ctx = new ipxk_context;
    Context* c = lp->ctx;
    c->device = device;
    IPXK_HIP(hipSetDevice(device));
    IPXK_HIP(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    hipStream_t s = c->stream;
    lp->num_constr = nc;
    lp->num_var = nv;

    // ---- upload and validation ----
    lp->rhs.resize(atleast1(nc)); lp->ctype.resize(atleast1(nc));
    lp->rhs.upload(rhs, (size_t)nc, s);
    lp->ctype.upload(reinterpret_cast<const unsigned char*>(constr_type), (size_t)nc, s);
    lp->obj.upload(obj, (size_t)nv, s);
    lp->lbu.upload(lbuser, (size_t)nv, s);
    lp->ubu.upload(ubuser, (size_t)nv, s);
    DevBuf<ipxint> ap64;
    ap64.upload(Ap, (size_t)nv + 1, s);
    DevBuf<long long> part((size_t)kNumSlots * kFlagGrid), first_dev(kNumSlots);
    hipLaunchKernelGGL(fill_kernel<long long>, dim3(gridn(kNumSlots * kFlagGrid)), dim3(kBlock), 0, s, (int64_t)kNumSlots * kFlagGrid, kNoIndex,
                       part.get());
    hipLaunchKernelGGL(check_vectors_kernel, dim3(grid_for(std::max(nc, nv), kFlagGrid)), dim3(kBlock), 0, s, nc, nv, lp->rhs.get(),
                       lp->ctype.get(), lp->obj.get(), lp->lbu.get(), lp->ubu.get(), ap64.get(), part.get());
    hipLaunchKernelGGL(first_index_kernel, dim3(kNumSlots), dim3(kBlock), 0, s, part.get(), first_dev.get());
    long long first[kNumSlots];
    first_dev.download(first, kNumSlots, s);
    if (first[0] != kNoIndex || first[1] != kNoIndex || first[2] != kNoIndex || first[3] != kNoIndex || first[4] != kNoIndex)
        throw_first_failure(first);                 // (the entries are not looked at behind column pointers that cannot be trusted)
    int64_t nz = Ap[nv];                           // (of the caller's arrays; of the loaded matrix from LoadFromArrays on)
    IPXK_REQUIRE(nz == 0 || (Ai && Ax), "NULL argument");
    IPXK_REQUIRE(nz < (int64_t(1) << 31) - kLongSeg - nv, "nnz exceeds 32-bit device indices");
    lp->uAp.resize((size_t)nv + 1); lp->uAi.resize(atleast1(nz)); lp->uAx.resize(atleast1(nz));
    lp->uTp.resize((size_t)nc + 2); lp->uTi.resize(atleast1(nz)); lp->uTx.resize(atleast1(nz));
    narrow_ints(nv + 1, ap64.get(), lp->uAp.get(), s);
    Tmp T;
    if (nz > 0) {
        DevBuf<ipxint> ai64;
        ai64.upload(Ai, (size_t)nz, s);
        lp->uAx.upload(Ax, (size_t)nz, s);
        hipLaunchKernelGGL(check_entries_kernel, dim3(grid_for(nz, kFlagGrid)), dim3(kBlock), 0, s, nz, nc, ai64.get(), lp->uAx.get(),
                           lp->uAi.get(), part.get());
        DevBuf<int> colof;
        device_transpose(T, colof, nv, nc + 1, nz, lp->uAp.get(), lp->uAi.get(), lp->uAx.get(), lp->uTp.get(), lp->uTi.get(), lp->uTx.get(), s);
        hipLaunchKernelGGL(check_duplicates_kernel, dim3(grid_for(nc, kFlagGrid)), dim3(kBlock), 0, s, nc, lp->uTp.get(), lp->uTi.get(),
                           lp->uAp.get(), lp->uAi.get(), part.get());
        hipLaunchKernelGGL(check_loaded_kernel, dim3(grid_for(nz, kFlagGrid)), dim3(kBlock), 0, s, nz, colof.get(), lp->uAi.get(), lp->uAx.get(),
                           part.get());
        hipLaunchKernelGGL(first_index_kernel, dim3(kNumSlots), dim3(kBlock), 0, s, part.get(), first_dev.get());
        first_dev.download(first, kNumSlots, s);     // (synchronizes: ai64 goes out of scope)
        throw_first_failure(first);                  // (the positions are those of the caller's arrays)
        if (first[kNumChecks] != kNoIndex) {
            // LoadFromArrays: the row-wise copy transposed back has every column in ascending row order (no row index
            // repeats, so this is the reference's sort of (index, value) pairs); then the explicit zeros go, and the
            // row-wise copy is taken again of what is left
            DevBuf<int> sAp((size_t)nv + 1), sAi((size_t)nz), mask((size_t)nz + 1), pos((size_t)nz + 1);
            DevBuf<double> sAx((size_t)nz);
            device_transpose(T, colof, nc + 1, nv, nz, lp->uTp.get(), lp->uTi.get(), lp->uTx.get(), sAp.get(), sAi.get(), sAx.get(), s);
            hipLaunchKernelGGL(nonzero_mask_kernel, dim3(gridn(nz + 1)), dim3(kBlock), 0, s, nz, sAx.get(), mask.get());
            scan_int(T, mask.get(), pos.get(), (size_t)nz + 1, s);
            hipLaunchKernelGGL(compact_entries_kernel, dim3(gridn(std::max(nz, nv + 1))), dim3(kBlock), 0, s, nz, nv, mask.get(), pos.get(),
                               sAi.get(), sAx.get(), lp->uAp.get(), lp->uAi.get(), lp->uAx.get());
            int nz_loaded = 0;
            IPXK_HIP(hipMemcpyAsync(&nz_loaded, pos.get() + nz, sizeof(int), hipMemcpyDeviceToHost, s));
            IPXK_HIP(hipStreamSynchronize(s));
            nz = nz_loaded;
            if (nz > 0)
                device_transpose(T, colof, nv, nc + 1, nz, lp->uAp.get(), lp->uAi.get(), lp->uAx.get(), lp->uTp.get(), lp->uTi.get(),
                                 lp->uTx.get(), s);
            else
                IPXK_HIP(hipMemsetAsync(lp->uTp.get(), 0, ((size_t)nc + 2) * sizeof(int), s));
        }
    } else {
        IPXK_HIP(hipMemsetAsync(lp->uTp.get(), 0, ((size_t)nc + 2) * sizeof(int), s));
    }

    // ---- ComputeUserModelAttributes; the flipped variables of LoadDual ----
    DevBuf<int> is_eq(atleast1(nc)), is_free((size_t)nv), is_boxed((size_t)nv), is_flipped((size_t)nv), pos(atleast1(std::max(nc, nv))), counts(4);
    lp->boxed.resize((size_t)nv); lp->flipped.resize((size_t)nv);
    hipLaunchKernelGGL(attribute_masks_kernel, dim3(gridn(std::max(nc, nv))), dim3(kBlock), 0, s, nc, nv, lp->ctype.get(), lp->lbu.get(),
                       lp->ubu.get(), is_eq.get(), is_free.get(), is_boxed.get(), is_flipped.get());
    list_of_mask(T, nc, is_eq.get(), pos.get(), counts.get() + 0, nullptr, s);
    list_of_mask(T, nv, is_free.get(), pos.get(), counts.get() + 1, nullptr, s);
    list_of_mask(T, nv, is_boxed.get(), pos.get(), counts.get() + 2, lp->boxed.get(), s);
    list_of_mask(T, nv, is_flipped.get(), pos.get(), counts.get() + 3, lp->flipped.get(), s);
    int h_counts[4];
    counts.download(h_counts, 4, s);
    const int64_t nb = h_counts[2];
    lp->num_boxed = nb;

    // ---- LoadPrimal / LoadDual ----
    bool dualize = dualize_prm < 0 ? nc > 2 * nv : dualize_prm != 0;      // :32-34
    lp->dualized = dualize;
    const int64_t m = dualize ? nv : nc, n = dualize ? nc + nb : nv, nnz = dualize ? nz + nb : nz;
    lp->num_flipped = dualize ? h_counts[3] : 0;     // (the primal form flips nothing: flipped_vars_ stays empty)
    c->m = m; c->n = n; c->nnz = nnz;
    c->pl_Ap.resize((size_t)n + 1); c->pl_Ai.resize(atleast1(nnz)); c->pl_Ax.resize(atleast1(nnz));
    lp->b.resize(atleast1(m)); lp->c.resize((size_t)(n + m)); lp->lb.resize((size_t)(n + m)); lp->ub.resize((size_t)(n + m));
    lp->colscale.resize(atleast1(n)); lp->rowscale.resize(atleast1(m));
    if (!dualize) {
        IPXK_HIP(hipMemcpyAsync(c->pl_Ap.get(), lp->uAp.get(), ((size_t)nv + 1) * sizeof(int), hipMemcpyDeviceToDevice, s));
        if (nz > 0) {
            IPXK_HIP(hipMemcpyAsync(c->pl_Ai.get(), lp->uAi.get(), (size_t)nz * sizeof(int), hipMemcpyDeviceToDevice, s));
            IPXK_HIP(hipMemcpyAsync(c->pl_Ax.get(), lp->uAx.get(), (size_t)nz * sizeof(double), hipMemcpyDeviceToDevice, s));
        }
        if (nc > 0) IPXK_HIP(hipMemcpyAsync(lp->b.get(), lp->rhs.get(), (size_t)nc * sizeof(double), hipMemcpyDeviceToDevice, s));
        hipLaunchKernelGGL(load_primal_kernel, dim3(gridn(nv + nc)), dim3(kBlock), 0, s, nc, nv, lp->ctype.get(), lp->obj.get(), lp->lbu.get(),
                           lp->ubu.get(), lp->c.get(), lp->lb.get(), lp->ub.get());
    } else {
        hipLaunchKernelGGL(load_dual_matrix_kernel, dim3(gridn(std::max(nz, nc + nb + 1))), dim3(kBlock), 0, s, nc, nb, nz, lp->uTp.get(),
                           lp->uTi.get(), lp->uTx.get(), is_flipped.get(), lp->boxed.get(), c->pl_Ap.get(), c->pl_Ai.get(), c->pl_Ax.get());
        hipLaunchKernelGGL(load_dual_vectors_kernel, dim3(gridn(n + nv)), dim3(kBlock), 0, s, nc, nb, nv, lp->ctype.get(), lp->rhs.get(),
                           lp->obj.get(), lp->lbu.get(), lp->ubu.get(), is_flipped.get(), lp->boxed.get(), lp->b.get(), lp->c.get(),
                           lp->lb.get(), lp->ub.get());
    }

    // ---- ScaleModel ----
    ipxint rounds = -1;
    if (scale_prm >= 1) {
        equilibrate_resident<int>(m, n, nnz, c->pl_Ap.get(), c->pl_Ai.get(), c->pl_Ax.get(), lp->colscale.get(), lp->rowscale.get(), &rounds, s);
    } else {
        hipLaunchKernelGGL(fill_kernel<double>, dim3(grid_for(n)), dim3(kBlock), 0, s, n, 1.0, lp->colscale.get());
        hipLaunchKernelGGL(fill_kernel<double>, dim3(grid_for(m)), dim3(kBlock), 0, s, m, 1.0, lp->rowscale.get());
    }
    if (rounds >= 0)           // (the reference's scaling vectors are empty otherwise)
        hipLaunchKernelGGL(scale_vectors_kernel, dim3(gridn(n + m)), dim3(kBlock), 0, s, m, n, lp->colscale.get(), lp->rowscale.get(),
                           lp->b.get(), lp->c.get(), lp->lb.get(), lp->ub.get());
    IPXK_HIP(hipStreamSynchronize(s));               // the masks go out of scope at the end of this function at the latest
    IPXK_HIP(hipGetLastError());

    // ---- the context from the resident matrix ----
    adopt_plain_model(c);
    build_model_resident(c, nullptr, nullptr, nullptr);

    if (info) {
        info->m = m; info->n = n; info->nnz = nnz;
        info->dualized = dualize ? 1 : 0;
        info->num_boxed = nb;
        info->num_flipped = lp->num_flipped;
        info->num_free_var = h_counts[1];
        info->num_eqconstr = h_counts[0];
        info->scale_rounds = rounds;
        info->num_dense_cols = c->num_dense;
        info->seconds = now_s() - t_start;
    }
    return lp.release();
}

void lp_destroy(Lp* lp) { delete lp; }
Context* lp_context(Lp* lp) { return lp->ctx; }
void lp_dims(const Lp* lp, int64_t* num_constr, int64_t* num_var) { *num_constr = lp->num_constr; *num_var = lp->num_var; }

void lp_get_model(Lp* lp, ipxint* Ap, ipxint* Ai, double* Ax, double* b, double* cc, double* lb, double* ub, double* colscale, double* rowscale) {
    Context* c = lp->ctx;
    hipStream_t s = c->stream;
    const int64_t m = c->m, n = c->n, nnz = c->nnz;
    if (Ap || Ai) {
        DevBuf<ipxint> wide((size_t)std::max(n + 1, nnz));
        if (Ap) {
            widen_ints(n + 1, c->pl_Ap.get(), wide.get(), s);
            wide.download(Ap, (size_t)n + 1, s);
        }
        if (Ai && nnz > 0) {
            widen_ints(nnz, c->pl_Ai.get(), wide.get(), s);
            wide.download(Ai, (size_t)nnz, s);
        }
    }
    if (Ax) c->pl_Ax.download(Ax, (size_t)nnz, s);
    if (b) lp->b.download(b, (size_t)m, s);
    if (cc) lp->c.download(cc, (size_t)(n + m), s);
    if (lb) lp->lb.download(lb, (size_t)(n + m), s);
    if (ub) lp->ub.download(ub, (size_t)(n + m), s);
    if (colscale) lp->colscale.download(colscale, (size_t)n, s);
    if (rowscale) lp->rowscale.download(rowscale, (size_t)m, s);
    IPXK_HIP(hipStreamSynchronize(s));
    IPXK_HIP(hipGetLastError());
}

void lp_solve(Lp* lp, const ipxk_solve_params* prm, ipxk_solve_info* info, ipxk_interrupt_fn interrupt, void* user) {
    Context* c = lp->ctx;
    IPXK_REQUIRE(!comm_active(c), kDeviceLuRefusal);
    lp->evaluated = false;
    lp->solved = lp->has_vertex = false;           // ClearSolution (src/lp_solver.cc:54)
    lp->basis.clear();
    std::vector<ipxint> basis((size_t)c->m, -1);   // (stays -1 when the solve ends before it has a basis)
    ipm_solve_dev(c, lp->b.get(), lp->c.get(), lp->lb.get(), lp->ub.get(), prm, info, basis.data(), nullptr, interrupt, user);
    IPXK_HIP(hipStreamSynchronize(c->stream));
    lp->solved = true;
    lp->status_ipm = info->status_ipm;
    if (!basis.empty() && basis[0] >= 0) lp->basis = std::move(basis);
}

void lp_postsolve_dev(Lp* lp, const double* out[7]) {
    Context* c = lp->ctx;
    IPXK_REQUIRE(c->it_set, "no iterate on the device (ipxk_lp_solve, ipxk_iterate_set)");
    hipStream_t s = c->stream;
    const int64_t nc = lp->num_constr, nv = lp->num_var, nb = lp->num_boxed, nf = lp->num_flipped;
    DevBuf<double>* var[5] = {&lp->px, &lp->pxl, &lp->pxu, &lp->pzl, &lp->pzu};
    for (DevBuf<double>* v : var) v->ensure((size_t)nv);
    lp->pslack.ensure(atleast1(nc)); lp->py.ensure(atleast1(nc));
    const Point pt{c->it_x.get(), c->it_xl.get(), c->it_xu.get(), c->it_y.get(), c->it_zl.get(), c->it_zu.get()};
    const UserPoint u{lp->px.get(), lp->pxl.get(), lp->pxu.get(), lp->pslack.get(), lp->py.get(), lp->pzl.get(), lp->pzu.get()};
    const int grid = gridn(std::max(nc, nv));
    if (!lp->dualized) {
        hipLaunchKernelGGL(postsolve_primal_kernel, dim3(grid), dim3(kBlock), 0, s, nc, nv, pt, lp->ctype.get(), lp->colscale.get(),
                           lp->rowscale.get(), u);
    } else {
        hipLaunchKernelGGL(postsolve_dual_kernel, dim3(grid), dim3(kBlock), 0, s, nc, nb, nv, pt, lp->ctype.get(), lp->lb.get(), lp->ub.get(),
                           lp->colscale.get(), lp->rowscale.get(), u);
        if (nb > 0) hipLaunchKernelGGL(postsolve_boxed_kernel, dim3(gridn(nb)), dim3(kBlock), 0, s, nc, nb, pt, lp->boxed.get(), lp->colscale.get(), u);
        if (nf > 0) hipLaunchKernelGGL(postsolve_flipped_kernel, dim3(gridn(nf)), dim3(kBlock), 0, s, nf, lp->flipped.get(), u);
    }
    IPXK_HIP(hipGetLastError());
    out[0] = u.x; out[1] = u.xl; out[2] = u.xu; out[3] = u.slack; out[4] = u.y; out[5] = u.zl; out[6] = u.zu;
}

void lp_evaluate(Lp* lp, ipxk_lp_eval* out) {
    Context* c = lp->ctx;
    hipStream_t s = c->stream;
    const int64_t nc = lp->num_constr, nv = lp->num_var;
    const double* p[7];
    lp_postsolve_dev(lp, p);
    const UserPoint u{lp->px.get(), lp->pxl.get(), lp->pxu.get(), lp->pslack.get(), lp->py.get(), lp->pzl.get(), lp->pzu.get()};
    lp->rb.ensure(atleast1(nc)); lp->rc.ensure((size_t)nv);
    lp->part.ensure((size_t)kNumEvalSlots * kEvalGrid); lp->result.ensure(kNumEvalSlots);
    const int grid_rows = grid_for(nc, kEvalGrid), grid_cols = grid_for(nv, kEvalGrid);
    hipLaunchKernelGGL(evaluate_rows_kernel, dim3(grid_rows), dim3(kBlock), 0, s, nc, lp->uTp.get(), lp->uTi.get(), lp->uTx.get(), lp->rhs.get(),
                       u.x, u.slack, u.y, lp->rb.get(), lp->part.get());
    hipLaunchKernelGGL(evaluate_columns_kernel, dim3(grid_cols), dim3(kBlock), 0, s, nv, lp->uAp.get(), lp->uAi.get(), lp->uAx.get(),
                       lp->obj.get(), lp->lbu.get(), lp->ubu.get(), u, lp->rc.get(), lp->part.get());
    hipLaunchKernelGGL(evaluate_finish_kernel, dim3(1), dim3(kBlock), 0, s, grid_rows, grid_cols, lp->part.get(), lp->result.get());
    double r[kNumEvalSlots];
    lp->result.download(r, kNumEvalSlots, s);
    IPXK_HIP(hipGetLastError());
    out->norm_obj = r[kVarMaxObj];
    out->norm_rhs = r[kRowMaxRhs];
    out->norm_bounds = r[kVarMaxBounds];
    out->abs_presidual = std::max(r[kRowMaxRb], r[kVarMaxBound]);
    if (r[kRowMaxRb] != r[kRowMaxRb] || r[kVarMaxBound] != r[kVarMaxBound]) out->abs_presidual = NAN;
    out->abs_dresidual = r[kVarMaxRc];
    out->rel_presidual = out->abs_presidual / (1.0 + std::max(out->norm_rhs, out->norm_bounds));
    out->rel_dresidual = out->abs_dresidual / (1.0 + out->norm_obj);
    out->pobjval = r[kVarObjX];
    out->dobjval = r[kRowRhsY] + r[kVarBoundZ];
    out->rel_objgap = (out->pobjval - out->dobjval) / (1.0 + 0.5 * std::fabs(out->pobjval + out->dobjval));
    out->complementarity = r[kVarComp] - r[kRowYSlack];
    out->normx = r[kVarMaxX];
    out->normy = r[kRowMaxY];
    out->normz = r[kVarMaxZ];
    lp->evaluated = true;
}

void lp_get_residuals(Lp* lp, double* rb, double* rc) {
    IPXK_REQUIRE(lp->evaluated, "no evaluation yet (ipxk_lp_evaluate)");
    hipStream_t s = lp->ctx->stream;
    if (rb) lp->rb.download(rb, (size_t)lp->num_constr, s);
    if (rc) lp->rc.download(rc, (size_t)lp->num_var, s);
    IPXK_HIP(hipStreamSynchronize(s));
}

namespace {

// the map on device statuses (lp->st_solver) into u, whose cbasis and vbasis are device arrays; refuses before it writes
void postsolve_basic_dev(Lp* lp, const double* x, const double* y, const double* z, const BasicPoint& u) {
    Context* c = lp->ctx;
    hipStream_t s = c->stream;
    const int64_t nc = lp->num_constr, nv = lp->num_var, nb = lp->dualized ? lp->num_boxed : 0, nf = lp->num_flipped, m = c->m, n = c->n;
    const SolverPoint pt{x, y, z, lp->st_solver.get()};
    lp->st_part.ensure((size_t)2 * kFlagGrid); lp->st_first.ensure(2);
    hipLaunchKernelGGL(fill_kernel<long long>, dim3(gridn(2 * kFlagGrid)), dim3(kBlock), 0, s, (int64_t)2 * kFlagGrid, kNoIndex, lp->st_part.get());
    hipLaunchKernelGGL(check_statuses_kernel, dim3(grid_for(std::max(m, nb), kFlagGrid)), dim3(kBlock), 0, s, n, m, nc, nb, pt.st,
                       lp->boxed.get(), lp->st_part.get());
    hipLaunchKernelGGL(first_index_kernel, dim3(2), dim3(kBlock), 0, s, lp->st_part.get(), lp->st_first.get());
    long long first[2];
    lp->st_first.download(first, 2, s);
    IPXK_HIP(hipGetLastError());
    char buf[256];
    if (first[0] != kNoIndex) {
        snprintf(buf, sizeof buf, "basic_statuses: a slack variable cannot be superbasic, first at slack %lld", first[0]);
        throw Error(IPXK_E_ARGUMENT, buf);
    }
    if (first[1] != kNoIndex) {
        snprintf(buf, sizeof buf, "basic_statuses: the added column of a boxed variable is basic and so is the variable's slack, "
                 "first at boxed variable number %lld", first[1]);
        throw Error(IPXK_E_ARGUMENT, buf);
    }
    const int grid = gridn(std::max(nc, nv));
    if (!lp->dualized) {
        hipLaunchKernelGGL(postsolve_basic_primal_kernel, dim3(grid), dim3(kBlock), 0, s, nc, nv, pt, lp->colscale.get(), lp->rowscale.get(),
                           lp->lbu.get(), lp->ubu.get(), u);
    } else {
        hipLaunchKernelGGL(postsolve_basic_dual_kernel, dim3(grid), dim3(kBlock), 0, s, nc, nb, nv, pt, lp->lb.get(), lp->ub.get(),
                           lp->colscale.get(), lp->rowscale.get(), u);
        if (nb > 0) hipLaunchKernelGGL(postsolve_basic_boxed_kernel, dim3(gridn(nb)), dim3(kBlock), 0, s, nc, nb, pt, lp->boxed.get(), lp->colscale.get(), u);
        if (nf > 0) hipLaunchKernelGGL(postsolve_basic_flipped_kernel, dim3(gridn(nf)), dim3(kBlock), 0, s, nf, lp->flipped.get(), u);
        hipLaunchKernelGGL(correct_basic_kernel, dim3(gridn(nv)), dim3(kBlock), 0, s, nv, lp->lbu.get(), lp->ubu.get(), u);
    }
    IPXK_HIP(hipGetLastError());
}

void ensure_status_buffers(Lp* lp) {
    lp->st_solver.ensure((size_t)(lp->ctx->n + lp->ctx->m));
    lp->st_cbasis.ensure(atleast1(lp->num_constr));
    lp->st_vbasis.ensure((size_t)lp->num_var);
}

// EvaluateBasicPoint of a user-form point on the device
void evaluate_basic_dev(Lp* lp, const BasicPoint& u, ipxk_lp_basic_eval* out) {
    hipStream_t s = lp->ctx->stream;
    const int64_t nc = lp->num_constr, nv = lp->num_var;
    lp->part.ensure((size_t)kNumEvalSlots * kEvalGrid); lp->result.ensure(kNumEvalSlots);
    const int grid = grid_for(std::max(nc, nv), kEvalGrid);
    hipLaunchKernelGGL(evaluate_basic_kernel, dim3(grid), dim3(kBlock), 0, s, nc, nv, lp->lbu.get(), lp->ubu.get(), lp->obj.get(), lp->ctype.get(),
                       u.x, u.slack, u.y, u.z, u.vbasis, lp->part.get());
    hipLaunchKernelGGL(evaluate_basic_finish_kernel, dim3(1), dim3(kBlock), 0, s, grid, lp->part.get(), lp->result.get());
    double r[kNumBasicSlots];
    lp->result.download(r, kNumBasicSlots, s);
    IPXK_HIP(hipGetLastError());
    out->primal_infeas = r[kBasicPrimal];
    out->dual_infeas = r[kBasicDual];
    out->objval = r[kBasicObjX];
}

}  // namespace

void lp_postsolve_basic(Lp* lp, const double* x_solver, const double* y_solver, const double* z_solver, const ipxint* statuses,
                        const LpBasicPoint& out) {
    hipStream_t s = lp->ctx->stream;
    ensure_status_buffers(lp);
    lp->st_solver.upload(statuses, (size_t)(lp->ctx->n + lp->ctx->m), s);
    postsolve_basic_dev(lp, x_solver, y_solver, z_solver, BasicPoint{out.x, out.slack, out.y, out.z, lp->st_cbasis.get(), lp->st_vbasis.get()});
    if (out.cbasis) lp->st_cbasis.download(out.cbasis, (size_t)lp->num_constr, s);
    if (out.vbasis) lp->st_vbasis.download(out.vbasis, (size_t)lp->num_var, s);
    IPXK_HIP(hipStreamSynchronize(s));
    IPXK_HIP(hipGetLastError());
}

// LpSolver::RunCrossover (src/lp_solver.cc:464-537) behind the gate of LpSolver::Solve (:64-67)
void lp_crossover(Lp* lp, const ipxk_crossover_params* prm, ipxk_crossover_info* info, ipxk_lp_basic_eval* eval, ipxk_interrupt_fn interrupt,
                  void* user) {
    Context* c = lp->ctx;
    IPXK_REQUIRE(!comm_active(c), kDeviceLuRefusal);
    IPXK_REQUIRE(lp->num_constr > 0, "ipxk_lp_crossover: the lp has no constraints, so there is no basis to push on");
    IPXK_REQUIRE(lp->solved, "ipxk_lp_crossover: no solve on this lp yet (ipxk_lp_solve)");
    hipStream_t s = c->stream;
    *info = ipxk_crossover_info{};
    ipxk_lp_basic_eval ev{};
    if (eval) *eval = ev;
    lp->has_vertex = false;
    if (lp->status_ipm != 1 && lp->status_ipm != 2) return;             // (:64-66: optimal or imprecise)
    IPXK_REQUIRE(!lp->basis.empty(), "ipxk_lp_crossover: the solve left no basis");
    ipxk_crossover_params p = prm ? *prm : ipxk_crossover_params{1e-7, 1e-7, 100};
    const double user_primal_tol = p.primal_feastol, user_dual_tol = p.dual_feastol;
    if (lp->dualized) std::swap(p.primal_feastol, p.dual_feastol);      // src/crossover.cc:83-84, :237-238
    const size_t m = (size_t)c->m, N = (size_t)(c->n + c->m);
    DevBuf<double> sx(N), sy(m), sz(N);                                 // the solver-form vertex
    std::vector<ipxint> statuses(N);
    crossover_run_dev(c, lp->b.get(), lp->c.get(), lp->lb.get(), lp->ub.get(), nullptr, lp->basis.data(), &p, info, sx.get(), sy.get(), sz.get(),
                      statuses.data(), nullptr, 0, interrupt, user);
    // the run reports 2 when the SOLVER-form vertex misses the tolerances; the reference decides on the user-form one (:534-536)
    if (info->status_crossover != 1 && info->status_crossover != 2) { IPXK_HIP(hipStreamSynchronize(s)); return; }
    ensure_status_buffers(lp);
    lp->st_solver.upload(statuses.data(), N, s);
    lp->vx.ensure((size_t)lp->num_var); lp->vz.ensure((size_t)lp->num_var);
    lp->vslack.ensure((size_t)lp->num_constr); lp->vy.ensure((size_t)lp->num_constr);
    const BasicPoint u{lp->vx.get(), lp->vslack.get(), lp->vy.get(), lp->vz.get(), lp->st_cbasis.get(), lp->st_vbasis.get()};
    postsolve_basic_dev(lp, sx.get(), sy.get(), sz.get(), u);
    lp->cbasis.resize((size_t)lp->num_constr); lp->vbasis.resize((size_t)lp->num_var);
    lp->st_cbasis.download(lp->cbasis.data(), lp->cbasis.size(), s);
    lp->st_vbasis.download(lp->vbasis.data(), lp->vbasis.size(), s);
    evaluate_basic_dev(lp, u, &ev);
    IPXK_HIP(hipStreamSynchronize(s));               // (sx, sy, sz go out of scope)
    lp->has_vertex = true;
    info->status_crossover = ev.primal_infeas > user_primal_tol || ev.dual_infeas > user_dual_tol ? 2 : 1;
    if (eval) *eval = ev;
}

void lp_evaluate_basic(Lp* lp, const double* x, const double* slack, const double* y, const double* z, const ipxint* vbasis,
                       ipxk_lp_basic_eval* out) {
    ensure_status_buffers(lp);
    lp->st_vbasis.upload(vbasis, (size_t)lp->num_var, lp->ctx->stream);
    // (the kernel only reads: the point is passed as the writable record the postsolve fills)
    evaluate_basic_dev(lp, BasicPoint{const_cast<double*>(x), const_cast<double*>(slack), const_cast<double*>(y), const_cast<double*>(z), nullptr,
                                      lp->st_vbasis.get()}, out);
}

void lp_basic_solution(Lp* lp, const double* out[4], const ipxint** cbasis, const ipxint** vbasis) {
    IPXK_REQUIRE(lp->has_vertex, "no basic solution (ipxk_lp_crossover with status_crossover 1 or 2)");
    out[0] = lp->vx.get(); out[1] = lp->vslack.get(); out[2] = lp->vy.get(); out[3] = lp->vz.get();
    *cbasis = lp->cbasis.data();
    *vbasis = lp->vbasis.data();
}

// LpSolver::GetBasis (src/lp_solver.cc:233-244)
void lp_get_basis(Lp* lp, ipxint* cbasis, ipxint* vbasis) {
    Context* c = lp->ctx;
    IPXK_REQUIRE(!lp->basis.empty(), "no basis (ipxk_lp_solve has not built one)");
    if (lp->has_vertex) {
        if (cbasis) std::copy(lp->cbasis.begin(), lp->cbasis.end(), cbasis);
        if (vbasis) std::copy(lp->vbasis.begin(), lp->vbasis.end(), vbasis);
        return;
    }
    hipStream_t s = c->stream;
    const int64_t m = c->m, N = c->n + c->m;
    for (ipxint j : lp->basis) IPXK_REQUIRE(j >= 0 && j < N, "the stored basis holds an index out of range");
    ensure_status_buffers(lp);
    DevBuf<ipxint> basis_dev;
    basis_dev.upload(lp->basis, s);
    hipLaunchKernelGGL(nonbasic_statuses_kernel, dim3(gridn(N)), dim3(kBlock), 0, s, N, lp->lb.get(), lp->ub.get(), lp->st_solver.get());
    hipLaunchKernelGGL(basic_statuses_kernel, dim3(gridn(m)), dim3(kBlock), 0, s, m, basis_dev.get(), lp->st_solver.get());
    postsolve_basic_dev(lp, nullptr, nullptr, nullptr, BasicPoint{nullptr, nullptr, nullptr, nullptr, lp->st_cbasis.get(), lp->st_vbasis.get()});
    if (cbasis) lp->st_cbasis.download(cbasis, (size_t)lp->num_constr, s);
    if (vbasis) lp->st_vbasis.download(vbasis, (size_t)lp->num_var, s);
    IPXK_HIP(hipStreamSynchronize(s));               // (basis_dev goes out of scope)
    IPXK_HIP(hipGetLastError());
}

}  // namespace ipxk
