// StartingBasis on the device (seventh piece): reference src/starting_basis.cc:128-185 for
// crash_basis = 0 -- the weights from the resident iterate, Basis::ConstructBasisFromWeights from the slack basis
// (src/basis.cc:353-385: PivotFreeVariablesIntoBasis :676-781, PivotFixedVariablesOutOfBasis :783-930), the status changes
// with make_fixed (:153-173) and PostprocessDependencies (:52-126).
//
// The basis itself is DeviceBasis (basis.hip), shared with Maxvolume: FTRAN and BTRAN on the resident factors plus the eta file,
// Basis::Factorize and Basis::ExchangeIfStable (src/basis.cc:286-321).  What is here:
//   * sb_column_kernel: the maxima of the tableau column over all positions and over those whose basic variable is not free,
//     the objective change of the primal ray and the column's number of nonzeros, in one pass over m;
//   * sb_row_kernel: the tableau row AI' btran over all n + m columns with the maxima of its two classes fused in -- one
//     gather pass over the plain CSC, eight lanes per column, the row written once; the only kernel here whose time is
//     proportional to nnz(A);
//   * sb_row_scaled_kernel: the second pass over the stored row, arg max r * weight among the entries r >= 0.1 rmax_nonfixed;
//   * the decisions themselves are taken by the one-workgroup kernels that finish these reductions, so that everything a
//     candidate needs (column, row, both pivots, both ray tests) is enqueued without a host round trip and ONE block of
//     scalars per candidate reaches the host, which keeps the stacks, the eta file and the refactorizations.
// Every reduction is a fixed-order tree over block partials, ties go to the lowest index (the reference's loops take the first
// strictly larger entry): two calls from the same iterate give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "context.hpp"
#include "trisolve.hpp"

namespace ipxk {

namespace {

constexpr int kSbGrid = 512;            // workgroups of the two-stage reductions = threads of the kernels that finish them
constexpr int kRowLanes = 8;            // lanes per column in sb_row_kernel
constexpr int kRowCols = kBlock / kRowLanes;

enum SbDecision { kSbStability = 1, kSbDependent = 2, kSbExchange = 3 };

// the scalars of one candidate, written by the device, read by the host
struct SbScalars {
    MvScalars mv;             // jn, pmax, jb, pivot_col, pivot_row, eta_nnz: what the kernels shared with Maxvolume read and write
    int decision;             // SbDecision
    int imax, imax_class;     // pmax / jmax; pmax_nonfree / jmax_nonfixed (-1: none)
    int jscaled;              // jmax_scaled
    double vmax, vmax_class;  // fmax / rmax; fmax_nonfree / rmax_nonfixed
    double threshold;         // 0.1 rmax_nonfixed
    double delta_obj;         // objective change along the primal / dual ray
};

using SbPart = Partial<2>;       // two indexed bests, a sum, a count (device_utils.hpp)


// ---- weights and the model vectors of the ray tests ---------------------------------------------------------------------
// starting_basis.cc:138-146: the scaling factor, inf exactly for lb = -inf, ub = +inf, and 0 where lb == ub
__global__ void sb_weights_kernel(int64_t N, const double* __restrict__ d, const double* __restrict__ lb, const double* __restrict__ ub,
                                  double* __restrict__ w, int* bad) {
    IPXK_GRID_STRIDE(j, N) {
        const bool free_bounds = isinf(lb[j]) && isinf(ub[j]);
        const double dj = d[j];
        if (free_bounds ? !(isinf(dj) && dj > 0.0) : !isfinite(dj)) atomicMin(bad, (int)j);
        w[j] = lb[j] == ub[j] ? 0.0 : dj;
    }
}
// basis.cc:795-801: b minus the columns of the variables with lb == ub != 0, row by row over the row-wise copy of A
__global__ void sb_b_minus_fixed_kernel(int m, int n, const int* __restrict__ Tp, const int* __restrict__ Ti, const double* __restrict__ Tx,
                                        const double* __restrict__ b, const double* __restrict__ lb, const double* __restrict__ ub,
                                        double* __restrict__ out) {
    IPXK_GRID_STRIDE(i, m) {
        double v = b[i];
        for (int q = Tp[i]; q < Tp[i + 1]; q++) {
            const int j = Ti[q];
            if (lb[j] == ub[j] && lb[j] != 0.0) v += -lb[j] * Tx[q];
        }
        if (lb[n + i] == ub[n + i] && lb[n + i] != 0.0) v += -lb[n + i];
        out[i] = v;
    }
}
__global__ void sb_slack_basis_kernel(int m, int n, ipxint* __restrict__ basis, int* __restrict__ posof) {
    IPXK_GRID_STRIDE(j, (int64_t)n + m) posof[j] = j >= n ? (int)(j - n) : -1;
    IPXK_GRID_STRIDE(i, m) basis[i] = n + i;
}
__global__ void sb_set_kernel(int jn, int pmax, int jb, SbScalars* S) { S->mv.jn = jn; S->mv.pmax = pmax; S->mv.jb = jb; }

// ---- the tableau column: basis.cc:699-715 (+ :730-737, the primal ray) ----------------------------------------------------
// v1 / i1: largest |f_p| over all positions, v2 / i2: over the positions whose basic variable is not free,
// s: sum of c_j f_p over the free ones, c: # nonzeros of the column
__global__ __launch_bounds__(kBlock) void sb_column_kernel(int m, const double* __restrict__ lhs, const ipxint* __restrict__ basis,
                                                           const double* __restrict__ w, const double* __restrict__ cc, SbPart* part) {
    SbPart p = partial_identity<2>();
    IPXK_GRID_STRIDE(q, m) {
        const double x = lhs[q], f = fabs(x);
        const ipxint j = basis[q];
        if (f > p.v[0]) { p.v[0] = f; p.i[0] = (int)q; }
        if (isinf(w[j])) p.s += cc[j] * x;
        else if (f > p.v[1]) { p.v[1] = f; p.i[1] = (int)q; }
        p.c += x != 0.0;
    }
    p = block_partial<kBlock>(p);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}
// free_loop: the three-way decision of basis.cc:717-767 and the position it exchanges at; else (the column of the variable
// that enters for a fixed slack): the pivot from the column at the slack's position only
__global__ __launch_bounds__(kSbGrid) void sb_column_final_kernel(int nparts, const SbPart* part, int free_loop, double dependency_tol,
                                                                  const double* __restrict__ cc, const double* __restrict__ lhs,
                                                                  const ipxint* __restrict__ basis, SbScalars* S) {
    const SbPart p = block_partial<kSbGrid>(load_partial(nparts, part));
    if (threadIdx.x != 0) return;
    S->mv.eta_nnz = p.c;
    if (!free_loop) { S->mv.pivot_col = lhs[S->mv.pmax]; return; }
    const int pmax = p.i[0] == INT_MAX ? -1 : p.i[0], pmax_nonfree = p.i[1] == INT_MAX ? -1 : p.i[1];
    S->vmax = p.v[0]; S->imax = pmax;
    S->vmax_class = p.v[1]; S->imax_class = pmax_nonfree;
    S->delta_obj = cc[S->mv.jn] - p.s;
    int decision, pos;
    if (p.v[0] > 4.0 && p.v[1] < 1.0) { decision = kSbStability; pos = pmax; }
    else if (p.v[1] <= dependency_tol) { decision = kSbDependent; pos = -1; }
    else { decision = kSbExchange; pos = pmax_nonfree; }
    S->decision = decision;
    S->mv.pmax = pos;                                   // (-1: the unit vector of the row pivot is zero, its result unused)
    S->mv.jb = pos >= 0 ? (int)basis[pos] : -1;
    S->mv.pivot_col = pos >= 0 ? lhs[pos] : 0.0;
}

// ---- the tableau row: Basis::TableauRow (basis.cc:219-284, dense branch) + basis.cc:832-851 ----------------------------------
// row[j] = a_j' btran for the nonbasic columns (slack columns: btran[j - n]), 0 for the basic ones.  Eight lanes share a column:
// lane l adds the products of the column's entries l, l + 8, ... in order, then a fixed tree over the eight.  The matrix is
// streamed once (12 bytes per entry, consecutive lanes on consecutive entries), btran is the only gathered vector (m doubles).
// v1 / i1: largest |r_j| over slack columns and structural columns of nonzero weight, v2 / i2: over columns of nonzero weight
__global__ __launch_bounds__(kBlock) void sb_row_kernel(int n, int64_t N, const int* __restrict__ Ap, const int* __restrict__ Ai,
                                                        const double* __restrict__ Ax, const double* __restrict__ btran,
                                                        const int* __restrict__ posof, const double* __restrict__ w,
                                                        double* __restrict__ row, SbPart* part) {
    SbPart p = partial_identity<2>();
    const int lane = threadIdx.x & (kRowLanes - 1), sub = threadIdx.x / kRowLanes;
    // (the trip count is the same for every thread of the workgroup: the lane exchanges below run with all lanes active)
    for (int64_t base = (int64_t)blockIdx.x * kRowCols; base < N; base += (int64_t)gridDim.x * kRowCols) {
        const int64_t j = base + sub;
        const bool nonbasic = j < N && posof[j] < 0;
        double sum = 0.0;
        if (nonbasic && j < n)
            for (int q = Ap[j] + lane; q < Ap[j + 1]; q += kRowLanes) sum += Ax[q] * btran[Ai[q]];
        sum = wave_sum<kRowLanes>(sum);
        if (lane == 0 && j < N) {
            if (nonbasic && j >= n) sum = btran[j - n];
            row[j] = sum;
            const double r = fabs(sum), wj = w[j];
            if (j >= n || wj != 0.0) {
                if (r > p.v[0]) { p.v[0] = r; p.i[0] = (int)j; }
                if (wj != 0.0 && r > p.v[1]) { p.v[1] = r; p.i[1] = (int)j; }
            }
        }
    }
    p = block_partial<kBlock>(p);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}
// the three-way decision of basis.cc:853-889 and the threshold of the second pass
__global__ __launch_bounds__(kSbGrid) void sb_row_final_kernel(int nparts, const SbPart* part, double dependency_tol, SbScalars* S) {
    const SbPart p = block_partial<kSbGrid>(load_partial(nparts, part));
    if (threadIdx.x != 0) return;
    S->vmax = p.v[0]; S->imax = p.i[0] == INT_MAX ? -1 : p.i[0];
    S->vmax_class = p.v[1]; S->imax_class = p.i[1] == INT_MAX ? -1 : p.i[1];
    S->decision = (p.v[0] > 4.0 && p.v[1] < 1.0) ? kSbStability : p.v[1] <= dependency_tol ? kSbDependent : kSbExchange;
    S->threshold = 0.1 * p.v[1];
}
// basis.cc:893-905: among the numerically stable pivots the one that maximizes the volume
__global__ __launch_bounds__(kBlock) void sb_row_scaled_kernel(int64_t N, const double* __restrict__ row, const double* __restrict__ w,
                                                               const SbScalars* S, SbPart* part) {
    SbPart p = partial_identity<2>();
    const double threshold = S->threshold;
    IPXK_GRID_STRIDE(j, N) {
        const double r = fabs(row[j]);
        if (r >= threshold) {
            const double rscaled = r * w[j];
            if (rscaled > p.v[0]) { p.v[0] = rscaled; p.i[0] = (int)j; }
        }
    }
    p = block_partial<kBlock>(p);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}
// the dual ray (basis.cc:876-884): btran' (b - sum of the fixed columns)
__global__ __launch_bounds__(kBlock) void sb_dot_kernel(int m, const double* __restrict__ u, const double* __restrict__ v, SbPart* part) {
    SbPart p = partial_identity<2>();
    IPXK_GRID_STRIDE(i, m) p.s += u[i] * v[i];
    p = block_partial<kBlock>(p);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}
// the column that enters and the pivot from the row.  (Dependent row: the slack itself, a valid column whose result is unused.)
__global__ __launch_bounds__(kSbGrid) void sb_row_choice_kernel(int nparts_scaled, const SbPart* part_scaled, int nparts_dot,
                                                                const SbPart* part_dot, const double* __restrict__ row, SbScalars* S) {
    const SbPart ps = block_partial<kSbGrid>(load_partial(nparts_scaled, part_scaled));
    __syncthreads();                                    // (the shared partials are written again)
    const SbPart pd = block_partial<kSbGrid>(load_partial(nparts_dot, part_dot));
    if (threadIdx.x != 0) return;
    S->jscaled = ps.i[0] == INT_MAX ? -1 : ps.i[0];
    S->delta_obj = pd.s;
    int jn = S->mv.jb;
    if (S->decision == kSbStability && S->imax >= 0) jn = S->imax;
    if (S->decision == kSbExchange && S->jscaled >= 0) jn = S->jscaled;
    S->mv.jn = jn;
    S->mv.pivot_row = row[jn];
}
__global__ void sb_exchange_kernel(const SbScalars* S, ipxint* basis, int* posof) {
    const int jn = S->mv.jn, jb = S->mv.jb, p = S->mv.pmax;      // Basis::ExchangeIfStable :308-313
    basis[p] = jn;
    posof[jn] = p;
    posof[jb] = -1;
}

// ---- the iterate: starting_basis.cc:165-173 and PostprocessDependencies (:52-126) -------------------------------------------
// Iterate::make_fixed(j, lb[j]) for the nonbasic variables with lb == ub
__global__ void sb_make_fixed_kernel(int64_t N, const int* __restrict__ posof, const double* __restrict__ lb, const double* __restrict__ ub,
                                     double* __restrict__ x, double* __restrict__ xl, double* __restrict__ xu, double* __restrict__ zl,
                                     double* __restrict__ zu, unsigned char* __restrict__ state) {
    IPXK_GRID_STRIDE(j, N)
        if (lb[j] == ub[j] && posof[j] < 0) { x[j] = lb[j]; xl[j] = xu[j] = zl[j] = zu[j] = 0.0; state[j] = IPXK_STATE_FIXED; }
}
// dx[j] = -x[j] and rhs += x[j] a_j for the dependent free columns, one after the other in the order of the list (one workgroup)
__global__ __launch_bounds__(kBlock) void sb_dependent_columns_kernel(int ndep, const int* __restrict__ list, const int* __restrict__ Ap,
                                                                      const int* __restrict__ Ai, const double* __restrict__ Ax,
                                                                      const double* __restrict__ x, double* dx, double* rhs) {
    for (int k = 0; k < ndep; k++) {
        const int j = list[k];
        const double xj = x[j];
        for (int q = Ap[j] + threadIdx.x; q < Ap[j + 1]; q += kBlock) rhs[Ai[q]] += xj * Ax[q];     // (distinct rows within a column)
        if (threadIdx.x == 0) dx[j] = -xj;
        __syncthreads();
    }
}
__global__ void sb_scatter_basic_kernel(int m, const ipxint* __restrict__ basis, const double* __restrict__ dxbasic, double* __restrict__ dx) {
    IPXK_GRID_STRIDE(p, m) dx[basis[p]] = dxbasic[p];
}
// dy[p] = -y[i] at the positions of the dependent rows' slacks (list: rows i)
__global__ void sb_dependent_rows_rhs_kernel(int ndep, const int* __restrict__ list, int n, const int* __restrict__ posof,
                                             const double* __restrict__ y, double* __restrict__ dy) {
    IPXK_GRID_STRIDE(k, ndep) dy[posof[n + list[k]]] = -y[list[k]];
}
__global__ void sb_dependent_rows_exact_kernel(int ndep, const int* __restrict__ list, const double* __restrict__ y, double* __restrict__ dy) {
    IPXK_GRID_STRIDE(k, ndep) dy[list[k]] = -y[list[k]];              // "would be already in exact arithmetic"
}
// make_fixed(j, 0.0) for the dependent columns; make_implied_eq for the slacks of the dependent rows (device state FREE)
__global__ void sb_make_dependent_kernel(int ncols, const int* __restrict__ cols, int nrows, const int* __restrict__ rows, int n,
                                         double* __restrict__ x, double* __restrict__ xl, double* __restrict__ xu, double* __restrict__ zl,
                                         double* __restrict__ zu, unsigned char* __restrict__ state) {
    IPXK_GRID_STRIDE(k, ncols) {
        const int j = cols[k];
        x[j] = 0.0; xl[j] = xu[j] = zl[j] = zu[j] = 0.0; state[j] = IPXK_STATE_FIXED;
    }
    IPXK_GRID_STRIDE(k, nrows) {
        const int j = n + rows[k];
        xl[j] = xu[j] = __builtin_huge_val(); zl[j] = zu[j] = 0.0; state[j] = IPXK_STATE_FREE;
    }
}

struct PinnedScalars {
    SbScalars* h = nullptr;
    PinnedScalars() { IPXK_HIP(hipHostMalloc(reinterpret_cast<void**>(&h), sizeof(SbScalars))); }
    ~PinnedScalars() { if (h) (void)hipHostFree(h); }
};

}  // namespace

void ipm_starting_basis_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub,
                            const ipxk_starting_basis_params* prm, ipxk_starting_basis_info* info, ipxint* basis_out,
                            ipxint* status_out, ipxint* log, ipxint log_cap, ipxk_interrupt_fn interrupt, void* user) {
    IPXK_REQUIRE(!comm_active(c), kDeviceLuRefusal);
    IPXK_REQUIRE(c->it_set, "no iterate on the device (ipxk_iterate_set)");
    IPXK_REQUIRE(c->have_plain, "no resident copy of the matrix");
    const int m = (int)c->m, n = (int)c->n;
    const int64_t N = (int64_t)n + m;
    IPXK_REQUIRE(m > 0, "empty model");
    hipStream_t s = c->stream;
    const double t_start = now_s();
    const double dependency_tol = std::max(0.0, prm ? prm->dependency_tol : 1e-6);
    const ipxint max_etas = prm ? prm->max_etas : 0;
    ipxk_starting_basis_info I{};
    c->sb.clear();
    c->drv.clear();
    maxvol_drop_etas(c);                       // an eta file of an earlier Maxvolume: history, the slack basis is factorized below
    if (!c->maxvol) c->maxvol = new MaxvolState;
    MaxvolState& M = *c->maxvol;
    M.part.ensure(kSbGrid); M.scalars.ensure(1);

    DevBuf<double> w((size_t)N), row((size_t)N), dx((size_t)N);
    DevBuf<double> bfix((size_t)m), dy((size_t)m);
    DevBuf<int> posof((size_t)N), flag(1);
    DevBuf<ipxint> basis((size_t)m);
    DevBuf<SbPart> part(kSbGrid), part_dot(kSbGrid);
    DevBuf<SbScalars> scalars(1);
    PinnedScalars pinned;
    SbScalars* S = scalars.get();
    IPXK_HIP(hipMemsetAsync(S, 0, sizeof(SbScalars), s));
    const int gm = grid_for(m, kSbGrid), gN = grid_for(N, kSbGrid);
    const int grow = (int)std::min<int64_t>(kSbGrid, (N + kRowCols - 1) / kRowCols);

    // ---- 1. weights (starting_basis.cc:138-146)
    const int kNoBad = INT_MAX;
    flag.upload(&kNoBad, 1, s);
    {
        DevBuf<int> nonbarrier(1);
        IPXK_HIP(hipMemsetAsync(nonbarrier.get(), 0, sizeof(int), s));
        iterate_scaling_factors_dev(c, dx.get(), nonbarrier.get());
        hipLaunchKernelGGL(sb_weights_kernel, dim3(gN), dim3(kBlock), 0, s, N, dx.get(), lb, ub, w.get(), flag.get());
        IPXK_HIP(hipStreamSynchronize(s));     // (nonbarrier goes out of scope)
    }
    int bad = kNoBad;
    flag.download(&bad, 1, s);
    std::vector<double> w_h((size_t)N);
    w.download(w_h.data(), (size_t)N, s);
    IPXK_HIP(hipStreamSynchronize(s));
    IPXK_REQUIRE(bad == kNoBad, "the scaling factor of variable " + std::to_string(bad) + " does not fit its bounds: inf is expected exactly for "
                                "lb = -inf, ub = +inf (the iterate's states must be those of Iterate::Initialize)");
    hipLaunchKernelGGL(sb_b_minus_fixed_kernel, dim3(gm), dim3(kBlock), 0, s, m, n, c->pl_Tp.get(), c->pl_Ti.get(), c->pl_Tx.get(), b, lb, ub,
                       bfix.get());

    // ---- 2. the slack basis (Basis::SetToSlackBasis), its factors and the operator the sweeps run on.  Inside the two loops every
    // basic variable is BASIC and every other one NONBASIC, as in the reference, and the operator's scaling is not used.
    const std::vector<double> ones((size_t)N, 1.0);
    DeviceBasis B(c, M, max_etas, false, ones.data(), &S->mv);
    std::vector<ipxint> &basis_h = B.basis_h, &status_h = B.status_h;
    std::vector<int> pos_h((size_t)N, -1);
    status_h.resize((size_t)N);
    for (int j = 0; j < n; j++) status_h[(size_t)j] = IPXK_NONBASIC;
    for (int i = 0; i < m; i++) { status_h[(size_t)n + i] = IPXK_BASIC; basis_h[(size_t)i] = n + i; pos_h[(size_t)n + i] = i; }
    hipLaunchKernelGGL(sb_slack_basis_kernel, dim3(gN), dim3(kBlock), 0, s, m, n, basis.get(), posof.get());
    (void)B.refactorize();

    auto poll_interrupt = [&]() -> ipxint {
        if (interrupt) return interrupt(user);
        return c->interrupt ? c->interrupt(c->interrupt_user) : 0;
    };
    // an accepted exchange: this driver's part between DeviceBasis::exchange_if_stable and commit.  Returns false when the candidate is to
    // be tried again (or B.errflag is set).
    auto exchange = [&](const SbScalars& a) {
        if (!B.exchange_if_stable(a.mv)) return false;
        hipLaunchKernelGGL(sb_exchange_kernel, dim3(1), dim3(1), 0, s, S, basis.get(), posof.get());
        if (log && I.updates_start < log_cap) { log[2 * I.updates_start] = a.mv.jb; log[2 * I.updates_start + 1] = a.mv.jn; }
        I.updates_start++;
        pos_h[(size_t)a.mv.jn] = a.mv.pmax;
        pos_h[(size_t)a.mv.jb] = -1;
        B.commit(a.mv);
        return true;
    };

    // ---- 3. Basis::PivotFreeVariablesIntoBasis (:676-781)
    std::vector<int> dependent_cols, dependent_rows;
    std::vector<ipxint> remaining;
    if (!B.errflag)
        for (int64_t j = 0; j < N; j++)
            if (std::isinf(w_h[(size_t)j]) && pos_h[(size_t)j] < 0) remaining.push_back(j);
    while (!remaining.empty() && !B.errflag) {
        const ipxint jn = remaining.back();
        if ((B.errflag = poll_interrupt()) != 0) break;
        hipLaunchKernelGGL(sb_set_kernel, dim3(1), dim3(1), 0, s, (int)jn, -1, -1, S);
        B.ftran();
        hipLaunchKernelGGL(sb_column_kernel, dim3(gm), dim3(kBlock), 0, s, m, B.lhs, basis.get(), w.get(), cc, part.get());
        hipLaunchKernelGGL(sb_column_final_kernel, dim3(1), dim3(kSbGrid), 0, s, gm, part.get(), 1, dependency_tol, cc, B.lhs, basis.get(), S);
        // the BTRAN of the leaving variable (ExchangeIfStable with sys = -1, :292-293): pivot from the row
        B.btran_unit();
        mv_pivot_from_row(c, B.btran, &S->mv);
        const SbScalars a = read_scalars(S, pinned.h, s);
        if (a.decision == kSbDependent) {
            // jn cannot be pivoted into the basis; the first such column that changes the objective is an unbounded primal ray
            if (!I.cols_inconsistent && std::abs(a.delta_obj) > dependency_tol) I.cols_inconsistent = 1;
            I.dependent_cols++;
            dependent_cols.push_back((int)jn);
            remaining.pop_back();
            continue;
        }
        if (!exchange(a)) continue;                             // "factorization was unstable, try again"
        remaining.pop_back();
        if (a.decision == kSbStability) { remaining.push_back(a.mv.jb); I.stability_pivots++; }
    }

    // ---- 4. Basis::PivotFixedVariablesOutOfBasis (:783-930)
    remaining.clear();
    if (!B.errflag)
        for (int64_t j = n; j < N; j++)
            if (w_h[(size_t)j] == 0.0 && pos_h[(size_t)j] >= 0) remaining.push_back(j);
    while (!remaining.empty() && !B.errflag) {
        const ipxint jb = remaining.back();
        if ((B.errflag = poll_interrupt()) != 0) break;
        hipLaunchKernelGGL(sb_set_kernel, dim3(1), dim3(1), 0, s, (int)jb, pos_h[(size_t)jb], (int)jb, S);
        B.btran_unit();
        hipLaunchKernelGGL(sb_row_kernel, dim3(grow), dim3(kBlock), 0, s, n, N, c->pl_Ap.get(), c->pl_Ai.get(), c->pl_Ax.get(), B.btran,
                           posof.get(), w.get(), row.get(), part.get());
        hipLaunchKernelGGL(sb_row_final_kernel, dim3(1), dim3(kSbGrid), 0, s, grow, part.get(), dependency_tol, S);
        hipLaunchKernelGGL(sb_row_scaled_kernel, dim3(gN), dim3(kBlock), 0, s, N, row.get(), w.get(), S, part.get());
        hipLaunchKernelGGL(sb_dot_kernel, dim3(gm), dim3(kBlock), 0, s, m, B.btran, bfix.get(), part_dot.get());
        hipLaunchKernelGGL(sb_row_choice_kernel, dim3(1), dim3(kSbGrid), 0, s, gN, part.get(), gm, part_dot.get(), row.get(), S);
        // the FTRAN of the entering variable (ExchangeIfStable with sys = +1, :290-291): pivot from the column, and the eta
        B.ftran();
        hipLaunchKernelGGL(sb_column_kernel, dim3(gm), dim3(kBlock), 0, s, m, B.lhs, basis.get(), w.get(), cc, part.get());
        hipLaunchKernelGGL(sb_column_final_kernel, dim3(1), dim3(kSbGrid), 0, s, gm, part.get(), 0, dependency_tol, cc, B.lhs, basis.get(), S);
        const SbScalars a = read_scalars(S, pinned.h, s);
        if (a.decision == kSbDependent) {
            // jb cannot be pivoted out of the basis; the first such row that changes the dual objective is an unbounded dual ray
            if (!I.rows_inconsistent && std::abs(a.delta_obj) > dependency_tol) I.rows_inconsistent = 1;
            I.dependent_rows++;
            dependent_rows.push_back((int)(jb - n));
            remaining.pop_back();
            continue;
        }
        if (!exchange(a)) continue;
        remaining.pop_back();
        if (a.decision == kSbStability) { remaining.push_back(a.mv.jn); I.stability_pivots++; }
    }
    IPXK_HIP(hipStreamSynchronize(s));
    check_sweep_abort(c);
    // fresh factors of the final basis: what the solves below and the main phase's Maxvolume start from
    if (!B.errflag && B.etas.K > 0) (void)B.refactorize();
    I.errflag = B.errflag;
    I.factorizations = B.factorizations;       // every attempt, as the reference's num_factorizations_
    if (I.errflag) {
        I.seconds = now_s() - t_start;
        if (info) *info = I;
        return;
    }

    // ---- 5. status changes and make_fixed (starting_basis.cc:153-173)
    for (int64_t j = 0; j < N; j++)
        if (w_h[(size_t)j] == 0.0 || std::isinf(w_h[(size_t)j])) status_h[(size_t)j] = pos_h[(size_t)j] >= 0 ? IPXK_BASIC_FREE : IPXK_NONBASIC_FIXED;
    hipLaunchKernelGGL(sb_make_fixed_kernel, dim3(gN), dim3(kBlock), 0, s, N, posof.get(), lb, ub, c->it_x.get(), c->it_xl.get(), c->it_xu.get(),
                       c->it_zl.get(), c->it_zu.get(), c->it_state.get());

    // ---- 6. PostprocessDependencies (:52-126)
    if (!dependent_cols.empty() || !dependent_rows.empty()) {
        std::sort(dependent_cols.begin(), dependent_cols.end());
        std::sort(dependent_rows.begin(), dependent_rows.end());
        DevBuf<int> cols_dev, rows_dev;
        const int nc = (int)dependent_cols.size(), nr = (int)dependent_rows.size();
        IPXK_HIP(hipMemsetAsync(dx.get(), 0, (size_t)N * sizeof(double), s));
        IPXK_HIP(hipMemsetAsync(dy.get(), 0, (size_t)m * sizeof(double), s));
        if (nc > 0) {
            cols_dev.upload(dependent_cols, s);
            IPXK_HIP(hipMemsetAsync(B.rhs, 0, (size_t)m * sizeof(double), s));
            hipLaunchKernelGGL(sb_dependent_columns_kernel, dim3(1), dim3(kBlock), 0, s, nc, cols_dev.get(), c->pl_Ap.get(), c->pl_Ai.get(),
                               c->pl_Ax.get(), c->it_x.get(), dx.get(), B.rhs);
            solve_dense_dev(c, B.rhs, B.lhs, 'N');
            hipLaunchKernelGGL(sb_scatter_basic_kernel, dim3(gm), dim3(kBlock), 0, s, m, basis.get(), B.lhs, dx.get());
        }
        if (nr > 0) {
            rows_dev.upload(dependent_rows, s);
            hipLaunchKernelGGL(sb_dependent_rows_rhs_kernel, dim3(grid_for(nr, kSbGrid)), dim3(kBlock), 0, s, nr, rows_dev.get(), n, posof.get(),
                               c->it_y.get(), dy.get());
            solve_dense_dev(c, dy.get(), dy.get(), 'T');
            hipLaunchKernelGGL(sb_dependent_rows_exact_kernel, dim3(grid_for(nr, kSbGrid)), dim3(kBlock), 0, s, nr, rows_dev.get(), c->it_y.get(), dy.get());
        }
        iterate_update_dev(c, 1.0, dx.get(), nullptr, nullptr, 1.0, dy.get(), nullptr, nullptr);
        hipLaunchKernelGGL(sb_make_dependent_kernel, dim3(grid_for(std::max(nc, nr), kSbGrid)), dim3(kBlock), 0, s, nc, cols_dev.get(), nr, rows_dev.get(), n,
                           c->it_x.get(), c->it_xl.get(), c->it_xu.get(), c->it_zl.get(), c->it_zu.get(), c->it_state.get());
        IPXK_HIP(hipStreamSynchronize(s));      // (the index lists go out of scope)
    }

    // ---- the operator of the starting basis with the statuses and scaling factors the main phase continues from
    {
        std::vector<double> colscale((size_t)N);
        IPXK_HIP(hipMemsetAsync(flag.get(), 0, sizeof(int), s));
        iterate_scaling_factors_dev(c, dx.get(), flag.get());
        dx.download(colscale.data(), (size_t)N, s);
        IPXK_HIP(hipStreamSynchronize(s));
        split_prepare_lu(c, status_h.data(), colscale.data());
    }
    IPXK_HIP(hipStreamSynchronize(s));
    IPXK_HIP(hipGetLastError());
    check_sweep_abort(c);
    c->sb.store(c, basis_h, status_h);
    I.seconds = now_s() - t_start;
    if (basis_out) std::copy(basis_h.begin(), basis_h.end(), basis_out);
    if (status_out) std::copy(status_h.begin(), status_h.end(), status_out);
    if (info) *info = I;
}

}  // namespace ipxk
