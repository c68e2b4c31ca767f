// Crossover in solver form on the device: the two push phases (reference src/crossover.cc), Basis::ComputeBasicSolution
// (src/basis.cc:324-351) and the call that strings them together (LpSolver::RunCrossover, src/lp_solver.cc:464-537, without the
// postsolve of the vertex).  The basis is DeviceBasis (basis.hip), as for Maxvolume, the starting basis and the drop procedures.
// What is here:
//   * cross_row_kernel: PushDual's tableau row.  One gather pass over the plain CSC of AI, eight lanes per column, forms
//     row[j] = a_j' btran for the nonbasic columns (0 for basic ones), STORES it -- the second pass of the ratio test and the update
//     read it again -- and folds the first pass of DualRatioTest into the same pass: the matrix is streamed once per push;
//   * the ratio tests in an order-free form.  The reference's first pass shrinks `step` entry by entry; in exact arithmetic its
//     result is the candidate ratio of least magnitude among the entries that block at the FULL step.  That is what the kernels
//     compute: a two-stage indexed arg min (least |ratio|, lowest index among equals) over the entries with |pivot| > kPivotZeroTol
//     that violate their bound by more than feastol at the full step, then the reference's second pass as a two-stage indexed arg
//     max of |pivot| (lowest index among equals; the reference's loop keeps the first strictly larger entry).  This equals the
//     reference's sequential loop wherever no two candidate ratios lie within rounding of each other, and exactly at exact ties;
//   * the one-workgroup kernels that finish the reductions take the decision: everything a candidate needs is enqueued without a
//     host round trip and ONE block of scalars per candidate reaches the host, which keeps the mirrors, the eta file, the
//     refactorizations and the stability check; only an accepted exchange launches the update;
//   * the basic solution: b - N x_N row by row from the resident row-wise copy, the two dense solves, z_N in one gather pass.
// Every reduction is a fixed-order tree over block partials and ties go to the lowest index: two calls from the same state give
// the same bits.  No kernel of this file uses scratch memory (-Rpass-analysis=kernel-resource-usage: ScratchSize 0 throughout;
// the rocprim radix sort that orders the weights once per ipxk_crossover_run is the library's own).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>
#include <vector>

#include "context.hpp"
#include "trisolve.hpp"

namespace ipxk {

namespace {

constexpr int kCrossGrid = 512;          // workgroups of the two-stage reductions = threads of the kernels that finish them
constexpr int kRowLanes = 8;             // lanes per column in the gather passes
constexpr int kRowCols = kBlock / kRowLanes;
constexpr double kPivotZeroTol = 1e-5;   // src/crossover.h:137
constexpr ipxint kOptimal = 1, kImprecise = 2, kTimeLimit = 5, kFailed = 8;      // include/ipx_status.h
constexpr ipxint kBasic = 0, kNonbasicLb = -1, kNonbasicUb = -2, kSuperbasic = -3;

// the scalars of one candidate, written by the device, read by the host
struct CrossScalars {
    MvScalars mv;            // jn, pmax, jb, pivot_col, pivot_row, eta_nnz: what DeviceBasis reads and writes
    int blocked;             // the first pass found a blocking entry
    int winner;              // jn (PushDual) / pblock (PushPrimal); -1: none
    int block_at_lb;
    double step0;            // the full step: z[jb] / x[jn] - move_to
    double move_to;
    double step1;            // the step after the first pass
    double step;             // the step of the update
    double bound;            // PushPrimal: the bound the leaving variable takes
};

using MaxPart = Partial<1>;                      // (largest |pivot|, its smallest index)
struct MinPart { double v; int i; int c; };      // (least |ratio|, its smallest index), a count

__device__ __forceinline__ MinPart min_identity() { return MinPart{__builtin_huge_val(), INT_MAX, 0}; }
// the workgroup's partial: wavefront butterflies, then the wavefronts in order; valid in thread 0
template <int kThreads>
__device__ __forceinline__ MinPart block_min(MinPart p) {
    __shared__ MinPart sh[kThreads / 64];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(p.v, d, 64);
        const int oi = __shfl_xor(p.i, d, 64);
        take_smaller(p.v, p.i, ov, oi);
    }
    p.c = wave_sum(p.c);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < kThreads / 64; k++) { take_smaller(p.v, p.i, sh[k].v, sh[k].i); p.c += sh[k].c; }
    return p;
}

// ---- argument checks (the reference's logic_error, :89-101, :243-252) and set-up ---------------------------------------------
__global__ void cross_restrict_kernel(int64_t N, const double* __restrict__ x, const double* __restrict__ lb, const double* __restrict__ ub,
                                      const double* __restrict__ z, unsigned char* __restrict__ restr, int* bad) {
    IPXK_GRID_STRIDE(j, N) {
        const int r = (x[j] != ub[j] ? 1 : 0) | (x[j] != lb[j] ? 2 : 0);      // :351-355
        restr[j] = (unsigned char)r;
        if (((r & 1) && z[j] < 0.0) || ((r & 2) && z[j] > 0.0)) atomicAdd(bad, 1);      // (a count: no dependence on the order)
    }
}
__global__ void cross_check_primal_kernel(int64_t N, const double* __restrict__ x, const double* __restrict__ lb, const double* __restrict__ ub,
                                          const unsigned char* __restrict__ fixed, int* bad) {
    IPXK_GRID_STRIDE(j, N) {
        bool wrong = x[j] < lb[j] || x[j] > ub[j];
        if (fixed && fixed[j] && x[j] != lb[j] && x[j] != ub[j]) wrong = true;
        if (wrong) atomicAdd(bad, 1);
    }
}
__global__ void cross_posof_kernel(int64_t N, int m, const ipxint* __restrict__ basis, int* __restrict__ posof, int fill) {
    if (fill) { IPXK_GRID_STRIDE(j, N) posof[j] = -1; }
    else { IPXK_GRID_STRIDE(p, m) posof[basis[p]] = (int)p; }
}
// CopyBasic (:106-115)
__global__ void cross_copy_basic_kernel(int m, const ipxint* __restrict__ basis, const double* __restrict__ x, const double* __restrict__ lb,
                                        const double* __restrict__ ub, const unsigned char* __restrict__ fixed, double* __restrict__ xb,
                                        double* __restrict__ lbb, double* __restrict__ ubb) {
    IPXK_GRID_STRIDE(p, m) {
        const ipxint j = basis[p];
        xb[p] = x[j];
        const bool f = fixed && fixed[j];
        lbb[p] = f ? x[j] : lb[j];
        ubb[p] = f ? x[j] : ub[j];
    }
}
__global__ void cross_scatter_basic_kernel(int m, const ipxint* __restrict__ basis, const double* __restrict__ v, double* __restrict__ x) {
    IPXK_GRID_STRIDE(p, m) x[basis[p]] = v[p];
}
__global__ void cross_set_dual_kernel(int jb, int p, const double* z, CrossScalars* S) {
    S->mv.jn = jb; S->mv.pmax = p; S->mv.jb = jb; S->step0 = z[jb];
}
__global__ void cross_set_primal_kernel(int jn, double step0, double move_to, CrossScalars* S) {
    S->mv.jn = jn; S->mv.pmax = -1; S->mv.jb = -1; S->step0 = step0; S->move_to = move_to;
}

// ---- PushDual: the tableau row with the first pass of DualRatioTest fused in (:270-272, :424-440) ------------------------------
__device__ __forceinline__ bool dual_ratio(double zj, double r, int restr, double step0, double feastol, double* ratio) {
    if ((restr & 1) && zj - step0 * r < -feastol) { *ratio = (zj + feastol) / r; return true; }
    if ((restr & 2) && zj - step0 * r > feastol) { *ratio = (zj - feastol) / r; return true; }
    return false;
}
__global__ __launch_bounds__(kBlock) void cross_row_kernel(int n, int64_t N, const int* __restrict__ Ap, const int* __restrict__ Ai,
                                                           const double* __restrict__ Ax, const double* __restrict__ btran,
                                                           const int* __restrict__ posof, const double* __restrict__ z,
                                                           const unsigned char* __restrict__ restr, double feastol, const CrossScalars* S,
                                                           double* __restrict__ row, MinPart* part) {
    const double step0 = S->step0;
    MinPart p = min_identity();
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
            if (!nonbasic) sum = 0.0;
            row[j] = sum;
            double ratio;
            if (fabs(sum) > kPivotZeroTol && dual_ratio(z[j], sum, restr[j], step0, feastol, &ratio))
                take_smaller(p.v, p.i, fabs(ratio), (int)j);                 // (j ascends: the first of equals stays)
        }
    }
    p = block_min<kBlock>(p);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}
__global__ __launch_bounds__(kCrossGrid) void cross_dual_first_kernel(int nparts, const MinPart* part, const double* __restrict__ row,
                                                                      const double* __restrict__ z, const unsigned char* __restrict__ restr,
                                                                      double feastol, CrossScalars* S) {
    MinPart p = (int)threadIdx.x < nparts ? part[threadIdx.x] : min_identity();
    p = block_min<kCrossGrid>(p);
    if (threadIdx.x != 0) return;
    S->blocked = p.i != INT_MAX;
    S->step1 = S->step0;
    if (p.i != INT_MAX) {
        double ratio = 0.0;
        (void)dual_ratio(z[p.i], row[p.i], restr[p.i], S->step0, feastol, &ratio);
        S->step1 = ratio;
    }
}
// the second pass (:446-462): the largest |row_j| among the entries that block within the step
__global__ __launch_bounds__(kBlock) void cross_dual_second_kernel(int64_t N, const double* __restrict__ row, const double* __restrict__ z,
                                                                   const unsigned char* __restrict__ restr, const CrossScalars* S,
                                                                   MaxPart* part) {
    MaxPart p = partial_identity<1>();
    if (S->blocked) {
        const double step = S->step1;
        IPXK_GRID_STRIDE(j, N) {
            const double r = row[j], a = fabs(r);
            if (a > kPivotZeroTol && fabs(z[j] / r) <= fabs(step)) {
                const int rs = restr[j];
                if ((((rs & 1) && step * r > 0.0) || ((rs & 2) && step * r < 0.0)) && a > p.v[0]) { p.v[0] = a; p.i[0] = (int)j; }
            }
        }
    }
    p = block_partial<kBlock>(p);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}
// the decision (:275-300).  Blocked: jn enters, row[jn] is the pivot from the row, step = z[jn] / row[jn].  Not blocked: the full
// step -- and jb itself as the column of the FTRAN that is enqueued either way (a valid column, its result unused).
__global__ __launch_bounds__(kCrossGrid) void cross_dual_final_kernel(int nparts, const MaxPart* part, const double* __restrict__ row,
                                                                      const double* __restrict__ z, CrossScalars* S) {
    const MaxPart p = block_partial<kCrossGrid>(load_partial(nparts, part));
    if (threadIdx.x != 0) return;
    if (S->blocked && p.i[0] != INT_MAX) {
        const int jn = p.i[0];
        S->mv.jn = jn;
        S->mv.pivot_row = row[jn];
        S->winner = jn;
        S->step = z[jn] / row[jn];
    } else {
        S->mv.jn = S->mv.jb;
        S->mv.pivot_row = 0.0;
        S->winner = -1;
        S->step = S->step0;
    }
}
// the pivot from the column at the leaving position and the column's number of nonzeros (one workgroup)
__global__ __launch_bounds__(1024) void cross_column_kernel(int m, const double* __restrict__ lhs, CrossScalars* S) {
    __shared__ int red[1024 / 64];
    int cnt = 0;
    for (int p = threadIdx.x; p < m; p += 1024) cnt += lhs[p] != 0.0;
    cnt = wave_sum(cnt);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int k = 0; k < 1024 / 64; k++) t += red[k];
        S->mv.eta_nnz = t;
        S->mv.pivot_col = lhs[S->mv.pmax];
    }
}
__global__ void cross_exchange_kernel(const CrossScalars* S, ipxint* basis, int* posof) {
    const int jn = S->mv.jn, jb = S->mv.jb, p = S->mv.pmax;
    basis[p] = jn;
    posof[jn] = p;
    posof[jb] = -1;
}
// y += step btran, z[j] -= step row[j] with the two clamps, z[jb] -= step, z[jn] = 0 (:302-320); the nonzeros only, as for_each_nonzero
__global__ void cross_dual_update_kernel(int64_t N, int m, const double* __restrict__ row, const double* __restrict__ btran,
                                         const unsigned char* __restrict__ restr, const CrossScalars* S, double* __restrict__ y,
                                         double* __restrict__ z) {
    const double step = S->step;
    const int jn = S->winner, jb = S->mv.jb;
    IPXK_GRID_STRIDE(j, N) {
        if ((int)j == jn) { z[j] = 0.0; continue; }                  // make clean
        if (step == 0.0) continue;
        if ((int)j == jb) { z[j] -= step; continue; }
        const double r = row[j];
        if (r != 0.0) {
            double v = z[j] - step * r;
            const int rs = restr[j];
            if (rs & 1) v = fmax(v, 0.0);
            if (rs & 2) v = fmin(v, 0.0);
            z[j] = v;
        }
    }
    if (step != 0.0) IPXK_GRID_STRIDE(i, m) { const double t = btran[i]; if (t != 0.0) y[i] += step * t; }
}

// ---- PushPrimal: PrimalRatioTest over the positions (:359-416) ------------------------------------------------------------------
__device__ __forceinline__ bool primal_ratio(double xb, double pivot, double lbb, double ubb, double step0, double feastol, double* ratio) {
    if (xb + step0 * pivot < lbb - feastol) { *ratio = (lbb - xb - feastol) / pivot; return true; }
    if (xb + step0 * pivot > ubb + feastol) { *ratio = (ubb - xb + feastol) / pivot; return true; }
    return false;
}
__global__ __launch_bounds__(kBlock) void cross_primal_first_kernel(int m, const double* __restrict__ lhs, const double* __restrict__ xb,
                                                                    const double* __restrict__ lbb, const double* __restrict__ ubb,
                                                                    double feastol, const CrossScalars* S, MinPart* part) {
    const double step0 = S->step0;
    MinPart p = min_identity();
    IPXK_GRID_STRIDE(q, m) {
        const double pivot = lhs[q];
        double ratio;
        if (fabs(pivot) > kPivotZeroTol && primal_ratio(xb[q], pivot, lbb[q], ubb[q], step0, feastol, &ratio))
            take_smaller(p.v, p.i, fabs(ratio), (int)q);
        p.c += pivot != 0.0;
    }
    p = block_min<kBlock>(p);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}
__global__ __launch_bounds__(kCrossGrid) void cross_primal_first_final_kernel(int nparts, const MinPart* part, const double* __restrict__ lhs,
                                                                              const double* __restrict__ xb, const double* __restrict__ lbb,
                                                                              const double* __restrict__ ubb, double feastol, CrossScalars* S) {
    MinPart p = (int)threadIdx.x < nparts ? part[threadIdx.x] : min_identity();
    p = block_min<kCrossGrid>(p);
    if (threadIdx.x != 0) return;
    S->mv.eta_nnz = p.c;
    S->blocked = p.i != INT_MAX;
    S->step1 = S->step0;
    if (p.i != INT_MAX) {
        double ratio = 0.0;
        (void)primal_ratio(xb[p.i], lhs[p.i], lbb[p.i], ubb[p.i], S->step0, feastol, &ratio);
        S->step1 = ratio;
    }
}
__global__ __launch_bounds__(kBlock) void cross_primal_second_kernel(int m, const double* __restrict__ lhs, const double* __restrict__ xb,
                                                                     const double* __restrict__ lbb, const double* __restrict__ ubb,
                                                                     const CrossScalars* S, MaxPart* part) {
    MaxPart p = partial_identity<1>();
    if (S->blocked) {
        const double step = S->step1;
        IPXK_GRID_STRIDE(q, m) {
            const double pivot = lhs[q], a = fabs(pivot);
            if (a > kPivotZeroTol && a > p.v[0]) {
                bool ok = false;
                if (step * pivot < 0.0) ok = fabs((lbb[q] - xb[q]) / pivot) <= fabs(step);
                if (step * pivot > 0.0) ok = fabs((ubb[q] - xb[q]) / pivot) <= fabs(step);
                if (ok) { p.v[0] = a; p.i[0] = (int)q; }
            }
        }
    }
    p = block_partial<kBlock>(p);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}
// the decision (:147-175).  Blocked: the variable at pblock leaves, the step comes from lbbasic / ubbasic (0 when a fixed-at-bound
// variable blocks).  Not blocked: the full step -- and position -1 for the BTRAN that is enqueued either way (the zero vector).
__global__ __launch_bounds__(kCrossGrid) void cross_primal_final_kernel(int nparts, const MaxPart* part, const double* __restrict__ lhs,
                                                                        const double* __restrict__ xb, const double* __restrict__ lbb,
                                                                        const double* __restrict__ ubb, const ipxint* __restrict__ basis,
                                                                        CrossScalars* S) {
    const MaxPart p = block_partial<kCrossGrid>(load_partial(nparts, part));
    if (threadIdx.x != 0) return;
    if (S->blocked && p.i[0] != INT_MAX) {
        const int q = p.i[0];
        const double pivot = lhs[q];
        const bool at_lb = S->step1 * pivot < 0.0;
        const double bound = at_lb ? lbb[q] : ubb[q];
        S->mv.pmax = q;
        S->mv.jb = (int)basis[q];
        S->mv.pivot_col = pivot;
        S->winner = q;
        S->block_at_lb = at_lb;
        S->bound = bound;
        S->step = (bound - xb[q]) / pivot;
    } else {
        S->mv.pmax = -1;
        S->mv.jb = -1;
        S->mv.pivot_col = 0.0;
        S->winner = -1;
        S->block_at_lb = 1;
        S->bound = 0.0;
        S->step = S->step0;
    }
}
// xbasic += step ftran with the clamps, x[jn] -= step, make clean, and the position's three entries replaced by jn's (:176-198)
__global__ void cross_primal_update_kernel(int m, const double* __restrict__ lhs, const double* __restrict__ lb, const double* __restrict__ ub,
                                           const CrossScalars* S, double* __restrict__ xb, double* __restrict__ lbb, double* __restrict__ ubb,
                                           double* __restrict__ x, ipxint* basis, int* posof) {
    const double step = S->step;
    const int pblock = S->winner, jn = S->mv.jn;
    IPXK_GRID_STRIDE(q, m) {
        const double f = lhs[q];
        if (step != 0.0 && f != 0.0) {
            double v = xb[q] + step * f;
            v = fmax(v, lbb[q]);
            v = fmin(v, ubb[q]);
            xb[q] = v;
        }
        if ((int)q == pblock) {                                      // (one thread: nobody else touches x[jn], x[jb])
            const int jb = S->mv.jb;
            const double xn = step != 0.0 ? x[jn] - step : x[jn];
            x[jb] = S->bound;
            x[jn] = xn;
            xb[q] = xn;
            lbb[q] = lb[jn];
            ubb[q] = ub[jn];
            basis[q] = jn;
            posof[jn] = (int)q;
            posof[jb] = -1;
        }
    }
    if (pblock < 0 && blockIdx.x == 0 && threadIdx.x == 0) x[jn] = S->move_to;
}

// ---- the basic solution (src/basis.cc:324-351) ---------------------------------------------------------------------------------
// rhs = b - N x_N, row by row from the row-wise copy (columns ascend within a row: the order of the reference's scatter loop)
__global__ void cross_b_minus_nx_kernel(int m, int n, const int* __restrict__ Tp, const int* __restrict__ Ti, const double* __restrict__ Tx,
                                        const double* __restrict__ b, const int* __restrict__ posof, const double* __restrict__ x,
                                        double* __restrict__ out) {
    IPXK_GRID_STRIDE(i, m) {
        double v = b[i];
        for (int q = Tp[i]; q < Tp[i + 1]; q++) {
            const int j = Ti[q];
            if (posof[j] < 0) v += -x[j] * Tx[q];
        }
        if (posof[n + i] < 0) v += -x[n + i];
        out[i] = v;
    }
}
__global__ void cross_cb_minus_zb_kernel(int m, const ipxint* __restrict__ basis, const double* __restrict__ cc, const double* __restrict__ z,
                                         double* __restrict__ out) {
    IPXK_GRID_STRIDE(p, m) out[p] = cc[basis[p]] - z[basis[p]];
}
// z_j = c_j - a_j'y on the nonbasic j: one gather pass, eight lanes per column
__global__ __launch_bounds__(kBlock) void cross_reduced_costs_kernel(int n, int64_t N, const int* __restrict__ Ap, const int* __restrict__ Ai,
                                                                     const double* __restrict__ Ax, const double* __restrict__ y,
                                                                     const int* __restrict__ posof, const double* __restrict__ cc,
                                                                     double* __restrict__ z) {
    const int lane = threadIdx.x & (kRowLanes - 1), sub = threadIdx.x / kRowLanes;
    for (int64_t base = (int64_t)blockIdx.x * kRowCols; base < N; base += (int64_t)gridDim.x * kRowCols) {
        const int64_t j = base + sub;
        const bool nonbasic = j < N && posof[j] < 0;
        double sum = 0.0;
        if (nonbasic && j < n)
            for (int q = Ap[j] + lane; q < Ap[j + 1]; q += kRowLanes) sum += Ax[q] * y[Ai[q]];
        sum = wave_sum<kRowLanes>(sum);
        if (lane == 0 && nonbasic) z[j] = cc[j] - (j >= n ? y[j - n] : sum);
    }
}
// the basic statuses (src/lp_solver.cc:499-512) and the two infeasibilities (src/model.cc:69-97) as block maxima
__global__ __launch_bounds__(kBlock) void cross_statuses_kernel(int64_t N, const int* __restrict__ posof, const double* __restrict__ x,
                                                                const double* __restrict__ z, const double* __restrict__ lb,
                                                                const double* __restrict__ ub, ipxint* __restrict__ statuses,
                                                                double* __restrict__ part) {
    __shared__ double scratch[2][kBlock / 64 + 1];
    double pinf = 0.0, dinf = 0.0;
    IPXK_GRID_STRIDE(j, N) {
        ipxint st;
        if (posof[j] >= 0) st = kBasic;
        else if (lb[j] == ub[j]) st = z[j] >= 0.0 ? kNonbasicLb : kNonbasicUb;
        else if (x[j] == lb[j]) st = kNonbasicLb;
        else if (x[j] == ub[j]) st = kNonbasicUb;
        else st = kSuperbasic;
        statuses[j] = st;
        pinf = fmax(pinf, fmax(lb[j] - x[j], x[j] - ub[j]));
        if (x[j] > lb[j]) dinf = fmax(dinf, z[j]);
        if (x[j] < ub[j]) dinf = fmax(dinf, -z[j]);
    }
    block_reduce2<MaxOp, MaxOp>(pinf, dinf, scratch[0], scratch[1]);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = pinf; part[2 * blockIdx.x + 1] = dinf; }
}
__global__ void cross_iota_kernel(int64_t N, int* v) { IPXK_GRID_STRIDE(j, N) v[j] = (int)j; }

// ---- what the four entry points share ------------------------------------------------------------------------------------------
struct Pushes {
    Context* c;
    const int m, n;
    const int64_t N;
    hipStream_t s;
    MaxvolState& M;
    ipxk_crossover_params prm;
    ipxk_crossover_info I{};
    DevBuf<ipxint>& basis;
    DevBuf<int> posof;
    DevBuf<MinPart> minpart;
    DevBuf<double> row, xb, lbb, ubb;
    DevBuf<unsigned char> restr, fixed;
    DevBuf<int> bad;
    CrossScalars *S = nullptr, *pinned = nullptr;
    std::unique_ptr<DeviceBasis> Bp;
    std::vector<int> pos_h;
    std::vector<double> ones;
    ipxint* log;
    ipxint log_cap, pivots = 0;
    ipxk_interrupt_fn interrupt;
    void* user;
    int gm, gN, grow;

    Pushes(Context* ctx, const ipxk_crossover_params* p, ipxint* log_, ipxint log_cap_, ipxk_interrupt_fn f, void* u)
        : c(ctx), m((int)ctx->m), n((int)ctx->n), N(ctx->n + ctx->m), s(ctx->stream), M(*(ctx->maxvol ? ctx->maxvol : (ctx->maxvol = new MaxvolState))),
          basis(M.drop_basis), log(log_), log_cap(log_cap_), interrupt(f), user(u) {
        prm = p ? *p : ipxk_crossover_params{1e-7, 1e-7, 100};
        IPXK_REQUIRE(prm.primal_feastol >= 0.0 && prm.dual_feastol >= 0.0 && std::isfinite(prm.primal_feastol) && std::isfinite(prm.dual_feastol),
                     "the feasibility tolerances must be finite and not negative");
        gm = grid_for(m, kCrossGrid);
        gN = grid_for(N, kCrossGrid);
        grow = (int)std::min<int64_t>(kCrossGrid, (N + kRowCols - 1) / kRowCols);
    }
    // the given basis: its mirrors, fresh factors and the operator of the sweeps with unit scaling factors.  false: singular (301)
    bool factorize(const ipxint* basis_in) {
        IPXK_REQUIRE(!comm_active(c), kDeviceLuRefusal);
        IPXK_REQUIRE(c->have_plain, "no resident copy of the matrix");
        IPXK_REQUIRE(m > 0, "empty model");
        pos_h.assign((size_t)N, -1);
        for (int p = 0; p < m; p++) {
            const ipxint j = basis_in[p];
            IPXK_REQUIRE(j >= 0 && j < N && pos_h[(size_t)j] < 0, "basis holds an index out of range or twice");
            pos_h[(size_t)j] = p;
        }
        M.part.ensure(kCrossGrid);
        minpart.ensure(kCrossGrid);
        M.scalars.ensure(1);                       // (the compact eta lists report their size there)
        M.drop_scalars.ensure(sizeof(CrossScalars));
        if (M.drop_h_bytes < sizeof(CrossScalars)) {
            if (M.drop_h) { (void)hipHostFree(M.drop_h); M.drop_h = nullptr; M.drop_h_bytes = 0; }
            IPXK_HIP(hipHostMalloc(&M.drop_h, sizeof(CrossScalars)));
            M.drop_h_bytes = sizeof(CrossScalars);
        }
        S = reinterpret_cast<CrossScalars*>(M.drop_scalars.get());
        pinned = static_cast<CrossScalars*>(M.drop_h);
        IPXK_HIP(hipMemsetAsync(S, 0, sizeof(CrossScalars), s));
        ones.assign((size_t)N, 1.0);
        maxvol_drop_etas(c);
        Bp.reset(new DeviceBasis(c, M, prm.max_etas > 0 ? prm.max_etas : 100, false, ones.data(), &S->mv));
        DeviceBasis& B = *Bp;
        B.basis_h.assign(basis_in, basis_in + m);
        B.status_h.assign((size_t)N, IPXK_NONBASIC);
        for (int p = 0; p < m; p++) B.status_h[(size_t)basis_in[p]] = IPXK_BASIC;
        basis.upload(B.basis_h, s);
        posof.ensure((size_t)N);
        hipLaunchKernelGGL(cross_posof_kernel, dim3(gN), dim3(kBlock), 0, s, N, m, basis.get(), posof.get(), 1);
        hipLaunchKernelGGL(cross_posof_kernel, dim3(gm), dim3(kBlock), 0, s, N, m, basis.get(), posof.get(), 0);
        bad.ensure(1);
        IPXK_HIP(hipMemsetAsync(bad.get(), 0, sizeof(int), s));
        if (!B.refactorize()) { I.errflag = B.errflag; return false; }
        return true;
    }
    int read_bad() {
        int v = 0;
        staged_d2h(&v, bad.get(), sizeof(int), s);
        IPXK_HIP(hipStreamSynchronize(s));
        IPXK_HIP(hipMemsetAsync(bad.get(), 0, sizeof(int), s));
        return v;
    }
    ipxint poll() {
        if (interrupt) return interrupt(user);
        return c->interrupt ? c->interrupt(c->interrupt_user) : 0;
    }
    // an accepted exchange: the host's part.  false: the candidate is tried again (or the basis has raised its errflag)
    bool accept(const CrossScalars& a) {
        DeviceBasis& B = *Bp;
        if (!B.exchange_if_stable(a.mv)) return false;
        pos_h[(size_t)a.mv.jn] = a.mv.pmax;
        pos_h[(size_t)a.mv.jb] = -1;
        if (log && pivots < log_cap) { log[2 * pivots] = a.mv.jb; log[2 * pivots + 1] = a.mv.jn; }
        pivots++;
        return true;
    }
    void set_status(ipxint err) {
        if (err == 999) { I.errflag = 0; I.status_crossover = kTimeLimit; }
        else if (err != 0) { I.errflag = err; I.status_crossover = kFailed; }
        else { I.errflag = 0; I.status_crossover = kOptimal; }
    }

    // Crossover::PushDual (:229-357).  z_h: the host's copy of z at entry (a basic candidate's z does not change before its turn)
    void push_dual(const double* x, const double* lb, const double* ub, double* y, double* z, const std::vector<ipxint>& variables,
                   const std::vector<double>& z_h) {
        const double t0 = now_s();
        DeviceBasis& B = *Bp;
        const double feastol = prm.dual_feastol;
        for (ipxint j : variables) IPXK_REQUIRE(j >= 0 && j < N && pos_h[(size_t)j] >= 0, "invalid variable in PushDual: not basic");
        restr.ensure((size_t)N);
        row.ensure((size_t)N);
        hipLaunchKernelGGL(cross_restrict_kernel, dim3(gN), dim3(kBlock), 0, s, N, x, lb, ub, z, restr.get(), bad.get());
        IPXK_REQUIRE(read_bad() == 0, "sign condition violated in PushDual");
        ipxint err = 0;
        size_t next = 0;
        while (next < variables.size() && !B.errflag) {
            if ((err = poll()) != 0) break;
            const int jb = (int)variables[next];
            if (z_h[(size_t)jb] == 0.0) { next++; continue; }         // nothing to do
            const int p = pos_h[(size_t)jb];
            hipLaunchKernelGGL(cross_set_dual_kernel, dim3(1), dim3(1), 0, s, jb, p, z, S);
            B.btran_unit();
            hipLaunchKernelGGL(cross_row_kernel, dim3(grow), dim3(kBlock), 0, s, n, N, c->pl_Ap.get(), c->pl_Ai.get(), c->pl_Ax.get(), B.btran,
                               posof.get(), z, restr.get(), feastol, S, row.get(), minpart.get());
            hipLaunchKernelGGL(cross_dual_first_kernel, dim3(1), dim3(kCrossGrid), 0, s, grow, minpart.get(), row.get(), z, restr.get(), feastol, S);
            hipLaunchKernelGGL(cross_dual_second_kernel, dim3(gN), dim3(kBlock), 0, s, N, row.get(), z, restr.get(), S, M.part.get());
            hipLaunchKernelGGL(cross_dual_final_kernel, dim3(1), dim3(kCrossGrid), 0, s, gN, M.part.get(), row.get(), z, S);
            // the FTRAN of the entering variable (ExchangeIfStable with sys = +1): pivot from the column, and the eta
            B.ftran();
            hipLaunchKernelGGL(cross_column_kernel, dim3(1), dim3(1024), 0, s, m, B.lhs, S);
            const CrossScalars a = read_scalars(S, pinned, s);
            if (a.blocked) {
                IPXK_REQUIRE(a.winner >= 0, "DualRatioTest: the second pass found no pivot");
                if (!accept(a)) continue;                             // "factorization was unstable, try again" (:291-292)
                hipLaunchKernelGGL(cross_exchange_kernel, dim3(1), dim3(1), 0, s, S, basis.get(), posof.get());
                I.dual_pivots++;
            }
            hipLaunchKernelGGL(cross_dual_update_kernel, dim3(gN), dim3(kBlock), 0, s, N, m, row.get(), B.btran, restr.get(), S, y, z);
            if (a.blocked) B.commit(a.mv);
            I.dual_pushes++;
            next++;
        }
        set_status(B.errflag ? B.errflag : err);
        I.seconds_dual = now_s() - t0;
    }

    // Crossover::PushPrimal (:73-220).  x_h, lb_h, ub_h: host copies at entry (a nonbasic candidate's x does not change before its turn)
    void push_primal(double* x, const double* lb, const double* ub, const std::vector<ipxint>& variables, const unsigned char* fixed_h,
                     const std::vector<double>& x_h, const std::vector<double>& lb_h, const std::vector<double>& ub_h) {
        const double t0 = now_s();
        DeviceBasis& B = *Bp;
        const double feastol = prm.primal_feastol;
        for (ipxint j : variables) IPXK_REQUIRE(j >= 0 && j < N && pos_h[(size_t)j] < 0, "invalid variable in PushPrimal: not nonbasic");
        const unsigned char* dfixed = nullptr;
        if (fixed_h) { fixed.ensure((size_t)N); staged_h2d(fixed.get(), fixed_h, (size_t)N, s); dfixed = fixed.get(); }
        hipLaunchKernelGGL(cross_check_primal_kernel, dim3(gN), dim3(kBlock), 0, s, N, x, lb, ub, dfixed, bad.get());
        IPXK_REQUIRE(read_bad() == 0, "bound condition violated in PushPrimal");
        xb.ensure((size_t)m); lbb.ensure((size_t)m); ubb.ensure((size_t)m);
        hipLaunchKernelGGL(cross_copy_basic_kernel, dim3(gm), dim3(kBlock), 0, s, m, basis.get(), x, lb, ub, dfixed, xb.get(), lbb.get(), ubb.get());
        ipxint err = 0;
        size_t next = 0;
        while (next < variables.size() && !B.errflag) {
            if ((err = poll()) != 0) break;
            const int jn = (int)variables[next];
            const double xj = x_h[(size_t)jn], l = lb_h[(size_t)jn], u = ub_h[(size_t)jn];
            if (xj == l || xj == u || (xj == 0.0 && std::isinf(l) && std::isinf(u))) { next++; continue; }      // nothing to do
            // the bound to push to: the nearer of two finite ones (ties to lb), the finite one, 0 for a free variable (:132-138)
            double move_to = 0.0;
            if (std::isfinite(l) && std::isfinite(u)) move_to = xj - l <= u - xj ? l : u;
            else if (std::isfinite(l)) move_to = l;
            else if (std::isfinite(u)) move_to = u;
            hipLaunchKernelGGL(cross_set_primal_kernel, dim3(1), dim3(1), 0, s, jn, xj - move_to, move_to, S);
            B.ftran();
            hipLaunchKernelGGL(cross_primal_first_kernel, dim3(gm), dim3(kBlock), 0, s, m, B.lhs, xb.get(), lbb.get(), ubb.get(), feastol, S, minpart.get());
            hipLaunchKernelGGL(cross_primal_first_final_kernel, dim3(1), dim3(kCrossGrid), 0, s, gm, minpart.get(), B.lhs, xb.get(), lbb.get(),
                               ubb.get(), feastol, S);
            hipLaunchKernelGGL(cross_primal_second_kernel, dim3(gm), dim3(kBlock), 0, s, m, B.lhs, xb.get(), lbb.get(), ubb.get(), S, M.part.get());
            hipLaunchKernelGGL(cross_primal_final_kernel, dim3(1), dim3(kCrossGrid), 0, s, gm, M.part.get(), B.lhs, xb.get(), lbb.get(), ubb.get(),
                               basis.get(), S);
            // the BTRAN of the leaving variable (ExchangeIfStable with sys = -1): pivot from the row
            B.btran_unit();
            mv_pivot_from_row(c, B.btran, &S->mv);
            const CrossScalars a = read_scalars(S, pinned, s);
            if (a.blocked) {
                IPXK_REQUIRE(a.winner >= 0, "PrimalRatioTest: the second pass found no pivot");
                if (!accept(a)) continue;                             // (:165-166)
                I.primal_pivots++;
            }
            hipLaunchKernelGGL(cross_primal_update_kernel, dim3(gm), dim3(kBlock), 0, s, m, B.lhs, lb, ub, S, xb.get(), lbb.get(), ubb.get(), x,
                               basis.get(), posof.get());
            if (a.blocked) B.commit(a.mv);
            I.primal_pushes++;
            next++;
        }
        hipLaunchKernelGGL(cross_scatter_basic_kernel, dim3(gm), dim3(kBlock), 0, s, m, basis.get(), xb.get(), x);
        set_status(B.errflag ? B.errflag : err);
        I.seconds_primal = now_s() - t0;
    }

    // fresh factors of the basis returned where etas stand behind the old ones; the counters of the basis
    void finish(ipxint* basis_io) {
        DeviceBasis& B = *Bp;
        IPXK_HIP(hipStreamSynchronize(s));
        IPXK_HIP(hipGetLastError());
        check_sweep_abort(c);
        if (!B.errflag && B.etas.K > 0 && !B.refactorize()) { I.errflag = B.errflag; I.status_crossover = kFailed; }
        IPXK_HIP(hipStreamSynchronize(s));
        std::copy(B.basis_h.begin(), B.basis_h.end(), basis_io);
        I.refused = B.refused;
        I.factorizations = B.factorizations;
    }

    // Basis::ComputeBasicSolution on the context's (fresh) factors of `basis`
    void basic_solution(const double* b, const double* cc, double* x, double* y, double* z) {
        DeviceBasis& B = *Bp;
        hipLaunchKernelGGL(cross_b_minus_nx_kernel, dim3(gm), dim3(kBlock), 0, s, m, n, c->pl_Tp.get(), c->pl_Ti.get(), c->pl_Tx.get(), b, posof.get(), x, B.rhs);
        solve_dense_dev(c, B.rhs, B.lhs, 'N');
        hipLaunchKernelGGL(cross_scatter_basic_kernel, dim3(gm), dim3(kBlock), 0, s, m, basis.get(), B.lhs, x);
        hipLaunchKernelGGL(cross_cb_minus_zb_kernel, dim3(gm), dim3(kBlock), 0, s, m, basis.get(), cc, z, B.unit);
        solve_dense_dev(c, B.unit, y, 'T');
        hipLaunchKernelGGL(cross_reduced_costs_kernel, dim3(grow), dim3(kBlock), 0, s, n, N, c->pl_Ap.get(), c->pl_Ai.get(), c->pl_Ax.get(), y,
                           posof.get(), cc, z);
    }
};

std::vector<double> download(const double* dev, size_t len, hipStream_t s) {
    std::vector<double> h(len);
    if (len) staged_d2h(h.data(), dev, len * sizeof(double), s);
    IPXK_HIP(hipStreamSynchronize(s));
    return h;
}

}  // namespace

void crossover_push_dual_dev(Context* c, const double* lb, const double* ub, const double* x, double* y, double* z, const ipxint* variables,
                             ipxint num_variables, ipxint* basis, const ipxk_crossover_params* prm, ipxk_crossover_info* info, ipxint* log,
                             ipxint log_cap, ipxk_interrupt_fn interrupt, void* user) {
    Pushes P(c, prm, log, log_cap, interrupt, user);
    if (P.factorize(basis)) {
        const std::vector<ipxint> vars(variables, variables + num_variables);
        P.I.dual_superbasics = num_variables;
        P.push_dual(x, lb, ub, y, z, vars, download(z, (size_t)P.N, P.s));
        P.finish(basis);
    } else {
        P.I.status_crossover = kFailed;
    }
    *info = P.I;
}

void crossover_push_primal_dev(Context* c, const double* lb, const double* ub, double* x, const ipxint* variables, ipxint num_variables,
                               const unsigned char* fixed_at_bound, ipxint* basis, const ipxk_crossover_params* prm, ipxk_crossover_info* info,
                               ipxint* log, ipxint log_cap, ipxk_interrupt_fn interrupt, void* user) {
    Pushes P(c, prm, log, log_cap, interrupt, user);
    if (P.factorize(basis)) {
        const std::vector<ipxint> vars(variables, variables + num_variables);
        P.I.primal_superbasics = num_variables;
        const size_t N = (size_t)P.N;
        P.push_primal(x, lb, ub, vars, fixed_at_bound, download(x, N, P.s), download(lb, N, P.s), download(ub, N, P.s));
        P.finish(basis);
    } else {
        P.I.status_crossover = kFailed;
    }
    *info = P.I;
}

void crossover_basic_solution_dev(Context* c, const double* b, const double* cc, const ipxint* basis, double* x, double* y, double* z) {
    Pushes P(c, nullptr, nullptr, 0, nullptr, nullptr);
    IPXK_REQUIRE(P.factorize(basis), "the basis is singular");
    P.basic_solution(b, cc, x, y, z);
    IPXK_HIP(hipStreamSynchronize(P.s));
    IPXK_HIP(hipGetLastError());
    check_sweep_abort(c);
}

void crossover_run_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub, const double* weights, ipxint* basis,
                       const ipxk_crossover_params* prm, ipxk_crossover_info* info, double* x, double* y, double* z, ipxint* statuses_out,
                       ipxint* log, ipxint log_cap, ipxk_interrupt_fn interrupt, void* user) {
    IPXK_REQUIRE(!comm_active(c), kDeviceLuRefusal);
    IPXK_REQUIRE(c->it_set, "no iterate on the device (ipxk_iterate_set)");
    IPXK_REQUIRE(c->postprocessed, "the resident iterate has not been postprocessed (ipxk_iterate_postprocess)");
    Pushes P(c, prm, log, log_cap, interrupt, user);
    hipStream_t s = P.s;
    const int64_t N = P.N;
    // 1. the complementary point
    iterate_drop_to_complementarity_dev(c, lb, ub, x, y, z);
    // 2. the order: Sortperm (src/utils.cc:87-104), ascending by (weight, index) -- a stable sort of the weights
    std::vector<int> perm((size_t)N);
    {
        DevBuf<double> w((size_t)N), wsorted((size_t)N);
        DevBuf<int> iota((size_t)N), order((size_t)N), flag(1);
        if (weights) IPXK_HIP(hipMemcpyAsync(w.get(), weights, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, s));
        else { IPXK_HIP(hipMemsetAsync(flag.get(), 0, sizeof(int), s)); iterate_scaling_factors_dev(c, w.get(), flag.get()); }
        hipLaunchKernelGGL(cross_iota_kernel, dim3(P.gN), dim3(kBlock), 0, s, N, iota.get());
        size_t bytes = 0;
        IPXK_HIP(rocprim::radix_sort_pairs(nullptr, bytes, w.get(), wsorted.get(), iota.get(), order.get(), (size_t)N, 0, 64, s));
        DevBuf<unsigned char> tmp(bytes > 0 ? bytes : 1);
        IPXK_HIP(rocprim::radix_sort_pairs(tmp.get(), bytes, w.get(), wsorted.get(), iota.get(), order.get(), (size_t)N, 0, 64, s));
        order.download(perm.data(), (size_t)N, s);
        IPXK_HIP(hipStreamSynchronize(s));
    }
    if (!P.factorize(basis)) { P.I.status_crossover = kFailed; *info = P.I; return; }
    // 3. PushAll (:15-71)
    {
        const std::vector<double> z_h = download(z, (size_t)N, s);
        std::vector<ipxint> dual;
        for (int64_t k = 0; k < N; k++) { const int j = perm[(size_t)k]; if (P.pos_h[(size_t)j] >= 0 && z_h[(size_t)j] != 0.0) dual.push_back(j); }
        P.I.dual_superbasics = (ipxint)dual.size();
        P.push_dual(x, lb, ub, y, z, dual, z_h);
    }
    if (P.I.status_crossover == kOptimal) {
        const std::vector<double> x_h = download(x, (size_t)N, s), lb_h = download(lb, (size_t)N, s), ub_h = download(ub, (size_t)N, s);
        std::vector<ipxint> primal;
        for (int64_t k = N - 1; k >= 0; k--) {
            const int j = perm[(size_t)k];
            const double xj = x_h[(size_t)j], l = lb_h[(size_t)j], u = ub_h[(size_t)j];
            if (P.pos_h[(size_t)j] < 0 && xj != l && xj != u && !(std::isinf(l) && std::isinf(u) && xj == 0.0)) primal.push_back(j);
        }
        P.I.primal_superbasics = (ipxint)primal.size();
        P.push_primal(x, lb, ub, primal, nullptr, x_h, lb_h, ub_h);
    }
    P.finish(basis);
    if (P.I.status_crossover != kOptimal) { *info = P.I; return; }             // (the point is discarded)
    // 4. - 7. the vertex, its statuses and infeasibilities
    P.basic_solution(b, cc, x, y, z);
    {
        DevBuf<ipxint> st((size_t)N);
        DevBuf<double> part((size_t)2 * P.gN);
        hipLaunchKernelGGL(cross_statuses_kernel, dim3(P.gN), dim3(kBlock), 0, s, N, P.posof.get(), x, z, lb, ub, st.get(), part.get());
        std::vector<double> part_h((size_t)2 * P.gN);
        part.download(part_h.data(), part_h.size(), s);
        if (statuses_out) st.download(statuses_out, (size_t)N, s);
        IPXK_HIP(hipStreamSynchronize(s));
        for (int k = 0; k < P.gN; k++) {
            P.I.primal_infeas = std::max(P.I.primal_infeas, part_h[(size_t)2 * k]);
            P.I.dual_infeas = std::max(P.I.dual_infeas, part_h[(size_t)2 * k + 1]);
        }
    }
    IPXK_HIP(hipGetLastError());
    check_sweep_abort(c);
    if (P.I.primal_infeas > P.prm.primal_feastol || P.I.dual_infeas > P.prm.dual_feastol) P.I.status_crossover = kImprecise;
    *info = P.I;
}

}  // namespace ipxk
