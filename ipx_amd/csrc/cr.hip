// Conjugate Residuals on the device             reference src/conjugate_residuals.cc
//   preconditioned CR (:90-213) for the diag path, plain CR (:14-88) for the basis path.
//
// The whole loop runs on the GPU without a host round trip per iteration:
//  * vectors and the loop scalars (cdot, alpha, beta, iteration count, errflag) live in HBM;
//  * every dot product / norm is produced as per-workgroup partials by the kernel that
//    touches the data anyway and is finished redundantly (bitwise identically) by every
//    workgroup of the consuming kernel -- no atomics, no extra "finalize" launches;
//  * the termination test, the error checks (:139-171) and the every-5th-iteration
//    refresh with its monotonicity check (:186-207) are evaluated by the control kernel,
//    which turns all later kernels into no-ops once `done` is set;
//  * single rank: the host follows two words in mapped host memory.  The direction kernel stores the number
//    of finished iterations into the progress word, the control kernel sets a flag together with `done`.
//    The host enqueues iteration k once progress >= k - R (R = kAhead iterations of run-ahead) and leaves
//    the loop when the flag is set: at most R + 1 iterations are enqueued past the final one, whatever the
//    timing, and nothing but the iterations themselves goes into the queue (no snapshot kernel, no event);
//  * partitioned, and single rank with IPXK_CR_PACE=cycles (the driver before; A/B runs and tests): the host
//    enqueues cycles of 5 iterations, stays at most kWindow cycles ahead of the GPU and leaves the loop by a
//    snapshot of `done` per cycle (partitioned: agreed between the ranks by an all-reduce).
// Steady state per PCR iteration: 4 launches (control, SpMV pass 1, SpMV pass 2, direction).  PcrDiag, single
// rank: the refresh of every fifth iteration (sresidual = residual ./ diag and the partials of
// residual'*sresidual) is made by that iteration's direction kernel (REFRESH), which has sresidual[i] and
// diag[i] in registers already; IPXK_CR_REFRESH=0 keeps it a launch of its own (same bits).
// The control kernel is the one pass 1 waits for; it updates the residuals only (PcrDiag: reads
// Cstep, residual, sresidual, diag, resscale, writes residual, sresidual: 7 vector accesses).  The
// solution update lhs += alpha*step of the same iteration is made by the direction kernel, which
// loads step anyway (reads (s)residual, step, Cres, Cstep, diag, lhs, writes step, Cstep, lhs: 9);
// alpha travels through CrState.  16 accesses per iteration, against 17 with the update in the
// control kernel (IPXK_CR_LAZY=0: that order, same bits) and ~22 in the unfused formulation.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <thread>

#include "context.hpp"
#include "spmv_kernels.hpp"

namespace ipxk {

constexpr int kWindow = 2;  // cycles (of 5 iterations) the host may run ahead (driver paced by cycles)
constexpr int kAhead = 3;   // iterations the host may run ahead (driver paced by the progress word); IPXK_CR_AHEAD

enum CrMode { kModePcrDiag = 0, kModePcrSmw = 1, kModePlain = 2 };

// The two vector kernels of an iteration run vec_grid(m) workgroups, which at 1M rows leaves a thread 4 elements of
// the grid-stride loop.  Taken one at a time, each element's loads wait for the stores of the one before (the
// vectors may alias as far as the compiler knows): 4 dependent round trips to HBM per thread.  So a thread loads
// kCrUnroll elements (indices clamped to the last one, so that the loads need no predicate), then updates and
// stores them in ascending order -- the same operations on the same values, and a thread's sums in the same order.
constexpr int kCrUnroll = 4;

struct CrVecs {
    int m;
    double* lhs;
    double* residual;
    double* sresidual;   // PCR only
    double* step;
    double* Cstep;
    double* Cres;        // C*sresidual (PCR) or C*residual (plain)
    double* pCstep;      // P*Cstep, SMW mode only
    const double* resscale;
    const double* diag;
};

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// out = rhs - sub (sub == nullptr: out = rhs); partial max |resscale .* out|
__global__ __launch_bounds__(kBlock) void residual_init_kernel(int m, const double* __restrict__ rhs,
                                                               const double* __restrict__ sub,
                                                               const double* __restrict__ resscale,
                                                               double* __restrict__ out,
                                                               double* partial) {
    __shared__ double red[kBlock / 64 + 1];
    double mx = 0.0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < m; i += gridDim.x * kBlock) {
        const double r = sub ? rhs[i] - sub[i] : rhs[i];
        out[i] = r;
        mx = MaxOp::apply(mx, fabs(resscale ? resscale[i] * r : r));
    }
    mx = block_reduce<MaxOp>(mx, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = mx;
}

__global__ __launch_bounds__(kBlock) void cr_init_state_kernel(CrState* st, double tol, long long maxiter,
                                                               long long hist_cap, PartRef rsdot, int mode) {
    __shared__ double red[kBlock / 64 + 1];
    const double r = rsdot.p ? reduce_partials<SumOp>(rsdot, red) : 0.0;
    if (threadIdx.x == 0) {
        st->tol = tol;
        st->maxiter = maxiter;
        st->k_started = 0;
        st->k_finished = 0;
        st->cdot[0] = st->cdot[1] = 0.0;
        st->rps[0] = r;
        st->rps[1] = 0.0;
        st->resnorm = 0.0;
        st->iter = 0;
        st->errflag = 0;
        st->done = 0;
        st->hist_cap = hist_cap;
        st->diag_rps_old = st->diag_rps_new = 0.0;
        st->mode = mode;
        st->alpha_pending = 0.0;
        st->k_pending = -1;
    }
}

// The elements i0, i0 + stride, ... (kCrUnroll of them) of the control kernel's loop: the loads, from indices clamped to
// `last`, and the update with its stores, which skips the elements past `last`.
struct CtlGroup {
    double q[kCrUnroll], r[kCrUnroll], sr[kCrUnroll], d[kCrUnroll], sc[kCrUnroll], s[kCrUnroll], l[kCrUnroll];
};
template <int MODE>
__device__ __forceinline__ void ctl_load(const CrVecs& v, int lazy, long long i0, long long stride, long long last, CtlGroup& g) {
#pragma unroll
    for (int u = 0; u < kCrUnroll; u++) {
        const long long i = min(i0 + u * stride, last);
        g.q[u] = v.Cstep[i];
        g.r[u] = v.residual[i];
        if (MODE != kModePlain) g.sr[u] = v.sresidual[i];
        if (MODE == kModePcrDiag) g.d[u] = v.diag[i];
        if (MODE == kModePcrSmw) g.d[u] = v.pCstep[i];
        if (v.resscale) g.sc[u] = v.resscale[i];
        if (!lazy) { g.s[u] = v.step[i]; g.l[u] = v.lhs[i]; }
    }
}
template <int MODE>
__device__ __forceinline__ void ctl_update(const CrVecs& v, int lazy, double alpha, long long i0, long long stride, long long last,
                                           const CtlGroup& g, double& mx) {
#pragma unroll
    for (int u = 0; u < kCrUnroll; u++) {
        const long long i = i0 + u * stride;
        if (i > last) break;
        if (!lazy) v.lhs[i] = g.l[u] + alpha * g.s[u];
        const double rn = g.r[u] - alpha * g.q[u];
        v.residual[i] = rn;
        if (MODE == kModePcrDiag) v.sresidual[i] = g.sr[u] - alpha * (g.q[u] / g.d[u]);
        if (MODE == kModePcrSmw) v.sresidual[i] = g.sr[u] - alpha * g.d[u];
        mx = MaxOp::apply(mx, fabs(v.resscale ? g.sc[u] * rn : rn));
    }
}

// Loop head + residual update of iteration k = st->k_finished.  The solution update lhs += alpha*step
// is left to the direction kernel of the same iteration (alpha goes through st->alpha_pending); with
// lazy == 0 it is done here, as it was before the update was deferred.  host_done (single rank, mapped
// host memory): set together with st->done, so that the host stops enqueuing without waiting for the
// cycle's snapshot.
// EARLY: none of the vector loads depends on a loop scalar (the addresses come from the arguments), so the thread's
// first group of loads is issued before anything waits for one: the fields of CrState are read in one batch, then the
// pdot partials, the group and the residual-norm partials (every fifth iteration the rsdot partials too) are all in
// flight together, and the two reductions share their barriers.  Those barriers also keep the loads where they are:
// the `done` test comes after them.  All stores stay behind that test and the errflag decisions, in the order of the
// other form.  A launch that finds `done` set or leaves through an errflag has then loaded what it does not use: three
// launches of a solve, from buffers that are valid for the whole solve.  !EARLY (IPXK_CR_EARLY=0) is the order before:
// the scalars one after another, then the loads.  Same operations on the same values either way.
template <int MODE, bool EARLY>
__global__ __launch_bounds__(kBlock) void cr_control_update_kernel(
    CrState* st, CrVecs v, PartRef res0, PartRef res1, PartRef pdot_ref, PartRef rsdot_ref,
    double* res_next0, double* res_next1, double* hist, int lazy, int* host_done) {
    __shared__ double red[kBlock / 64 + 1];
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    const long long stride = (long long)gridDim.x * kBlock, last = v.m - 1;
    const long long first = blockIdx.x * kBlock + threadIdx.x;
    long long k;
    int errflag = -1;  // -1: continue
    double resnorm, alpha = 0.0;
    CtlGroup g0{};
    if (EARLY) {
        __shared__ double red2[kBlock / 64 + 1];
        const int done = st->done;
        k = st->k_finished;
        const long long maxiter = st->maxiter, hist_cap = st->hist_cap;
        const double tol = st->tol, cdot0 = st->cdot[0], cdot1 = st->cdot[1], rps0 = st->rps[0], rps1 = st->rps[1];
        resnorm = st->resnorm;
        double pp[kPartialsPerThread], pr[kPartialsPerThread], ps[kPartialsPerThread];
        load_partials(pdot_ref, pp);
        ctl_load<MODE>(v, lazy, first, stride, last, g0);
        const bool check5 = MODE != kModePlain && k > 0 && k % 5 == 0;
        const PartRef res_ref = (k & 1) ? res1 : res0;
        load_partials(res_ref, pr);
        double rsdot = 0.0;
        if (check5) {
            load_partials(rsdot_ref, ps);
            rsdot = block_reduce<SumOp>(fold_partials<SumOp>(rsdot_ref, ps), red);
        }
        double rn = fold_partials<MaxOp>(res_ref, pr), pdot = fold_partials<SumOp>(pdot_ref, pp);
        block_reduce2<MaxOp, SumOp>(rn, pdot, red, red2);
        if (done) return;
        if (check5) {
            // :195-206 monotonicity of residual'*P*residual over the last 5 iterations
            const long long c5 = k / 5;
            const double rps_old = ((c5 - 1) & 1) ? rps1 : rps0;
            if (rsdot >= rps_old) {
                errflag = 204;                                     // IPX_ERROR_cr_no_progress
                if (writer) { st->diag_rps_old = rps_old; st->diag_rps_new = rsdot; }
            } else if (writer) st->rps[c5 & 1] = rsdot;
        }
        if (errflag < 0) {
            resnorm = rn;
            if (writer && k < hist_cap) hist[k] = resnorm;
            const double cdot = (k & 1) ? cdot1 : cdot0;
            if (resnorm <= tol) errflag = 0;
            else if (k == maxiter) errflag = 201;                 // IPX_ERROR_cr_iter_limit
            else if (cdot <= 0.0) errflag = 202;                  // IPX_ERROR_cr_matrix_not_posdef
            else if (MODE != kModePlain && pdot <= 0.0) errflag = 203;  // IPX_ERROR_cr_precond_not_posdef
            else {
                alpha = cdot / pdot;
                if (!isfinite(alpha)) errflag = 205;              // IPX_ERROR_cr_inf_or_nan
            }
        }
    } else {
        if (st->done) return;
        k = st->k_finished;
        resnorm = st->resnorm;
        if (MODE != kModePlain && k > 0 && k % 5 == 0) {
            // :195-206 monotonicity of residual'*P*residual over the last 5 iterations
            const double rsdot = reduce_partials<SumOp>(rsdot_ref, red);
            const long long c5 = k / 5;
            if (rsdot >= st->rps[(c5 - 1) & 1]) {
                errflag = 204;                                     // IPX_ERROR_cr_no_progress
                if (writer) { st->diag_rps_old = st->rps[(c5 - 1) & 1]; st->diag_rps_new = rsdot; }
            } else if (writer) st->rps[c5 & 1] = rsdot;
        }
        if (errflag < 0) {
            resnorm = reduce_partials<MaxOp>((k & 1) ? res1 : res0, red);
            if (writer && k < st->hist_cap) hist[k] = resnorm;
            const double cdot = st->cdot[k & 1];
            if (resnorm <= st->tol) errflag = 0;
            else if (k == st->maxiter) errflag = 201;             // IPX_ERROR_cr_iter_limit
            else if (cdot <= 0.0) errflag = 202;                  // IPX_ERROR_cr_matrix_not_posdef
            else {
                const double pdot = reduce_partials<SumOp>(pdot_ref, red);
                if (MODE != kModePlain && pdot <= 0.0) errflag = 203;  // IPX_ERROR_cr_precond_not_posdef
                else {
                    alpha = cdot / pdot;
                    if (!isfinite(alpha)) errflag = 205;          // IPX_ERROR_cr_inf_or_nan
                }
            }
        }
    }
    if (errflag >= 0) {
        if (writer) {
            st->errflag = errflag;
            st->iter = k;
            st->resnorm = resnorm;
            st->done = 1;
            if (host_done) __hip_atomic_store(host_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        return;
    }

    // :173-175 / :72-73, kCrUnroll elements of the grid-stride loop at a time (see kCrUnroll)
    double mx = 0.0;
    long long i0 = first;
    if (EARLY) {
        ctl_update<MODE>(v, lazy, alpha, i0, stride, last, g0, mx);
        i0 += kCrUnroll * stride;
    }
    for (; i0 < v.m; i0 += kCrUnroll * stride) {
        CtlGroup g{};
        ctl_load<MODE>(v, lazy, i0, stride, last, g);
        ctl_update<MODE>(v, lazy, alpha, i0, stride, last, g, mx);
    }
    mx = block_reduce<MaxOp>(mx, red);
    if (threadIdx.x == 0) ((k & 1) ? res_next0 : res_next1)[blockIdx.x] = mx;
    if (writer) {
        st->k_started = k + 1;
        st->resnorm = resnorm;
        if (lazy) { st->alpha_pending = alpha; st->k_pending = k; }
    }
}

// one group of the direction kernel's loop, as CtlGroup; lhs is loaded where with_lhs says so, residual for a REFRESH
struct DirGroup {
    double p[kCrUnroll], q[kCrUnroll], s[kCrUnroll], cs[kCrUnroll], d[kCrUnroll], l[kCrUnroll], r[kCrUnroll];
};
template <int MODE, bool INIT, bool REFRESH>
__device__ __forceinline__ void dir_load(const CrVecs& v, const double* src, bool with_lhs, long long i0, long long stride,
                                         long long last, DirGroup& g) {
#pragma unroll
    for (int u = 0; u < kCrUnroll; u++) {
        const long long i = min(i0 + u * stride, last);
        g.p[u] = src[i];
        g.q[u] = v.Cres[i];
        if (!INIT) { g.s[u] = v.step[i]; g.cs[u] = v.Cstep[i]; }
        if (MODE == kModePcrDiag) g.d[u] = v.diag[i];
        if (!INIT && with_lhs) g.l[u] = v.lhs[i];
        if (REFRESH) g.r[u] = v.residual[i];
    }
}
template <int MODE, bool INIT, bool REFRESH>
__device__ __forceinline__ void dir_update(const CrVecs& v, bool owed, double alpha, double beta, long long i0, long long stride,
                                           long long last, DirGroup& g, double& acc, double& rs) {
#pragma unroll
    for (int u = 0; u < kCrUnroll; u++) {
        const long long i = i0 + u * stride;
        if (i > last) break;
        if (!INIT) {
            if (owed) v.lhs[i] = g.l[u] + alpha * g.s[u];
            g.p[u] = g.p[u] + beta * g.s[u];
            g.q[u] = g.q[u] + beta * g.cs[u];
        }
        v.step[i] = g.p[u];
        v.Cstep[i] = g.q[u];
        if (MODE == kModePcrDiag) acc += (g.q[u] / g.d[u]) * g.q[u];   // pdot of diagonal_precond.cc:152-154
        if (MODE == kModePlain) acc += g.q[u] * g.q[u];                // Dot(Cstep,Cstep), :66
        if (REFRESH) {                                                 // :187-194, as diag_apply_kernel (precond.hip)
            const double l = g.r[u] / g.d[u];
            v.sresidual[i] = l;                                        // (the old value went into step[i] above)
            rs += l * g.r[u];
        }
    }
}

// :180-184 / :78-81  new search direction; INIT: step = (s)residual, Cstep = C*(s)residual.
// An owed solution update (:173 / :72, lhs += alpha*step with the alpha of this iteration's control
// kernel) is paid first, with the step[i] that is loaded anyway and before it is overwritten.  The mark
// is not cleared here (other workgroups may still be reading it): the store of k_finished retires it.
// EARLY, as in the control kernel: CrState in one batch, the cdot partials and the thread's first group of loads in
// flight before the reduction's barriers, the `done` test after them.  Whether an update is owed is not known when the
// group is loaded, so lhs is loaded with it and only the store is conditional; in the order run_cr enqueues the
// kernels every direction kernel of the loop owes one, so nothing is read for nothing there.
// REFRESH (PcrDiag, the launches with (k + 1) % 5 == 0): the kernel also makes the refresh sresidual = residual ./ diag
// with the partials of residual'*sresidual, which is diag_apply_kernel's work on the same thread-to-element map: an
// element's old sresidual has gone into its new step before it is overwritten, a thread adds its products in ascending
// element order and block_reduce is the same, so with equal grids the partials are diag_apply_kernel's bit for bit.
// host_progress (single rank, mapped host memory): the number of finished iterations, for the host's pacing alone.
template <int MODE, bool INIT, bool EARLY, bool REFRESH>
__global__ __launch_bounds__(kBlock) void cr_direction_kernel(CrState* st, CrVecs v, PartRef cdot_ref,
                                                              double* pdot_partial, double* rsdot_partial,
                                                              long long* host_progress) {
    static_assert(!REFRESH || (MODE == kModePcrDiag && !INIT), "the fused refresh is the diagonal preconditioner's");
    __shared__ double red[kBlock / 64 + 1];
    const double* src = MODE == kModePlain ? v.residual : v.sresidual;
    const long long stride = (long long)gridDim.x * kBlock, last = v.m - 1;
    const long long first = blockIdx.x * kBlock + threadIdx.x;
    long long k;
    double cdotnew, beta, alpha;
    bool owed;
    DirGroup g0{};
    if (EARLY) {
        const int done = st->done;
        const long long k_started = st->k_started, k_pending = st->k_pending;
        const double cdot0 = st->cdot[0], cdot1 = st->cdot[1];
        alpha = st->alpha_pending;
        double pc[kPartialsPerThread];
        load_partials(cdot_ref, pc);
        dir_load<MODE, INIT, REFRESH>(v, src, true, first, stride, last, g0);
        cdotnew = block_reduce<SumOp>(fold_partials<SumOp>(cdot_ref, pc), red);
        if (done) return;
        k = INIT ? -1 : k_started - 1;
        beta = INIT ? 0.0 : cdotnew / ((k & 1) ? cdot1 : cdot0);
        owed = !INIT && k_pending == k;
    } else {
        if (st->done) return;
        k = INIT ? -1 : st->k_started - 1;
        cdotnew = reduce_partials<SumOp>(cdot_ref, red);
        beta = INIT ? 0.0 : cdotnew / st->cdot[k & 1];
        owed = !INIT && st->k_pending == k;
        alpha = st->alpha_pending;
    }
    double acc = 0.0;   // a thread adds its elements in ascending order, unrolled or not: the partials keep their bits
    double rs = 0.0;    // REFRESH: residual'*sresidual, likewise
    long long i0 = first;
    if (EARLY) {
        dir_update<MODE, INIT, REFRESH>(v, owed, alpha, beta, i0, stride, last, g0, acc, rs);
        i0 += kCrUnroll * stride;
    }
    for (; i0 < v.m; i0 += kCrUnroll * stride) {
        DirGroup g{};
        dir_load<MODE, INIT, REFRESH>(v, src, owed, i0, stride, last, g);
        dir_update<MODE, INIT, REFRESH>(v, owed, alpha, beta, i0, stride, last, g, acc, rs);
    }
    if (MODE != kModePcrSmw) {
        acc = block_reduce<SumOp>(acc, red);
        if (threadIdx.x == 0) pdot_partial[blockIdx.x] = acc;
    }
    if (REFRESH) {
        rs = block_reduce<SumOp>(rs, red);
        if (threadIdx.x == 0) rsdot_partial[blockIdx.x] = rs;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->cdot[(k + 1) & 1] = cdotnew;
        st->k_finished = k + 1;
        if (host_progress) __hip_atomic_store(host_progress, k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Pays a solution update that no direction kernel paid.  In the order run_cr enqueues the kernels every
// control kernel that marks an update is followed by the direction kernel of its iteration, and nothing in
// between can set `done`, so on every way out of the loop this finds nothing owed; it is enqueued once after
// the loop so that lhs does not depend on that order staying as it is.  Not gated on `done`; writes no state.
__global__ __launch_bounds__(kBlock) void cr_flush_update_kernel(const CrState* st, CrVecs v) {
    if (st->k_pending < 0 || st->k_pending != st->k_finished) return;
    const double alpha = st->alpha_pending;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < v.m; i += gridDim.x * kBlock) v.lhs[i] += alpha * v.step[i];
}

__global__ __launch_bounds__(kBlock) void finalize_scalar_kernel(PartRef ref, int op, double* out) {
    __shared__ double red[kBlock / 64 + 1];
    const double v = op == 1 ? reduce_partials<MaxOp>(ref, red)
                   : op == 2 ? reduce_partials<MinOp>(ref, red) : reduce_partials<SumOp>(ref, red);
    if (threadIdx.x == 0) *out = v;
}

// `done` at the end of a cycle, for the host (mapped pinned memory).
__global__ void snapshot_done_kernel(const CrState* st, int* host_slot) {
    __hip_atomic_store(host_slot, st->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// Partitioned solves: the ranks must leave the loop in the same cycle whatever happens (every cycle
// enqueues collectives), so what the host reads is the MAXIMUM over the ranks of (done, interrupt flag):
// this rank's pair goes into `flags`, an all-reduce follows, the second kernel hands the result to the host.
__global__ void cycle_flags_kernel(const CrState* st, double interrupt_flag, double* flags) {
    flags[0] = (double)st->done;
    flags[1] = interrupt_flag;
}
__global__ void snapshot_flags_kernel(const double* flags, int* host_done, int* host_interrupt) {
    __hip_atomic_store(host_interrupt, (int)flags[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(host_done, (int)flags[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
constexpr int kDoneRing = kWindow + 2;
constexpr int kDoneNow = 2 * kDoneRing;   // slot of h_cycle_done the control kernel sets with st->done (single rank)
// the progress word (64 bits: two slots, 8-byte aligned): the number of finished iterations, stored by the direction kernel
constexpr int kProgress = kDoneNow + 2;
static_assert(kProgress % 2 == 0 && kProgress + 2 <= 64, "the progress word lies inside h_cycle_done, aligned");

// IPXK_CR_PACE=cycles: single rank too enqueues cycles of 5 iterations and leaves by the cycles' snapshots (the driver
// before the progress word; A/B runs and the tests' reference)
static bool cr_pace_cycles() {
    static const bool setting = [] { const char* e = getenv("IPXK_CR_PACE"); return e && std::string(e) == "cycles"; }();
    return setting;
}

// IPXK_CR_AHEAD=<R>: iterations the host may run ahead of the progress word (A/B runs and tests)
static long long cr_ahead() {
    static const long long setting = [] { const char* e = getenv("IPXK_CR_AHEAD"); return e && atoi(e) > 0 ? atoi(e) : kAhead; }();
    return setting;
}

// IPXK_CR_REFRESH=0: the refresh of every fifth iteration stays a launch of its own (A/B runs and tests)
static bool cr_refresh() {
    static const bool setting = [] { const char* e = getenv("IPXK_CR_REFRESH"); return !e || atoi(e) != 0; }();
    return setting;
}

// IPXK_CR_LAZY=0: the control kernel updates lhs itself (the order before the update was deferred; A/B runs and tests)
static bool cr_lazy() {
    static const bool setting = [] { const char* e = getenv("IPXK_CR_LAZY"); return !e || atoi(e) != 0; }();
    return setting;
}

// IPXK_CR_EARLY=0: the two vector kernels fetch their scalars first and load afterwards (the order before the loads were
// issued first; A/B runs and tests)
static bool cr_early() {
    static const bool setting = [] { const char* e = getenv("IPXK_CR_EARLY"); return !e || atoi(e) != 0; }();
    return setting;
}

// IPXK_CR_GRID=<g>: at most g workgroups for the vector kernels of the CR loop, so that a small system gives a thread
// several elements and runs the later groups of kCrUnroll (tests).  Same operations per element; the partition of the
// partial sums follows g, so results are bitwise comparable only between runs with the same g.
static int cr_grid_cap() {
    static const int setting = [] { const char* e = getenv("IPXK_CR_GRID"); return e ? atoi(e) : 0; }();
    return setting;
}

static void ensure_comm_buffers(Context* c) {
    if (c->comm_scalars.size() < 64) c->comm_scalars.resize(64);
    if (c->comm_send.size() < (size_t)kNumPartialSlots) {
        c->comm_send.resize(kNumPartialSlots);
        IPXK_HIP(hipMemsetAsync(c->comm_send.get(), 0, sizeof(double) * kNumPartialSlots, c->stream));
    }
    const size_t need = (size_t)c->nranks * kNumPartialSlots;
    if (c->comm_gather.size() < need) c->comm_gather.resize(need);
}

// Scalars of the CR loop across ranks.  Single rank: a consumer kernel reduces the producer's
// per-workgroup partials itself.  Partitioned: one finalize launch turns this rank's partials into
// scalars, one all-gather of the (tiny) scalar table makes every rank's values visible, and the
// consumer reduces over ranks in rank order -- every rank obtains bitwise identical scalars and
// therefore takes identical decisions.
struct Pub {
    Context* c;
    bool multi;
    // row partition only: with partitioned columns every rank computes the same scalars itself
    explicit Pub(Context* ctx) : c(ctx), multi(comm_rows(ctx)) { if (multi) ensure_comm_buffers(ctx); }
    PartRef ref(int slot, int nparts) const {
        if (!multi) return PartRef{c->part(slot), nparts, 1};
        return PartRef{c->comm_gather.get() + slot, c->nranks, kNumPartialSlots};
    }
    // op: 0 sum, 1 max, 2 min
    void publish(int slot0, int n0, int op0, int slot1 = -1, int n1 = 0, int op1 = 0) const {
        if (!multi) return;
        hipLaunchKernelGGL(finalize_scalar_kernel, dim3(1), dim3(kBlock), 0, c->stream,
                           PartRef{c->part(slot0), n0, 1}, op0, c->comm_send.get() + slot0);
        if (slot1 >= 0)
            hipLaunchKernelGGL(finalize_scalar_kernel, dim3(1), dim3(kBlock), 0, c->stream,
                               PartRef{c->part(slot1), n1, 1}, op1, c->comm_send.get() + slot1);
        comm_allgather(c, c->comm_send.get(), c->comm_gather.get(), kNumPartialSlots);
    }
};

PartRef publish_scalar(Context* c, int slot, int count, int op) {
    const Pub pub(c);
    pub.publish(slot, count, op);
    return pub.ref(slot, count);
}

// finalize this rank's partials of `slot` and reduce the scalar over the ranks (op: 0 sum, 1 max, 2 min)
PartRef allreduce_scalar(Context* c, int slot, int count, int op) {
    ensure_comm_buffers(c);
    double* out = c->comm_scalars.get() + 62;
    hipLaunchKernelGGL(finalize_scalar_kernel, dim3(1), dim3(kBlock), 0, c->stream,
                       PartRef{c->part(slot), count, 1}, op, out);
    if (op == 0) comm_allreduce_sum(c, out, 1);
    else if (op == 1) comm_allreduce_max(c, out, 1);
    else comm_allreduce_min(c, out, 1);
    return PartRef{out, 1, 1};
}

double reduce_partials_host(Context* c, int slot, int count, bool is_max) {
    ensure_comm_buffers(c);
    double* out = c->comm_scalars.get() + 63;
    hipLaunchKernelGGL(finalize_scalar_kernel, dim3(1), dim3(kBlock), 0, c->stream,
                       PartRef{c->part(slot), count, 1}, is_max ? 1 : 0, out);
    if (comm_rows(c)) {   // with partitioned columns the vectors, hence the scalar, are replicated
        if (is_max) comm_allreduce_max(c, out, 1);
        else comm_allreduce_sum(c, out, 1);
    }
    double v = 0.0;
    IPXK_HIP(hipMemcpyAsync(&v, out, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    IPXK_HIP(hipStreamSynchronize(c->stream));
    return v;
}

static void ensure_workspaces(Context* c) {
    const size_t m = (size_t)(c->m > 0 ? c->m : 1);
    if (c->v_residual.size() != m) {
        c->v_residual.resize(m); c->v_sresidual.resize(m); c->v_step.resize(m);
        c->v_Cstep.resize(m); c->v_Cres.resize(m); c->v_pCstep.resize(m);
    }
    c->ensure_partials();
    if (c->state.size() == 0) c->state.resize(1);
    if (!c->h_state) IPXK_HIP(hipHostMalloc(reinterpret_cast<void**>(&c->h_state), sizeof(CrState)));
    if (!c->ev_a) { IPXK_HIP(hipEventCreate(&c->ev_a)); IPXK_HIP(hipEventCreate(&c->ev_b)); }
    if (!c->h_cycle_done) {
        IPXK_HIP(hipHostMalloc(reinterpret_cast<void**>(&c->h_cycle_done), 64 * sizeof(int), hipHostMallocMapped));
        IPXK_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->d_cycle_done), c->h_cycle_done, 0));
    }
    while ((int)c->ev_window.size() < kWindow + 1) {
        hipEvent_t e;
        IPXK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->ev_window.push_back(e);
    }
}

// Operator / preconditioner hooks of one solve.
struct CrOps {
    int mode;
    // lhs = C rhs, dot partials into part(kPartCdot); returns their count
    int (*applyC)(Context*, const double* rhs, double* lhs, const int* done);
};

static int applyC_normal(Context* c, const double* rhs, double* lhs, const int* done) {
    int np = 0;
    time_mark(c, kTimeOp, true);
    normal_apply_dev(c, c->W, rhs, lhs, &np, done);
    time_mark(c, kTimeOp, false);
    return np;
}
static int applyC_split(Context* c, const double* rhs, double* lhs, const int* done) {
    return split_apply_dev(c, rhs, lhs, done);
}

// Single rank, paced by the progress word: waits until `need` iterations have finished or the control kernel has
// reported `done`.  The first look costs two loads from host memory; a host that is the slower side never gets further.
// Otherwise the thread yields between looks and asks the stream from time to time: while it holds work the device goes
// on and one of the two words must move, so the wait ends; an error is thrown; an empty stream that has moved neither
// word returns false (no iteration that is not `done` finishes without storing its number, so that is a broken queue).
// hipStreamQuery is not free for the device -- the runtime learns the state of a stream of kernels by putting a marker
// with a completion signal behind them, the barrier packet this driver exists to avoid -- so the first question comes
// after kQueryAfter of waiting (ten iterations at C3, where one takes 0.19 ms) and the later ones at doubling intervals.
static bool wait_for_progress(Context* c, hipStream_t s, long long need) {
    using clock = std::chrono::steady_clock;
    constexpr std::chrono::microseconds kQueryAfter(2000), kQueryMax(128000);
    const volatile int* done_now = c->h_cycle_done + kDoneNow;
    const volatile long long* progress = reinterpret_cast<const volatile long long*>(c->h_cycle_done + kProgress);
    if (*done_now || *progress >= need) return true;
    clock::time_point asked = clock::now();
    std::chrono::microseconds interval = kQueryAfter;
    for (unsigned looks = 1;; looks++) {
        std::this_thread::yield();
        if (*done_now || *progress >= need) return true;
        if (looks % 64 == 0 && clock::now() - asked >= interval) {
            const hipError_t e = hipStreamQuery(s);
            if (e != hipErrorNotReady) {
                IPXK_HIP(e);
                return *done_now || *progress >= need;     // everything enqueued has finished: the words are final
            }
            asked = clock::now();
            interval = std::min(interval * 2, kQueryMax);
        }
    }
}

template <int MODE>
static CrResult run_cr(Context* c, const CrOps& ops, const double* rhs, double tol,
                       const double* resscale, ipxint maxiter, double* lhs, bool lhs_is_zero,
                       ipxk_interrupt_fn interrupt, void* user, double* hist_host, ipxint hist_cap,
                       ipxk_times* times) {
    ensure_workspaces(c);
    time_start(c, times);
    hipStream_t s = c->stream;
    const int m = (int)c->m;
    if (maxiter < 0) maxiter = (comm_active(c) ? c->m_global : c->m) + 100;   // :114-115
    if (hist_cap < 0) hist_cap = 0;
    if (!hist_host) hist_cap = 0;
    if (c->hist.size() < (size_t)hist_cap + 1) c->hist.resize((size_t)hist_cap + 1);
    CrState* st = c->state.get();
    int* done = &st->done;
    const int g = cr_grid_cap() > 0 ? std::min(vec_grid(m), cr_grid_cap()) : vec_grid(m);
    const Pub pub(c);
    for (int i = 0; i < kProgress + 2; i++) c->h_cycle_done[i] = 0;   // previous solve is synchronized
    const bool multi = comm_active(c);
    const int lazy = cr_lazy() ? 1 : 0;
    const bool early = cr_early() && m > 0;   // (the early loads read element 0 of every vector)
    const auto control = early ? cr_control_update_kernel<MODE, true> : cr_control_update_kernel<MODE, false>;
    const auto direction0 = early ? cr_direction_kernel<MODE, true, true, false> : cr_direction_kernel<MODE, true, false, false>;
    const auto direction = early ? cr_direction_kernel<MODE, false, true, false> : cr_direction_kernel<MODE, false, false, false>;
    // the direction kernel that also makes the refresh of every fifth iteration (PcrDiag, single rank)
    auto direction5 = direction;
    bool fused_refresh = false;
    if constexpr (MODE == kModePcrDiag) {
        fused_refresh = !multi && cr_refresh();
        direction5 = early ? cr_direction_kernel<MODE, false, true, true> : cr_direction_kernel<MODE, false, false, true>;
    }
    // partitioned: every rank enqueues the same collectives, so the ranks leave by the agreed snapshots alone
    int* done_now = multi ? nullptr : c->d_cycle_done + kDoneNow;
    long long* progress = multi ? nullptr : reinterpret_cast<long long*>(c->d_cycle_done + kProgress);
    if (multi) ensure_comm_buffers(c);
    // what this run enqueues (ipxk_cr_loop_stats): iterations, launches of this file's kernels and of the diagonal
    // preconditioner's (the operator's and the dense-column preconditioner's are their own routines'), snapshots, events
    long long* stats = c->cr_loop_stats;
    stats[0] = stats[1] = stats[2] = stats[3] = 0;

    CrVecs v;
    v.m = m; v.lhs = lhs; v.residual = c->v_residual.get(); v.sresidual = c->v_sresidual.get();
    v.step = c->v_step.get(); v.Cstep = c->v_Cstep.get(); v.Cres = c->v_Cres.get();
    v.pCstep = c->v_pCstep.get(); v.resscale = resscale; v.diag = c->reord.in_use ? c->reord.diagonal.get() : c->diagonal.get();

    IPXK_HIP(hipEventRecord(c->ev_a, s));

    // ---- initialisation, :117-126 / :33-41 ----
    if (lhs_is_zero) {
        hipLaunchKernelGGL(residual_init_kernel, dim3(g), dim3(kBlock), 0, s, m, rhs,
                           (const double*)nullptr, resscale, v.residual, c->part(kPartRes0));
    } else {
        ops.applyC(c, lhs, v.Cres, nullptr);
        hipLaunchKernelGGL(residual_init_kernel, dim3(g), dim3(kBlock), 0, s, m, rhs,
                           (const double*)v.Cres, resscale, v.residual, c->part(kPartRes0));
    }
    stats[1]++;
    // the preconditioner's partials follow the grid of this loop (IPXK_CR_GRID), so that the refresh inside the
    // direction kernel and the one in a launch of its own give the same partials under every cap
    int nrsdot = 0;
    if (MODE != kModePlain) nrsdot = diag_apply_dev(c, v.residual, v.sresidual, kPartRsdot, nullptr, g);
    if (MODE == kModePcrDiag) stats[1]++;
    if (MODE != kModePlain) pub.publish(kPartRes0, g, 1, kPartRsdot, nrsdot, 0);
    else pub.publish(kPartRes0, g, 1);
    const PartRef res0 = pub.ref(kPartRes0, g), res1 = pub.ref(kPartRes1, g);
    const PartRef rsdot = MODE != kModePlain ? pub.ref(kPartRsdot, nrsdot) : PartRef{nullptr, 0, 1};
    hipLaunchKernelGGL(cr_init_state_kernel, dim3(1), dim3(kBlock), 0, s, st, tol, (long long)maxiter,
                       (long long)hist_cap, rsdot, (int)MODE);
    const double* csrc = MODE == kModePlain ? v.residual : v.sresidual;
    int ncdot = ops.applyC(c, csrc, v.Cres, nullptr);
    pub.publish(kPartCdot, ncdot, 0);
    hipLaunchKernelGGL(direction0, dim3(g), dim3(kBlock), 0, s, st, v,
                       pub.ref(kPartCdot, ncdot), c->part(kPartPdot), (double*)nullptr, progress);
    stats[1] += 2;
    int npdot = g;
    if (MODE == kModePcrSmw) npdot = diag_apply_dev(c, v.Cstep, v.pCstep, kPartPdot, nullptr, g);
    pub.publish(kPartPdot, npdot, 0);
    const PartRef pdot_ref = pub.ref(kPartPdot, npdot);

    // iteration k, for both drivers
    const auto enqueue_iteration = [&](long long k) {
        const bool refresh = MODE != kModePlain && (k + 1) % 5 == 0;   // :187-194
        hipLaunchKernelGGL(control, dim3(g), dim3(kBlock), 0, s, st, v,
                           res0, res1, pdot_ref, rsdot, c->part(kPartRes0), c->part(kPartRes1),
                           c->hist.get(), lazy, done_now);
        ncdot = ops.applyC(c, csrc, v.Cres, done);
        // the control kernel of iteration k wrote the residual-norm partials of parity (k+1)&1
        pub.publish(kPartCdot, ncdot, 0, ((k + 1) & 1) ? kPartRes1 : kPartRes0, g, 1);
        hipLaunchKernelGGL(refresh && fused_refresh ? direction5 : direction, dim3(g), dim3(kBlock), 0, s, st, v,
                           pub.ref(kPartCdot, ncdot), c->part(kPartPdot), c->part(kPartRsdot), progress);
        stats[0]++;
        stats[1] += 2;
        if (MODE == kModePcrSmw) diag_apply_dev(c, v.Cstep, v.pCstep, kPartPdot, done, g);
        if (refresh && !fused_refresh) {
            diag_apply_dev(c, v.residual, v.sresidual, kPartRsdot, done, g);
            if (MODE == kModePcrDiag) stats[1]++;
        }
        if (refresh) pub.publish(kPartPdot, npdot, 0, kPartRsdot, nrsdot, 0);
        else pub.publish(kPartPdot, npdot, 0);
    };

    // ---- main loop ----
    // Control::InterruptCheck (:209 / :84) is polled once per 5 iterations, not before the first five (a system
    // that needs no iteration returns its result whatever the callback says).  Single rank: a nonzero flag ends the
    // loop at once.  Partitioned: the flag travels with the cycle's `done` snapshot through one all-reduce (max), so
    // every rank leaves in the same cycle, kWindow cycles later.
    ipxint interrupt_flag = 0, my_interrupt = 0;
    bool agreed_done = false, tail = false, stalled = false;
    if (!multi && !cr_pace_cycles()) {
        // paced by the progress word: iteration k is enqueued once iteration k - R has finished, and never after the
        // control kernel has reported `done` -- at most iterations 0 .. K + R when iteration K is the final one
        const long long R = cr_ahead();
        for (long long k = 0; k <= maxiter; k++) {
            if (!wait_for_progress(c, s, k - R)) { stalled = true; break; }
            if (*(volatile int*)(c->h_cycle_done + kDoneNow)) break;
            if (interrupt && k > 0 && k % 5 == 0) {
                my_interrupt = interrupt(user);
                if (my_interrupt != 0) { interrupt_flag = my_interrupt; break; }
            }
            enqueue_iteration(k);
        }
    } else {
        // cycles of 5 iterations.  Single rank (IPXK_CR_PACE=cycles): once the control kernel has reported `done`
        // (kDoneNow) everything enqueued from then on would return at once, so the iterations are no longer enqueued;
        // the cycles' snapshots and events still are, and the loop is left through the snapshot of the cycle kWindow back.
        for (long long cycle = 0;; cycle++) {
            const long long k0 = cycle * 5;
            if (k0 > maxiter) break;
            if (cycle >= kWindow) {
                const long long cw = cycle - kWindow;
                IPXK_HIP(hipEventSynchronize(c->ev_window[cw % (kWindow + 1)]));
                if (*(volatile int*)(c->h_cycle_done + cw % kDoneRing)) { agreed_done = true; break; }
                if (multi) {
                    const int agreed = *(volatile int*)(c->h_cycle_done + kDoneRing + cw % kDoneRing);
                    if (agreed != 0) { interrupt_flag = agreed; break; }
                }
            }
            if (interrupt && cycle > 0) {
                my_interrupt = interrupt(user);
                if (!multi && my_interrupt != 0) { interrupt_flag = my_interrupt; break; }
            }
            for (long long k = k0; k < k0 + 5 && k <= maxiter; k++) {
                if (done_now && *(volatile int*)(c->h_cycle_done + kDoneNow)) tail = true;
                if (tail) break;
                enqueue_iteration(k);
            }
            if (multi) {
                double* flags = c->comm_scalars.get() + 56;
                hipLaunchKernelGGL(cycle_flags_kernel, dim3(1), dim3(1), 0, s, st, (double)my_interrupt, flags);
                comm_allreduce_max(c, flags, 2);
                hipLaunchKernelGGL(snapshot_flags_kernel, dim3(1), dim3(1), 0, s, flags, c->d_cycle_done + cycle % kDoneRing,
                                   c->d_cycle_done + kDoneRing + cycle % kDoneRing);
                stats[1] += 2;
            } else {
                hipLaunchKernelGGL(snapshot_done_kernel, dim3(1), dim3(1), 0, s, st, c->d_cycle_done + cycle % kDoneRing);
                stats[1]++;
            }
            stats[2]++;
            IPXK_HIP(hipEventRecord(c->ev_window[cycle % (kWindow + 1)], s));
            stats[3]++;
        }
    }
    if (lazy) {
        hipLaunchKernelGGL(cr_flush_update_kernel, dim3(g), dim3(kBlock), 0, s, st, v);
        stats[1]++;
    }
    IPXK_HIP(hipEventRecord(c->ev_b, s));
    IPXK_HIP(hipMemcpyAsync(c->h_state, st, sizeof(CrState), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
    IPXK_HIP(hipGetLastError());
    comm_check(c);

    // the ranks of a partitioned solve take identical decisions (identical scalars); if one of them saw the
    // others finish without finishing itself, the replicas have diverged
    if (multi && agreed_done && !c->h_state->done)
        throw Error(IPXK_E_HIP, "ranks of a partitioned solve diverged (another rank finished the CR loop, this one did not)");
    if (stalled && !c->h_state->done)
        throw Error(IPXK_E_HIP, "the CR loop's queue ran empty with iterations outstanding and the run not finished");
    CrResult res;
    if (c->h_state->done) {
        res.iter = c->h_state->iter;
        res.errflag = c->h_state->errflag;
    } else {
        // interrupted: the iterate of the last finished iteration is in lhs
        res.iter = c->h_state->k_finished;
        res.errflag = interrupt_flag;
    }
    if (hist_cap > 0) {
        long long nh = c->h_state->done && c->h_state->errflag != 204 ? res.iter + 1 : res.iter;
        if (!c->h_state->done) nh = c->h_state->k_started;
        if (nh > hist_cap) nh = hist_cap;
        for (long long i = nh; i < hist_cap; i++) hist_host[i] = std::nan("");
        if (nh > 0) {
            c->hist.download(hist_host, (size_t)nh, s);
            IPXK_HIP(hipStreamSynchronize(s));
        }
    }
    if (times) {
        float ms = 0.f;
        IPXK_HIP(hipEventElapsedTime(&ms, c->ev_a, c->ev_b));
        times->cr = ms * 1e-3;
        time_collect(c, times);
    }
    return res;
}

// infinity norm of a device vector (partials + host-side finish; diagnostics only)
__global__ __launch_bounds__(kBlock) void infnorm_partial_kernel(int m, const double* __restrict__ x, double* partial) {
    __shared__ double red[kBlock / 64 + 1];
    double mx = 0.0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < m; i += gridDim.x * kBlock) mx = MaxOp::apply(mx, fabs(x[i]));
    mx = block_reduce<MaxOp>(mx, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = mx;
}

void cr_diagnostics_dev(Context* c, ipxk_cr_diag* out) {
    *out = ipxk_cr_diag{};
    IPXK_REQUIRE(c->h_state != nullptr && c->state.size() > 0, "no CR run on this context yet");
    const CrState& st = *c->h_state;            // copied back at the end of the run
    out->errflag = st.done ? st.errflag : 0;
    out->iter = st.done ? st.iter : st.k_finished;
    out->maxiter = st.maxiter;
    out->resnorm = st.resnorm;
    out->tol = st.tol;
    out->cdot = st.cdot[out->iter & 1];
    out->rps_old = st.diag_rps_old;
    out->rps_new = st.diag_rps_new;
    if (st.done && st.errflag == 202) {         // the vectors of the run are still in the workspaces
        const int m = (int)c->m, g = vec_grid(m);
        auto norm = [&](const double* v) {
            hipLaunchKernelGGL(infnorm_partial_kernel, dim3(g), dim3(kBlock), 0, c->stream, m, v, c->part(kPartScratch));
            return reduce_partials_host(c, kPartScratch, g, true);
        };
        out->infnorm_residual = norm(c->v_residual.get());
        if (st.mode != kModePlain) out->infnorm_sresidual = norm(c->v_sresidual.get());
    }
}

void cr_loop_stats_dev(const Context* c, ipxint out[4]) {
    for (int i = 0; i < 4; i++) out[i] = (ipxint)c->cr_loop_stats[i];
}

CrResult pcr_solve_dev(Context* c, const double* rhs, double tol, const double* resscale,
                       ipxint maxiter, double* lhs, bool lhs_is_zero, ipxk_interrupt_fn interrupt,
                       void* user, double* hist_host, ipxint hist_cap, ipxk_times* times) {
    IPXK_REQUIRE(c->normal_prepared, "NormalMatrix not prepared");
    IPXK_REQUIRE(c->diag_factorized, "DiagonalPrecond not factorized");
    CrOps ops{c->kdense > 0 ? kModePcrSmw : kModePcrDiag, applyC_normal};
    if (c->kdense > 0)
        return run_cr<kModePcrSmw>(c, ops, rhs, tol, resscale, maxiter, lhs, lhs_is_zero, interrupt,
                                   user, hist_host, hist_cap, times);
    return run_cr<kModePcrDiag>(c, ops, rhs, tol, resscale, maxiter, lhs, lhs_is_zero, interrupt, user,
                                hist_host, hist_cap, times);
}

CrResult cr_solve_dev(Context* c, const double* rhs, double tol, const double* resscale,
                      ipxint maxiter, double* lhs, bool lhs_is_zero, ipxk_interrupt_fn interrupt,
                      void* user, double* hist_host, ipxint hist_cap, ipxk_times* times) {
    IPXK_REQUIRE(c->split != nullptr, "SplittedNormalMatrix not prepared");
    split_check_partition(c);
    CrOps ops{kModePlain, applyC_split};
    return run_cr<kModePlain>(c, ops, rhs, tol, resscale, maxiter, lhs, lhs_is_zero, interrupt, user,
                              hist_host, hist_cap, times);
}

}  // namespace ipxk
