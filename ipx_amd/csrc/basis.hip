// The basis of the exchange loops on the device: what Maxvolume (maxvolume.hip, both variants) and the starting basis
// (starting_basis.hip) share of the reference's ipx::Basis (src/basis.cc).
//   * The eta file.  The factorization is not updated in place: the factors of the last refactorized basis B0 stay fixed and every
//     exchange appends a product-form eta, B = B0 E_1 ... E_k with E_t = I + (eta_t - e_p) e_p', eta_t the tableau column of the
//     entering variable (EtaFile; as dense rows or as compact lists, and when to refactorize: see the comment at its methods).
//     A file that Maxvolume leaves behind the resident factors is applied by trisolve.hip through maxvol_apply_etas.
//   * DeviceBasis, one per call of a driver: FTRAN of the entering column and BTRAN of the leaving position (the two sweep pairs of
//     solve_dense_dev plus the etas), Basis::Factorize (:116-156), Basis::ExchangeIfStable (:286-321) with the ladder of the LU pivot
//     tolerance (Basis::TightenLuPivotTol, :490-503), the host mirrors of basis and status, and the refactorization of a full file.
// The drivers keep their pivot searches, their exchange kernels and their logs.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cmath>
#include <vector>

#include "context.hpp"
#include "trisolve.hpp"

namespace ipxk {

namespace {

constexpr int kEtaThreads = 1024;

using Scalars = MvScalars;     // the scalars of one step (internal.hpp)

// ---- the small kernels of an exchange: the entering column, the unit vector of the leaving position, the pivot from the row ----
__global__ void mv_scatter_column_kernel(int n, const Scalars* S, const int* __restrict__ Ap, const int* __restrict__ Ai,
                                         const double* __restrict__ Ax, double* __restrict__ rhs) {
    const int j = S->jn;
    if (j >= n) { if (blockIdx.x == 0 && threadIdx.x == 0) rhs[j - n] = 1.0; return; }
    for (int q = Ap[j] + blockIdx.x * blockDim.x + threadIdx.x; q < Ap[j + 1]; q += gridDim.x * blockDim.x) rhs[Ai[q]] = Ax[q];
}
__global__ void mv_unit_kernel(int m, const Scalars* S, double* v) {
    IPXK_GRID_STRIDE(p, m) v[p] = (int)p == S->pmax ? 1.0 : 0.0;
}
// the pivot from the row: btran' a_jn (one workgroup)
__global__ __launch_bounds__(kBlock) void mvs_pivot_row_kernel(int n, const int* __restrict__ Ap, const int* __restrict__ Ai,
                                                               const double* __restrict__ Ax, const double* __restrict__ btran, Scalars* S) {
    __shared__ double red[kBlock / 64];
    const int j = S->jn;
    double sum = 0.0;
    if (j >= n) { if (threadIdx.x == 0) S->pivot_row = btran[j - n]; return; }
    // (sequential order of the column's entries for few entries; a fixed tree over the threads otherwise)
    for (int q = Ap[j] + threadIdx.x; q < Ap[j + 1]; q += kBlock) sum += Ax[q] * btran[Ai[q]];
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) { double t = 0.0; for (int k = 0; k < kBlock / 64; k++) t += red[k]; S->pivot_row = t; }
}

// ---- the eta file ---------------------------------------------------------------------------------------------------------
// the etas, B^{-1} direction, oldest first: v_p <- v_p / piv; v_i <- v_i - eta_i v_p
__global__ __launch_bounds__(kEtaThreads) void mv_eta_ftran_kernel(int K, const int* __restrict__ ptr, const int* __restrict__ pos,
                                                                   const double* __restrict__ piv, const int* __restrict__ idx,
                                                                   const double* __restrict__ val, double* v) {
    __shared__ double s_vp;
    for (int t = 0; t < K; t++) {
        if (threadIdx.x == 0) { s_vp = v[pos[t]] / piv[t]; v[pos[t]] = s_vp; }
        __syncthreads();
        const double vp = s_vp;
        for (int e = ptr[t] + threadIdx.x; e < ptr[t + 1]; e += kEtaThreads) v[idx[e]] -= val[e] * vp;
        __syncthreads();
    }
}
// transposed direction, newest first: v_p <- (v_p - sum_i eta_i v_i) / piv
__global__ __launch_bounds__(kEtaThreads) void mv_eta_btran_kernel(int K, const int* __restrict__ ptr, const int* __restrict__ pos,
                                                                   const double* __restrict__ piv, const int* __restrict__ idx,
                                                                   const double* __restrict__ val, double* v) {
    __shared__ double red[kEtaThreads / 64];
    for (int t = K - 1; t >= 0; t--) {
        double sum = 0.0;
        for (int e = ptr[t] + threadIdx.x; e < ptr[t + 1]; e += kEtaThreads) sum += val[e] * v[idx[e]];
        sum = wave_sum(sum);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            double tot = 0.0;
            for (int k = 0; k < kEtaThreads / 64; k++) tot += red[k];
            v[pos[t]] = (v[pos[t]] - tot) / piv[t];
        }
        __syncthreads();
    }
}
// ---- the etas as DENSE vectors (round 5) -------------------------------------------------------------------------------------
// The two kernels above walk the etas one after the other -- 6.5 us per eta of 8000 entries, 0.65 ms per application with 100 of
// them, three applications per exchange: a third of Maxvolume's kernel time on the IPM's bases of a 24 000-row LP, whose tableau
// columns fill a third of the vector.  Stored as rows of a dense K x m matrix E (row s = eta s, 0 at its own pivot position), the
// same product form splits into a K x K triangular system for the multipliers and ONE pass over E:
//   forward:  alpha_t piv_t = base_t - sum_{prev(t) < s < t} E[s][pos_t] alpha_s,  base_t = alpha_prev(t) if position pos_t was
//             replaced before (prev(t) = the last such exchange), else v[pos_t];  then
//             v[i] = (alpha_last(i) or v[i]) - sum_{s > last(i)} E[s][i] alpha_s          (last(i): the last exchange at position i)
//   backward: d_t = E[t] . v;  w_t piv_t = cur_t - d_t - sum_{s > t, prev(s) <= t} E[t][pos_s] (w_s - v[pos_s]),  cur_t = w_next(t)
//             if the position is replaced again later, else v[pos_t];  then v[pos_t] = w_t for the first exchange of each position.
// The sums of the forward direction run in the order of the sequential kernel (s ascending, every product rounded before it is
// subtracted, zeros skipped): the same result bit for bit.  The triangular systems are solved by one workgroup, a barrier per
// eta (K <= 1024); T[t][s] = E[s][pos_t] (s < t) is kept both ways round so that either direction reads it contiguously.
constexpr int kEtaDenseMax = 1024;
__global__ void mv_eta_dense_append_kernel(int m, int K, int cap, const Scalars* S, const double* __restrict__ lhs, double* __restrict__ E,
                                           int* pos, double* piv, int* prev, int* next, int* last, double* __restrict__ T, double* __restrict__ Tt) {
    const int pmax = S->pmax;
    IPXK_GRID_STRIDE(p, m) E[(size_t)K * m + p] = (int)p == pmax ? 0.0 : lhs[p];
    IPXK_GRID_STRIDE(t, K) {                         // the older etas at the new pivot position
        const double e = E[(size_t)t * m + pmax];
        T[(size_t)K * cap + t] = e;
        Tt[(size_t)t * cap + K] = e;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        pos[K] = pmax;
        piv[K] = lhs[pmax];
        const int pr = last[pmax];
        prev[K] = pr;
        next[K] = -1;
        if (pr >= 0) next[pr] = K;
        last[pmax] = K;
    }
}
// (Blocked since the end of round 5: the 64 etas of a block are solved by ONE wavefront -- the multiplier of a step goes to the later lanes
// by a lane read, no barrier -- and the threads of the later blocks then subtract the block's 64 products in the same order from LDS: one
// workgroup barrier per 64 etas instead of two per eta.  Every r_t still receives its products in the order of the etas: the same bits.)
__global__ __launch_bounds__(kEtaDenseMax) void mv_eta_dense_ftran_solve_kernel(int K, int cap, const double* __restrict__ v, const int* __restrict__ pos,
                                                                               const double* __restrict__ piv, const int* __restrict__ prev,
                                                                               const double* __restrict__ Tt, double* __restrict__ alpha) {
    __shared__ double s_a[2][64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int pr = t < K ? prev[t] : -1;
    double r = (t < K && pr < 0) ? v[pos[t]] : 0.0;
    const double pv = t < K ? piv[t] : 1.0;
    for (int b0 = 0, blk = 0; b0 < K; b0 += 64, blk++) {
        const int b1 = min(b0 + 64, K);
        double* sa = s_a[blk & 1];
        // (the entries of T a thread needs for 16 steps are fetched together, ahead of the steps: a dependent load per step was most of a step)
        constexpr int CH = 16;
        if (wave == blk) {
            for (int s0 = b0; s0 < b1; s0 += CH) {
                double e[CH];
#pragma unroll
                for (int q = 0; q < CH; q++) e[q] = (s0 + q < b1 && t > s0 + q && t < K) ? Tt[(size_t)(s0 + q) * cap + t] : 0.0;
#pragma unroll
                for (int q = 0; q < CH; q++) {
                    const int s = s0 + q;
                    if (s < b1) {                                       // wave-uniform
                        const double mine = r / pv;                     // (only lane s - b0's value is used)
                        const int hi = __builtin_amdgcn_readlane(__double2hiint(mine), s - b0), lo = __builtin_amdgcn_readlane(__double2loint(mine), s - b0);
                        const double a = __hiloint2double(hi, lo);
                        if (t == s) { alpha[s] = a; sa[s - b0] = a; }
                        if (t > s && t < K) {
                            if (s == pr) r = a;
                            else if (s > pr && e[q] != 0.0) r -= e[q] * a;
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (wave > blk && t < K) {
            for (int s0 = b0; s0 < b1; s0 += CH) {
                double e[CH];
#pragma unroll
                for (int q = 0; q < CH; q++) e[q] = s0 + q < b1 ? Tt[(size_t)(s0 + q) * cap + t] : 0.0;
#pragma unroll
                for (int q = 0; q < CH; q++) {
                    const int s = s0 + q;
                    if (s < b1) {
                        const double a = sa[s - b0];
                        if (s == pr) r = a;
                        else if (s > pr && e[q] != 0.0) r -= e[q] * a;
                    }
                }
            }
        }
        // (the other buffer is written next, after everybody has passed this block's barrier: nobody still reads it)
    }
}
__global__ __launch_bounds__(kBlock) void mv_eta_dense_ftran_apply_kernel(int m, int K, const double* __restrict__ E, const double* __restrict__ alpha,
                                                                         const int* __restrict__ last, double* __restrict__ v) {
    __shared__ double sa[kEtaDenseMax];
    for (int t = threadIdx.x; t < K; t += kBlock) sa[t] = alpha[t];
    __syncthreads();
    IPXK_GRID_STRIDE(i, m) {
        const int l = last[i];
        double x = l >= 0 ? sa[l] : v[i];
        // eight entries of the column in flight at a time; the products are still subtracted one after the other in the order of the etas
        // (a thread walked its column one dependent load at a time before: 82 us per application with 400 etas of 24 000 entries)
        int s = l + 1;
        for (; s + 8 <= K; s += 8) {
            double e[8];
#pragma unroll
            for (int q = 0; q < 8; q++) e[q] = E[(size_t)(s + q) * m + i];
#pragma unroll
            for (int q = 0; q < 8; q++)
                if (e[q] != 0.0) x -= e[q] * sa[s + q];
        }
        for (; s < K; s++) {
            const double e = E[(size_t)s * m + i];
            if (e != 0.0) x -= e * sa[s];
        }
        v[i] = x;
    }
}
// d_t = E[t] . v (one workgroup per eta, fixed tree)
__global__ __launch_bounds__(kBlock) void mv_eta_dense_dots_kernel(int m, const double* __restrict__ E, const double* __restrict__ v, double* __restrict__ d) {
    __shared__ double red[kBlock / 64];
    const double* e = E + (size_t)blockIdx.x * m;
    double sum = 0.0;
    for (int i = threadIdx.x; i < m; i += kBlock) sum += e[i] * v[i];
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot = 0.0;
        for (int k = 0; k < kBlock / 64; k++) tot += red[k];
        d[blockIdx.x] = tot;
    }
}
// (blocked like the forward solve: the 64 etas of a block by one wavefront, from the last eta down; the earlier threads then add the block's
// products in the same descending order)
__global__ __launch_bounds__(kEtaDenseMax) void mv_eta_dense_btran_solve_kernel(int K, int cap, double* v, const int* __restrict__ pos,
                                                                               const double* __restrict__ piv, const int* __restrict__ prev,
                                                                               const int* __restrict__ next, const double* __restrict__ T,
                                                                               const double* __restrict__ d) {
    __shared__ double s_w[kEtaDenseMax];
    __shared__ double s_diff[2][64];
    __shared__ int s_prev[2][64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const double cv = t < K ? v[pos[t]] : 0.0;          // the vector as it came in, at this eta's position
    const double dt = t < K ? d[t] : 0.0, pv = t < K ? piv[t] : 1.0;
    const int nx = t < K ? next[t] : -1, myprev = t < K ? prev[t] : -1;
    double acc = 0.0;
    __syncthreads();
    const int nblk = (K + 63) / 64;
    for (int blk = nblk - 1, it = 0; blk >= 0; blk--, it++) {
        const int b0 = blk * 64, b1 = min(b0 + 64, K);
        double* sd = s_diff[it & 1];
        int* sp = s_prev[it & 1];
        constexpr int CH = 16;
        if (wave == blk) {
            for (int s1 = b1 - 1; s1 >= b0; s1 -= CH) {
                double e[CH];
#pragma unroll
                for (int q = 0; q < CH; q++) e[q] = (s1 - q >= b0 && t < s1 - q) ? T[(size_t)(s1 - q) * cap + t] : 0.0;
#pragma unroll
                for (int q = 0; q < CH; q++) {
                    const int s = s1 - q;
                    if (s >= b0) {                                      // wave-uniform
                        double diff_mine = 0.0;
                        if (t == s) {
                            // (s_w[nx], nx > s: written by this wavefront in an earlier step of this loop, or by a later block before its barrier)
                            const double cur = nx >= 0 ? s_w[nx] : cv;
                            const double w = (cur - dt - acc) / pv;
                            s_w[s] = w;
                            diff_mine = w - cv;
                            sd[s - b0] = diff_mine;
                            sp[s - b0] = myprev;
                        }
                        const int hi = __builtin_amdgcn_readlane(__double2hiint(diff_mine), s - b0), lo = __builtin_amdgcn_readlane(__double2loint(diff_mine), s - b0);
                        const double diff = __hiloint2double(hi, lo);
                        const int prs = __builtin_amdgcn_readlane(myprev, s - b0);
                        if (t < s && t >= b0 && e[q] != 0.0 && prs <= t) acc += e[q] * diff;
                    }
                }
            }
        }
        __syncthreads();
        if (wave < blk) {
            for (int s1 = b1 - 1; s1 >= b0; s1 -= CH) {
                double e[CH];
#pragma unroll
                for (int q = 0; q < CH; q++) e[q] = s1 - q >= b0 ? T[(size_t)(s1 - q) * cap + t] : 0.0;
#pragma unroll
                for (int q = 0; q < CH; q++) {
                    const int s = s1 - q;
                    // (prev[s] <= t: position pos_s is not replaced again between t and s, so eta t meets the value w_s there)
                    if (s >= b0 && e[q] != 0.0 && sp[s - b0] <= t) acc += e[q] * sd[s - b0];
                }
            }
        }
    }
    __syncthreads();
    if (t < K && myprev < 0) v[pos[t]] = s_w[t];
}

// ---- the two triangular systems as MATRICES (for the eta file that stays behind the factors after Maxvolume, see maxvol_apply_etas) ----
// The multipliers are linear in what the solve kernels read: forward  alpha = F vp  (vp = the vector at the positions of the etas that
// are the FIRST at their position, Kd of them), backward  w = G [d; vp].  One workgroup per unit input runs the solve kernel's own
// recurrence (same chains of repeated positions), all unit inputs in parallel; an application inside the CR loop of the KKT solve is
// then two small matrix-vector products instead of K dependent steps with two barriers each (0.55 us per eta: 0.25 ms at K = 450).
// Other rounding than the sequential form (sums in another order), which Maxvolume itself keeps for its decisions.
__global__ __launch_bounds__(kEtaDenseMax) void mv_eta_forward_matrix_kernel(int K, int Kd, int cap, const int* __restrict__ first, const double* __restrict__ piv,
                                                                            const int* __restrict__ prev, const double* __restrict__ Tt,
                                                                            double* __restrict__ F) {
    __shared__ double s_alpha;
    const int t = threadIdx.x, j = blockIdx.x;
    const int pr = t < K ? prev[t] : -1;
    double r = (t < K && t == first[j]) ? 1.0 : 0.0;                // unit input: 1 at the position whose first eta is first[j]
    const double pv = t < K ? piv[t] : 1.0;
    for (int s = 0; s < K; s++) {
        if (t == s) { const double a = r / pv; s_alpha = a; F[(size_t)s * Kd + j] = a; }
        __syncthreads();
        const double a = s_alpha;
        if (t > s && t < K) {
            if (s == pr) r = a;
            else if (s > pr) r -= Tt[(size_t)s * cap + t] * a;
        }
        __syncthreads();
    }
}
// unit input u < K: d = e_u, vp = 0;  u >= K: d = 0, vp = e_(u-K)
__global__ __launch_bounds__(kEtaDenseMax) void mv_eta_backward_matrix_kernel(int K, int Kd, int cap, const int* __restrict__ jof, const double* __restrict__ piv,
                                                                             const int* __restrict__ prev, const int* __restrict__ next,
                                                                             const double* __restrict__ T, double* __restrict__ G) {
    __shared__ double s_diff;
    __shared__ double s_w[kEtaDenseMax];
    const int t = threadIdx.x, u = blockIdx.x, W = K + Kd;
    const double cv = (t < K && u >= K && jof[t] == u - K) ? 1.0 : 0.0;
    const double dt = (t < K && u == t) ? 1.0 : 0.0, pv = t < K ? piv[t] : 1.0;
    const int nx = t < K ? next[t] : -1;
    double acc = 0.0;
    __syncthreads();
    for (int s = K - 1; s >= 0; s--) {
        if (t == s) {
            const double cur = nx >= 0 ? s_w[nx] : cv;
            const double w = (cur - dt - acc) / pv;
            s_w[s] = w;
            s_diff = w - cv;
            G[(size_t)s * W + u] = w;
        }
        __syncthreads();
        if (t < s && prev[s] <= t) acc += T[(size_t)s * cap + t] * s_diff;
        __syncthreads();
    }
}
// alpha[t] = F[t] . vp,  vp[j] = v[pos[first[j]]]   (one wavefront per row)
__global__ __launch_bounds__(kBlock) void mv_eta_forward_gemv_kernel(int K, int Kd, const double* __restrict__ F, const int* __restrict__ first,
                                                                    const int* __restrict__ pos, const double* __restrict__ v, double* __restrict__ alpha) {
    const int lane = threadIdx.x & 63;
    for (int t = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); t < K; t += gridDim.x * (kBlock / 64)) {
        double sum = 0.0;
        for (int j = lane; j < Kd; j += 64) sum += F[(size_t)t * Kd + j] * v[pos[first[j]]];
        sum = wave_sum(sum);
        if (lane == 0) alpha[t] = sum;
    }
}
// w[t] = G[t] . [d; vp]
__global__ __launch_bounds__(kBlock) void mv_eta_backward_gemv_kernel(int K, int Kd, const double* __restrict__ G, const int* __restrict__ first,
                                                                     const int* __restrict__ pos, const double* __restrict__ d, const double* __restrict__ v,
                                                                     double* __restrict__ w) {
    const int lane = threadIdx.x & 63, W = K + Kd;
    for (int t = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); t < K; t += gridDim.x * (kBlock / 64)) {
        double sum = 0.0;
        for (int u = lane; u < W; u += 64) sum += G[(size_t)t * W + u] * (u < K ? d[u] : v[pos[first[u - K]]]);
        sum = wave_sum(sum);
        if (lane == 0) w[t] = sum;
    }
}
// v[pos[first[j]]] = w[first[j]]
__global__ void mv_eta_backward_scatter_kernel(int Kd, const int* __restrict__ first, const int* __restrict__ pos, const double* __restrict__ w,
                                               double* __restrict__ v) {
    IPXK_GRID_STRIDE(j, Kd) v[pos[first[j]]] = w[first[j]];
}
// the compact lists: the nonzeros of the tableau column flagged, ranked by a scan, stored
__global__ void mv_eta_flag_kernel(int m, const Scalars* S, const double* __restrict__ lhs, int* __restrict__ flag) {
    IPXK_GRID_STRIDE(p, m) flag[p] = ((int)p != S->pmax && lhs[p] != 0.0) ? 1 : 0;
}
__global__ void mv_eta_store_kernel(int m, int K, const Scalars* S, const double* __restrict__ lhs, const int* __restrict__ flag,
                                    const int* __restrict__ rank, int* ptr, int* pos, double* piv, int* idx, double* val, Scalars* Sout) {
    const int base = ptr[K];
    IPXK_GRID_STRIDE(p, m) {
        if (flag[p]) { idx[base + rank[p]] = (int)p; val[base + rank[p]] = lhs[p]; }
        if (p == m - 1) {
            ptr[K + 1] = base + rank[p] + flag[p];
            pos[K] = S->pmax;
            piv[K] = lhs[S->pmax];
            Sout->eta_total = base + rank[p] + flag[p];
        }
    }
}

}  // namespace

// The etas of the exchanges since the last refactorization: dense rows (mv_eta_dense_*) where the
// K x m matrix fits and pays (EtaFile::reset: long vectors with short etas -- the slack bases of a 1M-row model -- keep the lists), else the
// compact lists walked one after the other.  When to refactorize: after max_etas exchanges (the
// reference's update limit, src/maxvolume.cc:318-319) -- or, with max_etas < 0 (what KKTSolverBasisHip passes), when the time
// the etas have cost since the last refactorization reaches the time a refactorization costs, both taken from a MODEL so that a
// run does not depend on the clock: a refactorization 25 ms + 3.5e-13 s x (rows of the dense block)^3 (LU + the block's inverse:
// 0.16 s at 7350 rows, 1.2 s at 15 000), an application of K etas K x (0.6 us + 8 m bytes at 2 TB/s), three applications per
// exchange; at least 100, at most 1024 etas.  (Measured on the 24 000 x 60 000 LP: 40 refactorizations of 0.15 s inside
// Maxvolume with the fixed limit of 100.)
// (the struct itself: internal.hpp)
EtaFile::EtaFile(Context* ctx, MaxvolState& state, int rows, ipxint max_etas_in, bool resume) : c(ctx), M(state), m(rows), s(ctx->stream) {
    adaptive = max_etas_in < 0;
    limit = (int)std::max<ipxint>(1, max_etas_in > 0 ? max_etas_in : 100);
    static const bool dense_off = getenv("IPXK_MAXVOL_DENSE_ETAS") && getenv("IPXK_MAXVOL_DENSE_ETAS")[0] == '0';
    const int64_t fit = (int64_t(1) << 28) / std::max(m, 1);                   // 2 GiB of etas
    cap = adaptive ? (int)std::min<int64_t>(kEtaDenseMax, std::max<int64_t>(limit, fit)) : limit;
    dense_possible = !dense_off && cap <= kEtaDenseMax && (int64_t)cap <= std::max<int64_t>(fit, 1);
    if (!dense_possible) { cap = limit; adaptive = false; }
    sparse_cap = std::max<int64_t>(4 * (int64_t)m, int64_t(1) << 20);
    M.eta_pos.ensure((size_t)cap); M.eta_piv.ensure((size_t)cap);
    const MaxvolState::Saved& sv = M.saved;
    if (resume && sv.live && sv.cap == cap && sv.m == m && (sv.dense ? dense_possible : true)) {
        // the etas of the previous call are still behind the factors: go on where it stopped
        dense = sv.dense; have_history = sv.have_history; K = sv.K; sparse_used = sv.sparse_used; seg_nnz = sv.seg_nnz;
        overhead_s = sv.overhead_s; refactor_s = sv.refactor_s;
        resumed = true;
    } else {
        reset(0);
    }
}
void EtaFile::save() {
    MaxvolState::Saved& sv = M.saved;
    sv.live = true; sv.dense = dense; sv.have_history = have_history; sv.K = K; sv.cap = cap; sv.m = m; sv.sparse_used = sparse_used;
    sv.seg_nnz = seg_nnz; sv.overhead_s = overhead_s; sv.refactor_s = refactor_s;
    sv.lu_generation = lu_generation(c);
    sv.Kd = 0;
    static const bool matrices_off = getenv("IPXK_MAXVOL_ETA_MATRICES") && getenv("IPXK_MAXVOL_ETA_MATRICES")[0] == '0';
    if (dense && K > 0 && !matrices_off) {
        // the two triangular systems as matrices, for the applications inside the KKT solve (mv_eta_*_matrix_kernel)
        std::vector<int> prev_h((size_t)K), pos_h((size_t)K), first, jof((size_t)K, -1);
        M.eta_prev.download(prev_h.data(), (size_t)K, s);
        M.eta_pos.download(pos_h.data(), (size_t)K, s);
        IPXK_HIP(hipStreamSynchronize(s));
        for (int t = 0; t < K; t++) {
            if (prev_h[t] < 0) { jof[t] = (int)first.size(); first.push_back(t); }
            else jof[t] = jof[prev_h[t]];
        }
        const int Kd = (int)first.size();
        M.eta_first.upload(first, s); M.eta_jof.upload(jof, s);
        M.etaF.ensure((size_t)K * Kd); M.etaG.ensure((size_t)K * (K + Kd)); M.eta_w.ensure((size_t)K);
        hipLaunchKernelGGL(mv_eta_forward_matrix_kernel, dim3(Kd), dim3(std::min(kEtaDenseMax, (K + 63) / 64 * 64)), 0, s, K, Kd, cap, M.eta_first.get(), M.eta_piv.get(),
                           M.eta_prev.get(), M.etaTt.get(), M.etaF.get());
        hipLaunchKernelGGL(mv_eta_backward_matrix_kernel, dim3(K + Kd), dim3(std::min(kEtaDenseMax, (K + 63) / 64 * 64)), 0, s, K, Kd, cap, M.eta_jof.get(), M.eta_piv.get(),
                           M.eta_prev.get(), M.eta_next.get(), M.etaT.get(), M.etaG.get());
        IPXK_HIP(hipStreamSynchronize(s));               // (the host vectors go out of scope)
        IPXK_HIP(hipGetLastError());
        sv.Kd = Kd;
    }
}
// what the K etas cost in the solves of one KKT solve (~ 100 CR iterations, one application per direction and iteration, a few dense
// solves around them) against what a refactorization costs: whether the etas stay behind the factors when Maxvolume is over
bool EtaFile::worth_keeping() const {
    if (K == 0 || full()) return false;
    // (dense form: the triangular systems go through their matrices inside the KKT solve -- what is left per eta is its row of E)
    const double per_eta = dense ? 8.0 * (double)m / 2e12 + 0.05e-6 : cost_list(K > 0 ? (double)seg_nnz / K : 0.0);
    return 220.0 * ((double)K * per_eta + 40e-6) < refactor_s;          // (40 us: the seven extra launches of an application)
}
// after a (re)factorization whose dense block has `block_rows` rows: the next segment's etas as dense rows or as lists, whichever
// the previous segment's etas would have cost less in (no segment yet: from m alone -- the lists only pay beyond ~ 475 000 rows)
void EtaFile::reset(int block_rows) {
    if (dense_possible) {
        const double avg = have_history && K > 0 ? (double)seg_nnz / K : 0.0;
        dense = cost_dense() < cost_list(avg);
        static const bool force = getenv("IPXK_MAXVOL_DENSE_ETAS") && getenv("IPXK_MAXVOL_DENSE_ETAS")[0] == '1';
        if (force) dense = true;
    } else {
        dense = false;
    }
    if (K > 0) have_history = true;
    K = 0;
    sparse_used = 0;
    seg_nnz = 0;
    overhead_s = 0.0;
    refactor_s = 0.025 + 3.5e-13 * (double)block_rows * (double)block_rows * (double)block_rows;
    if (dense) {
        M.etaE.ensure((size_t)cap * m); M.etaT.ensure((size_t)cap * cap); M.etaTt.ensure((size_t)cap * cap);
        M.eta_alpha.ensure((size_t)cap); M.eta_d.ensure((size_t)cap);
        M.eta_prev.ensure((size_t)cap); M.eta_next.ensure((size_t)cap);
        M.eta_last.ensure((size_t)m);
        IPXK_HIP(hipMemsetAsync(M.eta_last.get(), 0xff, (size_t)m * sizeof(int), s));
    } else {
        M.flag.ensure((size_t)m); M.rank.ensure((size_t)m);
        M.eta_ptr.ensure((size_t)cap + 1);
        M.eta_idx.ensure((size_t)sparse_cap + m); M.eta_val.ensure((size_t)sparse_cap + m);
        IPXK_HIP(hipMemsetAsync(M.eta_ptr.get(), 0, sizeof(int), s));
    }
}
// the eta of the exchange described by *S (pmax) from the tableau column lhs; eta_nnz: its number of nonzeros
void EtaFile::append(const MvScalars* S, const double* lhs, int eta_nnz) {
    const int gm = grid_for(m);
    if (dense) {
        hipLaunchKernelGGL(mv_eta_dense_append_kernel, dim3(gm), dim3(kBlock), 0, s, m, K, cap, S, lhs, M.etaE.get(), M.eta_pos.get(), M.eta_piv.get(),
                           M.eta_prev.get(), M.eta_next.get(), M.eta_last.get(), M.etaT.get(), M.etaTt.get());
    } else {
        hipLaunchKernelGGL(mv_eta_flag_kernel, dim3(gm), dim3(kBlock), 0, s, m, S, lhs, M.flag.get());
        size_t bytes = 0;
        IPXK_HIP(rocprim::exclusive_scan(nullptr, bytes, M.flag.get(), M.rank.get(), 0, (size_t)m, rocprim::plus<int>(), s));
        if (M.tmp.size() < bytes) M.tmp.resize(bytes);
        IPXK_HIP(rocprim::exclusive_scan(M.tmp.get(), bytes, M.flag.get(), M.rank.get(), 0, (size_t)m, rocprim::plus<int>(), s));
        hipLaunchKernelGGL(mv_eta_store_kernel, dim3(gm), dim3(kBlock), 0, s, m, K, S, lhs, M.flag.get(), M.rank.get(), M.eta_ptr.get(), M.eta_pos.get(),
                           M.eta_piv.get(), M.eta_idx.get(), M.eta_val.get(), M.scalars.get());
        sparse_used += eta_nnz;
    }
    K++;
    seg_nnz += eta_nnz;
    overhead_s += 3.0 * (dense ? (double)K * cost_dense() : (double)K * 2.5e-6 + 0.5e-9 * (double)seg_nnz);
}
bool EtaFile::full() const {                                                             // NeedFreshFactorization (src/maxvolume.cc:318-319)
    if (K >= cap) return true;
    if (!dense && sparse_used + m > sparse_cap) return true;
    if (adaptive) return K >= 100 && overhead_s >= refactor_s;
    return K >= limit;
}
void EtaFile::apply(bool transposed, double* v) { apply_etas(M, m, K, cap, dense, transposed, v, s); }
// Kd > 0: the triangular systems through their matrices (a kept file inside the KKT solve); 0: the sequential, bit-reproducible form
void EtaFile::apply_etas(MaxvolState& M, int m, int K, int cap, bool dense, bool transposed, double* v, hipStream_t s, int Kd) {
    if (K == 0) return;
    if (dense && Kd > 0) {
        const int gk = (K + kBlock / 64 - 1) / (kBlock / 64);
        if (transposed) {
            hipLaunchKernelGGL(mv_eta_dense_dots_kernel, dim3(K), dim3(kBlock), 0, s, m, M.etaE.get(), v, M.eta_d.get());
            hipLaunchKernelGGL(mv_eta_backward_gemv_kernel, dim3(gk), dim3(kBlock), 0, s, K, Kd, M.etaG.get(), M.eta_first.get(), M.eta_pos.get(),
                               M.eta_d.get(), v, M.eta_w.get());
            hipLaunchKernelGGL(mv_eta_backward_scatter_kernel, dim3(grid_for(Kd)), dim3(kBlock), 0, s, Kd, M.eta_first.get(), M.eta_pos.get(),
                               M.eta_w.get(), v);
        } else {
            hipLaunchKernelGGL(mv_eta_forward_gemv_kernel, dim3(gk), dim3(kBlock), 0, s, K, Kd, M.etaF.get(), M.eta_first.get(), M.eta_pos.get(), v,
                               M.eta_alpha.get());
            hipLaunchKernelGGL(mv_eta_dense_ftran_apply_kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, m, K, M.etaE.get(), M.eta_alpha.get(),
                               M.eta_last.get(), v);
        }
        return;
    }
    // (the one-workgroup solves: only as many wavefronts as there are etas -- their two barriers per eta cost by the wavefront)
    const int solve_threads = std::min(kEtaDenseMax, (K + 63) / 64 * 64);
    if (dense && transposed) {
        hipLaunchKernelGGL(mv_eta_dense_dots_kernel, dim3(K), dim3(kBlock), 0, s, m, M.etaE.get(), v, M.eta_d.get());
        hipLaunchKernelGGL(mv_eta_dense_btran_solve_kernel, dim3(1), dim3(solve_threads), 0, s, K, cap, v, M.eta_pos.get(), M.eta_piv.get(),
                           M.eta_prev.get(), M.eta_next.get(), M.etaT.get(), M.eta_d.get());
    } else if (dense) {
        hipLaunchKernelGGL(mv_eta_dense_ftran_solve_kernel, dim3(1), dim3(solve_threads), 0, s, K, cap, v, M.eta_pos.get(), M.eta_piv.get(),
                           M.eta_prev.get(), M.etaTt.get(), M.eta_alpha.get());
        hipLaunchKernelGGL(mv_eta_dense_ftran_apply_kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, m, K, M.etaE.get(), M.eta_alpha.get(),
                           M.eta_last.get(), v);
    } else if (transposed) {
        hipLaunchKernelGGL(mv_eta_btran_kernel, dim3(1), dim3(kEtaThreads), 0, s, K, M.eta_ptr.get(), M.eta_pos.get(), M.eta_piv.get(), M.eta_idx.get(),
                           M.eta_val.get(), v);
    } else {
        hipLaunchKernelGGL(mv_eta_ftran_kernel, dim3(1), dim3(kEtaThreads), 0, s, K, M.eta_ptr.get(), M.eta_pos.get(), M.eta_piv.get(), M.eta_idx.get(),
                           M.eta_val.get(), v);
    }
}

// Basis::TightenLuPivotTol (src/basis.cc:490-503): the next step of the reference's ladder, false at its top
bool tighten_pivottol(double& pivottol) {
    if (pivottol <= 0.05) pivottol = 0.1;
    else if (pivottol <= 0.25) pivottol = 0.3;
    else if (pivottol <= 0.5) pivottol = 0.9;
    else return false;
    return true;
}

// the small kernels of an exchange
void mv_scatter_column(Context* c, const MvScalars* S, double* rhs) {
    IPXK_HIP(hipMemsetAsync(rhs, 0, (size_t)c->m * sizeof(double), c->stream));
    hipLaunchKernelGGL(mv_scatter_column_kernel, dim3(4), dim3(kBlock), 0, c->stream, (int)c->n, S, c->pl_Ap.get(), c->pl_Ai.get(), c->pl_Ax.get(), rhs);
}
void mv_unit_vector(Context* c, const MvScalars* S, double* v) {
    hipLaunchKernelGGL(mv_unit_kernel, dim3(grid_for(c->m)), dim3(kBlock), 0, c->stream, (int)c->m, S, v);
}
void mv_pivot_from_row(Context* c, const double* btran, MvScalars* S) {
    hipLaunchKernelGGL(mvs_pivot_row_kernel, dim3(1), dim3(kBlock), 0, c->stream, (int)c->n, c->pl_Ap.get(), c->pl_Ai.get(), c->pl_Ax.get(), btran, S);
}

// ---- the etas behind the resident factors (Context::etas_live) -------------------------------------------------------------
// When Maxvolume is over and its last exchanges are few, the fresh factorization of the final basis that the reference asks for
// (src/kkt_solver_basis.cc:56-61, Basis::GetLuFactors) costs more than carrying the etas through the solves of the KKT solve that
// follows: B_new = B_old E_1 ... E_K, so  inverse(B_new) v = inverse(E_K) ... inverse(E_1) inverse(B_old) v  -- the resident factors and
// the eta file as they stand (the form Basis::SolveDense has after Forrest-Tomlin updates, src/forrest_tomlin.cc:67-78).  The operator
// of trisolve.hip and solve_dense_dev apply the etas through the two functions below; the next call of Maxvolume goes on with the same
// file.  A new operator (ipxk_split_prepare*) ends this state; a new factorization in the context (the LU kernel of the reference's
// Basis may share it) leaves operator and etas as they are -- they do not read the LU state -- but the next Maxvolume starts from fresh factors.
void maxvol_apply_etas(Context* c, bool transposed, double* v) {
    IPXK_REQUIRE(c->maxvol && c->maxvol->saved.live, "no eta file behind the factors");
    MaxvolState& M = *c->maxvol;
    EtaFile::apply_etas(M, M.saved.m, M.saved.K, M.saved.cap, M.saved.dense, transposed, v, c->stream, M.saved.Kd);
}
const ipxint* maxvol_current_basis(Context* c) {
    IPXK_REQUIRE(c->maxvol && c->maxvol->saved.live, "no eta file behind the factors");
    return c->maxvol->basis.get();
}
void maxvol_drop_etas(Context* c) {
    c->etas_live = false;
    if (c->maxvol) c->maxvol->saved.live = false;
}

// ---- DeviceBasis (the struct itself: internal.hpp) ----------------------------------------------------------------------------------
DeviceBasis::DeviceBasis(Context* ctx, MaxvolState& state, ipxint max_etas, bool resume, const double* colscale_in, MvScalars* scalars)
    : c(ctx), M(state), m((int)ctx->m), etas(ctx, state, (int)ctx->m, max_etas, resume), pivottol(ctx->maxvol_pivottol),
      basis_h((size_t)ctx->m), colscale(colscale_in), S(scalars) {
    for (DevBuf<double>* b : {&M.rhs, &M.lhs, &M.unit, &M.btran}) b->ensure((size_t)m);
    rhs = M.rhs.get(); lhs = M.lhs.get(); unit = M.unit.get(); btran = M.btran.get();
}
void DeviceBasis::ftran() {
    mv_scatter_column(c, S, rhs);
    solve_dense_dev(c, rhs, lhs, 'N');
    etas.apply(false, lhs);
}
void DeviceBasis::btran_unit() {
    mv_unit_vector(c, S, unit);
    etas.apply(true, unit);
    solve_dense_dev(c, unit, btran, 'T');
}
// Basis::Factorize (src/basis.cc:116-156) + the operator of the sweeps
bool DeviceBasis::refactorize() {
    ipxk_lu_info li{};
    lu_factorize_basis(c, basis_h.data(), pivottol, false, &li);
    factorizations++;
    if (li.num_dependent > 0) { errflag = 301; singular++; return false; }        // IPX_ERROR_basis_singular (:131-137)
    split_prepare_lu(c, status_h.data(), colscale);
    etas.reset((int)li.bump);
    return true;
}
// Basis::ExchangeIfStable (:286-321): the pivot from the row against the pivot from the column.  On fresh factors the pivot tolerance is
// tightened first, and only when that is no longer possible the basis is declared too ill conditioned (:299-306).
bool DeviceBasis::exchange_if_stable(const MvScalars& a) {
    const double pc = a.pivot_col, pr = a.pivot_row;
    const bool stable = pc != 0.0 && std::abs(pc - pr) <= 1e-8 * std::abs(pc);
    if (!stable) {
        refused++;
        if (etas.K == 0 && !tighten_pivottol(pivottol)) { errflag = 306; return false; }       // IPX_ERROR_basis_too_ill_conditioned
        (void)refactorize();
        return false;                                                                           // "try again" (:290-291)
    }
    etas.append(S, lhs, a.eta_nnz);
    return true;
}
void DeviceBasis::commit(const MvScalars& a) {
    basis_h[(size_t)a.pmax] = a.jn;
    status_h[(size_t)a.jn] = IPXK_BASIC;
    status_h[(size_t)a.jb] = IPXK_NONBASIC;
    if (etas.full()) (void)refactorize();                                                       // NeedFreshFactorization (:318-319)
}

}  // namespace ipxk
