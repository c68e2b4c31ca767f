// The dense LU of the bump (step 2 of lu.hip's header comment): partial pivoting, right-looking, in panels of 32 columns.
// Every entry receives its updates one pivot at a time in pivot order, products rounded before they are subtracted (the MFMA
// trailing update excepted, see there); rows are never swapped (a row carries the step at which it was pivoted).  One entry
// point, lu_dense_factorize (lu_internal.hpp); which kernels take a block of kb rows is decided by LuPolicy.
#include <climits>

#include "lu_internal.hpp"

namespace ipxk {

namespace {

struct Dense {
    int kb;
    double* D;             // column-major kb x kb
    int *brstep, *bcstep;  // pivot step of a bump row / column, -1 while unpivoted / for a dependent column
    int* bstep;            // [0] # pivots so far; [1] # pivots of the current (sub-)panel; [3] # pivots of the outer panel before it
                           // (look-ahead: two sets of bstep / prow / pcol, used by the outer panels alternately)
    int *prow, *pcol;      // rows / columns of the current panel's pivots
    double abstol;
};

// One panel of columns [c0, c1): partial pivoting (largest |entry| among the unpivoted rows, ties: smaller
// row), scaling, update of the panel's later columns.  One workgroup; the panel lives in L2.
__global__ __launch_bounds__(kPanelThreads) void lu_panel_kernel(Dense A, int c0, int c1) {
    __shared__ double red_v[kPanelThreads / 64];
    __shared__ int red_r[kPanelThreads / 64];
    __shared__ double su[kPanel];
    __shared__ int s_pr;
    __shared__ double s_piv;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kb = A.kb;
    int np = 0;
    int step = A.bstep[0];
    for (int c = c0; c < c1; c++) {
        double* col = A.D + (size_t)c * kb;
        double best = 0.0;
        int br = INT_MAX;
        for (int r = tid; r < kb; r += kPanelThreads)
            if (A.brstep[r] < 0) {
                const double a = fabs(col[r]);
                if (a > best) { best = a; br = r; }
            }
        wave_argmax(best, br);
        if (lane == 0) { red_v[wave] = best; red_r[wave] = br; }
        __syncthreads();
        if (tid == 0) {
            double bv = 0.0;
            int r = INT_MAX;
            for (int w = 0; w < kPanelThreads / 64; w++)
                if (red_v[w] > bv || (red_v[w] == bv && red_r[w] < r)) { bv = red_v[w]; r = red_r[w]; }
            if (r == INT_MAX || !(bv >= A.abstol) || bv == 0.0) {
                s_pr = -1;
                A.bcstep[c] = -1;
            } else {
                s_pr = r;
                s_piv = col[r];
                A.brstep[r] = step;
                A.bcstep[c] = step;
                A.prow[np] = r;
                A.pcol[np] = c;
            }
        }
        __syncthreads();
        const int pr = s_pr;
        if (pr < 0) continue;                 // dependent column (uniform over the workgroup)
        const double piv = s_piv;
        np++;
        step++;
        if (tid < c1 - c - 1) su[tid] = A.D[(size_t)(c + 1 + tid) * kb + pr];
        __syncthreads();
        for (int r = tid; r < kb; r += kPanelThreads) {
            if (A.brstep[r] >= 0) continue;   // pivoted rows (this step's included) keep their values
            const double l = col[r] / piv;
            col[r] = l;
            for (int c2 = c + 1; c2 < c1; c2++) {
                const double u = su[c2 - c - 1];
                if (u != 0.0) A.D[(size_t)c2 * kb + r] -= l * u;
            }
        }
        __syncthreads();
    }
    if (tid == 0) { A.bstep[0] = step; A.bstep[1] = np; }
}

// The same for bumps of at most kPanelThreads rows: a thread owns one row of the panel in registers, the pivot
// row travels through LDS; the panel is read and written once.  Same arithmetic, same order.  (The column steps
// are instantiated one by one: v[] must be indexed by constants to stay in registers.)
// (two copies of everything, used alternately by consecutive pivot steps: a step then needs two barriers, not four --
// every thread combines the wavefronts' candidates itself, and no barrier has to protect the buffers for the next step)
struct PanelShared {
    double red_v[2][kPanelThreads / 64];
    int red_r[2][kPanelThreads / 64];
    double su[2][kPanel];
};
// the pivot row of a step from the wavefronts' candidates (largest |entry|, ties: smaller row); -1: none / no column
__device__ __forceinline__ int panel_pivot_row(const PanelShared& sh, int par, bool col, double abstol, bool* dependent) {
    // (every lane reads one wavefront's candidate and the sixteen are combined by shuffles: the same selection -- a total order --
    // as a scan of all sixteen by every thread, at a third of the LDS traffic: the scan was 1 us of a 4.5 us pivot step)
    static_assert(kPanelThreads / 64 == 16, "sixteen wavefronts");
    double bv = sh.red_v[par][threadIdx.x & 15];
    int rr = sh.red_r[par][threadIdx.x & 15];
    if (!(bv > 0.0)) { bv = 0.0; rr = INT_MAX; }          // (no candidate, or not a number: never a pivot)
    wave_argmax<16>(bv, rr);
    *dependent = col && (rr == INT_MAX || !(bv >= abstol) || bv == 0.0);
    return col && !*dependent ? rr : -1;
}
template <int T>
__device__ __forceinline__ void panel_small_steps(const Dense& A, PanelShared& sh, double (&v)[kPanel], int c0, int c1, int r,
                                                  bool& active, int& np, int& step) {
    if constexpr (T < kPanel) {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const bool col = c0 + T < c1;                  // uniform
        double best = (col && active) ? fabs(v[T]) : 0.0;
        int br = best > 0.0 ? r : INT_MAX;
        wave_argmax(best, br);
        constexpr int par = T & 1;
        if (lane == 0) { sh.red_v[par][wave] = best; sh.red_r[par][wave] = br; }
        __syncthreads();
        bool dependent;
        const int pr = panel_pivot_row(sh, par, col, A.abstol, &dependent);      // uniform over the workgroup
        if (tid == 0) {
            if (dependent) A.bcstep[c0 + T] = -1;
            else if (pr >= 0) {
                A.brstep[pr] = step;
                A.bcstep[c0 + T] = step;
                A.prow[np] = pr;
                A.pcol[np] = c0 + T;
            }
        }
        if (pr >= 0 && r == pr) {
            active = false;
#pragma unroll
            for (int t2 = 0; t2 < kPanel; t2++) sh.su[par][t2] = v[t2];
        }
        __syncthreads();
        if (pr >= 0) { np++; step++; }
        if (pr >= 0 && active) {
            const double l = v[T] / sh.su[par][T];
            v[T] = l;
#pragma unroll
            for (int t2 = T + 1; t2 < kPanel; t2++) {
                const double u = sh.su[par][t2];
                if (c0 + t2 < c1 && u != 0.0) v[t2] -= l * u;
            }
        }
        panel_small_steps<T + 1>(A, sh, v, c0, c1, r, active, np, step);
    }
}
__global__ __launch_bounds__(kPanelThreads) void lu_panel_small_kernel(Dense A, int c0, int c1) {
    __shared__ PanelShared sh;
    const int kb = A.kb, r = threadIdx.x;
    const bool have = r < kb;
    bool active = have && A.brstep[r] < 0;
    double v[kPanel];
#pragma unroll
    for (int t = 0; t < kPanel; t++) v[t] = (have && c0 + t < c1) ? A.D[(size_t)(c0 + t) * kb + r] : 0.0;
    int np = 0;
    int step = A.bstep[0];
    panel_small_steps<0>(A, sh, v, c0, c1, r, active, np, step);
    if (have) {
#pragma unroll
        for (int t = 0; t < kPanel; t++)
            if (c0 + t < c1) A.D[(size_t)(c0 + t) * kb + r] = v[t];
    }
    if (threadIdx.x == 0) { A.bstep[0] = step; A.bstep[1] = np; }
}

template <int R, int W, int T>
__device__ __forceinline__ void panel_multi_steps(const Dense& A, PanelShared& sh, double (&v)[R][W], int c0, int c1,
                                                  unsigned& active, int& np, int& step) {
    if constexpr (T < W) {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        const bool col = c0 + T < c1;                  // uniform
        double best = 0.0;
        int br = INT_MAX;
#pragma unroll
        for (int q = 0; q < R; q++) {
            const double a = (col && ((active >> q) & 1u)) ? fabs(v[q][T]) : 0.0;
            if (a > best) { best = a; br = tid + q * kPanelThreads; }      // rows ascend with q: the first maximum stays
        }
        wave_argmax(best, br);
        constexpr int par = T & 1;
        if (lane == 0) { sh.red_v[par][wave] = best; sh.red_r[par][wave] = br; }
        __syncthreads();
        bool dependent;
        const int pr = panel_pivot_row(sh, par, col, A.abstol, &dependent);      // uniform over the workgroup
        if (tid == 0) {
            if (dependent) A.bcstep[c0 + T] = -1;
            else if (pr >= 0) {
                A.brstep[pr] = step;
                A.bcstep[c0 + T] = step;
                A.prow[np] = pr;
                A.pcol[np] = c0 + T;
            }
        }
        if (pr >= 0 && (pr % kPanelThreads) == tid) {
            const int qp = pr / kPanelThreads;
#pragma unroll
            for (int q = 0; q < R; q++)
                if (q == qp) {
                    active &= ~(1u << q);
#pragma unroll
                    for (int t2 = 0; t2 < W; t2++) sh.su[par][t2] = v[q][t2];
                }
        }
        __syncthreads();
        if (pr >= 0) {
            np++; step++;
#pragma unroll
            for (int q = 0; q < R; q++)
                if ((active >> q) & 1u) {
                    const double l = v[q][T] / sh.su[par][T];
                    v[q][T] = l;
#pragma unroll
                    for (int t2 = T + 1; t2 < W; t2++) {
                        const double u = sh.su[par][t2];
                        if (c0 + t2 < c1 && u != 0.0) v[q][t2] -= l * u;
                    }
                }
        }
        panel_multi_steps<R, W, T + 1>(A, sh, v, c0, c1, active, np, step);
    }
}
// Two-level panels (round 4): the kernel factorizes a SUB-panel [c0, c1) of an outer panel of kPanel columns; its pivots
// are appended to the outer panel's list (first_inner: the list starts again), bstep[3] = # pivots of the outer panel
// before this sub-panel, bstep[1] = # pivots of this sub-panel.  The sub-panel's update is applied to the rest of
// the outer panel only; the whole trailing matrix is updated once per outer panel with all its pivots (in pivot
// order, one rounded product at a time: every entry still receives exactly the arithmetic of the column-by-column
// elimination).  Before: a full-matrix update per 8- or 16-column panel, and bumps of more than 4096 rows went
// through lu_panel_kernel (one workgroup, the panel in L2: 1.2 ms per panel, 0.3 s for a 6000-row bump).
// (usub / c1o: the previous sub-panel's rows of U in the rest of the outer panel, columns [c0, c1o), which lu_subpanel_update_kernel
// left in a side buffer -- every one of its workgroups needs the rows as they were -- are written to their places here first.)
template <int R, int W>
__global__ __launch_bounds__(kPanelThreads) void lu_panel_multi_kernel(Dense A, int c0, int c1, int first_inner, const double* __restrict__ usub = nullptr,
                                                                       int c1o = 0, const int* __restrict__ step_src = nullptr) {
    __shared__ PanelShared sh;
    const int kb = A.kb, tid = threadIdx.x;
    const int base = first_inner ? 0 : A.bstep[3] + A.bstep[1];
    if (usub && !first_inner) {
        const int pf = A.bstep[3], pn = A.bstep[1], nc = c1o - c0;
        for (int e = tid; e < pn * nc; e += kPanelThreads) {
            const int t = e / nc, x = e - t * nc;
            if (t > 0) A.D[(size_t)(c0 + x) * kb + A.prow[pf + t]] = usub[t * kPanel + x];      // (the first pivot's row is unchanged)
        }
        __syncthreads();
    }
    A.prow += base; A.pcol += base;
    unsigned active = 0, have = 0;
    double v[R][W];
#pragma unroll
    for (int q = 0; q < R; q++) {
        const int r = tid + q * kPanelThreads;
        if (r < kb) { have |= 1u << q; if (A.brstep[r] < 0) active |= 1u << q; }
#pragma unroll
        for (int t = 0; t < W; t++) v[q][t] = (r < kb && c0 + t < c1) ? A.D[(size_t)(c0 + t) * kb + r] : 0.0;
    }
    int np = 0;
    int step = (first_inner && step_src) ? step_src[0] : A.bstep[0];       // (look-ahead: the count so far is in the other set)
    panel_multi_steps<R, W, 0>(A, sh, v, c0, c1, active, np, step);
#pragma unroll
    for (int q = 0; q < R; q++)
        if ((have >> q) & 1u) {
            const int r = tid + q * kPanelThreads;
#pragma unroll
            for (int t = 0; t < W; t++)
                if (c0 + t < c1) A.D[(size_t)(c0 + t) * kb + r] = v[q][t];
        }
    if (tid == 0) { A.bstep[0] = step; A.bstep[1] = np; A.bstep[3] = base; }
}

// COOPERATIVE OUTER PANEL (round 5).  The two-level scheme above spends a one-workgroup launch (24 us) per sub-panel of 2 ... 16 columns
// plus a launch (15 us) that carries the sub-panel's update to the rest of the outer panel: 316 us per 32 columns at 8000 rows, 620 us
// beyond 8192 rows -- 70 of the 80 ms of a 7350-row block, and the largest item of a whole LP solve
// (profiles/r05_lp_dropin_24000_kernel_summary_before_eta_rework.txt).  Here the WHOLE outer panel of kPanel columns is factorized by ONE launch
// of G <= 64 workgroups of 256 threads that share the rows (R = 1 / 2 rows of the panel per thread in registers: up to 8192 / 32 768 rows).  Per column ONE exchange: every workgroup publishes its best candidate (|entry|, row) TOGETHER with that row's 32
// panel entries (write-through stores, drained, then one agent-scope add to a counter); everyone polls the counter, reads the G
// messages past L1, takes the same winner (largest |entry|, ties: smaller row -- a total order, so the choice does not depend on G)
// and has the pivot row with it.  No second exchange, no sub-panels, no side buffer.  Every entry still receives its updates one pivot at
// a time in pivot order, products rounded before they are subtracted: the factors equal the other kernels' bit for bit.
// All G workgroups must be resident at once: G <= 64 (two per compute unit fit) on 256 compute units, nothing else on the stream (the
// look-ahead's late update runs under a CU mask that leaves 32 units free); a poll that does not see its word within kCoopSpinLimit polls raises an abort flag
// that ends every workgroup, and the factorization fails loudly instead of hanging.
constexpr int kCoopMaxG = 64;
constexpr int kCoopSlot = kPanel + 2;                 // a message: |entry|, row, the row's kPanel entries
constexpr int kCoopSpinLimit = 1 << 22;
struct CoopShared {
    double red_v[kCoopThreads / 64];
    int red_r[kCoopThreads / 64];
    double row[kPanel];
    double slots[kCoopMaxG * kCoopSlot];
    int abort;
    int part, G;            // this workgroup among the participants, their number
    int plain;              // all participants share one XCD (checked): messages and resets by plain stores that stay in its L2
};
struct Coop {
    double* slots;          // [5][G][kCoopSlot], every word the sentinel or a message
    int set0;               // the set of this launch's first step (the steps of a factorization take the five sets in turn)
    int* abort_flag;
    int xcd_mode;           // 1: only the workgroups with blockIdx % 8 == 0 take part (one XCD under the round-robin dispatch of gfx950)
    unsigned epoch;         // of the placement check
    unsigned long long* xcc_slots;
};
constexpr long long kCoopSentinel = 0x7ff8dead5eed0001LL;       // a quiet NaN with a payload of its own
template <int R, int T>
__device__ __forceinline__ void coop_steps(const Dense& A, CoopShared& sh, const Coop& C, double (&v)[R][kPanel], int c0, int c1, unsigned& active,
                                           int& np, int& step, bool& dead) {
    if constexpr (T < kPanel) {
        if (c0 + T >= c1 || dead) return;              // uniform over the grid
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, G = sh.G, part = sh.part;
        const bool plain = sh.plain != 0;
        const int row0 = part * R * kCoopThreads;
        if (wave == 1 + (T & 1)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the slot this wave reset two steps ago (see the exchange)
        double best = 0.0;
        int br = INT_MAX;
#pragma unroll
        for (int q = 0; q < R; q++) {
            const double a = ((active >> q) & 1u) ? fabs(v[q][T]) : 0.0;
            if (a > best) { best = a; br = row0 + q * kCoopThreads + tid; }       // rows ascend with q: the first maximum stays
        }
        wave_argmax(best, br);
        if (lane == 0) { sh.red_v[wave] = best; sh.red_r[wave] = br; }
        __syncthreads();
        double bv = 0.0;
        int rr = INT_MAX;
#pragma unroll
        for (int w = 0; w < kCoopThreads / 64; w++) take_larger(bv, rr, sh.red_v[w], sh.red_r[w]);
        if (!(bv > 0.0)) { bv = 0.0; rr = INT_MAX; }       // (no candidate, or not a number: never a pivot)
        if (rr != INT_MAX && (rr - row0) % kCoopThreads == tid) {
            const int qo = (rr - row0) / kCoopThreads;
#pragma unroll
            for (int q = 0; q < R; q++)
                if (q == qo) {
#pragma unroll
                    for (int t2 = 0; t2 < kPanel; t2++) sh.row[t2] = v[q][t2];
                }
        }
        __syncthreads();
        // ---- the exchange: a message IS its own flag.  FIVE sets of message slots are used in turn; a slot holds a sentinel (a NaN
        // pattern no candidate, row index or matrix entry is) until its workgroup writes the step's message there, word by word with
        // write-through stores and nothing else -- no drain, no counter: the readers poll every word past L1 until it is not the
        // sentinel.  A slot is reset three steps before its next use (it held the messages of step t - 2, and by the time a workgroup
        // has read all messages of step t everyone has published t - 1, i.e. finished reading t - 2); waves 1 and 2 take turns, and the
        // wave that reset a slot at step t waits for that store at the START of step t + 2 -- two steps later, so the wait is free --
        // in front of the barriers that precede the publication of step t + 2.  So whoever has seen a workgroup's message of step u
        // finds that workgroup's slot of step u + 1 reset or already written, never stale.
        const int set = (C.set0 + T) % 5;
        double* mine = C.slots + ((size_t)set * G + part) * kCoopSlot;
        if (wave == 0 && lane < kCoopSlot) {
            const double x = lane == 0 ? bv : lane == 1 ? __longlong_as_double((long long)rr) : sh.row[lane - 2];
            if (plain) __hip_atomic_store(mine + lane, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);     // stays in the XCD's L2
            else __hip_atomic_store(mine + lane, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);               // write-through
        }
        const double* all = C.slots + (size_t)set * G * kCoopSlot;
        int gone = 0;
        {
            // all of a thread's words are requested at once (independent loads: one round trip); only those still holding the
            // sentinel are asked for again
            constexpr int kPer = (kCoopMaxG * kCoopSlot + kCoopThreads - 1) / kCoopThreads;
            const int nw = G * kCoopSlot;
            double x[kPer];
#pragma unroll
            for (int k = 0; k < kPer; k++) {
                const int e = tid + k * kCoopThreads;
                x[k] = e < nw ? __hip_atomic_load(all + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
            }
            int spins = 0;
            for (;;) {
                bool pending = false;
#pragma unroll
                for (int k = 0; k < kPer; k++) pending |= __double_as_longlong(x[k]) == kCoopSentinel;
                if (!pending) break;
                __builtin_amdgcn_s_sleep(1);
                if (++spins > kCoopSpinLimit || ((spins & 1023) == 0 && __hip_atomic_load(C.abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                    __hip_atomic_store(C.abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    gone = 1;
                    break;
                }
#pragma unroll
                for (int k = 0; k < kPer; k++)
                    if (__double_as_longlong(x[k]) == kCoopSentinel) x[k] = __hip_atomic_load(all + tid + k * kCoopThreads, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int k = 0; k < kPer; k++) {
                const int e = tid + k * kCoopThreads;
                if (e < nw) sh.slots[e] = x[k];
            }
        }
        if (gone) sh.abort = 1;
        __syncthreads();
        if (sh.abort) { dead = true; return; }
        if (wave == 1 + (T & 1) && lane < kCoopSlot) {
            double* ahead = C.slots + ((size_t)((set + 3) % 5) * G + part) * kCoopSlot;
            if (plain) __hip_atomic_store(ahead + lane, __longlong_as_double(kCoopSentinel), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else __hip_atomic_store(ahead + lane, __longlong_as_double(kCoopSentinel), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // ---- the same winner everywhere
        double wv = lane < G ? sh.slots[lane * kCoopSlot] : 0.0;
        int wr = lane < G ? (int)__double_as_longlong(sh.slots[lane * kCoopSlot + 1]) : INT_MAX;
        int wg = lane;
        if (!(wv > 0.0)) { wv = 0.0; wr = INT_MAX; }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const double ov = __shfl_xor(wv, d, 64);
            const int orr = __shfl_xor(wr, d, 64);
            const int og = __shfl_xor(wg, d, 64);
            if (ov > wv || (ov == wv && orr < wr)) { wv = ov; wr = orr; wg = og; }
        }
        static_assert(kCoopMaxG <= 64, "the winner is combined over the 64 lanes of a wavefront");
        wv = __shfl(wv, 0, 64); wr = __shfl(wr, 0, 64); wg = __shfl(wg, 0, 64);
        const bool dependent = wr == INT_MAX || !(wv >= A.abstol) || wv == 0.0;
        const int pr = dependent ? -1 : wr;
        if (part == 0 && tid == 0) {
            if (dependent) A.bcstep[c0 + T] = -1;
            else {
                A.brstep[pr] = step;
                A.bcstep[c0 + T] = step;
                A.prow[np] = pr;
                A.pcol[np] = c0 + T;
            }
        }
        if (pr >= 0) {
            const double* su = sh.slots + wg * kCoopSlot + 2;
            if (pr >= row0 && pr < row0 + R * kCoopThreads && (pr - row0) % kCoopThreads == tid) active &= ~(1u << ((pr - row0) / kCoopThreads));
            np++; step++;
            const double piv = su[T];
#pragma unroll
            for (int q = 0; q < R; q++)
                if ((active >> q) & 1u) {
                    const double l = v[q][T] / piv;
                    v[q][T] = l;
#pragma unroll
                    for (int t2 = T + 1; t2 < kPanel; t2++) {
                        const double u = su[t2];
                        if (c0 + t2 < c1 && u != 0.0) v[q][t2] -= l * u;
                    }
                }
        }
        // (sh.slots / sh.row / red_* are rewritten only after the next step's first barrier, which every thread reaches after this read)
        coop_steps<R, T + 1>(A, sh, C, v, c0, c1, active, np, step, dead);
    }
}
template <int R>
__global__ __launch_bounds__(kCoopThreads) __attribute__((amdgpu_waves_per_eu(1, 2))) void lu_panel_coop_kernel(Dense A, Coop C, int c0, int c1, const int* __restrict__ step_src) {
    __shared__ CoopShared sh;
    if (C.xcd_mode && (blockIdx.x & 7)) return;
    const int kb = A.kb, tid = threadIdx.x;
    const int part = C.xcd_mode ? blockIdx.x >> 3 : blockIdx.x, G = C.xcd_mode ? (gridDim.x + 7) >> 3 : gridDim.x;
    const int row0 = part * R * kCoopThreads;
    if (tid == 0) { sh.abort = 0; sh.part = part; sh.G = G; sh.plain = 0; }
    if (C.xcd_mode && tid < 64) {
        // the placement is an observation, not a contract (as for the one-XCD runs of the sweeps, sweep.hip): every participant
        // publishes the XCD it runs on and reads everybody else's; plain stores only if all agree -- all see the same ids and decide alike
        unsigned xcc = 0;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= 0xff;
        if (tid == 0) __hip_atomic_store(C.xcc_slots + part, ((unsigned long long)C.epoch << 32) | xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        bool same = true;
        for (int i = tid; i < G; i += 64) {
            unsigned long long w;
            int spins = 0;
            while (((w = __hip_atomic_load(C.xcc_slots + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32) != C.epoch) {
                __builtin_amdgcn_s_sleep(1);
                if (++spins > kCoopSpinLimit) { __hip_atomic_store(C.abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
            }
            same &= (unsigned)(w & 0xff) == xcc && (w >> 32) == C.epoch;
        }
        same = __all(same);
        if (tid == 0) sh.plain = same ? 1 : 0;
    }
    unsigned active = 0, have = 0;
    double v[R][kPanel];
#pragma unroll
    for (int q = 0; q < R; q++) {
        const int r = row0 + q * kCoopThreads + tid;
        if (r < kb) { have |= 1u << q; if (A.brstep[r] < 0) active |= 1u << q; }
#pragma unroll
        for (int t = 0; t < kPanel; t++) v[q][t] = (r < kb && c0 + t < c1) ? A.D[(size_t)(c0 + t) * kb + r] : 0.0;
    }
    __syncthreads();
    int np = 0;
    int step = step_src ? step_src[0] : A.bstep[0];       // (look-ahead: the count so far is in the other set)
    bool dead = false;
    coop_steps<R, 0>(A, sh, C, v, c0, c1, active, np, step, dead);
    if (dead) return;                                      // nothing was written: the host finds the abort flag
#pragma unroll
    for (int q = 0; q < R; q++)
        if ((have >> q) & 1u) {
            const int r = row0 + q * kCoopThreads + tid;
#pragma unroll
            for (int t = 0; t < kPanel; t++)
                if (c0 + t < c1) A.D[(size_t)(c0 + t) * kb + r] = v[q][t];
        }
    if (part == 0 && tid == 0) { A.bstep[0] = step; A.bstep[1] = np; A.bstep[3] = 0; }
}

// The panel's rows of U in the trailing columns: row prow[t] of column c2 receives the updates of the panel's
// earlier pivots, in pivot order.  One thread per trailing column.
// mode 0: the pivots of the last panel call, prow[0 .. bstep[1]) (one-level panels); 1: those of the last SUB-panel,
// prow[bstep[3] .. bstep[3] + bstep[1]); 2: all pivots of the outer panel, prow[0 .. bstep[3] + bstep[1]).  Columns [c1, cend).
__device__ __forceinline__ void panel_pivots(const Dense& A, int mode, int* first, int* np) {
    *first = mode == 1 ? A.bstep[3] : 0;
    *np = mode == 2 ? A.bstep[3] + A.bstep[1] : A.bstep[1];
}
__global__ __launch_bounds__(kBlock) void lu_panel_rows_kernel(Dense A, int c1, int cend, int mode, double* __restrict__ ubuf = nullptr, int ldu = 0) {
    __shared__ double l11[kPanel][kPanel];
    __shared__ int prow[kPanel];
    int first, np;
    panel_pivots(A, mode, &first, &np);
    A.prow += first; A.pcol += first;
    const int kb = A.kb;
    for (int e = threadIdx.x; e < kPanel * kPanel; e += kBlock) {
        const int t2 = e / kPanel, t = e % kPanel;
        l11[t2][t] = (t < t2 && t2 < np) ? A.D[(size_t)A.pcol[t] * kb + A.prow[t2]] : 0.0;
    }
    if (threadIdx.x < kPanel) prow[threadIdx.x] = threadIdx.x < np ? A.prow[threadIdx.x] : 0;
    __syncthreads();
    if (np == 0) return;
    IPXK_GRID_STRIDE(cc, cend - c1) {
        double* col = A.D + (size_t)(c1 + cc) * kb;
        double v[kPanel];
#pragma unroll
        for (int t = 0; t < kPanel; t++) v[t] = t < np ? col[prow[t]] : 0.0;
#pragma unroll
        for (int t = 0; t < kPanel; t++) {
            const double u = v[t];
            if (t < np && u != 0.0) {
#pragma unroll
                for (int t2 = t + 1; t2 < kPanel; t2++)
                    if (t2 < np) v[t2] -= l11[t2][t] * u;
            }
            // (keeps the LDS reads of the later pivots from being hoisted up here: all 496 at once need 256 registers and 684
            // bytes of scratch per lane -- the kernel took 38-54 us; with the fence 40 registers)
            asm volatile("" ::: "memory");
        }
#pragma unroll
        for (int t = 1; t < kPanel; t++)
            if (t < np) col[prow[t]] = v[t];
        if (ubuf) {                       // the finished rows of U, pivot by pivot, contiguous along the columns (MFMA trailing update)
#pragma unroll
            for (int t = 0; t < kPanel; t++) ubuf[(size_t)t * ldu + cc] = t < np ? v[t] : 0.0;
        }
    }
}

// Trailing update on the matrix cores (round 4): D[r][c] -= sum_t L[r][t] U[t][c] over the np <= 32 pivots of an outer
// panel as v_mfma_f64_16x16x4_f64 products, for bumps of more than kMfmaMinRows rows.  The transposed product is
// formed (A operand = U', from the compact copy the rows kernel leaves; B operand = L, a column of D per pivot), so that
// the lane index of a result runs along the ROWS of D: loads and stores of a tile are 128-byte segments of D's columns.
// A workgroup takes 64 rows x 64 columns, a wavefront 16 rows x 64 columns (L fragment loaded once, 8 k-steps).  Rows
// pivoted already keep their values (their entries are entries of U).  The sums are accumulated by the matrix unit
// (fused, k ascending): no longer the one-rounded-product-at-a-time arithmetic of the restatement -- the factors are
// judged by the stability estimate (src/lu_factorization.cc:87-127) and agree with the restatement's to ~1e-13.
typedef double lu_d4 __attribute__((ext_vector_type(4)));
// (look-ahead: the update of columns [c1, cend) may run while the next outer panel is being factorized; a row that panel pivots
// meanwhile carries a step >= this panel's count bstep[0] and is still live for THIS update.  ubuf's columns start at cu.)
__global__ __launch_bounds__(kBlock) void lu_trailing_mfma_kernel(Dense A, const double* __restrict__ ubuf, int ldu, int c1, int cend, int cu) {
    const int np = A.bstep[3] + A.bstep[1], kb = A.kb;
    if (np == 0) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int r = blockIdx.x * 64 + wave * 16 + li;               // this lane's row of D (B operand / result column)
    const int rc = min(r, kb - 1);
    const int rs = A.brstep[rc];
    const bool live = r < kb && (rs < 0 || rs >= A.bstep[0]);
    // all rows of the wavefront's 16 pivoted already: nothing to do
    if (__ballot(live) == 0ull) return;
    double lf[8];                                                 // L[r][t = 4 ks + lk]
#pragma unroll
    for (int ks = 0; ks < 8; ks++) {
        const int t = 4 * ks + lk;
        lf[ks] = t < np ? A.D[(size_t)A.pcol[t] * kb + rc] : 0.0;
    }
    const int cb = c1 + blockIdx.y * 64;
#pragma unroll
    for (int ct = 0; ct < 4; ct++) {
        const int c0 = cb + ct * 16;
        if (c0 >= cend) break;
        const int ca = min(c0 + li, cend - 1) - cu;               // A operand: column c0 + li of the trailing part
        lu_d4 acc;
#pragma unroll
        for (int q = 0; q < 4; q++) {                             // result q: column c0 + lk + 4 q, row r
            const int c = min(c0 + lk + 4 * q, cend - 1);
            acc[q] = A.D[(size_t)c * kb + rc];
        }
#pragma unroll
        for (int ks = 0; ks < 8; ks++) {
            const double u = -ubuf[(size_t)(4 * ks + lk) * ldu + ca];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(u, lf[ks], acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int c = c0 + lk + 4 * q;
            if (live && c < cend) A.D[(size_t)c * kb + r] = acc[q];
        }
    }
}

// Trailing update: D[r][c2] -= sum over the panel's pivots t (in order, one rounded product at a time) of
// multiplier[r][t] * U[t][c2], for the rows not pivoted yet.  64 x 64 tile per workgroup, 4 x 4 per thread.
__global__ __launch_bounds__(kBlock) void lu_trailing_kernel(Dense A, int c1, int cend, int mode) {
    __shared__ double Ls[kPanel][64];
    __shared__ double Us[kPanel][64];
    __shared__ int live[64];
    int first, np;
    panel_pivots(A, mode, &first, &np);
    A.prow += first; A.pcol += first;
    const int kb = A.kb;
    if (np == 0) return;
    const int r0 = blockIdx.x * 64, cb = c1 + blockIdx.y * 64;
    const int tid = threadIdx.x;
    for (int e = tid; e < kPanel * 64; e += kBlock) {
        const int t = e / 64, x = e % 64;
        const int r = r0 + x, c2 = cb + x;
        Ls[t][x] = (t < np && r < kb) ? A.D[(size_t)A.pcol[t] * kb + r] : 0.0;
        Us[t][x] = (t < np && c2 < cend) ? A.D[(size_t)c2 * kb + A.prow[t]] : 0.0;
    }
    if (tid < 64) live[tid] = (r0 + tid < kb && A.brstep[r0 + tid] < 0) ? 1 : 0;
    __syncthreads();
    // a thread's 4 x 4 entries in registers, the pivots in the outer loop: sixteen independent chains instead of one (each entry
    // still receives its products one at a time in pivot order, and none for a zero of U)
    const int tx = tid & 15, ty = tid >> 4;
    double acc[4][4];
    bool on[4][4];
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
        for (int a = 0; a < 4; a++) {
            const int xc = ty + 16 * b, xr = tx + 16 * a;
            on[a][b] = cb + xc < cend && live[xr];
            acc[a][b] = on[a][b] ? A.D[(size_t)(cb + xc) * kb + r0 + xr] : 0.0;
        }
    for (int t = 0; t < np; t++) {
        double l[4], u[4];
#pragma unroll
        for (int a = 0; a < 4; a++) l[a] = Ls[t][tx + 16 * a];
#pragma unroll
        for (int b = 0; b < 4; b++) u[b] = Us[t][ty + 16 * b];
#pragma unroll
        for (int b = 0; b < 4; b++)
#pragma unroll
            for (int a = 0; a < 4; a++) {
                const double next = acc[a][b] - l[a] * u[b];
                acc[a][b] = u[b] != 0.0 ? next : acc[a][b];
            }
    }
#pragma unroll
    for (int b = 0; b < 4; b++)
#pragma unroll
        for (int a = 0; a < 4; a++)
            if (on[a][b]) A.D[(size_t)(cb + ty + 16 * b) * kb + r0 + tx + 16 * a] = acc[a][b];
}

// The update of the rest of the outer panel, columns [c1, cend), by the pivots of the last SUB-panel, in one launch (before:
// lu_panel_rows_kernel mode 1 + lu_trailing_kernel mode 1).  Every workgroup (64 rows) forms the sub-panel's rows of U for those
// columns itself in LDS -- np <= 16 pivots x <= 28 columns, the arithmetic of lu_panel_rows_kernel -- and updates its rows with
// them; workgroup 0 leaves the rows of U in `usub` ([t][x], kPanel apart), and the next lu_panel_multi_kernel writes them to
// their places: written here, they would race with the other workgroups' reads of the rows as they were.
__global__ __launch_bounds__(kBlock) void lu_subpanel_update_kernel(Dense A, int c1, int cend, double* __restrict__ usub) {
    __shared__ double l11[kNarrowWideMax][kNarrowWideMax];
    __shared__ double Us[kNarrowWideMax][kPanel];
    __shared__ double Ls[kNarrowWideMax][64];
    __shared__ int prow[kNarrowWideMax];
    __shared__ int live[64];
    const int first = A.bstep[3], np = A.bstep[1], kb = A.kb, nc = cend - c1, tid = threadIdx.x;
    if (np == 0 || nc <= 0) return;
    A.prow += first; A.pcol += first;
    const int r0 = blockIdx.x * 64;
    for (int e = tid; e < np * np; e += kBlock) {
        const int t2 = e / np, t = e - t2 * np;
        l11[t2][t] = t < t2 ? A.D[(size_t)A.pcol[t] * kb + A.prow[t2]] : 0.0;
    }
    for (int e = tid; e < np * nc; e += kBlock) {
        const int t = e / nc, x = e - t * nc;
        Us[t][x] = A.D[(size_t)(c1 + x) * kb + A.prow[t]];
    }
    for (int e = tid; e < np * 64; e += kBlock) {
        const int t = e / 64, x = e & 63;
        Ls[t][x] = r0 + x < kb ? A.D[(size_t)A.pcol[t] * kb + r0 + x] : 0.0;
    }
    if (tid < np) prow[tid] = A.prow[tid];
    if (tid < 64) live[tid] = (r0 + tid < kb && A.brstep[r0 + tid] < 0) ? 1 : 0;
    __syncthreads();
    if (tid < nc) {                       // the rows of U of column c1 + tid, pivot after pivot
        for (int t = 0; t < np; t++) {
            const double u = Us[t][tid];
            if (u != 0.0)
                for (int t2 = t + 1; t2 < np; t2++) Us[t2][tid] -= l11[t2][t] * u;
        }
        if (blockIdx.x == 0)
            for (int t = 0; t < np; t++) usub[t * kPanel + tid] = Us[t][tid];
    }
    __syncthreads();
    // 64 rows x nc columns: a thread takes a row and every fourth column
    const int xr = tid & 63;
    if (!live[xr]) return;
    for (int xc = tid >> 6; xc < nc; xc += kBlock / 64) {
        double* d = A.D + (size_t)(c1 + xc) * kb + r0 + xr;
        double acc = *d;
        for (int t = 0; t < np; t++) {
            const double u = Us[t][xc];
            if (u != 0.0) acc -= Ls[t][xr] * u;
        }
        *d = acc;
    }
}

// ---- driver ---------------------------------------------------------------------------------------
enum { kHPivots = 0, kHCoopAbort = 2 };      // the pinned block after a factorization: bstep[0 .. 1], the cooperative panel's abort flag

// one sub-panel [c0, c1) of `width` columns, kPanel / width ... rows per thread
void launch_panel_multi(hipStream_t s, int width, const Dense& P, int c0, int c1, int first, const double* us, int c1o, const int* step_src) {
    const dim3 one(1), threads(kPanelThreads);
    if (width == kNarrowWide) hipLaunchKernelGGL((lu_panel_multi_kernel<2, kNarrowWide>), one, threads, 0, s, P, c0, c1, first, us, c1o, step_src);
    else if (width == kNarrow) hipLaunchKernelGGL((lu_panel_multi_kernel<4, kNarrow>), one, threads, 0, s, P, c0, c1, first, us, c1o, step_src);
    else if (width == kNarrowDeep) hipLaunchKernelGGL((lu_panel_multi_kernel<8, kNarrowDeep>), one, threads, 0, s, P, c0, c1, first, us, c1o, step_src);
    else if (width == kNarrowHuge) hipLaunchKernelGGL((lu_panel_multi_kernel<16, kNarrowHuge>), one, threads, 0, s, P, c0, c1, first, us, c1o, step_src);
    else hipLaunchKernelGGL((lu_panel_multi_kernel<32, kNarrowGiant>), one, threads, 0, s, P, c0, c1, first, us, c1o, step_src);
}

// one-level panels: up to kPanelThreads rows (a row per thread), or IPXK_LU_TWO_LEVEL=0
void one_level_panels(hipStream_t s, const Dense& A) {
    const int kb = A.kb;
    const int width = kb <= kPanelThreads ? kPanel : kb <= 2 * kPanelThreads ? kNarrowWide : kb <= 4 * kPanelThreads ? kNarrow : kPanel;
    for (int c0 = 0; c0 < kb; c0 += width) {
        const int c1 = std::min(kb, c0 + width);
        if (kb <= kPanelThreads) hipLaunchKernelGGL(lu_panel_small_kernel, dim3(1), dim3(kPanelThreads), 0, s, A, c0, c1);
        else if (kb <= 4 * kPanelThreads) launch_panel_multi(s, width, A, c0, c1, 1, nullptr, 0, nullptr);
        else hipLaunchKernelGGL(lu_panel_kernel, dim3(1), dim3(kPanelThreads), 0, s, A, c0, c1);
        if (c1 < kb) {
            hipLaunchKernelGGL(lu_panel_rows_kernel, dim3(grid_for(kb - c1)), dim3(kBlock), 0, s, A, c1, kb, 0);
            hipLaunchKernelGGL(lu_trailing_kernel, dim3((kb + 63) / 64, (kb - c1 + 63) / 64), dim3(kBlock), 0, s, A, c1, kb, 0);
        }
    }
}

// the look-ahead's second stream (under a CU mask that leaves P.free_cus units to the panel kernels) and its events
void create_late_stream(LuDenseWork& W, const LuPolicy& P) {
    uint32_t mask[8];
    for (int w = 0; w < 8; w++) mask[w] = 0xffffffffu;
    // (bit b of the mask = unit b / 8 of XCC b % 8, scripts/bench_cumask.hip; an XCC whose bits are all clear keeps all its units: the
    // default frees 4 units of every XCD.  Measured and not used: 16 / 24 units of XCC 0 alone for a one-XCD panel of 16 / 24
    // workgroups with two rows per thread -- workgroups go to the XCCs in turn whatever the mask says, so the late update's share
    // on XCC 0 crawls on what is left of it: 8000 rows 62.7 -> 82 / 106 ms, 12 000 rows 149 -> 205 / 324 ms)
    for (int b = 0; b < (P.xcc0 ? P.xcc0 : P.free_cus); b++) {
        const int bit = P.xcc0 ? 8 * b : P.spread ? (b % 8) * 32 + b / 8 : b;
        mask[bit / 32] &= ~(1u << (bit % 32));
    }
    if (P.free_cus > 0 && hipExtStreamCreateWithCUMask(&W.s2, 8, mask) != hipSuccess) {
        (void)hipGetLastError();               // (a device the mask does not fit: a plain stream -- correct, no overlap to speak of)
        W.s2 = nullptr;
    }
    if (!W.s2) IPXK_HIP(hipStreamCreateWithFlags(&W.s2, hipStreamNonBlocking));
    for (hipEvent_t* e : {&W.ev_rows[0], &W.ev_rows[1], &W.ev_trail[0], &W.ev_trail[1]})
        IPXK_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
}

// the cooperative panel's message slots (all sentinels) and its abort flag
void coop_prepare(hipStream_t s, LuDenseWork& W) {
    W.coop_slots.ensure((size_t)5 * kCoopMaxG * kCoopSlot); W.coop_bar.ensure(2);
    if (W.coop_xcc.size() < (size_t)kCoopMaxG) { W.coop_xcc.ensure((size_t)kCoopMaxG); IPXK_HIP(hipMemsetAsync(W.coop_xcc.get(), 0, kCoopMaxG * sizeof(unsigned long long), s)); }
    IPXK_HIP(hipMemsetAsync(W.coop_bar.get(), 0, 2 * sizeof(unsigned), s));
    hipLaunchKernelGGL(fill_kernel<u64>, dim3(8), dim3(kBlock), 0, s, (int64_t)5 * kCoopMaxG * kCoopSlot, (u64)kCoopSentinel,
                       reinterpret_cast<u64*>(W.coop_slots.get()));
}

// the outer panel [c0, c1o) by one launch of G cooperating workgroups (a step per column: c0 steps lie behind this panel)
void coop_panel(hipStream_t s, LuDenseWork& W, const Dense& P, int R, int G, bool one_xcd, int c0, int c1o, const int* step_src) {
    if (++W.coop_epoch == 0) ++W.coop_epoch;
    const Coop C{W.coop_slots.get(), c0 % 5, reinterpret_cast<int*>(W.coop_bar.get() + 1), one_xcd ? 1 : 0, W.coop_epoch, W.coop_xcc.get()};
    const int grid = one_xcd ? G * 8 : G;
    if (R == 1) hipLaunchKernelGGL((lu_panel_coop_kernel<1>), dim3(grid), dim3(kCoopThreads), 0, s, P, C, c0, c1o, step_src);
    else hipLaunchKernelGGL((lu_panel_coop_kernel<2>), dim3(grid), dim3(kCoopThreads), 0, s, P, C, c0, c1o, step_src);
}

// the outer panel [c0, c1o) sub-panel by sub-panel, each followed by its update of the rest of the outer panel
// (measured and dropped: the whole outer panel in ONE launch, the sub-panels' updates of the rest of the outer
// panel by that one workgroup too -- bit-identical, but one CU moves those kb x 28 columns at 50-100 GB/s:
// 228 ms at 8000 rows against 130 with the three launches per sub-panel below)
void subpanels(hipStream_t s, LuDenseWork& W, const Dense& P, int width, bool fused_sub, int c0, int c1o, const int* step_src) {
    const int kb = P.kb;
    for (int ci = c0; ci < c1o; ci += width) {
        const int ce = std::min(c1o, ci + width);
        launch_panel_multi(s, width, P, ci, ce, ci == c0 ? 1 : 0, fused_sub ? W.usub.get() : nullptr, c1o, step_src);
        if (ce == c1o) continue;
        if (fused_sub) {
            hipLaunchKernelGGL(lu_subpanel_update_kernel, dim3((kb + 63) / 64), dim3(kBlock), 0, s, P, ce, c1o, W.usub.get());
        } else {
            hipLaunchKernelGGL(lu_panel_rows_kernel, dim3(1), dim3(kBlock), 0, s, P, ce, c1o, 1);
            hipLaunchKernelGGL(lu_trailing_kernel, dim3((kb + 63) / 64, 1), dim3(kBlock), 0, s, P, ce, c1o, 1);
        }
    }
}

// LOOK-AHEAD (with the matrix cores; IPXK_LU_LOOKAHEAD=0: off): an outer panel's update of the NEXT outer panel's columns
// runs first, on this stream; its update of everything beyond runs on a second stream while the next outer panel is
// factorized here.  The outer panels use two sets of pivot lists / counters alternately (the late update still reads
// its own), a row the next panel pivots meanwhile stays live for the late update (step >= that panel's count), and the
// next panel's rows of U beyond its columns wait for the late update.  Every entry still receives each panel's update
// exactly once, panels in order: the same factors bit for bit.
// Outer panel k's update of the columns [c1o, kb); last_late: the last outer panel with a late update in flight (-1: none), returned anew.
int lookahead_update(hipStream_t s, LuDenseWork& W, const Dense& P, int k, int c1o, int last_late) {
    const int kb = P.kb;
    if (last_late >= 0) IPXK_HIP(hipStreamWaitEvent(s, W.ev_trail[last_late & 1], 0));      // the columns beyond are up to date
    hipLaunchKernelGGL(lu_panel_rows_kernel, dim3(grid_for(kb - c1o)), dim3(kBlock), 0, s, P, c1o, kb, 2, W.ubuf.get(), kb);
    IPXK_HIP(hipEventRecord(W.ev_rows[k & 1], s));
    const int cl = std::min(kb, c1o + kPanel);
    hipLaunchKernelGGL(lu_trailing_mfma_kernel, dim3((kb + 63) / 64, 1), dim3(kBlock), 0, s, P, W.ubuf.get(), kb, c1o, cl, c1o);
    if (cl == kb) return -1;
    IPXK_HIP(hipStreamWaitEvent(W.s2, W.ev_rows[k & 1], 0));
    hipLaunchKernelGGL(lu_trailing_mfma_kernel, dim3((kb + 63) / 64, (kb - cl + 63) / 64), dim3(kBlock), 0, W.s2, P, W.ubuf.get(), kb, cl, kb, c1o);
    IPXK_HIP(hipEventRecord(W.ev_trail[k & 1], W.s2));
    return k;
}

// two-level panels: an outer panel of kPanel columns (cooperating workgroups, or sub-panels in registers, R rows per thread),
// then the trailing matrix once per outer panel
void two_level_panels(hipStream_t s, LuDenseWork& W, const Dense& A, const LuPolicy& Pol) {
    const int kb = A.kb, width = Pol.subpanel_width(kb);
    const bool use_mfma = Pol.use_mfma(kb), lookahead = Pol.lookahead_at(kb), coop = Pol.coop, coop_xcd = Pol.coop_one_xcd(kb);
    const int coopR = Pol.coop_rows(kb), coopG = Pol.coop_groups(kb);
    if (use_mfma) W.ubuf.ensure((size_t)kPanel * kb);
    W.usub.ensure((size_t)kNarrowWideMax * kPanel);
    Dense Ap[2] = {A, A};
    Ap[1].bstep = A.bstep + kBstepSet; Ap[1].prow = A.prow + kPanel; Ap[1].pcol = A.pcol + kPanel;
    if (lookahead && !W.s2) create_late_stream(W, Pol);
    if (coop) coop_prepare(s, W);
    int k = 0, last_late = -1;                  // outer panel index; the last outer panel with a late update in flight
    for (int c0 = 0; c0 < kb; c0 += kPanel, k++) {
        const int c1o = std::min(kb, c0 + kPanel);
        const Dense& P = lookahead ? Ap[k & 1] : A;
        const int* step_src = (lookahead && k > 0) ? Ap[(k - 1) & 1].bstep : nullptr;
        if (coop) coop_panel(s, W, P, coopR, coopG, coop_xcd, c0, c1o, step_src);
        else subpanels(s, W, P, width, Pol.fused_sub, c0, c1o, step_src);
        if (c1o == kb) continue;
        if (lookahead) {
            last_late = lookahead_update(s, W, P, k, c1o, last_late);
        } else if (use_mfma) {
            hipLaunchKernelGGL(lu_panel_rows_kernel, dim3(grid_for(kb - c1o)), dim3(kBlock), 0, s, P, c1o, kb, 2, W.ubuf.get(), kb);
            hipLaunchKernelGGL(lu_trailing_mfma_kernel, dim3((kb + 63) / 64, (kb - c1o + 63) / 64), dim3(kBlock), 0, s, P, W.ubuf.get(), kb, c1o, kb, c1o);
        } else {
            hipLaunchKernelGGL(lu_panel_rows_kernel, dim3(grid_for(kb - c1o)), dim3(kBlock), 0, s, P, c1o, kb, 2);
            hipLaunchKernelGGL(lu_trailing_kernel, dim3((kb + 63) / 64, (kb - c1o + 63) / 64), dim3(kBlock), 0, s, P, c1o, kb, 2);
        }
    }
    if (last_late >= 0) IPXK_HIP(hipStreamWaitEvent(s, W.ev_trail[last_late & 1], 0));
    if (lookahead && k > 0 && ((k - 1) & 1))        // the counters of the last outer panel to where they are read
        IPXK_HIP(hipMemcpyAsync(A.bstep, A.bstep + kBstepSet, 2 * sizeof(int), hipMemcpyDeviceToDevice, s));
}

}  // namespace

int lu_dense_factorize(hipStream_t s, LuDenseWork& W, int kb, double abstol, const LuPolicy& P, int* h) {
    W.prow.ensure(2 * kPanel); W.pcol.ensure(2 * kPanel);
    const Dense A{kb, W.D.get(), W.brstep.get(), W.bcstep.get(), W.bstep.get(), W.prow.get(), W.pcol.get(), abstol};
    if (kb <= kPanelThreads || !P.two_level) one_level_panels(s, A);
    else two_level_panels(s, W, A, P);
    fetch(s, h + kHPivots, W.bstep.get(), 2);
    h[kHCoopAbort] = 0;
    if (W.coop_bar.size() >= 2) fetch(s, h + kHCoopAbort, W.coop_bar.get() + 1);
    IPXK_HIP(hipStreamSynchronize(s));
    if (h[kHCoopAbort]) throw Error(IPXK_E_HIP, "LU: the cooperative panel kernel gave up waiting for its workgroups (IPXK_LU_COOP=0 selects the one-workgroup panels)");
    return h[kHPivots];
}

}  // namespace ipxk
