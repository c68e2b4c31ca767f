// Row-gather SpMV for gfx950: out[r] = finish(init(r) (+|-) sum_p prod(x[idx[p]], val[p])).
//
// One kernel serves every sparse product on the path (A'y, A t, diag(A W A'),
// right-hand-side assembly, solution recovery, the dense-column SMW terms and
// N N') through small epilogue functors.  HBM-bound: per nonzero it moves a
// 4-byte index and an 8-byte value exactly once with coalesced loads (lane i
// reads element base+i), the x gather is served by L2 / Infinity Cache.
//
// Summation order inside a row is the storage order (the owning thread adds the
// row's LDS-staged products sequentially), which is the reference's order:
//   * pass 1 of NormalMatrix::_Apply, d += rhs[Ai[p]]*Ax[p] (normal_matrix.cc:69-70)
//   * pass 2 equals the reference's one-pass scatter because row i of the
//     row-wise copy lists columns in ascending order (normal_matrix.cc:65-74).
// Products are rounded before they are added (they pass through LDS and the
// library is built with -ffp-contract=off), like the reference's x86 -O2 build.
#pragma once

#include <type_traits>

#include "device_utils.hpp"
#include "internal.hpp"

namespace ipxk {

constexpr int kLdsDoubles = kChunkNnz + kChunkNnz / 32;

// +1 double of padding per 32: rows of equal length 8 (stride 64 B) would
// otherwise hit 4 of the 64 LDS banks 8 ways in the per-row read phase.
__device__ __forceinline__ int lds_slot(int q) { return q + (q >> 5); }

// ---- epilogues ---------------------------------------------------------------
// init(r) starts a row sum, finish(r, acc, dot) ends it: both read what they need where they need it.  The combine
// kernel wants a row's inputs in flight together with its partial sums, so an epilogue may add a two-phase form:
// `In load(r)` reads the inputs of row r into a struct In, init(in) and finish(r, in, acc, dot) then only compute
// and store -- the same expressions on the same values.  (No __restrict__ on the members: debug_single_pass passes
// y == out.)  EpiRow picks that form where an epilogue has it and init(r) / finish(r, ...) where it has not.
template <class Epi, class = void>
struct EpiRow {
    struct In {};
    static __device__ __forceinline__ In load(const Epi&, long long) { return In{}; }
    static __device__ __forceinline__ double init(const Epi& e, long long r, const In&) { return e.init((int)r); }
    static __device__ __forceinline__ void finish(const Epi& e, long long r, const In&, double acc, double& dot) { e.finish((int)r, acc, dot); }
};
template <class Epi>
struct EpiRow<Epi, std::void_t<typename Epi::In>> {
    using In = typename Epi::In;
    static __device__ __forceinline__ In load(const Epi& e, long long r) { return e.load(r); }
    static __device__ __forceinline__ double init(const Epi& e, long long, const In& in) { return e.init(in); }
    static __device__ __forceinline__ void finish(const Epi& e, long long r, const In& in, double acc, double& dot) { e.finish(r, in, acc, dot); }
};

struct ProdMul {
    static __device__ __forceinline__ double prod(double xg, double v) { return xg * v; }
};
// (v * w) * v, the evaluation order of diagonal_precond.cc:37
struct ProdSquareWeighted {
    static __device__ __forceinline__ double prod(double xg, double v) { return (v * xg) * v; }
};

// out[r] = acc * w[r]  (w == nullptr: out[r] = acc)
struct EpiScale : ProdMul {
    const double* w; double* out;
    static constexpr bool kNeg = false;
    __device__ __forceinline__ double init(int) const { return 0.0; }
    __device__ __forceinline__ void finish(int r, double acc, double&) const {
        out[r] = w ? acc * w[r] : acc;
    }
    struct In { double w; };
    __device__ __forceinline__ In load(long long r) const { return In{w ? w[r] : 0.0}; }
    __device__ __forceinline__ double init(const In&) const { return 0.0; }
    __device__ __forceinline__ void finish(long long r, const In& in, double acc, double&) const {
        out[r] = w ? acc * in.w : acc;
    }
};
// out[r] = y[r]*wI[r] + acc, dot += y[r]*out[r]   (wI == nullptr: no slack term)
struct EpiNormalRows : ProdMul {
    const double* wI; const double* y; double* out;
    static constexpr bool kNeg = false;
    __device__ __forceinline__ double init(int r) const { return wI ? y[r] * wI[r] : 0.0; }
    __device__ __forceinline__ void finish(int r, double acc, double& dot) const {
        out[r] = acc;
        dot += y[r] * acc;
    }
    struct In { double y, wI; };
    __device__ __forceinline__ In load(long long r) const { return In{y[r], wI ? wI[r] : 0.0}; }
    __device__ __forceinline__ double init(const In& in) const { return wI ? in.y * in.wI : 0.0; }
    __device__ __forceinline__ void finish(long long r, const In& in, double acc, double& dot) const {
        out[r] = acc;
        dot += in.y * acc;
    }
};
// out[r] = wI[r] + sum (v*w)*v
struct EpiDiagonal : ProdSquareWeighted {
    const double* wI; double* out;
    static constexpr bool kNeg = false;
    __device__ __forceinline__ double init(int r) const { return wI ? wI[r] : 0.0; }
    __device__ __forceinline__ void finish(int r, double acc, double&) const { out[r] = acc; }
};
// out[r] = (-b[r] + acc) + wI[r]*aI[r]          (kkt_solver_diag.cc:90-92)
struct EpiKktRhs : ProdMul {
    const double* b; const double* wI; const double* aI; double* out;
    static constexpr bool kNeg = false;
    __device__ __forceinline__ double init(int r) const { return -b[r]; }
    __device__ __forceinline__ void finish(int r, double acc, double&) const {
        out[r] = acc + wI[r] * aI[r];
    }
};
// out[j] = w[j]*(a[j] - acc)                     (kkt_solver_diag.cc:111-112)
struct EpiRecoverX : ProdMul {
    const double* w; const double* a; double* out;
    static constexpr bool kNeg = false;
    __device__ __forceinline__ double init(int) const { return 0.0; }
    __device__ __forceinline__ void finish(int j, double acc, double&) const {
        out[j] = w[j] * (a[j] - acc);
    }
};
// out[i] = b[i] - sum                            (kkt_solver_diag.cc:108-116)
struct EpiResidualRows : ProdMul {
    const double* b; double* out;
    static constexpr bool kNeg = true;
    __device__ __forceinline__ double init(int r) const { return b[r]; }
    __device__ __forceinline__ void finish(int r, double acc, double&) const { out[r] = acc; }
};
// out[r] = (rhs[r] - acc)/diag[r], dot += out[r]*rhs[r]   (diagonal_precond.cc:145-149)
struct EpiSmwRows : ProdMul {
    const double* rhs; const double* diag; double* out;
    static constexpr bool kNeg = false;
    __device__ __forceinline__ double init(int) const { return 0.0; }
    __device__ __forceinline__ void finish(int r, double acc, double& dot) const {
        const double d = rhs[r] - acc;
        const double l = d / diag[r];
        out[r] = l;
        dot += l * rhs[r];
    }
    struct In { double rhs, diag; };
    __device__ __forceinline__ In load(long long r) const { return In{rhs[r], diag[r]}; }
    __device__ __forceinline__ double init(const In&) const { return 0.0; }
    __device__ __forceinline__ void finish(long long r, const In& in, double acc, double& dot) const {
        const double d = in.rhs - acc;
        const double l = d / in.diag;
        out[r] = l;
        dot += l * in.rhs;
    }
};
// out[j] = mask[j] * scale2[j] * (a[j] - acc)    (kkt_solver_basis.cc:101-120,178-188)
struct EpiBasisColumns : ProdMul {
    const double* scale2;   // colscale^2 on nonbasic columns, 0 elsewhere
    const double* a; double* out;
    static constexpr bool kNeg = false;
    __device__ __forceinline__ double init(int) const { return 0.0; }
    __device__ __forceinline__ void finish(int j, double acc, double&) const {
        const double s = scale2[j];
        out[j] = s != 0.0 ? (a[j] - acc) * s : 0.0;
    }
};
// ---- the kernels ---------------------------------------------------------------
// Time-tiled row-gather SpMV (layout: internal.hpp, GatherMatrix).  Workgroup w of G
// co-resident workgroups walks the phases of its rows; all workgroups are in the same
// phase at (roughly) the same time, so the slice of x being gathered stays in L2.
//
// Three-stage software pipeline over chunks of kChunkNnz entries: while chunk k's
// products are staged in LDS and added to the row accumulators, the x gathers of chunk
// k+1 and the coalesced (idx,val,count) stream loads of chunk k+2 are in flight, so
// neither the HBM nor the L2 gather latency sits on the per-chunk critical path.
// LDS is double-buffered: one barrier per chunk.
constexpr int kPerThread = kChunkNnz / kBlock;

template <int RT>
struct ChunkLoad {          // stream loads of one chunk held in registers
    int c[kPerThread];
    double v[kPerThread];
    unsigned char cb[RT];   // entry counts of my RT rows in the step (valid when the chunk opens a step)
    int start, nn, first, step;
};

template <int RT>
__device__ __forceinline__ void issue_stream(const GatherView& M, int k, int kend, int w, int tid,
                                             ChunkLoad<RT>& L) {
    L.nn = 0; L.first = 0; L.step = 0; L.start = 0;
#pragma unroll
    for (int u = 0; u < RT; u++) L.cb[u] = 0;
    if (k >= kend) {
        // past the end: harmless indices so that the (unused) gathers stay in bounds
#pragma unroll
        for (int e = 0; e < kPerThread; e++) { L.c[e] = 0; L.v[e] = 0.0; }
        return;
    }
    L.start = M.chunk_start[k];
    const int info = M.chunk_info[k];
    L.nn = info & 0xffffff;
    L.first = info >> 30;
    L.step = M.chunk_step[k];
#pragma unroll
    for (int e = 0; e < kPerThread; e++) {
        const int qq = e * kBlock + tid;
        const int pp = L.start + (qq < L.nn ? qq : 0);
        L.c[e] = __builtin_nontemporal_load(M.idx + pp);
        L.v[e] = __builtin_nontemporal_load(M.val + pp);
    }
    if (L.first) {
        // thread t owns the rows t, t + kBlock, t + 2 kBlock, ... of the workgroup (strided ownership:
        // consecutive rows -> consecutive threads, so every chunk of a step keeps many threads busy
        // whether a row has its entries spread over all phases or concentrated in one)
#pragma unroll
        for (int u = 0; u < RT; u++) L.cb[u] = M.counts[(size_t)L.step * (kBlock * RT) + u * kBlock + tid];
    }
}

template <class Epi, int RT, bool MASKED = false>
__global__ __launch_bounds__(kBlock, 4) void spmv_phased_kernel(GatherView M, const double* __restrict__ x,
                                                             Epi epi, double* dot_partials,
                                                             const int* done) {
    if (done && *done) return;
    __shared__ double lds[2][kLdsDoubles];
    __shared__ double red[kBlock / 64 + 1];
    __shared__ int wave_total[2][RT][kBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int w = blockIdx.x;
    double dotpart = 0.0;
    if (M.stamps && tid == 0) {
        // tuning aid: where this workgroup runs (XCC_ID = hwreg 20, HW_ID = hwreg 4)
        const unsigned xcc = __builtin_amdgcn_s_getreg((20) | (0 << 6) | (31 << 11));
        const unsigned hw = __builtin_amdgcn_s_getreg((4) | (0 << 6) | (31 << 11));
        M.stamps[(size_t)M.Q * M.P * M.G + w] = ((unsigned long long)xcc << 32) | hw;
    }

    for (int q = 0; q < M.Q; q++) {
        const int wg_row0 = (q * M.G + w) * M.RWrows;
        const int row_end = min(M.nrows, wg_row0 + M.RWrows);   // rows of this workgroup
        double acc[RT];
#pragma unroll
        for (int u = 0; u < RT; u++) {
            const int r = wg_row0 + u * kBlock + tid;
            acc[u] = r < row_end ? epi.init(r) : 0.0;
        }

        const int kbeg = M.wg_chunk_ptr[q * M.G + w], kend = M.wg_chunk_ptr[q * M.G + w + 1];
        ChunkLoad<RT> cur, nxt;
        double xg[kPerThread];
        issue_stream<RT>(M, kbeg, kend, w, tid, cur);
        issue_stream<RT>(M, kbeg + 1, kend, w, tid, nxt);
#pragma unroll
        for (int e = 0; e < kPerThread; e++) {                      // gathers of chunk 0
            if (MASKED) xg[e] = cur.v[e] != 0.0 ? x[cur.c[e]] : 0.0;    // masked value array (trisolve.hip): no gather for a zero entry
            else xg[e] = x[cur.c[e]];
        }

        int buf = 0, step_n0 = 0;
        int cnt[RT], off[RT];      // my rows' entry counts and first positions within the current step
#pragma unroll
        for (int u = 0; u < RT; u++) { cnt[u] = 0; off[u] = 0; }
        __syncthreads();   // LDS buffers free (previous round)
        for (int k = kbeg; k < kend; k++) {
            if (M.stamps && tid == 0 && cur.first) M.stamps[cur.step] = wall_clock64();
            // stage the products of chunk k (waits for its gathers only)
#pragma unroll
            for (int e = 0; e < kPerThread; e++) {
                const int qq = e * kBlock + tid;
                if (qq < cur.nn) lds[buf][lds_slot(qq)] = Epi::prod(xg[e], cur.v[e]);
            }
            // gathers of chunk k+1, stream loads of chunk k+2
            const int cstart = cur.start, cnn = cur.nn, cfirst = cur.first;
            int incl[RT];
            if (cfirst) {
                // positions of my rows' segments: the step stores rows in order, row u*kBlock + t
                // belongs to thread t -> one scan over the threads per u
                step_n0 = cstart;
#pragma unroll
                for (int u = 0; u < RT; u++) {
                    cnt[u] = cur.cb[u];
                    int v = cnt[u];
#pragma unroll
                    for (int o = 1; o < 64; o <<= 1) {
                        const int t = __shfl_up(v, o, 64);
                        if (lane >= o) v += t;
                    }
                    incl[u] = v;
                    if (lane == 63) wave_total[buf][u][wave] = v;
                }
            }
#pragma unroll
            for (int e = 0; e < kPerThread; e++) {
                if (MASKED) xg[e] = nxt.v[e] != 0.0 ? x[nxt.c[e]] : 0.0;
                else xg[e] = x[nxt.c[e]];
            }
            cur = nxt;
            issue_stream<RT>(M, k + 2, kend, w, tid, nxt);
            __syncthreads();
            if (cfirst) {
                int base = 0;
#pragma unroll
                for (int u = 0; u < RT; u++) {
                    int before = 0, total = 0;
#pragma unroll
                    for (int ww = 0; ww < kBlock / 64; ww++) {
                        const int t = wave_total[buf][u][ww];
                        if (ww < wave) before += t;
                        total += t;
                    }
                    off[u] = base + before + incl[u] - cnt[u];
                    base += total;
                }
            }
            // add my rows' products that lie in this chunk, in storage order
            const int shift = cstart - step_n0;
#pragma unroll
            for (int u = 0; u < RT; u++) {
                const int pos0 = off[u] - shift;
                if (pos0 >= cnn || pos0 + cnt[u] <= 0) continue;
                // the part of the row's segment inside this chunk, four LDS reads in flight at a time,
                // added strictly in storage order
                const int lo = max(pos0, 0), hi = min(pos0 + cnt[u], cnn);
                for (int pos = lo; pos < hi; pos += 4) {
                    double t[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) t[j] = lds[buf][lds_slot(min(pos + j, hi - 1))];
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (pos + j < hi) acc[u] = Epi::kNeg ? acc[u] - t[j] : acc[u] + t[j];
                }
            }
            buf ^= 1;
        }
#pragma unroll
        for (int u = 0; u < RT; u++) {
            const int r = wg_row0 + u * kBlock + tid;
            if (r < row_end && !(M.row_long && M.row_long[r])) epi.finish(r, acc[u], dotpart);
        }
    }
    if (dot_partials) {
        const double d = block_reduce<SumOp>(dotpart, red);
        if (tid == 0) dot_partials[blockIdx.x] = d;
    }
}

// One segment of a long row per workgroup: strided per-thread sums, fixed block tree.
template <class Epi>
__global__ __launch_bounds__(kBlock) void spmv_long_kernel(GatherView M, const double* __restrict__ x,
                                                           const int* done) {
    if (done && *done) return;
    __shared__ double red[kBlock / 64 + 1];
    const int sgm = blockIdx.x;
    double acc = 0.0;
    for (int p = M.seg_p0[sgm] + threadIdx.x; p < M.seg_p1[sgm]; p += kBlock) {
        const double v = __builtin_nontemporal_load(M.lval + p);
        acc += Epi::prod(v != 0.0 ? x[M.lidx[p]] : 0.0, v);
    }
    acc = block_reduce<SumOp>(acc, red);
    if (threadIdx.x == 0) M.long_partials[sgm] = acc;
}

// Combines the segment sums of long rows in segment order and runs the epilogue;
// its dot contribution goes to dot_partials[dot_slot].
template <class Epi>
__global__ __launch_bounds__(kBlock) void spmv_long_fixup_kernel(GatherView M, Epi epi,
                                                                 double* dot_partials, int dot_slot,
                                                                 const int* done) {
    if (done && *done) return;
    __shared__ double red[kBlock / 64 + 1];
    double dotpart = 0.0;
    for (int l = threadIdx.x; l < M.nlong; l += kBlock) {
        const int r = M.long_row[l];
        double acc = epi.init(r);
        for (int s = M.long_slot[l]; s < M.long_slot[l + 1]; s++) {
            const double t = M.long_partials[s];
            acc = Epi::kNeg ? acc - t : acc + t;
        }
        epi.finish(r, acc, dotpart);
    }
    if (dot_partials) {
        const double d = block_reduce<SumOp>(dotpart, red);
        if (threadIdx.x == 0) dot_partials[dot_slot] = d;
    }
}

// ---- XCD-sliced tile layout (internal.hpp, SlicedMatrix) -------------------------
// One tile per workgroup: the tile's entries are streamed with coalesced loads (8 in flight per
// thread, gathers issued together), their products are staged in LDS, then every thread adds up
// the products of its 4 consecutive rows in storage order and writes the 4 partial sums (32 B).
// FUSED (one slice = the whole index space): no partial vectors and no combine launch; the thread
// starts each row from epi.init, adds the row's products in storage order (the reference's order,
// bit for bit) and applies epi.finish itself; the tile's dot partial goes to dot_partials[tile].
template <class Epi, int RPT, bool FUSED, bool MASKED = false>
__global__ __launch_bounds__(kBlock) void spmv_sliced_tile_kernel(SlicedView M, const double* __restrict__ x,
                                                                  Epi epi, double* dot_partials, const int* done) {
    if (done && *done) return;
    extern __shared__ double sl_prod[];
    __shared__ int wave_sum[kBlock / 64];
    __shared__ double red[kBlock / 64 + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // rows per thread: a thread's row counts are one 8-, 16- or 32-bit load
    static_assert(RPT == 1 || RPT == 2 || RPT == 4, "rows per thread");
    constexpr int R = kBlock * RPT;
    constexpr int U = 8;
    const int ntiles = M.nrb * M.nslices;
    double dotpart = 0.0;
    // sliced: one tile per workgroup (tile = blockIdx.x fixes the XCD); fused: a workgroup walks
    // tiles blockIdx.x, blockIdx.x + gridDim.x, ... so that the launch has at most kMaxPartials dot partials
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int s = tile % M.nslices, rb = tile / M.nslices;
        const unsigned e0 = M.tile_ptr[tile];
        const int ne = (int)(M.tile_ptr[tile + 1] - e0);
        const unsigned char* cbase = M.cnt + (size_t)tile * R;
        const unsigned c4 = RPT == 4 ? reinterpret_cast<const unsigned*>(cbase)[tid]
                          : RPT == 2 ? (unsigned)reinterpret_cast<const unsigned short*>(cbase)[tid]
                                     : (unsigned)cbase[tid];
        for (int base = 0; base < ne; base += kBlock * U) {
            int ci[U];
            double v[U], xg[U];
            // unpredicated loads (lanes past the end re-read the tile's last entry), so that all 2*U
            // stream loads and then all U gathers of a thread are in flight together
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int i = min(base + u * kBlock + tid, ne - 1);
                ci[u] = __builtin_nontemporal_load(M.idx + e0 + i);
                v[u] = __builtin_nontemporal_load(M.val + e0 + i);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (MASKED) xg[u] = v[u] != 0.0 ? x[ci[u]] : 0.0;   // masked value array (trisolve.hip): a zero entry needs no gather
                else xg[u] = x[ci[u]];
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int i = base + u * kBlock + tid;
                if (i < ne) sl_prod[lds_slot(i)] = Epi::prod(xg[u], v[u]);
            }
        }
        // exclusive scan of the per-thread entry counts -> first staged product of my rows
        const int mine = (int)((c4 & 255u) + ((c4 >> 8) & 255u) + ((c4 >> 16) & 255u) + (c4 >> 24));   // unused bytes are 0
        int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int nb = __shfl_up(incl, d, 64);
            if (lane >= d) incl += nb;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int p = incl - mine;
        for (int w = 0; w < wave; w++) p += wave_sum[w];
        if (FUSED) {
#pragma unroll
            for (int q = 0; q < RPT; q++) {
                const int cq = (int)((c4 >> (8 * q)) & 255u);
                const int r = rb * R + tid * RPT + q;
                if (r < M.nrows && !(M.row_long && M.row_long[r])) {
                    double acc = epi.init(r);
                    for (int kk = 0; kk < cq; kk++) {
                        const double t = sl_prod[lds_slot(p + kk)];
                        acc = Epi::kNeg ? acc - t : acc + t;
                    }
                    epi.finish(r, acc, dotpart);
                }
                p += cq;
            }
            __syncthreads();          // the staging buffer is reused by the next tile
            continue;
        }
        double out[RPT];
#pragma unroll
        for (int q = 0; q < RPT; q++) {
            const int cq = (int)((c4 >> (8 * q)) & 255u);
            double acc = 0.0;
            for (int kk = 0; kk < cq; kk++) acc += sl_prod[lds_slot(p + kk)];
            p += cq;
            out[q] = acc;
        }
        double* dst = M.partial + (size_t)s * M.nrows_pad + (size_t)rb * R + (size_t)tid * RPT;
        if (RPT == 1) {
            dst[0] = out[0];
        } else {
#pragma unroll
            for (int q = 0; q < RPT; q += 2) reinterpret_cast<double2*>(dst)[q / 2] = make_double2(out[q], out[q + 1 < RPT ? q + 1 : q]);
        }
    }
    if (FUSED && dot_partials) {
        const double d = block_reduce<SumOp>(dotpart, red);
        if (tid == 0) dot_partials[blockIdx.x] = d;
    }
}

// ---- sorted fused tiles (internal.hpp, SortedMatrix) -------------------------------------------
// One workgroup of 256 threads walks tiles (row blocks) blockIdx.x, blockIdx.x + gridDim.x, ...  It streams a tile's entries in
// batches of 2048 (packed word + value, coalesced, non-temporal, 8 per thread in flight; the next batch's loads -- of this or
// the workgroup's next tile -- are issued while the gathers of the current one return), gathers x at ASCENDING addresses
// relative to the tile's smallest index (neighbouring lanes share lines: fewer L1->L2 requests than entries) and writes each
// product to its LDS slot (the entry's place in row order) -- batch after batch without a barrier, slots are distinct.  After
// ONE barrier the thread starts each of its RPT consecutive rows from epi.init, adds the row's products from consecutive
// slots in storage order (the reference's order, bit for bit as in the phased and fused layouts) and applies epi.finish
// itself.  The workgroup's dot partial goes to dot_partials[blockIdx.x].
template <class Epi, int RPT>
__global__ __launch_bounds__(kSortedThreads, kSortedThreads / 128) void spmv_sorted_fused_kernel(SortedView M, const double* __restrict__ x, Epi epi,
                                                                                           double* dot_partials, const int* done) {
    if (done && *done) return;
    extern __shared__ double so_prod[];
    __shared__ int wave_sum[kSortedThreads / 64];
    __shared__ double red[kSortedThreads / 64 + 1];
    static_assert(RPT == 1 || RPT == 2 || RPT == 4 || RPT == 8 || RPT == 16 || RPT == 32, "rows per thread");
    constexpr int U = 8;
    constexpr int kBatch = kSortedThreads * U;
    constexpr int RB = kSortedThreads * RPT;
    constexpr int CW = RPT >= 4 ? RPT / 4 : 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double dotpart = 0.0;
    unsigned pk[U];
    double v[U];
    auto stream = [&](int tile, int base) {
        const unsigned e0 = M.sub_ptr[tile];
        const int ne = (int)(M.sub_ptr[tile + 1] - e0);
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int i = min(base + u * kSortedThreads + tid, max(ne - 1, 0));
            pk[u] = __builtin_nontemporal_load(M.pack + e0 + i);
            v[u] = __builtin_nontemporal_load(M.val + e0 + i);
        }
    };
    if ((int)blockIdx.x < M.nrb) stream(blockIdx.x, 0);
    for (int tile = blockIdx.x; tile < M.nrb; tile += gridDim.x) {
        const int ne = (int)(M.sub_ptr[tile + 1] - M.sub_ptr[tile]);
        const double* __restrict__ xs = x + M.xmin[tile];
        unsigned cw[CW];
        {
            const unsigned char* cbase = M.cnt + (size_t)tile * RB + (size_t)tid * RPT;
            if (RPT >= 4) {
#pragma unroll
                for (int q = 0; q < CW; q++) cw[q] = reinterpret_cast<const unsigned*>(cbase)[q];
            } else if (RPT == 2) {
                cw[0] = (unsigned)reinterpret_cast<const unsigned short*>(cbase)[0];
            } else {
                cw[0] = (unsigned)cbase[0];
            }
        }
        for (int base = 0; base < ne || base == 0; base += kBatch) {
            double xg[U], vv[U];
            unsigned slot[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const unsigned off = pk[u] & ((1u << kSortedOffBits) - 1u);
                slot[u] = pk[u] >> kSortedOffBits;
                vv[u] = v[u];
                xg[u] = xs[off];
            }
            if (base + kBatch < ne) stream(tile, base + kBatch);
            else if (tile + (int)gridDim.x < M.nrb) stream(tile + gridDim.x, 0);
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int i = base + u * kSortedThreads + tid;
                if (i < ne) so_prod[lds_slot((int)slot[u])] = Epi::prod(xg[u], vv[u]);
            }
        }
        int mine = 0;
#pragma unroll
        for (int q = 0; q < CW; q++) mine += (int)((cw[q] & 255u) + ((cw[q] >> 8) & 255u) + ((cw[q] >> 16) & 255u) + (cw[q] >> 24));
        int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int nb = __shfl_up(incl, d, 64);
            if (lane >= d) incl += nb;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        int p = incl - mine;
        for (int w = 0; w < wave; w++) p += wave_sum[w];
#pragma unroll
        for (int q = 0; q < RPT; q++) {
            const int cq = (int)((cw[q / 4] >> (8 * (q & 3))) & 255u);
            const int r = tile * RB + tid * RPT + q;
            if (r < M.nrows && !(M.row_long && M.row_long[r])) {
                double acc = epi.init(r);
                for (int kk = 0; kk < cq; kk += 4) {           // four LDS reads in flight, added strictly in storage order
                    double t[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) t[j] = so_prod[lds_slot(p + min(kk + j, cq - 1))];
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (kk + j < cq) acc = Epi::kNeg ? acc - t[j] : acc + t[j];
                }
                epi.finish(r, acc, dotpart);
            }
            p += cq;
        }
        __syncthreads();                  // the staging buffer and wave_sum are reused by the next tile
    }
    if (dot_partials) {
        double d = dotpart;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) d += __shfl_down(d, o, 64);
        if (lane == 0) red[wave] = d;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int w = 0; w < kSortedThreads / 64; w++) t += red[w];
            dot_partials[blockIdx.x] = t;
        }
    }
}

// ---- accumulated tiles (internal.hpp, AccMatrix) -----------------------------------------------
// One workgroup of 512 threads per tile; the RB row sums live in LDS.  Batch after batch (at most 2048
// entries, 4 per thread): packed word + value streamed non-temporally, x gathered at ascending addresses (neighbouring
// lanes share lines), one barrier, one ds_add_f64 per entry -- the layout guarantees that a batch holds at most one
// entry of a row, so the adds of a batch hit distinct addresses and a row is summed in batch order.  The stream loads
// of batch k+1 are in flight while the gathers of batch k return.
//
// The pipeline of the two one-tile kernels below (the sliced form, one tile per (row block, slice), and the FUSED form): the
// batches [b0, b0 + nb) of a tile, gathered from xs (the slice's, or the tile window's, first element of x), added to
// ac_sum[0 .. M.RB), which starts from init(row in the tile); NEG: the products are subtracted.  On return every add is done
// and a barrier has passed.
struct AccRowsFromZero {
    __device__ double operator()(int) const { return 0.0; }
};
template <class Epi>
struct AccRowsFromEpi {             // rows r0 .. of the product start from the epilogue's value (padding rows: 0)
    const Epi& epi;
    int r0, nrows;
    __device__ double operator()(int r) const { return r0 + r < nrows ? epi.init(r0 + r) : 0.0; }
};
template <class Prod, bool NEG, class Init>
__device__ __forceinline__ void acc_tile_pipeline(const AccView& M, const double* __restrict__ xs, unsigned b0, int nb, Init init) {
    extern __shared__ double ac_sum[];
    constexpr int U = kAccPerThread, T = kAccThreads;
    const int tid = threadIdx.x;
    // first entry of batch k of this tile (wave-uniform: scalar loads), fetched well ahead of its use
    auto first = [&](int k) -> unsigned { return M.bptr[b0 + min(k, nb)]; };
    constexpr int NE = 6;
    unsigned e[NE];                       // e[i] = first(k + i) for the current batch k
#pragma unroll
    for (int i = 0; i < NE; i++) e[i] = first(i);
    // Three-stage software pipeline over the batches: while the products of batch k are added to the row sums, the
    // gathers of batch k + 1 and the stream loads of batches k + 2 and k + 3 are in flight -- an iteration waits only for
    // loads issued a whole iteration earlier (the iteration time was one dependent round trip stream -> gather before:
    // 2 us per batch of 2048 entries).  Three stream buffers and two gather buffers rotate; the loop is unrolled six times.
    unsigned pk[3][U];
    double v[3][U], xg[2][U];
    auto stream = [&](unsigned (&pkb)[U], double (&vb)[U], unsigned e0, unsigned e1) {       // entries [e0, e1) of a batch (none: e0 == e1)
        const int ne = (int)(e1 - e0);
        if (ne <= 0) return;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int i = min(u * T + tid, ne - 1);
            pkb[u] = __builtin_nontemporal_load(M.pack + e0 + i);
            vb[u] = __builtin_nontemporal_load(M.val + e0 + i);
        }
    };
    auto gather = [&](double (&xgb)[U], const unsigned (&pkb)[U]) {
#pragma unroll
        for (int u = 0; u < U; u++) xgb[u] = xs[pkb[u] & ((1u << kSortedOffBits) - 1u)];
    };
#pragma unroll
    for (int d = 0; d < 3; d++) {
#pragma unroll
        for (int u = 0; u < U; u++) { pk[d][u] = 0u; v[d][u] = 0.0; }
        stream(pk[d], v[d], e[d], e[d + 1]);
    }
    // (the rows are started here, behind the prologue's stream loads and in front of the first gather, which waits for them)
    for (int r = tid; r < M.RB; r += T) ac_sum[r] = init(r);
    if (nb > 0) gather(xg[0], pk[0]);
    for (int k0 = 0; k0 < nb; k0 += 6) {
#pragma unroll
        for (int d = 0; d < 6; d++) {
            const int k = k0 + d;
            if (k < nb) {
                const int ne = (int)(e[1] - e[0]);
                if (k + 1 < nb) gather(xg[(d + 1) & 1], pk[(d + 1) % 3]);          // batch k + 1
                const unsigned enew = first(k + NE);
                __syncthreads();                  // the adds of the previous batch (first batch: the rows' start values) are done
                // (a plain read-modify-write -- the rows of a batch are distinct -- measured 3 % slower than ds_add_f64)
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (u * T + tid < ne) {
                        const double p = Prod::prod(xg[d & 1][u], v[d % 3][u]);
                        __hip_atomic_fetch_add(ac_sum + (pk[d % 3][u] >> kSortedOffBits), NEG ? -p : p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                stream(pk[d % 3], v[d % 3], e[3], e[4]);               // batch k + 3 into the buffer just emptied
#pragma unroll
                for (int i = 0; i + 1 < NE; i++) e[i] = e[i + 1];
                e[NE - 1] = enew;
            }
        }
    }
    __syncthreads();
}

// The sliced form: tile (row block rb, slice s); the row sums start from zero and leave as one partial vector per slice.
template <class Prod>
__global__ __launch_bounds__(kAccThreads) void spmv_acc_tile_kernel(AccView M, const double* __restrict__ x, const int* done) {
    if (done && *done) return;
    extern __shared__ double ac_sum[];
    constexpr int T = kAccThreads;
    const int tid = threadIdx.x;
    const int tile = blockIdx.x, s = tile % M.nslices, rb = tile / M.nslices;
    const double* __restrict__ xs = x + (size_t)s * M.slice_elems;
    const unsigned b0 = M.tile_batch[tile];
    acc_tile_pipeline<Prod, false>(M, xs, b0, (int)(M.tile_batch[tile + 1] - b0), AccRowsFromZero{});
    double* dst = M.partial + (size_t)s * M.nrows_pad + (size_t)rb * M.RB;
    for (int r = 2 * tid; r < M.RB; r += 2 * T) reinterpret_cast<double2*>(dst + r)[0] = make_double2(ac_sum[r], ac_sum[r + 1]);
}

// The PERSISTENT form of the tile kernel (launch_acc_tiles; IPXK_ACC_PERSIST=0 selects the kernel above).  The grid is a
// multiple of nslices (acc_persist_grid); workgroup w takes tiles w, w + G, w + 2G, ..., all of slice w % nslices, and runs
// the pipeline above over the concatenation of their STEPS (internal.hpp: a batch, or a tile's short tail batches taken as
// one batch of the pipeline and added one after the other), so the first stream loads and step records of the next tile
// are in flight while the current one finishes.  At a tile boundary each thread moves its row pairs (2 tid + 2 T j) from LDS
// into registers and zeroes them in place between two barriers; the parked sums leave as 16-byte stores, kAccParkPerBatch
// pairs after each of the next tile's batches (after that batch's stream loads, so that no s_waitcnt of the pipeline waits
// for them).  The last tile's sums leave from LDS at the end.  Workgroups never wait for each other; each row sum is the
// same sequence of ds_add_f64 as in the one-tile kernel, so the partials are equal bit for bit.
constexpr int kAccParkPairs = kAccMaxRows / (2 * kAccThreads);       // 16 row pairs (64 VGPRs) per thread
constexpr int kAccParkPerBatch = 2;
// WIDE: the entries come from the wide stream (internal.hpp) -- per thread and step three 16-byte loads, of its four entry words
// and its four values, instead of four 4-byte and four 8-byte ones (the same bytes in flight as 72 instead of 190 load
// instructions per CU).  Tp = acc_wide_threads(ne) threads take part in a step, thread t holds the sorted positions u Tp + t;
// the padding positions >= ne are gathered (word 0: the slice's first element) and never added.  Which thread adds an entry
// cannot change a sum (the rows of a batch are distinct), so every row sum is the same sequence of ds_add_f64 between the same
// barriers as without.
// HEAD (only with IPXK_ACC_HEAD=1: measured, it takes 0.4 us off the start of a launch and shows in no trace, profiles/
// acc_cold_start.txt): the launch starts from the head tables (internal.hpp).  A workgroup's first six step records, the walker's state behind
// them, *done and (WIDE) the nine stream loads of its first three steps are all issued before anything waits, from addresses
// formed of the kernel's arguments, blockIdx.x and threadIdx.x alone: one trip through the caches that the kernel boundary has
// emptied where the form without takes three dependent ones (tile_step -> steps / wide_start -> the wide stream).  Behind the
// prologue pk, v, q and the walker hold what they hold without HEAD and the loop is the same; `done` is looked at where the
// records arrive, so a spare launch has loaded what it does not use (from tables that stay valid).  Without the wide stream
// only the records come from the head; the stream loads of pack / val need them and keep a level of their own.
// WARM (the default, with or without HEAD; IPXK_ACC_WARM=0: off): as its first load each thread loads one 128-byte line of its workgroup's slice of x, line (blockIdx.x / 8) 512 + tid --
// where workgroups are placed on the XCDs in turn, the 32 workgroups of an XCD cover a slice of 2 MiB once, so that the first
// gathers do not find the XCD's L2 empty.  No result reads the value: placement only decides what the loads are worth.
typedef unsigned acc_u32x4 __attribute__((ext_vector_type(4)));
typedef double acc_f64x2 __attribute__((ext_vector_type(2)));
template <class Prod, bool WIDE, bool HEAD = false, bool WARM = false>
// (the step tables come as __restrict__ arguments: the partial stores of the loop would otherwise keep the compiler from
// reading them with scalar loads, and a vector load of a step record waits vmcnt(0) -- for the whole pipeline)
__global__ __launch_bounds__(kAccThreads) void spmv_acc_persist_kernel(AccView M, const unsigned* __restrict__ tile_step,
                                                                       const uint4* __restrict__ steps, const unsigned* __restrict__ wide_start,
                                                                       const acc_u32x4* __restrict__ wide, const double* __restrict__ x,
                                                                       const int* done, const unsigned* __restrict__ head,
                                                                       const acc_u32x4* __restrict__ head_wide) {
    // *done is fetched together with the first step-table loads and tested when they are there, not in a round trip of its
    // own in front of them (no `done`: a word of the table, which counts for nothing)
    int dn = 0;
    if constexpr (!HEAD) dn = *(done ? done : reinterpret_cast<const int*>(tile_step));
    extern __shared__ double ac_sum[];
    constexpr int U = kAccPerThread, T = kAccThreads, NP = kAccParkPairs, PB = kAccParkPerBatch;
    static_assert(NP % PB == 0, "parked pairs per batch");
    const int tid = threadIdx.x;
    const int ntiles = M.nrb * M.nslices, G = gridDim.x;
    const int s = blockIdx.x % M.nslices;                       // the same for every tile of the workgroup (G % nslices == 0)
    const double* __restrict__ xs = x + (size_t)s * M.slice_elems;
    double* const part = M.partial + (size_t)s * M.nrows_pad;
    [[maybe_unused]] double warm = 0.0;
    if constexpr (WARM) {
        // (clamped to the slice's last element that x has: no predicate; every slice starts inside x, launch_acc_tiles.  The
        // first vector load of the kernel: loads return in order, so whoever waits for a stream load has this one too)
        const long long left = (long long)M.xlen - (long long)s * M.slice_elems;
        const long long e = min((long long)((blockIdx.x >> 3) * T + tid) * 16, min((long long)M.slice_elems, left) - 1);
        warm = xs[e];
        __builtin_amdgcn_sched_barrier(0);
    }
    // walker over the workgroup's steps (wave-uniform: scalar loads; a record and the first word of the next one, the step's
    // end); an empty tile has no record and yields one empty step, so that its partial is written (zeros) like any other.
    // A step (internal.hpp) is entries [e0, e1) of one tile: streamed and gathered as one batch, added as the batches
    // [e0, c1) [c1, c2) [c2, c3) [c3, e1) with a barrier in front of every non-empty one after the first.
    // WIDE: w0 = the step's first unit of the wide stream (an empty step: 0)
    struct Step { unsigned e0, e1, c1, c2, c3, w0; int tile; };    // tile -1: past the workgroup's last tile
    int wt = blockIdx.x, wq = 0, wnb = 0;
    unsigned wb0 = 0;
    if constexpr (!HEAD) {
        if (wt < ntiles) { wb0 = tile_step[wt]; wnb = (int)(tile_step[wt + 1] - wb0); }
        if (done && dn) return;
    }
    auto next = [&]() -> Step {
        Step b{0u, 0u, 0u, 0u, 0u, 0u, -1};
        if (wt >= ntiles) return b;
        b.tile = wt;
        if (wnb > 0) {
            const uint4 r = steps[wb0 + wq];
            b.e0 = r.x; b.c1 = r.y; b.c2 = r.z; b.c3 = r.w; b.e1 = steps[wb0 + wq + 1].x;
            if (WIDE) b.w0 = wide_start[wb0 + wq];
        }
        if (++wq >= max(wnb, 1)) {
            wt += G; wq = 0;
            if (wt < ntiles) { wb0 = tile_step[wt]; wnb = (int)(tile_step[wt + 1] - wb0); }
        }
        return b;
    };
    constexpr int NE = 6;
    static_assert(NE == kAccHeadSteps, "the head holds the records the kernel keeps ahead");
    Step q[NE];                           // q[i] = step k + i for the current step k
    if constexpr (HEAD) {
        const unsigned* __restrict__ h = head + (size_t)blockIdx.x * kAccHeadWords;
#pragma unroll
        for (int i = 0; i < NE; i++) q[i] = Step{h[8 * i], h[8 * i + 1], h[8 * i + 2], h[8 * i + 3], h[8 * i + 4], h[8 * i + 5], (int)h[8 * i + 6]};
        wt = (int)h[8 * NE]; wq = (int)h[8 * NE + 1]; wb0 = h[8 * NE + 2]; wnb = (int)h[8 * NE + 3];
        dn = *(done ? done : reinterpret_cast<const int*>(head));
        __builtin_amdgcn_sched_barrier(0);          // (the scalar loads first, and nothing that waits for one in between)
    } else {
#pragma unroll
        for (int i = 0; i < NE; i++) q[i] = next();
    }
    unsigned pk[3][U];
    double v[3][U], xg[2][U];
    // The loads of an empty batch are issued too, from entry 0 and x[0] (the product has at least one entry and one column):
    // a load issued on one path only makes the compiler's s_waitcnt after the join count the other path's loads, and an
    // empty batch k + 1 then turned the adds of batch k into a wait for everything in flight (vmcnt(0)) in every batch.
    // WIDE: unit min(tid, Tp - 1) of each of the step's three planes; an empty step (Tp = 0, w0 = 0) loads unit 0 three times
    auto stream = [&](unsigned (&pkb)[U], double (&vb)[U], const Step& b) {     // entries [e0, e1) of a step
        const int ne = (int)(b.e1 - b.e0);
        if constexpr (WIDE) {
            static_assert(U == 4, "a unit of the wide stream holds a thread's four entries");
            const int tp = acc_wide_threads(ne);
            const acc_u32x4* src = wide + b.w0 + min(tid, max(tp - 1, 0));
            const acc_u32x4 w = __builtin_nontemporal_load(src);
            const acc_f64x2 v01 = __builtin_nontemporal_load(reinterpret_cast<const acc_f64x2*>(src + tp));
            const acc_f64x2 v23 = __builtin_nontemporal_load(reinterpret_cast<const acc_f64x2*>(src + 2 * tp));
            pkb[0] = w.x; pkb[1] = w.y; pkb[2] = w.z; pkb[3] = w.w;
            vb[0] = v01.x; vb[1] = v01.y; vb[2] = v23.x; vb[3] = v23.y;
        } else {
            const unsigned base = ne > 0 ? b.e0 : 0u;
            const int last = max(ne - 1, 0);
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int i = min(u * T + tid, last);
                pkb[u] = __builtin_nontemporal_load(M.pack + base + i);
                vb[u] = __builtin_nontemporal_load(M.val + base + i);
            }
        }
    };
    auto gather = [&](double (&xgb)[U], const unsigned (&pkb)[U], const Step& b) {
        const bool live = b.e1 > b.e0;
        const double* __restrict__ xb = live ? xs : x;
        const unsigned mask = live ? (1u << kSortedOffBits) - 1u : 0u;
#pragma unroll
        for (int u = 0; u < U; u++) xgb[u] = xb[pkb[u] & mask];
    };
    if constexpr (HEAD && WIDE) {
        static_assert(kAccHeadStreams == 3, "the prologue streams three steps");
        const acc_u32x4* hw = head_wide + (size_t)blockIdx.x * (kAccHeadStreams * 3 * T) + tid;
#pragma unroll
        for (int d = 0; d < 3; d++) {
            const acc_u32x4 w = __builtin_nontemporal_load(hw + (3 * d) * T);
            const acc_f64x2 v01 = __builtin_nontemporal_load(reinterpret_cast<const acc_f64x2*>(hw + (3 * d + 1) * T));
            const acc_f64x2 v23 = __builtin_nontemporal_load(reinterpret_cast<const acc_f64x2*>(hw + (3 * d + 2) * T));
            pk[d][0] = w.x; pk[d][1] = w.y; pk[d][2] = w.z; pk[d][3] = w.w;
            v[d][0] = v01.x; v[d][1] = v01.y; v[d][2] = v23.x; v[d][3] = v23.y;
        }
    }
    // `done` set: the workgroup has no steps.  Not a return, and plain arithmetic on the records once they are there: a branch
    // on *done (a select becomes one) is moved up in front of the prologue's loads, whatever fence stands between -- the
    // compiler knows that nothing writes a __restrict__ table -- and is a round trip of its own again.  A spare launch has
    // loaded what it does not use, from tables that stay valid.
    [[maybe_unused]] int stopmask = 0;
    if constexpr (HEAD) {
        __builtin_amdgcn_sched_barrier(0);
        stopmask = -(int)(done != nullptr && dn != 0);
#pragma unroll
        for (int i = 0; i < NE; i++) q[i].tile |= stopmask;
    }
    if constexpr (!(HEAD && WIDE)) {
#pragma unroll
        for (int d = 0; d < 3; d++) {
#pragma unroll
            for (int u = 0; u < U; u++) { pk[d][u] = 0u; v[d][u] = 0.0; }
            stream(pk[d], v[d], q[d]);
        }
    }
    for (int r = tid; r < (M.RB & ~stopmask); r += T) ac_sum[r] = 0.0;
    gather(xg[0], pk[0], q[0]);
    // (the oldest vector load: it is back when the gather above has its entry words, so this adds no wait of its own)
    if constexpr (WARM) asm volatile("" :: "v"(warm));
    int cur = q[0].tile;                  // the tile whose row sums are in LDS
    // parked row sums of the previous tile: park[0] is row pair prow of pdst, the next PB * pleft pairs follow 2 T rows apart
    double2 park[NP];
#pragma unroll
    for (int j = 0; j < NP; j++) park[j] = make_double2(0.0, 0.0);
    int pleft = 0, prow = 0;
    double* pdst = part;
    auto store_parked = [&]() {           // PB pairs, then the rest moves down (static register indices)
#pragma unroll
        for (int j = 0; j < PB; j++)
            if (prow + 2 * T * j < M.RB) reinterpret_cast<double2*>(pdst + prow + 2 * T * j)[0] = park[j];
#pragma unroll
        for (int j = 0; j + PB < NP; j++) park[j] = park[j + PB];
        prow += 2 * T * PB;
        pleft--;
    };
    while (q[0].tile >= 0) {
#pragma unroll
        for (int d = 0; d < 6; d++) {
            if (q[0].tile >= 0) {
                const int ne = (int)(q[0].e1 - q[0].e0);
                gather(xg[(d + 1) & 1], pk[(d + 1) % 3], q[1]);          // batch k + 1
                __syncthreads();                  // the adds of the previous batch (first batch: the zeroing) are done
                if (q[0].tile != cur) {           // first batch of the next tile: park the finished row sums, zero them
                    while (pleft > 0) store_parked();          // (the tile before had fewer batches than NP / PB)
#pragma unroll
                    for (int j = 0; j < NP; j++) {
                        const int r = 2 * tid + 2 * T * j;
                        if (r < M.RB) {
                            park[j] = make_double2(ac_sum[r], ac_sum[r + 1]);
                            ac_sum[r] = 0.0;
                            ac_sum[r + 1] = 0.0;
                        }
                    }
                    pdst = part + (size_t)(cur / M.nslices) * M.RB;
                    prow = 2 * tid;
                    pleft = NP / PB;
                    cur = q[0].tile;
                    __syncthreads();
                }
                // the step's first batch, then (a tile's short tail batches taken as one step) up to three more, each behind a
                // barrier of its own: the same ds_add_f64 between the same barriers as one batch per step.  The cuts are
                // scalars, the same in every wave; a step of one batch (c1 == e1) pays one scalar compare for the rest
                // (S: the distance of a thread's entries -- T, or the step's Tp with the wide stream, whose threads >= Tp hold none)
                const int n1 = (int)(q[0].c1 - q[0].e0);
                const int S = WIDE ? acc_wide_threads(ne) : T;
                const bool mine = !WIDE || tid < S;
#pragma unroll
                for (int u = 0; u < U; u++)
                    if (mine && u * S + tid < n1)
                        __hip_atomic_fetch_add(ac_sum + (pk[d % 3][u] >> kSortedOffBits), Prod::prod(xg[d & 1][u], v[d % 3][u]), __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                if (n1 < ne) {
                    int lo = n1, hi = (int)(q[0].c2 - q[0].e0), hi2 = (int)(q[0].c3 - q[0].e0);
#pragma unroll 1
                    for (int p = 1; p < kAccStepBatches && lo < ne; p++) {
                        __syncthreads();
#pragma unroll
                        for (int u = 0; u < U; u++)
                            if (mine && u * S + tid >= lo && u * S + tid < hi)
                                __hip_atomic_fetch_add(ac_sum + (pk[d % 3][u] >> kSortedOffBits), Prod::prod(xg[d & 1][u], v[d % 3][u]),
                                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        lo = hi; hi = hi2; hi2 = ne;
                    }
                }
                stream(pk[d % 3], v[d % 3], q[3]);               // step k + 3 into the buffer just emptied
                if (pleft > 0) store_parked();
#pragma unroll
                for (int i = 0; i + 1 < NE; i++) q[i] = q[i + 1];
                q[NE - 1] = next();
            }
        }
    }
    __syncthreads();
    while (pleft > 0) store_parked();
    if (cur >= 0) {
        double* dst = part + (size_t)(cur / M.nslices) * M.RB;
        for (int r = 2 * tid; r < M.RB; r += 2 * T) reinterpret_cast<double2*>(dst + r)[0] = make_double2(ac_sum[r], ac_sum[r + 1]);
    }
}

// ---- plain rows (small matrices) --------------------------------------------------------------
// The matrix as it is (the device's plain copy, layout_device.hip): 8 lanes per row, lane k takes entries k, k + 8, ...
// (coalesced: a wavefront reads 64 consecutive entries), the first lane of the group adds the products in storage
// order (the reference's order, bit for bit as in the phased and fused layouts).  No LDS, no barrier, no tile
// tables: a pass is three dependent round trips (row pointers -> entries -> gathers).  For matrices of a few hundred
// thousand entries, where a pass of the tiled layouts is 10 us of latency chains for 10 MB (C2: 50k x 100k).
template <class Epi>
__global__ __launch_bounds__(kBlock) void spmv_rowgroup_kernel(int nrows, const int* __restrict__ ptr, const int* __restrict__ idx,
                                                               const double* __restrict__ val, const unsigned char* __restrict__ row_long,
                                                               const double* __restrict__ x, Epi epi, double* dot_partials, const int* done) {
    if (done && *done) return;
    __shared__ double red[kBlock / 64 + 1];
    const int lane8 = threadIdx.x & 7, lane = threadIdx.x & 63, g0 = lane & ~7;
    double dotpart = 0.0;
    const int ngroups = (gridDim.x * kBlock) >> 3;
    for (int r = (blockIdx.x * kBlock + threadIdx.x) >> 3; r < nrows; r += ngroups) {
        const bool live = !(row_long && row_long[r]);
        const int p0 = ptr[r], p1 = live ? ptr[r + 1] : p0;
        double acc = lane8 == 0 ? epi.init(r) : 0.0;
        for (int p = p0; p < p1; p += 8) {
            const int q = p + lane8;
            const double prod = q < p1 ? Epi::prod(x[idx[q]], val[q]) : 0.0;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const double t = __shfl(prod, g0 + k, 64);
                if (p + k < p1) acc = Epi::kNeg ? acc - t : acc + t;
            }
        }
        if (live && lane8 == 0) epi.finish(r, acc, dotpart);
    }
    if (dot_partials) {
        const double d = block_reduce<SumOp>(dotpart, red);
        if (threadIdx.x == 0) dot_partials[blockIdx.x] = d;
    }
}

// The FUSED form: one slice, a tile per row block, gathered indices relative to the tile's smallest one; the row sums
// start from epi.init, the products are added batch by batch (ascending address = storage order of sorted rows) by
// acc_tile_pipeline and the kernel applies epi.finish itself; the tile's dot partial goes to dot_partials[tile].
template <class Epi>
__global__ __launch_bounds__(kAccThreads) void spmv_acc_fused_kernel(AccView M, const double* __restrict__ x, Epi epi, double* dot_partials,
                                                                     const int* done) {
    if (done && *done) return;
    extern __shared__ double ac_sum[];
    __shared__ double red[kAccThreads / 64];
    constexpr int T = kAccThreads;
    const int tid = threadIdx.x;
    const int tile = blockIdx.x;
    const double* __restrict__ xs = x + M.xmin[tile];
    const unsigned b0 = M.tile_batch[tile];
    const int r0 = tile * M.RB;
    acc_tile_pipeline<Epi, Epi::kNeg>(M, xs, b0, (int)(M.tile_batch[tile + 1] - b0), AccRowsFromEpi<Epi>{epi, r0, M.nrows});
    double dotpart = 0.0;
    for (int r = tid; r < M.RB; r += T)
        if (r0 + r < M.nrows) epi.finish(r0 + r, ac_sum[r], dotpart);
    if (dot_partials) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dotpart += __shfl_down(dotpart, o, 64);
        if ((tid & 63) == 0) red[tid >> 6] = dotpart;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int w = 0; w < T / 64; w++) t += red[w];
            dot_partials[tile] = t;
        }
    }
}

// out[r] = finish(init(r) (+|-) partial[0][r] (+|-) partial[1][r] ...), slices in ascending order.
// EARLY: thread t of workgroup w owns rows r = w*kBlock + t + j*gridDim.x*kBlock as before and takes them in groups of R.
// Nothing a group loads depends on anything else it loads, so all of it is issued before the first wait: *done, the long-row
// flags (LONG: the matrix has long rows), the epilogue's inputs (EpiRow) and the R x NS partial sums -- about 16 loads per
// thread, at rows clamped to the last one so that none needs a predicate; then the adds (ascending slice), the `done` test,
// and the epilogue and the store row by row (ascending row: the order of the thread's dot contributions).  NS is the slice
// count the geometry produced (1, 2, 4, 8: R = 2 at 8 slices, 4 otherwise); NS = 0 takes any count, R = 2 rows and the slices
// in blocks of 8.  Every thread runs the first group, with or without a live row in it, so the `done` test is uniform; *done
// is read with every group (it only changes between launches), which keeps that load among the group's, and without a
// `done` the word read is the first of the partial sums and counts for nothing.  A launch that finds `done` set has loaded
// what it does not use, from buffers that stay valid.  Two empty asm statements hold the order against the compiler: the
// first keeps the loads above everything that waits (it would sink them to their uses, behind the test), the second has
// every row's sum formed on every path, a dead row's too, before the first branch -- a way round the adds would carry the
// group's loads, still counted as outstanding, into the next group, whose s_waitcnt then wait for them between its own loads.
// !EARLY (IPXK_COMBINE_EARLY=0) is the form before: per row flag -> epilogue inputs -> one partial after the other, each
// waited for, then the store.  Same operations on the same values either way.
template <class Epi, int NS, bool EARLY, bool LONG>
__global__ __launch_bounds__(kBlock) void spmv_sliced_combine_kernel(SlicedView M, Epi epi, double* dot_partials,
                                                                     const int* done) {
    __shared__ double red[kBlock / 64 + 1];
    double dotpart = 0.0;
    if constexpr (EARLY) {
        using Row = EpiRow<Epi>;
        constexpr int B = NS ? NS : 8, R = B == 8 ? 2 : 4;
        const int ns = NS ? NS : M.nslices;
        const long long stride = (long long)gridDim.x * kBlock, last = M.nrows - 1;
        const int* const dword = done ? done : reinterpret_cast<const int*>(M.partial);
        long long r0 = blockIdx.x * kBlock + threadIdx.x;
        if (M.nrows <= 0) {
            if (done && *done) return;
        } else do {
            long long rc[R];
            unsigned char lg[R];
            typename Row::In in[R];
            double t[R][B];
            const int dn = __hip_atomic_load(dword, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int j = 0; j < R; j++) {
                rc[j] = min(r0 + j * stride, last);
                lg[j] = LONG ? M.row_long[rc[j]] : (unsigned char)0;
            }
#pragma unroll
            for (int j = 0; j < R; j++) in[j] = Row::load(epi, rc[j]);
#pragma unroll
            for (int j = 0; j < R; j++)
#pragma unroll
                for (int u = 0; u < B; u++) t[j][u] = __builtin_nontemporal_load(M.partial + (size_t)min(u, ns - 1) * M.nrows_pad + rc[j]);
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);          // (nor may the instruction scheduler move a wait in between the loads)
            double acc[R];
            bool live[R];
#pragma unroll
            for (int j = 0; j < R; j++) {
                live[j] = r0 + j * stride <= last && !lg[j];       // (a long row is finished by the long-row fix-up kernel)
                acc[j] = live[j] ? Row::init(epi, rc[j], in[j]) : 0.0;
            }
            for (int s0 = 0; s0 < ns; s0 += B) {
                if (s0 > 0) {                                       // NS == 0 and more than 8 slices: the next block of them
#pragma unroll
                    for (int j = 0; j < R; j++)
#pragma unroll
                        for (int u = 0; u < B; u++) t[j][u] = __builtin_nontemporal_load(M.partial + (size_t)min(s0 + u, ns - 1) * M.nrows_pad + rc[j]);
                }
#pragma unroll
                for (int j = 0; j < R; j++)
#pragma unroll
                    for (int u = 0; u < B; u++)
                        if (NS || s0 + u < ns) acc[j] = Epi::kNeg ? acc[j] - t[j][u] : acc[j] + t[j][u];
            }
#pragma unroll
            for (int j = 0; j < R; j++) asm volatile("" : "+v"(acc[j]));
            if (done && dn) return;
#pragma unroll
            for (int j = 0; j < R; j++)
                if (live[j]) Row::finish(epi, rc[j], in[j], acc[j], dotpart);
            r0 += R * stride;
        } while (r0 <= last);
    } else {
        if (done && *done) return;
        for (int r = blockIdx.x * kBlock + threadIdx.x; r < M.nrows; r += gridDim.x * kBlock) {
            if (M.row_long && M.row_long[r]) continue;       // finished by the long-row fix-up kernel
            double acc = epi.init(r);
            for (int s = 0; s < M.nslices; s++) {
                const double t = __builtin_nontemporal_load(M.partial + (size_t)s * M.nrows_pad + r);
                acc = Epi::kNeg ? acc - t : acc + t;
            }
            epi.finish(r, acc, dotpart);
        }
    }
    if (dot_partials) {
        const double d = block_reduce<SumOp>(dotpart, red);
        if (threadIdx.x == 0) dot_partials[blockIdx.x] = d;
    }
}

// IPXK_COMBINE_EARLY=0: the combine kernel in the form it had before its loads were issued ahead of the first add (read
// once per process; tests/test_gpu_combine_loads.py compares the two)
inline bool combine_early() {
    static const bool setting = [] { const char* e = getenv("IPXK_COMBINE_EARLY"); return !e || atoi(e) != 0; }();
    return setting;
}

inline bool combine_generic() {
    static const bool setting = [] { const char* e = getenv("IPXK_COMBINE_GENERIC"); return e && atoi(e) != 0; }();
    return setting;
}

// The one launch of the combine kernel: on combine_grid_for(V.nrows) workgroups, the instantiation for V.nslices and for
// whether the matrix has long rows.  IPXK_COMBINE_GENERIC=1 (tests) runs the form for any slice count whatever the count.
template <class Epi, bool LONG>
inline void launch_combine_ns(const SlicedView& V, const Epi& epi, double* dot_partials, const int* done, hipStream_t s) {
    const dim3 grid(combine_grid_for(V.nrows)), block(kBlock);
    switch (combine_generic() ? 0 : V.nslices) {
        case 1: hipLaunchKernelGGL((spmv_sliced_combine_kernel<Epi, 1, true, LONG>), grid, block, 0, s, V, epi, dot_partials, done); break;
        case 2: hipLaunchKernelGGL((spmv_sliced_combine_kernel<Epi, 2, true, LONG>), grid, block, 0, s, V, epi, dot_partials, done); break;
        case 4: hipLaunchKernelGGL((spmv_sliced_combine_kernel<Epi, 4, true, LONG>), grid, block, 0, s, V, epi, dot_partials, done); break;
        case 8: hipLaunchKernelGGL((spmv_sliced_combine_kernel<Epi, 8, true, LONG>), grid, block, 0, s, V, epi, dot_partials, done); break;
        default: hipLaunchKernelGGL((spmv_sliced_combine_kernel<Epi, 0, true, LONG>), grid, block, 0, s, V, epi, dot_partials, done); break;
    }
}
template <class Epi>
inline void launch_combine(const SlicedView& V, const Epi& epi, double* dot_partials, const int* done, hipStream_t s) {
    if (!combine_early())
        hipLaunchKernelGGL((spmv_sliced_combine_kernel<Epi, 0, false, false>), dim3(combine_grid_for(V.nrows)), dim3(kBlock), 0, s, V, epi,
                           dot_partials, done);
    else if (V.row_long) launch_combine_ns<Epi, true>(V, epi, dot_partials, done, s);
    else launch_combine_ns<Epi, false>(V, epi, dot_partials, done, s);
}

// IPXK_ACC_WARM=0: the persistent kernel without the load that warms the slice (read once per process; A/B runs and the tests)
inline bool acc_warm_on() {
    static const bool setting = [] { const char* e = getenv("IPXK_ACC_WARM"); return !e || atoi(e) != 0; }();
    return setting;
}

// The tile kernel of the accumulated tiles (every unmasked product, nmatrix.hip's N N' passes too): the persistent kernel on
// acc_persist_grid workgroups (at most one per tile), or one workgroup per tile when IPXK_ACC_PERSIST=0.
template <class Prod>
inline void launch_acc_tiles(const AccView& W, const double* x, const int* done, hipStream_t s) {
    static bool lds_attr_set = false;       // per instantiation: dynamic LDS beyond 64 KB has to be allowed once
    if (!lds_attr_set) {
        for (const void* f : {reinterpret_cast<const void*>(spmv_acc_tile_kernel<Prod>),
                              reinterpret_cast<const void*>(spmv_acc_persist_kernel<Prod, false>),
                              reinterpret_cast<const void*>(spmv_acc_persist_kernel<Prod, true>),
                              reinterpret_cast<const void*>(spmv_acc_persist_kernel<Prod, false, false, true>),
                              reinterpret_cast<const void*>(spmv_acc_persist_kernel<Prod, true, false, true>),
                              reinterpret_cast<const void*>(spmv_acc_persist_kernel<Prod, false, true, false>),
                              reinterpret_cast<const void*>(spmv_acc_persist_kernel<Prod, true, true, false>),
                              reinterpret_cast<const void*>(spmv_acc_persist_kernel<Prod, false, true, true>),
                              reinterpret_cast<const void*>(spmv_acc_persist_kernel<Prod, true, true, true>)})
            IPXK_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kAccMaxRows * sizeof(double))));
        lds_attr_set = true;
    }
    const size_t lds = (size_t)W.RB * sizeof(double);
    const int ntiles = W.nrb * W.nslices, G = acc_persist_grid(W.nslices);
    const dim3 pgrid(std::min(G, ntiles));
    // WARM unless IPXK_ACC_WARM=0, and only where every slice starts inside x; the HEAD form (the head tables: built only with
    // IPXK_ACC_HEAD=1) only on the grid they were built for
    const bool warm = acc_warm_on() && (long long)(W.nslices - 1) * W.slice_elems < (long long)W.xlen;
    const bool head = G > 0 && W.head && W.head_grid == (int)pgrid.x && (W.head_wide != nullptr) == (W.wide != nullptr);
    if (head) {
        const acc_u32x4* hw = reinterpret_cast<const acc_u32x4*>(W.head_wide);
        const acc_u32x4* wd = reinterpret_cast<const acc_u32x4*>(W.wide);
        const dim3 blk(kAccThreads);
        if (wd && warm) hipLaunchKernelGGL((spmv_acc_persist_kernel<Prod, true, true, true>), pgrid, blk, lds, s, W, W.tile_step, W.steps, W.wide_start, wd, x, done, W.head, hw);
        else if (wd) hipLaunchKernelGGL((spmv_acc_persist_kernel<Prod, true, true, false>), pgrid, blk, lds, s, W, W.tile_step, W.steps, W.wide_start, wd, x, done, W.head, hw);
        else if (warm) hipLaunchKernelGGL((spmv_acc_persist_kernel<Prod, false, true, true>), pgrid, blk, lds, s, W, W.tile_step, W.steps, (const unsigned*)nullptr, wd, x, done, W.head, hw);
        else hipLaunchKernelGGL((spmv_acc_persist_kernel<Prod, false, true, false>), pgrid, blk, lds, s, W, W.tile_step, W.steps, (const unsigned*)nullptr, wd, x, done, W.head, hw);
    } else if (G > 0 && W.wide && warm)
        hipLaunchKernelGGL((spmv_acc_persist_kernel<Prod, true, false, true>), pgrid, dim3(kAccThreads), lds, s, W, W.tile_step, W.steps, W.wide_start,
                           reinterpret_cast<const acc_u32x4*>(W.wide), x, done, (const unsigned*)nullptr, (const acc_u32x4*)nullptr);
    else if (G > 0 && W.wide)       // (the wide stream: built unless IPXK_ACC_WIDE=0)
        hipLaunchKernelGGL((spmv_acc_persist_kernel<Prod, true>), pgrid, dim3(kAccThreads), lds, s, W, W.tile_step, W.steps, W.wide_start,
                           reinterpret_cast<const acc_u32x4*>(W.wide), x, done, (const unsigned*)nullptr, (const acc_u32x4*)nullptr);
    else if (G > 0 && warm)
        hipLaunchKernelGGL((spmv_acc_persist_kernel<Prod, false, false, true>), pgrid, dim3(kAccThreads), lds, s, W, W.tile_step, W.steps,
                           (const unsigned*)nullptr, (const acc_u32x4*)nullptr, x, done, (const unsigned*)nullptr, (const acc_u32x4*)nullptr);
    else if (G > 0)
        hipLaunchKernelGGL((spmv_acc_persist_kernel<Prod, false>), pgrid, dim3(kAccThreads), lds, s, W, W.tile_step, W.steps,
                           (const unsigned*)nullptr, (const acc_u32x4*)nullptr, x, done, (const unsigned*)nullptr, (const acc_u32x4*)nullptr);
    else hipLaunchKernelGGL((spmv_acc_tile_kernel<Prod>), dim3(ntiles), dim3(kAccThreads), lds, s, W, x, done);
}

// The tile kernel of the sliced / fused tiles and, with several slices, the combine.  COMPACT: the compacted copy of the tiles
// (GatherMatrix::compact_tiles) -- the plain kernels on fewer entries
template <class Epi, bool MASKED = false, bool COMPACT = false>
inline void launch_spmv_sliced(const GatherMatrix& M, const double* x, const Epi& epi, double* dot_partials,
                               const int* done, hipStream_t s) {
    static_assert(!(MASKED && COMPACT), "the compacted copy needs no mask");
    const SlicedView V = M.sliced_view(COMPACT ? 2 : MASKED ? 1 : 0);
    const size_t lds = (size_t)(M.sliced.max_tile + M.sliced.max_tile / 32 + 1) * sizeof(double);
    const dim3 grid(V.nrb * V.nslices), block(kBlock);
    if (V.nslices == 1) {       // fused: the tile kernel is the whole product
        const dim3 fgrid(M.fused_grid());
        if (V.R == kBlock * 4) hipLaunchKernelGGL((spmv_sliced_tile_kernel<Epi, 4, true, MASKED>), fgrid, block, lds, s, V, x, epi, dot_partials, done);
        else if (V.R == kBlock * 2) hipLaunchKernelGGL((spmv_sliced_tile_kernel<Epi, 2, true, MASKED>), fgrid, block, lds, s, V, x, epi, dot_partials, done);
        else hipLaunchKernelGGL((spmv_sliced_tile_kernel<Epi, 1, true, MASKED>), fgrid, block, lds, s, V, x, epi, dot_partials, done);
    } else {
        if (V.R == kBlock * 4) hipLaunchKernelGGL((spmv_sliced_tile_kernel<Epi, 4, false, MASKED>), grid, block, lds, s, V, x, epi, dot_partials, done);
        else if (V.R == kBlock * 2) hipLaunchKernelGGL((spmv_sliced_tile_kernel<Epi, 2, false, MASKED>), grid, block, lds, s, V, x, epi, dot_partials, done);
        else hipLaunchKernelGGL((spmv_sliced_tile_kernel<Epi, 1, false, MASKED>), grid, block, lds, s, V, x, epi, dot_partials, done);
        launch_combine(V, epi, dot_partials, done, s);
    }
}

// Launches the SpMV on M.layout (masked products: on the tile base) + the long-row kernels when the matrix has long rows.
// Returns the number of dot partials written (0 when dot_partials == nullptr).
template <class Epi, bool MASKED = false>
inline int launch_spmv(const GatherMatrix& M, const double* x, const Epi& epi, double* dot_partials,
                       const int* done, hipStream_t s) {
    switch (MASKED ? M.tile_base() : M.layout) {
        case SpmvLayout::accfused: {
            const AccView W = M.acc_fused_view();
            static bool lds_attr_set = false;
            if (!lds_attr_set) {
                IPXK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(spmv_acc_fused_kernel<Epi>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(kAccMaxRows * sizeof(double))));
                lds_attr_set = true;
            }
            hipLaunchKernelGGL((spmv_acc_fused_kernel<Epi>), dim3(W.nrb), dim3(kAccThreads), (size_t)W.RB * sizeof(double), s, W, x, epi, dot_partials, done);
            break;
        }
        case SpmvLayout::plain:
            hipLaunchKernelGGL(spmv_rowgroup_kernel<Epi>, dim3(M.plain_grid()), dim3(kBlock), 0, s, M.nrows, M.csr_ptr, M.csr_idx, M.csr_val,
                               M.nlong > 0 ? M.row_long.get() : nullptr, x, epi, dot_partials, done);
            break;
        case SpmvLayout::sortedfused: {
            const SortedView W = M.sorted_view();
            const size_t lds = (size_t)(M.sorted.max_sub + M.sorted.max_sub / 32 + 1) * sizeof(double);
            const dim3 grid(M.sorted_fused_grid()), block(kSortedThreads);
            switch (W.RB / kSortedThreads) {
                case 32: hipLaunchKernelGGL((spmv_sorted_fused_kernel<Epi, 32>), grid, block, lds, s, W, x, epi, dot_partials, done); break;
                case 16: hipLaunchKernelGGL((spmv_sorted_fused_kernel<Epi, 16>), grid, block, lds, s, W, x, epi, dot_partials, done); break;
                case 8: hipLaunchKernelGGL((spmv_sorted_fused_kernel<Epi, 8>), grid, block, lds, s, W, x, epi, dot_partials, done); break;
                case 4: hipLaunchKernelGGL((spmv_sorted_fused_kernel<Epi, 4>), grid, block, lds, s, W, x, epi, dot_partials, done); break;
                case 2: hipLaunchKernelGGL((spmv_sorted_fused_kernel<Epi, 2>), grid, block, lds, s, W, x, epi, dot_partials, done); break;
                default: hipLaunchKernelGGL((spmv_sorted_fused_kernel<Epi, 1>), grid, block, lds, s, W, x, epi, dot_partials, done); break;
            }
            break;
        }
        case SpmvLayout::acc: {         // accumulated tiles + the sliced layout's combine on their partial vectors
            const AccView W = M.acc_view();
            launch_acc_tiles<Epi>(W, x, done, s);
            SlicedView C = M.sliced_view(0);
            C.nrows_pad = W.nrows_pad; C.partial = W.partial;
            launch_combine(C, epi, dot_partials, done, s);
            break;
        }
        case SpmvLayout::sliced:
        case SpmvLayout::fused:
            if (MASKED && M.compact.valid) launch_spmv_sliced<Epi, false, true>(M, x, epi, dot_partials, done, s);
            else launch_spmv_sliced<Epi, MASKED>(M, x, epi, dot_partials, done, s);
            break;
        case SpmvLayout::phased: {
            const GatherView V = M.view(MASKED);
            const dim3 grid(M.G), block(kBlock);
            switch (M.RT) {
                case 1: hipLaunchKernelGGL((spmv_phased_kernel<Epi, 1, MASKED>), grid, block, 0, s, V, x, epi, dot_partials, done); break;
                case 2: hipLaunchKernelGGL((spmv_phased_kernel<Epi, 2, MASKED>), grid, block, 0, s, V, x, epi, dot_partials, done); break;
                case 4: hipLaunchKernelGGL((spmv_phased_kernel<Epi, 4, MASKED>), grid, block, 0, s, V, x, epi, dot_partials, done); break;
                default: hipLaunchKernelGGL((spmv_phased_kernel<Epi, 8, MASKED>), grid, block, 0, s, V, x, epi, dot_partials, done); break;
            }
            break;
        }
    }
    const int np = M.num_partials(MASKED);
    if (M.nlong > 0) {          // rows of more than kMaxRowLen entries: segment sums + ordered fix-up, whose dot partial comes last
        const GatherView G = M.view(MASKED);
        hipLaunchKernelGGL(spmv_long_kernel<Epi>, dim3(M.nseg), dim3(kBlock), 0, s, G, x, done);
        hipLaunchKernelGGL(spmv_long_fixup_kernel<Epi>, dim3(1), dim3(kBlock), 0, s, G, epi, dot_partials, np - 1, done);
    }
    return dot_partials ? np : 0;
}

}  // namespace ipxk
