// The inverted head / tail blocks of a sweep (Sweep::Block, trisolve.hpp): built and probed at Prepare, applied by
// run_block in front of / behind the level-scheduled launches of the sweep (sweep.hip).
#include "context.hpp"
#include "inverse_guard.hpp"
#include "trisolve.hpp"

namespace ipxk {

// ---------------------------------------------------------------------------
// inverted head / tail of a sweep (Sweep::Block, trisolve.hpp)
// ---------------------------------------------------------------------------
constexpr int kBlockInvThreads = 1024;
// slot of entry e of a row whose first entry sits at `base` (base < 0: a row of a long chunk, -(slot + 1))
__device__ __forceinline__ int row_slot(int base, int e) {
    return base >= 0 ? base + e * 64 : (-base - 1) + (e >> 3) * 64 + (e & 7);
}
// per block row: how many of its entries look at positions in front of the block (< p0) / inside it
__global__ void block_count_kernel(int K, int p0, const int* __restrict__ tpos, const int* __restrict__ base, const int* __restrict__ len,
                                   const int* __restrict__ idx, int* __restrict__ hcnt, int* __restrict__ tcnt) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < K; t += gridDim.x * blockDim.x) {
        const int L = len[tpos[t]] & ((1 << kLenBits) - 1), b = base[t];
        int h = 0;
        for (int e = 0; e < L; e++) h += idx[row_slot(b, e)] < p0 ? 1 : 0;
        hcnt[t] = h;
        tcnt[t] = L - h;
    }
}
// outside entries -> their slots (row order kept); inside entries -> (block rank of the dependency, unscaled value)
__global__ void block_fill_kernel(int K, int p0, const int* __restrict__ tpos, const int* __restrict__ base, const int* __restrict__ len,
                                  const int* __restrict__ idx, const double* __restrict__ val, const int* __restrict__ rank_of_pos,
                                  const int* __restrict__ hptr, const int* __restrict__ tptr, int* __restrict__ hslot,
                                  int* __restrict__ hidx, int* __restrict__ tcol, double* __restrict__ tval) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < K; t += gridDim.x * blockDim.x) {
        const int L = len[tpos[t]] & ((1 << kLenBits) - 1), b = base[t];
        int h = hptr[t], q = tptr[t];
        for (int e = 0; e < L; e++) {
            const int slot = row_slot(b, e), j = idx[slot];
            if (j < p0) { hslot[h] = slot; hidx[h] = j; h++; }
            else { tcol[q] = rank_of_pos[j - p0]; tval[q] = val[slot]; q++; }
        }
    }
}
// M = inverse(T22), T22 = diag + the inside entries, lower triangular in block order.  A workgroup owns 64 columns of M
// (lane = column) and walks the block's levels; the rows of a level are independent and shared among the wavefronts.
// Row i of the columns j0.. needs the rows k < i of the SAME columns: written by this workgroup in earlier levels.
__global__ __launch_bounds__(kBlockInvThreads) void block_inverse_kernel(int K, int nlev, const int* __restrict__ lev, const int* __restrict__ tptr,
                                                                         const int* __restrict__ tcol, const double* __restrict__ tval,
                                                                         const double* __restrict__ dg, const int* __restrict__ tpos,
                                                                         double* M) {
    const int j0 = blockIdx.x * 64, j = j0 + (threadIdx.x & 63), wave = threadIdx.x >> 6;
    for (int l = 0; l < nlev; l++) {
        const int r1 = lev[l + 1];
        for (int i = lev[l] + wave; i < r1; i += kBlockInvThreads / 64) {
            if (i < j0) continue;                                  // rows above the block's first column: zero (M is pre-filled)
            double s2 = i == j ? 1.0 : 0.0;
            for (int e = tptr[i]; e < tptr[i + 1]; e++) {
                const int k = tcol[e];
                if (k >= j0 && j < K) s2 -= tval[e] * M[(size_t)k * K + j];
            }
            if (j < K) M[(size_t)i * K + j] = s2 / dg[tpos[i]];
        }
        __syncthreads();                                           // (workgroup-scope release / acquire of the rows just written)
    }
}
// right-hand side of block unknown l as the block's kernels read it: xin[zsrc[l]]
__global__ void block_zsrc_kernel(int K, const int* __restrict__ tpos, const int* __restrict__ src, int* __restrict__ zsrc) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < K; t += gridDim.x * blockDim.x) zsrc[t] = src[tpos[t]];
}
// z[t] = (rhs of block row t minus its outside entries, all final: the launches of the earlier levels are over)
// [/ the column scale of unknown t: scaled U' sweep], 32 lanes per row
__global__ __launch_bounds__(kBlock) void block_gather_kernel(SweepView S, int K, const int* __restrict__ zsrc, const int* __restrict__ hptr,
                                                              const int* __restrict__ hslot, const int* __restrict__ hidx,
                                                              const int* __restrict__ unk, const double* __restrict__ pre_scale,
                                                              const double* __restrict__ xin, const double* __restrict__ y,
                                                              double* __restrict__ z, const int* done) {
    if (done && *done) return;
    const int g = threadIdx.x & 31;
    for (int t = (blockIdx.x * kBlock + threadIdx.x) >> 5; t < K; t += (gridDim.x * kBlock) >> 5) {
        const int e1 = hptr[t + 1];
        const double b = xin[zsrc[t]];
        double s2 = 0.0;
        for (int e = hptr[t] + g; e < e1; e += 32) s2 += S.val[hslot[e]] * y[hidx[e]];
        s2 = wave_sum<32>(s2);
        if (g == 0) {
            const double r = b - s2;
            z[t] = pre_scale ? r / pre_scale[unk[t]] : r;
        }
    }
}
// y[pos[t]] = (row t of M) z  [/ the column scale of unknown t: scaled U sweep]; M is lower triangular: a workgroup
// takes kGemvPairs pairs of rows (t, K-1-t) -- every pair K+1 entries together --, thread q the columns q, q + 256, ...
// of all its rows: z[l] is fetched (INLINE_Z: formed, two gathers and a division) once per workgroup and column, the
// 2 kGemvPairs loads of a column are independent, fixed reduction tree.
// INLINE_Z (a head: rows without outside entries): z[l] = xin[zsrc[l]] [/ pre_scale] is formed on the fly, no gather
// launch in front.  Second copy of the result as SweepView::dst2 asks.
// (Until round 5 one pair per workgroup: a head of 1800 unknowns formed its z 900 times over, 15.6 us for 12.5 MB.)
constexpr int kGemvPairs = 2;
template <bool INLINE_Z>
__global__ __launch_bounds__(kBlock) void block_gemv_kernel(int K, const double* __restrict__ M, const double* __restrict__ z,
                                                            const int* __restrict__ zsrc, const double* __restrict__ xin,
                                                            const double* __restrict__ pre_scale,
                                                            const int* __restrict__ tpos, const int* __restrict__ unk,
                                                            const double* __restrict__ post_scale, double* __restrict__ y,
                                                            const int* __restrict__ dst2, double* __restrict__ out2, const int* done) {
    if (done && *done) return;
    constexpr int R = 2 * kGemvPairs;
    __shared__ double red[R][kBlock / 64];
    // rows of the workgroup: pair r = (t0 + r, K - 1 - t0 - r); a pair past the middle is left out (row = -1)
    const int t0 = blockIdx.x * kGemvPairs;
    int row[R];
#pragma unroll
    for (int r = 0; r < kGemvPairs; r++) {
        const int ta = t0 + r, tb = K - 1 - ta;
        row[r] = ta <= tb ? ta : -1;
        row[kGemvPairs + r] = ta < tb ? tb : -1;
    }
    const int ncol = K - t0;                                       // the longest row of the workgroup: K - 1 - t0
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0;
    // four columns per round: their z and all the loads of M issued before the first product
    constexpr int UN = 4;
    for (int l0 = threadIdx.x; l0 < ncol; l0 += UN * kBlock) {
        double zl[UN], mv[UN][R];
#pragma unroll
        for (int u = 0; u < UN; u++) {
            const int l = l0 + u * kBlock;
            zl[u] = 0.0;
            if (l < ncol) {
                if (INLINE_Z) { zl[u] = xin[zsrc[l]]; if (pre_scale) zl[u] /= pre_scale[unk[l]]; }
                else zl[u] = z[l];
            }
#pragma unroll
            for (int r = 0; r < R; r++) mv[u][r] = l <= row[r] ? M[(size_t)row[r] * K + l] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < UN; u++)
#pragma unroll
            for (int r = 0; r < R; r++)
                if (l0 + u * kBlock <= row[r]) acc[r] += mv[u][r] * zl[u];      // (a column beyond the row contributes nothing, whatever its z)
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < R; r++) {
        wave_sum_each(acc[r]);
        if (lane == 0) red[r][wave] = acc[r];
    }
    __syncthreads();
    if (threadIdx.x < R) {
        int t = -1;
#pragma unroll
        for (int r = 0; r < R; r++) if (threadIdx.x == r) t = row[r];
        if (t >= 0) {
            double s2 = 0.0;
#pragma unroll
            for (int w = 0; w < kBlock / 64; w++) s2 += red[threadIdx.x][w];
            const double v = post_scale ? s2 / post_scale[unk[t]] : s2;
            const int pos = tpos[t];
            y[pos] = v;
            if (dst2 && dst2[pos] >= 0) out2[dst2[pos]] = v;
        }
    }
}

// w_q = M z_q for the lower-triangular M of an inverted head / tail (row major, K x K): one wavefront per row
__global__ __launch_bounds__(kBlock) void block_probe_mz_kernel(int K, const double* __restrict__ M, double* __restrict__ w) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); i < K; i += gridDim.x * (kBlock / 64)) {
        double s0 = 0.0, s1 = 0.0;
        for (int l = lane; l <= i; l += 64) { const double a = M[(size_t)i * K + l]; s0 += a * probe_z(0, l); s1 += a * probe_z(1, l); }
        wave_sum_each(s0, s1);
        if (lane == 0) { w[i] = s0; w[K + i] = s1; }
    }
}
// res[q] = max_i | (T22 w_q)_i - z_q(i) |,  T22 = diagonal + the block's inside entries (unscaled)
__global__ void block_probe_res_kernel(int K, const int* __restrict__ tptr, const int* __restrict__ tcol, const double* __restrict__ tval,
                                       const double* __restrict__ dg, const int* __restrict__ tpos, const double* __restrict__ w, double* res) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < K; i += gridDim.x * blockDim.x) {
        const double d = dg[tpos[i]];
        double r0 = d * w[i], r1 = d * w[K + i];
        for (int e = tptr[i]; e < tptr[i + 1]; e++) { const int k = tcol[e]; r0 += tval[e] * w[k]; r1 += tval[e] * w[K + k]; }
        probe_max(res + 0, fabs(r0 - probe_z(0, i)));
        probe_max(res + 1, fabs(r1 - probe_z(1, i)));
    }
}

// the levels [la, lb) of S as an inverted block
static void build_block(Context* c, Sweep& S, Sweep::Block& T, int la, int lb, const char* what) {
    hipStream_t s = c->stream;
    const int c0 = S.level_chunk[la], c1 = S.level_chunk[lb], nc = c1 - c0;
    int64_t K = 0;
    for (int l = la; l < lb; l++) K += S.level_width[l];
    std::vector<ChunkDesc> ch((size_t)nc);
    IPXK_HIP(hipMemcpyAsync(ch.data(), S.chunks.get() + c0, (size_t)nc * sizeof(ChunkDesc), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
    const int p0 = ch[0].pos0, p1 = ch.back().pos0 + (ch.back().width >= 0 ? 64 : kLongLanes), np = p1 - p0;
    std::vector<int> order((size_t)np);
    IPXK_HIP(hipMemcpyAsync(order.data(), S.order.get() + p0, (size_t)np * sizeof(int), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
    std::vector<int> tpos, unk, base, rank((size_t)np, -1), lev;
    tpos.reserve((size_t)K); unk.reserve((size_t)K); base.reserve((size_t)K);
    // block order = position order; level boundaries from the level widths (a merged chunk holds its levels in order)
    for (const ChunkDesc& d : ch) {
        const int npos_c = d.width >= 0 ? 64 : kLongLanes;
        for (int q = 0; q < npos_c; q++) {
            const int pos = d.pos0 + q;
            if (order[pos - p0] < 0) continue;
            rank[pos - p0] = (int)tpos.size();
            tpos.push_back(pos);
            unk.push_back(order[pos - p0]);
            base.push_back(d.width >= 0 ? d.ent0 + q : -(d.ent0 + 8 * q + 1));
        }
    }
    IPXK_REQUIRE((int64_t)tpos.size() == K, "inverted block of a sweep: positions and level widths disagree");
    lev.push_back(0);
    for (int l = la; l < lb; l++) lev.push_back(lev.back() + S.level_width[l]);
    const int Ki = (int)K;
    DevBuf<int> &dbase = T.w_base, &drank = T.w_rank, &hcnt = T.w_hcnt, &tcnt = T.w_tcnt, &dlev = T.w_lev, &tptr = T.w_tptr, &tcol = T.w_tcol;
    DevBuf<double>& tval = T.w_tval;
    hcnt.ensure((size_t)Ki); tcnt.ensure((size_t)Ki);
    T.pos.upload(tpos, s); T.unk.upload(unk, s);
    dbase.upload(base, s); drank.upload(rank, s); dlev.upload(lev, s);
    hipLaunchKernelGGL(block_count_kernel, dim3(vec_grid(Ki)), dim3(kBlock), 0, s, Ki, p0, T.pos.get(), dbase.get(), S.len.get(),
                       S.idx.get(), hcnt.get(), tcnt.get());
    std::vector<int> hc((size_t)Ki), tc((size_t)Ki), hp((size_t)Ki + 1, 0), tp((size_t)Ki + 1, 0);
    hcnt.download(hc.data(), hc.size(), s); tcnt.download(tc.data(), tc.size(), s);
    IPXK_HIP(hipStreamSynchronize(s));
    for (int t = 0; t < Ki; t++) { hp[t + 1] = hp[t] + hc[t]; tp[t + 1] = tp[t] + tc[t]; }
    T.hptr.upload(hp, s); tptr.upload(tp, s);
    T.nh = hp[Ki];
    T.hslot.ensure((size_t)std::max(T.nh, 1)); T.hidx.ensure((size_t)std::max(T.nh, 1)); T.zsrc.ensure((size_t)Ki); tcol.ensure((size_t)std::max(tp[Ki], 1)); tval.ensure((size_t)std::max(tp[Ki], 1));
    hipLaunchKernelGGL(block_fill_kernel, dim3(vec_grid(Ki)), dim3(kBlock), 0, s, Ki, p0, T.pos.get(), dbase.get(), S.len.get(),
                       S.idx.get(), S.val.get(), drank.get(), T.hptr.get(), tptr.get(), T.hslot.get(), T.hidx.get(), tcol.get(), tval.get());
    T.M.ensure((size_t)Ki * Ki); T.z.ensure((size_t)Ki);
    IPXK_HIP(hipMemsetAsync(T.M.get(), 0, (size_t)Ki * Ki * sizeof(double), s));
    hipLaunchKernelGGL(block_inverse_kernel, dim3((Ki + 63) / 64), dim3(kBlockInvThreads), 0, s, Ki, lb - la, dlev.get(), tptr.get(),
                       tcol.get(), tval.get(), S.diag.get(), T.pos.get(), T.M.get());
    // the guard: T22 (M z) against z for two fixed vectors
    T.w_probe.ensure((size_t)2 * Ki + 2);
    DevBuf<double>& pw = T.w_probe;
    const double resid = probe_residual(s, pw.get() + 2 * (size_t)Ki, [&] {
        hipLaunchKernelGGL(block_probe_mz_kernel, dim3((Ki + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, s, Ki, T.M.get(), pw.get());
        hipLaunchKernelGGL(block_probe_res_kernel, dim3(vec_grid(Ki)), dim3(kBlock), 0, s, Ki, tptr.get(), tcol.get(), tval.get(), S.diag.get(),
                           T.pos.get(), pw.get(), pw.get() + 2 * (size_t)Ki);
    });                                                            // (its synchronization also: the host vectors uploaded above go out of scope)
    IPXK_HIP(hipGetLastError());
    const bool good = resid <= inverse_tol();
    c->split_stats.inverse_probes++;
    record_verdict(c, resid, good);
    if (sweep_verbose())
        fprintf(stderr, "ipxk: sweep %s: levels %d..%d (%d unknowns, %d outside + %d inside entries) inverted; probe |T M z - z| = %.2e%s\n", what, la,
                lb - 1, Ki, T.nh, tp[Ki], resid, good ? "" : " -> REJECTED, these levels stay in the level-scheduled sweep");
    if (!good) { T.K = 0; return; }
    T.K = Ki; T.la = la; T.lb = lb; T.p0 = p0; T.p1 = p1;
}

void build_sweep_blocks(Context* c, Sweep& S, bool level_launches) {
    S.head.K = S.tail.K = 0;
    // IPXK_TAIL_INVERSE / IPXK_HEAD_INVERSE: unknowns at most (default 2048); 0: never.  Large factors only: below
    // IPXK_TAIL_MIN_DIM rows (default 200 000) the whole sweep is a few launches anyway, and the small cases of the
    // test-suite stay bit-identical to the reference's arithmetic.
    auto env_int = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    const int tail_max = env_int("IPXK_TAIL_INVERSE", 2048), head_max = env_int("IPXK_HEAD_INVERSE", 2048);
    const int min_dim = env_int("IPXK_TAIL_MIN_DIM", 200000);
    constexpr int kMinLevels = 8, kMinUnknowns = 256;
    const int nlev = S.nlevels;
    if (level_launches || nlev < kMinLevels + 1 || S.dim < min_dim) return;
    // the longest run of final levels with at most tail_max unknowns and at most 1/64 of the sweep
    int la = nlev;
    int64_t K = 0;
    for (const int64_t cap = std::min<int64_t>(tail_max, S.dim / 64); la > 1 && K + S.level_width[la - 1] <= cap;) K += S.level_width[--la];
    // (a block starts and ends with a chunk: consecutive tiny levels may share a MERGED chunk, which stays whole)
    while (la < nlev && la > 0 && S.level_chunk[la] == S.level_chunk[la - 1]) K -= S.level_width[la++];
    const bool tail = nlev - la >= kMinLevels && K >= kMinUnknowns;
    if (!tail) la = nlev;
    // ... and of first levels (their rows have no entries outside the block)
    int lb = 0;
    K = 0;
    for (const int64_t cap = std::min<int64_t>(head_max, S.dim / 64); lb < la - 1 && K + S.level_width[lb] <= cap;) K += S.level_width[lb++];
    while (lb > 0 && lb < nlev && S.level_chunk[lb] == S.level_chunk[lb - 1]) K -= S.level_width[--lb];
    const bool head = lb >= kMinLevels && K >= kMinUnknowns;
    if (getenv("IPXK_SWEEP_STATS"))
        fprintf(stderr, "ipxk: sweep blocks: %d levels, tail candidate %d.. (%s), head candidate ..%d (%lld unknowns, %s)\n", nlev, la,
                tail ? "taken" : "not taken", lb - 1, (long long)K, head ? "taken" : "not taken");
    if (head) build_block(c, S, S.head, 0, lb, "head");
    if (tail) build_block(c, S, S.tail, la, nlev, "tail");
}

// x2 = inverse(T22) (b2 - T21 x1) for the levels the plan leaves out (Sweep::Block); V: the sweep's view with its second destination
void run_block(Context* c, const Sweep& S, const Sweep::Block& T, const SweepView& V, bool scaled, const double* xin, const int* done) {
    double* xout = S.y.get();
    const double* us = scaled ? c->split->uscale.get() : nullptr;
    const double *pre = S.scale_mode == 1 ? us : nullptr, *post = S.scale_mode == 2 ? us : nullptr;
    const int wgs = ((T.K + 1) / 2 + kGemvPairs - 1) / kGemvPairs;
    if (T.nh == 0) {
        hipLaunchKernelGGL(block_gemv_kernel<true>, dim3(wgs), dim3(kBlock), 0, c->stream, T.K, T.M.get(), T.z.get(), T.zsrc.get(), xin, pre,
                           T.pos.get(), T.unk.get(), post, xout, V.dst2, V.out2, done);
        return;
    }
    hipLaunchKernelGGL(block_gather_kernel, dim3((T.K * 32 + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, V, T.K, T.zsrc.get(),
                       T.hptr.get(), T.hslot.get(), T.hidx.get(), T.unk.get(), pre, xin, xout, T.z.get(), done);
    hipLaunchKernelGGL(block_gemv_kernel<false>, dim3(wgs), dim3(kBlock), 0, c->stream, T.K, T.M.get(), T.z.get(), T.zsrc.get(), xin, pre,
                       T.pos.get(), T.unk.get(), post, xout, V.dst2, V.out2, done);
}

// where the blocks' right-hand sides sit in the sweep's input vector (after Sweep::src has been composed)
void locate_block_rhs(Context* c, Sweep& W) {
    for (Sweep::Block* T : {&W.head, &W.tail})
        if (T->K > 0)
            hipLaunchKernelGGL(block_zsrc_kernel, dim3(vec_grid(T->K)), dim3(kBlock), 0, c->stream, T->K, T->pos.get(), W.src.get(), T->zsrc.get());
}

}  // namespace ipxk
