// The gather-matrix layouts built ON THE DEVICE (round 4): long rows taken out, then the tile layouts (internal.hpp) by radix
// sorts -- the same scheme nmatrix.hip uses for N:
//   * a STABLE sort of the entries, enumerated in storage order, by (tile, row in tile) IS the sliced layout:
//     tile pointers by binary search in the sorted keys, per-row byte counts from the runs of equal keys, indices
//     and values by a gather through the sorted positions;
//   * the accumulated tiles: one sort by (tile, offset), then the greedy batches of a tile by one wavefront;
//   * the sorted fused tiles: the entries keep their storage order as slots (a row block's entries are contiguous), one sort
//     by (tile, gathered index) whose ties keep the slot order, exactly the host builder's comparator.
// Every array equals the host builder's (layout_host.hip) bit for bit (tests/test_gpu_layout.py compares them all); slices
// and row blocks come from layout_geometry.hpp on both sides.  GatherMatrix::build_device (spmv.hip) drives the builders.
#include <numeric>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "layout_scratch.hpp"

namespace ipxk {

// the sorts and the scan of layout_scratch.hpp
template <class K>
void sort_pairs(Tmp& T, const K* kin, K* kout, const unsigned* vin, unsigned* vout, size_t n, int bits, hipStream_t s) {
    size_t bytes = 0;
    IPXK_HIP(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, n, 0u, (unsigned)bits, s));
    IPXK_HIP(rocprim::radix_sort_pairs(T.need(bytes), bytes, kin, kout, vin, vout, n, 0u, (unsigned)bits, s));
}
template void sort_pairs<unsigned>(Tmp&, const unsigned*, unsigned*, const unsigned*, unsigned*, size_t, int, hipStream_t);
template void sort_pairs<u64>(Tmp&, const u64*, u64*, const unsigned*, unsigned*, size_t, int, hipStream_t);
void sort_keys(Tmp& T, u64* in, u64* out, size_t n, hipStream_t s) {
    size_t bytes = 0;
    IPXK_HIP(rocprim::radix_sort_keys(nullptr, bytes, in, out, n, 0u, 64u, s));
    IPXK_HIP(rocprim::radix_sort_keys(T.need(bytes), bytes, in, out, n, 0u, 64u, s));
}
void scan_int(Tmp& T, const int* in, int* out, size_t n, hipStream_t s) {
    size_t bytes = 0;
    IPXK_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, 0, n, rocprim::plus<int>(), s));
    IPXK_HIP(rocprim::exclusive_scan(T.need(bytes), bytes, in, out, 0, n, rocprim::plus<int>(), s));
}

namespace {

template <class K>
__global__ void lower_bounds_kernel(int64_t count, int64_t nz, const K* __restrict__ sorted, u64 stride, int shift, unsigned* __restrict__ out) {
    // out[t] = first position whose key is >= t * stride (shift: keys are compared after >> shift)
    IPXK_GRID_STRIDE(t, count) {
        const u64 want = (u64)t * stride;
        int64_t lo = 0, hi = nz;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (((u64)sorted[mid] >> shift) < want) lo = mid + 1; else hi = mid; }
        out[t] = (unsigned)lo;
    }
}
__global__ void row_extent_kernel(int n, const int* __restrict__ rows, const int* __restrict__ ptr, int* __restrict__ ext) {
    IPXK_GRID_STRIDE(l, n) { ext[2 * l] = ptr[rows[l]]; ext[2 * l + 1] = ptr[rows[l] + 1]; }
}
// key of the sliced layout: (tile, row in tile), tile = row block * ns + slice of the gathered index
__global__ void sliced_keys_kernel(int nrows, const int* __restrict__ ptr, const int* __restrict__ idx, int R, int ns, int slice,
                                   unsigned* __restrict__ key, unsigned* __restrict__ pos) {
    IPXK_GRID_STRIDE(r, nrows) {
        const unsigned base = (unsigned)(r / R) * (unsigned)ns, rr = (unsigned)(r % R);
        for (int p = ptr[r]; p < ptr[r + 1]; p++) {
            key[p] = (base + (unsigned)(idx[p] / slice)) * (unsigned)R + rr;
            pos[p] = (unsigned)p;
        }
    }
}
// byte counts per key from the runs of equal keys (cnt is zero on entry); a run of more than 255 raises *overflow
__global__ void run_counts_kernel(int64_t nz, const unsigned* __restrict__ sorted, unsigned char* __restrict__ cnt, int* overflow) {
    IPXK_GRID_STRIDE(e, nz) {
        const unsigned k = sorted[e];
        if (e > 0 && sorted[e - 1] == k) continue;
        int len = 1;
        while (e + len < nz && len <= 256 && sorted[e + len] == k) len++;
        if (len > 255) *overflow = 1;
        cnt[k] = (unsigned char)len;
    }
}
__global__ void gather_entries_kernel(int64_t nz, const unsigned* __restrict__ perm, const int* __restrict__ idx, const double* __restrict__ val,
                                      int* __restrict__ out_idx, double* __restrict__ out_val) {
    IPXK_GRID_STRIDE(e, nz) {
        const unsigned p = perm[e];
        out_idx[e] = idx[p];
        out_val[e] = val[p];
    }
}
// [0] = largest tile, [2..3] = (64 bits) sum over the row blocks of their fullest slice's entries
__global__ void tile_stats_kernel(int nrb, int ns, const unsigned* __restrict__ tile_ptr, int* out) {
    int best_tile = 0;
    u64 dom = 0;
    IPXK_GRID_STRIDE(rb, nrb) {
        unsigned best = 0;
        for (int sl = 0; sl < ns; sl++) best = max(best, tile_ptr[(size_t)rb * ns + sl + 1] - tile_ptr[(size_t)rb * ns + sl]);
        best_tile = max(best_tile, (int)best);
        dom += best;
    }
    best_tile = wave_max(best_tile);
    dom = wave_sum(dom);
    if ((threadIdx.x & 63) == 0) {
        atomicMax(out, best_tile);
        if (dom) atomicAdd(reinterpret_cast<u64*>(out + 2), dom);
    }
}
// ---- accumulated tiles -----------------------------------------------------------------------
// key = (tile << 18 | offset in the slice), enumerated in storage order (a stable sort keeps that order among ties)
__global__ void acc_keys_kernel(int nrows, const int* __restrict__ ptr, const int* __restrict__ idx, int RB, int ns, int slice,
                                u64* __restrict__ key, unsigned* __restrict__ pos, int* __restrict__ rowof) {
    IPXK_GRID_STRIDE(r, nrows) {
        const u64 tile0 = (u64)(r / RB) * (u64)ns;
        for (int p = ptr[r]; p < ptr[r + 1]; p++) {
            const int sl = idx[p] / slice, off = idx[p] - sl * slice;
            key[p] = ((tile0 + (u64)sl) << kSortedOffBits) | (u64)(unsigned)off;
            pos[p] = (unsigned)p;
            rowof[p] = (int)r;
        }
    }
}
// the entry words in sorted order: row in block << 18 | offset
__global__ void acc_words_kernel(int64_t nz, const u64* __restrict__ keys, const unsigned* __restrict__ perm, const int* __restrict__ rowof, int RB,
                                 unsigned* __restrict__ word) {
    IPXK_GRID_STRIDE(e, nz) word[e] = ((unsigned)(rowof[perm[e]] % RB) << kSortedOffBits) | (unsigned)(keys[e] & ((1u << kSortedOffBits) - 1u));
}
// The batches of one tile, by ONE wavefront: the tile's entries are walked in address order, 64 candidates at a time
// (the entries that waited from the previous batch first, then the stream); a candidate is taken unless its row
// already has an entry in the current batch (stamp) or an earlier candidate of the same group has the same row
// (claim: the lowest lane wins) or the batch is full; whoever is not taken waits for the next batch, in order.
// Sequential by nature (a greedy list schedule), but only ~ne/64 steps per tile and all tiles in parallel.
__global__ __launch_bounds__(64) void acc_batch_kernel(int RB, const unsigned* __restrict__ tile_ptr, const unsigned* __restrict__ word,
                                                        unsigned* __restrict__ dst, unsigned* pendA, unsigned* pendB, unsigned* __restrict__ bstart,
                                                        unsigned* __restrict__ nbatch, u64* deferred_total) {
    extern __shared__ unsigned ab_lds[];
    unsigned* stamp = ab_lds;
    unsigned* claim = ab_lds + RB;
    const int tile = blockIdx.x, lane = threadIdx.x;
    const unsigned e0 = tile_ptr[tile];
    const int ne = (int)(tile_ptr[tile + 1] - e0);
    for (int r = lane; r < RB; r += 64) { stamp[r] = 0u; claim[r] = 0xffffffffu; }
    __syncthreads();
    unsigned cur = 1;
    int fill = 0, out = 0, nb = 0, cursor = 0, na = 0, ia = 0, nbp = 0;
    u64 ndef = 0;
    unsigned *pa = pendA + e0, *pb = pendB + e0;
    if (ne > 0) { if (lane == 0) bstart[e0] = e0; nb = 1; }
    const u64 lt = (1ull << lane) - 1ull;
    while (out < ne) {
        int n = 0, c = 0;
        if (ia < na) {
            n = min(64, na - ia);
            if (lane < n) c = (int)__hip_atomic_load(pa + ia + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // written by this wave: read it past L1
            ia += n;
        } else if (fill < kAccBatch && cursor < ne) {
            n = min(64, ne - cursor);
            c = cursor + lane;
            cursor += n;
        } else {                                   // close the batch
            if (lane == 0) bstart[e0 + nb] = e0 + (unsigned)out;
            nb++; cur++; fill = 0;
            unsigned* t = pa; pa = pb; pb = t;
            na = nbp; ia = 0; nbp = 0;
            __syncthreads();                       // the waiting list written by this wave is read back below
            continue;
        }
        const bool live = lane < n;
        const unsigned row = live ? (word[e0 + c] >> kSortedOffBits) : 0u;
        const bool ok = live && stamp[row] != cur;
        if (ok) atomicMin(&claim[row], (unsigned)lane);
        __syncthreads();
        const bool win = ok && claim[row] == (unsigned)lane;
        __syncthreads();
        if (win) { claim[row] = 0xffffffffu; stamp[row] = cur; }
        const u64 wmask = __ballot(win);
        const int prefix = __popcll(wmask & lt);
        const bool take = win && prefix < kAccBatch - fill;
        if (take) dst[e0 + c] = e0 + (unsigned)(out + prefix);
        const int nt = __popcll(__ballot(take));
        const bool def = live && !take;
        const u64 dmask = __ballot(def);
        if (def) pb[nbp + __popcll(dmask & lt)] = (unsigned)c;
        const int nd = __popcll(dmask);
        nbp += nd; ndef += (u64)nd; out += nt; fill += nt;
        __syncthreads();
    }
    if (lane == 0) {
        nbatch[tile] = (unsigned)nb;
        if (ndef) atomicAdd(deferred_total, ndef);
    }
}
__global__ void acc_scatter_kernel(int64_t nz, const unsigned* __restrict__ dst, const unsigned* __restrict__ word, const unsigned* __restrict__ perm,
                                   const double* __restrict__ val, unsigned* __restrict__ pack, double* __restrict__ out_val) {
    IPXK_GRID_STRIDE(e, nz) {
        const unsigned d = dst[e];
        pack[d] = word[e];
        out_val[d] = val[perm[e]];
    }
}
__global__ void acc_bptr_kernel(int ntiles, const unsigned* __restrict__ tile_ptr, const unsigned* __restrict__ tile_batch,
                                const unsigned* __restrict__ bstart, unsigned nz, unsigned* __restrict__ bptr) {
    const int tile = blockIdx.x;
    if (tile >= ntiles) return;
    const unsigned e0 = tile_ptr[tile], b0 = tile_batch[tile], nb = tile_batch[tile + 1] - b0;
    for (unsigned q = threadIdx.x; q < nb; q += blockDim.x) bptr[b0 + q] = bstart[e0 + q];
    if (tile == ntiles - 1 && threadIdx.x == 0) bptr[tile_batch[ntiles]] = nz;
}

// The steps of one tile (internal.hpp): left to right over its batches, a step takes batches while their total is at most
// kAccBatch entries and it holds at most maxb of them.  emit(i, b, k): step i of the tile is batches [b, b + k).  Returns the
// number of steps.  The one statement of the rule: the count and the fill below both walk with it.
template <class Emit>
__device__ __forceinline__ unsigned acc_tile_steps(const unsigned* __restrict__ bptr, unsigned b0, unsigned b1, unsigned maxb, Emit emit) {
    unsigned ns = 0;
    for (unsigned b = b0; b < b1; ns++) {
        unsigned k = 1;
        while (k < maxb && b + k < b1 && bptr[b + k + 1] - bptr[b] <= (unsigned)kAccBatch) k++;
        emit(ns, b, k);
        b += k;
    }
    return ns;
}
__global__ void acc_step_count_kernel(int ntiles, const unsigned* __restrict__ tile_batch, const unsigned* __restrict__ bptr, unsigned maxb,
                                      unsigned* __restrict__ nstep) {
    IPXK_GRID_STRIDE(t, ntiles) nstep[t] = acc_tile_steps(bptr, tile_batch[t], tile_batch[t + 1], maxb, [](unsigned, unsigned, unsigned) {});
}
__global__ void acc_step_fill_kernel(int ntiles, const unsigned* __restrict__ tile_batch, const unsigned* __restrict__ bptr, unsigned maxb,
                                     const unsigned* __restrict__ tile_step, unsigned nz, uint4* __restrict__ steps) {
    IPXK_GRID_STRIDE(t, ntiles) {
        const unsigned s0 = tile_step[t];
        acc_tile_steps(bptr, tile_batch[t], tile_batch[t + 1], maxb, [&](unsigned i, unsigned b, unsigned k) {
            const unsigned end = bptr[b + k];
            steps[s0 + i] = make_uint4(bptr[b], k > 1 ? bptr[b + 1] : end, k > 2 ? bptr[b + 2] : end, k > 3 ? bptr[b + 3] : end);
        });
        if (t == ntiles - 1) steps[tile_step[ntiles]] = make_uint4(nz, nz, nz, nz);
    }
}

// The wide stream (internal.hpp) of the steps: the 16-byte units of every step, then (one workgroup per step) its three planes.
__global__ void acc_wide_count_kernel(int nsteps, const uint4* __restrict__ steps, unsigned* __restrict__ units) {
    IPXK_GRID_STRIDE(k, nsteps) units[k] = 3u * (unsigned)acc_wide_threads((int)(steps[k + 1].x - steps[k].x));
}
__global__ __launch_bounds__(kAccThreads) void acc_wide_fill_kernel(int nsteps, const uint4* __restrict__ steps, const unsigned* __restrict__ wide_start,
                                                                    const unsigned* __restrict__ pack, const double* __restrict__ val,
                                                                    uint4* __restrict__ wide) {
    const int t = threadIdx.x;
    for (int k = blockIdx.x; k < nsteps; k += gridDim.x) {
        const unsigned e0 = steps[k].x;
        const int ne = (int)(steps[k + 1].x - e0), tp = acc_wide_threads(ne);
        if (t >= tp) continue;
        unsigned w[kAccPerThread];
        double v[kAccPerThread];
#pragma unroll
        for (int u = 0; u < kAccPerThread; u++) {
            const int p = u * tp + t;
            w[u] = p < ne ? pack[e0 + p] : 0u;
            v[u] = p < ne ? val[e0 + p] : 0.0;
        }
        uint4* dst = wide + wide_start[k];
        dst[t] = make_uint4(w[0], w[1], w[2], w[3]);
        reinterpret_cast<double2*>(dst + tp)[t] = make_double2(v[0], v[1]);
        reinterpret_cast<double2*>(dst + 2 * tp)[t] = make_double2(v[2], v[3]);
    }
}

// The head tables (internal.hpp) of the launch grid P: one thread per workgroup walks its first kAccHeadSteps steps exactly as the
// persistent kernel's walker does (spmv_kernels.hpp: next()), then one workgroup per (workgroup, step) copies the units its
// threads load for that step.
__global__ void acc_head_fill_kernel(int P, int ntiles, const unsigned* __restrict__ tile_step, const uint4* __restrict__ steps,
                                     const unsigned* __restrict__ wide_start, unsigned* __restrict__ head) {
    IPXK_GRID_STRIDE(w, P) {
        unsigned* h = head + (size_t)w * kAccHeadWords;
        int wt = (int)w, wq = 0, wnb = 0;
        unsigned wb0 = 0;
        if (wt < ntiles) { wb0 = tile_step[wt]; wnb = (int)(tile_step[wt + 1] - wb0); }
        for (int i = 0; i < kAccHeadSteps; i++) {
            unsigned r[8] = {0u, 0u, 0u, 0u, 0u, 0u, ~0u, 0u};
            if (wt < ntiles) {
                r[6] = (unsigned)wt;
                if (wnb > 0) {
                    const uint4 a = steps[wb0 + wq];
                    r[0] = a.x; r[2] = a.y; r[3] = a.z; r[4] = a.w; r[1] = steps[wb0 + wq + 1].x;
                    if (wide_start) r[5] = wide_start[wb0 + wq];
                }
                if (++wq >= max(wnb, 1)) {
                    wt += P; wq = 0;
                    if (wt < ntiles) { wb0 = tile_step[wt]; wnb = (int)(tile_step[wt + 1] - wb0); }
                }
            }
            for (int j = 0; j < 8; j++) h[8 * i + j] = r[j];
        }
        h[8 * kAccHeadSteps] = (unsigned)wt; h[8 * kAccHeadSteps + 1] = (unsigned)wq; h[8 * kAccHeadSteps + 2] = wb0; h[8 * kAccHeadSteps + 3] = (unsigned)wnb;
        for (int j = 8 * kAccHeadSteps + 4; j < kAccHeadWords; j++) h[j] = 0u;
    }
}
__global__ __launch_bounds__(kAccThreads) void acc_head_wide_fill_kernel(int P, const unsigned* __restrict__ head, const uint4* __restrict__ wide,
                                                                         uint4* __restrict__ head_wide) {
    const int t = threadIdx.x;
    for (int k = blockIdx.x; k < P * kAccHeadStreams; k += gridDim.x) {
        const unsigned* r = head + (size_t)(k / kAccHeadStreams) * kAccHeadWords + 8 * (k % kAccHeadStreams);
        uint4* dst = head_wide + (size_t)k * 3 * kAccThreads;
        const bool live = (int)r[6] >= 0;
        const int tp = acc_wide_threads((int)(r[1] - r[0]));
        const uint4* src = wide + r[5] + min(t, max(tp - 1, 0));
        for (int p = 0; p < 3; p++) dst[p * kAccThreads + t] = live ? src[p * tp] : make_uint4(0u, 0u, 0u, 0u);
    }
}

// ---- one-slice (FUSED) forms: a tile is a row block, offsets are relative to the tile's smallest gathered index ----
// smallest / largest gathered index per tile, the rows' count bytes (optional), a flag for rows with descending / repeated indices
__global__ void tile_window_kernel(int nrows, const int* __restrict__ ptr, const int* __restrict__ idx, int RB, int* __restrict__ lo,
                                   int* __restrict__ hi, unsigned char* __restrict__ cnt, int* flags) {
    IPXK_GRID_STRIDE(r, nrows) {
        const int p0 = ptr[r], p1 = ptr[r + 1];
        if (cnt) { if (p1 - p0 > 255) flags[0] = 1; cnt[r] = (unsigned char)(p1 - p0); }
        if (p1 == p0) continue;
        int a = idx[p0], b = a;
        for (int p = p0 + 1; p < p1; p++) {
            const int v = idx[p];
            if (v <= idx[p - 1]) flags[1] = 1;                   // not ascending
            a = min(a, v); b = max(b, v);
        }
        atomicMin(lo + r / RB, a);
        atomicMax(hi + r / RB, b);
    }
}
// [0] widest window (hi - lo) of a tile, [1] most entries of a tile; empty tiles get lo = 0
__global__ void tile_window_stats_kernel(int nrb, int nrows, int RB, const int* __restrict__ ptr, int* __restrict__ lo, const int* __restrict__ hi,
                                         int* out) {
    IPXK_GRID_STRIDE(t, nrb) {
        const int r0 = (int)t * RB, r1 = min(nrows, r0 + RB);
        const int ne = ptr[r1] - ptr[r0];
        if (ne == 0) { lo[t] = 0; continue; }
        atomicMax(out + 0, hi[t] - lo[t]);
        atomicMax(out + 1, ne);
    }
}
// key = tile << 18 | (index - the tile's smallest index), enumerated in storage order
__global__ void fused_keys_kernel(int nrows, const int* __restrict__ ptr, const int* __restrict__ idx, int RB, const int* __restrict__ lo,
                                  u64* __restrict__ key, unsigned* __restrict__ pos, int* __restrict__ rowof) {
    IPXK_GRID_STRIDE(r, nrows) {
        const u64 t = (u64)(r / RB);
        const int base = lo[r / RB];
        for (int p = ptr[r]; p < ptr[r + 1]; p++) {
            key[p] = (t << kSortedOffBits) | (u64)(unsigned)(idx[p] - base);
            pos[p] = (unsigned)p;
            if (rowof) rowof[p] = (int)r;
        }
    }
}
// sorted fused tiles: slot = place of the entry in the tile's row-major (= storage) order
__global__ void sorted_fused_fill_kernel(int64_t nz, const u64* __restrict__ keys, const unsigned* __restrict__ perm, const int* __restrict__ ptr, int RB,
                                         const double* __restrict__ val, unsigned* __restrict__ pack, double* __restrict__ out_val) {
    IPXK_GRID_STRIDE(f, nz) {
        const u64 k = keys[f];
        const unsigned p = perm[f], t = (unsigned)(k >> kSortedOffBits);
        pack[f] = ((p - (unsigned)ptr[(size_t)t * RB]) << kSortedOffBits) | (unsigned)(k & ((1u << kSortedOffBits) - 1u));
        out_val[f] = val[p];
    }
}
__global__ void tile_ptr_from_rows_kernel(int nrb, int nrows, int RB, const int* __restrict__ ptr, unsigned* __restrict__ out) {
    IPXK_GRID_STRIDE(t, (int64_t)nrb + 1) out[t] = (unsigned)ptr[min((int64_t)nrows, t * RB)];
}
}  // namespace

// ---------------------------------------------------------------------------
// Long rows (more than kMaxRowLen entries: dense columns of A in the row-wise copy, dense rows in the column-wise one) taken out of a
// row-wise matrix on the device: the flags, the segment arrays of the long-row kernels -- equal to GatherMatrix::build()'s -- and the
// matrix with those rows left empty, from which the tile layouts are then built as for a matrix without long rows.
// (Until round 5 a single long row sent the whole model to the host builders: 1.1 s per gather matrix at 15 M entries.)
// ---------------------------------------------------------------------------
namespace {
constexpr int kMaxLongRowsDevice = 1 << 16;
__global__ void long_flag_kernel(int nrows, const int* __restrict__ ptr, unsigned char* __restrict__ flag, int* __restrict__ slen, int* counters,
                                 int* __restrict__ list, int cap) {
    IPXK_GRID_STRIDE(r, (int64_t)nrows + 1) {
        if (r == nrows) { slen[r] = 0; continue; }
        const int len = ptr[r + 1] - ptr[r];
        const bool lg = len > kMaxRowLen;
        flag[r] = lg ? 1 : 0;
        slen[r] = lg ? 0 : len;
        if (lg) {
            const int k = atomicAdd(counters, 1);
            if (k < cap) list[k] = (int)r;
        }
    }
}
__global__ void strip_copy_kernel(int nrows, const int* __restrict__ ptr, const int* __restrict__ sptr, const unsigned char* __restrict__ flag,
                                  const int* __restrict__ idx, const double* __restrict__ val, int* __restrict__ oidx, double* __restrict__ oval) {
    // 8 lanes per row: a wavefront copies 8 rows, consecutive entries by consecutive lanes
    const int g = threadIdx.x & 7;
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 3; r < nrows; r += ((int64_t)gridDim.x * blockDim.x) >> 3) {
        if (flag[r]) continue;
        const int p0 = ptr[r], len = ptr[r + 1] - p0, q0 = sptr[r];
        for (int t = g; t < len; t += 8) { oidx[q0 + t] = idx[p0 + t]; oval[q0 + t] = val[p0 + t]; }
    }
}
__global__ void long_copy_kernel(const int* __restrict__ lrow, const int* __restrict__ loff, const int* __restrict__ ptr, const int* __restrict__ idx,
                                 const double* __restrict__ val, int* __restrict__ lidx, double* __restrict__ lval) {
    const int l = blockIdx.x, r = lrow[l], p0 = ptr[r], len = ptr[r + 1] - p0, q0 = loff[l];
    for (int t = threadIdx.x; t < len; t += blockDim.x) { lidx[q0 + t] = idx[p0 + t]; lval[q0 + t] = val[p0 + t]; }
}
}  // namespace

bool device_strip_long_rows(LayoutScratch& S, GatherMatrix& G, int nrows, const int* dptr, const int* didx, const double* dval,
                            DevBuf<int>& sptr, DevBuf<int>& sidx, DevBuf<double>& sval, int64_t* nnz_short, hipStream_t s) {
    S.stats.ensure(8);
    IPXK_HIP(hipMemsetAsync(S.stats.get(), 0, 8 * sizeof(int), s));
    DevBuf<int> slen((size_t)nrows + 1), list((size_t)kMaxLongRowsDevice);
    G.row_long.ensure((size_t)nrows);
    hipLaunchKernelGGL(long_flag_kernel, dim3(gridn((int64_t)nrows + 1)), dim3(kBlock), 0, s, nrows, dptr, G.row_long.get(), slen.get(), S.stats.get(),
                       list.get(), kMaxLongRowsDevice);
    sptr.ensure((size_t)nrows + 1);
    scan_int(S.T, slen.get(), sptr.get(), (size_t)nrows + 1, s);
    int nl = 0, ns_total = 0;
    IPXK_HIP(hipMemcpyAsync(&nl, S.stats.get(), sizeof(int), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipMemcpyAsync(&ns_total, sptr.get() + nrows, sizeof(int), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
    if (nl <= 0 || nl > kMaxLongRowsDevice) return false;
    std::vector<int> lrow((size_t)nl);
    IPXK_HIP(hipMemcpyAsync(lrow.data(), list.get(), (size_t)nl * sizeof(int), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
    std::sort(lrow.begin(), lrow.end());                       // (the atomic appended them in no particular order)
    // their extents: two words per long row
    DevBuf<int> dl((size_t)nl), ext((size_t)2 * nl);
    dl.upload(lrow, s);
    hipLaunchKernelGGL(row_extent_kernel, dim3(gridn(nl)), dim3(kBlock), 0, s, nl, dl.get(), dptr, ext.get());
    std::vector<int> he((size_t)2 * nl);
    ext.download(he.data(), he.size(), s);
    IPXK_HIP(hipStreamSynchronize(s));
    std::vector<int> sp0, sp1, lslot, loff((size_t)nl);
    int64_t nlong_entries = 0;
    for (int l = 0; l < nl; l++) {
        const int len = he[2 * l + 1] - he[2 * l];
        loff[l] = (int)nlong_entries;
        lslot.push_back((int)sp0.size());
        for (int q0 = 0; q0 < len; q0 += kLongSeg) {
            sp0.push_back((int)(nlong_entries + q0));
            sp1.push_back((int)(nlong_entries + std::min(q0 + kLongSeg, len)));
        }
        nlong_entries += len;
    }
    lslot.push_back((int)sp0.size());
    G.nlong = nl;
    G.nseg = (int)sp0.size();
    G.seg_p0.upload(sp0, s); G.seg_p1.upload(sp1, s); G.long_row.upload(lrow, s); G.long_slot.upload(lslot, s);
    G.lidx.ensure((size_t)nlong_entries); G.lval.ensure((size_t)nlong_entries);
    DevBuf<int> doff((size_t)nl);
    doff.upload(loff, s);
    hipLaunchKernelGGL(long_copy_kernel, dim3(nl), dim3(kBlock), 0, s, dl.get(), doff.get(), dptr, didx, dval, G.lidx.get(), G.lval.get());
    G.long_partials.resize((size_t)std::max(G.nseg, 1));
    G.h_row_long.assign((size_t)nrows, 0);
    for (int r : lrow) G.h_row_long[(size_t)r] = 1;
    sidx.ensure((size_t)std::max(ns_total, 1)); sval.ensure((size_t)std::max(ns_total, 1));
    hipLaunchKernelGGL(strip_copy_kernel, dim3(gridn((int64_t)nrows * 8)), dim3(kBlock), 0, s, nrows, dptr, sptr.get(), G.row_long.get(), didx, dval,
                       sidx.get(), sval.get());
    IPXK_HIP(hipStreamSynchronize(s));                          // the host vectors and temporaries go out of scope
    IPXK_HIP(hipGetLastError());
    *nnz_short = ns_total;
    return true;
}

// ---------------------------------------------------------------------------
// XCD-sliced tiles (the arrays of GatherMatrix::build_sliced with ns_request = 0, bit for bit)
// ---------------------------------------------------------------------------
// returns false when the layout does not apply (x fits an XCD's L2, a tile does not fit LDS, > 255 entries of a row in
// one slice): the caller then takes the host path
bool device_build_sliced(LayoutScratch& S, SlicedMatrix& out, int nrows, int ncols, int64_t nnz, const int* dptr, const int* didx,
                         const double* dval, hipStream_t s, int ns_request) {
    out = SlicedMatrix();
    if (nrows == 0 || nnz == 0 || ncols == 0) return false;
    const Slices sl = model_slices(ncols, ns_request);
    if (sl.fits_l2) return false;
    const int ns = sl.ns;
    const int64_t slice = sl.width;
    RowBlockSearch search = sliced_rows(nrows, ns);
    int R = 0;
    const size_t nz = (size_t)nnz;
    S.k1.ensure(nz); S.k2.ensure(nz); S.v1.ensure(nz); S.v2.ensure(nz); S.stats.ensure(8);
    int nrb = 0, h[4] = {0, 0, 0, 0};
    int64_t ntiles = 0;
    for (;; search.next()) {
        R = search.rows;
        if (search.gave_up()) return false;
        nrb = (nrows + R - 1) / R;
        ntiles = (int64_t)nrb * ns;
        if ((u64)ntiles * (u64)R >= (u64(1) << 32)) return false;         // device only: the sort key (tile, row in tile) has 32 bits
        hipLaunchKernelGGL(sliced_keys_kernel, dim3(gridn(nrows)), dim3(kBlock), 0, s, nrows, dptr, didx, R, ns, (int)slice, S.k1.get(), S.v1.get());
        sort_pairs<unsigned>(S.T, S.k1.get(), S.k2.get(), S.v1.get(), S.v2.get(), nz, bits_for((u64)ntiles * (u64)R - 1), s);
        out.tile_ptr.ensure((size_t)ntiles + 1);
        hipLaunchKernelGGL(lower_bounds_kernel<unsigned>, dim3(gridn(ntiles + 1)), dim3(kBlock), 0, s, ntiles + 1, nnz, S.k2.get(), (u64)R, 0,
                           out.tile_ptr.get());
        IPXK_HIP(hipMemsetAsync(S.stats.get(), 0, 8 * sizeof(int), s));
        hipLaunchKernelGGL(tile_stats_kernel, dim3(gridn(nrb)), dim3(kBlock), 0, s, nrb, ns, out.tile_ptr.get(), S.stats.get());
        IPXK_HIP(hipMemcpyAsync(h, S.stats.get(), sizeof h, hipMemcpyDeviceToHost, s));
        IPXK_HIP(hipStreamSynchronize(s));
        if (search.fits(h[0])) break;
    }
    u64 dom = 0;
    memcpy(&dom, h + 2, sizeof dom);
    out.dominant_fraction = (double)(int64_t)dom / (double)nnz;
    const size_t nslots = (size_t)ntiles * R;
    out.cnt.ensure(nslots); out.idx.ensure(nz); out.val.ensure(nz);
    IPXK_HIP(hipMemsetAsync(out.cnt.get(), 0, nslots, s));
    IPXK_HIP(hipMemsetAsync(S.stats.get(), 0, 8 * sizeof(int), s));
    hipLaunchKernelGGL(run_counts_kernel, dim3(gridn(nnz)), dim3(kBlock), 0, s, nnz, S.k2.get(), out.cnt.get(), S.stats.get());
    hipLaunchKernelGGL(gather_entries_kernel, dim3(gridn(nnz)), dim3(kBlock), 0, s, nnz, S.v2.get(), didx, dval, out.idx.get(), out.val.get());
    int over = 0;
    IPXK_HIP(hipMemcpyAsync(&over, S.stats.get(), sizeof(int), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
    IPXK_HIP(hipGetLastError());
    if (over) { out = SlicedMatrix(); return false; }
    out.R = R; out.nslices = ns; out.nrb = nrb; out.nrows_pad = nrb * R; out.max_tile = h[0];
    out.partial.resize(ns > 1 ? (size_t)ns * out.nrows_pad : 1);
    out.built = true;
    return true;
}

// ---------------------------------------------------------------------------
// accumulated tiles (the arrays of GatherMatrix::build_acc, bit for bit); needs the sliced layout's slices
// ---------------------------------------------------------------------------
// (layout_geometry.hpp; here because it asks the device for its CU count)
int acc_persist_grid(int ns) {
    // IPXK_ACC_PERSIST: unset or 1 = on; 0 = one workgroup per tile; a larger number caps the grid (tests: many tiles per
    // workgroup on small matrices), still rounded down to a multiple of 8 and of ns
    static const int setting = [] { const char* e = getenv("IPXK_ACC_PERSIST"); return e ? std::max(0, atoi(e)) : 1; }();
    if (setting == 0 || ns < 1) return 0;
    static int cus[64] = {};
    int dev = 0;
    IPXK_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) dev = 0;
    if (cus[dev] == 0) IPXK_HIP(hipDeviceGetAttribute(&cus[dev], hipDeviceAttributeMultiprocessorCount, dev));
    const int L = std::lcm(8, ns);
    const int n = setting > 1 ? std::min(setting, cus[dev]) : cus[dev];
    return std::max(L, n / L * L);
}

int acc_rows_per_block(int nrows, int ns) {
    static const int cap = [] { const char* e = getenv("IPXK_ACC_ROWS"); return e && atoi(e) >= 1024 ? std::min(atoi(e), kAccMaxRows) & ~1 : kAccMaxRows; }();
    static const bool balance = !(getenv("IPXK_ACC_BALANCE") && getenv("IPXK_ACC_BALANCE")[0] == '0');   // (0: measuring aid)
    // persistent kernel: as many row blocks as fill every workgroup of the grid equally (a multiple of G / ns), each of
    // ceil(nrows / nrb) rows rounded up to an even number (16-byte partial stores); 1M rows, 8 slices, 256 CUs: 64 blocks of
    // 15626 rows instead of 62 of 16384 (the last one 576 rows) on the second round of 256 workgroups.  Only while that
    // shrinks the row block by at most 1/8 (smaller blocks hold fewer entries per line of a slice: 8192 rows cost 14 % per
    // pass at C3, below); otherwise the rule below
    if (const int G = balance ? acc_persist_grid(ns) : 0) {
        const int64_t per = G / ns;
        const int64_t nrb = (((int64_t)nrows + cap - 1) / cap + per - 1) / per * per;
        int rb = (int)(((int64_t)nrows + nrb - 1) / nrb);
        rb += rb & 1;
        if (rb >= 1024 && 8 * (int64_t)rb >= 7 * (int64_t)cap) return rb;
    }
    int RB = cap;
    // (at least one tile per CU; halving the row block halves the entries per line of the slice and doubles the waiting entries:
    // 1M x 2M with 8192 rows: 107 us per pass, with 16384: 94)
    while (RB > 1024 && ((int64_t)nrows + RB - 1) / RB * (int64_t)ns < 256) RB /= 2;
    return RB;
}

// The step table of the persistent tile kernel from A.tile_batch / A.bptr (both on the device), for the host and the device
// builder alike: fills A.tile_step / steps / nsteps.  IPXK_ACC_STEPS=0: every batch is a step (the schedule without steps;
// A/B runs and the tests' reference).  Synchronizes (the read-back of the step count; the temporary).
// wide (the sliced form, whose persistent kernel reads it): then the wide stream of those steps from A.pack / A.val, unless
// IPXK_ACC_WIDE=0 (the kernel then streams pack / val as before; A/B runs and the tests' reference) -- A.wide_start / wide /
// wide_units.  Not built either when the units could overflow 32 bits (more than 2^21 steps).
// The sliced form (A.nslices is set) with the persistent kernel also gets the head tables of its launch grid (internal.hpp) --
// A.head / head_wide / head_grid -- only with IPXK_ACC_HEAD=1 (measured: no gain, profiles/acc_cold_start.txt; A/B runs and the tests): head from the step table, head_wide
// from the wide stream when that was built.
static void acc_build_head(AccMatrix& A, int64_t ntiles, hipStream_t s) {
    static const bool head_on = [] { const char* e = getenv("IPXK_ACC_HEAD"); return e && atoi(e) != 0; }();
    A.head.release(); A.head_wide.release(); A.head_grid = 0;
    const int P = (int)std::min<int64_t>(acc_persist_grid(A.nslices), ntiles);
    if (!head_on || A.fused || P < 1 || A.nsteps == 0) return;
    A.head.ensure((size_t)P * kAccHeadWords);
    hipLaunchKernelGGL(acc_head_fill_kernel, dim3(gridn(P)), dim3(kBlock), 0, s, P, (int)ntiles, A.tile_step.get(), A.steps.get(),
                       A.wide_units > 0 ? A.wide_start.get() : nullptr, A.head.get());
    if (A.wide_units > 0) {
        A.head_wide.ensure((size_t)P * kAccHeadStreams * 3 * kAccThreads);
        hipLaunchKernelGGL(acc_head_wide_fill_kernel, dim3(P * kAccHeadStreams), dim3(kAccThreads), 0, s, P, A.head.get(), A.wide.get(), A.head_wide.get());
    }
    IPXK_HIP(hipStreamSynchronize(s));
    A.head_grid = P;
}
void acc_build_steps(AccMatrix& A, int64_t ntiles, int64_t nnz, bool wide, hipStream_t s) {
    static const bool merge = !(getenv("IPXK_ACC_STEPS") && getenv("IPXK_ACC_STEPS")[0] == '0');
    static const bool wide_on = !(getenv("IPXK_ACC_WIDE") && getenv("IPXK_ACC_WIDE")[0] == '0');
    static_assert(kAccStepBatches == 4, "a step record holds three cuts");
    const unsigned maxb = merge ? kAccStepBatches : 1;
    DevBuf<unsigned> nstep((size_t)ntiles + 1);
    hipLaunchKernelGGL(acc_step_count_kernel, dim3(gridn(ntiles)), dim3(kBlock), 0, s, (int)ntiles, A.tile_batch.get(), A.bptr.get(), maxb, nstep.get());
    A.tile_step.ensure((size_t)ntiles + 1);
    scan_u32((int)ntiles, nstep.get(), A.tile_step.get(), s);
    unsigned total = 0;
    IPXK_HIP(hipMemcpyAsync(&total, A.tile_step.get() + ntiles, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
    A.steps.ensure((size_t)total + 1);
    hipLaunchKernelGGL(acc_step_fill_kernel, dim3(gridn(ntiles)), dim3(kBlock), 0, s, (int)ntiles, A.tile_batch.get(), A.bptr.get(), maxb,
                       A.tile_step.get(), (unsigned)nnz, A.steps.get());
    IPXK_HIP(hipStreamSynchronize(s));          // nstep goes out of scope
    A.nsteps = total;
    A.wide_start.release(); A.wide.release(); A.wide_units = 0;
    A.head.release(); A.head_wide.release(); A.head_grid = 0;
    if (!wide) return;
    if (!wide_on || total == 0 || total > (1u << 21)) { acc_build_head(A, ntiles, s); return; }
    DevBuf<unsigned> units((size_t)total + 1);
    hipLaunchKernelGGL(acc_wide_count_kernel, dim3(gridn(total)), dim3(kBlock), 0, s, (int)total, A.steps.get(), units.get());
    A.wide_start.ensure((size_t)total + 1);
    scan_u32((int)total, units.get(), A.wide_start.get(), s);
    unsigned nunits = 0;
    IPXK_HIP(hipMemcpyAsync(&nunits, A.wide_start.get() + total, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
    A.wide.ensure((size_t)nunits);
    hipLaunchKernelGGL(acc_wide_fill_kernel, dim3(std::min<unsigned>(total, 8192u)), dim3(kAccThreads), 0, s, (int)total, A.steps.get(),
                       A.wide_start.get(), A.pack.get(), A.val.get(), A.wide.get());
    IPXK_HIP(hipStreamSynchronize(s));          // units goes out of scope
    A.wide_units = nunits;
    acc_build_head(A, ntiles, s);
}

// The tail both accumulated forms share.  On entry S.q2 / S.v2 hold the entries' keys (tile << 18 | offset) and storage positions
// in sorted order, T.rowof the row of every entry in storage order, T.tile_ptr the first sorted entry of each tile.  The entry
// words, the batches of every tile (acc_batch_kernel), the scan of their counts, then batch pointers and the scatter to batch
// order: fills out.tile_batch / bptr / pack / val, nbatches and deferred, then the step table (acc_build_steps).  Synchronizes for
// the read-back of the batch count and in acc_build_steps; the caller synchronizes once more before T goes out of scope.
struct AccTemps {
    DevBuf<int> rowof;
    DevBuf<unsigned> tile_ptr, nbatch, bstart;
    AccTemps(int64_t ntiles, size_t nz) : rowof(nz), tile_ptr((size_t)ntiles + 1), nbatch((size_t)ntiles + 1), bstart(nz) {}
};
static void acc_batches(LayoutScratch& S, AccMatrix& out, AccTemps& T, int64_t ntiles, int RB, int64_t nnz, const double* dval, bool wide,
                        hipStream_t s) {
    const size_t nz = (size_t)nnz;
    unsigned* word = S.k1.get();
    hipLaunchKernelGGL(acc_words_kernel, dim3(gridn(nnz)), dim3(kBlock), 0, s, nnz, S.q2.get(), S.v2.get(), T.rowof.get(), RB, word);
    IPXK_HIP(hipMemsetAsync(S.stats.get(), 0, 8 * sizeof(int), s));
    const size_t lds = (size_t)RB * 2 * sizeof(unsigned);
    IPXK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(acc_batch_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)(kAccMaxRows * 2 * sizeof(unsigned))));
    hipLaunchKernelGGL(acc_batch_kernel, dim3((unsigned)ntiles), dim3(64), lds, s, RB, T.tile_ptr.get(), word, S.k2.get(), S.v3.get(), S.v4.get(),
                       T.bstart.get(), T.nbatch.get(), reinterpret_cast<u64*>(S.stats.get()));
    out.tile_batch.ensure((size_t)ntiles + 1);
    scan_u32((int)ntiles, T.nbatch.get(), out.tile_batch.get(), s);
    unsigned nb_total = 0;
    u64 ndef = 0;
    IPXK_HIP(hipMemcpyAsync(&nb_total, out.tile_batch.get() + ntiles, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipMemcpyAsync(&ndef, S.stats.get(), sizeof(u64), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
    out.bptr.ensure((size_t)nb_total + 1); out.pack.ensure(nz); out.val.ensure(nz);
    hipLaunchKernelGGL(acc_bptr_kernel, dim3((unsigned)ntiles), dim3(64), 0, s, (int)ntiles, T.tile_ptr.get(), out.tile_batch.get(), T.bstart.get(),
                       (unsigned)nnz, out.bptr.get());
    hipLaunchKernelGGL(acc_scatter_kernel, dim3(gridn(nnz)), dim3(kBlock), 0, s, nnz, S.k2.get(), word, S.v2.get(), dval, out.pack.get(),
                       out.val.get());
    out.nbatches = nb_total; out.deferred = (int64_t)ndef;
    acc_build_steps(out, ntiles, nnz, wide, s);
}

// The prologue both fused forms share: smallest and largest gathered index of every tile of RB rows (lo, hi: nrb entries each; lo is
// the tile's xmin afterwards), the rows' count bytes if cnt is given (nrb * RB, zeroed here), and h[0] = widest window, h[1] = most
// entries of a tile, h[2] = a row of more than 255 entries (with cnt), h[3] = a row whose indices do not ascend.  Synchronizes.
static void tile_windows(LayoutScratch& S, int nrows, int nrb, int RB, const int* dptr, const int* didx, int* lo, int* hi, unsigned char* cnt,
                         int h[4], hipStream_t s) {
    IPXK_HIP(hipMemsetAsync(lo, 0x7f, (size_t)nrb * sizeof(int), s));
    IPXK_HIP(hipMemsetAsync(hi, 0xff, (size_t)nrb * sizeof(int), s));
    if (cnt) IPXK_HIP(hipMemsetAsync(cnt, 0, (size_t)nrb * RB, s));
    IPXK_HIP(hipMemsetAsync(S.stats.get(), 0, 8 * sizeof(int), s));
    hipLaunchKernelGGL(tile_window_kernel, dim3(gridn(nrows)), dim3(kBlock), 0, s, nrows, dptr, didx, RB, lo, hi, cnt, S.stats.get() + 2);
    hipLaunchKernelGGL(tile_window_stats_kernel, dim3(gridn(nrb)), dim3(kBlock), 0, s, nrb, nrows, RB, dptr, lo, hi, S.stats.get());
    IPXK_HIP(hipMemcpyAsync(h, S.stats.get(), 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
}

bool device_build_acc(LayoutScratch& S, AccMatrix& out, const SlicedMatrix& sliced, int nrows, int ncols, int64_t nnz, const int* dptr,
                      const int* didx, const double* dval, hipStream_t s) {
    out = AccMatrix();
    if (!sliced.built || sliced.nslices < 2 || nnz == 0) return false;
    const int ns = sliced.nslices;
    const int64_t slice = slice_width(ncols, ns);
    if (!offsets_fit(slice)) return false;
    const int RB = acc_rows_per_block(nrows, ns);
    const int nrb = (nrows + RB - 1) / RB;
    const int64_t ntiles = (int64_t)nrb * ns;
    const size_t nz = (size_t)nnz;
    S.q1.ensure(nz); S.q2.ensure(nz); S.v1.ensure(nz); S.v2.ensure(nz); S.v3.ensure(nz); S.v4.ensure(nz); S.k1.ensure(nz); S.k2.ensure(nz);
    S.stats.ensure(8);
    AccTemps T(ntiles, nz);
    hipLaunchKernelGGL(acc_keys_kernel, dim3(gridn(nrows)), dim3(kBlock), 0, s, nrows, dptr, didx, RB, ns, (int)slice, S.q1.get(), S.v1.get(), T.rowof.get());
    sort_pairs<u64>(S.T, S.q1.get(), S.q2.get(), S.v1.get(), S.v2.get(), nz, kSortedOffBits + bits_for((u64)std::max<int64_t>(ntiles, 2) - 1), s);
    hipLaunchKernelGGL(lower_bounds_kernel<u64>, dim3(gridn(ntiles + 1)), dim3(kBlock), 0, s, ntiles + 1, nnz, S.q2.get(), (u64)1, kSortedOffBits,
                       T.tile_ptr.get());
    // (the geometry first: acc_build_steps sizes the head tables by the slice count)
    out.nslices = ns; out.nrb = nrb; out.RB = RB; out.nrows_pad = nrb * RB; out.slice_elems = (int)slice; out.xlen = ncols;
    acc_batches(S, out, T, ntiles, RB, nnz, dval, true, s);
    IPXK_HIP(hipStreamSynchronize(s));       // the temporaries go out of scope
    IPXK_HIP(hipGetLastError());
    out.partial.resize((size_t)ns * out.nrows_pad);
    out.built = true;
    return true;
}

// ---------------------------------------------------------------------------
// FUSED sorted tiles (the arrays of GatherMatrix::build_sorted_fused, bit for bit)
// ---------------------------------------------------------------------------
bool device_build_sorted_fused(LayoutScratch& S, SortedMatrix& out, int nrows, int ncols, int64_t nnz, const int* dptr, const int* didx,
                               const double* dval, hipStream_t s) {
    out = SortedMatrix();
    if (nrows == 0 || nnz == 0 || ncols == 0) return false;
    const size_t nz = (size_t)nnz;
    S.q1.ensure(nz); S.q2.ensure(nz); S.v1.ensure(nz); S.v2.ensure(nz); S.stats.ensure(8);
    DevBuf<int> lo, hi;
    RowBlockSearch search = sorted_fused_rows(nrows);
    int RB = 0, nrb = 0, h[4] = {0, 0, 0, 0};
    for (;; search.next()) {
        RB = search.rows;
        if (search.gave_up()) return false;
        nrb = (nrows + RB - 1) / RB;
        lo.ensure((size_t)nrb); hi.ensure((size_t)nrb);
        out.cnt.ensure((size_t)nrb * RB);
        tile_windows(S, nrows, nrb, RB, dptr, didx, lo.get(), hi.get(), out.cnt.get(), h, s);
        if (h[2]) { out = SortedMatrix(); return false; }          // a row of more than 255 entries
        if (search.fits(h[1])) break;
    }
    if (!window_fits(h[0])) { out = SortedMatrix(); return false; }
    hipLaunchKernelGGL(fused_keys_kernel, dim3(gridn(nrows)), dim3(kBlock), 0, s, nrows, dptr, didx, RB, lo.get(), S.q1.get(), S.v1.get(), (int*)nullptr);
    sort_pairs<u64>(S.T, S.q1.get(), S.q2.get(), S.v1.get(), S.v2.get(), nz, kSortedOffBits + bits_for((u64)std::max(nrb, 2) - 1), s);
    out.sub_ptr.ensure((size_t)nrb + 1); out.pack.ensure(nz); out.val.ensure(nz); out.xmin.ensure((size_t)nrb);
    hipLaunchKernelGGL(tile_ptr_from_rows_kernel, dim3(gridn(nrb + 1)), dim3(kBlock), 0, s, nrb, nrows, RB, dptr, out.sub_ptr.get());
    hipLaunchKernelGGL(sorted_fused_fill_kernel, dim3(gridn(nnz)), dim3(kBlock), 0, s, nnz, S.q2.get(), S.v2.get(), dptr, RB, dval, out.pack.get(), out.val.get());
    IPXK_HIP(hipMemcpyAsync(out.xmin.get(), lo.get(), (size_t)nrb * sizeof(int), hipMemcpyDeviceToDevice, s));
    IPXK_HIP(hipStreamSynchronize(s));
    IPXK_HIP(hipGetLastError());
    out.nrb = nrb; out.RB = RB; out.nrows_pad = nrb * RB; out.max_sub = h[1];
    out.built = true;
    return true;
}

// ---------------------------------------------------------------------------
// FUSED accumulated tiles (the arrays of GatherMatrix::build_acc_fused, bit for bit)
// ---------------------------------------------------------------------------
bool device_build_acc_fused(LayoutScratch& S, AccMatrix& out, int nrows, int ncols, int64_t nnz, const int* dptr, const int* didx,
                            const double* dval, hipStream_t s) {
    out = AccMatrix();
    if (nrows == 0 || nnz == 0 || ncols == 0) return false;
    const int RB = acc_fused_rows(nrows);
    if (RB == 0) return false;
    const int nrb = (nrows + RB - 1) / RB;
    const size_t nz = (size_t)nnz;
    S.q1.ensure(nz); S.q2.ensure(nz); S.v1.ensure(nz); S.v2.ensure(nz); S.v3.ensure(nz); S.v4.ensure(nz); S.k1.ensure(nz); S.k2.ensure(nz);
    S.stats.ensure(8);
    DevBuf<int> lo((size_t)nrb), hi((size_t)nrb);
    AccTemps T(nrb, nz);
    int h[4] = {0, 0, 0, 0};
    tile_windows(S, nrows, nrb, RB, dptr, didx, lo.get(), hi.get(), nullptr, h, s);
    if (h[3]) return false;                                        // a row with descending indices: the sum would not be in storage order
    if (!window_fits(h[0])) return false;
    hipLaunchKernelGGL(fused_keys_kernel, dim3(gridn(nrows)), dim3(kBlock), 0, s, nrows, dptr, didx, RB, lo.get(), S.q1.get(), S.v1.get(), T.rowof.get());
    sort_pairs<u64>(S.T, S.q1.get(), S.q2.get(), S.v1.get(), S.v2.get(), nz, kSortedOffBits + bits_for((u64)std::max(nrb, 2) - 1), s);
    hipLaunchKernelGGL(tile_ptr_from_rows_kernel, dim3(gridn(nrb + 1)), dim3(kBlock), 0, s, nrb, nrows, RB, dptr, T.tile_ptr.get());
    out.xmin.ensure((size_t)nrb);
    acc_batches(S, out, T, nrb, RB, nnz, dval, false, s);
    IPXK_HIP(hipMemcpyAsync(out.xmin.get(), lo.get(), (size_t)nrb * sizeof(int), hipMemcpyDeviceToDevice, s));
    IPXK_HIP(hipStreamSynchronize(s));
    IPXK_HIP(hipGetLastError());
    out.nslices = 1; out.nrb = nrb; out.RB = RB; out.nrows_pad = nrb * RB; out.slice_elems = 0; out.fused = true;
    out.built = true;
    return true;
}

}  // namespace ipxk
