// The basis path's N N' on the model's gather matrices (internal.hpp: GatherMatrix::mask_values, compact_tiles): a second value
// array of the tile base in which the entries of the columns outside N are zero, and the stream compaction of the tiles to the
// entries of N alone.
#include <algorithm>

#include "context.hpp"

namespace ipxk {

// ---------------------------------------------------------------------------
// masked values (GatherMatrix::mask_values)
// ---------------------------------------------------------------------------
// row of every stored entry.  Both layouts store a unit (tile / step) row by row with one count per row:
// a workgroup scans the counts of its unit and labels the entries.
__global__ __launch_bounds__(kBlock) void rowof_sliced_kernel(SlicedView M, int* __restrict__ rowof) {
    __shared__ int wsum[kBlock / 64];
    const int tile = blockIdx.x, rb = tile / M.nslices, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rpt = M.R / kBlock;
    const unsigned char* cb = M.cnt + (size_t)tile * M.R + (size_t)tid * rpt;
    int mine = 0;
    for (int q = 0; q < rpt; q++) mine += cb[q];
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int p = (int)M.tile_ptr[tile] + incl - mine;
    for (int w = 0; w < wave; w++) p += wsum[w];
    for (int q = 0; q < rpt; q++) {
        const int r = rb * M.R + tid * rpt + q;
        for (int k = 0; k < cb[q]; k++) rowof[p++] = r;
    }
}
__global__ __launch_bounds__(kBlock) void rowof_phased_kernel(GatherView M, int64_t RW, int* __restrict__ rowof) {
    __shared__ int total;
    // one step per workgroup; its rows in order of the count slots (thread-serial scan in chunks of kBlock slots)
    const int64_t st = blockIdx.x;
    const int w = (int)(st % M.G), q = (int)(st / ((int64_t)M.P * M.G));
    const int64_t row0 = (int64_t)q * M.G * M.RWrows + (int64_t)w * M.RWrows;
    __shared__ int wsum[kBlock / 64];
    int base = M.step_ptr[st];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t l0 = 0; l0 < RW; l0 += kBlock) {
        const int64_t lr = l0 + tid;
        const int mine = lr < RW ? M.counts[(size_t)st * RW + lr] : 0;
        int incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int p = base + incl - mine;
        for (int ww = 0; ww < wave; ww++) p += wsum[ww];
        for (int k = 0; k < mine; k++) rowof[p + k] = (int)(row0 + lr);
        if (tid == kBlock - 1) total = p + mine;
        __syncthreads();
        base = total;
        __syncthreads();
    }
}
__global__ void mask_values_kernel(int64_t nz, const double* __restrict__ val, const int* __restrict__ key,
                                   const double* __restrict__ weight, double* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nz; e += (int64_t)gridDim.x * blockDim.x)
        out[e] = weight[key[e]] != 0.0 ? val[e] : 0.0;
}
__global__ void mask_long_rows_kernel(GatherView M, const double* __restrict__ weight, int by_row, double* __restrict__ out) {
    const int l = blockIdx.x;
    const int r = M.long_row[l];
    for (int sgm = M.long_slot[l]; sgm < M.long_slot[l + 1]; sgm++)
        for (int p = M.seg_p0[sgm] + threadIdx.x; p < M.seg_p1[sgm]; p += blockDim.x)
            out[p] = weight[by_row ? r : M.lidx[p]] != 0.0 ? M.lval[p] : 0.0;
}

void GatherMatrix::mask_values(const double* weight, bool by_row, hipStream_t s) {
    const bool tiles = tile_base() != SpmvLayout::phased;
    const int64_t nz = tiles ? (int64_t)sliced.idx.size() : (int64_t)idx.size();
    const int* gidx = tiles ? sliced.idx.get() : idx.get();
    const double* gval = tiles ? sliced.val.get() : val.get();
    if (by_row && rowof.size() == 0 && nz > 0) {
        rowof.resize((size_t)nz);
        IPXK_HIP(hipMemsetAsync(rowof.get(), 0, (size_t)nz * sizeof(int), s));
        if (tiles) {
            const SlicedView V = sliced_view();
            hipLaunchKernelGGL(rowof_sliced_kernel, dim3(V.nrb * V.nslices), dim3(kBlock), 0, s, V, rowof.get());
        } else {
            const GatherView V = view();
            const int64_t nsteps = (int64_t)Q * P * G;
            hipLaunchKernelGGL(rowof_phased_kernel, dim3((unsigned)nsteps), dim3(kBlock), 0, s, V, (int64_t)kBlock * RT, rowof.get());
        }
    }
    valM.ensure((size_t)std::max<int64_t>(nz, 1));
    if (nz > 0)
        hipLaunchKernelGGL(mask_values_kernel, dim3((unsigned)std::min<int64_t>(4096, (nz + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, nz, gval,
                           by_row ? rowof.get() : gidx, weight, valM.get());
    if (nlong > 0) {
        lvalM.ensure(lval.size());
        hipLaunchKernelGGL(mask_long_rows_kernel, dim3(nlong), dim3(kBlock), 0, s, view(), weight, by_row ? 1 : 0, lvalM.get());
    }
    IPXK_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------
// compacted tiles (GatherMatrix::compact_tiles)
// ---------------------------------------------------------------------------
// kept entries per row of the tile and per tile; one workgroup per tile.  wkey[e] addresses the weight of
// entry e (its row in the gather matrix, or its gathered index), rowof[e] its row.
__global__ __launch_bounds__(kBlock) void compact_count_kernel(SlicedView M, const int* __restrict__ rowof,
                                                               const int* __restrict__ wkey, const double* __restrict__ weight,
                                                               unsigned char* __restrict__ cnt_out, unsigned* __restrict__ tile_kept) {
    __shared__ int rowcnt[kSlicedRows];
    __shared__ int wsum[kBlock / 64];
    const int tile = blockIdx.x, rb = tile / M.nslices, tid = threadIdx.x;
    for (int r = tid; r < M.R; r += kBlock) rowcnt[r] = 0;
    __syncthreads();
    const unsigned e0 = M.tile_ptr[tile], e1 = M.tile_ptr[tile + 1];
    int mine = 0;
    for (unsigned e = e0 + tid; e < e1; e += kBlock)
        if (weight[wkey[e]] != 0.0) { atomicAdd(&rowcnt[rowof[e] - rb * M.R], 1); mine++; }
    __syncthreads();
    for (int r = tid; r < M.R; r += kBlock) cnt_out[(size_t)tile * M.R + r] = (unsigned char)rowcnt[r];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0) { int t = 0; for (int w = 0; w < kBlock / 64; w++) t += wsum[w]; tile_kept[tile] = (unsigned)t; }
}
// the kept entries of a tile, in order, to their new place; one workgroup per tile
__global__ __launch_bounds__(kBlock) void compact_fill_kernel(SlicedView M, const int* __restrict__ wkey, const double* __restrict__ weight,
                                                              const unsigned* __restrict__ new_ptr, int* __restrict__ idx_out,
                                                              double* __restrict__ val_out) {
    __shared__ int wsum[kBlock / 64];
    const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned e0 = M.tile_ptr[tile], e1 = M.tile_ptr[tile + 1];
    unsigned base = new_ptr[tile];
    for (unsigned c0 = e0; c0 < e1; c0 += kBlock) {
        const unsigned e = c0 + tid;
        const bool keep = e < e1 && weight[wkey[e]] != 0.0;
        const unsigned long long b = __ballot(keep);
        const int before = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = __popcll(b);
        __syncthreads();
        int wbefore = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; w++) { if (w < wave) wbefore += wsum[w]; total += wsum[w]; }
        if (keep) {
            idx_out[base + wbefore + before] = M.idx[e];
            val_out[base + wbefore + before] = M.val[e];
        }
        base += (unsigned)total;
        __syncthreads();
    }
}

void GatherMatrix::compact_tiles(const double* weight, bool by_row, hipStream_t s) {
    compact.valid = false;
    if (tile_base() == SpmvLayout::phased) return;
    const int64_t nz = (int64_t)sliced.idx.size();
    const SlicedView V = sliced_view(0);
    const int ntiles = V.nrb * V.nslices;
    if (nz == 0 || ntiles == 0) return;
    if (rowof.size() == 0) {
        rowof.resize((size_t)nz);
        IPXK_HIP(hipMemsetAsync(rowof.get(), 0, (size_t)nz * sizeof(int), s));
        hipLaunchKernelGGL(rowof_sliced_kernel, dim3(ntiles), dim3(kBlock), 0, s, V, rowof.get());
    }
    compact.tile_ptr.ensure((size_t)ntiles + 1);
    compact.tile_kept.ensure((size_t)ntiles);
    compact.cnt.ensure((size_t)ntiles * V.R);
    compact.idx.ensure((size_t)nz);
    compact.val.ensure((size_t)nz);
    const int* wkey = by_row ? rowof.get() : sliced.idx.get();
    hipLaunchKernelGGL(compact_count_kernel, dim3(ntiles), dim3(kBlock), 0, s, V, rowof.get(), wkey, weight, compact.cnt.get(),
                       compact.tile_kept.get());
    scan_u32(ntiles, compact.tile_kept.get(), compact.tile_ptr.get(), s);
    hipLaunchKernelGGL(compact_fill_kernel, dim3(ntiles), dim3(kBlock), 0, s, V, wkey, weight, compact.tile_ptr.get(),
                       compact.idx.get(), compact.val.get());
    IPXK_HIP(hipGetLastError());
    if (nlong > 0) {           // long rows stay with their masked values
        lvalM.ensure(lval.size());
        hipLaunchKernelGGL(mask_long_rows_kernel, dim3(nlong), dim3(kBlock), 0, s, view(), weight, by_row ? 1 : 0, lvalM.get());
        IPXK_HIP(hipGetLastError());
    }
    compact.valid = true;
}

}  // namespace ipxk
