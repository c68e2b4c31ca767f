// Device-side helpers: wave64 / workgroup reductions with a fixed combination
// tree (results are run-to-run reproducible; no atomics anywhere).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>

#include "internal.hpp"

// grid-stride loop of an elementwise kernel (the grid: grid_for / vec_grid, internal.hpp)
#define IPXK_GRID_STRIDE(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

namespace ipxk {

template <class T>
__global__ void fill_kernel(int64_t n, T v, T* __restrict__ a) { IPXK_GRID_STRIDE(i, n) a[i] = v; }

// exclusive prefix sum of n counts by ONE workgroup of kThreads threads (n = # tiles, a few thousand); out[n] = their sum
template <int kThreads>
__global__ __launch_bounds__(kThreads) void scan_u32_kernel(int n, const unsigned* __restrict__ in, unsigned* __restrict__ out) {
    __shared__ unsigned wsum[kThreads / 64];
    __shared__ unsigned carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += kThreads) {
        const int i = base + tid;
        const unsigned v = i < n ? in[i] : 0u;
        unsigned incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const unsigned t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned before = carry;
        for (int w = 0; w < wave; w++) before += wsum[w];
        if (i < n) out[i] = before + incl - v;
        __syncthreads();
        if (tid == kThreads - 1) carry = before + incl;
        __syncthreads();
    }
    if (tid == 0) out[n] = carry;
}
// (a template so that only the files that call it instantiate the kernel)
template <int kThreads = 1024>
void scan_u32(int n, const unsigned* in, unsigned* out, hipStream_t s) {
    hipLaunchKernelGGL(scan_u32_kernel<kThreads>, dim3(1), dim3(kThreads), 0, s, n, in, out);
}

struct SumOp {
    static __device__ __forceinline__ double identity() { return 0.0; }
    static __device__ __forceinline__ double apply(double a, double b) { return a + b; }
};
struct MaxOp {
    static __device__ __forceinline__ double identity() { return 0.0; }  // norms are >= 0
    // NaN-propagating max so that a NaN residual cannot pass the tolerance test
    static __device__ __forceinline__ double apply(double a, double b) {
        return (a != a) ? a : ((b != b) ? b : (a > b ? a : b));
    }
};
struct MinOp {
    static __device__ __forceinline__ double identity() { return __builtin_huge_val(); }
    static __device__ __forceinline__ double apply(double a, double b) { return a < b ? a : b; }
};

template <class Op>
__device__ __forceinline__ double wave_reduce(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = Op::apply(v, __shfl_xor(v, off, 64));
    return v;
}

// The same butterfly (offset kWidth/2 down to 1, v = op(v, other)) for any element type, over the kWidth consecutive lanes
// that share the lane index's high bits (64: the wavefront; 32 / 16: the sub-wave groups of the triangular solves).
struct AddOp {
    template <class T> static __device__ __forceinline__ T apply(T a, T b) { return a + b; }
};
struct PlainMaxOp {       // the overloaded max of the element type: unlike MaxOp, a NaN does not propagate
    template <class T> static __device__ __forceinline__ T apply(T a, T b) { return max(a, b); }
};
struct FmaxOp {
    static __device__ __forceinline__ double apply(double a, double b) { return fmax(a, b); }
};
template <class Op, int kWidth, class T>
__device__ __forceinline__ T wave_reduce(T v) {
#pragma unroll
    for (int off = kWidth / 2; off > 0; off >>= 1) v = Op::apply(v, __shfl_xor(v, off, 64));
    return v;
}
template <int kWidth = 64, class T>
__device__ __forceinline__ T wave_sum(T v) { return wave_reduce<AddOp, kWidth>(v); }
// several sums at once, in place, the butterflies interleaved step by step
template <int kWidth = 64, class... T>
__device__ __forceinline__ void wave_sum_each(T&... v) {
#pragma unroll
    for (int off = kWidth / 2; off > 0; off >>= 1) ((v += __shfl_xor(v, off, 64)), ...);
}
template <int kWidth = 64, class T>
__device__ __forceinline__ T wave_max(T v) { return wave_reduce<PlainMaxOp, kWidth>(v); }

// The indexed best: (value, index), larger value wins, equal values: smaller index wins -- every pivot search and arg max of
// the project (the reference's loops take the first strictly larger entry).  take_smaller is its mirror for the step to the
// boundary.  "No candidate" is (0.0, INT_MAX) resp. (the bound, one past the last index).
__device__ __forceinline__ void take_larger(double& v, int& i, double ov, int oi) {
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}
__host__ __device__ __forceinline__ void take_smaller(double& v, int& i, double ov, int oi) {   // host: step_to_boundary_dev's fold
    if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
}
template <int kWidth = 64>
__device__ __forceinline__ void wave_argmax(double& v, int& i) {
#pragma unroll
    for (int d = kWidth / 2; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(v, d, 64);
        const int oi = __shfl_xor(i, d, 64);
        take_larger(v, i, ov, oi);
    }
}
__device__ __forceinline__ void wave_argmin(double& v, int& i) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ov = __shfl_xor(v, d, 64);
        const int oi = __shfl_xor(i, d, 64);
        take_smaller(v, i, ov, oi);
    }
}

// The partial of a two-stage reduction (Partial<kBest>, internal.hpp: kBest indexed bests, a sum and a count).  Stage one: every workgroup writes
// block_partial of its threads' values to part[blockIdx.x]; stage two: one workgroup whose thread k holds partial k
// (load_partial) calls block_partial again.  The number of workgroups of stage one is part of the summation order.
template <int kBest>
__device__ __forceinline__ Partial<kBest> partial_identity() {
    Partial<kBest> p;
#pragma unroll
    for (int b = 0; b < kBest; b++) { p.v[b] = 0.0; p.i[b] = INT_MAX; }
    p.s = 0.0;
    p.c = 0;
    return p;
}
// the workgroup's partial: wavefront trees, then the wavefronts in order; valid in thread 0.  (The shared array is one per
// instantiation: a barrier between two calls in one kernel.)
template <int kThreads, int kBest>
__device__ __forceinline__ Partial<kBest> block_partial(Partial<kBest> p) {
    __shared__ Partial<kBest> sh[kThreads / 64];
#pragma unroll
    for (int b = 0; b < kBest; b++) wave_argmax(p.v[b], p.i[b]);
    p.s = wave_sum(p.s);
    p.c = wave_sum(p.c);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < kThreads / 64; k++) {
#pragma unroll
            for (int b = 0; b < kBest; b++) take_larger(p.v[b], p.i[b], sh[k].v[b], sh[k].i[b]);
            p.s += sh[k].s;
            p.c += sh[k].c;
        }
    return p;
}
// the indexed best alone
template <int kThreads>
__device__ __forceinline__ void block_argmax(double& v, int& i) {
    __shared__ double sv[kThreads / 64];
    __shared__ int si[kThreads / 64];
    wave_argmax(v, i);
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = i; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < kThreads / 64; k++) take_larger(v, i, sv[k], si[k]);
}
// thread k holds partial k, the identity beyond nparts
template <int kBest>
__device__ __forceinline__ Partial<kBest> load_partial(int nparts, const Partial<kBest>* part) {
    return (int)threadIdx.x < nparts ? part[threadIdx.x] : partial_identity<kBest>();
}

// All kBlock threads call; every thread receives the result.  `scratch` is a
// workgroup-shared array of at least kBlock/64 + 1 doubles.
template <class Op>
__device__ __forceinline__ double block_reduce(double v, double* scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = wave_reduce<Op>(v);
    __syncthreads();  // scratch may still be read by a previous call
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    double r = scratch[0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; w++) r = Op::apply(r, scratch[w]);
    return r;
}

// Reduces `count` per-workgroup partials written by an EARLIER kernel on the
// same stream.  Every workgroup of the consumer kernel calls this and obtains
// the bitwise identical value (fixed order: strided per thread, then the block
// tree) -- this replaces a separate "finalize" launch per scalar.
// `stride` > 1 addresses one scalar per rank in the all-gathered array of a
// multi-GPU run (comm.hip); single GPU: the producer's partial array, stride 1.
struct PartRef {
    const double* p;
    int count;
    int stride;
};

// A thread's partials are i = threadIdx.x, threadIdx.x + kBlock, ...: at most kPartialsPerThread of them, since no producer
// runs more than kMaxPartials workgroups.  Taken one by one each load waits for the one before (a round trip to L2 per
// partial), so the reduction is split: load_partials issues all of a thread's loads at once, from indices clamped to the
// last partial so that they need no predicate (part.p[0] is read even when count == 0); fold_partials then applies Op in ascending
// i to the partials below count, the order of the plain loop.  A kernel may issue the loads long before it folds them.
constexpr int kPartialsPerThread = kMaxPartials / kBlock;

__device__ __forceinline__ void load_partials(PartRef part, double (&v)[kPartialsPerThread]) {
    const int last = max(part.count - 1, 0);
#pragma unroll
    for (int j = 0; j < kPartialsPerThread; j++)
        v[j] = part.p[(size_t)min((int)threadIdx.x + j * kBlock, last) * part.stride];
}
template <class Op>
__device__ __forceinline__ double fold_partials(PartRef part, const double (&v)[kPartialsPerThread]) {
    double r = Op::identity();
#pragma unroll
    for (int j = 0; j < kPartialsPerThread; j++)
        if ((int)threadIdx.x + j * kBlock < part.count) r = Op::apply(r, v[j]);
    for (int i = threadIdx.x + kMaxPartials; i < part.count; i += kBlock)     // (no caller has that many)
        r = Op::apply(r, part.p[(size_t)i * part.stride]);
    return r;
}

template <class Op>
__device__ __forceinline__ double reduce_partials(PartRef part, double* scratch) {
    double v[kPartialsPerThread];
    load_partials(part, v);
    return block_reduce<Op>(fold_partials<Op>(part, v), scratch);
}

// Two reductions at once: block_reduce of va under OpA and of vb under OpB, each through its own unchanged tree and its own
// scratch array, behind one pair of barriers.
template <class OpA, class OpB>
__device__ __forceinline__ void block_reduce2(double& va, double& vb, double* scratch_a, double* scratch_b) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    va = wave_reduce<OpA>(va);
    vb = wave_reduce<OpB>(vb);
    __syncthreads();  // the scratch arrays may still be read by a previous call
    if (lane == 0) { scratch_a[wave] = va; scratch_b[wave] = vb; }
    __syncthreads();
    double ra = scratch_a[0], rb = scratch_b[0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; w++) { ra = OpA::apply(ra, scratch_a[w]); rb = OpB::apply(rb, scratch_b[w]); }
    va = ra;
    vb = rb;
}
// reduce_partials of two PartRefs: both sets of loads in flight together, each value through its own strided-then-tree order
template <class OpA, class OpB>
__device__ __forceinline__ void reduce_partials2(PartRef a, PartRef b, double* scratch_a, double* scratch_b, double& ra,
                                                 double& rb) {
    double va[kPartialsPerThread], vb[kPartialsPerThread];
    load_partials(a, va);
    load_partials(b, vb);
    ra = fold_partials<OpA>(a, va);
    rb = fold_partials<OpB>(b, vb);
    block_reduce2<OpA, OpB>(ra, rb, scratch_a, scratch_b);
}

}  // namespace ipxk
