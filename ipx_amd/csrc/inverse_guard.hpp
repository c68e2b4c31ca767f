// Guard of every explicit inverse (round 4): shared by the inverted blocks of a sweep (sweep_blocks.hip) and the dense
// bump (dense_bump.hip), each with probe kernels of its own.
#pragma once

#include "context.hpp"

namespace ipxk {

// IPX's late bases are ill conditioned by construction (that is why src/basis.cc:130-152 has a stability loop and
// src/lu_factorization.cc:87-127 a residual test): substitution with a triangular factor is backward stable whatever
// its condition, a product with its computed INVERSE is not (error ~ cond * eps).  So every inverse computed at
// Prepare is probed with two fixed vectors z:  || T (M z) - z ||_inf / || z ||_inf  must not exceed the tolerance
// (IPXK_INVERSE_TOL; default 1e-10 for the inverted levels of a sweep, 1e-8 for a dense block); a block that fails keeps its
// level-scheduled / blocked solve.
// Dense blocks of the factors (hundreds to thousands of rows of a dense LU) get 1e-8: || D X - I || of a computed inverse is
// ~ cond(D) * eps whoever computes it -- measured on well conditioned 1024 / 2048 / 4096 / 8000-row blocks: 9e-12 / 2e-10 /
// 8e-10 / 2e-9 by recursive doubling on the matrix cores, 3e-12 / 8e-11 / 1e-10 by one substitution per column (what a
// dtrsm does) -- and an inverse that good perturbs the solves far below every tolerance the IPM asks of a KKT solve
// (0.3 * sqrt(mu), src/ipm.cc:572); the catastrophes the guard is there for are orders of magnitude above it.
inline double inverse_tol(bool dense_block = false) {           // (read per Prepare: the tests switch it)
    const char* e = getenv("IPXK_INVERSE_TOL");
    return e ? atof(e) : dense_block ? 1e-8 : 1e-10;
}
__device__ __forceinline__ double probe_z(int q, int l) {       // entries in [0.5, 1.5], two unrelated sign patterns
    const unsigned h = (unsigned)l * 2654435761u + (unsigned)q * 40503u;
    const double mag = 0.5 + (double)((h >> 9) & 1023u) / 1024.0;
    return ((h >> 20) ^ (unsigned)(q * l)) & 1u ? -mag : mag;
}
__device__ __forceinline__ void probe_max(double* slot, double v) {   // maximum of non-negative doubles through their bit patterns
    if (!(v == v)) v = __builtin_huge_val();                           // a NaN residual fails the test
    atomicMax(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)__double_as_longlong(v));
}
// (z has entries of magnitude in [0.5, 1.5]: || z ||_inf is between 1 and 1.5 for any block of a few rows, the residuals are taken as they are)
// One probe: zeroes the two residual slots res[0..1] (device), lets `enqueue` put the probe's launches on the stream, reads
// the slots back and returns the larger residual.
template <class F>
double probe_residual(hipStream_t s, double* res, F enqueue) {
    IPXK_HIP(hipMemsetAsync(res, 0, 2 * sizeof(double), s));
    enqueue();
    double h[2] = {0.0, 0.0};
    IPXK_HIP(hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
    return std::max(h[0], h[1]);
}
// the verdict on an inverse whose last probe left `resid` (Context::split_stats; the probes are counted where they are made)
inline void record_verdict(Context* c, double resid, bool accepted) {
    c->split_stats.worst_probe = std::max(c->split_stats.worst_probe, resid);
    if (!accepted) c->split_stats.inverse_rejected++;
}

}  // namespace ipxk
