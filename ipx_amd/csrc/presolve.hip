// Model upload on the device: the two array transformations that define the
// solver-form matrix before the path starts,
//   Presolver::EquilibrateMatrix        reference src/presolver.cc:868-974
//   Transpose (AI -> AIt)               reference src/sparse_matrix.cc:120-151
// Both are exact arithmetic (maxima, powers of two, index permutations), so the results are bit-identical to
// the reference's whatever the order of evaluation.  Each is a routine on device-resident arrays (equilibrate_resident here,
// device_transpose in model.hip: what the user model of user_model.hip calls) and a stand-alone entry point on host arrays
// around it (no context: the context is created FROM their output).
#include <hip/hip_runtime.h>

#include <cmath>

#include "layout_scratch.hpp"

namespace ipxk {

namespace {

constexpr int kExpMin = 0, kExpMax = 3, kMaxRound = 10;     // src/presolver.cc:906-908

__device__ __forceinline__ double equilibration_factor(int exp) {   // :868-880
    if (exp < kExpMin) return ldexp(1.0, (kExpMin - exp + 1) / 2);
    if (exp > kExpMax) return ldexp(1.0, -((exp - kExpMax + 1) / 2));
    return 1.0;
}

// :912-924  is any entry outside [2^(expmin-1), 2^expmax) ?
__global__ void out_of_range_kernel(int64_t nz, const double* __restrict__ Ax, int* flag) {
    IPXK_GRID_STRIDE(p, nz) {
        int exp;
        frexp(fabs(Ax[p]), &exp);
        if (exp < kExpMin || exp > kExpMax) *flag = 1;
    }
}
// :934-944  infinity norm of each column and row.  A maximum of non-negative doubles is the maximum of
// their bit patterns as unsigned integers: exact and independent of the order, so an atomic max serves.
template <class P>       // P: the type of the column pointers (ipxint as uploaded, int in a context's plain copy)
__global__ void col_row_max_kernel(int64_t n, const P* __restrict__ Ap, const int* __restrict__ Ai,
                                   const double* __restrict__ Ax, double* __restrict__ colmax,
                                   unsigned long long* rowmax_bits) {
    IPXK_GRID_STRIDE(j, n) {
        double cm = 0.0;
        for (P p = Ap[j]; p < Ap[j + 1]; p++) {
            const double xa = fabs(Ax[p]);
            cm = xa > cm ? xa : cm;
            atomicMax(rowmax_bits + Ai[p], (unsigned long long)__double_as_longlong(xa));
        }
        colmax[j] = cm;
    }
}
// :946-964  this round's factors; accumulates them into the scaling vectors
__global__ void factors_kernel(int64_t len, double* __restrict__ mx, double* __restrict__ scale, int* out_of_range) {
    IPXK_GRID_STRIDE(i, len) {
        int exp;
        frexp(mx[i], &exp);
        const double f = equilibration_factor(exp);
        mx[i] = f;
        if (f != 1.0) { *out_of_range = 1; scale[i] *= f; }
    }
}
// :967-972
template <class P>
__global__ void rescale_kernel(int64_t n, const P* __restrict__ Ap, const int* __restrict__ Ai,
                               double* __restrict__ Ax, const double* __restrict__ colf, const double* __restrict__ rowf) {
    IPXK_GRID_STRIDE(j, n) {
        const double cf = colf[j];
        for (P p = Ap[j]; p < Ap[j + 1]; p++) {
            double v = Ax[p];
            v *= cf;              // column scaling
            v *= rowf[Ai[p]];     // row scaling
            Ax[p] = v;
        }
    }
}

__global__ void narrow_index_kernel(int64_t nz, const ipxint* __restrict__ in, int* __restrict__ out, int limit, int* bad) {
    IPXK_GRID_STRIDE(p, nz) {
        const ipxint v = in[p];
        if (v < 0 || v >= limit) *bad = 1;
        out[p] = (int)v;
    }
}

struct DeviceGuard {       // binds the device for the call, own stream
    hipStream_t s = nullptr;
    explicit DeviceGuard(int device) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count < 1) throw Error(IPXK_E_HIP, "no HIP device");
        IPXK_REQUIRE(device >= 0 && device < count, "device index out of range");
        IPXK_HIP(hipSetDevice(device));
        IPXK_HIP(hipStreamCreate(&s));
    }
    ~DeviceGuard() { if (s) (void)hipStreamDestroy(s); }
};

void check_csc(int64_t m, int64_t n, const ipxint* Ap) {
    IPXK_REQUIRE(m >= 0 && n >= 0 && m < (int64_t(1) << 31) - 1 && n < (int64_t(1) << 31) - 1, "dimension out of range");
    IPXK_REQUIRE(Ap[0] == 0, "colptr[0] must be 0");
    for (int64_t j = 0; j < n; j++) IPXK_REQUIRE(Ap[j] <= Ap[j + 1], "colptr not monotone");
    IPXK_REQUIRE(Ap[n] < (int64_t(1) << 31) - 1, "nnz exceeds 32-bit device indices");
}

}  // namespace

// EquilibrateMatrix on resident arrays: Ax[nz] is scaled in place, cs[n] and rs[m] receive the accumulated factors (1 where
// none), *rounds as ipxk_equilibrate's.  Row indices must be in range.  One flag crosses to the host per round.
template <class P>
void equilibrate_resident(int64_t m, int64_t n, int64_t nz, const P* dAp, const int* dAi, double* dAx, double* cs, double* rs,
                          ipxint* rounds, hipStream_t s) {
    DevBuf<int> flags(1);
    DevBuf<double> cmax((size_t)std::max<int64_t>(n, 1)), rmax((size_t)std::max<int64_t>(m, 1));
    IPXK_HIP(hipMemsetAsync(flags.get(), 0, sizeof(int), s));
    if (nz > 0) hipLaunchKernelGGL(out_of_range_kernel, dim3(grid_for(nz)), dim3(kBlock), 0, s, nz, dAx, flags.get());
    hipLaunchKernelGGL(fill_kernel<double>, dim3(grid_for(n)), dim3(kBlock), 0, s, n, 1.0, cs);
    hipLaunchKernelGGL(fill_kernel<double>, dim3(grid_for(m)), dim3(kBlock), 0, s, m, 1.0, rs);
    int out = 0;
    flags.download(&out, 1, s);
    *rounds = -1;
    if (out) {                                            // :926-973
        *rounds = 0;
        for (int round = 0; round < kMaxRound; round++) {
            IPXK_HIP(hipMemsetAsync(rmax.get(), 0, sizeof(double) * (size_t)std::max<int64_t>(m, 1), s));
            IPXK_HIP(hipMemsetAsync(flags.get(), 0, sizeof(int), s));
            hipLaunchKernelGGL(col_row_max_kernel<P>, dim3(grid_for(n)), dim3(kBlock), 0, s, n, dAp, dAi, dAx, cmax.get(),
                               reinterpret_cast<unsigned long long*>(rmax.get()));
            hipLaunchKernelGGL(factors_kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, m, rmax.get(), rs, flags.get());
            hipLaunchKernelGGL(factors_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, n, cmax.get(), cs, flags.get());
            out = 0;
            flags.download(&out, 1, s);
            if (!out) break;
            hipLaunchKernelGGL(rescale_kernel<P>, dim3(grid_for(n)), dim3(kBlock), 0, s, n, dAp, dAi, dAx, cmax.get(), rmax.get());
            (*rounds)++;
        }
    }
    IPXK_HIP(hipStreamSynchronize(s));                    // the temporaries go out of scope
    IPXK_HIP(hipGetLastError());
}
template void equilibrate_resident<int>(int64_t, int64_t, int64_t, const int*, const int*, double*, double*, double*, ipxint*, hipStream_t);

void equilibrate_device(int device, int64_t m, int64_t n, const ipxint* Ap, const ipxint* Ai, double* Ax,
                        double* colscale, double* rowscale, ipxint* rounds) {
    check_csc(m, n, Ap);
    DeviceGuard dev(device);
    hipStream_t s = dev.s;
    const int64_t nz = Ap[n];
    DevBuf<ipxint> dAp, dAi64;
    DevBuf<int> dAi((size_t)std::max<int64_t>(nz, 1)), bad(1);
    DevBuf<double> dAx, cs((size_t)std::max<int64_t>(n, 1)), rs((size_t)std::max<int64_t>(m, 1));
    dAp.upload(Ap, (size_t)n + 1, s);
    dAi64.upload(Ai, (size_t)nz, s);
    dAx.upload(Ax, (size_t)nz, s);
    IPXK_HIP(hipMemsetAsync(bad.get(), 0, sizeof(int), s));
    if (nz > 0) hipLaunchKernelGGL(narrow_index_kernel, dim3(grid_for(nz)), dim3(kBlock), 0, s, nz, dAi64.get(), dAi.get(), (int)m, bad.get());
    int flag = 0;
    bad.download(&flag, 1, s);
    IPXK_REQUIRE(flag == 0, "row index out of range");
    equilibrate_resident<ipxint>(m, n, nz, dAp.get(), dAi.get(), dAx.get(), cs.get(), rs.get(), rounds, s);
    if (*rounds >= 0) dAx.download(Ax, (size_t)nz, s);
    cs.download(colscale, (size_t)n, s);
    rs.download(rowscale, (size_t)m, s);
    IPXK_HIP(hipStreamSynchronize(s));
    IPXK_HIP(hipGetLastError());
}

// the host-array form of device_transpose (model.hip): upload, narrow, transpose, widen, download
void transpose_device(int device, int64_t m, int64_t n, const ipxint* Ap, const ipxint* Ai, const double* Ax,
                      ipxint* Tp, ipxint* Ti, double* Tx) {
    check_csc(m, n, Ap);
    DeviceGuard dev(device);
    hipStream_t s = dev.s;
    const int64_t nz = Ap[n];
    const size_t nz1 = (size_t)std::max<int64_t>(nz, 1);
    DevBuf<ipxint> dAp, dAi64, wide(std::max(nz1, (size_t)m + 1));
    DevBuf<int> ap32((size_t)n + 1), rows(nz1), tp32((size_t)m + 1), ti32(nz1), bad(1);
    DevBuf<double> dAx, dTx(nz1);
    dAp.upload(Ap, (size_t)n + 1, s);
    dAi64.upload(Ai, (size_t)nz, s);
    dAx.upload(Ax, (size_t)nz, s);
    IPXK_HIP(hipMemsetAsync(bad.get(), 0, sizeof(int), s));
    narrow_ints(n + 1, dAp.get(), ap32.get(), s);
    if (nz > 0) hipLaunchKernelGGL(narrow_index_kernel, dim3(grid_for(nz)), dim3(kBlock), 0, s, nz, dAi64.get(), rows.get(), (int)m, bad.get());
    int flag = 0;
    bad.download(&flag, 1, s);
    IPXK_REQUIRE(flag == 0, "row index out of range");
    if (nz > 0) {
        Tmp T;
        DevBuf<int> colof;
        device_transpose(T, colof, n, m, nz, ap32.get(), rows.get(), dAx.get(), tp32.get(), ti32.get(), dTx.get(), s);
    } else {
        IPXK_HIP(hipMemsetAsync(tp32.get(), 0, ((size_t)m + 1) * sizeof(int), s));
    }
    widen_ints(m + 1, tp32.get(), wide.get(), s);
    wide.download(Tp, (size_t)m + 1, s);
    if (nz > 0) {
        widen_ints(nz, ti32.get(), wide.get(), s);
        wide.download(Ti, (size_t)nz, s);
        dTx.download(Tx, (size_t)nz, s);
    }
    IPXK_HIP(hipStreamSynchronize(s));
    IPXK_HIP(hipGetLastError());
}

}  // namespace ipxk
