// The dense bump of an LU from the device (SplitOperator::DenseBump, trisolve.hpp): the cut of the trailing dense block
// out of the factors at Prepare, its explicit inverse with the guard, and the solve between the two sweeps of a pair.
#include "context.hpp"
#include "inverse_guard.hpp"
#include "trisolve.hpp"

namespace ipxk {

// ---------------------------------------------------------------------------
// The dense bump of an LU from the device (SplitOperator::DenseBump, trisolve.hpp)
// ---------------------------------------------------------------------------
constexpr int kBumpMin = 32;          // smaller bumps stay in the level-scheduled structure
constexpr int kBumpThreads = 1024;

// D22: bump column t = pivot stage s0 + t; U22 on and above the diagonal, L22 (multipliers) below
__global__ __launch_bounds__(kBlock) void bump_extract_kernel(int s0, int kb, const ipxint* __restrict__ Lp, const ipxint* __restrict__ Li,
                                                              const double* __restrict__ Lx, const ipxint* __restrict__ Up, const ipxint* __restrict__ Ui,
                                                              const double* __restrict__ Ux, double* __restrict__ D) {
    // a wavefront per column (a column of U holds up to s0 + kb entries, of which the last <= kb belong to the block)
    const int lane = threadIdx.x & 63;
    for (int t = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); t < kb; t += gridDim.x * (kBlock / 64)) {
        const int j = s0 + t;
        const ipxint u1 = Up[j + 1], u0 = max(Up[j], u1 - kb);     // indices ascend: entries with Ui >= s0 are among the last kb
        for (ipxint p = u0 + lane; p < u1; p += 64)
            if (Ui[p] >= s0) D[(size_t)t * kb + (Ui[p] - s0)] = Ux[p];
        for (ipxint p = Lp[j] + lane; p < Lp[j + 1]; p += 64) D[(size_t)t * kb + (Li[p] - s0)] = Lx[p];
    }
}
// U~: columns < s0 as they are; a bump column keeps its entries above the bump (a prefix: indices ascend) and gets
// the diagonal 1.  L~: columns >= s0 are empty (their entries all lie inside the bump).
__global__ void bump_ucount_kernel(int m, int s0, const ipxint* __restrict__ Up, const ipxint* __restrict__ Ui, int* __restrict__ cnt) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x) {
        int c = (int)(Up[j + 1] - Up[j]);
        if (j >= s0) {
            c = 1;
            for (ipxint p = Up[j]; p < Up[j + 1] && Ui[p] < s0; p++) c++;
        }
        cnt[j] = c;
    }
}
// first entry of every column of U~: unchanged in front of the bump, then the bump columns' counts accumulated
__global__ void bump_ustart_kernel(int m, int s0, const ipxint* __restrict__ Up, const int* __restrict__ cnt, int* __restrict__ start) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < m; j += gridDim.x * blockDim.x)
        if (j <= s0) start[j] = (int)Up[j];
}
__global__ void bump_ustart_tail_kernel(int m, int s0, const ipxint* __restrict__ Up, const int* __restrict__ cnt, int* __restrict__ start) {
    for (int j = s0 + 1; j < m; j++) start[j] = start[j - 1] + cnt[j - 1];     // <= 4096 columns, once per Prepare
}
__global__ void bump_ufill_kernel(int m, int s0, const ipxint* __restrict__ Up, const ipxint* __restrict__ Ui, const double* __restrict__ Ux,
                                  const int* __restrict__ start, const int* __restrict__ cnt, ipxint* __restrict__ Tp,
                                  ipxint* __restrict__ Ti, double* __restrict__ Tx, const ipxint* __restrict__ Lp, ipxint* __restrict__ TLp) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j <= m; j += gridDim.x * blockDim.x) {
        TLp[j] = Lp[j < s0 ? j : s0];
        if (j == m) { Tp[m] = start[m - 1] + cnt[m - 1]; continue; }
        const int q0 = start[j], c = cnt[j];
        Tp[j] = q0;
        for (int e = 0; e < c; e++) { Ti[q0 + e] = Ui[Up[j] + e]; Tx[q0 + e] = Ux[Up[j] + e]; }
        if (j >= s0) { Ti[q0 + c - 1] = j; Tx[q0 + c - 1] = 1.0; }
    }
}
// inverses of the 64 x 64 diagonal blocks of L22+I (unit lower, from below the diagonal of D) or of U22 (upper)
__global__ __launch_bounds__(64) void bump_invert_blocks_kernel(int kb, const double* __restrict__ D, double* __restrict__ inv, int upper) {
    __shared__ double T[64][65];
    const int b0 = blockIdx.x * 64, nb = min(64, kb - b0), c = threadIdx.x;
    for (int l = 0; l < 64; l++) {
        double v = c == l ? 1.0 : 0.0;
        if (c < nb && l < nb) {
            const double d = D[(size_t)(b0 + l) * kb + (b0 + c)];            // element (row c, column l) of the block
            if (upper) v = c <= l ? d : 0.0;
            else v = c > l ? d : (c == l ? 1.0 : 0.0);
        }
        T[c][l] = v;
    }
    __syncthreads();
    double x[64];
    if (!upper) {
#pragma unroll 1
        for (int i = 0; i < 64; i++) {                         // column c of the inverse: T x = e_c, forward
            double s2 = i == c ? 1.0 : 0.0;
            for (int l = c; l < i; l++) s2 -= T[i][l] * x[l];
            x[i] = i < c ? 0.0 : s2 / T[i][i];
        }
    } else {
#pragma unroll 1
        for (int i = 63; i >= 0; i--) {                        // backward
            double s2 = i == c ? 1.0 : 0.0;
            for (int l = i + 1; l <= c; l++) s2 -= T[i][l] * x[l];
            x[i] = i > c ? 0.0 : s2 / T[i][i];
        }
    }
    double* out = inv + (size_t)blockIdx.x * 64 * 64;
    for (int i = 0; i < 64; i++) out[i + 64 * c] = x[i];       // column major
}
// x_bump <- inverse(D22) x_bump (TRANS: inverse(D22')) in place in a sweep's result vector, between the two sweeps
// of a pair.  One workgroup, x in LDS; per 64-block one product with the inverted diagonal block and one update
// of the part of x still to be solved.
template <bool TRANS>
__device__ __forceinline__ void bump_solve_lds(int kb, const double* __restrict__ D, const double* __restrict__ invL,
                                               const double* __restrict__ invU, double* x, double* xb) {
    const int nblk = (kb + 63) / 64, tid = threadIdx.x;
    // two triangular solves; `first` is the lower-triangular-type one (blocks ascending)
    for (int phase = 0; phase < 2; phase++) {
        const bool lower = phase == 0;                       // !TRANS: L22+I then U22;  TRANS: U22' then (L22+I)'
        const double* inv = TRANS ? (lower ? invU : invL) : (lower ? invL : invU);
        for (int q = 0; q < nblk; q++) {
            const int bq = lower ? q : nblk - 1 - q;
            const int b0 = bq * 64, nb = min(64, kb - b0);
            const double* Ib = inv + (size_t)bq * 64 * 64;
            {   // x_b <- inverse(block) x_b (TRANS: its transpose); 16 threads per row, fixed combination order
                const int r = tid >> 4, g = tid & 15;
                double s2 = 0.0;
                if (r < nb)
                    for (int l = g; l < nb; l += 16) s2 += (TRANS ? Ib[l + 64 * r] : Ib[r + 64 * l]) * x[b0 + l];
                s2 = wave_sum<16>(s2);
                if (g == 0 && r < 64) xb[r] = s2;
            }
            __syncthreads();
            if (tid < nb) x[b0 + tid] = xb[tid];
            // the unknowns still to come lose this block's contribution
            const int i0 = lower ? b0 + nb : 0, i1 = lower ? kb : b0;
            for (int i = i0 + tid; i < i1; i += kBumpThreads) {
                double s2 = x[i];
                // element (row i, column b0 + l) of the triangular matrix of this phase
                //   !TRANS: D[(b0+l)*kb + i]   (L22 below / U22 above the diagonal, column major)
                //    TRANS: D[i*kb + b0 + l]   (the transposed factor)
                int l = 0;
                for (; l + 8 <= nb; l += 8) {
                    double v[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) v[u] = TRANS ? D[(size_t)i * kb + b0 + l + u] : D[(size_t)(b0 + l + u) * kb + i];
#pragma unroll
                    for (int u = 0; u < 8; u++) s2 -= v[u] * xb[l + u];
                }
                for (; l < nb; l++) s2 -= (TRANS ? D[(size_t)i * kb + b0 + l] : D[(size_t)(b0 + l) * kb + i]) * xb[l];
                x[i] = s2;
            }
            __syncthreads();
        }
    }
}
template <bool TRANS>
__global__ __launch_bounds__(kBumpThreads) void bump_solve_kernel(int kb, const double* __restrict__ D, const double* __restrict__ invL,
                                                                  const double* __restrict__ invU, const int* __restrict__ pos,
                                                                  double* y, const int* done, double* gx = nullptr) {
    if (done && *done) return;
    extern __shared__ double xs[];       // kb + 64; a block too large for LDS (more than kBumpLdsRows rows) keeps x in the global scratch gx
    double* x = gx ? gx : xs;
    double* xb = gx ? xs : xs + kb;
    const int tid = threadIdx.x;
    for (int t = tid; t < kb; t += kBumpThreads) x[t] = y[pos[t]];
    __syncthreads();
    bump_solve_lds<TRANS>(kb, D, invL, invU, x, xb);
    for (int t = tid; t < kb; t += kBumpThreads) y[pos[t]] = x[t];
}
// The blocked solve applied to the guard's two vectors: w[q kb + t] = (inverse(D22) z_q)[t] as the one-workgroup solve computes it
// (workgroup q).  Its residual is what an explicit inverse of the same block can be held to.
__global__ __launch_bounds__(kBumpThreads) void bump_probe_solve_kernel(int kb, const double* __restrict__ D, const double* __restrict__ invL,
                                                                        const double* __restrict__ invU, double* __restrict__ w, double* gx = nullptr) {
    extern __shared__ double xs[];       // kb + 64 (or 64 with x in the global scratch: one stretch of kb per workgroup)
    const int q = blockIdx.x;
    double* x = gx ? gx + (size_t)q * kb : xs;
    double* xb = gx ? xs : xs + kb;
    for (int t = threadIdx.x; t < kb; t += kBumpThreads) x[t] = probe_z(q, t);
    __syncthreads();
    bump_solve_lds<false>(kb, D, invL, invU, x, xb);
    for (int t = threadIdx.x; t < kb; t += kBumpThreads) w[(size_t)q * kb + t] = x[t];
}
// Explicit inverse of a large block: workgroup j solves D22 x = e_j with the blocked solve above; x = column j of
// inverse(D22) = row j of its transpose.  Both orientations are stored row major, so that either product below reads
// contiguous rows.
__global__ __launch_bounds__(kBumpThreads) void bump_inverse_kernel(int kb, const double* __restrict__ D, const double* __restrict__ invL,
                                                                    const double* __restrict__ invU, double* __restrict__ inv,
                                                                    double* __restrict__ invT) {
    extern __shared__ double xs[];       // kb + 64
    double* x = xs;
    double* xb = xs + kb;
    const int tid = threadIdx.x, j = blockIdx.x;
    for (int t = tid; t < kb; t += kBumpThreads) x[t] = t == j ? 1.0 : 0.0;
    __syncthreads();
    bump_solve_lds<false>(kb, D, invL, invU, x, xb);
    for (int t = tid; t < kb; t += kBumpThreads) {
        invT[(size_t)j * kb + t] = x[t];
        inv[(size_t)t * kb + j] = x[t];
    }
}
__global__ void bump_gather_kernel(int kb, const int* __restrict__ pos, const double* __restrict__ y, double* __restrict__ x, const int* done) {
    if (done && *done) return;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < kb; t += gridDim.x * blockDim.x) x[t] = y[pos[t]];
}
// y[pos[i]] = row i of M times x: one wavefront per row, lanes stride the row, fixed shuffle tree
__global__ __launch_bounds__(kBlock) void bump_gemv_kernel(int kb, const double* __restrict__ M, const double* __restrict__ x,
                                                           const int* __restrict__ pos, double* __restrict__ y, const int* done) {
    if (done && *done) return;
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); i < kb; i += gridDim.x * (kBlock / 64)) {
        const double* row = M + (size_t)i * kb;
        double s2 = 0.0;
        for (int l = lane; l < kb; l += 64) s2 += row[l] * x[l];
        s2 = wave_sum(s2);
        if (lane == 0) y[pos[i]] = s2;
    }
}
__global__ void bump_positions_kernel(int s0, int kb, const int* __restrict__ posof_fwd, const int* __restrict__ posof_bwd,
                                      int* __restrict__ pf, int* __restrict__ pb) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < kb; t += gridDim.x * blockDim.x) {
        pf[t] = posof_fwd[s0 + t];
        pb[t] = posof_bwd[s0 + t];
    }
}
// dense block D22 = (L22 + I) U22 (column major in D: L22 below, U22 on and above the diagonal), inv row major:
// w_q = inv z_q (one wavefront per row), t_q = U22 w_q, r_q = (L22 + I) t_q - z_q (one thread per row: lanes read a column's
// consecutive rows)
__global__ __launch_bounds__(kBlock) void bump_probe_mz_kernel(int kb, const double* __restrict__ inv, double* __restrict__ w) {
    const int lane = threadIdx.x & 63;
    for (int i = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); i < kb; i += gridDim.x * (kBlock / 64)) {
        double s0 = 0.0, s1 = 0.0;
        for (int l = lane; l < kb; l += 64) { const double a = inv[(size_t)i * kb + l]; s0 += a * probe_z(0, l); s1 += a * probe_z(1, l); }
        wave_sum_each(s0, s1);
        if (lane == 0) { w[i] = s0; w[kb + i] = s1; }
    }
}
// t = U22 w (upper part of D with the diagonal) and r = (L22 + I) t - z, D column major: a workgroup takes 64 rows and a
// chunk of 256 columns (lanes along the rows: every load is a 512-byte segment of a column of D, 4 column groups per
// workgroup), the chunks' partial sums are added in chunk order by the second kernel of each stage
constexpr int kProbeChunk = 256;
__global__ __launch_bounds__(kBlock) void bump_probe_partial_kernel(int kb, const double* __restrict__ D, const double* __restrict__ w, int upper,
                                                                    double* __restrict__ part) {
    __shared__ double red[2][4][64];
    const int r = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
    const int l0 = blockIdx.y * kProbeChunk, l1 = min(kb, l0 + kProbeChunk);
    double s0 = 0.0, s1 = 0.0;
    if (r < kb)
        for (int l = l0 + g; l < l1; l += 4) {
            const bool in = upper ? l >= r : l < r;            // U22: columns from the diagonal on; L22: strictly below it
            if (in) { const double a = D[(size_t)l * kb + r]; s0 += a * w[l]; s1 += a * w[kb + l]; }
        }
    red[0][g][threadIdx.x & 63] = s0; red[1][g][threadIdx.x & 63] = s1;
    __syncthreads();
    if (g == 0 && r < kb) {
        const int x = threadIdx.x;
        part[((size_t)blockIdx.y * 2 + 0) * kb + r] = ((red[0][0][x] + red[0][1][x]) + red[0][2][x]) + red[0][3][x];
        part[((size_t)blockIdx.y * 2 + 1) * kb + r] = ((red[1][0][x] + red[1][1][x]) + red[1][2][x]) + red[1][3][x];
    }
}
// stage 1 (res == nullptr): t = sum of the chunks;  stage 2: r = t + sum of the chunks - z, res[q] = max |r_q|
__global__ void bump_probe_finish_kernel(int kb, int nchunks, const double* __restrict__ part, const double* __restrict__ tin,
                                         double* __restrict__ tout, double* res) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < kb; i += gridDim.x * blockDim.x) {
        double s0 = tin ? tin[i] : 0.0, s1 = tin ? tin[kb + i] : 0.0;
        for (int c = 0; c < nchunks; c++) { s0 += part[((size_t)c * 2 + 0) * kb + i]; s1 += part[((size_t)c * 2 + 1) * kb + i]; }
        if (tout) { tout[i] = s0; tout[kb + i] = s1; }
        if (res) {
            probe_max(res + 0, fabs(s0 - probe_z(0, i)));
            probe_max(res + 1, fabs(s1 - probe_z(1, i)));
        }
    }
}
// between the two sweeps of a pair: `y` is the result of the first one
// the blocked solve keeps the kb unknowns of the block in LDS: beyond 64 KB of dynamic LDS the kernels have to be allowed; beyond the
// 160 KB of a compute unit (blocks of more than kBumpLdsRows rows -- what the LU leaves of an 80 000-row IPM basis) the unknowns live
// in a global scratch vector instead (one workgroup: its own stores are visible to it after a barrier)
constexpr int kBumpLdsRows = 160 * 1024 / 8 - 64;
static void allow_bump_lds(size_t bytes) {
    static size_t allowed = 64 * 1024;
    if (bytes <= allowed) return;
    IPXK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(bump_solve_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    IPXK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(bump_solve_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    IPXK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(bump_inverse_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    IPXK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(bump_probe_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    allowed = bytes;
}
void bump_between(Context* c, bool trans, double* y, const int* done) {
    SplitOperator::DenseBump& B = c->split->bump;
    if (B.size == 0) return;
    const int kb = B.size;
    if (B.explicit_inverse) {
        // large block: x_bump <- inverse(D22) x_bump (or its transpose) as one product over the chip
        const int* pos = trans ? B.pos_bwd.get() : B.pos_fwd.get();
        hipLaunchKernelGGL(bump_gather_kernel, dim3(vec_grid(kb)), dim3(kBlock), 0, c->stream, kb, pos, y, B.x.get(), done);
        hipLaunchKernelGGL(bump_gemv_kernel, dim3((kb + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, c->stream, kb,
                           trans ? B.invT.get() : B.inv.get(), B.x.get(), pos, y, done);
        return;
    }
    const bool in_lds = kb <= kBumpLdsRows;
    const size_t lds = (size_t)((in_lds ? kb : 0) + 64) * sizeof(double);
    double* gx = nullptr;
    if (in_lds) allow_bump_lds(lds);
    else { B.gx.ensure((size_t)2 * kb); gx = B.gx.get(); }
    if (trans) hipLaunchKernelGGL(bump_solve_kernel<true>, dim3(1), dim3(kBumpThreads), lds, c->stream, kb, B.D.get(), B.invL.get(),
                                  B.invU.get(), B.pos_bwd.get(), y, done, gx);
    else hipLaunchKernelGGL(bump_solve_kernel<false>, dim3(1), dim3(kBumpThreads), lds, c->stream, kb, B.D.get(), B.invL.get(),
                            B.invU.get(), B.pos_fwd.get(), y, done, gx);
}

// The guard's probe of a dense block from the two vectors w already in the workspace pw (pw[0 .. 2 kb), SplitOperator::DenseBump::probe):
// t = U22 w, then r = (L22 + I) t - z with the residuals into pw[4 kb], pw[4 kb + 1]; the chunks' partial sums behind them
static int probe_chunks(int kb) { return (kb + kProbeChunk - 1) / kProbeChunk; }
static void bump_probe_stages(hipStream_t s, int kb, const double* D, double* pw) {
    const int nchunks = probe_chunks(kb);
    double* part = pw + 4 * (size_t)kb + 2;
    const dim3 pgrid((kb + 63) / 64, nchunks);
    hipLaunchKernelGGL(bump_probe_partial_kernel, pgrid, dim3(kBlock), 0, s, kb, D, pw, 1, part);
    hipLaunchKernelGGL(bump_probe_finish_kernel, dim3(vec_grid(kb)), dim3(kBlock), 0, s, kb, nchunks, part, (const double*)nullptr, pw + 2 * (size_t)kb,
                       (double*)nullptr);
    hipLaunchKernelGGL(bump_probe_partial_kernel, pgrid, dim3(kBlock), 0, s, kb, D, pw + 2 * (size_t)kb, 0, part);
    hipLaunchKernelGGL(bump_probe_finish_kernel, dim3(vec_grid(kb)), dim3(kBlock), 0, s, kb, nchunks, part, pw + 2 * (size_t)kb, (double*)nullptr,
                       pw + 4 * (size_t)kb);
}

// Cuts the trailing block [s0, s0 + kb) = [s0, m) out of the factors: D22 = (L22 + I) U22 goes to S->bump.D (dense, with
// the inverted 64 x 64 diagonal blocks), the returned factors are L without L22 and U with U22 replaced by I (trisolve.hpp).
// Exact for ANY trailing block; it pays when the block is (nearly) dense.
static DeviceFactors cut_dense_block(Context* c, SplitOperator* S, const DeviceFactors& in, int s0, int kb) {
    hipStream_t s = c->stream;
    SplitOperator::DenseBump& B = S->bump;
    const int m = S->m, nblk = (kb + 63) / 64;
    B.D.ensure((size_t)kb * kb);
    IPXK_HIP(hipMemsetAsync(B.D.get(), 0, (size_t)kb * kb * sizeof(double), s));
    hipLaunchKernelGGL(bump_extract_kernel, dim3((kb + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, s, s0, kb, in.Lp, in.Li, in.Lx, in.Up, in.Ui,
                       in.Ux, B.D.get());
    DevBuf<int> &cnt = B.cut_cnt, &start = B.cut_start;
    cnt.ensure((size_t)m); start.ensure((size_t)m);
    hipLaunchKernelGGL(bump_ucount_kernel, dim3(vec_grid(m)), dim3(kBlock), 0, s, m, s0, in.Up, in.Ui, cnt.get());
    hipLaunchKernelGGL(bump_ustart_kernel, dim3(vec_grid(m)), dim3(kBlock), 0, s, m, s0, in.Up, cnt.get(), start.get());
    hipLaunchKernelGGL(bump_ustart_tail_kernel, dim3(1), dim3(1), 0, s, m, s0, in.Up, cnt.get(), start.get());
    B.cut_Lp.ensure((size_t)m + 1); B.cut_Up.ensure((size_t)m + 1);
    B.cut_Ui.ensure((size_t)std::max<int64_t>(in.nzU, 1)); B.cut_Ux.ensure((size_t)std::max<int64_t>(in.nzU, 1));
    hipLaunchKernelGGL(bump_ufill_kernel, dim3(vec_grid(m + 1)), dim3(kBlock), 0, s, m, s0, in.Up, in.Ui, in.Ux, start.get(), cnt.get(),
                       B.cut_Up.get(), B.cut_Ui.get(), B.cut_Ux.get(), in.Lp, B.cut_Lp.get());
    ipxint ends[2] = {0, 0};
    IPXK_HIP(hipMemcpyAsync(&ends[0], B.cut_Lp.get() + m, sizeof(ipxint), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipMemcpyAsync(&ends[1], B.cut_Up.get() + m, sizeof(ipxint), hipMemcpyDeviceToHost, s));
    B.invL.ensure((size_t)nblk * 64 * 64); B.invU.ensure((size_t)nblk * 64 * 64);
    hipLaunchKernelGGL(bump_invert_blocks_kernel, dim3(nblk), dim3(64), 0, s, kb, B.D.get(), B.invL.get(), 0);
    hipLaunchKernelGGL(bump_invert_blocks_kernel, dim3(nblk), dim3(64), 0, s, kb, B.D.get(), B.invU.get(), 1);
    // large blocks: the inverse itself (IPXK_BUMP_INVERSE_MIN rows and more, default 512; 0 = never), so that the solve
    // between two sweeps is one matrix-vector product over the chip instead of a blocked solve by one workgroup
    // (measured with a 1316-row block: 4.3 ms -> 0.06 ms per CR iteration of the drop-in solver; the reference's CPU solver: 0.54 ms)
    // ... up to IPXK_BUMP_INVERSE_MAX rows (default: every block the LU can produce).  The inverse costs kb workgroups a whole
    // blocked solve each -- about 1 s at 8000 rows -- but the one-workgroup solve it replaces takes 18 ms per application there:
    // measured on a 12 000 x 30 000 LP through the drop-in solver (24 Prepares, 1100 CR iterations): 23 + 0.7 s against 43 s
    static const int inverse_min = [] { const char* e = getenv("IPXK_BUMP_INVERSE_MIN"); return e ? atoi(e) : 512; }();
    static const int inverse_max = [] { const char* e = getenv("IPXK_BUMP_INVERSE_MAX"); return e ? atoi(e) : 32768; }();
    B.explicit_inverse = inverse_min > 0 && kb >= inverse_min && kb <= inverse_max;
    if (B.explicit_inverse) {
        B.inv.ensure((size_t)kb * kb); B.invT.ensure((size_t)kb * kb); B.x.ensure((size_t)kb);
        // blocks of IPXK_DENSE_INVERSE_MIN rows and more (default: all of them) on the matrix cores (dense_inverse.hip: triangular
        // inverses by recursive doubling + one product, v_mfma_f64_16x16x4_f64); below, or with IPXK_DENSE_INVERSE_MIN=0, the
        // older kernel: one blocked solve per column of the identity
        const char* di_env = getenv("IPXK_DENSE_INVERSE_MIN");          // (read per Prepare: the tests switch it)
        const int di_min = di_env ? atoi(di_env) : 1;
        const bool by_blas = di_min > 0 && kb >= di_min;
        const bool in_lds = kb <= kBumpLdsRows;
        if (in_lds) allow_bump_lds((size_t)(kb + 64) * sizeof(double));
        IPXK_REQUIRE(by_blas || in_lds, "a dense block of this size is inverted on the matrix cores only (IPXK_DENSE_INVERSE_MIN)");
        if (!by_blas) hipLaunchKernelGGL(bump_inverse_kernel, dim3(kb), dim3(kBumpThreads), (size_t)(kb + 64) * sizeof(double), s, kb, B.D.get(),
                           B.invL.get(), B.invU.get(), B.inv.get(), B.invT.get());
        // the guard (whoever computed the inverse): D22 (inverse z) against z; a block that fails keeps the blocked solve.  The
        // inverse from the matrix cores gets up to two refinement steps first (X += X (I - D22 X)) when the probe says they can
        // converge: the IPM's late bases are ill conditioned, and the product of two triangular inverses then misses the
        // tolerance by two or three digits (dense_inverse.hip) -- without the steps every block of a 12 000 x 30 000 LP's main
        // phase fell back to the one-workgroup solve, 12 ms per CR iteration instead of 0.5.
        B.probe.ensure((size_t)4 * kb + 2 + (size_t)2 * probe_chunks(kb) * kb);
        double* pw = B.probe.get();
        static const int max_refine = [] { const char* e = getenv("IPXK_DENSE_INVERSE_REFINE"); return e ? std::max(0, atoi(e)) : 2; }();
        double resid = 0.0, first_resid = 0.0;
        int refine = 0;
        for (;;) {
            if (by_blas) dense_lu_inverse(c, kb, B.D.get(), B.invL.get(), B.invU.get(), B.invT.get(), B.inv.get(), refine);
            resid = probe_residual(s, pw + 4 * (size_t)kb, [&] {
                hipLaunchKernelGGL(bump_probe_mz_kernel, dim3((kb + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, s, kb, B.inv.get(), pw);
                bump_probe_stages(s, kb, B.D.get(), pw);
            });
            if (refine == 0) first_resid = resid;
            c->split_stats.inverse_probes++;
            if (resid <= inverse_tol(true) || !by_blas || refine >= max_refine || !(resid < 0.25)) break;
            refine++;
            c->split_stats.inverse_refined++;
        }
        // an inverse that misses the tolerance narrowly is held against what it replaces: the blocked solve's own residual on the
        // same two vectors (an ill-conditioned block leaves neither at 1e-8); within four times that, it stays.  (That probe is
        // of the solve, not of an inverse: it is not counted.)
        double resid_solve = -1.0;
        if (!(resid <= inverse_tol(true)) && resid < 1e-5 && inverse_tol(true) > 0.0)         // (tolerance 0: "reject everything", tests)
            resid_solve = probe_residual(s, pw + 4 * (size_t)kb, [&] {
                double* gx = nullptr;
                if (!in_lds) { B.gx.ensure((size_t)2 * kb); gx = B.gx.get(); }
                hipLaunchKernelGGL(bump_probe_solve_kernel, dim3(2), dim3(kBumpThreads), (size_t)((in_lds ? kb : 0) + 64) * sizeof(double), s, kb, B.D.get(),
                                   B.invL.get(), B.invU.get(), pw, gx);
                bump_probe_stages(s, kb, B.D.get(), pw);
            });
        const bool accepted = resid <= inverse_tol(true) || (resid_solve >= 0.0 && resid <= 4.0 * resid_solve);
        record_verdict(c, resid, accepted);
        if (!accepted) B.explicit_inverse = false;
        if (resid_solve >= 0.0 && sweep_verbose())
            fprintf(stderr, "ipxk:   (the blocked solve's own probe on this block: %.2e)\n", resid_solve);
        if (sweep_verbose())
            fprintf(stderr, "ipxk: dense block of %d rows inverted (%s); probe |D (inverse z) - z| = %.2e%s%s\n", kb,
                    by_blas ? "recursive doubling on the matrix cores" : "one blocked solve per column", resid,
                    refine > 0 ? (refine == 1 ? " after one refinement step" : " after two refinement steps") : "",
                    B.explicit_inverse ? "" : " -> REJECTED, the blocked solve stays");
        if (refine > 0 && sweep_verbose()) fprintf(stderr, "ipxk:   (probe before the refinement %.2e)\n", first_resid);
    }
    IPXK_HIP(hipStreamSynchronize(s));               // cnt / start go out of scope; ends
    B.start = s0;
    B.size = kb;
    return DeviceFactors{B.cut_Lp.get(), in.Li, B.cut_Up.get(), B.cut_Ui.get(), in.Lx, B.cut_Ux.get(), ends[0], ends[1]};
}

// A dense trailing block in factors that come from the host (the dense bump of an LU kernel -- lu.hip's or any other
// -- is pivoted last).  Where
// the device computed the factors it knows the block (LuView); factors handed over by ipx::Basis have gone through
// the host, and without this a 2000-row bump is a chain of 2000 dependency levels (12 ms per operator application
// against 1 ms with the block cut out: the drop-in class on the IPM's random LPs).
int trailing_dense_block(int m, const ipxint* Lp) {
    // the largest trailing block (up to 32768 columns: the largest dense block the LU produces) whose part of L is at least 30 % full: a dense LU of a sparse bump
    // starts with sparse columns and fills up, so single columns say little; the block as a whole does
    int s0 = m;
    const int lo = std::max(0, m - 32768);
    for (int j = m - 2; j >= lo; j--) {
        const double kb = (double)(m - j), have = (double)(Lp[m] - Lp[j]);
        if (have >= 0.3 * (kb * (kb - 1.0) / 2.0)) s0 = j;
    }
    return s0;
}

void analyse_sweeps_cutting_bump(Context* c, SplitOperator* S, const DeviceFactors& F, bool cuttable, int s0, int kb,
                                 const ipxint* hLp, const ipxint* hLi, const ipxint* hUp, const ipxint* hUi) {
    SplitOperator::DenseBump& B = S->bump;
    const char* dense_env = getenv("IPXK_BUMP_DENSE");
    const int bump_min = getenv("IPXK_BUMP_MIN") ? atoi(getenv("IPXK_BUMP_MIN")) : kBumpMin;      // (tests)
    if (cuttable && kb >= bump_min && !(dense_env && dense_env[0] == '0'))
        analyse_sweeps_resident(c, S, cut_dense_block(c, S, F, s0, kb), nullptr, nullptr, nullptr, nullptr);
    else
        analyse_sweeps_resident(c, S, F, hLp, hLi, hUp, hUi);
    if (B.size > 0) {
        B.pos_fwd.ensure((size_t)B.size); B.pos_bwd.ensure((size_t)B.size);
        hipLaunchKernelGGL(bump_positions_kernel, dim3(vec_grid(B.size)), dim3(kBlock), 0, c->stream, B.start, B.size, S->Lf.posof.get(),
                           S->Ut.posof.get(), B.pos_fwd.get(), B.pos_bwd.get());
    }
}

}  // namespace ipxk
