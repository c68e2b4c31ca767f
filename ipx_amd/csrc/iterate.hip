// The IPM iterate on the device                       reference src/iterate.cc, src/ipm.cc
//   Iterate::Update                 iterate.cc:94-139   (steps truncated at kBarrierMin)
//   Iterate::ComputeResiduals       iterate.cc:536-588  rb = b - AI x, rc = c - AI'y - zl + zu, rl, ru
//   Iterate::ComputeComplementarity iterate.cc:642-670
//   StepToBoundary                  ipm.cc:320-339
// with the iterate resident, the vectors of an IPM iteration never
// cross PCIe.  The two sparse products reuse the gather SpMV with epilogues that reproduce the
// reference's evaluation order ((c - zl) + zu) - A_j'y and (b - sum_j a_ij x_j) - x_{n+i}.
#include "context.hpp"
#include "spmv_kernels.hpp"

namespace ipxk {

namespace {

constexpr double kBarrierMin = 1e-30;   // Iterate::kBarrierMin, src/iterate.h:204

__device__ __forceinline__ bool has_lb(unsigned char st) { return st == IPXK_STATE_BARRIER_LB || st == IPXK_STATE_BARRIER_BOXED; }
__device__ __forceinline__ bool has_ub(unsigned char st) { return st == IPXK_STATE_BARRIER_UB || st == IPXK_STATE_BARRIER_BOXED; }

__global__ void iterate_update_kernel(int N, int m, const unsigned char* __restrict__ state, double* __restrict__ x,
                                      double* __restrict__ xl, double* __restrict__ xu, double* __restrict__ y,
                                      double* __restrict__ zl, double* __restrict__ zu, double sp,
                                      const double* dx, const double* dxl, const double* dxu, double sd,
                                      const double* dy, const double* dzl, const double* dzu) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += gridDim.x * blockDim.x) {
        const unsigned char st = state[j];
        if (dx && st != IPXK_STATE_FIXED) x[j] += sp * dx[j];
        if (has_lb(st)) {
            if (dxl) xl[j] = fmax(xl[j] + sp * dxl[j], kBarrierMin);
            if (dzl) zl[j] = fmax(zl[j] + sd * dzl[j], kBarrierMin);
        }
        if (has_ub(st)) {
            if (dxu) xu[j] = fmax(xu[j] + sp * dxu[j], kBarrierMin);
            if (dzu) zu[j] = fmax(zu[j] + sd * dzu[j], kBarrierMin);
        }
        if (dy && j < m) y[j] += sd * dy[j];
    }
}

// rb[i] = (b[i] - sum_j a_ij x_j) - x[n+i]
struct EpiIterRb : ProdMul {
    const double* b; const double* xI; double* out;
    static constexpr bool kNeg = true;
    __device__ __forceinline__ double init(int r) const { return b[r]; }
    __device__ __forceinline__ void finish(int r, double acc, double&) const { out[r] = acc - xI[r]; }
};

// rc[j] = ((c[j] - zl[j]) + zu[j]) - A_j'y, 0 on fixed variables unless the iterate is postprocessed (iterate.cc:552-556)
struct EpiIterRc : ProdMul {
    const double* c; const double* zl; const double* zu; const unsigned char* state; double* out; bool postprocessed;
    static constexpr bool kNeg = false;
    __device__ __forceinline__ double init(int) const { return 0.0; }
    __device__ __forceinline__ void finish(int j, double acc, double&) const {
        out[j] = state[j] == IPXK_STATE_FIXED && !postprocessed ? 0.0 : ((c[j] - zl[j]) + zu[j]) - acc;
    }
};

// slack part of rc, and rl, ru for all variables
__global__ void iterate_bound_residuals_kernel(int n, int m, const unsigned char* __restrict__ state,
                                               const double* __restrict__ c, const double* __restrict__ lb,
                                               const double* __restrict__ ub, const double* __restrict__ x,
                                               const double* __restrict__ xl, const double* __restrict__ xu,
                                               const double* __restrict__ y, const double* __restrict__ zl,
                                               const double* __restrict__ zu, bool postprocessed,
                                               double* __restrict__ rc, double* __restrict__ rl,
                                               double* __restrict__ ru) {
    const int N = n + m;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += gridDim.x * blockDim.x) {
        const unsigned char st = state[j];
        if (j >= n) rc[j] = st == IPXK_STATE_FIXED && !postprocessed ? 0.0 : ((c[j] - zl[j]) + zu[j]) - y[j - n];
        rl[j] = has_lb(st) ? lb[j] - x[j] + xl[j] : 0.0;
        ru[j] = has_ub(st) ? ub[j] - x[j] - xu[j] : 0.0;
    }
}

// out[0*G + b] = max |rb|, |rl|, |ru| over the block's share; out[1*G + b] = max |rc|
__global__ __launch_bounds__(kBlock) void iterate_norms_kernel(int N, int m, const double* __restrict__ rb,
                                                               const double* __restrict__ rc,
                                                               const double* __restrict__ rl,
                                                               const double* __restrict__ ru, double* out) {
    __shared__ double red[kBlock / 64 + 1];
    double p = 0.0, d = 0.0;
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < N; j += gridDim.x * kBlock) {
        if (j < m) p = fmax(p, fabs(rb[j]));
        p = fmax(p, fmax(fabs(rl[j]), fabs(ru[j])));
        d = fmax(d, fabs(rc[j]));
    }
    p = block_reduce<MaxOp>(p, red);
    d = block_reduce<MaxOp>(d, red);
    if (threadIdx.x == 0) { out[blockIdx.x] = p; out[gridDim.x + blockIdx.x] = d; }
}

// per block: sum, min, max of the complementarity products and their count
__global__ __launch_bounds__(kBlock) void iterate_complementarity_kernel(int N, const unsigned char* __restrict__ state,
                                                                         const double* __restrict__ xl,
                                                                         const double* __restrict__ xu,
                                                                         const double* __restrict__ zl,
                                                                         const double* __restrict__ zu, double* out) {
    __shared__ double red[kBlock / 64 + 1];
    double sum = 0.0, mn = MinOp::identity(), mx = 0.0, cnt = 0.0;
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < N; j += gridDim.x * kBlock) {
        const unsigned char st = state[j];
        if (has_lb(st)) { const double p = xl[j] * zl[j]; sum += p; mn = fmin(mn, p); mx = fmax(mx, p); cnt += 1.0; }
        if (has_ub(st)) { const double p = xu[j] * zu[j]; sum += p; mn = fmin(mn, p); mx = fmax(mx, p); cnt += 1.0; }
    }
    sum = block_reduce<SumOp>(sum, red);
    mn = block_reduce<MinOp>(mn, red);
    mx = block_reduce<MaxOp>(mx, red);
    cnt = block_reduce<SumOp>(cnt, red);
    if (threadIdx.x == 0) {
        const int G = gridDim.x, b = blockIdx.x;
        out[b] = sum; out[G + b] = mn; out[2 * G + b] = mx; out[3 * G + b] = cnt;
    }
}

// per block: smallest candidate step and the smallest index attaining it
__global__ __launch_bounds__(kBlock) void step_to_boundary_kernel(int len, const double* __restrict__ x,
                                                                  const double* __restrict__ dx, double alpha0,
                                                                  double* out_alpha, double* out_index) {
    __shared__ double red[kBlock / 64 + 1];
    const double damp = 1.0 - 2.220446049250313e-16;
    double best = MinOp::identity();
    double bidx = 9.0e15;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < len; i += gridDim.x * kBlock) {
        if (x[i] + alpha0 * dx[i] < 0.0) {
            const double cand = -(x[i] * damp) / dx[i];
            if (cand < best) { best = cand; bidx = (double)i; }   // i ascends per thread: first index kept
        }
    }
    const double blockbest = block_reduce<MinOp>(best, red);
    const double myidx = best == blockbest ? bidx : 9.0e15;
    const double blockidx = block_reduce<MinOp>(myidx, red);
    if (threadIdx.x == 0) { out_alpha[blockIdx.x] = blockbest; out_index[blockIdx.x] = blockidx; }
}

// per-block partial sums for Iterate::ComputeObjectives (iterate.cc:590-640, the branch of an iterate that has
// not been postprocessed; fixed / free / barrier variables): [0] sum c_j x_j over non-fixed j, [1] over fixed j
// (offset_), [2] b'y + sum lb_j zl_j - sum ub_j zu_j - sum over fixed SLACK variables of x_j y_i
__global__ __launch_bounds__(kBlock) void iterate_objectives_kernel(int n, int m, const unsigned char* __restrict__ state,
                                                                    const double* __restrict__ b, const double* __restrict__ c,
                                                                    const double* __restrict__ lb, const double* __restrict__ ub,
                                                                    const double* __restrict__ x, const double* __restrict__ y,
                                                                    const double* __restrict__ zl, const double* __restrict__ zu,
                                                                    double* out) {
    __shared__ double red[kBlock / 64 + 1];
    const int N = n + m;
    double pobj = 0.0, offset = 0.0, dobj = 0.0;
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < N; j += gridDim.x * kBlock) {
        const unsigned char st = state[j];
        if (st != IPXK_STATE_FIXED) pobj += c[j] * x[j]; else offset += c[j] * x[j];
        if (st == IPXK_STATE_IMPLIED_LB || st == IPXK_STATE_IMPLIED_UB) {       // :621-626: the cost of j is decreased by zl - zu
            const double shift = (zl[j] - zu[j]) * x[j];
            pobj -= shift;
            offset += shift;
        }
        if (has_lb(st)) dobj += lb[j] * zl[j];
        if (has_ub(st)) dobj -= ub[j] * zu[j];
        if (j < m) dobj += b[j] * y[j];
        if (st == IPXK_STATE_FIXED && j >= n) dobj -= x[j] * y[j - n];
    }
    pobj = block_reduce<SumOp>(pobj, red);
    offset = block_reduce<SumOp>(offset, red);
    dobj = block_reduce<SumOp>(dobj, red);
    if (threadIdx.x == 0) { out[blockIdx.x] = pobj; out[gridDim.x + blockIdx.x] = offset; out[2 * gridDim.x + blockIdx.x] = dobj; }
}
// the branch of a postprocessed iterate (iterate.cc:599-609): [0] sum c_j x_j, [1] b'y + sum lb_j zl_j - sum ub_j zu_j over the
// finite bounds
__global__ __launch_bounds__(kBlock) void iterate_objectives_post_kernel(int n, int m, const double* __restrict__ b,
                                                                         const double* __restrict__ c, const double* __restrict__ lb,
                                                                         const double* __restrict__ ub, const double* __restrict__ x,
                                                                         const double* __restrict__ y, const double* __restrict__ zl,
                                                                         const double* __restrict__ zu, double* out) {
    __shared__ double red[kBlock / 64 + 1];
    const int N = n + m;
    double pobj = 0.0, dobj = 0.0;
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < N; j += gridDim.x * kBlock) {
        pobj += c[j] * x[j];
        if (j < m) dobj += b[j] * y[j];
        if (isfinite(lb[j])) dobj += lb[j] * zl[j];
        if (isfinite(ub[j])) dobj -= ub[j] * zu[j];
    }
    pobj = block_reduce<SumOp>(pobj, red);
    dobj = block_reduce<SumOp>(dobj, red);
    if (threadIdx.x == 0) { out[blockIdx.x] = pobj; out[gridDim.x + blockIdx.x] = dobj; }
}
// fixed structural variables: dot partial += x_j * (A_j'y)
struct EpiObjFixed : ProdMul {
    const unsigned char* state; const double* x;
    static constexpr bool kNeg = false;
    __device__ __forceinline__ double init(int) const { return 0.0; }
    __device__ __forceinline__ void finish(int j, double acc, double& dot) const {
        if (state[j] == IPXK_STATE_FIXED) dot += x[j] * acc;
    }
};
// Model::ComputeNorms (model.cc:58-67): per-block maxima of |b|, finite |lb|, |ub| and of |c|
__global__ __launch_bounds__(kBlock) void model_norms_kernel(int n, int m, const double* __restrict__ b,
                                                             const double* __restrict__ c, const double* __restrict__ lb,
                                                             const double* __restrict__ ub, double* out) {
    __shared__ double red[kBlock / 64 + 1];
    double nb = 0.0, nc = 0.0;
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < n + m; j += gridDim.x * kBlock) {
        if (j < m) nb = fmax(nb, fabs(b[j]));
        if (isfinite(lb[j])) nb = fmax(nb, fabs(lb[j]));
        if (isfinite(ub[j])) nb = fmax(nb, fabs(ub[j]));
        nc = fmax(nc, fabs(c[j]));
    }
    nb = block_reduce<MaxOp>(nb, red);
    nc = block_reduce<MaxOp>(nc, red);
    if (threadIdx.x == 0) { out[blockIdx.x] = nb; out[gridDim.x + blockIdx.x] = nc; }
}

// column partition: this rank's share of b - A x (b on rank 0, nullptr elsewhere), summed over the ranks afterwards
struct EpiIterRbPart : ProdMul {
    const double* b; double* out;
    static constexpr bool kNeg = true;
    __device__ __forceinline__ double init(int r) const { return b ? b[r] : 0.0; }
    __device__ __forceinline__ void finish(int r, double acc, double&) const { out[r] = acc; }
};
// ... then rb[i] = sum[i] - x[n+i]
__global__ void subtract_slack_kernel(int m, const double* __restrict__ xI, double* __restrict__ rb) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) rb[i] = rb[i] - xI[i];
}

// the four step-to-boundary problems of a step (xl, xu, zl, zu), problem k's block partials at part + 2 g k (alpha,
// then index).  Wave k reduces them to the smallest alpha below alpha0 and the smallest index attaining it -- the fold
// of step_to_boundary_dev; a block's index may lie in a later grid pass than a higher block's, so the fold compares
// indices, not block numbers -- and writes row[6k..6k+5] = alpha, GLOBAL blocking index (structural c0 + j, slack
// n_global + i; -1: none), and the x, dx, z, dz at the candidate that StepSizes reads (the l pair for problems 0 and 2,
// the u pair for 1 and 3).
__global__ __launch_bounds__(256) void boundary_row_kernel(int g, const double* __restrict__ part, double alpha0, int n,
                                                           double c0, double n_global, BoundaryVectors V,
                                                           double* __restrict__ row) {
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double* a = part + (size_t)2 * g * k;
    double alpha = alpha0;
    int idx = INT_MAX;                      // none; a block that holds a step below alpha0 holds its index too
    for (int i = lane; i < g; i += 64)
        if (a[i] < alpha0) take_smaller(alpha, idx, a[i], (int)a[g + i]);
    wave_argmin(alpha, idx);
    if (lane != 0) return;
    double* r = row + 6 * k;
    r[0] = alpha;
    if (idx != INT_MAX) {
        const int j = idx;
        const bool lower = (k & 1) == 0;
        r[1] = j < n ? c0 + j : n_global + (j - n);
        r[2] = lower ? V.xl[j] : V.xu[j];
        r[3] = lower ? V.dxl[j] : V.dxu[j];
        r[4] = lower ? V.zl[j] : V.zu[j];
        r[5] = lower ? V.dzl[j] : V.dzu[j];
    } else {
        r[1] = -1.0; r[2] = r[3] = r[4] = r[5] = 0.0;
    }
}

// ---- column-partitioned contexts (comm_cols) ----
// Every scalar of the iterate is formed the same way on every rank: each rank reduces its own block partials in block
// order (as the unpartitioned context does), one all-gather carries the small row of per-rank values, and every rank
// combines the table in rank order (sums) or in any order (max, min: exact).  The replicated slack entries and b'y enter
// on rank 0 only, so one rank reproduces the unpartitioned context bit for bit.  Vectors of length n+m are
// [own structural slice; all m slack entries]; rb is the one m-vector that needs an all-reduce.
const char* const kIterateRowRefusal =
    "the device IPM does not run on a row-partitioned system: partition the structural columns (ipxk_comm_init_columns)";

// rb, rc, rl, ru of the resident iterate
void residual_vectors(Context* c, const double* b, const double* cc, const double* lb, const double* ub, double* rb,
                      double* rc, double* rl, double* ru) {
    const int n = (int)c->n, m = (int)c->m, N = n + m;
    hipStream_t s = c->stream;
    residual_rb(c, b, c->it_x.get(), rb);
    EpiIterRc ec{{}, cc, c->it_zl.get(), c->it_zu.get(), c->it_state.get(), rc, c->postprocessed};
    launch_spmv(c->Acols, c->it_y.get(), ec, nullptr, nullptr, s);
    hipLaunchKernelGGL(iterate_bound_residuals_kernel, dim3(vec_grid(N)), dim3(kBlock), 0, s, n, m, c->it_state.get(),
                       cc, lb, ub, c->it_x.get(), c->it_xl.get(), c->it_xu.get(), c->it_y.get(), c->it_zl.get(),
                       c->it_zu.get(), c->postprocessed, rc, rl, ru);
}

// this rank's presidual, dresidual (max over its entries; rb is replicated)
void residual_norms_local(Context* c, const double* rb, const double* rc, const double* rl, const double* ru, double out2[2]) {
    const int m = (int)c->m, N = (int)(c->n + c->m);
    const int g = vec_grid(N);
    c->it_partials.resize((size_t)4 * 1024);
    hipLaunchKernelGGL(iterate_norms_kernel, dim3(g), dim3(kBlock), 0, c->stream, N, m, rb, rc, rl, ru, c->it_partials.get());
    std::vector<double> h((size_t)2 * g);
    c->it_partials.download(h.data(), h.size(), c->stream);
    IPXK_HIP(hipGetLastError());
    double p = 0.0, d = 0.0;
    for (int i = 0; i < g; i++) { p = std::max(p, h[i]); d = std::max(d, h[(size_t)g + i]); }
    out2[0] = p; out2[1] = d;
}

// this rank's sum, min, max and count of the barrier products (slack terms if with_replicated)
void complementarity_local(Context* c, double out4[4]) {
    const int N = (int)(with_replicated(c) ? c->n + c->m : c->n);
    const int g = vec_grid(N);
    c->it_partials.resize((size_t)4 * 1024);
    hipLaunchKernelGGL(iterate_complementarity_kernel, dim3(g), dim3(kBlock), 0, c->stream, N, c->it_state.get(),
                       c->it_xl.get(), c->it_xu.get(), c->it_zl.get(), c->it_zu.get(), c->it_partials.get());
    std::vector<double> h((size_t)4 * g);
    c->it_partials.download(h.data(), h.size(), c->stream);
    IPXK_HIP(hipGetLastError());
    double sum = 0.0, mn = INFINITY, mx = 0.0, cnt = 0.0;
    for (int i = 0; i < g; i++) {
        sum += h[i]; mn = std::min(mn, h[(size_t)g + i]); mx = std::max(mx, h[(size_t)2 * g + i]); cnt += h[(size_t)3 * g + i];
    }
    out4[0] = sum; out4[1] = mn; out4[2] = mx; out4[3] = cnt;
}

// this rank's sums pobj, offset, dobj (b'y and the slack terms if with_replicated) and the fixed structural x_j A_j'y
void objectives_local(Context* c, const double* b, const double* cc, const double* lb, const double* ub, double out4[4]) {
    // the kernel with m = 0 visits the structural slice only and leaves out b'y
    const int n = (int)c->n, m = with_replicated(c) ? (int)c->m : 0, N = n + m;
    hipStream_t s = c->stream;
    const int g = vec_grid(N);
    c->it_partials.resize((size_t)4 * 1024);
    if (c->postprocessed) {
        hipLaunchKernelGGL(iterate_objectives_post_kernel, dim3(g), dim3(kBlock), 0, s, n, m, b, cc, lb, ub, c->it_x.get(),
                           c->it_y.get(), c->it_zl.get(), c->it_zu.get(), c->it_partials.get());
        std::vector<double> h((size_t)2 * g);
        c->it_partials.download(h.data(), h.size(), s);
        IPXK_HIP(hipGetLastError());
        double pobj = 0.0, dobj = 0.0;
        for (int i = 0; i < g; i++) { pobj += h[i]; dobj += h[(size_t)g + i]; }
        out4[0] = pobj; out4[1] = 0.0; out4[2] = dobj; out4[3] = 0.0;
        return;
    }
    c->ensure_partials();
    hipLaunchKernelGGL(iterate_objectives_kernel, dim3(g), dim3(kBlock), 0, s, n, m, c->it_state.get(), b, cc, lb, ub,
                       c->it_x.get(), c->it_y.get(), c->it_zl.get(), c->it_zu.get(), c->it_partials.get());
    EpiObjFixed ef{{}, c->it_state.get(), c->it_x.get()};
    const int np = launch_spmv(c->Acols, c->it_y.get(), ef, c->part(kPartScratch), nullptr, s);
    std::vector<double> h((size_t)3 * g), hf((size_t)std::max(np, 1));
    c->it_partials.download(h.data(), h.size(), s);
    if (np > 0) staged_d2h(hf.data(), c->part(kPartScratch), sizeof(double) * (size_t)np, s);
    IPXK_HIP(hipGetLastError());
    double pobj = 0.0, offset = 0.0, dobj = 0.0, fixed = 0.0;
    for (int i = 0; i < g; i++) { pobj += h[i]; offset += h[(size_t)g + i]; dobj += h[(size_t)2 * g + i]; }
    for (int i = 0; i < np; i++) fixed += hf[i];
    out4[0] = pobj; out4[1] = offset; out4[2] = dobj; out4[3] = fixed;
}

}  // namespace

void residual_rb(Context* c, const double* b, const double* x, double* rb) {
    const int n = (int)c->n, m = (int)c->m;
    hipStream_t s = c->stream;
    if (comm_cols(c)) {
        // (b - sum_g A_g x_g) - x_slack: the partial sums go straight into the exchange buffer where there is one
        double* stage = comm_stage(c, (size_t)m);
        EpiIterRbPart eb{{}, c->rank == 0 ? b : nullptr, stage ? stage : rb};
        launch_spmv(c->Arows, x, eb, nullptr, nullptr, s);
        if (stage) comm_allreduce_sum_staged(c, rb, (size_t)m);
        else comm_allreduce_sum(c, rb, (size_t)m);
        hipLaunchKernelGGL(subtract_slack_kernel, dim3(vec_grid(m)), dim3(kBlock), 0, s, m, x + n, rb);
    } else {
        EpiIterRb eb{{}, b, x + n, rb};
        launch_spmv(c->Arows, x, eb, nullptr, nullptr, s);
    }
}

bool with_replicated(const Context* c) { return !comm_cols(c) || c->rank == 0; }

void combine_over_ranks(Context* c, double* row, const CombineOp* ops, int k) {
    if (!comm_cols(c)) return;
    c->it_row.upload(row, (size_t)k, c->stream);
    const std::vector<double> T = comm_gather_table(c, c->it_row.get(), (size_t)k);
    for (int f = 0; f < k; f++) {
        double v = T[(size_t)f];
        for (int r = 1; r < c->nranks; r++) {
            const double w = T[(size_t)r * k + f];
            v = ops[f] == kCombineSum ? v + w : ops[f] == kCombineMax ? std::max(v, w) : std::min(v, w);
        }
        row[f] = v;
    }
}

void iterate_scalars_dev(Context* c, unsigned what, const double* b, const double* cc, const double* lb, const double* ub,
                         double* rb, double* rc, double* rl, double* ru, IterScalars* out) {
    IPXK_REQUIRE(c->it_set, "no iterate on the device (ipxk_iterate_set)");
    double row[10];
    CombineOp ops[10];
    int k = 0;
    if (what & kIterResiduals) {
        IPXK_REQUIRE(!comm_rows(c), kIterateRowRefusal);
        residual_vectors(c, b, cc, lb, ub, rb, rc, rl, ru);
        residual_norms_local(c, rb, rc, rl, ru, row + k);
        ops[k++] = kCombineMax; ops[k++] = kCombineMax;
    }
    if (what & kIterComplementarity) {
        complementarity_local(c, row + k);
        ops[k++] = kCombineSum; ops[k++] = kCombineMin; ops[k++] = kCombineMax; ops[k++] = kCombineSum;
    }
    if (what & kIterObjectives) {
        IPXK_REQUIRE(!comm_rows(c), kIterateRowRefusal);
        objectives_local(c, b, cc, lb, ub, row + k);
        for (int f = 0; f < 4; f++) ops[k++] = kCombineSum;
    }
    combine_over_ranks(c, row, ops, k);
    k = 0;
    if (what & kIterResiduals) { out->presidual = row[k++]; out->dresidual = row[k++]; }
    if (what & kIterComplementarity) {
        double sum = row[k], mn = row[k + 1], mx = row[k + 2], cnt = row[k + 3];
        k += 4;
        // :666-669
        double mu = 0.0;
        if (cnt > 0) mu = sum / cnt; else mn = 0.0;
        out->comp[0] = sum; out->comp[1] = mu; out->comp[2] = mn; out->comp[3] = mx;
        out->num_terms = cnt;
    }
    if (what & kIterObjectives) {
        const double pobj = row[k], offset = row[k + 1], dobj = row[k + 2], fixed = row[k + 3];
        out->obj[0] = pobj; out->obj[1] = dobj - fixed; out->obj[2] = offset;
    }
}

// out3 = pobjective, dobjective, offset
void iterate_objectives_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub,
                            double out3[3]) {
    IterScalars S;
    iterate_scalars_dev(c, kIterObjectives, b, cc, lb, ub, nullptr, nullptr, nullptr, nullptr, &S);
    std::copy(S.obj, S.obj + 3, out3);
}

// out2 = norm_bounds, norm_c
void model_norms_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub, double out2[2]) {
    const int n = (int)c->n, m = (int)c->m, N = n + m;
    const int g = vec_grid(N);
    c->it_partials.resize((size_t)4 * 1024);
    hipLaunchKernelGGL(model_norms_kernel, dim3(g), dim3(kBlock), 0, c->stream, n, m, b, cc, lb, ub, c->it_partials.get());
    std::vector<double> h((size_t)2 * g);
    c->it_partials.download(h.data(), h.size(), c->stream);
    IPXK_HIP(hipGetLastError());
    out2[0] = out2[1] = 0.0;
    for (int i = 0; i < g; i++) { out2[0] = std::max(out2[0], h[i]); out2[1] = std::max(out2[1], h[(size_t)g + i]); }
    const CombineOp ops[2] = {kCombineMax, kCombineMax};
    combine_over_ranks(c, out2, ops, 2);
}

void iterate_update_dev(Context* c, double sp, const double* dx, const double* dxl, const double* dxu, double sd,
                        const double* dy, const double* dzl, const double* dzu) {
    IPXK_REQUIRE(c->it_set, "no iterate on the device (ipxk_iterate_set)");
    IPXK_REQUIRE(!c->postprocessed, kPostprocessedRefusal);
    const int n = (int)c->n, m = (int)c->m, N = n + m;
    hipLaunchKernelGGL(iterate_update_kernel, dim3(vec_grid(N)), dim3(kBlock), 0, c->stream, N, m, c->it_state.get(),
                       c->it_x.get(), c->it_xl.get(), c->it_xu.get(), c->it_y.get(), c->it_zl.get(), c->it_zu.get(),
                       sp, dx, dxl, dxu, sd, dy, dzl, dzu);
    IPXK_HIP(hipGetLastError());
}

void iterate_residuals_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub,
                           double* rb, double* rc, double* rl, double* ru, double* presidual, double* dresidual) {
    IterScalars S;
    iterate_scalars_dev(c, kIterResiduals, b, cc, lb, ub, rb, rc, rl, ru, &S);
    if (presidual) *presidual = S.presidual;
    if (dresidual) *dresidual = S.dresidual;
}

void iterate_complementarity_dev(Context* c, double out4[4], double* num_terms) {
    IterScalars S;
    iterate_scalars_dev(c, kIterComplementarity, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &S);
    std::copy(S.comp, S.comp + 4, out4);
    if (num_terms) *num_terms = S.num_terms;
}

// rank-local on every context: a generic vector primitive (the IPM step takes steps_to_boundary below)
double step_to_boundary_dev(Context* c, const double* x, const double* dx, int64_t len, double alpha0,
                            ipxint* blocking) {
    IPXK_REQUIRE(len >= 0 && len < (int64_t(1) << 31), "bad length");
    const int g = vec_grid(len);
    c->it_partials.resize((size_t)4 * 1024);
    hipLaunchKernelGGL(step_to_boundary_kernel, dim3(g), dim3(kBlock), 0, c->stream, (int)len, x, dx, alpha0,
                       c->it_partials.get(), c->it_partials.get() + g);
    std::vector<double> h((size_t)2 * g);
    c->it_partials.download(h.data(), h.size(), c->stream);
    IPXK_HIP(hipGetLastError());
    // the smallest step below alpha0 and the smallest index attaining it.  Block b holds the elements b*kBlock + t of
    // every grid pass, so among tied blocks the smallest index need not be the first block's: compare the indices
    double alpha = alpha0;
    int idx = INT_MAX;
    for (int i = 0; i < g; i++)
        if (h[i] < alpha0) take_smaller(alpha, idx, h[i], (int)h[(size_t)g + i]);
    if (blocking) *blocking = idx == INT_MAX ? -1 : idx;
    return alpha;
}

// the four problems over this rank's share (slack entries on rank 0 only), one all-gather of the rows (a download
// without a communicator), and per problem the lexicographic minimum of (alpha, global index) over the ranks -- the
// reference's first-index rule (ipm.cc:320-339) on the whole vector.  The winner's x, dx, z, dz come with it.
void steps_to_boundary(Context* c, const BoundaryVectors& V, double alpha0, Boundary out[4]) {
    learn_col_offsets(c);
    const int n = (int)c->n;
    const int len = with_replicated(c) ? (int)(c->n + c->m) : n;
    const int g = vec_grid(len);
    c->it_bnd.ensure((size_t)8 * g);
    c->it_row.ensure(24);
    const double* xs[4] = {V.xl, V.xu, V.zl, V.zu};
    const double* ds[4] = {V.dxl, V.dxu, V.dzl, V.dzu};
    for (int k = 0; k < 4; k++) {
        double* part = c->it_bnd.get() + (size_t)2 * g * k;
        hipLaunchKernelGGL(step_to_boundary_kernel, dim3(g), dim3(kBlock), 0, c->stream, len, xs[k], ds[k], alpha0, part,
                           part + g);
    }
    hipLaunchKernelGGL(boundary_row_kernel, dim3(1), dim3(256), 0, c->stream, g, c->it_bnd.get(), alpha0, n,
                       (double)c->col_offset, (double)c->n_global, V, c->it_row.get());
    IPXK_HIP(hipGetLastError());
    const std::vector<double> T = comm_gather_table(c, c->it_row.get(), 24);
    for (int k = 0; k < 4; k++) {
        Boundary b{alpha0, -1.0, 0.0, 0.0, 0.0, 0.0};
        for (int r = 0; r < c->nranks; r++) {
            const double* t = T.data() + (size_t)24 * r + 6 * k;
            if (t[1] < 0.0) continue;
            if (t[0] < b.alpha || (t[0] == b.alpha && (b.index < 0.0 || t[1] < b.index))) b = Boundary{t[0], t[1], t[2], t[3], t[4], t[5]};
        }
        out[k] = b;
    }
}

}  // namespace ipxk
