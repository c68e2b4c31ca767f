// The IPM starting point on the device                     reference src/ipm.cc, src/iterate.cc
//   IPM::ComputeStartingPoint  ipm.cc:125-259   two KKT solves with G = I, elementwise passes around them
//   IPM::LoadStartingPoint     ipm.cc:261-316   repair of a point the caller supplies
//   Iterate::Initialize        iterate.cc:61-92 the states from the bounds (lb == ub: BARRIER_BOXED)
//   Iterate::Iterate           iterate.cc:31-57 the point left behind when a solve fails
// The iterate is built in place in the resident vectors (it_*).  Every scalar is a reduction of per-block partials
// summed on the host in block order (no atomics, so two calls agree bit for bit); on a column partition each rank's
// value goes through combine_over_ranks, the slack entries counting on rank 0 only.
#include "context.hpp"
#include "spmv_kernels.hpp"

namespace ipxk {

namespace {

constexpr double kNoIndex = 9.0e15;     // "no invalid entry" of the per-block index minima

// Iterate::Initialize, iterate.cc:76-88
__device__ __forceinline__ unsigned char initial_state(double l, double u) {
    if (l == u) return IPXK_STATE_BARRIER_BOXED;
    if (isfinite(l) && isfinite(u)) return IPXK_STATE_BARRIER_BOXED;
    if (isfinite(l)) return IPXK_STATE_BARRIER_LB;
    if (isfinite(u)) return IPXK_STATE_BARRIER_UB;
    return IPXK_STATE_FREE;
}

// per block: the smallest j with lb > ub, lb = +inf, ub = -inf, or a NaN in c, lb, ub (or in b, j < m)
__global__ __launch_bounds__(kBlock) void start_check_kernel(int N, int m, const double* __restrict__ b,
                                                             const double* __restrict__ c, const double* __restrict__ lb,
                                                             const double* __restrict__ ub, double* out) {
    __shared__ double red[kBlock / 64 + 1];
    double bad = kNoIndex;
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < N; j += gridDim.x * kBlock) {
        const double l = lb[j], u = ub[j];
        const bool ok = l <= u && l != __builtin_huge_val() && u != -__builtin_huge_val() && !isnan(c[j]) &&
                        !(j < m && isnan(b[j]));      // l <= u is false for a NaN in either
        if (!ok && j < bad) bad = (double)j;
    }
    bad = block_reduce<MinOp>(bad, red);
    if (threadIdx.x == 0) out[blockIdx.x] = bad;
}

// x = clamp(0, lb, ub), ipm.cc:145-155
__global__ void start_clamp_kernel(int N, const double* __restrict__ lb, const double* __restrict__ ub,
                                   double* __restrict__ x) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += gridDim.x * blockDim.x) {
        double xj = 0.0;
        if (xj < lb[j]) xj = lb[j];
        if (xj > ub[j]) xj = ub[j];
        x[j] = xj;
    }
}

// per block: max |v|
__global__ __launch_bounds__(kBlock) void start_absmax_kernel(int len, const double* __restrict__ v, double* out) {
    __shared__ double red[kBlock / 64 + 1];
    double mx = 0.0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < len; i += gridDim.x * kBlock) mx = fmax(mx, fabs(v[i]));
    mx = block_reduce<MaxOp>(mx, red);
    if (threadIdx.x == 0) out[blockIdx.x] = mx;
}

// x += dx, xl = x - lb, xu = ub - x (:161-172); per block: xinfeas (max), sum c_j^2 over j < nsum (:174), max |c_j|
// (:184)
__global__ __launch_bounds__(kBlock) void start_primal_kernel(int N, int nsum, const double* __restrict__ lb,
                                                              const double* __restrict__ ub, const double* __restrict__ c,
                                                              const double* __restrict__ dx, double* __restrict__ x,
                                                              double* __restrict__ xl, double* __restrict__ xu, double* out) {
    __shared__ double red[kBlock / 64 + 1];
    double xinf = 0.0, c2 = 0.0, cmax = 0.0;
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < N; j += gridDim.x * kBlock) {
        const double xj = x[j] + dx[j];
        x[j] = xj;
        const double l = xj - lb[j], u = ub[j] - xj;
        xl[j] = l;
        xu[j] = u;
        xinf = fmax(xinf, fmax(-l, -u));
        const double cj = c[j];
        if (j < nsum) c2 += cj * cj;
        cmax = fmax(cmax, fabs(cj));
    }
    xinf = block_reduce<MaxOp>(xinf, red);
    c2 = block_reduce<SumOp>(c2, red);
    cmax = block_reduce<MaxOp>(cmax, red);
    if (threadIdx.x == 0) {
        const int G = gridDim.x, b = blockIdx.x;
        out[b] = xinf; out[G + b] = c2; out[2 * G + b] = cmax;
    }
}

// zl[j] = c[j] - A_j'y on the structural columns (:193-194), dot += zl[j]^2
struct EpiStartZ : ProdMul {
    const double* c; double* out;
    static constexpr bool kNeg = false;
    __device__ __forceinline__ double init(int) const { return 0.0; }
    __device__ __forceinline__ void finish(int j, double acc, double& dot) const {
        const double z = c[j] - acc;
        out[j] = z;
        dot += z * z;
    }
};

// ... and on the slack columns, zl[n+i] = c[n+i] - y[i]; per block: sum zl^2 if count
__global__ __launch_bounds__(kBlock) void start_slack_z_kernel(int n, int m, int count, const double* __restrict__ c,
                                                               const double* __restrict__ y, double* __restrict__ zl,
                                                               double* out) {
    __shared__ double red[kBlock / 64 + 1];
    double s = 0.0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < m; i += gridDim.x * kBlock) {
        const double z = c[n + i] - y[i];
        zl[n + i] = z;
        if (count) s += z * z;
    }
    s = block_reduce<SumOp>(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// zl += rho c and y *= yscale when rho != 0 (:202-207), the split into zl, zu by the bounds (:210-221); per block:
// zinfeas (max)
__global__ __launch_bounds__(kBlock) void start_split_kernel(int N, int m, double rho, double yscale,
                                                             const double* __restrict__ lb, const double* __restrict__ ub,
                                                             const double* __restrict__ c, double* __restrict__ zl,
                                                             double* __restrict__ zu, double* __restrict__ y, double* out) {
    __shared__ double red[kBlock / 64 + 1];
    double zinf = 0.0;
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < N; j += gridDim.x * kBlock) {
        double zval = zl[j];
        if (rho != 0.0) {
            zval = zval + rho * c[j];
            if (j < m) y[j] = y[j] * yscale;
        }
        const bool fl = isfinite(lb[j]), fu = isfinite(ub[j]);
        double l = 0.0, u = 0.0;
        if (fl && fu) { l = 0.5 * zval; u = -0.5 * zval; }
        else if (fl) l = zval;
        else if (fu) u = -zval;
        zl[j] = l;
        zu[j] = u;
        zinf = fmax(zinf, fmax(-l, -u));
    }
    zinf = block_reduce<MaxOp>(zinf, red);
    if (threadIdx.x == 0) out[blockIdx.x] = zinf;
}

// per block over j < nsum: the sums of xl, zl and xl.*zl over the finite bounds (:226-240), the first shifts applied
// on the fly (zero_obj: zl, zu = 1 at a finite bound, :176-181)
__global__ __launch_bounds__(kBlock) void start_level_kernel(int nsum, int zero_obj, double xshift1, double zshift1,
                                                             const double* __restrict__ lb, const double* __restrict__ ub,
                                                             const double* __restrict__ xl, const double* __restrict__ xu,
                                                             const double* __restrict__ zl, const double* __restrict__ zu,
                                                             double* out) {
    __shared__ double red[kBlock / 64 + 1];
    double xs = 0.0, zs = 0.0, mu = 0.0;
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < nsum; j += gridDim.x * kBlock) {
        if (isfinite(lb[j])) {
            const double x = xl[j] + xshift1, z = zero_obj ? 1.0 : zl[j] + zshift1;
            xs += x; zs += z; mu += x * z;
        }
        if (isfinite(ub[j])) {
            const double x = xu[j] + xshift1, z = zero_obj ? 1.0 : zu[j] + zshift1;
            xs += x; zs += z; mu += x * z;
        }
    }
    xs = block_reduce<SumOp>(xs, red);
    zs = block_reduce<SumOp>(zs, red);
    mu = block_reduce<SumOp>(mu, red);
    if (threadIdx.x == 0) {
        const int G = gridDim.x, b = blockIdx.x;
        out[b] = xs; out[G + b] = zs; out[2 * G + b] = mu;
    }
}

// both shifts of xl, xu, zl, zu (:171-172, :222-224, :243-251) and the states (Iterate::Initialize), in place
__global__ void start_final_kernel(int N, int zero_obj, double xshift1, double xshift2, double zshift1, double zshift2,
                                   const double* __restrict__ lb, const double* __restrict__ ub, double* __restrict__ xl,
                                   double* __restrict__ xu, double* __restrict__ zl, double* __restrict__ zu,
                                   unsigned char* __restrict__ state) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += gridDim.x * blockDim.x) {
        const double l = lb[j], u = ub[j];
        const bool fl = isfinite(l), fu = isfinite(u);
        xl[j] = (xl[j] + xshift1) + xshift2;
        xu[j] = (xu[j] + xshift1) + xshift2;
        double zlj, zuj;
        if (zero_obj) {
            zlj = fl ? 1.0 : 0.0;
            zuj = fu ? 1.0 : 0.0;
        } else {
            zlj = zl[j];
            zuj = zu[j];
            if (fl) zlj += zshift1;
            if (fu) zuj += zshift1;
        }
        if (fl) zlj += zshift2;
        if (fu) zuj += zshift2;
        zl[j] = zlj;
        zu[j] = zuj;
        state[j] = initial_state(l, u);
    }
}

// the point of the Iterate constructor (iterate.cc:31-57): x = 0, y = 0, xl / xu / zl / zu = 1 / inf / 0 by bound kind
__global__ void start_constructor_kernel(int N, int m, const double* __restrict__ lb, const double* __restrict__ ub,
                                         double* __restrict__ x, double* __restrict__ xl, double* __restrict__ xu,
                                         double* __restrict__ y, double* __restrict__ zl, double* __restrict__ zu,
                                         unsigned char* __restrict__ state) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += gridDim.x * blockDim.x) {
        const bool fl = isfinite(lb[j]), fu = isfinite(ub[j]);
        x[j] = 0.0;
        if (j < m) y[j] = 0.0;
        xl[j] = fl ? 1.0 : __builtin_huge_val();
        zl[j] = fl ? 1.0 : 0.0;
        xu[j] = fu ? 1.0 : __builtin_huge_val();
        zu[j] = fu ? 1.0 : 0.0;
        state[j] = initial_state(lb[j], ub[j]);
    }
}

// what LoadStartingPoint asserts of one pair (ipm.cc:287-309)
__device__ __forceinline__ bool pair_valid(double bound, double x, double z) {
    if (isfinite(bound)) return isfinite(x) && x >= 0.0 && isfinite(z) && z >= 0.0;
    return x == __builtin_huge_val() && z == 0.0;
}

// per block: the smallest j with an invalid pair, and over j < nsum the sum of the products with both factors > 0
// and their number (:270-283)
__global__ __launch_bounds__(kBlock) void load_check_kernel(int N, int nsum, const double* __restrict__ lb,
                                                            const double* __restrict__ ub, const double* __restrict__ xl,
                                                            const double* __restrict__ xu, const double* __restrict__ zl,
                                                            const double* __restrict__ zu, double* out) {
    __shared__ double red[kBlock / 64 + 1];
    double bad = kNoIndex, sum = 0.0, cnt = 0.0;
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < N; j += gridDim.x * kBlock) {
        const double xlj = xl[j], xuj = xu[j], zlj = zl[j], zuj = zu[j];
        if ((!pair_valid(lb[j], xlj, zlj) || !pair_valid(ub[j], xuj, zuj)) && j < bad) bad = (double)j;
        if (j < nsum) {
            if (xlj > 0.0 && zlj > 0.0) { sum += xlj * zlj; cnt += 1.0; }
            if (xuj > 0.0 && zuj > 0.0) { sum += xuj * zuj; cnt += 1.0; }
        }
    }
    bad = block_reduce<MinOp>(bad, red);
    sum = block_reduce<SumOp>(sum, red);
    cnt = block_reduce<SumOp>(cnt, red);
    if (threadIdx.x == 0) {
        const int G = gridDim.x, b = blockIdx.x;
        out[b] = bad; out[G + b] = sum; out[2 * G + b] = cnt;
    }
}

__device__ __forceinline__ void repair_pair(double bound, double& x, double& z, double mu, double sqrt_mu) {
    if (!isfinite(bound)) return;
    if (x == 0.0 && z == 0.0) x = z = sqrt_mu;
    else if (x == 0.0) x = mu / z;
    else if (z == 0.0) z = mu / x;
}

// the repair of zero entries (:285-311) and the states (Iterate::Initialize), in place
__global__ void load_repair_kernel(int N, double mu, double sqrt_mu, const double* __restrict__ lb,
                                   const double* __restrict__ ub, double* __restrict__ xl, double* __restrict__ xu,
                                   double* __restrict__ zl, double* __restrict__ zu, unsigned char* __restrict__ state) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += gridDim.x * blockDim.x) {
        const double l = lb[j], u = ub[j];
        double xlj = xl[j], xuj = xu[j], zlj = zl[j], zuj = zu[j];
        repair_pair(l, xlj, zlj, mu, sqrt_mu);
        repair_pair(u, xuj, zuj, mu, sqrt_mu);
        xl[j] = xlj; xu[j] = xuj; zl[j] = zlj; zu[j] = zuj;
        state[j] = initial_state(l, u);
    }
}

const char* const kStartRowRefusal =
    "the device IPM does not run on a row-partitioned system: partition the structural columns (ipxk_comm_init_columns)";

// this rank's reduction of k arrays of g block partials in it_partials, in block order (sum; max from 0; min)
void reduce_block_partials(Context* c, int g, const CombineOp* ops, int k, double* row) {
    std::vector<double> h((size_t)k * g);
    c->it_partials.download(h.data(), h.size(), c->stream);
    IPXK_HIP(hipGetLastError());
    for (int f = 0; f < k; f++) {
        double v = ops[f] == kCombineMin ? kNoIndex : 0.0;
        for (int i = 0; i < g; i++) {
            const double w = h[(size_t)f * g + i];
            v = ops[f] == kCombineSum ? v + w : ops[f] == kCombineMax ? std::max(v, w) : std::min(v, w);
        }
        row[f] = v;
    }
}

// ComputeStartingPoint after Factorize(nullptr); returns the errflag of a KKT solve (0: the point is in it_*)
ipxint compute_point(Context* c, const double* b, const double* cc, const double* lb, const double* ub, ipxint maxiter,
                     ipxk_ipm_info* info, ipxk_interrupt_fn interrupt, void* user) {
    const int n = (int)c->n, m = (int)c->m, N = n + m;
    const int nsum = with_replicated(c) ? N : n;
    const int g = vec_grid(N), gm = vec_grid(m);
    hipStream_t s = c->stream;
    double *x = c->it_x.get(), *xl = c->it_xl.get(), *xu = c->it_xu.get(), *y = c->it_y.get();
    double *zl = c->it_zl.get(), *zu = c->it_zu.get();
    double *rb = c->ipm[0].get(), *zero = c->ipm[1].get(), *dx = c->ipm[6].get(), *unused = c->ipm[7].get();
    double* part = c->it_partials.get();

    // :144-159  x within its bounds, rb = b - AI x, the minimum-norm correction
    hipLaunchKernelGGL(start_clamp_kernel, dim3(g), dim3(kBlock), 0, s, N, lb, ub, x);
    residual_rb(c, b, x, rb);
    hipLaunchKernelGGL(start_absmax_kernel, dim3(gm), dim3(kBlock), 0, s, m, rb, part);
    const CombineOp max1 = kCombineMax, sum1 = kCombineSum;
    double rbinf = 0.0;
    reduce_block_partials(c, gm, &max1, 1, &rbinf);           // rb is replicated: no exchange
    IPXK_HIP(hipMemsetAsync(zero, 0, sizeof(double) * N, s));
    CrResult r = kkt_diag_solve_dev(c, zero, rb, 0.1 * rbinf, maxiter, dx, y, interrupt, user, nullptr);
    info->kktiter += r.iter;
    if (r.errflag) return r.errflag;

    // :160-172
    hipLaunchKernelGGL(start_primal_kernel, dim3(g), dim3(kBlock), 0, s, N, nsum, lb, ub, cc, dx, x, xl, xu, part);
    double row[3];
    const CombineOp ops1[3] = {kCombineMax, kCombineSum, kCombineMax};
    reduce_block_partials(c, g, ops1, 3, row);
    combine_over_ranks(c, row, ops1, 3);
    const double xshift1 = 1.0 + 1.5 * row[0];
    const double cnorm = std::sqrt(row[1]), cinf = row[2];
    const bool zero_obj = cnorm == 0.0;

    double zshift1 = 0.0;
    if (!zero_obj) {
        // :185-224  y from AI'y ~ c, zl = c - AI'y, the 0.05 c correction, the split and the first shift
        IPXK_HIP(hipMemsetAsync(rb, 0, sizeof(double) * m, s));
        r = kkt_diag_solve_dev(c, cc, rb, 0.1 * cinf, maxiter, unused, y, interrupt, user, nullptr);
        info->kktiter += r.iter;
        if (r.errflag) return r.errflag;
        EpiStartZ ez{{}, cc, zl};
        const int np = launch_spmv(c->Acols, y, ez, c->part(kPartScratch), nullptr, s);
        hipLaunchKernelGGL(start_slack_z_kernel, dim3(gm), dim3(kBlock), 0, s, n, m, with_replicated(c) ? 1 : 0, cc, y,
                           zl, part);
        std::vector<double> hp((size_t)std::max(np, 1));
        if (np > 0) staged_d2h(hp.data(), c->part(kPartScratch), sizeof(double) * (size_t)np, s);
        double zsq = 0.0;
        reduce_block_partials(c, gm, &sum1, 1, &zsq);
        double zstruct = 0.0;
        for (int i = 0; i < np; i++) zstruct += hp[i];
        zsq = zstruct + zsq;
        combine_over_ranks(c, &zsq, &sum1, 1);
        const double rho = 0.05;
        const bool add_c = std::sqrt(zsq) < rho * cnorm;
        hipLaunchKernelGGL(start_split_kernel, dim3(g), dim3(kBlock), 0, s, N, m, add_c ? rho : 0.0, 1.0 - rho, lb, ub,
                           cc, zl, zu, y, part);
        double zinfeas = 0.0;
        reduce_block_partials(c, g, &max1, 1, &zinfeas);
        combine_over_ranks(c, &zinfeas, &max1, 1);
        zshift1 = 1.0 + 1.5 * zinfeas;
    }

    // :226-251  level the complementarity products
    const int gs = vec_grid(nsum);
    hipLaunchKernelGGL(start_level_kernel, dim3(gs), dim3(kBlock), 0, s, nsum, zero_obj ? 1 : 0, xshift1, zshift1, lb,
                       ub, xl, xu, zl, zu, part);
    const CombineOp ops3[3] = {kCombineSum, kCombineSum, kCombineSum};
    reduce_block_partials(c, gs, ops3, 3, row);
    combine_over_ranks(c, row, ops3, 3);
    const double xsum = 1.0 + row[0], zsum = 1.0 + row[1], mu = 1.0 + row[2];
    const double xshift2 = 0.5 * mu / zsum, zshift2 = 0.5 * mu / xsum;
    hipLaunchKernelGGL(start_final_kernel, dim3(g), dim3(kBlock), 0, s, N, zero_obj ? 1 : 0, xshift1, xshift2, zshift1,
                       zshift2, lb, ub, xl, xu, zl, zu, c->it_state.get());
    IPXK_HIP(hipGetLastError());
    return 0;
}

}  // namespace

void ipm_starting_point_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub,
                            const ipxk_ipm_params* prm, ipxk_ipm_info* info, ipxk_interrupt_fn interrupt, void* user) {
    IPXK_REQUIRE(!comm_rows(c), kStartRowRefusal);
    const int n = (int)c->n, m = (int)c->m, N = n + m;
    hipStream_t s = c->stream;
    const bool args = b && cc && lb && ub && prm && info;
    if (!comm_cols(c)) IPXK_REQUIRE(args, "NULL argument");
    c->it_partials.resize((size_t)4 * 1024);
    std::string err = args ? std::string() : std::string("NULL argument");
    if (args) {
        const int g = vec_grid(N);
        hipLaunchKernelGGL(start_check_kernel, dim3(g), dim3(kBlock), 0, s, N, m, b, cc, lb, ub, c->it_partials.get());
        const CombineOp op = kCombineMin;
        double bad = kNoIndex;
        reduce_block_partials(c, g, &op, 1, &bad);
        if (bad < kNoIndex)
            err = "ipxk_ipm_starting_point: invalid model entry " + std::to_string((long long)bad) +
                  " (lb > ub, lb = +inf, ub = -inf, or a NaN in b, c, lb or ub)";
    }
    if (comm_cols(c))
        agree_on_arguments(c, err, args ? model_fingerprint(c, b, cc, lb, ub) : 0, "ipxk_ipm_starting_point",
                           "b and the slack parts of c, lb and ub");
    else if (!err.empty())
        throw Error(IPXK_E_ARGUMENT, err);

    *info = ipxk_ipm_info{};
    c->it_set = false;
    DevBuf<double>* it[6] = {&c->it_x, &c->it_xl, &c->it_xu, &c->it_y, &c->it_zl, &c->it_zu};
    for (int k = 0; k < 6; k++) it[k]->resize((size_t)std::max(k == 3 ? m : N, 1));
    c->it_state.resize((size_t)std::max(N, 1));
    for (int k = 0; k < 12; k++) c->ipm[k].resize((size_t)std::max(k == 0 || k == 9 ? m : N, 1));

    ipxint errflag = 0;
    kkt_diag_factorize_dev(c, nullptr, nullptr, nullptr, nullptr, 0.0, prm->precond_dense_cols != 0, &errflag);   // :137
    if (!errflag) errflag = compute_point(c, b, cc, lb, ub, prm->kkt_maxiter, info, interrupt, user);
    if (errflag)
        hipLaunchKernelGGL(start_constructor_kernel, dim3(vec_grid(N)), dim3(kBlock), 0, s, N, m, lb, ub, c->it_x.get(),
                           c->it_xl.get(), c->it_xu.get(), c->it_y.get(), c->it_zl.get(), c->it_zu.get(), c->it_state.get());
    IPXK_HIP(hipGetLastError());
    IPXK_HIP(hipStreamSynchronize(s));
    c->it_set = true;

    // ipm.cc:31-41
    if (errflag == 999) info->status_ipm = 5;            // IPX_ERROR_interrupt_time -> IPX_STATUS_time_limit
    else if (errflag) { info->status_ipm = 8; info->errflag = errflag; }   // IPX_STATUS_failed
    else info->status_ipm = 0;                           // IPX_STATUS_not_run
    IterScalars S;                                       // the driver's one-table evaluation of the point
    iterate_scalars_dev(c, kIterResiduals | kIterComplementarity | kIterObjectives, b, cc, lb, ub, c->ipm[0].get(),
                        c->ipm[1].get(), c->ipm[2].get(), c->ipm[3].get(), &S);
    info->presidual = S.presidual;
    info->dresidual = S.dresidual;
    info->complementarity = S.comp[0];
    info->mu = S.comp[1];
    info->pobjective = S.obj[0] + S.obj[2];
    info->dobjective = S.obj[1] + S.obj[2];
}

void ipm_load_starting_point_dev(Context* c, const double* lb, const double* ub) {
    const int n = (int)c->n, m = (int)c->m, N = n + m;
    const int nsum = with_replicated(c) ? N : n;
    const int g = vec_grid(N);
    hipStream_t s = c->stream;
    c->it_partials.resize((size_t)4 * 1024);
    hipLaunchKernelGGL(load_check_kernel, dim3(g), dim3(kBlock), 0, s, N, nsum, lb, ub, c->it_xl.get(), c->it_xu.get(),
                       c->it_zl.get(), c->it_zu.get(), c->it_partials.get());
    double row[3];
    const CombineOp ops[3] = {kCombineMin, kCombineSum, kCombineSum};
    reduce_block_partials(c, g, ops, 3, row);
    std::string err;
    if (row[0] < kNoIndex)
        err = "ipxk_ipm_load_starting_point: invalid starting point at entry " + std::to_string((long long)row[0]) +
              (comm_cols(c) ? " of this rank's vectors" : "") +
              " (a finite bound needs finite, nonnegative x and z; an infinite one x = inf and z = 0)";
    if (comm_cols(c)) {
        // y and the slack parts of x, xl, xu, zl, zu, lb, ub
        std::vector<double> h((size_t)8 * m);
        const double* src[8] = {c->it_y.get(), c->it_x.get() + n, c->it_xl.get() + n, c->it_xu.get() + n,
                                c->it_zl.get() + n, c->it_zu.get() + n, lb + n, ub + n};
        for (int k = 0; k < 8; k++) staged_d2h(h.data() + (size_t)k * m, src[k], sizeof(double) * (size_t)m, s);
        Fingerprint F;
        F.add(h.data(), h.size());
        agree_on_arguments(c, err, F.h, "ipxk_ipm_load_starting_point", "y and the slack parts of x, xl, xu, zl, zu, lb and ub");
    } else if (!err.empty()) {
        throw Error(IPXK_E_ARGUMENT, err);
    }
    combine_over_ranks(c, row + 1, ops + 1, 2);
    const double mu = row[2] > 0.0 ? row[1] / row[2] : 1.0;     // :284
    hipLaunchKernelGGL(load_repair_kernel, dim3(g), dim3(kBlock), 0, s, N, mu, std::sqrt(mu), lb, ub, c->it_xl.get(),
                       c->it_xu.get(), c->it_zl.get(), c->it_zu.get(), c->it_state.get());
    IPXK_HIP(hipGetLastError());
    IPXK_HIP(hipStreamSynchronize(s));
    c->it_set = true;
}

}  // namespace ipxk
