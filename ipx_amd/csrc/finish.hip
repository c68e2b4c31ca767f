// The end of the interior point solve on the device        reference src/iterate.cc, src/lp_solver.cc
//   Iterate::Postprocess            iterate.cc:250-313  xl, xu, zl, zu of the fixed and implied variables
//   Iterate::DropToComplementarity  iterate.cc:315-391  the complementary point crossover starts from
//   Iterate::ResidualsFromDropping  iterate.cc:393-448  what term_crit_reached asks with crossover_start > 0 (:237-248)
//   LpSolver::InteriorPointSolve    lp_solver.cc:305-462 starting point, initial iterations, starting basis, main phase,
//                                                       postprocessing, evaluation, the "imprecise" verdict
// The device keeps seven states (IPXK_STATE_*); the reference's StateDetail is derived from the state and the bounds
// (detail_of).  Every rule is local to a column, so on a column partition each rank treats [its structural slice; all m
// slack entries] and only the two dropping residuals are combined (max, slack terms on rank 0).  The products a_j'y of
// the structural columns are one pass of the column gather matrix with EpiPostprocess; a dense column of A is a long row
// of that matrix and takes the long-row kernel like any other epilogue.
// No kernel of this file uses scratch memory (-Rpass-analysis=kernel-resource-usage: ScratchSize 0 throughout).
#include "context.hpp"
#include "spmv_kernels.hpp"

namespace ipxk {

namespace {

const char* const kFinishRowRefusal =
    "the device IPM does not run on a row-partitioned system: partition the structural columns (ipxk_comm_init_columns)";

// StateDetail of the variables that Postprocess touches; everything else is kOther
enum Detail { kOther, kFixed, kImpliedEq, kImpliedLb, kImpliedUb };

__device__ __forceinline__ Detail detail_of(unsigned char st, double l, double u) {
    if (st == IPXK_STATE_FIXED) return kFixed;
    if (st == IPXK_STATE_FREE && l == u && isfinite(l)) return kImpliedEq;     // the slack of a dependent equality row
    if (st == IPXK_STATE_IMPLIED_LB) return kImpliedLb;                        // DropPrimal (drop.hip)
    if (st == IPXK_STATE_IMPLIED_UB) return kImpliedUb;
    return kOther;
}

struct IterateVectors { double *x, *xl, *xu, *zl, *zu; };

// :261-310 for variable j of detail d, aty = a_j'y
__device__ __forceinline__ void postprocess_variable(Detail d, int j, double cj, double aty, double l, double u,
                                                     const IterateVectors& V) {
    switch (d) {
    case kFixed: {
        const double xj = V.x[j];
        V.xl[j] = xj - l;
        V.xu[j] = u - xj;
        if (l == u) {
            const double z = cj - aty;
            if (z >= 0.0) V.zl[j] = z; else V.zu[j] = -z;
        }
        break;
    }
    case kImpliedEq: {
        const double z = cj - aty;
        if (z >= 0.0) { V.zl[j] = z; V.zu[j] = 0.0; } else { V.zl[j] = 0.0; V.zu[j] = -z; }
        V.x[j] = l;
        V.xl[j] = 0.0;                          // x - lb and ub - x at x = lb = ub
        V.xu[j] = 0.0;
        break;
    }
    case kImpliedLb:
        V.zl[j] = cj - aty; V.zu[j] = 0.0; V.x[j] = l; V.xl[j] = 0.0; V.xu[j] = u - l;
        break;
    case kImpliedUb:
        V.zl[j] = 0.0; V.zu[j] = -(cj - aty); V.x[j] = u; V.xl[j] = u - l; V.xu[j] = 0.0;
        break;
    case kOther:
        break;
    }
}

// structural columns: acc = A_j'y
struct EpiPostprocess : ProdMul {
    const unsigned char* state; const double* c; const double* lb; const double* ub; IterateVectors V;
    static constexpr bool kNeg = false;
    __device__ __forceinline__ double init(int) const { return 0.0; }
    __device__ __forceinline__ void finish(int j, double acc, double&) const {
        const double l = lb[j], u = ub[j];
        const Detail d = detail_of(state[j], l, u);
        if (d != kOther) postprocess_variable(d, j, c[j], acc, l, u, V);
    }
};

// slack columns: a_j'y = y_i
__global__ void postprocess_slack_kernel(int n, int m, const unsigned char* __restrict__ state, const double* __restrict__ c,
                                         const double* __restrict__ lb, const double* __restrict__ ub,
                                         const double* __restrict__ y, IterateVectors V) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const int j = n + i;
        const double l = lb[j], u = ub[j];
        const Detail d = detail_of(state[j], l, u);
        if (d != kOther) postprocess_variable(d, j, c[j], y[i], l, u, V);
    }
}

// per block: # structural and # slack variables that Postprocess touches
__global__ __launch_bounds__(kBlock) void postprocess_count_kernel(int n, int m, const unsigned char* __restrict__ state,
                                                                   const double* __restrict__ lb,
                                                                   const double* __restrict__ ub, double* out) {
    __shared__ double red[kBlock / 64 + 1];
    double ns = 0.0, nk = 0.0, bad = MinOp::identity();
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < n + m; j += gridDim.x * kBlock) {
        const Detail d = detail_of(state[j], lb[j], ub[j]);
        if (d != kOther) { if (j < n) ns += 1.0; else nk += 1.0; }
        // Iterate::assert_consistency (:500-513): the bound a variable is implied at is finite
        if ((d == kImpliedLb && !isfinite(lb[j])) || (d == kImpliedUb && !isfinite(ub[j]))) bad = fmin(bad, (double)j);
    }
    ns = block_reduce<SumOp>(ns, red);
    nk = block_reduce<SumOp>(nk, red);
    bad = block_reduce<MinOp>(bad, red);
    if (threadIdx.x == 0) { out[blockIdx.x] = ns; out[gridDim.x + blockIdx.x] = nk; out[2 * gridDim.x + blockIdx.x] = bad; }
}

// max |a_ij| of every structural column, 8 lanes per column
__global__ __launch_bounds__(kBlock) void column_max_kernel(int n, const int* __restrict__ Ap, const double* __restrict__ Ax,
                                                            double* __restrict__ colmax) {
    const int lane8 = threadIdx.x & 7;
    const int per = kBlock / 8;
    for (int j0 = blockIdx.x * per; j0 < n; j0 += gridDim.x * per) {     // uniform trip count: the shuffles see whole waves
        const int j = j0 + (threadIdx.x >> 3);
        double mx = 0.0;
        if (j < n)
            for (int p = Ap[j] + lane8; p < Ap[j + 1]; p += 8) mx = fmax(mx, fabs(Ax[p]));
        mx = wave_reduce<FmaxOp, 8>(mx);
        if (j < n && lane8 == 0) colmax[j] = mx;
    }
}

// :402-443; per block: max |xdrop| * amax, max |zdrop|
__global__ __launch_bounds__(kBlock) void dropping_residuals_kernel(int n, int len, const unsigned char* __restrict__ state,
                                                                    const double* __restrict__ lb, const double* __restrict__ ub,
                                                                    const double* __restrict__ x, const double* __restrict__ xl,
                                                                    const double* __restrict__ xu, const double* __restrict__ zl,
                                                                    const double* __restrict__ zu,
                                                                    const double* __restrict__ colmax, double* out) {
    __shared__ double red[kBlock / 64 + 1];
    double pres = 0.0, dres = 0.0;
    for (int j = blockIdx.x * kBlock + threadIdx.x; j < len; j += gridDim.x * kBlock) {
        const unsigned char st = state[j];
        if (st != IPXK_STATE_BARRIER_LB && st != IPXK_STATE_BARRIER_UB && st != IPXK_STATE_BARRIER_BOXED) continue;
        bool lower = st == IPXK_STATE_BARRIER_LB;
        if (st == IPXK_STATE_BARRIER_BOXED) lower = zl[j] / xl[j] >= zu[j] / xu[j];
        double xdrop = 0.0, zdrop = 0.0;
        if (lower) {
            if (zl[j] >= xl[j]) xdrop = x[j] - lb[j]; else zdrop = zl[j] - zu[j];
        } else {
            if (zu[j] >= xu[j]) xdrop = x[j] - ub[j]; else zdrop = zl[j] - zu[j];
        }
        const double amax = j < n ? colmax[j] : 1.0;
        pres = fmax(pres, fabs(xdrop) * amax);
        dres = fmax(dres, fabs(zdrop));
    }
    pres = block_reduce<MaxOp>(pres, red);
    dres = block_reduce<MaxOp>(dres, red);
    if (threadIdx.x == 0) { out[blockIdx.x] = pres; out[gridDim.x + blockIdx.x] = dres; }
}

// :328-390
__global__ void drop_to_complementarity_kernel(int N, int m, const double* __restrict__ lb, const double* __restrict__ ub,
                                               const double* __restrict__ xv, const double* __restrict__ xl,
                                               const double* __restrict__ xu, const double* __restrict__ yv,
                                               const double* __restrict__ zl, const double* __restrict__ zu,
                                               double* __restrict__ x, double* __restrict__ y, double* __restrict__ z) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += gridDim.x * blockDim.x) {
        if (j < m) y[j] = yv[j];
        const double l = lb[j], u = ub[j], xlj = xl[j], xuj = xu[j], zlj = zl[j], zuj = zu[j];
        double xj = xv[j];
        xj = xj < l ? l : xj;                   // std::max(xj, lb[j])
        xj = u < xj ? u : xj;                   // std::min(xj, ub[j])
        const double d = zlj - zuj;
        const double dpos = 0.0 < d ? d : 0.0, dneg = d < 0.0 ? d : 0.0;    // std::max(0.0, d), std::min(0.0, d)
        const bool fl = isfinite(l), fu = isfinite(u);
        double xo = xj, zo = 0.0;
        if (l == u) { xo = l; zo = d; }                                     // fixed variable
        else if (fl && fu) {                                                // boxed variable
            if (zlj * xuj >= zuj * xlj) { if (zlj >= xlj) { xo = l; zo = dpos; } }
            else if (zuj >= xuj) { xo = u; zo = dneg; }
        }
        else if (fl) { if (zlj >= xlj) { xo = l; zo = dpos; } }             // lower bound only
        else if (fu) { if (zuj >= xuj) { xo = u; zo = dneg; } }             // upper bound only
        x[j] = xo;
        z[j] = zo;
    }
}

void ensure_column_max(Context* c) {
    if (c->have_colmax) return;
    IPXK_REQUIRE(c->have_plain, "no resident copy of the matrix");
    const int n = (int)c->n;
    c->colmax.resize((size_t)std::max(n, 1));
    if (n > 0)
        hipLaunchKernelGGL(column_max_kernel, dim3(grid_for((int64_t)n * 8, 4096)), dim3(kBlock), 0, c->stream, n, c->pl_Ap.get(),
                           c->pl_Ax.get(), c->colmax.get());
    IPXK_HIP(hipGetLastError());
    c->have_colmax = true;
}

}  // namespace

void iterate_postprocess_dev(Context* c, const double* cc, const double* lb, const double* ub) {
    IPXK_REQUIRE(c->it_set, "no iterate on the device (ipxk_iterate_set)");
    IPXK_REQUIRE(!comm_rows(c), kFinishRowRefusal);
    const int n = (int)c->n, m = (int)c->m, N = n + m;
    hipStream_t s = c->stream;
    const int g = vec_grid(N);
    c->it_partials.resize((size_t)4 * 1024);
    hipLaunchKernelGGL(postprocess_count_kernel, dim3(g), dim3(kBlock), 0, s, n, m, c->it_state.get(), lb, ub, c->it_partials.get());
    std::vector<double> h((size_t)3 * g);
    c->it_partials.download(h.data(), h.size(), s);
    IPXK_HIP(hipGetLastError());
    double nstruct = 0.0, nslack = 0.0, bad = INFINITY;
    for (int i = 0; i < g; i++) { nstruct += h[i]; nslack += h[(size_t)g + i]; bad = std::min(bad, h[(size_t)2 * g + i]); }
    IPXK_REQUIRE(std::isinf(bad), "variable " + std::to_string((long long)bad) + " is implied at an infinite bound");
    const IterateVectors V{c->it_x.get(), c->it_xl.get(), c->it_xu.get(), c->it_zl.get(), c->it_zu.get()};
    if (nstruct > 0.0) {
        EpiPostprocess ep{{}, c->it_state.get(), cc, lb, ub, V};
        launch_spmv(c->Acols, c->it_y.get(), ep, nullptr, nullptr, s);
    }
    if (nslack > 0.0)
        hipLaunchKernelGGL(postprocess_slack_kernel, dim3(vec_grid(m)), dim3(kBlock), 0, s, n, m, c->it_state.get(), cc, lb, ub,
                           c->it_y.get(), V);
    IPXK_HIP(hipGetLastError());
    c->postprocessed = true;
    c->sb.clear();                                            // the main phase does not go on from a postprocessed iterate
    c->drv.clear();
}

void iterate_dropping_residuals_dev(Context* c, const double* lb, const double* ub, double out2[2]) {
    IPXK_REQUIRE(c->it_set, "no iterate on the device (ipxk_iterate_set)");
    IPXK_REQUIRE(!comm_rows(c), kFinishRowRefusal);
    ensure_column_max(c);
    const int n = (int)c->n, len = (int)(with_replicated(c) ? c->n + c->m : c->n);
    const int g = vec_grid(len);
    c->it_partials.resize((size_t)4 * 1024);
    hipLaunchKernelGGL(dropping_residuals_kernel, dim3(g), dim3(kBlock), 0, c->stream, n, len, c->it_state.get(), lb, ub,
                       c->it_x.get(), c->it_xl.get(), c->it_xu.get(), c->it_zl.get(), c->it_zu.get(), c->colmax.get(),
                       c->it_partials.get());
    std::vector<double> h((size_t)2 * g);
    c->it_partials.download(h.data(), h.size(), c->stream);
    IPXK_HIP(hipGetLastError());
    out2[0] = out2[1] = 0.0;
    for (int i = 0; i < g; i++) { out2[0] = std::max(out2[0], h[i]); out2[1] = std::max(out2[1], h[(size_t)g + i]); }
    const CombineOp ops[2] = {kCombineMax, kCombineMax};
    combine_over_ranks(c, out2, ops, 2);
}

void iterate_drop_to_complementarity_dev(Context* c, const double* lb, const double* ub, double* x, double* y, double* z) {
    IPXK_REQUIRE(c->it_set, "no iterate on the device (ipxk_iterate_set)");
    IPXK_REQUIRE(c->postprocessed, "the resident iterate has not been postprocessed (ipxk_iterate_postprocess)");
    const int m = (int)c->m, N = (int)(c->n + c->m);
    hipLaunchKernelGGL(drop_to_complementarity_kernel, dim3(vec_grid(N)), dim3(kBlock), 0, c->stream, N, m, lb, ub, c->it_x.get(),
                       c->it_xl.get(), c->it_xu.get(), c->it_y.get(), c->it_zl.get(), c->it_zu.get(), x, y, z);
    IPXK_HIP(hipGetLastError());
}

// LpSolver::InteriorPointSolve / RunIPM (lp_solver.cc:305-359); the status values are those of include/ipx_status.h
void ipm_solve_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub, const ipxk_solve_params* prm,
                   ipxk_solve_info* info, ipxint* basis_out, ipxint* status_out, ipxk_interrupt_fn interrupt, void* user) {
    IPXK_REQUIRE(!comm_active(c), kDeviceLuRefusal);
    IPXK_REQUIRE(prm->crossover_start >= 0.0, "crossover_start must not be negative (0: off)");
    constexpr ipxint kNotRun = 0, kOptimal = 1, kImprecise = 2, kPrimalInfeas = 3, kDualInfeas = 4, kTimeLimit = 5, kIterLimit = 6,
                     kNoProgress = 7, kFailed = 8;
    *info = ipxk_solve_info{};
    c->sum_primal_dropped = c->sum_dual_dropped = c->sum_drop_updates = 0;
    struct Restore {                            // crossover_start holds for this call
        Context* c; double saved;
        ~Restore() { c->crossover_start = saved; }
    } restore{c, c->crossover_start};
    c->crossover_start = prm->crossover_start;
    const ipxint m = (ipxint)c->m;
    ipxk_ipm_params ip{prm->kkt_tol, prm->feasibility_tol, prm->optimality_tol, -1, prm->ipm_maxiter, prm->precond_dense_cols};
    ipxk_ipm_info gi{};
    auto take = [&](const ipxk_ipm_info& g) {   // Info runs on across the phases
        info->status_ipm = g.status_ipm;
        info->errflag = g.errflag;
        info->iter += g.iter;
        info->kktiter += g.kktiter;
        info->basis_updates += g.basis_updates;
        info->step_primal = g.step_primal;
        info->step_dual = g.step_dual;
    };
    auto run = [&] {                            // RunIPM, :334-359
        if (!prm->use_resident_point) {
            begin_new_iterate(c);
            ipm_starting_point_dev(c, b, cc, lb, ub, &ip, &gi, interrupt, user);
            info->status_ipm = gi.status_ipm;
            info->errflag = gi.errflag;
            info->kktiter += gi.kktiter;
            if (info->status_ipm != kNotRun) return;
            // RunInitialIPM, :384-420
            if (prm->switchiter < 0) ip.kkt_maxiter = std::min<ipxint>(500, 10 + m / 20);
            else ip.ipm_maxiter = std::min(prm->switchiter, prm->ipm_maxiter);
            ipm_driver_dev(c, b, cc, lb, ub, &ip, &gi, interrupt, user);
            take(gi);
            info->iter_initial = gi.iter;
            info->status_initial = gi.status_ipm;
            switch (info->status_ipm) {
            case kOptimal: case kNoProgress: info->status_ipm = kNotRun; break;
            case kFailed: info->status_ipm = kNotRun; info->errflag = 0; break;
            case kIterLimit: if (info->iter < prm->ipm_maxiter) info->status_ipm = kNotRun; break;    // stopped at switchiter
            default: break;
            }
            if (info->status_ipm != kNotRun) return;
        } else {
            IPXK_REQUIRE(c->it_set, "use_resident_point: no iterate on the device (ipxk_ipm_load_starting_point)");
        }
        // BuildStartingBasis, :422-454
        const ipxk_starting_basis_params sp{prm->dependency_tol, prm->max_etas};
        ipxk_starting_basis_info si{};
        ipm_starting_basis_dev(c, b, cc, lb, ub, &sp, &si, basis_out, status_out, nullptr, 0, interrupt, user);
        info->dependent_rows = si.dependent_rows;
        info->dependent_cols = si.dependent_cols;
        info->rows_inconsistent = si.rows_inconsistent;
        info->cols_inconsistent = si.cols_inconsistent;
        info->updates_start = si.updates_start;
        if (si.errflag == 999) { info->status_ipm = kTimeLimit; info->errflag = 0; return; }
        if (si.errflag) { info->status_ipm = kFailed; info->errflag = si.errflag; return; }
        if (si.rows_inconsistent) { info->status_ipm = kPrimalInfeas; return; }
        if (si.cols_inconsistent) { info->status_ipm = kDualInfeas; return; }
        // RunMainIPM, :456-462: ipm_maxiter counts the iterations of both phases
        ip.kkt_maxiter = -1;
        ip.ipm_maxiter = prm->ipm_maxiter - info->iter;
        ipm_driver_dev(c, b, cc, lb, ub, &ip, &gi, interrupt, user, true, basis_out, status_out);
        take(gi);
    };
    run();
    // :317-331
    iterate_postprocess_dev(c, cc, lb, ub);
    const int N = (int)(c->n + c->m);
    for (int k = 0; k < 4; k++) c->ipm[k].resize((size_t)std::max(k == 0 ? (int)c->m : N, 1));
    IterScalars S;
    iterate_scalars_dev(c, kIterResiduals | kIterComplementarity | kIterObjectives, b, cc, lb, ub, c->ipm[0].get(), c->ipm[1].get(),
                        c->ipm[2].get(), c->ipm[3].get(), &S);
    double norms[2], drop[2];
    model_norms_dev(c, b, cc, lb, ub, norms);
    iterate_dropping_residuals_dev(c, lb, ub, drop);
    info->pobjective = S.obj[0];
    info->dobjective = S.obj[1];
    info->presidual = info->abs_presidual = S.presidual;
    info->dresidual = info->abs_dresidual = S.dresidual;
    info->complementarity = S.comp[0];
    info->mu = S.comp[1];
    info->rel_presidual = S.presidual / (1.0 + norms[0]);
    info->rel_dresidual = S.dresidual / (1.0 + norms[1]);
    info->rel_objgap = (S.obj[0] - S.obj[1]) / (1.0 + 0.5 * std::abs(S.obj[0] + S.obj[1]));
    info->pres_dropping = drop[0];
    info->dres_dropping = drop[1];
    if (info->status_ipm == kOptimal &&
        (std::abs(info->rel_objgap) > prm->optimality_tol || info->rel_presidual > prm->feasibility_tol ||
         info->rel_dresidual > prm->feasibility_tol))
        info->status_ipm = kImprecise;
}

}  // namespace ipxk
