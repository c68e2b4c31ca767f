// KKTSolverBasis::_Solve (reference src/kkt_solver_basis.cc:75-194) on the basis-preconditioned operator (trisolve.hip).
#include "context.hpp"
#include "spmv_kernels.hpp"
#include "trisolve.hpp"

namespace ipxk {

// slack columns: tI[i] = W[n+i]*(a[n+i] - work[i])  (work == nullptr: W*a)   (:102-120, :178-188)
__global__ void basis_slack_kernel(int m, const double* __restrict__ WI, const double* __restrict__ aI,
                                   const double* __restrict__ work, double* __restrict__ tI) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const double s = WI[i];
        tI[i] = s != 0.0 ? (aI[i] - (work ? work[i] : 0.0)) * s : 0.0;
    }
}
// out[i] = acc + tI[i]  (acc = sum_j a_ij t_j starting from 0)
struct EpiBasisRhs : ProdMul {
    const double* tI; double* out;
    static constexpr bool kNeg = false;
    __device__ __forceinline__ double init(int) const { return 0.0; }
    __device__ __forceinline__ void finish(int i, double acc, double&) const { out[i] = acc + tI[i]; }
};
// out[i] = (b[i] - sum_j a_ij x_j) - tI[i]
struct EpiBasisResidual : ProdMul {
    const double* b; const double* tI; double* out;
    static constexpr bool kNeg = true;
    __device__ __forceinline__ double init(int i) const { return b[i]; }
    __device__ __forceinline__ void finish(int i, double acc, double&) const { out[i] = acc - tI[i]; }
};

// out[p] = v[loc[p]] for structural columns of this rank, 0 otherwise (an owner's contribution)
__global__ void pos_contrib_kernel(int m, int n, const int* __restrict__ loc, const double* __restrict__ v, double* __restrict__ out) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < m; p += gridDim.x * blockDim.x) {
        const int l = loc[p];
        out[p] = l >= 0 && l < n ? v[l] : 0.0;
    }
}
// after the all-reduce: slack positions from the replicated slack part
__global__ void pos_slack_kernel(int m, int n, const int* __restrict__ loc, const double* __restrict__ v, double* __restrict__ out) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < m; p += gridDim.x * blockDim.x) {
        const int l = loc[p];
        if (l >= n) out[p] = v[l];
    }
}
// kernels by basis position p: pos_status, pos_scale and aB hold status, colscale and a of column basis[p]
// work[p] = aB[p] for BASIC_FREE positions, 0 otherwise                     (:87-97)
__global__ void basis_free_rhs_pos_kernel(int m, const int* __restrict__ pos_status, const double* __restrict__ aB,
                                          double* __restrict__ work) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < m; p += gridDim.x * blockDim.x)
        work[p] = pos_status[p] == IPXK_BASIC_FREE ? aB[p] : 0.0;
}
// rhs[p] = (rhs[p]-work[p])/d + aB[p]*d for BASIC, 0 for BASIC_FREE         (:128-138)
__global__ void basis_reduce_rhs_pos_kernel(int m, const int* __restrict__ pos_status, const double* __restrict__ pos_scale,
                                            const double* __restrict__ aB, const double* __restrict__ work,
                                            double* __restrict__ rhs) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < m; p += gridDim.x * blockDim.x) {
        if (pos_status[p] == IPXK_BASIC) {
            const double d = pos_scale[p];
            rhs[p] = (rhs[p] - work[p]) / d + aB[p] * d;
        } else {
            rhs[p] = 0.0;
        }
    }
}
// y[p] = y[p]/d for BASIC, aB[p] for BASIC_FREE                             (:164-174)
__global__ void basis_unscale_y_pos_kernel(int m, const int* __restrict__ pos_status, const double* __restrict__ pos_scale,
                                           const double* __restrict__ aB, double* __restrict__ y) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < m; p += gridDim.x * blockDim.x)
        y[p] = pos_status[p] == IPXK_BASIC ? y[p] / pos_scale[p] : aB[p];
}
// x_B into the entries this rank holds: its own structural columns and every slack column          (:192-193)
__global__ void basis_scatter_x_pos_kernel(int m, const int* __restrict__ loc, const double* __restrict__ work,
                                           double* __restrict__ x) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < m; p += gridDim.x * blockDim.x) {
        const int l = loc[p];
        if (l >= 0) x[l] = work[p];
    }
}

// Column partition: three all-reduces of m (a_B, the right-hand side product, b - N x_N) plus one per CR Apply.
// Structural products are this rank's partials; b and the slack terms enter on rank 0 only.  Every m-vector is then the
// same on all ranks.  Unpartitioned, the all-reduces are no exchanges: each product is written to its destination.
CrResult kkt_basis_solve_dev(Context* c, const double* a, const double* b, double tol, ipxint maxiter,
                             double* x, double* y, ipxk_interrupt_fn interrupt, void* user, ipxk_times* times) {
    SplitOperator* S = c->split;
    const int m = S->m, n = (int)c->n;
    hipStream_t s = c->stream;
    const int g = vec_grid(m);
    const double* W = S->Wsplit.get();
    double* rhs = S->w2.get();
    double* work = S->w1.get();     // note: split_apply_dev uses w0/w1 only inside the CR loop
    if (c->v_lhs.size() < (size_t)std::max(m, 1)) c->v_lhs.resize(std::max(m, 1));
    if (c->v_rhs.size() < (size_t)std::max(m, 1)) c->v_rhs.resize(std::max(m, 1));
    double* lhs = c->v_lhs.get();
    double* crrhs = c->v_rhs.get();
    const bool lead = c->rank == 0;
    const double* zeros = S->zeros.get();
    double* aB = S->aB.get();

    // a_B[p] = a[basis[p]]: the owners' entries, then the slack positions
    allreduce_product(c, aB, (size_t)m, [&](double* out) {
        hipLaunchKernelGGL(pos_contrib_kernel, dim3(g), dim3(kBlock), 0, s, m, n, S->loc_map(), a, out);
    });
    hipLaunchKernelGGL(pos_slack_kernel, dim3(g), dim3(kBlock), 0, s, m, n, S->loc_map(), a, aB);
    // :87-99
    if (S->num_free > 0) {
        hipLaunchKernelGGL(basis_free_rhs_pos_kernel, dim3(g), dim3(kBlock), 0, s, m, S->pos_status.get(), (const double*)aB,
                           S->tI.get());
        solve_dense_dev(c, S->tI.get(), work, 'T');
    }
    const double* wk = S->num_free > 0 ? work : nullptr;
    // :101-121  rhs = sum over nonbasic j of AI[:,j] * d2_j*(a_j - AI[:,j]'work): this rank's columns, slacks on rank 0
    if (wk) {
        EpiBasisColumns ec{{}, W, a, c->tcols.get()};
        launch_spmv(c->Acols, wk, ec, nullptr, nullptr, s);
    } else {
        // no free variables: alpha_j = d2_j * a_j
        hipLaunchKernelGGL(basis_slack_kernel, dim3(vec_grid(n)), dim3(kBlock), 0, s, n, W, a,
                           (const double*)nullptr, c->tcols.get());
    }
    hipLaunchKernelGGL(basis_slack_kernel, dim3(g), dim3(kBlock), 0, s, m, W + n, a + n, wk, S->tI.get());
    allreduce_product(c, rhs, (size_t)m, [&](double* out) {
        EpiBasisRhs er{{}, lead ? S->tI.get() : zeros, out};
        launch_spmv(c->Arows, c->tcols.get(), er, nullptr, nullptr, s);
    });
    solve_dense_dev(c, rhs, rhs, 'N');
    // :124
    solve_dense_dev(c, b, work, 'N');
    // :128-138
    hipLaunchKernelGGL(basis_reduce_rhs_pos_kernel, dim3(g), dim3(kBlock), 0, s, m, S->pos_status.get(), S->pos_scale.get(),
                       (const double*)aB, work, rhs);
    // :141-157
    gather_perm(c, rhs, S->colperm.get(), crrhs, nullptr);
    IPXK_HIP(hipMemsetAsync(lhs, 0, sizeof(double) * m, s));
    CrResult res = cr_solve_dev(c, crrhs, tol, nullptr, maxiter, lhs, true, interrupt, user, nullptr, 0, times);
    // :160-175
    scatter_perm(c, lhs, S->colperm.get(), y, nullptr);
    hipLaunchKernelGGL(basis_unscale_y_pos_kernel, dim3(g), dim3(kBlock), 0, s, m, S->pos_status.get(), S->pos_scale.get(),
                       (const double*)aB, y);
    solve_dense_dev(c, y, y, 'T');
    // :178-188  x[nonbasic] of this rank's columns and of the slacks, work = b - N*x[nonbasic] summed over the ranks
    {
        EpiBasisColumns ec{{}, W, a, x};
        launch_spmv(c->Acols, y, ec, nullptr, nullptr, s);
        hipLaunchKernelGGL(basis_slack_kernel, dim3(g), dim3(kBlock), 0, s, m, W + n, a + n, (const double*)y,
                           x + n);
        allreduce_product(c, work, (size_t)m, [&](double* out) {
            EpiBasisResidual er{{}, lead ? b : zeros, lead ? x + n : zeros, out};
            launch_spmv(c->Arows, x, er, nullptr, nullptr, s);
        });
    }
    // :191-193
    solve_dense_dev(c, work, work, 'N');
    hipLaunchKernelGGL(basis_scatter_x_pos_kernel, dim3(g), dim3(kBlock), 0, s, m, S->loc_map(), work, x);
    IPXK_HIP(hipGetLastError());
    return res;
}

}  // namespace ipxk
