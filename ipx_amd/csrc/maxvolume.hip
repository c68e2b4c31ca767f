// Maxvolume on the device: Maxvolume::RunHeuristic with its Driver, ScaleFtran and
// FindLargest (reference src/maxvolume.cc:108-153, 179-337) and the part of ipx::Basis they drive -- SolveDense,
// SolveForUpdate, TableauRow, ExchangeIfStable (src/basis.cc:162-330) -- on the basis whose LU factors are
// resident (ipxk_lu_factorize_basis + ipxk_split_prepare_lu).
//
// What an exchange step costs on the CPU is a handful of sparse solves; here every piece is a data-parallel pass
// over vectors that stay in HBM, and the host only reads a block of scalars twice per step to take the
// reference's decisions:
//   * FindLargest: arg max |colweights| over the n+m columns (fixed-tree reduction, first index on ties);
//   * tableau column (FTRAN): the entering column scattered into an m-vector, the two forward sweeps on the
//     unscaled factors (trisolve.hip), then the update etas;
//   * ScaleFtran + the recomputed column weight: one fused reduction over the m positions;
//   * tableau row: e_p through the etas (transposed, last first), the two backward sweeps, then one gather
//     product A' btran masked to the NONBASIC columns (the SpMV of the KKT path; slack columns elementwise);
//   * the update of colweights / colscale / invscale_basic: one elementwise pass.
// The factorization is NOT updated in place: every exchange appends a product-form eta behind the factors of the last refactorized
// basis, and an exchange that fails the stability test (pivot from the row against pivot from the column, relative 1e-8 -- the role
// of kFtDiagErrorTol in the reference's Forrest-Tomlin update, src/ipx_internal.h:37) or fills the eta file has the basis
// refactorized on the device (lu.hip).  That part -- FTRAN, BTRAN, the eta file, Basis::Factorize and Basis::ExchangeIfStable -- is
// DeviceBasis (basis.hip), shared with the starting basis; here are the two drivers with their pivot searches, their weight updates
// and their exchange kernels.
// Any exact update represents the same matrix, so the decisions are the reference's up to rounding; the CPU
// restatement the tests compare with keeps the same etas.
#include <hip/hip_runtime.h>
#include <exception>

#include <algorithm>
#include <cmath>
#include <vector>

#include "context.hpp"
#include "spmv_kernels.hpp"
#include "trisolve.hpp"

namespace ipxk {

namespace {

constexpr int kRedGrid = 512;            // workgroups of the two-stage reductions
constexpr double kPivotZeroTol = 1e-7;   // src/maxvolume.h:34


using Scalars = MvScalars;     // the scalars of one step (internal.hpp)
using Part = MvPart;

// ---- FindLargest (src/maxvolume.cc:179-200): first index of the largest |w| ----------------------------------
__global__ __launch_bounds__(kBlock) void mv_argmax_kernel(int64_t N, const double* __restrict__ w, Part* part) {
    double best = 0.0;
    int bi = INT_MAX;
    IPXK_GRID_STRIDE(j, N) {
        const double a = fabs(w[j]);
        if (a > best || (a == best && a > 0.0 && (int)j < bi)) { best = a; bi = (int)j; }
    }
    block_argmax<kBlock>(best, bi);
    if (threadIdx.x == 0) {
        part[blockIdx.x].v[0] = best;
        part[blockIdx.x].i[0] = bi;
    }
}
// one workgroup of kRedGrid threads: thread k holds partial k
__global__ __launch_bounds__(kRedGrid) void mv_argmax_final_kernel(int nparts, const Part* part, const double* __restrict__ w, Scalars* S) {
    double best = (int)threadIdx.x < nparts ? part[threadIdx.x].v[0] : 0.0;
    int bi = (int)threadIdx.x < nparts ? part[threadIdx.x].i[0] : INT_MAX;
    block_argmax<kRedGrid>(best, bi);
    if (threadIdx.x == 0) {
        S->jn = bi == INT_MAX ? 0 : bi;             // all weights zero: index 0, weight 0 (the loop ends)
        S->weight = w[S->jn];
    }
}


// ---- ScaleFtran (src/maxvolume.cc:322-337) + the recomputed weight (:269-275) + # nonzeros of the column ----
__global__ __launch_bounds__(kBlock) void mv_scale_ftran_kernel(int m, const Scalars* S, const double* __restrict__ lhs,
                                                                const double* __restrict__ colscale, const double* __restrict__ invscale,
                                                                const int* __restrict__ slice_of, int slice, Part* part) {
    const double dj = colscale[S->jn];
    double best = 0.0, sum = 0.0;
    int bi = INT_MAX, cnt = 0;
    IPXK_GRID_STRIDE(p, m) {
        const double pivot = lhs[p];
        const double scaled = pivot * dj * invscale[p];
        const double v = fabs(scaled);
        if (fabs(pivot) > kPivotZeroTol && (v > best || (v == best && v > 0.0 && (int)p < bi))) { best = v; bi = (int)p; }
        if (slice_of[p] == slice) sum += scaled;
        cnt += pivot != 0.0;
    }
    const Part mine = block_partial<kBlock>(Part{{best}, {bi}, sum, cnt});
    if (threadIdx.x == 0) part[blockIdx.x] = mine;
}
__global__ __launch_bounds__(kRedGrid) void mv_scale_ftran_final_kernel(int nparts, const Part* part, const double* __restrict__ lhs,
                                            const double* __restrict__ colscale, const double* __restrict__ invscale,
                                            const int* __restrict__ slice_of, int slice, const ipxint* __restrict__ basis, Scalars* S) {
    const Part all = block_partial<kRedGrid>(load_partial(nparts, part));
    if (threadIdx.x != 0) return;
    const int pmax = all.i[0] == INT_MAX ? 0 : all.i[0];        // no entry qualified: position 0 (:325, :255-256)
    const double dj = colscale[S->jn];
    S->pmax = pmax;
    S->jb = (int)basis[pmax];
    S->vmax = fabs(lhs[pmax] * dj * invscale[pmax]);
    S->weight_recomp = all.s;
    S->colscale_jn = dj;
    S->invscale_pmax = invscale[pmax];
    S->pivot_col = lhs[pmax];
    S->used_pmax = slice_of[pmax] == slice ? 1 : 0;
    S->eta_nnz = all.c;
}
// skipped column (:259-266)
__global__ void mv_skip_kernel(const Scalars* S, double* colweights, double* colscale) {
    colweights[S->jn] = 0.0;
    colscale[S->jn] = 0.0;
}
// ---- tableau row ----------------------------------------------------------------------------------------------
__global__ void mv_row_slack_kernel(int m, int n, const double* __restrict__ btran, const double* __restrict__ mask,
                                    double* __restrict__ row) {
    IPXK_GRID_STRIDE(i, m) row[n + i] = mask[n + i] != 0.0 ? btran[i] : 0.0;
}
__global__ void mv_read_pivot_kernel(const double* __restrict__ row, Scalars* S) { S->pivot_row = row[S->jn]; }
// ---- exchange ---------------------------------------------------------------------------------------------------
// colweights update (:307-314); colscale / invscale_basic / basis / the NONBASIC mask by the kernel that follows
__global__ void mv_weights_kernel(int64_t N, const Scalars* S, double alpha, const double* __restrict__ row,
                                  const double* __restrict__ colscale, double* __restrict__ colweights) {
    const int jn = S->jn, jb = S->jb;
    const double wjb = (double)S->used_pmax + alpha / S->invscale_pmax;
    IPXK_GRID_STRIDE(j, N) {
        if ((int)j == jb) colweights[j] = wjb;
        else if ((int)j == jn) colweights[j] = 0.0;
        else colweights[j] += alpha * row[j] * colscale[j];
    }
}
__global__ void mv_exchange_kernel(const Scalars* S, ipxint* basis, int* map2basis, double* colscale, double* invscale, double* mask) {
    const int jn = S->jn, jb = S->jb, p = S->pmax;
    colscale[jb] = 1.0 / S->invscale_pmax;          // :301-303
    invscale[p] = 1.0 / S->colscale_jn;
    colscale[jn] = 0.0;
    basis[p] = jn;                                  // Basis::ExchangeIfStable :308-313
    map2basis[jn] = p;
    map2basis[jb] = -1;
    mask[jn] = 0.0;
    mask[jb] = 1.0;
}
// ---- Maxvolume::RunSequential (src/maxvolume.cc:14-106) ---------------------------------------------------------
// the candidate chosen by the host's pass order
__global__ void mvs_set_candidate_kernel(int j, double dj, Scalars* S) { S->jn = j; S->colscale_jn = dj; S->weight = dj; }
// search_pivot (:61-70): first position of the largest v = |x_p| * invscale_basic[p] * d_j; # nonzeros and sum of
// squares of the scaled column (tblnnz, frobnorm_squared)
__global__ __launch_bounds__(kBlock) void mvs_search_pivot_kernel(int m, const Scalars* S, const double* __restrict__ lhs,
                                                                  const double* __restrict__ invscale, Part* part) {
    const double dj = S->colscale_jn;
    double best = 0.0, sum = 0.0;
    int bi = INT_MAX, cnt = 0;
    IPXK_GRID_STRIDE(p, m) {
        const double v = fabs(lhs[p]) * invscale[p] * dj;
        if (v > best || (v == best && v > 0.0 && (int)p < bi)) { best = v; bi = (int)p; }
        sum += v * v;
        cnt += v != 0.0;
    }
    const Part mine = block_partial<kBlock>(Part{{best}, {bi}, sum, cnt});
    if (threadIdx.x == 0) part[blockIdx.x] = mine;
}
__global__ __launch_bounds__(kRedGrid) void mvs_search_pivot_final_kernel(int nparts, const Part* part, const double* __restrict__ lhs,
                                                                          const double* __restrict__ invscale, const ipxint* __restrict__ basis,
                                                                          Scalars* S) {
    const Part all = block_partial<kRedGrid>(load_partial(nparts, part));
    if (threadIdx.x != 0) return;
    const int pmax = all.i[0] == INT_MAX ? -1 : all.i[0];
    S->pmax = pmax;
    S->vmax = all.v[0];
    S->weight_recomp = all.s;                            // sum of squares of the scaled column
    S->eta_nnz = all.c;                                  // # nonzeros of the column (its eta has one fewer)
    S->jb = pmax >= 0 ? (int)basis[pmax] : -1;
    S->pivot_col = pmax >= 0 ? lhs[pmax] : 0.0;
    S->invscale_pmax = pmax >= 0 ? invscale[pmax] : 0.0;
    S->used_pmax = 0;
}
__global__ void mvs_exchange_kernel(const Scalars* S, ipxint* basis, int* map2basis, double* invscale) {
    const int jn = S->jn, jb = S->jb, p = S->pmax;
    invscale[p] = 1.0 / S->colscale_jn;                 // :88
    basis[p] = jn;                                      // Basis::ExchangeIfStable :308-313
    map2basis[jn] = p;
    map2basis[jb] = -1;
}

// ---- set-up -------------------------------------------------------------------------------------------------------
__global__ void mv_init_columns_kernel(int64_t N, const ipxint* __restrict__ status, const double* __restrict__ colscale_in,
                                       double* __restrict__ colscale, double* __restrict__ mask, int* __restrict__ map2basis) {
    IPXK_GRID_STRIDE(j, N) {
        const ipxint st = status[j];
        colscale[j] = st == IPXK_NONBASIC ? colscale_in[j] : 0.0;        // :130-133
        mask[j] = st == IPXK_NONBASIC ? 1.0 : 0.0;                       // TableauRow with ignore_fixed
        map2basis[j] = st == IPXK_NONBASIC_FIXED ? -2 : -1;              // basic ones by mv_init_basis_kernel
    }
}
__global__ void mv_init_basis_kernel(int m, const ipxint* __restrict__ basis, const ipxint* __restrict__ status,
                                     const double* __restrict__ colscale_in, double* __restrict__ invscale, int* __restrict__ map2basis) {
    IPXK_GRID_STRIDE(p, m) {
        const ipxint j = basis[p];
        invscale[p] = status[j] == IPXK_BASIC ? 1.0 / colscale_in[j] : 0.0;   // :120-126 (BASIC_FREE: 0, never leaves)
        map2basis[j] = status[j] == IPXK_BASIC_FREE ? (int)p + m : (int)p;
    }
}
__global__ void mv_slice_work_kernel(int m, const double* __restrict__ invscale, const int* __restrict__ slice_of, int slice,
                                     double* __restrict__ work) {
    IPXK_GRID_STRIDE(p, m) work[p] = slice_of[p] == slice ? invscale[p] : 0.0;     // :221-223
}
__global__ void mv_weights_slack_kernel(int m, int n, const double* __restrict__ work, const double* __restrict__ colscale,
                                        double* __restrict__ colweights) {
    IPXK_GRID_STRIDE(i, m) colweights[n + i] = colscale[n + i] != 0.0 ? work[i] * colscale[n + i] : 0.0;
}

// an eta file this call cannot take over: a fresh factorization of the basis it stands for first
void factorize_behind_etas(Context* c, const ipxint* status, const double* colscale) {
    maxvol_drop_etas(c);
    ipxk_lu_info li{};
    lu_factorize_basis(c, c->maxvol->basis_h.data(), c->maxvol_pivottol, false, &li);
    IPXK_REQUIRE(li.num_dependent == 0, "the basis behind the eta file is singular");
    split_prepare_lu(c, status, colscale);
}

// The set-up of both variants: the host mirrors of basis and status, the device copies, colscale / the NONBASIC mask / map2basis by
// column and invscale_basic by position (downloaded where the caller asks).  A call that goes on with an eta file has its basis already.
void set_up(DeviceBasis& B, const LuView& V, const ipxint* status_in, const double* colscale_in, bool resumed, double* invscale_h) {
    Context* c = B.c;
    MaxvolState& M = B.M;
    const int m = B.m;
    const int64_t N = c->n + (int64_t)m;
    hipStream_t s = c->stream;
    if (!M.h) IPXK_HIP(hipHostMalloc(reinterpret_cast<void**>(&M.h), sizeof(Scalars)));
    B.status_h.assign(status_in, status_in + N);
    if (resumed) B.basis_h = M.basis_h;
    else IPXK_HIP(hipMemcpyAsync(B.basis_h.data(), V.basis, (size_t)m * sizeof(ipxint), hipMemcpyDeviceToHost, s));
    DevBuf<double> colscale_dev;
    colscale_dev.upload(colscale_in, (size_t)N, s);
    M.status.upload(status_in, (size_t)N, s);
    M.basis.ensure((size_t)m);
    if (!resumed) IPXK_HIP(hipMemcpyAsync(M.basis.get(), V.basis, (size_t)m * sizeof(ipxint), hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(mv_init_columns_kernel, dim3(grid_for(N)), dim3(kBlock), 0, s, N, M.status.get(), colscale_dev.get(),
                       M.colscale.get(), M.mask.get(), M.map2basis.get());
    hipLaunchKernelGGL(mv_init_basis_kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, m, M.basis.get(), M.status.get(), colscale_dev.get(),
                       M.invscale.get(), M.map2basis.get());
    if (invscale_h) M.invscale.download(invscale_h, (size_t)m, s);
    IPXK_HIP(hipStreamSynchronize(s));
    for (int p = 0; p < m; p++)
        IPXK_REQUIRE(B.basis_h[p] >= 0 && B.basis_h[p] < N && B.status_h[B.basis_h[p]] >= 0, "status of a basic variable is not BASIC / BASIC_FREE");
    const int *Ap = nullptr, *Ai = nullptr;
    const double* Ax = nullptr;
    lu_plain_matrix(c, &Ap, &Ai, &Ax);       // (its check: the resident copy of the matrix that FTRAN and the pivot from the row read)
}

}  // namespace

void destroy_maxvol(MaxvolState* M) { delete M; }


void maxvolume_dev(Context* c, const ipxint* status_in, const double* colscale_in, const ipxk_maxvolume_params* prm_in,
                   ipxint* basis_out, ipxint* status_out, ipxk_maxvolume_info* info, ipxint* log, ipxint log_cap) {
    const ipxk_maxvolume_params defaults{2.0, 10, 10000, 100};       // include/ipx_parameters.h:69-71
    const ipxk_maxvolume_params* prm = prm_in ? prm_in : &defaults;
    LuView V;
    IPXK_REQUIRE(lu_view(c, &V) && V.from_basis && V.ndep == 0, "maxvolume needs the factorization of the current basis (ipxk_lu_factorize_basis)");
    IPXK_REQUIRE(c->split, "maxvolume needs the operator of the current basis (ipxk_split_prepare_lu)");
    const int m = (int)c->m, n = (int)c->n;
    const int64_t N = (int64_t)n + m;
    IPXK_REQUIRE(m > 0, "empty model");
    hipStream_t s = c->stream;
    if (!c->maxvol) c->maxvol = new MaxvolState;
    MaxvolState& M = *c->maxvol;
    const double t_start = now_s();
    const double volumetol = std::max(prm->volume_tol, 1.0);
    for (DevBuf<double>* b : {&M.colscale, &M.colweights, &M.row, &M.mask}) b->ensure((size_t)N);
    for (DevBuf<double>* b : {&M.invscale, &M.work}) b->ensure((size_t)m);
    M.map2basis.ensure((size_t)N); M.slice_of.ensure((size_t)m);
    M.part.ensure(kRedGrid); M.scalars.ensure(1);
    // the etas of the previous call may still stand behind the factors (see maxvol_apply_etas): this call goes on with them, and while it
    // runs it applies them itself -- the solves of trisolve.hip must not
    const bool resume = c->etas_live && M.saved.live && (int64_t)M.basis_h.size() == (int64_t)m && M.saved.lu_generation == lu_generation(c);
    DeviceBasis B(c, M, prm->max_etas, resume, colscale_in, M.scalars.get());
    EtaFile& etas = B.etas;
    const bool resumed = etas.resumed;
    if (c->etas_live && !resumed) {              // (other parameters)
        IPXK_REQUIRE((int64_t)M.basis_h.size() == (int64_t)m, "eta file without its basis");
        factorize_behind_etas(c, status_in, colscale_in);
        IPXK_REQUIRE(lu_view(c, &V), "no factorization");
    }
    c->etas_live = false;
    M.saved.live = false;
    // (a call that went on with an eta file and ends by an exception leaves an operator without the etas it needs: it goes, so that what
    // follows fails loudly -- "SplittedNormalMatrix not prepared" -- instead of solving with the wrong basis)
    struct ResumeGuard {
        Context* c; bool armed;
        ~ResumeGuard() { if (armed && std::uncaught_exceptions() > 0 && c->split) { destroy_split(c->split); c->split = nullptr; } }
    } resume_guard{c, resumed};
    if (!resumed) etas.reset(V.bump_size);
    std::vector<double> inv_h((size_t)m);
    set_up(B, V, status_in, colscale_in, resumed, inv_h.data());
    // slices: Sortperm of invscale_basic ascending (value, index), row perm[i] belongs to slice i % num_slices (:138-142)
    int num_slices = (int)std::min<int64_t>(m, 5 + std::max<int64_t>(m / std::max<ipxint>(prm->rows_per_slice, 1), 0));
    {
        std::vector<std::pair<double, int>> vi((size_t)m);
        for (int p = 0; p < m; p++) vi[p] = std::make_pair(inv_h[p], p);
        std::sort(vi.begin(), vi.end());
        std::vector<int> slice_of((size_t)m);
        for (int i = 0; i < m; i++) slice_of[vi[i].second] = i % num_slices;
        M.slice_of.upload(slice_of, s);
    }
    IPXK_HIP(hipStreamSynchronize(s));

    ipxk_maxvolume_info I{};
    I.slices = num_slices;
    const int gm = grid_for(m), gN = grid_for(N);
    const bool verbose = getenv("IPXK_VERBOSE") != nullptr && getenv("IPXK_VERBOSE")[0] == '2';

    for (int slice = 0; slice < num_slices; slice++) {
        // ---- Driver: column weights of the slice (:221-232)
        hipLaunchKernelGGL(mv_slice_work_kernel, dim3(gm), dim3(kBlock), 0, s, m, M.invscale.get(), M.slice_of.get(), slice, B.unit);
        etas.apply(true, B.unit);
        solve_dense_dev(c, B.unit, M.work.get(), 'T');
        {
            EpiScale e{{}, M.colscale.get(), M.colweights.get()};
            launch_spmv(c->Acols, M.work.get(), e, nullptr, nullptr, s);
            hipLaunchKernelGGL(mv_weights_slack_kernel, dim3(gm), dim3(kBlock), 0, s, m, n, M.work.get(), M.colscale.get(), M.colweights.get());
        }
        int64_t skipped = 0;
        while (true) {
            // FindLargest, tableau column, ScaleFtran
            hipLaunchKernelGGL(mv_argmax_kernel, dim3(kRedGrid), dim3(kBlock), 0, s, N, M.colweights.get(), M.part.get());
            hipLaunchKernelGGL(mv_argmax_final_kernel, dim3(1), dim3(kRedGrid), 0, s, kRedGrid, M.part.get(), M.colweights.get(), M.scalars.get());
            B.ftran();
            hipLaunchKernelGGL(mv_scale_ftran_kernel, dim3(kRedGrid), dim3(kBlock), 0, s, m, M.scalars.get(), B.lhs, M.colscale.get(),
                               M.invscale.get(), M.slice_of.get(), slice, M.part.get());
            hipLaunchKernelGGL(mv_scale_ftran_final_kernel, dim3(1), dim3(kRedGrid), 0, s, kRedGrid, M.part.get(), B.lhs, M.colscale.get(),
                               M.invscale.get(), M.slice_of.get(), slice, M.basis.get(), M.scalars.get());
            Scalars a = read_scalars(M.scalars.get(), M.h, s);
            if (verbose)
                fprintf(stderr, "ipxk: maxvolume slice %d: jn %d weight %.3e pmax %d jb %d vmax %.3e (etas %d, updates %lld, skipped %lld)\n", slice,
                        a.jn, a.weight, a.pmax, a.jb, a.vmax, etas.K, (long long)I.updates, (long long)skipped);
            if (a.weight == 0.0) break;                                             // :243-244
            if (c->interrupt && (B.errflag = c->interrupt(c->interrupt_user)) != 0) break;   // :250-251
            if (a.vmax <= volumetol) {                                              // :259-266
                hipLaunchKernelGGL(mv_skip_kernel, dim3(1), dim3(1), 0, s, M.scalars.get(), M.colweights.get(), M.colscale.get());
                if (++skipped > prm->maxskip_updates && prm->maxskip_updates >= 0) break;
                continue;
            }
            // tableau row of the leaving variable (:278-280)
            B.btran_unit();
            {
                EpiScale e{{}, M.mask.get(), M.row.get()};
                launch_spmv(c->Acols, B.btran, e, nullptr, nullptr, s);
                hipLaunchKernelGGL(mv_row_slack_kernel, dim3(gm), dim3(kBlock), 0, s, m, n, B.btran, M.mask.get(), M.row.get());
            }
            hipLaunchKernelGGL(mv_read_pivot_kernel, dim3(1), dim3(1), 0, s, M.row.get(), M.scalars.get());
            a.pivot_row = read_scalars(M.scalars.get(), M.h, s).pivot_row;
            if (!B.exchange_if_stable(a)) {
                if (B.errflag) break;
                continue;
            }
            const double alpha = ((double)a.used_pmax - a.weight_recomp) / (a.colscale_jn * a.pivot_row);      // :307
            hipLaunchKernelGGL(mv_weights_kernel, dim3(gN), dim3(kBlock), 0, s, N, M.scalars.get(), alpha, M.row.get(), M.colscale.get(),
                               M.colweights.get());
            hipLaunchKernelGGL(mv_exchange_kernel, dim3(1), dim3(1), 0, s, M.scalars.get(), M.basis.get(), M.map2basis.get(), M.colscale.get(),
                               M.invscale.get(), M.mask.get());
            if (log && I.updates < log_cap) { log[2 * I.updates] = a.jb; log[2 * I.updates + 1] = a.jn; }
            I.updates++;
            I.volinc += std::log2(a.vmax);                                          // :294
            B.commit(a);
            if (B.errflag) break;
        }
        I.skipped += skipped;
        if (B.errflag) break;
    }
    IPXK_HIP(hipStreamSynchronize(s));
    check_sweep_abort(c);
    // the tail of KKTSolverBasis::_Factorize (src/kkt_solver_basis.cc:56-61): a fresh factorization of the final
    // basis and the operator built from it
    // (IPXK_MAXVOL_SKIP_FINAL=1, measurements only: leaves the context with the factors of the last refactorized basis)
    // ... unless carrying the etas through the solves that follow is cheaper (EtaFile::worth_keeping; IPXK_MAXVOL_KEEP_ETAS=0: never,
    // =1: whenever the file is not full): the operator then only learns the new basis and its scaling
    // (a run that ends with an error flag keeps them too: factors + etas stay a consistent operator of the basis reported)
    if (etas.K > 0 && !getenv("IPXK_MAXVOL_SKIP_FINAL")) {
        const char* keep_env = getenv("IPXK_MAXVOL_KEEP_ETAS");
        const bool keep = B.errflag != 0 || (keep_env ? (keep_env[0] == '1' && !etas.full()) : etas.worth_keeping());
        if (keep) {
            etas.save();
            M.basis_h = B.basis_h;
            c->etas_live = true;
            split_follow_basis(c, M.basis.get(), B.status_h.data(), colscale_in);
            I.kept_etas = etas.K;
        } else {
            (void)B.refactorize();
        }
    }
    IPXK_HIP(hipStreamSynchronize(s));
    I.errflag = B.errflag;
    I.refused = B.refused;
    I.factorizations = B.factorizations - B.singular;
    I.seconds = now_s() - t_start;
    if (basis_out) std::copy(B.basis_h.begin(), B.basis_h.end(), basis_out);
    if (status_out) std::copy(B.status_h.begin(), B.status_h.end(), status_out);
    if (info) *info = I;
}

// Maxvolume::RunSequential on the device (update_heuristic == 0, src/kkt_solver_basis.cc:47-51): every NONBASIC column in
// decreasing order of its scaling factor gets its tableau column (the forward sweep pair + the etas), the host reads
// one block of scalars per candidate and takes the reference's decisions.  The reference does this with hypersparse
// solves; here a candidate costs two sweeps over all m unknowns, so the sequential variant is for moderate sizes --
// the heuristic (maxvolume_dev) is the one built for 1M rows.
void maxvolume_sequential_dev(Context* c, const ipxint* status_in, const double* colscale_in, double volume_tol, ipxint maxpasses,
                              ipxint max_etas_in, ipxint* basis_out, ipxint* status_out, ipxk_maxvolume_info* info, ipxint* log,
                              ipxint log_cap) {
    LuView V;
    // (the sequential variant starts from fresh factors: the basis behind an eta file of the other variant is factorized first)
    if (c->etas_live && c->maxvol && (int64_t)c->maxvol->basis_h.size() == c->m) factorize_behind_etas(c, status_in, colscale_in);
    IPXK_REQUIRE(lu_view(c, &V) && V.from_basis && V.ndep == 0, "maxvolume needs the factorization of the current basis (ipxk_lu_factorize_basis)");
    IPXK_REQUIRE(c->split, "maxvolume needs the operator of the current basis (ipxk_split_prepare_lu)");
    const int m = (int)c->m, n = (int)c->n;
    const int64_t N = (int64_t)n + m;
    IPXK_REQUIRE(m > 0, "empty model");
    hipStream_t s = c->stream;
    if (!c->maxvol) c->maxvol = new MaxvolState;
    MaxvolState& M = *c->maxvol;
    const double t_start = now_s();
    const double volumetol = std::max(volume_tol, 1.0);
    M.invscale.ensure((size_t)m);
    M.map2basis.ensure((size_t)N);
    M.part.ensure(kRedGrid); M.scalars.ensure(1);
    DeviceBasis B(c, M, max_etas_in, false, colscale_in, M.scalars.get());
    EtaFile& etas = B.etas;
    etas.reset(V.bump_size);
    M.colscale.ensure((size_t)N); M.mask.ensure((size_t)N);
    set_up(B, V, status_in, colscale_in, false, nullptr);
    ipxk_maxvolume_info I{};
    ipxint passes = 0;
    // candidates of a pass: Sortperm(n+m, colscale, false) (src/utils.cc:87-104), taken from the back
    std::vector<std::pair<double, ipxint>> cand;
    while ((passes < maxpasses || maxpasses < 0) && !B.errflag) {
        ipxint updates_last = 0;
        cand.resize((size_t)N);
        for (int64_t j = 0; j < N; j++) cand[(size_t)j] = std::make_pair(colscale_in[j], (ipxint)j);
        std::sort(cand.begin(), cand.end());
        while (!cand.empty()) {
            const ipxint j = cand.back().second;
            const double dj = cand.back().first;
            if (dj == 0.0) break;
            if (B.status_h[(size_t)j] != IPXK_NONBASIC) { cand.pop_back(); continue; }
            if (c->interrupt && (B.errflag = c->interrupt(c->interrupt_user)) != 0) break;   // :52-53
            // tableau column and search_pivot
            hipLaunchKernelGGL(mvs_set_candidate_kernel, dim3(1), dim3(1), 0, s, (int)j, dj, M.scalars.get());
            B.ftran();
            hipLaunchKernelGGL(mvs_search_pivot_kernel, dim3(kRedGrid), dim3(kBlock), 0, s, m, M.scalars.get(), B.lhs, M.invscale.get(),
                               M.part.get());
            hipLaunchKernelGGL(mvs_search_pivot_final_kernel, dim3(1), dim3(kRedGrid), 0, s, kRedGrid, M.part.get(), B.lhs,
                               M.invscale.get(), M.basis.get(), M.scalars.get());
            Scalars a = read_scalars(M.scalars.get(), M.h, s);
            if (a.vmax <= volumetol || a.pmax < 0) { I.skipped++; cand.pop_back(); continue; }      // :72-76
            // the BTRAN of the leaving variable (ExchangeIfStable with sys = -1, src/basis.cc:292-293): pivot from the row
            B.btran_unit();
            mv_pivot_from_row(c, B.btran, M.scalars.get());
            a.pivot_row = read_scalars(M.scalars.get(), M.h, s).pivot_row;
            if (!B.exchange_if_stable(a)) {
                if (B.errflag) break;
                continue;                                                           // "try again" (:86-87)
            }
            hipLaunchKernelGGL(mvs_exchange_kernel, dim3(1), dim3(1), 0, s, M.scalars.get(), M.basis.get(), M.map2basis.get(), M.invscale.get());
            if (log && I.updates + updates_last < log_cap) { log[2 * (I.updates + updates_last)] = a.jb; log[2 * (I.updates + updates_last) + 1] = j; }
            updates_last++;
            I.volinc += std::log2(a.vmax);                                          // :90
            cand.pop_back();
            B.commit(a);                                                            // (a.jn == j)
            if (B.errflag) break;
        }
        I.updates += updates_last;
        passes++;
        if (updates_last == 0) break;
    }
    IPXK_HIP(hipStreamSynchronize(s));
    check_sweep_abort(c);
    if (etas.K > 0 && !B.errflag) (void)B.refactorize();      // the tail of KKTSolverBasis::_Factorize (src/kkt_solver_basis.cc:56-61)
    IPXK_HIP(hipStreamSynchronize(s));
    I.slices = passes;                                 // (the field reports the passes for this variant)
    I.errflag = B.errflag;
    I.refused = B.refused;
    I.factorizations = B.factorizations - B.singular;
    I.seconds = now_s() - t_start;
    if (basis_out) std::copy(B.basis_h.begin(), B.basis_h.end(), basis_out);
    if (status_out) std::copy(B.status_h.begin(), B.status_h.end(), status_out);
    if (info) *info = I;
}

}  // namespace ipxk
