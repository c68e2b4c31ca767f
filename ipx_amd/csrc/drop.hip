// DropPrimal / DropDual on the device: reference src/kkt_solver_basis.cc:36-43 and :196-387.
// Before Maxvolume, KKTSolverBasis::_Factorize takes nearly degenerate variables out of the barrier problem: a basic variable
// that sits on a bound is pivoted out of the basis if that increases the volume, else it becomes implied at the bound
// (Iterate::make_implied_lb / _ub, basic free); a nonbasic variable whose dual is nearly zero is pivoted in, else fixed at its
// value (Iterate::make_fixed, nonbasic fixed).
//
// The basis is DeviceBasis (basis.hip), as for Maxvolume and the starting basis.  What is here:
//   * the two screenings: a flag per basis position / per variable, an exclusive scan, the candidates stored in ascending order
//     (no atomics: the list does not depend on the order the threads run in); the host reads the count, and the list only when
//     the count is positive;
//   * drop_row_kernel: DropPrimal's pivot search.  One gather pass over the plain CSC of AI, eight lanes per column, forms
//     r_j = a_j' btran for the NONBASIC columns (Basis::TableauRow with ignore_fixed) and folds |r_j| colscale_j invscale_p into a
//     two-stage indexed arg max under the two thresholds -- the row is never stored, the winner's r_j travels with its partial;
//   * drop_column_kernel: DropDual's search over the positions of the tableau column, and the column's number of nonzeros;
//   * the one-workgroup kernels that finish the reductions take the decision and, where there is no pivot, change the iterate,
//     the status and the scaling factors themselves: everything a candidate needs is enqueued without a host round trip and ONE
//     block of scalars per candidate reaches the host, which keeps the mirrors, the eta file and the refactorizations.
// Every reduction is a fixed-order tree over block partials and ties go to the lowest index (the reference's loops take the first
// strictly larger entry): two calls from the same state give the same bits.
// No kernel of this file uses scratch memory (-Rpass-analysis=kernel-resource-usage: ScratchSize 0 throughout).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <memory>
#include <vector>

#include "context.hpp"
#include "trisolve.hpp"

namespace ipxk {

namespace {

constexpr int kDropGrid = 512;           // workgroups of the two-stage reductions = threads of the kernels that finish them
constexpr int kRowLanes = 8;             // lanes per column in drop_row_kernel
constexpr int kRowCols = kBlock / kRowLanes;
constexpr double kPivotZeroTol = 1e-7;   // src/kkt_solver_basis.h
constexpr double kVolumeTol = 2.0;       // volume_tol of DropPrimal / DropDual (:205, :304)

enum DropAction { kExchanged = 0, kImpliedLb = 1, kImpliedUb = 2, kFixed = 3 };

// the scalars of one candidate, written by the device, read by the host
struct DropScalars {
    MvScalars mv;            // jn, pmax, jb, pivot_col, pivot_row, eta_nnz: what DeviceBasis reads and writes
    int winner;              // jmax (DropPrimal) / pmax (DropDual); -1: none
    int action;              // DropAction
    double vmax;             // the winner's scaled pivot
};

using DropPart = Partial<1>;     // (largest value, its smallest index); s carries the winner's r_j out of drop_row_kernel

struct IterateVectors { double *xl, *xu, *zl, *zu; unsigned char* state; };

// ---- screening (:209-226, :308-325) ----------------------------------------------------------------------------------------
__global__ void drop_primal_flag_kernel(int m, const ipxint* __restrict__ basis, const ipxint* __restrict__ status, IterateVectors V,
                                        double drop_primal, int* __restrict__ flag) {
    IPXK_GRID_STRIDE(p, m) {
        const ipxint jb = basis[p];
        int f = 0;
        if (status[jb] == IPXK_BASIC) {                           // (ignore free variables)
            double xj, zj;                                        // the nearer bound
            if (V.xl[jb] <= V.xu[jb]) { xj = V.xl[jb]; zj = V.zl[jb]; } else { xj = V.xu[jb]; zj = V.zu[jb]; }
            f = xj < 0.01 * zj && xj <= drop_primal;
        }
        flag[p] = f;
    }
}
__global__ void drop_dual_flag_kernel(int64_t N, const ipxint* __restrict__ status, IterateVectors V, double drop_dual,
                                      int* __restrict__ flag) {
    IPXK_GRID_STRIDE(j, N) {
        int f = 0;
        if (status[j] == IPXK_NONBASIC) {
            double xj, zj;                                        // the larger dual
            if (V.zl[j] >= V.zu[j]) { xj = V.xl[j]; zj = V.zl[j]; } else { xj = V.xu[j]; zj = V.zu[j]; }
            f = zj < 0.01 * xj && zj <= drop_dual;
        }
        flag[j] = f;
    }
}
// list[rank[i]] = basis[i] (or i itself) for the flagged i; *count = their number
__global__ void drop_store_kernel(int64_t len, const int* __restrict__ flag, const int* __restrict__ rank, const ipxint* __restrict__ basis,
                                  int* __restrict__ list, int* count) {
    IPXK_GRID_STRIDE(i, len) {
        if (flag[i]) list[rank[i]] = basis ? (int)basis[i] : (int)i;
        if (i == len - 1) *count = rank[i] + flag[i];
    }
}

__global__ void drop_set_kernel(int jn, int pmax, int jb, DropScalars* S) { S->mv.jn = jn; S->mv.pmax = pmax; S->mv.jb = jb; }
__global__ void drop_invscale_kernel(int m, const ipxint* __restrict__ basis, const ipxint* __restrict__ status,
                                     const double* __restrict__ colscale, double* __restrict__ invscale) {
    IPXK_GRID_STRIDE(p, m) invscale[p] = status[basis[p]] == IPXK_BASIC ? 1.0 / colscale[basis[p]] : 0.0;   // :233-238 (BASIC_FREE: 0, never leaves)
}

// ---- DropPrimal: the tableau row with the pivot search fused in (:246-259) -----------------------------------------------
// r_j = a_j' btran for the NONBASIC columns (slack columns: btran[j - n]).  Eight lanes share a column: lane l adds the products
// of the column's entries l, l + 8, ... in order, then a fixed tree over the eight.  The matrix is streamed once (12 bytes per
// entry, consecutive lanes on consecutive entries), btran is the only gathered vector (m doubles).  Candidates of the search:
// |r_j| > kPivotZeroTol and v_j = |r_j| colscale_j invscale_p > volume_tol, both strict; largest v_j, lowest j among equals.
__global__ __launch_bounds__(kBlock) void drop_row_kernel(int n, int64_t N, const int* __restrict__ Ap, const int* __restrict__ Ai,
                                                          const double* __restrict__ Ax, const double* __restrict__ btran,
                                                          const ipxint* __restrict__ status, const double* __restrict__ colscale,
                                                          const double* __restrict__ invscale, const DropScalars* S, DropPart* part) {
    __shared__ int s_win;
    __shared__ double s_r;
    const double s = invscale[S->mv.pmax];
    DropPart p = partial_identity<1>();
    double rbest = 0.0;
    const int lane = threadIdx.x & (kRowLanes - 1), sub = threadIdx.x / kRowLanes;
    // (the trip count is the same for every thread of the workgroup: the lane exchanges below run with all lanes active)
    for (int64_t base = (int64_t)blockIdx.x * kRowCols; base < N; base += (int64_t)gridDim.x * kRowCols) {
        const int64_t j = base + sub;
        const bool nonbasic = j < N && status[j] == IPXK_NONBASIC;
        double sum = 0.0;
        if (nonbasic && j < n)
            for (int q = Ap[j] + lane; q < Ap[j + 1]; q += kRowLanes) sum += Ax[q] * btran[Ai[q]];
        sum = wave_sum<kRowLanes>(sum);
        if (lane == 0 && nonbasic) {
            if (j >= n) sum = btran[j - n];
            const double r = fabs(sum);
            if (r > kPivotZeroTol) {
                const double v = r * colscale[j] * s;
                if (v > kVolumeTol && v > p.v[0]) { p.v[0] = v; p.i[0] = (int)j; rbest = sum; }     // (j ascends: the first of equals stays)
            }
        }
    }
    const int mine = p.i[0];
    p = block_partial<kBlock>(p);
    if (threadIdx.x == 0) s_win = p.i[0];
    __syncthreads();
    if (mine != INT_MAX && mine == s_win) s_r = rbest;            // (a column belongs to one thread)
    __syncthreads();
    if (threadIdx.x == 0) {
        p.s = p.i[0] == INT_MAX ? 0.0 : s_r;
        part[blockIdx.x] = p;
    }
}
// the decision (:260-290).  A winner: it enters, its r_j is the pivot from the row.  None: make_implied_lb / _ub (src/iterate.cc:160-172),
// Basis::FreeBasicVariable, invscale_basic[p] = 0, colscale[jb] = inf -- and jb itself as the column of the FTRAN that is enqueued
// either way (a valid column, its result unused).
__global__ __launch_bounds__(kDropGrid) void drop_row_final_kernel(int nparts, const DropPart* part, DropScalars* S, IterateVectors V,
                                                                   ipxint* status, double* colscale, double* invscale) {
    __shared__ int s_win;
    DropPart p = load_partial(nparts, part);
    const int mine = p.i[0];
    const double mine_r = p.s;
    p = block_partial<kDropGrid>(p);
    if (threadIdx.x == 0) { s_win = p.i[0]; S->vmax = p.v[0]; }
    __syncthreads();
    const int win = s_win;
    if (win != INT_MAX) {
        if (mine == win) {                                        // (a column belongs to one workgroup: one partial holds it)
            S->mv.jn = win;
            S->mv.pivot_row = mine_r;
            S->winner = win;
            S->action = kExchanged;
        }
    } else if (threadIdx.x == 0) {
        const int jb = S->mv.jb, pos = S->mv.pmax;
        const bool lower = V.zl[jb] / V.xl[jb] > V.zu[jb] / V.xu[jb];
        V.xl[jb] = __builtin_huge_val();
        V.xu[jb] = __builtin_huge_val();
        V.state[jb] = lower ? IPXK_STATE_IMPLIED_LB : IPXK_STATE_IMPLIED_UB;
        status[jb] = IPXK_BASIC_FREE;
        invscale[pos] = 0.0;
        colscale[jb] = __builtin_huge_val();
        S->mv.jn = jb;
        S->mv.pivot_row = 0.0;
        S->winner = -1;
        S->action = lower ? kImpliedLb : kImpliedUb;
    }
}

// ---- the tableau column: DropDual's pivot search (:343-356), and the column's number of nonzeros for either procedure --------
__global__ __launch_bounds__(kBlock) void drop_column_kernel(int m, int search, const double* __restrict__ lhs, const double* __restrict__ invscale,
                                                             const double* __restrict__ colscale, const DropScalars* S, DropPart* part) {
    const double s = search ? colscale[S->mv.jn] : 0.0;
    DropPart p = partial_identity<1>();
    IPXK_GRID_STRIDE(q, m) {
        const double x = lhs[q], pivot = fabs(x);
        if (search && pivot > kPivotZeroTol) {
            const double v = pivot * invscale[q] * s;
            if (v > kVolumeTol && v > p.v[0]) { p.v[0] = v; p.i[0] = (int)q; }
        }
        p.c += x != 0.0;
    }
    p = block_partial<kBlock>(p);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}
// DropPrimal (search = 0): the pivot from the column at the leaving position.  DropDual: the decision (:357-384).  A winner: the
// variable at pmax leaves.  None: Iterate::make_fixed (x kept), Basis::FixNonbasicVariable, colscale[jn] = 0 -- and position -1
// for the BTRAN that is enqueued either way (the zero vector, its result unused).
__global__ __launch_bounds__(kDropGrid) void drop_column_final_kernel(int nparts, const DropPart* part, int search, const double* __restrict__ lhs,
                                                                      const ipxint* __restrict__ basis, DropScalars* S, IterateVectors V,
                                                                      ipxint* status, double* colscale) {
    const DropPart p = block_partial<kDropGrid>(load_partial(nparts, part));
    if (threadIdx.x != 0) return;
    S->mv.eta_nnz = p.c;
    if (!search) { S->mv.pivot_col = lhs[S->mv.pmax]; return; }
    S->vmax = p.v[0];
    if (p.i[0] != INT_MAX) {
        const int pmax = p.i[0];
        S->mv.pmax = pmax;
        S->mv.jb = (int)basis[pmax];
        S->mv.pivot_col = lhs[pmax];
        S->winner = pmax;
        S->action = kExchanged;
    } else {
        const int jn = S->mv.jn;
        V.xl[jn] = V.xu[jn] = V.zl[jn] = V.zu[jn] = 0.0;
        V.state[jn] = IPXK_STATE_FIXED;
        status[jn] = IPXK_NONBASIC_FIXED;
        colscale[jn] = 0.0;
        S->mv.pmax = -1;
        S->mv.jb = -1;
        S->mv.pivot_col = 0.0;
        S->winner = -1;
        S->action = kFixed;
    }
}
// Basis::ExchangeIfStable :308-313 and invscale_basic[p] = 1 / colscale[jn] (:275, :373)
__global__ void drop_exchange_kernel(const DropScalars* S, ipxint* basis, ipxint* status, const double* colscale, double* invscale) {
    const int jn = S->mv.jn, jb = S->mv.jb, p = S->mv.pmax;
    basis[p] = jn;
    status[jn] = IPXK_BASIC;
    status[jb] = IPXK_NONBASIC;
    invscale[p] = 1.0 / colscale[jn];
}

// Iterate::assert_consistency for the implied states (src/iterate.cc:500-513), on the iterate's own vectors
__global__ void check_implied_kernel(int64_t N, const unsigned char* __restrict__ state, const double* __restrict__ xl,
                                     const double* __restrict__ xu, const double* __restrict__ zl, const double* __restrict__ zu, int* bad) {
    IPXK_GRID_STRIDE(j, N) {
        const unsigned char st = state[j];
        if (st != IPXK_STATE_IMPLIED_LB && st != IPXK_STATE_IMPLIED_UB) continue;
        const bool ok = isinf(xl[j]) && xl[j] > 0.0 && isinf(xu[j]) && xu[j] > 0.0 && zl[j] >= 0.0 && zu[j] >= 0.0;
        if (!ok) atomicMin(bad, (int)j);                          // (the smallest index: no dependence on the order of the threads)
    }
}

}  // namespace

int64_t iterate_check_implied_dev(Context* c) {
    const int64_t N = c->n + c->m;
    c->it_partials.resize((size_t)4 * 1024);
    int* flag = reinterpret_cast<int*>(c->it_partials.get());
    const int kNoBad = INT_MAX;
    staged_h2d(flag, &kNoBad, sizeof(int), c->stream);
    hipLaunchKernelGGL(check_implied_kernel, dim3(grid_for(N, kDropGrid)), dim3(kBlock), 0, c->stream, N, c->it_state.get(), c->it_xl.get(),
                       c->it_xu.get(), c->it_zl.get(), c->it_zu.get(), flag);
    int bad = kNoBad;
    staged_d2h(&bad, flag, sizeof(int), c->stream);
    IPXK_HIP(hipStreamSynchronize(c->stream));
    IPXK_HIP(hipGetLastError());
    return bad == kNoBad ? -1 : bad;
}

void ipm_drop_dev(Context* c, std::vector<ipxint>& basis_io, std::vector<ipxint>& status_io, std::vector<double>& colscale_h,
                  ipxk_drop_info* info, ipxint* log, ipxint log_cap, ipxk_interrupt_fn interrupt, void* user) {
    IPXK_REQUIRE(!comm_active(c), kDeviceLuRefusal);
    IPXK_REQUIRE(c->it_set, "no iterate on the device (ipxk_iterate_set)");
    IPXK_REQUIRE(c->have_plain, "no resident copy of the matrix");
    const int m = (int)c->m, n = (int)c->n;
    const int64_t N = (int64_t)n + m;
    IPXK_REQUIRE(m > 0, "empty model");
    IPXK_REQUIRE((int64_t)basis_io.size() == m && (int64_t)status_io.size() == N && (int64_t)colscale_h.size() == N, "basis, status or colscale of the wrong length");
    hipStream_t s = c->stream;
    const double t_start = now_s();
    ipxk_drop_info I{};
    if (!(c->drop_primal > 0.0) && !(c->drop_dual > 0.0)) { if (info) *info = I; return; }
    for (int p = 0; p < m; p++) {
        const ipxint j = basis_io[(size_t)p];
        IPXK_REQUIRE(j >= 0 && j < N && status_io[(size_t)j] >= 0, "status of a basic variable is not BASIC / BASIC_FREE");
    }

    // the grow-only workspaces of the basis exchanges (MaxvolState): nothing is allocated per call once they have their size
    if (!c->maxvol) c->maxvol = new MaxvolState;
    MaxvolState& M = *c->maxvol;
    DevBuf<ipxint> &basis = M.drop_basis, &status = M.drop_status;
    DevBuf<double> &colscale = M.drop_colscale, &invscale = M.invscale;
    DevBuf<int> &flag = M.flag, &rank = M.rank, &list = M.drop_list;
    DevBuf<unsigned char>& tmp = M.tmp;
    flag.ensure((size_t)N); rank.ensure((size_t)N); list.ensure((size_t)N + 1);
    int* const count = list.get() + N;
    basis.upload(basis_io, s);
    status.upload(status_io, s);
    colscale.upload(colscale_h, s);
    const IterateVectors V{c->it_xl.get(), c->it_xu.get(), c->it_zl.get(), c->it_zu.get(), c->it_state.get()};
    const int gm = grid_for(m, kDropGrid), gN = grid_for(N, kDropGrid);
    const int grow = (int)std::min<int64_t>(kDropGrid, (N + kRowCols - 1) / kRowCols);

    // the candidates: flags, an exclusive scan, the list in ascending order; the host reads the count, then the list if there is one
    auto screen = [&](bool primal) {
        const int64_t len = primal ? m : N;
        if (primal) hipLaunchKernelGGL(drop_primal_flag_kernel, dim3(gm), dim3(kBlock), 0, s, m, basis.get(), status.get(), V, c->drop_primal, flag.get());
        else hipLaunchKernelGGL(drop_dual_flag_kernel, dim3(gN), dim3(kBlock), 0, s, N, status.get(), V, c->drop_dual, flag.get());
        size_t bytes = 0;
        IPXK_HIP(rocprim::exclusive_scan(nullptr, bytes, flag.get(), rank.get(), 0, (size_t)len, rocprim::plus<int>(), s));
        if (tmp.size() < bytes) tmp.resize(bytes);
        IPXK_HIP(rocprim::exclusive_scan(tmp.get(), bytes, flag.get(), rank.get(), 0, (size_t)len, rocprim::plus<int>(), s));
        hipLaunchKernelGGL(drop_store_kernel, dim3(primal ? gm : gN), dim3(kBlock), 0, s, len, flag.get(), rank.get(),
                           primal ? basis.get() : (const ipxint*)nullptr, list.get(), count);
        int cnt = 0;
        staged_d2h(&cnt, count, sizeof(int), s);
        IPXK_HIP(hipStreamSynchronize(s));
        std::vector<int> cand((size_t)cnt);
        if (cnt > 0) { list.download(cand.data(), (size_t)cnt, s); IPXK_HIP(hipStreamSynchronize(s)); }
        return cand;
    };

    // the basis, its scalars and the scaling of the positions: set up when the first candidate is there
    DevBuf<DropPart>& part = M.part;
    part.ensure(kDropGrid);
    M.scalars.ensure(1);                       // (the compact eta lists report their size there)
    M.drop_scalars.ensure(sizeof(DropScalars));
    if (M.drop_h_bytes < sizeof(DropScalars)) {
        if (M.drop_h) { (void)hipHostFree(M.drop_h); M.drop_h = nullptr; M.drop_h_bytes = 0; }
        IPXK_HIP(hipHostMalloc(&M.drop_h, sizeof(DropScalars)));
        M.drop_h_bytes = sizeof(DropScalars);
    }
    DropScalars* const S = reinterpret_cast<DropScalars*>(M.drop_scalars.get());
    DropScalars* const pinned = static_cast<DropScalars*>(M.drop_h);
    std::unique_ptr<DeviceBasis> Bp;
    std::vector<int> pos_h;
    ipxint errflag = 0, interrupted = 0;
    auto ensure_basis = [&]() {
        if (Bp) return true;
        IPXK_HIP(hipMemsetAsync(S, 0, sizeof(DropScalars), s));
        // Maxvolume's last exchanges may still stand as etas behind the factors: this pass starts from fresh factors of that basis
        const bool behind = c->etas_live;
        if (behind) IPXK_REQUIRE(M.basis_h == basis_io, "the eta file behind the factors belongs to another basis");
        maxvol_drop_etas(c);
        Bp.reset(new DeviceBasis(c, M, 0, false, colscale_h.data(), &S->mv));
        Bp->basis_h = basis_io;
        Bp->status_h = status_io;
        if (behind) {
            if (!Bp->refactorize()) { errflag = Bp->errflag; return false; }
        } else {
            LuView Vw;
            IPXK_REQUIRE(lu_view(c, &Vw) && Vw.from_basis && Vw.ndep == 0, "the drop procedures need the factorization of the current basis");
            IPXK_REQUIRE(c->split, "the drop procedures need the operator of the current basis");
            Bp->etas.reset(Vw.bump_size);
        }
        pos_h.assign((size_t)N, -1);
        for (int p = 0; p < m; p++) pos_h[(size_t)basis_io[(size_t)p]] = p;
        invscale.ensure((size_t)m);
        hipLaunchKernelGGL(drop_invscale_kernel, dim3(gm), dim3(kBlock), 0, s, m, basis.get(), status.get(), colscale.get(), invscale.get());
        return true;
    };
    auto poll_interrupt = [&]() -> ipxint {
        if (interrupt) return interrupt(user);
        return c->interrupt ? c->interrupt(c->interrupt_user) : 0;
    };
    ipxint decisions = 0;
    auto record = [&](ipxint variable, ipxint action, ipxint partner) {
        if (log && decisions < log_cap) { log[3 * decisions] = variable; log[3 * decisions + 1] = action; log[3 * decisions + 2] = partner; }
        decisions++;
    };
    // an accepted exchange: this driver's part between DeviceBasis::exchange_if_stable and commit.  false: the candidate is tried again
    // (or the basis has raised its errflag)
    auto exchange = [&](const DropScalars& a) {
        DeviceBasis& B = *Bp;
        if (!B.exchange_if_stable(a.mv)) return false;
        hipLaunchKernelGGL(drop_exchange_kernel, dim3(1), dim3(1), 0, s, S, basis.get(), status.get(), colscale.get(), invscale.get());
        pos_h[(size_t)a.mv.jn] = a.mv.pmax;
        pos_h[(size_t)a.mv.jb] = -1;
        I.updates++;
        B.commit(a.mv);
        return true;
    };

    // ---- DropPrimal (:196-293)
    if (c->drop_primal > 0.0) {
        std::vector<int> cand = screen(true);
        I.primal_candidates = (ipxint)cand.size();
        if (!cand.empty() && ensure_basis()) {
            DeviceBasis& B = *Bp;
            while (!cand.empty() && !B.errflag) {
                const int jb = cand.back(), p = pos_h[(size_t)jb];
                IPXK_REQUIRE(p >= 0 && p < m, "a candidate of DropPrimal is not basic");
                if ((interrupted = poll_interrupt()) != 0) break;
                hipLaunchKernelGGL(drop_set_kernel, dim3(1), dim3(1), 0, s, jb, p, jb, S);
                B.btran_unit();
                hipLaunchKernelGGL(drop_row_kernel, dim3(grow), dim3(kBlock), 0, s, n, N, c->pl_Ap.get(), c->pl_Ai.get(), c->pl_Ax.get(), B.btran,
                                   status.get(), colscale.get(), invscale.get(), S, part.get());
                hipLaunchKernelGGL(drop_row_final_kernel, dim3(1), dim3(kDropGrid), 0, s, grow, part.get(), S, V, status.get(), colscale.get(),
                                   invscale.get());
                // the FTRAN of the entering variable (ExchangeIfStable with sys = +1, src/basis.cc:290-291): pivot from the column, and the eta
                B.ftran();
                hipLaunchKernelGGL(drop_column_kernel, dim3(gm), dim3(kBlock), 0, s, m, 0, B.lhs, invscale.get(), colscale.get(), S, part.get());
                hipLaunchKernelGGL(drop_column_final_kernel, dim3(1), dim3(kDropGrid), 0, s, gm, part.get(), 0, B.lhs, basis.get(), S, V, status.get(),
                                   colscale.get());
                const DropScalars a = read_scalars(S, pinned, s);
                if (a.winner >= 0) {
                    if (!exchange(a)) continue;                       // "factorization was unstable, try again" (:273-274)
                    record(jb, kExchanged, a.mv.jn);
                } else {
                    B.status_h[(size_t)jb] = IPXK_BASIC_FREE;
                    colscale_h[(size_t)jb] = INFINITY;
                    I.primal_dropped++;
                    record(jb, a.action, -1);
                }
                cand.pop_back();
            }
            errflag = B.errflag ? B.errflag : interrupted;
        }
    }
    // ---- DropDual (:295-387)
    if (c->drop_dual > 0.0 && !errflag) {
        std::vector<int> cand = screen(false);
        I.dual_candidates = (ipxint)cand.size();
        if (!cand.empty() && ensure_basis()) {
            DeviceBasis& B = *Bp;
            while (!cand.empty() && !B.errflag) {
                const int jn = cand.back();
                if ((interrupted = poll_interrupt()) != 0) break;
                hipLaunchKernelGGL(drop_set_kernel, dim3(1), dim3(1), 0, s, jn, -1, -1, S);
                B.ftran();
                hipLaunchKernelGGL(drop_column_kernel, dim3(gm), dim3(kBlock), 0, s, m, 1, B.lhs, invscale.get(), colscale.get(), S, part.get());
                hipLaunchKernelGGL(drop_column_final_kernel, dim3(1), dim3(kDropGrid), 0, s, gm, part.get(), 1, B.lhs, basis.get(), S, V, status.get(),
                                   colscale.get());
                // the BTRAN of the leaving variable (ExchangeIfStable with sys = -1, :292-293): pivot from the row
                B.btran_unit();
                mv_pivot_from_row(c, B.btran, &S->mv);
                const DropScalars a = read_scalars(S, pinned, s);
                if (a.winner >= 0) {
                    if (!exchange(a)) continue;                       // (:371-372)
                    record(jn, kExchanged, a.mv.jb);
                } else {
                    B.status_h[(size_t)jn] = IPXK_NONBASIC_FIXED;
                    colscale_h[(size_t)jn] = 0.0;
                    I.dual_dropped++;
                    record(jn, kFixed, -1);
                }
                cand.pop_back();
            }
            errflag = B.errflag ? B.errflag : interrupted;
        }
    }
    IPXK_HIP(hipStreamSynchronize(s));
    IPXK_HIP(hipGetLastError());
    if (Bp) {
        DeviceBasis& B = *Bp;
        check_sweep_abort(c);
        // the scaling factors as the deciding kernels have left them on the device: what the operator below is built from and the
        // caller goes on with
        colscale.download(colscale_h.data(), (size_t)N, s);
        IPXK_HIP(hipStreamSynchronize(s));
        // the operator of the basis that Maxvolume goes on from: fresh factors where exchanges stand behind the old ones, else the
        // same factors with the new statuses and scaling factors.  After an interrupt too: the exchanges and drops made so far
        // stay, and the context must not be left with the factors of an earlier basis.  Only a basis that has failed itself
        // (301 / 306) is left as it is.
        if (!B.errflag && I.updates + I.primal_dropped + I.dual_dropped > 0) {
            if (B.etas.K > 0) { if (!B.refactorize()) errflag = B.errflag; }
            else split_rescale_host(c, B.status_h.data(), colscale_h.data());
        }
        IPXK_HIP(hipStreamSynchronize(s));
        basis_io = B.basis_h;
        status_io = B.status_h;
        I.refused = B.refused;
        I.factorizations = B.factorizations;
    }
    I.errflag = errflag;
    I.seconds = now_s() - t_start;
    if (info) *info = I;
}

void ipm_drop_degenerate_dev(Context* c, const double* b, const double* cc, const double* lb, const double* ub, ipxk_drop_info* info,
                             ipxint* basis_out, ipxint* status_out, double* colscale_out, ipxint* log, ipxint log_cap,
                             ipxk_interrupt_fn interrupt, void* user) {
    IPXK_REQUIRE(!comm_active(c), kDeviceLuRefusal);
    IPXK_REQUIRE(c->it_set, "no iterate on the device (ipxk_iterate_set)");
    IPXK_REQUIRE(!c->postprocessed, kPostprocessedRefusal);
    IPXK_REQUIRE(c->sb.current(c) || c->drv.current(c), "no live basis: call ipxk_ipm_starting_basis or ipxk_ipm_driver_basis first");
    LiveBasis& live = c->sb.current(c) ? c->sb : c->drv;
    const int64_t N = c->n + c->m;
    hipStream_t s = c->stream;
    std::vector<ipxint> basis = live.basis, status = live.status;
    ipxk_drop_info I{};
    // the gate (:36), on the objectives without the offset
    double obj[3];
    iterate_objectives_dev(c, b, cc, lb, ub, obj);
    std::vector<double> colscale((size_t)N);
    {
        if (!c->maxvol) c->maxvol = new MaxvolState;
        c->maxvol->drop_colscale.ensure((size_t)N + 1);     // (the scaling factors and, behind them, the flag of the kernel)
        double* d = c->maxvol->drop_colscale.get();
        int* flag = reinterpret_cast<int*>(d + N);
        IPXK_HIP(hipMemsetAsync(flag, 0, sizeof(int), s));
        iterate_scaling_factors_dev(c, d, flag);
        staged_d2h(colscale.data(), d, (size_t)N * sizeof(double), s);
        IPXK_HIP(hipStreamSynchronize(s));
    }
    if (obj[0] >= obj[1]) {
        live.clear();                                       // (an exception inside the pass leaves no live basis)
        ipm_drop_dev(c, basis, status, colscale, &I, log, log_cap, interrupt, user);
        if (!I.errflag) live.store(c, basis, status);
    }
    if (basis_out) std::copy(basis.begin(), basis.end(), basis_out);
    if (status_out) std::copy(status.begin(), status.end(), status_out);
    if (colscale_out) std::copy(colscale.begin(), colscale.end(), colscale_out);
    if (info) *info = I;
}

}  // namespace ipxk
