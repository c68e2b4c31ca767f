// The gather matrices of the model and the NormalMatrix product
//   lhs = AI * W * AI' * rhs                 reference src/normal_matrix.cc:45-126
// as two row-gather SpMVs:  t = Ws .* (A' rhs);  lhs = W_I .* rhs + A t  with the
// dot product rhs'lhs fused into the second pass (src/normal_matrix.cc:123-124).
// Here: the phased layout's geometry, the choice of the layout, the drivers of the device builders and the views the kernels take.
// The arrays come from layout_host.hip or layout_device.hip, the masked and compacted forms from spmv_mask.hip.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

#include "context.hpp"
#include "spmv_kernels.hpp"

namespace ipxk {

// ---------------------------------------------------------------------------
// GatherMatrix
// ---------------------------------------------------------------------------
int slice_elems() {
    static int cached = 0;
    if (!cached) {
        int kb = 1024;
        if (const char* e = getenv("IPXK_SLICE_KB")) kb = atoi(e) > 0 ? atoi(e) : kb;
        cached = kb * 128;   // doubles
    }
    return cached;
}

// elements of the gathered vector per phase of the phased layout: ~1 MiB of x; at most kMaxPhases phases (the
// per-(row,phase) count table grows with P), so very long vectors get proportionally larger slices
int64_t phase_slice(int64_t ncols_) {
    constexpr int kMaxPhases = 64;
    int64_t slice = slice_elems();
    if ((ncols_ + slice - 1) / slice > kMaxPhases) slice = (ncols_ + kMaxPhases - 1) / kMaxPhases;
    return slice;
}

void GatherMatrix::set_geometry(int64_t nrows_, int64_t ncols_) {
    const int64_t slice = phase_slice(ncols_);
    P = (int)std::max<int64_t>(1, (ncols_ + slice - 1) / slice);
    int maxwg = kMaxWorkgroups;
    if (const char* e = getenv("IPXK_MAX_WG")) maxwg = atoi(e) > 0 ? atoi(e) : maxwg;
    G = (int)std::min<int64_t>(maxwg, std::max<int64_t>(1, (nrows_ + kBlock - 1) / kBlock));
    RT = 1;
    while (RT < kMaxRT && (int64_t)G * kBlock * RT < nrows_) RT *= 2;
    const int64_t RW = (int64_t)kBlock * RT;     // count slots per step
    // rows a workgroup owns per round: all RW slots, or -- for matrices too small to give
    // every CU several workgroups that way -- fewer (threads without a row still stream)
    RWrows = (int)RW;
    if (RT == 1 && nrows_ < (int64_t)kBlock * maxwg) {
        const int64_t want = (nrows_ + maxwg - 1) / maxwg;
        RWrows = (int)std::min<int64_t>(kBlock, std::max<int64_t>(32, (want + 31) / 32 * 32));
    }
    G = (int)std::max<int64_t>(1, std::min<int64_t>(maxwg, (nrows_ + RWrows - 1) / RWrows));
    Q = (int)std::max<int64_t>(1, (nrows_ + (int64_t)G * RWrows - 1) / ((int64_t)G * RWrows));
}

// an IPXK_SPMV_* switch set to 0
static bool env_off(const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '0';
}

// microseconds per call of `launch` on stream s: two warm-up calls, then five between events
template <class F>
static float time_launches(hipStream_t s, F&& launch) {
    hipEvent_t e0, e1;
    IPXK_HIP(hipEventCreate(&e0));
    IPXK_HIP(hipEventCreate(&e1));
    const int reps = 5;
    for (int r = 0; r < 2 + reps; r++) {
        if (r == 2) IPXK_HIP(hipEventRecord(e0, s));
        launch();
    }
    IPXK_HIP(hipEventRecord(e1, s));
    IPXK_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    IPXK_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return ms * 1e3f / reps;
}

// Times the unmasked product on layout L, whose arrays must be in place, x = 0.
float GatherMatrix::time_layout(SpmvLayout L, hipStream_t s) {
    const SpmvLayout in_use = layout;
    layout = L;
    DevBuf<double> tx((size_t)std::max(ncols, 1)), tout((size_t)std::max(nrows, 1));
    IPXK_HIP(hipMemsetAsync(tx.get(), 0, tx.size() * sizeof(double), s));
    const EpiScale epi{{}, nullptr, tout.get()};
    const float us = time_launches(s, [&] { launch_spmv(*this, tx.get(), epi, nullptr, nullptr, s); });
    layout = in_use;
    return tuned_us[(int)L] = us;
}

// The layout choice.  IPXK_SPMV_LAYOUT=<name> forces a layout where it can be built (else the tile base, else the phased layout);
// unset or "auto":
//   * the phased, fused, sorted fused, fused accumulated layouts and the plain rows add a row's products in the same (the
//     reference's) order and give bit-identical results, so a timing on the spot may choose among them: a candidate is kept if
//     it beats the layout in use by 5 %;
//   * the sliced layout associates a row's sum per slice, hence whether it is used must not depend on a timing: it is chosen by a
//     property of the matrix alone -- x does not fit an XCD's L2 and the gathers of a row block spread over the slices (share of
//     its fullest slice <= 1.5 / #slices: that is where confining every XCD to one slice of x pays; measured, C3-sized: uniformly
//     random indices 256 against 300 us per apply, banded ones 240-400 against 190-220).  The accumulated tiles give its partial
//     sums bit for bit for rows stored with ascending indices only, so they are used whenever they can be built (the host
//     builder refuses a matrix with long rows, the device path builds them from the matrix without its long rows;
//     IPXK_SPMV_ACC=0: never), never by a timing: no timing takes part in the choice for such a matrix.
// Masked products (the basis path's N N') keep the tile base whatever the choice; the arrays of the candidates that lost are
// released unless IPXK_BUILD_ALL_LAYOUTS is set (tests: the device builders against the host builders).
void GatherMatrix::select_layout(const std::function<bool(SpmvLayout)>& make, hipStream_t s) {
    using L = SpmvLayout;
    layout = L::phased;
    sliced = SlicedMatrix(); sorted = SortedMatrix(); acc = AccMatrix(); accf = AccMatrix();
    if (const char* e = getenv("IPXK_SPMV_LAYOUT")) {
        for (int f = 0; f < kNumSpmvLayouts; f++) {
            if (!kSpmvLayoutNames[f] || strcmp(e, kSpmvLayoutNames[f]) != 0) continue;
            if (L(f) == L::acc) make(L::sliced);          // its slices
            layout = make(L(f)) ? L(f) : tile_base();
            return;
        }
    }
    // small matrices (a few microseconds either way, not worth more copies of the matrix) and auxiliary ones: no timing
    if (nnz < (1 << 16) || tune_level == 0) return;
    const bool keep_all = getenv("IPXK_BUILD_ALL_LAYOUTS") != nullptr;
    auto drop = [&](L l) {                       // (never the tile base: the masked products use it)
        if (keep_all) return;
        if (l == L::sortedfused) sorted = SortedMatrix();
        else if (l == L::acc) acc = AccMatrix();
        else if (l == L::accfused) accf = AccMatrix();
    };
    // the tile base (tune_level 1: phased against fused only)
    const bool phased = make(L::phased);       // (not built by the device builders)
    if (phased) time_layout(L::phased, s);
    SlicedMatrix fusedm, slicedm;
    if (make(L::fused)) { time_layout(L::fused, s); fusedm = std::exchange(sliced, SlicedMatrix()); }
    if (tune_level > 1 && make(L::sliced)) { time_layout(L::sliced, s); slicedm = std::exchange(sliced, SlicedMatrix()); }
    const double share = slicedm.built ? slicedm.dominant_fraction : fusedm.built ? fusedm.dominant_fraction : 1.0;
    const bool spread = slicedm.built && share <= 1.5 / slicedm.nslices;
    if (spread) {
        sliced = std::move(slicedm);
        layout = L::sliced;
        if (!env_off("IPXK_SPMV_ACC") && make(L::acc)) {
            time_layout(L::acc, s);
            layout = L::acc;
        }
    } else {
        if (fusedm.built && (!phased || tuned_us[(int)L::fused] < 0.95f * tuned_us[(int)L::phased])) {
            sliced = std::move(fusedm);
            layout = L::fused;
        }
        auto consider = [&](L cand) {
            if (!make(cand)) return;
            if (time_layout(cand, s) < 0.95f * tuned_us[(int)layout]) { drop(layout); layout = cand; }
            else drop(cand);
        };
        if (tune_level > 1 && !env_off("IPXK_SPMV_SORTED")) consider(L::sortedfused);
        if (tune_level > 1 && !env_off("IPXK_SPMV_ACC")) consider(L::accfused);
        if (layout != L::accfused && nnz <= (int64_t(4) << 20) && !env_off("IPXK_SPMV_PLAIN")) consider(L::plain);
    }
    if (sliced.built) {        // the phased copy of the entries is not needed
        idx.release(); val.release(); counts.release(); step_ptr.release();
        wg_chunk_ptr.release(); chunk_start.release(); chunk_info.release(); chunk_step.release();
    }
    if (getenv("IPXK_VERBOSE")) {
        fprintf(stderr, "ipxk: gather matrix %d x %d nnz %lld:", nrows, ncols, (long long)nnz);
        for (int l = 0; l < kNumSpmvLayouts; l++)
            if (kSpmvLayoutNames[l] && tuned_us[l] > 0.f) fprintf(stderr, " %s %.1f us,", kSpmvLayoutNames[l], tuned_us[l]);
        fprintf(stderr, " fullest-slice share %.2f -> %s\n", share, kSpmvLayoutNames[(int)layout]);
        const AccMatrix& a = layout == L::accfused ? accf : acc;
        if (a.built)
            fprintf(stderr, "ipxk:   %d rows per tile, %lld steps / %lld batches, %.1f%% of the entries waited\n", a.RB, (long long)a.nsteps,
                    (long long)a.nbatches, 100.0 * (double)a.deferred / (double)nnz);
    }
}

// The device path for matrices whose gathers have locality, or whose gathered vector fits an XCD's L2 (round 4): the fused tiles
// (one slice; also what the masked products of the basis path use), the fused sorted tiles and the fused accumulated tiles, all
// built on the device and all bit-identical to the phased layout (the accumulated ones for sorted rows only: device_build_acc_fused
// checks), so a timing chooses among them; the plain rows join for small matrices.  The phased layout is not built on this path.
bool GatherMatrix::build_device_local(LayoutScratch& S, int64_t nrows_, int64_t ncols_, int64_t nnz_, const int* dptr, const int* didx,
                                      const double* dval, double share, hipStream_t s) {
    if (getenv("IPXK_LAYOUT_LOCAL") && getenv("IPXK_LAYOUT_LOCAL")[0] == 'h') return false;      // host builders for these matrices
    SlicedMatrix fu;
    if (!device_build_sliced(S, fu, (int)nrows_, (int)ncols_, nnz_, dptr, didx, dval, s, 1)) return false;
    nrows = (int)nrows_; ncols = (int)ncols_; nnz = nnz_;
    set_geometry(nrows_, ncols_);                 // (nlong, nseg, ... : set by build_device)
    fu.dominant_fraction = share;
    select_layout([&](SpmvLayout L) {
        switch (L) {
            case SpmvLayout::fused: sliced = std::move(fu); return true;
            case SpmvLayout::sortedfused: {
                SortedMatrix so;
                if (!device_build_sorted_fused(S, so, nrows, ncols, nnz_, dptr, didx, dval, s)) return false;
                sorted = std::move(so);
                return true;
            }
            case SpmvLayout::accfused: {
                AccMatrix af;
                if (nlong > 0 || !device_build_acc_fused(S, af, nrows, ncols, nnz_, dptr, didx, dval, s)) return false;
                accf = std::move(af);
                return true;
            }
            case SpmvLayout::plain: return csr_ptr != nullptr;
            default: return false;
        }
    }, s);
    return true;
}

// The device path (layout_device.hip): sliced and accumulated layouts by radix sorts, for matrices whose gathered vector needs
// slicing and whose gathers spread over the slices -- the same decision build() takes from the same property of the
// matrix, so a model gets the same layouts whichever path builds them.
bool GatherMatrix::build_device(LayoutScratch& S, int64_t nrows_, int64_t ncols_, int64_t nnz_, const int* dptr, const int* didx,
                                const double* dval, hipStream_t s) {
    if (const char* e = getenv("IPXK_LAYOUT_BUILD")) if (e[0] == 'h') return false;           // host: the test reference
    if (const char* e = getenv("IPXK_SPMV_LAYOUT")) if (std::string(e) != "auto") return false;
    if (tune_level < 2 || keep_plain || nnz_ < (1 << 16) || getenv("IPXK_STAMPS")) return false;
    if (nrows_ >= (int64_t(1) << 31) - 1 || ncols_ >= (int64_t(1) << 31) - 1 || nnz_ >= (int64_t(1) << 31) - kLongSeg) return false;
    nlong = 0; nseg = 0;
    h_row_long.clear();
    long_partials.resize(1);
    // long rows go to the long-row kernels' arrays; the tile layouts are built from the matrix without them
    DevBuf<int> sptr, sidx;
    DevBuf<double> sval;
    const int64_t nnz_all = nnz_;
    if (device_max_row_length(S, (int)nrows_, dptr, s) > kMaxRowLen) {
        if (getenv("IPXK_LONG_ROWS_HOST")) return false;                                // (tests: the host builders as the reference)
        if (!device_strip_long_rows(S, *this, (int)nrows_, dptr, didx, dval, sptr, sidx, sval, &nnz_, s)) return false;
        dptr = sptr.get(); didx = sidx.get(); dval = sval.get();
        if (nnz_ < (1 << 16)) { nlong = 0; nseg = 0; h_row_long.clear(); return false; }
    }
    SlicedMatrix sl;
    const bool slices = device_build_sliced(S, sl, (int)nrows_, (int)ncols_, nnz_, dptr, didx, dval, s);
    if (!slices || !(sl.dominant_fraction <= 1.5 / sl.nslices)) {
        const bool ok = build_device_local(S, nrows_, ncols_, nnz_, dptr, didx, dval, slices ? sl.dominant_fraction : 1.0, s);
        nnz = nnz_all;
        return ok;
    }
    nrows = (int)nrows_; ncols = (int)ncols_; nnz = nnz_;
    set_geometry(nrows_, ncols_);
    select_layout([&](SpmvLayout L) {
        switch (L) {
            case SpmvLayout::sliced: sliced = std::move(sl); return true;
            case SpmvLayout::acc: {
                AccMatrix ac;
                if (!device_build_acc(S, ac, sliced, nrows, ncols, nnz_, dptr, didx, dval, s)) return false;
                acc = std::move(ac);
                return true;
            }
            default: return false;
        }
    }, s);
    nnz = nnz_all;
    return true;
}

static AccView view_of(const AccMatrix& A, int nrows) {
    AccView V;
    A.fill_view(V, nrows);
    return V;
}
AccView GatherMatrix::acc_view() const { return view_of(acc, nrows); }
AccView GatherMatrix::acc_fused_view() const { return view_of(accf, nrows); }

SortedView GatherMatrix::sorted_view() const {
    SortedView V;
    V.xmin = sorted.xmin.get();
    V.row_long = nlong > 0 ? row_long.get() : nullptr;
    V.nrows = nrows; V.nrows_pad = sorted.nrows_pad; V.nrb = sorted.nrb; V.RB = sorted.RB;
    V.sub_ptr = sorted.sub_ptr.get(); V.cnt = sorted.cnt.get(); V.pack = sorted.pack.get(); V.val = sorted.val.get();
    return V;
}

SlicedView GatherMatrix::sliced_view(int which) const {
    SlicedView V;
    V.nrows = nrows; V.nrows_pad = sliced.nrows_pad; V.nslices = sliced.nslices; V.nrb = sliced.nrb; V.R = sliced.R;
    V.tile_ptr = sliced.tile_ptr.get(); V.cnt = sliced.cnt.get();
    V.idx = sliced.idx.get(); V.val = which == 1 ? valM.get() : sliced.val.get(); V.partial = sliced.partial.get();
    if (which == 2) {
        V.tile_ptr = compact.tile_ptr.get(); V.cnt = compact.cnt.get(); V.idx = compact.idx.get(); V.val = compact.val.get();
    }
    V.row_long = nlong > 0 ? row_long.get() : nullptr;
    V.masked = which == 1 ? 1 : 0;
    return V;
}

GatherView GatherMatrix::view(bool use_masked) const {
    GatherView V;
    V.nrows = nrows; V.ncols = ncols;
    V.P = P; V.G = G; V.RT = RT; V.Q = Q; V.RWrows = RWrows;
    V.step_ptr = step_ptr.get(); V.counts = counts.get();
    V.wg_chunk_ptr = wg_chunk_ptr.get(); V.chunk_start = chunk_start.get();
    V.chunk_info = chunk_info.get(); V.chunk_step = chunk_step.get();
    V.idx = idx.get(); V.val = (use_masked && tile_base() == SpmvLayout::phased) ? valM.get() : val.get();
    V.row_long = nlong > 0 ? row_long.get() : nullptr;
    V.nseg = nseg; V.seg_p0 = seg_p0.get(); V.seg_p1 = seg_p1.get();
    V.lidx = lidx.get(); V.lval = (use_masked && nlong > 0) ? lvalM.get() : lval.get();
    V.nlong = nlong; V.long_row = long_row.get(); V.long_slot = long_slot.get();
    V.long_partials = long_partials.get();
    V.stamps = stamps.size() ? stamps.get() : nullptr;
    V.masked = use_masked ? 1 : 0;
    return V;
}

// the time of the two products of NormalMatrix::Apply on a pair of gather matrices (microseconds)
float time_normal_pair(Context* c, GatherMatrix& Ac, GatherMatrix& Ar) {
    hipStream_t s = c->stream;
    const size_t m = (size_t)std::max<int64_t>(c->m, 1), n = (size_t)std::max<int64_t>(c->n, 1);
    DevBuf<double> y(m), t(n), out(m);
    IPXK_HIP(hipMemsetAsync(y.get(), 0, m * sizeof(double), s));
    EpiScale ep1{{}, nullptr, t.get()}, ep2{{}, nullptr, out.get()};
    return time_launches(s, [&] {
        launch_spmv(Ac, y.get(), ep1, nullptr, nullptr, s);
        launch_spmv(Ar, t.get(), ep2, nullptr, nullptr, s);
    });
}

// ---------------------------------------------------------------------------
// NormalMatrix::_Apply on device vectors
// ---------------------------------------------------------------------------
// W: device pointer to n+m weights.  Dot partials go to part(kPartCdot); *ndot
// receives their count (nullptr: no dot product wanted).
// column partition: lhs holds the cross-rank sum of A_g t_g; add the slack term, form the dot
__global__ __launch_bounds__(kBlock) void normal_finish_kernel(int m, const double* __restrict__ wI,
                                                               const double* __restrict__ y,
                                                               double* __restrict__ lhs, double* dot_partials,
                                                               const int* done) {
    if (done && *done) return;
    __shared__ double red[kBlock / 64 + 1];
    double dotpart = 0.0;
    for (int r = blockIdx.x * kBlock + threadIdx.x; r < m; r += gridDim.x * kBlock) {
        const double v = y[r] * wI[r] + lhs[r];
        lhs[r] = v;
        dotpart += y[r] * v;
    }
    if (dot_partials) {
        const double d = block_reduce<SumOp>(dotpart, red);
        if (threadIdx.x == 0) dot_partials[blockIdx.x] = d;
    }
}

void normal_apply_dev(Context* c, const double* W, const double* rhs, double* lhs, int* ndot,
                      const int* done) {
    const int64_t n = c->n;
    if (comm_cols(c)) {
        // this rank's columns: t_g = W_g .* (A_g' y) is local, lhs = sum over ranks of A_g t_g
        EpiScale e1{{}, W, c->tcols.get()};
        launch_spmv(c->Acols, rhs, e1, nullptr, done, c->stream);
        double* stage = comm_stage(c, (size_t)c->m);
        EpiScale e2{{}, nullptr, stage ? stage : lhs};
        launch_spmv(c->Arows, c->tcols.get(), e2, nullptr, done, c->stream);
        if (stage) comm_allreduce_sum_staged(c, lhs, (size_t)c->m);
        else comm_allreduce_sum(c, lhs, (size_t)c->m);
        const int g = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (c->m + kBlock - 1) / kBlock));
        hipLaunchKernelGGL(normal_finish_kernel, dim3(g), dim3(kBlock), 0, c->stream, (int)c->m, W + n, rhs, lhs,
                           ndot ? c->part(kPartCdot) : nullptr, done);
        if (ndot) *ndot = g;
        return;
    }
    if (c->reord.in_use) {
        // the CR loop of the diag path in the renumbered model (reorder.hip): rhs, lhs and the weights in the new numbering
        Reordered& R = c->reord;
        EpiScale e1{{}, R.W.get(), R.tcols.get()};
        launch_spmv(R.Acols, rhs, e1, nullptr, done, c->stream);
        EpiNormalRows e2{{}, R.W.get() + n, rhs, lhs};
        const int np = launch_spmv(R.Arows, R.tcols.get(), e2, ndot ? c->part(kPartCdot) : nullptr, done, c->stream);
        if (ndot) *ndot = np;
        return;
    }
    double* stage = comm_rows(c) ? comm_stage(c, (size_t)n) : nullptr;
    EpiScale e1{{}, W, stage ? stage : c->tcols.get()};
    launch_spmv(c->Acols, rhs, e1, nullptr, done, c->stream);
    if (stage) comm_allreduce_sum_staged(c, c->tcols.get(), (size_t)n);
    else if (comm_rows(c)) comm_allreduce_sum(c, c->tcols.get(), (size_t)n);
    EpiNormalRows e2{{}, W + n, rhs, lhs};
    const int np = launch_spmv(c->Arows, c->tcols.get(), e2, ndot ? c->part(kPartCdot) : nullptr,
                               done, c->stream);
    if (ndot) *ndot = np;
}

void debug_single_pass(Context* c, int which, const double* x, double* out) {
    if (which == 1) {
        EpiScale e1{{}, c->W, out};
        launch_spmv(c->Acols, x, e1, nullptr, nullptr, c->stream);
    } else {
        EpiNormalRows e2{{}, c->W + c->n, out, out};   // y := out (only timing matters)
        launch_spmv(c->Arows, x, e2, nullptr, nullptr, c->stream);
    }
}

}  // namespace ipxk
