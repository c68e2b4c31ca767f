// Basis LU factorization on the device behind the reference's
// LuFactorization contract, src/lu_factorization.h:21-58:
//     B[rowperm,colperm] = (L+I)*U,  L strictly lower without its diagonal, U upper with the diagonal last in
//     each column, indices sorted; dependent columns replaced by unit columns and listed.
// It takes the place of the reference's kernel src/basiclu_kernel.cc:31-82 (BASICLU, third party); the call
// sites are ForrestTomlin::_Factorize (src/forrest_tomlin.cc:28-30) and, through LuUpdate::Factorize,
// Basis::Factorize (src/basis.cc:116-156).
//
// LP bases are nearly triangular, and that is what this code is built for:
//   1. SINGLETON ROUNDS.  A column with one entry in the active rows is a pivot without arithmetic (its other
//      entries are entries of U); so is a row with one entry in the active columns (the rest of the pivot column,
//      divided by the pivot, is a column of L; nothing fills in).  All current column singletons, then all
//      current row singletons, are taken per round -- they are independent of each other -- until neither
//      exists.  Integer work over the CSC and a row-wise copy of B: one thread per column (row), conflicts (two
//      singleton columns in one row, two singleton rows in one column) settled by atomic min / max, the pivot
//      order inside a round fixed by a prefix sum over the indices, so the result does not depend on timing.
//   2. THE BUMP that remains (for LP bases: tens to a few thousand rows) is factorized as a DENSE matrix with
//      partial pivoting, right-looking, in panels of 32 columns: a one-workgroup panel kernel (pivot search,
//      scaling, update inside the panel), a kernel that finishes the panel's rows of U, and a tiled update of
//      the trailing matrix.  Every entry receives its updates one pivot at a time in pivot order, products
//      rounded before they are subtracted: the arithmetic of the plain column-by-column elimination, bit for
//      bit.  Rows are never swapped (a row carries the step at which it was pivoted).
//   3. ASSEMBLY.  Every entry of B outside the bump and every nonzero of the factorized bump is keyed by
//      (pivot stage of its column, pivot stage of its row); one radix sort per factor orders the columns and,
//      inside them, the rows.
// The rules (tolerances, tie breaks, order of the dependent columns) are restated on the CPU by the test
// infrastructure, which the tests compare against entry by entry; the reference's own
// LuFactorization::Factorize (stability estimate) and ForrestTomlin judge the factors there as well.
//   2b. TEARING.  A bump of more than IPXK_LU_BUMP_MAX rows (default 8192) is not factorized densely as it stands.
//      LP bumps are sparse and nearly triangular themselves -- a few columns (the ones recent basis exchanges
//      brought in) block the singleton rounds, and singleton peeling is all-or-nothing along dependency chains.
//      Whenever the rounds stall, the T active columns with the most active entries (ties: smaller index) are set
//      aside as SPIKES (T = 1, doubled up to 1024 while a tear frees fewer than 64 pivots, back to 1 otherwise)
//      and the rounds go on without them until no active column is left: the bump-and-spike ordering of
//      Hellerman and Rarick in rounds.  Round pivots still cost no arithmetic outside the spikes.  The spikes
//      receive the updates of the row singleton pivots in pivot order: a forward substitution with the L columns
//      found so far, run for 64 spikes at a time as a dense dim x 64 block (one wavefront per row, one lane per
//      spike, rows of one half-round in one launch, every row's products subtracted in pivot order).  Their
//      entries in pivoted rows become entries of U, their entries in the never-pivoted rows form the dense block
//      of step 2.
//   2c. ELIMINATION ROUNDS (round 4).  If the spikes themselves would exceed the limit, the basis is no longer refused: the
//      factorization starts again and, when the singleton rounds stall, eliminates the bump SPARSELY.  The active submatrix
//      becomes a compact problem of its own (rows / columns renumbered in order, CSC + a row-wise index).  A round
//        * picks one candidate per column: among the entries that pass the absolute and the relative pivot threshold, the one in
//          the shortest row; its Markowitz cost is (row count - 1)(column count - 1);
//        * lets the candidates of cost <= max(4, 2 x the cheapest, the quartile of all costs rounded up to 2^b - 1) compete: a row
//          keeps its best (cost, then column index), and a contender wins unless a better one has an entry in its pivot row or
//          its pivot row in this column -- the winners' pivots form a DIAGONAL block, so eliminating them together is exact
//          (Schur complement = A22 - sum over winners of column x row / pivot), and a singleton is simply a winner of cost 0;
//        * writes the updates -(a_i'j / pivot) a_ij' behind the surviving entries (which keep their order: the renumbering is
//          monotone), sorts the updates, merges the two sorted lists (stable: entry first, then the updates in ascending order of
//          the winner's column), sums equal positions in that order with the product rounded before it is subtracted, drops
//          sums that are exactly zero, and rebuilds pointers, row index and counts.  Entries whose row or column was pivoted
//          leave the matrix for the list E (indices in B, value at that time): E replaces B in the assembly of step 3.
//      The rounds end at IPXK_LU_SPARSE_MIN columns (512), or -- once the rest fits the dense code -- after two rounds in a row
//      that each eliminated fewer than 1 / 256 of the columns (what is left has no large independent pivot sets any more), or
//      when no column has an acceptable pivot; they are GIVEN UP (IPXK_E_UNSUPPORTED) when the current matrix grows beyond
//      IPXK_LU_SPARSE_FILL_MAX (8) x nnz(B) + 2^20 entries -- bounded work.  The rest is factorized densely as in step 2, its columns in ascending order
//      of their number of entries (fewer nonzeros in the dense factors).  Only if THAT rest exceeds the limit is the basis
//      refused (IPXK_E_UNSUPPORTED).  IPXK_LU_SPARSE=1: elimination rounds instead of tearing from the start; =0: never.
//      Every rule is restated sequentially on the CPU by the test infrastructure; the factors are bit-identical to that restatement.
// Where the steps live: 1, 2b, 2c, 3 and the driver lu_factorize_device here; 2 (the dense LU: struct Dense, the panel and
// trailing kernels, their driver) in lu_dense.hip; the policy record LuPolicy and the shared helpers in lu_internal.hpp.
#include <chrono>
#include <climits>
#include <cstdlib>

#include "lu_internal.hpp"
#include "trisolve.hpp"

namespace ipxk {

namespace {

constexpr u64 kNoKey = ~0ull;

int bits_for(int64_t n) { int b = 1; while ((int64_t(1) << b) < n) b++; return b; }

// The slots of LuWork::counters; a read-back leaves them at the same places of the pinned block h.
constexpr int kCounters = 32;
enum {
    kCntColSing = 1, kCntRowSing = 2,      // # column / row singletons (lu_count_kinds_kernel)
    kCntSpike = 3,                         // spikes: # entries of a batch in pivoted rows, then the cursor of their list
    kCntNoStage = 6,                       // a pivot stage is missing (lu_perm_kernel)
    kCntBadIndex = 7,                      // a row index of B out of range (lu_expand_kernel)
    kCntBusy = 8,                          // [kCntBusy + b]: iteration b of a batch of singleton rounds found a pivot
};
constexpr int kBatch = 8;                  // singleton rounds per read-back
// The slots of the elimination rounds' statistics (LuWork::Sp::stats, reset per round); read back to the same places of h,
// with the end of the updates' offsets behind them.
enum {
    kSpCheapest = 0, kSpCandidates = 1,    // cheapest cost, # candidates
    kSpLimit = 2,                          // the cost limit of the contenders
    kSpWinners = 3, kSpLeaving = 4,        // # winners, # entries of their pivot rows and columns
    kSpHist = 8,                           // [kSpHist + b]: # candidates of cost < 2^b
    kSpTooMany = 40,                       // a winner alone sends out more than 2^28 updates
    kSpUpdates64 = 42,                     // the round's number of updates in 64 bits (two slots)
    kSpStats = 48,
    kHUpdatesEnd = kSpStats,               // the end of the updates' offsets as an int: no longer read (the 64-bit count is), the copy is kept so that the copies of a round stay what they were
};
constexpr int kPinned = 64;                // ints of the pinned block
static_assert(kSpStats + 1 <= kPinned && kCntBusy + kBatch <= kPinned, "the pinned block holds every read-back");
enum { kHNnz = 0, kHLeft = 1 };            // h after sp_finish_matrix: entries of the new current matrix, length of E

// grows a buffer to at least `need` elements, keeping its first `used` ones
template <class T>
void grow_keep(DevBuf<T>& b, size_t used, size_t need, hipStream_t s) {
    if (need <= b.size()) return;
    DevBuf<T> nb(std::max(need, 2 * b.size()));
    if (used) IPXK_HIP(hipMemcpyAsync(nb.get(), b.get(), used * sizeof(T), hipMemcpyDeviceToDevice, s));
    IPXK_HIP(hipStreamSynchronize(s));
    b = std::move(nb);
}

// ---- row-wise copy ------------------------------------------------------------------------------
__global__ void lu_expand_kernel(int dim, const int* __restrict__ Bp, const int* __restrict__ Bi, int* __restrict__ colof,
                                 int* __restrict__ keys, int* __restrict__ pos, int* __restrict__ rc, int* __restrict__ cc,
                                 int* bad) {
    IPXK_GRID_STRIDE(j, dim) {
        cc[j] = Bp[j + 1] - Bp[j];
        for (int p = Bp[j]; p < Bp[j + 1]; p++) {
            const int i = Bi[p];
            if (i < 0 || i >= dim) { *bad = 1; continue; }
            colof[p] = (int)j;
            keys[p] = i;
            pos[p] = p;
            atomicAdd(rc + i, 1);
        }
    }
}
__global__ void lu_rows_kernel(int64_t nb, const int* __restrict__ pos_sorted, const int* __restrict__ colof, int* __restrict__ Rj) {
    IPXK_GRID_STRIDE(q, nb) Rj[q] = colof[pos_sorted[q]];
}

// ---- singleton rounds ---------------------------------------------------------------------------
// While the rounds run, rstage / cstage hold -1 for active rows / columns and the TAG of the round that pivoted
// them otherwise (2 * iteration for a column round, + 1 for a row round); the dense pivot stages are assigned
// afterwards by one sort of (tag, column index | row index): the order inside a round is by index whatever the
// order in which the threads ran.
struct Rounds {
    int dim;
    const int *Bp, *Bi;
    const double* Bx;
    const int *Rp, *Rj, *Rpos;
    int *rstage, *cstage, *rc, *cc;
    double* pivot;
    unsigned char* ckind;
    int *cand, *claim, *pivrow;
    u64 *cand_bits, *claim_abs;
    int* counters;        // [kCntBusy + b]: iteration b of the batch found a pivot
    double abstol, pivottol;
};

__global__ void lu_col_find_kernel(Rounds R) {
    IPXK_GRID_STRIDE(j, R.dim) {
        int cr = -1;
        if (R.cstage[j] == -1 && R.cc[j] == 1) {          // -1: active; -2: a spike (torn), never a round pivot
            for (int p = R.Bp[j]; p < R.Bp[j + 1]; p++) {
                const int i = R.Bi[p];
                if (R.rstage[i] >= 0) continue;
                if (fabs(R.Bx[p]) >= R.abstol) { cr = i; atomicMin(R.claim + i, (int)j); }
                break;
            }
        }
        R.cand[j] = cr;
    }
}
__global__ __launch_bounds__(kBlock) void lu_col_commit_kernel(Rounds R, int tag, int slot) {
    IPXK_GRID_STRIDE(j, R.dim) {
        if (!(R.cand[j] >= 0 && R.claim[R.cand[j]] == (int)j)) continue;
        R.counters[slot] = 1;                      // "this iteration found a pivot" (same value from every writer)
        const int i = R.cand[j];
        for (int p = R.Bp[j]; p < R.Bp[j + 1]; p++)
            if (R.Bi[p] == i) R.pivot[j] = R.Bx[p];
        R.cstage[j] = tag;
        R.rstage[i] = tag;
        R.pivrow[j] = i;
        R.ckind[j] = 1;
        R.claim[i] = INT_MAX;
        // row i leaves the active submatrix: its other columns lose an active entry (none of them is a pivot of
        // this round: such a column would have had two active entries)
        for (int q = R.Rp[i]; q < R.Rp[i + 1]; q++) {
            const int j2 = R.Rj[q];
            if (j2 != (int)j && R.cstage[j2] < 0) atomicSub(R.cc + j2, 1);
        }
    }
}
__global__ void lu_row_find_kernel(Rounds R) {
    IPXK_GRID_STRIDE(i, R.dim) {
        int cj = -1;
        u64 bits = 0;
        if (R.rstage[i] < 0 && R.rc[i] == 1) {
            for (int q = R.Rp[i]; q < R.Rp[i + 1]; q++) {
                const int j = R.Rj[q];
                if (R.cstage[j] != -1) continue;
                const double a = fabs(R.Bx[R.Rpos[q]]);
                double colmax = 0.0;
                for (int p = R.Bp[j]; p < R.Bp[j + 1]; p++)
                    if (R.rstage[R.Bi[p]] < 0) colmax = fmax(colmax, fabs(R.Bx[p]));
                if (a >= R.abstol && a >= R.pivottol * colmax) {
                    cj = j;
                    bits = (u64)__double_as_longlong(a);
                    atomicMax(R.claim_abs + j, bits);
                }
                break;
            }
        }
        R.cand[i] = cj;
        R.cand_bits[i] = bits;
    }
}
__global__ void lu_row_pick_kernel(Rounds R) {
    IPXK_GRID_STRIDE(i, R.dim) {
        const int j = R.cand[i];
        if (j >= 0 && R.cand_bits[i] == R.claim_abs[j]) atomicMin(R.claim + j, (int)i);
    }
}
__global__ __launch_bounds__(kBlock) void lu_row_commit_kernel(Rounds R, int tag, int slot) {
    IPXK_GRID_STRIDE(i, R.dim) {
        if (!(R.cand[i] >= 0 && R.claim[R.cand[i]] == (int)i)) continue;
        R.counters[slot] = 1;
        const int j = R.cand[i];
        R.rstage[i] = tag;
        R.cstage[j] = tag;
        R.pivrow[j] = (int)i;
        R.ckind[j] = 2;
        R.claim[j] = INT_MAX;          // (a loser reads the winner's index or this: neither is its own)
        R.claim_abs[j] = 0;
        // column j leaves: its other active rows lose an active entry (they become entries of L)
        for (int p = R.Bp[j]; p < R.Bp[j + 1]; p++) {
            const int r = R.Bi[p];
            if (r == (int)i) R.pivot[j] = R.Bx[p];
            else if (R.rstage[r] < 0) atomicSub(R.rc + r, 1);
        }
    }
}
// # column / row singletons: block-wise sums of the kinds, one atomic per workgroup
__global__ __launch_bounds__(kBlock) void lu_count_kinds_kernel(int dim, const unsigned char* __restrict__ ckind, int* counters) {
    __shared__ int s1, s2;
    if (threadIdx.x == 0) { s1 = 0; s2 = 0; }
    __syncthreads();
    int n1 = 0, n2 = 0;
    IPXK_GRID_STRIDE(j, dim) { n1 += ckind[j] == 1; n2 += ckind[j] == 2; }
    wave_sum_each(n1, n2);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&s1, n1); atomicAdd(&s2, n2); }
    __syncthreads();
    if (threadIdx.x == 0) { if (s1) atomicAdd(counters + kCntColSing, s1); if (s2) atomicAdd(counters + kCntRowSing, s2); }
}
// tags -> sort keys; after the sort: dense stages
__global__ void lu_stage_keys_kernel(int dim, const int* __restrict__ cstage, const int* __restrict__ pivrow,
                                     u64* __restrict__ keys, int* __restrict__ vals) {
    IPXK_GRID_STRIDE(j, dim) {
        const int tag = cstage[j];
        keys[j] = tag < 0 ? kNoKey : ((u64)(unsigned)tag << 32) | (unsigned)((tag & 1) ? pivrow[j] : (int)j);
        vals[j] = (int)j;
    }
}
__global__ void lu_stage_assign_kernel(int npiv, const int* __restrict__ order, const int* __restrict__ pivrow,
                                       int* __restrict__ cstage, int* __restrict__ rstage) {
    IPXK_GRID_STRIDE(q, npiv) {
        const int j = order[q];
        cstage[j] = (int)q;
        rstage[pivrow[j]] = (int)q;
    }
}

// ---- tearing ------------------------------------------------------------------------------------
// candidates for spikes: active columns by descending number of active entries, then ascending index
__global__ void lu_tear_keys_kernel(int dim, const int* __restrict__ cstage, const int* __restrict__ cc, u64* __restrict__ keys) {
    IPXK_GRID_STRIDE(j, dim)
        keys[j] = cstage[j] == -1 ? ((u64)(0x7fffffffu - (unsigned)cc[j]) << 32) | (unsigned)j : kNoKey;
}
// the first `take` candidates become spikes: they leave the active columns, their active rows lose an entry
__global__ void lu_tear_apply_kernel(Rounds R, const u64* __restrict__ sorted, int take) {
    IPXK_GRID_STRIDE(t, take) {
        const int j = (int)(sorted[t] & 0xffffffffull);
        R.cstage[j] = -2;
        for (int p = R.Bp[j]; p < R.Bp[j + 1]; p++) {
            const int i = R.Bi[p];
            if (R.rstage[i] < 0) atomicSub(R.rc + i, 1);
        }
    }
}
// the entries of L found by the rounds, keyed (stage of the row | stage of the pivot): an entry (r, j) of a row
// singleton column j below its pivot, i.e. r was still active when j was pivoted.  Rows that were never pivoted
// count as stages npiv.. in ascending row order.
__global__ void lu_lentry_keys_kernel(int64_t nb, const int* __restrict__ colof, const int* __restrict__ Bi,
                                      const double* __restrict__ Bx, const unsigned char* __restrict__ ckind,
                                      const int* __restrict__ pivrow, const int* __restrict__ rstage, const int* __restrict__ cstage,
                                      const int* __restrict__ rloc, const double* __restrict__ pivot, int npiv,
                                      u64* __restrict__ key, double* __restrict__ val) {
    IPXK_GRID_STRIDE(p, nb) {
        const int j = colof[p], r = Bi[p];
        key[p] = kNoKey;
        val[p] = 0.0;
        if (ckind[j] != 2 || r == pivrow[j]) continue;
        const int rs = rstage[r] >= 0 ? rstage[r] : npiv + rloc[r];
        if (rs < cstage[j]) continue;                          // pivoted before j: an entry of U
        key[p] = ((u64)(unsigned)rs << 32) | (unsigned)cstage[j];
        val[p] = Bx[p] / pivot[j];
    }
}
// L entries of the rows of each half-round (tag): which launches of the substitution have work
__global__ void lu_tagwork_kernel(int ntags, const ipxint* __restrict__ tagptr, const ipxint* __restrict__ lrp, int* __restrict__ work) {
    IPXK_GRID_STRIDE(t, ntags) work[t] = (int)(lrp[tagptr[t + 1]] - lrp[tagptr[t]]);
}
constexpr int kSpikeBatch = 64;      // spikes per dense block: one lane each
// X[stage of row][lane] = entries of the batch's spikes (X zero before)
// (all spike kernels: blockIdx.y = the batch of 64 spikes within a group of batches that travel together -- they are independent --,
// its block of X `xs` doubles behind the previous one's; kb = # spikes in all)
__global__ void lu_spike_scatter_kernel(int kb, int c0, size_t xs, const int* __restrict__ bcol, const int* __restrict__ Bp,
                                        const int* __restrict__ Bi, const double* __restrict__ Bx, const int* __restrict__ rstage,
                                        const int* __restrict__ rloc, int npiv, double* __restrict__ X) {
    const int l = blockIdx.x;
    c0 += kSpikeBatch * blockIdx.y;
    X += xs * blockIdx.y;
    if (c0 + l >= kb) return;
    const int j = bcol[c0 + l];
    for (int p = Bp[j] + threadIdx.x; p < Bp[j + 1]; p += blockDim.x) {
        const int r = Bi[p];
        const int rs = rstage[r] >= 0 ? rstage[r] : npiv + rloc[r];
        X[(size_t)rs * kSpikeBatch + l] = Bx[p];
    }
}
// rows [s0, s1) of the substitution: x[r] -= l_rj * x[stage of j] for the row's entries of L in pivot order, products
// rounded before they are subtracted (the elimination's own arithmetic); one wavefront per row, one lane per spike
__global__ __launch_bounds__(kBlock) void lu_spike_round_kernel(int s0, int s1, size_t xs, const ipxint* __restrict__ lrp, const u64* __restrict__ lkey,
                                                                const double* __restrict__ lval, double* __restrict__ X) {
    const int lane = threadIdx.x & 63;
    X += xs * blockIdx.y;
    for (int64_t r = (int64_t)s0 + (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); r < s1; r += (int64_t)gridDim.x * (kBlock / 64)) {
        const ipxint e0 = lrp[r], e1 = lrp[r + 1];
        if (e0 == e1) continue;
        double acc = X[(size_t)r * kSpikeBatch + lane];
        for (ipxint e = e0; e < e1; e++) {
            const size_t src = (size_t)(lkey[e] & 0xffffffffull);
            const double prod = lval[e] * X[src * kSpikeBatch + lane];
            acc = acc - prod;
        }
        X[(size_t)r * kSpikeBatch + lane] = acc;
    }
}
// The same for a RUN of consecutive half-rounds [t0, t1) that are small (a few rows each): one workgroup takes them one after the
// other with a barrier in between, instead of one launch per half-round -- thousands of tears leave thousands of half-rounds of
// a handful of rows (a 12 000 x 30 000 LP through the drop-in solver: 2.2 million launches of the kernel above, 37 % of all
// kernel time and more in launch latency).  A row's arithmetic is the same: its entries in pivot order, products rounded first.
constexpr int kSpikeRunThreads = 1024;
__global__ __launch_bounds__(kSpikeRunThreads) void lu_spike_run_kernel(int t0, int t1, size_t xs, const ipxint* __restrict__ tagptr,
                                                                        const ipxint* __restrict__ lrp, const u64* __restrict__ lkey,
                                                                        const double* __restrict__ lval, double* X) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    X += xs * blockIdx.y;
    for (int t = t0; t < t1; t++) {
        const int64_t s0 = tagptr[t], s1 = tagptr[t + 1];
        for (int64_t r = s0 + wave; r < s1; r += kSpikeRunThreads / 64) {
            const ipxint e0 = lrp[r], e1 = lrp[r + 1];
            if (e0 == e1) continue;
            double acc = X[(size_t)r * kSpikeBatch + lane];
            for (ipxint e = e0; e < e1; e++) {
                const size_t src = (size_t)(lkey[e] & 0xffffffffull);
                const double prod = lval[e] * X[src * kSpikeBatch + lane];
                acc = acc - prod;
            }
            X[(size_t)r * kSpikeBatch + lane] = acc;
        }
        __syncthreads();               // the rows of the next half-round read what this one wrote
    }
}
// the batch's part of the dense block: rows that were never pivoted
__global__ void lu_spike_dense_kernel(int kb, int c0, size_t xs, int npiv, const double* __restrict__ X, double* __restrict__ D) {
    c0 += kSpikeBatch * blockIdx.y;
    X += xs * blockIdx.y;
    const int nlanes = min(kSpikeBatch, kb - c0);
    IPXK_GRID_STRIDE(e, (int64_t)kb * nlanes) {
        const int l = (int)(e % nlanes), t = (int)(e / nlanes);
        D[(size_t)(c0 + l) * kb + t] = X[(size_t)(npiv + t) * kSpikeBatch + l];
    }
}
// the batch's entries in pivoted rows (future entries of U): counted, then appended as (bump column, stage, value)
__global__ void lu_spike_count_kernel(int kb, int c0, size_t xs, int npiv, const double* __restrict__ X, int* count) {
    c0 += kSpikeBatch * blockIdx.y;
    X += xs * blockIdx.y;
    const int nlanes = min(kSpikeBatch, kb - c0);
    int mine = 0;
    IPXK_GRID_STRIDE(e, (int64_t)npiv * kSpikeBatch) mine += (int)(e % kSpikeBatch) < nlanes && X[e] != 0.0;
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(count, mine);
}
__global__ void lu_spike_append_kernel(int kb, int c0, size_t xs, int npiv, const double* __restrict__ X, int* cursor,
                                       int* __restrict__ spk_c, int* __restrict__ spk_s, double* __restrict__ spk_v) {
    c0 += kSpikeBatch * blockIdx.y;
    X += xs * blockIdx.y;
    const int nlanes = min(kSpikeBatch, kb - c0);
    IPXK_GRID_STRIDE(e, (int64_t)npiv * kSpikeBatch) {
        const int l = (int)(e % kSpikeBatch);
        const double v = X[e];
        if (l >= nlanes || v == 0.0) continue;
        const int at = atomicAdd(cursor, 1);           // the order is irrelevant: the entries are sorted by key later
        spk_c[at] = c0 + l;
        spk_s[at] = (int)(e / kSpikeBatch);
        spk_v[at] = v;
    }
}

// ---- bump ---------------------------------------------------------------------------------------
__global__ void lu_active_flag_kernel(int dim, const int* __restrict__ stage, int* __restrict__ flag) {
    IPXK_GRID_STRIDE(i, dim) flag[i] = stage[i] < 0 ? 1 : 0;
}
__global__ void lu_compact_kernel(int dim, const int* __restrict__ flag, const int* __restrict__ rank, int* __restrict__ loc,
                                  int* __restrict__ list) {
    IPXK_GRID_STRIDE(i, dim) {
        loc[i] = flag[i] ? rank[i] : -1;
        if (flag[i]) list[rank[i]] = (int)i;
    }
}
__global__ __launch_bounds__(kBlock) void lu_dense_fill_kernel(int kb, const int* __restrict__ bcol, const int* __restrict__ Bp,
                                                               const int* __restrict__ Bi, const double* __restrict__ Bx,
                                                               const int* __restrict__ rloc, double* __restrict__ D) {
    const int lane = threadIdx.x & 63;                            // a wavefront per bump column
    for (int c = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); c < kb; c += gridDim.x * (kBlock / 64)) {
        const int j = bcol[c];
        for (int p = Bp[j] + lane; p < Bp[j + 1]; p += 64) {
            const int r = rloc[Bi[p]];
            if (r >= 0) D[(size_t)c * kb + r] = Bx[p];
        }
    }
}

// ---- elimination rounds ---------------------------------------------------------------------------
// (2c in the header comment.)  The CURRENT matrix of a round is a compact problem of its own: rows and columns renumbered to the
// active ones in ascending order (grow / gcol: their indices in B), every entry active, CSC plus a row-wise index.
struct Sparse {
    int dim;
    const int *Bp, *Bi, *colof;
    const double* Bx;
    const int *Rp, *Rj, *Rpos;
    const int *rc, *cc;
    int *candrow, *cost;
    u64 *key, *rowbest;
    int* stats;           // the slots kSp* above
    double abstol, pivottol;
};
// one candidate per column: among its entries that pass the absolute and the relative threshold, the one in the shortest row
// (ties: larger |entry|, then smaller row); cost = (row count - 1)(column count - 1).  One wavefront per column.
__global__ __launch_bounds__(kBlock) void sp_cand_kernel(Sparse S) {
    __shared__ int s_hist[33], s_min, s_n;
    if (threadIdx.x < 33) s_hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) { s_min = INT_MAX; s_n = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int64_t j = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); j < S.dim; j += (int64_t)gridDim.x * (kBlock / 64)) {
        const int p0 = S.Bp[j], p1 = S.Bp[j + 1];
        double colmax = 0.0;
        for (int p = p0 + lane; p < p1; p += 64) colmax = fmax(colmax, fabs(S.Bx[p]));
        colmax = wave_reduce<FmaxOp, 64>(colmax);
        int bi = INT_MAX, brc = INT_MAX;
        double ba = 0.0;
        const double rel = S.pivottol * colmax;
        for (int p = p0 + lane; p < p1; p += 64) {
            const double a = fabs(S.Bx[p]);
            if (!(a >= S.abstol && a >= rel)) continue;
            const int i = S.Bi[p], r = S.rc[i];
            if (r < brc || (r == brc && (a > ba || (a == ba && i < bi)))) { bi = i; brc = r; ba = a; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int oi = __shfl_xor(bi, d, 64), orc = __shfl_xor(brc, d, 64);
            const double oa = __shfl_xor(ba, d, 64);
            if (oi != INT_MAX && (orc < brc || (orc == brc && (oa > ba || (oa == ba && oi < bi))))) { bi = oi; brc = orc; ba = oa; }
        }
        if (lane) continue;
        S.candrow[j] = bi == INT_MAX ? -1 : bi;
        S.key[j] = kNoKey;
        if (bi == INT_MAX) continue;
        const long long c64 = (long long)(brc - 1) * (long long)(p1 - p0 - 1);
        const int c = (int)(c64 < 0x7fffffffLL ? c64 : 0x7fffffffLL);
        S.cost[j] = c;
        atomicMin(&s_min, c);
        atomicAdd(&s_hist[c == 0 ? 0 : 32 - __clz(c)], 1);
        atomicAdd(&s_n, 1);
    }
    __syncthreads();
    if (threadIdx.x < 33 && s_hist[threadIdx.x]) atomicAdd(S.stats + kSpHist + threadIdx.x, s_hist[threadIdx.x]);
    if (threadIdx.x == 0 && s_n) { atomicMin(S.stats + kSpCheapest, s_min); atomicAdd(S.stats + kSpCandidates, s_n); }
}
// the candidates that cost at most max(4, twice the cheapest) compete, and at least a quarter of all candidates (the smallest
// power of two that admits so many)
__global__ void sp_limit_kernel(int* stats) {
    if (blockIdx.x || threadIdx.x) return;
    const long long ncand = stats[kSpCandidates];
    long long limit = -1;
    if (ncand > 0) {
        limit = 2LL * stats[kSpCheapest] > 4 ? 2LL * stats[kSpCheapest] : 4;
        long long cum = 0;
        for (int b = 0; b <= 32; b++) {
            cum += stats[kSpHist + b];
            if (cum * 4 >= ncand) { const long long q = (1LL << b) - 1; if (q > limit) limit = q; break; }
        }
        if (limit > 0x7fffffffLL) limit = 0x7fffffffLL;
    }
    stats[kSpLimit] = (int)limit;
}
// a row keeps its best candidate (cost, then column index)
__global__ void sp_key_kernel(Sparse S) {
    const int limit = S.stats[kSpLimit];
    IPXK_GRID_STRIDE(j, S.dim) {
        if (S.candrow[j] < 0 || S.cost[j] > limit) continue;
        const u64 k = ((u64)(unsigned)S.cost[j] << 32) | (unsigned)j;
        S.key[j] = k;
        atomicMin(S.rowbest + S.candrow[j], k);
    }
}
// a contender (the best of its row) wins unless a better contender has an entry in its pivot row or its pivot row in this
// column: the winners' pivots form a diagonal block.  nupd: the products a winner sends out (pivot row x pivot column, all pairs).
// One wavefront per column.
__global__ __launch_bounds__(kBlock) void sp_win_kernel(Sparse S, int* __restrict__ winner, int* __restrict__ nupd, int* bad) {
    const int lane = threadIdx.x & 63;
    for (int64_t j = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); j < S.dim; j += (int64_t)gridDim.x * (kBlock / 64)) {
        const u64 k = S.key[j];
        bool win = false;
        int i = -1;
        if (k != kNoKey && S.rowbest[S.candrow[j]] == k) {           // (uniform over the wavefront)
            i = S.candrow[j];
            bool lose = false;
            for (int q = S.Rp[i] + lane; q < S.Rp[i + 1]; q += 64) {
                const int j2 = S.Rj[q];
                if (j2 == (int)j) continue;
                const u64 k2 = S.key[j2];
                if (k2 < k && S.rowbest[S.candrow[j2]] == k2) lose = true;       // (k2 < k implies k2 is a key)
            }
            for (int p = S.Bp[j] + lane; p < S.Bp[j + 1]; p += 64)
                if (S.Bi[p] != i && S.rowbest[S.Bi[p]] < k) lose = true;
            win = __ballot(lose) == 0;
        }
        if (lane) continue;
        winner[j] = win ? 1 : 0;
        int n = 0;
        if (win) {
            const long long n64 = (long long)S.rc[i] * S.cc[j];
            if (n64 > (1LL << 28)) *bad = 1; else n = (int)n64;
            atomicAdd(reinterpret_cast<unsigned long long*>(S.stats + kSpUpdates64), (unsigned long long)n);       // the round's total in 64 bits (the int scan below wraps beyond 2^31)
            atomicAdd(S.stats + kSpWinners, 1);
            atomicAdd(S.stats + kSpLeaving, S.rc[i] + S.cc[j] - 1);       // the entries of the pivot row and column leave the matrix
        }
        nupd[j] = n;
    }
}
constexpr int kSpRowsBySort = 1 << 18;
__global__ void sp_rowkeys_kernel(int64_t nnz, const int* __restrict__ Bi, int* __restrict__ keys, int* __restrict__ pos) {
    IPXK_GRID_STRIDE(p, nnz) { keys[p] = Bi[p]; pos[p] = (int)p; }
}
// the row-wise index of the current matrix.  The order of a row's entries is left to the atomics: nothing depends on it (the
// winners' test is a conjunction over the row, and a winner's updates have distinct positions, so the stable sort puts them in
// the same places whatever the order in which they were written).
__global__ void sp_rowcount_kernel(int64_t nnz, const int* __restrict__ Bi, int* __restrict__ rc) {
    IPXK_GRID_STRIDE(p, nnz) atomicAdd(rc + Bi[p], 1);
}
__global__ void sp_rowfill_kernel(int64_t nnz, const int* __restrict__ Bi, const int* __restrict__ colof, const int* __restrict__ Rp,
                                  int* __restrict__ cursor, int* __restrict__ Rj, int* __restrict__ Rpos) {
    IPXK_GRID_STRIDE(p, nnz) {
        const int i = Bi[p];
        const int at = Rp[i] + atomicAdd(cursor + i, 1);
        Rj[at] = colof[p];
        Rpos[at] = (int)p;
    }
}
struct SparseGlobal {     // where a round's pivots are recorded: the arrays of the singleton rounds, indexed as B is
    int *rstage, *cstage, *pivrow;
    double* pivot;
    unsigned char* ckind;
};
__global__ void sp_commit_kernel(Sparse S, const int* __restrict__ winner, const int* __restrict__ grow, const int* __restrict__ gcol,
                                 int tag, SparseGlobal G, int* __restrict__ rstL, int* __restrict__ cstL, double* __restrict__ pivl) {
    IPXK_GRID_STRIDE(j, S.dim) {
        if (!winner[j]) continue;
        const int i = S.candrow[j];
        double piv = 0.0;
        for (int p = S.Bp[j]; p < S.Bp[j + 1]; p++)
            if (S.Bi[p] == i) piv = S.Bx[p];
        pivl[j] = piv;
        rstL[i] = tag;
        cstL[j] = tag;
        const int gi = grow[i], gj = gcol[j];
        G.rstage[gi] = tag;
        G.cstage[gj] = tag;
        G.pivrow[gj] = gi;
        G.pivot[gj] = piv;
        G.ckind[gj] = 5;
    }
}
// the indices in B of the rows (columns) that stay
__global__ void sp_map_kernel(int n, const int* __restrict__ list, const int* __restrict__ gold, int* __restrict__ gnew) {
    IPXK_GRID_STRIDE(r, n) gnew[r] = gold ? gold[list[r]] : list[r];
}
// the entries of the current matrix: those whose row and column stay are keyed (new column | new row) for the next matrix, the
// others join the list of finished entries with their indices in B and their present values
__global__ void sp_entries_kernel(int64_t nnz, const int* __restrict__ Bi, const int* __restrict__ colof, const double* __restrict__ Bx,
                                  const int* __restrict__ newrow, const int* __restrict__ newcol, const int* __restrict__ grow,
                                  const int* __restrict__ gcol, u64* __restrict__ key, double* __restrict__ val, int* __restrict__ keep,
                                  int* cursor, int* __restrict__ Erow, int* __restrict__ Ecol, double* __restrict__ Eval) {
    IPXK_GRID_STRIDE(p, nnz) {
        const int i = Bi[p], j = colof[p];
        const int nr = newrow[i], nc = newcol[j];
        const bool stays = nr >= 0 && nc >= 0;
        if (keep) keep[p] = stays ? 1 : 0;
        const u64 leaving = __ballot(!stays);                 // one atomic per wavefront (the order in E is irrelevant: the assembly sorts by key)
        if (stays) {
            key[p] = ((u64)(unsigned)nc << 32) | (unsigned)nr;
            val[p] = Bx[p];
        } else {
            key[p] = kNoKey;
            val[p] = 0.0;
            const int lane = threadIdx.x & 63, leader = __ffsll((long long)leaving) - 1;
            int base = 0;
            if (lane == leader) base = atomicAdd(cursor, __popcll(leaving));
            base = __shfl(base, leader, 64);
            const int at = base + __popcll(leaving & ((1ull << lane) - 1));
            Erow[at] = grow ? grow[i] : i;
            Ecol[at] = gcol ? gcol[j] : j;
            Eval[at] = Bx[p];
        }
    }
}
__global__ void sp_carry_kernel(int64_t nnz, const int* __restrict__ keep, const int* __restrict__ pos, const u64* __restrict__ key,
                                const double* __restrict__ val, u64* __restrict__ okey, double* __restrict__ oval) {
    IPXK_GRID_STRIDE(p, nnz) {
        if (!keep[p]) continue;
        okey[pos[p]] = key[p];
        oval[pos[p]] = val[p];
    }
}
// the updates -(a_i'j / pivot) * a_ij' of the winners, behind the entries, winner after winner in ascending order of the column
// (the sort is stable: equal positions are then summed in that order); one thread per product, its winner found in the offsets
__global__ __launch_bounds__(kBlock) void sp_updates_kernel(Sparse S, const int* __restrict__ uoff, int64_t nupd, const double* __restrict__ pivl,
                                                            const int* __restrict__ newrow, const int* __restrict__ newcol, int64_t base,
                                                            u64* __restrict__ key, double* __restrict__ val) {
    IPXK_GRID_STRIDE(t, nupd) {
        int lo = 0, hi = S.dim;                       // the last column j with uoff[j] <= t (it has products: uoff[j + 1] > t)
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (uoff[mid] <= (int)t) lo = mid; else hi = mid;
        }
        const int j = lo, i = S.candrow[j], p0 = S.Bp[j], q0 = S.Rp[i], nq = S.Rp[i + 1] - q0;
        const int u = (int)t - uoff[j];
        const int pi = u / nq, qi = u - pi * nq;
        const int p = p0 + pi, q = q0 + qi;
        const int i2 = S.Bi[p], j2 = S.Rj[q];
        if (i2 == i || j2 == j) { key[base + t] = kNoKey; val[base + t] = 0.0; continue; }
        const double l = S.Bx[p] / pivl[j];
        const double prod = l * S.Bx[S.Rpos[q]];
        key[base + t] = ((u64)(unsigned)newcol[j2] << 32) | (unsigned)newrow[i2];
        val[base + t] = -prod;
    }
}
// equal keys are summed in order; a sum that is exactly zero leaves the pattern
__global__ void sp_combine_kernel(int64_t n, const u64* __restrict__ key, const double* __restrict__ val, int* __restrict__ flag,
                                  double* __restrict__ sum) {
    IPXK_GRID_STRIDE(e, n + 1) {
        int keep = 0;
        if (e < n) {
            const u64 k = key[e];
            if (k != kNoKey && (e == 0 || key[e - 1] != k)) {
                double acc = val[e];
                for (int64_t f = e + 1; f < n && key[f] == k; f++) acc = acc + val[f];
                sum[e] = acc;
                keep = acc != 0.0;
            }
        }
        flag[e] = keep;
    }
}
__global__ void sp_compact_kernel(int64_t n, const u64* __restrict__ key, const int* __restrict__ flag, const int* __restrict__ pos,
                                  const double* __restrict__ sum, int* __restrict__ Bi, int* __restrict__ colof, double* __restrict__ Bx) {
    IPXK_GRID_STRIDE(e, n) {
        if (!flag[e]) continue;
        const int at = pos[e];
        Bi[at] = (int)(key[e] & 0xffffffffull);
        colof[at] = (int)(key[e] >> 32);
        Bx[at] = sum[e];
    }
}
// column pointers from the (sorted) columns of the entries
__global__ void sp_colptr_kernel(int dim, int nnz, const int* __restrict__ colof, int* __restrict__ Bp) {
    IPXK_GRID_STRIDE(j, (int64_t)dim + 1) {
        int lo = 0, hi = nnz;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (colof[mid] < (int)j) lo = mid + 1; else hi = mid;
        }
        Bp[j] = lo;
    }
}
__global__ void sp_colcount_kernel(int dim, const int* __restrict__ Bp, int* __restrict__ cc) {
    IPXK_GRID_STRIDE(j, dim) cc[j] = Bp[j + 1] - Bp[j];
}
// the dense block's columns in ascending order of their number of entries (ties: index)
__global__ void sp_colorder_keys_kernel(int kb, const int* __restrict__ cc, u64* __restrict__ keys) {
    IPXK_GRID_STRIDE(c, kb) keys[c] = ((u64)(unsigned)cc[c] << 32) | (unsigned)c;
}
__global__ void sp_colorder_apply_kernel(int kb, const u64* __restrict__ sorted, const int* __restrict__ gcol, int* __restrict__ bcol,
                                         int* __restrict__ cloc, int* __restrict__ cposl) {
    IPXK_GRID_STRIDE(t, kb) {
        const int c = (int)(sorted[t] & 0xffffffffull);
        bcol[t] = gcol[c];
        cloc[gcol[c]] = (int)t;
        cposl[c] = (int)t;
    }
}
__global__ void sp_dense_fill_kernel(int64_t nnz, int kb, const int* __restrict__ Bi, const int* __restrict__ colof, const double* __restrict__ Bx,
                                     const int* __restrict__ cposl, double* __restrict__ D) {
    IPXK_GRID_STRIDE(p, nnz) D[(size_t)cposl[colof[p]] * kb + Bi[p]] = Bx[p];
}

// stages of the bump's pivots; dependent columns and left-over rows are flagged for the ranking that follows
__global__ void lu_bump_stage_kernel(int kb, int base, const int* __restrict__ step, const int* __restrict__ list,
                                     int* __restrict__ stage, int* __restrict__ flag, unsigned char* kind) {
    IPXK_GRID_STRIDE(x, kb) {
        const int s = step[x];
        flag[x] = s < 0 ? 1 : 0;
        if (s >= 0) {
            stage[list[x]] = base + s;
            if (kind) kind[list[x]] = 3;
        }
    }
}
__global__ void lu_bump_rest_kernel(int kb, int base, const int* __restrict__ flag, const int* __restrict__ rank,
                                    const int* __restrict__ list, int* __restrict__ stage, unsigned char* kind,
                                    ipxint* dependent) {
    IPXK_GRID_STRIDE(x, kb) {
        if (!flag[x]) continue;
        stage[list[x]] = base + rank[x];
        if (kind) kind[list[x]] = 4;
        if (dependent) dependent[rank[x]] = base + rank[x];
    }
}

// ---- assembly -----------------------------------------------------------------------------------
struct Assemble {
    int dim, kb;
    const int *Bp, *Bi, *colof;
    const double* Bx;
    const int *rstage, *cstage, *rloc, *cloc, *brow, *bcol, *bcstep;
    const double *pivot, *D;
    const unsigned char* ckind;
    u64 *lkey, *ukey;
    double *lval, *uval;
    int tearing;           // the bump's columns are spikes: their entries above the dense block come from the substitution
    int shift;             // keys are (stage of the column << shift) | stage of the row, 2^shift > dim: the sorts run over 2 * shift bits
};
__global__ void lu_keys_sparse_kernel(Assemble A, int64_t nb) {
    IPXK_GRID_STRIDE(p, nb) {
        const int j = A.colof[p], i = A.Bi[p];
        if (A.ckind[j] == 4) continue;                          // replaced by a unit column
        if (A.cloc[j] >= 0 && (A.tearing || A.rloc[i] >= 0)) continue;   // bump x bump: from the dense result; a spike: lu_keys_spike_kernel
        const int k = A.cstage[j], s = A.rstage[i];
        const u64 key = ((u64)(unsigned)k << A.shift) | (unsigned)s;
        if (s <= k) { A.ukey[p] = key; A.uval[p] = A.Bx[p]; }
        else { A.lkey[p] = key; A.lval[p] = A.Bx[p] / A.pivot[j]; }
    }
}
__global__ void lu_keys_dense_kernel(Assemble A, int64_t nb) {
    const int kb = A.kb;
    IPXK_GRID_STRIDE(e, (int64_t)kb * kb) {
        const int c = (int)(e / kb), r = (int)(e % kb);
        if (A.bcstep[c] < 0) continue;
        const int k = A.cstage[A.bcol[c]], s = A.rstage[A.brow[r]];
        const double v = A.D[e];
        const u64 key = ((u64)(unsigned)k << A.shift) | (unsigned)s;
        if (s == k) { A.ukey[nb + e] = key; A.uval[nb + e] = v; }
        else if (v != 0.0) {
            if (s < k) { A.ukey[nb + e] = key; A.uval[nb + e] = v; }
            else { A.lkey[nb + e] = key; A.lval[nb + e] = v; }
        }
    }
}
__global__ void lu_keys_spike_kernel(Assemble A, int64_t off, int nspk, const int* __restrict__ spk_c, const int* __restrict__ spk_s,
                                     const double* __restrict__ spk_v) {
    IPXK_GRID_STRIDE(e, nspk) {
        const int c = spk_c[e];
        if (A.bcstep[c] < 0) continue;                          // a dependent spike is replaced by a unit column
        const int k = A.cstage[A.bcol[c]];
        A.ukey[off + e] = ((u64)(unsigned)k << A.shift) | (unsigned)spk_s[e];
        A.uval[off + e] = spk_v[e];
    }
}
__global__ void lu_keys_unit_kernel(Assemble A, int64_t off) {
    IPXK_GRID_STRIDE(j, A.dim) {
        if (A.ckind[j] != 4) continue;
        const int k = A.cstage[j];
        A.ukey[off + j] = ((u64)(unsigned)k << A.shift) | (unsigned)k;
        A.uval[off + j] = 1.0;
    }
}
// column pointers of a factor from its sorted keys: ptr[k] = first key >= (k << shift), k = 0..dim
__global__ void lu_colptr_kernel(int dim, int64_t n, const u64* __restrict__ keys, ipxint* __restrict__ ptr, int shift = 32) {
    IPXK_GRID_STRIDE(k, (int64_t)dim + 1) {
        const u64 want = (u64)k << shift;
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (keys[mid] < want) lo = mid + 1; else hi = mid;
        }
        ptr[k] = lo;
    }
}
__global__ void lu_rowidx_kernel(int64_t nz, const u64* __restrict__ keys, ipxint* __restrict__ idx, int shift = 32) {
    IPXK_GRID_STRIDE(q, nz) idx[q] = (ipxint)(keys[q] & ((1ull << shift) - 1));
}
__global__ void lu_perm_kernel(int dim, const int* __restrict__ stage, ipxint* __restrict__ perm, int* bad) {
    IPXK_GRID_STRIDE(i, dim) {
        const int k = stage[i];
        if (k < 0 || k >= dim) *bad = 1; else perm[k] = i;
    }
}
// compact CSC of B = AI[:, basis] from the structural matrix resident on the device (slack columns: unit)
__global__ void lu_basis_count_kernel(int m, int n, const ipxint* __restrict__ basis, const int* __restrict__ Ap,
                                      int* __restrict__ cnt, int* bad) {
    IPXK_GRID_STRIDE(k, m) {
        const ipxint j = basis[k];
        if (j < 0 || j >= (ipxint)n + m) { *bad = 1; cnt[k] = 0; continue; }
        cnt[k] = j < n ? Ap[j + 1] - Ap[j] : 1;
    }
}
__global__ void lu_basis_fill_kernel(int m, int n, const ipxint* __restrict__ basis, const int* __restrict__ Ap,
                                     const int* __restrict__ Ai, const double* __restrict__ Ax, const int* __restrict__ Bp,
                                     int* __restrict__ Bi, double* __restrict__ Bx) {
    IPXK_GRID_STRIDE(k, m) {
        const ipxint j = basis[k];
        int q = Bp[k];
        if (j < n) {
            for (int p = Ap[j]; p < Ap[j + 1]; p++, q++) { Bi[q] = Ai[p]; Bx[q] = Ax[p]; }
        } else {
            Bi[q] = (int)(j - n);
            Bx[q] = 1.0;
        }
    }
}


// the n rows (columns) whose stage is < 0, in ascending order: list[rank] = index, loc[index] = rank or -1
void compact_active(hipStream_t s, Tmp& T, int n, const int* stage, int* flag, int* rank, int* loc, int* list) {
    const int g = grid_for(n);
    hipLaunchKernelGGL(lu_active_flag_kernel, dim3(g), dim3(kBlock), 0, s, n, stage, flag);
    scan_exclusive(T, flag, rank, (size_t)n, s);
    hipLaunchKernelGGL(lu_compact_kernel, dim3(g), dim3(kBlock), 0, s, n, flag, rank, loc, list);
}

}  // namespace

// The policy of a factorization from the environment: every default beside the reason it has.
LuPolicy lu_read_policy() {
    const auto env_int = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
    const auto env_off = [](const char* name) { const char* e = getenv(name); return e && e[0] == '0'; };
    LuPolicy P;
    P.kb_max = std::max(0, env_int("IPXK_LU_BUMP_MAX", 8192));      // (4096 until round 3: the IPM's bases on random 12 000-row LPs end in bumps of 8000 rows)
    // WHICH way a bump goes (round 5).  A bump of at most sparse_from rows (1024) is factorized densely as it stands.  A larger one
    // is eliminated SPARSELY in rounds (2c) as long as that pays, and only the rest -- a matrix that has become dense, typically a
    // third to a half of an IPM basis' bump -- goes to the dense code: on the bases of the IPM (random LPs, 16 000 rows, bump of
    // 10 700) that is nnz(L+U) 24.6 M and 60 ms where the dense bump as it stands gave 95 M and 330 ms; the sequential minimum-
    // Markowitz elimination of the same bases ends in 22.2 M, so there is no better order to be had.  The
    // rounds end at sparse_min columns; or, once at most rest_max columns are left (what the dense code takes), when the current
    // matrix holds more than dense_at x columns^2 entries, after two slow rounds, or when it has grown beyond fill_max x nnz(B) + 2^20
    // entries.  A bump of more than sparse_first_max rows (131 072: the chains of a 1M-row basis, where a round costs 1 ms and
    // frees a handful of pivots) is TORN first (2b) as until round 4, with the rounds as the fall-back; rounds that give up with
    // more than rest_max columns left start again with tearing.  Only a basis neither way can take is refused.
    //   IPXK_LU_SPARSE=t: tearing first for every bump beyond IPXK_LU_BUMP_MAX, rounds as the fall-back (the policy of round 4);
    //   =1: rounds instead of tearing for those bumps, round 4's end rules; =0: tearing only.
    const char* sparse_env = getenv("IPXK_LU_SPARSE");
    P.sparse_allowed = !(sparse_env && sparse_env[0] == '0');
    P.legacy_rounds = sparse_env && sparse_env[0] == '1';
    P.legacy = sparse_env && (sparse_env[0] == '0' || sparse_env[0] == '1' || sparse_env[0] == 't');
    // The limit decides WHETHER a bump is torn; the spikes themselves may fill the largest dense block the panel kernels take
    // (16 rows per thread: 16384 rows) before tearing gives up -- on the IPM bases of random LPs of 12 000 ... 24 000 rows tearing
    // ends with 8000 ... 11 000 spikes.  (A small limit set for tests binds the spikes too.)
    P.spike_max = P.kb_max > 4 * kPanelThreads ? std::max(P.kb_max, kDenseHardMax) : P.kb_max;
    P.rest_max = P.legacy ? P.kb_max : P.spike_max;
    P.sparse_min = std::max(0, env_int("IPXK_LU_SPARSE_MIN", 512));
    // ... or it fits the dense code and two rounds in a row each eliminate fewer than 1 / 256 (2048) of the columns
    P.slow_den = std::max(0, env_int("IPXK_LU_SPARSE_SLOW_DEN", P.legacy ? 256 : 2048));
    P.fill_max = std::max(0, env_int("IPXK_LU_SPARSE_FILL_MAX", 8));       // ... or the bump has filled in beyond 8 x nnz(B) + 2^20 entries
    P.sparse_from = std::max(0, env_int("IPXK_LU_SPARSE_FROM", P.legacy ? P.kb_max : std::min(P.kb_max, 1024)));
    P.sparse_first_max = std::max(0, env_int("IPXK_LU_SPARSE_FIRST_MAX", 131072));
    const char* density_env = getenv("IPXK_LU_SPARSE_DENSITY");
    P.dense_at = density_env ? atof(density_env) : P.legacy ? 0.0 : 0.2;
    // the batches of 64 spikes are independent: a GROUP of them travels together (one launch per half-round / run for the
    // whole group), as many as IPXK_LU_SPIKE_MEM_MB (4096) of dim x 64 blocks allow
    P.spike_mem_mb = (size_t)std::max(1, env_int("IPXK_LU_SPIKE_MEM_MB", 4096));
    // half-rounds of many rows: a launch over the chip each; runs of small ones: one workgroup per batch and run
    // (IPXK_LU_SPIKE_RUNS=0: a launch per half-round with work, as before)
    P.spike_runs = !env_off("IPXK_LU_SPIKE_RUNS");
    P.two_level = !env_off("IPXK_LU_TWO_LEVEL");      // sub-panels in registers, the trailing matrix once per kPanel columns
    P.panel_w = env_int("IPXK_LU_PANEL_W", 0);
    P.mfma_min = env_int("IPXK_LU_MFMA_MIN", kPanelThreads + 1);
    // the sub-panel's rows of U and its update of the rest of the outer panel in one launch (IPXK_LU_FUSED_SUB=0: two)
    P.fused_sub = !env_off("IPXK_LU_FUSED_SUB");
    const char* look_env = getenv("IPXK_LU_LOOKAHEAD");
    P.lookahead = look_env ? (look_env[0] != '0' ? 1 : 0) : -1;
    // the late update leaves some compute units to the panel kernels of the first stream (a one-workgroup kernel of 1024
    // threads does not get a slot on a chip that a 15 000-workgroup kernel keeps full): IPXK_LU_LOOKAHEAD_FREE_CUS
    P.free_cus = std::max(0, std::min(128, env_int("IPXK_LU_LOOKAHEAD_FREE_CUS", 32)));
    P.spread = getenv("IPXK_LU_LOOKAHEAD_SPREAD") != nullptr;       // (measurement: the free units taken from all eight words of the mask)
    P.xcc0 = std::max(0, std::min(31, env_int("IPXK_LU_LOOKAHEAD_XCC0", 0)));    // (measurement: that many units of XCC 0 only)
    // the outer panel by ONE launch of <= 32 cooperating workgroups (IPXK_LU_COOP=0: the sub-panel launches)
    P.coop = !env_off("IPXK_LU_COOP") && !getenv("IPXK_LU_PANEL_W");
    P.coop_R = env_int("IPXK_LU_COOP_R", 0);
    const char* xcd_env = getenv("IPXK_LU_COOP_XCD");
    P.coop_xcd = xcd_env && xcd_env[0] == '0' ? 0 : xcd_env && xcd_env[0] == '1' ? 1 : -1;
    return P;
}

// workspaces of a factorization, kept from one call to the next (grow-only)
struct LuWork {
    DevBuf<int> colof, keys, pos, keys2, Rpos, Rj, Rp, rstage, cstage, rc, cc, cand, flag, rank, claim, pivrow, counters;
    DevBuf<int> rloc, cloc, brow, bcol;
    DevBuf<u64> cand_bits, claim_abs, skey, skey2, lkey, lkey2, ukey, ukey2;
    DevBuf<double> pivot, lval, lval2, uval, uval2;
    DevBuf<unsigned char> ckind;
    DevBuf<u64> tkey, tkey2;          // tearing: candidate keys
    DevBuf<ipxint> lrp, tagptr;       // tearing: row pointers of the L entries by stage; first stage of each half-round
    DevBuf<int> tagwork, spk_c, spk_s;
    DevBuf<double> X, spk_v;
    DevBuf<int> Bp, Bi, cnt;          // B = AI[:, basis] (ipxk_lu_factorize_basis)
    DevBuf<double> Bx;
    // elimination rounds: the current matrix (two copies, used alternately), its row-wise index, the round's scratch, and the
    // list E of the entries that have left the current matrix (indices in B, value at that time)
    struct Sp {
        DevBuf<int> Bp[2], Bi[2], colof[2], grow[2], gcol[2];
        DevBuf<double> Bx[2];
        DevBuf<int> Rp, Rj, Rpos, rc, cc, k32a, k32b, pos;
        DevBuf<int> candrow, cost, winner, nupd, uoff, rstL, cstL, flag, rank, newrow, newcol, listr, listc, stats, cflag, cpos, cposl, ecur;
        DevBuf<u64> key, rowbest, skey, skey2, ukey, ukey2, okey, okey2;
        DevBuf<double> pivl, sval, sval2, uval, uval2, csum;
        DevBuf<int> Erow, Ecol;
        DevBuf<double> Eval;
    } sp;
    Tmp T;
    int* h = nullptr;                 // pinned: counters read back per batch of rounds
    LuDenseWork dense;                // (last: its events and second stream go before any buffer is freed)
    ~LuWork() { if (h) (void)hipHostFree(h); }
};

struct LuState {
    LuWork work;
    int dim = 0;
    int64_t lnz = 0, unz = 0;
    int ndep = 0;
    int bump_start = 0, bump_size = 0;      // pivot stages [bump_start, bump_start + bump_size) came from the dense bump
    bool valid = false, from_basis = false;
    DevBuf<ipxint> Lp, Li, Up, Ui, rowperm, colperm, dependent, basis;
    DevBuf<double> Lx, Ux;
    // plain CSC of the structural matrix (32-bit), uploaded at the first ipxk_lu_factorize_basis
    DevBuf<int> Ap, Ai;
    DevBuf<double> Ax;
    bool have_A = false;
    // what the resident factorization was computed with, and its statistics: ipxk_lu_factorize hands the factors of EXACTLY the
    // matrix it is given out again instead of computing them a second time (lu_reuse_resident)
    double pivottol_used = 0.0;
    bool strict_used = false;
    ipxk_lu_info last_info{};
    bool view = false;                  // ipxk_lu_get_factors returns colperm_view (the caller's column order) instead of colperm
    DevBuf<ipxint> colperm_view;
    DevBuf<int> reuse_cand, reuse_mark, reuse_sigma, reuse_flag;
    long generation = 0;                // counts the factorizations actually computed in this context
};

void destroy_lu(LuState* S) { delete S; }

static LuState* lu_state(Context* c) {
    if (!c->lu) c->lu = new LuState;
    return c->lu;
}

namespace {
__global__ void sp_stats_init_kernel(int* stats) {
    if (blockIdx.x == 0 && threadIdx.x < kSpStats) stats[threadIdx.x] = threadIdx.x == kSpCheapest ? INT_MAX : 0;
}
struct SparseOut {
    int kb = 0, cur = 0, pivots = 0, rounds = 0;
    int64_t nnz = 0, ne = 0;
};
// sorted (key, value) pairs -> the next current matrix in copy `dst`: equal keys summed in order, exact zeros dropped, column
// pointers, row-wise index, counts.  Reads back the number of entries (and the length of E).
void sp_finish_matrix(hipStream_t s, LuWork& W, const u64* skeys, const double* svals, int64_t n, int dimL, int dst, int64_t* nnz_out, int64_t* ne_out) {
    LuWork::Sp& P = W.sp;
    Tmp& T = W.T;
    int* h = W.h;
    P.cflag.ensure((size_t)n + 1); P.cpos.ensure((size_t)n + 1); P.csum.ensure((size_t)std::max<int64_t>(n, 1));
    hipLaunchKernelGGL(sp_combine_kernel, dim3(grid_for(n + 1)), dim3(kBlock), 0, s, n, skeys, svals, P.cflag.get(), P.csum.get());
    scan_exclusive(T, P.cflag.get(), P.cpos.get(), (size_t)n + 1, s);
    fetch(s, h + kHNnz, P.cpos.get() + n);
    read_back(s, h + kHLeft, P.ecur.get());
    const int64_t nnz = h[kHNnz];
    *nnz_out = nnz;
    *ne_out = h[kHLeft];
    const size_t z1 = (size_t)std::max<int64_t>(nnz, 1), d1 = (size_t)std::max(dimL, 1);
    P.Bi[dst].ensure(z1); P.colof[dst].ensure(z1); P.Bx[dst].ensure(z1); P.Bp[dst].ensure(d1 + 1);
    if (n > 0)
        hipLaunchKernelGGL(sp_compact_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, n, skeys, P.cflag.get(), P.cpos.get(), P.csum.get(),
                           P.Bi[dst].get(), P.colof[dst].get(), P.Bx[dst].get());
    hipLaunchKernelGGL(sp_colptr_kernel, dim3(grid_for(dimL + 1)), dim3(kBlock), 0, s, dimL, (int)nnz, P.colof[dst].get(), P.Bp[dst].get());
    // rows
    P.rc.ensure(d1 + 1); P.cc.ensure(d1); P.Rp.ensure(d1 + 1);
    for (DevBuf<int>* b : {&P.Rpos, &P.Rj}) b->ensure(z1);
    IPXK_HIP(hipMemsetAsync(P.rc.get(), 0, (d1 + 1) * sizeof(int), s));
    if (dimL > 0) hipLaunchKernelGGL(sp_colcount_kernel, dim3(grid_for(dimL)), dim3(kBlock), 0, s, dimL, P.Bp[dst].get(), P.cc.get());
    // the row-wise index: by atomics for small matrices, by a sort for large ones (a row with thousands of entries serializes
    // its atomics).  Nothing depends on the order of a row's entries.
    const bool rows_by_sort = nnz >= (int64_t)kSpRowsBySort;
    if (rows_by_sort) {
        for (DevBuf<int>* b : {&P.k32a, &P.k32b, &P.pos}) b->ensure(z1);
        hipLaunchKernelGGL(sp_rowkeys_kernel, dim3(grid_for(nnz)), dim3(kBlock), 0, s, nnz, P.Bi[dst].get(), P.k32a.get(), P.pos.get());
        sort_pairs(T, P.k32a.get(), P.k32b.get(), P.pos.get(), P.Rpos.get(), (size_t)nnz, bits_for(std::max(dimL, 2)), s);
        hipLaunchKernelGGL(lu_rows_kernel, dim3(grid_for(nnz)), dim3(kBlock), 0, s, nnz, P.Rpos.get(), P.colof[dst].get(), P.Rj.get());
        hipLaunchKernelGGL(sp_colptr_kernel, dim3(grid_for(dimL + 1)), dim3(kBlock), 0, s, dimL, (int)nnz, P.k32b.get(), P.Rp.get());
        hipLaunchKernelGGL(sp_colcount_kernel, dim3(grid_for(dimL)), dim3(kBlock), 0, s, dimL, P.Rp.get(), P.rc.get());
        return;
    }
    if (nnz > 0) hipLaunchKernelGGL(sp_rowcount_kernel, dim3(grid_for(nnz)), dim3(kBlock), 0, s, nnz, P.Bi[dst].get(), P.rc.get());
    scan_exclusive(T, P.rc.get(), P.Rp.get(), d1 + 1, s);
    if (nnz > 0) {
        P.k32a.ensure(d1);
        IPXK_HIP(hipMemsetAsync(P.k32a.get(), 0, d1 * sizeof(int), s));
        hipLaunchKernelGGL(sp_rowfill_kernel, dim3(grid_for(nnz)), dim3(kBlock), 0, s, nnz, P.Bi[dst].get(), P.colof[dst].get(), P.Rp.get(), P.k32a.get(),
                           P.Rj.get(), P.Rpos.get());
    }
}

// One elimination round's choice on the current matrix S (see the kernels): a candidate per column, the cost limit, the winners
// and the offsets of their updates.  The statistics of the round are in W.h on return (and the end of the offsets, see kHUpdatesEnd).
void sp_pick_winners(hipStream_t s, LuWork& W, const Sparse& S) {
    LuWork::Sp& P = W.sp;
    const int dimL = S.dim, gl = grid_for(dimL);
    const size_t l1 = (size_t)dimL;
    hipLaunchKernelGGL(sp_stats_init_kernel, dim3(1), dim3(64), 0, s, P.stats.get());
    hipLaunchKernelGGL(fill_kernel<u64>, dim3(gl), dim3(kBlock), 0, s, (int64_t)dimL, kNoKey, P.rowbest.get());
    hipLaunchKernelGGL(fill_kernel<int>, dim3(gl), dim3(kBlock), 0, s, (int64_t)dimL, -1, P.rstL.get());
    hipLaunchKernelGGL(fill_kernel<int>, dim3(gl), dim3(kBlock), 0, s, (int64_t)dimL, -1, P.cstL.get());
    IPXK_HIP(hipMemsetAsync(P.nupd.get(), 0, (l1 + 1) * sizeof(int), s));
    const int gw = (int)std::min<int64_t>(4096, ((int64_t)dimL + kBlock / 64 - 1) / (kBlock / 64));     // a wavefront per column
    hipLaunchKernelGGL(sp_cand_kernel, dim3(gw), dim3(kBlock), 0, s, S);
    hipLaunchKernelGGL(sp_limit_kernel, dim3(1), dim3(64), 0, s, P.stats.get());
    hipLaunchKernelGGL(sp_key_kernel, dim3(gl), dim3(kBlock), 0, s, S);
    hipLaunchKernelGGL(sp_win_kernel, dim3(gw), dim3(kBlock), 0, s, S, P.winner.get(), P.nupd.get(), P.stats.get() + kSpTooMany);
    scan_exclusive(W.T, P.nupd.get(), P.uoff.get(), l1 + 1, s);
    fetch(s, W.h, P.stats.get(), kSpStats);
    read_back(s, W.h + kHUpdatesEnd, P.uoff.get() + dimL);
}

// The round's elimination: the nwin winners are recorded (tag), the rows and columns that stay are renumbered in order, and the
// next current matrix (copy 1 - cur, dimL - nwin rows) is built from the entries that stay and the nupd updates.
void sp_eliminate(hipStream_t s, LuWork& W, const Sparse& S, const SparseGlobal& G, int cur, int tag, int nwin, int64_t nupd, int64_t* nnz, int64_t* ne) {
    LuWork::Sp& P = W.sp;
    Tmp& T = W.T;
    const int dimL = S.dim, gl = grid_for(dimL), dimN = dimL - nwin, nxt = 1 - cur;
    hipLaunchKernelGGL(sp_commit_kernel, dim3(gl), dim3(kBlock), 0, s, S, P.winner.get(), P.grow[cur].get(), P.gcol[cur].get(), tag, G, P.rstL.get(),
                       P.cstL.get(), P.pivl.get());
    // the rows and columns that stay, renumbered in order
    P.grow[nxt].ensure((size_t)std::max(dimN, 1)); P.gcol[nxt].ensure((size_t)std::max(dimN, 1));
    compact_active(s, T, dimL, P.rstL.get(), P.flag.get(), P.rank.get(), P.newrow.get(), P.listr.get());
    compact_active(s, T, dimL, P.cstL.get(), P.flag.get(), P.rank.get(), P.newcol.get(), P.listc.get());
    if (dimN > 0) {
        hipLaunchKernelGGL(sp_map_kernel, dim3(grid_for(dimN)), dim3(kBlock), 0, s, dimN, P.listr.get(), P.grow[cur].get(), P.grow[nxt].get());
        hipLaunchKernelGGL(sp_map_kernel, dim3(grid_for(dimN)), dim3(kBlock), 0, s, dimN, P.listc.get(), P.gcol[cur].get(), P.gcol[nxt].get());
    }
    // the entries that stay keep their order (the renumbering is monotone): compacted, then merged with the sorted updates
    // (the merge is stable: at equal positions the entry comes first, then the updates in the order of the winners)
    const int64_t nnz0 = *nnz, ne0 = *ne, ncarry = nnz0 - W.h[kSpLeaving], n = ncarry + nupd;
    IPXK_REQUIRE(ncarry >= 0 && n < (int64_t(1) << 31), "LU: the current matrix of an elimination round exceeds 32-bit positions");
    const size_t nz1 = (size_t)std::max<int64_t>(std::max(n, nnz0), 1), nu1 = (size_t)std::max<int64_t>(nupd, 1);
    for (DevBuf<u64>* b : {&P.skey, &P.skey2}) b->ensure(nz1);
    for (DevBuf<double>* b : {&P.sval, &P.sval2}) b->ensure(nz1);
    for (DevBuf<u64>* b : {&P.ukey, &P.ukey2}) b->ensure(nu1);
    for (DevBuf<double>* b : {&P.uval, &P.uval2}) b->ensure(nu1);
    P.cflag.ensure((size_t)nnz0 + 1); P.cpos.ensure((size_t)nnz0 + 1);
    grow_keep(P.Erow, (size_t)ne0, (size_t)(ne0 + nnz0), s);
    grow_keep(P.Ecol, (size_t)ne0, (size_t)(ne0 + nnz0), s);
    grow_keep(P.Eval, (size_t)ne0, (size_t)(ne0 + nnz0), s);
    if (nnz0 > 0) {
        hipLaunchKernelGGL(sp_entries_kernel, dim3(grid_for(nnz0)), dim3(kBlock), 0, s, nnz0, P.Bi[cur].get(), P.colof[cur].get(), P.Bx[cur].get(),
                           P.newrow.get(), P.newcol.get(), P.grow[cur].get(), P.gcol[cur].get(), P.skey.get(), P.sval.get(), P.cflag.get(),
                           P.ecur.get(), P.Erow.get(), P.Ecol.get(), P.Eval.get());
        scan_exclusive(T, P.cflag.get(), P.cpos.get(), (size_t)nnz0, s);
        hipLaunchKernelGGL(sp_carry_kernel, dim3(grid_for(nnz0)), dim3(kBlock), 0, s, nnz0, P.cflag.get(), P.cpos.get(), P.skey.get(), P.sval.get(),
                           P.skey2.get(), P.sval2.get());
    }
    const u64* mkeys = P.skey2.get();
    const double* mvals = P.sval2.get();
    if (nupd > 0) {
        hipLaunchKernelGGL(sp_updates_kernel, dim3(grid_for(nupd)), dim3(kBlock), 0, s, S, P.uoff.get(), nupd, P.pivl.get(), P.newrow.get(),
                           P.newcol.get(), (int64_t)0, P.ukey.get(), P.uval.get());
        sort_pairs(T, P.ukey.get(), P.ukey2.get(), P.uval.get(), P.uval2.get(), (size_t)nupd, 32 + bits_for(std::max(dimN, 2)), s);
        merge_by_key(T, P.skey2.get(), P.ukey2.get(), P.skey.get(), P.sval2.get(), P.uval2.get(), P.sval.get(), (size_t)ncarry, (size_t)nupd, s);
        mkeys = P.skey.get();
        mvals = P.sval.get();
    }
    sp_finish_matrix(s, W, mkeys, mvals, n, dimN, nxt, nnz, ne);
}

// what a factorization is given: B as compact 32-bit CSC on the device, and the tolerances
struct LuInput {
    int dim;
    int64_t nb;
    const int *Bp, *Bi;
    const double* Bx;
    double abstol, pivottol;
};

// 2c. ELIMINATION ROUNDS.  The singleton rounds have stalled with `nact` active rows and columns of B (rstage / cstage < 0).
// Until at most sparse_min are left (or no column has an acceptable pivot), a round picks pivots of low Markowitz cost that
// form a diagonal block, eliminates them at once and builds the next current matrix (see the kernels).  On return the current
// matrix (copy out.cur: out.kb rows, out.nnz entries, local indices = rank among the rows / columns of B that are still
// active) is what the dense code takes over, and W.sp.E* (out.ne entries) replaces B in the assembly.
SparseOut sparse_rounds(hipStream_t s, LuWork& W, const LuInput& B, int nact, const LuPolicy& Pol, int* rounds) {
    LuWork::Sp& P = W.sp;
    Tmp& T = W.T;
    SparseOut out;
    const int dim = B.dim, *h = W.h;
    const int64_t nb = B.nb;
    const size_t d1 = (size_t)std::max(dim, 1);
    // the rounds end at sparse_min columns; the dense code takes at most kb_max; round 5's policy hands a matrix that has become dense to it
    const int sparse_min = std::min(Pol.sparse_min, Pol.kb_max), kb_max = Pol.rest_max, slow_den = Pol.slow_den, fill_max = Pol.fill_max;
    const double dense_at = Pol.dense_at;
    const bool fill_to_dense = !Pol.legacy;
    const bool verbose = getenv("IPXK_VERBOSE") && atoi(getenv("IPXK_VERBOSE")) >= 2;
    const SparseGlobal G{W.rstage.get(), W.cstage.get(), W.pivrow.get(), W.pivot.get(), W.ckind.get()};
    P.stats.ensure(kSpStats); P.ecur.ensure(1);
    IPXK_HIP(hipMemsetAsync(P.ecur.get(), 0, sizeof(int), s));
    IPXK_HIP(hipMemsetAsync(P.stats.get(), 0, kSpStats * sizeof(int), s));
    // the active submatrix of B, renumbered; everything else of B is finished
    W.rloc.ensure(d1); W.cloc.ensure(d1); W.flag.ensure(d1); W.rank.ensure(d1);
    int dimL = nact, cur = 0;
    P.grow[0].ensure((size_t)std::max(dimL, 1)); P.gcol[0].ensure((size_t)std::max(dimL, 1));
    compact_active(s, T, dim, G.rstage, W.flag.get(), W.rank.get(), W.rloc.get(), P.grow[0].get());
    compact_active(s, T, dim, G.cstage, W.flag.get(), W.rank.get(), W.cloc.get(), P.gcol[0].get());
    const size_t nz1 = (size_t)std::max<int64_t>(nb, 1);
    for (DevBuf<u64>* b : {&P.skey, &P.skey2}) b->ensure(nz1);
    for (DevBuf<double>* b : {&P.sval, &P.sval2}) b->ensure(nz1);
    P.Erow.ensure(nz1); P.Ecol.ensure(nz1); P.Eval.ensure(nz1);
    hipLaunchKernelGGL(sp_entries_kernel, dim3(grid_for(nb)), dim3(kBlock), 0, s, nb, B.Bi, W.colof.get(), B.Bx, W.rloc.get(), W.cloc.get(), (const int*)nullptr,
                       (const int*)nullptr, P.skey.get(), P.sval.get(), (int*)nullptr, P.ecur.get(), P.Erow.get(), P.Ecol.get(), P.Eval.get());
    int64_t nnz = 0, ne = 0;
    if (nb > 0) sort_pairs(T, P.skey.get(), P.skey2.get(), P.sval.get(), P.sval2.get(), (size_t)nb, 32 + bits_for(std::max(dimL, 2)), s);
    sp_finish_matrix(s, W, P.skey2.get(), P.sval2.get(), nb, dimL, cur, &nnz, &ne);
    int slow = 0;
    while (dimL > sparse_min) {
        // (the rounds stop early once the current matrix fits the dense code and two rounds in a row have each eliminated fewer
        // than 1 / slow_den of the columns: what is left has no large sets of independent pivots any more)
        if (slow_den > 0 && dimL <= kb_max && slow >= 2) break;
        // ... or once it fits the dense code and holds more than dense_at x dimL^2 entries: a dense matrix in sparse storage
        if (dense_at > 0.0 && dimL <= kb_max && (double)nnz > dense_at * (double)dimL * (double)dimL) break;
        const size_t l1 = (size_t)dimL;
        for (DevBuf<int>* b : {&P.candrow, &P.cost, &P.winner, &P.rstL, &P.cstL, &P.flag, &P.rank, &P.newrow, &P.newcol, &P.listr, &P.listc}) b->ensure(l1);
        P.nupd.ensure(l1 + 1); P.uoff.ensure(l1 + 1); P.key.ensure(l1); P.rowbest.ensure(l1); P.pivl.ensure(l1);
        const Sparse S{dimL, P.Bp[cur].get(), P.Bi[cur].get(), P.colof[cur].get(), P.Bx[cur].get(), P.Rp.get(), P.Rj.get(), P.Rpos.get(), P.rc.get(),
                       P.cc.get(), P.candrow.get(), P.cost.get(), P.key.get(), P.rowbest.get(), P.stats.get(), B.abstol, B.pivottol};
        sp_pick_winners(s, W, S);
        const int nwin = h[kSpWinners];
        const int64_t nupd = (int64_t)(((unsigned long long)(unsigned)h[kSpUpdates64 + 1] << 32) | (unsigned long long)(unsigned)h[kSpUpdates64]);
        if (h[kSpTooMany] || nupd + nnz >= (int64_t(1) << 31)) {
            // more updates than 32-bit positions hold (a round of a matrix that has become dense): the dense code takes what is left if
            // it can (round 5's policy), else the rounds are given up
            if (fill_to_dense && dimL <= kb_max) break;
            throw Error(IPXK_E_UNSUPPORTED, "LU: an elimination round would send out more updates than 32-bit positions hold");
        }
        if (verbose)
            fprintf(stderr, "ipxk: elimination round %d: active %d nnz %lld cheapest %d limit %d candidates %d winners %d updates %lld\n", out.rounds + 1, dimL,
                    (long long)nnz, h[kSpCheapest], h[kSpLimit], h[kSpCandidates], nwin, (long long)nupd);
        if (nwin == 0) break;                      // no column has an acceptable pivot: what is left goes to the dense block
        const int tag = 2 * (*rounds);
        (*rounds)++;
        out.rounds++;
        out.pivots += nwin;
        sp_eliminate(s, W, S, G, cur, tag, nwin, nupd, &nnz, &ne);
        slow = (int64_t)nwin * slow_den < (int64_t)dimL ? slow + 1 : 0;
        cur = 1 - cur;
        dimL -= nwin;
        // bounded work: a bump whose elimination fills in beyond fill_max x nnz(B) (+ 2^20) is refused, and the caller's CPU
        // kernel takes over (measured: such bases take minutes here -- the 1M-row basis of scripts/gpu_maxvol_bench.py with a
        // tightened pivot tolerance: 14 941 rounds, 291 s, 103 x fill)
        // (round 5's policy: room for a current matrix the density rule will end -- dense_at x kb_max^2 entries -- whatever nnz(B) is)
        const int64_t fill_bound = std::max<int64_t>((int64_t)fill_max * nb + (1 << 20), fill_to_dense ? (int64_t)(dense_at * (double)kb_max * (double)kb_max) : 0);
        if (fill_max > 0 && nnz > fill_bound) {
            if (fill_to_dense && dimL <= kb_max) break;             // (round 5: the dense code takes what is left if it can)
            char msg[200];
            snprintf(msg, sizeof msg, "LU: after %d elimination rounds the bump holds %lld entries in %d columns, beyond the bound of the rounds "
                     "(IPXK_LU_SPARSE_FILL_MAX)", out.rounds, (long long)nnz, dimL);
            throw Error(IPXK_E_UNSUPPORTED, msg);
        }
    }
    out.kb = dimL; out.cur = cur; out.nnz = nnz; out.ne = ne;
    return out;
}

// ---- the phases of a factorization --------------------------------------------------------------
// how a factorization is attempted: a basis the first way cannot take starts again the other way
enum class LuAttempt {
    kFirst,                 // the policy decides between tearing and elimination rounds
    kRoundsAfterTearing,    // tearing overflowed (more than spike_max spikes): elimination rounds
    kTearingOnly,           // the elimination rounds gave up: tearing, and no way back
};
// what the phases of one attempt hand on
struct LuRun {
    int rounds = 0;                    // iterations of the singleton / elimination rounds so far (tags 2 r, 2 r + 1)
    bool tearing = false;              // the bump's columns are spikes
    int ntorn = 0;
    bool sparse_done = false;          // elimination rounds ran: sp describes what they left
    SparseOut sp;
    int npiv_sing = 0;                 // all pivots before the dense block
    int kb = 0;                        // rows of the dense block
    int64_t nspk = 0;                  // tearing: entries of the spikes in pivoted rows (future entries of U)
};

// study aid (IPXK_LU_DUMP=dir): the bases of a run as flat files (dim, nnz, Bp, Bi, Bx), every IPXK_LU_DUMP_EVERY-th
void dump_basis(const LuInput& B) {
    const char* dir = getenv("IPXK_LU_DUMP");
    if (!dir) return;
    static int calls = 0, written = 0;
    const int every = getenv("IPXK_LU_DUMP_EVERY") ? std::max(1, atoi(getenv("IPXK_LU_DUMP_EVERY"))) : 1;
    if (!(B.nb > B.dim && calls++ % every == 0 && written < 64)) return;
    std::vector<int> hp((size_t)B.dim + 1), hi((size_t)B.nb);
    std::vector<double> hx((size_t)B.nb);
    IPXK_HIP(hipMemcpy(hp.data(), B.Bp, hp.size() * sizeof(int), hipMemcpyDeviceToHost));
    IPXK_HIP(hipMemcpy(hi.data(), B.Bi, hi.size() * sizeof(int), hipMemcpyDeviceToHost));
    IPXK_HIP(hipMemcpy(hx.data(), B.Bx, hx.size() * sizeof(double), hipMemcpyDeviceToHost));
    char path[512];
    snprintf(path, sizeof path, "%s/basis_%03d.bin", dir, written++);
    if (FILE* f = fopen(path, "wb")) {
        const int64_t head[2] = {B.dim, B.nb};
        fwrite(head, sizeof(int64_t), 2, f);
        fwrite(hp.data(), sizeof(int), hp.size(), f); fwrite(hi.data(), sizeof(int), hi.size(), f); fwrite(hx.data(), sizeof(double), hx.size(), f);
        fclose(f);
    }
}

// The workspaces of the rounds in their initial state, and the row-wise index of B (Rp, Rj, Rpos).
void build_row_index(hipStream_t s, LuWork& W, const LuInput& B) {
    const int dim = B.dim, g = grid_for(dim);
    const int64_t nb = B.nb;
    const size_t d1 = (size_t)std::max(dim, 1), nz1 = (size_t)std::max<int64_t>(nb, 1);
    for (DevBuf<int>* b : {&W.colof, &W.keys, &W.pos, &W.keys2, &W.Rpos, &W.Rj}) b->ensure(nz1);
    for (DevBuf<int>* b : {&W.rstage, &W.cstage, &W.rc, &W.cc, &W.cand, &W.flag, &W.rank, &W.claim, &W.pivrow}) b->ensure(d1);
    W.Rp.ensure(d1 + 1); W.counters.ensure(kCounters);
    W.cand_bits.ensure(d1); W.claim_abs.ensure(d1); W.pivot.ensure(d1); W.ckind.ensure(d1);
    if (!W.h) IPXK_HIP(hipHostMalloc(reinterpret_cast<void**>(&W.h), kPinned * sizeof(int)));
    IPXK_HIP(hipMemsetAsync(W.rc.get(), 0, d1 * sizeof(int), s));
    IPXK_HIP(hipMemsetAsync(W.counters.get(), 0, kCounters * sizeof(int), s));
    IPXK_HIP(hipMemsetAsync(W.claim_abs.get(), 0, d1 * sizeof(u64), s));
    IPXK_HIP(hipMemsetAsync(W.ckind.get(), 0, d1, s));
    IPXK_HIP(hipMemsetAsync(W.pivot.get(), 0, d1 * sizeof(double), s));
    if (dim == 0) return;
    hipLaunchKernelGGL(fill_kernel<int>, dim3(g), dim3(kBlock), 0, s, (int64_t)dim, -1, W.rstage.get());
    hipLaunchKernelGGL(fill_kernel<int>, dim3(g), dim3(kBlock), 0, s, (int64_t)dim, -1, W.cstage.get());
    hipLaunchKernelGGL(fill_kernel<int>, dim3(g), dim3(kBlock), 0, s, (int64_t)dim, INT_MAX, W.claim.get());
    hipLaunchKernelGGL(lu_expand_kernel, dim3(g), dim3(kBlock), 0, s, dim, B.Bp, B.Bi, W.colof.get(), W.keys.get(), W.pos.get(),
                       W.rc.get(), W.cc.get(), W.counters.get() + kCntBadIndex);
    if (nb > 0) {
        sort_pairs(W.T, W.keys.get(), W.keys2.get(), W.pos.get(), W.Rpos.get(), (size_t)nb, bits_for(std::max(dim, 2)), s);
        hipLaunchKernelGGL(lu_rows_kernel, dim3(grid_for(nb)), dim3(kBlock), 0, s, nb, W.Rpos.get(), W.colof.get(), W.Rj.get());
    }
    scan_exclusive(W.T, W.rc.get(), W.Rp.get(), (size_t)dim, s);
    const int nb32 = (int)nb;
    IPXK_HIP(hipMemcpyAsync(W.Rp.get() + dim, &nb32, sizeof(int), hipMemcpyHostToDevice, s));
    IPXK_HIP(hipStreamSynchronize(s));             // nb32 is a stack variable
}

// # column and row singletons so far into h[kCntColSing], h[kCntRowSing]; returns their sum
int count_singletons(hipStream_t s, LuWork& W, int dim) {
    IPXK_HIP(hipMemsetAsync(W.counters.get() + kCntColSing, 0, 2 * sizeof(int), s));
    hipLaunchKernelGGL(lu_count_kinds_kernel, dim3(grid_for(dim)), dim3(kBlock), 0, s, dim, W.ckind.get(), W.counters.get());
    read_back(s, W.h, W.counters.get(), kCntBusy);
    return W.h[kCntColSing] + W.h[kCntRowSing];
}

// ---- 1. singleton rounds.  When they stall with active columns left, the policy decides: done (the bump is small enough to be
// factorized densely as it stands), elimination rounds (2c) on what is left, or `take` more spikes torn off (2b) and on with the
// rounds.  Returns false if this attempt cannot go on: *attempt is then the one to start again with.
bool singleton_rounds(hipStream_t s, LuWork& W, const LuInput& B, const LuPolicy& P, LuAttempt* attempt, LuRun& r) {
    const int dim = B.dim, g = grid_for(dim), *h = W.h;
    const LuAttempt mode = *attempt;
    const size_t d1 = (size_t)std::max(dim, 1);
    const Rounds R{dim, B.Bp, B.Bi, B.Bx, W.Rp.get(), W.Rj.get(), W.Rpos.get(), W.rstage.get(), W.cstage.get(), W.rc.get(), W.cc.get(), W.pivot.get(),
                   W.ckind.get(), W.cand.get(), W.claim.get(), W.pivrow.get(), W.cand_bits.get(), W.claim_abs.get(), W.counters.get(),
                   B.abstol, B.pivottol};
    int tear_width = 1, npiv_at_tear = 0;
    while (dim > 0) {
        IPXK_HIP(hipMemsetAsync(W.counters.get() + kCntBusy, 0, kBatch * sizeof(int), s));
        for (int b = 0; b < kBatch; b++) {
            const int tag = 2 * (r.rounds + b);
            hipLaunchKernelGGL(lu_col_find_kernel, dim3(g), dim3(kBlock), 0, s, R);
            hipLaunchKernelGGL(lu_col_commit_kernel, dim3(g), dim3(kBlock), 0, s, R, tag, kCntBusy + b);
            hipLaunchKernelGGL(lu_row_find_kernel, dim3(g), dim3(kBlock), 0, s, R);
            hipLaunchKernelGGL(lu_row_pick_kernel, dim3(g), dim3(kBlock), 0, s, R);
            hipLaunchKernelGGL(lu_row_commit_kernel, dim3(g), dim3(kBlock), 0, s, R, tag + 1, kCntBusy + b);
        }
        read_back(s, W.h, W.counters.get(), kCntBusy + kBatch);
        if (h[kCntBadIndex]) throw Error(IPXK_E_ARGUMENT, "row index of B out of range");
        int last_busy = -1;
        for (int b = 0; b < kBatch; b++) if (h[kCntBusy + b] > 0) last_busy = b;
        r.rounds += last_busy + 1 < kBatch ? last_busy + 2 : kBatch;      // the iteration that found nothing counts
        if (last_busy == kBatch - 1) continue;
        // the rounds stall: done, or (a bump beyond the dense limit) tear spikes off and go on
        const int npiv = count_singletons(s, W, dim), nact = dim - npiv - r.ntorn;
        if (nact == 0) break;

        const bool rounds_now = !r.tearing && P.sparse_allowed && nact > P.sparse_from &&
                                (mode == LuAttempt::kRoundsAfterTearing || P.legacy_rounds ||
                                 (!P.legacy && mode != LuAttempt::kTearingOnly && nact <= P.sparse_first_max));
        if (rounds_now) {                                               // 2c. elimination rounds down to sparse_min rows
            try {
                r.sp = sparse_rounds(s, W, B, nact, P, &r.rounds);
            } catch (const Error& e) {
                if (P.legacy || mode != LuAttempt::kFirst || e.code != IPXK_E_UNSUPPORTED) throw;
                if (getenv("IPXK_VERBOSE")) fprintf(stderr, "ipxk: LU dim %d: %s: starting again with tearing\n", dim, e.what());
                *attempt = LuAttempt::kTearingOnly;
                return false;
            }
            r.sparse_done = true;
            break;
        }
        if (!r.tearing) {
            if (nact <= (P.legacy ? P.kb_max : std::max(P.kb_max, P.sparse_from))) break;      // small enough: dense as it stands
            r.tearing = true;
        } else {
            tear_width = npiv - npiv_at_tear < 64 ? std::min(2 * tear_width, 1024) : 1;
        }
        const int take = std::min(tear_width, nact);
        W.tkey.ensure(d1); W.tkey2.ensure(d1);
        hipLaunchKernelGGL(lu_tear_keys_kernel, dim3(g), dim3(kBlock), 0, s, dim, W.cstage.get(), W.cc.get(), W.tkey.get());
        sort_keys(W.T, W.tkey.get(), W.tkey2.get(), (size_t)dim, 64, s);
        hipLaunchKernelGGL(lu_tear_apply_kernel, dim3(grid_for(take)), dim3(kBlock), 0, s, R, W.tkey2.get(), take);
        r.ntorn += take;
        npiv_at_tear = npiv;
        if (r.ntorn > P.spike_max && P.sparse_allowed && mode != LuAttempt::kTearingOnly) {
            if (getenv("IPXK_VERBOSE"))
                fprintf(stderr, "ipxk: LU dim %d: %d spikes torn off and %d columns still active: starting again with elimination rounds\n", dim, r.ntorn,
                        nact - take);
            *attempt = LuAttempt::kRoundsAfterTearing;
            return false;
        }
        if (r.ntorn > P.spike_max) {
            char msg[200];
            snprintf(msg, sizeof msg, "LU: %d spikes torn off the bump and %d columns still active: the dense block would exceed %d rows "
                     "(IPXK_LU_BUMP_MAX)", r.ntorn, nact - take, P.spike_max);
            throw Error(IPXK_E_UNSUPPORTED, msg);
        }
    }
    return true;
}

// Dense stages of the pivots found so far: rounds in order, inside a round by index.  Counts them (I, r.npiv_sing).
void number_stages(hipStream_t s, LuWork& W, int dim, LuRun& r, ipxk_lu_info& I) {
    if (dim > 0) count_singletons(s, W, dim);
    I.col_singletons = dim > 0 ? W.h[kCntColSing] : 0;
    I.row_singletons = dim > 0 ? W.h[kCntRowSing] : 0;
    I.sparse_pivots = r.sp.pivots;
    I.sparse_rounds = r.sp.rounds;
    I.rounds = r.rounds;
    r.npiv_sing = (int)(I.col_singletons + I.row_singletons) + r.sp.pivots;
    if (r.npiv_sing == 0) return;
    const size_t d1 = (size_t)std::max(dim, 1);
    W.skey.ensure(d1); W.skey2.ensure(d1);
    hipLaunchKernelGGL(lu_stage_keys_kernel, dim3(grid_for(dim)), dim3(kBlock), 0, s, dim, W.cstage.get(), W.pivrow.get(), W.skey.get(), W.cand.get());
    sort_pairs(W.T, W.skey.get(), W.skey2.get(), W.cand.get(), W.claim.get(), (size_t)dim, 64, s);
    hipLaunchKernelGGL(lu_stage_assign_kernel, dim3(grid_for(r.npiv_sing)), dim3(kBlock), 0, s, r.npiv_sing, W.claim.get(), W.pivrow.get(),
                       W.cstage.get(), W.rstage.get());
}

// ---- 2. the bump: the rows and columns never pivoted (brow / bcol, and rloc / cloc: their places in the bump or -1); r.kb
void gather_bump(hipStream_t s, LuWork& W, int dim, LuRun& r) {
    const size_t d1 = (size_t)std::max(dim, 1);
    W.rloc.ensure(d1); W.cloc.ensure(d1); W.dense.bstep.ensure(2 * kBstepSet);
    r.kb = 0;
    if (dim == 0) return;
    r.kb = dim - r.npiv_sing;
    W.brow.ensure((size_t)std::max(r.kb, 1)); W.bcol.ensure((size_t)std::max(r.kb, 1));
    compact_active(s, W.T, dim, W.rstage.get(), W.flag.get(), W.rank.get(), W.rloc.get(), W.brow.get());
    compact_active(s, W.T, dim, W.cstage.get(), W.flag.get(), W.rank.get(), W.cloc.get(), W.bcol.get());
}

// ---- 2b. the spikes through the row singleton pivots (forward substitution, 64 spikes at a time): their entries in the rows
// never pivoted fill D, those in pivoted rows are listed in W.spk_* (future entries of U); returns the length of that list
int64_t spike_substitution(hipStream_t s, LuWork& W, const LuInput& B, const LuPolicy& P, const LuRun& r) {
    const int dim = B.dim, kb = r.kb, npiv_sing = r.npiv_sing, *h = W.h;
    const int64_t nb = B.nb;
    const size_t d1 = (size_t)std::max(dim, 1), nz1 = (size_t)std::max<int64_t>(nb, 1);
    for (DevBuf<u64>* b : {&W.lkey, &W.lkey2}) b->ensure(nz1);
    for (DevBuf<double>* b : {&W.lval, &W.lval2}) b->ensure(nz1);
    hipLaunchKernelGGL(lu_lentry_keys_kernel, dim3(grid_for(nb)), dim3(kBlock), 0, s, nb, W.colof.get(), B.Bi, B.Bx, W.ckind.get(),
                       W.pivrow.get(), W.rstage.get(), W.cstage.get(), W.rloc.get(), W.pivot.get(), npiv_sing, W.lkey.get(), W.lval.get());
    sort_pairs(W.T, W.lkey.get(), W.lkey2.get(), W.lval.get(), W.lval2.get(), (size_t)nb, 64, s);
    W.lrp.ensure(d1 + 1);
    hipLaunchKernelGGL(lu_colptr_kernel, dim3(grid_for(dim + 1)), dim3(kBlock), 0, s, dim, nb, W.lkey2.get(), W.lrp.get());
    // first stage of every half-round (the stage sort left the tags in W.skey2), and which of them have work
    const int ntags = npiv_sing > 0 ? 2 * r.rounds : 0;
    W.tagptr.ensure((size_t)ntags + 1); W.tagwork.ensure((size_t)ntags);
    hipLaunchKernelGGL(lu_colptr_kernel, dim3(grid_for(ntags + 1)), dim3(kBlock), 0, s, ntags, (int64_t)dim, W.skey2.get(), W.tagptr.get());
    hipLaunchKernelGGL(lu_tagwork_kernel, dim3(grid_for(ntags)), dim3(kBlock), 0, s, ntags, W.tagptr.get(), W.lrp.get(), W.tagwork.get());
    std::vector<ipxint> tagptr((size_t)ntags + 1);
    std::vector<int> tagwork((size_t)ntags);
    IPXK_HIP(hipMemcpyAsync(tagptr.data(), W.tagptr.get(), tagptr.size() * sizeof(ipxint), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipMemcpyAsync(tagwork.data(), W.tagwork.get(), tagwork.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
    // a GROUP of batches travels together (P.spike_mem_mb)
    const int nbatches = (kb + kSpikeBatch - 1) / kSpikeBatch;
    const size_t xs = (size_t)dim * kSpikeBatch;
    const int gmax = (int)std::max<size_t>(1, std::min<size_t>(256, (P.spike_mem_mb << 20) / (xs * sizeof(double))));
    const int gsize = std::min(nbatches, gmax);
    W.X.ensure(xs * gsize);
    int64_t nspk = 0;
    for (int b0 = 0; b0 < nbatches; b0 += gsize) {
        const int G = std::min(gsize, nbatches - b0), c0 = b0 * kSpikeBatch;
        IPXK_HIP(hipMemsetAsync(W.X.get(), 0, xs * G * sizeof(double), s));
        hipLaunchKernelGGL(lu_spike_scatter_kernel, dim3(kSpikeBatch, G), dim3(kBlock), 0, s, kb, c0, xs, W.bcol.get(), B.Bp, B.Bi, B.Bx, W.rstage.get(),
                           W.rloc.get(), npiv_sing, W.X.get());
        auto rows = [&](int64_t s0, int64_t s1) {
            if (s1 <= s0) return;
            const int64_t wgs = std::min<int64_t>(2048, (s1 - s0 + kBlock / 64 - 1) / (kBlock / 64));
            hipLaunchKernelGGL(lu_spike_round_kernel, dim3((unsigned)wgs, G), dim3(kBlock), 0, s, (int)s0, (int)s1, xs, W.lrp.get(),
                               W.lkey2.get(), W.lval2.get(), W.X.get());
        };
        constexpr int kSmallRows = 4 * (kSpikeRunThreads / 64);      // up to four rows per wavefront
        for (int t = 0; t < ntags;) {
            const bool small = P.spike_runs && tagptr[t + 1] - tagptr[t] <= kSmallRows;
            if (!small) {
                if (tagwork[t] > 0) rows(tagptr[t], tagptr[t + 1]);
                t++;
                continue;
            }
            int t1 = t, work = 0;
            while (t1 < ntags && tagptr[t1 + 1] - tagptr[t1] <= kSmallRows) { work += tagwork[t1] > 0; t1++; }
            if (work == 1) {                                     // (a lone half-round with work: the plain launch)
                for (int q = t; q < t1; q++) if (tagwork[q] > 0) rows(tagptr[q], tagptr[q + 1]);
            } else if (work > 1) {
                hipLaunchKernelGGL(lu_spike_run_kernel, dim3(1, G), dim3(kSpikeRunThreads), 0, s, t, t1, xs, W.tagptr.get(), W.lrp.get(),
                                   W.lkey2.get(), W.lval2.get(), W.X.get());
            }
            t = t1;
        }
        rows(npiv_sing, dim);                                   // the rows that were never pivoted
        hipLaunchKernelGGL(lu_spike_dense_kernel, dim3(grid_for((int64_t)kb * kSpikeBatch), G), dim3(kBlock), 0, s, kb, c0, xs, npiv_sing,
                           W.X.get(), W.dense.D.get());
        IPXK_HIP(hipMemsetAsync(W.counters.get() + kCntSpike, 0, sizeof(int), s));
        hipLaunchKernelGGL(lu_spike_count_kernel, dim3(grid_for((int64_t)npiv_sing * kSpikeBatch), G), dim3(kBlock), 0, s, kb, c0, xs, npiv_sing,
                           W.X.get(), W.counters.get() + kCntSpike);
        read_back(s, W.h, W.counters.get(), kCntBusy);
        const int add = h[kCntSpike];
        if (add == 0) continue;
        grow_keep(W.spk_c, (size_t)nspk, (size_t)nspk + add, s);
        grow_keep(W.spk_s, (size_t)nspk, (size_t)nspk + add, s);
        grow_keep(W.spk_v, (size_t)nspk, (size_t)nspk + add, s);
        const int cur = (int)nspk;
        IPXK_HIP(hipMemcpyAsync(W.counters.get() + kCntSpike, &cur, sizeof(int), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(lu_spike_append_kernel, dim3(grid_for((int64_t)npiv_sing * kSpikeBatch), G), dim3(kBlock), 0, s, kb, c0, xs, npiv_sing,
                           W.X.get(), W.counters.get() + kCntSpike, W.spk_c.get(), W.spk_s.get(), W.spk_v.get());
        IPXK_HIP(hipStreamSynchronize(s));                  // `cur` is a stack variable
        nspk += add;
    }
    return nspk;
}

// The dense block D of the bump, ready for lu_dense_factorize: from what the elimination rounds left (columns in ascending
// order of their number of entries), from B as it stands, or from the spikes through the substitution (r.nspk).
void fill_dense_block(hipStream_t s, LuWork& W, const LuInput& B, const LuPolicy& Pol, LuRun& r) {
    const int kb = r.kb;
    LuDenseWork& DW = W.dense;
    if (kb > (r.tearing ? Pol.spike_max : r.sparse_done ? Pol.rest_max : Pol.kb_max)) {
        char msg[160];
        snprintf(msg, sizeof msg, "LU: after the singletons a bump of %d rows remains (limit %d, IPXK_LU_BUMP_MAX)", kb, Pol.kb_max);
        throw Error(IPXK_E_UNSUPPORTED, msg);
    }
    DW.brstep.ensure((size_t)std::max(kb, 1)); DW.bcstep.ensure((size_t)std::max(kb, 1));
    if (kb == 0) return;
    DW.D.ensure((size_t)kb * kb);
    IPXK_HIP(hipMemsetAsync(DW.D.get(), 0, (size_t)kb * kb * sizeof(double), s));
    IPXK_HIP(hipMemsetAsync(DW.bstep.get(), 0, 2 * kBstepSet * sizeof(int), s));
    const int gk = grid_for(kb);
    hipLaunchKernelGGL(fill_kernel<int>, dim3(gk), dim3(kBlock), 0, s, (int64_t)kb, -1, DW.brstep.get());
    hipLaunchKernelGGL(fill_kernel<int>, dim3(gk), dim3(kBlock), 0, s, (int64_t)kb, -1, DW.bcstep.get());
    if (r.sparse_done) {
        // the block's columns in ascending order of their number of entries (ties: index): fewer nonzeros in its factors
        LuWork::Sp& P = W.sp;
        const SparseOut& sp = r.sp;
        IPXK_REQUIRE(sp.kb == kb, "LU: the elimination rounds and the stages disagree about what is left");
        P.okey.ensure((size_t)kb); P.okey2.ensure((size_t)kb); P.cposl.ensure((size_t)kb);
        hipLaunchKernelGGL(sp_colorder_keys_kernel, dim3(gk), dim3(kBlock), 0, s, kb, P.cc.get(), P.okey.get());
        sort_keys(W.T, P.okey.get(), P.okey2.get(), (size_t)kb, 64, s);
        hipLaunchKernelGGL(sp_colorder_apply_kernel, dim3(gk), dim3(kBlock), 0, s, kb, P.okey2.get(), P.gcol[sp.cur].get(), W.bcol.get(), W.cloc.get(),
                           P.cposl.get());
        if (sp.nnz > 0)
            hipLaunchKernelGGL(sp_dense_fill_kernel, dim3(grid_for(sp.nnz)), dim3(kBlock), 0, s, sp.nnz, kb, P.Bi[sp.cur].get(), P.colof[sp.cur].get(),
                               P.Bx[sp.cur].get(), P.cposl.get(), DW.D.get());
    } else if (!r.tearing) {
        hipLaunchKernelGGL(lu_dense_fill_kernel, dim3((kb + kBlock / 64 - 1) / (kBlock / 64)), dim3(kBlock), 0, s, kb, W.bcol.get(), B.Bp, B.Bi, B.Bx,
                           W.rloc.get(), DW.D.get());
    } else {
        r.nspk = spike_substitution(s, W, B, Pol, r);
    }
}

// Stages of the bump: its bpiv pivots, then the dependent columns paired with the left-over rows, both ascending
void number_bump_stages(hipStream_t s, LuWork& W, LuState* S, const LuRun& r, int bpiv) {
    const int kb = r.kb, npiv_sing = r.npiv_sing, gk = grid_for(kb);
    S->dependent.ensure((size_t)std::max(kb - bpiv, 1));
    if (kb == 0) return;
    hipLaunchKernelGGL(lu_bump_stage_kernel, dim3(gk), dim3(kBlock), 0, s, kb, npiv_sing, W.dense.bcstep.get(), W.bcol.get(),
                       W.cstage.get(), W.flag.get(), W.ckind.get());
    scan_exclusive(W.T, W.flag.get(), W.rank.get(), (size_t)kb, s);
    hipLaunchKernelGGL(lu_bump_rest_kernel, dim3(gk), dim3(kBlock), 0, s, kb, npiv_sing + bpiv, W.flag.get(), W.rank.get(),
                       W.bcol.get(), W.cstage.get(), W.ckind.get(), S->dependent.get());
    hipLaunchKernelGGL(lu_bump_stage_kernel, dim3(gk), dim3(kBlock), 0, s, kb, npiv_sing, W.dense.brstep.get(), W.brow.get(),
                       W.rstage.get(), W.flag.get(), (unsigned char*)nullptr);
    scan_exclusive(W.T, W.flag.get(), W.rank.get(), (size_t)kb, s);
    hipLaunchKernelGGL(lu_bump_rest_kernel, dim3(gk), dim3(kBlock), 0, s, kb, npiv_sing + bpiv, W.flag.get(), W.rank.get(),
                       W.brow.get(), W.rstage.get(), (unsigned char*)nullptr, (ipxint*)nullptr);
}

// ---- 3. assembly of L, U and the permutations in S
void assemble(hipStream_t s, LuWork& W, LuState* S, const LuInput& B, const LuRun& r) {
    const int dim = B.dim, kb = r.kb, g = grid_for(dim), *h = W.h;
    const size_t d1 = (size_t)std::max(dim, 1);
    S->rowperm.ensure(d1); S->colperm.ensure(d1);
    S->Lp.ensure(d1 + 1); S->Up.ensure(d1 + 1);
    S->lnz = S->unz = 0;
    if (dim == 0) {
        IPXK_HIP(hipMemsetAsync(S->Lp.get(), 0, sizeof(ipxint), s));
        IPXK_HIP(hipMemsetAsync(S->Up.get(), 0, sizeof(ipxint), s));
        IPXK_HIP(hipStreamSynchronize(s));
        return;
    }
    // the entries outside the dense block: B itself, or (after elimination rounds) the list of the entries that left the
    // current matrix, with the values they had then
    const int64_t kbsq = (int64_t)kb * kb, nb = r.sparse_done ? r.sp.ne : B.nb, nspk = r.nspk;
    const int* asm_row = r.sparse_done ? W.sp.Erow.get() : B.Bi;
    const int* asm_col = r.sparse_done ? W.sp.Ecol.get() : W.colof.get();
    const double* asm_val = r.sparse_done ? W.sp.Eval.get() : B.Bx;
    const int64_t nl = nb + kbsq, nu = nb + kbsq + dim + nspk;
    for (DevBuf<u64>* b : {&W.lkey, &W.lkey2}) b->ensure((size_t)std::max<int64_t>(nl, 1));
    for (DevBuf<u64>* b : {&W.ukey, &W.ukey2}) b->ensure((size_t)nu);
    for (DevBuf<double>* b : {&W.lval, &W.lval2}) b->ensure((size_t)std::max<int64_t>(nl, 1));
    for (DevBuf<double>* b : {&W.uval, &W.uval2}) b->ensure((size_t)nu);
    if (nl > 0) hipLaunchKernelGGL(fill_kernel<u64>, dim3(grid_for(nl)), dim3(kBlock), 0, s, nl, kNoKey, W.lkey.get());
    hipLaunchKernelGGL(fill_kernel<u64>, dim3(grid_for(nu)), dim3(kBlock), 0, s, nu, kNoKey, W.ukey.get());
    const int kshift = bits_for((int64_t)dim + 1);            // 2^kshift > dim
    const Assemble A{dim, kb, B.Bp, asm_row, asm_col, asm_val, W.rstage.get(), W.cstage.get(), W.rloc.get(), W.cloc.get(), W.brow.get(), W.bcol.get(),
                     W.dense.bcstep.get(), W.pivot.get(), W.dense.D.get(), W.ckind.get(), W.lkey.get(), W.ukey.get(), W.lval.get(), W.uval.get(),
                     r.tearing ? 1 : 0, kshift};
    if (nb > 0) hipLaunchKernelGGL(lu_keys_sparse_kernel, dim3(grid_for(nb)), dim3(kBlock), 0, s, A, nb);
    if (kb > 0) hipLaunchKernelGGL(lu_keys_dense_kernel, dim3(grid_for(kbsq)), dim3(kBlock), 0, s, A, nb);
    hipLaunchKernelGGL(lu_keys_unit_kernel, dim3(g), dim3(kBlock), 0, s, A, nb + kbsq);
    if (nspk > 0)
        hipLaunchKernelGGL(lu_keys_spike_kernel, dim3(grid_for(nspk)), dim3(kBlock), 0, s, A, nb + kbsq + dim, (int)nspk,
                           W.spk_c.get(), W.spk_s.get(), W.spk_v.get());
    // (2 * kshift key bits instead of 64: five radix passes instead of eight at 1M rows; the unused slots hold all ones and
    // sort behind every key)
    if (nl > 0) sort_pairs(W.T, W.lkey.get(), W.lkey2.get(), W.lval.get(), W.lval2.get(), (size_t)nl, 2 * kshift, s);
    sort_pairs(W.T, W.ukey.get(), W.ukey2.get(), W.uval.get(), W.uval2.get(), (size_t)nu, 2 * kshift, s);
    hipLaunchKernelGGL(lu_colptr_kernel, dim3(grid_for(dim + 1)), dim3(kBlock), 0, s, dim, nl, W.lkey2.get(), S->Lp.get(), kshift);
    hipLaunchKernelGGL(lu_colptr_kernel, dim3(grid_for(dim + 1)), dim3(kBlock), 0, s, dim, nu, W.ukey2.get(), S->Up.get(), kshift);
    ipxint ends[2] = {0, 0};
    IPXK_HIP(hipMemcpyAsync(&ends[0], S->Lp.get() + dim, sizeof(ipxint), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipMemcpyAsync(&ends[1], S->Up.get() + dim, sizeof(ipxint), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
    const int64_t lnz = ends[0], unz = ends[1];
    S->Li.ensure((size_t)std::max<int64_t>(lnz, 1)); S->Lx.ensure((size_t)std::max<int64_t>(lnz, 1));
    S->Ui.ensure((size_t)std::max<int64_t>(unz, 1)); S->Ux.ensure((size_t)std::max<int64_t>(unz, 1));
    if (lnz > 0) {
        hipLaunchKernelGGL(lu_rowidx_kernel, dim3(grid_for(lnz)), dim3(kBlock), 0, s, lnz, W.lkey2.get(), S->Li.get(), kshift);
        IPXK_HIP(hipMemcpyAsync(S->Lx.get(), W.lval2.get(), (size_t)lnz * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(lu_rowidx_kernel, dim3(grid_for(unz)), dim3(kBlock), 0, s, unz, W.ukey2.get(), S->Ui.get(), kshift);
    IPXK_HIP(hipMemcpyAsync(S->Ux.get(), W.uval2.get(), (size_t)unz * sizeof(double), hipMemcpyDeviceToDevice, s));
    IPXK_HIP(hipMemsetAsync(W.counters.get() + kCntNoStage, 0, sizeof(int), s));
    hipLaunchKernelGGL(lu_perm_kernel, dim3(g), dim3(kBlock), 0, s, dim, W.rstage.get(), S->rowperm.get(), W.counters.get() + kCntNoStage);
    hipLaunchKernelGGL(lu_perm_kernel, dim3(g), dim3(kBlock), 0, s, dim, W.cstage.get(), S->colperm.get(), W.counters.get() + kCntNoStage);
    read_back(s, W.h, W.counters.get(), kCntBusy);               // (and the key buffers are free again)
    if (h[kCntNoStage]) throw Error(IPXK_E_HIP, "LU: a pivot stage is missing");
    S->lnz = lnz; S->unz = unz;
}
// IPXK_VERBOSE: one line per factorization
void report(const LuInput& B, const ipxk_lu_info& I, const LuRun& r) {
    if (!getenv("IPXK_VERBOSE")) return;
    fprintf(stderr, "ipxk: LU dim %d nnz %lld: %lld column + %lld row singletons in %d rounds (%.2f ms), bump %d (%.2f ms, %d dependent), "
            "assembly %.2f ms; nnz(L) %lld nnz(U) %lld; %d sparse pivots in %d elimination rounds, %d spikes\n", B.dim, (long long)B.nb, (long long)I.col_singletons, (long long)I.row_singletons,
            r.rounds, I.seconds_singletons * 1e3, r.kb, I.seconds_bump * 1e3, (int)I.num_dependent, I.seconds_assemble * 1e3, (long long)I.lnz, (long long)I.unz,
            (int)I.sparse_pivots, (int)I.sparse_rounds, (int)I.spikes);
}
}  // namespace

// B as compact 32-bit CSC on the device -> factors in S
static void lu_factorize_device(Context* c, LuState* S, int dim, int64_t nb, const int* Bp, const int* Bi,
                                const double* Bx, double pivottol, bool strict, ipxk_lu_info* info) {
    hipStream_t s = c->stream;
    LuWork& W = S->work;
    const LuPolicy P = lu_read_policy();
    const LuInput B{dim, nb, Bp, Bi, Bx, strict ? 1e-3 : 1e-14, pivottol};      // abstol: kLuDependencyTol (src/ipx_internal.h:26) / BASICLU's default
    S->valid = false;
    S->view = false;
    S->dim = dim;
    dump_basis(B);
    for (LuAttempt attempt = LuAttempt::kFirst;;) {
        ipxk_lu_info I{};
        LuRun r;
        const double t0 = now_s();
        build_row_index(s, W, B);
        if (!singleton_rounds(s, W, B, P, &attempt, r)) continue;      // start again, the other way
        number_stages(s, W, dim, r, I);
        const double t1 = now_s();
        gather_bump(s, W, dim, r);
        I.bump = r.kb;
        I.spikes = r.tearing ? r.ntorn : 0;
        fill_dense_block(s, W, B, P, r);
        const int bpiv = r.kb > 0 ? lu_dense_factorize(s, W.dense, r.kb, B.abstol, P, W.h) : 0;
        const int ndep = r.kb - bpiv;
        I.num_dependent = ndep;
        S->ndep = ndep;
        S->bump_start = r.npiv_sing;
        S->bump_size = bpiv;
        number_bump_stages(s, W, S, r, bpiv);
        const double t2 = now_s();
        assemble(s, W, S, B, r);
        I.lnz = S->lnz; I.unz = S->unz;
        I.seconds_singletons = t1 - t0;
        I.seconds_bump = t2 - t1;
        I.seconds_assemble = now_s() - t2;
        S->valid = true;
        S->pivottol_used = pivottol;
        S->strict_used = strict;
        S->last_info = I;
        S->generation++;
        if (info) *info = I;
        report(B, I, r);
        return;
    }
}
namespace {
// column j of the packed matrix against column cand[j] of [A I] as the context holds it: same length, same rows in the same
// order, same values (bit patterns); every candidate at most once
__global__ void lu_reuse_compare_kernel(int m, int n, const int* __restrict__ cand, const int* __restrict__ Bp, const int* __restrict__ Bi,
                                        const double* __restrict__ Bx, const int* __restrict__ Ap, const int* __restrict__ Ai,
                                        const double* __restrict__ Ax, int* __restrict__ mark, int* __restrict__ flag) {
    IPXK_GRID_STRIDE(j, m) {
        const int col = cand[j];
        const int b = Bp[j], len = Bp[j + 1] - b;
        bool same;
        if (col >= n) {
            same = len == 1 && Bi[b] == col - n && Bx[b] == 1.0;
        } else {
            const int a = Ap[col];
            same = len == Ap[col + 1] - a;
            for (int t = 0; same && t < len; t++)
                same = Bi[b + t] == Ai[a + t] && __double_as_longlong(Bx[b + t]) == __double_as_longlong(Ax[a + t]);
        }
        if (atomicExch(&mark[col], (int)j + 1) != 0) same = false;
        if (!same) *flag = 1;
    }
}
// position k of the resident basis -> the caller's column that holds the same variable
__global__ void lu_reuse_sigma_kernel(int m, const ipxint* __restrict__ basis, const int* __restrict__ mark, int* __restrict__ sigma, int* __restrict__ flag) {
    IPXK_GRID_STRIDE(k, m) {
        const int q = mark[basis[k]];
        if (q == 0) *flag = 1;
        sigma[k] = q - 1;
    }
}
__global__ void lu_reuse_colperm_kernel(int m, const ipxint* __restrict__ colperm, const int* __restrict__ sigma, ipxint* __restrict__ out) {
    IPXK_GRID_STRIDE(t, m) out[t] = sigma[colperm[t]];
}
}  // namespace

// Basis::Load / Basis::Factorize (src/basis.cc:81-156) of the reference's Basis right after Maxvolume on the device ask for the
// factorization of the basis whose factors this context ALREADY holds (ipxk_lu_factorize_basis at the end of ipxk_maxvolume), its
// columns in another order.  If the matrix handed in is exactly that basis -- every column compared entry by entry on the device
// with the column of [A I] its offsets name, the set of columns equal to the resident basis -- and the tolerances are the ones the
// resident factors were computed with, nothing is computed: the factors stay, and ipxk_lu_get_factors returns the column
// permutation in the caller's numbering.  IPXK_LU_REUSE=0 switches this off.
static bool lu_reuse_resident(Context* c, LuState* S, int dim, const ipxint* Bbegin, const ipxint* Bend, const int* dBp, const int* dBi,
                              const double* dBx, double pivottol, bool strict) {
    static const bool off = getenv("IPXK_LU_REUSE") && getenv("IPXK_LU_REUSE")[0] == '0';
    const int64_t m = c->m, n = c->n;
    if (off || !S->valid || !S->from_basis || S->ndep != 0 || dim == 0 || dim != (int)m || S->dim != dim || !c->have_plain) return false;
    if (pivottol != S->pivottol_used || strict != S->strict_used) return false;
    if ((int64_t)c->h_Ap.size() != n + 1) return false;
    const std::vector<ipxint>& Ap = c->h_Ap;
    std::vector<int> cand((size_t)dim);
    for (int j = 0; j < dim; j++) {
        const ipxint b = Bbegin[j], e = Bend[j];
        if (b >= Ap[(size_t)n]) {                        // a slack column of [A I]: one entry, stored behind the structural ones
            const ipxint i = b - Ap[(size_t)n];
            if (i >= m || e != b + 1) return false;
            cand[(size_t)j] = (int)(n + i);
        } else {
            const int64_t col = (std::upper_bound(Ap.begin(), Ap.end(), b) - Ap.begin()) - 1;
            if (col < 0 || col >= n || Ap[(size_t)col] != b || Ap[(size_t)col + 1] != e) return false;
            cand[(size_t)j] = (int)col;
        }
    }
    hipStream_t s = c->stream;
    S->reuse_cand.upload(cand, s);
    S->reuse_mark.ensure((size_t)(n + m)); S->reuse_sigma.ensure((size_t)dim); S->reuse_flag.ensure(1); S->colperm_view.ensure((size_t)dim);
    IPXK_HIP(hipMemsetAsync(S->reuse_mark.get(), 0, (size_t)(n + m) * sizeof(int), s));
    IPXK_HIP(hipMemsetAsync(S->reuse_flag.get(), 0, sizeof(int), s));
    const int g = grid_for(dim);
    hipLaunchKernelGGL(lu_reuse_compare_kernel, dim3(g), dim3(kBlock), 0, s, dim, (int)n, S->reuse_cand.get(), dBp, dBi, dBx, c->pl_Ap.get(),
                       c->pl_Ai.get(), c->pl_Ax.get(), S->reuse_mark.get(), S->reuse_flag.get());
    hipLaunchKernelGGL(lu_reuse_sigma_kernel, dim3(g), dim3(kBlock), 0, s, dim, S->basis.get(), S->reuse_mark.get(), S->reuse_sigma.get(),
                       S->reuse_flag.get());
    int flag = 0;
    IPXK_HIP(hipMemcpyAsync(&flag, S->reuse_flag.get(), sizeof(int), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
    if (flag) return false;
    hipLaunchKernelGGL(lu_reuse_colperm_kernel, dim3(g), dim3(kBlock), 0, s, dim, S->colperm.get(), S->reuse_sigma.get(), S->colperm_view.get());
    S->view = true;
    if (getenv("IPXK_VERBOSE")) fprintf(stderr, "ipxk: LU dim %d: the resident factors of this basis handed out again\n", dim);
    return true;
}

long lu_generation(const Context* c) { return c->lu ? c->lu->generation : 0; }

void lu_invalidate(Context* c) { if (c->lu) c->lu->valid = false; }

bool lu_view(const Context* c, LuView* out) {
    const LuState* S = c->lu;
    if (!S || !S->valid) return false;
    out->dim = S->dim;
    out->ndep = S->ndep;
    out->from_basis = S->from_basis;
    out->bump_start = S->bump_start;
    out->bump_size = S->bump_size;
    out->F = DeviceFactors{S->Lp.get(), S->Li.get(), S->Up.get(), S->Ui.get(), S->Lx.get(), S->Ux.get(), S->lnz, S->unz};
    out->rowperm = S->rowperm.get();
    out->colperm = S->colperm.get();
    out->basis = S->basis.get();
    return true;
}

// the plain CSC copy of the structural matrix that ipxk_lu_factorize_basis keeps on the device
void lu_plain_matrix(const Context* c, const int** Ap, const int** Ai, const double** Ax) {
    const LuState* S = c->lu;
    IPXK_REQUIRE(S && S->have_A, "no resident copy of the matrix (ipxk_lu_factorize_basis)");
    *Ap = c->pl_Ap.get(); *Ai = c->pl_Ai.get(); *Ax = c->pl_Ax.get();
}

void lu_factorize_host(Context* c, int64_t dim64, const ipxint* Bbegin, const ipxint* Bend, const ipxint* Bi,
                       const double* Bx, double pivottol, bool strict, ipxk_lu_info* info) {
    IPXK_REQUIRE(dim64 >= 0 && dim64 < (int64_t(1) << 30), "dimension out of range");
    IPXK_REQUIRE(pivottol > 0.0 && pivottol <= 1.0, "pivottol must lie in (0,1]");
    const int dim = (int)dim64;
    hipStream_t s = c->stream;
    LuState* S = lu_state(c);
    // pack the columns (they are ranges of a larger array on the caller's side, src/basis.cc:122-128)
    std::vector<int> bp((size_t)dim + 1, 0), bi;
    std::vector<double> bx;
    int64_t nb = 0;
    for (int j = 0; j < dim; j++) {
        IPXK_REQUIRE(Bend[j] >= Bbegin[j], "Bend < Bbegin");
        nb += Bend[j] - Bbegin[j];
    }
    IPXK_REQUIRE(nb < (int64_t(1) << 31), "nnz(B) exceeds 32 bits");
    bi.resize((size_t)nb); bx.resize((size_t)nb);
    int64_t q = 0;
    for (int j = 0; j < dim; j++) {
        for (ipxint p = Bbegin[j]; p < Bend[j]; p++, q++) {
            IPXK_REQUIRE(Bi[p] >= 0 && Bi[p] < dim, "row index of B out of range");
            bi[(size_t)q] = (int)Bi[p];
            bx[(size_t)q] = Bx[p];
        }
        bp[(size_t)j + 1] = (int)q;
    }
    DevBuf<int> dBp, dBi;
    DevBuf<double> dBx;
    dBp.upload(bp, s); dBi.upload(bi, s); dBx.upload(bx, s);
    dBi.ensure(1); dBx.ensure(1);
    IPXK_HIP(hipStreamSynchronize(s));
    if (lu_reuse_resident(c, S, dim, Bbegin, Bend, dBp.get(), dBi.get(), dBx.get(), pivottol, strict)) {
        if (info) {
            *info = S->last_info;
            info->seconds_singletons = info->seconds_bump = info->seconds_assemble = 0.0;
            info->reused = 1;
        }
        return;
    }
    S->from_basis = false;
    lu_factorize_device(c, S, dim, nb, dBp.get(), dBi.get(), dBx.get(), pivottol, strict, info);
}

void lu_factorize_basis(Context* c, const ipxint* basis, double pivottol, bool strict, ipxk_lu_info* info) {
    IPXK_REQUIRE(!comm_active(c), kDeviceLuRefusal);
    IPXK_REQUIRE(pivottol > 0.0 && pivottol <= 1.0, "pivottol must lie in (0,1]");
    const int m = (int)c->m, n = (int)c->n;
    hipStream_t s = c->stream;
    LuState* S = lu_state(c);
    IPXK_REQUIRE(c->have_plain, "no resident copy of the matrix");
    S->have_A = true;
    S->basis.upload(basis, (size_t)m, s);
    S->basis.ensure(1);
    const size_t m1 = (size_t)std::max(m, 1);
    LuWork& W = S->work;
    DevBuf<int> &cnt = W.cnt, &dBp = W.Bp, &dBi = W.Bi;
    DevBuf<double>& dBx = W.Bx;
    DevBuf<int> bad(1);
    cnt.ensure(m1); dBp.ensure(m1 + 1);
    Tmp& T = W.T;
    IPXK_HIP(hipMemsetAsync(bad.get(), 0, sizeof(int), s));
    int64_t nb = 0;
    if (m > 0) {
        hipLaunchKernelGGL(lu_basis_count_kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, m, n, S->basis.get(), c->pl_Ap.get(), cnt.get(), bad.get());
        scan_exclusive(T, cnt.get(), dBp.get(), (size_t)m, s);
        int last[2] = {0, 0}, hbad = 0;
        IPXK_HIP(hipMemcpyAsync(&last[0], dBp.get() + m - 1, sizeof(int), hipMemcpyDeviceToHost, s));
        IPXK_HIP(hipMemcpyAsync(&last[1], cnt.get() + m - 1, sizeof(int), hipMemcpyDeviceToHost, s));
        IPXK_HIP(hipMemcpyAsync(&hbad, bad.get(), sizeof(int), hipMemcpyDeviceToHost, s));
        IPXK_HIP(hipStreamSynchronize(s));
        if (hbad) throw Error(IPXK_E_ARGUMENT, "basis entry out of range");
        nb = (int64_t)last[0] + last[1];
        const int nb32 = (int)nb;
        IPXK_HIP(hipMemcpyAsync(dBp.get() + m, &nb32, sizeof(int), hipMemcpyHostToDevice, s));
        dBi.ensure((size_t)std::max<int64_t>(nb, 1)); dBx.ensure((size_t)std::max<int64_t>(nb, 1));
        hipLaunchKernelGGL(lu_basis_fill_kernel, dim3(grid_for(m)), dim3(kBlock), 0, s, m, n, S->basis.get(), c->pl_Ap.get(), c->pl_Ai.get(),
                           c->pl_Ax.get(), dBp.get(), dBi.get(), dBx.get());
        IPXK_HIP(hipStreamSynchronize(s));               // nb32
    } else {
        IPXK_HIP(hipMemsetAsync(dBp.get(), 0, sizeof(int), s));
        dBi.ensure(1); dBx.ensure(1);
    }
    lu_factorize_device(c, S, m, nb, dBp.get(), dBi.get(), dBx.get(), pivottol, strict, info);
    S->from_basis = true;
}

void lu_get_factors(Context* c, ipxint* Lp, ipxint* Li, double* Lx, ipxint* Up, ipxint* Ui, double* Ux,
                    ipxint* rowperm, ipxint* colperm, ipxint* dependent) {
    LuState* S = c->lu;
    IPXK_REQUIRE(S && S->valid, "no LU factorization in this context");
    hipStream_t s = c->stream;
    const size_t dim = (size_t)S->dim;
    if (Lp) S->Lp.download(Lp, dim + 1, s);
    if (Li) S->Li.download(Li, (size_t)S->lnz, s);
    if (Lx) S->Lx.download(Lx, (size_t)S->lnz, s);
    if (Up) S->Up.download(Up, dim + 1, s);
    if (Ui) S->Ui.download(Ui, (size_t)S->unz, s);
    if (Ux) S->Ux.download(Ux, (size_t)S->unz, s);
    if (rowperm) S->rowperm.download(rowperm, dim, s);
    if (colperm) (S->view ? S->colperm_view : S->colperm).download(colperm, dim, s);
    if (dependent) S->dependent.download(dependent, (size_t)S->ndep, s);
    IPXK_HIP(hipStreamSynchronize(s));
}

}  // namespace ipxk
