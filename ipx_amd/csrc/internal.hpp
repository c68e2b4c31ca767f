// Internal declarations shared by the translation units of libipx_kkt_hip.so.
// Nothing here is part of the ABI (see include/ipx_kkt_hip.h).
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ipx_kkt_hip.h"

namespace ipxk {

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

void set_last_error(const std::string& msg);

#define IPXK_HIP(expr)                                                         \
    do {                                                                       \
        hipError_t e_ = (expr);                                                \
        if (e_ != hipSuccess) {                                                \
            char buf_[512];                                                    \
            snprintf(buf_, sizeof buf_, "%s:%d: %s failed: %s", __FILE__,      \
                     __LINE__, #expr, hipGetErrorString(e_));                  \
            throw ::ipxk::Error(e_ == hipErrorOutOfMemory ? IPXK_E_ALLOC       \
                                                          : IPXK_E_HIP, buf_); \
        }                                                                      \
    } while (0)

#define IPXK_REQUIRE(cond, msg)                                                \
    do {                                                                       \
        if (!(cond))                                                           \
            throw ::ipxk::Error(IPXK_E_ARGUMENT, std::string(__func__) + ": " + (msg)); \
    } while (0)

// ---------------------------------------------------------------------------
// host <-> device copies of pageable memory
// ---------------------------------------------------------------------------
// hipMemcpyAsync on pageable memory pins the pages on demand: measured 8-36 ms per call on the
// MI355X box even for a few MB (profiles/, HIP API trace of the host-pointer path).  All copies of
// caller-owned memory therefore go through two pinned staging buffers owned by the library
// (memcpy into pinned memory, DMA from there, double-buffered in 8 MiB chunks).
// On return the host data has been fully consumed (h2d) / is complete (d2h).
void staged_h2d(void* dst_dev, const void* src_host, size_t bytes, hipStream_t s);
void staged_d2h(void* dst_host, const void* src_dev, size_t bytes, hipStream_t s);

// ---------------------------------------------------------------------------
// device memory
// ---------------------------------------------------------------------------
template <class T>
class DevBuf {
public:
    DevBuf() = default;
    explicit DevBuf(size_t n) { resize(n); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { release(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    void resize(size_t n) {
        if (n == n_) return;
        release();
        if (n > 0) IPXK_HIP(hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T)));
        // IPXK_POISON=1 (debugging aid): fresh buffers of doubles hold NaNs, so that a read of something never written shows
        if (n > 0 && std::is_same<T, double>::value) {
            static const bool poison = getenv("IPXK_POISON") != nullptr;
            if (poison) { IPXK_HIP(hipMemset(p_, 0xff, n * sizeof(T))); IPXK_HIP(hipDeviceSynchronize()); }   // (before anybody's stream writes it)
        }
        n_ = n;
    }
    // grow-only variant of resize: keeps the allocation when it is already large enough
    void ensure(size_t n) { if (n > n_) resize(n); }
    void release() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    T* get() const { return p_; }
    size_t size() const { return n_; }
    void upload(const T* host, size_t n, hipStream_t s) {
        if (n > n_) resize(n);
        if (n) staged_h2d(p_, host, n * sizeof(T), s);
    }
    void upload(const std::vector<T>& v, hipStream_t s) { upload(v.data(), v.size(), s); }
    void download(T* host, size_t n, hipStream_t s) const {
        if (n) staged_d2h(host, p_, n * sizeof(T), s);
    }
private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// ---------------------------------------------------------------------------
// "gather matrix": a sparse matrix stored by output row, out[r] = f(sum_p
// x[idx[p]] * val[p]).  The CSC of A is the gather matrix of A' (pass 1 of
// A W A'), the row-wise copy of A is the gather matrix of A (pass 2).
// 32-bit indices on the device (4 B per index in the roofline model).
//
// Layout ("time-tiled, LDS-staged partial rows").  Measured on MI355X
// (profiles/r01_gather_microbench.txt): random 8-byte gathers run at ~190 G/s
// when the gathered vector slice is L2-resident (<= 2 MB) but only 70-98 G/s from
// a 16 / 8 MB vector, while the (idx,val) stream alone runs at 6.6 TB/s.  So the
// entries are re-ordered such that, at any time, every workgroup gathers from the
// same slice of x:
//   * the gathered index space is cut into P "phases" of kSliceElems entries;
//   * G co-resident workgroups each own kBlock*RT consecutive output rows per
//     round (thread t owns RT consecutive rows, accumulators live in registers);
//   * storage is ordered (round, phase, workgroup): in step (q,p,w) workgroup w
//     streams -- with fully coalesced loads -- the entries of its rows whose index
//     falls into phase p, stages the products in LDS and each thread adds its
//     rows' products in storage order.  Per (row, phase) only an 8-bit count is
//     stored (no row pointers).
// Because phases ascend with the index, a row is still summed in ascending index
// order, i.e. in the reference's order (bit-exact row sums).
// Rows with more than kMaxRowLen entries ("long rows": dense columns) are cut into
// segments of kLongSeg entries that separate workgroups sum into `long_partials`,
// combined in segment order by a fix-up kernel (deterministic, atomic-free).
// ---------------------------------------------------------------------------
constexpr int kBlock = 256;        // threads per workgroup (4 waves)
constexpr int kChunkNnz = 1024;    // products staged in LDS at a time (4 per thread)
constexpr int kMaxRowLen = 255;    // longer rows take the long-row path
constexpr int kLongSeg = 2048;     // nonzeros per segment of a long row
constexpr int kMaxWorkgroups = 1024; // 4 per CU: all co-resident (16 waves/CU)
constexpr int kMaxPartials = 2048; // upper bound on grid size of reducing kernels
constexpr int kMaxRT = 8;          // rows per thread per round

// grid of a grid-stride kernel over n entries: one workgroup per kBlock entries, at least one, at most cap.  The cap is part
// of a result wherever the workgroups write partials of a two-stage sum: a call site keeps the one it has.
inline int grid_for(int64_t n, int cap = 4096) {
    int64_t g = (n + kBlock - 1) / kBlock;
    if (g < 1) g = 1;
    return (int)(g < cap ? g : cap);
}
inline int vec_grid(int64_t len) { return grid_for(len, 1024); }

struct GatherView {                // passed to kernels by value
    int nrows, ncols;
    int P, G, RT, Q;               // phases, workgroups, rows/thread, rounds
    int RWrows;                    // rows owned by a workgroup per round (<= kBlock*RT)
    const int* step_ptr;           // [Q*P*G+1] first entry of each step
    // per-workgroup chunk table: the non-empty steps of (round q, workgroup w) cut into
    // chunks of at most kChunkNnz entries, in phase order
    const int* wg_chunk_ptr;       // [Q*G+1]
    const int* chunk_start;        // first entry of the chunk
    const int* chunk_info;         // # entries | (first chunk of its step) << 30
    const int* chunk_step;         // step index (addresses the counts)
    const unsigned char* counts;   // [Q*P*G*kBlock*RT] entries per (row, phase)
    const int* idx;                // [nnz_short] gathered index
    const double* val;             // [nnz_short]
    const unsigned char* row_long; // [nrows] 1 for long rows, nullptr if there are none
    // long rows
    int nseg;                      // # segments (= workgroups of the long kernel)
    const int* seg_p0;             // [nseg] first entry in lidx/lval
    const int* seg_p1;
    const int* lidx;
    const double* lval;
    int nlong;                     // # long rows
    const int* long_row;           // [nlong] row index
    const int* long_slot;          // [nlong+1] segment range of each long row
    double* long_partials;         // [nseg]
    unsigned long long* stamps;    // tuning aid: wall clock at the start of each step (or nullptr)
    int masked;                    // val / lval are masked copies: entries with value zero are not gathered
};

// XCD-sliced tile layout (alternative to the phased layout for large gathered vectors).  The
// columns are cut into `nslices` contiguous slices of at most ~2 MiB of x, the rows into blocks of
// kSlicedRows.  Tile (rb, s) holds the entries of row block rb whose column lies in slice s, row by
// row in storage order; it is processed by workgroup rb*nslices + s, which under the round-robin
// workgroup -> XCD dispatch of gfx950 runs on XCD (rb*nslices + s) % 8: an XCD only ever gathers
// from the slice(s) congruent to its index, which therefore stay resident in its 4 MiB L2 no
// matter how far workgroups drift apart -- x is fetched from HBM about once instead of once per
// XCD.  (Placement affects speed only; the result does not depend on it.)  A tile writes one
// partial sum per row; a second streaming kernel adds the slices' partials in slice order and
// applies the epilogue.  Within a slice a row is summed in storage order, so results differ from
// the phased layout only by the association across slices (~1 ulp).
constexpr int kSlicedRows = 1024;      // rows per tile: 4 per thread, or 2 / 1 when tiles would not fit
constexpr int kSlicedMaxTile = 7680;   // entries per tile that fit the LDS staging buffer (62 KB)

struct SlicedView {
    int nrows, nrows_pad, nslices, nrb;
    int R;                             // rows per tile (kBlock * 1, 2 or 4)
    const unsigned* tile_ptr;          // [nrb*nslices + 1] first entry of each tile
    const unsigned char* cnt;          // [nrb*nslices][R] entries per row of the tile
    const int* idx;
    const double* val;
    double* partial;                   // [nslices][nrows_pad]
    const unsigned char* row_long;     // [nrows] 1 for long rows (handled by the long-row kernels), or nullptr
    int masked;                        // val is a masked copy: entries with value zero are not gathered
};

struct SlicedMatrix {
    bool built = false;
    int nslices = 0, nrb = 0, nrows_pad = 0, max_tile = 0, R = kSlicedRows;
    double dominant_fraction = 1.0;    // share of the entries that lie in their row block's fullest slice
    DevBuf<unsigned> tile_ptr;
    DevBuf<unsigned char> cnt;
    DevBuf<int> idx;
    DevBuf<double> val, partial;
};

// Sorted fused tiles: the gathers of a tile issued in ADDRESS order, for matrices whose gathers have locality.
// Measured (profiles/r03_gather_sorted_microbench.txt): random 8-byte gathers from an L2-resident slice cost
// ~41 us per 16M for issue + ~48 us per 16M L1->L2 line requests; lanes of one instruction (and consecutive
// instructions of a CU) that fall on the same 128-byte line share a request, so a tile whose entries are sorted by
// gathered index needs only as many requests as it touches lines: 0.63 of its entries when it holds as many
// entries as its window has lines (72 instead of 88 us), 0.43 at two entries per line (60 us); a banded tile touches
// a few hundred lines with thousands of entries, so almost all its gathers share requests.  Layout:
//   * one slice = all of x; tile t holds the entries of row block t (RB = 256 * RPT rows, as many as give the chip
//     1024 tiles; at most kSortedMaxSub entries) SORTED by gathered index;
//   * an entry is one 32-bit word (slot << 18 | index - `xmin`, the tile's smallest index: the tile's window must span
//     less than 2^18 entries) + its value: slot = the place of the entry when the tile's entries are listed row by
//     row in storage order -- the product goes to that LDS slot, batch after batch without a barrier in between, and
//     after one barrier every thread sums its RPT consecutive rows from consecutive slots;
//   * the thread starts each row from the epilogue's initial value, adds the row's products in storage order and
//     applies the epilogue itself -- bit-identical to the phased and fused layouts; no partial vectors, no combine.
constexpr int kSortedThreads = 256;
constexpr int kSortedMaxSub = 8192;    // entries per tile: 13 bits of slot
constexpr int kSortedOffBits = 18;     // index inside a tile's window (accumulated tiles: a slice of at most 2 MiB of x)
struct SortedView {
    int nrows, nrows_pad, nrb, RB;
    const int* xmin;                   // [nrb] smallest gathered index of the tile
    const unsigned char* row_long;     // rows left to the long-row kernels, or nullptr
    const unsigned* sub_ptr;           // [nrb + 1] first entry of each tile
    const unsigned char* cnt;          // [nrb][RB] entries per row of the tile
    const unsigned* pack;
    const double* val;
};
struct SortedMatrix {
    bool built = false;
    int nrb = 0, RB = 0, nrows_pad = 0, max_sub = 0;
    DevBuf<unsigned> sub_ptr, pack;
    DevBuf<unsigned char> cnt;
    DevBuf<double> val;
    DevBuf<int> xmin;
};

// Accumulated tiles (round 4; the headline's layout): the sliced layout's slices with the ROW SUMS of a row block kept
// in LDS.  Measured first (scripts/bench_ldsacc.hip, profiles/r04_ldsacc_microbench.txt): what the sorted sub-tiles pay
// for staging every product in an LDS slot (a byte count per row and sub-tile, a scan, a row-by-row sum phase, running
// sums in registers that cap the row block at 8192 rows) costs more than the gathers; with nothing but RB doubles of
// LDS per workgroup the row block grows to 16384 rows, a tile holds two entries per 128-byte line of its slice, and
// the sum phase disappears:
//   * tile (rb, s) = the entries of RB rows whose gathered index lies in slice s, in ascending order of the gathered
//     ADDRESS over the whole slice (ties in storage order), cut into BATCHES of at most kAccBatch entries;
//   * a batch holds at most ONE entry of a row: walking the entries in address order, an entry whose row already has
//     one in the current batch waits for the next batch (it goes first there), and a batch is closed when it is full
//     or nothing else is left -- so the ds_add_f64 of a batch hit distinct addresses, one workgroup barrier separates
//     two batches, and a row's products are added in ascending address order whatever the thread timing:
//     deterministic, and equal to the storage order (hence to the sliced layout's partial sums, bit for bit) when the
//     rows are stored with ascending indices, as the reference's Transpose and its sorted CSC give them;
//   * an entry is one 32-bit word (row in block << 18 | index - first index of the slice) + its value; batch q of
//     tile t is entries [bptr[tb[t] + q], bptr[tb[t] + q + 1]);
//   * partial vectors and the combine kernel are the sliced layout's (folding the partials into the last workgroup of
//     a row block to finish measured SLOWER than the combine launch: 109-145 against 95-101 us per pass);
//   * the persistent kernel walks STEPS, not batches: a step is a run of consecutive batches of one tile that is streamed
//     and gathered as one batch and whose adds run batch after batch with a barrier in between.  Per tile, left to right,
//     a step takes batches while their total is at most kAccBatch entries and it holds at most kAccStepBatches of them
//     (so a full batch stays alone, and a tile's short tail batches share one turn of the pipeline).  Step i of tile t is
//     record tile_step[t] + i of `steps`: {first entry, cut 1, cut 2, cut 3}; its end is the next record's first entry
//     (the last record is a sentinel at nnz), unused cuts equal the end.  A tile without entries has no record.
//     acc_build_steps (layout_device.hip) derives the table from tile_batch / bptr for both builders;
//     IPXK_ACC_STEPS=0 makes every batch a step of its own.
constexpr int kAccThreads = 512;
constexpr int kAccPerThread = 4;
constexpr int kAccBatch = kAccThreads * kAccPerThread;     // 2048 entries between two barriers
constexpr int kAccMaxRows = 16384;                         // 128 KB of row sums; 14 bits of row in the entry word
constexpr int kAccStepBatches = 4;                         // batches a step of the persistent kernel holds at most
//   * the WIDE stream (IPXK_ACC_WIDE=0: not built; the sliced form only): a copy of the entries that the persistent kernel
//     reads with three 16-byte loads per thread and step instead of four 4-byte and four 8-byte ones.  Derived from pack /
//     val / steps by acc_build_steps, which are unchanged.  A step of ne entries is taken by Tp = acc_wide_threads(ne)
//     threads (whole wavefronts; 512 for a full batch, 0 for none); thread t < Tp owns the sorted positions u Tp + t,
//     u = 0..3 -- for a full batch the entries it always had, and in every step four entries that lie Tp apart, so that
//     the lanes of a gather instruction still walk neighbouring addresses.  The step occupies 3 Tp units of 16 bytes from
//     wide_start[step]: Tp units with each thread's four entry words, Tp with its values u = 0, 1, Tp with its values
//     u = 2, 3 (a wavefront's load is one aligned KiB).  Positions >= ne hold word 0 and value 0.0 and are never added.
//     wide_start has one entry per step record (the sentinel's: the total).  Only a tile's last step is short: at C3
//     0.4 % more bytes than pack + val, and as much device memory again as those two (C3: 193 MB per gather matrix).
__host__ __device__ inline int acc_wide_threads(int ne) { return ne >= kAccBatch ? kAccThreads : ((ne + 3) / 4 + 63) & ~63; }
//   * the HEAD tables (built only with IPXK_ACC_HEAD=1 -- they gain nothing measurable, profiles/acc_cold_start.txt; the sliced form only): what a workgroup of the persistent kernel needs before
//     its first add, at addresses it can form from its arguments, blockIdx.x and threadIdx.x alone -- one round trip through the
//     caches that the kernel boundary has emptied instead of three dependent ones (tile_step -> steps / wide_start -> wide).
//     Derived by acc_build_steps for the launch grid head_grid = min(acc_persist_grid(nslices), # tiles); a launch on any other
//     grid does not use them.
//     head: kAccHeadWords (64) words per workgroup w < head_grid.  Words 0-47: the records of the first kAccHeadSteps (6) steps of
//     the workgroup's walk over tiles w, w + head_grid, ..., 8 words each: {e0, e1, c1, c2, c3, w0, tile, 0}; tile = -1 past
//     the workgroup's last tile, an empty tile gives its one empty step (all zeros but the tile).  Words 48-51: the walker's
//     state after those steps {tile, step in the tile, first step record of the tile, its steps}.  The rest is zero.
//     head_wide (only with the wide stream): for workgroup w, step d = 0, 1, 2 of its walk, plane p = 0, 1, 2 and thread
//     t < 512 the 16-byte unit ((w 3 + d) 3 + p) 512 + t is the unit thread t loads for that step and plane from the wide
//     stream, wide[w0 + p Tp + min(t, Tp - 1)] (an empty step: unit 0 in every plane); zeros where the workgroup has no
//     step d.  72 KB per workgroup (C3: 19 MB per gather matrix).
constexpr int kAccHeadWords = 64;
constexpr int kAccHeadSteps = 6;                           // the step records a workgroup holds ahead (the kernel's NE)
constexpr int kAccHeadStreams = 3;                         // the steps whose stream loads the kernel's prologue issues
//   * FUSED form (one slice = all of x, for matrices whose gathers have locality; round 4): a tile is a row block of RB rows
//     (as many as give every CU two tiles), the gathered index is stored relative to the tile's smallest one (`xmin`; the
//     tile's window of x must span less than 2^18 entries), the row sums start from the epilogue's initial value and the
//     tile kernel applies the epilogue itself: no partial vectors, no combine launch.  Rows must be stored with ascending
//     indices (then a row is summed in storage order: bit-identical to the phased, fused and sorted fused layouts, so the
//     timing at ipxk_create may choose among them).
struct AccView {
    int nrows, nrows_pad, nslices, nrb, RB, slice_elems;
    int xlen;                          // elements of the gathered vector (the last slice may be short); 0: not known
    int head_grid;                     // the launch grid the head tables are for
    const unsigned* head;              // [head_grid][kAccHeadWords]; nullptr: no head tables
    const uint4* head_wide;            // [head_grid][3][3][kAccThreads]; nullptr: no wide stream
    const int* xmin;                   // FUSED: [nrb] smallest gathered index of the tile; else nullptr
    const unsigned* tile_batch;        // [nrb*nslices + 1] first batch of each tile
    const unsigned* bptr;              // [# batches + 1] first entry of each batch
    const unsigned* tile_step;         // [# tiles + 1] first step of each tile
    const uint4* steps;                // [# steps + 1] {first entry, three cuts} of each step
    const unsigned* pack;
    const double* val;
    const unsigned* wide_start;        // [# steps + 1] first 16-byte unit of each step in `wide`; nullptr: no wide stream
    const uint4* wide;                 // [wide_start[# steps]] (the layout: above)
    double* partial;                  // [nslices][nrows_pad]
};
struct AccMatrix {
    bool built = false;
    int nslices = 0, nrb = 0, RB = 0, nrows_pad = 0, slice_elems = 0;
    int64_t nbatches = 0, deferred = 0, nsteps = 0, wide_units = 0;
    int xlen = 0;                      // elements of the gathered vector
    int head_grid = 0;                 // the grid the head tables are built for; 0: none
    DevBuf<unsigned> tile_batch, bptr, pack, tile_step, wide_start, head;
    DevBuf<uint4> steps, wide, head_wide;
    // the view's fields every accumulated form shares (spmv.hip, nmatrix.hip)
    void fill_view(AccView& V, int nrows) const;
    DevBuf<double> val, partial;
    bool fused = false;                // the FUSED form
    DevBuf<int> xmin;
};
// (the fused form has no partial vectors, step tables' head or wide stream, the sliced one no xmin: their buffers are empty, the pointers null)
inline void AccMatrix::fill_view(AccView& V, int nrows) const {
    V.nrows = nrows; V.nrows_pad = nrows_pad; V.nslices = nslices; V.nrb = nrb; V.RB = RB; V.slice_elems = slice_elems;
    V.xlen = xlen; V.head_grid = head_grid; V.head = head.get(); V.head_wide = head_wide.get();
    V.xmin = xmin.get();
    V.tile_batch = tile_batch.get(); V.bptr = bptr.get(); V.pack = pack.get(); V.val = val.get(); V.partial = partial.get();
    V.tile_step = tile_step.get(); V.steps = steps.get();
    V.wide_start = wide_start.get(); V.wide = wide.get();
}

struct LayoutScratch;                 // layout_scratch.hpp

// The layout of a gather matrix's unmasked products; the values are the codes ipxk_spmv_layout reports (ABI: they do not move).
// Code 3 was the sorted sub-tiles (docs/DESIGN_HISTORY.md), retired: no layout has it.
enum class SpmvLayout { phased = 0, sliced = 1, fused = 2, sortedfused = 4, acc = 5, plain = 6, accfused = 7 };
constexpr int kNumSpmvLayouts = 8;             // codes, the retired one included: tuned_us[] is indexed by code
// their names by code (IPXK_SPMV_LAYOUT, verbose lines; ipx_amd/kkt.py uses the same); nullptr: the retired code, which every
// loop over the table skips
inline constexpr const char* kSpmvLayoutNames[kNumSpmvLayouts] = {"phased", "sliced", "fused", nullptr, "sortedfused", "acc", "plain",
                                                                  "accfused"};

// workgroups of the combine kernel on a product of nrows rows (launch_combine, spmv_kernels.hpp), hence its dot partials.
// IPXK_COMBINE_GRID=<g> caps it (tests: a thread then owns several rows of a small matrix)
inline int combine_grid_for(int64_t nrows) {
    static const int cap = [] { const char* e = getenv("IPXK_COMBINE_GRID"); return e && atoi(e) > 0 ? std::min(atoi(e), 1024) : 1024; }();
    return (int)std::min<int64_t>(cap, std::max<int64_t>(1, (nrows + kBlock - 1) / kBlock));
}

struct GatherMatrix {
    int nrows = 0, ncols = 0;
    int64_t nnz = 0;
    int P = 1, G = 1, RT = 1, Q = 1, RWrows = kBlock;
    DevBuf<int> step_ptr, idx, wg_chunk_ptr, chunk_start, chunk_info, chunk_step;
    DevBuf<unsigned char> counts, row_long;
    DevBuf<double> val;
    int nseg = 0, nlong = 0;
    DevBuf<int> seg_p0, seg_p1, lidx, long_row, long_slot;
    DevBuf<double> lval, long_partials;
    DevBuf<unsigned long long> stamps;   // allocated only when IPXK_STAMPS=1
    // how much of the layout choice build() pays for: 2 = every layout built and timed (the model matrix: once per
    // model), 1 = phased against fused only, 0 = the phased layout, no timing (auxiliary matrices built inside a
    // Factorize: the dense columns' gather matrices)
    int tune_level = 2;
    // optional copy in plain row order (ptr/idx/val) for callers that address single rows
    bool keep_plain = false;
    std::vector<int> h_plain_ptr;
    DevBuf<int> plain_idx;
    DevBuf<double> plain_val;

    // Builds from host arrays with 64-bit indices (ptr has nrows+1 entries).
    void build(int64_t nrows_, int64_t ncols_, const ipxint* hptr, const ipxint* hidx,
               const double* hval, hipStream_t s);
    // Builds from the plain device copy (ptr / idx 32 bits) with radix sorts on the device (layout_device.hip), every array equal
    // to the host builders'.  Long rows are taken out first (device_strip_long_rows) and the tiles built from the rest; a matrix
    // whose x needs slicing and whose gathers spread over the slices gets the sliced and accumulated tiles, every other
    // one -- x fits an XCD's L2, or the gathers have locality -- the fused, sorted fused and fused accumulated tiles and the plain
    // rows (build_device_local).  Returns false -- the caller then runs build() on host arrays -- for small matrices
    // (nnz < 2^16, also after the long rows are out), tune_level < 2, keep_plain, a forced layout, IPXK_LAYOUT_BUILD=host and
    // when the fused tiles cannot be built (more than 255 entries of a row in a tile, a tile beyond the staging buffer).
    bool build_device(LayoutScratch& S, int64_t nrows_, int64_t ncols_, int64_t nnz_, const int* dptr, const int* didx,
                      const double* dval, hipStream_t s);
    bool build_device_local(LayoutScratch& S, int64_t nrows_, int64_t ncols_, int64_t nnz_, const int* dptr, const int* didx,
                            const double* dval, double share, hipStream_t s);
    void set_geometry(int64_t nrows_, int64_t ncols_);      // P, G, RT, Q, RWrows of the phased layout
    // The layout of the unmasked launches, chosen by select_layout.  Masked and compacted launches run on the tile base.
    SpmvLayout layout = SpmvLayout::phased;
    // the tile base: the sliced or fused tiles when they are built, the phased layout otherwise
    SpmvLayout tile_base() const { return !sliced.built ? SpmvLayout::phased : sliced.nslices == 1 ? SpmvLayout::fused : SpmvLayout::sliced; }
    float tuned_us[kNumSpmvLayouts] = {};       // microseconds per product measured by time_layout (0: not timed)
    float time_layout(SpmvLayout L, hipStream_t s);
    // The choice of `layout` (spmv.hip has the rules), shared by the host and the device builders: make(L) builds the arrays of
    // candidate L in place and returns whether it could; the routine times the candidates, keeps the winner and releases the
    // arrays of the losers.
    void select_layout(const std::function<bool(SpmvLayout)>& make, hipStream_t s);
    // XCD-sliced tiles (several slices) or fused tiles (one slice)
    SlicedMatrix sliced;
    // sorted fused tiles (independent of the sliced layout)
    SortedMatrix sorted;
    void build_sorted_fused(const ipxint* hptr, const ipxint* hidx, const double* hval, hipStream_t s);
    // accumulated tiles (the sliced layout's slices, row sums in LDS), and their FUSED form
    AccMatrix acc;
    void build_acc(const ipxint* hptr, const ipxint* hidx, const double* hval, hipStream_t s);     // host builders: layout_host.hip
    void build_acc_fused(const ipxint* hptr, const ipxint* hidx, const double* hval, hipStream_t s);
    AccMatrix accf;
    AccView acc_fused_view() const;
    AccView acc_view() const;
    // plain rows (small matrices): the device's plain copy of the matrix itself, 8 lanes per row (spmv_rowgroup_kernel); set by
    // the caller of build() (the model matrices)
    const int* csr_ptr = nullptr;
    const int* csr_idx = nullptr;
    const double* csr_val = nullptr;
    int plain_grid() const { return (int)std::min<int64_t>(kMaxPartials, std::max<int64_t>(1, ((int64_t)nrows * 8 + kBlock - 1) / kBlock)); }
    int sorted_fused_grid() const {
        static const int cap = [] { const char* e = getenv("IPXK_SF_GRID"); return e && atoi(e) > 0 ? std::min(atoi(e), kMaxPartials) : kMaxPartials; }();
        return std::min(sorted.nrb, cap);
    }
    SortedView sorted_view() const;
    // ns_request: 0 = as many slices as x needs (>= 2), 1 = the fused single-slice variant
    void build_sliced(const ipxint* hptr, const ipxint* hidx, const double* hval, hipStream_t s, int ns_request);
    // which: 0 = the matrix, 1 = the masked value array (mask_values), 2 = the compacted copy (compact_tiles)
    SlicedView sliced_view(int which = 0) const;
    int fused_grid() const { return std::min(sliced.nrb, kMaxPartials); }
    int combine_grid() const { return combine_grid_for(nrows); }

    GatherView view(bool masked = false) const;
    int grid() const { return G; }
    // Masked products (the basis path's N N' on the model matrix: entries of BASIC / fixed columns count for
    // nothing): a second value array of the tile base in which those entries are zero -- the kernels issue no
    // gather for an entry whose value is zero.  mask_values() fills it from a weight per ROW of the gather matrix
    // (by_row) or per GATHERED index; view(true) / sliced_view(true) show it (launch_spmv<Epi, true>).
    DevBuf<double> valM, lvalM;
    // Compacted copy of the tile layout (sliced / fused): only the entries whose weight is nonzero, tile by tile
    // in the same order, with their own tile pointers and per-row counts -- the basis path's N as a matrix of its
    // own (SplittedNormalMatrix::Prepare copies N, src/splitted_normal_matrix.cc:42-55; here the copy is a stream
    // compaction of the resident tiles on the device).  Same arithmetic as the masked form (the entries left out
    // contributed exact zeros), but the kernels no longer stream them.  Long rows keep their masked values.
    struct CompactTiles {
        bool valid = false;
        DevBuf<unsigned> tile_ptr, tile_kept;
        DevBuf<unsigned char> cnt;
        DevBuf<int> idx;
        DevBuf<double> val;
    } compact;
    void compact_tiles(const double* weight, bool by_row, hipStream_t s);
    DevBuf<int> rowof;                  // row of every stored short entry (built on first use by mask_values(by_row))
    void mask_values(const double* weight, bool by_row, hipStream_t s);
    // # dot partials a launch writes (launch_spmv returns it; masked launches run on the tile base): one per workgroup of the
    // kernel that applies the epilogue, then the long-row fix-up's
    int num_partials(bool masked = false) const {
        int n;
        switch (masked ? tile_base() : layout) {
            case SpmvLayout::phased: n = G; break;
            case SpmvLayout::fused: n = fused_grid(); break;
            case SpmvLayout::sortedfused: n = sorted_fused_grid(); break;
            case SpmvLayout::plain: n = plain_grid(); break;
            case SpmvLayout::accfused: n = accf.nrb; break;
            default: n = combine_grid(); break;         // sliced, acc: the combine kernel
        }
        return n + (nlong > 0 ? 1 : 0);
    }
    std::vector<unsigned char> h_row_long;   // host copy of row_long (empty: no long rows)
};

// elements of the gathered vector per phase (IPXK_SLICE_KB overrides, default 1 MiB); phase_slice: of a vector of ncols entries
int slice_elems();
int64_t phase_slice(int64_t ncols);

// ---------------------------------------------------------------------------
// CR loop state kept on the device (see cr.hip)
// ---------------------------------------------------------------------------
struct CrState {
    double tol;
    long long maxiter;
    long long k_started;     // written by the control kernel, read by the others
    long long k_finished;    // written by the direction-update kernel
    double cdot[2];          // indexed by iteration parity
    double rps[2];           // resnorm_precond_system, indexed by (iter/5) parity
    double resnorm;          // residual norm at the last loop head
    long long iter;          // result: # iterations
    int errflag;             // result
    int done;
    long long hist_cap;
    double diag_rps_old, diag_rps_new;   // errflag 204: the two values of the monotonicity check
    int mode;                            // CrMode of the run (cr.hip)
    // lazy solution update: lhs += alpha_pending * step of iteration k_pending is still owed while
    // k_pending == k_finished (the direction kernel that pays it moves k_finished on); -1: nothing owed
    double alpha_pending;
    long long k_pending;
};

// ---------------------------------------------------------------------------
// the basis exchanges of maxvolume.hip and starting_basis.hip: the eta file and the device Basis (basis.hip)
// ---------------------------------------------------------------------------
// the scalars of one exchange step, written by the device, read by the host
struct MvScalars {
    int jn;                  // FindLargest
    double weight;
    int pmax, jb;            // ScaleFtran
    double vmax, weight_recomp, colscale_jn, invscale_pmax, pivot_col;
    int used_pmax, eta_nnz;
    double pivot_row;        // row[jn]
    int eta_total;           // entries of all etas after the last exchange
};

// per-workgroup partial of the two-stage reductions (device_utils.hpp): kBest x (largest value, its smallest index), a sum, a count
template <int kBest>
struct Partial { double v[kBest]; int i[kBest]; double s; int c; };
using MvPart = Partial<1>;

struct MaxvolState {
    DevBuf<double> colscale, invscale, colweights, row, mask, rhs, lhs, unit, btran, work;
    DevBuf<int> map2basis, slice_of, flag, rank, eta_ptr, eta_pos, eta_idx;
    DevBuf<double> eta_piv, eta_val;
    // the etas as dense vectors (mv_eta_dense_*): E [cap][m], T / Tt [cap][cap], multipliers, dots, links between the exchanges of a position
    DevBuf<double> etaE, etaT, etaTt, eta_alpha, eta_d;
    DevBuf<int> eta_prev, eta_next, eta_last;
    DevBuf<double> etaF, etaG, eta_w;      // the triangular systems of a kept eta file as matrices (mv_eta_*_matrix_kernel)
    DevBuf<int> eta_first, eta_jof;
    DevBuf<ipxint> basis, status;
    DevBuf<MvPart> part;
    DevBuf<MvScalars> scalars;
    DevBuf<unsigned char> tmp;
    MvScalars* h = nullptr;    // pinned
    // the drop procedures (drop.hip): device copies of basis, status and scaling factors, the candidate list (+ its count), the
    // scalars of a candidate and their pinned mirror; grow-only like the rest
    DevBuf<ipxint> drop_basis, drop_status;
    DevBuf<double> drop_colscale;
    DevBuf<int> drop_list;
    DevBuf<unsigned char> drop_scalars;
    void* drop_h = nullptr;    // pinned
    size_t drop_h_bytes = 0;
    // the eta file kept BEHIND the resident factors between two calls (Context::etas_live): what EtaFile needs to go on, and the basis
    // the factors + etas represent (by basis position; the device copy is `basis`)
    struct Saved {
        bool live = false, dense = false, have_history = false;
        int K = 0, cap = 0, m = 0;
        int64_t sparse_used = 0, seg_nnz = 0;
        double overhead_s = 0.0, refactor_s = 0.0;
        long lu_generation = -1;       // of the factors the etas stand behind (a later factorization in the context: no resuming)
        int Kd = 0;                    // > 0: etaF / etaG hold the matrices of the two triangular systems (Kd etas are the first at their position)
    } saved;
    std::vector<ipxint> basis_h;
    ~MaxvolState() { if (h) (void)hipHostFree(h); if (drop_h) (void)hipHostFree(drop_h); }
};

struct Context;

// The etas of the exchanges since the last refactorization (basis.hip has the methods and what they cost)
struct EtaFile {
    Context* c;
    MaxvolState& M;
    int m;
    hipStream_t s;
    bool dense = false, dense_possible = false, adaptive = false;
    int cap = 100;                 // most etas the buffers hold
    int limit = 100;               // fixed mode: refactorize after so many
    int64_t sparse_cap = 0, sparse_used = 0;
    int K = 0;
    double overhead_s = 0.0, refactor_s = 0.0;
    int64_t seg_nnz = 0;           // entries of the etas of the current segment (decides the next segment's form)
    bool have_history = false;
    bool resumed = false;

    // cost of one eta in one application (seconds): the list kernels spend two workgroup barriers and a dependent load per eta plus
    // its entries through one workgroup; the dense form a barrier of the triangular solve plus the eta's row of E in the one pass
    double cost_list(double nnz) const { return 2.5e-6 + 0.5e-9 * nnz; }
    double cost_dense() const { return 0.6e-6 + 8.0 * (double)m / 2e12; }

    EtaFile(Context* ctx, MaxvolState& state, int rows, ipxint max_etas_in, bool resume = false);
    void save();
    bool worth_keeping() const;
    void reset(int block_rows);
    // the eta of the exchange described by *S (pmax) from the tableau column lhs; eta_nnz: its number of nonzeros
    void append(const MvScalars* S, const double* lhs, int eta_nnz);
    bool full() const;
    void apply(bool transposed, double* v);
    static void apply_etas(MaxvolState& M, int m, int K, int cap, bool dense, bool transposed, double* v, hipStream_t s, int Kd = 0);
};

// The reference's Basis (src/basis.cc) for one call of a driver that exchanges on the device -- maxvolume_dev, maxvolume_sequential_dev,
// ipm_starting_basis_dev -- on the resident factors plus the eta file.  A candidate goes  ftran / btran_unit  (and the driver's own pivot
// search), one read-back of its scalars, then  exchange_if_stable  ->  the driver's exchange kernel  ->  commit.
struct DeviceBasis {
    Context* c;
    MaxvolState& M;
    const int m;
    EtaFile etas;
    double& pivottol;                          // the context's LU pivot tolerance (Context::maxvol_pivottol), tightened by the ladder
    std::vector<ipxint> basis_h, status_h;     // host mirrors (refactorizations, results); filled by the driver before the first exchange
    const double* colscale;                    // host, n + m: what split_prepare_lu is given on a refactorization
    MvScalars* S;                              // device: jn, pmax, jb and the pivots of the current candidate
    double *rhs, *lhs, *unit, *btran;          // m-vectors of MaxvolState
    // factorizations counts every attempt, as the reference's num_factorizations_++ does, singular those that found the basis singular
    // (errflag 301): the starting basis reports the attempts, Maxvolume has always reported factorizations - singular.
    int64_t refused = 0, factorizations = 0, singular = 0;
    ipxint errflag = 0;

    DeviceBasis(Context* ctx, MaxvolState& state, ipxint max_etas, bool resume, const double* colscale_in, MvScalars* scalars);
    void ftran();                              // lhs = inverse(B) a_(S->jn), the etas applied
    void btran_unit();                         // btran = inverse(B') e_(S->pmax), the etas applied
    bool refactorize();                        // false: the basis is singular, errflag 301
    // a: the host's copy of *S with both pivots.  true: the exchange is accepted and its eta appended -- the driver launches its exchange
    // kernel and calls commit.  false: try the candidate again (the pivot tolerance is tightened where the factors were fresh, the basis
    // refactorized) unless errflag is set (306: the ladder is at its top, 301)
    bool exchange_if_stable(const MvScalars& a);
    void commit(const MvScalars& a);           // the host mirrors; a refactorization when the eta file is full (errflag 301 if that fails)
};

// the one device -> host copy of a candidate's scalars, through a pinned block
template <class T>
T read_scalars(const T* dev, T* pinned, hipStream_t s) {
    IPXK_HIP(hipMemcpyAsync(pinned, dev, sizeof(T), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
    return *pinned;
}

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace ipxk

#include "layout_geometry.hpp"     // (needs the constants above; spmv_kernels.hpp needs acc_persist_grid)
