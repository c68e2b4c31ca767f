// The geometry of the tile layouts (internal.hpp), stated once.  Every layout has a host builder (layout_host.hip) and a device
// builder (layout_device.hip) whose arrays must be equal bit for bit, and nmatrix.hip cuts N by the same rules: the number and
// width of the slices, the row blocks a builder tries, and when a layout does not apply all come from here.
// Plain host code, no HIP calls.  What stays with a builder is the measurement of its fullest tile (a host loop on one side, a
// kernel and a read-back on the other) and guards that belong to one implementation only (the width of the radix keys).
#pragma once

#include "internal.hpp"

namespace ipxk {

// ---- slices of the gathered vector x ----
// width: entries of x per slice, a multiple of 16; fits_l2: x fits an XCD's L2, nothing to slice -- the model builders decline, N
// takes one slice
struct Slices { int ns = 1; int64_t width = 0; bool fits_l2 = false; };
inline int64_t slice_width(int64_t ncols, int ns) { return ((ncols + ns - 1) / ns + 15) / 16 * 16; }
// one_slice: the fused forms.  Otherwise as many slices of 2 MiB (half of an XCD's L2; IPXK_SLICE_TEST_KB: tests make small
// matrices eligible) as x needs, 2, 4 or 8.  force2: two slices already for an x of more than one slice's size.
inline Slices slices_of(int64_t ncols, bool one_slice, bool force2 = false) {
    Slices S;
    if (!one_slice) {
        int64_t slice_bytes = int64_t(2) << 20;
        if (const char* e = getenv("IPXK_SLICE_TEST_KB"))
            if (atoi(e) > 0) slice_bytes = (int64_t)atoi(e) << 10;
        const int64_t x_bytes = ncols * 8;
        S.fits_l2 = x_bytes <= 2 * slice_bytes && !(force2 && x_bytes > slice_bytes);
        S.ns = S.fits_l2 ? 1 : 2;
        while (!S.fits_l2 && S.ns < 8 && x_bytes > (int64_t)S.ns * slice_bytes) S.ns *= 2;
    }
    S.width = slice_width(ncols, S.ns);
    return S;
}
// the model's gather matrices (ns_request: 0 = as many slices as x needs, 1 = one); IPXK_SLICE_FORCE2: experiments with two slices
inline Slices model_slices(int64_t ncols, int ns_request) { return slices_of(ncols, ns_request == 1, getenv("IPXK_SLICE_FORCE2") != nullptr); }

// ---- the 18 bits of an entry word's offset (sorted and accumulated tiles) ----
// a slice must not be wider, and a fused tile's window of x (largest - smallest gathered index) must stay below: wider means
// there is no locality to use
inline bool offsets_fit(int64_t slice) { return slice <= (int64_t(1) << kSortedOffBits); }
inline bool window_fits(int64_t span) { return span < (int64_t(1) << kSortedOffBits); }

// ---- rows per tile ----
// A builder tries `rows`, measures its fullest tile and halves until that fits; below `least` the layout is not used.
struct RowBlockSearch {
    int rows, least, max_entries;
    bool gave_up() const { return rows < least; }
    void next() { rows /= 2; }
    bool fits(int fullest_tile) const { return fullest_tile <= max_entries; }
};
inline int64_t row_blocks(int64_t nrows, int rows) { return (nrows + rows - 1) / rows; }
// sliced / fused tiles: as many rows as fit the LDS staging buffer (a matrix whose rows concentrate in one slice, e.g. a banded
// one, needs smaller tiles than a uniformly random one).  fill_chip (the model's matrices; not N): small matrices start with
// enough tiles to give every CU several workgroups (C2, 50k x 100k: 98 tiles of 1024 rows kept 98 of the 256 CUs busy with
// 8192 entries each)
inline RowBlockSearch sliced_rows(int nrows, int ns, bool fill_chip = true) {
    int R = kSlicedRows;
    while (fill_chip && R > kBlock && row_blocks(nrows, R) * ns < 2048) R /= 2;
    return {R, kBlock, kSlicedMaxTile};
}
// sorted fused tiles: enough tiles to fill the chip (IPXK_SF_MAXSUB: a smaller tile, measurements)
inline RowBlockSearch sorted_fused_rows(int nrows) {
    static const int cap = [] { const char* e = getenv("IPXK_SF_MAXSUB"); return e && atoi(e) >= 256 ? std::min(atoi(e), kSortedMaxSub) : kSortedMaxSub; }();
    int RB = 32 * kSortedThreads;
    while (RB > kSortedThreads && row_blocks(nrows, RB) < 1024) RB /= 2;
    return {RB, kSortedThreads, cap};
}
// fused accumulated tiles: as many rows as a batch has entries (a batch takes one entry per row: with fewer rows its batches could
// not fill, with more the greedy leaves more tail batches), doubled until there are at most kMaxPartials tiles; 0: too many rows.
// Measured on the banded probe, 8-entry rows: 2048 rows 43.9 us per pass (7816 batches for 16 M entries), 4096 rows 46.0 (9998);
// 16-entry rows: 1024 rows 112, 2048 rows 83 -- those keep the sorted fused tiles (58.6), the timing decides.
// (They also need a matrix without long rows whose rows are stored with ascending indices -- else the sum would not be in storage
// order -- and windows that fit: the builders check, a loop over the rows on the host, tile_window_kernel's flag on the device.)
inline int acc_fused_rows(int nrows) {
    int RB = kAccBatch;
    while (row_blocks(nrows, RB) > kMaxPartials) RB *= 2;
    return RB > kAccMaxRows ? 0 : RB;
}
// accumulated tiles: the row block follows the persistent kernel's grid.  Both ask the device for its CU count, hence are
// defined in layout_device.hip.
// workgroups of the persistent tile kernel on the current device: its CU count rounded down to a multiple of 8 (XCDs) and of
// ns, so that a workgroup's tiles are all of one slice and stay on one XCD; 0 with IPXK_ACC_PERSIST=0 (one workgroup per tile);
// IPXK_ACC_PERSIST=<g> caps it at g
int acc_persist_grid(int ns);
int acc_rows_per_block(int nrows, int ns);

}  // namespace ipxk
