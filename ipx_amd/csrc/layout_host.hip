// The host builders of the gather-matrix layouts (internal.hpp): the phased arrays with the long-row segments and the plain copy
// (GatherMatrix::build), and the five tile layouts by single-threaded loops.  They serve small matrices, forced layouts,
// tune_level < 2, the dense columns' gather matrices and every matrix the device builders (layout_device.hip) decline, and they
// are the reference tests/test_gpu_layout.py compares the device builders with, array by array.  Slices, sub-slices and row
// blocks: layout_geometry.hpp, shared with the device builders.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>

#include "context.hpp"

namespace ipxk {

void GatherMatrix::build(int64_t nrows_, int64_t ncols_, const ipxint* hptr, const ipxint* hidx,
                         const double* hval, hipStream_t s) {
    IPXK_REQUIRE(nrows_ >= 0 && ncols_ >= 0, "negative dimension");
    IPXK_REQUIRE(nrows_ < (int64_t(1) << 31) - 1 && ncols_ < (int64_t(1) << 31) - 1,
                 "dimension exceeds 32-bit device indices");
    const int64_t nz = hptr[nrows_];
    IPXK_REQUIRE(nz < (int64_t(1) << 31) - kLongSeg, "nnz exceeds 32-bit device indices");
    nrows = (int)nrows_;
    ncols = (int)ncols_;
    nnz = nz;

    set_geometry(nrows_, ncols_);
    const int64_t slice = phase_slice(ncols_);
    const int64_t RW = (int64_t)kBlock * RT;     // count slots per step
    const int64_t nsteps = (int64_t)Q * P * G;
    IPXK_REQUIRE(nsteps * RW < (int64_t(1) << 40), "matrix too large for the phased layout");

    // long rows
    std::vector<unsigned char> rlong;
    std::vector<int> sp0, sp1, lrow, lslot, li;
    std::vector<double> lv;
    for (int r = 0; r < nrows; r++) {
        const int64_t len = hptr[r + 1] - hptr[r];
        if (len <= kMaxRowLen) continue;
        if (rlong.empty()) rlong.assign(nrows, 0);
        rlong[r] = 1;
        lrow.push_back(r);
        lslot.push_back((int)sp0.size());
        for (int64_t q0 = hptr[r]; q0 < hptr[r + 1]; q0 += kLongSeg) {
            const int64_t q1 = std::min<int64_t>(q0 + kLongSeg, hptr[r + 1]);
            sp0.push_back((int)li.size());
            for (int64_t p = q0; p < q1; p++) { li.push_back((int)hidx[p]); lv.push_back(hval[p]); }
            sp1.push_back((int)li.size());
        }
    }
    lslot.push_back((int)sp0.size());
    nlong = (int)lrow.size();
    nseg = (int)sp0.size();
    h_row_long = rlong;

    // counts per (row, phase) and step sizes
    std::vector<unsigned char> cnt((size_t)nsteps * RW, 0);
    std::vector<int> sptr(nsteps + 1, 0);
    auto step_of = [&](int r, int p, int64_t& lr) {
        const int64_t per = (int64_t)G * RWrows;
        const int64_t q = r / per, rem = r % per;
        const int64_t w = rem / RWrows;
        lr = rem % RWrows;
        return (q * P + p) * G + w;
    };
    for (int r = 0; r < nrows; r++) {
        if (!rlong.empty() && rlong[r]) continue;
        for (int64_t p = hptr[r]; p < hptr[r + 1]; p++) {
            int64_t lr;
            const int64_t st = step_of(r, (int)(hidx[p] / slice), lr);
            cnt[(size_t)st * RW + lr]++;
            sptr[st + 1]++;
        }
    }
    for (int64_t st = 0; st < nsteps; st++) sptr[st + 1] += sptr[st];
    const int64_t nshort = sptr[nsteps];
    std::vector<int> i32((size_t)std::max<int64_t>(nshort, 1));
    std::vector<double> v64((size_t)std::max<int64_t>(nshort, 1));
    {
        std::vector<int> cursor(sptr.begin(), sptr.end() - 1);
        for (int r = 0; r < nrows; r++) {
            if (!rlong.empty() && rlong[r]) continue;
            for (int64_t p = hptr[r]; p < hptr[r + 1]; p++) {
                int64_t lr;
                const int64_t st = step_of(r, (int)(hidx[p] / slice), lr);
                const int put = cursor[st]++;
                i32[put] = (int)hidx[p];
                v64[put] = hval[p];
            }
        }
    }

    // chunk table
    std::vector<int> wcp((size_t)Q * G + 1, 0), cst, cinf, cstep;
    for (int q = 0; q < Q; q++)
        for (int w = 0; w < G; w++) {
            for (int p = 0; p < P; p++) {
                const int64_t st = ((int64_t)q * P + p) * G + w;
                for (int c0 = sptr[st]; c0 < sptr[st + 1]; c0 += kChunkNnz) {
                    cst.push_back(c0);
                    cinf.push_back(std::min(kChunkNnz, sptr[st + 1] - c0) | (c0 == sptr[st] ? (1 << 30) : 0));
                    cstep.push_back((int)st);
                }
            }
            wcp[(size_t)q * G + w + 1] = (int)cst.size();
        }
    for (int pad = 0; pad < 4; pad++) { cst.push_back(0); cinf.push_back(0); cstep.push_back(0); }
    wg_chunk_ptr.upload(wcp, s);
    chunk_start.upload(cst, s);
    chunk_info.upload(cinf, s);
    chunk_step.upload(cstep, s);
    step_ptr.upload(sptr, s);
    counts.upload(cnt, s);
    idx.upload(i32, s);
    val.upload(v64, s);
    if (nlong > 0) {
        row_long.upload(rlong, s);
        seg_p0.upload(sp0, s);
        seg_p1.upload(sp1, s);
        lidx.upload(li, s);
        lval.upload(lv, s);
        long_row.upload(lrow, s);
        long_slot.upload(lslot, s);
    }
    long_partials.resize(nseg > 0 ? nseg : 1);
    if (getenv("IPXK_STAMPS")) stamps.resize((size_t)nsteps + G);
    if (keep_plain) {
        h_plain_ptr.resize(nrows + 1);
        std::vector<int> pi((size_t)std::max<int64_t>(nz, 1));
        for (int r = 0; r <= nrows; r++) h_plain_ptr[r] = (int)hptr[r];
        for (int64_t p = 0; p < nz; p++) pi[p] = (int)hidx[p];
        plain_idx.upload(pi, s);
        plain_val.upload(hval, (size_t)nz, s);
    }
    IPXK_HIP(hipStreamSynchronize(s));  // host vectors go out of scope

    select_layout([&](SpmvLayout L) {
        switch (L) {
            case SpmvLayout::phased: return true;
            case SpmvLayout::sliced:
            case SpmvLayout::fused: build_sliced(hptr, hidx, hval, s, L == SpmvLayout::fused ? 1 : 0); return sliced.built;
            case SpmvLayout::sortedfused: build_sorted_fused(hptr, hidx, hval, s); return sorted.built;
            case SpmvLayout::acc: build_acc(hptr, hidx, hval, s); return acc.built;
            case SpmvLayout::accfused: build_acc_fused(hptr, hidx, hval, s); return accf.built;
            case SpmvLayout::plain: return csr_ptr != nullptr;
        }
        return false;
    }, s);
}

// Sliced layout (internal.hpp).  Eligible when x does not fit an XCD's L2, no row is "long" and
// every tile fits the LDS staging buffer.
void GatherMatrix::build_sliced(const ipxint* hptr, const ipxint* hidx, const double* hval, hipStream_t s,
                                int ns_request) {
    if (nrows == 0 || nnz == 0 || ncols == 0) return;
    // long rows (dense columns) stay with the long-row kernels, the tiles hold everything else
    const std::vector<unsigned char>& rlong = h_row_long;
    int64_t nshort = nnz;
    for (int r = 0; r < nrows && !rlong.empty(); r++) if (rlong[r]) nshort -= hptr[r + 1] - hptr[r];
    if (nshort == 0) return;
    const Slices sl = model_slices(ncols, ns_request);
    if (sl.fits_l2) return;                          // nothing to slice
    const int ns = sl.ns;
    const int64_t slice = sl.width;
    RowBlockSearch search = sliced_rows(nrows, ns);
    int R = 0, nrb = 0, max_tile = 0;
    int64_t ntiles = 0;
    std::vector<unsigned> tptr;
    std::vector<unsigned char> cnt;
    const bool verbose = getenv("IPXK_VERBOSE") != nullptr;
    for (;; search.next()) {
        R = search.rows;
        if (search.gave_up()) {
            if (verbose) fprintf(stderr, "ipxk: sliced layout not used for %d x %d: a tile of %d rows holds %d entries\n", nrows, ncols, 2 * R, max_tile);
            return;
        }
        nrb = (nrows + R - 1) / R;
        ntiles = (int64_t)nrb * ns;
        // pass 1: entries per (tile, row)
        tptr.assign((size_t)ntiles + 1, 0);
        cnt.assign((size_t)ntiles * R, 0);
        for (int r = 0; r < nrows; r++) {
            if (!rlong.empty() && rlong[r]) continue;
            const int64_t tile0 = (int64_t)(r / R) * ns;
            const int rr = r % R;
            for (ipxint p = hptr[r]; p < hptr[r + 1]; p++) {
                const int64_t tile = tile0 + hidx[p] / slice;
                unsigned char& cc = cnt[(size_t)tile * R + rr];
                if (cc == 255) {                                // count does not fit a byte
                    if (verbose) fprintf(stderr, "ipxk: sliced layout not used for %d x %d: row %d has > 255 entries in one slice\n", nrows, ncols, r);
                    return;
                }
                cc++;
                tptr[tile + 1]++;
            }
        }
        max_tile = 0;
        for (int64_t t = 0; t < ntiles; t++) {
            max_tile = std::max(max_tile, (int)tptr[t + 1]);
            tptr[t + 1] += tptr[t];
        }
        if ((int64_t)tptr[ntiles] != nshort) return;
        if (search.fits(max_tile)) break;
    }
    // how concentrated the gathers of a row block are: share of the entries in the block's fullest slice
    // (1/ns for uniformly spread indices, ~1 for a banded matrix)
    {
        int64_t dom = 0;
        for (int rb = 0; rb < nrb; rb++) {
            unsigned best = 0;
            for (int sl = 0; sl < ns; sl++) best = std::max(best, tptr[(size_t)rb * ns + sl + 1] - tptr[(size_t)rb * ns + sl]);
            dom += best;
        }
        sliced.dominant_fraction = (double)dom / (double)nshort;
    }
    // pass 2: fill, rows in order, a row's entries in storage order (no assumption that the indices
    // of a row are sorted)
    std::vector<int> ti((size_t)nshort);
    std::vector<double> tv((size_t)nshort);
    std::vector<unsigned> cursor(tptr.begin(), tptr.end() - 1);
    for (int r = 0; r < nrows; r++) {
        if (!rlong.empty() && rlong[r]) continue;
        const int64_t tile0 = (int64_t)(r / R) * ns;
        for (ipxint p = hptr[r]; p < hptr[r + 1]; p++) {
            const unsigned put = cursor[tile0 + hidx[p] / slice]++;
            ti[put] = (int)hidx[p];
            tv[put] = hval[p];
        }
    }
    sliced.R = R;
    sliced.nslices = ns;
    sliced.nrb = nrb;
    sliced.nrows_pad = nrb * R;
    sliced.max_tile = max_tile;
    sliced.tile_ptr.upload(tptr, s);
    sliced.cnt.upload(cnt, s);
    sliced.idx.upload(ti, s);
    sliced.val.upload(tv, s);
    sliced.partial.resize(ns > 1 ? (size_t)ns * sliced.nrows_pad : 1);
    IPXK_HIP(hipStreamSynchronize(s));
    sliced.built = true;
}

namespace {
// The batches of the accumulated tiles (internal.hpp), tile after tile: the greedy list schedule that acc_batch_kernel
// (layout_device.hip) runs with one wavefront per tile.
struct AccEntry { unsigned off, row; double v; };       // offset in the slice or window, row in the block, value
struct AccBatcher {
    std::vector<unsigned> pk, bp;      // the entry words; the first entry of every batch
    std::vector<double> tv;
    int64_t deferred = 0;              // entries that waited for a later batch, counted once per wait
    std::vector<int> stamp, pend, newpend;
    AccBatcher(int64_t nnz, int RB) : pk((size_t)nnz), tv((size_t)nnz), stamp((size_t)RB) {}
    // a: the ne entries of a tile in storage order, which take the places [base, base + ne)
    void tile(AccEntry* a, int ne, unsigned base) {
        std::stable_sort(a, a + ne, [](const AccEntry& x, const AccEntry& y) { return x.off < y.off; });
        std::fill(stamp.begin(), stamp.end(), -1);
        pend.clear();
        int cursor = 0, put = 0, batch = 0;
        while (put < ne) {
            bp.push_back(base + (unsigned)put);
            newpend.clear();
            int fill = 0;
            auto offer = [&](int i) {
                if (stamp[a[i].row] == batch || fill == kAccBatch) { newpend.push_back(i); deferred++; return; }
                stamp[a[i].row] = batch;
                pk[base + put] = (a[i].row << kSortedOffBits) | a[i].off;
                tv[base + put] = a[i].v;
                put++; fill++;
            };
            for (int i : pend) offer(i);                                   // whoever waited goes first, in order
            while (fill < kAccBatch && cursor < ne) offer(cursor++);      // then the stream
            pend.swap(newpend);
            batch++;
        }
    }
    // the arrays every accumulated form has, the step table from them; tb: first batch of every tile, its last entry still to be set
    void finish(AccMatrix& A, std::vector<unsigned>& tb, int64_t nnz, hipStream_t s) {
        tb.back() = (unsigned)bp.size();
        bp.push_back((unsigned)nnz);
        A.nbatches = (int64_t)bp.size() - 1; A.deferred = deferred;
        A.tile_batch.upload(tb, s);
        A.bptr.upload(bp, s);
        A.pack.upload(pk, s);
        A.val.upload(tv, s);
        acc_build_steps(A, (int64_t)tb.size() - 1, nnz, !A.fused, s);
    }
};
}  // namespace

// Accumulated tiles (internal.hpp)
void GatherMatrix::build_acc(const ipxint* hptr, const ipxint* hidx, const double* hval, hipStream_t s) {
    acc = AccMatrix();
    if (!sliced.built || sliced.nslices < 2 || nlong > 0 || nnz == 0) return;
    const int ns = sliced.nslices;
    const int64_t slice = slice_width(ncols, ns);
    if (!offsets_fit(slice)) return;
    const int RB = acc_rows_per_block(nrows, ns);
    const int nrb = (nrows + RB - 1) / RB;
    const int64_t ntiles = (int64_t)nrb * ns;
    std::vector<unsigned> tptr((size_t)ntiles + 1, 0);
    for (int r = 0; r < nrows; r++)
        for (ipxint p = hptr[r]; p < hptr[r + 1]; p++) tptr[(size_t)(r / RB) * ns + hidx[p] / slice + 1]++;
    for (int64_t t = 0; t < ntiles; t++) tptr[t + 1] += tptr[t];
    std::vector<AccEntry> all((size_t)nnz);
    {
        std::vector<unsigned> cursor(tptr.begin(), tptr.end() - 1);
        for (int r = 0; r < nrows; r++)
            for (ipxint p = hptr[r]; p < hptr[r + 1]; p++) {
                const int64_t sl = hidx[p] / slice;
                all[cursor[(size_t)(r / RB) * ns + sl]++] = AccEntry{(unsigned)(hidx[p] - sl * slice), (unsigned)(r % RB), hval[p]};
            }
    }
    std::vector<unsigned> tb((size_t)ntiles + 1, 0);
    AccBatcher B(nnz, RB);
    for (int64_t t = 0; t < ntiles; t++) {
        tb[t] = (unsigned)B.bp.size();
        B.tile(all.data() + tptr[t], (int)(tptr[t + 1] - tptr[t]), tptr[t]);
    }
    acc.nslices = ns; acc.nrb = nrb; acc.RB = RB; acc.nrows_pad = nrb * RB; acc.slice_elems = (int)slice; acc.xlen = ncols;
    B.finish(acc, tb, nnz, s);
    acc.partial.resize((size_t)ns * acc.nrows_pad);
    IPXK_HIP(hipStreamSynchronize(s));
    acc.built = true;
}

// FUSED accumulated tiles (internal.hpp): one slice, the epilogue in the tile kernel.  Only for matrices without long rows whose
// rows are stored with ascending indices and whose row blocks gather from windows of less than 2^18 entries.
void GatherMatrix::build_acc_fused(const ipxint* hptr, const ipxint* hidx, const double* hval, hipStream_t s) {
    accf = AccMatrix();
    if (nrows == 0 || nnz == 0 || ncols == 0 || nlong > 0) return;
    for (int r = 0; r < nrows; r++)
        for (ipxint p = hptr[r] + 1; p < hptr[r + 1]; p++)
            if (hidx[p] <= hidx[p - 1]) return;                    // unsorted row: the sum would not be in storage order
    const int RB = acc_fused_rows(nrows);
    if (RB == 0) return;
    const int nrb = (nrows + RB - 1) / RB;
    std::vector<AccEntry> a;
    std::vector<unsigned> tb((size_t)nrb + 1, 0);
    std::vector<int> xmin((size_t)nrb, 0);
    AccBatcher B(nnz, RB);
    unsigned base = 0;
    for (int t = 0; t < nrb; t++) {
        const int r1 = std::min(nrows, (t + 1) * RB);
        ipxint lo = ncols, hi = -1;
        for (int r = t * RB; r < r1; r++)
            for (ipxint p = hptr[r]; p < hptr[r + 1]; p++) { lo = std::min(lo, hidx[p]); hi = std::max(hi, hidx[p]); }
        tb[t] = (unsigned)B.bp.size();
        if (hi < 0) continue;
        if (!window_fits(hi - lo)) return;
        xmin[t] = (int)lo;
        a.clear();
        for (int r = t * RB; r < r1; r++)
            for (ipxint p = hptr[r]; p < hptr[r + 1]; p++) a.push_back(AccEntry{(unsigned)(hidx[p] - lo), (unsigned)(r - t * RB), hval[p]});
        B.tile(a.data(), (int)a.size(), base);
        base += (unsigned)a.size();
    }
    accf.nslices = 1; accf.nrb = nrb; accf.RB = RB; accf.nrows_pad = nrb * RB; accf.slice_elems = 0; accf.fused = true;
    B.finish(accf, tb, nnz, s);
    accf.xmin.upload(xmin, s);
    IPXK_HIP(hipStreamSynchronize(s));
    accf.built = true;
}

// Sorted fused tiles (internal.hpp): one slice, the epilogue in the tile kernel.
void GatherMatrix::build_sorted_fused(const ipxint* hptr, const ipxint* hidx, const double* hval, hipStream_t s) {
    sorted = SortedMatrix();
    if (nrows == 0 || nnz == 0 || ncols == 0) return;
    const std::vector<unsigned char>& rlong = h_row_long;
    RowBlockSearch search = sorted_fused_rows(nrows);
    int RB = 0, nrb = 0, max_sub = 0;
    int64_t nshort = 0;
    std::vector<unsigned> sptr;
    std::vector<unsigned char> cnt;
    for (;; search.next()) {
        RB = search.rows;
        if (search.gave_up()) return;
        nrb = (nrows + RB - 1) / RB;
        sptr.assign((size_t)nrb + 1, 0);
        cnt.assign((size_t)nrb * RB, 0);
        bool ok = true;
        for (int r = 0; r < nrows && ok; r++) {
            if (!rlong.empty() && rlong[r]) continue;
            const int64_t len = hptr[r + 1] - hptr[r];
            if (len > 255) { ok = false; break; }
            cnt[(size_t)(r / RB) * RB + r % RB] = (unsigned char)len;
            sptr[r / RB + 1] += (unsigned)len;
        }
        if (!ok) return;
        max_sub = 0;
        for (int t = 0; t < nrb; t++) { max_sub = std::max(max_sub, (int)sptr[t + 1]); sptr[t + 1] += sptr[t]; }
        nshort = sptr[nrb];
        if (search.fits(max_sub)) break;
    }
    if (nshort == 0) return;
    std::vector<int> xmin((size_t)nrb, 0);
    std::vector<unsigned> pk((size_t)nshort);
    std::vector<double> tv((size_t)nshort);
    std::vector<std::pair<ipxint, std::pair<unsigned, double>>> tmp;    // (index, (slot, value))
    for (int t = 0; t < nrb; t++) {
        tmp.clear();
        const int r1 = std::min(nrows, (t + 1) * RB);
        ipxint lo = ncols, hi = -1;
        for (int r = t * RB; r < r1; r++) {
            if (!rlong.empty() && rlong[r]) continue;
            for (ipxint p = hptr[r]; p < hptr[r + 1]; p++) {
                tmp.push_back({hidx[p], {(unsigned)tmp.size(), hval[p]}});
                lo = std::min(lo, hidx[p]); hi = std::max(hi, hidx[p]);
            }
        }
        if (tmp.empty()) continue;
        if (!window_fits(hi - lo)) return;
        xmin[t] = (int)lo;
        std::sort(tmp.begin(), tmp.end(), [](const std::pair<ipxint, std::pair<unsigned, double>>& a,
                                             const std::pair<ipxint, std::pair<unsigned, double>>& b) {
            return a.first != b.first ? a.first < b.first : a.second.first < b.second.first;
        });
        for (size_t e = 0; e < tmp.size(); e++) {
            pk[sptr[t] + e] = (tmp[e].second.first << kSortedOffBits) | (unsigned)(tmp[e].first - lo);
            tv[sptr[t] + e] = tmp[e].second.second;
        }
    }
    sorted.nrb = nrb; sorted.RB = RB; sorted.nrows_pad = nrb * RB; sorted.max_sub = max_sub;
    sorted.sub_ptr.upload(sptr, s);
    sorted.cnt.upload(cnt, s);
    sorted.pack.upload(pk, s);
    sorted.val.upload(tv, s);
    sorted.xmin.upload(xmin, s);
    IPXK_HIP(hipStreamSynchronize(s));
    sorted.built = true;
}

}  // namespace ipxk
