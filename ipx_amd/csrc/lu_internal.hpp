// What the two halves of the basis LU share: lu.hip (row-wise index, singleton rounds, tearing, elimination rounds, stages,
// assembly) and lu_dense.hip (the dense LU of the bump).  The policy record of a factorization, the dense workspaces, and the
// helpers around rocprim and the pinned read-back block.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/device/device_merge.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <cstdlib>

#include "context.hpp"

namespace ipxk {

using u64 = unsigned long long;
constexpr int kPanel = 32;           // columns per panel of the dense elimination
constexpr int kPanelThreads = 1024;
// Bumps of more than kPanelThreads rows: panels of kNarrow columns, a thread owns R rows of the panel in registers
// (R * kPanelThreads >= rows).  Same arithmetic, same order; the two kernels that follow a panel take the number
// of its pivots from bstep[1], so they serve both panel widths.
constexpr int kNarrow = 8;            // panel width with 4 rows per thread (bumps of 2049 .. 4096 rows)
constexpr int kNarrowWide = 16;       // ... with 2 rows per thread (1025 .. 2048 rows): half the panels, the same registers
constexpr int kNarrowDeep = 4;        // ... with 8 rows per thread (4097 .. 8192 rows)
constexpr int kNarrowHuge = 2;        // ... with 16 rows per thread (8193 .. 16384 rows: the dense fall-back of a bump that tearing cannot cut down)
constexpr int kNarrowGiant = 1;       // ... with 32 rows per thread (16385 .. 32768 rows: what the elimination rounds leave of the bump of an IPM basis of 50 000 rows and more)
constexpr int kDenseHardMax = 32 * 1024;
constexpr int kNarrowWideMax = 16;    // the widest sub-panel
constexpr int kCoopThreads = 256;     // cooperative outer panel (lu_dense.hip): threads per workgroup
constexpr int kBstepSet = 4;          // ints per set of Dense::bstep (lu_dense.hip); two sets, used by the outer panels alternately (look-ahead)

// ---- the policy of one factorization --------------------------------------------------------------
// Every IPXK_LU_* knob that steers a factorization and what follows from the knobs, read once at its start (the tests switch
// knobs inside one process).  What also depends on the size of the dense block is a function of kb below.
struct LuPolicy {
    // which way a bump goes
    int kb_max;                 // IPXK_LU_BUMP_MAX: the largest bump factorized densely as it stands
    bool sparse_allowed, legacy_rounds, legacy;      // IPXK_LU_SPARSE: != 0; == 1; any of 0, 1, t (the policies of rounds 3 and 4)
    int spike_max, rest_max;    // the largest dense block of spikes / of what the elimination rounds leave
    int sparse_from, sparse_first_max, sparse_min, slow_den, fill_max;
    double dense_at;
    // 2b. the substitution of the spikes
    size_t spike_mem_mb;
    bool spike_runs;
    // 2. the dense LU
    bool two_level, fused_sub, coop;
    int panel_w;                // IPXK_LU_PANEL_W (0: not set)
    int mfma_min;
    int lookahead;              // IPXK_LU_LOOKAHEAD: -1 not set (from 6144 rows), 0 never, 1 always with the matrix cores
    int free_cus, xcc0;
    bool spread;
    int coop_R;                 // IPXK_LU_COOP_R (0: not set)
    int coop_xcd;               // IPXK_LU_COOP_XCD: -1 not set, 0 never, 1 wherever at most 32 workgroups take part

    // two-level panels: the sub-panel width of a bump of kb rows (R = kPanel / width ... rows per thread in registers)
    int subpanel_width(int kb) const {
        const int w = kb <= 2 * kPanelThreads ? kNarrowWide : kb <= 4 * kPanelThreads ? kNarrow : kb <= 8 * kPanelThreads ? kNarrowDeep :
                      kb <= 16 * kPanelThreads ? kNarrowHuge : kNarrowGiant;
        // (tests: a narrower sub-panel than the bump needs -- more rows per thread)
        const bool valid = panel_w == 1 || panel_w == 2 || panel_w == 4 || panel_w == 8 || panel_w == 16;
        return valid && panel_w <= w ? panel_w : w;
    }
    // the matrix cores for the trailing update of large bumps (IPXK_LU_MFMA_MIN rows and more, default 1025; 0: never)
    bool use_mfma(int kb) const { return mfma_min > 0 && kb >= mfma_min; }
    // Measured (scripts/gpu_lu_fused_check.py): 107.7 -> 96.2 ms at 8000 rows with 32 compute units kept free for the panel
    // kernels (16: no gain; the same 32 spread over the mask's words: slower), nothing at 5000 rows -- so from 6144 rows on
    // (IPXK_LU_LOOKAHEAD=1: always with the matrix cores, =0: never).
    bool lookahead_at(int kb) const { return use_mfma(kb) && (lookahead >= 0 ? lookahead != 0 : kb >= 6144); }
    // cooperative outer panel: 1 row per thread up to 8192 rows (G <= 32), 2 beyond (G <= 64).  Measured at 8000 rows: 1 and 2
    // rows per thread 68.9 ms both (the exchange, not the width of the barrier, is what a column costs: ~5 us); 4 rows per
    // thread spill to scratch (146 ms) and are not used
    int coop_rows(int kb) const {
        const int r = kb <= 8 * kPanelThreads ? 1 : 2;
        return (coop_R == 1 || coop_R == 2) && coop_R >= r ? coop_R : r;           // (IPXK_LU_COOP_R: measurement)
    }
    int coop_groups(int kb) const { return (kb + coop_rows(kb) * kCoopThreads - 1) / (coop_rows(kb) * kCoopThreads); }
    // the participants on ONE XCD (its L2 is coherent: messages by plain stores) where one workgroup per compute unit of that
    // XCD holds them all and nothing else competes for the XCD: at most 24 workgroups, no look-ahead (blocks of up to 6144
    // rows).  Measured: 2600 / 5000 rows 16.0 / 37.4 -> 14.4 / 33.0 ms; with the look-ahead's late update on the other stream
    // the participants wait for compute units of their XCD, 8000 rows 62.8 -> 76.3 ms, 12 000 rows 149 -> 193 ms, so those
    // blocks keep all XCDs and write-through messages.  (IPXK_LU_COOP_XCD=0: never, =1: wherever at most 32 workgroups take part)
    bool coop_one_xcd(int kb) const {
        return coop && coop_xcd != 0 && (coop_xcd == 1 ? coop_groups(kb) <= 32 : (!lookahead_at(kb) && coop_groups(kb) <= 24));
    }
};

LuPolicy lu_read_policy();      // from the environment (lu.hip)

// ---- helpers --------------------------------------------------------------------------------------
struct Tmp {
    DevBuf<unsigned char> bytes;
    void* need(size_t n) { if (bytes.size() < n) bytes.resize(n); return bytes.get(); }
};

// rocprim's two calls (size of the temporary storage, then the work) in one
template <class F>
void with_tmp(Tmp& T, F call) {
    size_t bytes = 0;
    IPXK_HIP(call(nullptr, bytes));
    IPXK_HIP(call(T.need(bytes), bytes));
}
inline void scan_exclusive(Tmp& T, const int* in, int* out, size_t n, hipStream_t s) {
    with_tmp(T, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, in, out, 0, n, rocprim::plus<int>(), s); });
}
// radix sorts over the key bits [0, end_bit): (keys, vals) -> (keys2, vals2)
template <class K, class V>
void sort_pairs(Tmp& T, K* keys, K* keys2, V* vals, V* vals2, size_t n, int end_bit, hipStream_t s) {
    with_tmp(T, [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, keys, keys2, vals, vals2, n, 0u, (unsigned)end_bit, s); });
}
template <class K>
void sort_keys(Tmp& T, K* keys, K* keys2, size_t n, int end_bit, hipStream_t s) {
    with_tmp(T, [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, keys, keys2, n, 0u, (unsigned)end_bit, s); });
}
// stable merge of two sorted lists (at equal keys: a's first)
template <class K, class V>
void merge_by_key(Tmp& T, K* ka, K* kb, K* kout, V* va, V* vb, V* vout, size_t na, size_t nb, hipStream_t s) {
    with_tmp(T, [&](void* t, size_t& b) { return rocprim::merge(t, b, ka, kb, kout, va, vb, vout, na, nb, rocprim::less<K>(), s); });
}

// `n` counters from the device to the pinned block: in stream order / and wait for them
inline void fetch(hipStream_t s, int* h, const void* src, int n = 1) { IPXK_HIP(hipMemcpyAsync(h, src, n * sizeof(int), hipMemcpyDeviceToHost, s)); }
inline void read_back(hipStream_t s, int* h, const void* src, int n = 1) {
    fetch(s, h, src, n);
    IPXK_HIP(hipStreamSynchronize(s));
}

// ---- the dense LU of the bump (lu_dense.hip) ------------------------------------------------------
// its workspaces, kept from one call to the next (grow-only)
struct LuDenseWork {
    DevBuf<double> D;                  // column-major kb x kb
    DevBuf<int> brstep, bcstep, bstep, prow, pcol;      // (struct Dense, lu_dense.hip)
    DevBuf<double> ubuf;               // [kPanel][kb] the outer panel's rows of U, contiguous (MFMA trailing update)
    DevBuf<double> usub;               // [sub-panel pivot][kPanel] a sub-panel's rows of U in the rest of the outer panel
    DevBuf<double> coop_slots;         // cooperative outer panel: the workgroups' messages, [5][kCoopMaxG][kCoopSlot]
    DevBuf<unsigned> coop_bar;         // [1] abort flag
    DevBuf<unsigned long long> coop_xcc;   // placement check of the one-XCD form
    unsigned coop_epoch = 0;
    // look-ahead: the trailing update beyond the next outer panel runs on a second stream
    hipStream_t s2 = nullptr;
    hipEvent_t ev_rows[2] = {nullptr, nullptr}, ev_trail[2] = {nullptr, nullptr};
    ~LuDenseWork() {
        for (hipEvent_t e : {ev_rows[0], ev_rows[1], ev_trail[0], ev_trail[1]}) if (e) (void)hipEventDestroy(e);
        if (s2) (void)hipStreamDestroy(s2);
    }
};
// Factorizes the kb x kb block W.D in place (brstep / bcstep = -1, bstep = 0 on entry; kb > 0) and returns the number of its
// pivots; `h`: the pinned read-back block.
int lu_dense_factorize(hipStream_t s, LuDenseWork& W, int kb, double abstol, const LuPolicy& P, int* h);

}  // namespace ipxk
