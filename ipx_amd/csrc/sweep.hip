// The level-scheduled triangular sweeps of the basis-preconditioned operator (trisolve.hip): the sweep kernel, the
// launch plan, the pair of sweeps with the dense bump between them.
//   TriangularSolve / ForwardSolve / BackwardSolve   reference src/sparse_matrix.cc:224-311
//
// Triangular solves are level-scheduled gather sweeps WITHOUT a launch or a barrier per level.  For
// each of the four sweeps (U', L', L, U) Prepare computes the dependency level of every unknown and
// packs the rows level by level into chunks of one wavefront's work (prepare_device.hip).  A sweep
// is out of place and single-assignment: the result vector is pre-filled with a sentinel, every
// unknown is stored exactly once with one 8-byte store, and a consumer polls the values it needs
// with L1-bypassing loads until they differ from the sentinel -- the value IS the ready flag, no
// flags, no fences, no atomics.  Wavefront w of W resident wavefronts owns chunks w, w+W, w+2W, ...
// of the level-ordered chunk sequence; a chunk depends only on chunks before it, so the lowest
// unfinished chunk can always proceed: no deadlock whatever the dispatch order or placement.  While
// a wavefront waits for the dependencies of its chunk, the records of its next chunk are already in
// flight, so a level costs about one store-to-load hand-off (~1 us chip-wide) instead of a kernel
// boundary plus three dependent round trips (~6 us).  Runs of narrow levels are confined to the
// workgroups of ONE XCD, whose L2 then carries the hand-off (~0.6 us per level); see
// sweep_run_kernel for how that stays independent of the actual placement.
// Every row is summed in the reference's order:
//   transposed sweeps ('t'):  d = sum x[i]*a (ascending storage order); x = (x - d)/diag
//   forward sweeps   ('n'):   x -= a*x_j one at a time in the reference's column order
// so a sweep reproduces the reference's arithmetic (bit-exact given identical factors).
#include "context.hpp"
#include "trisolve.hpp"

namespace ipxk {

// ---------------------------------------------------------------------------
// sweep kernel
// ---------------------------------------------------------------------------
using gu64 = unsigned long long;
constexpr gu64 kSentinel = 0x7FF8DEAD5EEDBEEFull;   // a quiet NaN nobody computes
constexpr gu64 kPlainNan = 0x7FF8000000000000ull;
constexpr int kSpinLimit = 1 << 22;                 // polls (>= 0.2 us each) before a wave gives up

constexpr int kSweepGrid = 256;      // workgroups of an all-XCD run (one per CU: all resident)
constexpr int kSweepXcdWgs = 32;     // participating workgroups of a one-XCD run (one per CU of an XCD)
constexpr int kNarrowLevel = 96;     // levels of up to this many chunks may join a one-XCD run
constexpr int kMinXcdLevels = 10;    // shorter runs of narrow levels are not worth a launch of their own (4 until round 3: with the
                                     // inverted blocks below, the 6-10 level runs left next to them cost 5-10 us more than they saved)

__device__ __forceinline__ gu64 load_sc1(const gu64* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // bypasses L1, served by L2 / fabric
}

// What one lane needs for its part of a chunk; loaded one chunk ahead of use.
struct LaneRec {
    int src;        // index of the right-hand side in the input vector (-1: padding)
    int len;        // entries of the row
    int sub;        // merged chunks: which of the chunk's levels the row belongs to
    int dst2;       // second destination of the result (SweepView::dst2), -1: none
    double dg, xr;
    int j[8];       // dependency positions
    double a[8];
};

// long chunks: step of the row at which the FIRST round of 8 steps starts (0, or the last 8 steps when the
// rounds are taken from the end of the row)
__device__ __forceinline__ int first_round_step(const SweepView& S, const ChunkDesc& d) {
    return (d.width < -8 && S.newest_first && d.sub <= 1) ? -d.width - 8 : 0;
}

__device__ __forceinline__ void load_rec(LaneRec& R, const SweepView& S, const ChunkDesc& d, int lane,
                                         const double* __restrict__ xin) {
    // every address depends on the (scalar) descriptor only: one round trip, fully coalesced
    const int pos = d.width >= 0 ? d.pos0 + lane : d.pos0 + (lane >> 3);
    R.src = S.src[pos];
    R.dst2 = S.dst2 ? S.dst2[pos] : -1;
    R.dg = S.diag[pos];
    const int lenword = S.len[pos];
    R.len = lenword & ((1 << kLenBits) - 1);
    R.sub = lenword >> kLenBits;
    const int steps = d.width >= 0 ? d.width : min(-d.width, 8);     // wave-uniform
    const int ent = d.ent0 + first_round_step(S, d) * 64;            // scalar
#pragma unroll
    for (int e = 0; e < 8; e++) {
        R.j[e] = 0; R.a[e] = 0.0;
        if (e < steps) {
            R.j[e] = S.idx[ent + e * 64 + lane];
            R.a[e] = S.val[ent + e * 64 + lane];
        }
    }
    R.xr = R.src >= 0 ? xin[R.src] : 0.0;
}

// ---- how results travel from the wavefront that computes them to the wavefronts that need them ----
// (the value is the flag in every case: a slot holds the sentinel until its one and only store)
// Through memory: every look at a dependency bypasses L1; results are stored write-through, or with plain
// stores that stay in the XCD's L2 when all workgroups of the launch are known to share one XCD.
struct HandGlobal {
    const gu64* xo; double* xout; bool plain_store; double* out2;
    __device__ __forceinline__ gu64 look(int pj) const { return load_sc1(xo + pj); }
    __device__ __forceinline__ void store(int pos, gu64 out) const {
        if (plain_store) __hip_atomic_store(reinterpret_cast<gu64*>(xout) + pos, out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else __hip_atomic_store(reinterpret_cast<gu64*>(xout) + pos, out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
// first look at the dependencies of the lane's (up to 8) entries starting at entry `first`; dependencies at
// positions [lo, hi) belong to the (merged) chunk itself and travel through lane shuffles instead
template <class Hand>
__device__ __forceinline__ void issue_polls(const LaneRec& R, bool ell, int gl, int first, const Hand& H, gu64 (&bits)[8],
                                            int lo = 0, int hi = 0) {
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const int e = ell ? t : first + t * 8 + gl;
        bits[t] = 0ull;
        if (R.src >= 0 && e >= 0 && e < R.len && !(R.j[t] >= lo && R.j[t] < hi)) bits[t] = H.look(R.j[t]);
    }
}

// polls until every dependency holds a value; false on timeout (abort raised)
template <class Hand>
__device__ __forceinline__ bool wait_polls(const LaneRec& R, const Hand& H, gu64 (&bits)[8], int* abort_flag) {
    int spins = 0;
    for (;;) {
        bool ok = true;
#pragma unroll
        for (int t = 0; t < 8; t++) ok &= bits[t] != kSentinel;
        if (__all(ok)) return true;
        __builtin_amdgcn_s_sleep(1);
#pragma unroll
        for (int t = 0; t < 8; t++)
            if (bits[t] == kSentinel) bits[t] = H.look(R.j[t]);
        if (++spins > kSpinLimit ||
            ((spins & 255) == 0 && __hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
            __hip_atomic_store(abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
    }
}

template <class Hand>
__device__ __forceinline__ void store_result(const Hand& H, int pos, double res, int dst2 = -1) {
    gu64 out = (gu64)__double_as_longlong(res);
    if (out == kSentinel) out = kPlainNan;     // a result must never look unfinished
    H.store(pos, out);
    if (dst2 >= 0) H.out2[dst2] = res;         // second copy for the kernel AFTER this launch: a plain store
}

// value of lane (this lane + N) of the same 16-lane row (DPP row_shl:N); lanes whose source lies outside
// the row keep their own value
template <int N>
__device__ __forceinline__ double row_shift_left(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(lo, lo, 0x100 + N, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, 0x100 + N, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// acc -= / += the products held by the first `cnt` lanes of the 8-lane group, one at a time in lane
// order.  Only the group's FIRST lane ends up with the sum: it fetches its neighbours' products with DPP
// row shifts (plain VALU moves, no LDS crossbar as a shuffle would need; an aligned group of 8 never
// leaves its 16-lane row), then adds them in order.
template <bool RUNNING>
__device__ __forceinline__ double ordered_combine(double acc, double prod, int cnt) {
    double v[kLongLanes];
    v[0] = prod;
    v[1] = row_shift_left<1>(prod); v[2] = row_shift_left<2>(prod); v[3] = row_shift_left<3>(prod);
    v[4] = row_shift_left<4>(prod); v[5] = row_shift_left<5>(prod); v[6] = row_shift_left<6>(prod);
    v[7] = row_shift_left<7>(prod);
#pragma unroll
    for (int t = 0; t < kLongLanes; t++)
        if (t < cnt) acc = RUNNING ? acc - v[t] : acc + v[t];
    return acc;
}

// A MERGED chunk (trisolve.hpp): `sub` consecutive tiny levels in one chunk.  The dependencies outside the
// chunk have been polled (bits); the wavefront runs the levels in order, every lane recomputes its row in every
// round and keeps the value of the round that is its own level -- by then all its dependencies inside the chunk
// (rows of earlier levels: other lanes of this wavefront) hold their results, which travel by lane shuffles.
// Each row is still summed in its own order: bit-identical to the unmerged form.
template <bool RUNNING, class Hand>
__device__ __forceinline__ void solve_merged(const LaneRec& R, const ChunkDesc& d, int lane, const Hand& H, const gu64 (&bits)[8]) {
    const bool ell = d.width >= 0;
    const int gl = lane & 7;
    const int npos = ell ? 64 : kLongLanes;
    const int len = R.src >= 0 ? R.len : 0;
    double result = 0.0;
    const int steps = ell ? d.width : min(-d.width, 8);            // wave-uniform: entries (ELL) / steps of 8 (long rows)
    // where each dependency comes from: a lane of this wavefront (rows of earlier levels of the chunk) or memory
    int from[8];
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const int e = ell ? t : t * 8 + gl;
        const int off = R.j[t] - d.pos0;
        from[t] = (t < steps && e < len && off >= 0 && off < npos) ? (ell ? off : off << 3) : -1;
    }
    for (int s = 0; s < d.sub; s++) {
        // all shuffles of the round are issued before the first use, so their latencies overlap
        double xin[8];
#pragma unroll
        for (int t = 0; t < 8; t++)
            if (t < steps) xin[t] = __shfl(result, from[t] >= 0 ? from[t] : lane, 64);
        double acc = RUNNING ? R.xr : 0.0;
#pragma unroll
        for (int t = 0; t < 8; t++) {
            if (t >= steps) break;                                  // wave-uniform
            const int e = ell ? t : t * 8 + gl;
            double prod = 0.0;
            if (e < len) {
                const double xj = from[t] >= 0 ? xin[t] : __longlong_as_double((long long)bits[t]);
                prod = RUNNING ? R.a[t] * xj : xj * R.a[t];
            }
            if (ell) { if (e < len) acc = RUNNING ? acc - prod : acc + prod; }
            else acc = ordered_combine<RUNNING>(acc, prod, min(kLongLanes, len - t * 8));
        }
        if (R.sub == s && (ell || gl == 0)) result = R.src >= 0 ? (RUNNING ? acc : R.xr - acc) / R.dg : 0.0;
    }
    if (ell) store_result(H, d.pos0 + lane, result, R.dst2);
    else if (gl == 0) store_result(H, d.pos0 + (lane >> 3), result, R.dst2);
}

// solves the chunk whose records are in R (first look at the dependencies already issued into bits);
// false on timeout
template <bool RUNNING, bool MERGED, class Hand>
__device__ __forceinline__ bool solve_chunk(LaneRec& R, const ChunkDesc& d, int lane, const SweepView& S, const Hand& H,
                                            gu64 (&bits)[8], int* abort_flag) {
    const bool ell = d.width >= 0;
    if (!wait_polls(R, H, bits, abort_flag)) return false;
    if (MERGED && d.sub > 1) { solve_merged<RUNNING>(R, d, lane, H, bits); return true; }
    if (ell) {
        double acc = RUNNING ? R.xr : 0.0;
#pragma unroll
        for (int e = 0; e < 8; e++)
            if (e < R.len) {
                const double xj = __longlong_as_double((long long)bits[e]);
                const double prod = RUNNING ? R.a[e] * xj : xj * R.a[e];
                acc = RUNNING ? acc - prod : acc + prod;
            }
        // padding positions get a value too (1 wavefront = 1 contiguous store; nobody depends on them)
        store_result(H, d.pos0 + lane, R.src >= 0 ? (RUNNING ? acc : R.xr - acc) / R.dg : 0.0, R.dst2);
        return true;
    }
    const int gl = lane & 7;
    const int len = R.src >= 0 ? R.len : 0;
    double acc = RUNNING ? R.xr : 0.0;
    if (first_round_step(S, d) == 0) {
        for (int first = 0;;) {          // 64 entries of the row per round (one round unless the row is longer)
#pragma unroll
            for (int t = 0; t < 8; t++) {
                const int e0 = first + t * 8;                   // first entry of this step of the group
                if (!__any(e0 < len)) break;                    // wave-uniform
                double prod = 0.0;
                if (e0 + gl < len) {
                    const double xj = __longlong_as_double((long long)bits[t]);
                    prod = RUNNING ? R.a[t] * xj : xj * R.a[t];
                }
                acc = ordered_combine<RUNNING>(acc, prod, min(kLongLanes, len - e0));
            }
            first += 64;
            if (!__any(first < len)) break;
#pragma unroll
            for (int t = 0; t < 8; t++) {
                const int step = first / 8 + t;                 // wave-uniform
                R.j[t] = 0; R.a[t] = 0.0;
                if (step < -d.width) { R.j[t] = S.idx[d.ent0 + step * 64 + lane]; R.a[t] = S.val[d.ent0 + step * 64 + lane]; }
            }
            issue_polls(R, false, gl, first, H, bits);
            if (!wait_polls(R, H, bits, abort_flag)) return false;
        }
    } else {
        // rounds from the END of the row (SweepView::newest_first, rows of more than 64 entries): all rounds but
        // the last one wait for unknowns that were solved long ago
        const int nsteps = -d.width;
        for (int base = nsteps - 8;;) {
#pragma unroll
            for (int t = 0; t < 8; t++) {
                const int e0 = (base + t) * 8;
                if (e0 < 0 || !__any(e0 < len)) continue;       // wave-uniform
                double prod = 0.0;
                if (e0 + gl < len) {
                    const double xj = __longlong_as_double((long long)bits[t]);
                    prod = RUNNING ? R.a[t] * xj : xj * R.a[t];
                }
                acc = ordered_combine<RUNNING>(acc, prod, min(kLongLanes, len - e0));
            }
            base -= 8;
            if (base <= -8) break;
#pragma unroll
            for (int t = 0; t < 8; t++) {
                const int step = base + t;                      // wave-uniform
                R.j[t] = 0; R.a[t] = 0.0;
                if (step >= 0) { R.j[t] = S.idx[d.ent0 + step * 64 + lane]; R.a[t] = S.val[d.ent0 + step * 64 + lane]; }
            }
            issue_polls(R, false, gl, base * 8, H, bits);
            if (!wait_polls(R, H, bits, abort_flag)) return false;
        }
    }
    if (gl == 0) store_result(H, d.pos0 + (lane >> 3), R.src >= 0 ? (RUNNING ? acc : R.xr - acc) / R.dg : 0.0, R.dst2);
    return true;
}

__device__ __forceinline__ ChunkDesc scalar_desc(const ChunkDesc& v) {   // wave-uniform (scalar) values
    ChunkDesc d;
    d.pos0 = __builtin_amdgcn_readfirstlane(v.pos0);
    d.ent0 = __builtin_amdgcn_readfirstlane(v.ent0);
    d.width = __builtin_amdgcn_readfirstlane(v.width);
    d.npos = v.npos;
    d.sub = __builtin_amdgcn_readfirstlane(v.sub);
    return d;
}

// the wavefront's chunks c, c + NW, ... < c1; A holds the records of chunk c (descriptor d), dn is the
// descriptor of chunk c + NW
// (Round 3, measured and dropped: THREE chunks in flight per wavefront -- the first look at the dependencies of chunk
// c + NW and its right-hand side issued before chunk c waits, the records of chunk c + 2 NW behind them.  The wide
// levels move 11 G unknowns/s = 6.5 us per chunk and wavefront, which looks like a lack of overlapped round trips;
// but the deeper pipeline made both pairs slower, backward 272 -> 288 us, forward 300 -> 314 us.)
template <bool RUNNING, bool MERGED, class Hand>
__device__ __forceinline__ void chunk_loop(const SweepView& S, int c, int c1, int NW, int lane, const double* __restrict__ xin,
                                           const Hand& H, LaneRec& A, ChunkDesc d, ChunkDesc dn, int* abort_flag) {
    LaneRec B;
    for (;;) {
        gu64 bits[8];
        const int own = MERGED && d.sub > 1 ? (d.width >= 0 ? 64 : kLongLanes) : 0;     // merged: the chunk's own positions
        issue_polls(A, d.width >= 0, lane & 7, d.width >= 0 ? 0 : first_round_step(S, d) * 8, H, bits, d.pos0, d.pos0 + own);
        // the next chunk's records (and the descriptor after that) travel while this chunk waits
        const int cn = c + NW;
        ChunkDesc dnn = dn;
        if (cn < c1) {
            load_rec(B, S, dn, lane, xin);
            if (cn + NW < c1) dnn = scalar_desc(S.chunks[cn + NW]);
        }
        if (!solve_chunk<RUNNING, MERGED>(A, d, lane, S, H, bits, abort_flag)) return;
        if (cn >= c1) return;
        A = B; d = dn; dn = dnn; c = cn;
    }
}

// One run of consecutive levels = chunks [c0, c1) of a sweep.
// xcd_mode == 0: every workgroup takes part; results are stored write-through.
// xcd_mode == 1: only the workgroups with blockIdx % 8 == 0 take part -- under the round-robin
//   dispatch of gfx950 they share one XCD, whose L2 then serves the polls, and results are stored
//   with plain stores that stay in that L2.  That placement is an observation, not a contract, so
//   it is CHECKED: every participant publishes the id of the XCD it runs on (HW_REG_XCC_ID) and
//   reads everybody else's; only if all agree are plain stores used, otherwise every participant
//   falls back to write-through stores (all participants see the same ids and decide alike).
//   Correctness therefore never depends on where workgroups land, only the speed does.
// MERGED: the run contains merged chunks (the lean instantiation without that path serves all other runs)
template <bool RUNNING, bool MERGED>
__global__ __launch_bounds__(kBlock) void sweep_run_kernel(SweepView S, int c0, int c1, const double* __restrict__ xin,
                                                           double* xout, int xcd_mode, unsigned epoch, gu64* xcc_slots,
                                                           int* abort_flag, const int* done) {
    if (xcd_mode && (blockIdx.x & 7)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int part = xcd_mode ? blockIdx.x >> 3 : blockIdx.x;
    const int nparts = xcd_mode ? (gridDim.x + 7) >> 3 : gridDim.x;
    const int gw = part * (kBlock / 64) + wave, NW = nparts * (kBlock / 64);
    const gu64* xo = reinterpret_cast<const gu64*>(xout);
    int c = c0 + gw;
    const bool active = c < c1;
    // the first two descriptors travel while the `done` flag is read
    ChunkDesc raw = S.chunks[active ? c : c0], rawn = S.chunks[c + NW < c1 ? c + NW : c0];
    if (done && *done) return;
    unsigned xcc = 0;
    if (xcd_mode && wave == 0) {
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        xcc &= 0xff;
        if (lane == 0) __hip_atomic_store(xcc_slots + part, ((gu64)epoch << 32) | xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    ChunkDesc d = scalar_desc(raw), dn = scalar_desc(rawn);
    LaneRec A;
    if (active) load_rec(A, S, d, lane, xin);            // in flight during the placement check
    bool plain = false;
    if (xcd_mode) {
        __shared__ int same_xcd;
        if (wave == 0) {
            bool same = true;
            for (int i = lane; i < nparts; i += 64) {
                gu64 v;
                int spins = 0;
                while (((v = load_sc1(xcc_slots + i)) >> 32) != epoch) {
                    __builtin_amdgcn_s_sleep(1);
                    if (++spins > kSpinLimit) { __hip_atomic_store(abort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
                }
                same &= (unsigned)(v & 0xff) == xcc && (v >> 32) == epoch;
            }
            same = __all(same);
            if (lane == 0) same_xcd = same ? 1 : 0;
        }
        __syncthreads();
        plain = same_xcd != 0;
    }
    if (!active) return;
    const HandGlobal H{xo, xout, plain, S.out2};
    chunk_loop<RUNNING, MERGED>(S, c, c1, NW, lane, xin, H, A, d, dn, abort_flag);
}

// pre-fills the result vectors of up to four sweeps with the sentinel
struct FillList { gu64* p[4]; int n[4]; };
__global__ void fill_sentinel_kernel(FillList L, const int* done) {
    if (done && *done) return;
#pragma unroll
    for (int k = 0; k < 4; k++)
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L.n[k]; i += gridDim.x * blockDim.x) L.p[k][i] = kSentinel;
}

// out[i] = in[perm[i]]
__global__ void gather_perm_kernel(int m, const double* __restrict__ in, const int* __restrict__ perm,
                                   double* __restrict__ out, const int* done) {
    if (done && *done) return;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x)
        out[i] = in[perm[i]];
}
// out[perm[i]] = in[i]
__global__ void scatter_perm_kernel(int m, const double* __restrict__ in, const int* __restrict__ perm,
                                    double* __restrict__ out, const int* done) {
    if (done && *done) return;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x)
        out[perm[i]] = in[i];
}
// a sweep's result (by position) into index order: out[perm ? perm[k] : k] = y[posof[k]]
__global__ void unpack_result_kernel(int m, const double* __restrict__ y, const int* __restrict__ posof,
                                     const int* __restrict__ perm, double* __restrict__ out) {
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < m; k += gridDim.x * blockDim.x)
        out[perm ? perm[k] : k] = y[posof[k]];
}

// ---------------------------------------------------------------------------
// launch plan and sweeps
// ---------------------------------------------------------------------------
// Levels of at most kNarrowLevel chunks are "narrow"; a run of at least kMinXcdLevels narrow levels becomes
// a one-XCD launch, everything between two such runs one all-XCD launch.
// (Measured and dropped: runs of very narrow levels on ONE workgroup with the hand-off through LDS -- the
// hand-off itself is 5x cheaper, but one CU streams the runs' records at 25-50 GB/s and the C3 iteration
// got 70-200 us slower.)
void plan_sweep(Sweep& S, bool level_launches) {
    S.plan.clear();
    const int nlev = S.tail.K > 0 ? S.tail.la : S.nlevels;        // an inverted tail takes the levels from la on,
    const int lfirst = S.head.K > 0 ? S.head.lb : 0;              // an inverted head the levels below lb
    if (nlev == 0) return;
    auto push = [&](int l0, int l1, int kind) {
        const int c0 = S.level_chunk[l0], c1 = S.level_chunk[l1];
        if (c1 > c0) S.plan.push_back({c0, c1, kind, S.merged_prefix[c1] > S.merged_prefix[c0]});
    };
    if (level_launches) {
        for (int l = 0; l < nlev; l++) push(l, l + 1, Sweep::kAllXcds);
        return;
    }
    int narrow_max = kNarrowLevel, min_levels = kMinXcdLevels;
    if (const char* e = getenv("IPXK_SWEEP_NARROW")) narrow_max = atoi(e);
    if (const char* e = getenv("IPXK_SWEEP_MINLEVELS")) min_levels = std::max(1, atoi(e));
    auto nchunks = [&](int lv) { return S.level_chunk[lv + 1] - S.level_chunk[lv]; };
    std::vector<unsigned char> kind(nlev, Sweep::kAllXcds);
    for (int l = lfirst; l < nlev;) {
        if (nchunks(l) > narrow_max) { l++; continue; }
        int b = l;
        while (b < nlev && nchunks(b) <= narrow_max) b++;
        if (b - l >= min_levels) for (int t = l; t < b; t++) kind[t] = Sweep::kOneXcd;
        l = b;
    }
    for (int l = lfirst; l < nlev;) {
        int b = l + 1;
        while (b < nlev && kind[b] == kind[l]) b++;
        push(l, b, kind[l]);
        if (getenv("IPXK_SWEEP_STATS")) {
            int64_t unknowns = 0;
            for (int t = l; t < b; t++) unknowns += S.level_width[t];
            fprintf(stderr, "ipxk: sweep plan: levels %d..%d %s, %d chunks, %lld unknowns; widths", l, b - 1, kind[l] == Sweep::kOneXcd ? "one XCD" : "all XCDs",
                    S.level_chunk[b] - S.level_chunk[l], (long long)unknowns);
            for (int t = l; t < b; t++) fprintf(stderr, " %d", S.level_width[t]);
            fprintf(stderr, "\n");
        }
        l = b;
    }
}

// runs the sweep on the input vector xin (addressed through S.src); the result goes to S.y, which must
// hold the sentinel in every position (fill_results)
static void run_sweep(Context* c, const Sweep& S, bool scaled, const double* xin, const int* done,
                      const int* dst2 = nullptr, double* out2 = nullptr) {
    SplitOperator* sp = c->split;
    SweepView V = S.view(scaled);
    V.dst2 = dst2; V.out2 = out2;
    double* xout = S.y.get();
    // Every workgroup of a run must be resident (a wavefront may wait for a chunk that another workgroup of
    // the same launch owns): never launch more workgroups than the device holds at once.  One block per CU
    // is held back from what the occupancy query reports (it over-reports by one for some kernels).
    // (per operator, i.e. per context and device; the smallest occupancy of the four instantiations counts.  Two
    // contexts must not run basis sweeps on ONE device at the same time: their workgroups would compete for the
    // residency each of them assumes -- a violation ends in the bounded spin's time-out error, not in a hang.)
    if (sp->sweep_grid_all == 0) {
        const char* e = getenv("IPXK_SWEEP_GRID");
        int want = e && atoi(e) > 0 ? atoi(e) : kSweepGrid;
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) {
            int per_cu = 1 << 30, got = 0;
            auto ask = [&](auto kernel) {
                int v = 0;
                if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kernel, kBlock, 0) == hipSuccess) { per_cu = std::min(per_cu, v); got++; }
            };
            ask(sweep_run_kernel<true, true>); ask(sweep_run_kernel<true, false>);
            ask(sweep_run_kernel<false, true>); ask(sweep_run_kernel<false, false>);
            if (got == 4) want = std::max(1, std::min(want, prop.multiProcessorCount * std::max(1, per_cu - 1)));
        }
        sp->sweep_grid_all = want;
    }
    if (S.head.K > 0) run_block(c, S, S.head, V, scaled, xin, done);
    const int grid_all = sp->sweep_grid_all;
    static const int wgs_xcd = [] { const char* e = getenv("IPXK_SWEEP_XCD_WGS"); return e && atoi(e) > 0 ? std::min(atoi(e), 64) : kSweepXcdWgs; }();
    for (const Sweep::Launch& L : S.plan) {
        const bool one_xcd = L.kind == Sweep::kOneXcd;
        const int need = (L.c1 - L.c0 + kBlock / 64 - 1) / (kBlock / 64);     // workgroups with a chunk per wave
        int grid = std::max(1, std::min(need, one_xcd ? wgs_xcd : grid_all));
        unsigned epoch = 0;
        if (one_xcd) { grid *= 8; epoch = ++sp->epoch; if (epoch == 0) epoch = ++sp->epoch; }
        auto kernel = S.running ? (L.merged ? sweep_run_kernel<true, true> : sweep_run_kernel<true, false>)
                                : (L.merged ? sweep_run_kernel<false, true> : sweep_run_kernel<false, false>);
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), 0, c->stream, V, L.c0, L.c1, xin, xout, one_xcd ? 1 : 0, epoch,
                           sp->xcc_slots.get(), sp->abort_flag.get(), done);
    }
    if (S.tail.K > 0) run_block(c, S, S.tail, V, scaled, xin, done);
}

void run_pair(Context* c, const Sweep& first, const Sweep& second, bool trans, bool scaled, const double* xin, const int* done,
              const int* dst2, double* out2) {
    run_sweep(c, first, scaled, xin, done);
    bump_between(c, trans, first.y.get(), done);
    run_sweep(c, second, scaled, first.y.get(), done, dst2, out2);
}

void fill_results(Context* c, std::initializer_list<const Sweep*> sweeps, const int* done) {
    FillList L{};
    int k = 0, most = 1;
    for (const Sweep* S : sweeps) { L.p[k] = reinterpret_cast<gu64*>(S->y.get()); L.n[k] = S->npos; most = std::max(most, S->npos); k++; }
    hipLaunchKernelGGL(fill_sentinel_kernel, dim3(vec_grid(most)), dim3(kBlock), 0, c->stream, L, done);
}

void unpack_result(Context* c, const Sweep& S, const int* perm, double* out) {
    const int m = c->split->m;
    hipLaunchKernelGGL(unpack_result_kernel, dim3(vec_grid(m)), dim3(kBlock), 0, c->stream, m, S.y.get(), S.posof.get(),
                       perm, out);
}
void gather_perm(Context* c, const double* in, const int* perm, double* out, const int* done) {
    const int m = c->split->m;
    hipLaunchKernelGGL(gather_perm_kernel, dim3(vec_grid(m)), dim3(kBlock), 0, c->stream, m, in, perm, out, done);
}
void scatter_perm(Context* c, const double* in, const int* perm, double* out, const int* done) {
    const int m = c->split->m;
    hipLaunchKernelGGL(scatter_perm_kernel, dim3(vec_grid(m)), dim3(kBlock), 0, c->stream, m, in, perm, out, done);
}

// ForwardSolve: L then U (sparse_matrix.cc:303-306) on a vector in index order; in may be out.
// (The L sweep reads its right-hand side through rowperm, see split_prepare_host: undo that here.)
void forward_solve_dev(Context* c, const double* in, double* out, bool scaled, const int* done) {
    SplitOperator* S = c->split;
    scatter_perm(c, in, S->rowperm.get(), S->w3.get(), done);
    fill_results(c, {&S->Lf, &S->Uf}, done);
    run_pair(c, S->Lf, S->Uf, false, scaled, S->w3.get(), done);
    unpack_result(c, S->Uf, nullptr, out);
}
// BackwardSolve: U' then L' (sparse_matrix.cc:308-311); in may be out
void backward_solve_dev(Context* c, const double* in, double* out, bool scaled, const int* done) {
    SplitOperator* S = c->split;
    fill_results(c, {&S->Ut, &S->Lt}, done);
    run_pair(c, S->Ut, S->Lt, true, scaled, in, done);
    unpack_result(c, S->Lt, nullptr, out);
}

// raises if a sweep gave up waiting for a dependency (host side, after the stream has been synchronized)
void check_sweep_abort(Context* c) {
    SplitOperator* S = c->split;
    if (!S) return;
    int flag = 0;
    S->abort_flag.download(&flag, 1, c->stream);
    IPXK_HIP(hipStreamSynchronize(c->stream));
    if (flag) {
        IPXK_HIP(hipMemsetAsync(S->abort_flag.get(), 0, sizeof(int), c->stream));
        throw Error(IPXK_E_HIP, "triangular sweep timed out waiting for a dependency");
    }
}

void split_levels(const Context* c, ipxint levels[4]) {
    levels[0] = c->split->Ut.nlevels;
    levels[1] = c->split->Lt.nlevels;
    levels[2] = c->split->Lf.nlevels;
    levels[3] = c->split->Uf.nlevels;
}

}  // namespace ipxk
