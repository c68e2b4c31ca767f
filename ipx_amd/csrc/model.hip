// The model on the device (round 4).
//
// The reference's NormalMatrix stores a reference to the model and copies nothing (src/normal_matrix.h:20-27), so
// constructing a KKT solver is free; rounds 1-3 built every layout of the model matrix with single-threaded host
// loops (transpose, bucketing, std::sort per tile: 3.2 s at 1M x 2M, per solver object).  Here the matrix is uploaded
// once as it is (CSC, 64-bit indices), narrowed and validated, transposed by a radix sort, and both gather matrices get
// their layouts from the device builders (build_model; layout_device.hip) -- from the host builders (layout_host.hip), on
// host copies fetched on demand, only where those decline.  Also here: the dense-column classification.
#include <algorithm>
#include <chrono>
#include <cstdio>

#include "layout_scratch.hpp"

namespace ipxk {

namespace {
__global__ void narrow_kernel(int64_t nz, const ipxint* __restrict__ in, int* __restrict__ out, int limit, int* bad) {
    IPXK_GRID_STRIDE(p, nz) {
        const ipxint v = in[p];
        if (v < 0 || v >= limit) *bad = 1;
        out[p] = (int)v;
    }
}
// column (row of the gather matrix) and position of every entry, enumerated row by row
__global__ void rowof_kernel(int nrows, const int* __restrict__ ptr, int* __restrict__ rowof, unsigned* __restrict__ pos) {
    IPXK_GRID_STRIDE(r, nrows)
        for (int p = ptr[r]; p < ptr[r + 1]; p++) { rowof[p] = (int)r; if (pos) pos[p] = (unsigned)p; }
}
__global__ void gather_transposed_kernel(int64_t nz, const unsigned* __restrict__ perm, const int* __restrict__ colof,
                                         const double* __restrict__ Ax, int* __restrict__ Ti, double* __restrict__ Tx) {
    IPXK_GRID_STRIDE(t, nz) {
        const unsigned p = perm[t];
        Ti[t] = colof[p];
        Tx[t] = Ax[p];
    }
}
__global__ void row_pointers_kernel(int64_t m, int64_t nz, const unsigned* __restrict__ sorted_rows, int* __restrict__ Tp) {
    IPXK_GRID_STRIDE(i, m + 1) {
        int64_t lo = 0, hi = nz;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (sorted_rows[mid] < (unsigned)i) lo = mid + 1; else hi = mid; }
        Tp[i] = (int)lo;
    }
}
__global__ void max_len_kernel(int nrows, const int* __restrict__ ptr, int* out) {
    int best = 0;
    IPXK_GRID_STRIDE(r, nrows) best = max(best, ptr[r + 1] - ptr[r]);
    best = wave_max(best);
    if ((threadIdx.x & 63) == 0 && best > 0) atomicMax(out, best);
}
// hist[len] += 1 for every row (maxcnt: the largest len).  The rows of a sparse matrix share a handful of lengths, so those below
// kHistLds are counted per workgroup in LDS first, not with one global atomic per row on those few addresses.
constexpr int kHistLds = 256;
__global__ __launch_bounds__(kBlock) void count_histogram_kernel(int nrows, const int* __restrict__ ptr, int maxcnt, int* hist) {
    __shared__ int sh[kHistLds];
    for (int k = threadIdx.x; k < kHistLds; k += kBlock) sh[k] = 0;
    __syncthreads();
    IPXK_GRID_STRIDE(r, nrows) {
        const int len = ptr[r + 1] - ptr[r];
        if (len < kHistLds) atomicAdd(sh + len, 1); else atomicAdd(hist + len, 1);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kHistLds && k <= maxcnt; k += kBlock)
        if (sh[k]) atomicAdd(hist + k, sh[k]);
}
// the rows of at least `len` entries, in no particular order (cap of them: the caller knows how many there are)
__global__ void rows_at_least_kernel(int nrows, const int* __restrict__ ptr, int len, int cap, int* count, int* __restrict__ list) {
    IPXK_GRID_STRIDE(r, nrows)
        if (ptr[r + 1] - ptr[r] >= len) {
            const int k = atomicAdd(count, 1);
            if (k < cap) list[k] = (int)r;
        }
}
// entries of a list of columns, one after the other (dense columns: precond.hip)
__global__ void gather_columns_kernel(int k, const int* __restrict__ cols, const int* __restrict__ off, const int* __restrict__ Ap,
                                      const int* __restrict__ Ai, const double* __restrict__ Ax, ipxint* __restrict__ out_i, double* __restrict__ out_x) {
    const int kk = blockIdx.x;
    if (kk >= k) return;
    const int j = cols[kk], p0 = Ap[j], len = Ap[j + 1] - p0, o = off[kk];
    for (int t = threadIdx.x; t < len; t += blockDim.x) { out_i[o + t] = Ai[p0 + t]; out_x[o + t] = Ax[p0 + t]; }
}
__global__ void narrow_plain_kernel(int64_t len, const ipxint* __restrict__ in, int* __restrict__ out) { IPXK_GRID_STRIDE(p, len) out[p] = (int)in[p]; }
__global__ void widen_kernel(int64_t len, const int* __restrict__ in, ipxint* __restrict__ out) { IPXK_GRID_STRIDE(p, len) out[p] = in[p]; }
}  // namespace

void narrow_ints(int64_t len, const ipxint* in, int* out, hipStream_t s) {
    if (len > 0) hipLaunchKernelGGL(narrow_plain_kernel, dim3(gridn(len)), dim3(kBlock), 0, s, len, in, out);
}
void widen_ints(int64_t len, const int* in, ipxint* out, hipStream_t s) {
    if (len > 0) hipLaunchKernelGGL(widen_kernel, dim3(gridn(len)), dim3(kBlock), 0, s, len, in, out);
}

// ---------------------------------------------------------------------------
// the model on the device: CSC and the row-wise copy, 32-bit indices
// ---------------------------------------------------------------------------
void device_row_of_entries(int nrows, const int* ptr, int* rowof, unsigned* pos, hipStream_t s) {
    hipLaunchKernelGGL(rowof_kernel, dim3(gridn(nrows)), dim3(kBlock), 0, s, nrows, ptr, rowof, pos);
}
void device_row_pointers(int64_t nrows, int64_t nz, const unsigned* sorted_rows, int* ptr, hipStream_t s) {
    hipLaunchKernelGGL(row_pointers_kernel, dim3(gridn(nrows + 1)), dim3(kBlock), 0, s, nrows, nz, sorted_rows, ptr);
}
// Transpose (src/sparse_matrix.cc:120-151) of an n-column CSC with m rows: a stable sort by row of the entries enumerated
// column by column leaves every row in ascending source-column order, like the reference's counting sort.  colof: scratch.
// Synchronizes the stream.
void device_transpose(Tmp& T, DevBuf<int>& colof, int64_t n, int64_t m, int64_t nz, const int* Ap, const int* Ai, const double* Ax, int* Tp,
                      int* Ti, double* Tx, hipStream_t s) {
    const size_t nz1 = (size_t)std::max<int64_t>(nz, 1);
    colof.ensure(nz1);
    DevBuf<unsigned> pos(nz1), rows2(nz1), perm(nz1);
    device_row_of_entries((int)n, Ap, colof.get(), pos.get(), s);
    sort_pairs<unsigned>(T, reinterpret_cast<const unsigned*>(Ai), rows2.get(), pos.get(), perm.get(), (size_t)nz, bits_for((u64)std::max<int64_t>(m, 2) - 1), s);
    hipLaunchKernelGGL(gather_transposed_kernel, dim3(gridn(nz)), dim3(kBlock), 0, s, nz, perm.get(), colof.get(), Ax, Ti, Tx);
    device_row_pointers(m, nz, rows2.get(), Tp, s);
    IPXK_HIP(hipStreamSynchronize(s));           // temporaries go out of scope
}

void upload_plain_model(Context* c, const ipxint* Ap, const ipxint* Ai, const double* Ax) {
    const int64_t m = c->m, n = c->n;
    hipStream_t s = c->stream;
    IPXK_REQUIRE(m < (int64_t(1) << 31) - 1 && n < (int64_t(1) << 31) - 1, "dimension exceeds 32-bit device indices");
    IPXK_REQUIRE(Ap[0] == 0, "colptr[0] must be 0");
    const int64_t nz = Ap[n];
    IPXK_REQUIRE(nz >= 0 && nz < (int64_t(1) << 31) - kLongSeg, "nnz exceeds 32-bit device indices");
    c->h_Ap.assign(Ap, Ap + n + 1);
    std::vector<int> ap32((size_t)n + 1);
    for (int64_t j = 0; j < n; j++) {
        IPXK_REQUIRE(Ap[j] <= Ap[j + 1], "colptr not monotone");
        ap32[(size_t)j] = (int)Ap[j];
    }
    ap32[(size_t)n] = (int)nz;
    c->nnz = nz;
    const size_t nz1 = (size_t)std::max<int64_t>(nz, 1);
    c->pl_Ap.upload(ap32, s);
    c->pl_Ai.ensure(nz1); c->pl_Ax.ensure(nz1); c->pl_Tp.ensure((size_t)m + 1); c->pl_Ti.ensure(nz1); c->pl_Tx.ensure(nz1);
    DevBuf<int> bad(1);
    IPXK_HIP(hipMemsetAsync(bad.get(), 0, sizeof(int), s));
    if (nz > 0) {
        DevBuf<ipxint> ai64(nz1);
        ai64.upload(Ai, (size_t)nz, s);
        c->pl_Ax.upload(Ax, (size_t)nz, s);
        hipLaunchKernelGGL(narrow_kernel, dim3(gridn(nz)), dim3(kBlock), 0, s, nz, ai64.get(), c->pl_Ai.get(), (int)m, bad.get());
        int flag = 0;
        IPXK_HIP(hipMemcpyAsync(&flag, bad.get(), sizeof(int), hipMemcpyDeviceToHost, s));
        IPXK_HIP(hipStreamSynchronize(s));           // ai64 goes out of scope
        IPXK_REQUIRE(flag == 0, "row index out of range");
        DevBuf<int> colof;
        Tmp T;
        device_transpose(T, colof, n, m, nz, c->pl_Ap.get(), c->pl_Ai.get(), c->pl_Ax.get(), c->pl_Tp.get(), c->pl_Ti.get(), c->pl_Tx.get(), s);
    } else {
        IPXK_HIP(hipMemsetAsync(c->pl_Tp.get(), 0, ((size_t)m + 1) * sizeof(int), s));
        IPXK_HIP(hipStreamSynchronize(s));
    }
    IPXK_HIP(hipGetLastError());
    c->have_plain = true;
}

// host copies of the entries (64-bit indices) for the paths that still build on the host
void ensure_host_model(Context* c, bool rowwise) {
    hipStream_t s = c->stream;
    const size_t nz = (size_t)c->nnz;
    auto fetch = [&](const DevBuf<int>& ptr, size_t nptr, const DevBuf<int>& idx, const DevBuf<double>& val, std::vector<ipxint>& hp,
                     std::vector<ipxint>& hi, std::vector<double>& hx) {
        DevBuf<ipxint> wide(std::max(std::max(nz, nptr), (size_t)1));
        hp.resize(nptr); hi.resize(nz); hx.resize(nz);
        widen_ints((int64_t)nptr, ptr.get(), wide.get(), s);
        wide.download(hp.data(), nptr, s);
        if (nz) {
            widen_ints((int64_t)nz, idx.get(), wide.get(), s);
            wide.download(hi.data(), nz, s);
            val.download(hx.data(), nz, s);
        }
        IPXK_HIP(hipStreamSynchronize(s));
    };
    IPXK_REQUIRE(c->have_plain, "model not uploaded");
    if (!rowwise && c->h_Ai.size() != nz) {
        std::vector<ipxint> hp;
        fetch(c->pl_Ap, (size_t)c->n + 1, c->pl_Ai, c->pl_Ax, hp, c->h_Ai, c->h_Ax);
    }
    if (rowwise && (c->h_ATp.size() != (size_t)c->m + 1 || c->h_ATi.size() != nz))
        fetch(c->pl_Tp, (size_t)c->m + 1, c->pl_Ti, c->pl_Tx, c->h_ATp, c->h_ATi, c->h_ATx);
}

// the entries of `cols` (structural columns), one column after the other, on the host
void fetch_columns(Context* c, const std::vector<ipxint>& cols, std::vector<ipxint>& Cp, std::vector<ipxint>& Ci, std::vector<double>& Cx) {
    const int k = (int)cols.size();
    hipStream_t s = c->stream;
    Cp.assign((size_t)k + 1, 0);
    std::vector<int> c32((size_t)k), off((size_t)k);
    for (int kk = 0; kk < k; kk++) {
        const ipxint j = cols[(size_t)kk];
        c32[(size_t)kk] = (int)j;
        off[(size_t)kk] = (int)Cp[(size_t)kk];
        Cp[(size_t)kk + 1] = Cp[(size_t)kk] + (c->h_Ap[(size_t)j + 1] - c->h_Ap[(size_t)j]);
    }
    const size_t tot = (size_t)Cp[(size_t)k];
    Ci.resize(tot); Cx.resize(tot);
    if (k == 0 || tot == 0) return;
    DevBuf<int> dc, doff;
    DevBuf<ipxint> di(tot);
    DevBuf<double> dx(tot);
    dc.upload(c32, s); doff.upload(off, s);
    hipLaunchKernelGGL(gather_columns_kernel, dim3(k), dim3(kBlock), 0, s, k, dc.get(), doff.get(), c->pl_Ap.get(), c->pl_Ai.get(), c->pl_Ax.get(),
                       di.get(), dx.get());
    di.download(Ci.data(), tot, s);
    dx.download(Cx.data(), tot, s);
    IPXK_HIP(hipStreamSynchronize(s));
    IPXK_HIP(hipGetLastError());
}

int device_max_row_length(LayoutScratch& S, int nrows, const int* dptr, hipStream_t s) {
    S.stats.ensure(8);
    IPXK_HIP(hipMemsetAsync(S.stats.get(), 0, 8 * sizeof(int), s));
    hipLaunchKernelGGL(max_len_kernel, dim3(gridn(nrows)), dim3(kBlock), 0, s, nrows, dptr, S.stats.get());
    int h = 0;
    IPXK_HIP(hipMemcpyAsync(&h, S.stats.get(), sizeof(int), hipMemcpyDeviceToHost, s));
    IPXK_HIP(hipStreamSynchronize(s));
    return h;
}

// ---------------------------------------------------------------------------
// dense columns
// ---------------------------------------------------------------------------
// Dense-column classification of Model::FindDenseColumns (src/model.cc:34-56): with the column counts in ascending
// order, the first count that exceeds max(40, 10 * its predecessor) is the threshold.  Equal neighbours never
// satisfy that, so it is enough to walk the DISTINCT counts in ascending order (a histogram instead of a sort).
// hist[v] = # columns with v entries, ncols their sum; sets num_dense and nz_dense (m + 1: no dense column).
static void dense_threshold(const std::vector<int64_t>& hist, int64_t ncols, int64_t m, int64_t* num_dense, int64_t* nz_dense) {
    *num_dense = 0;
    *nz_dense = m + 1;
    if (ncols < 2) return;
    int64_t prev = -1, below = 0;       // below: # columns with a smaller count
    for (int64_t v = 0; v < (int64_t)hist.size(); v++) {
        if (hist[(size_t)v] == 0) continue;
        if (prev >= 0 && v > std::max<int64_t>(40, 10 * prev)) {
            *num_dense = ncols - below;
            *nz_dense = v;
            break;
        }
        prev = v;
        below += hist[(size_t)v];
    }
    if (*num_dense > 1000) {
        *num_dense = 0;
        *nz_dense = m + 1;
    }
}

// The counts come from the device's column pointers: their maximum, a histogram (integer atomics: exact in any order) and, if
// there are dense columns, the list of them (at most 1000; sorted on the host).  No host pass over the columns.
static void find_dense_columns(Context* c) {
    const int64_t n = c->n, m = c->m;
    hipStream_t s = c->stream;
    c->dense_cols.clear();
    LayoutScratch S;
    const int maxcnt = n > 0 ? device_max_row_length(S, (int)n, c->pl_Ap.get(), s) : 0;
    DevBuf<int> dhist((size_t)maxcnt + 1);
    IPXK_HIP(hipMemsetAsync(dhist.get(), 0, ((size_t)maxcnt + 1) * sizeof(int), s));
    if (n > 0) hipLaunchKernelGGL(count_histogram_kernel, dim3(grid_for(n, 1024)), dim3(kBlock), 0, s, (int)n, c->pl_Ap.get(), maxcnt, dhist.get());
    std::vector<int> h32((size_t)maxcnt + 1);
    dhist.download(h32.data(), h32.size(), s);
    const std::vector<int64_t> hist(h32.begin(), h32.end());
    dense_threshold(hist, n, m, &c->num_dense, &c->nz_dense);
    if (c->num_dense > 0) {
        DevBuf<int> list((size_t)c->num_dense), count(1);
        IPXK_HIP(hipMemsetAsync(count.get(), 0, sizeof(int), s));
        hipLaunchKernelGGL(rows_at_least_kernel, dim3(gridn(n)), dim3(kBlock), 0, s, (int)n, c->pl_Ap.get(), (int)c->nz_dense, (int)c->num_dense,
                           count.get(), list.get());
        std::vector<int> cols((size_t)c->num_dense);
        list.download(cols.data(), cols.size(), s);
        std::sort(cols.begin(), cols.end());
        c->dense_cols.assign(cols.begin(), cols.end());
    }
    IPXK_HIP(hipGetLastError());
}

// The same classification for the whole partitioned matrix, identical on every rank (comm_init).  Row partition: the
// counts of the n columns are summed over the ranks (one all-reduce of n).  Column partition: the counts are global
// already, but the rule looks at the counts of ALL columns -- the largest count (all-reduce max), then a histogram of
// the counts (all-reduce sum of maxcnt + 1 bins).  m is the global row count.  dense_cols keeps local column
// indices: under the column partition only the dense columns this rank owns.  Returns whether the classification
// differs from the one the context had (built from its own slab alone).
bool classify_dense_columns_global(Context* c) {
    const int64_t n = c->n;
    hipStream_t s = c->stream;
    std::vector<int64_t> cnt((size_t)n), hist;
    for (int64_t j = 0; j < n; j++) cnt[(size_t)j] = c->h_Ap[j + 1] - c->h_Ap[j];
    int64_t ncols = n;
    if (comm_rows(c)) {
        std::vector<double> h(cnt.begin(), cnt.end());
        DevBuf<double> d;
        d.upload(h, s);
        comm_allreduce_sum(c, d.get(), (size_t)n);
        d.download(h.data(), (size_t)n, s);
        IPXK_HIP(hipStreamSynchronize(s));
        comm_check(c);
        int64_t maxcnt = 0;
        for (int64_t j = 0; j < n; j++) { cnt[(size_t)j] = (int64_t)h[(size_t)j]; maxcnt = std::max(maxcnt, cnt[(size_t)j]); }
        hist.assign((size_t)maxcnt + 1, 0);
        for (int64_t j = 0; j < n; j++) hist[(size_t)cnt[(size_t)j]]++;
    } else {
        double mx = 0.0;
        for (int64_t j = 0; j < n; j++) mx = std::max(mx, (double)cnt[(size_t)j]);
        DevBuf<double> d(1);
        d.upload(&mx, 1, s);
        comm_allreduce_max(c, d.get(), 1);
        d.download(&mx, 1, s);
        IPXK_HIP(hipStreamSynchronize(s));
        comm_check(c);
        const int64_t maxcnt = (int64_t)mx;
        std::vector<double> h((size_t)maxcnt + 1, 0.0);
        for (int64_t j = 0; j < n; j++) h[(size_t)cnt[(size_t)j]] += 1.0;
        DevBuf<double> dh;
        dh.upload(h, s);
        comm_allreduce_sum(c, dh.get(), h.size());
        dh.download(h.data(), h.size(), s);
        IPXK_HIP(hipStreamSynchronize(s));
        comm_check(c);
        hist.assign(h.size(), 0);
        ncols = 0;
        for (size_t v = 0; v < h.size(); v++) { hist[v] = (int64_t)h[v]; ncols += hist[v]; }
    }
    int64_t num_dense = 0, nz_dense = 0;
    dense_threshold(hist, ncols, c->m_global, &num_dense, &nz_dense);
    std::vector<ipxint> cols;
    for (int64_t j = 0; j < n; j++)
        if (cnt[(size_t)j] >= nz_dense) cols.push_back(j);
    const bool changed = num_dense != c->num_dense || nz_dense != c->nz_dense || cols != c->dense_cols;
    c->num_dense = num_dense;
    c->nz_dense = nz_dense;
    c->dense_cols = cols;
    return changed;
}

static double ms_since(std::chrono::steady_clock::time_point& t0) {
    const auto t1 = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    t0 = t1;
    return ms;
}

// The model goes to the device as it is (one staged copy of the caller's arrays); validation, the narrowing to 32-bit
// indices, Transpose and the layouts of both gather matrices happen there (layout_device.hip).  Matrices the device
// builders do not cover take the host builders on host copies of the entries -- of the caller's arrays for the CSC, a
// download of the device's row-wise copy for the other gather matrix.
void build_model(Context* c, const ipxint* Ap, const ipxint* Ai, const double* Ax) {
    auto t0 = std::chrono::steady_clock::now();
    upload_plain_model(c, Ap, Ai, Ax);
    c->create_ms[0] = ms_since(t0);
    build_model_resident(c, Ap, Ai, Ax);
}

// The plain copy of a model that is on the device already (pl_Ap, pl_Ai, pl_Ax filled, m, n, nnz set: the user model of
// user_model.hip, which scales the matrix there): the column pointers on the host and the row-wise copy.
void adopt_plain_model(Context* c) {
    const int64_t m = c->m, n = c->n, nz = c->nnz;
    hipStream_t s = c->stream;
    IPXK_REQUIRE(m < (int64_t(1) << 31) - 1 && n < (int64_t(1) << 31) - 1, "dimension exceeds 32-bit device indices");
    IPXK_REQUIRE(nz >= 0 && nz < (int64_t(1) << 31) - kLongSeg, "nnz exceeds 32-bit device indices");
    const size_t nz1 = (size_t)std::max<int64_t>(nz, 1);
    DevBuf<ipxint> wide((size_t)n + 1);
    c->h_Ap.resize((size_t)n + 1);
    widen_ints(n + 1, c->pl_Ap.get(), wide.get(), s);
    wide.download(c->h_Ap.data(), (size_t)n + 1, s);
    c->pl_Ai.ensure(nz1); c->pl_Ax.ensure(nz1); c->pl_Tp.ensure((size_t)m + 1); c->pl_Ti.ensure(nz1); c->pl_Tx.ensure(nz1);
    if (nz > 0) {
        DevBuf<int> colof;
        Tmp T;
        device_transpose(T, colof, n, m, nz, c->pl_Ap.get(), c->pl_Ai.get(), c->pl_Ax.get(), c->pl_Tp.get(), c->pl_Ti.get(), c->pl_Tx.get(), s);
    } else {
        IPXK_HIP(hipMemsetAsync(c->pl_Tp.get(), 0, ((size_t)m + 1) * sizeof(int), s));
        IPXK_HIP(hipStreamSynchronize(s));
    }
    IPXK_HIP(hipGetLastError());
    c->have_plain = true;
}

// Everything of a context that follows the plain copy: the layouts of both gather matrices, the dense columns, the renumbering.
// Ap, Ai, Ax: the caller's host arrays for the host builders, or all NULL -- then they work on a download of the plain copy.
void build_model_resident(Context* c, const ipxint* Ap, const ipxint* Ai, const double* Ax) {
    const int64_t m = c->m, n = c->n;
    auto t0 = std::chrono::steady_clock::now();
    const int64_t nz = c->nnz;
    LayoutScratch S;
    c->Acols.csr_ptr = c->pl_Ap.get(); c->Acols.csr_idx = c->pl_Ai.get(); c->Acols.csr_val = c->pl_Ax.get();
    c->Arows.csr_ptr = c->pl_Tp.get(); c->Arows.csr_idx = c->pl_Ti.get(); c->Arows.csr_val = c->pl_Tx.get();
    if (!c->Acols.build_device(S, n, m, nz, c->pl_Ap.get(), c->pl_Ai.get(), c->pl_Ax.get(), c->stream)) {
        if (Ap) {
            c->Acols.build(n, m, Ap, Ai, Ax, c->stream);
        } else {
            ensure_host_model(c, false);
            c->Acols.build(n, m, c->h_Ap.data(), c->h_Ai.data(), c->h_Ax.data(), c->stream);
            c->h_Ai = std::vector<ipxint>(); c->h_Ax = std::vector<double>();
        }
    }
    c->create_ms[1] = ms_since(t0);
    if (!c->Arows.build_device(S, m, n, nz, c->pl_Tp.get(), c->pl_Ti.get(), c->pl_Tx.get(), c->stream)) {
        ensure_host_model(c, true);
        c->Arows.build(m, n, c->h_ATp.data(), c->h_ATi.data(), c->h_ATx.data(), c->stream);
        c->h_ATp = std::vector<ipxint>(); c->h_ATi = std::vector<ipxint>(); c->h_ATx = std::vector<double>();
    }
    c->create_ms[2] = ms_since(t0);
    S = LayoutScratch();                           // the builders' scratch is released before the rest allocates
    find_dense_columns(c);
    c->tcols.resize(n > 0 ? n : 1);
    prepare_dense_columns(c);
    if (c->num_dense == 0) {                       // (the Sherman-Morrison-Woodbury preconditioner keeps the numbering as given)
        try {
            reorder_model(c);
        } catch (const Error& e) {                 // an optional acceleration: a model is created without it rather than not at all
            if (getenv("IPXK_VERBOSE")) fprintf(stderr, "ipxk: reordering given up: %s\n", e.what());
            c->reord = Reordered();
        }
    }
    c->create_ms[3] = ms_since(t0);
    if (getenv("IPXK_VERBOSE"))
        fprintf(stderr, "ipxk: model %lld x %lld nnz %lld on the device: upload + transpose %.1f ms, A' layouts %.1f ms, A layouts %.1f ms, rest %.1f ms\n",
                (long long)m, (long long)n, (long long)nz, c->create_ms[0], c->create_ms[1], c->create_ms[2], c->create_ms[3]);
}

}  // namespace ipxk
