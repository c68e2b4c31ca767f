// Basis-preconditioned operator on the device.
//   SplittedNormalMatrix::Prepare / _Apply      reference src/splitted_normal_matrix.cc:18-117
//   Basis::SolveDense on fresh factors               src/basis.cc:168-170, src/forrest_tomlin.cc:67-78
// The triangular solves inside it are pairs of level-scheduled sweeps (sweep.hip, sweep_blocks.hip) with the dense bump of
// the LU between them (dense_bump.hip); KKTSolverBasis::_Solve on top of it is kkt_basis.hip.
//
// N N' is applied through the resident model matrix: N = AI[:,nonbasic] scaled by D and with
// rows in pivot order, hence N N' w = P A (M D^2) A' P' w with M the nonbasic mask -- the
// NormalMatrix kernels with weights W = M.*D^2 between two permutation kernels.  Prepare
// therefore uploads O(m + n) numbers plus the factors and never copies the matrix
// (the reference copies all of N every time, splitted_normal_matrix.cc:42-55).
#include "context.hpp"
#include "spmv_kernels.hpp"
#include "trisolve.hpp"

namespace ipxk {

void destroy_split(SplitOperator* s) { delete s; }

// out[p] = order[p] >= 0 ? map[order[p]] : -1   (map == nullptr: identity)
__global__ void compose_kernel(int n, const int* __restrict__ order, const int* __restrict__ map, int* __restrict__ out) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const int i = order[p];
        out[p] = i >= 0 ? (map ? map[i] : i) : -1;
    }
}

// out[map[i]] = i
__global__ void invert_map_kernel(int n, const int* __restrict__ map, int* __restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[map[i]] = i;
}

// lhs = free ? 0 : lhs + rhs;  partial dot rhs'lhs       (splitted_normal_matrix.cc:112-116)
__global__ __launch_bounds__(kBlock) void split_finish_kernel(int m, const double* __restrict__ rhs,
                                                              const unsigned char* __restrict__ free_mask,
                                                              const double* __restrict__ y, const int* __restrict__ posof,
                                                              double* __restrict__ lhs, double* partial,
                                                              const int* done) {
    if (done && *done) return;
    __shared__ double red[kBlock / 64 + 1];
    double acc = 0.0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < m; i += gridDim.x * kBlock) {
        const double r = rhs[i];
        const double l = free_mask[i] ? 0.0 : y[posof[i]] + r;
        lhs[i] = l;
        acc += r * l;
    }
    acc = block_reduce<SumOp>(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// ---------------------------------------------------------------------------
// Prepare
// ---------------------------------------------------------------------------
// scaling-dependent part of Prepare, from the raw status / colscale arrays on the device:
// N N' weights colscale^2 on NONBASIC columns (splitted_normal_matrix.cc:42-55)
__global__ void scaling_columns_kernel(int64_t N, const ipxint* __restrict__ status, const double* __restrict__ colscale,
                                       double* __restrict__ W, int* __restrict__ status32, int* bad) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += (int64_t)gridDim.x * blockDim.x) {
        const ipxint st = status[j];
        if (st < IPXK_NONBASIC_FIXED || st > IPXK_BASIC_FREE) *bad = 1;
        status32[j] = (int)st;
        W[j] = st == IPXK_NONBASIC ? colscale[j] * colscale[j] : 0.0;
    }
}
// ---- kernels by basis position ----
// On a column-partitioned context (comm_cols) L, U, the permutations and basis[] (global column numbers) are replicated;
// status, colscale, a and x are local ([this rank's structural slice; all m slack entries]).  What a kernel indexed by
// basis position needs of a column is formed through loc (SplitOperator::loc_map) by one all-reduce of the owners'
// contributions (every other rank adds 0, so the sum is exact); slack positions are filled in locally afterwards,
// identically on every rank.  Unpartitioned, the all-reduce is no exchange at all and the same kernels read basis[].
static const char* const kRowPartitionRefusal =
    "the basis path does not run on a row-partitioned system: partition the structural columns (ipxk_comm_init_columns)";

// an operator prepared under another communicator (or none) is not used: its basis numbering and its exchanges differ
void split_check_partition(const Context* c) {
    IPXK_REQUIRE(!comm_rows(c), kRowPartitionRefusal);
    IPXK_REQUIRE(c->split->part == comm_cols(c), "the split operator was prepared under another partition: Prepare it again");
}

// the ranks agree on the verdict and on the replicated arguments of the basis path (comm.hip)
static void agree_on_arguments(Context* c, const std::string& err, uint64_t h) {
    agree_on_arguments(c, err, h, "the basis path", "factors, permutations, basis, slack parts of status and colscale");
}

// local status entries in range (the scaling kernel's check, made before the ranks agree)
static void check_status_host(int64_t N, const ipxint* status) {
    for (int64_t j = 0; j < N; j++)
        IPXK_REQUIRE(status[j] >= IPXK_NONBASIC_FIXED && status[j] <= IPXK_BASIC_FREE, "status entry out of range");
}

// the owner's contributions to pos_status (sum[0..m)) and pos_scale (sum[m..2m))
__global__ void pos_scaling_contrib_kernel(int m, int n, const int* __restrict__ loc, const int* __restrict__ status32,
                                           const double* __restrict__ colscale, double* __restrict__ sum) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < m; p += gridDim.x * blockDim.x) {
        const int l = loc[p];
        const bool mine = l >= 0 && l < n;
        sum[p] = mine ? (double)status32[l] : 0.0;
        sum[m + p] = mine ? colscale[l] : 0.0;
    }
}
// pos_status / pos_scale from the summed contributions and the slack part
__global__ void pos_scaling_kernel(int m, int n, const int* __restrict__ loc, const double* __restrict__ sum,
                                   const int* __restrict__ status32, const double* __restrict__ colscale,
                                   int* __restrict__ pos_status, double* __restrict__ pos_scale) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < m; p += gridDim.x * blockDim.x) {
        const int l = loc[p];
        pos_status[p] = l >= n ? status32[l] : (int)sum[p];
        pos_scale[p] = l >= n ? colscale[l] : sum[m + p];
    }
}
// column scaling of U in pivot order (:30-39; nothing for BASIC_FREE) and the free positions (:58-64)
__global__ void scaling_pivots_pos_kernel(int m, const int* __restrict__ colperm, const int* __restrict__ pos_status,
                                          const double* __restrict__ pos_scale, double* __restrict__ uscale,
                                          unsigned char* __restrict__ fmask, int* num_free) {
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < m; k += gridDim.x * blockDim.x) {
        const int p = colperm[k];
        const int st = pos_status[p];
        uscale[k] = st == IPXK_BASIC ? pos_scale[p] : 1.0;
        fmask[k] = st == IPXK_BASIC_FREE ? 1 : 0;
        if (st == IPXK_BASIC_FREE) atomicAdd(num_free, 1);
    }
}

// status and scale of every basis position (from S->status, S->colscale): one all-reduce of 2m, then the slack
// positions locally; then the scaling of U and the free positions
static void scaling_positions(Context* c, SplitOperator* S) {
    const int m = S->m, n = (int)c->n;
    hipStream_t s = c->stream;
    const size_t mm = (size_t)std::max(m, 1);
    S->pos_sum.ensure(2 * mm); S->pos_status.ensure(mm); S->pos_scale.ensure(mm);
    if (m > 0) {
        allreduce_product(c, S->pos_sum.get(), 2 * (size_t)m, [&](double* out) {
            hipLaunchKernelGGL(pos_scaling_contrib_kernel, dim3(vec_grid(m)), dim3(kBlock), 0, s, m, n, S->loc_map(),
                               S->status.get(), S->colscale.get(), out);
        });
        hipLaunchKernelGGL(pos_scaling_kernel, dim3(vec_grid(m)), dim3(kBlock), 0, s, m, n, S->loc_map(), S->pos_sum.get(),
                           S->status.get(), S->colscale.get(), S->pos_status.get(), S->pos_scale.get());
        hipLaunchKernelGGL(scaling_pivots_pos_kernel, dim3(vec_grid(m)), dim3(kBlock), 0, s, m, S->colperm.get(), S->pos_status.get(),
                           S->pos_scale.get(), S->uscale.get(), S->free_mask.get(), S->counters.get() + 1);
    }
}

static void upload_scaling(Context* c, SplitOperator* S, const ipxint* status, const double* colscale) {
    const int m = S->m, n = (int)c->n;
    const size_t N = (size_t)n + m;
    hipStream_t s = c->stream;
    S->status_raw.upload(status, N, s);
    S->colscale.upload(colscale, N, s);
    S->Wsplit.ensure(N); S->status.ensure(N);
    S->uscale.ensure(std::max(m, 1)); S->free_mask.ensure(std::max(m, 1));
    S->counters.ensure(2);
    IPXK_HIP(hipMemsetAsync(S->counters.get(), 0, 2 * sizeof(int), s));
    hipLaunchKernelGGL(scaling_columns_kernel, dim3(vec_grid((int64_t)N)), dim3(kBlock), 0, s, (int64_t)N,
                       S->status_raw.get(), S->colscale.get(), S->Wsplit.get(), S->status.get(), S->counters.get());
    scaling_positions(c, S);
    int h[2] = {0, 0};
    S->counters.download(h, 2, s);
    if (h[0]) throw Error(IPXK_E_ARGUMENT, "status entry out of range");
    S->num_free = h[1];
    rescale_sweeps_device(c, S);
    // N N' runs on the model matrix with weights that are zero on the BASIC and fixed columns: value arrays in
    // which those columns' entries are zero let both passes skip the gathers of those entries (spmv_mask.hip)
    S->masked_values = !(getenv("IPXK_MASKED_VALUES") && getenv("IPXK_MASKED_VALUES")[0] == '0');
    // IPXK_COMPACT_N=0: keep streaming the whole model matrix with masked values (round-2 form)
    const bool compact = !(getenv("IPXK_COMPACT_N") && getenv("IPXK_COMPACT_N")[0] == '0');
    c->Acols.compact.valid = c->Arows.compact.valid = false;
    // large models: N as a pair of gather matrices of its own, built on the device (nmatrix.hip); otherwise ...
    S->real_N = S->masked_values && compact && nmatrix_prepare(c, S->Wsplit.get());
    if (S->masked_values && !S->real_N) {
        // N as a matrix of its own (splitted_normal_matrix.cc:42-55): the tiles of the two gather matrices without
        // the entries of zero-weight columns; layouts without tiles (phased) and long rows keep the masked values
        if (compact) {
            c->Acols.compact_tiles(S->Wsplit.get(), true, s);    // a row of the gather matrix = a structural column
            c->Arows.compact_tiles(S->Wsplit.get(), false, s);   // the gathered index = a structural column
        }
        if (!c->Acols.compact.valid) c->Acols.mask_values(S->Wsplit.get(), true, s);
        if (!c->Arows.compact.valid) c->Arows.mask_values(S->Wsplit.get(), false, s);
    }
}

// what follows the analysis of the factors and the upload of the permutations in a Prepare: scaling, work
// vectors, the composed gather maps of the four sweeps
static void finish_prepare(Context* c, SplitOperator* S, const ipxint* status, const double* colscale) {
    const int m = S->m;
    hipStream_t s = c->stream;
    upload_scaling(c, S, status, colscale);
    const size_t mm = (size_t)std::max(m, 1);
    S->w0.resize(mm); S->w1.resize(mm); S->w2.resize(mm); S->w3.resize(mm); S->tI.resize(mm);
    S->aB.ensure(mm);
    S->zeros.ensure(mm);
    IPXK_HIP(hipMemsetAsync(S->zeros.get(), 0, mm * sizeof(double), s));
    // where every sweep finds its right-hand side: U' in the input vector itself, L' in the result of U'
    // (by position), L in the input vector THROUGH rowperm (the operator's N N' product is formed in the row
    // order of A: the permutation into pivot order is folded into the gather), U in the result of L;
    // and where the row order of A finds the result of the backward pair
    {
        auto compose = [&](int n, const int* order, const int* map, int* out) {
            if (n > 0) hipLaunchKernelGGL(compose_kernel, dim3(vec_grid(n)), dim3(kBlock), 0, s, n, order, map, out);
        };
        compose(S->Ut.npos, S->Ut.order.get(), nullptr, S->Ut.src.get());
        compose(S->Lt.npos, S->Lt.order.get(), S->Ut.posof.get(), S->Lt.src.get());
        compose(S->Lf.npos, S->Lf.order.get(), S->rowperm.get(), S->Lf.src.get());
        compose(S->Uf.npos, S->Uf.order.get(), S->Lf.posof.get(), S->Uf.src.get());
        for (Sweep* W : {&S->Ut, &S->Lt, &S->Lf, &S->Uf}) locate_block_rhs(c, *W);    // inverted blocks: where their right-hand sides sit
        S->perm_after_backward.ensure(mm);
        compose(m, S->rowperm_inv.get(), S->Lt.posof.get(), S->perm_after_backward.get());
        // ... and its inverse, by position of the L' sweep (padding positions: -1)
        S->row_after_backward.ensure((size_t)std::max(S->Lt.npos, 1));
        IPXK_HIP(hipMemsetAsync(S->row_after_backward.get(), 0xff, (size_t)std::max(S->Lt.npos, 1) * sizeof(int), s));
        if (m > 0) hipLaunchKernelGGL(invert_map_kernel, dim3(vec_grid(m)), dim3(kBlock), 0, s, m, S->perm_after_backward.get(),
                                      S->row_after_backward.get());
    }
    S->xcc_slots.resize(64);
    IPXK_HIP(hipMemsetAsync(S->xcc_slots.get(), 0, 64 * sizeof(unsigned long long), s));
    S->abort_flag.resize(1);
    IPXK_HIP(hipMemsetAsync(S->abort_flag.get(), 0, sizeof(int), s));
    c->ensure_partials();
    IPXK_HIP(hipStreamSynchronize(s));
}

// Takes the operator out of the context for rebuilding.  The operator object (and its device buffers) is reused from one
// Prepare to the next; while it is being rebuilt the context has no operator, and a failure leaves it that way.
static std::unique_ptr<SplitOperator> take_operator(Context* c, int m) {
    std::unique_ptr<SplitOperator> S(c->split ? c->split : c->split_spare ? c->split_spare : new SplitOperator);
    if (!c->split) c->split_spare = nullptr;
    c->split = nullptr;
    S->m = m;
    if (const char* e = getenv("IPXK_TRISOLVE")) S->level_launches = std::string(e) == "levels";
    S->bump.start = S->bump.size = 0;
    return S;
}

void split_prepare_host(Context* c, const ipxint* Lp, const ipxint* Li, const double* Lx,
                        const ipxint* Up, const ipxint* Ui, const double* Ux, const ipxint* rowperm,
                        const ipxint* colperm, const ipxint* basis, const ipxint* status,
                        const double* colscale) {
    maxvol_drop_etas(c);
    const int m = (int)c->m, n = (int)c->n;
    hipStream_t s = c->stream;
    IPXK_REQUIRE(!comm_rows(c), kRowPartitionRefusal);
    const bool part = comm_cols(c);
    learn_col_offsets(c);
    const int64_t ncols = c->n_global;                  // the structural columns basis[] numbers
    auto check_arguments = [&] {
        IPXK_REQUIRE(ncols + m < (int64_t(1) << 31), "column count exceeds 32 bits");
        IPXK_REQUIRE(Lp[m] < (int64_t(1) << 31) && Up[m] < (int64_t(1) << 31), "factor nnz exceeds 32 bits");
        IPXK_REQUIRE(Lp[0] == 0 && Up[0] == 0, "column pointers must start at 0");
        for (int k = 0; k < m; k++) {
            IPXK_REQUIRE(Lp[k + 1] >= Lp[k] && Up[k + 1] > Up[k] && Up[k + 1] <= Up[m] && Lp[k + 1] <= Lp[m],
                         "factor column pointers not monotone");
            IPXK_REQUIRE(Ui[Up[k + 1] - 1] == k, "U must hold its diagonal last in each column");
            IPXK_REQUIRE(basis[k] >= 0 && basis[k] < ncols + m, "basis entry out of range");
            IPXK_REQUIRE(rowperm[k] >= 0 && rowperm[k] < m && colperm[k] >= 0 && colperm[k] < m, "permutation entry out of range");
        }
        {   // rowperm, colperm are permutations; basis entries distinct is the caller's contract
            std::vector<unsigned char> seen_r(m, 0), seen_c(m, 0);
            for (int k = 0; k < m; k++) {
                IPXK_REQUIRE(!seen_r[rowperm[k]] && !seen_c[colperm[k]], "rowperm / colperm is not a permutation");
                seen_r[rowperm[k]] = seen_c[colperm[k]] = 1;
            }
        }
    };
    if (part) {
        // every rank checks its arguments, then all ranks agree on the verdict and on the replicated arguments
        std::string err;
        uint64_t fp = 0;
        try {
            check_arguments();
            check_status_host((int64_t)n + m, status);
            Fingerprint F;
            F.add(Lp, (size_t)m + 1); F.add(Li, (size_t)Lp[m]); F.add(Lx, (size_t)Lp[m]);
            F.add(Up, (size_t)m + 1); F.add(Ui, (size_t)Up[m]); F.add(Ux, (size_t)Up[m]);
            F.add(rowperm, (size_t)m); F.add(colperm, (size_t)m); F.add(basis, (size_t)m);
            F.add(status + n, (size_t)m); F.add(colscale + n, (size_t)m);
            fp = F.h;
        } catch (const Error& e) {
            err = e.what();
        }
        agree_on_arguments(c, err, fp);
    } else {
        check_arguments();
    }
    std::unique_ptr<SplitOperator> S = take_operator(c, m);

    const bool verbose = getenv("IPXK_VERBOSE") != nullptr;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double tp0 = now();
    {
        // factors as given, on the device; a dense trailing block (the bump of the LU) is cut out of the sweeps
        DevBuf<ipxint> &dLp = S->in_Lp, &dLi = S->in_Li, &dUp = S->in_Up, &dUi = S->in_Ui;
        DevBuf<double> &dLx = S->in_Lx, &dUx = S->in_Ux;
        const int64_t nzL = Lp[m], nzU = Up[m];
        dLp.upload(Lp, (size_t)m + 1, s); dUp.upload(Up, (size_t)m + 1, s);
        dLi.upload(Li, (size_t)nzL, s);   dLx.upload(Lx, (size_t)nzL, s);
        dUi.upload(Ui, (size_t)nzU, s);   dUx.upload(Ux, (size_t)nzU, s);
        dLi.ensure(1); dLx.ensure(1);
        const DeviceFactors F0{dLp.get(), dLi.get(), dUp.get(), dUi.get(), dLx.get(), dUx.get(), nzL, nzU};
        const int s0 = m > 0 ? trailing_dense_block(m, Lp) : m;
        // the cut takes the entries of a U column above the block as a PREFIX of the column and the block's own as its last
        // entries: that needs ascending row indices inside the columns from s0 on.  The contract of ipxk_split_prepare asks
        // for the diagonal last only (the reference's GetLuFactors does return sorted columns); unsorted ones keep the whole
        // factors in the sweeps.
        bool sorted_U = true;
        for (int j = s0; j < m && sorted_U; j++)
            for (ipxint p = Up[j] + 1; p < Up[j + 1]; p++)
                if (Ui[p] <= Ui[p - 1]) { sorted_U = false; break; }
        analyse_sweeps_cutting_bump(c, S.get(), F0, sorted_U && m - s0 <= 32768, s0, m - s0, Lp, Li, Up, Ui);
        IPXK_HIP(hipStreamSynchronize(s));           // the uploaded factors go out of scope
    }
    const double tp1 = now();
    // permutations (InversePerm, utils.cc:73-80) and bookkeeping for KKTSolverBasis::_Solve
    {
        std::vector<int> rpm(m), rpi(m), cpm(m), bs(m);
        for (int i = 0; i < m; i++) { rpm[i] = (int)rowperm[i]; cpm[i] = (int)colperm[i]; bs[i] = (int)basis[i]; }
        for (int i = 0; i < m; i++) rpi[rpm[i]] = i;
        S->rowperm.upload(rpm, s);
        S->rowperm_inv.upload(rpi, s);
        S->colperm.upload(cpm, s);
        S->basis.upload(bs, s);
        S->part = part;
        if (part) {     // where each basis position lives in this rank's local vectors (SplitOperator::loc_map)
            const int64_t c0 = c->col_offset;
            std::vector<int> loc((size_t)m, -1);
            for (int p = 0; p < m; p++) {
                const int64_t j = basis[p];
                if (j >= ncols) loc[(size_t)p] = (int)(n + (j - ncols));
                else if (j >= c0 && j < c0 + n) loc[(size_t)p] = (int)(j - c0);
            }
            S->loc.upload(loc, s);
        }
    }
    finish_prepare(c, S.get(), status, colscale);
    if (verbose)
        fprintf(stderr, "ipxk: split_prepare: analysis and packing %.1f ms, permutations/scaling %.1f ms\n",
                (tp1 - tp0) * 1e3, (now() - tp1) * 1e3);
    c->split = S.release();
}

// 64-bit permutations / basis list on the device -> the operator's 32-bit copies (+ InversePerm, utils.cc:73-80)
__global__ void perms_from_lu_kernel(int m, const ipxint* __restrict__ rowperm, const ipxint* __restrict__ colperm,
                                     const ipxint* __restrict__ basis, int* __restrict__ rpm, int* __restrict__ rpi,
                                     int* __restrict__ cpm, int* __restrict__ bs) {
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < m; k += gridDim.x * blockDim.x) {
        const int r = (int)rowperm[k];
        rpm[k] = r;
        rpi[r] = k;
        cpm[k] = (int)colperm[k];
        bs[k] = (int)basis[k];
    }
}

// Prepare from the factors of the last ipxk_lu_factorize_basis: Basis::GetLuFactors (basis.cc:162-166) +
// SplittedNormalMatrix::Prepare (splitted_normal_matrix.cc:18-66) with L, U and the permutations never leaving the
// device.
void split_prepare_lu(Context* c, const ipxint* status, const double* colscale) {
    IPXK_REQUIRE(!comm_active(c), kDeviceLuRefusal);
    maxvol_drop_etas(c);
    LuView V;
    IPXK_REQUIRE(lu_view(c, &V) && V.from_basis, "no LU factorization of a basis of this context's matrix (ipxk_lu_factorize_basis)");
    IPXK_REQUIRE(V.ndep == 0, "the factorization replaced dependent columns: repair the basis and factorize again "
                              "(Basis::AdaptToSingularFactorization, src/basis.cc)");
    const int m = (int)c->m;
    IPXK_REQUIRE(V.dim == m, "dimension mismatch");
    hipStream_t s = c->stream;
    std::unique_ptr<SplitOperator> S = take_operator(c, m);
    S->part = false;
    // the dense bump leaves the level-scheduled structure (SplitOperator::DenseBump)
    analyse_sweeps_cutting_bump(c, S.get(), V.F, V.bump_size > 0 && V.bump_start + V.bump_size == m, V.bump_start, V.bump_size, nullptr, nullptr,
                                nullptr, nullptr);
    const size_t mm = (size_t)std::max(m, 1);
    S->rowperm.ensure(mm); S->rowperm_inv.ensure(mm); S->colperm.ensure(mm); S->basis.ensure(mm);
    if (m > 0)
        hipLaunchKernelGGL(perms_from_lu_kernel, dim3(vec_grid(m)), dim3(kBlock), 0, s, m, V.rowperm, V.colperm, V.basis,
                           S->rowperm.get(), S->rowperm_inv.get(), S->colperm.get(), S->basis.get());
    finish_prepare(c, S.get(), status, colscale);
    c->split = S.release();
}

// Same basis, new scaling factors: KKTSolverBasis::_Factorize without basis changes
// (kkt_solver_basis.cc:59-64 keeps the factorization; only the scaling of U and N changes,
// splitted_normal_matrix.cc:30-55).  The level schedule and the packed factors are reused.
void split_rescale_host(Context* c, const ipxint* status, const double* colscale) {
    SplitOperator* S = c->split;
    split_check_partition(c);
    if (S->part) {          // the ranks agree on the verdict and on the slack parts before the collective of the scaling
        const int m = S->m, n = (int)c->n;
        std::string err;
        uint64_t fp = 0;
        try {
            check_status_host((int64_t)n + m, status);
            Fingerprint F;
            F.add(status + n, (size_t)m); F.add(colscale + n, (size_t)m);
            fp = F.h;
        } catch (const Error& e) {
            err = e.what();
        }
        agree_on_arguments(c, err, fp);
    }
    upload_scaling(c, S, status, colscale);
    IPXK_HIP(hipStreamSynchronize(c->stream));
}

// ---- the operator behind an eta file (Context::etas_live, basis.hip) ----
// B_new = B_old E (E the product of Maxvolume's last exchanges, acting on vectors by basis position), hence with the column scaling S of
// the NEW basis   inverse(B~) = inverse(S) inverse(E) inverse(U) inverse(L),   inverse(B~') = inverse(L') inverse(U') inverse(E') inverse(S):
// the UNSCALED sweeps of the resident factors, the eta file between them and the scaling, and the scaling as a vector operation.
// t[colperm[k]] = rhs[k] / scale[k]          (pivot order -> basis position)
__global__ void eta_scatter_scale_kernel(int m, const double* __restrict__ rhs, const int* __restrict__ colperm, const double* __restrict__ scale,
                                         double* __restrict__ t, const int* done) {
    if (done && *done) return;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < m; k += gridDim.x * blockDim.x) t[colperm[k]] = rhs[k] / scale[k];
}
// lhs = free ? 0 : t[colperm[k]] / scale[k] + rhs;  partial dot rhs'lhs       (splitted_normal_matrix.cc:112-116)
__global__ __launch_bounds__(kBlock) void split_finish_etas_kernel(int m, const double* __restrict__ rhs, const unsigned char* __restrict__ free_mask,
                                                                   const double* __restrict__ t, const int* __restrict__ colperm,
                                                                   const double* __restrict__ scale, double* __restrict__ lhs, double* partial,
                                                                   const int* done) {
    if (done && *done) return;
    __shared__ double red[kBlock / 64 + 1];
    double acc = 0.0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < m; i += gridDim.x * kBlock) {
        const double r = rhs[i];
        const double l = free_mask[i] ? 0.0 : t[colperm[i]] / scale[i] + r;
        lhs[i] = l;
        acc += r * l;
    }
    acc = block_reduce<SumOp>(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
__global__ void narrow_basis_kernel(int m, const ipxint* __restrict__ in, int* __restrict__ out) {
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < m; p += gridDim.x * blockDim.x) out[p] = (int)in[p];
}
void split_follow_basis(Context* c, const ipxint* basis_dev, const ipxint* status, const double* colscale) {
    SplitOperator* S = c->split;
    IPXK_REQUIRE(S != nullptr, "SplittedNormalMatrix not prepared");
    const int m = S->m;
    if (m > 0) hipLaunchKernelGGL(narrow_basis_kernel, dim3(vec_grid(m)), dim3(kBlock), 0, c->stream, m, basis_dev, S->basis.get());
    S->eta_t.ensure((size_t)std::max(m, 1)); S->eta_in.ensure((size_t)std::max(m, 1));
    upload_scaling(c, S, status, colscale);       // scaling of the new basis in pivot order, free positions, weights / matrix of the new N
    IPXK_HIP(hipStreamSynchronize(c->stream));
}

// ---------------------------------------------------------------------------
// _Apply                                    (splitted_normal_matrix.cc:90-117)
// ---------------------------------------------------------------------------
int split_apply_dev(Context* c, const double* rhs, double* lhs, const int* done) {
    SplitOperator* S = c->split;
    const int m = S->m, n = (int)c->n;
    hipStream_t s = c->stream;
    const int g = vec_grid(m);
    double* work = S->w0.get();
    double* u = S->w1.get();
    const bool etas = c->etas_live;
    fill_results(c, {&S->Ut, &S->Lt, &S->Lf, &S->Uf}, done);
    // inverse(B') * rhs
    time_mark(c, kTimeBt, true);
    const double* bt_in = rhs;
    if (etas) {
        hipLaunchKernelGGL(eta_scatter_scale_kernel, dim3(g), dim3(kBlock), 0, s, m, rhs, S->colperm.get(), S->uscale.get(), S->eta_t.get(), done);
        maxvol_apply_etas(c, true, S->eta_t.get());
        gather_perm(c, S->eta_t.get(), S->colperm.get(), S->eta_in.get(), done);
        bt_in = S->eta_in.get();
    }
    // (the L' sweep also leaves its result in u in the row order of A, for the N N' product)
    run_pair(c, S->Ut, S->Lt, true, !etas, bt_in, done, S->row_after_backward.get(), u);
    time_mark(c, kTimeBt, false);
    time_mark(c, kTimeOp, true);
    // N N' of it: A (M D^2) A'.  Column partition: this rank's N_g N_g' (the slack term on rank 0 only), summed over
    // the ranks by one all-reduce of m -- enqueued whatever `done` says, so that every rank takes part in it
    auto product = [&](double* out) {
        const double* wI = S->part && c->rank != 0 ? nullptr : S->Wsplit.get() + n;
        EpiScale e1{{}, S->Wsplit.get(), c->tcols.get()};
        EpiNormalRows e2{{}, wI, u, out};
        if (S->real_N) {
            nmatrix_apply(c, wI, u, out, done);
        } else if (S->masked_values) {
            // the entries of BASIC / fixed columns have weight zero in both passes: masked value arrays, no gathers for them
            launch_spmv<EpiScale, true>(c->Acols, u, e1, nullptr, done, s);
            launch_spmv<EpiNormalRows, true>(c->Arows, c->tcols.get(), e2, nullptr, done, s);
        } else {
            launch_spmv(c->Acols, u, e1, nullptr, done, s);
            launch_spmv(c->Arows, c->tcols.get(), e2, nullptr, done, s);
        }
    };
    allreduce_product(c, work, (size_t)m, product);
    time_mark(c, kTimeOp, false);
    // inverse(B) * that (the L sweep reads `work` through rowperm)
    time_mark(c, kTimeB, true);
    run_pair(c, S->Lf, S->Uf, false, !etas, work, done);
    if (etas) {
        unpack_result(c, S->Uf, S->colperm.get(), S->eta_t.get());          // by basis position
        maxvol_apply_etas(c, false, S->eta_t.get());
    }
    time_mark(c, kTimeB, false);
    // lhs = result + rhs; zero free positions; dot
    if (etas)
        hipLaunchKernelGGL(split_finish_etas_kernel, dim3(g), dim3(kBlock), 0, s, m, rhs, S->free_mask.get(), S->eta_t.get(), S->colperm.get(),
                           S->uscale.get(), lhs, c->part(kPartCdot), done);
    else
        hipLaunchKernelGGL(split_finish_kernel, dim3(g), dim3(kBlock), 0, s, m, rhs, S->free_mask.get(), S->Uf.y.get(),
                           S->Uf.posof.get(), lhs, c->part(kPartCdot), done);
    return g;
}

// Basis::SolveDense on the fresh, unscaled factors (forrest_tomlin.cc:67-78); rhs may be lhs
void solve_dense_dev(Context* c, const double* rhs, double* lhs, char trans) {
    SplitOperator* S = c->split;
    const int m = S->m;
    hipStream_t s = c->stream;
    if (trans == 't' || trans == 'T') {
        double* work = S->w3.get();
        if (c->etas_live) {
            // inverse(B_new') = inverse(B_old') inverse(E'): the eta file first, on a copy (rhs may be lhs, and is not to be changed otherwise)
            IPXK_HIP(hipMemcpyAsync(S->eta_t.get(), rhs, (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, s));
            maxvol_apply_etas(c, true, S->eta_t.get());
            rhs = S->eta_t.get();
        }
        gather_perm(c, rhs, S->colperm.get(), work, nullptr);
        fill_results(c, {&S->Ut, &S->Lt}, nullptr);
        run_pair(c, S->Ut, S->Lt, true, false, work, nullptr);
        unpack_result(c, S->Lt, S->rowperm.get(), lhs);            // lhs[rowperm[k]] = solution[k]
    } else {
        fill_results(c, {&S->Lf, &S->Uf}, nullptr);
        run_pair(c, S->Lf, S->Uf, false, false, rhs, nullptr);      // reads rhs[rowperm[.]]
        unpack_result(c, S->Uf, S->colperm.get(), lhs);            // lhs[colperm[k]] = solution[k]
        if (c->etas_live) maxvol_apply_etas(c, false, lhs);        // inverse(B_new) = inverse(E) inverse(B_old)
    }
}

}  // namespace ipxk
