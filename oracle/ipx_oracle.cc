// TEST INFRASTRUCTURE ONLY -- see ipx_oracle.h.
//
// CPU restatement of the reference's KKT normal-equations path.  Written from
// the algorithm descriptions/loop orders of the cited reference lines, in this
// repo's own structure (flat arrays + callbacks instead of the reference's
// class hierarchy).  Sequential, one thread, int64 indices, fp64 -- the same
// arithmetic type and summation order as the reference so that it can be pinned
// bit-for-bit against oracle/_ref where no LAPACK call is involved.
//
// Pinning status (tests/test_oracle_vs_ref.py, tests/test_oracle_golden.py):
//   rows a1-a7, a9(apply from explicit factors)-a13, a15, a16: pinned against
//   the reference's own objects (oracle/_ref) and the committed golden vectors.
//   rows a8 (Prepare) and a14 (KKTSolverBasis::_Solve): the reference classes
//   need ipx::Basis, hence BASICLU -> not runnable on the CPU alone; this
//   restatement is pinned through their building blocks and the KKT-residual
//   property.  Round 3: with the device LU standing in for BASICLU (test harness
//   tests/dropin/basiclu_absent.cc) the reference's own SplittedNormalMatrix /
//   KKTSolverBasis / Maxvolume / IPM objects run on the MI355X box next to the
//   device code that the GPU tests hold equal to this restatement
//   (tests/dropin/basis_main.cc, maxvol_main.cc, ipm_main.cc): pinned through it.

#include "ipx_oracle.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <utility>
#include <vector>

typedef orc_int Int;
typedef std::vector<double> Vec;

// ----------------------------------------------------------------------------
// vector kernels
// ----------------------------------------------------------------------------

// src/utils.cc:39-45 -- left-to-right sum
extern "C" double orc_dot(Int m, const double* x, const double* y) {
    double d = 0.0;
    for (Int i = 0; i < m; i++) d += x[i] * y[i];
    return d;
}

// src/utils.cc:32-37
extern "C" double orc_infnorm(Int m, const double* x) {
    double norm = 0.0;
    for (Int i = 0; i < m; i++) norm = std::max(norm, std::abs(x[i]));
    return norm;
}

// ----------------------------------------------------------------------------
// index arithmetic
// ----------------------------------------------------------------------------

// src/sparse_matrix.cc:120-151: counting sort by row; within a row of A the
// entries appear in ascending source-column order.
extern "C" void orc_transpose(Int nrow, Int ncol, const Int* Ap, const Int* Ai,
                              const double* Ax, Int* ATp, Int* ATi,
                              double* ATx) {
    const Int nz = Ap[ncol];
    std::vector<Int> next(nrow, 0);
    for (Int p = 0; p < nz; p++) next[Ai[p]]++;
    Int sum = 0;
    for (Int i = 0; i < nrow; i++) {
        ATp[i] = sum;
        sum += next[i];
        next[i] = ATp[i];
    }
    ATp[nrow] = sum;
    for (Int j = 0; j < ncol; j++) {
        for (Int p = Ap[j]; p < Ap[j + 1]; p++) {
            Int put = next[Ai[p]]++;
            ATi[put] = j;
            ATx[put] = Ax[p];
        }
    }
}

// src/presolver.cc:868-880 (EquilibrationFactor) and :883-974 (Presolver::EquilibrateMatrix): recursive
// row and column equilibration by powers of 2 on the structural columns; returns the number of rounds that
// rescaled the matrix, or -1 when all entries are in range from the start (the reference then leaves
// colscale_ / rowscale_ empty; here they are set to 1).
static double equilibration_factor(int expmin, int expmax, int exp) {
    if (exp < expmin) return std::ldexp(1.0, (expmin - exp + 1) / 2);
    if (exp > expmax) return std::ldexp(1.0, -((exp - expmax + 1) / 2));
    return 1.0;
}
extern "C" Int orc_equilibrate(Int m, Int n, const Int* Ap, const Int* Ai, double* Ax, double* colscale,
                               double* rowscale) {
    constexpr int expmin = 0, expmax = 3;
    constexpr Int maxround = 10;
    for (Int j = 0; j < n; j++) colscale[j] = 1.0;
    for (Int i = 0; i < m; i++) rowscale[i] = 1.0;
    bool out_of_range = false;
    for (Int p = 0; p < Ap[n]; p++) {                      // :912-924 quick return
        int exp;
        std::frexp(std::abs(Ax[p]), &exp);
        if (exp < expmin || exp > expmax) { out_of_range = true; break; }
    }
    if (!out_of_range) return -1;
    std::vector<double> colmax(n), rowmax(m);
    Int rescaled = 0;
    for (Int round = 0; round < maxround; round++) {
        std::fill(rowmax.begin(), rowmax.end(), 0.0);      // :934-944
        for (Int j = 0; j < n; j++) {
            colmax[j] = 0.0;
            for (Int p = Ap[j]; p < Ap[j + 1]; p++) {
                const double xa = std::abs(Ax[p]);
                colmax[j] = std::max(colmax[j], xa);
                rowmax[Ai[p]] = std::max(rowmax[Ai[p]], xa);
            }
        }
        bool out = false;                                  // :946-964
        for (Int i = 0; i < m; i++) {
            int exp;
            std::frexp(rowmax[i], &exp);
            rowmax[i] = equilibration_factor(expmin, expmax, exp);
            if (rowmax[i] != 1.0) { out = true; rowscale[i] *= rowmax[i]; }
        }
        for (Int j = 0; j < n; j++) {
            int exp;
            std::frexp(colmax[j], &exp);
            colmax[j] = equilibration_factor(expmin, expmax, exp);
            if (colmax[j] != 1.0) { out = true; colscale[j] *= colmax[j]; }
        }
        if (!out) break;
        for (Int j = 0; j < n; j++)                        // :967-972
            for (Int p = Ap[j]; p < Ap[j + 1]; p++) {
                Ax[p] *= colmax[j];
                Ax[p] *= rowmax[Ai[p]];
            }
        rescaled++;
    }
    return rescaled;
}

// src/utils.cc:73-80
extern "C" void orc_inverse_perm(Int m, const Int* perm, Int* invperm) {
    for (Int i = 0; i < m; i++) invperm[perm[i]] = i;
}

// src/sparse_matrix.cc:153-166 (CopyColumns, PermuteRows) and
// src/sparse_matrix.h:122-128 (ScaleColumn)
extern "C" void orc_copy_permute_scale(Int nrow, const Int* Ap, const Int* Ai,
                                       const double* Ax, Int nsel,
                                       const Int* cols, const Int* perm,
                                       const double* scale, Int* Np, Int* Ni,
                                       double* Nx) {
    (void)nrow;
    Int put = 0;
    for (Int k = 0; k < nsel; k++) {
        const Int j = cols[k];
        Np[k] = put;
        for (Int p = Ap[j]; p < Ap[j + 1]; p++) {
            Ni[put] = perm ? perm[Ai[p]] : Ai[p];
            Nx[put] = scale ? Ax[p] * scale[k] : Ax[p];
            put++;
        }
    }
    Np[nsel] = put;
}

// src/model.cc:34-56
extern "C" Int orc_find_dense_columns(Int nrow, Int ncol, const Int* Ap,
                                      Int* nz_dense) {
    Int num_dense = 0;
    *nz_dense = nrow + 1;
    std::vector<Int> colcount(ncol);
    for (Int j = 0; j < ncol; j++) colcount[j] = Ap[j + 1] - Ap[j];
    std::sort(colcount.begin(), colcount.end());
    for (Int j = 1; j < ncol; j++) {
        if (colcount[j] > std::max<Int>(40, 10 * colcount[j - 1])) {
            num_dense = ncol - j;
            *nz_dense = colcount[j];
            break;
        }
    }
    if (num_dense > 1000) {
        num_dense = 0;
        *nz_dense = nrow + 1;
    }
    return num_dense;
}

// ----------------------------------------------------------------------------
// NormalMatrix::_Apply, one-pass variant (src/normal_matrix.cc:63-75,112-124)
// ----------------------------------------------------------------------------
extern "C" void orc_normal_apply(Int m, Int n, const Int* Ap, const Int* Ai,
                                 const double* Ax, const double* W,
                                 const double* rhs, double* lhs, double* dot) {
    if (W) {
        for (Int i = 0; i < m; i++) lhs[i] = rhs[i] * W[n + i];
        for (Int j = 0; j < n; j++) {
            const Int begin = Ap[j], end = Ap[j + 1];
            double d = 0.0;
            for (Int p = begin; p < end; p++) d += rhs[Ai[p]] * Ax[p];
            d *= W[j];
            for (Int p = begin; p < end; p++) lhs[Ai[p]] += d * Ax[p];
        }
    } else {
        for (Int i = 0; i < m; i++) lhs[i] = 0.0;
        for (Int j = 0; j < n; j++) {
            const Int begin = Ap[j], end = Ap[j + 1];
            double d = 0.0;
            for (Int p = begin; p < end; p++) d += rhs[Ai[p]] * Ax[p];
            for (Int p = begin; p < end; p++) lhs[Ai[p]] += d * Ax[p];
        }
    }
    if (dot) *dot = orc_dot(m, rhs, lhs);
}

// ----------------------------------------------------------------------------
// dense Cholesky (stands in for LAPACK dpotrf/dpotrs('L'); unblocked
// left-looking column algorithm, so rounding differs from a blocked LAPACK)
// ----------------------------------------------------------------------------
extern "C" Int orc_dpotrf_lower(Int k, double* a, Int lda) {
    for (Int j = 0; j < k; j++) {
        double d = a[j + j * lda];
        for (Int l = 0; l < j; l++) d -= a[j + l * lda] * a[j + l * lda];
        if (!(d > 0.0)) return j + 1;
        d = std::sqrt(d);
        a[j + j * lda] = d;
        for (Int i = j + 1; i < k; i++) {
            double s = a[i + j * lda];
            for (Int l = 0; l < j; l++) s -= a[i + l * lda] * a[j + l * lda];
            a[i + j * lda] = s / d;
        }
    }
    return 0;
}

extern "C" void orc_dpotrs_lower(Int k, const double* a, Int lda, double* b) {
    for (Int i = 0; i < k; i++) {  // L z = b
        double s = b[i];
        for (Int l = 0; l < i; l++) s -= a[i + l * lda] * b[l];
        b[i] = s / a[i + i * lda];
    }
    for (Int i = k - 1; i >= 0; i--) {  // L' x = z
        double s = b[i];
        for (Int l = i + 1; l < k; l++) s -= a[l + i * lda] * b[l];
        b[i] = s / a[i + i * lda];
    }
}

// ----------------------------------------------------------------------------
// DiagonalPrecond
// ----------------------------------------------------------------------------
struct orc_diag_precond {
    Int m = 0, k = 0;
    Vec diagonal;
    // dense columns of A stored by row: "column" i of Atd holds the entries of
    // row i, indices are positions 0..k-1 in the dense-column list.
    std::vector<Int> Atd_p, Atd_i;
    Vec Atd_x;
    Vec chol;
    Vec work;
};

// src/diagonal_precond.cc:17-111
extern "C" orc_diag_precond* orc_diag_factorize(
    Int m, Int n, const Int* Ap, const Int* Ai, const double* Ax,
    const double* W, Int nz_dense, Int precond_dense_cols, Int* errflag) {
    *errflag = 0;
    orc_diag_precond* P = new orc_diag_precond;
    P->m = m;
    P->diagonal.assign(m, 0.0);
    Vec& diag = P->diagonal;
    auto is_dense = [&](Int j) { return Ap[j + 1] - Ap[j] >= nz_dense; };

    // :28-46
    if (W) {
        for (Int i = 0; i < m; i++) diag[i] = W[n + i];
        for (Int j = 0; j < n; j++) {
            if (precond_dense_cols && is_dense(j)) continue;
            const double w = W[j];
            for (Int p = Ap[j]; p < Ap[j + 1]; p++)
                diag[Ai[p]] += Ax[p] * w * Ax[p];
        }
    } else {
        for (Int j = 0; j < n; j++) {
            if (precond_dense_cols && is_dense(j)) continue;
            for (Int p = Ap[j]; p < Ap[j + 1]; p++)
                diag[Ai[p]] += Ax[p] * Ax[p];
        }
    }

    std::vector<Int> dense_cols;
    if (precond_dense_cols)
        for (Int j = 0; j < n; j++)
            if (is_dense(j)) dense_cols.push_back(j);
    const Int k = dense_cols.size();
    P->k = k;
    if (k == 0) return P;

    // :59-65  Atdense = Transpose(CopyColumns(AI, dense_cols))
    {
        Int nzd = 0;
        for (Int j : dense_cols) nzd += Ap[j + 1] - Ap[j];
        std::vector<Int> Cp(k + 1), Ci(nzd);
        Vec Cx(nzd);
        orc_copy_permute_scale(m, Ap, Ai, Ax, k, dense_cols.data(), nullptr,
                               nullptr, Cp.data(), Ci.data(), Cx.data());
        P->Atd_p.resize(m + 1);
        P->Atd_i.resize(nzd);
        P->Atd_x.resize(nzd);
        orc_transpose(m, k, Cp.data(), Ci.data(), Cx.data(), P->Atd_p.data(),
                      P->Atd_i.data(), P->Atd_x.data());
    }

    // :68-85  Schur complement S = inv(Wd) + Ad' inv(E) Ad, column by column
    P->chol.assign(k * k, 0.0);
    for (Int kk = 0; kk < k; kk++) {
        const Int j = dense_cols[kk];
        double* col = &P->chol[kk * k];
        for (Int p = Ap[j]; p < Ap[j + 1]; p++) {
            const Int i = Ai[p];
            const double alpha = Ax[p] / diag[i];
            for (Int pp = P->Atd_p[i]; pp < P->Atd_p[i + 1]; pp++)
                col[P->Atd_i[pp]] += alpha * P->Atd_x[pp];
        }
        const double w = W ? W[j] : 1.0;
        col[kk] += 1.0 / w;
    }

    // :88-92
    if (orc_dpotrf_lower(k, P->chol.data(), k) != 0) {
        *errflag = ORC_ERROR_lapack_chol;
        delete P;
        return nullptr;
    }
    P->work.assign(k, 0.0);
    return P;
}

// src/diagonal_precond.cc:121-159
extern "C" void orc_diag_apply(orc_diag_precond* P, const double* rhs,
                               double* lhs, double* dot) {
    const Int m = P->m, k = P->k;
    const Vec& diag = P->diagonal;
    double rldot = 0.0;
    if (k > 0) {
        Vec& work = P->work;
        std::fill(work.begin(), work.end(), 0.0);
        for (Int i = 0; i < m; i++) {
            const double alpha = rhs[i] / diag[i];
            for (Int pp = P->Atd_p[i]; pp < P->Atd_p[i + 1]; pp++)
                work[P->Atd_i[pp]] += alpha * P->Atd_x[pp];
        }
        orc_dpotrs_lower(k, P->chol.data(), k, work.data());
        for (Int i = 0; i < m; i++) {
            double d = 0.0;
            for (Int pp = P->Atd_p[i]; pp < P->Atd_p[i + 1]; pp++)
                d += work[P->Atd_i[pp]] * P->Atd_x[pp];
            d = rhs[i] - d;
            lhs[i] = d / diag[i];
            rldot += lhs[i] * rhs[i];
        }
    } else {
        for (Int i = 0; i < m; i++) {
            lhs[i] = rhs[i] / diag[i];
            rldot += lhs[i] * rhs[i];
        }
    }
    if (dot) *dot = rldot;
}

extern "C" Int orc_diag_num_dense(const orc_diag_precond* P) { return P->k; }

extern "C" void orc_diag_get(const orc_diag_precond* P, double* diagonal,
                             double* chol) {
    if (diagonal)
        std::memcpy(diagonal, P->diagonal.data(), sizeof(double) * P->m);
    if (chol && P->k > 0)
        std::memcpy(chol, P->chol.data(), sizeof(double) * P->k * P->k);
}

extern "C" void orc_diag_free(orc_diag_precond* P) { delete P; }

// ----------------------------------------------------------------------------
// ConjugateResiduals
// ----------------------------------------------------------------------------
static double ScaledInfnorm(Int m, const double* resscale, const double* r) {
    // src/conjugate_residuals.cc:44-49 / :131-136
    double resnorm = 0.0;
    if (resscale) {
        for (Int i = 0; i < m; i++)
            resnorm = std::max(resnorm, std::abs(resscale[i] * r[i]));
    } else {
        resnorm = orc_infnorm(m, r);
    }
    return resnorm;
}

// src/conjugate_residuals.cc:90-213
extern "C" Int orc_pcr_solve(Int m, orc_apply_fn C, void* Cctx, orc_apply_fn P,
                             void* Pctx, const double* rhs, double tol,
                             const double* resscale, Int maxiter, double* lhs,
                             Int* iter_out, double* resnorm_hist,
                             Int hist_cap) {
    Vec residual(m), sresidual(m), step(m), Csresidual(m), Cstep(m);
    double cdot = 0.0;
    double resnorm_precond_system = 0.0;
    Int errflag = 0, iter = 0, nhist = 0;
    if (maxiter < 0) maxiter = m + 100;

    // :117-126
    if (orc_infnorm(m, lhs) == 0.0) {
        for (Int i = 0; i < m; i++) residual[i] = rhs[i];
    } else {
        C(Cctx, lhs, residual.data(), nullptr);
        for (Int i = 0; i < m; i++) residual[i] = rhs[i] - residual[i];
    }
    P(Pctx, residual.data(), sresidual.data(), &resnorm_precond_system);
    C(Cctx, sresidual.data(), Csresidual.data(), &cdot);
    step = sresidual;
    Cstep = Csresidual;

    while (true) {
        const double resnorm = ScaledInfnorm(m, resscale, residual.data());
        if (resnorm_hist && nhist < hist_cap) resnorm_hist[nhist++] = resnorm;
        if (resnorm <= tol) break;
        if (iter == maxiter) { errflag = ORC_ERROR_cr_iter_limit; break; }
        if (cdot <= 0.0) { errflag = ORC_ERROR_cr_matrix_not_posdef; break; }

        // :157-178 -- Csresidual doubles as storage for P*Cstep
        double cdotnew;
        {
            double* precond_Cstep = Csresidual.data();
            double pdot;
            P(Pctx, Cstep.data(), precond_Cstep, &pdot);
            if (pdot <= 0.0) {
                errflag = ORC_ERROR_cr_precond_not_posdef;
                break;
            }
            const double alpha = cdot / pdot;
            if (!std::isfinite(alpha)) {
                errflag = ORC_ERROR_cr_inf_or_nan;
                break;
            }
            for (Int i = 0; i < m; i++) lhs[i] += alpha * step[i];
            for (Int i = 0; i < m; i++) residual[i] -= alpha * Cstep[i];
            for (Int i = 0; i < m; i++) sresidual[i] -= alpha * precond_Cstep[i];
            C(Cctx, sresidual.data(), Csresidual.data(), &cdotnew);
        }

        // :180-184
        const double beta = cdotnew / cdot;
        for (Int i = 0; i < m; i++) step[i] = sresidual[i] + beta * step[i];
        for (Int i = 0; i < m; i++) Cstep[i] = Csresidual[i] + beta * Cstep[i];
        cdot = cdotnew;

        iter++;
        // :186-207 refresh of the preconditioned residual + monotonicity test
        if (iter % 5 == 0) {
            double rsdot;
            P(Pctx, residual.data(), sresidual.data(), &rsdot);
            if (rsdot >= resnorm_precond_system) {
                errflag = ORC_ERROR_cr_no_progress;
                break;
            }
            resnorm_precond_system = rsdot;
        }
        // :209 InterruptCheck(): no time limit in the oracle
    }
    *iter_out = iter;
    return errflag;
}

// src/conjugate_residuals.cc:14-88
extern "C" Int orc_cr_solve(Int m, orc_apply_fn C, void* Cctx,
                            const double* rhs, double tol,
                            const double* resscale, Int maxiter, double* lhs,
                            Int* iter_out, double* resnorm_hist,
                            Int hist_cap) {
    Vec residual(m), step(m), Cresidual(m), Cstep(m);
    double cdot = 0.0;
    Int errflag = 0, iter = 0, nhist = 0;
    if (maxiter < 0) maxiter = m + 100;

    if (orc_infnorm(m, lhs) == 0.0) {
        for (Int i = 0; i < m; i++) residual[i] = rhs[i];
    } else {
        C(Cctx, lhs, residual.data(), nullptr);
        for (Int i = 0; i < m; i++) residual[i] = rhs[i] - residual[i];
    }
    C(Cctx, residual.data(), Cresidual.data(), &cdot);
    step = residual;
    Cstep = Cresidual;

    while (true) {
        const double resnorm = ScaledInfnorm(m, resscale, residual.data());
        if (resnorm_hist && nhist < hist_cap) resnorm_hist[nhist++] = resnorm;
        if (resnorm <= tol) break;
        if (iter == maxiter) { errflag = ORC_ERROR_cr_iter_limit; break; }
        if (cdot <= 0.0) { errflag = ORC_ERROR_cr_matrix_not_posdef; break; }

        const double denom = orc_dot(m, Cstep.data(), Cstep.data());
        const double alpha = cdot / denom;
        if (!std::isfinite(alpha)) {
            errflag = ORC_ERROR_cr_inf_or_nan;
            break;
        }
        for (Int i = 0; i < m; i++) lhs[i] += alpha * step[i];
        for (Int i = 0; i < m; i++) residual[i] -= alpha * Cstep[i];
        double cdotnew;
        C(Cctx, residual.data(), Cresidual.data(), &cdotnew);

        const double beta = cdotnew / cdot;
        for (Int i = 0; i < m; i++) step[i] = residual[i] + beta * step[i];
        for (Int i = 0; i < m; i++) Cstep[i] = Cresidual[i] + beta * Cstep[i];
        cdot = cdotnew;
        iter++;
    }
    *iter_out = iter;
    return errflag;
}

// ----------------------------------------------------------------------------
// KKTSolverDiag
// ----------------------------------------------------------------------------
struct orc_kkt_diag {
    Int m, n;
    const Int *Ap, *Ai;
    const double* Ax;
    Int nz_dense, precond_dense_cols, maxiter;
    Vec W, resscale;
    orc_diag_precond* precond = nullptr;
    bool factorized = false;
};

extern "C" orc_kkt_diag* orc_kkt_diag_new(Int m, Int n, const Int* Ap,
                                          const Int* Ai, const double* Ax,
                                          Int nz_dense, Int precond_dense_cols,
                                          Int maxiter) {
    orc_kkt_diag* K = new orc_kkt_diag;
    K->m = m; K->n = n; K->Ap = Ap; K->Ai = Ai; K->Ax = Ax;
    K->nz_dense = nz_dense;
    K->precond_dense_cols = precond_dense_cols;
    K->maxiter = maxiter;
    K->W.assign(n + m, 0.0);
    K->resscale.assign(m, 0.0);
    return K;
}

// src/kkt_solver_diag.cc:18-65
extern "C" Int orc_kkt_diag_factorize(orc_kkt_diag* K, const double* xl,
                                      const double* xu, const double* zl,
                                      const double* zu, double mu) {
    const Int m = K->m, n = K->n;
    K->factorized = false;
    if (xl) {
        double regval = mu;
        for (Int j = 0; j < n + m; j++) {
            const double g = zl[j] / xl[j] + zu[j] / xu[j];
            if (g != 0.0 && g < regval) regval = g;
            K->W[j] = 1.0 / g;  // infinity if g is zero
        }
        for (Int j = 0; j < n + m; j++)
            if (std::isinf(K->W[j])) K->W[j] = 1.0 / regval;
    } else {
        std::fill(K->W.begin(), K->W.end(), 1.0);
    }
    for (Int i = 0; i < m; i++) K->resscale[i] = 1.0 / std::sqrt(K->W[n + i]);

    if (K->precond) { orc_diag_free(K->precond); K->precond = nullptr; }
    Int errflag = 0;
    K->precond = orc_diag_factorize(m, n, K->Ap, K->Ai, K->Ax, K->W.data(),
                                    K->nz_dense, K->precond_dense_cols,
                                    &errflag);
    if (errflag) return errflag;
    K->factorized = true;
    return 0;
}

static void KktDiagApplyC(void* ctx, const double* rhs, double* lhs,
                          double* dot) {
    orc_kkt_diag* K = static_cast<orc_kkt_diag*>(ctx);
    orc_normal_apply(K->m, K->n, K->Ap, K->Ai, K->Ax, K->W.data(), rhs, lhs,
                     dot);
}
static void KktDiagApplyP(void* ctx, const double* rhs, double* lhs,
                          double* dot) {
    orc_diag_apply(static_cast<orc_kkt_diag*>(ctx)->precond, rhs, lhs, dot);
}

// src/kkt_solver_diag.cc:82-118
extern "C" Int orc_kkt_diag_solve(orc_kkt_diag* K, const double* a,
                                  const double* b, double tol, double* x,
                                  double* y, Int* iter, double* resnorm_hist,
                                  Int hist_cap) {
    const Int m = K->m, n = K->n;
    const Int* Ap = K->Ap; const Int* Ai = K->Ai; const double* Ax = K->Ax;
    const Vec& W = K->W;

    // :90-92  rhs = -b + AI*W*a, columns of [A I] in order
    Vec rhs(m);
    for (Int i = 0; i < m; i++) rhs[i] = -b[i];
    for (Int j = 0; j < n; j++) {
        const double alpha = W[j] * a[j];
        for (Int p = Ap[j]; p < Ap[j + 1]; p++) rhs[Ai[p]] += alpha * Ax[p];
    }
    for (Int i = 0; i < m; i++) rhs[i] += W[n + i] * a[n + i] * 1.0;

    for (Int i = 0; i < m; i++) y[i] = 0.0;
    const Int errflag = orc_pcr_solve(m, KktDiagApplyC, K, KktDiagApplyP, K,
                                      rhs.data(), tol, K->resscale.data(),
                                      K->maxiter, y, iter, resnorm_hist,
                                      hist_cap);

    // :108-117
    for (Int i = 0; i < m; i++) x[n + i] = b[i];
    for (Int j = 0; j < n; j++) {
        double aty = 0.0;
        for (Int p = Ap[j]; p < Ap[j + 1]; p++) aty += y[Ai[p]] * Ax[p];
        x[j] = W[j] * (a[j] - aty);
        for (Int p = Ap[j]; p < Ap[j + 1]; p++) x[n + Ai[p]] -= x[j] * Ax[p];
    }
    return errflag;
}

extern "C" void orc_kkt_diag_get(const orc_kkt_diag* K, double* W,
                                 double* resscale) {
    if (W) std::memcpy(W, K->W.data(), sizeof(double) * (K->n + K->m));
    if (resscale)
        std::memcpy(resscale, K->resscale.data(), sizeof(double) * K->m);
}

extern "C" void orc_kkt_diag_free(orc_kkt_diag* K) {
    if (K && K->precond) orc_diag_free(K->precond);
    delete K;
}

// ----------------------------------------------------------------------------
// sparse triangular solves (src/sparse_matrix.cc:224-311)
// ----------------------------------------------------------------------------
extern "C" Int orc_trisolve(Int dim, const Int* Ap, const Int* Ai,
                            const double* Ax, double* x, char trans, char uplo,
                            Int unitdiag) {
    const bool transposed = trans == 't' || trans == 'T';
    const bool upper = uplo == 'u' || uplo == 'U';
    const Int skip = unitdiag ? 0 : 1;
    Int nz = 0;
    if (transposed && upper) {
        // :232-246 gather, ascending; diagonal is the last entry of the column
        for (Int i = 0; i < dim; i++) {
            const Int begin = Ap[i], end = Ap[i + 1] - skip;
            double d = 0.0;
            for (Int p = begin; p < end; p++) d += x[Ai[p]] * Ax[p];
            x[i] -= d;
            if (!unitdiag) x[i] /= Ax[end];
            if (x[i] != 0.0) nz++;
        }
    } else if (transposed) {
        // :248-263 gather, descending; diagonal is the first entry
        for (Int i = dim - 1; i >= 0; i--) {
            const Int begin = Ap[i] + skip, end = Ap[i + 1];
            double d = 0.0;
            for (Int p = begin; p < end; p++) d += x[Ai[p]] * Ax[p];
            x[i] -= d;
            if (!unitdiag) x[i] /= Ax[begin - 1];
            if (x[i] != 0.0) nz++;
        }
    } else if (upper) {
        // :267-281 scatter, descending
        for (Int j = dim - 1; j >= 0; j--) {
            const Int begin = Ap[j], end = Ap[j + 1] - skip;
            if (!unitdiag) x[j] /= Ax[end];
            const double temp = x[j];
            if (temp != 0.0) {
                for (Int p = begin; p < end; p++) x[Ai[p]] -= Ax[p] * temp;
                nz++;
            }
        }
    } else {
        // :283-297 scatter, ascending
        for (Int j = 0; j < dim; j++) {
            const Int begin = Ap[j] + skip, end = Ap[j + 1];
            if (!unitdiag) x[j] /= Ax[begin - 1];
            const double temp = x[j];
            if (temp != 0.0) {
                for (Int p = begin; p < end; p++) x[Ai[p]] -= Ax[p] * temp;
                nz++;
            }
        }
    }
    return nz;
}

// :303-306
extern "C" void orc_forward_solve(Int dim, const Int* Lp, const Int* Li,
                                  const double* Lx, const Int* Up,
                                  const Int* Ui, const double* Ux, double* x) {
    orc_trisolve(dim, Lp, Li, Lx, x, 'n', 'l', 1);
    orc_trisolve(dim, Up, Ui, Ux, x, 'n', 'u', 0);
}

// :308-311
extern "C" void orc_backward_solve(Int dim, const Int* Lp, const Int* Li,
                                   const double* Lx, const Int* Up,
                                   const Int* Ui, const double* Ux, double* x) {
    orc_trisolve(dim, Up, Ui, Ux, x, 't', 'u', 0);
    orc_trisolve(dim, Lp, Li, Lx, x, 't', 'l', 1);
}

// src/sparse_matrix.cc:211-222
extern "C" void orc_add_normal_product(Int nrow, Int ncol, const Int* Ap,
                                       const Int* Ai, const double* Ax,
                                       const double* D, const double* rhs,
                                       double* lhs) {
    (void)nrow;
    for (Int j = 0; j < ncol; j++) {
        double temp = 0.0;
        for (Int p = Ap[j]; p < Ap[j + 1]; p++) temp += rhs[Ai[p]] * Ax[p];
        if (D) temp *= D[j] * D[j];
        for (Int p = Ap[j]; p < Ap[j + 1]; p++) lhs[Ai[p]] += temp * Ax[p];
    }
}

// ----------------------------------------------------------------------------
// SplittedNormalMatrix and KKTSolverBasis::_Solve
// ----------------------------------------------------------------------------
struct orc_split {
    Int m, n;
    std::vector<Int> AIp, AIi; Vec AIx;        // [A I], m x (n+m)
    std::vector<Int> Lp, Li; Vec Lx;           // unscaled L
    std::vector<Int> Up, Ui; Vec Ux, Ux0;      // Ux scaled, Ux0 as given
    std::vector<Int> Np, Ni; Vec Nx;
    std::vector<Int> rowperm, colperm, rowperm_inv, free_positions;
    std::vector<Int> basis, status;
    Vec colscale;
    Vec work;
};

// src/splitted_normal_matrix.cc:18-66
extern "C" orc_split* orc_split_prepare(
    Int m, Int n, const Int* AIp, const Int* AIi, const double* AIx,
    const Int* Lp, const Int* Li, const double* Lx, const Int* Up,
    const Int* Ui, const double* Ux, const Int* rowperm, const Int* colperm,
    const Int* basis, const Int* status, const double* colscale) {
    orc_split* S = new orc_split;
    S->m = m; S->n = n;
    S->AIp.assign(AIp, AIp + n + m + 1);
    S->AIi.assign(AIi, AIi + AIp[n + m]);
    S->AIx.assign(AIx, AIx + AIp[n + m]);
    S->Lp.assign(Lp, Lp + m + 1);
    S->Li.assign(Li, Li + Lp[m]);
    S->Lx.assign(Lx, Lx + Lp[m]);
    S->Up.assign(Up, Up + m + 1);
    S->Ui.assign(Ui, Ui + Up[m]);
    S->Ux.assign(Ux, Ux + Up[m]);
    S->Ux0 = S->Ux;
    S->rowperm.assign(rowperm, rowperm + m);
    S->colperm.assign(colperm, colperm + m);
    S->basis.assign(basis, basis + m);
    S->status.assign(status, status + n + m);
    S->colscale.assign(colscale, colscale + n + m);
    S->rowperm_inv.resize(m);
    orc_inverse_perm(m, rowperm, S->rowperm_inv.data());

    // :30-39 scale columns of U
    for (Int k = 0; k < m; k++) {
        const Int j = basis[colperm[k]];
        if (status[j] == ORC_BASIC) {
            const double d = colscale[j];
            for (Int p = S->Up[k]; p < S->Up[k + 1]; p++) S->Ux[p] *= d;
        }
    }

    // :42-55 N = AI[:,nonbasic], rows mapped by rowperm_inv, columns scaled
    std::vector<Int> nonbasic;
    for (Int j = 0; j < n + m; j++)
        if (status[j] == ORC_NONBASIC) nonbasic.push_back(j);
    Int nnzN = 0;
    for (Int j : nonbasic) nnzN += AIp[j + 1] - AIp[j];
    Vec scale(nonbasic.size());
    for (size_t k = 0; k < nonbasic.size(); k++) scale[k] = colscale[nonbasic[k]];
    S->Np.resize(nonbasic.size() + 1);
    S->Ni.resize(nnzN);
    S->Nx.resize(nnzN);
    orc_copy_permute_scale(m, AIp, AIi, AIx, nonbasic.size(), nonbasic.data(),
                           S->rowperm_inv.data(), scale.data(), S->Np.data(),
                           S->Ni.data(), S->Nx.data());

    // :58-64
    for (Int k = 0; k < m; k++)
        if (status[basis[colperm[k]]] == ORC_BASIC_FREE)
            S->free_positions.push_back(k);
    S->work.assign(m, 0.0);
    return S;
}

// src/splitted_normal_matrix.cc:90-117
extern "C" void orc_split_apply(orc_split* S, const double* rhs, double* lhs,
                                double* dot) {
    const Int m = S->m;
    double* work = S->work.data();
    for (Int i = 0; i < m; i++) work[i] = rhs[i];
    orc_backward_solve(m, S->Lp.data(), S->Li.data(), S->Lx.data(),
                       S->Up.data(), S->Ui.data(), S->Ux.data(), work);
    for (Int i = 0; i < m; i++) lhs[i] = 0.0;
    orc_add_normal_product(m, (Int)S->Np.size() - 1, S->Np.data(),
                           S->Ni.data(), S->Nx.data(), nullptr, work, lhs);
    orc_forward_solve(m, S->Lp.data(), S->Li.data(), S->Lx.data(),
                      S->Up.data(), S->Ui.data(), S->Ux.data(), lhs);
    for (Int i = 0; i < m; i++) lhs[i] += rhs[i];
    for (Int i : S->free_positions) lhs[i] = 0.0;
    if (dot) *dot = orc_dot(m, rhs, lhs);
}

extern "C" Int orc_split_get_sizes(const orc_split* S, Int* nnzN, Int* ncolN,
                                   Int* nfree) {
    if (nnzN) *nnzN = S->Ni.size();
    if (ncolN) *ncolN = (Int)S->Np.size() - 1;
    if (nfree) *nfree = S->free_positions.size();
    return S->m;
}

extern "C" void orc_split_get(const orc_split* S, Int* Np, Int* Ni, double* Nx,
                              double* Ux_scaled, Int* rowperm_inv,
                              Int* free_positions) {
    if (Np) std::copy(S->Np.begin(), S->Np.end(), Np);
    if (Ni) std::copy(S->Ni.begin(), S->Ni.end(), Ni);
    if (Nx) std::copy(S->Nx.begin(), S->Nx.end(), Nx);
    if (Ux_scaled) std::copy(S->Ux.begin(), S->Ux.end(), Ux_scaled);
    if (rowperm_inv)
        std::copy(S->rowperm_inv.begin(), S->rowperm_inv.end(), rowperm_inv);
    if (free_positions)
        std::copy(S->free_positions.begin(), S->free_positions.end(),
                  free_positions);
}

// Dense solve with the fresh (unscaled) factors; permutation handling as in
// the reference's own LU wrapper (src/forrest_tomlin.cc:67-78):
//   'N': work[i] = rhs[rowperm[i]]; (L+I)U work = work; lhs[colperm[i]] = work[i]
//   'T': work[i] = rhs[colperm[i]]; ((L+I)U)' work = work; lhs[rowperm[i]] = work[i]
extern "C" void orc_split_solve_dense(const orc_split* S, const double* rhs,
                                      double* lhs, char trans) {
    const Int m = S->m;
    Vec work(m);
    if (trans == 't' || trans == 'T') {
        for (Int i = 0; i < m; i++) work[i] = rhs[S->colperm[i]];
        orc_backward_solve(m, S->Lp.data(), S->Li.data(), S->Lx.data(),
                           S->Up.data(), S->Ui.data(), S->Ux0.data(),
                           work.data());
        for (Int i = 0; i < m; i++) lhs[S->rowperm[i]] = work[i];
    } else {
        for (Int i = 0; i < m; i++) work[i] = rhs[S->rowperm[i]];
        orc_forward_solve(m, S->Lp.data(), S->Li.data(), S->Lx.data(),
                          S->Up.data(), S->Ui.data(), S->Ux0.data(),
                          work.data());
        for (Int i = 0; i < m; i++) lhs[S->colperm[i]] = work[i];
    }
}

static void SplitApplyC(void* ctx, const double* rhs, double* lhs,
                        double* dot) {
    orc_split_apply(static_cast<orc_split*>(ctx), rhs, lhs, dot);
}

// src/kkt_solver_basis.cc:75-194
extern "C" Int orc_kkt_basis_solve(orc_split* S, const double* a,
                                   const double* b, double tol, Int maxiter,
                                   double* x, double* y, Int* iter,
                                   double* resnorm_hist, Int hist_cap) {
    const Int m = S->m, n = S->n;
    const Int* AIp = S->AIp.data(); const Int* AIi = S->AIi.data();
    const double* AIx = S->AIx.data();
    const std::vector<Int>& basis = S->basis;
    const std::vector<Int>& status = S->status;
    const Vec& colscale = S->colscale;
    Vec rhs(m, 0.0), work(m, 0.0);
    auto dot_column = [&](Int j, const Vec& v) {
        double d = 0.0;
        for (Int p = AIp[j]; p < AIp[j + 1]; p++) d += v[AIi[p]] * AIx[p];
        return d;
    };
    auto scatter_column = [&](Int j, double alpha, Vec& v) {
        for (Int p = AIp[j]; p < AIp[j + 1]; p++) v[AIi[p]] += alpha * AIx[p];
    };

    // :87-99
    Int num_free = 0;
    for (Int p = 0; p < m; p++) {
        const Int j = basis[p];
        if (status[j] == ORC_BASIC_FREE) { work[p] = a[j]; num_free++; }
    }
    if (num_free > 0) {
        Vec tmp(work);
        orc_split_solve_dense(S, tmp.data(), work.data(), 'T');
    }

    // :101-121
    for (Int j = 0; j < n + m; j++) {
        if (status[j] != ORC_NONBASIC) continue;
        const double d2 = colscale[j] * colscale[j];
        double alpha;
        if (num_free > 0) {
            alpha = a[j] - dot_column(j, work);
            alpha *= d2;
        } else {
            alpha = d2 * a[j];
        }
        scatter_column(j, alpha, rhs);
    }
    {
        Vec tmp(rhs);
        orc_split_solve_dense(S, tmp.data(), rhs.data(), 'N');
    }

    // :124
    orc_split_solve_dense(S, b, work.data(), 'N');

    // :128-138
    for (Int p = 0; p < m; p++) {
        const Int j = basis[p];
        if (status[j] == ORC_BASIC) {
            const double d = colscale[j];
            rhs[p] = (rhs[p] - work[p]) / d + a[j] * d;
        } else {
            rhs[p] = 0.0;
        }
    }

    // :141-143
    for (Int k = 0; k < m; k++) work[k] = rhs[S->colperm[k]];

    // :146-157
    Vec lhs(m, 0.0);
    const Int errflag = orc_cr_solve(m, SplitApplyC, S, work.data(), tol,
                                     nullptr, maxiter, lhs.data(), iter,
                                     resnorm_hist, hist_cap);

    // :160-161
    for (Int k = 0; k < m; k++) y[S->colperm[k]] = lhs[k];

    // :164-175
    for (Int p = 0; p < m; p++) {
        const Int j = basis[p];
        if (status[j] == ORC_BASIC) y[p] /= colscale[j];
        else y[p] = a[j];
    }
    {
        Vec tmp(y, y + m);
        orc_split_solve_dense(S, tmp.data(), y, 'T');
    }

    // :178-188
    Vec yv(y, y + m);
    for (Int i = 0; i < m; i++) work[i] = b[i];
    for (Int j = 0; j < n + m; j++) {
        double xj = 0.0;
        if (status[j] == ORC_NONBASIC) {
            xj = a[j] - dot_column(j, yv);
            xj *= colscale[j] * colscale[j];
            scatter_column(j, -xj, work);
        }
        x[j] = xj;
    }

    // :191-193
    {
        Vec tmp(work);
        orc_split_solve_dense(S, tmp.data(), work.data(), 'N');
    }
    for (Int p = 0; p < m; p++) x[basis[p]] = work[p];
    return errflag;
}

extern "C" void orc_split_free(orc_split* S) { delete S; }

// ---------------------------------------------------------------------------
// IPM::SolveNewtonSystem, src/ipm.cc:532-645.
// ipm.cc cannot be linked on the CPU alone (it needs ipx::Basis, hence BASICLU); a
// line-by-line restatement, checked by the Newton equations it must satisfy (tests/)
// and, through the device code held equal to it, against the reference's own
// IPM::Driver (tests/dropin/ipm_main.cc, GPU box).
// state[j]: 0 fixed, 1 free, 2 barrier lb, 3 barrier ub, 4 barrier boxed
// (Iterate::StateOf / has_barrier_lb / has_barrier_ub, src/iterate.h:99-108).
// ---------------------------------------------------------------------------
namespace {
template <class Solve>
Int NewtonSolve(Int m, Int n, const Int* AIp, const Int* AIi, const double* AIx,
                bool have_identity, Solve&& kkt_solve, const double* rb,
                const double* rc, const double* rl, const double* ru,
                const double* sl, const double* su, const double* xl,
                const double* xu, const double* zl, const double* zu,
                const unsigned char* state, double* dx, double* dxl,
                double* dxu, double* dy, double* dzl, double* dzu) {
    auto has_lb = [&](Int j) { return state[j] == 2 || state[j] == 4; };
    auto has_ub = [&](Int j) { return state[j] == 3 || state[j] == 4; };
    auto fixed = [&](Int j) { return state[j] == 0; };
    auto barrier = [&](Int j) { return state[j] >= 2; };
    // :551-566
    Vec rhs1(n + m, 0.0), rhs2(m, 0.0);
    if (rc) for (Int j = 0; j < n + m; j++) rhs1[j] = -rc[j];
    for (Int j = 0; j < n + m; j++) {
        const double rlj = rl ? rl[j] : 0.0, ruj = ru ? ru[j] : 0.0;
        if (has_lb(j)) rhs1[j] += (sl[j] + zl[j] * rlj) / xl[j];
        if (has_ub(j)) rhs1[j] -= (su[j] - zu[j] * ruj) / xu[j];
        if (fixed(j)) rhs1[j] = 0.0;
    }
    if (rb) std::copy(rb, rb + m, rhs2.begin());
    // :569-573
    const Int errflag = kkt_solve(rhs1.data(), rhs2.data(), dx, dy);
    if (errflag) return errflag;
    // :576-611
    for (Int i = 0; i < m; i++) dy[i] *= -1.0;
    for (Int j = 0; j < n + m; j++) {
        if (!barrier(j)) { dxl[j] = 0.0; dzl[j] = 0.0; continue; }
        const double rlj = rl ? rl[j] : 0.0;
        dxl[j] = dx[j] - rlj;
        dzl[j] = (sl[j] - zl[j] * dxl[j]) / xl[j];
    }
    for (Int j = 0; j < n + m; j++) {
        if (!barrier(j)) { dxu[j] = 0.0; dzu[j] = 0.0; continue; }
        const double ruj = ru ? ru[j] : 0.0;
        dxu[j] = ruj - dx[j];
        dzu[j] = (su[j] - zu[j] * dxu[j]) / xu[j];
    }
    // :617-633
    for (Int j = 0; j < n + m; j++) {
        if (!barrier(j)) continue;
        double atdy = 0.0;
        if (j < n || have_identity) {
            for (Int p = AIp[j]; p < AIp[j + 1]; p++) atdy += dy[AIi[p]] * AIx[p];
        } else {
            atdy = dy[j - n] * 1.0;     // slack column of AI
        }
        const double rcj = rc ? rc[j] : 0.0;
        if (std::isfinite(xl[j]) && std::isfinite(xu[j])) {
            if (zl[j] * xu[j] >= zu[j] * xl[j]) dzl[j] = rcj + dzu[j] - atdy;
            else dzu[j] = -rcj + dzl[j] + atdy;
        } else if (std::isfinite(xl[j])) {
            dzl[j] = rcj + dzu[j] - atdy;
        } else {
            dzu[j] = -rcj + dzl[j] + atdy;
        }
    }
    return 0;
}
}  // namespace

extern "C" Int orc_newton_solve_diag(orc_kkt_diag* K, const double* rb,
    const double* rc, const double* rl, const double* ru, const double* sl,
    const double* su, const double* xl, const double* xu, const double* zl,
    const double* zu, const unsigned char* state, double tol, double* dx,
    double* dxl, double* dxu, double* dy, double* dzl, double* dzu, Int* iter) {
    return NewtonSolve(K->m, K->n, K->Ap, K->Ai, K->Ax, false,
        [&](const double* a, const double* b, double* x, double* y) {
            return orc_kkt_diag_solve(K, a, b, tol, x, y, iter, nullptr, 0);
        }, rb, rc, rl, ru, sl, su, xl, xu, zl, zu, state, dx, dxl, dxu, dy, dzl, dzu);
}

extern "C" Int orc_newton_solve_basis(orc_split* S, const double* rb,
    const double* rc, const double* rl, const double* ru, const double* sl,
    const double* su, const double* xl, const double* xu, const double* zl,
    const double* zu, const unsigned char* state, double tol, Int maxiter,
    double* dx, double* dxl, double* dxu, double* dy, double* dzl, double* dzu,
    Int* iter) {
    return NewtonSolve(S->m, S->n, S->AIp.data(), S->AIi.data(), S->AIx.data(), true,
        [&](const double* a, const double* b, double* x, double* y) {
            return orc_kkt_basis_solve(S, a, b, tol, maxiter, x, y, iter, nullptr, 0);
        }, rb, rc, rl, ru, sl, su, xl, xu, zl, zu, state, dx, dxl, dxu, dy, dzl, dzu);
}

// ---------------------------------------------------------------------------
// Iterate::Update / ComputeResiduals / ComputeComplementarity
// (src/iterate.cc:94-139, 536-588, 642-670) and StepToBoundary (src/ipm.cc:320-339).
// State codes as above.  Pinned against the reference's ipx::Iterate
// (oracle/_ref) in tests/test_oracle_vs_ref.py.
// ---------------------------------------------------------------------------
static const double kOrcBarrierMin = 1e-30;   // Iterate::kBarrierMin, src/iterate.h

extern "C" void orc_iterate_update(Int m, Int n, const unsigned char* state,
    double* x, double* xl, double* xu, double* y, double* zl, double* zu,
    double sp, const double* dx, const double* dxl, const double* dxu,
    double sd, const double* dy, const double* dzl, const double* dzu) {
    auto has_lb = [&](Int j) { return state[j] == 2 || state[j] == 4; };
    auto has_ub = [&](Int j) { return state[j] == 3 || state[j] == 4; };
    if (dx) for (Int j = 0; j < n + m; j++) if (state[j] != 0) x[j] += sp * dx[j];
    if (dxl) for (Int j = 0; j < n + m; j++) if (has_lb(j)) { xl[j] += sp * dxl[j]; xl[j] = std::max(xl[j], kOrcBarrierMin); }
    if (dxu) for (Int j = 0; j < n + m; j++) if (has_ub(j)) { xu[j] += sp * dxu[j]; xu[j] = std::max(xu[j], kOrcBarrierMin); }
    if (dy) for (Int i = 0; i < m; i++) y[i] += sd * dy[i];
    if (dzl) for (Int j = 0; j < n + m; j++) if (has_lb(j)) { zl[j] += sd * dzl[j]; zl[j] = std::max(zl[j], kOrcBarrierMin); }
    if (dzu) for (Int j = 0; j < n + m; j++) if (has_ub(j)) { zu[j] += sd * dzu[j]; zu[j] = std::max(zu[j], kOrcBarrierMin); }
}

// A: the n structural columns; the slack identity of AI is applied implicitly.
extern "C" void orc_iterate_residuals(Int m, Int n, const Int* Ap, const Int* Ai,
    const double* Ax, const unsigned char* state, const double* b,
    const double* c, const double* lb, const double* ub, const double* x,
    const double* xl, const double* xu, const double* y, const double* zl,
    const double* zu, double* rb, double* rc, double* rl, double* ru,
    double* norms) {
    // :543-545  rb = b - AI*x, columns in order (MultiplyAdd 'N', sparse_matrix.cc:194-209)
    for (Int i = 0; i < m; i++) rb[i] = b[i];
    for (Int j = 0; j < n; j++) {
        const double alpha = -1.0 * x[j];
        for (Int p = Ap[j]; p < Ap[j + 1]; p++) rb[Ai[p]] += alpha * Ax[p];
    }
    for (Int i = 0; i < m; i++) rb[i] += (-1.0 * x[n + i]) * 1.0;
    // :550-556  rc = c - zl + zu - AI'y, zero on fixed variables
    for (Int j = 0; j < n + m; j++) rc[j] = c[j] - zl[j] + zu[j];
    for (Int j = 0; j < n; j++) {
        double d = 0.0;
        for (Int p = Ap[j]; p < Ap[j + 1]; p++) d += y[Ai[p]] * Ax[p];
        rc[j] += -1.0 * d;
    }
    for (Int i = 0; i < m; i++) rc[n + i] += -1.0 * (y[i] * 1.0);
    for (Int j = 0; j < n + m; j++) if (state[j] == 0) rc[j] = 0.0;
    // :566-577
    for (Int j = 0; j < n + m; j++)
        rl[j] = (state[j] == 2 || state[j] == 4) ? lb[j] - x[j] + xl[j] : 0.0;
    for (Int j = 0; j < n + m; j++)
        ru[j] = (state[j] == 3 || state[j] == 4) ? ub[j] - x[j] - xu[j] : 0.0;
    // :584-587
    double pres = orc_infnorm(m, rb);
    pres = std::max(pres, orc_infnorm(n + m, rl));
    pres = std::max(pres, orc_infnorm(n + m, ru));
    norms[0] = pres;
    norms[1] = orc_infnorm(n + m, rc);
}

// out4: complementarity, mu, mu_min, mu_max
extern "C" void orc_iterate_complementarity(Int N, const unsigned char* state,
    const double* xl, const double* xu, const double* zl, const double* zu,
    double* out4) {
    double comp = 0.0, mu_min = INFINITY, mu_max = 0.0, mu = 0.0;
    Int num_finite = 0;
    for (Int j = 0; j < N; j++)
        if (state[j] == 2 || state[j] == 4) {
            comp += xl[j] * zl[j];
            mu_min = std::min(mu_min, xl[j] * zl[j]);
            mu_max = std::max(mu_max, xl[j] * zl[j]);
            num_finite++;
        }
    for (Int j = 0; j < N; j++)
        if (state[j] == 3 || state[j] == 4) {
            comp += xu[j] * zu[j];
            mu_min = std::min(mu_min, xu[j] * zu[j]);
            mu_max = std::max(mu_max, xu[j] * zu[j]);
            num_finite++;
        }
    if (num_finite > 0) mu = comp / num_finite;
    else mu = mu_min = 0.0;
    out4[0] = comp; out4[1] = mu; out4[2] = mu_min; out4[3] = mu_max;
}

// src/ipm.cc:320-339
extern "C" double orc_step_to_boundary(Int len, const double* x, const double* dx,
                                       double alpha, Int* blocking_index) {
    const double damp = 1.0 - std::numeric_limits<double>::epsilon();
    Int iblock = -1;
    for (Int i = 0; i < len; i++) {
        if (x[i] + alpha * dx[i] < 0.0) {
            alpha = -(x[i] * damp) / dx[i];
            iblock = i;
        }
    }
    if (blocking_index) *blocking_index = iblock;
    return alpha;
}

// ---------------------------------------------------------------------------
// One IPM step: IPM::Predictor, AddCorrector, StepSizes, MakeStep
// (src/ipm.cc:340-530) around KKTSolverDiag.  A restatement line by line, built
// from the pinned pieces above; pinned through the device code (tests/dropin/ipm_main.cc).
// info: step_primal, step_dual, mu_before, mu_after, sigma, kktiter_predictor,
//       kktiter_corrector  (7 doubles)
// ---------------------------------------------------------------------------
extern "C" Int orc_ipm_step_diag(orc_kkt_diag* K, const unsigned char* state,
    const double* b, const double* c, const double* lb, const double* ub,
    double* x, double* xl, double* xu, double* y, double* zl, double* zu,
    double kkt_tol, double* info) {
    const Int m = K->m, n = K->n, N = n + m;
    Vec rb(m), rc(N), rl(N), ru(N), sl(N), su(N), dx(N), dxl(N), dxu(N), dy(m), dzl(N), dzu(N);
    double norms[2], comp[4];
    orc_iterate_residuals(m, n, K->Ap, K->Ai, K->Ax, state, b, c, lb, ub, x, xl, xu, y, zl, zu,
                          rb.data(), rc.data(), rl.data(), ru.data(), norms);
    orc_iterate_complementarity(N, state, xl, xu, zl, zu, comp);
    const double mu = comp[1];
    info[2] = mu;
    const double tol = kkt_tol * std::sqrt(mu);
    auto has_lb = [&](Int j) { return state[j] == 2 || state[j] == 4; };
    auto has_ub = [&](Int j) { return state[j] == 3 || state[j] == 4; };
    // Predictor :340-371
    for (Int j = 0; j < N; j++) sl[j] = has_lb(j) ? -xl[j] * zl[j] : 0.0;
    for (Int j = 0; j < N; j++) su[j] = has_ub(j) ? -xu[j] * zu[j] : 0.0;
    Int iter = 0;
    Int err = orc_newton_solve_diag(K, rb.data(), rc.data(), rl.data(), ru.data(), sl.data(), su.data(),
                                    xl, xu, zl, zu, state, tol, dx.data(), dxl.data(), dxu.data(),
                                    dy.data(), dzl.data(), dzu.data(), &iter);
    info[5] = (double)iter;
    if (err) return err;
    // AddCorrector :373-435
    double step_xl = orc_step_to_boundary(N, xl, dxl.data(), 1.0, nullptr);
    double step_xu = orc_step_to_boundary(N, xu, dxu.data(), 1.0, nullptr);
    double step_zl = orc_step_to_boundary(N, zl, dzl.data(), 1.0, nullptr);
    double step_zu = orc_step_to_boundary(N, zu, dzu.data(), 1.0, nullptr);
    double maxp = std::min(step_xl, step_xu), maxd = std::min(step_zl, step_zu);
    double muaff = 0.0;
    Int num_finite = 0;
    for (Int j = 0; j < N; j++) {
        if (has_lb(j)) { muaff += (xl[j] + maxp * dxl[j]) * (zl[j] + maxd * dzl[j]); num_finite++; }
        if (has_ub(j)) { muaff += (xu[j] + maxp * dxu[j]) * (zu[j] + maxd * dzu[j]); num_finite++; }
    }
    muaff /= num_finite;
    const double ratio = muaff / mu;
    const double sigma = ratio * ratio * ratio;
    info[4] = sigma;
    for (Int j = 0; j < N; j++) sl[j] = has_lb(j) ? -xl[j] * zl[j] + sigma * mu - dxl[j] * dzl[j] : 0.0;
    for (Int j = 0; j < N; j++) su[j] = has_ub(j) ? -xu[j] * zu[j] + sigma * mu - dxu[j] * dzu[j] : 0.0;
    err = orc_newton_solve_diag(K, rb.data(), rc.data(), rl.data(), ru.data(), sl.data(), su.data(),
                                xl, xu, zl, zu, state, tol, dx.data(), dxl.data(), dxu.data(),
                                dy.data(), dzl.data(), dzu.data(), &iter);
    info[6] = (double)iter;
    if (err) return err;
    // StepSizes :437-516
    const double gammaf = 0.9, gammaa = 1.0 / (1.0 - gammaf);
    Int block_xl, block_xu, block_zl, block_zu;
    step_xl = orc_step_to_boundary(N, xl, dxl.data(), 1.0, &block_xl);
    step_xu = orc_step_to_boundary(N, xu, dxu.data(), 1.0, &block_xu);
    step_zl = orc_step_to_boundary(N, zl, dzl.data(), 1.0, &block_zl);
    step_zu = orc_step_to_boundary(N, zu, dzu.data(), 1.0, &block_zu);
    maxp = std::fmin(step_xl, step_xu);
    maxd = std::fmin(step_zl, step_zu);
    double mufull = 0.0;
    for (Int j = 0; j < N; j++) {
        if (has_lb(j)) mufull += (xl[j] + maxp * dxl[j]) * (zl[j] + maxd * dzl[j]);
        if (has_ub(j)) mufull += (xu[j] + maxp * dxu[j]) * (zu[j] + maxd * dzu[j]);
    }
    mufull /= num_finite;
    mufull /= gammaa;
    double alphap = 1.0, alphad = 1.0;
    if (maxp < 1.0) {
        double buffer;
        if (step_xl <= step_xu) {
            const Int bp = block_xl;
            buffer = mufull / (zl[bp] + maxd * dzl[bp]);
            alphap = (xl[bp] - buffer) / (-dxl[bp]);
        } else {
            const Int bp = block_xu;
            buffer = mufull / (zu[bp] + maxd * dzu[bp]);
            alphap = (xu[bp] - buffer) / (-dxu[bp]);
        }
        alphap = std::max(alphap, gammaf * maxp);
        alphap = std::min(alphap, 1.0);
    }
    if (maxd < 1.0) {
        double buffer;
        if (step_zl <= step_zu) {
            const Int bd = block_zl;
            buffer = mufull / (xl[bd] + maxp * dxl[bd]);
            alphad = (zl[bd] - buffer) / (-dzl[bd]);
        } else {
            const Int bd = block_zu;
            buffer = mufull / (xu[bd] + maxp * dxu[bd]);
            alphad = (zu[bd] - buffer) / (-dzu[bd]);
        }
        alphad = std::max(alphad, gammaf * maxd);
        alphad = std::min(alphad, 1.0);
    }
    const double sp = std::min(alphap, 1.0 - 1e-6), sd = std::min(alphad, 1.0 - 1e-6);
    info[0] = sp; info[1] = sd;
    // MakeStep :518-530
    orc_iterate_update(m, n, state, x, xl, xu, y, zl, zu, sp, dx.data(), dxl.data(), dxu.data(), sd,
                       dy.data(), dzl.data(), dzu.data());
    orc_iterate_complementarity(N, state, xl, xu, zl, zu, comp);
    info[3] = comp[1];
    return 0;
}

// ---------------------------------------------------------------------------
// Iterate::ComputeObjectives, src/iterate.cc:590-640, for an iterate that has not been postprocessed and
// whose variables are fixed / free / barrier (the implied states are only set by the basis solver's drop
// procedures).  out3 = pobjective, dobjective, offset (pobjective + offset is the primal objective after
// postprocessing, :203-211).  Pinned against the reference's Iterate (tests/test_oracle_vs_ref.py).
// ---------------------------------------------------------------------------
extern "C" void orc_iterate_objectives(Int m, Int n, const Int* Ap, const Int* Ai, const double* Ax,
    const unsigned char* state, const double* b, const double* c, const double* lb, const double* ub,
    const double* x, const double* y, const double* zl, const double* zu, double* out3) {
    const Int N = n + m;
    double offset = 0.0, pobj = 0.0;
    for (Int j = 0; j < N; j++) {                    // :615-626
        if (state[j] != 0) pobj += c[j] * x[j];
        else offset += c[j] * x[j];
    }
    double dobj = 0.0;                               // :627 Dot(b, y)
    for (Int i = 0; i < m; i++) dobj += b[i] * y[i];
    for (Int j = 0; j < N; j++) {                    // :628-638
        if (state[j] == 2 || state[j] == 4) dobj += lb[j] * zl[j];
        if (state[j] == 3 || state[j] == 4) dobj -= ub[j] * zu[j];
        if (state[j] == 0) {
            double d = 0.0;                          // DotColumn(AI, j, y)
            if (j < n) for (Int p = Ap[j]; p < Ap[j + 1]; p++) d += y[Ai[p]] * Ax[p];
            else d = y[j - n] * 1.0;
            dobj -= x[j] * d;
        }
    }
    out3[0] = pobj; out3[1] = dobj; out3[2] = offset;
}

// Model::ComputeNorms, src/model.cc:58-67: norm_bounds, norm_c
extern "C" void orc_model_norms(Int m, Int n, const double* b, const double* c, const double* lb,
                                const double* ub, double* out2) {
    double nb = 0.0, nc = 0.0;
    for (Int i = 0; i < m; i++) nb = std::max(nb, std::abs(b[i]));
    for (Int j = 0; j < n + m; j++) {
        nc = std::max(nc, std::abs(c[j]));
        if (std::isfinite(lb[j])) nb = std::max(nb, std::abs(lb[j]));
        if (std::isfinite(ub[j])) nb = std::max(nb, std::abs(ub[j]));
    }
    out2[0] = nb; out2[1] = nc;
}

// ---------------------------------------------------------------------------
// IPM::Driver, src/ipm.cc:56-123, around KKTSolverDiag: termination test (Iterate::term_crit_reached with
// crossover_start = 0, iterate.cc:221-249), divergence / bad-iteration test with the infeasibility
// classification, iteration limit, Factorize, Predictor + AddCorrector + MakeStep (orc_ipm_step_diag), the
// bad-iteration count and best complementarity of MakeStep (:520-530).  Built from pinned pieces; the device driver held
// equal to it runs against the reference's own IPM::Driver (tests/dropin/ipm_main.cc).  Returns status_ipm (IPX_STATUS_*).
// info[10] = iter, errflag, kktiter, pobjective and dobjective after postprocessing, presidual, dresidual,
//            complementarity, mu, last min(step_primal, step_dual)
// ---------------------------------------------------------------------------
extern "C" Int orc_ipm_driver_diag(orc_kkt_diag* K, const unsigned char* state, const double* b,
    const double* c, const double* lb, const double* ub, double* x, double* xl, double* xu, double* y,
    double* zl, double* zu, double kkt_tol, double feasibility_tol, double optimality_tol, Int ipm_maxiter,
    double* info) {
    const Int m = K->m, n = K->n, N = n + m;
    constexpr double kDivergeTol = 1e6;              // src/ipm.h:55
    double norms_model[2];
    orc_model_norms(m, n, b, c, lb, ub, norms_model);
    Vec rb(m), rc(N), rl(N), ru(N);
    double comp[4], res[2], obj[3];
    orc_iterate_complementarity(N, state, xl, xu, zl, zu, comp);
    double best_complementarity = comp[0];           // :315
    Int num_bad_iter = 0, iter = 0, errflag = 0, status = 0, kktiter = 0;
    double last_step = 0.0;
    while (true) {
        orc_iterate_residuals(m, n, K->Ap, K->Ai, K->Ax, state, b, c, lb, ub, x, xl, xu, y, zl, zu,
                              rb.data(), rc.data(), rl.data(), ru.data(), res);
        orc_iterate_complementarity(N, state, xl, xu, zl, zu, comp);
        orc_iterate_objectives(m, n, K->Ap, K->Ai, K->Ax, state, b, c, lb, ub, x, y, zl, zu, obj);
        const double pobjective = obj[0] + obj[2], dobjective = obj[1] + obj[2];
        info[3] = pobjective; info[4] = dobjective; info[5] = res[0]; info[6] = res[1];
        info[7] = comp[0]; info[8] = comp[1];
        const bool feasible = res[0] <= feasibility_tol * (1.0 + norms_model[0]) &&
                              res[1] <= feasibility_tol * (1.0 + norms_model[1]);
        const double mid = 0.5 * (pobjective + dobjective), gap = pobjective - dobjective;
        const bool optimal = std::abs(gap) <= optimality_tol * (1.0 + std::abs(mid));
        if (feasible && optimal) { status = 1; break; }                             // IPX_STATUS_optimal
        if (num_bad_iter >= 5 || comp[0] > kDivergeTol * best_complementarity) {     // :71-93
            if (dobjective > std::max(10.0 * std::abs(pobjective), 1.0)) status = 3;         // primal_infeas
            else if (pobjective < -std::max(10.0 * std::abs(dobjective), 1.0)) status = 4;   // dual_infeas
            else status = 7;                                                                 // no_progress
            break;
        }
        if (iter >= ipm_maxiter) { status = 6; break; }                              // iter_limit
        errflag = orc_kkt_diag_factorize(K, xl, xu, zl, zu, comp[1]);
        if (errflag) break;
        double sinfo[7];
        errflag = orc_ipm_step_diag(K, state, b, c, lb, ub, x, xl, xu, y, zl, zu, kkt_tol, sinfo);
        kktiter += (Int)sinfo[5] + (Int)sinfo[6];
        if (errflag) break;
        last_step = std::min(sinfo[0], sinfo[1]);     // :524-527
        if (last_step < 0.05) num_bad_iter++; else num_bad_iter = 0;
        orc_iterate_complementarity(N, state, xl, xu, zl, zu, comp);
        best_complementarity = std::min(best_complementarity, comp[0]);
        iter++;
    }
    if (errflag) status = errflag == 999 ? 5 : 8;     // :114-121 time_limit / failed
    info[0] = (double)iter; info[1] = (double)(errflag == 999 ? 0 : errflag); info[2] = (double)kktiter;
    info[9] = last_step;
    return status;
}

// ---------------------------------------------------------------------------
// LU factorization of a basis matrix behind the reference's LuFactorization contract
// (src/lu_factorization.h:21-58):  B[rowperm,colperm] = (L+I)*U, L strictly lower without its diagonal,
// U upper with the diagonal last in each column, indices sorted, dependent columns replaced by unit
// columns and listed.  The reference's kernel for this is BASICLU (third party, NOT in /root/reference:
// install.txt:1-3, pinned commit 7b41d962cd345057946b84ac41d525efaba4b871, call site
// src/basiclu_kernel.cc:31-82): its published scheme -- pivot the column singletons and the row singletons
// first (no arithmetic, no fill), then factorize the remaining "bump" with threshold pivoting -- is what is
// restated here, in the form the device code uses it:
//   * the singletons are taken in ROUNDS (all current column singletons, then all current row singletons,
//     until neither exists); within a round the pivots are independent, ordered by column (row) index;
//     two singleton columns in one row: the smaller column index wins; two singleton rows in one column:
//     the larger |entry| wins (ties: smaller row index); a row singleton must pass the relative threshold
//     |a| >= pivottol * max|active entries of its column| as well as the absolute one;
//   * the bump is factorized as a dense matrix with partial pivoting (largest |entry| of the column among
//     the rows not yet pivoted, ties: smaller row), columns in ascending index order; a column whose largest
//     entry is below the absolute tolerance (kLuDependencyTol if strict_abs_pivottol, src/ipx_internal.h:26,
//     else 1e-14, BASICLU's default) is dependent;
//   * dependent columns come last, paired with the left-over rows in ascending order;
//   * a bump of more than bump_limit rows is not factorized densely as it stands: it is TORN first.  Whenever the
//     rounds stall, the T active columns with the most active entries (ties: smaller index) are set aside as
//     SPIKES (T = 1, doubled up to 1024 while a tear frees fewer than 64 pivots, back to 1 otherwise) and the
//     rounds go on without them, until no active column is left.  Spikes are never pivots of a round, so every
//     round pivot still costs no arithmetic outside them; the spikes themselves receive the updates of the row
//     singleton pivots in pivot order (a forward substitution with the L columns found so far), their entries in
//     pivoted rows become entries of U, and their entries in the rows that were never pivoted form the dense block
//     that is then factorized with partial pivoting as above (refused if it has more than bump_limit rows).
//     This is the classical bump-and-spike ordering of LP bases (Hellerman-Rarick) restated for rounds.
// PARITY UNPINNED against BASICLU's pivot order and values (no fixture in the reference holds them:
// check/solver.cc asserts statuses only).  What IS pinned: the contract, through the reference's own
// LuFactorization::Factorize / stability() (src/lu_factorization.cc:87-127) and ForrestTomlin
// (src/forrest_tomlin.cc) running on these factors in oracle/ref_driver.cc.
// ---------------------------------------------------------------------------
struct orc_lu {
    Int dim = 0;
    std::vector<Int> Lp, Li, Up, Ui, rowperm, colperm, dependent;
    std::vector<double> Lx, Ux;
    Int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // col singletons, row singletons, bump size, rounds, dependent
};

static orc_lu* lu_factorize_impl(Int dim, const Int* Bbegin, const Int* Bend, const Int* Bi_in, const double* Bx_in,
                                 double pivottol, int strict_abs_pivottol, Int bump_limit, int sparse_rounds, Int sparse_min, Int slow_den, Int fill_max,
                                 Int sparse_from = -2, double dense_at = 0.0, int fill_to_dense = 0) {
    if (sparse_from == -2) sparse_from = bump_limit;       // (rounds for bumps of more than sparse_from rows; until round 4: the dense limit)
    const double abstol = strict_abs_pivottol ? 1e-3 : 1e-14;
    std::unique_ptr<orc_lu> F(new orc_lu);
    F->dim = dim;
    // the CURRENT matrix: B at first; with sparse rounds, the active submatrix after every elimination round
    std::vector<Int> cp(dim + 1, 0), ci;
    std::vector<double> cx;
    for (Int j = 0; j < dim; j++) {
        for (Int p = Bbegin[j]; p < Bend[j]; p++) { ci.push_back(Bi_in[p]); cx.push_back(Bx_in[p]); }
        cp[j + 1] = (Int)ci.size();
    }
    const int64_t nnz_B = cp[dim];
    // the entries that have left the current matrix because their row or column was pivoted, with the value they had then
    std::vector<Int> Ei, Ej;
    std::vector<double> Ex;
    // row-wise copy: entries of row i in ascending column order; counts of the entries
    std::vector<Int> rp, rj, rc(dim), cc(dim);
    std::vector<double> rx;
    auto rebuild_rows = [&]() {
        rp.assign(dim + 1, 0);
        for (Int j = 0; j < dim; j++)
            for (Int p = cp[j]; p < cp[j + 1]; p++) rp[ci[p] + 1]++;
        for (Int i = 0; i < dim; i++) rp[i + 1] += rp[i];
        rj.assign(rp[dim], 0);
        rx.assign(rp[dim], 0.0);
        std::vector<Int> cur(rp.begin(), rp.end() - 1);
        for (Int j = 0; j < dim; j++)
            for (Int p = cp[j]; p < cp[j + 1]; p++) { rj[cur[ci[p]]] = j; rx[cur[ci[p]]++] = cx[p]; }
        for (Int j = 0; j < dim; j++) cc[j] = cp[j + 1] - cp[j];
        for (Int i = 0; i < dim; i++) rc[i] = rp[i + 1] - rp[i];
    };
    rebuild_rows();
    std::vector<Int> rstage(dim, -1), cstage(dim, -1);
    std::vector<double> pivot(dim, 0.0);             // by column
    std::vector<char> ckind(dim, 0);                 // 1 column singleton, 2 row singleton, 3 bump, 4 dependent, 5 pivot of an elimination round
    Int npiv = 0, rounds = 0;
    std::vector<char> torn(dim, 0);                  // spike columns (set aside when the rounds stall)
    std::vector<Int> pivrow_of(dim, -1);             // pivot row of a pivoted column
    // (the limit decides whether a bump is torn; the spikes may fill the largest dense block the device's panel kernels take,
    // 32768 rows, unless a small limit -- tests -- binds them too)
    const Int spike_limit = bump_limit > 4096 ? std::max<Int>(bump_limit, 32768) : bump_limit;
    bool tearing = false, sparse_entered = false;
    Int ntorn = 0, tear_width = 1, npiv_at_tear = 0;
    while (true) {
        Int found = 0;
        // ---- column singletons
        {
            std::vector<Int> claim(dim, -1), piv_row(dim, -1);
            for (Int j = 0; j < dim; j++) {
                if (cstage[j] >= 0 || torn[j] || cc[j] != 1) continue;
                for (Int p = cp[j]; p < cp[j + 1]; p++) {
                    const Int i = ci[p];
                    if (rstage[i] >= 0) continue;
                    if (std::abs(cx[p]) >= abstol && claim[i] < 0) { claim[i] = j; piv_row[j] = i; pivot[j] = cx[p]; }
                    break;
                }
            }
            std::vector<Int> winners;
            for (Int j = 0; j < dim; j++) if (piv_row[j] >= 0) winners.push_back(j);
            for (Int j : winners) {
                const Int i = piv_row[j];
                rstage[i] = cstage[j] = npiv++;
                ckind[j] = 1;
                pivrow_of[j] = i;
            }
            for (Int j : winners) {
                const Int i = piv_row[j];
                for (Int q = rp[i]; q < rp[i + 1]; q++)
                    if (cstage[rj[q]] < 0) cc[rj[q]]--;
            }
            found += (Int)winners.size();
            F->info[0] += (Int)winners.size();
        }
        // ---- row singletons
        {
            std::vector<Int> best_row(dim, -1), piv_col(dim, -1);
            std::vector<double> best_abs(dim, 0.0);
            for (Int i = 0; i < dim; i++) {
                if (rstage[i] >= 0 || rc[i] != 1) continue;
                for (Int q = rp[i]; q < rp[i + 1]; q++) {
                    const Int j = rj[q];
                    if (cstage[j] >= 0 || torn[j]) continue;
                    const double a = std::abs(rx[q]);
                    double colmax = 0.0;
                    for (Int p = cp[j]; p < cp[j + 1]; p++)
                        if (rstage[ci[p]] < 0) colmax = std::max(colmax, std::abs(cx[p]));
                    if (a >= abstol && a >= pivottol * colmax && a > best_abs[j]) { best_abs[j] = a; best_row[j] = i; }
                    break;
                }
            }
            std::vector<Int> winners;                 // rows, ascending
            for (Int j = 0; j < dim; j++) if (best_row[j] >= 0) piv_col[best_row[j]] = j;
            for (Int i = 0; i < dim; i++) if (piv_col[i] >= 0) winners.push_back(i);
            for (Int i : winners) {
                const Int j = piv_col[i];
                rstage[i] = cstage[j] = npiv++;
                ckind[j] = 2;
                pivrow_of[j] = i;
                for (Int q = rp[i]; q < rp[i + 1]; q++) if (rj[q] == j) pivot[j] = rx[q];
            }
            for (Int i : winners) {
                const Int j = piv_col[i];
                for (Int p = cp[j]; p < cp[j + 1]; p++)
                    if (rstage[ci[p]] < 0) rc[ci[p]]--;
            }
            found += (Int)winners.size();
            F->info[1] += (Int)winners.size();
        }
        rounds++;
        if (found > 0) continue;
        // the rounds stall: done, or (a bump beyond the dense limit) tear spikes off and go on
        Int nact = 0;
        for (Int j = 0; j < dim; j++) nact += cstage[j] < 0 && !torn[j];
        if (nact == 0) break;
        if (sparse_rounds) {
            // ---- ELIMINATION ROUNDS on the stalled matrix (every active row and column has two entries or more).  From here on
            // the singleton rounds are not run any more: a singleton is a pivot of cost 0 of the next elimination round.
            const uint64_t kNone = ~uint64_t(0);
            std::vector<Int> candrow, winners;
            // the new current matrix: the entries whose row and column stay active, followed by the updates
            // -(a_i'j / pivot) * a_ij' in the order of the winners; equal positions are summed in that order, and an entry
            // that cancels exactly leaves the pattern (so do explicit zeros of B).  The other entries join the list E.
            auto rebuild = [&]() {
                std::vector<std::pair<uint64_t, double>> ent;
                for (Int j = 0; j < dim; j++)
                    for (Int p = cp[j]; p < cp[j + 1]; p++) {
                        const Int i = ci[p];
                        if (rstage[i] < 0 && cstage[j] < 0) ent.emplace_back(((uint64_t)j << 32) | (uint64_t)i, cx[p]);
                        else { Ei.push_back(i); Ej.push_back(j); Ex.push_back(cx[p]); }
                    }
                for (Int j : winners) {
                    const Int i = candrow[j];
                    for (Int p = cp[j]; p < cp[j + 1]; p++) {
                        const Int i2 = ci[p];
                        if (rstage[i2] >= 0) continue;                  // the pivot row itself (rows pivoted earlier are not in the matrix)
                        const double l = cx[p] / pivot[j];
                        for (Int q = rp[i]; q < rp[i + 1]; q++) {
                            const Int j2 = rj[q];
                            if (cstage[j2] >= 0) continue;
                            const double prod = l * rx[q];
                            ent.emplace_back(((uint64_t)j2 << 32) | (uint64_t)i2, -prod);
                        }
                    }
                }
                std::stable_sort(ent.begin(), ent.end(), [](const std::pair<uint64_t, double>& a, const std::pair<uint64_t, double>& b) { return a.first < b.first; });
                ci.clear(); cx.clear();
                std::fill(cp.begin(), cp.end(), 0);
                for (size_t e = 0; e < ent.size();) {
                    size_t f = e + 1;
                    double acc = ent[e].second;
                    while (f < ent.size() && ent[f].first == ent[e].first) acc = acc + ent[f++].second;
                    if (acc != 0.0) {
                        ci.push_back((Int)(ent[e].first & 0xffffffffu));
                        cx.push_back(acc);
                        cp[(ent[e].first >> 32) + 1]++;
                    }
                    e = f;
                }
                for (Int j = 0; j < dim; j++) cp[j + 1] += cp[j];
                rebuild_rows();
            };
            if (sparse_from < 0 || nact <= sparse_from) break;     // small enough: dense as it stands
            sparse_entered = true;
            rebuild();                                             // the active submatrix
            int slow = 0;
            while (nact > sparse_min) {
                // (the rounds stop early once the current matrix fits the dense code and two rounds in a row have each eliminated
                // fewer than 1 / slow_den of the columns: what is left has no large sets of independent pivots any more)
                if (slow_den > 0 && (bump_limit < 0 || nact <= bump_limit) && slow >= 2) break;
                // ... or once it fits the dense code and holds more than dense_at x nact^2 entries: a dense matrix in sparse storage
                if (dense_at > 0.0 && (bump_limit < 0 || nact <= bump_limit) && (double)cp[dim] > dense_at * (double)nact * (double)nact) break;
                // 1. one candidate per column: among its entries that pass the absolute and the relative threshold, the one in
                //    the shortest row (ties: larger |entry|, then smaller row); cost = (row count - 1)(column count - 1)
                candrow.assign(dim, -1);
                std::vector<uint64_t> key(dim, kNone), rowbest(dim, kNone);
                std::vector<int64_t> cost(dim, 0);
                int64_t mincost = INT64_MAX, hist[33] = {0}, ncand = 0;
                for (Int j = 0; j < dim; j++) {
                    if (cstage[j] >= 0) continue;
                    double colmax = 0.0;
                    for (Int p = cp[j]; p < cp[j + 1]; p++) colmax = std::max(colmax, std::abs(cx[p]));
                    Int bi = -1, brc = 0;
                    double ba = 0.0;
                    for (Int p = cp[j]; p < cp[j + 1]; p++) {
                        const Int i = ci[p];
                        const double a = std::abs(cx[p]);
                        if (!(a >= abstol && a >= pivottol * colmax)) continue;
                        if (bi < 0 || rc[i] < brc || (rc[i] == brc && (a > ba || (a == ba && i < bi)))) { bi = i; brc = rc[i]; ba = a; }
                    }
                    if (bi < 0) continue;
                    candrow[j] = bi;
                    cost[j] = std::min<int64_t>((int64_t)(brc - 1) * (cc[j] - 1), 0x7fffffff);
                    mincost = std::min(mincost, cost[j]);
                    int b = 0;
                    while (b < 32 && (int64_t(1) << b) <= cost[j]) b++;          // bucket b: cost < 2^b
                    hist[b]++;
                    ncand++;
                }
                if (ncand == 0) break;                              // no column has an acceptable pivot: what is left goes to the dense block
                // 2. the candidates that cost at most max(4, twice the cheapest) compete, and at least a quarter of all candidates
                //    (the smallest power of two that admits so many); a row keeps its best one (cost, then column index)
                int64_t limit = std::max<int64_t>(4, 2 * mincost);
                {
                    int64_t cum = 0;
                    for (int b = 0; b <= 32; b++) {
                        cum += hist[b];
                        if (cum * 4 >= ncand) { limit = std::max<int64_t>(limit, (int64_t(1) << b) - 1); break; }
                    }
                }
                for (Int j = 0; j < dim; j++)
                    if (candrow[j] >= 0 && cost[j] <= limit) {
                        key[j] = ((uint64_t)cost[j] << 32) | (uint64_t)j;
                        rowbest[candrow[j]] = std::min(rowbest[candrow[j]], key[j]);
                    }
                // 3. a contender (the best of its row) wins unless a better contender has an entry in its pivot row or its pivot row
                //    in this column: the winners' pivots form a diagonal block, so they can be eliminated together
                auto contender = [&](Int j) { return key[j] != kNone && rowbest[candrow[j]] == key[j]; };
                winners.clear();
                for (Int j = 0; j < dim; j++) {
                    if (!contender(j)) continue;
                    const Int i = candrow[j];
                    bool win = true;
                    for (Int q = rp[i]; q < rp[i + 1] && win; q++) {
                        const Int j2 = rj[q];
                        if (j2 != j && contender(j2) && key[j2] < key[j]) win = false;
                    }
                    for (Int p = cp[j]; p < cp[j + 1] && win; p++)
                        if (ci[p] != i && rowbest[ci[p]] < key[j]) win = false;
                    if (win) winners.push_back(j);
                }
                // 4. pivots in ascending order of the column
                for (Int j : winners) {
                    const Int i = candrow[j];
                    rstage[i] = cstage[j] = npiv++;
                    ckind[j] = 5;
                    pivrow_of[j] = i;
                    for (Int p = cp[j]; p < cp[j + 1]; p++) if (ci[p] == i) pivot[j] = cx[p];
                }
                F->info[6] += (Int)winners.size();
                F->info[7] += 1;
                rounds++;
                if (getenv("ORC_LU_DEBUG"))
                    fprintf(stderr, "elim round %lld: active %lld nnz %lld mincost %lld limit %lld candidates %lld winners %zu\n", (long long)F->info[7],
                            (long long)nact, (long long)cp[dim], (long long)mincost, (long long)limit, (long long)ncand, winners.size());
                rebuild();
                slow = (int64_t)winners.size() * slow_den < (int64_t)nact ? slow + 1 : 0;
                nact -= (Int)winners.size();
                const int64_t fill_bound = std::max<int64_t>((int64_t)fill_max * nnz_B + (1 << 20),
                                                             fill_to_dense ? (int64_t)(dense_at * (double)bump_limit * (double)bump_limit) : 0);
                if (fill_max > 0 && (int64_t)cp[dim] > fill_bound) {   // bounded work: given up
                    if (fill_to_dense && (bump_limit < 0 || nact <= bump_limit)) break;             // (round 5: the dense code takes what is left if it can)
                    return nullptr;
                }
            }
            break;
        }
        if (!tearing) {
            if (bump_limit < 0 || nact <= bump_limit) break;       // small enough: dense as it stands
            tearing = true;
        } else {
            tear_width = npiv - npiv_at_tear < 64 ? std::min<Int>(2 * tear_width, 1024) : 1;
        }
        std::vector<std::pair<Int, Int>> cand;                     // (-active entries, index)
        for (Int j = 0; j < dim; j++) if (cstage[j] < 0 && !torn[j]) cand.emplace_back(-cc[j], j);
        const size_t take = std::min<size_t>((size_t)tear_width, cand.size());
        std::partial_sort(cand.begin(), cand.begin() + take, cand.end());
        for (size_t t = 0; t < take; t++) {
            const Int j = cand[t].second;
            torn[j] = 1;
            for (Int p = cp[j]; p < cp[j + 1]; p++)
                if (rstage[ci[p]] < 0) rc[ci[p]]--;
        }
        ntorn += (Int)take;
        npiv_at_tear = npiv;
        if (ntorn > spike_limit) { F->info[2] = ntorn; return nullptr; }
    }
    F->info[3] = rounds;
    F->info[5] = ntorn;
    // ---- bump: dense, partial pivoting
    std::vector<Int> brow, bcol, rloc(dim, -1), cloc(dim, -1);
    for (Int i = 0; i < dim; i++) if (rstage[i] < 0) { rloc[i] = (Int)brow.size(); brow.push_back(i); }
    for (Int j = 0; j < dim; j++) if (cstage[j] < 0) { cloc[j] = (Int)bcol.size(); bcol.push_back(j); }
    if (sparse_entered && !getenv("ORC_NO_COLORDER")) {
        // the dense block's columns in ascending order of their number of entries (ties: index): fewer nonzeros in its factors
        std::stable_sort(bcol.begin(), bcol.end(), [&](Int a, Int b) { return cc[a] < cc[b]; });
        for (size_t c = 0; c < bcol.size(); c++) cloc[bcol[c]] = (Int)c;
    }
    const Int kb = (Int)bcol.size();
    F->info[2] = kb;
    if (bump_limit >= 0 && kb > (tearing ? spike_limit : bump_limit)) return nullptr;
    std::vector<double> D((size_t)kb * kb, 0.0);      // column-major
    std::vector<std::vector<std::pair<Int, double>>> spikeU;       // torn: entries of a spike in pivoted rows (stage, value)
    if (!tearing) {
        for (Int c = 0; c < kb; c++)
            for (Int p = cp[bcol[c]]; p < cp[bcol[c] + 1]; p++)
                if (rloc[ci[p]] >= 0) D[(size_t)c * kb + rloc[ci[p]]] = cx[p];
    } else {
        // the spikes through the row singleton pivots in pivot order: x[r] -= l_rj * x[i] for every row r that was
        // still active when (i, j) was pivoted (products rounded before they are subtracted)
        std::vector<Int> lpiv;                                     // row singleton columns by stage
        {
            std::vector<std::pair<Int, Int>> o;
            for (Int j = 0; j < dim; j++) if (ckind[j] == 2) o.emplace_back(cstage[j], j);
            std::sort(o.begin(), o.end());
            for (auto& e : o) lpiv.push_back(e.second);
        }
        spikeU.resize(kb);
        std::vector<double> x(dim, 0.0);
        for (Int c = 0; c < kb; c++) {
            const Int js = bcol[c];
            for (Int p = cp[js]; p < cp[js + 1]; p++) x[ci[p]] = cx[p];
            for (Int j : lpiv) {
                const Int i = pivrow_of[j], k = cstage[j];
                const double xi = x[i];
                if (xi == 0.0) continue;
                for (Int p = cp[j]; p < cp[j + 1]; p++) {
                    const Int r = ci[p];
                    if (r == i || (rstage[r] >= 0 && rstage[r] < k)) continue;
                    const double l = cx[p] / pivot[j];
                    x[r] -= l * xi;
                }
            }
            for (Int r = 0; r < dim; r++) {
                if (x[r] != 0.0) {
                    if (rstage[r] >= 0) spikeU[c].emplace_back(rstage[r], x[r]);
                    else D[(size_t)c * kb + rloc[r]] = x[r];
                }
                x[r] = 0.0;
            }
        }
    }
    std::vector<Int> brstep(kb, -1), bcstep(kb, -1);   // bump-local pivot step of a row / column
    Int bstep = 0;
    for (Int c = 0; c < kb; c++) {
        double* col = &D[(size_t)c * kb];
        Int pr = -1;
        double best = 0.0;
        for (Int r = 0; r < kb; r++)
            if (brstep[r] < 0 && std::abs(col[r]) > best) { best = std::abs(col[r]); pr = r; }
        if (pr < 0 || best < abstol) continue;         // dependent
        brstep[pr] = bcstep[c] = bstep++;
        const double piv = col[pr];
        for (Int r = 0; r < kb; r++)
            if (brstep[r] < 0) col[r] /= piv;           // multipliers stay in place
        for (Int c2 = c + 1; c2 < kb; c2++) {
            double* col2 = &D[(size_t)c2 * kb];
            const double u = col2[pr];
            if (u == 0.0) continue;
            for (Int r = 0; r < kb; r++)
                if (brstep[r] < 0) col2[r] -= col[r] * u;
        }
    }
    // stages of the bump pivots, then the dependent columns with the left-over rows
    for (Int c = 0; c < kb; c++)
        if (bcstep[c] >= 0) { cstage[bcol[c]] = npiv + bcstep[c]; ckind[bcol[c]] = 3; }
    for (Int r = 0; r < kb; r++)
        if (brstep[r] >= 0) rstage[brow[r]] = npiv + brstep[r];
    npiv += bstep;
    {
        std::vector<Int> lrows;
        for (Int r = 0; r < kb; r++) if (brstep[r] < 0) lrows.push_back(r);
        size_t t = 0;
        for (Int c = 0; c < kb; c++)
            if (bcstep[c] < 0) {
                cstage[bcol[c]] = npiv; ckind[bcol[c]] = 4;
                rstage[brow[lrows[t++]]] = npiv;
                F->dependent.push_back(npiv++);
            }
    }
    F->info[4] = (Int)F->dependent.size();
    F->rowperm.assign(dim, 0); F->colperm.assign(dim, 0);
    for (Int i = 0; i < dim; i++) F->rowperm[rstage[i]] = i;
    for (Int j = 0; j < dim; j++) F->colperm[cstage[j]] = j;
    // ---- assemble: column k of L and U, indices ascending.  With elimination rounds the entries come from the list of the
    // entries that left the current matrix (plus what is in it now); without, that list is B itself.
    if (sparse_entered) {
        for (Int j = 0; j < dim; j++)
            for (Int p = cp[j]; p < cp[j + 1]; p++) { Ei.push_back(ci[p]); Ej.push_back(j); Ex.push_back(cx[p]); }
        std::vector<Int> ep(dim + 1, 0);
        for (Int j : Ej) ep[j + 1]++;
        for (Int j = 0; j < dim; j++) ep[j + 1] += ep[j];
        std::vector<Int> cur(ep.begin(), ep.end() - 1), ei(Ei.size());
        std::vector<double> ex(Ei.size());
        for (size_t e = 0; e < Ei.size(); e++) { ei[cur[Ej[e]]] = Ei[e]; ex[cur[Ej[e]]++] = Ex[e]; }
        cp.swap(ep); ci.swap(ei); cx.swap(ex);
    }
    F->Lp.assign(1, 0); F->Up.assign(1, 0);
    std::vector<std::pair<Int, double>> lcol, ucol;
    for (Int k = 0; k < dim; k++) {
        const Int j = F->colperm[k];
        lcol.clear(); ucol.clear();
        if (ckind[j] == 4) {
            ucol.emplace_back(k, 1.0);
        } else {
            const Int c = cloc[j];
            if (c >= 0 && tearing) {
                for (auto& e : spikeU[c]) ucol.push_back(e);          // a spike above the dense block: its updated values
            } else {
                for (Int p = cp[j]; p < cp[j + 1]; p++) {
                    const Int i = ci[p];
                    if (c >= 0 && rloc[i] >= 0) continue;             // bump x bump: from the dense result
                    const Int s = rstage[i];
                    if (s < k) ucol.emplace_back(s, cx[p]);
                    else if (s > k) lcol.emplace_back(s, cx[p] / pivot[j]);
                }
            }
            if (c >= 0) {
                const double* col = &D[(size_t)c * kb];
                for (Int r = 0; r < kb; r++) {
                    const Int s = rstage[brow[r]];
                    if (s == k) { pivot[j] = col[r]; continue; }
                    if (col[r] == 0.0) continue;
                    if (s < k) ucol.emplace_back(s, col[r]); else lcol.emplace_back(s, col[r]);
                }
            }
            std::sort(ucol.begin(), ucol.end());
            std::sort(lcol.begin(), lcol.end());
            ucol.emplace_back(k, pivot[j]);
        }
        for (auto& e : lcol) { F->Li.push_back(e.first); F->Lx.push_back(e.second); }
        for (auto& e : ucol) { F->Ui.push_back(e.first); F->Ux.push_back(e.second); }
        F->Lp.push_back((Int)F->Li.size());
        F->Up.push_back((Int)F->Ui.size());
    }
    return F.release();
}

extern "C" orc_lu* orc_lu_factorize(Int dim, const Int* Bbegin, const Int* Bend, const Int* Bi, const double* Bx,
                                    double pivottol, int strict_abs_pivottol, Int bump_limit) {
    return lu_factorize_impl(dim, Bbegin, Bend, Bi, Bx, pivottol, strict_abs_pivottol, bump_limit, 0, 0, 0, 0);
}
// ... with ELIMINATION ROUNDS instead of tearing: when the singleton rounds stall with more than bump_limit active columns, sets
// of pivots with low Markowitz cost that form a diagonal block are eliminated at once (the fill-in enters the current matrix)
// until at most sparse_min columns are active, or at most bump_limit and two rounds in a row have each eliminated fewer than
// 1 / slow_den of the columns (slow_den 0: never); given up (NULL) when the current matrix exceeds fill_max x nnz(B) + 2^20 entries
// (0: never); what is left (at most bump_limit rows, else refused) is factorized densely, its columns in ascending
// order of their number of entries.
extern "C" orc_lu* orc_lu_factorize_sparse(Int dim, const Int* Bbegin, const Int* Bend, const Int* Bi, const double* Bx,
                                           double pivottol, int strict_abs_pivottol, Int bump_limit, Int sparse_min, Int slow_den, Int fill_max) {
    return lu_factorize_impl(dim, Bbegin, Bend, Bi, Bx, pivottol, strict_abs_pivottol, bump_limit, 1, sparse_min, slow_den, fill_max);
}

// ... with the policy of round 5 (ipx_amd/csrc/lu.hip, default): elimination rounds for every bump of more than sparse_from rows; they
// end at sparse_min columns, or -- once at most rest_limit columns are left, what the dense code takes -- after two slow rounds (as above),
// or when the current matrix holds more than dense_at x (columns left)^2 entries, or when it exceeds fill_max x nnz(B) + 2^20 entries;
// NULL only if more than rest_limit columns are left at that point.
extern "C" orc_lu* orc_lu_factorize_policy(Int dim, const Int* Bbegin, const Int* Bend, const Int* Bi, const double* Bx,
                                           double pivottol, int strict_abs_pivottol, Int sparse_from, Int rest_limit, Int sparse_min,
                                           Int slow_den, Int fill_max, double dense_at) {
    return lu_factorize_impl(dim, Bbegin, Bend, Bi, Bx, pivottol, strict_abs_pivottol, rest_limit, 1, sparse_min, slow_den, fill_max,
                             sparse_from, dense_at, 1);
}

extern "C" void orc_lu_sizes(const orc_lu* F, Int* lnz, Int* unz, Int* ndep, Int* info) {
    *lnz = (Int)F->Li.size(); *unz = (Int)F->Ui.size(); *ndep = (Int)F->dependent.size();
    if (info) std::copy(F->info, F->info + 8, info);
}
extern "C" void orc_lu_get(const orc_lu* F, Int* Lp, Int* Li, double* Lx, Int* Up, Int* Ui, double* Ux,
                           Int* rowperm, Int* colperm, Int* dependent) {
    std::copy(F->Lp.begin(), F->Lp.end(), Lp); std::copy(F->Li.begin(), F->Li.end(), Li);
    std::copy(F->Lx.begin(), F->Lx.end(), Lx); std::copy(F->Up.begin(), F->Up.end(), Up);
    std::copy(F->Ui.begin(), F->Ui.end(), Ui); std::copy(F->Ux.begin(), F->Ux.end(), Ux);
    std::copy(F->rowperm.begin(), F->rowperm.end(), rowperm);
    std::copy(F->colperm.begin(), F->colperm.end(), colperm);
    std::copy(F->dependent.begin(), F->dependent.end(), dependent);
}
extern "C" void orc_lu_free(orc_lu* F) { delete F; }

// ---------------------------------------------------------------------------
// Maxvolume: Maxvolume::RunHeuristic / Driver / ScaleFtran / FindLargest
// (src/maxvolume.cc:108-153, 179-320, 322-337) and the part of ipx::Basis it drives: SolveDense,
// SolveForUpdate, TableauRow (dense branch), ExchangeIfStable (src/basis.cc:162-330; status encoding
// src/basis.h:317-340).
// The reference keeps its factorization current with BASICLU's or ForrestTomlin's update (src/lu_update.h).
// Here -- as on the device -- the factorization of the LAST refactorized basis B0 stays fixed and every
// exchange appends a product-form eta:  B = B0 E_1 ... E_k,  E_t = I + (eta_t - e_p) e_p'  with eta_t the
// FTRAN of the entering column.  Any exact update represents the same matrix, so tableau columns / rows and
// hence the heuristic's decisions are those of the reference up to rounding (tests pin FTRAN / BTRAN after
// exchanges against the reference's own ForrestTomlin, oracle/ref_driver.cc).  Stability test of an exchange:
// the pivot from the tableau row (BTRAN) against the one from the tableau column (FTRAN), relative 1e-8
// (the role of kFtDiagErrorTol, src/ipx_internal.h:37); on failure, and after max_etas exchanges, the basis is
// refactorized (Basis::ExchangeIfStable :299-306, :318-319).
// Maxvolume needs a live ipx::Basis (BASICLU): pinned through the device code, which takes the same exchanges as this
// restatement (tests/test_gpu_maxvolume.py) and ends in the same basis as the reference's own ipx::Maxvolume
// (tests/dropin/maxvol_main.cc).
// ---------------------------------------------------------------------------
struct orc_basis {
    Int m = 0, n = 0;
    const Int *Ap = nullptr, *Ai = nullptr;
    const double* Ax = nullptr;
    std::vector<Int> basis, map2basis;      // map2basis: position, position + m (BASIC_FREE), -1 NONBASIC, -2 NONBASIC_FIXED
    std::unique_ptr<orc_lu> F;
    std::vector<Int> eta_pos;
    std::vector<double> eta_piv;
    std::vector<std::vector<std::pair<Int, double>>> eta;
    Vec last_ftran;                          // unscaled tableau column of the last SolveForUpdate(nonbasic)
    Int last_ftran_var = -1;
    Int max_etas = 100, num_factorizations = 0, num_updates = 0, num_ftran = 0, num_btran = 0;
    double pivottol = 0.1;

    Int position_of(Int j) const { const Int p = map2basis[j]; return p < 0 ? -1 : p < m ? p : p - m; }
    int status_of(Int j) const { const Int p = map2basis[j]; return p < 0 ? (p == -1 ? ORC_NONBASIC : ORC_NONBASIC_FIXED) : (p < m ? ORC_BASIC : ORC_BASIC_FREE); }

    Int factorize() {      // Basis::Factorize, src/basis.cc:116-156 (no tightening of the pivot tolerance here)
        std::vector<Int> begin(m), end(m), slack_i;
        std::vector<double> slack_x;
        // AI's arrays with the slack columns appended, as Model::AI() holds them
        std::vector<Int> bi(Ai, Ai + Ap[n]);
        std::vector<double> bx(Ax, Ax + Ap[n]);
        for (Int i = 0; i < m; i++) { bi.push_back(i); bx.push_back(1.0); }
        for (Int p = 0; p < m; p++) {
            const Int j = basis[p];
            begin[p] = j < n ? Ap[j] : Ap[n] + (j - n);
            end[p] = j < n ? Ap[j + 1] : Ap[n] + (j - n) + 1;
        }
        F.reset(orc_lu_factorize(m, begin.data(), end.data(), bi.data(), bx.data(), pivottol, 0, -1));
        eta_pos.clear(); eta_piv.clear(); eta.clear();
        num_factorizations++;
        return F->dependent.empty() ? 0 : 301;       // IPX_ERROR_basis_singular
    }
    // Basis::SolveDense (:168-170) = ForrestTomlin::_SolveDense (src/forrest_tomlin.cc:67-78) on B0, then the etas
    void solve_dense(const double* rhs, double* lhs, char trans) const {
        Vec work(m);
        if (trans == 't' || trans == 'T') {
            Vec v(rhs, rhs + m);                     // position space
            for (Int t = (Int)eta.size() - 1; t >= 0; t--) {
                double sum = 0.0;
                for (const auto& e : eta[t]) sum += e.second * v[e.first];
                v[eta_pos[t]] = (v[eta_pos[t]] - sum) / eta_piv[t];
            }
            for (Int i = 0; i < m; i++) work[i] = v[F->colperm[i]];
            orc_backward_solve(m, F->Lp.data(), F->Li.data(), F->Lx.data(), F->Up.data(), F->Ui.data(), F->Ux.data(), work.data());
            for (Int i = 0; i < m; i++) lhs[F->rowperm[i]] = work[i];
        } else {
            for (Int i = 0; i < m; i++) work[i] = rhs[F->rowperm[i]];
            orc_forward_solve(m, F->Lp.data(), F->Li.data(), F->Lx.data(), F->Up.data(), F->Ui.data(), F->Ux.data(), work.data());
            for (Int i = 0; i < m; i++) lhs[F->colperm[i]] = work[i];
            for (size_t t = 0; t < eta.size(); t++) {
                const double vp = lhs[eta_pos[t]] / eta_piv[t];
                for (const auto& e : eta[t]) lhs[e.first] -= e.second * vp;
                lhs[eta_pos[t]] = vp;
            }
        }
    }
    // Basis::SolveForUpdate (:172-196): tableau column of a nonbasic variable / row of inverse(B) of a basic one
    void solve_for_update(Int j, double* lhs) {
        const Int p = position_of(j);
        Vec rhs(m, 0.0);
        if (p < 0) {
            if (j < n) for (Int q = Ap[j]; q < Ap[j + 1]; q++) rhs[Ai[q]] = Ax[q];
            else rhs[j - n] = 1.0;
            solve_dense(rhs.data(), lhs, 'N');
            last_ftran.assign(lhs, lhs + m);
            last_ftran_var = j;
            num_ftran++;
        } else {
            rhs[p] = 1.0;
            solve_dense(rhs.data(), lhs, 'T');
            num_btran++;
        }
    }
    // Basis::TableauRow (:221-284), dense branch (the sparse branch computes the same numbers in another order)
    void tableau_row(Int jb, double* btran, double* row, bool ignore_fixed) {
        solve_for_update(jb, btran);
        for (Int j = 0; j < n + m; j++) {
            double result = 0.0;
            if (map2basis[j] == -1 || (map2basis[j] == -2 && !ignore_fixed)) {
                if (j < n) for (Int q = Ap[j]; q < Ap[j + 1]; q++) result += Ax[q] * btran[Ai[q]];
                else result += 1.0 * btran[j - n];
            }
            row[j] = result;
        }
    }
    // Basis::ExchangeIfStable (:286-321) with sys = 0
    Int exchange_if_stable(Int jb, Int jn, double tableau_entry, bool* exchanged) {
        *exchanged = false;
        const Int ib = position_of(jb);
        const double piv_ftran = last_ftran[ib];
        const bool unstable = last_ftran_var != jn ||
                              !(std::abs(piv_ftran - tableau_entry) <= 1e-8 * std::abs(piv_ftran)) || piv_ftran == 0.0;
        if (unstable) {
            if (eta.empty()) return 306;             // IPX_ERROR_basis_too_ill_conditioned: nothing to refresh
            return factorize();                      // refactorizes the OLD basis; the caller tries again
        }
        std::vector<std::pair<Int, double>> e;
        for (Int p = 0; p < m; p++) if (p != ib && last_ftran[p] != 0.0) e.emplace_back(p, last_ftran[p]);
        eta.push_back(std::move(e));
        eta_pos.push_back(ib);
        eta_piv.push_back(piv_ftran);
        basis[ib] = jn;
        map2basis[jn] = ib;
        map2basis[jb] = -1;
        num_updates++;
        last_ftran_var = -1;
        *exchanged = true;
        if ((Int)eta.size() >= max_etas) return factorize();
        return 0;
    }
};

extern "C" orc_basis* orc_basis_new(Int m, Int n, const Int* Ap, const Int* Ai, const double* Ax, const Int* basis,
                                    const Int* status, Int max_etas, Int* errflag) {
    std::unique_ptr<orc_basis> B(new orc_basis);
    B->m = m; B->n = n; B->Ap = Ap; B->Ai = Ai; B->Ax = Ax;
    B->basis.assign(basis, basis + m);
    B->map2basis.assign(n + m, -1);
    for (Int j = 0; j < n + m; j++) if (status[j] == ORC_NONBASIC_FIXED) B->map2basis[j] = -2;
    for (Int p = 0; p < m; p++) B->map2basis[basis[p]] = status[basis[p]] == ORC_BASIC_FREE ? p + m : p;
    if (max_etas > 0) B->max_etas = max_etas;
    *errflag = B->factorize();
    return B.release();
}
extern "C" void orc_basis_free(orc_basis* B) { delete B; }
extern "C" void orc_basis_get(const orc_basis* B, Int* basis, Int* status, Int* counts) {
    std::copy(B->basis.begin(), B->basis.end(), basis);
    for (Int j = 0; j < B->n + B->m; j++) status[j] = B->status_of(j);
    if (counts) {
        counts[0] = B->num_factorizations; counts[1] = B->num_updates; counts[2] = B->num_ftran;
        counts[3] = B->num_btran; counts[4] = (Int)B->eta.size();
    }
}
extern "C" void orc_basis_solve_dense(const orc_basis* B, const double* rhs, double* lhs, char trans) {
    Vec tmp(rhs, rhs + B->m);
    B->solve_dense(tmp.data(), lhs, trans);
}
extern "C" void orc_basis_solve_for_update(orc_basis* B, Int j, double* lhs) { B->solve_for_update(j, lhs); }
extern "C" void orc_basis_tableau_row(orc_basis* B, Int jb, double* btran, double* row, int ignore_fixed) {
    B->tableau_row(jb, btran, row, ignore_fixed != 0);
}
extern "C" Int orc_basis_exchange_if_stable(orc_basis* B, Int jb, Int jn, double tableau_entry, Int* exchanged) {
    bool ex = false;
    const Int err = B->exchange_if_stable(jb, jn, tableau_entry, &ex);
    *exchanged = ex ? 1 : 0;
    return err;
}

// Maxvolume::RunHeuristic (src/maxvolume.cc:108-153) with Driver (:202-320).  colscale: n+m scaling factors
// (KKTSolverBasis::_Factorize passes Iterate::ScalingFactor, src/kkt_solver_basis.cc:28-29,46-50).
// info[8] = updates, skipped, slices, volinc, # exchanges that were refused as unstable, errflag, 0, 0.
// log (may be NULL, capacity log_cap pairs): the accepted exchanges (jb, jn) in order.
// Maxvolume::RunSequential (src/maxvolume.cc:14-106), selected by update_heuristic == 0 (src/kkt_solver_basis.cc:47-51):
// passes over the columns in decreasing order of their scaling factor; for every NONBASIC candidate the tableau column
// (SolveForUpdate), the largest scaled entry v = |x_p| * invscale_basic[p] * d_j (first position on ties);
// an exchange if v > max(volume_tol, 1).
// CAVEAT on ties, here and in ScaleFtran of the heuristic below: the reference visits a SPARSE tableau column in the pattern
// order of its IndexedVector (for_each_nonzero), an LU detail, so at an exact tie the reference itself may pick another
// position than the first.  Ties are not measure zero on real LPs (+-1 coefficients, equal scaling factors, duplicated
// columns).  The contract that is pinned is device = this restatement, which takes the FIRST strictly larger entry in
// position order (tests/test_gpu_basis_ties.py on exact dyadic data); FindLargest's loop over the columns is in index order
// in the reference too.  ExchangeIfStable is called with sys = -1 (src/maxvolume.cc:83): the
// reference computes the BTRAN of the leaving variable for its LU update there; here the same BTRAN yields the pivot
// from the row, compared with the pivot from the column (exchange_if_stable above).
// info[8] = updates, skipped, passes, volinc, refused, errflag, tblnnz of the last pass, tblmax of the last pass.
extern "C" Int orc_maxvolume_sequential(orc_basis* B, const double* colscale, double volume_tol, Int maxpasses, double* info,
                                        Int* log, Int log_cap) {
    const Int m = B->m, n = B->n;
    Vec invscale_basic(m, 0.0), ftran(m), btran(m), row(n + m);
    for (Int p = 0; p < m; p++)
        if (B->status_of(B->basis[p]) == ORC_BASIC) invscale_basic[p] = colscale ? 1.0 / colscale[B->basis[p]] : 1.0;
    const double volumetol = std::max(volume_tol, 1.0);
    Int updates = 0, skipped = 0, passes = 0, refused = 0, errflag = 0, tblnnz = 0;
    double volinc = 0.0, tblmax = 0.0;
    while (passes < maxpasses || maxpasses < 0) {
        tblnnz = 0; tblmax = 0.0;
        Int updates_last = 0;
        std::vector<std::pair<double, Int>> cand(n + m);            // Sortperm(n+m, colscale, false), src/utils.cc:87-104
        for (Int j = 0; j < n + m; j++) cand[j] = std::make_pair(colscale ? colscale[j] : 1.0, j);
        std::sort(cand.begin(), cand.end());
        while (!cand.empty()) {
            const Int j = cand.back().second;
            const double dj = cand.back().first;
            if (dj == 0.0) break;
            if (B->status_of(j) != ORC_NONBASIC) { cand.pop_back(); continue; }
            B->solve_for_update(j, ftran.data());
            Int pmax = -1;
            double vmax = 0.0;
            for (Int p = 0; p < m; p++) {
                const double v = std::abs(ftran[p]) * invscale_basic[p] * dj;
                if (v > vmax) { vmax = v; pmax = p; }
                tblnnz += v != 0.0;
            }
            tblmax = std::max(tblmax, vmax);
            if (vmax <= volumetol) { skipped++; cand.pop_back(); continue; }
            const Int jb = B->basis[pmax];
            B->tableau_row(jb, btran.data(), row.data(), false);     // (the BTRAN of the leaving variable; row[j] = pivot from the row)
            bool exchanged = false;
            errflag = B->exchange_if_stable(jb, j, row[j], &exchanged);
            if (errflag) break;
            if (!exchanged) { refused++; continue; }                 // refactorized: try the same candidate again
            if (log && updates + updates_last < log_cap) { log[2 * (updates + updates_last)] = jb; log[2 * (updates + updates_last) + 1] = j; }
            invscale_basic[pmax] = 1.0 / dj;
            updates_last++;
            volinc += std::log2(vmax);
            cand.pop_back();
        }
        updates += updates_last;
        passes++;
        if (updates_last == 0 || errflag != 0) break;
    }
    info[0] = (double)updates; info[1] = (double)skipped; info[2] = (double)passes; info[3] = volinc;
    info[4] = (double)refused; info[5] = (double)errflag; info[6] = (double)tblnnz; info[7] = tblmax;
    return errflag;
}

extern "C" Int orc_maxvolume_heuristic(orc_basis* B, const double* colscale_in, double volume_tol, Int maxskip_updates,
                                       Int rows_per_slice, double* info, Int* log, Int log_cap) {
    const Int m = B->m, n = B->n;
    constexpr double kPivotZeroTol = 1e-7;            // src/maxvolume.h:34
    Vec colscale(n + m, 0.0), invscale_basic(m, 0.0), colweights(n + m, 0.0), work(m), lhs(m), row(n + m);
    std::vector<char> used(m, 0);
    Int updates = 0, skipped_total = 0, refused = 0, errflag = 0;
    double volinc = 0.0;
    Int num_slices = 5 + std::max<Int>(m / rows_per_slice, 0);     // :116-117
    num_slices = std::min(num_slices, m);
    for (Int p = 0; p < m; p++)                                     // :120-126
        if (B->status_of(B->basis[p]) == ORC_BASIC) invscale_basic[p] = colscale_in ? 1.0 / colscale_in[B->basis[p]] : 1.0;
    for (Int j = 0; j < n + m; j++)                                 // :130-133
        if (B->status_of(j) == ORC_NONBASIC) colscale[j] = colscale_in ? colscale_in[j] : 1.0;
    std::vector<std::pair<double, Int>> vi(m);                      // Sortperm, src/utils.cc:87-104
    for (Int i = 0; i < m; i++) vi[i] = std::make_pair(invscale_basic[i], i);
    std::sort(vi.begin(), vi.end());
    const double volumetol = std::max(volume_tol, 1.0);
    for (Int s = 0; s < num_slices && !errflag; s++) {
        for (Int i = 0; i < m; i++) used[vi[i].second] = i % num_slices == s;
        // ---- Driver
        for (Int p = 0; p < m; p++) work[p] = used[p] ? invscale_basic[p] : 0.0;     // :221-223
        {
            Vec tmp(work);
            B->solve_dense(tmp.data(), work.data(), 'T');
        }
        for (Int j = 0; j < n + m; j++) {                            // :224-232
            if (colscale[j] != 0.0) {
                double sum = 0.0;
                if (j < n) for (Int q = B->Ap[j]; q < B->Ap[j + 1]; q++) sum += B->Ax[q] * work[B->Ai[q]];
                else sum = work[j - n];                              // DotColumn over the unit column: 1.0 * work[i]
                colweights[j] = sum * colscale[j];
            } else colweights[j] = 0.0;
        }
        Int skipped = 0;
        while (true) {
            Int jn = 0;                                              // FindLargest (:179-200): first largest |w|
            double wmax = 0.0;
            for (Int j = 0; j < n + m; j++) if (std::abs(colweights[j]) > wmax) { wmax = std::abs(colweights[j]); jn = j; }
            const double weight = colweights[jn];
            if (weight == 0.0) break;
            B->solve_for_update(jn, lhs.data());                     // :253
            double vmax = 0.0;                                       // ScaleFtran :322-337
            Int pmax = 0;
            for (Int p = 0; p < m; p++) {
                const double pivot = lhs[p];
                const double scaled = pivot * colscale[jn] * invscale_basic[p];
                const double v = std::abs(scaled);
                if (v > vmax && std::abs(pivot) > kPivotZeroTol) { vmax = v; pmax = p; }
                lhs[p] = scaled;
            }
            vmax = std::abs(lhs[pmax]);                              // :255-256 (pmax = 0 if no entry qualified)
            if (vmax <= volumetol) {                                 // :259-266
                colweights[jn] = 0.0;
                colscale[jn] = 0.0;
                if (++skipped > maxskip_updates && maxskip_updates >= 0) break;
                continue;
            }
            double weight_recomp = 0.0;                              // :269-275
            for (Int p = 0; p < m; p++) if (used[p]) weight_recomp += lhs[p];
            const Int jb = B->basis[pmax];
            B->tableau_row(jb, lhs.data(), row.data(), true);        // :279 (lhs is overwritten by the BTRAN)
            const double pivot = row[jn];
            bool exchanged = false;
            errflag = B->exchange_if_stable(jb, jn, pivot, &exchanged);   // :287
            if (errflag) break;
            if (!exchanged) { refused++; continue; }
            if (log && updates < log_cap) { log[2 * updates] = jb; log[2 * updates + 1] = jn; }
            updates++;
            volinc += std::log2(vmax);
            const double dn = colscale[jn], dbinv = invscale_basic[pmax];       // :296-304
            colscale[jb] = 1.0 / invscale_basic[pmax];
            invscale_basic[pmax] = 1.0 / colscale[jn];
            colscale[jn] = 0.0;
            const double alpha = ((used[pmax] ? 1.0 : 0.0) - weight_recomp) / (dn * pivot);   // :307-314
            for (Int j = 0; j < n + m; j++) colweights[j] += alpha * row[j] * colscale[j];
            colweights[jb] = (used[pmax] ? 1.0 : 0.0) + alpha / dbinv;
            colweights[jn] = 0.0;
        }
        skipped_total += skipped;
    }
    info[0] = (double)updates; info[1] = (double)skipped_total; info[2] = (double)num_slices; info[3] = volinc;
    info[4] = (double)refused; info[5] = (double)errflag; info[6] = info[7] = 0.0;
    return errflag;
}
