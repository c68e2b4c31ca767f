"""A plain preconditioned Conjugate Residuals in numpy longdouble: the loop of reference
src/conjugate_residuals.cc:117-207 with C = A diag(W[:n]) A' + diag(W[n:]) (src/normal_matrix.cc) and the diagonal
preconditioner P = 1/diag(C) (src/diagonal_precond.cc:28-37, :151-154; no dense columns).  Nothing here is shared
with the product or the oracle: the matrix is used as COO triplets through np.add.at.  With the 64-bit mantissa
and the 15-bit exponent of x86 extended precision it serves as the high-precision reference of the PcrDiag tests
and, because it does not overflow where binary64 does, shows how far the overflow fixtures of
tests/test_gpu_cr_exits.py are from the edge of binary64.  C and P take weight vectors of their own."""
import collections

import numpy as np

LD = np.longdouble
PcrRun = collections.namedtuple("PcrRun", "lhs iter errflag hist cdot pdot rps")


class NormalOp:
    """v -> A diag(W[:n]) A' v + W[n:] v for a CSC matrix A (attributes nrow, ncol, p, i, x)"""

    def __init__(self, A, W):
        self.m, self.n = int(A.nrow), int(A.ncol)
        p = np.asarray(A.p, dtype=np.int64)
        self.rows = np.asarray(A.i, dtype=np.int64)
        self.cols = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(p))
        self.vals = np.asarray(A.x, dtype=LD)
        self.W = np.asarray(W, dtype=LD)
        assert self.W.shape == (self.n + self.m,)

    def apply(self, v):
        t = np.zeros(self.n, dtype=LD)
        np.add.at(t, self.cols, self.vals * v[self.rows])           # A' v
        t *= self.W[:self.n]
        out = self.W[self.n:] * v
        np.add.at(out, self.rows, self.vals * t[self.cols])         # A (W A' v)
        return out

    def diagonal(self):
        d = self.W[self.n:].copy()
        np.add.at(d, self.rows, self.vals * self.W[self.cols] * self.vals)
        return d


def pcr(A, W_C, W_P, rhs, tol, resscale, maxiter):
    """PCR from lhs = 0.  Returns PcrRun: lhs, iter, errflag, the residual-norm history (max |resscale .* residual|
    at the head of every iteration, the last one included, as :131-136), cdot and pdot of every iteration that
    computed them, and residual' P residual at iterations 0, 5, 10, ... (the values of :124 and :196)."""
    C = NormalOp(A, W_C)
    diag = NormalOp(A, W_P).diagonal()
    m = C.m
    rhs = np.asarray(rhs, dtype=LD)
    scale = None if resscale is None else np.asarray(resscale, dtype=LD)
    if maxiter < 0:
        maxiter = m + 100
    lhs = np.zeros(m, dtype=LD)
    residual = rhs.copy()
    sresidual = residual / diag
    rps = [np.dot(sresidual, residual)]
    Cres = C.apply(sresidual)
    cdot = np.dot(sresidual, Cres)
    step, Cstep = sresidual.copy(), Cres.copy()
    it, errflag, hist, cdots, pdots = 0, 0, [], [], []
    while True:
        resnorm = np.abs(residual if scale is None else scale * residual).max() if m else LD(0)
        hist.append(resnorm)
        if resnorm <= tol:
            break
        if it == maxiter:
            errflag = 201
            break
        if cdot <= 0:
            errflag = 202
            break
        pCstep = Cstep / diag
        pdot = np.dot(pCstep, Cstep)
        cdots.append(cdot)
        pdots.append(pdot)
        if pdot <= 0:
            errflag = 203
            break
        alpha = cdot / pdot
        if not np.isfinite(alpha):
            errflag = 205
            break
        lhs += alpha * step
        residual -= alpha * Cstep
        sresidual -= alpha * pCstep
        Cres = C.apply(sresidual)
        cdotnew = np.dot(sresidual, Cres)
        beta = cdotnew / cdot
        step = sresidual + beta * step
        Cstep = Cres + beta * Cstep
        cdot = cdotnew
        it += 1
        if it % 5 == 0:
            sresidual = residual / diag
            rsdot = np.dot(sresidual, residual)
            rps.append(rsdot)
            if rsdot >= rps[-2]:
                errflag = 204              # the history then has `it` entries, every other exit it + 1
                break
    return PcrRun(lhs, it, errflag, np.array(hist, dtype=LD), np.array(cdots, dtype=LD), np.array(pdots, dtype=LD),
                  np.array(rps, dtype=LD))
