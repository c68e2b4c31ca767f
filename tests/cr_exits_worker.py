"""One leg of tests/test_gpu_cr_exits.py, started by it as a separate process: IPXK_CR_GRID, IPXK_CR_EARLY and
IPXK_CR_LAZY are read once per process.  IPXK_CR_GRID (unset, 1 or 2) caps the grid of the CR loop's vector kernels
(ipx_amd/csrc/cr.hip), so that a thread has several elements and runs the later groups of kCrUnroll.  Every run's
solution, iteration count, errflag and residual-norm history go into one .npz, the exit cases' ipxk_cr_diagnostics too.
argv: outfile"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from cr_lazy_worker import put  # noqa: E402
from helpers import basis_problem, diag_problem  # noqa: E402
from ipx_amd import kkt  # noqa: E402

SHAPES = ((1024, 2100), (1025, 2100), (3000, 6000))     # rows x columns of the PcrDiag shape cases
MAXITERS = (1, 6, 11)
SEED = 21
PLAIN_SHAPE = (1025, 2300, 41)                          # basis_problem(m, n, seed): plain CR, shape cases
PLAIN_EXIT = (300, 700, 41)                             # plain CR, exit cases (rhs: default_rng(4))
SMALL_204 = (300, 700, 7)
DIAG_FIELDS = ("errflag", "iter", "maxiter", "resnorm", "tol", "cdot", "infnorm_residual", "infnorm_sresidual",
               "rps_old", "rps_new")


def diag_inputs(m, n, seed=SEED, num_dense=0):
    A, st = diag_problem(m, n, seed=seed, num_dense=num_dense)
    W = st["xl"] / st["zl"]
    return A, W, 1.0 / np.sqrt(W[n:]), np.random.default_rng(2).standard_normal(m)


def plain_inputs(m, n, seed):
    B, _, colscale = basis_problem(m, n, seed=seed)
    rhs = np.random.default_rng(4).standard_normal(m)
    rhs[np.nonzero(B["status"][B["basis"]] == 1)[0]] = 0.0      # positions of free basic variables
    return B, colscale, rhs


def plain_context(B, colscale):
    ctx = kkt.KktContext(B["A"])
    ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
    return ctx


def put_exit(out, name, ctx, res):
    y, it, err, hist, _ = res
    put(out, name, y, it, err, hist)
    d = ctx.cr_diagnostics()
    out[name + ".diagn"] = np.array([d[k] for k in DIAG_FIELDS], dtype=np.float64)


def shapes(out):
    for m, n in SHAPES:
        A, W, resscale, rhs = diag_inputs(m, n)
        ctx = kkt.KktContext(A)
        assert ctx.num_dense_cols == 0
        ctx.normal_prepare(W)
        assert ctx.diag_factorize(W, True) == 0
        for maxiter in MAXITERS:
            y, it, e, hist, _ = ctx.pcr_solve(rhs, 1e-30, resscale, maxiter, hist_cap=20)
            put(out, "diag.%d.maxiter%d" % (m, maxiter), y, it, e, hist)
        ctx.close()
    A, W, resscale, rhs = diag_inputs(3000, 6000, num_dense=5)
    ctx = kkt.KktContext(A)
    assert ctx.num_dense_cols > 0                           # PcrSmw
    ctx.normal_prepare(W)
    assert ctx.diag_factorize(W, True) == 0
    for maxiter in MAXITERS:
        y, it, e, hist, _ = ctx.pcr_solve(rhs, 1e-30, resscale, maxiter, hist_cap=20)
        put(out, "smw.maxiter%d" % maxiter, y, it, e, hist)
    ctx.close()
    B, colscale, rhs = plain_inputs(*PLAIN_SHAPE)
    ctx = plain_context(B, colscale)
    for maxiter in MAXITERS:
        y, it, e, hist, _ = ctx.cr_solve(rhs, 1e-30, None, maxiter, hist_cap=20)
        put(out, "plain.maxiter%d" % maxiter, y, it, e, hist)
    ctx.close()


def exits(out):
    # 204: residual' P residual overflows (C from W * 1e-60, P from W, rhs * 1e170), everything else stays finite
    for name, (m, n, seed) in (("exit204.3000", (3000, 6000, SEED)), ("exit204.300", SMALL_204)):
        A, W, _, rhs = diag_inputs(m, n, seed)
        ctx = kkt.KktContext(A)
        assert ctx.num_dense_cols == 0
        ctx.normal_prepare(W * 1e-60)
        assert ctx.diag_factorize(W, True) == 0
        put_exit(out, name, ctx, ctx.pcr_solve(rhs * 1e170, 0.0, None, 200, hist_cap=300))
        ctx.close()
    for mode, num_dense in (("diag", 0), ("smw", 5)):
        A, W, _, rhs = diag_inputs(3000, 6000, num_dense=num_dense)
        ctx = kkt.KktContext(A)
        assert (ctx.num_dense_cols > 0) == (num_dense > 0)
        if num_dense:                                       # the 204 input with dense columns: no 204 (see the test)
            ctx.normal_prepare(W * 1e-60)
            assert ctx.diag_factorize(W, True) == 0
            put_exit(out, "exit204.smw", ctx, ctx.pcr_solve(rhs * 1e170, 0.0, None, 12, hist_cap=300))
        ctx.normal_prepare(W)
        assert ctx.diag_factorize(W, True) == 0
        put_exit(out, "exit205." + mode, ctx, ctx.pcr_solve(rhs * 1e200, 0.0, None, 50, hist_cap=20))      # overflow
        put_exit(out, "exit202." + mode, ctx, ctx.pcr_solve(rhs * 1e-200, 0.0, None, 50, hist_cap=20))    # underflow
        if not num_dense:
            out["exit202.diag.d"] = ctx.diag_get()[0]
        ctx.close()
    B, colscale, rhs = plain_inputs(*PLAIN_EXIT)
    ctx = plain_context(B, colscale)
    put_exit(out, "exit205.plain", ctx, ctx.cr_solve(rhs * 1e200, 0.0, None, 50, hist_cap=20))
    put_exit(out, "exit202.plain", ctx, ctx.cr_solve(rhs * 1e-200, 0.0, None, 50, hist_cap=20))
    ctx.close()


if __name__ == "__main__":
    out = {}
    shapes(out)
    exits(out)
    out["grid"] = np.array([int(os.environ.get("IPXK_CR_GRID", "0"))])
    np.savez(sys.argv[1], **out)
