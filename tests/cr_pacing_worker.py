"""One leg of tests/test_gpu_cr_pacing.py, started by it as a separate process: IPXK_CR_PACE, IPXK_CR_AHEAD,
IPXK_CR_REFRESH and IPXK_CR_GRID are read once per process.  Every case's solution, iteration count, errflag,
residual-norm history and ipxk_cr_diagnostics go into one .npz, and under "<case>.stats" what ipxk_cr_loop_stats
reports for the run (iterations enqueued, launches, snapshots, loop events): the drivers differ there and only there.
argv: outfile tolfile (tolfile: the tolerances of the tol cases, "<m>.<k>" -> tol, computed once by the test)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from cr_exits_worker import (DIAG_FIELDS, PLAIN_SHAPE, SEED, SHAPES, SMALL_204, diag_inputs, plain_context,  # noqa: E402
                             plain_inputs)
from cr_lazy_worker import put  # noqa: E402
from ipx_amd import kkt  # noqa: E402

TOL_EXITS = (4, 5, 6, 9, 10, 11)
# seed of the right-hand side for which the reference's residual norm at iteration k lies at least 5 % below every
# earlier one (the history is not monotone), so that a tolerance between the two ends the loop at k and nowhere else
TOL_SEEDS = {1024: {4: 2, 5: 7, 6: 3, 9: 2, 10: 2, 11: 4},
             1025: {4: 6, 5: 2, 6: 6, 9: 2, 10: 3, 11: 6},
             3000: {4: 6, 5: 4, 6: 8, 9: 2, 10: 4, 11: 2}}
MAXITER_EXITS = (0, 1, 4, 5, 6)
CALLBACK_FLAG = 7                                        # what the callback returns at its second poll
OTHER_MAXITER = 11


def tol_rhs(m, k):
    return np.random.default_rng(TOL_SEEDS[m][k]).standard_normal(m)


def put_case(out, name, ctx, res):
    y, it, err, hist, _ = res
    put(out, name, y, it, err, hist)
    s = ctx.cr_loop_stats()                             # host counters of the run: before anything else is enqueued
    out[name + ".stats"] = np.array([s["iterations"], s["launches"], s["snapshots"], s["events"]], dtype=np.int64)
    d = ctx.cr_diagnostics()
    out[name + ".diagn"] = np.array([d[k] for k in DIAG_FIELDS], dtype=np.float64)


def second_poll():
    polls = [0]

    def cb():
        polls[0] += 1
        return CALLBACK_FLAG if polls[0] >= 2 else 0
    return cb


def diag_cases(out, tols):
    for m, n in SHAPES:
        A, W, resscale, rhs = diag_inputs(m, n)
        ctx = kkt.KktContext(A)
        assert ctx.num_dense_cols == 0
        ctx.normal_prepare(W)
        assert ctx.diag_factorize(W, True) == 0
        for k in TOL_EXITS:
            put_case(out, "tol.%d.k%d" % (m, k), ctx,
                     ctx.pcr_solve(tol_rhs(m, k), float(tols["%d.%d" % (m, k)]), resscale, 50, hist_cap=20))
        for maxiter in MAXITER_EXITS:
            put_case(out, "maxiter.%d.%d" % (m, maxiter), ctx, ctx.pcr_solve(rhs, 1e-30, resscale, maxiter, hist_cap=20))
        put_case(out, "callback.%d" % m, ctx, ctx.pcr_solve(rhs, 1e-30, resscale, 50, hist_cap=20, interrupt=second_poll()))
        ctx.close()


def errflag_cases(out):
    # 204 at iteration 5: residual' P residual overflows (tests/test_gpu_cr_exits.py), the refresh must give the same inf
    for name, (m, n, seed) in (("exit204.3000", (3000, 6000, SEED)), ("exit204.300", SMALL_204)):
        A, W, _, rhs = diag_inputs(m, n, seed)
        ctx = kkt.KktContext(A)
        assert ctx.num_dense_cols == 0
        ctx.normal_prepare(W * 1e-60)
        assert ctx.diag_factorize(W, True) == 0
        put_case(out, name, ctx, ctx.pcr_solve(rhs * 1e170, 0.0, None, 200, hist_cap=300))
        ctx.close()
    A, W, _, rhs = diag_inputs(3000, 6000)
    ctx = kkt.KktContext(A)
    ctx.normal_prepare(W)
    assert ctx.diag_factorize(W, True) == 0
    put_case(out, "exit205", ctx, ctx.pcr_solve(rhs * 1e200, 0.0, None, 50, hist_cap=20))       # overflow at k = 0
    put_case(out, "exit202", ctx, ctx.pcr_solve(rhs * 1e-200, 0.0, None, 50, hist_cap=20))     # underflow at k = 0
    ctx.close()


def other_modes(out):
    A, W, resscale, rhs = diag_inputs(3000, 6000, num_dense=5)
    ctx = kkt.KktContext(A)
    assert ctx.num_dense_cols > 0                           # PcrSmw
    ctx.normal_prepare(W)
    assert ctx.diag_factorize(W, True) == 0
    put_case(out, "smw", ctx, ctx.pcr_solve(rhs, 1e-30, resscale, OTHER_MAXITER, hist_cap=20))
    ctx.close()
    B, colscale, rhs = plain_inputs(*PLAIN_SHAPE)
    ctx = plain_context(B, colscale)
    put_case(out, "plain", ctx, ctx.cr_solve(rhs, 1e-30, None, OTHER_MAXITER, hist_cap=20))
    ctx.close()


if __name__ == "__main__":
    out = {}
    diag_cases(out, np.load(sys.argv[2]))
    errflag_cases(out)
    other_modes(out)
    out["grid"] = np.array([int(os.environ.get("IPXK_CR_GRID", "0"))])
    np.savez(sys.argv[1], **out)
