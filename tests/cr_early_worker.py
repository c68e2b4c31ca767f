"""One leg of tests/test_gpu_cr_early.py, started by it as a separate process: IPXK_CR_EARLY (like IPXK_CR_LAZY and
IPXK_SPMV_LAYOUT, which some legs set too) is read once per process.  The cases of tests/cr_lazy_worker.py have 3000 rows:
3 workgroups in the vector kernels, so at most one partial per thread in the reductions of the CR loop.  This one runs the
loop at 70001 rows: vec_grid(m) = 274 workgroups, hence threads with two residual-norm / pdot partials next to threads with
one, a ragged last workgroup (its clamped loads), and with IPXK_SPMV_LAYOUT=plain 2048 cdot partials, eight per thread.
argv: outfile"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from cr_lazy_worker import put  # noqa: E402
from ipx_amd import kkt, synth  # noqa: E402

PROBLEM = (70001, 150001, 33)       # m, n, seed
MAXITERS = (5, 6)                   # across the rsdot reduction of every fifth iteration (k = 5)


def main(outfile):
    m, n, seed = PROBLEM
    A = synth.synthetic_lp(m, n, 8, seed)
    st = synth.synthetic_ipm_state(m, n, 1.0, seed)
    W = st["xl"] / st["zl"]
    resscale = 1.0 / np.sqrt(W[n:])
    rhs = np.random.default_rng(4).standard_normal(m)
    out = {}
    ctx = kkt.KktContext(A)
    ctx.normal_prepare(W)
    assert ctx.diag_factorize(W, True) == 0
    out["layout"] = np.array(ctx.spmv_layout()[0])
    for maxiter in MAXITERS:
        y, it, e, hist, _ = ctx.pcr_solve(rhs, 1e-30, resscale, maxiter, hist_cap=20)
        put(out, "big.maxiter%d" % maxiter, y, it, e, hist)
    assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    x, y, it, e, _ = ctx.kkt_diag_solve(st["a"], st["b"], 0.3 * np.sqrt(st["mu"]), 500)
    put(out, "big.kkt", np.concatenate([x, y]), it, e)
    np.savez(outfile, **out)
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1])
