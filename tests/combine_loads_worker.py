"""One leg of tests/test_gpu_combine_loads.py, started by it as a separate process: IPXK_COMBINE_EARLY, IPXK_COMBINE_GRID and
IPXK_COMBINE_GENERIC are read once per process (IPXK_SPMV_LAYOUT and IPXK_SPMV_ACC, which the test sets too, with every
build).  The shapes are those of the `small` case of tests/test_gpu_acc_persistent.py that build 2, 4 and 8 slices under
IPXK_SLICE_TEST_KB, its dense case (dense columns: long rows in A'y, hence the combine's long-row flags, and the SMW
preconditioner) and its planted basis (N N' through nmatrix.hip).  Everything the products and solves return goes into
one .npz; the layout and the slice count in use are recorded next to it.
argv: outfile"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ipx_amd import kkt, synth  # noqa: E402

# m, n, seed, IPXK_SLICE_TEST_KB, IPXK_SLICE_FORCE2
SHAPES = ((9000, 20011, 1, "16", False), (20000, 45000, 2, "128", True), (33333, 70001, 3, "128", False))
SLICE_KEY = {"acc": "acc_nslices", "sliced": "nslices"}


def record_layout(out, tag, ctx):
    """the layout names of A'y and A t, the slice counts of those layouts and the numbers of long rows"""
    names = ctx.spmv_layout()[0]
    info = [ctx.layout_info(w)[0] for w in (0, 1)]
    out[tag + ".layout"] = np.array(names)
    out[tag + ".nslices"] = np.array([d[SLICE_KEY[nm]] if nm in SLICE_KEY else 0 for nm, d in zip(names, info)])
    out[tag + ".nlong"] = np.array([d["nlong"] for d in info])


def products_and_solve(out, tag, A, seed):
    m, n = A.nrow, A.ncol
    ctx = kkt.KktContext(A, device=0)
    record_layout(out, tag, ctx)
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.1, 10.0, m + n)
    ctx.normal_prepare(W)
    lhs, dot = ctx.normal_apply(rng.standard_normal(m))             # EpiScale (A'y), EpiNormalRows (A t) and its dot
    out[tag + ".lhs"] = lhs
    out[tag + ".dot"] = np.array(float(dot).hex())
    st = synth.synthetic_ipm_state(m, n, 1.0, seed)
    assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    x, y, it, err, _ = ctx.kkt_diag_solve(st["a"], st["b"], 0.3 * np.sqrt(st["mu"]), 500)     # + EpiKktRhs, EpiRecoverX, EpiDiagonal
    out[tag + ".x"], out[tag + ".y"], out[tag + ".it_err"] = x, y, np.array([it, err])
    return ctx, W


def main(outfile):
    out = {}
    for (m, n, seed, kb, force2) in SHAPES:
        os.environ["IPXK_SLICE_TEST_KB"] = kb
        if force2:
            os.environ["IPXK_SLICE_FORCE2"] = "1"                    # A'y: y of 160 KiB in two slices of 128 KiB
        ctx, _ = products_and_solve(out, "lp%d" % seed, synth.synthetic_lp(m, n, 8, seed), seed)
        ctx.close()
        os.environ.pop("IPXK_SLICE_FORCE2", None)
    os.environ["IPXK_SLICE_TEST_KB"] = "16"
    # dense columns: the solve above ran PCR with the SMW preconditioner; one application of it on its own as well
    ctx, W = products_and_solve(out, "dense", synth.synthetic_lp(20000, 45000, 8, 6, num_dense=8), 6)
    assert ctx.diag_factorize(W, True) == 0
    plhs, pdot = ctx.diag_apply(np.random.default_rng(60).standard_normal(20000))
    out["dense.smw_lhs"] = plhs
    out["dense.smw_dot"] = np.array(float(pdot).hex())
    ctx.close()
    # basis path: the N N' products of the basis preconditioner
    B = synth.planted_lu_basis(synth.synthetic_lp(20000, 45000, 8, 8), seed=8, num_free=2)
    cs = synth.synthetic_basis_state(B["status"], 1.0, 8)
    ctx = kkt.KktContext(B["A"], device=0)
    ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], cs)
    st = synth.synthetic_ipm_state(20000, 45000, 1.0, 8)
    xb, yb, itb, errb, _ = ctx.kkt_basis_solve(st["a"], st["b"], 1e-8)
    out["basis.x"], out["basis.y"], out["basis.it_err"] = xb, yb, np.array([itb, errb])
    ctx.close()
    np.savez(outfile, **out)


if __name__ == "__main__":
    main(sys.argv[1])
