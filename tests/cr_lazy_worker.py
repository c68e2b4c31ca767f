"""One leg of tests/test_gpu_cr_lazy.py, started by it as a separate process: IPXK_CR_LAZY is read once per
process, so the deferred and the immediate solution update of the CR loop (ipx_amd/csrc/cr.hip) each get a
process of their own.  Every run's solution, iteration count, errflag and residual-norm history go into one .npz.
argv: single outfile
      rank   outfile rank world idfile      (one rank of a row-partitioned solve on GPU 0, IPXK_COMM=direct)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ipx_amd import kkt, partition, synth  # noqa: E402
from ipx_amd.synth import CscMatrix  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
SYNTH = (3000, 6000, 21)            # m, n, seed: vec_grid(m) = 3 workgroups, the last one ragged
MAXITERS = (0, 1, 4, 5, 6, 11)      # errflag 201 at, before and after a cycle boundary (cycles of 5)
RANK_PROBLEM = (2501, 6007, 61)     # ragged slabs
RANK_MAXITER = 7


def put(out, name, y, it, err, hist=None):
    out[name + ".y"] = np.asarray(y)
    out[name + ".it_err"] = np.array([it, err], dtype=np.int64)
    if hist is not None:
        out[name + ".hist"] = np.asarray(hist)


def golden_diag(out, name):
    d = np.load(os.path.join(GOLD, name + ".npz"))
    m, n = int(d["m"]), int(d["n"])
    ctx = kkt.KktContext(CscMatrix(m, n, d["Ap"], d["Ai"], d["Ax"]))
    ctx.normal_prepare(d["W"])
    assert ctx.diag_factorize(d["W"], True) == int(d["prec_err"])
    y, it, e, hist, _ = ctx.pcr_solve(d["rhs"], float(d["pcr_tol"]), d["resscale"], 500, hist_cap=600)
    put(out, name, y, it, e, hist)
    # an indefinite weight vector: errflag 203 at k = 0 (diag_200), 202 at k = 1 (dense_300)
    ctx.normal_prepare(d["Wneg"])
    assert ctx.diag_factorize(d["Wneg"], False) == 0
    y, it, e, hist, _ = ctx.pcr_solve(d["rhs"], 1e-12, None, 200, hist_cap=20)
    put(out, name + ".neg", y, it, e, hist)
    ctx.close()


def golden_basis(out):
    d = np.load(os.path.join(GOLD, "basis_200.npz"))
    m, n = int(d["m"]), int(d["n"])
    ctx = kkt.KktContext(CscMatrix(m, n, d["Ap"], d["Ai"], d["Ax"]))
    ctx.split_prepare(CscMatrix(m, m, d["Lp"], d["Li"], d["Lx"]), CscMatrix(m, m, d["Up"], d["Ui"], d["Ux"]),
                      d["rowperm"], d["colperm"], d["basis"], d["status"], d["colscale"])
    x, y, it, e, _ = ctx.kkt_basis_solve(d["a"], d["b"], 1e-8)
    put(out, "basis_200.kkt", np.concatenate([x, y]), it, e)
    y, it, e, hist, _ = ctx.cr_solve(d["cr_rhs"], float(d["cr_tol"]), None, -1, hist_cap=300)
    put(out, "basis_200.cr", y, it, e, hist)
    ctx.close()


def synthetic(out):
    m, n, seed = SYNTH
    A = synth.synthetic_lp(m, n, 8, seed)
    st = synth.synthetic_ipm_state(m, n, 1.0, seed)
    W = st["xl"] / st["zl"]
    resscale = 1.0 / np.sqrt(W[n:])
    rhs = np.random.default_rng(2).standard_normal(m)
    ctx = kkt.KktContext(A)
    ctx.normal_prepare(W)
    assert ctx.diag_factorize(W, True) == 0
    for maxiter in MAXITERS:
        y, it, e, hist, _ = ctx.pcr_solve(rhs, 1e-30, resscale, maxiter, hist_cap=20)
        put(out, "synth.maxiter%d" % maxiter, y, it, e, hist)
    y, it, e, hist, _ = ctx.pcr_solve(rhs, 1e300, resscale, 50, hist_cap=20)      # converged at k = 0
    put(out, "synth.tol0", y, it, e, hist)
    y0 = 0.1 * np.random.default_rng(3).standard_normal(m)
    y, it, e, hist, _ = ctx.pcr_solve(rhs, 1e-8, resscale, 1000, lhs0=y0, hist_cap=1200)
    put(out, "synth.lhs0", y, it, e, hist)
    calls = []

    def interrupt():
        calls.append(0)
        return 999 if len(calls) == 2 else 0
    y, it, e, hist, _ = ctx.pcr_solve(rhs, 1e-300, resscale, 100000, hist_cap=40, interrupt=interrupt)
    put(out, "synth.interrupt", y, it, e, hist)
    out["synth.interrupt.calls"] = np.array([len(calls)])
    # the flagship entry point (what bench.py times) on the same model
    assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    x, y, it, e, _ = ctx.kkt_diag_solve(st["a"], st["b"], 0.3 * np.sqrt(st["mu"]), 500)
    put(out, "synth.kkt", np.concatenate([x, y]), it, e)
    ctx.close()


def single(outfile):
    out = {}
    golden_diag(out, "diag_200")
    golden_diag(out, "dense_300")
    golden_basis(out)
    synthetic(out)
    np.savez(outfile, **out)


def rank_leg(outfile, rank, world, idfile):
    m, n, seed = RANK_PROBLEM
    A = synth.synthetic_lp(m, n, 8, seed)
    st = synth.synthetic_ipm_state(m, n, 1.0, seed)
    slab = partition.row_slab(A, st, rank, world)
    ctx = kkt.KktContext(slab.A, device=0)
    if rank == 0:
        uid = ctx.comm_unique_id()
        with open(idfile + ".tmp", "wb") as f:
            f.write(uid)
        os.rename(idfile + ".tmp", idfile)
    else:
        t0 = time.time()
        while not os.path.exists(idfile):
            if time.time() - t0 > 60:
                raise SystemExit("rank 0 never published the communicator id")
            time.sleep(0.02)
        uid = open(idfile, "rb").read()
    ctx.comm_init(uid, rank, world, columns=False)
    assert ctx.kkt_diag_factorize(slab.xl, slab.xu, slab.zl, slab.zu, st["mu"], precond_dense_cols=False) == 0
    x, y, it, err, _ = ctx.kkt_diag_solve(slab.a, slab.b, 1e-30, RANK_MAXITER)
    out = {}
    put(out, "rank", np.concatenate([x, y]), it, err)
    # cdot and pdot overflow: errflag 205 at k = 0, the non-finite scalars go through Pub::publish and the all-gather
    x, y, it, err, _ = ctx.kkt_diag_solve(slab.a * 1e160, slab.b * 1e160, 1e-30, 200)
    put(out, "rank205", np.concatenate([x, y]), it, err)
    out["rank205.ny"] = np.array([y.size])
    np.savez(outfile, **out)
    ctx.close()


if __name__ == "__main__":
    if sys.argv[1] == "single":
        single(sys.argv[2])
    else:
        rank_leg(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
