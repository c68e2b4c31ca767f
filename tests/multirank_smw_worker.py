"""One rank of a partitioned KKTSolverDiag solve WITH dense-column (Sherman-Morrison-Woodbury) preconditioning,
started by tests/test_gpu_multirank_smw.py as a separate process.  All ranks share GPU 0 and exchange over the
library's direct transport (IPXK_COMM=direct), as in tests/multirank_worker.py.
argv: rank world idfile outprefix partition(rows|columns) model m n seed
model: a (synthetic dense columns), b (70 dense columns spread by a column permutation), c (one dense column
whose entries all lie in rank 0's rows), c5 (BASELINE config 5 at the given size, also solved without SMW)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ipx_amd import kkt, partition, synth  # noqa: E402
from ipx_amd.synth import CscMatrix  # noqa: E402


def smw_model(kind, m, n, seed):
    """The whole matrix and IPM state of one test model (every rank builds the same)."""
    st = synth.synthetic_ipm_state(m, n, 1.0, seed)
    if kind == "a":
        return synth.synthetic_lp(m, n, 8, seed, num_dense=8), st
    if kind == "c5":
        return synth.synthetic_lp(m, n, 8, seed, num_dense=32), st
    if kind == "b":
        A = synth.synthetic_lp(m, n, 8, seed, num_dense=70)
        perm = np.random.default_rng(seed + 1).permutation(n)       # new column j = old column perm[j]
    elif kind == "c":
        A = synth.synthetic_lp(m, n, 8, seed)
        r1 = partition.row_range(m, 0, 3)[1]                          # rank 0's rows for 2 and for 3 ranks
        rows = np.sort(np.random.default_rng(seed + 2).choice(r1, size=min(400, r1), replace=False))
        vals = np.random.default_rng(seed + 3).uniform(0.5, 4.0, rows.size)
        cnt = np.diff(A.p)
        cnt[0] = rows.size
        p = np.concatenate([[0], np.cumsum(cnt)])
        i = np.concatenate([rows, A.i[A.p[1]:]])
        x = np.concatenate([vals, A.x[A.p[1]:]])
        return CscMatrix(m, n, p, i, x), st
    else:
        raise ValueError(kind)
    cnt = np.diff(A.p)[perm]
    p = np.concatenate([[0], np.cumsum(cnt)])
    i = np.concatenate([A.i[A.p[j]:A.p[j + 1]] for j in perm])
    x = np.concatenate([A.x[A.p[j]:A.p[j + 1]] for j in perm])
    return CscMatrix(m, n, p, i, x), st


def main():
    rank, world = int(sys.argv[1]), int(sys.argv[2])
    idfile, out, part, kind = sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6]
    m, n, seed = int(sys.argv[7]), int(sys.argv[8]), int(sys.argv[9])
    columns = part == "columns"
    A, st = smw_model(kind, m, n, seed)
    slab = partition.col_slab(A, st, rank, world) if columns else partition.row_slab(A, st, rank, world)
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
    ctx.comm_init(uid, rank, world, columns=columns)
    k = ctx.num_dense_cols
    err_f = ctx.kkt_diag_factorize(slab.xl, slab.xu, slab.zl, slab.zu, st["mu"], precond_dense_cols=True)
    diag, factor = ctx.diag_get(k)
    W, _ = ctx.kkt_diag_get()
    u = np.random.default_rng(0).standard_normal(m)
    lhs, dot = ctx.diag_apply(u if columns else u[slab.r0:slab.r1])
    tol = 0.3 * np.sqrt(st["mu"])
    ctx.kkt_diag_solve(slab.a, slab.b, tol, 500)                         # warm-up (the timing below is a measurement)
    t0 = time.perf_counter()
    x, y, it, err, _ = ctx.kkt_diag_solve(slab.a, slab.b, tol, 500)
    t_solve = time.perf_counter() - t0
    res = dict(k=k, err_f=err_f, diag=diag, factor=factor, W=W, lhs=lhs, dot=dot, x=x, y=y, it=it, err=err,
               t_solve=t_solve)
    if kind == "c5":
        assert ctx.kkt_diag_factorize(slab.xl, slab.xu, slab.zl, slab.zu, st["mu"], precond_dense_cols=False) == 0
        _, _, it2, err2, _ = ctx.kkt_diag_solve(slab.a, slab.b, tol, 300)
        res.update(it_nosmw=it2, err_nosmw=err2)
    np.savez(out + ".rank%d.npz" % rank, **res)
    ctx.close()


if __name__ == "__main__":
    main()
