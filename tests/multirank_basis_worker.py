"""One rank of the basis path (split operator, KKTSolverBasis) on a column-partitioned system, started by
tests/test_gpu_multirank_basis.py as a separate process.  All ranks share GPU 0 and exchange over the library's
direct transport (IPXK_COMM=direct).  The parent writes the whole model and the global factors to an .npz.
argv: rank world idfile outprefix model.npz mode
mode: full (split_apply, cr_solve, kkt_basis_solve), mismatch (rank 1 perturbs one value of L; split_prepare must
fail on every rank), size (kkt_basis_solve only, timed)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ipx_amd import kkt, partition  # noqa: E402
from ipx_amd.synth import CscMatrix  # noqa: E402


def load_model(path):
    z = np.load(path)
    m, n = int(z["m"]), int(z["n"])
    A = CscMatrix(m, n, z["Ap"], z["Ai"], z["Ax"])
    L = CscMatrix(m, m, z["Lp"], z["Li"], z["Lx"])
    U = CscMatrix(m, m, z["Up"], z["Ui"], z["Ux"])
    return A, L, U, {k: z[k] for k in z.files}


def main():
    rank, world = int(sys.argv[1]), int(sys.argv[2])
    idfile, out, path, mode = sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6]
    A, L, U, z = load_model(path)
    m, n = A.nrow, A.ncol
    c0, c1 = partition.row_range(n, rank, world)
    loc = lambda v: partition.col_local_vector(v, n, c0, c1)
    ctx = kkt.KktContext(partition.col_slab_matrix(A, c0, c1), device=0)
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
    ctx.comm_init(uid, rank, world, columns=True)
    status, colscale = loc(z["status"]), loc(z["colscale"])
    # the basic structural columns this rank owns (the helper's view of the global basis)
    owner, _ = partition.col_owner(z["basis"], n, world)
    res = dict(owned=int(np.sum(owner == rank)))
    if mode == "mismatch":
        if rank == 1:
            L = CscMatrix(m, m, L.p, L.i, L.x.copy())
            L.x[L.nnz // 2] *= 1.0 + 1e-12
        t0 = time.perf_counter()
        try:
            ctx.split_prepare(L, U, z["rowperm"], z["colperm"], z["basis"], status, colscale)
            res["code"] = 0
        except kkt.KktError as e:
            res["code"] = e.code
        res["t"] = time.perf_counter() - t0
        np.savez(out + ".rank%d.npz" % rank, **res)
        ctx.close()
        return
    ctx.split_prepare(L, U, z["rowperm"], z["colperm"], z["basis"], status, colscale)
    tol = float(z["tol"])
    if mode == "full":
        res["lhs"], res["dot"] = ctx.split_apply(z["u"])
        lhs, it, err, _, _ = ctx.cr_solve(z["cr_rhs"], tol, None, -1)
        res.update(cr_lhs=lhs, cr_it=it, cr_err=err)
    ctx.kkt_basis_solve(loc(z["a"]), z["b"], tol)           # warm-up (the timing below is a measurement)
    t0 = time.perf_counter()
    x, y, it, err, _ = ctx.kkt_basis_solve(loc(z["a"]), z["b"], tol)
    res.update(x=x, y=y, it=it, err=err, t_solve=time.perf_counter() - t0)
    np.savez(out + ".rank%d.npz" % rank, **res)
    ctx.close()


if __name__ == "__main__":
    main()
