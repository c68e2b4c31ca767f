"""One rank of ipxk_ipm_starting_point on a column-partitioned system, started by tests/test_gpu_starting_point.py as a
separate process.  All ranks share GPU 0 and exchange over the library's direct transport (IPXK_COMM=direct).
argv: rank world idfile outprefix model.npz mode
mode: start (the starting point, then ipm_driver from it), mismatch_b (rank 1 perturbs b: ipm_starting_point must fail
on every rank)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ipx_amd import kkt, partition  # noqa: E402
from ipx_amd.synth import CscMatrix  # noqa: E402

INFO_KEYS = ("status_ipm", "errflag", "iter", "kktiter", "presidual", "dresidual", "pobjective", "dobjective",
             "complementarity", "mu")


def connect(ctx, rank, world, idfile):
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


def main():
    rank, world = int(sys.argv[1]), int(sys.argv[2])
    idfile, out, path, mode = sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6]
    z = np.load(path)
    m, n = int(z["m"]), int(z["n"])
    A = CscMatrix(m, n, z["Ap"], z["Ai"], z["Ax"])
    c0, c1 = partition.row_range(n, rank, world)
    ctx = kkt.KktContext(partition.col_slab_matrix(A, c0, c1), device=0)
    connect(ctx, rank, world, idfile)
    bl, cl, lbl, ubl = partition.col_slice_model(z["b"], z["c"], z["lb"], z["ub"], n, rank, world)
    res = dict(c0=c0, c1=c1)
    t0 = time.perf_counter()
    if mode == "mismatch_b":
        if rank == 1:
            bl = bl.copy()
            bl[m // 3] *= 1.0 + 1e-12
        try:
            ctx.ipm_starting_point(bl, cl, lbl, ubl)
            res["code"] = 0
        except kkt.KktError as e:
            res["code"] = e.code
    elif mode == "start":
        info = ctx.ipm_starting_point(bl, cl, lbl, ubl)
        res["info"] = np.array([float(info[k]) for k in INFO_KEYS])
        res.update({"it_" + k: v for k, v in ctx.iterate_get().items()})
        drv = ctx.ipm_driver(bl, cl, lbl, ubl, kkt_maxiter=5000, ipm_maxiter=100)
        res["drv"] = np.array([drv["status_ipm"], drv["iter"], drv["errflag"], drv["pobjective"]], dtype=float)
    res["t"] = time.perf_counter() - t0
    np.savez(out + ".rank%d.npz" % rank, **res)
    ctx.close()


if __name__ == "__main__":
    main()
