"""One rank of ipxk_ipm_driver with a positive crossover_start on a column-partitioned system, started by
tests/test_gpu_finish.py as a separate process.  All ranks share GPU 0 and exchange over the library's direct transport
(IPXK_COMM=direct).  Every rank builds synth.mixed_bounds_lp(300, 700, seed, free=False) itself, computes the starting
point, runs the driver and evaluates the dropping residuals of the iterate it stopped at.
argv: rank world idfile outprefix seed crossover_start kkt_tol"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ipx_amd import kkt, partition, synth  # noqa: E402


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
    idfile, out = sys.argv[3], sys.argv[4]
    seed, crossover_start, kkt_tol = int(sys.argv[5]), float(sys.argv[6]), float(sys.argv[7])
    m, n = 300, 700
    A, b, c, lb, ub, _ = synth.mixed_bounds_lp(m, n, seed, free=False)
    c0, c1 = partition.row_range(n, rank, world)
    ctx = kkt.KktContext(partition.col_slab_matrix(A, c0, c1), device=0)
    connect(ctx, rank, world, idfile)
    bl, cl, lbl, ubl = partition.col_slice_model(b, c, lb, ub, n, rank, world)
    assert ctx.ipm_starting_point(bl, cl, lbl, ubl)["status_ipm"] == 0
    ctx.ipm_set_crossover_start(crossover_start)
    g = ctx.ipm_driver(bl, cl, lbl, ubl, kkt_tol=kkt_tol, kkt_maxiter=5000, ipm_maxiter=100)
    drop = ctx.iterate_dropping_residuals(lbl, ubl)
    np.savez(out + ".rank%d.npz" % rank, drop=np.array(drop),
             info=np.array([float(g[k]) for k in ("status_ipm", "iter", "pobjective", "dobjective", "presidual", "dresidual")]))
    ctx.close()


if __name__ == "__main__":
    main()
