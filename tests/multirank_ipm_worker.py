"""One rank of the device IPM (ipxk_ipm_driver, ipxk_ipm_step) on a column-partitioned system, started by
tests/test_gpu_multirank_ipm.py as a separate process.  All ranks share GPU 0 and exchange over the library's direct
transport (IPXK_COMM=direct).  The parent writes the whole model and the starting iterate to an .npz (mode size: the
worker builds the model itself from the seed).
argv: rank world idfile outprefix model.npz mode
mode: driver (ipm_driver with the diag solver), step_basis (one ipm_step around host-supplied replicated factors),
mismatch_x (rank 1 perturbs a slack entry of x: iterate_set must fail on every rank), mismatch_b (rank 1 perturbs b:
ipm_driver must fail on every rank), interrupt (rank 1 alone interrupts the driver at IPM iteration 3), size (three
driver iterations of the full-size LP, timed)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from ipx_amd import kkt, partition  # noqa: E402
from ipx_amd.synth import CscMatrix  # noqa: E402

INFO_KEYS = ("status_ipm", "errflag", "iter", "kktiter", "basis_updates", "presidual", "dresidual", "pobjective",
             "dobjective", "complementarity", "mu", "step_primal", "step_dual")


def feasible_lp(m, n, seed, per_col=6):
    """min c'x, A x + s = b, x, s >= 0 with an interior point by construction, and the unit starting iterate
    (the construction of tests/test_gpu_ipm_step.py)."""
    from ipx_amd import synth
    rng = np.random.default_rng(seed)
    A = synth.synthetic_lp(m, n, per_col, seed)
    S = A.to_scipy()
    x0, s0 = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, m)
    y0 = -rng.uniform(0.5, 1.5, m)
    b = S @ x0 + s0
    c = np.concatenate([S.T @ y0 + rng.uniform(0.5, 2.0, n), np.zeros(m)])
    N = n + m
    lb, ub = np.zeros(N), np.full(N, np.inf)
    state = np.full(N, 2, dtype=np.uint8)
    it = dict(x=np.ones(N), xl=np.ones(N), xu=np.full(N, np.inf), y=np.zeros(m), zl=np.ones(N), zu=np.zeros(N))
    return A, b, c, lb, ub, state, it


def load_model(path):
    z = np.load(path)
    m, n = int(z["m"]), int(z["n"])
    A = CscMatrix(m, n, z["Ap"], z["Ai"], z["Ax"])
    it = {k: z["it_" + k] for k in ("x", "xl", "xu", "y", "zl", "zu")}
    return A, z["b"], z["c"], z["lb"], z["ub"], z["state"], it, {k: z[k] for k in z.files}


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


def info_array(info):
    return np.array([float(info[k]) for k in INFO_KEYS])


def main():
    rank, world = int(sys.argv[1]), int(sys.argv[2])
    idfile, out, path, mode = sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6]
    if mode == "size":
        z = dict(np.load(path))
        A, b, c, lb, ub, state, it = feasible_lp(int(z["m"]), int(z["n"]), int(z["seed"]), int(z["per_col"]))
    else:
        A, b, c, lb, ub, state, it, z = load_model(path)
    m, n = A.nrow, A.ncol
    c0, c1 = partition.row_range(n, rank, world)
    ctx = kkt.KktContext(partition.col_slab_matrix(A, c0, c1), device=0)
    connect(ctx, rank, world, idfile)
    itl, stl = partition.col_slice_iterate(it, state, n, rank, world)
    bl, cl, lbl, ubl = partition.col_slice_model(b, c, lb, ub, n, rank, world)
    res = dict(c0=c0, c1=c1)
    t0 = time.perf_counter()
    if mode == "mismatch_x":
        if rank == 1:
            itl["x"] = itl["x"].copy()
            itl["x"][c1 - c0 + m // 2] += 1e-12
        try:
            ctx.iterate_set(itl, stl)
            res["code"] = 0
        except kkt.KktError as e:
            res["code"] = e.code
    elif mode == "mismatch_b":
        ctx.iterate_set(itl, stl)
        if rank == 1:
            bl = bl.copy()
            bl[m // 3] *= 1.0 + 1e-12
        try:
            ctx.ipm_driver(bl, cl, lbl, ubl, kkt_maxiter=5000, ipm_maxiter=50)
            res["code"] = 0
        except kkt.KktError as e:
            res["code"] = e.code
    elif mode == "interrupt":
        calls = [0]

        def counting():
            calls[0] += 1
            return 0

        ctx.iterate_set(itl, stl)
        first = ctx.ipm_driver(bl, cl, lbl, ubl, kkt_maxiter=5000, ipm_maxiter=3, interrupt=counting)
        upto = calls[0]                 # the callback's calls in IPM iterations 0-2 (driver and CR cycles)
        calls[0] = 0

        def rank1_only():
            calls[0] += 1
            return 999 if rank == 1 and calls[0] == upto + 1 else 0     # the driver's check at iteration 3

        ctx.iterate_set(itl, stl)
        second = ctx.ipm_driver(bl, cl, lbl, ubl, kkt_maxiter=5000, ipm_maxiter=50, interrupt=rank1_only)
        res.update(first=info_array(first), info=info_array(second), calls=calls[0], upto=upto)
    elif mode == "step_basis":
        L = CscMatrix(m, m, z["Lp"], z["Li"], z["Lx"])
        U = CscMatrix(m, m, z["Up"], z["Ui"], z["Ux"])
        status, colscale = (partition.col_local_vector(z[k], n, c0, c1) for k in ("status", "colscale"))
        ctx.split_prepare(L, U, z["rowperm"], z["colperm"], z["basis"], status, colscale)
        ctx.iterate_set(itl, stl)
        info = ctx.ipm_step(True, bl, cl, lbl, ubl, kkt_tol=float(z["kkt_tol"]), maxiter=1000)
        res.update(step=np.array([info[k] for k in ("step_primal", "step_dual", "mu_before", "mu_after", "sigma",
                                                    "presidual", "dresidual")]),
                   kkt=np.array([info["kktiter_predictor"], info["kktiter_corrector"], info["errflag"]]))
        res.update({"it_" + k: v for k, v in ctx.iterate_get().items()})
    elif mode == "driver":
        ctx.iterate_set(itl, stl)
        info = ctx.ipm_driver(bl, cl, lbl, ubl, kkt_tol=float(z["kkt_tol"]), kkt_maxiter=int(z["kkt_maxiter"]),
                              ipm_maxiter=int(z["ipm_maxiter"]))
        res["info"] = info_array(info)
        res.update({"it_" + k: v for k, v in ctx.iterate_get().items()})
    elif mode == "size":
        ctx.iterate_set(itl, stl)
        infos, times = [], []
        for _ in range(int(z["iters"])):        # one IPM iteration per call: mu after each one
            t = time.perf_counter()
            infos.append(info_array(ctx.ipm_driver(bl, cl, lbl, ubl, ipm_maxiter=1)))
            times.append(time.perf_counter() - t)
        res.update(info=np.array(infos), times=np.array(times))
    res["t"] = time.perf_counter() - t0
    np.savez(out + ".rank%d.npz" % rank, **res)
    ctx.close()


if __name__ == "__main__":
    main()
