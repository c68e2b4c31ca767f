"""CPU, world_size 2 (gloo): KKTSolverBasis::_Solve on a column partition (ipx_amd/partition.py, col_slab), the
scheme the HIP library runs on column-partitioned contexts.  Each rank holds a slab of structural columns; the
factors of B and the basis (global numbering) are replicated.  Entries of a[basis] come from their owners (one
all-reduce in which every other rank adds 0), structural products are summed by all-reduce, b and the slack terms
enter once (on rank 0), and each rank writes x_B only into the entries it holds.  The local arithmetic is plain
numpy; the oracle's unpartitioned solve is the checker."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, N, SEED = 300, 700, 17


def _model():
    """The planted basis with free and fixed variables, structural columns permuted so that basic columns sit on
    both slabs (every rank builds the same)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import basis_problem
    from ipx_amd.synth import CscMatrix
    B, st, colscale = basis_problem(M, N, seed=SEED, num_free=3, num_fixed=4)
    A = B["A"]
    perm = np.random.default_rng(SEED).permutation(N)
    inv = np.empty(N, np.int64)
    inv[perm] = np.arange(N)
    S = A.to_scipy().tocsc()[:, perm].tocsc()
    S.sort_indices()
    A = CscMatrix(M, N, S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data)
    status, a = B["status"].copy(), st["a"].copy()
    for v in (status, colscale, a):
        v[:N] = v[:N][perm]
    basis = np.where(B["basis"] < N, inv[np.minimum(B["basis"], N - 1)], B["basis"])
    return dict(A=A, L=B["L"], U=B["U"], rowperm=B["rowperm"], colperm=B["colperm"], basis=basis, status=status,
                colscale=colscale, a=a, b=st["b"])


def basis_solve_cols(rank, world, allsum, Ag, basis, status, colscale, a, b, Bm, n):
    """x (local: [slab; slacks]), y (replicated) of KKTSolverBasis::_Solve on this rank's slab Ag (scipy CSC) with the
    replicated basis matrix Bm = AI[:, basis] (dense) and the global structural column count n."""
    from ipx_amd import partition
    m, nl = Ag.shape
    owner, idx = partition.col_owner(basis, n, world)
    loc = np.where(owner == rank, idx, np.where(owner == partition.REPLICATED, nl + idx, -1))
    mine, slack = (loc >= 0) & (loc < nl), loc >= nl

    def by_position(v):             # owners' entries summed over the ranks, then the slack positions
        out = allsum(np.where(mine, v[np.maximum(loc, 0)], 0.0))
        out[slack] = v[loc[slack]]
        return out

    pos_status, pos_scale, aB = by_position(status.astype(float)), by_position(colscale), by_position(a)
    free, basic = pos_status == 1, pos_status == 0
    W = np.where(status == -1, colscale ** 2, 0.0)
    Ws, WI, lead = W[:nl], W[nl:], 1.0 if rank == 0 else 0.0
    work = np.linalg.solve(Bm.T, np.where(free, aB, 0.0)) if free.any() else np.zeros(m)
    ts, tI = Ws * (a[:nl] - Ag.T @ work), WI * (a[nl:] - work)
    rhs = np.linalg.solve(Bm, allsum(Ag @ ts + lead * tI))
    work = np.linalg.solve(Bm, b)
    d = np.where(basic, pos_scale, 1.0)
    rhs = np.where(basic, (rhs - work) / d + aB * d, 0.0)
    # the normal equations (I + D^-1 B^-1 N N' B^-T D^-1) v = rhs on the non-free positions; N N' summed over the ranks
    NNt = allsum((Ag @ (Ag.T.multiply(Ws[:, None])).tocsc()).toarray() + lead * np.diag(WI))
    Binv = np.linalg.inv(Bm)
    Mop = np.eye(m) + (Binv @ NNt @ Binv.T) / np.outer(d, d)
    keep = ~free
    v = np.zeros(m)
    v[keep] = np.linalg.solve(Mop[np.ix_(keep, keep)], rhs[keep])
    y = np.linalg.solve(Bm.T, np.where(basic, v / d, aB))
    xs, xI = Ws * (a[:nl] - Ag.T @ y), WI * (a[nl:] - y)
    work = np.linalg.solve(Bm, allsum(lead * (b - xI) - Ag @ xs))
    x = np.concatenate([xs, xI])
    x[loc[loc >= 0]] = work[loc >= 0]
    return x, y


def _basis_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    from ipx_amd import partition
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        P = _model()
        A = P["A"]
        c0, c1 = partition.row_range(N, rank, world)
        Ag = partition.col_slab_matrix(A, c0, c1).to_scipy().tocsc()
        loc = lambda v: partition.col_local_vector(v, N, c0, c1)
        AIs = A.with_identity().to_scipy().tocsc()
        Bm = AIs[:, P["basis"]].toarray()

        def allsum(v):
            t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))
            dist.all_reduce(t)
            return t.numpy().copy()

        x, y = basis_solve_cols(rank, world, allsum, Ag, P["basis"], loc(P["status"]), loc(P["colscale"]), loc(P["a"]),
                                P["b"], Bm, N)
        gathered = [None] * world
        dist.all_gather_object(gathered, dict(x=x, y=y))
        if rank == 0:
            np.save(out, np.array([gathered], dtype=object), allow_pickle=True)
    finally:
        dist.destroy_process_group()


def test_basis_solve_column_partition_world2(oracle, tmp_path):
    import torch.multiprocessing as mp
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from ipx_amd import partition
    from oracle import pyoracle as po
    out = str(tmp_path / "bparts.npy")
    port = 33500 + os.getpid() % 2000
    mp.spawn(_basis_worker, args=(2, port, out), nprocs=2, join=True)
    parts = np.load(out, allow_pickle=True)[0]
    P = _model()
    A = P["A"]
    owner, _ = partition.col_owner(P["basis"], N, 2)
    assert (owner == 0).any() and (owner == 1).any()              # basic columns on both slabs
    AI = A.with_identity()
    csc = lambda T: po.Csc(T.nrow, T.ncol, T.p, T.i, T.x)
    S = oracle.split_prepare(csc(AI), N, csc(P["L"]), csc(P["U"]), P["rowperm"], P["colperm"], P["basis"],
                             P["status"], P["colscale"])
    x_ref, y_ref, it_ref, err_ref, _ = S.kkt_solve(P["a"], P["b"], 1e-12)
    assert err_ref == 0
    assert np.array_equal(parts[0]["y"], parts[1]["y"]) and np.array_equal(parts[0]["x"][-M:], parts[1]["x"][-M:])
    x = partition.assemble_cols(M, [p["x"] for p in parts])
    assert np.abs(parts[0]["y"] - y_ref).max() <= 1e-6 * np.abs(y_ref).max()
    assert np.abs(x - x_ref).max() <= 1e-6 * np.abs(x_ref).max()
    r = A.to_scipy() @ x[:N] + x[N:] - P["b"]
    assert np.linalg.norm(r) <= 1e-9 * np.linalg.norm(P["b"])


def test_col_owner():
    sys.path.insert(0, ROOT)
    from ipx_amd import partition
    for n, m in ((41, 7), (2, 5), (1000, 3)):
        j = np.arange(n + m)
        for world in (1, 2, 3, 8):
            rank, local = partition.col_owner(j, n, world)
            assert np.all(rank[n:] == partition.REPLICATED) and np.array_equal(local[n:], np.arange(m))
            for r in range(world):
                c0, c1 = partition.row_range(n, r, world)
                sel = rank == r
                assert np.array_equal(j[sel], np.arange(c0, c1))          # exactly this rank's slab
                assert np.array_equal(local[sel], np.arange(c1 - c0))
                v = np.arange(n + m, dtype=float)
                lv = partition.col_local_vector(v, n, c0, c1)
                assert np.array_equal(lv[local[sel]], v[sel])             # local index into the rank's vector
                assert np.array_equal(lv[(c1 - c0) + local[n:]], v[n:])  # slacks: n_local + slack index
            assert partition.col_owner(n - 1, n, world) == (int(rank[n - 1]), int(local[n - 1]))
            assert partition.col_owner(n, n, world) == (partition.REPLICATED, 0)
