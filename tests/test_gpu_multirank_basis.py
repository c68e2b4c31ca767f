"""GPU: the basis path (split operator, CR on it, KKTSolverBasis) on column-partitioned systems.

One rank through the collective code path (IPXK_FORCE_COMM) must reproduce the unpartitioned context bit for bit.
Separate rank processes share GPU 0 over the direct exchange (IPXK_COMM=direct, as tests/test_gpu_multirank_smw.py):
every rank must hold the same replicated vectors, and the reassembled results must match the oracle's unpartitioned
operator and solve.  Row partitions, the device LU and Maxvolume are refused; ranks given different factors fail
together."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import basis_problem, relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARGUMENT = -3


def iters_close(a, b):
    return abs(a - b) <= max(2, int(0.02 * max(a, b)))


def ocsc(po, M):
    return po.Csc(M.nrow, M.ncol, M.p, M.i, M.x)


def oracle_split(oracle, po, P):
    A = P["A"]
    AI = A.with_identity()
    return oracle.split_prepare(ocsc(po, AI), A.ncol, ocsc(po, P["L"]), ocsc(po, P["U"]), P["rowperm"], P["colperm"],
                                P["basis"], P["status"], P["colscale"])


def planted_model(m, n, seed, permute, band=None):
    """The planted basis with free and fixed variables; permute: structural columns in random order (basis
    renumbered), so that basic columns sit on every slab."""
    from ipx_amd.synth import CscMatrix
    B, st, colscale = basis_problem(m, n, seed=seed, num_free=6, num_fixed=9, band=band)
    A, status, basis = B["A"], B["status"].copy(), B["basis"].copy()
    a = st["a"].copy()
    if permute:
        perm = np.random.default_rng(seed + 7).permutation(n)       # new column j = old column perm[j]
        inv = np.empty(n, np.int64)
        inv[perm] = np.arange(n)
        cnt = np.diff(A.p)[perm]
        p = np.concatenate([[0], np.cumsum(cnt)])
        i = np.concatenate([A.i[A.p[j]:A.p[j + 1]] for j in perm])
        x = np.concatenate([A.x[A.p[j]:A.p[j + 1]] for j in perm])
        A = CscMatrix(m, n, p, i, x)
        for v in (status, colscale, a):
            v[:n] = v[:n][perm]
        basis = np.where(basis < n, inv[np.minimum(basis, n - 1)], basis)
    return dict(A=A, L=B["L"], U=B["U"], rowperm=B["rowperm"], colperm=B["colperm"], basis=basis, status=status,
                colscale=colscale, a=a, b=st["b"], tol=1e-8)


def mixed_model(oracle, m, n, world, seed):
    """A basis of slack and structural columns, none of them on the last rank's slab, factorized by the oracle's LU;
    dependent columns are replaced by the slack of their row and the basis is factorized again."""
    from ipx_amd import partition, synth
    rng = np.random.default_rng(seed)
    A = synth.synthetic_lp(m, n, 8, seed)
    c_last = partition.row_range(n, world - 1, world)[0]             # where the last rank's slab starts
    ns = m // 20
    struct = rng.choice(c_last, size=ns, replace=False)
    slacks = n + rng.choice(m, size=m - ns, replace=False)
    basis = rng.permutation(np.concatenate([struct, slacks])).astype(np.int64)
    AIs = A.with_identity().to_scipy().tocsc()

    def factorize(basis):
        Bm = AIs[:, basis].tocsc()
        Bm.sort_indices()
        return Bm, oracle.lu_factorize(m, Bm.indptr[:-1], Bm.indptr[1:], Bm.indices, Bm.data)

    Bm, F = factorize(basis)
    if len(F["dependent"]):
        for k in F["dependent"]:
            basis[F["colperm"][k]] = n + F["rowperm"][k]
        Bm, F = factorize(basis)
    assert len(F["dependent"]) == 0 and len(set(basis.tolist())) == m
    status = np.full(n + m, -1, np.int64)
    status[basis] = 0
    status[basis[basis < n][:3]] = 1                                  # free structural variables
    status[n + rng.choice(np.setdiff1d(np.arange(m), basis[basis >= n] - n), 4, replace=False)] = -2
    colscale = synth.synthetic_basis_state(status, 1.0, seed)
    st = synth.synthetic_ipm_state(m, n, 1.0, seed)
    return dict(A=A, L=F["L"], U=F["U"], rowperm=F["rowperm"], colperm=F["colperm"], basis=basis, status=status,
                colscale=colscale, a=st["a"], b=st["b"], tol=1e-8)


def save_model(path, P, u, cr_rhs):
    A, L, U = P["A"], P["L"], P["U"]
    np.savez(path, m=A.nrow, n=A.ncol, Ap=A.p, Ai=A.i, Ax=A.x, Lp=L.p, Li=L.i, Lx=L.x, Up=U.p, Ui=U.i, Ux=U.x,
             rowperm=P["rowperm"], colperm=P["colperm"], basis=P["basis"], status=P["status"],
             colscale=P["colscale"], a=P["a"], b=P["b"], tol=P["tol"], u=u, cr_rhs=cr_rhs)


def run_ranks(tmp_path, world, model_path, mode, timeout):
    env = dict(os.environ, IPXK_COMM="direct")
    env.pop("IPXK_FORCE_COMM", None)
    idfile, out = str(tmp_path / ("uid_" + mode)), str(tmp_path / ("res_" + mode))
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "multirank_basis_worker.py"), str(r),
                               str(world), idfile, out, model_path, mode], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=timeout)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            for q in procs:
                q.wait()
            pytest.fail("a rank did not finish:\n" + "\n".join(logs))
        if p.returncode != 0:
            for q in procs:
                q.kill()
            for q in procs:
                q.wait()
            pytest.fail("a rank failed:\n" + logs[-1])
    return [np.load(out + ".rank%d.npz" % r) for r in range(world)]


# --------------------------------------------------------------------------------------
# one rank through the collective code path
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("transport", ["rccl", "direct"])
def test_basis_single_rank_collective_path(monkeypatch, transport):
    from ipx_amd import kkt, partition
    kkt.load_library()
    m, n = 2500, 5200
    monkeypatch.setenv("IPXK_SPMV_LAYOUT", "phased")
    P = planted_model(m, n, seed=3, permute=False)
    A, L, U = P["A"], P["L"], P["U"]
    rng = np.random.default_rng(5)
    u, v = rng.standard_normal(m), rng.standard_normal(m)
    cs2 = P["colscale"] * rng.uniform(0.5, 2.0, n + m)
    args = (L, U, P["rowperm"], P["colperm"], P["basis"])

    def run(ctx, status, colscale, a, rescale_ctx=True):
        out = {}
        ctx.split_prepare(*args, status, colscale)
        out["levels"] = ctx.split_levels()
        out["fwd"], out["bwd"] = ctx.forward_solve(u), ctx.backward_solve(u)
        out["dN"], out["dT"] = ctx.solve_dense(u, "N"), ctx.solve_dense(u, "T")
        out["lhs"], out["dot"] = ctx.split_apply(u)
        out["cr"] = ctx.cr_solve(v, 1e-10, None, -1)[:3]
        out["kkt"] = ctx.kkt_basis_solve(a, P["b"], P["tol"])[:4]
        if rescale_ctx:             # Rescale, then the same solve as after a fresh Prepare with the new scaling
            ctx.split_rescale(status, cs2 if colscale is P["colscale"] else colscale)
            out["kkt_rescaled"] = ctx.kkt_basis_solve(a, P["b"], P["tol"])[:4]
            out["lhs_rescaled"] = ctx.split_apply(u)
        # the resident form
        ctx.set_pointer_mode(True)
        N = ctx.n + ctx.m
        da, db = kkt.DeviceVector(ctx, N, a), kkt.DeviceVector(ctx, m, P["b"])
        dx, dy = kkt.DeviceVector(ctx, N), kkt.DeviceVector(ctx, m)
        it, err, _ = ctx.kkt_basis_solve_resident(da, db, dx, dy, P["tol"])
        out["resident"] = (dx.download(), dy.download(), it, err)
        for d in (da, db, dx, dy):
            d.free()
        ctx.set_pointer_mode(False)
        return out

    c0 = kkt.KktContext(A)
    ref = run(c0, P["status"], P["colscale"], P["a"])
    c0.split_prepare(*args, P["status"], cs2)                  # a fresh Prepare with the new scaling
    ref_fresh = c0.kkt_basis_solve(P["a"], P["b"], P["tol"])[:4], c0.split_apply(u)
    c0.close()
    monkeypatch.setenv("IPXK_FORCE_COMM", "1")
    if transport == "direct":
        monkeypatch.setenv("IPXK_COMM", "direct")
    slab = partition.col_slab_matrix(A, 0, n)
    ctx = kkt.KktContext(slab)
    ctx.comm_init(ctx.comm_unique_id(), 0, 1, columns=True)
    assert partition.col_owner(P["basis"], n, 1)[0].max() == 0
    got = run(ctx, P["status"], P["colscale"], P["a"])
    ctx.close()
    assert got["levels"] == ref["levels"]
    for k in ("fwd", "bwd", "dN", "dT", "lhs"):
        assert np.array_equal(got[k], ref[k]), k
    assert got["dot"] == ref["dot"]
    lc, ic, ec = got["cr"]
    assert (ic, ec) == ref["cr"][1:] and np.array_equal(lc, ref["cr"][0])
    for key in ("kkt", "kkt_rescaled", "resident"):
        x, y, it, err = got[key]
        xr, yr, itr, errr = ref[key]
        assert (it, err) == (itr, errr) and err == 0, key
        assert np.array_equal(x, xr) and np.array_equal(y, yr), key
    # Rescale == fresh Prepare, bit for bit (partitioned context against the unpartitioned fresh one)
    x, y, it, err = got["kkt_rescaled"]
    (xf, yf, itf, errf), (lf, df) = ref_fresh
    assert (it, err) == (itf, errf) and np.array_equal(x, xf) and np.array_equal(y, yf)
    assert np.array_equal(got["lhs_rescaled"][0], lf)


# --------------------------------------------------------------------------------------
# separate rank processes
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("model", ["a", "b"])
def test_basis_partitioned_multiprocess(oracle, tmp_path, world, model):
    from ipx_amd import kkt, partition
    from oracle import pyoracle as po
    kkt.load_library()
    m, n = 2500, 5200
    P = planted_model(m, n, seed=3, permute=True) if model == "a" else mixed_model(oracle, 1500, 3200, world, 9)
    m, n = P["A"].nrow, P["A"].ncol
    rng = np.random.default_rng(11)
    S = oracle_split(oracle, po, P)
    # a right-hand side in the operator's range (zero at the free positions, as KKTSolverBasis builds it)
    u, cr_rhs = rng.standard_normal(m), S.apply(rng.standard_normal(m))[0]
    path = str(tmp_path / "model.npz")
    save_model(path, P, u, cr_rhs)
    res = run_ranks(tmp_path, world, path, "full", timeout=300)
    owned = [int(r["owned"]) for r in res]
    if model == "a":
        assert min(owned) > 0
    else:
        assert owned[-1] == 0 and sum(owned) > 0
    # replicated vectors and iteration counts are the same on every rank
    for key in ("lhs", "cr_lhs", "y"):
        assert all(np.array_equal(res[0][key], r[key]) for r in res), key
    assert all(np.array_equal(res[0]["x"][-m:], r["x"][-m:]) for r in res)
    assert len({(int(r["it"]), int(r["err"]), int(r["cr_it"]), int(r["cr_err"])) for r in res}) == 1
    lhs_ref, _ = S.apply(u)
    assert relerr(res[0]["lhs"], lhs_ref) <= 1e-12
    cr_ref, cr_it_ref, cr_err_ref, _ = oracle.cr_solve(S.apply, cr_rhs, P["tol"], None, -1)
    assert int(res[0]["cr_err"]) == cr_err_ref == 0 and iters_close(int(res[0]["cr_it"]), cr_it_ref)
    assert relerr(res[0]["cr_lhs"], cr_ref) < 1e-6
    x_ref, y_ref, it_ref, err_ref, _ = S.kkt_solve(P["a"], P["b"], P["tol"])
    assert int(res[0]["err"]) == err_ref == 0 and iters_close(int(res[0]["it"]), it_ref), (int(res[0]["it"]), it_ref)
    x = partition.assemble_cols(m, [r["x"] for r in res])
    assert relerr(res[0]["y"], y_ref) < 1e-6 and relerr(x, x_ref) < 1e-6
    r = P["A"].to_scipy() @ x[:n] + x[n:] - P["b"]
    assert np.linalg.norm(r) / np.linalg.norm(P["b"]) < 1e-9


# --------------------------------------------------------------------------------------
# refusals and agreement
# --------------------------------------------------------------------------------------
def test_basis_refusals(monkeypatch):
    from ipx_amd import kkt, partition
    kkt.load_library()
    m, n = 600, 1300
    P = planted_model(m, n, seed=8, permute=False)
    args = (P["L"], P["U"], P["rowperm"], P["colperm"], P["basis"], P["status"], P["colscale"])
    monkeypatch.setenv("IPXK_FORCE_COMM", "1")
    monkeypatch.setenv("IPXK_COMM", "direct")
    rows = kkt.KktContext(partition.slab_matrix(P["A"], 0, m))
    rows.comm_init(rows.comm_unique_id(), 0, 1, columns=False)
    with pytest.raises(kkt.KktError) as e:
        rows.split_prepare(*args)
    assert e.value.code == E_ARGUMENT and "ipxk_comm_init_columns" in str(e.value)
    rows.close()
    ctx = kkt.KktContext(partition.col_slab_matrix(P["A"], 0, n))
    ctx.comm_init(ctx.comm_unique_id(), 0, 1, columns=True)
    refused = [lambda: ctx.lu_factorize_basis(P["basis"]), lambda: ctx.split_prepare_lu(P["status"], P["colscale"]),
               lambda: ctx.maxvolume(P["status"], P["colscale"]),
               lambda: ctx.maxvolume_sequential(P["status"], P["colscale"])]
    for call in refused:
        with pytest.raises(kkt.KktError) as e:
            call()
        assert e.value.code == E_ARGUMENT and "ipxk_split_prepare" in str(e.value)
    # the context stays usable
    ctx.split_prepare(*args)
    x, y, it, err, _ = ctx.kkt_basis_solve(P["a"], P["b"], 1e-8)
    assert err == 0 and np.all(np.isfinite(x))
    ctx.close()


def test_basis_mismatched_factors_fail_together(tmp_path):
    P = planted_model(2500, 5200, seed=3, permute=True)
    path = str(tmp_path / "model.npz")
    save_model(path, P, np.zeros(2500), np.zeros(2500))
    res = run_ranks(tmp_path, 2, path, "mismatch", timeout=120)
    assert [int(r["code"]) for r in res] == [E_ARGUMENT, E_ARGUMENT]
    assert all(float(r["t"]) < 30.0 for r in res)


# --------------------------------------------------------------------------------------
# size
# --------------------------------------------------------------------------------------
def test_basis_partitioned_full_size(tmp_path):
    from ipx_amd import kkt, partition
    kkt.load_library()
    m, n = 200000, 400000
    P = planted_model(m, n, seed=5, permute=True, band=1000)
    path = str(tmp_path / "model.npz")
    save_model(path, P, np.zeros(m), np.zeros(m))
    res = run_ranks(tmp_path, 2, path, "size", timeout=900)
    c = kkt.KktContext(P["A"])
    c.split_prepare(P["L"], P["U"], P["rowperm"], P["colperm"], P["basis"], P["status"], P["colscale"])
    x_ref, y_ref, it_ref, err_ref, _ = c.kkt_basis_solve(P["a"], P["b"], P["tol"])
    c.close()
    its = [int(r["it"]) for r in res]
    assert all(int(r["err"]) == 0 for r in res) and its[0] == its[1] and err_ref == 0
    assert np.array_equal(res[0]["y"], res[1]["y"])
    x = partition.assemble_cols(m, [r["x"] for r in res])
    assert relerr(res[0]["y"], y_ref) < 1e-6 and relerr(x, x_ref) < 1e-6
    print("basis path, m=%d n=%d over 2 column ranks: %d iterations (unpartitioned %d), %.3f / %.3f ms per iteration"
          % (m, n, its[0], it_ref, 1e3 * float(res[0]["t_solve"]) / max(its[0], 1),
             1e3 * float(res[1]["t_solve"]) / max(its[1], 1)))
