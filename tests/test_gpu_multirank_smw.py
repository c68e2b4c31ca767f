"""GPU: dense-column (Sherman-Morrison-Woodbury) preconditioning on partitioned systems.

One rank through the collective code path (IPXK_FORCE_COMM), and separate rank processes that share GPU 0 over the
direct exchange (IPXK_COMM=direct, as tests/test_gpu_multirank.py).  Every rank must classify the same dense columns
as the oracle does on the whole matrix, hold the same k x k factor bit for bit and take the same CR iterations;
reassembled results are compared with the oracle's unpartitioned solve."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import diag_problem, kkt_residual_diag, relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def iters_close(a, b):
    return abs(a - b) <= max(2, int(0.02 * max(a, b)))


def ocsc(po, A):
    return po.Csc(A.nrow, A.ncol, A.p, A.i, A.x)


def oracle_solve(oracle, po, A, st, maxiter=500):
    Ao = ocsc(po, A)
    nd, nzd = oracle.find_dense_columns(Ao)
    ko = oracle.kkt_diag(Ao, nzd, True, maxiter)
    assert ko.factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    x, y, it, err, _ = ko.solve(st["a"], st["b"], 0.3 * np.sqrt(st["mu"]))
    return Ao, nd, nzd, ko, (x, y, it, err)


# --------------------------------------------------------------------------------------
# one rank through the collective code path
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("transport", ["rccl", "direct"])
@pytest.mark.parametrize("columns", [False, True])
@pytest.mark.parametrize("m,n,num_dense", [(3000, 6000, 5), (1500, 3100, 100)])   # k = 100: blocked factor, chunks
def test_smw_single_rank_collective_path(oracle, monkeypatch, transport, columns, m, n, num_dense):
    from ipx_amd import kkt, partition
    from oracle import pyoracle as po
    kkt.load_library()
    A, st = diag_problem(m, n, seed=21, num_dense=num_dense)
    Ao, nd, nzd, ko, (x2, y2, it2, e2) = oracle_solve(oracle, po, A, st)
    assert nd == num_dense
    rhs = np.random.default_rng(1).standard_normal(m)
    # the unpartitioned context
    c0 = kkt.KktContext(A)
    assert c0.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    d0, f0 = c0.diag_get(nd)
    l0, dot0 = c0.diag_apply(rhs)
    c0.close()
    monkeypatch.setenv("IPXK_FORCE_COMM", "1")
    if transport == "direct":
        monkeypatch.setenv("IPXK_COMM", "direct")
    slab = partition.col_slab(A, st, 0, 1) if columns else partition.row_slab(A, st, 0, 1)
    ctx = kkt.KktContext(slab.A)
    ctx.comm_init(ctx.comm_unique_id(), 0, 1, columns=columns)
    assert ctx.num_dense_cols == nd
    assert ctx.kkt_diag_factorize(slab.xl, slab.xu, slab.zl, slab.zu, st["mu"]) == 0
    d1, f1 = ctx.diag_get(nd)
    l1, dot1 = ctx.diag_apply(rhs)
    if columns:       # the diagonal is summed over the ranks by another route: rounding-level differences only
        assert relerr(d1, d0) <= 1e-14 and relerr(f1, f0) <= 1e-12 and relerr(l1, l0) <= 1e-12
    else:             # a one-rank all-reduce is the identity
        assert np.array_equal(d1, d0) and np.array_equal(f1, f0) and np.array_equal(l1, l0) and dot1 == dot0
    x1, y1, it1, e1, _ = ctx.kkt_diag_solve(slab.a, slab.b, 0.3 * np.sqrt(st["mu"]), 500)
    assert e1 == e2 == 0 and iters_close(it1, it2)
    loose = 100.0 if num_dense >= 100 else 1.0
    assert relerr(y1, y2) < 1e-6 * loose and relerr(x1, x2) < 1e-5 * loose
    ctx.close()


# --------------------------------------------------------------------------------------
# separate rank processes
# --------------------------------------------------------------------------------------
def run_ranks(tmp_path, part, world, model, m, n, seed, timeout):
    env = dict(os.environ, IPXK_COMM="direct")
    env.pop("IPXK_FORCE_COMM", None)
    idfile, out = str(tmp_path / "uid"), str(tmp_path / "res")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "multirank_smw_worker.py"), str(r), str(world),
                               idfile, out, part, model, str(m), str(n), str(seed)], env=env, stdout=subprocess.PIPE,
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


CASES = [(part, world, model) for part in ("rows", "columns") for world in (2, 3) for model in ("a", "b")] + \
        [("rows", 2, "c"), ("rows", 3, "c")]


@pytest.mark.parametrize("part,world,model", CASES)
def test_smw_partitioned_multiprocess(oracle, tmp_path, part, world, model):
    from ipx_amd import kkt, partition
    from oracle import pyoracle as po
    from multirank_smw_worker import smw_model
    kkt.load_library()
    m, n, seed = 2501, 6007, 61
    res = run_ranks(tmp_path, part, world, model, m, n, seed, timeout=300)
    A, st = smw_model(model, m, n, seed)
    Ao, nd, nzd, ko, (x_ref, y_ref, it_ref, err_ref) = oracle_solve(oracle, po, A, st)
    assert nd == {"a": 8, "b": 70, "c": 1}[model] and err_ref == 0
    assert all(int(r["k"]) == nd for r in res)
    assert all(int(r["err_f"]) == 0 and int(r["err"]) == 0 for r in res)
    assert all(np.array_equal(res[0]["factor"], r["factor"]) for r in res)
    its = [int(r["it"]) for r in res]
    assert len(set(its)) == 1 and iters_close(its[0], it_ref), (its, it_ref)
    W_ref = ko.get()[0]
    u = np.random.default_rng(0).standard_normal(m)
    P, e = oracle.diag_factorize(Ao, W_ref, nzd, True)
    assert e == 0
    lhs_ref, _ = P.apply(u)
    if part == "rows":
        lhs = np.concatenate([r["lhs"] for r in res])
        x, y = partition.assemble(n, [r["x"] for r in res], [r["y"] for r in res])
    else:
        lhs, y = res[0]["lhs"], res[0]["y"]
        assert all(np.array_equal(res[0]["y"], r["y"]) and np.array_equal(res[0]["lhs"], r["lhs"]) for r in res)
        x = partition.assemble_cols(m, [r["x"] for r in res])
    assert relerr(lhs, lhs_ref) <= 1e-12
    loose = 100.0 if nd >= 100 else 1.0
    assert relerr(y, y_ref) < 1e-6 * loose and relerr(x, x_ref) < 1e-5 * loose


def test_smw_partitioned_c5_full_size(tmp_path):
    """BASELINE config 5 (m=200k, n=400k, 32 dense columns) over 2 row ranks: with SMW the solve converges as the
    unpartitioned one does (tests/test_gpu_parity.py::test_dense_column_stress_full_size); the same slabs without the
    dense-column treatment stop at the cap."""
    from ipx_amd import partition
    m, n = 200000, 400000
    res = run_ranks(tmp_path, "rows", 2, "c5", m, n, 12345, timeout=900)
    A, st = diag_problem(m, n, seed=12345, num_dense=32)
    assert all(int(r["k"]) == 32 and int(r["err_f"]) == 0 for r in res)
    assert np.array_equal(res[0]["factor"], res[1]["factor"])
    its = [int(r["it"]) for r in res]
    assert all(int(r["err"]) == 0 for r in res) and its[0] == its[1] and its[0] < 150
    x, y = partition.assemble(n, [r["x"] for r in res], [r["y"] for r in res])
    W, _ = partition.assemble(n, [r["W"] for r in res], [np.zeros(0)] * 2)
    tol = 0.3 * np.sqrt(st["mu"])
    res1, res2 = kkt_residual_diag(A, W, st["a"], st["b"], x, y)
    assert np.abs(res2).max() < 1e-9 * (1 + np.abs(x).max())
    assert np.abs(np.sqrt(W[n:]) * res1[n:]).max() <= tol * (1 + 1e-9)
    assert all((int(r["it_nosmw"]), int(r["err_nosmw"])) == (300, 201) for r in res)
    print("C5, 2 row ranks: %d iterations, solve %.1f / %.1f ms" % (its[0], 1e3 * float(res[0]["t_solve"]),
                                                                     1e3 * float(res[1]["t_solve"])))
