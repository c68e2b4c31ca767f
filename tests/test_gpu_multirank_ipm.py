"""GPU: the device IPM (iterate reductions, Newton solve, ipm_step, ipm_driver) on column-partitioned systems.

One rank through the collective code path (IPXK_FORCE_COMM) must reproduce the unpartitioned context: bit for bit
for the iterate's residuals, complementarity and objectives and for the basis-preconditioned Newton solve and step;
to the diag solver's tolerance for the diag path (the one-rank column-partition diag solve is not bit-identical, see
test_gpu_parity.py).  Separate rank processes share GPU 0 over the direct exchange (IPXK_COMM=direct, as
tests/test_gpu_multirank_basis.py): every rank must return the same driver info, and the assembled results must match
the unpartitioned run and scipy.  Row partitions are refused; ranks with different replicated inputs fail together;
an interrupt on one rank ends every rank in the same iteration."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import basis_problem, relerr
from multirank_ipm_worker import INFO_KEYS, feasible_lp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARGUMENT = -3
I = {k: i for i, k in enumerate(INFO_KEYS)}
KEYS = ("x", "xl", "xu", "y", "zl", "zu")
# Driver runs compared with an unpartitioned one use a tighter KKT tolerance than the reference's 0.3: the partitioned
# diag solve differs from the unpartitioned one in rounding, and with 0.3 two such runs may take IPM paths that end two or
# three iterations apart (the oracle's driver itself needs 14 iterations at 0.3 and 12 at 1e-3 on one of these LPs).
KKT_TOL_DRIVER = 1e-3


def iters_close(a, b):
    return abs(a - b) <= max(2, int(0.02 * max(a, b)))


def mixed_iterate(m, n, seed):
    """synthetic_iterate (free, upper-bounded, boxed, lower-bounded variables) plus fixed structural and slack ones"""
    from ipx_amd import synth
    P = synth.synthetic_iterate(m, n, seed)
    state = P["state"].copy()
    rng = np.random.default_rng(seed + 1)
    fx = np.concatenate([rng.choice(n, n // 20, replace=False), n + rng.choice(m, m // 25, replace=False)])
    state[fx] = 0
    it = {k: v.copy() for k, v in P["it"].items()}
    for k in ("xl", "xu"):
        it[k][fx] = np.inf
    for k in ("zl", "zu"):
        it[k][fx] = 0.0
    assert {0, 1, 2, 3, 4} <= set(np.unique(state).tolist())
    return P["A"], P["rhs"], np.concatenate([P["obj"], np.zeros(m)]), P["lbs"], P["ubs"], state, it, P["step"]


def basis_iterate(m, n, seed):
    """planted LU factors and an iterate with free, fixed and barrier variables (test_gpu_ipm_step.py's basis step)"""
    B, _, colscale = basis_problem(m, n, seed=seed, num_free=3, num_fixed=4)
    N = n + m
    rng = np.random.default_rng(seed)
    state = np.full(N, 2, dtype=np.uint8)
    state[np.isinf(colscale)] = 1
    state[colscale == 0.0] = 0
    bar = state == 2
    zl = 10.0 ** rng.uniform(-1, 1, N)
    xl = colscale ** 2 * zl
    xl[~bar] = np.inf
    zl[~bar] = 0.0
    xu, zu = np.full(N, np.inf), np.zeros(N)
    fx = state == 0
    xl[fx] = xu[fx] = zl[fx] = zu[fx] = 0.0
    it = dict(x=rng.uniform(-1, 1, N), y=rng.uniform(-1, 1, m), xl=xl, xu=xu, zl=zl, zu=zu)
    lb = np.where(state == 1, -np.inf, 0.0)
    ub = np.where(fx, 0.0, np.inf)
    b, c = rng.uniform(-1, 1, m), rng.uniform(-1, 1, N)
    return B, colscale, b, c, lb, ub, state, it


def forced_context(kkt, A, transport, monkeypatch):
    from ipx_amd import partition
    monkeypatch.setenv("IPXK_FORCE_COMM", "1")
    if transport == "direct":
        monkeypatch.setenv("IPXK_COMM", "direct")
    else:
        monkeypatch.delenv("IPXK_COMM", raising=False)
    ctx = kkt.KktContext(partition.col_slab_matrix(A, 0, A.ncol))
    ctx.comm_init(ctx.comm_unique_id(), 0, 1, columns=True)
    return ctx


def save_model(path, A, b, c, lb, ub, state, it, **extra):
    np.savez(path, m=A.nrow, n=A.ncol, Ap=A.p, Ai=A.i, Ax=A.x, b=b, c=c, lb=lb, ub=ub, state=state,
             **{"it_" + k: v for k, v in it.items()}, **extra)


def run_ranks(tmp_path, world, model_path, mode, timeout):
    env = dict(os.environ, IPXK_COMM="direct")
    env.pop("IPXK_FORCE_COMM", None)
    idfile, out = str(tmp_path / ("uid_" + mode)), str(tmp_path / ("res_" + mode))
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "multirank_ipm_worker.py"), str(r),
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


@pytest.fixture(scope="module")
def kkt():
    from ipx_amd import kkt as k
    k.load_library()
    return k


# --------------------------------------------------------------------------------------
# one rank through the collective code path
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("transport", ["rccl", "direct"])
def test_ipm_single_rank_reductions_and_basis_step(kkt, monkeypatch, transport):
    m, n = 700, 1600
    A, b, c, lb, ub, state, it, step = mixed_iterate(m, n, 51)

    def reductions(ctx):
        ctx.iterate_set(it, state)
        out = dict(res=ctx.iterate_residuals(b, c, lb, ub), comp=ctx.iterate_complementarity(),
                   obj=ctx.iterate_objectives(b, c, lb, ub))
        ctx.iterate_update(0.7, step["dx"], step["dxl"], step["dxu"], 0.6, step["dy"], step["dzl"], step["dzu"])
        out["comp_after"] = ctx.iterate_complementarity()
        ctx.close()
        return out

    ref = reductions(kkt.KktContext(A))
    got = reductions(forced_context(kkt, A, transport, monkeypatch))
    for key in ("rb", "rc", "rl", "ru"):
        assert np.array_equal(got["res"][key], ref["res"][key]), key
    assert (got["res"]["presidual"], got["res"]["dresidual"]) == (ref["res"]["presidual"], ref["res"]["dresidual"])
    assert got["comp"] == ref["comp"] and got["comp_after"] == ref["comp_after"]
    assert got["obj"] == ref["obj"] and ref["obj"][2] != 0.0

    # the basis-preconditioned Newton solve and step (the one-rank basis solve is bit-identical)
    B, colscale, b2, c2, lb2, ub2, state2, it2 = basis_iterate(600, 1400, 29)
    fac = (B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
    bar2 = state2 == 2
    sl = np.zeros(len(state2))
    sl[bar2] = -it2["xl"][bar2] * it2["zl"][bar2]                     # the predictor's complementarity targets

    def basis_run(ctx):
        ctx.split_prepare(*fac)
        ctx.iterate_set(it2, state2)
        r = ctx.iterate_residuals(b2, c2, lb2, ub2)
        out = dict(newton=ctx.newton_solve(True, r["rb"], r["rc"], r["rl"], r["ru"], sl, np.zeros_like(sl), it2["xl"],
                                           it2["xu"], it2["zl"], it2["zu"], state2, 1e-8))
        out["step"] = ctx.ipm_step(True, b2, c2, lb2, ub2, kkt_tol=0.3, maxiter=1000)
        out["it"] = ctx.iterate_get()
        ctx.close()
        return out

    monkeypatch.delenv("IPXK_FORCE_COMM")
    ref = basis_run(kkt.KktContext(B["A"]))
    got = basis_run(forced_context(kkt, B["A"], transport, monkeypatch))
    assert ref["newton"]["errflag"] == 0 and ref["step"]["errflag"] == 0
    for key in ("dx", "dxl", "dxu", "dy", "dzl", "dzu"):
        assert np.array_equal(got["newton"][key], ref["newton"][key]), key
    assert got["newton"]["iter"] == ref["newton"]["iter"]
    assert got["step"] == ref["step"]
    for key in KEYS:
        assert np.array_equal(got["it"][key], ref["it"][key]), key


@pytest.mark.parametrize("transport", ["rccl", "direct"])
def test_ipm_single_rank_diag_path(kkt, monkeypatch, transport):
    m, n = 300, 640
    A, b, c, lb, ub, state, it = feasible_lp(m, n, 72)

    def run(ctx):
        out = {}
        ctx.iterate_set(it, state)
        assert ctx.iterate_factorize_diag() == 0
        r = ctx.iterate_residuals(b, c, lb, ub)
        sl, su = -it["xl"] * it["zl"], np.zeros(n + m)
        out["newton"] = ctx.newton_solve(False, r["rb"], r["rc"], r["rl"], r["ru"], sl, su, it["xl"], it["xu"],
                                         it["zl"], it["zu"], state, 1e-8, 5000)
        out["step"] = ctx.ipm_step(False, b, c, lb, ub, kkt_tol=1e-7, maxiter=5000)
        out["it"] = ctx.iterate_get()
        ctx.iterate_set(it, state)
        out["driver"] = ctx.ipm_driver(b, c, lb, ub, kkt_tol=KKT_TOL_DRIVER, kkt_maxiter=5000, ipm_maxiter=100)
        ctx.close()
        return out

    ref = run(kkt.KktContext(A))
    got = run(forced_context(kkt, A, transport, monkeypatch))
    assert got["newton"]["errflag"] == ref["newton"]["errflag"] == 0
    assert iters_close(got["newton"]["iter"], ref["newton"]["iter"])
    assert relerr(got["newton"]["dy"], ref["newton"]["dy"]) < 1e-6
    for key in ("dx", "dxl", "dzl"):
        assert relerr(got["newton"][key], ref["newton"][key]) < 1e-5, key
    assert got["step"]["errflag"] == ref["step"]["errflag"] == 0
    for key in ("step_primal", "step_dual", "mu_before", "mu_after", "sigma"):
        assert abs(got["step"][key] - ref["step"][key]) <= 1e-5 * abs(ref["step"][key]), key
    assert got["driver"]["status_ipm"] == ref["driver"]["status_ipm"] == 1
    assert abs(got["driver"]["iter"] - ref["driver"]["iter"]) <= 1
    for key in ("pobjective", "dobjective"):
        assert abs(got["driver"][key] - ref["driver"][key]) <= 1e-6 * (1.0 + abs(ref["driver"][key])), key


# --------------------------------------------------------------------------------------
# separate rank processes
# --------------------------------------------------------------------------------------
def at_bound_tail(m, n, seed, world):
    """feasible_lp in which the last rank's columns have nonnegative entries and positive costs: any x_j > 0 there
    only costs and uses capacity, so they stay at their bound 0 (b widened so that the interior point stays one)"""
    from ipx_amd import partition
    from ipx_amd.synth import CscMatrix
    A, b, c, lb, ub, state, it = feasible_lp(m, n, seed)
    c0 = partition.row_range(n, world - 1, world)[0]
    x = A.x.copy()
    x[A.p[c0]:] = np.abs(x[A.p[c0]:])
    A = CscMatrix(m, n, A.p, A.i, x)
    tail = CscMatrix(m, n - c0, A.p[c0:] - A.p[c0], A.i[A.p[c0]:], x[A.p[c0]:]).to_scipy()
    b = b + tail @ np.full(n - c0, 2.0)
    c = c.copy()
    c[c0:n] = np.random.default_rng(seed).uniform(0.5, 2.0, n - c0)
    return A, b, c, lb, ub, state, it


@pytest.mark.parametrize("world,case", [(2, "plain"), (3, "plain"), (3, "at_bound")])
def test_ipm_driver_partitioned_multiprocess(kkt, tmp_path, world, case):
    from scipy.optimize import linprog
    from ipx_amd import partition
    m, n = 300, 640
    A, b, c, lb, ub, state, it = (feasible_lp(m, n, 81) if case == "plain" else at_bound_tail(m, n, 82, world))
    path = str(tmp_path / "model.npz")
    save_model(path, A, b, c, lb, ub, state, it, kkt_tol=KKT_TOL_DRIVER, kkt_maxiter=5000, ipm_maxiter=100)
    res = run_ranks(tmp_path, world, path, "driver", timeout=300)
    ctx = kkt.KktContext(A)
    ctx.iterate_set(it, state)
    ref = ctx.ipm_driver(b, c, lb, ub, kkt_tol=KKT_TOL_DRIVER, kkt_maxiter=5000, ipm_maxiter=100)
    it_ref = ctx.iterate_get()
    ctx.close()
    info = res[0]["info"]
    assert all(np.array_equal(info, r["info"]) for r in res)                   # every rank returns the same info
    assert ref["status_ipm"] == 1, ref
    assert int(info[I["status_ipm"]]) == 1, info
    assert abs(int(info[I["iter"]]) - ref["iter"]) <= max(2, int(0.1 * ref["iter"]))
    got = partition.assemble_iterate(m, [{k: r["it_" + k] for k in KEYS} for r in res])
    assert all(np.array_equal(res[0]["it_y"], r["it_y"]) for r in res)
    assert relerr(got["x"], it_ref["x"]) < 1e-6 and relerr(got["y"], it_ref["y"]) < 1e-6
    f = float(info[I["pobjective"]])
    assert abs(f - ref["pobjective"]) <= 1e-6 * (1.0 + abs(ref["pobjective"]))
    r = linprog(c[:n], A_ub=A.to_scipy(), b_ub=b, bounds=[(0, None)] * n, method="highs")
    assert r.status == 0 and abs(f - r.fun) <= 1e-6 * (1.0 + abs(r.fun))
    if case == "at_bound":
        c0 = partition.row_range(n, world - 1, world)[0]
        assert np.abs(r.x[c0:]).max() < 1e-9 and np.abs(got["x"][c0:n]).max() < 1e-5


def test_ipm_step_basis_partitioned(kkt, tmp_path):
    from ipx_amd import partition
    B, colscale, b, c, lb, ub, state, it = basis_iterate(600, 1400, 29)
    m, n = 600, 1400
    path = str(tmp_path / "model.npz")
    save_model(path, B["A"], b, c, lb, ub, state, it, Lp=B["L"].p, Li=B["L"].i, Lx=B["L"].x, Up=B["U"].p, Ui=B["U"].i,
               Ux=B["U"].x, rowperm=B["rowperm"], colperm=B["colperm"], basis=B["basis"], status=B["status"],
               colscale=colscale, kkt_tol=1e-7)
    res = run_ranks(tmp_path, 2, path, "step_basis", timeout=300)
    ctx = kkt.KktContext(B["A"])
    ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
    ctx.iterate_set(it, state)
    ref = ctx.ipm_step(True, b, c, lb, ub, kkt_tol=1e-7, maxiter=1000)
    it_ref = ctx.iterate_get()
    ctx.close()
    assert ref["errflag"] == 0 and all(int(r["kkt"][2]) == 0 for r in res)
    assert np.array_equal(res[0]["step"], res[1]["step"]) and np.array_equal(res[0]["kkt"], res[1]["kkt"])
    for k, key in enumerate(("step_primal", "step_dual", "mu_before", "mu_after")):
        assert abs(res[0]["step"][k] - ref[key]) <= 1e-5 * abs(ref[key]), key
    got = partition.assemble_iterate(m, [{k: r["it_" + k] for k in KEYS} for r in res])
    for key in ("x", "y", "zl"):
        f = np.isfinite(it_ref[key])
        assert relerr(got[key][f], it_ref[key][f]) < 1e-5, key


# --------------------------------------------------------------------------------------
# refusals and agreement
# --------------------------------------------------------------------------------------
def test_ipm_refusals(kkt, monkeypatch):
    from ipx_amd import partition
    m, n = 200, 450
    A, b, c, lb, ub, state, it = feasible_lp(m, n, 5)
    monkeypatch.setenv("IPXK_FORCE_COMM", "1")
    monkeypatch.setenv("IPXK_COMM", "direct")
    rows = kkt.KktContext(partition.slab_matrix(A, 0, m))
    rows.comm_init(rows.comm_unique_id(), 0, 1, columns=False)
    rows.iterate_set(it, state)
    assert rows.iterate_factorize_diag() == 0
    z = np.zeros(n + m)
    refused = [lambda: rows.iterate_residuals(b, c, lb, ub), lambda: rows.iterate_objectives(b, c, lb, ub),
               lambda: rows.newton_solve(False, b, c, z, z, z, z, it["xl"], it["xu"], it["zl"], it["zu"], state, 1e-6),
               lambda: rows.ipm_step(False, b, c, lb, ub), lambda: rows.ipm_driver(b, c, lb, ub)]
    for call in refused:
        with pytest.raises(kkt.KktError) as e:
            call()
        assert e.value.code == E_ARGUMENT and "ipxk_comm_init_columns" in str(e.value)
    rows.close()
    cols = forced_context(kkt, A, "direct", monkeypatch)
    cols.iterate_set(it, state)
    with pytest.raises(kkt.KktError) as e:
        cols.ipm_driver_basis(b, c, lb, ub, ipm_maxiter=5)
    assert e.value.code == E_ARGUMENT and "ipxk_split_prepare" in str(e.value)
    g = cols.ipm_driver(b, c, lb, ub, kkt_maxiter=5000, ipm_maxiter=100)        # the context stays usable
    assert g["status_ipm"] == 1
    cols.close()


@pytest.mark.parametrize("mode", ["mismatch_x", "mismatch_b"])
def test_ipm_mismatched_inputs_fail_together(tmp_path, mode):
    A, b, c, lb, ub, state, it = feasible_lp(300, 640, 81)
    path = str(tmp_path / "model.npz")
    save_model(path, A, b, c, lb, ub, state, it)
    res = run_ranks(tmp_path, 2, path, mode, timeout=120)
    assert [int(r["code"]) for r in res] == [E_ARGUMENT, E_ARGUMENT]
    assert all(float(r["t"]) < 30.0 for r in res)


def test_ipm_interrupt_on_one_rank(tmp_path):
    A, b, c, lb, ub, state, it = feasible_lp(300, 640, 81)
    path = str(tmp_path / "model.npz")
    save_model(path, A, b, c, lb, ub, state, it)
    res = run_ranks(tmp_path, 2, path, "interrupt", timeout=300)
    assert all(int(r["first"][I["status_ipm"]]) == 6 and int(r["first"][I["iter"]]) == 3 for r in res)
    assert int(res[0]["upto"]) == int(res[1]["upto"])
    for r in res:
        assert int(r["info"][I["status_ipm"]]) == 5 and int(r["info"][I["iter"]]) == 3, r["info"]
        assert int(r["calls"]) == int(r["upto"]) + 1
    assert np.array_equal(res[0]["info"], res[1]["info"])


# --------------------------------------------------------------------------------------
# size
# --------------------------------------------------------------------------------------
def test_ipm_driver_partitioned_full_size(kkt, tmp_path):
    from ipx_amd import partition
    import time
    m, n, seed, per_col, iters = 1000000, 2000000, 7, 8, 3
    path = str(tmp_path / "size.npz")
    np.savez(path, m=m, n=n, seed=seed, per_col=per_col, iters=iters)
    res = run_ranks(tmp_path, 2, path, "size", timeout=1500)
    A, b, c, lb, ub, state, it = feasible_lp(m, n, seed, per_col)
    ctx = kkt.KktContext(A)
    ctx.iterate_set(it, state)
    ref, t_ref = [], []
    for _ in range(iters):
        t = time.perf_counter()
        g = ctx.ipm_driver(b, c, lb, ub, ipm_maxiter=1)
        t_ref.append(time.perf_counter() - t)
        ref.append([float(g[k]) for k in INFO_KEYS])
    ctx.close()
    ref = np.array(ref)
    assert np.array_equal(res[0]["info"], res[1]["info"])
    got = res[0]["info"]
    assert (got[:, I["status_ipm"]] == 6).all() and (ref[:, I["status_ipm"]] == 6).all()
    assert (got[:, I["errflag"]] == 0).all()
    mu, mu_ref = got[:, I["mu"]], ref[:, I["mu"]]
    assert (np.abs(mu - mu_ref) <= 1e-3 * mu_ref).all(), (mu, mu_ref)
    assert mu[-1] < mu[0]
    print("ipm driver, m=%d n=%d over 2 column ranks: %s s per IPM iteration (ranks), %s s unpartitioned; mu %s"
          % (m, n, np.round(res[0]["times"], 3).tolist() + np.round(res[1]["times"], 3).tolist(),
             np.round(t_ref, 3).tolist(), mu.tolist()))
