"""GPU: ipxk_ipm_starting_point = IPM::ComputeStartingPoint (reference src/ipm.cc:125-259) and
ipxk_ipm_load_starting_point = IPM::LoadStartingPoint (:261-316) on the device, against numpy restatements of the
reference's glue around the oracle's KKTSolverDiag (and, where oracle/_ref is built, the reference's own), on models
with every bound kind and row type; then the driver from the computed point, the failure exits, the refusals, the
column partition and one large model.

Gate of the iterate against the restatement: 1e-8 relative in the inf-norm (finite entries).  The two KKT solves stop
at a relative tolerance of 0.1 in the scaled residual, so the point is only as close to the restatement's as the two
CR runs are to each other; the measured worst case is printed (-s) and recorded in DESIGN.md."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import relerr
from ipx_amd import synth

pytestmark = pytest.mark.gpu
KEYS = ("x", "xl", "xu", "y", "zl", "zu")
E_ARGUMENT = -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-8
STATE_FREE, STATE_LB, STATE_UB, STATE_BOXED = 1, 2, 3, 4


@pytest.fixture(scope="module")
def kkt():
    from ipx_amd import kkt as k
    k.load_library()
    return k


def states_of(lb, ub):
    """Iterate::Initialize, iterate.cc:76-88"""
    fl, fu = np.isfinite(lb), np.isfinite(ub)
    st = np.full(lb.size, STATE_FREE, np.uint8)
    st[fl & ~fu] = STATE_LB
    st[~fl & fu] = STATE_UB
    st[(fl & fu) | (lb == ub)] = STATE_BOXED
    return st


def constructor_point(lb, ub, m):
    """Iterate::Iterate, iterate.cc:31-57"""
    fl, fu = np.isfinite(lb), np.isfinite(ub)
    return dict(x=np.zeros(lb.size), y=np.zeros(m), xl=np.where(fl, 1.0, np.inf), xu=np.where(fu, 1.0, np.inf),
                zl=np.where(fl, 1.0, 0.0), zu=np.where(fu, 1.0, 0.0))


def starting_point(factorize, solve, AI, b, c, lb, ub):
    """IPM::ComputeStartingPoint (ipm.cc:125-259) around a KKTSolverDiag given as factorize() / solve(a, b, tol) ->
    (x, y, iter, errflag); AI the m x (n+m) scipy matrix.  Returns (iterate, errflag, kktiter, add_c)."""
    m, N = AI.shape
    err = factorize()
    if err:
        return None, err, 0, False
    x = np.minimum(np.maximum(0.0, lb), ub)
    rb = b - AI @ x
    dx, y, it1, err = solve(np.zeros(N), rb, 0.1 * np.abs(rb).max())
    if err:
        return None, err, it1, False
    x = x + dx
    xl, xu = x - lb, ub - x
    xinfeas = max(0.0, (-xl).max(), (-xu).max())
    xl, xu = xl + (1.0 + 1.5 * xinfeas), xu + (1.0 + 1.5 * xinfeas)
    fl, fu = np.isfinite(lb), np.isfinite(ub)
    cnorm = np.sqrt(np.sum(c * c))
    add_c, it2 = False, 0
    if cnorm == 0.0:
        zl, zu = np.where(fl, 1.0, 0.0), np.where(fu, 1.0, 0.0)
    else:
        _, y, it2, err = solve(c, np.zeros(m), 0.1 * np.abs(c).max())
        if err:
            return None, err, it1 + it2, False
        z = c - AI.T @ y
        add_c = np.sqrt(np.sum(z * z)) < 0.05 * cnorm
        if add_c:
            z = z + 0.05 * c
            y = y * (1.0 - 0.05)
        zl = np.where(fl & fu, 0.5 * z, np.where(fl, z, 0.0))
        zu = np.where(fl & fu, -0.5 * z, np.where(~fl & fu, -z, 0.0))
        zinfeas = max(0.0, (-zl).max(), (-zu).max())
        zl = np.where(fl, zl + (1.0 + 1.5 * zinfeas), zl)
        zu = np.where(fu, zu + (1.0 + 1.5 * zinfeas), zu)
    xsum = 1.0 + xl[fl].sum() + xu[fu].sum()
    zsum = 1.0 + zl[fl].sum() + zu[fu].sum()
    mu = 1.0 + (xl[fl] * zl[fl]).sum() + (xu[fu] * zu[fu]).sum()
    xl, xu = xl + 0.5 * mu / zsum, xu + 0.5 * mu / zsum
    zl = np.where(fl, zl + 0.5 * mu / xsum, zl)
    zu = np.where(fu, zu + 0.5 * mu / xsum, zu)
    return dict(x=x, xl=xl, xu=xu, y=y, zl=zl, zu=zu), 0, it1 + it2, add_c


def oracle_start(oracle, A, b, c, lb, ub, maxiter=-1):
    from oracle import pyoracle as po
    import scipy.sparse as sp
    k = oracle.kkt_diag(po.Csc(A.nrow, A.ncol, A.p, A.i, A.x), maxiter=maxiter)
    AI = sp.hstack([A.to_scipy(), sp.identity(A.nrow)]).tocsr()
    return starting_point(k.factorize, lambda a, rhs, tol: k.solve(a, rhs, tol)[:4], AI, b, c, lb, ub)


def compare(got, want, info, kktiter):
    """the gates of test 1; returns the worst relative difference"""
    assert info["errflag"] == 0 and info["status_ipm"] == 0 and info["iter"] == 0
    assert abs(info["kktiter"] - kktiter) <= max(2, 0.02 * kktiter), (info["kktiter"], kktiter)
    worst = 0.0
    for key in KEYS:
        g, w = got[key], want[key]
        assert np.array_equal(np.isinf(g), np.isinf(w)), key
        if key in ("zl", "zu"):
            assert np.array_equal(g == 0.0, w == 0.0), key
        f = np.isfinite(w)
        worst = max(worst, relerr(g[f], w[f]))
    assert worst < TOL, worst
    return worst


def model(kind, m=300, n=700, seed=11):
    if kind == "dense":
        A, b, c, lb, ub, _ = synth.mixed_bounds_lp(m, n, seed, num_dense=3)
    else:
        A, b, c, lb, ub, _ = synth.mixed_bounds_lp(m, n, seed)
    if kind == "zero_obj":
        c = np.zeros_like(c)
    elif kind == "c_in_range":
        y0 = np.random.default_rng(seed).uniform(-1.0, 1.0, m)
        c = np.concatenate([A.to_scipy().T @ y0, y0])         # c = AI'y0
    return A, b, c, lb, ub


KINDS = ["mixed", "zero_obj", "c_in_range", "dense"]


# --------------------------------------------------------------------------------------
# 1. against the oracle
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_starting_point_vs_oracle(kkt, oracle, kind):
    A, b, c, lb, ub = model(kind)
    want, err, kktiter, add_c = oracle_start(oracle, A, b, c, lb, ub)
    assert err == 0
    assert add_c == (kind == "c_in_range")                   # the 0.05 c branch is taken exactly there
    ctx = kkt.KktContext(A)
    if kind == "dense":
        assert ctx.num_dense_cols > 0                       # Factorize(nullptr) runs the SMW preconditioner
    info = ctx.ipm_starting_point(b, c, lb, ub)
    got = ctx.iterate_get()
    worst = compare(got, want, info, kktiter)
    print("starting point %s: kktiter %d, worst relative difference %.2e" % (kind, info["kktiter"], worst))
    # the states: the driver's evaluation of the point sees the bound kinds of Iterate::Initialize
    ctx.iterate_set(got, states_of(lb, ub))
    again = ctx.iterate_objectives(b, c, lb, ub)
    assert abs(info["pobjective"] - (again[0] + again[2])) <= 1e-12 * (1 + abs(info["pobjective"]))
    r = ctx.iterate_residuals(b, c, lb, ub)
    assert info["presidual"] == r["presidual"] and info["dresidual"] == r["dresidual"]
    ctx.close()


# --------------------------------------------------------------------------------------
# 2. against the reference's own objects
# --------------------------------------------------------------------------------------
def test_starting_point_vs_reference(kkt, ref):
    from oracle import pyoracle as po
    m, n = 200, 450
    A, b, c, lb, ub, _ = synth.mixed_bounds_lp(m, n, 23)
    # the reference's Model from user form: rows A x (<, >, =) rhs, bounds on the structurals
    constr = "".join("<" if np.isinf(ub[n + i]) else ">" if np.isinf(lb[n + i]) else "=" for i in range(m))
    rm = ref.model(po.Csc(m, n, A.p, A.i, A.x), b, constr, c[:n], lb[:n], ub[:n])
    assert rm.dualized == 0
    AI = rm.AI()
    bb, cc, lbb, ubb = rm.vectors()
    k = rm.kkt_diag()
    want, err, kktiter, _ = starting_point(lambda: k.factorize()[0], lambda a, rhs, tol: k.solve(a, rhs, tol), AI.to_scipy().tocsr(),
                                           bb, cc, lbb, ubb)
    assert err == 0
    # the device gets exactly the model the reference built
    ns, nz = rm.n, int(AI.p[rm.n])
    ctx = kkt.KktContext(synth.CscMatrix(rm.m, ns, AI.p[:ns + 1].copy(), AI.i[:nz].copy(), AI.x[:nz].copy()))
    info = ctx.ipm_starting_point(bb, cc, lbb, ubb)
    got = ctx.iterate_get()
    compare(got, want, info, kktiter)
    ri = rm.iterate()
    ri.initialize(got)
    assert np.array_equal(ri.states(), states_of(lbb, ubb))
    ctx.close()


# --------------------------------------------------------------------------------------
# 3. determinism
# --------------------------------------------------------------------------------------
def test_starting_point_bit_identical(kkt):
    A, b, c, lb, ub = model("mixed", 2000, 4500, 5)
    ctx = kkt.KktContext(A)
    i1 = ctx.ipm_starting_point(b, c, lb, ub)
    p1 = ctx.iterate_get()
    i2 = ctx.ipm_starting_point(b, c, lb, ub)
    p2 = ctx.iterate_get()
    assert i1 == i2
    for key in KEYS:
        assert np.array_equal(p1[key], p2[key]), key
    ctx.close()


# --------------------------------------------------------------------------------------
# 4. to optimality from the computed point
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,m,n,free", [(31, 120, 260, True), (32, 300, 640, True), (33, 300, 640, False)])
def test_driver_from_starting_point(kkt, oracle, seed, m, n, free):
    from scipy.optimize import linprog
    import scipy.sparse as sp
    from oracle import pyoracle as po
    A, b, c, lb, ub, _ = synth.mixed_bounds_lp(m, n, seed, free=free)
    S = A.to_scipy()
    r = linprog(c, A_eq=sp.hstack([S, sp.identity(m)]), b_eq=b, bounds=list(zip(lb, ub)), method="highs")
    assert r.status == 0
    ctx = kkt.KktContext(A)
    assert ctx.ipm_starting_point(b, c, lb, ub)["status_ipm"] == 0
    start = ctx.iterate_get()
    ig = ctx.ipm_driver(b, c, lb, ub, kkt_maxiter=5000, ipm_maxiter=100)
    assert ig["status_ipm"] == 1, ig
    assert abs(ig["pobjective"] - r.fun) <= 1e-6 * (1.0 + abs(r.fun)), (ig["pobjective"], r.fun)
    # the oracle's driver from its own start.  At the reference's kkt_tol = 0.3 the CR loops stop early enough that
    # starting points equal to 1e-14 take paths up to two iterations apart (measured: 18 against 20)
    k = oracle.kkt_diag(po.Csc(m, n, A.p, A.i, A.x), maxiter=5000)
    own, err, _, _ = oracle_start(oracle, A, b, c, lb, ub)
    assert err == 0
    _, io = k.ipm_driver(states_of(lb, ub), b, c, lb, ub, own, ipm_maxiter=100)
    assert io["status_ipm"] == 1 and abs(ig["iter"] - io["iter"]) <= 2, (ig, io)
    for key in ("pobjective", "dobjective"):
        assert abs(ig[key] - io[key]) <= 1e-6 * (1.0 + abs(io[key])), key
    if not free:                                            # the switch to the basis solver
        ctx.iterate_set(start, states_of(lb, ub))
        first = ctx.ipm_driver(b, c, lb, ub, kkt_maxiter=5000, ipm_maxiter=4)
        assert first["status_ipm"] == 6
        second = ctx.ipm_driver_basis(b, c, lb, ub, ipm_maxiter=100)
        assert second["status_ipm"] == 1, second
        assert abs(second["pobjective"] - r.fun) <= 1e-6 * (1.0 + abs(r.fun))
    ctx.close()


# --------------------------------------------------------------------------------------
# 5. failure exits
# --------------------------------------------------------------------------------------
def assert_constructor_point(ctx, lb, ub, m):
    got, want = ctx.iterate_get(), constructor_point(lb, ub, m)
    for key in KEYS:
        assert np.array_equal(got[key], want[key]), key


def test_starting_point_failures(kkt):
    m, n = 400, 900
    A, b, c, lb, ub = model("mixed", m, n, 17)
    ctx = kkt.KktContext(A)
    ok = ctx.ipm_starting_point(b, c, lb, ub)
    assert ok["status_ipm"] == 0 and ok["kktiter"] > 10          # a solve runs more than 5 CR iterations
    calls = [0]

    def interrupt():
        calls[0] += 1
        return 999

    info = ctx.ipm_starting_point(b, c, lb, ub, interrupt=interrupt)
    assert calls[0] > 0 and info["status_ipm"] == 5 and info["errflag"] == 0, info
    assert_constructor_point(ctx, lb, ub, m)
    assert ctx.ipm_starting_point(b, c, lb, ub)["status_ipm"] == 0
    info = ctx.ipm_starting_point(b, c, lb, ub, kkt_maxiter=1)
    assert info["status_ipm"] == 8 and info["errflag"] == 201 and info["kktiter"] == 1, info
    assert_constructor_point(ctx, lb, ub, m)
    ctx.close()


# --------------------------------------------------------------------------------------
# 6. refusals
# --------------------------------------------------------------------------------------
def test_starting_point_refusals(kkt, monkeypatch):
    from ipx_amd import partition
    m, n = 200, 450
    A, b, c, lb, ub = model("mixed", m, n, 19)
    ctx = kkt.KktContext(A)
    bad = []
    j = int(np.flatnonzero(np.isfinite(ub[:n]))[0])
    lb2 = lb.copy(); lb2[j] = ub[j] + 1.0; bad.append((b, c, lb2, ub))
    lb3 = lb.copy(); lb3[n + 3] = np.inf; bad.append((b, c, lb3, ub))
    ub4 = ub.copy(); ub4[5] = -np.inf; bad.append((b, c, lb, ub4))
    c5 = c.copy(); c5[11] = np.nan; bad.append((b, c5, lb, ub))
    b6 = b.copy(); b6[2] = np.nan; bad.append((b6, c, lb, ub))
    bad.append((None, c, lb, ub))
    bad.append((b, c, None, ub))
    for args in bad:
        with pytest.raises(kkt.KktError) as e:
            ctx.ipm_starting_point(*args)
        assert e.value.code == E_ARGUMENT
    assert ctx.ipm_starting_point(b, c, lb, ub)["status_ipm"] == 0      # the context stays usable
    ctx.close()
    monkeypatch.setenv("IPXK_FORCE_COMM", "1")
    monkeypatch.setenv("IPXK_COMM", "direct")
    rows = kkt.KktContext(partition.slab_matrix(A, 0, m))
    rows.comm_init(rows.comm_unique_id(), 0, 1, columns=False)
    for call in (lambda: rows.ipm_starting_point(b, c, lb, ub),):
        with pytest.raises(kkt.KktError) as e:
            call()
        assert e.value.code == E_ARGUMENT and "ipxk_comm_init_columns" in str(e.value)
    rows.close()


# --------------------------------------------------------------------------------------
# 7. column partition
# --------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("transport", ["rccl", "direct"])
@pytest.mark.parametrize("kind", ["mixed", "zero_obj", "c_in_range"])
def test_starting_point_single_rank(kkt, monkeypatch, transport, kind):
    """One rank through the collective code path.  The KKT solves of a column-partitioned context assemble their
    right-hand side and recover x in another order than the unpartitioned context's (kkt_diag.hip), so the point agrees
    to the gate of test 1 and the CR iterations exactly, not bit for bit; the elementwise passes and reductions around
    the solves are bit for bit (ipxk_ipm_load_starting_point below, which has no solve)."""
    A, b, c, lb, ub = model(kind, 300, 640, 41)

    def run(ctx):
        info = ctx.ipm_starting_point(b, c, lb, ub)
        it = ctx.iterate_get()
        ctx.close()
        return info, it

    ref_info, ref_it = run(kkt.KktContext(A))
    info, it = run(forced_context(kkt, A, transport, monkeypatch))
    assert info["status_ipm"] == ref_info["status_ipm"] == 0 and info["kktiter"] == ref_info["kktiter"]
    for key in ("presidual", "dresidual", "complementarity", "mu", "pobjective", "dobjective"):
        assert abs(info[key] - ref_info[key]) <= TOL * abs(ref_info[key]), key
    for key in KEYS:
        f = np.isfinite(ref_it[key])
        assert np.array_equal(np.isfinite(it[key]), f) and relerr(it[key][f], ref_it[key][f]) < TOL, key


def run_ranks(tmp_path, world, model_path, mode, timeout):
    env = dict(os.environ, IPXK_COMM="direct")
    env.pop("IPXK_FORCE_COMM", None)
    idfile, out = str(tmp_path / ("uid_" + mode)), str(tmp_path / ("res_" + mode))
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "multirank_start_worker.py"), str(r),
                               str(world), idfile, out, model_path, mode], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs, failed = [], False
    for p in procs:
        try:
            logs.append(p.communicate(timeout=timeout)[0])
        except subprocess.TimeoutExpired:
            failed = True
            break
        if p.returncode != 0:
            failed = True
            break
    if failed:
        for q in procs:
            q.kill()
        for q in procs:
            q.wait()
        pytest.fail("a rank failed or did not finish:\n" + "\n".join(logs))
    return [np.load(out + ".rank%d.npz" % r) for r in range(world)]


@pytest.mark.parametrize("world,case", [(2, "plain"), (3, "plain"), (3, "at_bound")])
def test_starting_point_partitioned_multiprocess(kkt, tmp_path, world, case):
    from ipx_amd import partition
    m, n = 300, 640
    tail = n - partition.row_range(n, world - 1, world)[0] if case == "at_bound" else 0     # the last rank's columns
    A, b, c, lb, ub, _ = synth.mixed_bounds_lp(m, n, 61, tail=tail)
    path = str(tmp_path / "model.npz")
    np.savez(path, m=m, n=n, Ap=A.p, Ai=A.i, Ax=A.x, b=b, c=c, lb=lb, ub=ub)
    ctx = kkt.KktContext(A)
    ref_info = ctx.ipm_starting_point(b, c, lb, ub)
    ref_it = ctx.iterate_get()
    ref_drv = ctx.ipm_driver(b, c, lb, ub, kkt_maxiter=5000, ipm_maxiter=100)
    ctx.close()
    assert ref_drv["status_ipm"] == (1 if case == "plain" else ref_drv["status_ipm"])
    res = run_ranks(tmp_path, world, path, "start", timeout=300)
    parts = [{k: r["it_" + k] for k in KEYS} for r in res]
    got = partition.assemble_iterate(m, parts)
    for key in KEYS:
        f = np.isfinite(ref_it[key])
        assert np.array_equal(np.isfinite(got[key]), f), key
        assert relerr(got[key][f], ref_it[key][f]) < TOL, key
    for r in res[1:]:
        assert np.array_equal(r["info"], res[0]["info"]) and np.array_equal(r["drv"], res[0]["drv"])
        assert np.array_equal(r["it_y"], res[0]["it_y"])
        for key in ("x", "xl", "xu", "zl", "zu"):
            assert np.array_equal(r["it_" + key][-m:], res[0]["it_" + key][-m:]), key
    status, _, _, pobj = res[0]["drv"]
    assert int(status) == ref_drv["status_ipm"]       # at_bound: the diag solver's CR cap ends both (IPX_STATUS_failed)
    if int(status) == 1:
        assert abs(pobj - ref_drv["pobjective"]) <= 1e-6 * (1.0 + abs(ref_drv["pobjective"]))


def test_starting_point_mismatched_b_fails_together(tmp_path):
    m, n = 300, 640
    A, b, c, lb, ub, _ = synth.mixed_bounds_lp(m, n, 62)
    path = str(tmp_path / "model.npz")
    np.savez(path, m=m, n=n, Ap=A.p, Ai=A.i, Ax=A.x, b=b, c=c, lb=lb, ub=ub)
    res = run_ranks(tmp_path, 2, path, "mismatch_b", timeout=120)
    assert [int(r["code"]) for r in res] == [E_ARGUMENT, E_ARGUMENT]
    assert all(float(r["t"]) < 30.0 for r in res)


# --------------------------------------------------------------------------------------
# 8. ipxk_ipm_load_starting_point
# --------------------------------------------------------------------------------------
def load_point(it, lb, ub):
    """IPM::LoadStartingPoint, ipm.cc:261-316"""
    out = {k: np.array(v, dtype=float) for k, v in it.items()}
    prods = [out["xl"] * out["zl"], out["xu"] * out["zu"]]
    masks = [(out["xl"] > 0) & (out["zl"] > 0), (out["xu"] > 0) & (out["zu"] > 0)]
    cnt = sum(int(k.sum()) for k in masks)
    mu = sum(p[k].sum() for p, k in zip(prods, masks)) / cnt if cnt else 1.0
    for x, z, bound in (("xl", "zl", lb), ("xu", "zu", ub)):
        X, Z = out[x], out[z]
        f = np.isfinite(bound)
        both, x0, z0 = f & (X == 0) & (Z == 0), f & (X == 0) & (Z != 0), f & (X != 0) & (Z == 0)
        X[both] = Z[both] = np.sqrt(mu)
        X[x0] = mu / Z[x0]
        Z[z0] = mu / X[z0]
    return out


def loadable(lb, ub, m, seed, zeros=True, positive=True):
    rng = np.random.default_rng(seed)
    N = lb.size
    fl, fu = np.isfinite(lb), np.isfinite(ub)
    it = dict(x=rng.uniform(-1, 1, N), y=rng.uniform(-1, 1, m))
    for x, z, f in (("xl", "zl", fl), ("xu", "zu", fu)):
        X = np.where(f, rng.uniform(0.5, 2.0, N) if positive else 0.0, np.inf)
        Z = np.where(f, rng.uniform(0.5, 2.0, N) if positive else 0.0, 0.0)
        if zeros:
            pick = rng.integers(0, 4, N)
            X[f & (pick == 1)] = 0.0
            Z[f & (pick == 2)] = 0.0
            X[f & (pick == 3)] = 0.0
            Z[f & (pick == 3)] = 0.0
        it[x], it[z] = X, Z
    return it


def test_load_starting_point(kkt, monkeypatch):
    m, n = 300, 640
    A, b, c, lb, ub = model("mixed", m, n, 71)
    ctx = kkt.KktContext(A)
    for positive in (True, False):                                # False: no positive pair, mu = 1
        it = loadable(lb, ub, m, 3, positive=positive)
        want = load_point(it, lb, ub)
        ctx.ipm_load_starting_point(it, lb, ub)
        got = ctx.iterate_get()
        for key in KEYS:
            assert np.array_equal(np.isinf(got[key]), np.isinf(want[key])), key
            f = np.isfinite(want[key])
            assert relerr(got[key][f], want[key][f]) < 1e-13, key
    fl = np.isfinite(lb)
    assert np.all(got["xl"][fl] == 1.0) and np.all(got["zl"][fl] == 1.0)        # sqrt(1) everywhere
    # every invalid pattern is refused, with the index
    it = loadable(lb, ub, m, 4)
    fl, fu = np.isfinite(lb), np.isfinite(ub)
    j_fin, j_inf = int(np.flatnonzero(fl)[3]), int(np.flatnonzero(~fl)[0])
    j_ufin = int(np.flatnonzero(fu)[2])
    cases = [("xl", j_fin, -1.0), ("xl", j_fin, np.inf), ("zl", j_fin, -0.5), ("zl", j_fin, np.nan),
             ("xl", j_inf, 1.0), ("zl", j_inf, 1.0), ("xu", j_ufin, -1.0), ("zu", j_ufin, np.inf)]
    for key, j, v in cases:
        bad = {k: a.copy() for k, a in it.items()}
        bad[key][j] = v
        with pytest.raises(kkt.KktError) as e:
            ctx.ipm_load_starting_point(bad, lb, ub)
        assert e.value.code == E_ARGUMENT and str(j) in str(e.value), (key, j)
    # one forced column rank loads the same bits; the driver reaches the optimum from a loaded point
    ctx.ipm_load_starting_point(it, lb, ub)
    loaded = ctx.iterate_get()
    assert ctx.ipm_driver(b, c, lb, ub, kkt_maxiter=5000, ipm_maxiter=100)["status_ipm"] == 1
    ctx.close()
    fc = forced_context(kkt, A, "direct", monkeypatch)
    fc.ipm_load_starting_point(it, lb, ub)
    other = fc.iterate_get()
    for key in KEYS:
        assert np.array_equal(other[key], loaded[key]), key
    assert fc.ipm_driver(b, c, lb, ub, kkt_maxiter=5000, ipm_maxiter=100)["status_ipm"] == 1
    fc.close()


# --------------------------------------------------------------------------------------
# 9. size
# --------------------------------------------------------------------------------------
def test_starting_point_size(kkt):
    import time
    m, n = 200000, 400000
    A, b, c, lb, ub, _ = synth.mixed_bounds_lp(m, n, 91)
    ctx = kkt.KktContext(A)
    ctx.ipm_starting_point(b, c, lb, ub)                          # warm-up
    t = time.perf_counter()
    info = ctx.ipm_starting_point(b, c, lb, ub)
    dt = time.perf_counter() - t
    it = ctx.iterate_get()
    assert info["errflag"] == 0 and info["status_ipm"] == 0
    for key in KEYS:
        assert not np.isnan(it[key]).any(), key
    fl, fu = np.isfinite(lb), np.isfinite(ub)
    assert np.all(np.isfinite(it["x"])) and np.all(np.isfinite(it["y"]))
    assert np.all(it["xl"][fl] * it["zl"][fl] > 0) and np.all(it["xu"][fu] * it["zu"][fu] > 0)
    print("starting point %d x %d: %.1f ms, %d CR iterations" % (m, n, dt * 1e3, info["kktiter"]))
    ctx.close()
