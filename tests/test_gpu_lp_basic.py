"""GPU: basic solutions in user form -- ipxk_lp_postsolve_basic, ipxk_lp_evaluate_basic, ipxk_lp_crossover,
ipxk_lp_get_basic_solution, ipxk_lp_get_basis (ipx_amd/csrc/user_model.hip).

(a) ipxk_lp_postsolve_basic equals tests/lp_basic_reference.py (held to something other than itself by
    tests/test_lp_basic_reference.py) entry for entry on planted points and planted valid statuses, in both pointer modes
    and with every output NULL in turn.
(b) The reductions of EvaluateBasicPoint past one grid pass: maxima planted in the last 337 entries and in entry 0, tied
    across lanes, wavefronts and workgroups, come out exactly; objval within the bound worked out at objval_bound; two
    calls give the same bits.
(c) Refusals; an interrupted crossover.  (d) num_constr == 0.
(e) solve, crossover, the vertex: three models on the device alone.
(f) The same three models through the reference's own LpSolver, where that program has been built.
(g) The ctypes mirror of ipxk_lp_basic_eval; the example program prints the known vertex and a consistent basis.

Seeds of (e) / (f).  Tried with crossover_start = 1e-8 on the device (MI355X): see SEEDS below; every seed listed ended
status_ipm 1 and status_crossover 1 at the first attempt, none was replaced.
"""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import lp_basic_reference as lbr
import test_gpu_user_model as um
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

INF = np.inf
EPS = np.finfo(np.float64).eps
E_ARGUMENT = -3
KEYS = ("x", "slack", "y", "z", "cbasis", "vbasis")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (e), (f): name -> (how it is built, the seed, how it ended on the device with crossover_start = 1e-8)
SEEDS = {"primal": 11,        # make_lp(130, 300, 11): status_ipm 1, status_crossover 1
         "dualized": 12,      # make_lp(400, 90, 12, eq_every=10, unsorted=True): 1, 1
         "duplicates": 11}    # the first with 20 columns appended again: 1, 1


def with_duplicate_columns(M, cols):
    """M with the columns `cols` appended again (same entries, obj and bounds): the optimum is not unique"""
    A = M["A"]
    parts = [(A.i[A.p[j]:A.p[j + 1]], A.x[A.p[j]:A.p[j + 1]]) for j in cols]
    Ap = np.concatenate([A.p, A.p[-1] + np.cumsum([len(r) for r, _ in parts])]).astype(np.int64)
    Ai = np.concatenate([A.i] + [r for r, _ in parts]).astype(np.int64)
    Ax = np.concatenate([A.x] + [v for _, v in parts])
    out = dict(M)
    out.update(A=po.Csc(A.nrow, A.ncol + len(cols), Ap, Ai, Ax), nv=M["nv"] + len(cols))
    for k in ("obj", "lb", "ub"):
        out[k] = np.concatenate([M[k], M[k][cols]])
    return out


CASES = {"primal": lambda: um.make_lp(130, 300, SEEDS["primal"]),
         "dualized": lambda: um.make_lp(400, 90, SEEDS["dualized"], eq_every=10, unsorted=True),
         "duplicates": lambda: with_duplicate_columns(um.make_lp(130, 300, SEEDS["duplicates"]), np.arange(10, 30))}
_models = {}


def model(name):
    if name not in _models:
        _models[name] = CASES[name]()
    return _models[name]


def assert_point_equal(got, want, keys=KEYS):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k


# ---- (a) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1, 0])
@pytest.mark.parametrize("name", ["primal", "dualized"])
def test_postsolve_basic_equals_restatement(name, scale):
    M = model(name)
    S = um.np_presolve(M, scale=scale)
    lp = um.new_lp(M, scale=scale)
    assert lp.info["dualized"] == S["dualized"] == int(name == "dualized") and (lp.info["scale_rounds"] >= 2) == bool(scale)
    n, N = S["n"], S["n"] + S["m"]
    rng = np.random.default_rng(41)
    x, y, z = rng.normal(size=N), rng.normal(size=S["m"]), rng.normal(size=N)
    ub_state = {}
    for device in (False, True):
        lp.context.set_pointer_mode(device)
        for phase in (0, 1):
            st = lbr.planted_statuses(M, S, 42, phase)
            assert set(st[:n]) == {0, -1, -2, -3} and set(st[n:]) == {0, -1, -2}
            want = lbr.postsolve_basic(M, S, x, y, z, st)
            assert_point_equal(lp.postsolve_basic(x, y, z, st), want)
            ub_state[phase] = want["vbasis"] == -2
        for k in KEYS:                               # every output NULL in turn (st, want: phase 1)
            rest = [q for q in KEYS if q != k]
            got = lp.postsolve_basic(x, y, z, st, want=rest)
            assert k not in got
            assert_point_equal(got, want, rest)
    if S["dualized"]:                                # every boxed and every flipped variable in both states
        assert S["boxed"].size > 2 and S["flipped"].size > 2
        assert (ub_state[0][S["boxed"]] != ub_state[1][S["boxed"]]).all() and (ub_state[0][S["flipped"]] != ub_state[1][S["flipped"]]).all()
    lp.context.set_pointer_mode(False)
    lp.close()


# ---- (b) ---------------------------------------------------------------------------------------------------------------------
BIG = 1024 * 256 + 337
KIND_LB, KIND_UB, KIND_BOXED, KIND_FIXED, KIND_FREE = range(5)


def big_model(rows_big):
    """one entry per column (rows_big: per row) in 64 rows (columns); bounds are multiples of 1/4, so that the planted
    violations are exact differences; obj has three dominating entries, in entry 0 and in the last 337"""
    nc, nv = (BIG, 64) if rows_big else (64, BIG)
    rng = np.random.default_rng(43)
    if rows_big:
        Ai = np.argsort(np.arange(nc) % 64, kind="stable").astype(np.int64)    # column j: rows j, j + 64, ...
        Ap = np.concatenate([[0], np.cumsum(np.bincount(np.arange(nc) % 64, minlength=64))]).astype(np.int64)
    else:
        Ap, Ai = np.arange(nv + 1, dtype=np.int64), (np.arange(nv) % 64).astype(np.int64)
    kind = np.arange(nv) % 5
    base = rng.integers(-8, 9, nv) / 4.0
    lb = np.where((kind == KIND_UB) | (kind == KIND_FREE), -INF, base)
    ub = np.where((kind == KIND_LB) | (kind == KIND_FREE), INF, np.where(kind == KIND_FIXED, base, base + 1.0))
    obj = rng.uniform(-1.0, 1.0, nv)
    for j in ((0, nv - 1) if rows_big else (0, nv - 300, nv - 1)):
        obj[j] = 1.5 * 2.0 ** 20
    ct = "".join("<>="[i % 3] for i in range(nc))
    return dict(A=po.Csc(nc, nv, Ap, Ai, np.ones(Ai.size)), rhs=np.zeros(nc), ct=ct, obj=obj, lb=lb, ub=ub, nc=nc, nv=nv, kind=kind)


def objval_bound(nterms):
    """Every operation of the sum rounds by at most u = EPS / 2 of a partial sum, which is at most sum|terms|.  A term passes
    through: its product; at most ceil(nterms / (1024 * 256)) additions in its thread's chain; 6 levels of the wavefront tree
    and 3 additions over the wavefronts; in the finishing workgroup at most 1024 / 256 = 4 additions in a thread's chain, 6
    levels and 3 additions again.  k u sum|terms| with that k bounds the error to first order; the test allows k EPS."""
    return math.ceil(nterms / (1024 * 256)) + 1 + 6 + 3 + 4 + 6 + 3


@pytest.mark.parametrize("rows_big", [False, True])
def test_evaluate_basic_past_one_grid_pass(rows_big):
    M = big_model(rows_big)
    nc, nv, kind, lb, ub = M["nc"], M["nv"], M["kind"], M["lb"], M["ub"]
    lp = um.new_lp(M, dualize=1 if rows_big else 0)
    assert lp.info["dualized"] == int(rows_big)
    rng = np.random.default_rng(44)
    ct = np.array(list(M["ct"]))
    # a feasible point with every sign right ...
    vb = rng.integers(-3, 1, nv)
    vb[(vb == -1) & ~np.isfinite(lb)] = -3
    vb[(vb == -2) & ~np.isfinite(ub)] = -3
    x = np.where(np.isfinite(lb), lb + 0.25 * (kind != KIND_FIXED), np.where(np.isfinite(ub), ub - 0.25, 0.5))
    z = np.where(vb == -1, rng.uniform(0.5, 2.0, nv), np.where(vb == -2, -rng.uniform(0.5, 2.0, nv), 0.0))
    slack = np.where(ct == "<", 1.0, np.where(ct == ">", -1.0, 0.0)) * rng.uniform(0.5, 2.0, nc)
    y = np.where(ct == "<", -1.0, np.where(ct == ">", 1.0, 0.0)) * rng.uniform(0.5, 2.0, nc)
    # ... small violations all over, and the largest ones tied in entry 0, across lanes (1), wavefronts (64), workgroups (256,
    # 256 * 7 + 5), in the second grid pass (1024 * 256 + 2) and in the last 337 entries; in the variables or in the rows,
    # whichever loop is the long one
    big = nv if not rows_big else nc
    where = np.array([0, 1, 64, 256, 256 * 7 + 5, 1024 * 256 + 2, big - 337, big - 1])
    some = rng.choice(big, 5000, replace=False)
    P, D = 3.5, 7.25
    if not rows_big:
        some, where = some[kind[some] != KIND_FREE], where + (kind[where] == KIND_FREE)     # (a free variable violates no bound)
        assert (kind[where] != KIND_FREE).all()
        x[some] = np.where(np.isfinite(lb[some]), lb[some] - 1.25, ub[some] + 1.25)
        vb[some], z[some] = 0, rng.choice([-2.5, 2.5], some.size)
        x[where] = np.where(np.isfinite(lb[where]), lb[where] - P, ub[where] + P)
        vb[where], z[where] = 0, np.where(np.arange(where.size) % 2 == 0, D, -D)
    else:
        some, where = some[ct[some] != "="], where + (ct[where] == "=")                     # (an equality row's y has no sign)
        assert (ct[where] != "=").all()
        slack[some] *= -0.5
        y[some] *= -0.5
        slack[where] = np.where(ct[where] == "<", -P, P)
        y[where] = np.where(ct[where] == "<", D, -D)
    u = dict(x=x, slack=slack, y=y, z=z, vbasis=vb)
    pinf, dinf, objval, mag = lbr.evaluate_basic(M, u)
    assert (pinf, dinf) == (P, D)                   # (the restatement sees the planted maxima)
    if not rows_big:                                # (obj'x is dominated by entry 0 and two of the last 337)
        assert np.abs(M["obj"] * x)[[0, nv - 300, nv - 1]].sum() > 0.9 * mag
    ev, ev2 = lp.evaluate_basic(u), lp.evaluate_basic(u)
    lp.close()
    print("primal_infeas %r dual_infeas %r objval %r (fsum %r), |difference| / (EPS sum|terms|) = %.3g, allowed %d"
          % (ev["primal_infeas"], ev["dual_infeas"], ev["objval"], objval, abs(ev["objval"] - objval) / (EPS * mag), objval_bound(nv)))
    assert ev == ev2                                # the same bits
    assert ev["primal_infeas"] == P and ev["dual_infeas"] == D
    assert abs(ev["objval"] - objval) <= objval_bound(nv) * EPS * mag


# ---- (c) ---------------------------------------------------------------------------------------------------------------------
def refused(kkt, match, call, *args, **kw):
    with pytest.raises(kkt.KktError, match=match) as e:
        call(*args, **kw)
    assert e.value.code == E_ARGUMENT


def test_refusals(monkeypatch):
    from ipx_amd import kkt
    for name in ("primal", "dualized"):
        M = model(name)
        S = um.np_presolve(M)
        lp = um.new_lp(M)
        n, N = S["n"], S["n"] + S["m"]
        v = np.zeros(N)
        st = lbr.planted_statuses(M, S, 45)
        bad = st.copy()
        bad[[n + 17, n + 60]] = -3
        refused(kkt, "slack 17", lp.postsolve_basic, v, v[:S["m"]], v, bad)
        if S["dualized"]:
            nc = n - S["boxed"].size
            bad = st.copy()
            bad[[nc + 3, n + S["boxed"][3]]] = 0
            refused(kkt, "number 3", lp.postsolve_basic, v, v[:S["m"]], v, bad)
        refused(kkt, "no solve", lp.crossover)
        refused(kkt, "no basic solution", lp.basic_solution)
        refused(kkt, "no basis", lp.basis)
        # a solve that ends neither optimal nor imprecise: crossover does not run
        info = lp.solve(ipm_maxiter=1, crossover_start=1e-8)
        assert info["status_ipm"] not in (1, 2), info
        cinfo, ev = lp.crossover()
        assert cinfo["status_crossover"] == 0 and cinfo["errflag"] == 0 and ev == dict(primal_infeas=0.0, dual_infeas=0.0, objval=0.0)
        refused(kkt, "no basic solution", lp.basic_solution)
        lp.close()
    # a partitioned context
    monkeypatch.setenv("IPXK_FORCE_COMM", "1")
    monkeypatch.setenv("IPXK_COMM", "direct")
    lp = um.new_lp(model("primal"))
    lp.context.comm_init(lp.context.comm_unique_id(), 0, 1, columns=True)
    refused(kkt, "does not run on a partitioned system", lp.crossover)
    lp.close()


# ---- (d) ---------------------------------------------------------------------------------------------------------------------
def test_postsolve_basic_without_constraints():
    M = um.model("e")
    assert M["nc"] == 0
    S = um.np_presolve(M)
    lp = um.new_lp(M)
    rng = np.random.default_rng(46)
    x, y, z = rng.normal(size=S["n"]), np.zeros(0), rng.normal(size=S["n"])
    st = lbr.planted_statuses(M, S, 47)
    st[(st == -1) & np.isinf(M["lb"])] = -3         # (a variable sits on finite bounds only: the evaluation below has no inf - inf)
    st[(st == -2) & np.isinf(M["ub"])] = -3
    assert S["m"] == 0 and set(st) == {0, -1, -2, -3}
    want = lbr.postsolve_basic(M, S, x, y, z, st)
    got = lp.postsolve_basic(x, y, z, st)
    assert_point_equal(got, want)
    assert got["slack"].size == got["y"].size == got["cbasis"].size == 0
    u = dict(got)
    ev = lp.evaluate_basic(u)
    pinf, dinf, objval, mag = lbr.evaluate_basic(M, u)
    assert (ev["primal_infeas"], ev["dual_infeas"]) == (pinf, dinf) and abs(ev["objval"] - objval) <= objval_bound(M["nv"]) * EPS * mag
    from ipx_amd import kkt
    refused(kkt, "no constraints", lp.crossover)    # (what the header says the call does without constraints)
    lp.close()


# ---- (e) ---------------------------------------------------------------------------------------------------------------------
_runs = {}


def run_on_device(name):
    """solve, basis(), crossover(), basic_solution() of a case, once for the tests that look at it"""
    if name not in _runs:
        lp = um.new_lp(model(name))
        info = lp.solve(crossover_start=1e-8)        # what solve(crossover=True) does, with basis() in between
        info["pobjval"] = lp.evaluate()["pobjval"]   # of the interior solution, in user form
        early = lp.basis()
        cinfo, ev = lp.crossover()
        _runs[name] = dict(info=info, early=early, cinfo=cinfo, ev=ev, u=lp.basic_solution() if cinfo["status_crossover"] in (1, 2) else None,
                           basis=lp.basis() if cinfo["status_crossover"] in (1, 2) else None, dualized=lp.info["dualized"])
        lp.close()
    return _runs[name]


@pytest.mark.parametrize("name", ["primal", "dualized", "duplicates"])
def test_vertex_end_to_end(name):
    M = model(name)
    nc, nv, A = M["nc"], M["nv"], M["A"]
    R = run_on_device(name)
    info, cinfo, ev, u = R["info"], R["cinfo"], R["ev"], R["u"]
    print(name, "pushes: dual %d (pivots %d), primal %d (pivots %d); superbasics %d / %d; vertex in solver form: infeasibilities %.2e / %.2e"
          % (cinfo["dual_pushes"], cinfo["dual_pivots"], cinfo["primal_pushes"], cinfo["primal_pivots"], cinfo["dual_superbasics"],
             cinfo["primal_superbasics"], cinfo["primal_infeas"], cinfo["dual_infeas"]))
    assert info["status_ipm"] == 1 and cinfo["status_crossover"] == 1, (info, cinfo)
    assert R["dualized"] == int(name == "dualized")
    cb, vb = u["cbasis"], u["vbasis"]
    assert set(cb) <= {0, -1} and set(vb) <= {0, -1, -2, -3}
    assert np.array_equal(u["x"][vb == -1], M["lb"][vb == -1]) and np.array_equal(u["x"][vb == -2], M["ub"][vb == -2])
    assert (u["z"][vb == 0] == 0.0).all() and (u["slack"][cb == -1] == 0.0).all() and (u["y"][cb == 0] == 0.0).all()
    assert (vb == 0).sum() + (cb == 0).sum() == nc
    for got, want in zip(R["basis"], (cb, vb)):     # GetBasis after crossover: the vertex's statuses
        assert np.array_equal(got, want)
    ecb, evb = R["early"]                            # GetBasis before crossover: the IPM's basis
    assert (evb == 0).sum() + (ecb == 0).sum() == nc and set(ecb) <= {0, -1} and set(evb) <= {0, -1, -2, -3}
    assert ev["primal_infeas"] <= 1e-7 and ev["dual_infeas"] <= 1e-7, ev
    pinf, dinf, objval, mag = lbr.evaluate_basic(M, u)
    assert (ev["primal_infeas"], ev["dual_infeas"]) == (pinf, dinf) and abs(ev["objval"] - objval) <= objval_bound(nv) * EPS * mag
    assert abs(ev["objval"] - info["pobjval"]) <= 1e-6 * (1.0 + abs(ev["objval"])), (ev, info["pobjval"])
    # residuals of the vertex in user form, in extended precision
    L = np.longdouble
    colof = np.repeat(np.arange(nv), np.diff(A.p))
    rb = M["rhs"].astype(L) - u["slack"].astype(L)
    np.subtract.at(rb, A.i, A.x.astype(L) * u["x"].astype(L)[colof])
    rc = M["obj"].astype(L) - u["z"].astype(L)
    np.subtract.at(rc, colof, A.x.astype(L) * u["y"].astype(L)[A.i])
    bounds = np.concatenate([M["lb"][np.isfinite(M["lb"])], M["ub"][np.isfinite(M["ub"])]])
    norm_p, norm_d = max(np.abs(M["rhs"]).max(), np.abs(bounds).max()), np.abs(M["obj"]).max()
    print(name, "user-form residuals of the vertex: primal %.2e / (1 + %.3g), dual %.2e / (1 + %.3g); objval %.12g, interior pobjval %.12g"
          % (float(np.abs(rb).max()), norm_p, float(np.abs(rc).max()), norm_d, ev["objval"], info["pobjval"]))
    assert np.abs(rb).max() <= 1e-9 * (1.0 + norm_p) and np.abs(rc).max() <= 1e-9 * (1.0 + norm_d)
    if name == "duplicates":
        assert cinfo["primal_pushes"] + cinfo["dual_pushes"] >= 1, cinfo


def test_crossover_interrupted():
    """an interrupt at the first candidate: status 5 (time limit), errflag 0, no basic solution; nothing has been pushed, so a
    second call without the interrupt still ends optimal"""
    from ipx_amd import kkt
    lp = um.new_lp(model("duplicates"))
    assert lp.solve(crossover_start=1e-8)["status_ipm"] == 1
    cinfo, ev = lp.crossover(interrupt=lambda: 999)
    assert (cinfo["status_crossover"], cinfo["errflag"]) == (5, 0) and ev == dict(primal_infeas=0.0, dual_infeas=0.0, objval=0.0), cinfo
    refused(kkt, "no basic solution", lp.basic_solution)
    cb, vb = lp.basis()
    assert (vb == 0).sum() + (cb == 0).sum() == lp.num_constr
    cinfo, ev = lp.crossover()
    assert cinfo["status_crossover"] == 1 and ev["primal_infeas"] <= 1e-7 and ev["dual_infeas"] <= 1e-7, (cinfo, ev)
    lp.basic_solution()
    lp.solve()                                       # a new solve clears the vertex
    refused(kkt, "no basic solution", lp.basic_solution)
    lp.close()


def test_solve_with_the_crossover_flag():
    """solve(crossover=True) on the LP of examples/lp_user.cc: crossover_start becomes 1e-8, both records come back, and
    the vertex is the known one, x = (1.5, -0.5, 3, 1.5) (worked out in the example's head)"""
    A = po.Csc(3, 4, np.array([0, 2, 4, 5, 7]), np.array([0, 1, 0, 2, 0, 1, 2]), np.ones(7))
    M = dict(A=A, rhs=np.array([4.0, 3.0, 1.0]), ct="=<>", obj=np.array([1.0, 2.0, -1.0, 0.0]),
             lb=np.array([0.0, -INF, 0.0, -INF]), ub=np.array([INF, 5.0, 3.0, INF]))
    for dualize in (0, 1):
        lp = um.new_lp(M, dualize=dualize)
        out = lp.solve(crossover=True)
        u = lp.basic_solution()
        lp.close()
        assert out["status_ipm"] == 1 and out["crossover"]["status_crossover"] == 1, out
        assert np.abs(u["x"] - [1.5, -0.5, 3.0, 1.5]).max() <= 1e-9 and abs(out["basic_eval"]["objval"] + 2.5) <= 1e-9
        assert u["x"][2] == 3.0 and u["vbasis"].tolist() == [0, 0, -2, 0] and u["cbasis"].tolist() == [-1, -1, -1]


# ---- (f) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["primal", "dualized", "duplicates"])
def test_vertex_against_reference_solver(name, tmp_path):
    """The reference's whole LpSolver with crossover (tests/dropin/lp_main.cc) on the same model: both end optimal / optimal,
    the objectives of the two vertices agree to 1e-8 (1 + |objval|) (both are vertices of the same optimal face), and where
    the statuses are the same so is x, to 1e-9 (1 + |x|).  No seed had to be replaced."""
    import test_gpu_lp_dropin as dropin
    if not os.path.exists(dropin.REF_BIN):
        pytest.skip("oracle/_ref/test_lp_ref not built (needs the reference sources at build time)")
    M = model(name)
    A = M["A"]
    R = run_on_device(name)
    din, dout = str(tmp_path / "in"), str(tmp_path / "ref")
    dropin.write_model(din, M["obj"], M["lb"], M["ub"], A.p, A.i, A.x, M["rhs"], list(M["ct"]), crossover=1)
    ri, ra, rout = dropin.run(dropin.REF_BIN, din, dout, timeout=300)
    assert ri["status_ipm"] == 1 and ri["status_crossover"] == 1, rout
    assert R["info"]["status_ipm"] == 1 and R["cinfo"]["status_crossover"] == 1
    assert abs(R["ev"]["objval"] - ri["objval"]) <= 1e-8 * (1.0 + abs(ri["objval"])), (R["ev"], ri["objval"])
    rcb = np.fromfile(os.path.join(dout, "cbasis.bin"), np.int64)
    rvb = np.fromfile(os.path.join(dout, "vbasis.bin"), np.int64)
    same = np.array_equal(rcb, R["u"]["cbasis"]) and np.array_equal(rvb, R["u"]["vbasis"])
    print(name, "statuses equal the reference's:", same, "objval", R["ev"]["objval"], "reference", ri["objval"])
    if same:
        assert (np.abs(R["u"]["x"] - ra["bx"]) <= 1e-9 * (1.0 + np.abs(ra["bx"]))).all()


# ---- (g) ---------------------------------------------------------------------------------------------------------------------
def test_basic_eval_struct_matches_compiler(tmp_path):
    """the method of tests/test_user_model_abi.py for the new struct: field order and types from the header, size and
    offsets from the compiler"""
    import test_user_model_abi as abi
    from ipx_amd import kkt
    fields = abi.header_fields("ipxk_lp_basic_eval")
    assert [f for _, f in fields] == [f for f, _ in kkt.LpBasicEval._fields_]
    assert [abi.CTYPES[t] for t, _ in fields] == [t for _, t in kkt.LpBasicEval._fields_]
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "ipx_kkt_hip.h"', "int main() {",
             '    std::printf("size %zu\\n", sizeof(ipxk_lp_basic_eval));']
    lines += ['    std::printf("%s %%zu\\n", offsetof(ipxk_lp_basic_eval, %s));' % (f, f) for _, f in fields]
    src = tmp_path / "layout.cc"
    src.write_text("\n".join(lines + ["}"]) + "\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([cxx, "-std=c++14", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(ln.split() for ln in subprocess.check_output([exe], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(kkt.LpBasicEval)
    for f, _ in kkt.LpBasicEval._fields_:
        assert int(got[f]) == getattr(kkt.LpBasicEval, f).offset, f


@pytest.mark.parametrize("dualize", ["-1", "1"])
def test_example_prints_the_vertex(dualize):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    r = subprocess.run([os.path.join(ROOT, "examples", "lp_user"), dualize], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"^status_crossover 1\b", r.stdout, flags=re.M), r.stdout
    rows = re.findall(r"^vertex x(\d) = +(\S+) +z = +(\S+) +vbasis (-?\d)", r.stdout, flags=re.M)
    x, z, vb = [float(v[1]) for v in rows], [float(v[2]) for v in rows], [int(v[3]) for v in rows]
    assert len(rows) == 4 and np.abs(np.array(x) - [1.5, -0.5, 3.0, 1.5]).max() <= 1e-9, r.stdout
    cons = re.findall(r"^vertex row (\d) \(.\): slack = +(\S+) +y = +(\S+) +cbasis (-?\d)", r.stdout, flags=re.M)
    slack, y, cb = [float(v[1]) for v in cons], [float(v[2]) for v in cons], [int(v[3]) for v in cons]
    assert len(cons) == 3
    # a consistent basis: as many basic variables and rows as there are rows; nonbasic variables on their bounds, basic ones
    # with z = 0; nonbasic rows with slack 0, basic rows with y 0
    assert sum(v == 0 for v in vb) + sum(c == 0 for c in cb) == 3
    lb, ub = [0.0, -INF, 0.0, -INF], [INF, 5.0, 3.0, INF]
    for j in range(4):
        assert (vb[j] != -1 or x[j] == lb[j]) and (vb[j] != -2 or x[j] == ub[j]) and (vb[j] != 0 or z[j] == 0.0), r.stdout
    for i in range(3):
        assert (cb[i] != -1 or slack[i] == 0.0) and (cb[i] != 0 or y[i] == 0.0), r.stdout
    assert abs(float(re.search(r"vertex objval ([-+.\de]+)", r.stdout).group(1)) + 2.5) <= 1e-9, r.stdout
