"""GPU: the end of the device interior point solve -- ipxk_iterate_postprocess (Iterate::Postprocess, reference
src/iterate.cc:250-313), the postprocessed branches of the residuals and objectives (:552-556, :599-609),
ipxk_iterate_dropping_residuals (:393-448) with the crossover_start part of term_crit_reached (:237-248),
ipxk_iterate_drop_to_complementarity (:315-391) and ipxk_ipm_solve (LpSolver::InteriorPointSolve, src/lp_solver.cc:305-462).

The cited lines are element-wise rules; they are restated in numpy below and the device is held to them: exactly where a
rule has no sum (the library is built with -ffp-contract=off), to the project's operator parity gate 1e-12 (|c_j| + sum_i
|a_ij y_i|) where it has the row sum a_j'y, whose association differs between the gather layouts."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ipx_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "test_lp_ref")
KEYS = ("x", "xl", "xu", "y", "zl", "zu")
E_ARGUMENT = -3
FIXED, FREE, LB, UB, BOXED = range(5)
BASIC, BASIC_FREE, NONBASIC, NONBASIC_FIXED = 0, 1, -1, -2
M, N_ = 300, 700                      # not a multiple of the block size; more than 255 rows: a full column is a long row


@pytest.fixture(scope="module")
def kkt():
    from ipx_amd import kkt as k
    k.load_library()
    return k


# ---- the LP family of tests/test_gpu_starting_basis.py (a copy of its generator) ------------------------------------------
def general_lp(m, n, seed, dep=2, eq_share=0.4, kinds=(0.7, 0.1, 0.1, 0.1), break_row=False, break_col=False):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    k = 6
    rows = np.concatenate([rng.choice(m, k, replace=False) for _ in range(n)])
    cols = np.repeat(np.arange(n), k)
    vals = rng.choice([-1.0, 1.0], n * k) * rng.uniform(0.5, 4.0, n * k)
    A = sp.csc_matrix((vals, (rows, cols)), shape=(m, n)).tolil()
    kind = rng.choice(4, n, p=list(kinds))                  # 0 lower bound only, 1 free, 2 fixed, 3 boxed
    eq = rng.random(m) < eq_share
    free, eqi = np.nonzero(kind == 1)[0], np.nonzero(eq)[0]
    copies_c = [(free[2 * t + 1], free[2 * t]) for t in range(dep)]
    copies_r = [(eqi[2 * t + 1], eqi[2 * t]) for t in range(dep)]
    for dst, src in copies_c:
        A[:, dst] = A[:, src]
    for dst, src in copies_r:
        A[dst, :] = A[src, :]
    A = A.tocsc()
    A.sort_indices()
    x0 = rng.uniform(0.5, 2.0, n)
    lb, ub = np.zeros(n), np.full(n, np.inf)
    lb[kind == 1] = -np.inf
    lb[kind == 2] = ub[kind == 2] = x0[kind == 2]
    ub[kind == 3] = x0[kind == 3] + rng.uniform(0.5, 2.0, (kind == 3).sum())
    s0 = np.where(eq, 0.0, rng.uniform(0.5, 2.0, m))
    b = A @ x0 + s0
    y0 = np.where(eq, rng.uniform(-1.5, 1.5, m), -rng.uniform(0.5, 1.5, m))
    z = rng.uniform(0.5, 2.0, n)
    z[kind == 1] = 0.0
    z[kind == 3] *= rng.choice([-1.0, 1.0], (kind == 3).sum())
    c = A.T @ y0 + z
    for dst, src in copies_c:
        c[dst] = c[src]
    if break_row:
        b[copies_r[0][0]] += 1.0
    if break_col:
        c[copies_c[0][0]] += 1.0
    lbs = np.concatenate([lb, np.where(eq, 0.0, 0.0)])
    ubs = np.concatenate([ub, np.where(eq, 0.0, np.inf)])
    Mx = synth.CscMatrix(m, n, A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.copy())
    return dict(A=Mx, S=A, b=b, c=np.concatenate([c, np.zeros(m)]), lb=lbs, ub=ubs, eq=eq, kind=kind,
                copies_c=copies_c, copies_r=copies_r, m=m, n=n)


def highs(P):
    from scipy.optimize import linprog
    S, eq, n = P["S"], P["eq"], P["n"]
    bounds = [(None if np.isinf(l) else l, None if np.isinf(u) else u) for l, u in zip(P["lb"][:n], P["ub"][:n])]
    r = linprog(P["c"][:n], A_ub=S[~eq] if (~eq).any() else None, b_ub=P["b"][~eq] if (~eq).any() else None,
                A_eq=S[eq] if eq.any() else None, b_eq=P["b"][eq] if eq.any() else None, bounds=bounds, method="highs")
    assert r.status == 0, r
    return r.fun


def with_identity(S, m):
    import scipy.sparse as sp
    return sp.hstack([S, sp.identity(m)]).tocsc()


def initial_states(lb, ub):
    """Iterate::Initialize (src/iterate.cc:76-88); lb == ub gives BARRIER_BOXED"""
    st = np.full(len(lb), BOXED, np.uint8)
    st[np.isinf(lb) & np.isinf(ub)] = FREE
    st[np.isfinite(lb) & np.isinf(ub)] = LB
    st[np.isinf(lb) & np.isfinite(ub)] = UB
    return st


# ---- the numpy restatement of src/iterate.cc:250-448 ----------------------------------------------------------------------
def details(state, lb, ub):
    """the reference's StateDetail of the variables Postprocess touches, from the five device states and the bounds"""
    fixed = state == FIXED
    implied_eq = (state == FREE) & (lb == ub) & np.isfinite(lb)
    return fixed, implied_eq


def restate_postprocess(AI, c, lb, ub, it, state):
    """:250-313"""
    fixed, impl = details(state, lb, ub)
    out = {k: v.copy() for k, v in it.items()}
    with np.errstate(invalid="ignore"):
        z = c - AI.T @ it["y"]
        out["xl"][fixed] = (it["x"] - lb)[fixed]
        out["xu"][fixed] = (ub - it["x"])[fixed]
    feq = fixed & (lb == ub)
    out["zl"][feq & (z >= 0)] = z[feq & (z >= 0)]
    out["zu"][feq & ~(z >= 0)] = -z[feq & ~(z >= 0)]
    out["zl"][impl] = np.where(z >= 0, z, 0.0)[impl]
    out["zu"][impl] = np.where(z >= 0, 0.0, -z)[impl]
    out["x"][impl] = lb[impl]
    out["xl"][impl] = 0.0
    out["xu"][impl] = 0.0
    return out, fixed | impl


def row_sum_scale(AI, c, y):
    """|c_j| + sum_i |a_ij y_i|: what the operator parity gate 1e-12 multiplies"""
    return np.abs(c) + abs(AI).T @ np.abs(y)


def restate_rc(AI, c, it):
    """:550-551 of a postprocessed iterate: no variable is masked"""
    return c - AI.T @ it["y"] - it["zl"] + it["zu"]


def restate_objectives(b, c, lb, ub, it):
    """:599-609; returns pobjective, dobjective and the sum of the absolute terms of each"""
    fl, fu = np.isfinite(lb), np.isfinite(ub)
    pterms = c * it["x"]
    dterms = np.concatenate([b * it["y"], lb[fl] * it["zl"][fl], -(ub[fu] * it["zu"][fu])])
    return pterms.sum(), dterms.sum(), np.abs(pterms).sum(), np.abs(dterms).sum()


def restate_dropping(AI, state, lb, ub, it):
    """:393-448; returns pres, dres and the histogram of the six barrier branches"""
    x, xl, xu, zl, zu = (it[k] for k in ("x", "xl", "xu", "zl", "zu"))
    with np.errstate(divide="ignore", invalid="ignore"):
        lower = np.where(state == BOXED, zl / xl >= zu / xu, state == LB)
    barrier = (state == LB) | (state == UB) | (state == BOXED)
    active = np.where(lower, zl >= xl, zu >= xu)
    with np.errstate(invalid="ignore"):
        xdrop = np.where(barrier & active, np.where(lower, x - lb, x - ub), 0.0)
        zdrop = np.where(barrier & ~active, zl - zu, 0.0)
    amax = np.asarray(abs(AI).max(axis=0).toarray()).ravel()
    hist = {}
    for name, st in (("lb", LB), ("ub", UB)):
        hist[name + "_active"] = int(((state == st) & active).sum())
        hist[name + "_inactive"] = int(((state == st) & ~active).sum())
    for side, sel in (("lower", lower), ("upper", ~lower)):
        hist["boxed_" + side + "_active"] = int(((state == BOXED) & sel & active).sum())
        hist["boxed_" + side + "_inactive"] = int(((state == BOXED) & sel & ~active).sum())
    return float((np.abs(xdrop) * amax).max()), float(np.abs(zdrop).max()), hist


def restate_drop(lb, ub, it):
    """:315-391; returns x, y, z and the branch histogram"""
    x, xl, xu, zl, zu = (it[k] for k in ("x", "xl", "xu", "zl", "zu"))
    xj = np.minimum(np.maximum(x, lb), ub)
    d = zl - zu
    dpos, dneg = np.maximum(0.0, d), np.minimum(0.0, d)
    fl, fu = np.isfinite(lb), np.isfinite(ub)
    eq = lb == ub
    boxed, lo, up, free = ~eq & fl & fu, ~eq & fl & ~fu, ~eq & ~fl & fu, ~eq & ~fl & ~fu
    with np.errstate(invalid="ignore"):
        lower = zl * xu >= zu * xl
    al, au = zl >= xl, zu >= xu
    br = {"fixed": eq, "boxed_lower_active": boxed & lower & al, "boxed_lower_inactive": boxed & lower & ~al,
          "boxed_upper_active": boxed & ~lower & au, "boxed_upper_inactive": boxed & ~lower & ~au,
          "lb_active": lo & al, "lb_inactive": lo & ~al, "ub_active": up & au, "ub_inactive": up & ~au, "free": free}
    assert sum(v.sum() for v in br.values()) == len(x)
    at_l = br["fixed"] | br["boxed_lower_active"] | br["lb_active"]
    at_u = br["boxed_upper_active"] | br["ub_active"]
    xo = np.where(at_l, lb, np.where(at_u, ub, xj))
    zo = np.where(br["fixed"], d, np.where(br["boxed_lower_active"] | br["lb_active"], dpos, np.where(at_u, dneg, 0.0)))
    return xo, it["y"].copy(), zo, {k: int(v.sum()) for k, v in br.items()}


# ---- models and iterates --------------------------------------------------------------------------------------------------
def mixed_model(seed=11, dense=False):
    """synth.mixed_bounds_lp at the base size; dense: the first three columns hold all 300 rows (long rows of the column
    gather matrix), two of them with lb == ub"""
    A, b, c, lb, ub, kind = synth.mixed_bounds_lp(M, N_, seed)
    if dense:
        import scipy.sparse as sp
        rng = np.random.default_rng(seed + 5)
        S = A.to_scipy().tolil()
        for j in range(3):
            S[:, j] = (rng.choice([-1.0, 1.0], M) * rng.uniform(0.5, 4.0, M)).reshape(-1, 1)
        S = sp.csc_matrix(S)
        S.sort_indices()
        A = synth.CscMatrix(M, N_, S.indptr.astype(np.int64), S.indices.astype(np.int64), S.data.copy())
        lb, ub = lb.copy(), ub.copy()
        lb[0] = ub[0] = 0.75
        lb[1] = ub[1] = -1.25
        lb[2], ub[2] = 0.0, np.inf
    return A, b, c, lb, ub


def mixed_iterate(lb, ub, n, seed, with_special=True, exact=False):
    """an iterate with all five states: barrier variables by the bounds; of the lb == ub variables two thirds FIXED (x = lb,
    or off it unless exact: the rule xl = x - lb is element-wise), of the '=' slacks a quarter implied (FREE, xl = xu =
    inf) and a quarter FIXED; of the free structurals a third FIXED at 0 (dependent columns)"""
    rng = np.random.default_rng(seed)
    N, m = len(lb), len(lb) - n
    hl, hu = np.isfinite(lb), np.isfinite(ub)
    state = initial_states(lb, ub)
    it = dict(x=rng.uniform(-2.0, 2.0, N), y=rng.uniform(-1.0, 1.0, m))
    it["xl"] = np.where(hl, 10.0 ** rng.uniform(-2, 1, N), np.inf)
    it["xu"] = np.where(hu, 10.0 ** rng.uniform(-2, 1, N), np.inf)
    it["zl"] = np.where(hl, 10.0 ** rng.uniform(-2, 1, N), 0.0)
    it["zu"] = np.where(hu, 10.0 ** rng.uniform(-2, 1, N), 0.0)
    if not with_special:
        return it, state
    u = rng.random(N)
    eq = lb == ub
    slack = np.arange(N) >= n
    fixed = (eq & ~slack & (u < 0.67)) | (eq & slack & (u < 0.25)) | ((state == FREE) & (u < 0.33))
    implied = eq & slack & (u >= 0.25) & (u < 0.5)
    state[fixed] = FIXED
    state[implied] = FREE
    for k in ("xl", "xu", "zl", "zu"):
        it[k][fixed] = 0.0
    it["x"][fixed & eq] = lb[fixed & eq] if exact else (lb + np.where(u < 0.1, 0.125, 0.0))[fixed & eq]
    it["x"][fixed & ~eq] = 0.0
    it["xl"][implied] = it["xu"][implied] = np.inf
    it["zl"][implied] = it["zu"][implied] = 0.0
    assert set(np.unique(state).tolist()) == {0, 1, 2, 3, 4}
    assert (fixed & eq & ~slack).any() and (fixed & eq & slack).any() and (fixed & ~eq).any() and implied.any()
    return it, state


def check_postprocess(ctx, A, c, lb, ub, it, state):
    AI = with_identity(A.to_scipy(), A.nrow)
    want, touched = restate_postprocess(AI, c, lb, ub, it, state)
    ctx.iterate_set(it, state)
    ctx.iterate_postprocess(c, lb, ub)
    got = ctx.iterate_get()
    for k in ("x", "xl", "xu", "y"):
        assert np.array_equal(got[k], want[k]), k
    scale = row_sum_scale(AI, c, it["y"])
    for k in ("zl", "zu"):
        err = np.abs(got[k] - want[k])
        print("%s: worst error over the gate %.3e" % (k, (err / (1e-12 * scale)).max()))
        assert (err <= 1e-12 * scale).all(), k
        assert np.array_equal(got[k] == 0.0, want[k] == 0.0), k
    for k in KEYS:
        if k != "y":
            assert got[k][~touched].tobytes() == np.ascontiguousarray(it[k][~touched]).tobytes(), k
    return got, touched


# ---- 1. postprocess against the restatement -------------------------------------------------------------------------------
def force_layout(monkeypatch, layout):
    """the sliced layouts associate a row's sum per slice: slices of 1 KiB make y (300 entries) span four of them"""
    if layout:
        monkeypatch.setenv("IPXK_SPMV_LAYOUT", layout)
    if layout in ("sliced", "acc"):
        monkeypatch.setenv("IPXK_SLICE_TEST_KB", "1")


@pytest.mark.parametrize("layout", [None, "phased", "fused", "sliced", "acc"])
def test_postprocess_against_restatement(kkt, monkeypatch, layout):
    force_layout(monkeypatch, layout)
    A, b, c, lb, ub = mixed_model()
    ctx = kkt.KktContext(A)
    used = ctx.spmv_layout()[0][0]
    print("layout of A'y:", used)
    assert layout is None or used == layout
    it, state = mixed_iterate(lb, ub, N_, 3)
    _, touched = check_postprocess(ctx, A, c, lb, ub, it, state)
    assert touched[:N_].any() and touched[N_:].any()
    ctx.close()


@pytest.mark.parametrize("layout", [None, "sliced"])
def test_postprocess_dense_columns(kkt, monkeypatch, layout):
    force_layout(monkeypatch, layout)
    A, b, c, lb, ub = mixed_model(dense=True)
    ctx = kkt.KktContext(A)
    assert layout is None or ctx.spmv_layout()[0][0] == layout
    assert ctx.layout_info(0)[0]["nlong"] == 3                # the dense columns take the long-row kernels
    it, state = mixed_iterate(lb, ub, N_, 4)
    state[:2] = FIXED
    for k in ("xl", "xu", "zl", "zu"):
        it[k][:2] = 0.0
    it["x"][:2] = lb[:2]
    got, touched = check_postprocess(ctx, A, c, lb, ub, it, state)
    assert touched[0] and touched[1] and not touched[2]
    assert (got["zl"][:2] + got["zu"][:2] > 0).all()
    ctx.close()


def test_postprocess_without_fixed_or_implied(kkt):
    A, b, c, lb, ub = mixed_model()
    ctx = kkt.KktContext(A)
    it, state = mixed_iterate(lb, ub, N_, 5, with_special=False)
    assert not (state == FIXED).any()
    assert not any(details(state, lb, ub)[k].any() for k in (0, 1))
    ctx.iterate_set(it, state)
    ctx.iterate_postprocess(c, lb, ub)
    got = ctx.iterate_get()
    for k in KEYS:
        assert got[k].tobytes() == np.ascontiguousarray(it[k]).tobytes(), k
    with pytest.raises(kkt.KktError, match="postprocessed") as e:            # the flag is set all the same
        ctx.iterate_update(0.5, it["x"], None, None, 0.5, None, None, None)
    assert e.value.code == E_ARGUMENT
    ctx.close()


# ---- 2. the flagged evaluation ---------------------------------------------------------------------------------------------
def test_flagged_evaluation(kkt):
    A, b, c, lb, ub = mixed_model()
    AI = with_identity(A.to_scipy(), M)
    it, state = mixed_iterate(lb, ub, N_, 6)
    fresh = kkt.KktContext(A)                                 # a context that never postprocesses
    fresh.iterate_set(it, state)
    r_fresh = fresh.iterate_residuals(b, c, lb, ub)
    o_fresh = fresh.iterate_objectives(b, c, lb, ub)
    fresh.close()
    ctx = kkt.KktContext(A)
    ctx.iterate_set(it, state)
    assert ctx.iterate_factorize_diag() == 0
    ctx.iterate_postprocess(c, lb, ub)
    post = ctx.iterate_get()
    r = ctx.iterate_residuals(b, c, lb, ub)
    fixed = state == FIXED
    assert not r_fresh["rc"][fixed].any()
    want = restate_rc(AI, c, post)
    scale = row_sum_scale(AI, c, post["y"])
    assert (np.abs(r["rc"] - want) <= 1e-12 * scale).all()
    assert r["dresidual"] == np.abs(r["rc"]).max()
    # fixed variables with infinite bounds keep their reduced cost: rc is no longer masked there
    assert np.abs(r["rc"][fixed & np.isinf(lb)]).max() > 1e-3
    assert not r["rl"][fixed].any() and not r["ru"][fixed].any()
    pobj, dobj, offset = ctx.iterate_objectives(b, c, lb, ub)
    wp, wd, sp_, sd_ = restate_objectives(b, c, lb, ub, post)
    assert offset == 0.0
    assert abs(pobj - wp) <= 1e-12 * sp_ and abs(dobj - wd) <= 1e-12 * sd_
    assert o_fresh[2] != 0.0
    # the iterate no longer advances
    z = np.zeros(N_ + M)
    for call in (lambda: ctx.iterate_update(0.5, z, z, z, 0.5, np.zeros(M), z, z),
                 lambda: ctx.ipm_step(False, b, c, lb, ub), lambda: ctx.ipm_driver(b, c, lb, ub, ipm_maxiter=2)):
        with pytest.raises(kkt.KktError, match="postprocessed") as e:
            call()
        assert e.value.code == E_ARGUMENT
    after = ctx.iterate_get()
    for k in KEYS:
        assert after[k].tobytes() == post[k].tobytes(), k
    # ipxk_iterate_set: the old behaviour is back
    ctx.iterate_set(it, state)
    r2 = ctx.iterate_residuals(b, c, lb, ub)
    for k in ("rb", "rc", "rl", "ru"):
        assert r2[k].tobytes() == r_fresh[k].tobytes(), k
    assert (r2["presidual"], r2["dresidual"]) == (r_fresh["presidual"], r_fresh["dresidual"])
    assert ctx.iterate_objectives(b, c, lb, ub) == o_fresh
    ctx.iterate_update(0.5, z, z, z, 0.5, np.zeros(M), z, z)
    ctx.close()


# ---- 3. dropping residuals and the drop --------------------------------------------------------------------------------------
def dropping_and_drop(kkt, ctx, A, c, lb, ub, it, state):
    AI = with_identity(A.to_scipy(), A.nrow)
    ctx.iterate_set(it, state)
    raw = ctx.iterate_get()
    got = ctx.iterate_dropping_residuals(lb, ub)
    pres, dres, hist = restate_dropping(AI, state, lb, ub, raw)
    print("dropping residuals", got, hist)
    assert min(hist.values()) > 0, hist                       # both sides of zl/xl >= zu/xu and of zl >= xl, zu >= xu
    assert got == (pres, dres) and pres > 0 and dres > 0
    with pytest.raises(kkt.KktError, match="not been postprocessed") as e:
        ctx.iterate_drop_to_complementarity(lb, ub)
    assert e.value.code == E_ARGUMENT
    ctx.iterate_postprocess(c, lb, ub)
    post = ctx.iterate_get()
    for k in ("xl", "xu", "zl", "zu"):
        assert (post[k] >= 0).all(), k                        # what DropToComplementarity asserts
    x, y, z = ctx.iterate_drop_to_complementarity(lb, ub)
    wx, wy, wz, branches = restate_drop(lb, ub, post)
    print("drop to complementarity", branches)
    assert min(branches.values()) > 0, branches               # the eight barrier branches, fixed and free
    assert np.array_equal(x, wx) and np.array_equal(y, wy) and np.array_equal(z, wz)
    assert ctx.iterate_dropping_residuals(lb, ub) == restate_dropping(AI, state, lb, ub, post)[:2]
    return got, (x, y, z), post


def test_dropping_residuals_and_drop(kkt):
    A, b, c, lb, ub = mixed_model()
    it, state = mixed_iterate(lb, ub, N_, 7, exact=True)
    ctx = kkt.KktContext(A)
    dropping_and_drop(kkt, ctx, A, c, lb, ub, it, state)
    ctx.close()


# ---- 4. the test that fails without the feature: the interior solution of an LP with '=' rows and fixed variables ---------
SOLVE_CASES = [(1, 60, 150), (2, 600, 1500)]
FEAS_TOL = 1e-6


def full_dual_residual(P, it):
    AI = with_identity(P["S"], P["m"])
    return np.abs(P["c"] - AI.T @ it["y"] - it["zl"] + it["zu"]).max()


def assert_bounds_postprocessed(P, it, status):
    lb, ub = P["lb"], P["ub"]
    fixed = status == NONBASIC_FIXED
    implied = (lb == ub) & (status == BASIC_FREE)
    sel = fixed | implied
    with np.errstate(invalid="ignore"):
        assert np.array_equal(it["xl"][sel], (it["x"] - lb)[sel]) and np.array_equal(it["xu"][sel], (ub - it["x"])[sel])
    assert np.array_equal(it["x"][implied], lb[implied])
    return fixed, implied


@pytest.mark.parametrize("seed,m,n", SOLVE_CASES)
def test_solve_returns_the_interior_solution(kkt, seed, m, n):
    P = general_lp(m, n, seed, dep=2)
    b, c, lb, ub = P["b"], P["c"], P["lb"], P["ub"]
    f = highs(P)
    bound = FEAS_TOL * (1.0 + np.abs(c).max())
    ctx = kkt.KktContext(P["A"])
    g = ctx.ipm_solve(b, c, lb, ub)
    print({k: v for k, v in g.items() if np.isscalar(v)}, "HiGHS", f)
    assert g["status_ipm"] == 1 and g["errflag"] == 0, g
    assert g["dependent_rows"] == 2 and g["dependent_cols"] == 2
    it = ctx.iterate_get()
    dres = full_dual_residual(P, it)
    print("full dual residual %.3e (bound %.3e)" % (dres, bound))
    assert dres <= bound
    fixed, implied = assert_bounds_postprocessed(P, it, g["status"])
    assert implied.sum() == 2 and (np.nonzero(implied)[0] >= n).all() and fixed.sum() >= (P["kind"] == 2).sum()
    assert abs(g["pobjective"] - f) <= 1e-6 * (1.0 + abs(f))
    assert g["pobjective"] == ctx.iterate_objectives(b, c, lb, ub)[0]
    ctx.close()
    # what the hand-chained sequence leaves behind: fixed variables count as dual feasible although they are not
    ctx = kkt.KktContext(P["A"])
    assert ctx.ipm_starting_point(b, c, lb, ub)["status_ipm"] == 0
    assert ctx.ipm_driver(b, c, lb, ub, kkt_maxiter=5000, ipm_maxiter=4)["status_ipm"] in (1, 6)
    assert ctx.ipm_starting_basis(b, c, lb, ub)["errflag"] == 0
    g2 = ctx.ipm_driver_basis(b, c, lb, ub, ipm_maxiter=100)
    assert g2["status_ipm"] == 1
    dres_chain = full_dual_residual(P, ctx.iterate_get())
    print("hand-chained: full dual residual %.3e" % dres_chain)
    assert dres_chain > bound
    ctx.close()


# ---- 5. ipxk_ipm_solve against the reference ---------------------------------------------------------------------------------
def run_reference(P, tmp_path, extra=""):
    n, m = P["n"], P["m"]
    din, dout = str(tmp_path / "in"), str(tmp_path / "out")
    os.makedirs(din)
    os.makedirs(dout)
    i64, f64 = np.int64, np.float64
    A = P["A"]
    np.array([n, m], i64).tofile(os.path.join(din, "dims.bin"))
    for k, v in (("obj", P["c"][:n]), ("lb", P["lb"][:n]), ("ub", P["ub"][:n]), ("rhs", P["b"]), ("Ax", A.x)):
        np.ascontiguousarray(v, f64).tofile(os.path.join(din, k + ".bin"))
    for k, v in (("Ap", A.p), ("Ai", A.i)):
        np.ascontiguousarray(v, i64).tofile(os.path.join(din, k + ".bin"))
    with open(os.path.join(din, "constr_type.bin"), "wb") as fh:
        fh.write("".join("=" if e else "<" for e in P["eq"]).encode())
    with open(os.path.join(din, "params.txt"), "w") as fh:
        fh.write("crash_basis 0\ndualize 0\ncrossover 0\n" + extra)
    r = subprocess.run([REF_BIN, din, dout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DONE" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    ref = {}
    for ln in open(os.path.join(dout, "info.txt")):
        k, v = ln.split()
        ref[k] = float(v)
    return ref


@pytest.mark.parametrize("broken", [None, "row", "col"])
@pytest.mark.parametrize("seed,m,n", SOLVE_CASES)
def test_solve_against_the_reference(kkt, tmp_path, seed, m, n, broken):
    if not os.path.exists(REF_BIN):
        pytest.skip("oracle/_ref/test_lp_{ref,hip} not built (needs the reference sources at build time)")
    P = general_lp(m, n, seed, dep=2, break_row=broken == "row", break_col=broken == "col")
    b, c, lb, ub = P["b"], P["c"], P["lb"], P["ub"]
    ref = run_reference(P, tmp_path)
    ctx = kkt.KktContext(P["A"])
    g = ctx.ipm_solve(b, c, lb, ub)
    print("IPM iterations: reference %d, device %d (%d initial); status reference %d, device %d"
          % (ref["iter"], g["iter"], g["iter_initial"], ref["status_ipm"], g["status_ipm"]))
    want = {None: 1, "row": 3, "col": 4}[broken]
    assert ref["status_ipm"] == want and g["status_ipm"] == want, (ref["status_ipm"], g)
    for k in ("dependent_rows", "dependent_cols", "rows_inconsistent", "cols_inconsistent"):
        assert ref[k] == g[k], (k, ref[k], g[k])
    if broken is None:
        assert abs(g["pobjective"] - ref["pobjval"]) <= 1e-6 * (1.0 + abs(ref["pobjval"]))
        for side, src in (("reference", ref), ("device", g)):
            print(side, src["rel_presidual"], src["rel_dresidual"], src["rel_objgap"])
            assert src["rel_presidual"] <= FEAS_TOL and src["rel_dresidual"] <= FEAS_TOL, side
            assert abs(src["rel_objgap"]) <= 1e-8, side
    # postprocessed whatever the status: the flag is set and the bound residuals of the fixed and implied variables are 0
    it = ctx.iterate_get()
    assert_bounds_postprocessed(P, it, g["status"])
    with pytest.raises(kkt.KktError, match="postprocessed"):
        ctx.ipm_driver(b, c, lb, ub, ipm_maxiter=1)
    ctx.close()


def test_solve_status_mappings(kkt):
    P = general_lp(60, 150, 1, dep=2)
    b, c, lb, ub = P["b"], P["c"], P["lb"], P["ub"]
    ctx = kkt.KktContext(P["A"])
    full = ctx.ipm_solve(b, c, lb, ub, switchiter=4)
    assert full["status_ipm"] == 1 and full["iter_initial"] == 4 and full["status_initial"] == 6 and full["iter"] > 6, full
    # switchiter = 0 goes straight to the basis
    g = ctx.ipm_solve(b, c, lb, ub, switchiter=0)
    assert g["status_ipm"] == 1 and g["iter_initial"] == 0 and g["status_initial"] == 6 and g["updates_start"] > 0, g
    # the iteration limit counts both phases
    g = ctx.ipm_solve(b, c, lb, ub, switchiter=4, ipm_maxiter=6)
    assert g["status_ipm"] == 6 and g["iter"] == 6 and g["iter_initial"] == 4, g
    g = ctx.ipm_solve(b, c, lb, ub, switchiter=4, ipm_maxiter=3)
    assert g["status_ipm"] == 6 and g["iter"] == 3 and g["updates_start"] == 0, g
    # an interrupt that fires in the starting basis: the calls before it are those of the starting point (the driver with
    # switchiter = 0 ends before its first check)
    calls = [0]

    def counting():
        calls[0] += 1
        return 0
    assert ctx.ipm_starting_point(b, c, lb, ub, interrupt=counting)["status_ipm"] == 0
    before = calls[0]
    calls[0] = 0

    def in_the_basis():
        calls[0] += 1
        return 999 if calls[0] == before + 2 else 0
    g = ctx.ipm_solve(b, c, lb, ub, switchiter=0, interrupt=in_the_basis)
    assert g["status_ipm"] == 5 and g["errflag"] == 0 and calls[0] == before + 2, (g, calls, before)
    # a loaded starting point: the starting point and the initial iterations are skipped
    assert ctx.ipm_starting_point(b, c, lb, ub)["status_ipm"] == 0
    ctx.ipm_load_starting_point(ctx.iterate_get(), lb, ub)
    g = ctx.ipm_solve(b, c, lb, ub, use_resident_point=True)
    assert g["status_ipm"] == 1 and g["iter_initial"] == 0 and g["status_initial"] == 0, g
    ctx.close()


# ---- 6. crossover_start -----------------------------------------------------------------------------------------------------
# Seeds 1 to 16 of synth.mixed_bounds_lp(300, 700, seed, free=False) were tried on the CPU: the oracle's starting point, then
# IPM::Driver restated around the oracle's Factorize and step with term_crit_reached from restate_dropping.  With the diag
# solver most of them end with no_progress once the dropping residuals are asked for (1, 4, 6, 9-13, 15; 16 fails in CR,
# 14 meets them at once); 2, 5, 7 and 8 reach them.  Seed 2 has the widest margins: with crossover_start = 0 it stops after
# 19 iterations with pres 1.49e-6 against the bound 3.06e-7; with 1e-8 after 22 with pres 1.60e-7, dres 3.6e-9 (bound 1.83e-7).
CROSSOVER_SEED = 2
CROSSOVER_START = 1e-8


def model_norms(b, c, lb, ub):
    """Model::ComputeNorms, src/model.cc:58-67"""
    nb = max(np.abs(b).max(), np.abs(lb[np.isfinite(lb)]).max(initial=0.0), np.abs(ub[np.isfinite(ub)]).max(initial=0.0))
    return nb, np.abs(c).max()


def within_dropping_bound(drop, norms, value=CROSSOVER_START):
    return drop[0] <= value * (1.0 + norms[0]) and drop[1] <= value * (1.0 + norms[1])


def crossover_model():
    A, b, c, lb, ub, _ = synth.mixed_bounds_lp(M, N_, CROSSOVER_SEED, free=False)
    return A, b, c, lb, ub


def test_crossover_start(kkt):
    A, b, c, lb, ub = crossover_model()
    norms = model_norms(b, c, lb, ub)
    ctx = kkt.KktContext(A)
    assert ctx.ipm_starting_point(b, c, lb, ub)["status_ipm"] == 0
    start = ctx.iterate_get()
    g0 = ctx.ipm_driver(b, c, lb, ub, kkt_maxiter=5000, ipm_maxiter=100)
    drop0 = ctx.iterate_dropping_residuals(lb, ub)
    print("crossover_start 0: %d iterations, dropping residuals %s, bounds %s"
          % (g0["iter"], drop0, tuple(CROSSOVER_START * (1.0 + v) for v in norms)))
    assert g0["status_ipm"] == 1
    assert not within_dropping_bound(drop0, norms)
    ctx.ipm_set_crossover_start(CROSSOVER_START)
    ctx.iterate_set(start, initial_states(lb, ub))
    g1 = ctx.ipm_driver(b, c, lb, ub, kkt_maxiter=5000, ipm_maxiter=100)
    drop1 = ctx.iterate_dropping_residuals(lb, ub)
    print("crossover_start 1e-8: %d iterations, dropping residuals %s" % (g1["iter"], drop1))
    assert g1["status_ipm"] == 1 and g1["iter"] > g0["iter"]
    assert within_dropping_bound(drop1, norms)
    with pytest.raises(kkt.KktError) as e:
        ctx.ipm_set_crossover_start(-1.0)
    assert e.value.code == E_ARGUMENT
    # ipxk_reset_solver_state restores the default: the run stops where the first one did
    ctx.reset_solver_state()
    ctx.iterate_set(start, initial_states(lb, ub))
    g2 = ctx.ipm_driver(b, c, lb, ub, kkt_maxiter=5000, ipm_maxiter=100)
    assert g2["status_ipm"] == 1 and g2["iter"] == g0["iter"]
    ctx.close()


# ---- 7. column partition -----------------------------------------------------------------------------------------------------
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
def test_one_forced_column_rank_reproduces_the_bits(kkt, monkeypatch, transport):
    A, b, c, lb, ub = mixed_model()
    it, state = mixed_iterate(lb, ub, N_, 7, exact=True)
    ref_ctx = kkt.KktContext(A)
    ref = dropping_and_drop(kkt, ref_ctx, A, c, lb, ub, it, state)
    ref_ctx.close()
    ctx = forced_context(kkt, A, transport, monkeypatch)
    got = dropping_and_drop(kkt, ctx, A, c, lb, ub, it, state)
    assert got[0] == ref[0]
    for a, w in zip(got[1], ref[1]):
        assert a.tobytes() == w.tobytes()
    for k in KEYS:
        assert got[2][k].tobytes() == ref[2][k].tobytes(), k
    res = ctx.iterate_residuals(b, c, lb, ub)
    obj = ctx.iterate_objectives(b, c, lb, ub)
    ctx.close()
    monkeypatch.delenv("IPXK_FORCE_COMM")
    again = kkt.KktContext(A)
    again.iterate_set(it, state)
    again.iterate_postprocess(c, lb, ub)
    assert again.iterate_residuals(b, c, lb, ub)["rc"].tobytes() == res["rc"].tobytes()
    assert again.iterate_objectives(b, c, lb, ub) == obj
    again.close()


def test_solve_is_refused_on_a_partitioned_context(kkt, monkeypatch):
    P = general_lp(60, 150, 1, dep=2)
    ctx = forced_context(kkt, P["A"], "direct", monkeypatch)
    with pytest.raises(kkt.KktError, match="does not run on a partitioned system") as e:
        ctx.ipm_solve(P["b"], P["c"], P["lb"], P["ub"])
    assert e.value.code == E_ARGUMENT
    with pytest.raises(kkt.KktError, match="no iterate"):     # nothing was launched: no starting point was computed
        ctx.iterate_get()
    ctx.close()


KKT_TOL_RANKS = 1e-3                  # tests/test_gpu_multirank_ipm.py, KKT_TOL_DRIVER: why the comparison is not made at 0.3


def test_crossover_start_on_two_column_ranks(kkt, tmp_path):
    A, b, c, lb, ub = crossover_model()
    norms = model_norms(b, c, lb, ub)
    world = 2
    env = dict(os.environ, IPXK_COMM="direct")
    env.pop("IPXK_FORCE_COMM", None)
    idfile, out = str(tmp_path / "uid"), str(tmp_path / "res")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "multirank_finish_worker.py"), str(r), str(world),
                               idfile, out, str(CROSSOVER_SEED), repr(CROSSOVER_START), repr(KKT_TOL_RANKS)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    logs = []
    for p in procs:
        try:
            logs.append(p.communicate(timeout=240)[0])
        except subprocess.TimeoutExpired:
            p.returncode = -9
        if p.returncode != 0:                                 # one failed rank ends the test: no second attempt
            for q in procs:
                q.kill()
            for q in procs:
                q.wait()
            pytest.fail("a rank failed or did not finish:\n" + "\n".join(logs))
    res = [np.load(out + ".rank%d.npz" % r) for r in range(world)]
    assert np.array_equal(res[0]["info"], res[1]["info"])     # status, iterations and every scalar: the same on both ranks
    assert np.array_equal(res[0]["drop"], res[1]["drop"])
    status, iters, pobj = int(res[0]["info"][0]), int(res[0]["info"][1]), float(res[0]["info"][2])
    ctx = kkt.KktContext(A)
    assert ctx.ipm_starting_point(b, c, lb, ub)["status_ipm"] == 0
    ctx.ipm_set_crossover_start(CROSSOVER_START)
    ref = ctx.ipm_driver(b, c, lb, ub, kkt_tol=KKT_TOL_RANKS, kkt_maxiter=5000, ipm_maxiter=100)
    ctx.close()
    print("two ranks: status %d, %d iterations, dropping residuals %s; unpartitioned: %d iterations"
          % (status, iters, res[0]["drop"], ref["iter"]))
    assert status == 1 and ref["status_ipm"] == 1
    assert within_dropping_bound(tuple(res[0]["drop"]), norms)
    assert abs(iters - ref["iter"]) <= max(2, int(0.1 * ref["iter"]))
    assert abs(pobj - ref["pobjective"]) <= 1e-6 * (1.0 + abs(ref["pobjective"]))
