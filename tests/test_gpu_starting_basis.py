"""GPU: ipxk_ipm_starting_basis -- StartingBasis (reference src/starting_basis.cc:128-185, crash_basis = 0) on the
resident iterate -- and the main phase that goes on from its result (ipxk_ipm_driver_basis).

The LP family has a planted interior primal-dual point (feasible and bounded by construction): 6 entries per column,
+-U[0.5, 4); structural kinds lower bound only / free / fixed / boxed with probabilities 0.7 / 0.1 / 0.1 / 0.1; 40 % of
the rows '=' (slack lb = ub = 0); planted dependencies: d free columns that are copies of other free columns, d
equality rows that are copies of other equality rows (b and c formed after copying, so both stay consistent).

Measured on the MI355X (this file's own prints): see DESIGN.md section 8f."""
import os
import subprocess

import numpy as np
import pytest

from ipx_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "test_lp_ref")
BASIC, BASIC_FREE, NONBASIC, NONBASIC_FIXED = 0, 1, -1, -2
SIZES = [(1, 60, 150), (2, 600, 1500), (3, 2000, 5000)]


@pytest.fixture(scope="module")
def kkt():
    from ipx_amd import kkt as k
    k.load_library()
    return k


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
    M = synth.CscMatrix(m, n, A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.copy())
    return dict(A=M, S=A, b=b, c=np.concatenate([c, np.zeros(m)]), lb=lbs, ub=ubs, eq=eq, kind=kind,
                copies_c=copies_c, copies_r=copies_r, m=m, n=n)


def initial_states(lb, ub):
    """Iterate::Initialize (src/iterate.cc:76-88); lb == ub gives BARRIER_BOXED"""
    st = np.full(len(lb), 4, np.uint8)
    st[np.isinf(lb) & np.isinf(ub)] = 1
    st[np.isfinite(lb) & np.isinf(ub)] = 2
    st[np.isinf(lb) & np.isfinite(ub)] = 3
    return st


def random_iterate(P, seed):
    """a valid interior iterate whose scaling factors spread over a few orders of magnitude"""
    rng = np.random.default_rng(seed)
    N, m = P["n"] + P["m"], P["m"]
    lb, ub = P["lb"], P["ub"]
    hl, hu = np.isfinite(lb), np.isfinite(ub)
    it = dict(x=rng.uniform(0.5, 2.0, N), y=rng.uniform(-1.0, 1.0, m))
    it["xl"] = np.where(hl, 10.0 ** rng.uniform(-2, 1, N), np.inf)
    it["xu"] = np.where(hu, 10.0 ** rng.uniform(-2, 1, N), np.inf)
    it["zl"] = np.where(hl, 10.0 ** rng.uniform(-2, 1, N), 0.0)
    it["zu"] = np.where(hu, 10.0 ** rng.uniform(-2, 1, N), 0.0)
    return it, initial_states(lb, ub)


def highs(P):
    from scipy.optimize import linprog
    S, eq, n = P["S"], P["eq"], P["n"]
    bounds = [(None if np.isinf(l) else l, None if np.isinf(u) else u) for l, u in zip(P["lb"][:n], P["ub"][:n])]
    r = linprog(P["c"][:n], A_ub=S[~eq] if (~eq).any() else None, b_ub=P["b"][~eq] if (~eq).any() else None,
                A_eq=S[eq] if eq.any() else None, b_eq=P["b"][eq] if eq.any() else None, bounds=bounds, method="highs")
    assert r.status == 0, r
    return r.fun


def AI_of(P):
    import scipy.sparse as sp
    return sp.hstack([P["S"], sp.identity(P["m"])]).tocsc()


def states_from_iterate(it):
    fixed = (it["xl"] == 0) & (it["xu"] == 0)
    free = np.isinf(it["xl"]) & np.isinf(it["xu"])
    return fixed, free


def assert_consistency(P, it, status):
    """AssertConsistency, src/starting_basis.cc:13-50"""
    n = P["n"]
    lb, ub = P["lb"], P["ub"]
    fixed, free = states_from_iterate(it)
    j = np.arange(len(lb))
    eqb = lb == ub
    fb = np.isinf(lb) & np.isinf(ub)
    ok_eq = (fixed & (status == NONBASIC_FIXED)) | (free & (status == BASIC_FREE) & (j >= n))
    ok_free = (fixed & (status == NONBASIC_FIXED)) | (free & (status == BASIC_FREE))
    ok_bar = ~fixed & ~free & ((status == BASIC) | (status == NONBASIC))
    ok = np.where(eqb, ok_eq, np.where(fb, ok_free, ok_bar))
    assert ok.all(), np.nonzero(~ok)[0][:10]


def check_invariants(kkt, ctx, P, g, it0, dep):
    m, n = P["m"], P["n"]
    lb, ub, b, c = P["lb"], P["ub"], P["b"], P["c"]
    it = ctx.iterate_get()
    status, basis = g["status"], g["basis"]
    assert g["errflag"] == 0
    assert_consistency(P, it, status)
    assert g["dependent_cols"] == dep and g["dependent_rows"] == dep, g
    assert g["rows_inconsistent"] == 0 and g["cols_inconsistent"] == 0
    assert len(basis) == m and sorted(basis) == sorted(np.nonzero(status >= 0)[0])
    AI = AI_of(P)
    rhs = np.random.default_rng(1).standard_normal(m)
    x = ctx.solve_dense(rhs, "n")
    assert np.abs(AI[:, basis] @ x - rhs).max() <= 1e-7 * (1 + np.abs(x).max())
    fixed, free = states_from_iterate(it)
    made_fixed = (lb == ub) & (status == NONBASIC_FIXED)
    assert np.array_equal(it["x"][made_fixed], lb[made_fixed])
    for k in ("xl", "xu", "zl", "zu"):
        assert not it[k][made_fixed].any()
    depc = np.nonzero(np.isinf(lb) & np.isinf(ub) & (status == NONBASIC_FIXED))[0]
    assert len(depc) == dep and not it["x"][depc].any()
    # AI x: unchanged except for what make_fixed moved
    x0 = it0["x"].copy()
    touched = np.zeros(m, bool)
    moved = made_fixed & (x0 != lb)
    touched[np.unique(AI[:, np.nonzero(moved)[0]].nonzero()[0])] = True
    d = np.abs(AI @ it["x"] - AI @ x0)
    print("AI x change on untouched rows %.3e" % (d[~touched].max() if (~touched).any() else 0.0))
    assert d[~touched].max() <= 1e-9 * (1 + np.abs(b).max())
    impl = np.nonzero((lb == ub) & (status == BASIC_FREE))[0]
    assert len(impl) == dep and (impl >= n).all()
    assert not it["y"][impl - n].any() and not it["zl"][impl].any() and not it["zu"][impl].any()
    dd = np.abs(AI.T @ it["y"] - AI.T @ it0["y"])[:n]
    print("AI'y change on structural columns %.3e" % dd.max())
    assert dd.max() <= 1e-9 * (1 + np.abs(c).max())


# ---- 1. invariants -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dep", [0, 2])
@pytest.mark.parametrize("seed,m,n", SIZES)
def test_invariants_after_starting_basis(kkt, seed, m, n, dep):
    P = general_lp(m, n, seed, dep=dep)
    ctx = kkt.KktContext(P["A"])
    it0, state = random_iterate(P, seed + 100)
    ctx.iterate_set(it0, state)
    g = ctx.ipm_starting_basis(P["b"], P["c"], P["lb"], P["ub"])
    print({k: v for k, v in g.items() if np.isscalar(v)})
    check_invariants(kkt, ctx, P, g, it0, dep)
    ctx.close()


# ---- 2. decisions against a dense restatement ----------------------------------------------------------------------------
def restatement(P, it, tol=1e-6):
    """the two loops of Basis::ConstructBasisFromWeights (src/basis.cc:676-930) from the slack basis with dense solves.
    Returns the exchange log, the dependent sets, the flags and the smallest relative margin of any comparison taken."""
    m, n = P["m"], P["n"]
    N = n + m
    lb, ub, c = P["lb"], P["ub"], P["c"]
    AI = AI_of(P).toarray()
    with np.errstate(divide="ignore", invalid="ignore"):
        w = 1.0 / np.sqrt(it["zl"] / it["xl"] + it["zu"] / it["xu"])
    w[np.isinf(lb) & np.isinf(ub)] = np.inf
    w[lb == ub] = 0.0
    basis = list(range(n, N))
    pos = np.full(N, -1)
    pos[n:] = np.arange(m)
    margins = []

    def margin(a, bb):
        d = max(abs(a), abs(bb))
        margins.append(abs(a - bb) / d if d > 0 else 1.0)

    def argmax(v, mask):
        idx = np.nonzero(mask & (v > 0))[0]
        if len(idx) == 0:
            return 0.0, -1, 1.0
        vals = v[idx]
        o = np.argsort(-vals, kind="stable")
        best = vals[o[0]]
        runner = vals[o[1]] if len(o) > 1 else 0.0
        mg = 0.0 if best == runner else ((best - runner) / best if np.isfinite(best) else 1.0)
        return best, int(idx[o[0]]), mg

    log, dep_cols, dep_rows = [], [], []
    cols_inc = rows_inc = 0

    def exchange(p, jn):
        jb = basis[p]
        log.append((jb, jn))
        basis[p] = jn
        pos[jn] = p
        pos[jb] = -1

    remaining = [j for j in range(N) if np.isinf(w[j]) and pos[j] < 0]
    while remaining:
        jn = remaining[-1]
        f = np.linalg.solve(AI[:, basis], AI[:, jn])
        af = np.abs(f)
        isfree = np.isinf(w[basis])
        fmax, pmax, mg_all = argmax(af, np.ones(m, bool))
        fnf, pnf, mg_nf = argmax(af, ~isfree)
        margin(fmax, 4.0)
        if fmax > 4.0:
            margin(fnf, 1.0)
        if fmax > 4.0 and fnf < 1.0:
            margins.append(mg_all)
            jb = basis[pmax]
            exchange(pmax, jn)
            remaining.pop()
            remaining.append(jb)
        else:
            margin(fnf, tol)
            if fnf <= tol:
                if not cols_inc:
                    delta = c[jn] - sum(c[basis[p]] * f[p] for p in range(m) if isfree[p])
                    margin(abs(delta), tol)
                    cols_inc = int(abs(delta) > tol)
                dep_cols.append(jn)
                remaining.pop()
            else:
                margins.append(mg_nf)
                exchange(pnf, jn)
                remaining.pop()
    bfix = P["b"].copy()
    for j in range(N):
        if lb[j] == ub[j] and lb[j] != 0.0:
            bfix -= lb[j] * AI[:, j]
    remaining = [j for j in range(n, N) if w[j] == 0.0 and pos[j] >= 0]
    jj = np.arange(N)
    while remaining:
        jb = remaining[-1]
        p = pos[jb]
        e = np.zeros(m)
        e[p] = 1.0
        bt = np.linalg.solve(AI[:, basis].T, e)
        row = AI.T @ bt
        row[pos >= 0] = 0.0
        ar = np.abs(row)
        rmax, jmax, mg_all = argmax(ar, (jj >= n) | (w != 0.0))
        rnf, jnf, _ = argmax(ar, w != 0.0)
        margin(rmax, 4.0)
        if rmax > 4.0:
            margin(rnf, 1.0)
        if rmax > 4.0 and rnf < 1.0:
            margins.append(mg_all)
            exchange(p, jmax)
            remaining.pop()
            remaining.append(jmax)
        else:
            margin(rnf, tol)
            if rnf <= tol:
                if not rows_inc:
                    delta = bt @ bfix
                    margin(abs(delta), tol)
                    rows_inc = int(abs(delta) > tol)
                dep_rows.append(jb - n)
                remaining.pop()
            else:
                nz = ar > 1e-13 * rnf                       # (entries that are zero in exact arithmetic lie far below 0.1 rnf)
                for r in ar[nz]:
                    margin(r, 0.1 * rnf)
                cand = ar >= 0.1 * rnf
                with np.errstate(invalid="ignore"):
                    rs = np.where(cand, ar * w, 0.0)
                _, jsc, mg = argmax(np.nan_to_num(rs, nan=0.0, posinf=np.inf), cand)
                margins.append(mg)
                exchange(p, jsc)
                remaining.pop()
    return dict(log=log, dep_cols=sorted(dep_cols), dep_rows=sorted(dep_rows), cols_inconsistent=cols_inc,
                rows_inconsistent=rows_inc, margin=min(margins) if margins else 1.0, basis=basis)


# seeds chosen on the CPU with the restatement alone: every comparison it takes has a relative margin >= 1e-6
DECISION_CASES = [(13, 60, 150), (13, 300, 700)]


@pytest.mark.parametrize("seed,m,n", DECISION_CASES)
def test_decisions_against_dense_restatement(kkt, seed, m, n):
    P = general_lp(m, n, seed, dep=2)
    it0, state = random_iterate(P, seed + 100)
    R = restatement(P, it0)
    print("restatement: %d exchanges, smallest margin %.3e" % (len(R["log"]), R["margin"]))
    assert R["margin"] >= 1e-6, "the generator changed: choose a seed whose decisions are not ties"
    ctx = kkt.KktContext(P["A"])
    ctx.iterate_set(it0, state)
    g = ctx.ipm_starting_basis(P["b"], P["c"], P["lb"], P["ub"])
    assert g["errflag"] == 0 and g["updates_start"] == len(R["log"])
    assert [tuple(e) for e in g["exchanges"].tolist()] == [tuple(int(v) for v in e) for e in R["log"]]
    assert list(g["basis"]) == [int(j) for j in R["basis"]]
    st = g["status"]
    assert sorted(np.nonzero(np.isinf(P["lb"]) & np.isinf(P["ub"]) & (st == NONBASIC_FIXED))[0]) == R["dep_cols"]
    assert sorted(np.nonzero((P["lb"] == P["ub"]) & (st == BASIC_FREE))[0] - n) == R["dep_rows"]
    assert g["cols_inconsistent"] == R["cols_inconsistent"] == 0 and g["rows_inconsistent"] == R["rows_inconsistent"] == 0
    ctx.close()


# ---- 3. end to end on the device -----------------------------------------------------------------------------------------
def solve_on_device(ctx, P):
    b, c, lb, ub = P["b"], P["c"], P["lb"], P["ub"]
    g0 = ctx.ipm_starting_point(b, c, lb, ub)
    assert g0["status_ipm"] == 0 and g0["errflag"] == 0, g0
    g1 = ctx.ipm_driver(b, c, lb, ub, kkt_maxiter=5000, ipm_maxiter=4)               # switchiter = 4
    assert g1["status_ipm"] in (1, 6), g1
    gs = ctx.ipm_starting_basis(b, c, lb, ub)
    assert gs["errflag"] == 0, gs
    g2 = ctx.ipm_driver_basis(b, c, lb, ub, ipm_maxiter=100)
    return g1, gs, g2


@pytest.mark.parametrize("seed,m,n", SIZES)
def test_end_to_end_on_the_device(kkt, seed, m, n):
    P = general_lp(m, n, seed, dep=2)
    f = highs(P)
    ctx = kkt.KktContext(P["A"])
    g1, gs, g2 = solve_on_device(ctx, P)
    print("starting basis:", {k: v for k, v in gs.items() if np.isscalar(v)})
    print("main phase:", {k: v for k, v in g2.items() if np.isscalar(v)}, "HiGHS", f)
    assert gs["dependent_cols"] == 2 and gs["dependent_rows"] == 2
    assert g2["status_ipm"] == 1, g2
    assert abs(g2["pobjective"] - f) <= 1e-6 * (1.0 + abs(f))
    assert abs(g2["pobjective"] - g2["dobjective"]) <= 1e-8 * (1.0 + abs(f))
    st = g2["status"]
    free = np.nonzero(P["kind"] == 1)[0]
    copies = {int(d) for d, _ in P["copies_c"]} | {int(s) for _, s in P["copies_c"]}
    for j in free:
        if int(j) not in copies:
            assert st[j] == BASIC_FREE, j
    assert not (st[P["lb"] == P["ub"]] == BASIC).any()
    ctx.close()


def test_end_to_end_standard_form(kkt):
    """the textbook LP: all rows '=', all columns lb = 0"""
    P = general_lp(600, 1500, 5, dep=0, eq_share=2.0, kinds=(1.0, 0.0, 0.0, 0.0))
    assert P["eq"].all()
    f = highs(P)
    ctx = kkt.KktContext(P["A"])
    g1, gs, g2 = solve_on_device(ctx, P)
    print(gs["updates_start"], g2["iter"], g2["pobjective"], f)
    assert gs["updates_start"] >= 600 and gs["dependent_rows"] == 0
    assert g2["status_ipm"] == 1, g2
    assert abs(g2["pobjective"] - f) <= 1e-6 * (1.0 + abs(f))
    assert abs(g2["pobjective"] - g2["dobjective"]) <= 1e-8 * (1.0 + abs(f))
    assert not (g2["status"][1500:] >= 0).any()
    ctx.close()


# ---- 4. against the reference itself ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,m,n", SIZES[1:])
def test_against_the_reference_itself(kkt, tmp_path, seed, m, n):
    if not os.path.exists(REF_BIN):
        pytest.skip("oracle/_ref/test_lp_{ref,hip} not built (needs the reference sources at build time)")
    P = general_lp(m, n, seed, dep=2)
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
        fh.write("crash_basis 0\ndualize 0\ncrossover 0\nswitchiter 4\n")
    r = subprocess.run([REF_BIN, din, dout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DONE" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    ref = {}
    for ln in open(os.path.join(dout, "info.txt")):
        k, v = ln.split()
        ref[k] = float(v)
    ctx = kkt.KktContext(P["A"])
    g1, gs, g2 = solve_on_device(ctx, P)
    neq = int(P["eq"].sum())
    print("updates_start: reference %d, device %d (%d equality rows); seconds: reference %.3f, device %.3f"
          % (ref["updates_start"], gs["updates_start"], neq, ref["time_starting_basis"], gs["seconds"]))
    assert ref["status_ipm"] == 1 and g2["status_ipm"] == 1
    for k in ("dependent_rows", "dependent_cols", "rows_inconsistent", "cols_inconsistent"):
        assert ref[k] == gs[k], (k, ref[k], gs[k])
    f = ref["pobjval"]
    assert abs(g2["pobjective"] - f) <= 1e-6 * (1.0 + abs(f))
    ctx.close()


# ---- 5. inconsistent models ----------------------------------------------------------------------------------------------
def test_inconsistent_models_are_reported(kkt):
    for kw, key in ((dict(break_row=True), "rows_inconsistent"), (dict(break_col=True), "cols_inconsistent")):
        P = general_lp(600, 1500, 2, dep=2, **kw)
        ctx = kkt.KktContext(P["A"])
        it0, state = random_iterate(P, 7)
        ctx.iterate_set(it0, state)
        g = ctx.ipm_starting_basis(P["b"], P["c"], P["lb"], P["ub"])
        assert g["errflag"] == 0 and g[key] == 1, g
        assert g["dependent_rows"] == 2 and g["dependent_cols"] == 2
        other = "cols_inconsistent" if key == "rows_inconsistent" else "rows_inconsistent"
        assert g[other] == 0
        ctx.close()


# ---- 6. state handling -----------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(kkt):
    P = general_lp(600, 1500, 2, dep=2)
    ctx = kkt.KktContext(P["A"])
    it0, state = random_iterate(P, 9)
    out = []
    for _ in range(2):
        ctx.iterate_set(it0, state)
        g = ctx.ipm_starting_basis(P["b"], P["c"], P["lb"], P["ub"])
        out.append((g, ctx.iterate_get()))
    (ga, ia), (gb, ib) = out
    assert ga["updates_start"] > 0
    assert np.array_equal(ga["basis"], gb["basis"]) and np.array_equal(ga["status"], gb["status"])
    assert np.array_equal(ga["exchanges"], gb["exchanges"])
    for k in ia:
        assert ia[k].tobytes() == ib[k].tobytes(), k
    ctx.close()


def test_interrupt_and_dropped_state(kkt):
    P = general_lp(60, 150, 1, dep=2)
    b, c, lb, ub = P["b"], P["c"], P["lb"], P["ub"]
    ctx = kkt.KktContext(P["A"])
    it0, state = random_iterate(P, 3)
    ctx.iterate_set(it0, state)
    calls = [0]

    def third():
        calls[0] += 1
        return 999 if calls[0] == 3 else 0
    g = ctx.ipm_starting_basis(b, c, lb, ub, interrupt=third)
    assert g["errflag"] == 999 and calls[0] == 3
    it = ctx.iterate_get()
    for k in it:
        assert it[k].tobytes() == np.ascontiguousarray(it0[k], np.float64).tobytes()          # the iterate is untouched
    with pytest.raises(kkt.KktError, match="barrier variables only"):                        # no live starting basis
        ctx.ipm_driver_basis(b, c, lb, ub, ipm_maxiter=2)
    # a completed call makes the main phase run; iterate_set ends that
    g = ctx.ipm_starting_basis(b, c, lb, ub)
    assert g["errflag"] == 0
    g2 = ctx.ipm_driver_basis(b, c, lb, ub, ipm_maxiter=1)
    assert g2["status_ipm"] in (1, 6)
    ctx.iterate_set(it0, state)
    with pytest.raises(kkt.KktError, match="barrier variables only"):
        ctx.ipm_driver_basis(b, c, lb, ub, ipm_maxiter=2)
    ctx.close()


def test_partitioned_context_is_refused(kkt, monkeypatch):
    from ipx_amd import partition
    P = general_lp(60, 150, 1, dep=2)
    monkeypatch.setenv("IPXK_FORCE_COMM", "1")
    monkeypatch.delenv("IPXK_COMM", raising=False)
    ctx = kkt.KktContext(partition.col_slab_matrix(P["A"], 0, P["A"].ncol))
    ctx.comm_init(ctx.comm_unique_id(), 0, 1, columns=True)
    it0, state = random_iterate(P, 3)
    ctx.iterate_set(it0, state)
    with pytest.raises(kkt.KktError, match="does not run on a partitioned system"):
        ctx.ipm_starting_basis(P["b"], P["c"], P["lb"], P["ub"])
    ctx.close()
