"""GPU: DropPrimal / DropDual on the device (drop.hip, ipxk_ipm_drop_degenerate) and the two implied states.

1. the decisions on planted states against the dense restatement (tests/drop_reference.py), entry for entry;
2. the two pivot searches at exact ties, below their thresholds and past their grid passes (dyadic inputs: equality);
3. an iterate holding both implied states against a long-double host evaluation;
4. tolerances 0, 0 (and tolerances that screen nothing) leave ipxk_ipm_solve's bits alone;
5. a degenerate LP end to end against the reference's LpSolver with the same drop tolerances.

Measured on the MI355X: see DESIGN.md section 8f."""
import os

import numpy as np
import pytest

import drop_reference as dr
from ipx_amd import synth
from test_drop_reference import DROP_TOL, PLANTED
from test_gpu_finish import (FEAS_TOL, REF_BIN, assert_bounds_postprocessed, general_lp, restate_drop, row_sum_scale, run_reference,
                             with_identity)

pytestmark = pytest.mark.gpu

E_ARGUMENT = -3
KEYS = ("x", "xl", "xu", "y", "zl", "zu")


@pytest.fixture(scope="module")
def kkt():
    from ipx_amd import kkt as k
    k.load_library()
    return k


def matrix_of(P):
    return synth.CscMatrix(P["m"], P["n"], P["Ap"], P["Ai"], P["Ax"])


def on_slack_basis(kkt, P, drop_primal, drop_dual, A=None):
    """the planted iterate, the starting basis (the slack basis: no free variable is nonbasic, no fixed slack basic), the tolerances"""
    m, n = P["m"], P["n"]
    ctx = kkt.KktContext(A if A is not None else matrix_of(P))
    ctx.iterate_set(P["it"], P["state"])
    sb = ctx.ipm_starting_basis(P["b"], P["c"], P["lb"], P["ub"])
    assert sb["errflag"] == 0 and sb["updates_start"] == 0 and np.array_equal(sb["basis"], np.arange(n, n + m))
    ctx.ipm_set_drop_tolerances(drop_primal, drop_dual)
    return ctx, sb


def drop_on_slack_basis(kkt, P, drop_primal, drop_dual, A=None, interrupt=None):
    """... and one pass"""
    ctx, sb = on_slack_basis(kkt, P, drop_primal, drop_dual, A)
    g = ctx.ipm_drop_degenerate(P["b"], P["c"], P["lb"], P["ub"], interrupt=interrupt)
    return ctx, sb, g


class StopAt:
    """an interrupt callback that returns 999 from its k-th call on"""
    def __init__(self, k):
        self.k, self.calls = k, 0

    def __call__(self):
        self.calls += 1
        return 999 if self.calls >= self.k else 0


# ---- 1. decisions ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted():
    out = {}
    for m, n, seed in PLANTED:
        P = dr.planted_state(m, n, seed)
        out[(m, n)] = (P, dr.restatement(P, DROP_TOL, DROP_TOL))
    return out


@pytest.mark.parametrize("m,n,seed", PLANTED)
def test_decisions_follow_the_restatement(kkt, planted, m, n, seed):
    P, R = planted[(m, n)]
    runs = []
    for _ in range(2):                                          # a second context from the same state: the same bits
        ctx, sb, g = drop_on_slack_basis(kkt, P, DROP_TOL, DROP_TOL)
        assert np.array_equal(sb["status"], P["status"])
        it, st = ctx.iterate_get(), ctx.iterate_get_state()
        runs.append((g, it, st))
        ctx.close()
    g, it, st = runs[0]
    print({k: v for k, v in g.items() if np.isscalar(v)})
    assert g["errflag"] == 0 and g["refused"] == 0
    assert g["log"].tolist() == [list(e) for e in R["log"]]
    acts = [a for _, a, _ in R["log"]]
    assert g["updates"] == acts.count(dr.EXCHANGED) and g["dual_dropped"] == acts.count(dr.FIXED)
    assert g["primal_dropped"] == acts.count(dr.IMPLIED_LB) + acts.count(dr.IMPLIED_UB)
    assert np.array_equal(g["basis"], R["basis"]) and np.array_equal(g["status"], R["status"])
    assert np.array_equal(st, R["state"])
    for k in ("xl", "xu", "zl", "zu", "x", "y"):                # copies, zeros and infinities
        assert np.array_equal(it[k], R["it"][k]), k
    assert np.array_equal(g["colscale"], R["colscale"])          # read back from the device after the pass
    g2, it2, st2 = runs[1]
    assert g2["colscale"].tobytes() == g["colscale"].tobytes()
    assert g2["log"].tobytes() == g["log"].tobytes() and g2["basis"].tobytes() == g["basis"].tobytes()
    assert g2["status"].tobytes() == g["status"].tobytes() and st2.tobytes() == st.tobytes()
    for k in KEYS:
        assert it2[k].tobytes() == it[k].tobytes(), k


def test_gate_and_preconditions(kkt):
    m, n, seed = PLANTED[0]
    P = dr.planted_state(m, n, seed, gate_open=False)
    ctx, sb, g = drop_on_slack_basis(kkt, P, DROP_TOL, DROP_TOL)
    assert len(g["log"]) == 0 and g["primal_candidates"] == 0 and g["dual_candidates"] == 0
    assert np.array_equal(ctx.iterate_get_state(), P["state"]) and np.array_equal(g["status"], P["status"])
    # no live basis after a new iterate; bad tolerances
    ctx.iterate_set(P["it"], P["state"])
    with pytest.raises(kkt.KktError, match="no live basis") as e:
        ctx.ipm_drop_degenerate(P["b"], P["c"], P["lb"], P["ub"])
    assert e.value.code == E_ARGUMENT
    for bad in ((-1.0, 0.0), (0.0, np.inf), (np.nan, 0.0)):
        with pytest.raises(kkt.KktError, match="drop tolerances") as e:
            ctx.ipm_set_drop_tolerances(*bad)
        assert e.value.code == E_ARGUMENT
    ctx.close()


def decided_so_far(P, R, k):
    """status and state after the first k decisions of the restatement's log (the basis exchanges included)"""
    n = P["n"]
    status, state = P["status"].copy(), P["state"].copy()
    for j, a, partner in R["log"][:k]:
        if a == dr.EXCHANGED:
            jb, jn = (j, partner) if P["status"][j] == dr.BASIC else (partner, j)
            status[jn], status[jb] = dr.BASIC, dr.NONBASIC
        elif a == dr.FIXED:
            status[j], state[j] = dr.NONBASIC_FIXED, dr.ST_FIXED
        else:
            status[j], state[j] = dr.BASIC_FREE, dr.ST_IMPLIED_LB if a == dr.IMPLIED_LB else dr.ST_IMPLIED_UB
    return status, state


@pytest.mark.parametrize("where", ["pass", "driver"])
def test_interrupt_inside_the_pass(kkt, planted, where):
    """The callback returns 999 at a candidate that follows an exchange and a drop.  What was decided stays (as in the reference),
    the errflag is reported, the context holds the operator of the basis returned (a step on it works), and nothing goes on from
    that basis: the next pass is refused.  Inside ipxk_ipm_driver_basis the same interrupt ends the phase as a time limit."""
    P, R = planted[PLANTED[0][:2]]
    b, c, lb, ub = P["b"], P["c"], P["lb"], P["ub"]
    acts = [a for _, a, _ in R["log"]]
    k = max(acts.index(dr.EXCHANGED), min(acts.index(dr.IMPLIED_LB), acts.index(dr.IMPLIED_UB))) + 1     # decisions before the stop
    assert 2 <= k < len(acts) and dr.EXCHANGED in acts[:k]
    want_status, want_state = decided_so_far(P, R, k)
    if where == "pass":
        cb = StopAt(k + 1)                                      # one poll per candidate
        ctx, sb, g = drop_on_slack_basis(kkt, P, DROP_TOL, DROP_TOL, interrupt=cb)
        assert g["errflag"] == 999 and g["refused"] == 0
        assert g["log"].tolist() == [list(e) for e in R["log"][:k]]
        assert np.array_equal(g["status"], want_status)
        assert sorted(g["basis"].tolist()) == np.nonzero(want_status >= 0)[0].tolist()
        for j, a, _ in R["log"][:k]:
            if a != dr.EXCHANGED:
                assert g["colscale"][j] == (0.0 if a == dr.FIXED else np.inf)
        later = [j for j, a, _ in R["log"][k:] if a != dr.EXCHANGED]
        assert np.isfinite(g["colscale"][later]).all() and (g["colscale"][later] > 0).all()
    else:
        cb = StopAt(k + 2)                                      # the driver's own poll comes first
        ctx, sb = on_slack_basis(kkt, P, DROP_TOL, DROP_TOL)
        g = ctx.ipm_driver_basis(b, c, lb, ub, interrupt=cb)
        assert g["status_ipm"] == 5 and g["errflag"] == 0 and g["iter"] == 0, g
        counts = ctx.ipm_drop_counts()
        assert sum(counts) == k and counts[2] == acts[:k].count(dr.EXCHANGED) and g["basis_updates"] == counts[2]
    assert np.array_equal(ctx.iterate_get_state(), want_state)  # variables already dropped stay dropped
    with pytest.raises(kkt.KktError, match="no live basis") as e:
        ctx.ipm_drop_degenerate(b, c, lb, ub)
    assert e.value.code == E_ARGUMENT
    if where == "pass":
        # the factors are those of the basis returned, not of the slack basis the pass started from: B w through them gives w.
        # (No step is taken here: half way through the pass the planted state still holds the degenerate variables that make
        # the preconditioned system ill conditioned -- CR ends with 201 on it, whatever the factors.)
        B = dr.dense_AI(P)[:, g["basis"]]
        assert not np.array_equal(g["basis"], sb["basis"])
        assert np.linalg.cond(B) < 1e4
        w = np.random.default_rng(9).uniform(0.5, 2.0, P["m"])
        for trans, M in (("N", B), ("T", B.T)):
            got = ctx.solve_dense(M @ w, trans)
            assert np.abs(got - w).max() <= 1e-9 * np.linalg.cond(B), trans
    else:
        # no starting basis is live any more: the phase would have to build the slack basis, which it refuses with dropped variables
        with pytest.raises(kkt.KktError, match="barrier variables only"):
            ctx.ipm_driver_basis(b, c, lb, ub, ipm_maxiter=1)
    ctx.close()


def test_pass_on_the_basis_the_driver_leaves(kkt):
    """no starting basis: ipxk_ipm_driver_basis builds the slack basis itself, stops at its iteration limit and leaves its basis --
    with Maxvolume's last exchanges possibly kept as etas behind the factors -- for one pass; the operator the pass leaves serves a
    step"""
    P = degenerate_lp(300, 700, 2, eq_share=0.0)              # barrier variables only: the driver builds the slack basis
    m, n = P["m"], P["n"]
    b, c, lb, ub = P["b"], P["c"], P["lb"], P["ub"]
    ctx = kkt.KktContext(P["A"])
    assert ctx.ipm_starting_point(b, c, lb, ub)["status_ipm"] == 0
    assert ctx.ipm_driver(b, c, lb, ub, kkt_maxiter=5000, ipm_maxiter=4)["status_ipm"] in (1, 6)
    g = ctx.ipm_driver_basis(b, c, lb, ub, ipm_maxiter=10)
    assert g["status_ipm"] in (1, 6) and g["errflag"] == 0, g
    ctx.ipm_set_drop_tolerances(1e-2, 1e-2)
    d = ctx.ipm_drop_degenerate(b, c, lb, ub)
    print("after %d + %d iterations, mu %.2e, objectives %s:" % (4, g["iter"], g["mu"], ctx.iterate_objectives(b, c, lb, ub)),
          {k: v for k, v in d.items() if np.isscalar(v)})
    assert d["errflag"] == 0
    assert d["primal_candidates"] + d["dual_candidates"] >= 1, "input fault: nothing to drop after these iterations"
    assert len(d["log"]) == d["updates"] + d["primal_dropped"] + d["dual_dropped"]
    basis, status, st = d["basis"], d["status"], ctx.iterate_get_state()
    assert sorted(basis.tolist()) == np.nonzero(status >= 0)[0].tolist() and len(basis) == m
    for j, a, partner in d["log"].tolist():
        if a == dr.EXCHANGED:                                   # (either variable may be met again by a later candidate)
            assert 0 <= partner < n + m and partner != j
        elif a == dr.FIXED:
            assert status[j] == dr.NONBASIC_FIXED and st[j] == dr.ST_FIXED
        else:
            assert status[j] == dr.BASIC_FREE and st[j] == (dr.ST_IMPLIED_LB if a == dr.IMPLIED_LB else dr.ST_IMPLIED_UB)
    unchanged = np.setdiff1d(np.arange(n + m), d["log"][:, 0])
    moved = np.concatenate([d["log"][:, 0], d["log"][:, 2][d["log"][:, 2] >= 0]])
    assert np.array_equal(np.delete(status, moved), np.delete(g["status"], moved)) and len(unchanged) > 0
    s = ctx.ipm_step(True, b, c, lb, ub)
    assert s["errflag"] == 0 and s["step_primal"] > 0 and s["step_dual"] > 0
    ctx.close()


# ---- 2. ties and grid passes -----------------------------------------------------------------------------------------------
def expected_from_log(P):
    m, n = P["m"], P["n"]
    basis = np.arange(n, n + m)
    status = np.concatenate([np.full(n, dr.NONBASIC), np.full(m, dr.BASIC)])
    status[(P["lb"] == P["ub"])] = dr.NONBASIC_FIXED             # (structural: the starting basis leaves them nonbasic)
    status[np.isinf(P["lb"]) & np.isinf(P["ub"])] = dr.BASIC_FREE     # (free slacks stay basic)
    state = P["state"].copy()
    state[P["lb"] == P["ub"]] = dr.ST_FIXED
    for j, a, partner in P["expected_log"]:
        if a == dr.EXCHANGED:
            jb, jn = (j, partner) if j >= n else (partner, j)   # DropPrimal logs the leaving, DropDual the entering variable
            basis[jb - n] = jn
            status[jn], status[jb] = dr.BASIC, dr.NONBASIC
        elif a == dr.FIXED:
            status[j], state[j] = dr.NONBASIC_FIXED, dr.ST_FIXED
        else:
            status[j], state[j] = dr.BASIC_FREE, dr.ST_IMPLIED_LB if a == dr.IMPLIED_LB else dr.ST_IMPLIED_UB
    return basis, status, state


@pytest.mark.parametrize("which", ["row", "column"])
def test_searches_at_ties_and_past_the_grid(kkt, which):
    P = dr.row_search_case(7) if which == "row" else dr.column_search_case(8)
    tol = (dr.DROP_TOL, 0.0) if which == "row" else (0.0, dr.DROP_TOL)
    ctx, sb, g = drop_on_slack_basis(kkt, P, *tol)
    st = ctx.iterate_get_state()
    ctx.close()
    print({k: v for k, v in g.items() if np.isscalar(v)})
    assert g["errflag"] == 0 and g["refused"] == 0
    got = [tuple(e) for e in g["log"].tolist()]
    for want, have in zip(P["expected_log"], got):
        cls = [c["kind"] for c in P["classes"] if (P["n"] + c["row"] if which == "row" else c["col"]) == want[0]]
        assert have == want, (cls, want, have)
    assert len(got) == len(P["expected_log"])
    basis, status, state = expected_from_log(P)
    assert np.array_equal(g["basis"], basis) and np.array_equal(g["status"], status) and np.array_equal(st, state)
    assert (g["primal_candidates"], g["dual_candidates"]) == ((len(got), 0) if which == "row" else (0, len(got)))


# ---- 3. an iterate with implied states ---------------------------------------------------------------------------------------
def longdouble_evaluation(P, it, state):
    """residuals, objectives with the offset and complementarity in long double (src/iterate.cc:536-670)"""
    L = np.longdouble
    n, m = P["n"], P["m"]
    AI = dr.dense_AI(P).astype(L)
    x, y, xl, xu, zl, zu = (it[k].astype(L) for k in ("x", "y", "xl", "xu", "zl", "zu"))
    b, c, lb, ub = (P[k].astype(L) for k in ("b", "c", "lb", "ub"))
    has_lb, has_ub = (state == dr.ST_LB) | (state == dr.ST_BOXED), (state == dr.ST_UB) | (state == dr.ST_BOXED)
    fixed, implied = state == dr.ST_FIXED, (state == dr.ST_IMPLIED_LB) | (state == dr.ST_IMPLIED_UB)
    with np.errstate(invalid="ignore"):
        rc = np.where(fixed, 0.0, c - AI.T @ y - zl + zu)
        rl = np.where(has_lb, lb - x + xl, 0.0)
        ru = np.where(has_ub, ub - x - xu, 0.0)
        shift = np.where(implied, (zl - zu) * x, 0.0)
        pterms = np.concatenate([np.where(fixed, 0.0, c * x), -shift])
        oterms = np.concatenate([np.where(fixed, c * x, 0.0), shift])
        dterms = np.concatenate([b * y, np.where(has_lb, lb * zl, 0.0), -np.where(has_ub, ub * zu, 0.0),
                                 -np.where(fixed, x * (AI.T @ y), 0.0)])
        comp = np.concatenate([(xl * zl)[has_lb], (xu * zu)[has_ub]])
    return dict(rb=b - AI @ x, rc=rc, rl=rl, ru=ru, pobj=pterms.sum(), offset=oterms.sum(), dobj=dterms.sum(),
                pscale=np.abs(pterms).sum(), oscale=np.abs(oterms).sum(), dscale=np.abs(dterms).sum(), comp=comp.sum(), nterms=len(comp))


def restate_postprocess_implied(P, it, state):
    """src/iterate.cc:250-313 with the implied states (:294-308)"""
    AI = dr.dense_AI(P)
    lb, ub, c = P["lb"], P["ub"], P["c"]
    out = {k: v.copy() for k, v in it.items()}
    z = c - AI.T @ it["y"]
    fx, il, iu = state == dr.ST_FIXED, state == dr.ST_IMPLIED_LB, state == dr.ST_IMPLIED_UB
    with np.errstate(invalid="ignore"):
        out["xl"][fx], out["xu"][fx] = (it["x"] - lb)[fx], (ub - it["x"])[fx]
        out["zl"][il], out["zu"][il], out["x"][il] = z[il], 0.0, lb[il]
        out["zl"][iu], out["zu"][iu], out["x"][iu] = 0.0, -z[iu], ub[iu]
        sel = il | iu
        out["xl"][sel], out["xu"][sel] = (out["x"] - lb)[sel], (ub - out["x"])[sel]
    return out, fx | sel


def test_iterate_with_implied_states(kkt, planted):
    P, R = planted[PLANTED[1][:2]]
    m, n = P["m"], P["n"]
    b, c, lb, ub = P["b"], P["c"], P["lb"], P["ub"]
    it, state = R["it"], R["state"]
    il, iu = state == dr.ST_IMPLIED_LB, state == dr.ST_IMPLIED_UB
    boxed_b = np.isfinite(lb) & np.isfinite(ub)
    assert (il & boxed_b).any() and (il & ~boxed_b).any() and (iu & boxed_b).any() and (iu & ~boxed_b).any()     # boxed and one-sided
    ctx = kkt.KktContext(matrix_of(P))
    ctx.iterate_set(it, state)
    assert np.array_equal(ctx.iterate_get_state(), state)
    W = longdouble_evaluation(P, it, state)
    AIs = with_identity(matrix_of(P).to_scipy(), m)
    r = ctx.iterate_residuals(b, c, lb, ub)
    has_lb, has_ub = (state == dr.ST_LB) | (state == dr.ST_BOXED), (state == dr.ST_UB) | (state == dr.ST_BOXED)
    with np.errstate(invalid="ignore"):                           # two operations per entry, in the kernel's order
        assert np.array_equal(r["rl"], np.where(has_lb, lb - it["x"] + it["xl"], 0.0))
        assert np.array_equal(r["ru"], np.where(has_ub, ub - it["x"] - it["xu"], 0.0))
    assert np.abs(r["rl"] - W["rl"].astype(np.float64)).max() <= 1e-12 * (1.0 + np.abs(it["x"]).max())
    assert not r["rl"][il | iu].any() and not r["ru"][il | iu].any()
    scale = row_sum_scale(AIs, c, it["y"]) + it["zl"] + it["zu"]
    assert (np.abs(r["rc"] - W["rc"]) <= 1e-12 * scale).all()
    assert np.abs(r["rc"][il | iu]).max() > 0                       # rc keeps (c - zl) + zu - a'y on implied variables
    bscale = np.abs(b) + abs(AIs) @ np.abs(it["x"])
    assert (np.abs(r["rb"] - W["rb"]) <= 1e-12 * bscale).all()
    pobj, dobj, offset = ctx.iterate_objectives(b, c, lb, ub)
    print("objectives", pobj, dobj, offset, "long double", W["pobj"], W["dobj"], W["offset"])
    assert abs(pobj - W["pobj"]) <= 1e-12 * W["pscale"] and abs(dobj - W["dobj"]) <= 1e-12 * W["dscale"]
    assert abs(offset - W["offset"]) <= 1e-12 * W["oscale"] and W["oscale"] > 0
    comp = ctx.iterate_complementarity()
    assert abs(comp["complementarity"] - float(W["comp"])) <= 1e-13 * float(W["comp"])
    assert abs(comp["mu"] - float(W["comp"] / W["nterms"])) <= 1e-13 * float(W["comp"] / W["nterms"])
    # one step of the main phase on the basis the pass has left: the implied variables move like free ones (xl, xu, zl, zu keep
    # their bits), the fixed ones keep x
    ctx.close()
    ctx, sb, g = drop_on_slack_basis(kkt, P, DROP_TOL, DROP_TOL)
    before = ctx.iterate_get()
    assert np.array_equal(ctx.iterate_get_state(), state)
    # the scaling factors as the device holds them after the pass, against the host formula on the final iterate
    assert np.array_equal(g["colscale"], dr.scaling_factors(it, state))
    assert np.isinf(g["colscale"][il | iu]).all() and (g["colscale"][state == dr.ST_FIXED] == 0).all()
    # the step is taken against a perturbed b and c, so that there are residuals to reduce
    rng = np.random.default_rng(5)
    b2, c2 = b + rng.uniform(-1.0, 1.0, m), c + rng.uniform(-1.0, 1.0, n + m)
    r0 = ctx.iterate_residuals(b2, c2, lb, ub)
    s = ctx.ipm_step(True, b2, c2, lb, ub)
    print(s)
    assert s["errflag"] == 0 and 0.0 < s["step_primal"] <= 1.0 and 0.0 < s["step_dual"] <= 1.0
    r1 = ctx.iterate_residuals(b2, c2, lb, ub)
    # a damped Newton step reduces the linear residuals by (1 - step) up to the KKT tolerance (test_ipm_step_with_basis_solver) ...
    assert r1["presidual"] < r0["presidual"] and r1["dresidual"] < r0["dresidual"]
    # ... and exactly so where the basis solver is exact: rb (x_B is solved for from b - N x_N) and the dual equation of a basic
    # free variable, which is what an implied variable must be to the Newton system (its zl, zu do not move)
    sp, sd = s["step_primal"], s["step_dual"]
    y1 = ctx.iterate_get()["y"]
    bs = np.abs(b2) + abs(AIs) @ np.abs(before["x"])
    assert (np.abs(r1["rb"] - (1.0 - sp) * r0["rb"]) <= 1e-9 * bs).all()
    imp = il | iu
    cs = row_sum_scale(AIs, c2, y1) + row_sum_scale(AIs, c2, it["y"]) + it["zl"] + it["zu"]
    assert np.abs(r0["rc"][imp]).max() > 1e-3
    assert (np.abs(r1["rc"][imp] - (1.0 - sd) * r0["rc"][imp]) <= 1e-9 * cs[imp]).all()
    after = ctx.iterate_get()
    fx = state == dr.ST_FIXED
    for k in ("xl", "xu", "zl", "zu"):
        assert np.array_equal(after[k][il | iu | fx], before[k][il | iu | fx]), k
    assert np.array_equal(after["x"][fx], before["x"][fx]) and not np.array_equal(after["x"][il | iu], before["x"][il | iu])
    bar = ~(il | iu | fx)
    assert (after["xl"][bar] > 0).all() and (after["xu"][bar] > 0).all() and not np.array_equal(after["zl"][bar], before["zl"][bar])
    # postprocess (:294-308) and the drop to complementarity
    ctx.iterate_set(it, state)
    ctx.iterate_postprocess(c, lb, ub)
    got = ctx.iterate_get()
    want, touched = restate_postprocess_implied(P, it, state)
    for k in ("x", "xl", "xu", "y"):
        assert np.array_equal(got[k], want[k]), k
    assert (got["xl"][il] == 0).all() and (got["xu"][iu] == 0).all() and (got["xl"][touched] >= 0).all() and (got["xu"][touched] >= 0).all()
    zscale = row_sum_scale(AIs, c, it["y"])
    for k in ("zl", "zu"):
        assert (np.abs(got[k] - want[k]) <= 1e-12 * zscale).all(), k
        assert np.array_equal(got[k] == 0.0, want[k] == 0.0), k
        assert got[k][~touched].tobytes() == np.ascontiguousarray(it[k][~touched]).tobytes(), k
    x, y, z = ctx.iterate_drop_to_complementarity(lb, ub)
    wx, wy, wz, _ = restate_drop(lb, ub, got)
    assert np.array_equal(x, wx) and np.array_equal(y, wy) and np.array_equal(z, wz)
    # ipxk_iterate_set: the conditions of Iterate::assert_consistency, the first offending index
    first, second = np.nonzero(il | iu)[0][:2]
    for key, value in (("xl", 1.0), ("xu", 2.0), ("zl", -1.0), ("zu", np.nan)):
        bad = {k: v.copy() for k, v in it.items()}
        bad[key][second] = value
        bad[key][first] = value
        with pytest.raises(kkt.KktError, match=r"variable %d is in an implied state" % first) as e:
            ctx.iterate_set(bad, state)
        assert e.value.code == E_ARGUMENT
    # the bound a variable is implied at must be finite: ipxk_iterate_set does not see the bounds, the postprocess does and
    # refuses before it writes anything
    j = int(np.nonzero(iu & ~boxed_b)[0][0])                      # upper bound only: lb = -inf
    wrong = state.copy()
    wrong[j] = dr.ST_IMPLIED_LB
    ctx.iterate_set(it, wrong)
    with pytest.raises(kkt.KktError, match=r"variable %d is implied at an infinite bound" % j) as e:
        ctx.iterate_postprocess(c, lb, ub)
    assert e.value.code == E_ARGUMENT
    same = ctx.iterate_get()
    for k in KEYS:
        assert same[k].tobytes() == np.ascontiguousarray(it[k]).tobytes(), k
    ctx.close()


# ---- 4. off means untouched ----------------------------------------------------------------------------------------------------
def test_off_means_untouched(kkt):
    P = general_lp(60, 150, 1, dep=2)
    b, c, lb, ub = P["b"], P["c"], P["lb"], P["ub"]
    runs = []
    for tol in (None, (0.0, 0.0), (1e-300, 1e-300)):
        ctx = kkt.KktContext(P["A"])
        if tol is not None:
            ctx.ipm_set_drop_tolerances(*tol)
        g = ctx.ipm_solve(b, c, lb, ub)
        runs.append((g, ctx.iterate_get(), ctx.iterate_get_state(), ctx.ipm_drop_counts()))
        ctx.close()
    g0, it0, st0, counts0 = runs[0]
    assert g0["status_ipm"] == 1 and counts0 == (0, 0, 0)
    for g, it, st, counts in runs[1:]:
        assert counts == (0, 0, 0)
        for k in KEYS:
            assert it[k].tobytes() == it0[k].tobytes(), k
        assert st.tobytes() == st0.tobytes()
        for k, v in g.items():
            if np.isscalar(v):
                assert v == g0[k], k
            else:
                assert np.array_equal(v, g0[k]), k


# ---- 5. end to end against the reference's LpSolver -----------------------------------------------------------------------------
def degenerate_lp(m, n, seed, eq_share=0.3):
    """A primal and dual degenerate LP with a planted optimal pair: about m/4 positive structurals and m/4 positive slacks (m/2
    positive basics, so every optimal basis holds variables at a bound), reduced costs positive on only 60 % of the columns at 0
    (fewer than n - m), 30 % '=' rows unless eq_share says otherwise.  6 entries per column, +-U[0.5, 4); all structurals have lb = 0, ub = inf."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    k = 6
    rows = np.concatenate([rng.choice(m, k, replace=False) for _ in range(n)])
    cols = np.repeat(np.arange(n), k)
    vals = rng.choice([-1.0, 1.0], n * k) * rng.uniform(0.5, 4.0, n * k)
    A = sp.csc_matrix((vals, (rows, cols)), shape=(m, n))
    A.sort_indices()
    eq = rng.random(m) < eq_share
    support = rng.choice(n, m // 4, replace=False)
    x0 = np.zeros(n)
    x0[support] = rng.uniform(0.5, 2.0, len(support))
    loose = ~eq & (rng.random(m) < (m / 4.0) / max((~eq).sum(), 1))
    s0 = np.where(loose, rng.uniform(0.5, 2.0, m), 0.0)
    b = A @ x0 + s0
    y0 = np.where(eq, rng.uniform(-1.5, 1.5, m), np.where(loose, 0.0, -rng.uniform(0.5, 1.5, m)))
    z = np.where(rng.random(n) < 0.6, rng.uniform(0.5, 2.0, n), 0.0)
    z[support] = 0.0
    c = A.T @ y0 + z
    assert (x0 > 0).sum() + (s0 > 0).sum() <= 0.6 * m and (z > 0).sum() < n - m
    M = synth.CscMatrix(m, n, A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.copy())
    return dict(A=M, S=A, b=b, c=np.concatenate([c, np.zeros(m)]), lb=np.zeros(n + m), ub=np.concatenate([np.full(n, np.inf), np.where(eq, 0.0, np.inf)]),
                eq=eq, m=m, n=n, fopt=float(c @ x0))


# the first seed of 1..8 on which the reference itself drops a variable (all eight do).  Reference on seed 1 at 1e-6: 18 iterations,
# primal_dropped 142, dual_dropped 1, updates_ipm 341; the device: 20 iterations (2 initial), 144 and 1, 343 basis updates
DEGENERATE_SEED = 1
DEGENERATE_TOL = 1e-6
REF_PARAMS = "ipm_drop_primal %g\nipm_drop_dual %g\n" % (DEGENERATE_TOL, DEGENERATE_TOL)


def test_degenerate_lp_against_the_reference(kkt, tmp_path):
    if not os.path.exists(REF_BIN):
        pytest.skip("oracle/_ref/test_lp_{ref,hip} not built (needs the reference sources at build time)")
    m, n = 300, 700
    P = degenerate_lp(m, n, DEGENERATE_SEED)
    b, c, lb, ub = P["b"], P["c"], P["lb"], P["ub"]
    ref = run_reference(P, tmp_path, REF_PARAMS)
    print("reference: status %d, iter %d, primal_dropped %d, dual_dropped %d, updates_ipm %d"
          % (ref["status_ipm"], ref["iter"], ref["primal_dropped"], ref["dual_dropped"], ref["updates_ipm"]))
    assert ref["primal_dropped"] + ref["dual_dropped"] >= 1, "input fault: the reference drops nothing on this seed"
    ctx = kkt.KktContext(P["A"])
    ctx.ipm_set_drop_tolerances(DEGENERATE_TOL, DEGENERATE_TOL)
    g = ctx.ipm_solve(b, c, lb, ub)
    counts = ctx.ipm_drop_counts()
    it, st = ctx.iterate_get(), ctx.iterate_get_state()
    ctx.close()
    print("device: status %d, iter %d (%d initial), primal_dropped %d, dual_dropped %d, drop exchanges %d, basis_updates %d"
          % ((g["status_ipm"], g["iter"], g["iter_initial"]) + counts + (g["basis_updates"],)))
    assert ref["status_ipm"] == 1 and g["status_ipm"] == 1
    assert counts[0] + counts[1] >= 1
    assert abs(g["pobjective"] - ref["pobjval"]) <= 1e-6 * (1.0 + abs(ref["pobjval"]))
    print("device", g["rel_presidual"], g["rel_dresidual"], g["rel_objgap"])
    assert g["rel_presidual"] <= FEAS_TOL and g["rel_dresidual"] <= FEAS_TOL and abs(g["rel_objgap"]) <= 1e-8
    # postprocessed: no variable is left implied or fixed with a bound residual
    assert_bounds_postprocessed(P, it, g["status"])
    sel = (st == dr.ST_IMPLIED_LB) | (st == dr.ST_IMPLIED_UB) | (st == dr.ST_FIXED)
    assert sel.sum() >= counts[0] + counts[1]
    with np.errstate(invalid="ignore"):
        assert np.array_equal(it["xl"][sel], (it["x"] - lb)[sel]) and np.array_equal(it["xu"][sel], (ub - it["x"])[sel])
    implied = (st == dr.ST_IMPLIED_LB) | (st == dr.ST_IMPLIED_UB)
    assert (it["xl"][implied] >= 0).all() and (it["xu"][implied] >= 0).all()
    assert (it["x"][st == dr.ST_IMPLIED_LB] == lb[st == dr.ST_IMPLIED_LB]).all() and (it["x"][st == dr.ST_IMPLIED_UB] == ub[st == dr.ST_IMPLIED_UB]).all()
