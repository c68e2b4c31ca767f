"""GPU: crossover in solver form on the device (crossover.hip): ipxk_crossover_push_dual / _push_primal / _basic_solution / _run.

1. the pushes on planted points against the dense restatement (tests/crossover_reference.py): pivot log and counts exactly, the
   exact invariants of a pushed point, x, y, z against the restatement run in long double;
2. the two ratio tests at exact ties, at their thresholds and past their grid passes (dyadic inputs: equality);
3. the basic solution against a dense long-double solve, and the basic statuses;
4. refusals, the interrupt, and the factors the context holds afterwards;
5. an LP end to end against the reference's LpSolver with crossover on.

Measured on the MI355X: see DESIGN.md section 8g."""
import os

import numpy as np
import pytest

import crossover_reference as cr
from helpers import relerr
from ipx_amd import synth
from test_crossover_reference import PLANTED, assert_vertex_invariants, dual_alone, fixed_at_bound_of, primal_alone
from test_gpu_drop import StopAt
from test_gpu_finish import REF_BIN, forced_context, general_lp, initial_states, run_reference

pytestmark = pytest.mark.gpu

E_ARGUMENT = -3
GATE = 1e-9                                      # the project's relative gate for solve outputs (the golden tests')
L = np.longdouble


@pytest.fixture(scope="module")
def kkt():
    from ipx_amd import kkt as k
    k.load_library()
    return k


def matrix_of(P):
    return synth.CscMatrix(P["m"], P["n"], P["Ap"], P["Ai"], P["Ax"])


@pytest.fixture(scope="module")
def planted():
    """per size: the point, and the restatement of each phase alone and of PushAll + the basic solution, in long double"""
    out = {}
    for m, n, seed in PLANTED:
        P = cr.planted_point(m, n, seed)
        out[(m, n)] = dict(P=P, dual=dual_alone(P, L=L), primal=primal_alone(P, L=L), run=cr.push_all(P, P["weights"], L=L))
    return out


def interior_iterate(P):
    """a postprocessed iterate whose DropToComplementarity is the planted point, bit for bit: z_j != 0 at a bound is an active
    barrier term (zl >= xl resp. zu >= xu), z_j = 0 an inactive one (x is kept, z becomes 0)"""
    lb, ub, x, z = P["lb"], P["ub"], P["x"], P["z"]
    fl, fu = np.isfinite(lb), np.isfinite(ub)
    xl, xu = np.where(fl, 1.0, np.inf), np.where(fu, 1.0, np.inf)
    zl, zu = np.zeros(len(x)), np.zeros(len(x))
    pos, neg = z > 0, z < 0
    xl[pos], zl[pos], xu[pos & fu] = 0.01, z[pos], 10.0
    xu[neg], zu[neg], xl[neg] = 0.01, -z[neg], 10.0
    return dict(x=x.copy(), xl=xl, xu=xu, y=P["y"].copy(), zl=zl, zu=zu), initial_states(lb, ub)


def assert_close(got, want, what):
    err = relerr(got, np.asarray(want, np.float64))
    print("%s: relative deviation from the long-double restatement %.3e" % (what, err))
    assert err < GATE, (what, err)
    return err


# ---- 1. the pushes follow the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,seed", PLANTED)
def test_dual_pushes_follow_the_restatement(kkt, planted, m, n, seed):
    P, R = planted[(m, n)]["P"], planted[(m, n)]["dual"]
    lb, ub = P["lb"], P["ub"]
    runs = []
    for _ in range(2):
        ctx = kkt.KktContext(matrix_of(P))
        runs.append(ctx.crossover_push_dual(lb, ub, P["x"], P["y"], P["z"], R["variables"], P["basis"]))
        ctx.close()
    g = runs[0]
    print({k: v for k, v in g.items() if np.isscalar(v)})
    assert g["errflag"] == 0 and g["status_crossover"] == 1 and g["refused"] == 0
    assert [tuple(e) for e in g["log"].tolist()] == R["log"]
    assert (g["dual_pushes"], g["dual_pivots"], g["dual_superbasics"]) == (R["pushes"], R["pivots"], len(R["variables"]))
    assert np.array_equal(g["basis"], R["basis"])
    assert (g["z"][g["basis"]] == 0).all() and cr.dual_infeasibility(lb, ub, P["x"], g["z"]) == 0
    assert_close(g["y"], R["y"], "dual push %dx%d y" % (m, n))
    assert_close(g["z"], R["z"], "dual push %dx%d z" % (m, n))
    for k in ("y", "z", "basis", "log"):
        assert runs[1][k].tobytes() == g[k].tobytes(), k


@pytest.mark.parametrize("m,n,seed", PLANTED)
def test_primal_pushes_follow_the_restatement(kkt, planted, m, n, seed):
    P, R = planted[(m, n)]["P"], planted[(m, n)]["primal"]
    lb, ub = P["lb"], P["ub"]
    runs = []
    for _ in range(2):
        ctx = kkt.KktContext(matrix_of(P))
        runs.append(ctx.crossover_push_primal(lb, ub, P["x"], R["variables"], P["basis"], fixed_at_bound=fixed_at_bound_of(P)))
        ctx.close()
    g = runs[0]
    print({k: v for k, v in g.items() if np.isscalar(v)})
    assert g["errflag"] == 0 and g["status_crossover"] == 1 and g["refused"] == 0
    assert [tuple(e) for e in g["log"].tolist()] == R["log"]
    assert (g["primal_pushes"], g["primal_pivots"]) == (R["pushes"], R["pivots"])
    assert np.array_equal(g["basis"], R["basis"])
    x = g["x"]
    nonbasic = np.setdiff1d(np.arange(n + m), g["basis"])
    free = np.isinf(lb) & np.isinf(ub)
    assert ((x[nonbasic] == lb[nonbasic]) | (x[nonbasic] == ub[nonbasic]) | (free[nonbasic] & (x[nonbasic] == 0))).all()
    assert (x >= lb).all() and (x <= ub).all() and cr.primal_infeasibility(lb, ub, x) == 0
    fixed = fixed_at_bound_of(P).astype(bool)
    assert np.array_equal(x[fixed], P["x"][fixed])                  # a fixed-at-bound variable blocks with step 0
    assert_close(x, R["x"], "primal push %dx%d x" % (m, n))
    for k in ("x", "basis", "log"):
        assert runs[1][k].tobytes() == g[k].tobytes(), k


@pytest.mark.parametrize("m,n,seed", PLANTED)
def test_run_follows_push_all(kkt, planted, m, n, seed):
    P, R = planted[(m, n)]["P"], planted[(m, n)]["run"]
    lb, ub, b, c = P["lb"], P["ub"], P["b"], P["c"]
    it, state = interior_iterate(P)
    runs = []
    for _ in range(2):
        ctx = kkt.KktContext(matrix_of(P))
        ctx.iterate_set(it, state)
        ctx.iterate_postprocess(c, lb, ub)
        x0, y0, z0 = ctx.iterate_drop_to_complementarity(lb, ub)
        assert np.array_equal(x0, P["x"]) and np.array_equal(y0, P["y"]) and np.array_equal(z0, P["z"])
        runs.append(ctx.crossover_run(b, c, lb, ub, P["basis"], weights=P["weights"]))
        ctx.close()
    g = runs[0]
    print({k: v for k, v in g.items() if np.isscalar(v)})
    assert g["errflag"] == 0 and g["status_crossover"] == 1 and g["refused"] == 0
    assert [tuple(e) for e in g["log"].tolist()] == R["log"]
    assert (g["dual_superbasics"], g["primal_superbasics"]) == (len(R["dual_superbasics"]), len(R["primal_superbasics"]))
    assert (g["dual_pushes"], g["dual_pivots"]) == (R["dual"]["pushes"], R["dual"]["pivots"])
    assert (g["primal_pushes"], g["primal_pivots"]) == (R["primal"]["pushes"], R["primal"]["pivots"])
    assert np.array_equal(g["basis"], R["basis"])
    # What stays exact through the basic solution: z_B = 0 and x_N at a bound (neither is recomputed).  x_B and z_N are: the two
    # infeasibilities are exactly 0 after the pushes (the two tests above assert that on each phase) but carry the rounding of
    # the dense solves here, as in the reference -- they are held to the gate of the solve outputs and to the host's own maxima.
    assert_vertex_invariants(P, g)
    assert g["primal_infeas"] == cr.primal_infeasibility(lb, ub, g["x"]) and g["dual_infeas"] == cr.dual_infeasibility(lb, ub, g["x"], g["z"])
    print("vertex %dx%d: primal infeasibility %.3e, dual infeasibility %.3e" % (m, n, g["primal_infeas"], g["dual_infeas"]))
    assert g["primal_infeas"] <= GATE * (1 + np.abs(g["x"]).max()) and g["dual_infeas"] <= GATE * (1 + np.abs(g["z"]).max())
    assert np.array_equal(g["basic_statuses"], R["statuses"])     # (no planted variable has lb == ub: x_N decides, and it is exact)
    for k in ("x", "y", "z"):
        assert_close(g[k], R[k], "run %dx%d %s" % (m, n, k))
    for k in ("x", "y", "z", "basis", "log", "basic_statuses"):
        assert runs[1][k].tobytes() == g[k].tobytes(), k


# ---- 2. ties and grid passes -----------------------------------------------------------------------------------------------
def test_dual_ratio_test_at_ties_and_past_the_grid(kkt):
    D = cr.dual_ratio_case(11)
    n = D["n"]
    ctx = kkt.KktContext(matrix_of(D))
    g = ctx.crossover_push_dual(D["lb"], D["ub"], D["x"], D["y"], D["z"], D["variables"], D["basis"], feastol=(D["feastol"], D["feastol"]))
    ctx.close()
    print({k: v for k, v in g.items() if np.isscalar(v)})
    assert g["errflag"] == 0 and g["status_crossover"] == 1 and g["refused"] == 0
    got = [tuple(e) for e in g["log"].tolist()]
    for c in D["classes"]:
        have = [jn for jb, jn in got if jb == n + c["row"]]
        assert have == ([c["winner"]] if c["winner"] >= 0 else []), (c["kind"], c["winner"], have)
        assert g["y"][c["row"]] == c["step"], (c["kind"], g["y"][c["row"]], c["step"])          # y started at 0: the step, exactly
        assert g["z"][n + c["row"]] == 1.0 - c["step"]
        if c["winner"] >= 0:
            assert g["z"][c["winner"]] == 0.0
    assert got == D["expected_log"]
    assert g["dual_pushes"] == len(D["classes"]) and g["dual_pivots"] == len(got)
    assert (g["z"][:n][D["ub"][:n] == np.inf] >= 0).all()


def test_primal_ratio_test_at_ties_and_past_the_grid(kkt):
    D = cr.primal_ratio_case(12)
    n = D["n"]
    ctx = kkt.KktContext(matrix_of(D))
    g = ctx.crossover_push_primal(D["lb"], D["ub"], D["x"], D["variables"], D["basis"], feastol=(D["feastol"], D["feastol"]))
    ctx.close()
    print({k: v for k, v in g.items() if np.isscalar(v)})
    assert g["errflag"] == 0 and g["status_crossover"] == 1 and g["refused"] == 0
    got = [tuple(e) for e in g["log"].tolist()]
    for c in D["classes"]:
        have = [jb for jb, jn in got if jn == c["col"]]
        assert have == ([n + c["winner"]] if c["winner"] >= 0 else []), (c["kind"], c["winner"], have)
        if c["winner"] >= 0:
            assert g["x"][n + c["winner"]] == (0.0 if c["at_lb"] else 4.0), c["kind"]          # block_at_lb
            assert g["x"][c["col"]] == 1.0 - c["step"], (c["kind"], g["x"][c["col"]], c["step"])
        else:
            assert g["x"][c["col"]] == 0.0
    assert got == D["expected_log"]
    assert g["primal_pushes"] == len(D["classes"]) and g["primal_pivots"] == len(got)
    assert (g["x"] >= D["lb"]).all() and (g["x"] <= D["ub"]).all()


# ---- 3. the basic solution ---------------------------------------------------------------------------------------------------
def test_basic_solution(kkt, planted):
    m, n, _ = PLANTED[1]
    P = planted[(m, n)]["P"]
    rng = np.random.default_rng(4)
    basis = P["basis"]
    nonbasic = np.setdiff1d(np.arange(n + m), basis)
    x, z = P["x"].copy(), P["z"].copy()
    x[basis], z[nonbasic] = rng.uniform(-1, 1, m), rng.uniform(-1, 1, n)            # overwritten by the call
    x[nonbasic] += rng.uniform(0.0, 0.5, n)                                         # x_N, z_B: as given, any values
    z[basis] += rng.uniform(-0.5, 0.5, m)
    ctx = kkt.KktContext(matrix_of(P))
    gx, gy, gz = ctx.crossover_basic_solution(P["b"], P["c"], basis, x, rng.uniform(-1, 1, m), z)
    ctx.close()
    assert gx[nonbasic].tobytes() == x[nonbasic].tobytes() and gz[basis].tobytes() == z[basis].tobytes()
    B = cr.DenseBasis(cr.dense_AI(P).astype(L), basis)
    wx, wy, wz = x.astype(L), np.zeros(m, L), z.astype(L)
    cr.basic_solution(B, P["b"].astype(L), P["c"].astype(L), wx, wy, wz)
    assert_close(gx[basis], wx[basis], "basic solution x_B")
    assert_close(gy, wy, "basic solution y")
    assert_close(gz[nonbasic], wz[nonbasic], "basic solution z_N")
    st = cr.basic_statuses(B, P["lb"], P["ub"], gx, gz)
    assert (st[basis] == 0).all() and (st[nonbasic] != 0).all()


# ---- 4. refusals and the interrupt -------------------------------------------------------------------------------------------
def test_argument_checks(kkt, planted):
    m, n, _ = PLANTED[0]
    P, Rd, Rp = (planted[(m, n)][k] for k in ("P", "dual", "primal"))
    lb, ub, basis = P["lb"], P["ub"], P["basis"]
    ctx = kkt.KktContext(matrix_of(P))

    def refused(match, call, *args, **kw):
        with pytest.raises(kkt.KktError, match=match) as e:
            call(*args, **kw)
        assert e.value.code == E_ARGUMENT

    nonbasic = np.setdiff1d(np.arange(n + m), basis)
    refused("not basic", ctx.crossover_push_dual, lb, ub, P["x"], P["y"], P["z"], [int(nonbasic[0])], basis)
    refused("not nonbasic", ctx.crossover_push_primal, lb, ub, P["x"], [int(basis[0])], basis)
    z = P["z"].copy()
    j = int(np.nonzero(z > 0)[0][0])
    z[j] = -z[j]
    refused("sign condition", ctx.crossover_push_dual, lb, ub, P["x"], P["y"], z, Rd["variables"], basis)
    x = P["x"].copy()
    x[int(np.nonzero(np.isfinite(lb))[0][0])] = -1.0
    refused("bound condition", ctx.crossover_push_primal, lb, ub, x, Rp["variables"], basis)
    fixed = np.zeros(n + m, np.uint8)
    fixed[Rp["variables"][0]] = 1                                   # a superbasic variable cannot be fixed at a bound
    refused("bound condition", ctx.crossover_push_primal, lb, ub, P["x"], Rp["variables"], basis, fixed_at_bound=fixed)
    twice = basis.copy()
    twice[1] = twice[0]
    refused("twice", ctx.crossover_push_primal, lb, ub, P["x"], [], twice)
    # run needs a postprocessed iterate
    refused("no iterate", ctx.crossover_run, P["b"], P["c"], lb, ub, basis)
    it, state = interior_iterate(P)
    ctx.iterate_set(it, state)
    refused("not been postprocessed", ctx.crossover_run, P["b"], P["c"], lb, ub, basis)
    ctx.close()


def test_refused_on_a_partitioned_context(kkt, planted, monkeypatch):
    m, n, _ = PLANTED[0]
    P, Rd, Rp = (planted[(m, n)][k] for k in ("P", "dual", "primal"))
    lb, ub, basis = P["lb"], P["ub"], P["basis"]
    ctx = forced_context(kkt, matrix_of(P), "direct", monkeypatch)
    calls = [lambda: ctx.crossover_push_dual(lb, ub, P["x"], P["y"], P["z"], Rd["variables"], basis),
             lambda: ctx.crossover_push_primal(lb, ub, P["x"], Rp["variables"], basis),
             lambda: ctx.crossover_basic_solution(P["b"], P["c"], basis, P["x"], P["y"], P["z"]),
             lambda: ctx.crossover_run(P["b"], P["c"], lb, ub, basis)]
    for call in calls:
        with pytest.raises(kkt.KktError, match="does not run on a partitioned system") as e:
            call()
        assert e.value.code == E_ARGUMENT
    ctx.close()


@pytest.mark.parametrize("phase", ["dual", "primal"])
def test_interrupt_inside_a_phase(kkt, planted, phase):
    """The callback returns 999 at candidate k + 1: status 5, errflag 0, the log is the beginning of the full run's, what has
    been pushed stays pushed and the point still satisfies the sign / bound conditions; the context holds the factors of the
    basis returned."""
    m, n, _ = PLANTED[0]
    P, R = planted[(m, n)]["P"], planted[(m, n)][phase]
    lb, ub = P["lb"], P["ub"]
    k = len(R["variables"]) // 2
    alone = dual_alone if phase == "dual" else primal_alone
    want = alone(P, stop_at=k + 1)
    assert want["status"] == 5 and 1 <= want["pivots"] < R["pivots"]
    ctx = kkt.KktContext(matrix_of(P))
    cb = StopAt(k + 1)
    if phase == "dual":
        g = ctx.crossover_push_dual(lb, ub, P["x"], P["y"], P["z"], R["variables"], P["basis"], interrupt=cb)
        x, z = P["x"], g["z"]
        assert (g["dual_pushes"], g["dual_pivots"]) == (want["pushes"], want["pivots"])
        assert relerr(z, want["z"]) < GATE
    else:
        g = ctx.crossover_push_primal(lb, ub, P["x"], R["variables"], P["basis"], fixed_at_bound=fixed_at_bound_of(P), interrupt=cb)
        x, z = g["x"], P["z"]
        assert (g["primal_pushes"], g["primal_pivots"]) == (want["pushes"], want["pivots"])
        assert relerr(x, want["x"]) < GATE
    assert cb.calls == k + 1
    assert g["status_crossover"] == 5 and g["errflag"] == 0
    got = [tuple(e) for e in g["log"].tolist()]
    assert got == want["log"] and got == R["log"][:len(got)]
    assert np.array_equal(g["basis"], want["basis"])
    assert (x >= lb).all() and (x <= ub).all() and cr.dual_infeasibility(lb, ub, x, z) == 0
    # the factors are those of the basis returned: B w through them gives w
    B = cr.dense_AI(P)[:, g["basis"]]
    w = np.random.default_rng(9).uniform(0.5, 2.0, m)
    for trans, M in (("N", B), ("T", B.T)):
        got_w = ctx.solve_dense(M @ w, trans)
        assert np.abs(got_w - w).max() <= 1e-9 * np.linalg.cond(B), trans
    ctx.close()


# ---- 5. end to end against the reference's LpSolver ----------------------------------------------------------------------------
def test_end_to_end_against_the_reference(kkt, tmp_path):
    """Pushes and pivots of both sides are printed, not asserted: the reference scales the model and ends its IPM elsewhere.
    (Measured: this LP is nondegenerate -- updates_crossover 0 there, 0 pushes here, vertex objective 2.015942334637e+02 on both
    sides.)"""
    if not os.path.exists(REF_BIN):
        pytest.skip("oracle/_ref/test_lp_{ref,hip} not built (needs the reference sources at build time)")
    m, n = 300, 700
    P = general_lp(m, n, 1)
    b, c, lb, ub = P["b"], P["c"], P["lb"], P["ub"]
    ref = run_reference(P, tmp_path, "crossover 1\n")
    ctx = kkt.KktContext(P["A"])
    s = ctx.ipm_solve(b, c, lb, ub, crossover_start=1e-8)
    assert s["status_ipm"] == 1, s
    g = ctx.crossover_run(b, c, lb, ub, s["basis"])
    ctx.close()
    print("reference: status_crossover %d, updates_crossover %d, time_crossover %s, objval %.12e, infeasibilities %.2e %.2e"
          % (ref["status_crossover"], ref["updates_crossover"], ref.get("time_crossover"), ref["objval"], ref["primal_infeas"], ref["dual_infeas"]))
    print("device: status_crossover %d, %d dual pushes (%d pivots), %d primal pushes (%d pivots), %.3f + %.3f s, infeasibilities %.2e %.2e"
          % (g["status_crossover"], g["dual_pushes"], g["dual_pivots"], g["primal_pushes"], g["primal_pivots"], g["seconds_dual"],
             g["seconds_primal"], g["primal_infeas"], g["dual_infeas"]))
    assert ref["status_crossover"] == 1 and g["status_crossover"] == 1
    objective = float(c @ g["x"])
    print("vertex objective: device %.12e" % objective)
    assert abs(objective - ref["objval"]) <= 1e-8 * (1.0 + abs(ref["objval"]))
    assert g["primal_infeas"] <= 1e-7 and g["dual_infeas"] <= 1e-7
    basis = g["basis"]
    assert len(basis) == m and len(set(basis.tolist())) == m
    assert (g["basic_statuses"] == 0).sum() == m
    # the exact invariants of a vertex: x_N at a bound (0 for a free variable), z_B = 0
    nonbasic = np.setdiff1d(np.arange(n + m), basis)
    free = np.isinf(lb) & np.isinf(ub)
    x, z = g["x"], g["z"]
    assert (z[basis] == 0).all()
    assert ((x[nonbasic] == lb[nonbasic]) | (x[nonbasic] == ub[nonbasic]) | (free[nonbasic] & (x[nonbasic] == 0))).all()
