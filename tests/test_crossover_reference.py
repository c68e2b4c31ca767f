"""CPU: the inputs of tests/test_gpu_crossover.py, not the product.  On the planted points the sequential and the order-free
form of both ratio tests pick the same index and the same step bits on every push (asserted inside the restatement), every
decision is taken with a relative margin, all outcomes of a push occur and the final invariants hold; the dyadic cases are exact
and carry their own expectations; ipxk_crossover_info mirrors the header and the examples compile against it."""
import ctypes
import os
import re

import numpy as np
import pytest

import crossover_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ipx_kkt_hip.h")
PLANTED = [(60, 150, 1), (300, 700, 2)]          # (m, n, seed): the cases of test_gpu_crossover.py
MARGIN = 1e-6                                    # the margin the drop tests use


def fixed_at_bound_of(P):
    return (P["z"] != 0).astype(np.uint8)


def primal_alone(P, out=None, L=np.float64, stop_at=None):
    """PushPrimal alone on the planted point with fixed_at_bound = (z != 0): the candidates in descending index order"""
    AI = cr.dense_AI(P).astype(L)
    lb, ub, x = (P[k].astype(L) for k in ("lb", "ub", "x"))
    B = cr.DenseBasis(AI, P["basis"])
    _, primal = cr.superbasics(B, lb, ub, x, P["z"], np.arange(P["n"] + P["m"]))
    r = cr.push_primal(B, lb, ub, x, primal, fixed_at_bound=fixed_at_bound_of(P), out=out, stop_at=stop_at)
    r.update(x=x, basis=B.basis.copy(), variables=primal)
    return r


def dual_alone(P, out=None, L=np.float64, stop_at=None):
    """PushDual alone: the candidates in ascending index order"""
    AI = cr.dense_AI(P).astype(L)
    lb, ub, x, y, z = (P[k].astype(L) for k in ("lb", "ub", "x", "y", "z"))
    B = cr.DenseBasis(AI, P["basis"])
    dual, _ = cr.superbasics(B, lb, ub, x, z, np.arange(P["n"] + P["m"]))
    r = cr.push_dual(B, lb, ub, x, y, z, dual, out=out, stop_at=stop_at)
    r.update(y=y, z=z, basis=B.basis.copy(), variables=dual)
    return r


def assert_vertex_invariants(P, R):
    """z = 0 on the basic variables, every nonbasic x at a bound (0 for a free one), lb <= x <= ub"""
    lb, ub, x, z, basis = P["lb"], P["ub"], R["x"], R["z"], R["basis"]
    N = P["n"] + P["m"]
    nonbasic = np.setdiff1d(np.arange(N), basis)
    assert len(set(basis.tolist())) == P["m"]
    assert (z[basis] == 0).all()
    free = np.isinf(lb) & np.isinf(ub)
    assert ((x[nonbasic] == lb[nonbasic]) | (x[nonbasic] == ub[nonbasic]) | (free[nonbasic] & (x[nonbasic] == 0))).all()


@pytest.fixture(scope="module")
def outcomes():
    out = cr.Outcomes()
    runs = {}
    for m, n, seed in PLANTED:
        P = cr.planted_point(m, n, seed)
        runs[(m, n)] = (P, cr.push_all(P, P["weights"], out=out, basic=False), primal_alone(P, out=out), dual_alone(P, out=out))
    return out, runs


@pytest.mark.parametrize("m,n,seed", PLANTED)
def test_planted_points(outcomes, m, n, seed):
    out, runs = outcomes
    P, R, Rp, Rd = runs[(m, n)]
    lb, ub = P["lb"], P["ub"]
    # the input: a basis with structural columns, a complementary point with superbasics of both kinds
    assert (P["basis"] < n).sum() == m // 3
    assert len(R["dual_superbasics"]) >= 5 and len(R["primal_superbasics"]) >= 5
    assert cr.dual_infeasibility(lb, ub, P["x"], P["z"]) == 0 and cr.primal_infeasibility(lb, ub, P["x"]) == 0
    assert R["dual"]["status"] == 1 and R["primal"]["status"] == 1
    assert R["dual"]["pivots"] >= 1 and R["primal"]["pivots"] >= 1
    # after the pushes (no basic solution yet): the exact invariants
    assert_vertex_invariants(P, R)
    assert cr.dual_infeasibility(lb, ub, R["x"], R["z"]) == 0 and cr.primal_infeasibility(lb, ub, R["x"]) == 0
    # the pushes keep A x = b and A'y + z = c up to rounding
    AI = cr.dense_AI(P)
    assert np.abs(AI @ R["x"] - P["b"]).max() <= 1e-9 * (1 + np.abs(P["b"]).max())
    assert np.abs(AI.T @ R["y"] + R["z"] - P["c"]).max() <= 1e-9 * (1 + np.abs(P["c"]).max())
    # PushPrimal alone with fixed_at_bound: the fixed variables have not moved
    fixed = fixed_at_bound_of(P).astype(bool)
    assert np.array_equal(Rp["x"][fixed], P["x"][fixed])
    assert (Rd["z"][Rd["basis"]] == 0).all()


def test_margins_and_outcomes(outcomes):
    out, _ = outcomes
    print("margins: ratio %.3e, pivot %.3e; outcomes %s" % (out.ratio.value, out.pivot.value, sorted(out.seen)))
    assert out.ratio.value >= MARGIN and out.pivot.value >= MARGIN
    assert {"dual_blocked", "dual_free", "primal_lb", "primal_ub", "primal_free", "boxed_to_bound", "free_to_zero",
            "fixed_step_zero"} <= out.seen


def test_long_double_takes_the_same_decisions(outcomes):
    """the reference of the GPU test: the same logs in long double"""
    _, runs = outcomes
    P, R, _, _ = runs[PLANTED[0][:2]]
    RL = cr.push_all(P, P["weights"], L=np.longdouble, basic=False)
    assert RL["log"] == R["log"] and np.array_equal(RL["basis"], R["basis"])
    assert np.abs(RL["x"] - R["x"]).max() <= 1e-9 and np.abs(RL["z"] - R["z"]).max() <= 1e-9


def test_basic_solution_and_order():
    P = cr.planted_point(*PLANTED[0])
    AI = cr.dense_AI(P)
    B = cr.DenseBasis(AI, P["basis"])
    rng = np.random.default_rng(3)
    x, z = P["x"] + 0.0, P["z"] + 0.0
    x[B.basis] = rng.uniform(-1, 1, P["m"])                          # x_B and z_N are recomputed, y comes out of it
    nonbasic = np.setdiff1d(np.arange(P["n"] + P["m"]), B.basis)
    z[nonbasic] = rng.uniform(-1, 1, len(nonbasic))
    y = np.zeros(P["m"])
    cr.basic_solution(B, P["b"], P["c"], x, y, z)
    assert np.abs(x - P["x"]).max() <= 1e-9 and np.abs(y - P["y"]).max() <= 1e-9 and np.abs(z - P["z"]).max() <= 1e-9
    w = np.array([2.0, 1.0, 2.0, 1.0, np.inf, 0.0])
    assert cr.sortperm(w).tolist() == [5, 1, 3, 0, 2, 4]
    st = cr.basic_statuses(B, P["lb"], P["ub"], P["x"], P["z"])
    assert (st[B.basis] == cr.IPX_BASIC).all() and {cr.IPX_NONBASIC_LB, cr.IPX_NONBASIC_UB, cr.IPX_SUPERBASIC} <= set(st.tolist())


def test_argument_checks():
    P = cr.planted_point(*PLANTED[0])
    AI = cr.dense_AI(P)
    lb, ub = P["lb"], P["ub"]
    B = cr.DenseBasis(AI, P["basis"])
    nonbasic = np.setdiff1d(np.arange(P["n"] + P["m"]), B.basis)
    with pytest.raises(cr.ArgumentError):
        cr.push_dual(B, lb, ub, P["x"], P["y"].copy(), P["z"].copy(), [int(nonbasic[0])])
    with pytest.raises(cr.ArgumentError):
        cr.push_primal(B, lb, ub, P["x"].copy(), [int(B.basis[0])])
    z = P["z"].copy()
    j = int(np.nonzero(z > 0)[0][0])
    z[j] = -z[j]
    with pytest.raises(cr.ArgumentError):
        cr.push_dual(B, lb, ub, P["x"], P["y"].copy(), z, [])
    x = P["x"].copy()
    x[int(np.nonzero(np.isfinite(lb))[0][0])] = -1.0
    with pytest.raises(cr.ArgumentError):
        cr.push_primal(B, lb, ub, x, [])


def test_dyadic_cases_are_exact():
    D = cr.dual_ratio_case(11)
    assert D["n"] + D["m"] > 3 * cr.G_ROW
    kinds = [c["kind"] for c in D["classes"]]
    assert set(cr.TIE_KINDS) | {"strict", "pivot_zero", "within_tol", "basic_decoy"} == set(kinds)
    assert len(D["expected_log"]) == len(kinds) - 1                 # within_tol: the full step, no pivot
    for c in D["classes"]:
        if c["winner"] >= 0:
            assert c["step"] == 2.0 ** -3 - cr.DYADIC_FEASTOL / abs(c["r"][c["cols"].index(c["winner"])])
    Pm = cr.primal_ratio_case(12)
    assert Pm["m"] > cr.G
    kinds = [c["kind"] for c in Pm["classes"]]
    assert set(cr.TIE_KINDS) | {"strict", "pivot_zero", "within_tol"} == set(kinds)
    won = [c["at_lb"] for c in Pm["classes"] if c["winner"] >= 0]
    assert True in won and False in won                             # block_at_lb differs between the classes' winners
    for c in Pm["classes"]:
        if c["kind"] in cr.TIE_KINDS:                               # ... and between the tied members of a class
            assert len({bool(p < 0) for p in c["pivots"]}) == 2


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_crossover_info_mirror():
    """every member of ipxk_crossover_info is 8 bytes, in the header's order"""
    from ipx_amd import kkt
    body = re.search(r"typedef\s+struct\s+ipxk_crossover_info\s*\{(.*?)\}\s*ipxk_crossover_info\s*;", header_text(), flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            assert ctype in ("ipxint", "double")
            fields += [(nm.strip(), ctype) for nm in names.split(",")]
    assert [f for f, _ in fields] == ["errflag", "status_crossover", "dual_superbasics", "primal_superbasics", "dual_pushes", "dual_pivots",
                                      "primal_pushes", "primal_pivots", "refused", "factorizations", "primal_infeas", "dual_infeas",
                                      "seconds_dual", "seconds_primal"]
    assert [f for f, _ in fields] == [f for f, _ in kkt.CrossoverInfo._fields_]
    assert ctypes.sizeof(kkt.CrossoverInfo) == 8 * len(fields)
    for k, (fname, ctype) in enumerate(fields):
        assert getattr(kkt.CrossoverInfo, fname).offset == 8 * k
        assert kkt.CrossoverInfo._fields_[k][1] is (ctypes.c_int64 if ctype == "ipxint" else ctypes.c_double)
    assert [f for f, _ in kkt.CrossoverParams._fields_] == ["primal_feastol", "dual_feastol", "max_etas"]


def test_status_codes_against_the_header():
    """the IPX_* basic statuses as the header states them for ipxk_crossover_run"""
    text = open(HEADER).read()
    for name, value in (("IPX_basic", cr.IPX_BASIC), ("IPX_nonbasic_lb", cr.IPX_NONBASIC_LB), ("IPX_nonbasic_ub", cr.IPX_NONBASIC_UB),
                        ("IPX_superbasic", cr.IPX_SUPERBASIC)):
        found = re.search(r"%s\s+(-?\d+)" % name, text)
        assert found and int(found.group(1)) == value, name
    for fn in ("ipxk_crossover_push_dual", "ipxk_crossover_push_primal", "ipxk_crossover_basic_solution", "ipxk_crossover_run"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, header_text()), fn


@pytest.mark.parametrize("example", ["ipm_loop.cc", "lp_user.cc"])
def test_examples_compile_against_the_header(example):
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    subprocess.check_call([cxx, "-std=c++14", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", example)])
    if example == "ipm_loop.cc":
        assert "ipxk_crossover_run" in open(os.path.join(ROOT, "examples", example)).read()
