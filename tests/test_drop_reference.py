"""CPU: the inputs of tests/test_gpu_drop.py, not the product.  The planted states must be decided with a margin (so that the
device's rounding cannot change a decision), must meet all four outcomes of DropPrimal / DropDual, and the gate case must do
nothing; the dyadic cases must be exact and carry their own expectations; and ipxk_drop_info mirrors the header."""
import ctypes
import os
import re

import numpy as np
import pytest

import drop_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ipx_kkt_hip.h")
PLANTED = [(60, 150, 1), (300, 700, 2)]          # (m, n, seed): the cases of test_gpu_drop.py
DROP_TOL = 1e-9


@pytest.mark.parametrize("m,n,seed", PLANTED)
def test_planted_states_are_decided_with_margins(m, n, seed):
    P = dr.planted_state(m, n, seed)
    R = dr.restatement(P, DROP_TOL, DROP_TOL)
    assert R["margin"].value >= 1e-6, R["margin"].value
    log = R["log"]
    actions = {a for _, a, _ in log}
    assert actions == {dr.EXCHANGED, dr.IMPLIED_LB, dr.IMPLIED_UB, dr.FIXED}, actions
    # an exchange in each procedure (DropPrimal's candidates are basic at the start, DropDual's nonbasic); the restatement
    # asserts that every exchange it follows is accepted at once
    assert any(a == dr.EXCHANGED and P["status"][j] == dr.BASIC for j, a, _ in log)
    assert any(a == dr.EXCHANGED and P["status"][j] == dr.NONBASIC for j, a, _ in log)
    # the iterate changes: implied variables keep zl, zu; fixed ones lose everything but x
    it0, it1 = P["it"], R["it"]
    for j, a, _ in log:
        if a in (dr.IMPLIED_LB, dr.IMPLIED_UB):
            assert np.isinf(it1["xl"][j]) and np.isinf(it1["xu"][j]) and it1["zl"][j] == it0["zl"][j] and it1["zu"][j] == it0["zu"][j]
            assert R["status"][j] == dr.BASIC_FREE and np.isinf(R["colscale"][j])
        if a == dr.FIXED:
            assert it1["xl"][j] == it1["xu"][j] == it1["zl"][j] == it1["zu"][j] == 0.0 and it1["x"][j] == it0["x"][j]
            assert R["status"][j] == dr.NONBASIC_FIXED and R["colscale"][j] == 0.0
    assert sorted(R["basis"].tolist()) == sorted(np.nonzero(R["status"] >= 0)[0].tolist())


@pytest.mark.parametrize("m,n,seed", PLANTED)
def test_gate_case_does_nothing(m, n, seed):
    P = dr.planted_state(m, n, seed, gate_open=False)
    pobj, dobj = dr.objectives(P, P["it"], P["state"])
    assert pobj < dobj and (dobj - pobj) >= 1e-6 * abs(dobj)
    R = dr.restatement(P, DROP_TOL, DROP_TOL)
    assert R["log"] == [] and np.array_equal(R["state"], P["state"]) and np.array_equal(R["status"], P["status"])


def test_dyadic_row_case():
    P = dr.row_search_case(7)
    m, n = P["m"], P["n"]
    assert n + m > 3 * dr.G_ROW
    kinds = {c["kind"] for c in P["classes"]}
    assert {"lanes", "waves", "blocks", "later_pass", "same_thread", "strict", "third_pass", "pivot_zero", "volume_two",
            "fixed_decoy"} <= kinds
    d = dr.scaling_factors(P["it"], P["state"])
    for c in P["classes"]:
        for j, w in zip(c["cols"], c["wexp"]):
            if np.isinf(P["ub"][j]):                                 # (the fixed decoy has lb = ub = 0)
                assert d[j] == 2.0 ** w
        assert d[n + c["row"]] == 2.0 ** -20
    acts = [a for _, a, _ in P["expected_log"]]
    assert acts.count(dr.IMPLIED_LB) == 1 and acts.count(dr.EXCHANGED) == len(acts) - 1


def test_dyadic_column_case():
    P = dr.column_search_case(8)
    m, n = P["m"], P["n"]
    assert m > dr.G
    kinds = {c["kind"] for c in P["classes"]}
    assert {"lanes", "waves", "blocks", "later_pass", "same_thread", "strict", "free_decoy", "volume_two"} <= kinds
    d = dr.scaling_factors(P["it"], P["state"])
    for c in P["classes"]:
        assert d[c["col"]] == 2.0 ** 16
        for p, e in zip(c["rows"], c["invexp"]):
            if P["state"][n + p] != dr.ST_FREE:
                assert 1.0 / d[n + p] == 2.0 ** e
    acts = [a for _, a, _ in P["expected_log"]]
    assert acts.count(dr.FIXED) == 1 and acts.count(dr.EXCHANGED) == len(acts) - 1


def test_drop_info_mirror():
    """every member of ipxk_drop_info is 8 bytes, in the header's order"""
    from ipx_amd import kkt
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+ipxk_drop_info\s*\{(.*?)\}\s*ipxk_drop_info\s*;", text, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            assert ctype in ("ipxint", "double")
            fields += [(nm.strip(), ctype) for nm in names.split(",")]
    assert [f for f, _ in fields] == ["errflag", "primal_candidates", "dual_candidates", "primal_dropped", "dual_dropped", "updates",
                                      "refused", "factorizations", "seconds"]
    assert [f for f, _ in fields] == [f for f, _ in kkt.DropInfo._fields_]
    assert ctypes.sizeof(kkt.DropInfo) == 8 * len(fields)
    for k, (fname, ctype) in enumerate(fields):
        assert getattr(kkt.DropInfo, fname).offset == 8 * k
        assert kkt.DropInfo._fields_[k][1] is (ctypes.c_int64 if ctype == "ipxint" else ctypes.c_double)


@pytest.mark.parametrize("example", ["ipm_loop.cc", "lp_user.cc"])
def test_examples_compile_against_the_header(example):
    import shutil
    import subprocess
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed"
    subprocess.check_call([cxx, "-std=c++14", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", example)])


def test_state_codes():
    from ipx_amd import kkt
    text = open(HEADER).read()
    for name, value in (("FIXED", 0), ("FREE", 1), ("BARRIER_LB", 2), ("BARRIER_UB", 3), ("BARRIER_BOXED", 4), ("IMPLIED_LB", 5),
                        ("IMPLIED_UB", 6)):
        assert re.search(r"#define IPXK_STATE_%s %d\b" % (name, value), text), name
        assert getattr(kkt, "STATE_" + name) == value
