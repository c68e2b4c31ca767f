"""CPU: the exact-tie generators of tests/basis_ties_reference.py -- their integer-arithmetic exactness assertions, the
planted starting-basis log against the dense restatement of tests/test_gpu_starting_basis.py, and the CPU oracle's Maxvolume
log: every planted class was met and went to its lowest member, at least one class per placement was decided.  The device
is held to the same expectations in tests/test_gpu_basis_ties.py."""
import numpy as np
import pytest

import basis_ties_reference as R


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


def test_placements_are_where_they_claim():
    P = R.placements(64, R.K_BLOCK, R.G, R.G + 257)
    thread = lambda q: (q % R.G) // R.K_BLOCK * R.K_BLOCK + q % R.K_BLOCK          # workgroup * 256 + thread of index q
    wg, wave, npass = (lambda q: (q % R.G) // R.K_BLOCK), (lambda q: (q % R.K_BLOCK) // 64), (lambda q: q // R.G)
    a = P["lanes"]
    assert len({(npass(q), wg(q), wave(q)) for q in a}) == 1
    a = P["waves"]
    assert len({(npass(q), wg(q)) for q in a}) == 1 and wave(a[0]) != wave(a[1])
    a = P["blocks"]
    assert npass(a[0]) == npass(a[1]) and wg(a[0]) != wg(a[1])
    lo, hi = P["later_pass"]
    assert (lo, hi) == (76807, 131077) and npass(lo) == 0 and npass(hi) == 1 and wg(hi) < wg(lo)
    lo, hi = P["same_thread"]
    assert thread(lo) == thread(hi) and npass(lo) + 1 == npass(hi)
    # sb_row_kernel: 8 columns per wavefront, 32 per workgroup, G_ROW per pass
    Q = R.placements(R.K_ROW_LANES, R.ROW_COLS, R.G_ROW, R.G, b=25)
    assert len({q // 8 for q in Q["lanes"]}) == 1
    assert len({q // 32 for q in Q["waves"]}) == 1 and len({q // 8 for q in Q["waves"]}) == 2
    lo, hi = Q["later_pass"]
    assert lo // R.G_ROW == 0 and hi // R.G_ROW == 1 and (hi % R.G_ROW) // 32 < lo // 32
    lo, hi = Q["same_thread"]
    assert hi - lo == R.G_ROW
    # one pass only: the multi-pass placements are left out, never emptied silently
    assert set(R.placements(64, R.K_BLOCK, R.G, 700)) == {"lanes", "waves", "blocks", "strict"}


@pytest.mark.parametrize("shape", [R.SMALL, R.TALL, R.WIDE])
def test_starting_basis_generator_is_exact_and_complete(shape):
    m, n = shape
    P = R.starting_basis_case(m, n, seed=1)                       # (asserts exactness in integers and the disjoint structure)
    E = P["expected"]
    assert len(E["log"]) == len(P["col_classes"]) + len(P["row_classes"])
    kinds_c = {c["kind"] for c in P["col_classes"]}
    kinds_s = {c["kind"] for c in P["row_classes"] if c["unit"] == "scaled"}
    kinds_r = {c["kind"] for c in P["row_classes"] if c["unit"] == "row"}
    one_pass = {"lanes", "waves", "blocks", "strict"}
    every = one_pass | set(R.MULTI_PASS)
    if shape == R.SMALL:
        assert kinds_c == kinds_s == kinds_r == one_pass
    elif shape == R.TALL:
        assert kinds_c == every and kinds_s == kinds_r == one_pass
    else:
        assert kinds_s == kinds_r == every and n >= 2 * R.G_ROW + 300
        far = [c for c in P["row_classes"] if c["kind"] == "threshold"][0]["cols"][2]
        assert far // R.G_ROW == 2                               # the row maximum of `threshold` in the third pass of sb_row_kernel
    assert {c["kind"] for c in P["row_classes"] if c["unit"] == "special"} == {"rw", "threshold", "fixed_decoy"}
    # a "lowest index always" shortcut and a "largest |r|" shortcut both miss some class
    assert any(c["winner"] != min(c["cols"]) for c in P["row_classes"]) and any(c["winner"] != min(c["rows"]) for c in P["col_classes"])
    st = E["status"]
    assert (st[[c["col"] for c in P["col_classes"]]] == R.BASIC_FREE).all()
    assert (st[[n + c["row"] for c in P["row_classes"]]] == R.NONBASIC_FIXED).all()
    assert sorted(E["basis"]) == sorted(np.nonzero(st >= 0)[0])


def test_planted_log_equals_the_dense_restatement():
    """the planted expectation against the two loops with dense LAPACK solves (its margin is 0 here by design: every decision
    is an exact tie or a dyadic step, and the restatement's stable sort takes the first of equals)"""
    import scipy.sparse as sp
    from test_gpu_starting_basis import restatement
    m, n = R.SMALL                                                # (dense solves: every one-pass class of rows and of columns)
    P = R.starting_basis_case(m, n, seed=3)
    S = sp.csc_matrix((P["Ax"], P["Ai"], P["Ap"]), shape=(m, n))
    got = restatement(dict(m=m, n=n, lb=P["lb"], ub=P["ub"], b=P["b"], c=P["c"], S=S), P["it"])
    assert [(int(a), int(b)) for a, b in got["log"]] == P["expected"]["log"]
    assert [int(j) for j in got["basis"]] == P["expected"]["basis"].tolist()
    assert got["dep_cols"] == [] and got["dep_rows"] == [] and got["cols_inconsistent"] == 0 and got["rows_inconsistent"] == 0
    assert got["margin"] == 0.0


def oracle_runs(oracle, po, P):
    Ao = po.Csc(P["m"], P["n"], P["Ap"], P["Ai"], P["Ax"])
    out = {}
    for variant in ("heuristic", "sequential"):
        B = oracle.basis(Ao, P["basis"], P["status"])
        if variant == "heuristic":
            r = B.maxvolume(P["colscale"], volume_tol=2.0, maxskip_updates=10, rows_per_slice=P["rows_per_slice"])
        else:
            r = B.maxvolume_sequential(P["colscale"], volume_tol=2.0)
        r["basis"], r["status"], _ = B.get()
        out[variant] = r
    return out


@pytest.mark.parametrize("shape", [R.SMALL, R.TALL, R.WIDE])
def test_oracle_meets_every_planted_maxvolume_class(oracle, po, shape):
    m, n = shape
    P = R.maxvolume_case(m, n, seed=2, rows_per_slice=R.ROWS_PER_SLICE[shape])
    variants = ("heuristic",) if shape == R.WIDE else ("heuristic", "sequential")    # (sequential: a solve per column)
    runs = oracle_runs(oracle, po, P) if len(variants) == 2 else None
    if runs is None:
        B = oracle.basis(po.Csc(m, n, P["Ap"], P["Ai"], P["Ax"]), P["basis"], P["status"])
        runs = {"heuristic": B.maxvolume(P["colscale"], volume_tol=2.0, maxskip_updates=10, rows_per_slice=P["rows_per_slice"])}
    one_pass = {"lanes", "waves", "blocks", "strict"}
    every = one_pass | set(R.MULTI_PASS)
    for variant in variants:
        r = runs[variant]
        assert r["errflag"] == 0 and r["refused"] == 0 and 0 < r["updates"] <= 40, (variant, r["updates"])
        met = R.maxvolume_classes_met(P, r["exchanges"], variant)                     # (asserts: zero classes unmet)
        print(variant, shape, "updates", r["updates"], "skipped", r["skipped"], "volinc", r["volinc"])
        assert met["ftran"] == {R.SMALL: one_pass, R.TALL: every, R.WIDE: {"lanes", "strict"}}[shape]
        if variant == "heuristic":
            assert met["argmax"] == ({"dup"} | (every if shape == R.WIDE else one_pass))
        assert r["volinc"] == float(int(r["volinc"]))             # a sum of log2 of powers of two
