"""CPU: the references of tests/epilogue_reference.py against themselves and against the oracle, on the models that
tests/test_gpu_epilogue_layouts.py runs on the device.

1. The sequential double value lies within the gate of the long-double value: the reference alone satisfies the gate.
2. So do the sums taken in reversed and in pairwise order: the gate holds whatever the association.
3. Where the oracle has the operation, the sequential double value equals the oracle's bit for bit, which ties the new
   reference to what test_oracle_vs_ref.py ties to the reference project.
"""
import numpy as np
import pytest

import epilogue_reference as er

LD = np.longdouble


def within_gate(op, what):
    for name, v in (("sequential", op.seq), ("reversed", op.alt["reversed"]), ("pairwise", op.alt["pairwise"])):
        err = np.abs(np.asarray(v, np.float64).astype(LD) - op.ld)
        assert np.isfinite(v).all() and (err <= op.gate).all(), (what, name, float((err / np.maximum(op.gate, LD(1e-300))).max()))


def ocsc(A):
    from oracle import pyoracle as po
    return po.Csc(A.nrow, A.ncol, A.p, A.i, A.x)


@pytest.fixture(scope="module", params=er.MODELS)
def M(request):
    return er.any_model(request.param)


def test_models_have_what_the_device_tests_need():
    L = er.model("long")
    Gc, Gr = er.acols(L["A"]), er.arows(L["A"])
    assert list(np.flatnonzero(Gc.long_rows)) == list(er.DENSE_COLS) and list(np.flatnonzero(Gr.long_rows)) == [er.LONG_ROW]
    assert Gr.len[er.EMPTY_ROW] == 0 and Gc.len[er.EMPTY_COL] == 0
    assert (L["state"][:2] == er.FIXED).all() and L["state"][2] != er.FIXED
    for name in ("mixed", "square", "wide", "banded"):
        P = er.any_model(name)
        assert not er.acols(P["A"]).long_rows.any() and not er.arows(P["A"]).long_rows.any()
    # rows are stored with ascending indices in both gather matrices (what `acc` and `accfused` need)
    for G in (Gc, Gr):
        inner = np.ones(G.idx.size, bool)
        inner[G.ptr[:-1][G.len > 0]] = False
        assert (np.diff(G.idx, prepend=-1)[inner] > 0).all()


def test_residuals(M, oracle):
    A, it, st = M["A"], M["it"], M["state"]
    rb = er.iter_rb(A, M["b"], it["x"])
    rc = er.iter_rc(A, M["c"], it["zl"], it["zu"], it["y"], st, False)
    post = er.iter_rc(A, M["c"], it["zl"], it["zu"], it["y"], st, True)
    for name, op in (("rb", rb), ("rc", rc), ("rc postprocessed", post)):
        within_gate(op, name)
    n = M["n"]
    fixed = st[:n] == er.FIXED
    assert not rc.seq[fixed].any() and not rc.ld[fixed].any() and not rc.gate[fixed].any()
    assert post.seq[fixed].any() and (post.gate > 0).all()
    want = oracle.iterate_residuals(ocsc(A), st, M["b"], M["c"], M["lb"], M["ub"], it)
    assert np.array_equal(rb.seq, want["rb"]) and np.array_equal(rc.seq, want["rc"][:n])


def test_fixed_objective(M, oracle):
    A, st = M["A"], M["state"]
    b0, lb0, ub0, it0 = er.objective_inputs(M)
    d = er.obj_fixed(A, it0["y"], it0["x"], st)
    assert d.gate > 0 and abs(LD(d.seq) - d.ld) <= d.gate
    _, dobj, _ = oracle.iterate_objectives(ocsc(A), st, b0, M["c"], lb0, ub0, it0)
    assert dobj == -d.seq


def test_diagonal(M, oracle):
    A = M["A"]
    W = 10.0 ** np.random.default_rng(3).uniform(-2, 2, M["n"] + M["m"])
    op = er.diagonal(A, W)
    within_gate(op, "diagonal")
    P, err = oracle.diag_factorize(ocsc(A), W, M["m"] + 1, precond_dense_cols=False)
    assert err == 0 and np.array_equal(op.seq, P.get()[0])


def test_diag_solve_recovery_and_newton_shift(M, oracle):
    A, it, st, n = M["A"], M["it"], M["state"], M["n"]
    k = oracle.kkt_diag(ocsc(A), maxiter=2000)
    nw = er.newton_inputs(st, it, 5)
    xl, xu, zl, zu = er.barrier_weights(it, st)
    assert k.factorize(xl, xu, zl, zu, nw["mu"]) == 0
    W = k.get()[0]
    rng = np.random.default_rng(6)
    a, b = rng.uniform(-0.5, 0.5, n + M["m"]), rng.uniform(-0.5, 0.5, M["m"])
    x, y, _, err, _ = k.solve(a, b, 1e-6)
    assert err == 0
    rx, rs = er.recover_x(A, W, a, y), er.residual_rows(A, b, x[:n])
    within_gate(rx, "recover x")
    within_gate(rs, "slack part of x")
    assert np.array_equal(rx.seq, x[:n]) and np.array_equal(rs.seq, x[n:])
    step = k.newton_solve(nw["rb"], nw["rc"], nw["rl"], nw["ru"], nw["sl"], nw["su"], it["xl"], it["xu"], it["zl"], it["zu"],
                          st, 1e-6)
    assert step["errflag"] == 0
    lower, upper, lo, up = er.newton_shift(A, nw["rc"], step["dzl"], step["dzu"], it["xl"], it["xu"], it["zl"], it["zu"], st,
                                           step["dy"])
    assert lower.any() and upper.any()
    within_gate(lo, "dzl")
    within_gate(up, "dzu")
    assert np.array_equal(lo.seq[lower], step["dzl"][:n][lower]) and np.array_equal(up.seq[upper], step["dzu"][:n][upper])


def test_basis_columns(M):
    rng = np.random.default_rng(8)
    n, m = M["n"], M["m"]
    scale2 = np.where(rng.random(n) < 0.6, (0.3 * 10.0 ** -rng.random(n)) ** 2, 0.0)
    op = er.basis_columns(M["A"], scale2, rng.uniform(-0.5, 0.5, n + m), rng.uniform(-1, 1, m))
    within_gate(op, "basis columns")
    assert not op.seq[scale2 == 0].any() and not op.gate[scale2 == 0].any()


def test_the_gate_is_not_slack_by_orders_of_magnitude(M):
    """a wrong sign or a dropped init is far outside: the largest |init| is many gates wide"""
    op = er.iter_rb(M["A"], M["b"], M["it"]["x"])
    assert (np.abs(M["b"]) > 1e6 * op.gate.astype(np.float64)).any()
