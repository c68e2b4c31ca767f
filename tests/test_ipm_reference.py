"""CPU: the restatements of tests/ipm_reference.py against the oracle, which tests/test_oracle_vs_ref.py pins bit for bit
to the reference's ipx::Iterate -- so that tests/test_gpu_ipm_vectors.py may hold the device to either.

1. Elementwise work and max/min are equal bit for bit; the oracle's sequential double sums lie within sum_bound (one
   thread, one block: `count` additions) of the long-double sums.
2. `sequential` equals the oracle's StepToBoundary bit for bit at every length and on every input the device test uses;
   on all of them but the near-tie families `parallel_min` -- the device's rule -- returns the same alpha and index.
3. On the near-tie families the two rules differ: by how much is measured here, CPU against CPU, and held.
"""
import numpy as np
import pytest

import ipm_reference as ir
from ipx_amd import synth

LD = np.longdouble
M, N_ = 120, 300


def ocsc(A):
    from oracle import pyoracle as po
    return po.Csc(A.nrow, A.ncol, A.p, A.i, A.x)


@pytest.fixture(scope="module")
def P():
    """synthetic_iterate at (120, 300) with fixed structural and slack variables, as test_iterate_objectives_vs_oracle"""
    P = synth.synthetic_iterate(M, N_, 77)
    rng = np.random.default_rng(5)
    fx = np.concatenate([rng.choice(N_, 20, replace=False), N_ + rng.choice(M, 9, replace=False)])
    P["state"][fx] = ir.FIXED
    for k in ("xl", "xu"):
        P["it"][k][fx] = np.inf
    for k in ("zl", "zu"):
        P["it"][k][fx] = 0.0
    P["b"], P["c"] = P["rhs"], np.concatenate([P["obj"], np.zeros(M)])
    return P


def test_update(P, oracle):
    st, state, it = P["step"], P["state"], P["it"]
    for sp_, sd_, skip in ir.UPDATES:
        a = {k: (None if k in skip else st[k]) for k in ("dx", "dxl", "dxu", "dy", "dzl", "dzu")}
        want = oracle.iterate_update(M, N_, state, it, sp_, a["dx"], a["dxl"], a["dxu"], sd_, a["dy"], a["dzl"], a["dzu"])
        got = ir.update(M, N_, state, it, sp_, a["dx"], a["dxl"], a["dxu"], sd_, a["dy"], a["dzl"], a["dzu"])
        for key in ir.IT_KEYS:
            assert np.array_equal(want[key], got[key]), (key, sp_)
        assert np.array_equal(got["x"][state == ir.FIXED], it["x"][state == ir.FIXED])
        if sp_ == 3.0:                                               # the long step runs into the clamp
            assert all((got[key] == ir.BARRIER_MIN).any() for key in ("xl", "xu", "zl", "zu"))


def test_residuals(P, oracle):
    want = oracle.iterate_residuals(ocsc(P["A"]), P["state"], P["b"], P["c"], P["lbs"], P["ubs"], P["it"])
    got = ir.residuals(P["A"], P["state"], P["b"], P["c"], P["lbs"], P["ubs"], P["it"])
    for key in ("rb", "rc", "rl", "ru"):
        assert np.array_equal(want[key], got[key]), key
    assert (want["presidual"], want["dresidual"]) == (got["presidual"], got["dresidual"])
    assert not got["rc"][P["state"] == ir.FIXED].any() and got["rc"][N_:].any()


def test_complementarity(P, oracle):
    want = oracle.iterate_complementarity(P["state"], P["it"])
    got = ir.complementarity(P["state"], P["it"])
    assert (want["mu_min"], want["mu_max"]) == (got["mu_min"], got["mu_max"])
    bound = ir.sum_bound(got["products"], got["count"], 1)
    assert 0 < bound < 1e-12 * got["sum"]
    assert abs(LD(want["complementarity"]) - got["sum"]) <= bound
    assert abs(LD(want["mu"]) - got["mu"]) <= bound / got["count"] + LD(ir.U) * got["mu"]      # one more rounding: the division
    assert got["count"] == int(ir.has_lb(P["state"]).sum() + ir.has_ub(P["state"]).sum())
    # no barrier term: mu = 0 and min = 0
    state = np.where(np.arange(M + N_) % 2 == 0, ir.FIXED, ir.FREE).astype(np.uint8)
    none = ir.complementarity(state, P["it"])
    want = oracle.iterate_complementarity(state, P["it"])
    assert (none["count"], float(none["sum"]), float(none["mu"]), none["mu_min"], none["mu_max"]) == (0, 0.0, 0.0, 0.0, 0.0)
    assert (want["complementarity"], want["mu"], want["mu_min"], want["mu_max"]) == (0.0, 0.0, 0.0, 0.0)


def test_objectives(P, oracle):
    pobj, dobj, offset = oracle.iterate_objectives(ocsc(P["A"]), P["state"], P["b"], P["c"], P["lbs"], P["ubs"], P["it"])
    got = ir.objectives(P["A"], P["state"], P["b"], P["c"], P["lbs"], P["ubs"], P["it"])
    assert offset != 0.0 and got["fixed_terms"].size == 20 and got["fixed_terms"].all()
    assert abs(LD(pobj) - got["pobj"]) <= ir.sum_bound(got["pterms"], got["pterms"].size, 1)
    assert abs(LD(offset) - got["offset"]) <= ir.sum_bound(got["oterms"], got["oterms"].size, 1)
    # the oracle adds every fixed column's products (8 each), multiplies by x_j (one rounding) and subtracts
    bound = ir.sum_bound(np.concatenate([got["dterms"], got["fixed_products"]]), got["dterms"].size + 20 + 8 + 1, 1)
    assert abs(LD(dobj) - got["dobj"]) <= bound and bound < 1e-12 * (1 + abs(dobj))
    # the double terms of the fixed structural variables are the long-double products' sums, rounded
    assert abs(ir.ldsum(got["fixed_terms"]) - ir.ldsum(got["fixed_products"])) <= ir.sum_bound(got["fixed_products"], 9, 1)


def test_newton_recovery(P, oracle):
    """the oracle's whole IPM::SolveNewtonSystem; from its dx, dy the restatement must give its other four vectors"""
    A, state, it = P["A"], P["state"], P["it"]
    r = ir.residuals(A, state, P["b"], P["c"], P["lbs"], P["ubs"], it)
    comp = ir.complementarity(state, it)
    mu = float(comp["mu"])
    lbm, ubm = ir.has_lb(state), ir.has_ub(state)
    sl = np.where(lbm, mu - synth.xl_safe(it["xl"]) * it["zl"], 0.0)
    su = np.where(ubm, mu - synth.xl_safe(it["xu"]) * it["zu"], 0.0)
    k = oracle.kkt_diag(ocsc(A), maxiter=2000)
    assert k.factorize(it["xl"], it["xu"], it["zl"], it["zu"], mu) == 0
    for res in ((r["rb"], r["rc"], r["rl"], r["ru"]), (None, None, None, None)):
        o = k.newton_solve(*res, sl, su, it["xl"], it["xu"], it["zl"], it["zu"], state, 1e-8)
        assert o["errflag"] == 0
        got = ir.newton_recover(A, state, res[1], res[2], res[3], sl, su, it["xl"], it["xu"], it["zl"], it["zu"], o["dx"], o["dy"])
        for key in ("dxl", "dxu", "dzl", "dzu"):
            assert np.array_equal(got[key], o[key]), key
        boxed = state == ir.BOXED
        assert got["lower"][boxed].any() and got["upper"][boxed].any() and not (got["lower"] & got["upper"]).any()
        assert np.array_equal(got["lower"] | got["upper"], state >= ir.LB)


@pytest.mark.parametrize("length", ir.STEP_LENGTHS)
def test_step_rules_agree_where_the_device_test_uses_either(oracle, length):
    for name, x, dx, alpha0 in ir.step_cases(length):
        s = ir.sequential(x, dx, alpha0)
        assert s == oracle.step_to_boundary(x, dx, alpha0), (name, length)
        assert s == ir.parallel_min(x, dx, alpha0), (name, length)
        if name == "nothing blocks":
            assert s == (1.0, -1)
        elif name == "only the last index blocks":
            assert s == (0.5 * ir.DAMP, length - 1)
        elif name == "only index G blocks":
            assert s == (0.5 * ir.DAMP, ir.G)
        elif name.startswith("alpha0 = 0.5"):
            assert s == (0.5, -1) and (length < 63 or (x + dx < 0).any())
        elif name.startswith("x = 0"):
            assert s == (0.0, length // 3)
        elif length >= 63:
            assert 0.0 < s[0] < 1.0 and s[1] >= 0


def test_exact_ties(oracle):
    for name, x, dx, want in ir.exact_ties():
        s = ir.sequential(x, dx)
        assert s == oracle.step_to_boundary(x, dx) == ir.parallel_min(x, dx), name
        assert s == ((0.75 * ir.DAMP) / 1.5, want), name
        assert ((-(x * ir.DAMP) / dx) == s[0]).sum() == 2 and (x + dx < 0).sum() > 1000, name


def window(seeds, length=5000, oracle=None):
    worst, differ = 0.0, 0
    for seed in seeds:
        x, dx, alpha0 = ir.near_tie_family(length, seed)
        a1, i1 = ir.sequential(x, dx, alpha0)
        a2, i2 = ir.parallel_min(x, dx, alpha0)
        if oracle is not None and seed % 20 == 0:
            assert (a1, i1) == oracle.step_to_boundary(x, dx, alpha0), seed
        assert a2 <= a1                                              # the parallel minimum is never the longer step
        worst = max(worst, (a1 - a2) / a2 / ir.EPS)
        differ += i1 != i2
    return worst, differ / len(seeds)


def test_the_window_between_the_two_step_rules(oracle):
    """The documented exception: on scaled copies of one (x, dx) pair the sequential scan
    and the parallel minimum pick different blocking indices in most trials, and alpha differs by up to 1.95 eps.
    Measured over ir.WINDOW_SEEDS: 1.9474 eps, index differs in 69.85 % of the trials; on random data: never."""
    worst, share = window(ir.WINDOW_SEEDS, oracle=oracle)
    print("window: %.4f eps, blocking index differs in %.2f %% of %d trials" % (worst, 100 * share, len(ir.WINDOW_SEEDS)))
    assert 1.0 < worst <= ir.MEASURED_WINDOW_EPS and abs(share - ir.MEASURED_INDEX_SHARE) < 0.005
    other, share2 = window(range(10000, 11000))
    print("other seeds: %.4f eps, %.2f %%" % (other, 100 * share2))
    assert other <= 2.0 * ir.MEASURED_WINDOW_EPS and share2 > 0.5
    for seed in range(300):
        x, dx = ir.random_step(5000, seed)
        assert ir.sequential(x, dx) == ir.parallel_min(x, dx)
    # the lengths of the device test: the oracle's scan there, too
    for length, seed in ir.NEAR_TIE_DEVICE_CASES:
        x, dx, alpha0 = ir.near_tie_family(length, seed)
        assert ir.sequential(x, dx, alpha0) == oracle.step_to_boundary(x, dx, alpha0)
        a1, a2 = ir.sequential(x, dx, alpha0)[0], ir.parallel_min(x, dx, alpha0)[0]
        assert 0 <= (a1 - a2) / a2 / ir.EPS <= 2.0 * ir.MEASURED_WINDOW_EPS


@pytest.mark.parametrize("name", list(ir.SHAPES))
def test_shapes_have_what_the_device_tests_need(name):
    P = ir.shape_model(name)
    n, m, N, state, G = P["n"], P["m"], P["N"], P["state"], ir.G
    assert N > G and ir.vec_grid(N) == ir.GRID_CAP and (name == "wide") == (N == G + 257) and (name == "tall") == (m == G + 257)
    by_row, by_col = ir.row_lengths(P["A"])
    assert by_row.max() <= ir.MAX_ROW_LEN and by_col.max() <= ir.MAX_ROW_LEN
    for st_ in range(5):                                             # every state in both passes
        assert (state[:G] == st_).any() and (state[G:] == st_).any(), st_
    fx = state == ir.FIXED
    assert 0.005 < fx.mean() < 0.02 and fx[:n].any() and fx[n:].any()
    assert (state[list(P["edges"])] == ir.BOXED).all() and (state[P["boxed"]] == ir.BOXED).all()
    it = P["it"]
    assert np.isinf(it["xl"][fx]).all() and not it["zl"][fx].any() and np.isinf(it["xu"][fx]).all() and not it["zu"][fx].any()
    lbm, ubm = ir.has_lb(state), ir.has_ub(state)
    assert np.isfinite(it["xl"][lbm]).all() and np.isfinite(P["lbs"][lbm]).all() and np.isfinite(P["ubs"][ubm]).all()
    # the large update clamps entries of the second pass
    st = P["step"]
    up = ir.update(m, n, state, it, 3.0, st["dx"], st["dxl"], st["dxu"], 5.0, st["dy"], st["dzl"], st["dzu"])
    for key in ("xl", "xu", "zl", "zu"):
        assert (up[key][G:] == ir.BARRIER_MIN).any(), key
