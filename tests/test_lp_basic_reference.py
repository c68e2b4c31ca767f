"""CPU: tests/lp_basic_reference.py, the NumPy restatement the GPU tests of the user-form basic solution compare against, held to
something other than itself.

1. Residual identity.  A solver-form point with AI x = b and z = c - AI'y (the slack part of x and all of z computed in
   extended precision and rounded once) must map to a user-form point with rhs - slack - A x = 0 and obj - z - A'y = 0 up to
   rounding: the presolve is sign flips, copies and powers of two, so the only errors are the one rounding of each computed
   entry and that of the boxed variables' subtraction, each at most u = EPS / 2 times a term of the row or column.  The bound
   is k EPS sum|terms| with k = entries + 3; the comparison value is computed in extended precision.
2. The status map against a scalar transcription of the rule, entry by entry, and the correction: every entry it owns is the
   user bound or 0.0 exactly, every other entry is the general point's bit for bit.
3. The asserts of PostsolveBasis raise on planted violations.
"""
import numpy as np
import pytest

import lp_basic_reference as lbr
from test_gpu_user_model import make_lp, np_presolve

EPS = np.finfo(np.float64).eps
L = np.longdouble

CASES = {"primal": lambda: make_lp(130, 300, 11), "dualized": lambda: make_lp(400, 90, 12, eq_every=10, unsorted=True)}
_models = {}


def model(name):
    if name not in _models:
        _models[name] = CASES[name]()
    return _models[name]


def dense(nrow, ncol, Ap, Ai, Ax):
    D = np.zeros((nrow, ncol), L)
    D[Ai, np.repeat(np.arange(ncol), np.diff(Ap))] = Ax
    return D


def consistent_point(S, seed):
    """x, y, z in solver form with AI x = b and z = c - AI'y up to one rounding per computed entry"""
    rng = np.random.default_rng(seed)
    m, n = S["m"], S["n"]
    D = dense(m, n, S["Ap"], S["Ai"], S["Ax"])
    xs, y = rng.normal(size=n), rng.normal(size=m)
    slack = (S["b"].astype(L) - D @ xs.astype(L)).astype(np.float64)
    z = np.concatenate([(S["c"][:n].astype(L) - D.T @ y.astype(L)).astype(np.float64), S["c"][n:] - y])
    return np.concatenate([xs, slack]), y, z


@pytest.mark.parametrize("scale", [1, 0])
@pytest.mark.parametrize("name", ["primal", "dualized"])
def test_general_point_keeps_the_residuals(name, scale):
    M = model(name)
    S = np_presolve(M, scale=scale)
    assert S["dualized"] == (name == "dualized") and (S["rounds"] >= 2) == bool(scale)
    if S["dualized"]:
        assert S["boxed"].size > 2 and S["flipped"].size > 2
    nc, nv, A = M["nc"], M["nv"], M["A"]
    x, y, z = consistent_point(S, 5)
    u = lbr.general_point(M, S, x, y, z)
    D = dense(nc, nv, *np_load_sorted(A))
    rb = (M["rhs"].astype(L) - u["slack"].astype(L)) - D @ u["x"].astype(L)
    rb_mag = np.abs(M["rhs"]) + np.abs(u["slack"]) + np.abs(D) @ np.abs(u["x"]).astype(L)
    krow = np.bincount(A.i[A.x != 0.0], minlength=nc) + 3
    print("largest |rb| / bound: %.3g" % float(np.max(np.abs(rb)[rb_mag > 0] / (krow * EPS * rb_mag)[rb_mag > 0])))
    assert (np.abs(rb) <= krow * EPS * rb_mag).all()
    rc = (M["obj"].astype(L) - u["z"].astype(L)) - D.T @ u["y"].astype(L)
    rc_mag = np.abs(M["obj"]) + np.abs(u["z"]) + np.abs(D.T) @ np.abs(u["y"]).astype(L)
    kcol = np.count_nonzero(D, axis=0) + 3
    print("largest |rc| / bound: %.3g" % float(np.max(np.abs(rc)[rc_mag > 0] / (kcol * EPS * rc_mag)[rc_mag > 0])))
    assert (np.abs(rc) <= kcol * EPS * rc_mag).all()


def np_load_sorted(A):
    from test_gpu_user_model import np_load
    return np_load(A)


def scalar_status_map(M, S, st):
    """PostsolveBasis transcribed entry by entry"""
    nc, nv, n = M["nc"], M["nv"], S["n"]
    cb, vb = [0] * nc, [0] * nv
    if S["dualized"]:
        for i in range(nc):
            cb[i] = -1 if st[i] == 0 else 0
        for j in range(nv):
            vb[j] = (-1 if S["lb"][n + j] != S["ub"][n + j] else -3) if st[n + j] == 0 else 0
        for k, j in enumerate(S["boxed"]):
            if st[nc + k] == 0:
                assert vb[j] == 0
                vb[j] = -2
        for j in S["flipped"]:
            assert vb[j] != -2
            if vb[j] == -1:
                vb[j] = -2
    else:
        for i in range(nc):
            cb[i] = 0 if st[n + i] == 0 else -1
        for j in range(nv):
            vb[j] = int(st[j])
    return np.array(cb, np.int64), np.array(vb, np.int64)


@pytest.mark.parametrize("phase", [0, 1])
@pytest.mark.parametrize("name", ["primal", "dualized"])
def test_status_map_and_correction(name, phase):
    M = model(name)
    S = np_presolve(M)
    n = S["n"]
    st = lbr.planted_statuses(M, S, 7, phase)
    assert set(st[:n]) == {0, -1, -2, -3} and set(st[n:]) == {0, -1, -2}
    cb, vb = lbr.postsolve_basis(M, S, st)
    cb2, vb2 = scalar_status_map(M, S, st)
    assert np.array_equal(cb, cb2) and np.array_equal(vb, vb2)
    assert set(cb) == {0, -1} and set(vb) == {0, -1, -2, -3}
    if S["dualized"]:
        other = lbr.postsolve_basis(M, S, lbr.planted_statuses(M, S, 7, 1 - phase))[1]
        assert ((vb[S["boxed"]] == -2) != (other[S["boxed"]] == -2)).all()           # each boxed variable in both states
        assert ((vb[S["flipped"]] == -2) != (other[S["flipped"]] == -2)).all()       # each flipped variable likewise
    rng = np.random.default_rng(8)
    x, y, z = rng.normal(size=n + S["m"]), rng.normal(size=S["m"]), rng.normal(size=n + S["m"])
    g = lbr.general_point(M, S, x, y, z)
    u = lbr.postsolve_basic(M, S, x, y, z, st)
    for j in range(M["nv"]):
        want_x = M["lb"][j] if vb[j] == -1 else M["ub"][j] if vb[j] == -2 else g["x"][j]
        want_z = 0.0 if vb[j] == 0 else g["z"][j]
        assert u["x"][j].tobytes() == np.float64(want_x).tobytes() and u["z"][j].tobytes() == np.float64(want_z).tobytes(), j
    for i in range(M["nc"]):
        want_s = 0.0 if cb[i] == -1 else g["slack"][i]
        want_y = 0.0 if cb[i] == 0 else g["y"][i]
        assert u["slack"][i].tobytes() == np.float64(want_s).tobytes() and u["y"][i].tobytes() == np.float64(want_y).tobytes(), i


def test_asserts_raise():
    for name in ("primal", "dualized"):
        M = model(name)
        S = np_presolve(M)
        st = lbr.planted_statuses(M, S, 9)
        lbr.check_statuses(S, st)
        bad = st.copy()
        bad[S["n"] + 17] = -3
        with pytest.raises(ValueError, match="slack 17"):
            lbr.postsolve_basis(M, S, bad)
    nb = S["boxed"].size
    nc = S["n"] - nb
    bad = st.copy()
    bad[nc + 3] = 0
    bad[S["n"] + S["boxed"][3]] = 0
    with pytest.raises(ValueError, match="number 3"):
        lbr.postsolve_basis(M, S, bad)


def test_build_statuses_and_evaluation_on_a_tiny_model():
    """worked by hand: 2 variables, rows '<' and '>'"""
    S = dict(lb=np.array([0.0, -np.inf, -np.inf, 0.0]), ub=np.array([np.inf, 1.0, np.inf, 0.0]))
    assert lbr.build_statuses(S, [1, 2]).tolist() == [-1, 0, 0, -1]
    assert lbr.build_statuses(S, [0, 3]).tolist() == [0, -2, -3, 0]
    M = dict(nc=2, ct="<>", lb=np.array([0.0, -np.inf]), ub=np.array([np.inf, 1.0]), obj=np.array([2.0, -3.0]))
    u = dict(x=np.array([-0.25, 1.5]), slack=np.array([-0.125, 0.0625]), y=np.array([0.5, 2.0]), z=np.array([-4.0, 8.0]),
             vbasis=np.array([-1, -2]))
    # primal: lb - x = 0.25, x - ub = 0.5, -slack('<') = 0.125, slack('>') = 0.0625; dual: z[0] at lb may be anything above:
    # -z[0] = 4; z[1] at ub: z[1] = 8; y('<') = 0.5; -y('>') = -2
    assert lbr.evaluate_basic(M, u)[:3] == (0.5, 8.0, -5.0)
