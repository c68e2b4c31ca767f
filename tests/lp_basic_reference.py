"""NumPy restatement of the user-form basic solution: Presolver::PostsolveGeneralPoint (src/presolver.cc:566-616),
PostsolveBasis (:795-845), CorrectBasicSolution (:847-867), LpSolver's BuildBasicStatuses (src/lp_solver.cc:212-231) and
UserModel::EvaluateBasicPoint (src/user_model.cc:173-211).  No device code.  M is a model of test_gpu_user_model.make_lp,
S the result of its np_presolve.  tests/test_lp_basic_reference.py holds this file to something other than itself."""
import math

import numpy as np

BASIC, NONBASIC, NONBASIC_LB, NONBASIC_UB, SUPERBASIC = 0, -1, -1, -2, -3


def general_point(M, S, x, y, z):
    """PostsolveGeneralPoint: dict(x, slack, y, z) in user form, one IEEE operation per entry (two for a boxed variable's z)"""
    nc, nv, n = M["nc"], M["nv"], S["n"]
    cs, rs = S["colscale"], S["rowscale"]
    if S["dualized"]:
        nb = S["boxed"].size
        xu = -y * rs
        zu = x[n:] / rs
        slack = -z[:nc] / cs[:nc]
        yu = x[:nc] * cs[:nc]
        zu[S["boxed"]] = zu[S["boxed"]] - x[nc:nc + nb] * cs[nc:nc + nb]       # (the product is exact: colscale is a power of two)
        f = S["flipped"]
        xu[f] = xu[f] * -1.0
        zu[f] = zu[f] * -1.0
    else:
        xu, zu = x[:nv] * cs, z[:nv] / cs
        slack, yu = x[n:] / rs, y * rs
    return dict(x=xu, slack=slack, y=yu, z=zu)


def check_statuses(S, st):
    """the asserts of PostsolveBasis as exceptions"""
    n, st = S["n"], np.asarray(st)
    if (st[n:] == SUPERBASIC).any():
        raise ValueError("a slack variable is superbasic: slack %d" % int(np.nonzero(st[n:] == SUPERBASIC)[0][0]))
    if S["dualized"]:
        nc, nb = n - S["boxed"].size, S["boxed"].size
        bad = (st[nc:nc + nb] == BASIC) & (st[n + S["boxed"]] == BASIC)
        if bad.any():
            raise ValueError("the added column of boxed variable number %d is basic and so is its slack" % int(np.nonzero(bad)[0][0]))


def postsolve_basis(M, S, st):
    """PostsolveBasis: (cbasis, vbasis)"""
    check_statuses(S, st)
    nc, nv, n, st = M["nc"], M["nv"], S["n"], np.asarray(st, np.int64)
    if S["dualized"]:
        nb = S["boxed"].size
        cbasis = np.where(st[:nc] == BASIC, NONBASIC, BASIC)
        vbasis = np.where(st[n:] == BASIC, np.where(S["lb"][n:] != S["ub"][n:], NONBASIC_LB, SUPERBASIC), BASIC)
        j = S["boxed"][st[nc:nc + nb] == BASIC]
        vbasis[j] = NONBASIC_UB
        f = S["flipped"]
        vbasis[f] = np.where(vbasis[f] == NONBASIC_LB, NONBASIC_UB, vbasis[f])
    else:
        cbasis = np.where(st[n:] == BASIC, BASIC, NONBASIC)
        vbasis = st[:nv].copy()
    return cbasis.astype(np.int64), vbasis.astype(np.int64)


def correct(M, u, cbasis, vbasis):
    """CorrectBasicSolution on a copy of u"""
    x, slack, y, z = (u[k].copy() for k in ("x", "slack", "y", "z"))
    x[vbasis == NONBASIC_LB] = M["lb"][vbasis == NONBASIC_LB]
    x[vbasis == NONBASIC_UB] = M["ub"][vbasis == NONBASIC_UB]
    z[vbasis == BASIC] = 0.0
    slack[cbasis == NONBASIC] = 0.0
    y[cbasis == BASIC] = 0.0
    return dict(x=x, slack=slack, y=y, z=z)


def postsolve_basic(M, S, x, y, z, st):
    """PostsolveBasicSolution: dict(x, slack, y, z, cbasis, vbasis)"""
    cbasis, vbasis = postsolve_basis(M, S, st)
    out = correct(M, general_point(M, S, x, y, z), cbasis, vbasis)
    out.update(cbasis=cbasis, vbasis=vbasis)
    return out


def build_statuses(S, basis):
    """BuildBasicStatuses"""
    st = np.where(np.isfinite(S["lb"]), NONBASIC_LB, np.where(np.isfinite(S["ub"]), NONBASIC_UB, SUPERBASIC)).astype(np.int64)
    st[np.asarray(basis, np.int64)] = BASIC
    return st


def evaluate_basic(M, u):
    """EvaluateBasicPoint: (primal_infeas, dual_infeas, objval as math.fsum of the rounded products, the sum of their
    magnitudes).  std::max(a, b) keeps a when b is a NaN and the running maximum starts at 0, so a NaN (inf - inf at an
    infinite bound) never enters: np.fmax.  The maxima then do not depend on the order they are taken in."""
    ct = np.array(list(M["ct"]), dtype="U1") if M["nc"] else np.zeros(0, "U1")
    x, slack, y, z, vb = u["x"], u["slack"], u["y"], u["z"], u["vbasis"]
    with np.errstate(invalid="ignore"):
        p = [M["lb"] - x, x - M["ub"], -slack[ct == "<"], slack[ct == ">"], np.abs(slack[ct == "="])]
        d = [z[vb != NONBASIC_LB], -z[vb != NONBASIC_UB], y[ct == "<"], -y[ct == ">"]]
        terms = M["obj"] * x
    return (float(np.fmax.reduce(np.concatenate(p), initial=0.0)), float(np.fmax.reduce(np.concatenate(d), initial=0.0)),
            math.fsum(terms), math.fsum(np.abs(terms)))


def planted_statuses(M, S, seed, phase=0):
    """Valid solver-form statuses in which every value occurs on structurals and every legal one (all but superbasic) on
    slacks.  For a dualized model the added column of every other boxed variable and the slack of every other flipped
    variable is basic, the rest nonbasic; phase 1 swaps the two halves, so that over both phases every boxed and every
    flipped variable occurs in both states."""
    rng = np.random.default_rng(seed)
    n, m = S["n"], S["m"]
    st = np.concatenate([rng.integers(-3, 1, n), rng.integers(-2, 1, m)]).astype(np.int64)
    if S["dualized"]:
        nb, nc = S["boxed"].size, n - S["boxed"].size
        st[nc:n] = np.where(np.arange(nb) % 2 == phase, BASIC, rng.integers(-3, 0, nb))
        own = n + S["boxed"]
        st[own] = np.where(st[nc:n] == BASIC, rng.integers(-2, 0, nb), st[own])   # a basic added column needs a nonbasic slack
        f = n + S["flipped"]
        st[f] = np.where(np.arange(f.size) % 2 == phase, BASIC, NONBASIC_LB)
    return st
