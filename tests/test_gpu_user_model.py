"""GPU: an LP in user form through ipxk_lp_* (ipx_amd/csrc/user_model.hip) -- presolve, postsolve, evaluation, solve.

1. The solver form equals the reference's UserModel::Load + Presolver::PresolveModel bit for bit (`ref.model`, recorded in
   tests/golden/ref_calls/test_gpu_user_model.npz), and equals this file's NumPy restatement of src/sparse_matrix.cc:49-69
   and src/presolver.cc:118-292, 883-974 (np_presolve).  Cases g and h have unsorted columns and explicit zeros, in the
   primal and in the dualized form.  The reference's Control in ref.model has default parameters only, so the forced modes
   (dualize = 0 / 1 against the automatic choice) are compared against np_presolve alone -- which the same test holds
   against the reference on the automatic cases.
2. One invalid model per check -1 .. -8 of src/user_model.cc:217-264.  (A rejection raises inside the reference call,
   which the recorder cannot store: the reference's verdicts are kept in tests/golden/user_model_rejections.json under a
   digest of the arguments, and held against the live build where there is one.)
3. ipxk_lp_postsolve equals np_postsolve (src/presolver.cc:618-793) exactly on a random iterate.
4. ipxk_lp_evaluate: norms exact, residuals and objectives within the rounding bounds worked out below, twice the same bits.
5. Solve, postsolve, evaluate on LPs with a planted primal-dual pair; the objective against the reference's own solver.
"""
import json
import os

import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

INF = np.inf
EPS = np.finfo(np.float64).eps
FEASIBILITY_TOL = 1e-6
LB, UB, BOXED, FREE_STATE = 2, 3, 4, 1


# ---- models ------------------------------------------------------------------------------------------------------------
def make_lp(nc, nv, seed, eq_every=3, unsorted=False, well_scaled=False, kmax=5, zeros=0):
    """A = R B C with |B| in [1, 2) and R, C powers of two with exponents in [-6, 6]: magnitudes 2^u, u in [-12, 12], so
    that several equilibration rounds run (well_scaled: all entries in [0.5, 8) instead).  Row types cycle through
    = < > (an equality every eq_every rows), bound kinds through lower-only, upper-only, boxed, fixed, free; a column has 1
    to kmax entries; column 3 and row 5 are empty; `zeros` of the entries are explicit zeros.  rhs and obj come from a planted
    strictly complementary primal-dual pair, so the LP is feasible and bounded."""
    rng = np.random.default_rng(seed)
    R = 2.0 ** rng.integers(-6, 7, nc)
    Cs = 2.0 ** rng.integers(-6, 7, nv)
    if well_scaled:
        R[:], Cs[:] = 1.0, 1.0
    cols = []
    allowed = np.setdiff1d(np.arange(nc), [5])
    for j in range(nv):
        k = 0 if j == 3 or nc < 8 else int(rng.integers(1, kmax + 1))
        rows = rng.choice(allowed, size=k, replace=False) if k else np.zeros(0, np.int64)
        rows = rows if unsorted else np.sort(rows)
        vals = rng.choice([-1.0, 1.0], k) * (rng.uniform(0.5, 8.0, k) if well_scaled else rng.uniform(1.0, 2.0, k))
        cols.append((rows.astype(np.int64), vals * R[rows] * Cs[j]))
    Ap = np.concatenate([[0], np.cumsum([len(r) for r, _ in cols])]).astype(np.int64)
    Ai = np.concatenate([r for r, _ in cols]).astype(np.int64) if nv else np.zeros(0, np.int64)
    Ax = np.concatenate([v for _, v in cols]) if nv else np.zeros(0)
    if zeros:
        Ax[np.random.default_rng(seed + 1000).choice(Ax.size, zeros, replace=False)] = 0.0
    ct = np.array(["=" if i % eq_every == 0 else "<" if i % 2 else ">" for i in range(nc)], dtype="U1")
    if nc > 5:
        ct[5] = "<"
    kind = np.arange(nv) % 5                      # 0 lower-only, 1 upper-only, 2 boxed, 3 fixed, 4 free
    kind[3 % nv] = 0
    # planted pair, in the scaled variables xh = C x, yh = y / R
    xh = rng.uniform(-2.0, 2.0, nv)
    lbh, ubh = np.full(nv, -INF), np.full(nv, INF)
    zl, zu = np.zeros(nv), np.zeros(nv)
    active = rng.random(nv) < 0.5
    for j in range(nv):
        z = rng.uniform(0.5, 2.0)
        if kind[j] == 0:
            lbh[j] = xh[j] if active[j] else xh[j] - rng.uniform(0.5, 2.0)
            zl[j] = z if active[j] else 0.0
        elif kind[j] == 1:
            ubh[j] = xh[j] if active[j] else xh[j] + rng.uniform(0.5, 2.0)
            zu[j] = z if active[j] else 0.0
        elif kind[j] == 2:
            lbh[j], ubh[j] = xh[j] - rng.uniform(0.5, 2.0), xh[j] + rng.uniform(0.5, 2.0)
            if active[j]:
                if rng.random() < 0.5:
                    lbh[j], zl[j] = xh[j], z
                else:
                    ubh[j], zu[j] = xh[j], z
        elif kind[j] == 3:
            lbh[j] = ubh[j] = xh[j]
            zl[j], zu[j] = (z, 0.0) if active[j] else (0.0, z)
    x, lb, ub = xh / Cs, lbh / Cs, ubh / Cs
    zl, zu = zl * Cs, zu * Cs
    yh = rng.uniform(-2.0, 2.0, nc)
    slack = np.zeros(nc)
    tight = rng.random(nc) < 0.5
    for i in range(nc):
        if ct[i] == "<":
            yh[i], slack[i] = (-abs(yh[i]) - 0.5, 0.0) if tight[i] else (0.0, rng.uniform(0.5, 2.0))
        elif ct[i] == ">":
            yh[i], slack[i] = (abs(yh[i]) + 0.5, 0.0) if tight[i] else (0.0, -rng.uniform(0.5, 2.0))
    y, slack = yh / R, slack * R
    A = po.Csc(nc, nv, Ap, Ai, Ax)
    colof = np.repeat(np.arange(nv), np.diff(Ap))
    rhs = np.bincount(Ai, Ax * x[colof], minlength=nc)[:nc] + slack if nc else np.zeros(0)
    obj = np.bincount(colof, Ax * y[Ai], minlength=nv) + zl - zu
    return dict(A=A, rhs=rhs, ct="".join(ct), obj=obj, lb=lb, ub=ub, nc=nc, nv=nv, planted_objective=float(obj @ x))


CASES = {
    "a": lambda: make_lp(130, 300, 11),
    "b": lambda: make_lp(400, 90, 12, eq_every=10, unsorted=True),
    "g": lambda: make_lp(130, 300, 16, unsorted=True, zeros=7),             # primal: LoadFromArrays sorts the columns, drops the zeros
    "h": lambda: make_lp(400, 90, 17, eq_every=10, unsorted=True, zeros=5),  # dualized
    "d": lambda: make_lp(60, 140, 13, well_scaled=True),
    "e": lambda: make_lp(0, 40, 14),
    "f": lambda: make_lp(4000, 9000, 15, kmax=16),           # more than 2^16 entries: the layouts are built on the device
}
_models = {}


def model(name):
    if name not in _models:
        _models[name] = CASES[name]()
    return _models[name]


# ---- NumPy restatements --------------------------------------------------------------------------------------------------
def np_equilibrate(m, n, Ap, Ai, Ax):
    """Presolver::EquilibrateMatrix (src/presolver.cc:883-974): (Ax, colscale, rowscale, rounds)"""
    Ax = Ax.copy()
    cs, rs = np.ones(n), np.ones(m)
    exp = np.frexp(np.abs(Ax))[1]
    if not ((exp < 0) | (exp > 3)).any():
        return Ax, cs, rs, -1
    colof = np.repeat(np.arange(n), np.diff(Ap))

    def factor(mx):
        e = np.frexp(mx)[1]
        return np.where(e < 0, np.ldexp(1.0, (0 - e + 1) // 2), np.where(e > 3, np.ldexp(1.0, -((e - 3 + 1) // 2)), 1.0))
    rounds = 0
    for _ in range(10):
        cmax, rmax = np.zeros(n), np.zeros(m)
        np.maximum.at(cmax, colof, np.abs(Ax))
        np.maximum.at(rmax, Ai, np.abs(Ax))
        cf, rf = factor(cmax), factor(rmax)
        rs, cs = rs * rf, cs * cf
        if (cf == 1.0).all() and (rf == 1.0).all():
            break
        Ax = Ax * cf[colof] * rf[Ai]
        rounds += 1
    return Ax, cs, rs, rounds


def np_load(A):
    """SparseMatrix::LoadFromArrays (src/sparse_matrix.cc:49-69), the end of UserModel::CopyInput: the explicit zeros are
    dropped and every column is sorted by row index (no index repeats in a valid model): (Ap, Ai, Ax)"""
    colof = np.repeat(np.arange(A.ncol), np.diff(A.p))
    keep = A.x != 0.0
    colof, i, x = colof[keep], A.i[keep], A.x[keep]
    order = np.lexsort((i, colof))
    p = np.concatenate([[0], np.cumsum(np.bincount(colof, minlength=A.ncol))]).astype(np.int64)
    return p, i[order].astype(np.int64), x[order]


def np_presolve(M, dualize=-1, scale=1):
    """LoadFromArrays, ComputeUserModelAttributes, LoadPrimal / LoadDual, ScaleModel (src/presolver.cc:118-292)"""
    A, rhs, obj, lbu, ubu, nc, nv = M["A"], M["rhs"], M["obj"], M["lb"], M["ub"], M["nc"], M["nv"]
    ct = np.array(list(M["ct"]), dtype="U1") if nc else np.zeros(0, "U1")
    has_lb, has_ub = np.isfinite(lbu), np.isfinite(ubu)
    boxed = np.nonzero(has_lb & has_ub)[0]
    Lp, Li, Lx = np_load(A)
    if dualize < 0:
        dualize = nc > 2 * nv
    if not dualize:
        m, n = nc, nv
        Ap, Ai, Ax = Lp, Li, Lx
        b = rhs.copy()
        c = np.concatenate([obj, np.zeros(nc)])
        lb = np.concatenate([lbu, np.where(ct == ">", -INF, 0.0)])
        ub = np.concatenate([ubu, np.where(ct == "<", INF, 0.0)])
        flipped = np.zeros(0, np.int64)
    else:
        m, n = nv, nc + boxed.size
        isflip = np.isinf(lbu) & has_ub
        flipped = np.nonzero(isflip)[0]
        colof = np.repeat(np.arange(nv), np.diff(Lp))
        order = np.argsort(Li, kind="stable")                       # Transpose: ascending source column within a row
        Ti, Tx = colof[order], Lx[order].copy()
        Tp = np.concatenate([[0], np.cumsum(np.bincount(Li, minlength=nc))]).astype(np.int64)
        Tx[isflip[Ti]] *= -1.0
        Ap = np.concatenate([Tp, Tp[-1] + 1 + np.arange(boxed.size)]).astype(np.int64)
        Ai = np.concatenate([Ti, boxed]).astype(np.int64)
        Ax = np.concatenate([Tx, -np.ones(boxed.size)])
        b = np.where(isflip, obj * -1.0, obj)
        l = np.where(isflip, -ubu, lbu)
        c = np.concatenate([-rhs, ubu[boxed], np.where(np.isfinite(l), -l, 0.0)])
        lb = np.concatenate([np.where(ct == ">", 0.0, -INF), np.zeros(boxed.size), np.zeros(nv)])
        ub = np.concatenate([np.where(ct == "<", 0.0, INF), np.full(boxed.size, INF), np.where(np.isfinite(l), INF, 0.0)])
    cs, rs, rounds = np.ones(n), np.ones(m), -1
    if scale >= 1:
        Ax, cs, rs, rounds = np_equilibrate(m, n, Ap, Ai, Ax)
    with np.errstate(invalid="ignore"):
        c[:n] *= cs; lb[:n] /= cs; ub[:n] /= cs
        b *= rs; c[n:] /= rs; lb[n:] *= rs; ub[n:] *= rs
    return dict(m=m, n=n, dualized=int(bool(dualize)), Ap=Ap, Ai=Ai, Ax=Ax, b=b, c=c, lb=lb, ub=ub, colscale=cs, rowscale=rs,
                rounds=rounds, boxed=boxed, flipped=flipped)


def np_postsolve(M, S, it):
    """Presolver::PostsolveInteriorPoint (src/presolver.cc:618-793); S = np_presolve's result, it = the solver's iterate"""
    nc, nv, n = M["nc"], M["nv"], S["n"]
    ct = np.array(list(M["ct"]), dtype="U1") if nc else np.zeros(0, "U1")
    cs, rs = S["colscale"], S["rowscale"]
    eq, lt = ct == "=", ct == "<"
    with np.errstate(invalid="ignore"):
        if S["dualized"]:
            nb = S["boxed"].size
            x = -it["y"] * rs
            y = np.where(eq, it["x"][:nc] * cs[:nc], np.where(lt, -it["xu"][:nc] * cs[:nc], it["xl"][:nc] * cs[:nc]))
            fixed = S["lb"][n:] == S["ub"][n:]                       # the lb == ub slack rule
            zl = np.where(fixed, 0.0, it["xl"][n:] / rs)
            zu = np.zeros(nv)
            zu[S["boxed"]] = it["xl"][nc:nc + nb] * cs[nc:nc + nb]
            xl = np.where(fixed, INF, it["zl"][n:] * rs)
            xu = np.full(nv, INF)
            xu[S["boxed"]] = it["zl"][nc:nc + nb] / cs[nc:nc + nb]
            slack = np.where(eq, 0.0, np.where(lt, it["zu"][:nc] / cs[:nc], -it["zl"][:nc] / cs[:nc]))
            f = S["flipped"]
            x[f] *= -1.0
            xu[f] = xl[f]; xl[f] = INF
            zu[f] = zl[f]; zl[f] = 0.0
        else:
            x = it["x"][:nv] * cs
            y = np.where(eq, it["y"] * rs, np.where(lt, -it["zl"][n:] * rs, it["zu"][n:] * rs))
            zl, zu = it["zl"][:nv] / cs, it["zu"][:nv] / cs
            xl, xu = it["xl"][:nv] * cs, it["xu"][:nv] * cs
            slack = np.where(eq, 0.0, np.where(lt, it["xl"][n:] / rs, -it["xu"][n:] / rs))
    return dict(x=x, xl=xl, xu=xu, slack=slack, y=y, zl=zl, zu=zu)


def random_iterate(S, seed):
    """a valid solver-form iterate (infinite xl / xu and zero zl / zu at infinite bounds) and Iterate::Initialize's states"""
    rng = np.random.default_rng(seed)
    m, N = S["m"], S["n"] + S["m"]
    lb, ub = S["lb"], S["ub"]
    it = dict(x=rng.normal(size=N), y=rng.normal(size=m),
              xl=np.where(np.isfinite(lb), rng.uniform(0.1, 2.0, N), INF), xu=np.where(np.isfinite(ub), rng.uniform(0.1, 2.0, N), INF),
              zl=np.where(np.isfinite(lb), rng.uniform(0.1, 2.0, N), 0.0), zu=np.where(np.isfinite(ub), rng.uniform(0.1, 2.0, N), 0.0))
    st = np.full(N, BOXED, np.uint8)
    st[np.isinf(lb) & np.isinf(ub)] = FREE_STATE
    st[np.isfinite(lb) & np.isinf(ub)] = LB
    st[np.isinf(lb) & np.isfinite(ub)] = UB
    return it, st


def new_lp(M, **kw):
    from ipx_amd import kkt
    return kkt.Lp(M["A"], M["rhs"], M["ct"], M["obj"], M["lb"], M["ub"], **kw)


def with_identity(m, Ap, Ai, Ax):
    return (np.concatenate([Ap, Ap[-1] + 1 + np.arange(m)]), np.concatenate([Ai, np.arange(m)]), np.concatenate([Ax, np.ones(m)]))


def assert_model_equals(got, S):
    for k in ("Ap", "Ai", "Ax", "b", "c", "lb", "ub", "colscale", "rowscale"):
        assert np.array_equal(got[k], S[k]), k


# ---- 1. presolve -------------------------------------------------------------------------------------------------------
def reference_answers(ref, M):
    """every question a presolve test asks of the reference, in this order (the recording depends on it)"""
    R = ref.model(M["A"], M["rhs"], M["ct"], M["obj"], M["lb"], M["ub"])
    return dict(m=R.m, n=R.n, dualized=R.dualized, num_dense=R.num_dense, AI=R.AI(), vectors=R.vectors())


def unsorted_columns(A):
    return sum(bool((np.diff(A.i[A.p[j]:A.p[j + 1]]) < 0).any()) for j in range(A.ncol))


@pytest.mark.parametrize("name", ["a", "b", "g", "h", "d", "e"])
def test_presolve_matches_reference(ref, name):
    M = model(name)
    if name in ("g", "h"):                          # (properties of the cases: what LoadFromArrays has to do)
        assert unsorted_columns(M["A"]) > 10 and (M["A"].x == 0.0).sum() >= 5
    R = reference_answers(ref, M)
    S = np_presolve(M)
    lp = new_lp(M)
    got = lp.model()
    info = lp.info
    assert (info["m"], info["n"], info["dualized"], info["num_dense_cols"]) == (R["m"], R["n"], int(R["dualized"]), R["num_dense"])
    assert info["dualized"] == (1 if name in ("b", "h") else 0)
    assert info["nnz"] == (M["A"].x != 0.0).sum() + (S["boxed"].size if S["dualized"] else 0)
    p, i, x = with_identity(lp.m, got["Ap"], got["Ai"], got["Ax"])
    assert np.array_equal(p, R["AI"].p) and np.array_equal(i, R["AI"].i) and np.array_equal(x, R["AI"].x)
    for k, v in zip(("b", "c", "lb", "ub"), R["vectors"]):
        assert np.array_equal(got[k], v), k
    # the restatement says the same, scaling vectors and attributes included
    assert_model_equals(got, S)
    assert info["scale_rounds"] == S["rounds"]
    assert info["num_boxed"] == S["boxed"].size and info["num_flipped"] == S["flipped"].size
    assert info["num_free_var"] == int((np.isinf(M["lb"]) & np.isinf(M["ub"])).sum())
    assert info["num_eqconstr"] == M["ct"].count("=")
    if name in ("a", "b"):
        assert S["rounds"] >= 2                     # (a property of the case: several equilibration rounds run)
    if name == "d":
        assert info["scale_rounds"] == -1 and (got["colscale"] == 1.0).all() and (got["rowscale"] == 1.0).all()
    lp.close()


@pytest.mark.parametrize("name,dualize", [("b", 0), ("a", 1), ("h", 0), ("g", 1)])
def test_presolve_forced_mode(name, dualize):
    """The reference object of the tests has default parameters only: the forced modes are held against np_presolve."""
    M = model(name)
    S = np_presolve(M, dualize=dualize)
    lp = new_lp(M, dualize=dualize)
    assert (lp.info["m"], lp.info["n"], lp.info["dualized"]) == (S["m"], S["n"], dualize)
    assert_model_equals(lp.model(), S)
    assert lp.info["num_boxed"] == S["boxed"].size and lp.info["num_flipped"] == S["flipped"].size
    lp.close()


def test_presolve_without_scaling():
    M = model("a")
    S = np_presolve(M, scale=0)
    lp = new_lp(M, scale=0)
    assert lp.info["scale_rounds"] == -1
    assert_model_equals(lp.model(), S)
    lp.close()


def test_presolve_and_solve_beyond_the_small_matrices():
    """From 2^16 entries on the context's layouts come from the device builders, which have no host arrays to fall back on
    here.  The presolve is held against np_presolve; the solve against the planted optimum: the returned point's
    objectives bracket it up to the permitted infeasibility (weak duality), as in test_objective_against_reference_solver."""
    M = model("f")
    assert M["A"].nnz >= 1 << 16
    S = np_presolve(M)
    lp = new_lp(M)
    assert_model_equals(lp.model(), S)
    info = lp.solve()
    ev = lp.evaluate()
    lp.close()
    assert info["status_ipm"] == 1, info
    p = M["planted_objective"]
    assert abs(ev["pobjval"] - p) <= abs(ev["pobjval"] - ev["dobjval"]) + FEASIBILITY_TOL * (1.0 + abs(p)), (ev, p)


def test_recording_is_small():
    import refcalls
    path = os.path.join(refcalls.GOLD, "test_gpu_user_model.npz")
    assert os.path.exists(path) and os.path.getsize(path) <= refcalls.MAX_BYTES


# ---- 2. validation -----------------------------------------------------------------------------------------------------
def invalid_models():
    """(check number, first offending index, model): one model per check of CheckVectors / CheckMatrix"""
    base = make_lp(12, 20, 21)

    def variant(**kw):
        M = dict(base)
        for k, v in kw.items():
            M[k] = v
        return M

    def changed(a, idx, val):
        a = a.copy()
        a[idx] = val
        return a
    A = base["A"]
    out = [(-1, 7, variant(rhs=changed(changed(base["rhs"], 9, INF), 7, np.nan))),
           (-2, 4, variant(obj=changed(base["obj"], 4, -INF))),
           (-3, 2, variant(lb=changed(base["lb"], 2, INF))),
           (-3, 6, variant(lb=changed(base["lb"], 6, 1.0), ub=changed(base["ub"], 6, 0.5))),
           (-4, 3, variant(ct=base["ct"][:3] + "x" + base["ct"][4:])),
           (-5, 5, variant(A=po.Csc(12, 20, changed(A.p, 6, A.p[5] - 1), A.i, A.x))),
           (-6, 10, variant(A=po.Csc(12, 20, A.p, A.i, changed(A.x, 10, np.nan)))),
           (-7, 8, variant(A=po.Csc(12, 20, A.p, changed(changed(A.i, 8, 12), A.nnz - 1, -1), A.x)))]
    # a row index twice in a column whose entries are not sorted: column j gets (r, s, r)
    j = int(np.nonzero(np.diff(A.p) >= 3)[0][0])
    p0 = int(A.p[j])
    r = int(A.i[p0 + 1])
    s = int(np.setdiff1d(np.arange(12), A.i[p0:A.p[j + 1]]).max())
    Ai = changed(changed(changed(A.i, p0, r), p0 + 1, s), p0 + 2, r)
    out.append((-8, p0 + 2, variant(A=po.Csc(12, 20, A.p, Ai, A.x))))
    return out


REJECTIONS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "user_model_rejections.json")


def reference_verdict(live_ref, M):
    """What ref.model says to a model: "accepted" or the name of what it raises.  Asked of the live build where there is
    one (IPXK_REF=record stores the answer); the recorded verdict is the one for these very arguments, bit for bit."""
    import refcalls
    args = (M["A"], M["rhs"], M["ct"], M["obj"], M["lb"], M["ub"])
    key = refcalls.digest(args, {})
    recorded = {}
    if os.path.exists(REJECTIONS):
        with open(REJECTIONS) as f:
            recorded = json.load(f)
    if live_ref is None:
        assert key in recorded, "no recorded verdict of the reference for this model (re-record)"
        return recorded[key]
    try:
        live_ref.model(*args)
        verdict = "accepted"
    except Exception as e:
        verdict = type(e).__name__
    if os.environ.get("IPXK_REF") == "record":
        recorded[key] = verdict
        with open(REJECTIONS, "w") as f:
            json.dump(dict(sorted(recorded.items())), f, indent=0)
            f.write("\n")
    else:
        assert recorded.get(key) == verdict, "the recorded verdict differs from the live build's (re-record)"
    return verdict


@pytest.mark.parametrize("k", range(9))
def test_validation(live_ref, k):
    from ipx_amd import kkt
    check, index, M = invalid_models()[k]
    with pytest.raises(kkt.KktError) as e:
        new_lp(M)
    assert e.value.code == -3                    # IPXK_E_ARGUMENT
    assert "check %d " % check in str(e.value) and str(e.value).endswith("index %d" % index), str(e.value)
    assert reference_verdict(live_ref, M) == "ValueError"


def test_validation_dimensions():
    from ipx_amd import kkt
    M = make_lp(4, 6, 22)
    with pytest.raises(kkt.KktError):
        kkt.Lp(po.Csc(4, 0, np.zeros(1, np.int64), np.zeros(0, np.int64), np.zeros(0)), M["rhs"], M["ct"], np.zeros(0), np.zeros(0),
               np.zeros(0))


# ---- 3. / 4. postsolve and evaluation of a given iterate -------------------------------------------------------------------
@pytest.fixture(scope="module", params=["a", "b"])
def loaded(request):
    M = model(request.param)
    S = np_presolve(M)
    lp = new_lp(M)
    it, st = random_iterate(S, 31)
    lp.context.iterate_set(it, st)
    yield M, S, lp, it
    lp.close()


def test_postsolve(loaded):
    M, S, lp, it = loaded
    got, want = lp.interior_solution(), np_postsolve(M, S, it)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    # the restatement's branches are all taken
    ct = M["ct"]
    assert all(t in ct for t in "=<>")
    if S["dualized"]:
        n = S["n"]
        assert S["boxed"].size and S["flipped"].size and (S["lb"][n:] == S["ub"][n:]).any()
        assert np.isinf(got["xl"][S["flipped"]]).all() and (got["zl"][S["flipped"]] == 0.0).all()
        assert np.isfinite(got["xu"][S["boxed"]]).all()


def test_evaluate(loaded):
    M, S, lp, it = loaded
    nc, nv, A = M["nc"], M["nv"], M["A"]
    u = np_postsolve(M, S, it)
    ev = lp.evaluate(residuals=True)
    ev2 = lp.evaluate(residuals=True)
    for k in ev:
        assert np.array_equal(ev[k], ev2[k]), k                   # two calls, the same bits
    lbf, ubf = np.isfinite(M["lb"]), np.isfinite(M["ub"])
    # max-norm quantities: exact
    assert ev["normx"] == np.abs(u["x"]).max() and ev["normy"] == np.abs(u["y"]).max()
    assert ev["normz"] == max(np.abs(u["zl"]).max(), np.abs(u["zu"]).max())
    assert ev["norm_obj"] == np.abs(M["obj"]).max() and ev["norm_rhs"] == np.abs(M["rhs"]).max()
    assert ev["norm_bounds"] == max(np.abs(M["lb"][lbf]).max(), np.abs(M["ub"][ubf]).max())
    with np.errstate(invalid="ignore"):          # (inf - inf at the infinite bounds, masked out)
        bound_res = max(np.abs(M["lb"] - u["x"] + u["xl"])[lbf].max(), np.abs(M["ub"] - u["x"] - u["xu"])[ubf].max())
    assert ev["abs_presidual"] == max(np.abs(ev["rb"]).max(), bound_res)
    assert ev["abs_dresidual"] == np.abs(ev["rc"]).max()
    assert ev["rel_presidual"] == ev["abs_presidual"] / (1.0 + max(ev["norm_rhs"], ev["norm_bounds"]))
    assert ev["rel_dresidual"] == ev["abs_dresidual"] / (1.0 + ev["norm_obj"])
    # residual vectors: a sum of k terms evaluated in any order is within (k - 1) u sum|terms| (1 + O(u)) of the exact sum,
    # u = EPS / 2, and every product adds u |term|; k * EPS * sum|terms| with k = row length + 2 covers both.  The
    # comparison value is computed in extended precision, whose own error is 2^-11 of that.
    L = np.longdouble
    D = np.zeros((nc, nv), L)
    colof = np.repeat(np.arange(nv), np.diff(A.p))
    D[A.i, colof] = A.x
    rb = (M["rhs"].astype(L) - u["slack"].astype(L)) - D @ u["x"].astype(L)
    rb_mag = np.abs(D) @ np.abs(u["x"]).astype(L) + np.abs(u["slack"]) + np.abs(M["rhs"])
    krow = np.bincount(A.i, minlength=nc) + 2
    assert (np.abs(ev["rb"] - rb) <= krow * EPS * rb_mag).all()
    rc = (M["obj"].astype(L) - u["zl"].astype(L) + u["zu"].astype(L)) - D.T @ u["y"].astype(L)
    rc_mag = np.abs(D.T) @ np.abs(u["y"]).astype(L) + np.abs(u["zl"]) + np.abs(u["zu"]) + np.abs(M["obj"])
    kcol = np.diff(A.p) + 3
    assert (np.abs(ev["rc"] - rc) <= kcol * EPS * rc_mag).all()
    # dot products: the same bound with k = the number of terms
    pobj = (M["obj"].astype(L) * u["x"].astype(L)).sum()
    assert abs(ev["pobjval"] - pobj) <= nv * EPS * np.abs(M["obj"] * u["x"]).sum()
    tl, tu = np.where(lbf, M["lb"], 0.0) * u["zl"], np.where(ubf, M["ub"], 0.0) * u["zu"]
    dobj = (M["rhs"].astype(L) * u["y"].astype(L)).sum() + tl.astype(L).sum() - tu.astype(L).sum()
    dmag = np.abs(M["rhs"] * u["y"]).sum() + np.abs(tl).sum() + np.abs(tu).sum()
    assert abs(ev["dobjval"] - dobj) <= (nc + 2 * nv) * EPS * dmag
    comp = (np.where(lbf, u["xl"], 0.0) * u["zl"]).astype(L).sum() + (np.where(ubf, u["xu"], 0.0) * u["zu"]).astype(L).sum() \
        - (u["y"].astype(L) * u["slack"].astype(L)).sum()
    cmag = np.abs(np.where(lbf, u["xl"], 0.0) * u["zl"]).sum() + np.abs(np.where(ubf, u["xu"], 0.0) * u["zu"]).sum() \
        + np.abs(u["y"] * u["slack"]).sum()
    assert abs(ev["complementarity"] - comp) <= (nc + 2 * nv) * EPS * cmag
    assert ev["rel_objgap"] == (ev["pobjval"] - ev["dobjval"]) / (1.0 + 0.5 * abs(ev["pobjval"] + ev["dobjval"]))


def test_postsolve_and_evaluate_without_constraints():
    """num_constr = 0: no y, slack or rb, the row quantities are maxima and sums of nothing, and rc has no A'y in it"""
    M = model("e")
    S = np_presolve(M)
    lp = new_lp(M)
    it, st = random_iterate(S, 32)
    lp.context.iterate_set(it, st)
    got, want = lp.interior_solution(), np_postsolve(M, S, it)
    ev, ev2 = lp.evaluate(residuals=True), lp.evaluate(residuals=True)
    lp.close()
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    for k in ev:
        assert np.array_equal(ev[k], ev2[k]), k
    assert ev["rb"].size == 0 and ev["normy"] == 0.0 and ev["norm_rhs"] == 0.0
    assert np.array_equal(ev["rc"], (0.0 - (want["zl"] - want["zu"])) + M["obj"])      # (the kernel's operations, in its order)
    assert ev["abs_dresidual"] == np.abs(ev["rc"]).max() and ev["normx"] == np.abs(want["x"]).max()


# ---- 5. end to end -------------------------------------------------------------------------------------------------------
_solved = {}


def solved(name):
    """solve, postsolve and evaluate of a case, once for the tests that look at it"""
    if name not in _solved:
        lp = new_lp(model(name))
        info = lp.solve()
        _solved[name] = (info, lp.interior_solution(), lp.evaluate(residuals=True))
        lp.close()
    return _solved[name]


@pytest.mark.parametrize("name", ["a", "b"])
def test_solve_end_to_end(name):
    M = model(name)
    nc, nv, A, ct = M["nc"], M["nv"], M["A"], np.array(list(M["ct"]))
    info, u, ev = solved(name)
    assert info["status_ipm"] == 1, info          # IPX_STATUS_optimal
    # sign conditions
    for k in ("xl", "xu", "zl", "zu"):
        assert (u[k] >= 0.0).all(), k
    assert (u["slack"][ct == "="] == 0.0).all() and (u["slack"][ct == "<"] >= 0.0).all() and (u["slack"][ct == ">"] <= 0.0).all()
    assert (u["y"][ct == "<"] <= 0.0).all() and (u["y"][ct == ">"] >= 0.0).all()
    # The residuals of the returned point are what the evaluation reports.  Both sides are rounded here: each is within
    # k u sum|terms| of the exact value (u = EPS / 2, k as in test_evaluate), so they are within k EPS sum|terms| of each other.
    colof = np.repeat(np.arange(nv), np.diff(A.p))
    Ax_ = np.bincount(A.i, A.x * u["x"][colof], minlength=nc)
    mag = np.bincount(A.i, np.abs(A.x * u["x"][colof]), minlength=nc) + np.abs(u["slack"]) + np.abs(M["rhs"])
    krow = np.bincount(A.i, minlength=nc) + 2
    assert (np.abs((Ax_ + u["slack"] - M["rhs"]) + ev["rb"]) <= krow * EPS * mag).all()
    Aty = np.bincount(colof, A.x * u["y"][A.i], minlength=nv)
    mag = np.bincount(colof, np.abs(A.x * u["y"][A.i]), minlength=nv) + np.abs(u["zl"]) + np.abs(u["zu"]) + np.abs(M["obj"])
    kcol = np.diff(A.p) + 3
    assert (np.abs((M["obj"] - Aty - u["zl"] + u["zu"]) - ev["rc"]) <= kcol * EPS * mag).all()
    assert ev["abs_dresidual"] == np.abs(ev["rc"]).max() and ev["abs_presidual"] >= np.abs(ev["rb"]).max()
    assert ev["rel_presidual"] <= FEASIBILITY_TOL and ev["rel_dresidual"] <= FEASIBILITY_TOL


@pytest.mark.parametrize("name", ["a", "b"])
def test_objective_against_reference_solver(name, tmp_path):
    """The reference's whole solver (tests/dropin/lp_main.cc) on the same model.  Weak duality brackets the optimum for
    each run up to its permitted infeasibility."""
    import test_gpu_lp_dropin as dropin
    if not os.path.exists(dropin.REF_BIN):
        pytest.skip("oracle/_ref/test_lp_ref not built (needs the reference sources at build time)")
    M = model(name)
    A = M["A"]
    info, u, ev = solved(name)
    din = str(tmp_path / "in")
    dropin.write_model(din, M["obj"], M["lb"], M["ub"], A.p, A.i, A.x, M["rhs"], list(M["ct"]), crossover=0)
    ri, _, rout = dropin.run(dropin.REF_BIN, din, str(tmp_path / "ref"), timeout=300)
    assert ri["status_ipm"] == dropin.IPX_STATUS_optimal, rout
    assert abs(ev["pobjval"] - ri["pobjval"]) <= abs(ri["pobjval"] - ri["dobjval"]) + abs(ev["pobjval"] - ev["dobjval"]) \
        + FEASIBILITY_TOL * (1.0 + abs(ri["pobjval"])), (ev, ri)


@pytest.mark.parametrize("dualize", ["-1", "1"])
def test_example_lp_user(dualize):
    """examples/lp_user.cc through the C ABI only: all three row types and the four kinds of bounds; the optimum is known
    (x = (1.5, -0.5, 3, 1.5), objective -2.5, worked out in the file's head), in the primal and in the dual form."""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "examples")])
    r = subprocess.run([os.path.join(root, "examples", "lp_user"), dualize], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ("dualized" if dualize == "1" else "primal") in r.stdout
    x = [float(v) for v in re.findall(r"^x\d = +(\S+)", r.stdout, flags=re.M)]
    # the optimum is the vertex x2 = 3, x0 + x3 = 3, x1 + x3 = 1, x0 + x1 + x2 = 4, whose inverse has row sums of at most 2:
    # residuals within 1e-6 (1 + 4) move it by at most 1e-5
    assert np.allclose(x, [1.5, -0.5, 3.0, 1.5], atol=1e-5, rtol=0), r.stdout
    # an `optimal` point's objective is within the gap (1e-8 relative) plus the permitted infeasibility of the optimum
    assert abs(float(re.search(r"objective (\S+)", r.stdout).group(1)) + 2.5) <= (FEASIBILITY_TOL + 1e-8) * (1.0 + 2.5), r.stdout
