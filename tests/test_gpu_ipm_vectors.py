"""GPU: the vector kernels of the device interior-point layer (iterate.hip, ipm_step.hip, newton.hip) past one pass of
their grid and at ties, against tests/ipm_reference.py and the oracle (tests/test_ipm_reference.py pins the one to the
other, tests/test_oracle_vs_ref.py the oracle to the reference's ipx::Iterate).

Every kernel there is a grid-stride loop over vec_grid(len) = min(ceil(len / 256), 1024) workgroups of 256 threads: one
pass covers G = 262 144 elements.  The two shapes are the smallest that reach the second pass, the capped grid and the
host's fold over 1024 partials:
  wide  N = n + m = G + 257 (m = 8192, 3 entries per column): the second pass is one full block and one element;
  tall  m = G + 257 (n = 512, 8 entries per column): everything guarded by j < m, and the loops over m.
Elementwise results, max / min and the blocking index are held bit for bit (rb, rc and the shifted Newton component: in
the phased SpMV layout, which keeps the storage order; the other layouts' epilogues are test_gpu_epilogue_layouts.py's);
sums within ipm_reference.sum_bound of the long-double sum, with every term asserted to be more than 1000 bounds wide.
ipxk_step_to_boundary is held to the parallel-minimum rule everywhere, exact and near ties included; how far that rule
lies from the reference's sequential scan is test_ipm_reference.py's measurement, not the device's.
"""
import numpy as np
import pytest

import ipm_reference as ir
from helpers import relerr
from ipx_amd import synth

pytestmark = pytest.mark.gpu
LD = np.longdouble
G = ir.G
STEP_KEYS = ("dx", "dxl", "dxu", "dy", "dzl", "dzu")


@pytest.fixture(scope="module")
def kkt():
    from ipx_amd import kkt as k
    k.load_library()
    return k


@pytest.fixture(autouse=True)
def stop_after_a_device_fault(request):
    """a case that ends in a HIP error ends the file's run: nothing more is started on a device that has faulted"""
    yield
    rep = getattr(request.node, "rep_call", None)
    if rep is not None and rep.failed and any(s in str(rep.longrepr) for s in ("illegal memory access", "hipError", "HIP error")):
        pytest.exit("a HIP error in %s: not starting further cases" % request.node.nodeid, returncode=3)


@pytest.fixture
def phased(monkeypatch):
    """the layout that keeps the storage order of a row's products: rb and rc are bit-exact there"""
    for var in ("IPXK_SLICE_TEST_KB", "IPXK_SLICE_FORCE2", "IPXK_FORCE_COMM", "IPXK_COMM"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("IPXK_SPMV_LAYOUT", "phased")
    return monkeypatch


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def model(name, fixed=True):
    """the shape's model (never modified: the tests copy what they change) with its residuals, computed once"""
    def make():
        P = ir.shape_model(name, fixed)
        by_row, by_col = ir.row_lengths(P["A"])
        assert by_row.max() <= ir.MAX_ROW_LEN and by_col.max() <= ir.MAX_ROW_LEN       # no row takes the long-row path
        assert P["N"] > G and ir.vec_grid(P["N"]) == ir.GRID_CAP
        P["res"] = ir.residuals(P["A"], P["state"], P["b"], P["c"], P["lbs"], P["ubs"], P["it"])
        return P
    return cached((name, fixed), make)


def context(kkt, A):
    ctx = kkt.KktContext(A)
    assert ctx.spmv_layout()[0] == ("phased", "phased")
    return ctx


def ocsc(A):
    from oracle import pyoracle as po
    return po.Csc(A.nrow, A.ncol, A.p, A.i, A.x)


def copy_it(it):
    return {k: v.copy() for k, v in it.items()}


def within(value, want, bound, what):
    err = abs(LD(value) - want)
    print("%s: error %.3g, bound %.3g" % (what, float(err), float(bound)))
    assert np.isfinite(value) and err <= bound, (what, value, float(want), float(err), float(bound))


def terms_are_wide(terms, bound, what):
    """one dropped or doubled element cannot hide: every nonzero term is more than 1000 bounds (a zero term changes no sum)"""
    t = np.abs(terms[terms != 0.0])
    print("%s: smallest |term| %.3g = %.3g bounds" % (what, t.min(), float(t.min() / bound)))
    assert t.size and t.min() > 1000.0 * bound, what


# ---- (a) elementwise work and reductions ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ir.SHAPES))
def test_set_get_and_update(kkt, oracle, phased, name):
    P = model(name)
    m, n, state, it, st = P["m"], P["n"], P["state"], P["it"], P["step"]
    ctx = context(kkt, P["A"])
    ctx.iterate_set(it, state)
    got = ctx.iterate_get()
    for key in ir.IT_KEYS:
        assert np.array_equal(got[key], it[key]), key
    for sp_, sd_, skip in ir.UPDATES:
        a = {k: (None if k in skip else st[k]) for k in STEP_KEYS}
        want = oracle.iterate_update(m, n, state, it, sp_, a["dx"], a["dxl"], a["dxu"], sd_, a["dy"], a["dzl"], a["dzu"])
        if sp_ == 3.0:                                               # the clamp is reached in the second pass
            assert all((want[key][G:] == ir.BARRIER_MIN).any() for key in ("xl", "xu", "zl", "zu"))
        assert not np.array_equal(want["x"][G:], it["x"][G:]) or "dx" in skip
        assert name != "tall" or "dy" in skip or not np.array_equal(want["y"][G:], it["y"][G:])
        ctx.iterate_set(it, state)
        ctx.iterate_update(sp_, a["dx"], a["dxl"], a["dxu"], sd_, a["dy"], a["dzl"], a["dzu"])
        got = ctx.iterate_get()
        for key in ir.IT_KEYS:
            assert np.array_equal(want[key], got[key]), (key, sp_)
    ctx.close()


@pytest.mark.parametrize("name", list(ir.SHAPES))
def test_residuals_and_their_norms(kkt, phased, name):
    P = model(name)
    A, state, it, want = P["A"], P["state"], P["it"], P["res"]
    b, c, lb, ub, n, m, N = P["b"], P["c"], P["lbs"], P["ubs"], P["n"], P["m"], P["N"]
    ctx = context(kkt, A)
    ctx.iterate_set(it, state)
    got = ctx.iterate_residuals(b, c, lb, ub)
    for key in ("rl", "ru", "rc", "rb"):
        assert np.array_equal(got[key], want[key]), key
    assert (got["presidual"], got["dresidual"]) == (want["presidual"], want["dresidual"])
    assert want["rl"][G:].any() and want["ru"][G:].any() and want["rc"][G:].any() and (name != "tall" or want["rb"][G:].any())
    # the largest |rl|, |ru|, |rc| (|rb|) at every edge in turn: a kernel that drops the tail or the second pass fails
    aty = np.concatenate([ir.col_dots(A, it["y"]), it["y"]])
    places = [(key, j) for key in ("rl", "ru", "rc") for j in P["edges"]] + ([("rb", G), ("rb", m - 1)] if name == "tall" else [])
    for key, j in places:
        b2, c2, lb2, ub2 = b.copy(), c.copy(), lb.copy(), ub.copy()
        vec = {"rl": lb2, "ru": ub2, "rc": c2, "rb": b2}[key]
        vec[j] = (abs(vec[j]) + 1.0) * 1e6
        exp = {k: want[k].copy() for k in ("rb", "rc", "rl", "ru")}
        exp[key][j] = {"rl": lambda: lb2[j] - it["x"][j] + it["xl"][j], "ru": lambda: ub2[j] - it["x"][j] - it["xu"][j],
                       "rc": lambda: ((c2[j] - it["zl"][j]) + it["zu"][j]) - aty[j],
                       "rb": lambda: ir.residual_rb(A, b2, it["x"])[j]}[key]()
        norms = ir.residual_norms(**exp)
        top = norms["dresidual" if key == "rc" else "presidual"]
        assert top == abs(exp[key][j]) > 1e5 and top > 1e3 * max(want["presidual"], want["dresidual"]), (key, j)
        r = ctx.iterate_residuals(b2, c2, lb2, ub2)
        assert r[key][j] == exp[key][j], (key, j)
        assert (r["presidual"], r["dresidual"]) == (norms["presidual"], norms["dresidual"]), (key, j)
    ctx.close()


@pytest.mark.parametrize("name", list(ir.SHAPES))
def test_complementarity(kkt, phased, name):
    P = model(name)
    state, it = P["state"], P["it"]
    ctx = context(kkt, P["A"])

    def check(it_, what, mn=None, mx=None):
        ctx.iterate_set(it_, state)
        got, want = ctx.iterate_complementarity(), ir.complementarity(state, it_)
        bound = ir.sum_bound(want["products"], 2, ir.GRID_CAP)
        assert (got["mu_min"], got["mu_max"]) == (want["mu_min"], want["mu_max"]), what
        assert mn is None or (got["mu_min"], got["mu_max"]) == (mn, mx), what
        within(got["complementarity"], want["sum"], bound, "%s %s: complementarity" % (name, what))
        within(got["mu"], want["mu"], bound / want["count"] + LD(ir.U) * want["mu"], "%s %s: mu" % (name, what))
        assert got["mu"] == got["complementarity"] / want["count"], what          # the count is exact: mu = sum / count
        return want, bound

    want, bound = check(it, "as generated")
    terms_are_wide(want["products"], bound, "%s complementarity" % name)
    lo, hi = 2.0 ** -8, 2.0 ** 10
    assert lo < want["mu_min"] and hi > want["mu_max"]
    for j in P["edges"]:                                             # the extreme products at every edge in turn
        it2 = copy_it(it)
        it2["xl"][j] = it2["zl"][j] = 2.0 ** -4
        it2["xu"][j] = it2["zu"][j] = 2.0 ** 5
        check(it2, "extremes at %d" % j, lo, hi)
    ctx.close()


def test_complementarity_without_a_barrier_term(kkt, phased):
    """cnt == 0: mu = 0 and mu_min = 0 (iterate.cc:666-669)"""
    m, n = 40, 90
    A = synth.synthetic_lp(m, n, 4, 3)
    N = n + m
    state = np.where(np.arange(N) % 3 == 0, ir.FIXED, ir.FREE).astype(np.uint8)
    rng = np.random.default_rng(3)
    it = dict(x=rng.uniform(-1, 1, N), y=rng.uniform(-1, 1, m), xl=np.full(N, np.inf), xu=np.full(N, np.inf), zl=np.zeros(N),
              zu=np.zeros(N))
    ctx = kkt.KktContext(A)
    ctx.iterate_set(it, state)
    assert ctx.iterate_complementarity() == dict(complementarity=0.0, mu=0.0, mu_min=0.0, mu_max=0.0)
    ctx.close()


def objective_inputs(P):
    """the shape's model with every factor of an objective term at least 0.5 in magnitude, so that no term is small"""
    rng = np.random.default_rng(17)
    N, m, n = P["N"], P["m"], P["n"]
    away = lambda q: rng.uniform(0.5, 1.5, q) * rng.choice([-1.0, 1.0], q)
    it = copy_it(P["it"])
    it["x"], it["y"] = away(N), away(m)
    b, c = away(m), np.concatenate([away(n), np.zeros(m)])
    lb = np.where(np.isfinite(P["lbs"]) & (P["lbs"] != 0.0), -rng.uniform(0.5, 2.0, N), P["lbs"])
    return b, c, lb, P["ubs"], it


@pytest.mark.parametrize("name", list(ir.SHAPES))
def test_objectives(kkt, phased, name):
    P = model(name)
    A, state = P["A"], P["state"]
    b, c, lb, ub, it = cached(("objective inputs", name), lambda: objective_inputs(P))
    want = cached(("objectives", name), lambda: ir.objectives(A, state, b, c, lb, ub, it))
    ctx = context(kkt, A)
    ctx.iterate_set(it, state)
    pobj, dobj, offset = ctx.iterate_objectives(b, c, lb, ub)
    ctx.close()
    assert offset != 0.0 and want["fixed_terms"].size >= 4 and (state[P["n"]:] == ir.FIXED).any()
    # additions per thread: two passes; per element one term of pobj or offset, up to four of dobj (b_j y_j, lb_j zl_j,
    # ub_j zu_j, the fixed slack's x_j y_i)
    bp = ir.sum_bound(want["pterms"], 2, ir.GRID_CAP)
    bo = ir.sum_bound(want["oterms"], 2, ir.GRID_CAP)
    # dobj = (the vector kernel's sum) - (the fixed structural x_j A_j'y through the SpMV's dot: whatever its shape, a
    # product passes through its own rounding, at most one addition per product of the dot, the multiplication by x_j,
    # and the final subtraction)
    fp = want["fixed_products"]
    bd = ir.sum_bound(want["dterms"], 8, ir.GRID_CAP) + LD(fp.size + 3) * LD(ir.U) * np.sum(np.abs(fp).astype(LD)) \
        + LD(ir.U) * abs(want["dobj"])
    within(pobj, want["pobj"], bp, name + ": pobjective")
    within(offset, want["offset"], bo, name + ": offset")
    within(dobj, want["dobj"], bd, name + ": dobjective")
    terms_are_wide(want["pterms"], bp, name + ": pobjective")
    terms_are_wide(want["oterms"], bo, name + ": offset")
    terms_are_wide(np.concatenate([want["dterms"], want["fixed_terms"]]), bd, name + ": dobjective")


def test_one_rank_column_partition_reproduces_the_tall_shape(kkt, phased):
    """residuals, complementarity and objectives through the collective code path (IPXK_FORCE_COMM, a one-rank column
    communicator) equal the unpartitioned context's bit for bit, as iterate.hip states: the one way to subtract_slack_kernel
    and EpiIterRbPart on one GPU, here with m > G"""
    from ipx_amd import partition
    P = model("tall")
    A, state, it, b, c, lb, ub = (P[k] for k in ("A", "state", "it", "b", "c", "lbs", "ubs"))

    def run(ctx):
        ctx.iterate_set(it, state)
        out = dict(res=ctx.iterate_residuals(b, c, lb, ub), comp=ctx.iterate_complementarity(),
                   obj=ctx.iterate_objectives(b, c, lb, ub))
        ctx.close()
        return out

    ref = run(context(kkt, A))
    phased.setenv("IPXK_FORCE_COMM", "1")
    phased.setenv("IPXK_COMM", "direct")
    pc = context(kkt, partition.col_slab_matrix(A, 0, A.ncol))
    pc.comm_init(pc.comm_unique_id(), 0, 1, columns=True)
    got = run(pc)
    for key in ("rb", "rc", "rl", "ru"):
        assert np.array_equal(got["res"][key], ref["res"][key]), key
        assert np.array_equal(got["res"][key], P["res"][key]), key
    assert (got["res"]["presidual"], got["res"]["dresidual"]) == (ref["res"]["presidual"], ref["res"]["dresidual"])
    assert got["comp"] == ref["comp"] and got["obj"] == ref["obj"] and ref["obj"][2] != 0.0


# ---- (b) ipxk_step_to_boundary ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(kkt):
    ctx = kkt.KktContext(synth.synthetic_lp(30, 70, 4, 2))
    yield ctx
    ctx.close()


@pytest.mark.parametrize("length", ir.STEP_LENGTHS)
def test_step_to_boundary(tiny, length):
    """random data, nothing blocks, one blocker at the end or at G, would-be blockers beyond alpha0, x = 0: the cases on
    which both rules agree (test_ipm_reference.py), so the reference's scan is the expectation"""
    names = []
    for what, x, dx, alpha0 in ir.step_cases(length):
        assert tiny.step_to_boundary(x, dx, alpha0) == ir.sequential(x, dx, alpha0), (what, length)
        names.append(what)
    assert len(names) == 3 + (length > 0) + (length > G) + (length >= 3)


def test_step_to_boundary_exact_ties(tiny):
    """identical (x, dx) pairs: the smaller index, wherever the smallest-index rule is applied -- per thread over the
    passes, within a wave, over the waves, and over blocks whose smallest index may lie in a later pass"""
    for what, x, dx, want in ir.exact_ties():
        assert tiny.step_to_boundary(x, dx) == ((0.75 * ir.DAMP) / 1.5, want), what


def test_step_to_boundary_near_ties(tiny):
    """scaled copies of one pair: bit-equal to the parallel-minimum rule in alpha and index (the sequential scan differs
    here, inside the window that test_ipm_reference.py measures)"""
    differ = 0
    for length, seed in ir.NEAR_TIE_DEVICE_CASES:
        x, dx, alpha0 = ir.near_tie_family(length, seed)
        want = ir.parallel_min(x, dx, alpha0)
        assert tiny.step_to_boundary(x, dx, alpha0) == want, (length, seed)
        differ += want != ir.sequential(x, dx, alpha0)
    assert differ >= 3                                               # the inputs do separate the two rules


# ---- (c) the Newton step's elementwise work as a function of the device's own (dx, dy) ---------------------------------------
def newton_inputs(P, spread=1.0):
    """the shape's state and residuals; the barrier vectors raised to the power `spread` (a narrower range of the KKT
    weights shortens the CR solve); at the planted boxed variables zl xu == zu xl exactly, in powers of two"""
    state, it = P["state"], P["it"]
    with np.errstate(invalid="ignore"):
        v = {k: np.where(np.isfinite(it[k]) & (it[k] > 0), it[k] ** spread, it[k]) for k in ("xl", "xu", "zl", "zu")}
    tied = np.setdiff1d(P["boxed"], P["edges"])
    assert tied.size == 10 and (tied < G).sum() == 5
    e = np.arange(tied.size) % 4
    v["xl"][tied], v["xu"][tied] = 2.0 ** (1 - e), 2.0 ** (2 + e)
    v["zl"][tied], v["zu"][tied] = 2.0 ** (-1 - e), 2.0 ** e               # zl xu = zu xl = 2
    assert np.array_equal(v["zl"][tied] * v["xu"][tied], v["zu"][tied] * v["xl"][tied])
    lbm, ubm = ir.has_lb(state), ir.has_ub(state)
    prod = np.concatenate([v["xl"][lbm] * v["zl"][lbm], v["xu"][ubm] * v["zu"][ubm]])
    mu = float(prod.mean())
    sl = np.where(lbm, mu - synth.xl_safe(v["xl"]) * v["zl"], 0.0)
    su = np.where(ubm, mu - synth.xl_safe(v["xu"]) * v["zu"], 0.0)
    r = P["res"]
    return dict(v, state=state, mu=mu, sl=sl, su=su, rb=r["rb"], rc=r["rc"], rl=r["rl"], ru=r["ru"], tied=tied)


def newton_args(nw, residuals=True):
    res = [nw[k] if residuals else None for k in ("rb", "rc", "rl", "ru")]
    return res + [nw[k] for k in ("sl", "su", "xl", "xu", "zl", "zu", "state")]


@pytest.mark.parametrize("name", list(ir.SHAPES))
def test_newton_recovery_from_the_device_step(kkt, phased, name):
    P = model(name)
    A, state = P["A"], P["state"]
    nw = cached(("newton", name), lambda: newton_inputs(P, 0.25))
    for st_ in range(5):
        assert (state[:G] == st_).any() and (state[G:] == st_).any()
    ctx = context(kkt, A)
    assert ctx.kkt_diag_factorize(nw["xl"], nw["xu"], nw["zl"], nw["zu"], nw["mu"]) == 0
    for residuals in (True, False):                                  # False: the corrector's call, the four residuals NULL
        g = ctx.newton_solve(False, *newton_args(nw, residuals), 0.3 * np.sqrt(nw["mu"]), 2000)
        assert g["errflag"] == 0
        print("%s, residuals %s: %d CR iterations" % (name, residuals, g["iter"]))
        rc, rl, ru = (nw[k] if residuals else None for k in ("rc", "rl", "ru"))
        want = ir.newton_recover(A, state, rc, rl, ru, nw["sl"], nw["su"], nw["xl"], nw["xu"], nw["zl"], nw["zu"], g["dx"], g["dy"])
        lower, upper = want["lower"], want["upper"]
        assert lower[nw["tied"]].all() and lower[state == ir.LB].all() and upper[state == ir.UB].all()
        assert lower[state == ir.BOXED].sum() > 10 and upper[state == ir.BOXED].any()
        assert all(mask[:G].any() and mask[G:].any() for mask in (lower, upper))
        for key in ("dxl", "dxu", "dzl", "dzu"):
            assert np.isfinite(g[key]).all(), key
            bad = np.flatnonzero(g[key] != want[key])
            assert bad.size == 0, (key, bad[:5], g[key][bad[:5]], want[key][bad[:5]], state[bad[:5]], lower[bad[:5]])
        # which component took the shifted value, for every variable: the other one still solves its complementarity row
        with np.errstate(invalid="ignore", divide="ignore"):
            plain_l = (nw["sl"] - nw["zl"] * g["dxl"]) / nw["xl"]
            plain_u = (nw["su"] - nw["zu"] * g["dxu"]) / nw["xu"]
        assert np.array_equal(g["dzu"][lower], plain_u[lower]) and np.array_equal(g["dzl"][upper], plain_l[upper])
        nb = state < ir.LB
        assert not any(g[key][nb].any() for key in ("dxl", "dxu", "dzl", "dzu"))
    ctx.close()


def test_newton_solve_vs_oracle_past_the_cap(kkt, oracle, phased):
    """the whole solve on the wide shape against the oracle's at the gate of test_newton_solve_diag (1e-6): the
    right-hand-side kernel, too.  Barrier vectors 10^(U[-1,1]/4), so that the CPU solve is short: 6 CR iterations."""
    P = model("wide")
    A = P["A"]
    nw = cached(("newton", "wide"), lambda: newton_inputs(P, 0.25))
    tol = 0.3 * np.sqrt(nw["mu"])
    ctx = context(kkt, A)
    assert ctx.kkt_diag_factorize(nw["xl"], nw["xu"], nw["zl"], nw["zu"], nw["mu"]) == 0
    g = ctx.newton_solve(False, *newton_args(nw), tol, 500)
    ctx.close()
    k = oracle.kkt_diag(ocsc(A), maxiter=500)
    assert k.factorize(nw["xl"], nw["xu"], nw["zl"], nw["zu"], nw["mu"]) == 0
    o = k.newton_solve(*newton_args(nw), tol)
    print("CR iterations: device %d, oracle %d" % (g["iter"], o["iter"]))
    assert g["errflag"] == o["errflag"] == 0 and abs(g["iter"] - o["iter"]) <= 2 and o["iter"] < 100
    for key in STEP_KEYS:
        assert relerr(g[key], o[key]) < 1e-6, key


# ---- (d) one predictor-corrector step past the cap -------------------------------------------------------------------------
def finite_rel(a, b):
    f = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), f)
    return relerr(a[f], b[f])


def test_ipm_step_vs_oracle_past_the_cap(kkt, oracle, phased):
    """test_ipm_step_vs_oracle's loop on the wide shape, two steps, its gates unchanged: the one way to
    boundary_row_kernel with 1024 partials per problem and to the complementarity kernels of ipm_step.hip at N > G"""
    P = model("wide", fixed=False)
    A, state, m, n = P["A"], P["state"], P["m"], P["n"]
    b, c, it = P["b"], P["c"], P["it"]
    ctx = context(kkt, A)
    k = oracle.kkt_diag(ocsc(A), maxiter=3000)
    kkt_tol = 1e-7
    blocked = 0
    for step in range(2):
        comp = oracle.iterate_complementarity(state, it)
        assert k.factorize(it["xl"], it["xu"], it["zl"], it["zu"], comp["mu"]) == 0
        ctx.iterate_set(it, state)
        assert ctx.iterate_factorize_diag() == 0
        new_o, io = k.ipm_step(state, b, c, P["lbs"], P["ubs"], it, kkt_tol=kkt_tol)
        ig = ctx.ipm_step(False, b, c, P["lbs"], P["ubs"], kkt_tol=kkt_tol, maxiter=3000)
        new_g = ctx.iterate_get()
        print("step %d: CR iterations %d + %d (oracle %d + %d), steps %.6f %.6f" % (
            step, ig["kktiter_predictor"], ig["kktiter_corrector"], io["kktiter_predictor"], io["kktiter_corrector"],
            ig["step_primal"], ig["step_dual"]))
        assert ig["errflag"] == io["errflag"] == 0
        assert abs(ig["kktiter_predictor"] - io["kktiter_predictor"]) <= max(2, 0.02 * io["kktiter_predictor"])
        assert abs(ig["kktiter_corrector"] - io["kktiter_corrector"]) <= max(2, 0.02 * io["kktiter_corrector"])
        for key in ("step_primal", "step_dual", "mu_before", "mu_after", "sigma"):
            assert abs(ig[key] - io[key]) <= 1e-5 * abs(io[key]), (step, key, ig[key], io[key])
        for key in ir.IT_KEYS:
            assert finite_rel(new_g[key], new_o[key]) < 1e-5, (step, key)
        assert 0.0 < ig["step_primal"] < 1.0 and 0.0 < ig["step_dual"] < 1.0
        blocked += ig["step_primal"] < 1.0 - 1e-6 and ig["step_dual"] < 1.0 - 1e-6
        it = new_o
    assert blocked >= 1                                              # a blocking index was selected at all
    ctx.close()
