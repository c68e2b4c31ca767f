"""Pure numpy restatements of the device interior-point layer's vector work (ipx_amd/csrc/iterate.hip, ipm_step.hip,
newton.hip), in the reference's order: no GPU, no oracle.  tests/test_ipm_reference.py pins every function here to the
oracle, which tests/test_oracle_vs_ref.py pins bit for bit to the reference's ipx::Iterate; tests/test_gpu_ipm_vectors.py
holds the kernels to it past one pass of their grid.

Elementwise results are float64 and exact: the library is built with -ffp-contract=off, so a kernel that evaluates the same
expression in the same order gives the same bits.  Sums are taken in np.longdouble (np.sum: pairwise, so the reference's own
error is a few 2^-64 of the sum of magnitudes whatever the length) and come with their terms, for sum_bound.

The grid: every kernel of the layer is a grid-stride loop launched with vec_grid(len) = min(ceil(len / 256), 1024)
workgroups of kBlock = 256 threads, so one pass covers G = 262 144 elements and block b, thread t holds the elements
b * 256 + t + k * G.
"""
import numpy as np

from ipx_amd import synth

LD = np.longdouble
U = 2.0 ** -53
EPS = 2.0 ** -52
KBLOCK, GRID_CAP = 256, 1024
G = KBLOCK * GRID_CAP
BARRIER_MIN = 1e-30                    # Iterate::kBarrierMin, src/iterate.h:204
DAMP = 1.0 - EPS                       # StepToBoundary's damping factor, src/ipm.cc:323
FIXED, FREE, LB, UB, BOXED = range(5)
IT_KEYS = ("x", "xl", "xu", "y", "zl", "zu")
MAX_ROW_LEN = 255                      # kMaxRowLen: longer rows leave the plain row kernels


def has_lb(state):
    return (state == LB) | (state == BOXED)


def has_ub(state):
    return (state == UB) | (state == BOXED)


def vec_grid(length):
    return min(max((int(length) + KBLOCK - 1) // KBLOCK, 1), GRID_CAP)


# ---- the summation bound ------------------------------------------------------------------------------------------------
def sum_bound(terms, per_thread, blocks):
    """Worst-case rounding error of the kernels' summation shape over the given (already rounded) terms.

    A term is added into its thread's accumulator in the grid-stride loop: per_thread additions at the most on that
    path.  block_reduce (device_utils.hpp) then runs the wave butterfly wave_reduce, offsets 32, 16, 8, 4, 2, 1: 6
    additions; lane 0 of each of the kBlock / 64 = 4 waves stores its value and r = scratch[0] + scratch[1] + scratch[2]
    + scratch[3] is 3 more.  The host loops (`for (i = 0; i < g; i++) sum += h[i]` in iterate.hip and ipm_step.hip) fold
    the `blocks` partials one by one: blocks - 1 additions after the first, which enters a zero exactly.  Every term
    therefore passes through at most k = per_thread + 6 + 3 + (blocks - 1) rounded additions, each of relative error
    u = 2^-53 on a partial sum no larger in magnitude than the sum of |terms|, which gives k u sum|terms| to first order.
    No device result enters it."""
    k = per_thread + 6 + 3 + (blocks - 1)
    return LD(k) * LD(U) * np.sum(np.abs(np.asarray(terms, np.float64)).astype(LD))


def ldsum(terms):
    return np.sum(np.asarray(terms, np.float64).astype(LD))


# ---- Iterate::Update, src/iterate.cc:94-139 -------------------------------------------------------------------------------
# (step_primal, step_dual, the directions passed as None): a short step, a long one that runs into the clamp, and the
# two None directions of test_iterate_vs_oracle
UPDATES = ((0.7, 0.4, ()), (3.0, 5.0, ()), (1.0, 1.0, ("dxu", "dzl")))


def update(m, n, state, it, sp, dx, dxl, dxu, sd, dy, dzl, dzu):
    """x += sp dx off the fixed variables, y += sd dy, the four barrier vectors on the variables that have the term and
    clamped at kBarrierMin; a step that is None is skipped"""
    out = {k: np.array(it[k], np.float64, copy=True) for k in IT_KEYS}
    lbm, ubm = has_lb(state), has_ub(state)
    if dx is not None:
        mv = state != FIXED
        out["x"][mv] = (out["x"] + sp * dx)[mv]
    if dy is not None:
        out["y"] = out["y"] + sd * dy
    for key, step, mask, s in (("xl", dxl, lbm, sp), ("xu", dxu, ubm, sp), ("zl", dzl, lbm, sd), ("zu", dzu, ubm, sd)):
        if step is not None:
            out[key][mask] = np.maximum(out[key][mask] + s * step[mask], BARRIER_MIN)
    return out


# ---- Iterate::ComputeResiduals, src/iterate.cc:536-588 --------------------------------------------------------------------
def _fold_rows(nrows, ptr, prod, init, neg):
    """init (-|+) the products of each row, one by one in storage order (adding the 0.0 behind a row's end is exact)"""
    lens = np.diff(ptr)
    width = int(lens.max()) if lens.size else 0
    P = np.zeros((nrows, max(width, 1)))
    P[np.repeat(np.arange(nrows), lens), np.arange(ptr[-1]) - np.repeat(ptr[:-1], lens)] = prod
    acc = np.array(init, np.float64, copy=True)
    for k in range(width):
        acc = acc - P[:, k] if neg else acc + P[:, k]
    return acc


def row_lengths(A):
    """entries per row of A (the rows of Arows) and per column (the rows of Acols)"""
    return np.bincount(A.i, minlength=A.nrow), np.diff(A.p)


def col_dots(A, y):
    """DotColumn(AI, j, y) for the structural columns: sum_p y[Ai[p]] * Ax[p] from 0.0 in storage order"""
    return _fold_rows(A.ncol, A.p, y[A.i] * A.x, np.zeros(A.ncol), False)


def residual_rb(A, b, x):
    """rb = b - AI x as MultiplyAdd('N') leaves it: per row, b_i minus the products x_j a_ij with j ascending, then the
    slack entry"""
    n, m = A.ncol, A.nrow
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.p))
    order = np.argsort(A.i, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(A.i, minlength=m))])
    return _fold_rows(m, ptr, x[cols[order]] * A.x[order], b, True) - x[n:]


def residuals(A, state, b, c, lb, ub, it):
    """rb, rc, rl, ru and the two norms; rc = ((c - zl) + zu) - AI_j'y, 0 on fixed variables"""
    n = A.ncol
    lbm, ubm = has_lb(state), has_ub(state)
    aty = np.concatenate([col_dots(A, it["y"]), it["y"]])
    rc = np.where(state == FIXED, 0.0, ((c - it["zl"]) + it["zu"]) - aty)
    with np.errstate(invalid="ignore"):
        rl = np.where(lbm, lb - it["x"] + it["xl"], 0.0)
        ru = np.where(ubm, ub - it["x"] - it["xu"], 0.0)
    rb = residual_rb(A, b, it["x"])
    return dict(rb=rb, rc=rc, rl=rl, ru=ru, **residual_norms(rb, rc, rl, ru))


def residual_norms(rb, rc, rl, ru):
    amax = lambda v: float(np.abs(v).max()) if v.size else 0.0
    return dict(presidual=max(amax(rb), amax(rl), amax(ru)), dresidual=amax(rc))


# ---- Iterate::ComputeComplementarity, src/iterate.cc:642-670 --------------------------------------------------------------
def complementarity(state, it):
    """the rounded products (lower terms, then upper terms), their long-double sum and mu, min, max and count; without a
    barrier term mu = 0 and min = 0 (:666-669)"""
    lbm, ubm = has_lb(state), has_ub(state)
    prod = np.concatenate([it["xl"][lbm] * it["zl"][lbm], it["xu"][ubm] * it["zu"][ubm]])
    cnt = int(prod.size)
    s = ldsum(prod)
    return dict(products=prod, sum=s, count=cnt, mu=s / cnt if cnt else LD(0), mu_min=float(prod.min()) if cnt else 0.0,
                mu_max=float(prod.max()) if cnt else 0.0)


# ---- Iterate::ComputeObjectives, src/iterate.cc:590-640, not postprocessed ------------------------------------------------
def objectives(A, state, b, c, lb, ub, it):
    """pobj = sum over the variables that are not fixed of c_j x_j, offset = the same over the fixed ones, dobj = b'y +
    sum lb_j zl_j - sum ub_j zu_j - sum over the fixed j of x_j AI_j'y.  Returns the three long-double values and, per
    value, the rounded terms a kernel adds.  The fixed structural terms of dobj are listed apart, as products
    x_j (y_i a_ij): the device sums them through the SpMV's dot, not through the vector kernel."""
    n = A.ncol
    x, y = it["x"], it["y"]
    fx = state == FIXED
    lbm, ubm = has_lb(state), has_ub(state)
    cx = c * x
    fs = np.flatnonzero(fx[n:])
    with np.errstate(invalid="ignore"):
        dterms = np.concatenate([b * y, (lb * it["zl"])[lbm], -(ub * it["zu"])[ubm], -(x[n + fs] * y[fs])])
    cols = np.repeat(np.arange(n), np.diff(A.p))
    sel = fx[cols]
    fixed_prod = (x[cols[sel]].astype(LD) * (y[A.i[sel]].astype(LD) * A.x[sel].astype(LD)))
    dobj = ldsum(dterms) - np.sum(fixed_prod)
    return dict(pobj=ldsum(cx[~fx]), offset=ldsum(cx[fx]), dobj=dobj, pterms=cx[~fx], oterms=cx[fx], dterms=dterms,
                fixed_products=np.asarray(fixed_prod, np.float64), fixed_terms=x[:n][fx[:n]] * col_dots(A, y)[fx[:n]])


# ---- the Newton recovery, src/ipm.cc:577-633 ------------------------------------------------------------------------------
def newton_recover(A, state, rc, rl, ru, sl, su, xl, xu, zl, zu, dx, dy):
    """dxl, dxu, dzl, dzu from a given (dx, dy) -- dy after its sign change -- and `lower`: where dzl is the component
    that takes the shifted value rc + dzu - AI_j'dy (elsewhere on the barrier variables dzu = -rc + dzl + AI_j'dy does).
    lower = zl xu >= zu xl when both bound distances are finite, else whichever is finite; all four are 0 off the barrier
    variables.  rc, rl, ru may be None (the corrector's call)."""
    N = state.size
    zero = np.zeros(N)
    rc, rl, ru = (zero if v is None else v for v in (rc, rl, ru))
    bar = state >= LB
    with np.errstate(invalid="ignore", divide="ignore"):
        dxl = np.where(bar, dx - rl, 0.0)
        dzl = np.where(bar, (sl - zl * dxl) / xl, 0.0)
        dxu = np.where(bar, ru - dx, 0.0)
        dzu = np.where(bar, (su - zu * dxu) / xu, 0.0)
        fl, fu = np.isfinite(xl), np.isfinite(xu)
        lower = bar & np.where(fl & fu, zl * xu >= zu * xl, fl)
    upper = bar & ~lower
    atdy = np.concatenate([col_dots(A, dy), dy])
    dzl = np.where(lower, rc + dzu - atdy, dzl)
    dzu = np.where(upper, -rc + dzl + atdy, dzu)
    return dict(dxl=dxl, dxu=dxu, dzl=dzl, dzu=dzu, lower=lower, upper=upper)


# ---- StepToBoundary, src/ipm.cc:320-339: both rules -----------------------------------------------------------------------
def sequential(x, dx, alpha0=1.0):
    """the reference's scan: for i ascending, if x_i + alpha dx_i < 0 with the RUNNING alpha, alpha = -(x_i damp) / dx_i
    and i blocks.  (Vectorised: the next index that blocks at the current alpha is looked for in chunks.)"""
    x, dx = np.asarray(x, np.float64), np.asarray(dx, np.float64)
    alpha, blk, i, n = float(alpha0), -1, 0, x.size
    chunk = 4096
    while i < n:
        hit = np.flatnonzero(x[i:i + chunk] + alpha * dx[i:i + chunk] < 0.0)
        if hit.size == 0:
            i += chunk
            chunk = min(2 * chunk, 1 << 20)
            continue
        j = i + int(hit[0])
        alpha, blk, i = float(-(x[j] * DAMP) / dx[j]), j, j + 1
    return alpha, blk


def parallel_min(x, dx, alpha0=1.0):
    """the rule of step_to_boundary_kernel and step_to_boundary_dev: the candidates are the elements with
    x_i + alpha0 dx_i < 0 at the FIXED alpha0, cand_i = -(x_i damp) / dx_i; (min cand, smallest index attaining it) if
    that minimum is below alpha0, else (alpha0, -1)"""
    x, dx = np.asarray(x, np.float64), np.asarray(dx, np.float64)
    idx = np.flatnonzero(x + alpha0 * dx < 0.0)
    if idx.size == 0:
        return float(alpha0), -1
    cand = -(x[idx] * DAMP) / dx[idx]
    k = int(np.argmin(cand))                  # the first occurrence of the minimum
    return (float(cand[k]), int(idx[k])) if cand[k] < alpha0 else (float(alpha0), -1)


STEP_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, G - 1, G, G + 1, G + 257, 3 * G + 5)


def random_step(length, seed):
    """x in [0.01, 1], dx normal: about a sixth of the entries are candidates at alpha0 = 1"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.01, 1.0, length), rng.standard_normal(length)


def nonblocking(length, seed):
    """no entry blocks at alpha0 = 1: the steps to the boundary lie in (1.25, inf)"""
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.5, 1.0, length)
    return x, -x * rng.uniform(0.0, 0.8, length)


def step_cases(length):
    """(name, x, dx, alpha0) at one length: the cases on which the two rules agree, so that either serves as reference"""
    L = length
    yield "random", *random_step(L, 100 + L % 1000), 1.0
    yield "nothing blocks", *nonblocking(L, 200), 1.0
    if L > 0:
        x, dx = nonblocking(L, 201)
        x[L - 1], dx[L - 1] = 0.5, -1.0
        yield "only the last index blocks", x, dx, 1.0
    if L > G:
        x, dx = nonblocking(L, 202)
        x[G], dx[G] = 0.5, -1.0
        yield "only index G blocks", x, dx, 1.0
    # would-be blockers between 0.5 and 1 with alpha0 = 0.5: ignored
    x, dx = nonblocking(L, 203)
    rng = np.random.default_rng(204)
    w = rng.random(L) < 0.1
    dx[w] = -x[w] / rng.uniform(0.55, 0.95, int(w.sum()))
    yield "alpha0 = 0.5, steps in (0.5, 1)", x, dx, 0.5
    if L >= 3:
        x, dx = random_step(L, 205)
        at = sorted({L - 1, L // 2, L // 3})
        x[at], dx[at] = 0.0, -1.0
        yield "x = 0 at several indices", x, dx, 1.0


def exact_ties(length=3 * G + 5):
    """(name, x, dx, the index that must be returned): two identical (x, dx) pairs that block first, among entries that
    do not block or block later, for every place where the smallest-index rule is applied"""
    b = 517
    pairs = [("one thread, two passes", 77, 77 + G),
             ("two lanes of one wave", b * KBLOCK + 5, b * KBLOCK + 41),
             ("two waves of one block", b * KBLOCK + 5, b * KBLOCK + 64 + 5),
             ("blocks b and b + 1", b * KBLOCK + 200, (b + 1) * KBLOCK + 3),
             ("blocks b and b + 64", b * KBLOCK + 200, (b + 64) * KBLOCK + 3),
             ("pass 2 in a lower thread than pass 1", 10, G + 3),
             ("pass 2 in a lower block than pass 1", 300, G + 3),
             ("passes 2 and 3, the later pass in the lower block", 2 * G + 3, G + 5 * KBLOCK + 9)]
    out = []
    for k, (name, i, j) in enumerate(pairs):
        x, dx = nonblocking(length, 900 + k)
        later = np.random.default_rng(950 + k).choice(length, 2000, replace=False)
        dx[later] = -x[later] * 1.5                                   # these block at 2/3 (damped)
        x[[i, j]], dx[[i, j]] = 0.75, -1.5                            # the pair blocks at 1/2 (damped)
        out.append((name, x, dx, min(i, j)))
    return out


def near_tie_family(length, seed):
    """Scaled copies x = s x0, dx = -s d0 of one pair, s spanning 40 binades, so that the candidates -(x damp) / dx agree
    to an ulp or two without being equal; a third of the entries are replaced by unrelated ones (x in [0.01, 1], a step that
    moves away from the bound or reaches it later than the family), and alpha0 is 1 or lies within 3 ulp of x0 / d0.
    Returns x, dx, alpha0."""
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(0.1, 1.0)
    d0 = x0 / rng.uniform(0.2, 0.9)
    s = 2.0 ** rng.uniform(-20.0, 20.0, length)
    x, dx = s * x0, -(s * d0)
    other = rng.random(length) < 1.0 / 3.0
    k = int(other.sum())
    x[other] = rng.uniform(0.01, 1.0, k)
    # half of them move away from the bound; the others reach it later than the family does, before or after alpha0 = 1
    dx[other] = np.where(rng.random(k) < 0.5, rng.uniform(0.0, 2.0, k), -x[other] / (x0 / d0 * rng.uniform(1.001, 4.0, k)))
    alpha0 = 1.0
    if rng.random() < 0.5:
        alpha0 = float(x0 / d0)
        k = int(rng.integers(-3, 4))
        for _ in range(abs(k)):
            alpha0 = float(np.nextafter(alpha0, np.inf if k > 0 else -np.inf))
    return x, dx, alpha0


# the window between the two rules over near_tie_family(5000, seed), seed in WINDOW_SEEDS, as
# tests/test_ipm_reference.py::test_the_window_between_the_two_step_rules measured it (CPU against CPU): the largest
# |alpha_sequential - alpha_parallel_min| / alpha_parallel_min in units of eps = 2^-52, and the share of seeds in which the
# blocking index differs
WINDOW_SEEDS = range(4000)
NEAR_TIE_DEVICE_CASES = [(5000, s) for s in range(8)] + [(G + 257, 8), (3 * G + 5, 9)]      # (length, seed) on the device
MEASURED_WINDOW_EPS = 1.9475           # measured 1.94741...; on random_step data the two rules never differ
MEASURED_INDEX_SHARE = 0.6985


# ---- the two shapes -----------------------------------------------------------------------------------------------------
SHAPES = {"wide": dict(m=8192, n=G + 257 - 8192, k=3, seed=811),      # N = G + 257: pass 2 = one full block + 1 element
          "tall": dict(m=G + 257, n=512, k=8, seed=812)}              # m > G: everything guarded by j < m, the m-loops
EDGES = lambda N: (0, 255, 256, G - 1, G, N - 1)


def shape_model(name, fixed=True):
    """synth.synthetic_iterate on a matrix with k entries per column (no row longer than kMaxRowLen), with
      * the variables at EDGES(N) and five more per pass boxed (where the tests plant residuals, products and ties),
      * free, lb, ub and boxed variables in both passes,
      * about 1 % of the variables fixed (state 0; xl = xu = inf, zl = zu = 0 as test_iterate_objectives_vs_oracle sets
        them), over structural and slack columns and both passes -- unless fixed is False.
    Returns synthetic_iterate's dict with b, c (cost incl. slacks), N, edges, boxed (the planted boxed indices) added."""
    S = SHAPES[name]
    m, n = S["m"], S["n"]
    N = n + m
    P = _iterate_on(synth.synthetic_lp(m, n, S["k"], S["seed"]), S["seed"])
    rng = np.random.default_rng(S["seed"] + 1)
    edges = EDGES(N)
    boxed = np.array(sorted(set(edges) | {1000 + 37 * k for k in range(5)} | {G + 11 + 47 * k for k in range(5)}))
    free2 = np.array([G + 2, G + 100])                                 # free variables in pass 2 (slack columns)
    pos = lambda q: 10.0 ** rng.uniform(-1, 1, q)
    state, it = P["state"], P["it"]
    for idx, st_ in ((boxed, BOXED), (free2, FREE)):
        state[idx] = st_
        lo, up = st_ == BOXED, st_ == BOXED
        P["lbs"][idx] = -rng.uniform(0.5, 2.0, idx.size) if lo else -np.inf
        P["ubs"][idx] = rng.uniform(1.0, 3.0, idx.size) if up else np.inf
        it["xl"][idx], it["zl"][idx] = (pos(idx.size), pos(idx.size)) if lo else (np.inf, 0.0)
        it["xu"][idx], it["zu"][idx] = (pos(idx.size), pos(idx.size)) if up else (np.inf, 0.0)
    if fixed:
        keep = np.ones(N, bool)
        keep[boxed] = keep[free2] = False
        cand = np.flatnonzero(keep)
        assert n < G                                                   # the second pass holds slack columns only
        fx = np.concatenate([rng.choice(cand[cand < n], max(n // 100, 8), replace=False),
                             rng.choice(cand[(cand >= n) & (cand < G)], max(m // 100, 8), replace=False),
                             rng.choice(cand[cand >= G], 12, replace=False)])
        state[fx] = FIXED
        for k in ("xl", "xu"):
            it[k][fx] = np.inf
        for k in ("zl", "zu"):
            it[k][fx] = 0.0
    P.update(b=P["rhs"], c=np.concatenate([P["obj"], np.zeros(m)]), N=N, m=m, n=n, edges=edges, boxed=boxed)
    return P


def _iterate_on(A, seed):
    """synth.synthetic_iterate's iterate, bounds and step for a given matrix (its own has 8 entries per column)"""
    m, n = A.nrow, A.ncol
    rng = np.random.default_rng(seed)
    N = n + m
    lb, ub = np.zeros(n), np.full(n, np.inf)
    k = int(0.15 * n)
    sp = rng.permutation(n)[:3 * k]
    lb[sp[:k]] = -np.inf; ub[sp[:k]] = rng.uniform(1, 3, k)
    lb[sp[k:2 * k]] = rng.uniform(-2, 0, k); ub[sp[k:2 * k]] = rng.uniform(1, 3, k)
    lb[sp[2 * k:]] = -np.inf
    ct = rng.choice(list("<>="), size=m, p=[0.6, 0.25, 0.15])
    lbs = np.concatenate([lb, np.where(ct == ">", -np.inf, 0.0)])
    ubs = np.concatenate([ub, np.where(ct == "<", np.inf, 0.0)])
    fl, fu = np.isfinite(lbs), np.isfinite(ubs)
    state = np.where(fl & fu, BOXED, np.where(fl, LB, np.where(fu, UB, FREE))).astype(np.uint8)
    pos = lambda: 10.0 ** rng.uniform(-1, 1, N)
    it = dict(x=rng.uniform(-1, 1, N), y=rng.uniform(-1, 1, m), xl=np.where(fl, pos(), np.inf), zl=np.where(fl, pos(), 0.0),
              xu=np.where(fu, pos(), np.inf), zu=np.where(fu, pos(), 0.0))
    Ur = lambda q: rng.uniform(-1, 1, q)
    step = dict(dx=Ur(N), dxl=Ur(N), dxu=Ur(N), dy=Ur(m), dzl=Ur(N), dzu=Ur(N))
    return dict(A=A, rhs=rng.uniform(-1, 1, m), obj=rng.uniform(-1, 1, n), lbs=lbs, ubs=ubs, state=state, it=it, step=step)
