"""Crossover in solver form (reference src/crossover.cc, src/basis.cc:324-351, src/lp_solver.cc:464-537, src/utils.cc:87-104)
restated in dense NumPy: PushDual, PushPrimal, both ratio tests -- each as the reference's sequential loop in index order AND in
the order-free form crossover.hip computes --, ComputeBasicSolution, PushAll's screening and Sortperm's order; planted inputs on
which every outcome of a push occurs; exact dyadic cases for the two ratio tests.  NumPy only.

The restatement runs in any float type (float64, longdouble): the basis inverse is kept explicitly (Gauss-Jordan, then the
product-form update of an exchange, from scratch every 32 exchanges), and every exchange is asserted to be one the basis accepts
at once: the pivot from the dense FTRAN and the pivot from the dense BTRAN agree to 1e-10."""
import numpy as np

from basis_ties_reference import G, G_ROW, K_BLOCK, K_ROW_LANES, ROW_COLS, placements
from drop_reference import Margin, csc, dense_AI

PIVOT_ZERO_TOL = 1e-5                       # src/crossover.h:137
FEASTOL = 1e-7
IPX_BASIC, IPX_NONBASIC_LB, IPX_NONBASIC_UB, IPX_SUPERBASIC = 0, -1, -2, -3
STATUS_OPTIMAL, STATUS_IMPRECISE, STATUS_TIME_LIMIT, STATUS_FAILED = 1, 2, 5, 8


class ArgumentError(ValueError):
    """the reference's std::logic_error"""


# ---- the ratio tests ---------------------------------------------------------------------------------------------------------
def dual_ratio_sequential(z, row, restrict, step, feastol):
    """Crossover::DualRatioTest (:418-465) as written: (jblock, step after the first pass)"""
    jblock = -1
    for j in np.nonzero(row)[0]:
        pivot = row[j]
        if abs(pivot) > PIVOT_ZERO_TOL:
            if (restrict[j] & 1) and z[j] - step * pivot < -feastol:
                step, jblock = (z[j] + feastol) / pivot, j
            if (restrict[j] & 2) and z[j] - step * pivot > feastol:
                step, jblock = (z[j] - feastol) / pivot, j
    if jblock < 0:
        return -1, step
    jblock, max_pivot = -1, PIVOT_ZERO_TOL
    for j in np.nonzero(row)[0]:
        pivot = row[j]
        if abs(pivot) > max_pivot and abs(z[j] / pivot) <= abs(step):
            if (restrict[j] & 1) and step * pivot > 0.0:
                jblock, max_pivot = j, abs(pivot)
            if (restrict[j] & 2) and step * pivot < 0.0:
                jblock, max_pivot = j, abs(pivot)
    assert jblock >= 0
    return int(jblock), step


def _least(ratios, idx, M):
    """the ratio of least magnitude, the lowest index among equals; the margin to the runner-up"""
    a = np.abs(ratios)
    k = int(np.argmin(a))                                           # (the first of equals)
    if M is not None and len(a) > 1:
        M.cmp(a[k], np.delete(a, k).min())
    return ratios[k], int(idx[k])


def _largest(a, idx, M):
    k = int(np.argmax(a))
    if M is not None and len(a) > 1:
        M.cmp(a[k], np.delete(a, k).max())
    return int(idx[k])


def dual_ratio_free(z, row, restrict, step0, feastol, M=None, Mp=None):
    """the order-free form: among |row_j| > 1e-5 the entries that block at the FULL step, the ratio of least magnitude; then
    the second pass as an arg max of |row_j| with ties to the lowest j"""
    with np.errstate(divide="ignore", invalid="ignore"):
        big = np.abs(row) > PIVOT_ZERO_TOL
        t = z - step0 * row
        lo = big & ((restrict & 1) != 0) & (t < -feastol)
        hi = big & ((restrict & 2) != 0) & (t > feastol) & ~lo
        ratio = np.where(lo, (z + feastol) / row, (z - feastol) / row)
        cand = np.nonzero(lo | hi)[0]
        if len(cand) == 0:
            return -1, step0
        step, _ = _least(ratio[cand], cand, M)
        sr = step * row
        ok = big & (np.abs(z / row) <= abs(step)) & ((((restrict & 1) != 0) & (sr > 0)) | (((restrict & 2) != 0) & (sr < 0)))
    cand = np.nonzero(ok)[0]
    assert len(cand) > 0
    return _largest(np.abs(row[cand]), cand, Mp), step


def primal_ratio_sequential(xb, ftran, lbb, ubb, step, feastol):
    """Crossover::PrimalRatioTest (:359-416) as written: (pblock, block_at_lb, step after the first pass)"""
    pblock, at_lb = -1, True
    for p in np.nonzero(ftran)[0]:
        pivot = ftran[p]
        if abs(pivot) > PIVOT_ZERO_TOL:
            if xb[p] + step * pivot < lbb[p] - feastol:
                step, pblock, at_lb = (lbb[p] - xb[p] - feastol) / pivot, p, True
            if xb[p] + step * pivot > ubb[p] + feastol:
                step, pblock, at_lb = (ubb[p] - xb[p] + feastol) / pivot, p, False
    if pblock < 0:
        return -1, True, step
    pblock, max_pivot = -1, PIVOT_ZERO_TOL
    for p in np.nonzero(ftran)[0]:
        pivot = ftran[p]
        if abs(pivot) > max_pivot:
            if step * pivot < 0.0 and abs((lbb[p] - xb[p]) / pivot) <= abs(step):
                pblock, at_lb, max_pivot = p, True, abs(pivot)
            if step * pivot > 0.0 and abs((ubb[p] - xb[p]) / pivot) <= abs(step):
                pblock, at_lb, max_pivot = p, False, abs(pivot)
    assert pblock >= 0
    return int(pblock), at_lb, step


def primal_ratio_free(xb, ftran, lbb, ubb, step0, feastol, M=None, Mp=None):
    with np.errstate(divide="ignore", invalid="ignore"):
        big = np.abs(ftran) > PIVOT_ZERO_TOL
        t = xb + step0 * ftran
        lo = big & (t < lbb - feastol)
        hi = big & (t > ubb + feastol) & ~lo
        ratio = np.where(lo, (lbb - xb - feastol) / ftran, (ubb - xb + feastol) / ftran)
        cand = np.nonzero(lo | hi)[0]
        if len(cand) == 0:
            return -1, True, step0
        step, _ = _least(ratio[cand], cand, M)
        sp = step * ftran
        ok = big & (((sp < 0) & (np.abs((lbb - xb) / ftran) <= abs(step))) | ((sp > 0) & (np.abs((ubb - xb) / ftran) <= abs(step))))
    cand = np.nonzero(ok)[0]
    assert len(cand) > 0
    p = _largest(np.abs(ftran[cand]), cand, Mp)
    return p, bool(step * ftran[p] < 0), step


# ---- the basis: an explicit inverse in the float type of the run ---------------------------------------------------------------
def inverse(B):
    """Gauss-Jordan with partial pivoting, in B's own float type"""
    m = len(B)
    A = np.concatenate([B, np.eye(m, dtype=B.dtype)], axis=1)
    for k in range(m):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
        A[k] = A[k] / A[k, k]
        col = A[:, k].copy()
        col[k] = 0
        A -= np.outer(col, A[k])
    return A[:, m:]


class DenseBasis:
    def __init__(self, AI, basis):
        self.AI, self.basis = AI, np.array(basis, np.int64)
        self.m, self.N = AI.shape
        self.pos = np.full(self.N, -1, np.int64)
        self.pos[self.basis] = np.arange(self.m)
        self.inv = inverse(AI[:, self.basis])
        self.exchanges = 0

    def btran(self, p):
        return self.inv[p].copy()

    def ftran(self, j):
        return self.inv @ self.AI[:, j]

    def row(self, btran):
        r = self.AI.T @ btran
        r[self.basis] = 0
        return r

    def exchange(self, p, jn, pivot_col, pivot_row):
        """Basis::ExchangeIfStable: both pivots agree (the restatement cannot follow a refused exchange)"""
        assert pivot_col != 0 and abs(pivot_col - pivot_row) <= 1e-10 * abs(pivot_col), "an exchange the restatement cannot follow"
        jb = self.basis[p]
        self.basis[p] = jn
        self.pos[jn], self.pos[jb] = p, -1
        self.exchanges += 1
        if self.exchanges % 32 == 0:
            self.inv = inverse(self.AI[:, self.basis])               # from scratch now and then: no drift
        else:                                                        # the product-form update of the inverse
            u = self.inv @ self.AI[:, jn]
            rowp = self.inv[p] / u[p]
            u[p] = 0
            self.inv -= np.outer(u, rowp)
            self.inv[p] = rowp


class Outcomes:
    """which outcomes of a push have occurred, and the smallest margins of the ratio tests"""
    def __init__(self):
        self.seen = set()
        self.ratio, self.pivot = Margin(), Margin()


def _both_dual(z, row, restrict, step0, feastol, out):
    jn, step = dual_ratio_free(z, row, restrict, step0, feastol, out.ratio if out else None, out.pivot if out else None)
    js, ss = dual_ratio_sequential(z, row, restrict, step0, feastol)
    assert jn == js and np.array(step).tobytes() == np.array(ss).tobytes(), ("dual ratio test: the two forms differ", jn, js, step, ss)
    return jn, step


def _both_primal(xb, ftran, lbb, ubb, step0, feastol, out):
    p, at_lb, step = primal_ratio_free(xb, ftran, lbb, ubb, step0, feastol, out.ratio if out else None, out.pivot if out else None)
    ps, als, ss = primal_ratio_sequential(xb, ftran, lbb, ubb, step0, feastol)
    assert p == ps and (p < 0 or at_lb == als) and np.array(step).tobytes() == np.array(ss).tobytes(), \
        ("primal ratio test: the two forms differ", p, ps, step, ss)
    return p, at_lb, step


# ---- the push phases ---------------------------------------------------------------------------------------------------------
def push_dual(B, lb, ub, x, y, z, variables, feastol=FEASTOL, out=None, stop_at=None):
    """Crossover::PushDual (:229-357) on the DenseBasis B; y, z are updated in place.  stop_at: the interrupt returns 999 at
    its stop_at-th poll.  Returns dict(status, pushes, pivots, log)."""
    N = B.N
    for j in variables:
        if B.pos[j] < 0:
            raise ArgumentError("invalid variable in PushDual")
    restrict = (x != ub).astype(np.int64) | ((x != lb).astype(np.int64) << 1)
    if ((((restrict & 1) != 0) & (z < 0)) | (((restrict & 2) != 0) & (z > 0))).any():
        raise ArgumentError("sign condition violated in PushDual")
    log, pushes, polls, status = [], 0, 0, STATUS_OPTIMAL
    for jb in variables:
        polls += 1
        if stop_at is not None and polls >= stop_at:
            status = STATUS_TIME_LIMIT
            break
        if z[jb] == 0:
            continue
        p = B.pos[jb]
        btran = B.btran(p)
        row = B.row(btran)
        step = z[jb]
        jn, _ = _both_dual(z, row, restrict, step, feastol, out)
        if jn >= 0:
            B.exchange(p, jn, B.ftran(jn)[p], row[jn])
            step = z[jn] / row[jn]
            log.append((int(jb), int(jn)))
        if out is not None:
            out.seen.add("dual_blocked" if jn >= 0 else "dual_free")
        if step != 0:
            y += step * btran
            nz = row != 0
            znew = z - step * row
            znew = np.where((restrict & 1) != 0, np.maximum(znew, 0), znew)
            znew = np.where((restrict & 2) != 0, np.minimum(znew, 0), znew)
            z[nz] = znew[nz]
            z[jb] -= step
        if jn >= 0:
            z[jn] = 0
        else:
            assert z[jb] == 0
        pushes += 1
    return dict(status=status, pushes=pushes, pivots=len(log), log=log)


def push_primal(B, lb, ub, x, variables, fixed_at_bound=None, feastol=FEASTOL, out=None, stop_at=None):
    """Crossover::PushPrimal (:73-220); x is updated in place"""
    for j in variables:
        if B.pos[j] >= 0:
            raise ArgumentError("invalid variable in PushPrimal")
    if ((x < lb) | (x > ub)).any():
        raise ArgumentError("bound condition violated in PushPrimal")
    if fixed_at_bound is not None and (fixed_at_bound.astype(bool) & (x != lb) & (x != ub)).any():
        raise ArgumentError("bound condition violated in PushPrimal")
    xb, lbb, ubb = x[B.basis].copy(), lb[B.basis].copy(), ub[B.basis].copy()
    if fixed_at_bound is not None:
        f = fixed_at_bound.astype(bool)[B.basis]
        lbb[f] = xb[f]
        ubb[f] = xb[f]
    log, pushes, polls, status = [], 0, 0, STATUS_OPTIMAL
    for jn in variables:
        polls += 1
        if stop_at is not None and polls >= stop_at:
            status = STATUS_TIME_LIMIT
            break
        if x[jn] == lb[jn] or x[jn] == ub[jn] or (x[jn] == 0 and np.isinf(lb[jn]) and np.isinf(ub[jn])):
            continue
        boxed = np.isfinite(lb[jn]) and np.isfinite(ub[jn])
        move_to = x.dtype.type(0)
        if boxed:
            move_to = lb[jn] if x[jn] - lb[jn] <= ub[jn] - x[jn] else ub[jn]
        elif np.isfinite(lb[jn]):
            move_to = lb[jn]
        elif np.isfinite(ub[jn]):
            move_to = ub[jn]
        step = x[jn] - move_to
        ftran = B.ftran(jn)
        p, at_lb, _ = _both_primal(xb, ftran, lbb, ubb, step, feastol, out)
        jb = -1
        if p >= 0:
            jb = int(B.basis[p])
            B.exchange(p, jn, ftran[p], B.AI[:, jn] @ B.btran(p))
            step = ((lbb[p] if at_lb else ubb[p]) - xb[p]) / ftran[p]
            log.append((jb, int(jn)))
        if out is not None:
            out.seen.add(("primal_lb" if at_lb else "primal_ub") if p >= 0 else "primal_free")
            if p >= 0 and step == 0 and fixed_at_bound is not None:
                out.seen.add("fixed_step_zero")
            if p < 0:
                out.seen.add("boxed_to_bound" if boxed else "free_to_zero" if not (np.isfinite(lb[jn]) or np.isfinite(ub[jn])) else "onesided")
        if step != 0:
            nz = ftran != 0
            xnew = np.minimum(np.maximum(xb + step * ftran, lbb), ubb)
            xb[nz] = xnew[nz]
            x[jn] -= step
        if p >= 0:
            x[jb] = lbb[p] if at_lb else ubb[p]
            xb[p], lbb[p], ubb[p] = x[jn], lb[jn], ub[jn]
        else:
            x[jn] = move_to
        pushes += 1
    x[B.basis] = xb
    return dict(status=status, pushes=pushes, pivots=len(log), log=log)


def basic_solution(B, b, c, x, y, z):
    """Basis::ComputeBasicSolution (:324-351): x_B, y, z_N in place; x_N, z_B as given"""
    nonbasic = B.pos < 0
    rhs = b - B.AI[:, nonbasic] @ x[nonbasic]
    x[B.basis] = B.inv @ rhs
    y[:] = B.inv.T @ (c[B.basis] - z[B.basis])
    z[nonbasic] = (c - B.AI.T @ y)[nonbasic]


def sortperm(weights):
    """Sortperm (src/utils.cc:87-104) with reverse = false: ascending by (weight, index)"""
    return np.lexsort((np.arange(len(weights)), weights))


def superbasics(B, lb, ub, x, z, perm):
    """PushAll's two screenings (:34-56); the primal one is to be called after the dual phase"""
    dual = [int(j) for j in perm if B.pos[j] >= 0 and z[j] != 0]
    primal = [int(j) for j in perm[::-1]
              if B.pos[j] < 0 and x[j] != lb[j] and x[j] != ub[j] and not (np.isinf(lb[j]) and np.isinf(ub[j]) and x[j] == 0)]
    return dual, primal


def basic_statuses(B, lb, ub, x, z):
    """src/lp_solver.cc:499-512"""
    st = np.full(B.N, IPX_SUPERBASIC, np.int64)
    st[x == ub] = IPX_NONBASIC_UB
    st[x == lb] = IPX_NONBASIC_LB
    eq = lb == ub
    st[eq] = np.where(z[eq] >= 0, IPX_NONBASIC_LB, IPX_NONBASIC_UB)
    st[B.basis] = IPX_BASIC
    return st


def primal_infeasibility(lb, ub, x):
    return max(0.0, float(np.max(lb - x)), float(np.max(x - ub)))


def dual_infeasibility(lb, ub, x, z):
    return max(0.0, float(np.max(np.where(x > lb, z, 0.0))), float(np.max(np.where(x < ub, -z, 0.0))))


def push_all(P, weights, L=np.float64, out=None, basic=True):
    """Crossover::PushAll (:15-71) and, with basic, the basic solution on the planted input P in the float type L.  Returns
    the vertex, the basis, both logs and the counts."""
    AI = dense_AI(P).astype(L)
    lb, ub, b, c = (P[k].astype(L) for k in ("lb", "ub", "b", "c"))
    x, y, z = (P[k].astype(L) for k in ("x", "y", "z"))
    B = DenseBasis(AI, P["basis"])
    perm = sortperm(weights)
    dual, _ = superbasics(B, lb, ub, x, z, perm)
    d = push_dual(B, lb, ub, x, y, z, dual, out=out)
    _, primal = superbasics(B, lb, ub, x, z, perm)
    p = push_primal(B, lb, ub, x, primal, out=out)
    if basic:
        basic_solution(B, b, c, x, y, z)
    return dict(x=x, y=y, z=z, basis=B.basis.copy(), dual=d, primal=p, dual_superbasics=dual, primal_superbasics=primal,
                log=d["log"] + p["log"], statuses=basic_statuses(B, lb, ub, x, z))


# ---- planted inputs ----------------------------------------------------------------------------------------------------------
def planted_point(m, n, seed):
    """A basis with m // 3 structural columns (each dominant in its own row: well conditioned), a complementary point with dual
    superbasics (basic, at a bound, z != 0) and primal superbasics (nonbasic, off its bounds, z = 0), lower-bounded, boxed and
    free variables, and b = AI x, c = AI'y + z.  Planted so that every outcome occurs:
      quiet rows   slack basic with z != 0, no basic structural entry, nonbasic entries only from `tame` columns with z = 5: the
                   tableau row is the raw row and nothing blocks the dual push;
      quiet cols   nonbasic superbasic columns supported in `roomy` rows only (slack basic at x = 5 of [0, inf)): the tableau
                   column is the raw column and nothing blocks the primal push -- one boxed near lb, one boxed near ub, one
                   free, one lower-bounded."""
    rng = np.random.default_rng(seed)
    N = n + m
    k = m // 3
    rows = rng.permutation(m)
    piv_rows, quiet_rows, roomy_rows, other_rows = rows[:k], rows[k:k + 3], rows[k + 3:k + 9], rows[k + 9:]
    cols = rng.permutation(n)
    basic_cols, quiet_cols, tame_cols, normal = cols[:k], cols[k:k + 4], cols[k + 4:k + 8], cols[k + 8:]
    loud = np.setdiff1d(np.arange(m), quiet_rows)
    R, Cc, V = [], [], []

    def add(rr, j, vv):
        R.extend(int(r) for r in rr); Cc.extend([int(j)] * len(rr)); V.extend(float(v) for v in vv)

    def vals(cnt):
        return rng.choice([-1.0, 1.0], cnt) * rng.uniform(0.5, 2.0, cnt)

    for t, j in enumerate(basic_cols):
        rr = rng.choice(np.setdiff1d(loud, [piv_rows[t]]), 3, replace=False)
        add([piv_rows[t]], j, [8.0 * rng.choice([-1.0, 1.0])])
        add(rr, j, vals(3))
    for j in normal:
        add(rng.choice(loud, 4, replace=False), j, vals(4))
    for t, j in enumerate(tame_cols):
        add([quiet_rows[t % 3], quiet_rows[(t + 1) % 3]], j, vals(2))
        add(rng.choice(other_rows, 2, replace=False), j, vals(2))
    for j in quiet_cols:
        add(rng.choice(roomy_rows, 3, replace=False), j, vals(3))
    Ap, Ai, Ax = csc(m, n, R, Cc, V)
    basis = n + np.arange(m)
    basis[piv_rows] = basic_cols
    isbasic = np.zeros(N, bool)
    isbasic[basis] = True

    kind = rng.choice(3, N, p=[0.55, 0.30, 0.15])                    # 0: [0, inf), 1: [0, 10], 2: free
    kind[n:] = rng.choice(2, m, p=[0.8, 0.2])                       # slacks: lower-bounded or boxed
    kind[tame_cols] = 0
    kind[n + roomy_rows] = 0
    kind[n + quiet_rows] = [0, 1, 0]
    kind[quiet_cols] = [1, 1, 2, 0]
    lb = np.where(kind == 2, -np.inf, 0.0)
    ub = np.where(kind == 0, np.inf, np.where(kind == 1, 10.0, np.inf))
    x, z = np.zeros(N), np.zeros(N)
    u = rng.random(N)
    at_ub = (kind == 1) & (rng.random(N) < 0.5)
    for j in range(N):
        if kind[j] == 2:
            x[j] = rng.uniform(-2.0, 2.0) if (isbasic[j] or u[j] < 0.7) else 0.0
            continue
        if isbasic[j]:
            if u[j] < 0.3:                                          # dual superbasic
                x[j], z[j] = (ub[j], -rng.uniform(0.5, 2.0)) if at_ub[j] else (lb[j], rng.uniform(0.5, 2.0))
            else:
                d = rng.uniform(0.05, 2.0)
                x[j] = ub[j] - d if at_ub[j] else lb[j] + d
        elif u[j] < 0.25:                                           # primal superbasic
            x[j] = rng.uniform(0.3, 9.7) if kind[j] == 1 else rng.uniform(0.3, 3.0)
        else:
            zz = 0.0 if u[j] > 0.9 else rng.uniform(0.05, 2.0)
            x[j], z[j] = (ub[j], -zz) if at_ub[j] else (lb[j], zz)
    x[tame_cols], z[tame_cols] = 0.0, 5.0
    x[n + roomy_rows], z[n + roomy_rows] = 5.0, 0.0
    x[n + quiet_rows], z[n + quiet_rows] = [0.0, 10.0, 0.0], [rng.uniform(0.5, 2.0), -rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0)]
    x[quiet_cols], z[quiet_cols] = [3.0, 7.5, 1.5, 0.7], 0.0
    y = rng.uniform(-1.0, 1.0, m)
    P = dict(m=m, n=n, Ap=Ap, Ai=Ai, Ax=Ax, lb=lb, ub=ub, x=x, y=y, z=z, basis=basis, quiet_cols=quiet_cols, quiet_rows=quiet_rows)
    AI = dense_AI(P)
    P["b"] = AI @ x
    P["c"] = AI.T @ y + z
    P["weights"] = rng.uniform(0.1, 10.0, N)                        # the order of the pushes: any weights will do
    return P


# ---- exact dyadic cases for the two ratio tests --------------------------------------------------------------------------------
# Slack basis; a candidate's tableau row / column is the raw row / column of A because the candidates' rows hold no entering
# column but their own class's.  Entries +-2^a, z and x multiples of 2^-12 of moderate size, feastol = 2^-20: every quotient,
# sum and product the tests compare is exact, so any order of evaluation gives the same bits.
DYADIC_FEASTOL = 2.0 ** -20
DUAL_SHAPE = (300, 3 * G_ROW + 900)         # n + m past three passes of cross_row_kernel (G_ROW columns each)
PRIMAL_SHAPE = (G + 257, 1500)              # m past one pass of the kernels over the positions (G each)
TIE_KINDS = ("lanes", "waves", "blocks", "later_pass", "same_thread")
RATIO = 2.0 ** -3                           # the ratio every blocking member of a class has


def dual_ratio_case(seed):
    """DualRatioTest.  One dual superbasic slack per class (x = lb = 0, z = 1: step0 = 1), its row holding the class members:
    nonbasic at lb with z_j >= 0 (bit 1, row_j > 0) or at ub with z_j <= 0 (bit 2, row_j < 0), each with the ratio
    (z_j +- feastol) / row_j = 2^-3 exactly.
      tie kinds    (placements: lanes / waves / blocks / later_pass / same_thread) equal ratios AND equal |row_j|, mixed signs:
                   the lowest index wins the second pass;
      strict       equal ratios, the HIGHER index holds the strictly larger |row_j|: it wins the second pass;
      pivot_zero   |row_j| = 1e-5 exactly at an entry with z_j = 0, which would block with the least ratio: not a candidate;
      within_tol   the row's only entry has z_j - step0 row_j = -feastol exactly: it must not block, the push takes the full step;
      basic_decoy  the row's largest entry belongs to a BASIC structural column (it stands at the position of the slack of a row
                   nobody else touches), which would block with the least ratio: no candidate.
    Candidates are pushed in ascending order of the row.  Expected: the pivot log and, per class, the step of the update (it
    can be read off y, which starts at 0: y_i = step)."""
    m, n = DUAL_SHAPE
    rng = np.random.default_rng(seed)
    ft = DYADIC_FEASTOL
    sets = placements(K_ROW_LANES, ROW_COLS, G_ROW, n, b=3)
    assert set(TIE_KINDS) < set(sets) and "strict" in sets
    sets["pivot_zero"] = [ROW_COLS * 52 + 1, ROW_COLS * 52 + 9]
    sets["within_tol"] = [ROW_COLS * 54 + 3]
    sets["basic_decoy"] = [ROW_COLS * 56 + 1, ROW_COLS * 56 + 9]
    used = sorted(j for v in sets.values() for j in v)
    assert len(set(used)) == len(used) and max(used) < n
    cand_rows = np.linspace(5, m - 40, len(sets)).astype(int)
    assert len(set(cand_rows)) == len(sets)
    decoy, decoy_row = sets["basic_decoy"][0], m - 3                 # the decoy column stands at the position of slack decoy_row
    filler = np.setdiff1d(np.arange(m - 20), cand_rows)
    N = n + m
    lb, ub, x, z = np.zeros(N), np.full(N, np.inf), np.zeros(N), np.zeros(N)
    z[:n] = 8.0                                                      # background: at lb, far from blocking
    R, Cc, V = [], [], []
    classes, log = [], []
    for (kind, members), i in zip(sets.items(), cand_rows):
        k = len(members)
        r = np.full(k, 0.5)
        win = members[0]
        if kind == "strict":
            r, win = np.array([0.5, 1.0]), members[1]
        zz = r * RATIO - ft                                          # (zz + ft) / r = 2^-3
        if kind in TIE_KINDS:                                        # the second member sits at its upper bound: bit 2
            j = members[1]
            r[1], zz[1] = -r[1], -zz[1]
            ub[j], x[j] = 1.0, 1.0
        elif kind == "pivot_zero":
            r, zz, win = np.array([1e-5, 0.5]), np.array([0.0, 0.5 * RATIO - ft]), members[1]
        elif kind == "within_tol":
            r, zz, win = np.array([2.0]), np.array([2.0 - ft]), -1
        elif kind == "basic_decoy":
            r, zz, win = np.array([4.0, 0.5]), np.array([0.0, 0.5 * RATIO - ft]), members[1]
        R += [int(i)] * k; Cc += list(members); V += list(r)
        z[list(members)] = zz
        step = 1.0 if win < 0 else float(zz[members.index(win)] / r[members.index(win)])
        classes.append(dict(kind=kind, row=int(i), cols=list(members), r=r, z=zz, winner=int(win), step=step))
        if win >= 0:
            log.append((n + int(i), int(win)))
    R.append(decoy_row); Cc.append(decoy); V.append(1.0)
    bg = np.setdiff1d(np.arange(n), used)
    R += list(filler[rng.integers(0, len(filler), len(bg))]); Cc += list(bg); V += list(rng.choice([-1.0, 1.0], len(bg)) * 2.0 ** rng.integers(-2, 3, len(bg)))
    for c in classes:                                                # an entering column also holds an entry in a row that is never pivoted on
        if c["winner"] >= 0:
            R.append(int(filler[rng.integers(0, len(filler))])); Cc.append(c["winner"]); V.append(0.25)
    Ap, Ai, Ax = csc(m, n, R, Cc, V)
    basis = n + np.arange(m)
    basis[decoy_row] = decoy
    x[decoy], z[decoy] = 1.0, 0.0                                    # basic, off its bounds
    z[n + cand_rows] = 1.0
    z[n + decoy_row] = 8.0                                           # nonbasic at lb; its row entry is -4
    # the two forms of the test on every class's raw row agree with the expectation
    for c in classes:
        row, restrict = np.zeros(N), (x != ub).astype(np.int64) | ((x != lb).astype(np.int64) << 1)
        row[c["cols"]] = c["r"]
        row[decoy] = 0.0
        for form in (dual_ratio_free, dual_ratio_sequential):
            jn, _ = form(z, row, restrict, 1.0, ft)
            assert jn == c["winner"], (c["kind"], form.__name__, jn)
    return dict(m=m, n=n, Ap=Ap, Ai=Ai, Ax=Ax, lb=lb, ub=ub, x=x, y=np.zeros(m), z=z, basis=basis, classes=classes,
                variables=[n + int(i) for i in cand_rows], expected_log=log, feastol=ft, decoy_row=decoy_row)


def primal_ratio_case(seed):
    """PrimalRatioTest.  One primal superbasic column per class (x = 1 in [0, inf): move_to = 0, step0 = 1), its entries at the
    member positions of the slack basis.  A member blocks at lb (pivot < 0, slack in [0, inf) at x_p = d) or at ub (pivot > 0,
    slack in [0, 4] at x_p = 4 - d), each with the ratio (d + feastol) / |pivot| = 2^-3 exactly; tied members differ in it.
      tie kinds    equal ratios and equal |pivot|: the lowest position wins, with ITS block_at_lb;
      strict       equal ratios, the higher position holds the larger |pivot|;
      pivot_zero   |pivot| = 1e-5 exactly at a slack sitting on its bound, which would block with the least ratio: no candidate;
      within_tol   the column's only entry has x_p + step0 pivot = lb - feastol exactly: it must not block.
    Candidates are pushed in ascending order of the column.  Expected: the pivot log, block_at_lb (the value x of the leaving
    slack: 0 or 4) and the step (x_jn = 1 - step afterwards)."""
    m, n = PRIMAL_SHAPE
    rng = np.random.default_rng(seed)
    ft = DYADIC_FEASTOL
    sets = placements(64, K_BLOCK, G, m)
    assert set(TIE_KINDS) < set(sets) and "strict" in sets
    sets["pivot_zero"] = [K_BLOCK * 40 + 1, K_BLOCK * 40 + 70]
    sets["within_tol"] = [K_BLOCK * 43 + 5]
    used = sorted(p for v in sets.values() for p in v)
    assert len(set(used)) == len(used) and max(used) < m
    cand_cols = np.linspace(9, n - 11, len(sets)).astype(int)
    assert len(set(cand_cols)) == len(sets)
    filler = np.setdiff1d(np.arange(m), used)
    N = n + m
    lb, ub, x = np.zeros(N), np.full(N, np.inf), np.zeros(N)
    x[n:] = 64.0                                                     # background slacks: far from blocking
    R, Cc, V = [], [], []
    classes, log = [], []
    for t, ((kind, members), j) in enumerate(zip(sets.items(), cand_cols)):
        k = len(members)
        sgn = np.array([-1.0, 1.0, 1.0, -1.0])[:k] * (1.0 if t % 2 == 0 else -1.0)      # pivot < 0: towards lb; > 0: towards ub
        a = np.full(k, 0.5)
        win = members[0]
        if kind == "strict":
            a, win = np.array([0.5, 1.0]), members[1]
        d = a * RATIO - ft                                           # the distance to the bound: ratio (d + ft) / a = 2^-3
        if kind == "pivot_zero":
            a, d, sgn, win = np.array([1e-5, 0.5]), np.array([0.0, 0.5 * RATIO - ft]), np.array([-1.0, 1.0]), members[1]
        elif kind == "within_tol":
            a, d, sgn, win = np.array([2.0]), np.array([2.0 - ft]), np.array([-1.0]), -1
        for p, s, dd in zip(members, sgn, d):
            if s < 0:
                x[n + p] = dd
            else:
                ub[n + p], x[n + p] = 4.0, 4.0 - dd
        R += list(members); Cc += [int(j)] * k; V += list(sgn * a)
        w = members.index(win) if win >= 0 else -1
        classes.append(dict(kind=kind, col=int(j), rows=list(members), pivots=sgn * a, d=d, winner=int(win),
                            at_lb=bool(w >= 0 and sgn[w] < 0), step=1.0 if w < 0 else float(d[w] / a[w])))
        if win >= 0:
            log.append((n + int(win), int(j)))
    x[cand_cols] = 1.0
    bg = np.setdiff1d(np.arange(n), cand_cols)
    R += list(filler[rng.integers(0, len(filler), len(bg))]); Cc += list(bg); V += list(rng.choice([-1.0, 1.0], len(bg)) * 2.0 ** rng.integers(-2, 3, len(bg)))
    Ap, Ai, Ax = csc(m, n, R, Cc, V)
    for c in classes:                                                # the two forms on every class's raw column
        f = np.zeros(m)
        f[c["rows"]] = c["pivots"]
        for form in (primal_ratio_free, primal_ratio_sequential):
            p, at_lb, _ = form(x[n:], f, lb[n:], ub[n:], 1.0, ft)
            assert p == c["winner"] and (p < 0 or at_lb == c["at_lb"]), (c["kind"], form.__name__, p, at_lb)
    return dict(m=m, n=n, Ap=Ap, Ai=Ai, Ax=Ax, lb=lb, ub=ub, x=x, basis=n + np.arange(m), classes=classes,
                variables=[int(j) for j in cand_cols], expected_log=log, feastol=ft)

