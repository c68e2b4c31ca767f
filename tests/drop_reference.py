"""DropPrimal / DropDual (reference src/kkt_solver_basis.cc:196-387) restated in dense NumPy, the three iterate changes that
go with them (make_implied_lb / _ub, make_fixed), planted states on which all four outcomes occur, and exact dyadic cases for
the two pivot searches of drop.hip.  NumPy only.

Actions of the decision log (variable, action, partner): 0 exchanged, 1 implied at lb, 2 implied at ub, 3 fixed."""
import numpy as np

from basis_ties_reference import BASIC, BASIC_FREE, G, G_ROW, K_BLOCK, K_ROW_LANES, NONBASIC, NONBASIC_FIXED, ROW_COLS, _signs, placements, winner

EXCHANGED, IMPLIED_LB, IMPLIED_UB, FIXED = 0, 1, 2, 3
ST_FIXED, ST_FREE, ST_LB, ST_UB, ST_BOXED, ST_IMPLIED_LB, ST_IMPLIED_UB = range(7)
PIVOT_ZERO_TOL, VOLUME_TOL = 1e-7, 2.0


def scaling_factors(it, state):
    """Iterate::ScalingFactor (src/iterate.cc:183-198) with the device's formula"""
    with np.errstate(divide="ignore", invalid="ignore"):
        d = 1.0 / np.sqrt(it["zl"] / it["xl"] + it["zu"] / it["xu"])
    d[state == ST_FIXED] = 0.0
    d[(state == ST_FREE) | (state == ST_IMPLIED_LB) | (state == ST_IMPLIED_UB)] = np.inf
    return d


def objectives(P, it, state):
    """Iterate::ComputeObjectives (src/iterate.cc:610-638), without the offset: (pobjective, dobjective)"""
    n, m = P["n"], P["m"]
    x, c = it["x"], P["c"]
    implied = (state == ST_IMPLIED_LB) | (state == ST_IMPLIED_UB)
    pobj = np.sum(np.where(state != ST_FIXED, c * x, 0.0)) - np.sum(np.where(implied, (it["zl"] - it["zu"]) * x, 0.0))
    has_lb, has_ub = (state == ST_LB) | (state == ST_BOXED), (state == ST_UB) | (state == ST_BOXED)
    with np.errstate(invalid="ignore"):
        dobj = P["b"] @ it["y"] + np.sum(np.where(has_lb, P["lb"] * it["zl"], 0.0)) - np.sum(np.where(has_ub, P["ub"] * it["zu"], 0.0))
    fixed = np.nonzero(state == ST_FIXED)[0]
    if len(fixed):
        AI = dense_AI(P)
        dobj -= np.sum(x[fixed] * (AI[:, fixed].T @ it["y"]))
    return pobj, dobj


def dense_AI(P):
    m, n = P["m"], P["n"]
    AI = np.zeros((m, n + m))
    cols = np.repeat(np.arange(n), np.diff(P["Ap"]))
    AI[P["Ai"], cols] = P["Ax"]
    AI[np.arange(m), n + np.arange(m)] = 1.0
    return AI


class Margin:
    """the smallest relative distance |a - b| / max(|a|, |b|) of any comparison taken"""
    def __init__(self):
        self.value = np.inf

    def cmp(self, a, b):
        a, b = np.broadcast_arrays(np.asarray(a, float), np.asarray(b, float))
        ok = np.isfinite(a) & np.isfinite(b) & ((a != 0) | (b != 0))
        if ok.any():
            self.value = min(self.value, float(np.min(np.abs(a[ok] - b[ok]) / np.maximum(np.abs(a[ok]), np.abs(b[ok])))))

    def best(self, v):
        """index of the first largest entry of v (len >= 1); the margin to the runner-up"""
        k = int(np.argmax(v))
        rest = np.delete(v, k)
        if len(rest):
            self.cmp(v[k], rest.max())
        return k


def restatement(P, drop_primal, drop_dual):
    """Both procedures on the state P (model Ap/Ai/Ax/b/c/lb/ub, iterate it, state, basis, status), dense solves.  Returns the
    log, the final basis / status / state / iterate vectors / colscale and the smallest relative margin of any comparison."""
    m, n = P["m"], P["n"]
    N = n + m
    AI = dense_AI(P)
    it = {k: v.copy() for k, v in P["it"].items()}
    state, basis, status = P["state"].copy(), P["basis"].copy(), P["status"].copy()
    xl, xu, zl, zu = it["xl"], it["xu"], it["zl"], it["zu"]
    M = Margin()
    log = []
    colscale = scaling_factors(it, state)
    out = dict(log=log, basis=basis, status=status, state=state, it=it, colscale=colscale, margin=M)
    pobj, dobj = objectives(P, it, state)
    M.cmp(pobj, dobj)
    if not pobj >= dobj:                                                        # the gate (:36)
        return out
    pos = np.full(N, -1)
    pos[basis] = np.arange(m)

    def invscale_basic():
        with np.errstate(divide="ignore"):
            return np.where(status[basis] == BASIC, 1.0 / colscale[basis], 0.0)

    def stable(pc, pr):
        assert pc != 0.0 and abs(pc - pr) <= 1e-10 * abs(pc), "an exchange the restatement cannot follow (refused or nearly so)"

    def exchange(p, jb, jn):
        basis[p] = jn
        pos[jn], pos[jb] = p, -1
        status[jn], status[jb] = BASIC, NONBASIC

    # ---- DropPrimal
    if drop_primal > 0.0:
        cand = []
        for p in range(m):
            jb = basis[p]
            if status[jb] != BASIC:
                continue
            xj, zj = (xl[jb], zl[jb]) if xl[jb] <= xu[jb] else (xu[jb], zu[jb])
            M.cmp(xl[jb], xu[jb]); M.cmp(xj, 0.01 * zj); M.cmp(xj, drop_primal)
            if xj < 0.01 * zj and xj <= drop_primal:
                cand.append(int(jb))
        inv = invscale_basic() if cand else None
        while cand:
            jb = cand[-1]
            p = pos[jb]
            B = AI[:, basis]
            btran = np.linalg.solve(B.T, np.eye(m)[p])
            r = AI.T @ btran
            nb = np.nonzero(status == NONBASIC)[0]
            a = np.abs(r[nb])
            M.cmp(a, PIVOT_ZERO_TOL)
            keep = a > PIVOT_ZERO_TOL
            v = a[keep] * colscale[nb[keep]] * inv[p]
            M.cmp(v, VOLUME_TOL)
            ok = v > VOLUME_TOL
            if ok.any():
                jmax = int(nb[keep][ok][M.best(v[ok])])
                stable(np.linalg.solve(B, AI[:, jmax])[p], r[jmax])
                exchange(p, jb, jmax)
                inv[p] = 1.0 / colscale[jmax]
                log.append((jb, EXCHANGED, jmax))
            else:
                with np.errstate(divide="ignore", invalid="ignore"):
                    ql, qu = zl[jb] / xl[jb], zu[jb] / xu[jb]
                M.cmp(ql, qu)
                lower = ql > qu
                state[jb] = ST_IMPLIED_LB if lower else ST_IMPLIED_UB
                xl[jb] = xu[jb] = np.inf
                status[jb] = BASIC_FREE
                inv[p] = 0.0
                colscale[jb] = np.inf
                log.append((jb, IMPLIED_LB if lower else IMPLIED_UB, -1))
            cand.pop()
    # ---- DropDual
    if drop_dual > 0.0:
        cand = []
        for jn in range(N):
            if status[jn] != NONBASIC:
                continue
            xj, zj = (xl[jn], zl[jn]) if zl[jn] >= zu[jn] else (xu[jn], zu[jn])
            M.cmp(zl[jn], zu[jn]); M.cmp(zj, 0.01 * xj); M.cmp(zj, drop_dual)
            if zj < 0.01 * xj and zj <= drop_dual:
                cand.append(jn)
        inv = invscale_basic() if cand else None
        while cand:
            jn = cand[-1]
            B = AI[:, basis]
            lhs = np.linalg.solve(B, AI[:, jn])
            a = np.abs(lhs)
            M.cmp(a, PIVOT_ZERO_TOL)
            v = a * inv * colscale[jn]
            M.cmp(v[a > PIVOT_ZERO_TOL], VOLUME_TOL)
            ok = np.nonzero((a > PIVOT_ZERO_TOL) & (v > VOLUME_TOL))[0]
            if len(ok):
                pmax = int(ok[M.best(v[ok])])
                jb = int(basis[pmax])
                stable(lhs[pmax], AI[:, jn] @ np.linalg.solve(B.T, np.eye(m)[pmax]))
                exchange(pmax, jb, jn)
                inv[pmax] = 1.0 / colscale[jn]
                log.append((jn, EXCHANGED, jb))
            else:
                xl[jn] = xu[jn] = zl[jn] = zu[jn] = 0.0
                state[jn] = ST_FIXED
                status[jn] = NONBASIC_FIXED
                colscale[jn] = 0.0
                log.append((jn, FIXED, -1))
            cand.pop()
    return out


def csc(m, n, rows, cols, vals):
    rows, cols, vals = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(vals, np.float64)
    o = np.lexsort((rows, cols))
    rows, cols, vals = rows[o], cols[o], vals[o]
    assert not ((rows[1:] == rows[:-1]) & (cols[1:] == cols[:-1])).any(), "duplicate entry"
    p = np.zeros(n + 1, np.int64)
    np.add.at(p, cols + 1, 1)
    return np.cumsum(p), rows, vals


def planted_state(m, n, seed, gate_open=True):
    """The slack basis (its factors are the identity) of a random sparse model without free or fixed variables, and an iterate in
    which chosen basic slacks have xj tiny against zj and chosen nonbasic columns zj tiny against xj:
      primal candidates   `exchange` rows hold ordinary nonbasic columns (one enters); `implied` rows hold only `dead` columns,
                          whose scaling factor 1e-10 cannot reach the volume tolerance: lower bound only and boxed slacks near lb
                          become implied at lb, upper bound only and boxed ones near ub implied at ub;
      dual candidates     `enter` columns have ordinary support (a basic slack leaves); `fix` columns are supported in `heavy` rows
                          only, whose slacks have scaling factor 1e10.
    b = AI x and c = AI'y + zl - zu, so pobjective - dobjective is the complementarity sum: the gate is open.  gate_open=False
    moves b along y until dobjective exceeds pobjective."""
    rng = np.random.default_rng(seed)
    N = n + m
    rows_p = rng.permutation(m)
    k_imp, k_exc, k_heavy = 4, 4, max(4, m // 10)
    implied_rows, exchange_rows, heavy_rows = rows_p[:k_imp], rows_p[k_imp:k_imp + k_exc], rows_p[k_imp + k_exc:k_imp + k_exc + k_heavy]
    normal_rows = rows_p[k_imp + k_exc + k_heavy:]
    cols_p = rng.permutation(n)
    k_dead, k_enter, k_fix = max(6, n // 10), 4, 3
    dead, enter, fix = cols_p[:k_dead], cols_p[k_dead:k_dead + k_enter], cols_p[k_dead + k_enter:k_dead + k_enter + k_fix]
    normal = cols_p[k_dead + k_enter + k_fix:]
    R, Cc = [], []
    for j in normal:                                                # never in an implied row
        rr = rng.choice(np.concatenate([exchange_rows, heavy_rows, normal_rows]), 4, replace=False)
        R += list(rr); Cc += [j] * 4
    for j in dead:
        rr = rng.choice(np.concatenate([implied_rows, normal_rows, heavy_rows]), 4, replace=False)
        R += list(rr); Cc += [j] * 4
    for t, i in enumerate(implied_rows):                            # every implied row holds a dead column
        R.append(i); Cc.append(dead[t])
    for j in enter:
        rr = rng.choice(normal_rows, 4, replace=False)
        R += list(rr); Cc += [j] * 4
    for j in fix:
        rr = rng.choice(heavy_rows, 3, replace=False)
        R += list(rr); Cc += [j] * 3
    R, Cc = np.array(R), np.array(Cc)
    _, first = np.unique(R * n + Cc, return_index=True)
    R, Cc = R[first], Cc[first]
    V = rng.choice([-1.0, 1.0], len(R)) * rng.uniform(0.5, 2.0, len(R))
    Ap, Ai, Ax = csc(m, n, R, Cc, V)

    lb, ub = np.zeros(N), np.full(N, np.inf)
    xl, zl = rng.uniform(0.5, 2.0, N), rng.uniform(0.5, 2.0, N)
    xu, zu = np.full(N, np.inf), np.zeros(N)
    boxed = np.concatenate([normal[::7], n + normal_rows[::5]])
    ub[boxed] = 10.0
    xu[boxed], zu[boxed] = rng.uniform(0.5, 2.0, len(boxed)), rng.uniform(0.5, 2.0, len(boxed))
    xl[dead], zl[dead] = 1e-20, 1.0
    xl[n + heavy_rows], zl[n + heavy_rows] = 1.0, 1e-20
    xl[n + exchange_rows], zl[n + exchange_rows] = 1e-12 * rng.uniform(1.0, 2.0, k_exc), 1.0
    xl[enter], zl[enter] = 1.0, 1e-12 * rng.uniform(1.0, 2.0, k_enter)
    xl[fix], zl[fix] = 1.0, 1e-12 * rng.uniform(1.0, 2.0, k_fix)
    j = fix[0]                                                      # a boxed dual candidate: the larger dual is zl
    ub[j], xu[j], zu[j] = 10.0, 2.0, 1e-13
    i0, i1, i2, i3 = n + implied_rows
    xl[i0], zl[i0] = 1e-12, 1.0                                     # lower bound only: implied at lb
    lb[i1], ub[i1] = -np.inf, 0.0                                   # upper bound only: implied at ub
    xl[i1], zl[i1], xu[i1], zu[i1] = np.inf, 0.0, 1e-12, 1.0
    ub[i2] = 10.0                                                   # boxed, near lb
    xl[i2], zl[i2], xu[i2], zu[i2] = 1e-12, 1.0, 1.0, 1e-3
    ub[i3] = 10.0                                                   # boxed, near ub
    xl[i3], zl[i3], xu[i3], zu[i3] = 1.0, 1e-3, 1e-12, 1.0
    with np.errstate(invalid="ignore"):
        x = np.where(np.isfinite(lb), lb + xl, ub - xu)
    xu = np.where(np.isfinite(ub), ub - x, np.inf)                  # (boxed: xl + xu = ub - lb up to rounding; the residual is not tested)
    xu[i3] = 1e-12; xu[i1] = 1e-12; xu[j] = 2.0
    y = rng.uniform(-1.0, 1.0, m)
    state = np.where(np.isinf(lb), ST_UB, np.where(np.isinf(ub), ST_LB, ST_BOXED)).astype(np.uint8)
    it = dict(x=x, xl=xl, xu=xu, y=y, zl=zl, zu=zu)
    P = dict(m=m, n=n, Ap=Ap, Ai=Ai, Ax=Ax, lb=lb, ub=ub, it=it, state=state, basis=np.arange(n, N),
             status=np.concatenate([np.full(n, NONBASIC), np.full(m, BASIC)]).astype(np.int64))
    AI = dense_AI(P)
    P["b"] = AI @ x
    P["c"] = AI.T @ y + zl - zu
    if not gate_open:
        pobj, dobj = objectives(P, it, state)
        P["b"] = P["b"] + y * (2.0 * (pobj - dobj) + 1.0) / (y @ y)
    return P


# ---- exact dyadic cases for the two searches ------------------------------------------------------------------------------
# Slack basis; a candidate's tableau row / column is the raw row / column of A because no entering column touches a pivot row but
# its own and no two candidates share a row.  Scaling factors 2^b come from xl = 4^b, zl = 1 (or zl = 4^-b, xl = 1): the quotient, its
# root and the reciprocal are exact, and so is every product the searches compare.
ROW_SHAPE = (300, 3 * G_ROW + 900)          # n + m past three passes of drop_row_kernel (G_ROW columns each)
COL_SHAPE = (G + 257, 1500)                 # m past one pass of drop_column_kernel (G positions)
DROP_TOL = 2.0 ** -30                       # xj = 4^-20 and zj = 4^-16 are below it


def _finish_dyadic(m, n, R, Cc, V, wexp, cand_slack=(), cand_cols=(), free_slack=(), fixed_cols=(), slack_wexp=None):
    """model + iterate: column j has scaling factor 2^wexp[j]; candidate slacks xl = 4^-20, zl = 1 (2^-20); candidate columns
    zl = 4^-16, xl = 1 (2^16); free slacks lb = -inf, ub = inf; fixed columns lb = ub = 0"""
    N = n + m
    Ap, Ai, Ax = csc(m, n, R, Cc, V)
    e = np.zeros(N)
    e[:n] = wexp
    if slack_wexp is not None:
        e[n:] = slack_wexp
    lb, ub = np.zeros(N), np.full(N, np.inf)
    xl, zl = 4.0 ** e, np.ones(N)
    cs, cc, fs, fc = (np.asarray(a, np.int64) for a in (cand_slack, cand_cols, free_slack, fixed_cols))
    xl[n + cs] = 4.0 ** -20
    xl[cc], zl[cc] = 1.0, 4.0 ** -16
    lb[n + fs] = -np.inf
    xl[n + fs], zl[n + fs] = np.inf, 0.0
    ub[fc] = 0.0
    it = dict(x=np.where(np.isfinite(lb), lb + np.where(np.isfinite(xl), xl, 0.0), 0.0), xl=xl, xu=np.full(N, np.inf), y=np.zeros(m),
              zl=zl, zu=np.zeros(N))
    it["xu"][fc], it["zu"][fc], it["xl"][fc], it["x"][fc] = 1.0, 1.0, 1.0, 0.0          # lb == ub: Iterate::Initialize gives boxed
    state = np.where(np.isinf(lb), ST_FREE, np.where(np.isinf(ub), ST_LB, ST_BOXED)).astype(np.uint8)
    # c = 1 on the slacks of the candidate rows: pobjective > 0 = dobjective (y = 0, lb = 0 wherever zl counts)
    c = np.zeros(N)
    c[n:] = 1.0
    c[n + fs] = 0.0
    return dict(m=m, n=n, Ap=Ap, Ai=Ai, Ax=Ax, lb=lb, ub=ub, b=np.zeros(m), c=c, it=it, state=state)


def row_search_case(seed):
    """DropPrimal's fused row search.  One candidate slack per class (invscale 2^20), its row holding the class members:
      placements(8 lanes, 32 columns, G_ROW): |r_j| colscale_j ties from different r and colscale (lanes / waves / blocks /
        later_pass / same_thread), strict: the larger index strictly larger;
      third_pass   members in the first and in the fourth pass;
      pivot_zero   an entry |r| = 1e-7 (not > kPivotZeroTol) with the largest scaling factor must not count: the winner is the other;
      volume_two   the only entry gives v = 2.0 exactly: no winner, the slack becomes implied at lb;
      fixed_decoy  a NONBASIC_FIXED column (lb == ub) holds the row's largest entry at the lowest index and is no candidate.
    Expected log: candidates from the back of the position list (descending row)."""
    m, n = ROW_SHAPE
    rng = np.random.default_rng(seed)
    sets = placements(K_ROW_LANES, ROW_COLS, G_ROW, n, b=3)
    sets["third_pass"] = [ROW_COLS * 50 + 4, 3 * G_ROW + ROW_COLS * 2 + 6]
    sets["pivot_zero"] = [ROW_COLS * 52 + 1, ROW_COLS * 52 + 9]
    sets["volume_two"] = [ROW_COLS * 54 + 3]
    sets["fixed_decoy"] = [ROW_COLS * 56 + 1, ROW_COLS * 56 + 9, ROW_COLS * 57 + 2]
    used = sorted(j for v in sets.values() for j in v)
    assert len(set(used)) == len(used) and max(used) < n
    cand_rows = np.linspace(5, m - 7, len(sets)).astype(int)
    assert len(set(cand_rows)) == len(sets)
    filler = np.setdiff1d(np.arange(m), cand_rows)
    R, Cc, V = [], [], []
    wexp = rng.integers(-6, -3, n).astype(float)                    # background columns: small scaling factors, off the candidate rows
    classes = []
    for (kind, members), i in zip(sets.items(), cand_rows):
        k = len(members)
        t = int(rng.integers(-17, -14))                             # |r| w = 2^t: v = 2^(t + 20) in 8 .. 32
        a = np.array([-1, 1, 0, 2])[:k]
        r, w = 2.0 ** a * _signs(k), (t - a).astype(float)
        win = winner(kind, members)
        if kind == "strict":
            r, w = np.array([2.0, -2.0]), np.array([t - 1.0, t])
        elif kind == "pivot_zero":
            r, w = np.array([1e-7, 1.0]), np.array([12.0, float(t)])         # (counted, it would give v = 429)
            win = members[1]
        elif kind == "volume_two":
            r, w = np.array([0.5]), np.array([-18.0])               # 0.5 * 2^-18 * 2^20 = 2.0
            win = -1
        elif kind == "fixed_decoy":
            r, w = np.array([4.0, 1.0, -1.0]), np.array([0.0, float(t), float(t)])
            win = members[1]
        R += [i] * k; Cc += list(members); V += list(r)
        wexp[members] = w
        classes.append(dict(kind=kind, row=int(i), cols=list(members), r=r, wexp=w, winner=int(win)))
    bg = np.setdiff1d(np.arange(n), used)
    R += list(filler[rng.integers(0, len(filler), len(bg))]); Cc += list(bg); V += list(rng.choice([-1.0, 1.0], len(bg)) * 2.0 ** rng.integers(-2, 3, len(bg)))
    for c in classes:                                               # an entering column also holds an entry in a row that is never pivoted on
        if c["winner"] >= 0:
            R.append(int(filler[rng.integers(0, len(filler))])); Cc.append(c["winner"]); V.append(0.25)
    P = _finish_dyadic(m, n, R, Cc, V, wexp, cand_slack=cand_rows, fixed_cols=[sets["fixed_decoy"][0]])
    P["classes"] = classes
    # the expectation, in exact arithmetic: v = |r| 2^wexp 2^20
    log = []
    for c in sorted(classes, key=lambda c: -c["row"]):
        v = [abs(r) * 2.0 ** w * 2.0 ** 20 if abs(r) > PIVOT_ZERO_TOL and j != sets["fixed_decoy"][0] else 0.0
             for j, r, w in zip(c["cols"], c["r"], c["wexp"])]
        ok = [j for j, x in zip(c["cols"], v) if x > VOLUME_TOL and x == max(v)]
        assert (min(ok) if ok else -1) == c["winner"], c
        if c["kind"] not in ("pivot_zero", "volume_two", "fixed_decoy"):
            assert (len(ok) >= 2) != (c["kind"] == "strict")
        log.append((n + c["row"], EXCHANGED, c["winner"]) if ok else (n + c["row"], IMPLIED_LB, -1))
    P["expected_log"] = log
    return P


def column_search_case(seed):
    """DropDual's search over the positions.  One candidate column per class (scaling factor 2^16), its entries at the member
    positions with |a_p| invscale_p ties from different a and invscale; `free_decoy`: a BASIC_FREE slack (a free row) holds the
    column's largest entry at the lowest position and can never win; `volume_two`: v = 2.0 exactly, the column is fixed.
    Expected log: candidates in descending j."""
    m, n = COL_SHAPE
    rng = np.random.default_rng(seed)
    sets = placements(64, K_BLOCK, G, m)
    sets["free_decoy"] = [K_BLOCK * 40 + 1, K_BLOCK * 40 + 70, K_BLOCK * 41 + 2]
    sets["volume_two"] = [K_BLOCK * 43 + 5]
    used = sorted(p for v in sets.values() for p in v)
    assert len(set(used)) == len(used) and max(used) < m
    cand_cols = np.linspace(9, n - 11, len(sets)).astype(int)
    assert len(set(cand_cols)) == len(sets)
    filler = np.setdiff1d(np.arange(m), used)
    R, Cc, V = [], [], []
    slack_wexp = np.zeros(m)
    classes = []
    for (kind, members), j in zip(sets.items(), cand_cols):
        k = len(members)
        t = int(rng.integers(-13, -10))                             # |a| invscale = 2^t: v = 2^(t + 16) in 8 .. 32
        e = np.array([-1, 1, 0, 2])[:k]
        a, inv = 2.0 ** e * _signs(k), (t - e).astype(float)
        win = winner(kind, members)
        if kind == "strict":
            a, inv = np.array([2.0, -2.0]), np.array([t - 1.0, t])
        elif kind == "free_decoy":
            a, inv = np.array([4.0, 1.0, -1.0]), np.array([0.0, float(t), float(t)])
            win = members[1]
        elif kind == "volume_two":
            a, inv = np.array([0.5]), np.array([-14.0])             # 0.5 * 2^-14 * 2^16 = 2.0
            win = -1
        R += list(members); Cc += [j] * k; V += list(a)
        slack_wexp[members] = -inv                                  # invscale = 1 / colscale of the slack
        classes.append(dict(kind=kind, col=int(j), rows=list(members), a=a, invexp=inv, winner=int(win)))
    bg = np.setdiff1d(np.arange(n), cand_cols)
    R += list(filler[rng.integers(0, len(filler), len(bg))]); Cc += list(bg); V += list(rng.choice([-1.0, 1.0], len(bg)) * 2.0 ** rng.integers(-2, 3, len(bg)))
    P = _finish_dyadic(m, n, R, Cc, V, rng.integers(-6, -3, n).astype(float), cand_cols=cand_cols, free_slack=[sets["free_decoy"][0]],
                       slack_wexp=slack_wexp)
    P["classes"] = classes
    log = []
    for c in sorted(classes, key=lambda c: -c["col"]):
        v = [abs(a) * 2.0 ** e * 2.0 ** 16 if p != sets["free_decoy"][0] else 0.0 for p, a, e in zip(c["rows"], c["a"], c["invexp"])]
        ok = [p for p, x in zip(c["rows"], v) if x > VOLUME_TOL and x == max(v)]
        assert (min(ok) if ok else -1) == c["winner"], c
        if c["kind"] not in ("free_decoy", "volume_two"):
            assert (len(ok) >= 2) != (c["kind"] == "strict")
        log.append((c["col"], EXCHANGED, n + c["winner"]) if ok else (c["col"], FIXED, -1))
    P["expected_log"] = log
    return P
