"""Exact-tie inputs for the pivot searches of the basis phase (starting_basis.hip, maxvolume.hip) and the answers they
must give.  NumPy only.

All data are dyadic: matrix entries +-2^a with |a| <= 2, scaling factors 2^b with |b| <= 6, at most 8 entries per column,
and every basis on the way is a permuted triangular matrix whose diagonal entries are powers of two.  Every product, sum
and quotient the searches compare is then exactly representable, so any summation order and any correct elimination order
give the same bits: a device result that differs from the expectation is a wrong decision, never rounding.  The generators
recompute what they plant in integer arithmetic (as_int: scale by 2^k, Python ints) and assert equality with the float64
values.

The searches are two-stage reductions with the rule "larger value wins, equal values: the LOWER index wins".  A tie class
is a set of two to four indices whose compared values are equal (mixed signs); the placements put its members where the
rule is applied by different pieces of code:
  lanes        one wavefront: the butterfly of wave_argmax (take_larger's oi < i)
  waves        two wavefronts of one workgroup: the fold over the wavefronts in block_partial / block_argmax
  blocks       two workgroups of one pass: the kernel that finishes the reduction
  later_pass   a LOWER workgroup in the second grid pass against a HIGHER workgroup in the first one: block order is not
               index order there (index gpass + 5 against 256 * 300 + 7: the winner is 76 807, a fold by block order
               answers 131 077)
  same_thread  indices q and q + gpass, which one thread visits one after the other: its loop keeps the first of equals
               only while its compare is strict
  strict       the LARGER index holds the strictly larger value (one dyadic step): "lowest index always" fails on it
The unit of a placement is the kernel's own: 64 lanes, 256 threads and gpass = G = 512 * 256 indices for the grid-stride
kernels; for sb_row_kernel (eight lanes per column) a wavefront holds 8 columns, a workgroup 32 and a pass G_ROW = 512 * 32."""
import numpy as np

K_BLOCK = 256                   # kBlock (internal.hpp): threads per workgroup
K_GRID = 512                    # kSbGrid (starting_basis.hip) = kRedGrid (maxvolume.hip): workgroups of every search kernel
K_ROW_LANES = 8                 # kRowLanes (starting_basis.hip): lanes per column in sb_row_kernel
G = K_GRID * K_BLOCK            # indices per grid pass of the grid-stride kernels
ROW_COLS = K_BLOCK // K_ROW_LANES
G_ROW = K_GRID * ROW_COLS       # columns per grid pass of sb_row_kernel
BASIC, BASIC_FREE, NONBASIC, NONBASIC_FIXED = 0, 1, -1, -2
MULTI_PASS = ("later_pass", "same_thread")


def as_int(x, k):
    """x * 2^k as a Python int (the scaling is exact in binary floating point); asserts that x is a multiple of 2^-k"""
    y = float(x) * 2.0 ** k
    assert np.isfinite(y) and y == int(y), (x, k)
    return int(y)


def placements(wave, block, gpass, limit, b=0):
    """{placement: member indices, ascending} for indices below limit; b: the first workgroup used (so that two sets on
    one index range do not meet).  Placements that do not fit below limit are left out; without a second pass `strict`
    spans two workgroups instead."""
    W, B = wave, block
    P = {"lanes": [B * b + 1, B * b + 3, B * b + W - 2],
         "waves": [B * (b + 1) + W + 1, B * (b + 1) + 3 * W + 2],
         "blocks": [B * b + 2 * W + 5, B * (b + 2) + W + 7],
         "later_pass": [B * (b + 300) + 7, gpass + B * b + 5],
         "same_thread": [B * b + 2 * W + 9, gpass + B * b + 2 * W + 9],
         "strict": [B * b + W + 20, gpass + B * b + W + 24]}
    if P["strict"][1] >= limit:
        P["strict"] = [B * b + W + 20, B * (b + 1) + 4]
    P = {k: v for k, v in P.items() if max(v) < limit}
    used = [i for v in P.values() for i in v]
    assert len(set(used)) == len(used)
    return P


def winner(kind, members):
    return max(members) if kind == "strict" else min(members)


def _signs(k):
    return np.array([1.0, -1.0, -1.0, 1.0])[:k]


def _csc(m, n, rows, cols, vals):
    rows, cols, vals = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(vals, np.float64)
    o = np.lexsort((rows, cols))
    rows, cols, vals = rows[o], cols[o], vals[o]
    assert not ((rows[1:] == rows[:-1]) & (cols[1:] == cols[:-1])).any(), "duplicate entry"
    p = np.zeros(n + 1, np.int64)
    np.add.at(p, cols + 1, 1)
    p = np.cumsum(p)
    assert (np.diff(p) <= 8).all() and np.isin(np.abs(vals), [0.25, 0.5, 1.0, 2.0, 4.0]).all()
    return p, rows, vals


def _background(rng, cols, rows_allowed, wexp):
    """one or two entries +-2^a per column in the allowed rows; the columns' scaling factors 2^b, b from wexp"""
    k = rng.integers(1, 3, len(cols))
    cc = np.repeat(cols, k)
    first = np.concatenate([[0], np.cumsum(k)[:-1]])
    r0 = rng.integers(0, len(rows_allowed), len(cols))
    off = np.arange(len(cc)) - np.repeat(first, k)                  # 0 or 1: the second entry in the cyclically next row
    rr = rows_allowed[(np.repeat(r0, k) + off * (1 + len(rows_allowed) // 3)) % len(rows_allowed)]
    vv = rng.choice([-1.0, 1.0], len(cc)) * 2.0 ** rng.integers(-2, 3, len(cc))
    return rr, cc, vv, 2.0 ** rng.choice(wexp, len(cols))


# ---- (a), (b): StartingBasis ------------------------------------------------------------------------------------------------
def starting_basis_case(m, n, seed):
    """A model whose exchanges have pairwise disjoint pivot rows and whose entering columns touch no pivot row but their own:
    from the slack basis every tableau column IS the raw column of A and every tableau row the raw row (the etas contribute
    zero multipliers), so the exchange log follows from A and the weights alone (expected_starting_basis).

    Free loop (sb_column_kernel): one free column per placement (64 / 256 / G on the ROWS); the tie members are its entries
    of largest magnitude, two smaller entries lie in rows that are never pivoted on.
    Fixed loop (sb_row_kernel, sb_row_scaled_kernel): one equality row per placement, once in the units of sb_row_scaled_kernel
    (64 / 256 / G on the COLUMNS, |r| and w differ inside a class, |r| w ties) and once in those of sb_row_kernel (8 / 32 / G_ROW,
    equal |r| and equal w: the row maximum itself ties); and three more rows:
      rw           2 * 1/2 against 1 * 1 against 4 * 1/4
      threshold    the row maximum 4 (in the third pass of sb_row_kernel where n allows) has a tiny weight; an entry 1/4 < 0.1 * 4 with
                   the largest weight must NOT qualify; the winner is the entry 1/2.  A row maximum missed by sb_row_kernel lowers
                   the threshold and lets the 1/4 in.
      fixed_decoy  a column with lb == ub (weight 0) holds the row's largest entry at the lowest index and is no candidate
    Weights: the device forms 1 / sqrt(zl / xl + zu / xu) (scaling_factor_kernel); with xu = inf, zu = 0, zl = 1 and
    xl = 4^b the quotient zl / xl = 4^-b, its root 2^-b and the reciprocal 2^b are all exact."""
    rng = np.random.default_rng(seed)
    N = n + m
    col_sets = placements(64, K_BLOCK, G, m)                                    # members: rows
    row_sets = {("scaled", k): v for k, v in placements(64, K_BLOCK, G, n).items()}
    row_sets.update({("row", k): v for k, v in placements(K_ROW_LANES, ROW_COLS, G_ROW, n, b=25).items()})
    far = 2 * G_ROW + ROW_COLS * 40 + 1 if n > 2 * G_ROW + ROW_COLS * 41 else ROW_COLS * 42 + 1
    row_sets[("special", "rw")] = [ROW_COLS * 40 + 3, ROW_COLS * 41 + 5, ROW_COLS * 41 + 14]
    row_sets[("special", "threshold")] = [ROW_COLS * 43 + 2, ROW_COLS * 43 + 19, far]
    row_sets[("special", "fixed_decoy")] = [ROW_COLS * 44 + 1, ROW_COLS * 44 + 9, ROW_COLS * 45 + 2]
    res_cols = np.array(sorted(j for v in row_sets.values() for j in v))
    res_rows = np.array(sorted(i for v in col_sets.values() for i in v))
    assert len(set(res_cols)) == len(res_cols) and res_cols.max() < n and res_rows.max() < m
    free_pool = np.setdiff1d(np.arange(n), res_cols)
    free_cols = free_pool[np.linspace(5, len(free_pool) - 7, len(col_sets)).astype(int)]
    row_pool = np.setdiff1d(np.arange(m), res_rows)
    eq_rows = row_pool[np.linspace(3, len(row_pool) - 5, len(row_sets)).astype(int)]
    filler = np.setdiff1d(row_pool, eq_rows)                                    # inequality rows that are never pivoted on
    assert len(set(free_cols)) == len(free_cols) and len(set(eq_rows)) == len(eq_rows) and len(filler) >= 16

    R, Cc, V = [], [], []
    w = np.zeros(N)
    lb, ub = np.zeros(N), np.full(N, np.inf)
    col_classes, row_classes = [], []
    for (kind, members), j in zip(col_sets.items(), free_cols):
        x = 2.0 ** rng.integers(0, 3)
        vals = x * _signs(len(members))
        if kind == "strict":
            vals = np.array([x / 2, -x])
        helpers = filler[rng.choice(len(filler), 2, replace=False)]
        R += list(members) + list(helpers); Cc += [j] * (len(members) + 2); V += list(vals) + [0.25, -0.25]
        lb[j], ub[j], w[j] = -np.inf, np.inf, np.inf
        col_classes.append(dict(kind=kind, col=int(j), rows=list(members), vals=vals, winner=winner(kind, members)))
    for ((unit, kind), members), i in zip(row_sets.items(), eq_rows):
        k = len(members)
        t = int(rng.integers(-2, 3))
        if unit == "scaled":
            a = np.array([-1, 1, 0, 2])[:k]                                     # |r| = 2^a, w = 2^(t - a): |r| w = 2^t
            if kind == "strict":
                a = np.array([1, 1])
            r, wj = 2.0 ** a * _signs(k), 2.0 ** (t - a)
            if kind == "strict":
                wj[1] *= 2.0
        elif unit == "row":
            r, wj = 2.0 ** t * _signs(k), np.full(k, 2.0 ** int(rng.integers(-3, 4)))
            if kind == "strict":
                r = 2.0 ** min(t, 1) * np.array([1.0, -2.0])
        elif kind == "rw":
            r, wj = np.array([2.0, -1.0, 4.0]), np.array([0.5, 1.0, 0.25])
        elif kind == "threshold":
            r, wj = np.array([0.25, -0.5, 4.0]), np.array([64.0, 0.5, 2.0 ** -6])
        else:
            r, wj = np.array([4.0, 1.0, -1.0]), np.array([0.0, 2.0, 2.0])
            ub[members[0]] = 0.0                                                # lb == ub == 0: weight 0
        R += [i] * k + list(filler[rng.choice(len(filler), k, replace=False)])
        Cc += list(members) * 2
        V += list(r) + list(rng.choice([-1.0, 1.0], k) * 2.0 ** rng.integers(-2, 3, k))
        w[members] = wj
        ub[n + i] = 0.0                                                         # an equality row: slack lb == ub == 0
        win = {"rw": members[0], "threshold": members[1], "fixed_decoy": members[1]}.get(kind, winner(kind, members))
        row_classes.append(dict(unit=unit, kind=kind, row=int(i), cols=list(members), r=r, w=wj, winner=int(win)))
    bg = np.setdiff1d(free_pool, free_cols)
    rr, cc, vv, wbg = _background(rng, bg, filler, np.arange(-6, 7))
    w[bg] = wbg
    w[n:] = np.where(ub[n:] == 0.0, 0.0, 1.0)
    Ap, Ai, Ax = _csc(m, n, np.concatenate([R, rr]), np.concatenate([Cc, cc]), np.concatenate([V, vv]))

    # the iterate whose scaling factors are w (Iterate::Initialize states: 1 free, 2 lower bound only, 4 boxed)
    free, fixed = np.isinf(lb), lb == ub
    bexp = np.zeros(N)
    bar = ~free & ~fixed
    bexp[bar] = np.log2(w[bar])
    assert np.array_equal(2.0 ** bexp[bar], w[bar]) and np.abs(bexp).max() <= 6
    it = dict(x=np.ones(N), y=np.zeros(m),
              xl=np.where(free, np.inf, np.where(fixed, 1.0, 4.0 ** bexp)), xu=np.where(fixed, 1.0, np.inf),
              zl=np.where(free, 0.0, 1.0), zu=np.where(fixed, 1.0, 0.0))
    with np.errstate(divide="ignore"):
        d = 1.0 / np.sqrt(it["zl"] / it["xl"] + it["zu"] / it["xu"])
    assert np.array_equal(d[bar], w[bar])                                       # the device's formula gives the planted weights
    state = np.where(free, 1, np.where(fixed, 4, 2)).astype(np.uint8)
    P = dict(m=m, n=n, Ap=Ap, Ai=Ai, Ax=Ax, lb=lb, ub=ub, b=np.zeros(m), c=np.zeros(N), w=w, it=it, state=state,
             col_classes=col_classes, row_classes=row_classes)
    P["expected"] = expected_starting_basis(P)
    assert_starting_basis_exact(P)
    return P


def expected_starting_basis(P):
    """The two loops of Basis::ConstructBasisFromWeights from the slack basis on a model of starting_basis_case: no solve.
    Returns the log (jb, jn), the final basis by position and the statuses; asserts the structure that makes it valid."""
    m, n, Ap, Ai, Ax, w = P["m"], P["n"], P["Ap"], P["Ai"], P["Ax"], P["w"]
    N = n + m
    cols = np.repeat(np.arange(n), np.diff(Ap))
    o = np.lexsort((cols, Ai))                                                  # the row-wise copy, columns ascending
    Tj, Tx = cols[o], Ax[o]
    Tp = np.concatenate([[0], np.cumsum(np.bincount(Ai, minlength=m))])
    basis = np.arange(n, N)
    pos = np.full(N, -1)
    pos[n:] = np.arange(m)
    log = []
    # free loop: candidates in descending j (remaining.back()); leaving: the slack of the FIRST row of max |a_ij| over the
    # positions whose basic variable is not free
    for jn in [j for j in range(N - 1, -1, -1) if np.isinf(w[j]) and pos[j] < 0]:
        rows, f = Ai[Ap[jn]:Ap[jn + 1]], np.abs(Ax[Ap[jn]:Ap[jn + 1]])
        keep = ~np.isinf(w[basis[rows]])
        assert f.max() <= 4.0 and f[keep].max() > 1e-6                          # no stability pivot, not dependent
        p = int(rows[keep][np.argmax(f[keep])])                                 # (rows ascend: argmax takes the first)
        log.append((int(basis[p]), jn))
        pos[basis[p]], pos[jn], basis[p] = -1, p, jn
    # fixed loop: equality slacks in descending order; entering: the first j maximising |a_ij| w_j among |a_ij| >= 0.1 max
    for jb in [j for j in range(N - 1, n - 1, -1) if w[j] == 0.0 and pos[j] >= 0]:
        i = jb - n
        assert pos[jb] == i
        j, r = Tj[Tp[i]:Tp[i + 1]], np.abs(Tx[Tp[i]:Tp[i + 1]])
        keep = (pos[j] < 0) & (w[j] != 0.0)
        j, r = j[keep], r[keep]
        assert r.max() <= 4.0 and r.max() > 1e-6
        cand = r >= 0.1 * r.max()
        jn = int(j[cand][np.argmax(r[cand] * w[j[cand]])])
        log.append((jb, jn))
        pos[jb], pos[jn], basis[i] = -1, i, jn
    # the structure: an entering column touches no pivot row but its own
    pivot_rows = {jb - n for jb, _ in log}
    assert len(pivot_rows) == len(log)
    for jb, jn in log:
        assert set(Ai[Ap[jn]:Ap[jn + 1]].tolist()) & pivot_rows == {jb - n}, (jb, jn)
    status = np.where(pos >= 0, BASIC, NONBASIC)
    special = (w == 0.0) | np.isinf(w)
    status[special] = np.where(pos[special] >= 0, BASIC_FREE, NONBASIC_FIXED)
    return dict(log=log, basis=basis, status=status)


def assert_starting_basis_exact(P):
    """what the searches compare, in integers: |a| 2^2, w 2^6 and |a| w 2^8; and the planted winners are the expected ones"""
    n, w = P["n"], P["w"]
    entered = {jn: jb for jb, jn in P["expected"]["log"]}
    for c in P["col_classes"]:
        v = [as_int(abs(x), 2) for x in c["vals"]]
        best = max(v)
        tied = [r for r, x in zip(c["rows"], v) if x == best]
        assert (len(tied) >= 2) != (c["kind"] == "strict") and c["winner"] == min(tied)
        assert entered[c["col"]] == n + c["winner"]
    for c in P["row_classes"]:
        assert np.array_equal(w[c["cols"]], c["w"])
        prod = [as_int(abs(r), 2) * as_int(x, 6) for r, x in zip(c["r"], c["w"])]
        assert prod == [as_int(abs(r) * x, 8) for r, x in zip(c["r"], c["w"])]
        rmax = max(as_int(abs(r), 2) for r, x in zip(c["r"], c["w"]) if x != 0.0)
        ok = [10 * as_int(abs(r), 2) >= rmax and x != 0.0 for r, x in zip(c["r"], c["w"])]      # |r| >= 0.1 rmax, in integers
        best = max(q for q, k in zip(prod, ok) if k)
        tied = [j for j, q, k in zip(c["cols"], prod, ok) if k and q == best]
        if c["unit"] != "special" or c["kind"] == "rw":
            assert (len(tied) >= 2) != (c["kind"] == "strict")
        assert c["winner"] == min(tied) and entered[c["winner"]] == n + c["row"]
        for r in c["r"]:                                                        # 0.1 rmax is no dyadic number: never an exact tie
            assert (abs(r) >= 0.1 * (rmax / 4.0)) == (10 * as_int(abs(r), 2) >= rmax)


# ---- (c): Maxvolume -------------------------------------------------------------------------------------------------------
def maxvolume_case(m, n, seed, rows_per_slice=10000):
    """A slack basis with dyadic scaling factors; only planted columns carry a large one, and their supports are pairwise
    disjoint (the duplicate of the `dup` class apart), the other columns stay off the planted rows: every basis on the way is
    permuted triangular with powers of two on its diagonal, so RunHeuristic and RunSequential are exact.
      ftran classes   (mv_scale_ftran_kernel, mvs_search_pivot_kernel; 64 / 256 / G on the POSITIONS): one column per
                      placement whose scaled entries |a_p| invscale_p d_j tie (from different a and invscale) at the members;
                      a fourth, smaller entry keeps its column weight nonzero in some slice whatever the signs cancel
      argmax classes  (mv_argmax_kernel; 64 / 256 / G on the COLUMNS): columns of equal |sum a invscale| d_j, all rows of a class
                      in one slice: single entries with different a, invscale and d_j, and a two-entry column 4 - 2;
                      `dup`: a column and its negated copy with the same scaling factor (only the first can enter)
    Expectations come from the CPU oracle; maxvolume_classes_met reads its log."""
    rng = np.random.default_rng(seed)
    N = n + m
    num_slices = min(m, 5 + m // rows_per_slice)
    ftran_sets = placements(64, K_BLOCK, G, m)                                  # members: positions = rows (slack basis)
    argmax_sets = placements(64, K_BLOCK, G, n)                                 # members: columns
    argmax_sets["dup"] = [K_BLOCK + 7, K_BLOCK + 64 + 9]
    res_cols = np.array(sorted(j for v in argmax_sets.values() for j in v))
    res_rows = np.array(sorted(i for v in ftran_sets.values() for i in v))
    assert len(set(res_cols)) == len(res_cols) and res_cols.max() < n
    col_pool = np.setdiff1d(np.arange(n), res_cols)
    ftran_cols = col_pool[np.linspace(9, len(col_pool) - 11, len(ftran_sets)).astype(int)]
    inv = 2.0 ** rng.integers(-1, 2, m)                                         # invscale_basic = 1 / colscale of the slacks
    R, Cc, V = [], [], []
    d = np.zeros(N)
    scaled_of = {}
    for kind, members in ftran_sets.items():                                    # (a, invscale) by member: a invscale = x
        x = 2.0 ** rng.integers(0, 2)
        for k, p in enumerate(members):
            inv[p] = 2.0 if kind == "strict" and k == 1 else (1.0, 0.5, 2.0, 1.0)[k]     # (strict: equal a, invscale decides)
            scaled_of[p] = x * (2.0 if kind == "strict" and k == 1 else 1.0)
    order = np.lexsort((np.arange(m), inv))                                     # Sortperm of (invscale, position)
    slice_of = np.zeros(m, np.int64)
    slice_of[order] = np.arange(m) % num_slices
    free_rows = np.setdiff1d(np.arange(m), res_rows)
    buckets = {}
    for p in free_rows[::-1]:
        buckets.setdefault((inv[p], int(slice_of[p])), []).append(int(p))

    def take(v, s):
        return buckets[(v, s)].pop()

    ftran_classes, argmax_classes = [], []
    for (kind, members), j in zip(ftran_sets.items(), ftran_cols):
        a = np.array([scaled_of[p] / inv[p] for p in members]) * _signs(len(members))
        x = min(scaled_of[p] for p in members)
        helper = take(1.0, int(rng.integers(0, num_slices)))
        R += list(members) + [helper]; Cc += [j] * (len(members) + 1); V += list(a) + [x / 4]
        d[j] = 2.0 ** rng.integers(5, 7)
        ftran_classes.append(dict(kind=kind, col=int(j), rows=list(members), a=a, winner=winner(kind, members)))
    for c, (kind, members) in enumerate(argmax_sets.items()):
        s = c % num_slices
        q = 2.0 ** (c // num_slices)                                            # classes that share a slice: different levels
        dj = 16.0
        cols = []
        for k, j in enumerate(members):
            sign = _signs(4)[k]
            if kind == "dup":
                if k == 0:
                    dup_rows = [take(1.0, s), take(2.0, s)]
                R += dup_rows; Cc += [j, j]; V += [sign * 2 * q, sign * -q / 2]          # 2q - q: sum a invscale = +-q
                d[j] = dj
            elif kind == "strict":
                R += [take(1.0, s)]; Cc += [j]; V += [sign * q * (2.0 if k == 1 else 1.0)]
                d[j] = dj
            elif k == 0:
                R += [take(1.0, s)]; Cc += [j]; V += [sign * q]                          # q * 1 * d
                d[j] = dj
            elif k == 1:
                R += [take(2.0, s)]; Cc += [j]; V += [sign * q]                          # q * 2 * d / 2
                d[j] = dj / 2
            else:
                R += [take(1.0, s), take(1.0, s)]; Cc += [j, j]; V += [sign * 2 * q, sign * -q]   # (2q - q) * 1 * d
                d[j] = dj
            cols.append(int(j))
        argmax_classes.append(dict(kind=kind, cols=cols, slice=s, winner=winner(kind, members)))
    planted_rows = np.unique(np.array(R))
    bg_rows = np.setdiff1d(np.arange(m), planted_rows)
    bg = np.setdiff1d(col_pool, ftran_cols)
    rr, cc, vv, dbg = _background(rng, bg, bg_rows, np.array([-6, -5]))
    d[bg] = dbg
    d[n:] = 1.0 / inv
    Ap, Ai, Ax = _csc(m, n, np.concatenate([R, rr]), np.concatenate([Cc, cc]), np.concatenate([V, vv]))
    status = np.concatenate([np.full(n, NONBASIC), np.full(m, BASIC)]).astype(np.int64)
    P = dict(m=m, n=n, Ap=Ap, Ai=Ai, Ax=Ax, basis=np.arange(n, N), status=status, colscale=d, inv=inv, slice_of=slice_of,
             num_slices=num_slices, rows_per_slice=rows_per_slice, ftran_classes=ftran_classes, argmax_classes=argmax_classes)
    assert_maxvolume_exact(P)
    return P


def assert_maxvolume_exact(P):
    """the scaled tableau columns a_p d_j invscale_p and the column weights sum over a slice of a_p invscale_p d_j of the planted
    columns from the slack basis, in integers (a 2^2, invscale 2^1, d 2^6)"""
    Ap, Ai, Ax, d, inv, n = P["Ap"], P["Ai"], P["Ax"], P["colscale"], P["inv"], P["n"]

    def column(j):
        rows, a = Ai[Ap[j]:Ap[j + 1]], Ax[Ap[j]:Ap[j + 1]]
        scaled = a * d[j] * inv[rows]
        ints = [as_int(x, 2) * as_int(d[j], 6) * as_int(v, 1) for x, v in zip(a, inv[rows])]
        assert ints == [as_int(x, 9) for x in scaled]
        return rows, ints, scaled
    planted = set()
    for c in P["ftran_classes"]:
        rows, ints, _ = column(c["col"])
        best = max(abs(x) for x in ints)
        assert best > 2 << 9                                                    # above the volume tolerance
        tied = [int(r) for r, x in zip(rows, ints) if abs(x) == best]
        assert (len(tied) >= 2) != (c["kind"] == "strict") and min(tied) == c["winner"]
        planted |= set(rows.tolist())
    for c in P["argmax_classes"]:
        weights = []
        for j in c["cols"]:
            rows, ints, scaled = column(j)
            assert (P["slice_of"][rows] == c["slice"]).all()
            assert sum(ints) == as_int(float(np.sum(scaled)), 9)
            weights.append(abs(sum(ints)))
            if c["kind"] != "dup" or j == c["cols"][0]:
                assert not planted & set(rows.tolist())
                planted |= set(rows.tolist())
        assert min(weights) > 2 << 9
        if c["kind"] == "strict":
            assert weights[1] == 2 * weights[0]
        else:
            assert len(set(weights)) == 1
    other = np.setdiff1d(np.arange(n), [c["col"] for c in P["ftran_classes"]] + [j for c in P["argmax_classes"] for j in c["cols"]])
    assert not np.isin(Ai[np.concatenate([np.arange(Ap[j], Ap[j + 1]) for j in other[:2000]])], sorted(planted)).any()
    assert d[other].max() <= 2.0 ** -5


def maxvolume_classes_met(P, log, variant):
    """From a log of exchanges (jb, jn): which planted classes were decided, and that each went to the stated rule.  Returns the
    placements decided, by search.  variant 'sequential' visits the columns in the order of their scaling factors: only the
    ftran classes apply."""
    n = P["n"]
    at = {int(jn): (k, int(jb)) for k, (jb, jn) in enumerate(np.asarray(log).tolist())}
    met = {"ftran": set(), "argmax": set()}
    for c in P["ftran_classes"]:
        assert c["col"] in at, "the column of ftran class %s never entered" % c["kind"]
        assert at[c["col"]][1] == n + c["winner"], (c["kind"], at[c["col"]], c["winner"])
        met["ftran"].add(c["kind"])
    if variant == "heuristic":
        for c in P["argmax_classes"]:
            cols = c["cols"]
            assert c["winner"] in at, "argmax class %s was not met" % c["kind"]
            if c["kind"] == "dup":
                assert all(j not in at for j in cols[1:])
            else:
                assert all(j in at for j in cols), "argmax class %s: a member never entered" % c["kind"]
                rest = sorted(j for j in cols if j != c["winner"])
                seq = [at[c["winner"]][0]] + [at[j][0] for j in rest]
                assert seq == sorted(seq), (c["kind"], seq)                     # the winner first, then ascending
            met["argmax"].add(c["kind"])
    return met


# ---- the shapes: the smallest that can still go wrong ---------------------------------------------------------------------
SMALL = (700, 1500)             # three workgroups' worth of positions, nine of columns: lanes, waves, blocks, strict
TALL = (G + 257, 1500)          # m one workgroup and a wavefront past a grid pass: sb_column, mv_scale_ftran, mvs_search_pivot
WIDE = (300, G + 257)           # n past a grid pass (n + m = G + 557), eight passes of sb_row_kernel: sb_row*, mv_argmax
ROWS_PER_SLICE = {SMALL: 10000, TALL: 100000, WIDE: 10000}      # 5, 6 and 5 slices
