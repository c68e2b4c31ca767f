"""Pure numpy references for the SpMV epilogues (ipx_amd/csrc/spmv_kernels.hpp and the files that launch them): no GPU,
no oracle.

Every epilogue is out[r] = finish(init(r) (+|-) sum_p prod(x[idx[p]], val[p])) over one row r of a gather matrix G: Acols
(row j = column j of A, gathers y, gives A'y) or Arows (row i = row i of A with ascending columns, gathers a column vector,
gives A t).  For an operation this module returns an Op with, per output entry,

  ld    the long-double value (products and sums in np.longdouble, the epilogue's expression in np.longdouble);
  seq   the sequential double value: every product rounded to double, added one by one in storage order starting from
        init, then the epilogue's own expression order in double -- what the header of spmv_kernels.hpp promises for the
        layouts that keep the storage order;
  alt   the same in double with the row summed in reversed and in pairwise order (tests/test_epilogue_reference.py holds
        them to the gate: any association must pass it);
  gate  g_r = (len_r + c_epi + 2) * 2^-53 * S_r, with len_r the row's entry count, c_epi the floating-point operations of
        the epilogue after the sum (counted from the functor, next to each function below) and S_r the long-double sum of
        |init|, of every |product| and of every further addend of the epilogue -- multiplied by the |factor| where the
        epilogue scales its result (EpiRecoverX, EpiBasisColumns), so that S_r is a magnitude of the output.

The gate is the standard bound for a sum of rounded products in any association: a term passes through at most one
rounding of its product (two for (v*w)*v), at most len_r additions and the c_epi operations, hence the error is at most
(len_r + c_epi + 1) u S_r to first order in u = 2^-53; one more u covers the second-order terms and the long-double
reference's own error (2^-64 per operation).  It is derived; no device result enters it.  A dot output has the same form
with len replaced by (number of rows + longest row) and S by the sum of the absolute contributions.

EpiSmwRows is pinned by test_gpu_smw_dense.py and test_gpu_combine_loads.py, EpiScale and EpiNormalRows by normal_apply in
test_gpu_parity.py (test_spmv_layouts_agree, test_sorted_fused_layout_on_a_banded_matrix) and the acc_* tests,
EpiPostprocess by test_gpu_finish.py; they have no function here.
"""
import numpy as np

from ipx_amd import synth

LD = np.longdouble
U = 2.0 ** -53
FIXED, FREE, LB, UB, BOXED = range(5)
MAX_ROW_LEN = 255                      # kMaxRowLen: longer rows go to the long-row kernels (segment sums)


# ---- gather matrices ----------------------------------------------------------------------------------------------------
class Gather:
    """rows of a gather matrix: ptr, idx, val (storage order)"""

    def __init__(self, nrows, ncols, ptr, idx, val):
        self.nrows, self.ncols = int(nrows), int(ncols)
        self.ptr, self.idx, self.val = np.asarray(ptr, np.int64), np.asarray(idx, np.int64), np.asarray(val, np.float64)
        self.len = np.diff(self.ptr)

    @property
    def long_rows(self):
        return self.len > MAX_ROW_LEN


def acols(A):
    """gathers by column: row j lists column j of A in its storage order"""
    return Gather(A.ncol, A.nrow, A.p, A.i, A.x)


def arows(A):
    """gathers by row: row i lists row i of A, columns ascending (a stable sort of the CSC entries by row)"""
    cols = np.repeat(np.arange(A.ncol, dtype=np.int64), np.diff(A.p))
    order = np.argsort(A.i, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(A.i, minlength=A.nrow))])
    return Gather(A.nrow, A.ncol, ptr, cols[order], A.x[order])


class Op:
    def __init__(self, ld, seq, alt, gate, length):
        self.ld, self.seq, self.alt, self.gate, self.len = ld, seq, alt, gate, length


def _padded(G, values, dtype):
    """nrows x (longest row) matrix of the rows' values in storage order, zeros behind a row's end (adding 0.0 is exact)"""
    width = int(G.len.max()) if G.nrows and G.len.size else 0
    P = np.zeros((G.nrows, max(width, 1)), dtype)
    rows = np.repeat(np.arange(G.nrows), G.len)
    pos = np.arange(G.ptr[-1]) - np.repeat(G.ptr[:-1], G.len)
    P[rows, pos] = values
    return P


def _fold(P, init, neg, order):
    """init (+|-) the entries of each row of P, one by one (sequential, reversed) or init (+|-) their pairwise sum"""
    acc = np.array(init, dtype=P.dtype, copy=True)
    if order == "pairwise":
        Q = P
        while Q.shape[1] > 1:
            if Q.shape[1] % 2:
                Q = np.concatenate([Q, np.zeros((Q.shape[0], 1), Q.dtype)], axis=1)
            Q = Q[:, 0::2] + Q[:, 1::2]
        return acc - Q[:, 0] if neg else acc + Q[:, 0]
    cols = range(P.shape[1]) if order == "sequential" else range(P.shape[1] - 1, -1, -1)
    for k in cols:
        acc = acc - P[:, k] if neg else acc + P[:, k]
    return acc


def row_op(G, x, init, neg, finish, extra_abs, c_epi, factor=None, square=False):
    """One epilogue over the rows of G.  finish(acc, cast) is the epilogue's expression after the sum, written once and
    evaluated in double and in long double (cast converts its inputs); extra_abs the |further addends| per row; factor the
    multiplier of the result, if any; square: prod = (v*x)*v (ProdSquareWeighted) instead of x*v (ProdMul)."""
    x = np.asarray(x, np.float64)
    xg, v = x[G.idx], G.val
    prod = (v * xg) * v if square else xg * v                            # rounded products
    xl_, vl_ = xg.astype(LD), v.astype(LD)
    prod_ld = (vl_ * xl_) * vl_ if square else xl_ * vl_
    init = np.zeros(G.nrows) if init is None else np.asarray(init, np.float64)
    P, Pl = _padded(G, prod, np.float64), _padded(G, prod_ld, LD)
    f64 = lambda a: np.asarray(a, np.float64)
    fld = lambda a: np.asarray(a, np.float64).astype(LD)
    seq = finish(_fold(P, init, neg, "sequential"), f64)
    alt = {o: finish(_fold(P, init, neg, o), f64) for o in ("reversed", "pairwise")}
    ld = finish(_fold(Pl, init.astype(LD), neg, "pairwise"), fld)
    S = np.abs(init).astype(LD) + np.abs(Pl).sum(axis=1) + np.asarray(extra_abs, np.float64).astype(LD)
    if factor is not None:
        S = S * np.abs(np.asarray(factor, np.float64)).astype(LD)
    gate = (G.len + c_epi + 2) * LD(U) * S
    return Op(ld, seq, alt, gate, G.len)


# ---- the epilogues ------------------------------------------------------------------------------------------------------
def diagonal(A, W):
    """EpiDiagonal: out[i] = W[n+i] + sum_j (a_ij * W[j]) * a_ij.  c_epi = 0 (finish stores the sum); the product has two
    roundings, the second of which the gate's spare u covers."""
    n = A.ncol
    return row_op(arows(A), W[:n], W[n:], False, lambda acc, c: acc, 0.0, 0, square=True)


def recover_x(A, W, a, y):
    """EpiRecoverX: x[j] = W[j] * (a[j] - A_j'y).  c_epi = 2 (one subtraction, one multiplication)."""
    n = A.ncol
    return row_op(acols(A), y, None, False, lambda acc, c: c(W[:n]) * (c(a[:n]) - acc), np.abs(a[:n]), 2, factor=W[:n])


def residual_rows(A, b, xs):
    """EpiResidualRows (kNeg): out[i] = b[i] - sum_j a_ij xs[j].  c_epi = 0."""
    return row_op(arows(A), xs, b, True, lambda acc, c: acc, 0.0, 0)


def iter_rb(A, b, x):
    """EpiIterRb (kNeg), and EpiIterRbPart followed by subtract_slack_kernel: rb[i] = (b[i] - sum_j a_ij x[j]) - x[n+i].
    c_epi = 1 (the slack subtraction)."""
    n = A.ncol
    return row_op(arows(A), x[:n], b, True, lambda acc, c: acc - c(x[n:]), np.abs(x[n:]), 1)


def iter_rc(A, c, zl, zu, y, state, postprocessed):
    """EpiIterRc: rc[j] = ((c[j] - zl[j]) + zu[j]) - A_j'y, exactly 0 on FIXED variables unless the iterate is
    postprocessed.  c_epi = 3 (two operations on c, zl, zu and the subtraction of the sum)."""
    n = A.ncol
    zero = (np.asarray(state[:n]) == FIXED) & (not postprocessed)

    def finish(acc, cast):
        return np.where(zero, cast(0.0), ((cast(c[:n]) - cast(zl[:n])) + cast(zu[:n])) - acc)
    op = row_op(acols(A), y, None, False, finish, np.abs(c[:n]) + np.abs(zl[:n]) + np.abs(zu[:n]), 3)
    op.gate = np.where(zero, LD(0.0), op.gate)
    return op


def newton_shift(A, rc, dzl, dzu, xl, xu, zl, zu, state, dy):
    """EpiNewtonShift (newton.hip, newton_shift): on a barrier variable j either dzl[j] = (rc[j] + dzu[j]) - A_j'dy (the
    lower side, chosen by zl*xu >= zu*xl when both bounds are finite) or dzu[j] = (-rc[j] + dzl[j]) + A_j'dy; the other
    of the two is not touched, so the returned one is the reference's input.  c_epi = 2.  Returns (lower, upper, Op for
    dzl where lower, Op for dzu where upper); the entries outside their mask are meaningless."""
    n = A.ncol
    st = np.asarray(state[:n])
    barrier = st >= LB
    fl, fu = np.isfinite(xl[:n]), np.isfinite(xu[:n])
    with np.errstate(invalid="ignore"):
        lower = np.where(fl & fu, zl[:n] * xu[:n] >= zu[:n] * xl[:n], fl) & barrier
    upper = barrier & ~lower
    G = acols(A)
    lo = row_op(G, dy, None, False, lambda acc, c: (c(rc[:n]) + c(dzu[:n])) - acc, np.abs(rc[:n]) + np.abs(dzu[:n]), 2)
    up = row_op(G, dy, None, False, lambda acc, c: (-c(rc[:n]) + c(dzl[:n])) + acc, np.abs(rc[:n]) + np.abs(dzl[:n]), 2)
    return lower, upper, lo, up


def basis_columns(A, scale2, a, y):
    """EpiBasisColumns: x[j] = (a[j] - A_j'y) * scale2[j] where scale2[j] != 0, else exactly 0 (scale2 = colscale^2 on
    NONBASIC columns, 0 elsewhere).  c_epi = 2."""
    n = A.ncol
    s = np.asarray(scale2[:n], np.float64)

    def finish(acc, cast):
        return np.where(s != 0.0, (cast(a[:n]) - acc) * cast(s), cast(0.0))
    return row_op(acols(A), y, None, False, finish, np.abs(a[:n]), 2, factor=s)


class Dot:
    def __init__(self, ld, seq, gate):
        self.ld, self.seq, self.gate = ld, seq, gate


def obj_fixed(A, y, x, state):
    """EpiObjFixed: the dot output sum over FIXED structural j of x[j] * (A_j'y).  Per contribution one multiplication
    after the row sum (c_epi = 1); gate = (number of rows + longest row + 1 + 2) u S, S = sum_j |x_j| sum_i |a_ij y_i|.
    seq adds the contributions in row order (the oracle's order)."""
    n = A.ncol
    G = acols(A)
    fixed = np.asarray(state[:n]) == FIXED
    rows = row_op(G, y, None, False, lambda acc, c: np.where(fixed, c(x[:n]) * acc, c(0.0)), 0.0, 1, factor=x[:n])
    seq = 0.0
    for v in rows.seq[fixed]:
        seq += v
    ld = rows.ld[fixed].sum(dtype=LD)
    S = (rows.gate / ((G.len + 3) * LD(U)))[fixed].sum(dtype=LD)
    longest = int(G.len.max()) if G.len.size else 0
    return Dot(ld, seq, (G.nrows + longest + 1 + 2) * LD(U) * S)


def normal_matrix_residual(A, W, a, b, y):
    """EpiKktRhs is internal (v_rhs); what a converged solve shows of it: the long-double rhs = (-b + A (W a)_s) + W_I a_I
    and (A W_s A' + W_I) y.  Returns (rhs, product)."""
    n = A.ncol
    Gr, Gc = arows(A), acols(A)
    Wl, al, yl = np.asarray(W, np.float64).astype(LD), np.asarray(a, np.float64).astype(LD), np.asarray(y, np.float64).astype(LD)

    def rows_times(G, x):
        return _padded(G, x[G.idx] * G.val.astype(LD), LD).sum(axis=1)
    rhs = (-np.asarray(b, np.float64).astype(LD) + rows_times(Gr, Wl[:n] * al[:n])) + Wl[n:] * al[n:]
    t = Wl[:n] * rows_times(Gc, yl)
    return rhs, rows_times(Gr, t) + Wl[n:] * yl


# ---- models --------------------------------------------------------------------------------------------------------------
def initial_states(lb, ub):
    """Iterate::Initialize (reference src/iterate.cc:76-88); lb == ub gives BARRIER_BOXED"""
    st = np.full(len(lb), BOXED, np.uint8)
    st[np.isinf(lb) & np.isinf(ub)] = FREE
    st[np.isfinite(lb) & np.isinf(ub)] = LB
    st[np.isinf(lb) & np.isfinite(ub)] = UB
    return st


def iterate_for(lb, ub, n, seed):
    """an iterate with all five states: barrier variables by their bounds, two thirds of the lb == ub structurals and a
    third of the free ones FIXED (all four bound vectors 0), a quarter of the '=' slacks FIXED"""
    rng = np.random.default_rng(seed)
    N, m = len(lb), len(lb) - n
    hl, hu = np.isfinite(lb), np.isfinite(ub)
    state = initial_states(lb, ub)
    it = dict(x=rng.uniform(-2.0, 2.0, N), y=rng.uniform(-1.0, 1.0, m))
    it["xl"] = np.where(hl, 10.0 ** rng.uniform(-2, 1, N), np.inf)
    it["xu"] = np.where(hu, 10.0 ** rng.uniform(-2, 1, N), np.inf)
    it["zl"] = np.where(hl, 10.0 ** rng.uniform(-2, 1, N), 0.0)
    it["zu"] = np.where(hu, 10.0 ** rng.uniform(-2, 1, N), 0.0)
    u = rng.random(N)
    eq, slack = lb == ub, np.arange(N) >= n
    fixed = (eq & ~slack & (u < 0.67)) | (eq & slack & (u < 0.25)) | ((state == FREE) & ~slack & (u < 0.33))
    state[fixed] = FIXED
    for k in ("xl", "xu", "zl", "zu"):
        it[k][fixed] = 0.0
    return it, state


def newton_inputs(state, it, seed):
    """residuals and complementarity targets for newton_solve on the iterate's states (synth.synthetic_newton_state's
    rules): rl, sl on variables with a lower bound, ru, su on those with an upper one, 0 elsewhere"""
    rng = np.random.default_rng(seed)
    N = state.size
    m = it["y"].size
    lbm, ubm = (state == LB) | (state == BOXED), (state == UB) | (state == BOXED)
    nb = int(lbm.sum() + ubm.sum())
    mu = float((it["xl"][lbm] * it["zl"][lbm]).sum() + (it["xu"][ubm] * it["zu"][ubm]).sum()) / max(nb, 1)
    V = lambda k: rng.uniform(-0.5, 0.5, k)
    return dict(rb=V(m), rc=V(N), rl=np.where(lbm, V(N), 0.0), ru=np.where(ubm, V(N), 0.0),
                sl=np.where(lbm, mu - synth.xl_safe(it["xl"]) * it["zl"], 0.0),
                su=np.where(ubm, mu - synth.xl_safe(it["xu"]) * it["zu"], 0.0), mu=mu)


EMPTY_ROW, LONG_ROW, EMPTY_COL = 41, 7, 699
DENSE_COLS = (0, 1, 2)


def with_long_rows(A, seed):
    """Columns 0, 1, 2 hold every row but EMPTY_ROW (299 entries: long rows of the column gather), row LONG_ROW holds 320
    columns (a long row of the row gather), row EMPTY_ROW and column EMPTY_COL hold nothing."""
    m, n = A.nrow, A.ncol
    rng = np.random.default_rng(seed)
    D = np.zeros((m, n))
    D[A.i, np.repeat(np.arange(n), np.diff(A.p))] = A.x
    vals = lambda k: rng.choice([-1.0, 1.0], k) * rng.uniform(0.5, 4.0, k)
    for j in DENSE_COLS:
        D[:, j] = vals(m)
    D[LONG_ROW, 10:330] = vals(320)
    D[EMPTY_ROW, :] = 0.0
    D[:, EMPTY_COL] = 0.0
    cols, rows = np.nonzero(D.T)                                # column-major: ascending rows within a column
    p = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))])
    return synth.CscMatrix(m, n, p, rows, D[rows, cols])


def model(name):
    """dict(A, b, c, lb, ub, it, state): "mixed" 300 x 700, "square" 256 x 512, "wide" 1024 x 2100 and "long", the first
    with long rows in both gather matrices, an empty row and an empty column, and dense columns 0 and 1 FIXED"""
    m, n, seed = {"mixed": (300, 700, 11), "square": (256, 512, 12), "wide": (1024, 2100, 13), "long": (300, 700, 11)}[name]
    A, b, c, lb, ub, _ = synth.mixed_bounds_lp(m, n, seed)
    if name == "long":
        A = with_long_rows(A, seed + 5)
        lb, ub = lb.copy(), ub.copy()
        lb[0] = ub[0] = 0.75
        lb[1] = ub[1] = -1.25
        lb[2], ub[2] = 0.0, np.inf
    it, state = iterate_for(lb, ub, n, seed + 1)
    if name == "long":
        state[:2] = FIXED
        for k in ("xl", "xu", "zl", "zu"):
            it[k][:2] = 0.0
    assert set(np.unique(state).tolist()) == {FIXED, FREE, LB, UB, BOXED}
    assert (state[:n] == FIXED).any() and (state[n:] == FIXED).any()
    return dict(name=name, A=A, m=m, n=n, b=b, c=c, lb=lb, ub=ub, it=it, state=state)


BANDED = (520, 1100, 64, 14)            # m, n, band, seed


def any_model(name):
    return banded_model(*BANDED) if name == "banded" else model(name)


MODELS = ("mixed", "square", "wide", "long", "banded")


def banded_model(m, n, band, seed):
    """synth.banded_lp with the bounds, vectors and iterate of a mixed model of the same size (gathers with locality: what the
    fused sorted and fused accumulated tiles are built for)"""
    _, b, c, lb, ub, _ = synth.mixed_bounds_lp(m, n, seed)
    A = synth.banded_lp(m, n, 8, band, seed)
    it, state = iterate_for(lb, ub, n, seed + 1)
    return dict(name="banded", A=A, m=m, n=n, b=b, c=c, lb=lb, ub=ub, it=it, state=state)


def objective_inputs(M):
    """(b, lb, ub, iterate) with which dobjective is EpiObjFixed's dot alone: dobjective = b'y + sum lb zl - sum ub zu
    - sum over FIXED slacks of x y - sum over FIXED structurals of x_j A_j'y (iterate.cc:627-638), so b = lb = ub = 0 and
    x = 0 on the FIXED slacks leave exactly -(the dot), every other term being an exact zero"""
    N, n = M["state"].size, M["n"]
    it = {k: v.copy() for k, v in M["it"].items()}
    it["x"][n:][M["state"][n:] == FIXED] = 0.0
    return np.zeros(M["m"]), np.zeros(N), np.zeros(N), it


def barrier_weights(it, state):
    """xl, xu, zl, zu for kkt_diag_factorize from an iterate.  The diag solver forms g = zl/xl + zu/xu for every variable
    and regularizes g = 0 by mu (kkt_solver_diag.cc:44-56): FIXED variables (all four vectors 0) get xl = xu = inf so that
    they take that branch like the FREE ones, not 0/0."""
    xl, xu = np.where(state == FIXED, np.inf, it["xl"]), np.where(state == FIXED, np.inf, it["xu"])
    return xl, xu, it["zl"], it["zu"]
