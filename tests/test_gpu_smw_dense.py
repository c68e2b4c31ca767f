"""GPU: the dense-column (Sherman-Morrison-Woodbury) preconditioner of ipx_amd/csrc/precond.hip at its kernel
boundaries, held to the long-double restatement of tests/smw_reference.py.

Which kernels run depends on the number k of dense columns alone, so k sits on every boundary: 1 and 2; 63, 64, 65
(one wavefront / the blocked family, a second 64-row block of one row); 96, 97 (a last panel of 32 columns without a
trailing update / of one column); 128, 129; 1000 (the most the classification allows) and 1001 (none).  The models
have m = 300 rows: no multiple of the 32-row chunk of schur_gemm_kernel, one slab.  m1000_k65 has three slabs, the
last one ragged -- from diag_factorize_dev: nt = ceil(65 / 64) = 2 tiles, ntri = 3, nslabs = min(256, 2048 / 3) = 256,
then min(256, max(1, 1000 / 256)) = 3; rows per slab = ceil(ceil(1000 / 3) / 32) * 32 = 352; ceil(1000 / 352) = 3 slabs
of 352, 352 and 296 rows, 296 = 9 chunks and 8 rows.  The ladder model has dense columns of 81 entries (one above
the threshold next to columns of eight) up to full columns.

ORACLE_ERR is the oracle's normwise error (max |difference| / max |reference|) against long double for the factor,
lhs and rhs . lhs, as tests/test_smw_reference.py measures it (and checks that this table is what it measures): the
error of plain double arithmetic on these inputs.  The device gets 8 times that and never less than 16 eps; the 8
covers its other order of summation (Schur entries by slab, tile and 4 x 4 block, 16-lane partials in
potrs_blocked_kernel) and the compiler's contraction into fused multiply-adds.  No gate comes from a device result.

    model      oracle: factor, lhs, dot   | gates: factor, lhs, dot      | device (MI355X, one run): factor, lhs, dot
    k1         6.80e-17 2.80e-17 6.43e-16 | 3.55e-15 3.55e-15 5.14e-15 | 6.80e-17 2.80e-17 4.87e-17
    k2         2.14e-16 2.48e-16 9.97e-17 | 3.55e-15 3.55e-15 3.55e-15 | 2.14e-16 2.48e-16 9.97e-17
    k5         7.74e-17 1.24e-16 3.77e-16 | 3.55e-15 3.55e-15 3.55e-15 | 7.74e-17 1.24e-16 1.03e-16
    k40        1.82e-16 3.36e-16 2.22e-16 | 3.55e-15 3.55e-15 3.55e-15 | 1.82e-16 4.45e-16 4.26e-17
    k63        2.28e-16 2.76e-16 7.29e-16 | 3.55e-15 3.55e-15 5.83e-15 | 2.28e-16 4.57e-16 1.00e-16
    k64        4.11e-16 4.15e-16 3.57e-16 | 3.55e-15 3.55e-15 3.55e-15 | 4.11e-16 3.23e-16 2.97e-16
    k65        2.11e-16 3.01e-16 4.26e-16 | 3.55e-15 3.55e-15 3.55e-15 | 2.11e-16 3.01e-16 5.68e-17
    k96        3.25e-16 1.48e-15 1.53e-16 | 3.55e-15 1.18e-14 3.55e-15 | 3.25e-16 9.70e-16 1.97e-17
    k97        1.90e-16 5.01e-16 2.44e-16 | 3.55e-15 4.01e-15 3.55e-15 | 1.90e-16 9.82e-16 2.44e-16
    k128       5.12e-16 7.70e-16 2.27e-16 | 4.10e-15 6.16e-15 3.55e-15 | 5.12e-16 5.63e-16 1.81e-16
    k129       7.07e-16 1.89e-15 5.33e-16 | 5.66e-15 1.51e-14 4.26e-15 | 7.07e-16 7.20e-16 4.27e-17
    m1000_k65  2.79e-15 1.55e-14 5.96e-16 | 2.23e-14 1.24e-13 4.77e-15 | 8.38e-16 4.94e-15 7.67e-16
    k1000      1.02e-15 3.55e-13 2.44e-15 | 8.16e-15 2.84e-12 1.95e-14 | 1.21e-15 1.66e-13 2.15e-15
    ladder     2.36e-16 9.99e-16 2.86e-16 | 3.55e-15 7.99e-15 3.55e-15 | 2.36e-16 5.38e-16 1.41e-16

The device's factor error equals the oracle's on most models: both kernel families give an entry its products one at a
time in ascending order, the oracle's arithmetic, and the Schur entries differ only where slabs or tiles split a sum.
With IPXK_SCHUR_BLOCKED=0 the factor of k2 and k65 is bit for bit the blocked form's, the ladder's within 9.0e-17.
"""
import numpy as np
import pytest

import smw_reference as R

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)

# name -> the oracle's error of (factor, lhs, dot), three digits
ORACLE_ERR = {
    "k1": (6.80e-17, 2.80e-17, 6.43e-16),
    "k2": (2.14e-16, 2.48e-16, 9.97e-17),
    "k5": (7.74e-17, 1.24e-16, 3.77e-16),
    "k40": (1.82e-16, 3.36e-16, 2.22e-16),
    "k63": (2.28e-16, 2.76e-16, 7.29e-16),
    "k64": (4.11e-16, 4.15e-16, 3.57e-16),
    "k65": (2.11e-16, 3.01e-16, 4.26e-16),
    "k96": (3.25e-16, 1.48e-15, 1.53e-16),
    "k97": (1.90e-16, 5.01e-16, 2.44e-16),
    "k128": (5.12e-16, 7.70e-16, 2.27e-16),
    "k129": (7.07e-16, 1.89e-15, 5.33e-16),
    "m1000_k65": (2.79e-15, 1.55e-14, 5.96e-16),
    "k1000": (1.02e-15, 3.55e-13, 2.44e-15),
    "ladder": (2.36e-16, 9.99e-16, 2.86e-16),
}


def gates(name):
    return tuple(max(8.0 * e, 16.0 * EPS) for e in ORACLE_ERR[name])


@pytest.fixture(scope="module")
def kkt():
    from ipx_amd import kkt as K
    K.load_library()
    return K


def ocsc(A):
    from oracle import pyoracle as po
    return po.Csc(A.nrow, A.ncol, A.p, A.i, A.x)


def relerr(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def sum_bound(A):
    """a row of the diagonal is a sum of positive terms, one per entry of the row and the slack weight: in whatever
    order, its relative error is at most (number of terms + 1) eps (a product's rounding and the additions)"""
    return (int(np.bincount(A.i, minlength=A.nrow).max()) + 2) * EPS


MAX_ROW_LEN = 255     # kMaxRowLen of ipx_amd/csrc/internal.hpp: a longer row leaves the layout for the long-row kernels


def check_diagonal(ctx, A, d, d_oracle):
    """bit for bit the oracle's where the row gather of A is in the phased layout (ascending columns; as
    tests/test_gpu_parity.py::test_fused_layout_random_shapes demands), else 1e-14.  Rows of more than MAX_ROW_LEN
    entries (k1000 and k1001 have about 390 per row) are not in that layout: the long-row kernels sum them in
    segments, so they are held to 1e-14 like the other layouts."""
    short = np.bincount(A.i, minlength=A.nrow) <= MAX_ROW_LEN
    if ctx.spmv_layout()[0][1] == "phased":
        assert np.array_equal(d[short], d_oracle[short])
    assert relerr(d, d_oracle) <= 1e-14


def check_against_reference(ctx, oracle, name, tag):
    """Factorize, the factor and one Apply on a fresh context of model `name` against the long-double reference;
    returns (diagonal, factor, lhs, dot)"""
    A, W, rhs = R.model(name)
    ref = R.reference(name)
    k = ref["dense"].size
    gf, gl, gd = gates(name)
    assert ctx.num_dense_cols == k
    assert ctx.diag_factorize(W, True) == 0
    d, f = ctx.diag_get(k)
    nd, nzd = oracle.find_dense_columns(ocsc(A))
    P, err = oracle.diag_factorize(ocsc(A), W, nzd, True)
    assert nd == k and err == 0
    lhs, dot = ctx.diag_apply(rhs)
    ef, el = R.normwise(np.tril(f), ref["L"]), R.normwise(lhs, ref["lhs"])
    ed = abs(float((dot - ref["dot"]) / ref["dot"]))
    row = np.abs(lhs - ref["lhs"]) / (np.abs(rhs) / ref["E"] + np.abs(ref["lhs"]).max())
    print("%s %-10s factor %.2e (gate %.2e)  lhs %.2e (%.2e)  dot %.2e (%.2e)  worst row %.2e" %
          (tag, name, ef, gf, el, gl, ed, gd, float(row.max())))
    check_diagonal(ctx, A, d, P.get()[0])
    assert ef <= gf
    assert el <= gl and ed <= gd
    assert float(row.max()) <= gl, int(np.argmax(row))       # a single wrong row cannot hide behind the largest one
    return d, f, lhs, dot


_clean = {}


def clean_result(kkt, name):
    """(diagonal, factor, lhs, dot) of a context of model `name` that did nothing but Factorize and Apply"""
    if name not in _clean:
        A, W, rhs = R.model(name)
        k = R.reference(name)["dense"].size
        ctx = kkt.KktContext(A)
        assert ctx.diag_factorize(W, True) == 0
        _clean[name] = ctx.diag_get(k) + ctx.diag_apply(rhs)
        ctx.close()
    return _clean[name]


def same_as_clean(kkt, ctx, name):
    """diagonal, factor and lhs of `ctx` (factorized) are bit for bit those of a context that did nothing else.  Not the
    dot: the layout of the m short rows of Ad is chosen by timing per context, and its block partials differ between
    layouts (build_dense_structures), so the dot is held to the reference like any other."""
    A, W, rhs = R.model(name)
    ref = R.reference(name)
    d0, f0, lhs0, _ = clean_result(kkt, name)
    d, f = ctx.diag_get(ref["dense"].size)
    lhs, dot = ctx.diag_apply(rhs)
    assert np.array_equal(d, d0) and np.array_equal(f, f0) and np.array_equal(lhs, lhs0)
    assert abs(float((dot - ref["dot"]) / ref["dot"])) <= gates(name)[2]


# --------------------------------------------------------------------------------------
# every model, blocked Schur complement
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FACTOR_MODELS)
def test_factor_and_apply_against_long_double(kkt, oracle, monkeypatch, name):
    monkeypatch.delenv("IPXK_SCHUR_BLOCKED", raising=False)
    ctx = kkt.KktContext(R.model(name)[0])
    check_against_reference(ctx, oracle, name, "blocked")
    ctx.close()


# --------------------------------------------------------------------------------------
# the Schur complement one column at a time (what a model with m * k above 2^30 takes)
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k2", "k65", "ladder"])
def test_unblocked_schur_complement(kkt, oracle, monkeypatch, name):
    monkeypatch.delenv("IPXK_SCHUR_BLOCKED", raising=False)
    f_blocked = clean_result(kkt, name)[1]
    monkeypatch.setenv("IPXK_SCHUR_BLOCKED", "0")            # read at every Factorize
    ctx = kkt.KktContext(R.model(name)[0])
    f = check_against_reference(ctx, oracle, name, "unblocked")[1]
    ctx.close()
    diff = relerr(np.tril(f), np.tril(f_blocked))
    print("unblocked %-10s factor against the blocked form %.2e" % (name, diff))
    assert diff <= 1e-13


# --------------------------------------------------------------------------------------
# precond_dense_cols = False, then True on the same context
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k5", "k65"])
def test_without_dense_column_treatment_then_with(kkt, oracle, monkeypatch, name):
    monkeypatch.delenv("IPXK_SCHUR_BLOCKED", raising=False)
    A, W, rhs = R.model(name)
    ref = R.reference(name)
    k, n = ref["dense"].size, A.ncol
    ctx = kkt.KktContext(A)
    assert ctx.num_dense_cols == k
    assert ctx.diag_factorize(W, False) == 0
    d = ctx.diag_get()[0]
    P, err = oracle.diag_factorize(ocsc(A), W, oracle.find_dense_columns(ocsc(A))[1], False)
    assert err == 0 and P.num_dense == 0
    check_diagonal(ctx, A, d, P.get()[0])
    # the diagonal now includes the dense columns
    Ad = R._dense_matrix(A)[:, ref["dense"]]
    full = ref["E"] + (Ad * Ad) @ W[:n].astype(R.LD)[ref["dense"]]
    assert R.normwise(d, full) <= sum_bound(A) and R.normwise(d, ref["E"]) > 0.1
    lhs, dot = ctx.diag_apply(rhs)
    assert np.array_equal(lhs, rhs / d)
    exact = float((rhs.astype(R.LD) * lhs.astype(R.LD)).sum())
    assert abs(dot - exact) <= A.nrow * EPS * exact          # a sum of m positive terms, in whatever order
    assert ctx.diag_factorize(W, True) == 0
    same_as_clean(kkt, ctx, name)
    ctx.close()


# --------------------------------------------------------------------------------------
# Cholesky failure: errflag 401, the context unfactorized but reusable
# --------------------------------------------------------------------------------------
# k = 40: one workgroup (cholesky_lower_kernel), first and last column.  k = 129: panels of 32 -- the first column, both
# sides of a panel edge, a column after three trailing updates, the last panel of one column.
FAILURES = [("k40", j, -1e-30) for j in (0, 39)] + [("k129", j, -1e-30) for j in (0, 31, 32, 100, 128)] + \
           [("k40", 0, np.nan), ("k129", 32, np.nan)]


@pytest.mark.parametrize("name,j,bad", FAILURES)
def test_cholesky_failure_leaves_the_context_reusable(kkt, oracle, monkeypatch, name, j, bad):
    """W of dense column j negative (S_jj about -1e30) or NaN: no earlier pivot changes, the dense weights being
    masked out of E, so the first failing pivot is j + 1"""
    monkeypatch.delenv("IPXK_SCHUR_BLOCKED", raising=False)
    A, W, rhs = R.model(name)
    ref = R.reference(name)
    k = ref["dense"].size
    Wbad = W.copy()
    Wbad[ref["dense"][j]] = bad
    assert R.factorize(A, Wbad, ref["dense"])[3] == j + 1
    assert oracle.diag_factorize(ocsc(A), Wbad, oracle.find_dense_columns(ocsc(A))[1], True)[1] == 401
    ctx = kkt.KktContext(A)
    ctx.normal_prepare(W)
    for _ in range(2):                                       # on a fresh context, then on a factorized one
        assert ctx.diag_factorize(Wbad, True) == 401         # IPX_ERROR_lapack_chol
        with pytest.raises(kkt.KktError, match="not factorized"):
            ctx.diag_apply(rhs)
        with pytest.raises(kkt.KktError, match="not factorized"):
            ctx.pcr_solve(rhs, 1e-8, None, 50)
        with pytest.raises(kkt.KktError, match="not factorized"):
            ctx.diag_get(k)
        assert ctx.diag_factorize(W, True) == 0
        same_as_clean(kkt, ctx, name)
    ctx.close()


# --------------------------------------------------------------------------------------
# 1001 long columns: no dense columns at all
# --------------------------------------------------------------------------------------
def test_1001_long_columns_are_not_dense(kkt, oracle):
    A, W, rhs = R.model("k1001")
    assert R.dense_columns(A.p, A.ncol).size == 0 and oracle.find_dense_columns(ocsc(A))[0] == 0
    ctx = kkt.KktContext(A)
    assert ctx.num_dense_cols == 0
    assert ctx.diag_factorize(W, True) == 0
    d, f = ctx.diag_get(0)
    assert f.size == 0
    P, err = oracle.diag_factorize(ocsc(A), W, A.nrow + 1, True)
    assert err == 0 and P.num_dense == 0
    check_diagonal(ctx, A, d, P.get()[0])
    E = R.factorize(A, W, [])[0]                               # every column in the diagonal
    assert R.normwise(d, E) <= sum_bound(A)
    lhs, dot = ctx.diag_apply(rhs)
    assert np.array_equal(lhs, rhs / d)
    exact = float((rhs.astype(R.LD) * lhs.astype(R.LD)).sum())
    assert abs(dot - exact) <= A.nrow * EPS * exact
    ctx.close()
