"""CPU: the long-double restatement of the dense-column preconditioner (tests/smw_reference.py) against the oracle.

Two jobs.  The cross-check guards against the restatement and the oracle sharing a misreading of
src/diagonal_precond.cc, and it measures the error of plain double-precision arithmetic on the models of
tests/test_gpu_smw_dense.py: the table ORACLE_ERR there (from which the device's gates follow) is this test's
measurement, and this test fails when the table no longer is.  The classification edges hold dense_columns to
oracle.find_dense_columns where a column count sits exactly on the threshold."""
import numpy as np
import pytest

import smw_reference as R
from ipx_amd import synth

EPS = float(np.finfo(np.float64).eps)


def ocsc(A):
    from oracle import pyoracle as po
    return po.Csc(A.nrow, A.ncol, A.p, A.i, A.x)


def oracle_errors(oracle, name):
    """the oracle's normwise errors (factor, lhs, dot) against the long-double reference, after checking that both
    mean the same thing"""
    A, W, rhs = R.model(name)
    ref = R.reference(name)
    nd, nzd = oracle.find_dense_columns(ocsc(A))
    assert nd == ref["dense"].size == R.SHAPES[name][2]
    P, err = oracle.diag_factorize(ocsc(A), W, nzd, True)
    assert err == 0 and P.num_dense == nd
    d, f = P.get()
    lhs, dot = P.apply(rhs)
    # a row of E is a sum of positive terms, one per entry of the row and the slack weight
    assert R.normwise(d, ref["E"]) <= (int(np.bincount(A.i, minlength=A.nrow).max()) + 2) * EPS
    return R.normwise(np.tril(f), ref["L"]), R.normwise(lhs, ref["lhs"]), abs(float((dot - ref["dot"]) / ref["dot"]))


@pytest.mark.parametrize("name", R.FACTOR_MODELS)
def test_oracle_against_long_double(oracle, name):
    import test_gpu_smw_dense as G
    assert np.finfo(R.LD).eps < 1e-18, "np.longdouble is no wider than double here: nothing is measured"
    ef, el, ed = oracle_errors(oracle, name)
    print("%-10s factor %.2e  lhs %.2e  dot %.2e" % (name, ef, el, ed))
    # a shared misreading would show as an error of the size of the entries.  The bound: an entry of S is a sum of up
    # to m terms and a factor's column one of up to k more, each rounded once, and the factor and the solves magnify
    # a perturbation of S by cond(S) at the worst (<= 3.7e4 on these models); lhs goes through the factor four times.
    m, _, k = R.SHAPES[name]
    bound = (m + k) * EPS * np.linalg.cond(R.reference(name)["S"].astype(np.float64))
    assert ef <= bound and el <= 4 * bound and ed <= 4 * bound
    # the table the device's gates are computed from is this measurement (three digits)
    for got, rec in zip((ef, el, ed), G.ORACLE_ERR[name]):
        assert abs(got - rec) <= 0.01 * rec + 1e-19, (name, (ef, el, ed), G.ORACLE_ERR[name])


def test_restatement_pieces():
    """S = L L' and the solve's residual in long double, the failing pivot's index, and no dense columns"""
    ref = R.reference("k129")
    L, S = ref["L"], ref["S"]
    assert R.normwise(L @ L.T, S) <= 1e-17
    A, W, rhs = R.model("k129")
    Ad = R._dense_matrix(A)[:, ref["dense"]]
    w = W.astype(R.LD)
    P = np.diag(ref["E"]) + (Ad * w[ref["dense"]]) @ Ad.T     # E + Ad Wd Ad'
    assert R.normwise(P @ ref["lhs"], rhs) <= 1e-15
    for j in (0, 31, 128):
        for bad in (-1e-30, np.nan):
            Wb = W.copy()
            Wb[ref["dense"][j]] = bad
            E, _, Lb, info = R.factorize(A, Wb, ref["dense"])
            assert info == j + 1 and np.array_equal(E, ref["E"]) and np.array_equal(Lb[:, :j], L[:, :j])
    A, W, rhs = R.model("k1001")
    none = R.dense_columns(A.p, A.ncol)
    assert none.size == 0
    lhs, dot = R.apply(A, W, none, rhs)
    S = A.to_scipy()
    diag = W[A.ncol:] + (S.multiply(S)) @ W[:A.ncol]
    assert R.normwise(lhs, rhs / diag) <= 8 * EPS


def counts_model(counts, m):
    counts = np.asarray(counts, dtype=np.int64)
    p = np.concatenate([[0], np.cumsum(counts)])
    i = np.concatenate([np.arange(c, dtype=np.int64) for c in counts])
    return synth.CscMatrix(m, counts.size, p, i, np.ones(int(p[-1])))


EDGES = {
    # next to columns of 8 the threshold is 80
    "80_next_to_8": ([8] * 50 + [80] * 3, 0),
    "81_next_to_8": ([8] * 50 + [81] * 3, 3),
    "80_and_81": ([8] * 50 + [80, 81, 81], 0),               # 81 follows 80: no jump of a factor 10
    # next to columns of 1 to 4 the threshold is 40
    "40_next_to_1to4": ([1, 2, 3, 4] * 10 + [40] * 2, 0),
    "41_next_to_1to4": ([1, 2, 3, 4] * 10 + [41] * 2, 2),
    "41_first_among_longer": ([41, 300] + [1, 2, 3, 4] * 10 + [41], 3),
    "1000_long": ([8] * 30 + [100] * 1000, 1000),
    "1001_long": ([8] * 30 + [100] * 1001, 0),
    "all_equal": ([8] * 30, 0),
    "one_column": ([200], 0),
}


@pytest.mark.parametrize("case", sorted(EDGES))
def test_classification_edges(oracle, case):
    counts, want = EDGES[case]
    counts = np.random.default_rng(5).permutation(counts)          # the rule sorts; the order as given is arbitrary
    A = counts_model(counts, 300)
    mine = R.dense_columns(A.p, A.ncol)
    nd, nzd = oracle.find_dense_columns(ocsc(A))
    assert mine.size == nd == want
    assert np.array_equal(mine, np.nonzero(counts >= nzd)[0])
