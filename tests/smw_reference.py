"""The dense-column form of DiagonalPrecond (reference src/diagonal_precond.cc:17-159) restated in plain NumPy with
np.longdouble arithmetic, and the models on which tests/test_smw_reference.py (CPU) and tests/test_gpu_smw_dense.py
(GPU) compare the oracle and the device with it.  No oracle, reference or product code is involved; importable
without a GPU.

    dense_columns(Ap, ncol)          the classification rule of src/model.cc:34-56
    factorize(A, W, dense)           E, S, the lower Cholesky factor of S, failing pivot (1-based) or 0
    apply(A, W, dense, rhs)          lhs = (inv(E) - inv(E) Ad inv(S) Ad' inv(E)) rhs and rhs . lhs

Everything is dense and vectorized (one matrix-vector product per Cholesky column), so the largest case the
classification allows, k = 1000 at m = 257, takes a few seconds."""
import numpy as np

from ipx_amd import synth

LD = np.longdouble


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def dense_columns(Ap, ncol):
    """Indices (ascending) of the dense columns: with the column counts sorted, the first count greater than
    max(40, 10 * the one before it) starts the dense columns; more than 1000 of them means none."""
    cnt = np.diff(np.asarray(Ap, dtype=np.int64)[:ncol + 1])
    srt = np.sort(cnt)
    jump = np.nonzero(srt[1:] > np.maximum(40, 10 * srt[:-1]))[0]
    if jump.size == 0 or ncol - (jump[0] + 1) > 1000:
        return np.zeros(0, dtype=np.int64)
    return np.nonzero(cnt >= srt[jump[0] + 1])[0].astype(np.int64)


def _dense_matrix(A):
    M = np.zeros((A.nrow, A.ncol), dtype=LD)
    M[A.i, np.repeat(np.arange(A.ncol), np.diff(A.p))] = A.x
    return M


def cholesky_lower(S):
    """Column by column: (L, info); the columns before the failing one are final, the rest are zero."""
    k = S.shape[0]
    L = np.zeros((k, k), dtype=LD)
    for j in range(k):
        v = S[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:                         # non-positive or NaN
            return L, j + 1
        L[j:, j] = v / np.sqrt(v[0])
    return L, 0


def factorize(A, W, dense):
    """E = W_slack + sum over the non-dense columns of W_j a_ij^2; S = Ad' inv(E) Ad + diag(1 / W_dense);
    S = L L'.  Returns (E, S, L, info), all long double."""
    m, n = A.nrow, A.ncol
    dense = np.asarray(dense, dtype=np.int64)
    M = _dense_matrix(A)
    w = np.asarray(W, dtype=np.float64).astype(LD)
    wcols = w[:n].copy()
    wcols[dense] = 0                             # left out of E whatever their weight is (negative, NaN)
    E = w[n:] + (M * M) @ wcols
    Ad = M[:, dense]
    S = Ad.T @ (Ad / E[:, None]) + np.diag(1 / w[dense])
    L, info = cholesky_lower(S)
    return E, S, L, info


def apply(A, W, dense, rhs, fact=None):
    """(lhs, rhs . lhs) in long double; fact: the result of factorize(A, W, dense), if at hand."""
    E, S, L, info = factorize(A, W, dense) if fact is None else fact
    assert info == 0
    dense = np.asarray(dense, dtype=np.int64)
    r = np.asarray(rhs, dtype=np.float64).astype(LD)
    if dense.size == 0:
        lhs = r / E
        return lhs, r @ lhs
    Ad = _dense_matrix(A)[:, dense]
    x = Ad.T @ (r / E)
    k = dense.size
    for j in range(k):                           # L z = b
        x[j] /= L[j, j]
        x[j + 1:] -= L[j + 1:, j] * x[j]
    for j in range(k - 1, -1, -1):               # L' x = z
        x[j] /= L[j, j]
        x[:j] -= L[j, :j] * x[j]
    lhs = (r - Ad @ x) / E
    return lhs, r @ lhs


# ------------------------------------------------------------------------------------------------
# the models
# ------------------------------------------------------------------------------------------------
SYNTH_K = (1, 2, 5, 40, 63, 64, 65, 96, 97, 128, 129)
# name -> (m, n, k): k dense columns of about 0.39 m entries in front of n - k columns of eight
SHAPES = {"k%d" % k: (300, 700 + k, k) for k in SYNTH_K}
SHAPES["m1000_k65"] = (1000, 765, 65)            # three slabs of rows in the blocked Schur complement
SHAPES["k1000"] = (257, 1300, 1000)              # the most dense columns the classification allows
SHAPES["k1001"] = (257, 1301, 0)                 # one more: no dense columns at all
SHAPES["ladder"] = (300, 770, 70)                # dense columns of 81 (the threshold + 1) up to m entries
FACTOR_MODELS = tuple(name for name in SHAPES if name != "k1001")
_cache = {}


def ladder_lp(m=300, nsparse=700, k=70, seed=99):
    """k dense columns whose lengths are spread evenly from 81 (one above 10 x 8) to m (a full column), in front of
    nsparse columns of eight entries"""
    rng = np.random.default_rng(seed)
    base = synth.synthetic_lp(m, nsparse, 8, seed)
    lens = np.rint(np.linspace(81, m, k)).astype(np.int64)
    ci = [np.sort(rng.choice(m, ln, replace=False)).astype(np.int64) for ln in lens]
    cx = [rng.uniform(0.5, 4.0, ln) * rng.choice([-1.0, 1.0], ln) for ln in lens]
    p = np.concatenate([[0], np.cumsum(lens), lens.sum() + base.p[1:]])
    return synth.CscMatrix(m, nsparse + k, p, np.concatenate(ci + [base.i]), np.concatenate(cx + [base.x]))


def model(name):
    """(A, W, rhs) of a named model; W = 10^U[-2,2], rhs standard normal, fixed seeds.  Shared, do not modify."""
    if name not in _cache:
        m, n, k = SHAPES[name]
        seed = 1000 + sorted(SHAPES).index(name)
        A = ladder_lp() if name == "ladder" else synth.synthetic_lp(m, n, 8, seed, num_dense=1001 if name == "k1001" else k)
        rng = np.random.default_rng(seed + 500)
        W = 10.0 ** rng.uniform(-2.0, 2.0, n + m)
        rhs = rng.standard_normal(m)
        for v in (A.p, A.i, A.x, W, rhs):
            v.setflags(write=False)
        _cache[name] = (A, W, rhs)
    return _cache[name]


def reference(name):
    """dict(dense, E, S, L, lhs, dot) of a named model in long double, computed once"""
    key = ("ref", name)
    if key not in _cache:
        A, W, rhs = model(name)
        dense = dense_columns(A.p, A.ncol)
        fact = factorize(A, W, dense)
        assert fact[3] == 0
        lhs, dot = apply(A, W, dense, rhs, fact)
        _cache[key] = dict(dense=dense, E=fact[0], S=fact[1], L=fact[2], lhs=lhs, dot=dot)
    return _cache[key]


def normwise(x, ref):
    """max |x - ref| / max |ref|, as a float"""
    x, ref = np.asarray(x, dtype=LD), np.asarray(ref, dtype=LD)
    return float(np.abs(x - ref).max() / np.abs(ref).max())
