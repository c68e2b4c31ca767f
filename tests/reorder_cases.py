"""The matrices, solve inputs and extended-precision answers shared by tests/test_reorder_reference.py (CPU) and
tests/test_gpu_reorder.py (GPU).  Inputs only: numpy, scipy and ipx_amd.synth; the answers come from
tests/reorder_reference.py and tests/cr_reference.py.  Everything is computed once per process and left unchanged.

Every matrix has at least 65 536 entries (below that GatherMatrix::build_device refuses and reorder_model discards the
numbering) and no dense column (dense columns switch the renumbering off)."""
import functools

import numpy as np
import scipy.sparse as sp

import cr_reference
import reorder_reference
from ipx_amd import synth

LD = np.longdouble
MIN_NNZ = 65536
LAYERS = (16, 17, 32)                   # row levels of the layered graphs: one batch of kBfsBatch, one more, two batches
SOLVE_CASES = ("banded", "many_components", "few_components")
NAMES = SOLVE_CASES + ("wide_frontier",) + tuple("layers%d" % L for L in LAYERS)
STATE_SEED = {"banded": 31, "many_components": 32, "few_components": 33}
MANY_SHUFFLE_SEED = 297                 # the first shuffle of the many-components matrix that leaves row 0 empty
SECOND_SEED = 41                        # the weights of the second factorize (banded case)


def from_scipy(M):
    M = sp.csc_matrix(M)
    M.sort_indices()
    return synth.CscMatrix(M.shape[0], M.shape[1], M.indptr, M.indices, M.data)


def blocks_with_empties(blocks, empty_rows, empty_cols, shuffle_seed):
    """the blocks on the diagonal, then rows and columns without an entry, then everything shuffled"""
    D = sp.block_diag([b.to_scipy() for b in blocks], format="csc")
    M = sp.csc_matrix((D.data, D.indices, np.concatenate([D.indptr, np.full(empty_cols, D.indptr[-1])])),
                      shape=(D.shape[0] + empty_rows, D.shape[1] + empty_cols))
    return synth.shuffled(from_scipy(M), shuffle_seed)[0]


def tree(shuffle_seed):
    """row 0 has 200 columns, each of those 20 new rows, each of those rows 20 new columns, each of those columns one
    new row: 84 001 x 80 200 with 164 200 entries.  From a leaf the search has 5 row levels, and its last row frontier
    and the column frontier before it hold 79 600 entries each: more than the 65 536 threads of a level's launch."""
    r1 = 1 + np.arange(4000)                                # children of the 200 columns of row 0
    c2 = 200 + np.arange(80000)                             # the 20 columns of each of those rows
    r2 = 4001 + np.arange(80000)                            # one leaf row per column
    rows = np.concatenate([np.zeros(200, dtype=np.int64), r1, np.repeat(r1, 20), r2])
    cols = np.concatenate([np.arange(200), np.repeat(np.arange(200), 20), c2, c2])
    vals = np.random.default_rng(3).uniform(0.5, 4.0, rows.size) * np.random.default_rng(4).choice([-1.0, 1.0], rows.size)
    return synth.shuffled(from_scipy(sp.csc_matrix((vals, (rows, cols)), shape=(84001, 80200))), shuffle_seed)[0]


LAYER_LINKS = 4


def layered(L, shuffle_seed):
    """rows in L layers of equal width w; every column joins two rows of adjacent layers: for each pair of layers and
    each of LAYER_LINKS random permutations p of 0..w-1, row i of the lower layer and row p[i] of the upper one.  A search
    reaches about 4^l rows of the layer l steps away, so from a row of an end layer it takes whole layers after a few
    levels and has exactly L row levels (tests/test_reorder_reference.py asserts that).  Rows have at most 8 entries and
    columns 2, which the device layout builders accept; w is the smallest width that gives MIN_NNZ entries."""
    k = LAYER_LINKS
    w = -(-MIN_NNZ // (2 * (L - 1) * k))
    rng = np.random.default_rng(100 + L)
    lower = np.concatenate([l * w + np.arange(w) for l in range(L - 1) for _ in range(k)])
    upper = np.concatenate([(l + 1) * w + rng.permutation(w) for l in range(L - 1) for _ in range(k)])
    ncol = lower.size
    rows = np.concatenate([lower, upper])
    cols = np.concatenate([np.arange(ncol), np.arange(ncol)])
    vals = rng.uniform(0.5, 4.0, rows.size) * rng.choice([-1.0, 1.0], rows.size)
    return synth.shuffled(from_scipy(sp.csc_matrix((vals, (rows, cols)), shape=(L * w, ncol))), shuffle_seed)[0]


@functools.lru_cache(maxsize=None)
def matrix(name):
    if name == "banded":
        return synth.shuffled(synth.banded_lp(4200, 8400, 8, 128, 5), 6)[0]
    if name == "many_components":       # 70 components, 6 more than the cap; row 0 is empty
        return blocks_with_empties([synth.banded_lp(64, 128, 8, 16, 7 + b) for b in range(70)], 37, 53, MANY_SHUFFLE_SEED)
    if name == "few_components":
        return blocks_with_empties([synth.banded_lp(900, 1800, 8, 64, 8 + b) for b in range(5)], 3, 5, 8)
    if name == "wide_frontier":
        return tree(9)
    if name.startswith("layers"):
        return layered(int(name[6:]), 10)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expander():
    """the uniformly random LP of test_expander_is_left_alone: above the size from which an unforced renumbering is looked for"""
    return synth.synthetic_lp(150000, 300000, 8, 7)


@functools.lru_cache(maxsize=None)
def numbering(name, force=True):
    A = matrix(name)
    return reorder_reference.reorder(A.nrow, A.ncol, A.p, A.i, force=force)


def num_dense_columns(A):
    """IPX's rule for dense columns (no column count above max(40, 10 x the next smaller one)), restated"""
    cnt = np.sort(np.diff(A.p))
    jump = np.nonzero(cnt[1:] > np.maximum(40, 10 * cnt[:-1]))[0]
    return int(cnt.size - 1 - jump[0]) if jump.size else 0


# ---- the solve on the renumbered copy ----
VARIANTS = ("first", "second", "identity")


def solve_inputs(name, variant="first"):
    """(arguments of kkt_diag_factorize, a, b).  "second": another seed's weights under the same a, b; "identity":
    Factorize(nullptr), G = I"""
    A = matrix(name)
    st = synth.synthetic_ipm_state(A.nrow, A.ncol, 1.0, STATE_SEED[name])
    if variant == "identity":
        return (), st["a"], st["b"]
    w = st if variant == "first" else synth.synthetic_ipm_state(A.nrow, A.ncol, 1.0, SECOND_SEED)
    return (w["xl"], w["xu"], w["zl"], w["zu"], w["mu"]), st["a"], st["b"]


class Solve:
    """x, y of KKTSolverDiag::Solve after exactly `maxiter` CR iterations in extended precision, in the numbering as
    given: rhs = -b + A (W a) + W_I a_I, PCR with C = A W A' + W_I and P = 1 / diag(C), x = W (a - A'y), slack b - A x"""

    def __init__(self, A, W, resscale, a, b, maxiter):
        n = A.ncol
        op = cr_reference.NormalOp(A, W)
        Wl, al, bl = np.asarray(W, dtype=LD), np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
        rhs = -bl + Wl[n:] * al[n:]
        np.add.at(rhs, op.rows, op.vals * (Wl[:n] * al[:n])[op.cols])
        self.W, self.resscale, self.rhs = np.array(W), np.array(resscale), rhs
        self.run = cr_reference.pcr(A, W, W, rhs, 1e-30, resscale, maxiter)
        self.y = self.run.lhs
        aty = np.zeros(n, dtype=LD)
        np.add.at(aty, op.cols, op.vals * self.y[op.rows])
        xs = Wl[:n] * (al[:n] - aty)
        slack = bl.copy()
        np.subtract.at(slack, op.rows, op.vals * xs[op.cols])
        self.x = np.concatenate([xs, slack])


_solves = {}


def reference(name, variant, maxiter, W, resscale):
    """the Solve of (case, variant, maxiter) for the weights and the residual scaling that the factorization under
    test reports; they are the same bits for the device and the oracle, so one run serves both"""
    key = (name, variant, maxiter)
    if key not in _solves:
        _, a, b = solve_inputs(name, variant)
        _solves[key] = Solve(matrix(name), W, resscale, a, b, maxiter)
    assert np.array_equal(_solves[key].W, W) and np.array_equal(_solves[key].resscale, resscale)
    return _solves[key]


def dist(a, b):
    """max |a - b| / max |b| with b in extended precision"""
    b = np.asarray(b, dtype=LD)
    return float(np.abs(np.asarray(a, dtype=LD) - b).max() / np.abs(b).max())
