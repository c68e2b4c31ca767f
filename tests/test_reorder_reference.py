"""CPU: tests/reorder_reference.py, the restatement of reorder_model that tests/test_gpu_reorder.py holds the device to,
checked here without the device: against numberings worked out by hand, against scipy.sparse.csgraph (so that it is not
its own witness), and for the properties that make each matrix of tests/reorder_cases.py a case -- level counts at and
around a batch of 16, more components than the cap of 64, rows and columns that are never reached, an empty row 0, a
frontier wider than one launch.  The solve inputs of the GPU tests are checked too: the CPU oracle has to be within
1e-13 of the extended-precision CR on every one of them, else a GPU failure would point at the input.

Measured (oracle against tests/cr_reference.py, relative to the largest entry, the worst over maxiter 1, 6, 11):
  banded y 1.3e-15, x 5.5e-15; many components y 9.5e-16, x 9.6e-15; few components y 2.9e-15, x 1.1e-14;
  banded at maxiter 6 with the second weights y 2.7e-15, x 1.8e-14, with G = I y 5.5e-16, x 8.0e-15.
  smallest |y_i| / largest over these runs: 9.3e-8 (many components, maxiter 11), 3.2e-7 to 1.0e-4 elsewhere."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse import csgraph

import reorder_cases as cases
import reorder_reference as rr
from cr_exits_worker import MAXITERS


def csc(m, n, columns):
    """(m, n, Ap, Ai) from the row lists of the columns"""
    Ap = np.concatenate([[0], np.cumsum([len(c) for c in columns])])
    return m, n, Ap, np.array([r for c in columns for r in c], dtype=np.int64)


# ---- by hand ----
def test_path_by_hand():
    """4 -c3- 2 -c0- 0 -c1- 3 -c2- 1.  Pass 1 from row 0: {0}, {2, 3}, {1, 4}; the far end is row 1, the smaller of the
    last level.  From row 1 the rows come as 1, 3, 0, 2, 4 and the columns as c2, c1, c0, c3."""
    R = rr.reorder(*csc(5, 4, [[0, 2], [0, 3], [1, 3], [2, 4]]))
    assert R.frontiers == [[1, 2, 2], [1, 1, 1, 1, 1]] and R.starts == [0, 1]
    assert R.rowperm.tolist() == [1, 3, 0, 2, 4] and R.colperm.tolist() == [2, 1, 0, 3]
    assert R.row_level.tolist() == [2, 0, 3, 1, 4] and R.col_level.tolist() == [2, 1, 0, 3]
    assert (R.levels, R.components, R.unreached_rows, R.unreached_cols) == (5, 1, 0, 0)


def test_ties_by_old_index():
    """c0 = {0, 1, 3}, c1 = {2, 3}, c2 = {1, 2}.  Pass 1 from row 0 ends in {2}.  From row 2: c1 and c2 at level 0, rows 1
    and 3 at level 1, c0 at level 1, row 0 at level 2; equal levels keep the order as given."""
    R = rr.reorder(*csc(4, 3, [[0, 1, 3], [2, 3], [1, 2]]))
    assert R.frontiers == [[1, 2, 1], [1, 2, 1]] and R.starts == [0, 2]
    assert R.rowperm.tolist() == [2, 1, 3, 0] and R.colperm.tolist() == [1, 2, 0]


def test_components_and_empties_by_hand():
    """Row 0 and column 2 are empty; c0 = {1, 2}, c1 = {2, 3}; c3 = {4, 5}, c4 = {5}.  first_unvisited is row 1; pass 1
    ends in {3}.  Pass 2 from row 3: rows 3, 2, 1 at levels 0, 1, 2, columns c1, c0 at 0, 1.  The second component
    starts from row 4 at level 3: row 5, reached through c3, has level 4, and so has c4, reached from row 5.  Then no
    unvisited non-empty row is left.  Row 0 and column 2 are numbered last."""
    R = rr.reorder(*csc(6, 5, [[1, 2], [2, 3], [], [4, 5], [5]]))
    assert R.starts == [1, 3, 4] and R.frontiers == [[1, 1, 1], [1, 1, 1], [1, 1]]
    assert R.row_level.tolist() == [-1, 2, 1, 0, 3, 4] and R.col_level.tolist() == [1, 0, -1, 3, 4]
    assert R.rowperm.tolist() == [3, 2, 1, 4, 5, 0] and R.colperm.tolist() == [1, 0, 3, 4, 2]
    assert (R.levels, R.components, R.unreached_rows, R.unreached_cols) == (5, 2, 1, 1)


def test_nothing_to_number():
    assert rr.reorder(*csc(1, 1, [[0]])).rowperm is None                        # m < 2
    assert rr.reorder(*csc(3, 2, [[], []])).rowperm is None                     # no entry
    assert rr.reorder(*csc(5, 4, [[0, 2], [0, 3], [1, 3], [2, 4]]), force=False).levels == 0      # unforced and small


def path(m):
    return csc(m, m - 1, [[j, j + 1] for j in range(m - 1)])


def test_expander_exit_by_hand(monkeypatch):
    """a path from row 0 reaches 9 rows within row levels 0..8: half of 18 rows, less than half of 19"""
    monkeypatch.setattr(rr, "MIN_NNZ_UNFORCED", 0)
    R = rr.reorder(*path(18), force=False)
    assert R.rowperm is None and R.colperm is None and (R.levels, R.components) == (18, 0) and R.frontiers == [[1] * 18]
    R = rr.reorder(*path(19), force=False)
    assert R.rowperm.tolist() == list(range(18, -1, -1)) and R.colperm.tolist() == list(range(17, -1, -1))
    assert (R.levels, R.components) == (19, 1)
    assert rr.reorder(*path(18), force=True).rowperm.tolist() == list(range(17, -1, -1))


def test_component_cap_by_hand():
    """66 rows with one column each: 64 searches, rows 64 and 65 and their columns stay without a level"""
    R = rr.reorder(*csc(66, 66, [[j] for j in range(66)]))
    assert (R.levels, R.components, R.unreached_rows, R.unreached_cols) == (64, 64, 2, 2)
    assert R.rowperm.tolist() == list(range(66)) and R.starts == list(range(1)) + list(range(64))


# ---- against scipy.sparse.csgraph ----
def distances(A, start):
    """edges from row `start` in the bipartite graph on m + n nodes (rows first); inf where there is no path"""
    B = sp.csr_matrix((np.ones(A.nnz), A.i, A.p), shape=(A.ncol, A.nrow))       # columns x rows
    G = sp.bmat([[None, B.T], [B, None]], format="csr")
    return csgraph.shortest_path(G, unweighted=True, indices=start)


def check_search(A, R, start, level0, sizes):
    """the rows at 2 l edges from `start` have row level level0 + l, the columns at 2 l + 1 edges column level level0 + l"""
    d = distances(A, start)
    rows, cols = np.nonzero(np.isfinite(d[:A.nrow]))[0], np.nonzero(np.isfinite(d[A.nrow:]))[0]
    dr, dc = d[rows].astype(np.int64), d[A.nrow + cols].astype(np.int64)
    assert not np.any(dr % 2) and np.all(dc % 2 == 1)
    assert np.bincount(dr // 2).tolist() == sizes
    if R is not None:
        assert np.array_equal(R.row_level[rows], level0 + dr // 2) and np.array_equal(R.col_level[cols], level0 + dc // 2)
    return rows[dr == dr.max()].min()


@pytest.mark.parametrize("name", cases.NAMES)
def test_levels_are_breadth_first_levels(name):
    A, R = cases.matrix(name), cases.numbering(name)
    counts = np.bincount(A.i, minlength=A.nrow)
    assert R.starts[0] == np.nonzero(counts)[0][0]
    far = check_search(A, None, R.starts[0], 0, R.frontiers[0])
    assert R.starts[1] == far                                   # the smallest row of the last level of pass 1
    level0, seen = 0, np.zeros(A.nrow, dtype=bool)
    for k, (start, sizes) in enumerate(zip(R.starts[1:], R.frontiers[1:])):
        if k > 0:                                               # the smallest non-empty row that no search has reached
            assert start == np.nonzero(~seen & (counts > 0))[0][0]
        check_search(A, R, start, level0, sizes)
        seen |= (R.row_level >= level0) & (R.row_level < level0 + len(sizes))
        level0 += len(sizes)
    assert level0 == R.levels and R.components == len(R.frontiers) - 1
    assert np.array_equal(seen, R.row_level >= 0)
    left = ~seen & (counts > 0)
    assert R.components == rr.MAX_COMPONENTS or not left.any()


# ---- what makes each matrix a case ----
@pytest.mark.parametrize("name", cases.NAMES)
def test_case_is_renumbered_at_all(oracle, name):
    from oracle import pyoracle as po
    A, R = cases.matrix(name), cases.numbering(name)
    assert A.nnz >= cases.MIN_NNZ
    assert cases.num_dense_columns(A) == 0 and oracle.find_dense_columns(po.Csc(A.nrow, A.ncol, A.p, A.i, A.x))[0] == 0
    assert np.array_equal(np.sort(R.rowperm), np.arange(A.nrow)) and np.array_equal(np.sort(R.colperm), np.arange(A.ncol))
    for perm, level in ((R.rowperm, R.row_level), (R.colperm, R.col_level)):
        key = np.where(level < 0, rr.NEVER, level)[perm]
        assert np.all((key[1:] > key[:-1]) | ((key[1:] == key[:-1]) & (perm[1:] > perm[:-1])))
    assert np.bincount(A.i, minlength=A.nrow).max() <= 200      # no long-row path of the level kernel's inner loop


def test_banded_case():
    R = cases.numbering("banded")
    assert (R.components, R.levels, len(R.frontiers[0])) == (1, 38, 33)
    assert R.starts[1] != R.starts[0]                           # the second pass really starts elsewhere
    assert (R.unreached_rows, R.unreached_cols) == (0, 0)


def test_many_components_case():
    A, R = cases.matrix("many_components"), cases.numbering("many_components")
    B = sp.csr_matrix((np.ones(A.nnz), A.i, A.p), shape=(A.ncol, A.nrow))
    ncomp, _ = csgraph.connected_components(sp.bmat([[None, B.T], [B, None]]), directed=False)
    assert ncomp == 70 + 37 + 53                                # 70 blocks; every empty row or column is a node of its own
    assert R.components == rr.MAX_COMPONENTS == 64 and R.levels == sum(len(f) for f in R.frontiers[1:])
    assert (R.unreached_rows, R.unreached_cols) == (6 * 64 + 37, 6 * 128 + 53) == (421, 821)
    assert np.array_equal(R.rowperm[-421:], np.nonzero(R.row_level < 0)[0])      # last, by old index
    assert np.array_equal(R.colperm[-821:], np.nonzero(R.col_level < 0)[0])
    assert A.p[-1] > 0 and not np.any(A.i == 0) and R.starts[0] != 0 and R.rowperm[-421] == 0     # row 0 is empty


def test_few_components_case():
    A, R = cases.matrix("few_components"), cases.numbering("few_components")
    assert (R.components, R.levels) == (5, 80)
    assert (R.unreached_rows, R.unreached_cols) == (3, 5)       # the empty ones: the loop ends because no row is left
    assert sum(sum(f) for f in R.frontiers[1:]) == A.nrow - 3 < A.nrow


def test_wide_frontier_case():
    A, R = cases.matrix("wide_frontier"), cases.numbering("wide_frontier")
    assert (A.nrow, A.ncol, A.nnz) == (84001, 80200, 164200)
    assert (R.components, R.levels) == (1, 5)
    assert max(R.frontiers[1]) == 79600 > 65536 and np.bincount(R.col_level).max() == 79600 > 65536
    assert np.bincount(A.i, minlength=A.nrow).max() == 200


@pytest.mark.parametrize("L", cases.LAYERS)
def test_layered_cases(L):
    R = cases.numbering("layers%d" % L)
    assert R.components == 1 and len(R.frontiers[1]) == R.levels == L
    assert len(R.frontiers[0]) < L                              # pass 1 starts inside, pass 2 from an end layer


def test_expander_case():
    A = cases.expander()
    R = rr.reorder(A.nrow, A.ncol, A.p, A.i, force=False)
    assert A.nnz >= rr.MIN_NNZ_UNFORCED and R.rowperm is None and 0 < R.levels <= 12
    assert 2 * sum(R.frontiers[0][:9]) >= A.nrow


# ---- the solve inputs ----
SOLVES = [(name, "first", k) for name in cases.SOLVE_CASES for k in MAXITERS] + [("banded", "second", 6), ("banded", "identity", 6)]


@pytest.mark.parametrize("name,variant,maxiter", SOLVES)
def test_oracle_is_within_1e_13_of_extended_precision(oracle, name, variant, maxiter):
    from oracle import pyoracle as po
    A = cases.matrix(name)
    fact, a, b = cases.solve_inputs(name, variant)
    ko = oracle.kkt_diag(po.Csc(A.nrow, A.ncol, A.p, A.i, A.x), None, True, maxiter)
    assert ko.factorize(*fact) == 0
    W, resscale = ko.get()
    if variant == "identity":
        assert np.all(W == 1.0) and np.all(resscale == 1.0)
    ref = cases.reference(name, variant, maxiter, W, resscale)
    assert (ref.run.iter, ref.run.errflag) == (maxiter, 201)
    x, y, it, err, _ = ko.solve(a, b, 1e-30)
    print("%s %s maxiter %d: oracle y %.2e x %.2e; min|y|/max|y| %.2e"
          % (name, variant, maxiter, cases.dist(y, ref.y), cases.dist(x, ref.x), np.abs(y).min() / np.abs(y).max()))
    assert (it, err) == (maxiter, 201)
    assert cases.dist(y, ref.y) < 1e-13 and cases.dist(x, ref.x) < 1e-13
    # a row that took another row's data is off by about its own size: even the smallest is 1e4 times the 1e-12 gate
    assert np.abs(y).min() > 1e-8 * np.abs(y).max()
