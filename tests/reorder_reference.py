"""A NumPy restatement of reorder_model (ipx_amd/csrc/reorder.hip), written from that file's header comment and host
code; nothing here is shared with the product or the oracle.  Integer arithmetic only, so the device's answer is held to
it bit for bit (tests/test_gpu_reorder.py); its levels are held to scipy.sparse.csgraph and to hand-worked graphs in
tests/test_reorder_reference.py.

What is restated:
  * the bipartite graph rows <-> columns of the CSC matrix; a breadth-first search from a row gives row level l to the
    rows first met after l column steps, and a column the level of the row frontier it was reached from;
  * first_unvisited: the smallest row that has no level yet and is not empty (-1 if there is none);
  * pass 1 from first_unvisited of the untouched graph; when the renumbering is not forced, rows reached within row
    levels 0..8 being at least half of all rows ends everything: `levels` is pass 1's count, no permutation (rows_by_8);
  * pass 2 on cleared levels, from the smallest row of pass 1's last non-empty row frontier; then further components,
    each from first_unvisited, until 64 searches have run, every row has a level, or no unvisited non-empty row is left;
    level numbers continue across components (level0 += row levels of the component);
  * keys (level, old index), rows and columns without a level keyed 0x7fffffff: last, by old index; perm[new] = old.
Not restated: the cap of 2^20 levels per search, and the gather layouts, their timing and the 10 % rule that follow the
numbering (a forced renumbering is kept whatever the timing says)."""
import collections

import numpy as np

MAX_COMPONENTS = 64                     # kMaxComponents
NEVER = 0x7fffffff
MIN_NNZ_UNFORCED = 1 << 20              # below this an unforced reorder_model does not look at the graph at all

Reordering = collections.namedtuple(
    "Reordering", "rowperm colperm levels components frontiers starts unreached_rows unreached_cols row_level col_level")


class Graph:
    """both directions of the bipartite graph, as pointer / index arrays"""

    def __init__(self, m, n, Ap, Ai):
        self.m, self.n = int(m), int(n)
        self.cp = np.asarray(Ap, dtype=np.int64)
        self.ci = np.asarray(Ai, dtype=np.int64)                    # column -> its rows
        assert self.cp.shape == (self.n + 1,) and self.ci.shape == (int(self.cp[-1]),)
        colof = np.repeat(np.arange(self.n, dtype=np.int64), np.diff(self.cp))
        order = np.argsort(self.ci, kind="stable")
        self.ri = colof[order]                                      # row -> its columns
        self.rp = np.concatenate([[0], np.cumsum(np.bincount(self.ci, minlength=self.m))]).astype(np.int64)


def neighbours(ptr, idx, front):
    """every entry of the lists of `front`, duplicates included"""
    cnt = ptr[front + 1] - ptr[front]
    total = int(cnt.sum())
    if total == 0:
        return np.zeros(0, dtype=np.int64)
    first = np.repeat(ptr[front], cnt)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return idx[first + within]


def first_unvisited(g, row_level):
    cand = np.nonzero((row_level < 0) & (g.rp[1:] > g.rp[:-1]))[0]
    return int(cand[0]) if cand.size else -1


def bfs(g, start, level0, row_level, col_level):
    """levels of what `start` reaches among the rows and columns that have none yet, written into row_level / col_level.
    Returns (sizes of the non-empty row frontiers, the last of those frontiers)."""
    row_level[start] = level0
    front = np.array([start], dtype=np.int64)
    sizes, last = [], front
    L = 0
    while front.size:
        sizes.append(int(front.size))
        last = front
        cols = neighbours(g.rp, g.ri, front)
        cols = np.unique(cols[col_level[cols] < 0])
        col_level[cols] = level0 + L
        rows = neighbours(g.cp, g.ci, cols)
        rows = np.unique(rows[row_level[rows] < 0])
        row_level[rows] = level0 + L + 1
        front = rows
        L += 1
    return sizes, last


def reorder(m, n, Ap, Ai, force=True):
    """Reordering of the m x n CSC pattern (Ap, Ai).  rowperm / colperm are None where reorder_model keeps none: m < 2,
    no column, no entry, unforced below 2^20 entries, no non-empty row, or the unforced expander exit (then `levels` is
    pass 1's count and `frontiers` holds pass 1 alone).  frontiers[0] is pass 1, frontiers[1:] the searches of pass 2."""
    g = Graph(m, n, Ap, Ai)
    nz = int(g.cp[-1])
    none = Reordering(None, None, 0, 0, [], [], m, n, None, None)
    if m < 2 or n < 1 or nz < 1 or (not force and nz < MIN_NNZ_UNFORCED):
        return none
    row_level, col_level = np.full(m, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    start = first_unvisited(g, row_level)
    if start < 0:
        return none
    sizes1, last1 = bfs(g, start, 0, row_level, col_level)
    frontiers, starts = [sizes1], [start]
    if not force and 2 * sum(sizes1[:9]) >= m:
        return Reordering(None, None, len(sizes1), 0, frontiers, starts, m, n, None, None)
    row_level[:] = -1
    col_level[:] = -1
    level0 = comps = reached = 0
    start = int(last1.min())
    while start >= 0 and comps < MAX_COMPONENTS:
        sizes, _ = bfs(g, start, level0, row_level, col_level)
        frontiers.append(sizes)
        starts.append(start)
        level0 += len(sizes)
        reached += sum(sizes)
        comps += 1
        if reached >= m:
            break
        start = first_unvisited(g, row_level)
    rowkey = np.where(row_level < 0, NEVER, row_level)
    colkey = np.where(col_level < 0, NEVER, col_level)
    rowperm = np.argsort(rowkey, kind="stable").astype(np.int64)     # stable: ties of the level by old index
    colperm = np.argsort(colkey, kind="stable").astype(np.int64)
    return Reordering(rowperm, colperm, level0, comps, frontiers, starts, int((row_level < 0).sum()),
                      int((col_level < 0).sum()), row_level, col_level)
