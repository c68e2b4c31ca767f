"""GPU: the persistent accumulated-tile kernel walking STEPS (a tile's short tail batches streamed and gathered as one
batch of the pipeline, their adds kept apart by barriers; internal.hpp) against the same kernel with every batch a step
of its own (IPXK_ACC_STEPS=0: the schedule before there were steps).  A row's partial sum is the same sequence of
ds_add_f64 between the same barriers in both, so every product and every solve must agree byte for byte; the products
must also equal the sliced layout's.  Each setting runs in a process of its own (the settings are read once per process),
each shape with the kernel's own grid and with the grid capped at 16 workgroups (IPXK_ACC_PERSIST=16: a workgroup walks
many tiles).  The workers read the batch and step tables back, recompute the steps from the batches by the rule and
record what the steps look like, so that a test cannot pass on tables without multi-batch steps.

Shapes: "random" = the random LPs of test_gpu_acc_persistent.py (tiles of one to a few batches, ragged last row blocks,
2 / 4 / 8 slices) and its block LP (empty tiles between non-empty ones); "collide" = rows with 1 to 40 entries in one
slice and row blocks of 1024 rows (a tile's batches shrink from 1024 entries to a few: steps of 2, 3 and 4 batches, the
cap of four cutting a chain that could go on), and the boundary of the 2048-entry rule (batches 1024 + 1024: one full
step; 1024 + 1024 + 1: the third batch starts a new step); "special" = long rows with the SMW preconditioner
(num_dense=8), and the basis path's N N' products."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from ipx_amd import kkt, synth

group, out, layout = sys.argv[2], sys.argv[3], sys.argv[4]
os.environ["IPXK_SPMV_LAYOUT"] = layout
res = {}
BATCH, MAXB = 2048, 4

def from_triplets(m, n, rows, cols, rng):
    order = np.lexsort((rows, cols))
    rows, cols = rows[order], cols[order]
    Ap = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    Ax = rng.uniform(0.5, 4.0, rows.size) * rng.choice([-1.0, 1.0], rows.size)
    return synth.CscMatrix(m, n, Ap, rows, Ax)

def block_lp(m, n, seed):
    # (test_gpu_acc_persistent.py) the columns of each run of 1024 touch one of three bands of rows, in turn: row blocks of
    # the transposed product whose tiles in some slices are empty, between row blocks where they are not
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 12, n)
    Ap = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    Ai = np.empty(Ap[-1], np.int64)
    for j in range(n):
        band = (j // 1024) % 3
        lo, hi = band * m // 3, (band + 1) * m // 3
        Ai[Ap[j]:Ap[j + 1]] = np.sort(rng.choice(np.arange(lo, hi), lens[j], replace=False))
    Ax = rng.uniform(0.5, 4.0, Ap[-1]) * rng.choice([-1.0, 1.0], Ap[-1])
    return synth.CscMatrix(m, n, Ap, Ai, Ax)

def ragged_lp(m, seed):
    # 8192 columns = 4 slices of 2048 (IPXK_SLICE_TEST_KB=16); row r has 1 .. 40 entries in slice 0 and 1 .. 6 in each of the
    # others, at distinct random columns: with 1024 rows per tile (IPXK_ACC_ROWS) batch k of a tile holds the rows of more
    # than k entries -- 1024 entries down to a few
    rng = np.random.default_rng(seed)
    n, W = 8192, 2048
    rows, cols = [], []
    for r in range(m):
        for s in range(4):
            c = rng.choice(W, int(rng.integers(1, 41 if s == 0 else 7)), replace=False) + s * W
            rows.append(np.full(c.size, r)); cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    empty = np.setdiff1d(np.arange(n), cols)                  # no empty column: one entry more in some row
    rows = np.concatenate([rows, rng.integers(0, m, empty.size)]); cols = np.concatenate([cols, empty])
    return from_triplets(m, n, rows, cols, rng)

def boundary_lp(seed):
    # 2048 rows = two row blocks of 1024, 8192 columns = 4 slices of 2048: every row has exactly two entries in every slice
    # (batches 1024 + 1024 in every tile), but row 1031 has three in slice 2 (tile (1, 2): batches 1024, 1024, 1)
    rng = np.random.default_rng(seed)
    m, n, W = 2048, 8192, 2048
    rows, cols = [], []
    for s in range(4):
        p = rng.permutation(W)
        for q in (p, np.roll(p, int(rng.integers(1, W)))):        # two different columns per row, every column twice
            rows.append(np.arange(m)); cols.append(q[np.arange(m) % W] + s * W)
    extra = next(c for c in range(2 * W, 3 * W) if c not in (cols[4][1031], cols[5][1031]))
    rows.append(np.array([1031])); cols.append(np.array([extra]))
    return from_triplets(m, n, np.concatenate(rows), np.concatenate(cols), rng)

def steps_of(tb, bp):
    # the rule, per tile, left to right: a step takes consecutive batches while their total is at most BATCH entries and it
    # holds at most MAXB of them.  Returns tile_step, the records and, per tile, the batch sizes of each step
    tile_step, recs, groups = [0], [], []
    for t in range(tb.size - 1):
        b, b1, g = int(tb[t]), int(tb[t + 1]), []
        while b < b1:
            k = 1
            while k < MAXB and b + k < b1 and int(bp[b + k + 1]) - int(bp[b]) <= BATCH:
                k += 1
            end = int(bp[b + k])
            recs.append([int(bp[b])] + [int(bp[b + i]) if i < k else end for i in (1, 2, 3)])
            g.append([int(bp[b + i + 1]) - int(bp[b + i]) for i in range(k)])
            b += k
        tile_step.append(len(recs))
        groups.append(g)
    recs.append([int(bp[-1])] * 4)
    return np.array(tile_step, np.uint32), np.array(recs, np.uint32).reshape(-1, 4), groups

def inspect(tag, ctx):
    # the step tables against the rule, and what they hold
    info = [ctx.layout_info(w)[0] for w in (0, 1)]
    res[tag + "_layout"] = [[d["use_acc"], d["acc_nslices"], d["acc_nrb"], d["acc_RB"], d["nlong"], d["acc_nbatches"], d["acc_nsteps"]]
                            for d in info]
    if layout != "acc":
        return
    shapes = []
    for w, d in enumerate(info):
        if not d["use_acc"]:
            shapes.append(None)
            continue
        tb, bp = ctx.layout_array(w, 11), ctx.layout_array(w, 12)
        ts, rec = ctx.layout_array(w, 21), ctx.layout_array(w, 22).reshape(-1, 4)
        assert tb.size == d["acc_nslices"] * d["acc_nrb"] + 1 and bp.size == d["acc_nbatches"] + 1, (tag, w)
        assert ts.size == tb.size and rec.shape[0] == d["acc_nsteps"] + 1 and int(ts[-1]) == d["acc_nsteps"], (tag, w)
        if os.environ.get("IPXK_ACC_STEPS") == "0":
            assert d["acc_nsteps"] == d["acc_nbatches"] and np.array_equal(ts, tb), (tag, w)
            assert np.array_equal(rec[:, 0], bp) and all(np.array_equal(rec[:-1, i], bp[1:]) for i in (1, 2, 3)), (tag, w)
            shapes.append(None)
            continue
        ts2, rec2, groups = steps_of(tb, bp)
        assert np.array_equal(ts, ts2) and np.array_equal(rec, rec2), (tag, w)
        sizes = sorted({len(s) for g in groups for s in g})
        four_then_more = any(len(s) == MAXB and i + 1 < len(g) for g in groups for i, s in enumerate(g))
        empty_after_multi = any(not groups[t] and t > 0 and groups[t - 1] and len(groups[t - 1][-1]) > 1 for t in range(len(groups)))
        distinct = sorted({json.dumps(g) for g in groups})
        shapes.append({"sizes": sizes, "four_then_more": four_then_more, "empty_tiles": sum(not g for g in groups),
                       "empty_after_multi": empty_after_multi, "groupings": [json.loads(g) for g in distinct[:16]], "ndistinct": len(distinct)})
    res[tag + "_steps"] = shapes

def products_and_solve(tag, A, seed, maxiter=500):
    m, n = A.nrow, A.ncol
    ctx = kkt.KktContext(A, device=0)
    inspect(tag, ctx)
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.1, 10.0, m + n)
    y = rng.standard_normal(m)
    ctx.normal_prepare(W)
    lhs, dot = ctx.normal_apply(y)            # EpiScale (A'y) and EpiNormalRows (A t)
    np.save("%s/%s_lhs.npy" % (out, tag), lhs)
    if layout == "acc":
        st = synth.synthetic_ipm_state(m, n, 1.0, seed)
        assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
        x, yy, it, err, _ = ctx.kkt_diag_solve(st["a"], st["b"], 0.3 * np.sqrt(st["mu"]), maxiter)   # + EpiKktRhs, EpiRecoverX
        np.save("%s/%s_x.npy" % (out, tag), x)
        np.save("%s/%s_y.npy" % (out, tag), yy)
        res[tag + "_scalars"] = [float(dot).hex(), int(it), int(err)]
    ctx.close()

if group == "random":
    # slices of 16 to 256 KiB: 2, 4 and 8 slices, ragged last row blocks
    for (m, n, seed, kb) in ((9000, 20011, 1, "16"), (20000, 45000, 2, "128"), (33333, 70001, 3, "128"), (70001, 150007, 4, "256"),
                             (60000, 130000, 7, "16")):
        os.environ["IPXK_SLICE_TEST_KB"] = kb
        if seed == 2:
            os.environ["IPXK_SLICE_FORCE2"] = "1"          # A'y: y of 160 KiB in two slices of 128 KiB
        products_and_solve("lp%d" % seed, synth.synthetic_lp(m, n, 8, seed), seed)
        os.environ.pop("IPXK_SLICE_FORCE2", None)
    os.environ["IPXK_SLICE_TEST_KB"] = "16"
    products_and_solve("block", block_lp(30000, 40000, 5), 5)
elif group == "collide":
    os.environ["IPXK_SLICE_TEST_KB"] = "16"
    os.environ["IPXK_ACC_ROWS"] = "1024"
    products_and_solve("ragged", ragged_lp(3 * 1024 + 500, 11), 11, maxiter=60)
    products_and_solve("boundary", boundary_lp(12), 12, maxiter=60)
else:
    os.environ["IPXK_SLICE_TEST_KB"] = "16"
    products_and_solve("dense", synth.synthetic_lp(20000, 45000, 8, 6, num_dense=8), 6)
    if layout == "acc":
        # basis path: the N N' products of the basis preconditioner
        B = synth.planted_lu_basis(synth.synthetic_lp(20000, 45000, 8, 8), seed=8, num_free=2)
        cs = synth.synthetic_basis_state(B["status"], 1.0, 8)
        ctx = kkt.KktContext(B["A"], device=0)
        inspect("basis", ctx)
        ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], cs)
        st = synth.synthetic_ipm_state(20000, 45000, 1.0, 8)
        xb, yb, itb, errb, _ = ctx.kkt_basis_solve(st["a"], st["b"], 1e-8)
        ctx.close()
        np.save(out + "/basis_x.npy", xb)
        np.save(out + "/basis_y.npy", yb)
        res["basis_scalars"] = [int(itb), int(errb)]

with open(out + "/res.json", "w") as f:
    json.dump(res, f)
"""


def _run(group, tmp, name, layout, **env):
    out = tmp / name
    out.mkdir()
    subprocess.run([sys.executable, "-c", WORKER, ROOT, group, str(out), layout], env=dict(os.environ, **env), check=True, timeout=600)
    with open(out / "res.json") as f:
        return out, json.load(f)


@pytest.fixture(scope="module")
def sliced_products(tmp_path_factory):
    """The products of every shape through the sliced layout: once per group, shared by both grids."""
    cache = {}

    def get(group):
        if group not in cache:
            cache[group] = _run(group, tmp_path_factory.mktemp("sliced_" + group), "sliced", "sliced")
        return cache[group]
    return get


def _acc(res):
    """(tag, which, layout scalars, step shapes) of every matrix of a run that went through the accumulated tiles"""
    for k in sorted(res):
        if k.endswith("_layout"):
            tag = k[:-len("_layout")]
            for w, l in enumerate(res[k]):
                if l[0]:
                    yield tag, w, l, (res.get(tag + "_steps") or [None, None])[w]


@pytest.mark.parametrize("persist", ["1", "16"])
@pytest.mark.parametrize("group", ["random", "collide", "special"])
def test_steps_equal_one_batch_per_step(group, persist, tmp_path, sliced_products):
    d0, r0 = _run(group, tmp_path, "steps0", "acc", IPXK_ACC_PERSIST=persist, IPXK_ACC_STEPS="0")
    d1, r1 = _run(group, tmp_path, "steps1", "acc", IPXK_ACC_PERSIST=persist, IPXK_ACC_STEPS="1")
    # byte-equal products, solves, iteration counts and flags
    assert sorted(r0) == sorted(r1)
    for k in r0:
        if k.endswith("_layout"):
            assert [l[:6] for l in r0[k]] == [l[:6] for l in r1[k]], (k, r0[k], r1[k])       # the same tiles and batches
            assert all(l[6] == l[5] for l in r0[k] if l[0]), (k, r0[k])                        # IPXK_ACC_STEPS=0: a step per batch
        elif not k.endswith("_steps"):
            assert r0[k] == r1[k], (k, r0[k], r1[k])
    files = sorted(p.name for p in d0.glob("*.npy"))
    assert files == sorted(p.name for p in d1.glob("*.npy")) and files
    for name in files:
        assert (d0 / name).read_bytes() == (d1 / name).read_bytes(), name
    # the products equal the sliced layout's
    ds, rs = sliced_products(group)
    prods = sorted(p.name for p in ds.glob("*_lhs.npy"))
    assert prods == [f for f in files if f.endswith("_lhs.npy")]
    for name in prods:
        a, b = np.load(ds / name), np.load(d1 / name)
        assert a.shape == b.shape and np.array_equal(a, b), name
    assert all(not l[0] for k in rs if k.endswith("_layout") for l in rs[k]), rs
    # the run did go through multi-batch steps
    acc = list(_acc(r1))
    tags = {"random": ["block", "lp1", "lp2", "lp3", "lp4", "lp7"], "collide": ["boundary", "ragged"], "special": ["basis", "dense"]}[group]
    assert sorted({a[0] for a in acc}) == tags, acc                                            # every shape has a matrix in accumulated tiles
    for tag, w, l, shape in acc:
        assert shape is not None, (tag, w)
        if tag != "boundary":
            assert l[6] < l[5], (tag, w, l)                                                    # fewer steps than batches
            assert max(shape["sizes"]) > 1, (tag, w, shape)
    if group == "random":
        assert {2, 8} <= {l[1] for _, _, l, _ in acc}, acc                                     # 2 and 8 slices among the shapes
        block = [s for tag, _, _, s in acc if tag == "block"]
        assert any(s["empty_tiles"] and s["empty_after_multi"] for s in block), block          # an empty tile right after a multi-phase step
        if persist == "16":
            assert any(l[1] * l[2] >= 4 * 16 for _, _, l, _ in acc), acc                       # many tiles per workgroup
    if group == "collide":
        (rag,) = [(l, s) for tag, w, l, s in acc if tag == "ragged" and w == 1]
        assert rag[0][3] == 1024 and {2, 3, 4} <= set(rag[1]["sizes"]) and rag[1]["four_then_more"], rag
        (bnd,) = [(l, s) for tag, w, l, s in acc if tag == "boundary" and w == 1]
        assert bnd[0][3] == 1024 and bnd[0][1] * bnd[0][2] == 8, bnd
        assert sorted(bnd[1]["groupings"]) == [[[1024, 1024]], [[1024, 1024], [1]]] and bnd[1]["ndistinct"] == 2, bnd
        assert bnd[0][5] == 17 and bnd[0][6] == 9, bnd                                         # 7 tiles of one full step, one of two steps
