"""Worker of test_gpu_acc_head.py (one process per setting: IPXK_ACC_HEAD, IPXK_ACC_WARM, IPXK_ACC_WIDE, IPXK_ACC_STEPS,
IPXK_ACC_PERSIST and IPXK_ACC_ROWS are read once per process).  argv: repository root, group, output directory.
Writes the products and solves as .npy files and what it saw of the tables as res.json.  The shape builders are those of
acc_wide_worker.py, "tp" with four more tiles."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, sys.argv[1])
from ipx_amd import kkt, synth  # noqa: E402

group, out = sys.argv[2], sys.argv[3]
os.environ["IPXK_SPMV_LAYOUT"] = "auto" if group == "builders" else "acc"
HEAD_ON = os.environ.get("IPXK_ACC_HEAD", "0") != "0"          # (the head tables are built only on request)
WIDE_ON = os.environ.get("IPXK_ACC_WIDE") != "0"
res = {}
THREADS, HEAD_WORDS, HEAD_STEPS, HEAD_STREAMS = 512, 64, 6, 3
TP_SIZES = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048]
FULL_BATCHES = [3, 4, 6, 7]


def from_triplets(m, n, rows, cols, rng):
    order = np.lexsort((rows, cols))
    rows, cols = rows[order], cols[order]
    Ap = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    Ax = rng.uniform(0.5, 4.0, rows.size) * rng.choice([-1.0, 1.0], rows.size)
    return synth.CscMatrix(m, n, Ap, rows.astype(np.int64), Ax)


def ragged_lp(m, seed):
    # 8192 columns = 4 slices of 2048; row r has 1 .. 40 entries in slice 0 and 1 .. 6 in each of the others: with 1024 rows per
    # tile batch k of a tile holds the rows of more than k entries -- 1024 entries down to a few (steps of several batches)
    rng = np.random.default_rng(seed)
    n, W = 8192, 2048
    rows, cols = [], []
    for r in range(m):
        for s in range(4):
            c = rng.choice(W, int(rng.integers(1, 41 if s == 0 else 7)), replace=False) + s * W
            rows.append(np.full(c.size, r))
            cols.append(c)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    empty = np.setdiff1d(np.arange(n), cols)
    rows = np.concatenate([rows, rng.integers(0, m, empty.size)])
    cols = np.concatenate([cols, empty])
    return from_triplets(m, n, rows, cols, rng)


def boundary_lp(seed):
    # two row blocks of 1024, 4 slices of 2048: every row has exactly two entries in every slice (batches 1024 + 1024 in every
    # tile), but row 1031 has three in slice 2 (tile (1, 2): batches 1024, 1024, 1)
    rng = np.random.default_rng(seed)
    m, W = 2048, 2048
    rows, cols = [], []
    for s in range(4):
        p = rng.permutation(W)
        for q in (p, np.roll(p, int(rng.integers(1, W)))):
            rows.append(np.arange(m))
            cols.append(q[np.arange(m) % W] + s * W)
    extra = next(c for c in range(2 * W, 3 * W) if c not in (cols[4][1031], cols[5][1031]))
    rows.append(np.array([1031]))
    cols.append(np.array([extra]))
    return from_triplets(m, 8192, np.concatenate(rows), np.concatenate(cols), rng)


def tp_lp(seed):
    # 32 row blocks of 4096 rows (IPXK_ACC_ROWS=4096), 8 slices of 2048 columns (IPXK_SLICE_TEST_KB=16): 256 tiles, one per
    # workgroup of the full grid.  Row block rb has one entry per row in slice rb % 8, every column of the slice twice: a tile of
    # two full batches.  Row block k < len(sizes) has sizes[k] more entries, in distinct rows, in slice (k + 1) % 8: a tile of one
    # batch of that size (2049: batches 2048 + 1).  Row block 20 + i has FULL_BATCHES[i] entries in each of its first 2048 rows in
    # slice (rb + 3) % 8: a tile of that many full batches.  Every other tile is empty.
    rng = np.random.default_rng(seed)
    RB, nrb, W, ns = 4096, 32, 2048, 8
    rows, cols = [], []
    for rb in range(nrb):
        rows.append(rb * RB + np.arange(RB))
        cols.append((rb % ns) * W + np.concatenate([rng.permutation(W), rng.permutation(W)]))
    for k, size in enumerate(TP_SIZES + [2049, 1000]):
        rows.append(k * RB + rng.choice(RB, size, replace=False))
        cols.append(((k + 1) % ns) * W + rng.integers(0, W, size))
    for i, nb in enumerate(FULL_BATCHES):
        rb = 20 + i
        for r in range(2048):
            rows.append(np.full(nb, rb * RB + r))
            cols.append(((rb + 3) % ns) * W + rng.choice(W, nb, replace=False))
    return from_triplets(RB * nrb, W * ns, np.concatenate(rows), np.concatenate(cols), rng)


def wide_threads(ne):
    return min(THREADS, ((ne + 3) // 4 + 63) // 64 * 64)


def head_of(ts, rec, wstart, wide, P):
    # the head tables by their definition: the persistent kernel's walker from tile w, step 0, on a grid of P workgroups
    ntiles = ts.size - 1
    head = np.zeros((P, HEAD_WORDS), np.uint32)
    hw = np.zeros((P, HEAD_STREAMS, 3, THREADS, 4), np.uint32) if wide is not None else None
    units = wide.reshape(-1, 4) if wide is not None else None
    total, first_ne = [], []
    t = np.arange(THREADS)
    for w in range(P):
        total.append(sum(max(int(ts[k + 1]) - int(ts[k]), 1) for k in range(w, ntiles, P)))
        wt, wq = w, 0
        wb0, wnb = int(ts[wt]), int(ts[wt + 1]) - int(ts[wt])
        for i in range(HEAD_STEPS):
            r = [0, 0, 0, 0, 0, 0, 0xFFFFFFFF, 0]
            if wt < ntiles:
                r[6] = wt
                if wnb > 0:
                    a = rec[wb0 + wq]
                    r[0], r[2], r[3], r[4], r[1] = int(a[0]), int(a[1]), int(a[2]), int(a[3]), int(rec[wb0 + wq + 1][0])
                    if wstart is not None:
                        r[5] = int(wstart[wb0 + wq])
                wq += 1
                if wq >= max(wnb, 1):
                    wt, wq = wt + P, 0
                    if wt < ntiles:
                        wb0, wnb = int(ts[wt]), int(ts[wt + 1]) - int(ts[wt])
            head[w, 8 * i:8 * i + 8] = r
            if i == 0:
                first_ne.append(r[1] - r[0])
            if hw is not None and i < HEAD_STREAMS and r[6] != 0xFFFFFFFF:
                tp = wide_threads(r[1] - r[0])
                src = r[5] + np.minimum(t, max(tp - 1, 0))
                for p in range(3):
                    hw[w, i, p] = units[src + p * tp]
        head[w, 8 * HEAD_STEPS:8 * HEAD_STEPS + 4] = [wt, wq, wb0, wnb]
    return head.ravel(), (hw.ravel() if hw is not None else None), total, first_ne


def inspect(tag, ctx):
    info = [ctx.layout_info(w)[0] for w in (0, 1)]
    res[tag + "_layout"] = [[d["use_acc"], d["acc_nslices"], d["acc_nrb"], d["acc_RB"], d["nlong"], d["acc_nbatches"], d["acc_nsteps"]]
                            for d in info]
    seen = []
    for w, d in enumerate(info):
        if not d["acc_built"]:
            seen.append(None)
            continue
        head, hwide = ctx.layout_array(w, 25), ctx.layout_array(w, 26)
        if not HEAD_ON:
            assert d["acc_head_grid"] == 0 and head.size == 0 and hwide.size == 0, (tag, w)
            seen.append(None)
            continue
        P, ntiles = d["acc_head_grid"], d["acc_nrb"] * d["acc_nslices"]
        persist = int(os.environ.get("IPXK_ACC_PERSIST", "1"))
        assert 0 < P <= ntiles and (P == ntiles or P % 8 == 0) and (persist == 1 or P <= persist), (tag, w, P, ntiles)
        ts, rec = ctx.layout_array(w, 21), ctx.layout_array(w, 22).reshape(-1, 4)
        wide = ctx.layout_array(w, 23) if WIDE_ON else None
        wstart = ctx.layout_array(w, 24) if WIDE_ON else None
        assert (d["acc_wide_units"] > 0) == WIDE_ON, (tag, w)
        head2, hwide2, total, first_ne = head_of(ts, rec, wstart, wide, P)
        assert head.size == P * HEAD_WORDS and np.array_equal(head, head2), (tag, w, int(np.flatnonzero(head != head2)[0]) if head.size == head2.size else -1)
        if WIDE_ON:
            assert hwide.size == P * HEAD_STREAMS * 3 * THREADS * 4 and np.array_equal(hwide, hwide2), (tag, w)
        else:
            assert hwide.size == 0, (tag, w)
        nt = np.diff(ts.astype(np.int64))
        seen.append({"P": P, "ntiles": ntiles, "steps_per_wg": sorted(set(total)), "first_ne": sorted(set(first_ne)),
                     "first_tile_empty": int(sum(nt[w_] == 0 for w_ in range(P))),
                     "only_tile_empty": int(sum(nt[w_] == 0 and w_ + P >= ntiles for w_ in range(P))),
                     "tiles_per_wg": -(-ntiles // P),
                     # most batches in a step among the first three steps of a workgroup's first tile
                     "batches_in_head_step": max([1] + [int((rec[int(ts[w_]) + i, 1:] < rec[int(ts[w_]) + i + 1, 0]).sum()) + 1
                                                        for w_ in range(P) for i in range(min(int(nt[w_]), HEAD_STREAMS))])})
    res[tag + "_head"] = seen
    return info


def rows_touching(A, colmask):
    entry_col = np.repeat(np.arange(A.ncol), np.diff(np.asarray(A.p)))
    return np.unique(np.asarray(A.i)[colmask[entry_col]])


def padding(tag, ctx, A, info, seed):
    # A padding position of the wide stream and every position of an empty step hold word 0: the slice's first element is
    # gathered for it.  Make that element NaN (inf) in every slice: only rows with an entry there may come out non-finite.
    m, n = A.nrow, A.ncol
    rng = np.random.default_rng(seed + 100)
    W0, y0 = rng.uniform(0.1, 10.0, m + n), rng.standard_normal(m)
    for name, bad in (("nan", np.nan), ("inf", np.inf)):
        if info[1]["use_acc"]:
            J = np.arange(info[1]["acc_nslices"]) * info[1]["acc_slice_elems"]
            J = J[J < n]
            W = W0.copy()
            W[J] = bad
            ctx.normal_prepare(W)
            lhs, _ = ctx.normal_apply(y0)
            mask = np.zeros(n, bool)
            mask[J] = True
            allowed, got = rows_touching(A, mask), np.flatnonzero(~np.isfinite(lhs))
            assert got.size > 0 and np.isin(got, allowed).all(), (tag, name, "weights", got[:8], allowed[:8])
            np.save("%s/%s_pad_w_%s.npy" % (out, tag, name), lhs)
        if info[0]["use_acc"]:
            I = np.arange(info[0]["acc_nslices"]) * info[0]["acc_slice_elems"]
            I = I[I < m]
            y = y0.copy()
            y[I] = bad
            ctx.normal_prepare(W0)
            lhs, _ = ctx.normal_apply(y)
            hit = np.isin(np.asarray(A.i), I)
            entry_col = np.repeat(np.arange(n), np.diff(np.asarray(A.p)))
            mask = np.zeros(n, bool)
            mask[entry_col[hit]] = True
            allowed, got = np.union1d(rows_touching(A, mask), I), np.flatnonzero(~np.isfinite(lhs))
            assert got.size > 0 and np.isin(got, allowed).all(), (tag, name, "y", got[:8], allowed[:8])
            np.save("%s/%s_pad_y_%s.npy" % (out, tag, name), lhs)


def products_and_solve(tag, A, seed, maxiter=60, pad=False):
    m, n = A.nrow, A.ncol
    ctx = kkt.KktContext(A, device=0)
    info = inspect(tag, ctx)
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.1, 10.0, m + n)
    y = rng.standard_normal(m)
    ctx.normal_prepare(W)
    lhs, dot = ctx.normal_apply(y)            # both gather matrices: EpiScale (A'y) and EpiNormalRows (A t)
    np.save("%s/%s_lhs.npy" % (out, tag), lhs)
    st = synth.synthetic_ipm_state(m, n, 1.0, seed)
    assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    x, yy, it, err, _ = ctx.kkt_diag_solve(st["a"], st["b"], 0.3 * np.sqrt(st["mu"]), maxiter)
    np.save("%s/%s_x.npy" % (out, tag), x)
    np.save("%s/%s_y.npy" % (out, tag), yy)
    res[tag + "_scalars"] = [float(dot).hex(), int(it), int(err)]
    if pad:
        padding(tag, ctx, A, info, seed)
    ctx.close()


def basis_solve(tag, m, n, seed):
    # basis path: the N N' products of the basis preconditioner
    B = synth.planted_lu_basis(synth.synthetic_lp(m, n, 8, seed), seed=seed, num_free=2)
    cs = synth.synthetic_basis_state(B["status"], 1.0, seed)
    ctx = kkt.KktContext(B["A"], device=0)
    inspect(tag, ctx)
    ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], cs)
    st = synth.synthetic_ipm_state(m, n, 1.0, seed)
    xb, yb, itb, errb, _ = ctx.kkt_basis_solve(st["a"], st["b"], 1e-8)
    ctx.close()
    np.save("%s/%s_x.npy" % (out, tag), xb)
    np.save("%s/%s_y.npy" % (out, tag), yb)
    res[tag + "_scalars"] = [int(itb), int(errb)]


if group == "rows4096":
    os.environ["IPXK_SLICE_TEST_KB"] = "16"
    os.environ["IPXK_ACC_ROWS"] = "4096"
    products_and_solve("tp", tp_lp(13), 13, pad=True)
elif group == "rows1024":
    # 1024-row tiles: the several-batch steps of "ragged" and "boundary" (16 and 8 tiles: fewer than the grid), random LPs with
    # 4, 2 and 8 slices and ragged last row blocks (36, 20 and 472 tiles), the basis path
    os.environ["IPXK_SLICE_TEST_KB"] = "16"
    os.environ["IPXK_ACC_ROWS"] = "1024"
    products_and_solve("ragged", ragged_lp(3 * 1024 + 500, 11), 11)
    products_and_solve("boundary", boundary_lp(12), 12)
    products_and_solve("lp1", synth.synthetic_lp(9000, 20011, 8, 1), 1, pad=True)
    basis_solve("basis1", 9000, 20011, 1)
    os.environ["IPXK_SLICE_TEST_KB"] = "64"
    os.environ["IPXK_SLICE_FORCE2"] = "1"              # A'y: y of 80 KiB in two slices of 64 KiB
    products_and_solve("lp2", synth.synthetic_lp(10000, 22000, 8, 2), 2)
    basis_solve("basis2", 10000, 22000, 2)
    os.environ.pop("IPXK_SLICE_FORCE2", None)
    os.environ["IPXK_SLICE_TEST_KB"] = "128"
    products_and_solve("lp7", synth.synthetic_lp(60000, 130000, 8, 7), 7)
    os.environ["IPXK_SLICE_TEST_KB"] = "16"
    basis_solve("basis", 8000, 18000, 8)
elif group == "builders":
    # the host builders against the device builders (layout "auto"; a shape of test_gpu_layout.py, whose layouts are acc + acc)
    os.environ["IPXK_SLICE_TEST_KB"] = "16"
    os.environ["IPXK_BUILD_ALL_LAYOUTS"] = "1"
    A = synth.synthetic_lp(9000, 20011, 8, 1)
    ctxs = []
    for build in ("host", "device"):
        os.environ["IPXK_LAYOUT_BUILD"] = build
        ctxs.append(kkt.KktContext(A, device=0))
    inspect("lp1", ctxs[1])                   # the device builder's against the definition
    for w in (0, 1):
        ih, idv = ctxs[0].layout_info(w)[0], ctxs[1].layout_info(w)[0]
        assert ih["acc_built"] == idv["acc_built"] == 1 and ih["acc_head_grid"] == idv["acc_head_grid"] > 0, (w, ih, idv)
        for a in (21, 22, 25, 26):
            x, z = ctxs[0].layout_array(w, a), ctxs[1].layout_array(w, a)
            assert x.size > 0 and np.array_equal(x, z), (w, a)
    for c in ctxs:
        c.close()
else:
    raise SystemExit("unknown group " + group)

with open(out + "/res.json", "w") as f:
    json.dump(res, f)
