"""Worker of test_gpu_acc_wide.py (one process per setting: IPXK_ACC_WIDE, IPXK_ACC_STEPS, IPXK_ACC_PERSIST and IPXK_ACC_ROWS are
read once per process).  argv: repository root, group, output directory, layout (IPXK_SPMV_LAYOUT; "auto" for the builders).
Writes the products and solves as .npy files and what it saw of the tables as res.json."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, sys.argv[1])
from ipx_amd import kkt, synth  # noqa: E402

group, out, layout = sys.argv[2], sys.argv[3], sys.argv[4]
os.environ["IPXK_SPMV_LAYOUT"] = layout
WIDE_ON = os.environ.get("IPXK_ACC_WIDE") != "0"
res = {}
BATCH, THREADS = 2048, 512
TP_SIZES = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048]


def from_triplets(m, n, rows, cols, rng):
    order = np.lexsort((rows, cols))
    rows, cols = rows[order], cols[order]
    Ap = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int64)
    Ax = rng.uniform(0.5, 4.0, rows.size) * rng.choice([-1.0, 1.0], rows.size)
    return synth.CscMatrix(m, n, Ap, rows.astype(np.int64), Ax)


def ragged_lp(m, seed):
    # (test_gpu_acc_steps.py) 8192 columns = 4 slices of 2048; row r has 1 .. 40 entries in slice 0 and 1 .. 6 in each of the
    # others: with 1024 rows per tile batch k of a tile holds the rows of more than k entries -- 1024 entries down to a few
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
    # (test_gpu_acc_steps.py) two row blocks of 1024, 4 slices of 2048: every row has exactly two entries in every slice
    # (batches 1024 + 1024 in every tile), but row 1031 has three in slice 2 (tile (1, 2): batches 1024, 1024, 1)
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
    # 32 row blocks of 4096 rows (IPXK_ACC_ROWS=4096; 32 x 8 tiles keep the row block at 4096), 8 slices of 2048 columns
    # (IPXK_SLICE_TEST_KB=16).  Row block rb has one entry per row in slice rb % 8, every column of the slice twice: one tile of
    # two full batches.  Row block k < len(sizes) has sizes[k] more entries, in distinct rows, in slice (k + 1) % 8: a tile of
    # one batch of that size (2049: batches 2048 + 1).  Every other tile is empty.
    rng = np.random.default_rng(seed)
    RB, nrb, W, ns = 4096, 32, 2048, 8
    rows, cols = [], []
    for rb in range(nrb):
        rows.append(rb * RB + np.arange(RB))
        cols.append((rb % ns) * W + np.concatenate([rng.permutation(W), rng.permutation(W)]))
    for k, size in enumerate(TP_SIZES + [2049, 1000]):
        rows.append(k * RB + rng.choice(RB, size, replace=False))
        cols.append(((k + 1) % ns) * W + rng.integers(0, W, size))
    return from_triplets(RB * nrb, W * ns, np.concatenate(rows), np.concatenate(cols), rng)


def wide_of(pack, val, rec):
    # the wide stream by its definition: step k of ne entries from rec[k, 0], Tp = min(512, roundup64(ceil(ne / 4))) threads,
    # 3 Tp units of 16 bytes: {words of positions t, Tp + t, 2 Tp + t, 3 Tp + t}, {values of the first two}, {of the last two}
    e = rec[:, 0].astype(np.int64)
    ne = np.diff(e)
    tp = np.minimum(THREADS, ((ne + 3) // 4 + 63) // 64 * 64)
    start = np.concatenate([[0], np.cumsum(3 * tp)])
    wide = np.zeros(int(start[-1]) * 4, np.uint32)
    words, values = wide.reshape(-1, 4), wide.view(np.float64).reshape(-1, 2)
    for k in range(ne.size):
        T, w0, n = int(tp[k]), int(start[k]), int(ne[k])
        pw, pv = np.zeros(4 * T, np.uint32), np.zeros(4 * T)
        pw[:n], pv[:n] = pack[e[k]:e[k] + n], val[e[k]:e[k] + n]
        words[w0:w0 + T] = pw.reshape(4, T).T
        values[w0 + T:w0 + 2 * T] = pv.reshape(4, T)[:2].T
        values[w0 + 2 * T:w0 + 3 * T] = pv.reshape(4, T)[2:].T
    return wide, start.astype(np.uint32), ne


def inspect(tag, ctx):
    # layout scalars; with the accumulated tiles the wide stream against its definition, and the step sizes it holds
    info = [ctx.layout_info(w)[0] for w in (0, 1)]
    res[tag + "_layout"] = [[d["use_acc"], d["acc_nslices"], d["acc_nrb"], d["acc_RB"], d["nlong"], d["acc_nbatches"], d["acc_nsteps"]]
                            for d in info]
    if layout == "sliced":
        return info
    seen = []
    for w, d in enumerate(info):
        if not d["acc_built"]:
            seen.append(None)
            continue
        wide, start = ctx.layout_array(w, 23), ctx.layout_array(w, 24)
        if not WIDE_ON:
            assert d["acc_wide_units"] == 0 and wide.size == 0 and start.size == 0, (tag, w)
            seen.append(None)
            continue
        ts, rec = ctx.layout_array(w, 21), ctx.layout_array(w, 22).reshape(-1, 4)
        wide2, start2, ne = wide_of(ctx.layout_array(w, 13), ctx.layout_array(w, 14), rec)
        assert start.size == d["acc_nsteps"] + 1 and int(start[-1]) == d["acc_wide_units"] and wide.size == 4 * d["acc_wide_units"], (tag, w)
        assert np.array_equal(start, start2), (tag, w)
        assert np.array_equal(wide, wide2), (tag, w, int(np.flatnonzero(wide != wide2)[0]))
        seen.append({"ne": sorted({int(v) for v in ne}), "empty_tiles": int((np.diff(ts.astype(np.int64)) == 0).sum()),
                     "short_steps": int((ne < BATCH).sum()), "nsteps": int(ne.size)})
    res[tag + "_wide"] = seen
    return info


def rows_touching(A, colmask):
    entry_col = np.repeat(np.arange(A.ncol), np.diff(np.asarray(A.p)))
    return np.unique(np.asarray(A.i)[colmask[entry_col]])


def padding(tag, ctx, A, info, seed):
    # A padding position of the wide stream holds word 0: the slice's first element is gathered for it.  Make that element NaN
    # (inf) in every slice: only rows with an entry there may come out non-finite.  Pass 2 gathers t = W .* (A'y), pass 1 gathers y.
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
            hit = np.isin(np.asarray(A.i), I)                   # entries in the rows I -> their columns -> those columns' rows
            entry_col = np.repeat(np.arange(n), np.diff(np.asarray(A.p)))
            mask = np.zeros(n, bool)
            mask[entry_col[hit]] = True
            allowed, got = np.union1d(rows_touching(A, mask), I), np.flatnonzero(~np.isfinite(lhs))
            assert got.size > 0 and np.isin(got, allowed).all(), (tag, name, "y", got[:8], allowed[:8])
            np.save("%s/%s_pad_y_%s.npy" % (out, tag, name), lhs)


def products_and_solve(tag, A, seed, maxiter=500, pad=True):
    m, n = A.nrow, A.ncol
    ctx = kkt.KktContext(A, device=0)
    info = inspect(tag, ctx)
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
        if pad:
            padding(tag, ctx, A, info, seed)
    ctx.close()


if group == "random":
    # 4, 2 and 8 slices, ragged last row blocks
    for (m, n, seed, kb) in ((9000, 20011, 1, "16"), (20000, 45000, 2, "128"), (60000, 130000, 7, "256")):
        os.environ["IPXK_SLICE_TEST_KB"] = kb
        if seed == 2:
            os.environ["IPXK_SLICE_FORCE2"] = "1"          # A'y: y of 160 KiB in two slices of 128 KiB
        products_and_solve("lp%d" % seed, synth.synthetic_lp(m, n, 8, seed), seed, pad=seed == 1)
        os.environ.pop("IPXK_SLICE_FORCE2", None)
elif group == "collide":
    os.environ["IPXK_SLICE_TEST_KB"] = "16"
    os.environ["IPXK_ACC_ROWS"] = "1024"
    products_and_solve("ragged", ragged_lp(3 * 1024 + 500, 11), 11, maxiter=60)
    products_and_solve("boundary", boundary_lp(12), 12, maxiter=60)
elif group == "tp":
    os.environ["IPXK_SLICE_TEST_KB"] = "16"
    os.environ["IPXK_ACC_ROWS"] = "4096"
    products_and_solve("tp", tp_lp(13), 13, maxiter=60)
elif group == "special":
    os.environ["IPXK_SLICE_TEST_KB"] = "16"
    products_and_solve("dense", synth.synthetic_lp(20000, 45000, 8, 6, num_dense=8), 6, pad=False)
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
elif group == "builders":
    # the host builders against the device builders (layout "auto"; the shapes of test_gpu_layout.py, whose layouts are acc + acc)
    os.environ["IPXK_SLICE_TEST_KB"] = "16"
    os.environ["IPXK_BUILD_ALL_LAYOUTS"] = "1"
    for (m, n, seed) in ((9000, 20011, 1), (33333, 70001, 3)):
        A = synth.synthetic_lp(m, n, 8, seed)
        ctxs = []
        for build in ("host", "device"):
            os.environ["IPXK_LAYOUT_BUILD"] = build
            ctxs.append(kkt.KktContext(A, device=0))
        inspect("lp%d" % seed, ctxs[1])                   # the device builder's against the definition
        for w in (0, 1):
            ih, idv = ctxs[0].layout_info(w)[0], ctxs[1].layout_info(w)[0]
            assert ih["acc_built"] == idv["acc_built"] == 1 and ih["acc_wide_units"] == idv["acc_wide_units"] > 0, (seed, w, ih, idv)
            for a in (21, 22, 23, 24):
                x, z = ctxs[0].layout_array(w, a), ctxs[1].layout_array(w, a)
                assert x.size > 0 and np.array_equal(x, z), (seed, w, a)
        for c in ctxs:
            c.close()
else:
    raise SystemExit("unknown group " + group)

with open(out + "/res.json", "w") as f:
    json.dump(res, f)
