"""GPU: the persistent accumulated-tile kernel (spmv_acc_persist_kernel, workgroup w takes tiles w, w + G, ... and parks
the finished row sums in registers) against the one-tile-per-workgroup kernel (IPXK_ACC_PERSIST=0, which also keeps the
row blocks of 16384 rows instead of the ones that balance the persistent grid).  A row's partial sum is the same sequence
of ds_add_f64 in both, whatever the row block, so every product and every solve must agree bit for bit.  Each setting
runs in a process of its own (the setting is read once per process).  The small shapes run with the grid capped at 16
workgroups as well (IPXK_ACC_PERSIST=16), so that a workgroup walks many tiles: tiles of one to a few batches (the parked
sums of a tile still leaving when the next tile ends, and at the end of the walk), empty tiles between non-empty ones,
short last row blocks, 2 slices."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from ipx_amd import kkt, synth

case, out = sys.argv[2], sys.argv[3]
res = {}

def block_lp(m, n, seed):
    # the columns of each run of 1024 touch one of three bands of rows, in turn: row blocks of the transposed product whose
    # tiles in some slices are empty, between row blocks where they are not
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

def products_and_solve(tag, A, seed, maxiter=500):
    m, n = A.nrow, A.ncol
    ctx = kkt.KktContext(A, device=0)
    info = [ctx.layout_info(w)[0] for w in (0, 1)]
    res[tag + "_layout"] = [[d["use_acc"], d["acc_nslices"], d["acc_nrb"], d["acc_RB"], d["nlong"], d["acc_nbatches"]] for d in info]
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.1, 10.0, m + n)
    y = rng.standard_normal(m)
    ctx.normal_prepare(W)
    lhs, dot = ctx.normal_apply(y)            # EpiScale (A'y) and EpiNormalRows (A t)
    st = synth.synthetic_ipm_state(m, n, 1.0, seed)
    assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    x, yy, it, err, _ = ctx.kkt_diag_solve(st["a"], st["b"], 0.3 * np.sqrt(st["mu"]), maxiter)   # + EpiKktRhs, EpiRecoverX
    ctx.close()
    np.save("%s/%s_lhs.npy" % (out, tag), lhs)
    np.save("%s/%s_x.npy" % (out, tag), x)
    np.save("%s/%s_y.npy" % (out, tag), yy)
    res[tag + "_scalars"] = [float(dot).hex(), int(it), int(err)]

if case == "small":
    import os
    os.environ["IPXK_SPMV_LAYOUT"] = "acc"
    # slices of 16 to 128 KiB: 2, 4 and 8 slices, ragged last row blocks
    for (m, n, seed, kb) in ((9000, 20011, 1, "16"), (20000, 45000, 2, "128"), (33333, 70001, 3, "128"), (70001, 150007, 4, "256"),
                             (60000, 130000, 7, "16")):
        os.environ["IPXK_SLICE_TEST_KB"] = kb
        if seed == 2:
            os.environ["IPXK_SLICE_FORCE2"] = "1"          # A'y: y of 160 KiB in two slices of 128 KiB
        products_and_solve("lp%d" % seed, synth.synthetic_lp(m, n, 8, seed), seed)
        os.environ.pop("IPXK_SLICE_FORCE2", None)
    os.environ["IPXK_SLICE_TEST_KB"] = "16"
    products_and_solve("block", block_lp(30000, 40000, 5), 5)
    products_and_solve("dense", synth.synthetic_lp(20000, 45000, 8, 6, num_dense=8), 6)
    # basis path: the N N' products of the basis preconditioner
    B = synth.planted_lu_basis(synth.synthetic_lp(20000, 45000, 8, 8), seed=8, num_free=2)
    cs = synth.synthetic_basis_state(B["status"], 1.0, 8)
    ctx = kkt.KktContext(B["A"], device=0)
    ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], cs)
    st = synth.synthetic_ipm_state(20000, 45000, 1.0, 8)
    xb, yb, itb, errb, _ = ctx.kkt_basis_solve(st["a"], st["b"], 1e-8)
    ctx.close()
    np.save(out + "/basis_x.npy", xb)
    np.save(out + "/basis_y.npy", yb)
    res["basis_scalars"] = [int(itb), int(errb)]
else:
    products_and_solve("c3", synth.synthetic_lp(1000000, 2000000, 8, 12345), 12345)

with open(out + "/res.json", "w") as f:
    json.dump(res, f)
"""


def _run(case, persist, tmp_path):
    """persist: the IPXK_ACC_PERSIST setting ("0": one workgroup per tile)"""
    out = tmp_path / ("%s_%s" % (case, persist))
    out.mkdir()
    env = dict(os.environ, IPXK_ACC_PERSIST=persist)
    subprocess.run([sys.executable, "-c", WORKER, ROOT, case, str(out)], env=env, check=True, timeout=900)
    with open(out / "res.json") as f:
        return out, json.load(f)


def _compare(case, tmp_path, persist="1", d0r0=None):
    d0, r0 = d0r0 or _run(case, "0", tmp_path)
    d1, r1 = _run(case, persist, tmp_path)
    for k in r0:
        if k.endswith("_layout"):
            # the same products through the accumulated tiles in both; the row blocks may differ
            assert [l[0] for l in r0[k]] == [l[0] for l in r1[k]], (k, r0[k], r1[k])
            assert [l[1] for l in r0[k]] == [l[1] for l in r1[k]], (k, r0[k], r1[k])
        else:
            assert r0[k] == r1[k], (k, r0[k], r1[k])
    files = sorted(p.name for p in d0.glob("*.npy"))
    assert files == sorted(p.name for p in d1.glob("*.npy")) and files
    for name in files:
        a, b = np.load(d0 / name), np.load(d1 / name)
        assert a.shape == b.shape and np.array_equal(a, b), name
    return (d0, r0), r1


def test_persistent_tiles_equal_one_tile_per_workgroup_ragged_shapes(tmp_path):
    base, r1 = _compare("small", tmp_path, "1")
    _, r16 = _compare("small", tmp_path, "16", base)
    acc = [l for k, v in r16.items() if k.endswith("_layout") for l in v if l[0]]
    assert acc, r16
    assert {2, 8} <= {l[1] for l in acc}, acc                   # 2 and 8 slices among the shapes
    assert any(l[3] % 1024 for l in acc), acc                   # balanced row blocks (not a power of two)
    # with 16 workgroups: products of many tiles per workgroup, among them tiles of fewer than 8 batches (the parked
    # sums leave at the next boundary or at the end), and a row block that does not divide the rows
    multi = [l for l in acc if l[1] * l[2] >= 4 * 16]
    assert multi and any(l[5] < 8 * l[1] * l[2] for l in multi), acc
    assert any(l[1] == 2 for l in multi), acc
    assert r16["block_layout"][0][0] or r16["block_layout"][1][0], r16


def test_persistent_tiles_equal_one_tile_per_workgroup_c3(tmp_path):
    (_, r0), r1 = _compare("c3", tmp_path)
    assert all(l[0] == 1 for l in r1["c3_layout"]), r1
    assert r1["c3_scalars"][2] == 0
    # the persistent path's row blocks (grid-balanced, even, not the 16384 of the one-tile kernel) were in use
    for l0, l1 in zip(r0["c3_layout"], r1["c3_layout"]):
        assert l0[3] == 16384 and l1[3] != l0[3] and l1[3] % 2 == 0 and l1[3] >= 14336, (l0, l1)
