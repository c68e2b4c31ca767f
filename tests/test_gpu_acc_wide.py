"""GPU: the persistent accumulated-tile kernel reading the WIDE stream (internal.hpp: per thread and step three 16-byte
loads of a derived copy of the entries) against the same kernel streaming pack / val (IPXK_ACC_WIDE=0: no copy is built).
Thread t of a step's Tp threads holds the sorted positions u Tp + t; which thread adds an entry cannot change a row sum
(the rows of a batch are distinct), so a row's partial sum is the same sequence of ds_add_f64 between the same barriers
in both and every product and every solve must agree byte for byte; the products must also equal the sliced layout's.
Each setting runs in a process of its own (tests/acc_wide_worker.py; the settings are read once per process), each shape
with the kernel's own grid and with the grid capped at 16 workgroups, with a tile's tail batches merged into steps and
with a step per batch.

Shapes (the small ones of test_gpu_acc_steps.py): "random" = random LPs with 4, 2 and 8 slices; "collide" = rows of
1 .. 40 entries in one slice with 1024-row tiles, and the 1024 + 1024 (+ 1) boundary; "special" = 8 dense columns, and the
basis path's N N'; "tp" = a crafted matrix with 4096-row tiles whose steps hold 1, 63, 64, 65, 255, 256, 257, 511, 512,
513, 2047 and 2048 entries (every Tp from one wavefront to eight, and both sides of each boundary), with empty tiles.

The workers recompute the wide stream from pack, val and the step table by its definition, and give the gathered
vector a NaN (an inf) at offset 0 of every slice -- what a padding position gathers: only rows with an entry there may be
non-finite, and the results are compared with IPXK_ACC_WIDE=0 byte for byte like everything else (the sign of zeros
included)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "acc_wide_worker.py")
TP_SIZES = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048]
TAGS = {"random": ["lp1", "lp2", "lp7"], "collide": ["boundary", "ragged"], "special": ["basis", "dense"], "tp": ["tp"]}


def _run(group, tmp, name, layout, **env):
    out = tmp / name
    out.mkdir()
    subprocess.run([sys.executable, WORKER, ROOT, group, str(out), layout], env=dict(os.environ, **env), check=True, timeout=600)
    with open(out / "res.json") as f:
        return out, json.load(f)


@pytest.fixture(scope="module")
def sliced_products(tmp_path_factory):
    """The products of every shape through the sliced layout: once per group, shared by all settings."""
    cache = {}

    def get(group):
        if group not in cache:
            cache[group] = _run(group, tmp_path_factory.mktemp("sliced_" + group), "sliced", "sliced")
        return cache[group]
    return get


@pytest.mark.parametrize("steps", ["1", "0"])
@pytest.mark.parametrize("persist", ["1", "16"])
@pytest.mark.parametrize("group", ["random", "collide", "special", "tp"])
def test_wide_stream_equals_narrow_stream(group, persist, steps, tmp_path, sliced_products):
    d0, r0 = _run(group, tmp_path, "wide0", "acc", IPXK_ACC_PERSIST=persist, IPXK_ACC_STEPS=steps, IPXK_ACC_WIDE="0")
    d1, r1 = _run(group, tmp_path, "wide1", "acc", IPXK_ACC_PERSIST=persist, IPXK_ACC_STEPS=steps, IPXK_ACC_WIDE="1")
    # the same tiles, batches and steps; byte-equal products, solves, iteration counts and flags (the padding runs among them)
    assert sorted(r0) == sorted(r1)
    for k in r0:
        if not k.endswith("_wide"):
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
    # every shape went through the accumulated tiles and a wide stream with short steps (padding positions) in it
    acc = [(k[:-len("_layout")], w) for k in sorted(r1) if k.endswith("_layout") for w, l in enumerate(r1[k]) if l[0]]
    assert sorted({t for t, _ in acc}) == TAGS[group], acc
    for tag, w in acc:
        seen0, seen1 = r0[tag + "_wide"][w], r1[tag + "_wide"][w]
        assert seen0 is None and seen1 is not None and seen1["short_steps"] > 0, (tag, w, seen0, seen1)
    if group in ("random", "tp"):
        pads = [f for f in files if "_pad_" in f]
        assert any("_pad_w_nan" in f for f in pads) and any("_pad_y_inf" in f for f in pads), files
    if group == "random":
        assert {2, 8} <= {l[1] for k in r1 if k.endswith("_layout") for l in r1[k] if l[0]}, r1
    if group == "tp":
        (seen,) = [r1["tp_wide"][w] for tag, w in acc if w == 1]
        assert r1["tp_layout"][1][3] == 4096 and seen["empty_tiles"] > 0, (r1["tp_layout"], seen)
        assert set(TP_SIZES) <= set(seen["ne"]), seen["ne"]


def test_host_and_device_builders_give_the_same_wide_stream(tmp_path):
    _, r = _run("builders", tmp_path, "builders", "auto")
    for tag in ("lp1", "lp3"):
        assert all(s is not None and s["nsteps"] > 0 for s in r[tag + "_wide"]), r
