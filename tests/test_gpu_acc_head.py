"""GPU: the persistent accumulated-tile kernel with the load that warms its slice (IPXK_ACC_WARM, the default) and started from
the HEAD tables (IPXK_ACC_HEAD=1; off by default: profiles/acc_cold_start.txt), each against the kernel without.  The HEAD tables (internal.hpp: a workgroup's first six step
records, the walker's state behind them and the stream loads of its first three steps at addresses formed of blockIdx.x and
threadIdx.x; with IPXK_ACC_WARM one more load per thread, of a line of the slice) against the same kernel finding its way
through tile_step -> steps -> the wide stream (IPXK_ACC_HEAD=0, the default: no head is built).  Behind the prologue the kernel holds the
same registers and runs the same loop, so every row sum is the same sequence of ds_add_f64 between the same barriers and
every product and every solve must agree byte for byte, the sign of zeros included.

Each setting runs in processes of its own (tests/acc_head_worker.py; the settings are read once per process): IPXK_ACC_WIDE
{0, 1} x IPXK_ACC_STEPS {0, 1} x IPXK_ACC_PERSIST {1, 16, 8} x IPXK_ACC_WARM {0, 1}; the reference side (IPXK_ACC_HEAD=0
IPXK_ACC_WARM=0: the kernel as it was before either) is computed once per (wide, steps, persist).  The warming load on the
kernel that walks the tables (IPXK_ACC_HEAD=0 IPXK_ACC_WARM=1, what a default process runs) is compared with the same reference.

Shapes.  "rows4096": the crafted "tp" matrix, 32 x 8 tiles of 4096 rows -- on the full grid one tile per workgroup: first steps of
1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047 and 2048 entries, workgroups whose only tile is empty, workgroups of exactly 1,
2, 3, 4, 6 and 7 steps (fewer than the prologue's three, fewer than the head's six, and the walker handed over exactly at the
seventh); on 16 and 8 workgroups 16 and 32 tiles each, the first one empty for some.  "rows1024": "ragged" and "boundary" (steps
of several batches among a workgroup's first three; 16 and 8 tiles, fewer than any grid, so the grid is the tile count), random
LPs with 4, 2 and 8 slices and ragged last row blocks (472 tiles on 256 workgroups), and the basis path's N N' on three random LPs
(the planted factors of synth.planted_lu_basis are made for a random LP, not for the crafted matrices, which get the diag solve
only).  One slice is the fused form: the accumulated tiles are not built for fewer than two slices, so it has no head, no
warming load and is not touched.

The workers recompute head and head_wide in numpy from tile_step, steps, wide_start, wide and the grid by their definition
and compare with what the library built; with IPXK_ACC_HEAD=0 both are empty.  "tp" and one random LP get a NaN (an inf) at
offset 0 of every slice of the gathered vector -- what padding lanes and empty steps gather and never add."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "acc_head_worker.py")
TP_SIZES = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048]
GROUPS = {"rows4096": ["tp"], "rows1024": ["basis", "basis1", "basis2", "boundary", "lp1", "lp2", "lp7", "ragged"]}


def _run(group, out, **env):
    out.mkdir()
    subprocess.run([sys.executable, WORKER, ROOT, group, str(out)], env=dict(os.environ, **env), check=True, timeout=600)
    with open(out / "res.json") as f:
        return out, json.load(f)


@pytest.fixture(scope="module")
def without_head(tmp_path_factory):
    """Every shape with IPXK_ACC_HEAD=0 IPXK_ACC_WARM=0: once per (group, wide, steps, persist), shared by all other settings."""
    cache = {}

    def get(group, wide, steps, persist):
        key = (group, wide, steps, persist)
        if key not in cache:
            cache[key] = _run(group, tmp_path_factory.mktemp("head0") / "out", IPXK_ACC_HEAD="0", IPXK_ACC_WARM="0", IPXK_ACC_WIDE=wide,
                              IPXK_ACC_STEPS=steps, IPXK_ACC_PERSIST=persist)
        return cache[key]
    return get


@pytest.mark.parametrize("warm", ["0", "1"])
@pytest.mark.parametrize("persist", ["1", "16", "8"])
@pytest.mark.parametrize("steps", ["1", "0"])
@pytest.mark.parametrize("wide", ["1", "0"])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_head_start_equals_walked_start(group, wide, steps, persist, warm, tmp_path, without_head):
    d0, r0 = without_head(group, wide, steps, persist)
    d1, r1 = _run(group, tmp_path / "head1", IPXK_ACC_HEAD="1", IPXK_ACC_WARM=warm, IPXK_ACC_WIDE=wide, IPXK_ACC_STEPS=steps,
                  IPXK_ACC_PERSIST=persist)
    # the same tiles, batches and steps; byte-equal products, solves, iteration counts and flags (the padding runs among them)
    assert sorted(r0) == sorted(r1)
    for k in r0:
        if not k.endswith("_head"):
            assert r0[k] == r1[k], (k, r0[k], r1[k])
    files = sorted(p.name for p in d0.glob("*.npy"))
    assert files == sorted(p.name for p in d1.glob("*.npy")) and files
    for name in files:
        assert (d0 / name).read_bytes() == (d1 / name).read_bytes(), name
    # every shape went through the accumulated tiles in both products, with a head (checked against its definition by the
    # worker) on one side and none on the other
    acc = [(k[:-len("_layout")], w) for k in sorted(r1) if k.endswith("_layout") for w, l in enumerate(r1[k]) if l[0]]
    assert sorted({t for t, _ in acc}) == GROUPS[group], acc
    seen = {}
    for tag, w in acc:
        assert r0[tag + "_head"][w] is None and r1[tag + "_head"][w] is not None, (tag, w)
        seen[tag, w] = r1[tag + "_head"][w]
    assert any("_pad_w_nan" in f for f in files) and any("_pad_y_inf" in f for f in files), files
    # the cases the prologue can get wrong, as the tables read back show them
    if group == "rows4096":
        s = seen["tp", 1]
        assert r1["tp_layout"][1][1:4] == [8, 32, 4096] and s["ntiles"] == 256, (r1["tp_layout"], s)
        if persist == "1":
            assert s["P"] == 256 and s["tiles_per_wg"] == 1 and s["only_tile_empty"] > 0, s
            assert {0} | set(TP_SIZES) <= set(s["first_ne"]), s
            assert {1, 2, 3, 4, 6, 7} <= set(s["steps_per_wg"]), s
        else:
            assert s["P"] == int(persist) and s["tiles_per_wg"] == 256 // int(persist) and s["first_tile_empty"] > 0, s
            assert s["only_tile_empty"] == 0 and min(s["steps_per_wg"]) > 7, s
    else:
        # (1 slice cannot occur: the accumulated tiles are built for two slices or more, one slice is the fused form)
        slices = {r1[t + "_layout"][w][1] for t, w in acc}
        assert {2, 4, 8} <= slices, slices
        for tag in ("ragged", "boundary"):           # fewer tiles than workgroups: the grid is the tile count (or the cap)
            for w in (w_ for t_, w_ in acc if t_ == tag):
                s = seen[tag, w]
                assert s["ntiles"] <= 16 and s["P"] == (min(s["ntiles"], 8) if persist == "8" else s["ntiles"]), (tag, w, s)
        if steps == "1":
            assert seen["ragged", 1]["batches_in_head_step"] > 1 and seen["boundary", 1]["batches_in_head_step"] > 1, seen
        s = seen["lp7", 1]
        assert s["ntiles"] > 256 and s["tiles_per_wg"] >= (2 if persist == "1" else 256 // int(persist)), s


@pytest.mark.parametrize("persist", ["1", "16", "8"])
@pytest.mark.parametrize("steps", ["1", "0"])
@pytest.mark.parametrize("wide", ["1", "0"])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_warming_load_changes_nothing(group, wide, steps, persist, tmp_path, without_head):
    """The default: no head, the kernel that walks the tables with the warming load in front, against the same kernel without it."""
    d0, r0 = without_head(group, wide, steps, persist)
    d1, r1 = _run(group, tmp_path / "warm", IPXK_ACC_HEAD="0", IPXK_ACC_WARM="1", IPXK_ACC_WIDE=wide, IPXK_ACC_STEPS=steps, IPXK_ACC_PERSIST=persist)
    assert r0 == r1
    files = sorted(p.name for p in d0.glob("*.npy"))
    assert files == sorted(p.name for p in d1.glob("*.npy")) and files
    for name in files:
        assert (d0 / name).read_bytes() == (d1 / name).read_bytes(), name
    assert any("_pad_w_nan" in f for f in files) and any("_pad_y_inf" in f for f in files), files


def test_host_and_device_builders_give_the_same_head(tmp_path):
    _, r = _run("builders", tmp_path / "builders", IPXK_ACC_HEAD="1")
    assert all(s is not None and s["P"] > 0 for s in r["lp1_head"]), r
