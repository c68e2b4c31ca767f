"""GPU: the combine kernel of the sliced and accumulated layouts with a row group's loads issued before the first
add (the default) against the form before (IPXK_COMBINE_EARLY=0: per row the flag, the epilogue's inputs and one partial
sum after the other, each waited for), bit for bit.  Only the order of the loads differs -- the slices of a row are added
in ascending order, a thread's rows contribute to its dot partial in ascending order, the grid and the thread-to-row map
are the same -- so every product, every dot and everything a solve returns must be equal, not close.  The setting is read
once per process: each form runs in a process of its own (tests/combine_loads_worker.py) and leaves an .npz behind.

Legs: IPXK_SPMV_LAYOUT = acc, sliced (the two that end in the combine kernel; without the accumulated tiles
the N N' products of the basis path take nmatrix.hip's sliced tiles), each on the kernel's own grid -- at most one row per
thread at these sizes, so a group with one live row and clamped loads for the rest -- and with IPXK_COMBINE_GRID=4: a
thread owns 8 to 9 rows of the 9000-row product and up to 69 of the largest, full groups and a ragged last one, some
threads of a workgroup with a row in the last group and some without.  The shapes build 2, 4 and 8 slices (R = 4, 4, 2
rows per group); one more leg runs the form for any slice count on them (IPXK_COMBINE_GENERIC=1)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "combine_loads_worker.py")
SETTINGS = ("0", "1")
LP_TAGS = ("lp1", "lp2", "lp3")


def run_legs(tmp_path, layout, env_extra):
    """the two forms side by side, one process each; returns ({setting: arrays}, {setting: log})"""
    env = dict(os.environ, IPXK_SPMV_LAYOUT=layout, IPXK_VERBOSE="1", **env_extra)
    if layout != "acc":
        env["IPXK_SPMV_ACC"] = "0"
    files = {e: str(tmp_path / ("early%s.npz" % e)) for e in SETTINGS}
    procs = {e: subprocess.Popen([sys.executable, WORKER, files[e]], env=dict(env, IPXK_COMBINE_EARLY=e), stdout=subprocess.PIPE,
                                 stderr=subprocess.STDOUT, text=True) for e in SETTINGS}
    logs = {}
    for e, p in procs.items():
        try:
            logs[e] = p.communicate(timeout=240)[0]
        except subprocess.TimeoutExpired:
            for q in procs.values():
                q.kill()
            pytest.fail("the leg IPXK_COMBINE_EARLY=%s did not finish:\n%s" % (e, "\n".join(logs.values())))
    assert all(p.returncode == 0 for p in procs.values()), "\n".join(logs.values())
    return {e: dict(np.load(files[e])) for e in SETTINGS}, logs


def all_equal(before, early):
    assert sorted(before) == sorted(early) and len(early) >= 30
    for k in early:
        assert before[k].shape == early[k].shape and before[k].dtype == early[k].dtype, k
        if before[k].dtype.kind in "fc":
            assert np.array_equal(before[k], early[k], equal_nan=True), k
        else:
            assert np.array_equal(before[k], early[k]), k


def check(tmp_path, layout, env_extra):
    out, logs = run_legs(tmp_path, layout, env_extra)
    before, early = out["0"], out["1"]
    all_equal(before, early)
    # the legs ran what they are there for: the forced layout on both products of every shape, 2, 4 and 8 slices among
    # them, long rows in the dense case's A'y, solves that converged, N N' on N as a matrix of its own
    for tag in LP_TAGS + ("dense",):
        if tag == "dense":          # (a product with long rows may keep the sliced tiles: the combine kernel all the same)
            assert early[tag + ".layout"][0] in ("sliced", layout) and early[tag + ".layout"][1] == layout, early[tag + ".layout"]
            assert min(early[tag + ".nslices"]) > 1, early[tag + ".nslices"]
        else:
            assert tuple(early[tag + ".layout"]) == (layout, layout), (tag, early[tag + ".layout"])
        assert early[tag + ".it_err"][1] == 0 and early[tag + ".it_err"][0] > 0, (tag, early[tag + ".it_err"])
        assert np.isfinite(early[tag + ".lhs"]).all() and np.any(early[tag + ".lhs"] != 0.0)
    assert tuple(early["lp1.nslices"]) == (8, 8) and tuple(early["lp2.nslices"]) == (2, 4) and tuple(early["lp3.nslices"]) == (4, 8), \
        [early[t + ".nslices"] for t in LP_TAGS]
    assert early["dense.nlong"][0] > 0, early["dense.nlong"]
    assert np.any(early["dense.smw_lhs"] != 0.0)
    assert early["basis.it_err"][1] == 0 and early["basis.it_err"][0] > 0
    for log in logs.values():
        assert "N built on the device" in log, log
    return early


@pytest.fixture(scope="module")
def library():
    from ipx_amd import kkt
    kkt.load_library()


@pytest.mark.parametrize("layout", ("acc", "sliced"))
def test_one_group_per_thread(library, tmp_path, layout):
    check(tmp_path, layout, {})


@pytest.mark.parametrize("layout", ("acc", "sliced"))
def test_several_groups_per_thread(library, tmp_path, layout):
    check(tmp_path, layout, {"IPXK_COMBINE_GRID": "4"})


def test_form_for_any_slice_count(library, tmp_path):
    check(tmp_path, "acc", {"IPXK_COMBINE_GRID": "4", "IPXK_COMBINE_GENERIC": "1"})
