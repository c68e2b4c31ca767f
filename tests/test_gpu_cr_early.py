"""GPU: the two vector kernels of the CR loop with their vector loads issued ahead of the loop scalars (the default)
against the order before (IPXK_CR_EARLY=0: the scalars one after another, then the loads), bit for bit.  Only the order of
the loads differs -- no floating-point operation, operand or summation order does -- so everything a solve returns (the
solution, the iteration count, the errflag, the residual-norm history) must be equal, not close, on every way out of the
loop.  The setting is read once per process: each order runs in a process of its own and leaves an .npz behind.

Legs: every case of tests/cr_lazy_worker.py (3000 rows: PcrDiag, PcrSmw and plain CR on the golden fixtures, the 202 and
203 exits, errflag 201 around a cycle boundary, no iteration, a nonzero start, the interrupt), its two-rank leg (the
reduction helper with stride > 1; a 205 exit whose non-finite scalars cross the all-gather), and tests/cr_early_worker.py (70001 rows: more than one partial per thread, a ragged last
workgroup) as it is, with IPXK_CR_LAZY=0 (the control kernel's loads of step and lhs) and with IPXK_SPMV_LAYOUT=plain
(2048 cdot partials: the reduction helper's eight loads per thread).  The legs at 70001 rows all name their SpMV layout: left
to itself a matrix of that size gets the fastest of several layouts by a timing on the spot, and with the layout the number
of cdot partials, hence the order of that sum, would differ from process to process."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAZY_WORKER = os.path.join(ROOT, "tests", "cr_lazy_worker.py")
EARLY_WORKER = os.path.join(ROOT, "tests", "cr_early_worker.py")
SETTINGS = ("0", "1")


def run_legs(worker, argv_of, out_arg, nprocs, env_extra, what):
    """one process per (setting, rank); argv_of(...)[out_arg] is the process's .npz; returns {setting: [npz per rank]}.
    Single-process legs run their two settings side by side, the ranks of a partitioned solve one setting after the other."""
    def start(e):
        return [subprocess.Popen([sys.executable, worker] + argv_of(e, r), env=dict(os.environ, IPXK_CR_EARLY=e, **env_extra),
                                 stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(nprocs)]

    def finish(procs):
        logs = []
        for p in procs:
            try:
                logs.append(p.communicate(timeout=240)[0])
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                pytest.fail("%s did not finish:\n%s" % (what, "\n".join(logs)))
        assert all(p.returncode == 0 for p in procs), "%s:\n%s" % (what, "\n".join(logs))

    if nprocs == 1:
        finish([p for e in SETTINGS for p in start(e)])
    else:
        for e in SETTINGS:
            finish(start(e))
    return {e: [dict(np.load(argv_of(e, r)[out_arg])) for r in range(nprocs)] for e in SETTINGS}


def all_equal(before, early, at_least):
    assert sorted(before) == sorted(early) and len(early) >= at_least
    for k in early:
        assert before[k].shape == early[k].shape and before[k].dtype == early[k].dtype, k
        if before[k].dtype.kind in "fc":
            assert np.array_equal(before[k], early[k], equal_nan=True), k
        else:
            assert np.array_equal(before[k], early[k]), k


@pytest.fixture(scope="module")
def library():
    from ipx_amd import kkt
    kkt.load_library()


def test_cases_of_the_lazy_worker(library, tmp_path):
    out = run_legs(LAZY_WORKER, lambda e, r: ["single", str(tmp_path / ("early%s.npz" % e))], 1, 1, {}, "single-rank leg")
    before, early = out["0"][0], out["1"][0]
    all_equal(before, early, 40)
    # the legs did what the cases are there for
    assert tuple(early["diag_200.it_err"])[1] == 0 and tuple(early["dense_300.it_err"])[1] == 0
    assert tuple(early["dense_300.neg.it_err"]) == (1, 202) and tuple(early["diag_200.neg.it_err"]) == (0, 203)
    for maxiter in (0, 1, 4, 5, 6, 11):
        assert tuple(early["synth.maxiter%d.it_err" % maxiter]) == (maxiter, 201)
        assert len(early["synth.maxiter%d.hist" % maxiter]) == maxiter + 1
    assert tuple(early["synth.tol0.it_err"]) == (0, 0) and tuple(early["synth.interrupt.it_err"]) == (10, 999)
    assert early["synth.lhs0.it_err"][1] == 0 and early["synth.kkt.it_err"][1] == 0 and early["basis_200.cr.it_err"][0] > 0


def big_legs(tmp_path, env_extra, what):
    out = run_legs(EARLY_WORKER, lambda e, r: [str(tmp_path / ("early%s.npz" % e))], 0, 1, env_extra, what)
    before, early = out["0"][0], out["1"][0]
    all_equal(before, early, 9)
    for maxiter in (5, 6):                                 # the rsdot reduction at k = 5 let the loop go on
        assert tuple(early["big.maxiter%d.it_err" % maxiter]) == (maxiter, 201)
        hist = early["big.maxiter%d.hist" % maxiter]
        assert len(hist) == maxiter + 1 and np.isfinite(hist).all() and np.any(early["big.maxiter%d.y" % maxiter] != 0.0)
    it, err = (int(v) for v in early["big.kkt.it_err"])
    assert err == 0 and it > 5 and np.isfinite(early["big.kkt.y"]).all()
    return early


def test_more_than_one_partial_per_thread(library, tmp_path):
    big_legs(tmp_path, {"IPXK_SPMV_LAYOUT": "acc"}, "70001 rows")


def test_update_in_the_control_kernel(library, tmp_path):
    big_legs(tmp_path, {"IPXK_SPMV_LAYOUT": "acc", "IPXK_CR_LAZY": "0"}, "70001 rows, IPXK_CR_LAZY=0")


def test_plain_layout_eight_partials_per_thread(library, tmp_path):
    early = big_legs(tmp_path, {"IPXK_SPMV_LAYOUT": "plain"}, "70001 rows, plain layout")
    if tuple(early["layout"]) != ("plain", "plain"):
        pytest.skip("IPXK_SPMV_LAYOUT=plain was not honoured at 70001 x 150001: the layout in use is %s" % (tuple(early["layout"]),))


def test_row_partitioned_two_ranks(library, tmp_path):
    world = 2
    out = run_legs(LAZY_WORKER, lambda e, r: ["rank", str(tmp_path / ("early%s.rank%d.npz" % (e, r))), str(r), str(world),
                                              str(tmp_path / ("uid" + e))], 1, world, {"IPXK_COMM": "direct"}, "2-rank leg")
    for r in range(world):
        all_equal(out["0"][r], out["1"][r], 5)
        assert tuple(out["1"][r]["rank.it_err"]) == (7, 201) and np.any(out["1"][r]["rank.y"] != 0.0)
        assert tuple(out["1"][r]["rank205.it_err"]) == (0, 205)      # overflow in cdot and pdot, on both ranks
