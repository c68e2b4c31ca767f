"""GPU: the CR loop with the solution update deferred to the direction kernel (the default) against the loop
with the update in the control kernel (IPXK_CR_LAZY=0), bit for bit.  lhs += alpha*step is the same
multiply and add on the same operands in both orders, one kernel later in the deferred one, so everything a
solve returns -- the solution, the iteration count, the errflag, the residual-norm history -- must be equal,
not close, on every way out of the loop.  The setting is read once per process: each order runs in a process of
its own (tests/cr_lazy_worker.py) and leaves an .npz behind.

A 202 exit: the golden fixtures' indefinite weight vector gives one on dense_300 (at k = 1, after one solution
update) and a 203 on diag_200 (at k = 0); both are in.  The two-rank leg ends its second solve with a 205 at k = 0
(overflow in cdot and pdot); the 204 exit and the 205 and 202 exits of the three modes on one rank are in
tests/test_gpu_cr_exits.py, which runs both orders of the update too."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "cr_lazy_worker.py")


def run_legs(argv_of, nprocs, env_extra, what):
    """one process per (order, rank); returns {order: [npz per rank]}"""
    res = {}
    for lazy in ("0", "1"):
        env = dict(os.environ, IPXK_CR_LAZY=lazy, **env_extra)
        procs = [subprocess.Popen([sys.executable, WORKER] + argv_of(lazy, r), env=env, stdout=subprocess.PIPE,
                                  stderr=subprocess.STDOUT, text=True) for r in range(nprocs)]
        logs = []
        for p in procs:
            try:
                logs.append(p.communicate(timeout=240)[0])
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                pytest.fail("%s, IPXK_CR_LAZY=%s did not finish:\n%s" % (what, lazy, "\n".join(logs)))
        assert all(p.returncode == 0 for p in procs), "\n".join(logs)
        res[lazy] = [argv_of(lazy, r)[1] for r in range(nprocs)]
    return {lazy: [dict(np.load(f)) for f in files] for lazy, files in res.items()}


@pytest.fixture(scope="module")
def legs(tmp_path_factory):
    from ipx_amd import kkt
    kkt.load_library()
    d = tmp_path_factory.mktemp("cr_lazy")
    out = run_legs(lambda lazy, r: ["single", str(d / ("lazy%s.npz" % lazy))], 1, {}, "single-rank leg")
    return out["0"][0], out["1"][0]


def same(eager, lazy, name, hist=True):
    keys = [name + ".y", name + ".it_err"] + ([name + ".hist"] if hist else [])
    for k in keys:
        assert eager[k].shape == lazy[k].shape and np.array_equal(eager[k], lazy[k], equal_nan=True), k
    it, err = (int(v) for v in lazy[name + ".it_err"])
    return lazy[name + ".y"], it, err, lazy.get(name + ".hist")


def test_both_legs_ran_the_same_cases(legs):
    eager, lazy = legs
    assert sorted(eager) == sorted(lazy) and len(eager) >= 40


@pytest.mark.parametrize("name,mode_check", [("diag_200", 0), ("dense_300", 4)])
def test_golden_pcr(legs, name, mode_check):
    """PcrDiag (no dense column) and PcrSmw (4 dense columns), converged runs of ~130 iterations"""
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    assert int(d["num_dense"]) == mode_check
    y, it, err, hist = same(*legs, name)
    assert err == 0 and abs(it - int(d["pcr_iter"])) <= 2 and len(hist) == it + 1 and np.any(y != 0.0)


def test_indefinite_weights_202_and_203(legs):
    d2, d3 = (np.load(os.path.join(ROOT, "tests", "golden", n + ".npz")) for n in ("dense_300", "diag_200"))
    y, it, err, hist = same(*legs, "dense_300.neg")
    assert (it, err) == (int(d2["neg_iter"]), int(d2["neg_err"])) == (1, 202)
    assert np.any(y != 0.0) and len(hist) == 2            # the update of iteration 0 is in lhs
    y, it, err, hist = same(*legs, "diag_200.neg")
    assert (it, err) == (int(d3["neg_iter"]), int(d3["neg_err"])) == (0, 203)
    assert not np.any(y) and len(hist) == 1               # no update was made


def test_golden_basis_plain_cr(legs):
    d = np.load(os.path.join(ROOT, "tests", "golden", "basis_200.npz"))
    xy, it, err, _ = same(*legs, "basis_200.kkt", hist=False)
    assert err == 0 and it > 0 and np.isfinite(xy).all()
    y, it, err, hist = same(*legs, "basis_200.cr")
    assert (it, err) == (int(d["cr_iter"]), int(d["cr_err"])) and len(hist) == it + 1


@pytest.mark.parametrize("maxiter", [0, 1, 4, 5, 6, 11])
def test_iteration_limit_around_a_cycle_boundary(legs, maxiter):
    y, it, err, hist = same(*legs, "synth.maxiter%d" % maxiter)
    assert (it, err) == (maxiter, 201) and len(hist) == maxiter + 1
    assert np.any(y != 0.0) == (maxiter > 0)              # exactly the updates of iterations 0 .. maxiter-1
    if maxiter > 0:                                       # one update more than the shorter run: the last one is not lost
        prev = legs[1]["synth.maxiter%d.y" % {1: 0, 4: 1, 5: 4, 6: 5, 11: 6}[maxiter]]
        assert not np.array_equal(y, prev)


def test_run_that_needs_no_iteration(legs):
    y, it, err, hist = same(*legs, "synth.tol0")
    assert (it, err) == (0, 0) and not np.any(y) and len(hist) == 1


def test_nonzero_starting_iterate(legs):
    y, it, err, hist = same(*legs, "synth.lhs0")
    assert err == 0 and it > 5 and len(hist) == it + 1 and hist[-1] <= 1e-8


def test_interrupted_single_rank(legs):
    """the callback is polled before the cycles 1, 2, ...: its second call ends the loop after two cycles"""
    y, it, err, hist = same(*legs, "synth.interrupt")
    assert (it, err) == (10, 999) and len(hist) == 10 and int(legs[1]["synth.interrupt.calls"][0]) == 2
    assert np.any(y != 0.0)


def test_kkt_diag_solve(legs):
    xy, it, err, _ = same(*legs, "synth.kkt", hist=False)
    assert err == 0 and it > 5 and np.isfinite(xy).all()


def test_row_partitioned_two_ranks(tmp_path, oracle):
    """every rank's x and y, bit for bit between the two orders; errflag 201 after 7 iterations on both ranks, then
    errflag 205 at k = 0 on both ranks for a right-hand side whose cdot and pdot overflow"""
    from cr_lazy_worker import RANK_PROBLEM
    from ipx_amd import kkt, synth
    from oracle import pyoracle as po
    kkt.load_library()
    m, n, seed = RANK_PROBLEM
    A, st = synth.synthetic_lp(m, n, 8, seed), synth.synthetic_ipm_state(m, n, 1.0, seed)
    ko = oracle.kkt_diag(po.Csc(m, n, A.p, A.i, A.x), precond_dense_cols=False, maxiter=200)
    assert ko.factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    xo, yo, ito, erro, _ = ko.solve(st["a"] * 1e160, st["b"] * 1e160, 1e-30)
    assert (ito, erro) == (0, 205) and not np.any(yo) and np.isfinite(xo).all()
    world = 2
    out = run_legs(lambda lazy, r: ["rank", str(tmp_path / ("lazy%s.rank%d.npz" % (lazy, r))), str(r), str(world),
                                    str(tmp_path / ("uid" + lazy))], world, {"IPXK_COMM": "direct"}, "2-rank leg")
    for r in range(world):
        xy, it, err, _ = same(out["0"][r], out["1"][r], "rank", hist=False)
        assert (it, err) == (7, 201) and np.any(xy != 0.0)
        xy, it, err, _ = same(out["0"][r], out["1"][r], "rank205", hist=False)
        ny = int(out["1"][r]["rank205.ny"][0])
        assert (it, err) == (0, 205) and not np.any(xy[-ny:]) and np.isfinite(xy[:-ny]).all()      # y zero, x finite
