"""GPU: the two drivers of the CR loop (ipx_amd/csrc/cr.hip) and the refresh of every fifth iteration inside the direction
kernel, at every way out of the loop.

Drivers.  Single rank, the host follows a progress word the direction kernel stores and enqueues iteration k once
iteration k - R has finished (R: IPXK_CR_AHEAD); IPXK_CR_PACE=cycles is the driver before, cycles of 5 iterations with a
snapshot kernel and an event each.  IPXK_CR_REFRESH=0 keeps the refresh sresidual = residual ./ diag (with the partials of
residual'*sresidual) a launch of its own; by default the direction kernel of the iterations with (k + 1) % 5 == 0 makes
it.  Neither changes a floating-point operation, so for each IPXK_CR_GRID in {unset, 1, 2} (which sets the partition of the
partial sums) the eight legs (cycles, default) x AHEAD (1, 3) x REFRESH (0, 1) must agree bit for bit, NaN included, on
y, (iterations, errflag), the history and ipxk_cr_diagnostics.  Leg 0 (cycles, REFRESH=0) is the code path before.

Cases (tests/cr_pacing_worker.py), with 1024, 1025 and 3000 rows: under grid 1 and 2 a thread has exactly one group of
kCrUnroll = 4 elements, a fifth element, and three groups with a ragged last one, so the fused refresh's later groups and
its sums over two partials run.
  * exit through tol at k = 4, 5, 6, 9, 10, 11 (every residue mod 5 next to a refresh).  The reference's history is not
    monotone, so each (rows, k) has a right-hand side whose norm at k is at least 5 % below every earlier one, and
    tol = sqrt(hist[k] * min(hist[:k])): 2.4 % from either, against 1e-12 between the device and the reference.
  * 201 at maxiter 0, 1, 4, 5, 6.
  * 204 at iteration 5 on the overflow input of tests/test_gpu_cr_exits.py (the fused refresh must produce the same inf),
    205 and 202 at k = 0.
  * the callback returns nonzero at its second poll: both drivers have then enqueued exactly 10 iterations.
  * one PcrSmw and one plain-CR run (the paced driver without the fused refresh), held to the oracle at the gates of
    tests/test_gpu_parity.py.
The PcrDiag cases are held to tests/cr_reference.py (extended precision) at 1e-12, the operator-level parity gate.

Launch accounting (ipxk_cr_loop_stats) of every progress-paced leg: no snapshot, no event inside the loop, and at most
iterations + 1 + R iterations enqueued -- the host enqueues k only after iteration k - R has finished, and the final
iteration K never finishes, so k <= K + R whatever the timing.  Launches: the counter holds the launches of the loop's own
kernels (the operator's depend on the SpMV layout and are its routine's).  PcrDiag: 2 per enqueued iteration (control,
direction) plus 5 (residual, preconditioner, state, first direction; the flush), plus with REFRESH=0 one per enqueued
iteration with (k + 1) % 5 == 0.

Measured on an MI355X: the tol cases' y and history within 1.1e-15 of the reference in every grid; on these small systems
the host is always ahead, so at an exit through tol a paced leg enqueues exactly iterations + 1 + R (3000 rows, exit
at 11: 15 with R = 3, against 20 by the cycles)."""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import cr_reference
from cr_exits_worker import DIAG_FIELDS, PLAIN_SHAPE, SEED, SHAPES, SMALL_204, diag_inputs, plain_inputs
from cr_pacing_worker import CALLBACK_FLAG, MAXITER_EXITS, OTHER_MAXITER, TOL_EXITS, tol_rhs
from helpers import relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "cr_pacing_worker.py")
GRIDS = ("", "1", "2")                                   # IPXK_CR_GRID; "": unset
# (IPXK_CR_PACE, IPXK_CR_AHEAD, IPXK_CR_REFRESH); "": unset.  Leg 0 is the code path before.
LEGS = tuple(itertools.product(("cycles", ""), ("1", "3"), ("0", "1")))
NCOLS = dict(SHAPES)
ROWS = [s[0] for s in SHAPES]
HEAD_TAIL = 5                                            # launches of a PcrDiag run outside its iterations


def dist(a, b):
    """max |a - b| / max |b| with b in extended precision"""
    b = np.asarray(b, dtype=np.longdouble)
    return float(np.abs(np.asarray(a, dtype=np.longdouble) - b).max() / np.abs(b).max())


# ---- CPU side: computed once, shared by every grid and leg ----
@functools.lru_cache(maxsize=None)
def tol_reference(m, k):
    """(tol, the reference run with it): the loop must end at k"""
    A, W, resscale, _ = diag_inputs(m, NCOLS[m])
    rhs = tol_rhs(m, k)
    h = cr_reference.pcr(A, W, W, rhs, 1e-30, resscale, k).hist
    assert len(h) == k + 1 and h[:k].min() >= 1.05 * h[k], (m, k, h)
    tol = float(np.sqrt(h[k] * h[:k].min()))
    ref = cr_reference.pcr(A, W, W, rhs, tol, resscale, 50)
    assert (ref.iter, ref.errflag) == (k, 0)
    return tol, ref


@functools.lru_cache(maxsize=None)
def maxiter_reference(m, maxiter):
    A, W, resscale, rhs = diag_inputs(m, NCOLS[m])
    return cr_reference.pcr(A, W, W, rhs, 1e-30, resscale, maxiter)


@functools.lru_cache(maxsize=None)
def reference_204(m, n, seed):
    """five updates of the 204 input in extended precision, where nothing overflows"""
    A, W, _, rhs = diag_inputs(m, n, seed)
    return cr_reference.pcr(A, W * 1e-60, W, rhs * 1e170, 0.0, None, 5)


@pytest.fixture(scope="module")
def legs(tmp_path_factory):
    """{grid: [npz of each leg]}.  One batch per grid, its eight legs side by side, one process each.  A batch that does not
    finish or does not exit with 0 fails the fixture: no further batch is started, nothing is tried again."""
    from ipx_amd import kkt
    kkt.load_library()
    d = tmp_path_factory.mktemp("cr_pacing")
    tolfile = str(d / "tols.npz")
    np.savez(tolfile, **{"%d.%d" % (m, k): np.array(tol_reference(m, k)[0]) for m in ROWS for k in TOL_EXITS})
    res = {}
    for grid in GRIDS:
        procs, files = [], []
        for pace, ahead, refresh in LEGS:
            env = dict(os.environ, IPXK_CR_AHEAD=ahead, IPXK_CR_REFRESH=refresh)
            for name in ("IPXK_CR_GRID", "IPXK_CR_PACE", "IPXK_CR_EARLY", "IPXK_CR_LAZY"):
                env.pop(name, None)
            if grid:
                env["IPXK_CR_GRID"] = grid
            if pace:
                env["IPXK_CR_PACE"] = pace
            files.append(str(d / ("grid%s.%s.ahead%s.refresh%s.npz" % (grid or "default", pace or "progress", ahead, refresh))))
            procs.append(subprocess.Popen([sys.executable, WORKER, files[-1], tolfile], env=env, stdout=subprocess.PIPE,
                                          stderr=subprocess.STDOUT, text=True))
        logs = []
        for p in procs:
            try:
                logs.append(p.communicate(timeout=240)[0])
            except subprocess.TimeoutExpired:
                for q in procs:
                    q.kill()
                for q in procs:
                    q.wait()
                pytest.fail("legs with IPXK_CR_GRID=%r did not finish:\n%s" % (grid, "\n".join(logs)))
        if any(p.returncode != 0 for p in procs):
            pytest.fail("legs with IPXK_CR_GRID=%r: exit status %s\n%s" % (grid, [p.returncode for p in procs], "\n".join(logs)))
        res[grid] = [dict(np.load(f)) for f in files]
    return res


def case(leg, name):
    it, err = (int(v) for v in leg[name + ".it_err"])
    return leg[name + ".y"], it, err, leg[name + ".hist"]


def diagnostics(leg, name):
    return dict(zip(DIAG_FIELDS, leg[name + ".diagn"]))


def case_names(leg):
    return sorted(k[:-2] for k in leg if k.endswith(".y"))


NUM_CASES = len(ROWS) * (len(TOL_EXITS) + len(MAXITER_EXITS) + 1) + 4 + 2


# ---- the legs of one grid ----
@pytest.mark.parametrize("grid", GRIDS)
def test_legs_agree_bitwise(legs, grid):
    a = legs[grid][0]
    assert int(a["grid"][0]) == int(grid or 0)
    assert len(case_names(a)) == NUM_CASES
    for b in legs[grid][1:]:
        assert sorted(a) == sorted(b)
        for k in a:
            if k.endswith(".stats"):                    # what was enqueued: the drivers differ there
                continue
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
            assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k


@pytest.mark.parametrize("grid", GRIDS)
def test_launch_accounting(legs, grid):
    for (pace, ahead, refresh), leg in zip(LEGS, legs[grid]):
        for name in case_names(leg):
            enq, launches, snapshots, events = (int(v) for v in leg[name + ".stats"])
            it = int(leg[name + ".it_err"][0])
            print("grid %r pace %r ahead %s refresh %s %s: iterations %d, enqueued %d, launches %d, snapshots %d, events %d"
                  % (grid, pace, ahead, refresh, name, it, enq, launches, snapshots, events))
            if pace == "cycles":
                continue
            assert snapshots == 0 and events == 0, name
            assert enq <= it + 1 + int(ahead), name      # the hard bound: needs no margin
            if name not in ("smw", "plain"):
                fifths = 0 if refresh == "1" else enq // 5          # enqueued iterations 0 .. enq - 1 with (k + 1) % 5 == 0
                assert launches == 2 * enq + HEAD_TAIL + fifths, name


# ---- every exit against extended precision ----
@pytest.mark.parametrize("k", TOL_EXITS)
@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("grid", GRIDS)
def test_exit_through_tol(legs, grid, m, k):
    tol, ref = tol_reference(m, k)
    y, it, err, hist = case(legs[grid][0], "tol.%d.k%d" % (m, k))
    print("grid %r m %d k %d: tol %.6g, device y %.2e hist %.2e" % (grid, m, k, tol, dist(y, ref.lhs), dist(hist, ref.hist)))
    assert (it, err) == (k, 0) and len(hist) == k + 1
    assert dist(y, ref.lhs) <= 1e-12 and dist(hist, ref.hist) <= 1e-12


@pytest.mark.parametrize("maxiter", MAXITER_EXITS)
@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("grid", GRIDS)
def test_exit_through_maxiter(legs, grid, m, maxiter):
    ref = maxiter_reference(m, maxiter)
    assert (ref.iter, ref.errflag) == (maxiter, 201)
    y, it, err, hist = case(legs[grid][0], "maxiter.%d.%d" % (m, maxiter))
    assert (it, err) == (maxiter, 201) and len(hist) == maxiter + 1
    if maxiter == 0:
        assert not np.any(y)
    else:
        assert dist(y, ref.lhs) <= 1e-12
    assert dist(hist, ref.hist) <= 1e-12


@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("grid", GRIDS)
def test_exit_through_callback(legs, grid, m):
    """polls before iterations 5 and 10; the second returns nonzero: ten iterations are in the queue and are finished"""
    ref = maxiter_reference(m, 10)
    y, it, err, hist = case(legs[grid][0], "callback.%d" % m)
    assert (it, err) == (10, CALLBACK_FLAG) and len(hist) == 10
    assert dist(y, ref.lhs) <= 1e-12 and dist(hist, ref.hist[:10]) <= 1e-12
    for leg in legs[grid]:
        assert int(leg["callback.%d.stats" % m][0]) == 10


@pytest.mark.parametrize("name,shape", [("exit204.3000", (3000, 6000, SEED)), ("exit204.300", SMALL_204)])
@pytest.mark.parametrize("grid", GRIDS)
def test_no_progress_204(legs, grid, name, shape):
    ref = reference_204(*shape)
    assert ref.iter == 5 and np.all(np.log10(ref.rps) > 330)
    y, it, err, hist = case(legs[grid][0], name)
    assert (it, err) == (5, 204) and len(hist) == 5
    assert np.isfinite(y).all() and dist(y, ref.lhs) <= 1e-12 and dist(hist, ref.hist[:5]) <= 1e-12
    d = diagnostics(legs[grid][0], name)
    assert d["rps_old"] == np.inf and d["rps_new"] == np.inf
    assert (d["errflag"], d["iter"], d["maxiter"], d["tol"]) == (204, 5, 200, 0.0)


@pytest.mark.parametrize("errflag", [205, 202])
@pytest.mark.parametrize("grid", GRIDS)
def test_exit_at_iteration_0(legs, grid, errflag):
    rhs = diag_inputs(3000, 6000)[3] * (1e200 if errflag == 205 else 1e-200)
    y, it, err, hist = case(legs[grid][0], "exit%d" % errflag)
    assert (it, err) == (0, errflag)
    assert not np.any(y) and len(hist) == 1 and hist[0] == np.abs(rhs).max()
    d = diagnostics(legs[grid][0], "exit%d" % errflag)
    assert (d["errflag"], d["iter"], d["maxiter"], d["tol"]) == (errflag, 0, 50, 0.0)


# ---- the other modes ----
def ocsc(M):
    from oracle import pyoracle as po
    return po.Csc(M.nrow, M.ncol, M.p, M.i, M.x)


def check_vs_oracle(run, orc):
    y, it, err, hist = run
    yo, ito, erro, histo = orc[:4]
    assert (it, err) == (ito, erro) == (OTHER_MAXITER, 201) and len(hist) == OTHER_MAXITER + 1
    assert np.abs(hist[:10] - histo[:10]).max() <= 1e-9 * histo[:10].max()
    assert relerr(y, yo) < 1e-6


def test_pcrsmw_vs_oracle(legs, oracle):
    A, W, resscale, rhs = diag_inputs(3000, 6000, num_dense=5)
    Ao = ocsc(A)
    P, err = oracle.diag_factorize(Ao, W, oracle.find_dense_columns(Ao)[1], True)
    assert err == 0
    orc = oracle.pcr_solve(lambda v: oracle.normal_apply(Ao, W, v), P.apply, rhs, 1e-30, resscale, OTHER_MAXITER, hist_cap=20)
    for grid in GRIDS:
        check_vs_oracle(case(legs[grid][0], "smw"), orc)


def test_plain_vs_oracle(legs, oracle):
    B, colscale, rhs = plain_inputs(*PLAIN_SHAPE)
    n = B["A"].ncol
    S = oracle.split_prepare(ocsc(B["A"].with_identity()), n, ocsc(B["L"]), ocsc(B["U"]), B["rowperm"], B["colperm"],
                             B["basis"], B["status"], colscale)
    orc = oracle.cr_solve(S.apply, rhs, 1e-30, None, OTHER_MAXITER, hist_cap=20)
    for grid in GRIDS:
        check_vs_oracle(case(legs[grid][0], "plain"), orc)
