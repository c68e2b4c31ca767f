"""GPU: the ways out of the CR loop (ipx_amd/csrc/cr.hip) that no other test takes, and the later element groups of its
two vector kernels.

Exits.  204 (IPX_ERROR_cr_no_progress, the check of every fifth iteration, reference src/conjugate_residuals.cc:186-207),
205 (IPX_ERROR_cr_inf_or_nan, :168-172 and :67-71) and 202 at k = 0 are reached by overflow and underflow in the
arithmetic alone; every buffer keeps its size and every index its range.
  * 204: C from W * 1e-60, P from W, rhs * 1e170.  residual' P residual is about 1e341, i.e. inf in binary64, at iterations
    0 and 5, and `inf >= inf` ends the run at iteration 5 whatever the order of the sum; cdot, pdot, alpha and lhs stay
    finite.  The margins are re-derived below from tests/cr_reference.py (extended precision does not overflow there).
  * 205 at k = 0: rhs * 1e200 makes cdot and pdot inf or NaN, alpha is not finite.  202 at k = 0: rhs * 1e-200, every
    product underflows, cdot is 0.
After every exit case the worker stores ipxk_cr_diagnostics.

Element groups.  A thread of the vector kernels has a second element only above 262 144 rows and enters the loop after
its first group of kCrUnroll = 4 only above 1 048 576 rows.  IPXK_CR_GRID caps the grid, so that 1024, 1025 and 3000 rows
give a thread exactly 4 elements (grid 1), a fifth for thread 0 alone, 11 or 12 (three groups, the last one ragged) and, at
grid 2, 5 or 6 with sums over two partials.  The PcrDiag runs are compared with tests/cr_reference.py at 1e-12, the
project's operator-level parity gate: an element that missed one update, or took its neighbour's,
stands out by many orders (the smallest |y_i| is above 4e-6 of the largest).  The CPU oracle must itself be within 1e-13
of that reference, else the input is wrong, not the kernel.  PcrSmw and plain CR are held to the oracle at the gates of
tests/test_gpu_parity.py.

Legs: tests/cr_exits_worker.py in a process of its own for grid in {unset, 1, 2} x (IPXK_CR_EARLY, IPXK_CR_LAZY) in
{(1,1), (0,1), (1,0)}; for each grid the three orders must agree bit for bit, NaN included.

Measured on the CPU (oracle against tests/cr_reference.py, relative to the largest entry):
  PcrDiag shape cases, 3 shapes x 3 maxiter: y within 1.4e-15, history within 2.1e-15; smallest |y_i| / largest 4.2e-6.
  204 runs: y after five updates within 1.3e-15 (3000 rows) and 2.6e-16 (300 rows), the five history entries within
  3.9e-15; log10 of residual' P residual at iterations 0 and 5: 341.1 and 340.1 (3000 rows), 340.0 and 338.9 (300 rows);
  largest log10 of cdot and of pdot over iterations 0..4: 281.1 and 221.4 (3000 rows), 280.0 and 220.3 (300 rows).
  With five dense columns the oracle runs the 204 input to (12, 201), and to (200, 201) with maxiter 200.
  Two-rank problem of tests/cr_lazy_worker.py with a, b * 1e160: oracle (0, 205), y zero, x finite.
Measured on an MI355X (device against tests/cr_reference.py, the worst over the three grids and the three maxiter):
  PcrDiag shape cases: y within 4.7e-16, history within 7.3e-16.  204 runs: y within 1.8e-16 (3000 rows) and 1.7e-16
  (300 rows).  The 204 input with dense columns: (12, 201), as the oracle.
A deliberately wrong build (the direction kernel's loop after the first group not paying the owed solution update) moved
y by 2e-2 to 1e0 in every grid-1 and grid-2 case with more than four elements per thread and left the others alone."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cr_reference
from cr_exits_worker import DIAG_FIELDS, MAXITERS, PLAIN_EXIT, PLAIN_SHAPE, SHAPES, SMALL_204, diag_inputs, plain_inputs
from helpers import relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "cr_exits_worker.py")
GRIDS = ("", "1", "2")                                  # IPXK_CR_GRID; "": unset
ORDERS = (("1", "1"), ("0", "1"), ("1", "0"))           # (IPXK_CR_EARLY, IPXK_CR_LAZY)
NCOLS = dict(SHAPES)


@pytest.fixture(scope="module")
def legs(tmp_path_factory):
    """{grid: [npz of each order]}.  One batch per grid, its three orders side by side.  A batch that does not finish or
    does not exit with 0 fails the fixture: no further batch is started, nothing is tried again."""
    from ipx_amd import kkt
    kkt.load_library()
    d = tmp_path_factory.mktemp("cr_exits")
    res = {}
    for grid in GRIDS:
        procs, files = [], []
        for early, lazy in ORDERS:
            env = dict(os.environ, IPXK_CR_EARLY=early, IPXK_CR_LAZY=lazy)
            env.pop("IPXK_CR_GRID", None)
            if grid:
                env["IPXK_CR_GRID"] = grid
            files.append(str(d / ("grid%s.early%s.lazy%s.npz" % (grid or "default", early, lazy))))
            procs.append(subprocess.Popen([sys.executable, WORKER, files[-1]], env=env, stdout=subprocess.PIPE,
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


def dist(a, b):
    """max |a - b| / max |b| with b in extended precision"""
    b = np.asarray(b, dtype=np.longdouble)
    return float(np.abs(np.asarray(a, dtype=np.longdouble) - b).max() / np.abs(b).max())


# ---- CPU side: computed once, shared by the cases of every grid ----
def ocsc(M):
    from oracle import pyoracle as po
    return po.Csc(M.nrow, M.ncol, M.p, M.i, M.x)


_oracle_runs = {}


def oracle_pcr(oracle, key, A, W_C, W_P, rhs, tol, resscale, maxiter, hist_cap):
    if key not in _oracle_runs:
        Ao = ocsc(A)
        P, err = oracle.diag_factorize(Ao, W_P, oracle.find_dense_columns(Ao)[1], True)
        assert err == 0
        _oracle_runs[key] = oracle.pcr_solve(lambda v: oracle.normal_apply(Ao, W_C, v), P.apply, rhs, tol, resscale, maxiter,
                                             hist_cap=hist_cap)
    return _oracle_runs[key]


def oracle_plain(oracle, key, shape, scale, tol, maxiter, hist_cap):
    if key not in _oracle_runs:
        B, colscale, rhs = plain_inputs(*shape)
        n = B["A"].ncol
        S = oracle.split_prepare(ocsc(B["A"].with_identity()), n, ocsc(B["L"]), ocsc(B["U"]), B["rowperm"], B["colperm"],
                                 B["basis"], B["status"], colscale)
        free = S.get()["free_positions"]
        assert not np.any(rhs[free])                    # zeroed at the free positions, as in test_basis_path_vs_oracle
        _oracle_runs[key] = oracle.cr_solve(S.apply, rhs * scale, tol, None, maxiter, hist_cap=hist_cap) + (rhs * scale,)
    return _oracle_runs[key]


@functools.lru_cache(maxsize=None)
def reference_shape(m, maxiter):
    A, W, resscale, rhs = diag_inputs(m, NCOLS[m])
    return cr_reference.pcr(A, W, W, rhs, 1e-30, resscale, maxiter)


@functools.lru_cache(maxsize=None)
def reference_204(m, n, seed):
    """five updates of the 204 input in extended precision, where nothing overflows"""
    A, W, _, rhs = diag_inputs(m, n, seed)
    return cr_reference.pcr(A, W * 1e-60, W, rhs * 1e170, 0.0, None, 5)


# ---- the three orders of the kernels ----
@pytest.mark.parametrize("grid", GRIDS)
def test_orders_agree_bitwise(legs, grid):
    a = legs[grid][0]
    assert int(a["grid"][0]) == int(grid or 0)
    assert len([k for k in a if k.endswith(".y")]) == 24      # 15 shape cases, 9 exit cases
    for b in legs[grid][1:]:
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
            assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k


# ---- element groups ----
@pytest.mark.parametrize("maxiter", MAXITERS)
@pytest.mark.parametrize("m", [s[0] for s in SHAPES])
@pytest.mark.parametrize("grid", GRIDS)
def test_pcrdiag_groups_vs_extended_precision(legs, oracle, grid, m, maxiter):
    y, it, err, hist = case(legs[grid][0], "diag.%d.maxiter%d" % (m, maxiter))
    ref = reference_shape(m, maxiter)
    assert (ref.iter, ref.errflag) == (maxiter, 201)
    A, W, resscale, rhs = diag_inputs(m, NCOLS[m])
    yo, ito, erro, histo = oracle_pcr(oracle, ("shape", m, maxiter), A, W, W, rhs, 1e-30, resscale, maxiter, 20)
    print("grid %r m %d maxiter %d: device y %.2e hist %.2e; oracle y %.2e hist %.2e; min|y|/max|y| %.2e"
          % (grid, m, maxiter, dist(y, ref.lhs), dist(hist, ref.hist), dist(yo, ref.lhs), dist(histo, ref.hist),
             np.abs(y).min() / np.abs(y).max()))
    assert (ito, erro) == (maxiter, 201) and dist(yo, ref.lhs) < 1e-13 and dist(histo, ref.hist) < 1e-13
    assert (it, err) == (maxiter, 201) and len(hist) == maxiter + 1
    assert dist(y, ref.lhs) <= 1e-12 and dist(hist, ref.hist) <= 1e-12


def check_vs_oracle(run, orc, maxiter):
    y, it, err, hist = run
    yo, ito, erro, histo = orc[:4]
    assert (it, err) == (ito, erro) == (maxiter, 201) and len(hist) == maxiter + 1
    assert np.abs(hist[:10] - histo[:10]).max() <= 1e-9 * histo[:10].max()
    assert relerr(y, yo) < 1e-6


@pytest.mark.parametrize("maxiter", MAXITERS)
@pytest.mark.parametrize("grid", GRIDS)
def test_pcrsmw_groups_vs_oracle(legs, oracle, grid, maxiter):
    A, W, resscale, rhs = diag_inputs(3000, 6000, num_dense=5)
    orc = oracle_pcr(oracle, ("smw", maxiter), A, W, W, rhs, 1e-30, resscale, maxiter, 20)
    check_vs_oracle(case(legs[grid][0], "smw.maxiter%d" % maxiter), orc, maxiter)


@pytest.mark.parametrize("maxiter", MAXITERS)
@pytest.mark.parametrize("grid", GRIDS)
def test_plain_groups_vs_oracle(legs, oracle, grid, maxiter):
    orc = oracle_plain(oracle, ("plain", maxiter), PLAIN_SHAPE, 1.0, 1e-30, maxiter, 20)
    check_vs_oracle(case(legs[grid][0], "plain.maxiter%d" % maxiter), orc, maxiter)


# ---- 204 ----
@pytest.mark.parametrize("name,shape", [("exit204.3000", (3000, 6000, 21)), ("exit204.300", SMALL_204)])
@pytest.mark.parametrize("grid", GRIDS)
def test_no_progress_204(legs, oracle, grid, name, shape):
    A, W, _, rhs = diag_inputs(*shape)
    ref = reference_204(*shape)
    # the fixture's margins: residual' P residual is far above the largest binary64 (1.8e308) at iterations 0 and 5,
    # cdot and pdot of the five iterations far below it
    assert ref.iter == 5 and len(ref.rps) == 2 and len(ref.cdot) == len(ref.pdot) == 5
    print("%s: log10 r'Pr %s, log10 cdot %s, log10 pdot %s" % (name, np.log10(ref.rps), np.log10(ref.cdot), np.log10(ref.pdot)))
    assert np.all(np.log10(ref.rps) > 330) and np.all(np.log10(ref.cdot) < 290) and np.all(np.log10(ref.pdot) < 290)
    assert np.all(ref.cdot > 0) and np.all(ref.pdot > 0)
    yo, ito, erro, histo = oracle_pcr(oracle, name, A, W * 1e-60, W, rhs * 1e170, 0.0, None, 200, 300)
    assert (ito, erro) == (5, 204)
    y, it, err, hist = case(legs[grid][0], name)
    print("%s grid %r: device y %.2e, oracle y %.2e" % (name, grid, dist(y, ref.lhs), dist(yo, ref.lhs)))
    assert (it, err) == (5, 204)
    assert len(hist) == 5 and np.abs(hist - histo[:5]).max() <= 1e-12 * histo[:5].max()      # `iter` entries, not iter + 1
    assert np.isfinite(y).all() and dist(yo, ref.lhs) < 1e-13
    assert dist(y, ref.lhs) <= 1e-12                                                         # exactly five updates are in lhs
    d = diagnostics(legs[grid][0], name)
    assert d["rps_old"] == np.inf and d["rps_new"] == np.inf
    assert (d["errflag"], d["iter"], d["maxiter"], d["tol"]) == (204, 5, 200, 0.0)


@pytest.mark.parametrize("grid", GRIDS)
def test_204_input_with_dense_columns(legs, oracle, grid):
    """With five dense columns residual' P residual of this input is NaN in the oracle, not inf: the correction of
    reference src/diagonal_precond.cc:144-148 makes 71 of the products lhs[i] * rhs[i] negative, so the sum is
    inf - inf.  `NaN >= x` is false as in the reference (src/conjugate_residuals.cc:197): no 204, the run goes to its iteration limit.  Only
    the agreement with the oracle is asked."""
    A, W, _, rhs = diag_inputs(3000, 6000, num_dense=5)
    yo, ito, erro, histo = oracle_pcr(oracle, "exit204.smw", A, W * 1e-60, W, rhs * 1e170, 0.0, None, 12, 300)
    y, it, err, hist = case(legs[grid][0], "exit204.smw")
    print("204 input with dense columns, grid %r: device %s, oracle %s" % (grid, (it, err), (ito, erro)))
    assert (it, err) == (ito, erro)
    d = diagnostics(legs[grid][0], "exit204.smw")
    assert (d["errflag"], d["iter"], d["maxiter"], d["tol"]) == (err, it, 12, 0.0)


# ---- 205 and 202 at k = 0 ----
def exit_inputs(oracle, mode, errflag):
    scale = 1e200 if errflag == 205 else 1e-200
    key = "exit%d.%s" % (errflag, mode)
    if mode == "plain":
        orc = oracle_plain(oracle, key, PLAIN_EXIT, scale, 0.0, 50, 20)
        return key, orc[:4], orc[4]
    A, W, _, rhs = diag_inputs(3000, 6000, num_dense=5 if mode == "smw" else 0)
    return key, oracle_pcr(oracle, key, A, W, W, rhs * scale, 0.0, None, 50, 20), rhs * scale


@pytest.mark.parametrize("errflag", [205, 202])
@pytest.mark.parametrize("mode", ["diag", "smw", "plain"])
@pytest.mark.parametrize("grid", GRIDS)
def test_exit_at_iteration_0(legs, oracle, grid, mode, errflag):
    key, (yo, ito, erro, histo), rhs = exit_inputs(oracle, mode, errflag)
    assert (ito, erro) == (0, errflag)
    y, it, err, hist = case(legs[grid][0], key)
    assert (it, err) == (0, errflag)
    assert not np.any(y) and len(hist) == 1 and hist[0] == np.abs(rhs).max()
    d = diagnostics(legs[grid][0], key)
    assert (d["errflag"], d["iter"], d["maxiter"], d["tol"]) == (errflag, 0, 50, 0.0)
    if errflag == 202:
        assert d["cdot"] == 0.0 and d["infnorm_residual"] == np.abs(rhs).max()
        if mode == "diag":
            want = np.abs(rhs / legs[grid][0]["exit202.diag.d"]).max()
            assert abs(d["infnorm_sresidual"] - want) <= 1e-12 * want
        if mode == "plain":
            assert d["infnorm_sresidual"] == 0.0
