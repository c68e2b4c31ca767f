"""GPU: the pivot searches of the basis phase at exact ties and past one grid pass (tests/basis_ties_reference.py).

ipm_starting_basis against the planted expectation (no solve: from the slack basis the tableau columns and rows of these
models are the raw columns and rows of A), maxvolume and maxvolume_sequential against the CPU oracle, whose loops are the
stated rule (the first strictly larger entry).  All data are dyadic, so every comparison is EXACT: a device result that
differs is a wrong decision of a thread loop, of wave_argmax / block_partial / block_argmax (take_larger's oi < i) or of
a finishing kernel, never rounding.  A wrong tie break is silent otherwise: the basis is still a basis.

tests/test_basis_ties_reference.py checks on the CPU that every planted class is met by the oracle and goes to its lowest
member, so equality with the oracle's log means the device decided every class the same way.

Measured on the MI355X (this file's own prints): see DESIGN.md section 8f."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

import basis_ties_reference as R
from ipx_amd import synth

pytestmark = pytest.mark.gpu

# The shapes mirror the kernels' launch constants: kBlock = 256 threads, kSbGrid = kRedGrid = 512 workgroups, so the grid-stride
# kernels cover G = 512 * 256 = 131 072 indices per pass; kRowLanes = 8 lanes per column give sb_row_kernel 256 / 8 = 32 columns per
# workgroup and G_ROW = 512 * 32 = 16 384 per pass.
assert (R.K_BLOCK, R.K_GRID, R.K_ROW_LANES, R.G, R.G_ROW) == (256, 512, 8, 131072, 16384)
SMALL = (700, 1500)             # one pass: lanes of a wavefront, wavefronts of a workgroup, workgroups
TALL = (131072 + 257, 1500)     # m = G + 257: a second pass over the positions (sb_column, mv_scale_ftran, mvs_search_pivot)
WIDE = (300, 131072 + 257)      # n = G + 257 >= 2 G_ROW + 300: a second pass over the columns (sb_row_scaled, mv_argmax), eight of sb_row
assert (SMALL, TALL, WIDE) == (R.SMALL, R.TALL, R.WIDE)
IDS = ["small", "tall", "wide"]


@pytest.fixture(scope="module")
def kkt():
    from ipx_amd import kkt as k
    k.load_library()
    assert k.load_library().ipxk_device_count() > 0, "no GPU visible"
    return k


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


def matrix_of(P):
    return synth.CscMatrix(P["m"], P["n"], P["Ap"], P["Ai"], P["Ax"])


def assert_same_log(got, want):
    got, want = np.asarray(got).reshape(-1, 2), np.asarray(want).reshape(-1, 2)
    k = min(len(got), len(want))
    diff = np.nonzero((got[:k] != want[:k]).any(axis=1))[0]
    first = int(diff[0]) if len(diff) else k
    assert len(got) == len(want) and not len(diff), \
        "exchange %d of %d / %d: device (jb, jn) = %s, expected %s" % (first, len(got), len(want), got[first:first + 1].tolist(),
                                                                      want[first:first + 1].tolist())


@pytest.mark.parametrize("shape", [SMALL, TALL, WIDE], ids=IDS)
def test_starting_basis_takes_the_planted_exchanges(kkt, shape):
    m, n = shape
    P = R.starting_basis_case(m, n, seed=1)
    E = P["expected"]
    t0 = time.perf_counter()
    ctx = kkt.KktContext(matrix_of(P))
    t1 = time.perf_counter()
    ctx.iterate_set(P["it"], P["state"])
    g = ctx.ipm_starting_basis(P["b"], P["c"], P["lb"], P["ub"])
    t2 = time.perf_counter()
    print("m %d n %d: context %.3f s, starting basis %.3f s (%d exchanges, %d factorizations)"
          % (m, n, t1 - t0, t2 - t1, g["updates_start"], g["factorizations"]))
    assert g["errflag"] == 0
    assert_same_log(g["exchanges"], E["log"])
    assert g["updates_start"] == len(E["log"])
    assert np.array_equal(g["basis"], E["basis"]) and np.array_equal(g["status"], E["status"])
    assert (g["dependent_cols"], g["dependent_rows"], g["cols_inconsistent"], g["rows_inconsistent"], g["stability_pivots"]) == (0, 0, 0, 0, 0)
    # the context holds the operator of the final basis
    AI = sp.hstack([sp.csc_matrix((P["Ax"], P["Ai"], P["Ap"]), shape=(m, n)), sp.identity(m)]).tocsc()
    rhs = np.random.default_rng(1).standard_normal(m)
    x = ctx.solve_dense(rhs, "n")
    assert np.abs(AI[:, g["basis"]] @ x - rhs).max() <= 1e-7 * (1 + np.abs(x).max())
    ctx.close()


_CASES = {}


def mv_case(shape, oracle, po):
    """one model per shape and the oracle's runs on it, computed once, shared by the cases below and left unchanged"""
    if shape not in _CASES:
        m, n = shape
        P = R.maxvolume_case(m, n, seed=2, rows_per_slice=R.ROWS_PER_SLICE[shape])
        Ao = po.Csc(m, n, P["Ap"], P["Ai"], P["Ax"])
        want = {}
        # (sequential: a tableau column per candidate column, and its search runs over the m positions: SMALL and TALL show all of it)
        for variant in ("heuristic", "sequential") if shape != WIDE else ("heuristic",):
            B = oracle.basis(Ao, P["basis"], P["status"])
            if variant == "heuristic":
                r = B.maxvolume(P["colscale"], volume_tol=2.0, maxskip_updates=10, rows_per_slice=P["rows_per_slice"])
            else:
                r = B.maxvolume_sequential(P["colscale"], volume_tol=2.0)
            r["basis"], r["status"], _ = B.get()
            R.maxvolume_classes_met(P, r["exchanges"], variant)      # zero classes unmet (as the CPU test asserts)
            want[variant] = r
        _CASES[shape] = (P, want)
    return _CASES[shape]


def prepared_context(kkt, P):
    t0 = time.perf_counter()
    ctx = kkt.KktContext(matrix_of(P))
    t1 = time.perf_counter()
    ctx.lu_factorize_basis(P["basis"], 0.1, download=False)
    ctx.split_prepare_lu(P["status"], P["colscale"])
    return ctx, t1 - t0, time.perf_counter() - t1


def assert_same_run(got, want, counters):
    assert got["errflag"] == 0
    assert_same_log(got["exchanges"], want["exchanges"])
    assert tuple(got[k] for k in counters) == tuple(want[k] for k in counters), counters
    assert np.array_equal(got["basis"], want["basis"]) and np.array_equal(got["status"], want["status"])
    # every accepted vmax is a power of two: volinc is a sum of integers, equal bit for bit
    assert got["volinc"] == want["volinc"] == float(int(want["volinc"]))


@pytest.mark.parametrize("shape", [SMALL, TALL, WIDE], ids=IDS)
def test_maxvolume_heuristic_decides_every_tie_like_the_oracle(kkt, oracle, po, shape):
    P, want = mv_case(shape, oracle, po)
    ctx, t_ctx, t_prep = prepared_context(kkt, P)
    t0 = time.perf_counter()
    got = ctx.maxvolume(P["status"], P["colscale"], volume_tol=2.0, maxskip_updates=10, rows_per_slice=P["rows_per_slice"])
    print("m %d n %d: context %.3f s, factorize + prepare %.3f s, maxvolume %.3f s (%d updates, %d skipped, %d slices)"
          % (P["m"], P["n"], t_ctx, t_prep, time.perf_counter() - t0, got["updates"], got["skipped"], got["slices"]))
    assert_same_run(got, want["heuristic"], ("updates", "skipped", "slices", "refused"))
    ctx.close()


@pytest.mark.parametrize("shape", [SMALL, TALL], ids=IDS[:2])
def test_maxvolume_sequential_decides_every_tie_like_the_oracle(kkt, oracle, po, shape):
    P, want = mv_case(shape, oracle, po)
    ctx, t_ctx, t_prep = prepared_context(kkt, P)
    t0 = time.perf_counter()
    got = ctx.maxvolume_sequential(P["status"], P["colscale"], volume_tol=2.0)
    print("m %d n %d: context %.3f s, factorize + prepare %.3f s, sequential %.3f s (%d updates, %d skipped, %d passes)"
          % (P["m"], P["n"], t_ctx, t_prep, time.perf_counter() - t0, got["updates"], got["skipped"], got["passes"]))
    assert_same_run(got, want["sequential"], ("updates", "skipped", "passes", "refused"))
    ctx.close()
