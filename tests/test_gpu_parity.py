"""GPU parity tests: the HIP path (through the C ABI of libipx_kkt_hip.so) against the CPU oracle
on seeded inputs and against the committed golden vectors of the reference.

Tolerances ("Parity gate"):
  * index / permutation arrays: bit-exact;
  * operator applications: relative inf-norm error <= 1e-12 (most rows are in fact bit-exact because
    the kernels add a row's products in the reference's order);
  * CR runs: identical errflag, |iter_gpu - iter_cpu| <= max(2, 2%), first 10 residual norms within
    1e-9 relative, final solution within 1e-6 relative for runs <= ~150 iterations, and the KKT
    residual of the returned point recomputed on the CPU within the requested tolerance.
"""
import os

import time

import numpy as np
import pytest

from helpers import basis_problem, diag_problem, kkt_residual_diag, relerr
from ipx_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def kkt():
    from ipx_amd import kkt as k
    k.load_library()          # raises if the HIP library was not built: no fallback
    assert k.load_library().ipxk_device_count() > 0, "no GPU visible"
    return k


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


def ocsc(po, A):
    return po.Csc(A.nrow, A.ncol, A.p, A.i, A.x)


def iters_close(a, b):
    return abs(a - b) <= max(2, int(0.02 * max(a, b)))


# --------------------------------------------------------------------------------------
# golden vectors of the reference
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["diag_200", "dense_300"])
def test_golden_diag(kkt, po, name):
    from ipx_amd.synth import CscMatrix
    d = np.load(os.path.join(GOLD, name + ".npz"))
    m, n = int(d["m"]), int(d["n"])
    A = CscMatrix(m, n, d["Ap"], d["Ai"], d["Ax"])
    ctx = kkt.KktContext(A)
    assert ctx.num_dense_cols == int(d["num_dense"])
    p, i, x = ctx.get_rowwise()
    keep = d["AIti"] < n
    assert np.array_equal(i, d["AIti"][keep]) and np.array_equal(x, d["AItx"][keep])
    W, rhs = d["W"], d["rhs"]
    ctx.normal_prepare(W)
    lhs, dot = ctx.normal_apply(rhs)
    assert relerr(lhs, d["normal_lhs"]) <= 1e-12 and abs(dot - float(d["normal_dot"])) <= 1e-12 * abs(dot)
    ctx.normal_prepare(None)
    lhs, dot = ctx.normal_apply(rhs)
    assert relerr(lhs, d["normal0_lhs"]) <= 1e-12
    assert ctx.diag_factorize(W, True) == int(d["prec_err"])
    pl, pd = ctx.diag_apply(rhs)
    assert relerr(pl, d["prec_lhs"]) <= 1e-12 and abs(pd - float(d["prec_dot"])) <= 1e-12 * abs(pd)
    ctx.normal_prepare(W)
    y, it, e, hist, _ = ctx.pcr_solve(rhs, float(d["pcr_tol"]), d["resscale"], 500, hist_cap=600)
    assert e == int(d["pcr_err"]) and iters_close(it, int(d["pcr_iter"]))
    assert relerr(y, d["pcr_y"]) < 1e-6 and hist[-1] <= float(d["pcr_tol"])
    _, it, e, _, _ = ctx.pcr_solve(rhs, 1e-30, d["resscale"], 7)
    assert (it, e) == (7, 201)
    ctx.normal_prepare(d["Wneg"])
    assert ctx.diag_factorize(d["Wneg"], False) == 0
    _, it, e, _, _ = ctx.pcr_solve(rhs, 1e-12, None, 200)
    assert (it, e) == (int(d["neg_iter"]), int(d["neg_err"]))
    assert ctx.kkt_diag_factorize(d["xl"], d["xu"], d["zl"], d["zu"], float(d["mu"])) == 0
    x, yk, it, e, _ = ctx.kkt_diag_solve(d["a"], d["b"], float(d["kkt_tol"]), 500)
    assert e == int(d["kkt_err"]) and iters_close(it, int(d["kkt_iter"]))
    assert relerr(x, d["kkt_x"]) < 1e-6 and relerr(yk, d["kkt_y"]) < 1e-6
    ctx.close()


def test_golden_afiro(kkt):
    from ipx_amd.synth import CscMatrix
    d = np.load(os.path.join(GOLD, "afiro.npz"))
    m, n = int(d["m"]), int(d["n"])
    AIp, AIi, AIx = d["AIp"], d["AIi"], d["AIx"]
    A = CscMatrix(m, n, AIp[: n + 1], AIi[: AIp[n]], AIx[: AIp[n]])
    ctx = kkt.KktContext(A)
    assert ctx.kkt_diag_factorize() == 0          # Factorize(nullptr)
    x, y, it, e, _ = ctx.kkt_diag_solve(d["a"], d["b"], float(d["tol"]))
    assert (it, e) == (int(d["iter"]), int(d["errflag"]))
    assert relerr(x, d["x"]) < 1e-9 and relerr(y, d["y"]) < 1e-9
    assert ctx.kkt_diag_factorize(d["xl"], d["xu"], d["zl"], d["zu"], float(d["mu"])) == 0
    x, y, it, e, _ = ctx.kkt_diag_solve(d["a"], d["b"], float(d["tol2"]))
    assert (it, e) == (int(d["iter2"]), int(d["errflag2"]))
    assert relerr(x, d["x2"]) < 1e-9 and relerr(y, d["y2"]) < 1e-9
    ctx.close()


def test_golden_basis(kkt):
    from ipx_amd.synth import CscMatrix
    d = np.load(os.path.join(GOLD, "basis_200.npz"))
    m, n = int(d["m"]), int(d["n"])
    A = CscMatrix(m, n, d["Ap"], d["Ai"], d["Ax"])
    L = CscMatrix(m, m, d["Lp"], d["Li"], d["Lx"])
    U = CscMatrix(m, m, d["Up"], d["Ui"], d["Ux"])
    ctx = kkt.KktContext(A)
    ctx.split_prepare(L, U, d["rowperm"], d["colperm"], d["basis"], d["status"], d["colscale"])
    lhs, dot = ctx.split_apply(d["x0"])
    assert relerr(lhs, d["split_lhs"]) <= 1e-12 and abs(dot - float(d["split_dot"])) <= 1e-12 * abs(dot)
    y, it, e, hist, _ = ctx.cr_solve(d["cr_rhs"], float(d["cr_tol"]), None, -1, hist_cap=300)
    assert (it, e) == (int(d["cr_iter"]), int(d["cr_err"])) and relerr(y, d["cr_y"]) < 1e-9
    _, it, e, _, _ = ctx.cr_solve(d["cr_rhs"], 1e-30, None, 5)
    assert (it, e) == (5, 201)
    # SolveDense on the unscaled factors == the reference's ForwardSolve/BackwardSolve between the
    # permutations of src/forrest_tomlin.cc:67-78 (fwd/bwd of the fixture were computed on x0)
    rp, cp = d["rowperm"], d["colperm"]
    rp_inv, cp_inv = np.argsort(rp), np.argsort(cp)
    xN = ctx.solve_dense(d["x0"][rp_inv], "N")        # work = rhs[rowperm] == x0
    assert np.array_equal(xN[cp], d["fwd"])
    xT = ctx.solve_dense(d["x0"][cp_inv], "T")        # work = rhs[colperm] == x0
    assert np.array_equal(xT[rp], d["bwd"])
    ctx.close()


# --------------------------------------------------------------------------------------
# HIP vs oracle on seeded inputs
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,num_dense,spread", [(64, 100, 0, 1.0), (2000, 4100, 0, 1.0),
                                                  (3000, 6000, 5, 1.0), (5000, 9000, 0, 0.0),
                                                  (1500, 3100, 100, 1.0), (1600, 3300, 330, 1.0)])   # blocked Cholesky / solves
def test_diag_path_vs_oracle(kkt, po, oracle, m, n, num_dense, spread):
    A, st = diag_problem(m, n, seed=21, spread=spread, num_dense=num_dense)
    Ao = ocsc(po, A)
    ctx = kkt.KktContext(A)
    nd, nzd = oracle.find_dense_columns(Ao)
    assert ctx.num_dense_cols == nd
    AT = oracle.transpose(Ao)
    p, i, x = ctx.get_rowwise()
    assert np.array_equal(p, AT.p) and np.array_equal(i, AT.i) and np.array_equal(x, AT.x)
    rng = np.random.default_rng(1)
    rhs = rng.standard_normal(m)
    mu = st["mu"]
    assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], mu) == 0
    ko = oracle.kkt_diag(Ao, nzd, True, 500)
    assert ko.factorize(st["xl"], st["xu"], st["zl"], st["zu"], mu) == 0
    W1, r1 = ctx.kkt_diag_get()
    W2, r2 = ko.get()
    assert np.array_equal(W1, W2) and np.array_equal(r1, r2)
    lhs, dot = ctx.normal_apply(rhs)
    lhs2, dot2 = oracle.normal_apply(Ao, W2, rhs)
    assert relerr(lhs, lhs2) <= 1e-12 and abs(dot - dot2) <= 1e-12 * abs(dot2)
    if num_dense == 0:
        assert np.array_equal(lhs, lhs2)          # rows are added in the reference's order
    pl, pd = ctx.diag_apply(rhs)
    pl2, pd2 = ko_precond_apply(oracle, Ao, W2, nzd, rhs)
    assert relerr(pl, pl2) <= 1e-12 and abs(pd - pd2) <= 1e-12 * abs(pd2)
    tol = 0.3 * np.sqrt(mu)
    x1, y1, it1, e1, _ = ctx.kkt_diag_solve(st["a"], st["b"], tol, 500)
    x2, y2, it2, e2, _ = ko.solve(st["a"], st["b"], tol)
    assert e1 == e2 == 0 and iters_close(it1, it2)
    # many dense columns: the Schur complement is ill-conditioned enough for two runs that stop at the same
    # tolerance to differ by more (the preconditioner applications above agree to 1e-12; the contract below holds)
    loose = 100.0 if num_dense >= 100 else 1.0
    assert relerr(y1, y2) < 1e-6 * loose and relerr(x1, x2) < 1e-5 * loose
    # the returned point satisfies the contract of src/kkt_solver.h:21-27
    res1, res2 = kkt_residual_diag(A, W2, st["a"], st["b"], x1, y1)
    assert np.abs(res2).max() < 1e-9 * max(1.0, np.abs(st["b"]).max() + np.abs(x1).max())
    assert np.abs(res1[:n]).max() < 1e-9 * max(1.0, np.abs(x1 / W2).max())
    assert np.abs(np.sqrt(W2[n:]) * res1[n:]).max() <= tol * (1 + 1e-9)
    ctx.close()


def test_diag_path_stress_spread3(kkt, po, oracle):
    """SURVEY 8d stress point: scaling spread s = 3 (W spans 12 decades): the diag-preconditioned CR
    does not converge within the cap; both sides stop at the cap with errflag 201 (or agree on an earlier
    breakdown flag)"""
    m, n = 3000, 6200
    A, st = diag_problem(m, n, seed=23, spread=3.0)
    Ao = ocsc(po, A)
    ctx = kkt.KktContext(A)
    assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    ko = oracle.kkt_diag(Ao, maxiter=300)
    assert ko.factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    tol = 0.3 * np.sqrt(st["mu"])
    x1, y1, it1, e1, _ = ctx.kkt_diag_solve(st["a"], st["b"], tol, 300)
    x2, y2, it2, e2, _ = ko.solve(st["a"], st["b"], tol)
    assert e1 == e2 and e1 in (201, 204, 202, 203) and iters_close(it1, it2)
    assert np.isfinite(y1).all() and np.isfinite(x1).all()
    ctx.close()


def ko_precond_apply(oracle, Ao, W, nzd, rhs):
    P, err = oracle.diag_factorize(Ao, W, nzd, True)
    assert err == 0
    return P.apply(rhs)


def test_pcr_trajectory_vs_oracle(kkt, po, oracle):
    m, n = 1500, 3200
    A, st = diag_problem(m, n, seed=33, spread=1.0)
    Ao = ocsc(po, A)
    W = st["xl"] / st["zl"]
    resscale = 1.0 / np.sqrt(W[n:])
    rhs = np.random.default_rng(2).standard_normal(m)
    ctx = kkt.KktContext(A)
    ctx.normal_prepare(W)
    assert ctx.diag_factorize(W, True) == 0
    y1, it1, e1, h1, _ = ctx.pcr_solve(rhs, 1e-8, resscale, 1000, hist_cap=1200)
    P, _ = oracle.diag_factorize(Ao, W, m + 1, True)
    y2, it2, e2, h2 = oracle.pcr_solve(lambda v: oracle.normal_apply(Ao, W, v), P.apply, rhs, 1e-8,
                                       resscale, 1000, hist_cap=1200)
    assert e1 == e2 == 0 and iters_close(it1, it2)
    assert np.abs(h1[:10] - h2[:10]).max() <= 1e-9 * h2[:10].max()
    assert len(h1) == it1 + 1 and h1[-1] <= 1e-8
    assert relerr(y1, y2) < 1e-5
    # nonzero starting iterate takes the general initialisation branch (conjugate_residuals.cc:118-123)
    y0 = 0.1 * np.random.default_rng(3).standard_normal(m)
    y3, it3, e3, _, _ = ctx.pcr_solve(rhs, 1e-8, resscale, 1000, lhs0=y0)
    y4, it4, e4, _ = oracle.pcr_solve(lambda v: oracle.normal_apply(Ao, W, v), P.apply, rhs, 1e-8,
                                      resscale, 1000, lhs0=y0)
    assert e3 == e4 == 0 and iters_close(it3, it4) and relerr(y3, y4) < 1e-5
    # interrupt callback plays Control::InterruptCheck (errflag 999 = IPX_ERROR_interrupt_time)
    _, it5, e5, _, _ = ctx.pcr_solve(rhs, 1e-300, resscale, 100000, interrupt=lambda: 999)
    assert e5 == 999
    ctx.close()


def synth_csc_empty(m):
    from ipx_amd.synth import CscMatrix
    return CscMatrix(m, m, np.zeros(m + 1, np.int64), np.zeros(0, np.int64), np.zeros(0))


def synth_identity_model(m, n):
    """any model matrix of the right shape (the sweeps under test only see L and U)"""
    from ipx_amd import synth
    return synth.synthetic_lp(m, n, 4, 99)


SWEEP_MODES = {
    "default": {},                                   # one-XCD runs for narrow levels, all-XCD runs otherwise
    "levels": {"IPXK_TRISOLVE": "levels"},           # one launch per level
    "allxcd": {"IPXK_SWEEP_NARROW": "0"},            # every run chip-wide (write-through hand-off)
    "nomerge": {"IPXK_SWEEP_MERGE": "0"},            # tiny levels keep a chunk each (no merged chunks)
    "onexcd": {"IPXK_SWEEP_NARROW": "1000000000", "IPXK_SWEEP_MINLEVELS": "1"},   # every run on one XCD
    "onexcd-2wgs": {"IPXK_SWEEP_NARROW": "1000000000", "IPXK_SWEEP_MINLEVELS": "1", "IPXK_SWEEP_XCD_WGS": "2"},
}


@pytest.mark.parametrize("mode", list(SWEEP_MODES))
@pytest.mark.parametrize("m,n,num_free,num_fixed", [(150, 320, 0, 0), (2500, 5200, 6, 9)])
def test_basis_path_vs_oracle(kkt, po, oracle, monkeypatch, mode, m, n, num_free, num_fixed):
    # the sweeps as runs of levels in single launches (the launch plan forced into each of its forms)
    for k, v in SWEEP_MODES[mode].items():
        monkeypatch.setenv(k, v)
    B, st, colscale = basis_problem(m, n, seed=41, num_free=num_free, num_fixed=num_fixed)
    A, L, U = B["A"], B["L"], B["U"]
    AI = A.with_identity()
    ctx = kkt.KktContext(A)
    ctx.split_prepare(L, U, B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
    S = oracle.split_prepare(ocsc(po, AI), n, ocsc(po, L), ocsc(po, U), B["rowperm"], B["colperm"],
                             B["basis"], B["status"], colscale)
    pre = S.get()
    Us = po.Csc(m, m, U.p, U.i, pre["Ux"])
    rhs = np.random.default_rng(4).standard_normal(m)
    # level-scheduled sweeps reproduce the sequential reference arithmetic exactly
    assert np.array_equal(ctx.forward_solve(rhs), oracle.forward_solve(ocsc(po, L), Us, rhs))
    assert np.array_equal(ctx.backward_solve(rhs), oracle.backward_solve(ocsc(po, L), Us, rhs))
    for tr in "NT":
        assert np.array_equal(ctx.solve_dense(rhs, tr), S.solve_dense(rhs, tr))
    lv = ctx.split_levels()
    assert all(1 <= v <= m for v in lv)
    l1, d1 = ctx.split_apply(rhs)
    l2, d2 = S.apply(rhs)
    assert relerr(l1, l2) <= 1e-12 and abs(d1 - d2) <= 1e-12 * abs(d2)
    free = pre["free_positions"]
    assert np.all(l1[free] == 0.0)
    rhs_cr = rhs.copy()
    rhs_cr[free] = 0.0
    y1, it1, e1, h1, _ = ctx.cr_solve(rhs_cr, 1e-9, None, -1, hist_cap=2000)
    y2, it2, e2, h2 = oracle.cr_solve(S.apply, rhs_cr, 1e-9, None, -1, hist_cap=2000)
    assert e1 == e2 == 0 and iters_close(it1, it2) and relerr(y1, y2) < 1e-6
    assert np.abs(h1[:10] - h2[:10]).max() <= 1e-9 * h2[:10].max()
    x1, yy1, it1, e1, _ = ctx.kkt_basis_solve(st["a"], st["b"], 1e-8)
    x2, yy2, it2, e2, _ = S.kkt_solve(st["a"], st["b"], 1e-8)
    assert e1 == e2 == 0 and iters_close(it1, it2)
    assert relerr(x1, x2) < 1e-6 and relerr(yy1, yy2) < 1e-6
    AIs = AI.to_scipy()
    assert relerr(AIs @ x1, st["b"]) < 1e-9
    ctx.close()


def test_real_N_matrix_vs_oracle_and_masked_form(kkt, po, oracle, monkeypatch):
    """N built on the device as a matrix of its own (nmatrix.hip; the slice size shrunk so that a small model
    qualifies): the split operator against the oracle (1e-12), against the masked / compacted model-matrix form
    (1e-13: the same products, another association across the slices of the compact vector), a rescale with other
    weights and with another set of fixed variables (N must be rebuilt), and the KKT solve"""
    monkeypatch.setenv("IPXK_SPMV_LAYOUT", "sliced")
    monkeypatch.setenv("IPXK_SLICE_TEST_KB", "4")
    m, n = 2500, 5200
    B, st, colscale = basis_problem(m, n, seed=41, num_free=6, num_fixed=9)
    A, L, U = B["A"], B["L"], B["U"]
    AI = A.with_identity()
    rhs = np.random.default_rng(4).standard_normal(m)
    out = {}
    for real in ("1", "0"):
        monkeypatch.setenv("IPXK_REAL_N", real)
        monkeypatch.setenv("IPXK_VERBOSE", "1")
        ctx = kkt.KktContext(A)
        assert ctx.spmv_layout()[0] == ("sliced", "sliced")
        ctx.split_prepare(L, U, B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
        l1, d1 = ctx.split_apply(rhs)
        x1, yy1, it1, e1, _ = ctx.kkt_basis_solve(st["a"], st["b"], 1e-8)
        # other weights on the same columns; then some more columns fixed (weight 0): another N
        cs2 = colscale * np.where(np.isfinite(colscale) & (colscale > 0), 10.0 ** np.random.default_rng(8).uniform(-0.3, 0.3, n + m), 1.0)
        ctx.split_rescale(B["status"], cs2)
        l2, d2 = ctx.split_apply(rhs)
        status3 = B["status"].copy()
        nb = np.nonzero(status3[:n] == -1)[0][:40]
        status3[nb] = -2                                          # NONBASIC_FIXED
        cs3 = cs2.copy()
        cs3[nb] = 0.0
        ctx.split_rescale(status3, cs3)
        l3, d3 = ctx.split_apply(rhs)
        out[real] = (l1, d1, x1, yy1, it1, e1, l2, l3)
        ctx.close()
    S = oracle.split_prepare(ocsc(po, AI), n, ocsc(po, L), ocsc(po, U), B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
    lo, do = S.apply(rhs)
    a, b = out["1"], out["0"]
    assert relerr(a[0], lo) <= 1e-12 and abs(a[1] - do) <= 1e-12 * abs(do)
    for k in (0, 6, 7):
        assert relerr(a[k], b[k]) <= 1e-13, k
    assert not np.array_equal(a[0], b[0])                          # ... so N was really used (its slices are those of the compact t)
    assert not np.array_equal(a[6], a[7])                          # the fixed columns did change the operator
    assert a[5] == b[5] == 0 and abs(a[4] - b[4]) <= 2 and relerr(a[2], b[2]) < 1e-6 and relerr(a[3], b[3]) < 1e-6


def test_inverted_head_and_tail_of_the_sweeps(kkt, po, oracle, monkeypatch, capfd):
    """Sweep::Block (trisolve.hpp): the first levels of the transposed sweeps and the last levels of every sweep --
    few unknowns, one hand-off each -- replaced by x2 = inverse(T22) (b2 - T21 x1).  The bound on the dimension is
    lowered so that a 60 000-row planted basis qualifies.  Against the level-scheduled form (whose arithmetic is the
    oracle's, bit for bit: the other tests) the solves agree to 1e-12; unscaled (Basis::SolveDense) and scaled (the
    operator, after a rescale too: the inverse is that of the UNSCALED block, the column scaling of U is applied
    around it)."""
    m, n = 60000, 125000
    B, st, colscale = basis_problem(m, n, seed=23)
    A, L, U = B["A"], B["L"], B["U"]
    rng = np.random.default_rng(9)
    rhs = rng.standard_normal(m)
    cs2 = colscale * np.where(np.isfinite(colscale) & (colscale > 0), 10.0 ** rng.uniform(-0.5, 0.5, n + m), 1.0)
    out = {}
    monkeypatch.setenv("IPXK_TAIL_MIN_DIM", "1000")
    monkeypatch.setenv("IPXK_VERBOSE", "1")
    for cap in ("900", "0"):
        monkeypatch.setenv("IPXK_TAIL_INVERSE", cap)
        monkeypatch.setenv("IPXK_HEAD_INVERSE", cap)
        ctx = kkt.KktContext(A)
        ctx.split_prepare(L, U, B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
        err = capfd.readouterr().err
        print(err)
        assert (err.count("sweep tail: levels") >= 2 and err.count("sweep head: levels") == 2) == (cap != "0"), err
        fwd = ctx.solve_dense(rhs, "N")
        bwd = ctx.solve_dense(rhs, "T")
        l1, d1 = ctx.split_apply(rhs)
        ctx.split_rescale(B["status"], cs2)
        l2, d2 = ctx.split_apply(rhs)
        x, y, it, e, _ = ctx.kkt_basis_solve(st["a"], st["b"], 1e-8)
        out[cap] = (fwd, bwd, l1, l2, x, y, it, e)
        ctx.close()
    a, b = out["900"], out["0"]
    Bm = A.to_scipy()[:, :m]                                                      # basis[p] = p
    for v in (a, b):
        assert relerr(Bm @ v[0], rhs) <= 1e-10 and relerr(Bm.T @ v[1], rhs) <= 1e-10
    for k in (0, 1, 2, 3):
        assert relerr(a[k], b[k]) <= 1e-12, (k, relerr(a[k], b[k]))
        assert not np.array_equal(a[k], b[k])
    # (CR to 1e-8 takes ~255 iterations here; the count moves by a few with the rounding of the operator)
    assert a[7] == b[7] == 0 and abs(a[6] - b[6]) <= 3 + b[6] // 50 and relerr(a[4], b[4]) < 1e-6 and relerr(a[5], b[5]) < 1e-6


def test_ill_conditioned_block_is_not_inverted(kkt, monkeypatch, capfd):
    """The guard of the explicit inverses (inverse_guard.hpp; IPX's bases get ill conditioned late in a solve: that is what
    the stability loop of src/basis.cc:130-152 and the residual test of src/lu_factorization.cc:87-127 are for).  A
    planted basis whose L has entries of magnitude 3 in its last rows: along the dependency chains of those rows the
    inverse of the tail block grows like 3^depth (probe residual |T M z - z| ~ 1e2, i.e. cond * eps with cond ~ 1e18).
    Substitution with that block is backward stable, a product with its computed inverse is not.  With the guard the
    block keeps its level-scheduled solve and B x = r is solved to 1e-9 for a right-hand side with a moderate solution;
    with the guard switched off (IPXK_INVERSE_TOL=1e300) the same solve is wrong by orders of magnitude, which shows
    that the planted block does what it is meant to."""
    from ipx_amd import synth
    m, n = 60000, 130000
    B = synth.planted_lu_basis(synth.synthetic_lp(m, n, 8, 3), seed=3, big_rows=0.03, big=3.0)
    cs = synth.synthetic_basis_state(B["status"], 1.0, 3)
    Bm = B["A"].to_scipy()[:, :m].tocsr()
    xt = np.random.default_rng(1).standard_normal(m)
    monkeypatch.setenv("IPXK_TAIL_MIN_DIM", "1000")
    monkeypatch.setenv("IPXK_VERBOSE", "1")
    res = {}
    for tol in ("1e-10", "1e300"):
        monkeypatch.setenv("IPXK_INVERSE_TOL", tol)
        ctx = kkt.KktContext(B["A"])
        ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], cs)
        probes, rejected, worst = ctx.split_inverse_stats()
        err = capfd.readouterr().err
        assert probes >= 3 and worst >= 1e-4, (probes, worst)              # cond * eps >= 1e-4: cond >= 1e12
        assert (rejected >= 1) == (tol == "1e-10") and ("REJECTED" in err) == (tol == "1e-10"), (rejected, err)
        out = []
        for trans, M in (("N", Bm), ("T", Bm.T)):
            r = M @ xt
            x = ctx.solve_dense(r, trans)
            out.append(float(np.abs(M @ x - r).max() / np.abs(r).max()))
        res[tol] = out
        ctx.close()
    assert max(res["1e-10"]) <= 1e-9, res
    assert max(res["1e300"]) >= 1e-6, res          # the unguarded inverse really is that bad on this block


def test_guard_that_rejects_everything_equals_no_blocks(kkt, monkeypatch):
    """IPXK_INVERSE_TOL=0 rejects every inverted block: the operator must then be, bit for bit, the one built with
    the blocks switched off (IPXK_TAIL_INVERSE=0, IPXK_HEAD_INVERSE=0) -- the fall-back leaves nothing behind."""
    m, n = 60000, 125000
    B, st, colscale = basis_problem(m, n, seed=23)
    rhs = np.random.default_rng(9).standard_normal(m)
    monkeypatch.setenv("IPXK_TAIL_MIN_DIM", "1000")
    out = []
    for env in ({"IPXK_INVERSE_TOL": "0"}, {"IPXK_TAIL_INVERSE": "0", "IPXK_HEAD_INVERSE": "0"}):
        for k in ("IPXK_INVERSE_TOL", "IPXK_TAIL_INVERSE", "IPXK_HEAD_INVERSE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctx = kkt.KktContext(B["A"])
        ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
        out.append((ctx.solve_dense(rhs, "N"), ctx.solve_dense(rhs, "T"), ctx.split_apply(rhs)[0], ctx.split_inverse_stats()))
        ctx.close()
    assert out[0][3][1] == out[0][3][0] >= 3 and out[1][3][0] == 0          # all probed blocks rejected / no block built
    for k in range(3):
        assert np.array_equal(out[0][k], out[1][k]), k


def test_inverted_blocks_on_chains_of_tiny_levels(kkt, po, oracle, monkeypatch, capfd):
    """a block must start and end with a chunk: factors whose levels hold one or two unknowns each (a bidiagonal L
    under a banded U: long stretches of MERGED chunks) with the blocks forced on -- Prepare must not trip over a block
    boundary inside a merged chunk, and the solves agree with the level-scheduled form"""
    import scipy.sparse as sp
    from ipx_amd.synth import CscMatrix
    m, n = 40000, 80500                                                       # (a block holds at most dim / 64 unknowns and at least 256)
    rng = np.random.default_rng(12)
    sub = rng.uniform(0.1, 0.5, m - 1) * rng.choice([-1.0, 1.0], m - 1)
    Lm = sp.diags(sub, -1, shape=(m, m), format="csc")                        # a pure chain: m levels of one unknown
    Lm.sort_indices()
    up = rng.uniform(0.1, 0.5, m - 2) * rng.choice([-1.0, 1.0], m - 2)
    Um = (sp.diags(rng.uniform(0.5, 2.0, m) * rng.choice([-1.0, 1.0], m)) + sp.diags(up, 2, shape=(m, m))).tocsc()   # two interleaved chains
    Um.sort_indices()
    L = CscMatrix(m, m, Lm.indptr, Lm.indices, Lm.data)
    U = CscMatrix(m, m, Um.indptr, Um.indices, Um.data)
    A = synth_identity_model(m, n)
    ident = np.arange(m, dtype=np.int64)
    status = np.full(n + m, -1, dtype=np.int64); status[:m] = 0
    colscale = np.ones(n + m)
    rhs = rng.standard_normal(m)
    out = {}
    monkeypatch.setenv("IPXK_TAIL_MIN_DIM", "1000")
    monkeypatch.setenv("IPXK_VERBOSE", "1")
    for cap in ("1000", "0"):
        monkeypatch.setenv("IPXK_TAIL_INVERSE", cap)
        monkeypatch.setenv("IPXK_HEAD_INVERSE", cap)
        ctx = kkt.KktContext(A)
        ctx.split_prepare(L, U, ident, ident, ident, status, colscale)
        err = capfd.readouterr().err
        assert (err.count("inverted") >= 4) == (cap != "0"), err                 # heads and tails of the sweeps over L and U
        out[cap] = (ctx.solve_dense(rhs, "N"), ctx.solve_dense(rhs, "T"))
        ctx.close()
    Lo, Uo = ocsc(po, L), ocsc(po, U)
    assert np.array_equal(out["0"][0], oracle.forward_solve(Lo, Uo, rhs)) and np.array_equal(out["0"][1], oracle.backward_solve(Lo, Uo, rhs))
    for k in (0, 1):
        assert relerr(out["1000"][k], out["0"][k]) <= 1e-11, (k, relerr(out["1000"][k], out["0"][k]))


def test_level_analysis_one_launch_against_the_relaxation(kkt, monkeypatch):
    """the dependency levels of the four sweeps from ONE sync-free launch (level_sweep_kernel, the default) and from the
    relaxation launches it replaced (IPXK_LEVEL_SWEEP=0, kept as the fall-back): the same levels, hence the same packed
    factors and bit-identical solves -- on planted factors, on a banded structure with thousands of levels and on factors
    with rows and columns of hundreds of entries (the rows the wavefront evaluates together)"""
    import scipy.sparse as sp
    from ipx_amd.synth import CscMatrix
    rng = np.random.default_rng(21)
    cases = [basis_problem(30000, 62000, seed=61), basis_problem(6000, 12500, seed=47, band=12)]
    for B, st, colscale in cases:
        m = B["A"].nrow
        rhs = rng.standard_normal(m)
        out = {}
        for mode in ("1", "0"):
            monkeypatch.setenv("IPXK_LEVEL_SWEEP", mode)
            ctx = kkt.KktContext(B["A"])
            ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
            out[mode] = (ctx.split_levels(), ctx.forward_solve(rhs), ctx.backward_solve(rhs), ctx.split_apply(rhs)[0])
            ctx.close()
        assert out["1"][0] == out["0"][0]
        for k in (1, 2, 3):
            assert np.array_equal(out["1"][k], out["0"][k]), k
    # long rows: a few rows / columns of 300 entries in L and U
    m, n = 4000, 8200
    def tri(lower):
        rows, cols = [], []
        for j in range(m - 1):
            k = rng.integers(0, 4)
            r = np.unique(rng.integers(j + 1, m, size=k)) if lower else np.unique(rng.integers(0, j + 1, size=k))
            rows.append(r); cols.append(np.full(r.size, j if lower else j + 1))
        for i in (m - 1, m - 9, m // 2):
            c = rng.choice(i, size=300, replace=False)
            rows.append(np.full(300, i) if lower else c); cols.append(c if lower else np.full(300, i))
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        v = rng.uniform(0.05, 0.3, rows.size) * rng.choice([-1.0, 1.0], rows.size)
        T = sp.coo_matrix((v, (rows, cols)), shape=(m, m)).tocsc()
        T.sum_duplicates()
        return sp.tril(T, -1).tocsc() if lower else sp.triu(T, 1).tocsc()
    Lm = tri(True); Lm.sort_indices()
    Um = (tri(False) + sp.diags(rng.uniform(0.5, 2.0, m) * rng.choice([-1.0, 1.0], m))).tocsc(); Um.sort_indices()
    L = CscMatrix(m, m, Lm.indptr, Lm.indices, Lm.data); U = CscMatrix(m, m, Um.indptr, Um.indices, Um.data)
    A = synth_identity_model(m, n)
    ident = np.arange(m, dtype=np.int64)
    status = np.full(n + m, -1, dtype=np.int64); status[:m] = 0
    rhs = rng.standard_normal(m)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("IPXK_LEVEL_SWEEP", mode)
        ctx = kkt.KktContext(A)
        ctx.split_prepare(L, U, ident, ident, ident, status, np.ones(n + m))
        out[mode] = (ctx.split_levels(), ctx.solve_dense(rhs, "N"), ctx.solve_dense(rhs, "T"))
        ctx.close()
    assert out["1"][0] == out["0"][0] and np.array_equal(out["1"][1], out["0"][1]) and np.array_equal(out["1"][2], out["0"][2])


def test_operator_timers(kkt):
    """ipx_info::time_cr1_AAt / time_cr1_pre / time_cr2_NNt / _B / _Bt equivalents (ipxk_times)."""
    A, st = diag_problem(20000, 42000, seed=77)
    ctx = kkt.KktContext(A)
    ctx.set_profiling(True)
    assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    x, y, it, e, tm = ctx.kkt_diag_solve(st["a"], st["b"], 1e-3, 500)
    assert e == 0 and tm.cr > 0 and tm.op > 0 and tm.precond > 0
    assert tm.op + tm.precond <= tm.cr * 1.05 and tm.op > tm.precond
    ctx.set_profiling(False)
    _, _, _, _, tm2 = ctx.kkt_diag_solve(st["a"], st["b"], 1e-3, 500)
    assert tm2.cr > 0 and tm2.op == 0.0
    ctx.close()
    B, st, colscale = basis_problem(3000, 6500, seed=78)
    ctx = kkt.KktContext(B["A"])
    ctx.set_profiling(True)
    ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
    _, _, it, e, tm = ctx.kkt_basis_solve(st["a"], st["b"], 1e-8)
    assert e == 0 and min(tm.op, tm.solve_B, tm.solve_Bt) > 0
    assert tm.op + tm.solve_B + tm.solve_Bt <= tm.cr * 1.05
    ctx.close()


# --------------------------------------------------------------------------------------
# edge cases: empty rows / columns, tiny and ragged shapes, iteration caps
# --------------------------------------------------------------------------------------
def test_edge_cases(kkt, po, oracle):
    import scipy.sparse as sp
    from ipx_amd.synth import CscMatrix
    rng = np.random.default_rng(9)
    for (m, n, dens) in [(1, 1, 1.0), (5, 4, 0.0), (7, 3, 0.5), (40, 90, 0.05), (300, 17, 0.02), (33, 700, 0.01)]:
        M = sp.random(m, n, density=dens, random_state=int(rng.integers(1 << 30)), format="csc")
        M.sort_indices()
        A = CscMatrix(m, n, M.indptr, M.indices, M.data)       # has empty rows and columns
        ctx = kkt.KktContext(A)
        W = 10.0 ** rng.uniform(-1, 1, n + m)
        rhs = rng.standard_normal(m)
        ctx.normal_prepare(W)
        l1, d1 = ctx.normal_apply(rhs)
        l2, d2 = oracle.normal_apply(ocsc(po, A), W, rhs)
        assert relerr(l1, l2) <= 1e-12 and abs(d1 - d2) <= 1e-12 * max(abs(d2), 1e-300)
        assert ctx.diag_factorize(W, True) == 0
        y, it, e, hist, _ = ctx.pcr_solve(rhs, 1e-10, None, -1, hist_cap=m + 200)
        assert e == 0 and relerr(ctx.normal_apply(y)[0], rhs) < 1e-8
        _, it, e, _, _ = ctx.pcr_solve(rhs, 1e-300, None, 0)     # maxiter = 0
        assert (it, e) == (0, 201)
        _, it, e, _, _ = ctx.pcr_solve(np.zeros(m), 1e-10, None, 50)   # zero rhs converges at once
        assert (it, e) == (0, 0)
        ctx.close()
    with pytest.raises(kkt.KktError):
        bad = CscMatrix(3, 2, [0, 1, 2], [0, 5], [1.0, 1.0])   # row index out of range
        kkt.KktContext(bad)


def test_reset_solver_state(kkt):
    """ipxk_reset_solver_state (what HipModel calls when it hands a cached context to the next solver object): nothing the
    previous object prepared can be used any more, the model stays, and a new factorization gives the same answer as before"""
    A, st = diag_problem(3000, 7000, seed=77)
    B = basis_problem(600, 1300, seed=78)
    ctx = kkt.KktContext(A)
    assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    tol = 0.3 * np.sqrt(st["mu"])
    x1, y1, it1, e1, _ = ctx.kkt_diag_solve(st["a"], st["b"], tol, 500)
    ctx.reset_solver_state(0.0625)
    with pytest.raises(kkt.KktError):
        ctx.kkt_diag_solve(st["a"], st["b"], tol, 500)
    with pytest.raises(kkt.KktError):
        ctx.normal_apply(st["b"])
    assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    x2, y2, it2, e2, _ = ctx.kkt_diag_solve(st["a"], st["b"], tol, 500)
    assert (it1, e1) == (it2, e2) and np.array_equal(x1, x2) and np.array_equal(y1, y2)
    ctx.close()
    # basis path: operator and factors are gone after the reset; Prepare again reproduces the solve bit for bit
    Bp, st2, cs = B
    ctx = kkt.KktContext(Bp["A"])
    ctx.split_prepare(Bp["L"], Bp["U"], Bp["rowperm"], Bp["colperm"], Bp["basis"], Bp["status"], cs)
    xb, yb, itb, eb, _ = ctx.kkt_basis_solve(st2["a"], st2["b"], 1e-8)
    ctx.reset_solver_state()
    with pytest.raises(kkt.KktError):
        ctx.kkt_basis_solve(st2["a"], st2["b"], 1e-8)
    with pytest.raises(kkt.KktError):
        ctx.split_apply(st2["b"])
    ctx.split_prepare(Bp["L"], Bp["U"], Bp["rowperm"], Bp["colperm"], Bp["basis"], Bp["status"], cs)
    xb2, yb2, itb2, eb2, _ = ctx.kkt_basis_solve(st2["a"], st2["b"], 1e-8)
    assert (itb, eb) == (itb2, eb2) and np.array_equal(xb, xb2) and np.array_equal(yb, yb2)
    ctx.close()


# --------------------------------------------------------------------------------------
# BASELINE sizes: size-independent properties (the oracle would take minutes here)
# --------------------------------------------------------------------------------------
def test_full_size_properties(kkt):
    m, n = 1000000, 2000000
    A, st = diag_problem(m, n, seed=12345, spread=1.0)
    ctx = kkt.KktContext(A)
    W = st["xl"] / st["zl"]
    ctx.normal_prepare(W)
    rng = np.random.default_rng(0)
    u, v = rng.standard_normal(m), rng.standard_normal(m)
    Cu, uCu = ctx.normal_apply(u)
    Cv, vCv = ctx.normal_apply(v)
    Cuv, _ = ctx.normal_apply(u + 2.0 * v)
    assert relerr(Cuv, Cu + 2.0 * Cv) < 1e-12            # linearity
    assert abs(np.dot(v, Cu) - np.dot(u, Cv)) <= 1e-11 * abs(np.dot(v, Cu))   # symmetry
    assert uCu > 0 and vCv > 0 and abs(uCu - np.dot(u, Cu)) <= 1e-12 * uCu    # SPD, fused dot
    S = A.to_scipy()                                      # independent check with scipy
    ref = S @ (W[:n] * (S.T @ u)) + W[n:] * u
    assert relerr(Cu, ref) < 1e-12
    assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    tol = 0.3 * np.sqrt(st["mu"])
    x, y, it, e, _ = ctx.kkt_diag_solve(st["a"], st["b"], tol, 500)
    assert e == 0 and 20 <= it <= 200
    # the same solve by the CPU checker at full size (the reference's own KKTSolverDiag when oracle/_ref is there,
    # else the restatement that is pinned bitwise against it): identical errflag, iteration counts within
    # max(2, 2 %) (SURVEY 8d parity gate; the bench line's 80 / 80), solutions to the accuracy 80 CR iterations leave
    from oracle import pyoracle as po
    Ao = po.Csc(m, n, A.p, A.i, A.x)
    if po.ref_available():
        v = synth.lp_vectors(m, n)
        rm = po.Ref().model(Ao, v["rhs"], v["constr_type"], v["obj"], v["lb"], v["ub"])
        assert rm.m == m and rm.n == n and not rm.dualized
        k = rm.kkt_diag(maxiter=500)
        k.factorize(np.ones(n + m), st["xl"], st["xu"], np.zeros(m), st["zl"], st["zu"])
        xr, yr, itr, er = k.solve(st["a"], st["b"], tol)
    else:
        k = po.Oracle().kkt_diag(Ao, maxiter=500)
        k.factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"])
        xr, yr, itr, er, _ = k.solve(st["a"], st["b"], tol)
    assert er == 0 and abs(it - itr) <= max(2, 0.02 * itr), (it, itr)
    # (the final iterate of an 80-iteration run that stops at tol = 0.3 sqrt(mu) is only determined to about tol
    # relative to the solution -- measured 2e-4 --, SURVEY 8d: gate on iteration counts and on the residual below)
    assert relerr(y, yr) < 5e-3 and relerr(x, xr) < 5e-3
    res1, res2 = kkt_residual_diag(A, W, st["a"], st["b"], x, y)
    assert np.abs(res2).max() < 1e-8 * (1 + np.abs(x).max())
    assert np.abs(np.sqrt(W[n:]) * res1[n:]).max() <= tol * (1 + 1e-9)
    assert np.abs(res1[:n]).max() < 1e-8 * np.abs(x[:n] / W[:n]).max()
    ctx.close()


# --------------------------------------------------------------------------------------
# the three SpMV layouts (phased / XCD-sliced tiles / fused tiles) on a matrix large enough for the sliced one
# --------------------------------------------------------------------------------------
def test_spmv_layouts_agree(kkt, po, oracle, monkeypatch):
    m, n = 300000, 700000                      # A t gathers from 5.6 MB: sliced layout eligible
    A, st = diag_problem(m, n, seed=77)
    W = st["xl"] / st["zl"]
    rng = np.random.default_rng(5)
    u = rng.standard_normal(m)
    ref, ref_dot = oracle.normal_apply(ocsc(po, A), W, u)
    out = {}
    for layout in ("phased", "sliced", "fused", "acc"):
        monkeypatch.setenv("IPXK_SPMV_LAYOUT", layout)
        ctx = kkt.KktContext(A)
        assert ctx.spmv_layout()[0][1] == layout
        ctx.normal_prepare(W)
        lhs, dot = ctx.normal_apply(u)
        assert relerr(lhs, ref) < 1e-12 and abs(dot - ref_dot) <= 1e-12 * abs(ref_dot), layout
        assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
        x, y, it, e, _ = ctx.kkt_diag_solve(st["a"], st["b"], 0.3 * np.sqrt(st["mu"]), 500)
        out[layout] = (lhs, x, y, it, e)
        ctx.close()
    assert np.array_equal(out["phased"][0], ref)        # phased layout: the reference's summation order
    assert np.array_equal(out["fused"][0], ref)         # fused tiles: one slice, same order
    # (the dot products are reduced over different workgroup partitions, so solves agree to rounding only)
    assert relerr(out["fused"][2], out["phased"][2]) < 1e-8 and abs(out["fused"][3] - out["phased"][3]) <= 2
    assert relerr(out["sliced"][0], out["phased"][0]) < 1e-14
    # accumulated tiles: a row is summed in ascending address order = the storage order of these (sorted) rows
    assert np.array_equal(out["acc"][0], out["sliced"][0]) and out["acc"][3] == out["sliced"][3]
    assert np.array_equal(out["acc"][2], out["sliced"][2])
    assert out["sliced"][4] == out["phased"][4] == 0 and abs(out["sliced"][3] - out["phased"][3]) <= 2
    assert relerr(out["sliced"][2], out["phased"][2]) < 1e-8


def test_sorted_fused_layout_on_a_banded_matrix(kkt, po, oracle, monkeypatch):
    """gathers with locality (8 rows per column inside a 2048-row band): the fused tiles with the gathers of a tile
    in address order -- row sums in the reference's order, bit for bit, like the phased and fused layouts; the
    layout is refused (and the phased one used) when a tile's window of x is too wide"""
    m, n = 120000, 250000
    A = synth.banded_lp(m, n, 8, 2048, 5)
    rng = np.random.default_rng(2)
    W = 10.0 ** rng.uniform(-2, 2, n + m)
    u = rng.standard_normal(m)
    ref, ref_dot = oracle.normal_apply(ocsc(po, A), W, u)
    res = {}
    for layout in ("phased", "sortedfused", "accfused", None):       # accfused: the fused accumulated tiles (round 4), same bits
        if layout: monkeypatch.setenv("IPXK_SPMV_LAYOUT", layout)
        else: monkeypatch.delenv("IPXK_SPMV_LAYOUT")
        ctx = kkt.KktContext(A)
        if layout: assert ctx.spmv_layout()[0] == (layout, layout)
        ctx.normal_prepare(W)
        lhs, dot = ctx.normal_apply(u)
        assert np.array_equal(lhs, ref) and abs(dot - ref_dot) <= 1e-12 * abs(ref_dot), layout
        st = synth.synthetic_ipm_state(m, n, 1.0, 5)
        assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
        x, y, it, e, _ = ctx.kkt_diag_solve(st["a"], st["b"], 0.3 * np.sqrt(st["mu"]), 500)
        res[layout] = (x, y, it, e, ctx.spmv_layout())
        ctx.close()
    assert res["sortedfused"][3] == res["phased"][3] == 0 and abs(res["sortedfused"][2] - res["phased"][2]) <= 2
    assert relerr(res["sortedfused"][1], res["phased"][1]) < 1e-8
    assert res["accfused"][3] == 0 and abs(res["accfused"][2] - res["phased"][2]) <= 2 and relerr(res["accfused"][1], res["phased"][1]) < 1e-8
    print("auto choice on the banded matrix:", res[None][4])
    # uniformly random indices: no tile has a narrow window -> not built, the phased layout serves
    monkeypatch.setenv("IPXK_SPMV_LAYOUT", "sortedfused")
    A2, _ = diag_problem(20000, 600000, seed=3)
    ctx = kkt.KktContext(A2)
    assert ctx.spmv_layout()[0][1] == "phased"
    ctx.close()


def test_split_prepare_rejects_bad_factors(kkt):
    """indices that violate the factor contract (src/lu_update.h:43-60) are refused before any kernel uses them"""
    m, n = 300, 700
    B, st, colscale = basis_problem(m, n, seed=51)
    ctx = kkt.KktContext(B["A"])
    args = lambda L, U, rp=B["rowperm"], cp=B["colperm"]: (L, U, rp, cp, B["basis"], B["status"], colscale)
    ctx.split_prepare(*args(B["L"], B["U"]))                        # the good factors are accepted
    from ipx_amd.synth import CscMatrix
    L, U = B["L"], B["U"]
    bad_i = L.i.copy(); bad_i[len(bad_i) // 2] = m + 5               # row index out of range
    with pytest.raises(kkt.KktError):
        ctx.split_prepare(*args(CscMatrix(m, m, L.p, bad_i, L.x), U))
    bad_i = L.i.copy(); bad_i[0] = 0                                  # not strictly lower (column 0 holds row 0)
    with pytest.raises(kkt.KktError):
        ctx.split_prepare(*args(CscMatrix(m, m, L.p, bad_i, L.x), U))
    bad_u = U.i.copy(); bad_u[U.p[m // 2 + 1] - 1] = 0                # diagonal not last
    with pytest.raises(kkt.KktError):
        ctx.split_prepare(*args(L, CscMatrix(m, m, U.p, bad_u, U.x)))
    rp = B["rowperm"].copy(); rp[1] = rp[0]                           # not a permutation
    with pytest.raises(kkt.KktError):
        ctx.split_prepare(*args(L, U, rp=rp))
    ctx.split_prepare(*args(L, U))                                    # and the context is still usable
    assert ctx.split_levels()[0] >= 1
    ctx.close()


def test_sweeps_with_a_spike_of_70000_entries(kkt, po, oracle):
    """factors as a torn LU leaves them (lu.hip step 2b): columns of U that hold most of the dimension -- more than
    65 535 entries, which the packed layout's 16-bit row length could not hold (a GPU memory fault at 1M rows before
    the length word was widened to 24 bits) -- and the rows of U that cross them; L empty, two spikes, a sparse rest"""
    import scipy.sparse as sp
    from ipx_amd.synth import CscMatrix
    m, n = 72000, 150000
    rng = np.random.default_rng(5)
    rows, cols = [], []
    for j in range(1, m - 2):                                     # one random entry above the diagonal in most columns
        if rng.random() < 0.7:
            rows.append(rng.integers(0, j)); cols.append(j)
    for j, cnt in ((m - 1, 70000), (m - 2, 66000)):              # the spikes
        r = rng.choice(j, size=cnt, replace=False)
        rows += list(r); cols += [j] * cnt
    rows, cols = np.array(rows), np.array(cols)
    vals = rng.uniform(0.05, 0.3, rows.size) * rng.choice([-1.0, 1.0], rows.size) / np.sqrt(1 + np.bincount(cols, minlength=m)[cols])
    Um = (sp.coo_matrix((vals, (rows, cols)), shape=(m, m)) + sp.diags(rng.uniform(0.5, 2.0, m) * rng.choice([-1.0, 1.0], m))).tocsc()
    Um.sum_duplicates(); Um.sort_indices()
    U = CscMatrix(m, m, Um.indptr, Um.indices, Um.data)
    A = synth_identity_model(m, n)
    ctx = kkt.KktContext(A)
    ident = np.arange(m, dtype=np.int64)
    status = np.full(n + m, -1, dtype=np.int64); status[:m] = 0
    colscale = np.ones(n + m)
    ctx.split_prepare(synth_csc_empty(m), U, ident, ident, ident, status, colscale)
    rhs = rng.standard_normal(m)
    Lnone = po.Csc(m, m, np.zeros(m + 1, np.int64), np.zeros(0, np.int64), np.zeros(0))
    Uo = ocsc(po, U)
    # U' (transposed, ascending): every row in the reference's order, the 70000-entry ones included
    assert np.array_equal(ctx.solve_dense(rhs, "T"), oracle.backward_solve(Lnone, Uo, rhs))
    # U (forward, descending): rows crossing the spikes
    assert np.array_equal(ctx.solve_dense(rhs, "N"), oracle.forward_solve(Lnone, Uo, rhs))
    ctx.close()


@pytest.mark.parametrize("mode", ["default", "allxcd", "onexcd", "nomerge"])
def test_sweeps_with_dense_rows_and_columns(kkt, po, oracle, monkeypatch, mode):
    """factors with a few rows AND columns of 70 / 300 / 1500 entries next to short ones: rows longer than
    one 64-entry round of the 8-lane form in all four sweeps (dense rows of L and U in the forward sweeps,
    dense columns in the transposed ones); still bit-identical to the sequential reference arithmetic -- except
    the L' sweep, whose rows of more than 64 entries are summed round by round from their END (their first
    entries are the unknowns solved last: taking those first would stall every round behind the chain), which
    changes the association of those few sums: 1e-13 there"""
    import scipy.sparse as sp
    from ipx_amd.synth import CscMatrix
    for k, v in SWEEP_MODES[mode].items():
        monkeypatch.setenv(k, v)
    m, n = 3000, 6100
    rng = np.random.default_rng(77)

    def strict_lower():
        rows, cols = [], []
        for j in range(m - 1):                                    # 0..3 random entries below the diagonal
            k = rng.integers(0, 4)
            r = np.unique(rng.integers(j + 1, m, size=k))
            rows.append(r); cols.append(np.full(r.size, j))
        for i, cnt in ((m - 1, 1500), (m - 7, 300), (m // 2, 70)):  # dense rows
            c = rng.choice(i, size=cnt, replace=False)
            rows.append(np.full(cnt, i)); cols.append(c)
        for j, cnt in ((0, 1500), (5, 300), (m // 3, 70)):          # dense columns
            r = j + 1 + rng.choice(m - j - 1, size=cnt, replace=False)
            rows.append(r); cols.append(np.full(cnt, j))
        rows, cols = np.concatenate(rows), np.concatenate(cols)
        vals = rng.uniform(0.05, 0.3, rows.size) * rng.choice([-1.0, 1.0], rows.size) / np.sqrt(1 + np.bincount(rows, minlength=m)[rows])
        T = sp.coo_matrix((vals, (rows, cols)), shape=(m, m)).tocsc()
        T.sum_duplicates(); T.sort_indices()
        return T

    Lm = strict_lower()
    Um = (strict_lower().T + sp.diags(rng.uniform(0.5, 2.0, m) * rng.choice([-1.0, 1.0], m))).tocsc()
    Um.sort_indices()                                                # diagonal last in each column
    mk = lambda M: CscMatrix(m, m, M.indptr, M.indices, M.data)
    L, U = mk(Lm), mk(Um)
    A = synth_identity_model(m, n)
    ctx = kkt.KktContext(A)
    ident = np.arange(m, dtype=np.int64)
    status = np.full(n + m, -1, dtype=np.int64); status[:m] = 0
    colscale = 10.0 ** rng.uniform(-1, 1, n + m)
    ctx.split_prepare(L, U, ident, ident, ident, status, colscale)
    Us = po.Csc(m, m, U.p, U.i, U.x * np.repeat(colscale[:m], np.diff(U.p)))     # ScaleColumn of the BASIC columns
    rhs = rng.standard_normal(m)
    assert np.array_equal(ctx.forward_solve(rhs), oracle.forward_solve(ocsc(po, L), Us, rhs))
    assert relerr(ctx.backward_solve(rhs), oracle.backward_solve(ocsc(po, L), Us, rhs)) < 1e-13
    # unscaled factors: Basis::SolveDense with identity permutations
    Uo = ocsc(po, U)
    assert np.array_equal(ctx.solve_dense(rhs, "N"), oracle.forward_solve(ocsc(po, L), Uo, rhs))
    assert relerr(ctx.solve_dense(rhs, "T"), oracle.backward_solve(ocsc(po, L), Uo, rhs)) < 1e-13
    # the U' sweep alone keeps the reference's order for every row: a right-hand side that L' leaves alone
    Lnone = po.Csc(m, m, np.zeros(m + 1, np.int64), np.zeros(0, np.int64), np.zeros(0))
    ctx.split_prepare(synth_csc_empty(m), U, ident, ident, ident, status, colscale)
    assert np.array_equal(ctx.solve_dense(rhs, "T"), oracle.backward_solve(Lnone, Uo, rhs))
    ctx.close()


@pytest.mark.parametrize("mode", ["default", "allxcd", "onexcd", "nomerge"])
def test_deep_level_structure(kkt, po, oracle, monkeypatch, mode):
    """banded planted factors: thousands of narrow levels (SURVEY 8d stress point) -- one long one-XCD run,
    and more relaxation launches than the device-side level analysis allows itself (host scan instead)"""
    for k, v in SWEEP_MODES[mode].items():
        monkeypatch.setenv(k, v)
    m, n = 6000, 12500
    B, st, colscale = basis_problem(m, n, seed=47, band=12)
    A, L, U = B["A"], B["L"], B["U"]
    ctx = kkt.KktContext(A)
    ctx.split_prepare(L, U, B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
    lv = ctx.split_levels()
    assert min(lv) > 600, lv                                   # deeper than kTailLevelsLds
    S = oracle.split_prepare(ocsc(po, A.with_identity()), n, ocsc(po, L), ocsc(po, U), B["rowperm"], B["colperm"],
                             B["basis"], B["status"], colscale)
    Us = po.Csc(m, m, U.p, U.i, S.get()["Ux"])
    rhs = np.random.default_rng(4).standard_normal(m)
    assert np.array_equal(ctx.forward_solve(rhs), oracle.forward_solve(ocsc(po, L), Us, rhs))
    assert np.array_equal(ctx.backward_solve(rhs), oracle.backward_solve(ocsc(po, L), Us, rhs))
    l1, d1 = ctx.split_apply(rhs)
    l2, d2 = S.apply(rhs)
    assert relerr(l1, l2) <= 1e-10
    ctx.close()


def test_fused_layout_random_shapes(kkt, po, oracle, monkeypatch):
    """the fused-tile layout forced onto many small random shapes (ragged last tiles, empty rows and
    columns, rows of up to 200 entries, single rows/columns): bit-identical to the oracle"""
    import scipy.sparse as sp
    from ipx_amd.synth import CscMatrix
    monkeypatch.setenv("IPXK_SPMV_LAYOUT", "fused")
    rng = np.random.default_rng(2024)
    shapes = [(1, 1, 1.0), (1, 50, 0.5), (50, 1, 0.5), (255, 257, 0.02), (256, 1024, 0.01), (1025, 300, 0.03),
              (2049, 4100, 0.002), (300, 40, 0.6), (40, 300, 0.6), (5000, 9000, 0.001), (777, 778, 0.25)]
    for (m, n, dens) in shapes:
        M = sp.random(m, n, density=dens, random_state=int(rng.integers(1 << 30)), format="csc")
        M.sort_indices()
        A = CscMatrix(m, n, M.indptr, M.indices, M.data)
        ctx = kkt.KktContext(A)
        W = 10.0 ** rng.uniform(-1, 1, n + m)
        rhs = rng.standard_normal(m)
        ctx.normal_prepare(W)
        l1, d1 = ctx.normal_apply(rhs)
        l2, d2 = oracle.normal_apply(ocsc(po, A), W, rhs)
        assert np.array_equal(l1, l2), (m, n)
        assert abs(d1 - d2) <= 1e-12 * max(abs(d2), 1e-300), (m, n)
        assert ctx.diag_factorize(W, False) == 0
        P, err = oracle.diag_factorize(ocsc(po, A), W, 10 ** 9, False)
        assert np.array_equal(ctx.diag_get()[0], P.get()[0]), (m, n)
        ctx.close()


@pytest.mark.parametrize("layout", ["phased", "fused", "sliced", "auto"])
def test_long_rows_in_every_layout(kkt, po, oracle, monkeypatch, layout):
    """a few columns AND rows of ~5k entries (dense columns, src/diagonal_precond.cc:48-101) next to short ones:
    the long rows go to the long-row kernels, the rest of the matrix keeps the chosen layout"""
    import scipy.sparse as sp
    from ipx_amd.synth import CscMatrix
    if layout != "auto":
        monkeypatch.setenv("IPXK_SPMV_LAYOUT", layout)
    if layout == "sliced":
        monkeypatch.setenv("IPXK_SLICE_TEST_KB", "16")
    m, n = 20000, 41000
    rng = np.random.default_rng(31)
    base = sp.random(m, n, density=8.0 / m, random_state=5, format="lil")
    for j in (3, 17000, n - 1):                                     # dense columns (long rows of A')
        r = rng.choice(m, 5000, replace=False)
        base[r, j] = rng.uniform(0.5, 2.0, r.size)
    for i in (0, 9999):                                             # dense rows (long rows of A)
        c = rng.choice(n, 5000, replace=False)
        base[i, c] = rng.uniform(0.5, 2.0, c.size)
    M = base.tocsc(); M.sort_indices()
    A = CscMatrix(m, n, M.indptr, M.indices, M.data)
    ctx = kkt.KktContext(A)
    lay, _ = ctx.spmv_layout()
    if layout != "auto":
        assert lay == (layout, layout), lay
    W = 10.0 ** rng.uniform(-1, 1, n + m)
    rhs = rng.standard_normal(m)
    ctx.normal_prepare(W)
    l1, d1 = ctx.normal_apply(rhs)
    l2, d2 = oracle.normal_apply(ocsc(po, A), W, rhs)
    assert relerr(l1, l2) <= 1e-12 and abs(d1 - d2) <= 1e-12 * abs(d2)
    assert ctx.diag_factorize(W, False) == 0
    P, err = oracle.diag_factorize(ocsc(po, A), W, 10 ** 9, False)
    assert relerr(ctx.diag_get()[0], P.get()[0]) <= 1e-12
    ctx.close()


def test_sliced_layout_random_shapes(kkt, po, oracle, monkeypatch):
    """the XCD-sliced layout on small ragged shapes (slice size shrunk to 1 KB of x so that they are
    eligible): 2, 4 and 8 slices, empty rows / columns / tiles; 1e-13 of the oracle (sums are
    associated per slice)"""
    import scipy.sparse as sp
    from ipx_amd.synth import CscMatrix
    monkeypatch.setenv("IPXK_SPMV_LAYOUT", "sliced")
    monkeypatch.setenv("IPXK_SLICE_TEST_KB", "1")
    rng = np.random.default_rng(77)
    for (m, n, dens) in [(300, 300, 0.05), (257, 513, 0.02), (1025, 1500, 0.01), (2049, 4100, 0.002),
                         (600, 700, 0.3), (5000, 9000, 0.001), (3, 2000, 0.05)]:
        M = sp.random(m, n, density=dens, random_state=int(rng.integers(1 << 30)), format="csc")
        M.sort_indices()
        A = CscMatrix(m, n, M.indptr, M.indices, M.data)
        ctx = kkt.KktContext(A)
        lay, _ = ctx.spmv_layout()
        assert "sliced" in lay, (m, n, lay)                   # at least one of the two products is sliced
        W = 10.0 ** rng.uniform(-1, 1, n + m)
        rhs = rng.standard_normal(m)
        ctx.normal_prepare(W)
        l1, d1 = ctx.normal_apply(rhs)
        l2, d2 = oracle.normal_apply(ocsc(po, A), W, rhs)
        assert relerr(l1, l2) <= 1e-13 and abs(d1 - d2) <= 1e-12 * max(abs(d2), 1e-300), (m, n)
        ctx.close()


# --------------------------------------------------------------------------------------
# the collective code path (RCCL), exercised with a one-rank communicator: IPXK_FORCE_COMM
# routes a single rank through finalize + all-gather + all-reduce exactly as N ranks would run
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("columns", [False, True])
def test_partitioned_code_path_single_rank(kkt, po, oracle, monkeypatch, columns):
    from ipx_amd import partition
    monkeypatch.setenv("IPXK_FORCE_COMM", "1")
    m, n = 2000, 4300
    A, st = diag_problem(m, n, seed=55)
    slab = partition.col_slab(A, st, 0, 1) if columns else partition.row_slab(A, st, 0, 1)
    ctx = kkt.KktContext(slab.A)
    ctx.comm_init(ctx.comm_unique_id(), 0, 1, columns=columns)
    assert ctx.kkt_diag_factorize(slab.xl, slab.xu, slab.zl, slab.zu, st["mu"], precond_dense_cols=False) == 0
    tol = 0.3 * np.sqrt(st["mu"])
    x1, y1, it1, e1, _ = ctx.kkt_diag_solve(slab.a, slab.b, tol, 500)
    ko = oracle.kkt_diag(ocsc(po, A), maxiter=500)
    ko.factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"])
    x2, y2, it2, e2, _ = ko.solve(st["a"], st["b"], tol)
    assert e1 == e2 == 0 and iters_close(it1, it2)
    assert relerr(y1, y2) < 1e-6 and relerr(x1, x2) < 1e-5
    rhs = np.random.default_rng(6).standard_normal(m)
    l1, d1 = ctx.normal_apply(rhs)
    l2, d2 = oracle.normal_apply(ocsc(po, A), ko.get()[0], rhs)
    assert relerr(l1, l2) <= 1e-12 and abs(d1 - d2) <= 1e-12 * abs(d2)
    # interrupt flags are agreed on across ranks (Control::InterruptCheck, conjugate_residuals.cc:209)
    calls = []
    x3, y3, it3, e3, _ = ctx.kkt_diag_solve(slab.a, slab.b, tol, 500, interrupt=lambda: calls.append(0) or 0)
    assert e3 == 0 and it3 == it1 and len(calls) >= 1
    x4, y4, it4, e4, _ = ctx.kkt_diag_solve(slab.a, slab.b, tol, 500,
                                            interrupt=lambda: calls.append(1) or (999 if len(calls) > 3 else 0))
    assert e4 == 999 and it4 < it1
    ctx.close()


def test_dense_column_stress_full_size(kkt):
    """BASELINE config 5: m=200k, n=400k, 32 dense columns (~79k entries each) -- the
    Sherman-Morrison-Woodbury preconditioner path (src/diagonal_precond.cc:48-101,133-149)."""
    m, n = 200000, 400000
    A, st = diag_problem(m, n, seed=12345, num_dense=32)
    ctx = kkt.KktContext(A)
    assert ctx.num_dense_cols == 32
    assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    W, _ = ctx.kkt_diag_get()
    # P is the inverse of E + Ad Wd Ad' (form (2) of src/diagonal_precond.h:12-23): check P*(M v) == v
    S = A.to_scipy()
    dense = np.arange(32)
    sparse_part = S[:, 32:]
    E = W[n:] + (sparse_part.multiply(sparse_part)) @ W[32:n]
    Ad = S[:, :32]
    v = np.random.default_rng(0).standard_normal(m)
    Mv = E * v + Ad @ (W[dense] * (Ad.T @ v))
    Pv, dot = ctx.diag_apply(Mv)
    assert relerr(Pv, v) < 1e-9 and abs(dot - Mv @ v) <= 1e-9 * abs(dot)
    tol = 0.3 * np.sqrt(st["mu"])
    x, y, it, e, _ = ctx.kkt_diag_solve(st["a"], st["b"], tol, 500)
    assert e == 0 and it < 150
    res1, res2 = kkt_residual_diag(A, W, st["a"], st["b"], x, y)
    assert np.abs(res2).max() < 1e-9 * (1 + np.abs(x).max())
    assert np.abs(np.sqrt(W[n:]) * res1[n:]).max() <= tol * (1 + 1e-9)
    # without the dense-column treatment the diag-PCR hits its cap: the case the SMW form exists for
    assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"], precond_dense_cols=False) == 0
    _, _, it2, e2, _ = ctx.kkt_diag_solve(st["a"], st["b"], tol, 300)
    assert (it2, e2) == (300, 201)
    ctx.close()


def test_basis_path_full_size_properties(kkt, monkeypatch):
    """BASELINE config 3: m=1M, n=2M, basis-preconditioned CR on planted LU factors.  The oracle
    would need minutes here: check the KKT system the result must satisfy
    (src/kkt_solver_basis.cc:69-74, src/kkt_solver.h:21-27) and the triangular solves by residual."""
    m, n = 1000000, 2000000
    B, st, colscale = basis_problem(m, n, seed=12345)
    A = B["A"]
    ctx = kkt.KktContext(A)
    ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
    assert all(10 <= v <= 500 for v in ctx.split_levels())
    AI = A.with_identity().to_scipy()
    Bm = AI[:, B["basis"]]
    r = np.random.default_rng(1).standard_normal(m)
    assert relerr(Bm @ ctx.solve_dense(r, "N"), r) < 1e-9            # B x = r
    assert relerr(Bm.T @ ctx.solve_dense(r, "T"), r) < 1e-9          # B'x = r
    # C = I + inv(B~) N~ N~' inv(B~') is symmetric positive definite
    u, v = r, np.random.default_rng(2).standard_normal(m)
    Cu, uCu = ctx.split_apply(u)
    Cv, _ = ctx.split_apply(v)
    assert abs(v @ Cu - u @ Cv) <= 1e-10 * abs(v @ Cu) and uCu > u @ u * (1 - 1e-12)
    tol = 0.3 * np.sqrt(st["mu"])
    x, y, it, e, _ = ctx.kkt_basis_solve(st["a"], st["b"], tol, 500)
    assert e == 0 and it < 200
    assert relerr(AI @ x, st["b"]) < 1e-9                             # primal equation
    g = AI.T @ y
    res = x / colscale ** 2 + g - st["a"]                            # dual equation, barrier variables
    nb = B["status"] == -1
    assert np.abs(res[nb]).max() < 1e-9 * (1 + np.abs(st["a"]).max() + np.abs(g).max())   # exact on nonbasic
    assert np.abs(res[~nb] * colscale[~nb]).max() <= tol * (1 + 1e-6)                      # tol on basic
    # the inverted tails of the forward sweeps (Sweep::Block; on by default at this size) against the level-scheduled form
    xN1, xT1 = ctx.solve_dense(r, "N"), ctx.solve_dense(r, "T")
    fw1, bw1 = ctx.forward_solve(r), ctx.backward_solve(r)
    monkeypatch.setenv("IPXK_TAIL_INVERSE", "0")
    monkeypatch.setenv("IPXK_HEAD_INVERSE", "0")
    ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
    # the single-launch runs reproduce what one launch per level computes, bit for bit
    xN, xT = ctx.solve_dense(r, "N"), ctx.solve_dense(r, "T")
    fw, bw = ctx.forward_solve(r), ctx.backward_solve(r)
    for v1, v0 in ((xN1, xN), (fw1, fw), (xT1, xT), (bw1, bw)):
        assert relerr(v1, v0) <= 1e-12 and not np.array_equal(v1, v0)
    lv = ctx.split_levels()
    monkeypatch.setenv("IPXK_TRISOLVE", "levels")
    ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
    assert ctx.split_levels() == lv
    assert np.array_equal(ctx.solve_dense(r, "N"), xN) and np.array_equal(ctx.solve_dense(r, "T"), xT)
    assert np.array_equal(ctx.forward_solve(r), fw) and np.array_equal(ctx.backward_solve(r), bw)
    monkeypatch.delenv("IPXK_TRISOLVE")
    monkeypatch.delenv("IPXK_TAIL_INVERSE")
    monkeypatch.delenv("IPXK_HEAD_INVERSE")
    ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
    # same basis, new scaling factors: ipxk_split_rescale == a full Prepare (src/kkt_solver_basis.cc:59-64)
    cs2 = colscale * np.where(np.isfinite(colscale), 10.0 ** np.random.default_rng(5).uniform(-0.5, 0.5, colscale.size), 1.0)
    t0 = time.time()
    ctx.split_rescale(B["status"], cs2)
    t_rescale = time.time() - t0
    a1, d1 = ctx.split_apply(u)
    f1, b1 = ctx.forward_solve(r), ctx.backward_solve(r)
    t0 = time.time()
    ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], cs2)
    t_prepare = time.time() - t0
    a2, d2 = ctx.split_apply(u)
    assert np.array_equal(a1, a2) and d1 == d2
    assert np.array_equal(ctx.forward_solve(r), f1) and np.array_equal(ctx.backward_solve(r), b1)
    print("prepare %.1f ms, rescale %.1f ms" % (t_prepare * 1e3, t_rescale * 1e3))
    assert t_rescale < 0.5 * t_prepare
    ctx.close()


# --------------------------------------------------------------------------------------
# model upload on the device: exact arithmetic, bit-identical to the oracle
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,m,n", [(301, 150, 320), (302, 4000, 9100), (303, 20000, 7000)])
def test_equilibrate_and_transpose_on_device(kkt, po, oracle, seed, m, n):
    from ipx_amd import synth
    from test_oracle_vs_ref import badly_scaled_lp
    A = badly_scaled_lp(m, n, seed)
    Ao = ocsc(po, A)
    x1, cs1, rs1, r1 = kkt.equilibrate(A)
    x2, cs2, rs2, r2 = oracle.equilibrate(Ao)
    assert r1 == r2 >= 1
    assert np.array_equal(x1, x2) and np.array_equal(cs1, cs2) and np.array_equal(rs1, rs2)
    B = synth.synthetic_lp(m, n, 5, seed)                     # already in range: untouched
    x3, cs3, rs3, r3 = kkt.equilibrate(B)
    assert r3 == -1 and np.array_equal(x3, B.x) and np.all(cs3 == 1.0) and np.all(rs3 == 1.0)
    # Transpose: index arithmetic, bit-exact (ascending source column inside a row)
    p, i, x = kkt.transpose(A)
    T = oracle.transpose(Ao)
    assert np.array_equal(p, T.p) and np.array_equal(i, T.i) and np.array_equal(x, T.x)
    bad = synth.CscMatrix(m, n, A.p, np.where(np.arange(A.nnz) == 7, m + 3, A.i), A.x)
    with pytest.raises(kkt.KktError):
        kkt.transpose(bad)
    with pytest.raises(kkt.KktError):
        kkt.equilibrate(bad)


def test_sweep_edge_cases(kkt, po, oracle, monkeypatch):
    """degenerate factor shapes: a 1 x 1 system, L without entries and U diagonal only (every unknown in level 0),
    and a bidiagonal pair (a chain: as many levels as unknowns, one unknown each -- the pure hand-off chain)"""
    import scipy.sparse as sp
    from ipx_amd.synth import CscMatrix
    rng = np.random.default_rng(11)

    def check(Lm, Um, m):
        n = 2 * m + 3
        mk = lambda M: CscMatrix(m, m, M.indptr, M.indices, M.data)
        L, U = mk(sp.csc_matrix(Lm)), mk(sp.csc_matrix(Um))
        ctx = kkt.KktContext(synth_identity_model(m, n))
        ident = np.arange(m, dtype=np.int64)
        status = np.full(n + m, -1, dtype=np.int64); status[:m] = 0
        ctx.split_prepare(L, U, ident, ident, ident, status, np.ones(n + m))
        rhs = rng.standard_normal(m)
        assert np.array_equal(ctx.forward_solve(rhs), oracle.forward_solve(ocsc(po, L), ocsc(po, U), rhs))
        assert np.array_equal(ctx.backward_solve(rhs), oracle.backward_solve(ocsc(po, L), ocsc(po, U), rhs))
        lv = ctx.split_levels()
        ctx.close()
        return lv

    assert check(sp.csc_matrix((1, 1)), sp.csc_matrix([[2.5]]), 1) == [1, 1, 1, 1]
    m = 777
    assert check(sp.csc_matrix((m, m)), sp.diags(rng.uniform(0.5, 2.0, m)).tocsc(), m) == [1, 1, 1, 1]
    m = 3000
    Lc = sp.diags(rng.uniform(-0.9, 0.9, m - 1), -1, shape=(m, m)).tocsc()
    Uc = (sp.diags(rng.uniform(-0.9, 0.9, m - 1), 1, shape=(m, m)) + sp.diags(rng.uniform(1.0, 2.0, m))).tocsc()
    Uc.sort_indices()
    assert check(Lc, Uc, m) == [m, m, m, m]
