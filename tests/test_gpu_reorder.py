"""GPU: the locality-recovering renumbering of the model (ipx_amd/csrc/reorder.hip, reorder_model; SURVEY.md section 7
"row/column reordering ... must stay a pure permutation").  Index arithmetic bit-exact, solves equal to the unpermuted ones.

The numbering.  rowperm, colperm, the level count and the component count are held bit for bit to
tests/reorder_reference.py, a NumPy restatement whose levels tests/test_reorder_reference.py holds to
scipy.sparse.csgraph, on the matrices of tests/reorder_cases.py: a shuffled band whose second pass starts elsewhere; 70
components (64 are numbered, 421 rows and 821 columns stay without a level and come last by old index; row 0 is empty,
so the first search does not start there); 5 components and a few empty rows and columns, where the loop ends because
no row is left; a tree whose last row frontier and the column frontier before it hold 79 600 entries, more than the
65 536 threads of a level's launch; layered graphs of exactly 16, 17 and 32 row levels, i.e. one batch of kBfsBatch
levels, one level more, and two batches.  Every case is forced (IPXK_REORDER=1) and asserts active == 1: a failure inside
reorder_model is swallowed by build_model_resident and would otherwise leave a context without a renumbering.

The solve.  On the three band-like cases the diag path's solve on the renumbered copy is stopped after 1, 6 and 11 CR
iterations and compared with tests/cr_reference.py run in the numbering as given, at 1e-12 relative to the largest
entry (the operator-level parity gate, SURVEY section 8d, as tests/test_gpu_cr_exits.py): a row or column that received
another one's weight, preconditioner entry, residual scale or right-hand side is off by about its own size, and the
smallest |y_i| is 9.3e-8 of the largest.  The CPU oracle must itself be within 1e-13 of that reference.  The same gate
holds a second factorize with other weights, Factorize(nullptr) and a solve after one that the interrupt callback ended.

Measured on the CPU (oracle against the reference, the worst over maxiter 1, 6, 11): see tests/test_reorder_reference.py;
y within 2.9e-15, x within 1.8e-14 over all inputs.
Measured on an MI355X (device against the reference, the worst over maxiter 1, 6, 11):
  banded y 1.4e-15, x 4.8e-15; many components y 2.8e-16, x 5.2e-15; few components y 1.5e-16, x 4.6e-15;
  banded at maxiter 6 with the second weights y 8.1e-16, x 3.1e-15, with G = I y 5.2e-16, x 7.1e-15, after the
  interrupted solve y 7.3e-16, x 3.6e-15.  The converged run: 59 iterations on both sides, y within 2.8e-10 and x within
  5.2e-8 of the oracle's.  Every new test takes less than 0.3 s.
Deliberately wrong builds, each run once against these tests and not kept:
  1. level_keys_kernel keying rows and columns by old index alone: all seven numbering tests fail (and the row-span
     assertion of the first test of this file); the solves still pass, the numbering then being the identity.
  2. reorder_permute_weights copying the slack half of W without permuting it: the nine stopped solves are off by 6e-4
     to 1.6 in y and 2e-3 to 3.0 in x, the converged run takes 51 iterations and is off by 1.4 in y, the second
     factorize and the solve after the interrupted one fail alike; the G = I test passes, all its weights being 1.
  The released build passes everything."""
import numpy as np
import pytest
import scipy.sparse as sp

import reorder_cases as cases
import reorder_reference
from cr_exits_worker import MAXITERS
from helpers import kkt_residual_diag, relerr
from ipx_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kkt():
    from ipx_amd import kkt as k
    k.load_library()
    assert k.load_library().ipxk_device_count() > 0, "no GPU visible"
    return k


def solve_both(kkt, A, st, monkeypatch, force=True):
    out = {}
    for mode in ("0", "1" if force else None):
        if mode is None:
            monkeypatch.delenv("IPXK_REORDER", raising=False)
        else:
            monkeypatch.setenv("IPXK_REORDER", mode)
        ctx = kkt.KktContext(A)
        info = ctx.reorder_info()
        assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
        x, y, it, err, _ = ctx.kkt_diag_solve(st["a"], st["b"], 0.3 * np.sqrt(st["mu"]) * 1e-4, 500)
        perms = ctx.reordering() if info["levels"] > 0 and (info["active"] or mode == "1") else None
        ctx.close()
        out[mode] = (x, y, it, err, info, perms)
    return out


def test_renumbering_is_a_pure_permutation_and_the_solve_is_the_same(kkt, monkeypatch):
    """a banded LP with rows and columns shuffled, forced through the renumbered copy (IPXK_REORDER=1): rowperm / colperm are
    permutations, the renumbered matrix has its entries back within a few thousand rows of each other (the band is found), and
    the KKT solve returns the same x, y (1e-8 / 1e-6) in the same number of CR iterations (+-2) as on the model as given"""
    m, n = 20000, 41000
    A0 = synth.banded_lp(m, n, 8, 512, 5)
    A, _, _ = synth.shuffled(A0, 6)
    st = synth.synthetic_ipm_state(m, n, 1.0, 5)
    out = solve_both(kkt, A, st, monkeypatch)
    x0, y0, it0, e0, i0, _ = out["0"]
    x1, y1, it1, e1, i1, perms = out["1"]
    assert i0["active"] == 0 and i1["active"] == 1 and i1["levels"] > 8
    rp, cp = perms
    assert np.array_equal(np.sort(rp), np.arange(m)) and np.array_equal(np.sort(cp), np.arange(n))
    M = sp.csc_matrix((A.x, A.i, A.p), shape=(m, n))[rp][:, cp].tocsc()
    M.sort_indices()
    span = np.array([M.indices[M.indptr[j]:M.indptr[j + 1]].max() - M.indices[M.indptr[j]:M.indptr[j + 1]].min() for j in range(0, n, 97)])
    span_given = np.array([A.i[A.p[j]:A.p[j + 1]].max() - A.i[A.p[j]:A.p[j + 1]].min() for j in range(0, n, 97)])
    print("row span of a column: as given median %d, renumbered median %d (band of the unshuffled matrix: 512)" % (np.median(span_given), np.median(span)))
    assert np.median(span) < 4096 < np.median(span_given)
    assert e0 == e1 == 0 and abs(it0 - it1) <= 2, (it0, it1)
    assert relerr(y1, y0) < 1e-8 and relerr(x1, x0) < 1e-6        # (two solves stopped at the same tolerance, row sums in different orders)


def test_expander_is_left_alone(kkt, monkeypatch):
    """the uniformly random LP has nothing to recover: recognised within 8 levels, no copy, no change"""
    monkeypatch.delenv("IPXK_REORDER", raising=False)
    m, n = 150000, 300000                        # nnz 2.4 M: above the size from which a renumbering is looked for
    A = synth.synthetic_lp(m, n, 8, 7)
    ctx = kkt.KktContext(A)
    info = ctx.reorder_info()
    ctx.close()
    print(info)
    assert info["active"] == 0 and 0 < info["levels"] <= 12 and info["ms"] < 100
    # the count is that of the first pass of the restatement, which takes the same way out
    R = reorder_reference.reorder(m, n, A.p, A.i, force=False)
    assert R.rowperm is None and info["levels"] == R.levels == len(R.frontiers[0]) and info["components"] == 0


def test_renumbering_chosen_by_timing_at_scale(kkt, monkeypatch):
    """1M x 2M banded LP, shuffled: the renumbering is found, the renumbered copy's two products are faster than those on the model
    as given, so it is in use without being forced -- and the solve agrees with the one on the model as given"""
    m, n = 1000000, 2000000
    A0 = synth.banded_lp(m, n, 8, 4096, 12345)
    A, _, _ = synth.shuffled(A0, 7)
    st = synth.synthetic_ipm_state(m, n, 1.0, 12345)
    out = solve_both(kkt, A, st, monkeypatch, force=False)
    x0, y0, it0, e0, i0, _ = out["0"]
    x1, y1, it1, e1, i1, _ = out[None]
    print(i1)
    assert i1["active"] == 1 and i1["us_reordered"] < 0.9 * i1["us_original"] and i1["ms"] < 500
    assert e0 == e1 == 0 and abs(it0 - it1) <= 2
    assert relerr(y1, y0) < 1e-6 and relerr(x1, x0) < 1e-5


# ---- the numbering against its restatement ----
def forced_context(kkt, monkeypatch, A):
    monkeypatch.setenv("IPXK_REORDER", "1")
    monkeypatch.delenv("IPXK_SPMV_LAYOUT", raising=False)       # a layout that a copy cannot be built in drops the numbering
    ctx = kkt.KktContext(A)
    info = ctx.reorder_info()
    assert ctx.num_dense_cols == 0 and info["active"] == 1, info
    return ctx, info


@pytest.mark.parametrize("name", cases.NAMES)
def test_numbering_equals_restatement(kkt, monkeypatch, name):
    A, R = cases.matrix(name), cases.numbering(name)
    assert A.nnz >= cases.MIN_NNZ
    ctx, info = forced_context(kkt, monkeypatch, A)
    rp, cp = ctx.reordering()
    ctx.close()
    print(name, info, "restatement: %d levels, %d components, %d rows and %d columns without a level"
          % (R.levels, R.components, R.unreached_rows, R.unreached_cols))
    assert info["levels"] == R.levels and info["components"] == R.components
    assert np.array_equal(rp, R.rowperm) and np.array_equal(cp, R.colperm)


def test_no_renumbering_no_permutation(kkt, monkeypatch):
    monkeypatch.setenv("IPXK_REORDER", "0")
    ctx = kkt.KktContext(cases.matrix("banded"))
    info = ctx.reorder_info()
    assert (info["active"], info["levels"], info["components"]) == (0, 0, 0)
    with pytest.raises(kkt.KktError):
        ctx.reordering()
    ctx.close()


# ---- the solve on the renumbered copy against extended precision ----
def ocsc(A):
    from oracle import pyoracle as po
    return po.Csc(A.nrow, A.ncol, A.p, A.i, A.x)


def iters_close(a, b):
    return abs(a - b) <= max(2, int(0.02 * max(a, b)))


def factorize_as_oracle(ctx, oracle, name, variant, maxiter):
    """factorizes the context and an oracle solver of `maxiter` iterations: same W, same resscale, bit for bit"""
    fact, a, b = cases.solve_inputs(name, variant)
    assert ctx.kkt_diag_factorize(*fact) == 0
    ko = oracle.kkt_diag(ocsc(cases.matrix(name)), None, True, maxiter)
    assert ko.factorize(*fact) == 0
    W, resscale = ctx.kkt_diag_get()
    Wo, ro = ko.get()
    assert np.array_equal(W, Wo) and np.array_equal(resscale, ro)
    return ko, W, resscale, a, b


def check_solve(ctx, oracle, name, variant, maxiter):
    ko, W, resscale, a, b = factorize_as_oracle(ctx, oracle, name, variant, maxiter)
    ref = cases.reference(name, variant, maxiter, W, resscale)
    assert (ref.run.iter, ref.run.errflag) == (maxiter, 201)
    xo, yo, ito, erro, _ = ko.solve(a, b, 1e-30)
    x, y, it, err, _ = ctx.kkt_diag_solve(a, b, 1e-30, maxiter)
    print("%s %s maxiter %d: device y %.2e x %.2e; oracle y %.2e x %.2e; min|y|/max|y| %.2e"
          % (name, variant, maxiter, cases.dist(y, ref.y), cases.dist(x, ref.x), cases.dist(yo, ref.y), cases.dist(xo, ref.x),
             np.abs(y).min() / np.abs(y).max()))
    assert (ito, erro) == (maxiter, 201) and cases.dist(yo, ref.y) < 1e-13 and cases.dist(xo, ref.x) < 1e-13
    assert (it, err) == (maxiter, 201)
    assert cases.dist(y, ref.y) <= 1e-12 and cases.dist(x, ref.x) <= 1e-12


@pytest.mark.parametrize("maxiter", MAXITERS)
@pytest.mark.parametrize("name", cases.SOLVE_CASES)
def test_renumbered_solve_vs_extended_precision(kkt, oracle, monkeypatch, name, maxiter):
    ctx, _ = forced_context(kkt, monkeypatch, cases.matrix(name))
    check_solve(ctx, oracle, name, "first", maxiter)
    ctx.close()


def test_renumbered_solve_converged_vs_oracle(kkt, oracle, monkeypatch):
    """the assertions of test_diag_path_vs_oracle (tests/test_gpu_parity.py) on the forced banded case; the residual of
    the slack rows, scaled by sqrt(W), is what a mispermuted resscale would push over the tolerance"""
    A = cases.matrix("banded")
    n = A.ncol
    ctx, _ = forced_context(kkt, monkeypatch, A)
    ko, W, _, a, b = factorize_as_oracle(ctx, oracle, "banded", "first", 500)
    tol = 0.3 * np.sqrt(cases.solve_inputs("banded")[0][4])
    x1, y1, it1, e1, _ = ctx.kkt_diag_solve(a, b, tol, 500)
    x2, y2, it2, e2, _ = ko.solve(a, b, tol)
    ctx.close()
    print("converged: device %d iterations, oracle %d; y %.2e x %.2e" % (it1, it2, relerr(y1, y2), relerr(x1, x2)))
    assert e1 == e2 == 0 and iters_close(it1, it2)
    assert relerr(y1, y2) < 1e-6 and relerr(x1, x2) < 1e-5
    res1, res2 = kkt_residual_diag(A, W, a, b, x1, y1)
    assert np.abs(res2).max() < 1e-9 * max(1.0, np.abs(b).max() + np.abs(x1).max())
    assert np.abs(res1[:n]).max() < 1e-9 * max(1.0, np.abs(x1 / W).max())
    assert np.abs(np.sqrt(W[n:]) * res1[n:]).max() <= tol * (1 + 1e-9)


# ---- state of the renumbered copy that must not go stale ----
def test_second_factorize_refreshes_the_permuted_weights(kkt, oracle, monkeypatch):
    ctx, _ = forced_context(kkt, monkeypatch, cases.matrix("banded"))
    check_solve(ctx, oracle, "banded", "first", 6)
    check_solve(ctx, oracle, "banded", "second", 6)
    ctx.close()


def test_factorize_nullptr_on_a_renumbered_context(kkt, oracle, monkeypatch):
    """Factorize(nullptr), G = I, after a factorize with weights: the copy's weights, diagonal and scaling follow"""
    ctx, _ = forced_context(kkt, monkeypatch, cases.matrix("banded"))
    assert ctx.kkt_diag_factorize(*cases.solve_inputs("banded", "first")[0]) == 0
    check_solve(ctx, oracle, "banded", "identity", 6)
    ctx.close()


def test_interrupted_solve_leaves_the_copy_out_of_use(kkt, oracle, monkeypatch):
    """a solve that the interrupt callback ends (errflag 999) leaves Reordered::in_use cleared: the operator and the
    preconditioner applied from outside the loop are those of the model as given, bit for bit what a context without a
    renumbering returns, and the next solve is right"""
    A = cases.matrix("banded")
    fact, a, b = cases.solve_inputs("banded", "first")
    rhs = np.random.default_rng(5).standard_normal(A.nrow)
    monkeypatch.setenv("IPXK_REORDER", "0")
    plain = kkt.KktContext(A)
    assert plain.reorder_info()["active"] == 0 and plain.kkt_diag_factorize(*fact) == 0
    want = plain.normal_apply(rhs), plain.diag_apply(rhs)
    plain.close()
    ctx, _ = forced_context(kkt, monkeypatch, A)
    assert ctx.kkt_diag_factorize(*fact) == 0
    _, _, it, err, _ = ctx.kkt_diag_solve(a, b, 1e-300, 100000, interrupt=lambda: 999)
    assert err == 999 and it < 100000
    got = ctx.normal_apply(rhs), ctx.diag_apply(rhs)
    for (lhs, dot), (lhs0, dot0) in zip(got, want):
        assert np.array_equal(lhs, lhs0) and dot == dot0
    check_solve(ctx, oracle, "banded", "first", 6)
    ctx.close()
