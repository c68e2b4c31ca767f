"""GPU: every SpMV epilogue that had no tight test, in every gather layout, against tests/epilogue_reference.py.

launch_spmv (ipx_amd/csrc/spmv_kernels.hpp) instantiates its kernels per epilogue functor and per layout; this file forces
each layout (IPXK_SPMV_LAYOUT, read per context), asserts through spmv_layout() that BOTH gather matrices took it, and
holds every entry of every output to the derived gate of the reference,

    |device - long double| <= (len_r + c_epi + 2) * 2^-53 * S_r,

and, where the layout keeps the storage order (phased, fused, sortedfused, accfused, plain), rows of at most 255 entries to
the sequential double value bit for bit (long rows are summed by segments and get the gate only).  `acc` must reproduce
`sliced` bit for bit: the rows are stored with ascending indices.

What runs per case (the reference's inputs are the call's own returned vectors, so the check sits at the kernel boundary):
  EpiIterRb, EpiIterRc        iterate_residuals, before and after iterate_postprocess (both branches of EpiIterRc)
  EpiIterRbPart               the same on a one-rank column partition (IPXK_FORCE_COMM)
  EpiObjFixed                 iterate_objectives with inputs that leave the dot alone in dobjective
  EpiDiagonal                 diag_factorize(W, False) + diag_get
  EpiRecoverX                 x[:n] of kkt_diag_solve from the returned y and kkt_diag_get's W
  EpiResidualRows             x[n:] of the same call from the returned x[:n]
  EpiKktRhs                   loosely: the solve is run to a relative 1e-12 and (A W A' + W_I) y must meet the long-double
                              right-hand side within 100 x that; this catches a wrong sign, a missing term or misplaced rows,
                              not ulps (v_rhs is internal)
  EpiNewtonShift              dzl[:n], dzu[:n] of newton_solve(False, ...) from the returned dy and the untouched side
  EpiBasisColumns             the NONBASIC structural entries of kkt_basis_solve's x from the returned y (planted basis,
                              helpers.basis_problem; EpiBasisRhs and EpiBasisResidual feed dense solves and are seen through
                              the call succeeding only)
  EpiStartZ                   test_gpu_starting_point.py's comparison with the oracle on its smallest model, its helpers and
                              tolerances, under every layout

Slices.  With IPXK_SLICE_TEST_KB=1 a slice holds 128 doubles.  layout_geometry.hpp's slices_of gives 2, 4 or 8 slices and
no other count (x of at most two slices' size is not sliced at all unless IPXK_SLICE_FORCE2 is set, which gives 2; more than
8 slices' worth still gets 8 wider ones), so the 300-, 700-, 1024- and 2100-entry vectors get 4, 8, 8 and 8 slices and the
256- and 512-entry ones, with IPXK_SLICE_FORCE2, 2 and 4: the counts 2, 4 and 8 all occur (SLICES below, asserted per case).
Three, or more than eight, cannot be produced through a context; the any-count form of the combine kernel (NS = 0) runs in
tests/test_gpu_combine_loads.py (IPXK_COMBINE_GENERIC, read once per process).

The accumulated tiles (`acc`, `accfused`) are not built for a matrix with long rows (layout_host.hip: build_acc, build_acc_fused
return at nlong > 0), so the long-row model runs under every other layout.

Worst error / gate per epilogue and layout, over all models, from the run on an MI355X (0 = equal to the long-double value
rounded; the ordered layouts are also bit-equal to the sequential value):

  output              default      phased       fused      sliced         acc sortedfused    accfused       plain
  rb                    0.265       0.265       0.265       0.265       0.265       0.119       0.119       0.265
  rc                    0.198       0.198       0.198       0.155       0.155       0.137       0.137       0.198
  rb post               0.265       0.265       0.265       0.265       0.265       0.119       0.119       0.265
  rc post               0.198       0.198       0.198       0.155       0.155       0.137       0.137       0.198
  diagonal              0.277       0.277       0.277       0.277       0.277       0.224       0.224       0.277
  x                     0.243       0.243       0.231       0.288       0.256       0.164       0.163       0.248
  x slack               0.190       0.190       0.290       0.169       0.169       0.119       0.108       0.211
  dzl                   0.225       0.225       0.234       0.232       0.232       0.181       0.242       0.222
  dzu                   0.260       0.260       0.214       0.195       0.195       0.151       0.193       0.235
  rb partitioned        0.265       0.265       0.265       0.265       0.265       0.119       0.119       0.265
  dobjective          0.00010     0.00010     0.00023     0.00006     0.00006     0.00001     0.00005     0.00010
  x nonbasic            0.167       0.167       0.167       0.185       0.185           -           -       0.167

(`acc` has no long-row model, `sortedfused` and `accfused` run on the banded model only, hence their smaller maxima; the
inputs of x, x slack, dzl and dzu are each call's own returned y or dy, which differ between layouts by the CR loop's
rounding.)  EpiKktRhs: 322 to 610 CR iterations, the scaled residual of the long-double system between 0.5 and 1.0 times
the tolerance in every case.  EpiStartZ: worst relative difference 3.8e-15 to 4.6e-15 against the gate 1e-8.  The table
documents the margin; it sets no gate.
"""
import numpy as np
import pytest

import epilogue_reference as er
from helpers import basis_problem

pytestmark = pytest.mark.gpu
LD = np.longdouble
ORDERED = ("phased", "fused", "sortedfused", "accfused", "plain")
SLICED = ("sliced", "acc")
# slices of (the vector Acols gathers: m entries, the vector Arows gathers: n entries)
SLICES = {"mixed": (4, 8), "square": (2, 4), "wide": (8, 8), "long": (4, 8)}
assert {s for pair in SLICES.values() for s in pair} == {2, 4, 8}
NLONG = {"long": (3, 1)}
GENERAL = [None, "phased", "fused", "sliced", "acc", "plain"]
CASES = ([(mdl, lay) for mdl in ("mixed", "square", "wide") for lay in GENERAL]
         + [("long", lay) for lay in GENERAL if lay != "acc"]
         + [("banded", "sortedfused"), ("banded", "accfused")])


@pytest.fixture(scope="module")
def kkt():
    from ipx_amd import kkt as k
    k.load_library()
    return k


@pytest.fixture(autouse=True)
def stop_after_a_device_fault(request):
    """a case that ends in a HIP error ends the file's run: nothing more is started on a device that has faulted"""
    yield
    rep = getattr(request.node, "rep_call", None)
    if rep is not None and rep.failed and any(s in str(rep.longrepr) for s in ("illegal memory access", "hipError", "HIP error")):
        pytest.exit("a HIP error in %s: not starting further cases" % request.node.nodeid, returncode=3)


_models, _runs, _start = {}, {}, {}


def model_of(name):
    if name not in _models:
        _models[name] = er.any_model(name)
    return _models[name]


def force_layout(mp, name, layout):
    for var in ("IPXK_SPMV_LAYOUT", "IPXK_SLICE_TEST_KB", "IPXK_SLICE_FORCE2", "IPXK_FORCE_COMM", "IPXK_COMM"):
        mp.delenv(var, raising=False)
    if layout:
        mp.setenv("IPXK_SPMV_LAYOUT", layout)
    if layout in SLICED:
        mp.setenv("IPXK_SLICE_TEST_KB", "1")
        if name == "square":
            mp.setenv("IPXK_SLICE_FORCE2", "1")               # 256 doubles: two slices' size, sliced only when forced


def check_layout(ctx, name, layout):
    used = ctx.spmv_layout()[0]
    assert used == ((layout or "phased"),) * 2, (name, layout, used)       # unset: small matrices take the phased layout
    infos = [ctx.layout_info(w)[0] for w in (0, 1)]
    assert tuple(i["nlong"] for i in infos) == NLONG.get(name, (0, 0))
    if layout in SLICED:
        key = {"sliced": "nslices", "acc": "acc_nslices"}[layout]
        assert tuple(i[key] for i in infos) == SLICES[name], (name, layout, [i[key] for i in infos])
    return used


def context(kkt, A, name, layout):
    ctx = kkt.KktContext(A)
    check_layout(ctx, name, layout)
    return ctx


def run_case(kkt, name, layout):
    """every operation of one (model, layout); returns {output name: (device array, reference Op)} and the dot pair"""
    key = (name, layout)
    if key in _runs:
        return _runs[key]
    M = model_of(name)
    A, b, c, lb, ub, it, st, n, m = (M[k] for k in ("A", "b", "c", "lb", "ub", "it", "state", "n", "m"))
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        force_layout(mp, name, layout)
        ctx = context(kkt, A, name, layout)
        # EpiObjFixed
        b0, lb0, ub0, it0 = er.objective_inputs(M)
        ctx.iterate_set(it0, st)
        dobj = ctx.iterate_objectives(b0, c, lb0, ub0)[1]
        dot = (-dobj, er.obj_fixed(A, it0["y"], it0["x"], st))
        # EpiIterRb, EpiIterRc
        ctx.iterate_set(it, st)
        r = ctx.iterate_residuals(b, c, lb, ub)
        out["rb"] = (r["rb"], er.iter_rb(A, b, it["x"]))
        out["rc"] = (r["rc"][:n], er.iter_rc(A, c, it["zl"], it["zu"], it["y"], st, False))
        fixed = st[:n] == er.FIXED
        assert fixed.any() and not r["rc"][:n][fixed].any()
        ctx.iterate_postprocess(c, lb, ub)
        post = ctx.iterate_get()
        r = ctx.iterate_residuals(b, c, lb, ub)
        out["rb post"] = (r["rb"], er.iter_rb(A, b, post["x"]))
        out["rc post"] = (r["rc"][:n], er.iter_rc(A, c, post["zl"], post["zu"], post["y"], st, True))
        # EpiDiagonal
        W0 = 10.0 ** np.random.default_rng(3).uniform(-2, 2, n + m)
        assert ctx.diag_factorize(W0, False) == 0
        out["diagonal"] = (ctx.diag_get()[0], er.diagonal(A, W0))
        # EpiKktRhs (loosely), EpiRecoverX, EpiResidualRows
        nw = er.newton_inputs(st, it, 5)
        assert ctx.kkt_diag_factorize(*er.barrier_weights(it, st), nw["mu"]) == 0
        W, resscale = ctx.kkt_diag_get()
        rng = np.random.default_rng(6)
        a, rhs_b = rng.uniform(-0.5, 0.5, n + m), rng.uniform(-0.5, 0.5, m)
        rhs = er.normal_matrix_residual(A, W, a, rhs_b, np.zeros(m))[0]
        tol = 1e-12 * float(np.abs(resscale * rhs.astype(np.float64)).max())
        x, y, iters, err, _ = ctx.kkt_diag_solve(a, rhs_b, tol, 5000)
        assert err == 0, (err, iters)
        rhs, prod = er.normal_matrix_residual(A, W, a, rhs_b, y)
        res = float(np.abs(resscale.astype(LD) * (rhs - prod)).max())
        print("%s %s: EpiKktRhs: %d CR iterations, scaled residual %.2e (tolerance %.2e)" % (name, layout, iters, res, tol))
        assert res <= 100.0 * tol
        out["x"] = (x[:n], er.recover_x(A, W, a, y))
        out["x slack"] = (x[n:], er.residual_rows(A, rhs_b, x[:n]))
        # EpiNewtonShift
        step = ctx.newton_solve(False, nw["rb"], nw["rc"], nw["rl"], nw["ru"], nw["sl"], nw["su"], it["xl"], it["xu"],
                                it["zl"], it["zu"], st, 1e-8 * float(np.abs(nw["rb"]).max()), 5000)
        assert step["errflag"] == 0
        lower, upper, lo, up = er.newton_shift(A, nw["rc"], step["dzl"], step["dzu"], it["xl"], it["xu"], it["zl"], it["zu"],
                                               st, step["dy"])
        assert lower.any() and upper.any() and not (lower & upper).any()
        out["dzl"] = (step["dzl"][:n], lo, lower)
        out["dzu"] = (step["dzu"][:n], up, upper)
        neither = ~(lower | upper)
        assert not step["dzl"][:n][neither & (st[:n] < er.LB)].any() and not step["dzu"][:n][neither & (st[:n] < er.LB)].any()
        ctx.close()
        # EpiIterRbPart: one rank through the column-partitioned path
        from ipx_amd import partition
        mp.setenv("IPXK_FORCE_COMM", "1")
        mp.setenv("IPXK_COMM", "direct")
        pc = context(kkt, partition.col_slab_matrix(A, 0, A.ncol), name, layout)
        pc.comm_init(pc.comm_unique_id(), 0, 1, columns=True)
        pc.iterate_set(it, st)
        out["rb partitioned"] = (pc.iterate_residuals(b, c, lb, ub)["rb"], out["rb"][1])
        pc.close()
    _runs[key] = (out, dot)
    return _runs[key]


def ratio(dev, op, mask=None):
    """worst error / gate over the entries the epilogue writes (mask; all of them without one); where the gate is 0 the
    value must be exact"""
    err = np.abs(np.asarray(dev, np.float64).astype(LD) - op.ld)
    gate = op.gate
    assert np.isfinite(dev).all()
    if mask is not None:
        err, gate = err[mask], gate[mask]
    exact_zero = gate == 0
    assert not err[exact_zero].any()
    q = np.where(exact_zero, LD(0), err / np.where(exact_zero, LD(1), gate))
    return float(q.max()) if q.size else 0.0


def hold(name, layout, what, entry, table):
    dev, op = entry[0], entry[1]
    mask = entry[2] if len(entry) > 2 else None
    worst = ratio(dev, op, mask)
    table[what] = worst
    print("%-8s %-12s %-15s worst error / gate %.3f" % (name, layout or "default", what, worst))
    assert worst <= 1.0, (name, layout, what, worst)
    if (layout or "phased") in ORDERED:
        short = op.len <= er.MAX_ROW_LEN
        if mask is not None:
            short = short & mask
        assert short.any() and np.array_equal(np.asarray(dev)[short], op.seq[short]), (name, layout, what)


@pytest.mark.parametrize("name,layout", CASES, ids=["%s-%s" % (a, b or "default") for a, b in CASES])
def test_epilogues(kkt, name, layout):
    out, (dot_dev, dot) = run_case(kkt, name, layout)
    table = {}
    for what, entry in out.items():
        hold(name, layout, what, entry, table)
    worst = float(abs(LD(dot_dev) - dot.ld) / dot.gate)
    print("%-8s %-12s %-15s worst error / gate %.5f (value %.6e)" % (name, layout or "default", "dobjective", worst, dot_dev))
    assert dot_dev != 0.0 and worst <= 1.0, (name, layout, "dobjective", worst)
    if layout == "acc":
        ref, (ref_dot, _) = run_case(kkt, name, "sliced")
        for what, entry in out.items():
            assert np.array_equal(entry[0], ref[what][0]), (name, layout, what)
        assert dot_dev == ref_dot


BASIS = {"mixed": (300, 700, 2), "square": (256, 512, 0), "wide": (1024, 2100, 3)}
BASIS_CASES = [(mdl, lay) for mdl in BASIS for lay in GENERAL]


def run_basis(kkt, name, layout):
    key = ("basis", name, layout)
    if key in _runs:
        return _runs[key]
    m, n, num_free = BASIS[name]
    B, st, colscale = basis_problem(m, n, seed=21, num_free=num_free, num_fixed=3)
    with pytest.MonkeyPatch.context() as mp:
        force_layout(mp, name, layout)
        ctx = context(kkt, B["A"], name, layout)
        ctx.split_prepare(B["L"], B["U"], B["rowperm"], B["colperm"], B["basis"], B["status"], colscale)
        x, y, iters, err, _ = ctx.kkt_basis_solve(st["a"], st["b"], 1e-8, 2000)
        ctx.close()
    assert err == 0
    scale2 = np.where(B["status"][:n] == -1, colscale[:n] * colscale[:n], 0.0)
    assert (scale2 != 0).any() and (scale2 == 0).sum() >= m
    nonbasic = B["status"][:n] < 0
    _runs[key] = (x, y, (x[:n], er.basis_columns(B["A"], scale2, st["a"], y), nonbasic))
    return _runs[key]


@pytest.mark.parametrize("name,layout", BASIS_CASES, ids=["%s-%s" % (a, b or "default") for a, b in BASIS_CASES])
def test_basis_epilogues(kkt, name, layout):
    x, y, entry = run_basis(kkt, name, layout)
    hold(name, layout, "x nonbasic", entry, {})
    if layout == "acc":
        xs, ys, _ = run_basis(kkt, name, "sliced")
        assert np.array_equal(x, xs) and np.array_equal(y, ys)


START_LAYOUTS = GENERAL


@pytest.mark.parametrize("layout", START_LAYOUTS, ids=[lay or "default" for lay in START_LAYOUTS])
def test_starting_point(kkt, oracle, layout):
    """EpiStartZ: zl = c - A'y of the second solve and the dot sum zl^2 that decides the 0.05 c correction"""
    import test_gpu_starting_point as sp
    A, b, c, lb, ub = sp.model("mixed")
    if "want" not in _start:
        _start["want"] = sp.oracle_start(oracle, A, b, c, lb, ub)
    want, err, kktiter, add_c = _start["want"]
    assert err == 0 and not add_c
    with pytest.MonkeyPatch.context() as mp:
        force_layout(mp, "mixed", layout)
        ctx = context(kkt, A, "mixed", layout)
        info = ctx.ipm_starting_point(b, c, lb, ub)
        got = ctx.iterate_get()
        ctx.close()
    worst = sp.compare(got, want, info, kktiter)
    print("starting point under %s: kktiter %d, worst relative difference %.2e" % (layout or "default", info["kktiter"], worst))
