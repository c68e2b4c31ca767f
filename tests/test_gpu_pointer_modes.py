"""GPU: the two pointer modes of the C boundary give the same bits.

A call with host pointers stages every vector argument in a device copy and copies the outputs back; a call with device
pointers hands the caller's memory through.  Both then run the identical device path, so for each entry point below the
host form, the resident form and the host form again -- on ONE context, so that whatever a call leaves behind in the
context's staging meets the next call -- must agree bit for bit: np.array_equal on every output vector, equality of the
iteration counts, error flags and step info.  No tolerance is involved.  (ipxk_pcr_solve is not here: its host form skips
one operator application when lhs is zero, so its two forms run different arithmetic.)

m = 257, n = 600: m != n + m and neither is a multiple of the 256-thread block, so a length m taken for n + m (or the
reverse) changes what is copied.  Nothing else in the staging depends on the size below the 8 MB pinned chunk.

Every host output array and every device output vector is filled with NaN before the call: an output that is never
written, or never copied back, compares unequal to anything."""
import ctypes as C

import numpy as np
import pytest

from helpers import diag_problem
from ipx_amd import synth

pytestmark = pytest.mark.gpu
M, NS = 257, 600
N = NS + M
STEP_KEYS = ("dx", "dxl", "dxu", "dy", "dzl", "dzu")
IT_KEYS = ("x", "xl", "xu", "y", "zl", "zu")
NEWTON_IN = ("rb", "rc", "rl", "ru", "sl", "su", "xl", "xu", "zl", "zu")


@pytest.fixture(scope="module")
def kkt():
    from ipx_amd import kkt as k
    k.load_library()
    return k


@pytest.fixture(scope="module")
def problem(kkt):
    A, st = diag_problem(M, NS)
    ctx = kkt.KktContext(A)
    yield ctx, st
    ctx.close()


def nans(length):
    return np.full(length, np.nan)


def fp(kkt, a):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(kkt.P_f64)


def three_runs(host_form, resident_form):
    """host, resident, host again (a resident form switches to device pointers for its one call only)"""
    return [host_form(), resident_form(), host_form()]


def assert_same(runs, vector_keys, scalar_keys):
    first = runs[0]
    for key in vector_keys:
        assert np.isfinite(first[key]).any(), key
        assert not np.isnan(first[key]).any(), key
    for which, other in zip(("resident", "host again"), runs[1:]):
        for key in vector_keys:
            assert np.array_equal(first[key], other[key]), (which, key)
        for key in scalar_keys:
            assert first[key] == other[key], (which, key, first[key], other[key])


def test_kkt_diag_solve(kkt, problem):
    ctx, st = problem
    assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    tol, maxiter = 0.3 * np.sqrt(st["mu"]), 500
    null_cb = C.cast(None, kkt.INTERRUPT_FN)

    def host_form():
        # KktContext.kkt_diag_solve with NaN in the outputs
        a, b = (np.ascontiguousarray(st[k], dtype=np.float64) for k in ("a", "b"))
        x, y = nans(N), nans(M)
        it, err, times = C.c_int64(0), C.c_int64(0), kkt.Times()
        ctx._check(ctx.lib.ipxk_kkt_diag_solve(ctx.h, fp(kkt, a), fp(kkt, b), C.c_double(tol), C.c_int64(maxiter), fp(kkt, x),
                                               fp(kkt, y), C.byref(it), C.byref(err), null_cb, None, C.byref(times)))
        return dict(x=x, y=y, iter=int(it.value), errflag=int(err.value))

    def resident_form():
        vec = [ctx.vector(N, st["a"]), ctx.vector(M, st["b"]), ctx.vector(N, nans(N)), ctx.vector(M, nans(M))]
        ctx.set_pointer_mode(True)
        it, err, _ = ctx.kkt_diag_solve_resident(*vec, tol, maxiter)
        ctx.set_pointer_mode(False)
        out = dict(x=vec[2].download(), y=vec[3].download(), iter=it, errflag=err)
        for v in vec:
            v.free()
        return out

    runs = three_runs(host_form, resident_form)
    print("kkt_diag_solve: %d CR iterations" % runs[0]["iter"])
    assert runs[0]["errflag"] == 0 and runs[0]["iter"] > 0
    assert_same(runs, ("x", "y"), ("iter", "errflag"))


def newton_state():
    """synth.synthetic_newton_state with a few free, fixed and boxed variables.  Its fixed variables carry xl = xu = 0, for
    which KKTSolverDiag::Factorize forms 0/0; the diag path takes a fixed variable as the other tests set it (xl = xu = inf,
    zl = zu = 0: weight 1/regval), so the vectors stay free of NaN and np.array_equal means what it says."""
    st = synth.synthetic_newton_state(M, NS, 5, num_free=4, num_fixed=3, num_boxed=6)
    fixed = st["state"] == 0
    assert fixed.sum() == 3 and (st["state"] == 1).sum() == 4 and (st["state"] == 4).sum() == 6
    st["xl"][fixed] = st["xu"][fixed] = np.inf
    return st


def test_newton_solve(kkt, problem):
    ctx, _ = problem
    st = newton_state()
    assert ctx.kkt_diag_factorize(st["xl"], st["xu"], st["zl"], st["zu"], st["mu"]) == 0
    tol, maxiter = 0.3 * np.sqrt(st["mu"]), 500
    null_cb = C.cast(None, kkt.INTERRUPT_FN)
    lengths = [M if key == "dy" else N for key in STEP_KEYS]

    def host_form():
        # KktContext.newton_solve with NaN in the outputs
        ins = [np.ascontiguousarray(st[key], dtype=np.float64) for key in NEWTON_IN]
        state = np.ascontiguousarray(st["state"], dtype=np.uint8)
        outs = [nans(length) for length in lengths]
        it, err, times = C.c_int64(0), C.c_int64(0), kkt.Times()
        ctx._check(ctx.lib.ipxk_newton_solve(ctx.h, C.c_int(0), *[fp(kkt, v) for v in ins],
                                             state.ctypes.data_as(C.POINTER(C.c_ubyte)), C.c_double(tol), C.c_int64(maxiter),
                                             *[fp(kkt, v) for v in outs], C.byref(it), C.byref(err), null_cb, None,
                                             C.byref(times)))
        return dict(zip(STEP_KEYS, outs), iter=int(it.value), errflag=int(err.value))

    def resident_form():
        dev_in = [ctx.vector(M if key == "rb" else N, st[key]) for key in NEWTON_IN]
        state = ctx.state_vector(st["state"])
        dev_out = [ctx.vector(length, nans(length)) for length in lengths]
        ctx.set_pointer_mode(True)
        it, err, _ = ctx.newton_solve_resident(False, dev_in, state, tol, maxiter, dev_out)
        ctx.set_pointer_mode(False)
        out = dict(zip(STEP_KEYS, (v.download() for v in dev_out)), iter=it, errflag=err)
        for v in dev_in + [state] + dev_out:
            v.free()
        return out

    runs = three_runs(host_form, resident_form)
    print("newton_solve: %d CR iterations" % runs[0]["iter"])
    assert runs[0]["errflag"] == 0 and runs[0]["iter"] > 0
    assert_same(runs, STEP_KEYS, ("iter", "errflag"))


def test_ipm_step(kkt, problem):
    ctx, _ = problem
    P = synth.synthetic_iterate(M, NS, 1)                 # (seed 1: the matrix of the context)
    b, c = P["rhs"], np.concatenate([P["obj"], np.zeros(M)])
    info_keys = [name for name, _ in kkt.IpmStepInfo._fields_]

    def after(info):
        # KktContext.iterate_get with NaN in the outputs
        out = {key: nans(M if key == "y" else N) for key in IT_KEYS}
        ctx._check(ctx.lib.ipxk_iterate_get(ctx.h, *[fp(kkt, out[key]) for key in IT_KEYS]))
        return dict(out, **info)

    def before():
        ctx.iterate_set(P["it"], P["state"])
        assert ctx.iterate_factorize_diag() == 0

    def host_form():
        before()
        return after(ctx.ipm_step(False, b, c, P["lbs"], P["ubs"], maxiter=2000))

    def resident_form():
        before()
        vec = [ctx.vector(M, b), ctx.vector(N, c), ctx.vector(N, P["lbs"]), ctx.vector(N, P["ubs"])]
        ctx.set_pointer_mode(True)
        info = ctx.ipm_step_resident(False, *vec, maxiter=2000)
        ctx.set_pointer_mode(False)
        for v in vec:
            v.free()
        return after(info)

    runs = three_runs(host_form, resident_form)
    print("ipm_step: CR iterations %d + %d, steps %.6f %.6f" % (
        runs[0]["kktiter_predictor"], runs[0]["kktiter_corrector"], runs[0]["step_primal"], runs[0]["step_dual"]))
    assert runs[0]["errflag"] == 0 and runs[0]["kktiter_predictor"] > 0 and runs[0]["kktiter_corrector"] > 0
    assert any(not np.array_equal(runs[0][key], P["it"][key]) for key in IT_KEYS)        # the step moved the iterate
    assert_same(runs, IT_KEYS, info_keys)
