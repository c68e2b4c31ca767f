"""Times the user-form basic postsolve and evaluation next to the interior pair on one lp and one iterate (DESIGN.md section 8,
"Basic solutions in user form"):  ipxk_lp_postsolve_basic + ipxk_lp_evaluate_basic  against  ipxk_lp_postsolve  and
ipxk_lp_evaluate.  The 1M x 2M matrix of bench.py, row types and bound kinds cycling; device-pointer mode, so that a call
moves no vector over PCIe (the status arrays of the basic postsolve are host memory by its interface: they are part of its
time).  Wall time of the blocking call, the calls alternating in one process, median of 5 after one warm-up of each.

    python scripts/gpu_lp_basic_bench.py [rows cols]
"""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ipx_amd import kkt, synth  # noqa: E402


def main():
    m, n = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (1000000, 2000000)
    rng = np.random.default_rng(1)
    A = synth.synthetic_lp(m, n, 8, 12345)
    ct = "".join("=<>"[i % 3] for i in range(3)) * (m // 3 + 1)
    kind = np.arange(n) % 5
    lb = np.where((kind == 1) | (kind == 4), -np.inf, 0.0)
    ub = np.where((kind == 0) | (kind == 4), np.inf, np.where(kind == 3, 0.0, 1.0))
    for dualize in (0, 1):
        lp = kkt.Lp(A, rng.normal(size=m), ct[:m], rng.normal(size=n), lb, ub, dualize=dualize)
        ctx, N, M = lp.context, lp.n + lp.m, lp.m
        S = lp.model()
        it = dict(x=rng.normal(size=N), y=rng.normal(size=M))
        for k, b, fill in (("xl", "lb", np.inf), ("xu", "ub", np.inf), ("zl", "lb", 0.0), ("zu", "ub", 0.0)):
            it[k] = np.where(np.isfinite(S[b]), rng.uniform(0.1, 2.0, N), fill)
        state = np.where(np.isfinite(S["lb"]), np.where(np.isfinite(S["ub"]), 4, 2), np.where(np.isfinite(S["ub"]), 3, 1)).astype(np.uint8)
        ctx.iterate_set(it, state)
        st = np.concatenate([rng.integers(-3, 1, lp.n), rng.integers(-2, 1, M)]).astype(np.int64)
        if dualize:                                   # a basic added column needs a nonbasic slack
            nb = lp.info["num_boxed"]
            boxed = np.nonzero(np.isfinite(lb) & np.isfinite(ub))[0]
            st[lp.n + boxed[st[lp.n - nb:lp.n] == 0]] = -1
        ctx.set_pointer_mode(True)
        dev = {k: ctx.vector(len(v), v) for k, v in (("xs", it["x"]), ("ys", it["y"]), ("zs", it["zl"] - it["zu"]))}
        out = {k: ctx.vector(lp.num_var if k in "xz" else lp.num_constr) for k in ("x", "slack", "y", "z")}
        seven = [ctx.vector(lp.num_constr if k in ("slack", "y") else lp.num_var) for k in lp.PT_KEYS]
        cb, vb = np.zeros(lp.num_constr, np.int64), np.zeros(lp.num_var, np.int64)
        ev, bev = kkt.LpEval(), kkt.LpBasicEval()
        L, h = lp.lib, lp.h

        def basic_postsolve():
            lp._check(L.ipxk_lp_postsolve_basic(h, dev["xs"].as_arg(), dev["ys"].as_arg(), dev["zs"].as_arg(), kkt._ip(st), out["x"].as_arg(),
                                                out["slack"].as_arg(), out["y"].as_arg(), out["z"].as_arg(), kkt._ip(cb), kkt._ip(vb)))

        def basic_evaluate():
            lp._check(L.ipxk_lp_evaluate_basic(h, out["x"].as_arg(), out["slack"].as_arg(), out["y"].as_arg(), out["z"].as_arg(), kkt._ip(vb),
                                               C.byref(bev)))

        def basic_postsolve_no_status_out():          # (the statuses still go up; cbasis and vbasis do not come down)
            lp._check(L.ipxk_lp_postsolve_basic(h, dev["xs"].as_arg(), dev["ys"].as_arg(), dev["zs"].as_arg(), kkt._ip(st), out["x"].as_arg(),
                                                out["slack"].as_arg(), out["y"].as_arg(), out["z"].as_arg(), None, None))

        calls = {"ipxk_lp_postsolve": lambda: lp._check(L.ipxk_lp_postsolve(h, *[v.as_arg() for v in seven])),
                 "ipxk_lp_evaluate": lambda: lp._check(L.ipxk_lp_evaluate(h, C.byref(ev))),
                 "ipxk_lp_postsolve_basic": basic_postsolve, "  without cbasis, vbasis": basic_postsolve_no_status_out,
                 "ipxk_lp_evaluate_basic": basic_evaluate}
        times = {k: [] for k in calls}
        for rep in range(6):
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                times[k].append((time.perf_counter() - t0) * 1e3)
        print("%d x %d, %s form: ms, median of 5 after one warm-up (range)" % (m, n, "dual" if dualize else "primal"))
        for k, t in times.items():
            t = t[1:]
            print("  %-26s %8.3f (%.3f - %.3f)" % (k, float(np.median(t)), min(t), max(t)))
        sys.stdout.flush()
        lp.close()


if __name__ == "__main__":
    main()
