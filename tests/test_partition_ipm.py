"""CPU, world_size 2 (gloo): the reductions of the device IPM on a column partition (ipx_amd/partition.py, col_slab),
the scheme the HIP library runs on column-partitioned contexts.  Each rank holds a slab of structural columns and all
m slack entries; y and b are replicated.  Each rank reduces its own entries, one all-gather carries the small row of
per-rank values, and every rank combines the table in rank order.  The slack terms and b'y enter on rank 0 only.
A step-to-boundary problem returns the GLOBAL blocking index (structural c0 + j, slack n + i) with the four values
StepSizes reads there; the lexicographic minimum of (alpha, index) over the ranks is the reference's first-index rule.
The oracle's unpartitioned iterate is the checker: max, min and indices exactly, sums to 1e-14."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, N, SEED = 300, 700, 23
DAMP = 1.0 - 2.220446049250313e-16


def _model():
    """synthetic_iterate (free, upper-bounded, boxed, lower-bounded) with fixed structural and slack variables"""
    from ipx_amd import synth
    P = synth.synthetic_iterate(M, N, SEED)
    state = P["state"].copy()
    rng = np.random.default_rng(SEED)
    fx = np.concatenate([rng.choice(N, 30, replace=False), N + rng.choice(M, 12, replace=False)])
    state[fx] = 0
    it = {k: v.copy() for k, v in P["it"].items()}
    for k in ("xl", "xu"):
        it[k][fx] = np.inf
    for k in ("zl", "zu"):
        it[k][fx] = 0.0
    return dict(A=P["A"], b=P["rhs"], c=np.concatenate([P["obj"], np.zeros(M)]), lb=P["lbs"], ub=P["ubs"], state=state,
                it=it, step=P["step"])


def _boundary(x, dx, alpha0=1.0):
    """StepToBoundary on one rank's entries: (alpha, first local index or -1)"""
    cand = np.where(x + alpha0 * dx < 0.0, -(x * DAMP) / np.where(dx != 0.0, dx, 1.0), np.inf)
    j = int(np.argmin(cand)) if cand.size else -1
    return (float(cand[j]), j) if j >= 0 and cand[j] < alpha0 else (alpha0, -1)


def ipm_scalars_cols(rank, world, gather, allsum, Ag, n, c0, b, c, lb, ub, state, it, step):
    """The partitioned reductions on this rank's share; returns the replicated scalars and this rank's vectors."""
    m, nl = Ag.shape
    lead = rank == 0
    x, xl, xu, y, zl, zu = (it[k] for k in ("x", "xl", "xu", "y", "zl", "zu"))
    hl, hu = (state == 2) | (state == 4), (state == 3) | (state == 4)
    fixed = state == 0
    # rb: this rank's share of b - A x (b on rank 0), summed over the ranks, then - x_slack
    rb = allsum((b if lead else 0.0) - Ag @ x[:nl]) - x[nl:]
    aty = np.concatenate([Ag.T @ y, y])
    rc = np.where(fixed, 0.0, ((c - zl) + zu) - aty)
    rl = np.where(hl, lb - x + xl, 0.0)
    ru = np.where(hu, ub - x - xu, 0.0)
    mine = slice(None) if lead else slice(0, nl)          # the slack entries are replicated: rank 0 counts them

    def rows(values):
        T = np.array(gather(np.array(values, dtype=np.float64)))   # world x k, rank order
        return T

    p = max(np.abs(rb).max(), np.abs(rl).max(), np.abs(ru).max())
    d = np.abs(rc).max()
    prod = np.concatenate([(xl * zl)[mine][hl[mine]], (xu * zu)[mine][hu[mine]]])
    comp = [prod.sum(), prod.min() if prod.size else np.inf, prod.max() if prod.size else 0.0, float(prod.size)]
    st, xm, cm = state[mine], x[mine], c[mine]
    pobj = np.sum(np.where(st != 0, cm * xm, 0.0))
    offset = np.sum(np.where(st == 0, cm * xm, 0.0))
    dobj = np.sum(np.where(hl[mine], lb[mine] * zl[mine], 0.0)) - np.sum(np.where(hu[mine], ub[mine] * zu[mine], 0.0))
    if lead:
        dobj += b @ y - np.sum(np.where(fixed[nl:], x[nl:] * y, 0.0))
    fix = np.sum(np.where(fixed[:nl], x[:nl] * aty[:nl], 0.0))
    T = rows([p, d] + comp + [pobj, offset, dobj, fix])
    out = dict(presidual=T[:, 0].max(), dresidual=T[:, 1].max())
    s, mn, mx, cnt = T[0, 2], T[:, 3].min(), T[:, 4].max(), T[0, 5]
    for r in range(1, world):                               # sums in rank order
        s, cnt = s + T[r, 2], cnt + T[r, 5]
    out.update(complementarity=s, mu=s / cnt, mu_min=mn, mu_max=mx, count=cnt)
    sums = T[0, 6:10].copy()
    for r in range(1, world):
        sums += T[r, 6:10]
    out.update(pobjective=sums[0], dobjective=sums[2] - sums[3], offset=sums[1])
    # the four step-to-boundary problems, each with the values StepSizes reads at the winner
    dxl, dxu, dzl, dzu = (step[k] for k in ("dxl", "dxu", "dzl", "dzu"))
    probs = [(xl, dxl), (xu, dxu), (zl, dzl), (zu, dzu)]
    carry = [(xl, dxl, zl, dzl), (xu, dxu, zu, dzu)] * 2
    row = []
    lenr = nl + m if lead else nl
    for k, (v, dv) in enumerate(probs):
        a, j = _boundary(v[:lenr], dv[:lenr])
        if j < 0:
            row += [a, -1.0, 0.0, 0.0, 0.0, 0.0]
        else:
            gidx = c0 + j if j < nl else n + (j - nl)
            row += [a, float(gidx)] + [float(w[j]) for w in carry[k]]
    T = rows(row)
    bnd = []
    for k in range(4):
        best = (1.0, -1.0, 0.0, 0.0, 0.0, 0.0)
        for r in range(world):
            t = tuple(T[r, 6 * k:6 * k + 6])
            if t[1] >= 0 and (t[0] < best[0] or (t[0] == best[0] and (best[1] < 0 or t[1] < best[1]))):
                best = t
        bnd.append(best)
    out["boundary"] = bnd
    # complementarity at the trial point (ap, ad) = (min step xl/xu, min step zl/zu)
    ap, ad = min(bnd[0][0], bnd[1][0]), min(bnd[2][0], bnd[3][0])
    tl = ((xl + ap * dxl) * (zl + ad * dzl))[mine][hl[mine]]
    tu = ((xu + ap * dxu) * (zu + ad * dzu))[mine][hu[mine]]
    T = rows([tl.sum() + tu.sum()])
    tsum = T[0, 0]
    for r in range(1, world):
        tsum += T[r, 0]
    out["trial"] = tsum
    return out, dict(rb=rb, rc=rc, rl=rl, ru=ru)


def _ipm_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    from ipx_amd import partition
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        P = _model()
        c0, c1 = partition.row_range(N, rank, world)
        Ag = partition.col_slab_matrix(P["A"], c0, c1).to_scipy().tocsc()
        itl, stl = partition.col_slice_iterate(P["it"], P["state"], N, rank, world)
        b, c, lb, ub = partition.col_slice_model(P["b"], P["c"], P["lb"], P["ub"], N, rank, world)
        step = {k: partition.col_local_vector(P["step"][k], N, c0, c1) for k in ("dxl", "dxu", "dzl", "dzu")}

        def allsum(v):
            t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))
            dist.all_reduce(t)
            return t.numpy().copy()

        def gather(row):
            parts = [torch.zeros(row.size, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(parts, torch.from_numpy(row))
            return [p.numpy() for p in parts]

        scalars, vecs = ipm_scalars_cols(rank, world, gather, allsum, Ag, N, c0, b, c, lb, ub, stl, itl, step)
        gathered = [None] * world
        dist.all_gather_object(gathered, dict(scalars=scalars, vecs=vecs))
        if rank == 0:
            np.save(out, np.array([gathered], dtype=object), allow_pickle=True)
    finally:
        dist.destroy_process_group()


def test_ipm_reductions_column_partition_world2(oracle, tmp_path):
    import torch.multiprocessing as mp
    from ipx_amd import partition
    from oracle import pyoracle as po
    out = str(tmp_path / "ipm_parts.npy")
    port = 35500 + os.getpid() % 2000
    mp.spawn(_ipm_worker, args=(2, port, out), nprocs=2, join=True)
    parts = np.load(out, allow_pickle=True)[0]
    P = _model()
    A, it, state, st = P["A"], P["it"], P["state"], P["step"]
    Ao = po.Csc(M, N, A.p, A.i, A.x)
    s0, s1 = parts[0]["scalars"], parts[1]["scalars"]
    for key in s0:                                   # every scalar is replicated bit for bit
        assert np.array_equal(np.asarray(s0[key]), np.asarray(s1[key])), key
    close = lambda a, b: abs(a - b) <= 1e-14 * max(1.0, abs(b))
    # residuals: the assembled vectors and the norms
    ref = oracle.iterate_residuals(Ao, state, P["b"], P["c"], P["lb"], P["ub"], it)
    assert np.array_equal(parts[0]["vecs"]["rb"], parts[1]["vecs"]["rb"])
    assert np.abs(parts[0]["vecs"]["rb"] - ref["rb"]).max() <= 1e-14 * np.abs(ref["rb"]).max()
    for key in ("rc", "rl", "ru"):
        got = partition.assemble_cols(M, [p["vecs"][key] for p in parts])
        assert np.abs(got - ref[key]).max() <= 1e-14 * max(1.0, np.abs(ref[key]).max()), key
    assert close(s0["presidual"], ref["presidual"]) and close(s0["dresidual"], ref["dresidual"])
    # complementarity: min, max and count exactly, the sum to 1e-14
    cref = oracle.iterate_complementarity(state, it)
    assert s0["mu_min"] == cref["mu_min"] and s0["mu_max"] == cref["mu_max"]
    hl, hu = (state == 2) | (state == 4), (state == 3) | (state == 4)
    assert s0["count"] == hl.sum() + hu.sum()
    assert close(s0["complementarity"], cref["complementarity"]) and close(s0["mu"], cref["mu"])
    # objectives (offset of the fixed variables and the A_j'y x_j shift included)
    oref = oracle.iterate_objectives(Ao, state, P["b"], P["c"], P["lb"], P["ub"], it)
    assert oref[2] != 0.0
    for got, want in zip((s0["pobjective"], s0["dobjective"], s0["offset"]), oref):
        assert close(got, want), (got, want)
    # step to boundary: alpha, the first global index and the four values there, exactly
    pairs = [("xl", "dxl", "l"), ("xu", "dxu", "u"), ("zl", "dzl", "l"), ("zu", "dzu", "u")]
    for k, (v, dv, side) in enumerate(pairs):
        alpha, blk = oracle.step_to_boundary(it[v], st[dv])
        a, g, x, dx, z, dz = s0["boundary"][k]
        assert a == alpha and int(g) == blk and blk >= 0, (v, a, alpha, g, blk)
        assert (x, dx, z, dz) == (it["x" + side][blk], st["dx" + side][blk], it["z" + side][blk], st["dz" + side][blk])
    owners = {partition.col_owner(int(s0["boundary"][k][1]), N, 2)[0] for k in range(4)}
    assert len(owners) > 1                                         # winners on more than one rank (or replicated)
    # complementarity at the trial point
    ap = min(s0["boundary"][0][0], s0["boundary"][1][0])
    ad = min(s0["boundary"][2][0], s0["boundary"][3][0])
    with np.errstate(invalid="ignore"):
        trial = np.sum(((it["xl"] + ap * st["dxl"]) * (it["zl"] + ad * st["dzl"]))[hl]) + \
            np.sum(((it["xu"] + ap * st["dxu"]) * (it["zu"] + ad * st["dzu"]))[hu])
    assert close(s0["trial"], trial)
