"""Shapes, inputs and group helpers of the sharded-handle tests (tests/test_host_sharded_cases.py on the CPU,
tests/test_gpu_sharded_paths.py on the GPU).  TEST INFRASTRUCTURE: no test functions here.

Every field is TDChain(Dense(D+1 => H, tanh), Dense(H+1 => D)), the MLP handle's; the shapes are the smallest that
still select each kernel family on a sharded handle, the batches leave every rank a ragged last tile (no local batch
is a multiple of 4 or 16)."""
import contextlib

import numpy as np

f32 = np.float32

# name -> (D, H): Q the 4-column family (fused host loop, deferred parameter-gradient GEMM with its late all-reduce);
# V1 the 16-column family with k_vjp<1> (D % 4 != 0), V4 with k_vjp<4> (H > 112): the plain host loop
SHAPES = {"Q": (32, 64), "V1": (30, 24), "V4": (32, 120)}
# global batch -> (ranks, local batch)
GROUPS = {21: (3, 7), 34: (2, 17), 20: (4, 5)}

# The time-series pullback's inputs: tol 1e-4, times [0.5, 1.0], cotangents default_rng(11); `big` multiplies the cotangent
# at t = 0.5 by 1000.  counts: (naccept, nreject, nf) of the float64 and of the float32 restatement of the reversed solve
# (equal: chain_adjoint_np.PINNED's selection condition (1), asserted in tests/test_host_sharded_cases.py for every entry).
# rows = "restatement": the input also meets condition (2) with margin (ROW_MARGIN) and the GPU's trace is held to the
# restatement's attempt by attempt (CA.check_rows); rows = "unsharded": it fails condition (2) — its mixed twins leave
# check_rows' bounds, the decisions of its first attempts are rounding — and the trace is held to the unsharded handle's.
# All ten seed-0 inputs first proposed for the row check (scale 3; Q and V1 at B = 21 and 34, V4 at B = 21, plain and impulse)
# fail condition (2): they stay for everything but the row check.  The row-checked inputs were found on the CPU alone, over
# seeds 0..159 and scales 3, 3.5 and 4.  Condition (3), for every entry: the float64 restatement's own distance to float64
# autograd through RK4 plus the bound its gradients are held to (max(1e-5, 4 x rel(float32 twin, float64))) stays within the
# 3e-4 of the RK4 comparison — at tol 1e-4 the adaptive solve's truncation is of that order (scale 4: up to 2e-3), and an
# input on which the restatement itself misses the bar says nothing about the kernels.
TS_TOL, TS_TIMES, TS_BIG = 1e-4, [0.5, 1.0], (0, 1000.0)
TS_SCALE = 3.0
# Condition (2) as selected here, all on the CPU.  check_rows' bound is max(floor, 4 x |row32 - row64|); on the first attempts
# of a reversed solve mu is still below abstol / reltol, the mu part of utilde is a difference of K's that cancels to ~1e-7
# of them, and its share of EEst is rounding: whoever sums the parameter cotangent in another order lands percents away.
# So the yardstick has to hold more than the two mixed twins with room to spare:
#   (2a) the mixed twins within ROW_MARGIN of the bounds;
#   (2b) the oracle's reversed solve (the unsharded handle's arithmetic bit for bit: the kernels' summation orders, the
#        record's polynomial form) within ORACLE_MARGIN over the attempts before the first impulse (its pullback takes one
#        cotangent, at t2; with a stop at 0.5 those attempts are the time series');
#   (2c) both restatements with the parameter cotangent summed per shard, then over the shards in rank order in float32
#        (rank_regrouped_field: what a sharded handle's VJP does differently) within ROW_MARGIN.
# Selected on (2a) alone, three of ten inputs left the bounds on the MI355X by a factor 1.2 in the EEst of attempts 2
# and 7 (Q 3 x 7, scale 3, seed 27, plain and impulse: 6.4 % against 5.4 %; Q 2 x 17, scale 3.5, seed 35) — on inputs where
# the oracle itself reaches 0.81 and 1.04 of the bound; the same sharded code on one RCCL rank returns the unsharded handle's
# bits, and lrnde_vjp on shards the exact rank-order sum, so those were draws of the rounding, and the inputs were replaced.
# The margins are chosen, not derived: a sharded handle is the oracle's arithmetic plus the regrouping by rank, so the oracle
# gets half the bound (ORACLE_MARGIN) and the regrouping the other half; ROW_MARGIN, a round number, leaves the twins 0.3 of
# the bound for what no CPU statement models.  Both were fixed before the row-checked inputs below ran on the GPU; there
# they reach 0.23 .. 0.67 of the bounds.
# `python tests/sharded_cases.py SHAPE-B[,SHAPE-B...] SCALES SEED0:SEED1 [plain|impulse]` prints every input that meets
# (1), (2a-c) and (3) (select_row_inputs below).  The table was drawn from Q-21,Q-34,V1-21,V1-34,V4-21 3,3.5 0:70 and, for
# the impulse inputs of Q and V1-21, which that left without a rejecting one, 3,3.5 70:160 and 4 0:90 impulse.
ROW_MARGIN, ORACLE_MARGIN = 0.7, 0.5
TS_CASES = {
    "Q-21-plain": dict(shape="Q", B=21, big=None, counts=(18, 0, 112), rows="unsharded"),
    "Q-21-impulse": dict(shape="Q", B=21, big=TS_BIG, counts=(22, 2, 148), rows="unsharded", rejects=True),
    "Q-34-plain": dict(shape="Q", B=34, big=None, counts=(18, 0, 112), rows="unsharded"),
    "Q-34-impulse": dict(shape="Q", B=34, big=TS_BIG, counts=(21, 1, 136), rows="unsharded", rejects=True),
    "V1-21-plain": dict(shape="V1", B=21, big=None, counts=(17, 0, 106), rows="unsharded"),
    "V1-21-impulse": dict(shape="V1", B=21, big=TS_BIG, counts=(20, 0, 124), rows="unsharded"),
    "V1-34-plain": dict(shape="V1", B=34, big=None, counts=(20, 0, 124), rows="unsharded"),
    "V1-34-impulse": dict(shape="V1", B=34, big=TS_BIG, counts=(23, 0, 142), rows="unsharded"),
    "V4-21-plain": dict(shape="V4", B=21, big=None, counts=(18, 0, 112), rows="unsharded"),
    "V4-21-impulse": dict(shape="V4", B=21, big=TS_BIG, counts=(21, 0, 130), rows="unsharded"),
    # row-checked: conditions (1), (2a-c) and (3); the same five shape / rank layouts, plain and impulse
    "row-Q-21-plain": dict(shape="Q", B=21, scale=3.0, seed=43, big=None, counts=(19, 0, 118), rows="restatement"),
    "row-Q-21-impulse": dict(shape="Q", B=21, scale=3.5, seed=104, big=TS_BIG, counts=(26, 1, 166), rows="restatement", rejects=True),
    "row-Q-34-plain": dict(shape="Q", B=34, scale=3.5, seed=39, big=None, counts=(22, 0, 136), rows="restatement"),
    "row-Q-34-impulse": dict(shape="Q", B=34, scale=3.0, seed=103, big=TS_BIG, counts=(20, 2, 136), rows="restatement", rejects=True),
    "row-V1-21-plain": dict(shape="V1", B=21, scale=3.0, seed=58, big=None, counts=(15, 0, 94), rows="restatement"),
    "row-V1-21-impulse": dict(shape="V1", B=21, scale=4.0, seed=35, big=TS_BIG, counts=(32, 2, 208), rows="restatement", rejects=True),
    "row-V1-34-plain": dict(shape="V1", B=34, scale=3.0, seed=19, big=None, counts=(17, 0, 106), rows="restatement"),
    "row-V1-34-impulse": dict(shape="V1", B=34, scale=3.0, seed=19, big=TS_BIG, counts=(20, 1, 130), rows="restatement", rejects=True),
    "row-V4-21-plain": dict(shape="V4", B=21, scale=3.0, seed=36, big=None, counts=(16, 0, 100), rows="restatement"),
    "row-V4-21-impulse": dict(shape="V4", B=21, scale=3.5, seed=47, big=TS_BIG, counts=(21, 1, 136), rows="restatement", rejects=True),
    # a cotangent at t0 (save_start): yardsticks 1 and 4 and RK4 autograd
    "V1-21-t0": dict(shape="V1", B=21, big=None, times=[0.0, 0.5, 1.0], save_start=True, counts=None, rows="unsharded"),
}

# Adams rejecting case, rank consistency only (the oracle: 134 accepted, 1 rejected)
ADAMS_REJECT = dict(shape="V1", B=21, scale=10.0, tol=1e-3, solver="vcab3")


def model_of(P, shape):
    D, H = SHAPES[shape]
    return P.TDChain(P.Chain(P.Dense(D + 1, H, "tanh"), P.Dense(H + 1, D)))


def inputs(P, shape, B, scale=2.0, seed=0):
    """(model, p, x) as tests/test_gpu_backward._mk draws them"""
    D, _H = SHAPES[shape]
    model = model_of(P, shape)
    p = P.glorot_params(model, seed=seed) * f32(scale)
    p = (p + np.random.default_rng(seed + 1).standard_normal(p.size).astype(f32) * f32(0.02)).astype(f32)
    x = np.random.default_rng(seed + 2).random((B, D), dtype=f32)
    return model, p, x


def ts_cotangents(B, D, times=TS_TIMES, big=None):
    cots = np.random.default_rng(11).standard_normal((len(times), B, D)).astype(f32)
    if big is not None:
        cots[big[0]] *= f32(big[1])
    return cots


def ts_case_inputs(P, name):
    """(model, p, x, times, cots, tol) of a TS_CASES entry"""
    c = TS_CASES[name]
    model, p, x = inputs(P, c["shape"], c["B"], scale=c.get("scale", TS_SCALE), seed=c.get("seed", 0))
    times = list(c.get("times", TS_TIMES))
    return model, p, x, times, ts_cotangents(c["B"], SHAPES[c["shape"]][0], times=times, big=c["big"]), TS_TOL


def shard(a, r, nranks, axis=0):
    """rank r's contiguous block of samples along `axis`"""
    B = a.shape[axis]
    assert B % nranks == 0
    per = B // nranks
    return np.ascontiguousarray(np.take(a, range(r * per, (r + 1) * per), axis=axis))


def rank_order_sum(parts):
    """((g_0 + g_1) + g_2 ...) in float32: what the in-process communicator's sum kernel returns on every rank"""
    acc = np.asarray(parts[0], f32).copy()
    for g in parts[1:]:
        acc = (acc + np.asarray(g, f32)).astype(f32)
    return acc


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def rank_regrouped_field(nranks):
    """chain_adjoint_np.Field with the parameter cotangent summed per shard and then over the shards in rank order in
    float32: the one thing the VJP of a sharded handle does differently"""
    import chain_adjoint_np as CA
    base = CA.Field

    class RankRegrouped(base):
        def vjp(self, y, t, lam):
            per = y.shape[0] // nranks
            parts = [base.vjp(self, y[r * per:(r + 1) * per], t, lam[r * per:(r + 1) * per]) for r in range(nranks)]
            return np.concatenate([q[0] for q in parts], axis=0), rank_order_sum([q[1] for q in parts])
    return RankRegrouped


def rows_ratio(rows, r64, r32, before_s=None):
    """worst |row - row64| / bound over `rows` (those with s < before_s), chain_adjoint_np.check_rows' bounds"""
    import chain_adjoint_np as CA
    smax = max(abs(r[0]) for r in r64["rows"])
    worst = 0.0
    for i, (g, a, b) in enumerate(zip(rows, r64["rows"], r32["rows"])):
        if before_s is not None and a[0] >= before_s:
            break
        floors = (CA.S_FLOOR * smax, (CA.DT0_FLOOR if i == 0 else CA.DT_FLOOR) * abs(a[1]), CA.EEST_FLOOR * abs(a[2]))
        for k in range(3):
            worst = max(worst, abs(g[k] - a[k]) / max(floors[k], CA.MARGIN * abs(b[k] - a[k])))
    return worst


# ---- GPU side ---------------------------------------------------------------------------------------------------------
def unsharded(P, model, p):
    import torch
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    h = Handle(_mlp_desc(model))
    h.set_params(torch.from_numpy(p))
    return h


@contextlib.contextmanager
def group(P, model, p, nranks):
    """nranks handles, each on its own stream, joined to one fresh in-process communicator (as
    test_gpu_sharded_loopback._handles); closed on the way out whatever happened — a communicator is never reused after a
    failed call"""
    import torch
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    lc = P.LocalComm(nranks)
    hs = []
    try:
        for r in range(nranks):
            h = Handle(_mlp_desc(model), stream=torch.cuda.Stream())
            h.set_params(torch.from_numpy(p))
            lc.join(h, r)
            hs.append(h)
        torch.cuda.synchronize()
        yield hs
    finally:
        torch.cuda.synchronize()
        lc.close()
        for h in hs:
            h.close()


def on_ranks(P, hs, fn):
    """fn(rank, handle) of every rank on its own host thread, with the handle's stream current (what the wrappers allocate
    and clear for the call is then ordered with the call's kernels); results in rank order"""
    import torch

    def one(r):
        with torch.cuda.stream(hs[r]._stream):
            return fn(r, hs[r])
    out = P.run_ranks([(lambda r=r: one(r)) for r in range(len(hs))])
    torch.cuda.synchronize()
    return out


def dev_shards(a, nranks, axis=0):
    import torch
    out = [torch.from_numpy(shard(a, r, nranks, axis)).cuda() for r in range(nranks)]
    torch.cuda.synchronize()
    return out


def traced(h, fn, cap=4096):
    """fn() with the adjoint trace on: (result, rows)"""
    h.set_adjoint_trace(cap)
    try:
        out = fn()
        rows = h.adjoint_trace()
    finally:
        h.set_adjoint_trace(0)
    return out, rows


def np_(t):
    return t.detach().cpu().numpy()


# ---- the CPU search that produced the row-checked entries of TS_CASES ---------------------------------------------------
def select_row_inputs(P, O, shape, B, scales, seeds, bigs=(None, TS_BIG)):
    """yields (scale, seed, big, counts, dict of the worst ratios) for every input of the shape and batch that meets
    conditions (1), (2a), (2b), (2c) and (3); P the package, O the oracle module.  CPU only."""
    import chain_adjoint_np as CA
    from test_gpu_timeseries_pullback import _reference_grads
    D, H = SHAPES[shape]
    nranks = GROUPS[B][0]
    times, tol = list(TS_TIMES), TS_TOL
    base = CA.Field

    def worst(r, r64, r32):
        if r["counts"] != r64["counts"] or [q[3] for q in r["rows"]] != [q[3] for q in r64["rows"]]:
            return float("inf")
        return rows_ratio(r["rows"], r64, r32)
    for scale in scales:
        for seed in seeds:
            model, p, x = inputs(P, shape, B, scale=scale, seed=seed)
            fld = O.MlpField(D, H, p, nthreads=2)
            for big in bigs:
                cots = ts_cotangents(B, D, times=times, big=big)
                try:
                    r64 = CA.pullback(model, p, x, times, cots, tol)
                    r32 = CA.pullback(model, p, x, times, cots, tol, dtype=np.float32)
                except RuntimeError:
                    continue
                if not (r64["counts"] == r32["counts"] and r64["fwd"] == r32["fwd"]
                        and [q[3] for q in r64["rows"]] == [q[3] for q in r32["rows"]]):
                    continue                                                               # (1)
                ro = O.node_backward(fld, x, 0.0, 1.0, tol, tol, cots[-1], mode="unbiased", t1_or_rand=times[0], w_reg=0.0, trace=True)
                w_or = rows_ratio(ro["trace_bwd"], r64, r32, before_s=-float(f32(times[0])))
                if w_or > ORACLE_MARGIN:
                    continue                                                               # (2b)
                w_mx = max(worst(CA.pullback(model, p, x, times, cots, tol, **kw), r64, r32)
                           for kw in (dict(dtype=np.float32, interp=np.float64), dict(dtype=np.float64, interp=np.float32)))
                if w_mx > ROW_MARGIN:
                    continue                                                               # (2a)
                CA.Field = rank_regrouped_field(nranks)
                try:
                    w_rg = max(worst(CA.pullback(model, p, x, times, cots, tol, dtype=dt), r64, r32) for dt in (np.float32, np.float64))
                finally:
                    CA.Field = base
                if w_rg > ROW_MARGIN:
                    continue                                                               # (2c)
                gx, gp = _reference_grads(p, x, D, H, times, cots)
                tot = max(rel(r64[k], g) + max(1e-5, 4.0 * rel(r32[k], r64[k])) for k, g in (("dx", gx), ("dp", gp)))
                if tot > 3e-4:
                    continue                                                               # (3)
                yield scale, seed, big, r64["counts"], dict(oracle=w_or, mixed=w_mx, regrouped=w_rg, rk4_plus_bound=tot)


if __name__ == "__main__":
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "oracle"), os.path.join(root, "tests")]
    import lrnde_amd
    import oracle
    oracle.build()
    lo, hi = sys.argv[3].split(":")
    kind = sys.argv[4] if len(sys.argv) > 4 else None
    bigs = {None: (None, TS_BIG), "plain": (None,), "impulse": (TS_BIG,)}[kind]
    for case in sys.argv[1].split(","):
        shape, B = case.split("-")
        for scale, seed, big, counts, w in select_row_inputs(lrnde_amd, oracle, shape, int(B), [float(v) for v in sys.argv[2].split(",")],
                                                              range(int(lo), int(hi)), bigs):
            print(f"{shape} B={B} scale={scale} seed={seed} {'impulse' if big else 'plain'} counts={counts} "
                  + " ".join(f"{k}={v:.2g}" for k, v in w.items()), flush=True)
