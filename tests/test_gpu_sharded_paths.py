"""What a batch-sharded MLP handle (nranks > 1) runs besides its forward solve (that one: tests/test_gpu_sharded_loopback.py):
lrnde_vjp and lrnde_step_reg_grad called directly, the time-series pullback, the regulariser's sweep, the Adams solvers,
the fused forward + head — on 2, 3 and 4 ranks of the in-process communicator, ragged local batches, the 4-column family
(shape Q: fused host loop, deferred GEMM with its late all-reduce) and the 16-column one (V1: k_vjp<1>, V4: k_vjp<4>, the
plain host loop); and the time-series pullback and an Adams solve on one RCCL rank.  Shapes, inputs, group helpers:
tests/sharded_cases.py; what is asserted of the inputs on the CPU: tests/test_host_sharded_cases.py.

Yardsticks.  (1) across ranks, exact: every rank computes its controller from the same all-reduced scalars, so stats,
every row of the adjoint trace, reg_val, t1, the loss and the replicated gradients are equal bit for bit.  (2) the
rank-order float32 sum of the oracle's per-shard parameter cotangents, exact.  (3) the float64 restatement of the GLOBAL
batch (tests/chain_adjoint_np.py): gradients within max(1e-5, 4 x rel(float32 twin, float64)), and within 3e-4 of float64
autograd through RK4; trace rows by CA.check_rows on the inputs that meet its selection conditions.  (4) the unsharded
handle (bit-equal to the oracle), where the estimate is rounding-dominated: forward equal bit for bit, |naccept
difference| <= 1, first trace row (s equal, dt within CA.DT0_FLOOR, EEst within CA.EEST_FLOOR), gradients at 2e-4."""
import functools

import numpy as np
import pytest

import sharded_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture
def plain(gpu_pkg):
    """maker of unsharded handles, closed when the test is over"""
    made = []

    def make(model, p):
        made.append(SC.unsharded(gpu_pkg, model, p))
        return made[-1]
    yield make
    for h in made:
        h.close()


def _counts(st):
    return (st["naccept"], st["nreject"], st["nf"])


def _loops(tag, got, ref, shape):
    """which adjoint loop ran (lrnde_last_adjoint_info): the host-controlled one (kind 0) on every rank of a sharded group;
    on the unsharded handle the device-controlled one (kind 1) for the 4-column shape Q, the host loop for V1 and V4 — so a
    change of the routing that moves a shape to another kernel family does not leave these tests green"""
    assert [q["kind"] for q in got] == [0] * len(got), (tag, [q["kind"] for q in got])
    assert ref["kind"] == (1 if shape == "Q" else 0), (tag, shape, ref["kind"])


def _yardstick1(tag, outs, keys=("stats_bwd", "rows", "dp")):
    for r, o in enumerate(outs[1:], 1):
        for k in keys:
            a, b = outs[0][k], o[k]
            if hasattr(a, "detach"):
                assert np.array_equal(SC.np_(a), SC.np_(b)), (tag, k, "rank", r)
            elif isinstance(a, np.ndarray):
                assert np.array_equal(a, b), (tag, k, "rank", r)
            else:
                assert a == b, (tag, k, "rank", r, a, b)


def _yardstick4(tag, got, ref, dx, bar=2e-4, steps=True):
    """got: rank 0's dict(stats_bwd, rows, dp) (the ranks agree: yardstick 1), dx the stacked blocks; ref: the unsharded
    handle's dict(stats_bwd, rows, dx, dp).  steps=False: the gradients alone (and the numbers printed)"""
    import chain_adjoint_np as CA
    dn = got["stats_bwd"]["naccept"] - ref["stats_bwd"]["naccept"]
    g, a = got["rows"][0], ref["rows"][0]
    ddt, dee = abs(g[1] - a[1]) / abs(a[1]), abs(g[2] - a[2]) / abs(a[2])
    rx, rp = SC.rel(dx, SC.np_(ref["dx"])), SC.rel(SC.np_(got["dp"]), SC.np_(ref["dp"]))
    print(f"{tag}: vs the unsharded handle: adjoint counts {_counts(got['stats_bwd'])} / {_counts(ref['stats_bwd'])}, first row "
          f"dt {ddt:.2e} (floor {CA.DT0_FLOOR:.0e}) EEst {dee:.2e} (floor {CA.EEST_FLOOR:.0e}), dx {rx:.2e} dp {rp:.2e} (bar {bar:.0e})")
    assert got["stats_bwd"]["retcode"] == 0
    if steps:
        assert abs(dn) <= 1
        assert g[0] == a[0] and ddt <= CA.DT0_FLOOR and dee <= CA.EEST_FLOOR, (tag, g, a)
    assert rx < bar and rp < bar, (tag, rx, rp)


# ---- 1. lrnde_vjp on shards -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,B", [(s, B) for s in SC.SHAPES for B in (21, 34)] + [("Q", 20)])
def test_vjp_on_shards_is_the_rank_order_sum_of_the_oracles_shards(oracle, gpu_pkg, shape, B):
    """lrnde_vjp called directly on 3 x 7, 2 x 17 and 4 x 5 samples: every rank's gp is ((g_0 + g_1) + g_2 ...) in float32
    of the oracle's per-shard cotangents, bit for bit (a rank's local sum has the oracle's bits, the communicator adds in
    rank order), and the stacked dy is the oracle's dy of the global batch, bit for bit.  Measured: equal on all 7 cases."""
    P = gpu_pkg
    D, H = SC.SHAPES[shape]
    nranks, _ = SC.GROUPS[B]
    model, p, x = SC.inputs(P, shape, B)
    lam = np.random.default_rng(9).standard_normal(x.shape).astype(np.float32)
    fld = oracle.MlpField(D, H, p, nthreads=4)
    dy_ref, _ = oracle.mlp_vjp(fld, x, 0.3, lam)
    want = SC.rank_order_sum([oracle.mlp_vjp(fld, SC.shard(x, r, nranks), 0.3, SC.shard(lam, r, nranks))[1] for r in range(nranks)])
    with SC.group(P, model, p, nranks) as hs:
        xs, ls = SC.dev_shards(x, nranks), SC.dev_shards(lam, nranks)
        got = SC.on_ranks(P, hs, lambda r, h: h.vjp(xs[r], 0.3, ls[r]))
        dy = np.concatenate([SC.np_(g[0]) for g in got], axis=0)
        gps = [SC.np_(g[1]) for g in got]
    print(f"{shape} {nranks} x {B // nranks}: rel(gp, rank-order sum) {[SC.rel(g, want) for g in gps]}, rel(dy, oracle) {SC.rel(dy, dy_ref):.1e}")
    assert np.array_equal(dy, dy_ref)
    for r, g in enumerate(gps):
        assert np.array_equal(g, gps[0]), ("gp must come out replicated", r)
        assert np.array_equal(g, want), (r, SC.rel(g, want))


# ---- 2. lrnde_step_reg_grad on shards ---------------------------------------------------------------------------------
@pytest.mark.parametrize("reg_type", ["error_estimate", "stiffness_estimate"])
@pytest.mark.parametrize("shape", ["Q", "V1"])
def test_step_reg_grad_on_shards(oracle, gpu_pkg, shape, reg_type):
    """the reverse sweep through one local step on 3 x 7 samples (inputs of test_reg_gradient_matches_oracle): reg_val on
    every rank is the oracle's value of the GLOBAL batch bit for bit, gp is replicated and within 3e-4 of the oracle's
    global gradient (that test's docstring: same cotangent seeds, regrouped sums).  Measured rel(gp, oracle): error_estimate
    4.8e-6 (Q) and 5.2e-6 (V1), stiffness_estimate 2.2e-7 and 2.3e-7; reg_val equal on all ranks."""
    P = gpu_pkg
    D, H = SC.SHAPES[shape]
    nranks, B = 3, 21
    model, p, x = SC.inputs(P, shape, B, scale=3.0)
    fld = oracle.MlpField(D, H, p, nthreads=4)
    k1 = fld.rhs(x, 0.2)
    gp_ref, rv_ref = oracle.step_reg_grad(fld, x, k1, 0.2, 0.1, 1e-3, 1e-3, reg_type)
    with SC.group(P, model, p, nranks) as hs:
        xs, ks = SC.dev_shards(x, nranks), SC.dev_shards(k1, nranks)
        got = SC.on_ranks(P, hs, lambda r, h: h.step_reg_grad(xs[r], ks[r], 0.2, 0.1, 1e-3, 1e-3, reg_type))
        gps = [SC.np_(g[0]) for g in got]
    d = SC.rel(gps[0], gp_ref)
    print(f"step_reg_grad {shape} {reg_type} 3 x 7: reg_val {[float(g[1]) for g in got]} oracle {float(rv_ref)}; rel(gp, oracle) {d:.2e}")
    for r, g in enumerate(got):
        assert g[1] == rv_ref, (r, g[1], rv_ref)
        assert np.array_equal(gps[r], gps[0]), ("gp must come out replicated", r)
    assert np.isfinite(gps[0]).all() and (gps[0] != 0).any()
    assert d <= 3e-4, d


# ---- 3. the time-series pullback on shards ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _restatement(name):
    """(r64, r32, (gx, gp) of float64 RK4 autograd) of a time-series case, computed once"""
    import lrnde_amd as P
    import chain_adjoint_np as CA
    from test_gpu_timeseries_pullback import _reference_grads
    c = SC.TS_CASES[name]
    model, p, x, times, cots, tol = SC.ts_case_inputs(P, name)
    kw = dict(save_start=c.get("save_start", False))
    r64 = CA.pullback(model, p, x, times, cots, tol, **kw)
    r32 = CA.pullback(model, p, x, times, cots, tol, dtype=np.float32, **kw)
    D, H = SC.SHAPES[c["shape"]]
    return r64, r32, _reference_grads(p, x, D, H, times, cots)


def _ts_forward_backward(h, x, cots, times, tol, save_start):
    fw = h.node_forward_record_ts(x, 0.0, 1.0, tol, tol, [t for t in times if t > 0.0], mode="none", maxiters=10000,
                                  save_start=save_start)
    bw, rows = SC.traced(h, lambda: h.node_backward_recorded_ts(cots, 0.0))
    bw.update(rows=rows, u=fw["u"], t=fw["t"], stats_fwd=fw["stats"], kind=h.last_adjoint_info()["kind"])
    return bw


@pytest.mark.parametrize("name", list(SC.TS_CASES))
def test_timeseries_pullback_on_shards(gpu_pkg, plain, name):
    """lrnde_node_forward_record_ts + lrnde_node_backward_recorded_ts, mode none, cotangents at t = 0.5 (an impulse on the
    local lambda block, K1 re-evaluated with an all-reduced mu, the tstop hit on every rank) and t = 1; the `impulse` inputs
    multiply the first by 1000 (Q: the attempts after it are rejected), `t0` adds save_start with a cotangent at t0.
    Forward series stacked == the unsharded handle's, bit for bit; yardstick 1 on stats and every trace row;
    nf == 3 + 6 x attempts + impulses inside the span; gradients by yardstick 3 (restatement and RK4); the trace by
    CA.check_rows where the input meets the selection conditions (sharded_cases.TS_CASES `rows`), by yardstick 4 otherwise.
    Measured on the MI355X.  Row-checked inputs, worst |row - row64| / bound over (s, dt, EEst): Q 3 x 7 0.23 plain, 0.42
    impulse (26 accepted, 1 rejected); Q 2 x 17 0.34, 0.41 (20, 2); V1 3 x 7 0.24, 0.31 (32, 2); V1 2 x 17 0.27, 0.67 (20, 1);
    V4 3 x 7 0.47, 0.26 (21, 1); counts equal to the restatement's on all ten.  The ten inputs off the row check: counts equal
    to the unsharded handle's on all, first-row dt equal or 3e-7 apart, EEst 1.7e-3 .. 1.1e-2 apart (floor 2e-2), gradients
    7e-7 .. 4e-6 from the unsharded handle's; on V1 2 x 17 impulse both handles take (24, 0) steps, the restatements (23, 0).
    Gradients, all 21 inputs: 6e-7 .. 5.0e-5 from the float64 restatement (each within its bound; the nearest V1-21-plain
    5.6e-6 against 1.0e-5, V1-34-plain 5.0e-5 against 1.7e-4), 2.6e-6 .. 1.0e-4 from RK4 autograd (bar 3e-4).  t0 case: counts
    (17, 0, 106) on both handles, first-row EEst 1.6e-3 apart, gradients 3.9e-6 / 1.8e-6 from the unsharded handle's."""
    import torch
    import chain_adjoint_np as CA
    P = gpu_pkg
    c = SC.TS_CASES[name]
    nranks, _ = SC.GROUPS[c["B"]]
    model, p, x, times, cots, tol = SC.ts_case_inputs(P, name)
    save_start = c.get("save_start", False)
    r64, r32, (gx, gp) = _restatement(name)
    hu = plain(model, p)
    ref = _ts_forward_backward(hu, torch.from_numpy(x).cuda(), torch.from_numpy(cots).cuda(), times, tol, save_start)
    with SC.group(P, model, p, nranks) as hs:
        xs, cs = SC.dev_shards(x, nranks), SC.dev_shards(cots, nranks, axis=1)
        got = SC.on_ranks(P, hs, lambda r, h: _ts_forward_backward(h, xs[r], cs[r], times, tol, save_start))
        u = np.concatenate([SC.np_(g["u"]) for g in got], axis=1)
        dx = np.concatenate([SC.np_(g["dx"]) for g in got], axis=0)
        dp = SC.np_(got[0]["dp"])
    assert [float(t) for t in got[0]["t"]] == [float(np.float32(t)) for t in times]
    assert np.array_equal(u, SC.np_(ref["u"])), "the forward series differs from the unsharded run"
    _yardstick1(name, got, keys=("stats_fwd", "stats_bwd", "rows", "dp", "t"))
    _loops(name, got, ref, c["shape"])
    assert got[0]["stats_fwd"] == ref["stats_fwd"]
    sb, rows = got[0]["stats_bwd"], got[0]["rows"]
    inside = sum(1 for t in times if 0.0 < t < 1.0)
    assert sb["retcode"] == 0 and len(rows) == sb["naccept"] + sb["nreject"] and sb["nf"] == 3 + 6 * len(rows) + inside
    if c["rows"] == "restatement":
        CA.check_rows(f"{name} on {nranks} ranks", dict(counts=_counts(sb), rows=rows), r64, r32)
        if c.get("rejects"):
            assert sb["nreject"] >= 1
    else:
        _yardstick4(name, got[0], ref, dx)
    bx, bp = max(1e-5, 4.0 * SC.rel(r32["dx"], r64["dx"])), max(1e-5, 4.0 * SC.rel(r32["dp"], r64["dp"]))
    print(f"{name} on {nranks} ranks: adjoint counts {_counts(sb)} restatement {r64['counts']}; vs float64 restatement dx "
          f"{SC.rel(dx, r64['dx']):.2e} (bound {bx:.2e}) dp {SC.rel(dp, r64['dp']):.2e} (bound {bp:.2e}); vs RK4 autograd dx "
          f"{SC.rel(dx, gx):.2e} dp {SC.rel(dp, gp):.2e} (bar 3e-4)")
    assert SC.rel(dx, r64["dx"]) <= bx and SC.rel(dp, r64["dp"]) <= bp
    assert SC.rel(dx, gx) < 3e-4 and SC.rel(dp, gp) < 3e-4


# ---- 4. the regulariser on shards -------------------------------------------------------------------------------------
REG_RUNS = [("unbiased", "stiffness_estimate", 0.0), ("unbiased", "stiffness_estimate", 2.5),
            ("biased", "error_estimate", 0.0), ("biased", "error_estimate", 1.0)]


def _reg_runs(h, x, g, tol):
    out = []
    for mode, reg_type, w in REG_RUNS:
        fw = h.node_forward_record(x, 0.0, 1.0, tol, tol, mode=mode, reg_type=reg_type, t1_or_rand=0.43, maxiters=10000)
        bw, rows = SC.traced(h, lambda: h.node_backward_recorded(g, w))
        bw.update(rows=rows, reg_val=fw["reg_val"], t1=fw["t1"], nfe=fw["nfe"], stats_fwd=fw["stats"], u_end=fw["u_end"],
                  kind=h.last_adjoint_info()["kind"])
        out.append(bw)
    return out


@pytest.mark.parametrize("shape", ["Q", "V1"])
def test_regulariser_on_shards(gpu_pkg, plain, shape):
    """the recorded forward and the pullback with the regulariser's sweep on 3 x 7 samples (scale 3, tol 1e-4,
    t1_or_rand 0.43), on one group: :unbiased + stiffness_estimate with w_reg 0 and 2.5, :biased + error_estimate with w_reg 0
    and 1 (one w_reg = 0 run per mode: the reversed solve stops at the mode's t1).  reg_val, t1, nfe == the unsharded handle's
    bit for bit; dx of the w_reg != 0 run == the w_reg = 0 run's bit for bit; (dp_w - dp_0), the sweep's contribution, within
    3e-4 of the same difference on the unsharded handle (test_reg_gradient_matches_oracle's bound); yardstick 1 throughout.
    Besides: dx and dp of every run within 2e-4 of the unsharded handle's.  The adjoint's steps are printed, not compared:
    these inputs are the rounding-dominated kind (V1: the float64 restatement of the :unbiased solve takes 15 steps, the float32
    one 22; the first attempt's EEst is 2.09e-3 / 2.14e-3 / 2.16e-3 in the restatements and the oracle, 2.23e-3 on the shards),
    and :biased stops the reversed solve at every accepted forward step, each stop leaves a remainder step of dt 1e-4 .. 1e-3
    whose estimate (1e-6 .. 1e-5) is rounding alone, and the controller climbs back from it over five to seven attempts
    steered by that noise — the unsharded handle takes 49 steps on shape Q, the shards 41, with gradients 1e-6 apart.
    (On the CPU seven correct statements of that solve take 31 .. 49 steps on Q and 29 .. 41 on V1, and regrouping by rank alone
    moves the restatement's count: tests/test_host_sharded_cases.py.)
    Measured: reg_val, t1, nfe, u_end equal on both shapes; (dp_w - dp_0) against the unsharded handle's 2.9e-7 (:unbiased
    stiffness_estimate, Q and V1: the term is 1.4 and 4.5 times |dp_0|), 1.3e-4 (Q) and 2.0e-4 (V1) for :biased error_estimate,
    where the term is 5e-5 of |dp_0| and the float32 subtraction on either side leaves it 1e-3 of rounding per element;
    dx and dp of every run 4e-7 .. 2.5e-6 from the unsharded handle's; adjoint steps (accepted, sharded / unsharded) Q 18 / 18
    and 41 / 49, V1 15 / 15 and 29 / 29, first-row EEst 3.3e-3 (Q) and 3.3e-2 (V1) apart."""
    import torch
    P = gpu_pkg
    nranks, B, tol = 3, 21, 1e-4
    model, p, x = SC.inputs(P, shape, B, scale=3.0)
    g = np.random.default_rng(4).standard_normal(x.shape).astype(np.float32)
    hu = plain(model, p)
    ref = _reg_runs(hu, torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), tol)
    with SC.group(P, model, p, nranks) as hs:
        xs, gs = SC.dev_shards(x, nranks), SC.dev_shards(g, nranks)
        got = SC.on_ranks(P, hs, lambda r, h: _reg_runs(h, xs[r], gs[r], tol))
        dxs = [np.concatenate([SC.np_(got[r][i]["dx"]) for r in range(nranks)], axis=0) for i in range(len(REG_RUNS))]
        ues = [np.concatenate([SC.np_(got[r][i]["u_end"]) for r in range(nranks)], axis=0) for i in range(len(REG_RUNS))]
    for i, (mode, reg_type, w) in enumerate(REG_RUNS):
        tag = f"{shape} {mode} {reg_type} w_reg={w}"
        runs = [got[r][i] for r in range(nranks)]
        _yardstick1(tag, runs, keys=("stats_fwd", "stats_bwd", "rows", "dp", "reg_val", "t1", "nfe"))
        q, a = runs[0], ref[i]
        _loops(tag, runs, a, shape)
        assert q["reg_val"] == a["reg_val"] and q["t1"] == a["t1"] and q["nfe"] == a["nfe"] and q["stats_fwd"] == a["stats_fwd"], tag
        assert q["reg_val"] > 0 and np.array_equal(ues[i], SC.np_(a["u_end"]))
        _yardstick4(tag, q, a, dxs[i], steps=False)
    for i0, iw in ((0, 1), (2, 3)):
        mode, reg_type, w = REG_RUNS[iw]
        assert np.array_equal(dxs[iw], dxs[i0]), "the regulariser has no gradient to x"
        dgot = SC.np_(got[0][iw]["dp"]).astype(np.float64) - SC.np_(got[0][i0]["dp"]).astype(np.float64)
        dref = SC.np_(ref[iw]["dp"]).astype(np.float64) - SC.np_(ref[i0]["dp"]).astype(np.float64)
        d = SC.rel(dgot, dref)
        print(f"{shape} {mode} {reg_type}: |dp_w - dp_0| / |dp_0| {np.linalg.norm(dref) / np.linalg.norm(SC.np_(ref[i0]['dp'])):.2e}; "
              f"rel(sharded difference, unsharded difference) {d:.2e} (bar 3e-4)")
        assert np.linalg.norm(dref) > 0 and d <= 3e-4, d


# ---- 5. the Adams solvers on shards -----------------------------------------------------------------------------------
def _adams_runs(h, x, g, tol, sv):
    sol = h.solve(x, 0.0, 1.0, tol, tol, saveat=sv, maxiters=10000, trace=True)
    fw = h.node_forward_record(x, 0.0, 1.0, tol, tol, mode="unbiased", t1_or_rand=0.43, maxiters=10000)
    bw, rows = SC.traced(h, lambda: h.node_backward_recorded(g, 0.0))
    bw.update(rows=rows, reg_val=fw["reg_val"], t1=fw["t1"], nfe=fw["nfe"], stats_fwd=fw["stats"], u_end=fw["u_end"],
              stats=sol["stats"], trace=sol["trace"], t=sol["t"], u=sol["u"], kind=h.last_adjoint_info()["kind"])
    return bw


@pytest.mark.parametrize("solver", ["vcab3", "vcabm3"])
@pytest.mark.parametrize("shape,B", [("Q", 21), ("V1", 34)])
def test_adams_on_shards(gpu_pkg, plain, shape, B, solver):
    """lrnde_set_solver(vcab3 | vcabm3) on a sharded handle (3 x 7, 2 x 17; scale 3, tol 1e-4, saveat [0.37, 1]): the solve's
    norms are all-reduced rank slots, so stats and every trace row agree across ranks bit for bit; against the unsharded
    handle (bit-equal to the oracle, tests/test_gpu_adams.py) equal (naccept, nreject, nf), first dt within CA.DT0_FLOOR,
    saved states within 1e-5 of their scale.  Then the recorded Adams forward (:unbiased) and its pullback on the same
    shards: yardsticks 1 and 4 (stats, t1, nfe, reg_val and u_end of the forward bit for bit).  Measured: the sharded solve's stats, trace rows and saved states EQUAL the unsharded handle's on all four cases
    (vcab3 58 / 51 accepted steps on Q / V1, vcabm3 36 / 32; first dt and states 0.0 apart), so do the recorded forward's
    u_end and reg_val; the pullback takes the unsharded handle's step counts (18 on Q, 17 on V1), first-row EEst 7e-4 .. 9e-3
    apart, dx / dp 1e-6 .. 2.2e-6 apart."""
    import torch
    import chain_adjoint_np as CA
    P = gpu_pkg
    nranks, _ = SC.GROUPS[B]
    tol, sv = 1e-4, [0.37, 1.0]
    model, p, x = SC.inputs(P, shape, B, scale=3.0)
    g = np.random.default_rng(4).standard_normal(x.shape).astype(np.float32)
    hu = plain(model, p)
    hu.set_solver(solver)
    ref = _adams_runs(hu, torch.from_numpy(x).cuda(), torch.from_numpy(g).cuda(), tol, sv)
    with SC.group(P, model, p, nranks) as hs:
        for h in hs:
            h.set_solver(solver)
        xs, gs = SC.dev_shards(x, nranks), SC.dev_shards(g, nranks)
        got = SC.on_ranks(P, hs, lambda r, h: _adams_runs(h, xs[r], gs[r], tol, sv))
        u = np.concatenate([SC.np_(q["u"]) for q in got], axis=1)
        dx = np.concatenate([SC.np_(q["dx"]) for q in got], axis=0)
        ue = np.concatenate([SC.np_(q["u_end"]) for q in got], axis=0)
    tag = f"{solver} {shape} {nranks} x {B // nranks}"
    _yardstick1(tag, got, keys=("stats", "trace", "t", "stats_fwd", "stats_bwd", "rows", "dp", "reg_val", "t1", "nfe"))
    _loops(tag, got, ref, shape)
    q = got[0]
    uref = SC.np_(ref["u"])
    ddt = abs(float(q["trace"]["dt"][0]) - float(ref["trace"]["dt"][0])) / float(ref["trace"]["dt"][0])
    du = float(np.abs(u - uref).max() / np.abs(uref).max())
    print(f"{tag}: solve counts {_counts(q['stats'])} / unsharded {_counts(ref['stats'])}, first dt {ddt:.2e} (floor {CA.DT0_FLOOR:.0e}), "
          f"saved states {du:.2e} of scale (bar 1e-5), trace rows equal to the unsharded run's: "
          f"{bool(np.array_equal(q['trace'], ref['trace']))}")
    assert q["stats"]["retcode"] == 0 and _counts(q["stats"]) == _counts(ref["stats"])
    assert np.array_equal(q["t"], ref["t"]) and ddt <= CA.DT0_FLOOR and du <= 1e-5
    # the recorded Adams forward and the pullback over its Hermite record
    # (yardstick 4: the forward bit for bit — the norms' fp64 sums are regrouped by rank, their float32 results are not moved)
    assert q["stats_fwd"] == ref["stats_fwd"] and q["t1"] == ref["t1"] and q["nfe"] == ref["nfe"]
    assert q["reg_val"] == ref["reg_val"] and q["reg_val"] > 0, (tag, q["reg_val"], ref["reg_val"])
    assert np.array_equal(ue, SC.np_(ref["u_end"])), "the recorded Adams forward's u_end differs from the unsharded run"
    _yardstick4(tag, q, ref, dx)


def test_adams_rejecting_solve_on_shards_keeps_the_ranks_together(gpu_pkg):
    """V1, 3 x 7, scale 10, tol 1e-3, vcab3 (the oracle: 134 accepted, 1 rejected; asserted in the host test).  At that
    stiffness the oracle's own gradient is 0.6 away from float64, so nothing is compared across implementations: yardstick 1
    on stats and every trace row, retcode 0 and a rejected attempt on the GPU.  Measured: 134 accepted, 1 rejected, nf 142 on every rank — the oracle's counts."""
    P = gpu_pkg
    c = SC.ADAMS_REJECT
    nranks, _ = SC.GROUPS[c["B"]]
    model, p, x = SC.inputs(P, c["shape"], c["B"], scale=c["scale"])
    with SC.group(P, model, p, nranks) as hs:
        for h in hs:
            h.set_solver(c["solver"])
        xs = SC.dev_shards(x, nranks)
        got = SC.on_ranks(P, hs, lambda r, h: h.solve(xs[r], 0.0, 1.0, c["tol"], c["tol"], saveat=[1.0], maxiters=10000, trace=True))
    print(f"{c['solver']} rejecting case on {nranks} ranks: {got[0]['stats']}")
    _yardstick1("adams reject", got, keys=("stats", "trace", "t", "retcode"))
    assert got[0]["retcode"] == 0 and got[0]["stats"]["retcode"] == 0 and got[0]["stats"]["nreject"] >= 1
    assert len(got[0]["trace"]) == got[0]["stats"]["naccept"] + got[0]["stats"]["nreject"]


# ---- 6. the fused forward + head on shards ----------------------------------------------------------------------------
def _ce_runs(h, x, pc, K, lab, tol):
    fw, hd = h.node_forward_record_ce(x, 0.0, 1.0, tol, tol, pc, K, lab, mode="unbiased", t1_or_rand=0.43, maxiters=10000)
    bw, rows = SC.traced(h, lambda: h.node_backward_recorded(hd["du"], 2.5))
    bw.update(rows=rows, reg_val=fw["reg_val"], t1=fw["t1"], nfe=fw["nfe"], stats_fwd=fw["stats"], u_end=fw["u_end"],
              loss=hd["loss"], logits=hd["logits"], du=hd["du"], dpc=hd["dpc"], kind=h.last_adjoint_info()["kind"])
    return bw


@pytest.mark.parametrize("K", [10, 7])
@pytest.mark.parametrize("shape,B", [("Q", 34), ("V1", 21)])
def test_fused_forward_and_head_on_shards(gpu_pkg, plain, shape, B, K):
    """lrnde_node_forward_record_ce (the head's two collectives issued from inside the solve's tail; K = 10 the compile-time
    form of the head, K = 7 the runtime one) and lrnde_node_backward_recorded of the head's du with w_reg 2.5, :unbiased, on
    2 x 17 and 3 x 7 samples (scale 3, tol 1e-4).  Yardstick 1 on the loss, dpc, the forward's scalars and the adjoint; against
    the unsharded handle's same two calls: u_end bit for bit, the ranks' logits blocks 1e-6, loss 2e-6, dpc 1e-5, stacked du
    1e-6 (test_sharded_backward_and_training_step's bars), dx / dp by yardstick 4.  Measured: loss, logits and du EQUAL the unsharded handle's on all four cases, dpc 1e-7 apart; the pullback takes its
    step counts (8 on Q, 10 on V1), first-row dt equal, EEst 3e-4 .. 5e-4 (Q) and 4e-6 .. 9e-6 (V1) apart, dx / dp 3e-6 (Q)
    and 2.8e-5 / 1.6e-5 (V1) apart."""
    import torch
    P = gpu_pkg
    D, _H = SC.SHAPES[shape]
    nranks, _ = SC.GROUPS[B]
    tol = 1e-4
    model, p, x = SC.inputs(P, shape, B, scale=3.0)
    rng = np.random.default_rng(7)
    pc = torch.from_numpy((rng.random(K * (D + 1), dtype=np.float32) - np.float32(0.5)) * np.float32(0.1)).cuda()
    labels = rng.integers(0, K, B).astype(np.int32)
    hu = plain(model, p)
    ref = _ce_runs(hu, torch.from_numpy(x).cuda(), pc, K, torch.from_numpy(labels).cuda(), tol)
    with SC.group(P, model, p, nranks) as hs:
        xs, ls = SC.dev_shards(x, nranks), SC.dev_shards(labels, nranks)
        got = SC.on_ranks(P, hs, lambda r, h: _ce_runs(h, xs[r], pc, K, ls[r], tol))
        stack = lambda k: np.concatenate([SC.np_(q[k]) for q in got], axis=0)
        dx, du, ue, lg = stack("dx"), stack("du"), stack("u_end"), stack("logits")
    tag = f"{shape} {nranks} x {B // nranks} K={K}"
    _yardstick1(tag, got, keys=("loss", "dpc", "stats_fwd", "reg_val", "t1", "nfe", "stats_bwd", "rows", "dp"))
    _loops(tag, got, ref, shape)
    q = got[0]
    assert q["stats_fwd"] == ref["stats_fwd"] and q["reg_val"] == ref["reg_val"] and q["t1"] == ref["t1"] and q["nfe"] == ref["nfe"]
    assert np.array_equal(ue, SC.np_(ref["u_end"]))
    dl = abs(float(q["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    dlg, dpc, ddu = SC.rel(lg, SC.np_(ref["logits"])), SC.rel(SC.np_(q["dpc"]), SC.np_(ref["dpc"])), SC.rel(du, SC.np_(ref["du"]))
    print(f"{tag}: loss {dl:.2e} (bar 2e-6) logits {dlg:.2e} (1e-6) dpc {dpc:.2e} (1e-5) du {ddu:.2e} (1e-6)")
    assert dl <= 2e-6 and dlg < 1e-6 and dpc < 1e-5 and ddu < 1e-6
    _yardstick4(tag, q, ref, dx)


# ---- 7. one RCCL rank -------------------------------------------------------------------------------------------------
def test_timeseries_pullback_and_adams_on_one_rccl_rank(gpu_pkg, plain, monkeypatch):
    """LRNDE_FORCE_COMM: the sharded code on one rank with ncclAllReduce itself as the transport (Q, B = 24) — the only place
    it carries the time-series pullback's and the Adams solve's traffic.  Yardstick 4 against a plain handle; the Adams
    solve as in test_adams_on_shards.  Measured: every trace row, dx and dp EQUAL the plain handle's (the sharded host loop with its rank slots and
    n_lam * nranks + P count against the device-controlled loop, bit for bit), and so are the vcab3 solve's counts (57, 0, 64),
    first dt and saved states."""
    import torch
    import chain_adjoint_np as CA
    P = gpu_pkg
    B, tol, times = 24, SC.TS_TOL, list(SC.TS_TIMES)
    model, p, x = SC.inputs(P, "Q", B, scale=SC.TS_SCALE)
    cots = SC.ts_cotangents(B, SC.SHAPES["Q"][0])
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(cots).cuda()
    hp = plain(model, p)
    monkeypatch.setenv("LRNDE_FORCE_COMM", "1")
    hc = plain(model, p)
    P.init_comm(hc, 0, 1)
    assert hc.comm_count() == (1, 1) and hp.comm_count() == (1, 0)
    ref = _ts_forward_backward(hp, xd, cd, times, tol, False)
    got = _ts_forward_backward(hc, xd, cd, times, tol, False)
    assert got["kind"] == 0 and ref["kind"] == 1, "a handle with a communicator takes the host-controlled loop"
    assert torch.equal(got["u"], ref["u"]) and got["stats_fwd"] == ref["stats_fwd"] and np.array_equal(got["t"], ref["t"])
    sb = got["stats_bwd"]
    assert sb["nf"] == 3 + 6 * len(got["rows"]) + 1
    _yardstick4("one RCCL rank, time series", got, ref, SC.np_(got["dx"]))
    sv = [0.37, 1.0]
    hp.set_solver("vcab3"); hc.set_solver("vcab3")
    a = hp.solve(xd, 0.0, 1.0, tol, tol, saveat=sv, maxiters=10000, trace=True)
    b = hc.solve(xd, 0.0, 1.0, tol, tol, saveat=sv, maxiters=10000, trace=True)
    ddt = abs(float(b["trace"]["dt"][0]) - float(a["trace"]["dt"][0])) / float(a["trace"]["dt"][0])
    du = float(np.abs(SC.np_(b["u"]) - SC.np_(a["u"])).max() / np.abs(SC.np_(a["u"])).max())
    print(f"one RCCL rank, vcab3: counts {_counts(b['stats'])} / plain {_counts(a['stats'])}, first dt {ddt:.2e}, saved states {du:.2e} of scale")
    assert b["retcode"] == 0 and _counts(b["stats"]) == _counts(a["stats"]) and ddt <= CA.DT0_FLOOR and du <= 1e-5
