"""The Dense-chain handle's device-controlled continuous adjoint (csrc/lrnde_chain_adjoint.hpp).

Yardstick for gradients: float64 torch autograd through a fine RK4 integration (test_gpu_chain.py's reference_grads,
restated here with `nsteps` and a cotangent at t0), bound 3e-4 of each gradient's norm at tol 1e-6 — the bound
test_physionet_series_pullback_vs_float64_autograd and test_td3_end_state_pullback_vs_float64_autograd hold the same
quantities to.  The yardstick's own error for the 49-time series is measured on the CPU in tests/test_host_chain_adjoint.py.

Second yardstick (sections 9-13): the float64 restatement of the whole pullback, tests/chain_adjoint_np.py, pinned on the
CPU against the RK4 yardstick to 3e-7 .. 8e-7 (tests/test_host_chain_adjoint.py).  Both adjoint loops are held to it: the
reversed solve's steps attempt by attempt on inputs where the error estimate is truncation (CA.PINNED), dx / dp and the
regulariser's gradient at max(1e-5, 4 x the distance of the float32 restatement from the float64 one), and the two loops
to each other bit for bit.

Fixed launches of a reversed solve besides the 2 per attempted step (LAUNCH_C): 1 k_chadj_begin (one more per further
64 saved times: test_80_saved_times_take_two_begin_launches_and_the_serial_tstop_scan), 4 for initdt (two evaluations, each a step-family and a mu-family launch), 2 for the launch pair
whose prologue reports the end, 1 k_adj_out, and at most 2 k_axpy for cotangents at the solve's two end points."""
import numpy as np
import pytest
import torch

import chain_adjoint_np as CA
from test_gpu_chain import ODD, mk, physionet, rel, shapes, torch_field

pytestmark = pytest.mark.gpu

LAUNCH_C = 10
TOL = 1e-6


def reference_grads(model, p, x, times, cots, nsteps=200):
    """float64 autograd through RK4 on [0, 1]; a time 0.0 in `times` takes its cotangent at the initial state"""
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    f = torch_field(model, pt)
    h = 1.0 / nsteps
    u, loss = xt, 0.0
    marks = {int(round(t * nsteps)): i for i, t in enumerate(times)}
    assert len(marks) == len(times) and all(abs(k / nsteps - t) < 1e-12 for k, t in zip(sorted(marks), sorted(times)))
    if 0 in marks:
        loss = loss + (u * torch.tensor(cots[marks[0]], dtype=torch.float64)).sum()
    for k in range(nsteps):
        t = k * h
        k1 = f(u, t); k2 = f(u + 0.5 * h * k1, t + 0.5 * h); k3 = f(u + 0.5 * h * k2, t + 0.5 * h); k4 = f(u + h * k3, t + h)
        u = u + (h / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)
        if k + 1 in marks:
            loss = loss + (u * torch.tensor(cots[marks[k + 1]], dtype=torch.float64)).sum()
    loss.backward()
    return xt.grad.numpy(), pt.grad.numpy()


@pytest.fixture
def host_loop(gpu_pkg):
    """switches LRNDE_ADJ_HOST on for the calls made through it, and off again afterwards"""
    class Ctx:
        def __enter__(self):
            gpu_pkg.set_option("LRNDE_ADJ_HOST", 1)

        def __exit__(self, *a):
            gpu_pkg.set_option("LRNDE_ADJ_HOST", 0)
    yield Ctx()
    gpu_pkg.set_option("LRNDE_ADJ_HOST", 0)


def make_node(P, model, regularize="unbiased", times=None, save_start=False, maxiters=10000, tol=TOL):
    kw = dict(regularize=regularize, abstol=tol, reltol=tol, maxiters=maxiters, field="dense_chain")
    if times is not None:
        kw.update(saveat=list(times), save_start=save_start)
    return P.NeuralODE(model, **kw)


def run(node, x, p, cots, seed=3, w_reg=0.0):
    st = node.initialstates(np.random.default_rng(seed))
    xd, ps = torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()
    dx, dp, info = node.pullback(xd, ps, st, torch.from_numpy(np.asarray(cots, np.float32)).cuda(), w_reg=w_reg)
    ai = node.handle(xd).last_adjoint_info()
    return dx.cpu().numpy(), dp.cpu().numpy(), info, ai


def n_inside(times):
    return sum(1 for t in times if 0.0 < t < 1.0)


def check_identity(info, times):
    sb = info["stats_bwd"]
    assert sb["nf"] == 3 + 6 * (sb["naccept"] + sb["nreject"]) + n_inside(times), (sb, times)


# ---- 1. which loop ran, launches, host waits ----------------------------------------------------------------------
@pytest.mark.parametrize("B", [12, 512])
def test_loop_kind_launches_and_host_waits(gpu_pkg, host_loop, B):
    P = gpu_pkg
    model = physionet(P)
    h, p, x = mk(P, model, B, scale=1.5)
    times = [0.25, 0.5, 1.0]
    cots = np.random.default_rng(11).standard_normal((3, B, 20)).astype(np.float32)
    node = make_node(P, model, times=times)
    _, _, info, ai = run(node, x, p, cots)
    sb = info["stats_bwd"]
    print(f"B={B} device loop: {ai} naccept {sb['naccept']} nreject {sb['nreject']}")
    assert ai["kind"] == 2 and info["adjoint_loop"] == "chain_device"
    assert ai["host_waits"] == 0
    assert ai["launches"] <= 2 * (sb["naccept"] + sb["nreject"]) + LAUNCH_C
    with host_loop:
        _, _, info_h, ai_h = run(node, x, p, cots)
    print(f"B={B} host loop: {ai_h} naccept {info_h['stats_bwd']['naccept']}")
    assert ai_h["kind"] == 0 and info_h["adjoint_loop"] == "host"
    assert ai_h["host_waits"] >= info_h["stats_bwd"]["naccept"]


def test_mlp_handle_reports_its_device_loop(gpu_pkg):
    P = gpu_pkg
    D, H, B = 32, 64, 40
    model = P.TDChain(P.Chain(P.Dense(D + 1, H, "tanh"), P.Dense(H + 1, D)))
    p = P.glorot_params(model, seed=5)
    x = np.random.default_rng(2).random((B, D), dtype=np.float32)
    node = P.NeuralODE(model, regularize="unbiased", abstol=1e-6, reltol=1e-6)
    st = node.initialstates(np.random.default_rng(0))
    xd = torch.from_numpy(x).cuda()
    cot = torch.from_numpy(np.random.default_rng(9).standard_normal((B, D)).astype(np.float32)).cuda()
    _, _, info = node.pullback(xd, torch.from_numpy(p).cuda(), st, cot)
    ai = node.handle(xd).last_adjoint_info()
    assert ai["kind"] == 1 and info["adjoint_loop"] == "device" and ai["launches"] > 0 and ai["host_waits"] == 0


# ---- 2. gradients against float64 autograd ---------------------------------------------------------------------
@pytest.mark.parametrize("regularize", ["none", "unbiased", "biased"])
@pytest.mark.parametrize("B", [1, 12, 37, 512])
def test_physionet_series_vs_float64_autograd(gpu_pkg, regularize, B):
    P = gpu_pkg
    model = physionet(P)
    h, p, x = mk(P, model, B, scale=1.5)
    times = [0.25, 0.5, 1.0]
    cots = np.random.default_rng(11).standard_normal((3, B, 20)).astype(np.float32)
    dx, dp, info, ai = run(make_node(P, model, regularize, times), x, p, cots)
    gx, gp = reference_grads(model, p, x, times, cots)
    print(f"{regularize} B={B}: dx rel {rel(dx, gx):.2e} dp rel {rel(dp, gp):.2e} {ai}")
    assert ai["kind"] == 2
    assert rel(dx, gx) < 3e-4 and rel(dp, gp) < 3e-4
    check_identity(info, times)


@pytest.mark.parametrize("name", ["td3_tanh", "td3_gelu"])
def test_td3_end_state_vs_float64_autograd(gpu_pkg, name):
    P = gpu_pkg
    model = shapes(P)[name]
    h, p, x = mk(P, model, 9, scale=1.5)
    cot = np.random.default_rng(12).standard_normal((9, 32)).astype(np.float32)
    dx, dp, info, ai = run(make_node(P, model), x, p, cot, seed=5)
    gx, gp = reference_grads(model, p, x, [1.0], [cot])
    print(f"{name}: dx rel {rel(dx, gx):.2e} dp rel {rel(dp, gp):.2e} {ai}")
    assert ai["kind"] == 2
    assert rel(dx, gx) < 3e-4 and rel(dp, gp) < 3e-4
    check_identity(info, [1.0])


@pytest.mark.parametrize("B,nsteps", [(12, 196), (512, 245)])
def test_49_time_series_vs_float64_autograd(gpu_pkg, B, nsteps):
    P = gpu_pkg
    model = physionet(P)
    h, p, x = mk(P, model, B, scale=1.5)
    times = [(i + 1) / 49.0 for i in range(49)]
    cots = np.random.default_rng(13).standard_normal((49, B, 20)).astype(np.float32)
    dx, dp, info, ai = run(make_node(P, model, "unbiased", times), x, p, cots)
    gx, gp = reference_grads(model, p, x, times, cots, nsteps=nsteps)
    sb = info["stats_bwd"]
    print(f"49 times B={B}: dx rel {rel(dx, gx):.2e} dp rel {rel(dp, gp):.2e} {ai} naccept {sb['naccept']} nreject {sb['nreject']}")
    assert ai["kind"] == 2 and ai["host_waits"] == 0
    assert ai["launches"] <= 2 * (sb["naccept"] + sb["nreject"]) + LAUNCH_C
    assert rel(dx, gx) < 3e-4 and rel(dp, gp) < 3e-4
    check_identity(info, times)


def test_series_with_the_start_time_and_save_start(gpu_pkg):
    """the impulse at the solve's end (t0)"""
    P = gpu_pkg
    model = physionet(P)
    B = 12
    h, p, x = mk(P, model, B, scale=1.5)
    times = [0.0, 0.5, 1.0]
    node = make_node(P, model, "unbiased", times, save_start=True)
    st = node.initialstates(np.random.default_rng(3))
    sol, _ = node(torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda(), st)
    assert [float(t) for t in sol.t] == times
    cots = np.random.default_rng(14).standard_normal((3, B, 20)).astype(np.float32)
    dx, dp, info, ai = run(node, x, p, cots)
    gx, gp = reference_grads(model, p, x, times, cots)
    print(f"series with t0: dx rel {rel(dx, gx):.2e} dp rel {rel(dp, gp):.2e} {ai}")
    assert ai["kind"] == 2
    assert rel(dx, gx) < 3e-4 and rel(dp, gp) < 3e-4
    check_identity(info, times)


def test_cotangent_at_t2_only_through_the_series_form(gpu_pkg):
    P = gpu_pkg
    model = physionet(P)
    B = 12
    h, p, x = mk(P, model, B, scale=1.5)
    times = [0.25, 0.5, 1.0]
    cots = np.zeros((3, B, 20), np.float32)
    cots[2] = np.random.default_rng(15).standard_normal((B, 20)).astype(np.float32)
    dx, dp, info, ai = run(make_node(P, model, "unbiased", times), x, p, cots)
    gx, gp = reference_grads(model, p, x, [1.0], [cots[2]])
    print(f"t2 only: dx rel {rel(dx, gx):.2e} dp rel {rel(dp, gp):.2e}")
    assert ai["kind"] == 2
    assert rel(dx, gx) < 3e-4 and rel(dp, gp) < 3e-4
    check_identity(info, times)


# ---- 3. both loops on the same inputs ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,ntimes", [(12, 3), (512, 3), (512, 49)])
def test_device_and_host_loop_on_the_same_inputs(gpu_pkg, host_loop, B, ntimes):
    P = gpu_pkg
    model = physionet(P)
    h, p, x = mk(P, model, B, scale=1.5)
    times = [0.25, 0.5, 1.0] if ntimes == 3 else [(i + 1) / 49.0 for i in range(49)]
    cots = np.random.default_rng(16).standard_normal((ntimes, B, 20)).astype(np.float32)
    node = make_node(P, model, "unbiased", times)
    dx, dp, info, ai = run(node, x, p, cots)
    with host_loop:
        dxh, dph, infoh, aih = run(node, x, p, cots)
    assert ai["kind"] == 2 and aih["kind"] == 0
    gx, gp = reference_grads(model, p, x, times, cots, nsteps=200 if ntimes == 3 else 196)
    cnt = lambda i: (i["stats_bwd"]["naccept"], i["stats_bwd"]["nreject"], i["stats_bwd"]["nf"])
    print(f"B={B} {ntimes} times: rel(device, host) dx {rel(dx, dxh):.2e} dp {rel(dp, dph):.2e}; "
          f"device (naccept, nreject, nf) {cnt(info)} host {cnt(infoh)}; "
          f"vs float64: device dx {rel(dx, gx):.2e} dp {rel(dp, gp):.2e}, host dx {rel(dxh, gx):.2e} dp {rel(dph, gp):.2e}")
    assert rel(dx, gx) < 3e-4 and rel(dp, gp) < 3e-4
    assert rel(dxh, gx) < 3e-4 and rel(dph, gp) < 3e-4
    check_identity(info, times)
    check_identity(infoh, times)
    # the summation orders give the two loops the same bits
    assert cnt(info) == cnt(infoh)
    assert np.array_equal(dx, dxh) and np.array_equal(dp, dph)


# ---- 4. determinism -------------------------------------------------------------------------------------------
def test_two_pullbacks_give_the_same_bits(gpu_pkg):
    P = gpu_pkg
    model = physionet(P)
    h, p, x = mk(P, model, 512)
    times = [(i + 1) / 49.0 for i in range(49)]
    cots = np.random.default_rng(17).standard_normal((49, 512, 20)).astype(np.float32)
    node = make_node(P, model, "unbiased", times)
    a, b = run(node, x, p, cots, w_reg=2.0), run(node, x, p, cots, w_reg=2.0)
    assert a[3]["kind"] == 2
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[2]["stats_bwd"] == b[2]["stats_bwd"] and a[3] == b[3]


# ---- 5. regulariser --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regularize", ["unbiased", "biased"])
def test_regulariser_gradient_rides_on_the_device_loop(gpu_pkg, host_loop, regularize):
    P = gpu_pkg
    model = physionet(P)
    B = 12
    h, p, x = mk(P, model, B, scale=1.5)
    times = [0.25, 0.5, 1.0]
    cots = np.random.default_rng(11).standard_normal((3, B, 20)).astype(np.float32)
    node = make_node(P, model, regularize, times)
    st = node.initialstates(np.random.default_rng(3))
    sol, st2 = node(torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda(), st)
    dx0, dp0, _, ai0 = run(node, x, p, cots, w_reg=0.0)
    dxr, dpr, infr, air = run(node, x, p, cots, w_reg=3.0)
    assert ai0["kind"] == 2 and air["kind"] == 2 and air["host_waits"] == 0
    assert infr["reg_val"] == st2["reg_val"] and infr["reg_val"] > 0
    assert rel(dxr, dx0) < 1e-5   # the regulariser has no gradient to x
    assert not np.array_equal(dpr, dp0) and np.isfinite(dpr).all()
    with host_loop:
        _, dp0h, _, _ = run(node, x, p, cots, w_reg=0.0)
        _, dprh, _, aih = run(node, x, p, cots, w_reg=3.0)
    assert aih["kind"] == 0
    d, dh = dpr.astype(np.float64) - dp0, dprh.astype(np.float64) - dp0h
    print(f"{regularize}: rel(dp(w_reg) - dp(0), device vs host) {rel(d, dh):.2e}")
    assert rel(d, dh) < 3e-4


# ---- 6. status paths --------------------------------------------------------------------------------------------
def test_maxiters_status_and_recovery(gpu_pkg, host_loop):
    P = gpu_pkg
    model = physionet(P)
    B = 12
    h, p, x = mk(P, model, B, scale=1.5)
    xd = torch.from_numpy(x).cuda()
    times = [0.25, 0.5, 1.0]
    cots = torch.from_numpy(np.random.default_rng(11).standard_normal((3, B, 20)).astype(np.float32)).cuda()

    errs = []
    for use_host in (False, True):
        # the backward takes maxiters from the record: a loose forward without tstops fits 3 attempts (initdt's step, then
        # two that may each grow tenfold), the adjoint on [lambda; mu] does not
        fw = h.node_forward_record(xd, 0.0, 1.0, 1e-1, 1e-1, mode="none", maxiters=3)
        assert fw["stats"]["retcode"] == 0
        try:
            if use_host:
                with host_loop:
                    h.node_backward_recorded(cots[2])
            else:
                h.node_backward_recorded(cots[2])
            errs.append(None)
        except RuntimeError as e:
            errs.append(str(e))
        errs.append(h.last_adjoint_info()["kind"])
    print("maxiters=3:", errs)
    assert errs[1] == 2 and errs[3] == 0
    assert errs[0] is not None and errs[2] is not None
    assert "MaxIters" in errs[0] and "adjoint solve stopped with retcode" in errs[0]
    assert errs[0] == errs[2]
    # the handle goes on: a sane pullback afterwards, twice, same bits
    outs = []
    for _ in range(2):
        h.node_forward_record_ts(xd, 0.0, 1.0, TOL, TOL, times, mode="none", maxiters=10000)
        outs.append(h.node_backward_recorded_ts(cots))
    assert h.last_adjoint_info()["kind"] == 2
    assert torch.equal(outs[0]["dx"], outs[1]["dx"]) and torch.equal(outs[0]["dp"], outs[1]["dp"])
    assert outs[0]["stats_bwd"] == outs[1]["stats_bwd"] and outs[0]["stats_bwd"]["retcode"] == 0
    gx, gp = reference_grads(model, p, x, times, cots.cpu().numpy())
    assert rel(outs[0]["dx"].cpu().numpy(), gx) < 3e-4 and rel(outs[0]["dp"].cpu().numpy(), gp) < 3e-4


def test_stale_record_is_still_detected(gpu_pkg):
    P = gpu_pkg
    model = physionet(P)
    B = 12
    h, p, x = mk(P, model, B)
    xd = torch.from_numpy(x).cuda()
    cot = torch.from_numpy(np.random.default_rng(1).standard_normal((B, 20)).astype(np.float32)).cuda()
    assert h.record_generation() == 0
    h.node_forward_record(xd, 0.0, 1.0, TOL, TOL, mode="none")
    g1 = h.record_generation()
    h.node_forward_record(xd * 0.5, 0.0, 1.0, TOL, TOL, mode="none")
    assert h.record_generation() == g1 + 1
    h.node_backward_recorded(cot)
    assert h.last_adjoint_info()["kind"] == 2
    assert h.record_generation() == 0   # consumed
    with pytest.raises(RuntimeError):
        h.node_backward_recorded(cot)


# ---- 7. outside the gate ---------------------------------------------------------------------------------------
def test_chain_outside_the_gate_takes_the_host_loop(gpu_pkg):
    """16 layers of width 42: forward image 118 KB + activation record 53 KB exceed the 160 KB of LDS the step kernel may use"""
    P = gpu_pkg
    model = P.Chain(P.Activation("tanh"), *[P.Dense(42, 42, "tanh") for _ in range(16)])
    B = 9
    h, p, x = mk(P, model, B)
    cot = np.random.default_rng(18).standard_normal((B, 42)).astype(np.float32)
    dx, dp, info, ai = run(make_node(P, model), x, p, cot)
    gx, gp = reference_grads(model, p, x, [1.0], [cot])
    print(f"outside the gate: {ai} dx rel {rel(dx, gx):.2e} dp rel {rel(dp, gp):.2e}")
    assert ai["kind"] == 0 and info["adjoint_loop"] == "host"
    assert rel(dx, gx) < 3e-4 and rel(dp, gp) < 3e-4


# ---- 8. trace hook ---------------------------------------------------------------------------------------------
def test_trace_rows_of_the_device_loop(gpu_pkg):
    P = gpu_pkg
    model = physionet(P)
    B = 37
    h, p, x = mk(P, model, B, scale=1.5)
    xd = torch.from_numpy(x).cuda()
    times = [0.25, 0.5, 1.0]
    cots = torch.from_numpy(np.random.default_rng(11).standard_normal((3, B, 20)).astype(np.float32)).cuda()
    h.node_forward_record_ts(xd, 0.0, 1.0, TOL, TOL, times, mode="none", maxiters=10000)
    h.set_adjoint_trace(4096)
    bw = h.node_backward_recorded_ts(cots)
    rows = h.adjoint_trace()
    h.set_adjoint_trace(0)
    sb = bw["stats_bwd"]
    assert h.last_adjoint_info()["kind"] == 2
    assert len(rows) == sb["naccept"] + sb["nreject"]
    ts = [r[0] for r in rows]
    assert all(b >= a for a, b in zip(ts, ts[1:])) and ts[0] == -1.0
    assert sum(1 for r in rows if r[3] == 1) == sb["naccept"]
    ends = [np.float32(r[0]) + np.float32(r[1]) for r in rows if r[3] == 1]
    for t in times:
        if 0.0 < t < 1.0:   # up to the controller's tstop snap: 100 eps of the time's magnitude
            assert any(abs(float(e) + t) <= 100 * np.finfo(np.float32).eps * t for e in ends), (t, ends)


# ---- 9. both loops against the float64 restatement of the pullback (tests/chain_adjoint_np.py) --------------------
MARGIN = CA.MARGIN   # (the row bounds: CA.check_rows)


def handle_for(P, model, p):
    from localregneuralde_jl_amd.layers import Handle, _chain_desc
    h = Handle(_chain_desc(model))
    h.set_params(torch.from_numpy(p))
    return h


def run_ts(h, x, times, cots, tol, mode="none", reg_type="error_estimate", t1_or_rand=0.43, w_reg=0.0, save_start=False):
    """recorded forward + pullback through the handle-level entry points, with the trace of the reversed solve"""
    xd = torch.from_numpy(x).cuda()
    fw = h.node_forward_record_ts(xd, 0.0, 1.0, tol, tol, times, mode=mode, reg_type=reg_type, t1_or_rand=t1_or_rand,
                                  maxiters=10000, save_start=save_start)
    h.set_adjoint_trace(16384)
    bw = h.node_backward_recorded_ts(torch.from_numpy(np.asarray(cots, np.float32)).cuda(), w_reg=w_reg)
    rows = h.adjoint_trace()
    h.set_adjoint_trace(0)
    sb = bw["stats_bwd"]
    return dict(dx=bw["dx"].cpu().numpy(), dp=bw["dp"].cpu().numpy(), counts=(sb["naccept"], sb["nreject"], sb["nf"]), rows=rows,
                reg_val=float(fw["reg_val"]), t1=float(fw["t1"]), ai=h.last_adjoint_info(),
                fwd=(fw["stats"]["naccept"], fw["stats"]["nreject"]))


def on_both_loops(host_loop, fn):
    """[(loop name, result)]: fn() on the device loop and again under LRNDE_ADJ_HOST=1, the loop kind asserted"""
    dev = fn()
    assert dev["ai"]["kind"] == 2, dev["ai"]
    with host_loop:
        host = fn()
    assert host["ai"]["kind"] == 0, host["ai"]
    return [("device loop (kind 2)", dev), ("host loop (kind 0)", host)]


def check_grads(tag, got, r64, r32):
    for key in ("dx", "dp"):
        bound = max(1e-5, MARGIN * rel(r32[key], r64[key]))
        e = rel(got[key], r64[key])
        print(f"{tag}: rel({key}, float64 restatement) {e:.2e} bound {bound:.2e}")
        assert e <= bound, (tag, key, e, bound)


def check_same_bits(res):
    (_, dev), (_, host) = res
    print(f"device vs host loop: counts {dev['counts']} / {host['counts']}, rel dx {rel(dev['dx'], host['dx']):.2e} dp {rel(dev['dp'], host['dp']):.2e}")
    assert dev["counts"] == host["counts"]
    assert np.array_equal(dev["dx"], host["dx"]) and np.array_equal(dev["dp"], host["dp"])


@pytest.mark.parametrize("name", list(CA.PINNED))
def test_steps_and_gradients_of_both_loops_vs_the_restatement(gpu_pkg, host_loop, name):
    """Every attempted step of the reversed solve against the restatement's: equal (naccept, nreject, nf) and accept
    pattern; s, dt, EEst within max(floor, 4 |row32 - row64|) (CA.check_rows).  The inputs and how they were selected
    on the CPU: CA.PINNED.  The impulse case has a rejected attempt directly after the impulse at s = -0.5 (asserted on
    the CPU and again here).  Measured on the MI355X (both loops, same bits): worst |row - row64| / bound over
    the three inputs s 0.35, dt 0.57, EEst 0.50; rel(dx), rel(dp) 5.0e-6 .. 5.5e-5 at bounds 1.2e-5 .. 1.8e-4."""
    P = gpu_pkg
    model, p, x, times, cots, tol = CA.pinned_inputs(P, name)
    r64 = CA.pullback(model, p, x, times, cots, tol)
    r32 = CA.pullback(model, p, x, times, cots, tol, dtype=np.float32)
    h = handle_for(P, model, p)
    res = on_both_loops(host_loop, lambda: run_ts(h, x, times, cots, tol))
    for loop, got in res:
        tag = f"{name} {loop}"
        assert got["fwd"] == r64["fwd"], (tag, got["fwd"], r64["fwd"])
        CA.check_rows(tag, got, r64, r32)
        check_grads(tag, got, r64, r32)
        if CA.PINNED[name]["rejects"]:
            assert got["counts"][1] >= 1
            at_imp = [r for r in got["rows"] if r[0] == -0.5]
            assert len(at_imp) >= 2 and at_imp[0][3] == 0, at_imp
    check_same_bits(res)


@pytest.mark.parametrize("case", ["3_times", "49_times", "with_t0"])
def test_physionet_gradients_of_both_loops_vs_the_restatement(gpu_pkg, host_loop, case):
    """PhysioNet at tol 1e-6: the estimate is rounding of the parameter-cotangent sums there (the two restatements take
    different step counts), so steps are not compared; the gradients are"""
    P = gpu_pkg
    model = physionet(P)
    h, p, x = mk(P, model, 12, scale=1.5)
    times = {"3_times": [0.25, 0.5, 1.0], "49_times": [(i + 1) / 49.0 for i in range(49)], "with_t0": [0.0, 0.5, 1.0]}[case]
    cots = np.random.default_rng(13).standard_normal((len(times), 12, 20)).astype(np.float32)
    kw = dict(mode="unbiased", t1_or_rand=0.43, save_start=(case == "with_t0"))
    r64 = CA.pullback(model, p, x, times, cots, TOL, want_reg=False, **kw)
    r32 = CA.pullback(model, p, x, times, cots, TOL, want_reg=False, dtype=np.float32, **kw)
    res = on_both_loops(host_loop, lambda: run_ts(h, x, times, cots, TOL, **kw))
    for loop, got in res:
        print(f"{case} {loop}: counts {got['counts']} restatement {r64['counts']} / float32 {r32['counts']}")
        check_grads(f"{case} {loop}", got, r64, r32)
        assert got["counts"][2] == 3 + 6 * (got["counts"][0] + got["counts"][1]) + n_inside(times)
    check_same_bits(res)


# ---- 10. the regulariser's gradient through a chain pullback --------------------------------------------------------
@pytest.mark.parametrize("reg_type", ["error_estimate", "stiffness_estimate"])
@pytest.mark.parametrize("mode", ["unbiased", "biased"])
def test_regulariser_value_and_gradient_vs_the_restatement(gpu_pkg, host_loop, mode, reg_type):
    """sol(t1) from the dense record -> init_dt -> one step -> the reverse sweep -> added to mu's result, against float64
    autograd through the restatement's frozen step (uprev = sol(t1), k1, dt constant).  Inputs and their selection on the
    CPU: CA.REG_CASE.  The cotangents are scaled by 0.01 to keep dp(w_reg = 0) small beside 3 d reg/dp in the float32
    difference dp(3) - dp(0).  Measured on the MI355X (both loops, same bits): reg_val off by
    6.7e-4 / 1.7e-5 (unbiased error / stiffness estimate) and 6.1e-4 / 3.5e-6 (biased) at the 1e-3 bar; gradient rel 1.25e-2 /
    3.4e-4 and 7.2e-3 / 2.3e-4 at bounds 5.2e-2 / 1.2e-3 and 3.3e-2 / 1.1e-3 (error estimate: |dp(0)| = 26 beside
    |3 d reg/dp| = 0.10, so the float32 difference itself carries ~1e-3)."""
    P = gpu_pkg
    model, p, x, times, cots, tol = CA.reg_inputs(P)
    h = handle_for(P, model, p)
    kw = dict(mode=mode, reg_type=reg_type, t1_or_rand=CA.REG_CASE["t1_or_rand"])
    r64 = CA.pullback(model, p, x, times, cots, tol, **kw)
    r32 = CA.pullback(model, p, x, times, cots, tol, dtype=np.float32, **kw)
    bound = max(1e-5, MARGIN * rel(r32["reg_grad"], r64["reg_grad"]))
    for use_host in (False, True):
        outs = []
        for w in (0.0, 3.0):
            if use_host:
                with host_loop:
                    outs.append(run_ts(h, x, times, cots, tol, w_reg=w, **kw))
            else:
                outs.append(run_ts(h, x, times, cots, tol, w_reg=w, **kw))
        g0, g3 = outs
        assert g0["ai"]["kind"] == g3["ai"]["kind"] == (0 if use_host else 2)
        assert g3["t1"] == np.float32(r64["t1"]), (g3["t1"], r64["t1"])
        d = g3["dp"].astype(np.float64) - g0["dp"].astype(np.float64)
        e = rel(d, 3.0 * r64["reg_grad"])
        print(f"{mode} {reg_type} loop kind {g3['ai']['kind']}: t1 {g3['t1']:.4f} reg_val {g3['reg_val']:.6e} restatement {r64['reg_val']:.6e}; "
              f"rel(dp(3) - dp(0), 3 d reg/dp) {e:.2e} bound {bound:.2e}; |dp(0)| {np.linalg.norm(g0['dp']):.3e} |3 d reg/dp| {3 * np.linalg.norm(r64['reg_grad']):.3e}")
        assert abs(g3["reg_val"] - r64["reg_val"]) <= CA.REG_BAR * r64["reg_val"]
        assert np.array_equal(g3["dx"], g0["dx"])   # the regulariser has no gradient to x
        assert e <= bound, (e, bound)


# ---- 11. shapes that reach the branches no other test does ----------------------------------------------------------
def shape_case(P, host_loop, model, B, times, tol=TOL, scale=1.5, launch_c=LAUNCH_C):
    h, p, x = mk(P, model, B, scale=scale)
    D = x.shape[1]
    cots = np.random.default_rng(21).standard_normal((len(times), B, D)).astype(np.float32)
    kw = dict(mode="unbiased", t1_or_rand=0.43)
    r64 = CA.pullback(model, p, x, times, cots, tol, want_reg=False, **kw)
    r32 = CA.pullback(model, p, x, times, cots, tol, want_reg=False, dtype=np.float32, **kw)
    res = on_both_loops(host_loop, lambda: run_ts(h, x, times, cots, tol, **kw))
    for loop, got in res:
        print(f"B={B} D={D} P={p.size} {loop}: {got['ai']} counts {got['counts']} restatement {r64['counts']}")
        check_grads(loop, got, r64, r32)
        assert got["counts"][2] == 3 + 6 * (got["counts"][0] + got["counts"][1]) + n_inside(times)   # (t1 is a tstop without an impulse)
    dev = res[0][1]
    assert dev["ai"]["host_waits"] == 0
    assert dev["ai"]["launches"] <= 2 * (dev["counts"][0] + dev["counts"][1]) + launch_c
    check_same_bits(res)
    return res, p


def test_80_saved_times_take_two_begin_launches_and_the_serial_tstop_scan(gpu_pkg, host_loop):
    """80 saved times (i + 1) / 80 and t1: 80 tstops and 79 impulses inside the span.  k_chadj_begin takes 64 entries of
    each table per launch, so chadj_solve_device launches it twice (LAUNCH_C + 1), and with g.nstops = 80 > 64
    chadj_prologue leaves the one-tstop-per-lane ballot for the serial scan of g.stops"""
    P = gpu_pkg
    times = [(i + 1) / 80.0 for i in range(80)]
    res, _ = shape_case(P, host_loop, physionet(P), 12, times, launch_c=LAUNCH_C + 1)
    assert res[0][1]["ai"]["launches"] > 2 * sum(res[0][1]["counts"][:2]) + 4 + 2 + 1 + 1   # more than one begin launch


def test_backward_image_in_l2_and_two_parameter_chunks_per_mu_block(gpu_pkg, host_loop):
    """Chain(Dense(128, 96, tanh), Dense(96, 128)), by lrnde_create_chain's formulas: forward image (129 x 96 + 97 x 128)
    = 24800 floats = 99.2 KB; activation record ch_vjp_lds = ((128 + 96) + (96 + 128) + 128 + 2 x 128) x 8 floats =
    26.6 KB; the step kernel's LDS without the backward image = 99.2 + 26.6 + 0.4 KB <= 160 KB, so chain_device_gate accepts; the
    backward image is 128 x 96 + 96 x 128 = 24576 floats = 98.3 KB and with it 224 KB > 160 KB: wg_lds = 0, k_chadj_step
    reads W^T from L2.  P = 24800 > 64 x CHADJ_MAX_MU_BLOCKS = 16384: 388 chunks of 64 parameters on 256 blocks, so blocks
    0..131 of k_chadj_mu go round their chunk loop twice."""
    P = gpu_pkg
    from localregneuralde_jl_amd import _lib as L
    model = P.Chain(P.Dense(128, 96, "tanh"), P.Dense(96, 128))
    fwd_image = L.chain_weight_image_bytes([128, 96, 128], False)
    record = ((128 + 96) + (96 + 128) + 128 + 2 * 128) * 8 * 4
    assert fwd_image == 24800 * 4 and fwd_image + record + 1024 <= 160 * 1024 < fwd_image + 24576 * 4 + record
    res, p = shape_case(P, host_loop, model, 12, [0.25, 0.5, 1.0])
    assert p.size == 24800 and p.size > 64 * 256


@pytest.mark.parametrize("B", [100, 65])
def test_slot_sum_with_a_full_group_and_a_tail(gpu_pkg, host_loop, B):
    """B = 100: nwg = 13 = one group of 8 partials and a tail of 5 in chadj_slot_sum, last tile 4 columns; B = 65 = 8 x 8 + 1:
    nwg = 9, tail of 1, and the last tile holds one column"""
    P = gpu_pkg
    shape_case(P, host_loop, physionet(P), B, [0.25, 0.5, 1.0])


@pytest.mark.parametrize("name", ODD)
def test_odd_widths_through_both_loops(gpu_pkg, host_loop, name):
    """odd `out`: chain_layer's second row of a float2 pair is the zero padding of k_pack_chain and is masked by
    o0 + 1 < out; chain_slots maps e % D, e / D with D odd; D = 1 leaves 8 state elements per tile"""
    P = gpu_pkg
    shape_case(P, host_loop, shapes(P)[name], 11, [0.25, 0.5, 1.0])
