"""The Dense-chain handle's device-controlled continuous adjoint (csrc/lrnde_chain_adjoint.hpp).

Yardstick for gradients: float64 torch autograd through a fine RK4 integration (test_gpu_chain.py's reference_grads,
restated here with `nsteps` and a cotangent at t0), bound 3e-4 of each gradient's norm at tol 1e-6 — the bound
test_physionet_series_pullback_vs_float64_autograd and test_td3_end_state_pullback_vs_float64_autograd hold the same
quantities to.  The yardstick's own error for the 49-time series is measured on the CPU in tests/test_host_chain_adjoint.py.

Fixed launches of a reversed solve besides the 2 per attempted step (LAUNCH_C): 1 k_chadj_begin (the series here have
at most 64 saved times), 4 for initdt (two evaluations, each a step-family and a mu-family launch), 2 for the launch pair
whose prologue reports the end, 1 k_adj_out, and at most 2 k_axpy for cotangents at the solve's two end points."""
import numpy as np
import pytest
import torch

from test_gpu_chain import mk, physionet, rel, shapes, torch_field

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
