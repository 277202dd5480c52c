"""The wide Dense-chain handle's device-controlled continuous adjoint (csrc/lrnde_wide_adjoint.hpp):
opt-in through NeuralODE(adjoint_loop="device") / Handle.set_adjoint_loop("device"), two launches per attempted step, held
to the bits of the host-controlled loop (LRNDE_ADJ_HOST=1 on the same handle and inputs).

Yardsticks for the gradients: the float64 restatement of the whole pullback (tests/chain_adjoint_np.py), bound
max(1e-5, 4 x the distance of its float32 instance from its float64 one), and float64 autograd through RK4
(wide_chain_cases.reference_grads) at 3e-4.  Fixed launches besides the 2 per attempted step: WA.LAUNCH_C."""
import numpy as np
import pytest
import torch

import chain_adjoint_np as CA
import wide_chain_adjoint_cases as WA
import wide_chain_cases as WC

pytestmark = pytest.mark.gpu

TOL = WA.TOL


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


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


def on_both_loops(host_loop, fn):
    dev = fn()
    assert dev["ai"]["kind"] == 3 and dev["ai"]["host_waits"] == 0, dev["ai"]
    with host_loop:
        host = fn()
    assert host["ai"]["kind"] == 0, host["ai"]
    return dev, host


def check_same_bits(tag, dev, host):
    first = next((i for i, (a, b) in enumerate(zip(dev["rows"], host["rows"])) if a != b), None)
    print(f"{tag}: counts {dev['counts']} / {host['counts']} launches {dev['ai']['launches']} / {host['ai']['launches']} "
          f"host waits {host['ai']['host_waits']} rel dx {WC.rel(dev['dx'], host['dx']):.2e} dp {WC.rel(dev['dp'], host['dp']):.2e}"
          + ("" if first is None else f" first differing row {first}: {dev['rows'][first]} / {host['rows'][first]}"))
    assert dev["counts"] == host["counts"]
    assert dev["rows"] == host["rows"]
    assert np.array_equal(dev["dx"], host["dx"]) and np.array_equal(dev["dp"], host["dp"])
    assert dev["ai"]["launches"] <= 2 * (dev["counts"][0] + dev["counts"][1]) + WA.LAUNCH_C + (len(dev["times"]) > 64)


def bits_case(P, host_loop, name, B, times, tol=TOL, scale=1.5, big=None, save_start=False, **kw):
    model = WC.shapes(P)[name]
    p, x = WC.mk_inputs(P, model, B, scale=scale)
    h = WA.handle_for(P, model, p)
    cots = WA.cotangents(times, x, big=big)
    dev, host = on_both_loops(host_loop, lambda: dict(WA.run_ts(h, x, times, cots, tol, save_start=save_start, **kw), times=times))
    check_same_bits(f"{name} B={B} {len(times)} times", dev, host)
    inside = sum(1 for t in times if 0.0 < t < 1.0)   # one K1 re-evaluation per impulse inside the span
    assert dev["counts"][2] == 3 + 6 * (dev["counts"][0] + dev["counts"][1]) + inside
    return dev, host


# ---- 1. which loop ran ----------------------------------------------------------------------------------------------
def test_which_loop_ran(gpu_pkg):
    P = gpu_pkg
    model = WC.shapes(P)["mnist3"]
    B = 33
    p, x = WC.mk_inputs(P, model, B, scale=1.5)
    times = [0.25, 0.5, 1.0]
    cots = WA.cotangents(times, x)
    kw = dict(regularize="unbiased", abstol=TOL, reltol=TOL, saveat=times, save_start=False, maxiters=10000, field="wide_chain")
    out = {}
    for tag, node in (("device", P.NeuralODE(model, adjoint_loop="device", **kw)), ("default", P.NeuralODE(model, **kw))):
        st = node.initialstates(np.random.default_rng(3))
        dx, dp, info = node.pullback(cu(x), cu(p), st, cu(cots))
        ai = node.handle().last_adjoint_info()
        sb = info["stats_bwd"]
        print(f"{tag}: {ai} {info['adjoint_loop']} naccept {sb['naccept']} nreject {sb['nreject']}")
        out[tag] = (dx, dp, info, ai, sb)
    dx, dp, info, ai, sb = out["device"]
    assert ai["kind"] == 3 and info["adjoint_loop"] == "wide_device" and ai["host_waits"] == 0
    assert ai["launches"] <= 2 * (sb["naccept"] + sb["nreject"]) + WA.LAUNCH_C
    dxh, dph, infoh, aih, sbh = out["default"]
    assert aih["kind"] == 0 and infoh["adjoint_loop"] == "host" and aih["host_waits"] >= sbh["naccept"]
    assert torch.equal(dx, dxh) and torch.equal(dp, dph)


# ---- 2. both loops, same bits -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("series", list(WA.SERIES))
@pytest.mark.parametrize("B", WA.BITS_BATCHES)
@pytest.mark.parametrize("name", WA.BITS_SHAPES)
def test_both_loops_same_bits(gpu_pkg, host_loop, name, B, series):
    bits_case(gpu_pkg, host_loop, name, B, WA.SERIES[series])


def test_rejected_step_after_an_impulse(gpu_pkg, host_loop):
    """the cotangent at 0.5 scaled x1000 (CA.PINNED's `big`): the attempt after the impulse is too long and is rejected;
    it keeps K1's slot of the stage record"""
    dev, _ = bits_case(gpu_pkg, host_loop, "mnist3", 17, [0.5, 1.0], tol=1e-4, scale=3.0, big=(0, 1000.0))
    assert dev["counts"][1] >= 1
    at_imp = [r for r in dev["rows"] if r[0] == -0.5]
    assert len(at_imp) >= 2 and at_imp[0][3] == 0, at_imp


def test_80_saved_times_take_two_begin_launches(gpu_pkg, host_loop):
    times = [(i + 1) / 80.0 for i in range(80)]
    dev, _ = bits_case(gpu_pkg, host_loop, "physionet", 17, times)
    assert dev["ai"]["launches"] > 2 * sum(dev["counts"][:2]) + 4 + 2 + 1 + 1   # more than one begin launch


def test_save_start_and_a_cotangent_at_t0(gpu_pkg, host_loop):
    bits_case(gpu_pkg, host_loop, "odd_td", 17, [0.0, 0.5, 1.0], save_start=True)


# ---- 4. against the float64 restatement and float64 autograd ---------------------------------------------------------------
@pytest.mark.parametrize("name,B", [("mnist3", 17), ("odd_td", 9)])
def test_gradients_vs_the_float64_restatement(gpu_pkg, name, B):
    """Measured on the MI355X, rel against the float64 restatement (bound 1e-5 in all four: 4 x the float32 twin's
    distance is below the floor) and against RK4 autograd (bar 3e-4): mnist3 B = 17 dx 4.7e-7 / 4.6e-7, dp 7.5e-7 / 7.3e-7;
    odd_td B = 9 dx 6.6e-7 / 6.4e-7, dp 8.9e-7 / 8.4e-7."""
    P = gpu_pkg
    model = WC.shapes(P)[name]
    p, x = WC.mk_inputs(P, model, B, scale=1.5)
    times = [0.25, 0.5, 1.0]
    cots = WA.cotangents(times, x)
    r64 = CA.pullback(model, p, x, times, cots, TOL)
    r32 = CA.pullback(model, p, x, times, cots, TOL, dtype=np.float32)
    got = WA.run_ts(WA.handle_for(P, model, p), x, times, cots, TOL)
    assert got["ai"]["kind"] == 3
    gx, gp = WC.reference_grads(model, p, x, times, cots)
    ref = dict(dx=gx, dp=gp)
    for key in ("dx", "dp"):
        bound = max(1e-5, 4.0 * WC.rel(r32[key], r64[key]))
        e, e_rk4 = WC.rel(got[key], r64[key]), WC.rel(got[key], ref[key])
        print(f"{name} B={B}: rel({key}, float64 restatement) {e:.2e} bound {bound:.2e}; rel({key}, RK4 autograd) {e_rk4:.2e}")
        assert e <= bound, (key, e, bound)
        assert e_rk4 < 3e-4, (key, e_rk4)


# ---- 5. regulariser ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["unbiased", "biased"])
def test_regulariser_has_the_host_loops_bits(gpu_pkg, host_loop, mode):
    P = gpu_pkg
    model = WC.shapes(P)["mnist3"]
    B = 17
    p, x = WC.mk_inputs(P, model, B, scale=1.5)
    h = WA.handle_for(P, model, p)
    times = [0.25, 0.5, 1.0]
    cots = WA.cotangents(times, x)
    kw = dict(mode=mode, t1_or_rand=0.43)
    d0 = WA.run_ts(h, x, times, cots, TOL, w_reg=0.0, **kw)
    d2 = WA.run_ts(h, x, times, cots, TOL, w_reg=2.0, **kw)
    with host_loop:
        h2 = WA.run_ts(h, x, times, cots, TOL, w_reg=2.0, **kw)
    assert d0["ai"]["kind"] == d2["ai"]["kind"] == 3 and h2["ai"]["kind"] == 0
    assert d2["reg_val"] == h2["reg_val"] and d2["reg_val"] > 0
    assert np.array_equal(d2["dp"], h2["dp"]) and not np.array_equal(d2["dp"], d0["dp"])
    assert np.array_equal(d2["dx"], d0["dx"]) and np.array_equal(d2["dx"], h2["dx"])   # the regulariser has no gradient to x


# ---- 6. training step -------------------------------------------------------------------------------------------------
def test_training_step_equals_the_default_nodes(gpu_pkg):
    P = gpu_pkg
    model = WC.shapes(P)["mnist3"]
    B, K, D = 16, 10, 784
    p, x = WC.mk_inputs(P, model, B)
    rng = np.random.default_rng(2)
    xd, ps = cu(x), cu(p)
    pc = cu((rng.random(K * (D + 1), dtype=np.float32) - np.float32(0.5)) * np.float32(0.1))
    lab = cu(rng.integers(0, K, B).astype(np.int32))
    kw = dict(regularize="unbiased", abstol=1e-5, reltol=1e-5, save_start=False, maxiters=10000, field="wide_chain")
    res = []
    for loop in ("device", "auto"):
        node = P.NeuralODE(model, adjoint_loop=loop, **kw)
        st = node.initialstates(np.random.default_rng(0))
        loss, _st2, stats, grads, _times = P.run_training_step(node, ps, pc, st, xd, lab, 2.5)
        res.append((loss, stats["y_pred"], grads, node.handle().last_adjoint_info()["kind"]))
    (l1, y1, g1, k1), (l0, y0, g0, k0) = res
    assert k1 == 3 and k0 == 0
    assert l1 == l0 and torch.equal(y1, y0)
    for key in ("neural_ode", "classifier", "x"):
        assert torch.equal(g1[key], g0[key]), key


# ---- 7. repeat and recovery ----------------------------------------------------------------------------------------------
def test_repeat_maxiters_and_stale_record(gpu_pkg):
    P = gpu_pkg
    model = WC.shapes(P)["mnist3"]
    B = 17
    p, x = WC.mk_inputs(P, model, B, scale=1.5)
    h = WA.handle_for(P, model, p)
    xd = cu(x)
    times = [0.25, 0.5, 1.0]
    cots = cu(WA.cotangents(times, x))
    outs = []
    for _ in range(2):
        h.node_forward_record_ts(xd, 0.0, 1.0, TOL, TOL, times, mode="none", maxiters=10000)
        outs.append(h.node_backward_recorded_ts(cots))
        assert h.last_adjoint_info()["kind"] == 3
    assert torch.equal(outs[0]["dx"], outs[1]["dx"]) and torch.equal(outs[0]["dp"], outs[1]["dp"])
    assert outs[0]["stats_bwd"] == outs[1]["stats_bwd"] and outs[0]["stats_bwd"]["retcode"] == 0
    # the backward takes maxiters from the record: a loose forward fits 3 attempts, the adjoint on [lambda; mu] does not
    fw = h.node_forward_record(xd, 0.0, 1.0, 1e-1, 1e-1, mode="none", maxiters=3)
    assert fw["stats"]["retcode"] == 0
    with pytest.raises(RuntimeError, match="MaxIters") as ei:
        h.node_backward_recorded(cots[2])
    assert "adjoint solve stopped with retcode" in str(ei.value) and h.last_adjoint_info()["kind"] == 3
    h.node_forward_record_ts(xd, 0.0, 1.0, TOL, TOL, times, mode="none", maxiters=10000)
    again = h.node_backward_recorded_ts(cots)
    assert h.last_adjoint_info()["kind"] == 3
    assert torch.equal(again["dx"], outs[0]["dx"]) and torch.equal(again["dp"], outs[0]["dp"])
    # a forward at another batch in between: the record is not this batch's
    h.node_forward_record(xd, 0.0, 1.0, TOL, TOL, mode="none")
    h.node_forward_record(xd[:9].contiguous(), 0.0, 1.0, TOL, TOL, mode="none")
    with pytest.raises(RuntimeError):
        h.node_backward_recorded(cots[2])


# ---- 8. gate ---------------------------------------------------------------------------------------------------------
def test_gate_refuses_and_auto_completes(gpu_pkg):
    P = gpu_pkg
    from localregneuralde_jl_amd import _lib as L
    model = WC.shapes(P)["full1024"]
    dims = WC.model_dims(model)
    B = WA.first_refused_batch(dims)
    assert B == 1633 and WA.gate(dims, B)["why"] == "WIDE_SCRATCH_MAX" and WA.gate(dims, B - 1)["fits"]
    p, x = WC.mk_inputs(P, model, B)
    h = WA.handle_for(P, model, p)
    xd = cu(x)
    cot = cu(np.random.default_rng(5).standard_normal(x.shape).astype(np.float32))
    fw = h.node_forward_record(xd, 0.0, 1.0, 1e-2, 1e-2, mode="none")
    print(f"full1024 B={B}: forward naccept {fw['stats']['naccept']}")
    with pytest.raises((NotImplementedError, L.LrndeError)) as ei:
        h.node_backward_recorded(cot)
    assert isinstance(ei.value, NotImplementedError) or ei.value.code == 8   # LRNDE_UNSUPPORTED
    assert "WIDE_SCRATCH_MAX" in str(ei.value) and f"B = {B}" in str(ei.value)
    h.set_adjoint_loop("auto")
    bw = h.node_backward_recorded(cot)   # the same handle and record, on the host loop
    assert h.last_adjoint_info()["kind"] == 0 and bw["stats_bwd"]["retcode"] == 0
    assert torch.isfinite(bw["dx"]).all() and torch.isfinite(bw["dp"]).all()
