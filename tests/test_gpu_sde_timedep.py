"""The SDE stack with a time-dependent drift on the device, through the C ABI (SdeHandle) and the layer (NeuralDSDE).

The reference hands both closures ArrayAndTime(u, t) (src/layers/neural_sde.jl:55-66) and its steps evaluate the drift at
t and t + dt (Euler-Heun), t (Milstein), t, t + c02 dt, t + c03 dt, t + c04 dt (SRI).  A handle with time_dep = 1 runs the generic
kernels and the host-controlled loop; every time it passes is a live input here (tests/test_host_sde_timedep.py shows on the
reference alone that a wrong time moves each compared quantity by at least 1e-3 of its norm).

* steps and fixed-grid solves == the C oracle bit for bit (u, eest, reg_val) on every shape of sde_timedep_cases.STEP_CASES;
* the adaptive layer forward == tests/sde_adaptive_np.py's loop bit for bit, all three modes, default and LRNDE_SDE_HOST_LOOP=1;
* every pullback against float64 torch autograd of the float64 steps of tests/sde_timedep_cases.py, at the bounds the project
  holds the same kernels to with a time-independent drift (tests/test_gpu_sde_gradients.py, test_gpu_sde_adaptive_alg.py);
  every measured error is printed;
* lrnde_sde_sri_step_backward's contract row by row: du_new set or NULL, w_reg 0 / 1 / 2, dx wanted or not, dp_* ADDED to;
* the NeuralDSDE layer built on a TDChain drift."""
import copy

import numpy as np
import pytest
import torch

import sde_timedep_cases as TC

pytestmark = pytest.mark.gpu
f32 = np.float32
t, dt = TC.T_STEP, TC.DT_STEP


def _desc(P, D, H):
    from localregneuralde_jl_amd.layers import _mlp_desc
    return _mlp_desc(P.TDChain(P.Chain(P.Dense(D + 1, H, "tanh"), P.Dense(H + 1, D))))


def _handle(P, D, H, inp):
    h = P.SdeHandle(_desc(P, D, H))
    h.set_params(inp["pd"], inp["pg"])
    return h


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fields():
    from localregneuralde_jl_amd import _lib as L
    return L.SRI_FIELDS


def _same(got, ref, what):
    gu = got["u"].cpu().numpy()
    assert np.array_equal(gu.view(np.int32), ref["u"].view(np.int32)), (what, float(np.abs(gu - ref["u"]).max()))
    assert got["eest"] == ref["eest"] and got["reg_val"] == ref["reg_val"], (what, got["eest"], ref["eest"], got["reg_val"], ref["reg_val"])


def _report(what, errs, bounds):
    print(what + ": rel err vs float64 autograd " + ", ".join(f"{k} {v:.2e} (bound {bounds[k]:.0e})" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < bounds[k], (what, k, v, bounds[k])


def _errs(got, ref):
    return {k: TC.rel(got[k].cpu().numpy(), r) for k, r in zip(("dx", "dp_drift", "dp_diff"), ref) if got.get(k) is not None}


# ---- steps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", TC.STEP_CASES, ids=TC.step_id)
def test_steps_equal_the_oracle_bit_for_bit(oracle, gpu_pkg, c):
    D, H, B = c
    inp = TC.step_inputs(D, H, B)
    drift, diff = TC.oracle_fields(oracle, D, H, inp["pd"], inp["pg"])
    h = _handle(gpu_pkg, D, H, inp)
    x, dW, dZ = _dev(inp["x"]), _dev(inp["dW"]), _dev(inp["dZ"])
    _same(h.euler_heun_step(x, dW, t, dt, TC.TOL, TC.TOL, TC.DELTA),
          oracle.euler_heun_step(drift, diff, inp["x"], inp["dW"], t, dt, TC.TOL, TC.TOL, TC.DELTA), "euler-heun")
    _same(h.rkmil_step(x, dW, t, dt, TC.TOL, TC.TOL), oracle.rkmil_step(drift, diff, inp["x"], inp["dW"], t, dt, TC.TOL, TC.TOL), "milstein")
    T = TC.sri_tableau(TC.TAB_SEED)
    _same(h.sri_step(T, x, dW, dZ, t, dt, TC.TOL, TC.TOL, TC.DELTA),
          oracle.sri_step(drift, diff, T, inp["x"], inp["dW"], inp["dZ"], t, dt, TC.TOL, TC.TOL, TC.DELTA), "sri")


@pytest.mark.parametrize("solver", ["EulerHeun", "RKMil"])
@pytest.mark.parametrize("c", TC.STEP_CASES, ids=TC.step_id)
def test_fixed_grid_solve_equals_the_oracle_step_loop(oracle, gpu_pkg, c, solver):
    """n = 5 steps from t0 = 0.2: step i starts at t0 + i dt"""
    D, H, B = c
    n = 5
    inp = TC.grid_inputs(D, H, B, n)
    drift, diff = TC.oracle_fields(oracle, D, H, inp["pd"], inp["pg"])
    t0, dtg = inp["t0"], inp["dt"]
    got = _handle(gpu_pkg, D, H, inp).solve_fixed(_dev(inp["x"]), _dev(inp["dW"]), t0, dtg, TC.TOL, TC.TOL, TC.DELTA, solver=solver)
    u = inp["x"]
    for i in range(n):
        ti = f32(f32(t0) + f32(i) * dtg)
        r = (oracle.euler_heun_step(drift, diff, u, inp["dW"][i], ti, dtg, TC.TOL, TC.TOL, TC.DELTA) if solver == "EulerHeun" else
             oracle.rkmil_step(drift, diff, u, inp["dW"][i], ti, dtg, TC.TOL, TC.TOL))
        _same(dict(u=got["u"][i], eest=got["eest"][i], reg_val=got["reg_val"][i]), r, f"{solver} step {i}")
        u = r["u"]


# ---- the adaptive layer's forward -------------------------------------------------------------------------------------------
def _forward(h, c, inp, T, mode, saveat=(), t1_or_rand=TC.T1, dt0=None):
    return h.node_forward_record(_dev(inp["x"]), _dev(inp["W"]), TC.T0, TC.T2, c["tol"], c["tol"], mode=mode, t1_or_rand=t1_or_rand,
                                 z_local=_dev(inp["z"]), saveat=saveat, dt0=c["dt0"] if dt0 is None else dt0, solver=c["kind"],
                                 tableau=None if T is None else [T[k] for k in _fields()], path_z=_dev(inp["Z"]), z_local2=_dev(inp["z2"]))


def _check_forward(got, ref, what):
    assert got["stats"]["naccept"] == ref["naccept"] and got["stats"]["nreject"] == ref["nreject"], (what, got["stats"], ref["naccept"], ref["nreject"])
    assert got["nfe_drift"] == ref["nfe_drift"] and got["nfe_diffusion"] == ref["nfe_diffusion"], (what, got["nfe_drift"], ref["nfe_drift"])
    assert np.array_equal(got["t"], ref["t"]), (what, got["t"], ref["t"])
    assert got["reg_val"] == ref["reg_val"], (what, got["reg_val"], ref["reg_val"])
    gu = got["u"].cpu().numpy()
    assert gu.shape == ref["u"].shape, (what, gu.shape, ref["u"].shape)
    assert np.array_equal(gu, ref["u"]), (what, float(np.abs(gu - ref["u"]).max()))
    assert got["t1"] == ref["t1"], what


@pytest.mark.parametrize("mode", TC.MODES)
@pytest.mark.parametrize("c", TC.ADAPTIVE_CASES, ids=TC.adaptive_id)
def test_adaptive_forward_equals_the_reference_loop_on_both_routes(oracle, gpu_pkg, c, mode):
    D, H, B, nfine = c["shape"]
    inp, T, ref = TC.adaptive_reference(oracle, c, mode)
    h = _handle(gpu_pkg, D, H, inp)
    got = _forward(h, c, inp, T, mode)
    _check_forward(got, ref, f"{TC.adaptive_id(c)} {mode}")
    gpu_pkg.set_option("LRNDE_SDE_HOST_LOOP", 1)
    try:
        host = _forward(h, c, inp, T, mode)
    finally:
        gpu_pkg.set_option("LRNDE_SDE_HOST_LOOP", 0)
    _check_forward(host, ref, f"{TC.adaptive_id(c)} {mode}, host loop")
    assert torch.equal(got["u"], host["u"]) and got["reg_val"] == host["reg_val"]
    assert ref["nreject"] >= 1
    print(f"{TC.adaptive_id(c)} {mode}: accepted {ref['naccept']}, rejected {ref['nreject']}, series {len(ref['t'])}, reg_val {ref['reg_val']:.4g}")


# ---- pullbacks against float64 autograd -----------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["EulerHeun", "RKMil"])
@pytest.mark.parametrize("c", TC.STEP_CASES, ids=TC.step_id)
def test_fixed_grid_pullback_and_regulariser_gradient(gpu_pkg, c, solver):
    """solve_fixed_backward over n = 5 steps from t0 = 0.2 (Euler-Heun 2e-5, Milstein 5e-6 of each gradient's norm) and the
    local step's d (EEst dt) / d ps at t = 0.4 (2e-5)"""
    D, H, B = c
    n = 5
    inp = TC.grid_inputs(D, H, B, n)
    t0, dtg = inp["t0"], inp["dt"]
    h = _handle(gpu_pkg, D, H, inp)
    x, dW = _dev(inp["x"]), _dev(inp["dW"])
    tr = h.solve_fixed(x, dW, t0, dtg, TC.TOL, TC.TOL, TC.DELTA, solver=solver)
    bw = h.solve_fixed_backward(x, tr["u"], dW, t0, dtg, _dev(inp["du"]), solver=solver)
    step = TC.eh_step64 if solver == "EulerHeun" else TC.mil_step64
    pdt, pgt, xt = TC.leaves(inp)
    f, g = TC.fields64(pdt, pgt, D, H)
    u = xt
    for i in range(n):
        u = step(f, g, u, TC.tt(inp["dW"][i]), t0 + i * float(dtg), float(dtg))[0]
    assert TC.rel(tr["u"][-1].cpu().numpy(), u.detach().numpy()) < 1e-5
    (u * TC.tt(inp["du"])).sum().backward()
    b = 2e-5 if solver == "EulerHeun" else 5e-6
    _report(f"{solver} {TC.step_id(c)} fixed-grid pullback", _errs(bw, (xt.grad.numpy(), pdt.grad.numpy(), pgt.grad.numpy())),
            dict(dx=b, dp_drift=b, dp_diff=b))
    # the regulariser of one local step
    u1 = tr["u"][n // 2].contiguous()
    w1 = _dev(inp["dZ"][0])
    rg = (h.euler_heun_reg_grad(u1, w1, t, dtg, TC.TOL, TC.TOL, TC.DELTA) if solver == "EulerHeun" else
          h.rkmil_reg_grad(u1, w1, t, dtg, TC.TOL, TC.TOL))
    pdt, pgt, _ = TC.leaves(inp)
    f, g = TC.fields64(pdt, pgt, D, H)
    val = step(f, g, TC.tt(u1.cpu().numpy()), TC.tt(inp["dZ"][0]), t, float(dtg))[1]
    assert abs(float(val.detach()) - float(rg["reg_val"])) < 2e-5 * abs(float(val.detach()))
    val.backward()
    _report(f"{solver} {TC.step_id(c)} regulariser gradient", _errs(rg, (None, pdt.grad.numpy(), pgt.grad.numpy())),
            dict(dp_drift=2e-5, dp_diff=2e-5))
    assert (rg["dp_drift"] != 0).any() and (rg["dp_diff"] != 0).any()


@pytest.mark.parametrize("c", TC.CONTRACT_CASES, ids=TC.step_id)
def test_sri_step_chain_pullback_and_regulariser_gradient(gpu_pkg, c):
    """a chain of n = 3 SRI steps from t0 = 0.2 swept newest first (1e-5), and the local step's regulariser alone (5e-5)"""
    D, H, B = c
    n = 3
    inp = TC.grid_inputs(D, H, B, n)
    t0, dtg = inp["t0"], inp["dt"]
    T = TC.sri_tableau(TC.TAB_SEED)
    tab = [T[k] for k in _fields()]
    h = _handle(gpu_pkg, D, H, inp)
    x = _dev(inp["x"])
    us, u = [], x
    for i in range(n):
        u = h.sri_step(tab, u, _dev(inp["dW"][i]), _dev(inp["dZ"][i]), t0 + i * float(dtg), dtg, TC.TOL, TC.TOL, TC.DELTA)["u"]
        us.append(u)
    ub, dpf, dpg = _dev(inp["du"]), None, None
    for i in range(n - 1, -1, -1):
        r = h.sri_step_backward(tab, x if i == 0 else us[i - 1], _dev(inp["dW"][i]), _dev(inp["dZ"][i]), t0 + i * float(dtg), dtg,
                                TC.TOL, TC.TOL, TC.DELTA, du_new=ub, dp_drift=dpf, dp_diff=dpg)
        ub, dpf, dpg = r["dx"], r["dp_drift"], r["dp_diff"]
    pdt, pgt, xt = TC.leaves(inp)
    f, g = TC.fields64(pdt, pgt, D, H)
    u64 = xt
    for i in range(n):
        u64 = TC.sri_step64(f, g, T, u64, TC.tt(inp["dW"][i]), TC.tt(inp["dZ"][i]), t0 + i * float(dtg), float(dtg))[0]
    assert TC.rel(us[-1].cpu().numpy(), u64.detach().numpy()) < 1e-5
    (u64 * TC.tt(inp["du"])).sum().backward()
    _report(f"sri {TC.step_id(c)} step chain", _errs(dict(dx=ub, dp_drift=dpf, dp_diff=dpg), (xt.grad.numpy(), pdt.grad.numpy(), pgt.grad.numpy())),
            dict(dx=1e-5, dp_drift=1e-5, dp_diff=1e-5))
    u1 = us[1].contiguous()
    rg = h.sri_step_backward(tab, u1, _dev(inp["dW"][0]), _dev(inp["dZ"][1]), t, dtg, TC.TOL, TC.TOL, TC.DELTA, du_new=None, w_reg=1.0, want_dx=False)
    pdt, pgt, _ = TC.leaves(inp)
    f, g = TC.fields64(pdt, pgt, D, H)
    val = TC.sri_step64(f, g, T, TC.tt(u1.cpu().numpy()), TC.tt(inp["dW"][0]), TC.tt(inp["dZ"][1]), t, float(dtg))[1]
    assert abs(float(val.detach()) - float(rg["reg_val"])) < 5e-5 * abs(float(val.detach()))
    val.backward()
    _report(f"sri {TC.step_id(c)} regulariser gradient", _errs(rg, (None, pdt.grad.numpy(), pgt.grad.numpy())), dict(dp_drift=5e-5, dp_diff=5e-5))


@pytest.mark.parametrize("c", TC.ADAPTIVE_CASES, ids=TC.adaptive_id)
def test_recorded_pullback_matches_float64_autograd(oracle, gpu_pkg, c):
    """loss = sum_j <du_j, sol.u[j]> + 2 reg_val with a user saveat that has an interpolated entry: 5e-6 of each gradient's norm.
    The recorded step (i, m) is swept at t0 + i h, the local step at t1 (the float64 side: sde_timedep_cases.adaptive_autograd64)."""
    D, H, B, nfine = c["shape"]
    inp, T, ref = TC.adaptive_reference(oracle, c, "unbiased", saveat=TC.SAVEAT)
    h = _handle(gpu_pkg, D, H, inp)
    got = _forward(h, c, inp, T, "unbiased", saveat=TC.SAVEAT)
    _check_forward(got, ref, TC.adaptive_id(c))
    assert any(0.0 < float(th) < 1.0 for (_, k, th) in ref["series"])
    du = np.random.default_rng(5).standard_normal((len(ref["t"]), B, D)).astype(f32)
    bw = h.node_backward_recorded(_dev(du), w_reg=2.0)
    _report(f"{TC.adaptive_id(c)} recorded pullback, {ref['naccept']} steps", _errs(bw, TC.adaptive_autograd64(c, inp, T, ref, du, 2.0)),
            dict(dx=5e-6, dp_drift=5e-6, dp_diff=5e-6))


@pytest.mark.parametrize("c", TC.ADAPTIVE_CASES, ids=TC.adaptive_id)
def test_recorded_regulariser_gradient_alone(oracle, gpu_pkg, c):
    """zero cotangents on the series, w_reg = 1: d reg_val / d ps within 2e-5, d reg_val / d x exactly zero"""
    D, H, B, nfine = c["shape"]
    inp, T, ref = TC.adaptive_reference(oracle, c, "unbiased")
    h = _handle(gpu_pkg, D, H, inp)
    got = _forward(h, c, inp, T, "unbiased")
    _check_forward(got, ref, TC.adaptive_id(c))
    assert float(ref["reg_val"]) > 1e-6
    du = np.zeros((len(ref["t"]), B, D), f32)
    bw = h.node_backward_recorded(_dev(du), w_reg=1.0)
    gx, gpd, gpg = TC.adaptive_autograd64(c, inp, T, ref, du, 1.0)
    assert not bw["dx"].cpu().numpy().any() and not gx.any()
    assert np.abs(gpd).max() > 0 and np.abs(gpg).max() > 0
    _report(f"{TC.adaptive_id(c)} regulariser alone, reg_val {ref['reg_val']:.4g}", _errs(dict(dp_drift=bw["dp_drift"], dp_diff=bw["dp_diff"]), (None, gpd, gpg)),
            dict(dp_drift=2e-5, dp_diff=2e-5))


# ---- lrnde_sde_sri_step_backward: the contract of include/lrnde.h, row by row ---------------------------------------------
@pytest.mark.parametrize("w_reg", [0.0, 1.0, 2.0])
@pytest.mark.parametrize("with_du", [True, False], ids=["du_new", "du_null"])
@pytest.mark.parametrize("c", TC.CONTRACT_CASES, ids=TC.step_id)
def test_sri_step_backward_contract(gpu_pkg, c, with_du, w_reg):
    """loss = <du_new, u'> + w_reg EEst dt  ->  dx (when asked for), dp_drift / dp_diff ADDED to what the caller passes in.
    dx, dp_*: 1e-5 of each gradient's norm when du_new is set, 5e-5 when the loss is the regulariser alone (the bounds of
    test_sri_solve_and_regulariser_gradients_match_float64_autograd); a zero loss leaves dp_* as they were and dx zero.  The
    pre-filled dp_* are N(0,1) times the float64 gradient's rms, so the sum is rounded at the gradient's own magnitude."""
    D, H, B = c
    inp = TC.step_inputs(D, H, B)
    T = TC.sri_tableau(TC.TAB_SEED)
    tab = [T[k] for k in _fields()]
    h = _handle(gpu_pkg, D, H, inp)
    x, dW, dZ = _dev(inp["x"]), _dev(inp["dW"]), _dev(inp["dZ"])
    pdt, pgt, xt = TC.leaves(inp)
    f, g = TC.fields64(pdt, pgt, D, H)
    un, reg = TC.sri_step64(f, g, T, xt, TC.tt(inp["dW"]), TC.tt(inp["dZ"]), t, dt)
    zero_loss = not with_du and w_reg == 0.0
    if zero_loss:
        ref = [np.zeros((B, D)), np.zeros(pdt.numel()), np.zeros(pgt.numel())]
    else:
        ((un * TC.tt(inp["du"])).sum() * (1.0 if with_du else 0.0) + w_reg * reg).backward()
        ref = [xt.grad.numpy(), pdt.grad.numpy(), pgt.grad.numpy()]
    rng = np.random.default_rng(9)
    rms = lambda a: float(np.sqrt(np.mean(a * a))) or 1.0
    pre = [None, (rng.standard_normal(ref[1].size) * rms(ref[1])).astype(f32), (rng.standard_normal(ref[2].size) * rms(ref[2])).astype(f32)]
    b = 1e-5 if with_du else 5e-5
    for want_dx in (True, False):
        dpf, dpg = _dev(pre[1]), _dev(pre[2])
        r = h.sri_step_backward(tab, x, dW, dZ, t, dt, TC.TOL, TC.TOL, TC.DELTA, du_new=_dev(inp["du"]) if with_du else None, w_reg=w_reg,
                                want_dx=want_dx, dp_drift=dpf, dp_diff=dpg)
        assert r["dp_drift"] is dpf and r["dp_diff"] is dpg and (r["dx"] is not None) == want_dx
        assert abs(float(r["reg_val"]) - float(reg.detach())) < 5e-5 * float(reg.detach())
        what = f"sri contract {TC.step_id(c)} du_new={'set' if with_du else 'NULL'} w_reg={w_reg:g} dx={'yes' if want_dx else 'no'}"
        if zero_loss:
            assert torch.equal(dpf, _dev(pre[1])) and torch.equal(dpg, _dev(pre[2])), what
            assert not want_dx or not r["dx"].cpu().numpy().any(), what
            continue
        # dp_* minus what was passed in, in float64
        added = dict(dx=r["dx"], dp_drift=(dpf.double().cpu() - torch.from_numpy(pre[1]).double()), dp_diff=(dpg.double().cpu() - torch.from_numpy(pre[2]).double()))
        _report(what, _errs(added, ref), dict(dx=b, dp_drift=b, dp_diff=b))


# ---- the layer --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", TC.ADAPTIVE_CASES, ids=TC.adaptive_id)
def test_layer_on_a_tdchain_drift(oracle, gpu_pkg, c):
    P = gpu_pkg
    D, H, B, nfine = c["shape"]
    inp = TC.adaptive_inputs(c)
    T = TC.sri_tableau(*c["tab"]) if c["kind"] == "SRI" else None
    node = P.NeuralDSDE(P.TDChain(P.Chain(P.Dense(D + 1, H, "tanh"), P.Dense(H + 1, D))), P.Dense(D, D), solver=c["kind"],
                        tableau=None if T is None else [T[k] for k in _fields()], tspan=(TC.T0, TC.T2), regularize="unbiased",
                        adaptive=True, nfine=nfine, dt0=c["dt0"], abstol=c["tol"], reltol=c["tol"], maxiters=10000)
    assert node.desc.time_dep == 1
    st = node.initialstates(np.random.default_rng(0))
    ps = dict(drift=inp["pd"], diffusion=inp["pg"])
    x = _dev(inp["x"])
    kw = dict(path=_dev(inp["W"]), z_local=_dev(inp["z"]), path_z=_dev(inp["Z"]), z_local2=_dev(inp["z2"]))
    sol, st2 = node(x, ps, st, **kw)
    # the layer's t1: one float32 uniform draw from its stream, mapped onto the span (src/layers/neural_sde.jl:92)
    r01 = f32(copy.deepcopy(st["rng"]).random(dtype=f32))
    t1 = f32(r01 * (node.tspan[1] - node.tspan[0]) + node.tspan[0])
    _, _, ref = TC.adaptive_reference(oracle, c, "unbiased", t1_or_rand=float(t1))
    assert len(sol.u) == len(ref["t"]) and all(a == b for a, b in zip(sol.t, ref["t"]))
    assert np.array_equal(torch.stack(list(sol.u)).cpu().numpy(), ref["u"])
    assert st2["reg_val"] == ref["reg_val"] and st2["nfe_drift"] == ref["nfe_drift"] and st2["nfe_diffusion"] == ref["nfe_diffusion"]
    assert sol.stats["naccept"] == ref["naccept"] and sol.stats["nreject"] == ref["nreject"] >= 1
    du_end = torch.ones_like(x)
    dx0, dps0, _ = node.pullback_series(x, ps, st, None, du_end=du_end, w_reg=0.0, **kw)
    dx2, dps2, info = node.pullback_series(x, ps, st, None, du_end=du_end, w_reg=2.0, **kw)
    assert torch.isfinite(dx0).all() and (dx0 != 0).any() and torch.equal(dx0, dx2) and info["dx_reg"] is None
    assert not torch.equal(dps0["drift"], dps2["drift"]) and not torch.equal(dps0["diffusion"], dps2["diffusion"])
    assert torch.equal(info["sol"].u[-1], sol.u[-1])
