"""The adaptive NeuralDSDE layer with the Milstein (src/perform_step.jl:108-170) and four-stage SRI (:49-106) steps on the device.

* forward: `lrnde_sde_node_forward_record_alg` == tests/sde_adaptive_np.py (the oracle's loop with the step as a parameter; pinned
  to oracle.sde_node_forward in tests/test_host_sde_adaptive.py, which also fixes the cases used here) BIT FOR BIT: every state of
  the series, sol.t, reg_val, the closures' call counts, accepted / rejected steps, t1.  Milstein: the one-launch kernel with the
  controller in its footer (k_sde_mil_fast) on every branch of its templates, and the generic kernel under the host-controlled
  loop; the same bits on all three routes.  SRI: the host-controlled loop.
* pullback: `lrnde_sde_node_backward_recorded` on a Milstein / SRI record against float64 torch autograd over the recorded grid
  (the float64 steps of test_gpu_sde_gradients.py): 5e-6 of each gradient's norm, the bound those reverse kernels already meet
  there and in test_gpu_sde_layer.py; the regulariser alone: 2e-5, dx exactly zero.
* records of different kinds do not mix; the layer with noise_source="device" (streams 4 / 5 for SRI's second path and draw)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import philox_np as PX
import sde_adaptive_np as S
from test_gpu_sde_gradients import _fields64, _mil_step64, _rel, _sri_step64
from test_host_sde_adaptive import CASES, MODES, case_id, case_reference

pytestmark = pytest.mark.gpu
f32 = np.float32
MIL = [c for c in CASES if c["kind"] == "RKMil"]
SRI = [c for c in CASES if c["kind"] == "SRI"]


def _check_forward(got, ref, what):
    assert got["stats"]["naccept"] == ref["naccept"] and got["stats"]["nreject"] == ref["nreject"], (what, got["stats"], ref["naccept"], ref["nreject"])
    assert got["nfe_drift"] == ref["nfe_drift"] and got["nfe_diffusion"] == ref["nfe_diffusion"], (what, got["nfe_drift"], ref["nfe_drift"])
    assert np.array_equal(got["t"], ref["t"]), (what, got["t"], ref["t"])
    assert got["reg_val"] == ref["reg_val"], (what, got["reg_val"], ref["reg_val"])
    gu = got["u"].cpu().numpy()
    assert gu.shape == ref["u"].shape, (what, gu.shape, ref["u"].shape)
    assert np.array_equal(gu, ref["u"]), (what, float(np.abs(gu - ref["u"]).max()))
    assert got["t1"] == ref["t1"], what


def _handle(P, c, inp):
    from localregneuralde_jl_amd.layers import _mlp_desc
    D, H, B, nfine = c["shape"]
    h = P.SdeHandle(_mlp_desc(P.Chain(P.Dense(D, H, "tanh"), P.Dense(H, D))))
    h.set_params(inp["pd"], inp["pg"])
    return h


def _forward(h, c, inp, T, mode, **kw):
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    args = dict(mode=mode, t1_or_rand=0.43, saveat=(), save_start=-1, dt0=c["dt0"])
    args.update(kw)
    return h.node_forward_record(dev(inp["x"]), dev(inp["W"]), 0.0, 1.0, c["tol"], c["tol"], z_local=dev(inp["z"]), solver=c["kind"],
                                 tableau=None if T is None else [T[k] for k in S_FIELDS()], path_z=dev(inp["Z"]), z_local2=dev(inp["z2"]), **args)


def S_FIELDS():
    from localregneuralde_jl_amd import _lib as L
    return L.SRI_FIELDS


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", MIL, ids=case_id)
def test_milstein_forward_equals_the_helper(oracle, gpu_pkg, c, mode):
    inp, T, ref = case_reference(oracle, c, mode)
    h = _handle(gpu_pkg, c, inp)
    got = _forward(h, c, inp, T, mode)
    _check_forward(got, ref, f"{case_id(c)} {mode}")
    assert got["stats"]["nf"] == ref["naccept"] + ref["nreject"]      # one drift evaluation per attempted step
    assert (got["reg_val"] == 0) == (mode == "none")
    print(f"{case_id(c)} {mode}: accepted {ref['naccept']}, rejected {ref['nreject']}, series {len(ref['t'])}, reg_val {ref['reg_val']:.4g}")


@pytest.mark.parametrize("c", [MIL[0], MIL[5]], ids=case_id)
def test_milstein_same_bits_on_all_three_routes(oracle, gpu_pkg, c):
    """the fused kernel with the device controller, the host-controlled loop on the generic kernel (LRNDE_SDE_HOST_LOOP), and
    lrnde_sde_rkmil_step fed the recorded (i, m) steps one by one"""
    assert c["shape"] == (32, 64, 40, 64)
    inp, T, ref = case_reference(oracle, c, "biased")      # :biased with saveat = (): the series is every accepted step's end state
    h = _handle(gpu_pkg, c, inp)
    fused = _forward(h, c, inp, T, "biased")
    gpu_pkg.set_option("LRNDE_SDE_HOST_LOOP", 1)
    try:
        host = _forward(h, c, inp, T, "biased")
    finally:
        gpu_pkg.set_option("LRNDE_SDE_HOST_LOOP", 0)
    _check_forward(fused, ref, "fused")
    _check_forward(host, ref, "host loop")
    assert torch.equal(fused["u"], host["u"]) and fused["reg_val"] == host["reg_val"]
    assert all(fused["stats"][k] == host["stats"][k] for k in ("retcode", "naccept", "nreject", "nf", "iters"))
    nfine = c["shape"][3]
    hh = f32(f32(1.0) / f32(nfine))
    W = torch.from_numpy(inp["W"]).cuda()
    u = torch.from_numpy(inp["x"]).cuda()
    assert len(ref["steps"]) + 1 == fused["u"].shape[0]
    for k, (i, m) in enumerate(ref["steps"]):
        r = h.rkmil_step(u, (W[i + m] - W[i]).contiguous(), f32(f32(i) * hh), f32(f32(m) * hh), c["tol"], c["tol"])
        u = r["u"]
        assert torch.equal(u, fused["u"][k + 1]), k
    if c["dt0"]:
        assert ref["nreject"] >= 1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", SRI, ids=case_id)
def test_sri_forward_equals_the_helper(oracle, gpu_pkg, c, mode):
    inp, T, ref = case_reference(oracle, c, mode)
    h = _handle(gpu_pkg, c, inp)
    got = _forward(h, c, inp, T, mode)
    _check_forward(got, ref, f"{case_id(c)} {mode}")
    assert got["stats"]["nf"] == 4 * (ref["naccept"] + ref["nreject"])
    print(f"{case_id(c)} {mode}: accepted {ref['naccept']}, rejected {ref['nreject']}, series {len(ref['t'])}, reg_val {ref['reg_val']:.4g}")


@pytest.mark.parametrize("c,mode,saveat", [(MIL[0], "unbiased", (0.0, 0.43, 0.7, 1.0)), (SRI[0], "biased", ())],
                         ids=["milstein-corrected", "sri-biased"])
def test_saveat_and_corrected_solution(oracle, gpu_pkg, c, mode, saveat):
    """:unbiased adds t1 to a user saveat and `_CorrectedDESolution` drops every entry at t1 again (0.43 is in the user's list:
    both go); :biased with saveat = () saves every step and draws t1 from sol.t[1:end-1]"""
    inp, T, ref = case_reference(oracle, c, mode, saveat=saveat)
    got = _forward(_handle(gpu_pkg, c, inp), c, inp, T, mode, saveat=saveat)
    _check_forward(got, ref, f"{case_id(c)} {mode} {saveat}")
    if saveat:
        assert f32(0.43) not in got["t"] and list(got["t"]) == [f32(0.0), f32(0.7), f32(1.0)]
    else:
        assert got["t1"] in got["t"][:-1] and len(got["t"]) == ref["naccept"] + 1


def _autograd64(c, inp, T, ref, du_series, w_reg):
    """loss = sum_j <du_j, sol.u[j]> + w_reg * reg_val in float64 over the RECORDED grid (ref['steps']), by torch autograd"""
    D, H, B, nfine = c["shape"]
    tol, delta = c["tol"], 1.0 / 6.0
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    pdt, pgt, xt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (inp["pd"], inp["pg"], inp["x"]))
    f, g = _fields64(pdt, pgt, D, H)
    hh = 1.0 / nfine
    Wt = t64(inp["W"])
    Zt = t64(inp["Z"]) if c["kind"] == "SRI" else None

    def step(u, dW, dZ, dt):
        if c["kind"] == "RKMil":
            un = _mil_step64(f, g, u, dW, dt)
            r = (un - u) / (tol + torch.maximum(u.abs(), un.abs()) * tol)     # :166-169, the four-argument residual
            return un, torch.sqrt((r * r).mean()) * dt
        return _sri_step64(f, g, T, u, dW, dZ, dt, tol, tol, delta)
    states, u = [], xt
    for (i, m) in ref["steps"]:
        u = step(u, Wt[i + m] - Wt[i], None if Zt is None else Zt[i + m] - Zt[i], m * hh)[0]
        states.append(u)
    loss = 0.0
    for j, (ts, k, th) in enumerate(ref["series"]):
        if k < 0:
            val = xt
        else:
            a = xt if k == 0 else states[k - 1]
            val = (1.0 - float(th)) * a + float(th) * states[k]
        loss = loss + (val * t64(du_series[j])).sum()
    if ref["u1"] is not None and w_reg != 0.0:
        loss = loss + w_reg * step(t64(ref["u1"]), t64(ref["dW_local"]), None if ref["dZ_local"] is None else t64(ref["dZ_local"]),
                                   float(ref["dt_local"]))[1]
    loss.backward()
    return xt.grad.numpy(), pdt.grad.numpy(), pgt.grad.numpy()


@pytest.mark.parametrize("c,saveat", [(MIL[0], (0.3, 0.77, 1.0)), (MIL[0], ()), (MIL[4], ()), (SRI[1], (0.3, 0.77, 1.0)), (SRI[1], ())],
                         ids=["milstein-saveat", "milstein-default", "milstein-outside-gate", "sri-saveat", "sri-default"])
def test_pullback_matches_float64_autograd(oracle, gpu_pkg, c, saveat):
    """loss = sum_j <du_j, sol.u[j]> + 2 reg_val; the measured errors are printed (bound 5e-6 on dx, dp_drift, dp_diff:
    DESIGN.md 4.3.1)"""
    mode = "unbiased"
    inp, T, ref = case_reference(oracle, c, mode, saveat=saveat, t1_or_rand=0.37)
    h = _handle(gpu_pkg, c, inp)
    got = _forward(h, c, inp, T, mode, saveat=saveat, t1_or_rand=0.37)
    _check_forward(got, ref, f"{case_id(c)} {saveat}")
    if saveat:
        assert any(0.0 < float(th) < 1.0 for (_, k, th) in ref["series"])      # interpolated entries
    ns, (D, H, B, nfine) = len(ref["t"]), c["shape"]
    du = np.random.default_rng(5).standard_normal((ns, B, D)).astype(f32)
    bw = h.node_backward_recorded(torch.from_numpy(du).cuda(), w_reg=2.0)
    gx, gpd, gpg = _autograd64(c, inp, T, ref, du, 2.0)
    errs = {n: _rel(a.cpu().numpy(), b) for n, a, b in (("dx", bw["dx"], gx), ("dp_drift", bw["dp_drift"], gpd), ("dp_diff", bw["dp_diff"], gpg))}
    print(f"{case_id(c)} saveat={saveat}: {ref['naccept']} recorded steps, series {ns}; rel err vs float64 autograd " +
          ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < 5e-6, (k, v)


@pytest.mark.parametrize("c", [MIL[0], SRI[1]], ids=case_id)
def test_regulariser_gradient_alone(oracle, gpu_pkg, c):
    """zero cotangents on the series, w_reg = 1, explicit dt0 = 0.05 (the automatic one makes reg_val ~ 1e-6): d reg_val / d ps
    alone within 2e-5 of float64 autograd, d reg_val / d x exactly zero (test/runtests.jl:388-392: `=== nothing`)"""
    c = dict(c, dt0=0.05)
    inp, T, ref = case_reference(oracle, c, "unbiased", t1_or_rand=0.41)
    h = _handle(gpu_pkg, c, inp)
    got = _forward(h, c, inp, T, "unbiased", t1_or_rand=0.41)
    _check_forward(got, ref, case_id(c))
    assert float(ref["reg_val"]) > 1e-6
    ns, (D, H, B, nfine) = len(ref["t"]), c["shape"]
    du = np.zeros((ns, B, D), f32)
    bw = h.node_backward_recorded(torch.from_numpy(du).cuda(), w_reg=1.0)
    gx, gpd, gpg = _autograd64(c, inp, T, ref, du, 1.0)
    assert not bw["dx"].cpu().numpy().any()
    assert np.abs(gpd).max() > 0 and np.abs(gpg).max() > 0
    for k, a, b in (("dp_drift", bw["dp_drift"], gpd), ("dp_diff", bw["dp_diff"], gpg)):
        e = _rel(a.cpu().numpy(), b)
        print(f"{case_id(c)}: regulariser alone, {k} rel err {e:.2e} (max |ref| {np.abs(b).max():.3e}), reg_val {ref['reg_val']:.4g}")
        assert e < 2e-5, (k, e)


def test_record_kinds_do_not_mix(oracle, gpu_pkg):
    """an Euler-Heun recorded forward, then a Milstein one, then backward on ONE handle == the Milstein backward on a fresh
    handle; the record's generation advances by one per forward"""
    from localregneuralde_jl_amd import _lib as L
    c = MIL[0]
    inp, T, ref = case_reference(oracle, c, "unbiased")
    D, H, B, nfine = c["shape"]
    du = torch.from_numpy(np.random.default_rng(6).standard_normal((len(ref["t"]), B, D)).astype(f32)).cuda()

    def gen(h):
        g = C.c_uint64()
        assert L.lib.lrnde_sde_record_generation(h._h, C.byref(g)) == 0
        return g.value
    h1 = _handle(gpu_pkg, c, inp)
    g0 = gen(h1)
    _forward(h1, dict(c, kind="EulerHeun"), inp, None, "unbiased")
    assert gen(h1) == g0 + 1
    got = _forward(h1, c, inp, T, "unbiased")
    assert gen(h1) == g0 + 2
    _check_forward(got, ref, "second forward")
    a = h1.node_backward_recorded(du, w_reg=1.5)
    h2 = _handle(gpu_pkg, c, inp)
    _forward(h2, c, inp, T, "unbiased")
    b = h2.node_backward_recorded(du, w_reg=1.5)
    for k in ("dx", "dp_drift", "dp_diff"):
        assert torch.equal(a[k], b[k]), k
    # ... and the other way round: the Euler-Heun sweep after a Milstein forward is the Euler-Heun sweep
    e1 = _forward(h1, dict(c, kind="EulerHeun"), inp, None, "unbiased")
    due = torch.from_numpy(np.random.default_rng(7).standard_normal(tuple(e1["u"].shape)).astype(f32)).cuda()
    a = h1.node_backward_recorded(due, w_reg=1.5)
    h3 = _handle(gpu_pkg, c, inp)
    _forward(h3, dict(c, kind="EulerHeun"), inp, None, "unbiased")
    b = h3.node_backward_recorded(due, w_reg=1.5)
    for k in ("dx", "dp_drift", "dp_diff"):
        assert torch.equal(a[k], b[k]), k


def test_wrong_combinations_return_badarg_with_a_message(oracle, gpu_pkg):
    c = SRI[1]
    inp, T, _ = case_reference(oracle, c, "none")
    h = _handle(gpu_pkg, c, inp)
    dev = lambda a: torch.from_numpy(a).cuda()
    x, W, Z, z = dev(inp["x"]), dev(inp["W"]), dev(inp["Z"]), dev(inp["z"])
    tab = [T[k] for k in S_FIELDS()]
    for kw in (dict(tableau=None, path_z=Z), dict(tableau=tab, path_z=None)):
        with pytest.raises(gpu_pkg.LrndeError) as e:
            h.solve_adaptive(x, W, 0.0, 1.0, 0.5, 0.5, solver="SRI", **kw)
        assert e.value.code == 4 and "SRI" in str(e.value)
        with pytest.raises(gpu_pkg.LrndeError) as e:
            h.node_forward_record(x, W, 0.0, 1.0, 0.5, 0.5, mode="none", solver="SRI", **kw)
        assert e.value.code == 4
    with pytest.raises(gpu_pkg.LrndeError) as e:    # regularising SRI needs the local step's second draw
        h.node_forward_record(x, W, 0.0, 1.0, 0.5, 0.5, mode="unbiased", z_local=z, solver="SRI", tableau=tab, path_z=Z)
    assert e.value.code == 4 and "z2_local" in str(e.value)
    from localregneuralde_jl_amd import _lib as L
    o = L.SdeAdaptOpts(0.5, 0.5, 1.0 / 6.0, 0.1, 0.9, 0.2, 1.125, 0.14, 0.08, 100)
    st, u_end = L.Stats(), torch.empty_like(x)
    for which in (-1, 3):
        rc = L.lib.lrnde_sde_solve_adaptive_alg(h._h, C.c_void_p(x.data_ptr()), C.c_void_p(W.data_ptr()), c["shape"][3], c["shape"][2], 0.0, 1.0,
                                                C.byref(o), C.c_void_p(u_end.data_ptr()), C.byref(st), None, 0, which, None, None)
        assert rc == 4 and b"which" in L.lib.lrnde_sde_last_error(h._h)
    # the plain adaptive solve with the Milstein step: the end state of the layer's solve
    ref = case_reference(oracle, MIL[0], "none")
    hm = _handle(gpu_pkg, MIL[0], ref[0])
    r = hm.solve_adaptive(dev(ref[0]["x"]), dev(ref[0]["W"]), 0.0, 1.0, MIL[0]["tol"], MIL[0]["tol"], dt0=float(ref[2]["dt0"]), solver="RKMil")
    assert np.array_equal(r["u_end"].cpu().numpy(), ref[2]["u"][-1]) and r["stats"]["naccept"] == ref[2]["naccept"]
    assert int(r["trace"]["accepted"].sum()) == ref[2]["naccept"]


def _layer(P, D, H, **kw):
    return P.NeuralDSDE(P.Chain(P.Dense(D, H, "tanh"), P.Dense(H, D)), P.Dense(D, D), noise_source="device", adaptive=True, **kw)


def test_layer_milstein_adaptive_device_noise(gpu_pkg):
    P = gpu_pkg
    D, H, B = 32, 64, 8
    pd, pg = S.sde_params(D, H, 3)
    ps = dict(drift=pd, diffusion=pg)
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((B, D)).astype(f32)).cuda()
    node = _layer(P, D, H, solver="RKMil", regularize="unbiased", abstol=0.8, reltol=0.8, nfine=32)
    st = node.initialstates(np.random.default_rng(0))
    a, sa = node(x, ps, st)
    b, sb = node(x, ps, st)
    assert torch.equal(a.u[-1], b.u[-1]) and sa["reg_val"] == sb["reg_val"] != 0 and sa["nfe_drift"] == sb["nfe_drift"]
    att = a.stats["naccept"] + a.stats["nreject"]
    assert sa["nfe_drift"] == att + 1 + 4 and sa["nfe_diffusion"] == 2 * (att + 1) + 4       # (1, 2) per step, two automatic initial dts
    dx0, dps0, _ = node.pullback(x, ps, st, torch.ones_like(x), w_reg=0.0)
    dx1, dps1, info = node.pullback(x, ps, st, torch.ones_like(x), w_reg=2.0)
    assert torch.isfinite(dx0).all() and (dx0 != 0).any() and torch.equal(dx0, dx1) and info["dx_reg"] is None
    assert not torch.equal(dps0["drift"], dps1["drift"]) and not torch.equal(dps0["diffusion"], dps1["diffusion"])
    assert torch.equal(info["sol"].u[-1], a.u[-1])


def test_layer_sri_adaptive_device_noise_draws_the_second_path_from_stream_4(oracle, gpu_pkg):
    P = gpu_pkg
    D, H, B, nfine = 4, 8, 3, 16
    pd, pg = S.sde_params(D, H, 3)
    ps = dict(drift=pd, diffusion=pg)
    T = S.sri_tableau(oracle, 41, 0.1)
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((B, D)).astype(f32)).cuda()
    node = _layer(P, D, H, solver="SRI", tableau=[T[k] for k in S_FIELDS()], regularize="unbiased", abstol=0.5, reltol=0.5, nfine=nfine)
    st = node.initialstates(np.random.default_rng(0))
    sol, st2 = node(x, ps, st)
    seed = node._draw_seed(copy.deepcopy(st["rng"]))
    hh = f32(f32(1.0) / f32(nfine))
    Zref = PX.path(seed, 4, nfine, B, D, f32(np.sqrt(hh)))
    Zgot = node._last_path_z.cpu().numpy()
    assert Zgot.shape == Zref.shape and np.array_equal(Zgot.view(np.int32), Zref.view(np.int32))
    assert st2["reg_val"] != 0 and torch.isfinite(sol.u[-1]).all() and sol.stats["naccept"] >= 1
    att = sol.stats["naccept"] + sol.stats["nreject"]
    assert st2["nfe_drift"] == st2["nfe_diffusion"] == 4 * (att + 1) + 4
    dx, dps, info = node.pullback(x, ps, st, torch.ones_like(x), w_reg=1.0)
    assert torch.isfinite(dx).all() and (dx != 0).any() and info["dx_reg"] is None
