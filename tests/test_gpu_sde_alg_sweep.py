"""The one-launch reverse sweep of Milstein and SRI records (csrc/lrnde_sde_bwd_alg_fused.hpp; `lrnde_sde_node_backward_recorded`
on a record with which != 0, `lrnde_sde_last_backward_info`).

1. the route is taken: `SdeHandle.last_backward_info()` says kind 1 inside the gate, kind 0 with LRNDE_NO_SDE_BWD_FUSED=1 and
   outside the gate; the number of launches does not depend on the number of recorded steps or on `saveat`;
2. gradients against float64 torch autograd over the recorded grid (tests/sde_alg_sweep_cases.py): 5e-6 of each gradient's norm
   on dx, dp_drift, dp_diff — the project's bound for these reverse passes — and 2e-5 for the regulariser
   alone with dx exactly zero, in every mode and cotangent form;
3. the two routes against each other: rel(route 0, route 1) <= e0 + e1 + 1e-7 per gradient, e0 / e1 being each route's error
   against float64 (the triangle inequality; the last term is the fp32 rounding of the comparison itself);
4. determinism and records; 5. the diffusion without a bias; 6. the MNIST-SDE model's training step with the SRI step.
Every measured error is printed.  tests/test_host_sde_alg_sweep.py shows that the compared gradients react to what the sweep must
get right."""
import copy

import numpy as np
import pytest
import torch

import sde_alg_sweep_cases as AC
import sde_model_cases as MC
from sde_alg_sweep_cases import FORMS, GATE_CORNER, MIL, NOBIAS, SRI, SWEEP_CASES, cid

pytestmark = pytest.mark.gpu
f32 = np.float32
S = AC.S
SWITCH = "LRNDE_NO_SDE_BWD_FUSED"
GRADS = ("dx", "dp_drift", "dp_diff")


def _handle(P, c, inp):
    from localregneuralde_jl_amd.layers import _mlp_desc
    D, H, B, nfine = c["shape"]
    h = P.SdeHandle(_mlp_desc(P.Chain(P.Dense(D, H, "tanh"), P.Dense(H, D))), diffusion_bias=AC.has_bias(c))
    h.set_params(inp["pd"], inp["pg"])
    return h


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tab(T):
    from localregneuralde_jl_amd import _lib as L
    return None if T is None else [T[k] for k in L.SRI_FIELDS]


def _forward(h, c, inp, T, mode="unbiased", t1=0.43, saveat=(), save_start=-1, kind=None):
    kind = kind or c["kind"]
    return h.node_forward_record(_cu(inp["x"]), _cu(inp["W"]), 0.0, 1.0, c["tol"], c["tol"], mode=mode, t1_or_rand=t1, z_local=_cu(inp["z"]),
                                 saveat=saveat, save_start=save_start, dt0=c["dt0"], solver=kind, tableau=_tab(T) if kind == "SRI" else None,
                                 path_z=_cu(inp["Z"]) if kind == "SRI" else None, z_local2=_cu(inp["z2"]) if kind == "SRI" else None)


def _forward_form(h, c, inp, T, form):
    f = FORMS[form]
    return _forward(h, c, inp, T, f["mode"], f["t1"], f["saveat"], f["save_start"])


def _check_forward(got, ref, what):
    assert got["stats"]["naccept"] == ref["naccept"] and got["stats"]["nreject"] == ref["nreject"], (what, got["stats"])
    assert np.array_equal(got["t"], ref["t"]) and got["reg_val"] == ref["reg_val"], what
    assert np.array_equal(got["u"].cpu().numpy(), ref["u"]), what


def _with_switch(P, on, fn):
    P.set_option(SWITCH, 1 if on else 0)
    try:
        return fn()
    finally:
        P.set_option(SWITCH, 0)


def _backward(P, h, du, w_reg, per_step):
    """(gradients as numpy, last_backward_info) of one pullback from the handle's record on the given route"""
    def run():
        bw = h.node_backward_recorded(_cu(du), w_reg=w_reg)
        return {k: bw[k].cpu().numpy() for k in GRADS}, h.last_backward_info()
    return _with_switch(P, per_step, run)


# ---- 1. the route ----
def test_the_one_launch_sweep_is_taken_inside_the_gate_and_says_so(oracle, gpu_pkg):
    P = gpu_pkg
    infos = {}
    for c in (MIL[0], SRI[1], SRI[0]):
        assert AC.sweep_gate(*c["shape"][:2], c["kind"])
        for saveat in ((), (0.3, 0.77, 1.0)):
            inp, T, ref = AC.reference(oracle, c, mode="unbiased", t1_or_rand=0.37, saveat=saveat)
            h = _handle(P, c, inp)
            _check_forward(_forward(h, c, inp, T, "unbiased", 0.37, saveat), ref, cid(c))
            du = np.random.default_rng(5).standard_normal((len(ref["t"]), c["shape"][2], c["shape"][0])).astype(f32)
            _, info = _backward(P, h, du, 2.0, False)
            print(f"{cid(c)} saveat={saveat}: K = {ref['naccept']}, {info}")
            assert info["kind"] == 1 and info["host_waits"] <= 1 and info["launches"] >= 1, info
            infos[(cid(c), bool(saveat))] = (info, ref["naccept"])
            _, off = _backward(P, h, du, 2.0, True)           # the switch selects the per-step route for these kinds too
            assert off["kind"] == 0, off
    # the number of launches depends neither on the number of recorded steps nor on saveat
    assert infos[(cid(SRI[0]), False)][1] != infos[(cid(SRI[1]), False)][1]
    assert len({v[0]["launches"] for k, v in infos.items() if k[0].startswith("SRI")}) == 1, infos
    assert infos[(cid(MIL[0]), False)][0]["launches"] == infos[(cid(MIL[0]), True)][0]["launches"]
    # outside the gate (D = 72): the per-step route
    c = MIL[4]
    assert c["shape"][:2] == (72, 32) and not AC.sweep_gate(72, 32, "RKMil")
    inp, T, ref = AC.reference(oracle, c, mode="unbiased", t1_or_rand=0.37)
    h = _handle(P, c, inp)
    _forward(h, c, inp, T, "unbiased", 0.37)
    du = np.random.default_rng(5).standard_normal((len(ref["t"]), c["shape"][2], c["shape"][0])).astype(f32)
    assert _backward(P, h, du, 2.0, False)[1]["kind"] == 0
    # an Euler-Heun record at (32, 64): its own one-launch sweep, reported by the same hook
    c = MIL[0]
    inp, T, _ = AC.reference(oracle, c, mode="unbiased", t1_or_rand=0.37)
    h = _handle(P, c, inp)
    e = _forward(h, dict(c, tol=0.14), inp, None, "unbiased", 0.37, kind="EulerHeun")
    du = np.random.default_rng(5).standard_normal(tuple(e["u"].shape)).astype(f32)
    _, info = _backward(P, h, du, 2.0, False)
    assert info["kind"] == 1 and info["host_waits"] <= 1 and info["launches"] >= 2, info
    assert _backward(P, h, du, 2.0, True)[1]["kind"] == 0


# ---- 2. and 3.: both routes against float64 autograd over the recorded grid, and against each other ----
_RUNS = {}


def _both_routes(P, O, c, form, reg_alone=False):
    """one forward, the pullback on both routes, the float64 reference: computed once per (case, form)"""
    key = (cid(c), form, reg_alone)
    if key in _RUNS:
        return _RUNS[key]
    f = FORMS[form]
    if reg_alone:      # an explicit first step: the automatic one makes reg_val ~ 1e-6 (tests/test_gpu_sde_adaptive_alg.py)
        c = dict(c, dt0=0.05)
    inp, T, ref = AC.reference(O, c, form)
    h = _handle(P, c, inp)
    got = _forward_form(h, c, inp, T, form)
    _check_forward(got, ref, f"{cid(c)} {form}")
    assert ref["naccept"] >= 3
    du = AC.cotangents(c, ref, form)
    w_reg = f["w_reg"]
    if reg_alone:
        du[:] = 0
        w_reg = 1.0
        assert float(ref["reg_val"]) > 1e-6
    g1, info1 = _backward(P, h, du, w_reg, False)
    g0, info0 = _backward(P, h, du, w_reg, True)
    r64 = dict(zip(GRADS, AC.autograd64(c, inp, T, ref, du, w_reg)))
    out = dict(ref=ref, g0=g0, g1=g1, info0=info0, info1=info1, r64=r64,
               e0={k: AC._rel(g0[k], r64[k]) for k in GRADS}, e1={k: AC._rel(g1[k], r64[k]) for k in GRADS},
               e01={k: AC._rel(g0[k], g1[k]) for k in GRADS})
    _RUNS[key] = out
    return out


def _expect_kind(c):
    return 1 if AC.sweep_gate(*c["shape"][:2], c["kind"]) else 0


ALL = SWEEP_CASES + [GATE_CORNER]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("c", ALL, ids=cid)
def test_gradients_match_float64_autograd_over_the_recorded_grid(oracle, gpu_pkg, c, form):
    """bound 5e-6 of each gradient's norm on dx, dp_drift, dp_diff, on the route the gate gives the case"""
    r = _both_routes(gpu_pkg, oracle, c, form)
    ref = r["ref"]
    if c in SWEEP_CASES:
        assert _expect_kind(c) == 1
    assert r["info1"]["kind"] == _expect_kind(c), (r["info1"], AC.sweep_lds_bytes(*c["shape"][:2], c["kind"]))
    assert r["info0"]["kind"] == 0
    if form == "saveat-interpolated":
        assert any(0.0 < float(th) < 1.0 for (_, k, th) in ref["series"])
    if form == "saveat-with-start":
        assert any(k < 0 for (_, k, th) in ref["series"])
    if c is MIL[5] or c is SRI[2]:
        assert ref["nreject"] >= 1                   # a record slot was rewritten
    print(f"{cid(c)} {form}: K = {ref['naccept']}, rejected {ref['nreject']}, series {len(ref['t'])}, route kind {r['info1']['kind']} "
          f"({r['info1']['launches']} launches, {r['info1']['host_waits']} waits); rel err vs float64 autograd " +
          ", ".join(f"{k} {v:.2e}" for k, v in r["e1"].items()))
    for k, v in r["e1"].items():
        assert np.abs(r["r64"][k]).max() > 0 and v < 5e-6, (k, v)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("c", ALL, ids=cid)
def test_the_two_routes_agree_within_their_errors_against_float64(oracle, gpu_pkg, c, form):
    r = _both_routes(gpu_pkg, oracle, c, form)
    for k in GRADS:
        lim = r["e0"][k] + r["e1"][k] + 1e-7
        print(f"{cid(c)} {form} {k}: rel(route 0, route 1) {r['e01'][k]:.2e}; e0 {r['e0'][k]:.2e}, e1 {r['e1'][k]:.2e}, bound {lim:.2e}")
        assert r["e01"][k] <= lim, (k, r["e01"][k], lim)


@pytest.mark.parametrize("c", [MIL[0], MIL[2], SRI[0], SRI[1]], ids=cid)
def test_regulariser_alone(oracle, gpu_pkg, c):
    """zero cotangents on the series, w_reg = 1, explicit dt0 = 0.05: d reg_val / d ps within 2e-5 of float64 autograd on the
    sweep's route, d reg_val / d x exactly zero; the two routes agree within their errors"""
    r = _both_routes(gpu_pkg, oracle, c, "unbiased-w2", reg_alone=True)
    assert r["info1"]["kind"] == 1 and r["info0"]["kind"] == 0
    assert not r["g1"]["dx"].any() and not r["g0"]["dx"].any()
    for k in ("dp_drift", "dp_diff"):
        assert np.abs(r["r64"][k]).max() > 0
        lim = r["e0"][k] + r["e1"][k] + 1e-7
        print(f"{cid(c)} regulariser alone {k}: e1 {r['e1'][k]:.2e} (route 0: {r['e0'][k]:.2e}), rel(route 0, route 1) {r['e01'][k]:.2e}, "
              f"reg_val {r['ref']['reg_val']:.4g}")
        assert r["e1"][k] < 2e-5, (k, r["e1"][k])
        assert r["e01"][k] <= lim, (k, r["e01"][k], lim)


# ---- 4. determinism and records ----
def test_the_same_backward_twice_gives_equal_bits_and_record_kinds_do_not_mix(oracle, gpu_pkg):
    P = gpu_pkg
    cs, cm = SRI[0], MIL[0]
    inps, Ts, refs = AC.reference(oracle, cs, "unbiased-w2")
    inpm, Tm, refm = AC.reference(oracle, cm, "unbiased-w2")
    assert cs["shape"][:2] == cm["shape"][:2]
    dus = AC.cotangents(cs, refs, "unbiased-w2")
    dum = AC.cotangents(cm, refm, "unbiased-w2")
    h = _handle(P, cs, inps)
    _forward_form(h, cs, inps, Ts, "unbiased-w2")
    a, ia = _backward(P, h, dus, 1.5, False)
    b, ib = _backward(P, h, dus, 1.5, False)
    assert ia["kind"] == ib["kind"] == 1 and ia == ib
    for k in GRADS:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    # a Milstein record after the SRI record on one handle == the Milstein backward on a fresh handle
    h.set_params(inpm["pd"], inpm["pg"])
    h1 = h
    _forward_form(h1, cm, inpm, Tm, "unbiased-w2")
    m1, i1 = _backward(P, h1, dum, 1.5, False)
    h2 = _handle(P, cm, inpm)
    _forward_form(h2, cm, inpm, Tm, "unbiased-w2")
    m2, i2 = _backward(P, h2, dum, 1.5, False)
    assert i1["kind"] == i2["kind"] == 1
    for k in GRADS:
        assert np.array_equal(m1[k].view(np.int32), m2[k].view(np.int32)), k


def test_a_backward_without_a_usable_record_is_refused_as_before(oracle, gpu_pkg):
    P = gpu_pkg
    c = SRI[1]
    inp, T, ref = AC.reference(oracle, c, "unbiased-w2")
    D, H, B, nfine = c["shape"]
    du = AC.cotangents(c, ref, "unbiased-w2")
    h = _handle(P, c, inp)
    with pytest.raises(P.LrndeError, match=r"no forward record"):
        h.node_backward_recorded(_cu(du), w_reg=1.0)
    _forward_form(h, c, inp, T, "unbiased-w2")
    with pytest.raises(P.LrndeError, match=r"cotangents for a series"):          # a cotangent count of another series
        h.node_backward_recorded(_cu(np.concatenate([du, du[:1]])), w_reg=1.0)
    first, _ = _backward(P, h, du, 1.0, False)
    # the single-step SRI pullback uses the record's scratch: it consumes the record
    x, w, z = _cu(inp["x"]), _cu(inp["W"][1]), _cu(inp["Z"][1])
    h.sri_step_backward(_tab(T), x, w, z, 0.0, 1.0 / nfine, c["tol"], c["tol"], 1.0 / 6.0, du_new=torch.ones_like(x))
    with pytest.raises(P.LrndeError, match=r"no forward record"):
        h.node_backward_recorded(_cu(du), w_reg=1.0)
    _forward_form(h, c, inp, T, "unbiased-w2")
    again, info = _backward(P, h, du, 1.0, False)
    assert info["kind"] == 1 and all(np.array_equal(first[k], again[k]) for k in GRADS)


def test_a_record_whose_scratch_the_per_step_sri_route_used_is_not_swept_with_a_regulariser(oracle, gpu_pkg):
    """the per-step SRI route recomputes every step's u' into the record's scratch, where the forward left the local step's u';
    the sweep's regulariser kernel reads that u'.  After such a pullback the same record takes the per-step route again when a
    regulariser is asked for (and says so), the sweep without one, and the sweep again after a new forward."""
    P = gpu_pkg
    c = SRI[1]
    inp, T, ref = AC.reference(oracle, c, "unbiased-w2")
    du = AC.cotangents(c, ref, "unbiased-w2")
    h = _handle(P, c, inp)
    _forward_form(h, c, inp, T, "unbiased-w2")
    want, info = _backward(P, h, du, 1.5, False)
    assert info["kind"] == 1
    _backward(P, h, du, 0.0, True)                      # the per-step route, no regulariser: the scratch holds step 0's u'
    got, info = _backward(P, h, du, 1.5, False)
    assert info["kind"] == 0
    r64 = dict(zip(GRADS, AC.autograd64(c, inp, T, ref, du, 1.5)))
    for k in GRADS:                                     # (two routes: within their errors against float64, not the same bits)
        assert AC._rel(got[k], want[k]) <= AC._rel(got[k], r64[k]) + AC._rel(want[k], r64[k]) + 1e-7, k
        assert AC._rel(got[k], r64[k]) < 5e-6, k
    assert _backward(P, h, du, 0.0, False)[1]["kind"] == 1
    _forward_form(h, c, inp, T, "unbiased-w2")
    again, info = _backward(P, h, du, 1.5, False)
    assert info["kind"] == 1 and all(np.array_equal(again[k], want[k]) for k in GRADS)


# ---- 5. diffusion without a bias ----
@pytest.mark.parametrize("c", NOBIAS, ids=cid)
def test_diffusion_without_a_bias(oracle, gpu_pkg, c):
    D = c["shape"][0]
    r = _both_routes(gpu_pkg, oracle, c, "unbiased-w2")
    assert r["info1"]["kind"] == 1 and r["info0"]["kind"] == 0
    assert r["g1"]["dp_diff"].shape == (D * D,) and r["g0"]["dp_diff"].shape == (D * D,)
    for k in GRADS:
        lim = r["e0"][k] + r["e1"][k] + 1e-7
        print(f"{cid(c)} {k}: e1 {r['e1'][k]:.2e}, e0 {r['e0'][k]:.2e}, rel(route 0, route 1) {r['e01'][k]:.2e}, bound {lim:.2e}")
        assert r["e1"][k] < 5e-6, (k, r["e1"][k])
        assert r["e01"][k] <= lim, (k, r["e01"][k], lim)


# ---- 6. the model ----
def test_the_sri_training_step_inherits_the_sweep(oracle, gpu_pkg):
    """run_sde_training_step with construct_mlp_sde(..., solver="SRI") at (784 -> 32, H 64, B 24): with the switch 0 / 1 the loss
    and y_pred are the same bits (the forward is untouched) and the three gradient groups agree within their errors against the
    float64 model reference.  lrnde_sde_model_backward_recorded sets defer_wait around the layer's pullback, so the sweep reports
    no synchronisation of its own: host_waits == 0 (the model call's one wait covers it)."""
    P, O = gpu_pkg, oracle
    Din, D, H, K, B, tol, nfine, w_reg = 784, 32, 64, 10, 24, 0.14, 64, 2.0
    c = MC.model_case(Din, D, H, K, B, nfine, seed=21, kind="SRI")
    T = S.sri_tableau(O, 41, 0.1)
    model = P.construct_mlp_sde(in_dims=Din, state_dims=D, hidden_dims=H, num_classes=K, abstol=tol, reltol=tol, nfine=nfine, solver="SRI",
                                tableau=_tab(T), adaptive=True)
    ps = dict(downsample=_cu(c["pds"]), neural_dsde=dict(drift=_cu(c["pd"]), diffusion=_cu(c["pg"])), classifier=_cu(c["pc"]))
    st = model.initialstates(np.random.default_rng(5))
    x, lab = _cu(c["x"]), _cu(c["labels"])
    draws = dict(path=_cu(c["W"]), z_local=_cu(c["z"]), path_z=_cu(c["Z"]), z_local2=_cu(c["z2"]))
    h = model.neural_dsde.handle()

    def step():
        loss, _, stats, grads, _ = P.run_sde_training_step(model, ps, st, x, lab, w_reg, **draws)
        return loss, stats, grads, h.last_backward_info()
    l1, s1, g1, i1 = _with_switch(P, False, step)
    l0, s0, g0, i0 = _with_switch(P, True, step)
    assert i1["kind"] == 1 and i1["host_waits"] == 0 and i0["kind"] == 0, (i1, i0)
    assert l1 == l0 and torch.equal(s1["y_pred"], s0["y_pred"]) and s1["reg_val"] == s0["reg_val"] != 0
    assert torch.equal(g1["classifier"], g0["classifier"])
    # the float64 reference over the grid the step recorded: the t1 the step drew (seed first: the device noise source), the oracle's
    # loop fed the device's u0
    rng = copy.deepcopy(st["neural_dsde"]["rng"])
    rng.integers(0, 2 ** 64, dtype=np.uint64)
    t1 = f32(f32(rng.random(dtype=np.float32)) * f32(1.0) + f32(0.0))
    u0 = h.dense_forward(x, ps["downsample"]).cpu().numpy()
    drift, diff = S.oracle_fields(O, D, H, c["pd"], c["pg"])
    ref = S.sde_node_forward(O, "SRI", drift, diff, u0, c["W"], 0.0, 1.0, tol, tol, mode="unbiased", t1_or_rand=float(t1), z_local=c["z"],
                             saveat=(), save_start=0, dt0=0.0, tableau=T, Z=c["Z"], z2_local=c["z2"])
    assert ref["reg_val"] == s1["reg_val"] and ref["naccept"] >= 3
    r64 = MC.model_reference(c, ref, D, H, K, w_reg, tol, torch.float64, kind="SRI", tableau=T)
    for name, a1, a0, key in (("downsample", g1["downsample"], g0["downsample"], "d_downsample"),
                              ("drift", g1["neural_dsde"]["drift"], g0["neural_dsde"]["drift"], "d_drift"),
                              ("diffusion", g1["neural_dsde"]["diffusion"], g0["neural_dsde"]["diffusion"], "d_diffusion")):
        a1, a0 = a1.cpu().numpy(), a0.cpu().numpy()
        e1, e0, e01 = AC._rel(a1, r64[key]), AC._rel(a0, r64[key]), AC._rel(a0, a1)
        print(f"SRI model step {name}: e1 {e1:.2e}, e0 {e0:.2e}, rel(route 0, route 1) {e01:.2e}, bound {e0 + e1 + 1e-7:.2e}; K = {ref['naccept']}, {i1}")
        assert e01 <= e0 + e1 + 1e-7, (name, e01, e0, e1)


def test_the_layer_pullback_says_which_route_ran(oracle, gpu_pkg):
    P = gpu_pkg
    D, H, B = 32, 64, 8
    pd, pg = S.sde_params(D, H, 3)
    ps = dict(drift=pd, diffusion=pg)
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((B, D)).astype(f32)).cuda()
    node = P.NeuralDSDE(P.Chain(P.Dense(D, H, "tanh"), P.Dense(H, D)), P.Dense(D, D), noise_source="device", adaptive=True, solver="RKMil",
                        regularize="unbiased", abstol=0.8, reltol=0.8, nfine=32)
    st = node.initialstates(np.random.default_rng(0))
    dx1, dps1, info1 = node.pullback(x, ps, st, torch.ones_like(x), w_reg=2.0)
    dx0, dps0, info0 = _with_switch(P, True, lambda: node.pullback(x, ps, st, torch.ones_like(x), w_reg=2.0))
    assert info1["backward"]["kind"] == 1 and info0["backward"]["kind"] == 0
    assert torch.isfinite(dx1).all() and (dx1 != 0).any()
    assert AC._rel(dx1.cpu().numpy(), dx0.cpu().numpy()) < 1e-5 and AC._rel(dps1["drift"].cpu().numpy(), dps0["drift"].cpu().numpy()) < 1e-5
