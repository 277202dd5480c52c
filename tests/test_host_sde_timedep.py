"""The SDE stack with a time-dependent drift — CPU side: the yardstick of tests/test_gpu_sde_timedep.py is pinned here.

* the C oracle's three steps with a TDChain drift against the float64 steps of tests/sde_timedep_cases.py, which evaluate the
  drift at the reference's times (src/perform_step.jl:174-193, :127, :62-84): u within 1e-6 of its norm, reg_val within 1e-5.
* time is OBSERVABLE on these inputs, shown on the float64 steps alone: the step with wrong times (Euler-Heun: t for t + dt; SRI:
  every stage at t, and c0j <-> c1j; Milstein, whose every live evaluation is at t: t against t + 0.1) differs from the right one
  by at least 1e-3 of the norm.  A case that falls below gets another seed, never another bound.
* the adaptive loop (tests/sde_adaptive_np.py) over a time-dependent drift, one case per step kind, pinned as
  tests/test_host_sde_adaptive.py pins its cases; every case rejects a step, so a step after a rejection carries a time.
* the float64 gradient over the recorded grid moves by at least 1e-3 of its norm when every step's start time i h and the local
  step's t1 are replaced by t0: the pullback tests can see the times.
* the SRI contract inputs have at least 25 % of their entries on each side of |uprev| >= |u'|."""
import numpy as np
import pytest
import torch

import sde_adaptive_np as S
import sde_timedep_cases as TC

f32 = np.float32
t, dt = TC.T_STEP, TC.DT_STEP


def _setup(oracle, c):
    D, H, B = c
    inp = TC.step_inputs(D, H, B)
    drift, diff = TC.oracle_fields(oracle, D, H, inp["pd"], inp["pg"])
    f, g = TC.fields64(TC.tt(inp["pd"]), TC.tt(inp["pg"]), D, H)
    return inp, drift, diff, f, g, TC.tt(inp["x"]), TC.tt(inp["dW"]), TC.tt(inp["dZ"])


def _check(ref, un, reg, what):
    eu = TC.rel(ref["u"], un.numpy())
    er = abs(float(ref["reg_val"]) - float(reg)) / abs(float(reg))
    assert ref["reg_val"] == f32(ref["eest"] * f32(dt))
    print(f"{what}: oracle vs float64, u {eu:.2e} (bound 1e-6), reg_val {er:.2e} (bound 1e-5)")
    assert eu < 1e-6 and er < 1e-5, (what, eu, er)


def _margin(right, wrong, what):
    m = TC.rel(wrong.numpy(), right.numpy())
    print(f"{what}: wrong times move the float64 step by {m:.2e} of its norm (at least 1e-3)")
    assert m >= 1e-3, (what, m)


@pytest.mark.parametrize("c", TC.STEP_CASES, ids=TC.step_id)
def test_euler_heun_step_with_a_time_dependent_drift(oracle, c):
    inp, drift, diff, f, g, x, dW, _ = _setup(oracle, c)
    ref = oracle.euler_heun_step(drift, diff, inp["x"], inp["dW"], t, dt, TC.TOL, TC.TOL, TC.DELTA)
    un, reg = TC.eh_step64(f, g, x, dW, t, dt)
    _check(ref, un, reg, f"euler-heun {TC.step_id(c)}")
    _margin(un, TC.eh_step64(f, g, x, dW, t, dt, times=(t, t, t))[0], f"euler-heun {TC.step_id(c)}, t for t + dt")


@pytest.mark.parametrize("c", TC.STEP_CASES, ids=TC.step_id)
def test_milstein_step_with_a_time_dependent_drift(oracle, c):
    inp, drift, diff, f, g, x, dW, _ = _setup(oracle, c)
    ref = oracle.rkmil_step(drift, diff, inp["x"], inp["dW"], t, dt, TC.TOL, TC.TOL)
    un, reg = TC.mil_step64(f, g, x, dW, t, dt)
    _check(ref, un, reg, f"milstein {TC.step_id(c)}")
    _margin(un, TC.mil_step64(f, g, x, dW, t, dt, times=(t + 0.1,))[0], f"milstein {TC.step_id(c)}, t + 0.1 for t")


@pytest.mark.parametrize("c", TC.STEP_CASES, ids=TC.step_id)
def test_sri_step_with_a_time_dependent_drift(oracle, c):
    inp, drift, diff, f, g, x, dW, dZ = _setup(oracle, c)
    T = TC.sri_tableau(TC.TAB_SEED)
    cs = sorted(T[k] for k in TC.C_NAMES)
    assert min(abs(v) for v in cs) > 0.05 and min(b - a for a, b in zip(cs, cs[1:])) > 0.05
    ref = oracle.sri_step(drift, diff, T, inp["x"], inp["dW"], inp["dZ"], t, dt, TC.TOL, TC.TOL, TC.DELTA)
    un, reg = TC.sri_step64(f, g, T, x, dW, dZ, t, dt)
    _check(ref, un, reg, f"sri {TC.step_id(c)}")
    _margin(un, TC.sri_step64(f, g, T, x, dW, dZ, t, dt, times=(t, t, t, t))[0], f"sri {TC.step_id(c)}, every stage at t")
    _margin(un, TC.sri_step64(f, g, T, x, dW, dZ, t, dt, times=TC.sri_times_swapped(T, t, dt))[0], f"sri {TC.step_id(c)}, c0j <-> c1j")


@pytest.mark.parametrize("c", TC.CONTRACT_CASES, ids=TC.step_id)
def test_sri_contract_inputs_fall_on_both_sides_of_the_scale(oracle, c):
    """the residual's scale abstol + max(|uprev|, |u'|) reltol takes its derivative from uprev on one side and from u' on the
    other: at least a quarter of the entries on each; and dropping the uprev side from autograd moves dx (du_new set, w_reg = 1) by more than
    1e-4 of its norm, ten times the bound the device test holds it to"""
    inp, _, _, _, _, _, dW, dZ = _setup(oracle, c)
    D, H, B = c
    T = TC.sri_tableau(TC.TAB_SEED)
    grads = []
    for side in (True, False):
        pdt, pgt, xt = TC.leaves(inp)
        f, g = TC.fields64(pdt, pgt, D, H)
        un, reg = TC.sri_step64(f, g, T, xt, dW, dZ, t, dt, scale_up_side=side)
        ((un * TC.tt(inp["du"])).sum() + reg).backward()
        grads.append(xt.grad.numpy())
    share = float((xt.detach().abs() >= un.detach().abs()).double().mean())
    print(f"sri contract {TC.step_id(c)}: {100 * share:.0f} % of the entries have |uprev| >= |u'|; without that side of the scale dx "
          f"(du_new set, w_reg = 1) is off by {TC.rel(grads[1], grads[0]):.2e}")
    assert 0.25 <= share <= 0.75, share
    assert TC.rel(grads[1], grads[0]) > 1e-4


# ---- the adaptive loop ----------------------------------------------------------------------------------------------------
def test_helper_with_the_euler_heun_step_is_the_oracle_loop_on_a_time_dependent_drift(oracle):
    c = TC.ADAPTIVE_CASES[0]
    assert c["kind"] == "EulerHeun"
    D, H, B, nfine = c["shape"]
    for mode in TC.MODES:
        inp, _, a = TC.adaptive_reference(oracle, c, mode)
        drift, diff = TC.oracle_fields(oracle, D, H, inp["pd"], inp["pg"])
        b = oracle.sde_node_forward(drift, diff, inp["x"], inp["W"], TC.T0, TC.T2, c["tol"], c["tol"], mode=mode, t1_or_rand=TC.T1,
                                    z_local=inp["z"], dt0=c["dt0"])
        assert a["dZ_local"] is None and set(a) == set(b) | {"dZ_local"}
        for k, vb in b.items():
            va = a[k]
            if vb is None:
                assert va is None, k
            elif isinstance(vb, np.ndarray):
                assert va.dtype == vb.dtype and va.shape == vb.shape and np.array_equal(va, vb), k
            elif k in ("steps", "series"):
                assert len(va) == len(vb) and all(tuple(x) == tuple(y) for x, y in zip(va, vb)), k
            else:
                assert type(va) is type(vb) and va == vb, (k, va, vb)


@pytest.mark.parametrize("c", TC.ADAPTIVE_CASES, ids=TC.adaptive_id)
def test_adaptive_cases_end_ok_reject_a_step_and_go_on_after_it(oracle, c):
    nf, ng = S.KINDS[c["kind"]]["nf"], S.KINDS[c["kind"]]["ng"]
    nfine = c["shape"][3]
    assert nfine in (32, 64)
    for mode in TC.MODES:
        _, _, r = TC.adaptive_reference(oracle, c, mode)       # (raises on MaxIters / DtLessThanMin / DtNaN)
        assert r["naccept"] >= 3 and r["nreject"] >= 1, (mode, r["naccept"], r["nreject"])
        assert np.isfinite(r["u"]).all() and (r["reg_val"] > 0) == (mode != "none")
        att, loc = r["naccept"] + r["nreject"], 0 if mode == "none" else 1
        assert r["nfe_drift"] == nf * (att + loc) and r["nfe_diffusion"] == ng * (att + loc)      # explicit dt0: no automatic one
        assert sum(m for _, m in r["steps"]) == nfine
        assert r["steps"][0][1] < max(int(c["dt0"] * nfine), 1)      # the first accepted step is shorter than the one asked for
        assert any(i > 0 for i, _ in r["steps"])                       # ... and steps after it start at times other than t0
        if mode == "unbiased":
            assert TC.T0 < float(r["t1"]) == float(f32(TC.T1)) < TC.T2
        print(f"{TC.adaptive_id(c)} {mode}: accepted {r['naccept']}, rejected {r['nreject']}, reg_val {r['reg_val']:.4g}, t1 {r['t1']:.4g}")


@pytest.mark.parametrize("c", TC.ADAPTIVE_CASES, ids=TC.adaptive_id)
def test_adaptive_loop_sees_the_times(oracle, c):
    """the same loop over the same inputs with the drift's time frozen at t0 ends elsewhere: the forward comparison sees the times"""
    D, H, B, nfine = c["shape"]
    inp, T, r = TC.adaptive_reference(oracle, c, "none")
    drift, diff = TC.oracle_fields(oracle, D, H, inp["pd"], inp["pg"])
    step = S.make_step(oracle, c["kind"], drift, diff, c["tol"], c["tol"], TC.DELTA, T)
    hh = f32(f32(TC.T2 - TC.T0) / f32(nfine))
    u = v = inp["x"]
    for (i, m) in r["steps"]:
        dW = (inp["W"][i + m] - inp["W"][i]).astype(f32)
        dZ = None if inp["Z"] is None else (inp["Z"][i + m] - inp["Z"][i]).astype(f32)
        u = step(u, dW, dZ, f32(TC.T0 + f32(i) * hh), f32(f32(m) * hh))["u"]
        v = step(v, dW, dZ, f32(TC.T0), f32(f32(m) * hh))["u"]
    assert np.array_equal(u, r["u"][-1])
    m_ = TC.rel(v, u)
    print(f"{TC.adaptive_id(c)}: every recorded step at t0 moves the end state by {m_:.2e} of its norm")
    assert m_ >= 1e-3


@pytest.mark.parametrize("c", TC.ADAPTIVE_CASES, ids=TC.adaptive_id)
def test_recorded_grid_gradient_sees_the_times(oracle, c):
    """float64 autograd over the recorded grid (user saveat with an interpolated entry, w_reg = 2): each step at its own start
    time t0 + i h, the local step at t1; all of them at t0 instead moves every gradient by at least 1e-3 of its norm"""
    inp, T, ref = TC.adaptive_reference(oracle, c, "unbiased", saveat=TC.SAVEAT)
    assert any(0.0 < float(th) < 1.0 for (_, k, th) in ref["series"])
    D, H, B, nfine = c["shape"]
    du = np.random.default_rng(5).standard_normal((len(ref["t"]), B, D)).astype(f32)
    right = TC.adaptive_autograd64(c, inp, T, ref, du, 2.0)
    wrong = TC.adaptive_autograd64(c, inp, T, ref, du, 2.0, all_at_t0=True)
    for name, a, b in zip(("dx", "dp_drift", "dp_diff"), right, wrong):
        m_ = TC.rel(b, a)
        print(f"{TC.adaptive_id(c)}: {name} moves by {m_:.2e} of its norm with every time at t0")
        assert m_ >= 1e-3, (name, m_)
    # the regulariser alone: the local step's t1
    zero = np.zeros_like(du)
    right = TC.adaptive_autograd64(c, inp, T, ref, zero, 1.0)
    wrong = TC.adaptive_autograd64(c, inp, T, ref, zero, 1.0, all_at_t0=True)
    assert not right[0].any()
    for name, a, b in zip(("dp_drift", "dp_diff"), right[1:], wrong[1:]):
        m_ = TC.rel(b, a)
        print(f"{TC.adaptive_id(c)}: regulariser alone, {name} moves by {m_:.2e} with the local step at t0")
        assert m_ >= 1e-3, (name, m_)


def test_layer_constructor_accepts_a_tdchain_drift():
    import lrnde_amd as P
    D, H = 4, 8
    node = P.NeuralDSDE(P.TDChain(P.Chain(P.Dense(D + 1, H, "tanh"), P.Dense(H + 1, D))), P.Dense(D, D), solver="RKMil", adaptive=True)
    assert node.desc.time_dep == 1 and node.desc.state_dim == D and node.desc.hidden_dim == H
