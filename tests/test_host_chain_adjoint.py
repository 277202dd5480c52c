"""Host side of the chain handle's device-controlled adjoint: the hook's declaration, the documented info key, and the
error of the float64 yardstick tests/test_gpu_chain_adjoint.py holds the 49-time series to, and the pins of the
float64 restatement of the pullback (tests/chain_adjoint_np.py) that the GPU tests hold both adjoint loops to.  No GPU
needed."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_last_adjoint_info_is_a_hook_not_part_of_the_main_header():
    hooks = open(os.path.join(ROOT, "include", "lrnde_hooks.h")).read()
    main = open(os.path.join(ROOT, "include", "lrnde.h")).read()
    assert re.search(r"int\s+lrnde_last_adjoint_info\s*\(\s*lrnde_ctx\s*\*", hooks)
    assert "lrnde_last_adjoint_info" not in main
    import lrnde_amd  # noqa: F401
    from localregneuralde_jl_amd import _lib as L
    assert "lrnde_last_adjoint_info" in [s[0] for s in L.SYMBOLS]


def test_pullback_documents_the_adjoint_loop_key():
    import lrnde_amd as P
    doc = inspect.getdoc(P.NeuralODE.pullback)
    assert "info['adjoint_loop']" in doc
    for name in ('"host"', '"device"', '"chain_device"'):
        assert name in doc
    from localregneuralde_jl_amd.layers import Handle
    assert Handle.ADJOINT_LOOPS == ("host", "device", "chain_device") and callable(Handle.last_adjoint_info)


def test_chain_adjoint_kernel_args_are_value_initialised():
    src = open(os.path.join(ROOT, "localregneuralde.jl_amd", "csrc", "lrnde_kernels.hip")).read()
    for decl in ("ChAdjArgs a{};", "ChAdjBegin b{};"):
        assert decl in src


def test_float64_yardstick_of_the_49_time_series_agrees_with_itself():
    """RK4 with 196 and with 245 steps (both divisible by 49): the two float64 gradients agree to well under the 3e-4 the
    GPU results are held to, so the yardstick's own error does not eat the bound"""
    import lrnde_amd as P
    ACT = torch.tanh
    model = P.Chain(P.Activation("tanh"), *[P.Dense(20, 40, "tanh") if i % 2 == 0 else P.Dense(40, 20, "tanh") for i in range(8)])
    B = 12
    p = P.glorot_chain_params(model, seed=0, scale=1.5)
    p = (p + np.random.default_rng(1).standard_normal(p.size).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    x = (np.random.default_rng(2).random((B, 20), dtype=np.float32) - np.float32(0.5)) * np.float32(2)
    times = [(i + 1) / 49.0 for i in range(49)]
    cots = np.random.default_rng(13).standard_normal((49, B, 20)).astype(np.float32)

    def grads(nsteps):
        pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
        xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
        Wb, o = [], 0
        for l in model.layers[1:]:
            i, n = l.in_dims, l.out_dims
            Wb.append((pt[o:o + n * i].reshape(i, n).T, pt[o + n * i:o + n * i + n]))
            o += n * i + n

        def f(u):
            h = ACT(u)
            for W, b in Wb:
                h = ACT(h @ W.T + b)
            return h
        h, u, loss = 1.0 / nsteps, xt, 0.0
        marks = {int(round(t * nsteps)): i for i, t in enumerate(times)}
        assert len(marks) == 49
        for k in range(nsteps):
            k1 = f(u); k2 = f(u + 0.5 * h * k1); k3 = f(u + 0.5 * h * k2); k4 = f(u + h * k3)
            u = u + (h / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)
            if k + 1 in marks:
                loss = loss + (u * torch.tensor(cots[marks[k + 1]], dtype=torch.float64)).sum()
        loss.backward()
        return xt.grad.numpy(), pt.grad.numpy()

    (gx1, gp1), (gx2, gp2) = grads(196), grads(245)
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))
    print(f"RK4 196 vs 245 steps: dx {rel(gx1, gx2):.2e} dp {rel(gp1, gp2):.2e}")
    assert rel(gx1, gx2) < 3e-6 and rel(gp1, gp2) < 3e-6


# ---- the restatement of the pullback (tests/chain_adjoint_np.py) ----------------------------------------------------
def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _rk4_case(P, name):
    """(model, p, x, times, save_start, cots, (coarse, fine) RK4 resolutions)"""
    from test_gpu_chain import mk_inputs, physionet, shapes
    if name == "td3_gelu":
        model, B, times, ns = shapes(P)["td3_gelu"], 9, [0.5, 1.0], (200, 400)
    else:
        model, B = physionet(P), 12
        times, ns = {"physionet_3": ([0.25, 0.5, 1.0], (200, 400)), "physionet_t0": ([0.0, 0.5, 1.0], (200, 400)),
                     "physionet_49": ([(i + 1) / 49.0 for i in range(49)], (196, 392))}[name]
    p, x = mk_inputs(P, model, B, scale=1.5)
    cots = np.random.default_rng(13).standard_normal((len(times),) + x.shape).astype(np.float32)
    return model, p, x, times, times[0] == 0.0, cots, ns


# measured rel(restatement at tol 1e-8, RK4) of (dx, dp) at the coarse / fine RK4 resolution; the bound is 4 x the larger
RK4_MEASURED = {
    "physionet_3": ((2.25e-07, 3.33e-07), (2.26e-07, 3.33e-07)),    # RK4 200 / 400 steps
    "physionet_49": ((2.84e-06, 3.44e-06), (2.84e-06, 3.45e-06)),   # RK4 196 / 392 steps
    "physionet_t0": ((2.38e-07, 3.29e-07), (2.38e-07, 3.29e-07)),   # a cotangent at t0 (save_start)
    "td3_gelu": ((2.28e-07, 2.57e-07), (2.28e-07, 2.57e-07)),       # TDChain 32/64/64/32, gelu
}


@pytest.mark.parametrize("name", list(RK4_MEASURED))
def test_restatement_gradients_vs_float64_rk4_autograd(name):
    """The restatement at tol 1e-8 (its own truncation out of the way) against float64 autograd through RK4 at two
    resolutions.  Measured rel of (dx, dp), coarse / fine RK4: PhysioNet 3 times 2.25e-7, 3.33e-7 / 2.26e-7, 3.33e-7;
    49 times 2.84e-6, 3.44e-6 / 2.84e-6, 3.45e-6 (481 accepted steps of a float32 state at tol 1e-8: rounding, not
    truncation); with t0 2.38e-7, 3.29e-7 / 2.38e-7, 3.29e-7; TDChain gelu 2.28e-7, 2.57e-7 / 2.28e-7, 2.57e-7.  The two
    resolutions agree, so what is left is the restatement's float32 state.  The bound is 4 x the larger measured value
    of the case (RK4_MEASURED), at least twenty times below the 3e-4 of the GPU tests."""
    import lrnde_amd as P
    import chain_adjoint_np as CA
    from test_gpu_chain_adjoint import reference_grads
    model, p, x, times, save_start, cots, ns = _rk4_case(P, name)
    r = CA.pullback(model, p, x, times, cots, 1e-8, save_start=save_start, maxiters=100000)
    got = []
    for n in ns:
        gx, gp = reference_grads(model, p, x, times, cots, nsteps=n)
        got.append((_rel(r["dx"], gx), _rel(r["dp"], gp)))
    print(f"{name}: restatement (tol 1e-8, counts {r['counts']}) vs RK4 {ns[0]} steps dx {got[0][0]:.2e} dp {got[0][1]:.2e}; "
          f"{ns[1]} steps dx {got[1][0]:.2e} dp {got[1][1]:.2e}")
    bound = 4.0 * max(max(m) for m in RK4_MEASURED[name])
    assert max(max(g) for g in got) <= bound, (got, bound)


@pytest.mark.parametrize("mode", ["unbiased", "biased"])
@pytest.mark.parametrize("reg_type", ["error_estimate", "stiffness_estimate"])
def test_restatement_regulariser_gradient_vs_central_differences(mode, reg_type):
    """d reg_val / dp of the restatement (float64 autograd, uprev = sol(t1), k1 and dt frozen) against central
    differences of its own reg_val(p) along three random directions: O(h^2) truncation + rounding, far below 1e-6"""
    import lrnde_amd as P
    import chain_adjoint_np as CA
    from test_gpu_chain import mk_inputs, shapes
    model = shapes(P)["td3_gelu"]
    p, x = mk_inputs(P, model, 10, scale=3.0)
    times = [0.25, 0.5, 1.0]
    cots = np.zeros((3,) + x.shape, np.float32)
    r = CA.pullback(model, p, x, times, cots, 1e-4, mode=mode, reg_type=reg_type, t1_or_rand=0.43)
    assert r["t1"] == (float(np.float32(0.43)) if mode == "unbiased" else 0.25)   # biased: ts[int(0.43 * 2)]
    assert r["reg_val"] > 0
    rng = np.random.default_rng(5)
    p64 = p.astype(np.float64)
    for _ in range(3):
        d = rng.standard_normal(p.size)
        d /= np.linalg.norm(d)
        h = 1e-5
        fd = (r["reg_fn"](p64 + h * d) - r["reg_fn"](p64 - h * d)) / (2 * h)
        an = float(r["reg_grad"] @ d)
        print(f"{mode} {reg_type}: directional derivative autograd {an:.8e} central differences {fd:.8e}")
        assert abs(fd - an) <= 1e-6 * max(abs(an), np.linalg.norm(r["reg_grad"]) / np.sqrt(p.size))


def test_pinned_inputs_meet_their_selection_conditions():
    """the inputs the GPU tests compare step by step: the float64 and the float32 restatement take the same accepted and
    rejected steps (the estimate is truncation, not rounding), the reject cases have a reject, the impulse case has
    one directly after the impulse, and the mixed twins pass the row check the GPU loops are held to (CA.PINNED)"""
    import lrnde_amd as P
    import chain_adjoint_np as CA
    for name, c in CA.PINNED.items():
        model, p, x, times, cots, tol = CA.pinned_inputs(P, name)
        r64 = CA.pullback(model, p, x, times, cots, tol)
        r32 = CA.pullback(model, p, x, times, cots, tol, dtype=np.float32)
        print(f"{name}: float64 {r64['counts']} float32 {r32['counts']} forward {r64['fwd']} / {r32['fwd']}; "
              f"rel(float32, float64) dx {_rel(r32['dx'], r64['dx']):.2e} dp {_rel(r32['dp'], r64['dp']):.2e}")
        assert r64["counts"] == r32["counts"] and r64["fwd"] == r32["fwd"]
        assert [q[3] for q in r64["rows"]] == [q[3] for q in r32["rows"]]
        assert (r64["counts"][1] >= 1) == c["rejects"]
        assert r64["counts"][2] == 3 + 6 * (r64["counts"][0] + r64["counts"][1]) + sum(1 for t in times if 0.0 < t < 1.0)
        for tag, kw in (("float32 field, float64 interpolant", dict(dtype=np.float32, interp=np.float64)),
                        ("float64 field, float32 interpolant", dict(dtype=np.float64, interp=np.float32))):
            CA.check_rows(f"{name} {tag}", CA.pullback(model, p, x, times, cots, tol, **kw), r64, r32)
        if c["big"] is not None:
            s_imp = -float(np.float32(times[c["big"][0]]))
            after = [q for q in r64["rows"] if q[0] == s_imp]
            assert len(after) >= 2 and after[0][3] == 0, after   # the first attempt from the impulse time is rejected


def test_regulariser_inputs_meet_their_selection_condition():
    """CA.REG_CASE: 4 x the distance of the two restatements in reg_val is within the bar the GPU is held to"""
    import lrnde_amd as P
    import chain_adjoint_np as CA
    model, p, x, times, cots, tol = CA.reg_inputs(P)
    for mode in ("unbiased", "biased"):
        for reg_type in ("error_estimate", "stiffness_estimate"):
            kw = dict(mode=mode, reg_type=reg_type, t1_or_rand=CA.REG_CASE["t1_or_rand"])
            r64 = CA.pullback(model, p, x, times, cots, tol, **kw)
            r32 = CA.pullback(model, p, x, times, cots, tol, dtype=np.float32, **kw)
            d = abs(r32["reg_val"] - r64["reg_val"]) / r64["reg_val"]
            print(f"{mode} {reg_type}: reg_val {r64['reg_val']:.6e} float32 {r32['reg_val']:.6e} ({d:.1e})")
            assert 4.0 * d <= CA.REG_BAR
