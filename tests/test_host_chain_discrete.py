"""The mathematics of the Dense-chain handle's discrete adjoint on the CPU, before any kernel runs: the
reverse sweep restated in numpy float64 (tests/chain_discrete_np.py, (b)) against float64 autograd through the frozen-grid
forward ((a)), its approach to the continuous gradient as the tolerance falls, the selection condition of the pinned
rejecting forward, and the layer's argument handling.  No GPU needed."""
import numpy as np
import pytest

f32 = np.float32


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _inputs(P, name, B):
    from test_gpu_chain import mk_inputs, shapes
    model = shapes(P)[name]
    p, x = mk_inputs(P, model, B, scale=1.5)
    return model, p, x


def test_vjp64_is_field_vjp_without_its_roundings():
    """Field64.vjp64 at a float32 time, rounded once, is chain_adjoint_np.Field.vjp"""
    import lrnde_amd as P
    import chain_adjoint_np as CA
    import chain_discrete_np as CD
    for name in ("physionet", "td3_tanh", "td3_gelu"):
        model, p, x = _inputs(P, name, 3)
        lam = np.random.default_rng(5).standard_normal(x.shape).astype(f32)
        t = f32(0.37)
        a, b = CA.Field(model, p).vjp(x, t, lam), CD.Field64(model, p).vjp64(x, t, lam)
        assert np.array_equal(a[0], b[0].astype(f32)) and np.array_equal(a[1], b[1].astype(f32))


@pytest.mark.parametrize("name,B", [("physionet", 3), ("td3_tanh", 2)])
@pytest.mark.parametrize("case", ["mixed", "two_in_one_step"])
def test_sweep_equals_autograd_of_the_frozen_forward(name, B, case):
    """(b) = autograd of (a) to 1e-10 relative.  "mixed" (grid of tol 1e-4): a saved start state, a save strictly inside a
    step, a save equal to the end of a step inside the span, and the end time.  "two_in_one_step" (grid of tol 1e-2): 0.30,
    0.31 and 0.32, of which at least two fall inside one step, and the end time."""
    import lrnde_amd as P
    import chain_adjoint_np as CA
    import chain_discrete_np as CD
    model, p, x = _inputs(P, name, B)
    tol = 1e-4 if case == "mixed" else 1e-2
    grid = CD.grid_of(CA.forward(CA.Field(model, p), x, 0.0, 1.0, tol, tol)["steps"])
    assert len(grid) >= 3
    if case == "mixed":
        k = len(grid) // 2
        inside = f32(grid[k + 1][0] + f32(0.3) * grid[k + 1][1])
        times = [0.0, float(grid[k][0]), float(inside), 1.0]
        pl = CD.place(grid, 0.0, 1.0, times)
        assert pl[0] == ("start",) and pl[1] == ("end", k - 1) and pl[2][:2] == ("in", k + 1) and pl[3] == ("end", len(grid) - 1)
    else:
        times = [0.30, 0.31, 0.32, 1.0]
        pl = CD.place(grid, 0.0, 1.0, times)
        steps = [e[1] for e in pl[:3] if e[0] == "in"]
        assert len(steps) - len(set(steps)) >= 1, pl   # two saves inside one step
    cots = np.random.default_rng(17).standard_normal((len(times),) + x.shape).astype(f32)
    gx, gp, _ = CD.frozen_grads(model, p, x, grid, 0.0, 1.0, times, cots)
    dx, dp = CD.sweep64(model, p, x, grid, 0.0, 1.0, times, cots)
    print(f"{name} {case}: {len(grid)} steps, places {pl}; rel dx {_rel(dx, gx):.2e} dp {_rel(dp, gp):.2e}")
    assert _rel(dx, gx) <= 1e-10 and _rel(dp, gp) <= 1e-10


def test_discrete_gradient_approaches_the_continuous_one():
    """on the grids of tol 1e-4, 1e-6, 1e-8 the discrete gradient approaches float64 autograd through RK4
    (test_gpu_chain.reference_grads) and is within the project's 3e-4 at 1e-6"""
    import lrnde_amd as P
    import chain_adjoint_np as CA
    import chain_discrete_np as CD
    from test_gpu_chain import reference_grads
    model, p, x = _inputs(P, "physionet", 3)
    times = [0.25, 0.5, 1.0]
    cots = np.random.default_rng(13).standard_normal((3,) + x.shape).astype(f32)
    rx, rp = reference_grads(model, p, x, times, cots, nsteps=400)
    errs = []
    for tol in (1e-4, 1e-6, 1e-8):
        grid = CD.grid_of(CA.forward(CA.Field(model, p), x, 0.0, 1.0, tol, tol, maxiters=100000)["steps"])
        dx, dp = CD.sweep64(model, p, x, grid, 0.0, 1.0, times, cots)
        errs.append((_rel(dx, rx), _rel(dp, rp)))
        print(f"tol {tol:g}: {len(grid)} steps, rel dx {errs[-1][0]:.2e} dp {errs[-1][1]:.2e}")
    assert max(errs[1]) <= 3e-4
    for k in range(2):
        assert errs[2][k] < errs[1][k] < errs[0][k], errs


def test_rejecting_forward_meets_its_selection_conditions():
    """CD.REJECTS: the forward rejects at least two attempts with the float64 field and with the float32 field, and on
    its grid 4 x the distance of the float32 twin of the yardstick from float64 is within CD.REJECTS_BAR"""
    import torch
    import lrnde_amd as P
    import chain_adjoint_np as CA
    import chain_discrete_np as CD
    model, p, x, times, cots, tol = CD.rejects_inputs(P)
    fws = [CA.forward(CA.Field(model, p, dtype), x, 0.0, 1.0, tol, tol, saveat=times) for dtype in (np.float64, np.float32)]
    print("float64 / float32 (naccept, nreject):", [(fw["naccept"], fw["nreject"]) for fw in fws])
    assert min(fw["nreject"] for fw in fws) >= 2
    grid = CD.grid_of(fws[0]["steps"])
    y64 = CD.frozen_grads(model, p, x, grid, 0.0, 1.0, times, cots)
    y32 = CD.frozen_grads(model, p, x, grid, 0.0, 1.0, times, cots, dtype=torch.float32)
    d = [_rel(y32[k], y64[k]) for k in range(2)]
    print(f"twins apart: dx {d[0]:.2e} dp {d[1]:.2e}")
    assert 4.0 * max(d) <= CD.REJECTS_BAR


def test_layer_sensealg_arguments():
    import lrnde_amd as P
    from localregneuralde_jl_amd import _lib as L
    from localregneuralde_jl_amd.layers import Handle
    from test_gpu_chain import physionet
    assert "lrnde_set_sensealg" in [s[0] for s in L.SYMBOLS]
    assert Handle.ADJOINT_LOOP_NAMES[4] == "chain_discrete" and Handle.ADJOINT_LOOPS == ("host", "device", "chain_device")
    assert callable(Handle.set_sensealg)
    chain = physionet(P)
    mlp = P.TDChain(P.Chain(P.Dense(5, 8, "tanh"), P.Dense(9, 4)))
    for s in (None, "InterpolatingAdjoint", "InterpolatingAdjoint()"):
        assert P.NeuralODE(chain, sensealg=s, field="dense_chain").sense == "interpolating"
        assert P.NeuralODE(mlp, sensealg=s).sense == "interpolating"
        assert P.NeuralODE(chain, sensealg=s, field="wide_chain").sense == "interpolating"
    for s in ("TrackerAdjoint", "TrackerAdjoint()", "ReverseDiffAdjoint", "ReverseDiffAdjoint()", "discrete"):
        node = P.NeuralODE(chain, sensealg=s, field="dense_chain")
        assert node.sense == "discrete" and node.sensealg == s
        with pytest.raises(NotImplementedError):
            P.NeuralODE(mlp, sensealg=s)
        with pytest.raises(NotImplementedError):
            P.NeuralODE(chain, sensealg=s, field="wide_chain")
    for s in ("ForwardDiffSensitivity", "tracker", ""):
        with pytest.raises(ValueError):
            P.NeuralODE(chain, sensealg=s, field="dense_chain")
    # the Latent-ODE constructor forwards the keyword to the layer
    m = P.construct_time_series(37, 40, 50, 20, saveat=[(i + 1) / 49.0 for i in range(49)], sensealg="TrackerAdjoint")
    assert m.neural_ode.sense == "discrete" and m.neural_ode.field == "dense_chain"
