"""The recorded layer forward's plan (csrc/lrnde_layer_plan.hpp: the solve's saveat, the slot of sol(t1), the corrected
series) on the device, at the smallest MLP shape of the 4-column path and once more on the 16-column path: the forward
with the companion stream (the slot of sol(t1) predicted before the solve) against the forward in order on the handle's
stream — same sol.t, same bits of sol.u, reg_val and t1 — and sol.t against NeuralODE.__call__, which goes through
Handle.solve and the Python-side statement of the same plan."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, H, B = 32, 64, 12
T0, T2, TOL = np.float32(0.0), np.float32(1.0), 1e-5
SEED = 3

# (regularize, save_start, the layer's saveat: None, a list, or "t1": one that contains the drawn t1 exactly)
CASES = [("unbiased", ss, sv) for ss in (False, True) for sv in ([0.25, 0.5, 1.0], [0.0, 0.5, 1.0], "t1")]
CASES += [("biased", True, None), ("biased", True, [0.25, 0.5, 1.0]), ("none", False, None)]


@pytest.fixture(scope="module")
def setup(gpu_pkg):
    import torch
    P = gpu_pkg
    model = P.TDChain(P.Chain(P.Dense(D + 1, H, "tanh"), P.Dense(H + 1, D)))
    ps = torch.from_numpy(P.glorot_params(model, seed=1) * np.float32(1.5))
    x = torch.from_numpy(np.random.default_rng(2).random((B, D), dtype=np.float32)).cuda()
    return model, ps, x


@pytest.mark.parametrize("no_qtile", [0, 1])
@pytest.mark.parametrize("mode,save_start,saveat", CASES)
def test_recorded_forward_follows_the_plan(gpu_pkg, setup, mode, save_start, saveat, no_qtile):
    import torch
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    P = gpu_pkg
    model, ps, x = setup
    # the one draw of the layer (NeuralODE.__call__ / pullback): t1 in :unbiased, the index draw in :biased
    r01 = np.float32(np.random.default_rng(SEED).random(dtype=np.float32))
    t1 = np.float32(r01 * (T2 - T0) + T0)
    if saveat == "t1":
        saveat = sorted([np.float32(0.25), t1, np.float32(1.0)])
    P.set_option("LRNDE_NO_QTILE", no_qtile)
    try:
        h = Handle(_mlp_desc(model))
        h.set_params(ps)
        out = []
        for on in (True, False):
            h.set_overlap(on)
            out.append(h.node_forward_record_ts(x, T0, T2, TOL, TOL, [] if saveat is None else saveat, mode=mode,
                                                t1_or_rand=t1 if mode == "unbiased" else r01, maxiters=1000, save_start=save_start))
        a, b = out
        assert np.array_equal(a["t"], b["t"]), (a["t"], b["t"])
        assert torch.equal(a["u"], b["u"])
        assert a["reg_val"].tobytes() == b["reg_val"].tobytes() and a["t1"].tobytes() == b["t1"].tobytes(), (a["reg_val"], b["reg_val"])
        assert a["nfe"] == b["nfe"] and a["stats"] == b["stats"]
        kw = dict(abstol=TOL, reltol=TOL, save_start=save_start)
        if saveat is not None:
            kw["saveat"] = saveat
        node = P.NeuralODE(model, tspan=(T0, T2), regularize=mode, maxiters=1000, **kw)
        st = dict(model={}, nfe=-1, reg_val=np.float32(0.0), rng=np.random.default_rng(SEED), training=True)
        sol, _ = node(x, ps, st)
        assert np.array_equal(np.asarray(sol.t, dtype=np.float32), a["t"]), (sol.t, a["t"])
        if mode == "unbiased":
            assert a["t1"] == t1
            assert saveat is None or not np.any(a["t"] == t1), "the corrected solution leaves the entries at t1 out"
    finally:
        P.set_option("LRNDE_NO_QTILE", 0)
