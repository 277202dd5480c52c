"""Host side of the wide Dense-chain field (lrnde_create_wide_chain, layers._wide_chain_desc, NeuralODE(field="wide_chain")),
its float32 host restatement (tests/wide_chain_host.cpp) and the step-count condition of the GPU solve cases: no GPU needed.

Tolerances: tests/test_gpu_chain.py's rules — 1e-5 scale-relative on f-evals, or 4 x the distance of a float32-BLAS run
from float64 where depth or weight scale amplifies rounding."""
import os

import numpy as np
import pytest

import np_restatement as R
import wide_chain_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide_desc_validation_and_routing():
    import lrnde_amd as P
    from localregneuralde_jl_amd import _lib as L
    from localregneuralde_jl_amd.layers import _chain_desc, _wide_chain_desc
    S = WC.shapes(P)
    m3 = S["mnist3"]
    # today's routes keep their refusals for these models
    with pytest.raises(NotImplementedError):
        P.NeuralODE(m3)
    with pytest.raises(NotImplementedError, match="1..128"):
        P.NeuralODE(m3, field="dense_chain")
    with pytest.raises(NotImplementedError, match="1..128"):
        _chain_desc(S["seg_edges"])
    node = P.NeuralODE(m3, field="wide_chain")
    assert node.field == "wide_chain" and isinstance(node.desc, L.WideChainDesc) and isinstance(node.desc, L.ChainDesc)
    assert (node.desc.nlayers, node.desc.time_dep, node.desc.input_act) == (3, 1, 0)
    assert list(node.desc.dims)[:4] == [784, 100, 100, 784] and list(node.desc.act)[:3] == [1, 1, 0]
    d16 = _wide_chain_desc(S["deep16"])
    assert (d16.nlayers, d16.time_dep, d16.input_act) == (16, 0, 2) and list(d16.dims) == [144] * 17
    _wide_chain_desc(P.Chain(P.Dense(1024, 1024, "tanh")))                     # the width limit itself
    _wide_chain_desc(P.TDChain(P.Chain(P.Dense(1025, 1024, "tanh"))))          # 1024 + the t row
    with pytest.raises(NotImplementedError, match="1..1024"):
        _wide_chain_desc(P.Chain(P.Dense(4, 1025), P.Dense(1025, 4)))
    with pytest.raises(NotImplementedError, match="1..16"):
        _wide_chain_desc(P.Chain(*[P.Dense(4, 4) for _ in range(17)]))
    with pytest.raises(ValueError, match="do not chain"):
        _wide_chain_desc(P.Chain(P.Dense(4, 300), P.Dense(299, 4)))
    with pytest.raises(ValueError, match="same width"):
        _wide_chain_desc(P.Chain(P.Dense(4, 300), P.Dense(300, 5)))
    with pytest.raises(NotImplementedError, match="first element"):
        _wide_chain_desc(P.Chain(P.Dense(4, 8), P.Activation("tanh"), P.Dense(8, 4)))
    with pytest.raises(NotImplementedError, match="TDChain"):
        _wide_chain_desc(P.TDChain(P.Chain(P.Activation("tanh"), P.Dense(5, 4))))
    for solver in ("VCAB3", "vcabm3"):
        with pytest.raises(NotImplementedError):
            P.NeuralODE(m3, solver=solver, field="wide_chain")
    with pytest.raises(ValueError):
        P.NeuralODE(m3, field="wide")
    assert "lrnde_create_wide_chain" in {n for n, _, _ in L.SYMBOLS} and L.WIDE_CHAIN_MAX_WIDTH == 1024
    hdr = open(os.path.join(ROOT, "include", "lrnde.h")).read()
    assert "#define LRNDE_WIDE_CHAIN_MAX_WIDTH 1024" in hdr


def test_flat_layout_of_wide_models():
    """per layer vec(W) (out x (in+td), column-major, t column last) then b; the count is lrnde_chain_param_count's"""
    import ctypes
    import torch
    import lrnde_amd as P
    from localregneuralde_jl_amd import _lib as L
    from localregneuralde_jl_amd.layers import _wide_chain_desc, chain_param_count
    S = WC.shapes(P)
    d = _wide_chain_desc(S["mnist3"])
    n = 100 * 785 + 100 + 100 * 101 + 100 + 784 * 101 + 784
    assert chain_param_count(d) == n == 168768 == L.lib.lrnde_chain_param_count(ctypes.byref(d))
    assert P.glorot_chain_params(S["mnist3"]).size == n
    assert P.glorot_chain_params(S["w1024"]).size == 16 * 1024 + 16 + 1024 * 16 + 1024
    # the 2-layer shape has the MLP field's stream and layout
    assert np.array_equal(P.glorot_chain_params(S["mnist2"], seed=3), P.glorot_params(S["mnist2"], seed=3))
    rng = np.random.default_rng(0)
    Wb = [(rng.standard_normal((o, i + 1)).astype(np.float32), rng.standard_normal(o).astype(np.float32))
          for i, o in ((130, 257), (257, 131), (131, 130))]
    flat = P.flatten_chain_params([(torch.from_numpy(W), torch.from_numpy(b)) for W, b in Wb]).numpy()
    assert flat.size == chain_param_count(_wide_chain_desc(S["odd_td"]))
    back = WC.unflatten(flat, WC.spec(S["odd_td"]))
    for (W, b), (W2, b2) in zip(Wb, back):
        assert np.array_equal(W, W2) and np.array_equal(b, b2)


@pytest.mark.parametrize("name", ["mnist2", "mnist3", "seg_edges", "odd_td", "deep16", "w1024", "physionet"])
def test_host_restatement_vs_float64(name):
    import lrnde_amd as P
    model = WC.shapes(P)[name]
    p, x = WC.mk_inputs(P, model, 5)
    f64, f32 = WC.Chain64(model, p), WC.Chain32(model, p)
    for t in (0.0, 0.37):
        got, want = WC.run_host(model, p, x, t), f64.f64(x, t)
        bar = max(1e-5, 4.0 * WC.err(f32(x, t), want))
        e = WC.err(got, want)
        print(f"{name} t={t}: host restatement err {e:.2e} (bar {bar:.2e})")
        assert e <= bar, (name, t, e, bar)


@pytest.mark.parametrize("name,scale,tol", WC.GPU_COUNT_CASES)
def test_step_counts_agree_between_float64_and_float32(name, scale, tol):
    """the condition under which the GPU's (naccept, nreject) can be held to the float64 restatement's: at these weight
    scales the error estimate is truncation, and a second float32 summation order takes the same steps"""
    import lrnde_amd as P
    model, B = WC.count_shapes(P)[name]
    p, x = WC.mk_inputs(P, model, B, scale=scale)
    r64 = R.solve(WC.Chain64(model, p), x, 0.0, 1.0, tol, tol, save_t=0.5)
    r32 = R.solve(WC.Chain32(model, p), x, 0.0, 1.0, tol, tol, save_t=0.5)
    print(f"{name} x{scale} tol {tol:g}: float64 {(r64['naccept'], r64['nreject'])} float32 {(r32['naccept'], r32['nreject'])}")
    assert (r64["naccept"], r64["nreject"]) == (r32["naccept"], r32["nreject"])
    assert r64["naccept"] >= 9
    if (name, scale) == ("td200", 6.0):
        assert r64["nreject"] >= 1   # the case with a rejected step


def test_julia_binding_routes_wide_chains():
    src = open(os.path.join(ROOT, "julia", "LRNDEBackend.jl")).read()
    layer = open(os.path.join(ROOT, "julia", "LRNDELayer.jl")).read()
    assert ":lrnde_create_wide_chain" in src and "UNTESTED" in src
    assert "wide" in layer.lower()
