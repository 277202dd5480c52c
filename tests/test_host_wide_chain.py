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


ALL = ["mnist2", "mnist3", "seg_edges", "odd_td", "deep16", "w1024", "physionet", "sq520", "cap_mixed", "cap_fwd", "full1024"]


def test_shapes_reach_every_branch_of_wide_gemm():
    """forward and transposed product each take every path of wide_gemm on some shape, and one handle (cap_mixed) holds a
    layer that spreads its segments inside the partial region beside one that does not fit it"""
    import lrnde_amd as P
    S = WC.shapes(P)
    assert sorted(S) == sorted(ALL)
    seen = {name: WC.gemm_paths(WC.model_dims(m)) for name, m in S.items()}
    for name, paths in seen.items():
        print(name, WC.partcap(WC.model_dims(S[name])), paths)
    for d in (0, 1):
        assert {lp[d] for paths in seen.values() for lp in paths} == set(WC.GEMM_PATHS), d
    # the region at width 1024: 160 KiB less the two 64-KiB buffers and the tail, in whole 256-float rows
    assert WC.partcap([1024, 16, 100, 1024]) == 7936 and WC.part_want(1, 64) == 2560 and WC.part_want(7, 64) == 17920
    assert seen["cap_mixed"] == [("split", "single"), ("single", "single"), ("single", "cap_fallback")]
    assert seen["cap_fwd"] == [("cap_fallback", "single"), ("single", "cap_fallback")]
    assert seen["sq520"] == [("unsplit_multi", "unsplit_multi_trips"), ("unsplit_multi_trips", "unsplit_multi")]
    assert seen["full1024"] == [("unsplit_multi_trips",) * 2] * 2
    # what the suite had before: a product with several segments always spread them, one with >= 8 groups had one segment
    old = {lp[d] for n in ALL[:7] for lp in seen[n] for d in (0, 1)}
    assert old == {"single", "split"}
    # the chunked VJP launch: 30 of full1024's workgroups fit one launch's scratch, so B = 497 (32 workgroups) takes two
    assert WC.vjp_chunk([1024, 1024, 1024], 0) == 30 and WC.vjp_chunk([784, 100, 100, 784], 1) > 280


@pytest.mark.parametrize("name", ALL)
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


@pytest.mark.parametrize("name", ALL)
def test_vjp_host_restatement_vs_float64_autograd(name):
    import lrnde_amd as P
    model = WC.shapes(P)[name]
    p, x = WC.mk_inputs(P, model, 17)
    lam = np.random.default_rng(7).standard_normal(x.shape).astype(np.float32)
    t = 0.61
    for B in (5, 17):
        (dy64, gp64), (bar_dy, bar_gp), e32 = WC.vjp_bars(model, p, x[:B], lam[:B], t)
        dy, gp = WC.run_vjp_host(model, p, x[:B], lam[:B], t)
        edy, egp = WC.err(dy, dy64), WC.err(gp, gp64)
        print(f"{name} B={B}: restatement dy err {edy:.2e} gp err {egp:.2e}; float32 autograd {e32[0]:.2e} {e32[1]:.2e}; "
              f"bars {bar_dy:.2e} {bar_gp:.2e}")
        assert edy <= bar_dy and egp <= bar_gp, (name, B, edy, egp, bar_dy, bar_gp)


@pytest.mark.parametrize("name", ["odd_td", "sq520", "cap_mixed"])
def test_vjp_host_restatement_columns_are_independent(name):
    """dy of a column alone is dy of the column inside a batch (any place in its tile), whatever the sum over the tiles
    does; gp does depend on how that sum is cut once a later launch holds two tiles: (p0 + p1) + (p2 + p3) is not
    ((p0 + p1) + p2) + p3 — what the library's several-launch VJP must therefore not compute"""
    import lrnde_amd as P
    model = WC.shapes(P)[name]
    p, x = WC.mk_inputs(P, model, 64)
    lam = np.random.default_rng(7).standard_normal(x.shape).astype(np.float32)
    dy, gp = WC.run_vjp_host(model, p, x, lam, 0.61)
    for c in (0, 15, 16, 63):
        assert np.array_equal(WC.run_vjp_host(model, p, x[c:c + 1], lam[c:c + 1], 0.61)[0][0], dy[c]), (name, c)
    assert np.array_equal(WC.run_vjp_host(model, p, x[:33], lam[:33], 0.61)[0], dy[:33])
    dy2, gp2 = WC.run_vjp_host(model, p, x, lam, 0.61, chunk=2)
    assert np.array_equal(dy2, dy)
    ndiff = int((gp2 != gp).sum())
    print(f"{name}: {ndiff} of {gp.size} parameter cotangents differ when launches of two tiles each sum from 0")
    assert ndiff > 0 and WC.err(gp2, gp) < 1e-5


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


@pytest.mark.parametrize("name,scale,tol", WC.FOOTER_CASES)
def test_footer_cases_put_two_saves_in_one_step(name, scale, tol):
    """the save grid of the GPU footer cases: two of its times fall inside one accepted step of the float64 solve (and of
    the float32 one: the GPU's steps are as close), odd130 x6 rejects a step; the restatement's savevalues! against its own
    single-time form"""
    import lrnde_amd as P
    model, B = WC.count_shapes(P)[name]
    p, x = WC.mk_inputs(P, model, B, scale=scale)
    f64 = WC.Chain64(model, p)
    r0 = R.solve(f64, x, 0.0, 1.0, tol, tol)
    saves = WC.footer_saves(r0["t_steps"])
    assert 0.0 < saves[0] < saves[1] < saves[2] < 1.0
    hold = WC.steps_holding(r0["t_steps"], saves)
    assert hold[1] == hold[2] != hold[0]
    r32 = R.solve(WC.Chain32(model, p), x, 0.0, 1.0, tol, tol)
    assert WC.steps_holding(r32["t_steps"], saves) == hold
    if name == "odd130":
        assert r0["nreject"] >= 1 and len(r0["dts"]) == r0["naccept"] + r0["nreject"] > len(r0["t_steps"])
        assert model.layers[0].in_dims - 1 == 130 and 130 % 4 != 0
    r = R.solve(f64, x, 0.0, 1.0, tol, tol, saveat=saves + [1.0], save_start=True, save_t=saves[1])
    assert (r["naccept"], r["nreject"]) == (r0["naccept"], r0["nreject"]) and np.array_equal(r["u"], r0["u"])
    assert np.array_equal(r["t_saved"], np.array([0.0] + saves + [1.0], np.float32)) and len(r["u_saved"]) == 5
    assert np.array_equal(r["u_saved"][0], x) and np.array_equal(r["u_saved"][2], r["u_save"]) and np.array_equal(r["u_saved"][4], r["u"])
    e = R.solve(f64, x, 0.0, 1.0, tol, tol, saveat=saves, save_start=True, save_everystep=True)
    assert len(e["t_saved"]) == 1 + 3 + e["naccept"] and e["t_saved"][-1] == 1.0 and np.array_equal(e["u_saved"][-1], r0["u"])
    assert np.all(np.diff(e["t_saved"]) > 0)
    at = np.flatnonzero(np.isin(e["t_saved"], np.array(saves, np.float32)))
    assert [int(i) for i in at] == [1 + hold[0] + 0, 1 + hold[1] + 1, 1 + hold[2] + 2]   # before the step's own end, in order
    for i, j in zip(at, (1, 2, 3)):
        assert np.array_equal(e["u_saved"][i], r["u_saved"][j])


def test_julia_binding_routes_wide_chains():
    src = open(os.path.join(ROOT, "julia", "LRNDEBackend.jl")).read()
    layer = open(os.path.join(ROOT, "julia", "LRNDELayer.jl")).read()
    assert ":lrnde_create_wide_chain" in src and "UNTESTED" in src
    assert "wide" in layer.lower()
