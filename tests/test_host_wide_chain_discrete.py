"""CPU side of the wide Dense-chain handle's discrete adjoint (csrc/lrnde_wide_discrete.hpp): the
layer's keyword and the names, the gate's arithmetic and the fixed launches against hand-computed values, the branch table
of the two kernels from the shapes alone, the method's float64 statement (chain_discrete_np.sweep64) against float64
autograd through the frozen-grid forward on two wide shapes, and the selection condition of the rejecting forward.
No GPU needed."""
import inspect
import os
import re

import numpy as np
import pytest

import wide_chain_adjoint_cases as WA
import wide_chain_cases as WC
import wide_chain_discrete_cases as WD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def P():
    import lrnde_amd
    return lrnde_amd


def test_layer_keyword_and_names(P):
    from localregneuralde_jl_amd.layers import Handle
    model = WC.shapes(P)["physionet"]
    node = P.NeuralODE(model, field="wide_chain", adjoint_loop="discrete")
    assert node.adjoint_loop == "discrete" and node.sense == "interpolating"
    for field in ("dense_chain", "auto"):
        with pytest.raises(NotImplementedError):
            P.NeuralODE(WC.shapes(P)["mnist2"] if field == "auto" else model, field=field, adjoint_loop="discrete")
    for bad in ("Discrete", "tracker", "", "sometimes"):
        with pytest.raises(ValueError):
            P.NeuralODE(model, field="wide_chain", adjoint_loop=bad)
    assert Handle.ADJOINT_LOOP_CHOICES == {"auto": 0, "device": 1, "discrete": 2}
    assert Handle.ADJOINT_LOOP_NAMES[5] == "wide_discrete" and len(Handle.ADJOINT_LOOP_NAMES) == 6
    assert Handle.ADJOINT_LOOP_NAMES[:5] == ("host", "device", "chain_device", "wide_device", "chain_discrete")
    assert '"wide_discrete"' in inspect.getdoc(P.NeuralODE.pullback)


def test_header_and_julia_declare_the_choice():
    hdr = open(os.path.join(ROOT, "include", "lrnde.h")).read()
    assert re.search(r"^enum\s*\{\s*LRNDE_ADJ_LOOP_DISCRETE\s*=\s*2\s*\};\s*$", hdr, re.M)
    jl = open(os.path.join(ROOT, "julia", "LRNDEBackend.jl")).read()
    assert re.search(r"ADJ_LOOP_DISCRETE\s*=.*Int32\(2\)", jl)


def test_gate_and_launches_by_hand(P):
    # mnist3 at B = 512: 6 slots x 32 tiles x 44800 floats of records, 14 vectors of 512 x 784
    g = WD.gate([784, 100, 100, 784], 512)
    assert g["fits"] and g["nwg"] == 32 and g["nitems"] == 233 and g["nmu"] == 233
    assert g["bytes"] == (6 * 32 * 44800 + 14 * 512 * 784) * 4 == 56885248
    assert g["lds"] == 2 * 784 * 16 * 4 + 4 * WC.partcap([784, 100, 100, 784]) + WC.LDS_TAIL <= WC.WIDE_LDS_MAX
    # the refused batch of the GPU test: w1024, record rows 1024 + 16 | 16 + 1024 and act0' 1024: 3104 rows x 16 columns
    dims = WC.model_dims(WC.shapes(P)[WD.REFUSED_SHAPE])
    assert dims == [1024, 16, 1024] and WA.rec_floats(dims) == 49664
    assert 6 * 49664 * 4 == 1191936 and 14 * 1024 * 4 == 57344      # bytes per tile of records, per column of vectors
    assert 127 * 1191936 + 2032 * 57344 == 267898880 <= WD.SCRATCH_MAX < 128 * 1191936 + 2033 * 57344 == 269148160
    assert WD.gate(dims, 2032)["fits"] and WD.gate(dims, 2032)["bytes"] == 267898880
    g = WD.gate(dims, 2033)
    assert not g["fits"] and g["why"] == "WIDE_SCRATCH_MAX" and g["bytes"] == 269148160
    assert WD.first_refused_batch(dims) == 2033
    # it is the shape whose refused batch costs the least forward work
    work = {}
    for name, model in WC.shapes(P).items():
        d = WC.model_dims(model)
        work[name] = WD.forward_work(d, WD.first_refused_batch(d))
    assert min(work, key=work.get) == WD.REFUSED_SHAPE, work
    # the workgroup limit comes first only for a narrow chain
    g = WD.gate([20, 40, 20], 4096 * 16 + 1)
    assert not g["fits"] and g["why"] == "CHADJ_MAX_WG"
    # fixed launches: one series-table launch (two from 65 times), the tail pair, k_adj_out; no launch zeroes mu
    assert WD.LAUNCH_C == WD.launch_c(3) == 1 + 2 + 1 == 4 and WD.launch_c(64) == 4 and WD.launch_c(80) == 5


def test_branch_table(P):
    """every branch of k_wdisc_step / k_wdisc_mu is taken by the case named for it, and those cases are among the ones GPU
    tests 1 and 2 run; every mu-item branch of WA.BRANCHES that does not concern the controller is among them"""
    assert set(WD.BRANCH_CASE) == set(WD.BRANCHES)
    assert set(WD.MU_BRANCHES) == set(WA.BRANCHES) - {"impulse", "end_only"}
    cases = {(n, B) for n, B, _s in WD.SHAPE_CASES}
    for br, case in WD.BRANCH_CASE.items():
        if br.startswith("place_"):
            assert case in WD.PLACEMENTS and br == "place_" + case
            continue
        assert case in cases, (br, case)
        assert br in WD.shape_branches(P, *case), (br, case)
    # the shapes reach every branch of wide_gemm (WC.gemm_paths), as the continuous loop's cases do
    paths = set()
    for name, _B, _s in WD.SHAPE_CASES:
        for f, g in WC.gemm_paths(WC.model_dims(WC.shapes(P)[name])):
            paths.update((f, g))
    assert {"single", "split", "cap_fallback"} <= paths, paths


def _cpu_grid(P, name, B, tol, scale=1.0):
    import chain_adjoint_np as CA
    import chain_discrete_np as CD
    model = WC.shapes(P)[name]
    p, x = WC.mk_inputs(P, model, B, scale=scale)
    return model, p, x, CD.grid_of(CA.forward(CA.Field(model, p), x, 0.0, 1.0, tol, tol)["steps"])


@pytest.mark.parametrize("name,B", [("mnist3", 3), ("odd_td", 2)])
@pytest.mark.parametrize("case", ["mixed", "two_in_one_step"])
def test_sweep_equals_autograd_of_the_frozen_forward(P, name, B, case):
    """sweep64 = autograd of the frozen-grid forward to 1e-10 relative on wide shapes, on the series
    tests/test_host_chain_discrete.py builds: "mixed" (grid of tol 1e-4): a saved start state, a save equal to an inner
    step's end, a save strictly inside a step, the end time; "two_in_one_step": two saves inside one step of a coarse grid"""
    import chain_discrete_np as CD
    model, p, x, grid = _cpu_grid(P, name, B, 1e-4 if case == "mixed" else 1e-2, scale=1.5)
    assert len(grid) >= 3
    if case == "mixed":
        k = len(grid) // 2
        inside = f32(grid[k + 1][0] + f32(0.3) * grid[k + 1][1])
        times = [0.0, float(grid[k][0]), float(inside), 1.0]
        pl = CD.place(grid, 0.0, 1.0, times)
        assert pl[0] == ("start",) and pl[1] == ("end", k - 1) and pl[2][:2] == ("in", k + 1) and pl[3] == ("end", len(grid) - 1)
    else:
        k = int(np.argmax([float(dt) for _t, dt in grid]))
        t, dt = grid[k]
        times = [float(f32(t + f32(th) * dt)) for th in (0.3, 0.6)] + [1.0]
        pl = CD.place(grid, 0.0, 1.0, times)
        assert pl[0][:2] == pl[1][:2] == ("in", k), pl
    cots = np.random.default_rng(17).standard_normal((len(times),) + x.shape).astype(f32)
    gx, gp, _ = CD.frozen_grads(model, p, x, grid, 0.0, 1.0, times, cots)
    dx, dp = CD.sweep64(model, p, x, grid, 0.0, 1.0, times, cots)
    print(f"{name} {case}: {len(grid)} steps, places {pl}; rel dx {WC.rel(dx, gx):.2e} dp {WC.rel(dp, gp):.2e}")
    assert WC.rel(dx, gx) <= 1e-10 and WC.rel(dp, gp) <= 1e-10


@pytest.mark.parametrize("kind", WD.PLACEMENTS)
def test_placements_lie_where_they_are_meant_to(P, kind):
    """WD.placement on the float64 restatement's grid of the placement case (the GPU test repeats this on its own grid)"""
    import chain_discrete_np as CD
    _m, _p, _x, grid = _cpu_grid(P, WD.PLACE_SHAPE, WD.PLACE_B, WD.TOL)
    times, save_start, want = WD.placement(kind, grid)
    pl = WD.check_placement(CD, kind, grid, times, save_start, want)
    print(kind, len(grid), "steps:", pl[:4])


def test_rejecting_forward_meets_its_selection_conditions(P):
    """WD.REJECTS: the forward rejects at least one attempt with the float64 field and with the float32 field, on the
    float64 grid 4 x the distance of the float32 twin of the yardstick from float64 is within WD.REJECTS_BAR, and the state
    stays within WD.REJECTS_STATE_MAX"""
    import torch
    import chain_adjoint_np as CA
    import chain_discrete_np as CD
    model, p, x, times, cots, tol = WD.rejects_inputs(P)
    fws = [CA.forward(CA.Field(model, p, dtype), x, 0.0, 1.0, tol, tol, saveat=times) for dtype in (np.float64, np.float32)]
    print("float64 / float32 (naccept, nreject):", [(fw["naccept"], fw["nreject"]) for fw in fws])
    assert min(fw["nreject"] for fw in fws) >= 1
    umax = max(float(np.abs(s[2]).max()) for fw in fws for s in fw["steps"])
    print(f"largest |u| along the solves: {umax:.3g}")
    assert umax <= WD.REJECTS_STATE_MAX
    grid = CD.grid_of(fws[0]["steps"])
    y64 = CD.frozen_grads(model, p, x, grid, 0.0, 1.0, times, cots)
    y32 = CD.frozen_grads(model, p, x, grid, 0.0, 1.0, times, cots, dtype=torch.float32)
    d = [WC.rel(y32[k], y64[k]) for k in range(2)]
    print(f"twins apart: dx {d[0]:.2e} dp {d[1]:.2e}")
    assert 4.0 * max(d) <= WD.REJECTS_BAR
