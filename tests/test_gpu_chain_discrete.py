"""The Dense-chain handle's discrete adjoint (csrc/lrnde_chain_discrete.hpp; lrnde_set_sensealg,
NeuralODE(field="dense_chain", sensealg="TrackerAdjoint")): one launch over the recorded steps.

Yardstick: float64 autograd through the forward map on the FROZEN step grid (tests/chain_discrete_np.py, (a)), the grid
being the accepted rows of Handle.solve(..., trace=True) on the same inputs (the forward repeats bitwise).  Every gradient
block is held to max(1e-5, 4 x |float32 twin - float64|) relative to its norm, computed here on the CPU
(tests/test_gpu_chain.py's convention); measured and bound are printed.  The mathematics of the yardstick is pinned on the
CPU in tests/test_host_chain_discrete.py.

Measured on the MI355X (rel to the yardstick -> bound), dx / dp:
  PhysioNet B = 9 tol 1e-4: 3 times 1.8e-6 / 1.7e-6, 49 times 2.0e-6 / 2.3e-6, saved start 2.4e-6 / 2.4e-6 -> 1.0e-5 .. 1.1e-5
  td3_tanh 7.4e-7 / 7.6e-7, td3_gelu 5.4e-7 / 7.1e-7, one_layer 1.9e-7 / 1.1e-6, odd_21_37 3.3e-7 / 5.1e-7,
  odd_td_127_33 5.1e-7 / 7.4e-7, width_1 2.6e-7 / 4.1e-7, w128_td 4.2e-7 / 6.2e-7 -> 1e-5; 12 x Dense(40, 40) 6.3e-6 / 6.5e-6
  -> 1.2e-5 / 1.3e-5
  rejecting forward (CD.REJECTS; 23 accepted, 4 rejected): 6.3e-5 / 4.3e-5 -> 1.6e-4 / 1.2e-4
  regulariser difference against the continuous path's: 3.6e-8 .. 1.2e-6 -> 1.1e-3 .. 5.2e-2; discrete against continuous at
  tol 1e-6: 6.8e-6 / 6.9e-6 -> 3e-4; Latent-ODE step at tol 1e-6: neural_ode 7.1e-7, latent 4.9e-7 -> 3e-4
Parameter partial of the workgroup: in LDS for every shape here but w128_td (P = 16640 floats beside two 65 KB images) and
12 x Dense(40, 40) (whose backward image stays in L2 as well): global memory, read-modify-write by the owning thread."""
import numpy as np
import pytest
import torch

import chain_adjoint_np as CA
import chain_discrete_np as CD
from test_gpu_chain import mk, mk_inputs, physionet, rel, shapes

pytestmark = pytest.mark.gpu

f32 = np.float32
T49 = [(i + 1) / 49.0 for i in range(49)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def make_node(P, model, tol, times, sensealg="TrackerAdjoint", save_start=False, mode="none", reg_type="error_estimate"):
    return P.NeuralODE(model, regularize=mode, regularize_type=reg_type, abstol=tol, reltol=tol, saveat=list(times), save_start=save_start,
                       maxiters=10000, field="dense_chain", sensealg=sensealg)


def run(node, x, p, cots, w_reg=0.0, seed=3):
    st = node.initialstates(np.random.default_rng(seed))
    xd = dev(x)
    dx, dp, info = node.pullback(xd, dev(p), st, dev(cots), w_reg=w_reg)
    return dict(dx=dx.cpu().numpy(), dp=dp.cpu().numpy(), info=info, ai=node.handle(xd).last_adjoint_info())


def gpu_grid(node, x, p, tol):
    """the frozen grid: the accepted rows of the same solve's trace"""
    h = node._bind(dev(p), dev(x))
    r = h.solve(dev(x), 0.0, 1.0, tol, tol, saveat=[1.0], save_everystep=False, maxiters=10000, trace=True)
    return CD.grid_of_trace(r["trace"]), r["stats"]


def check_vs_yardstick(tag, got, model, p, x, grid, times, cots):
    y64 = CD.frozen_grads(model, p, x, grid, 0.0, 1.0, times, cots)
    y32 = CD.frozen_grads(model, p, x, grid, 0.0, 1.0, times, cots, dtype=torch.float32)
    for k, name in enumerate(("dx", "dp")):
        e, b = rel(got[name], y64[k]), CD.bound(y32[k], y64[k])
        print(f"{tag}: {len(grid)} steps, {name} rel {e:.2e} bound {b:.2e}")
        assert e <= b, (tag, name, e, b)
    assert got["ai"]["kind"] == 4 and got["info"]["adjoint_loop"] == "chain_discrete" and got["ai"]["host_waits"] == 0
    sb = got["info"]["stats_bwd"]
    N = len(grid)
    assert (sb["naccept"], sb["nreject"], sb["iters"], sb["nf"], sb["retcode"]) == (N, 0, N, 6 * N + 1, 0), sb
    assert sb["naccept"] == got["info"]["stats_fwd"]["naccept"]


# ---- 1. PhysioNet: a full tile and a one-column tile; 3 times, 49 times, a saved start state --------------------------
@pytest.mark.parametrize("case", ["three", "t49", "save_start"])
def test_physionet_vs_frozen_grid_autograd(gpu_pkg, case):
    P = gpu_pkg
    model = physionet(P)
    p, x = mk_inputs(P, model, 9, scale=1.5)
    tol = 1e-4
    times = T49 if case == "t49" else [0.25, 0.5, 1.0]
    series = ([0.0] if case == "save_start" else []) + list(times)
    cots = np.random.default_rng(11).standard_normal((len(series),) + x.shape).astype(f32)
    node = make_node(P, model, tol, times, save_start=case == "save_start")
    got = run(node, x, p, cots)
    assert [float(t) for t in got["info"]["sol_t"]] == [float(f32(t)) for t in series]
    grid, _ = gpu_grid(node, x, p, tol)
    check_vs_yardstick(f"physionet {case}", got, model, p, x, grid, series, cots)


# ---- 2. the other shapes: stage times (TDChain), one layer, odd widths, D = 1, the backward image beside a large P ------
@pytest.mark.parametrize("name,B", [("td3_tanh", 5), ("td3_gelu", 5), ("one_layer", 1), ("odd_21_37", 9), ("odd_td_127_33", 9),
                                    ("width_1", 9), ("w128_td", 3), ("deep40", 3)])
def test_shapes_vs_frozen_grid_autograd(gpu_pkg, name, B):
    """LDS plan of the sweep: every shape keeps both weight images and the workgroup's parameter partial in LDS, except
    w128_td (both images, 149 KB; the partial of 16640 floats in global memory) and deep40 (12 x Dense(40, 40): forward
    image and activation record 116 KB; backward image read from L2, partial in global memory)"""
    P = gpu_pkg
    model = P.Chain(*[P.Dense(40, 40, "tanh") for _ in range(12)]) if name == "deep40" else shapes(P)[name]
    p, x = mk_inputs(P, model, B, scale=1.5)
    tol, times = 1e-4, [0.3, 0.7, 1.0]
    cots = np.random.default_rng(12).standard_normal((3,) + x.shape).astype(f32)
    node = make_node(P, model, tol, times)
    got = run(node, x, p, cots)
    grid, _ = gpu_grid(node, x, p, tol)
    check_vs_yardstick(f"{name} B={B}", got, model, p, x, grid, times, cots)


# ---- 3. a forward that rejects steps: they do not appear in the sweep --------------------------------------------------
def test_rejected_attempts_do_not_appear(gpu_pkg):
    P = gpu_pkg
    model, p, x, times, cots, tol = CD.rejects_inputs(P)
    node = make_node(P, model, tol, times)
    got = run(node, x, p, cots)
    grid, st = gpu_grid(node, x, p, tol)
    sf, sb = got["info"]["stats_fwd"], got["info"]["stats_bwd"]
    print(f"forward naccept {sf['naccept']} nreject {sf['nreject']}; sweep {sb}")
    assert sf["nreject"] >= 1 and sb["naccept"] == sf["naccept"] == st["naccept"] and sb["nreject"] == 0
    check_vs_yardstick("rejecting forward", got, model, p, x, grid, times, cots)


# ---- 4. the regulariser rides on top, unchanged --------------------------------------------------------------------
@pytest.mark.parametrize("reg_type", ["error_estimate", "stiffness_estimate"])
@pytest.mark.parametrize("mode", ["unbiased", "biased"])
def test_regulariser_gradient_is_the_continuous_paths(gpu_pkg, mode, reg_type):
    """dp(w_reg = 2.5) - dp(0) on the discrete path against the same difference on the continuous path, at the bound of
    the regulariser row of DESIGN 4.9.1's table: max(1e-5, 4 x the distance of the float32 restatement's d reg / dp from the
    float64 one's) on CA.REG_CASE; dx does not depend on w_reg, bit for bit"""
    P = gpu_pkg
    model, p, x, times, cots, tol = CA.reg_inputs(P)
    kw = dict(mode=mode, reg_type=reg_type, t1_or_rand=CA.REG_CASE["t1_or_rand"])
    r64 = CA.pullback(model, p, x, times, cots, tol, **kw)
    r32 = CA.pullback(model, p, x, times, cots, tol, dtype=np.float32, **kw)
    bound = max(1e-5, 4.0 * rel(r32["reg_grad"], r64["reg_grad"]))
    d = {}
    for sense in ("TrackerAdjoint", None):
        node = make_node(P, model, tol, times, sensealg=sense, mode=mode, reg_type=reg_type)
        g0, gw = run(node, x, p, cots, w_reg=0.0), run(node, x, p, cots, w_reg=2.5)
        assert g0["ai"]["kind"] == gw["ai"]["kind"] == (4 if sense else 2)
        assert np.array_equal(g0["dx"], gw["dx"])
        assert gw["info"]["reg_val"] > 0
        d[sense] = gw["dp"].astype(np.float64) - g0["dp"].astype(np.float64)
    e = rel(d["TrackerAdjoint"], d[None])
    print(f"{mode} {reg_type}: rel(discrete dp(2.5) - dp(0), continuous) {e:.2e} bound {bound:.2e}; |difference| {np.linalg.norm(d[None]):.3e}")
    assert e <= bound, (e, bound)


# ---- 5. the two methods agree as the grid refines --------------------------------------------------------------------
def test_discrete_and_continuous_pullbacks_agree_at_tol_1e6(gpu_pkg):
    P = gpu_pkg
    model = physionet(P)
    p, x = mk_inputs(P, model, 9, scale=1.5)
    times = [0.25, 0.5, 1.0]
    cots = np.random.default_rng(11).standard_normal((3,) + x.shape).astype(f32)
    d = run(make_node(P, model, 1e-6, times), x, p, cots)
    c = run(make_node(P, model, 1e-6, times, sensealg=None), x, p, cots)
    assert d["ai"]["kind"] == 4 and c["ai"]["kind"] == 2
    print(f"tol 1e-6: rel(discrete, continuous) dx {rel(d['dx'], c['dx']):.2e} dp {rel(d['dp'], c['dp']):.2e}")
    assert rel(d["dx"], c["dx"]) <= 3e-4 and rel(d["dp"], c["dp"]) <= 3e-4


# ---- 6. one launch for all steps -----------------------------------------------------------------------------------
def test_launch_count_does_not_depend_on_the_step_count(gpu_pkg):
    P = gpu_pkg
    model = physionet(P)
    p, x = mk_inputs(P, model, 9, scale=1.5)
    times = [0.25, 0.5, 1.0]
    cots = np.random.default_rng(11).standard_normal((3,) + x.shape).astype(f32)
    a = run(make_node(P, model, 1e-3, times), x, p, cots)
    b = run(make_node(P, model, 1e-6, times), x, p, cots)
    na, nb = a["info"]["stats_bwd"]["naccept"], b["info"]["stats_bwd"]["naccept"]
    print(f"tol 1e-3: {na} steps {a['ai']}; tol 1e-6: {nb} steps {b['ai']}")
    assert nb > na
    assert a["ai"]["launches"] == b["ai"]["launches"] < max(na, nb)
    assert a["ai"]["host_waits"] == 0 and b["ai"]["host_waits"] == 0


# ---- 7. the same bits twice; a column does not depend on its neighbours or its place ------------------------------------
def test_repeats_bitwise_and_columns_are_independent(gpu_pkg):
    """The step grid belongs to the whole batch (the error norm runs over it), so a column "alone" is compared with a batch
    of 17 copies of it (three tiles, the last with one column), and a batch of 17 different columns with its permutation;
    the test first asserts that the compared solves took the same grid."""
    P = gpu_pkg
    model = physionet(P)
    p, X = mk_inputs(P, model, 17, scale=1.5)
    tol, times = 1e-4, [0.3, 0.31, 1.0]
    cots = np.random.default_rng(14).standard_normal((3,) + X.shape).astype(f32)
    node = make_node(P, model, tol, times)
    r1, r2 = run(node, X, p, cots), run(node, X, p, cots)
    assert np.array_equal(r1["dx"], r2["dx"]) and np.array_equal(r1["dp"], r2["dp"])
    same_grid = lambda a, b: len(a) == len(b) and all(s == t for s, t in zip(a, b))
    perm = np.random.default_rng(3).permutation(17)
    rp = run(node, X[perm], p, cots[:, perm])
    assert same_grid(gpu_grid(node, X, p, tol)[0], gpu_grid(node, X[perm], p, tol)[0])
    assert np.array_equal(rp["dx"], r1["dx"][perm])
    x1, c1 = X[5:6], cots[:, 5:6]
    alone = run(node, x1, p, c1)
    xs, cs = np.repeat(x1, 17, axis=0), np.repeat(c1, 17, axis=1)
    many = run(node, xs, p, cs)
    assert same_grid(gpu_grid(node, x1, p, tol)[0], gpu_grid(node, xs, p, tol)[0])
    for c in range(17):
        assert np.array_equal(many["dx"][c], alone["dx"][0]), c


# ---- 8. refusals leave the handle usable -----------------------------------------------------------------------------
def test_refusals(gpu_pkg):
    P = gpu_pkg
    from localregneuralde_jl_amd import _lib as L
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc, _wide_chain_desc
    model = physionet(P)
    h, p, x = mk(P, model, 9, scale=1.5)
    assert L.lib.lrnde_set_sensealg(h._ctx, 2) == 4 and L.lib.lrnde_set_sensealg(h._ctx, -1) == 4
    assert L.lib.lrnde_set_sensealg(h._ctx, 1) == 0 and L.lib.lrnde_set_sensealg(h._ctx, 0) == 0
    with pytest.raises(ValueError):
        h.set_sensealg("tracker")
    # a backward call without a record
    h.set_sensealg("discrete")
    with pytest.raises(L.LrndeError) as ei:
        h.node_backward_recorded(dev(x))
    assert ei.value.code == 4
    fw = h.node_forward_record(dev(x), 0.0, 1.0, 1e-4, 1e-4, mode="none")
    bw = h.node_backward_recorded(dev(np.ones_like(x)))
    assert fw["stats"]["retcode"] == 0 and h.last_adjoint_info()["kind"] == 4 and torch.isfinite(bw["dp"]).all()
    # handles of the other fields
    mlp = P.TDChain(P.Chain(P.Dense(5, 8, "tanh"), P.Dense(9, 4)))
    hm = Handle(_mlp_desc(mlp))
    hw = Handle(_wide_chain_desc(model))
    for hh in (hm, hw):
        assert L.lib.lrnde_set_sensealg(hh._ctx, 1) == 8
        msg = L.lib.lrnde_last_error(hh._ctx).decode()
        assert "small Dense-chain handle" in msg, msg
        assert L.lib.lrnde_set_sensealg(hh._ctx, 0) == 0
    pm = P.glorot_params(mlp, seed=0)
    hm.set_params(torch.from_numpy(pm))
    xm = dev(np.random.default_rng(0).random((3, 4), dtype=np.float32))
    assert torch.isfinite(hm.rhs(xm, 0.1)).all()
    # a chain outside the gate (16 x Dense(42, 42): 116 KB forward image + 53 KB activation record; the continuous device
    # loop's gate refuses it too and its pullback takes the host loop)
    big = P.Chain(*[P.Dense(42, 42, "tanh") for _ in range(16)])
    hb, pb, xb = mk(P, big, 3)
    hb.set_sensealg("discrete")
    hb.node_forward_record(dev(xb), 0.0, 1.0, 1e-3, 1e-3, mode="none")
    gen = hb.record_generation()
    with pytest.raises(L.LrndeError) as ei:
        hb.node_backward_recorded(dev(np.ones_like(xb)))
    assert ei.value.code == 8 and "LDS" in str(ei.value), str(ei.value)
    assert hb.record_generation() == gen != 0   # the record is still there
    hb.set_sensealg("interpolating")
    bw = hb.node_backward_recorded(dev(np.ones_like(xb)))
    assert hb.last_adjoint_info()["kind"] == 0 and torch.isfinite(bw["dx"]).all() and torch.isfinite(bw["dp"]).all()


# ---- 9. the Latent-ODE training step takes the new path with no other change --------------------------------------------
def test_latent_training_step_takes_the_discrete_path(gpu_pkg):
    import latent_cases as LC
    P = gpu_pkg
    dims, B, T = LC.PHYSIONET, 8, 49
    flat, nodep = LC.make_params(dims, seed=11), LC.make_node_params(dims, seed=12)
    data, mask, dt = LC.make_batch(dims, B, T, seed=13, unobserved_column=False)
    mask[:, 0, 0] = 1
    ps = dict(latent=dev(flat), neural_ode=dev(nodep))
    batch = (dev(data), dev(mask), dev(dt))
    out = {}
    for tol in (1e-3, 1e-6):
        for sense in ("TrackerAdjoint", None):
            kw = dict(saveat=T49, abstol=tol, reltol=tol, maxiters=10000)
            if sense:
                kw["sensealg"] = sense
            model = P.construct_time_series(*dims, **kw)
            st = model.initialstates(np.random.default_rng(5))
            loss, _st, _stats, grads, tm = P.run_latent_training_step(model, ps, st, batch, (0.0, 0.5))
            kind = model.neural_ode.handle().last_adjoint_info()["kind"]
            assert kind == (4 if sense else 2)
            out[(tol, sense)] = (loss, grads["neural_ode"].cpu().numpy(), grads["latent"].cpu().numpy(), tm["adjoint"])
    for tol in (1e-3, 1e-6):
        assert out[(tol, "TrackerAdjoint")][0] == out[(tol, None)][0]   # the forward is the same code: the same bits
    d, c = out[(1e-6, "TrackerAdjoint")], out[(1e-6, None)]
    print(f"tol 1e-6: sweep {d[3]}, continuous {c[3]}; rel neural_ode {rel(d[1], c[1]):.2e} latent {rel(d[2], c[2]):.2e}")
    assert rel(d[1], c[1]) <= 3e-4 and rel(d[2], c[2]) <= 3e-4
