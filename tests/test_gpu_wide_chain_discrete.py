"""The wide Dense-chain handle's discrete adjoint (csrc/lrnde_wide_discrete.hpp, DESIGN.md 4.12.2;
lrnde_set_adjoint_loop(ctx, LRNDE_ADJ_LOOP_DISCRETE), NeuralODE(field="wide_chain", adjoint_loop="discrete")): two launches
per recorded step, newest first, no host wait.

Yardstick: float64 autograd through the forward map on the FROZEN step grid (tests/chain_discrete_np.py, frozen_grads), the
grid being the accepted rows of Handle.solve(..., trace=True) on the same inputs.  Every gradient block is held to
max(1e-5, 4 x |float32 twin - float64|) relative to its norm, computed here on the CPU; measured and bound are printed.
The mathematics of the yardstick on wide shapes, the gate and the branch table are pinned on the CPU in
tests/test_host_wide_chain_discrete.py; the cases are tests/wide_chain_discrete_cases.py's.

Measured on the MI355X (rel to the yardstick -> bound), dx / dp, tol 1e-4 (DESIGN.md 4.12.2 has the table):
  mnist3 B = 1 / 17 / 33: 3.0e-7 / 7.9e-7, 3.0e-7 / 8.3e-7, 2.9e-7 / 8.2e-7; odd_td 2.3e-7 / 8.1e-7; seg_edges 4.1e-7 / 7.9e-7;
  cap_mixed 1.3e-7 / 6.6e-7; deep16 4.1e-7 / 1.6e-6; physionet x1.5 2.3e-6 / 2.1e-6 -> 1e-5 each
  placements on mnist3 B = 17: 2.5e-7 .. 3.7e-7 / 8.0e-7 .. 8.4e-7 -> 1e-5
  rejecting forward (WD.REJECTS; 23 accepted, 4 rejected): 6.3e-5 / 4.3e-5 -> 1.6e-4 / 1.2e-4
  regulariser difference against the host loop's: 3.2e-8 .. 3.7e-6 -> 0.14 .. 5.7; discrete against continuous at tol 1e-6:
  3.1e-7 / 6.4e-7 -> 3e-4; physionet through both sweeps: dx bit-equal, dp 1.8e-7 apart -> 2e-5; training step at tol 1e-6:
  7.0e-7 / 0 / 3.9e-7 -> 3e-4"""
import numpy as np
import pytest
import torch

import chain_adjoint_np as CA
import chain_discrete_np as CD
import wide_chain_cases as WC
import wide_chain_discrete_cases as WD
from wide_chain_discrete_cases import dev, make_node, run

pytestmark = pytest.mark.gpu

f32 = np.float32
rel = WC.rel
_YARD = {}


def yardstick(key, model, p, x, grid, times, cots):
    """(float64, float32 twin) frozen-grid gradients, computed once per case"""
    k = (key, tuple(grid), tuple(times))
    if k not in _YARD:
        _YARD[k] = (CD.frozen_grads(model, p, x, grid, 0.0, 1.0, times, cots)[:2],
                    CD.frozen_grads(model, p, x, grid, 0.0, 1.0, times, cots, dtype=torch.float32)[:2])
    return _YARD[k]


def check_path(got, N):
    assert got["ai"]["kind"] == 5 and got["info"]["adjoint_loop"] == "wide_discrete" and got["ai"]["host_waits"] == 0, got["ai"]
    sb = got["info"]["stats_bwd"]
    assert (sb["naccept"], sb["nreject"], sb["iters"], sb["nf"], sb["retcode"]) == (N, 0, N, 6 * N + 1, 0), sb
    assert sb["naccept"] == got["info"]["stats_fwd"]["naccept"]


def check_vs_yardstick(tag, got, model, p, x, grid, times, cots):
    y64, y32 = yardstick(tag, model, p, x, grid, times, cots)
    for k, name in enumerate(("dx", "dp")):
        e, b = rel(got[name], y64[k]), CD.bound(y32[k], y64[k])
        print(f"{tag}: {len(grid)} steps, {name} rel {e:.2e} bound {b:.2e}")
        assert e <= b, (tag, name, e, b)
    check_path(got, len(grid))


# ---- 1. shapes and tiles ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,scale", WD.SHAPE_CASES)
def test_shapes_vs_frozen_grid_autograd(gpu_pkg, name, B, scale):
    P = gpu_pkg
    model = WC.shapes(P)[name]
    p, x = WC.mk_inputs(P, model, B, scale=scale)
    cots = np.random.default_rng(12).standard_normal((3,) + x.shape).astype(f32)
    node = make_node(P, model, WD.TOL, WD.TIMES)
    got = run(node, x, p, cots)
    grid, _ = WD.gpu_grid(CD, node, x, p, WD.TOL)
    check_vs_yardstick(f"{name} B={B}", got, model, p, x, grid, WD.TIMES, cots)


# ---- 2. placements of saves, chosen from the GPU's own grid --------------------------------------------------------------
@pytest.mark.parametrize("kind", WD.PLACEMENTS)
def test_placements_of_saves(gpu_pkg, kind):
    P = gpu_pkg
    model = WC.shapes(P)[WD.PLACE_SHAPE]
    p, x = WC.mk_inputs(P, model, WD.PLACE_B)
    grid0, _ = WD.gpu_grid(CD, make_node(P, model, WD.TOL, [1.0]), x, p, WD.TOL)
    times, save_start, want = WD.placement(kind, grid0)
    series = list(times)
    node = make_node(P, model, WD.TOL, [t for t in times if t > 0.0], save_start=save_start)
    cots = np.random.default_rng(31).standard_normal((len(series),) + x.shape).astype(f32)
    got = run(node, x, p, cots)
    assert [float(t) for t in got["info"]["sol_t"]] == [float(f32(t)) for t in series]
    grid, _ = WD.gpu_grid(CD, node, x, p, WD.TOL)
    assert grid == grid0
    pl = WD.check_placement(CD, kind, grid, series, save_start, want)
    print(f"{kind}: places {pl[:4]}{' ...' if len(pl) > 4 else ''}; launches {got['ai']['launches']}")
    assert got["ai"]["launches"] == 2 * len(grid) + WD.launch_c(len(series))
    check_vs_yardstick(f"placement {kind}", got, model, p, x, grid, series, cots)


# ---- 3. a forward that rejects steps: they do not appear in the sweep --------------------------------------------------
def test_rejected_attempts_do_not_appear(gpu_pkg):
    P = gpu_pkg
    model, p, x, times, cots, tol = WD.rejects_inputs(P)
    node = make_node(P, model, tol, times)
    got = run(node, x, p, cots)
    grid, st = WD.gpu_grid(CD, node, x, p, tol)
    sf, sb = got["info"]["stats_fwd"], got["info"]["stats_bwd"]
    print(f"forward naccept {sf['naccept']} nreject {sf['nreject']}; sweep {sb}")
    assert sf["nreject"] >= 1 and sb["naccept"] == sf["naccept"] == st["naccept"] and sb["nreject"] == 0
    check_vs_yardstick("rejecting forward", got, model, p, x, grid, times, cots)


# ---- 4. the regulariser rides on top, unchanged --------------------------------------------------------------------
@pytest.mark.parametrize("reg_type", ["error_estimate", "stiffness_estimate"])
@pytest.mark.parametrize("mode", ["unbiased", "biased"])
def test_regulariser_gradient_is_the_continuous_paths(gpu_pkg, mode, reg_type):
    """dp(w_reg = 2.5) - dp(0) on the discrete path against the same difference on the default (host-loop) path, at the
    bound of the regulariser row of DESIGN 4.9.1's table: max(1e-5, 4 x the distance of the float32 restatement's
    d reg / dp from the float64 one's); dx does not depend on w_reg, bit for bit"""
    P = gpu_pkg
    model = WC.shapes(P)["odd_td"]
    p, x = WC.mk_inputs(P, model, 9)
    times, tol, t1r = [0.25, 0.5, 1.0], WD.TOL, 0.43
    cots = np.random.default_rng(19).standard_normal((3,) + x.shape).astype(f32)
    kw = dict(mode=mode, reg_type=reg_type, t1_or_rand=t1r)
    r64 = CA.pullback(model, p, x, times, cots, tol, **kw)
    r32 = CA.pullback(model, p, x, times, cots, tol, dtype=np.float32, **kw)
    bound = max(1e-5, 4.0 * rel(r32["reg_grad"], r64["reg_grad"]))
    d = {}
    for loop in ("discrete", "auto"):
        node = make_node(P, model, tol, times, loop=loop, mode=mode, reg_type=reg_type)
        g0, gw = run(node, x, p, cots, w_reg=0.0), run(node, x, p, cots, w_reg=2.5)
        assert g0["ai"]["kind"] == gw["ai"]["kind"] == (5 if loop == "discrete" else 0)
        assert np.array_equal(g0["dx"], gw["dx"])
        assert gw["info"]["reg_val"] > 0
        d[loop] = gw["dp"].astype(np.float64) - g0["dp"].astype(np.float64)
    e = rel(d["discrete"], d["auto"])
    print(f"{mode} {reg_type}: rel(discrete dp(2.5) - dp(0), host loop's) {e:.2e} bound {bound:.2e}; |difference| {np.linalg.norm(d['auto']):.3e}")
    assert e <= bound, (e, bound)


# ---- 5. the two methods agree as the grid refines --------------------------------------------------------------------
def test_discrete_and_continuous_pullbacks_agree_at_tol_1e6(gpu_pkg):
    P = gpu_pkg
    model = WC.shapes(P)["mnist3"]
    p, x = WC.mk_inputs(P, model, 17)
    cots = np.random.default_rng(11).standard_normal((3,) + x.shape).astype(f32)
    d = run(make_node(P, model, 1e-6, WD.TIMES), x, p, cots)
    c = run(make_node(P, model, 1e-6, WD.TIMES, loop="auto"), x, p, cots)
    assert d["ai"]["kind"] == 5 and c["ai"]["kind"] == 0
    print(f"tol 1e-6: {d['info']['stats_bwd']['naccept']} steps, rel(discrete, continuous) dx {rel(d['dx'], c['dx']):.2e} dp {rel(d['dp'], c['dp']):.2e}")
    assert rel(d["dx"], c["dx"]) <= 3e-4 and rel(d["dp"], c["dp"]) <= 3e-4


# ---- 6. two launches per recorded step -----------------------------------------------------------------------------
def test_two_launches_per_recorded_step(gpu_pkg):
    P = gpu_pkg
    model = WC.shapes(P)["mnist3"]
    p, x = WC.mk_inputs(P, model, 17)
    cots = np.random.default_rng(11).standard_normal((3,) + x.shape).astype(f32)
    a = run(make_node(P, model, 1e-3, WD.TIMES), x, p, cots)
    b = run(make_node(P, model, 1e-6, WD.TIMES), x, p, cots)
    na, nb = a["info"]["stats_bwd"]["naccept"], b["info"]["stats_bwd"]["naccept"]
    print(f"tol 1e-3: {na} steps {a['ai']}; tol 1e-6: {nb} steps {b['ai']}")
    assert nb > na
    assert a["ai"]["launches"] == 2 * na + WD.LAUNCH_C and b["ai"]["launches"] == 2 * nb + WD.LAUNCH_C
    assert a["ai"]["host_waits"] == 0 and b["ai"]["host_waits"] == 0


# ---- 7. the same bits twice; a column does not depend on its neighbours or its place ------------------------------------
def test_repeats_bitwise_and_columns_are_independent(gpu_pkg):
    """The step grid belongs to the whole batch (the error norm runs over it), so a column "alone" is compared with a batch
    of 33 copies of it (three tiles, the last with one column), and a batch of 33 different columns with its permutation;
    the test first asserts that the compared solves took the same grid."""
    P = gpu_pkg
    model = WC.shapes(P)["mnist3"]
    p, X = WC.mk_inputs(P, model, 33)
    tol, times = WD.TOL, [0.3, 0.31, 1.0]
    cots = np.random.default_rng(14).standard_normal((3,) + X.shape).astype(f32)
    node = make_node(P, model, tol, times)
    r1, r2 = run(node, X, p, cots), run(node, X, p, cots)
    assert np.array_equal(r1["dx"], r2["dx"]) and np.array_equal(r1["dp"], r2["dp"])
    perm = np.random.default_rng(3).permutation(33)
    rp = run(node, X[perm], p, cots[:, perm])
    assert WD.gpu_grid(CD, node, X, p, tol)[0] == WD.gpu_grid(CD, node, X[perm], p, tol)[0]
    assert np.array_equal(rp["dx"], r1["dx"][perm])
    x1, c1 = X[5:6], cots[:, 5:6]
    alone = run(node, x1, p, c1)
    xs, cs = np.repeat(x1, 33, axis=0), np.repeat(c1, 33, axis=1)
    many = run(node, xs, p, cs)
    assert WD.gpu_grid(CD, node, x1, p, tol)[0] == WD.gpu_grid(CD, node, xs, p, tol)[0]
    for c in range(33):
        assert np.array_equal(many["dx"][c], alone["dx"][0]), c


# ---- 8. against the small chain's sweep ------------------------------------------------------------------------------
def test_physionet_through_both_discrete_sweeps(gpu_pkg):
    P = gpu_pkg
    model = WC.shapes(P)["physionet"]
    p, x = WC.mk_inputs(P, model, 9, scale=1.5)
    cots = np.random.default_rng(12).standard_normal((3,) + x.shape).astype(f32)
    wide_node = make_node(P, model, WD.TOL, WD.TIMES)
    small_node = make_node(P, model, WD.TOL, WD.TIMES, loop="auto", field="dense_chain", sensealg="TrackerAdjoint")
    w, s = run(wide_node, x, p, cots), run(small_node, x, p, cots)
    assert w["ai"]["kind"] == 5 and s["ai"]["kind"] == 4
    gw, gs = WD.gpu_grid(CD, wide_node, x, p, WD.TOL)[0], WD.gpu_grid(CD, small_node, x, p, WD.TOL)[0]
    print(f"grids equal: {gw == gs} ({len(gw)} / {len(gs)} steps); dx bit-equal: {np.array_equal(w['dx'], s['dx'])}; "
          f"rel(wide, small) dx {rel(w['dx'], s['dx']):.2e} dp {rel(w['dp'], s['dp']):.2e}")
    y64, y32 = yardstick("physionet both", model, p, x, gw, WD.TIMES, cots)
    for got, grid, tag in ((w, gw, "wide"), (s, gs, "small")):
        ys = (y64, y32) if grid == gw else yardstick("physionet small", model, p, x, grid, WD.TIMES, cots)
        for k, name in enumerate(("dx", "dp")):
            e, b = rel(got[name], ys[0][k]), CD.bound(ys[1][k], ys[0][k])
            print(f"physionet {tag} sweep: {name} rel {e:.2e} bound {b:.2e}")
            assert e <= b, (tag, name, e, b)
    assert rel(w["dx"], s["dx"]) <= 2e-5 and rel(w["dp"], s["dp"]) <= 2e-5


# ---- 9. refusals leave things usable ---------------------------------------------------------------------------------
def test_refusals(gpu_pkg):
    P = gpu_pkg
    from localregneuralde_jl_amd import _lib as L
    from localregneuralde_jl_amd.layers import Handle, _chain_desc, _mlp_desc
    phys = WC.shapes(P)["physionet"]
    mlp = P.TDChain(P.Chain(P.Dense(5, 8, "tanh"), P.Dense(9, 4)))
    hm, hs = Handle(_mlp_desc(mlp)), Handle(_chain_desc(phys))
    for hh in (hm, hs):
        assert L.lib.lrnde_set_adjoint_loop(hh._ctx, 2) == 8
        msg = L.lib.lrnde_last_error(hh._ctx).decode()
        assert "wide Dense-chain handle" in msg and "lrnde_set_sensealg" in msg, msg
        assert L.lib.lrnde_set_adjoint_loop(hh._ctx, 3) == 4
        assert L.lib.lrnde_set_adjoint_loop(hh._ctx, 1) == 0 and L.lib.lrnde_set_adjoint_loop(hh._ctx, 0) == 0
    pm = P.glorot_params(mlp, seed=0)
    hm.set_params(torch.from_numpy(pm))
    assert torch.isfinite(hm.rhs(dev(np.random.default_rng(0).random((3, 4), dtype=np.float32)), 0.1)).all()
    ps, xs = WC.mk_inputs(P, phys, 9, scale=1.5)
    hs.set_params(torch.from_numpy(ps))
    hs.node_forward_record(dev(xs), 0.0, 1.0, 1e-3, 1e-3, mode="none")
    assert torch.isfinite(hs.node_backward_recorded(dev(np.ones_like(xs)))["dp"]).all()
    # the wide handle: other codes, a backward without a record
    hw, p, x = WC.mk(P, phys, 9, scale=1.5)
    assert L.lib.lrnde_set_adjoint_loop(hw._ctx, 3) == 4 and L.lib.lrnde_set_adjoint_loop(hw._ctx, -1) == 4
    assert L.lib.lrnde_set_adjoint_loop(hw._ctx, 2) == 0
    with pytest.raises(L.LrndeError) as ei:
        hw.node_backward_recorded(dev(x))
    assert ei.value.code == 4
    hw.node_forward_record(dev(x), 0.0, 1.0, 1e-4, 1e-4, mode="none")
    bw = hw.node_backward_recorded(dev(np.ones_like(x)))
    assert hw.last_adjoint_info()["kind"] == 5 and torch.isfinite(bw["dp"]).all()
    # one batch past the gate
    model = WC.shapes(P)[WD.REFUSED_SHAPE]
    dims = WC.model_dims(model)
    B = WD.first_refused_batch(dims)
    assert WD.gate(dims, B)["why"] == "WIDE_SCRATCH_MAX" and WD.gate(dims, B - 1)["fits"]
    hb, pb, xb = WC.mk(P, model, B)
    hb.set_adjoint_loop("discrete")
    cot = dev(np.random.default_rng(5).standard_normal(xb.shape).astype(f32))
    fw = hb.node_forward_record(dev(xb), 0.0, 1.0, 1e-2, 1e-2, mode="none")
    gen = hb.record_generation()
    print(f"{WD.REFUSED_SHAPE} B={B}: forward naccept {fw['stats']['naccept']}")
    with pytest.raises(L.LrndeError) as ei:
        hb.node_backward_recorded(cot)
    assert ei.value.code == 8 and "WIDE_SCRATCH_MAX" in str(ei.value) and f"B = {B}" in str(ei.value), str(ei.value)
    assert hb.record_generation() == gen != 0   # the record is still there
    hb.set_adjoint_loop("auto")
    bw = hb.node_backward_recorded(cot)   # the same handle and record, on the host loop
    assert hb.last_adjoint_info()["kind"] == 0 and bw["stats_bwd"]["retcode"] == 0
    assert torch.isfinite(bw["dx"]).all() and torch.isfinite(bw["dp"]).all()


# ---- 10. training step ---------------------------------------------------------------------------------------------------
def test_training_step_takes_the_discrete_path(gpu_pkg):
    P = gpu_pkg
    model = WC.shapes(P)["mnist3"]
    B, K, D = 17, 10, 784
    p, x = WC.mk_inputs(P, model, B)
    rng = np.random.default_rng(2)
    xd, ps = dev(x), dev(p)
    pc = dev((rng.random(K * (D + 1), dtype=np.float32) - f32(0.5)) * f32(0.1))
    lab = torch.from_numpy(rng.integers(0, K, B).astype(np.int32)).cuda()
    kw = dict(regularize="unbiased", abstol=1e-6, reltol=1e-6, save_start=False, maxiters=10000, field="wide_chain")
    res = []
    for loop in ("discrete", "auto"):
        node = P.NeuralODE(model, adjoint_loop=loop, **kw)
        st = node.initialstates(np.random.default_rng(0))
        loss, _st2, stats, grads, _times = P.run_training_step(node, ps, pc, st, xd, lab, 2.5)
        res.append((loss, stats["y_pred"], grads, node.handle().last_adjoint_info()["kind"]))
    (l1, y1, g1, k1), (l0, y0, g0, k0) = res
    assert k1 == 5 and k0 == 0
    from localregneuralde_jl_amd.layers import Handle
    assert Handle.ADJOINT_LOOP_NAMES[k1] == "wide_discrete" and Handle.ADJOINT_LOOP_NAMES[k0] == "host"
    assert l1 == l0 and torch.equal(y1, y0)
    for key in ("neural_ode", "classifier", "x"):
        e = rel(g1[key].cpu().numpy(), g0[key].cpu().numpy())
        print(f"training step tol 1e-6: rel({key}) {e:.2e}")
        assert e <= 3e-4, (key, e)
