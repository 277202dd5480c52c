"""VCAB3 / VCABM3 on the conv handle (csrc/lrnde_conv_adams.hpp; lrnde_conv_set_solver).

Two yardsticks, neither of them the code under test:
  (R) the C oracle's adams_solve (start-up, recurrences, controller, Hermite saves, counters) run around the handle's OWN
      f-evals: oracle.PyField over ConvHandle.rhs.  Everything the solver adds is held to it with ==, the method of
      tests/test_gpu_chain_adams.py.
  (O) the oracle with its own conv f-evals (oracle.ConvField): accept patterns, counters and — at the bars
      tests/test_gpu_conv.py holds the Tsit5 solve to — states, the layer forward and the pullback.
Cases and their reasons: tests/conv_adams_cases.py (tests/test_host_conv_adams.py re-derives them on the CPU)."""
import copy

import numpy as np
import pytest
import torch

import conv_adams_cases as K
from conv_sharded_cases import BN0, _dist, _handle, _ranks, _rel, _run, _shards

pytestmark = pytest.mark.gpu

SOLVERS = K.SOLVERS
STAT_KEYS = ("nf", "naccept", "nreject", "iters", "nsaved", "t_final", "eest_last", "dt_init")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rhs_field(O, h, D):
    """the oracle's view of the handle's field: upload, the handle's five f-eval launches, download"""
    return O.PyField(D, lambda u, t: h.rhs(cu(u), float(t)).cpu().numpy())


def solve_equal(got, ref):
    assert len(got["trace"]) == len(ref["trace"]), (len(got["trace"]), len(ref["trace"]))
    for i, (a, b) in enumerate(zip(got["trace"], ref["trace"])):
        assert tuple(a) == tuple(b), (i, tuple(a), tuple(b))
    for k in STAT_KEYS:
        assert got["stats"][k] == ref["stats"][k], (k, got["stats"], ref["stats"])
    assert np.array_equal(got["t"], ref["t"])
    assert np.array_equal(got["u"].cpu().numpy().reshape(ref["u"].shape), ref["u"])


def nf_of(trace, solver):
    """3 for the initial dt, 3 per start-up attempt, 1 (VCAB3) or 2 (VCABM3) per multistep attempt"""
    per = 2 if solver == "vcabm3" else 1
    nstart = acc = 0
    for r in trace:
        nstart += acc < 2
        acc += int(r["accepted"])
    return 3 + 3 * nstart + per * (len(trace) - nstart)


# ---- 1. bits: solve == the oracle's adams_solve around the handle's f-evals, attempt by attempt ----
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", list(K.CASES))
def test_solve_equals_the_oracle_attempt_by_attempt(oracle, gpu_pkg, name, solver):
    c = K.CASES[name]
    h, x = K.handle(c)
    D = x[0].numel()
    ref = oracle.solve(rhs_field(oracle, h, D), x.cpu().numpy().reshape(c["B"], -1), 0.0, 1.0, c["tol"], c["tol"], saveat=K.SAVEAT,
                       save_start=True, solver=solver)
    h.set_solver(solver)
    got = h.solve(x, 0.0, 1.0, c["tol"], c["tol"], saveat=K.SAVEAT, save_start=True, trace=True)
    assert ref["retcode"] == 0 and got["retcode"] == 0
    cov = K.coverage(ref["trace"])
    print(name, solver, cov)
    assert cov["attempts"] <= K.MAX_ATTEMPTS
    if name in K.MULTISTEP_REJECTS[solver]:
        assert cov["multistep_rejects"] >= 1, cov
    if name == "kick":
        assert cov["startup_rejects"] >= 1, cov
    assert cov["max_points_in_a_step"] >= 2
    solve_equal(got, ref)
    assert list(ref["t"]) == [np.float32(s) for s in K.SAVEAT]
    assert got["stats"]["nf"] == nf_of(ref["trace"], solver)


@pytest.mark.parametrize("solver", SOLVERS)
def test_solve_equals_the_oracle_in_another_compute_dtype(oracle, gpu_pkg, solver):
    """the loop only calls the handle's f-eval: the bf16 kernels under the same solver, same bits"""
    c = K.CASES[K.DTYPE_CASE]
    h, x = K.handle(c, dtype=K.OTHER_DTYPE)
    ref = oracle.solve(rhs_field(oracle, h, x[0].numel()), x.cpu().numpy().reshape(c["B"], -1), 0.0, 1.0, c["tol"], c["tol"],
                       saveat=K.SAVEAT, save_start=True, solver=solver)
    h32, _ = K.handle(c)
    assert not torch.equal(h.rhs(x, 0.3), h32.rhs(x, 0.3))   # it IS another f-eval
    h.set_solver(solver)
    got = h.solve(x, 0.0, 1.0, c["tol"], c["tol"], saveat=K.SAVEAT, save_start=True, trace=True)
    assert ref["retcode"] == 0
    solve_equal(got, ref)


@pytest.mark.parametrize("solver", SOLVERS)
def test_every_step_series_with_a_start_value_equals_the_oracle(oracle, gpu_pkg, solver):
    c = K.CASES["plain8"]
    h, x = K.handle(c)
    ref = oracle.solve(rhs_field(oracle, h, x[0].numel()), x.cpu().numpy().reshape(c["B"], -1), 0.0, 1.0, c["tol"], c["tol"],
                       save_start=True, solver=solver)
    h.set_solver(solver)
    got = h.solve(x, 0.0, 1.0, c["tol"], c["tol"], save_start=True, trace=True)
    solve_equal(got, ref)
    assert len(ref["t"]) == ref["stats"]["naccept"] + 1 > 10 and ref["t"][0] == 0.0


# ---- 2. against the oracle's own conv f-evals ----
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("name", K.ORACLE_CASES)
def test_solve_matches_the_oracle_field_step_for_step(oracle, gpu_pkg, name, solver):
    """test_conv_solve_matches_oracle_step_for_step's assertions and bars; the running statistics after the solve at
    test_conv_running_statistics_match_oracle's tolerance"""
    c = K.CASES[name]
    fld, u = K.oracle_field(c)
    ro = oracle.solve(fld, u, 0.0, 1.0, c["tol"], c["tol"], saveat=[0.37, 1.0], solver=solver)
    h, x = K.handle(c)
    h.set_solver(solver)
    rg = h.solve(x, 0.0, 1.0, c["tol"], c["tol"], saveat=[0.37, 1.0], trace=True)
    so, sg = ro["stats"], rg["stats"]
    assert ro["retcode"] == 0
    e = ro["trace"]["eest"]
    assert not np.any((e >= 0.95) & (e <= 1.05)), "the oracle's own trace has an attempt at the accept threshold"
    assert (sg["naccept"], sg["nreject"], sg["nf"]) == (so["naccept"], so["nreject"], so["nf"])
    assert np.array_equal(rg["trace"]["accepted"], ro["trace"]["accepted"])
    np.testing.assert_allclose(rg["trace"]["dt"], ro["trace"]["dt"], rtol=1e-2)
    assert list(rg["t"]) == [np.float32(0.37), np.float32(1.0)]
    for i in range(2):
        d = _dist(rg["u"][i], ro["u"][i])
        print(f"{name} {solver} save {i}: {d:.3e} of scale")
        assert d <= 2e-5
    np.testing.assert_allclose(h.get_bn_state().cpu().numpy(), fld.bn_run, rtol=5e-3, atol=5e-4)


# ---- 3. layer ----
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("mode,reg_type", [("unbiased", "error_estimate"), ("biased", "stiffness_estimate"), ("none", "error_estimate")])
def test_node_forward_matches_the_oracle(oracle, gpu_pkg, mode, reg_type, solver):
    """test_conv_node_forward_matches_oracle's assertions and tolerances, on its inputs (case plain8)"""
    c = K.CASES["plain8"]
    fld, u = K.oracle_field(c)
    ro = oracle.node_forward(fld, u, 0.0, 1.0, 1e-3, 1e-3, mode=mode, reg_type=reg_type, t1_or_rand=0.41, solver=solver)
    h, x = K.handle(c)
    h.set_solver(solver)
    rg = h.node_forward(x, 0.0, 1.0, 1e-3, 1e-3, mode=mode, reg_type=reg_type, t1_or_rand=0.41)
    assert ro["retcode"] == 0
    assert rg["nfe"] == ro["nfe"]
    assert rg["stats"]["naccept"] == ro["stats"]["naccept"] and rg["stats"]["nreject"] == ro["stats"]["nreject"]
    assert _dist(rg["u_end"], ro["u_end"]) <= 2e-5
    if mode == "none":
        assert rg["reg_val"] == 0.0 and ro["reg_val"] == 0.0 and rg["nfe"] == rg["stats"]["nf"]
    else:
        assert rg["nfe"] == rg["stats"]["nf"] + 9       # the local step stays Tsit5: 3 for its dt, 6 stages
        assert abs(float(rg["reg_val"]) - float(ro["reg_val"])) <= 1e-1 * abs(float(ro["reg_val"]))
        if mode == "unbiased":
            assert rg["t1"] == ro["t1"] == np.float32(0.41)
        else:
            assert abs(float(rg["t1"]) - float(ro["t1"])) <= 2e-3


def _core(P):
    return P.TDChain(P.Chain(P.Chain(P.Conv((3, 3), 9, 64), P.BatchNorm(64, "gelu")), P.Chain(P.Conv((3, 3), 65, 64), P.BatchNorm(64, "gelu")),
                             P.Conv((3, 3), 65, 8)))


def test_the_layer_call_runs_the_handles_solver_and_keeps_it_across_image_sizes(gpu_pkg):
    P = gpu_pkg
    c = K.CASES["plain8"]
    p, u, _st, _act = K.inputs(c)
    node = P.NeuralODE(_core(P), regularize="unbiased", abstol=1e-3, reltol=1e-3, save_start=False, maxiters=1000)
    ps, x = cu(p), cu(u)
    st = node.initialstates(np.random.default_rng(0))
    node.handle(x).set_solver("vcab3")
    sol, st2 = node(x, ps, st)
    t1 = np.float32(copy.deepcopy(st["rng"]).random(dtype=np.float32) * np.float32(1.0) + np.float32(0.0))
    h = _handle(c["W"], c["H"], p, None)
    h.set_solver("vcab3")
    fw = h.node_forward(x, 0.0, 1.0, 1e-3, 1e-3, mode="unbiased", t1_or_rand=t1, maxiters=1000)
    assert torch.equal(sol.u[-1], fw["u_end"]) and st2["nfe"] == fw["nfe"] == sol.destats.nf + 9
    assert np.float32(st2["reg_val"]) == np.float32(fw["reg_val"]) and sol.destats.naccept == fw["stats"]["naccept"]
    h.set_solver("tsit5")
    h.set_bn_state(BN0)
    assert h.node_forward(x, 0.0, 1.0, 1e-3, 1e-3, mode="unbiased", t1_or_rand=t1)["stats"]["nf"] != fw["stats"]["nf"]
    # another image size: the layer rebuilds its conv handle, the new one inherits the solver
    c16 = K.CASES["plain16"]
    p16, u16, _s, _a = K.inputs(c16)
    old = node.handle()
    sol16, _ = node(cu(u16), cu(p16), st)
    assert node.handle() is not old and node.handle().solver == "vcab3"
    h16 = _handle(16, 16, p16, None)
    h16.set_solver("vcab3")
    fw16 = h16.node_forward(cu(u16), 0.0, 1.0, 1e-3, 1e-3, mode="unbiased", t1_or_rand=t1, maxiters=1000)
    assert torch.equal(sol16.u[-1], fw16["u_end"]) and sol16.destats.nf == fw16["stats"]["nf"]


# ---- 4. pullback ----
def _pullback_inputs():
    c = K.PULLBACK
    wv = np.random.default_rng(3).standard_normal((c["B"], 8, c["H"], c["W"])).astype(np.float32)
    return c, wv


@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("mode", ["unbiased", "none"])
def test_node_backward_matches_the_oracle(oracle, gpu_pkg, mode, solver):
    """test_conv_node_backward_matches_oracle's inputs and bars: dx 2e-3, dp 5e-3, forward accepted equal, backward accepted +-1"""
    c, wv = _pullback_inputs()
    fld, u = K.oracle_field(c)
    bo = oracle.node_backward(fld, u, 0.0, 1.0, c["tol"], c["tol"], wv.reshape(c["B"], -1), mode=mode, t1_or_rand=0.41, w_reg=2.5,
                              maxiters=5000, solver=solver)
    h, x = K.handle(c)
    h.set_solver(solver)
    bg = h.node_backward(x, 0.0, 1.0, c["tol"], c["tol"], cu(wv), mode=mode, t1_or_rand=0.41, w_reg=2.5, maxiters=5000)
    assert bo["retcode"] == 0
    assert bg["stats_fwd"]["naccept"] == bo["stats_fwd"]["naccept"] and bg["stats_fwd"]["nf"] == bo["stats_fwd"]["nf"]
    assert abs(bg["stats_bwd"]["naccept"] - bo["stats_bwd"]["naccept"]) <= 1
    ex, ep = _rel(bg["dx"].cpu().numpy().reshape(c["B"], -1), bo["dx"]), _rel(bg["dp"], bo["dp"])
    print(f"{solver} {mode}: dx {ex:.3e} dp {ep:.3e}")
    assert ex <= 2e-3 and ep <= 5e-3


@pytest.mark.parametrize("solver", SOLVERS)
def test_recorded_backward_equals_the_one_call_form_and_the_record_is_invalidated(gpu_pkg, solver):
    P = gpu_pkg
    c, wv = _pullback_inputs()
    B, tol = c["B"], c["tol"]
    h, x = K.handle(c)
    w = cu(wv)
    # the Tsit5 pullback of a handle that never saw another solver: the parent's path
    tsit5 = h.node_backward(x, 0.0, 1.0, tol, tol, w, mode="unbiased", t1_or_rand=0.37, w_reg=2.5, maxiters=5000)
    h.set_solver(solver)
    h.set_bn_state(BN0)
    one = h.node_backward(x, 0.0, 1.0, tol, tol, w, mode="unbiased", t1_or_rand=0.37, w_reg=2.5, maxiters=5000)
    h.set_bn_state(BN0)
    fw_plain = h.node_forward(x, 0.0, 1.0, tol, tol, mode="unbiased", t1_or_rand=0.37, maxiters=5000)
    h.set_bn_state(BN0)
    fw = h.node_forward_record(x, 0.0, 1.0, tol, tol, mode="unbiased", t1_or_rand=0.37, maxiters=5000)
    assert torch.equal(fw["u_end"], fw_plain["u_end"]) and fw["reg_val"] == fw_plain["reg_val"] and fw["nfe"] == fw_plain["nfe"]
    two = h.node_backward_recorded(B, w, w_reg=2.5)
    assert torch.equal(two["dx"], one["dx"]) and torch.equal(two["dp"], one["dp"]) and two["stats_bwd"] == one["stats_bwd"]
    assert one["stats_fwd"]["nf"] != tsit5["stats_fwd"]["nf"] and not torch.equal(one["dx"], tsit5["dx"])
    # for scale only (the oracle's Adams and Tsit5 pullbacks differ by 1e-4 .. 1.1e-3 on these inputs)
    print(solver, "vs Tsit5: dx", _rel(one["dx"], tsit5["dx"]), "dp", _rel(one["dp"], tsit5["dp"]))
    # a plain solve invalidates the record; so does the setter
    h.solve(x, 0.0, 1.0, tol, tol, saveat=[1.0])
    with pytest.raises(P.LrndeError):
        h.node_backward_recorded(B, w, w_reg=2.5)
    h.set_bn_state(BN0)
    h.node_forward_record(x, 0.0, 1.0, tol, tol, mode="unbiased", t1_or_rand=0.37, maxiters=5000)
    h.set_solver("tsit5")
    with pytest.raises(P.LrndeError):
        h.node_backward_recorded(B, w, w_reg=2.5)
    # a Tsit5 record made after switching back pulls back to the bits of the handle that never switched
    h.set_bn_state(BN0)
    h.node_forward_record(x, 0.0, 1.0, tol, tol, mode="unbiased", t1_or_rand=0.37, maxiters=5000)
    back = h.node_backward_recorded(B, w, w_reg=2.5)
    assert torch.equal(back["dx"], tsit5["dx"]) and torch.equal(back["dp"], tsit5["dp"]) and back["stats_bwd"] == tsit5["stats_bwd"]


# ---- 5. sharded ----
@pytest.mark.parametrize("solver", SOLVERS)
def test_sharded_solve(oracle, gpu_pkg, solver):
    """two ranks through the local communicator, case plain8 split 2 + 2: test_sharded_solve_and_node_forward's criterion —
    stats and traces equal on all ranks and equal to the unsharded handle's, counters equal the oracle's, saved states within
    2e-5 of scale of both"""
    c = K.CASES["plain8"]
    R, tol = 2, c["tol"]
    p, u, st, act = K.inputs(c)
    fld, uf = K.oracle_field(c)
    ro = oracle.solve(fld, uf, 0.0, 1.0, tol, tol, saveat=[0.37, 1.0], solver=solver)
    hu, x = K.handle(c)
    hu.set_solver(solver)
    ru = hu.solve(x, 0.0, 1.0, tol, tol, saveat=[0.37, 1.0], trace=True)
    lc, hs = _ranks(R, c["W"], c["H"], p, None)
    for h in hs:
        h.set_solver(solver)
    us = _shards(u, R)
    got = _run([(lambda r=r: hs[r].solve(us[r], 0.0, 1.0, tol, tol, saveat=[0.37, 1.0], trace=True)) for r in range(R)])
    so = ro["stats"]
    for g in got:
        assert g["stats"] == got[0]["stats"] and g["stats"] == ru["stats"]
        assert (g["stats"]["naccept"], g["stats"]["nreject"], g["stats"]["nf"]) == (so["naccept"], so["nreject"], so["nf"])
        for f in ("t", "dt", "eest", "accepted"):
            assert np.array_equal(g["trace"][f], got[0]["trace"][f]), f
        assert list(g["t"]) == [np.float32(0.37), np.float32(1.0)]
    for i in range(2):
        ui = torch.cat([g["u"][i] for g in got])
        du, do = _dist(ui, ru["u"][i].cpu().numpy()), _dist(ui, ro["u"][i])
        print(f"{solver} save {i}: vs unsharded {du:.3e}, vs oracle {do:.3e}")
        assert du <= 2e-5 and do <= 2e-5
    bn = [h.get_bn_state() for h in hs]
    assert torch.equal(bn[0], bn[1])
    lc.close()


# ---- 6. training step ----
def test_cifar_training_step_with_the_handle_on_vcab3(oracle, gpu_pkg):
    """test_cifar_training_step_runs_and_is_consistent's assertions with the NeuralODE's handle on VCAB3, on case plain8's
    field; the step's solve takes fewer f-evals than the Tsit5 step's"""
    P, O = gpu_pkg, oracle
    c = K.CASES["plain8"]
    W, H, B, Kc = c["W"], c["H"], c["B"], 10
    pn = K.inputs(c)[0]
    rng = np.random.default_rng(12)
    ps = (rng.standard_normal(156) * 0.3).astype(np.float32); ps[140:148] = 1.0; ps[148:156] = 0.0
    ph = (rng.standard_normal(73 + Kc * H * W + Kc) * 0.1).astype(np.float32)
    x = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    lab = rng.integers(0, Kc, B).astype(np.int32)
    params = dict(stem=cu(ps), neural_ode=cu(pn), head=cu(ph))
    out = {}
    for solver in ("tsit5", "vcab3"):
        node = P.NeuralODE(_core(P), regularize="unbiased", abstol=1e-3, reltol=1e-3, save_start=False, maxiters=2000)
        st = node.initialstates(np.random.default_rng(0))
        node.handle(torch.empty((B, 8, H, W), device="cuda")).set_solver(solver)
        out[solver] = P.run_cifar_training_step(node, params, st, cu(x), cu(lab), 2.5)
    loss, st_, stats, grads, times = out["vcab3"]
    assert times["forward"]["nf"] < out["tsit5"][4]["forward"]["nf"]
    assert stats["nfe"] == times["forward"]["nf"] + 9
    assert np.isfinite(loss) and times["fwd_time"] > 0 and times["bwd_time"] > 0
    assert grads["stem"].shape == (156,) and grads["neural_ode"].shape == (47560,) and grads["head"].shape == ph.shape
    assert all(torch.isfinite(g).all() and g.abs().max() > 0 for g in grads.values())
    t1 = np.float32(copy.deepcopy(st["rng"]).random(dtype=np.float32))
    u0 = O.cifar_stem_forward(x, ps)
    fld = O.ConvField(W, H, 8, 64, pn, nthreads=8)
    fo = O.node_forward(fld, u0.reshape(B, -1), 0.0, 1.0, 1e-3, 1e-3, mode="unbiased", t1_or_rand=t1, maxiters=2000, solver="vcab3")
    lo, lg, du, dph = O.cifar_head_ce(fo["u_end"].reshape(B, 8, H, W), ph, Kc, lab)
    assert abs(float(stats["ce_loss"]) - float(lo)) <= 1e-4 * abs(float(lo))
    bo = O.node_backward(fld, u0.reshape(B, -1), 0.0, 1.0, 1e-3, 1e-3, du.reshape(B, -1), mode="unbiased", t1_or_rand=t1, w_reg=2.5,
                         maxiters=2000, solver="vcab3")
    dstem = O.cifar_stem_backward(x, ps, bo["dx"].reshape(B, 8, H, W))
    assert _rel(grads["neural_ode"], bo["dp"]) <= 1e-2
    assert _rel(grads["head"], dph) <= 1e-3
    assert _rel(grads["stem"], dstem) <= 1e-2


# ---- 7. the setter ----
def test_the_setter_refuses_other_codes_and_tsit5_after_adams_gives_the_parents_bits(gpu_pkg):
    import ctypes as C
    from localregneuralde_jl_amd import _lib as L
    P = gpu_pkg
    c = K.CASES["plain8"]
    h, x = K.handle(c)
    fresh = h.solve(x, 0.0, 1.0, c["tol"], c["tol"], saveat=K.SAVEAT, save_start=True, trace=True)
    for bad in (-1, 3, 17):
        assert L.lib.lrnde_conv_set_solver(h._ctx, C.c_int32(bad)) == 4   # LRNDE_BADARG
    with pytest.raises(ValueError):
        h.set_solver("rk4")
    h.set_bn_state(BN0)
    again = h.solve(x, 0.0, 1.0, c["tol"], c["tol"], saveat=K.SAVEAT, save_start=True, trace=True)   # still usable, still Tsit5
    solve_equal(again, dict(fresh, u=fresh["u"].cpu().numpy()))
    h.set_solver("vcabm3")
    adams = h.solve(x, 0.0, 1.0, c["tol"], c["tol"], saveat=K.SAVEAT, save_start=True, trace=True)
    assert adams["stats"]["nf"] != fresh["stats"]["nf"]
    h.set_solver("Tsit5()")
    h.set_bn_state(BN0)
    back = h.solve(x, 0.0, 1.0, c["tol"], c["tol"], saveat=K.SAVEAT, save_start=True, trace=True)
    solve_equal(back, dict(fresh, u=fresh["u"].cpu().numpy()))
    assert torch.equal(h.get_bn_state(), _bn_after_fresh(c))


def _bn_after_fresh(c):
    h, x = K.handle(c)
    h.solve(x, 0.0, 1.0, c["tol"], c["tol"], saveat=K.SAVEAT, save_start=True)
    return h.get_bn_state()
