"""The conv handle's discrete adjoint (lrnde_conv_set_sensealg(LRNDE_SENSE_DISCRETE), csrc/lrnde_conv_discrete.hpp) through
ConvHandle against the frozen-grid yardstick of tests/conv_discrete_cases.py: torch autograd in float64 through Tsit5 steps
on the grid that record_steps() returns, over the torch restatement of the field (not the project's own C).  Per quantity
(dx and the five parameter blocks of dp): max |got - ref| over max |ref| of that quantity, bar max(5e-5, 4 x d32), d32 the
distance of the yardstick's own float32 run from its float64 run on the same grid (tests/test_host_conv_discrete.py caps
it at 2.5e-3; it is at most 2e-6 at every case, so every bar sits at the floor).  Every test prints its distances.

Measured on an MI355X, worst quantity of a row, d32 -> this device's (the three modes of a row share one grid and give the
same figures): 8x8 (7 steps) 1.6e-6 -> 2.5e-6, 8x8-test (6) 1.4e-6 -> 2.0e-6, 16x16-tanh (6) 2.1e-6 -> 3.0e-6, 12x3 (11)
1.2e-6 -> 2.2e-6, 4x2-train (7) 1.1e-6 -> 2.3e-6, 20x7-identity (8) 1.3e-6 -> 1.8e-6, 4x2-fwd-reject (21 accepted, 1
rejected) 1.1e-6 -> 1.7e-6, 8x8 with a global batch of 6 on 2 and on 3 ranks (8 steps) 1.6e-6 -> 2.5e-6.  At 8x8, tol 1e-4
the continuous route's gradient is 2.3e-6 of its scale from the discrete one: the bars tell a wrong sweep from a right
one, not one method from the other — the stats, the bitwise tests and nf do that."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import conv_discrete_cases as D
import conv_geometry_cases as G
import conv_pullback_cases as K

pytestmark = pytest.mark.gpu

YARD = [pytest.param(K.CASE[n], id=n) for n in D.YARDSTICK_CASES]
BADARG, UNSUPPORTED = 4, 8


def _handle(case, dtype="f32", inputs=None, sense="discrete"):
    import lrnde_amd as P
    p, _u, st = (inputs or K.case_inputs(case))[:3]
    h = P.ConvHandle(case.W, case.H, G.C, G.HC, act=case.act, bn_train=case.train, compute_dtype=dtype)
    if st is not None:
        h.set_bn_state(np.array(st))
    h.set_params(np.array(p))     # copies: the shared arrays are read-only
    if sense != "interpolating":
        h.set_sensealg(sense)
    return h


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()


def _check(what, case, dx, dp, dx_ref, dp_ref, bar, d32):
    """every quantity within its bar of the float64 yardstick; prints `d32 -> this device's / bar`"""
    d = K.distances(dx.cpu().numpy(), dp.cpu().numpy(), dx_ref, dp_ref)
    print(f"{what}: " + " ".join(f"{k} {d32[k]:.1e}->{v:.1e}/{bar[k]:.1e}" for k, v in d.items()))
    for name, v in d.items():
        where = ""
        if name == "dx":
            err = np.abs(dx.cpu().numpy().astype(np.float64) - np.asarray(dx_ref).reshape(tuple(dx.shape)))
            where = "; " + G.describe(err, case.W, case.H)
        assert np.isfinite(v) and v <= bar[name], f"{what}: {name}: {v:.3e} of its scale from the yardstick > {bar[name]:.3e}{where}"


def _record(h, case, mode, t1=K.T1, reg_type="error_estimate"):
    _p, u, _st, _w = K.case_inputs(case)
    return h.node_forward_record(_dev(u), K.T0, K.T2, case.tol, case.tol, mode=mode, reg_type=reg_type, t1_or_rand=t1,
                                 maxiters=K.MAXITERS)


def _stats_are_the_sweeps(sb, nsteps):
    assert (sb["naccept"], sb["iters"], sb["nreject"], sb["nf"]) == (nsteps, nsteps, 0, 6 * nsteps), (sb, nsteps)


def _traced_grid(h, case):
    """the accepted rows of a traced solve of the case's input"""
    _p, u, _st, _w = K.case_inputs(case)
    sol = h.solve(_dev(u), K.T0, K.T2, case.tol, case.tol, saveat=[K.T2], maxiters=K.MAXITERS, trace=True)
    acc = sol["trace"][sol["trace"]["accepted"] != 0]
    return acc["t"].copy(), acc["dt"].copy(), sol["stats"]


def _against_yardstick(case, modes):
    _p, _u, _st, w = K.case_inputs(case)
    h = _handle(case)
    tt, td, _ss = _traced_grid(h, case)
    for mode, t1 in modes:
        fw = _record(h, case, mode, t1)
        t, dt = h.record_steps()
        assert t.dtype == np.float32 and np.array_equal(t, tt) and np.array_equal(dt, td), (case.name, mode, t, tt, dt, td)
        assert len(t) == fw["stats"]["naccept"]
        grid = D.as_grid(t, dt)
        bw = h.node_backward_recorded(case.B, _dev(w), w_reg=0.0)
        _stats_are_the_sweeps(bw["stats_bwd"], len(t))
        _ue, dx64, dp64 = D.frozen_grads(case, grid)
        bar, d = D.bars(case, grid)
        _check(f"{case.name} {mode} ({len(t)} steps, {fw['stats']['nreject']} rejected)", case, bw["dx"], bw["dp"], dx64, dp64, bar, d)
    return len(tt)


# ---- 1. against the yardstick ----
@pytest.mark.parametrize("case", YARD)
def test_conv_discrete_adjoint_meets_the_frozen_grid_yardstick(case):
    """w_reg = 0 in the modes none, unbiased (t1 0.41) and biased: record_steps() is the accepted rows of a traced solve of
    the same input; dx and every block of dp are within the bars of float64 autograd through the Tsit5 steps of that grid"""
    nsteps = _against_yardstick(case, D.MODES)
    if case.name == "12x3":
        assert nsteps >= 6


# ---- 2. the rejecting case ----
def test_conv_discrete_adjoint_leaves_rejected_attempts_out():
    case = D.REJECT
    h = _handle(case)
    fw = _record(h, case, "none")
    assert fw["stats"]["nreject"] >= 1, f"{case.name}: the forward solve rejected nothing: {fw['stats']}"
    t, _dt = h.record_steps()
    assert len(t) == fw["stats"]["naccept"]
    _against_yardstick(case, (("none", K.T1), ("unbiased", K.T1)))


# ---- 3. stats ----
@pytest.mark.parametrize("name", ["12x3", "8x8-test"])
def test_conv_discrete_backward_stats(name):
    case = K.CASE[name]
    _p, u, _st, w = K.case_inputs(case)
    h = _handle(case)
    one = h.node_backward(_dev(u), K.T0, K.T2, case.tol, case.tol, _dev(w), mode="unbiased", t1_or_rand=K.T1, w_reg=2.5,
                          maxiters=K.MAXITERS)
    t, _dt = h.record_steps()
    if name == "12x3":
        assert len(t) >= 6
    assert one["stats_fwd"]["naccept"] == len(t)
    _stats_are_the_sweeps(one["stats_bwd"], len(t))
    assert one["stats_bwd"]["retcode"] == 0


# ---- 4. the regulariser alone ----
@pytest.mark.parametrize("mode", K.REG_LAYER_MODES)
def test_conv_discrete_regulariser_alone_is_the_continuous_routes(mode):
    """zero cotangent, w_reg = 1, both regulariser types: dx is exactly zero and dp is bit for bit what the continuous
    route returns from the same record"""
    case = K.CASE[D.REG_CASE]
    _p, _u, _st, w = K.case_inputs(case)
    zero = torch.zeros_like(_dev(w))
    h = _handle(case)
    for reg_type in K.REG_TYPES:
        _record(h, case, mode, reg_type=reg_type)
        bd = h.node_backward_recorded(case.B, zero, w_reg=1.0)
        h.set_sensealg("interpolating")
        bc = h.node_backward_recorded(case.B, zero, w_reg=1.0)
        h.set_sensealg("discrete")
        what = f"{case.name} {mode} {reg_type}"
        assert not torch.any(bd["dx"]), f"{what}: dx of a zero cotangent is not zero"
        assert float(bc["dp"].abs().max()) > 0.0, what
        assert torch.equal(bd["dp"], bc["dp"]), f"{what}: " + K.fmt(G.block_errors(bd["dp"].cpu().numpy(), bc["dp"].cpu().numpy().astype(np.float64)))


# ---- 5. one record, both routes ----
def test_conv_one_record_serves_both_routes():
    case = K.CASE["8x8"]
    _p, u, _st, w = K.case_inputs(case)
    ud, wd = _dev(u), _dev(w)
    h = _handle(case)
    fw = _record(h, case, "unbiased", reg_type="stiffness_estimate")
    a = h.node_backward_recorded(case.B, wd, w_reg=2.5)
    b = h.node_backward_recorded(case.B, wd, w_reg=2.5)
    assert torch.equal(a["dx"], b["dx"]) and torch.equal(a["dp"], b["dp"]) and a["stats_bwd"] == b["stats_bwd"]
    h.set_sensealg("interpolating")
    c = h.node_backward_recorded(case.B, wd, w_reg=2.5)
    fresh = _handle(case, sense="interpolating").node_backward(ud, K.T0, K.T2, case.tol, case.tol, wd, mode="unbiased",
                                                               reg_type="stiffness_estimate", t1_or_rand=K.T1, w_reg=2.5,
                                                               maxiters=K.MAXITERS)
    assert fresh["stats_fwd"] == fw["stats"]
    assert torch.equal(c["dx"], fresh["dx"]) and torch.equal(c["dp"], fresh["dp"]) and c["stats_bwd"] == fresh["stats_bwd"]
    assert c["stats_bwd"]["nf"] != a["stats_bwd"]["nf"] and not torch.equal(c["dp"], a["dp"])
    # the two methods differentiate the same map up to the solver's tolerance
    print("discrete against continuous: " + K.fmt(K.distances(a["dx"].cpu().numpy(), a["dp"].cpu().numpy(), c["dx"].cpu().numpy().astype(np.float64),
                                                               c["dp"].cpu().numpy().astype(np.float64))))


# ---- 6. refusals ----
def _raw_backward(h, B, du, w_reg, dx, dp):
    from localregneuralde_jl_amd import _lib as L
    sb = L.Stats()
    rc = L.lib.lrnde_conv_node_backward_recorded(h._ctx, int(B), C.c_void_p(du.data_ptr()), float(w_reg), C.c_void_p(dx.data_ptr()),
                                                 C.c_void_p(dp.data_ptr()), C.byref(sb))
    torch.cuda.synchronize()
    msg = L.lib.lrnde_conv_last_error(h._ctx)
    return rc, (msg.decode() if msg else "")


def test_conv_discrete_refusals_leave_the_handle_and_the_record_usable():
    from localregneuralde_jl_amd import _lib as L
    case = K.CASE["8x8"]
    _p, u, _st, w = K.case_inputs(case)
    ud, wd = _dev(u), _dev(w)
    h = _handle(case, sense="interpolating")
    f0 = h.rhs(ud, 0.3)
    # a bad code
    for bad in (-1, 2, 17):
        assert L.lib.lrnde_conv_set_sensealg(h._ctx, C.c_int32(bad)) == BADARG
    with pytest.raises(ValueError):
        h.set_sensealg("backsolve")
    assert torch.equal(h.rhs(ud, 0.3), f0)
    # record_steps without a record: a new handle, and after a plain solve has overwritten one
    with pytest.raises(L.LrndeError) as e:
        h.record_steps()
    assert e.value.code == BADARG and "no forward record" in str(e.value)
    _record(h, case, "none")
    assert len(h.record_steps()[0]) >= 1
    h.solve(ud, K.T0, K.T2, case.tol, case.tol, saveat=[K.T2])
    with pytest.raises(L.LrndeError) as e:
        h.record_steps()
    assert e.value.code == BADARG
    # cap too small: the count comes back, the arrays are left alone
    _record(h, case, "none")
    t1, dt1, n = np.full(1, -7.0, np.float32), np.full(1, -7.0, np.float32), C.c_int32(0)
    fp = C.POINTER(C.c_float)
    assert L.lib.lrnde_conv_record_steps(h._ctx, t1.ctypes.data_as(fp), dt1.ctypes.data_as(fp), 1, C.byref(n)) == BADARG
    assert n.value == len(h.record_steps()[0]) > 1 and t1[0] == -7.0 and dt1[0] == -7.0
    # DISCRETE on the other compute dtypes
    for dtype in ("bf16", "f32_split"):
        hd = _handle(case, dtype, sense="interpolating")
        with pytest.raises(L.LrndeError) as e:
            hd.set_sensealg("discrete")
        assert e.value.code == UNSUPPORTED and dtype in str(e.value)
        assert hd.sensealg == "interpolating"
        bw = hd.node_backward(ud, K.T0, K.T2, case.tol, case.tol, wd, mode="none", maxiters=K.MAXITERS)   # still usable, continuous
        assert bw["stats_bwd"]["nf"] != 6 * bw["stats_bwd"]["naccept"] and bool(torch.isfinite(bw["dp"]).all())
    # DISCRETE with a VCAB3 record
    h.set_solver("vcab3")
    h.set_sensealg("discrete")
    _record(h, case, "unbiased")
    gen = h.record_steps()
    dx, dp = torch.full_like(ud, -3.0), torch.full((h.param_count(),), -3.0, device="cuda")
    rc, msg = _raw_backward(h, case.B, wd, 2.5, dx, dp)
    assert rc == UNSUPPORTED and "not a Tsit5 stage record" in msg, (rc, msg)
    assert bool((dx == -3.0).all()) and bool((dp == -3.0).all()), "a refused backward wrote to its outputs"
    with pytest.raises(L.LrndeError) as e:   # the one-call form refuses before its forward
        h.node_backward(ud, K.T0, K.T2, case.tol, case.tol, wd, mode="unbiased", t1_or_rand=K.T1, maxiters=K.MAXITERS)
    assert e.value.code == UNSUPPORTED and "not a Tsit5 stage record" in str(e.value)
    again = h.record_steps()
    assert np.array_equal(gen[0], again[0]) and np.array_equal(gen[1], again[1])
    h.set_sensealg("interpolating")
    bw = h.node_backward_recorded(case.B, wd, w_reg=2.5)   # the same record, served by the continuous route
    ref = _handle(case, sense="interpolating")
    ref.set_solver("vcab3")
    want = ref.node_backward(ud, K.T0, K.T2, case.tol, case.tol, wd, mode="unbiased", t1_or_rand=K.T1, w_reg=2.5, maxiters=K.MAXITERS)
    assert torch.equal(bw["dx"], want["dx"]) and torch.equal(bw["dp"], want["dp"])


# ---- 7. sharded ----
@pytest.mark.parametrize("R", [2, 3])
def test_conv_discrete_adjoint_sharded(R):
    """R ranks through LocalComm on one GPU, a global batch of 6 from the 8x8 row's recipe: the concatenated dx and every
    rank's dp meet the yardstick on the global batch; dp is bitwise equal across ranks"""
    import conv_sharded_cases as S
    base = K.CASE[D.SHARDED_CASE]
    case = base._replace(name="8x8-B6", B=6)
    p, u, st, w = K.case_inputs(case)
    Bl = case.B // R
    lc, hs = S._ranks(R, case.W, case.H, np.array(p), None, act=case.act, train=case.train)
    for h in hs:
        h.set_sensealg("discrete")
    us, ws = S._shards(np.array(u), R), S._shards(np.array(w), R)

    def rank(r):
        fw = hs[r].node_forward_record(us[r], K.T0, K.T2, case.tol, case.tol, mode="unbiased", t1_or_rand=K.T1, maxiters=K.MAXITERS)
        return fw, hs[r].record_steps(), hs[r].node_backward_recorded(Bl, ws[r], w_reg=0.0)

    got = S._run([(lambda r=r: rank(r)) for r in range(R)])
    t, dt = got[0][1]
    for fw, steps, bw in got:
        assert np.array_equal(steps[0], t) and np.array_equal(steps[1], dt)
        _stats_are_the_sweeps(bw["stats_bwd"], len(t))
        assert torch.equal(bw["dp"], got[0][2]["dp"]), "dp must come out replicated"
    grid = D.as_grid(t, dt)
    _ue, dx64, dp64 = D.frozen_grads(case, grid)
    bar, d = D.bars(case, grid)
    dx = torch.cat([g[2]["dx"] for g in got])
    for r in range(R):
        _check(f"{case.name} rank {r} ({len(t)} steps)", case, dx, got[r][2]["dp"], dx64, dp64, bar, d)
    lc.close()


# ---- 8. the training step follows the layer ----
def test_cifar_training_step_follows_the_layers_sensealg():
    import lrnde_amd as P
    W = H = 8; B = 4; Kc = 10
    rng = np.random.default_rng(12)
    core = P.TDChain(P.Chain(P.Chain(P.Conv((3, 3), 9, 64), P.BatchNorm(64, "gelu")),
                             P.Chain(P.Conv((3, 3), 65, 64), P.BatchNorm(64, "gelu")), P.Conv((3, 3), 65, 8)))
    pn = P.glorot_conv_params(8, 64, seed=0)
    ps = (rng.standard_normal(156) * 0.3).astype(np.float32); ps[140:148] = 1.0; ps[148:156] = 0.0
    ph = (rng.standard_normal(73 + Kc * H * W + Kc) * 0.1).astype(np.float32)
    x = _dev(rng.standard_normal((B, 3, H, W)))
    lab = torch.from_numpy(rng.integers(0, Kc, B).astype(np.int32)).cuda()
    params = dict(stem=_dev(ps), neural_ode=_dev(pn), head=_dev(ph))
    kw = dict(regularize="unbiased", abstol=1e-3, reltol=1e-3, save_start=False, maxiters=2000)
    node = P.NeuralODE(core, sensealg="TrackerAdjoint", **kw)
    st = node.initialstates(np.random.default_rng(0))
    loss, _st, stats, grads, times = P.run_cifar_training_step(node, params, copy.deepcopy(st), x, lab, 2.5)
    assert node.handle().sensealg == "discrete"
    # the handle-level discrete pullback of the same du
    t1 = np.float32(copy.deepcopy(st["rng"]).random(dtype=np.float32))
    h = P.ConvHandle(W, H, 8, 64, act="gelu", bn_train=True)
    h.set_params(pn)
    h.set_sensealg("discrete")
    u0 = h.cifar_stem_forward(x, params["stem"])
    fw = h.node_forward_record(u0, 0.0, 1.0, 1e-3, 1e-3, mode="unbiased", reg_type="error_estimate", t1_or_rand=t1, maxiters=2000)
    head = h.cifar_head_ce(fw["u_end"], params["head"], Kc, lab)
    nsteps = len(h.record_steps()[0])
    bw = h.node_backward_recorded(B, head["du"], w_reg=2.5)
    assert fw["stats"] == times["forward"] and nsteps == times["forward"]["naccept"]
    assert torch.equal(grads["neural_ode"], bw["dp"])
    assert times["adjoint"]["nf"] == 6 * nsteps and times["adjoint"] == bw["stats_bwd"]
    # pullback names the route; a rebuilt handle (another image size) inherits the setting
    stp = node.initialstates(np.random.default_rng(0))
    _dx, _dp, info = node.pullback(u0, params["neural_ode"], stp, head["du"], w_reg=2.5)
    assert info["adjoint_loop"] == "conv_discrete" and info["stats_bwd"]["nf"] == 6 * nsteps
    assert torch.equal(_dp, bw["dp"])
    assert node.handle(torch.empty((2, 8, 4, 4), device="cuda")).sensealg == "discrete"
    # the default layer: the continuous counts
    node_c = P.NeuralODE(core, **kw)
    _l, _s, _stats, grads_c, times_c = P.run_cifar_training_step(node_c, params, copy.deepcopy(st), x, lab, 2.5)
    adj = times_c["adjoint"]
    assert node_c.handle().sensealg == "interpolating"
    assert adj["nf"] == 3 + 6 * (adj["naccept"] + adj["nreject"]) and adj["iters"] == adj["naccept"] + adj["nreject"]
    assert times_c["forward"] == times["forward"] and not torch.equal(grads_c["neural_ode"], grads["neural_ode"])
    _dx, _dp, info_c = node_c.pullback(u0, params["neural_ode"], stp, head["du"], w_reg=2.5)
    assert info_c["adjoint_loop"] is None
