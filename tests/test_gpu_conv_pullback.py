"""The conv field's layer pullback (lrnde_conv_node_backward, lrnde_conv_node_backward_recorded,
lrnde_conv_step_reg_grad) through ConvHandle against float64: classical RK4 with autograd for the solution cotangent, one
float64 Tsit5 step with autograd for the regulariser (tests/conv_pullback_cases.py, neither is the project's own C).
Per quantity (dx and each of the five parameter blocks of dp): max |got - ref| over max |ref| of that quantity, bar
max(5e-5, 4 x the fp32 oracle's own distance from float64).  tests/test_host_conv_pullback.py caps those distances at
2.5e-3, so no bar exceeds 1e-2.  Every test prints its distances; a failure names the block, and for dx the strip and tile.

Measured, worst quantity of each row, fp32 oracle's distance from float64 -> MI355X's (none / unbiased 0.41 / biased):
  8x8 3.5e-6 -> 3.7e-6 / 2.4e-6 -> 2.3e-6 / 1.5e-6 -> 1.9e-6 (t1 1.2e-4: 3.4e-6 -> 3.8e-6, t1 0.9995: 2.4e-6 -> 3.3e-6);
  8x8-test 1.5e-6 -> 1.4e-6 / 1.8e-6 -> 1.3e-6 / 1.3e-6 -> 1.5e-6; 16x16-tanh 5.0e-5 -> 2.5e-5 / 6.7e-6 -> 5.8e-6 /
  4.8e-6 -> 5.5e-6; 12x3 2.0e-6 -> 2.0e-6 / 1.8e-6 -> 1.8e-6 / 2.0e-6 -> 1.7e-6; 4x2-test 1.1e-6 -> 1.6e-6 / 1.1e-6 -> 1.5e-6 /
  1.3e-6 -> 7.0e-7; 4x2-train 2.0e-6 -> 2.5e-6 / 1.4e-6 -> 2.3e-6 / 1.3e-6 -> 1.5e-6; 20x7-identity 1.9e-6 -> 2.7e-6 /
  1.6e-6 -> 1.6e-6 / 1.6e-6 -> 1.3e-6; 4x2-reject (adjoint 19 accepted, 1 rejected on both) 4.4e-5 -> 2.9e-5 / 4.3e-5 -> 5.5e-5 /
  2.2e-6 -> 2.4e-6.  f32_split, 8x8 unbiased: 2.4e-6 -> 1.8e-6.  Forward step counts equal the oracle's everywhere; the
  adjoint's equal it or differ by one step in `none` and `unbiased` except at 8x8-test unbiased (17 against 12), and
  differ in `biased` (12x3: 49 against 27, 4x2-reject: 62 against 40), with the same distances: not asserted.
step_reg_grad, error_estimate (scale 3, dt 0.5): 8x8 3.4e-5 -> 3.2e-5, 8x8-test 4.5e-4 -> 8.1e-4, 16x16-tanh 3.2e-5 -> 3.1e-5,
  12x3 4.9e-5 -> 4.5e-5, 20x7-identity 4.6e-5 -> 4.7e-5, 4x2-train 5.3e-5 -> 6.0e-5; stiffness_estimate (scale 2, dt 0.25), same
  order: 1.6e-4 -> 1.4e-4, 1.2e-4 -> 1.1e-4, 1.3e-4 -> 1.4e-4, 1.6e-4 -> 1.5e-4, 8.5e-5 -> 7.6e-5, 1.8e-4 -> 1.7e-4.
The regulariser through the layer (zero cotangent, w_reg = 1; unbiased / biased), stiffness_estimate: 8x8-reg 7.9e-4 -> 7.1e-4 /
  5.4e-4 -> 6.5e-4, 8x8-test-reg 9.7e-5 -> 9.4e-5 / 1.0e-4 -> 8.1e-5, 16x16-tanh-reg 5.8e-4 -> 6.2e-4 / 4.6e-4 -> 3.9e-4,
  4x2-train-reg 6.6e-4 -> 7.7e-4 / 4.3e-4 -> 3.6e-4, f32_split 8x8-reg 7.9e-4 -> 6.0e-4; error_estimate with running statistics
  (8x8-test-reg) 1.7e-3 -> 1.1e-3 / 1.3e-3 -> 1.2e-3.  error_estimate with batch statistics is not held to float64: at the
  automatic initial dt the gradient is rounding noise of the fp32 stages, the oracle is 1.5e-2 .. 8.9e-2 from float64 there and
  this device 1.3e-2 .. 7.9e-2 (tests/test_host_conv_pullback.py says why no case can change that); those rows are held to
  the handle's own step_reg_grad at its own local step, bit for bit, as every other row is too.  dx of a zero cotangent
  is exactly zero everywhere.

Running statistics (lrnde_conv_node_forward kept them across its local step in the head of the step workspace, which is
free only up to the state's size): before they got a buffer of their own, 192 of the 256 statistics changed in test mode
at 4x2 B=1 (64 floats of state) and 128 at 8x2 B=1, the train-mode state at 4x2 B=3 missed the oracle's, and 8x8 passed.

That the tests bite (value-only edits of the host code, not kept): with step 3 of lrnde_conv_node_backward_recorded
skipped, every test of the isolated regulariser, the f32_split test and the recorded-pair test fail while
test_conv_node_backward_matches_oracle[unbiased-2.5] passes; with the bn2 block of launch_vjp's gp scaled by 1.01, all 8
node_backward and all 12 step_reg_grad tests fail, each in block bn2 alone."""
import numpy as np
import pytest
import torch

import conv_geometry_cases as G
import conv_pullback_cases as K

pytestmark = pytest.mark.gpu

RTOL = 1e-5          # f-eval against the oracle, of the output scale (tests/test_gpu_conv.py)
LAYER = [pytest.param(c, id=c.name) for c in K.LAYER_CASES]
REG_LAYER = [pytest.param(c, id=c.name) for c in K.REG_LAYER_CASES]
POINTS = [pytest.param(p, id=p.name) for p in K.STEP_POINTS]


def _handle(case, dtype="f32", inputs=None):
    import lrnde_amd as P
    p, _u, st = (inputs or K.case_inputs(case))[:3]
    h = P.ConvHandle(case.W, case.H, G.C, G.HC, act=case.act, bn_train=case.train, compute_dtype=dtype)
    if st is not None:
        h.set_bn_state(np.array(st))
    h.set_params(np.array(p))     # copies: the shared arrays are read-only
    return h


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()


def _check(what, case, dx, dp, dx_ref, dp_ref, bar, oracle_d):
    """every quantity within its bar of float64; prints `oracle's distance -> this device's / bar`"""
    d = K.distances(None if dx is None else dx.cpu().numpy(), dp.cpu().numpy(), dx_ref, dp_ref)
    print(f"{what}: " + " ".join(f"{k} {oracle_d[k]:.1e}->{v:.1e}/{bar[k]:.1e}" for k, v in d.items()))
    for name, v in d.items():
        where = ""
        if name == "dx":
            err = np.abs(dx.cpu().numpy().astype(np.float64) - np.asarray(dx_ref).reshape(tuple(dx.shape)))
            where = "; " + G.describe(err, case.W, case.H)
        assert np.isfinite(v) and v <= bar[name], f"{what}: {name}: {v:.3e} of its scale from float64 > {bar[name]:.3e}{where}"
    return d


def _backward(h, case, mode, t1, cot, w_reg=0.0, reg_type="error_estimate"):
    _p, u, _st, _w = K.case_inputs(case)
    return h.node_backward(_dev(u), K.T0, K.T2, case.tol, case.tol, cot, mode=mode, reg_type=reg_type, t1_or_rand=t1,
                           w_reg=w_reg, maxiters=K.MAXITERS)


# ---- 1. the solution cotangent alone ----
def _layer_against_rk4(case, dtype, modes):
    _p, _u, _st, w = K.case_inputs(case)
    _ue, dx64, dp64 = K.rk4_pullback64(case)
    h = _handle(case, dtype)
    for mode, t1 in modes:
        bo = K.oracle_layer(case, mode, t1)
        bg = _backward(h, case, mode, t1, _dev(w))
        sf, so = bg["stats_fwd"], bo["stats_fwd"]
        print(f"{case.name} {dtype} {mode} t1={t1:g}: forward {sf['naccept']}/{sf['nreject']}, adjoint "
              f"{bg['stats_bwd']['naccept']}/{bg['stats_bwd']['nreject']} (oracle {bo['stats_bwd']['naccept']}/{bo['stats_bwd']['nreject']})")
        assert (sf["naccept"], sf["nreject"]) == (so["naccept"], so["nreject"])
        bar, d = K.bars(case, mode, None, t1)
        _check(f"{case.name} {dtype} {mode} t1={t1:g}", case, bg["dx"], bg["dp"], dx64, dp64, bar, d)


@pytest.mark.parametrize("case", LAYER)
def test_conv_node_backward_meets_float64(case):
    """w_reg = 0 in the modes none, unbiased (t1 0.41; on the 8x8 row also a stop 1.2e-4 behind the start and 5e-4 before
    the end of the span) and biased: dx and every block of dp within the bars of RK4 in float64; forward step counts are the
    oracle's"""
    _layer_against_rk4(case, "f32", K.layer_modes(case))


# ---- 2. the regulariser's step gradient ----
@pytest.mark.parametrize("reg_type", K.REG_TYPES)
@pytest.mark.parametrize("point", POINTS)
def test_conv_step_reg_grad_meets_float64(point, reg_type):
    """value within 5e-3 relative of float64, every gradient block within the bars"""
    p, u, st, k1, dt = K.point_inputs(point, reg_type)
    h = _handle(point, inputs=(p, u, st))
    g, rv = h.step_reg_grad(_dev(u), _dev(k1), K.STEP_T, dt, K.STEP_TOL, K.STEP_TOL, reg_type=reg_type)
    v64, g64 = K.step_reg64(p, u, k1, K.STEP_T, dt, K.STEP_TOL, K.STEP_TOL, point.W, point.H, point.act, point.train, st, reg_type)
    print(f"{point.name} {reg_type}: reg_val {float(rv):.7g}, float64 {v64:.9g}")
    assert abs(float(rv) - v64) <= 5e-3 * abs(v64)
    bar, d = K.bars(point, reg_type=reg_type)
    _check(f"{point.name} {reg_type} step", point, None, g, None, g64, bar, d)


# ---- 3. the regulariser through the layer, isolated ----
def _local_step(h, case, mode, t1u):
    """(u(t1), k1, dt) of the handle's own local step: the solve's save at t1 (unbiased) or the accepted step t1_used names
    (biased), and init_dt on (t1, 1)"""
    _p, u, _st, _w = K.case_inputs(case)
    if mode == "unbiased":
        sol = h.solve(_dev(u), K.T0, K.T2, case.tol, case.tol, saveat=[t1u, K.T2], maxiters=K.MAXITERS)
        u1 = sol["u"][0].clone()
    else:
        sol = h.solve(_dev(u), K.T0, K.T2, case.tol, case.tol, maxiters=K.MAXITERS)
        idx = [i for i, t in enumerate(sol["t"]) if t == np.float32(t1u)]
        assert len(idx) == 1, (t1u, sol["t"])
        u1 = sol["u"][idx[0]].clone()
    dt, k1 = h.init_dt(u1, t1u, K.T2, case.tol, case.tol)
    return u1, k1, float(dt)


def _regulariser_through_layer(case, dtype, modes, reg_types):
    _p, u, _st, w = K.case_inputs(case)
    h = _handle(case, dtype)
    zero = torch.zeros_like(_dev(w))
    for mode in modes:
        fw = h.node_forward(_dev(u), K.T0, K.T2, case.tol, case.tol, mode=mode, t1_or_rand=K.T1, maxiters=K.MAXITERS)
        t1u = float(fw["t1"])
        u1, k1, dt = _local_step(h, case, mode, t1u)
        for reg_type in reg_types:
            what = f"{case.name} {dtype} {mode} {reg_type} through the layer"
            bg = _backward(h, case, mode, K.T1, zero, w_reg=1.0, reg_type=reg_type)
            assert not torch.any(bg["dx"]), f"{what}: dx of a zero cotangent is not zero"
            # the layer's term is the handle's own step gradient at its own local step (same kernels, fixed-order sums)
            g_own, _rv = h.step_reg_grad(u1, k1, t1u, dt, case.tol, case.tol, reg_type=reg_type)
            assert torch.equal(bg["dp"], g_own), f"{what}: dp differs from step_reg_grad at (u(t1), k1, dt): " + \
                K.fmt(G.block_errors(bg["dp"].cpu().numpy(), g_own.cpu().numpy().astype(np.float64)))
            _v64, g64 = K.reg_layer64(case, t1u, u1.cpu().numpy(), k1.cpu().numpy(), dt, reg_type)
            bar, d = K.bars(case, mode, reg_type)
            if K.reg_layer_pinned(case, reg_type):
                _check(what + f" (t1 {t1u:.4f}, dt {dt:.3g})", case, None, bg["dp"], None, g64, bar, d)
            else:   # error_estimate with batch statistics: rounding noise at the automatic dt, no float64 bar (host test)
                print(f"{what}: not pinned; oracle {K.fmt(d)}; this device {K.fmt(G.block_errors(bg['dp'].cpu().numpy(), g64))}")
            if reg_type == "stiffness_estimate":
                # with a real cotangent: what w_reg adds to dp is w_reg x that gradient
                b0 = _backward(h, case, mode, K.T1, _dev(w), w_reg=0.0, reg_type=reg_type)
                b25 = _backward(h, case, mode, K.T1, _dev(w), w_reg=2.5, reg_type=reg_type)
                assert torch.equal(b0["dx"], b25["dx"])
                diff = (b25["dp"].double() - b0["dp"].double()) / 2.5
                _check(what + ", (dp(2.5) - dp(0)) / 2.5", case, None, diff, None, bg["dp"].cpu().numpy().astype(np.float64), bar, d)
            # error_estimate: the term is 2.5 x 1e-5 .. 1e-3 against a dp of scale 10 .. 100, below the fp32 resolution of dp
            # (6e-8 of its scale per element), so the difference of two pullbacks says nothing about it: not asserted


@pytest.mark.parametrize("case", REG_LAYER)
def test_conv_layer_regulariser_gradient_isolated(case):
    """zero cotangent, w_reg = 1, unbiased and biased, both regulariser types: dx is exactly zero (the oracle's is), dp is
    bit for bit the handle's step_reg_grad at its own u(t1), init_dt k1 and dt, and within the bars of the float64 step at
    that point (stiffness_estimate at every row, error_estimate with running statistics: the host test says why)"""
    _regulariser_through_layer(case, "f32", K.REG_LAYER_MODES, K.REG_TYPES)


# ---- 4. the recorded pair ----
@pytest.mark.parametrize("case", LAYER + REG_LAYER)
def test_conv_recorded_pair_gives_the_bits_of_the_one_call_form(case):
    _p, u, st, w = K.case_inputs(case)
    h = _handle(case)
    ud, wd = _dev(u), _dev(w)
    st0 = h.get_bn_state().clone()
    for mode, t1 in K.layer_modes(case):
        for reg_type in (K.REG_TYPES if mode != "none" else K.REG_TYPES[:1]):
            w_reg = 0.0 if mode == "none" else 2.5
            h.set_bn_state(st0)
            one = _backward(h, case, mode, t1, wd, w_reg=w_reg, reg_type=reg_type)
            h.set_bn_state(st0)
            fw = h.node_forward_record(ud, K.T0, K.T2, case.tol, case.tol, mode=mode, reg_type=reg_type, t1_or_rand=t1,
                                       maxiters=K.MAXITERS)
            two = h.node_backward_recorded(case.B, wd, w_reg=w_reg)
            what = f"{case.name} {mode} t1={t1:g} {reg_type}"
            assert fw["stats"] == one["stats_fwd"], what
            assert torch.equal(two["dx"], one["dx"]), what + ": dx; " + G.describe((two["dx"] - one["dx"]).abs().cpu().numpy(), case.W, case.H)
            assert torch.equal(two["dp"], one["dp"]), what + ": dp " + K.fmt(G.block_errors(two["dp"].cpu().numpy(), one["dp"].cpu().numpy().astype(np.float64)))
            assert two["stats_bwd"] == one["stats_bwd"], what
            if reg_type == "stiffness_estimate":
                # the same record pulled back again without the regulariser: same adjoint, and a dp that lacks the term
                # (the one-call form runs the recorded one, so equal bits alone would not notice a term missing from both)
                bare = h.node_backward_recorded(case.B, wd, w_reg=0.0)
                assert torch.equal(bare["dx"], two["dx"]) and bare["stats_bwd"] == two["stats_bwd"], what
                gap = G.block_errors(two["dp"].cpu().numpy(), bare["dp"].cpu().numpy().astype(np.float64))
                # on the oracle 2.5 x the stiffness gradient is 1e-3 (8x8-test-reg) .. 1 of dp's scale in every block; a
                # missing term leaves exactly 0, fp32 rounding of the sum 6e-8
                assert min(gap.values()) > 1e-5, what +": w_reg = 2.5 leaves dp where w_reg = 0 does: " + K.fmt(gap)


# ---- 5. running statistics around the layer call ----
@pytest.mark.parametrize("W,H,B,train", K.STATS_CASES, ids=[f"{W}x{H}-B{B}-{'train' if tr else 'test'}" for (W, H, B, tr) in K.STATS_CASES])
def test_conv_running_statistics_around_the_layer_call(W, H, B, train):
    """the layer returns the model state as it was when the solve returned: the local step's f-evals leave no trace in it.
    States smaller than the 256 statistics (4x2 at B <= 3, 8x2 at B = 1) and a control above"""
    import oracle as O
    case = K.LayerCase(f"stats-{W}x{H}", W, H, B, "gelu", train, 50 + W + H + B, 1.5, 1e-3)
    p, u, st, w = K.case_inputs(case)
    h = _handle(case)
    ud, wd = _dev(u), _dev(w)
    n = B * G.C * H * W
    if not train:
        set_to = torch.from_numpy(np.array(st)).cuda()
        f_ref = K._field(case, p, st).rhs(u.reshape(B, -1), 0.3).reshape(u.shape)
        before = h.rhs(ud, 0.3)
        assert float((before.cpu() - torch.from_numpy(f_ref)).abs().max()) <= RTOL * float(np.abs(f_ref).max())
        calls = [("node_forward unbiased", lambda: h.node_forward(ud, K.T0, K.T2, case.tol, case.tol, mode="unbiased", t1_or_rand=K.T1)),
                 ("node_forward biased", lambda: h.node_forward(ud, K.T0, K.T2, case.tol, case.tol, mode="biased", t1_or_rand=K.T1)),
                 ("node_backward", lambda: _backward(h, case, "unbiased", K.T1, wd, w_reg=2.5))]
        for name, call in calls:
            call()
            got = h.get_bn_state()
            bad = int((got != set_to).sum())
            assert bad == 0, f"{W}x{H} B={B} (state of {n} floats) after {name}: {bad} of 256 running statistics changed in test mode"
            after = h.rhs(ud, 0.3)
            assert torch.equal(after, before), f"after {name}: " + G.describe((after - before).abs().cpu().numpy(), W, H)
    else:
        for mode in ("unbiased", "biased"):
            hh = _handle(case)
            fld = K._field(case, p, st)
            rg = hh.node_forward(ud, K.T0, K.T2, case.tol, case.tol, mode=mode, t1_or_rand=K.T1)
            # the oracle's statistics when its solve returns (its node_forward rewinds the local step too: checked here by
            # running the solve alone)
            ro = O.solve(fld, u.reshape(B, -1), K.T0, K.T2, case.tol, case.tol, saveat=[K.T1, K.T2] if mode == "unbiased" else ())
            assert rg["stats"]["nf"] == ro["stats"]["nf"]
            got = hh.get_bn_state().cpu().numpy()
            err = np.abs(got - fld.bn_run)
            print(f"{W}x{H} B={B} train {mode}: running statistics max |diff| {err.max():.2e}")
            np.testing.assert_allclose(got, fld.bn_run, rtol=5e-3, atol=5e-4,
                                       err_msg=f"{W}x{H} B={B} (state of {n} floats) after node_forward {mode}")


# ---- 6. compute_dtype = f32_split ----
def test_conv_f32_split_pullback_meets_float64():
    """the 8x8 rows with conv2 / conv3 on the fp16 MFMA pipe (hi + lo operand pairs): unbiased with w_reg = 0, and the
    zero-cotangent stiffness gradient, at the bars of the fp32 handle"""
    _layer_against_rk4(K.CASE["8x8"], "f32_split", [("unbiased", K.T1)])
    _regulariser_through_layer(K.CASE["8x8-reg"], "f32_split", ["unbiased"], ["stiffness_estimate"])

# 7. bf16 is not here: its backward is the fp32 adjoint over a bf16 trajectory (test_conv_bf16_handle_backward_is_the_fp32_adjoint),
# and no float64 bar can be derived for that.
