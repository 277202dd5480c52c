"""Host side of the conv layer pullback's float64 pin (tests/conv_pullback_cases.py): no GPU needed.  It checks that the
yardstick is sound and that the conditions tests/test_gpu_conv_pullback.py relies on hold at every case:

  * classical RK4 in float64 at 32 steps against 64 steps moves no quantity (dx, each parameter block of dp) by more than
    1e-6 of its scale (the rejection row, whose trajectory grows: 64 against 128);
  * the float64 Tsit5 step's regulariser value agrees with the oracle's to 1e-4 relative at every regulariser point;
  * a condition, not a measurement: every distance of the fp32 oracle from float64 that a GPU bar is built on is at most
    2.5e-3, so no bar exceeds 1e-2 (a wider one would let a dropped strip or term of a small block through).  A case that
    misses the cap is replaced, not waived;
  * every layer case takes at least 3 accepted steps forward, `biased` saves at least 2, the rejection row's adjoint
    rejects a step, every regulariser point has EEst > 1e-2.

The distances are printed (pytest -s): oracle to float64 here, MI355X to float64 in the GPU test.

Where the cap cannot hold: the `error_estimate` gradient of the layer's local step in train mode.  The step runs at the
automatic initial dt, where utilde = dt * sum(btilde_j k_j) is rounding noise of the fp32 stages (sum btilde = 0), and
batch statistics make the field's time scale follow the weight scale, so no weight scale moves dt out of that regime: the
oracle's gradient is 9e-2 (8x8), 5e-2 (16x16) and 4e-2 (4x2) from float64 at scale 3, tol 1e-2, and still 2.8e-3 at tol 1.
test_error_estimate_layer_gradient_in_train_mode_is_not_conditioned records that; the GPU test holds those cases to the
handle's own step_reg_grad bit for bit instead, and step_reg_grad to float64 at the conditioned points."""
import numpy as np
import pytest

import conv_pullback_cases as K

LAYER = [pytest.param(c, id=c.name) for c in K.LAYER_CASES]
REG_LAYER = [pytest.param(c, id=c.name) for c in K.REG_LAYER_CASES]
POINTS = [pytest.param(p, id=p.name) for p in K.STEP_POINTS]


def _capped(what, d):
    print(f"{what}: oracle to float64 {K.fmt(d)}")
    for name, v in d.items():
        assert np.isfinite(v) and v <= K.CAP, f"{what}: {name} is {v:.2e} from float64, above the cap {K.CAP:g}: replace the case"


@pytest.mark.parametrize("case", LAYER)
def test_rk4_yardstick_has_converged(case):
    _u32, dx32, dp32 = K.rk4_pullback64(case)
    u64, dx64, dp64 = K.rk4_pullback64(case, 2 * case.nsteps)
    d = K.distances(dx32, dp32, dx64, dp64)
    print(f"{case.name}: RK4 {case.nsteps} against {2 * case.nsteps} steps {K.fmt(d)}")
    assert all(v <= 1e-6 for v in d.values()), d
    assert case.nsteps == 32 or case.name == K.REJECT_CASE
    assert dx32.dtype == np.float64 and not dx32.flags.writeable and not dp32.flags.writeable
    assert K.rk4_pullback64(case)[2] is dp32              # computed once per case


@pytest.mark.parametrize("case", LAYER)
def test_oracle_layer_pullback_is_conditioned(case):
    import oracle as O
    p, u, st, _w = K.case_inputs(case)
    for mode, t1 in K.layer_modes(case):
        bo = K.oracle_layer(case, mode, t1)
        sf, sb = bo["stats_fwd"], bo["stats_bwd"]
        print(f"{case.name} {mode} t1={t1:g}: forward {sf['naccept']}/{sf['nreject']}, adjoint {sb['naccept']}/{sb['nreject']}")
        assert sf["naccept"] >= 3
        _capped(f"{case.name} {mode} t1={t1:g}", K.oracle_distance(case, mode, None, t1))
        if mode == "biased":
            sol = O.solve(K._field(case, p, st), u.reshape(case.B, -1), K.T0, K.T2, case.tol, case.tol, maxiters=K.MAXITERS)
            assert sol["stats"]["nsaved"] >= 2
        if case.name == K.REJECT_CASE and mode == "none":
            assert sb["nreject"] >= 1


def test_the_case_table_is_the_one_asked_for():
    names = {c.name: c for c in K.LAYER_CASES}
    assert any(c.W * c.H * c.B * 8 < 256 and not c.train and c.B == 1 for c in K.LAYER_CASES)     # n < 256, test mode
    assert any(c.W * c.H * c.B * 8 < 256 and c.train for c in K.LAYER_CASES)                       # n < 256, train mode
    c = names["20x7-identity"]
    TR, TP, _MT, strips = K.G.geometry(c.W, c.H)
    assert TR == 1 and strips == 7 and TP % 16 != 0 and c.act == "identity"
    assert K.REJECT_CASE in names
    assert {(p.W, p.H, p.B, p.train) for p in K.STEP_POINTS} == {(8, 8, 3, True), (8, 8, 3, False), (16, 16, 2, True),
                                                                   (12, 3, 2, True), (20, 7, 3, True), (4, 2, 3, True)}
    assert K.STEP_AT == {"error_estimate": (3.0, 0.5), "stiffness_estimate": (2.0, 0.25)}
    assert {(c.W, c.H, c.train) for c in K.REG_LAYER_CASES} == {(8, 8, True), (8, 8, False), (16, 16, True), (4, 2, True)}
    for (W, H, B, _train) in K.STATS_CASES[:3]:
        assert W * H * B * 8 < 256 and K.G.legal(W, H)
    assert all(W * H * B * 8 >= 256 for (W, H, B, _t) in K.STATS_CASES[3:])


@pytest.mark.parametrize("reg_type", K.REG_TYPES)
@pytest.mark.parametrize("point", POINTS)
def test_oracle_step_reg_grad_is_conditioned(point, reg_type):
    import oracle as O
    p, u, st, k1, dt = K.point_inputs(point, reg_type)
    B = point.B
    fld = K._field(point, p, st)
    so = O.tsit5_step(fld, u.reshape(B, -1), k1.reshape(B, -1), K.STEP_T, dt, K.STEP_TOL, K.STEP_TOL)
    assert float(so["eest"]) > 1e-2
    _g, rv = O.step_reg_grad(fld, u.reshape(B, -1), k1.reshape(B, -1), K.STEP_T, dt, K.STEP_TOL, K.STEP_TOL, reg_type=reg_type)
    v64, _g64 = K.step_reg64(p, u, k1, K.STEP_T, dt, K.STEP_TOL, K.STEP_TOL, point.W, point.H, point.act, point.train, st, reg_type)
    print(f"{point.name} {reg_type}: EEst {float(so['eest']):.3g}, reg_val oracle {float(rv):.7g} float64 {v64:.9g}")
    assert abs(float(rv) - v64) <= 1e-4 * abs(v64)
    _capped(f"{point.name} {reg_type} step", K.oracle_distance(point, reg_type=reg_type))


@pytest.mark.parametrize("case", REG_LAYER)
def test_oracle_layer_regulariser_is_conditioned(case):
    """zero cotangent, w_reg = 1: dx is exactly zero, dp is the local step's gradient; held to the cap wherever the GPU
    test builds a bar on it (K.reg_layer_pinned)"""
    for mode in K.REG_LAYER_MODES:
        t1u, _u1, _k1, dt, fwd = K.oracle_local_step(case, mode)
        assert fwd["stats"]["naccept"] >= 3 and fwd["retcode"] == 0
        for reg_type in K.REG_TYPES:
            bo = K.oracle_layer(case, mode, K.T1, reg_type)
            assert not np.any(bo["dx"])
            d = K.oracle_distance(case, mode, reg_type)
            what = f"{case.name} {mode} {reg_type} through the layer (t1 {t1u:.4f}, dt {dt:.3g}, scale {np.abs(bo['dp']).max():.2e})"
            if K.reg_layer_pinned(case, reg_type):
                _capped(what, d)
            else:
                print(f"{what}: oracle to float64 {K.fmt(d)} (not conditioned, no bar)")


def test_error_estimate_layer_gradient_in_train_mode_is_not_conditioned():
    """the reason K.reg_layer_pinned leaves these out: at the automatic initial dt the oracle itself is percents away from
    float64, at any weight scale; if this ever fails, the cases can be pinned and reg_layer_pinned should say so"""
    worst = {}
    for case in K.REG_LAYER_CASES:
        if not K.reg_layer_pinned(case, "error_estimate"):
            worst[case.name] = max(max(K.oracle_distance(case, mode, "error_estimate").values()) for mode in K.REG_LAYER_MODES)
    print("error_estimate through the layer, train mode, worst quantity: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert worst and all(v > K.CAP for v in worst.values()), worst
