"""schedulers (experiments/src/utils.jl:1-68) on the host, update rules (experiments/src/construct.jl:104-126)
on the device against a numpy float64 restatement of the Optimisers.jl formulas."""
import math

import numpy as np
import pytest


def test_schedulers_follow_the_reference_formulas():
    import lrnde_amd as P
    e = P.ExponentialDecay(1e-2, 1e-4, 1000)
    assert math.isclose(e(0), 1e-2) and math.isclose(e(1000), 1e-4, rel_tol=1e-12) and math.isclose(e(500), 1e-3, rel_tol=1e-12)
    assert math.isclose(P.InverseDecay(0.1, 0.5)(4), 0.1 / 3)
    s = P.Step(0.1, 0.5, [3, 6])                      # lr0 * gamma^(searchsortedfirst(steps, t-1) - 1)
    assert [s(t) for t in (1, 4, 5, 7, 8)] == [0.1, 0.1, 0.05, 0.05, 0.025]
    assert P.Step(0.1, 0.1, 5)(7) == pytest.approx(0.01)
    c = P.CosineAnneal(0.1, 0.001, 10, restart=True, dampen=1.2)
    assert c(1) == pytest.approx(0.1) and c(11) == pytest.approx(0.1 / 1.2) and c(6) == pytest.approx((0.099 * (1 + math.cos(math.pi * 0.5)) / 2 + 0.001))
    c2 = P.CosineAnneal(0.1, 0.001, 10)
    assert c2(11) == pytest.approx(0.001)
    assert P.Constant(3e-4)(99) == 3e-4
    sch = P.construct_scheduler("exponential", 1e-3, total_steps=100, exponential_lr_div_factor=10.0)
    assert math.isclose(sch(100), 1e-4, rel_tol=1e-12)
    with pytest.raises(ValueError, match="unknown value for `scheduler`"):
        P.construct_scheduler("linear", 1e-3)
    with pytest.raises(ValueError, match="unknown value for `optimizer`"):
        P.Optimiser("rmsprop")


def _ref_update(kind, x, g, s1, s2, eta, rho, b1, b2, eps, t, wd):
    x, g = x.astype(np.float64), g.astype(np.float64)
    if kind == "sgd":
        d = eta * g
    elif kind == "momentum":
        s1[:] = rho * s1 - eta * g; d = -s1
    elif kind == "nesterov":
        d = -rho * rho * s1 + (1 + rho) * eta * g; s1[:] = rho * s1 - eta * g
    elif kind == "adam":
        s1[:] = b1 * s1 + (1 - b1) * g; s2[:] = b2 * s2 + (1 - b2) * g * g
        d = s1 / (1 - b1 ** t) / (np.sqrt(s2 / (1 - b2 ** t)) + eps) * eta
    else:
        s1[:] = b1 * s1 + (1 - b1) * g; s2[:] = np.maximum(b2 * s2, np.abs(g))
        d = eta / (1 - b1 ** t) * s1 / (s2 + eps)
    return x - (d + wd * x)


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", [("sgd", {}), ("momentum", dict(momentum=0.9)), ("nesterov", dict(momentum=0.9, nesterov=True)),
                                     ("adam", {}), ("adam", dict(weight_decay=1e-2)), ("adamax", {})])
def test_update_rules_match_float64_restatement(gpu_pkg, name, kw):
    import torch
    P = gpu_pkg
    n = 158568
    rng = np.random.default_rng(0)
    x = rng.standard_normal(n).astype(np.float32)
    opt = P.Optimiser("sgd" if name in ("sgd", "momentum", "nesterov") else name, learning_rate=1e-2, **kw)
    xd = torch.from_numpy(x.copy()).cuda()
    xr = x.astype(np.float64)
    s1, s2 = np.zeros(n), np.zeros(n)
    sched = P.CosineAnneal(1e-2, 1e-4, 5, restart=True)
    for t in range(1, 8):
        g = rng.standard_normal(n).astype(np.float32)
        lr = sched(t)
        opt.update(xd, torch.from_numpy(g).cuda(), lr=lr)
        xr = _ref_update(name, xr, g, s1, s2, lr, kw.get("momentum", 0.0), 0.9, 0.999, 1e-8, t, kw.get("weight_decay", 0.0))
    err = np.abs(xd.cpu().numpy() - xr).max() / np.abs(xr).max()
    assert err < 1e-6, err


# ---- one step at a time, from the device's own state ----
RULES = [("sgd", {}), ("momentum", dict(momentum=0.9)), ("nesterov", dict(momentum=0.9, nesterov=True)),
         ("adam", {}), ("adam", dict(weight_decay=1e-2)), ("adamax", {})]
# the launch is capped at 2048 workgroups of 256 threads and strides: 524 288 is the last size without a second trip,
# 524 291 = 2048*256 + 3 a first strided trip with three elements, 1 200 000 two or three trips for every thread
SIZES = (1, 255, 257, 524288, 524291, 1200000)
LR = 1e-2


def _step(name, x, g, s1, s2, eta, rho, b1, b2, eps, t, wd, dt):
    """one update in the arithmetic `dt` from the float32 state (x, s1, s2): the formulas of _ref_update with the scalars first
    rounded to float32, as the ABI takes them.  Returns (x_new, s1_new, s2_new)."""
    eta, rho, b1, b2, eps, wd, one, tt = (dt(np.float32(v)) for v in (eta, rho, b1, b2, eps, wd, 1.0, t))
    x, g = x.astype(dt), g.astype(dt)
    s1 = None if s1 is None else s1.astype(dt)
    s2 = None if s2 is None else s2.astype(dt)
    if name == "sgd":
        d = eta * g
    elif name == "momentum":
        s1 = rho * s1 - eta * g; d = -s1
    elif name == "nesterov":
        d = -rho * rho * s1 + (one + rho) * eta * g; s1 = rho * s1 - eta * g
    elif name == "adam":
        s1 = b1 * s1 + (one - b1) * g; s2 = b2 * s2 + (one - b2) * g * g
        d = s1 / (one - b1 ** tt) / (np.sqrt(s2 / (one - b2 ** tt)) + eps) * eta
    else:
        s1 = b1 * s1 + (one - b1) * g; s2 = np.maximum(b2 * s2, np.abs(g))
        d = eta / (one - b1 ** tt) * s1 / (s2 + eps)
    x_new = x - (d + wd * x)
    assert x_new.dtype == dt and (s1 is None or s1.dtype == dt) and (s2 is None or s2.dtype == dt)
    return x_new, s1, s2


def _rel(a, ref):
    n = np.linalg.norm(ref)
    return float(np.linalg.norm(a - ref) / n) if n > 0 else float(np.linalg.norm(a))


def _optimiser(P, name, kw):
    return P.Optimiser("sgd" if name in ("sgd", "momentum", "nesterov") else name, learning_rate=LR, **kw)


def _state(opt, i=0):
    return tuple(None if s is None else s.cpu().numpy() for s in opt._state.get(i, (None, None)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name,kw", RULES)
def test_every_step_and_both_moments_match_float64_from_the_device_state(gpu_pkg, name, kw, n):
    """Three steps; each is compared with a float64 restatement that starts from the device's float32 state before that step,
    so nothing accumulates: the update x_new - x_old (formed in float64 from the two float32 arrays), s1 and s2, each within
    max(1e-5, 4 x the distance of a float32 numpy run of the same formulas), relative to the float64 array's norm.  |x| is 0.1:
    at |x| ~ 1 the rounding of x itself is 2.5e-6 to 6e-6 of an update of size lr = 1e-2.

    Measured on an MI355X, worst over the six sizes and three steps, beside the bound (the float32 numpy run is that close
    to float64 too: the kernel's error is the arithmetic's, with or without strided trips):
        update  sgd 5.1e-07, momentum 2.6e-07, nesterov 1.9e-07, adamax 6.6e-07 (bound 1e-05);
                adam 3.7e-06 (bound 1.5e-05), adam + weight decay 3.8e-06 (bound 1.5e-05) -- 1 - b2^t in float32
        s1      <= 4.0e-08, s2 <= 4.6e-08 (bound 1e-05)"""
    import torch
    P = gpu_pkg
    rng = np.random.default_rng([7, n])
    x0 = (0.1 * rng.standard_normal(n)).astype(np.float32)
    opt = _optimiser(P, name, kw)
    xd = torch.from_numpy(x0.copy()).cuda()
    rho, wd = kw.get("momentum", 0.0), kw.get("weight_decay", 0.0)
    zeros = lambda have: np.zeros(n, np.float32) if have else None
    worst = {}
    for t in (1, 2, 3):
        g = rng.standard_normal(n).astype(np.float32)
        x_old = xd.cpu().numpy()
        s1_old, s2_old = _state(opt) if t > 1 else (zeros(name != "sgd"), zeros(name in ("adam", "adamax")))
        opt.update(xd, torch.from_numpy(g).cuda(), lr=LR)
        x_new = xd.cpu().numpy()
        s1_new, s2_new = _state(opt)
        r64 = _step(name, x_old, g, s1_old, s2_old, LR, rho, 0.9, 0.999, 1e-8, t, wd, np.float64)
        r32 = _step(name, x_old, g, s1_old, s2_old, LR, rho, 0.9, 0.999, 1e-8, t, wd, np.float32)
        xo = x_old.astype(np.float64)
        rows = [("update", x_new.astype(np.float64) - xo, r32[0].astype(np.float64) - xo, r64[0] - xo)]
        assert (s1_new is None) == (r64[1] is None) and (s2_new is None) == (r64[2] is None)
        if s1_new is not None:
            rows.append(("s1", s1_new.astype(np.float64), r32[1].astype(np.float64), r64[1]))
        if s2_new is not None:
            rows.append(("s2", s2_new.astype(np.float64), r32[2].astype(np.float64), r64[2]))
        for what, got, f32, f64 in rows:
            assert got.shape == f64.shape == (n,) and np.linalg.norm(f64) > 0
            e, d32 = _rel(got, f64), _rel(f32, f64)
            bnd = max(1e-5, 4.0 * d32)
            print(f"{name} {kw} n={n} step {t} {what}: gpu {e:.2e} numpy-f32 {d32:.2e} bound {bnd:.2e}")
            worst[what] = max(worst.get(what, 0.0), e / bnd)
            assert e <= bnd, (what, t, e, bnd)


@pytest.mark.gpu
def test_a_list_of_vectors_updates_each_as_its_own_run(gpu_pkg):
    """Optimiser.update([p0, p1], [g0, g1]) keys the state by the position in the list: each vector, its s1 and its s2 end with
    the bits of an optimiser that only ever saw that vector"""
    import torch
    P = gpu_pkg
    sizes = (1000, 524291)
    rng = np.random.default_rng(11)
    xs = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in sizes]
    gs = [[rng.standard_normal(n).astype(np.float32) for n in sizes] for _ in range(3)]
    kw = dict(weight_decay=1e-2)
    both = _optimiser(P, "adam", kw)
    pd = [torch.from_numpy(x.copy()).cuda() for x in xs]
    for g in gs:
        both.update(pd, [torch.from_numpy(a).cuda() for a in g], lr=LR)
    for i in range(2):
        alone = _optimiser(P, "adam", kw)
        p = torch.from_numpy(xs[i].copy()).cuda()
        for g in gs:
            alone.update(p, torch.from_numpy(g[i]).cuda(), lr=LR)
        assert torch.equal(p, pd[i]) and not torch.equal(p.cpu(), torch.from_numpy(xs[i]))
        for a, b in zip(_state(alone), _state(both, i)):
            assert a.shape == (sizes[i],) and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["adam", "adamax"])
def test_a_zero_gradient_from_zero_state_changes_nothing(gpu_pkg, name):
    """0 / (sqrt(0) + eps) = 0: x keeps its bits (no weight decay) and both moments stay exactly zero, strided trips included"""
    import torch
    P = gpu_pkg
    n = 524291
    x0 = (0.1 * np.random.default_rng(13).standard_normal(n)).astype(np.float32)
    opt = _optimiser(P, name, {})
    xd = torch.from_numpy(x0.copy()).cuda()
    g = torch.zeros(n, dtype=torch.float32, device="cuda")
    for _ in range(3):
        opt.update(xd, g, lr=LR)
        assert np.array_equal(xd.cpu().numpy().view(np.uint32), x0.view(np.uint32))
        s1, s2 = _state(opt)
        assert s1.shape == s2.shape == (n,) and not s1.any() and not s2.any()
