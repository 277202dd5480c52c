"""The small Dense-chain vector field (lrnde_create_chain, csrc/lrnde_chain.hpp; NeuralODE(field="dense_chain")):
the PhysioNet latent ODE's gen_dynamics (experiments/src/construct.jl:236-244) and other Chain / TDChain shapes.

References: float64 restatements written here (a numpy field rounded once to float32, np_restatement's generic Tsit5
step / solve over it) and float64 torch autograd through a fine RK4 integration for the gradients — no code shared with
the kernels.  Tolerances as tests/test_gpu_independent_parity.py and tests/test_gpu_timeseries_pullback.py state them:
1e-5 scale-relative on f-evals, steps and solutions; 3e-4 of each gradient's norm for pullbacks; accepted / rejected
counts equal only where the error estimate is truncation, not rounding (weights x3 / x6)."""
import numpy as np
import pytest
import torch

import np_restatement as R

pytestmark = pytest.mark.gpu

ACT64 = {"identity": lambda z: z, "tanh": np.tanh,
         "gelu": lambda z: z / (1.0 + np.exp(-1.5957691216057308 * z * (1.0 + 0.044715 * z * z)))}
ACT_T = {"identity": lambda z: z, "tanh": torch.tanh,
         "gelu": lambda z: z * torch.sigmoid(1.5957691216057308 * z * (1.0 + 0.044715 * z * z))}


def physionet(P, latent=20, hidden=40):
    """gen_dynamics: Chain(tanh.(u), 8 Dense layers alternating latent <-> hidden, all tanh) — construct.jl:236-244"""
    ls = [P.Dense(latent, hidden, "tanh") if i % 2 == 0 else P.Dense(hidden, latent, "tanh") for i in range(8)]
    return P.Chain(P.Activation("tanh"), *ls)


def spec(model):
    """(td, input activation, [(in, out, act)]) of a chain model"""
    from localregneuralde_jl_amd.layers import Activation, TDChain
    td = isinstance(model, TDChain)
    ia = model.layers[0].activation if isinstance(model.layers[0], Activation) else "identity"
    return td, ia, [(l.in_dims - int(td), l.out_dims, l.activation) for l in model.layers if not isinstance(l, Activation)]


def unflatten(p, sp):
    td, _, ls = sp
    out, o = [], 0
    for i, n, _a in ls:
        W = np.asarray(p[o:o + n * (i + td)], np.float64).reshape(i + td, n).T
        o += n * (i + td)
        out.append((W, np.asarray(p[o:o + n], np.float64)))
        o += n
    assert o == len(p)
    return out


class Chain64:
    """the field in float64, rounded once to float32 (np_restatement's field convention)"""

    def __init__(self, model, p):
        self.sp = spec(model)
        self.Wb = unflatten(p, self.sp)

    def f64(self, x, t):
        td, ia, ls = self.sp
        h = ACT64[ia](np.asarray(x, np.float64))
        for (W, b), (_i, _o, a) in zip(self.Wb, ls):
            z = h @ W[:, :W.shape[1] - td].T + b
            if td:
                z = z + float(t) * W[:, -1]
            h = ACT64[a](z)
        return h

    def __call__(self, x, t):
        return self.f64(x, t).astype(np.float32)


class Chain32(Chain64):
    """the same field in float32 arithmetic (numpy BLAS): a second summation order, to size rounding amplification"""

    def __call__(self, x, t):
        td, ia, ls = self.sp
        h = ACT64[ia](np.asarray(x, np.float32)).astype(np.float32)
        for (W, b), (_i, _o, a) in zip(self.Wb, ls):
            W32, b32 = W.astype(np.float32), b.astype(np.float32)
            z = h @ W32[:, :W32.shape[1] - td].T + b32
            if td:
                z = z + np.float32(t) * W32[:, -1]
            h = ACT64[a](z).astype(np.float32)
        return h


def torch_field(model, pt):
    td, ia, ls = spec(model)
    Wb, o = [], 0
    for i, n, _a in ls:
        W = pt[o:o + n * (i + td)].reshape(i + td, n).T
        o += n * (i + td)
        Wb.append((W, pt[o:o + n]))
        o += n

    def f(u, t):
        h = ACT_T[ia](u)
        for (W, b), (i, _n, a) in zip(Wb, ls):
            z = h @ W[:, :i].T + b
            if td:
                z = z + t * W[:, i]
            h = ACT_T[a](z)
        return h
    return f


def err(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def mk_inputs(P, model, B, scale=1.0, seed=0, noise=0.01):
    """(p, x) of mk, without a handle (the CPU tests of the restatement use the same inputs)"""
    p = P.glorot_chain_params(model, seed=seed, scale=scale)
    p = (p + np.random.default_rng(seed + 1).standard_normal(p.size).astype(np.float32) * np.float32(noise)).astype(np.float32)
    x = (np.random.default_rng(seed + 2).random((B, spec(model)[2][0][0]), dtype=np.float32) - np.float32(0.5)) * np.float32(2)
    return p, x


def mk(P, model, B, scale=1.0, seed=0, noise=0.01):
    from localregneuralde_jl_amd.layers import Handle, _chain_desc
    p, x = mk_inputs(P, model, B, scale, seed, noise)
    h = Handle(_chain_desc(model))
    h.set_params(torch.from_numpy(p))
    return h, p, x


def shapes(P):
    td3 = lambda act: P.TDChain(P.Chain(P.Dense(33, 64, act), P.Dense(65, 64, act), P.Dense(65, 32)))
    return {
        "physionet": physionet(P),
        "td3_tanh": td3("tanh"),
        "td3_gelu": td3("gelu"),
        "one_layer": P.Chain(P.Dense(8, 8, "tanh")),
        "sixteen": P.Chain(P.Activation("gelu"), *[P.Dense(24, 24, "tanh") for _ in range(16)]),
        "w128_td": P.TDChain(P.Chain(P.Dense(129, 128, "tanh"))),
        "w128_64_td": P.TDChain(P.Chain(P.Dense(129, 64, "gelu"), P.Dense(65, 128))),
        # odd widths: the second row of chain_layer's float2 pair is k_pack_chain's zero padding; D = 1
        "odd_21_37": P.Chain(P.Activation("tanh"), P.Dense(21, 37, "tanh"), P.Dense(37, 21, "tanh")),
        "odd_td_127_33": P.TDChain(P.Chain(P.Dense(128, 33, "tanh"), P.Dense(34, 127))),
        "width_1": P.Chain(P.Dense(1, 5, "tanh"), P.Dense(5, 1)),
    }


ODD = ("odd_21_37", "odd_td_127_33", "width_1")


@pytest.mark.parametrize("name,B", [("physionet", 1), ("physionet", 37), ("physionet", 512), ("td3_tanh", 19), ("td3_gelu", 19),
                                    ("one_layer", 5), ("sixteen", 9), ("w128_td", 11), ("w128_64_td", 13),
                                    ("odd_21_37", 9), ("odd_td_127_33", 11), ("width_1", 7), ("width_1", 1)])
def test_rhs_and_vjp_vs_float64(gpu_pkg, name, B):
    P = gpu_pkg
    model = shapes(P)[name]
    h, p, x = mk(P, model, B)
    f = Chain64(model, p)
    xd = torch.from_numpy(x).cuda()
    for t in (0.0, 0.37):
        e = err(h.rhs(xd, t).cpu().numpy(), f.f64(x, t))
        assert e <= 1e-5, (name, "rhs", t, e)
    lam = np.random.default_rng(7).standard_normal(x.shape).astype(np.float32)
    t = 0.61
    dy, gp = h.vjp(xd, t, torch.from_numpy(lam).cuda())
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    ut = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    (torch_field(model, pt)(ut, t) * torch.tensor(lam, dtype=torch.float64)).sum().backward()
    assert err(dy.cpu().numpy(), ut.grad.numpy()) <= 1e-5, (name, "dy", err(dy.cpu().numpy(), ut.grad.numpy()))
    assert err(gp.cpu().numpy(), pt.grad.numpy()) <= 1e-5, (name, "gp", err(gp.cpu().numpy(), pt.grad.numpy()))


@pytest.mark.parametrize("name", ("physionet",) + ODD)
def test_columns_are_independent_and_runs_repeat_bitwise(gpu_pkg, name):
    P = gpu_pkg
    model = shapes(P)[name]
    h, p, x = mk(P, model, 512)
    xd = torch.from_numpy(x).cuda()
    k1 = torch.from_numpy(Chain64(model, p)(x, 0.2)).cuda()
    full = h.rhs(xd, 0.3)
    stp = h.perform_step(xd, k1, 0.2, 0.05, 1e-6, 1e-6)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(512)).cuda()
    assert torch.equal(h.rhs(xd[perm].contiguous(), 0.3), full[perm])
    sp = h.perform_step(xd[perm].contiguous(), k1[perm].contiguous(), 0.2, 0.05, 1e-6, 1e-6)
    assert torch.equal(sp["u"], stp["u"][perm]) and torch.equal(sp["k7"], stp["k7"][perm])
    for c in (0, 7, 8, 200, 511):
        xc, kc = xd[c:c + 1].contiguous(), k1[c:c + 1].contiguous()
        assert torch.equal(h.rhs(xc, 0.3)[0], full[c])
        s1 = h.perform_step(xc, kc, 0.2, 0.05, 1e-6, 1e-6)
        assert torch.equal(s1["u"][0], stp["u"][c]) and torch.equal(s1["k7"][0], stp["k7"][c])
    # forward + pullback twice: identical bits, parameter gradients included
    node = P.NeuralODE(model, regularize="unbiased", abstol=1e-6, reltol=1e-6, saveat=[0.25, 0.5, 1.0], save_start=False,
                       field="dense_chain")
    st = node.initialstates(np.random.default_rng(1))
    ps = torch.from_numpy(p).cuda()
    cots = torch.from_numpy(np.random.default_rng(4).standard_normal((3, 512, x.shape[1])).astype(np.float32)).cuda()
    runs = [node.pullback(xd, ps, st, cots, w_reg=2.0) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2]["sol_u"], runs[1][2]["sol_u"])


@pytest.mark.parametrize("name,scale", [("physionet", 1.0), ("physionet", 3.0), ("td3_tanh", 1.0), ("td3_tanh", 3.0),
                                        ("td3_gelu", 3.0), ("sixteen", 1.0), ("odd_21_37", 1.0), ("odd_td_127_33", 1.0),
                                        ("odd_td_127_33", 3.0), ("width_1", 1.0)])
def test_perform_step_vs_float64(gpu_pkg, name, scale):
    P = gpu_pkg
    model = shapes(P)[name]
    h, p, x = mk(P, model, 33, scale=scale)
    f = Chain64(model, p)
    k1 = f(x, 0.1)
    ref = R.tsit5_step(f, x, k1, 0.1, 0.05, 1e-4, 1e-4)
    got = h.perform_step(torch.from_numpy(x).cuda(), torch.from_numpy(k1).cuda(), 0.1, 0.05, 1e-4, 1e-4)
    # a deep chain at weights x3 amplifies fp32 rounding through its layers: the bar is 1e-5, or what a second fp32
    # summation order of the same field (numpy BLAS) lands at, with a margin
    r32 = R.tsit5_step(Chain32(model, p), x, k1, 0.1, 0.05, 1e-4, 1e-4)
    for key in ("u", "k7"):
        bar = max(1e-5, 4.0 * err(r32[key], ref[key]))
        assert err(got[key].cpu().numpy(), ref[key]) <= bar, (key, err(got[key].cpu().numpy(), ref[key]), bar)
    # EEst / stiffness: at weights x3 the estimate is truncation and agrees to 2 %; at the glorot scale it is fp32 rounding
    # noise of the stage values (test_gpu_independent_parity.py docstring): finite and positive only
    print(f"{name} x{scale}: EEst gpu {got['eest']:.6g} ref {ref['eest']:.6g}; stiffness gpu {got['reg_stiff']:.6g} "
          f"ref {ref['reg_stiff']:.6g}")
    assert np.isfinite(got["eest"]) and got["eest"] > 0 and np.isfinite(got["reg_stiff"]) and got["reg_stiff"] >= 0
    if scale >= 3.0:
        for key in ("eest", "reg_stiff"):
            bar = max(2e-2 * float(ref[key]), 4.0 * abs(float(r32[key]) - float(ref[key])))
            assert abs(float(got[key]) - float(ref[key])) <= bar, (key, float(got[key]), float(ref[key]), float(r32[key]))
    dt_ref, f0 = R.init_dt(f, x, 0.0, 1.0, 1e-4, 1e-4)
    dt, k1g = h.init_dt(torch.from_numpy(x).cuda(), 0.0, 1.0, 1e-4, 1e-4)
    assert abs(float(dt) - float(dt_ref)) <= 1e-4 * float(dt_ref)
    assert err(k1g.cpu().numpy(), f0) <= 1e-5


@pytest.mark.parametrize("scale,tol", [(3.0, 1e-4), (3.0, 1e-5), (6.0, 1e-4), (6.0, 1e-5)])
def test_solve_counts_equal_where_truncation_dominates(gpu_pkg, scale, tol):
    P = gpu_pkg
    model = shapes(P)["td3_tanh"]
    h, p, x = mk(P, model, 64, scale=scale)
    got = h.solve(torch.from_numpy(x).cuda(), 0.0, 1.0, tol, tol, saveat=[0.5, 1.0], maxiters=10000)
    ref = R.solve(Chain64(model, p), x, 0.0, 1.0, tol, tol, save_t=0.5)
    assert (got["stats"]["naccept"], got["stats"]["nreject"]) == (ref["naccept"], ref["nreject"])
    # at x6 the field amplifies fp32 rounding along the solve: the bar is also what a second fp32 summation order
    # (numpy BLAS) on the same steps lands at, with a margin
    r32 = R.solve(Chain32(model, p), x, 0.0, 1.0, tol, tol, save_t=0.5)
    bar = max(1e-5, 0.5 * tol, 4.0 * err(r32["u"], ref["u"]))
    print(f"x{scale} tol {tol:g}: gpu err {err(got['u'][1].cpu().numpy(), ref['u']):.2e}, float32-BLAS err {err(r32['u'], ref['u']):.2e}")
    assert err(got["u"][1].cpu().numpy(), ref["u"]) <= bar
    assert err(got["u"][0].cpu().numpy(), ref["u_save"]) <= max(1e-5, 0.5 * tol, 4.0 * err(r32["u_save"], ref["u_save"]))


@pytest.mark.parametrize("mode", ["none", "unbiased", "biased"])
def test_node_forward_modes_vs_float64(gpu_pkg, mode):
    """glorot scale: counts bounded, not asserted equal (module docstring)"""
    P = gpu_pkg
    model = physionet(P)
    h, p, x = mk(P, model, 64)
    xd = torch.from_numpy(x).cuda()
    tol = 1e-7
    got = h.node_forward(xd, 0.0, 1.0, tol, tol, mode=mode, t1_or_rand=0.43, maxiters=10000)
    ref = R.solve(Chain64(model, p), x, 0.0, 1.0, tol, tol)
    assert got["stats"]["retcode"] == 0
    assert err(got["u_end"].cpu().numpy(), ref["u"]) <= 1e-5
    assert ref["naccept"] <= got["stats"]["naccept"] <= 2 * ref["naccept"] + 2 and got["stats"]["nreject"] <= 3
    # (reg_val at this tolerance and scale is EEst * dt of a rounding-dominated estimate: positive and finite only)
    assert np.isfinite(got["reg_val"]) and (got["reg_val"] > 0) == (mode != "none")
    # the layer with a saveat series in all three modes: sol.u against the float64 RK4 states
    times = [0.25, 0.5, 1.0]
    node = P.NeuralODE(model, regularize=mode, abstol=tol, reltol=tol, saveat=times, save_start=False, maxiters=10000,
                       field="dense_chain")
    st = node.initialstates(np.random.default_rng(2))
    sol, st2 = node(xd, torch.from_numpy(p).cuda(), st)
    assert [float(t) for t in sol.t] == times
    want = rk4_states(Chain64(model, p).f64, x, times)
    for u, w in zip(sol.u, want):
        assert err(u.cpu().numpy(), w) <= 1e-5
    assert (st2["reg_val"] > 0) == (mode != "none")


def rk4_states(f64, x, times, nsteps=400):
    u, out, h = np.asarray(x, np.float64), [], 1.0 / nsteps
    marks = {int(round(t * nsteps)) for t in times}
    for k in range(nsteps):
        t = k * h
        k1 = f64(u, t); k2 = f64(u + 0.5 * h * k1, t + 0.5 * h); k3 = f64(u + 0.5 * h * k2, t + 0.5 * h); k4 = f64(u + h * k3, t + h)
        u = u + (h / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)
        if k + 1 in marks:
            out.append(u.copy())
    return out


def test_cross_check_against_the_mlp_handle(gpu_pkg):
    """a 2-layer TDChain through field="dense_chain" and through the MLP handle, same parameters"""
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    P = gpu_pkg
    D, H, B = 32, 64, 40
    model = P.TDChain(P.Chain(P.Dense(D + 1, H, "tanh"), P.Dense(H + 1, D)))
    assert np.array_equal(P.glorot_chain_params(model, seed=5), P.glorot_params(model, seed=5))
    for scale in (1.0, 3.0):
        hc, p, x = mk(P, model, B, scale=scale)
        hm = Handle(_mlp_desc(model))
        hm.set_params(torch.from_numpy(p))
        xd = torch.from_numpy(x).cuda()
        assert err(hc.rhs(xd, 0.3).cpu().numpy(), hm.rhs(xd, 0.3).cpu().numpy()) <= 1e-5
        k1 = hm.rhs(xd, 0.1)
        sc, sm = hc.perform_step(xd, k1, 0.1, 0.05, 1e-5, 1e-5), hm.perform_step(xd, k1, 0.1, 0.05, 1e-5, 1e-5)
        assert err(sc["u"].cpu().numpy(), sm["u"].cpu().numpy()) <= 1e-5
        gc = hc.solve(xd, 0.0, 1.0, 1e-5, 1e-5, saveat=[1.0])
        gm = hm.solve(xd, 0.0, 1.0, 1e-5, 1e-5, saveat=[1.0])
        assert err(gc["u"][-1].cpu().numpy(), gm["u"][-1].cpu().numpy()) <= 1e-5
        if scale == 3.0:
            assert (gc["stats"]["naccept"], gc["stats"]["nreject"]) == (gm["stats"]["naccept"], gm["stats"]["nreject"])
    ps = torch.from_numpy(p).cuda()
    cot = torch.from_numpy(np.random.default_rng(9).standard_normal((B, D)).astype(np.float32)).cuda()
    nc = P.NeuralODE(model, regularize="unbiased", abstol=1e-6, reltol=1e-6, field="dense_chain")
    nm = P.NeuralODE(model, regularize="unbiased", abstol=1e-6, reltol=1e-6)
    st = nc.initialstates(np.random.default_rng(0))
    dxc, dpc, ic = nc.pullback(xd, ps, st, cot, w_reg=0.5)
    dxm, dpm, im = nm.pullback(xd, ps, st, cot, w_reg=0.5)
    assert rel(dxc.cpu().numpy(), dxm.cpu().numpy()) <= 3e-4 and rel(dpc.cpu().numpy(), dpm.cpu().numpy()) <= 3e-4
    with pytest.raises(NotImplementedError):
        P.NeuralODE(model, solver="vcab3", field="dense_chain")


def reference_grads(model, p, x, times, cots, nsteps=200):
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    f = torch_field(model, pt)
    h = 1.0 / nsteps
    u, loss = xt, 0.0
    marks = {int(round(t * nsteps)): i for i, t in enumerate(times)}
    for k in range(nsteps):
        t = k * h
        k1 = f(u, t); k2 = f(u + 0.5 * h * k1, t + 0.5 * h); k3 = f(u + 0.5 * h * k2, t + 0.5 * h); k4 = f(u + h * k3, t + h)
        u = u + (h / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)
        if k + 1 in marks:
            loss = loss + (u * torch.tensor(cots[marks[k + 1]], dtype=torch.float64)).sum()
    loss.backward()
    return xt.grad.numpy(), pt.grad.numpy()


@pytest.mark.parametrize("regularize", ["none", "unbiased", "biased"])
def test_physionet_series_pullback_vs_float64_autograd(gpu_pkg, regularize):
    P = gpu_pkg
    model = physionet(P)
    h, p, x = mk(P, model, 12, scale=1.5)
    times = [0.25, 0.5, 1.0]
    node = P.NeuralODE(model, regularize=regularize, abstol=1e-6, reltol=1e-6, saveat=times, save_start=False, maxiters=10000,
                       field="dense_chain")
    st = node.initialstates(np.random.default_rng(3))
    xd, ps = torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()
    cots = np.random.default_rng(11).standard_normal((3, 12, 20)).astype(np.float32)
    dx, dp, info = node.pullback(xd, ps, st, torch.from_numpy(cots).cuda(), w_reg=0.0)
    gx, gp = reference_grads(model, p, x, times, cots)
    print(f"{regularize}: dx rel {rel(dx.cpu().numpy(), gx):.2e} dp rel {rel(dp.cpu().numpy(), gp):.2e}")
    assert rel(dx.cpu().numpy(), gx) < 3e-4 and rel(dp.cpu().numpy(), gp) < 3e-4
    if regularize != "none":
        sol, st2 = node(xd, ps, st)
        dxr, dpr, infr = node.pullback(xd, ps, st, torch.from_numpy(cots).cuda(), w_reg=3.0)
        assert infr["reg_val"] == st2["reg_val"] and infr["reg_val"] > 0
        assert rel(dxr.cpu().numpy(), dx.cpu().numpy()) < 1e-5   # the regulariser has no gradient to x
        assert not torch.equal(dpr, dp) and torch.isfinite(dpr).all()


def test_td3_end_state_pullback_vs_float64_autograd(gpu_pkg):
    P = gpu_pkg
    model = shapes(P)["td3_tanh"]
    h, p, x = mk(P, model, 9, scale=1.5)
    node = P.NeuralODE(model, regularize="unbiased", abstol=1e-6, reltol=1e-6, maxiters=10000, field="dense_chain")
    st = node.initialstates(np.random.default_rng(5))
    cot = np.random.default_rng(12).standard_normal((9, 32)).astype(np.float32)
    dx, dp, _ = node.pullback(torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda(), st, torch.from_numpy(cot).cuda())
    gx, gp = reference_grads(model, p, x, [1.0], [cot])
    assert rel(dx.cpu().numpy(), gx) < 3e-4 and rel(dp.cpu().numpy(), gp) < 3e-4


@pytest.mark.parametrize("reg_type", ["error_estimate", "stiffness_estimate"])
def test_step_reg_grad_vs_float64_autograd(gpu_pkg, reg_type):
    """d (EEst*dt) / dp and d stiffness / dp of one Tsit5 step (uprev, k1, dt constant) by float64 autograd"""
    P = gpu_pkg
    model = shapes(P)["td3_gelu"]
    h, p, x = mk(P, model, 10, scale=3.0)
    f = Chain64(model, p)
    t, dt, tol = 0.2, 0.1, 1e-4
    k1 = f(x, t)
    g, rv = h.step_reg_grad(torch.from_numpy(x).cuda(), torch.from_numpy(k1).cuda(), t, dt, tol, tol, reg_type=reg_type)
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    ft = torch_field(model, pt)
    up, ks = torch.tensor(x, dtype=torch.float64), [torch.tensor(k1, dtype=torch.float64)]
    cs = [R.C[0], R.C[1], R.C[2], R.C[3], 1.0, 1.0]
    xs = {}
    for s in range(2, 8):
        xs[s] = up + dt * sum(a * k for a, k in zip(R.A[s], ks))
        ks.append(ft(xs[s], t + cs[s - 2] * dt))
    u = xs[7]
    utilde = dt * sum(b * k for b, k in zip(R.BT, ks))
    rms = lambda v: torch.sqrt((v * v).mean())
    if reg_type == "error_estimate":
        val = rms(utilde / (tol + torch.maximum(up.abs(), u.abs()) * tol)) * dt
    else:
        val = (rms(ks[6] - ks[5]) / (rms(u - xs[6]) + float(np.finfo(np.float32).eps))).abs() / 3.5068
    val.backward()
    assert abs(float(rv) - float(val.detach())) <= 1e-3 * float(val.detach())
    assert rel(g.cpu().numpy(), pt.grad.numpy()) < 3e-4, rel(g.cpu().numpy(), pt.grad.numpy())


def test_physionet_end_to_end_b512(gpu_pkg):
    """the experiment's configuration: B = 512, tol 1.4e-8, :unbiased, a saveat series (physionet.yml)"""
    P = gpu_pkg
    model = physionet(P)
    h, p, x = mk(P, model, 512)
    times = [0.25, 0.5, 0.75, 1.0]
    node = P.NeuralODE(model, regularize="unbiased", abstol=1.4e-8, reltol=1.4e-8, saveat=times, save_start=False, maxiters=100000,
                       field="dense_chain")
    st = node.initialstates(np.random.default_rng(0))
    xd, ps = torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda()
    sol, st2 = node(xd, ps, st)
    assert sol.retcode == "Success" and np.isfinite(float(st2["reg_val"]))
    for u, w in zip(sol.u, rk4_states(Chain64(model, p).f64, x, times)):
        assert torch.isfinite(u).all() and err(u.cpu().numpy(), w) <= 1e-5
    cots = torch.from_numpy(np.random.default_rng(1).standard_normal((4, 512, 20)).astype(np.float32)).cuda()
    dx, dp, info = node.pullback(xd, ps, st, cots, w_reg=100.0)
    assert info["stats_bwd"]["retcode"] == 0 and torch.isfinite(dx).all() and torch.isfinite(dp).all()
