"""The wide Dense-chain vector field (lrnde_create_wide_chain, csrc/lrnde_wide_chain.hpp; NeuralODE(field="wide_chain")):
Dense chains wider than 128 — the MNIST TDChain with two hidden layers among them — with weights streamed as MFMA operands.

Yardsticks.  Bits: the float32 host restatements in the canonical order (tests/wide_chain_host.cpp for the field,
tests/wide_chain_vjp_host.cpp for its vector-Jacobian product) on shapes that between them take every branch of wide_gemm
in both directions (tests/test_host_wide_chain.py holds wide_chain_cases.gemm_paths to that), the MLP handle and the
C oracle on the two-layer MNIST shape, the small chain handle on the PhysioNet shape.  Everything else: float64
restatements (a numpy field rounded once to float32 under np_restatement's Tsit5 step / solve) and float64 torch autograd
through a fine RK4 integration — no code shared with the kernels.  Tolerances are tests/test_gpu_chain.py's: 1e-5
scale-relative on f-evals, steps and solutions; max(1e-5, 4 x the distance of a float32-BLAS run from float64) where depth or
weight scale amplifies rounding; 3e-4 of each gradient's norm for pullbacks; accepted / rejected counts equal only on the
cases tests/test_host_wide_chain.py holds a second float32 summation order to the float64 counts on (weights x3 / x6)."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import np_restatement as R
import wide_chain_cases as WC

pytestmark = pytest.mark.gpu

ALL = ["mnist2", "mnist3", "seg_edges", "odd_td", "deep16", "w1024", "physionet", "sq520", "cap_mixed", "cap_fwd", "full1024"]


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. bits ----
@pytest.mark.parametrize("name", ALL)
def test_rhs_is_the_host_restatement_bit_for_bit(gpu_pkg, name):
    P = gpu_pkg
    model = WC.shapes(P)[name]
    h, p, x = WC.mk(P, model, max(WC.BATCHES))
    for B in WC.BATCHES:
        for t in (0.0, 0.37):
            got = h.rhs(cu(x[:B]), t).cpu().numpy()
            want = WC.run_host(model, p, x[:B], t)
            assert np.array_equal(got, want), (name, B, t, WC.err(got, want))


def _vjp_inputs(P, name, B):
    model = WC.shapes(P)[name]
    h, p, x = WC.mk(P, model, B)
    lam = np.random.default_rng(7).standard_normal(x.shape).astype(np.float32)
    return model, h, p, x, lam


@pytest.mark.parametrize("name", ALL)
def test_vjp_is_the_host_restatement_bit_for_bit(gpu_pkg, name):
    """dy and the parameter cotangent in the order the header states: 112-output segments of W^T delta left to right, the
    tile's columns 0..15 as one fma chain per weight, the t column by fma, the bias a plain sum, tiles in tile order"""
    P = gpu_pkg
    t = 0.61
    model, h, p, x, lam = _vjp_inputs(P, name, max(WC.BATCHES))
    for B in WC.BATCHES:
        dy, gp = h.vjp(cu(x[:B]), t, cu(lam[:B]))
        wdy, wgp = WC.run_vjp_host(model, p, x[:B], lam[:B], t)
        dy, gp = dy.cpu().numpy(), gp.cpu().numpy()
        assert np.array_equal(dy, wdy), (name, B, "dy", WC.err(dy, wdy), int((dy != wdy).sum()))
        assert np.array_equal(gp, wgp), (name, B, "gp", WC.err(gp, wgp), int((gp != wgp).sum()))
        dy2, none = h.vjp(cu(x[:B]), t, cu(lam[:B]), want_gp=False)
        assert none is None and np.array_equal(dy2.cpu().numpy(), wdy), (name, B, "dy without gp")


def test_vjp_over_two_launches_is_the_host_restatement(gpu_pkg):
    """full1024 at B = 497: 32 workgroups, of which one launch's scratch (256 MiB: a record and a P-float partial each)
    holds 30; the second launch runs workgroups 30 and 31, the last with one column"""
    P = gpu_pkg
    name, B, t = "full1024", 497, 0.61
    dims = WC.model_dims(WC.shapes(P)[name])
    nwg, chunk = -(-B // WC.NB), WC.vjp_chunk(dims, 0)
    assert chunk == 30 < nwg == 32 and B - 31 * WC.NB == 1
    model, h, p, x, lam = _vjp_inputs(P, name, B)
    dy, gp = h.vjp(cu(x), t, cu(lam))
    dy, gp = dy.cpu().numpy(), gp.cpu().numpy()
    wdy, wgp = WC.run_vjp_host(model, p, x, lam, t)
    assert np.array_equal(dy, wdy), ("dy", WC.err(dy, wdy), int((dy != wdy).sum()))
    assert np.array_equal(gp, wgp), ("gp", WC.err(gp, wgp), int((gp != wgp).sum()))
    # (what each launch summing from 0 would have given is another vector)
    assert not np.array_equal(WC.run_vjp_host(model, p, x[:64], lam[:64], t, chunk=2)[1], WC.run_vjp_host(model, p, x[:64], lam[:64], t)[1])
    (dy64, gp64), (bar_dy, bar_gp), e32 = WC.vjp_bars(model, p, x, lam, t)
    edy, egp = WC.err(dy, dy64), WC.err(gp, gp64)
    print(f"{name} B={B}: dy err {edy:.2e} gp err {egp:.2e}; float32 autograd {e32[0]:.2e} {e32[1]:.2e}; bars {bar_dy:.2e} {bar_gp:.2e}")
    assert edy <= bar_dy and egp <= bar_gp
    dy2, none = h.vjp(cu(x), t, cu(lam), want_gp=False)   # 32 records fit one launch
    assert none is None and np.array_equal(dy2.cpu().numpy(), wdy)


@pytest.mark.parametrize("B", [16, 33])
def test_mnist2_rhs_is_the_mlp_handle_and_the_oracle_bit_for_bit(gpu_pkg, oracle, B):
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    P = gpu_pkg
    model = WC.shapes(P)["mnist2"]
    h, p, x = WC.mk(P, model, B)
    hm = Handle(_mlp_desc(model))
    hm.set_params(torch.from_numpy(p))
    fld = oracle.MlpField(784, 100, p)
    for t in (0.0, 0.61):
        got = h.rhs(cu(x), t)
        assert torch.equal(got, hm.rhs(cu(x), t)), (B, t)
        assert np.array_equal(got.cpu().numpy(), fld.rhs(x, t)), (B, t)


@pytest.mark.parametrize("B", [1, 17, 33])
def test_physionet_rhs_is_the_small_chain_handle_bit_for_bit(gpu_pkg, B):
    """every input width there is <= 112: one segment, the small handle's single fma chain"""
    from localregneuralde_jl_amd.layers import Handle, _chain_desc
    P = gpu_pkg
    model = WC.shapes(P)["physionet"]
    h, p, x = WC.mk(P, model, B)
    hs = Handle(_chain_desc(model))
    hs.set_params(torch.from_numpy(p))
    for t in (0.0, 0.3):
        assert torch.equal(h.rhs(cu(x), t), hs.rhs(cu(x), t))


# ---- 2. column independence and repeatability ----
@pytest.mark.parametrize("name", ["mnist3", "odd_td"])
def test_columns_are_independent(gpu_pkg, name):
    P = gpu_pkg
    model = WC.shapes(P)[name]
    h, p, x = WC.mk(P, model, 512)
    xd = cu(x)
    k1 = h.rhs(xd, 0.2)
    full = h.rhs(xd, 0.3)
    stp = h.perform_step(xd, k1, 0.2, 0.05, 1e-6, 1e-6)
    perm = torch.from_numpy(np.random.default_rng(3).permutation(512)).cuda()
    assert torch.equal(h.rhs(xd[perm].contiguous(), 0.3), full[perm])
    sp = h.perform_step(xd[perm].contiguous(), k1[perm].contiguous(), 0.2, 0.05, 1e-6, 1e-6)
    assert torch.equal(sp["u"], stp["u"][perm]) and torch.equal(sp["k7"], stp["k7"][perm])
    for c in (0, 15, 16, 200, 511):
        xc, kc = xd[c:c + 1].contiguous(), k1[c:c + 1].contiguous()
        assert torch.equal(h.rhs(xc, 0.3)[0], full[c])
        s1 = h.perform_step(xc, kc, 0.2, 0.05, 1e-6, 1e-6)
        assert torch.equal(s1["u"][0], stp["u"][c]) and torch.equal(s1["k7"][0], stp["k7"][c])


@pytest.mark.parametrize("name", ["mnist3", "odd_td"])
def test_forward_and_pullback_repeat_bitwise(gpu_pkg, name):
    P = gpu_pkg
    model = WC.shapes(P)[name]
    p, x = WC.mk_inputs(P, model, 33)
    node = P.NeuralODE(model, regularize="unbiased", abstol=1e-5, reltol=1e-5, saveat=[0.25, 0.5, 1.0], save_start=False,
                       field="wide_chain")
    st = node.initialstates(np.random.default_rng(1))
    xd, ps = cu(x), cu(p)
    cots = cu(np.random.default_rng(4).standard_normal((3,) + x.shape).astype(np.float32))
    runs = [node.pullback(xd, ps, st, cots, w_reg=2.0) for _ in range(2)]
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2]["sol_u"], runs[1][2]["sol_u"])
    assert runs[0][2]["adjoint_loop"] == "host"
    lam = cu(np.random.default_rng(5).standard_normal(x.shape).astype(np.float32))
    h = node.handle()
    a, b = h.vjp(xd, 0.4, lam), h.vjp(xd, 0.4, lam)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 3. perform_step and init_dt ----
@pytest.mark.parametrize("name", ["mnist3", "seg_edges", "odd_td", "deep16", "sq520", "cap_mixed"])
@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_perform_step_and_init_dt_vs_float64(gpu_pkg, name, scale):
    P = gpu_pkg
    model = WC.shapes(P)[name]
    h, p, x = WC.mk(P, model, 33, scale=scale)
    f = WC.Chain64(model, p)
    k1 = f(x, 0.1)
    ref = R.tsit5_step(f, x, k1, 0.1, 0.05, 1e-4, 1e-4)
    got = h.perform_step(cu(x), cu(k1), 0.1, 0.05, 1e-4, 1e-4)
    # a deep chain at weights x3 amplifies fp32 rounding through its layers: the bar is 1e-5, or what a second fp32
    # summation order of the same field (numpy BLAS) lands at, with a margin
    f32 = WC.Chain32(model, p)
    r32 = R.tsit5_step(f32, x, k1, 0.1, 0.05, 1e-4, 1e-4)
    for key in ("u", "k7"):
        bar = max(1e-5, 4.0 * WC.err(r32[key], ref[key]))
        e = WC.err(got[key].cpu().numpy(), ref[key])
        print(f"{name} x{scale} {key}: gpu err {e:.2e} bar {bar:.2e}")
        assert e <= bar, (key, e, bar)
    # EEst / stiffness: at weights x3 the estimate is truncation and agrees to 2 %; at the glorot scale it is fp32 rounding
    # noise of the stage values: finite and positive only
    print(f"{name} x{scale}: EEst gpu {got['eest']:.6g} ref {ref['eest']:.6g}; stiffness gpu {got['reg_stiff']:.6g} "
          f"ref {ref['reg_stiff']:.6g}")
    assert np.isfinite(got["eest"]) and got["eest"] > 0 and np.isfinite(got["reg_stiff"]) and got["reg_stiff"] >= 0
    if scale >= 3.0:
        for key in ("eest", "reg_stiff"):
            bar = max(2e-2 * float(ref[key]), 4.0 * abs(float(r32[key]) - float(ref[key])))
            assert abs(float(got[key]) - float(ref[key])) <= bar, (key, float(got[key]), float(ref[key]), float(r32[key]))
    dt_ref, f0 = R.init_dt(f, x, 0.0, 1.0, 1e-4, 1e-4)
    dt, k1g = h.init_dt(cu(x), 0.0, 1.0, 1e-4, 1e-4)
    assert abs(float(dt) - float(dt_ref)) <= 1e-4 * float(dt_ref), (float(dt), float(dt_ref))
    assert WC.err(k1g.cpu().numpy(), f0) <= max(1e-5, 4.0 * WC.err(f32(x, 0.0), f.f64(x, 0.0)))


# ---- 4. solve ----
@pytest.mark.parametrize("name,scale,tol", WC.GPU_COUNT_CASES)
def test_solve_counts_and_states_vs_float64(gpu_pkg, name, scale, tol):
    P = gpu_pkg
    model, B = WC.count_shapes(P)[name]
    h, p, x = WC.mk(P, model, B, scale=scale)
    got = h.solve(cu(x), 0.0, 1.0, tol, tol, saveat=[0.5, 1.0], maxiters=10000)
    ref = R.solve(WC.Chain64(model, p), x, 0.0, 1.0, tol, tol, save_t=0.5)
    assert (got["stats"]["naccept"], got["stats"]["nreject"]) == (ref["naccept"], ref["nreject"])
    r32 = R.solve(WC.Chain32(model, p), x, 0.0, 1.0, tol, tol, save_t=0.5)
    bar = max(1e-5, 0.5 * tol, 4.0 * WC.err(r32["u"], ref["u"]))
    e = WC.err(got["u"][1].cpu().numpy(), ref["u"])
    print(f"{name} x{scale} tol {tol:g}: gpu err {e:.2e}, float32-BLAS err {WC.err(r32['u'], ref['u']):.2e}")
    assert e <= bar
    assert WC.err(got["u"][0].cpu().numpy(), ref["u_save"]) <= max(1e-5, 0.5 * tol, 4.0 * WC.err(r32["u_save"], ref["u_save"]))


def _saved_bar(tol, u32, u64):
    return max(1e-5, 0.5 * tol, 4.0 * WC.err(u32, u64))


@pytest.mark.parametrize("name,scale,tol", WC.FOOTER_CASES)
def test_save_footer_saveat_and_save_start_vs_float64(gpu_pkg, name, scale, tol):
    """k_step_wide's savevalues footer: the start value, two save times inside one accepted step (its slot loop), one in
    another step, the end copy; odd130 at D % 4 != 0 and with a rejected step between"""
    P = gpu_pkg
    model, B = WC.count_shapes(P)[name]
    h, p, x = WC.mk(P, model, B, scale=scale)
    f64, f32 = WC.Chain64(model, p), WC.Chain32(model, p)
    saves = WC.footer_saves(R.solve(f64, x, 0.0, 1.0, tol, tol)["t_steps"]) + [1.0]
    ref = R.solve(f64, x, 0.0, 1.0, tol, tol, saveat=saves, save_start=True)
    r32 = R.solve(f32, x, 0.0, 1.0, tol, tol, saveat=saves, save_start=True)
    hold = WC.steps_holding(ref["t_steps"], saves[:3])
    assert hold[1] == hold[2] != hold[0]
    got = h.solve(cu(x), 0.0, 1.0, tol, tol, saveat=saves, save_start=True, save_everystep=False, maxiters=10000)
    assert (got["stats"]["naccept"], got["stats"]["nreject"]) == (ref["naccept"], ref["nreject"])
    assert np.array_equal(got["t"], ref["t_saved"]) and len(got["t"]) == 5
    assert torch.equal(got["u"][0], cu(x))
    for i in range(5):
        e, bar = WC.err(got["u"][i].cpu().numpy(), ref["u_saved"][i]), _saved_bar(tol, r32["u_saved"][i], ref["u_saved"][i])
        print(f"{name} x{scale} t={got['t'][i]:.4f}: gpu err {e:.2e} bar {bar:.2e}")
        assert e <= bar, (i, e, bar)


@pytest.mark.parametrize("name,scale,tol", WC.FOOTER_CASES)
def test_save_footer_everystep_vs_float64(gpu_pkg, name, scale, tol):
    """save_everystep beside save times and save_start: per accepted step the save times it passes, then its end.  The
    times the call gives (start, save times, t1) are exact and sit at the restatement's places in the series; a step's end
    is where the float32 controller put it (the float64 restatement's differs in the last digits), so its state is held
    to the float64 solution at that very time"""
    P = gpu_pkg
    model, B = WC.count_shapes(P)[name]
    h, p, x = WC.mk(P, model, B, scale=scale)
    f64, f32 = WC.Chain64(model, p), WC.Chain32(model, p)
    saves = WC.footer_saves(R.solve(f64, x, 0.0, 1.0, tol, tol)["t_steps"])
    ref = R.solve(f64, x, 0.0, 1.0, tol, tol, saveat=saves, save_start=True, save_everystep=True)
    got = h.solve(cu(x), 0.0, 1.0, tol, tol, saveat=saves, save_start=True, save_everystep=True, maxiters=10000)
    assert (got["stats"]["naccept"], got["stats"]["nreject"]) == (ref["naccept"], ref["nreject"])
    tg = got["t"]
    assert len(tg) == len(ref["t_saved"]) == 1 + 3 + ref["naccept"]
    given = np.isin(ref["t_saved"], np.array([0.0] + saves, np.float32))
    assert np.array_equal(tg[given], ref["t_saved"][given]) and tg[-1] == np.float32(1.0) and np.all(np.diff(tg) > 0)
    print(f"{name} x{scale}: step ends differ from the float64 solve's by at most {np.abs(tg - ref['t_saved']).max():.2e}")
    ends = [float(v) for v in tg[~given]]
    at64 = R.solve(f64, x, 0.0, 1.0, tol, tol, saveat=ends)["u_saved"]
    at32 = R.solve(f32, x, 0.0, 1.0, tol, tol, saveat=ends)["u_saved"]
    assert len(at64) == len(ends) == ref["naccept"]
    want = iter(at64); w32 = iter(at32)
    r32 = R.solve(f32, x, 0.0, 1.0, tol, tol, saveat=saves, save_start=True, save_everystep=True)
    worst = 0.0
    for i in range(len(tg)):
        u64, u32 = (ref["u_saved"][i], r32["u_saved"][i]) if given[i] else (next(want), next(w32))
        e, bar = WC.err(got["u"][i].cpu().numpy(), u64), _saved_bar(tol, u32, u64)
        worst = max(worst, e / bar)
        assert e <= bar, (i, float(tg[i]), bool(given[i]), e, bar)
    print(f"{name} x{scale}: {len(tg)} saved states, worst err / bar {worst:.2f}")


# ---- 5. layer forward ----
@pytest.fixture(scope="module")
def mnist3_rk4(gpu_pkg):
    P = gpu_pkg
    model = WC.shapes(P)["mnist3"]
    p, x = WC.mk_inputs(P, model, 16)
    times = [0.25, 0.5, 1.0]
    return model, p, x, times, WC.rk4_states(WC.Chain64(model, p).f64, x, times)


@pytest.mark.parametrize("mode", ["none", "unbiased", "biased"])
def test_layer_forward_modes_vs_float64(gpu_pkg, mnist3_rk4, mode):
    P = gpu_pkg
    model, p, x, times, want = mnist3_rk4
    tol = 1e-7
    node = P.NeuralODE(model, regularize=mode, abstol=tol, reltol=tol, saveat=times, save_start=False, maxiters=10000,
                       field="wide_chain")
    st = node.initialstates(np.random.default_rng(2))
    sol, st2 = node(cu(x), cu(p), st)
    assert [float(t) for t in sol.t] == times
    for u, w in zip(sol.u, want):
        assert WC.err(u.cpu().numpy(), w) <= 1e-5
    assert np.isfinite(st2["reg_val"]) and (st2["reg_val"] > 0) == (mode != "none")
    got = node.handle().node_forward(cu(x), 0.0, 1.0, tol, tol, mode=mode, t1_or_rand=0.43, maxiters=10000)
    assert got["stats"]["retcode"] == 0 and WC.err(got["u_end"].cpu().numpy(), want[-1]) <= 1e-5
    assert (got["reg_val"] > 0) == (mode != "none")


# ---- 6. VJP ----
@pytest.mark.parametrize("name", ALL)
def test_vjp_vs_float64_autograd(gpu_pkg, name):
    P = gpu_pkg
    model, h, p, x, lam = _vjp_inputs(P, name, 17)
    t = 0.61
    dy, gp = h.vjp(cu(x), t, cu(lam))
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    ut = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    (WC.torch_field(model, pt)(ut, t) * torch.tensor(lam, dtype=torch.float64)).sum().backward()
    edy, egp = WC.err(dy.cpu().numpy(), ut.grad.numpy()), WC.err(gp.cpu().numpy(), pt.grad.numpy())
    print(f"{name}: dy err {edy:.2e} gp err {egp:.2e}")
    assert edy <= 1e-5 and egp <= 1e-5
    dy2, none = h.vjp(cu(x), t, cu(lam), want_gp=False)
    assert none is None and torch.equal(dy2, dy)


# ---- 7. pullbacks ----
@pytest.mark.parametrize("name,B", [("mnist3", 16), ("odd_td", 9)])
def test_pullbacks_vs_float64_autograd(gpu_pkg, name, B):
    P = gpu_pkg
    model = WC.shapes(P)[name]
    p, x = WC.mk_inputs(P, model, B, scale=1.5)
    xd, ps = cu(x), cu(p)
    times = [0.25, 0.5, 1.0]
    rng = np.random.default_rng(11)
    # a series of cotangents
    node = P.NeuralODE(model, regularize="unbiased", abstol=1e-6, reltol=1e-6, saveat=times, save_start=False, maxiters=10000,
                       field="wide_chain")
    st = node.initialstates(np.random.default_rng(3))
    cots = rng.standard_normal((3,) + x.shape).astype(np.float32)
    dx, dp, info = node.pullback(xd, ps, st, cu(cots), w_reg=0.0)
    gx, gp = WC.reference_grads(model, p, x, times, cots)
    print(f"{name} series: dx rel {WC.rel(dx.cpu().numpy(), gx):.2e} dp rel {WC.rel(dp.cpu().numpy(), gp):.2e}")
    assert WC.rel(dx.cpu().numpy(), gx) < 3e-4 and WC.rel(dp.cpu().numpy(), gp) < 3e-4
    sol, st2 = node(xd, ps, st)
    dxr, dpr, infr = node.pullback(xd, ps, st, cu(cots), w_reg=3.0)
    assert infr["reg_val"] == st2["reg_val"] and infr["reg_val"] > 0
    assert WC.rel(dxr.cpu().numpy(), dx.cpu().numpy()) < 1e-5   # the regulariser has no gradient to x
    assert not torch.equal(dpr, dp) and torch.isfinite(dpr).all()
    # the end state's cotangent
    node = P.NeuralODE(model, regularize="unbiased", abstol=1e-6, reltol=1e-6, maxiters=10000, field="wide_chain")
    cot = rng.standard_normal(x.shape).astype(np.float32)
    dx, dp, _ = node.pullback(xd, ps, st, cu(cot))
    gx, gp = WC.reference_grads(model, p, x, [1.0], [cot])
    print(f"{name} end: dx rel {WC.rel(dx.cpu().numpy(), gx):.2e} dp rel {WC.rel(dp.cpu().numpy(), gp):.2e}")
    assert WC.rel(dx.cpu().numpy(), gx) < 3e-4 and WC.rel(dp.cpu().numpy(), gp) < 3e-4


def test_training_step_on_mnist3(gpu_pkg):
    P = gpu_pkg
    model = WC.shapes(P)["mnist3"]
    B, K, D = 16, 10, 784
    p, x = WC.mk_inputs(P, model, B)
    rng = np.random.default_rng(2)
    xd, ps = cu(x), cu(p)
    pc = cu((rng.random(K * (D + 1), dtype=np.float32) - np.float32(0.5)) * np.float32(0.1))
    lab = cu(rng.integers(0, K, B).astype(np.int32))
    node = P.NeuralODE(model, regularize="unbiased", abstol=1e-5, reltol=1e-5, save_start=False, maxiters=10000, field="wide_chain")
    st = node.initialstates(np.random.default_rng(0))
    loss, st2, stats, grads, times = P.run_training_step(node, ps, pc, st, xd, lab, 2.5)
    assert np.isfinite(float(loss)) and stats["y_pred"].shape == (B, K) and float(stats["reg_val"]) > 0
    assert grads["neural_ode"].shape == (p.size,) and grads["classifier"].shape == pc.shape and grads["x"].shape == xd.shape
    assert all(torch.isfinite(g).all() for g in grads.values())
    # the same cotangent through the separate pullback gives the same parameter gradient
    _, _, info0 = node.pullback(xd, ps, st, torch.zeros_like(xd), w_reg=2.5)
    head = node.handle().classifier_ce(info0["u_end"].contiguous(), pc, K, lab)
    assert torch.equal(head["logits"], stats["y_pred"]) and head["loss"] == stats["ce_loss"]
    dx, dp, info = node.pullback(xd, ps, st, head["du"], w_reg=2.5)
    assert info["reg_val"] == stats["reg_val"] and loss == np.float32(head["loss"] + np.float32(2.5) * info["reg_val"])
    assert torch.equal(dp, grads["neural_ode"]) and torch.equal(dx, grads["x"])


# ---- 8. cross-check against the MLP handle ----
def test_mnist2_cross_check_against_the_mlp_handle(gpu_pkg):
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    P = gpu_pkg
    model = WC.shapes(P)["mnist2"]
    B = 24
    for scale in (1.0, 3.0):
        hc, p, x = WC.mk(P, model, B, scale=scale)
        hm = Handle(_mlp_desc(model))
        hm.set_params(torch.from_numpy(p))
        xd = cu(x)
        k1 = hm.rhs(xd, 0.1)
        sc, sm = hc.perform_step(xd, k1, 0.1, 0.05, 1e-5, 1e-5), hm.perform_step(xd, k1, 0.1, 0.05, 1e-5, 1e-5)
        assert WC.err(sc["u"].cpu().numpy(), sm["u"].cpu().numpy()) <= 1e-5
        assert WC.err(sc["k7"].cpu().numpy(), sm["k7"].cpu().numpy()) <= 1e-5
        gc_ = hc.solve(xd, 0.0, 1.0, 1e-5, 1e-5, saveat=[1.0])
        gm = hm.solve(xd, 0.0, 1.0, 1e-5, 1e-5, saveat=[1.0])
        assert WC.err(gc_["u"][-1].cpu().numpy(), gm["u"][-1].cpu().numpy()) <= 1e-5
        if scale == 3.0:
            assert (gc_["stats"]["naccept"], gc_["stats"]["nreject"]) == (gm["stats"]["naccept"], gm["stats"]["nreject"])
    ps = cu(p)
    cot = cu(np.random.default_rng(9).standard_normal(x.shape).astype(np.float32))
    nc = P.NeuralODE(model, regularize="unbiased", abstol=1e-6, reltol=1e-6, field="wide_chain")
    nm = P.NeuralODE(model, regularize="unbiased", abstol=1e-6, reltol=1e-6)
    st = nc.initialstates(np.random.default_rng(0))
    dxc, dpc, _ = nc.pullback(xd, ps, st, cot, w_reg=0.5)
    dxm, dpm, _ = nm.pullback(xd, ps, st, cot, w_reg=0.5)
    assert WC.rel(dxc.cpu().numpy(), dxm.cpu().numpy()) <= 3e-4 and WC.rel(dpc.cpu().numpy(), dpm.cpu().numpy()) <= 3e-4


# ---- 9. refusals ----
def test_refusals_leave_the_handle_usable(gpu_pkg):
    from localregneuralde_jl_amd import _lib as L
    P = gpu_pkg

    def desc(dims, td=0):
        d = L.WideChainDesc()
        d.nlayers, d.time_dep, d.input_act = len(dims) - 1, td, 0
        for i, v in enumerate(dims):
            d.dims[i] = v
        return d

    ctx = C.c_void_p()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.lib.lrnde_create_wide_chain(C.byref(ctx), C.byref(desc([8, 1025, 8])), 0, stream) == 8 and not ctx.value
    assert b"1024" in L.lib.lrnde_last_error(None)
    d17 = desc([8] * 17)
    d17.nlayers = 17
    assert L.lib.lrnde_create_wide_chain(C.byref(ctx), C.byref(d17), 0, stream) == 8 and not ctx.value
    assert b"1..16" in L.lib.lrnde_last_error(None)
    assert L.lib.lrnde_create_wide_chain(C.byref(ctx), C.byref(desc([8, 300, 9])), 0, stream) == 4 and not ctx.value

    model = WC.shapes(P)["seg_edges"]
    h, p, x = WC.mk(P, model, 5)
    before = h.rhs(cu(x), 0.2)
    for alg in (1, 2):
        assert L.lib.lrnde_set_solver(h._ctx, alg) == 8 and b"Tsit5" in L.lib.lrnde_last_error(h._ctx)
    comm = C.c_void_p()
    assert L.lib.lrnde_local_comm_create(C.byref(comm), 1) == 0
    assert L.lib.lrnde_comm_init_local(h._ctx, comm, 0) == 8 and L.lib.lrnde_last_error(h._ctx)
    assert L.lib.lrnde_local_comm_destroy(comm) == 0
    with pytest.raises(L.LrndeError) as e1:
        h.bench_step(cu(x), before, 0.0, 0.01, 1e-4, 1e-4, reps=1)
    with pytest.raises(L.LrndeError) as e2:
        h.bench_exchange(5, reps=1)
    with pytest.raises(L.LrndeError) as e3:
        h.set_overlap(False)
    assert e1.value.code == e2.value.code == e3.value.code == 8
    assert all("MLP field's handle" in str(e.value) for e in (e1, e2, e3))   # each refusal carries its message
    assert torch.equal(h.rhs(cu(x), 0.2), before)
    got = h.solve(cu(x), 0.0, 1.0, 1e-4, 1e-4, saveat=[1.0])
    assert got["retcode"] == 0 and torch.isfinite(got["u"][-1]).all()


# ---- 10. resources ----
def _free_bytes():
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


def test_create_use_destroy_returns_device_memory(gpu_pkg):
    P = gpu_pkg
    model = WC.shapes(P)["mnist3"]
    B, K, D = 32, 10, 784
    p, x = WC.mk_inputs(P, model, B)
    xd, ps = cu(x), cu(p)
    pc = torch.zeros(K * (D + 1), device="cuda")
    lab = cu(np.random.default_rng(0).integers(0, K, B).astype(np.int32))

    def one_round(seed):
        node = P.NeuralODE(model, regularize="unbiased", abstol=1e-3, reltol=1e-3, save_start=False, maxiters=10000, field="wide_chain")
        st = node.initialstates(np.random.default_rng(seed))
        loss, *_ = P.run_training_step(node, ps, pc, st, xd, lab, 2.5)
        assert np.isfinite(float(loss))
        return node

    for i in range(2):
        one_round(i)._handle.close()
    before = _free_bytes()
    for i in range(6):
        one_round(10 + i)._handle.close()
    after = _free_bytes()
    print(f"6 rounds: free memory changed by {(after - before) / 2**20:+.1f} MiB")
    # one leaked handle of this shape holds > 6 MB (weight images 2 x 1 MB, state workspace, dense record, VJP partials 1.3 MB)
    assert before - after < (4 << 20)
    held = [one_round(20 + i) for i in range(3)]
    live = _free_bytes()
    for node in held:
        node._handle.close()
    held.clear()
    assert after - live > (6 << 20) and _free_bytes() - live > (6 << 20)
