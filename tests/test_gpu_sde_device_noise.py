"""Gaussian noise drawn on the device (lrnde_sde_draw_noise, csrc/lrnde_noise.hpp) and the NeuralDSDE layer
with noise_source="device".

* the device Philox-4x32-10 returns the Random123 known-answer vectors; its normals equal the numpy restatement
  (tests/philox_np.py) to within one float32 ulp, and almost always bit for bit;
* the path is exactly the sequential float32 sum of the device's own increments; a column's noise does not depend on B or
  on nsteps; the statistics of 4 M normals are those of N(0, 1);
* the layer's forward equals the oracle loop fed the W and z that draw_noise gives for the seed the layer drew, and its
  pullbacks equal the same calls given those arrays explicitly (adaptive, EulerHeun, RKMil; SRI against the step loop)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import philox_np as PX
from test_gpu_sde_gradients import _params
from test_gpu_sde_layer import _check_forward
from test_philox_restatement import KAT

pytestmark = pytest.mark.gpu
f32 = np.float32
SEED = 0x243F6A8885A308D3


def _handle(P, D, H=16):
    from localregneuralde_jl_amd.layers import _mlp_desc
    return P.SdeHandle(_mlp_desc(P.Chain(P.Dense(D, H, "tanh"), P.Dense(H, D))))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def test_device_philox_returns_the_random123_vectors(gpu_pkg):
    from localregneuralde_jl_amd import _lib as L
    for ctr, key, want in KAT:
        out = (C.c_uint32 * 4)()
        assert L.lib.lrnde_hook_philox4x32_10((C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), out) == 0
        assert tuple(out) == want, ([hex(v) for v in out], [hex(v) for v in want])


@pytest.mark.parametrize("nsteps,B,D", [(256, 512, 32), (7, 3, 5), (33, 10, 72)])
def test_normals_match_the_numpy_restatement(gpu_pkg, nsteps, B, D):
    h = _handle(gpu_pkg, D)
    for stream in (0, 1, 3):
        got = h.draw_noise(SEED, stream, nsteps, B, 1.0, False).cpu().numpy()
        ref = PX.increments(SEED, stream, nsteps, B, D, 1.0)
        assert got.shape == ref.shape == (nsteps, B, D)
        assert np.isfinite(got).all()
        assert (np.abs(got.astype(np.float64) - ref) <= np.spacing(np.abs(ref))).all(), float(np.abs(got - ref).max())
        share = float((_bits(got) == _bits(ref)).mean())
        print(f"nsteps={nsteps} B={B} D={D} stream {stream}: {share * 100:.4f} % of {got.size} normals bit-equal to the restatement")
        assert share >= 0.9999


@pytest.mark.parametrize("nsteps,B,D,scale", [(256, 512, 32, f32(np.sqrt(f32(1.0 / 256)))), (130, 3, 5, f32(0.3)), (1, 2, 72, f32(2.0)),
                                              (0, 4, 6, f32(1.0))])
def test_path_is_the_sequential_float32_sum_of_the_increments(gpu_pkg, nsteps, B, D, scale):
    h = _handle(gpu_pkg, D)
    inc = h.draw_noise(SEED, 0, nsteps, B, scale, False).cpu().numpy()
    W = h.draw_noise(SEED, 0, nsteps, B, scale, True).cpu().numpy()
    assert inc.shape == (nsteps, B, D) and W.shape == (nsteps + 1, B, D)
    ref = np.concatenate([np.zeros((1, B, D), f32), np.cumsum(inc, axis=0, dtype=f32)], axis=0)
    assert np.array_equal(_bits(W), _bits(ref))
    assert np.array_equal(_bits(inc), _bits(h.draw_noise(SEED, 0, nsteps, B, 1.0, False).cpu().numpy() * scale))


def test_noise_does_not_depend_on_the_batch_or_the_length(gpu_pkg):
    D = 32
    h = _handle(gpu_pkg, D)
    sc = f32(np.sqrt(f32(1.0 / 256)))
    for cum in (False, True):
        big = h.draw_noise(SEED, 0, 256, 512, sc, cum).cpu().numpy()
        small = h.draw_noise(SEED, 0, 256, 7, sc, cum).cpu().numpy()
        assert np.array_equal(_bits(small), _bits(big[:, :7]))
        short = h.draw_noise(SEED, 0, 100, 512, sc, cum).cpu().numpy()
        assert np.array_equal(_bits(short), _bits(big[:short.shape[0]]))
    a = h.draw_noise(SEED, 0, 64, 16, 1.0, False)
    for other in (h.draw_noise(SEED + 1, 0, 64, 16, 1.0, False), h.draw_noise(SEED, 1, 64, 16, 1.0, False),
                  h.draw_noise(SEED ^ (1 << 40), 0, 64, 16, 1.0, False)):
        assert not torch.equal(a, other)
        assert float((a == other).float().mean()) < 1e-3


def test_statistics_of_four_million_normals(gpu_pkg):
    nsteps, B, D = 256, 512, 32
    h = _handle(gpu_pkg, D)
    z = h.draw_noise(SEED, 2, nsteps, B, 1.0, False).double().reshape(nsteps, B * D)
    n = z.numel()
    assert n >= 4_000_000
    mean, var = float(z.mean()), float(z.var())
    lag_step = float((z[1:] * z[:-1]).mean())
    lag_col = float((z[:, 1:] * z[:, :-1]).mean())
    print(f"{n} normals: mean {mean:.3e}, var {var:.5f}, lag-1 corr along steps {lag_step:.3e}, across columns {lag_col:.3e}")
    assert abs(mean) < 6 / np.sqrt(n)
    assert abs(var - 1) < 6 * np.sqrt(2 / n)
    assert abs(lag_step) < 6 / np.sqrt(n - B * D)
    assert abs(lag_col) < 6 / np.sqrt(n - nsteps)
    W = h.draw_noise(SEED, 0, nsteps, B, f32(np.sqrt(f32(1.0 / nsteps))), True)[nsteps].double().ravel()
    vw = float(W.var())
    print(f"Var(W[nfine]) over {W.numel()} columns: {vw:.4f} (t2 - t0 = 1)")
    assert abs(vw - 1.0) < 6 * np.sqrt(2 / W.numel())


def _layer(P, D, H, tol, nfine=256, **kw):
    return P.NeuralDSDE(P.Chain(P.Dense(D, H, "tanh"), P.Dense(H, D)), P.Dense(D, D), nfine=nfine, abstol=tol, reltol=tol,
                        noise_source="device", **kw)


def _replica(st):
    rng = copy.deepcopy(st["rng"])
    return rng, int(rng.integers(0, 2 ** 64, dtype=np.uint64))


@pytest.mark.parametrize("D,H,B,tol,nfine", [(32, 64, 512, 0.14, 256),    # BASELINE config 5
                                             (72, 32, 6, 0.1, 32)])        # D > 64: the generic kernels
@pytest.mark.parametrize("mode", ["unbiased", "biased", "none"])
def test_device_noise_layer_forward_equals_the_oracle_loop(oracle, gpu_pkg, D, H, B, tol, nfine, mode):
    P = gpu_pkg
    pd, pg = _params(D, H, 7)
    pd = (pd * f32(2.0)).astype(f32)
    ps = dict(drift=pd, diffusion=pg)
    x = np.random.default_rng(107).standard_normal((B, D)).astype(f32)
    node = _layer(P, D, H, tol, nfine, regularize=mode)
    st = node.initialstates(np.random.default_rng(0))
    sol, st2 = node(torch.from_numpy(x).cuda(), ps, st)
    # what the layer drew: the seed first, then (when regularising) the t1 draw, both from st["rng"]
    rng, seed = _replica(st)
    r01 = f32(rng.random(dtype=f32)) if mode != "none" else f32(0)
    t0, t2 = f32(0.0), f32(1.0)
    t1_or_rand = f32(r01 * (t2 - t0) + t0) if mode == "unbiased" else r01
    assert rng.bit_generator.state == st2["rng"].bit_generator.state
    assert st2["rng"].bit_generator.state != st["rng"].bit_generator.state
    h = node.handle()
    hh = f32((t2 - t0) / f32(nfine))
    W = h.draw_noise(seed, 0, nfine, B, f32(np.sqrt(hh)), True).cpu().numpy()
    z = h.draw_noise(seed, 1, 1, B, 1.0, False)[0].cpu().numpy()
    drift = oracle.MlpField(D, H, pd, time_dep=False, act="tanh", nthreads=4)
    p2 = np.concatenate([np.eye(D, dtype=f32).ravel(), np.zeros(D, f32), pg])
    diff = oracle.MlpField(D, D, p2, time_dep=False, act="identity", nthreads=4)
    ref = oracle.sde_node_forward(drift, diff, x, W, 0.0, 1.0, tol, tol, mode=mode, t1_or_rand=float(t1_or_rand), z_local=z, saveat=(),
                                  save_start=-1, maxiters=node.maxiters)
    got = dict(stats=sol.stats, nfe_drift=st2["nfe_drift"], nfe_diffusion=st2["nfe_diffusion"], t=np.array(sol.t, f32),
               reg_val=st2["reg_val"], u=torch.stack(sol.u), t1=ref["t1"])
    what = f"device noise D={D} H={H} B={B} tol={tol} nfine={nfine} {mode}"
    _check_forward(got, ref, what)
    assert (st2["reg_val"] == 0) == (mode == "none")
    sol_b, st2_b = node(torch.from_numpy(x).cuda(), ps, st)      # same st: the same bits
    assert all(torch.equal(a, b) for a, b in zip(sol.u, sol_b.u)) and st2_b["reg_val"] == st2["reg_val"]
    print(f"{what}: accepted {ref['naccept']}, rejected {ref['nreject']}, reg_val {ref['reg_val']:.4g}")


@pytest.mark.parametrize("D,H,B,tol,nfine,mode", [(32, 64, 512, 0.14, 256, "unbiased"), (32, 64, 64, 0.14, 64, "biased"),
                                                  (72, 32, 6, 0.1, 32, "unbiased")])
def test_device_noise_pullback_equals_the_explicit_arrays(gpu_pkg, D, H, B, tol, nfine, mode):
    P = gpu_pkg
    pd, pg = _params(D, H, 21)
    ps = dict(drift=(pd * f32(1.5)).astype(f32), diffusion=pg)
    xd = torch.from_numpy(np.random.default_rng(5).standard_normal((B, D)).astype(f32)).cuda()
    node = _layer(P, D, H, tol, nfine, regularize=mode)
    st = node.initialstates(np.random.default_rng(3))
    sol, _ = node(xd, ps, st)
    du = torch.from_numpy(np.random.default_rng(9).standard_normal((len(sol.u), B, D)).astype(f32)).cuda()
    dx, dps, info = node.pullback_series(xd, ps, st, du, w_reg=2.0)
    _, seed = _replica(st)
    h = node.handle()
    W = h.draw_noise(seed, 0, nfine, B, f32(np.sqrt(f32(f32(1.0) / f32(nfine)))), True)
    z = h.draw_noise(seed, 1, 1, B, 1.0, False)[0]
    dx_e, dps_e, info_e = node.pullback_series(xd, ps, st, du, w_reg=2.0, path=W, z_local=z)
    assert torch.equal(dx, dx_e) and torch.equal(dps["drift"], dps_e["drift"]) and torch.equal(dps["diffusion"], dps_e["diffusion"])
    assert info["st"]["reg_val"] == info_e["st"]["reg_val"] and torch.isfinite(dx).all() and (dx != 0).any()
    dx1, dps1, _ = node.pullback(xd, ps, st, du[-1], w_reg=2.0)          # pullback = pullback_series with du on sol.u[end]
    dx1_e, dps1_e, _ = node.pullback(xd, ps, st, du[-1], w_reg=2.0, noise=W)
    assert torch.equal(dx1, dx1_e) and torch.equal(dps1["drift"], dps1_e["drift"]) and torch.equal(dps1["diffusion"], dps1_e["diffusion"])


@pytest.mark.parametrize("solver", ["EulerHeun", "RKMil"])
def test_fixed_grid_device_noise_equals_the_explicit_increments(gpu_pkg, solver):
    P = gpu_pkg
    D, H, B, n = 32, 64, 40, 8
    pd, pg = _params(D, H, 4)
    ps = dict(drift=pd, diffusion=pg)
    xd = torch.from_numpy(np.random.default_rng(6).standard_normal((B, D)).astype(f32)).cuda()
    node = _layer(P, D, H, 0.14, solver=solver, adaptive=False, nsteps=n, regularize="unbiased")
    st = node.initialstates(np.random.default_rng(1))
    sol, st2 = node(xd, ps, st)
    rng, seed = _replica(st)
    rng.random(dtype=f32)
    assert rng.bit_generator.state == st2["rng"].bit_generator.state
    dt = f32((f32(1.0) - f32(0.0)) / f32(n))
    noise = node.handle().draw_noise(seed, 2, n + 1, B, f32(np.sqrt(dt)), False)
    sol_e, st2_e = node(xd, ps, st, noise=noise)
    assert torch.equal(sol.u[-1], sol_e.u[-1]) and st2["reg_val"] == st2_e["reg_val"] and st2["reg_val"] != 0
    du = torch.from_numpy(np.random.default_rng(8).standard_normal((B, D)).astype(f32)).cuda()
    dx, dps, _ = node.pullback(xd, ps, st, du, w_reg=2.0)
    dx_e, dps_e, _ = node.pullback(xd, ps, st, du, w_reg=2.0, noise=noise)
    assert torch.equal(dx, dx_e) and torch.equal(dps["drift"], dps_e["drift"]) and torch.equal(dps["diffusion"], dps_e["diffusion"])
    assert torch.isfinite(dx).all() and (dx != 0).any()


def test_sri_device_noise_equals_the_step_loop(gpu_pkg):
    """the layer draws dZ from its noise source even when noise= is given, so the reference is the handle-level loop of
    sri_step / sri_step_backward over the device dW (stream 2) and dZ (stream 3) — the tableau of the existing SRI tests"""
    P = gpu_pkg
    from localregneuralde_jl_amd import _lib as L
    D, H, B, n = 32, 64, 16, 4
    trng = np.random.default_rng(41)
    tab = [float(f32(trng.uniform(-0.6, 0.9))) for _ in L.SRI_FIELDS]
    pd, pg = _params(D, H, 6)
    ps = dict(drift=pd, diffusion=pg)
    xd = torch.from_numpy(np.random.default_rng(2).standard_normal((B, D)).astype(f32)).cuda()
    node = _layer(P, D, H, 0.14, solver="SRI", tableau=tab, nsteps=n, regularize="unbiased")
    st = node.initialstates(np.random.default_rng(0))
    sol, st2 = node(xd, ps, st)
    rng, seed = _replica(st)
    h = node.handle()
    t0, t2 = f32(0.0), f32(1.0)
    dt = f32((t2 - t0) / f32(n))
    dW = h.draw_noise(seed, 2, n + 1, B, f32(np.sqrt(dt)), False)
    dZ = h.draw_noise(seed, 3, n + 1, B, f32(np.sqrt(dt)), False)
    us, u = [], xd
    for i in range(n):
        u = h.sri_step(tab, u, dW[i].contiguous(), dZ[i].contiguous(), f32(t0 + f32(i) * dt), dt, 0.14, 0.14, node.delta)["u"]
        us.append(u)
    assert torch.equal(sol.u[-1], us[-1])
    # the local step (sde.py's unbiased branch, restated)
    ts = [f32(t0 + f32(i + 1) * dt) if i + 1 < n else t2 for i in range(n)]
    t1 = f32(rng.random(dtype=f32) * (t2 - t0) + t0)
    j = min(int((t1 - t0) / dt), n - 1)
    ta, ua = (t0, xd) if j == 0 else (ts[j - 1], us[j - 1])
    th = f32((t1 - ta) / (ts[j] - ta))
    u1 = (ua + th * (us[j] - ua)).contiguous()
    r = h.sri_step(tab, u1, dW[n].contiguous(), dZ[n].contiguous(), t1, f32(min(dt, f32(t2 - t1))), 0.14, 0.14, node.delta)
    assert r["reg_val"] == st2["reg_val"] != 0
    du = torch.from_numpy(np.random.default_rng(8).standard_normal((B, D)).astype(f32)).cuda()
    dx, dps, _ = node.pullback(xd, ps, st, du, w_reg=0.0)
    ub, dpf, dpg = du, None, None
    for i in range(n - 1, -1, -1):
        rb = h.sri_step_backward(tab, xd if i == 0 else us[i - 1], dW[i].contiguous(), dZ[i].contiguous(), f32(t0 + f32(i) * dt), dt,
                                 0.14, 0.14, node.delta, du_new=ub, dp_drift=dpf, dp_diff=dpg)
        ub, dpf, dpg = rb["dx"], rb["dp_drift"], rb["dp_diff"]
    assert torch.equal(dx, ub) and torch.equal(dps["drift"], dpf) and torch.equal(dps["diffusion"], dpg)


def test_bad_arguments_return_badarg_with_a_message(gpu_pkg):
    from localregneuralde_jl_amd import _lib as L
    h = _handle(gpu_pkg, 4)
    out = torch.empty((9, 3, 4), dtype=torch.float32, device="cuda")
    ptr = C.c_void_p(out.data_ptr())
    for args, word in (((-1, 3, 1.0, 1, ptr), "nsteps"), ((8, 0, 1.0, 1, ptr), "batch"), ((8, 3, 1.0, 1, None), "null"),
                       ((8, 3, float("inf"), 0, ptr), "finite"), ((8, 3, float("nan"), 0, ptr), "finite"), ((8, 3, 1.0, 2, ptr), "cumulative")):
        assert L.lib.lrnde_sde_draw_noise(h._h, SEED, 0, *args) == 4, args
        assert word in L.lib.lrnde_sde_last_error(h._h).decode(), (args, L.lib.lrnde_sde_last_error(h._h))
    with pytest.raises(gpu_pkg.LrndeError):
        h.draw_noise(SEED, 0, 8, 3, float("nan"), True)
    with pytest.raises(ValueError):
        gpu_pkg.NeuralDSDE(gpu_pkg.Chain(gpu_pkg.Dense(4, 8), gpu_pkg.Dense(8, 4)), gpu_pkg.Dense(4, 4), noise_source="gpu")
    assert L.lib.lrnde_sde_draw_noise(None, SEED, 0, 8, 3, 1.0, 1, ptr) == 4
