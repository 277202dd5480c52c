"""The Latent-ODE kernels (csrc/lrnde_latent.hpp) on the GPU.

  encoder forward: bit for bit the float32 host restatement (tests/latent_host.cpp), independent of B and of the tile;
  encoder pullback, decode + loss: against float64 autograd of tests/latent_np.py at
      max(1e-5, 4 x the distance of its float32 torch run from its float64 run), per block, relative to the block's norm;
  end to end (run_latent_training_step, tolerance 1e-6, 4 saved times): every gradient block within 3e-4 of float64
      autograd through encoder -> RK4 (200 steps; its own error: tests/test_host_latent.py) -> decoder -> loss — what
      tests/test_gpu_chain_adjoint.py holds the chain's series pullback to at that tolerance.

Shapes: tiny 3/5/3/2 (F = 7) with T = 4 and B in {1, 9, 13} (one tile short, 8+1, 8+5), T = 1, and the experiment's 37/40/50/20
with T = 49 at B = 12.  Every batch has a step unobserved in all columns and (B > 1) a column unobserved at every step; the
loss masks have an observed entry in every column."""
import ctypes

import numpy as np
import pytest
import torch

import latent_cases as LC

pytestmark = pytest.mark.gpu

CASES = [(LC.TINY, 1, 4), (LC.TINY, 9, 4), (LC.TINY, 13, 4), (LC.TINY, 9, 1), (LC.PHYSIONET, 12, 49)]
_REF = {}


def case(dims, B, T):
    """inputs and the two torch runs of a case, computed once"""
    key = (dims, B, T)
    if key not in _REF:
        flat = LC.make_params(dims, seed=21)
        data, mask, dt = LC.make_batch(dims, B, T, seed=22)
        x = LC.x_of(data, mask, dt)
        rng = np.random.default_rng(23)
        eps = rng.standard_normal((B, dims[3])).astype(np.float32)
        cots = [rng.standard_normal((B, dims[3])).astype(np.float32) for _ in range(3)]
        _REF[key] = dict(flat=flat, x=x, eps=eps, cots=cots,
                         r64=LC.encoder_reference(dims, flat, x, eps, cots, torch.float64),
                         r32=LC.encoder_reference(dims, flat, x, eps, cots, torch.float32))
    return _REF[key]


def handle(P, dims, flat):
    h = P.LatentHandle(*dims)
    h.set_params(torch.from_numpy(flat))
    return h


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def encode(h, c, training=True, x=None, eps=None):
    out = h.encode(dev(c["x"] if x is None else x), dev(c["eps"] if eps is None else eps) if training else None, training=training)
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("dims,B,T", CASES)
@pytest.mark.parametrize("training", [True, False])
def test_encoder_forward_is_the_host_restatements_bits(gpu_pkg, dims, B, T, training):
    c = case(dims, B, T)
    h = handle(gpu_pkg, dims, c["flat"])
    got = encode(h, c, training)
    ref = LC.run_host(dims, c["flat"], c["x"], c["eps"], training)
    for k in ("y", "mu", "logvar", "z0"):
        assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (k, float(np.abs(got[k] - ref[k]).max()))
    again = encode(h, c, training)
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), k
    if B > 1:   # the column that is never observed
        L = dims[2]
        assert np.array_equal(got["y"][B - 1], np.concatenate([np.zeros(L, np.float32), np.ones(L, np.float32)]))
    assert h.last_launches()["encode"] == 1


def test_a_column_does_not_depend_on_the_batch_or_its_tile(gpu_pkg):
    c = case(LC.TINY, 13, 4)
    h = handle(gpu_pkg, LC.TINY, c["flat"])
    full = encode(h, c)
    part = encode(h, c, x=c["x"][8:13], eps=c["eps"][8:13])      # columns 8..12: tile 1 of the first run, tile 0 of this one
    for k in full:
        assert np.array_equal(full[k][8:13].view(np.uint32), part[k].view(np.uint32)), k


@pytest.mark.parametrize("dims,B,T", CASES)
def test_encoder_pullback_against_float64_autograd(gpu_pkg, dims, B, T):
    c = case(dims, B, T)
    h = handle(gpu_pkg, dims, c["flat"])
    xd, cz, cm, cl = dev(c["x"]), *(dev(a) for a in c["cots"])

    def run():
        h.encode(xd, dev(c["eps"]), training=True)
        bw = h.encode_backward(xd, dz0=cz, dmu=cm, dlogvar=cl)
        return bw["dp"].cpu().numpy(), bw["dx"].cpu().numpy()

    dp, dx = run()
    dp2, dx2 = run()
    assert np.array_equal(dp.view(np.uint32), dp2.view(np.uint32)) and np.array_equal(dx.view(np.uint32), dx2.view(np.uint32))
    assert h.last_launches() == dict(encode=1, backward=2)    # the reverse walk + the sum of its per-workgroup partials
    npar = dp.size
    g64, g32 = c["r64"]["dp"][:npar], c["r32"]["dp"][:npar]
    assert np.all(c["r64"]["dp"][npar:] == 0)                 # gen_to_data is not part of the encoder
    full = lambda g: LC.split_blocks(np.concatenate([g, np.zeros(LC.param_count(dims) - npar, g.dtype)]), dims)
    b64, b32, bg = full(g64), full(g32), full(dp)
    for k in ("update_gate", "reset_gate", "new_state", "rec_to_gen"):
        bnd, e = LC.bound(b32[k], b64[k]), LC.rel(bg[k], b64[k])
        print(f"{dims} B={B} T={T} {k}: gpu {e:.2e} torch-f32 {LC.rel(b32[k], b64[k]):.2e} bound {bnd:.2e}")
        assert e <= bnd, (k, e, bnd)
    bnd, e = LC.bound(c["r32"]["dx"], c["r64"]["dx"]), LC.rel(dx, c["r64"]["dx"])
    print(f"{dims} B={B} T={T} dx: gpu {e:.2e} bound {bnd:.2e}")
    assert e <= bnd
    # latent_ode.jl:37: the mean half of new_state's second layer is dead; its cotangent is exactly zero
    I, H, L, N = dims
    K = 2 * L + 2 * I + 1
    g = bg["new_state"]
    W2 = g[H * K + H:H * K + H + 2 * L * H].reshape(H, 2 * L).T
    assert np.all(W2[:L] == 0) and np.all(g[H * K + H + 2 * L * H:][:L] == 0) and np.any(W2[L:] != 0)


def test_encoder_pullback_in_test_mode(gpu_pkg):
    dims, B, T = LC.TINY, 9, 4
    c = case(dims, B, T)
    h = handle(gpu_pkg, dims, c["flat"])
    r64 = LC.encoder_reference(dims, c["flat"], c["x"], c["eps"], c["cots"], torch.float64, training=False)
    r32 = LC.encoder_reference(dims, c["flat"], c["x"], c["eps"], c["cots"], torch.float32, training=False)
    xd = dev(c["x"])
    h.encode(xd, None, training=False)
    bw = h.encode_backward(xd, dz0=dev(c["cots"][0]), dmu=dev(c["cots"][1]), dlogvar=dev(c["cots"][2]))
    dp = bw["dp"].cpu().numpy()
    assert LC.rel(dp, r64["dp"][:dp.size]) <= LC.bound(r32["dp"][:dp.size], r64["dp"][:dp.size])
    assert LC.rel(bw["dx"].cpu().numpy(), r64["dx"]) <= LC.bound(r32["dx"], r64["dx"])


def test_recurrence_layer_alone(gpu_pkg):
    P = gpu_pkg
    dims, B, T = LC.TINY, 9, 4
    I, H, L, N = dims
    c = case(dims, B, T)
    rec = P.Recurrence(P.LatentGRUCell(I, H, L))
    ncell = rec.cell.param_count()
    ps = torch.from_numpy(c["flat"][:ncell]).cuda()
    y, _ = rec(dev(c["x"]), ps, {})
    assert np.array_equal(y.cpu().numpy().view(np.uint32), LC.run_host(dims, c["flat"], c["x"], c["eps"])["y"].view(np.uint32))
    dy = np.random.default_rng(31).standard_normal((B, 2 * L)).astype(np.float32)
    dx, dps = rec.pullback(dev(c["x"]), ps, {}, dev(dy))
    grads = {}
    for dt in (torch.float64, torch.float32):
        p = torch.tensor(c["flat"], dtype=dt, requires_grad=True)
        xt = torch.tensor(c["x"], dtype=dt, requires_grad=True)
        import latent_np as LN
        (LN.recurrence(LN.unflatten(p, *dims), L, xt) * torch.tensor(dy, dtype=dt)).sum().backward()
        grads[dt] = (p.grad.numpy()[:ncell], xt.grad.numpy())
    assert LC.rel(dps.cpu().numpy(), grads[torch.float64][0]) <= LC.bound(grads[torch.float32][0], grads[torch.float64][0])
    assert LC.rel(dx.cpu().numpy(), grads[torch.float64][1]) <= LC.bound(grads[torch.float32][1], grads[torch.float64][1])


@pytest.mark.parametrize("dims,B,T", [(LC.TINY, 1, 4), (LC.TINY, 13, 4), (LC.TINY, 9, 1), (LC.PHYSIONET, 12, 49)])
def test_decode_and_loss_against_float64(gpu_pkg, dims, B, T):
    I, H, L, N = dims
    flat = LC.make_params(dims, seed=41)
    rng = np.random.default_rng(42)
    series = rng.standard_normal((T, B, N)).astype(np.float32)
    data = rng.standard_normal((B, T, I)).astype(np.float32)
    mask = LC.loss_mask(dims, B, T, seed=43)
    mu, lv = (0.5 * rng.standard_normal((B, N))).astype(np.float32), (0.5 * rng.standard_normal((B, N))).astype(np.float32)
    w_kl = 0.7
    r64 = LC.decode_reference(dims, flat, series, data, mask, mu, lv, w_kl, torch.float64)
    r32 = LC.decode_reference(dims, flat, series, data, mask, mu, lv, w_kl, torch.float32)
    h = handle(gpu_pkg, dims, flat)
    args = (dev(series), dev(data), dev(mask), dev(mu), dev(lv), w_kl)
    got = h.decode_loss(*args)
    again = h.decode_loss(*args)
    for k in ("ll", "kl", "dseries", "dmu", "dlogvar", "dpg"):
        g = got[k].cpu().numpy()
        assert np.array_equal(g.view(np.uint32), again[k].cpu().numpy().view(np.uint32)), k
        bnd, e = LC.bound(r32[k], r64[k]), LC.rel(g, r64[k])
        print(f"{dims} B={B} T={T} {k}: gpu {e:.2e} torch-f32 {LC.rel(r32[k], r64[k]):.2e} bound {bnd:.2e}")
        assert e <= bnd, (k, e, bnd)
    bnd = max(1e-5, 4 * abs(r32["loss"] - r64["loss"]) / abs(r64["loss"]))
    e = abs(float(got["loss"]) - r64["loss"]) / abs(r64["loss"])
    print(f"loss: gpu {e:.2e} bound {bnd:.2e}")
    assert e <= bnd and got["loss"] == again["loss"]
    assert abs(float(got["neg_log_likelihood"]) + r64["ll"].mean()) <= bnd * abs(r64["ll"].mean())
    assert abs(float(got["kl_div"]) - r64["kl"].mean()) <= max(1e-5, bnd) * abs(r64["kl"].mean())
    pred = h.predict(dev(series)).cpu().numpy()
    assert LC.rel(pred, r64["pred"]) <= LC.bound(r32["pred"], r64["pred"])


def e2e_setup(P, regularize, B=9):
    dims, T = LC.TINY, 4
    times = [0.25, 0.5, 0.75, 1.0]
    model = P.construct_time_series(*dims, saveat=times, regularize=regularize, abstol=1e-6, reltol=1e-6, maxiters=10000)
    flat, node = LC.make_params(dims, seed=11), LC.make_node_params(dims, seed=12)
    data, mask, dt = LC.make_batch(dims, B, T, seed=13, unobserved_column=False)   # (the loss divides by the column's mask sum)
    mask[:, 0, 0] = 1
    ps = dict(latent=dev(flat), neural_ode=dev(node))
    st = model.initialstates(np.random.default_rng(5))
    return dims, times, model, flat, node, (data, mask, dt), ps, st


def test_end_to_end_training_step_against_float64(gpu_pkg):
    P = gpu_pkg
    dims, times, model, flat, node, (data, mask, dt), ps, st = e2e_setup(P, "none")
    B = data.shape[0]
    eps, _ = model.reparam.draw(st["reparam"], B, dims[3])
    w_kl = 0.5
    loss, st_, stats, grads, tm = P.run_latent_training_step(model, ps, st, (dev(data), dev(mask), dev(dt)), (0.0, w_kl))
    ref = LC.model_reference(dims, flat, node, LC.x_of(data, mask, dt), eps, data, mask, times, w_kl, 200)
    print(f"loss gpu {float(loss):.6e} float64 {ref['loss']:.6e}  times {tm['fwd_time']:.4f} {tm['bwd_time']:.4f}")
    assert abs(float(loss) - ref["loss"]) <= 3e-4 * abs(ref["loss"])
    g, r = LC.split_blocks(grads["latent"].cpu().numpy(), dims), LC.split_blocks(ref["dp"], dims)
    errs = {k: LC.rel(g[k], r[k]) for k in LC.BLOCKS}
    errs["neural_ode"] = LC.rel(grads["neural_ode"].cpu().numpy(), ref["dnode"])
    print("relative to each block's norm:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert max(errs.values()) <= 3e-4, errs
    assert set(stats) == {"neg_log_likelihood", "kl_div", "loss", "nfe", "reg_val"} and stats["reg_val"] == 0 and stats["nfe"] > 0
    assert {"fwd_time", "bwd_time", "opt_time"} <= set(tm)
    assert st_["reparam"]["mu0"].shape == (B, dims[3]) and st_["neural_ode"]["nfe"] == stats["nfe"]
    # the model's own forward and the loss function agree with the training step
    y, st_f = model(dev(LC.x_of(data, mask, dt)), ps, st)
    assert tuple(y.shape) == (B, 4, dims[0]) and LC.rel(y.cpu().numpy(), ref["pred"]) <= 3e-4
    loss2, _, stats2 = P.latent_ode_loss(model, ps, st, (dev(data), dev(mask), dev(dt)), (0.0, w_kl))
    assert abs(float(loss2) - float(loss)) <= 1e-5 * abs(float(loss))
    assert torch.equal(st_f["reparam"]["mu0"], st_["reparam"]["mu0"])


def test_regularised_training_step_reports_the_layers_reg_val(gpu_pkg):
    P = gpu_pkg
    dims, times, model, flat, node, (data, mask, dt), ps, st = e2e_setup(P, "unbiased")
    B = data.shape[0]
    loss, st_, stats, grads, _ = P.run_latent_training_step(model, ps, st, (dev(data), dev(mask), dev(dt)), (2.0, 0.5))
    eps, _ = model.reparam.draw(st["reparam"], B, dims[3])
    h = handle(P, dims, flat)
    z0 = h.encode(dev(LC.x_of(data, mask, dt)), dev(eps))["z0"]
    twin = P.NeuralODE(model.gen_dynamics, field="dense_chain", saveat=times, save_start=False, regularize="unbiased", abstol=1e-6,
                       reltol=1e-6, maxiters=10000)   # the start time is not in saveat: 4 saved states, as the model's own layer
    _, _, info = twin.pullback(z0, ps["neural_ode"], st["neural_ode"], torch.zeros((4, B, dims[3]), device="cuda"), w_reg=2.0)
    assert stats["reg_val"] == info["reg_val"] and stats["nfe"] == info["nfe"] and stats["reg_val"] > 0
    assert np.isfinite(float(loss)) and all(bool(torch.isfinite(v).all()) for v in grads.values())


def test_unsupported_shape_is_refused_with_a_message(gpu_pkg):
    from localregneuralde_jl_amd import _lib
    with pytest.raises(NotImplementedError, match="hidden_dims"):
        gpu_pkg.LatentHandle(37, 64, 50, 20)          # 3 * 64 rows side by side > 128
    with pytest.raises(NotImplementedError, match="LDS"):
        gpu_pkg.LatentHandle(37, 40, 120, 20)         # the weight image does not fit a CU's LDS
    hp = ctypes.c_void_p()
    d = _lib.LatentDesc(37, 64, 50, 20)
    assert _lib.lib.lrnde_latent_create(ctypes.byref(hp), ctypes.byref(d), 0, None) == 8 and not hp.value
    assert b"hidden_dims" in _lib.lib.lrnde_latent_last_error(None)
    gpu_pkg.LatentHandle(*LC.PHYSIONET)                # the experiment's shape is supported


def test_record_generation_and_stale_record(gpu_pkg):
    P = gpu_pkg
    c = case(LC.TINY, 9, 4)
    h = handle(P, LC.TINY, c["flat"])
    xd, eps = dev(c["x"]), dev(c["eps"])
    assert h.record_generation() == 0
    h.encode(xd, eps)
    assert h.record_generation() == 1
    h.encode(xd, eps)
    assert h.record_generation() == 2
    h.encode_backward(xd, dz0=eps)
    assert h.record_generation() == 0                 # consumed
    with pytest.raises(P.LrndeError, match="no recorded encode"):
        h.encode_backward(xd, dz0=eps)
    h.encode(xd, eps)
    h.set_params(torch.from_numpy(c["flat"]))         # new parameters: the record is of the old ones
    assert h.record_generation() == 0
    with pytest.raises(P.LrndeError):
        h.encode_backward(xd, dz0=eps)
    h.encode(xd, eps)
    with pytest.raises(P.LrndeError, match="record is of B = 9"):
        h.encode_backward(xd[:5].contiguous(), dz0=eps[:5].contiguous())
