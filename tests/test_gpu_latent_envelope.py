"""The Latent-ODE kernels (csrc/lrnde_latent.hpp) on their own loop, tile and size edges: LC.ENVELOPE.

  forward: bit for bit the float32 host restatement (tests/latent_host.cpp), at every case, in both modes;
  pullback: every LC.sub_blocks entry of dp and every LC.dx_rows entry of dx against float64 autograd at
      max(1e-5, 4 x the distance of the float32 torch run), relative to that SUB-BLOCK's float64 norm
      (tests/test_host_latent.py holds the float32 distance below 2.5e-6, so each bound is the floor 1e-5);
  exact zeros: dx where a column is unobserved, whether its tile skipped the step or ran it; the dead rows of new_state;
  the T limits, the create limit, the decode kernel's LDS limit; two handles of different sizes interleaved;
  end to end at the experiment's shape against float64 autograd at the 3e-4 bar of tests/test_gpu_latent.py.

Every batch is LC.mixed_batch: the last column is never observed, one step is unobserved everywhere, and with two full
tiles each tile skips a step that the other runs.

Measured on the MI355X (ROCm 7.2.0; printed by the tests): worst sub-block of a case 2.9e-7 .. 1.4e-6 (`long`,
update_gate.l2_b) against the bound 1e-5; t_fit(37/40/50/20) = 2221, the refusal at 2222 prints 163848 of 163840 bytes;
the interleaved handles return the bits of a handle run alone (this runtime does not enforce the kernel's dynamic-LDS
attribute below the device limit); end to end 4.0e-7 .. 1.5e-6 per gradient block against the bar 3e-4."""
import ctypes
import re

import numpy as np
import pytest
import torch

import latent_cases as LC
import test_gpu_latent as TG
from test_gpu_latent import dev, encode, handle

pytestmark = pytest.mark.gpu

KEYS = ("y", "mu", "logvar", "z0")


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def pullback(h, c, training=True, given=None, dy=None, want_dx=True):
    """encode, then encode_backward with the cotangents `given` (dz0, dmu, dlogvar; None: absent) and dy"""
    xd = dev(c["x"])
    cz, cm, cl = (None if a is None else dev(a) for a in (c["cots"] if given is None else given))
    h.encode(xd, dev(c["eps"]) if training else None, training=training)
    bw = h.encode_backward(xd, dz0=cz, dmu=cm, dlogvar=cl, want_dx=want_dx, dy=None if dy is None else dev(dy))
    return bw["dp"].cpu().numpy(), None if bw["dx"] is None else bw["dx"].cpu().numpy()


def check_sub_blocks(label, dims, dp, dx, r64, r32):
    """every sub-block within LC.bound of float64 relative to its own norm; a sub-block that is zero in float64 is zero here"""
    worst = (0.0, None)
    for (name, a, b), (_, e, twin, norm) in zip(LC.sub_blocks(dims) + LC.dx_rows(dims[0]), LC.sub_block_errors(dims, dp, dx, r64, r32)):
        bnd = max(1e-5, 4.0 * twin)
        print(f"{label} {name}: gpu {e:.2e} torch-f32 {twin:.2e} bound {bnd:.2e}")
        if norm == 0:
            got = dp[a:b] if not name.startswith("dx.") else dx[..., a:b]
            assert np.all(got == 0), (label, name)
        else:
            assert e <= bnd, (label, name, e, bnd)
        worst = max(worst, (e / bnd, name))
    print(f"{label}: worst sub-block {worst[1]} at {worst[0]:.3f} of its bound")


# ---- G1 ----
@pytest.mark.parametrize("name", LC.ENVELOPE_NAMES)
@pytest.mark.parametrize("training", [True, False])
def test_forward_is_the_host_restatements_bits(gpu_pkg, name, training):
    c = LC.envelope_case(name)
    dims, B = c["dims"], c["B"]
    h = handle(gpu_pkg, dims, c["flat"])
    got = encode(h, c, training)
    ref = LC.run_host(dims, c["flat"], c["x"], c["eps"], training)
    for k in KEYS:
        assert bits_equal(got[k], ref[k]), (k, float(np.abs(got[k] - ref[k]).max()))
    again = encode(h, c, training)
    for k in KEYS:
        assert bits_equal(got[k], again[k]), k
    assert h.last_launches()["encode"] == 1
    L = dims[2]
    never = ~LC.observed(c["x"], dims[0]).any(axis=1)
    assert never[B - 1]
    assert np.array_equal(got["y"][never], np.tile(np.concatenate([np.zeros(L, np.float32), np.ones(L, np.float32)]), (never.sum(), 1)))


# ---- G2 ----
def test_a_column_does_not_depend_on_its_tile_or_its_neighbours_masks(gpu_pkg):
    c = LC.envelope_case("lwide")
    h = handle(gpu_pkg, c["dims"], c["flat"])
    full = encode(h, c)
    part = encode(h, c, x=c["x"][8:16], eps=c["eps"][8:16])   # tile 1 of the first run alone: one full tile
    for k in KEYS:
        assert bits_equal(full[k][8:16], part[k]), k


# ---- G3, G4 ----
@pytest.mark.parametrize("name", LC.ENVELOPE_NAMES)
def test_pullback_per_sub_block_against_float64_autograd(gpu_pkg, name):
    c = LC.envelope_case(name)
    dims = c["dims"]
    h = handle(gpu_pkg, dims, c["flat"])
    dp, dx = pullback(h, c)
    dp2, dx2 = pullback(h, c)
    assert bits_equal(dp, dp2) and bits_equal(dx, dx2)
    assert h.last_launches() == dict(encode=1, backward=2)
    assert np.all(c["r64"]["dp"][dp.size:] == 0)              # gen_to_data is not part of the encoder
    check_sub_blocks(name, dims, dp, dx, c["r64"], c["r32"])
    # exact zeros: dx of a column at a step it is not observed at (its tile skipped the step, or ran it for a neighbour)
    obs = LC.observed(c["x"], dims[0])
    assert np.all(dx[~obs] == 0) and np.any(dx[obs] != 0)
    tile_ran = np.repeat(np.stack([obs[i:i + LC.LNB].any(axis=0) for i in range(0, c["B"], LC.LNB)]), LC.LNB, axis=0)[:c["B"]]
    assert (~obs & ~tile_ran).any()                           # a skipped step in every case ...
    if c["B"] % LC.LNB == 0:                                  # ... and, where the never-observed column has neighbours, a step run for them
        assert (~obs & tile_ran).any()
    assert np.all(dp[LC.dead_rows(dims)] == 0)                # latent_ode.jl:37


@pytest.mark.parametrize("dims,B,T", TG.CASES)
def test_pullback_per_sub_block_on_the_merged_cases(gpu_pkg, dims, B, T):
    c = TG.case(dims, B, T)
    h = handle(gpu_pkg, dims, c["flat"])
    dp, dx = pullback(h, c)
    check_sub_blocks(f"{dims} B={B} T={T}", dims, dp, dx, c["r64"], c["r32"])


# ---- G5 ----
@pytest.mark.parametrize("run", [r[0] for r in LC.OPTIONAL_RUNS])
def test_optional_cotangents_and_want_dx(gpu_pkg, run):
    c = LC.optional_case(run)
    dims = c["dims"]
    h = handle(gpu_pkg, dims, c["flat"])
    dp, dx = pullback(h, c, training=c["training"], given=c["given"], dy=c["dy"])
    check_sub_blocks(f"hmax run {run}", dims, dp, dx, c["r64"], c["r32"])
    dp_only, none = pullback(h, c, training=c["training"], given=c["given"], dy=c["dy"], want_dx=False)
    assert none is None and bits_equal(dp, dp_only)


# ---- G6 ----
def long_inputs(dims, B, T):
    if B > 1:
        return LC.envelope_inputs(dims, B, T)
    c = LC.envelope_inputs(dims, 2, T)                         # (a batch of one column has no never-observed column)
    return dict(c, B=1, x=np.ascontiguousarray(c["x"][:1]), eps=np.ascontiguousarray(c["eps"][:1]))


def assert_forward_bits(h, c, training=True):
    got = encode(h, c, training)
    ref = LC.run_host(c["dims"], c["flat"], c["x"], c["eps"], training)
    for k in KEYS:
        assert bits_equal(got[k], ref[k]), (k, float(np.abs(got[k] - ref[k]).max()))


@pytest.mark.parametrize("dims,B", [(LC.TINY, 9), (LC.PHYSIONET, 1)])
def test_the_largest_T_and_the_first_refused(gpu_pkg, dims, B):
    tf = LC.t_fit(dims)
    c = long_inputs(dims, B, tf)
    h = handle(gpu_pkg, dims, c["flat"])
    assert_forward_bits(h, c)
    assert h.last_launches()["encode"] == 1
    over = long_inputs(dims, B, tf + 1)
    with pytest.raises(NotImplementedError, match=f"T = {tf + 1}") as ei:
        h.encode(dev(over["x"]), dev(over["eps"]))
    m = re.search(r"\((\d+) of (\d+) bytes\)", str(ei.value))
    print(f"{dims}: t_fit {tf}; refusal: {ei.value}")
    assert m and int(m.group(1)) == LC.lat_smem_bytes(dims, True, tf + 1) and int(m.group(2)) == LC.LAT_MAX_LDS
    if dims == LC.PHYSIONET:   # the LDS arm: the last accepted fits, the first refused does not
        assert LC.lat_smem_bytes(dims, True, tf) <= LC.LAT_MAX_LDS < int(m.group(1)) and tf < LC.LAT_MAX_T
    else:                      # the LAT_MAX_T arm
        assert tf == LC.LAT_MAX_T and int(m.group(1)) <= LC.LAT_MAX_LDS
    assert_forward_bits(h, long_inputs(dims, B, 4))           # the refusal left a usable handle


# ---- G7 ----
def test_hidden_dims_limit_is_42(gpu_pkg):
    from localregneuralde_jl_amd import _lib
    with pytest.raises(NotImplementedError, match="hidden_dims"):
        gpu_pkg.LatentHandle(3, 43, 4, 2)                     # 129 rows side by side
    hp = ctypes.c_void_p()
    d = _lib.LatentDesc(3, 43, 4, 2)
    assert _lib.lib.lrnde_latent_create(ctypes.byref(hp), ctypes.byref(d), 0, None) == 8 and not hp.value
    assert b"hidden_dims = 43" in _lib.lib.lrnde_latent_last_error(None)
    gpu_pkg.LatentHandle(3, 42, 4, 2)


# ---- G8 ----
def decode_inputs(dims, B, T):
    I, H, L, N = dims
    rng = np.random.default_rng(42)
    series = rng.standard_normal((T, B, N)).astype(np.float32)
    data = rng.standard_normal((B, T, I)).astype(np.float32)
    mask = LC.loss_mask(dims, B, T, seed=43)
    mu, lv = (0.5 * rng.standard_normal((B, N))).astype(np.float32), (0.5 * rng.standard_normal((B, N))).astype(np.float32)
    return LC.make_params(dims, seed=41), series, data, mask, mu, lv, 0.7


@pytest.mark.parametrize("dims,B,T", [((128, 1, 1, 115), 3, 2), (LC.ENVELOPE[4][1], 3, 3), (LC.ENVELOPE[0][1], 3, 3)])
def test_decode_and_loss_widths_against_float64(gpu_pkg, dims, B, T):
    """(128, 1, 1, 115): gen_to_data's 14 848 floats make the decode kernel's LDS exactly 60 KiB, the last accepted size;
    N = 70 (`nwider`) and every width 1 (`min`)"""
    flat, series, data, mask, mu, lv, w_kl = decode_inputs(dims, B, T)
    if dims[0] == 128:
        assert 8 * 256 + 4 * (dims[0] * dims[3] + dims[0]) == 60 * 1024
    r64 = LC.decode_reference(dims, flat, series, data, mask, mu, lv, w_kl, torch.float64)
    r32 = LC.decode_reference(dims, flat, series, data, mask, mu, lv, w_kl, torch.float32)
    h = handle(gpu_pkg, dims, flat)
    args = (dev(series), dev(data), dev(mask), dev(mu), dev(lv), w_kl)
    got = h.decode_loss(*args)
    for k in ("ll", "kl", "dseries", "dmu", "dlogvar", "dpg"):
        g = got[k].cpu().numpy()
        bnd, e = LC.bound(r32[k], r64[k]), LC.rel(g, r64[k])
        print(f"{dims} B={B} T={T} {k}: gpu {e:.2e} torch-f32 {LC.rel(r32[k], r64[k]):.2e} bound {bnd:.2e}")
        assert e <= bnd, (k, e, bnd)
    bnd = max(1e-5, 4 * abs(r32["loss"] - r64["loss"]) / abs(r64["loss"]))
    e = abs(float(got["loss"]) - r64["loss"]) / abs(r64["loss"])
    print(f"loss: gpu {e:.2e} bound {bnd:.2e}")
    assert e <= bnd
    assert abs(float(got["neg_log_likelihood"]) + r64["ll"].mean()) <= bnd * abs(r64["ll"].mean())
    assert abs(float(got["kl_div"]) - r64["kl"].mean()) <= max(1e-5, bnd) * abs(r64["kl"].mean())
    pred = h.predict(dev(series)).cpu().numpy()
    assert LC.rel(pred, r64["pred"]) <= LC.bound(r32["pred"], r64["pred"])
    bare = h.decode_loss(*args, want_grads=False)
    assert set(bare) == {"ll", "kl", "loss", "neg_log_likelihood", "kl_div"}
    for k in ("ll", "kl"):
        assert bits_equal(got[k].cpu().numpy(), bare[k].cpu().numpy()), k
    for k in ("loss", "neg_log_likelihood", "kl_div"):
        assert got[k].tobytes() == bare[k].tobytes(), k


def test_decode_refuses_a_gen_to_data_past_its_lds(gpu_pkg):
    dims, B, T = (128, 1, 1, 116), 3, 2
    flat, series, data, mask, mu, lv, w_kl = decode_inputs(dims, B, T)
    h = handle(gpu_pkg, dims, flat)
    with pytest.raises(NotImplementedError, match="gen_to_data"):
        h.decode_loss(dev(series), dev(data), dev(mask), dev(mu), dev(lv), w_kl)
    r64 = LC.decode_reference(dims, flat, series, data, mask, mu, lv, w_kl, torch.float64)
    r32 = LC.decode_reference(dims, flat, series, data, mask, mu, lv, w_kl, torch.float32)
    pred = h.predict(dev(series)).cpu().numpy()                # no LDS in k_lat_pred: the handle still serves it
    assert LC.rel(pred, r64["pred"]) <= LC.bound(r32["pred"], r64["pred"])


# ---- G9 ----
def test_two_handles_of_different_sizes_interleaved(gpu_pkg):
    """the dynamic-LDS limit belongs to the kernel, not to a handle: a small handle's launch between two launches of a large
    one must not leave the large one with the small limit"""
    P = gpu_pkg
    big, small = LC.envelope_inputs(LC.PHYSIONET, 9, 4), LC.envelope_inputs(LC.TINY, 9, 4)

    def enc(h, c):
        return {k: v.cpu().numpy() for k, v in h.encode(dev(c["x"]), dev(c["eps"])).items()}

    def bwd(h, c):
        cz, cm, cl = (dev(a) for a in c["cots"])
        bw = h.encode_backward(dev(c["x"]), dz0=cz, dmu=cm, dlogvar=cl)
        return dict(dp=bw["dp"].cpu().numpy(), dx=bw["dx"].cpu().numpy())

    def same(got, ref):
        for k in ref:
            assert bits_equal(got[k], ref[k]), k

    alone = handle(P, LC.PHYSIONET, big["flat"])
    ref_f, ref_b = enc(alone, big), bwd(alone, big)
    alone.close()
    host = LC.run_host(LC.PHYSIONET, big["flat"], big["x"], big["eps"])
    same(ref_f, host)

    A = handle(P, LC.PHYSIONET, big["flat"])
    same(enc(A, big), ref_f)
    Bh = handle(P, LC.TINY, small["flat"])
    small_f, small_b = enc(Bh, small), bwd(Bh, small)
    same(enc(A, big), ref_f)                                   # A's encode after B's smaller one
    same(bwd(A, big), ref_b)
    # the other kernel: a fresh small handle's backward between A's encode and A's backward
    same(enc(A, big), ref_f)
    B2 = handle(P, LC.TINY, small["flat"])
    same(enc(B2, small), small_f)
    same(bwd(B2, small), small_b)
    same(bwd(A, big), ref_b)
    same(enc(Bh, small), small_f)
    same(bwd(Bh, small), small_b)


# ---- G10 ----
@pytest.mark.parametrize("sensealg", [None, "TrackerAdjoint"])
def test_end_to_end_at_the_experiments_shape(gpu_pkg, sensealg):
    P = gpu_pkg
    dims, B, times, w_kl = LC.PHYSIONET, 9, [0.25, 0.5, 0.75, 1.0], 0.5
    kw = dict(saveat=times, regularize="none", abstol=1e-6, reltol=1e-6, maxiters=10000)
    if sensealg:
        kw["sensealg"] = sensealg
    model = P.construct_time_series(*dims, **kw)
    st = model.initialstates(np.random.default_rng(5))
    eps, _ = model.reparam.draw(st["reparam"], B, dims[3])
    c = LC.e2e_physionet(200, True, eps=eps)
    ref = c["ref"]
    ps = dict(latent=dev(c["flat"]), neural_ode=dev(c["node"]))
    batch = (dev(c["data"]), dev(c["mask"]), dev(c["dt"]))
    loss, st_, stats, grads, tm = P.run_latent_training_step(model, ps, st, batch, (0.0, w_kl))
    assert model.neural_ode.handle().last_adjoint_info()["kind"] == (4 if sensealg else 2)
    e_loss = abs(float(loss) - ref["loss"]) / abs(ref["loss"])
    g, r = LC.split_blocks(grads["latent"].cpu().numpy(), dims), LC.split_blocks(ref["dp"], dims)
    errs = {k: LC.rel(g[k], r[k]) for k in LC.BLOCKS}
    errs["neural_ode"] = LC.rel(grads["neural_ode"].cpu().numpy(), ref["dnode"])
    print(f"sensealg={sensealg}: loss {e_loss:.2e}; relative to each block's norm:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert e_loss <= 3e-4
    assert max(errs.values()) <= 3e-4, errs
    # the evaluation forward: z0 = mu (common.jl:73-77), the layer in test mode
    st_eval = dict(st, reparam=dict(st["reparam"], training=False), neural_ode=dict(st["neural_ode"], training=False))
    x = LC.x_of(c["data"], c["mask"], c["dt"])
    y, st_e = model(dev(x), ps, st_eval)
    ref_eval = LC.e2e_physionet(200, False)["ref"]["pred"]
    e_y = LC.rel(y.cpu().numpy(), ref_eval)
    print(f"sensealg={sensealg}: evaluation forward {e_y:.2e} of the prediction's norm")
    assert tuple(y.shape) == (B, 4, dims[0]) and e_y <= 3e-4
    assert torch.equal(st_e["reparam"]["mu0"], st_e["reparam"]["logvar"])
    assert LC.rel(ref_eval, ref["pred"]) > 3e-4                # (the two modes differ by more than the bar: the check binds)
