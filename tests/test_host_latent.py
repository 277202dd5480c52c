"""Latent-ODE layers off the GPU: sigmoid_c of csrc/lrnde_math.hpp against float64, the float32 host restatement of the encoder
(tests/latent_host.cpp, the bits the GPU kernel must return) against the float64 transcription of the reference
(tests/latent_np.py), exact properties of that transcription, the parameter layout helpers, and the error of the end-to-end
yardstick itself.

Measured (printed by the tests):
  sigmoid_c max abs error 8.87e-08 (at x = 7.38) against tanhf_c's 7.75e-08 over the same sweep: bound 4 x 7.75e-08;
  host float32 restatement vs float64: 3e-08..2.7e-07 of each output's norm at both shapes, the torch float32 run the same:
  every bound is the rule's floor 1e-5;
  RK4 200 vs 400 steps, tiny shape: at most 1.1e-10 of a gradient block's norm (bound 1e-4)."""
import os
import subprocess
import textwrap

import numpy as np
import pytest
import torch

import latent_cases as LC
import latent_np as LN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGMOID_SRC = textwrap.dedent(r'''
    #include "lrnde_math.hpp"
    #include <cmath>
    #include <cstdio>
    #include <cstring>
    #include <cstdint>
    int main() {
      double es = 0.0, et = 0.0; float xs = 0.f, xt = 0.f; unsigned long long n = 0;
      auto check = [&](float x) {
        if (x != x || std::isinf(x)) return;
        const double s = 1.0 / (1.0 + std::exp(-(double)x)), t = std::tanh((double)x);
        const double ds = std::fabs((double)lrnde::sigmoid_c(x) - s), dt = std::fabs((double)lrnde::tanhf_c(x) - t);
        if (ds > es) { es = ds; xs = x; }
        if (dt > et) { et = dt; xt = x; }
        ++n;
      };
      for (uint64_t u = 0; u < (1ull << 32); u += 61) { uint32_t v = (uint32_t)u; float x; memcpy(&x, &v, 4); check(x); }
      // the pieces of sigmoid_c are those of expf_c(-x) (the clamps at 87) and, through sigmoid(x) = (1 + tanh(x/2)) / 2, of
      // tanhf_c (0.625, 9) and their doubles; 0 and 1 as in tests/test_math_header.py
      const float edges[] = {0.625f, 9.0f, 1.25f, 18.0f, 43.5f, 87.0f, 0.0f, 1.0f};
      for (float e : edges) {
        uint32_t v; memcpy(&v, &e, 4);
        for (int d = -20000; d <= 20000; ++d) { uint32_t w = v + (uint32_t)d; float x; memcpy(&x, &w, 4); check(x); check(-x); }
      }
      printf("checked %llu sigmoid %.9e at %a tanh %.9e at %a\n", n, es, xs, et, xt);
      return 0;
    }
''')


def test_sigmoid_c_against_float64(tmp_path):
    src = tmp_path / "s.cpp"
    src.write_text(SIGMOID_SRC)
    exe = tmp_path / "s"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "localregneuralde.jl_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    w = r.stdout.split()
    es, et = float(w[3]), float(w[7])
    assert et > 0
    assert es <= 4 * et, r.stdout


@pytest.mark.parametrize("dims,B,T,training", [(LC.TINY, 9, 4, True), (LC.TINY, 9, 4, False), (LC.TINY, 5, 1, True),
                                               (LC.PHYSIONET, 3, 49, True)])
def test_host_float32_restatement_against_float64(dims, B, T, training):
    flat = LC.make_params(dims, seed=1)
    data, mask, dt = LC.make_batch(dims, B, T, seed=2)
    x = LC.x_of(data, mask, dt)
    eps = np.random.default_rng(3).standard_normal((B, dims[3])).astype(np.float32)
    zero = [np.zeros((B, dims[3]), np.float32)] * 3
    r64 = LC.encoder_reference(dims, flat, x, eps, zero, torch.float64, training)
    r32 = LC.encoder_reference(dims, flat, x, eps, zero, torch.float32, training)
    got = LC.run_host(dims, flat, x, eps, training)
    for k in ("y", "mu", "logvar", "z0"):
        b = LC.bound(r32[k], r64[k])
        e = LC.rel(got[k], r64[k])
        print(f"{dims} B={B} T={T} training={training} {k}: host {e:.2e} torch-f32 {LC.rel(r32[k], r64[k]):.2e} bound {b:.2e}")
        assert e <= b, (k, e, b)
    if B > 1:   # the column that is never observed keeps the first call's carry, in the host program too
        L = dims[2]
        assert np.array_equal(got["y"][B - 1], np.concatenate([np.zeros(L, np.float32), np.ones(L, np.float32)]))


def test_exact_properties_of_the_float64_restatement():
    dims, B, T = LC.TINY, 5, 4
    I, H, L, N = dims
    flat = LC.make_params(dims, seed=4)
    data, mask, dt = LC.make_batch(dims, B, T, seed=5)
    x = LC.x_of(data, mask, dt)
    p = torch.tensor(flat, dtype=torch.float64, requires_grad=True)
    ps = LN.unflatten(p, *dims)
    y = LN.recurrence(ps, L, torch.tensor(x, dtype=torch.float64))
    # a column whose mask rows and dt are zero at every step: exactly the first call's carry
    assert torch.equal(y[B - 1].detach(), torch.cat([torch.zeros(L, dtype=torch.float64), torch.ones(L, dtype=torch.float64)]))
    assert not torch.equal(y[0].detach(), y[B - 1].detach())
    # T = 1 takes the first-call path: y_mean = 0, y_std = 1 (latent_ode.jl:19-23)
    x1 = torch.tensor(x[:, :1], dtype=torch.float64)
    y1 = LN.recurrence(ps, L, x1)
    y1b, _ = LN.gru_cell(ps, L, x1[:, 0], (torch.zeros((B, L), dtype=torch.float64), torch.ones((B, L), dtype=torch.float64)))
    assert torch.equal(y1, y1b)
    # latent_ode.jl:37: new_state's mean half never reaches an output, so its rows of layer 2 have an exactly zero gradient
    (y * torch.tensor(np.random.default_rng(6).standard_normal(tuple(y.shape)))).sum().backward()
    g = LC.split_blocks(p.grad.numpy(), dims)["new_state"]
    K = 2 * L + 2 * I + 1
    W2 = g[H * K + H:H * K + H + 2 * L * H].reshape(H, 2 * L).T    # (out, in)
    b2 = g[H * K + H + 2 * L * H:]
    assert np.all(W2[:L] == 0) and np.all(b2[:L] == 0)
    assert np.any(W2[L:] != 0) and np.any(b2[L:] != 0)


def test_parameter_split_and_join_round_trip():
    import lrnde_amd as P
    for dims in (LC.TINY, LC.PHYSIONET):
        flat = LC.make_params(dims, seed=7)
        blocks = P.split_latent_params(flat, dims)
        assert list(blocks) == list(LC.BLOCKS)
        assert {k: v.size for k, v in blocks.items()} == LN.block_sizes(*dims) == P.latent_block_sizes(*dims)
        assert np.array_equal(P.join_latent_params(blocks, dims), flat)
        t = torch.from_numpy(flat)
        assert torch.equal(P.join_latent_params(P.split_latent_params(t, dims), dims), t)
        for name, ref in LC.split_blocks(flat, dims).items():
            assert np.array_equal(blocks[name], ref)
    with pytest.raises(ValueError):
        P.split_latent_params(np.zeros(10, np.float32), LC.TINY)


def test_parameter_count_of_the_experiment():
    import ctypes
    import lrnde_amd as P
    from localregneuralde_jl_amd import _lib
    d = _lib.LatentDesc(37, 40, 50, 20)
    assert _lib.lib.lrnde_latent_param_count(ctypes.byref(d)) == 29320 + 7090 + 777
    s = P.latent_block_sizes(37, 40, 50, 20)
    assert s["update_gate"] + s["reset_gate"] + s["new_state"] == 29320 and s["rec_to_gen"] == 7090 and s["gen_to_data"] == 777
    assert LC.param_count(LC.PHYSIONET) == 29320 + 7090 + 777
    model = P.construct_time_series(saveat=[0.5, 1.0])
    ps = P.glorot_latent_params(model, seed=0)
    assert ps["latent"].size == 29320 + 7090 + 777 and ps["neural_ode"].size == 4 * (20 * 40 + 40 + 40 * 20 + 20)
    assert _lib.lib.lrnde_latent_param_count(ctypes.byref(_lib.LatentDesc(0, 40, 50, 20))) == 0


def test_the_series_has_one_state_per_saveat_time():
    """construct.jl:244-248 passes no save_start: DiffEq saves the start state only where tspan[1] is one of the saveat times,
    so y has the (B, T, I) of the data the loss compares it with"""
    import lrnde_amd as P
    assert P.construct_time_series(saveat=[0.5, 1.0]).neural_ode.kwargs["save_start"] is False
    assert P.construct_time_series(saveat=[0.0, 0.5, 1.0]).neural_ode.kwargs["save_start"] is True
    assert P.construct_time_series(saveat=[0.5, 1.0], tspan=(0.5, 1.0)).neural_ode.kwargs["save_start"] is True
    assert P.construct_time_series(saveat=[0.0, 1.0], save_start=False).neural_ode.kwargs["save_start"] is False


def test_reparameterize_layer_state():
    import lrnde_amd as P
    rp = P.ReparameterizeLayer()
    rng = np.random.default_rng(0)
    st = rp.initialstates(rng)
    ref = np.random.default_rng(0)
    ref.standard_normal(1)                                # common.jl:51 burns one draw
    assert st["rng"].bit_generator.state == ref.bit_generator.state and st["training"] is True
    eps, adv = rp.draw(st, 4, 2)
    assert st["rng"].bit_generator.state == ref.bit_generator.state   # the state's own rng is not advanced: a copy is
    assert np.array_equal(eps, ref.standard_normal((4, 2), dtype=np.float32)) and adv.bit_generator.state == ref.bit_generator.state
    x = torch.arange(8.).reshape(2, 4)
    z, st2 = rp(x, None, dict(st, training=False))       # common.jl:73-77
    assert torch.equal(z, x[:, :2]) and torch.equal(st2["mu0"], x[:, :2]) and torch.equal(st2["logvar"], x[:, :2])


def test_end_to_end_yardstick_error():
    """RK4 with 200 steps against 400 on the tiny shape: the yardstick of test_gpu_latent's end-to-end check must itself be
    within 1e-4 of every gradient block's norm"""
    dims, B, T = LC.TINY, 9, 4
    times = [0.25, 0.5, 0.75, 1.0]
    flat, node = LC.make_params(dims, seed=11), LC.make_node_params(dims, seed=12)
    data, mask, dt = LC.make_batch(dims, B, T, seed=13, unobserved_column=False)
    mask[:, 0, 0] = 1
    x = LC.x_of(data, mask, dt)
    eps = np.random.default_rng(14).standard_normal((B, dims[3])).astype(np.float32)
    a = LC.model_reference(dims, flat, node, x, eps, data, mask, times, 0.5, 200)
    b = LC.model_reference(dims, flat, node, x, eps, data, mask, times, 0.5, 400)
    ga, gb = LC.split_blocks(a["dp"], dims), LC.split_blocks(b["dp"], dims)
    errs = {k: LC.rel(ga[k], gb[k]) for k in LC.BLOCKS}
    errs["neural_ode"] = LC.rel(a["dnode"], b["dnode"])
    print("RK4 200 vs 400 steps, relative to each block's norm:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(np.linalg.norm(gb[k]) > 0 for k in LC.BLOCKS)
    assert max(errs.values()) <= 1e-4, errs
