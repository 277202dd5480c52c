"""Latent-ODE layers off the GPU: sigmoid_c of csrc/lrnde_math.hpp against float64, the float32 host restatement of the encoder
(tests/latent_host.cpp, the bits the GPU kernel must return) against the float64 transcription of the reference
(tests/latent_np.py), exact properties of that transcription, the parameter layout helpers, and the error of the end-to-end
yardstick itself.

Measured (printed by the tests):
  sigmoid_c max abs error 8.87e-08 (at x = 7.38) against tanhf_c's 7.75e-08 over the same sweep: bound 4 x 7.75e-08;
  host float32 restatement vs float64: 3e-08..2.7e-07 of each output's norm at both shapes, the torch float32 run the same:
  every bound is the rule's floor 1e-5;
  RK4 200 vs 400 steps, tiny shape: at most 1.1e-10 of a gradient block's norm (bound 1e-4); at the experiment's shape
  1.2e-10..2.4e-10, gen_to_data 2.7e-11;
  LC.ENVELOPE (the shapes of tests/test_gpu_latent_envelope.py): torch float32 against float64 per LC.sub_blocks / LC.dx_rows
  entry and forward output at most 5.5e-7 on the envelope, 6.5e-7 on the optional-argument runs, 1.7e-6 on the merged cases
  (update_gate.l2_b of 3/5/3/2 B = 9 T = 4): asserted <= 2.5e-6, where max(1e-5, 4 x twin) is still its floor."""
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


# ---- the shape envelope of tests/test_gpu_latent_envelope.py (LC.ENVELOPE) ---------------------------------------------------
TWIN_CAP = 2.5e-6   # 4 x this is the floor 1e-5 of LC.bound: while every twin distance is below it the rule cannot widen


@pytest.mark.parametrize("name,dims,B,T", LC.ENVELOPE)
def test_envelope_batches_meet_their_selection_conditions(name, dims, B, T):
    c = LC.envelope_inputs(dims, B, T)
    obs = LC.observed(c["x"], dims[0])                                  # (B, T)
    nt = (B + LC.LNB - 1) // LC.LNB
    tile = np.stack([obs[i * LC.LNB:(i + 1) * LC.LNB].any(axis=0) for i in range(nt)])   # (tiles, T): the tile runs the step
    assert (~obs).all(axis=0).any()                                     # a step unobserved everywhere
    assert not obs[B - 1].any() and obs[:B - 1].any(axis=1).all()       # only the last column is never observed
    if B >= 16:
        assert (~tile[0] & tile[1]).any() and (tile[0] & ~tile[1]).any()   # the tiles skip different steps
        assert obs[:16].any(axis=0)[:2].all()                           # ... which the other tile runs
    if name in ("lwide", "nwide"):
        assert (~tile.any(axis=1)).any()                                # a tile that skips every step
    assert (B % LC.LNB == 0) == (name in ("min", "hmax", "physionet3"))  # full last tiles
    assert set(np.unique(c["x"][:, :, dims[0]:2 * dims[0]])) <= {0.0, 1.0}


@pytest.mark.parametrize("name", LC.ENVELOPE_NAMES)
@pytest.mark.parametrize("training", [True, False])
def test_host_restatement_on_the_envelope(name, training):
    c = LC.envelope_case(name)
    dims, B = c["dims"], c["B"]
    zero = [np.zeros_like(c["eps"])] * 3
    if training:
        r64, r32 = c["r64"], c["r32"]
    else:
        r64, r32 = (LC.encoder_reference(dims, c["flat"], c["x"], c["eps"], zero, dt, False) for dt in (torch.float64, torch.float32))
    got = LC.run_host(dims, c["flat"], c["x"], c["eps"], training)
    for k in ("y", "mu", "logvar", "z0"):
        b, e = LC.bound(r32[k], r64[k]), LC.rel(got[k], r64[k])
        print(f"{name} training={training} {k}: host {e:.2e} torch-f32 {LC.rel(r32[k], r64[k]):.2e} bound {b:.2e}")
        assert e <= b, (k, e, b)
    L = dims[2]
    assert np.array_equal(got["y"][B - 1], np.concatenate([np.zeros(L, np.float32), np.ones(L, np.float32)]))


def _twin_rows(c):
    rows = [(n, twin) for n, _, twin, _ in LC.sub_block_errors(c["dims"], c["r64"]["dp"], c["r64"]["dx"], c["r64"], c["r32"])]
    return rows + [(k, LC.rel(c["r32"][k], c["r64"][k])) for k in ("y", "mu", "logvar", "z0")]


def _assert_twin(label, rows):
    worst = max(rows, key=lambda r: r[1])
    print(f"{label}: worst float32 twin distance {worst[1]:.2e} ({worst[0]}) of {len(rows)} entries")
    assert worst[1] <= TWIN_CAP, (label, worst)


@pytest.mark.parametrize("name", LC.ENVELOPE_NAMES)
def test_the_yardstick_binds_on_the_envelope(name):
    """a condition, not a measurement: the float32 torch run is within 2.5e-6 of the float64 run on every sub-block, dx row
    group and forward output, so max(1e-5, 4 x twin) is its floor 1e-5 wherever the GPU tests apply it"""
    _assert_twin(name, _twin_rows(LC.envelope_case(name)))


@pytest.mark.parametrize("run", [r[0] for r in LC.OPTIONAL_RUNS])
def test_the_yardstick_binds_on_the_optional_argument_runs(run):
    _assert_twin("hmax run " + run, _twin_rows(LC.optional_case(run)))


def test_the_yardstick_binds_on_the_merged_cases():
    import test_gpu_latent as TG
    for dims, B, T in TG.CASES:
        _assert_twin(f"{dims} B={B} T={T}", _twin_rows(dict(TG.case(dims, B, T), dims=dims)))


@pytest.mark.parametrize("name", LC.ENVELOPE_NAMES)
def test_exact_zeros_of_the_float64_restatement_on_the_envelope(name):
    c = LC.envelope_case(name)
    dims = c["dims"]
    obs = LC.observed(c["x"], dims[0])
    dx, dp = c["r64"]["dx"], c["r64"]["dp"]
    assert np.all(dx[~obs] == 0) and np.any(dx[obs] != 0)
    dead = LC.dead_rows(dims)
    assert dead.size == dims[2] * dims[1] + dims[2] and np.all(dp[dead] == 0)
    for n, a, b in LC.sub_blocks(dims):   # every sub-block is reached by the cotangents: none of the GPU's bounds is vacuous
        assert np.any(dp[a:b] != 0), n


def test_sub_blocks_tile_the_encoder_vector():
    for dims in (LC.TINY, LC.PHYSIONET, (1, 1, 1, 1)):
        I, H, L, N = dims
        sb = LC.sub_blocks(dims)
        assert sb[0][1] == 0 and all(a[2] == b[1] for a, b in zip(sb, sb[1:])) and sb[-1][2] == LC.param_count(dims) - (I * N + I)
        sizes, pos = LN.block_sizes(*dims), 0
        for blk in LC.BLOCKS[:4]:   # the sub-blocks of a block tile that block
            mine = [s for s in sb if s[0].startswith(blk + ".")]
            assert mine[0][1] == pos and mine[-1][2] == pos + sizes[blk]
            pos += sizes[blk]
        # the named ranges are what unflatten reads: mark new_state's first layer and look at (out, in)
        flat = torch.zeros(LC.param_count(dims))
        rng = {n: (a, b) for n, a, b in sb}
        for v, n in enumerate(("new_state.l1_carry", "new_state.l1_x", "new_state.l1_b", "new_state.l2_W", "new_state.l2_b"), 1):
            flat[rng[n][0]:rng[n][1]] = v
        (W1, b1), (W2, b2) = LN.unflatten(flat, *dims)["new_state"]
        assert torch.all(W1[:, :2 * L] == 1) and torch.all(W1[:, 2 * L:] == 2) and torch.all(b1 == 3)
        assert torch.all(W2 == 4) and torch.all(b2 == 5)
        marked = torch.zeros(LC.param_count(dims))
        marked[torch.from_numpy(LC.dead_rows(dims))] = 1
        (_, _), (W2, b2) = LN.unflatten(marked, *dims)["new_state"]
        assert torch.all(W2[:L] == 1) and torch.all(W2[L:] == 0) and torch.all(b2[:L] == 1) and torch.all(b2[L:] == 0)
        assert marked.sum() == L * H + L
    assert LC.dx_rows(3) == [("dx.data", 0, 3), ("dx.mask", 3, 6), ("dx.dt", 6, 7)]


def test_lds_bytes_and_the_largest_T():
    """lat_smem_bytes / the encode gate of csrc/lrnde_latent.hpp restated: the header's "37/40/50/20 needs 143 KiB"; derived
    here, run by tests/test_gpu_latent_envelope.py (the refusal prints the byte count)"""
    assert LC.lat_smem_bytes(LC.PHYSIONET, True, 1) == 146048 + 8 * 2 + 16
    assert LC.lat_smem_bytes(LC.PHYSIONET, True, 1) // 1024 == 142 and round(LC.lat_smem_bytes(LC.PHYSIONET, True, 1) / 1024) == 143
    assert LC.lat_smem_bytes(LC.PHYSIONET, False, 1) < LC.lat_smem_bytes(LC.PHYSIONET, True, 1)
    assert LC.t_fit(LC.TINY) == 4096
    tf = LC.t_fit(LC.PHYSIONET)
    assert tf == 2221 and tf < 4096
    assert LC.lat_smem_bytes(LC.PHYSIONET, True, tf) <= 160 * 1024 < LC.lat_smem_bytes(LC.PHYSIONET, True, tf + 1)
    for _, dims, _, T in LC.ENVELOPE:   # every envelope case is inside both limits
        assert T <= LC.t_fit(dims)


def test_end_to_end_yardstick_error_at_the_experiments_shape():
    """RK4 with 200 steps against 400 at 37/40/50/20, B = 9, 4 saved times: within 1e-4 of every gradient block's norm, three
    orders of magnitude inside the 3e-4 bar of tests/test_gpu_latent_envelope.py's end-to-end check"""
    a, b = LC.e2e_physionet(200), LC.e2e_physionet(400)
    dims = a["dims"]
    ga, gb = LC.split_blocks(a["ref"]["dp"], dims), LC.split_blocks(b["ref"]["dp"], dims)
    errs = {k: LC.rel(ga[k], gb[k]) for k in LC.BLOCKS}
    errs["neural_ode"] = LC.rel(a["ref"]["dnode"], b["ref"]["dnode"])
    print("RK4 200 vs 400 steps, relative to each block's norm:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(np.linalg.norm(gb[k]) > 0 for k in LC.BLOCKS)
    assert max(errs.values()) <= 1e-4, errs
    assert abs(a["ref"]["loss"] - b["ref"]["loss"]) <= 1e-4 * abs(b["ref"]["loss"])
