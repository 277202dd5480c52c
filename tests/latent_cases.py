"""Inputs, parameters and the compiled float32 host restatement shared by tests/test_host_latent.py,
tests/test_gpu_latent.py and tests/test_gpu_latent_envelope.py.  Nothing here imports the package."""
import os
import subprocess
import tempfile

import numpy as np
import torch

import latent_np as LN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = (3, 5, 3, 2)           # I, H, L, N: F = 7; odd widths
PHYSIONET = (37, 40, 50, 20)  # experiments/configs/physionet.yml
BLOCKS = ("update_gate", "reset_gate", "new_state", "rec_to_gen", "gen_to_data")


def param_count(dims):
    return sum(LN.block_sizes(*dims).values())


def make_params(dims, seed, scale=1.0):
    """glorot-like weights and SMALL NONZERO biases (a zero bias would hide a misplaced bias row), float32"""
    I, H, L, N = dims
    K = 2 * L + 2 * I + 1
    rng = np.random.default_rng(seed)
    parts = []

    def dense(out, inn):
        parts.append(((rng.random((inn, out)) - 0.5) * np.sqrt(24.0 / (inn + out)) * scale).astype(np.float32).ravel())
        parts.append(((rng.random(out) - 0.5) * 0.2).astype(np.float32))

    for out2 in (L, L, 2 * L):
        dense(H, K); dense(out2, H)
    dense(L, 2 * L); dense(2 * N, L); dense(I, N)
    flat = np.concatenate(parts)
    assert flat.size == param_count(dims)
    return flat


def make_node_params(dims, seed, scale=1.5):
    I, H, L, N = dims
    rng = np.random.default_rng(seed)
    parts = []
    for i in range(8):
        inn, out = (N, H) if i % 2 == 0 else (H, N)
        parts.append(((rng.random((inn, out)) - 0.5) * np.sqrt(24.0 / (inn + out)) * scale).astype(np.float32).ravel())
        parts.append(((rng.random(out) - 0.5) * 0.2).astype(np.float32))
    return np.concatenate(parts)


def make_batch(dims, B, T, seed, unobserved_column=True):
    """data, mask (B, T, I), dt (B, T, 1), float32.  Mask entries are exactly 0 or 1 and dt >= 0, so mask_t does not depend
    on the order of its sum.  One step is unobserved in every column (mask 0, dt 0) when T > 1; with `unobserved_column`
    (and B > 1) the last column is unobserved at every step."""
    I = dims[0]
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((B, T, I)).astype(np.float32)
    mask = (rng.random((B, T, I)) < 0.5).astype(np.float32)
    dt = (rng.random((B, T, 1)) * 0.1).astype(np.float32)
    if T > 1:
        tu = T // 2
        mask[:, tu] = 0; dt[:, tu] = 0
    if unobserved_column and B > 1:
        mask[B - 1] = 0; dt[B - 1] = 0
    return data, mask, dt


# Shapes on the kernels' own loop and tile edges (csrc/lrnde_latent.hpp: LNB = 8 columns per workgroup, thread rows
# j = 0..63, create limit 3H <= 128): (name, (I, H, L, N), B, T)
ENVELOPE = [
    ("min", (1, 1, 1, 1), 8, 3),           # every width 1, a padded pair in phase A (3H = 3 of OPA = 4), one exactly full tile
    ("hmax", (3, 42, 4, 2), 16, 5),        # 3H = 126, the create limit; two full tiles
    ("lwide", (3, 8, 70, 2), 17, 6),       # L > 64: second trip of every L loop, third of every 2L loop; three workgroups, tile 2 one never-observed column
    ("nwide", (3, 8, 5, 40), 17, 6),       # 2N = 80: second trip of rec_to_gen's second layer and of the backward's 2N contraction
    ("nwider", (2, 4, 3, 70), 9, 4),       # N > 64: second trip of the reparameterisation loops, forward and backward
    ("physionet3", PHYSIONET, 24, 49),     # the experiment's shape on three full tiles
    ("long", TINY, 9, 130),                # a long reverse walk; T * LNB past one pass of the 512 threads over the mask table
]
ENVELOPE_NAMES = [c[0] for c in ENVELOPE]
LNB = 8                                    # columns per workgroup
LAT_MAX_T = 4096
LAT_MAX_LDS = 160 * 1024


def observed(x, I):
    """mask_t of latent_ode.jl:40 per (column, step): the mask rows and dt of x_t sum to more than zero"""
    return x[:, :, I:].sum(axis=2) > 0


def mixed_batch(dims, B, T, seed):
    """make_batch with its never-observed last column; with two full tiles (B >= 16, T >= 3) tile 0 is unobserved at step 0
    while tile 1 is observed there, and the other way round at step 1: the tiles skip different steps"""
    data, mask, dt = make_batch(dims, B, T, seed)
    if B >= 16 and T >= 3:
        mask[0:8, 0] = 0; dt[0:8, 0] = 0; mask[8, 0, 0] = 1
        mask[8:16, 1] = 0; dt[8:16, 1] = 0; mask[0, 1, 0] = 1
    return data, mask, dt


def sub_blocks(dims):
    """[(name, start, stop)] over the flat encoder vector: per gate the first layer's carry rows, x_t rows and bias, then the
    second layer's weight and bias; then rec_to_gen's two layers.  A Dense is W[k][o] at k * out + o (inputs: the carry
    first, then x_t), then b."""
    I, H, L, N = dims
    F = 2 * I + 1
    out, pos = [], 0

    def add(name, n):
        nonlocal pos
        out.append((name, pos, pos + n))
        pos += n

    for gate, out2 in (("update_gate", L), ("reset_gate", L), ("new_state", 2 * L)):
        add(gate + ".l1_carry", 2 * L * H); add(gate + ".l1_x", F * H); add(gate + ".l1_b", H)
        add(gate + ".l2_W", H * out2); add(gate + ".l2_b", out2)
    add("rec_to_gen.l1_W", 2 * L * L); add("rec_to_gen.l1_b", L)
    add("rec_to_gen.l2_W", L * 2 * N); add("rec_to_gen.l2_b", 2 * N)
    assert pos == param_count(dims) - (I * N + I)
    return out


def dx_rows(I):
    """[(name, start, stop)] over the last axis of dx: vcat(data, mask, dt)"""
    return [("dx.data", 0, I), ("dx.mask", I, 2 * I), ("dx.dt", 2 * I, 2 * I + 1)]


def dead_rows(dims):
    """flat indices of rows 0..L-1 of new_state's second layer (weights and bias): latent_ode.jl:37 never reads them"""
    I, H, L, N = dims
    K = 2 * L + 2 * I + 1
    gate = H * K + H + L * H + L
    w2 = 2 * gate + H * K + H
    idx = (w2 + np.arange(H)[:, None] * 2 * L + np.arange(L)[None, :]).ravel()
    return np.concatenate([idx, w2 + 2 * L * H + np.arange(L)])


def lat_smem_bytes(dims, bwd, T):
    """lat_smem_bytes of csrc/lrnde_latent.hpp: the gates' weight image, the tile's activations and the mask table"""
    I, H, L, N = dims
    F, even = 2 * I + 1, lambda v: v + (v & 1)
    OPA, OPB, OPD = even(3 * H), even(2 * L), even(L)
    ldsw = ((F + 2 * L + 1) * OPA + (H + 1) * OPB + (H + 1) * OPD + 3) // 4 * 4
    act = (F + 2 * L + OPA + 3 * L + 2 * L + 2 * N) * LNB
    if bwd:
        act += (2 * (2 * L) + OPA + 2 * L + L + 2 * L) * LNB
    return (ldsw + act) * 4 + (T + 1) * LNB + 16


def t_fit(dims):
    """the largest T lrnde_latent_encode accepts: LAT_MAX_T, or what the backward's LDS leaves for the mask table"""
    return min(LAT_MAX_T, (LAT_MAX_LDS - lat_smem_bytes(dims, True, -1)) // LNB - 1)


_ENV = {}


def envelope_inputs(dims, B, T):
    """parameters (seed 21), mixed_batch (22), eps and the three cotangents (23), as test_gpu_latent.case draws them"""
    flat = make_params(dims, seed=21)
    x = x_of(*mixed_batch(dims, B, T, seed=22))
    rng = np.random.default_rng(23)
    eps = rng.standard_normal((B, dims[3])).astype(np.float32)
    cots = [rng.standard_normal((B, dims[3])).astype(np.float32) for _ in range(3)]
    return dict(dims=dims, B=B, T=T, flat=flat, x=x, eps=eps, cots=cots)


def envelope_case(name):
    """inputs and the two torch runs of an ENVELOPE case, computed once and left unchanged"""
    if name not in _ENV:
        _, dims, B, T = ENVELOPE[ENVELOPE_NAMES.index(name)]
        c = envelope_inputs(dims, B, T)
        c["r64"] = encoder_reference(dims, c["flat"], c["x"], c["eps"], c["cots"], torch.float64)
        c["r32"] = encoder_reference(dims, c["flat"], c["x"], c["eps"], c["cots"], torch.float32)
        _ENV[name] = c
    return _ENV[name]


# encode_backward's optional arguments on `hmax`: (run, dy, dz0, dmu, dlogvar, training)
OPTIONAL_RUNS = [("a", False, False, True, False, True), ("b", False, False, False, True, True),
                 ("c", True, True, False, False, True), ("d", True, True, True, True, False)]


def optional_case(run):
    """the `hmax` inputs with the cotangents of an OPTIONAL_RUNS row (an absent one is None; dy from seed 24) and its two
    torch runs, computed once"""
    key = ("optional", run)
    if key not in _ENV:
        _, use_dy, use_z, use_m, use_l, training = OPTIONAL_RUNS[[r[0] for r in OPTIONAL_RUNS].index(run)]
        base = envelope_case("hmax")
        dims, B = base["dims"], base["B"]
        dy = np.random.default_rng(24).standard_normal((B, 2 * dims[2])).astype(np.float32) if use_dy else None
        given = [c if use else None for c, use in zip(base["cots"], (use_z, use_m, use_l))]
        cots = [np.zeros_like(base["eps"]) if g is None else g for g in given]
        c = dict(base, dy=dy, given=given, training=training)
        for k, dt in (("r64", torch.float64), ("r32", torch.float32)):
            c[k] = encoder_reference(dims, base["flat"], base["x"], base["eps"], cots, dt, training, dy=dy)
        _ENV[key] = c
    return _ENV[key]


def e2e_physionet(nsteps=200, training=True, eps=None):
    """the end-to-end inputs of test_end_to_end_yardstick_error (seeds 11 / 12 / 13 / 14, B = 9, 4 saved times) at the
    experiment's shape, and float64 autograd through encoder, RK4 with `nsteps` steps, decoder and loss; computed once.
    `eps` replaces the seed-14 draw (a model draws its own from its state)."""
    key = ("e2e", nsteps, training, None if eps is None else eps.tobytes())
    if key not in _ENV:
        dims, B, T, times = PHYSIONET, 9, 4, [0.25, 0.5, 0.75, 1.0]
        flat, node = make_params(dims, seed=11), make_node_params(dims, seed=12)
        data, mask, dt = make_batch(dims, B, T, seed=13, unobserved_column=False)
        mask[:, 0, 0] = 1
        if eps is None:
            eps = np.random.default_rng(14).standard_normal((B, dims[3])).astype(np.float32)
        c = dict(dims=dims, B=B, T=T, times=times, flat=flat, node=node, data=data, mask=mask, dt=dt, eps=eps, w_kl=0.5)
        c["ref"] = model_reference(dims, flat, node, x_of(data, mask, dt), eps, data, mask, times, 0.5, nsteps, training=training)
        _ENV[key] = c
    return _ENV[key]


def sub_block_errors(dims, dp, dx, r64, r32):
    """[(name, error of (dp, dx), distance of r32, float64 norm)] per sub_blocks / dx_rows entry, each relative to the float64
    sub-block's norm (absolute where that norm is zero)"""
    rows = []
    for name, a, b in sub_blocks(dims):
        ref = r64["dp"][a:b]
        rows.append((name, rel(dp[a:b], ref), rel(r32["dp"][a:b], ref), float(np.linalg.norm(ref))))
    if dx is not None:
        for name, a, b in dx_rows(dims[0]):
            ref = r64["dx"][..., a:b]
            rows.append((name, rel(dx[..., a:b], ref), rel(r32["dx"][..., a:b], ref), float(np.linalg.norm(ref))))
    return rows


def loss_mask(dims, B, T, seed):
    """a 0/1 mask (B, T, I) with at least one observed entry per column (no division by zero in utils.jl:97)"""
    rng = np.random.default_rng(seed)
    m = (rng.random((B, T, dims[0])) < 0.5).astype(np.float32)
    m[:, 0, 0] = 1
    return m


def x_of(data, mask, dt):
    return np.ascontiguousarray(np.concatenate([data, mask, dt], axis=2))   # vcat(data, mask, dt), construct.jl:40


def rel(a, ref):
    a, ref = np.asarray(a, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    n = np.linalg.norm(ref)
    return float(np.linalg.norm(a - ref) / n) if n > 0 else float(np.linalg.norm(a))


def bound(f32_value, f64_value):
    """the suite's rule (tests/test_gpu_chain_adjoint.py): max(1e-5, 4 x the distance of the float32 torch restatement from
    its float64 run), relative to the float64 value's norm"""
    return max(1e-5, 4.0 * rel(f32_value, f64_value))


def split_blocks(flat, dims):
    sizes, out, pos = LN.block_sizes(*dims), {}, 0
    for name in BLOCKS:
        out[name] = flat[pos:pos + sizes[name]]
        pos += sizes[name]
    return out


def encoder_reference(dims, flat, x, eps, cots, dtype, training=True, dy=None):
    """forward values and, for loss = <cz, z0> + <cm, mu> + <cl, logvar> (+ <dy, y>), the cotangents of the parameters and of x"""
    p = torch.tensor(flat, dtype=dtype, requires_grad=True)
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    ps = LN.unflatten(p, *dims)
    y, mu, lv, z0 = LN.encode(ps, dims[2], xt, torch.tensor(eps, dtype=dtype), training)
    cz, cm, cl = (torch.tensor(c, dtype=dtype) for c in cots)
    loss = (z0 * cz).sum() + (mu * cm).sum() + (lv * cl).sum()
    if dy is not None:
        loss = loss + (y * torch.tensor(dy, dtype=dtype)).sum()
    loss.backward()
    return dict(y=y.detach().numpy(), mu=mu.detach().numpy(), logvar=lv.detach().numpy(), z0=z0.detach().numpy(),
                dp=p.grad.numpy(), dx=xt.grad.numpy())


def decode_reference(dims, flat, series, data, mask, mu, lv, w_kl, dtype):
    p = torch.tensor(flat, dtype=dtype, requires_grad=True)
    s, m, l = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (series, mu, lv))
    ps = LN.unflatten(p, *dims)
    loss, ll, kl, y = LN.decode_loss(ps, s, torch.tensor(data, dtype=dtype), torch.tensor(mask, dtype=dtype), m, l, w_kl)
    loss.backward()
    return dict(loss=float(loss.detach()), ll=ll.detach().numpy(), kl=kl.detach().numpy(), pred=y.detach().numpy(), dseries=s.grad.numpy(),
                dmu=m.grad.numpy(), dlogvar=l.grad.numpy(), dpg=split_blocks(p.grad.numpy(), dims)["gen_to_data"])


def model_reference(dims, flat, node_flat, x, eps, data, mask, times, w_kl, nsteps, dtype=torch.float64, training=True):
    p = torch.tensor(flat, dtype=dtype, requires_grad=True)
    q = torch.tensor(node_flat, dtype=dtype, requires_grad=True)
    t = lambda a: torch.tensor(a, dtype=dtype)
    loss, ll, kl, y = LN.model_loss(p, q, dims, t(x), t(eps), t(data), t(mask), list(times), w_kl, nsteps, training)
    loss.backward()
    return dict(loss=float(loss.detach()), dp=p.grad.numpy(), dnode=q.grad.numpy(), pred=y.detach().numpy())


_HOST_EXE = {}


def host_exe():
    """tests/latent_host.cpp compiled with -O2 -ffp-contract=off (as tests/test_math_header.py compiles its program)"""
    if "exe" not in _HOST_EXE:
        d = tempfile.mkdtemp(prefix="latent_host_")
        exe = os.path.join(d, "latent_host")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "localregneuralde.jl_amd", "csrc"),
                        os.path.join(ROOT, "tests", "latent_host.cpp"), "-o", exe], check=True)
        _HOST_EXE["exe"], _HOST_EXE["dir"] = exe, d
    return _HOST_EXE["exe"]


def run_host(dims, flat, x, eps, training=True):
    """the float32 host restatement: dict(y, mu, logvar, z0)"""
    I, H, L, N = dims
    B, T = x.shape[0], x.shape[1]
    exe = host_exe()
    fin, fout = os.path.join(_HOST_EXE["dir"], "in.bin"), os.path.join(_HOST_EXE["dir"], "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([I, H, L, N, B, T, int(training)], np.int32).tobytes())
        for a in (flat, x, eps):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    subprocess.run([exe, fin, fout], check=True)
    raw = np.fromfile(fout, np.float32)
    assert raw.size == B * (2 * L + 3 * N)
    y, rest = raw[:B * 2 * L].reshape(B, 2 * L), raw[B * 2 * L:].reshape(3, B, N)
    return dict(y=y, mu=rest[0], logvar=rest[1], z0=rest[2])
