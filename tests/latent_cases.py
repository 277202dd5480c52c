"""Inputs, parameters and the compiled float32 host restatement shared by tests/test_host_latent.py and
tests/test_gpu_latent.py.  Nothing here imports the package."""
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


def encoder_reference(dims, flat, x, eps, cots, dtype, training=True):
    """forward values and, for loss = <cz, z0> + <cm, mu> + <cl, logvar>, the cotangents of the parameters and of x"""
    p = torch.tensor(flat, dtype=dtype, requires_grad=True)
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    ps = LN.unflatten(p, *dims)
    y, mu, lv, z0 = LN.encode(ps, dims[2], xt, torch.tensor(eps, dtype=dtype), training)
    cz, cm, cl = (torch.tensor(c, dtype=dtype) for c in cots)
    ((z0 * cz).sum() + (mu * cm).sum() + (lv * cl).sum()).backward()
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


def model_reference(dims, flat, node_flat, x, eps, data, mask, times, w_kl, nsteps, dtype=torch.float64):
    p = torch.tensor(flat, dtype=dtype, requires_grad=True)
    q = torch.tensor(node_flat, dtype=dtype, requires_grad=True)
    t = lambda a: torch.tensor(a, dtype=dtype)
    loss, ll, kl, y = LN.model_loss(p, q, dims, t(x), t(eps), t(data), t(mask), list(times), w_kl, nsteps)
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
