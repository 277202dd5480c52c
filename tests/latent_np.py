"""The Latent-ODE layers restated in torch, line for line from the reference, in the dtype of the parameters it is given
(float64: the yardstick of tests/test_host_latent.py and tests/test_gpu_latent.py; float32: the restatement whose distance
from the float64 run sets those tests' bounds).  Gradients come from autograd.

  src/layers/latent_ode.jl:1-48      LatentGRUCell, walked by Lux's Recurrence (return_sequence = false)
  src/layers/common.jl:55-77         ReparameterizeLayer
  experiments/src/utils.jl:94-101    log_likelihood_loss, kl_divergence
  experiments/src/construct.jl:36-76,230-252   the loss and the model

Arrays are batch first: x (B, T, F) is Julia's (F, T, B).  The flat parameter vector is the Lux ComponentArray:
gru.update_gate, gru.reset_gate, gru.new_state, rec_to_gen, gen_to_data (each Dense: vec(W) column-major out x in, then b);
`neural_ode` (gen_dynamics, construct.jl:235-243) is a vector of its own.  This file does not import the package."""
import math

import torch


def block_sizes(I, H, L, N):
    K = 2 * L + 2 * I + 1
    gate = H * K + H + L * H + L
    return dict(update_gate=gate, reset_gate=gate, new_state=H * K + H + 2 * L * H + 2 * L,
                rec_to_gen=L * 2 * L + L + 2 * N * L + 2 * N, gen_to_data=I * N + I)


def _take(flat, pos, out, inn):
    W = flat[pos:pos + out * inn].reshape(inn, out).t()   # column-major out x in
    b = flat[pos + out * inn:pos + out * inn + out]
    return (W, b), pos + out * inn + out


def unflatten(flat, I, H, L, N):
    """flat vector -> dict of blocks, each a list of (W (out, in), b)"""
    K, pos, ps = 2 * L + 2 * I + 1, 0, {}
    for name, out2 in (("update_gate", L), ("reset_gate", L), ("new_state", 2 * L)):
        l1, pos = _take(flat, pos, H, K)
        l2, pos = _take(flat, pos, out2, H)
        ps[name] = [l1, l2]
    l1, pos = _take(flat, pos, L, 2 * L)
    l2, pos = _take(flat, pos, 2 * N, L)
    ps["rec_to_gen"] = [l1, l2]
    l1, pos = _take(flat, pos, I, N)
    ps["gen_to_data"] = [l1]
    assert pos == flat.numel()
    return ps


def dense(layer, x, act=None):
    W, b = layer
    y = x @ W.t() + b
    return y if act is None else act(y)


def gru_cell(ps, L, x, carry=None):
    """latent_ode.jl:19-47"""
    if carry is None:                                             # :19-23
        y_mean = torch.zeros((x.shape[0], L), dtype=x.dtype)
        y_std = torch.ones((x.shape[0], L), dtype=x.dtype)
    else:
        y_mean, y_std = carry
    y_concat = torch.cat([y_mean, y_std, x], dim=1)               # :26
    update_gate = dense(ps["update_gate"][1], dense(ps["update_gate"][0], y_concat, torch.tanh), torch.sigmoid)   # :28
    reset_gate = dense(ps["reset_gate"][1], dense(ps["reset_gate"][0], y_concat, torch.tanh), torch.sigmoid)      # :29
    concat = torch.cat([y_mean * reset_gate, y_std * reset_gate, x], dim=1)                                       # :31
    new_state = dense(ps["new_state"][1], dense(ps["new_state"][0], concat, torch.tanh), torch.tanh)              # :33
    new_state_mean = new_state[:, :L]                             # :34 (never used again)
    new_state_std = new_state[:, L:]                              # :35
    del new_state_mean
    new_y_mean = (1 - update_gate) * new_state_std + update_gate * y_mean   # :37 — new_state_STD, as written
    new_y_std = (1 - update_gate) * new_state_std + update_gate * y_std     # :38
    F = x.shape[1]
    mask = (x[:, F // 2:].sum(dim=1, keepdim=True) > 0).to(x.dtype)         # :40
    new_y_mean = mask * new_y_mean + (1 - mask) * y_mean          # :42
    new_y_std = mask * new_y_std + (1 - mask) * y_std             # :43
    return torch.cat([new_y_mean, new_y_std], dim=1), (new_y_mean, new_y_std)   # :45-46


def recurrence(ps, L, x):
    """Lux.Recurrence(cell) with return_sequence = false over the second-to-last Julia dimension: x (B, T, F)"""
    y, carry = gru_cell(ps, L, x[:, 0])
    for t in range(1, x.shape[1]):
        y, carry = gru_cell(ps, L, x[:, t], carry)
    return y


def reparameterize(training, out, eps):
    """common.jl:61-77: returns (z0, mu0, logvar)"""
    N = out.shape[1] // 2
    mu = out[:, :N]
    if not training:
        return mu, mu, mu
    logvar = out[:, N:]
    return mu + torch.exp(logvar / 2) * eps, mu, logvar


def encode(ps, L, x, eps, training=True):
    y = recurrence(ps, L, x)
    out = dense(ps["rec_to_gen"][1], dense(ps["rec_to_gen"][0], y, torch.tanh))
    z0, mu, logvar = reparameterize(training, out, eps)
    return y, mu, logvar, z0


def log_likelihood_loss(dpred, mask):
    """utils.jl:94-98: dpred, mask (B, T, I)"""
    sigma = 0.01
    sample = -(dpred ** 2) / (2 * sigma ** 2) - math.log(sigma) - math.log(2 * math.pi) / 2
    return sample.sum(dim=(1, 2)) / mask.sum(dim=(1, 2))


def kl_divergence(mu, logvar):
    """utils.jl:101"""
    return (torch.exp(logvar) + mu ** 2 - 1 - logvar).mean(dim=1) / 2


def decode_loss(ps, series, data, mask, mu, logvar, w_kl):
    """series (T, B, N) -> y (B, T, I); construct.jl:43-50.  Returns (loss, ll, kl, y)."""
    y = dense(ps["gen_to_data"][0], series).permute(1, 0, 2)
    dpred = y * mask - data * mask
    ll = log_likelihood_loss(dpred, mask)
    kl = kl_divergence(mu, logvar)
    return -(ll - w_kl * kl).mean(), ll, kl, y


def gen_dynamics(node_flat, N, H):
    """construct.jl:235-243: tanh.(u) then eight Dense layers N => H => N ..., all tanh"""
    layers, pos = [], 0
    for i in range(8):
        inn, out = (N, H) if i % 2 == 0 else (H, N)
        l, pos = _take(node_flat, pos, out, inn)
        layers.append(l)
    assert pos == node_flat.numel()

    def f(u):
        h = torch.tanh(u)
        for l in layers:
            h = dense(l, h, torch.tanh)
        return h
    return f


def rk4_series(f, z0, times, nsteps):
    """classical RK4 on [0, 1] with nsteps steps; the states at `times` (each a multiple of 1 / nsteps) stacked (T, B, N)"""
    h = 1.0 / nsteps
    marks = {int(round(t * nsteps)): i for i, t in enumerate(times)}
    assert len(marks) == len(times) and all(abs(k / nsteps - times[i]) < 1e-9 for k, i in marks.items())
    out, u = [None] * len(times), z0
    if 0 in marks:
        out[marks[0]] = u
    for k in range(nsteps):
        k1 = f(u); k2 = f(u + 0.5 * h * k1); k3 = f(u + 0.5 * h * k2); k4 = f(u + h * k3)
        u = u + (h / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)
        if k + 1 in marks:
            out[marks[k + 1]] = u
    return torch.stack(out, dim=0)


def model_loss(flat, node_flat, dims, x, eps, data, mask, times, w_kl, nsteps=200, training=True):
    """the whole model and its loss without the regulariser (construct.jl:38-55): (loss, ll, kl, y)"""
    I, H, L, N = dims
    ps = unflatten(flat, I, H, L, N)
    _, mu, logvar, z0 = encode(ps, L, x, eps, training)
    series = rk4_series(gen_dynamics(node_flat, N, H), z0, times, nsteps)
    return decode_loss(ps, series, data, mask, mu, logvar, w_kl)
