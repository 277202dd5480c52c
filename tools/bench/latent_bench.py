"""Latent-ODE layers at the PhysioNet shape (37/40/50/20, T = 49, B = 512): encoder forward, encoder backward, decode + loss and
one whole training step, each the median of 30 synchronised wall-clock runs after 5 warm-up runs, against the same float32
restatement (tests/latent_np.py) run as torch ops on the same GPU (one launch per op and per step; backward by autograd).
Prints one JSON line.  Not part of bench.py.

    python tools/bench/latent_bench.py [--B 512] [--T 49] [--reps 30] [--out profiles/latent/latent_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import latent_np as LN  # noqa: E402
import lrnde_amd as P   # noqa: E402


def median_ms(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(ts), 4), round(min(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=512)
    ap.add_argument("--T", type=int, default=49)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dims = (37, 40, 50, 20)
    I, H, Ld, N = dims
    B, T = a.B, a.T
    times = [float(np.float32((i + 1) / T)) for i in range(T)]
    model = P.construct_time_series(*dims, saveat=times, regularize="none", abstol=a.tol, reltol=a.tol, maxiters=10000)
    psn = P.glorot_latent_params(model, seed=0)
    ps = {k: torch.from_numpy(v).cuda() for k, v in psn.items()}
    rng = np.random.default_rng(1)
    data = torch.from_numpy(rng.standard_normal((B, T, I)).astype(np.float32)).cuda()
    mask = torch.from_numpy((rng.random((B, T, I)) < 0.3).astype(np.float32)).cuda()
    mask[:, 0, 0] = 1
    dt = torch.from_numpy((rng.random((B, T, 1)) * 0.02).astype(np.float32)).cuda()
    x = torch.cat([data, mask, dt], dim=2).contiguous()
    eps = torch.from_numpy(rng.standard_normal((B, N)).astype(np.float32)).cuda()
    series = torch.from_numpy(rng.standard_normal((T, B, N)).astype(np.float32)).cuda()
    cot = torch.from_numpy(rng.standard_normal((B, N)).astype(np.float32)).cuda()
    h = model.handle()
    h.set_params(ps["latent"])
    st = model.initialstates(np.random.default_rng(2))
    res = dict(shape=dims, B=B, T=T, reps=a.reps, tol=a.tol)

    res["encode_ms"] = median_ms(lambda: h.encode(x, eps), a.reps)

    def enc_bwd():
        h.encode(x, eps)
        h.encode_backward(x, dz0=cot, dmu=cot, dlogvar=cot, want_dx=False)
    res["encode_plus_backward_ms"] = median_ms(enc_bwd, a.reps)
    enc = h.encode(x, eps)
    res["decode_loss_ms"] = median_ms(lambda: h.decode_loss(series, data, mask, enc["mu"], enc["logvar"], 0.5), a.reps)
    res["training_step_ms"] = median_ms(lambda: P.run_latent_training_step(model, ps, st, (data, mask, dt), (0.0, 0.5)), a.reps)

    # the per-op form: the same float32 restatement as torch ops on this GPU
    torch.set_default_device("cuda")
    flat = ps["latent"].clone().requires_grad_(True)

    def t_fwd():
        with torch.no_grad():
            return LN.encode(LN.unflatten(flat, *dims), Ld, x, eps)

    def t_fwd_bwd():
        flat.grad = None
        _, mu, lv, z0 = LN.encode(LN.unflatten(flat, *dims), Ld, x, eps)
        ((z0 * cot).sum() + (mu * cot).sum() + (lv * cot).sum()).backward()

    def t_dec():
        flat.grad = None
        s = series.clone().requires_grad_(True)
        m, l = enc["mu"].clone().requires_grad_(True), enc["logvar"].clone().requires_grad_(True)
        LN.decode_loss(LN.unflatten(flat, *dims), s, data, mask, m, l, 0.5)[0].backward()
    res["torch_encode_ms"] = median_ms(t_fwd, a.reps)
    res["torch_encode_plus_backward_ms"] = median_ms(t_fwd_bwd, a.reps)
    res["torch_decode_loss_ms"] = median_ms(t_dec, a.reps)
    res["note"] = "each entry [median, min] ms of synchronised wall-clock runs; encode_backward alone = encode_plus_backward - encode"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
