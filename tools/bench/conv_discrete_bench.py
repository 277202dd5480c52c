"""The two methods of the conv handle's pullback — the reversed Tsit5 solve (the default) and the discrete adjoint over the
step record (ConvHandle.set_sensealg("discrete"), csrc/lrnde_conv_discrete.hpp) — measured in one process and one session
at the CIFAR block: 32x32x8, B = 256, f32, train-mode BatchNorm, tol 1e-4, unbiased / error_estimate, pullback of
<g, sol.u[end]> + 2.5 reg_val with g ~ 1e-3 N(0,1); inputs as bench.py's conv_measure draws them.

  python tools/bench/conv_discrete_bench.py [--reps 10] [--warmup 2] [--out profiles/conv_discrete/conv_discrete_bench.json]
      per method: forward + pullback ms (device events; median, min, max) and the backward's nf, accepted / rejected steps;
      the recorded forward alone; how far the two gradients are apart (they differentiate the same map up to the solver's
      tolerance)"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

W = H = 32
B = 256
TOL = 1e-4
T1 = 0.41
W_REG = 2.5
METHODS = ("interpolating", "discrete")


def setup():
    import torch
    import lrnde_amd as P
    params = P.glorot_conv_params(8, 64, seed=0)
    xh = np.random.default_rng(0).standard_normal((B, 8, H, W)).astype(np.float32)
    x = torch.from_numpy(xh).cuda()
    g = torch.from_numpy((np.random.default_rng(2).standard_normal(xh.shape) * 1e-3).astype(np.float32)).cuda()
    h = P.ConvHandle(W, H, 8, 64, act="gelu", bn_train=True, compute_dtype="f32")
    h.set_params(params)
    return torch, h, x, g


def timed(torch, fn, reps, warmup):
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return out, dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)), reps=reps)


def rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).abs().max() / b.abs().max())


def bench(args):
    torch, h, x, g = setup()

    def forward():
        return h.node_forward_record(x, 0.0, 1.0, TOL, TOL, mode="unbiased", t1_or_rand=T1, maxiters=10000)

    fw, tf = timed(torch, forward, args.reps, args.warmup)
    res, grads = {}, {}
    for m in METHODS:
        h.set_sensealg(m)

        def both():
            f = forward()
            return f, h.node_backward_recorded(B, g, w_reg=W_REG)
        (fr, bw), tb = timed(torch, both, args.reps, args.warmup)
        sb = bw["stats_bwd"]
        grads[m] = (bw["dx"], bw["dp"])
        res[m] = dict(forward_plus_pullback_ms=tb, pullback_ms_median=tb["median"] - tf["median"],
                      backward=dict(nf=sb["nf"], naccept=sb["naccept"], nreject=sb["nreject"]))
        print(m, json.dumps(res[m]), flush=True)
    st = fw["stats"]
    out = dict(setup=f"CIFAR block {W}x{H}x8, B={B}, f32, train-mode BatchNorm, abstol=reltol={TOL:g}, tspan=(0,1), unbiased / error_estimate, "
                     f"t1={T1}, pullback of <g, sol.u[end]> + {W_REG} reg_val (g ~ 1e-3 N(0,1)); one process, device events",
               device=torch.cuda.get_device_name(0), us_per_feval=h.bench_rhs(x, 0.3, reps=20),
               forward=dict(recorded_forward_ms=tf, nf=st["nf"], naccept=st["naccept"], nreject=st["nreject"], record_steps=len(h.record_steps()[0])),
               methods=res,
               discrete_against_interpolating=dict(dx=rel(grads["discrete"][0], grads["interpolating"][0]),
                                                   dp=rel(grads["discrete"][1], grads["interpolating"][1]),
                                                   measure="max |a - b| / max |b|"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_discrete", "conv_discrete_bench.json"))
    bench(ap.parse_args())
