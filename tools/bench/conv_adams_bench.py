"""Tsit5 / VCAB3 / VCABM3 as the global solver of the NeuralODE layer over the conv field, measured in one process and one
session at the CIFAR block: 32x32x8, B = 256, f32, train-mode BatchNorm, tol 1e-4, inputs as bench.py's conv_measure draws
them.  Writes profiles/conv_adams/bench.json.

  python tools/bench/conv_adams_bench.py [--reps 20] [--warmup 3] [--out profiles/conv_adams/bench.json]
      per solver: layer forward ms and forward + pullback ms (device events; median, min, max), nf, accepted / rejected
      steps, record bytes
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR/LEG -o ka -- python tools/bench/conv_adams_bench.py --trace-run LEG
      three forwards of one leg for the profiler (a run of its own per leg: no timing is taken here).  LEG: vcab3, vcabm3
      (mode none, no record) or vcab3_record, vcabm3_record (the recorded forward: VCAB3's residual kernel then also writes the
      attempt's P2 / P3 and its record kernel only copies, VCABM3's record kernel forms them)
  python tools/bench/conv_adams_bench.py --merge-stats DIR [--out ...]
      adds the per-kernel times of every DIR/LEG (the new elementwise kernels beside the f-eval's launches) to the JSON"""
import argparse
import csv
import glob
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

W = H = 32
B = 256
TOL = 1e-4
SOLVERS = ("tsit5", "vcab3", "vcabm3")
FEVAL = ("k_conv_wide_f32", "k_conv_out_f32", "k_bn_finalize_t")
ELEMENTWISE = ("k_cadams_pred", "k_cadams_resid", "k_cadams_bs3", "k_cadams_record", "k_cadams_eval", "k_lincomb4", "k_sums_err", "k_sums_init")


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


def bench(args):
    torch, h, x, g = setup()
    n = x.numel()
    t1 = 0.41
    res = {}
    for s in SOLVERS:
        h.set_solver(s)
        fw, tf = timed(torch, lambda: h.node_forward(x, 0.0, 1.0, TOL, TOL, mode="unbiased", t1_or_rand=t1, maxiters=10000), args.reps, args.warmup)

        def both():
            f = h.node_forward_record(x, 0.0, 1.0, TOL, TOL, mode="unbiased", t1_or_rand=t1, maxiters=10000)
            return f, h.node_backward_recorded(B, g, w_reg=2.5)
        (fr, bw), tb = timed(torch, both, args.reps, args.warmup)
        st = fw["stats"]
        arrays = 8 if s == "tsit5" else 4
        res[s] = dict(forward_ms=tf, forward_plus_pullback_ms=tb, nf=st["nf"], nfe=fw["nfe"], naccept=st["naccept"], nreject=st["nreject"],
                      record_bytes_used=4 * n * arrays * st["naccept"], record_bytes_allocated=4 * n * 8 * st["naccept"],
                      adjoint=dict(naccept=bw["stats_bwd"]["naccept"], nreject=bw["stats_bwd"]["nreject"], nf=bw["stats_bwd"]["nf"]),
                      reg_val=float(fw["reg_val"]))
        print(s, json.dumps(res[s]), flush=True)
    us = h.bench_rhs(x, 0.3, reps=20)
    out = dict(setup=f"CIFAR block {W}x{H}x8, B={B}, f32, train-mode BatchNorm, abstol=reltol={TOL:g}, tspan=(0,1), unbiased / error_estimate, "
                     f"t1={t1}, pullback of <g, sol.u[end]> + 2.5 reg_val (g ~ 1e-3 N(0,1)); one process, device events",
               device=torch.cuda.get_device_name(0), us_per_feval=us, state_floats=n, solvers=res)
    write(args.out, out)


LEGS = ("vcab3", "vcabm3", "vcab3_record", "vcabm3_record")


def trace_run(args):
    torch, h, x, g = setup()
    solver, _, rec = args.trace_run.partition("_")
    h.set_solver(solver)
    fn = h.node_forward_record if rec else h.node_forward
    for _ in range(3):
        fn(x, 0.0, 1.0, TOL, TOL, mode="none", maxiters=10000)
    torch.cuda.synchronize()


def leg_stats(d):
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))[0]
    rows = {}
    for r in csv.DictReader(open(f)):
        m = re.search(r"(k_\w+)", r["Name"])
        if not m or not m.group(1).startswith(FEVAL + ELEMENTWISE):
            continue
        e = rows.setdefault(m.group(1), dict(calls=0, total_ns=0.0))
        e["calls"] += int(r["Calls"]); e["total_ns"] += float(r["TotalDurationNs"])
    nfeval = max(1, sum(v["calls"] for k, v in rows.items() if k.startswith("k_conv_out_f32")))   # one conv3 launch per f-eval
    return dict(feval_us=round(sum(v["total_ns"] for k, v in rows.items() if k.startswith(FEVAL)) / 1e3 / nfeval, 2), fevals=nfeval,
                kernels={k: dict(calls=v["calls"], avg_us=round(v["total_ns"] / v["calls"] / 1e3, 2)) for k, v in sorted(rows.items())})


def merge_stats(args):
    out = json.load(open(args.out))
    out["kernel_trace"] = dict(run="rocprofv3 --kernel-trace --stats, one run per leg of --trace-run: three mode=none forwards of the leg's solver, "
                                   "plain or recorded",
                               legs={leg: leg_stats(os.path.join(args.merge_stats, leg)) for leg in LEGS
                                     if os.path.isdir(os.path.join(args.merge_stats, leg))})
    write(args.out, out)


def write(path, out):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_adams", "bench.json"))
    ap.add_argument("--trace-run", default=None, choices=LEGS)
    ap.add_argument("--merge-stats", default=None)
    a = ap.parse_args()
    if a.trace_run:
        trace_run(a)
    elif a.merge_stats:
        merge_stats(a)
    else:
        bench(a)
