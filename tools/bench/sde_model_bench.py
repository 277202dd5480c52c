"""The MNIST-SDE model at BASELINE config 5 (784 -> 32, hidden 64, 10 classes, B = 512, abstol = reltol = 0.14).  Prints one JSON
object (kept as profiles/sde_model/bench.json).  Not part of bench.py.

  downsample : lrnde_sde_dense_forward / lrnde_sde_dense_backward against torch.addmm / (torch.mm + sum) in fp32 on the same
               tensors.  One repetition = device events around [the call, a stream synchronisation] for BOTH sides (the library
               call ends in one, so the torch side gets one too); the alternatives alternate inside every repetition.
  step       : run_sde_training_step (one forward solve, the pullback from its record) against what the package offered before
               it for the same result: torch.addmm -> NeuralDSDE forward -> a torch head and its autograd -> NeuralDSDE.pullback
               (which solves again) -> torch.mm for the downsample cotangent.  Same parameters, batch and layer state.

    python tools/bench/sde_model_bench.py [--reps 30] [--out profiles/sde_model/bench.json]
    python tools/bench/sde_model_bench.py --only ours|parent --steps 20      # a bare loop of steps, for a profiler"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import lrnde_amd as P  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    torch.cuda.current_stream().synchronize()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleaved(fns, reps, warm):
    """{name: [ms per repetition]}; every repetition runs each alternative once, in turn"""
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            out[k].append(event_ms(f))
    return out


def summary(ts):
    return dict(median_ms=round(statistics.median(ts), 5), min_ms=round(min(ts), 5), max_ms=round(max(ts), 5),
                spread_ms=round(max(ts) - min(ts), 5), reps=len(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--tol", type=float, default=0.14)
    ap.add_argument("--w-reg", type=float, default=1.0)
    ap.add_argument("--only", choices=("ours", "parent"), default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Din, D, H, K, B = 784, 32, 64, 10, a.B
    model = P.construct_mlp_sde(Din, D, H, K, abstol=a.tol, reltol=a.tol, nfine=128, regularize="unbiased")
    p0 = P.glorot_mlp_sde_params(model, seed=0)
    ps = dict(downsample=torch.from_numpy(p0["downsample"]).cuda(), neural_dsde={k: torch.from_numpy(v).cuda() for k, v in p0["neural_dsde"].items()},
              classifier=torch.from_numpy(p0["classifier"]).cuda())
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.random((B, Din), dtype=np.float32)).cuda()
    lab = torch.from_numpy(rng.integers(0, K, B).astype(np.int32)).cuda()
    lab64 = lab.long()
    du0 = torch.from_numpy(rng.standard_normal((B, D)).astype(np.float32)).cuda()
    st = model.initialstates(np.random.default_rng(2))
    nsde, h = model.neural_dsde, model.neural_dsde.handle()
    pd = ps["downsample"]
    Wt, bt = pd[:D * Din].view(Din, D), pd[D * Din:]          # x @ Wt + b: the Lux block read as (Din, D) row-major
    Wc, bc = ps["classifier"][:K * D].view(D, K), ps["classifier"][K * D:]

    def ours():
        return P.run_sde_training_step(model, ps, st, x, lab, a.w_reg)

    def parent():
        sn = st["neural_dsde"]
        u0 = torch.addmm(bt, x, Wt)
        sol, sn2 = nsde(u0, ps["neural_dsde"], sn)
        ue = sol.u[-1].detach().requires_grad_(True)
        wc, bcl = Wc.detach().requires_grad_(True), bc.detach().requires_grad_(True)
        ce = torch.nn.functional.cross_entropy(ue @ wc + bcl, lab64)
        ce.backward()
        dx, dps, _ = nsde.pullback(u0, ps["neural_dsde"], sn, ue.grad, w_reg=a.w_reg)
        dWd, dbd = x.t() @ dx, dx.sum(0)
        loss = float(ce) + a.w_reg * float(sn2["reg_val"])
        return loss, (dWd, dbd, dps, wc.grad, bcl.grad)

    if a.only:
        f = ours if a.only == "ours" else parent
        for _ in range(a.steps):
            f()
        torch.cuda.synchronize()
        print(json.dumps(dict(path=a.only, steps=a.steps)))
        return

    res = dict(shape=dict(Din=Din, D=D, H=H, K=K, B=B), tol=a.tol, w_reg=a.w_reg, reps=a.reps, warm=a.warm)
    # the two paths compute the same step: same loss, same downsample cotangent up to the summation order
    lo, _, _, go, _ = ours()
    lp, gp = parent()
    res["same_result"] = dict(loss_ours=float(lo), loss_parent=float(lp),
                              downsample_rel_diff=float((go["downsample"][:D * Din].view(Din, D) - gp[0]).norm() / gp[0].norm()),
                              drift_rel_diff=float((go["neural_dsde"]["drift"] - gp[2]["drift"]).norm() / gp[2]["drift"].norm()))
    dn = interleaved({"ours_forward": lambda: h.dense_forward(x, pd), "torch_addmm": lambda: torch.addmm(bt, x, Wt),
                      "ours_backward": lambda: h.dense_backward(x, pd, du0), "torch_mm_sum": lambda: (du0.t() @ x, du0.sum(0))},
                     a.reps, a.warm)
    res["downsample"] = {k: summary(v) for k, v in dn.items()}
    for ours_k, torch_k, name in (("ours_forward", "torch_addmm", "forward"), ("ours_backward", "torch_mm_sum", "backward")):
        o, t = res["downsample"][ours_k], res["downsample"][torch_k]
        res["downsample"][name + "_meets_bar"] = bool(o["median_ms"] <= t["median_ms"] + t["spread_ms"])
    stp = interleaved({"ours": ours, "parent": parent}, a.reps, a.warm)
    res["step"] = {k: summary(v) for k, v in stp.items()}
    o, p = res["step"]["ours"], res["step"]["parent"]
    res["step"]["gain_ms"] = round(p["median_ms"] - o["median_ms"], 5)
    res["step"]["faster_by_more_than_parent_spread"] = bool(p["median_ms"] - o["median_ms"] > p["spread_ms"])
    # the layer alone, for scale: one recorded forward, one pullback from the record
    u0 = h.dense_forward(x, pd)
    fw = interleaved({"layer_forward": lambda: nsde(u0, ps["neural_dsde"], st["neural_dsde"])}, a.reps, a.warm)
    res["layer_forward"] = summary(fw["layer_forward"])
    res["note"] = ("device events around [call, stream synchronisation]; alternatives alternate inside each repetition; spread = max - min; "
                   "bar for the downsample kernels: our median <= torch's median + torch's spread; for the step: parent median - our median > parent spread")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
