"""Wide Dense-chain field bench (lrnde_create_wide_chain) at B = 512, abstol = reltol = 1.4e-8, :unbiased.

Prints one JSON line (and writes it to --out) with, each the median of --reps runs after 3 warm-ups, timed by device events:
  (a) mnist2  TDChain [784,100,784] through the wide handle: us per attempted step of the solve, layer forward ms;
  (b) the same model through the MLP handle with the 4-column family switched off (LRNDE_NO_QTILE, DESIGN.md 4.6: the
      16-column k_step<W> family) and with the default routing;
  (c) mnist3  TDChain [784,100,100,784] through the wide handle: step, layer forward, forward + pullback;
  (d) mnist3's adaptive Tsit5 solve written in eager torch fp32 on the same GPU (host-side controller, one EEst read-back
      per attempted step).
  (e) --only adjoint: case (c)'s forward + pullback with the host-controlled adjoint loop (adjoint_loop="auto") and with the
      device-controlled one (adjoint_loop="device") in the same process: attempts of the reversed solve,
      launches per attempt, host waits, and us per attempt = (forward + pullback - layer forward) / attempts; and, third,
      with the discrete adjoint over the step record (adjoint_loop="discrete"): recorded steps walked,
      launches, host waits, us per recorded step.  Same process, same inputs.
"us per attempted step" is the solve's kernel time (the library's event bracket around its launches,
lrnde_last_solve_kernel_ms) over accepted + rejected steps.

    python tools/bench/wide_chain_bench.py [--reps 30] [--B 512] [--out profiles/wide_chain/wide_chain_bench.json]
    rocprofv3 --kernel-trace --stats -- python tools/bench/wide_chain_bench.py --only mnist3 --reps 5 --no-eager
    python tools/bench/wide_chain_bench.py --only adjoint --out profiles/wide_chain/wide_discrete_bench.json
    rocprofv3 --kernel-trace --stats -- python tools/bench/wide_chain_bench.py --only adjoint --reps 5
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lrnde_amd as P  # noqa: E402
from localregneuralde_jl_amd import _lib as L  # noqa: E402

TOL = 1.4e-8
WARM = 3
A = [[0.161], [-0.008480655492356989, 0.335480655492357], [2.8971530571054935, -6.359448489975075, 4.3622954328695815],
     [5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525],
     [5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383],
     [0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774]]
CS = [0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0]
BT = [-0.00178001105222577714, -0.0008164344596567469, 0.007880878010261995, -0.1447110071732629,
      0.5823571654525552, -0.45808210592918697, 0.015151515151515152]


def td_chain(dims, acts):
    return P.TDChain(P.Chain(*[P.Dense(dims[l] + 1, dims[l + 1], acts[l]) for l in range(len(dims) - 1)]))


def timed(fn, reps):
    """median / min / max ms of fn() between two device events, after WARM warm-ups"""
    ms = []
    for i in range(reps + WARM):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= WARM:
            ms.append(e0.elapsed_time(e1))
    return dict(median=round(statistics.median(ms), 4), min=round(min(ms), 4), max=round(max(ms), 4))


def leg(model, field, xd, ps, reps, pullback):
    node = P.NeuralODE(model, regularize="unbiased", abstol=TOL, reltol=TOL, save_start=False, maxiters=100000, field=field)
    st = node.initialstates(np.random.default_rng(0))
    h = node._bind(ps)
    h.solve(xd, 0.0, 1.0, TOL, TOL, saveat=[1.0], maxiters=100000)
    h.last_solve_kernel_ms()   # (the first call switches the solve's event bracket on)
    per, r = [], None
    for i in range(reps + WARM):
        r = h.solve(xd, 0.0, 1.0, TOL, TOL, saveat=[1.0], maxiters=100000)
        ms, _ = h.last_solve_kernel_ms()
        if i >= WARM:
            per.append(1e3 * ms / max(r["stats"]["naccept"] + r["stats"]["nreject"], 1))
    out = dict(naccept=r["stats"]["naccept"], nreject=r["stats"]["nreject"],
               us_per_attempted_step=dict(median=round(statistics.median(per), 3), min=round(min(per), 3), max=round(max(per), 3)),
               layer_forward_ms=timed(lambda: node(xd, ps, st), reps))
    if pullback:
        cot = torch.from_numpy(np.random.default_rng(1).standard_normal(tuple(xd.shape)).astype(np.float32)).cuda()
        out["layer_forward_pullback_ms"] = timed(lambda: node.pullback(xd, ps, st, cot, w_reg=10.0), reps)
        out["adjoint"] = h.last_adjoint_info()
    node._handle.close()
    return out


def adjoint_legs(model, xd, ps, reps):
    """case (c)'s forward + pullback under both continuous adjoint loops of the wide handle, host loop first, then under its
    discrete adjoint"""
    cot = torch.from_numpy(np.random.default_rng(1).standard_normal(tuple(xd.shape)).astype(np.float32)).cuda()
    out = {}
    keys = {"auto": "host_loop", "device": "device_loop", "discrete": "discrete_sweep"}
    for loop in ("auto", "device", "discrete"):
        node = P.NeuralODE(model, regularize="unbiased", abstol=TOL, reltol=TOL, save_start=False, maxiters=100000,
                           field="wide_chain", adjoint_loop=loop)
        st = node.initialstates(np.random.default_rng(0))
        fwd = timed(lambda: node(xd, ps, st), reps)
        both = timed(lambda: node.pullback(xd, ps, st, cot, w_reg=10.0), reps)
        _, _, info = node.pullback(xd, ps, st, cot, w_reg=10.0)
        ai, sb = node.handle().last_adjoint_info(), info["stats_bwd"]
        attempts = sb["naccept"] + sb["nreject"]
        out[keys[loop]] = dict(
            adjoint_loop=info["adjoint_loop"], layer_forward_ms=fwd, layer_forward_pullback_ms=both, attempts=attempts,
            naccept=sb["naccept"], nreject=sb["nreject"], launches=ai["launches"],
            launches_per_attempt=round(ai["launches"] / max(attempts, 1), 2), host_waits=ai["host_waits"],
            us_per_attempt=round(1e3 * (both["median"] - fwd["median"]) / max(attempts, 1), 2))
        node._handle.close()
    h, d = out["host_loop"]["layer_forward_pullback_ms"], out["device_loop"]["layer_forward_pullback_ms"]
    out["device_over_host_pullback"] = round(d["median"] / h["median"], 3)
    out["device_below_host_by_more_than_the_spread"] = bool(d["max"] < h["min"])
    # (the discrete row's "attempts" are the recorded steps it walked: naccept = the forward's, nreject = 0)
    s = out["discrete_sweep"]["layer_forward_pullback_ms"]
    out["discrete_over_device_pullback"] = round(s["median"] / d["median"], 3)
    out["discrete_below_device_by_more_than_the_spread"] = bool(s["max"] < d["min"] and d["min"] - s["max"] > max(s["max"] - s["min"], d["max"] - d["min"]))
    return out


def eager_solve(Ws, acts, x, t0, t1, tol, maxiters=100000):
    """adaptive Tsit5 (initdt, PI controller with the same constants) over the TDChain in eager torch fp32: the baseline"""
    fa = {"tanh": torch.tanh, "identity": lambda z: z}

    def f(u, t):
        h = u
        for (W, wt, b), a in zip(Ws, acts):
            h = fa[a](torch.addmm(b + t * wt, h, W.t()))
        return h

    def sc(a, b=None):
        m = a.abs() if b is None else torch.maximum(a.abs(), b.abs())
        return tol + m * tol
    rms = lambda v: float(torch.sqrt((v * v).mean()))
    u, t = x, t0
    k1 = f(u, t)
    d0, d1 = rms(u / sc(u)), rms(k1 / sc(u))
    dt0 = 1e-6 if d0 < 1e-5 or d1 < 1e-5 else 0.01 * d0 / d1
    d2 = rms((f(u + dt0 * k1, t + dt0) - k1) / sc(u)) / dt0
    dt = min(100 * dt0, 10 ** (-(2 + np.log10(max(d1, d2, 1e-15))) / 5), t1 - t0)
    qold, nacc, nrej = 1e-4, 0, 0
    for _ in range(maxiters):
        if t >= t1:
            break
        dt = min(dt, t1 - t)
        ks = [k1]
        for s in range(6):
            acc = ks[0] * A[s][0]
            for j in range(1, s + 1):
                acc = acc + ks[j] * A[s][j]
            y = u + dt * acc
            ks.append(f(y, t + CS[s] * dt))
        utilde = dt * sum(b * k for b, k in zip(BT, ks))
        eest = rms(utilde / sc(u, y))
        q = max(0.1, min(5.0, eest ** 0.14 / qold ** 0.08 / 0.9)) if eest > 0 else 0.1
        if eest <= 1.0:
            u, k1, t, qold, nacc = y, ks[6], t + dt, max(eest, 1e-4), nacc + 1
            dt = dt / q
        else:
            nrej += 1
            dt = dt / min(5.0, eest ** 0.14 / 0.9)
    return u, nacc, nrej


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--B", type=int, default=512)
    ap.add_argument("--only", choices=["all", "mnist2", "mnist3", "adjoint"], default="all")
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    B = args.B
    x = (np.random.default_rng(2).random((B, 784), dtype=np.float32) - np.float32(0.5)) * np.float32(2)
    xd = torch.from_numpy(x).cuda()
    res = dict(workload="wide_dense_chain", B=B, tol=TOL, reps=args.reps, warmups=WARM)
    if args.only in ("all", "mnist2"):
        m2 = td_chain([784, 100, 784], ["tanh", "identity"])
        ps2 = torch.from_numpy(P.glorot_chain_params(m2, seed=0)).cuda()
        res["a_mnist2_wide"] = leg(m2, "wide_chain", xd, ps2, args.reps, False)
        L.set_option("LRNDE_NO_QTILE", 1)
        res["b_mnist2_mlp_16col"] = leg(m2, "auto", xd, ps2, args.reps, False)
        L.set_option("LRNDE_NO_QTILE", 0)
        res["b_mnist2_mlp_default"] = leg(m2, "auto", xd, ps2, args.reps, False)
        res["a_over_b16_step"] = round(res["a_mnist2_wide"]["us_per_attempted_step"]["median"] /
                                       res["b_mnist2_mlp_16col"]["us_per_attempted_step"]["median"], 3)
    if args.only in ("all", "mnist3"):
        acts = ["tanh", "tanh", "identity"]
        m3 = td_chain([784, 100, 100, 784], acts)
        p3 = P.glorot_chain_params(m3, seed=0)
        ps3 = torch.from_numpy(p3).cuda()
        res["c_mnist3_wide"] = leg(m3, "wide_chain", xd, ps3, args.reps, True)
        if not args.no_eager:
            Ws, o = [], 0
            for l in m3.layers:
                n, k = l.out_dims, l.in_dims
                W = p3[o:o + n * k].reshape(k, n).T
                Ws.append((torch.from_numpy(W[:, :k - 1].copy()).cuda(), torch.from_numpy(W[:, k - 1].copy()).cuda(),
                           torch.from_numpy(p3[o + n * k:o + n * k + n].copy()).cuda()))
                o += n * k + n
            info = {}

            def run():
                info["u"], info["na"], info["nr"] = eager_solve(Ws, acts, xd, 0.0, 1.0, TOL)
            res["d_mnist3_eager_torch_fp32_solve_ms"] = timed(run, args.reps)
            res["d_eager_naccept"], res["d_eager_nreject"] = info["na"], info["nr"]
    if args.only == "adjoint":
        m3 = td_chain([784, 100, 100, 784], ["tanh", "tanh", "identity"])
        ps3 = torch.from_numpy(P.glorot_chain_params(m3, seed=0)).cuda()
        res["workload"] = "wide_dense_chain_adjoint"
        res["c_mnist3_wide_adjoint"] = adjoint_legs(m3, xd, ps3, args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
