# The adaptive NeuralDSDE layer with the four-stage SRI step at BASELINE config 5's shape (state 32, hidden 64, B = 512,
# nfine = 128, abstol = reltol = 0.14): the recorded forward, wall time per call and per attempted step, in ONE session on
#   * the default route: one launch per attempted step (k_sde_sri_fast) with the controller in its footer, and
#   * LRNDE_SDE_HOST_LOOP=1: the host-controlled loop on lrnde_sde_sri_step (two k_sde_dw, k_sri_chi, eight f-evals, three
#     k_sri_stage, k_sri_final, a copy and a stream sync per attempt) — the route every SRI solve took before, the yardstick.
# A run is the median of 30 calls after 3 warm-ups; the two routes alternate for `rounds` runs each (5 by default) and the
# JSON holds every run's median, and per route the median, minimum and maximum over the runs.  The fused route stays the
# default only if its per-attempt median lies below the yardstick's minimum ("fused_below_yardstick_min").
#   python tools/bench/sde_sri_adaptive_bench.py [out.json] [--rounds N] [--route both|fused|host] [--mode unbiased|none]
# (--route fused --mode none --rounds 1 under `rocprofv3 --kernel-trace --stats` shows the solve's launches alone: the
#  device loop enqueues k_sde_sri_fast in batches of eight, so its row counts the attempts rounded up, plus the launches
#  that found the solve finished.)
import argparse, json, os, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import lrnde_amd as P
from localregneuralde_jl_amd import _lib as L
from localregneuralde_jl_amd.layers import _mlp_desc
ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--route", default="both", choices=("both", "fused", "host"))
ap.add_argument("--mode", default="unbiased", choices=("unbiased", "none"))
ap.add_argument("--tol", type=float, default=0.14)
a = ap.parse_args()
D, H, B, nfine = 32, 64, 512, 128
f32 = np.float32
rng = np.random.default_rng(0)
h = P.SdeHandle(_mlp_desc(P.Chain(P.Dense(D, H, "tanh"), P.Dense(H, D))))
npd = D * H + H + H * D + D
pd = (rng.standard_normal(npd) * 0.3).astype(f32); pg = (rng.standard_normal(D * D + D) * 0.05).astype(f32)
h.set_params(pd, pg)
x = torch.from_numpy(rng.standard_normal((B, D)).astype(f32)).cuda()
hh = f32(1.0 / nfine)
path = lambda: torch.from_numpy(np.concatenate([np.zeros((1, B, D), f32), np.cumsum((rng.standard_normal((nfine, B, D)) * np.sqrt(hh)).astype(f32),
                                                                                   axis=0, dtype=f32)], axis=0)).cuda()
Wd, Zd = path(), path()
z = torch.from_numpy(rng.standard_normal((B, D)).astype(f32)).cuda()
z2 = torch.from_numpy(rng.standard_normal((B, D)).astype(f32)).cuda()
trng = np.random.default_rng(41)
tab = [float(f32(trng.uniform(-0.6, 0.9) * 0.1)) for _ in L.SRI_FIELDS]


def run(host_loop):
    P.set_option("LRNDE_SDE_HOST_LOOP", int(host_loop))
    try:
        ts = []
        for i in range(33):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fw = h.node_forward_record(x, Wd, 0.0, 1.0, a.tol, a.tol, z_local=z, mode=a.mode, t1_or_rand=0.37, saveat=(), save_start=-1,
                                       solver="SRI", tableau=tab, path_z=Zd, z_local2=z2)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            if i >= 3: ts.append(t1 - t0)
        info = h.last_solve_info()
    finally:
        P.set_option("LRNDE_SDE_HOST_LOOP", 0)
    st = fw["stats"]
    att = st["naccept"] + st["nreject"]
    return dict(forward_ms=float(np.median(ts) * 1e3), us_per_attempt=float(np.median(ts) / att * 1e6), attempted=att, accepted=st["naccept"],
                u_end_sum=float(fw["u_end"].double().sum()), reg_val=float(fw["reg_val"]), info=info)


routes = dict(fused=("sri fused (k_sde_sri_fast, device controller)", False), host=("sri host-controlled loop (lrnde_sde_sri_step)", True))
want = ("fused", "host") if a.route == "both" else (a.route,)
runs = {k: [] for k in want}
for r in range(a.rounds):
    for k in want:
        runs[k].append(run(routes[k][1]))
        print(f"round {r} {routes[k][0]}: forward+record {runs[k][-1]['forward_ms']:.3f} ms, {runs[k][-1]['attempted']} attempted, "
              f"{runs[k][-1]['us_per_attempt']:.1f} us per attempt, {runs[k][-1]['info']}", flush=True)
rows = []
for k in want:
    pa = [q["us_per_attempt"] for q in runs[k]]; fm = [q["forward_ms"] for q in runs[k]]
    rows.append(dict(route=k, label=routes[k][0], kind=runs[k][0]["info"]["kind"], attempted=runs[k][0]["attempted"], accepted=runs[k][0]["accepted"],
                     us_per_attempt=dict(median=float(np.median(pa)), min=min(pa), max=max(pa), runs=pa),
                     forward_ms=dict(median=float(np.median(fm)), min=min(fm), max=max(fm), runs=fm),
                     u_end_sum=runs[k][0]["u_end_sum"], reg_val=runs[k][0]["reg_val"]))
    print(f"{routes[k][0]}: per attempt median {rows[-1]['us_per_attempt']['median']:.1f} us (min {min(pa):.1f}, max {max(pa):.1f}); "
          f"forward median {rows[-1]['forward_ms']['median']:.3f} ms (min {min(fm):.3f}, max {max(fm):.3f})", flush=True)
res = dict(shape=dict(D=D, H=H, B=B, nfine=nfine), tol=a.tol, mode=a.mode, reps=30, warmup=3, rounds=a.rounds, rows=rows)
if a.route == "both":
    f_, h_ = rows
    assert f_["kind"] == 1 and h_["kind"] == 0, (f_["kind"], h_["kind"])
    assert f_["u_end_sum"] == h_["u_end_sum"] and f_["attempted"] == h_["attempted"] and f_["reg_val"] == h_["reg_val"]   # the same solve on both routes
    res["fused_below_yardstick_min"] = bool(f_["us_per_attempt"]["median"] < h_["us_per_attempt"]["min"])
    print("fused per-attempt median below the yardstick's minimum:", res["fused_below_yardstick_min"], flush=True)
if a.out:
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
