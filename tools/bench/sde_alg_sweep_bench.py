# The pullback of the adaptive NeuralDSDE layer with the Milstein and the four-stage SRI step at BASELINE config 5's shape
# (state 32, hidden 64, B = 512, nfine = 128, abstol = reltol = 0.14, :unbiased, w_reg = 1): lrnde_sde_node_backward_recorded
# from one record, wall time per call, in ONE process on
#   * the default route: the one-launch reverse sweep (k_sde_alg_bwd_fused / k_sde_alg_reg_fused, lrnde_sde_bwd_alg_fused.hpp), and
#   * LRNDE_NO_SDE_BWD_FUSED=1: launch sequences per recorded step (sde_node_backward_alg) — the route every Milstein / SRI
#     record took before, the yardstick.
# Per (kind, route): median, minimum and maximum of 30 calls after 3 warm-ups (tools/bench/wide_chain_bench.py's protocol), with
# what SdeHandle.last_backward_info() says ran.  The sweep stays the default for a kind only if its MAXIMUM lies below the
# yardstick's MINIMUM ("sweep_max_below_per_step_min": disjoint ranges).
#   python tools/bench/sde_alg_sweep_bench.py [out.json] [--kind both|RKMil|SRI] [--route both|sweep|per-step] [--reps N]
# (--route sweep --reps 3 under `rocprofv3 --kernel-trace --stats` shows the sweep's launches alone.)
import argparse, json, os, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import lrnde_amd as P
from localregneuralde_jl_amd import _lib as L
from localregneuralde_jl_amd.layers import _mlp_desc
ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--kind", default="both", choices=("both", "RKMil", "SRI"))
ap.add_argument("--route", default="both", choices=("both", "sweep", "per-step"))
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--tol", type=float, default=0.14)
a = ap.parse_args()
D, H, B, nfine, W_REG, WARM = 32, 64, 512, 128, 1.0, 3
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
KW = dict(RKMil=dict(solver="RKMil"), SRI=dict(solver="SRI", tableau=tab, path_z=Zd, z_local2=z2))


def measure(kind, per_step):
    fw = h.node_forward_record(x, Wd, 0.0, 1.0, a.tol, a.tol, z_local=z, mode="unbiased", t1_or_rand=0.37, saveat=(), save_start=-1, **KW[kind])
    du = torch.from_numpy(np.random.default_rng(5).standard_normal(tuple(fw["u"].shape)).astype(f32)).cuda()
    P.set_option("LRNDE_NO_SDE_BWD_FUSED", int(per_step))
    try:
        ts = []
        for i in range(WARM + a.reps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            bw = h.node_backward_recorded(du, w_reg=W_REG)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            if i >= WARM: ts.append((t1 - t0) * 1e3)
        info = h.last_backward_info()
    finally:
        P.set_option("LRNDE_NO_SDE_BWD_FUSED", 0)
    K = fw["stats"]["naccept"]
    return dict(kind=kind, route="per-step" if per_step else "sweep", recorded_steps=K, series=int(fw["u"].shape[0]), reg_val=float(fw["reg_val"]),
                backward_ms=dict(median=float(np.median(ts)), min=float(min(ts)), max=float(max(ts))), info=info,
                norms={k: float(bw[k].double().norm()) for k in ("dx", "dp_drift", "dp_diff")})


kinds = ("RKMil", "SRI") if a.kind == "both" else (a.kind,)
routes = (False, True) if a.route == "both" else ((a.route == "per-step"),)
rows, verdict = [], {}
for kind in kinds:
    got = {}
    for per_step in routes:
        r = measure(kind, per_step)
        rows.append(r); got[per_step] = r
        m = r["backward_ms"]
        print(f"{kind} {r['route']}: K = {r['recorded_steps']}, pullback median {m['median']:.3f} ms (min {m['min']:.3f}, max {m['max']:.3f}), {r['info']}", flush=True)
    if len(got) == 2:
        assert got[False]["info"]["kind"] == 1 and got[True]["info"]["kind"] == 0, (got[False]["info"], got[True]["info"])
        for k, v in got[False]["norms"].items():       # the same gradients on both routes, to fp32 rounding
            assert abs(v - got[True]["norms"][k]) <= 1e-5 * abs(got[True]["norms"][k]), (kind, k, v, got[True]["norms"][k])
        verdict[kind] = bool(got[False]["backward_ms"]["max"] < got[True]["backward_ms"]["min"])
        print(f"{kind}: the sweep's maximum below the per-step route's minimum: {verdict[kind]}", flush=True)
res = dict(shape=dict(D=D, H=H, B=B, nfine=nfine), tol=a.tol, mode="unbiased", w_reg=W_REG, reps=a.reps, warmup=WARM, rows=rows,
           sweep_max_below_per_step_min=verdict)
if a.out:
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
