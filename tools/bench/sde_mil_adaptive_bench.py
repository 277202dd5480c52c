# The adaptive NeuralDSDE layer with the Milstein and four-stage SRI steps at BASELINE config 5's shape (state 32, hidden 64,
# B = 512, nfine = 128, abstol = reltol = tol): the recorded forward, wall time per call and per attempted step, median of 30
# after 3 warm-ups, in ONE session:
#   * Milstein through the one-launch kernel with the controller in its footer (k_sde_mil_fast; the default at this shape),
#   * the same inputs through the host-controlled loop on the generic kernel (LRNDE_SDE_HOST_LOOP=1) — the yardstick,
#   * SRI through its own one-launch kernel (k_sde_sri_fast; tools/bench/sde_sri_adaptive_bench.py compares it with its host loop).
#   python tools/bench/sde_mil_adaptive_bench.py [out.json] [tol]
# tol: 0.14 (config 5's) by default, for both kinds.
import json, os, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import lrnde_amd as P
from localregneuralde_jl_amd import _lib as L
from localregneuralde_jl_amd.layers import _mlp_desc
D, H, B, nfine = 32, 64, 512, 128
out = sys.argv[1] if len(sys.argv) > 1 else None
tol = float(sys.argv[2]) if len(sys.argv) > 2 else 0.14
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


def measure(label, tol, host_loop, **kw):
    P.set_option("LRNDE_SDE_HOST_LOOP", int(host_loop))
    try:
        ts = []
        for i in range(33):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fw = h.node_forward_record(x, Wd, 0.0, 1.0, tol, tol, z_local=z, mode="unbiased", t1_or_rand=0.37, saveat=(), save_start=-1, **kw)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            if i >= 3: ts.append(t1 - t0)
    finally:
        P.set_option("LRNDE_SDE_HOST_LOOP", 0)
    st = fw["stats"]
    att = st["naccept"] + st["nreject"]
    r = dict(label=label, tol=tol, forward_ms=float(np.median(ts) * 1e3), attempted=att, accepted=st["naccept"],
             us_per_attempt=float(np.median(ts) / att * 1e6), u_end_sum=float(fw["u_end"].double().sum()))
    print(f"{label}: forward+record {r['forward_ms']:.3f} ms ({att} attempted, {st['naccept']} accepted steps: {r['us_per_attempt']:.1f} us per attempt)", flush=True)
    return r


rows = [measure("milstein fused (k_sde_mil_fast, device controller)", tol, False, solver="RKMil"),
        measure("milstein host-controlled loop (k_sde_rkmil)", tol, True, solver="RKMil"),
        measure("sri fused (k_sde_sri_fast, device controller)", tol, False, solver="SRI", tableau=tab, path_z=Zd, z_local2=z2)]
assert rows[0]["u_end_sum"] == rows[1]["u_end_sum"] and rows[0]["attempted"] == rows[1]["attempted"]   # the same solve on both routes
if out:
    with open(out, "w") as f:
        json.dump(dict(shape=dict(D=D, H=H, B=B, nfine=nfine), reps=30, warmup=3, rows=rows), f, indent=1)
