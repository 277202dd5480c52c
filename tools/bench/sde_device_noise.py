# Device-drawn SDE noise (lrnde_sde_draw_noise) at BASELINE config 5, set up as bench.py's sde_layer_leg
# (state 32, hidden 64, B = 512, nfine = 256, abstol = reltol = 0.14, :unbiased):
#   * generation time of the path W (257 x 512 x 32) and of the local step's z: HIP events, warmed, median of 100;
#   * the handle-level forward (node_forward_record on a resident path, wall time around synchronisations as sde_layer_leg);
#   * NeuralDSDE.__call__ with noise_source="host" and "device", alternating in the same process (parameters and x resident).
#   python tools/bench/sde_device_noise.py [reps]       -> a readable table and one JSON line
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import lrnde_amd as P
from localregneuralde_jl_amd.layers import _mlp_desc

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
D, H, B, nfine, tol = 32, 64, 512, 256, 0.14
f32 = np.float32
rng = np.random.default_rng(0)
lim1, lim2 = np.sqrt(6.0 / (D + H)), np.sqrt(6.0 / (H + D))
pd = np.concatenate([(rng.random(H * D, dtype=f32) * 2 - 1) * f32(lim1), np.zeros(H, f32),
                     (rng.random(D * H, dtype=f32) * 2 - 1) * f32(lim2), np.zeros(D, f32)]).astype(f32)
pg = np.concatenate([(rng.random(D * D, dtype=f32) * 2 - 1) * f32(np.sqrt(6.0 / (2 * D))), np.zeros(D, f32)]).astype(f32)
x = torch.from_numpy(rng.standard_normal((B, D)).astype(f32)).cuda()
h = P.SdeHandle(_mlp_desc(P.Chain(P.Dense(D, H, "tanh"), P.Dense(H, D))))
h.set_params(pd, pg)
scale = f32(np.sqrt(f32(1.0 / nfine)))
seed = 0x243F6A8885A308D3


def events(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        fn()
    out = []
    for _ in range(n):
        e0.record(); fn(); e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(out))


gen_W_us = events(lambda: h.draw_noise(seed, 0, nfine, B, scale, True), 100)
gen_inc_us = events(lambda: h.draw_noise(seed, 2, nfine, B, scale, False), 100)
gen_z_us = events(lambda: h.draw_noise(seed, 1, 1, B, 1.0, False), 100)
# the handle forward gets exactly what the device layer below draws from its st: the seed's W and z, then its t1
st = {"drift": {}, "diffusion": {}, "rng": np.random.default_rng(1), "training": True}
rep = np.random.default_rng(1)
seed = int(rep.integers(0, 2 ** 64, dtype=np.uint64))
t1 = float(f32(f32(rep.random(dtype=f32)) * f32(1.0)))
Wd = h.draw_noise(seed, 0, nfine, B, scale, True)
zd = h.draw_noise(seed, 1, 1, B, 1.0, False)[0]


def wall(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


handle_fwd = lambda: h.node_forward_record(x, Wd, 0.0, 1.0, tol, tol, z_local=zd, mode="unbiased", t1_or_rand=t1, saveat=(), save_start=-1)
solve_ms = events(handle_fwd, 50) / 1e3
ps = dict(drift=torch.from_numpy(pd).cuda(), diffusion=torch.from_numpy(pg).cuda())
layers = {src: P.NeuralDSDE(P.Chain(P.Dense(D, H, "tanh"), P.Dense(H, D)), P.Dense(D, D), nfine=nfine, abstol=tol, reltol=tol,
                            regularize="unbiased", noise_source=src) for src in ("host", "device")}
for lay in layers.values():
    for _ in range(3):
        lay(x, ps, st)
sol_dev, _ = layers["device"](x, ps, st)
fw = handle_fwd()
assert torch.equal(sol_dev.u[-1], fw["u_end"]), "the device layer and the handle forward solved different problems"
steps = fw["stats"]["naccept"] + fw["stats"]["nreject"]
dev = layers["device"]
# where the device layer's time goes beyond the handle forward: its per-call parameter upload and the two draws (wall)
parts = {"set_params": lambda: dev.handle().set_params(ps["drift"], ps["diffusion"]),
         "draws": lambda: (dev.handle().draw_noise(seed, 0, nfine, B, scale, True), dev.handle().draw_noise(seed, 1, 1, B, 1.0, False))}
t = {"handle": [], "host": [], "device": [], "set_params": [], "draws": []}
for i in range(reps):
    t["handle"].append(wall(handle_fwd))
    t["host"].append(wall(lambda: layers["host"](x, ps, st)))
    t["device"].append(wall(lambda: dev(x, ps, st)))
    for k, fn in parts.items():
        t[k].append(wall(fn))
med = {k: float(np.median(v)) for k, v in t.items()}
res = dict(what="device noise at BASELINE config 5 (D 32, H 64, B 512, nfine 256, tol 0.14, :unbiased)",
           gen_path_us=gen_W_us, gen_increments_us=gen_inc_us, gen_z_us=gen_z_us, handle_forward_event_ms=solve_ms,
           path_share_of_forward=gen_W_us / 1e3 / solve_ms,
           handle_forward_ms=med["handle"], layer_forward_host_noise_ms=med["host"], layer_forward_device_noise_ms=med["device"],
           device_over_handle=med["device"] / med["handle"], host_over_device=med["host"] / med["device"],
           set_params_wall_ms=med["set_params"], draws_wall_ms=med["draws"], attempted_steps=steps, reps=reps)
print(f"path W (257 x 512 x 32) {gen_W_us:.1f} us, increments {gen_inc_us:.1f} us, z {gen_z_us:.1f} us "
      f"({100 * res['path_share_of_forward']:.1f} % of the handle forward's {solve_ms:.3f} ms by events)")
print(f"forward wall ms (median of {reps}): handle {med['handle']:.3f}, layer device noise {med['device']:.3f} "
      f"(x{res['device_over_handle']:.2f}), layer host noise {med['host']:.3f} (x{res['host_over_device']:.1f} the device layer)")
print(f"device layer beyond the handle forward: set_params {med['set_params']:.3f} ms, the two draws {med['draws']:.3f} ms (wall, each alone)")
print(json.dumps(res))
