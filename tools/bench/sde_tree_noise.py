# The adaptive NeuralDSDE forward on the virtual Brownian tree (lrnde_sde_set_path_tree) against the array path,
# at BASELINE config 5 (state 32, hidden 64, B = 512, abstol = reltol = 0.14, :unbiased, Euler-Heun), in one process:
#   * nfine = 256: the handle-level forward (node_forward_record) on the tree, on a resident array, and the array's draw_noise;
#   * L = 12 and L = 16: the forward on the tree, beside the array's size and — where the array still fits (L = 12) — its
#     draw_noise time, the forward on it and the time of materialising the tree (tree_path).
# HIP events, warmed, median of 100.
#   python tools/bench/sde_tree_noise.py [out.json]       -> a readable table and one JSON line (also written to out.json)
import json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import lrnde_amd as P
from localregneuralde_jl_amd.layers import _mlp_desc

D, H, B, tol = 32, 64, 512, 0.14
f32 = np.float32
rng = np.random.default_rng(0)
lim1, lim2 = np.sqrt(6.0 / (D + H)), np.sqrt(6.0 / (H + D))
pd = np.concatenate([(rng.random(H * D, dtype=f32) * 2 - 1) * f32(lim1), np.zeros(H, f32),
                     (rng.random(D * H, dtype=f32) * 2 - 1) * f32(lim2), np.zeros(D, f32)]).astype(f32)
pg = np.concatenate([(rng.random(D * D, dtype=f32) * 2 - 1) * f32(np.sqrt(6.0 / (2 * D))), np.zeros(D, f32)]).astype(f32)
x = torch.from_numpy(rng.standard_normal((B, D)).astype(f32)).cuda()
h = P.SdeHandle(_mlp_desc(P.Chain(P.Dense(D, H, "tanh"), P.Dense(H, D))))
h.set_params(pd, pg)
seed = 0x243F6A8885A308D3
zd = h.draw_noise(seed, 1, 1, B, 1.0, False)[0]
N = 100


def events(fn, n=N):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        fn()
    out = []
    for _ in range(n):
        e0.record(); fn(); e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(out))


def forward(W, nfine, maxiters):
    return h.node_forward_record(x, W, 0.0, 1.0, tol, tol, z_local=zd, mode="unbiased", t1_or_rand=0.37, saveat=(), save_start=-1,
                                 maxiters=maxiters, nfine=nfine)


rows = []
for L in (8, 12, 16):
    nfine = 1 << L
    array_mb = (nfine + 1) * B * D * 4 / 1e6
    row = dict(L=L, nfine=nfine, array_MB=array_mb)
    h.set_path_tree(seed)
    fw = forward(None, nfine, 1000)
    row.update(attempted=fw["stats"]["naccept"] + fw["stats"]["nreject"], accepted=fw["stats"]["naccept"],
               tree_forward_us=events(lambda: forward(None, nfine, 1000)))
    row["tree_us_per_attempt"] = row["tree_forward_us"] / row["attempted"]
    h.clear_path_tree()
    if L <= 12:   # the array still fits: the tree's own array (the same solve), and what drawing an array of this size costs
        W = h.tree_path(seed, 6, L, B, 0.0, 1.0)
        fa = forward(W, nfine, 1000)
        assert torch.equal(fa["u_end"], fw["u_end"]) and fa["stats"] == fw["stats"], "the tree and its array solved different problems"
        row["array_forward_us"] = events(lambda: forward(W, nfine, 1000))
        row["array_us_per_attempt"] = row["array_forward_us"] / row["attempted"]
        row["tree_path_us"] = events(lambda: h.tree_path(seed, 6, L, B, 0.0, 1.0), 30)
        del W
        sc = f32(np.sqrt(f32(1.0 / nfine)))
        row["draw_noise_path_us"] = events(lambda: h.draw_noise(seed, 0, nfine, B, sc, True), 30)
        row["array_plus_draw_us"] = row["array_forward_us"] + row["draw_noise_path_us"]
        row["tree_over_array_plus_draw"] = row["tree_forward_us"] / row["array_plus_draw_us"]
        torch.cuda.empty_cache()
    rows.append(row)
    print(f"L={L:2d} nfine={nfine:6d} array {array_mb:8.1f} MB: tree forward {row['tree_forward_us']:9.1f} us ({row['attempted']} attempts, "
          f"{row['tree_us_per_attempt']:.1f} us each)" +
          (f"; array forward {row['array_forward_us']:.1f} us + draw_noise {row['draw_noise_path_us']:.1f} us = {row['array_plus_draw_us']:.1f} us "
           f"(tree x{row['tree_over_array_plus_draw']:.2f}); tree_path {row['tree_path_us']:.1f} us" if "array_forward_us" in row else ""))

res = dict(what="tree noise at BASELINE config 5 (D 32, H 64, B 512, tol 0.14, :unbiased, Euler-Heun; node_forward_record, HIP events, median of 100)",
           rows=rows)
print(json.dumps(res))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
