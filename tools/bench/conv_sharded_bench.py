"""What one MI355X can say about the batch-sharded conv handle; several GPUs: not measured.

(a) the UNSHARDED handle's f-eval (lrnde_conv_bench_rhs, 32x32, B=256, fp32) of this tree's liblrnde.so against a library
    built from the parent commit (--parent-lib), alternating the two in one process.  The unsharded path is meant to be
    launch-for-launch what it was: the two must agree within the spread of the parent's own repeats, and give equal bits.
(b) the same f-eval and one node_forward on a handle that joined a ONE-rank RCCL communicator (LRNDE_FORCE_COMM), against
    the unsharded handle: the price per f-eval of the two extra launch pairs (rank sums + all-reduce) with nobody to
    talk to.  There is no target.

  python tools/bench/conv_sharded_bench.py --parent-lib /path/to/parent/liblrnde.so --out profiles/conv/sharded_onerank.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import lrnde_amd as P  # noqa: E402
from localregneuralde_jl_amd import _lib as L  # noqa: E402

W = H = 32
B = 256


class RawConv:
    """an unsharded conv handle over a given liblrnde.so (the parent's has no communicator entry points)"""
    NAMES = ("lrnde_conv_create", "lrnde_conv_destroy", "lrnde_conv_set_params", "lrnde_conv_rhs", "lrnde_conv_bench_rhs")

    def __init__(self, path, params):
        self.lib = C.CDLL(path)
        table = {n: (res, args) for n, res, args in L.SYMBOLS}
        for n in self.NAMES:
            getattr(self.lib, n).restype, getattr(self.lib, n).argtypes = table[n]
        self.desc = L.ConvDesc(W, H, 8, 64, L.ACT["gelu"], 1, L.DTYPE["f32"], 1e-5)
        self.ctx = C.c_void_p()
        self.stream = torch.cuda.current_stream()
        self._chk(self.lib.lrnde_conv_create(C.byref(self.ctx), C.byref(self.desc), torch.cuda.current_device(),
                                             C.c_void_p(self.stream.cuda_stream)))
        self.params = params
        self._chk(self.lib.lrnde_conv_set_params(self.ctx, C.c_void_p(params.data_ptr()), params.numel()))

    @staticmethod
    def _chk(rc):
        if rc != 0:
            raise RuntimeError(f"liblrnde status {rc}")

    def rhs(self, u, t):
        du = torch.empty_like(u)
        self._chk(self.lib.lrnde_conv_rhs(self.ctx, C.c_void_p(u.data_ptr()), float(t), u.shape[0], C.c_void_p(du.data_ptr())))
        return du

    def bench_rhs(self, u, t, reps):
        us = C.c_float()
        self._chk(self.lib.lrnde_conv_bench_rhs(self.ctx, C.c_void_p(u.data_ptr()), float(t), u.shape[0], int(reps), C.byref(us)))
        return float(us.value)

    def close(self):
        self.lib.lrnde_conv_destroy(self.ctx)


def summary(xs):
    return dict(samples=[round(x, 3) for x in xs], median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3),
                spread=round(max(xs) - min(xs), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="liblrnde.so built from the parent commit (part (a))")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv", "sharded_onerank.json"))
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--reps", type=int, default=100)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("conv_sharded_bench needs a GPU: nothing here can be measured without one")
    torch.manual_seed(0)
    params = torch.from_numpy(P.glorot_conv_params(8, 64, seed=0)).cuda()
    u = torch.randn(B, 8, H, W, device="cuda")
    res = dict(shape=dict(W=W, H=H, B=B, dtype="f32"), device=torch.cuda.get_device_name(0), reps_per_sample=a.reps,
               several_gpus="not measured")

    # ---- (a) unsharded f-eval: this tree against the parent, alternating ----
    if a.parent_lib:
        cur, par = RawConv(L.LIB_PATH, params), RawConv(a.parent_lib, params)
        same_bits = bool(torch.equal(cur.rhs(u, 0.3), par.rhs(u, 0.3)))
        for h in (par, cur):
            h.bench_rhs(u, 0.3, a.reps)  # warm-up of each library's code objects
        t_par, t_cur = [], []
        for _ in range(a.rounds):
            t_par.append(par.bench_rhs(u, 0.3, a.reps))
            t_cur.append(cur.bench_rhs(u, 0.3, a.reps))
        sp, sc = summary(t_par), summary(t_cur)
        res["a_unsharded_feval_us"] = dict(parent=sp, this_commit=sc, median_difference=round(sc["median"] - sp["median"], 3),
                                           within_parent_spread=bool(abs(sc["median"] - sp["median"]) <= sp["spread"]),
                                           equal_bits=same_bits)
        cur.close(); par.close()
    else:
        res["a_unsharded_feval_us"] = "not measured (no --parent-lib)"

    # ---- (b) one forced-RCCL rank against unsharded ----
    def handle():
        h = P.ConvHandle(W, H, 8, 64, act="gelu", bn_train=True)
        h.set_params(params)
        return h

    hu, hf = handle(), handle()
    os.environ["LRNDE_FORCE_COMM"] = "1"
    os.environ.pop("LRNDE_GATHER_TILES", None)
    P.init_comm(hf, 0, 1)
    assert hf.comm_count() == (1, 1) and hu.comm_count() == (1, 0)
    for h in (hu, hf):
        h.bench_rhs(u, 0.3, a.reps)
    t_u, t_f = [], []
    for _ in range(a.rounds):
        t_u.append(hu.bench_rhs(u, 0.3, a.reps))
        t_f.append(hf.bench_rhs(u, 0.3, a.reps))
    su, sf = summary(t_u), summary(t_f)
    res["b_feval_us"] = dict(unsharded=su, one_forced_rccl_rank=sf, price_per_feval_us=round(sf["median"] - su["median"], 3))

    tol = 1e-3
    bn0 = np.concatenate([np.zeros(64), np.ones(64), np.zeros(64), np.ones(64)]).astype(np.float32)

    def fwd_ms(h):
        h.set_bn_state(bn0)
        torch.cuda.synchronize()
        tic = time.perf_counter()
        r = h.node_forward(u, 0.0, 1.0, tol, tol, mode="unbiased", t1_or_rand=0.41)
        torch.cuda.synchronize()
        return (time.perf_counter() - tic) * 1e3, r

    fwd_ms(hu); fwd_ms(hf)
    m_u, m_f = [], []
    for _ in range(max(3, a.rounds // 2)):
        tu, ru = fwd_ms(hu); tf, rf = fwd_ms(hf)
        m_u.append(tu); m_f.append(tf)
    n0 = hf.comm_stats()
    _, rf = fwd_ms(hf)
    n1 = hf.comm_stats()
    res["b_node_forward_ms"] = dict(unsharded=summary(m_u), one_forced_rccl_rank=summary(m_f), nfe=int(rf["nfe"]), tol=tol,
                                    exchanges_per_call=n1[0] - n0[0], bytes_per_call=n1[1] - n0[1],
                                    equal_bits=bool(torch.equal(ru["u_end"], rf["u_end"]) and ru["reg_val"] == rf["reg_val"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
