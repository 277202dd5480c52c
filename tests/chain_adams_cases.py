"""Shapes and inputs of the Dense-chain VCAB3 / VCABM3 tests (tests/test_gpu_chain_adams.py, tests/test_host_chain_adams.py),
importable without a GPU.

The GPU tests hold the one-launch-per-attempt kernel (csrc/lrnde_chain_adams.hpp) to the C oracle's adams_solve run around the
handle's own f-evals.  Which branches a case reaches (a rejected multistep attempt, a rejected start-up attempt, an accepted
step without a saveat point directly after one with two) depends on its inputs; they were picked on the CPU with the oracle
over the float32 numpy field below, and the host test re-derives that before anyone spends a GPU run on a drifted case."""
import numpy as np

SAVEAT = [0.0, 0.31, 0.31, 0.77, 1.0]   # a duplicate, two interpolated points, the end point as a copy
SOLVERS = ("vcab3", "vcabm3")
MAX_ATTEMPTS = 400


def models(P):
    phys = [P.Dense(20, 40, "tanh") if i % 2 == 0 else P.Dense(40, 20, "tanh") for i in range(8)]
    return {
        "physionet": P.Chain(P.Activation("tanh"), *phys),                                          # gen_dynamics, construct.jl:236-244
        "td3": P.TDChain(P.Chain(P.Dense(33, 64, "tanh"), P.Dense(65, 64, "tanh"), P.Dense(65, 32))),  # the time row
        "one_layer": P.Chain(P.Dense(8, 8, "tanh")),
        "width_7": P.Chain(P.Activation("tanh"), P.Dense(7, 7, "tanh"), P.Dense(7, 7)),             # odd out: the padded row
        "w128_td": P.TDChain(P.Chain(P.Dense(129, 128, "tanh"))),                                   # two elements per thread
        "sixteen": P.Chain(P.Activation("gelu"), *[P.Dense(24, 24, "tanh") for _ in range(16)]),
        "td_kick": P.TDChain(P.Chain(P.Dense(9, 8, "tanh"))),                                       # kick_inputs: a start-up rejection
        "small3": P.Chain(P.Dense(12, 12, "tanh"), P.Dense(12, 12, "tanh"), P.Dense(12, 12)),       # the float64 comparisons
    }


# name -> (model, B, weight scale, tolerance).  B = 17: three workgroups, the last with one column; 8: one full tile; 1.
CASES = {
    "physionet_b17": ("physionet", 17, 3.0, 1e-5),
    "physionet_b8": ("physionet", 8, 1.0, 1e-3),
    "physionet_b1": ("physionet", 1, 3.0, 1e-4),
    "td3": ("td3", 11, 2.0, 1e-4),
    "one_layer": ("one_layer", 5, 12.0, 1e-2),
    "width_7": ("width_7", 10, 3.0, 1e-4),
    "w128_td_b9": ("w128_td", 9, 2.0, 1e-4),
    "sixteen": ("sixteen", 6, 2.0, 1e-4),
    "td_kick": ("td_kick", 5, None, 1e-3),
}


def spec(model):
    """(td, input activation, [(in, out, act)]) of a chain model"""
    from localregneuralde_jl_amd.layers import Activation, TDChain
    td = isinstance(model, TDChain)
    ia = model.layers[0].activation if isinstance(model.layers[0], Activation) else "identity"
    return td, ia, [(l.in_dims - int(td), l.out_dims, l.activation) for l in model.layers if not isinstance(l, Activation)]


def inputs(P, model, B, scale, seed=0):
    """(p, x): glorot_chain_params x scale plus a little noise (no zero biases), x uniform in (-1, 1)"""
    p = P.glorot_chain_params(model, seed=seed, scale=scale)
    p = (p + np.random.default_rng(seed + 1).standard_normal(p.size).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    D = spec(model)[2][0][0]
    x = (np.random.default_rng(seed + 2).random((B, D), dtype=np.float32) - np.float32(0.5)) * np.float32(2)
    return p, x


def kick_inputs(B, kappa=300.0, tstar=0.2, seed=3):
    """(p, x) of "td_kick": f = tanh(W u + w_t (t - ~tstar)), |w_t| ~ kappa — every component swings from one saturation
    to the other around t = tstar.  The start-up steps grow dt on a flat field and run into the swing: the cheapest
    start-up rejection found (a stiff field that rejects there takes thousands of attempts over the span)."""
    rng = np.random.default_rng(seed)
    W = (0.5 * rng.standard_normal((8, 8))).astype(np.float32)
    wt = (kappa * (1.0 + 0.2 * rng.standard_normal(8))).astype(np.float32)
    b = (-wt * tstar * (1.0 + 0.3 * rng.standard_normal(8))).astype(np.float32)
    Wf = np.concatenate([W, wt[:, None]], 1)   # out x (in + 1): the t column last
    p = np.concatenate([Wf.T.reshape(-1), b]).astype(np.float32)
    x = ((rng.random((B, 8), dtype=np.float32) - np.float32(0.5)) * np.float32(2)).astype(np.float32)
    return p, x


def case(P, name):
    mname, B, scale, tol = CASES[name]
    model = models(P)[mname]
    p, x = kick_inputs(B) if mname == "td_kick" else inputs(P, model, B, scale)
    return model, p, x, tol


_ACT = {"identity": lambda z: z, "tanh": np.tanh,
        "gelu": lambda z: z / (1.0 + np.exp(-1.5957691216057308 * z * (1.0 + 0.044715 * z * z)))}


def np_field(model, p):
    """the field in float32 numpy (another summation order than the kernels'): what the cases were picked with"""
    td, ia, ls = spec(model)
    Wb, o = [], 0
    for i, n, _a in ls:
        W = np.asarray(p[o:o + n * (i + td)], np.float32).reshape(i + td, n).T
        o += n * (i + td)
        Wb.append((W, np.asarray(p[o:o + n], np.float32)))
        o += n
    assert o == len(p)

    def f(u, t):
        h = _ACT[ia](np.asarray(u, np.float32)).astype(np.float32)
        for (W, b), (i, _n, a) in zip(Wb, ls):
            z = h @ W[:, :i].T + b
            if td:
                z = z + np.float32(t) * W[:, i]
            h = _ACT[a](z.astype(np.float32)).astype(np.float32)
        return h
    return f


def coverage(trace, saveat=SAVEAT, t0=0.0):
    """what a solve's trace rows (t, dt, eest, accepted) reach: rejected multistep attempts, rejected start-up attempts
    (the Bogacki-Shampine attempts: fewer than two steps accepted so far), and whether an accepted step with no saveat point follows directly one with two"""
    sv = [np.float32(s) for s in saveat if np.float32(s) > np.float32(t0)]
    acc = multi_rej = start_rej = 0
    counts = []
    rows = [r for r in trace]
    for k, r in enumerate(rows):
        if not r["accepted"]:
            if acc < 2:
                start_rej += 1
            else:
                multi_rej += 1
            continue
        acc += 1
        # the step ends where the next attempt starts (the last one at the span's end)
        nxt = [q["t"] for q in rows[k + 1:]]
        tend = nxt[0] if nxt else np.float32(saveat[-1])
        counts.append(sum(1 for s in sv if r["t"] < s <= tend))
    two_then_none = any(a == 2 and b == 0 for a, b in zip(counts, counts[1:]))
    return dict(attempts=len(rows), multistep_rejects=multi_rej, startup_rejects=start_rej, two_then_none=two_then_none)
