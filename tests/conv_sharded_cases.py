"""Case recipes and helpers of the batch-sharded conv handle's tests (tests/test_gpu_conv_sharded.py,
tests/test_gpu_conv_sharded_envelope.py, tests/test_host_conv_sharded.py): the input recipe of test_gpu_conv._case
restated, the two yardsticks' constructors, R handles joined through the in-process local communicator, the two distance
measures — and, for the envelope file, the solve cases it selects with the oracle's own answers for them, computed once
and shared (read-only).  Importing this module needs no GPU; the handle helpers do when they are called."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

C, HC = 8, 64
N1 = 9 * (C + 1) * HC; N2 = N1 + 2 * HC; N3 = N2 + 9 * (HC + 1) * HC; N4 = N3 + 2 * HC
BLOCKS = (("w1", slice(0, N1)), ("bn1", slice(N1, N2)), ("w2", slice(N2, N3)), ("bn2", slice(N3, N4)), ("w3", slice(N4, None)))
BN0 = np.concatenate([np.zeros(HC), np.ones(HC), np.zeros(HC), np.ones(HC)]).astype(np.float32)
MODES = [("unbiased", "error_estimate"), ("biased", "stiffness_estimate"), ("none", "error_estimate")]


def _mods():
    import lrnde_amd as P
    import oracle as O
    return P, O


@functools.lru_cache(maxsize=None)
def _inputs(W, H, B, seed, train=True, scale=1.0):
    """test_gpu_conv._case's recipe: (params, state, running statistics or None)"""
    P, O = _mods()
    rng = np.random.default_rng(seed)
    p = O.glorot_conv_params(C, HC, seed=seed) * np.float32(scale)
    p[N1:N1 + HC] = rng.uniform(0.5, 1.5, HC); p[N1 + HC:N2] = rng.uniform(-0.3, 0.3, HC)
    p[N3:N3 + HC] = rng.uniform(0.5, 1.5, HC); p[N3 + HC:N4] = rng.uniform(-0.3, 0.3, HC)
    p = p.astype(np.float32)
    u = rng.standard_normal((B, C, H, W)).astype(np.float32)
    st = None
    if not train:
        st = np.concatenate([rng.normal(0, 0.2, HC), rng.uniform(0.5, 2, HC), rng.normal(0, 0.2, HC),
                             rng.uniform(0.5, 2, HC)]).astype(np.float32)
    return p, u, st


def _field(W, H, p, st, act="gelu", train=True, bf16=False):
    P, O = _mods()
    return O.ConvField(W, H, C, HC, p, act=act, bn_train=train, bn_state=st, nthreads=8, bf16=bf16)


def _handle(W, H, p, st, act="gelu", train=True, dtype="f32", stream=None):
    P, O = _mods()
    h = P.ConvHandle(W, H, C, HC, act=act, bn_train=train, compute_dtype=dtype, stream=stream)
    if st is not None:
        h.set_bn_state(st)
    h.set_params(p)
    return h


def _ranks(R, W, H, p, st, act="gelu", train=True, dtype="f32", gather=False):
    """R handles on their own streams, joined to one local communicator"""
    P, O = _mods()
    old = os.environ.pop("LRNDE_GATHER_TILES", None)
    if gather:
        os.environ["LRNDE_GATHER_TILES"] = "1"
    try:
        lc = P.LocalComm(R)
        hs = []
        for r in range(R):
            h = _handle(W, H, p, st, act, train, dtype, stream=torch.cuda.Stream())
            lc.join(h, r)
            hs.append(h)
    finally:
        os.environ.pop("LRNDE_GATHER_TILES", None)
        if old is not None:
            os.environ["LRNDE_GATHER_TILES"] = old
    torch.cuda.synchronize()
    return lc, hs


def _shards(a, R):
    P, O = _mods()
    out = [torch.from_numpy(np.ascontiguousarray(P.shard_columns(a, r, R))).cuda() for r in range(R)]
    torch.cuda.synchronize()
    return out


def _run(fns):
    P, O = _mods()
    out = P.run_ranks(fns)
    torch.cuda.synchronize()
    return out


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _dist(got, ref):
    """max abs error in units of the reference's scale (the measure of test_gpu_conv._close)"""
    got = _np(got); ref = np.asarray(ref).reshape(got.shape)
    return float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


def _rel(a, b):
    a, b = _np(a).astype(np.float64).ravel(), _np(b).astype(np.float64).ravel()
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


# ---- the envelope file's solve cases (tests/test_gpu_conv_sharded_envelope.py) -----------------------------------------
# Each is (R, B per rank, W, H, seed, scale, tol, training mode).  The figures behind "expect" are what the oracle gives on
# the global batch; tests/test_host_conv_sharded.py asserts them on the oracle alone, so that a changed seed or recipe
# cannot silently turn a case into another one.
TEST_MODE_CASE = (2, 2, 8, 8, 41, 1.5, 1e-4, False)     # expect: 6 / 0 forward, 12 / 0 adjoint (unbiased, w_reg 2.5)
BACKWARD_CASES = {                                       # expect: forward accepted / rejected, adjoint accepted / rejected
    "2x2@16x16": ((2, 2, 16, 16, 5, 1.5, 1e-3, True), (5, 0, 11, 0)),   # two strips per image
    "2x3@12x8": ((2, 3, 12, 8, 7, 1.5, 1e-3, True), (6, 0, 11, 0)),     # three images per rank, the MT = 6 kernels
}
STOP_CASE = (2, 2, 8, 8, 21, 2.0, 1e-3)                  # NaN: test mode, retcode 3, 1 iteration, 9 f-evals;
STOP_MAXITERS = 3                                        # maxiters: training mode, retcode 1, 3 accepted in 4 iterations
LONG_LIST = (2, 260, 8, 8)                               # 260 workgroups per rank: two trips of the 256-thread loops
STEM_SHAPES = {                                          # (R, B per rank, W, H): blocks of 256 pixels per rank
    "2x3@12x8": (2, 3, 12, 8),                           # 288 pixels: two blocks, the second ragged
    "3x2@16x16": (3, 2, 16, 16),                         # two full blocks
    "2x65@32x32": (2, 65, 32, 32),                       # 260 blocks (stem only)
}
W_REG = 2.5
T1 = 0.41
SAVEAT = (0.37, 1.0)


def cotangent(shape, seed=3):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        elif isinstance(v, dict):
            _frozen(v)
    return d


def at_threshold(trace):
    """an attempted step whose EEst lies in [0.98, 1.02]: there a last-bit difference may flip accept / reject"""
    e = trace["eest"]
    return bool(np.any((e >= 0.98) & (e <= 1.02)))


@functools.lru_cache(maxsize=None)
def oracle_solve(case, maxiters=1000):
    """O.solve on the global batch with saveat = SAVEAT (trace included)"""
    P, O = _mods()
    R, Bl, W, H, seed, scale, tol, train = case
    B = R * Bl
    p, u, st = _inputs(W, H, B, seed, train, scale)
    ro = O.solve(_field(W, H, p, st, train=train), u.reshape(B, -1), 0.0, 1.0, tol, tol, saveat=list(SAVEAT), maxiters=maxiters)
    return _frozen(ro)


@functools.lru_cache(maxsize=None)
def oracle_node_forward(case, mode, reg_type):
    P, O = _mods()
    R, Bl, W, H, seed, scale, tol, train = case
    B = R * Bl
    p, u, st = _inputs(W, H, B, seed, train, scale)
    return _frozen(O.node_forward(_field(W, H, p, st, train=train), u.reshape(B, -1), 0.0, 1.0, tol, tol, mode=mode, reg_type=reg_type,
                                  t1_or_rand=T1))


@functools.lru_cache(maxsize=None)
def oracle_node_backward(case, mode="unbiased", w_reg=W_REG):
    """O.node_backward on the global batch for the cotangent of `cotangent` (maxiters 5000, t1 = T1)"""
    P, O = _mods()
    R, Bl, W, H, seed, scale, tol, train = case
    B = R * Bl
    p, u, st = _inputs(W, H, B, seed, train, scale)
    wv = cotangent(u.shape)
    bo = O.node_backward(_field(W, H, p, st, train=train), u.reshape(B, -1), 0.0, 1.0, tol, tol, wv.reshape(B, -1), mode=mode,
                         t1_or_rand=T1, w_reg=w_reg, maxiters=5000)
    return _frozen(bo)


def step_counts(bo):
    """(forward accepted, rejected, adjoint accepted, rejected) of a node_backward result"""
    return (bo["stats_fwd"]["naccept"], bo["stats_fwd"]["nreject"], bo["stats_bwd"]["naccept"], bo["stats_bwd"]["nreject"])


def stop_inputs(kind):
    """(params, state, running statistics or None, training mode, maxiters) of a stop-code case.  "nan": test mode, one NaN
    pixel in the LAST image — test-mode BatchNorm has no cross-sample sum, so the NaN stays inside that image: rank 0's own
    data is finite and only the exchanged norm is NaN.  "maxiters": training mode, three iterations allowed."""
    R, Bl, W, H, seed, scale, tol = STOP_CASE
    train = kind == "maxiters"
    p, u, st = _inputs(W, H, R * Bl, seed, train, scale)
    if kind == "nan":
        u = u.copy()
        u[-1, 3, 4, 5] = np.nan
    return p, u, st, train, (STOP_MAXITERS if train else 1000)


@functools.lru_cache(maxsize=None)
def oracle_stop(kind):
    P, O = _mods()
    R, Bl, W, H, seed, scale, tol = STOP_CASE
    p, u, st, train, maxiters = stop_inputs(kind)
    B = R * Bl
    ro = O.solve(_field(W, H, p, st, train=train), u.reshape(B, -1), 0.0, 1.0, tol, tol, saveat=[1.0], maxiters=maxiters)
    fo = O.node_forward(_field(W, H, p, st, train=train), u.reshape(B, -1), 0.0, 1.0, tol, tol, mode="unbiased", t1_or_rand=T1,
                        maxiters=maxiters)
    return _frozen(dict(solve=ro, fwd=fo))


EIGHT = (8, 1, 8, 8, 16, 2.0)                            # R, B per rank, W, H, seed, scale of the eight-rank case
EIGHT_STEP = (0.1, 0.3, 1e-4)                            # t, dt, tol of its Tsit5 step (test_conv_init_dt_and_step_match_oracle's)


@functools.lru_cache(maxsize=None)
def eight_ranks_step_ref():
    """(dt, k1) of the oracle's init_dt and its Tsit5 step on the global batch of the eight-rank case"""
    P, O = _mods()
    R, Bl, W, H, seed, scale = EIGHT
    B = R * Bl
    p, u, st = _inputs(W, H, B, seed, True, scale)
    t, dt, tol = EIGHT_STEP
    fld = _field(W, H, p, None)
    dt_o, k1_o = O.init_dt(fld, u.reshape(B, -1), t, 1.0, tol, tol)
    so = O.tsit5_step(_field(W, H, p, None), u.reshape(B, -1), k1_o, t, dt, tol, tol)
    return dt_o, k1_o, _frozen(so)


# ---- exchange counts of whole calls (default form) -------------------------------------------------------
def exchanges_feval(train):
    return 2 if train else 0                  # the two BatchNorm statistics exchanges; test mode exchanges nothing


def exchanges_vjp_gp(train):
    return exchanges_feval(train) + 2 + 3     # the recompute, one per BatchNorm backward, one per weight block


def exchanges_init_dt(train):
    return 2 * exchanges_feval(train) + 2     # two f-evals, two norms


def exchanges_step(train):
    return 6 * exchanges_feval(train) + 1     # six f-evals, one norm


def exchanges_node_forward(stats, mode, train):
    """what a node_forward that returned `stats` must have issued: the solve's init_dt, one Tsit5 step per attempt
    (accepted or rejected), and — unless mode is "none" — the local step's init_dt and step"""
    n = exchanges_init_dt(train) + (stats["naccept"] + stats["nreject"]) * exchanges_step(train)
    if mode != "none":
        n += exchanges_init_dt(train) + exchanges_step(train)
    return n


def exchanges_adjoint(stats_bwd, mode, w_reg, train):
    """the recorded backward: the adjoint's start is an init_dt over [lambda; mu] whose two f-evals are VJPs with gp; every
    attempt is six such VJPs and one norm (43 in training mode, 31 in test mode); the regulariser term — unless mode is
    "none" or w_reg is zero — is an init_dt, one Tsit5 step and the six VJPs of its reverse sweep"""
    v = exchanges_vjp_gp(train)
    n = 2 * v + 2 + (stats_bwd["naccept"] + stats_bwd["nreject"]) * (6 * v + 1)
    if mode != "none" and w_reg != 0.0:
        n += exchanges_init_dt(train) + exchanges_step(train) + 6 * v
    return n


def exchanges_node_backward(stats_fwd, stats_bwd, mode, w_reg, train):
    return exchanges_node_forward(stats_fwd, mode, train) + exchanges_adjoint(stats_bwd, mode, w_reg, train)
