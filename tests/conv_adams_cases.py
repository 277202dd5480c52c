"""Cases of the conv handle's VCAB3 / VCABM3 tests (tests/test_gpu_conv_adams.py, tests/test_host_conv_adams.py), importable
without a GPU.

Inputs follow test_gpu_conv._case (glorot x scale, BN scale in [0.5, 1.5], bias in [-0.3, 0.3], C = 8, Hc = 64) through its
restatement conv_sharded_cases._inputs.  Which branches a case reaches (a rejected multistep attempt, a rejected start-up
attempt, an accepted step that carries two saveat points) was found on the CPU with the oracle's ConvField; the host test
re-derives it, and also that no attempted step of a case that is compared with ConvField on the GPU has an error estimate
within 5 % of the accept threshold — the condition for asserting equal accept patterns across two f-eval implementations."""
import numpy as np

from conv_sharded_cases import C, HC, N1, _field, _inputs

SAVEAT = [0.0, 0.37, 0.37, 0.8, 1.0]   # a point at the start, a duplicate, interpolated points, the end as a copy
SOLVERS = ("vcab3", "vcabm3")
MAX_ATTEMPTS = 150

# name -> W, H, B, seed, weight scale, tolerance, training-mode BatchNorm, activation
CASES = {
    "plain16": dict(W=16, H=16, B=2, seed=5, scale=1.5, tol=1e-4, train=True),    # two strips per image
    "plain8": dict(W=8, H=8, B=4, seed=21, scale=2.0, tol=1e-3, train=True),
    "ragged": dict(W=12, H=8, B=5, seed=9, scale=3.0, tol=1e-4, train=True),      # odd batch, 96-pixel strips
    # rejected multistep attempts: test-mode BatchNorm with _case's running statistics
    "rej_8x8_s7": dict(W=8, H=8, B=3, seed=7, scale=4.0, tol=1e-2, train=False),   # vcab3 rejects
    "rej_8x4_s3": dict(W=8, H=4, B=2, seed=3, scale=4.0, tol=1e-2, train=False),   # vcabm3 rejects
    "rej_8x8_s1": dict(W=8, H=8, B=3, seed=1, scale=4.0, tol=1e-2, train=False),   # vcabm3 rejects
    # a rejected start-up attempt: kick_inputs
    "kick": dict(W=8, H=8, B=2, seed=3, scale=None, tol=1e-3, train=False, act="tanh"),
}
ORACLE_CASES = ("plain16", "plain8", "ragged")   # compared with the oracle's own conv f-evals on the GPU
MULTISTEP_REJECTS = {"vcab3": ("rej_8x8_s7",), "vcabm3": ("rej_8x4_s3", "rej_8x8_s1")}
DTYPE_CASE, OTHER_DTYPE = "plain8", "bf16"
# the pullback case of test_conv_node_backward_matches_oracle
PULLBACK = dict(W=8, H=8, B=3, seed=41, scale=1.5, tol=1e-4, train=True)
BN_UNIT = np.concatenate([np.zeros(HC), np.ones(HC), np.zeros(HC), np.ones(HC)]).astype(np.float32)


def kick_inputs(W=8, H=8, B=2, kappa=300.0, tstar=0.2, seed=3):
    """(p, u, running statistics): the conv analogue of chain_adams_cases.kick_inputs.  conv1's t-channel has only its centre
    tap, kappa (1 + 0.2 N(0,1)) per output channel, and BN1's bias is -tap t* (1 + 0.3 N(0,1)): with tanh and unit running
    statistics every hidden channel swings from one saturation to the other around t = t*.  The start-up steps grow dt on a
    flat field and run into the swing."""
    import oracle as O
    rng = np.random.default_rng(seed)
    p = O.glorot_conv_params(C, HC, seed=seed).astype(np.float32)
    tap = (kappa * (1.0 + 0.2 * rng.standard_normal(HC))).astype(np.float32)
    w1 = p[:N1].reshape(HC, C + 1, 3, 3)   # [out][in, the t channel last][ky][kx]
    w1[:, C, :, :] = 0.0
    w1[:, C, 1, 1] = tap
    p[N1 + HC:N1 + 2 * HC] = (-tap * tstar * (1.0 + 0.3 * rng.standard_normal(HC))).astype(np.float32)
    u = rng.standard_normal((B, C, H, W)).astype(np.float32)
    return p, u, BN_UNIT.copy()


def inputs(c):
    """(p, u, running statistics or None, activation) of a case dict"""
    act = c.get("act", "gelu")
    if c["scale"] is None:
        return kick_inputs(c["W"], c["H"], c["B"], seed=c["seed"]) + (act,)
    return _inputs(c["W"], c["H"], c["B"], c["seed"], c["train"], c["scale"]) + (act,)


def oracle_field(c):
    """a fresh oracle ConvField of the case (its running statistics start at 0 / 1) and the flat state"""
    p, u, st, act = inputs(c)
    return _field(c["W"], c["H"], p, st, act, c["train"]), u.reshape(c["B"], -1)


def handle(c, dtype="f32", stream=None):
    """a fresh ConvHandle of the case and its state on the device"""
    import torch
    from conv_sharded_cases import _handle
    p, u, st, act = inputs(c)
    return _handle(c["W"], c["H"], p, st, act, c["train"], dtype, stream), torch.from_numpy(u).cuda()


def coverage(trace, saveat=SAVEAT, t0=0.0, t1=1.0):
    """what a solve's trace rows reach: attempts, rejected multistep attempts, the accepted-step counts at which attempts
    were rejected, the largest number of saveat points inside one accepted step, the smallest distance of an EEst from 1"""
    sv = [np.float32(s) for s in saveat if np.float32(s) > np.float32(t0)]
    acc = multi = 0
    rej_at, per_step = [], []
    rows = list(trace)
    for k, r in enumerate(rows):
        if not r["accepted"]:
            rej_at.append(acc)
            multi += acc >= 2
            continue
        acc += 1
        tend = rows[k + 1]["t"] if k + 1 < len(rows) else np.float32(t1)
        per_step.append(sum(1 for s in sv if r["t"] < s <= tend))
    margin = min(abs(float(r["eest"]) - 1.0) for r in rows)
    return dict(attempts=len(rows), multistep_rejects=multi, rejected_at=rej_at, startup_rejects=sum(1 for a in rej_at if a < 2),
                max_points_in_a_step=max(per_step) if per_step else 0, margin=margin)
