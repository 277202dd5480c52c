"""Cases and torch references of the MNIST-SDE model (experiments/src/construct.jl:202-210), shared by
tests/test_host_sde_model.py and tests/test_gpu_sde_model.py.  Nothing here imports the package.

  downsample : u0 = x W^T + b, parameters [vec(W) (D x Din, column-major: W[o][k] at o + D*k); b (D)]
  model      : downsample -> the NeuralDSDE steps over a RECORDED grid (the accepted steps of a float32 run) -> Dense(D => K) on
               sol.u[end] -> logitcrossentropy + w_reg * reg_val of the recorded local step (its start state a constant)

Every array is compared with the float64 run under the suite's rule (latent_cases.bound): max(1e-5, 4 x the distance of the
float32 torch run from the float64 run), relative to the float64 value's norm."""
import numpy as np
import torch

import sde_adaptive_np as S
from head_cases import make_labels
from latent_cases import bound, rel  # noqa: F401  (the suite's rule, re-exported)
from test_gpu_sde_gradients import _eh_reg64, _eh_step64, _fields64, _mil_step64, _sri_step64

f32 = np.float32

# The downsample kernels' tile constants (csrc/lrnde_sde_model.hpp): the forward holds 16 samples x 64 outputs per workgroup,
# eight waves each summing one K segment of 4 * ceil(ceil(Din / 4) / 8) values in staged trips of 64; the backward sums the
# batch in groups of 4 samples, eight waves taking the groups in turn (a round = 32 samples), four groups per loop trip
# (128 samples).  The table of the issue with its rows moved onto those edges — (Din, D, B): why.
DENSE_CASES = [
    (1, 32, 5),       # Din below the MFMA depth 4; scalar staging
    (3, 16, 3),       # Din < 4, D on one tile, B below a group
    (4, 17, 4),       # Din on the depth (vector staging), D one past a tile, B on a group
    (5, 1, 1),        # Din past the depth, a single output, a single sample
    (31, 33, 15),     # one below Din = 32 (the last Din at which every wave's segment is one group); D past two tiles
    (32, 64, 16),     # every wave exactly one group of 4; D on the four-tile edge; B on the sample tile
    (33, 72, 17),     # segments grow to 8: waves 5..7 idle; D past 64: two workgroup rows; B past the sample tile
    (512, 32, 31),    # segment 64 = exactly one staged trip; B one below the backward's round of 32
    (516, 32, 32),    # segment 68: a second trip holding one group (vector staging); B on the round
    (513, 20, 33),    # the same edge through the scalar staging; B past the round
    (50, 32, 127),    # B one below the backward's loop trip of 128 samples
    (50, 32, 128),    # on it
    (50, 32, 129),    # past it: a second trip with one sample
    (784, 32, 512),   # the experiment's own shape (config 5)
]


def dense_block(rng, Din, D, bias=0.2):
    """[vec(W) (D x Din, column-major); b]: glorot-uniform weights and SMALL NONZERO biases (a zero bias hides a misplaced row)"""
    w = ((rng.random(D * Din) - 0.5) * np.sqrt(24.0 / (Din + D))).astype(f32)
    b = ((rng.random(D) - 0.5) * bias).astype(f32)
    return np.concatenate([w, b])


def dense_case(Din, D, B, seed=43):
    rng = np.random.default_rng([seed, Din, D, B])
    return dict(x=rng.standard_normal((B, Din)).astype(f32), pd=dense_block(rng, Din, D), du0=rng.standard_normal((B, D)).astype(f32))


def dense_apply(x, pd, D):
    """u0 = x W^T + b with W[o][k] at pd[o + D*k] and the bias at pd[D*Din + o] (torch tensors of one dtype)"""
    Din = x.shape[1]
    return x @ pd[:D * Din].reshape(Din, D) + pd[D * Din:]


def dense_reference(x, pd, D, du0, dtype):
    """dict(u0, dpd, dx): the layer and the pullback of <du0, u0>"""
    xt = torch.tensor(np.asarray(x, f32), dtype=dtype, requires_grad=True)
    pt = torch.tensor(np.asarray(pd, f32), dtype=dtype, requires_grad=True)
    u0 = dense_apply(xt, pt, D)
    (u0 * torch.tensor(np.asarray(du0, f32), dtype=dtype)).sum().backward()
    return dict(u0=u0.detach().numpy(), dpd=pt.grad.numpy(), dx=xt.grad.numpy())


_REF = {}


def dense_ref(Din, D, B):
    """the case and its two torch runs, computed once: dict(x, pd, du0, r64, r32)"""
    key = ("dense", Din, D, B)
    if key not in _REF:
        c = dense_case(Din, D, B)
        c["r64"] = dense_reference(c["x"], c["pd"], D, c["du0"], torch.float64)
        c["r32"] = dense_reference(c["x"], c["pd"], D, c["du0"], torch.float32)
        _REF[key] = c
    return _REF[key]


def check(name, got, r64, r32, keys):
    """every array of `got` within the rule; prints the measured error beside the bound; returns {key: (error, bound)}"""
    out = {}
    for k in keys:
        e, b = rel(got[k], r64[k]), bound(r32[k], r64[k])
        print(f"{name} {k}: got {e:.2e} torch-f32 {rel(r32[k], r64[k]):.2e} bound {b:.2e}")
        out[k] = (e, b)
    bad = {k: v for k, v in out.items() if not v[0] <= v[1]}
    assert not bad, (name, bad)
    return out


# ---- the whole model ----
def model_case(Din, D, H, K, B, nfine, seed=7, kind="EulerHeun", scale=1.5):
    """the pinned inputs of a model case: x (B, Din), the four parameter blocks, the layer's path(s) and local draws, labels"""
    lay = S.case_inputs(D, H, B, nfine, seed, scale=scale, second_path=kind == "SRI")
    rng = np.random.default_rng([seed, Din, D, K, B])
    return dict(x=rng.standard_normal((B, Din)).astype(f32), pds=dense_block(rng, Din, D), pd=lay["pd"], pg=lay["pg"],
                pc=dense_block(rng, D, K), labels=make_labels(rng, K, B), W=lay["W"], z=lay["z"], Z=lay["Z"], z2=lay["z2"])


def dense_np32(x, pds, D):
    """the downsample in float32 numpy (a stand-in for the device's u0 where no device is there)"""
    Din = x.shape[1]
    return (x @ pds[:D * Din].reshape(Din, D) + pds[D * Din:]).astype(f32)


def model_reference(c, ref, D, H, K, w_reg, tol, dtype, kind="EulerHeun", tableau=None, delta=1.0 / 6.0, want_dx=False):
    """the model over the recorded grid ref["steps"] (a result of oracle.sde_node_forward / sde_adaptive_np.sde_node_forward)
    by torch autograd in `dtype`: dict(u0, u_end, logits, ce, reg_val, loss, d_downsample, d_drift, d_diffusion, d_classifier[, dx])"""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    leaf = lambda a: torch.tensor(np.asarray(a, f32), dtype=dtype, requires_grad=True)
    pds, pd, pg, pc = leaf(c["pds"]), leaf(c["pd"]), leaf(c["pg"]), leaf(c["pc"])
    x = leaf(c["x"]) if want_dx else t(c["x"])
    f, g = _fields64(pd, pg, D, H)
    nfine = c["W"].shape[0] - 1
    hh = 1.0 / nfine
    Wt = t(c["W"])
    Zt = t(c["Z"]) if kind == "SRI" else None

    def step(u, dW, dZ, dt):
        """(u', EEst * dt) of the layer's step kind"""
        if kind == "EulerHeun":
            return _eh_step64(f, g, u, dW, dt)[0], None
        if kind == "RKMil":
            un = _mil_step64(f, g, u, dW, dt)
            r = (un - u) / (tol + torch.maximum(u.abs(), un.abs()) * tol)
            return un, torch.sqrt((r * r).mean()) * dt
        return _sri_step64(f, g, tableau, u, dW, dZ, dt, tol, tol, delta)

    u0 = dense_apply(x, pds, D)
    states, u = [], u0
    for (i, m) in ref["steps"]:
        u = step(u, Wt[i + m] - Wt[i], None if Zt is None else Zt[i + m] - Zt[i], m * hh)[0]
        states.append(u)
    _, k, th = ref["series"][-1]                       # sol.u[end]
    a = u0 if k <= 0 else states[k - 1]
    u_end = u0 if k < 0 else (1.0 - float(th)) * a + float(th) * states[k]
    lg = dense_apply(u_end, pc, K)
    lab = torch.as_tensor(np.asarray(c["labels"]), dtype=torch.long)
    ce = (torch.logsumexp(lg, dim=1) - lg[torch.arange(lg.shape[0]), lab]).mean()
    reg = torch.zeros((), dtype=dtype)
    if ref["u1"] is not None:                          # the local step: its start state is a constant of the tape
        u1, dWl, dtl = t(ref["u1"]), t(ref["dW_local"]), float(ref["dt_local"])
        if kind == "EulerHeun":
            reg = _eh_reg64(f, g, u1, dWl, dtl, tol, tol, delta)
        else:
            reg = step(u1, dWl, None if ref.get("dZ_local") is None else t(ref["dZ_local"]), dtl)[1]
    loss = ce + w_reg * reg
    loss.backward()
    z = lambda p: (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    out = dict(u0=u0.detach().numpy(), u_end=u_end.detach().numpy(), logits=lg.detach().numpy(), ce=float(ce.detach()),
               reg_val=float(reg.detach()), loss=float(loss.detach()), d_downsample=z(pds), d_drift=z(pd), d_diffusion=z(pg),
               d_classifier=z(pc))
    if want_dx:
        out["dx"] = z(x)
    return out


def clustered_batch(i, B, Din, K):
    """batch i of the synthetic clustered data of tests/test_gpu_training_loop.py: a sample = its class centre + noise, in [0, 1]"""
    centers = np.random.default_rng(0).random((K, Din), dtype=f32)
    g = np.random.default_rng(1000 + i)
    lab = g.integers(0, K, B).astype(np.int32)
    x = (centers[lab] + 0.15 * g.standard_normal((B, Din)).astype(f32)).clip(0, 1).astype(f32)
    return x, lab
