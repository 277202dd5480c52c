"""Cases and torch references of the two classifier heads, shared by tests/test_host_heads.py, tests/test_gpu_heads.py and
tests/test_oracle_cifar.py.  Nothing here imports the package.

  MLP-handle head: Dense(D => K) + logitcrossentropy (csrc/lrnde_cls_fused.hpp; experiments/src/construct.jl:199, utils.jl:88)
  CIFAR head:      Conv(8 => 1, 3x3, pad 1, gelu) + flatten + Dense(H*W => K) + logitcrossentropy (lrnde_cifar_head_ce)

A case is compared with the float64 run of its reference under the suite's rule (latent_cases.bound): max(1e-5, 4 x the
distance of the float32 torch run from the float64 run), relative to the float64 value's norm, per array."""
import numpy as np
import torch

from latent_cases import bound, rel  # noqa: F401  (the suite's rule, re-exported)

# (D, K, B, scale of the weights): why the shape is here.  256 threads = 4 waves = 4 samples per workgroup, 64 lanes over D
# eight elements per trip (stride 512); the K x (D+1) block is staged in LDS while it has at most 61440 bytes, 8192 words
# per staging trip; K = 10 is a compile-time form of its own.
MLP_CASES = [
    (5, 10, 1, 1.0),      # D < 64 lanes; one wave of the workgroup live
    (64, 10, 3, 1.0),     # D on the lane count; partial workgroup
    (65, 10, 5, 1.0),     # one element in the second lane trip; two workgroups, the second with one wave
    (513, 10, 9, 1.0),    # second k0 trip (stride 512) holding a single element
    (1535, 10, 5, 1.0),   # K*(D+1)*4 == 61440: the last shape that stages in LDS
    (1536, 10, 5, 1.0),   # first shape past the limit: read from memory
    (40, 1, 5, 1.0),      # K = 1: loss, du, dpc exactly 0
    (40, 2, 7, 1.0),      # runtime K in LDS, smallest softmax
    (100, 7, 133, 1.0),   # runtime K; five 32-sample blocks in the parameter-gradient tiles, the last with 5 samples
    (600, 16, 5, 1.0),    # runtime K at the array bound; 9616 staged words: second staging trip
    (959, 16, 5, 1.0),    # 61440 bytes exactly at K = 16
    (960, 16, 9, 1.0),    # read from memory at K = 16
    (784, 10, 9, 40.0),   # |logit| ~ 190: saturated softmax, the exp clamp at -87
    (100, 7, 6, 40.0),    # the same at a runtime K
]

# (W, H, B, K, scale of the dense weights); k_cls_bwd_w sums the batch 16 samples, then 4, then 1 at a time
CIFAR_CASES = [
    (8, 8, 1, 10, 1.0),    # B = 1
    (8, 8, 5, 3, 1.0),     # small K, partial workgroup
    (12, 8, 6, 16, 1.0),   # K = 16, D = 96 (half the lanes take a second element), non-square
    (16, 16, 17, 7, 1.0),  # the 16-sample loop + 1 tail
    (8, 8, 23, 10, 1.0),   # all three loops (16 + 4 + 3)
    (8, 8, 5, 10, 40.0),   # dense weights x 40
]


def make_labels(rng, K, B):
    """int32 labels with the first and the last class present at the ends of the batch"""
    lab = rng.integers(0, K, B).astype(np.int32)
    lab[0] = 0
    if B > 1:
        lab[-1] = K - 1
    return lab


def dense_block(rng, D, K, scale):
    """[vec(W) (K x D, column-major); b]: glorot-uniform weights x scale (logits of size ~1 at scale 1 for inputs of size
    ~1) and SMALL NONZERO biases (a zero bias would hide a misplaced bias row)"""
    w = ((rng.random(K * D) - 0.5) * np.sqrt(24.0 / (D + K)) * scale).astype(np.float32)
    b = ((rng.random(K) - 0.5) * 0.2).astype(np.float32)
    return np.concatenate([w, b])


def mlp_case(D, K, B, scale=1.0, seed=31):
    """dict(u (B, D), pc (K*(D+1)), labels (B)), float32 / int32"""
    rng = np.random.default_rng([seed, D, K, B])
    u = rng.standard_normal((B, D)).astype(np.float32)
    return dict(u=u, pc=dense_block(rng, D, K, scale), labels=make_labels(rng, K, B))


def cifar_case(W, H, B, K, scale=1.0, seed=37):
    """dict(u (B, 8, H, W), ph (73 + K*H*W + K), labels (B)); `scale` multiplies the dense weights"""
    rng = np.random.default_rng([seed, W, H, B, K])
    u = rng.standard_normal((B, 8, H, W)).astype(np.float32)
    conv = np.concatenate([(rng.standard_normal(72) * 0.2).astype(np.float32), np.array([0.05], np.float32)])
    return dict(u=u, ph=np.concatenate([conv, dense_block(rng, H * W, K, scale)]), labels=make_labels(rng, K, B))


def _dense_ce(v, pd, K, labels):
    """logits = W v + b with the weight of class c, input k at pd[c + K*k] and the bias at pd[K*D + c]; the loss is the mean
    over the batch of logsumexp(logits) - logits[label]"""
    B, D = v.shape
    Wd = pd[:K * D].reshape(D, K)                  # [k][c]
    lg = v @ Wd + pd[K * D:]
    lab = torch.as_tensor(np.asarray(labels), dtype=torch.long)
    return lg, (torch.logsumexp(lg, dim=1) - lg[torch.arange(B), lab]).mean()


def classifier_reference(u, pc, K, labels, dtype):
    ut = torch.tensor(np.asarray(u, np.float32), dtype=dtype, requires_grad=True)
    pt = torch.tensor(np.asarray(pc, np.float32), dtype=dtype, requires_grad=True)
    lg, ce = _dense_ce(ut, pt, K, labels)
    ce.backward()
    return dict(loss=float(ce.detach()), logits=lg.detach().numpy(), du=ut.grad.numpy(), dpc=pt.grad.numpy())


def gelu_tanh(z):
    """the tanh form (geluf_c of csrc/lrnde_math.hpp)"""
    return 0.5 * z * (1.0 + torch.tanh(np.sqrt(2.0 / np.pi) * (z + 0.044715 * z ** 3)))


def cifar_head_reference(u, ph, K, labels, dtype):
    """72 conv weights at kx + 3*(ky + 3*ci), 1 conv bias, then the dense block (lrnde_cifar_head_param_count)"""
    ut = torch.tensor(np.asarray(u, np.float32), dtype=dtype, requires_grad=True)
    pt = torch.tensor(np.asarray(ph, np.float32), dtype=dtype, requires_grad=True)
    B, _, H, W = ut.shape
    w = torch.flip(pt[:72].reshape(1, 8, 3, 3), dims=(2, 3))      # (kx,ky,ci,co) column-major -> (co,ci,ky,kx), NNlib.conv flips
    v = gelu_tanh(torch.nn.functional.conv2d(ut, w, bias=pt[72:73], padding=1)).reshape(B, H * W)  # Julia flatten of (W,H,1,B): w fastest
    lg, ce = _dense_ce(v, pt[73:], K, labels)
    ce.backward()
    return dict(loss=float(ce.detach()), logits=lg.detach().numpy(), du=ut.grad.numpy(), dph=pt.grad.numpy())


def loss_bound(l32, l64):
    """the rule for the scalar: max(1e-5, 4 x |f32 - f64| / |f64|) of |f64| (absolute where the float64 loss is 0)"""
    return max(1e-5, 4.0 * rel_loss(l32, l64))


def rel_loss(a, l64):
    return abs(float(a) - l64) / abs(l64) if l64 != 0 else abs(float(a))


_REF = {}


def mlp_ref(D, K, B, scale=1.0):
    """the case and its two torch runs, computed once: dict(u, pc, labels, r64, r32)"""
    key = ("mlp", D, K, B, scale)
    if key not in _REF:
        c = mlp_case(D, K, B, scale)
        c["r64"] = classifier_reference(c["u"], c["pc"], K, c["labels"], torch.float64)
        c["r32"] = classifier_reference(c["u"], c["pc"], K, c["labels"], torch.float32)
        _REF[key] = c
    return _REF[key]


def cifar_ref(W, H, B, K, scale=1.0):
    key = ("cifar", W, H, B, K, scale)
    if key not in _REF:
        c = cifar_case(W, H, B, K, scale)
        c["r64"] = cifar_head_reference(c["u"], c["ph"], K, c["labels"], torch.float64)
        c["r32"] = cifar_head_reference(c["u"], c["ph"], K, c["labels"], torch.float32)
        _REF[key] = c
    return _REF[key]


def check(name, got, c, keys, split=None):
    """every array of `got` (numpy) within the rule of the case's float64 reference; prints the measured error beside the
    bound.  split: {key: index} compares key[:index] and key[index:] separately.  Returns {label: (error, bound)}."""
    out = {}
    r64, r32 = c["r64"], c["r32"]
    e, b = rel_loss(got["loss"], r64["loss"]), loss_bound(r32["loss"], r64["loss"])
    print(f"{name} loss: got {e:.2e} torch-f32 {rel_loss(r32['loss'], r64['loss']):.2e} bound {b:.2e}")
    out["loss"] = (e, b)
    for k in keys:
        parts = [(k, slice(None))] if not split or k not in split else [(f"{k}[:{split[k]}]", slice(0, split[k])),
                                                                         (f"{k}[{split[k]}:]", slice(split[k], None))]
        for label, sl in parts:
            g, a64, a32 = (np.asarray(a).reshape(-1)[sl] if k in (split or {}) else np.asarray(a) for a in (got[k], r64[k], r32[k]))
            e, b = rel(g, a64), bound(a32, a64)
            print(f"{name} {label}: got {e:.2e} torch-f32 {rel(a32, a64):.2e} bound {b:.2e}")
            out[label] = (e, b)
    bad = {k: v for k, v in out.items() if not v[0] <= v[1]}
    assert not bad, (name, bad)
    return out
