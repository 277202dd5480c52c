"""Strip geometries of the conv vector field (csrc/lrnde_conv.hip) that tests/test_host_conv_geometry.py and
tests/test_gpu_conv_geometry.py hold to the oracle: the table, the restated geometry, the case builder, a
dtype-generic torch-CPU restatement of the field (float64 = the yardstick of the oracle, float32 = the measure of what a
different summation order costs) and the failure locator.  Nothing here needs a GPU.

Every image is cut into strips of TR rows (csrc/lrnde_conv_geom.hpp): TR is the largest divisor of H with
TR*W <= 128, a strip has TP = TR*W pixels in MT = ceil(TP/16) M tiles of 16, and every conv kernel is instantiated per
MT in 1..8.  A strip is ragged when TP % 16 != 0: the last tile's lanes beyond the strip read pixel 0 and must not store."""
import functools

import numpy as np
import torch

C, HC = 8, 64                      # state / hidden channels of the CIFAR block
MAXPX = 128                        # 16 * MAXMT pixels per strip
N1 = 9 * (C + 1) * HC              # flat layout: w1 | bn1 scale, bias | w2 | bn2 scale, bias | w3
N2 = N1 + 2 * HC
N3 = N2 + 9 * (HC + 1) * HC
N4 = N3 + 2 * HC
BLOCKS = (("w1", slice(0, N1)), ("bn1", slice(N1, N2)), ("w2", slice(N2, N3)), ("bn2", slice(N3, N4)),
          ("w3", slice(N4, None)))


def geometry(W, H):
    """(TR, TP, MT, strips) of a W x H image: strip_rows of lrnde_conv.hip restated"""
    TR = 1
    for tr in range(1, H + 1):
        if H % tr == 0 and tr * W <= MAXPX:
            TR = tr
    TP = TR * W
    return TR, TP, (TP + 15) // 16, H // TR


def legal(W, H):
    """what lrnde_conv_create accepts"""
    return W % 4 == 0 and 4 <= W <= MAXPX and H >= 2


def wgrad_lds_bytes(W, H):
    """dynamic LDS of the three weight-gradient launches of a VJP, in launch order: conv3 (8 cotangent channels, 64
    inputs), conv2 (64 x 64), conv1 (64 cotangent channels, 8 inputs).  G tile [TP][GS] + IN halo tile [(TR+2)(W+2)][IS],
    stride 80 floats for a 64-channel operand and 16 for an 8-channel one."""
    TR, TP, _MT, _s = geometry(W, H)
    npos = (TR + 2) * (W + 2)
    return {"w3": 4 * (TP * 16 + npos * 80), "w2": 4 * (TP * 80 + npos * 80), "w1": 4 * (TP * 80 + npos * 16)}


WGRAD_LDS_LIMIT = 160 * 1024       # a launch above it is refused (LRNDE_UNSUPPORTED, "weight-gradient")


def wgrad_max_workgroups(lds_bytes):
    """grid of a persistent weight-gradient launch = min(strips, this): two workgroups per CU where the tiles fit twice"""
    return 512 if lds_bytes <= 80 * 1024 else 256


# (W, H, B train, B test, TR, TP, MT, strips, what it is there for)
GEOMETRIES = (
    (4, 2, 8, 1, 2, 8, 1, 1, "smallest legal image; half-filled single tile"),
    (8, 2, 4, 1, 2, 16, 1, 1, "MT=1, full tile"),
    (4, 37, 1, 1, 1, 4, 1, 37, "TR=1 with interior strips; 4 of 16 lanes live; 18 halo positions for 256 threads"),
    (8, 3, 3, 2, 3, 24, 2, 1, "MT=2 ragged, odd H"),
    (32, 7, 2, 2, 1, 32, 2, 7, "TR=1 interior, MT=2 full"),
    (20, 7, 3, 2, 1, 20, 2, 7, "TR=1 interior, ragged, 16 % W != 0"),
    (12, 3, 2, 2, 3, 36, 3, 1, "MT=3 ragged"),
    (16, 3, 2, 2, 3, 48, 3, 1, "MT=3 full; one idle wave in k_conv_out"),
    (52, 3, 2, 2, 1, 52, 4, 3, "MT=4 ragged (the tested 8x8 fills its four tiles), TR=1 interior"),
    (16, 5, 2, 2, 5, 80, 5, 1, "MT=5 full; first use of the second accumulator"),
    (68, 3, 2, 2, 1, 68, 5, 3, "MT=5 ragged, W in (64,128), TR=1 interior"),
    (28, 3, 2, 2, 3, 84, 6, 1, "MT=6 ragged"),
    (12, 9, 2, 2, 9, 108, 7, 1, "MT=7 ragged, TR = H = 9"),
    (36, 3, 1, 1, 3, 108, 7, 1, "MT=7 ragged, W > 32"),
    (40, 3, 2, 1, 3, 120, 8, 1, "MT=8 ragged"),
    (124, 3, 2, 2, 1, 124, 8, 3, "widest width whose VJP is supported (160 640 B of LDS)"),
)

# tanh and identity: one ragged row and one TR == 1 row each (gelu runs on every row)
EXTRA_ACT_ROWS = ((12, 3), (20, 7))
EXTRA_ACTS = ("tanh", "identity")

# multi-strip weight gradient and statistics, train mode, gelu: (W, H, B, the weight-gradient launches that must loop)
MULTI_STRIP = (
    (4, 2, 520, ("w3", "w2", "w1")),   # 520 strips > 512: all three loop; k_bn_finalize_t reduces 520 partials
    (68, 3, 87, ("w2",)),              # 261 strips; the 64 x 64 tiles need 88 960 B > 80 KiB -> 256 workgroups
)


def row_batch(row, train):
    return row[2] if train else row[3]


def seed_of(W, H, B, train, act="gelu"):
    """one seed per case, chosen freely (the host test holds the oracle to float64 at every one of them)"""
    return 1000 + 7 * W + 131 * H + 17 * B + (3 if train else 0) + {"gelu": 0, "tanh": 1, "identity": 2}[act]


def all_cases():
    """(W, H, B, act, train) of every small case: the table in both BatchNorm modes + the extra activations"""
    out = []
    for row in GEOMETRIES:
        for train in (True, False):
            out.append((row[0], row[1], row_batch(row, train), "gelu", train))
    by_wh = {(r[0], r[1]): r for r in GEOMETRIES}
    for wh in EXTRA_ACT_ROWS:
        for act in EXTRA_ACTS:
            for train in (True, False):
                out.append((wh[0], wh[1], row_batch(by_wh[wh], train), act, train))
    return out


def make_case(W, H, B, seed, act="gelu", train=True, scale=1.0):
    """(params, u (B, C, H, W), bn_state or None): Glorot weights, non-trivial BatchNorm scale / bias, and in test mode a
    running-statistics state — _case of tests/test_gpu_conv.py without the handles"""
    import oracle as O
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


def cotangent(shape, seed=17):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def oracle_field(W, H, p, act, train, st, bf16=False):
    import oracle as O
    return O.ConvField(W, H, C, HC, p, act=act, bn_train=train, bn_state=st, nthreads=8, bf16=bf16)


@functools.lru_cache(maxsize=None)
def reference(W, H, B, act, train, ts=(0.0, 0.613), t_vjp=0.41):
    """the oracle's answers for one case, computed once and shared (read-only): dict with p, u, st, lam,
    rhs[t] (B, C, H, W), dy, gp"""
    import oracle as O
    p, u, st = make_case(W, H, B, seed_of(W, H, B, train, act), act=act, train=train)
    fld = oracle_field(W, H, p, act, train, st)
    out = dict(p=p, u=u, st=st, rhs={t: fld.rhs(u.reshape(B, -1), t).reshape(u.shape) for t in ts})
    lam = cotangent(u.shape)
    dy, gp = O.conv_vjp(fld, u.reshape(B, -1), t_vjp, lam.reshape(B, -1))
    out.update(lam=lam, dy=dy.reshape(u.shape), gp=gp)
    for v in list(out.values()) + list(out["rhs"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference_bf16(W, H, B, act, train, ts=(0.0, 0.613)):
    """{t: the oracle's bf16 emulation of the f-eval} at the case of reference()"""
    ref = reference(W, H, B, act, train)
    fb = oracle_field(W, H, ref["p"], act, train, ref["st"], bf16=True)
    return {t: fb.rhs(ref["u"].reshape(B, -1), t).reshape(ref["u"].shape) for t in ts}


def torch_field(u, p, t, W, H, act, train, st=None, eps=1e-5):
    """the conv field on torch tensors of one dtype (float64 or float32), differentiable in u and p: conv2d with the kernel
    flipped (= NNlib.conv), the t plane as the last channel of every conv, train / test-mode BatchNorm, tanh-form gelu —
    torch_conv_field of tests/test_oracle_conv.py made differentiable (the host test holds the two to each other)"""
    B = u.shape[0]
    dt = u.dtype
    x = u.reshape(B, C, H, W)
    off = [0]

    def take(n):
        v = p[off[0]:off[0] + n]; off[0] += n
        return v

    def weight(cin, cout):
        return torch.flip(take(9 * cin * cout).reshape(cout, cin, 3, 3), dims=(2, 3))

    def tcat(z):
        return torch.cat([z, torch.full((B, 1, H, W), float(t), dtype=dt)], dim=1)

    def fact(z):
        if act == "gelu":
            return 0.5 * z * (1.0 + torch.tanh(float(np.sqrt(2.0 / np.pi)) * (z + 0.044715 * z ** 3)))
        return torch.tanh(z) if act == "tanh" else z

    def bn(z, k):
        g, b = take(HC), take(HC)
        if train:
            mu = z.mean(dim=(0, 2, 3), keepdim=True)
            var = z.var(dim=(0, 2, 3), unbiased=False, keepdim=True)
        else:
            s = torch.tensor(np.asarray(st, dtype=np.float64)).to(dt)
            mu = s[2 * k * HC:(2 * k + 1) * HC].reshape(1, HC, 1, 1)
            var = s[(2 * k + 1) * HC:(2 * k + 2) * HC].reshape(1, HC, 1, 1)
        return fact((z - mu) / torch.sqrt(var + eps) * g.reshape(1, HC, 1, 1) + b.reshape(1, HC, 1, 1))

    z = bn(torch.nn.functional.conv2d(tcat(x), weight(C + 1, HC), padding=1), 0)
    z = bn(torch.nn.functional.conv2d(tcat(z), weight(HC + 1, HC), padding=1), 1)
    z = torch.nn.functional.conv2d(tcat(z), weight(HC + 1, C), padding=1)
    assert off[0] == p.numel()
    return z.reshape(B, -1)


def torch_vjp(u, p, t, lam, W, H, act, train, st=None, dtype=torch.float64):
    """(f, dy, gp) as float64 numpy arrays from torch-CPU autograd run in `dtype`"""
    ut = torch.tensor(np.asarray(u).reshape(u.shape[0], -1), dtype=dtype, requires_grad=True)
    pt = torch.tensor(np.asarray(p), dtype=dtype, requires_grad=True)
    f = torch_field(ut, pt, t, W, H, act, train, st)
    (f * torch.tensor(np.asarray(lam).reshape(u.shape[0], -1), dtype=dtype)).sum().backward()
    return (f.detach().double().numpy(), ut.grad.double().numpy(), pt.grad.double().numpy())


def block_errors(got, ref):
    """{block: max |got - ref| / max |ref|} over the five parameter blocks"""
    got = np.asarray(got, dtype=np.float64); ref = np.asarray(ref, dtype=np.float64)
    return {name: float(np.abs(got[sl] - ref[sl]).max() / max(np.abs(ref[sl]).max(), 1e-300)) for name, sl in BLOCKS}


@functools.lru_cache(maxsize=None)
def f32_distance(W, H, B, act, train, t_vjp=0.41):
    """per parameter block, the distance of a float32 torch-CPU autograd run from the float64 one at the case's input
    (both reference-side): what summing the same products in another order and precision costs at this size"""
    p, u, st = make_case(W, H, B, seed_of(W, H, B, train, act), act=act, train=train)
    lam = cotangent(u.shape)
    _f64, _dy64, gp64 = torch_vjp(u, p, t_vjp, lam, W, H, act, train, st, torch.float64)
    _f32, _dy32, gp32 = torch_vjp(u, p, t_vjp, lam, W, H, act, train, st, torch.float32)
    return block_errors(gp32, gp64)


def multi_strip_bars(W, H, B, act, train):
    """{block: max(5e-5, 4 x the float32-to-float64 distance)}: the small cases' bar, or four times what a different
    summation order costs the reference itself (the factor tests/test_gpu_latent.py gives one)"""
    d = f32_distance(W, H, B, act, train)
    return {k: max(5e-5, 4.0 * v) for k, v in d.items()}, d


def locate(err, W, H):
    """arg-max of an error array of a (B, C, H, W) state -> (sample, channel, y, x, strip = y // TR,
    tile = ((y % TR) * W + x) // 16): the M tile of the strip's instantiation a failure points at"""
    err = np.asarray(err).reshape(-1, C, H, W)
    n, c, y, x = (int(v) for v in np.unravel_index(int(np.argmax(err)), err.shape))
    TR = geometry(W, H)[0]
    return n, c, y, x, y // TR, ((y % TR) * W + x) // 16


def describe(err, W, H):
    n, c, y, x, strip, tile = locate(err, W, H)
    TR, TP, MT, strips = geometry(W, H)
    return (f"worst at sample {n} channel {c} y {y} x {x}: strip {strip} of {strips}, M tile {tile} of MT={MT} "
            f"(TR={TR}, TP={TP}{', ragged' if TP % 16 else ''})")
