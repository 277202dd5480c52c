"""Shared by tests/test_host_wide_chain.py and tests/test_gpu_wide_chain.py: the wide Dense-chain shapes, the input
generator, the float64 / float32-BLAS numpy fields, the float64 torch field and RK4 references, and the float32 host
restatements (tests/wide_chain_host.cpp, tests/wide_chain_vjp_host.cpp), and gemm_paths: which branch of wide_gemm every
product of a shape takes.  No code is shared with the kernels."""
import os
import subprocess
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ACT64 = {"identity": lambda z: z, "tanh": np.tanh,
         "gelu": lambda z: z / (1.0 + np.exp(-1.5957691216057308 * z * (1.0 + 0.044715 * z * z)))}
ACT_T = {"identity": lambda z: z, "tanh": torch.tanh,
         "gelu": lambda z: z * torch.sigmoid(1.5957691216057308 * z * (1.0 + 0.044715 * z * z))}
ACT_CODE = {"identity": 0, "tanh": 1, "gelu": 2}

BATCHES = (1, 16, 17, 33)   # tile tails of the 16-column tile; 512 only for the column-independence case


def td_chain(P, dims, acts):
    """TDChain of Dense(dims[l] + 1 => dims[l+1], acts[l])"""
    return P.TDChain(P.Chain(*[P.Dense(dims[l] + 1, dims[l + 1], acts[l]) for l in range(len(dims) - 1)]))


def chain(P, dims, acts, in_act=None):
    ls = [P.Dense(dims[l], dims[l + 1], acts[l]) for l in range(len(dims) - 1)]
    return P.Chain(*([P.Activation(in_act)] if in_act else []), *ls)


def shapes(P):
    return {
        "mnist2": td_chain(P, [784, 100, 784], ["tanh", "identity"]),                      # the bitwise yardsticks
        "mnist3": td_chain(P, [784, 100, 100, 784], ["tanh", "tanh", "identity"]),          # the experiment's shape
        "seg_edges": chain(P, [224, 113, 225, 224], ["tanh", "tanh", "identity"]),          # segment ends at 112 / 113 / 224 / 225
        "odd_td": td_chain(P, [130, 257, 131, 130], ["gelu", "gelu", "identity"]),          # no multiple of 4 or 16
        "deep16": chain(P, [144] * 17, ["tanh"] * 16, in_act="gelu"),                       # the layer limit
        "w1024": chain(P, [1024, 16, 1024], ["tanh", "identity"]),                          # the LDS budget
        "physionet": chain(P, [20, 40] * 4 + [20], ["tanh"] * 8, in_act="tanh"),            # bits shared with the small handle
        # wide_gemm's other branches (gemm_paths): 8 row-tile groups and 9 (a second trip of wave 0, its last group one real
        # tile) with 5 segments, forward and transposed
        "sq520": chain(P, [520, 500, 520], ["tanh", "identity"]),
        # 1024 -> 16 spreads its 10 segments inside the partial region, the transposed 100 -> 1024 wants 17920 floats of it
        # and keeps its segments in one wave: both in one handle, D at the LDS limit
        "cap_mixed": td_chain(P, [1024, 16, 100, 1024], ["tanh", "gelu", "identity"]),
        "cap_fwd": chain(P, [1024, 100, 1024], ["tanh", "identity"]),                       # the same fall-back, forward product
        "full1024": chain(P, [1024, 1024, 1024], ["tanh", "identity"]),                     # 16 groups x 10 segments; P = 2 099 200
    }


# ---- which branch of wide_gemm (csrc/lrnde_wide_chain.hpp) a product takes, from its three conditions ----
WT, NW, SEGK, NB = 4, 8, 7, 16           # row tiles per wave, waves, k-groups per segment, columns per tile
WIDE_LDS_MAX = 160 * 1024
LDS_TAIL = NW * 3 * 8 + 16 * 4 + 16      # wide_smem_bytes beside the buffers: the fp64 partials, Bcast (16 words), padding
GEMM_PATHS = ("single", "split", "unsplit_multi", "unsplit_multi_trips", "cap_fallback")


def ceil16(n):
    return (n + 15) // 16 * 16


def part_want(MT, KG):
    ngrp, nseg = -(-MT // WT), -(-KG // SEGK)
    return nseg * MT * 256 if (ngrp < NW and nseg > 1) else 0


def partcap(dims):
    """floats of the segment-partial region lrnde_create_wide_chain gives a chain of these widths"""
    want = 0
    for i, o in zip(dims[:-1], dims[1:]):
        MT, KG = ceil16(o) // 16, ceil16(i) // 16
        want = max(want, part_want(MT, KG), part_want(KG, MT))
    fixed = 2 * ceil16(max(dims)) * NB * 4 + LDS_TAIL
    return min(want, ((WIDE_LDS_MAX - fixed) // 4) & ~255)


def gemm_path(MT, KG, cap):
    ngrp, nseg = -(-MT // WT), -(-KG // SEGK)
    if nseg == 1:
        return "single"
    if ngrp < NW:
        return "split" if nseg * MT * 256 <= cap else "cap_fallback"
    return "unsplit_multi" if ngrp <= NW else "unsplit_multi_trips"


def gemm_paths(dims):
    """[(forward path, transposed path)] per layer: single (one segment), split (segments over the waves, partials in
    LDS), unsplit_multi (a wave adds its segments itself), unsplit_multi_trips (and takes more than one row-tile group),
    cap_fallback (would split, but its partials do not fit the region)"""
    cap = partcap(dims)
    out = []
    for i, o in zip(dims[:-1], dims[1:]):
        MT, KG = ceil16(o) // 16, ceil16(i) // 16
        out.append((gemm_path(MT, KG, cap), gemm_path(KG, MT, cap)))
    return out


def model_dims(model):
    ls = spec(model)[2]
    return [ls[0][0]] + [o for _i, o, _a in ls]


def vjp_chunk(dims, td, with_gp=True):
    """workgroups one VJP launch may run (lrnde_kernels.hip wide_vjp_chunk): its records and partial vectors within 256 MiB"""
    P = sum(o * (i + td) + o for i, o in zip(dims[:-1], dims[1:]))
    rec = sum((ceil16(i) + ceil16(o)) * NB for i, o in zip(dims[:-1], dims[1:])) + ceil16(dims[0]) * NB
    return (256 << 20) // ((rec + (P if with_gp else 0)) * 4)


def count_shapes(P):
    """the shapes whose float64 and float32 restatements take equal step counts at weights x3 / x6 (test_host_wide_chain)"""
    return {
        "mnist3": (shapes(P)["mnist3"], 16),
        "td200": (td_chain(P, [200, 160, 144, 200], ["tanh", "tanh", "identity"]), 48),
        "c136": (chain(P, [136, 260, 136], ["tanh", "identity"]), 24),
        # D % 4 != 0 (odd_td's widths): the scalar loads and stores of the step kernel and of its save footer
        "odd130": (td_chain(P, [130, 257, 131, 130], ["tanh", "tanh", "identity"]), 17),
    }


# (shape, scale, tol) solved on the GPU with the counts asserted: x3 / x6 only, the x6 case with a rejected step included
GPU_COUNT_CASES = [("mnist3", 3.0, 1e-4), ("mnist3", 6.0, 1e-5), ("td200", 6.0, 1e-4), ("c136", 3.0, 1e-5), ("c136", 6.0, 1e-4),
                   ("odd130", 6.0, 1e-4)]
# (shape, scale, tol) of the save-footer grid: save_start, two save times inside one accepted step, a third elsewhere, the
# end; and every accepted step saved.  odd130 x6 has a rejected step.
FOOTER_CASES = [("odd130", 6.0, 1e-4), ("mnist3", 3.0, 1e-4)]


def footer_saves(t_steps):
    """three save times from a solve's accepted steps [(tprev, t)]: 1/3 and 2/3 into the longest step that is neither the
    first nor the last (two saves of one step), and the middle of the step two before it — each a third of a step from
    the nearest step end, where a float32 run's step ends differ from these by parts in 1e4"""
    inner = t_steps[2:-1]
    j = 2 + int(np.argmax([float(b) - float(a) for a, b in inner]))
    (a, b), (c, d) = t_steps[j], t_steps[j - 2]
    a, b, c, d = float(a), float(b), float(c), float(d)
    return [float(np.float32(v)) for v in (0.5 * (c + d), a + (b - a) / 3.0, a + 2.0 * (b - a) / 3.0)]


def steps_holding(t_steps, times):
    """index of the accepted step (tprev, t] that holds each time"""
    return [next(i for i, (a, b) in enumerate(t_steps) if float(a) < float(np.float32(ts)) <= float(b)) for ts in times]


def spec(model):
    """(td, input activation, [(in, out, act)]) of a chain model"""
    from localregneuralde_jl_amd.layers import Activation, TDChain
    td = isinstance(model, TDChain)
    ia = model.layers[0].activation if isinstance(model.layers[0], Activation) else "identity"
    return td, ia, [(l.in_dims - int(td), l.out_dims, l.activation) for l in model.layers if not isinstance(l, Activation)]


def unflatten(p, sp):
    td, _, ls = sp
    out, o = [], 0
    for i, n, _a in ls:
        W = np.asarray(p[o:o + n * (i + td)], np.float64).reshape(i + td, n).T
        o += n * (i + td)
        out.append((W, np.asarray(p[o:o + n], np.float64)))
        o += n
    assert o == len(p)
    return out


class Chain64:
    """the field in float64, rounded once to float32 (np_restatement's field convention)"""

    def __init__(self, model, p):
        self.sp = spec(model)
        self.Wb = unflatten(p, self.sp)

    def f64(self, x, t):
        td, ia, ls = self.sp
        h = ACT64[ia](np.asarray(x, np.float64))
        for (W, b), (_i, _o, a) in zip(self.Wb, ls):
            z = h @ W[:, :W.shape[1] - td].T + b
            if td:
                z = z + float(t) * W[:, -1]
            h = ACT64[a](z)
        return h

    def __call__(self, x, t):
        return self.f64(x, t).astype(np.float32)


class Chain32(Chain64):
    """the same field in float32 arithmetic (numpy BLAS): a second summation order, to size rounding amplification"""

    def __call__(self, x, t):
        td, ia, ls = self.sp
        h = ACT64[ia](np.asarray(x, np.float32)).astype(np.float32)
        for (W, b), (_i, _o, a) in zip(self.Wb, ls):
            W32, b32 = W.astype(np.float32), b.astype(np.float32)
            z = h @ W32[:, :W32.shape[1] - td].T + b32
            if td:
                z = z + np.float32(t) * W32[:, -1]
            h = ACT64[a](z).astype(np.float32)
        return h


def torch_field(model, pt):
    td, ia, ls = spec(model)
    Wb, o = [], 0
    for i, n, _a in ls:
        W = pt[o:o + n * (i + td)].reshape(i + td, n).T
        o += n * (i + td)
        Wb.append((W, pt[o:o + n]))
        o += n

    def f(u, t):
        h = ACT_T[ia](u)
        for (W, b), (i, _n, a) in zip(Wb, ls):
            z = h @ W[:, :i].T + b
            if td:
                z = z + t * W[:, i]
            h = ACT_T[a](z)
        return h
    return f


def err(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def mk_inputs(P, model, B, scale=1.0, seed=0, noise=0.01):
    """(p, x): glorot x scale plus `noise` normal noise (so the biases are not zero), x uniform in [-1, 1]"""
    p = P.glorot_chain_params(model, seed=seed, scale=scale)
    p = (p + np.random.default_rng(seed + 1).standard_normal(p.size).astype(np.float32) * np.float32(noise)).astype(np.float32)
    x = (np.random.default_rng(seed + 2).random((B, spec(model)[2][0][0]), dtype=np.float32) - np.float32(0.5)) * np.float32(2)
    return p, x


def mk(P, model, B, scale=1.0, seed=0, noise=0.01):
    """(wide-chain handle with the parameters set, p, x)"""
    from localregneuralde_jl_amd.layers import Handle, _wide_chain_desc
    p, x = mk_inputs(P, model, B, scale, seed, noise)
    h = Handle(_wide_chain_desc(model))
    h.set_params(torch.from_numpy(p))
    return h, p, x


def rk4_states(f64, x, times, nsteps=400):
    u, out, h = np.asarray(x, np.float64), [], 1.0 / nsteps
    marks = {int(round(t * nsteps)) for t in times}
    for k in range(nsteps):
        t = k * h
        k1 = f64(u, t); k2 = f64(u + 0.5 * h * k1, t + 0.5 * h); k3 = f64(u + 0.5 * h * k2, t + 0.5 * h); k4 = f64(u + h * k3, t + h)
        u = u + (h / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)
        if k + 1 in marks:
            out.append(u.copy())
    return out


def reference_grads(model, p, x, times, cots, nsteps=200):
    """(dx, dp) of sum_i <cots[i], u(times[i])> by float64 autograd through RK4"""
    pt = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    f = torch_field(model, pt)
    h = 1.0 / nsteps
    u, loss = xt, 0.0
    marks = {int(round(t * nsteps)): i for i, t in enumerate(times)}
    for k in range(nsteps):
        t = k * h
        k1 = f(u, t); k2 = f(u + 0.5 * h * k1, t + 0.5 * h); k3 = f(u + 0.5 * h * k2, t + 0.5 * h); k4 = f(u + h * k3, t + h)
        u = u + (h / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)
        if k + 1 in marks:
            loss = loss + (u * torch.tensor(cots[marks[k + 1]], dtype=torch.float64)).sum()
    loss.backward()
    return xt.grad.numpy(), pt.grad.numpy()


_HOST_EXE = {}


def _compile(src, flags=("-O2",)):
    if "dir" not in _HOST_EXE:
        _HOST_EXE["dir"] = tempfile.mkdtemp(prefix="wide_chain_host_")
    exe = os.path.join(_HOST_EXE["dir"], src[:-4])
    subprocess.run(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "localregneuralde.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", src), "-o", exe], check=True)
    return exe


def host_exe():
    """tests/wide_chain_host.cpp compiled with -O2 -ffp-contract=off (as tests/latent_cases.py compiles its program)"""
    if "exe" not in _HOST_EXE:
        _HOST_EXE["exe"] = _compile("wide_chain_host.cpp")
    return _HOST_EXE["exe"]


def vjp_host_exe():
    """tests/wide_chain_vjp_host.cpp, -ffp-contract=off.  -O3 -march=native only vectorise its independent accumulators
    and turn fmaf calls into the instruction (both correctly rounded): no operation of any chain changes.  Where the
    compiler refuses the flags the plain -O2 build computes the same bits, slower."""
    if "vjp" not in _HOST_EXE:
        try:
            _HOST_EXE["vjp"] = _compile("wide_chain_vjp_host.cpp", ("-O3", "-march=native"))
        except subprocess.CalledProcessError:
            _HOST_EXE["vjp"] = _compile("wide_chain_vjp_host.cpp")
    return _HOST_EXE["vjp"]


def run_host(model, p, x, t):
    """f(x, t) by the float32 host restatement in the canonical order: (B, D) float32"""
    td, ia, ls = spec(model)
    dims = [ls[0][0]] + [o for _i, o, _a in ls]
    exe = host_exe()
    fin, fout = os.path.join(_HOST_EXE["dir"], "in.bin"), os.path.join(_HOST_EXE["dir"], "out.bin")
    x = np.ascontiguousarray(x, np.float32)
    with open(fin, "wb") as f:
        f.write(np.array([len(ls), int(td), ACT_CODE[ia], x.shape[0]] + dims + [ACT_CODE[a] for _i, _o, a in ls], np.int32).tobytes())
        f.write(np.float32(t).tobytes())
        f.write(np.ascontiguousarray(p, np.float32).tobytes())
        f.write(x.tobytes())
    subprocess.run([exe, fin, fout], check=True)
    return np.fromfile(fout, np.float32).reshape(x.shape)


def run_vjp_host(model, p, y, lam, t, chunk=0):
    """(dy (B, D), gp (P)) of the float32 host restatement of the VJP in the canonical order; chunk > 0: the parameter
    cotangent as launches of `chunk` workgroups summed it before the running sum was carried through them"""
    td, ia, ls = spec(model)
    dims = [ls[0][0]] + [o for _i, o, _a in ls]
    exe = vjp_host_exe()
    fin, fout = os.path.join(_HOST_EXE["dir"], "vjp_in.bin"), os.path.join(_HOST_EXE["dir"], "vjp_out.bin")
    y, lam = np.ascontiguousarray(y, np.float32), np.ascontiguousarray(lam, np.float32)
    assert y.shape == lam.shape
    with open(fin, "wb") as f:
        f.write(np.array([len(ls), int(td), ACT_CODE[ia], y.shape[0], chunk] + dims + [ACT_CODE[a] for _i, _o, a in ls], np.int32).tobytes())
        f.write(np.float32(t).tobytes())
        f.write(np.ascontiguousarray(p, np.float32).tobytes())
        f.write(y.tobytes())
        f.write(lam.tobytes())
    subprocess.run([exe, fin, fout], check=True)
    out = np.fromfile(fout, np.float32)
    return out[:y.size].reshape(y.shape), out[y.size:]


def autograd_vjp(model, p, x, lam, t, dtype=torch.float64):
    """(dy, gp) of <lam, f(x, t)> by torch autograd in `dtype` (float32: a second summation order of the same quantities)"""
    pt = torch.tensor(p, dtype=dtype, requires_grad=True)
    ut = torch.tensor(x, dtype=dtype, requires_grad=True)
    (torch_field(model, pt)(ut, t) * torch.tensor(lam, dtype=dtype)).sum().backward()
    return ut.grad.numpy(), pt.grad.numpy()


def vjp_bars(model, p, x, lam, t):
    """((dy64, gp64), (bar_dy, bar_gp), (second-order distances)): 1e-5 scale-relative, or 4 x the distance of float32
    torch autograd from float64 where width amplifies rounding"""
    d64 = autograd_vjp(model, p, x, lam, t)
    d32 = autograd_vjp(model, p, x, lam, t, torch.float32)
    e32 = (err(d32[0], d64[0]), err(d32[1], d64[1]))
    return d64, (max(1e-5, 4.0 * e32[0]), max(1e-5, 4.0 * e32[1])), e32
