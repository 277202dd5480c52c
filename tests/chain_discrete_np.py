"""Yardsticks of the Dense-chain handle's discrete adjoint (NeuralODE(field="dense_chain", sensealg="TrackerAdjoint");
csrc/lrnde_chain_discrete.hpp).  TEST INFRASTRUCTURE, CPU only, written from the method's statement (the
frozen step grid, FSAL differentiated, saves inside a step by the Tsit5 interpolant), not from the kernel.

  (a) frozen_forward / frozen_grads: the forward map on a FROZEN grid [(t_n, dt_n)] as torch code over torch_field — the
      Tsit5 stages with FSAL (k1 of step n+1 is k7 of step n), the interpolant for a save inside a step, a copy for a save
      at a step's end or at the start — and its gradient by autograd.  dtype float64 is the yardstick; its float32 twin
      (the same graph in torch.float32) sizes rounding: a GPU gradient is held to max(1e-5, 4 x |twin - float64|).
  (b) sweep64: the reverse sweep of DESIGN 4.9.3 restated in numpy float64 over the analytic products of
      chain_adjoint_np.Field.vjp.  Field.vjp rounds its time to float32 and its results once to float32 (the convention of
      the continuous restatement); held to 1e-10 against (a) the sweep needs them unrounded, so Field64.vjp64 repeats those
      products without the two roundings (tests/test_host_chain_discrete.py checks it against Field.vjp).

The times t_n, dt_n and every theta = (ts - t_n) / dt_n are float32 values, as the forward's footer forms them."""
import numpy as np
import torch

import chain_adjoint_np as CA
import np_restatement as R
from test_gpu_chain import ACT64, mk_inputs, shapes, torch_field

f32 = np.float32
CS = [R.C[0], R.C[1], R.C[2], R.C[3], 1.0, 1.0]


def grid_of(steps):
    """[(t_n, dt_n)] of chain_adjoint_np.forward(...)['steps']"""
    return [(f32(s[0]), f32(s[1])) for s in steps]


def grid_of_trace(trace):
    """[(t_n, dt_n)]: the accepted rows of Handle.solve(..., trace=True)['trace']"""
    return [(f32(r["t"]), f32(r["dt"])) for r in trace if r["accepted"]]


def place(grid, t0, t2, times):
    """where the forward's footer takes each saved time from: ("start",) for ts <= t0; ("end", n) for ts == t_{n+1};
    ("in", n, theta) for t_n < ts < t_{n+1}, theta = (ts - t_n) / dt_n in float32.  t_{n+1} is the next step's start, t2
    for the last step."""
    N = len(grid)
    ends = [grid[n + 1][0] if n + 1 < N else f32(t2) for n in range(N)]
    out = []
    for ts in times:
        ts = f32(ts)
        if ts <= f32(t0):
            out.append(("start",))
            continue
        n = next(i for i in range(N) if ts <= ends[i])
        assert ts > grid[n][0]
        out.append(("end", n) if ts == ends[n] else ("in", n, f32(f32(ts - grid[n][0]) / grid[n][1])))
    return out


def bweights(theta):
    """b_1..b_7(theta) of the Tsit5 interpolant in float64 from the float32 theta"""
    th = float(f32(theta))
    b = [th * (R._R[0][0] + th * (R._R[0][1] + th * (R._R[0][2] + th * R._R[0][3])))]
    return b + [th * th * (r[0] + th * (r[1] + th * r[2])) for r in R._R[1:]]


# ---- (a) the frozen-grid forward in torch -------------------------------------------------------------------------
def frozen_forward(f, x, grid, t0, t2, times):
    """the saved states (in the order of `times`) of the frozen-grid Tsit5 solve of du/dt = f(u, t) from x"""
    pl = place(grid, t0, t2, times)
    out = [None] * len(times)
    u, k1 = x, f(x, float(grid[0][0]))
    for i, e in enumerate(pl):
        if e[0] == "start":
            out[i] = x
    for n, (t, dt) in enumerate(grid):
        t, dt = float(t), float(dt)
        ks = [k1]
        for s in range(2, 8):
            xs = u + dt * sum(a * k for a, k in zip(R.A[s], ks))
            ks.append(f(xs, t + CS[s - 2] * dt))
        unew = xs
        for i, e in enumerate(pl):
            if e[0] == "end" and e[1] == n:
                out[i] = unew
            elif e[0] == "in" and e[1] == n:
                out[i] = u + dt * sum(b * k for b, k in zip(bweights(e[2]), ks))
        u, k1 = unew, ks[6]
    return out


def frozen_grads(model, p, x, grid, t0, t2, times, cots, dtype=torch.float64):
    """(dx, dp, saved states) of loss = sum_i <cots[i], state_i> on the frozen grid, by autograd"""
    pt = torch.tensor(np.asarray(p), dtype=dtype, requires_grad=True)
    xt = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    states = frozen_forward(torch_field(model, pt), xt, grid, t0, t2, times)
    loss = sum((s * torch.tensor(np.asarray(c), dtype=dtype)).sum() for s, c in zip(states, cots))
    loss.backward()
    return xt.grad.numpy().astype(np.float64), pt.grad.numpy().astype(np.float64), [s.detach().numpy() for s in states]


# ---- (b) the reverse sweep in numpy float64 -----------------------------------------------------------------------
class Field64(CA.Field):
    """chain_adjoint_np.Field in float64 with nothing rounded: f64(y, t), and vjp64 = Field.vjp's analytic products
    without its rounding of t and of the results to float32"""

    def __init__(self, model, p):
        super().__init__(model, p, np.float64)

    def f64(self, y, t):
        return self.f.f64(y, float(t))

    def vjp64(self, y, t, lam):
        td, ia, ls = self.sp
        y, g, t = np.asarray(y, np.float64), np.asarray(lam, np.float64), float(t)
        h = ACT64[ia](y)
        d0 = CA._dact(ia, y, h)
        hs, ds = [], []
        for (W, b), (i, _o, a) in zip(self.Wb, ls):
            hs.append(h)
            z = h @ W[:, :i].T + b
            if td:
                z = z + t * W[:, i]
            h = ACT64[a](z)
            ds.append(CA._dact(a, z, h))
        parts = []
        for l in range(len(ls) - 1, -1, -1):
            W, _b = self.Wb[l]
            i = ls[l][0]
            delta = g * ds[l]
            gb = delta.sum(axis=0)
            cols = [delta.T @ hs[l]] + ([(gb * t)[:, None]] if td else [])
            parts.append(np.concatenate([np.concatenate(cols, axis=1).T.reshape(-1), gb]))
            g = delta @ W[:, :i]
        return g * d0, np.concatenate(parts[::-1])


def sweep64(model, p, x, grid, t0, t2, times, cots):
    """(dx, dp) by the reverse sweep: lam is the cotangent of the state at the current time, kap that of the next
    step's k1; per step the interior saves (descending), stage 7, stages 6..2; after step 0 the Jacobian of k1_0"""
    fld = Field64(model, p)
    pl = place(grid, t0, t2, times)
    cots = [np.asarray(c, np.float64) for c in cots]
    N = len(grid)
    # the forward along the grid, keeping (uprev, k1..k6, the stage inputs) of every step
    rec = []
    u, k1 = np.asarray(x, np.float64), fld.f64(x, grid[0][0])
    for t, dt in grid:
        t, dt = float(t), float(dt)
        ks, xs = [k1], {}
        for s in range(2, 8):
            xs[s] = u + dt * sum(a * k for a, k in zip(R.A[s], ks))
            ks.append(fld.f64(xs[s], t + CS[s - 2] * dt))
        rec.append((u, ks, xs))
        u, k1 = xs[7], ks[6]
    lam = np.zeros_like(u)
    for e, c in zip(pl, cots):
        if e == ("end", N - 1):
            lam = lam + c
    kap = np.zeros_like(u)
    mu = np.zeros(fld.P)
    for n in range(N - 1, -1, -1):
        t, dt = float(grid[n][0]), float(grid[n][1])
        _u, _ks, xs = rec[n]
        ck = [None] + [np.zeros_like(lam) for _ in range(6)] + [kap]   # ck[1..7]
        cu = np.zeros_like(lam)
        inner = sorted(((float(times[i]), i) for i, e in enumerate(pl) if e[0] == "in" and e[1] == n), reverse=True)
        for _ts, i in inner:
            cu = cu + cots[i]
            for j, b in enumerate(bweights(pl[i][2])):
                ck[j + 1] = ck[j + 1] + (dt * b) * cots[i]
        w, gp = fld.vjp64(xs[7], t + dt, ck[7])
        mu = mu + gp
        lam = lam + w
        cu = cu + lam
        for j in range(1, 7):
            ck[j] = ck[j] + (dt * R.A[7][j - 1]) * lam
        for s in range(6, 1, -1):
            w, gp = fld.vjp64(xs[s], t + CS[s - 2] * dt, ck[s])
            mu = mu + gp
            cu = cu + w
            for j in range(1, s):
                ck[j] = ck[j] + (dt * R.A[s][j - 1]) * w
        lam = cu
        if n > 0:
            for e, c in zip(pl, cots):
                if e == ("end", n - 1):
                    lam = lam + c
        kap = ck[1]
    w, gp = fld.vjp64(x, grid[0][0], kap)
    lam, mu = lam + w, mu + gp
    for e, c in zip(pl, cots):
        if e[0] == "start":
            lam = lam + c
    return lam, mu


# ---- inputs -------------------------------------------------------------------------------------------------------
# A forward that rejects steps (rejected attempts do not appear in the sweep).  Selection conditions, found
# and asserted on the CPU alone (tests/test_host_chain_discrete.py): (1) chain_adjoint_np.forward rejects at least two
# attempts with the float64 field and with the float32 field; (2) the yardstick still says something there: on that grid
# 4 x the distance of the float32 twin from float64 is within REJECTS_BAR for dx and dp.  Fields that reject are close to
# losing their gradient to rounding: of the 40 rejecting inputs found (PhysioNet, 16 x Dense(24, 24) and TDChain gelu at
# weights x2 .. x6, tol 1e-2 .. 1e-5, four seeds) the twins are 1e-3 .. 1e+4 apart on most — PhysioNet x3 at tol 1e-3 is
# 1e-2 apart on the CPU's grid and 1.15 apart on the MI355X's, which holds a gradient to nothing.
# PhysioNet at weights x2.5, B = 9, tol 1e-4: 23 accepted and 4 rejected attempts with either field, twins 3.1e-5 (dx) and
# 1.7e-5 (dp) apart.
REJECTS = dict(shape="physionet", B=9, scale=2.5, tol=1e-4, times=[0.5, 1.0])
REJECTS_BAR = 1e-3


def rejects_inputs(P):
    c = REJECTS
    model = shapes(P)[c["shape"]]
    p, x = mk_inputs(P, model, c["B"], scale=c["scale"])
    cots = np.random.default_rng(23).standard_normal((len(c["times"]),) + x.shape).astype(f32)
    return model, p, x, list(c["times"]), cots, c["tol"]


def bound(v32, v64, floor=1e-5, margin=4.0):
    """the bar a float32 implementation's gradient block is held to against the float64 yardstick: `floor`, or `margin`
    x the distance of the float32 twin (relative, 2-norm)"""
    v32, v64 = np.asarray(v32, np.float64), np.asarray(v64, np.float64)
    return max(floor, margin * float(np.linalg.norm(v32 - v64) / np.linalg.norm(v64)))
