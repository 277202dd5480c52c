"""Helper, not a test: the shared inputs of the SDE tests with a TIME-DEPENDENT drift (tests/test_host_sde_timedep.py pins
them on the CPU, tests/test_gpu_sde_timedep.py runs the library on them).  Imports the oracle's Python side only, never the
package under test.

The reference applies both closures to ArrayAndTime(u, t) (src/layers/neural_sde.jl:55-66), so a TDChain drift sees the time
every step passes it.  Drift: TDChain(Dense(D+1 => H, tanh), Dense(H+1 => D)) in the flat layout of
oracle.glorot_mlp_params(..., time_dep=True) — the time column LAST in both layers (the unpacking of
tests/test_oracle_backward.py::_field64, reused; the field around it is restated so the dtype follows the input).  Diffusion: Dense(D => D) with bias,
built as tests/test_gpu_parity.py::_sde_fields builds it; it does not see the time.

The float64 steps below take `t` and evaluate the drift at the reference's times, cited line by line to
src/perform_step.jl; `times=` replaces those times, so a test can build a wrong-time variant from the reference alone."""
import numpy as np
import torch

from test_oracle_backward import _unpack      # (W1, b1, W2, b2) of the flat layout, the time column last in both layers

f32 = np.float32

# (D, H, B) of the step-level tests
STEP_CASES = [
    (2, 4, 3),
    (20, 48, 5),      # D not a multiple of 4
    (32, 64, 16),     # inside the one-launch kernels' shape gate: time_dep alone keeps the handle off them
    (32, 64, 40),     # partial last 16-column tile
    (72, 32, 6),      # outside the gate
]
CONTRACT_CASES = STEP_CASES[:3]     # the SRI step's backward contract
T_STEP, DT_STEP, TOL, DELTA = 0.4, 0.25, 0.14, 1.0 / 6.0
C_NAMES = ("c02", "c03", "c04", "c11", "c12", "c13", "c14")
TAB_SEED = 45      # the step-level SRI tableau: the seed whose seven c's move every step case by more than 4e-3 (seed 41: 7e-4)


def step_id(c):
    return "%dx%dx%d" % tuple(c)


def params(D, H, seed):
    """(pd, pg): glorot weights plus 0.05 N(0,1) everywhere, so the time rows and the biases are non-zero"""
    import oracle as O
    rng = np.random.default_rng(seed + 1)
    pd = O.glorot_mlp_params(D, H, time_dep=True, seed=seed)
    pd = (pd + rng.standard_normal(pd.size).astype(f32) * f32(0.05)).astype(f32)
    Wg = ((rng.random((D, D), dtype=f32) - f32(0.5)) * f32(0.6)).astype(f32)     # (in, out) = column-major out x in
    bg = (rng.standard_normal(D) * 0.05).astype(f32)
    return pd, np.concatenate([Wg.ravel(), bg]).astype(f32)


def oracle_fields(O, D, H, pd, pg):
    """the C oracle's closures: time-dependent drift; Dense(D => D) held as an identity Dense followed by the Dense"""
    p2 = np.concatenate([np.eye(D, dtype=f32).ravel(), np.zeros(D, f32), pg])
    return (O.MlpField(D, H, pd, time_dep=True, act="tanh", nthreads=4),
            O.MlpField(D, D, p2, time_dep=False, act="identity", nthreads=4))


def fields64(pd, pg, D, H):
    """f(u, t), g(u) on (B, D) torch tensors (float64 in the tests; the dtype is the parameters')"""
    def f(u, t):
        W1, b1, W2, b2 = _unpack(pd, D, H, 1)
        tc = torch.full((u.shape[0], 1), float(t), dtype=u.dtype)
        h = torch.tanh(torch.cat([u, tc], 1) @ W1.T + b1)
        return torch.cat([h, tc], 1) @ W2.T + b2

    def g(u):
        return u @ pg[:D * D].reshape(D, D) + pg[D * D:]       # flat = (in, out) row-major: u Wg' + bg
    return f, g


def _residual_reg(num, u, un, dt, abstol, reltol):
    r = num / (abstol + torch.maximum(u.abs(), un.abs()) * reltol)
    return torch.sqrt((r * r).mean()) * dt


def eh_times(t, dt):
    """the drift's times in src/perform_step.jl:174 (du1), :191 (f(tmp)), :193 (du2)"""
    return (t, t + dt, t + dt)


def eh_step64(f, g, u, dW, t, dt, abstol=TOL, reltol=TOL, delta=DELTA, times=None):
    """src/perform_step.jl:172-206 -> (u', EEst * dt)"""
    ta, tb, tc = eh_times(t, dt) if times is None else times
    du1 = f(u, ta); L = g(u)                                   # :174, :176
    K = u + dt * du1                                           # :175
    tmp = K + L * dW                                           # :179, :183
    un = u + (dt / 2) * (du1 + f(tmp, tb)) + 0.5 * (L + g(tmp)) * dW      # :184, :186, :191
    Ed = dt * (f(K, tc) - du1) / 2                             # :193-194
    sq = np.sqrt(dt)
    En = ((g(u + L * sq) - L) / sq) * dW * dW / 2              # :196-198
    return un, _residual_reg(delta * Ed + En, u, un, dt, abstol, reltol)   # :200-205


def mil_times(t, dt):
    """the drift's one live time, src/perform_step.jl:127 (du2 of :163 is dead: :166 overwrites what it feeds)"""
    return (t,)


def mil_step64(f, g, u, dW, t, dt, abstol=TOL, reltol=TOL, times=None):
    """src/perform_step.jl:108-170, diagonal noise, Ito -> (u', EEst * dt) with the four-argument residual (:166-169)"""
    (ta,) = mil_times(t, dt) if times is None else times
    du1 = f(u, ta); L = g(u)                                   # :127-128
    K = u + dt * du1                                           # :130
    sq = np.sqrt(dt)
    Dgj = (g(K + sq * L) - L) / sq                             # :133-136
    J = dW * dW / 2 - dt / 2                                   # :116, :121
    un = K + L * dW + Dgj * J                                  # :138
    return un, _residual_reg(un - u, u, un, dt, abstol, reltol)


def sri_times(T, t, dt):
    """the drift's times in src/perform_step.jl:62, :68, :74, :84"""
    return (t, t + T["c02"] * dt, t + T["c03"] * dt, t + T["c04"] * dt)


def sri_times_swapped(T, t, dt):
    """c0j <-> c1j: the drift at the DIFFUSION's times (:63, :69, :75, :85)"""
    return (t + T["c11"] * dt, t + T["c12"] * dt, t + T["c13"] * dt, t + T["c14"] * dt)


def sri_step64(f, g, T, u, dW, dZ, t, dt, abstol=TOL, reltol=TOL, delta=DELTA, times=None, scale_up_side=True):
    """src/perform_step.jl:49-106 -> (u', EEst * dt).  scale_up_side=False drops d scale / d uprev on the |uprev| >= |u'| side
    from autograd (the value is unchanged): the fault the step's backward had"""
    t1, t2, t3, t4 = sri_times(T, t, dt) if times is None else times
    sq = np.sqrt(dt)
    chi1 = (dW ** 2 - abs(dt)) / (2 * sq)                      # :58
    chi2 = (dW + dZ / np.sqrt(3.0)) / 2                        # :59
    chi3 = (dW ** 3 - 3 * dW * dt) / (6 * dt)                  # :60
    k1 = f(u, t1); g1 = g(u)                                   # :62-63
    H01 = u + dt * T["a021"] * k1 + T["b021"] * chi2 * g1      # :65
    H11 = u + dt * T["a121"] * k1 + sq * T["b121"] * g1        # :66
    k2 = f(H01, t2); g2 = g(H11)                               # :68-69
    H02 = u + dt * (T["a031"] * k1 + T["a032"] * k2) + chi2 * (T["b031"] * g1 + T["b032"] * g2)     # :71
    H12 = u + dt * (T["a131"] * k1 + T["a132"] * k2) + sq * (T["b131"] * g1 + T["b132"] * g2)       # :72
    k3 = f(H02, t3); g3 = g(H12)                               # :74-75
    H03 = u + dt * (T["a041"] * k1 + T["a042"] * k2 + T["a043"] * k3) + chi2 * (T["b041"] * g1 + T["b042"] * g2 + T["b043"] * g3)   # :77-79
    H13 = u + dt * (T["a141"] * k1 + T["a142"] * k2 + T["a143"] * k3) + sq * (T["b141"] * g1 + T["b142"] * g2 + T["b143"] * g3)     # :80-82
    k4 = f(H03, t4); g4 = g(H13)                               # :84-85
    E2 = chi2 * (T["beta31"] * g1 + T["beta32"] * g2 + T["beta33"] * g3 + T["beta34"] * g4) + \
        chi3 * (T["beta41"] * g1 + T["beta42"] * g2 + T["beta43"] * g3 + T["beta44"] * g4)          # :87-88
    un = u + dt * (T["alpha1"] * k1 + T["alpha2"] * k2 + T["alpha3"] * k3 + T["alpha4"] * k4) + E2 + \
        dW * (T["beta11"] * g1 + T["beta12"] * g2 + T["beta13"] * g3 + T["beta14"] * g4) + \
        chi1 * (T["beta21"] * g1 + T["beta22"] * g2 + T["beta23"] * g3 + T["beta24"] * g4)          # :90-94
    E1 = dt * (k1 + k2 + k3 + k4)                              # :98
    ua = u.abs() if scale_up_side else torch.where(u.abs() >= un.abs(), u.abs().detach(), u.abs())
    r = (delta * E1 + E2) / (abstol + torch.maximum(ua, un.abs()) * reltol)                         # :100-103
    return un, torch.sqrt((r * r).mean()) * dt                 # :105


def sri_tableau(seed, scale=1.0):
    """a fixed-seed tableau (the project does not restate SOSRI's): float32 uniform(-0.6, 0.9) draws as the gradient tests use;
    every coefficient but the seven c's times `scale`.  Redrawn until the c's are pairwise more than 0.05 apart and none lies
    within 0.05 of 0: every stage time is then a different one, and none is t."""
    import oracle as O
    rng = np.random.default_rng(seed)
    while True:
        T = {k: float(f32(rng.uniform(-0.6, 0.9))) for k in O.SRI_FIELDS}
        c = sorted(T[k] for k in C_NAMES)
        if min(abs(v) for v in c) > 0.05 and min(b - a for a, b in zip(c, c[1:])) > 0.05:
            break
    return {k: (v if k in C_NAMES else float(f32(v * scale))) for k, v in T.items()}


def step_inputs(D, H, B, seed=0):
    """dict(pd, pg, x, dW, dZ, du): one step from T_STEP of length DT_STEP"""
    pd, pg = params(D, H, seed)
    rng = np.random.default_rng(seed + 50)
    x = rng.standard_normal((B, D)).astype(f32)
    dW = (rng.standard_normal((B, D)) * np.sqrt(DT_STEP)).astype(f32)
    dZ = (rng.standard_normal((B, D)) * np.sqrt(DT_STEP)).astype(f32)
    du = rng.standard_normal((B, D)).astype(f32)
    return dict(pd=pd, pg=pg, x=x, dW=dW, dZ=dZ, du=du)


def grid_inputs(D, H, B, n, seed=0, span=0.5):
    """a fixed grid of n steps: dict(pd, pg, x, dW (n,B,D), dZ, du, dt, t0 = 0.2)"""
    pd, pg = params(D, H, seed)
    rng = np.random.default_rng(seed + 60)
    dt = f32(span / n)
    x = rng.standard_normal((B, D)).astype(f32)
    dW = (rng.standard_normal((n, B, D)) * np.sqrt(dt)).astype(f32)
    dZ = (rng.standard_normal((n, B, D)) * np.sqrt(dt)).astype(f32)
    du = rng.standard_normal((B, D)).astype(f32)
    return dict(pd=pd, pg=pg, x=x, dW=dW, dZ=dZ, du=du, dt=dt, t0=0.2)


def leaves(inp, dtype=torch.float64):
    return tuple(torch.tensor(inp[k], dtype=dtype, requires_grad=True) for k in ("pd", "pg", "x"))


def tt(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype)


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---- the adaptive layer -------------------------------------------------------------------------------------------------
# kind, (D, H, B, nfine), seed, tol, dt0, tableau (seed, scale), tspan.  The span does not start at 0 and h = 1/32 or 1/64 is a
# power of two, so every grid time t0 + i h is exact in float32.  Each case starts from a too long first step dt0 (no case of
# these sizes rejects on its own: tests/test_host_sde_adaptive.py), so the reference loop rejects and a step FOLLOWS a rejection.
T0, T2 = 0.25, 1.25
ADAPTIVE_CASES = [
    dict(kind="EulerHeun", shape=(32, 64, 16, 32), seed=7, tol=0.1, dt0=0.5),    # inside the one-launch kernels' gate
    dict(kind="RKMil", shape=(32, 64, 40, 64), seed=8, tol=0.56, dt0=1.0),        # inside the gate, partial last tile
    dict(kind="SRI", shape=(20, 48, 7, 32), seed=8, tol=0.14, dt0=0.4, tab=(45, 0.1)),
]
MODES = ("unbiased", "biased", "none")
T1 = 0.68      # :unbiased: t1 inside (T0, T2)
SAVEAT = (0.55, 1.02, 1.25)


def adaptive_id(c):
    return "%s-%dx%dx%d-n%d" % ((c["kind"],) + c["shape"])


def adaptive_inputs(c, scale=2.0):
    """parameters (drift scaled: a rougher field), x, the path W and the local draw z; for SRI the second path Z and draw z2"""
    import sde_adaptive_np as S
    D, H, B, nfine = c["shape"]
    pd, pg = params(D, H, c["seed"])
    pd = (pd * f32(scale)).astype(f32)
    rng = np.random.default_rng(c["seed"] + 100)
    x = rng.standard_normal((B, D)).astype(f32)
    W = S.brownian_path(rng, nfine, B, D, span=T2 - T0)
    z = rng.standard_normal((B, D)).astype(f32)
    out = dict(pd=pd, pg=pg, x=x, W=W, z=z, Z=None, z2=None)
    if c["kind"] == "SRI":
        out["Z"] = S.brownian_path(rng, nfine, B, D, span=T2 - T0)
        out["z2"] = rng.standard_normal((B, D)).astype(f32)
    return out


_REF = {}


def adaptive_reference(O, c, mode, saveat=(), t1_or_rand=T1, dt0=None):
    """(inputs, tableau, the result of tests/sde_adaptive_np.py's loop over the oracle's steps); computed once per key"""
    import sde_adaptive_np as S
    key = (adaptive_id(c), mode, tuple(saveat), float(t1_or_rand), dt0)
    if key not in _REF:
        D, H, B, nfine = c["shape"]
        inp = adaptive_inputs(c)
        drift, diff = oracle_fields(O, D, H, inp["pd"], inp["pg"])
        T = sri_tableau(*c["tab"]) if c["kind"] == "SRI" else None
        r = S.sde_node_forward(O, c["kind"], drift, diff, inp["x"], inp["W"], T0, T2, c["tol"], c["tol"], mode=mode, t1_or_rand=t1_or_rand,
                               z_local=inp["z"], saveat=saveat, dt0=c["dt0"] if dt0 is None else dt0, tableau=T, Z=inp["Z"], z2_local=inp["z2"])
        _REF[key] = (inp, T, r)
    return _REF[key]


def step64(c, f, g, T, u, dW, dZ, t, dt):
    """the case's step in the restatement's dtype -> (u', EEst * dt)"""
    tol = c["tol"]
    if c["kind"] == "EulerHeun":
        return eh_step64(f, g, u, dW, t, dt, tol, tol, DELTA)
    if c["kind"] == "RKMil":
        return mil_step64(f, g, u, dW, t, dt, tol, tol)
    return sri_step64(f, g, T, u, dW, dZ, t, dt, tol, tol, DELTA)


def adaptive_autograd64(c, inp, T, ref, du_series, w_reg, all_at_t0=False, dtype=torch.float64):
    """loss = sum_j <du_j, sol.u[j]> + w_reg * reg_val over the RECORDED grid ref['steps'] by torch autograd: (dx, dp_drift,
    dp_diff).  Recorded step (i, m) starts at t0 + i h, the local step at t1; all_at_t0 puts every one of them at t0 instead
    (the wrong-time variant, from the reference alone)."""
    D, H, B, nfine = c["shape"]
    pdt, pgt, xt = leaves(inp, dtype)
    f, g = fields64(pdt, pgt, D, H)
    hh = (T2 - T0) / nfine
    Wt = tt(inp["W"], dtype)
    Zt = tt(inp["Z"], dtype) if c["kind"] == "SRI" else None
    states, u = [], xt
    for (i, m) in ref["steps"]:
        t = T0 if all_at_t0 else T0 + i * hh
        u = step64(c, f, g, T, u, Wt[i + m] - Wt[i], None if Zt is None else Zt[i + m] - Zt[i], t, m * hh)[0]
        states.append(u)
    loss = 0.0
    for j, (ts, k, th) in enumerate(ref["series"]):
        if k < 0:
            val = xt
        else:
            a = xt if k == 0 else states[k - 1]
            val = (1.0 - float(th)) * a + float(th) * states[k]
        loss = loss + (val * tt(du_series[j], dtype)).sum()
    if ref["u1"] is not None and w_reg != 0.0:
        t1 = T0 if all_at_t0 else float(ref["t1"])
        loss = loss + w_reg * step64(c, f, g, T, tt(ref["u1"], dtype), tt(ref["dW_local"], dtype),
                                     None if ref["dZ_local"] is None else tt(ref["dZ_local"], dtype), t1, float(ref["dt_local"]))[1]
    loss.backward()
    return xt.grad.numpy(), pdt.grad.numpy(), pgt.grad.numpy()
