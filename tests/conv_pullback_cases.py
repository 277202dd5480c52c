"""Float64 yardsticks for the conv field's layer pullback (lrnde_conv_node_backward, lrnde_conv_step_reg_grad) that
tests/test_host_conv_pullback.py and tests/test_gpu_conv_pullback.py hold the oracle and the HIP handle to.  Nothing here
needs a GPU and nothing here is the project's own C: the field is torch_field of tests/conv_geometry_cases.py in float64,
the layer's gradient is autograd through classical RK4 on [0, 1], the regulariser's is autograd through one Tsit5 step
restated from src/perform_step.jl of the reference with the tableau of oracle/np_restatement.py.

Distances are per quantity: dx and each of the five parameter blocks of dp, max |got - ref| over max |ref| of that
quantity.  A bar is max(5e-5, 4 x the fp32 oracle's own distance from float64) (bars): 5e-5 is the per-block bar of the conv
VJP, 4 the factor a different summation order is given (multi_strip_bars).  The host test caps every oracle distance at
2.5e-3, so no bar exceeds 1e-2."""
import collections
import functools

import numpy as np
import torch

import conv_geometry_cases as G
import np_restatement as NP

LayerCase = collections.namedtuple("LayerCase", "name W H B act train seed scale tol nsteps", defaults=(32,))   # nsteps: of the RK4 yardstick
StepPoint = collections.namedtuple("StepPoint", "name W H B act train seed")

T0, T2 = 0.0, 1.0
T1 = 0.41                          # the unbiased t1 of every case
T1_EDGE = (1.2e-4, 0.9995)         # 8x8 row only: a stop next to either end of the span (the tstop snap)
MAXITERS = 5000
QUANTITIES = ("dx",) + tuple(name for name, _sl in G.BLOCKS)
FLOOR, FACTOR, CAP = 5e-5, 4.0, 2.5e-3

LAYER_CASES = (
    LayerCase("8x8", 8, 8, 3, "gelu", True, 41, 1.5, 1e-4),            # the case of test_conv_node_backward_matches_oracle
    LayerCase("8x8-test", 8, 8, 3, "gelu", False, 41, 1.5, 1e-4),      # running statistics
    LayerCase("16x16-tanh", 16, 16, 2, "tanh", True, 42, 1.5, 1e-3),   # two strips per image
    LayerCase("12x3", 12, 3, 2, "gelu", True, 43, 2.0, 1e-5),          # MT=3 ragged
    LayerCase("4x2-test", 4, 2, 1, "gelu", False, 44, 1.5, 1e-4),      # n = 64 < 256 = the running statistics
    LayerCase("4x2-train", 4, 2, 3, "gelu", True, 45, 1.5, 1e-4),      # n = 192 < 256
    LayerCase("20x7-identity", 20, 7, 3, "identity", True, 46, 1.5, 1e-4),   # TR=1, seven ragged strips per image
    # the oracle's adjoint rejects a step (19 accepted, 1 rejected in `none`).  Found by a search over seed, scale and
    # tolerance: with batch statistics, or below scale 3, no adjoint of 700 tried rejected; it takes running statistics and
    # a trajectory that grows, and that one needs 64 RK4 steps to move by less than 1e-6 against twice as many.
    LayerCase("4x2-reject", 4, 2, 3, "tanh", False, 43, 3.0, 1e-5, 64),
)
CASE = {c.name: c for c in LAYER_CASES}
REJECT_CASE = "4x2-reject"

# (mode, t1_or_rand) of a layer case with the solution cotangent alone
def layer_modes(case):
    out = [("none", T1), ("unbiased", T1)]
    if case.name == "8x8":
        out += [("unbiased", t) for t in T1_EDGE]
    return out + [("biased", T1)]


REG_TYPES = ("error_estimate", "stiffness_estimate")
# the regulariser through the layer, isolated (zero cotangent, w_reg = 1).  The local step runs at the automatic initial
# dt, so the rows have their own scale and tolerance: at the tolerances above that dt is so small that the fp32 oracle's
# stiffness gradient is 5e-3 .. 1.8e-2 from float64 (above the cap); at scale 3, tol 1e-2 it is within 1e-3.
REG_LAYER_CASES = (
    LayerCase("8x8-reg", 8, 8, 3, "gelu", True, 41, 3.0, 1e-2),
    LayerCase("8x8-test-reg", 8, 8, 3, "gelu", False, 41, 3.0, 1e-2),
    LayerCase("16x16-tanh-reg", 16, 16, 2, "tanh", True, 41, 3.0, 1e-2),
    LayerCase("4x2-train-reg", 4, 2, 3, "gelu", True, 41, 3.0, 1e-2),
)
REG_LAYER_MODES = ("unbiased", "biased")
CASE.update({c.name: c for c in REG_LAYER_CASES})


def reg_layer_pinned(case, reg_type):
    """whether the layer's regulariser gradient can be held to float64 at a row: stiffness_estimate everywhere,
    error_estimate with running statistics only (docstring of tests/test_host_conv_pullback.py)"""
    return reg_type == "stiffness_estimate" or not case.train

# one Tsit5 step at t = 0.2, tol 1e-4: error_estimate where its gradient is well conditioned in fp32, stiffness_estimate
# at the point of test_conv_step_reg_grad_matches_oracle
STEP_T, STEP_TOL = 0.2, 1e-4
STEP_AT = {"error_estimate": (3.0, 0.5), "stiffness_estimate": (2.0, 0.25)}     # reg_type -> (scale, dt)
STEP_POINTS = (
    StepPoint("8x8", 8, 8, 3, "gelu", True, 31),
    StepPoint("8x8-test", 8, 8, 3, "gelu", False, 31),
    StepPoint("16x16-tanh", 16, 16, 2, "tanh", True, 32),
    StepPoint("12x3", 12, 3, 2, "gelu", True, 33),
    StepPoint("20x7-identity", 20, 7, 3, "identity", True, 34),
    StepPoint("4x2-train", 4, 2, 3, "gelu", True, 35),
)
POINT = {p.name: p for p in STEP_POINTS}

# running statistics around the layer call: (W, H, B, train), the last one the control with n >= 256
STATS_CASES = ((4, 2, 1, False), (4, 2, 3, True), (8, 2, 1, False), (8, 8, 3, True), (8, 8, 3, False))


def _ro(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(p, u (B, C, H, W), st or None, w) of a layer case, read-only; w = default_rng(3).standard_normal(u.shape)"""
    p, u, st = G.make_case(case.W, case.H, case.B, case.seed, act=case.act, train=case.train, scale=case.scale)
    w = np.random.default_rng(3).standard_normal(u.shape).astype(np.float32)
    return _ro(p, u, st, w)


@functools.lru_cache(maxsize=None)
def point_inputs(point, reg_type):
    """(p, u, st, k1, dt) of a regulariser-step point: k1 = the oracle's f(u, STEP_T) (a constant of the step)"""
    scale, dt = STEP_AT[reg_type]
    p, u, st = G.make_case(point.W, point.H, point.B, point.seed, act=point.act, train=point.train, scale=scale)
    k1 = G.oracle_field(point.W, point.H, p, point.act, point.train, st).rhs(u.reshape(point.B, -1), STEP_T).reshape(u.shape)
    return _ro(p, u, st, k1) + (dt,)


def _t64(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=grad)


@functools.lru_cache(maxsize=None)
def rk4_pullback64(case, nsteps=None):
    """(u_end, dx, dp) as read-only float64 arrays: classical RK4 with `nsteps` (default: the case's, 32) equal steps on
    [0, 1] over the float64 field, autograd of <w, u(1)>"""
    if nsteps is None:
        return rk4_pullback64(case, case.nsteps)
    p, u, st, w = case_inputs(case)
    B = case.B
    x = _t64(u.reshape(B, -1), grad=True)
    pt = _t64(p, grad=True)

    def f(y, t):
        return G.torch_field(y, pt, t, case.W, case.H, case.act, case.train, st)

    h = (T2 - T0) / nsteps
    y = x
    for i in range(nsteps):
        t = T0 + i * h
        k1 = f(y, t); k2 = f(y + 0.5 * h * k1, t + 0.5 * h); k3 = f(y + 0.5 * h * k2, t + 0.5 * h); k4 = f(y + h * k3, t + h)
        y = y + (h / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    (y * _t64(w.reshape(B, -1))).sum().backward()
    return _ro(y.detach().numpy().reshape(u.shape), x.grad.numpy().reshape(u.shape), pt.grad.numpy())


def step_reg64(p, u, k1, t, dt, abstol, reltol, W, H, act, train, st, reg_type):
    """(reg_val, d reg_val / d p) in float64 of one Tsit5 step from (u, t) with k1, dt and uprev = u constants:
    src/perform_step.jl:10-47 of the reference.  error_estimate = rms(utilde / (abstol + max(|uprev|, |u1|) reltol)) dt,
    stiffness_estimate = rms(k7 - k6) / (rms(u1 - g6) + eps(Float32)) / 3.5068"""
    B = np.asarray(u).shape[0]
    uprev = _t64(np.asarray(u).reshape(B, -1))
    pt = _t64(p, grad=True)
    dt = float(dt); t = float(t)
    cs = [NP.C[0], NP.C[1], NP.C[2], NP.C[3], 1.0, 1.0]
    ks = [_t64(np.asarray(k1).reshape(B, -1))]
    xs = {}
    for s in range(2, 8):
        acc = sum(a * k for a, k in zip(NP.A[s], ks))
        xs[s] = uprev + dt * acc
        ks.append(G.torch_field(xs[s], pt, t + cs[s - 2] * dt, W, H, act, train, st))
    g6, u1 = xs[6], xs[7]
    if reg_type == "error_estimate":
        utilde = dt * sum(b * k for b, k in zip(NP.BT, ks))
        resid = utilde / (abstol + torch.maximum(uprev.abs(), u1.abs()) * reltol)
        val = torch.sqrt((resid ** 2).mean()) * dt
    else:
        den = torch.sqrt(((u1 - g6) ** 2).mean())
        val = torch.sqrt(((ks[6] - ks[5]) ** 2).mean()) / (den + float(np.finfo(np.float32).eps)) / 3.5068
    val.backward()
    return float(val.detach()), pt.grad.numpy()


def distances(dx, dp, dx_ref, dp_ref):
    """{quantity: max |got - ref| / max |ref|}; dx None leaves it out"""
    out = {}
    if dx is not None:
        a = np.asarray(dx, dtype=np.float64).reshape(-1); b = np.asarray(dx_ref, dtype=np.float64).reshape(-1)
        out["dx"] = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))
    out.update(G.block_errors(np.asarray(dp).reshape(-1), dp_ref))
    return out


def _field(case, p, st):
    return G.oracle_field(case.W, case.H, p, case.act, case.train, st)


@functools.lru_cache(maxsize=None)
def oracle_layer(case, mode, t1=T1, reg_type=None):
    """the fp32 oracle's lro_conv_node_backward at a case: the solution cotangent with w_reg = 0 (reg_type None), or a
    zero cotangent with w_reg = 1"""
    import oracle as O
    p, u, st, w = case_inputs(case)
    B = case.B
    cot = w if reg_type is None else np.zeros_like(w)
    bo = O.node_backward(_field(case, p, st), u.reshape(B, -1), T0, T2, case.tol, case.tol, cot.reshape(B, -1), mode=mode,
                         reg_type=reg_type or "error_estimate", t1_or_rand=t1, w_reg=0.0 if reg_type is None else 1.0,
                         maxiters=MAXITERS)
    assert bo["retcode"] == 0
    _ro(bo["dx"], bo["dp"])
    return bo


@functools.lru_cache(maxsize=None)
def oracle_local_step(case, mode, t1=T1):
    """(t1_used, u(t1), k1, dt, reg_val by type) of the oracle's own local step: what its regulariser gradient is taken at"""
    import oracle as O
    p, u, st, _w = case_inputs(case)
    B = case.B
    fwd = O.node_forward(_field(case, p, st), u.reshape(B, -1), T0, T2, case.tol, case.tol, mode=mode, t1_or_rand=t1,
                         maxiters=MAXITERS)
    t1u = fwd["t1"]
    if mode == "unbiased":
        sol = O.solve(_field(case, p, st), u.reshape(B, -1), T0, T2, case.tol, case.tol, saveat=[t1u, T2], maxiters=MAXITERS)
        u1 = sol["u"][0]
    else:
        sol = O.solve(_field(case, p, st), u.reshape(B, -1), T0, T2, case.tol, case.tol, maxiters=MAXITERS)
        idx = [i for i, t in enumerate(sol["t"]) if t == t1u]
        assert len(idx) == 1, (t1u, sol["t"])
        u1 = sol["u"][idx[0]]
    dt, k1 = O.init_dt(_field(case, p, st), u1, t1u, T2, case.tol, case.tol)
    return float(t1u), np.array(u1).reshape(u.shape), np.array(k1).reshape(u.shape), float(dt), fwd


def reg_layer64(case, t1u, u1, k1, dt, reg_type):
    """step_reg64 at a local step of a layer case"""
    p, _u, st, _w = case_inputs(case)
    return step_reg64(p, u1, k1, t1u, dt, case.tol, case.tol, case.W, case.H, case.act, case.train, st, reg_type)


@functools.lru_cache(maxsize=None)
def oracle_distance(case, mode="none", reg_type=None, t1=T1):
    """{quantity: the fp32 oracle's distance from the float64 reference}.  A LayerCase with reg_type None: node_backward
    with the solution cotangent against rk4_pullback64; a LayerCase with a reg_type: the zero-cotangent, w_reg = 1 pullback
    against step_reg64 at the oracle's own local step (no dx: it is exactly zero); a StepPoint: step_reg_grad against
    step_reg64."""
    import oracle as O
    if isinstance(case, StepPoint):
        p, u, st, k1, dt = point_inputs(case, reg_type)
        g, _rv = O.step_reg_grad(_field(case, p, st), u.reshape(case.B, -1), k1.reshape(case.B, -1), STEP_T, dt, STEP_TOL, STEP_TOL,
                                 reg_type=reg_type)
        _v, g64 = step_reg64(p, u, k1, STEP_T, dt, STEP_TOL, STEP_TOL, case.W, case.H, case.act, case.train, st, reg_type)
        return distances(None, g, None, g64)
    bo = oracle_layer(case, mode, t1, reg_type)
    if reg_type is None:
        _ue, dx64, dp64 = rk4_pullback64(case)
        return distances(bo["dx"], bo["dp"], dx64, dp64)
    t1u, u1, k1, dt, _fwd = oracle_local_step(case, mode, t1)
    _v, g64 = reg_layer64(case, t1u, u1, k1, dt, reg_type)
    return distances(None, bo["dp"], None, g64)


def bars(case, mode="none", reg_type=None, t1=T1):
    """({quantity: max(5e-5, 4 x oracle_distance)}, the oracle distances)"""
    d = oracle_distance(case, mode, reg_type, t1)
    return {k: max(FLOOR, FACTOR * v) for k, v in d.items()}, d


def fmt(d, bar=None):
    return " ".join(f"{k} {v:.1e}" + (f"/{bar[k]:.1e}" if bar else "") for k, v in d.items())
