"""float64 restatement of a Dense-chain layer's pullback (NeuralODE(field="dense_chain")): the recorded forward solve,
the reversed-time Tsit5 solve on z = [lambda; mu] and the local regulariser's gradient.  TEST INFRASTRUCTURE, CPU only.

Written from DESIGN.md 4.4 / 4.9.1 and SURVEY.md 3.5 (solve loop, PI controller, ode_determine_initdt, the
InterpolatingAdjoint restatement), not from the kernels: the field and its vector-Jacobian products are analytic numpy
in float64 from float32 operands, rounded once to float32 (Chain64's convention); everything the solver does in Float32
broadcasts (stage sums, utilde, residuals, the controller) is float32 numpy, norms accumulate in float64
(np_restatement's conventions).  A second instance (dtype=np.float32) runs the field and the products in float32 numpy
BLAS (Chain32's convention): the distance between the two is the yardstick for how far apart two correct
implementations may land.

    pullback(model, p, x, times, cots, tol, mode=..., t1_or_rand=...) -> dict(dx, dp, counts, rows, reg_val, reg_grad, ...)

`rows` has the layout of Handle.adjoint_trace(): one (s, dt, EEst, accepted) per attempted step of the reversed solve."""
import numpy as np
import torch

import np_restatement as R
from test_gpu_chain import ACT64, Chain32, Chain64, mk_inputs, shapes, spec, torch_field, unflatten

f32 = np.float32
_GC, _GK = 1.5957691216057308, 0.044715


def _dact(a, z, h):
    """act'(z), h = act(z)"""
    if a == "identity":
        return np.ones_like(z)
    if a == "tanh":
        return 1.0 - h * h
    s = 1.0 / (1.0 + np.exp(-_GC * z * (1.0 + _GK * z * z)))   # gelu as z * sigmoid(g(z))
    return s + z * s * (1.0 - s) * (_GC * (1.0 + 3.0 * _GK * z * z))


class Field:
    """f(y, t) and its products J^T lam, (df/dp)^T lam (flat Lux order: per layer vec(W (out x (in+td))) column-major,
    then b), analytic.  dtype float64: float64 arithmetic on the float32 operands, results rounded once; float32: numpy
    float32 throughout."""

    def __init__(self, model, p, dtype=np.float64):
        self.sp = spec(model)
        self.T = dtype
        self.P = int(np.asarray(p).size)
        self.Wb = [(W.astype(dtype), b.astype(dtype)) for W, b in unflatten(p, self.sp)]
        self.f = Chain64(model, p) if dtype == np.float64 else Chain32(model, p)

    def __call__(self, y, t):
        return self.f(y, t)

    def vjp(self, y, t, lam):
        T = self.T
        td, ia, ls = self.sp
        y, g, t = np.asarray(y, T), np.asarray(lam, T), T(f32(t))
        h = ACT64[ia](y)
        d0 = _dact(ia, y, h)
        hs, ds = [], []
        for (W, b), (i, _o, a) in zip(self.Wb, ls):
            hs.append(h)
            z = h @ W[:, :i].T + b
            if td:
                z = z + t * W[:, i]
            h = ACT64[a](z)
            ds.append(_dact(a, z, h))
        parts = []
        for l in range(len(ls) - 1, -1, -1):
            W, _b = self.Wb[l]
            i = ls[l][0]
            delta = g * ds[l]
            gb = delta.sum(axis=0)
            cols = [delta.T @ hs[l]] + ([(gb * t)[:, None]] if td else [])
            gW = np.concatenate(cols, axis=1)             # (out, in + td)
            parts.append(np.concatenate([gW.T.reshape(-1), gb]))
            g = delta @ W[:, :i]
        return (g * d0).astype(f32), np.concatenate(parts[::-1]).astype(f32)


def _eps(x):
    return np.spacing(f32(abs(x)))


def _q(eest, qold):
    """PI controller's factor (SURVEY 3.5 loopfooter!): returns (q, q11)"""
    gamma, qmin, qmax = f32(0.9), f32(0.2), f32(10)
    if eest == 0:
        return f32(f32(1) / qmax), None
    q11 = R.fastpow(eest, f32(7.0 / 50.0))
    q = f32(q11 / R.fastpow(qold, f32(2.0 / 25.0)))
    return max(f32(f32(1) / qmax), min(f32(f32(1) / qmin), f32(q / gamma))), q11


def forward(f, x, t0, t2, abstol, reltol, saveat=(), save_start=False, maxiters=10000):
    """adaptive Tsit5 keeping every accepted step (t, dt, uprev, k1..k7); saveat points are filled by dense output, they
    are not tstops; a saveat entry at t0 is the start value (saved once, with save_start)"""
    t0, t2 = f32(t0), f32(t2)
    dt, k1 = R.init_dt(f, x, t0, t2, abstol, reltol)
    qoldinit = f32(1e-4)
    dtmax, dtmin = f32(t2 - t0), max(_eps(t2), _eps(t0))
    t, uprev, qold, q11, dtpropose = t0, x, qoldinit, f32(1), dt
    accept, it, naccept, nreject, nf = False, 0, 0, 0, 3
    u = k7 = None
    steps, ts, us = [], [], []
    if save_start:
        ts.append(t0); us.append(x)
    pend = [f32(s) for s in saveat if f32(s) > t0]
    while t < t2:
        if it > 0:
            if accept:
                uprev, k1, dt = u, k7, dtpropose
            else:
                dt = f32(dt / min(f32(5), f32(q11 / f32(0.9))))
        it += 1
        dt = max(min(dtmax, dt), dtmin)
        dt = min(f32(abs(dt)), f32(abs(t2 - t)))
        if it > maxiters or not dt > dtmin:
            raise RuntimeError("restatement forward did not finish")
        r = R.tsit5_step(f, uprev, k1, t, dt, abstol, reltol)
        u, k7, eest = r["u"], r["k7"], r["eest"]
        nf += 6
        q, q11n = _q(eest, qold)
        q11 = q11 if q11n is None else q11n
        accept = bool(eest <= 1)
        if not accept:
            nreject += 1
            continue
        naccept += 1
        qold = max(eest, qoldinit)
        ttmp, tprev = f32(t + dt), t
        t = t2 if abs(f32(ttmp - t2)) < f32(f32(100) * _eps(max(t, t2))) else ttmp
        steps.append((tprev, dt, uprev, r["ks"]))
        while pend and pend[0] <= t:
            s = pend.pop(0)
            ts.append(s)
            us.append(u if s == t else R.tsit5_interp(uprev, r["ks"], dt, f32(f32(s - tprev) / dt)))
        dtpropose = max(min(dtmax, f32(dt / q)), max(_eps(t), dtmin))
    return dict(u=u, steps=steps, ts=ts, us=us, naccept=naccept, nreject=nreject, nf=nf)


def interp64(uprev, ks, dt, theta):
    """the Tsit5 interpolant of SURVEY 3.5 in float64 from the float32 record, rounded once"""
    th = float(f32(theta))
    b = [th * (R._R[0][0] + th * (R._R[0][1] + th * (R._R[0][2] + th * R._R[0][3])))]
    b += [th * th * (r[0] + th * (r[1] + th * r[2])) for r in R._R[1:]]
    acc = sum(bi * k.astype(np.float64) for bi, k in zip(b, ks))
    return (uprev.astype(np.float64) + float(f32(dt)) * acc).astype(f32)


class Record:
    """y(t) of a forward's dense record: the step with the largest start time <= t, theta = (t - t_lo) / dt_lo.
    The float64 instance evaluates the interpolant in float64 and rounds once (its field convention), the float32
    instance with np_restatement.tsit5_interp.  This matters: the weights b_i(theta) reach 88 and cancel, so the float32
    form carries ~3e-7 |k| dt of rounding in y, and on attempts whose estimate is small (EEst < 1e-3: the first ones
    after initdt) that rounding IS the estimate (TDChain x3, tol 1e-4, attempt 0: EEst 1.1e-4 with the float64
    interpolant, 5.7e-4 with the float32 one, 3.1e-4 on the MI355X with the polynomial record of DESIGN 4.4)."""

    def __init__(self, steps, dtype=np.float64):
        self.steps = steps
        self.t = np.array([s[0] for s in steps], f32)
        self.interp = interp64 if dtype == np.float64 else R.tsit5_interp

    def __call__(self, t):
        t = f32(t)
        lo = max(int(np.searchsorted(self.t, t, side="right")) - 1, 0)
        t_lo, dt_lo, uprev, ks = self.steps[lo]
        return self.interp(uprev, ks, dt_lo, f32(f32(t - t_lo) / dt_lo))


def _norm(rl, rm, N):
    s = np.square(rl.astype(np.float64)).sum() + np.square(rm.astype(np.float64)).sum()
    return f32(np.sqrt(s / N))


def _lin(base, dt, coefs, Ks):
    acc = sum(f32(c) * k for c, k in zip(coefs, Ks))
    return (dt * acc).astype(f32) if base is None else (base + dt * acc).astype(f32)


def reverse(fld, rec, t0, t2, abstol, reltol, lam0, impulses, stops, maxiters=10000):
    """Tsit5 on z = [lam; mu] in s = -t from -t2 to -t0.  dlam/ds = J^T lam, dmu/ds = (df/dp)^T lam at y(-s) of the
    record.  `impulses`: [(s, du)] ascending with s0 < s; those inside the span are added to lam when an accepted step
    lands on them (K1 re-evaluated, nf += 1), those at s1 after the solve.  `stops`: tstops, ascending, inside the span.
    Returns lam, mu, (naccept, nreject, nf), rows."""
    abstol, reltol = f32(abstol), f32(reltol)
    s0, s1 = f32(-f32(t2)), f32(-f32(t0))
    lam, mu = lam0.astype(f32), np.zeros(fld.P, f32)
    N = lam.size + mu.size
    rhs = lambda l, s: fld.vjp(rec(f32(-f32(s))), f32(-f32(s)), l)
    dtmax, dtmin = f32(s1 - s0), max(_eps(s1), _eps(s0))
    # ode_determine_initdt on z
    skl, skm = abstol + np.abs(lam) * reltol, abstol + np.abs(mu) * reltol
    K1 = rhs(lam, s0)
    d0, d1 = _norm(lam / skl, mu / skm, N), _norm(K1[0] / skl, K1[1] / skm, N)
    dt0 = f32(1e-6) if (float(d0) < 1e-5 or float(d1) < 1e-5) else f32(f32(d0 / d1) / f32(100))
    dt0 = min(dt0, dtmax)
    F1 = rhs((lam + dt0 * K1[0]).astype(f32), f32(s0 + dt0))
    d2 = f32(_norm((F1[0] - K1[0]) / skl, (F1[1] - K1[1]) / skm, N) / dt0)
    md = max(d1, d2)
    if float(md) <= 1e-15:
        dt1 = max(f32(1e-6), f32(dt0 * f32(1e-3)))
    else:
        dt1 = f32(10.0 ** float(f32(-(f32(2) + f32(np.log10(float(md)))) / f32(5))))
    dt = min(f32(f32(100) * dt0), dt1, dtmax)
    qoldinit = f32(1e-4)
    s, qold, q11, dtpropose = s0, qoldinit, f32(1), dt
    accept, it, naccept, nreject, nf = False, 0, 0, 0, 3
    imps = [(f32(a), du) for a, du in impulses if f32(a) > s0]
    stops = [f32(a) for a in stops if s0 < f32(a) < s1]
    rows = []
    cs = [R.C[0], R.C[1], R.C[2], R.C[3], 1.0, 1.0]
    lam_n = mu_n = K7 = None
    while s < s1:
        while stops and stops[0] <= s:
            stops.pop(0)
        tstop = stops[0] if stops else s1
        if it > 0:
            if accept:
                lam, mu, K1, dt = lam_n, mu_n, K7, dtpropose
                while imps and imps[0][0] < s:
                    imps.pop(0)
                hit = False
                while imps and imps[0][0] == s and s < s1:
                    lam = (lam + imps.pop(0)[1]).astype(f32)
                    hit = True
                if hit:
                    K1 = rhs(lam, s)
                    nf += 1
            else:
                dt = f32(dt / min(f32(5), f32(q11 / f32(0.9))))
        it += 1
        dt = max(min(dtmax, dt), dtmin)
        dt = min(f32(abs(dt)), f32(abs(f32(tstop - s))))
        if it > maxiters or not dt > dtmin:
            raise RuntimeError("restatement reversed solve did not finish")
        Ks = [K1]
        for st in range(2, 8):
            xl = _lin(lam, dt, R.A[st], [k[0] for k in Ks])
            Ks.append(rhs(xl, f32(s + f32(cs[st - 2]) * dt)))
        lam_n, mu_n, K7 = xl, _lin(mu, dt, R.A[7], [k[1] for k in Ks[:6]]), Ks[6]
        nf += 6
        utl, utm = _lin(None, dt, R.BT, [k[0] for k in Ks]), _lin(None, dt, R.BT, [k[1] for k in Ks])
        eest = _norm(utl / (abstol + np.maximum(np.abs(lam), np.abs(lam_n)) * reltol),
                     utm / (abstol + np.maximum(np.abs(mu), np.abs(mu_n)) * reltol), N)
        q, q11n = _q(eest, qold)
        q11 = q11 if q11n is None else q11n
        accept = bool(eest <= 1)
        rows.append((float(s), float(dt), float(eest), int(accept)))
        if not accept:
            nreject += 1
            continue
        naccept += 1
        qold = max(eest, qoldinit)
        stmp = f32(s + dt)
        s = tstop if abs(f32(stmp - tstop)) < f32(f32(100) * _eps(max(abs(s), abs(tstop)))) else stmp
        dtpropose = max(min(dtmax, f32(dt / q)), max(_eps(s), dtmin))
    if accept:
        lam, mu = lam_n, mu_n
    for a, du in imps:
        if a >= s1:
            lam = (lam + du).astype(f32)
    return lam, mu, (naccept, nreject, nf), rows


def reg_torch(model, p, u1, k1, t1, dt, abstol, reltol, reg_type, dtype=torch.float64):
    """reg_val of one Tsit5 step from (u1, t1) with uprev = u1, k1 and dt constant, as a function of p, and its gradient
    by autograd (the graph of test_step_reg_grad_vs_float64_autograd): returns (value, gradient, value_fn(p))"""
    up, kk1 = torch.tensor(np.asarray(u1), dtype=dtype), torch.tensor(np.asarray(k1), dtype=dtype)
    t1, dt, abstol, reltol = float(f32(t1)), float(f32(dt)), float(f32(abstol)), float(f32(reltol))
    cs = [R.C[0], R.C[1], R.C[2], R.C[3], 1.0, 1.0]
    rms = lambda v: torch.sqrt((v * v).mean())

    def val(pt):
        ft = torch_field(model, pt)
        ks, xs = [kk1], {}
        for s in range(2, 8):
            xs[s] = up + dt * sum(a * k for a, k in zip(R.A[s], ks))
            ks.append(ft(xs[s], t1 + cs[s - 2] * dt))
        u = xs[7]
        if reg_type == "error_estimate":
            utilde = dt * sum(b * k for b, k in zip(R.BT, ks))
            return rms(utilde / (abstol + torch.maximum(up.abs(), u.abs()) * reltol)) * dt
        return (rms(ks[6] - ks[5]) / (rms(u - xs[6]) + float(np.finfo(np.float32).eps))).abs() / 3.5068

    pt = torch.tensor(np.asarray(p), dtype=dtype, requires_grad=True)
    v = val(pt)
    v.backward()
    fn = lambda q: float(val(torch.tensor(np.asarray(q), dtype=dtype)))
    return float(v.detach()), pt.grad.numpy().astype(np.float64), fn


def pullback(model, p, x, times, cots, tol, mode="none", reg_type="error_estimate", t1_or_rand=0.5, save_start=False,
             t0=0.0, t2=1.0, dtype=np.float64, maxiters=10000, want_reg=True, interp=None):
    """the layer's pullback for loss = sum_i <cots[i], sol.u[i]> (+ the regulariser, returned apart as reg_val and
    reg_grad = d reg_val / dp).  `times`: the layer's saveat (ascending, in [t0, t2]; t0 among them needs save_start).
    mode "unbiased": t1 = t1_or_rand joins the saveat of the solve (a tstop of the reversed solve, no cotangent);
    "biased": t1 = ts[int(t1_or_rand * (nsaved - 1))] of the saved times, the last excluded."""
    fld = Field(model, p, dtype)
    times = [float(f32(t)) for t in times]
    sv = list(times)
    if mode == "unbiased":
        t1 = float(f32(t1_or_rand))
        assert t1 not in sv and t0 < t1 < t2
        sv = sorted(sv + [t1])
    fw = forward(fld, x, t0, t2, tol, tol, saveat=sv, save_start=save_start, maxiters=maxiters)
    ts = [float(t) for t in fw["ts"]]
    if mode == "biased":
        mm = len(ts) - 1
        assert mm >= 1
        t1 = ts[min(max(int(f32(t1_or_rand) * f32(mm)), 0), mm - 1)]
    series = [t for t in ts if not (mode == "unbiased" and t == t1)]
    assert len(series) == len(cots), (series, len(cots))
    lam0 = np.zeros_like(x, dtype=f32)
    imps = []
    for t, du in zip(series, cots):
        if t >= f32(t2):
            lam0 = (lam0 + np.asarray(du, f32)).astype(f32)
        else:
            imps.append((-t, np.asarray(du, f32)))
    imps.sort(key=lambda e: e[0])
    stops = sorted(-t for t in ts if t0 < t < t2)
    dx, dp, counts, rows = reverse(fld, Record(fw["steps"], interp or dtype), t0, t2, tol, tol, lam0, imps, stops, maxiters)
    out = dict(dx=dx, dp=dp, counts=counts, rows=rows, fwd=(fw["naccept"], fw["nreject"]), ts=ts, series=series)
    if mode != "none" and want_reg:
        u1 = fw["us"][ts.index(t1)]
        dt1, k1 = R.init_dt(fld, u1, t1, t2, tol, tol)
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        val, grad, fn = reg_torch(model, p, u1, k1, t1, dt1, tol, tol, reg_type, tdt)
        out.update(t1=t1, u1=u1, k1=k1, dt1=float(dt1), reg_val=val, reg_grad=grad, reg_fn=fn)
    return out


# Inputs on which the reversed solve's steps are compared attempt by attempt.  The selection conditions (asserted in
# tests/test_host_chain_adjoint.py on every CPU run, found on the CPU alone): (1) the float64 and the float32 restatement
# take the same (naccept, nreject) and accept pattern, i.e. the decisions are truncation, not rounding of the
# parameter-cotangent sums; (2) the yardstick is self-consistent: two more correct implementations, the mixed twins
# (float32 field with the float64 interpolant, float64 field with the float32 interpolant), pass check_rows, the very
# check the GPU loops are held to.  Where (2) fails, 4 x |row32 - row64| is one unlucky draw of the rounding and says
# nothing about a third implementation: TDChain x3 at tol 1e-5 with an impulse x300 at B = 9 and B = 64 meets (1) and fails
# (2) in the EEst of attempts 10 / 5 and 2 — the rows at which both loops on the MI355X leave the bound too (4.0 % and
# 4.2 % against 2 % and 3.2 %), so those inputs are not used.  `big` multiplies the cotangent of one saved time: the step
# after that impulse is then too long and is rejected.  No input whose plain solve (no impulse) rejects met (1).
PINNED = {
    "td3_x3_tol1e-4_b17": dict(shape="td3_tanh", B=17, scale=3.0, tol=1e-4, times=[0.5, 1.0], big=None, rejects=False),
    "td3_x3_tol1e-4_b33": dict(shape="td3_tanh", B=33, scale=3.0, tol=1e-4, times=[0.5, 1.0], big=None, rejects=False),
    "td3_x3_tol1e-4_impulse_b17": dict(shape="td3_tanh", B=17, scale=3.0, tol=1e-4, times=[0.5, 1.0], big=(0, 1000.0), rejects=True),
}

# Inputs of the regulariser comparison.  reg_val = EEst * dt of a step straight from initdt is small, and its rounding is
# of the order of the 1e-3 bar it is held to (twins 1e-4 .. 3e-3 apart over TDChain tanh / gelu x3, B = 10 / 33 / 64, tol
# 1e-3 / 1e-4).  Selection condition (CPU): 4 x the twins' distance in reg_val is within the bar for both modes and both
# reg_types.  Of the twelve inputs tried this one meets it.
REG_CASE = dict(shape="td3_tanh", B=64, scale=3.0, tol=1e-4, times=[0.25, 0.5, 1.0], t1_or_rand=0.43, cot_scale=0.01)
REG_BAR = 1e-3


def reg_inputs(P):
    c = REG_CASE
    model = shapes(P)[c["shape"]]
    p, x = mk_inputs(P, model, c["B"], scale=c["scale"])
    cots = np.random.default_rng(19).standard_normal((len(c["times"]),) + x.shape).astype(f32) * f32(c["cot_scale"])
    return model, p, x, list(c["times"]), cots, c["tol"]


def pinned_inputs(P, name):
    """(model, p, x, times, cots, tol) of a PINNED case"""
    c = PINNED[name]
    model = shapes(P)[c["shape"]]
    p, x = mk_inputs(P, model, c["B"], scale=c["scale"])
    cots = np.random.default_rng(11).standard_normal((len(c["times"]),) + x.shape).astype(f32)
    if c["big"] is not None:
        cots[c["big"][0]] *= f32(c["big"][1])
    return model, p, x, list(c["times"]), cots, c["tol"]


# the bounds a reversed solve's trace is held to against the float64 restatement's (r64) with the float32 one (r32) as the
# yardstick: relative floors for s (of the span), EEst and dt (dt follows EEst through q = EEst^(7/50): 0.14 x 2e-2), the
# first attempt's dt (initdt, no EEst involved) at 1e-4; each or 4 x |row32 - row64|
S_FLOOR, EEST_FLOOR, DT_FLOOR, DT0_FLOOR, MARGIN = 1e-5, 2e-2, 0.14 * 2e-2, 1e-4, 4.0


def check_rows(tag, got, r64, r32):
    """got: dict(counts, rows) of an implementation; asserts equal counts and accept pattern and every row within bounds"""
    assert got["counts"] == r64["counts"], (tag, got["counts"], r64["counts"])
    assert len(got["rows"]) == len(r64["rows"]) == len(r32["rows"])
    smax = max(abs(r[0]) for r in r64["rows"])
    worst = {"s": 0.0, "dt": 0.0, "EEst": 0.0}
    for i, (g, a, b) in enumerate(zip(got["rows"], r64["rows"], r32["rows"])):
        assert g[3] == a[3], (tag, "accepted", i, g, a)
        floors = (S_FLOOR * smax, (DT0_FLOOR if i == 0 else DT_FLOOR) * abs(a[1]), EEST_FLOOR * abs(a[2]))
        for k, name in enumerate(("s", "dt", "EEst")):
            bound = max(floors[k], MARGIN * abs(b[k] - a[k]))
            d = abs(g[k] - a[k])
            worst[name] = max(worst[name], d / bound)
            assert d <= bound, (tag, name, "attempt", i, g, a, b, bound)
    print(f"{tag}: counts {got['counts']}, {len(got['rows'])} rows; worst |row - row64| / bound: "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    return worst
