"""Helper, not a test: oracle.sde_node_forward's loop restated in float32 numpy with the STEP as a parameter — the reference
passes whatever n.solver is to `solve` and to the local step (src/layers/neural_sde.jl:68-69,96,116).  The steps themselves
are the committed C oracle's (oracle.euler_heun_step / rkmil_step / sri_step, read-only), as are the automatic initial dt
(oracle.sde_init_dt with the kind's strong order) and lro_fastpow.  Everything else — the PI controller on EEst, the
quantisation of the proposal to the path's grid, the series / entry / value rules, the per-kind evaluation counts and the
local step — follows oracle.sde_node_forward line by line; tests/test_host_sde_adaptive.py pins the Euler-Heun case to it
bit for bit.

Per attempted step (drift, diffusion) evaluations: Euler-Heun (3, 3), Milstein (1, 2), SRI (4, 4); automatic initial dt (2, 2).
Strong orders for the initial dt (UPSTREAM-RECALL): 1/2, 1, 3/2."""
import numpy as np

KINDS = {"EulerHeun": dict(nf=3, ng=3, order=0.5), "RKMil": dict(nf=1, ng=2, order=1.0), "SRI": dict(nf=4, ng=4, order=1.5)}
f32 = np.float32


def _as32(a):
    return np.ascontiguousarray(a, dtype=f32)


def make_step(O, kind, drift, diffusion, abstol, reltol, delta, tableau=None):
    """step(u, dW, dZ, t, dt) -> dict(u, eest, reg_val) through the C oracle"""
    if kind == "EulerHeun":
        return lambda u, dW, dZ, t, dt: O.euler_heun_step(drift, diffusion, u, dW, t, dt, abstol, reltol, delta)
    if kind == "RKMil":
        return lambda u, dW, dZ, t, dt: O.rkmil_step(drift, diffusion, u, dW, t, dt, abstol, reltol)
    if kind == "SRI":
        assert tableau is not None
        return lambda u, dW, dZ, t, dt: O.sri_step(drift, diffusion, tableau, u, dW, dZ, t, dt, abstol, reltol, delta)
    raise ValueError(kind)


def grid_begin(dt0, h, nfine):
    """the fresh state of the controller on the path's grid: dt0 quantised to whole intervals of h (at least one, at most the
    grid), the first attempt counted, the proposal kept as a real number"""
    dt0, h = f32(dt0), f32(h)
    return dict(status="running", i=0, m=min(max(int(f32(dt0 / h)), 1), nfine), naccept=0, nreject=0, iters=1, qold=f32(1e-4), dtc=dt0)


def grid_update(c, ee, dt, h, nfine, consts, fp):
    """one attempt's verdict on the state `c` (in place): the PI controller on EEst with the caller's constants (fp: the
    oracle's fastpow), the proposal as a real number and its floor on the grid, the reject rule, the clamp to the end of
    the grid, the attempt count.  status: "running", "done", "DtNaN", "DtLessThanMin" (maxiters is the caller's check of iters)"""
    gamma, qmin, qmax, beta1, beta2 = consts
    ee, dt, h = f32(ee), f32(dt), f32(h)
    if not ee == ee:
        c["status"] = "DtNaN"
        return c
    q = f32(f32(1) / qmax) if ee == 0 else max(f32(f32(1) / qmax), min(f32(f32(1) / qmin), f32(f32(fp(ee, beta1) / fp(c["qold"], beta2)) / gamma)))
    c["dtc"] = f32((max(c["dtc"], dt) if ee <= 1 else dt) / q)   # the proposal stays a real number; the step is its floor on the grid
    mnew = max(int(f32(c["dtc"] / h)), 1)
    if ee <= 1:
        c["naccept"] += 1
        c["qold"], c["i"], c["m"] = max(ee, f32(1e-4)), c["i"] + c["m"], mnew
        if c["i"] >= nfine:
            c["status"] = "done"
            return c
    else:
        c["nreject"] += 1
        if c["m"] == 1:
            c["status"] = "DtLessThanMin"
            return c
        c["m"] = mnew if mnew < c["m"] else c["m"] - 1
    c["m"] = min(c["m"], nfine - c["i"])
    c["iters"] += 1
    return c


def series_plan(t0, t2, nfine, steps, mode, t1_or_rand, save_start, saveat):
    """(sol, e1, t1, series) on the accepted steps [(i, m)]: what the solve saves as entries (t, k, theta) — the value is
    (1 - theta) state_before(step k) + theta state_after(step k), k = -1 the start value —, where the local step starts, and the
    caller's series after the corrected-solution filter.  Raises AssertionError with the layer's text for its refusals."""
    t0, t2 = f32(t0), f32(t2)
    h = f32(f32(t2 - t0) / f32(nfine))
    K = len(steps)
    tk = lambda k: f32(t0 + f32(steps[k][0]) * h)
    tk1 = lambda k: t2 if steps[k][0] + steps[k][1] >= nfine else f32(t0 + f32(steps[k][0] + steps[k][1]) * h)

    def entry(ts):
        ts = f32(ts)
        if not ts > t0:
            return (ts, -1, f32(0))
        k = 0
        while k < K - 1 and tk1(k) < ts:
            k += 1
        th = f32(1) if ts >= tk1(k) else f32(f32(ts - tk(k)) / f32(f32(steps[k][1]) * h))
        return (ts, k, th)

    sv_user = [f32(v) for v in saveat]
    needs_corr = everystep = False
    t1 = t2
    if mode == "unbiased":
        t1 = f32(t1_or_rand)
        assert t0 <= t1 <= t2, "t1 outside tspan"
        if sv_user:
            sv = sorted(sv_user + [t1]); needs_corr = True
        else:
            sv = [t1, t2]
    elif sv_user:
        sv = sv_user
    elif mode == "biased":
        sv, everystep = [], True
    else:
        sv = [t2]
    with_start = save_start > 0 if save_start >= 0 else (everystep or (len(sv) > 0 and sv[0] == t0))
    sol = [(t0, -1, f32(0))] if with_start else []
    if everystep:
        sol += [(tk1(k), k, f32(1)) for k in range(K)]
    else:
        sol += [entry(ts) for ts in sv if not (ts == t0 and with_start)]
    assert sol, "the solve saves nothing"
    e1 = None
    if mode == "biased":
        mm = len(sol) - 1
        assert mm >= 1, ":biased needs at least two saved times"
        idx = min(max(int(f32(t1_or_rand) * f32(mm)), 0), mm - 1)
        e1 = sol[idx]; t1 = e1[0]
    elif mode == "unbiased":
        e1 = entry(t1)
    if mode != "none":
        assert t1 < t2, "t1 must lie before the end of tspan"
    return sol, e1, t1, [e for e in sol if not (needs_corr and e[0] == t1)]


def sde_node_forward(O, kind, drift, diffusion, x, W, t0, t2, abstol, reltol, mode="unbiased", t1_or_rand=0.5, z_local=None, saveat=(),
                     save_start=-1, delta=1.0 / 6.0, dt0=0.0, gamma=0.9, qmin=0.2, qmax=1.125, beta1=7.0 / 50.0, beta2=2.0 / 25.0,
                     maxiters=10000, tableau=None, Z=None, z2_local=None):
    """dict(u (nseries,B,D), t, reg_val, nfe_drift, nfe_diffusion, naccept, nreject, steps [(i, m)], t1, dt_local, u1, dW_local,
    series, dt0) as oracle.sde_node_forward, plus dZ_local.  Raises AssertionError where that loop does (maxiters, DtLessThanMin)."""
    K_ = KINDS[kind]
    x = _as32(x); W = _as32(W)
    if kind == "SRI":
        Z = _as32(Z)
        assert Z.shape == W.shape
    nfine = W.shape[0] - 1
    t0, t2 = f32(t0), f32(t2)
    h = f32(f32(t2 - t0) / f32(nfine))
    fp = lambda a, b: f32(O.lib().lro_fastpow(float(a), float(b)))
    gamma, qmin, qmax, beta1, beta2 = f32(gamma), f32(qmin), f32(qmax), f32(beta1), f32(beta2)
    step = make_step(O, kind, drift, diffusion, abstol, reltol, delta, tableau)
    nff = ngg = 0
    d0 = f32(dt0)
    if not d0 > 0:
        d0 = O.sde_init_dt(drift, diffusion, x, t0, t2, abstol, reltol, order=K_["order"]); nff += 2; ngg += 2
    c, u = grid_begin(d0, h, nfine), x
    steps, states = [], []
    while c["i"] < nfine:
        assert c["iters"] <= maxiters
        i, m = c["i"], c["m"]
        t, dt = f32(t0 + f32(i) * h), f32(f32(m) * h)
        dZ = (Z[i + m] - Z[i]).astype(f32) if kind == "SRI" else None
        r = step(u, (W[i + m] - W[i]).astype(f32), dZ, t, dt)
        grid_update(c, r["eest"], dt, h, nfine, (gamma, qmin, qmax, beta1, beta2), fp)
        assert c["status"] != "DtNaN", "DtNaN"
        assert c["status"] != "DtLessThanMin", "DtLessThanMin: the path's grid cannot be refined further"
        if r["eest"] <= 1:
            steps.append((i, m)); states.append(r["u"]); u = r["u"]
    nacc, nrej = c["naccept"], c["nreject"]
    nff += K_["nf"] * (nacc + nrej); ngg += K_["ng"] * (nacc + nrej)

    def value(e):
        ts, k, th = e
        if k < 0:
            return x
        if th == 1:
            return states[k]
        a = x if k == 0 else states[k - 1]
        return (f32(f32(1) - th) * a + th * states[k]).astype(f32)

    sol, e1, t1, series = series_plan(t0, t2, nfine, steps, mode, t1_or_rand, save_start, saveat)
    reg, dtl, u1, dwl, dzl = f32(0), f32(0), None, None, None
    if mode != "none":
        u1 = value(e1)
        dtl = f32(dt0)
        if not dtl > 0:
            dtl = O.sde_init_dt(drift, diffusion, u1, t1, t2, abstol, reltol, order=K_["order"]); nff += 2; ngg += 2
        dtl = min(dtl, f32(t2 - t1))
        dwl = (f32(np.sqrt(dtl)) * _as32(z_local)).astype(f32)
        if kind == "SRI":
            dzl = (f32(np.sqrt(dtl)) * _as32(z2_local)).astype(f32)
        reg = step(u1, dwl, dzl, t1, dtl)["reg_val"]
        nff += K_["nf"]; ngg += K_["ng"]
    return dict(u=np.stack([value(e) for e in series]), t=np.array([e[0] for e in series], f32), reg_val=reg, nfe_drift=nff,
                nfe_diffusion=ngg, naccept=nacc, nreject=nrej, steps=steps, t1=t1, dt_local=dtl, u1=u1, dW_local=dwl, dZ_local=dzl,
                series=series, dt0=d0)


def brownian_path(rng, nfine, B, D, span=1.0):
    """(nfine + 1, B, D) float32, row 0 zero: the running float32 sum of sqrt(h) N(0, 1) increments"""
    h = f32(span) / f32(nfine)
    inc = (rng.standard_normal((nfine, B, D)) * np.sqrt(h)).astype(f32)
    return np.concatenate([np.zeros((1, B, D), f32), np.cumsum(inc, axis=0, dtype=f32)], axis=0)


def sde_params(D, H, seed):
    """flat Lux parameters of drift Chain(Dense(D => H), Dense(H => D)) and diffusion Dense(D => D): glorot-uniform weights, small biases"""
    rng = np.random.default_rng(seed)
    l1, l2, l3 = np.sqrt(6.0 / (D + H)), np.sqrt(6.0 / (H + D)), np.sqrt(6.0 / (2 * D))
    pd = np.concatenate([(rng.random(H * D) * 2 - 1) * l1, rng.standard_normal(H) * 0.05,
                         (rng.random(D * H) * 2 - 1) * l2, rng.standard_normal(D) * 0.05]).astype(f32)
    pg = np.concatenate([(rng.random(D * D) * 2 - 1) * l3, rng.standard_normal(D) * 0.05]).astype(f32)
    return pd, pg


def oracle_fields(O, D, H, pd, pg, act="tanh"):
    drift = O.MlpField(D, H, pd, time_dep=False, act=act, nthreads=4)
    p2 = np.concatenate([np.eye(D, dtype=f32).ravel(), np.zeros(D, f32), pg])
    return drift, O.MlpField(D, D, p2, time_dep=False, act="identity", nthreads=4)


def case_inputs(D, H, B, nfine, seed, scale=2.0, second_path=False):
    """the pinned inputs of a case: parameters (drift scaled), x, W, z and — for SRI — Z, z2, all from the case's seed"""
    pd, pg = sde_params(D, H, seed)
    pd = (pd * f32(scale)).astype(f32)
    rng = np.random.default_rng(seed + 100)
    x = rng.standard_normal((B, D)).astype(f32)
    W = brownian_path(rng, nfine, B, D)
    z = rng.standard_normal((B, D)).astype(f32)
    out = dict(pd=pd, pg=pg, x=x, W=W, z=z, Z=None, z2=None)
    if second_path:
        out["Z"] = brownian_path(rng, nfine, B, D)
        out["z2"] = rng.standard_normal((B, D)).astype(f32)
    return out


def sri_tableau(O, seed, scale):
    """a fixed-seed tableau (the project does not restate SOSRI's): uniform(-0.6, 0.9) draws as the gradient tests use, times `scale`"""
    rng = np.random.default_rng(seed)
    return {k: float(f32(rng.uniform(-0.6, 0.9) * scale)) for k in O.SRI_FIELDS}
