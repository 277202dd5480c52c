"""What tests/test_gpu_sde_alg_sweep.py and tests/test_host_sde_alg_sweep.py share: the cases of the one-launch reverse sweep of
Milstein / SRI records (csrc/lrnde_sde_bwd_alg_fused.hpp), the float64 autograd reference over the recorded grid, and the
sweep's gate restated on the CPU side.

* the shapes are the pinned cases of tests/test_host_sde_adaptive.py::CASES (each ends OK with >= 3 accepted steps in every mode)
  plus two 12 x 20 cases for the diffusion without a bias, pinned the same way by the host suite here;
* `autograd64` is `_autograd64` of tests/test_gpu_sde_adaptive_alg.py (float64 torch autograd through the float64 steps of
  tests/test_gpu_sde_gradients.py over ref["steps"]), with three switches the host suite uses to show that each compared gradient
  reacts to what the sweep must get right: other (i, m) pairs, dZ replaced by dW, a series cotangent put wholly on one step end;
* `sweep_lds_bytes` / `sweep_gate` restate sbf_smem_bytes_xg and sde_alg_bwd_fused_ok (csrc)."""
import numpy as np
import torch

import sde_adaptive_np as S
from test_gpu_sde_gradients import _fields64, _mil_step64, _rel, _sri_step64  # noqa: F401  (_rel re-exported)
from test_host_sde_adaptive import CASES, case_id

f32 = np.float32
MIL = [c for c in CASES if c["kind"] == "RKMil"]
SRI = [c for c in CASES if c["kind"] == "SRI"]
# diffusion Dense(D => D, bias = false): dp_diff has D * D entries
NOBIAS = [dict(kind="RKMil", shape=(12, 20, 9, 32), seed=7, tol=1.5, dt0=0.0, bias=False),
          dict(kind="SRI", shape=(12, 20, 9, 32), seed=7, tol=0.5, dt0=0.0, tab=(41, 0.1), bias=False)]
SWEEP_CASES = [MIL[1], MIL[2], MIL[0], MIL[5], SRI[0], SRI[2], SRI[1]]      # each must take the one-launch sweep
GATE_CORNER = MIL[3]                                                          # (64, 128): whichever route the gate gives it

# mode, w_reg, saveat, save_start, which series entries carry a cotangent, t1_or_rand
FORMS = {
    "unbiased-w2": dict(mode="unbiased", w_reg=2.0, saveat=(), save_start=-1, du="all", t1=0.37),
    "biased": dict(mode="biased", w_reg=2.0, saveat=(), save_start=-1, du="all", t1=0.43),
    "none-w0": dict(mode="none", w_reg=0.0, saveat=(), save_start=-1, du="all", t1=0.43),
    "saveat-interpolated": dict(mode="unbiased", w_reg=2.0, saveat=(0.3, 0.77, 1.0), save_start=-1, du="all", t1=0.37),
    "saveat-with-start": dict(mode="unbiased", w_reg=2.0, saveat=(0.0, 0.5, 1.0), save_start=1, du="all", t1=0.37),
    "end-state-only": dict(mode="unbiased", w_reg=2.0, saveat=(), save_start=-1, du="end", t1=0.37),
}


def cid(c):
    return case_id(c) + ("" if c.get("bias", True) else "-nobias")


def has_bias(c):
    return c.get("bias", True)


_REF = {}


def reference(O, c, form=None, **kw):
    """(inputs, tableau, the helper's forward result) of a case, computed once per (case, arguments) and left unchanged"""
    args = {}
    if form is not None:
        f = FORMS[form]
        args = dict(mode=f["mode"], t1_or_rand=f["t1"], saveat=f["saveat"], save_start=f["save_start"])
    args.update(kw)
    key = (cid(c), c["dt0"], tuple(sorted((k, tuple(v) if isinstance(v, (tuple, list)) else v) for k, v in args.items())))
    if key not in _REF:
        D, H, B, nfine = c["shape"]
        inp = S.case_inputs(D, H, B, nfine, c["seed"], second_path=c["kind"] == "SRI")
        if not has_bias(c):
            inp["pg"] = np.ascontiguousarray(inp["pg"][:D * D])
        pg_full = inp["pg"] if has_bias(c) else np.concatenate([inp["pg"], np.zeros(D, f32)])
        drift, diff = S.oracle_fields(O, D, H, inp["pd"], pg_full)
        T = S.sri_tableau(O, *c["tab"]) if c["kind"] == "SRI" else None
        a = dict(mode="unbiased", t1_or_rand=0.43, z_local=inp["z"], dt0=c["dt0"], tableau=T, Z=inp["Z"], z2_local=inp["z2"])
        a.update(args)
        _REF[key] = (inp, T, S.sde_node_forward(O, c["kind"], drift, diff, inp["x"], inp["W"], 0.0, 1.0, c["tol"], c["tol"], **a))
    return _REF[key]


def cotangents(c, ref, form):
    """the series cotangents of a form: standard normal on every entry, or on sol.u[end] alone"""
    D, H, B, nfine = c["shape"]
    ns = len(ref["t"])
    du = np.random.default_rng(5).standard_normal((ns, B, D)).astype(f32)
    if FORMS[form]["du"] == "end":
        du[:-1] = 0
    return du


def autograd64(c, inp, T, ref, du_series, w_reg, steps=None, swap_dz=False, series_end=None):
    """loss = sum_j <du_j, sol.u[j]> + w_reg * reg_val in float64 over the RECORDED grid (ref['steps']), by torch autograd:
    (dx, dp_drift, dp_diff).  steps: other (i, m) pairs; swap_dz: dZ := dW in every step; series_end: 0 / 1 puts every
    interpolated series value wholly on its step's start / end state"""
    D, H, B, nfine = c["shape"]
    tol, delta = c["tol"], 1.0 / 6.0
    t64 = lambda a: torch.tensor(a, dtype=torch.float64)
    pdt, pgt, xt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (inp["pd"], inp["pg"], inp["x"]))
    pg_full = pgt if has_bias(c) else torch.cat([pgt, torch.zeros(D, dtype=torch.float64)])
    f, g = _fields64(pdt, pg_full, D, H)
    hh = 1.0 / nfine
    Wt = t64(inp["W"])
    Zt = t64(inp["Z"]) if c["kind"] == "SRI" else None

    def step(u, dW, dZ, dt):
        if c["kind"] == "RKMil":
            un = _mil_step64(f, g, u, dW, dt)
            r = (un - u) / (tol + torch.maximum(u.abs(), un.abs()) * tol)     # :166-169, the four-argument residual
            return un, torch.sqrt((r * r).mean()) * dt
        return _sri_step64(f, g, T, u, dW, dW if swap_dz else dZ, dt, tol, tol, delta)
    states, u = [], xt
    for (i, m) in (ref["steps"] if steps is None else steps):
        u = step(u, Wt[i + m] - Wt[i], None if Zt is None else Zt[i + m] - Zt[i], m * hh)[0]
        states.append(u)
    loss = 0.0
    for j, (ts, k, th) in enumerate(ref["series"]):
        if k < 0:
            val = xt
        else:
            a = xt if k == 0 else states[k - 1]
            th = float(th)
            if series_end is not None and 0.0 < th < 1.0:
                th = float(series_end)
            val = (1.0 - th) * a + th * states[k]
        loss = loss + (val * t64(du_series[j])).sum()
    if ref["u1"] is not None and w_reg != 0.0:
        loss = loss + w_reg * step(t64(ref["u1"]), t64(ref["dW_local"]), None if ref["dZ_local"] is None else t64(ref["dZ_local"]),
                                   float(ref["dt_local"]))[1]
    loss.backward()
    z = lambda p: (p.grad if p.grad is not None else torch.zeros_like(p)).numpy()
    return z(xt), z(pdt), z(pgt)


# ---- the sweep's gate on the CPU side (sbf_off / sbf_smem_bytes_xg / sde_alg_bwd_fused_ok) ----
SBF_NS, SBF_MAXSER, LDS_LIMIT = 4, 512, 160 * 1024


def _up4(n):
    return (n + 3) & ~3


def sweep_lds_bytes(D, H, kind):
    """dynamic LDS of the sweep (and of the regulariser's kernel) of a kind: weights with odd leading dimensions and biases, the
    four samples' vector blocks (Milstein 2 evaluation points, SRI 4 with their own diffusion input), the parameter cotangent"""
    nev, own = (4, True) if kind == "SRI" else (2, False)
    Dq, Hq = _up4(D), _up4(H)
    VS = Dq + 4 + Hq + Hq + Dq + Dq + (Dq if own else 0)
    return 4 * (_up4((H + 1) * Dq + 4) + _up4((D + 1) * Hq + 4) + _up4((D + 1) * Dq + 4) + Hq + 2 * Dq + SBF_NS * nev * VS
                + D * H * 2 + H + D + D * D + D)


def sweep_gate(D, H, kind, nseries=1):
    """True where lrnde_sde_node_backward_recorded takes the one-launch sweep for an unsharded handle without a time input"""
    return D <= 64 and H <= 128 and nseries <= SBF_MAXSER and sweep_lds_bytes(D, H, kind) + 8 * SBF_MAXSER + 1024 <= LDS_LIMIT
