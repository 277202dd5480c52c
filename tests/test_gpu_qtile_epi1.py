"""Epilogue 1 of the 4-column kernels (lrnde_qtile.hpp Epi1Q, q_epilogue1): the Dense-1 segment sum, time column, bias
and activation of one C-fragment element per thread, as straight-line code whose per-thread invariants the register form
of k_step_q makes once per launch.  What the code decides, and the smallest shapes that reach each side of it:
  D = 784, 112           seven K-segments (every add real) and one (offsets clamped, no add)
  H = 100, 64, 36        two row groups with a ragged second (KT = 1: the register form, invariants hoisted); one exact
                         group (KT = 4: the LDS form, invariants per f-eval); one ragged group (KT = 1), threads past the
                         256 elements that own nothing
  B = 4, 5               a full tile; a second workgroup with a single valid column
  time-dependent or not  the t column's fma or none
  tanh, gelu, identity   the wave-uniform dispatch; tanh in its select form
tanh runs twice per shape: with the Glorot draw (pre-activations about +-0.8: the polynomial and the exp piece), and with
W1 and b1 scaled by 8 so that the saturated piece occurs too.  The condition is checked on the CPU, before the GPU is
asked, on the pre-activations recomputed in float64 from the parameters the oracle gets: at least 5 % of the real h
values in each of |x| < 0.625 and 0.625 <= |x| < 9, and at least 8 with |x| >= 9.  (Scale 12 leaves under 5 % below 0.625
in 9 of the 24 shapes, scales of 6 and less fewer than 8 saturated values in some; 8 meets it in all: 5.6 .. 13 %,
12 .. 74 values.)  Every comparison is `==` against the C oracle."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DS = [784, 112]
HS = [100, 64, 36]
BS = [4, 5]
CASES = [(D, H, B, td, act, scaled)
         for D in DS for H in HS for B in BS for td in (True, False)
         for act, scaled in (("tanh", False), ("tanh", True), ("gelu", False), ("identity", False))]
SCALE = 8.0   # of W1 (with its t column) and b1 in the scaled tanh run


def _model(pkg, D, H, td, act):
    k = int(td)
    chain = pkg.Chain(pkg.Dense(D + k, H, act), pkg.Dense(H + k, D))
    return pkg.TDChain(chain) if td else chain


def _preact(p, x, t, D, H, td):
    """W1 [x; t] + b1 in float64, (B, H)"""
    k = int(td)
    W1 = p[:H * (D + k)].astype(np.float64).reshape(D + k, H)
    b1 = p[H * (D + k):H * (D + k) + H].astype(np.float64)
    xx = np.concatenate([x.astype(np.float64), np.full((x.shape[0], 1), t)], axis=1) if td else x.astype(np.float64)
    return xx @ W1 + b1


def _pieces(pre):
    a = np.abs(pre)
    return float((a < 0.625).mean()), float(((a >= 0.625) & (a < 9.0)).mean()), int((a >= 9.0).sum())


T_RHS = 0.37


@functools.lru_cache(maxsize=None)
def _mk(D, H, B, td, act, scaled):
    import torch
    import lrnde_amd as pkg
    import oracle as O
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    seed = D + H + B + 2 * int(td)
    model = _model(pkg, D, H, td, act)
    p = pkg.glorot_params(model, seed=seed)
    rng = np.random.default_rng(seed + 1)
    p = p + (rng.standard_normal(p.size).astype(np.float32) * np.float32(0.01))  # non-zero biases
    x = rng.random((B, D), dtype=np.float32)
    if scaled:
        p[:H * (D + int(td)) + H] *= np.float32(SCALE)
    fld = O.MlpField(D, H, p, time_dep=td, act=act, nthreads=8)
    h = Handle(_mlp_desc(model))
    h.set_params(torch.from_numpy(p))
    return fld, h, x, p


def _eq(a, b, what):
    a = np.asarray(a); b = np.asarray(b)
    assert a.shape == b.shape, what
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    assert not bad.any(), f"{what}: {bad.sum()} of {a.size} differ, max abs {np.abs(a - b)[bad].max()}"


def _step_eq(oracle, fld, h, x, t, dt):
    import torch
    k1 = fld.rhs(x, t)
    ref = oracle.tsit5_step(fld, x, k1, t, dt, 1e-4, 1e-4)
    got = h.perform_step(torch.from_numpy(x).cuda(), torch.from_numpy(k1).cuda(), t, dt, 1e-4, 1e-4)
    _eq(got["u"].cpu().numpy(), ref["u"], "u")
    _eq(got["k7"].cpu().numpy(), ref["k7"], "k7")
    for k in ("eest", "reg_error", "reg_stiff"):
        _eq(np.float64(got[k]), np.float64(ref[k]), k)


@pytest.mark.parametrize("D,H,B,td,act,scaled", CASES)
def test_rhs_step_forward_bit_exact(oracle, gpu_pkg, D, H, B, td, act, scaled):
    import torch
    fld, h, x, p = _mk(D, H, B, td, act, scaled)
    if act == "tanh":  # the pieces of tanh this case reaches, from the CPU alone
        small, mid, sat = _pieces(_preact(p, x, T_RHS, D, H, td))
        assert small >= 0.05 and mid >= 0.05 and (sat >= 8 or not scaled), (small, mid, sat)
    xd = torch.from_numpy(x).cuda()
    _eq(h.rhs(xd, T_RHS).cpu().numpy(), fld.rhs(x, T_RHS), "rhs")
    _step_eq(oracle, fld, h, x, 0.1, 0.05)
    tol = 1e-3
    ref = oracle.node_forward(fld, x, 0.0, 1.0, tol, tol, mode="unbiased", reg_type="error_estimate", t1_or_rand=0.43,
                              maxiters=10000)
    got = h.node_forward(xd, 0.0, 1.0, tol, tol, mode="unbiased", reg_type="error_estimate", t1_or_rand=0.43,
                         maxiters=10000)
    assert got["nfe"] == ref["nfe"] and got["reg_val"] == ref["reg_val"], (got["nfe"], ref["nfe"], got["reg_val"], ref["reg_val"])
    for k in ("naccept", "nreject"):
        assert got["stats"][k] == ref["stats"][k], (k, got["stats"], ref["stats"])
    _eq(got["u_end"].cpu().numpy(), ref["u_end"], "sol.u[end]")


@pytest.mark.parametrize("H", HS)
def test_nan_in_one_column(oracle, gpu_pkg, H):
    """one NaN in one sample's input: that sample's h, hence its k, is NaN in every row, the other columns of the tile
    (and the padded Dense-1 rows, whose h meets zero weights) stay what they are"""
    import torch
    D, B = 112, 5
    fld, h, x, _ = _mk(D, H, B, True, "tanh", False)
    x = x.copy()
    x[1, 3] = np.nan
    ref = fld.rhs(x, T_RHS)
    assert np.isnan(ref[1]).all() and not np.isnan(np.delete(ref, 1, axis=0)).any()
    got = h.rhs(torch.from_numpy(x).cuda(), T_RHS).cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern of k"
    _eq(got, ref, "rhs")
    _step_eq(oracle, fld, h, x, 0.1, 0.05)
