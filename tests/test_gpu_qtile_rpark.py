"""The weight stream of the 4-column kernels addresses a fragment as (lane offset + quad in the load's immediate offset,
one scalar base per block and row group), and the register form of the step kernel (k_step_q<*, 1>: H = 97..100) keeps
one stream block per wave in registers for the whole launch (lrnde_qtile.hpp q_stream_fetch_quad, QRPARK): each wave loads
the block's eight fragments at the head of the launch and every f-eval's MFMAs take them where they lie.  What can go
wrong: a quad or a block offset that lands on another fragment (immediate against scalar part, Dense-1 against Dense-2
base, the base carried from one block to the next past a parked block), out-of-range lanes that must stay out of range
with the immediate added (rows past H or D, the 16 rows of the next wave's segment, waves without rows: their register
block is all zeros), a register block that survives a launch (parameters replaced), the block's registers clobbered by
the epilogues of the recorded forward, and the generic form (H = 64: KT = 4), whose Dense-2 quads past ceil(H/4) must
fetch zeros.  Every comparison is `==` against the C oracle."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DS = [784, 336, 112, 100]   # all seven waves own rows; three; one; one with a ragged segment (waves 1..6 park zeros)
HS = [100, 97]              # both KT = 1 (25 k-quads); 97: one real k in the last Dense-2 quad, 33 rows in W1's second group
BS = [4, 6, 509]            # one full tile; a second workgroup with two columns; 128 workgroups, the last with one column
SHAPES = [(D, H, B) for D in DS for H in HS for B in BS]


def _params(D, H, seed, scale):
    import lrnde_amd as pkg
    model = pkg.TDChain(pkg.Chain(pkg.Dense(D + 1, H, "tanh"), pkg.Dense(H + 1, D)))
    p = pkg.glorot_params(model, seed=seed) * np.float32(scale)
    rng = np.random.default_rng(seed + 1)
    return model, p + (rng.standard_normal(p.size).astype(np.float32) * np.float32(0.01))  # non-zero biases


@functools.lru_cache(maxsize=None)
def _mk(D, H, B, scale):
    import torch
    import oracle as O
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    seed = 3 * D + H + B
    model, p = _params(D, H, seed, scale)
    x = np.random.default_rng(seed + 2).random((B, D), dtype=np.float32)
    fld = O.MlpField(D, H, p, time_dep=True, act="tanh", nthreads=8)
    h = Handle(_mlp_desc(model))
    h.set_params(torch.from_numpy(p))
    return fld, h, x


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
        assert got[k] == ref[k], (k, got[k], ref[k])


def _solve_eq(oracle, fld, h, x, t1, tol):
    import torch
    ref = oracle.solve(fld, x, 0.0, t1, tol, tol, maxiters=10000, cap=600)
    assert ref["retcode"] == 0 and ref["stats"]["naccept"] >= 2, ref["stats"]
    got = h.solve(torch.from_numpy(x).cuda(), 0.0, t1, tol, tol, maxiters=10000, cap=600)
    for k in ("nf", "naccept", "nreject", "iters", "nsaved", "dt_init", "t_final"):
        assert got["stats"][k] == ref["stats"][k], (k, got["stats"], ref["stats"])
    _eq(got["t"], ref["t"], "sol.t")
    _eq(got["u"].cpu().numpy(), ref["u"], "sol.u")


@pytest.mark.parametrize("D,H,B", SHAPES)
def test_perform_step_bit_exact(oracle, gpu_pkg, D, H, B):
    """one attempted step: six f-evals on the register block the head of the same launch loaded"""
    fld, h, x = _mk(D, H, B, 1.0)
    _step_eq(oracle, fld, h, x, 0.1, 0.05)


@pytest.mark.parametrize("D,H,B", SHAPES)
def test_short_solve_bit_exact(oracle, gpu_pkg, D, H, B):
    """a short adaptive solve at tol 1e-4 (weights x4: a handful of steps): the init launches (k_init*_q: the generic
    stream with one f-eval) and every step launch load their own block"""
    fld, h, x = _mk(D, H, B, 4.0)
    _solve_eq(oracle, fld, h, x, 0.5, 1e-4)


def test_parameters_replaced_between_launches(oracle, gpu_pkg):
    """step, set_params with other weights, step on the same handle: the second launch's head reloads the register block"""
    import torch
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    D, H, B = 336, 100, 6
    model, p1 = _params(D, H, 31, 1.0)
    _, p2 = _params(D, H, 32, 1.5)
    assert not np.array_equal(p1, p2)
    x = np.random.default_rng(33).random((B, D), dtype=np.float32)
    h = Handle(_mlp_desc(model))
    for p in (p1, p2):
        h.set_params(torch.from_numpy(p))
        _step_eq(oracle, oracle.MlpField(D, H, p, time_dep=True, act="tanh", nthreads=8), h, x, 0.1, 0.05)


@pytest.mark.parametrize("D,H,B", [(336, 100, 6), (112, 97, 4)])
def test_recorded_forward_and_backward_bit_exact(oracle, gpu_pkg, D, H, B):
    """the dense record on: node_forward_record (store_k = 1, the in-kernel record slot written from the lane's
    registers beside the register block), then the recorded backward: dx and dp against the oracle"""
    import torch
    fld, h, x = _mk(D, H, B, 1.5)
    tol, t1 = 1e-4, 0.43
    ref = oracle.node_forward(fld, x, 0.0, 1.0, tol, tol, mode="unbiased", reg_type="error_estimate", t1_or_rand=t1, maxiters=10000)
    got = h.node_forward_record(torch.from_numpy(x).cuda(), 0.0, 1.0, tol, tol, mode="unbiased", reg_type="error_estimate",
                                t1_or_rand=t1, maxiters=10000)
    assert got["nfe"] == ref["nfe"] and got["reg_val"] == ref["reg_val"], (got["nfe"], ref["nfe"], got["reg_val"], ref["reg_val"])
    assert got["reg_val"] != 0.0
    for k in ("naccept", "nreject"):
        assert got["stats"][k] == ref["stats"][k], (k, got["stats"], ref["stats"])
    _eq(got["u_end"].cpu().numpy(), ref["u_end"], "sol.u[end]")
    g = (np.random.default_rng(D + B).standard_normal(x.shape) * 1e-2).astype(np.float32)
    bo = oracle.node_backward(fld, x, 0.0, 1.0, tol, tol, g, mode="unbiased", reg_type="error_estimate", t1_or_rand=t1, w_reg=1.5)
    bg = h.node_backward_recorded(torch.from_numpy(g).cuda(), w_reg=1.5)
    assert bo["retcode"] == 0
    for k in ("naccept", "nreject", "nf"):
        assert bg["stats_bwd"][k] == bo["stats_bwd"][k], (k, bg["stats_bwd"], bo["stats_bwd"])
    _eq(bg["dx"].cpu().numpy(), bo["dx"], "dx")
    _eq(bg["dp"].cpu().numpy(), bo["dp"], "dp")


def test_generic_form_h64_bit_exact(oracle, gpu_pkg):
    """H = 64: 16 real Dense-2 k-quads of 28, KT = 4.  The generic offset path: the twelve quads past ceil(H/4) are
    fetched out of range (zeros) in every f-eval, W1 has one row group (the second is out of range as a whole)"""
    D, H, B = 336, 64, 6
    fld, h, x = _mk(D, H, B, 1.0)
    _step_eq(oracle, fld, h, x, 0.1, 0.05)
    fld4, h4, x4 = _mk(D, H, B, 4.0)
    _solve_eq(oracle, fld4, h4, x4, 0.5, 1e-4)
