"""The register form of the step kernel (k_step_q<*, 1>: H = 97..100) requests its weight stream by a compile-time
schedule (lrnde_qsched.hpp, QSchedEarly): a quad of the next global block goes into a ring slot's quad as soon as the
MFMAs that read those registers are done, the parked blocks hold no slot of their own, the slot a block's MFMAs read is
the table's and no longer a rotation, and the last f-eval of a launch requests nothing for a seventh.  What can go wrong on
the device: MFMAs that read another slot than the one the schedule filled (a wrong fragment, or one still in flight
where the counted wait was derived for another register), a parked read that overwrites a quad still to be multiplied,
a launch that starts from the slot state the head leaves after a launch that ended without wrap loads, the epilogue
stores and the g6 / record traffic that share the stream's counter, parameters replaced between launches, and the generic
form (H = 64: KT = 4), which keeps the closed-form schedule.  Every comparison is `==` against the C oracle.  (That every
block is requested at all, which no bit comparison can see, is tests/test_host_qsched.py's.)"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DS = [784, 336, 112, 100]   # all seven waves own rows; three; one; one with a ragged segment
HS = [100, 97]              # both KT = 1 (25 k-quads); 97: one real k in the last Dense-2 quad
BS = [4, 6, 509]            # one full tile; a second workgroup with two columns; 128 workgroups, the last with one column
SHAPES = [(D, H, B) for D in DS for H in HS for B in BS]
TWO = [(336, 100, 6), (112, 97, 4)]


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
    seed = 5 * D + H + B
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
    """one attempted step: six chained f-evals, each with its own table and slot map"""
    fld, h, x = _mk(D, H, B, 1.0)
    _step_eq(oracle, fld, h, x, 0.1, 0.05)


@pytest.mark.parametrize("D,H,B", SHAPES)
def test_short_solve_bit_exact(oracle, gpu_pkg, D, H, B):
    """a short adaptive solve at tol 1e-4 (weights x4, at least two accepted steps): a launch follows a launch whose
    last f-eval issued no wrap loads, and starts again from the slot state the head leaves"""
    fld, h, x = _mk(D, H, B, 4.0)
    _solve_eq(oracle, fld, h, x, 0.5, 1e-4)


@pytest.mark.parametrize("D,H,B", TWO)
def test_forward_with_stiffness_estimate_bit_exact(oracle, gpu_pkg, D, H, B):
    """node_forward with reg_type = stiffness_estimate: the g6 store of stage 5, its load in the last epilogue and the
    stiffness sums ride in the stream's vmcnt count"""
    import torch
    fld, h, x = _mk(D, H, B, 1.5)
    tol, t1 = 1e-4, 0.43
    ref = oracle.node_forward(fld, x, 0.0, 1.0, tol, tol, mode="unbiased", reg_type="stiffness_estimate", t1_or_rand=t1, maxiters=10000)
    got = h.node_forward(torch.from_numpy(x).cuda(), 0.0, 1.0, tol, tol, mode="unbiased", reg_type="stiffness_estimate",
                         t1_or_rand=t1, maxiters=10000)
    assert got["nfe"] == ref["nfe"] and got["reg_val"] == ref["reg_val"], (got["nfe"], ref["nfe"], got["reg_val"], ref["reg_val"])
    assert got["reg_val"] != 0.0
    for k in ("naccept", "nreject"):
        assert got["stats"][k] == ref["stats"][k], (k, got["stats"], ref["stats"])
    _eq(got["u_end"].cpu().numpy(), ref["u_end"], "sol.u[end]")


@pytest.mark.parametrize("D,H,B", TWO)
def test_recorded_forward_and_backward_bit_exact(oracle, gpu_pkg, D, H, B):
    """node_forward_record (store_k = 1: the k stores of every stage and the in-kernel record slot beside the stream), then
    the recorded backward: dx and dp against the oracle"""
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


def test_parameters_replaced_between_launches(oracle, gpu_pkg):
    """step, set_params with other weights, step on the same handle: nothing of the first launch's stream survives"""
    import torch
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    D, H, B = 336, 100, 6
    model, p1 = _params(D, H, 41, 1.0)
    _, p2 = _params(D, H, 42, 1.5)
    assert not np.array_equal(p1, p2)
    x = np.random.default_rng(43).random((B, D), dtype=np.float32)
    h = Handle(_mlp_desc(model))
    for p in (p1, p2):
        h.set_params(torch.from_numpy(p))
        _step_eq(oracle, oracle.MlpField(D, H, p, time_dep=True, act="tanh", nthreads=8), h, x, 0.1, 0.05)


def test_generic_form_h64_bit_exact(oracle, gpu_pkg):
    """H = 64 (KT = 4, the LDS form, which keeps the closed-form schedule): one step and one short solve"""
    D, H, B = 336, 64, 6
    fld, h, x = _mk(D, H, B, 1.0)
    _step_eq(oracle, fld, h, x, 0.1, 0.05)
    fld4, h4, x4 = _mk(D, H, B, 4.0)
    _solve_eq(oracle, fld4, h4, x4, 0.5, 1e-4)
