"""The register form of the 4-column step kernel (k_step_q<*, 1>: H = 97..100) parks two weight stream blocks per wave in
LDS for the whole launch (lrnde_qtile.hpp QPARK): waves 1..6 fill all seven waves' regions at the head of the launch with
the stream's own buffer loads, and every f-eval reads the parked fragments back with ds_read_b128.  What can go wrong is
the fill's addressing (a fragment of another wave, quad or row group in a wave's region; out-of-range lanes that must
park zeros: rows past H or D, the 16 rows of the next wave's segment, waves without rows), the ordering of the fill
before the first parked read, a region that survives a launch (parameters replaced, a second workgroup on the CU), and
the unparked generic form (H = 96, KT = 4) picking anything up.  Every comparison is `==` against the C oracle."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DS = [784, 700, 112, 100]   # all waves own rows; a ragged 7th wave without a second group; one wave, six empty regions; one ragged segment
HS = [100, 97, 96]          # KT = 1 twice (97: 33 real rows in W1's second row group, one real k in the last Dense-2 quad); 96: KT = 4, unparked
BS = [4, 5]                 # a full tile; a second workgroup with three empty columns
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
    seed = D + H + B
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


@pytest.mark.parametrize("D,H,B", SHAPES)
def test_perform_step_bit_exact(oracle, gpu_pkg, D, H, B):
    """one launch: every f-eval of it reads the fragments the head of the same launch parked"""
    fld, h, x = _mk(D, H, B, 1.0)
    _step_eq(oracle, fld, h, x, 0.1, 0.05)


@pytest.mark.parametrize("D,H,B", SHAPES)
def test_short_solve_with_a_rejection_bit_exact(oracle, gpu_pkg, D, H, B):
    """weights x20 at a loose tolerance over a short span: the controller's dt is too long two to seven times, depending
    on the shape, in 44 to 68 accepted steps, so the launches of the solve (accepted, rejected, repeated) each fill and
    read their own park"""
    import torch
    fld, h, x = _mk(D, H, B, 20.0)
    t1, tol = 1.0, 1e-3
    ref = oracle.solve(fld, x, 0.0, t1, tol, tol, maxiters=10000, cap=600)
    assert ref["retcode"] == 0 and ref["stats"]["nreject"] >= 1, ref["stats"]
    got = h.solve(torch.from_numpy(x).cuda(), 0.0, t1, tol, tol, maxiters=10000, cap=600)
    for k in ("nf", "naccept", "nreject", "iters", "nsaved", "dt_init", "t_final"):
        assert got["stats"][k] == ref["stats"][k], (k, got["stats"], ref["stats"])
    _eq(got["t"], ref["t"], "sol.t")
    _eq(got["u"].cpu().numpy(), ref["u"], "sol.u")


def test_parameters_replaced_between_launches(oracle, gpu_pkg):
    """step, set_params with other weights, step on the same handle: the second launch parks the new weights"""
    import torch
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    D, H, B = 112, 100, 5
    model, p1 = _params(D, H, 11, 1.0)
    _, p2 = _params(D, H, 12, 1.5)
    assert not np.array_equal(p1, p2)
    x = np.random.default_rng(13).random((B, D), dtype=np.float32)
    h = Handle(_mlp_desc(model))
    for p in (p1, p2):
        h.set_params(torch.from_numpy(p))
        _step_eq(oracle, oracle.MlpField(D, H, p, time_dep=True, act="tanh", nthreads=8), h, x, 0.1, 0.05)


def test_two_rounds_of_workgroups_on_one_cu(oracle, gpu_pkg):
    """257 workgroups on a chip of 256 CUs, one workgroup per CU at a time: the one that runs second on its CU finds the
    first one's park in LDS and must refill it with its own"""
    D, H, B = 112, 100, 1028
    model, p = _params(D, H, 21, 1.0)
    import torch
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    x = np.random.default_rng(22).random((B, D), dtype=np.float32)
    h = Handle(_mlp_desc(model))
    h.set_params(torch.from_numpy(p))
    _step_eq(oracle, oracle.MlpField(D, H, p, time_dep=True, act="tanh", nthreads=8), h, x, 0.1, 0.05)


def test_recorded_forward_bit_exact(oracle, gpu_pkg):
    """node_forward_record: store_k = 1 and the in-kernel dense record beside the parked stream"""
    import torch
    D, H, B = 112, 100, 5
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
