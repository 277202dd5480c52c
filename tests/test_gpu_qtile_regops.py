"""The 4-column step kernel keeps the stage operands (uprev, k1 .. k6) of a tile in the registers of the lane that produces
the rows (lrnde_qtile.hpp RegOpsQ): every wave preloads both candidate (uprev, k1) pairs of its own Dense-2 rows, selects
one with the prologue's parity, and forms x2 for its own segment of the x tile.  What can go wrong is ownership (which
lane holds which row: ragged last segment, waves without rows, a second row group with fewer than 48 real rows, columns
past the batch) and the parity select (a rejected step repeats from the un-flipped pair).  Every comparison is `==`
against the C oracle, on every shape: the single step, a solve with rejected steps that saves inside steps and at every
step, and the recorded forward (the in-kernel dense record and store_k = 1) with both regularisers, whose record is
checked through the pullback it feeds."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DS = [784, 700, 112, 100]   # 7 segments; a ragged 7th (28 rows: no second group); one full segment; one ragged (36 rows in group 1)
HS = [100, 64]              # the Dense-2 tail specialisation (25 k-quads) and the generic form
BS = [4, 5, 9]              # a full tile; one and three empty columns in the last tile; more than one workgroup
SHAPES = [(D, H, B) for D in DS for H in HS for B in BS]


@functools.lru_cache(maxsize=None)
def _mk(D, H, B, scale):
    import torch
    import oracle as O
    import lrnde_amd as pkg
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    seed = D + H + B
    model = pkg.TDChain(pkg.Chain(pkg.Dense(D + 1, H, "tanh"), pkg.Dense(H + 1, D)))
    p = pkg.glorot_params(model, seed=seed) * np.float32(scale)
    rng = np.random.default_rng(seed + 1)
    p = p + (rng.standard_normal(p.size).astype(np.float32) * np.float32(0.01))  # non-zero biases
    x = rng.random((B, D), dtype=np.float32)
    fld = O.MlpField(D, H, p, time_dep=True, act="tanh", nthreads=8)
    h = Handle(_mlp_desc(model))
    h.set_params(torch.from_numpy(p))
    return fld, h, x


def _eq(a, b, what):
    a = np.asarray(a); b = np.asarray(b)
    assert a.shape == b.shape, what
    bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
    assert not bad.any(), f"{what}: {bad.sum()} of {a.size} differ, max abs {np.abs(a - b)[bad].max()}"


@pytest.mark.parametrize("D,H,B", SHAPES)
def test_perform_step_bit_exact(oracle, gpu_pkg, D, H, B):
    """lrnde_perform_step: one launch, parity 0, u / k7 / the error norm and both regulariser sums"""
    import torch
    fld, h, x = _mk(D, H, B, 1.0)
    k1 = fld.rhs(x, 0.1)
    ref = oracle.tsit5_step(fld, x, k1, 0.1, 0.05, 1e-4, 1e-4)
    got = h.perform_step(torch.from_numpy(x).cuda(), torch.from_numpy(k1).cuda(), 0.1, 0.05, 1e-4, 1e-4)
    _eq(got["u"].cpu().numpy(), ref["u"], "u")
    _eq(got["k7"].cpu().numpy(), ref["k7"], "k7")
    for k in ("eest", "reg_error", "reg_stiff"):
        assert got[k] == ref[k], (k, got[k], ref[k])


@pytest.mark.parametrize("D,H,B", SHAPES)
def test_solve_with_rejections_and_saves_bit_exact(oracle, gpu_pkg, D, H, B):
    """weights x6 over a long span at a loose tolerance: the controller's dt is repeatedly too long and steps are rejected
    (3 to 23 of them, depending on the shape), so the launch after a rejection selects the pair of the un-flipped parity;
    the save points lie strictly inside steps, and every step is saved"""
    import torch
    fld, h, x = _mk(D, H, B, 6.0)
    t1, tol = 25.0, 5e-4
    sv = [t1 * f for f in (0.137, 0.5, 0.823)]
    ref = oracle.solve(fld, x, 0.0, t1, tol, tol, saveat=sv, save_everystep=True, maxiters=10000, cap=600)
    assert ref["retcode"] == 0 and ref["stats"]["nreject"] >= 1, ref["stats"]
    acc = ref["trace"][ref["trace"]["accepted"] != 0]
    for ts in np.float32(sv):  # each save point is interpolated: no accepted step starts or ends on it
        assert ((acc["t"] < ts) & (ts < acc["t"] + acc["dt"])).any(), (ts, acc)
    got = h.solve(torch.from_numpy(x).cuda(), 0.0, t1, tol, tol, saveat=sv, save_everystep=True, maxiters=10000, cap=600)
    for k in ("nf", "naccept", "nreject", "iters", "nsaved", "dt_init", "t_final"):
        assert got["stats"][k] == ref["stats"][k], (k, got["stats"], ref["stats"])
    _eq(got["t"], ref["t"], "sol.t")
    _eq(got["u"].cpu().numpy(), ref["u"], "sol.u")


@pytest.mark.parametrize("reg_type", ["error_estimate", "stiffness_estimate"])
@pytest.mark.parametrize("D,H,B", SHAPES)
def test_recorded_forward_and_its_record_bit_exact(oracle, gpu_pkg, D, H, B, reg_type):
    """the recorded layer forward: every attempted step writes its record slot from the lane's registers and stores
    k2..k6 (store_k = 1); stiffness_estimate adds the g6 store of stage 5 and its load in the last epilogue.  The record
    is what the pullback integrates over, so dx and dp equal to the oracle's are the check of its contents."""
    import torch
    fld, h, x = _mk(D, H, B, 1.5)
    tol, t1 = 1e-4, 0.43
    ref = oracle.node_forward(fld, x, 0.0, 1.0, tol, tol, mode="unbiased", reg_type=reg_type, t1_or_rand=t1, maxiters=10000)
    got = h.node_forward_record(torch.from_numpy(x).cuda(), 0.0, 1.0, tol, tol, mode="unbiased", reg_type=reg_type,
                                t1_or_rand=t1, maxiters=10000)
    assert got["nfe"] == ref["nfe"] and got["reg_val"] == ref["reg_val"], (got["nfe"], ref["nfe"], got["reg_val"], ref["reg_val"])
    assert got["reg_val"] != 0.0
    for k in ("naccept", "nreject"):
        assert got["stats"][k] == ref["stats"][k], (k, got["stats"], ref["stats"])
    _eq(got["u_end"].cpu().numpy(), ref["u_end"], "sol.u[end]")
    g = (np.random.default_rng(D + B).standard_normal(x.shape) * 1e-2).astype(np.float32)
    bo = oracle.node_backward(fld, x, 0.0, 1.0, tol, tol, g, mode="unbiased", reg_type=reg_type, t1_or_rand=t1, w_reg=1.5)
    bg = h.node_backward_recorded(torch.from_numpy(g).cuda(), w_reg=1.5)
    assert bo["retcode"] == 0
    for k in ("naccept", "nreject", "nf"):
        assert bg["stats_bwd"][k] == bo["stats_bwd"][k], (k, bg["stats_bwd"], bo["stats_bwd"])
    _eq(bg["dx"].cpu().numpy(), bo["dx"], "dx")
    _eq(bg["dp"].cpu().numpy(), bo["dp"], "dp")
