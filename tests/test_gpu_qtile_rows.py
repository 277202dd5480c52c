"""The 4-column kernels' Dense-2 row ownership (lrnde_qtile.hpp q_w2_groups): wave w produces the rows of its own Dense-1
segment, [112w, 112w + 112), so the segment count and the last wave's partial group vary with D.  The step, rhs and
init launches are compared bit for bit with the oracle over state sizes that give 7, 4 and 1 segments and partial last
segments, hidden sizes on both sides of the Dense-2 tail specialisation, and batches that fill or leave columns of the
last workgroup empty.  H = 128 is beyond the 4-column family (H <= 112) and checks the 16-column kernels at the same
shapes; every other case runs the 4-column kernels, whose row mapping has no fallback (every accepted D maps)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DS = [784, 700, 336, 112, 100]
HS = [100, 64, 128]
BS = [512, 509, 4]


def _mk(O, pkg, D, H, B, seed=0):
    import torch
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    model = pkg.TDChain(pkg.Chain(pkg.Dense(D + 1, H, "tanh"), pkg.Dense(H + 1, D)))
    p = pkg.glorot_params(model, seed=seed)
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


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("D", DS)
def test_step_rhs_init_bit_exact(oracle, gpu_pkg, D, H, B):
    import torch
    fld, h, x = _mk(oracle, gpu_pkg, D, H, B, seed=D + H + B)
    xd = torch.from_numpy(x).cuda()
    ref_rhs = fld.rhs(x, 0.37)
    _eq(h.rhs(xd, 0.37).cpu().numpy(), ref_rhs, "rhs")
    dt_ref, f0_ref = oracle.init_dt(fld, x, 0.0, 1.0, 1e-4, 1e-4)
    dt, f0 = h.init_dt(xd, 0.0, 1.0, 1e-4, 1e-4)
    assert dt == dt_ref, (dt, dt_ref)
    _eq(f0.cpu().numpy(), f0_ref, "fsalfirst")
    k1 = fld.rhs(x, 0.1)
    ref = oracle.tsit5_step(fld, x, k1, 0.1, 0.05, 1e-4, 1e-4)
    got = h.perform_step(xd, torch.from_numpy(k1).cuda(), 0.1, 0.05, 1e-4, 1e-4)
    _eq(got["u"].cpu().numpy(), ref["u"], "u")
    _eq(got["k7"].cpu().numpy(), ref["k7"], "k7")
    for k in ("eest", "reg_error", "reg_stiff"):
        assert got[k] == ref[k], (k, got[k], ref[k])


@pytest.mark.parametrize("D,H,B", [(700, 64, 509), (100, 100, 4)])
def test_regularised_forward_bit_exact(oracle, gpu_pkg, D, H, B):
    """a whole regularised forward (many step launches, the dense record written by the step itself) at
    shapes whose last segment is partial"""
    import torch
    fld, h, x = _mk(oracle, gpu_pkg, D, H, B, seed=7)
    for reg_type in ("error_estimate", "stiffness_estimate"):
        ref = oracle.node_forward(fld, x, 0.0, 1.0, 1e-5, 1e-5, mode="unbiased", reg_type=reg_type, t1_or_rand=0.43,
                                  maxiters=10000)
        got = h.node_forward(torch.from_numpy(x).cuda(), 0.0, 1.0, 1e-5, 1e-5, mode="unbiased", reg_type=reg_type,
                             t1_or_rand=0.43, maxiters=10000)
        assert got["nfe"] == ref["nfe"] and got["reg_val"] == ref["reg_val"], (got["nfe"], ref["nfe"])
        _eq(got["u_end"].cpu().numpy(), ref["u_end"], "sol.u[end] " + reg_type)
