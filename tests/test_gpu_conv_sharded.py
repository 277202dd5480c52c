"""The batch-sharded conv handle (lrnde_conv_comm_*) on ONE GPU: R `ConvHandle`s of this process, each on
its own HIP stream and host thread, joined by the in-process local communicator — as tests/test_gpu_sharded_loopback.py
does for the MLP handle.  Rank r owns images [r*B, (r+1)*B) of the global batch.

Two yardsticks, neither of them the code under test:
  (U) one unsharded handle of the same library on the global batch,
  (O) oracle.ConvField on the global batch.
Bars against (O) are the ones tests/test_gpu_conv.py holds the unsharded handle to; each is cited where it is used.
Inputs follow test_gpu_conv._case (seeded glorot parameters times `scale`, random BatchNorm affine), restated in
tests/conv_sharded_cases.py with the helpers this file and tests/test_gpu_conv_sharded_envelope.py share.

Seeds of the solve cases: for every seed used below the oracle's trace on the global batch was checked on the CPU
(seeds 5, 6, 7, 8 at 16x16 B=4 for tol 1e-3 / scale 3 and tol 1e-4 / scale 1.5; 21, 22, 23 at 8x8 B=4, tol 1e-3, scale 2;
41, 42, 43 at 8x8 B=3, tol 1e-4, scale 1.5).  All of them take 6-8 accepted steps, reject none, and their largest EEst of
an attempted step is below 0.01, far outside [0.98, 1.02]: equal accept / reject counts are a condition the oracle itself
meets with margin.  The tests use seeds 5, 21 and 41; each asserts the margin again on the oracle's trace.
None of those solves rejects a step (at scales up to 12, tolerances down to 1e-4 and spans up to (0, 16) the field's EEst
stays below 0.04), so test_sharded_solve_takes_the_oracles_rejected_step adds one that does: seed 21 at 8x8 B=4, scale 40,
tol 1e-5 (checked with scales 40 and 150, gelu and tanh): 29 accepted steps and one rejected at EEst 1.28, the largest
accepted EEst 0.68 - both a quarter away from the threshold."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu

from conv_sharded_cases import (BLOCKS, BN0, _dist, _field, _handle, _inputs, _mods, _ranks, _rel,  # noqa: E402
                                _run, _shards)


# R, B per rank, W, H, activation, training mode
RHS_SHAPES = [
    pytest.param(2, 1, 8, 8, "gelu", True, id="2x1@8x8"),        # one image per rank, one strip per image
    pytest.param(3, 1, 16, 16, "gelu", True, id="3x1@16x16"),    # odd rank count, two strips per image
    pytest.param(2, 3, 12, 8, "tanh", True, id="2x3@12x8-tanh"),  # ragged strip
    pytest.param(2, 2, 32, 32, "gelu", True, id="2x2@32x32"),    # CIFAR shape
    pytest.param(2, 2, 28, 28, "gelu", False, id="2x2@28x28-test"),
]
TS = (0.0, 0.613)


@functools.lru_cache(maxsize=None)
def _rhs_refs(R, Bl, W, H, act, train, dtype="f32"):
    """(U) and (O) of the f-eval cases, computed once: U at both times (one fresh handle, in order), its running
    statistics after the first f-eval, and the oracle's f-evals (fp32 only)"""
    B = R * Bl
    p, u, st = _inputs(W, H, B, W + B, train)
    hu = _handle(W, H, p, st, act, train, dtype)
    ud = torch.from_numpy(u).cuda()
    U, bn1 = [], None
    for t in TS:
        U.append(hu.rhs(ud, t).cpu().numpy())
        if bn1 is None:
            bn1 = hu.get_bn_state().cpu().numpy()
    Oo = None
    if dtype == "f32":
        fld = _field(W, H, p, st, act, train)
        Oo = [fld.rhs(u.reshape(B, -1), t).reshape(u.shape) for t in TS]
    return U, bn1, Oo


# ---- 1. rhs, gather form: the unsharded bits -------------------------------------------------------------------------
@pytest.mark.parametrize("R,Bl,W,H,act,train", RHS_SHAPES)
def test_rhs_gather_form_gives_the_unsharded_bits(R, Bl, W, H, act, train):
    B = R * Bl
    p, u, st = _inputs(W, H, B, W + B, train)
    U, _, _ = _rhs_refs(R, Bl, W, H, act, train)
    lc, hs = _ranks(R, W, H, p, st, act, train, gather=True)
    us = _shards(u, R)
    for i, t in enumerate(TS):
        got = _run([(lambda r=r: hs[r].rhs(us[r], t)) for r in range(R)])
        assert torch.equal(torch.cat(got).cpu(), torch.from_numpy(U[i])), f"t={t}"
    lc.close()


@pytest.mark.parametrize("dtype", ["bf16", "f32_split"])
def test_rhs_gather_form_gives_the_unsharded_bits_other_dtypes(dtype):
    R, Bl, W, H = 2, 2, 8, 8
    p, u, st = _inputs(W, H, R * Bl, W + R * Bl, True)
    U, _, _ = _rhs_refs(R, Bl, W, H, "gelu", True, dtype)
    lc, hs = _ranks(R, W, H, p, st, dtype=dtype, gather=True)
    us = _shards(u, R)
    for i, t in enumerate(TS):
        got = _run([(lambda r=r: hs[r].rhs(us[r], t)) for r in range(R)])
        assert torch.equal(torch.cat(got).cpu(), torch.from_numpy(U[i])), f"t={t}"
    lc.close()


# ---- 2. rhs, default (pre-reduced) form ------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Bl,W,H,act,train", RHS_SHAPES)
def test_rhs_default_form_matches_unsharded_and_oracle(R, Bl, W, H, act, train):
    """<= 1e-5 of scale against (U) and (O) (test_conv_rhs_matches_oracle's RTOL); the running statistics after one
    training-mode f-eval equal (U)'s at rtol 2e-5, atol 1e-6 (test_conv_running_statistics_match_oracle) and are the same
    bits on every rank"""
    B = R * Bl
    p, u, st = _inputs(W, H, B, W + B, train)
    U, bn1, Oo = _rhs_refs(R, Bl, W, H, act, train)
    lc, hs = _ranks(R, W, H, p, st, act, train)
    us = _shards(u, R)
    for i, t in enumerate(TS):
        got = torch.cat(_run([(lambda r=r: hs[r].rhs(us[r], t)) for r in range(R)]))
        du, do = _dist(got, U[i]), _dist(got, Oo[i])
        print(f"rhs default form {R}x{Bl}@{W}x{H} t={t}: vs U {du:.3e} (zero: {du == 0.0}), vs O {do:.3e}")
        assert du <= 1e-5 and do <= 1e-5
        if i == 0:
            bn = [h.get_bn_state() for h in hs]
            for b in bn:
                assert torch.equal(b, bn[0])
                if train:
                    np.testing.assert_allclose(b.cpu().numpy(), bn1, rtol=2e-5, atol=1e-6)
                    assert not np.array_equal(b.cpu().numpy(), BN0)
                else:
                    assert np.array_equal(b.cpu().numpy(), st)
    lc.close()


# ---- 3. one forced rank: RCCL itself as the transport ----------------------------------------------------------------
def test_one_forced_rccl_rank_gives_the_unsharded_bits(monkeypatch):
    P, O = _mods()
    W = H = 8; B = 3
    p, u, st = _inputs(W, H, B, 61, True, 3.0)
    monkeypatch.setenv("LRNDE_FORCE_COMM", "1")
    monkeypatch.delenv("LRNDE_GATHER_TILES", raising=False)
    hu = _handle(W, H, p, st)
    hf = _handle(W, H, p, st)
    assert hu.comm_count() == (1, 0)
    P.init_comm(hf, 0, 1)
    assert hf.comm_count() == (1, 1)
    ud = torch.from_numpy(u).cuda()
    lam = torch.from_numpy(np.random.default_rng(3).standard_normal(u.shape).astype(np.float32)).cuda()
    tol = 1e-3

    def battery(h):
        out = {}
        h.set_bn_state(BN0)
        out["rhs"] = h.rhs(ud, 0.3)
        dt, k1 = h.init_dt(ud, 0.0, 1.0, tol, tol)
        out["dt"], out["k1"] = dt, k1
        out["step"] = h.perform_step(ud, k1, 0.0, 0.2, tol, tol)
        h.set_bn_state(BN0)
        out["solve"] = h.solve(ud, 0.0, 1.0, tol, tol, saveat=[0.37, 1.0], trace=True)
        h.set_bn_state(BN0)
        out["fwd"] = h.node_forward(ud, 0.0, 1.0, tol, tol, mode="unbiased", t1_or_rand=0.41)
        out["vjp"] = h.vjp(ud, 0.41, lam)
        h.set_bn_state(BN0)
        out["bwd"] = h.node_backward(ud, 0.0, 1.0, tol, tol, lam, mode="unbiased", t1_or_rand=0.41, w_reg=2.5, maxiters=5000)
        out["bn"] = h.get_bn_state()
        return out

    a, b = battery(hu), battery(hf)
    assert hf.comm_stats()[0] > 0 and hu.comm_stats() == (0, 0)
    assert torch.equal(a["rhs"], b["rhs"]) and a["dt"] == b["dt"] and torch.equal(a["k1"], b["k1"])
    for k in ("u", "k7"):
        assert torch.equal(a["step"][k], b["step"][k])
    for k in ("eest", "reg_error", "reg_stiff"):
        assert a["step"][k] == b["step"][k], k
    assert a["solve"]["stats"] == b["solve"]["stats"] and torch.equal(a["solve"]["u"], b["solve"]["u"])
    for f in ("t", "dt", "eest", "accepted"):
        assert np.array_equal(a["solve"]["trace"][f], b["solve"]["trace"][f]), f
    assert a["solve"]["stats"]["naccept"] >= 3
    assert torch.equal(a["fwd"]["u_end"], b["fwd"]["u_end"]) and a["fwd"]["reg_val"] == b["fwd"]["reg_val"]
    assert a["fwd"]["nfe"] == b["fwd"]["nfe"] and a["fwd"]["stats"] == b["fwd"]["stats"]
    assert torch.equal(a["vjp"][0], b["vjp"][0]) and torch.equal(a["vjp"][1], b["vjp"][1])
    assert torch.equal(a["bwd"]["dx"], b["bwd"]["dx"]) and torch.equal(a["bwd"]["dp"], b["bwd"]["dp"])
    assert a["bwd"]["stats_fwd"] == b["bwd"]["stats_fwd"] and a["bwd"]["stats_bwd"] == b["bwd"]["stats_bwd"]
    assert torch.equal(a["bn"], b["bn"])
    hf.close()


# ---- 4. solve and node_forward ---------------------------------------------------------------------------------------
SOLVE_CASES = [pytest.param(2, 2, 16, 1e-3, 3.0, 5, id="2x2@16x16-tol1e-3"), pytest.param(2, 2, 16, 1e-4, 1.5, 5, id="2x2@16x16-tol1e-4"),
               pytest.param(4, 1, 8, 1e-3, 2.0, 21, id="4x1@8x8-tol1e-3")]
MODES = [("unbiased", "error_estimate"), ("biased", "stiffness_estimate"), ("none", "error_estimate")]


@functools.lru_cache(maxsize=None)
def _solve_refs(R, Bl, W, tol, scale, seed):
    P, O = _mods()
    B = R * Bl
    p, u, st = _inputs(W, W, B, seed, True, scale)
    fld = _field(W, W, p, None)
    ro = O.solve(fld, u.reshape(B, -1), 0.0, 1.0, tol, tol, saveat=[0.37, 1.0])
    fo = {m: O.node_forward(_field(W, W, p, None), u.reshape(B, -1), 0.0, 1.0, tol, tol, mode=m, reg_type=rt, t1_or_rand=0.41)
          for m, rt in MODES}
    hu = _handle(W, W, p, None)
    ud = torch.from_numpy(u).cuda()
    ru = hu.solve(ud, 0.0, 1.0, tol, tol, saveat=[0.37, 1.0], trace=True)
    fu = {}
    for m, rt in MODES:
        hu.set_bn_state(BN0)
        fu[m] = hu.node_forward(ud, 0.0, 1.0, tol, tol, mode=m, reg_type=rt, t1_or_rand=0.41)
    return ro, fo, ru, fu


@pytest.mark.parametrize("R,Bl,W,tol,scale,seed", SOLVE_CASES)
def test_sharded_solve_and_node_forward(R, Bl, W, tol, scale, seed):
    """stats equal on all ranks and equal to (U)'s; (naccept, nreject, nf) equal (O)'s; saved states within 2e-5 of scale of
    (O) (test_conv_solve_matches_oracle_step_for_step) and of (U); reg_val equal on all ranks and within 1e-1 relative of
    (O) (test_conv_node_forward_matches_oracle: the local step's estimate is a difference of nearly equal fp32 numbers)"""
    B = R * Bl
    p, u, st = _inputs(W, W, B, seed, True, scale)
    ro, fo, ru, fu = _solve_refs(R, Bl, W, tol, scale, seed)
    e = ro["trace"]["eest"]
    assert not np.any((e >= 0.98) & (e <= 1.02)), "the oracle's own trace has an attempt at the accept threshold"
    lc, hs = _ranks(R, W, W, p, None)
    us = _shards(u, R)
    got = _run([(lambda r=r: hs[r].solve(us[r], 0.0, 1.0, tol, tol, saveat=[0.37, 1.0], trace=True)) for r in range(R)])
    so = ro["stats"]
    for g in got:
        assert g["stats"] == got[0]["stats"] and g["stats"] == ru["stats"]
        assert (g["stats"]["naccept"], g["stats"]["nreject"], g["stats"]["nf"]) == (so["naccept"], so["nreject"], so["nf"])
        for f in ("t", "dt", "eest", "accepted"):
            assert np.array_equal(g["trace"][f], got[0]["trace"][f]), f
        assert list(g["t"]) == [np.float32(0.37), np.float32(1.0)]
    assert so["naccept"] >= 3
    for i in range(2):
        ui = torch.cat([g["u"][i] for g in got])
        du, do = _dist(ui, ru["u"][i].cpu().numpy()), _dist(ui, ro["u"][i])
        print(f"solve {R}x{Bl}@{W}x{W} tol {tol:g} save {i}: vs U {du:.3e} (zero: {du == 0.0}), vs O {do:.3e}")
        assert du <= 2e-5 and do <= 2e-5
    for m, rt in MODES:
        for h in hs:
            h.set_bn_state(BN0)
        gf = _run([(lambda r=r: hs[r].node_forward(us[r], 0.0, 1.0, tol, tol, mode=m, reg_type=rt, t1_or_rand=0.41)) for r in range(R)])
        o_, u_ = fo[m], fu[m]
        for g in gf:
            assert g["stats"] == gf[0]["stats"] and g["stats"] == u_["stats"] and g["nfe"] == u_["nfe"] == o_["nfe"]
            assert (g["stats"]["naccept"], g["stats"]["nreject"]) == (o_["stats"]["naccept"], o_["stats"]["nreject"])
            assert g["reg_val"] == gf[0]["reg_val"] and g["t1"] == gf[0]["t1"]
            if m == "none":
                assert g["reg_val"] == 0.0
            else:
                assert abs(float(g["reg_val"]) - float(o_["reg_val"])) <= 1e-1 * abs(float(o_["reg_val"]))
        ue = torch.cat([g["u_end"] for g in gf])
        du, do = _dist(ue, u_["u_end"].cpu().numpy()), _dist(ue, o_["u_end"])
        print(f"node_forward {m}: u_end vs U {du:.3e} (zero: {du == 0.0}), vs O {do:.3e}; reg_val {gf[0]['reg_val']} U {u_['reg_val']} O {o_['reg_val']}")
        assert du <= 2e-5 and do <= 2e-5
        bn = [h.get_bn_state() for h in hs]
        assert all(torch.equal(b, bn[0]) for b in bn)
    lc.close()


def test_sharded_solve_takes_the_oracles_rejected_step():
    """a solve whose trace HAS a rejected step (module docstring: scale 40, tol 1e-5): every rank rejects the attempt that
    (U) and (O) reject.  stats and the whole trace equal (U)'s and each other's, (naccept, nreject, nf) equal (O)'s, saved
    states within 2e-5 of scale of (U).  No state bar against (O): tests/test_gpu_conv.py holds the unsharded handle to
    none at 30 steps of a field this stiff, so there is none to cite."""
    P, O = _mods()
    R, Bl, W, tol, scale, seed = 2, 2, 8, 1e-5, 40.0, 21
    B = R * Bl
    p, u, st = _inputs(W, W, B, seed, True, scale)
    ro = O.solve(_field(W, W, p, None), u.reshape(B, -1), 0.0, 1.0, tol, tol, saveat=[1.0], maxiters=3000)
    e = ro["trace"]["eest"]
    assert ro["stats"]["nreject"] >= 1 and not np.any((e >= 0.98) & (e <= 1.02))
    ru = _handle(W, W, p, None).solve(torch.from_numpy(u).cuda(), 0.0, 1.0, tol, tol, saveat=[1.0], maxiters=3000, trace=True)
    lc, hs = _ranks(R, W, W, p, None)
    us = _shards(u, R)
    got = _run([(lambda r=r: hs[r].solve(us[r], 0.0, 1.0, tol, tol, saveat=[1.0], maxiters=3000, trace=True)) for r in range(R)])
    so = ro["stats"]
    print(f"rejecting solve: O {so['naccept']}/{so['nreject']}, U {ru['stats']['naccept']}/{ru['stats']['nreject']}, "
          f"ranks {[(g['stats']['naccept'], g['stats']['nreject']) for g in got]}; rejected EEst "
          f"{[float(x) for x, a in zip(got[0]['trace']['eest'], got[0]['trace']['accepted']) if not a]}")
    for g in got:
        assert g["stats"] == ru["stats"]
        assert (g["stats"]["naccept"], g["stats"]["nreject"], g["stats"]["nf"]) == (so["naccept"], so["nreject"], so["nf"])
        for f in ("t", "dt", "eest", "accepted"):
            assert np.array_equal(g["trace"][f], ru["trace"][f]), f
        assert np.array_equal(g["trace"]["accepted"], ro["trace"]["accepted"][:len(g["trace"])])
    assert _dist(torch.cat([g["u"][0] for g in got]), ru["u"][0].cpu().numpy()) <= 2e-5
    lc.close()


# ---- 5. vjp ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,Bl,W,H,train", [pytest.param(2, 2, 8, 8, True, id="2x2@8x8"), pytest.param(3, 1, 16, 16, True, id="3x1@16x16"),
                                            pytest.param(2, 2, 28, 28, False, id="2x2@28x28-test")])
def test_sharded_vjp_matches_oracle(R, Bl, W, H, train):
    """dy blocks and every block of gp (w1, bn1, w2, bn2, w3) within 5e-5 of that block's scale against (O)
    (test_conv_vjp_matches_oracle); a BatchNorm block summed twice, or a weight block not summed, misses it by a factor.
    gp comes out replicated: the same bits on every rank"""
    P, O = _mods()
    B = R * Bl
    p, u, st = _inputs(W, H, B, W + B + 3, train)
    lam = np.random.default_rng(17).standard_normal(u.shape).astype(np.float32)
    dy_ref, gp_ref = O.conv_vjp(_field(W, H, p, st, train=train), u.reshape(B, -1), 0.41, lam.reshape(B, -1))
    lc, hs = _ranks(R, W, H, p, st, train=train)
    us, ls = _shards(u, R), _shards(lam, R)
    got = _run([(lambda r=r: hs[r].vjp(us[r], 0.41, ls[r])) for r in range(R)])
    assert _dist(torch.cat([g[0] for g in got]), dy_ref) <= 5e-5
    gp = got[0][1].cpu().numpy()
    for g in got:
        assert torch.equal(g[1], got[0][1]), "gp must come out replicated"
    for name, sl in BLOCKS:
        sc = np.abs(gp_ref[sl]).max()
        err = np.abs(gp[sl] - gp_ref[sl]).max()
        assert err <= 5e-5 * sc, f"{name}: {err:.3e} vs scale {sc:.3e}"
    # without gp: the same dy
    got2 = _run([(lambda r=r: hs[r].vjp(us[r], 0.41, ls[r], want_gp=False)) for r in range(R)])
    assert all(torch.equal(a[0], b[0]) for a, b in zip(got, got2))
    lc.close()


# ---- 6. step_reg_grad ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg_type", ["error_estimate", "stiffness_estimate"])
def test_sharded_step_reg_grad_matches_oracle(reg_type):
    """the bars of test_conv_step_reg_grad_matches_oracle: reg_val 5e-3 relative, gradient 1e-2 of its scale and norm"""
    P, O = _mods()
    R, Bl, W = 2, 2, 8
    B = R * Bl
    p, u, st = _inputs(W, W, B, 31, True, 2.0)
    fld = _field(W, W, p, None)
    k1 = fld.rhs(u.reshape(B, -1), 0.2)
    dt = 0.25
    g_ref, rv_ref = O.step_reg_grad(fld, u.reshape(B, -1), k1, 0.2, dt, 1e-4, 1e-4, reg_type=reg_type)
    lc, hs = _ranks(R, W, W, p, None)
    us, ks = _shards(u, R), _shards(k1.reshape(u.shape), R)
    got = _run([(lambda r=r: hs[r].step_reg_grad(us[r], ks[r], 0.2, dt, 1e-4, 1e-4, reg_type=reg_type)) for r in range(R)])
    for g, rv in got:
        assert rv == got[0][1] and torch.equal(g, got[0][0])
        assert abs(float(rv) - float(rv_ref)) <= 5e-3 * abs(float(rv_ref))
    g = got[0][0].cpu().numpy()
    assert np.abs(g - g_ref).max() <= 1e-2 * np.abs(g_ref).max()
    assert _rel(g, g_ref) <= 1e-2
    lc.close()


# ---- 7. node_backward and the recorded pair --------------------------------------------------------------------------
@pytest.mark.parametrize("mode,w_reg", [("unbiased", 2.5), ("none", 0.0)])
def test_sharded_node_backward_matches_oracle(mode, w_reg):
    """test_conv_node_backward_matches_oracle's bars on 3 ranks of one image: forward naccept equal to (O)'s, adjoint
    naccept equal on all ranks and within 1 of (O), dx 2e-3 and dp 5e-3 in the relative norm; dp replicated; the recorded
    pair gives the one-call form's bits on every rank"""
    P, O = _mods()
    R, Bl, W = 3, 1, 8
    B = R * Bl
    p, u, st = _inputs(W, W, B, 41, True, 1.5)
    wv = np.random.default_rng(3).standard_normal(u.shape).astype(np.float32)
    tol = 1e-4
    bo = O.node_backward(_field(W, W, p, None), u.reshape(B, -1), 0.0, 1.0, tol, tol, wv.reshape(B, -1), mode=mode, t1_or_rand=0.41,
                         w_reg=w_reg, maxiters=5000)
    assert bo["retcode"] == 0
    hu = _handle(W, W, p, None)
    bu = hu.node_backward(torch.from_numpy(u).cuda(), 0.0, 1.0, tol, tol, torch.from_numpy(wv).cuda(), mode=mode, t1_or_rand=0.41,
                          w_reg=w_reg, maxiters=5000)
    lc, hs = _ranks(R, W, W, p, None)
    us, ws = _shards(u, R), _shards(wv, R)
    kw = dict(mode=mode, t1_or_rand=0.41, maxiters=5000)
    got = _run([(lambda r=r: hs[r].node_backward(us[r], 0.0, 1.0, tol, tol, ws[r], w_reg=w_reg, **kw)) for r in range(R)])
    for g in got:
        assert g["stats_fwd"]["naccept"] == bo["stats_fwd"]["naccept"]
        assert g["stats_bwd"] == got[0]["stats_bwd"]
        assert abs(g["stats_bwd"]["naccept"] - bo["stats_bwd"]["naccept"]) <= 1
        assert torch.equal(g["dp"], got[0]["dp"]), "dp must come out replicated"
        assert _rel(g["dp"], bo["dp"]) <= 5e-3
    dx = torch.cat([g["dx"] for g in got])
    assert _rel(dx.cpu().numpy().reshape(B, -1), bo["dx"]) <= 2e-3
    ddx, ddp = _rel(dx, bu["dx"]), _rel(got[0]["dp"], bu["dp"])
    print(f"node_backward {mode}: vs U dx {ddx:.3e} dp {ddp:.3e} (zero: {ddx == 0.0 and ddp == 0.0}); "
          f"vs O dx {_rel(dx.cpu().numpy().reshape(B, -1), bo['dx']):.3e} dp {_rel(got[0]['dp'], bo['dp']):.3e}")
    for h in hs:
        h.set_bn_state(BN0)

    def pair(r):
        fw = hs[r].node_forward_record(us[r], 0.0, 1.0, tol, tol, **kw)
        return fw, hs[r].node_backward_recorded(Bl, ws[r], w_reg=w_reg)

    two = _run([(lambda r=r: pair(r)) for r in range(R)])
    for r in range(R):
        assert torch.equal(two[r][1]["dx"], got[r]["dx"]) and torch.equal(two[r][1]["dp"], got[r]["dp"])
        assert two[r][1]["stats_bwd"] == got[r]["stats_bwd"] and two[r][0]["stats"] == got[r]["stats_fwd"]
    lc.close()


# ---- 8. stem, head and the training step -----------------------------------------------------------------------------
def test_sharded_stem_and_head_match_oracle():
    """O.cifar_stem_* / O.cifar_head_ce on the global batch at the bars of test_cifar_stem_matches_oracle (1e-5 forward and
    state, 5e-5 backward) and test_cifar_head_matches_oracle (loss 2e-5, logits 2e-5, du 5e-5, dph 5e-5)"""
    P, O = _mods()
    R, Bl, W, K = 2, 2, 8, 10
    B = R * Bl
    rng = np.random.default_rng(W + B)
    x = rng.standard_normal((B, 3, W, W)).astype(np.float32)
    ps = (rng.standard_normal(156) * 0.3).astype(np.float32); ps[140:148] = rng.uniform(0.5, 1.5, 8)
    g = rng.standard_normal((B, 8, W, W)).astype(np.float32)
    p, _, _ = _inputs(W, W, B, 1)
    lc, hs = _ranks(R, W, W, p, None)
    xs, gs = _shards(x, R), _shards(g, R)
    pd = torch.from_numpy(ps).cuda()
    u_o, st_o = O.cifar_stem_forward(x, ps, bn_train=True, return_state=True)
    got = _run([(lambda r=r: hs[r].cifar_stem_forward(xs[r], pd, None, return_state=True)) for r in range(R)])
    assert _dist(torch.cat([q[0] for q in got]), u_o) <= 1e-5
    for q in got:
        assert torch.equal(q[1], got[0][1])
        np.testing.assert_allclose(q[1].cpu().numpy(), st_o, rtol=1e-5, atol=1e-6)
    ref = O.cifar_stem_backward(x, ps, g, bn_train=True)
    gb = _run([(lambda r=r: hs[r].cifar_stem_backward(xs[r], pd, gs[r], None)) for r in range(R)])
    for q in gb:
        assert torch.equal(q, gb[0])
    assert np.abs(gb[0].cpu().numpy() - ref).max() <= 5e-5 * np.abs(ref).max()
    # head
    u = rng.standard_normal((B, 8, W, W)).astype(np.float32)
    ph = (rng.standard_normal(73 + K * W * W + K) * 0.1).astype(np.float32)
    lab = rng.integers(0, K, B).astype(np.int32)
    lo, lg, du, dph = O.cifar_head_ce(u, ph, K, lab)
    uh = _shards(u, R)
    labs = [torch.from_numpy(lab[r * Bl:(r + 1) * Bl].copy()).cuda() for r in range(R)]
    phd = torch.from_numpy(ph).cuda()
    torch.cuda.synchronize()
    hr = _run([(lambda r=r: hs[r].cifar_head_ce(uh[r], phd, K, labs[r])) for r in range(R)])
    for q in hr:
        assert q["loss"] == hr[0]["loss"] and torch.equal(q["dph"], hr[0]["dph"])
        assert abs(float(q["loss"]) - float(lo)) <= 2e-5 * max(1.0, abs(float(lo)))
    assert _dist(torch.cat([q["logits"] for q in hr]), lg) <= 2e-5
    assert _dist(torch.cat([q["du"] for q in hr]), du) <= 5e-5
    assert np.abs(hr[0]["dph"].cpu().numpy() - dph).max() <= 5e-5 * np.abs(dph).max()
    lc.close()


def test_sharded_cifar_training_step():
    """run_cifar_training_step, unchanged, on two joined NeuralODE handles (node.handle(x_shard) is what joins): loss and
    ce_loss equal on both ranks and each within 1e-4 relative of the oracle chain on the global batch (loss: of
    ce(O) + w_reg * reg_val(O)), and loss == float32(ce_loss + w_reg * reg_val) of the returned stats; gradients at the
    bars of test_cifar_training_step_runs_and_is_consistent (neural_ode 1e-2, head 1e-3, stem 1e-2, relative norm).
    Measured on the MI355X: loss and ce_loss 1.0e-7 relative from (O) and 1.0e-7 from the unsharded handle's step (one
    float32 ulp: the stem's BatchNorm(8) sums are grouped by rank); reg_val 3.758e-6 against (O) 3.720e-6, (U) 3.851e-6 —
    the cancellation noise of the local step's estimate, 1e-6 of the loss."""
    import copy
    P, O = _mods()
    R, Bl, W, K = 2, 2, 8, 10
    B = R * Bl
    rng = np.random.default_rng(12)
    pn = P.glorot_conv_params(8, 64, seed=0)
    ps = (rng.standard_normal(156) * 0.3).astype(np.float32); ps[140:148] = 1.0; ps[148:156] = 0.0
    ph = (rng.standard_normal(73 + K * W * W + K) * 0.1).astype(np.float32)
    x = rng.standard_normal((B, 3, W, W)).astype(np.float32)
    lab = rng.integers(0, K, B).astype(np.int32)
    params = dict(stem=torch.from_numpy(ps).cuda(), neural_ode=torch.from_numpy(pn).cuda(), head=torch.from_numpy(ph).cuda())
    xs = _shards(x, R)
    labs = [torch.from_numpy(lab[r * Bl:(r + 1) * Bl].copy()).cuda() for r in range(R)]
    lc = P.LocalComm(R)
    nodes, streams = [], []
    for r in range(R):
        core = P.TDChain(P.Chain(P.Chain(P.Conv((3, 3), 9, 64), P.BatchNorm(64, "gelu")),
                                 P.Chain(P.Conv((3, 3), 65, 64), P.BatchNorm(64, "gelu")), P.Conv((3, 3), 65, 8)))
        node = P.NeuralODE(core, regularize="unbiased", abstol=1e-3, reltol=1e-3, save_start=False, maxiters=2000)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            lc.join(node.handle(torch.empty((Bl, 8, W, W), device="cuda")), r)
        nodes.append(node); streams.append(s)
    st = nodes[0].initialstates(np.random.default_rng(0))
    torch.cuda.synchronize()

    def step(r):
        with torch.cuda.stream(streams[r]):
            return P.run_cifar_training_step(nodes[r], params, copy.deepcopy(st), xs[r], labs[r], 2.5)

    got = _run([(lambda r=r: step(r)) for r in range(R)])
    t1 = np.float32(copy.deepcopy(st["rng"]).random(dtype=np.float32))
    u0 = O.cifar_stem_forward(x, ps)
    fld = O.ConvField(W, W, 8, 64, pn, nthreads=8)
    fo = O.node_forward(fld, u0.reshape(B, -1), 0.0, 1.0, 1e-3, 1e-3, mode="unbiased", t1_or_rand=t1, maxiters=2000)
    lo, lg, du, dph = O.cifar_head_ce(fo["u_end"].reshape(B, 8, W, W), ph, K, lab)
    bo = O.node_backward(fld, u0.reshape(B, -1), 0.0, 1.0, 1e-3, 1e-3, du.reshape(B, -1), mode="unbiased", t1_or_rand=t1, w_reg=2.5,
                         maxiters=2000)
    dstem = O.cifar_stem_backward(x, ps, bo["dx"].reshape(B, 8, W, W))
    lo_tot = float(lo) + 2.5 * float(fo["reg_val"])
    # (U): the same step on one unsharded handle over the global batch — reported, the bars are against (O)
    node_u = P.NeuralODE(P.TDChain(P.Chain(P.Chain(P.Conv((3, 3), 9, 64), P.BatchNorm(64, "gelu")),
                                           P.Chain(P.Conv((3, 3), 65, 64), P.BatchNorm(64, "gelu")), P.Conv((3, 3), 65, 8))),
                         regularize="unbiased", abstol=1e-3, reltol=1e-3, save_start=False, maxiters=2000)
    lu, _, su, _, _ = P.run_cifar_training_step(node_u, params, copy.deepcopy(st), torch.from_numpy(x).cuda(), torch.from_numpy(lab).cuda(), 2.5)
    l0, s0 = got[0][0], got[0][2]
    print(f"training step: loss {float(l0):.9g} (O {lo_tot:.9g}: {abs(float(l0) - lo_tot) / abs(lo_tot):.3e} relative; U {float(lu):.9g}: "
          f"{abs(float(l0) - float(lu)) / abs(float(lu)):.3e}), ce_loss {float(s0['ce_loss']):.9g} (O {float(lo):.9g}: "
          f"{abs(float(s0['ce_loss']) - float(lo)) / abs(float(lo)):.3e}; U {float(su['ce_loss']):.9g}), reg_val {float(s0['reg_val']):.6g} "
          f"(O {float(fo['reg_val']):.6g}, U {float(su['reg_val']):.6g})")
    for loss, st_, stats, grads, times in got:
        assert loss == got[0][0] and stats["ce_loss"] == got[0][2]["ce_loss"] and stats["reg_val"] == got[0][2]["reg_val"]
        assert abs(float(stats["ce_loss"]) - float(lo)) <= 1e-4 * abs(float(lo))
        assert abs(float(loss) - lo_tot) <= 1e-4 * abs(lo_tot)
        assert loss == np.float32(stats["ce_loss"] + np.float32(2.5) * stats["reg_val"])
        for k in grads:
            assert torch.equal(grads[k], got[0][3][k]), k
        assert _rel(grads["neural_ode"], bo["dp"]) <= 1e-2
        assert _rel(grads["head"], dph) <= 1e-3
        assert _rel(grads["stem"], dstem) <= 1e-2
        assert torch.equal(st_["model"]["bn_state"], got[0][1]["model"]["bn_state"])
    lc.close()


# ---- 9. counts and refusals ------------------------------------------------------------------------------------------
# exchanges per call of the default form: an f-eval is two BatchNorm statistics exchanges in training mode and
# none in test mode; init_dt is two f-evals and two norm exchanges; a step is six f-evals and one norm exchange; a VJP is
# the recompute's two, one per BatchNorm backward (needed for m1 / m2 in training mode, for d scale / d bias when gp is
# asked for), and one per weight block when gp is asked for.  The batch check rides in the call's first exchange.
EXCHANGES = {
    ("rhs", True): 2, ("rhs", False): 0,
    ("init_dt", True): 2 * 2 + 2, ("init_dt", False): 2,
    ("perform_step", True): 6 * 2 + 1, ("perform_step", False): 1,
    ("vjp", True): 2 + 2, ("vjp", False): 0,
    ("vjp_gp", True): 2 + 2 + 3, ("vjp_gp", False): 2 + 3,
}


@pytest.mark.parametrize("train", [True, False])
def test_exchange_counts(train):
    R, Bl, W = 2, 2, 8
    p, u, st = _inputs(W, W, R * Bl, 71, train)
    lc, hs = _ranks(R, W, W, p, st, train=train)
    us = _shards(u, R)
    k1 = _run([(lambda r=r: hs[r].rhs(us[r], 0.0)) for r in range(R)])
    calls = {
        "rhs": lambda r: hs[r].rhs(us[r], 0.2),
        "init_dt": lambda r: hs[r].init_dt(us[r], 0.0, 1.0, 1e-3, 1e-3),
        "perform_step": lambda r: hs[r].perform_step(us[r], k1[r], 0.0, 0.1, 1e-3, 1e-3),
        "vjp": lambda r: hs[r].vjp(us[r], 0.3, k1[r], want_gp=False),
        "vjp_gp": lambda r: hs[r].vjp(us[r], 0.3, k1[r]),
    }
    for name, fn in calls.items():
        before = [h.comm_stats() for h in hs]
        _run([(lambda r=r: fn(r)) for r in range(R)])
        after = [h.comm_stats() for h in hs]
        for b, a in zip(before, after):
            assert a[0] - b[0] == EXCHANGES[(name, train)], (name, train, a[0] - b[0])
            assert (a[1] > b[1]) == (EXCHANGES[(name, train)] > 0)
    assert all(h.comm_count() == (R, 2) for h in hs)
    lc.close()


def test_refusals_and_leaving():
    P, O = _mods()
    from localregneuralde_jl_amd import _lib as L
    import ctypes
    import time
    R, W, K = 2, 8, 10
    p, u, st = _inputs(W, W, 6, 81)
    hu = _handle(W, W, p, None)
    ud = torch.from_numpy(u[:4]).cuda()
    want = hu.rhs(ud, 0.3)
    lc, hs = _ranks(R, W, W, p, None)
    # two ranks called with B = 2 and B = 3: both raise BADARG (4) at once, and both handles stay usable
    a, b = torch.from_numpy(u[:2].copy()).cuda(), torch.from_numpy(u[2:5].copy()).cuda()
    torch.cuda.synchronize()
    errs = [None, None]

    def call(r, x):
        try:
            hs[r].rhs(x, 0.3)
        except P.LrndeError as e:
            errs[r] = e

    tic = time.perf_counter()
    _run([lambda: call(0, a), lambda: call(1, b)])
    assert time.perf_counter() - tic < 10.0
    assert all(e is not None and e.code == 4 for e in errs), errs
    assert "2, 3" in str(errs[0]) and "2, 3" in str(errs[1])
    us = _shards(u[:4], R)
    for h in hs:
        h.set_bn_state(BN0)
    got = torch.cat(_run([(lambda r=r: hs[r].rhs(us[r], 0.3)) for r in range(R)]))
    assert _dist(got, want.cpu().numpy()) <= 1e-5
    # a bad label on one rank only: both ranks raise BADARG
    rng = np.random.default_rng(2)
    ph = torch.from_numpy((rng.standard_normal(73 + K * W * W + K) * 0.1).astype(np.float32)).cuda()
    labs = [torch.tensor([1, 2], dtype=torch.int32).cuda(), torch.tensor([3, K], dtype=torch.int32).cuda()]
    torch.cuda.synchronize()
    errs = [None, None]

    def head(r):
        try:
            hs[r].cifar_head_ce(us[r], ph, K, labs[r])
        except P.LrndeError as e:
            errs[r] = e

    _run([lambda: head(0), lambda: head(1)])
    assert all(e is not None and e.code == 4 and "label" in str(e) for e in errs), errs
    # joining a rank twice, and a rank outside the communicator
    extra = _handle(W, W, p, None)
    with pytest.raises(P.LrndeError) as ei:
        lc.join(extra, 1)
    assert ei.value.code == 4
    uid = (ctypes.c_uint8 * 128)()
    assert L.lib.lrnde_conv_comm_init(extra._ctx, uid, 2, 2) == 4
    assert L.lib.lrnde_conv_comm_init(extra._ctx, uid, -1, 2) == 4
    assert extra.comm_count() == (1, 0)
    # after LocalComm.close() the handles run unsharded and give the unsharded bits again
    lc.close()
    for h in hs:
        assert h.comm_count() == (1, 0)
        h.set_bn_state(BN0)
        n0 = h.comm_stats()[0]
        assert torch.equal(h.rhs(ud, 0.3), want)
        assert h.comm_stats()[0] == n0
