"""The batch-sharded conv handle off the shapes tests/test_gpu_conv_sharded.py runs it at: partial lists
long enough for a second trip of the rank-sum loops, test-mode BatchNorm through every entry point, the backward pass at
more than one image and more than one strip per rank and on bf16 / f32_split handles, solves that stop with a retcode,
the same-B check through every first exchange, eight ranks, and the exchange counts of whole calls.

Same set-up as that file: R `ConvHandle`s of this process on their own streams and host threads, joined by the local
communicator, rank r owning images [r*B, (r+1)*B); the same two yardsticks, neither the code under test:
  (U) one unsharded handle of the same library on the global batch,
  (O) oracle.ConvField on the global batch.
Every bar against (O) is one tests/test_gpu_conv.py or tests/test_gpu_conv_sharded.py already holds the same quantity
to, cited where it is used.  Distances to (U) are printed (DESIGN.md §5 records them) and are no bars except where a test
says "bits".  The solve cases and what selects them are in tests/conv_sharded_cases.py; tests/test_host_conv_sharded.py
asserts the selection conditions (step counts, the margin of every EEst from the accept threshold, the retcodes, the
lengths of the partial lists) on the oracle alone."""
import functools
import time

import numpy as np
import pytest
import torch

import conv_sharded_cases as S
from conv_sharded_cases import (BLOCKS, BN0, MODES, _dist, _field, _handle, _inputs, _mods, _ranks, _rel, _run,
                                _shards)

pytestmark = pytest.mark.gpu

TS = (0.0, 0.613)
T_VJP = 0.41


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _counted(hs, fns):
    """runs one callable per rank; -> (results, exchanges each rank issued meanwhile)"""
    before = [h.comm_stats()[0] for h in hs]
    out = _run(fns)
    return out, [h.comm_stats()[0] - b for h, b in zip(hs, before)]


def _same_stats(a, b):
    """two lrnde_stats dicts hold the same values (a NaN equals a NaN: a solve stopped by a NaN estimate reports one)"""
    return a.keys() == b.keys() and all(np.array_equal(np.float64(a[k]), np.float64(b[k]), equal_nan=True) for k in a)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _gp_blocks(gp, gp_ref, bar=5e-5):
    """every block of gp (w1, bn1, w2, bn2, w3) within `bar` of that block's scale (test_conv_vjp_matches_oracle); a
    BatchNorm block summed twice, or a weight block not summed, misses it by a factor"""
    gp = np.asarray(gp)
    worst = {}
    for name, sl in BLOCKS:
        sc = np.abs(gp_ref[sl]).max()
        worst[name] = float(np.abs(gp[sl] - gp_ref[sl]).max() / sc)
    for name, e in worst.items():
        assert e <= bar, f"{name}: {e:.3e} of its scale (all blocks: {worst})"
    return worst


# ---- A. long partial lists -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_refs():
    """the 2 x 260 @ 8x8 case: inputs, (U) at both times with its running statistics after the first f-eval, and (O)'s
    f-evals and VJP — computed once, shared by the tests of this section"""
    P, O = _mods()
    R, Bl, W, H = S.LONG_LIST
    B = R * Bl
    p, u, st = _inputs(W, H, B, W + B, True)
    hu = _handle(W, H, p, None)
    ud = _dev(u)
    U, bn1 = [], None
    for t in TS:
        U.append(hu.rhs(ud, t).cpu().numpy())
        if bn1 is None:
            bn1 = hu.get_bn_state().cpu().numpy()
    fld = _field(W, H, p, None)
    Oo = [fld.rhs(u.reshape(B, -1), t).reshape(u.shape) for t in TS]
    lam = S.cotangent(u.shape, 17)
    dy_ref, gp_ref = O.conv_vjp(_field(W, H, p, None), u.reshape(B, -1), T_VJP, lam.reshape(B, -1))
    return dict(p=p, u=u, U=U, bn1=bn1, O=Oo, lam=lam, dy=dy_ref.reshape(u.shape), gp=gp_ref)


def test_long_lists_rhs_gather_form_gives_the_unsharded_bits():
    """260 workgroups per rank: the gather form's 520 columns are the unsharded run's, in its order"""
    R, Bl, W, H = S.LONG_LIST
    ref = _long_refs()
    lc, hs = _ranks(R, W, H, ref["p"], None, gather=True)
    us = _shards(ref["u"], R)
    for i, t in enumerate(TS):
        got = _run([(lambda r=r: hs[r].rhs(us[r], t)) for r in range(R)])
        assert torch.equal(torch.cat(got).cpu(), torch.from_numpy(ref["U"][i])), f"t={t}"
    lc.close()


def test_long_lists_rhs_default_form_matches_unsharded_and_oracle():
    """k_bn_rank_sums' strided loop takes a second trip (260 partials per channel, 256 threads): <= 1e-5 of scale against
    (U) and (O) (test_conv_rhs_matches_oracle's RTOL); running statistics after one f-eval at rtol 2e-5, atol 1e-6 of (U)'s
    (test_conv_running_statistics_match_oracle) and the same bits on both ranks"""
    R, Bl, W, H = S.LONG_LIST
    ref = _long_refs()
    lc, hs = _ranks(R, W, H, ref["p"], None)
    us = _shards(ref["u"], R)
    for i, t in enumerate(TS):
        got = torch.cat(_run([(lambda r=r: hs[r].rhs(us[r], t)) for r in range(R)]))
        du, do = _dist(got, ref["U"][i]), _dist(got, ref["O"][i])
        print(f"long lists rhs default form 2x260@8x8 t={t}: vs U {du:.3e} (zero: {du == 0.0}), vs O {do:.3e}")
        assert du <= 1e-5 and do <= 1e-5
        if i == 0:
            bn = [h.get_bn_state() for h in hs]
            assert torch.equal(bn[0], bn[1])
            np.testing.assert_allclose(bn[0].cpu().numpy(), ref["bn1"], rtol=2e-5, atol=1e-6)
            assert not np.array_equal(bn[0].cpu().numpy(), BN0)
            print(f"long lists running statistics vs U: max rel {np.abs(bn[0].cpu().numpy() / ref['bn1'] - 1)[ref['bn1'] != 0].max():.3e}")
    lc.close()


def test_long_lists_vjp_matches_oracle():
    """dy and every block of gp within 5e-5 of its scale against (O) (test_conv_vjp_matches_oracle) with 260 workgroups
    per rank in the recompute's statistics and 260 strips per rank in the weight gradients; gp replicated bit for bit"""
    R, Bl, W, H = S.LONG_LIST
    ref = _long_refs()
    lc, hs = _ranks(R, W, H, ref["p"], None)
    us, ls = _shards(ref["u"], R), _shards(ref["lam"], R)
    got = _run([(lambda r=r: hs[r].vjp(us[r], T_VJP, ls[r])) for r in range(R)])
    d = _dist(torch.cat([g[0] for g in got]), ref["dy"])
    assert torch.equal(got[0][1], got[1][1]), "gp must come out replicated"
    worst = _gp_blocks(got[0][1].cpu().numpy(), ref["gp"])
    print(f"long lists vjp 2x260@8x8 vs O: dy {d:.3e}, gp blocks {worst}")
    assert d <= 5e-5
    lc.close()


def test_long_lists_one_forced_rccl_rank_gives_the_unsharded_bits(monkeypatch):
    """one forced RCCL rank at B = 260 @ 8x8: k_bn_rank_sums over 260 partials, then k_bn_finalize_t over the one slot,
    must add in k_bn_finalize_t's own order over 260 — the one-rank "bit-identical" claim past 256 partials.  rhs,
    init_dt, perform_step and vjp equal the unsharded handle bit for bit"""
    P, O = _mods()
    W = H = 8; B = 260
    p, u, st = _inputs(W, H, B, 61, True, 3.0)
    monkeypatch.setenv("LRNDE_FORCE_COMM", "1")
    monkeypatch.delenv("LRNDE_GATHER_TILES", raising=False)
    hu, hf = _handle(W, H, p, None), _handle(W, H, p, None)
    P.init_comm(hf, 0, 1)
    assert hu.comm_count() == (1, 0) and hf.comm_count() == (1, 1)
    ud = _dev(u)
    lam = _dev(S.cotangent(u.shape, 3))
    tol = 1e-3

    def battery(h):
        out = {}
        h.set_bn_state(BN0)
        out["rhs"] = h.rhs(ud, 0.3)
        out["dt"], out["k1"] = h.init_dt(ud, 0.0, 1.0, tol, tol)
        out["step"] = h.perform_step(ud, out["k1"], 0.0, 0.2, tol, tol)
        out["vjp"] = h.vjp(ud, T_VJP, lam)
        out["bn"] = h.get_bn_state()
        return out

    a, b = battery(hu), battery(hf)
    assert hf.comm_stats()[0] == 2 + 6 + 13 + 7 and hu.comm_stats() == (0, 0)
    assert torch.equal(a["rhs"], b["rhs"]) and a["dt"] == b["dt"] and torch.equal(a["k1"], b["k1"])
    for k in ("u", "k7"):
        assert torch.equal(a["step"][k], b["step"][k]), k
    for k in ("eest", "reg_error", "reg_stiff"):
        assert a["step"][k] == b["step"][k], k
    assert torch.equal(a["vjp"][0], b["vjp"][0]) and torch.equal(a["vjp"][1], b["vjp"][1])
    assert torch.equal(a["bn"], b["bn"])
    hf.close()


def _stem_inputs(B, W, H, train):
    """test_cifar_stem_matches_oracle's recipe"""
    rng = np.random.default_rng(W + B)
    x = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    ps = (rng.standard_normal(156) * 0.3).astype(np.float32); ps[140:148] = rng.uniform(0.5, 1.5, 8)
    st = None if train else np.concatenate([rng.normal(0, 0.2, 8), rng.uniform(0.5, 2, 8)]).astype(np.float32)
    g = rng.standard_normal((B, 8, H, W)).astype(np.float32)
    return rng, x, ps, st, g


@pytest.mark.parametrize("train", [True, False], ids=["train", "test"])
@pytest.mark.parametrize("shape", list(S.STEM_SHAPES))
def test_stem_and_head_on_several_blocks_per_rank(shape, train):
    """k_blk_rank_sums (stem forward) and k_blk_rank_sums_seq (stem backward) over two blocks per rank — the second ragged
    at 12x8, full at 16x16 — and over 260 at 32x32, and the head's per-rank loss and dph sums at the same shapes, against
    O.cifar_stem_* / O.cifar_head_ce on the global batch: test_cifar_stem_matches_oracle's bars (1e-5 forward and state,
    5e-5 backward) and test_cifar_head_matches_oracle's (loss 2e-5, logits 2e-5, du 5e-5, dph 5e-5).  In test mode the
    stem's forward exchanges nothing; its backward still exchanges d scale / d bias and the weight block"""
    P, O = _mods()
    R, Bl, W, H = S.STEM_SHAPES[shape]
    B, K = R * Bl, 10
    rng, x, ps, st, g = _stem_inputs(B, W, H, train)
    p, _, _ = _inputs(8, 8, 1, 1)
    lc, hs = _ranks(R, W, H, p, None, train=train)
    xs, gs = _shards(x, R), _shards(g, R)
    pd = _dev(ps)
    std = None if st is None else _dev(st)
    u_o, st_o = O.cifar_stem_forward(x, ps, bn_train=train, bn_state=st, return_state=True)
    got, n = _counted(hs, [(lambda r=r: hs[r].cifar_stem_forward(xs[r], pd, std, return_state=True)) for r in range(R)])
    assert n == [1 if train else 0] * R, n
    d = _dist(torch.cat([q[0] for q in got]), u_o)
    assert d <= 1e-5
    for q in got:
        assert torch.equal(q[1], got[0][1])
        np.testing.assert_allclose(q[1].cpu().numpy(), st_o, rtol=1e-5, atol=1e-6)
        if not train:
            assert np.array_equal(q[1].cpu().numpy(), st)
    ref = O.cifar_stem_backward(x, ps, g, bn_train=train, bn_state=st)
    gb, n = _counted(hs, [(lambda r=r: hs[r].cifar_stem_backward(xs[r], pd, gs[r], std)) for r in range(R)])
    assert n == [3 if train else 2] * R, n
    for q in gb:
        assert torch.equal(q, gb[0])
    db = float(np.abs(gb[0].cpu().numpy() - ref).max() / np.abs(ref).max())
    # (U), reported: the same two calls on one unsharded handle over the global batch
    hu = _handle(W, H, p, None, train=train)
    uu = hu.cifar_stem_forward(_dev(x), pd, std)
    bu = hu.cifar_stem_backward(_dev(x), pd, _dev(g), std)
    print(f"stem {shape} {'train' if train else 'test'}: forward vs O {d:.3e}, vs U {_dist(torch.cat([q[0] for q in got]), uu.cpu().numpy()):.3e}; "
          f"backward vs O {db:.3e}, vs U {_dist(gb[0], bu.cpu().numpy()):.3e}")
    assert db <= 5e-5
    if shape == "2x65@32x32":   # the stem alone at 260 blocks per rank
        lc.close()
        return
    u = rng.standard_normal((B, 8, H, W)).astype(np.float32)
    ph = (rng.standard_normal(73 + K * H * W + K) * 0.1).astype(np.float32)
    lab = rng.integers(0, K, B).astype(np.int32)
    lo, lg, du, dph = O.cifar_head_ce(u, ph, K, lab)
    uh = _shards(u, R)
    labs = [_dev(lab[r * Bl:(r + 1) * Bl].copy()) for r in range(R)]
    phd = _dev(ph)
    hr, n = _counted(hs, [(lambda r=r: hs[r].cifar_head_ce(uh[r], phd, K, labs[r])) for r in range(R)])
    assert n == [2] * R, n
    for q in hr:
        assert q["loss"] == hr[0]["loss"] and torch.equal(q["dph"], hr[0]["dph"])
        assert abs(float(q["loss"]) - float(lo)) <= 2e-5 * max(1.0, abs(float(lo)))
    hd = hu.cifar_head_ce(_dev(u), phd, K, _dev(lab))
    dl, ddu = _dist(torch.cat([q["logits"] for q in hr]), lg), _dist(torch.cat([q["du"] for q in hr]), du)
    dd = float(np.abs(hr[0]["dph"].cpu().numpy() - dph).max() / np.abs(dph).max())
    print(f"head {shape}: loss {float(hr[0]['loss']):.9g} (O {float(lo):.9g}, U {float(hd['loss']):.9g}); vs O logits {dl:.3e} du {ddu:.3e} "
          f"dph {dd:.3e}; vs U du {_dist(torch.cat([q['du'] for q in hr]), hd['du'].cpu().numpy()):.3e} dph {_dist(hr[0]['dph'], hd['dph'].cpu().numpy()):.3e}")
    assert dl <= 2e-5 and ddu <= 5e-5 and dd <= 5e-5
    lc.close()


# ---- B. test-mode BatchNorm on shards --------------------------------------------------------------------------------
def test_test_mode_solve_and_node_forward():
    """test_sharded_solve_and_node_forward's assertions with bn_train = False on random running statistics: stats equal on
    both ranks and equal to (U)'s; (naccept, nreject, nf) equal (O)'s; saved states within 2e-5 of scale of (O)
    (test_conv_solve_matches_oracle_step_for_step) and of (U); reg_val equal on both ranks and within 1e-1 relative of (O)
    (test_conv_node_forward_matches_oracle).  The running statistics stay the bits that were set, and every call issued
    the exchanges its stats imply (no f-eval exchanges anything in test mode: one per norm)"""
    case = S.TEST_MODE_CASE
    R, Bl, W, H, seed, scale, tol, train = case
    B = R * Bl
    p, u, st = _inputs(W, H, B, seed, train, scale)
    ro = S.oracle_solve(case)
    assert not S.at_threshold(ro["trace"]), "the oracle's own trace has an attempt at the accept threshold"
    hu = _handle(W, H, p, st, train=False)
    ud = _dev(u)
    ru = hu.solve(ud, 0.0, 1.0, tol, tol, saveat=list(S.SAVEAT), trace=True)
    lc, hs = _ranks(R, W, H, p, st, train=False)
    us = _shards(u, R)
    got, n = _counted(hs, [(lambda r=r: hs[r].solve(us[r], 0.0, 1.0, tol, tol, saveat=list(S.SAVEAT), trace=True)) for r in range(R)])
    so = ro["stats"]
    for g in got:
        assert g["stats"] == got[0]["stats"] and g["stats"] == ru["stats"]
        assert (g["stats"]["naccept"], g["stats"]["nreject"], g["stats"]["nf"]) == (so["naccept"], so["nreject"], so["nf"])
        for f in ("t", "dt", "eest", "accepted"):
            assert np.array_equal(g["trace"][f], got[0]["trace"][f]), f
        assert list(g["t"]) == [np.float32(S.SAVEAT[0]), np.float32(S.SAVEAT[1])]
    assert so["naccept"] >= 3
    assert n == [S.exchanges_node_forward(got[0]["stats"], "none", False)] * R, n
    for i in range(2):
        ui = torch.cat([g["u"][i] for g in got])
        du, do = _dist(ui, ru["u"][i].cpu().numpy()), _dist(ui, ro["u"][i])
        print(f"test-mode solve 2x2@8x8 save {i}: vs U {du:.3e} (zero: {du == 0.0}), vs O {do:.3e}")
        assert du <= 2e-5 and do <= 2e-5
    for m, rt in MODES:
        o_ = S.oracle_node_forward(case, m, rt)
        u_ = hu.node_forward(ud, 0.0, 1.0, tol, tol, mode=m, reg_type=rt, t1_or_rand=S.T1)
        gf, n = _counted(hs, [(lambda r=r: hs[r].node_forward(us[r], 0.0, 1.0, tol, tol, mode=m, reg_type=rt, t1_or_rand=S.T1))
                              for r in range(R)])
        assert n == [S.exchanges_node_forward(gf[0]["stats"], m, False)] * R, (m, n)
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
        print(f"test-mode node_forward {m}: u_end vs U {du:.3e} (zero: {du == 0.0}), vs O {do:.3e}; reg_val {gf[0]['reg_val']} "
              f"U {u_['reg_val']} O {o_['reg_val']}")
        assert du <= 2e-5 and do <= 2e-5
    for h in hs + [hu]:
        assert np.array_equal(h.get_bn_state().cpu().numpy(), st), "test mode must not touch the running statistics"
    lc.close()


def _backward_case(case, mode, w_reg, tag):
    """test_sharded_node_backward_matches_oracle's assertions at `case` (test_conv_node_backward_matches_oracle's bars):
    forward naccept equal to (O)'s, adjoint naccept equal on all ranks and within 1 of (O), dx 2e-3 and dp 5e-3 in the
    relative norm, dp replicated, and the recorded pair gives the one-call form's bits on every rank.  Also: the call
    issued the exchanges its own stats imply (S.exchanges_node_backward: 43 / 31 per adjoint attempt plus its start)"""
    R, Bl, W, H, seed, scale, tol, train = case
    B = R * Bl
    p, u, st = _inputs(W, H, B, seed, train, scale)
    wv = S.cotangent(u.shape)
    bo = S.oracle_node_backward(case, mode, w_reg)
    assert bo["retcode"] == 0
    kw = dict(mode=mode, t1_or_rand=S.T1, maxiters=5000)
    hu = _handle(W, H, p, st, train=train)
    bu = hu.node_backward(_dev(u), 0.0, 1.0, tol, tol, _dev(wv), w_reg=w_reg, **kw)
    lc, hs = _ranks(R, W, H, p, st, train=train)
    us, ws = _shards(u, R), _shards(wv, R)
    got, n = _counted(hs, [(lambda r=r: hs[r].node_backward(us[r], 0.0, 1.0, tol, tol, ws[r], w_reg=w_reg, **kw)) for r in range(R)])
    assert n == [S.exchanges_node_backward(got[0]["stats_fwd"], got[0]["stats_bwd"], mode, w_reg, train)] * R, n
    dx = torch.cat([g["dx"] for g in got])
    edx, edp = _rel(dx.cpu().numpy().reshape(B, -1), bo["dx"]), _rel(got[0]["dp"], bo["dp"])
    print(f"node_backward {tag} {mode}: vs U dx {_rel(dx, bu['dx']):.3e} dp {_rel(got[0]['dp'], bu['dp']):.3e}; vs O dx {edx:.3e} dp {edp:.3e}; "
          f"steps fwd {got[0]['stats_fwd']['naccept']}/{got[0]['stats_fwd']['nreject']} bwd {got[0]['stats_bwd']['naccept']}/"
          f"{got[0]['stats_bwd']['nreject']} (O {S.step_counts(bo)}, U bwd {bu['stats_bwd']['naccept']}/{bu['stats_bwd']['nreject']}); "
          f"{n[0]} exchanges")
    for g in got:
        assert g["stats_fwd"]["naccept"] == bo["stats_fwd"]["naccept"]
        assert g["stats_bwd"] == got[0]["stats_bwd"]
        assert abs(g["stats_bwd"]["naccept"] - bo["stats_bwd"]["naccept"]) <= 1
        assert torch.equal(g["dp"], got[0]["dp"]), "dp must come out replicated"
        assert _rel(g["dp"], bo["dp"]) <= 5e-3
    assert edx <= 2e-3
    for h in hs:
        h.set_bn_state(BN0 if train else st)

    def pair(r):
        fw = hs[r].node_forward_record(us[r], 0.0, 1.0, tol, tol, **kw)
        return fw, hs[r].node_backward_recorded(Bl, ws[r], w_reg=w_reg)

    two = _run([(lambda r=r: pair(r)) for r in range(R)])
    for r in range(R):
        assert torch.equal(two[r][1]["dx"], got[r]["dx"]) and torch.equal(two[r][1]["dp"], got[r]["dp"])
        assert two[r][1]["stats_bwd"] == got[r]["stats_bwd"] and two[r][0]["stats"] == got[r]["stats_fwd"]
    if not train:
        for h in hs:
            assert np.array_equal(h.get_bn_state().cpu().numpy(), st), "test mode must not touch the running statistics"
    lc.close()


def test_test_mode_node_backward_matches_oracle():
    """31 exchanges per adjoint attempt instead of 43: the BatchNorm-backward exchange only carries d scale / d bias"""
    _backward_case(S.TEST_MODE_CASE, "unbiased", S.W_REG, "test-mode 2x2@8x8")


def _step_reg_grad_case(R, Bl, W, H, train, reg_type, tag):
    """the bars of test_conv_step_reg_grad_matches_oracle: reg_val 5e-3 relative, gradient 1e-2 of its scale and norm; value
    and gradient the same bits on every rank"""
    P, O = _mods()
    B = R * Bl
    p, u, st = _inputs(W, H, B, 31, train, 2.0)
    fld = _field(W, H, p, st, train=train)
    k1 = fld.rhs(u.reshape(B, -1), 0.2)
    dt = 0.25
    g_ref, rv_ref = O.step_reg_grad(_field(W, H, p, st, train=train), u.reshape(B, -1), k1, 0.2, dt, 1e-4, 1e-4, reg_type=reg_type)
    hu = _handle(W, H, p, st, train=train)
    g_u, rv_u = hu.step_reg_grad(_dev(u), _dev(k1.reshape(u.shape)), 0.2, dt, 1e-4, 1e-4, reg_type=reg_type)
    lc, hs = _ranks(R, W, H, p, st, train=train)
    us, ks = _shards(u, R), _shards(k1.reshape(u.shape), R)
    got, n = _counted(hs, [(lambda r=r: hs[r].step_reg_grad(us[r], ks[r], 0.2, dt, 1e-4, 1e-4, reg_type=reg_type)) for r in range(R)])
    assert n == [S.exchanges_step(train) + 6 * S.exchanges_vjp_gp(train)] * R, n
    g = got[0][0].cpu().numpy()
    print(f"step_reg_grad {tag} {reg_type}: reg_val {got[0][1]} (O {rv_ref}, U {rv_u}); gradient vs O {_rel(g, g_ref):.3e}, vs U {_rel(g, g_u):.3e}")
    for gg, rv in got:
        assert rv == got[0][1] and torch.equal(gg, got[0][0])
        assert abs(float(rv) - float(rv_ref)) <= 5e-3 * abs(float(rv_ref))
    assert np.abs(g - g_ref).max() <= 1e-2 * np.abs(g_ref).max()
    assert _rel(g, g_ref) <= 1e-2
    if not train:
        for h in hs:
            assert np.array_equal(h.get_bn_state().cpu().numpy(), st)
    lc.close()


@pytest.mark.parametrize("reg_type", ["error_estimate", "stiffness_estimate"])
def test_test_mode_step_reg_grad_matches_oracle(reg_type):
    _step_reg_grad_case(2, 2, 8, 8, False, reg_type, "test-mode 2x2@8x8")


# ---- C. the backward pass off the 8x8 one-image case ------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.BACKWARD_CASES))
def test_node_backward_at_more_images_and_strips_per_rank(name):
    """2 x 2 @ 16x16: two strips per image, so every rank's weight gradient adds four strips before the all-reduce;
    2 x 3 @ 12x8: three images per rank through the MT = 6 kernels"""
    case, expect = S.BACKWARD_CASES[name]
    assert not S.at_threshold(S.oracle_solve(case)["trace"]), "the oracle's own trace has an attempt at the accept threshold"
    _backward_case(case, "unbiased", S.W_REG, name)


@pytest.mark.parametrize("reg_type", ["error_estimate", "stiffness_estimate"])
def test_step_reg_grad_at_two_strips_per_image(reg_type):
    _step_reg_grad_case(2, 2, 16, 16, True, reg_type, "2x2@16x16")


@pytest.mark.parametrize("dtype", ["bf16", "f32_split"])
def test_rhs_default_form_other_dtypes(dtype):
    """two ranks of bf16 / f32_split handles in the default (pre-reduced) form, 2 x 3 @ 12x8, at the dtype's own bar against
    (O): f32_split 1e-5 of scale against the fp32 oracle (test_conv_f32_split_rhs_meets_the_fp32_bar), bf16 5e-3 against the
    oracle's bf16 emulation (test_conv_bf16_rhs)"""
    R, Bl, W, H = 2, 3, 12, 8
    B = R * Bl
    p, u, st = _inputs(W, H, B, W + 7, True)
    fld = _field(W, H, p, None, bf16=(dtype == "bf16"))
    hu = _handle(W, H, p, None, dtype=dtype)
    lc, hs = _ranks(R, W, H, p, None, dtype=dtype)
    us = _shards(u, R)
    for t in TS:
        got = torch.cat(_run([(lambda r=r: hs[r].rhs(us[r], t)) for r in range(R)]))
        want_u = hu.rhs(_dev(u), t)
        do, du = _dist(got, fld.rhs(u.reshape(B, -1), t)), _dist(got, want_u.cpu().numpy())
        print(f"rhs default form {dtype} 2x3@12x8 t={t}: vs U {du:.3e} (zero: {du == 0.0}), vs O {do:.3e}")
        assert do <= (5e-3 if dtype == "bf16" else 1e-5)
    bn = [h.get_bn_state() for h in hs]
    assert torch.equal(bn[0], bn[1])
    lc.close()


def test_bf16_ranks_backward_is_the_fp32_adjoint():
    """test_conv_bf16_handle_backward_is_the_fp32_adjoint on two ranks of two images: the VJP of bf16 ranks IS the fp32
    ranks' VJP (same kernels, same packs, the same exchanges) even with bf16 activations left in the workspace; a bf16
    f-eval still runs the bf16 kernels afterwards (3e-2 of scale against the fp32 oracle, and not the fp32 ranks' bits);
    node_backward differs from the fp32 ranks' only through the bf16 forward trajectory (5e-2 in the relative norm at
    tol 1e-2); dp replicated"""
    R, Bl, W, H = 2, 2, 8, 8
    B = R * Bl
    p, u, st = _inputs(W, H, B, 43, True, 1.5)
    fld = _field(W, H, p, None)
    lc32, h32 = _ranks(R, W, H, p, None)
    lcb, hb = _ranks(R, W, H, p, None, dtype="bf16")
    us = _shards(u, R)
    ls = _shards(S.cotangent(u.shape, 4), R)
    v32 = _run([(lambda r=r: h32[r].vjp(us[r], 0.3, ls[r])) for r in range(R)])
    _run([(lambda r=r: hb[r].rhs(us[r], 0.3)) for r in range(R)])   # leaves bf16 activations in the workspace
    vb = _run([(lambda r=r: hb[r].vjp(us[r], 0.3, ls[r])) for r in range(R)])
    for r in range(R):
        assert torch.equal(vb[r][0], v32[r][0]) and torch.equal(vb[r][1], v32[r][1])
        assert torch.equal(vb[r][1], vb[0][1])
    fb = torch.cat(_run([(lambda r=r: hb[r].rhs(us[r], 0.3)) for r in range(R)]))
    f32 = torch.cat(_run([(lambda r=r: h32[r].rhs(us[r], 0.3)) for r in range(R)]))
    assert _dist(fb, fld.rhs(u.reshape(B, -1), 0.3)) <= 3e-2 and not torch.equal(fb, f32)
    ws = _shards(S.cotangent(u.shape, 5), R)
    tol = 1e-2  # above the bf16 field's rounding noise, so both solves take comparable steps
    kw = dict(mode="unbiased", t1_or_rand=S.T1, w_reg=S.W_REG, maxiters=5000)
    b32 = _run([(lambda r=r: h32[r].node_backward(us[r], 0.0, 1.0, tol, tol, ws[r], **kw)) for r in range(R)])
    bb = _run([(lambda r=r: hb[r].node_backward(us[r], 0.0, 1.0, tol, tol, ws[r], **kw)) for r in range(R)])
    assert torch.equal(bb[0]["dp"], bb[1]["dp"]) and bb[0]["stats_bwd"] == bb[1]["stats_bwd"]
    ddx = _rel(torch.cat([b["dx"] for b in bb]), torch.cat([b["dx"] for b in b32]))
    ddp = _rel(bb[0]["dp"], b32[0]["dp"])
    print(f"bf16 ranks node_backward vs fp32 ranks: dx {ddx:.3e} dp {ddp:.3e}")
    assert ddx <= 5e-2 and ddp <= 5e-2
    lc32.close(); lcb.close()


def test_f32_split_ranks_backward_matches_oracle():
    """two ranks of f32_split handles through the VJP with gp (fp32 transposed convs on the split forward's activations):
    test_conv_f32_split_solve_and_backward's bars, dy 5e-5 of scale and gp 5e-5 in the relative norm against (O); gp
    replicated"""
    P, O = _mods()
    R, Bl, W, H = 2, 2, 16, 16
    B = R * Bl
    p, u, st = _inputs(W, H, B, 5, True, 1.5)
    lam = S.cotangent(u.shape, 17)
    dy_ref, gp_ref = O.conv_vjp(_field(W, H, p, None), u.reshape(B, -1), T_VJP, lam.reshape(B, -1))
    lc, hs = _ranks(R, W, H, p, None, dtype="f32_split")
    us, ls = _shards(u, R), _shards(lam, R)
    got = _run([(lambda r=r: hs[r].vjp(us[r], T_VJP, ls[r])) for r in range(R)])
    assert torch.equal(got[0][1], got[1][1])
    d, dg = _dist(torch.cat([g[0] for g in got]), dy_ref), _rel(got[0][1], gp_ref)
    print(f"f32_split ranks vjp 2x2@16x16 vs O: dy {d:.3e} gp {dg:.3e}")
    assert d <= 5e-5 and dg <= 5e-5
    lc.close()


# ---- D. stop codes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["nan", "maxiters"])
def test_sharded_solve_stops_alike_on_every_rank(kind):
    """DESIGN.md §5's deadlock rule: a NaN estimate and maxiters are decided from exchanged values, so both ranks return the
    same retcode from the same iteration and nobody is left in the local communicator's 60-second rendezvous.  "nan": test
    mode, the NaN pixel is in rank 1's last image, rank 0's own data and f-evals are finite and only the exchanged norm is
    NaN (retcode 3 after one iteration).  "maxiters": training mode, maxiters 3 (retcode 1 at the fourth header)"""
    P, O = _mods()
    R, Bl, W, H, seed, scale, tol = S.STOP_CASE
    p, u, st, train, maxiters = S.stop_inputs(kind)
    o = S.oracle_stop(kind)
    code = o["solve"]["retcode"]
    assert code == (3 if kind == "nan" else 1)
    kw = dict(saveat=[1.0], maxiters=maxiters, raise_on_retcode=False)
    hu = _handle(W, H, p, st, train=train)
    ru = hu.solve(_dev(u), 0.0, 1.0, tol, tol, **kw)
    so, su = o["solve"]["stats"], ru["stats"]
    print(f"stop code {kind}: O retcode {code} stats {so}; U retcode {ru['retcode']} stats {su}")
    assert ru["retcode"] == code and su["retcode"] == code
    assert (su["naccept"], su["nreject"], su["iters"]) == (so["naccept"], so["nreject"], so["iters"])
    lc, hs = _ranks(R, W, H, p, st, train=train)
    us = _shards(u, R)
    assert bool(torch.isfinite(us[0]).all()), "rank 0's own data is finite in both cases"
    before = _run([(lambda r=r: hs[r].rhs(us[r], 0.3)) for r in range(R)])
    tic = time.perf_counter()
    got = _run([(lambda r=r: hs[r].solve(us[r], 0.0, 1.0, tol, tol, **kw)) for r in range(R)])
    took = time.perf_counter() - tic
    assert took < 10.0, f"{took:.1f} s: a rank sat in the rendezvous"
    for g in got:
        assert g["retcode"] == code
        assert _same_stats(g["stats"], su), (g["stats"], su)

    errs = [None] * R

    def fwd(r):
        try:
            hs[r].node_forward(us[r], 0.0, 1.0, tol, tol, mode="unbiased", t1_or_rand=S.T1, maxiters=maxiters)
        except P.LrndeError as e:
            errs[r] = e

    tic = time.perf_counter()
    _run([(lambda r=r: fwd(r)) for r in range(R)])
    took = time.perf_counter() - tic
    assert took < 10.0, f"{took:.1f} s: a rank sat in the rendezvous"
    assert all(e is not None and e.code == code for e in errs), errs
    assert o["fwd"]["retcode"] == code
    after = _run([(lambda r=r: hs[r].rhs(us[r], 0.3)) for r in range(R)])
    for a, b in zip(before, after):
        assert torch.equal(_bits(a), _bits(b)), "the handles stay usable and give the same f-eval"
    assert bool(torch.isfinite(after[0]).all())
    lc.close()


# ---- E. same B, everywhere -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["vjp", "init_dt", "stem", "head", "rhs_gather"])
def test_same_batch_check_rides_every_first_exchange(entry):
    """two ranks called with B = 2 and B = 3: both return BADARG naming "2, 3" at once — the check rides in the first
    exchange of the call, whose count does not depend on B (BatchNorm statistics of the VJP's recompute and of init_dt's
    first f-eval, the stem's BatchNorm(8) statistics, the head's loss slots); in the gather form, whose payload does depend
    on B, it is an exchange of its own of 2 R doubles that both ranks issue first — and the handles stay usable"""
    P, O = _mods()
    R, W, K = 2, 8, 10
    p, u, st = _inputs(W, W, 6, 81)
    lc, hs = _ranks(R, W, W, p, None, gather=(entry == "rhs_gather"))
    rng = np.random.default_rng(2)
    x3 = rng.standard_normal((6, 3, W, W)).astype(np.float32)
    ps = _dev((rng.standard_normal(156) * 0.3).astype(np.float32))
    ph = _dev((rng.standard_normal(73 + K * W * W + K) * 0.1).astype(np.float32))
    lab = rng.integers(0, K, 6).astype(np.int32)
    xs = [_dev(u[:2].copy()), _dev(u[2:5].copy())]
    x3s = [_dev(x3[:2].copy()), _dev(x3[2:5].copy())]
    labs = [_dev(lab[:2].copy()), _dev(lab[2:5].copy())]
    calls = {
        "vjp": lambda r: hs[r].vjp(xs[r], 0.3, xs[r]),
        "init_dt": lambda r: hs[r].init_dt(xs[r], 0.0, 1.0, 1e-3, 1e-3),
        "stem": lambda r: hs[r].cifar_stem_forward(x3s[r], ps, None),
        "head": lambda r: hs[r].cifar_head_ce(xs[r], ph, K, labs[r]),
        "rhs_gather": lambda r: hs[r].rhs(xs[r], 0.3),
    }
    errs = [None, None]

    def call(r):
        try:
            calls[entry](r)
        except P.LrndeError as e:
            errs[r] = e

    tic = time.perf_counter()
    _, n = _counted(hs, [lambda: call(0), lambda: call(1)])
    took = time.perf_counter() - tic
    assert took < 10.0, f"{took:.1f} s: a rank sat in the rendezvous"
    assert all(e is not None and e.code == 4 for e in errs), errs
    assert "2, 3" in str(errs[0]) and "2, 3" in str(errs[1])
    assert n == [1, 1], f"the refusal follows the call's first exchange: {n}"
    # usable afterwards: the f-eval of the first four images against the unsharded handle
    want = _handle(W, W, p, None).rhs(_dev(u[:4]), 0.3)
    us = _shards(u[:4], R)
    got = torch.cat(_run([(lambda r=r: hs[r].rhs(us[r], 0.3)) for r in range(R)]))
    if entry == "rhs_gather":
        assert torch.equal(got, want)
    else:
        assert _dist(got, want.cpu().numpy()) <= 1e-5
    lc.close()


# ---- F. eight ranks --------------------------------------------------------------------------------------------------
def test_eight_ranks():
    """8 x 1 @ 8x8, the target rank count: rhs in the gather form gives (U)'s bits and in the default form <= 1e-5 of scale
    of (U) and (O); vjp with gp at 5e-5 per block, gp replicated; init_dt and one Tsit5 step at the bars of
    test_conv_init_dt_and_step_match_oracle (dt 1e-4 relative, k1 and u 1e-5 and k7 5e-5 of scale, EEst and both
    regularisation values 5e-3 relative, all of them the same on every rank); the head at
    test_cifar_head_matches_oracle's bars; the per-call exchange counts of test_gpu_conv_sharded.EXCHANGES unchanged"""
    P, O = _mods()
    from test_gpu_conv_sharded import EXCHANGES
    R, Bl, W, H, seed, scale = S.EIGHT
    B, K = R * Bl, 10
    p, u, st = _inputs(W, H, B, seed, True, scale)
    hu = _handle(W, H, p, None)
    ud = _dev(u)
    U = hu.rhs(ud, 0.3)
    Oo = _field(W, H, p, None).rhs(u.reshape(B, -1), 0.3)
    us = _shards(u, R)
    lcg, hg = _ranks(R, W, H, p, None, gather=True)
    got = torch.cat(_run([(lambda r=r: hg[r].rhs(us[r], 0.3)) for r in range(R)]))
    assert torch.equal(got, U)
    lcg.close()
    lc, hs = _ranks(R, W, H, p, None)
    assert all(h.comm_count() == (R, 2) for h in hs)
    got, n = _counted(hs, [(lambda r=r: hs[r].rhs(us[r], 0.3)) for r in range(R)])
    got = torch.cat(got)
    du, do = _dist(got, U.cpu().numpy()), _dist(got, Oo)
    print(f"eight ranks rhs default form: vs U {du:.3e} (zero: {du == 0.0}), vs O {do:.3e}")
    assert du <= 1e-5 and do <= 1e-5 and n == [EXCHANGES[("rhs", True)]] * R
    bn = [h.get_bn_state() for h in hs]
    assert all(torch.equal(b, bn[0]) for b in bn)
    # vjp with gp
    lam = S.cotangent(u.shape, 17)
    dy_ref, gp_ref = O.conv_vjp(_field(W, H, p, None), u.reshape(B, -1), T_VJP, lam.reshape(B, -1))
    ls = _shards(lam, R)
    gv, n = _counted(hs, [(lambda r=r: hs[r].vjp(us[r], T_VJP, ls[r])) for r in range(R)])
    assert n == [EXCHANGES[("vjp_gp", True)]] * R
    assert all(torch.equal(g[1], gv[0][1]) for g in gv), "gp must come out replicated"
    d = _dist(torch.cat([g[0] for g in gv]), dy_ref)
    worst = _gp_blocks(gv[0][1].cpu().numpy(), gp_ref)
    dyu, gpu = hu.vjp(ud, T_VJP, _dev(lam))
    print(f"eight ranks vjp: dy vs O {d:.3e}, vs U {_dist(torch.cat([g[0] for g in gv]), dyu.cpu().numpy()):.3e}; gp blocks vs O {worst}, "
          f"gp vs U {_rel(gv[0][1], gpu):.3e}")
    assert d <= 5e-5
    _, n = _counted(hs, [(lambda r=r: hs[r].vjp(us[r], T_VJP, ls[r], want_gp=False)) for r in range(R)])
    assert n == [EXCHANGES[("vjp", True)]] * R
    # init_dt and one step
    dt_o, k1_o, so = S.eight_ranks_step_ref()
    assert float(so["eest"]) > 1e-2, "a step large enough that the embedded error is truncation error, not cancellation noise"
    t0, dt, tol = S.EIGHT_STEP
    gi, n = _counted(hs, [(lambda r=r: hs[r].init_dt(us[r], t0, 1.0, tol, tol)) for r in range(R)])
    assert n == [EXCHANGES[("init_dt", True)]] * R and all(g[0] == gi[0][0] for g in gi)
    dtu, k1u = hu.init_dt(ud, t0, 1.0, tol, tol)
    print(f"eight ranks init_dt {gi[0][0]} (U {dtu}, O {dt_o})")
    assert abs(float(gi[0][0]) - float(dt_o)) <= 1e-4 * float(dt_o)
    k1 = [g[1] for g in gi]
    assert _dist(torch.cat(k1), k1_o) <= 1e-5
    gs, n = _counted(hs, [(lambda r=r: hs[r].perform_step(us[r], k1[r], t0, dt, tol, tol)) for r in range(R)])
    assert n == [EXCHANGES[("perform_step", True)]] * R
    su = hu.perform_step(ud, k1u, t0, dt, tol, tol)
    for k, bar in (("u", 1e-5), ("k7", 5e-5)):
        a = torch.cat([g[k] for g in gs])
        print(f"eight ranks step {k}: vs U {_dist(a, su[k].cpu().numpy()):.3e}, vs O {_dist(a, so[k]):.3e}")
        assert _dist(a, so[k]) <= bar
    print(f"eight ranks step EEst {gs[0]['eest']} (U {su['eest']}, O {so['eest']})")
    for g in gs:
        for k in ("eest", "reg_error", "reg_stiff"):
            assert g[k] == gs[0][k], k
    for k in ("eest", "reg_error", "reg_stiff"):
        assert abs(float(gs[0][k]) - float(so[k])) <= 5e-3 * abs(float(so[k])) + 1e-12, k
    # head
    rng = np.random.default_rng(W)
    uh_ = rng.standard_normal((B, 8, H, W)).astype(np.float32)
    ph = (rng.standard_normal(73 + K * H * W + K) * 0.1).astype(np.float32)
    lab = rng.integers(0, K, B).astype(np.int32)
    lo, lg, du_o, dph = O.cifar_head_ce(uh_, ph, K, lab)
    uh = _shards(uh_, R)
    labs = [_dev(lab[r * Bl:(r + 1) * Bl].copy()) for r in range(R)]
    phd = _dev(ph)
    hr, n = _counted(hs, [(lambda r=r: hs[r].cifar_head_ce(uh[r], phd, K, labs[r])) for r in range(R)])
    assert n == [2] * R
    for q in hr:
        assert q["loss"] == hr[0]["loss"] and torch.equal(q["dph"], hr[0]["dph"])
    assert abs(float(hr[0]["loss"]) - float(lo)) <= 2e-5 * max(1.0, abs(float(lo)))
    dl, ddu = _dist(torch.cat([q["logits"] for q in hr]), lg), _dist(torch.cat([q["du"] for q in hr]), du_o)
    dd = float(np.abs(hr[0]["dph"].cpu().numpy() - dph).max() / np.abs(dph).max())
    print(f"eight ranks head: loss {float(hr[0]['loss']):.9g} (O {float(lo):.9g}); vs O logits {dl:.3e} du {ddu:.3e} dph {dd:.3e}")
    assert dl <= 2e-5 and ddu <= 5e-5 and dd <= 5e-5
    lc.close()


# ---- G. counts of whole calls ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", [True, False], ids=["train", "test"])
def test_exchange_counts_of_whole_calls(train):
    """from the stats a call returns, the exchanges it must have issued (S.exchanges_*: 2 per training-mode f-eval and 0 in
    test mode, 1 per norm, 43 / 31 per adjoint attempt plus the adjoint's start of two VJPs and two norms, and the
    regulariser's init_dt, step and six VJPs), asserted from comm_stats() for node_forward in all three modes and for
    node_backward with and without the regulariser, 2 x 2 @ 8x8"""
    R, Bl, W, H, seed, scale, tol, _ = S.TEST_MODE_CASE
    B = R * Bl
    p, u, st = _inputs(W, H, B, seed, train, scale)
    lc, hs = _ranks(R, W, H, p, st, train=train)
    us, ws = _shards(u, R), _shards(S.cotangent(u.shape), R)
    assert (S.exchanges_feval(train), S.exchanges_vjp_gp(train), 6 * S.exchanges_vjp_gp(train) + 1) == ((2, 7, 43) if train else (0, 5, 31))
    for m, rt in MODES:
        gf, n = _counted(hs, [(lambda r=r: hs[r].node_forward(us[r], 0.0, 1.0, tol, tol, mode=m, reg_type=rt, t1_or_rand=S.T1))
                              for r in range(R)])
        want = S.exchanges_node_forward(gf[0]["stats"], m, train)
        print(f"node_forward {m} {'train' if train else 'test'}: {gf[0]['stats']['naccept']}/{gf[0]['stats']['nreject']} steps, nfe {gf[0]['nfe']}, "
              f"{n[0]} exchanges")
        assert n == [want] * R, (m, n, want)
        assert gf[0]["stats"]["naccept"] >= 3
    for m, w_reg in (("unbiased", S.W_REG), ("none", 0.0), ("unbiased", 0.0)):
        gb, n = _counted(hs, [(lambda r=r: hs[r].node_backward(us[r], 0.0, 1.0, tol, tol, ws[r], mode=m, t1_or_rand=S.T1, w_reg=w_reg,
                                                               maxiters=5000)) for r in range(R)])
        want = S.exchanges_node_backward(gb[0]["stats_fwd"], gb[0]["stats_bwd"], m, w_reg, train)
        print(f"node_backward {m} w_reg {w_reg} {'train' if train else 'test'}: fwd {gb[0]['stats_fwd']['naccept']}/{gb[0]['stats_fwd']['nreject']}, "
              f"bwd {gb[0]['stats_bwd']['naccept']}/{gb[0]['stats_bwd']['nreject']}, {n[0]} exchanges")
        assert n == [want] * R, (m, w_reg, n, want)
        assert gb[0]["stats_bwd"]["naccept"] >= 3
    lc.close()
