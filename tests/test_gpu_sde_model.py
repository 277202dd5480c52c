"""The MNIST-SDE model on the device (experiments/src/construct.jl:202-210, BASELINE config 5): the downsample kernels, the head
on the SDE handle, the model's recorded forward and pullback (csrc/lrnde_sde_model.hpp) and `run_sde_training_step`.

Every float array is compared with the float64 torch run of tests/sde_model_cases.py under the suite's rule
(latent_cases.bound): max(1e-5, 4 x the distance of the float32 torch run from the float64 run) of the float64 norm; the
measured error is printed beside the bound.  Bit-for-bit claims are `torch.equal` / `==`."""
import numpy as np
import pytest
import torch

import head_cases as HC
import sde_model_cases as MC
from test_gpu_sde_layer import _check_forward

pytestmark = pytest.mark.gpu
f32 = np.float32
S = MC.S


def _handle(P, D, H):
    from localregneuralde_jl_amd.layers import _mlp_desc
    return P.SdeHandle(_mlp_desc(P.Chain(P.Dense(D, H, "tanh"), P.Dense(H, D))))


def _cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the downsample kernels alone ----
@pytest.mark.parametrize("Din,D,B", MC.DENSE_CASES)
def test_downsample_forward_and_backward(gpu_pkg, Din, D, B):
    c = MC.dense_ref(Din, D, B)
    h = _handle(gpu_pkg, D, 4)
    x, pd, du0 = _cu(c["x"]), _cu(c["pd"]), _cu(c["du0"])
    u0 = h.dense_forward(x, pd)
    bw = h.dense_backward(x, pd, du0, want_dx=True)
    got = dict(u0=u0.cpu().numpy(), dpd=bw["dpd"].cpu().numpy(), dx=bw["dx"].cpu().numpy())
    MC.check(f"Din={Din} D={D} B={B}", got, c["r64"], c["r32"], ["u0", "dpd", "dx"])
    nodx = h.dense_backward(x, pd, du0)                      # dx = NULL: the same parameter cotangent, nothing else written
    assert nodx["dx"] is None and torch.equal(nodx["dpd"], bw["dpd"])
    assert torch.equal(h.dense_forward(x, pd), u0)           # runs repeat bitwise
    again = h.dense_backward(x, pd, du0, want_dx=True)
    assert torch.equal(again["dpd"], bw["dpd"]) and torch.equal(again["dx"], bw["dx"])
    assert np.abs(c["pd"][D * Din:]).min() > 0               # (the biases of the case are non-zero)


@pytest.mark.parametrize("Din,D", [(784, 32), (513, 20), (50, 72)])
def test_a_samples_u0_is_the_same_bits_alone_and_inside_a_batch_of_33(gpu_pkg, Din, D):
    c = MC.dense_ref(Din, D, 33)
    h = _handle(gpu_pkg, D, 4)
    x, pd = _cu(c["x"]), _cu(c["pd"])
    u0 = h.dense_forward(x, pd)
    for b in (0, 15, 16, 32):                                 # ends of the first tile, start of the second, the third's only row
        one = h.dense_forward(x[b:b + 1].clone(), pd)
        assert torch.equal(one[0], u0[b]), (b, float((one[0] - u0[b]).abs().max()))


def test_dense_calls_refuse_bad_arguments(gpu_pkg):
    import ctypes as C
    from localregneuralde_jl_amd import _lib as L
    h = _handle(gpu_pkg, 8, 4)
    x, pd, u0 = torch.zeros(2, 5).cuda(), torch.zeros(8 * 6).cuda(), torch.zeros(2, 8).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.lib.lrnde_sde_dense_forward(h._h, p(x), 0, 5, p(pd), p(u0)) == 4
    assert L.lib.lrnde_sde_dense_forward(h._h, p(x), 2, 0, p(pd), p(u0)) == 4
    assert L.lib.lrnde_sde_dense_forward(h._h, None, 2, 5, p(pd), p(u0)) == 4
    assert L.lib.lrnde_sde_dense_backward(h._h, p(x), 2, 5, p(pd), None, p(pd), None) == 4
    assert L.lib.lrnde_sde_model_backward_recorded(h._h, 2, 0.0, p(pd), p(pd), p(pd), None) == 4     # no record
    assert b"record" in L.lib.lrnde_sde_last_error(h._h)
    assert L.lib.lrnde_sde_dense_forward(h._h, p(x), 2, 5, p(pd), p(u0)) == 0


# ---- the head ----
@pytest.mark.parametrize("D", [32, 72])
def test_head_on_the_sde_handle(gpu_pkg, D):
    K, B = 10, 9
    c = HC.mlp_ref(D, K, B)
    h = _handle(gpu_pkg, D, 4)
    u, pc, lab = _cu(c["u"]), _cu(c["pc"]), _cu(c["labels"])
    r = h.classifier_ce(u, pc, K, lab)
    got = dict(loss=float(r["loss"]), logits=r["logits"].cpu().numpy(), du=r["du"].cpu().numpy(), dpc=r["dpc"].cpu().numpy())
    HC.check(f"sde head D={D}", got, c, ["logits", "du", "dpc"])
    bad = c["labels"].copy(); bad[B // 2] = K
    with pytest.raises(gpu_pkg.LrndeError, match=r"label is outside"):
        h.classifier_ce(u, pc, K, _cu(bad))
    from localregneuralde_jl_amd import _lib as L
    import ctypes as C
    loss = C.c_float()
    assert L.lib.lrnde_sde_classifier_ce(h._h, C.c_void_p(u.data_ptr()), B, C.c_void_p(pc.data_ptr()), 17, C.c_void_p(lab.data_ptr()),
                                         C.byref(loss), None, None, None) == 4


# ---- the model: forward == the three calls == the oracle; pullback against float64 autograd ----
# Din, D, H, K, B, tol, nfine, mode, kind, dt0 — the issue's table, then one case each with the Milstein and the SRI step (their
# tolerances and explicit first steps are those of tests/test_host_sde_adaptive.py's pinned cases of the same widths)
MODEL_CASES = [
    (784, 32, 64, 10, 512, 0.14, 128, "unbiased", "EulerHeun", 0.0),     # BASELINE config 5
    (50, 32, 64, 10, 16, 0.05, 64, "biased", "EulerHeun", 0.0),
    (7, 2, 4, 3, 1, 0.05, 32, "none", "EulerHeun", 0.0),
    (100, 20, 48, 7, 33, 0.05, 64, "unbiased", "EulerHeun", 0.0),
    (60, 72, 32, 10, 6, 0.1, 32, "unbiased", "EulerHeun", 0.0),          # D > 64: generic kernels, host-controlled loop
    (50, 32, 64, 10, 40, 0.8, 64, "unbiased", "RKMil", 0.0),
    (50, 20, 48, 7, 7, 0.5, 32, "unbiased", "SRI", 0.0),
]
_ids = lambda c: "%s-%dx%dx%dx%d-B%d-%s" % (c[8], c[0], c[1], c[2], c[3], c[4], c[7]) if isinstance(c, tuple) else None


def _model_setup(P, O, case, seed=21):
    Din, D, H, K, B, tol, nfine, mode, kind, dt0 = case
    c = MC.model_case(Din, D, H, K, B, nfine, seed=seed, kind=kind)
    T = S.sri_tableau(O, 41, 0.1) if kind == "SRI" else None
    h = _handle(P, D, H)
    h.set_params(c["pd"], c["pg"])
    dev = {k: _cu(c[k]) for k in ("x", "pds", "pc", "labels", "W", "z", "Z", "z2")}
    lay = dict(mode=mode, t1_or_rand=0.37, z_local=dev["z"], saveat=(), save_start=0, dt0=dt0, solver=kind,
               tableau=None if T is None else [T[k] for k in O.SRI_FIELDS], path_z=dev["Z"], z_local2=dev["z2"])
    return c, T, h, dev, lay


def _oracle_forward(O, case, c, T, u0):
    Din, D, H, K, B, tol, nfine, mode, kind, dt0 = case
    drift, diff = S.oracle_fields(O, D, H, c["pd"], c["pg"])
    if kind == "EulerHeun":
        return O.sde_node_forward(drift, diff, u0, c["W"], 0.0, 1.0, tol, tol, mode=mode, t1_or_rand=0.37, z_local=c["z"], saveat=(),
                                  save_start=0, dt0=dt0)
    return S.sde_node_forward(O, kind, drift, diff, u0, c["W"], 0.0, 1.0, tol, tol, mode=mode, t1_or_rand=0.37, z_local=c["z"], saveat=(),
                              save_start=0, dt0=dt0, tableau=T, Z=c["Z"], z2_local=c["z2"])


@pytest.mark.parametrize("case", MODEL_CASES, ids=_ids)
def test_model_forward_equals_the_three_calls_and_the_oracle_and_pullback_matches_float64(oracle, gpu_pkg, case):
    Din, D, H, K, B, tol, nfine, mode, kind, dt0 = case
    c, T, h, dev, lay = _model_setup(gpu_pkg, oracle, case)
    # the three separate calls
    u0 = h.dense_forward(dev["x"], dev["pds"])
    f3 = h.node_forward_record(u0, dev["W"], 0.0, 1.0, tol, tol, **lay)
    h3 = h.classifier_ce(f3["u_end"].contiguous(), dev["pc"], K, dev["labels"])
    gen0 = h.record_generation()
    # the one call: the same bits
    fw = h.model_forward_record_ce(dev["x"], dev["pds"], dev["W"], 0.0, 1.0, tol, tol, dev["pc"], K, dev["labels"], **lay)
    assert fw["generation"] == gen0 + 1
    assert torch.equal(fw["u"], f3["u"]) and np.array_equal(fw["t"], f3["t"]) and fw["reg_val"] == f3["reg_val"] and fw["t1"] == f3["t1"]
    assert (fw["nfe_drift"], fw["nfe_diffusion"]) == (f3["nfe_drift"], f3["nfe_diffusion"]) and fw["stats"] == f3["stats"]
    assert fw["loss"] == h3["loss"] and torch.equal(fw["logits"], h3["logits"]) and torch.equal(fw["dpc"], h3["dpc"])
    # the layer part == the oracle fed the device's u0
    ref = _oracle_forward(oracle, case, c, T, u0.cpu().numpy())
    _check_forward(fw, ref, str(case))
    assert ref["naccept"] >= 2 and (fw["reg_val"] == 0) == (mode == "none")
    assert fw["nfe_drift"] != fw["nfe_diffusion"] or kind != "RKMil"     # (Milstein: 1 drift, 2 diffusion evaluations per step)
    # the pullback from the record, w_reg = 2
    bw = h.model_backward_recorded(w_reg=2.0, want_dx=True)
    r64 = MC.model_reference(c, ref, D, H, K, 2.0, tol, torch.float64, kind=kind, tableau=T, want_dx=True)
    r32 = MC.model_reference(c, ref, D, H, K, 2.0, tol, torch.float32, kind=kind, tableau=T, want_dx=True)
    got = dict(u0=u0.cpu().numpy(), u_end=fw["u_end"].cpu().numpy(), logits=fw["logits"].cpu().numpy(), d_classifier=fw["dpc"].cpu().numpy(),
               d_downsample=bw["dpd"].cpu().numpy(), d_drift=bw["dp_drift"].cpu().numpy(), d_diffusion=bw["dp_diff"].cpu().numpy(),
               dx=bw["dx"].cpu().numpy())
    print(f"{_ids(case)}: accepted {ref['naccept']}, rejected {ref['nreject']}, series {len(ref['t'])}, ce {fw['loss']:.5f}, reg_val {fw['reg_val']:.4g}")
    MC.check(_ids(case), got, r64, r32, ["u0", "u_end", "logits", "d_classifier", "d_downsample", "d_drift", "d_diffusion", "dx"])
    e, b = HC.rel_loss(fw["loss"], r64["ce"]), HC.loss_bound(r32["ce"], r64["ce"])
    print(f"{_ids(case)} ce: got {e:.2e} bound {b:.2e}")
    assert e <= b
    # dx = NULL gives the same parameter cotangents; a second pullback from the same record repeats bitwise
    bw2 = h.model_backward_recorded(w_reg=2.0)
    assert bw2["dx"] is None and all(torch.equal(bw2[k], bw[k]) for k in ("dpd", "dp_drift", "dp_diff"))


def test_regulariser_gradient_alone_through_the_model(oracle, gpu_pkg):
    """w_reg = 1 and a head whose weights are zero: the head sends no cotangent to sol.u[end], so the drift and diffusion
    cotangents are d reg_val / d ps alone and the downsample's is exactly zero.  An explicit first step (0.05) as in
    tests/test_gpu_sde_layer.py: the automatic one makes reg_val ~ 1e-6."""
    case = (50, 32, 64, 10, 64, 0.14, 64, "unbiased", "EulerHeun", 0.05)
    Din, D, H, K, B, tol, nfine, mode, kind, dt0 = case
    c, T, h, dev, lay = _model_setup(gpu_pkg, oracle, case, seed=33)
    c["pc"][:K * D] = 0
    dev["pc"] = _cu(c["pc"])
    u0 = h.dense_forward(dev["x"], dev["pds"])
    fw = h.model_forward_record_ce(dev["x"], dev["pds"], dev["W"], 0.0, 1.0, tol, tol, dev["pc"], K, dev["labels"], **lay)
    ref = _oracle_forward(oracle, case, c, T, u0.cpu().numpy())
    _check_forward(fw, ref, "regulariser alone")
    assert float(ref["reg_val"]) > 1e-6
    bw = h.model_backward_recorded(w_reg=1.0, want_dx=True)
    r64 = MC.model_reference(c, ref, D, H, K, 1.0, tol, torch.float64)
    r32 = MC.model_reference(c, ref, D, H, K, 1.0, tol, torch.float32)
    assert not bw["dpd"].any() and not bw["dx"].any() and not r64["d_downsample"].any()
    got = dict(d_drift=bw["dp_drift"].cpu().numpy(), d_diffusion=bw["dp_diff"].cpu().numpy(), d_classifier=fw["dpc"].cpu().numpy())
    assert np.abs(r64["d_drift"]).max() > 0 and np.abs(r64["d_diffusion"]).max() > 0
    MC.check("regulariser alone", got, r64, r32, ["d_drift", "d_diffusion", "d_classifier"])


def test_a_second_forward_between_forward_and_backward_is_detected(oracle, gpu_pkg):
    case = MODEL_CASES[1]
    Din, D, H, K, B, tol, nfine, mode, kind, dt0 = case
    c, T, h, dev, lay = _model_setup(gpu_pkg, oracle, case)
    fw = h.model_forward_record_ce(dev["x"], dev["pds"], dev["W"], 0.0, 1.0, tol, tol, dev["pc"], K, dev["labels"], **lay)
    first = h.model_backward_recorded(w_reg=2.0)
    u0 = h.dense_forward(dev["x"], dev["pds"])
    h.node_forward_record(u0, dev["W"], 0.0, 1.0, tol, tol, **lay)       # an evaluation pass on the same handle
    assert h.record_generation() == fw["generation"] + 1
    with pytest.raises(gpu_pkg.LrndeError, match=r"no usable record"):
        h.model_backward_recorded(w_reg=2.0)
    fw2 = h.model_forward_record_ce(dev["x"], dev["pds"], dev["W"], 0.0, 1.0, tol, tol, dev["pc"], K, dev["labels"], **lay)
    again = h.model_backward_recorded(w_reg=2.0)
    assert fw2["loss"] == fw["loss"] and all(torch.equal(again[k], first[k]) for k in ("dpd", "dp_drift", "dp_diff"))


# ---- the Python step ----
def _py_model(P, **kw):
    args = dict(in_dims=50, state_dims=32, hidden_dims=64, num_classes=10, abstol=0.14, reltol=0.14, nfine=64)
    args.update(kw)
    return P.construct_mlp_sde(**args)


def test_run_sde_training_step_equals_the_c_calls(oracle, gpu_pkg):
    P = gpu_pkg
    case = (50, 32, 64, 10, 16, 0.14, 64, "unbiased", "EulerHeun", 0.0)
    Din, D, H, K, B, tol, nfine, mode, kind, dt0 = case
    c = MC.model_case(Din, D, H, K, B, nfine, seed=21)
    model = _py_model(P)
    ps = dict(downsample=_cu(c["pds"]), neural_dsde=dict(drift=_cu(c["pd"]), diffusion=_cu(c["pg"])), classifier=_cu(c["pc"]))
    st = model.initialstates(np.random.default_rng(5))
    x, lab, W, z = _cu(c["x"]), _cu(c["labels"]), _cu(c["W"]), _cu(c["z"])
    loss, st_, stats, grads, times = P.run_sde_training_step(model, ps, st, x.reshape(B, 1, 5, 10), lab, 2.0, path=W, z_local=z)
    sn = st_["neural_dsde"]
    assert stats["nfe"] == (sn["nfe_drift"], sn["nfe_diffusion"]) and sn["reg_val"] == stats["reg_val"] != 0 and "rng" in sn
    assert loss == f32(stats["ce_loss"] + f32(2.0) * stats["reg_val"]) and times["fwd_time"] > 0 and times["bwd_time"] > 0
    # the same step through the separate C calls on a second handle: the t1 the step drew, then every piece
    import copy
    rng = copy.deepcopy(st["neural_dsde"]["rng"])
    rng.integers(0, 2 ** 64, dtype=np.uint64)                     # (device noise source: the seed comes first)
    t1 = f32(f32(rng.random(dtype=np.float32)) * f32(1.0) + f32(0.0))
    h = _handle(P, D, H)
    h.set_params(c["pd"], c["pg"])
    u0 = h.dense_forward(x, ps["downsample"])
    f3 = h.node_forward_record(u0, W, 0.0, 1.0, tol, tol, mode="unbiased", t1_or_rand=float(t1), z_local=z, saveat=(), save_start=0,
                               maxiters=10_000)
    h3 = h.classifier_ce(f3["u_end"].contiguous(), ps["classifier"], K, lab)
    du = torch.zeros_like(f3["u"]); du[-1] = h3["du"]
    b3 = h.node_backward_recorded(du, w_reg=2.0)
    d3 = h.dense_backward(x, ps["downsample"], b3["dx"])
    assert stats["ce_loss"] == h3["loss"] and stats["reg_val"] == f3["reg_val"] and torch.equal(stats["y_pred"], h3["logits"])
    assert stats["nfe"] == (f3["nfe_drift"], f3["nfe_diffusion"])
    assert torch.equal(grads["classifier"], h3["dpc"]) and torch.equal(grads["downsample"], d3["dpd"])
    assert torch.equal(grads["neural_dsde"]["drift"], b3["dp_drift"]) and torch.equal(grads["neural_dsde"]["diffusion"], b3["dp_diff"])
    # model(x, ps, st): the same y_pred and state; test mode runs mode none
    y, st_c = model(x, ps, st, path=W, z_local=z)
    assert torch.equal(y, stats["y_pred"]) and st_c["neural_dsde"]["reg_val"] == sn["reg_val"]
    assert (st_c["neural_dsde"]["nfe_drift"], st_c["neural_dsde"]["nfe_diffusion"]) == stats["nfe"]
    lt, st_t, stats_t, _, _ = P.run_sde_training_step(model, ps, model.testmode(st), x, lab, 2.0, path=W, z_local=z)
    assert stats_t["reg_val"] == 0 and st_t["neural_dsde"]["reg_val"] == 0 and lt == stats_t["ce_loss"]
    y_t, st_ct = model(x, ps, model.testmode(st), path=W, z_local=z)
    assert st_ct["neural_dsde"]["reg_val"] == 0 and torch.equal(y_t, stats_t["y_pred"])


def _train(P, nstep, B, Din, lr, seed):
    K = 10
    model = _py_model(P, in_dims=Din, nfine=32)
    p0 = P.glorot_mlp_sde_params(model, seed=seed)
    ps = dict(downsample=_cu(p0["downsample"]), neural_dsde={k: _cu(v) for k, v in p0["neural_dsde"].items()}, classifier=_cu(p0["classifier"]))
    flat = lambda d: [d["downsample"], d["neural_dsde"]["drift"], d["neural_dsde"]["diffusion"], d["classifier"]]
    opt = P.Optimiser("adam", learning_rate=lr)
    st = model.initialstates(np.random.default_rng(seed + 1))
    losses = []
    for i in range(nstep):
        x, lab = MC.clustered_batch(i, B, Din, K)
        loss, st, stats, grads, _ = P.run_sde_training_step(model, ps, st, _cu(x), _cu(lab), 1.0)
        assert np.isfinite(float(loss)) and stats["nfe"][0] > 0
        opt.update(flat(ps), flat(grads))
        losses.append(float(loss))
    return losses, [p.clone() for p in flat(ps)]


def test_two_runs_from_the_same_seeds_are_identical(gpu_pkg):
    la, pa = _train(gpu_pkg, 4, 16, 50, 2e-3, seed=3)
    lb, pb = _train(gpu_pkg, 4, 16, 50, 2e-3, seed=3)
    assert la == lb and all(torch.equal(a, b) for a, b in zip(pa, pb))
    assert len(set(la)) == len(la)                                # (the draws and the parameters move from step to step)


def test_a_short_adam_run_learns(gpu_pkg):
    losses, _ = _train(gpu_pkg, 40, 64, 784, 2e-3, seed=0)
    ratio = float(np.mean(losses[-5:]) / losses[0])
    print(f"loss {losses[0]:.4f} -> {np.mean(losses[-5:]):.4f} in {len(losses)} steps: ratio {ratio:.3f}")
    assert np.mean(losses[-5:]) < losses[0]
