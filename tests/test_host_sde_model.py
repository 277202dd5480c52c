"""The MNIST-SDE model (experiments/src/construct.jl:202-210) — CPU side: the five C entry points are declared, exported and
bound and refuse a NULL handle; the model's parameter blocks have the reference's sizes and the Lux layout; the float64
restatement the GPU suite compares with (tests/sde_model_cases.py) agrees with the oracle's pieces."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import sde_model_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW = ("lrnde_sde_dense_forward", "lrnde_sde_dense_backward", "lrnde_sde_classifier_ce", "lrnde_sde_model_forward_record_ce",
       "lrnde_sde_model_backward_recorded")


def test_the_five_symbols_are_declared_exported_and_bound():
    import lrnde_amd  # noqa: F401
    from localregneuralde_jl_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lrnde.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, hdr, re.S)
        assert m, f"{name} is not declared in include/lrnde.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in bound and len(bound[name]) == len(m.group(1).split(",")), f"{name}: ctypes arity differs from the header"
    # every new entry point cites the reference lines it replaces
    doc = open(os.path.join(ROOT, "include", "lrnde.h")).read()
    blk = doc[doc.index("the MNIST-SDE model around the layer"):doc.index("int lrnde_sde_dense_forward(")]
    paras = {p.split()[0]: p for p in blk.split("\n * lrnde_")[1:]}
    for name in NEW:
        assert re.search(r"construct\.jl:\d+", paras[name[len("lrnde_"):]]), f"{name} cites no reference lines"
    src = open(os.path.join(ROOT, "julia", "LRNDEBackend.jl")).read()
    for name in NEW:
        assert ":" + name in src, f"{name} has no ccall wrapper in julia/LRNDEBackend.jl"


def test_a_null_handle_gives_a_status_not_a_crash():
    from localregneuralde_jl_amd import _lib
    lib = _lib.lib
    assert lib.lrnde_sde_dense_forward(None, None, 1, 1, None, None) == 4
    assert lib.lrnde_sde_dense_backward(None, None, 1, 1, None, None, None, None) == 4
    assert lib.lrnde_sde_classifier_ce(None, None, 1, None, 10, None, None, None, None, None) == 4
    assert lib.lrnde_sde_model_backward_recorded(None, 1, 0.0, None, None, None, None) == 4
    args = [None] * 35
    for i, a in enumerate(_lib.SYMBOLS[[n for n, _, _ in _lib.SYMBOLS].index("lrnde_sde_model_forward_record_ce")][2]):
        if a is _lib._i32:
            args[i] = 1
        elif a is _lib._f:
            args[i] = 0.0
    assert lib.lrnde_sde_model_forward_record_ce(*args) == 4


def test_construct_mlp_sde_has_the_references_blocks():
    import lrnde_amd as P
    model = P.construct_mlp_sde()
    ps = P.glorot_mlp_sde_params(model, seed=0)
    assert set(ps) == {"downsample", "neural_dsde", "classifier"} and set(ps["neural_dsde"]) == {"drift", "diffusion"}
    counts = dict(downsample=ps["downsample"].size, drift=ps["neural_dsde"]["drift"].size, diffusion=ps["neural_dsde"]["diffusion"].size,
                  classifier=ps["classifier"].size)
    assert counts == dict(downsample=25120, drift=4192, diffusion=1056, classifier=330), counts
    assert all(v.dtype == np.float32 for v in (ps["downsample"], ps["classifier"], ps["neural_dsde"]["drift"], ps["neural_dsde"]["diffusion"]))
    assert not ps["downsample"][32 * 784:].any() and ps["downsample"][:32 * 784].all()      # Lux: zero biases behind the weights
    nd = model.neural_dsde
    assert nd.kwargs["save_start"] is False and nd.maxiters == 10_000 and nd.noise_source == "device" and nd.adaptive
    assert nd.solver == "EulerHeun" and nd.regularize == "unbiased" and nd.desc.state_dim == 32 and nd.desc.hidden_dim == 64
    assert P.construct_mlp_sde(noise_source="host", regularize="biased", abstol=0.14).neural_dsde.noise_source == "host"
    st = model.initialstates(np.random.default_rng(0))
    assert st["neural_dsde"]["training"] is True and st["neural_dsde"]["nfe_diffusion"] == -1 and "rng" in st["neural_dsde"]
    assert model.testmode(st)["neural_dsde"]["training"] is False and st["neural_dsde"]["training"] is True
    small = P.construct_mlp_sde(in_dims=7, state_dims=2, hidden_dims=4, num_classes=3)
    p2 = P.glorot_mlp_sde_params(small, seed=1)
    assert [p2["downsample"].size, p2["neural_dsde"]["drift"].size, p2["neural_dsde"]["diffusion"].size, p2["classifier"].size] == [16, 22, 6, 9]
    with pytest.raises(ValueError):
        P.construct_mlp_sde(num_classes=17)
    assert model.flatten(torch.zeros(3, 1, 28, 28)).shape == (3, 784)
    with pytest.raises(ValueError):
        model.flatten(torch.zeros(3, 5))


def test_the_reference_reads_one_weight_at_a_time_from_the_lux_layout():
    """W[o][k] sits at o + D*k and the bias at D*Din + o: one entry set to one, everything else zero"""
    Din, D, B = 5, 3, 2
    x = torch.tensor(np.arange(1.0, 1.0 + B * Din).reshape(B, Din), dtype=torch.float64)
    for o in range(D):
        for k in range(Din):
            pd = torch.zeros(D * Din + D, dtype=torch.float64)
            pd[o + D * k] = 1.0
            u0 = MC.dense_apply(x, pd, D)
            want = torch.zeros(B, D, dtype=torch.float64)
            want[:, o] = x[:, k]
            assert torch.equal(u0, want), (o, k)
        pd = torch.zeros(D * Din + D, dtype=torch.float64)
        pd[D * Din + o] = 1.0
        want = torch.zeros(B, D, dtype=torch.float64)
        want[:, o] = 1.0
        assert torch.equal(MC.dense_apply(x, pd, D), want), o
    # and the pullback puts a cotangent where the weight sits
    c = MC.dense_case(Din, D, B)
    r = MC.dense_reference(c["x"], c["pd"], D, c["du0"], torch.float64)
    dW = c["du0"].astype(np.float64).T @ c["x"].astype(np.float64)          # [o][k]
    assert np.allclose(r["dpd"][:D * Din].reshape(Din, D).T, dW, rtol=1e-13, atol=0)
    assert np.allclose(r["dpd"][D * Din:], c["du0"].astype(np.float64).sum(0), rtol=1e-13, atol=0)
    assert np.allclose(r["dx"], c["du0"].astype(np.float64) @ c["pd"][:D * Din].astype(np.float64).reshape(Din, D).T, rtol=1e-13, atol=0)


@pytest.mark.parametrize("Din,D,H,K,B,tol,nfine,mode", [(50, 32, 64, 10, 16, 0.05, 64, "biased"), (7, 2, 4, 3, 1, 0.05, 32, "none"),
                                                        (100, 20, 48, 7, 33, 0.05, 64, "unbiased")])
def test_the_float64_model_agrees_with_the_oracles_pieces(oracle, Din, D, H, K, B, tol, nfine, mode):
    """float32 downsample -> oracle.sde_node_forward -> oracle.classifier_ce against the float64 restatement over the grid the
    oracle recorded: sol.u[end], logits, the loss, reg_val and the head's parameter cotangent, under the suite's rule"""
    c = MC.model_case(Din, D, H, K, B, nfine, seed=21)
    drift, diff = MC.S.oracle_fields(oracle, D, H, c["pd"], c["pg"])
    u0 = MC.dense_np32(c["x"], c["pds"], D)
    ref = oracle.sde_node_forward(drift, diff, u0, c["W"], 0.0, 1.0, tol, tol, mode=mode, t1_or_rand=0.37, z_local=c["z"], saveat=(), save_start=0)
    assert ref["naccept"] >= 2
    loss, logits, du, dpc = oracle.classifier_ce(ref["u"][-1], c["pc"], K, c["labels"])
    r64 = MC.model_reference(c, ref, D, H, K, 2.0, tol, torch.float64)
    r32 = MC.model_reference(c, ref, D, H, K, 2.0, tol, torch.float32)
    got = dict(u0=u0, u_end=ref["u"][-1], logits=logits, d_classifier=dpc)
    MC.check(f"Din={Din} D={D} B={B} {mode}", got, r64, r32, ["u0", "u_end", "logits", "d_classifier"])
    for name, a, b64, b32 in (("ce", float(loss), r64["ce"], r32["ce"]), ("reg_val", float(ref["reg_val"]), r64["reg_val"], r32["reg_val"])):
        e, bnd = MC.rel([a], [b64]), MC.bound([b32], [b64])
        print(f"{name}: got {e:.2e} bound {bnd:.2e}")
        assert e <= bnd, (name, e, bnd)
    assert (ref["reg_val"] == 0) == (mode == "none") and (r64["reg_val"] == 0) == (mode == "none")
    for k in ("d_downsample", "d_drift", "d_diffusion"):
        assert np.isfinite(r64[k]).all() and r64[k].any(), k
