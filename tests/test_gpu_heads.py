"""The classifier heads on the GPU against float64 autograd (tests/head_cases.py), at every launch form.

  MLP-handle head (lrnde_classifier_ce: k_cls_fwd_bwdx<WLDS, KT> + k_cls_bwdw_loss, csrc/lrnde_cls_fused.hpp): the three
      instantiations <true,10> (K = 10, weights in LDS), <true,0> (any other K, weights in LDS), <false,0> (parameter block
      over 61440 bytes, read from memory), both sides of that boundary at K = 10 and K = 16, the second LDS staging trip,
      K = 1 and K = 16, the parameter-gradient tiles at H := K with a ragged last block, weights x 40;
  CIFAR head (lrnde_cifar_head_ce: k_head_conv, k_cls_fwd / k_cls_bwd_x / k_cls_bwd_w of csrc/lrnde_cls.hpp, k_head_bwd):
      B = 1, K = 3 / 7 / 16, a non-square image, all three batch loops of k_cls_bwd_w, dense weights x 40.

Every array (logits, du, dpc; for the CIFAR head dph[:73] and dph[73:]) is compared with the float64 reference and passes at
rel <= max(1e-5, 4 x the distance of the float32 torch run from the float64 run), relative to the float64 array's norm; the
loss at max(1e-5, 4 x |f32 - f64| / |f64|).  Every call runs twice and must return the same bits.  The shapes and what each
one reaches are listed beside head_cases.MLP_CASES / CIFAR_CASES.

Measured on an MI355X (worst relative error over the cases of a form, beside its bound; the float32 torch run is at most
1.8e-6 from the float64 run at every case, so the floor of 1e-5 is the bound everywhere):

    form                  loss      logits    du        dpc       bound
    <true,10>             1.1e-07   1.4e-07   7.8e-07   7.7e-07   1e-05     (du, dpc: the x 40 case)
    <true,0>              7.7e-08   9.9e-08   1.3e-06   1.3e-06   1e-05     (du, dpc: the x 40 case; 1.3e-07 without it)
    <false,0>             2.5e-08   1.1e-07   1.3e-07   1.3e-07   1e-05
    <false,0>, dpc of the rows shared with the LDS form: 7.7e-07 (D = 784 in 1536) and 9.1e-08 (D = 600 in 960)
    CIFAR head            1.6e-07   2.1e-07   7.7e-07   dph[:73] 6.1e-07, dph[73:] 8.2e-07   1e-05   (x 40; 2.5e-07 without it)

K = 1 returns exact zeros; the bitwise form-against-form, want_grads=False, fused-entry and repeat checks hold."""
import numpy as np
import pytest
import torch

import head_cases as HC

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def form(D, K):
    """the instantiation cls_enqueue picks (csrc/lrnde_kernels.hip)"""
    lds = 4 * K * (D + 1) <= 60 * 1024
    return "<true,10>" if lds and K == 10 else "<true,0>" if lds else "<false,0>"


def mlp_handle(P, D, H=4):
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    return Handle(_mlp_desc(P.TDChain(P.Chain(P.Dense(D + 1, H, "tanh"), P.Dense(H + 1, D)))))


def host(r):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


def same_bits(a, b, keys):
    for k in keys:
        x, y = np.asarray(a[k], np.float32), np.asarray(b[k], np.float32)
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), k


def run_mlp(h, u, pc, K, labels, want_grads=True):
    return host(h.classifier_ce(dev(u), dev(pc), K, dev(labels), want_grads=want_grads))


@pytest.mark.parametrize("D,K,B,scale", HC.MLP_CASES)
def test_classifier_head_against_float64(gpu_pkg, D, K, B, scale):
    c = HC.mlp_ref(D, K, B, scale)
    h = mlp_handle(gpu_pkg, D)
    got = run_mlp(h, c["u"], c["pc"], K, c["labels"])
    same_bits(got, run_mlp(h, c["u"], c["pc"], K, c["labels"]), ("loss", "logits", "du", "dpc"))
    assert got["logits"].shape == (B, K) and got["du"].shape == (B, D) and got["dpc"].shape == (K * (D + 1),)
    HC.check(f"mlp {form(D, K)} D={D} K={K} B={B} x{scale:g}", got, c, ("logits", "du", "dpc"))
    if K == 1:   # softmax of one class: expf_c(0) == 1, so nothing is left of the loss or of its cotangents
        assert got["loss"] == 0 and not got["du"].any() and not got["dpc"].any()


@pytest.mark.parametrize("D,K,B,scale", [(100, 7, 6, 40.0), (784, 10, 9, 40.0)])
def test_classifier_head_without_gradients(gpu_pkg, D, K, B, scale):
    """du = dpc = NULL: no state cotangent pass and no parameter-gradient tiles; loss and logits are the same bits"""
    c = HC.mlp_ref(D, K, B, scale)
    h = mlp_handle(gpu_pkg, D)
    full = run_mlp(h, c["u"], c["pc"], K, c["labels"])
    fwd = run_mlp(h, c["u"], c["pc"], K, c["labels"], want_grads=False)
    assert fwd["du"] is None and fwd["dpc"] is None
    same_bits(full, fwd, ("loss", "logits"))
    same_bits(fwd, run_mlp(h, c["u"], c["pc"], K, c["labels"], want_grads=False), ("loss", "logits"))
    same_bits(full, run_mlp(h, c["u"], c["pc"], K, c["labels"]), ("loss", "logits", "du", "dpc"))


@pytest.mark.parametrize("D,K,B,scale,Dbig", [(784, 10, 9, 40.0, 1536), (600, 16, 5, 1.0, 960)])
def test_the_forms_agree_bit_for_bit(gpu_pkg, D, K, B, scale, Dbig):
    """"same values, same order": the same samples zero-padded to Dbig columns run the form that reads the weights from memory;
    fma(w, +0, acc) leaves every lane's partial sum as it is, so logits, loss and du[:, :D] are the bits of the LDS form.  The
    rows D.. of the padded weights are random.  dpc of the shared rows (and the bias) is summed by other tiles: within the rule."""
    c = HC.mlp_ref(D, K, B, scale)
    assert form(D, K) != form(Dbig, K) == "<false,0>"
    small = run_mlp(mlp_handle(gpu_pkg, D), c["u"], c["pc"], K, c["labels"])
    rng = np.random.default_rng(41)
    up = np.zeros((B, Dbig), np.float32); up[:, :D] = c["u"]
    extra = ((rng.random(K * (Dbig - D)) - 0.5) * 0.1 * scale).astype(np.float32)
    pcp = np.concatenate([c["pc"][:K * D], extra, c["pc"][K * D:]])
    hb = mlp_handle(gpu_pkg, Dbig)
    big = run_mlp(hb, up, pcp, K, c["labels"])
    same_bits(big, run_mlp(hb, up, pcp, K, c["labels"]), ("loss", "logits", "du", "dpc"))
    same_bits(small, dict(loss=big["loss"], logits=big["logits"], du=np.ascontiguousarray(big["du"][:, :D])), ("loss", "logits", "du"))
    shared = np.concatenate([big["dpc"][:K * D], big["dpc"][K * Dbig:]])
    e, b = HC.rel(shared, c["r64"]["dpc"]), HC.bound(c["r32"]["dpc"], c["r64"]["dpc"])
    print(f"mlp {form(Dbig, K)} D={D} padded to {Dbig} K={K} B={B} dpc shared rows: got {e:.2e} bound {b:.2e}")
    assert e <= b
    assert not big["dpc"][K * D:K * Dbig].any()       # the cotangent of a weight whose input is zero in every sample


@pytest.mark.parametrize("D,K,B", [(100, 7, 6), (600, 16, 5)])
def test_classifier_head_refuses_a_label_outside_the_classes(gpu_pkg, D, K, B):
    P = gpu_pkg
    c = HC.mlp_ref(D, K, B, 40.0 if K == 7 else 1.0)
    h = mlp_handle(P, D)
    for wrong in (-1, K):
        bad = c["labels"].copy(); bad[B // 2] = wrong
        with pytest.raises(P.LrndeError, match="label"):
            run_mlp(h, c["u"], c["pc"], K, bad)
    after = run_mlp(h, c["u"], c["pc"], K, c["labels"])
    same_bits(after, run_mlp(mlp_handle(P, D), c["u"], c["pc"], K, c["labels"]), ("loss", "logits", "du", "dpc"))


def test_fused_forward_and_head_equal_the_two_calls_at_three_classes(gpu_pkg):
    """lrnde_node_forward_record_ce == lrnde_node_forward_record then lrnde_classifier_ce, bit for bit, at a runtime K
    (tests/test_gpu_training_loop.py holds this at K = 10)"""
    from localregneuralde_jl_amd.layers import Handle, _mlp_desc
    P = gpu_pkg
    D, H, K, B = 40, 24, 3, 16
    model = P.TDChain(P.Chain(P.Dense(D + 1, H, "tanh"), P.Dense(H + 1, D)))
    p = torch.from_numpy(P.glorot_params(model, seed=5) * np.float32(1.5))
    c = HC.mlp_ref(D, K, B, 1.0)
    x, pc, lab = dev(c["u"]), dev(c["pc"]), dev(c["labels"])
    ha, hb = Handle(_mlp_desc(model)), Handle(_mlp_desc(model))
    ha.set_params(p); hb.set_params(p)
    kw = dict(mode="unbiased", reg_type="error_estimate", t1_or_rand=0.43, maxiters=10000)
    for rep in range(2):
        fa = ha.node_forward_record(x, 0.0, 1.0, 1e-5, 1e-5, **kw)
        qa = ha.classifier_ce(fa["u_end"], pc, K, lab)
        fb, qb = hb.node_forward_record_ce(x, 0.0, 1.0, 1e-5, 1e-5, pc, K, lab, **kw)
        assert torch.equal(fa["u_end"], fb["u_end"]) and fa["reg_val"] == fb["reg_val"] and fa["nfe"] == fb["nfe"] and fa["stats"] == fb["stats"]
        same_bits(host(qa), host(qb), ("loss", "logits", "du", "dpc"))
    assert fa["stats"]["naccept"] > 1


# ---- the CIFAR head ----
def run_cifar(h, u, ph, K, labels, want_grads=True):
    return host(h.cifar_head_ce(dev(u), dev(ph), K, dev(labels), want_grads=want_grads))


@pytest.mark.parametrize("W,H,B,K,scale", HC.CIFAR_CASES)
def test_cifar_head_against_float64(gpu_pkg, W, H, B, K, scale):
    c = HC.cifar_ref(W, H, B, K, scale)
    h = gpu_pkg.ConvHandle(W, H, 8, 64)
    got = run_cifar(h, c["u"], c["ph"], K, c["labels"])
    same_bits(got, run_cifar(h, c["u"], c["ph"], K, c["labels"]), ("loss", "logits", "du", "dph"))
    assert got["logits"].shape == (B, K) and got["du"].shape == (B, 8, H, W) and got["dph"].shape == (73 + K * (H * W + 1),)
    HC.check(f"cifar {W}x{H} B={B} K={K} x{scale:g}", got, c, ("logits", "du", "dph"), split=dict(dph=73))


@pytest.mark.parametrize("W,H,B,K,scale", [(8, 8, 23, 10, 1.0), (12, 8, 6, 16, 1.0)])
def test_cifar_head_without_gradients(gpu_pkg, W, H, B, K, scale):
    c = HC.cifar_ref(W, H, B, K, scale)
    h = gpu_pkg.ConvHandle(W, H, 8, 64)
    full = run_cifar(h, c["u"], c["ph"], K, c["labels"])
    fwd = run_cifar(h, c["u"], c["ph"], K, c["labels"], want_grads=False)
    assert fwd["du"] is None and fwd["dph"] is None
    same_bits(full, fwd, ("loss", "logits"))
    same_bits(fwd, run_cifar(h, c["u"], c["ph"], K, c["labels"], want_grads=False), ("loss", "logits"))


@pytest.mark.parametrize("W,H,B,K", [(16, 16, 17, 7), (12, 8, 6, 16)])
def test_cifar_head_refuses_a_label_outside_the_classes(gpu_pkg, W, H, B, K):
    """as the MLP-handle head: LRNDE_BADARG, "a label is outside [0, K)", and the handle goes on"""
    P = gpu_pkg
    c = HC.cifar_ref(W, H, B, K, 1.0)
    h = P.ConvHandle(W, H, 8, 64)
    for wrong in (-1, K):
        bad = c["labels"].copy(); bad[B // 2] = wrong
        with pytest.raises(P.LrndeError, match=r"a label is outside \[0, %d\)" % K) as e:
            run_cifar(h, c["u"], c["ph"], K, bad)
        assert e.value.code == 4   # LRNDE_BADARG
    after = run_cifar(h, c["u"], c["ph"], K, c["labels"])
    same_bits(after, run_cifar(P.ConvHandle(W, H, 8, 64), c["u"], c["ph"], K, c["labels"]), ("loss", "logits", "du", "dph"))
