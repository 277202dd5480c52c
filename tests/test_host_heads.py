"""The float64 references of tests/head_cases.py against the oracle's classifier and CIFAR heads, at every case of the two
tables the GPU tests (tests/test_gpu_heads.py) run: loss, logits and every gradient array within the suite's rule.  This
checks the references themselves, without a GPU."""
import numpy as np
import pytest

import head_cases as HC


@pytest.mark.parametrize("D,K,B,scale", HC.MLP_CASES)
def test_classifier_reference_matches_the_oracle(oracle, D, K, B, scale):
    c = HC.mlp_ref(D, K, B, scale)
    loss, lg, du, dpc = oracle.classifier_ce(c["u"], c["pc"], K, c["labels"])
    HC.check(f"oracle D={D} K={K} B={B} x{scale:g}", dict(loss=loss, logits=lg, du=du, dpc=dpc), c, ("logits", "du", "dpc"))
    assert c["labels"][0] == 0 and c["labels"][-1] == (K - 1 if B > 1 else 0)
    assert np.all(c["pc"][K * D:] != 0)
    if K == 1:
        assert c["r64"]["loss"] == 0 and not c["r64"]["du"].any() and not c["r64"]["dpc"].any()
        assert loss == 0 and not du.any() and not dpc.any()
    if scale > 1:   # the saturated cases are saturated: a class below the clamp of the kernels' exp at -87
        lg64 = c["r64"]["logits"]
        assert (lg64 - lg64.max(axis=1, keepdims=True)).min() < -87 and np.abs(lg64).max() > 100


@pytest.mark.parametrize("W,H,B,K,scale", HC.CIFAR_CASES)
def test_cifar_head_reference_matches_the_oracle(oracle, W, H, B, K, scale):
    c = HC.cifar_ref(W, H, B, K, scale)
    assert c["ph"].size == oracle.lib().lro_cifar_head_param_count(H, W, K)
    loss, lg, du, dph = oracle.cifar_head_ce(c["u"], c["ph"], K, c["labels"])
    HC.check(f"oracle {W}x{H} B={B} K={K} x{scale:g}", dict(loss=loss, logits=lg, du=du, dph=dph), c, ("logits", "du", "dph"),
             split=dict(dph=73))


def test_the_reference_reads_the_layout_of_the_kernels():
    """one weight at a time: class c, input k sits at pc[c + K*k], the bias of class c at pc[K*D + c]"""
    D, K = 3, 4
    u = np.array([[1.0, 2.0, 4.0]], np.float32)
    for c in range(K):
        for k in range(D + 1):
            pc = np.zeros(K * (D + 1), np.float32)
            pc[c + K * k] = 1.0
            lg = HC.classifier_reference(u, pc, K, [0], HC.torch.float64)["logits"][0]
            want = np.zeros(K); want[c] = u[0, k] if k < D else 1.0
            assert np.array_equal(lg, want), (c, k, lg)
