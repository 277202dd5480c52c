"""CPU side of the wide Dense-chain handle's device-controlled adjoint loop: the C ABI entry point and
its bindings, the layer's keyword, the branch table of the two kernels from the shapes alone, and the gate's arithmetic
against hand-computed values."""
import inspect
import os
import re

import pytest

import wide_chain_adjoint_cases as WA
import wide_chain_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    import lrnde_amd
    return lrnde_amd


def test_entry_point_is_declared_bound_and_ccalled(P):
    from localregneuralde_jl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lrnde.h")).read()
    assert re.search(r"int\s+lrnde_set_adjoint_loop\(lrnde_ctx\*\s*\w*,\s*int32_t\s+\w+\);", hdr)
    assert re.search(r"enum\s*\{\s*LRNDE_ADJ_LOOP_AUTO\s*=\s*0,\s*LRNDE_ADJ_LOOP_DEVICE\s*=\s*1\s*\}", hdr)
    assert "Its continuous adjoint runs the host-controlled loop. */" not in hdr
    sym = {n: a for n, _r, a in _lib.SYMBOLS}
    assert "lrnde_set_adjoint_loop" in sym and len(sym["lrnde_set_adjoint_loop"]) == 2
    jl = open(os.path.join(ROOT, "julia", "LRNDEBackend.jl")).read()
    m = re.search(r"ccall\(\(:lrnde_set_adjoint_loop, lib\), Cint, \((.*?)\),(.*?)\)\)", jl)
    assert m and len(m.group(1).split(",")) == 2 and len(m.group(2).split(",")) == 2


def test_layer_keyword(P):
    model = WC.shapes(P)["physionet"]
    with pytest.raises(ValueError):
        P.NeuralODE(model, field="wide_chain", adjoint_loop="sometimes")
    for field in ("dense_chain", "wide_chain"):
        for loop in ("auto", "device"):
            assert P.NeuralODE(model, field=field, adjoint_loop=loop).adjoint_loop == loop
    mlp = WC.shapes(P)["mnist2"]
    assert P.NeuralODE(mlp, field="auto", adjoint_loop="device").adjoint_loop == "device"
    assert P.NeuralODE(mlp).adjoint_loop == "auto"


def test_loop_names_and_docstring(P):
    from localregneuralde_jl_amd.layers import Handle
    assert Handle.ADJOINT_LOOPS == ("host", "device", "chain_device")
    assert Handle.ADJOINT_LOOP_NAMES[:3] == Handle.ADJOINT_LOOPS and Handle.ADJOINT_LOOP_NAMES[3] == "wide_device"
    assert '"wide_device"' in inspect.getdoc(P.NeuralODE.pullback)


def test_branch_table(P):
    """every branch of k_wadj_step / k_wadj_mu is taken by the case of test_both_loops_same_bits named for it, and those
    cases are among the ones that test runs"""
    assert set(WA.BRANCH_CASE) == set(WA.BRANCHES)
    for br, (name, B, series) in WA.BRANCH_CASE.items():
        assert name in WA.BITS_SHAPES and B in WA.BITS_BATCHES and series in WA.SERIES
        assert br in WA.case_branches(P, name, B, series), (br, name, B, series)
    # the shapes reach every branch of wide_gemm too, forward and transposed (WC.gemm_paths)
    paths = set()
    for name in WA.BITS_SHAPES:
        for f, g in WC.gemm_paths(WC.model_dims(WC.shapes(P)[name])):
            paths.update((f, g))
    assert {"single", "split", "cap_fallback"} <= paths, paths


def test_work_items_by_hand():
    # mnist3: 784 -> 100: 7 x 49 blocks = 4 x 25 groups, 2 chunks; 100 -> 100: 4 x 4, 2; 100 -> 784: 25 x 4, 13
    assert WA.mu_items([784, 100, 100, 784]) == [(100, 2), (16, 2), (100, 13)]
    # full1024: 64 x 64 blocks = 32 x 32 groups and 16 chunks per layer
    assert WA.mu_items([1024, 1024, 1024]) == [(1024, 16), (1024, 16)]
    # deep16: 9 x 9 blocks = 5 x 5 groups, 3 chunks, 16 layers: more than the grid
    assert sum(g + c for g, c in WA.mu_items([144] * 17)) == 448 > WA.MAX_MU_BLOCKS


def test_gate_by_hand():
    # mnist3 at B = 512: record rows 784 + 112 | 112 + 112 | 112 + 784, act0' 784: 2800 rows x 16 columns
    assert WA.rec_floats([784, 100, 100, 784]) == 44800
    g = WA.gate([784, 100, 100, 784], 512)
    assert g["fits"] and g["nwg"] == 32 and g["nitems"] == 233 and g["nmu"] == 233
    assert g["bytes"] == 8 * 32 * 44800 * 4 + 2 * 212 + 5 * (32 + 233) * 8 == 45886224
    assert g["lds"] <= WC.WIDE_LDS_MAX
    # full1024: 2 x (1024 + 1024) + 1024 rows; 8 slots of one tile are 2 621 440 bytes, 102 tiles fit 256 MiB, 103 do not
    assert WA.rec_floats([1024, 1024, 1024]) == 81920
    assert 8 * 81920 * 4 == 2621440
    g = WA.gate([1024, 1024, 1024], 102 * 16)
    assert g["fits"] and g["nmu"] == 256 and g["bytes"] == 102 * 2621440 + 424 + 5 * (102 + 256) * 8 <= WA.SCRATCH_MAX
    g = WA.gate([1024, 1024, 1024], 102 * 16 + 1)
    assert not g["fits"] and g["why"] == "WIDE_SCRATCH_MAX" and g["bytes"] > WA.SCRATCH_MAX
    assert WA.first_refused_batch([1024, 1024, 1024]) == 1633
    # the step kernel's LDS at D = 1024: two 64 KiB activation buffers, the partial region the forward kernels have, the tail
    assert g["lds"] == 2 * 1024 * 16 * 4 + 4 * WC.partcap([1024, 1024, 1024]) + WC.LDS_TAIL + 212 <= WC.WIDE_LDS_MAX
    # the workgroup limit comes first only for a narrow chain
    g = WA.gate([20, 40, 20], 4096 * 16 + 1)
    assert not g["fits"] and g["why"] == "CHADJ_MAX_WG"
