"""Host side of the Dense-chain field (lrnde_chain_desc, lrnde_chain_param_count, layers._chain_desc, the flat layout,
NeuralODE(field=...)): no GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _desc(nl, td, dims, acts=None, in_act=0):
    from localregneuralde_jl_amd import _lib as L
    d = L.ChainDesc()
    d.nlayers, d.time_dep, d.input_act = nl, td, in_act
    for i, v in enumerate(dims):
        d.dims[i] = v
    for i, a in enumerate(acts or [0] * nl):
        d.act[i] = a
    return d


def test_chain_desc_layout_and_param_counts():
    import lrnde_amd  # noqa: F401
    from localregneuralde_jl_amd import _lib as L
    assert ctypes.sizeof(L.ChainDesc) == 144   # 3 + 17 + 16 int32 (include/lrnde.h)
    assert L.ChainDesc.dims.offset == 12 and L.ChainDesc.act.offset == 80
    phys = _desc(8, 0, [20, 40] * 4 + [20], [1] * 8, in_act=1)
    assert L.lib.lrnde_chain_param_count(ctypes.byref(phys)) == 8 * 40 * 20 + 4 * 40 + 4 * 20 == 6640
    # no size limits in the count: the 784-wide MNIST TDChain with two hidden layers
    mn = _desc(3, 1, [784, 100, 100, 784])
    assert L.lib.lrnde_chain_param_count(ctypes.byref(mn)) == 168768
    # the 2-layer shape has the MLP field's count
    d2 = _desc(2, 1, [784, 100, 784])
    assert L.lib.lrnde_chain_param_count(ctypes.byref(d2)) == L.lib.lrnde_param_count(ctypes.byref(L.ModelDesc(784, 100, 1, 1)))
    assert L.lib.lrnde_chain_param_count(ctypes.byref(_desc(0, 0, [4]))) == 0


def test_physionet_desc():
    import lrnde_amd as P
    from localregneuralde_jl_amd.layers import _chain_desc, chain_param_count
    m = P.Chain(P.Activation("tanh"), *[P.Dense(20, 40, "tanh") if i % 2 == 0 else P.Dense(40, 20, "tanh") for i in range(8)])
    d = _chain_desc(m)
    assert (d.nlayers, d.time_dep, d.input_act) == (8, 0, 1)
    assert list(d.dims)[:9] == [20, 40] * 4 + [20] and list(d.act)[:8] == [1] * 8
    assert chain_param_count(d) == 6640 and P.glorot_chain_params(m).size == 6640


def test_chain_desc_validation():
    import lrnde_amd as P
    from localregneuralde_jl_amd.layers import _chain_desc
    with pytest.raises(ValueError, match="do not chain"):
        _chain_desc(P.Chain(P.Dense(4, 8), P.Dense(7, 4)))
    with pytest.raises(ValueError, match="same width"):
        _chain_desc(P.Chain(P.Dense(4, 8), P.Dense(8, 5)))
    with pytest.raises(ValueError, match="do not chain"):
        _chain_desc(P.TDChain(P.Chain(P.Dense(5, 8), P.Dense(8, 4))))      # second Dense lacks the t row
    with pytest.raises(NotImplementedError, match="1..128"):
        _chain_desc(P.Chain(P.Dense(4, 129), P.Dense(129, 4)))
    _chain_desc(P.TDChain(P.Chain(P.Dense(129, 128))))                       # 128 + the t row is fine
    with pytest.raises(NotImplementedError, match="weight image"):
        _chain_desc(P.TDChain(P.Chain(P.Dense(129, 128), P.Dense(129, 128))))  # 2 x 130 x 128 fp32 > 128 KB
    with pytest.raises(NotImplementedError, match="first element"):
        _chain_desc(P.Chain(P.Dense(4, 8), P.Activation("tanh"), P.Dense(8, 4)))
    with pytest.raises(NotImplementedError, match="TDChain"):
        _chain_desc(P.TDChain(P.Chain(P.Activation("tanh"), P.Dense(5, 4))))
    with pytest.raises(NotImplementedError, match="1..16"):
        _chain_desc(P.Chain(*[P.Dense(4, 4) for _ in range(17)]))
    with pytest.raises(ValueError):
        P.Activation("relu")


def test_flat_layout_is_lux_order():
    """per layer vec(W) (out x (in+td), column-major, t column last) then b"""
    import lrnde_amd as P
    W1 = torch.arange(15.).reshape(3, 5)   # TDChain Dense(4+1 => 3)
    b1 = torch.tensor([100., 101., 102.])
    W2 = torch.arange(20., 36.).reshape(4, 4)  # Dense(3+1 => 4)
    b2 = torch.tensor([200., 201., 202., 203.])
    flat = P.flatten_chain_params([(W1, b1), (W2, b2)])
    hand = [W1[o, k].item() for k in range(5) for o in range(3)] + b1.tolist() + \
           [W2[o, k].item() for k in range(4) for o in range(4)] + b2.tolist()
    assert flat.tolist() == hand
    assert torch.equal(flat, P.flatten_params(W1, b1, W2, b2))   # the 2-layer form is the MLP field's layout
    m = P.TDChain(P.Chain(P.Dense(5, 3, "tanh"), P.Dense(4, 4)))
    assert np.array_equal(P.glorot_chain_params(m, seed=3), P.glorot_params(m, seed=3))


def test_field_routing():
    import lrnde_amd as P
    m3 = P.Chain(P.Dense(2, 4), P.Dense(4, 4), P.Dense(4, 2))
    with pytest.raises(NotImplementedError):
        P.NeuralODE(m3)                                   # "auto" keeps today's routing
    node = P.NeuralODE(m3, field="dense_chain")
    assert node.field == "dense_chain" and node.desc.nlayers == 3
    node2 = P.NeuralODE(P.TDChain(P.Chain(P.Dense(3, 4), P.Dense(5, 2))), field="dense_chain")
    assert node2.desc.time_dep == 1 and list(node2.desc.dims)[:3] == [2, 4, 2]
    with pytest.raises(NotImplementedError):
        P.NeuralODE(m3, solver="VCAB3", field="dense_chain")
    with pytest.raises(ValueError):
        P.NeuralODE(m3, field="mlp")


def test_julia_binding_routes_chains():
    src = open(os.path.join(ROOT, "julia", "LRNDEBackend.jl")).read()
    layer = open(os.path.join(ROOT, "julia", "LRNDELayer.jl")).read()
    assert ":lrnde_create_chain" in src and ":lrnde_chain_param_count" in src
    assert "UNTESTED" in src and "chain" in layer.lower()
