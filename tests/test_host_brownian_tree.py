"""The virtual Brownian tree's numpy restatement (tests/brownian_tree_np.py; csrc/lrnde_sde_tree.hpp) on the CPU:

* the descent to one index equals the full build at every index, and a coarser tree is every 2^(L'-L)-th row of a finer one,
  bit for bit;
* the level scales the kernels form by scaling s_1 / s_2 with a power of two are the definition's own;
* over >= 4 M increments of Philox normals (tests/philox_np.py) the path is a Brownian motion: increment variance, lag-1
  correlation along the grid and Var(W[nfine]) / span inside 6-sigma bands;
* the layer's constructor takes noise_source="tree" and refuses a grid that is no power of two and a fixed-grid solve."""
import numpy as np
import pytest

import brownian_tree_np as BT
import philox_np as PX

f32 = np.float32
SEED = 0x13198A2E03707344


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


@pytest.mark.parametrize("L", [0, 1, 6])
@pytest.mark.parametrize("span", [1.0, 1.5])
def test_descent_equals_the_build_at_every_index(L, span):
    nfine = 1 << L
    z = PX.normals(SEED, 6, max(nfine, 1), 37)
    W = BT.build(z, L, span)
    assert W.shape == (nfine + 1, 37) and W.dtype == f32 and not W[0].any()
    assert np.array_equal(_bits(W[nfine]), _bits(BT.scale_top(span) * z[0]))
    for k in range(nfine + 1):
        assert np.array_equal(_bits(BT.descend(z, L, span, k)), _bits(W[k])), k
    assert [BT.levels_of(k, 3) for k in range(9)] == [0, 3, 2, 3, 1, 3, 2, 3, 0]


def test_refinement_consistency_is_bitwise():
    z = PX.normals(SEED, 6, 256, 29)
    W8 = BT.build(z, 8, 0.75)
    for L in (0, 1, 5):
        assert np.array_equal(_bits(BT.build(z, L, 0.75)), _bits(W8[:: 1 << (8 - L)])), L
    # ... and a descent at the coarse level is the descent to the same time at the fine one
    assert np.array_equal(_bits(BT.descend(z, 5, 0.75, 11)), _bits(BT.descend(z, 8, 0.75, 88)))


@pytest.mark.parametrize("span", [1.0, 1.5, 0.3, 7.25, 1e-3, 20.0])
def test_level_scales_are_two_base_values_times_powers_of_two(span):
    """what the kernels do: s_l = s_1 2^-((l-1)/2) for odd l, s_2 2^-((l-2)/2) for even l — a power of four under a float64 square
    root is a power of two outside it, and a power of two commutes with the rounding to float32"""
    s1, s2 = BT.scale_level(span, 1), BT.scale_level(span, 2)
    for l in range(1, 21):
        base = s1 if l & 1 else s2
        assert BT.scale_level(span, l) == f32(np.ldexp(base, -((l - 1) >> 1))), (span, l)
    assert BT.scale_top(span) == f32(np.sqrt(np.float64(f32(span))))


def test_statistics_of_four_million_tree_increments():
    L, ncols, span = 8, 16384, f32(1.5)
    nfine = 1 << L
    z = PX.normals(SEED, 6, nfine, ncols)
    W = BT.build(z, L, span).astype(np.float64)
    inc = np.diff(W, axis=0)
    n = inc.size
    assert n >= 4_000_000
    h = float(span) / nfine
    x = inc / np.sqrt(h)                                  # standard normal if W is a Brownian motion on the grid
    mean, var = float(x.mean()), float(x.var())
    lag = float((x[1:] * x[:-1]).mean())
    vT = float(W[nfine].var()) / float(span)
    print(f"{n} increments: mean {mean:.3e}, var/h {var:.5f}, lag-1 corr along the grid {lag:.3e}, Var(W[nfine])/span {vT:.4f}")
    assert abs(mean) < 6 / np.sqrt(n)
    assert abs(var - 1) < 6 * np.sqrt(2 / n)
    assert abs(lag) < 6 / np.sqrt(n - ncols)
    assert abs(vT - 1) < 6 * np.sqrt(2 / ncols)
    # increments over a longer lag (32 intervals, non-overlapping): the variance grows linearly
    x32 = np.diff(W[::32], axis=0) / np.sqrt(32 * h)
    assert abs(float(x32.var()) - 1) < 6 * np.sqrt(2 / x32.size)


def test_constructor_takes_the_tree_and_refuses_what_it_cannot_run():
    import lrnde_amd as P
    mk = lambda **kw: P.NeuralDSDE(P.Chain(P.Dense(4, 8, "tanh"), P.Dense(8, 4)), P.Dense(4, 4), noise_source="tree", **kw)
    node = mk(nfine=64)
    assert node.noise_source == "tree" and node.adaptive and node.nfine == 64
    assert mk(nfine=1 << 20).nfine == 1 << 20 and mk(nfine=1).nfine == 1
    for bad in (100, 0, 1 << 21, 48):
        with pytest.raises(ValueError, match="nfine"):
            mk(nfine=bad)
    with pytest.raises(ValueError, match="adaptive"):
        mk(nfine=64, adaptive=False)
    with pytest.raises(ValueError, match="adaptive"):
        mk(nfine=64, solver="RKMil")     # (Milstein marches the fixed grid unless adaptive=True)
    assert mk(nfine=64, solver="RKMil", adaptive=True).solver == "RKMil"
    from localregneuralde_jl_amd.sde_model import construct_mlp_sde
    m = construct_mlp_sde(in_dims=12, state_dims=8, hidden_dims=16, num_classes=3, nfine=32, noise_source="tree")
    assert m.neural_dsde.noise_source == "tree" and m.neural_dsde.nfine == 32
