"""Host side of the conv field's geometry coverage (tests/conv_geometry_cases.py): no GPU needed.

  * geometry() of the cases module is the function the kernels use: csrc/lrnde_conv_geom.hpp compiled into
    tests/conv_geom_host.cpp, over the table and over every legal (W, H) with H <= 40;
  * what the table claims to cover is asserted: every MT in 1..8 ragged where that is possible, MT 1, 2, 3, 5 also with a
    full last tile, TR == 1 with interior strips, widths strictly between 64 and 128, and the multi-strip cases really
    exceeding the workgroup cap of the weight-gradient launches they are meant to make loop;
  * the reference is good enough to carry the GPU bars at these shapes: the oracle's f-eval within 3e-6 of the output
    scale of the float64 torch restatement (tests/test_oracle_conv.py), its VJP within 1e-5 per parameter block of float64
    autograd, at every case of tests/test_gpu_conv_geometry.py."""
import os
import subprocess

import numpy as np
import pytest
import torch

import conv_geometry_cases as G
from test_oracle_conv import torch_conv_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def geom_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_geom") / "conv_geom_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "localregneuralde.jl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "conv_geom_host.cpp"), "-o", exe], check=True)
    return exe


def _strip_rows(exe, pairs):
    out = {}
    for i in range(0, len(pairs), 400):
        chunk = pairs[i:i + 400]
        r = subprocess.run([exe] + [str(v) for wh in chunk for v in wh], check=True, capture_output=True, text=True)
        for line in r.stdout.split("\n"):
            if line:
                w, h, tr = (int(v) for v in line.split())
                out[(w, h)] = tr
    return out


def test_geometry_is_the_header_the_kernels_use(geom_exe):
    src = open(os.path.join(ROOT, "localregneuralde.jl_amd", "csrc", "lrnde_conv.hip")).read()
    assert '#include "lrnde_conv_geom.hpp"' in src
    assert src.count("conv_strip_rows(") == 2   # the forward strips (strip_rows) and the weight-gradient strips
    assert "for (int tr = 1; tr <=" not in src   # no second copy of the loop
    pairs = [(r[0], r[1]) for r in G.GEOMETRIES] + [(w, h) for (w, h, _b, _l) in G.MULTI_STRIP]
    pairs += [(w, h) for w in range(4, 129, 4) for h in range(2, 41)]
    assert all(G.legal(w, h) for w, h in pairs)
    got = _strip_rows(geom_exe, pairs)
    assert len(got) == len(set(pairs))
    for (w, h) in pairs:
        TR, TP, MT, strips = G.geometry(w, h)
        assert got[(w, h)] == TR, (w, h)
        assert h % TR == 0 and TP == TR * w <= 128 and 1 <= MT <= 8 and strips * TR == h


def test_table_columns_are_the_restated_geometry():
    for (W, H, Bt, Be, TR, TP, MT, strips, _why) in G.GEOMETRIES:
        assert G.legal(W, H) and G.geometry(W, H) == (TR, TP, MT, strips), (W, H)
        assert Bt >= 1 and Be >= 1 and Bt * W * H >= 8      # train-mode statistics over at least 8 pixels
        assert W * H <= 744                                   # images stay small: a few launches each
        assert max(G.wgrad_lds_bytes(W, H).values()) <= G.WGRAD_LDS_LIMIT


def test_table_covers_what_it_claims():
    rows = G.GEOMETRIES
    ragged = {r[6] for r in rows if r[5] % 16 != 0}
    full = {r[6] for r in rows if r[5] % 16 == 0}
    # every instantiation with a partly filled last tile (MT = 4 too: TP = 52 at 52 x 3), and the ones no test of
    # tests/test_gpu_conv.py reaches with a full one
    assert ragged == set(range(1, 9))
    assert full >= {1, 2, 3, 5}
    assert sum(1 for r in rows if r[4] == 1 and r[7] >= 3) >= 3          # TR == 1 with an interior strip
    assert sum(1 for r in rows if 64 < r[0] < 128) >= 2
    by_wh = {(r[0], r[1]): r for r in rows}
    kinds = [by_wh[wh] for wh in G.EXTRA_ACT_ROWS]
    assert any(r[5] % 16 != 0 for r in kinds) and any(r[4] == 1 and r[7] >= 3 for r in kinds)
    assert set(G.EXTRA_ACTS) == {"tanh", "identity"}
    # the refusal line: 124 is the widest width whose 64 x 64 weight-gradient tiles fit, 128 is refused
    assert G.wgrad_lds_bytes(124, 3)["w2"] == 160640 and G.WGRAD_LDS_LIMIT - 160640 == 3200
    assert G.wgrad_lds_bytes(128, 2)["w2"] > G.WGRAD_LDS_LIMIT


def test_multi_strip_cases_make_the_intended_launches_loop():
    for (W, H, B, loops) in G.MULTI_STRIP:
        TR, TP, MT, strips = G.geometry(W, H)
        nstrips = B * strips
        assert nstrips > 256                       # k_bn_finalize_t: more partials than its 256 threads
        lds = G.wgrad_lds_bytes(W, H)
        for name in ("w3", "w2", "w1"):
            assert lds[name] <= G.WGRAD_LDS_LIMIT
            assert (nstrips > G.wgrad_max_workgroups(lds[name])) == (name in loops), (W, H, name, lds[name])
        assert B * W * H <= 20000                  # the oracle stays under a second
    assert G.wgrad_lds_bytes(68, 3)["w2"] == 88960 and G.geometry(68, 3)[0] == 1
    assert G.geometry(4, 2)[3] * 520 == 520 > 512
    # today's oracle-checked shapes never loop: the largest has 40 strips
    for (W, H, B) in ((32, 32, 2), (28, 28, 2), (16, 16, 3), (4, 32, 5)):
        assert B * G.geometry(W, H)[3] <= 40


def test_locate_names_strip_and_tile():
    err = np.zeros((2, 8, 7, 20)); err[1, 3, 5, 17] = 1.0
    assert G.locate(err, 20, 7) == (1, 3, 5, 17, 5, 1)           # TR = 1: strip = row, tile 17 // 16
    err = np.zeros((1, 8, 9, 12)); err[0, 7, 8, 11] = 2.0
    assert G.locate(err, 12, 9) == (0, 7, 8, 11, 0, 6)           # one strip of 108 pixels, the ragged seventh tile
    assert "ragged" in G.describe(err, 12, 9)


_CASES = G.all_cases() + [(W, H, B, "gelu", True) for (W, H, B, _l) in G.MULTI_STRIP] + [(4, 2, 520, "gelu", False)]


@pytest.mark.parametrize("W,H,B,act,train", _CASES)
def test_oracle_is_conditioned_at_every_case(W, H, B, act, train):
    """f-eval within 3e-6 of the output scale of the float64 restatement; VJP within 1e-5 per block of float64 autograd"""
    ref = G.reference(W, H, B, act, train)
    p, u, st, lam = ref["p"], ref["u"], ref["st"], ref["lam"]
    for t in (0.0, 0.613):
        f64 = torch_conv_field(u.reshape(B, -1), t, p, W, H, G.C, G.HC, act, train, st)
        mine = G.torch_field(torch.tensor(u.reshape(B, -1), dtype=torch.float64), torch.tensor(p, dtype=torch.float64), t,
                             W, H, act, train, st).numpy()
        assert np.abs(mine - f64).max() <= 1e-12 * np.abs(f64).max()   # the differentiable restatement is the same function
        err = np.abs(ref["rhs"][t].reshape(B, -1) - f64)
        d = float(err.max() / np.abs(f64).max())
        print(f"{W}x{H} B={B} {act} train={train} t={t}: oracle f-eval {d:.2e} of scale from float64")
        assert d <= 3e-6, G.describe(err, W, H)
    _f, dy64, gp64 = G.torch_vjp(u, p, 0.41, lam, W, H, act, train, st)
    ddy = float(np.abs(ref["dy"].reshape(B, -1) - dy64).max() / np.abs(dy64).max())
    blocks = G.block_errors(ref["gp"], gp64)
    print(f"{W}x{H} B={B} {act} train={train}: oracle vjp dy {ddy:.2e}, blocks " + " ".join(f"{k} {v:.2e}" for k, v in blocks.items()))
    assert ddy <= 1e-5
    for name, v in blocks.items():
        assert v <= 1e-5, name


def test_multi_strip_bars_are_recorded():
    """the float32-to-float64 distances behind the multi-strip parameter bars (module docstring of
    tests/test_gpu_conv_geometry.py): printed, and bounded so that a bar cannot silently become loose"""
    for (W, H, B, act, train) in [(W, H, B, "gelu", True) for (W, H, B, _l) in G.MULTI_STRIP] + [(4, 2, 520, "gelu", False)]:
        bars, d = G.multi_strip_bars(W, H, B, act, train)
        print(f"{W}x{H} B={B} train={train}: float32-vs-float64 " + " ".join(f"{k} {v:.2e}" for k, v in d.items()))
        for name in d:
            assert bars[name] == max(5e-5, 4 * d[name]) and bars[name] <= 2e-4, (name, d[name])
