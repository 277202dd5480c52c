"""The batch-sharded conv handle's entry points, as far as a machine without a GPU can see them: the declarations in
include/lrnde.h (the boundary) and include/lrnde_hooks.h (the test hooks), the ctypes table, the exported symbols and the
arity of julia/LRNDEBackend.jl's ccalls.  What they compute is in tests/test_gpu_conv_sharded.py and
tests/test_gpu_conv_sharded_envelope.py; the conditions the latter selects its cases by are asserted here on the oracle."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BOUNDARY = {"lrnde_conv_comm_init": 4, "lrnde_conv_comm_destroy": 1, "lrnde_conv_comm_count": 3}
HOOKS = {"lrnde_conv_comm_init_local": 3, "lrnde_conv_comm_stats": 3}


def _decls(header):
    """name -> number of parameters, of every function declared in the header"""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
            for m in re.finditer(r"\b(lrnde_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt)}


def test_boundary_declares_the_conv_communicator_entry_points():
    decl = _decls("lrnde.h")
    for name, n in BOUNDARY.items():
        assert decl.get(name) == n, (name, decl.get(name))
    txt = open(os.path.join(ROOT, "include", "lrnde.h")).read()
    assert re.search(r"int lrnde_conv_comm_init\(lrnde_conv\* c, const void\* uid, int32_t rank, int32_t nranks\);", txt)
    assert re.search(r"int lrnde_conv_comm_count\(lrnde_conv\* c, int32_t\* nranks_host, int32_t\* kind_host\);", txt)


def test_hooks_are_declared_outside_the_boundary():
    hooks, boundary = _decls("lrnde_hooks.h"), _decls("lrnde.h")
    for name, n in HOOKS.items():
        assert hooks.get(name) == n, (name, hooks.get(name))
        assert name not in boundary, f"{name} is a test hook: it does not belong in include/lrnde.h"
    for name in BOUNDARY:
        assert name not in hooks


def test_ctypes_table_binds_them_with_the_header_arity():
    import lrnde_amd  # noqa: F401
    from localregneuralde_jl_amd import _lib
    table = {n: (res, args) for n, res, args in _lib.SYMBOLS}
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name, n in {**BOUNDARY, **HOOKS}.items():
        assert name in table, f"{name} is missing from _lib.SYMBOLS"
        assert table[name][0] is ctypes.c_int and len(table[name][1]) == n, name
        assert hasattr(raw, name), f"{name} is not exported by liblrnde.so"
    assert table["lrnde_conv_comm_stats"][1][1:] == [ctypes.POINTER(ctypes.c_uint64)] * 2


def test_julia_wrappers_call_them_with_the_header_arity():
    src = open(os.path.join(ROOT, "julia", "LRNDEBackend.jl")).read()
    calls = dict(re.findall(r"ccall\(\(:(lrnde_conv_comm_\w+), lib\), Cint,\s*\((.*?)\),\s*\n?", src, flags=re.S))
    assert set(calls) == set(BOUNDARY), sorted(calls)
    for name, types in calls.items():
        n = len([t for t in types.split(",") if t.strip()])
        assert n == BOUNDARY[name], (name, types)


class _RecordingLib:
    """stands in for the loaded library: every entry point returns LRNDE_OK and is written down with its handle"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args[0] if args else None))
            return 0
        return fn


def test_python_dispatches_on_the_handle_type(monkeypatch):
    """sharding.init_comm / LocalComm.join / LocalComm.close call the conv entry points for a ConvHandle and the MLP
    ones for any other handle (the calls themselves are recorded; what they compute is the GPU tests' business)"""
    import types
    import lrnde_amd  # noqa: F401
    from localregneuralde_jl_amd import conv, sharding
    rec = _RecordingLib()
    monkeypatch.setattr(sharding, "L", types.SimpleNamespace(lib=rec, LrndeError=RuntimeError))

    def fake(cls, ctx):
        h = cls.__new__(cls)
        h._ctx = ctx
        h._chk = lambda rc: None
        return h

    hc = fake(conv.ConvHandle, "conv-ctx")
    hm = fake(type("MlpLike", (), {}), "mlp-ctx")
    sharding.init_comm(hc, 0, 1)
    sharding.init_comm(hm, 0, 1)
    lc = sharding.LocalComm(2)
    lc._lc = ctypes.c_void_p(1)   # the stand-in creates nothing: any non-null rendezvous pointer
    lc.join(hc, 0)
    lc.join(hm, 1)
    lc.close()
    hc._ctx = hm._ctx = None   # nothing real to destroy
    by_handle = {ctx: [n for n, a in rec.calls if a == ctx] for ctx in ("conv-ctx", "mlp-ctx")}
    assert by_handle["conv-ctx"] == ["lrnde_conv_comm_init", "lrnde_conv_comm_init_local", "lrnde_conv_comm_destroy"]
    assert by_handle["mlp-ctx"] == ["lrnde_comm_init", "lrnde_comm_init_local", "lrnde_comm_destroy"]
    assert callable(conv.ConvHandle.comm_count) and callable(conv.ConvHandle.comm_stats)


# ---- what tests/test_gpu_conv_sharded_envelope.py selects its cases by, asserted on the oracle alone ------------------
# (tests/conv_sharded_cases.py holds the recipes; a changed seed or recipe must fail here, not quietly change a GPU case)
def test_envelope_long_list_shapes_take_a_second_trip():
    """260 images @ 8x8 are 260 workgroups per rank (one strip per image), past the 256 threads of k_bn_rank_sums; the stem
    and head shapes give two blocks of 256 pixels per rank, the second ragged or full, and 260 blocks"""
    import conv_geometry_cases as G
    import conv_sharded_cases as S
    R, Bl, W, H = S.LONG_LIST
    assert G.geometry(W, H)[3] == 1 and Bl * G.geometry(W, H)[3] == 260 > 256
    blocks = {k: (-(-Bl * W * H // 256), (Bl * W * H) % 256) for k, (R, Bl, W, H) in S.STEM_SHAPES.items()}
    assert blocks == {"2x3@12x8": (2, 32), "3x2@16x16": (2, 0), "2x65@32x32": (260, 0)}


def test_envelope_test_mode_case_is_the_one_the_issue_names():
    import conv_sharded_cases as S
    bo = S.oracle_node_backward(S.TEST_MODE_CASE)
    assert bo["retcode"] == 0 and S.step_counts(bo) == (6, 0, 12, 0)
    ro = S.oracle_solve(S.TEST_MODE_CASE)
    assert ro["retcode"] == 0 and (ro["stats"]["naccept"], ro["stats"]["nreject"]) == (6, 0)
    assert not S.at_threshold(ro["trace"]) and len(ro["trace"]) == 6
    p, u, st = S._inputs(8, 8, 4, 41, False, 1.5)
    assert st is not None and not np.array_equal(st, S.BN0), "test mode runs on random running statistics"


def test_envelope_backward_cases_take_the_expected_steps_with_margin():
    import conv_sharded_cases as S
    for name, (case, expect) in S.BACKWARD_CASES.items():
        bo = S.oracle_node_backward(case)
        assert bo["retcode"] == 0 and S.step_counts(bo) == expect, (name, S.step_counts(bo))
        ro = S.oracle_solve(case)
        assert len(ro["trace"]) == expect[0] + expect[1] and not S.at_threshold(ro["trace"]), name
    import conv_geometry_cases as G
    assert G.geometry(16, 16)[3] == 2, "16x16: two strips per image"
    # 12x8 is one strip of 96 pixels per image: the MT = 6 instantiation (8x8 runs MT = 4, 16x16 MT = 8), three images
    # per rank.  Its strip fills its six tiles: what is ragged at this shape is the stem's and head's last 256-pixel block.
    assert G.geometry(12, 8) == (8, 96, 6, 1)


def test_envelope_stop_cases_stop_the_oracle_as_stated():
    import conv_sharded_cases as S
    R, Bl, W, H, seed, scale, tol = S.STOP_CASE
    B = R * Bl
    # NaN: one pixel of the last image; in test mode it stays inside that image, so rank 0's shard and f-eval are finite
    p, u, st, train, maxiters = S.stop_inputs("nan")
    assert not train and np.isfinite(u[:B - 1]).all() and np.isnan(u[B - 1]).sum() == 1
    f = S._field(W, H, p, st, train=False).rhs(u.reshape(B, -1), 0.0).reshape(u.shape)
    assert np.isfinite(f[:B - 1]).all() and np.isnan(f[B - 1]).any()
    o = S.oracle_stop("nan")
    so = o["solve"]["stats"]
    assert o["solve"]["retcode"] == 3 and o["fwd"]["retcode"] == 3
    assert (so["iters"], so["nf"], so["naccept"], so["nreject"]) == (1, 9, 0, 0)
    # maxiters
    p, u, st, train, maxiters = S.stop_inputs("maxiters")
    assert train and maxiters == 3 and np.isfinite(u).all()
    o = S.oracle_stop("maxiters")
    so = o["solve"]["stats"]
    assert o["solve"]["retcode"] == 1 and o["fwd"]["retcode"] == 1
    assert (so["naccept"], so["nreject"], so["iters"]) == (3, 0, 4)


def test_envelope_eight_rank_step_is_truncation_error():
    """the eight-rank case's Tsit5 step is large enough that its EEst is truncation error, not fp32 cancellation noise
    (the condition test_conv_init_dt_and_step_match_oracle puts on its own step before it holds EEst to 5e-3)"""
    import conv_sharded_cases as S
    dt_o, k1_o, so = S.eight_ranks_step_ref()
    assert float(so["eest"]) > 1e-2 and np.isfinite(so["u"]).all() and float(dt_o) > 0


def test_envelope_exchange_formula_gives_the_documented_counts():
    """an adjoint attempt is 43 / 31 exchanges, and the node_forward it quotes (42 f-evals: five attempts)
    issues 90"""
    import conv_sharded_cases as S
    one = dict(naccept=1, nreject=0)
    none = dict(naccept=0, nreject=0)
    for train, per in ((True, 43), (False, 31)):
        assert S.exchanges_adjoint(one, "none", 0.0, train) - S.exchanges_adjoint(none, "none", 0.0, train) == per
    assert S.exchanges_node_forward(dict(naccept=5, nreject=0), "unbiased", True) == 90
    assert S.exchanges_node_forward(dict(naccept=4, nreject=1), "unbiased", False) == 2 + 5 + 2 + 1
    assert S.exchanges_node_forward(dict(naccept=5, nreject=0), "none", True) == 6 + 5 * 13
