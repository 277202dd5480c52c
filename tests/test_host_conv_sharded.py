"""The batch-sharded conv handle's entry points, as far as a machine without a GPU can see them: the declarations in
include/lrnde.h (the boundary) and include/lrnde_hooks.h (the test hooks), the ctypes table, the exported symbols and the
arity of julia/LRNDEBackend.jl's ccalls.  What they compute is in tests/test_gpu_conv_sharded.py."""
import ctypes
import os
import re

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
