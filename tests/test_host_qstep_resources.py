"""The register form of the step kernel, k_step_q<*, 1>, has to fit the register file without help: at most 256 VGPRs
(two waves per SIMD), no spilled VGPR and no private segment.  Its issue schedule (csrc/lrnde_qsched.hpp) keeps up to
twelve ring quads busy where the closed form kept nine, and how many it may keep in which f-eval (LRNDE_QCAP, LRNDE_QWRAP)
was derived from what one compiler's register allocator leaves: another compiler can turn the same source into a kernel
that spills, silently.  This reads the kernels' metadata out of the gfx950 code objects of the built library, so the
build that is tested and shipped is the one that is checked.  If it fails, re-derive the caps (lower the late f-evals
first: profiles/qsched/resource_usage.txt)."""
import os
import re
import shutil
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "localregneuralde.jl_amd", "liblrnde.so")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    p = shutil.which(name)
    assert p, f"{name} not found (ROCm's llvm tools)"
    return p


def _step_kernels(tmp_path):
    """{mangled name: {field: int}} of every k_step_q instantiation in the library's gfx950 code objects"""
    fat = tmp_path / "fat.bin"
    subprocess.run([_tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", LIB, str(tmp_path / "copy.so")], check=True)
    d = fat.read_bytes()
    out = {}
    for m in re.finditer(MAGIC, d):   # one bundle per translation unit: [magic][n][offset, size, len, triple]...
        p0 = m.start()
        n, = struct.unpack_from("<Q", d, p0 + len(MAGIC))
        o = p0 + len(MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", d, o)
            triple = d[o + 24:o + 24 + tl].decode()
            o += 24 + tl
            if "gfx950" not in triple or size == 0:
                continue
            co = tmp_path / "co.o"
            co.write_bytes(d[p0 + off:p0 + off + size])
            notes = subprocess.run([_tool("llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout
            for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                if "k_step_qILb" in name:
                    out[name] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1))
                                 for k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    return out


def test_register_form_of_the_step_kernel_fits_without_spill(tmp_path):
    ks = _step_kernels(tmp_path)
    reg = {n: v for n, v in ks.items() if "ELi1E" in n}   # k_step_q<false, 1>, k_step_q<true, 1>
    assert len(reg) == 2, sorted(ks)
    for n, v in reg.items():
        print(n, v)
        assert v["vgpr_count"] <= 256, (n, v)
        assert v["vgpr_spill_count"] == 0, (n, v)
        assert v["private_segment_fixed_size"] == 0, (n, v)
