"""Register budget of the solo exact-bf16 scene kernels compiled for the canonical model (txp_x6.hip, Shape::Canon /
Shape::Canon32), read from the code-object metadata of the built library with the ROCm LLVM tools -- no GPU needed.

A folded layout must not buy its fewer instructions with spills: every Canon / Canon32 instantiation spills no more
VGPRs than the Generic build of the same kernel did before the fold (forward 4, backward 15), and fewer SGPRs than the
Generic build in the same library."""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "social_stgcnn_amd", "csrc", "libstgcnn_hip.so")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
VGPR_SPILL_BUDGET = {"txp_fwd_x6_kernel": 4, "txp_bwd_x6_kernel": 15}
SHAPES = {"0": "Generic", "1": "Canon", "2": "Canon32"}


def _tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else shutil.which(name)


def _code_objects(tmp_path):
    """gfx950 code objects of the library: its .hip_fatbin section holds one offload bundle per translation unit."""
    objcopy = _tool("llvm-objcopy")
    if objcopy is None or not os.path.exists(LIB):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    fatbin = tmp_path / "fatbin.bin"
    subprocess.run([objcopy, "--dump-section", ".hip_fatbin=%s" % fatbin, LIB], check=True, capture_output=True)
    data = fatbin.read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out = []
    start = data.find(magic)
    while start >= 0:
        (n_entries,) = struct.unpack_from("<Q", data, start + len(magic))
        q = start + len(magic) + 8
        for _ in range(n_entries):
            off, size, tlen = struct.unpack_from("<QQQ", data, q)
            q += 24
            triple = data[q:q + tlen].decode()
            q += tlen
            if triple.endswith("gfx950"):
                out.append(data[start + off:start + off + size])
        start = data.find(magic, start + 1)
    return out


def _kernel_metadata(tmp_path):
    readelf = _tool("llvm-readelf")
    if readelf is None:
        pytest.skip("needs llvm-readelf")
    meta = {}
    for k, co in enumerate(_code_objects(tmp_path)):
        path = tmp_path / ("co%d.o" % k)
        path.write_bytes(co)
        notes = subprocess.run([readelf, "--notes", str(path)], check=True, capture_output=True, text=True).stdout
        if "x6_kernel" not in notes:
            continue
        # one YAML map per kernel: '- .agpr_count' opens it, the keys follow in alphabetical order
        for entry in notes.split("  - .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", entry)
            if name is None:
                continue
            fields = dict(re.findall(r"\.(sgpr_spill_count|vgpr_spill_count):\s+(\d+)", entry))
            meta[name.group(1)] = {k: int(v) for k, v in fields.items()}
    return meta


def _solo_x6(meta):
    """{(kernel, WPB, BF, shape): metadata} of the solo x6 kernels (mangled: kernelILi<W>ELb<B>ELNS0_5ShapeE<S>EE)"""
    out = {}
    for name, m in meta.items():
        hit = re.search(r"(txp_(?:fwd|bwd)_x6_kernel)ILi(\d)ELb(\d)ELN\w*?5ShapeE(\d)E", name)
        if hit:
            out[(hit.group(1), int(hit.group(2)), int(hit.group(3)), SHAPES[hit.group(4)])] = m
    return out


def test_canonical_x6_kernels_keep_the_register_budget(tmp_path):
    solo = _solo_x6(_kernel_metadata(tmp_path))
    assert solo, "no solo x6 kernels found in the library's code objects"
    canon = [k for k in solo if k[3] != "Generic"]
    # Canon32 for both kernels, both storage formats and both workgroup sizes; Canon at least for fp32 storage
    for kern in VGPR_SPILL_BUDGET:
        for wpb in (4, 8):
            for bf in (0, 1):
                assert (kern, wpb, bf, "Canon32") in solo, (kern, wpb, bf)
                assert (kern, wpb, bf, "Generic") in solo, (kern, wpb, bf)
            assert (kern, wpb, 0, "Canon") in solo, (kern, wpb)
    for key in canon:
        kern, wpb, bf, shape = key
        m, g = solo[key], solo[(kern, wpb, bf, "Generic")]
        assert m["vgpr_spill_count"] <= VGPR_SPILL_BUDGET[kern], (key, m)
        assert m["vgpr_spill_count"] <= g["vgpr_spill_count"], (key, m, g)
        assert m["sgpr_spill_count"] < g["sgpr_spill_count"], (key, m, g)
