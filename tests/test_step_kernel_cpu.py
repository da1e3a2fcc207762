"""Register budget of the one-launch scene kernel of the training step (txp_x6.hip, txp_step_x6_kernel: forward and backward
of a Canon32 scene in one wave), read from the code-object metadata of the built library -- no GPU needed.

The kernel is the two solo scene functions one behind the other, so it may cost no more than they do: no spilled VGPR,
no scratch memory, and no more spilled SGPRs than the solo Canon32 forward and backward kernels of the same library
(four waves per workgroup, same storage format) spill together."""
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "social_stgcnn_amd", "csrc", "libstgcnn_hip.so")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
FIELDS = ("sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size", "vgpr_count", "sgpr_count")


def _tool(name):
    path = os.path.join(LLVM, name)
    return path if os.path.exists(path) else shutil.which(name)


def _x6_metadata(tmp_path):
    """{kernel name: {field: value}} of every kernel of the code object that holds the x6 kernels"""
    objcopy, readelf = _tool("llvm-objcopy"), _tool("llvm-readelf")
    if objcopy is None or readelf is None or not os.path.exists(LIB):
        pytest.skip("needs the built library and the ROCm LLVM tools")
    fatbin = tmp_path / "fatbin.bin"
    subprocess.run([objcopy, "--dump-section", ".hip_fatbin=%s" % fatbin, LIB], check=True, capture_output=True)
    data = fatbin.read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    meta = {}
    start, k = data.find(magic), 0
    while start >= 0:
        (n_entries,) = struct.unpack_from("<Q", data, start + len(magic))
        q = start + len(magic) + 8
        for _ in range(n_entries):
            off, size, tlen = struct.unpack_from("<QQQ", data, q)
            q += 24
            triple = data[q:q + tlen].decode()
            q += tlen
            if not triple.endswith("gfx950"):
                continue
            path = tmp_path / ("co%d.o" % k)
            k += 1
            path.write_bytes(data[start + off:start + off + size])
            notes = subprocess.run([readelf, "--notes", str(path)], check=True, capture_output=True, text=True).stdout
            if "txp_step_x6_kernel" not in notes:
                continue
            for entry in notes.split("  - .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", entry)
                if name is not None:
                    found = dict(re.findall(r"\.(%s):\s+(\d+)" % "|".join(FIELDS), entry))
                    meta[name.group(1)] = {f: int(v) for f, v in found.items()}
        start = data.find(magic, start + 1)
    return meta


def test_step_kernel_keeps_the_register_budget(tmp_path):
    meta = _x6_metadata(tmp_path)
    step, solo = {}, {}
    for name, m in meta.items():
        hit = re.search(r"txp_step_x6_kernelILi(\d)ELb(\d)E", name)
        if hit:
            step[(int(hit.group(1)), int(hit.group(2)))] = m
        hit = re.search(r"txp_(fwd|bwd)_x6_kernelILi(\d)ELb(\d)ELN\w*?5ShapeE2E", name)       # (Shape 2 = Canon32)
        if hit:
            solo[(hit.group(1), int(hit.group(2)), int(hit.group(3)))] = m
    assert (4, 0) in step, "the fp32-storage one-launch scene kernel is missing from the library: %s" % sorted(step)
    for (wpb, bf), m in sorted(step.items()):
        f, b = solo[("fwd", wpb, bf)], solo[("bwd", wpb, bf)]
        print("txp_step_x6_kernel<%d, %d>: %s   solo forward: %s   solo backward: %s" % (wpb, bf, m, f, b))
        assert m["vgpr_spill_count"] == 0, (wpb, bf, m)
        assert m["private_segment_fixed_size"] == 0, (wpb, bf, m)
        assert m["sgpr_spill_count"] <= f["sgpr_spill_count"] + b["sgpr_spill_count"], (wpb, bf, m, f, b)
        assert m["vgpr_count"] <= 256, (wpb, bf, m)


def test_stamp_offsets_exist_only_in_the_diagnostic_build():
    """stg_model_fwd_stamps_offset / stg_model_bwd_stamps_offset (what tools/stamps_x6.py reads the stamps by): the shipped
    library writes no stamps and says so; bad sizes are the size queries' errors"""
    import ctypes
    from social_stgcnn_amd import _lib, ops
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    d = ctypes.byref(ops.make_desc(1, 5, 2, 5, 8, 12, 3, 2, False, True))
    if not _lib.DIAG:
        assert L.stg_model_fwd_stamps_offset(d, 2048, 32) == _lib.EUNSUPPORTED
        assert L.stg_model_bwd_stamps_offset(d, 2048, 32) == _lib.EUNSUPPORTED
    assert L.stg_model_fwd_stamps_offset(d, 2048, 0) == -1
    assert L.stg_model_bwd_stamps_offset(d, 0, 32) == -1
