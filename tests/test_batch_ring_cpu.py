"""The batched fp32 tracer's resources, from the code-object metadata of the built library.

The kernel holds one spare generated ray per lane in registers (nr_trace.hip, RREG) and must still
run 4 workgroups of 4 waves per CU: at most 128 VGPRs, no scratch, and at most a quarter of the
CU's 160 KB of LDS per workgroup with the flagship network's weights staged beside its static LDS.
"""
import os
import re
import shutil
import subprocess

import pytest

import cudaneuralrender_amd as nr
from cudaneuralrender_amd import _lib

BATCHED_FP32 = "_ZN2nr7k_traceILi0ELb0ELb0ELb1ELb0ELb0ELb1EEEvNS_10RenderArgsENS_7MlpArgsENS_9TraceArgsE"


def kernel_metadata(lib_path, tmp_path, symbol):
    """The metadata entry of one kernel of lib_path's gfx950 code objects, as {field: int}."""
    readelf, objdump = "/opt/rocm/lib/llvm/bin/llvm-readelf", "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not (os.path.exists(readelf) and os.path.exists(objdump)):
        pytest.skip("llvm-readelf / llvm-objdump not available")
    so = tmp_path / "libnr.so"
    shutil.copy(lib_path, so)
    subprocess.run([objdump, "--offloading", str(so)], cwd=tmp_path, check=True, capture_output=True)
    for p in sorted(p for p in tmp_path.iterdir() if "amdgcn" in p.name and "gfx950" in p.name):
        notes = subprocess.run([readelf, "--notes", str(p)], check=True, capture_output=True, text=True).stdout
        # one entry per kernel, from its first field (.agpr_count) to the next kernel's
        for kern in notes.split("  - .agpr_count:")[1:]:
            if re.search(r"^\s+\.name:\s+" + re.escape(symbol) + r"\s*$", kern, re.M):
                out = {k: int(v) for k, v in re.findall(r"^    \.(\w+):\s+(\d+)\s*$", kern, re.M)}
                out["agpr_count"] = int(kern.split()[0])
                return out
    raise AssertionError(f"{symbol} not in {lib_path}")


def fp32_pack_bytes(nh):
    """Dynamic LDS of an fp32 k_trace launch: the fp32 pack of a network with nh 32x32 hidden
    layers (nr_internal.h pk_floats: PK_HID + nh * PK_HID_STRIDE + 36 floats, padded to 16 bytes;
    nr_mlp16.h smem16_bytes)."""
    return ((160 + nh * (1024 + 32) + 36) * 4 + 15) // 16 * 16


def test_batched_fp32_tracer_fits_four_workgroups_per_cu(tmp_path):
    r = kernel_metadata(_lib.LIB_PATH, tmp_path, BATCHED_FP32)
    print(r)
    assert r["max_flat_workgroup_size"] == 256, r
    assert r["vgpr_count"] <= 128 and r["agpr_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    dims, _, _ = nr.read_keras_h5(nr.geometry_path("plane_1"))  # the flagship network
    assert list(dims) == [3] + [32] * 8 + [1]
    nh = len(dims) - 3  # of the len(dims) - 1 layers, those between the first and the last
    lds = r["group_segment_fixed_size"] + fp32_pack_bytes(nh)
    print("LDS per workgroup:", r["group_segment_fixed_size"], "+", fp32_pack_bytes(nh))
    assert lds <= 40960, (r["group_segment_fixed_size"], fp32_pack_bytes(nh))
