"""The unit pack under the kernel's prefetched LDS reads, without a GPU.

The batched fp32 tracer's unit form (nr_mlp16.h mlp64_fp32_units) reads its hidden weights four
units at a time (one 16-byte read per lane: units 4k .. 4k + 3 of the lane's row) and a layer's bias
as four 16-byte reads per lane, all from inline asm, one step ahead of their use.  Here: every weight
and bias of the five bundled networks and of a random one sits where those reads expect it (the
layout nr_internal.h documents); the farthest byte a read can touch, formed from the constants of
nr_internal.h and the offsets written in nr_mlp16.h, is inside the pack at every depth -- the read
ahead of the last layer's end included; and the built kernel keeps its registers and its LDS.
"""
import glob
import os
import re

import numpy as np
import pytest

import cudaneuralrender_amd as nr
import depth_nets
import test_batch_ring_cpu as ring
import test_prune_cpu as prune

F = np.float32
CSRC = os.path.join(os.path.dirname(os.path.abspath(nr.__file__)), "csrc")
GEOMETRIES = sorted(os.path.splitext(os.path.basename(p))[0]
                    for p in glob.glob(os.path.join(os.path.dirname(nr.geometry_path("plane_1")), "*.h5")))


def _constants():
    """PK_* of nr_internal.h, the byte offsets of the weight reads and the bias reads of nr_mlp16.h."""
    text = open(os.path.join(CSRC, "nr_internal.h")).read()
    c = {k: int(v) for k, v in re.findall(r"constexpr int (PK_\w+) = (\d+);", text)}
    m = re.search(r"constexpr int PK_HID_STRIDE = (\d+) \+ (\d+);", text)
    c["PK_HID_STRIDE"] = int(m.group(1)) + int(m.group(2))
    src = open(os.path.join(CSRC, "nr_mlp16.h")).read()
    body = src[src.index("__device__ __forceinline__ void units_wread"):src.index("// The batched fp32 tracer's MLP while M.pku is set")]
    c["wread"] = sorted({int(v) for v in re.findall(r"units_wread<(\d+)>\(", body)})
    c["bread"] = sorted({32 * int(q) + e for q in re.findall(r"units_bread<(\d+)>\(", body) for e in (0, 32)})
    return c


def test_constants_are_the_documented_layout():
    c = _constants()
    assert (c["PK_L0W"], c["PK_L0B"], c["PK_HID"], c["PK_HID_STRIDE"]) == (0, 128, 160, 1056)
    # eight reads of four units each, 32 rows of 16 bytes apart; the four quarters of a lane's bias
    assert c["wread"] == [512 * k for k in range(8)]
    assert c["bread"] == [0, 32, 64, 96]


def _network(name):
    if name == "random":
        dims, K, B = depth_nets.cached_net(5, 3)
    else:
        dims, K, B = nr.read_keras_h5(nr.geometry_path(name))
    return list(dims), list(K), list(B)


def test_five_bundled_networks():
    assert len(GEOMETRIES) == 5, GEOMETRIES


@pytest.mark.parametrize("name", GEOMETRIES + ["random"])
def test_every_read_finds_its_weights(name):
    """What lane (row r, half h) reads at the kernel's addresses is what the chain needs: the four
    weights (unit 4k + i -> row r) of hidden layer j at byte 4 (PK_HID + j STRIDE) + 512 k + 16 r, the
    bias of rows 8q + 4h .. + 3 at byte 4 (PK_HID + j STRIDE + 1024) + 16 h + 32 q."""
    c = _constants()
    dims, K, B = _network(name)
    nh = len(dims) - 3
    pack = nr.pack_fp32_units(dims, K, B)
    assert pack is not None and pack.size == c["PK_HID"] + nh * c["PK_HID_STRIDE"] + 36
    full = nr.pack_fp32_pruned(dims, K, B, 0)
    assert full["clamp"] == 1
    K0, hid, biases, fin, fbias, s0 = prune._decode(full["full"], nh, False)
    bits = lambda a: np.asarray(a, F).view(np.uint32)
    rows = np.arange(32)
    for j in range(nh):
        base = 4 * (c["PK_HID"] + j * c["PK_HID_STRIDE"])
        for k, off in enumerate(c["wread"]):
            for i in range(4):
                at = (base + off + 16 * rows) // 4 + i
                assert np.array_equal(bits(pack[at]), bits(hid[j, 4 * k + i])), (j, k, i)
        for h in range(2):
            for q, off in enumerate(c["bread"]):
                at = (base + 4 * 1024 + 16 * h + off) // 4
                assert np.array_equal(bits(pack[at:at + 4]), bits(biases[j + 1][8 * q + 4 * h:8 * q + 4 * h + 4])), (j, h, q)
    # layer 0's bias goes through the same four reads
    for h in range(2):
        for q, off in enumerate(c["bread"]):
            at = (4 * c["PK_L0B"] + 16 * h + off) // 4
            assert np.array_equal(bits(pack[at:at + 4]), bits(biases[0][8 * q + 4 * h:8 * q + 4 * h + 4])), (h, q)
    fo = c["PK_HID"] + nh * c["PK_HID_STRIDE"]
    assert np.array_equal(bits(pack[fo:fo + 32]), bits(fin))
    assert bits(pack[fo + 32]) == bits(fbias) and bits(pack[fo + 33]) == bits(s0)


@pytest.mark.parametrize("nh", [0, 1, 2, 7, 8])
def test_no_read_leaves_the_pack(nh):
    """The farthest byte of any read the kernel can form.  The weight address starts at the first
    hidden layer (layer 0's weights when there is none) and advances by a layer only while another
    layer follows, so the read issued during the last layer's epilogue repeats that layer's first
    weights; the bias address is layer 0's, then hidden layer j's for j < nh."""
    c = _constants()
    floats = c["PK_HID"] + nh * c["PK_HID_STRIDE"] + 36
    w_bases = [4 * (c["PK_HID"] + j * c["PK_HID_STRIDE"]) for j in range(nh)] or [0]
    # (without a hidden layer only the read of offset 0 is issued)
    w_offs = c["wread"] if nh else [0]
    w_end = max(w_bases) + 16 * 31 + max(w_offs) + 16
    b_bases = [4 * c["PK_L0B"]] + [4 * (c["PK_HID"] + j * c["PK_HID_STRIDE"] + 1024) for j in range(nh)]
    b_end = max(b_bases) + 16 * 1 + max(c["bread"]) + 16
    print(nh, "pack bytes", 4 * floats, "weight reads end", w_end, "bias reads end", b_end)
    assert w_end <= 4 * floats and b_end <= 4 * floats
    assert min(w_bases) >= 0 and all(b % 16 == 0 for b in w_bases + b_bases)  # 16-byte reads, aligned


def test_batched_fp32_tracer_resources(tmp_path):
    r = ring.kernel_metadata(nr._lib.LIB_PATH, tmp_path, ring.BATCHED_FP32)
    print(r)
    assert r["vgpr_count"] + r["agpr_count"] <= 128, r
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    dims, _, _ = nr.read_keras_h5(nr.geometry_path("plane_1"))
    lds = r["group_segment_fixed_size"] + ring.fp32_pack_bytes(len(dims) - 3)
    print("LDS per workgroup:", lds)
    assert lds <= 40960, lds
