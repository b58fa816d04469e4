"""The unit pack (nr_pack.cpp pack_fp32_units) and the kernel that runs it, without a GPU.

The batched fp32 tracer's unit form (nr_mlp16.h mlp64_fp32_units) issues one matrix instruction per
hidden input unit, units ascending, and skips the instruction of a unit whose activation is +0 in
every live lane.  Here: a chain with its +0 terms dropped equals the full chain once the bias is
added, the -0 corners included; every weight of plane_1 and of a 4-input network sits at its
documented position of the pack; the networks that must not take the form get no pack; the kernel's
registers and scratch; the new symbols.
"""
import ctypes

import numpy as np
import pytest

import cudaneuralrender_amd as nr
import depth_nets
import test_batch_ring_cpu as ring
import test_prune_cpu as prune

F = np.float32
PK_L0W, PK_L0B, PK_HID, PK_STRIDE = 0, 128, 160, 1056


def _skip_chain(ws, acts):
    """The kernel's chain: unit 0 always issued, a later unit only if its activation's bits are nonzero."""
    acc = prune._fma32(ws[0], acts[0], F(0.0))
    for w, a in zip(ws[1:], acts[1:]):
        if prune._bits(a) != 0:
            acc = prune._fma32(w, a, acc)
    return acc


# ---- chain exactness ------------------------------------------------------------------------

def test_dropping_plus_zero_terms_changes_no_activation():
    """Random chains with a third of the activations +0, weights of both signs: the chain with those
    terms dropped is the full chain bit for bit, and so is the clamped activation."""
    rng = np.random.default_rng(11)
    for n in range(60):
        ws = rng.standard_normal(32).astype(F)
        acts = (np.maximum(rng.standard_normal(32), 0) * 0.3).astype(F)
        acts[rng.choice(32, 11, replace=False)] = 0.0
        if n % 3 == 0:
            acts[0] = 0.0  # unit 0 dead: it is issued all the same, fma(w, +0, +0) = +0
        full, skip = prune._chain(ws, acts), _skip_chain(ws, acts)
        assert prune._bits(full) == prune._bits(skip)


def test_minus_zero_corners():
    """The corners tests/test_prune_cpu.py drives: a negative product below 2^-150 rounds the chain
    to -0; a dropped term fma(w > 0, +0, -0) would have turned it into +0, so the chains end as zeros
    of different sign, and the bias add (never -0) gives the same bits.  And a -0 or NaN activation
    has a nonzero bit pattern: it is issued, never skipped."""
    tiny_w, tiny_a = F(-2.0 ** -100), F(2.0 ** -60)
    for tail_act in (0.0, 0.375):
        ws = np.full(32, 0.5, F)
        ws[0] = tiny_w
        ws[13] = F(-0.25)
        acts = np.zeros(32, F)
        acts[0] = tiny_a
        acts[20] = F(tail_act)
        full, skip = prune._chain(ws, acts), _skip_chain(ws, acts)
        if tail_act == 0.0:
            assert prune._bits(full) == 0 and prune._bits(skip) == 0x80000000
        else:
            assert prune._bits(full) == prune._bits(skip)
        for b in (0.0, 1.5, -0.25, 2.0 ** -149):
            zf, zs = prune._add32(full, b), prune._add32(skip, b)
            assert prune._bits(zf) == prune._bits(zs), (tail_act, b)
            clamp = lambda z: min(max(z, F(0.0)), F(1.0))
            assert prune._bits(clamp(zf)) == prune._bits(clamp(zs))
    # the case the pack refuses: a bias of -0 keeps the sign of a zero chain
    assert prune._bits(prune._add32(F(0.0), F(-0.0))) != prune._bits(prune._add32(F(-0.0), F(-0.0)))
    # -0 is issued: with w < 0 it adds +0 to a -0 chain, exactly as the full chain does
    ws = np.array([tiny_w, -0.5, 0.5], F)
    acts = np.array([tiny_a, -0.0, 0.0], F)
    assert prune._bits(acts[1]) != 0
    assert prune._bits(_skip_chain(ws, acts)) == prune._bits(prune._chain(ws[:2], acts[:2])) == 0


# ---- the pack's layout ----------------------------------------------------------------------

def _scaled(dims, K, B):
    """The scaled weights the full pack holds, decoded from it (tests/test_prune_cpu.py _decode)."""
    P = nr.pack_fp32_pruned(list(dims), list(K), list(B), 0)
    assert P["clamp"] == 1
    nh = len(dims) - 3
    return prune._decode(P["full"], nh, False)


@pytest.mark.parametrize("name", ["plane_1", "four_inputs"])
def test_every_weight_at_its_documented_position(name):
    if name == "plane_1":
        dims, K, B = nr.read_keras_h5(nr.geometry_path("plane_1"))
    else:
        dims, K, B = depth_nets.cached_net(3, 4)
    dims, K, B = list(dims), list(K), list(B)
    nh, in0 = len(dims) - 3, dims[0]
    pack = nr.pack_fp32_units(dims, K, B)
    full = nr.pack_fp32_pruned(dims, K, B, 0)["full"]
    assert pack is not None and pack.size == full.size == PK_HID + nh * PK_STRIDE + 36
    K0, hid, biases, fin, fbias, s0 = _scaled(dims, K, B)
    bits = lambda a: np.asarray(a, F).view(np.uint32)
    # layer 0: [input 4][row 32], unscaled; 0 for the missing 4th input
    for kk in range(4):
        want = K[0][kk] if kk < in0 else np.zeros(32, F)
        assert np.array_equal(bits(pack[PK_L0W + 32 * kk:PK_L0W + 32 * kk + 32]), bits(want)), kk
        assert np.array_equal(bits(K0[kk]), bits(want))
    assert np.array_equal(bits(pack[PK_L0B:PK_L0B + 32]), bits(biases[0]))
    # hidden layer j: weight of (input unit k, row) at base + ((k >> 2) * 32 + row) * 4 + (k & 3)
    for j in range(nh):
        base = PK_HID + j * PK_STRIDE
        for k in range(32):
            idx = base + ((k >> 2) * 32 + np.arange(32)) * 4 + (k & 3)
            assert np.array_equal(bits(pack[idx]), bits(hid[j, k])), (j, k)
        assert np.array_equal(bits(pack[base + 1024:base + 1056]), bits(biases[j + 1])), j
    fo = PK_HID + nh * PK_STRIDE
    assert np.array_equal(bits(pack[fo:fo + 32]), bits(fin))
    assert bits(pack[fo + 32]) == bits(fbias) and bits(pack[fo + 33]) == bits(s0)
    # the scales are powers of two: every packed weight is the network's times one
    ratio = hid[0][K[1] != 0] / K[1][K[1] != 0]
    assert np.all(np.log2(ratio) == np.round(np.log2(ratio)))


def test_networks_that_get_no_unit_pack():
    dims, K, B = nr.read_keras_h5(nr.geometry_path("plane_1"))
    for bad in (np.nan, np.inf):
        K2 = [k.copy() for k in K]
        K2[3][5, 7] = bad
        assert nr.pack_fp32_units(dims, K2, B) is None, bad
    K2 = [k.copy() for k in K]
    K2[2][1, 1] = F(1e-30)  # the scaled pack refused (a weight below 2^-60)
    assert nr.pack_fp32_units(dims, K2, B) is None
    B2 = [b.copy() for b in B]
    B2[4][9] = F(-0.0)
    assert nr.pack_fp32_units(dims, K, B2) is None
    assert nr.pack_fp32_units(dims, K, B) is not None


# ---- the kernel's resources and the exports -------------------------------------------------

def test_batched_fp32_tracer_resources(tmp_path):
    r = ring.kernel_metadata(nr._lib.LIB_PATH, tmp_path, ring.BATCHED_FP32)
    print(r)
    assert r["vgpr_count"] + r["agpr_count"] <= 128, r
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r


def test_exports():
    L = ctypes.CDLL(nr._lib.LIB_PATH)
    for sym in ("nr_set_unit_skip", "nr_unit_skip_counts", "nr_pack_fp32_units"):
        assert hasattr(L, sym), sym
        assert sym in nr._lib.EXPORTS
    assert nr.lib().nr_abi_version() == 3
