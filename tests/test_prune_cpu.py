"""The pruned fp32 pack (nr_pack.cpp pack_fp32_16_pruned) and the kernel that runs it, without a GPU.

The batched fp32 tracer skips the k-steps of hidden units that fire nowhere in the marched volume
(nr_mlp16.h mlp16_fp32_pruned).  Here: the pruned order of every bundled network and of a dense
random one is a permutation with the live units ascending and a multiple of 4 candidates behind
them; the pruned pack holds the full pack's values under that permutation; networks that must not
be pruned are not; the exactness argument's corner (a chain that is -0 where a candidate's term is
dropped) against the reference form of the chain; and the kernel's registers, scratch and LDS.
"""
import fractions
import functools

import numpy as np
import pytest

import cudaneuralrender_amd as nr
import depth_nets
import test_batch_ring_cpu as ring

F = np.float32
BUNDLED = ["plane_1", "car_1", "plane_2", "plane_3", "3a3d4a90a2db90b4203936772104a82d.obj"]
PK_HID, PK_STRIDE = 160, 1056


@functools.lru_cache(maxsize=None)
def _net(name):
    if name == "dense":
        dims, K, B = depth_nets.cached_net(6, 3)
        return list(dims), list(K), list(B)
    return nr.read_keras_h5(nr.geometry_path(name))


@functools.lru_cache(maxsize=None)
def _packs(name, mode):
    dims, K, B = _net(name)
    return nr.pack_fp32_pruned(dims, K, B, mode)


def _decode(pack, nh, final_by_position):
    """(K0 [4][32], hidden [nh][32 in][32 out], biases [nh + 1][32], final [32], final bias, scale)
    of a pack in position space: position 4k + g = register k of lane group g (the last ReLU layer
    of the full pack: 8g + k)."""
    def out_pos(mt, i, fin):
        gp, rp = i >> 2, i & 3
        return 8 * gp + 4 * mt + rp if fin else 16 * mt + 4 * rp + gp

    def reg_pos(g, k, fin):
        return 8 * g + k if fin else 4 * k + g

    K0 = np.zeros((4, 32), F)
    for mt in range(2):
        for lane in range(64):
            K0[lane >> 4, out_pos(mt, lane & 15, nh == 0 and not final_by_position)] = pack[mt * 64 + lane]
    biases = np.zeros((nh + 1, 32), F)
    for g in range(4):
        for k in range(8):
            biases[0, reg_pos(g, k, nh == 0 and not final_by_position)] = pack[128 + g * 8 + k]
    hid = np.zeros((nh, 32, 32), F)
    for j in range(nh):
        fin = j == nh - 1 and not final_by_position
        base = PK_HID + j * PK_STRIDE
        for st in range(8):
            for mt in range(2):
                m = 2 * st + mt
                for lane in range(64):
                    hid[j, 4 * st + (lane >> 4), out_pos(mt, lane & 15, fin)] = pack[base + ((m >> 2) * 64 + lane) * 4 + (m & 3)]
        for g in range(4):
            for k in range(8):
                biases[j + 1, reg_pos(g, k, fin)] = pack[base + 1024 + g * 8 + k]
    fo = PK_HID + nh * PK_STRIDE
    return K0, hid, biases, pack[fo:fo + 32].copy(), pack[fo + 32], pack[fo + 33]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", BUNDLED + ["dense"])
def test_order_and_weights(name, mode):
    dims, _, _ = _net(name)
    nh = len(dims) - 3
    P = _packs(name, mode)
    assert P["clamp"] == 1 and P["pruned"] is not None
    cand, ks, order = P["cand"], P["ks"], P["order"]
    print(name, mode, "candidates", cand.tolist(), "k-steps", ks.tolist())
    assert len(cand) == nh + 1
    for l in range(nh + 1):
        c = int(cand[l])
        assert c % 4 == 0 and 0 <= c <= 16 and ks[l] == (32 - c) // 4
        assert sorted(order[l].tolist()) == list(range(32))
        live = order[l][:32 - c].tolist()
        assert live == sorted(live)
        if mode == 2:
            assert c == 4 and sorted(order[l][28:].tolist()) == [28, 29, 30, 31]
    # the full pack in unit space (its positions are units), the pruned pack through the order
    K0, hid, bias, fin, fb, sc = _decode(P["full"], nh, False)
    Kp0, hidp, biasp, finp, fbp, scp = _decode(P["pruned"], nh, True)
    assert fb.tobytes() == fbp.tobytes() and sc.tobytes() == scp.tobytes()
    assert np.array_equal(Kp0.view(np.uint32), K0[:, order[0]].view(np.uint32))
    assert np.array_equal(biasp[0].view(np.uint32), bias[0][order[0]].view(np.uint32))
    for j in range(nh):
        want = hid[j][order[j]][:, order[j + 1]]
        assert np.array_equal(hidp[j].view(np.uint32), want.view(np.uint32)), j
        assert np.array_equal(biasp[j + 1].view(np.uint32), bias[j + 1][order[j + 1]].view(np.uint32)), j
    assert np.array_equal(finp.view(np.uint32), fin[order[nh]].view(np.uint32))


def test_mode_0_is_the_identity():
    P = _packs("plane_1", 0)
    assert P["cand"].sum() == 0 and (P["ks"] == 8).all()
    assert (P["order"] == np.arange(32)).all()


def test_selection_is_deterministic_and_finds_candidates():
    """The flagship network has never-firing units in its last layers; the choice is a function of
    the network alone (fixed sample)."""
    dims, K, B = _net("plane_1")
    a = nr.pack_fp32_pruned(dims, K, B, 1)
    b = _packs("plane_1", 1)
    assert np.array_equal(a["order"], b["order"]) and np.array_equal(a["cand"], b["cand"])
    assert a["cand"].sum() >= 8


def _no_candidates(P):
    return P["pruned"] is None or (P["cand"].sum() == 0 and (P["ks"] == 8).all())


def test_networks_that_are_not_pruned():
    dims, K, B = _net("plane_1")
    for bad in (np.nan, np.inf):
        K2 = [k.copy() for k in K]
        K2[3][5, 7] = bad
        assert _no_candidates(nr.pack_fp32_pruned(dims, K2, B, 1)), bad
        assert _no_candidates(nr.pack_fp32_pruned(dims, K2, B, 2)), bad
    # 4 inputs
    d4, K4, B4 = depth_nets.cached_net(3, 4)
    P = nr.pack_fp32_pruned(list(d4), list(K4), list(B4), 1)
    assert P["clamp"] == 1 and _no_candidates(P)
    assert _no_candidates(nr.pack_fp32_pruned(list(d4), list(K4), list(B4), 2))
    # the scaled pack refused (a weight below 2^-60): no pruned pack at all
    K2 = [k.copy() for k in K]
    K2[2][1, 1] = F(1e-30)
    P = nr.pack_fp32_pruned(dims, K2, B, 1)
    assert P["clamp"] == 0 and P["pruned"] is None
    # a bias of -0: the exactness argument below needs c + b to lose the sign of a zero chain
    B2 = [b.copy() for b in B]
    B2[4][9] = F(-0.0)
    assert _no_candidates(nr.pack_fp32_pruned(dims, K, B2, 2))


# ---- the exactness argument's corner -------------------------------------------------------

def _round32(q, zero_sign):
    """The exact rational q rounded to f32 (RNE); an exact zero takes zero_sign."""
    if q == 0:
        return F(-0.0) if zero_sign else F(0.0)
    with np.errstate(under="ignore"):
        v = F(float(q))  # f64 holds every case used here exactly or far from an f32 tie
    if v == 0:
        return F(-0.0) if q < 0 else F(0.0)
    return v


def _fma32(w, a, c):
    w, a, c = F(w), F(a), F(c)
    psign = bool(np.signbit(w)) != bool(np.signbit(a))
    if w == 0 or a == 0:
        if c != 0:
            return c
        return F(-0.0) if (psign and np.signbit(c)) else F(0.0)  # (+-0) + (+-0): -0 only for two -0
    q = fractions.Fraction(float(w)) * fractions.Fraction(float(a)) + fractions.Fraction(float(c))
    return _round32(q, False)  # an exact cancellation gives +0


def _add32(x, y):
    x, y = F(x), F(y)
    if x == 0 and y == 0:
        return F(-0.0) if (np.signbit(x) and np.signbit(y)) else F(0.0)
    return _round32(fractions.Fraction(float(x)) + fractions.Fraction(float(y)), False)


def _chain(ws, acts):
    acc = F(0.0)
    for w, a in zip(ws, acts):
        acc = _fma32(w, a, acc)
    return acc


def _bits(v):
    return int(np.asarray(v, F).view(np.uint32))


def test_minus_zero_chain_corner():
    """A negative product below 2^-150 rounds a +0 chain to -0.  In the original order a candidate's
    term fma(w, +0, -0) with w > 0 then gives +0, while the pruned chain (live units only) stays -0:
    the chains differ in the sign of a zero.  The bias add maps both to the same bits unless the
    bias is -0 (which the pack refuses), so the activation -- fmaxf(z, 0) in the reference form,
    the clamp to [0, 1] in the kernel -- is the same, bit for bit."""
    tiny_w, tiny_a = F(-2.0 ** -100), F(2.0 ** -60)  # product -2^-160: rounds to -0
    assert _bits(_fma32(tiny_w, tiny_a, 0.0)) == 0x80000000
    # units 0..31: unit 0 live with the tiny product, candidates at 1, 5, 9, 13 (activation +0, weights
    # of both signs), the other live units at +0 too, or one of them nonzero
    cand = [1, 5, 9, 13]
    for tail_act in (0.0, 0.375):
        ws = np.full(32, -0.5, F)  # live units at +0 add -0: a -0 chain stays -0
        ws[0] = tiny_w
        ws[cand] = F(0.5)          # a candidate's +0 product turns it into +0
        ws[13] = F(-0.25)
        acts = np.zeros(32, F)
        acts[0] = tiny_a
        acts[20] = F(tail_act)
        full = _chain(ws, acts)
        live = [u for u in range(32) if u not in cand]
        pruned = _chain(ws[live], acts[live])
        if tail_act == 0.0:
            assert _bits(full) == 0 and _bits(pruned) == 0x80000000  # the corner: zeros of different sign
        else:
            assert _bits(full) == _bits(pruned)
        for b in (0.0, 1.5, -0.25, 2.0 ** -149):
            zf, zp = _add32(full, b), _add32(pruned, b)
            assert _bits(zf) == _bits(zp), (tail_act, b)
            ref = zf if zf > 0 else F(0.0)                       # fmaxf(z, 0): z is never -0 here
            assert not (zf == 0 and np.signbit(zf))
            clamp = min(max(zp, F(0.0)), F(1.0)) if zp == zp else F(0.0)
            if ref <= 1:
                assert _bits(ref) == _bits(clamp), (tail_act, b)
    # and the case the pack refuses: with a bias of -0 the two pre-activations do differ
    assert _bits(_add32(F(0.0), F(-0.0))) != _bits(_add32(F(-0.0), F(-0.0)))


def test_leading_and_interleaved_zero_terms_leave_the_chain_alone():
    """The general step of the argument on random chains: dropping terms whose activation is +0
    changes no bit of a chain that never passes through -0 (weights of both signs, f32 fmaf)."""
    rng = np.random.default_rng(5)
    for _ in range(50):
        ws = rng.standard_normal(32).astype(F)
        acts = np.maximum(rng.standard_normal(32), 0).astype(F) * F(0.3)
        dead = rng.choice(32, 8, replace=False)
        acts[dead] = 0.0
        live = [u for u in range(32) if u not in set(dead.tolist())]
        assert _bits(_chain(ws, acts)) == _bits(_chain(ws[live], acts[live]))


# ---- the kernel's resources -----------------------------------------------------------------

def test_batched_fp32_tracer_resources(tmp_path):
    """As tests/test_batch_ring_cpu.py: 128 VGPRs, no AGPRs, no scratch, and the flagship network's
    pack (the pruned one has the full one's size) beside the static LDS within a quarter of a CU's."""
    r = ring.kernel_metadata(nr._lib.LIB_PATH, tmp_path, ring.BATCHED_FP32)
    print(r)
    assert r["vgpr_count"] <= 128 and r["agpr_count"] == 0, r
    assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r
    P = _packs("plane_1", 1)
    assert P["pruned"].size == P["full"].size
    nh = len(_net("plane_1")[0]) - 3
    assert ring.fp32_pack_bytes(nh) == (P["full"].size * 4 + 15) // 16 * 16
    assert r["group_segment_fixed_size"] + ring.fp32_pack_bytes(nh) <= 40960, r
