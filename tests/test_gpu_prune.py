"""The batched fp32 tracer on the pruned pack (nr_mlp16.h mlp16_fp32_pruned) against the CPU oracle,
bit for bit, in every mode of nr_set_prune.

Mode 1 skips the k-steps of the units the pack found never firing and redoes a wave's evaluation on
the full pack when one fires after all; mode 2 makes the four highest-numbered units of every layer
candidates whatever they do, so the redo runs constantly; mode 0 has no candidates.  Frames of
16x16, 24x40 and 48x32 pixels, one to three per batch, at 24 to 32 steps: waves of one, two, three
and four 16-point tiles and the drained tail.  Frames and statistics are the oracle's in all three
modes; the redo counter is positive in mode 2 and zero in mode 0.
"""
import functools

import numpy as np
import pytest

import cudaneuralrender_amd as nr
import designed_nets
import oracle

pytestmark = pytest.mark.gpu

CAMS = {"mid": (-15.0, 30.0, 2.0), "far": (10.0, 200.0, 8.0), "inside": (0.0, 75.0, 1.0)}
# (W, H, cameras of the batch, steps)
SHAPES = [(16, 16, ("mid",), 24), (24, 40, ("mid", "inside"), 28), (48, 32, ("mid", "far", "inside"), 32)]
STAT_KEYS = ("ray_steps", "shade_evals", "rays_hit", "rays_shaded")
NETS = ("plane_1", "car_1", "designed")


@functools.lru_cache(maxsize=None)
def _weights(name):
    if name == "designed":
        # a tilted plane through the volume: two live units per layer, thirty that never fire; the
        # live ones moved from units 0, 1 to 30, 31, so that test mode's candidates (28-31) fire
        dims, K, B = designed_nets.linear_net((0.3, 0.8, -0.5), 0.05, nh=3)
        perm = np.arange(32)
        perm[[0, 1, 30, 31]] = [30, 31, 0, 1]
        K = [K[0][:, perm]] + [k[perm][:, perm] for k in K[1:-1]] + [K[-1][perm]]
        B = [b[perm] for b in B[:-1]] + [B[-1]]
        return dims, [np.ascontiguousarray(k) for k in K], B
    return nr.read_keras_h5(nr.geometry_path(name))


@functools.lru_cache(maxsize=None)
def _chrome():
    return nr.load_png(nr.matcap_path("Chrome"))


@functools.lru_cache(maxsize=None)
def _ref(name, W, H, cam, steps):
    """The oracle's frame and statistics (once per network and shape; read-only)."""
    _, K, B = _weights(name)
    iv, nm = nr.camera(*CAMS[cam])
    img, st = oracle.OracleNet(K, B).render(W, H, iv, nm, color_type=1, matcap=_chrome(), max_steps=steps)
    img.setflags(write=False)
    return img, st


@pytest.fixture(scope="module", params=NETS)
def rend(request):
    r = nr.Renderer(0)
    dims, K, B = _weights(request.param)
    r.load_mlp(dims, K, B).set_precision("fp32").set_static(nr.NR_COLOR_MATCAP, 3).set_scene("v1")
    r.set_matcap(_chrome())
    yield request.param, r
    r.close()


def _render(r, mode, W, H, names, steps):
    r.set_prune(mode)
    try:
        imgs, st = r.render_batch(W, H, [(*nr.camera(*CAMS[c]), 0) for c in names], steps)
        return imgs, st, r.prune_redos(), r.prune_info()
    finally:
        r.set_prune(1)


@pytest.mark.parametrize("W,H,names,steps", SHAPES)
def test_modes_match_the_oracle(rend, W, H, names, steps):
    name, r = rend
    refs = [_ref(name, W, H, c, steps) for c in names]
    out = {}
    for mode in (1, 2, 0):
        imgs, st, redos, info = _render(r, mode, W, H, names, steps)
        print(name, (W, H), "mode", mode, "candidates", info["cand"].tolist(), "redos", redos, "ray_steps", st["ray_steps"])
        for k, (img, (ref, _)) in enumerate(zip(imgs, refs)):
            assert np.array_equal(img, ref), (mode, names[k], int((img != ref).sum()))
        for key in STAT_KEYS:
            assert st[key] == sum(x[1][key] for x in refs), (mode, key)
        assert st["iterations"] == max(x[1]["iterations"] for x in refs), mode
        out[mode] = (imgs, {k: st[k] for k in STAT_KEYS + ("iterations",)}, redos, info)
    # the three modes: identical frames and statistics
    for mode in (2, 0):
        assert out[mode][1] == out[1][1]
        assert all(np.array_equal(a, b) for a, b in zip(out[mode][0], out[1][0]))
    assert out[0][2] == 0 and out[0][3]["cand"].sum() == 0
    assert (out[2][3]["cand"] == 4).all()
    if sum(x[1]["ray_steps"] for x in refs) > 0:
        assert out[2][2] > 0, "test mode never took the redo"


def test_designed_network_skips_the_most():
    """The designed network's thirty dead units per layer: mode 1 takes the largest candidate set
    (16 per layer, k-steps 0-3 only)."""
    dims, K, B = _weights("designed")
    P = nr.pack_fp32_pruned(dims, K, B, 1)
    assert (P["cand"] == 16).all() and (P["ks"] == 4).all()
