"""The batched fp32 tracer's unit form with its weights and biases read ahead of their use
(nr_mlp16.h mlp64_fp32_units), on its default settings, bit for bit against the CPU oracle and
against the same call with the unit form off (nr_set_unit_skip 0).

Frames: plane_1 and car_1 at 96 x 96; one 72 x 40 frame (a ragged last block); three cameras in one
batch; max_steps 24; a 4-input network, whose layer 0 issues its fourth unit.

Designed networks (nr_load_mlp) on an 8 x 8 frame, one wave's worth of rays: every ray starts on
the bounding sphere (|p| = 1.2), so a cap p . n > t around the start point of pixel L holds that
point alone, and one layer-0 unit u = relu(s (p . n - t)) fires for that ray's first evaluation and
for no other.  The unit is carried through the hidden layers on the diagonal (unit u of every
layer) and enters the output with weight -1 against a bias of 0.05: the ray of pixel L hits at its
first step and is shaded, every other ray marches through an all-dead network (scene "tanh": no
sphere grid beside the network's surface).  With all 64 rays
in one wave (set_wave_rays 64; the 8 x 8 block is dealt in pixel order) pixel (L & 7, L >> 3) sits in
lane L: units 1, 7, 8, 15, 16, 31 times lanes 0, 31, 32, 63 put the one nonzero activation at both
ends and both sides of every boundary of a test group of 8, 16 or 32 units and of the wave's halves.
Depths: 1, 2, 7 and 8 hidden 32 x 32 layers -- the read issued during the last layer's epilogue with
one layer and with many.  Plus a network that keeps only unit 0 of every layer alive, and one in
which every unit fires.
"""
import functools

import numpy as np
import pytest

import cudaneuralrender_amd as nr
import depth_nets
import oracle

pytestmark = pytest.mark.gpu

F = np.float32
CAMS = {"front": (0.0, 0.0, 2.0), "mid": (-15.0, 30.0, 2.0), "far": (10.0, 200.0, 8.0), "inside": (0.0, 75.0, 1.0)}
STAT_KEYS = ("ray_steps", "shade_evals", "rays_hit", "rays_shaded")
# name: (network, W, H, cameras, max_steps)
FRAMES = {
    "plane_1": ("plane_1", 96, 96, ("mid",), 64),
    "car_1": ("car_1", 96, 96, ("mid",), 64),
    "ragged": ("plane_1", 72, 40, ("mid",), 48),
    "three_cameras": ("plane_1", 48, 32, ("mid", "far", "inside"), 32),
    "steps_24": ("plane_1", 64, 64, ("front",), 24),
    "four_inputs": ("four_inputs", 48, 48, ("mid", "front"), 48),
}
DEPTHS = (1, 2, 7, 8)
UNITS = (1, 7, 8, 15, 16, 31)
LANES = (0, 31, 32, 63)
DESIGNED_STEPS = 24


@functools.lru_cache(maxsize=None)
def _chrome():
    return nr.load_png(nr.matcap_path("Chrome"))


@functools.lru_cache(maxsize=None)
def _weights(name):
    if name == "four_inputs":
        dims, K, B = depth_nets.cached_net(2, 4)
    else:
        dims, K, B = nr.read_keras_h5(nr.geometry_path(name))
    return list(dims), list(K), list(B)


def _oracle(dims, K, B, W, H, cam, frame, steps, scene):
    iv, nm = nr.camera(*CAMS[cam])
    return oracle.OracleNet(K, B).render(W, H, iv, nm, frame=frame, color_type=1, num_inputs=dims[0],
                                         scene=nr.NR_SCENE[scene], matcap=_chrome(), max_steps=steps, nthreads=16)


def _both_modes(r, W, H, cams, steps):
    """(images, stats, (issued, skipped)) with the unit form on (the default) and off."""
    out = []
    for us in (1, 0):
        r.set_unit_skip(us)
        try:
            imgs, st = r.render_batch(W, H, cams, steps)
            out.append((imgs, st, r.unit_skip_counts()))
        finally:
            r.set_unit_skip(1)
    return out


def _check(r, dims, K, B, W, H, names, frames, steps, scene="v1"):
    cams = [(*nr.camera(*CAMS[c]), f) for c, f in zip(names, frames)]
    refs = [_oracle(dims, K, B, W, H, c, f, steps, scene) for c, f in zip(names, frames)]
    (imgs, st, counts), (imgs0, st0, counts0) = _both_modes(r, W, H, cams, steps)
    print("issued, skipped:", counts, "stats:", st)
    for k, (img, img0, (ref, _)) in enumerate(zip(imgs, imgs0, refs)):
        assert np.array_equal(img, ref), (names[k], int((img != ref).sum()))
        assert np.array_equal(img0, ref), (names[k], int((img0 != ref).sum()))
    for key in STAT_KEYS:
        assert st[key] == sum(x[1][key] for x in refs), key
    assert st["iterations"] == max(x[1]["iterations"] for x in refs)
    for key in st:  # every nr_stats field but the time
        if key != "ms_total":
            assert st[key] == st0[key], key
    assert counts0 == (0, 0)
    return st, counts, refs


@pytest.mark.parametrize("case", sorted(FRAMES))
def test_frames(case):
    net, W, H, names, steps = FRAMES[case]
    dims, K, B = _weights(net)
    frames = [3 + 7 * k if dims[0] == 4 else 0 for k in range(len(names))]
    with nr.Renderer(0) as r:
        r.load_mlp(dims, K, B).set_precision("fp32").set_static(nr.NR_COLOR_MATCAP, dims[0]).set_scene("v1")
        r.set_matcap(_chrome())
        st, (issued, skipped), refs = _check(r, dims, K, B, W, H, names, frames, steps)
    assert nr.pack_fp32_units(dims, K, B) is not None
    units = dims[0] + 32 * (len(dims) - 3)
    evals = sum(x[1]["ray_steps"] + x[1]["shade_evals"] for x in refs)
    assert evals > 0 and st["rays_hit"] > 0
    assert issued % units == 0 and issued >= units * ((evals + 63) // 64) and 0 < skipped <= issued


# ---- designed networks ----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _start_points():
    """[64, 3] float64: where the rays of the 8 x 8 frame of camera "front" enter the bounding sphere
    (initMarcher: u, v = 2 x / W - 1, 2 y / H - 1, d = normalize(u, v, -2) turned by the view)."""
    iv = np.asarray(nr.camera(*CAMS["front"])[0], np.float64).reshape(3, 4)
    o = iv[:, 3]
    P = []
    for L in range(64):
        d = np.array([(L & 7) / 8 * 2 - 1, (L >> 3) / 8 * 2 - 1, -2.0])
        d = iv[:, :3] @ (d / np.linalg.norm(d))
        b = o @ d
        disc = b * b - (o @ o - 1.2 * 1.2)
        assert disc > 0
        P.append(o + (-b - np.sqrt(disc)) * d)
    return np.array(P)


def one_unit_net(nh, u, L, gain=100.0):
    """The network of the module's docstring, nh hidden 32 x 32 layers."""
    P = _start_points()
    n = P[L] / np.linalg.norm(P[L])
    dots = P @ n
    t = 0.5 * (dots[L] + np.max(np.delete(dots, L)))
    dims = [3] + [32] * (nh + 1) + [1]
    K = [np.zeros((dims[i], dims[i + 1]), F) for i in range(nh + 2)]
    B = [np.zeros(dims[i + 1], F) for i in range(nh + 2)]
    K[0][:, u] = (gain * n).astype(F)
    B[0][u] = F(-gain * t)
    for j in range(1, nh + 1):
        K[j][u, u] = 1.0
    K[-1][u, 0] = -1.0
    B[-1][0] = F(0.05)
    # the design, restated: of the 64 start points the unit fires at point L alone, by a margin far
    # above f32 rounding of the three-term chain (|terms| <= 120, so errors ~1e-5)
    act = P @ K[0][:, u].astype(np.float64) + float(B[0][u])
    assert act[L] > 1e-2 and np.all(np.delete(act, L) < -1e-2), (act[L], np.max(np.delete(act, L)))
    return dims, K, B


def unit0_only_net(nh):
    """Unit 0 of every layer fires at every point (a constant 0.5 carried on the diagonal), units
    1-31 never: every test of every layer fails."""
    dims = [3] + [32] * (nh + 1) + [1]
    K = [np.zeros((dims[i], dims[i + 1]), F) for i in range(nh + 2)]
    B = [np.zeros(dims[i + 1], F) for i in range(nh + 2)]
    B[0][0] = 0.5
    for j in range(1, nh + 1):
        K[j][0, 0] = 1.0
    K[-1][0, 0] = 0.25
    B[-1][0] = F(-0.05)  # 0.125 - 0.05: marches through
    return dims, K, B


def all_fire_net(nh):
    """Positive weights and biases throughout: every unit of every layer is nonzero at every point."""
    rng = np.random.default_rng(5)
    dims = [3] + [32] * (nh + 1) + [1]
    K = [np.zeros((dims[i], dims[i + 1]), F) for i in range(nh + 2)]
    B = [np.zeros(dims[i + 1], F) for i in range(nh + 2)]
    K[0][:] = rng.uniform(-0.05, 0.05, K[0].shape)
    B[0][:] = rng.uniform(0.3, 0.6, 32)  # |w . p| <= 0.05 * 1.2 * sqrt(3) < 0.3
    for j in range(1, nh + 1):
        K[j][:] = rng.uniform(0.0, 1.0 / 32, K[j].shape)
        B[j][:] = rng.uniform(0.01, 0.1, 32)
    K[-1][:, 0] = rng.uniform(-0.02, 0.02, 32)
    B[-1][0] = F(0.04)
    return dims, K, B


@pytest.fixture(scope="module")
def small():
    r = nr.Renderer(0)
    # (the scene without the sphere grid: what is hit is the network's surface alone)
    r.set_precision("fp32").set_static(nr.NR_COLOR_MATCAP, 3).set_scene("tanh").set_matcap(_chrome())
    yield r
    r.close()


def _designed(r, dims, K, B):
    r.load_mlp(dims, K, B).set_wave_rays(64)
    try:
        assert nr.pack_fp32_units(dims, K, B) is not None
        return _check(r, dims, K, B, 8, 8, ("front",), (0,), DESIGNED_STEPS, "tanh")
    finally:
        r.set_wave_rays(0)


@pytest.mark.parametrize("nh", DEPTHS)
def test_one_unit_in_one_lane(small, nh):
    for u in UNITS:
        for L in LANES:
            dims, K, B = one_unit_net(nh, u, L)
            st, (issued, skipped), refs = _designed(small, dims, K, B)
            ref = refs[0][0]
            # the oracle's frame is the design: pixel L hit at its first step, nothing else
            assert st["rays_hit"] == 64 and st["rays_shaded"] == 1, (u, L, st)
            assert ref[L >> 3, L & 7] != 0 and np.count_nonzero(ref) == 1, (u, L)
            # an evaluation executes layer 0's three instructions and unit 0 of every hidden layer;
            # beyond those, unit u of every hidden layer at least once, and next to nothing else
            assert issued % (3 + 32 * nh) == 0
            evals = issued // (3 + 32 * nh)
            fired = issued - skipped - evals * (3 + nh)
            assert nh <= fired <= 8 * nh, (u, L, issued, skipped)


@pytest.mark.parametrize("nh", DEPTHS)
def test_only_unit_0_alive(small, nh):
    st, (issued, skipped), _ = _designed(small, *unit0_only_net(nh))
    units = 3 + 32 * nh
    # of every evaluation's 3 + 32 nh instructions exactly the 31 nh tested ones are skipped
    assert issued % units == 0 and skipped == issued // units * 31 * nh, (issued, skipped)


@pytest.mark.parametrize("nh", DEPTHS)
def test_every_unit_fires(small, nh):
    st, (issued, skipped), _ = _designed(small, *all_fire_net(nh))
    assert issued > 0 and skipped == 0, (issued, skipped)
