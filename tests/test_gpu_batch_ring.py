"""The batched fp32 tracer's register ring (nr_trace.hip, RREG) against the CPU oracle, bit for bit.

The batched fp32 k_trace generates rays 64 queue positions at a time, keeps the hits as one spare
ray per lane and deals them to the slots that free up by cross-lane reads.  Which lane marches
which pixel is all that may differ from the oracle: frames and statistics are compared exactly, at
the shapes where such a ring can go wrong -- one 64-pixel chunk, launches whose pixel count is no
multiple of 64, generations that yield few spares (most rays miss the bounding sphere) or 64 of
them (every ray hits), rays that end after 0, 1 or 2 iterations, waves capped at 16 or 32 rays,
few waves for many pixels (each wave generates many times), row-band shards and the iteration map.
"""
import functools

import numpy as np
import pytest

import cudaneuralrender_amd as nr
import oracle

pytestmark = pytest.mark.gpu

GEOM = "plane_1"
# (rx, ry, zoom): an ordinary view; zoomed out, so that most rays miss the bounding sphere; the eye
# inside the bounding sphere (radius 1.2), so that every ray hits it
CAMS = {"mid": (-15.0, 30.0, 2.0), "far": (10.0, 200.0, 8.0), "inside": (0.0, 75.0, 1.0)}
THREE = ("mid", "far", "inside")
STAT_KEYS = ("ray_steps", "shade_evals", "rays_hit", "rays_shaded")


@pytest.fixture(scope="module")
def rend():
    r = nr.Renderer(0)
    dims, K, B = nr.read_keras_h5(nr.geometry_path(GEOM))
    r.load_mlp(dims, K, B).set_precision("fp32").set_static(nr.NR_COLOR_MATCAP, 3).set_scene("v1")
    r.set_matcap(_chrome())
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def _chrome():
    return nr.load_png(nr.matcap_path("Chrome"))


@functools.lru_cache(maxsize=None)
def _net():
    _, K, B = nr.read_keras_h5(nr.geometry_path(GEOM))
    return oracle.OracleNet(K, B)


@functools.lru_cache(maxsize=None)
def _ref(W, H, cam, steps):
    """The oracle's frame and statistics (computed once per shape; read-only)."""
    iv, nm = nr.camera(*CAMS[cam])
    img, st = _net().render(W, H, iv, nm, color_type=1, matcap=_chrome(), max_steps=steps)
    img.setflags(write=False)
    return img, st


def _cams(names):
    return [(*nr.camera(*CAMS[c]), 0) for c in names]


def _check(imgs, st, W, H, names, steps):
    refs = [_ref(W, H, c, steps) for c in names]
    for k, (img, (ref, _)) in enumerate(zip(imgs, refs)):
        assert np.array_equal(img, ref), (names[k], int((img != ref).sum()))
    for key in STAT_KEYS:
        assert st[key] == sum(r[1][key] for r in refs), key
    assert st["iterations"] == max(r[1]["iterations"] for r in refs)


@pytest.mark.parametrize("W,H,names", [(8, 8, ("mid",)), (16, 8, THREE), (67, 45, THREE)])
def test_launch_sizes(rend, W, H, names):
    """One 64-pixel chunk; two chunks per frame in a 3-frame batch; ragged 8x8 blocks with
    frames x pixels no multiple of 64."""
    imgs, st = rend.render_batch(W, H, _cams(names), 64)
    _check(imgs, st, W, H, names, 64)


def test_three_cameras(rend):
    """Three cameras in one launch: generations of the zoomed-out frame yield few spares, those of
    the frame seen from inside the bounding sphere 64."""
    W = H = 96
    assert _ref(W, H, "far", 96)[1]["rays_hit"] < W * H // 4
    assert _ref(W, H, "inside", 96)[1]["rays_hit"] == W * H
    imgs, st = rend.render_batch(W, H, _cams(THREE), 96)
    _check(imgs, st, W, H, THREE, 96)


@pytest.mark.parametrize("steps", [0, 1, 2])
def test_max_steps(rend, steps):
    """Every ray ends at once (0: none is kept as a spare), after one iteration or after two."""
    imgs, st = rend.render_batch(67, 45, _cams(THREE), steps)
    _check(imgs, st, 67, 45, THREE, steps)


@pytest.mark.parametrize("rays", [16, 32])
def test_wave_rays(rend, rays):
    """Waves capped at 16 / 32 rays generate and hold at most that many."""
    rend.set_wave_rays(rays)
    try:
        imgs, st = rend.render_batch(67, 45, _cams(THREE), 64)
    finally:
        rend.set_wave_rays(0)
    _check(imgs, st, 67, 45, THREE, 64)


@pytest.mark.parametrize("rays", [0, 16])
def test_one_workgroup_per_cu(rend, rays):
    """The fewest waves nr_set_occupancy allows (one workgroup per CU) for 12 frames: every wave
    runs out of spares and generates again several times (with 16 rays per wave: about 7 times)."""
    names = THREE * 4
    rend.set_occupancy(1).set_wave_rays(rays)
    try:
        imgs, st = rend.render_batch(96, 96, _cams(names), 64)
    finally:
        rend.set_occupancy(0).set_wave_rays(0)
    _check(imgs, st, 96, 96, names, 64)


def test_three_shards_band_1(rend):
    """Rows dealt to 3 shards one at a time: the shards' batches re-assemble to the oracle's frames
    and their statistics add up to its."""
    W, H = 67, 45
    full = [np.zeros((H, W), np.uint32) for _ in THREE]
    tot = dict.fromkeys(STAT_KEYS, 0)
    for s in range(3):
        imgs, st = rend.render_batch(W, H, _cams(THREE), 64, band=1, nshards=3, shard=s)
        for f, img in zip(full, imgs):
            f[s::3] = img
        for key in STAT_KEYS:
            tot[key] += st[key]
    tot["iterations"] = max(_ref(W, H, c, 64)[1]["iterations"] for c in THREE)
    _check(full, tot, W, H, THREE, 64)


def test_iteration_map(rend):
    """Debug bit 3: every pixel holds the iterations its ray used (a converged ray counts its
    colouring iteration too) -- per frame the map sums to the oracle's ray-steps + shaded rays, its
    maximum is the oracle's, and it is zero exactly where no ray was generated."""
    W, H = 67, 45
    rend.set_debug(8)
    try:
        maps, st = rend.render_batch(W, H, _cams(THREE), 64)
    finally:
        rend.set_debug(0)
    for c, m in zip(THREE, maps):
        ref, rst = _ref(W, H, c, 64)
        assert int(m.astype(np.int64).sum()) == rst["ray_steps"] + rst["rays_shaded"], c
        assert int(m.max()) == rst["iterations"], c
        assert int((m > 0).sum()) == rst["rays_hit"], c
        assert ((m > 0) | (ref == 0)).all(), c
    for key in STAT_KEYS:
        assert st[key] == sum(_ref(W, H, c, 64)[1][key] for c in THREE), key
