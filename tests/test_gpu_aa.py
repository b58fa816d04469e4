"""nr_render_aa on the GPU (nr_aa.hip) against tests/aa_ref.py applied to the CPU oracle's
S W x S H frame (aa_ref is pinned by tests/test_aa_cpu.py).  The call always runs the fp32 MLP,
whose contract is bit-exactness: every image comparison is exact uint32 equality, edge counts are
compared with the reference's mask and the statistics with rule 5 of the contract."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import aa_ref
import cudaneuralrender_amd as nr
import oracle
from conftest import REF_CAMERAS

pytestmark = pytest.mark.gpu
# where torch bundles a HIP runtime of its own beside libnr's, torch has to open the GPU first
if torch.cuda.is_available():
    torch.cuda.init()

STEPS = 300
STAT_KEYS = ("ray_steps", "shade_evals", "rays_hit", "rays_shaded", "iterations")
# (rx, ry, zoom, tx, ty).  "close": the reference camera's angles near enough for the frame border to
# cut the object; "inside": the eye inside the bounding sphere (the tnear clamp); "off": translated
# until no ray meets the bounding sphere
CAMERAS = {"ref": REF_CAMERAS["plane_1"] + (0.0, 0.0),
           "close": REF_CAMERAS["plane_1"][:2] + (0.9, 0.0, 0.0),
           "inside": (10.0, 40.0, 0.6, 0.0, 0.0),
           "off": REF_CAMERAS["plane_1"] + (50.0, 0.0)}
COLORS = {"facing": nr.NR_COLOR_FACING, "matcap": nr.NR_COLOR_MATCAP}


@functools.lru_cache(maxsize=None)
def matcap():
    return nr.load_png(nr.matcap_path("Chrome"))


@functools.lru_cache(maxsize=None)
def plane_net(four):
    """plane_1's network and its oracle; four: a 4th input row appended to the first kernel, as
    test_gpu_query.py builds one."""
    dims, K, B = nr.read_keras_h5(nr.geometry_path("plane_1"))
    if four:
        K = [np.concatenate([K[0], np.random.default_rng(4).normal(0, 0.01, (1, 32)).astype(np.float32)], 0)] + K[1:]
        dims = [4] + list(dims[1:])
    return dims, K, B, oracle.OracleNet(K, B)


@functools.lru_cache(maxsize=None)
def oracle_frame(cam, W, H, scene="v1", color="facing", steps=STEPS, four=False, frame=0):
    """The oracle's W x H frame and stats: computed once per configuration, shared, never modified."""
    iv, nm = nr.camera(*CAMERAS[cam])
    img, st = plane_net(four)[3].render(W, H, iv, nm, frame=frame, color_type=COLORS[color], num_inputs=4 if four else 3,
                                        scene=nr.NR_SCENE[scene], matcap=matcap() if color == "matcap" else None,
                                        max_steps=steps)
    img.setflags(write=False)
    return img, st


def reference(cam, W, H, S, contrast=32, full=False, **kw):
    """(antialiased frame, edge mask, the S W x S H frame, its stats)"""
    big, bst = oracle_frame(cam, S * W, S * H, **kw)
    out, mask = aa_ref.resolve(big, S, contrast, full)
    return out, mask, big, bst


@pytest.fixture(scope="module")
def rend():
    dims, K, B, _ = plane_net(False)
    r = nr.Renderer(0)
    r.load_mlp(dims, K, B).set_precision("fp32").set_matcap(matcap())
    yield r
    r.close()


def setup(r, cam, scene="v1", color="facing", frame=0, inputs=3):
    r.set_view(*nr.camera(*CAMERAS[cam]), frame).set_scene(scene).set_static(COLORS[color], inputs)
    return r


def assert_frame(got, ref):
    assert got.shape == ref.shape and got.dtype == np.uint32
    bad = got != ref
    assert not bad.any(), (f"{int(bad.sum())} of {bad.size} pixels differ, first (y, x) = {np.argwhere(bad)[0]}: "
                           f"{got[bad][0]:#010x} != {ref[bad][0]:#010x}")


def floors(cam, out, mask, base, contrast):
    """The reference exercises what the case is there for (counts from the CPU oracle)."""
    assert mask.sum() >= 50
    alpha = out >> 24
    assert ((alpha > 0) & (alpha < 255)).sum() >= 20
    if cam in ("close", "inside"):
        # (at contrast 0 nearly every coloured pixel is an edge)
        assert ((base != 0) & ~mask).sum() >= (50 if contrast else 0)
        border = np.ones_like(mask)
        border[1:-1, 1:-1] = False
        assert (mask & border).sum() >= 4


def sub_sample_stats(r, mask, W, H, S, steps):
    """The statistics of the sub-sample rays other than (0, 0) of the masked pixels, from the
    per-pixel geometry buffer of the S W x S H view (k_query; test_gpu_query.py pins it)."""
    g, gst = r.render_gbuffer(S * W, S * H, steps, normals=False, with_stats=True)
    sel = np.repeat(np.repeat(mask, S, 0), S, 1)
    sel[::S, ::S] = False
    status, st = g["status"][sel], g["steps"][sel]
    hit = status == nr.NR_RAY_HIT
    # a coloured ray is shaded by the iteration after the one it converged in (nr_render's count)
    its = int((st + hit).max()) if st.size else 0
    return {"ray_steps": int(st.sum()), "rays_hit": int((status != nr.NR_RAY_MISS).sum()), "rays_shaded": int(hit.sum()),
            "shade_evals": 4 * int(hit.sum()), "iterations": its}, gst


def check_adaptive(r, cam, W, H, S, contrast=32, steps=STEPS, check_floors=True, **kw):
    ref, mask, big, bst = reference(cam, W, H, S, contrast, steps=steps, **kw)
    if check_floors:
        floors(cam, ref, mask, big[::S, ::S], contrast)
    img, st = r.render_aa(W, H, S, "adaptive", contrast, steps)
    assert_frame(img, ref)
    assert st["edge_pixels"] == int(mask.sum())
    # rule 5: the base frame's statistics plus those of the additional sub-sample rays
    _, base_st = oracle_frame(cam, W, H, steps=steps, **kw)
    sub, gst = sub_sample_stats(r, mask, W, H, S, steps)
    assert gst["ray_steps"] == bst["ray_steps"] and gst["rays_hit"] == bst["rays_hit"]
    for k in STAT_KEYS[:4]:
        assert st[k] == base_st[k] + sub[k], (k, st, base_st, sub)
    assert st["iterations"] == max(base_st["iterations"], sub["iterations"]), (st, base_st, sub)
    return img, st


ADAPTIVE = [  # W, H, S, camera, scene, colouring
    (37, 29, 3, "ref", "v1", "facing"),
    (37, 29, 3, "close", "tanh", "matcap"),
    (37, 29, 3, "inside", "displace", "matcap"),
    (64, 48, 2, "ref", "tanh", "facing"),
    (64, 48, 2, "close", "v1", "matcap"),
    (64, 48, 2, "inside", "v1", "facing"),
    (64, 48, 4, "close", "v1", "facing"),
    (64, 48, 4, "inside", "tanh", "matcap"),
    (64, 48, 4, "ref", "displace", "facing"),
    (40, 24, 8, "close", "v1", "facing"),
    (40, 24, 8, "ref", "tanh", "matcap"),
    (40, 24, 8, "inside", "v1", "matcap"),
]


@pytest.mark.parametrize("W,H,S,cam,scene,color", ADAPTIVE)
def test_adaptive_bitexact(rend, W, H, S, cam, scene, color):
    check_adaptive(setup(rend, cam, scene, color), cam, W, H, S, scene=scene, color=color)


@pytest.mark.parametrize("contrast", [0, 254])
def test_contrasts(rend, contrast):
    """0: every gradient is an edge; 254: the silhouette alone (alpha 255 against 0)."""
    _, st = check_adaptive(setup(rend, "close"), "close", 64, 48, 2, contrast)
    _, m32, _, _ = reference("close", 64, 48, 2, 32)
    n32 = int(m32.sum())
    assert st["edge_pixels"] > n32 + 50 if contrast == 0 else 50 <= st["edge_pixels"] < n32 - 50


@pytest.mark.parametrize("W,H,S,cam,scene,color", [(64, 48, 2, "close", "v1", "facing"),
                                                    (37, 29, 3, "inside", "tanh", "matcap")])
def test_full_mode(rend, W, H, S, cam, scene, color):
    """Every pixel resolved: the box filter of nr_render's own S W x S H frame and of the oracle's,
    with nr_render's statistics for that frame."""
    setup(rend, cam, scene, color)
    ref, mask, big, bst = reference(cam, W, H, S, full=True, scene=scene, color=color)
    gbig, gst = rend.render(S * W, S * H, STEPS)
    img, st = rend.render_aa(W, H, S, "full", 32, STEPS)
    assert_frame(gbig, big)
    assert_frame(img, aa_ref.resolve(gbig, S, 32, True)[0])
    assert_frame(img, ref)
    assert st["edge_pixels"] == W * H
    for k in STAT_KEYS:
        assert st[k] == gst[k] == bst[k], (k, st, gst, bst)
    # the contrast is not read in FULL mode
    assert_frame(rend.render_aa(W, H, S, "full", 255, STEPS, with_stats=False), ref)


@pytest.mark.parametrize("cam,S,mode,contrast", [("close", 1, "adaptive", 32), ("close", 1, "full", 32),
                                                 ("close", 4, "adaptive", 255), ("off", 4, "adaptive", 0)])
def test_identities(rend, cam, S, mode, contrast):
    """One sample per pixel, a contrast no difference exceeds, or a frame without an edge: the call
    is nr_render's frame bit for bit, and no sub-sample ray is traced."""
    W, H = 64, 48
    setup(rend, cam)
    base, bst = rend.render(W, H, STEPS)
    assert_frame(base, oracle_frame(cam, W, H)[0])
    assert (base != 0).sum() >= (0 if cam == "off" else 50) and (cam != "off" or not base.any())
    img, st = rend.render_aa(W, H, S, mode, contrast, STEPS)
    assert_frame(img, base)
    assert st["edge_pixels"] == (W * H if mode == "full" else 0)
    for k in STAT_KEYS:
        assert st[k] == bst[k], (k, st, bst)


@pytest.mark.parametrize("W,H", [(1, 1), (1, 7), (7, 1)])
@pytest.mark.parametrize("mode", ["adaptive", "full"])
def test_degenerate_frames(rend, W, H, mode):
    S = 4
    setup(rend, "inside")
    ref, mask, big, bst = reference("inside", W, H, S, 0, mode == "full")
    assert (big != 0).sum() >= 4
    img, st = rend.render_aa(W, H, S, mode, 0, STEPS)
    assert_frame(img, ref)
    assert st["edge_pixels"] == int(mask.sum())
    if mode == "full":
        for k in STAT_KEYS:
            assert st[k] == bst[k], (k, st, bst)


def test_step_cap_12(rend):
    """Rays inside the silhouette that have not converged after 12 iterations stay background."""
    W, H, S = 64, 48, 2
    setup(rend, "close", "tanh")
    ref12, _, big12, _ = reference("close", W, H, S, steps=12, scene="tanh")
    big = oracle_frame("close", S * W, S * H, scene="tanh")[0]
    assert ((big12 == 0) & (big != 0)).sum() >= 50 and (big12 != 0).sum() >= 50
    check_adaptive(rend, "close", W, H, S, steps=12, scene="tanh", check_floors=False)


@pytest.mark.parametrize("steps", [12, 2, 1])
def test_step_caps_full(rend, steps):
    """A converged ray needs an iteration left to be shaded: FULL mode traces every sub-sample under
    the cap, and its statistics are the S W x S H frame's."""
    W, H, S = 64, 48, 2
    setup(rend, "close", "tanh")
    ref, _, big, bst = reference("close", W, H, S, full=True, steps=steps, scene="tanh")
    assert bst["rays_hit"] >= 50 and bst["ray_steps"] >= bst["rays_hit"]
    if steps <= 2:
        assert bst["rays_shaded"] == 0 and not big.any()
    img, st = rend.render_aa(W, H, S, "full", 32, steps)
    assert_frame(img, ref)
    for k in STAT_KEYS:
        assert st[k] == bst[k], (k, st, bst)


def test_four_input_network():
    """(float)frame is the network's 4th input, at a frame number other than 0 (scene v1 reads the
    frame number too)."""
    W, H, S, frame = 64, 48, 2, 5
    dims, K, B, _ = plane_net(True)
    kw = dict(four=True, frame=frame)
    assert not np.array_equal(oracle_frame("close", S * W, S * H, **kw)[0], oracle_frame("close", S * W, S * H, four=True, frame=0)[0])
    with nr.Renderer(0) as r:
        r.load_mlp(dims, K, B)
        setup(r, "close", frame=frame, inputs=4)
        check_adaptive(r, "close", W, H, S, **kw)


def test_refills(rend):
    """More sub-samples than the launch has ray slots (one workgroup per CU, 256 lanes each): every
    wave refills from the cursor."""
    W, H, S = 160, 120, 4
    setup(rend, "close")
    ref, mask, _, _ = reference("close", W, H, S, 0)
    slots = torch.cuda.get_device_properties(0).multi_processor_count * 256
    assert int(mask.sum()) * (S * S - 1) > slots
    try:
        rend.set_occupancy(1)
        img, st = rend.render_aa(W, H, S, "adaptive", 0, STEPS)
    finally:
        rend.set_occupancy(0)
    assert_frame(img, ref)
    assert st["edge_pixels"] == int(mask.sum())
    # any grid gives the same bits
    assert_frame(rend.render_aa(W, H, S, "adaptive", 0, STEPS, with_stats=False), ref)


def test_settings_ignored_and_preserved(rend):
    W, H, S = 64, 48, 2
    setup(rend, "close")
    ref = reference("close", W, H, S)[0]
    try:
        rend.set_precision("bf16").set_schedule("wavefront")
        before, _ = rend.render(W, H, STEPS)
        img, st = rend.render_aa(W, H, S, "adaptive", 32, STEPS)
        after, _ = rend.render(W, H, STEPS)
    finally:
        rend.set_precision("fp32").set_schedule("persistent")
    assert_frame(img, ref)
    assert_frame(after, before)
    # (the bf16 frame is not the fp32 one: the setting was in force around the call)
    assert not np.array_equal(before, oracle_frame("close", W, H)[0])


def test_aa_leaves_precision_and_schedule_alone(rend):
    """In a bf16 context on the wavefront schedule the call gives the frame an fp32 persistent
    context gives, and the context's own renders before and after it are the same frame."""
    W, H, S, steps = 96, 77, 2, 64
    setup(rend, "close")
    ref, rst = rend.render_aa(W, H, S, "adaptive", 32, steps)
    assert rst["edge_pixels"] >= 50
    try:
        rend.set_precision("bf16").set_schedule("wavefront")
        before, bst = rend.render(W, H, steps)
        img, st = rend.render_aa(W, H, S, "adaptive", 32, steps)
        after, ast = rend.render(W, H, steps)
    finally:
        rend.set_precision("fp32").set_schedule("persistent")
    assert_frame(after, before)
    assert_frame(img, ref)
    assert st["edge_pixels"] == rst["edge_pixels"]
    for k in STAT_KEYS:
        assert st[k] == rst[k] and ast[k] == bst[k], k


def test_determinism_and_device_output(rend):
    """Two calls give the same bits; a device buffer on a caller-supplied stream holds what the host
    output holds."""
    W, H, S = 64, 48, 4
    setup(rend, "close")
    ref, mask, _, _ = reference("close", W, H, S)
    a, ast = rend.render_aa(W, H, S, "adaptive", 32, STEPS)
    b, bst = rend.render_aa(W, H, S, "adaptive", 32, STEPS)
    assert_frame(a, ref)
    assert_frame(b, a)
    for k in STAT_KEYS + ("edge_pixels",):
        assert ast[k] == bst[k]
    dev = torch.device("cuda:0")
    out = torch.full((H, W), 0x55555555, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    try:
        with torch.cuda.stream(stream):
            rend.set_stream(stream.cuda_stream)
            edges = rend.render_aa_device(out.data_ptr(), W, H, S, "adaptive", 32, STEPS)
            rend.synchronize()
        stream.synchronize()
    finally:
        rend.set_stream(None, own=True)
    assert edges == int(mask.sum())
    assert_frame(out.cpu().numpy().view(np.uint32), ref)


def test_errors(rend):
    L = nr.lib()
    buf = np.zeros(64, np.uint32)

    def call(r, out=buf.ctypes.data, W=4, H=4, S=2, mode=0, contrast=32, steps=10):
        return L.nr_render_aa(r._ctx if r is not None else None, out, W, H, S, mode, contrast, steps, 0, None, None)

    setup(rend, "close")
    assert call(rend) == 0
    assert call(None) == -1 and call(rend, out=None) == -1  # NR_E_INVALID
    assert call(rend, W=0) == -1 and call(rend, H=0) == -1 and call(rend, W=-3) == -1
    assert call(rend, S=0) == -1 and call(rend, S=9) == -1
    assert call(rend, mode=2) == -1 and call(rend, mode=-1) == -1
    assert call(rend, contrast=-1) == -1 and call(rend, contrast=256) == -1
    assert call(rend, W=1 << 15, H=(1 << 15) + 1, S=1) == -1  # S W * S H = 2^30 + 2^15 > 2^30
    assert call(rend, W=1 << 14, H=(1 << 14) + 1, S=2) == -1  # 4 (2^28 + 2^14)
    assert call(rend, W=(1 << 30) + 1, H=1, S=1) == -1 and call(rend, W=1 << 28, H=1, S=8) == -1
    assert call(rend, steps=-1) == -1  # as nr_render
    assert L.nr_render(rend._ctx, buf.ctypes.data, 4, 4, -1, 0, None) == -1
    edges = ctypes.c_long(-7)
    assert L.nr_render_aa(rend._ctx, buf.ctypes.data, 4, 4, 2, 1, 32, 10, 0, ctypes.byref(edges), None) == 0
    assert edges.value == 16
    with nr.Renderer(0) as r:
        assert call(r) == -5  # NR_E_STATE: no network
        rng = np.random.default_rng(0)
        r.load_mlp([3, 16, 1], [rng.normal(size=(3, 16)).astype(np.float32), rng.normal(size=(16, 1)).astype(np.float32)],
                   [np.zeros(16, np.float32), np.zeros(1, np.float32)])
        assert call(r) == -4  # NR_E_FORMAT: not a network of the fused kernels, and no layered fallback
        assert L.nr_render(r._ctx, buf.ctypes.data, 4, 4, 10, 0, None) == 0
    # what nr_render reports for the context, as nr_render reports it
    dims, K, B, _ = plane_net(False)
    with nr.Renderer(0) as r:
        r.load_mlp(dims, K, B).set_static(nr.NR_COLOR_MATCAP, 3)
        assert call(r) == L.nr_render(r._ctx, buf.ctypes.data, 4, 4, 10, 0, None) == -5  # matcap colouring, no matcap
        r.set_static(nr.NR_COLOR_FACING, 4)
        assert call(r) == L.nr_render(r._ctx, buf.ctypes.data, 4, 4, 10, 0, None) == -5  # numInputs mismatch
