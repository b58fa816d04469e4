"""nr_render_lit on the GPU (nr_light.hip) against tests/light_ref.py, the numpy restatement of its
contract (pinned by tests/test_light_cpu.py), against nr_render's frame and against the library's
own ray queries.  Every comparison is exact: frames as uint32, ao and shadow on their uint32 views."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cudaneuralrender_amd as nr
from cudaneuralrender_amd import _lib
import designed_nets
import light_ref
import oracle
from light_cases import CASES, FRAME, IV, LIGHT, LIGHT_DIR, NM, network, reference, view
from query_ref import ESCAPED, HIT, MISS

pytestmark = pytest.mark.gpu
STAT_KEYS = ("ray_steps", "shade_evals", "rays_hit", "rays_shaded", "iterations")
BUFS = ("out", "ao", "shadow")
# where torch bundles a HIP runtime of its own beside libnr's, torch has to open the GPU first
# (as tools/layered_bench.py does): opened second, it finds no device
if torch.cuda.is_available():
    torch.cuda.init()


@pytest.fixture(scope="module")
def rend():
    dims, K, B, _ = network("plane_1")
    r = nr.Renderer(0)
    r.load_mlp(dims, K, B).set_precision("fp32").set_static(nr.NR_COLOR_FACING, 3)
    r.set_matcap(nr.load_png(nr.matcap_path("Chrome")))
    yield r
    r.close()


@pytest.fixture(scope="module")
def rend4():
    """The 4-input network's context."""
    dims, K, B, _ = network("depth7x4")
    r = nr.Renderer(0)
    r.load_mlp(dims, K, B).set_precision("fp32").set_static(nr.NR_COLOR_FACING, 4)
    yield r
    r.close()


def setup(r, case):
    scene = CASES[case][1]
    r.set_view(*view(case), FRAME).set_scene(scene)
    return CASES[case][2], CASES[case][3], CASES[case][5]


def lit(r, case, shadow_steps=64, light_dir=LIGHT_DIR, **kw):
    """render_lit of a case with the tests' light: ({out, ao, shadow}, stats)."""
    W, H, steps = setup(r, case)
    out, ao, sh, st = r.render_lit(W, H, light_dir, shadow_steps=shadow_steps, max_steps=steps, buffers=True,
                                   with_stats=True, **dict(LIGHT, **kw))
    return {"out": out, "ao": ao, "shadow": sh}, st


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, ref, keys=BUFS):
    for k in keys:
        g, r = got[k], ref[k]
        assert g.shape == r.shape and g.dtype == r.dtype, (k, g.shape, r.shape, g.dtype, r.dtype)
        bad = bits(g) != bits(r)
        assert not bad.any(), f"{k}: {int(bad.sum())} of {bad.size} values differ, first pixel {np.argwhere(bad)[0]}"


def raw(r, W, H, steps, want=BUFS, device=False, shadow_steps=64, light_dir=LIGHT_DIR, **kw):
    """nr_render_lit through the C ABI with the outputs named in `want` only (the others NULL), into
    host arrays or torch tensors on cuda:0.  Returns (rc, {name: numpy array})."""
    lt = r._light(light_dir, shadow_steps, **dict(LIGHT, **kw))
    dtypes = {"out": np.uint32, "ao": np.float32, "shadow": np.float32}
    if device:
        bufs = {k: torch.full((H, W), 0x55555555, dtype=torch.int32, device="cuda:0") for k in want}
        ptr = {k: ctypes.c_void_p(v.data_ptr()) for k, v in bufs.items()}
        torch.cuda.synchronize()  # (the fills ran on torch's stream, the call runs on the context's)
    else:
        bufs = {k: np.full((H, W), 0x55555555, np.uint32).view(dtypes[k]) for k in want}
        ptr = {k: v.ctypes.data for k, v in bufs.items()}
    rc = r._L.nr_render_lit(r._ctx, ptr.get("out"), W, H, steps, ctypes.byref(lt), ptr.get("ao"), ptr.get("shadow"),
                            _lib.NR_DEVICE if device else _lib.NR_HOST, None)
    if device:
        r.synchronize()
        bufs = {k: v.cpu().numpy().view(dtypes[k]) for k, v in bufs.items()}
    return rc, bufs


# ---- 1. the light switched off: nr_render's fp32 frame

@pytest.mark.parametrize("scene", ["v1", "tanh"])
@pytest.mark.parametrize("color", ["facing", "matcap"])
def test_identity(rend, color, scene):
    W, H, steps = setup(rend, "A")
    try:
        rend.set_scene(scene).set_static(nr.NR_COLOR_MATCAP if color == "matcap" else nr.NR_COLOR_FACING, 3)
        frame, _ = rend.render(W, H, steps)
        out, ao, sh = rend.render_lit(W, H, LIGHT_DIR, max_steps=steps, buffers=True, **light_ref.LIGHT_OFF)
    finally:
        rend.set_static(nr.NR_COLOR_FACING, 3)
    assert (frame != 0).sum() >= 200 and len(np.unique(frame)) >= 20
    assert np.array_equal(out, frame), f"{(out != frame).sum()} pixels differ"
    assert np.array_equal(bits(ao), bits(np.ones((H, W), np.float32)))
    assert np.array_equal(bits(sh), bits(np.ones((H, W), np.float32)))


# ---- 2. / 5. against the reference

# Case B deals 64 pixels per refill to waves whose lanes are all free, and 2,222 of its 3,072 pixels
# hit: the occlusion list takes up to 64 entries in one refill on top of a pass's leftover, and is
# emptied by full 16-pixel passes, by the pass of the drained cursor and with leftovers below 16.
@pytest.mark.parametrize("case,shadow_steps", [("A", 64), ("A", 32), ("B", 64), ("T", 64), ("AO", 64)])
def test_against_the_reference(rend, case, shadow_steps):
    ref = reference(case, shadow_steps)
    got, st = lit(rend, case, shadow_steps)
    assert_same(got, ref)
    for k in STAT_KEYS:
        assert st[k] == ref["stats"][k], (k, st, ref["stats"])
    assert st["launches"] == 5 and st["ms_total"] > 0


def test_four_input_network(rend4):
    """(float)frame is the network's 4th input in the geometry buffer, the occlusion samples and the
    shadow march alike."""
    ref = reference("F4")
    got, st = lit(rend4, "F4")
    assert_same(got, ref)
    for k in STAT_KEYS:
        assert st[k] == ref["stats"][k], (k, st, ref["stats"])


# ---- 3. against the library's own queries

@pytest.mark.parametrize("case,shadow_steps", [("A", 64), ("A", 32)])
def test_hard_shadows_against_trace_rays(rend, case, shadow_steps):
    """With shadow_k = 0 the shadow is 1 exactly where nr_trace_rays, given the rays o = p + n * bias
    built on the host from nr_render_gbuffer, reports ESCAPED or MISS."""
    W, H, steps = setup(rend, case)
    got, st = lit(rend, case, shadow_steps, shadow_k=0.0)
    g, gst = rend.render_gbuffer(W, H, steps, with_stats=True)
    L = np.asarray(LIGHT_DIR, np.float32)
    n, p = g["normal"].reshape(-1, 3), g["position"].reshape(-1, 3)
    hit = g["status"].reshape(-1) == HIT
    dd = (n[:, 0] * L[0] + n[:, 1] * L[1]) + n[:, 2] * L[2]
    sel = np.flatnonzero(hit & (dd > 0))
    assert sel.size >= 200 and sel.size < hit.sum()
    o = (p[sel] + n[sel] * np.float32(LIGHT["shadow_bias"])).astype(np.float32)
    q, qst = rend.trace_rays(o, np.broadcast_to(L, o.shape), shadow_steps, normals=False, with_stats=True)
    expect = np.ones(W * H, np.float32)
    expect[hit] = 0.0
    expect[sel[(q["status"] == ESCAPED) | (q["status"] == MISS)]] = 1.0
    assert int((expect[hit] == 0).sum()) >= 100 and int((expect[hit] == 1).sum()) >= 200
    assert np.array_equal(bits(got["shadow"].reshape(-1)), bits(expect))
    assert st["ray_steps"] - gst["ray_steps"] == qst["ray_steps"]
    for k in ("rays_hit", "rays_shaded"):
        assert st[k] == gst[k]


# ---- 4. independence

def test_host_device_and_null_outputs(rend):
    """The same bits in host arrays and device buffers, with any subset of the three outputs."""
    W, H, steps = setup(rend, "A")
    ref = reference("A")
    for device in (False, True):
        for want in (BUFS, ("out",), ("ao",), ("shadow",), ("out", "ao"), ("out", "shadow"), ("ao", "shadow")):
            rc, got = raw(rend, W, H, steps, want, device)
            assert rc == 0, (rend._L.nr_last_error(rend._ctx), want, device)
            assert_same(got, ref, want)


def test_device_output_on_a_caller_stream(rend):
    W, H, steps = setup(rend, "B")
    ref = reference("B")
    dev = torch.device("cuda:0")
    out = torch.full((H, W), 0x55555555, dtype=torch.int32, device=dev)
    ao = torch.full((H, W), -1.0, dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(dev)
    try:
        with torch.cuda.stream(stream):
            rend.set_stream(stream.cuda_stream)
            rend.render_lit_device(out.data_ptr(), W, H, LIGHT_DIR, max_steps=steps, ao_ptr=ao.data_ptr(), **LIGHT)
            rend.synchronize()
        stream.synchronize()
    finally:
        rend.set_stream(None, own=True)
    assert_same({"out": out.cpu().numpy().view(np.uint32), "ao": ao.cpu().numpy()}, ref, ("out", "ao"))


@pytest.mark.parametrize("bpc", [1, 3])
def test_occupancy(rend, bpc):
    try:
        rend.set_occupancy(bpc)
        for case in ("A", "B"):
            assert_same(lit(rend, case)[0], reference(case))
    finally:
        rend.set_occupancy(0)


def test_repeated_calls_reuse_the_scratch(rend):
    """Twice in a row, and a smaller frame after a larger one and back."""
    a, ast = lit(rend, "A")
    b, bst = lit(rend, "A")
    assert_same(a, reference("A"))
    assert_same(b, a)
    for k in STAT_KEYS:
        assert ast[k] == bst[k]
    assert_same(lit(rend, "AO")[0], reference("AO"))
    assert_same(lit(rend, "A")[0], reference("A"))


@pytest.mark.parametrize("W,H,hits", [(1, 1, 0), (7, 3, 15), (64, 1, 51), (65, 5, 231)])
def test_ragged_frames(rend, W, H, hits):
    """A lone pixel, partial tiles, one full wave, partial waves: case B's view."""
    _, _, steps = setup(rend, "B")
    ref = light_ref.render(network("plane_1")[3], W, H, view("B")[0], steps, LIGHT_DIR, 64, scene=0, frame=FRAME, **LIGHT)
    assert int((ref["gbuffer"]["status"] == HIT).sum()) == hits
    out, ao, sh, st = rend.render_lit(W, H, LIGHT_DIR, max_steps=steps, buffers=True, with_stats=True, **LIGHT)
    assert_same({"out": out, "ao": ao, "shadow": sh}, ref)
    for k in STAT_KEYS:
        assert st[k] == ref["stats"][k], (k, st, ref["stats"])


def test_a_view_without_hits(rend):
    """The eye at (0, 0, 2) looking away from the model: every ray crosses the bounding sphere and
    leaves it."""
    away = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 2], np.float32)
    rend.set_view(away, NM, FRAME).set_scene("v1")
    out, ao, sh, st = rend.render_lit(16, 8, LIGHT_DIR, max_steps=128, buffers=True, with_stats=True, **LIGHT)
    assert not out.any() and (ao == 1).all() and (sh == 1).all()
    assert st["rays_hit"] == 128 and st["rays_shaded"] == 0 and st["shade_evals"] == 0 and st["ray_steps"] == 128


def test_a_light_behind_every_surface():
    """The plane z = 0 seen from +z and lit from -z: ndl is 0 at every hit, so the shadow is 0
    everywhere on it and no shadow ray is marched."""
    dims, K, B = designed_nets.linear_net((0.0, 0.0, 1.0))
    W, H, steps, L = 32, 24, 64, (0.0, 0.0, -1.0)
    ref = light_ref.render(oracle.OracleNet(K, B), W, H, IV, steps, L, 64, scene=nr.NR_SCENE["tanh"], frame=FRAME, **LIGHT)
    hit = ref["gbuffer"]["status"] == HIT
    assert hit.sum() >= 100 and ref["ray_pix"].size == 0 and not ref["shadow"].reshape(-1)[hit].any()
    with nr.Renderer(0) as r:
        r.load_mlp(dims, K, B).set_static(nr.NR_COLOR_FACING, 3).set_scene("tanh").set_view(IV, NM, FRAME)
        out, ao, sh, st = r.render_lit(W, H, L, max_steps=steps, buffers=True, with_stats=True, **LIGHT)
        _, gst = r.render_gbuffer(W, H, steps, with_stats=True)
    assert_same({"out": out, "ao": ao, "shadow": sh}, ref)
    assert st["ray_steps"] == gst["ray_steps"] == ref["stats"]["ray_steps"]


def test_one_effect_at_a_time(rend):
    """ao_strength = 0 with shadows on: ao is 1 and its evaluations are not counted; shadow_steps = 0
    with occlusion on: shadow is 1 and no shadow ray adds a step."""
    ref = reference("A", 64, ao_strength=0.0)
    got, st = lit(rend, "A", 64, ao_strength=0.0)
    assert_same(got, ref)
    assert (got["ao"] == 1).all() and st["shade_evals"] == 4 * st["rays_shaded"] == ref["stats"]["shade_evals"]
    assert st["ray_steps"] == ref["stats"]["ray_steps"]
    ref = reference("A", 0)
    got, st = lit(rend, "A", 0)
    assert_same(got, ref)
    assert (got["shadow"] == 1).all() and st["shade_evals"] == 8 * st["rays_shaded"]
    assert st["ray_steps"] == ref["stats"]["ray_steps"] == int(ref["gbuffer"]["steps"].sum())


# ---- 6. the context is left alone

def test_context_settings_ignored_and_preserved(rend):
    """In a bf16 context on the wavefront schedule the call gives what an fp32 persistent context
    gives, and the context's own frame is the same before and after it."""
    W, H, steps = setup(rend, "A")
    fp32, _ = rend.render(W, H, steps)
    try:
        rend.set_precision("bf16").set_schedule("wavefront")
        before, bst = rend.render(W, H, steps)
        got, st = lit(rend, "A")
        after, ast = rend.render(W, H, steps)
    finally:
        rend.set_precision("fp32").set_schedule("persistent")
    assert_same(got, reference("A"))
    assert np.array_equal(after, before)
    for k in STAT_KEYS:
        assert ast[k] == bst[k], k
    # (the bf16 frame is not the fp32 one: the setting was in force around the call)
    assert not np.array_equal(before, fp32)
    g = rend.render_gbuffer(W, H, steps)  # the view is the one set before the call
    assert np.array_equal(g["status"].reshape(-1), reference("A")["gbuffer"]["status"])


# ---- 7. errors

def test_errors(rend):
    L = nr.lib()
    buf = np.zeros(64, np.uint32)
    fb = np.zeros(64, np.float32)
    W, H, steps = setup(rend, "A")

    def call(r, out=buf.ctypes.data, ao=None, shadow=None, W=4, H=4, steps=10, light=True, **kw):
        f = dict(LIGHT, light_dir=LIGHT_DIR, shadow_steps=8)
        f.update(kw)
        lt = nr.Renderer._light(**f)
        return L.nr_render_lit(r._ctx if r is not None else None, out, W, H, steps, ctypes.byref(lt) if light else None,
                               ao, shadow, 0, None)

    assert call(rend) == 0
    assert call(rend, out=None, ao=fb.ctypes.data) == 0 and call(rend, out=None, shadow=fb.ctypes.data) == 0
    assert call(None) == -1 and call(rend, light=False) == -1  # NR_E_INVALID
    assert call(rend, out=None) == -1
    assert call(rend, W=0) == -1 and call(rend, H=0) == -1 and call(rend, W=-3) == -1
    assert call(rend, W=(1 << 15) + 1, H=1 << 15) == -1 and call(rend, W=(1 << 30) + 1, H=1) == -1
    assert call(rend, steps=0) == -1 and call(rend, steps=-1) == -1
    assert call(rend, shadow_steps=-1) == -1
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(rend, light_dir=(bad, 0.0, 1.0)) == -1 and call(rend, light_dir=(0.0, 1.0, bad)) == -1
        for field in ("shadow_bias", "shadow_k", "ao_step", "ao_strength", "ambient"):
            assert call(rend, **{field: bad}) == -1, (field, bad)
    assert call(rend, light_dir=(0.0, 0.0, 0.0)) == -1 and call(rend, light_dir=(0.0, -0.0, 0.0)) == -1
    assert call(rend, shadow_k=-1.0) == -1 and call(rend, ao_step=-0.01) == -1 and call(rend, ao_strength=-2.0) == -1
    assert call(rend, ambient=-0.1) == -1 and call(rend, ambient=1.5) == -1
    assert call(rend, shadow_bias=-0.01) == 0 and call(rend, ambient=0.0) == 0 and call(rend, ambient=1.0) == 0
    with nr.Renderer(0) as r:
        assert call(r) == -5  # NR_E_STATE: no network
        rng = np.random.default_rng(0)
        r.load_mlp([3, 16, 1], [rng.normal(size=(3, 16)).astype(np.float32), rng.normal(size=(16, 1)).astype(np.float32)],
                   [np.zeros(16, np.float32), np.zeros(1, np.float32)])
        assert call(r) == -4  # NR_E_FORMAT: not a network of the fused kernels, and no layered fallback
        assert L.nr_render(r._ctx, buf.ctypes.data, 4, 4, 10, 0, None) == 0
    # a following valid call still works
    assert_same(lit(rend, "A")[0], reference("A"))
