"""nr_compose_render_lit on the GPU (nr_compose_light.hip) against tests/compose_light_ref.py, the
numpy restatement of its contract (pinned by tests/test_compose_light_cpu.py), against the library's
own composed ray queries, against nr_compose_render and against nr_render_lit for a lone identity
part.  Every comparison is exact: frames and maps as integers, ao and shadow on their uint32 views."""
import ctypes

import numpy as np
import pytest
import torch

import compose_light_ref
import cudaneuralrender_amd as nr
from cudaneuralrender_amd import _lib
import designed_nets
import light_ref
import oracle
from compose_light_cases import LIGHT, LIGHT_DIR, NM, SCENES, eye_at, network, reference
from compose_ref import part
from query_ref import ESCAPED, HIT, LIMIT, MISS

pytestmark = pytest.mark.gpu
F = np.float32
BUFS = ("out", "ao", "shadow", "part", "occluder")
STAT_KEYS = ("ray_steps", "shade_evals", "rays_hit", "rays_shaded", "iterations", "part_evals")
DTYPES = {"out": np.uint32, "ao": np.float32, "shadow": np.float32, "part": np.int32, "occluder": np.int32}
# where torch bundles a HIP runtime of its own beside libnr's, torch has to open the GPU first
if torch.cuda.is_available():
    torch.cuda.init()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, ref, keys=BUFS):
    for k in keys:
        g, r = got[k], ref[k]
        assert g.shape == r.shape and g.dtype == r.dtype, (k, g.shape, r.shape, g.dtype, r.dtype)
        bad = bits(g) != bits(r)
        assert not bad.any(), f"{k}: {int(bad.sum())} of {bad.size} values differ, first pixel {np.argwhere(bad)[0]}"


@pytest.fixture(scope="module")
def sources():
    """One renderer per network of the scenes, in scene tanh."""
    out = {}
    for g in ("plane_1", "plane_2", "plane_3", "car_1", "plane_1x4"):
        dims, K, B, _ = network(g)
        r = nr.Renderer(0)
        r.load_mlp(dims, K, B).set_precision("fp32").set_static(nr.NR_COLOR_FACING, dims[0]).set_scene("tanh")
        out[g] = r
    yield out
    for r in out.values():
        r.close()


@pytest.fixture(scope="module")
def scenes(sources):
    """(owner, composition) per scene: the owner has no network, only the scene's view and frame."""
    out = {}
    for k, (names, parts, iv, steps, frame, ld) in SCENES.items():
        owner = nr.Renderer(0)
        owner.set_static(nr.NR_COLOR_FACING, 3).set_view(iv, NM, frame)
        out[k] = (owner, nr.Composition(owner, [sources[g] for g in names], parts))
    yield out
    for owner, comp in out.values():
        comp.close()
        owner.close()


def lit(scenes, scene, W, H, shadow_steps=64, light_dir=None, **kw):
    """render_lit of a scene with the tests' light: ({out, ao, shadow, part, occluder}, stats)."""
    steps, ld = SCENES[scene][3], SCENES[scene][5]
    res = scenes[scene][1].render_lit(W, H, ld if light_dir is None else light_dir, shadow_steps=shadow_steps, max_steps=steps,
                                      buffers=True, with_part=True, with_occluder=True, with_stats=True, **dict(LIGHT, **kw))
    return dict(zip(BUFS, res[:5])), res[5]


def cross_part(r):
    return int(((r["occluder"] >= 0) & (r["occluder"] != r["part"])).sum())


# ---- 1. against the reference

@pytest.mark.parametrize("shadow_steps", [64, 8])
@pytest.mark.parametrize("W,H", [(96, 96), (45, 37)])
def test_l3_against_the_reference(scenes, W, H, shadow_steps):
    ref = reference("l3", W, H, shadow_steps)
    got, st = lit(scenes, "l3", W, H, shadow_steps)
    assert_same(got, ref)
    for k in STAT_KEYS:
        assert st[k] == ref["stats"][k], (k, st, ref["stats"])
    assert st["launches"] == 5 and st["ms_total"] > 0 and st["wave_evals"] > 0


# ---- 2. against the library's own composed queries

@pytest.mark.parametrize("shadow_steps", [64, 8])
def test_hard_shadows_against_trace_rays(scenes, shadow_steps):
    """With shadow_k = 0 the call is gbuffer -> o = p + n * bias on the host -> trace_rays along the
    light: shadow 0 where that ray ends HIT or LIMIT, 1 otherwise, occluder that call's part.  This
    pins k_compose_light to k_compose without the numpy reference."""
    owner, comp = scenes["l3"]
    W, H, steps = 96, 96, SCENES["l3"][3]
    got, st = lit(scenes, "l3", W, H, shadow_steps, shadow_k=0.0)
    g, gst = comp.gbuffer(W, H, steps, with_stats=True)
    L = np.asarray(LIGHT_DIR, F)
    n, p = g["normal"].reshape(-1, 3), g["position"].reshape(-1, 3)
    hit = g["status"].reshape(-1) == HIT
    sel = np.flatnonzero(hit & (light_ref.ndl_of(n, L) > 0))
    assert sel.size >= 500 and sel.size < hit.sum()
    o = (p[sel] + n[sel] * F(LIGHT["shadow_bias"])).astype(F)
    q, qst = comp.trace_rays(o, np.broadcast_to(L, o.shape), shadow_steps, normals=False, with_stats=True)
    blocked = (q["status"] == HIT) | (q["status"] == LIMIT)
    assert int(blocked.sum()) >= 100 and (shadow_steps == 8 or int((~blocked).sum()) >= 300)
    assert np.array_equal(bits(got["shadow"].reshape(-1)[sel]), bits(np.where(blocked, F(0), F(1))))
    assert np.array_equal(got["occluder"].reshape(-1)[sel], q["part"])
    assert np.array_equal(got["part"], g["part"])
    assert st["ray_steps"] - gst["ray_steps"] == qst["ray_steps"]
    assert st["part_evals"] - gst["part_evals"] == qst["part_evals"]
    for k in ("rays_hit", "rays_shaded"):
        assert st[k] == gst[k]


# ---- 3. the light switched off: nr_compose_render's frame

@pytest.mark.parametrize("color", ["facing", "matcap"])
def test_identity(scenes, color):
    owner, comp = scenes["l3"]
    W, H, steps = 96, 96, SCENES["l3"][3]
    try:
        if color == "matcap":
            owner.set_matcap(nr.load_png(nr.matcap_path("Chrome"))).set_static(nr.NR_COLOR_MATCAP, 3)
        frame, owners, _ = comp.render(W, H, steps, with_part=True)
        out, ao, sh, prt, occ = comp.render_lit(W, H, LIGHT_DIR, max_steps=steps, buffers=True, with_part=True,
                                                with_occluder=True, **light_ref.LIGHT_OFF)
    finally:
        owner.set_static(nr.NR_COLOR_FACING, 3)
    assert (frame != 0).sum() >= 1000 and len(np.unique(frame)) >= 20
    assert np.array_equal(out, frame), f"{(out != frame).sum()} pixels differ"
    assert np.array_equal(bits(ao), bits(np.ones((H, W), F))) and np.array_equal(bits(sh), bits(np.ones((H, W), F)))
    assert np.array_equal(prt, owners) and (occ == -1).all()


# ---- 4. a lone identity part is the single-network call

def test_lone_identity_part_occlusion(scenes, sources):
    car = sources["car_1"]
    W, H, steps = 48, 48, SCENES["one"][3]
    car.set_view(SCENES["one"][2], NM, 0)
    _, ao1, _ = car.render_lit(W, H, LIGHT_DIR, max_steps=steps, buffers=True, **LIGHT)
    g1 = car.render_gbuffer(W, H, steps)
    got, _ = lit(scenes, "one", W, H)
    g = scenes["one"][1].gbuffer(W, H, steps)
    both = (g1["status"] == HIT) & (g["status"] == HIT)
    assert int(both.sum()) >= 200 and int((ao1[both] < 1).sum()) >= 100
    assert np.array_equal(bits(got["ao"])[both], bits(ao1)[both])
    assert_same(got, reference("one", W, H))


# ---- 5. grouping and scratch reuse

def test_grouping_and_repeated_calls(scenes):
    """nr_set_occupancy on the owner takes the 256-thread workgroup instead of the 768-thread default
    of a scene with two packs; consecutive calls reuse the composition's scratch."""
    owner, comp = scenes["l3"]
    ref = reference("l3", 45, 37)
    a, ast = lit(scenes, "l3", 45, 37)
    b, bst = lit(scenes, "l3", 45, 37)
    assert_same(a, ref)
    assert_same(b, a)
    try:
        for bpc in (1, 2, 3):
            owner.set_occupancy(bpc)
            c, cst = lit(scenes, "l3", 45, 37)
            assert_same(c, a)
            for k in STAT_KEYS:
                assert cst[k] == ast[k] == bst[k], (bpc, k)
    finally:
        owner.set_occupancy(0)
    # a larger frame after a smaller one and back
    assert_same(lit(scenes, "l3", 96, 96)[0], reference("l3", 96, 96))
    assert_same(lit(scenes, "l3", 45, 37)[0], ref)


# ---- 6. four packs, and a 4-input network that takes the owner's frame

@pytest.mark.parametrize("scene", ["four", "f4"])
def test_other_scenes_against_the_reference(scenes, scene):
    ref = reference(scene, 48, 48)
    assert cross_part(ref) >= 10
    got, st = lit(scenes, scene, 48, 48)
    assert_same(got, ref)
    for k in STAT_KEYS:
        assert st[k] == ref["stats"][k], (k, st, ref["stats"])
    if scene == "four":
        try:
            scenes[scene][0].set_occupancy(1)
            assert_same(lit(scenes, scene, 48, 48)[0], ref)
        finally:
            scenes[scene][0].set_occupancy(0)


# ---- 7. one effect at a time

def test_one_effect_at_a_time(scenes):
    W, H = 45, 37
    ref = reference("l3", W, H, ao_strength=0.0)
    got, st = lit(scenes, "l3", W, H, ao_strength=0.0)
    assert_same(got, ref)
    assert (got["ao"] == 1).all() and st["shade_evals"] == 4 * st["rays_shaded"] == ref["stats"]["shade_evals"]
    assert st["ray_steps"] == ref["stats"]["ray_steps"]
    ref = reference("l3", W, H, 0)
    got, st = lit(scenes, "l3", W, H, 0)
    assert_same(got, ref)
    assert (got["shadow"] == 1).all() and (got["occluder"] == -1).all() and st["shade_evals"] == 8 * st["rays_shaded"]
    assert st["ray_steps"] == ref["stats"]["ray_steps"] == int(ref["gbuffer"]["steps"].sum())


def test_a_light_behind_every_surface():
    """The plane z = 0 seen from +z and lit from -z: ndl is 0 at every hit, so the shadow is 0
    everywhere on it, no shadow ray is marched and ray_steps is the geometry buffer's."""
    dims, K, B = designed_nets.linear_net((0.0, 0.0, 1.0))
    W, H, steps, L = 32, 24, 64, (0.0, 0.0, -1.0)
    parts = [part(0)]
    c, r = nr.compose_bound(parts, 1)
    ref = compose_light_ref.render([oracle.OracleNet(K, B)], parts, c, r, W, H, eye_at(2.0), steps, L, 64, **LIGHT)
    hit = ref["gbuffer"]["status"] == HIT
    assert hit.sum() >= 100 and ref["ray_pix"].size == 0 and not ref["shadow"].reshape(-1)[hit].any()
    with nr.Renderer(0) as src:
        src.load_mlp(dims, K, B).set_static(nr.NR_COLOR_FACING, 3).set_view(eye_at(2.0), NM, 0)
        with nr.Composition(src, [src], parts) as comp:
            out, ao, sh, prt, occ, st = comp.render_lit(W, H, L, max_steps=steps, buffers=True, with_part=True,
                                                        with_occluder=True, with_stats=True, **LIGHT)
            _, gst = comp.gbuffer(W, H, steps, with_stats=True)
    assert_same({"out": out, "ao": ao, "shadow": sh, "part": prt, "occluder": occ}, ref)
    assert st["ray_steps"] == gst["ray_steps"] == ref["stats"]["ray_steps"]
    assert st["part_evals"] == gst["part_evals"]


def test_a_view_without_hits(scenes):
    """The eye at (0, 0, 2.4) looking away from the parts: every ray crosses the bound and leaves it."""
    owner, comp = scenes["l3"]
    away = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 2.4], F)
    try:
        owner.set_view(away, NM, 0)
        out, ao, sh, prt, occ, st = comp.render_lit(16, 8, LIGHT_DIR, max_steps=96, buffers=True, with_part=True,
                                                    with_occluder=True, with_stats=True, **LIGHT)
    finally:
        owner.set_view(SCENES["l3"][2], NM, 0)
    assert not out.any() and (ao == 1).all() and (sh == 1).all() and (prt == -1).all() and (occ == -1).all()
    assert st["rays_hit"] == 128 and st["rays_shaded"] == 0 and st["shade_evals"] == 0 and st["ray_steps"] == 128


# ---- 8. outputs and locations

def raw(comp, W, H, steps, want, device):
    """nr_compose_render_lit through the C ABI with the outputs named in `want` only (the others
    NULL), into host arrays or torch tensors on cuda:0.  Returns (rc, {name: numpy array})."""
    lt = nr.Renderer._light(LIGHT_DIR, 64, **LIGHT)
    if device:
        bufs = {k: torch.full((H, W), 0x55555555, dtype=torch.int32, device="cuda:0") for k in want}
        ptr = {k: ctypes.c_void_p(v.data_ptr()) for k, v in bufs.items()}
        torch.cuda.synchronize()  # (the fills ran on torch's stream, the call runs on the owner's)
    else:
        bufs = {k: np.full((H, W), 0x55555555, np.uint32).view(DTYPES[k]) for k in want}
        ptr = {k: v.ctypes.data for k, v in bufs.items()}
    rc = comp._L.nr_compose_render_lit(comp._c, ptr.get("out"), W, H, steps, ctypes.byref(lt), ptr.get("ao"), ptr.get("shadow"),
                                       ptr.get("part"), ptr.get("occluder"), _lib.NR_DEVICE if device else _lib.NR_HOST, None)
    if device:
        comp.owner.synchronize()
        bufs = {k: v.cpu().numpy().view(DTYPES[k]) for k, v in bufs.items()}
    return rc, bufs


WANTS = [BUFS, ("out",), ("ao",), ("shadow",), ("out", "ao"), ("out", "shadow"), ("ao", "shadow"), ("out", "part"),
         ("ao", "occluder"), ("shadow", "part", "occluder"), ("out", "ao", "shadow", "occluder")]


@pytest.mark.parametrize("device", [False, True])
def test_host_device_and_null_outputs(scenes, device):
    owner, comp = scenes["l3"]
    W, H, steps = 45, 37, SCENES["l3"][3]
    ref = reference("l3", W, H)
    for want in WANTS:
        rc, got = raw(comp, W, H, steps, want, device)
        assert rc == 0, (comp._L.nr_last_error(owner._ctx), want, device)
        assert_same(got, ref, want)


def test_device_outputs_on_a_caller_stream(scenes):
    owner, comp = scenes["l3"]
    W, H, steps = 45, 37, SCENES["l3"][3]
    ref = reference("l3", W, H)
    dev = torch.device("cuda:0")
    t = {k: torch.full((H, W), 0x55555555, dtype=torch.int32, device=dev) for k in BUFS}
    stream = torch.cuda.Stream(dev)
    try:
        with torch.cuda.stream(stream):
            owner.set_stream(stream.cuda_stream)
            comp.render_lit_device(t["out"].data_ptr(), W, H, LIGHT_DIR, max_steps=steps, ao_ptr=t["ao"].data_ptr(),
                                   shadow_ptr=t["shadow"].data_ptr(), part_ptr=t["part"].data_ptr(),
                                   occluder_ptr=t["occluder"].data_ptr(), **LIGHT)
            owner.synchronize()
        stream.synchronize()
    finally:
        owner.set_stream(None, own=True)
    assert_same({k: v.cpu().numpy().view(DTYPES[k]) for k, v in t.items()}, ref)


# ---- 9. set_parts

def test_set_parts_moves_the_shadow(sources):
    """The plane that shades the car, moved out of the light's way: the cross-part occluders go, and
    the composition needs nothing from its sources for that (they are closed: no pack is uploaded)."""
    names, parts, iv, steps, frame, ld = SCENES["l3"]
    W, H = 45, 37
    moved = [dict(p) for p in parts]
    moved[1]["pos"] = np.array([0.0, -2.6, 0.0], F)
    srcs = []
    for g in names:
        dims, K, B, _ = network(g)
        srcs.append(nr.Renderer(0).load_mlp(dims, K, B))
    with nr.Renderer(0) as owner:
        owner.set_static(nr.NR_COLOR_FACING, 3).set_view(iv, NM, frame)
        with nr.Composition(owner, srcs, parts) as comp:
            for r in srcs:
                r.close()
            kw = dict(max_steps=steps, buffers=True, with_part=True, with_occluder=True, **LIGHT)
            before = dict(zip(BUFS, comp.render_lit(W, H, ld, **kw)))
            assert_same(before, reference("l3", W, H))
            comp.set_parts(moved)
            after = dict(zip(BUFS, comp.render_lit(W, H, ld, **kw)))
            with nr.Composition(owner, [sources[g] for g in names], moved) as fresh:
                assert_same(after, dict(zip(BUFS, fresh.render_lit(W, H, ld, **kw))))
    # before: 17 pixels in the shadow of another part (18 blocked by the plane); after: none, the plane blocks nothing
    assert cross_part(before) >= 10 and cross_part(after) == 0
    hist = [np.bincount(r["occluder"].reshape(-1) + 1, minlength=4).tolist() for r in (before, after)]
    assert hist[0][2] >= 10 and hist[1][2] == 0 and hist[0] != hist[1]


# ---- 10. errors

def test_errors(scenes, sources):
    L = nr.lib()
    owner, comp = scenes["l3"]
    buf = np.zeros(64, np.uint32)
    fb = np.zeros(64, np.float32)
    ib = np.zeros(64, np.int32)

    def call(cp, out=buf.ctypes.data, ao=None, shadow=None, prt=None, occ=None, W=4, H=4, steps=10, light=True, **kw):
        f = dict(LIGHT, light_dir=LIGHT_DIR, shadow_steps=8)
        f.update(kw)
        lt = nr.Renderer._light(**f)
        return L.nr_compose_render_lit(cp._c if cp is not None else None, out, W, H, steps, ctypes.byref(lt) if light else None,
                                       ao, shadow, prt, occ, 0, None)

    assert call(comp) == 0
    assert call(comp, out=None, ao=fb.ctypes.data) == 0 and call(comp, out=None, shadow=fb.ctypes.data) == 0
    assert call(None) == -1 and call(comp, light=False) == -1  # NR_E_INVALID
    assert call(comp, out=None) == -1
    assert call(comp, out=None, prt=ib.ctypes.data, occ=ib.ctypes.data) == -1  # none of out, ao, shadow
    assert call(comp, W=0) == -1 and call(comp, H=0) == -1 and call(comp, W=-3) == -1
    assert call(comp, W=(1 << 15) + 1, H=1 << 15) == -1 and call(comp, W=(1 << 30) + 1, H=1) == -1
    assert call(comp, steps=0) == -1 and call(comp, steps=-1) == -1
    assert call(comp, shadow_steps=-1) == -1
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(comp, light_dir=(bad, 0.0, 1.0)) == -1 and call(comp, light_dir=(0.0, 1.0, bad)) == -1
        for field in ("shadow_bias", "shadow_k", "ao_step", "ao_strength", "ambient"):
            assert call(comp, **{field: bad}) == -1, (field, bad)
    assert call(comp, light_dir=(0.0, 0.0, 0.0)) == -1 and call(comp, light_dir=(0.0, -0.0, 0.0)) == -1
    assert call(comp, shadow_k=-1.0) == -1 and call(comp, ao_step=-0.01) == -1 and call(comp, ao_strength=-2.0) == -1
    assert call(comp, ambient=-0.1) == -1 and call(comp, ambient=1.5) == -1
    assert b"nr_compose_render_lit" in L.nr_last_error(owner._ctx)
    assert call(comp, shadow_bias=-0.01) == 0 and call(comp, ambient=0.0) == 0 and call(comp, ambient=1.0) == 0
    # matcap colouring without a matcap: an error only where the frame is wanted
    with nr.Renderer(0) as bare:
        bare.set_static(nr.NR_COLOR_MATCAP, 3)
        with nr.Composition(bare, [sources["car_1"]], [part(0)]) as c2:
            assert call(c2) == -5  # NR_E_STATE
            assert call(c2, out=None, ao=fb.ctypes.data, shadow=fb.ctypes.data) == 0
    # a following valid call still works
    assert_same(lit(scenes, "l3", 45, 37)[0], reference("l3", 45, 37))
