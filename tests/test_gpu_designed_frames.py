"""The tracers, the ray queries and the mesh extraction on designed networks (tests/designed_nets.py),
against the CPU oracle bit for bit.

A network whose output does not depend on the point has a zero gradient: the normal is
0 * (1 / sqrt(0)) = NaN, the facing colour is opaque black, a matcap pixel is texel [0, 0], and with
a surface value below the marching epsilon every ray that enters the bounding sphere converges at
iteration 0.  No trained network renders that.  The flat fields (const_net(0), const_net(5e-7)), an
escaping field (const_net(0.3)) and a planar one (linear_net((0, 0, 1), 0.25)) run through k_trace,
k_march16 / k_shade16, the layered kernels, k_query and k_vnormal; what the frames must hold is
asserted literally as well as against the oracle.
"""
import functools

import numpy as np
import pytest

import cudaneuralrender_amd as nr
import designed_nets as dn
import mesh_ref
import oracle
import query_ref
from query_ref import ESCAPED, HIT

pytestmark = pytest.mark.gpu
F = np.float32
W, H, STEPS = 96, 80, 64
CAM = (-15.0, 30.0, 3.0)  # the bounding sphere leaves the frame's corners free
CAMS3 = (CAM, (10.0, 200.0, 8.0), (0.0, 75.0, 1.0))  # ordinary, zoomed out, eye inside the sphere
BLACK = 0xff000000
TEXEL00 = 0xff123456  # texel [0, 0] of this module's matcap: unlike opaque black, unlike every other texel
STAT_KEYS = ("ray_steps", "shade_evals", "rays_hit", "rays_shaded", "iterations")
SCHEDULES = ("persistent", "wavefront", "layered")
COLOR = {"facing": nr.NR_COLOR_FACING, "matcap": nr.NR_COLOR_MATCAP}


@functools.lru_cache(maxsize=None)
def matcap():
    m = dn.coded_matcap(6, 9)
    m[0, 0] = TEXEL00
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def ref_frame(net, scene, color, cam=CAM):
    """The oracle's frame and statistics (computed once per case; read-only)."""
    _, K, B = (dn.const_net if net[0] == "const" else dn.linear_net)(*net[1:])
    iv, nm = nr.camera(*cam)
    img, st = oracle.OracleNet(K, B).render(W, H, iv, nm, color_type=COLOR[color], scene=nr.NR_SCENE[scene],
                                            matcap=matcap() if color == "matcap" else None, max_steps=STEPS)
    img.setflags(write=False)
    return img, st


@pytest.fixture(scope="module")
def rend():
    r = nr.Renderer(0)
    yield r
    r.close()


def setup(rend, net, scene, color, precision="fp32", schedule="persistent", cam=CAM):
    dims, K, B = (dn.const_net if net[0] == "const" else dn.linear_net)(*net[1:])
    rend.load_mlp(dims, K, B).set_precision(precision).set_schedule(schedule)
    rend.set_static(COLOR[color], 3).set_scene(scene).set_matcap(matcap()).set_view(*nr.camera(*cam), 0)


def same_or_nan(got, ref):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    if got.dtype != F:
        return bool((got == ref).all())
    return bool(np.where(np.isnan(ref), np.isnan(got), got.view(np.uint32) == ref.view(np.uint32)).all())


FLAT = [(c, scene, color) for c in (0.0, 5e-7) for scene in ("tanh", "v1") for color in ("facing", "matcap")]


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("c,scene,color", FLAT)
def test_flat_field(rend, c, scene, color, schedule):
    ref, rst = ref_frame(("const", c), scene, color)
    # every ray that enters the sphere converges at iteration 0; with tanh the gradient is zero everywhere
    assert rst["ray_steps"] == rst["rays_hit"] == rst["rays_shaded"] and rst["iterations"] == 2
    assert W * H > rst["rays_hit"] > 1000  # and some rays miss the bounding sphere
    try:
        setup(rend, ("const", c), scene, color, schedule=schedule)
        img, st = rend.render(W, H, STEPS)
    finally:
        rend.set_schedule("persistent")
    assert int((img != 0).sum()) == rst["rays_hit"]
    if scene == "tanh":  # NaN normal: opaque black (facing) or texel [0, 0] of the matcap
        assert set(np.unique(img).tolist()) == {0, TEXEL00 if color == "matcap" else BLACK}
    assert np.array_equal(img, ref), int((img != ref).sum())
    for k in STAT_KEYS:
        assert st[k] == rst[k], (k, st, rst)


@pytest.mark.parametrize("c,scene", [(0.0, "tanh"), (5e-7, "v1")])
def test_flat_field_batch(rend, c, scene):
    setup(rend, ("const", c), scene, "matcap")
    imgs, st = rend.render_batch(W, H, [(*nr.camera(*cam), 0) for cam in CAMS3], STEPS)
    refs = [ref_frame(("const", c), scene, "matcap", cam) for cam in CAMS3]
    assert refs[2][1]["rays_hit"] == W * H  # from inside the sphere every ray enters
    for img, (ref, _), cam in zip(imgs, refs, CAMS3):
        assert np.array_equal(img, ref), (cam, int((img != ref).sum()))
    for k in STAT_KEYS[:4]:
        assert st[k] == sum(r[1][k] for r in refs), k


@pytest.mark.parametrize("endgame", [0.0, nr._lib.NR_ENDGAME_DEFAULT])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_flat_field_16bit_schedules_agree(rend, prec, endgame):
    try:
        rend.set_endgame(endgame)
        for c, scene, color in FLAT:
            setup(rend, ("const", c), scene, color, precision=prec, schedule="wavefront")
            a, sa = rend.render(W, H, STEPS)
            rend.set_schedule("persistent")
            b, sb = rend.render(W, H, STEPS)
            assert np.array_equal(a, b), (c, scene, color, int((a != b).sum()))
            for k in STAT_KEYS[:4]:
                assert sa[k] == sb[k], (c, scene, color, k, sa, sb)
            assert int((a != 0).sum()) == sa["rays_hit"] == ref_frame(("const", c), scene, color)[1]["rays_hit"]
            if scene == "tanh":
                assert set(np.unique(a).tolist()) == {0, TEXEL00 if color == "matcap" else BLACK}
    finally:
        rend.set_endgame(nr._lib.NR_ENDGAME_DEFAULT).set_precision("fp32").set_schedule("persistent")


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_escaping_field(rend, schedule):
    ref, rst = ref_frame(("const", 0.3), "tanh", "facing")
    assert not ref.any() and rst["rays_shaded"] == 0 and rst["ray_steps"] > 3 * rst["rays_hit"] > 3000
    try:
        setup(rend, ("const", 0.3), "tanh", "facing", schedule=schedule)
        img, st = rend.render(W, H, STEPS)
    finally:
        rend.set_schedule("persistent")
    assert not img.any()
    for k in STAT_KEYS:
        assert st[k] == rst[k], (k, st, rst)


@functools.lru_cache(maxsize=None)
def planar_reference():
    _, K, B = dn.linear_net((0.0, 0.0, 1.0), 0.25)
    O, D = query_ref.pixel_rays(W, H, nr.camera(*CAM)[0])
    out, st = query_ref.trace(oracle.OracleNet(K, B), O, D, STEPS, scene=nr.NR_SCENE["tanh"], frame=0)
    for a in out.values():
        a.setflags(write=False)
    return out, st


def test_planar_field_gbuffer(rend):
    ref, rst = planar_reference()
    hit = ref["status"] == HIT
    assert hit.sum() > 1000
    setup(rend, ("linear", (0.0, 0.0, 1.0), 0.25), "tanh", "facing")
    g, st = rend.render_gbuffer(W, H, STEPS, with_stats=True)
    for k in ("status", "steps", "t", "position", "normal"):
        assert same_or_nan(g[k].reshape(ref[k].shape), ref[k]), k
    for k in STAT_KEYS:
        assert st[k] == rst[k], (k, st, rst)
    n = g["normal"].reshape(-1, 3)[hit]
    assert np.abs(n - np.array([0, 0, 1], F)).max() < 1e-3
    assert np.abs(g["position"].reshape(-1, 3)[hit][:, 2] + 0.25).max() < 1e-5  # the plane z = -0.25


def designed_rays():
    """100 rays from inside the bounding sphere (radius 1.2), a third of them not unit length."""
    rng = np.random.default_rng(11)
    o = rng.normal(size=(100, 3))
    o *= (rng.uniform(0.05, 1.1, (100, 1)) / np.linalg.norm(o, axis=1, keepdims=True))
    d = rng.normal(size=(100, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[::3] *= 0.5
    return o.astype(F), d.astype(F)


@pytest.mark.parametrize("scene", ["tanh", "v1"])
@pytest.mark.parametrize("c", [0.0, 0.3, -0.2])
def test_trace_rays_constant_field(rend, c, scene):
    _, K, B = dn.const_net(c)
    o, d = designed_rays()
    ref, rst = query_ref.trace(oracle.OracleNet(K, B), o, d, STEPS, scene=nr.NR_SCENE[scene], frame=0)
    if scene == "tanh":
        if c == 0.3:
            assert (ref["status"] == ESCAPED).all() and ref["steps"].min() >= 1
        else:  # the first step is below the marching epsilon: a hit at iteration 0, NaN normal
            assert (ref["status"] == HIT).all() and (ref["steps"] == 1).all() and np.isnan(ref["normal"]).all()
        if c == 0.0:
            assert same_or_nan(ref["position"], o) and not ref["t"].any()  # p = o
    setup(rend, ("const", c), scene, "facing")
    out, st = rend.trace_rays(o, d, STEPS, with_stats=True)
    for k in ("status", "steps", "t", "position", "normal"):
        assert same_or_nan(out[k], ref[k]), k
    for k in STAT_KEYS:
        assert st[k] == rst[k], (k, st, rst)
    bare, bst = rend.trace_rays(o, d, STEPS, normals=False, with_stats=True)  # normal = NULL
    assert "normal" not in bare and bst["shade_evals"] == 0
    for k in ("status", "steps", "t", "position"):
        assert same_or_nan(bare[k], ref[k]), k


def test_extract_mesh_exact_plane(rend):
    """linear_net((0, 0, 1)) is z: the lattice plane z = 0 is exactly iso, so it counts as outside, and
    every vertex lies on it (t = 1 on the edges from z = -0.125)."""
    origin, step, dims = (-0.3, -0.25, -0.25), (0.12, 0.13, 0.125), (6, 5, 4)
    _, K, B = dn.linear_net((0.0, 0.0, 1.0), 0.0)
    net = oracle.OracleNet(K, B)
    sdf = mesh_ref.sample(net, origin, step, dims, scene=nr.NR_SCENE["tanh"], frame=0)
    assert (sdf[2] == 0).all() and (sdf[:2] < 0).all() and (sdf[3] > 0).all()
    rV, rT, cells, keys = mesh_ref.mesh(sdf, origin, step, 0.0)
    rN = mesh_ref.normals(net, rV, scene=nr.NR_SCENE["tanh"], frame=0)
    assert len(rV) > 30 and len(rT) == 8 * 5 * 4 and (rV[:, 2] == 0).all() and not np.isnan(rN).any()
    setup(rend, ("linear", (0.0, 0.0, 1.0), 0.0), "tanh", "facing")
    out, st = rend.extract_mesh(origin, step, dims, with_stats=True)
    V, T, N = out["vertices"], out["triangles"], out["normals"]
    assert (len(V), len(T)) == (len(rV), len(rT))
    assert same_or_nan(V, rV) and same_or_nan(N, rN)
    assert T.dtype == np.int32 and T.min() >= 0 and T.max() < len(rV)
    assert mesh_ref.cell_sets(T, mesh_ref.triangle_cells(T, keys, dims)) == mesh_ref.cell_sets(rT, cells)
    assert np.abs(N - np.array([0, 0, 1], F)).max() < 1e-3
    assert (st["ray_steps"], st["rays_shaded"], st["shade_evals"]) == (6 * 5 * 4, len(rV), 4 * len(rV))
