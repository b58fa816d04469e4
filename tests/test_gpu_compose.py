"""Composed scenes on the GPU (nr_compose_*, nr_compose.hip) against tests/compose_ref.py, the numpy
restatement of the contract (pinned to query_ref by tests/test_compose_cpu.py), and against the
single-network calls for a lone identity part.  The field is fp32 and the contract is bit-exactness:
every comparison is on uint32 views."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import compose_ref
import cudaneuralrender_amd as nr
import oracle
import query_ref
import test_gpu_query
from compose_ref import SUBTRACT, UNION, part, rot_xyz
from query_ref import ESCAPED, HIT, LIMIT, MISS

pytestmark = pytest.mark.gpu
F = np.float32
KEYS = ("status", "steps", "t", "position", "normal", "part")
STAT_KEYS = ("ray_steps", "shade_evals", "rays_hit", "rays_shaded", "iterations", "part_evals")
GEOMS = ("plane_1", "plane_2", "plane_3", "car_1")
if torch.cuda.is_available():
    torch.cuda.init()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, ref, rows=None, keys=KEYS):
    for k in keys:
        r = ref[k] if rows is None else ref[k][rows]
        g = got[k]
        assert g.shape == r.shape and g.dtype == r.dtype, (k, g.shape, r.shape, g.dtype)
        bad = bits(g) != bits(r)
        assert not bad.any(), f"{k}: {int(bad.sum())} of {bad.size} values differ, first ray {np.argwhere(bad)[0]}"


def counts(status):
    return [int(v) for v in np.bincount(status, minlength=4)]


@functools.lru_cache(maxsize=None)
def onet(name):
    dims, K, B = nr.read_keras_h5(nr.geometry_path(name))
    return oracle.OracleNet(K, B)


@pytest.fixture(scope="module")
def rends(nets):
    """One renderer per bundled geometry used here, each a possible source or owner."""
    out = {}
    for g in GEOMS:
        dims, K, B = nets[g]
        r = nr.Renderer(0)
        r.load_mlp(dims, K, B).set_precision("fp32").set_static(nr.NR_COLOR_FACING, 3).set_scene("tanh")
        r.set_view(*nr.camera(0.0, 0.0, 2.0), 0)
        out[g] = r
    yield out
    for r in out.values():
        r.close()


# ---- scene S3: nets (plane_1, car_1)
S3_NETS = ("plane_1", "car_1")
S3 = [part(0, UNION, None, (-0.9, 0.0, 0.0), 1.0),
      part(1, UNION, rot_xyz(0.3, 1.0, -0.2), (1.0, 0.2, 0.1), 0.75),
      part(1, SUBTRACT, rot_xyz(1.2, 0.4, 0.5), (-0.9, 0.0, 0.0), 0.6)]
# two parts with disjoint bounds, and four networks spread out
TWO_NETS = ("plane_1", "car_1")
TWO = [part(0, UNION, None, (-1.5, 0.0, 0.0), 1.0), part(1, UNION, rot_xyz(0.0, 0.7, 0.0), (1.5, 0.1, 0.0), 1.0)]
FOUR_NETS = GEOMS
FOUR = [part(i, UNION, rot_xyz(0.1 * i, 0.2, 0.3 * i), p, s)
        for i, (p, s) in enumerate([((-1.5, 0.9, 0.0), 0.8), ((1.4, 1.0, 0.2), 1.0), ((-1.3, -1.0, -0.3), 0.9), ((1.5, -0.9, 0.1), 1.1)])]
SCENES = {"s3": (S3_NETS, S3), "two": (TWO_NETS, TWO), "four": (FOUR_NETS, FOUR)}


@pytest.fixture(scope="module")
def comps(rends):
    """The three compositions, owned by the plane_1 renderer."""
    out = {k: nr.Composition(rends["plane_1"], [rends[g] for g in names], parts) for k, (names, parts) in SCENES.items()}
    yield out
    for c in out.values():
        c.close()


def bound(scene):
    names, parts = SCENES[scene]
    return nr.compose_bound(parts, len(names))


def scene_rays(scene, n, seed):
    """Origins around the scene, targets inside the parts' bounds (S3: the issue's box), every third
    direction random, all unit length, every second one halved."""
    names, parts = SCENES[scene]
    rng = np.random.default_rng(seed)
    if scene == "s3":
        o = rng.uniform(-3.2, 3.2, (n, 3))
        tgt = rng.uniform(-1.3, 1.3, (n, 3)) * np.array([1.0, 0.4, 0.4])
    else:
        o = rng.uniform(-4.0, 4.0, (n, 3))
        which = rng.integers(0, len(parts), n)
        tgt = np.array([parts[w]["pos"] for w in which], np.float64) + rng.uniform(-0.35, 0.35, (n, 3))
    d = tgt - o
    d[::3] = rng.normal(size=d[::3].shape)
    d = d.astype(F)
    with np.errstate(all="ignore"):
        d = (d / np.sqrt(query_ref.dot3(d, d))[:, None]).astype(F)
    d[1::2] *= F(0.5)
    return o.astype(F), d


RAYS = {"s3": (2000, 39), "two": (600, 22), "four": (600, 23)}


@functools.lru_cache(maxsize=None)
def reference(scene, steps, frame=0):
    """compose_ref.trace on the scene's rays, computed once per case and shared (never modified)."""
    names, parts = SCENES[scene]
    c, r = bound(scene)
    o, d = scene_rays(scene, *RAYS[scene])
    out, st = compose_ref.trace([onet(g) for g in names], parts, c, r, o, d, steps, frame)
    for a in out.values():
        a.setflags(write=False)
    return out, st


# ---- 1. the field
@functools.lru_cache(maxsize=None)
def field_reference():
    c, r = bound("s3")
    rng = np.random.default_rng(4)
    v = rng.normal(size=(4096, 3))
    v *= (rng.uniform(0, 1, (4096, 1)) ** (1 / 3)) / np.linalg.norm(v, axis=1, keepdims=True)
    P = (c.astype(np.float64) + v * float(r) * 1.2).astype(F)
    d, own, pairs = compose_ref.field([onet(g) for g in S3_NETS], S3, P)
    return P, d, own, pairs


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096])
def test_field(comps, n):
    P, d, own, pairs = field_reference()
    c, r = bound("s3")
    dist = np.linalg.norm(P.astype(np.float64) - c, axis=1)
    # the points cover the ground: some outside the bound, every part owning some, both branches of each term
    # (the subtracted part owns only the thin shell where its cut is the surface)
    assert (dist > float(r)).sum() >= 500 and all((own == j).sum() >= m for j, m in enumerate((100, 100, 1)))
    assert 500 <= pairs <= 3 * 4096 - 500
    out, st = comps["s3"].sample(P[:n], with_stats=True)
    assert np.array_equal(bits(out["value"]), bits(d[:n])) and np.array_equal(out["owner"], own[:n])
    if n == 4096:
        assert st["part_evals"] == pairs and st["ray_steps"] == 4096


def test_lattice_samples_feed_mesh_grid(rends, comps):
    """The composed field on the points of a lattice is what nr_mesh_grid takes: the mesh of S3 has
    vertices on the zero set, owned by every part."""
    c, r = bound("s3")
    n = 40
    step = np.full(3, 2 * float(r) / (n - 1), F)
    origin = (c - F(r)).astype(F)
    k, j, i = np.mgrid[0:n, 0:n, 0:n]
    P = np.stack([origin[0] + i.astype(F) * step[0], origin[1] + j.astype(F) * step[1], origin[2] + k.astype(F) * step[2]], -1)
    vals = comps["s3"].sample(P.reshape(-1, 3).astype(F))["value"].reshape(n, n, n)
    V, T = rends["plane_1"].mesh_grid(vals, origin, step)
    assert len(V) >= 200 and len(T) >= 200
    at = comps["s3"].sample(V)
    # an edge is at most sqrt(3) steps long and |grad| of a term is about 1 (0.75 ... 1 scaled): the
    # value at an interpolated crossing stays within an edge length of 0
    assert np.abs(at["value"]).max() <= np.sqrt(3) * float(step[0])
    assert set(at["owner"].tolist()) == {0, 1, 2}


# ---- 2. rays on S3: (max_steps, MISS / ESCAPED / HIT / LIMIT of the reference, hits owned by each part,
# the statuses the case is there for)
S3_CASES = [(300, [391, 1213, 395, 1], [157, 225, 13], (MISS, ESCAPED, HIT)),
            (24, [391, 688, 123, 798], [42, 75, 6], (MISS, ESCAPED, HIT, LIMIT))]


@pytest.mark.parametrize("steps,expect,owners,wanted", S3_CASES)
def test_s3_rays_bitexact(comps, steps, expect, owners, wanted):
    ref, rst = reference("s3", steps)
    cnt = counts(ref["status"])
    own = [int((ref["part"] == j).sum()) for j in range(3)]
    assert cnt == expect and own == owners, (cnt, own)
    # the reference itself covers the ground (not a vacuous comparison)
    assert all(cnt[s] >= 50 for s in wanted), cnt
    assert all(v >= 5 for v in own), own
    assert not np.isnan(ref["normal"]).any()
    o, d = scene_rays("s3", *RAYS["s3"])
    out, st = comps["s3"].trace_rays(o, d, steps, with_stats=True)
    assert_same(out, ref)
    for k in STAT_KEYS:
        assert st[k] == rst[k], (k, st, rst)


# ---- 3. a lone identity part is the single-network tracer
def unit_rays():
    o, d = test_gpu_query.rays()
    with np.errstate(all="ignore"):
        d = (d / np.sqrt(query_ref.dot3(d, d))[:, None]).astype(F)
    return o, d


def test_anchor_rays(rends):
    car = rends["car_1"]
    o, d = unit_rays()
    ref = car.trace_rays(o, d, 300)
    with nr.Composition(car, [car], [part(0)]) as comp:
        info = comp.info()
        assert info["nets"] == 1 and info["parts"] == 1
        assert bits(info["center"]).tolist() == [0, 0, 0] and float(info["radius"]) == float(F(1.2))
        out = comp.trace_rays(o, d, 300)
    cnt = counts(ref["status"])
    assert cnt[HIT] >= 50 and cnt[ESCAPED] >= 50 and cnt[MISS] >= 50, cnt
    assert np.array_equal(out["status"], ref["status"])
    hit = ref["status"] == HIT
    for k in ("steps", "t", "position", "normal"):
        assert np.array_equal(bits(out[k])[hit], bits(ref[k])[hit]), k
        if k != "steps":
            assert not bits(out[k])[~hit].any(), k
    assert np.array_equal(out["part"], np.where(hit, 0, -1))


@pytest.mark.parametrize("W,H,matcap", [(64, 48, False), (32, 16, False), (64, 48, True)])
def test_anchor_frame(rends, W, H, matcap):
    car = rends["car_1"]
    try:
        if matcap:
            car.set_matcap(nr.load_png(nr.matcap_path("Chrome"))).set_static(nr.NR_COLOR_MATCAP, 3)
        ref, rst = car.render(W, H, 300)
        with nr.Composition(car, [car], [part(0)]) as comp:
            img, owner, st = comp.render(W, H, 300, with_part=True)
    finally:
        car.set_static(nr.NR_COLOR_FACING, 3)
    assert (ref != 0).sum() >= 20
    assert np.array_equal(img, ref)
    assert np.array_equal(owner == 0, ref != 0) and np.array_equal(owner == -1, ref == 0)
    assert st["rays_shaded"] == rst["rays_shaded"] and st["rays_hit"] == rst["rays_hit"] and st["launches"] == 3


# ---- 4. culling: parts with disjoint bounds
def test_culling(comps):
    (pa, pb) = TWO
    gap = np.linalg.norm(pa["pos"].astype(np.float64) - pb["pos"]) - np.sqrt(1.45) * (float(pa["scale"]) + float(pb["scale"]))
    assert gap > 0.5  # no point is inside both bounds
    ref, rst = reference("two", 300)
    own = [int((ref["part"] == j).sum()) for j in range(2)]
    assert all(v >= 20 for v in own), own
    o, d = scene_rays("two", *RAYS["two"])
    out, st = comps["two"].trace_rays(o, d, 300, with_stats=True)
    assert_same(out, ref)
    assert st["part_evals"] == rst["part_evals"] and st["ray_steps"] == rst["ray_steps"]
    assert st["part_evals"] < 1.5 * st["ray_steps"]
    assert st["wave_skips"] > 0 and st["wave_evals"] > 0


# ---- 5. four networks: the one-workgroup-per-CU instance
def test_four_networks(comps):
    ref, rst = reference("four", 300)
    own = [int((ref["part"] == j).sum()) for j in range(4)]
    assert all(v >= 5 for v in own), own
    o, d = scene_rays("four", *RAYS["four"])
    info = comps["four"].info()
    c, r = bound("four")
    assert info["nets"] == 4 and np.array_equal(bits(info["center"]), bits(c)) and info["radius"] == r
    out, st = comps["four"].trace_rays(o, d, 300, with_stats=True)
    assert_same(out, ref)
    for k in STAT_KEYS:
        assert st[k] == rst[k], (k, st, rst)


# ---- 6. order and grouping independence
@pytest.mark.parametrize("scene", ["s3", "four"])
def test_occupancy_does_not_change_the_outputs(rends, comps, scene):
    o, d = scene_rays(scene, *RAYS[scene])
    a, ast = comps[scene].trace_rays(o, d, 300, with_stats=True)
    try:
        rends["plane_1"].set_occupancy(1)
        b, bst = comps[scene].trace_rays(o, d, 300, with_stats=True)
    finally:
        rends["plane_1"].set_occupancy(0)
    assert_same(b, a)
    for k in STAT_KEYS:
        assert ast[k] == bst[k], k
    perm = np.random.default_rng(11).permutation(len(o))
    p = comps[scene].trace_rays(o[perm], d[perm], 300)
    assert_same(p, a, perm)


def test_gbuffer_is_trace_rays_on_the_pixel_rays(rends, comps):
    W, H = 40, 24
    owner = rends["plane_1"]
    iv, nm = nr.camera(15.0, 30.0, 4.0)
    try:
        owner.set_view(iv, nm, 0)
        g, gst = comps["s3"].gbuffer(W, H, 300, with_stats=True)
        O, D = query_ref.pixel_rays(W, H, iv)
        q, qst = comps["s3"].trace_rays(O, D, 300, with_stats=True)
        img, part_map, ist = comps["s3"].render(W, H, 300, with_part=True)
    finally:
        owner.set_view(*nr.camera(0.0, 0.0, 2.0), 0)
    assert g["status"].shape == (H, W) and g["normal"].shape == (H, W, 3) and g["part"].shape == (H, W)
    assert len(set(g["part"][g["status"] == HIT].tolist())) >= 2
    assert_same({k: g[k].reshape(q[k].shape) for k in KEYS}, q)
    for k in STAT_KEYS:
        assert gst[k] == qst[k], k
    assert np.array_equal(part_map, g["part"])
    assert np.array_equal(img, query_ref.facing(g["normal"], D, g["status"]).reshape(H, W))


# ---- 7. parts and outputs
def test_set_parts(rends, comps):
    moved = [dict(p) for p in S3]
    moved[1]["pos"] = np.array([0.4, -0.3, 0.2], F)
    moved[2]["op"] = UNION
    moved[2]["scale"] = F(0.5)
    o, d = scene_rays("s3", 300, 31)
    srcs = [rends[g] for g in S3_NETS]
    with nr.Composition(rends["plane_1"], srcs, S3) as comp, nr.Composition(rends["plane_1"], srcs, moved) as fresh:
        before = comp.info()
        base = comp.trace_rays(o, d, 100)
        comp.set_parts(moved)
        after, want = comp.info(), fresh.info()
        c, r = nr.compose_bound(moved, 2)
        assert np.array_equal(bits(after["center"]), bits(c)) and after["radius"] == r
        assert not np.array_equal(bits(after["center"]), bits(before["center"]))
        assert np.array_equal(bits(after["center"]), bits(want["center"])) and after["radius"] == want["radius"]
        a, b = comp.trace_rays(o, d, 100), fresh.trace_rays(o, d, 100)
        assert_same(a, b)
        assert (bits(a["t"]) != bits(base["t"])).sum() >= 20
        # a rejected update leaves the composition as it was
        with pytest.raises(nr.NRError):
            comp.set_parts([part(0, SUBTRACT)])
        assert_same(comp.trace_rays(o, d, 100), b)
        # fewer parts
        comp.set_parts(moved[:1])
        assert comp.info()["parts"] == 1 and set(comp.trace_rays(o, d, 100)["part"].tolist()) <= {-1, 0}


def test_without_normals(comps):
    ref, rst = reference("s3", 300)
    o, d = scene_rays("s3", *RAYS["s3"])
    out, st = comps["s3"].trace_rays(o, d, 300, normals=False, with_stats=True)
    assert "normal" not in out
    assert_same(out, ref, keys=("status", "steps", "t", "position", "part"))
    assert st["shade_evals"] == 0
    for k in ("ray_steps", "rays_hit", "rays_shaded", "iterations", "part_evals"):
        assert st[k] == rst[k], (k, st, rst)


def test_four_input_network_uses_the_owners_frame(rends):
    dims, K, B, net4 = test_gpu_query.plane_net(True)
    parts = [part(0, UNION, rot_xyz(0.2, 0.1, 0.0), (-0.5, 0.0, 0.0), 0.9), part(1, UNION, None, (0.8, 0.0, 0.0), 0.7)]
    c, r = nr.compose_bound(parts, 2)
    o, d = scene_rays("s3", 300, 41)
    refs = [compose_ref.trace([net4, onet("car_1")], parts, c, r, o, d, 200, frame)[0] for frame in (0, 5)]
    assert int((bits(refs[0]["t"]) != bits(refs[1]["t"])).sum()) >= 20
    with nr.Renderer(0) as owner, nr.Renderer(0) as src:
        src.load_mlp(dims, K, B)
        with nr.Composition(owner, [src, rends["car_1"]], parts) as comp:
            for frame, ref in zip((0, 5), refs):
                owner.set_view(*nr.camera(0.0, 0.0, 2.0), frame)
                assert_same(comp.trace_rays(o, d, 200), ref)


def test_errors_that_need_a_device(rends):
    L = nr.lib()
    owner = rends["plane_1"]
    one = nr.make_parts([part(0)])

    def create(srcs, parts=one, nparts=1):
        arr = (ctypes.c_void_p * len(srcs))(*[s._ctx.value if s is not None else None for s in srcs])
        out = ctypes.c_void_p()
        rc = L.nr_compose_create(owner._ctx, arr, len(srcs), parts, nparts, ctypes.byref(out))
        assert (rc == 0) == bool(out)
        if out:
            L.nr_compose_destroy(out)
        return rc

    assert create([owner]) == 0
    assert create([owner] * 5) == -1 and create([]) == -1             # nnets outside 1..4
    assert create([None]) == -1
    assert create([owner], nr.make_parts([part(1)])) == -1             # a net index out of range
    assert b"net 1" in L.nr_last_error(owner._ctx)
    rng = np.random.default_rng(0)
    with nr.Renderer(0) as r:
        assert create([r]) == -5                                        # NR_E_STATE: no network
        r.load_mlp([3, 16, 1], [rng.normal(size=(3, 16)).astype(F), rng.normal(size=(16, 1)).astype(F)],
                   [np.zeros(16, F), np.zeros(1, F)])
        assert create([r]) == -4                                        # NR_E_FORMAT: no fp32 pack
    # three 16-hidden-layer packs (68 KB each) are more LDS than a CU has; two fit
    deep = []
    try:
        for i in range(3):
            dims = [3] + [32] * 17 + [1]
            K = [rng.normal(0, 0.2, (dims[l], dims[l + 1])).astype(F) for l in range(len(dims) - 1)]
            B = [rng.normal(0, 0.05, dims[l + 1]).astype(F) for l in range(len(dims) - 1)]
            deep.append(nr.Renderer(0).load_mlp(dims, K, B))
        assert create(deep[:2]) == 0
        assert create(deep) == -1 and b"LDS" in L.nr_last_error(owner._ctx)
        assert create([deep[0]] * 3) == 0                               # one distinct pack, staged once
    finally:
        for r in deep:
            r.close()
    with nr.Composition(owner, [owner], [part(0)]) as comp:
        z = np.zeros((4, 3), F)
        zp = z.ctypes.data
        st = nr.NRComposeStats()
        assert L.nr_compose_trace_rays(comp._c, zp, zp, (1 << 30) + 1, 10, None, None, None, None, None, None, 0, None) == -1
        assert L.nr_compose_trace_rays(comp._c, zp, zp, -1, 10, None, None, None, None, None, None, 0, None) == -1
        assert L.nr_compose_trace_rays(comp._c, zp, zp, 4, 0, None, None, None, None, None, None, 0, None) == -1
        assert L.nr_compose_trace_rays(comp._c, None, None, 4, 10, None, None, None, None, None, None, 0, None) == -1
        assert L.nr_compose_sample(comp._c, zp, (1 << 30) + 1, None, None, 0, None) == -1
        assert L.nr_compose_sample(comp._c, None, 4, None, None, 0, None) == -1
        assert L.nr_compose_gbuffer(comp._c, 65536, 16385, 10, None, None, None, None, None, None, 0, None) == -1
        assert L.nr_compose_gbuffer(comp._c, 0, 4, 10, None, None, None, None, None, None, 0, None) == -1
        assert L.nr_compose_render(comp._c, None, 4, 4, 10, None, 0, None) == -1
        assert L.nr_compose_render(comp._c, zp, 65536, 16385, 10, None, 0, None) == -1
        # n = 0: NR_OK without a launch; NULL outputs are not written
        assert L.nr_compose_trace_rays(comp._c, None, None, 0, 10, None, None, None, None, None, None, 0, ctypes.byref(st)) == 0
        assert st.launches == 0 and st.ray_steps == 0
        assert L.nr_compose_sample(comp._c, None, 0, None, None, 0, ctypes.byref(st)) == 0 and st.launches == 0
        assert L.nr_compose_trace_rays(comp._c, zp, zp, 4, 10, None, None, None, None, None, None, 0, ctypes.byref(st)) == 0
        assert st.launches == 2
        out = comp.trace_rays(np.zeros((0, 3), F), np.zeros((0, 3), F), 10)
        assert out["status"].shape == (0,) and out["part"].shape == (0,)
    # matcap colouring without a matcap
    with nr.Renderer(0) as bare:
        bare.set_static(nr.NR_COLOR_MATCAP, 3)
        with nr.Composition(bare, [owner], [part(0)]) as comp:
            with pytest.raises(nr.NRError) as e:
                comp.render(8, 8, 10)
            assert e.value.code == -5
            assert comp.gbuffer(8, 8, 10)["status"].shape == (8, 8)
