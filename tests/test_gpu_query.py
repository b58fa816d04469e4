"""Ray queries and geometry buffers on the GPU (nr_trace_rays / nr_render_gbuffer, nr_query.hip)
against tests/query_ref.py, the numpy transposition of the CPU oracle (pinned by
tests/test_query_cpu.py).  The queries always run the fp32 MLP, whose contract is bit-exactness:
every comparison is on uint32 views, so NaN payloads and -0 count."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cudaneuralrender_amd as nr
import oracle
import query_ref
from query_ref import HIT, LIMIT

pytestmark = pytest.mark.gpu
FRAME = 3
KEYS = ("status", "steps", "t", "position", "normal")
STAT_KEYS = ("ray_steps", "shade_evals", "rays_hit", "rays_shaded", "iterations")
# where torch bundles a HIP runtime of its own beside libnr's, torch has to open the GPU first
# (as tools/layered_bench.py does): opened second, it finds no device
if torch.cuda.is_available():
    torch.cuda.init()


@pytest.fixture(scope="module")
def rend(nets):
    dims, K, B = nets["plane_1"]
    r = nr.Renderer(0)
    r.load_mlp(dims, K, B).set_precision("fp32").set_static(nr.NR_COLOR_FACING, 3)
    r.set_view(*nr.camera(0.0, 0.0, 2.0), FRAME)
    yield r
    r.close()


def rays():
    """The ray set R: origins inside and outside the bounding sphere, directions towards the
    model or random, half of them not unit length."""
    rng = np.random.default_rng(7)
    n = 1000
    o = rng.uniform(-1.6, 1.6, (n, 3))
    tgt = rng.uniform(-0.5, 0.5, (n, 3))
    d = tgt - o
    d[::3] = rng.normal(size=d[::3].shape)
    d[1::2] *= 0.5
    return o.astype(np.float32), d.astype(np.float32)


@functools.lru_cache(maxsize=None)
def plane_net(four):
    """plane_1's oracle network; four: with a 4th input row appended to the first kernel."""
    dims, K, B = nr.read_keras_h5(nr.geometry_path("plane_1"))
    if four:
        K = [np.concatenate([K[0], np.random.default_rng(4).normal(0, 0.01, (1, 32)).astype(np.float32)], 0)] + K[1:]
        dims = [4] + list(dims[1:])
    return dims, K, B, oracle.OracleNet(K, B)


@functools.lru_cache(maxsize=None)
def reference(scene, steps, frame=FRAME, four=False):
    """query_ref.trace on R, computed once per case and shared (never modified)."""
    o, d = rays()
    out, st = query_ref.trace(plane_net(four)[3], o, d, steps, scene=nr.NR_SCENE[scene], frame=frame)
    for a in out.values():
        a.setflags(write=False)
    return out, st


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


# (scene, max_steps, the reference's MISS / ESCAPED / HIT / LIMIT counts on R)
R_CASES = [("tanh", 300, [171, 620, 209, 0]), ("v1", 300, [171, 612, 217, 0]),
           ("tanh", 12, [171, 499, 74, 256]), ("v1", 12, [171, 481, 72, 276])]


@pytest.mark.parametrize("scene,steps,expect", R_CASES)
def test_rays_bitexact(rend, scene, steps, expect):
    ref, rst = reference(scene, steps)
    # the reference itself covers every status it is expected to (not a vacuous comparison)
    assert counts(ref["status"]) == expect
    assert all(c >= 50 for c in expect if c), expect
    assert not np.isnan(ref["normal"]).any()
    o, d = rays()
    out, st = rend.set_scene(scene).trace_rays(o, d, steps, with_stats=True)
    assert_same(out, ref)
    for k in STAT_KEYS:
        assert st[k] == rst[k], (k, st, rst)


@pytest.mark.parametrize("steps,hits", [(2, 1), (1, 0)])
def test_an_iteration_left_to_shade(rend, steps, hits):
    """A ray that converges in its last permitted iteration is LIMIT, not HIT: with 2 iterations
    only a ray that converged at iteration 0 is a hit, with 1 none is."""
    ref, rst = reference("tanh", steps)
    assert counts(ref["status"])[HIT] == hits
    if hits:
        assert ref["steps"][ref["status"] == HIT].tolist() == [1]
    assert counts(ref["status"])[LIMIT] >= 50
    o, d = rays()
    out, st = rend.set_scene("tanh").trace_rays(o, d, steps, with_stats=True)
    assert_same(out, ref)
    for k in STAT_KEYS:
        assert st[k] == rst[k], (k, st, rst)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 257, 4099])
def test_ragged_sizes(rend, n):
    """A lone lane, tile and wave edges, several workgroups and refills: prefixes of R, and R
    tiled to 4,099 rays, each equal to the reference's rows."""
    ref, _ = reference("v1", 300)
    o, d = rays()
    rows = np.arange(n) % len(o)
    out = rend.set_scene("v1").trace_rays(o[rows], d[rows], 300)
    assert_same(out, ref, rows)


def test_order_determinism_and_precision(rend):
    ref, _ = reference("v1", 300)
    o, d = rays()
    rend.set_scene("v1")
    perm = np.random.default_rng(11).permutation(len(o))
    assert_same(rend.trace_rays(o[perm], d[perm], 300), ref, perm)
    a, b = rend.trace_rays(o, d, 300), rend.trace_rays(o, d, 300)
    assert_same(a, b)
    try:
        rend.set_precision("bf16")  # ignored: the queries always run the fp32 MLP
        assert_same(rend.trace_rays(o, d, 300), ref)
    finally:
        rend.set_precision("fp32")


def test_without_normals(rend):
    ref, rst = reference("v1", 300)
    o, d = rays()
    out, st = rend.set_scene("v1").trace_rays(o, d, 300, normals=False, with_stats=True)
    assert "normal" not in out
    assert_same(out, ref, keys=KEYS[:4])
    assert st["shade_evals"] == 0
    for k in ("ray_steps", "rays_hit", "rays_shaded", "iterations"):
        assert st[k] == rst[k], (k, st, rst)


# two of test_gpu_parity.py test_render_bitexact's cases: W, H, scene, rx, ry, zoom, steps
@pytest.mark.parametrize("W,H,scene,rx,ry,zoom,steps", [(97, 61, "v1", 25.0, 40.0, 2.0, 64),
                                                         (64, 64, "v1", 10.0, 300.0, 3.0, 6000)])
def test_gbuffer_against_the_frame(rend, W, H, scene, rx, ry, zoom, steps):
    iv, nm = nr.camera(rx, ry, zoom)
    try:
        rend.set_view(iv, nm, 0).set_scene(scene)
        img, ist = rend.render(W, H, steps)
        g, gst = rend.render_gbuffer(W, H, steps, with_stats=True)
        O, D = query_ref.pixel_rays(W, H, iv)
        q = rend.trace_rays(O, D, steps)
    finally:
        rend.set_view(*nr.camera(0.0, 0.0, 2.0), FRAME)
    assert (img != 0).sum() >= 50
    assert g["status"].shape == (H, W) and g["normal"].shape == (H, W, 3)
    assert np.array_equal(g["status"] == HIT, img != 0)
    assert np.array_equal(query_ref.facing(g["normal"], D, g["status"]).reshape(H, W), img)
    assert_same({k: g[k].reshape(q[k].shape) for k in KEYS}, q)
    for k in ("ray_steps", "shade_evals", "rays_hit", "rays_shaded"):
        assert gst[k] == ist[k], (k, gst, ist)


def test_four_input_network(nets):
    """(float)frame is the network's 4th input.  The scene is tanh, which does not read the
    frame, so the two frames differ only through that input."""
    dims, K, B, _ = plane_net(True)
    o, d = rays()
    refs = [reference("tanh", 300, frame, True)[0] for frame in (0, 5)]
    # the 4th input is live: the hit parameter differs between the frames on many rays
    assert int((bits(refs[0]["t"]) != bits(refs[1]["t"])).sum()) >= 50
    with nr.Renderer(0) as r:
        r.load_mlp(dims, K, B).set_static(nr.NR_COLOR_FACING, 4).set_scene("tanh")
        for frame, ref in zip((0, 5), refs):
            r.set_view(*nr.camera(0.0, 0.0, 2.0), frame)
            assert_same(r.trace_rays(o, d, 300), ref)


def test_device_path(rend):
    """torch tensors on cuda:0 through trace_rays_device on torch's current stream (the null
    stream here; the library's own synchronize() waits for the launch)."""
    ref, _ = reference("v1", 300)
    o, d = rays()
    n = len(o)
    dev = torch.device("cuda:0")
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    outs = {"status": torch.full((n,), -1, dtype=torch.int32, device=dev),
            "steps": torch.full((n,), -1, dtype=torch.int32, device=dev),
            "t": torch.full((n,), -1.0, dtype=torch.float32, device=dev),
            "position": torch.full((n, 3), -1.0, dtype=torch.float32, device=dev),
            "normal": torch.full((n, 3), -1.0, dtype=torch.float32, device=dev)}
    try:
        rend.set_scene("v1").set_stream(torch.cuda.current_stream(dev).cuda_stream)
        rend.trace_rays_device(to.data_ptr(), td.data_ptr(), n, 300, outs["status"].data_ptr(), outs["steps"].data_ptr(),
                               outs["t"].data_ptr(), outs["position"].data_ptr(), outs["normal"].data_ptr())
        rend.synchronize()
        torch.cuda.current_stream(dev).synchronize()
    finally:
        rend.set_stream(None, own=True)
    assert_same({k: v.cpu().numpy() for k, v in outs.items()}, ref)


def test_errors(rend, nets):
    L = nr.lib()
    z = np.zeros((4, 3), np.float32)

    def call(r, n=4, steps=10):
        return L.nr_trace_rays(r._ctx, z.ctypes.data, z.ctypes.data, n, steps, None, None, None, None, None, 0, None)

    with nr.Renderer(0) as r:
        assert call(r) == -5  # NR_E_STATE: no network
        assert L.nr_render_gbuffer(r._ctx, 4, 4, 10, None, None, None, None, None, 0, None) == -5
        rng = np.random.default_rng(0)
        r.load_mlp([3, 16, 1], [rng.normal(size=(3, 16)).astype(np.float32), rng.normal(size=(16, 1)).astype(np.float32)],
                   [np.zeros(16, np.float32), np.zeros(1, np.float32)])
        assert call(r) == -4  # NR_E_FORMAT: not a network of the fused kernels
        assert L.nr_render_gbuffer(r._ctx, 4, 4, 10, None, None, None, None, None, 0, None) == -4
    assert call(rend, n=-1) == -1
    assert call(rend, steps=0) == -1
    assert L.nr_render_gbuffer(rend._ctx, 0, 4, 10, None, None, None, None, None, 0, None) == -1
    assert L.nr_trace_rays(rend._ctx, None, None, 4, 10, None, None, None, None, None, 0, None) == -1
    st = nr._lib.NRStats()
    assert L.nr_trace_rays(rend._ctx, None, None, 0, 10, None, None, None, None, None, 0, ctypes.byref(st)) == 0
    assert st.ray_steps == 0 and st.launches == 0
    out = rend.trace_rays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 10)
    assert out["status"].shape == (0,) and out["normal"].shape == (0, 3)
