"""The analytic gradient on the GPU (nr_mlp_gradient, nr_grad.hip) against tests/grad_ref.py, the
numpy restatement of its chains on an exact fmaf (pinned by tests/test_grad_cpu.py).  The contract
is bit-exactness: every comparison is on uint32 views, so NaN payloads and -0 count."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cudaneuralrender_amd as nr
import grad_ref

pytestmark = pytest.mark.gpu
KEYS = ("value", "grad", "normal")
NP = 4135  # 64 full chunks and a tail of 39
# where torch bundles a HIP runtime of its own beside libnr's, torch has to open the GPU first
if torch.cuda.is_available():
    torch.cuda.init()


@functools.lru_cache(maxsize=None)
def plane_net(four):
    """plane_1's network; four: with a 4th input row appended to the first kernel (as
    test_gpu_query.plane_net)."""
    dims, K, B = nr.read_keras_h5(nr.geometry_path("plane_1"))
    if four:
        K = [np.concatenate([K[0], np.random.default_rng(4).normal(0, 0.01, (1, 32)).astype(np.float32)], 0)] + K[1:]
        dims = [4] + list(dims[1:])
    return dims, K, B


def shallow_net(nh=1):
    """A small random [3, 32 x (nh + 1), 1] network."""
    rng = np.random.default_rng(21)
    dims = [3] + [32] * (nh + 1) + [1]
    K = [rng.normal(0, 0.4, (dims[i], dims[i + 1])).astype(np.float32) for i in range(len(dims) - 1)]
    B = [rng.normal(0, 0.1, (dims[i + 1],)).astype(np.float32) for i in range(len(dims) - 1)]
    return dims, K, B


@functools.lru_cache(maxsize=None)
def points(four=False):
    """P: uniform in [-1, 1]^3 (a 4th column in [-1, 1] for a 4-input network), seeded."""
    X = np.random.default_rng(5).uniform(-1, 1, (NP, 4)).astype(np.float32)
    X = np.ascontiguousarray(X[:, : 4 if four else 3])
    X.setflags(write=False)
    return X


def _frozen(ref):
    out = dict(zip(KEYS, ref))
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(four=False):
    """grad_ref.gradient on P, computed once per network and shared (never modified)."""
    _, K, B = plane_net(four)
    return _frozen(grad_ref.gradient(K, B, points(four)))


def far_points():
    """The first 256 points of P with a coordinate of 1500.0 (beyond F32_INPUT_BOUND = 1024) in every
    third point of the second chunk: that wave takes the add + max form, its other points with it."""
    X = points().copy()[:256]
    X[64:128:3, 0] = 1500.0
    X[65:128:3, 2] = -1500.0
    return X


@functools.lru_cache(maxsize=None)
def far_reference():
    _, K, B = plane_net(False)
    return _frozen(grad_ref.gradient(K, B, far_points()))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(out, ref, n=None, keys=KEYS):
    for k in keys:
        r = ref[k] if n is None else ref[k][:n]
        assert out[k].shape == r.shape, (k, out[k].shape, r.shape)
        same = bits(out[k]) == bits(r)
        assert same.all(), f"{k}: {(~same).sum()} of {same.size} words differ, first at {np.argwhere(~same)[0]}"


@pytest.fixture(scope="module")
def rend():
    dims, K, B = plane_net(False)
    r = nr.Renderer(0)
    r.load_mlp(dims, K, B).set_precision("fp32")
    yield r
    r.close()


@pytest.fixture(scope="module")
def rend4():
    dims, K, B = plane_net(True)
    r = nr.Renderer(0)
    r.load_mlp(dims, K, B).set_precision("fp32")
    yield r
    r.close()


def all3(r, X, **kw):
    return r.mlp_gradient(X, value=True, grad=True, normal=True, **kw)


def device_call(r, X):
    dev = torch.device("cuda:0")
    n, cols = X.shape
    tx = torch.from_numpy(np.array(X, np.float32)).to(dev)  # (a writable copy of the shared points)
    outs = {"value": torch.full((n,), -1.0, dtype=torch.float32, device=dev),
            "grad": torch.full((n, cols), -1.0, dtype=torch.float32, device=dev),
            "normal": torch.full((n, 3), -1.0, dtype=torch.float32, device=dev)}
    try:
        r.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        r.mlp_gradient_device(tx.data_ptr(), n, outs["value"].data_ptr(), outs["grad"].data_ptr(),
                              outs["normal"].data_ptr())
        r.synchronize()
        torch.cuda.current_stream(dev).synchronize()
    finally:
        r.set_stream(None, own=True)
    return {k: v.cpu().numpy() for k, v in outs.items()}


def test_bit_exact_host_3_inputs(rend):
    assert_same(all3(rend, points()), reference())


def test_bit_exact_host_4_inputs(rend4):
    assert_same(all3(rend4, points(True)), reference(True))


def test_bit_exact_device_3_inputs(rend):
    assert_same(device_call(rend, points()), reference())


def test_bit_exact_device_4_inputs(rend4):
    assert_same(device_call(rend4, points(True)), reference(True))


def test_value_is_mlp_forward(rend):
    v = rend.mlp_gradient(points(), grad=False)["value"]
    assert np.array_equal(bits(v), bits(rend.mlp_forward(points())[:, 0]))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65])
def test_sizes(rend, n):
    """Prefixes of P across the tile and chunk edges."""
    assert_same(all3(rend, points()[:n]), reference(), n)


def test_zero_points(rend):
    """n = 0: NR_OK, no launch, outputs untouched."""
    L = nr.lib()
    st = nr._lib.NRStats()
    st.launches = 7
    v = np.full(4, 3.0, np.float32)
    assert L.nr_mlp_gradient(rend._ctx, None, 0, v.ctypes.data, None, None, 0, ctypes.byref(st)) == 0
    assert st.launches == 0 and st.ray_steps == 0
    assert (v == 3.0).all()
    out = all3(rend, np.zeros((0, 3), np.float32))
    assert out["value"].shape == (0,) and out["grad"].shape == (0, 3) and out["normal"].shape == (0, 3)


def test_many_chunks_per_wave_and_split_calls(rend):
    """P repeated 64 times (264,640 points, 4,135 chunks: more than the grid's wave slots) is the
    reference tiled, and so are the same points issued in three unequal calls."""
    X = np.tile(points(), (64, 1))
    ref = {k: np.tile(reference()[k], (64,) + (1,) * (reference()[k].ndim - 1)) for k in KEYS}
    out = all3(rend, X)
    assert_same(out, ref)
    cuts = [0, 1000, 1000 + 77777, len(X)]
    parts = [all3(rend, X[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    for k in KEYS:
        assert np.array_equal(bits(np.concatenate([p[k] for p in parts])), bits(out[k])), k


def test_shallow_network():
    """One hidden 32 x 32 layer: both ReLU layers' masks in the first word, the last one transposed."""
    dims, K, B = shallow_net(1)
    X = points()[:333]
    ref = _frozen(grad_ref.gradient(K, B, X))
    with nr.Renderer(0) as r:
        r.load_mlp(dims, K, B)
        assert_same(all3(r, X), ref)


def test_more_hidden_layers_than_the_masks_hold():
    """8 hidden 32 x 32 layers (9 ReLU layers): the forward takes it, the gradient is NR_E_FORMAT."""
    dims, K, B = shallow_net(8)
    X = points()[:64]
    with nr.Renderer(0) as r:
        r.load_mlp(dims, K, B)
        assert r.mlp_forward(X).shape == (64, 1)
        with pytest.raises(nr.NRError) as e:
            all3(r, X)
        assert e.value.code == -4


def test_unclamped_form(rend):
    """A wave with inputs beyond F32_INPUT_BOUND (add + max ReLU) and its in-bound neighbours."""
    assert_same(all3(rend, far_points()), far_reference())


@pytest.mark.parametrize("keys", [("value",), ("grad",), ("normal",), ("value", "grad"), ("value", "normal"),
                                  ("grad", "normal")])
def test_output_subsets(rend, keys):
    out = rend.mlp_gradient(points(), **{k: k in keys for k in KEYS})
    assert tuple(out) == keys
    assert_same(out, reference(), keys=keys)


def test_stats(rend):
    _, st = all3(rend, points(), with_stats=True)
    assert st["ray_steps"] == NP and st["launches"] >= 1 and st["ms_total"] > 0
    for k in ("shade_evals", "rays_hit", "rays_shaded", "iterations", "endgame_evals", "endgame_switches"):
        assert st[k] == 0, (k, st)


def test_precision_is_ignored(rend):
    try:
        rend.set_precision("bf16")
        assert_same(all3(rend, points()), reference())
    finally:
        rend.set_precision("fp32")


def test_errors(rend):
    L = nr.lib()
    z = np.zeros((4, 3), np.float32)
    o = np.zeros((4, 3), np.float32)

    def call(r, n=4, x=z.ctypes.data, v=o.ctypes.data):
        return L.nr_mlp_gradient(r._ctx if r else None, x, n, v, None, None, 0, None)

    assert call(None) == -1
    assert call(rend, n=-1) == -1
    assert call(rend, n=(1 << 30) + 1) == -1
    assert call(rend, x=None) == -1
    assert call(rend, v=None) == -1  # every output NULL
    with nr.Renderer(0) as r:
        assert call(r) == -5  # NR_E_STATE: no network
        rng = np.random.default_rng(0)
        r.load_mlp([3, 16, 1], [rng.normal(size=(3, 16)).astype(np.float32), rng.normal(size=(16, 1)).astype(np.float32)],
                   [np.zeros(16, np.float32), np.zeros(1, np.float32)])
        assert call(r) == -4  # NR_E_FORMAT: not a network of the fused kernels
    assert call(rend) == 0


def test_deterministic(rend):
    a, b = all3(rend, points()), all3(rend, points())
    for k in KEYS:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def test_normal_agrees_with_the_gbuffer(rend):
    """On the HIT points of a 64 x 64 G-buffer of plane_1 (NR_SCENE_TANH), the analytic normal and the
    G-buffer's tetrahedral finite-difference normal (four fp32 evaluations at epsilon 1e-5) are two
    estimators of one direction: the median angle between them is below 1 degree (0.23 degrees
    between the two on 4,096 volume points on the CPU).  On these 132 hit points the median
    measured 0.0406 degrees (p95 0.16, max 4.06; DESIGN.md section 5, Analytic gradient) -- near the
    surface the values are near 0, where fp32 is finer and the finite difference cancels less --
    so the bound is 4 x that record."""
    rend.set_scene("tanh").set_static(nr.NR_COLOR_FACING, 3).set_view(*nr.camera(0.0, 0.0, 2.0), 0)
    try:
        gb = rend.render_gbuffer(64, 64, 6000)
    finally:
        rend.set_scene("v1")
    hit = gb["status"].reshape(-1) == nr.NR_RAY_HIT
    assert hit.sum() > 100
    pos = gb["position"].reshape(-1, 3)[hit]
    fd = gb["normal"].reshape(-1, 3)[hit].astype(np.float64)
    an = rend.mlp_gradient(pos, value=False, grad=False, normal=True)["normal"].astype(np.float64)
    cos = np.clip((fd * an).sum(1) / (np.linalg.norm(fd, axis=1) * np.linalg.norm(an, axis=1)), -1, 1)
    ang = np.degrees(np.arccos(cos))
    print(f"hits {int(hit.sum())}: median {np.median(ang):.4f} deg, p95 {np.percentile(ang, 95):.4f}, max {ang.max():.4f}")
    assert np.median(ang) < 1.0
    assert np.median(ang) < 4 * 0.0406
