"""nr_project_points on the GPU (nr_project.hip) against tests/project_ref.py, the numpy restatement
of its loop on grad_ref's exact chains (pinned by tests/test_project_cpu.py).  The contract is
bit-exactness: every comparison is on uint32 views, so NaN payloads and -0 count."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cudaneuralrender_amd as nr
from cudaneuralrender_amd import _lib
import grad_ref
import project_ref
from test_gpu_grad import far_points, plane_net, shallow_net

pytestmark = pytest.mark.gpu
KEYS = project_ref.KEYS
NP = 1063  # 16 full chunks of 64 and a tail of 39
NV = 333   # the variants' prefix: 5 chunks and a tail of 13
DEFAULTS = dict(iso=0.0, tol=1e-5, max_step=0.25, max_iters=32)
ATANH_004 = float(np.arctanh(np.float32(0.04)))  # NR_SCENE_ROUND's level
# where torch bundles a HIP runtime of its own beside libnr's, torch has to open the GPU first
if torch.cuda.is_available():
    torch.cuda.init()


@functools.lru_cache(maxsize=None)
def points(four=False):
    """P: uniform in [-1, 1]^3, seeded (test_project_cpu's sample); four: a 4th column in [-1, 1]."""
    X = np.random.default_rng(7).uniform(-1, 1, (NP, 3)).astype(np.float32)
    if four:
        X = np.concatenate([X, np.random.default_rng(8).uniform(-1, 1, (NP, 1)).astype(np.float32)], 1)
    X = np.ascontiguousarray(X)
    X.setflags(write=False)
    return X


def _frozen(out):
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(four=False):
    """project_ref.project on P with the defaults, computed once per network and shared (never modified)."""
    _, K, B = plane_net(four)
    return _frozen(project_ref.project(K, B, points(four), **DEFAULTS))


@functools.lru_cache(maxsize=None)
def variant(**kw):
    """The reference of the first NV points of P with some options changed."""
    _, K, B = plane_net(False)
    return _frozen(project_ref.project(K, B, points()[:NV], **{**DEFAULTS, **kw}))


def flat_net():
    """shallow_net(1) with the first kernel's rows y and z zero, its row x positive and the first bias
    0: at x < 0 every first-layer unit is dead and the gradient is +0.  The later kernels and the
    second bias are made non-negative, so the value is convex and increasing in x > 0, and the last
    bias puts its root at x = 0.5: Newton steps from x > 0 stay at x > 0."""
    dims, K, B = shallow_net(1)
    K = [np.abs(k) for k in K]
    B = [b.copy() for b in B]
    K[0][0] += np.float32(0.05)
    K[0][1:] = 0
    B[0][:] = 0
    B[1] = np.abs(B[1])
    B[2][:] = 0
    B[2][0] = -grad_ref.forward_masks(K, B, np.array([[0.5, 0, 0]], np.float32))[0][0]
    return dims, K, B


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(out, ref, n=None, keys=KEYS):
    for k in keys:
        r = ref[k] if n is None else ref[k][:n]
        assert out[k].shape == r.shape and out[k].dtype == r.dtype, (k, out[k].shape, r.shape, out[k].dtype)
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


def device_call(r, X, **kw):
    dev = torch.device("cuda:0")
    n = X.shape[0]
    tx = torch.from_numpy(np.array(X, np.float32)).to(dev)  # (a writable copy of the shared points)
    f32, i32 = torch.float32, torch.int32
    outs = {"position": torch.full((n, 3), -1.0, dtype=f32, device=dev), "value": torch.full((n,), -1.0, dtype=f32, device=dev),
            "normal": torch.full((n, 3), -1.0, dtype=f32, device=dev), "distance": torch.full((n,), -1.0, dtype=f32, device=dev),
            "iters": torch.full((n,), -1, dtype=i32, device=dev), "status": torch.full((n,), -1, dtype=i32, device=dev)}
    try:
        r.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        r.project_points_device(tx.data_ptr(), n, **{**DEFAULTS, **kw}, **{k + "_ptr": v.data_ptr() for k, v in outs.items()})
        r.synchronize()
        torch.cuda.current_stream(dev).synchronize()
    finally:
        r.set_stream(None, own=True)
    return {k: v.cpu().numpy() for k, v in outs.items()}


def test_bit_exact_host_3_inputs(rend):
    assert_same(rend.project_points(points()), reference())


def test_bit_exact_host_4_inputs(rend4):
    assert_same(rend4.project_points(points(True)), reference(True))


def test_bit_exact_device_3_inputs(rend):
    assert_same(device_call(rend, points()), reference())


def test_bit_exact_device_4_inputs(rend4):
    assert_same(device_call(rend4, points(True)), reference(True))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65])
def test_sizes(rend, n):
    """Prefixes of P across the tile and chunk edges."""
    assert_same(rend.project_points(points()[:n]), reference(), n)


def test_zero_points(rend):
    """n = 0: NR_OK, no launch, outputs untouched."""
    L = nr.lib()
    st = _lib.NRStats()
    st.launches = 7
    v = np.full(4, 3.0, np.float32)
    opts = _lib.NRProjectOpts(0.0, 1e-5, 0.25, 32)
    assert L.nr_project_points(rend._ctx, None, 0, opts, None, v.ctypes.data, None, None, None, None, 0, ctypes.byref(st)) == 0
    assert st.launches == 0 and st.ray_steps == 0
    assert (v == 3.0).all()
    out = rend.project_points(np.zeros((0, 3), np.float32))
    assert out["position"].shape == (0, 3) and out["status"].shape == (0,)


def test_oversubscribed_grid_split_calls_and_order(rend):
    """P repeated 256 times (272,128 points: more than 256 CUs x 2 workgroups x 4 waves x 64 slots hold,
    so every wave refills and drains) is the reference tiled; the same points in three unequal calls
    and in reversed order give the same bits per point."""
    X = np.tile(points(), (256, 1))
    ref = {k: np.tile(reference()[k], (256,) + (1,) * (reference()[k].ndim - 1)) for k in KEYS}
    out = rend.project_points(X)
    assert_same(out, ref)
    cuts = [0, 1000, 1000 + 77777, len(X)]
    parts = [rend.project_points(X[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    rev = rend.project_points(X[::-1])
    for k in KEYS:
        assert np.array_equal(bits(np.concatenate([p[k] for p in parts])), bits(out[k])), k
        assert np.array_equal(bits(rev[k][::-1]), bits(out[k])), k


def test_occupancy(rend):
    """One workgroup per CU (nr_set_occupancy) gives the default grid's bits."""
    X = np.tile(points(), (64, 1))
    a = rend.project_points(X)
    try:
        rend.set_occupancy(1)
        b = rend.project_points(X)
    finally:
        rend.set_occupancy(0)
    assert_same(b, a)
    assert_same({k: v[:NP] for k, v in a.items()}, reference())


def test_value_and_normal_are_the_other_entry_points(rend):
    out = rend.project_points(points())
    assert np.array_equal(bits(out["value"]), bits(rend.mlp_forward(out["position"])[:, 0]))
    g = rend.mlp_gradient(out["position"], value=True, grad=False, normal=True)
    assert np.array_equal(bits(out["normal"]), bits(g["normal"]))
    assert np.array_equal(bits(out["value"]), bits(g["value"]))


def test_max_iters_zero_is_mlp_gradient(rend):
    out = rend.project_points(points(), max_iters=0)
    g = rend.mlp_gradient(points(), value=True, grad=False, normal=True)
    assert np.array_equal(bits(out["value"]), bits(g["value"]))
    assert np.array_equal(bits(out["normal"]), bits(g["normal"]))
    assert np.array_equal(bits(out["position"]), bits(points()))
    assert (out["iters"] == 0).all()
    assert ((out["status"] == nr.NR_PROJ_CONVERGED) == (np.abs(g["value"]) <= np.float32(1e-5))).all()
    assert ((out["status"] == nr.NR_PROJ_LIMIT) == (np.abs(g["value"]) > np.float32(1e-5))).all()
    assert_same(rend.project_points(points()[:NV], max_iters=0), variant(max_iters=0))


def test_limit_path(rend):
    ref = variant(max_iters=3)
    lim = ref["status"] == project_ref.LIMIT
    assert lim.mean() > 0.5
    out = rend.project_points(points()[:NV], max_iters=3)
    assert_same(out, ref)
    assert (out["iters"][lim] == 3).all()


@pytest.mark.parametrize("max_step", [0.0, 0.01])
def test_step_clamp(rend, max_step):
    """Unlimited steps, and a clamp that is on at nearly every step."""
    assert_same(rend.project_points(points()[:NV], max_step=max_step), variant(max_step=max_step))


@pytest.mark.parametrize("iso", [0.05, ATANH_004])
def test_level_sets(rend, iso):
    assert_same(rend.project_points(points()[:NV], iso=iso), variant(iso=iso))


def test_flat_path():
    """Points at x < 0 of flat_net are FLAT at once, beside points at x > 0 that converge or reach the limit."""
    dims, K, B = flat_net()
    X = points()[:NV]
    ref = project_ref.project(K, B, X, **DEFAULTS)
    left = X[:, 0] < 0
    assert 0.3 < left.mean() < 0.7
    assert (ref["status"][left] == project_ref.FLAT).all() and (ref["status"][~left] != project_ref.FLAT).all()
    with nr.Renderer(0) as r:
        r.load_mlp(dims, K, B)
        out = r.project_points(X)
    assert_same(out, ref)
    assert (out["iters"][left] == 0).all()
    assert np.array_equal(bits(out["position"][left]), bits(X[left]))


def test_unclamped_form(rend):
    """A chunk with points beyond F32_INPUT_BOUND (add + max ReLU) beside in-bound points."""
    _, K, B = plane_net(False)
    X = far_points()
    assert_same(rend.project_points(X), project_ref.project(K, B, X, **DEFAULTS))


@pytest.mark.parametrize("keys", [(k,) for k in KEYS] + [("position", "status"), ("value", "iters"), ("normal", "distance")])
def test_output_subsets(rend, keys):
    out = rend.project_points(points(), outputs=keys)
    assert tuple(out) == tuple(k for k in KEYS if k in keys)
    assert_same(out, reference(), keys=keys)


def test_stats(rend):
    out, st = rend.project_points(points(), with_stats=True)
    assert_same(out, reference())
    want = project_ref.stats(reference())
    assert st["ray_steps"] == want["ray_steps"] == int((out["iters"] + 1).sum())
    assert st["rays_shaded"] == want["rays_shaded"] == int((out["status"] == nr.NR_PROJ_CONVERGED).sum())
    assert st["iterations"] == want["iterations"] == int(out["iters"].max()) + 1
    assert st["launches"] >= 1 and st["ms_total"] > 0
    for k in ("shade_evals", "rays_hit", "endgame_evals", "endgame_switches"):
        assert st[k] == 0, (k, st)


def test_settings_are_ignored_and_kept(rend):
    """nr_set_precision is ignored, and still in force for the next nr_mlp_forward."""
    f32 = rend.mlp_forward(points())
    try:
        rend.set_precision("bf16")
        before = rend.mlp_forward(points())
        assert_same(rend.project_points(points()), reference())
        after = rend.mlp_forward(points())
        assert np.array_equal(bits(before), bits(after)) and not np.array_equal(bits(before), bits(f32))
    finally:
        rend.set_precision("fp32")


def test_deterministic(rend):
    a, b = rend.project_points(points()), rend.project_points(points())
    for k in KEYS:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


def test_errors(rend):
    L = nr.lib()
    z = np.zeros((4, 3), np.float32)
    o = np.zeros((4, 3), np.float32)
    good = dict(iso=0.0, tol=1e-5, max_step=0.25, max_iters=32)

    def call(r, n=4, x=z.ctypes.data, p=o.ctypes.data, null_opts=False, **kw):
        f = {**good, **kw}
        opts = None if null_opts else _lib.NRProjectOpts(f["iso"], f["tol"], f["max_step"], f["max_iters"])
        return L.nr_project_points(r._ctx if r else None, x, n, opts, p, None, None, None, None, None, 0, None)

    assert call(None) == -1
    assert call(rend, null_opts=True) == -1
    assert call(rend, n=-1) == -1
    assert call(rend, n=(1 << 30) + 1) == -1
    assert call(rend, x=None) == -1
    assert call(rend, p=None) == -1  # every output NULL
    assert call(rend, tol=-1e-6) == -1
    assert call(rend, max_step=-0.1) == -1
    for field in ("iso", "tol", "max_step"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(rend, **{field: bad}) == -1, (field, bad)
    assert call(rend, max_iters=-1) == -1
    assert call(rend, max_iters=4097) == -1
    assert call(rend, max_iters=4096, tol=1.0) == 0
    with nr.Renderer(0) as r:
        assert call(r) == -5  # NR_E_STATE: no network
        rng = np.random.default_rng(0)
        r.load_mlp([3, 16, 1], [rng.normal(size=(3, 16)).astype(np.float32), rng.normal(size=(16, 1)).astype(np.float32)],
                   [np.zeros(16, np.float32), np.zeros(1, np.float32)])
        assert call(r) == -4  # NR_E_FORMAT: not a network of the fused kernels
    assert call(rend) == 0


def test_more_hidden_layers_than_the_masks_hold():
    """8 hidden 32 x 32 layers: NR_E_FORMAT, as nr_mlp_gradient."""
    dims, K, B = shallow_net(8)
    with nr.Renderer(0) as r:
        r.load_mlp(dims, K, B)
        with pytest.raises(nr.NRError) as e:
            r.project_points(points()[:64])
        assert e.value.code == -4
