"""Fitting on the GPU (nr_fit_*, nr_fit.hip) against tests/fit_ref.py, the numpy restatement of the
arithmetic in include/neural_render.h (pinned by tests/test_fit_cpu.py).  The contract is
bit-exactness: every comparison is on uint32 views.  partials = 4 unless a test says otherwise, so
that a partial's second tile and the ragged tail are reached with few points."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cudaneuralrender_amd as nr
import fit_ref

pytestmark = pytest.mark.gpu
F = np.float32
SIZES = (1, 15, 16, 17, 64, 65, 133)  # 133: 9 tiles on 4 partials (up to 3 tiles each) and a tail of 5
# where torch bundles a HIP runtime of its own beside libnr's, torch has to open the GPU first
if torch.cuda.is_available():
    torch.cuda.init()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@functools.lru_cache(maxsize=None)
def net(name):
    """"seeded": a random [3, 32, 32, 1]; "plane": plane_1's own weights (7 hidden layers)."""
    if name == "plane":
        dims, K, B = nr.read_keras_h5(nr.geometry_path("plane_1"))
        return list(dims), K, B
    rng = np.random.default_rng(31)
    dims = [3, 32, 32, 1]
    K = [rng.normal(0, 1.0 / np.sqrt(i), (i, o)).astype(F) for i, o in zip(dims[:-1], dims[1:])]
    B = [rng.normal(0, 0.1, o).astype(F) for o in dims[1:]]
    return dims, K, B


@functools.lru_cache(maxsize=None)
def data(n):
    """n seeded points in [-1, 1]^3 and targets: plane_1's values plus seeded noise of 0.01."""
    rng = np.random.default_rng(1000 + n)
    X = rng.uniform(-1, 1, (n, 3)).astype(F)
    _, K, B = net("plane")
    Y = (fit_ref.forward_acts(K, B, X)[0] + rng.normal(0, 0.01, n)).astype(F)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


@functools.lru_cache(maxsize=None)
def reference(name, clamp, n, partials=4):
    """fit_ref.gradient, computed once per case and shared (never modified)."""
    _, K, B = net(name)
    out = fit_ref.gradient(K, B, *data(n), clamp, partials)
    for a in (out["grad"], out["value"]):
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def rend():
    with nr.Renderer(0) as r:
        yield r


def assert_same(got_loss, got_flat, got_value, ref, what):
    assert bits(np.array([got_loss]))[0] == bits(np.array([ref["loss"]]))[0], f"{what}: loss {got_loss} vs {ref['loss']}"
    bad = bits(got_flat) != bits(ref["grad"])
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} gradient entries differ, first at {np.flatnonzero(bad)[:4]}"
    assert np.array_equal(bits(got_value), bits(ref["value"])), f"{what}: value"


@pytest.mark.parametrize("loc", ["host", "device"])
@pytest.mark.parametrize("clamp", [0.0, 0.05])
@pytest.mark.parametrize("name", ["seeded", "plane"])
def test_gradient_bits(rend, name, clamp, loc):
    dims, K, B = net(name)
    with nr.Fit(rend, dims, K, B, clamp=clamp, partials=4) as f:
        for n in SIZES:
            X, Y = data(n)
            ref = reference(name, clamp, n)
            if loc == "host":
                out = f.gradient(X, Y, value=True)
                assert_same(out["loss"], out["flat"], out["value"], ref, f"{name} n={n}")
                K2, B2 = out["grad"]
                assert np.array_equal(fit_ref.flatten(K2, B2), out["flat"]) and [k.shape for k in K2] == [k.shape for k in K]
            else:
                tx, ty = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(Y.copy()).cuda()
                tl = torch.full((1,), -1.0, device="cuda")
                tg = torch.full((f.num_params,), -1.0, device="cuda")
                tv = torch.full((n,), -1.0, device="cuda")
                torch.cuda.synchronize()
                f.gradient_device(tx.data_ptr(), ty.data_ptr(), n, tl.data_ptr(), tg.data_ptr(), tv.data_ptr())
                rend.synchronize()
                assert_same(tl.cpu().numpy()[0], tg.cpu().numpy(), tv.cpu().numpy(), ref, f"{name} n={n} (device)")


def test_default_partials(rend):
    """partials = 0 is 1024: n = 16 S + 5 gives the first partial a second tile, a ragged one."""
    S = fit_ref.DEFAULT_PARTIALS
    n = 16 * S + 5
    dims, K, B = net("seeded")
    ref = reference("seeded", 0.05, n, 0)
    with nr.Fit(rend, dims, K, B, clamp=0.05) as f:
        out = f.gradient(*data(n), value=True)
    assert_same(out["loss"], out["flat"], out["value"], ref, "default partials")


@pytest.mark.parametrize("name", ["seeded", "plane"])
def test_value_is_mlp_forward(rend, name):
    dims, K, B = net(name)
    X, Y = data(133)
    with nr.Fit(rend, dims, K, B, partials=4) as f, nr.Renderer(0) as r2:
        val = f.gradient(X, Y, value=True)["value"]
        want = r2.load_mlp(dims, K, B).mlp_forward(X)[:, 0]
    assert np.array_equal(bits(val), bits(want))


@pytest.mark.parametrize("partials", [8, 0])
def test_grid_independence(rend, partials):
    """grid = 1 (4 waves: several partials per wave, one after another), grid = 3 and the default
    grid give the same bits; so do two identical calls."""
    dims, K, B = net("plane")
    X, Y = data(1000)
    outs = []
    for grid in (1, 3, 0, 0):
        with nr.Fit(rend, dims, K, B, clamp=0.05, partials=partials, grid=grid) as f:
            o = f.gradient(X, Y, value=True)
            outs.append(np.concatenate([bits(np.array([o["loss"]])), bits(o["flat"]), bits(o["value"])]))
            if grid == 0:
                o = f.gradient(X, Y, value=True)
                outs.append(np.concatenate([bits(np.array([o["loss"]])), bits(o["flat"]), bits(o["value"])]))
    for o in outs[1:]:
        assert np.array_equal(o, outs[0])
    assert outs[0][1:1 + 96].any()


@pytest.mark.parametrize("name", ["seeded", "plane"])
def test_run_steps(rend, name):
    """3 steps of batch 64: losses and weights are the restatement's; the re-packed weights are the
    master weights (load_into, then mlp_forward, is the fit object's own value)."""
    dims, K, B = net(name)
    X, Y = data(192)
    ref = fit_ref.Fit(dims, K, B, lr=1e-3, clamp=0.05, partials=4)
    want = ref.run(X, Y, 64)
    with nr.Fit(rend, dims, K, B, lr=1e-3, clamp=0.05, partials=4) as f, nr.Renderer(0) as r2:
        got, st = f.run(X, Y, 64, with_stats=True)
        d2, K2, B2, step = f.weights()
        own = f.gradient(X, Y, value=True)["value"]
        f.load_into(r2)
        fwd = r2.mlp_forward(X)[:, 0]
    assert step == 3 and d2 == dims
    assert np.array_equal(bits(got), bits(want)), (got, want)
    assert np.array_equal(bits(fit_ref.flatten(K2, B2)), bits(ref.theta))
    assert not np.array_equal(bits(ref.theta), bits(fit_ref.flatten(K, B)))
    assert np.array_equal(bits(own), bits(fwd))
    assert st["ray_steps"] == 192 and 0 < st["launches"] <= 9 and st["ms_total"] > 0
    assert all(st[k] == 0 for k in st if k not in ("ray_steps", "launches", "ms_total"))


def test_run_device_pointers(rend):
    dims, K, B = net("seeded")
    X, Y = data(192)
    ref = fit_ref.Fit(dims, K, B, lr=1e-3, partials=4)
    want = ref.run(X, Y, 64)
    tx, ty = torch.from_numpy(X.copy()).cuda(), torch.from_numpy(Y.copy()).cuda()
    tl = torch.full((3,), -1.0, device="cuda")
    torch.cuda.synchronize()
    with nr.Fit(rend, dims, K, B, lr=1e-3, partials=4) as f:
        assert f.run_device(tx.data_ptr(), ty.data_ptr(), 192, 64, tl.data_ptr()) is None
        _, K2, B2, step = f.weights()
    assert step == 3
    assert np.array_equal(bits(tl.cpu().numpy()), bits(want))
    assert np.array_equal(bits(fit_ref.flatten(K2, B2)), bits(ref.theta))


def test_gradient_leaves_weights_alone(rend):
    dims, K, B = net("seeded")
    X, Y = data(192)
    ref = fit_ref.Fit(dims, K, B, lr=1e-3, partials=4)
    ref.run(X[:128], Y[:128], 64)
    with nr.Fit(rend, dims, K, B, lr=1e-3, partials=4) as f:
        f.run(X[:128], Y[:128], 64)
        before = f.weights()
        g = f.gradient(X, Y)
        after = f.weights()
        assert before[3] == after[3] == 2
        assert np.array_equal(bits(fit_ref.flatten(*before[1:3])), bits(fit_ref.flatten(*after[1:3])))
        assert np.array_equal(bits(g["flat"]), bits(ref.gradient(X, Y)["grad"]))
        # and the moments: the next step is still the restatement's third
        got = f.run(X[128:], Y[128:], 64)
        want = ref.run(X[128:], Y[128:], 64)
        assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(bits(fit_ref.flatten(*f.weights()[1:3])), bits(ref.theta))


def test_error_codes(rend):
    L = nr.lib()
    NR_E_INVALID, NR_E_FORMAT = -1, -4

    def code(fn):
        with pytest.raises(nr.NRError) as e:
            fn()
        return e.value.code

    def rnd(dims):
        rng = np.random.default_rng(2)
        return ([rng.normal(0, 0.3, (i, o)).astype(F) for i, o in zip(dims[:-1], dims[1:])],
                [np.zeros(o, F) for o in dims[1:]])

    for dims in ([3, 16, 1], [4, 32, 32, 1], [3] + [32] * 9 + [1], [3, 32, 32, 2]):
        assert code(lambda: nr.Fit(rend, dims, *rnd(dims))) == NR_E_FORMAT, dims
    dims, K, B = net("seeded")
    for kw in ({"lr": 0.0}, {"lr": float("nan")}, {"beta1": 1.0}, {"beta2": -0.1}, {"eps": 0.0}, {"clamp": -1.0},
               {"partials": 4097}, {"partials": -1}, {"grid": -1}):
        assert code(lambda: nr.Fit(rend, dims, K, B, **kw)) == NR_E_INVALID, kw
    X, Y = data(133)
    with nr.Fit(rend, dims, K, B, partials=4) as f:
        assert code(lambda: f.run(X, Y, 64)) == NR_E_INVALID          # n % batch != 0
        assert code(lambda: f.run(X[:128], Y[:128], 0)) == NR_E_INVALID
        assert f.weights()[3] == 0
        h = f._f
        x, y = X.ctypes.data, Y.ctypes.data
        assert L.nr_fit_gradient(h, None, y, 133, None, None, None, 0) == NR_E_INVALID
        assert L.nr_fit_gradient(h, x, None, 133, None, None, None, 0) == NR_E_INVALID
        assert L.nr_fit_gradient(h, x, y, 0, None, None, None, 0) == NR_E_INVALID
        assert L.nr_fit_gradient(h, x, y, (1 << 30) + 1, None, None, None, 0) == NR_E_INVALID
        assert L.nr_fit_gradient(None, x, y, 133, None, None, None, 0) == NR_E_INVALID
        assert L.nr_fit_run(h, None, y, 128, 64, None, 0, None) == NR_E_INVALID
        assert L.nr_fit_run(None, x, y, 128, 64, None, 0, None) == NR_E_INVALID
        assert L.nr_fit_weights(None, None, None) == NR_E_INVALID
        assert L.nr_fit_weights(h, None, None) == NR_E_INVALID
        assert L.nr_fit_num_params(h, None) == NR_E_INVALID
        out = ctypes.c_void_p()
        opts = nr.NRFitOpts(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0)
        assert L.nr_fit_create(rend._ctx, 3, None, None, None, ctypes.byref(opts), ctypes.byref(out)) == NR_E_INVALID
        assert L.nr_fit_create(None, 3, None, None, None, ctypes.byref(opts), ctypes.byref(out)) == NR_E_INVALID
        assert not out
    assert L.nr_fit_destroy(None) == 0
