"""CPU side of nr_mlp_gradient: tests/grad_ref.py (the numpy restatement the GPU tests compare
against) has the oracle's forward bits and a gradient that agrees with a finite difference of the
same weights in f64, and libnr.so exports the entry point."""
import functools

import numpy as np

import cudaneuralrender_amd as nr
from cudaneuralrender_amd import _lib
import grad_ref
import oracle

N = 4096


def plane_net(four):
    """plane_1's network; four: with a 4th input row appended to the first kernel (as
    test_gpu_query.plane_net)."""
    dims, K, B = nr.read_keras_h5(nr.geometry_path("plane_1"))
    if four:
        K = [np.concatenate([K[0], np.random.default_rng(4).normal(0, 0.01, (1, 32)).astype(np.float32)], 0)] + K[1:]
    return K, B


@functools.lru_cache(maxsize=None)
def points(cols):
    X = np.random.default_rng(11).uniform(-1, 1, (N, cols)).astype(np.float32)
    X.setflags(write=False)
    return X


def test_forward_bits_are_the_oracles_3_inputs():
    K, B = plane_net(False)
    v, masks = grad_ref.forward_masks(K, B, points(3))
    ref = oracle.OracleNet(K, B).forward(points(3))[:, 0]
    assert np.array_equal(v.view(np.uint32), ref.view(np.uint32))
    assert len(masks) == len(K) - 1 and all(m.shape == (N, 32) for m in masks)


def test_forward_bits_are_the_oracles_4_inputs():
    K, B = plane_net(True)
    v, _ = grad_ref.forward_masks(K, B, points(4))
    ref = oracle.OracleNet(K, B).forward(points(4))[:, 0]
    assert np.array_equal(v.view(np.uint32), ref.view(np.uint32))


def test_fmaf_is_correctly_rounded():
    """Cases a double-rounded a * b + c gets wrong: the f64 sum is a tie of f32 only through rounding."""
    F = np.float32
    a = F(1 + 2.0 ** -12)
    c = F(2.0 ** -60)  # below the f64 sum's last bit: only the sticky bit of round-to-odd keeps it
    # a * a = 1 + 2^-11 + 2^-24: a tie between 1 + 2^-11 and its successor; c breaks it upwards
    assert grad_ref.fmaf(a, a, c) == F(1 + 2.0 ** -11 + 2.0 ** -23)
    assert grad_ref.fmaf(a, a, -c) == F(1 + 2.0 ** -11)
    assert grad_ref.fmaf(a, a, F(0)) == F(1 + 2.0 ** -11)  # the tie itself: to even
    assert grad_ref.fmaf(F(3), F(5), F(-15)) == 0


def f64_forward(K, B, X):
    a = np.asarray(X, np.float64)
    masks = []
    for l, (W, b) in enumerate(zip(K, B)):
        z = a @ np.asarray(W, np.float64) + np.asarray(b, np.float64)
        if l == len(K) - 1:
            return z[:, 0], masks
        masks.append(z > 0)
        a = np.maximum(z, 0)


def test_gradient_agrees_with_a_central_difference():
    """Against (f(x + h e_c) - f(x - h e_c)) / 2h in f64, h = 1e-6: at least 99 % of the points within
    1e-5 absolute in every component; at each of the others the three f64 evaluations and the f32
    forward do not share one ReLU pattern (the point straddles a kink, where the difference
    quotient mixes two linear pieces).  Measured: 99.93 % within 1e-6."""
    K, B = plane_net(False)
    X = points(3)
    _, g, _ = grad_ref.gradient(K, B, X)
    _, m32 = grad_ref.forward_masks(K, B, X)
    h = 1e-6
    _, m0 = f64_forward(K, B, X)
    bad = np.zeros(N, bool)
    kink = np.zeros(N, bool)
    for c in range(3):
        d = np.zeros(3)
        d[c] = h
        fp, mp = f64_forward(K, B, X.astype(np.float64) + d)
        fm, mm = f64_forward(K, B, X.astype(np.float64) - d)
        fd = (fp - fm) / (2 * h)
        bad |= np.abs(fd - g[:, c]) > 1e-5
        for a, b, z, f in zip(mp, mm, m0, m32):
            kink |= (a != b).any(1) | (a != z).any(1) | (z != f).any(1)
    print(f"within 1e-5: {100 * (1 - bad.mean()):.3f} %, not within: {int(bad.sum())}, of them at a kink: "
          f"{int((bad & kink).sum())}")
    assert bad.mean() <= 0.01
    assert not (bad & ~kink).any()


def test_library_exports_the_gradient():
    """nr_mlp_gradient exists in libnr.so, the binding declares it, and it rejects a NULL context
    without touching a device."""
    L = nr.lib()
    assert "nr_mlp_gradient" in _lib.EXPORTS
    assert hasattr(L, "nr_mlp_gradient")
    assert L.nr_mlp_gradient.argtypes is not None and len(L.nr_mlp_gradient.argtypes) == 8
    z = np.zeros(3, np.float32)
    assert L.nr_mlp_gradient(None, z.ctypes.data, 1, z.ctypes.data, None, None, _lib.NR_HOST, None) == -1
    assert b"NULL" in L.nr_last_error(None)
    assert L.nr_abi_version() == 3
    assert hasattr(nr.Renderer, "mlp_gradient") and hasattr(nr.Renderer, "mlp_gradient_device")
