"""Reference for nr_mlp_gradient: a helper, not a test.

The numpy restatement of the semantics in include/neural_render.h: the fp32 forward pass as the
oracle's dense layer (an ascending fmaf chain from +0, then + bias), the ReLU masks z > 0, and the
backward pass as fmaf chains over the Keras kernels, on an exact f32 fmaf.  tests/test_grad_cpu.py
pins the forward against OracleNet.forward bit for bit, so the oracle stays the yardstick.

fmaf: the product of two f32 is exact in f64 (48 bits); the sum p + c is rounded to odd in f64
(TwoSum gives the error; an inexact even result moves to its odd neighbour on the error's side),
and 53 >= 2 * 24 + 2 bits make the final rounding to f32 the correctly rounded fma.
"""
import numpy as np

from query_ref import normalize3

F = np.float32


def fmaf(a, b, c):
    """Correctly rounded f32 a * b + c, elementwise (finite operands)."""
    a, b, c = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64)
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)  # TwoSum: p + c = s + e exactly
    fix = (e != 0) & ((np.ascontiguousarray(s).view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def _chain(W, A):
    """acc[n, u] = chain over k ascending of fmaf(W[k][u], A[n][k], acc) from +0 (W: in x out)."""
    acc = np.zeros((A.shape[0], W.shape[1]), F)
    for k in range(W.shape[0]):
        acc = fmaf(W[k][None, :], A[:, k][:, None], acc)
    return acc


def forward_masks(K, B, X):
    """(value [n], masks): masks[l] [n, width] = z_l > 0 of ReLU layer l (every layer but the last)."""
    a = np.ascontiguousarray(X, F)
    masks = []
    for l, (W, b) in enumerate(zip(K, B)):
        z = (_chain(np.asarray(W, F), a) + np.asarray(b, F)[None, :]).astype(F)
        if l == len(K) - 1:
            return z[:, 0], masks
        masks.append(z > 0)
        a = np.maximum(z, F(0))


def gradient(K, B, X):
    """(value [n], grad [n, inputs], normal [n, 3]) of nr_mlp_gradient."""
    value, masks = forward_masks(K, B, X)
    nh = len(K) - 2
    g = np.where(masks[nh], np.asarray(K[-1], F)[:, 0][None, :], F(0)).astype(F)
    for l in range(nh, 0, -1):
        acc = _chain(np.asarray(K[l], F).T, g)  # acc[i] = chain over j of K_l[i][j] g[j]
        g = np.where(masks[l - 1], acc, F(0)).astype(F)
    grad = _chain(np.asarray(K[0], F).T, g)
    return value, grad, normalize3(grad[:, :3])
