"""Dense random fused-shape networks of every depth: a helper, not a test.

Every bundled geometry has 7 hidden 32x32 layers, the depth at which the fused kernels take their
unrolled and streamed instances.  depth_net(nh, in0) is a [in0, 32 x (nh + 1), 1] network with dense
random weights for any nh in 0..MAX_HIDDEN (and 17, the first depth the fused kernels refuse), whose
last layer is re-centred and re-scaled so that its zero set crosses the unit box: the tracers hit it
from CAMERA.  pad_to_seven appends identity layers, which a ReLU network evaluates exactly, so a
shallower network can be set against the 7-layer instances.

x3_error_table measures the fp32x3 emulation (oracle precision 4 over the library's own pack)
against fp64 at every depth; run as a script it prints the table of profiles/x3_depth_error.txt.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))

import oracle

F = np.float32
MAX_HIDDEN = 16
# the view, size and step cap of the depth frames (tests/test_gpu_depth.py)
CAMERA, FRAME_W, FRAME_H, FRAME_STEPS, FRAME = (-20.0, 35.0, 2.0), 72, 56, 96, 3


def depth_net(nh, in0, frame=3, scale=1.4):
    """(dims, kernels, biases) of a dense random network with nh hidden 32x32 layers: N(0, scale^2 /
    fan-in) kernels (the 4th input's row times 0.01: it carries the frame number), N(0, 0.01) biases,
    seeded by the depth.  The last layer is scaled so that the output over the unit box (4th input =
    frame) spans +-0.5 around its median, and shifted so that the median is 0."""
    rng = np.random.default_rng(100 + nh)
    dims = [in0] + [32] * (nh + 1) + [1]
    K = [(rng.standard_normal((i, o)) * scale / np.sqrt(i)).astype(F) for i, o in zip(dims[:-1], dims[1:])]
    B = [(rng.standard_normal(o) * 0.1).astype(F) for o in dims[1:]]
    if in0 == 4:
        K[0][3] *= 0.01
    P = rng.uniform(-1, 1, (4096, in0)).astype(F)
    if in0 == 4:
        P[:, 3] = frame
    B[-1][0] = 0.0
    y = oracle.OracleNet(K, B).forward(P, precision=3)[:, 0]          # fp64
    s = F(0.5 / max(np.abs(y - np.median(y)).max(), 1e-6))
    K[-1] = (K[-1] * s).astype(F)
    B[-1][0] = F(-np.median(y) * s)
    return dims, K, B


@functools.lru_cache(maxsize=None)
def cached_net(nh, in0):
    """depth_net(nh, in0), computed once and shared: read-only."""
    dims, K, B = depth_net(nh, in0)
    for a in K + B:
        a.setflags(write=False)
    return tuple(dims), tuple(K), tuple(B)


def pad_to_seven(K, B):
    """(dims, kernels, biases) with identity 32x32 layers (zero bias) appended before the final layer
    until there are 7 hidden layers: relu(I h + 0) = h for h >= 0, so the function is the same and so
    is every f32 chain of the layers before and after."""
    K, B = list(K), list(B)
    assert len(K) - 2 <= 7
    while len(K) - 2 < 7:
        K.insert(len(K) - 1, np.eye(32, dtype=F))
        B.insert(len(B) - 1, np.zeros(32, F))
    dims = [K[0].shape[0]] + [32] * (len(K) - 1) + [1]
    return dims, K, B


def insert_identity(K, B, extra, at=4):
    """The networks of test_gpu_endgame.test_endgame_deep_networks: `extra` identity layers inserted
    at layer `at`."""
    K, B = list(K), list(B)
    for _ in range(extra):
        K.insert(at, np.eye(32, dtype=F))
        B.insert(at, np.zeros(32, F))
    dims = [K[0].shape[0]] + [32] * (len(K) - 1) + [1]
    return dims, K, B


def cloud(in0, n=4096, seed=7, bound=1.2, frames=(3,)):
    """n points uniform in +-bound; a 4th column drawn from `frames`."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-bound, bound, (n, 3)).astype(F)
    if in0 == 4:
        X = np.concatenate([X, rng.choice(np.asarray(frames, F), (n, 1)).astype(F)], 1)
    return X


def x3_errors(dims, K, B, X):
    """The fp32x3 emulation and the f32 chain against fp64 on X: a dict with the pack's ok flag, the
    max and mean errors of both and max |y64|.  The pack is the library's (nr_pack_x3; host only)."""
    import cudaneuralrender_amd as nr
    a, f, ok = nr.pack_x3(list(dims), list(K), list(B))
    net = oracle.OracleNet(list(K), list(B), x3_pack=(a, f))
    y64 = net.forward(X, precision=3)[:, 0].astype(np.float64)
    e32 = np.abs(net.forward(X, precision=0)[:, 0].astype(np.float64) - y64)
    e3 = np.abs(net.forward(X, precision=4)[:, 0].astype(np.float64) - y64)
    return {"ok": int(ok), "x3_max": e3.max(), "x3_mean": e3.mean(), "f32_max": e32.max(), "f32_mean": e32.mean(),
            "scale": np.abs(y64).max()}


def in_band(r):
    """The band tests/test_gpu_fp32x3.py asserts for 7 hidden layers."""
    return r["x3_max"] <= 1e-5 * max(1.0, r["scale"]) and r["x3_mean"] <= 5 * r["f32_mean"] + 1e-9


def x3_error_table():
    """One line per depth 0..16: the error of what NR_PRECISION_FP32X3 computes (the split's
    emulation where nr_pack_x3 accepts the network, the f32 chain where it refuses it) against fp64
    as a multiple of the f32 chain's (max and mean, 3-input / 4-input network) on cloud(in0), and
    the pack's ok flags."""
    lines = ["hidden  ok (3/4)  x3 / f32 max (3-in / 4-in)   x3 / f32 mean (3-in / 4-in)   x3 max abs (3-in / 4-in)"]
    for nh in range(MAX_HIDDEN + 1):
        r = [x3_errors(*cached_net(nh, in0), cloud(in0)) for in0 in (3, 4)]
        for x in r:
            if not x["ok"]:
                x["x3_max"], x["x3_mean"] = x["f32_max"], x["f32_mean"]
        lines.append("%4d    %d / %d     %9.1f / %-9.1f       %9.1f / %-9.1f          %.2e / %.2e" % (
            nh, r[0]["ok"], r[1]["ok"], r[0]["x3_max"] / r[0]["f32_max"], r[1]["x3_max"] / r[1]["f32_max"],
            r[0]["x3_mean"] / r[0]["f32_mean"], r[1]["x3_mean"] / r[1]["f32_mean"], r[0]["x3_max"], r[1]["x3_max"]))
    return "\n".join(lines)


if __name__ == "__main__":
    print(x3_error_table())
