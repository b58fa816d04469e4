"""The oracle's restatements and the library's fp32x3 pack at every network depth the fused kernels
take (0..16 hidden 32x32 layers), on the CPU: tests/depth_nets.py's dense random networks, 4096
points uniform in +-1.2 (4th input 3).

fp32x3 is documented as fp32-class (include/neural_render.h: ~2-3x the f32 chain's error).  The
pack's scales come from interval bounds whose slack compounds with depth; past ~8 dense hidden
layers the activations sink so far below the scales' window that the fp16 residuals underflow and
the error grows 2-3x per layer (profiles/x3_depth_error.txt).  The contract checked here: at every
depth the pack either keeps the band tests/test_gpu_fp32x3.py asserts at 7 hidden layers, or
nr_pack_x3 refuses it (ok = 0: the kernels run the fp32 MLP).  tests/test_gpu_depth.py holds the
GPU to these restatements bit for bit.
"""
import functools

import numpy as np
import pytest

import cudaneuralrender_amd as nr
import depth_nets
import oracle
from conftest import GEOMS

DEPTHS = list(range(depth_nets.MAX_HIDDEN + 1))


@functools.lru_cache(maxsize=None)
def errors(nh, in0):
    return depth_nets.x3_errors(*depth_nets.cached_net(nh, in0), depth_nets.cloud(in0))


def assert_band(r, what):
    assert r["x3_max"] <= 1e-5 * max(1.0, r["scale"]), (what, r)
    assert r["x3_mean"] <= 5 * r["f32_mean"] + 1e-9, (what, r)


@pytest.mark.parametrize("in0", [3, 4])
@pytest.mark.parametrize("nh", DEPTHS)
def test_x3_pack_fp32_class_or_refused(nh, in0):
    r = errors(nh, in0)
    print(f"nh {nh} in0 {in0}: ok {r['ok']} x3 max {r['x3_max']:.3e} mean {r['x3_mean']:.3e}, "
          f"f32 max {r['f32_max']:.3e} mean {r['f32_mean']:.3e}, max |y64| {r['scale']:.3f}")
    if not r["ok"]:
        return
    assert_band(r, (nh, in0))


def test_x3_pack_kept_at_shallow_depths():
    """The refusal is not a blanket one: up to 7 hidden layers (the bundled shape) every depth
    network keeps its pack."""
    for in0 in (3, 4):
        for nh in range(8):
            assert errors(nh, in0)["ok"], (nh, in0)


def test_x3_pack_refusal_is_deterministic():
    """ok is a function of the network alone: the same network packed twice, and after another
    network was packed in between, gives the same flag and the same pack."""
    net = [list(x) for x in depth_nets.cached_net(12, 4)]
    a0, f0, ok0 = nr.pack_x3(*net)
    nr.pack_x3(*[list(x) for x in depth_nets.cached_net(3, 3)])
    a1, f1, ok1 = nr.pack_x3(*net)
    assert ok0 == ok1 and np.array_equal(a0, a1) and np.array_equal(f0.view(np.uint32), f1.view(np.uint32))


@pytest.mark.parametrize("geom", GEOMS)
def test_bundled_networks_keep_their_pack(nets, geom):
    dims, K, B = nets[geom]
    r = depth_nets.x3_errors(dims, K, B, depth_nets.cloud(3))
    assert r["ok"] == 1, geom
    assert_band(r, geom)


@pytest.mark.parametrize("extra", [2, 5])
def test_identity_deepened_network_keeps_its_pack(nets, extra):
    """test_gpu_endgame.test_endgame_deep_networks' networks (plane_1 with identity layers inserted: 9
    and 12 hidden layers): identity layers add no slack to the bounds, so depth alone refuses nothing."""
    dims, K, B = depth_nets.insert_identity(nets["plane_1"][1], nets["plane_1"][2], extra)
    assert len(dims) - 3 == 7 + extra
    r = depth_nets.x3_errors(dims, K, B, depth_nets.cloud(3))
    assert r["ok"] == 1
    assert_band(r, extra)


@pytest.mark.parametrize("in0", [3, 4])
@pytest.mark.parametrize("nh", range(7))
def test_identity_padding_is_exact_on_the_oracle(nh, in0):
    dims, K, B = depth_nets.cached_net(nh, in0)
    pd, pK, pB = depth_nets.pad_to_seven(K, B)
    assert pd == [in0] + [32] * 8 + [1] and len(pK) == 9
    X = depth_nets.cloud(in0)
    y = oracle.OracleNet(list(K), list(B)).forward(X)
    yp = oracle.OracleNet(pK, pB).forward(X)
    assert np.array_equal(y.view(np.uint32), yp.view(np.uint32))
    assert np.abs(y).max() > 0.05


@pytest.mark.parametrize("in0", [3, 4])
@pytest.mark.parametrize("nh", DEPTHS)
def test_emulations_do_not_run_away(nh, in0):
    """The bf16 and fp16 restatements (precision 1, 2) and what fp32x3 computes (precision 4 over an
    accepted pack, the f32 chain for a refused one) against fp64: within 0.1, 0.02 and the fp32x3
    band on outputs spanning +-0.5.  Measured maxima over all depths: 0.05 (bf16), 0.006 (fp16)."""
    dims, K, B = depth_nets.cached_net(nh, in0)
    X = depth_nets.cloud(in0)
    net = oracle.OracleNet(list(K), list(B))
    y64 = net.forward(X, precision=3)[:, 0].astype(np.float64)
    e = {p: np.abs(net.forward(X, precision=p)[:, 0].astype(np.float64) - y64).max() for p in (1, 2)}
    r = errors(nh, in0)
    x3 = r["x3_max"] if r["ok"] else r["f32_max"]
    print(f"nh {nh} in0 {in0}: bf16 {e[1]:.3e} fp16 {e[2]:.3e} fp32x3 {x3:.3e}")
    assert np.abs(y64).max() > 0.4
    assert e[1] < 0.1 and e[2] < 0.02, e
    assert x3 <= 1e-5 * max(1.0, r["scale"])
