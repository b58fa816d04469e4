"""The inputs the nr_render_lit tests share, and light_ref.render on them: a helper, not a test.

tests/test_light_cpu.py asserts on the reference alone that these inputs exercise every rule;
tests/test_gpu_light.py compares the library against the same cached results."""
import functools

import numpy as np

import cudaneuralrender_amd as nr
import depth_nets
import light_ref
import oracle
from conftest import REF_CAMERAS

FRAME = 3
LIGHT_DIR = (-0.8, 0.6, 0.0)
LIGHT = dict(shadow_bias=0.01, shadow_k=8.0, ao_step=0.02, ao_strength=2.0, ambient=0.3)
# eye at (0, 0, 2), identity rotation (the context's default view)
IV = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 2], np.float32)
NM = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -2, 0, 0, 0, 1], np.float32)
# network, scene, W, H, camera (rx, ry, zoom) or None for the default view, max_steps
CASES = {
    "A": ("plane_1", "v1", 96, 80, REF_CAMERAS["plane_1"], 128),
    "B": ("plane_1", "v1", 64, 48, (-35.0, 30.0, 1.3), 128),
    "T": ("plane_1", "tanh", 64, 48, (-35.0, 30.0, 1.3), 128),
    "F4": ("depth7x4", "v1", 72, 56, depth_nets.CAMERA, 96),
    "AO": ("plane_1", "v1", 48, 40, None, 128),
}


@functools.lru_cache(maxsize=None)
def network(name):
    """(dims, kernels, biases, OracleNet): plane_1, or the 4-input random network of 7 hidden layers."""
    if name == "depth7x4":
        dims, K, B = depth_nets.cached_net(7, 4)
    else:
        dims, K, B = nr.read_keras_h5(nr.geometry_path(name))
    return list(dims), list(K), list(B), oracle.OracleNet(list(K), list(B))


def view(case):
    cam = CASES[case][4]
    return (IV, NM) if cam is None else nr.camera(*cam)


@functools.lru_cache(maxsize=None)
def reference(case, shadow_steps=64, shadow_k=8.0, ao_strength=2.0, light_dir=LIGHT_DIR):
    """light_ref.render for a case, computed once and shared (never modified)."""
    name, scene, W, H, _, steps = CASES[case]
    lt = dict(LIGHT, shadow_k=shadow_k, ao_strength=ao_strength)
    r = light_ref.render(network(name)[3], W, H, view(case)[0], steps, light_dir, shadow_steps, scene=nr.NR_SCENE[scene],
                         frame=FRAME, **lt)
    for a in list(r.values()) + list(r["gbuffer"].values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return r
