"""The inputs the nr_compose_render_lit tests share, and compose_light_ref.render on them: a helper,
not a test.

tests/test_compose_light_cpu.py asserts on the reference alone that these inputs exercise every rule;
tests/test_gpu_compose_light.py compares the library against the same cached results."""
import functools

import numpy as np

import compose_light_ref
import cudaneuralrender_amd as nr
import oracle
import test_gpu_query
from compose_ref import SUBTRACT, UNION, part, rot_xyz

F = np.float32


def unit(v):
    """v normalised in double, rounded to float32."""
    v = np.asarray(v, np.float64)
    return tuple(float(x) for x in (v / np.sqrt((v * v).sum())).astype(F))


LIGHT_DIR = unit((0.15, 1.0, 0.35))
LIGHT_BELOW = unit((0.1, -1.0, 0.2))
LIGHT = dict(shadow_bias=0.01, shadow_k=8.0, ao_step=0.02, ao_strength=2.0, ambient=0.3)
NM = np.eye(4, dtype=F).reshape(16)


def eye_at(z):
    """inv_view of an eye at (0, 0, z) looking down -z, set directly (not derived from nr.camera)."""
    return np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, z], F)


# L3: a plane above a car, lit from above, and a car-shaped cut in the plane
L3 = [part(1, UNION, None, (0.0, -0.15, 0.0), 1.0),
      part(0, UNION, None, (0.0, 0.35, 0.0), 1.2),
      part(1, SUBTRACT, rot_xyz(0.4, 0.2, 1.1), (0.1, -0.1, 0.35), 0.7)]
# the `four` scene of tests/test_gpu_compose.py: four packs, the LDS-tight case
FOUR = [part(i, UNION, rot_xyz(0.1 * i, 0.2, 0.3 * i), p, s)
        for i, (p, s) in enumerate([((-1.5, 0.9, 0.0), 0.8), ((1.4, 1.0, 0.2), 1.0), ((-1.3, -1.0, -0.3), 0.9), ((1.5, -0.9, 0.1), 1.1)])]
# a 4-input source network (net 0) that takes the owner's frame number
F4 = [part(0, UNION, rot_xyz(0.2, 0.1, 0.0), (-0.5, 0.0, 0.0), 0.9), part(1, UNION, None, (0.8, 0.0, 0.0), 0.7)]
# networks, parts, inv_view, max_steps, frame, light direction
SCENES = {
    "l3": (("plane_1", "car_1"), L3, eye_at(2.4), 96, 0, LIGHT_DIR),
    "one": (("car_1",), [part(0)], eye_at(2.0), 96, 0, LIGHT_DIR),
    "four": (("plane_1", "plane_2", "plane_3", "car_1"), FOUR, eye_at(4.8), 96, 0, unit((0.1, 1.0, 0.3))),
    "f4": (("plane_1x4", "car_1"), F4, eye_at(2.6), 96, 5, unit((1.0, 0.1, 0.3))),
}


@functools.lru_cache(maxsize=None)
def network(name):
    """(dims, kernels, biases, OracleNet) of a bundled geometry; plane_1x4: plane_1 with a 4th input."""
    if name == "plane_1x4":
        dims, K, B, net = test_gpu_query.plane_net(True)
    else:
        dims, K, B = nr.read_keras_h5(nr.geometry_path(name))
        net = oracle.OracleNet(list(K), list(B))
    return list(dims), list(K), list(B), net


def bound(scene):
    names, parts = SCENES[scene][:2]
    return nr.compose_bound(parts, len(names))


@functools.lru_cache(maxsize=None)
def reference(scene, W, H, shadow_steps=64, shadow_k=8.0, ao_strength=2.0, light_dir=None):
    """compose_light_ref.render for a scene, computed once and shared (never modified)."""
    names, parts, iv, steps, frame, ld = SCENES[scene]
    c, r = bound(scene)
    lt = dict(LIGHT, shadow_k=shadow_k, ao_strength=ao_strength)
    res = compose_light_ref.render([network(g)[3] for g in names], parts, c, r, W, H, iv, steps,
                                   ld if light_dir is None else light_dir, shadow_steps, frame=frame, **lt)
    for a in list(res.values()) + list(res["gbuffer"].values()):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return res
