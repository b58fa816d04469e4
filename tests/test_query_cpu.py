"""CPU side of the ray queries: tests/query_ref.py (the numpy restatement the GPU tests compare
against) reproduces the oracle's frames bit for bit, and libnr.so exports the entry points."""
import ctypes

import numpy as np
import pytest

import cudaneuralrender_amd as nr
from cudaneuralrender_amd import _lib
import oracle
import query_ref

# eye at (0, 0, 2), identity rotation (the context's default view)
IV = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 2], np.float32)
NM = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -2, 0, 0, 0, 1], np.float32)
FRAME = 3


# (scene, W, H, max_steps, the oracle's ray-steps, rays that reach the iteration cap)
@pytest.mark.parametrize("scene,W,H,steps,ray_steps,nlimit",
                         [("tanh", 40, 40, 6000, 19863, 0), ("v1", 32, 32, 6000, 15111, 0),
                          ("tanh", 40, 40, 20, 14317, 131)])
def test_reference_reproduces_the_oracle_frame(nets, scene, W, H, steps, ray_steps, nlimit):
    """The helper's HIT mask + facing() is or_render's frame, and the sum of its steps the oracle's
    ray-steps: the helper only transposes the oracle from pixels to rays."""
    dims, K, B = nets["plane_1"]
    net = oracle.OracleNet(K, B)
    sc = nr.NR_SCENE[scene]
    frame, rst = net.render(W, H, IV, NM, frame=FRAME, color_type=0, scene=sc, max_steps=steps)
    O, D = query_ref.pixel_rays(W, H, IV)
    out, st = query_ref.trace(net, O, D, steps, scene=sc, frame=FRAME)
    img = query_ref.facing(out["normal"], D, out["status"]).reshape(H, W)
    assert np.array_equal(img, frame), f"{(img != frame).sum()} pixels differ"
    assert np.array_equal(out["status"].reshape(H, W) == query_ref.HIT, frame != 0)
    assert st["ray_steps"] == rst["ray_steps"] == ray_steps
    for k in ("shade_evals", "rays_hit", "rays_shaded"):
        assert st[k] == rst[k], (k, st, rst)
    assert int((out["status"] == query_ref.LIMIT).sum()) == nlimit
    # the unshaded statuses carry zeros, a miss took no step
    off = out["status"] != query_ref.HIT
    assert not out["t"][off].any() and not out["position"][off].any() and not out["normal"][off].any()
    assert not out["steps"][out["status"] == query_ref.MISS].any()


def test_library_exports_the_ray_queries():
    """nr_trace_rays and nr_render_gbuffer exist in libnr.so, the binding declares them, and both
    reject a NULL context without touching a device."""
    L = nr.lib()
    for name in ("nr_trace_rays", "nr_render_gbuffer"):
        assert name in _lib.EXPORTS
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None
    z = np.zeros(3, np.float32)
    assert L.nr_trace_rays(None, z.ctypes.data, z.ctypes.data, 1, 10, None, None, None, None, None, _lib.NR_HOST,
                           None) == -1
    assert L.nr_render_gbuffer(None, 4, 4, 10, None, None, None, None, None, _lib.NR_HOST, None) == -1
    assert b"NULL" in L.nr_last_error(None)
    assert (nr.NR_RAY_MISS, nr.NR_RAY_ESCAPED, nr.NR_RAY_HIT, nr.NR_RAY_LIMIT) == (0, 1, 2, 3)
    assert ctypes.sizeof(_lib.NRStats) == 64  # nr_stats is unchanged: the ABI version stays 3
    assert L.nr_abi_version() == 3
