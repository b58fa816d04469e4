"""sceneSDF on the device at points and surface values chosen against its shortcuts: nr_sample_grid
on the designed networks and lattices of tests/designed_nets.py, against the CPU oracle.

A trained network feeds the scene kernels correlated, finite, small surface values at neighbouring
points.  Here the network is an instrument (an all-zero network is its last bias, a ReLU pair is a
linear function of the point) and the lattice is built against one claim of nr_device.h at a time:
waves that straddle the v1 screen q >= T2 by ulps, waves with T <= 0, a wave scattered over all nine
spheres, a wave in which one row's q overflows (the sqrtf chain) or sits next to FLT_MAX (the short
root), NaN / infinite / tiny surface values, arguments of nr_tanh and nr_sin far outside what a
network produces, lines across |d1 + d2| = k of the smooth subtraction, and a 4-input network.
tests/test_designed_cpu.py pins that the networks compute what they are designed to and that every
lattice meets its condition.

Reference: oracle.scene_sdf(p, OracleNet(K, B).forward(p), scene, frame) at mesh_ref.lattice's
points.  Comparison: bit for bit where the reference is not NaN, NaN exactly where it is (neither
the payload nor the sign of a NaN is compared).
"""
import numpy as np
import pytest
import torch

import cudaneuralrender_amd as nr
import designed_nets as dn

pytestmark = pytest.mark.gpu
F = np.float32
CASES = {c.id: c for c in dn.cases()}
# where torch bundles a HIP runtime of its own beside libnr's, torch has to open the GPU first
if torch.cuda.is_available():
    torch.cuda.init()


@pytest.fixture(scope="module")
def rend():
    r = nr.Renderer(0)
    yield r
    r.close()


def assert_values(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype)
    nan = np.isnan(ref)
    bad = np.where(nan, ~np.isnan(got), got.view(np.uint32) != ref.view(np.uint32))
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {at}: "
                             f"{got[at]!r} ({got.view(np.uint32)[at]:#010x}) for {ref[at]!r} ({ref.view(np.uint32)[at]:#010x})")


@pytest.mark.parametrize("cid", list(CASES))
def test_scene_points(rend, cid):
    case = CASES[cid]
    _, ref = dn.reference(cid)
    dims, K, B = case.network()
    n = case.dims[0] * case.dims[1] * case.dims[2]
    rend.load_mlp(dims, K, B).set_precision("fp32").set_static(nr.NR_COLOR_FACING, dims[0]).set_scene(case.scene)
    rend.set_view(*nr.camera(0.0, 0.0, 2.0), case.frame)
    got, st = rend.sample_grid(case.origin, case.step, case.dims, with_stats=True)
    assert_values(got, ref, cid + " host")
    assert st["ray_steps"] == n and st["launches"] == 1
    if not case.device:
        return
    # the device path, on torch's current stream, with a guard band behind the lattice
    dev = torch.device("cuda:0")
    out = torch.full((n + 64,), -7.0, dtype=torch.float32, device=dev)
    try:
        rend.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        dst = rend.sample_grid_device(out.data_ptr(), case.origin, case.step, case.dims, with_stats=True)
        rend.synchronize()
    finally:
        rend.set_stream(None, own=True)
    host = out.cpu().numpy()
    assert_values(host[:n].reshape(case.dims[::-1]), ref, cid + " device")
    assert (host[n:] == -7.0).all()  # nothing is written past the lattice
    assert dst["ray_steps"] == n

