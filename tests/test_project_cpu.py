"""CPU side of nr_project_points: libnr.so exports the entry point, and tests/project_ref.py (the numpy
restatement the GPU tests compare against) returns points whose values have the oracle's bits, lie on
the level set, and take step counts spread widely enough to exercise the kernel's refill."""
import functools

import numpy as np

import cudaneuralrender_amd as nr
from cudaneuralrender_amd import _lib
import grad_ref
import oracle
import project_ref

NP = 1063  # 16 full chunks of 64 and a tail of 39
TOL, MAX_STEP, MAX_ITERS = 1e-5, 0.25, 32


@functools.lru_cache(maxsize=None)
def plane():
    _, K, B = nr.read_keras_h5(nr.geometry_path("plane_1"))
    return K, B


@functools.lru_cache(maxsize=None)
def points():
    X = np.random.default_rng(7).uniform(-1, 1, (NP, 3)).astype(np.float32)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def reference():
    K, B = plane()
    out = project_ref.project(K, B, points(), 0.0, TOL, MAX_STEP, MAX_ITERS)
    for a in out.values():
        a.setflags(write=False)
    return out


def test_library_exports_the_projection():
    """nr_project_points exists in libnr.so, the binding declares it, and it rejects a NULL context
    without touching a device."""
    L = nr.lib()
    assert "nr_project_points" in _lib.EXPORTS
    assert hasattr(L, "nr_project_points")
    assert L.nr_project_points.argtypes is not None and len(L.nr_project_points.argtypes) == 12
    z = np.zeros(3, np.float32)
    opts = _lib.NRProjectOpts(0.0, 1e-5, 0.25, 32)
    assert L.nr_project_points(None, z.ctypes.data, 1, opts, z.ctypes.data, None, None, None, None, None, _lib.NR_HOST,
                               None) == -1
    assert b"NULL" in L.nr_last_error(None)
    assert L.nr_abi_version() == 3
    assert hasattr(nr.Renderer, "project_points") and hasattr(nr.Renderer, "project_points_device")
    assert (_lib.NR_PROJ_CONVERGED, _lib.NR_PROJ_LIMIT, _lib.NR_PROJ_FLAT) == (0, 1, 2)


def test_converged_values_are_the_oracles_bits():
    K, B = plane()
    ref = reference()
    conv = ref["status"] == project_ref.CONVERGED
    v = oracle.OracleNet(K, B).forward(ref["position"][conv])[:, 0]
    assert np.array_equal(v.view(np.uint32), ref["value"][conv].view(np.uint32))


def test_converged_points_lie_on_the_level_set_in_f64():
    """|f64 forward - iso| <= tol + 5e-6 (the bound tests/golden/mlp_kat.npz pins between the fp32
    oracle and fp64)."""
    K, B = plane()
    ref = reference()
    conv = ref["status"] == project_ref.CONVERGED
    a = ref["position"][conv].astype(np.float64)
    for l, (W, b) in enumerate(zip(K, B)):
        a = a @ np.asarray(W, np.float64) + np.asarray(b, np.float64)
        if l < len(K) - 1:
            a = np.maximum(a, 0)
    err = np.abs(a[:, 0] - 0.0)
    print(f"max |f64 value| over {int(conv.sum())} converged points: {err.max():.3e}")
    assert err.max() <= TOL + 5e-6


def test_converged_share_and_step_histogram():
    """At least 99 % of the points converge (a condition on the sample, fixed in advance), and the
    step counts span 2..max_iters, so that the GPU test's waves refill with mixed lifetimes."""
    ref = reference()
    share = (ref["status"] == project_ref.CONVERGED).mean()
    hist = np.bincount(ref["iters"], minlength=MAX_ITERS + 1)
    print(f"converged {share:.4f}; steps min {ref['iters'].min()}, median {int(np.median(ref['iters']))}, "
          f"max {ref['iters'].max()}; histogram {hist.tolist()}")
    assert share >= 0.99
    assert ref["iters"].min() <= 2 and ref["iters"].max() == MAX_ITERS
    lim = ref["status"] == project_ref.LIMIT
    assert (ref["iters"][lim] == MAX_ITERS).all()
    assert set(np.unique(ref["status"])) <= {project_ref.CONVERGED, project_ref.LIMIT, project_ref.FLAT}


def test_distance_is_the_signed_chord():
    ref = reference()
    K, B = plane()
    v0 = grad_ref.gradient(K, B, points())[0]
    d = np.linalg.norm(ref["position"].astype(np.float64) - points().astype(np.float64), axis=1)
    assert np.allclose(np.abs(ref["distance"]), d, rtol=1e-5, atol=1e-7)
    assert np.array_equal(np.signbit(ref["distance"]), v0 < 0)


def test_max_iters_zero_is_the_gradient():
    K, B = plane()
    X = points()
    out = project_ref.project(K, B, X, 0.0, TOL, MAX_STEP, 0)
    v, _, nrm = grad_ref.gradient(K, B, X)
    assert np.array_equal(out["value"].view(np.uint32), v.view(np.uint32))
    assert np.array_equal(out["normal"].view(np.uint32), nrm.view(np.uint32))
    assert np.array_equal(out["position"].view(np.uint32), X.view(np.uint32))
    assert (out["iters"] == 0).all()
    assert set(np.unique(out["status"])) <= {project_ref.CONVERGED, project_ref.LIMIT}
    assert project_ref.stats(out)["ray_steps"] == NP
