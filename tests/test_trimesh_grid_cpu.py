"""A triangle mesh's lattice calls without a GPU: the library exports them, and tests/trimesh_grid_ref.py
(existing references composed: lattice, distance / winding, marching tetrahedra) has the properties the
feature is for -- the winding-signed distance of an open mesh remeshes closed, and the default band of
the brick-sparse form is sound on the inputs tests/test_gpu_trimesh_grid.py uses."""
import ctypes

import numpy as np
import pytest

import cudaneuralrender_amd as nr
import mesh_ref
import sparse_mesh_ref as SR
import trimesh_grid_ref as G

SYMBOLS = ("nr_mesh_sample_grid", "nr_mesh_remesh", "nr_mesh_remesh_sparse")
METHODS = ("sample_grid", "sample_grid_device", "remesh", "remesh_device", "remesh_sparse", "remesh_sparse_device")
NR_HOST, NR_E_INVALID = 0, -1  # include/neural_render.h


def test_exports():
    L = ctypes.CDLL(nr._lib.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(L, s), f"libnr.so does not export {s}"
        assert getattr(nr.lib(), s).argtypes is not None, f"{s} has no ctypes prototype"
    for m in METHODS:
        assert callable(getattr(nr.TriMesh, m, None)), f"TriMesh.{m} is missing"
    assert nr.lib().nr_abi_version() == 3


def test_null_mesh_is_invalid_without_a_context():
    L = nr.lib()
    o, s, d = (ctypes.c_float * 3)(0, 0, 0), (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_int * 3)(2, 2, 2)
    buf = (ctypes.c_float * 8)()
    nv, nt = ctypes.c_long(7), ctypes.c_long(7)
    assert L.nr_mesh_sample_grid(None, o, s, d, 0, 0.0, 0, buf, NR_HOST, None) == NR_E_INVALID
    assert b"nr_mesh_sample_grid" in L.nr_last_error(None)
    assert L.nr_mesh_remesh(None, o, s, d, 0.0, 0, 0.0, None, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt),
                               NR_HOST, None) == NR_E_INVALID
    assert b"nr_mesh_remesh" in L.nr_last_error(None)
    assert L.nr_mesh_remesh_sparse(None, o, s, d, 0.0, 0, 0.0, 4, 0.0, None, None, None, 0, None, 0, ctypes.byref(nv),
                                      ctypes.byref(nt), None, NR_HOST, None) == NR_E_INVALID
    assert b"nr_mesh_remesh_sparse" in L.nr_last_error(None)


def test_repair_reference():
    """the reason for the feature, on the references alone: the winding sign closes what the
    pseudonormal sign leaves open"""
    closed = G.remesh(*G.repair_values("cube", "normal")[:3])
    wind = G.remesh(*G.repair_values("open_cube", "exact")[:3])
    assert mesh_ref.is_closed_oriented(closed[1])
    assert mesh_ref.is_closed_oriented(wind[1])
    print(f"cube: {len(closed[0])} vertices, {len(closed[1])} triangles; open_cube, winding sign: {len(wind[0])}, {len(wind[1])}")
    assert (len(wind[0]), len(wind[1])) == (len(closed[0]), len(closed[1])) == (2594, 5184)
    normal = G.remesh(*G.repair_values("open_cube", "normal")[:3])
    print(f"open_cube, pseudonormal sign: {len(normal[0])} vertices, {len(normal[1])} triangles")
    assert not mesh_ref.is_closed_oriented(normal[1])
    assert len(normal[0]) == 4522


@pytest.mark.parametrize("iso", G.SPARSE_ISOS)
@pytest.mark.parametrize("name", list(G.SPARSE_CASES))
def test_default_band_is_sound(name, iso):
    """the GPU tests' sparse inputs: every brick with a crossing cell is active at the default band,
    and a sparse test cannot pass by keeping every brick"""
    sign = "exact" if G.SPARSE_CASES[name] == "winding" else "normal"
    sdf, origin, step, dims = G.repair_values(name, sign)
    B = 4
    band = SR.default_band(step, B)
    need = SR.smallest_sound_band(sdf, B, iso)
    active = SR.active_bricks(sdf, B, iso, band)
    print(f"{name} iso {iso}: {int(active.sum())} of {active.size} bricks active; sound band {need:.4f}, default {float(band):.4f}")
    assert active.size == 990
    assert need <= float(band)
    assert 1 <= active.sum() <= 0.75 * active.size
    assert not (SR.crossing_bricks(sdf, B, iso) & ~active).any()
