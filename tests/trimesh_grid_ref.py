"""Reference for a triangle mesh's lattice calls (nr_mesh_sample_grid, nr_mesh_remesh,
nr_mesh_remesh_sparse): a helper, not a test.

There is no arithmetic here: the contract in include/neural_render.h composes existing rules, and so
does this file -- mesh_ref.lattice's points, then trimesh_ref.distance (the pseudonormal sign) or that
magnitude signed by winding_ref's winding number, then mesh_ref.mesh / sparse_mesh_ref.mesh."""
import functools

import numpy as np

import mesh_ref
import sparse_mesh_ref
import trimesh_ref as R
import winding_ref as WR

F = np.float32
GROW_LO, GROW_HI = 1.13, 1.07      # the repair lattice: the mesh's bound grown by these, per axis
REPAIR_DIMS = (45, 41, 37)         # no axis a multiple of 4 cells plus one on all three; 11 x 10 x 9 bricks of 4
MESHES = dict(WR.MESHES, degenerate_torus=(R.degenerate_torus, "torus"))


@functools.lru_cache(maxsize=None)
def mesh(name):
    V, T = MESHES[name][0]()
    V, T = np.array(V, F), np.array(T, np.int32)
    V.setflags(write=False)
    T.setflags(write=False)
    return V, T


def bound_lattice(V, dims, lo=GROW_LO, hi=GROW_HI):
    """(origin, step) of a dims lattice over the vertices' bound grown by lo below and hi above"""
    a = np.asarray(V, np.float64).min(0) - lo
    b = np.asarray(V, np.float64).max(0) + hi
    step = [(b[k] - a[k]) / max(dims[k] - 1, 1) for k in range(3)]
    return tuple(float(F(x)) for x in a), tuple(float(F(x)) for x in step)


def signed(magnitude, w):
    """nr_mesh_winding's sdf rule: -|m| where w >= 0.5 (f32 compare for an f32 w), |m| elsewhere, a NaN kept"""
    m = np.asarray(magnitude, F)
    with np.errstate(all="ignore"):
        inside = np.asarray(w) >= (F(0.5) if np.asarray(w).dtype == F else 0.5)
        out = np.where(inside, -np.abs(m), np.abs(m)).astype(F)
    return np.where(np.isnan(m), m, out).astype(F)


def values(V, T, origin, step, dims, sign="normal", beta=2.0, tree=None, brute=False, normal=None):
    """nr_mesh_sample_grid's values [nz, ny, nx].  sign "normal": trimesh_ref.distance's sdf.
    "winding": its magnitude signed by winding_ref.winding through `tree` = (nodes, order, moments)
    of nr_mesh_hierarchy.  "exact": signed by winding_ref.exact (plain float64; no library needed).
    normal: the "normal" values of this lattice where the caller has them (the magnitude is theirs)."""
    P = mesh_ref.lattice(origin, step, dims)
    d = R.distance(V, T, P)["sdf"] if normal is None else np.asarray(normal, F).reshape(-1)
    if sign == "winding":
        nodes, order, moments = tree[:3]
        d = signed(d, WR.winding(V, T, P, beta, nodes, order, moments, brute=brute))
    elif sign == "exact":
        d = signed(d, WR.exact(V, T, P))
    else:
        assert sign == "normal", sign
    return d.reshape(dims[2], dims[1], dims[0])


def remesh(sdf, origin, step, iso=0.0):
    """nr_mesh_remesh's (V, T, cells, keys) for the values sdf: mesh_ref.mesh"""
    return mesh_ref.mesh(sdf, origin, step, iso)


def remesh_sparse(sdf, origin, step, B, iso, band):
    """nr_mesh_remesh_sparse's (V, T, cells, keys, active) in key order: sparse_mesh_ref.mesh"""
    return sparse_mesh_ref.mesh(sdf, origin, step, B, iso, band)


# the sparse tests' inputs (GPU and CPU): mesh -> the sign its field is taken with
SPARSE_CASES = {"cube": "normal", "tetrahedron": "normal", "open_cube": "winding"}
SPARSE_ISOS = (0.0, 0.05)


@functools.lru_cache(maxsize=None)
def repair_values(name, sign):
    """values() of mesh `name` on its repair lattice, computed once and shared (read-only):
    (sdf, origin, step, dims)"""
    V, T = mesh(name)
    origin, step = bound_lattice(V, REPAIR_DIMS)
    sdf = values(V, T, origin, step, REPAIR_DIMS, sign)
    sdf.setflags(write=False)
    return sdf, origin, step, REPAIR_DIMS
