"""Reference for the composed-scene lattice calls (nr_compose_sample_grid, nr_compose_extract_mesh,
nr_compose_extract_mesh_sparse): a helper, not a test.

Nothing new is stated here: the contract composes existing ones, and so does this file -- the
composed field of tests/compose_ref.py on the lattice points of tests/mesh_ref.py, meshed by
mesh_ref.mesh (dense) or sparse_mesh_ref.mesh (brick-culled), with the tetrahedral normal rule of
compose_ref.trace applied to the vertex positions and compose_ref.field's owner at the vertices as
the part.  tests/test_compose_mesh_cpu.py pins what it gives on the cases the GPU test uses.  The
scenes and lattices of those cases live here, so both test files share them.
"""
import functools

import numpy as np

import compose_ref
import cudaneuralrender_amd as nr
import mesh_ref
import oracle
import sparse_mesh_ref as sref
from compose_ref import SUBTRACT, UNION, part, rot_xyz
from query_ref import NORMAL_EPSILON, TET, normalize3

F = np.float32

# scene S3 of tests/test_gpu_compose.py (nets plane_1, car_1) and its four-network scene
S3_NETS = ("plane_1", "car_1")
S3 = [part(0, UNION, None, (-0.9, 0.0, 0.0), 1.0),
      part(1, UNION, rot_xyz(0.3, 1.0, -0.2), (1.0, 0.2, 0.1), 0.75),
      part(1, SUBTRACT, rot_xyz(1.2, 0.4, 0.5), (-0.9, 0.0, 0.0), 0.6)]
FOUR_NETS = ("plane_1", "plane_2", "plane_3", "car_1")
FOUR = [part(i, UNION, rot_xyz(0.1 * i, 0.2, 0.3 * i), p, s)
        for i, (p, s) in enumerate([((-1.5, 0.9, 0.0), 0.8), ((1.4, 1.0, 0.2), 1.0), ((-1.3, -1.0, -0.3), 0.9), ((1.5, -0.9, 0.1), 1.1)])]
SCENES = {"s3": (S3_NETS, S3), "four": (FOUR_NETS, FOUR)}

# the S3 lattice (183,015 points: the largest shape any test uses) and its ragged variant, whose last
# bricks of 4 are 1, 3 and 2 cells
S3_ORIGIN, S3_STEP, S3_DIMS = (-2.15, -1.2, -1.15), (0.05, 0.055, 0.05), (83, 45, 49)
RAGGED_DIMS = (82, 44, 47)
# a coarse lattice over the four-network scene (n % 64 != 0)
FOUR_ORIGIN, FOUR_STEP, FOUR_DIMS = (-2.6, -2.1, -1.4), (0.23, 0.21, 0.25), (23, 21, 11)
# the lone identity part: a lattice inside the bound, every point and tetrahedron sample with qq <= 1.45
LONE_ORIGIN, LONE_STEP, LONE_DIMS = (-0.66, -0.68, -0.69), (0.055, 0.052, 0.049), (25, 27, 29)


@functools.lru_cache(maxsize=None)
def onet(name):
    dims, K, B = nr.read_keras_h5(nr.geometry_path(name))
    return oracle.OracleNet(K, B)


def scene_nets(scene):
    return [onet(g) for g in SCENES[scene][0]]


def sample(nets, parts, origin, step, dims, frame=0):
    """nr_compose_sample_grid: (value [nz, ny, nx], owner [nz, ny, nx], in-bound (point, part) pairs)"""
    d, own, pairs = compose_ref.field(nets, parts, mesh_ref.lattice(origin, step, dims), frame)
    shape = (dims[2], dims[1], dims[0])
    return d.reshape(shape), own.reshape(shape), pairs


def normals(nets, parts, V, frame=0):
    """The composed vertex normals: compose_ref.trace's tetrahedron formula at each vertex."""
    V = np.ascontiguousarray(V, F).reshape(-1, 3)
    if not len(V):
        return np.zeros((0, 3), F)
    acc = None
    with np.errstate(all="ignore"):
        for q in range(4):
            pq = (V + TET[q] * NORMAL_EPSILON).astype(F)
            c = TET[q][None, :] * compose_ref.field(nets, parts, pq, frame)[0][:, None]
            acc = c if acc is None else acc + c
        return normalize3(acc)


def owners(nets, parts, V, frame=0):
    """part[v]: the owner of the composed field at each vertex"""
    V = np.ascontiguousarray(V, F).reshape(-1, 3)
    return compose_ref.field(nets, parts, V, frame)[1] if len(V) else np.zeros(0, np.int32)


def inbound_counts(parts, origin, step, dims):
    """[nz, ny, nx]: the number of parts whose bound holds each lattice point (compose_ref.field's
    arithmetic for qq) -- what a point adds to part_evals each time it is evaluated"""
    P = mesh_ref.lattice(origin, step, dims)
    cnt = np.zeros(len(P), np.int64)
    with np.errstate(all="ignore"):
        for p in parts:
            R = p["rot"].reshape(9)
            inv_s = F(1.0) / F(p["scale"])
            v = (P - p["pos"][None, :]).astype(F)
            q = np.stack([((v[:, 0] * R[0 + k] + v[:, 1] * R[3 + k]) + v[:, 2] * R[6 + k]) * inv_s for k in range(3)], 1).astype(F)
            cnt += compose_ref.dot3(q, q) <= compose_ref.IN_BOUND
    return cnt.reshape(dims[2], dims[1], dims[0])


def sparse_pairs(cnt, active, B):
    """part_evals of the sparse call: the counts at the brick corners plus, for every active brick,
    over its point set"""
    nz, ny, nx = cnt.shape
    total = int(sref.corner_values(cnt, B).sum())
    for bz, by, bx in np.argwhere(active):
        total += int(cnt[B * bz:min(B * bz + B, nz - 1) + 1, B * by:min(B * by + B, ny - 1) + 1,
                         B * bx:min(B * bx + B, nx - 1) + 1].sum())
    return total


# ---- the shared references: computed once per case, never modified -----------------------------

def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def ref_grid(scene, origin=S3_ORIGIN, step=S3_STEP, dims=S3_DIMS):
    """(value, owner, pairs) of the scene on a lattice"""
    return _frozen(*sample(scene_nets(scene), SCENES[scene][1], origin, step, dims))


@functools.lru_cache(maxsize=None)
def ref_dense(scene, iso=0.0, origin=S3_ORIGIN, step=S3_STEP, dims=S3_DIMS):
    """(V, T, cells, keys, N, part) of nr_compose_extract_mesh"""
    V, T, cells, keys = mesh_ref.mesh(ref_grid(scene, origin, step, dims)[0], origin, step, iso)
    nets, parts = scene_nets(scene), SCENES[scene][1]
    return _frozen(V, T, cells, keys, normals(nets, parts, V), owners(nets, parts, V))


@functools.lru_cache(maxsize=None)
def ref_sparse(scene, brick, band, dims=S3_DIMS, iso=0.0, origin=S3_ORIGIN, step=S3_STEP):
    """(V, T, cells, keys, N, active, part) of nr_compose_extract_mesh_sparse, in key order (the
    layout tests/test_gpu_sparse_mesh.py's comparisons take, with the part appended)"""
    V, T, cells, keys, active = sref.mesh(ref_grid(scene, origin, step, dims)[0], origin, step, brick, iso, F(band))
    nets, parts = scene_nets(scene), SCENES[scene][1]
    return _frozen(V, T, cells, keys, normals(nets, parts, V), active, owners(nets, parts, V))
