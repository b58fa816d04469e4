"""CPU side of the isosurface extraction: tests/mesh_ref.py (the numpy restatement the GPU tests
compare against) produces closed, consistently oriented meshes that lie on the surface, reaches
every case of the triangle rule, and shares vertices between cells; nr_obj_save round-trips."""
import ctypes

import numpy as np
import pytest

import cudaneuralrender_amd as nr
from cudaneuralrender_amd import _lib
import mesh_ref

F = np.float32
# a sphere of radius 0.5 on an anisotropic 13 x 11 x 9 lattice that contains it
R = 0.5
S_ORIGIN, S_STEP, S_DIMS = (-0.8, -0.75, -0.7), (0.13, 0.15, 0.17), (13, 11, 9)


@pytest.fixture(scope="module")
def sphere():
    P = mesh_ref.lattice(S_ORIGIN, S_STEP, S_DIMS)
    sdf = (np.sqrt((P.astype(np.float64) ** 2).sum(1)) - R).astype(F).reshape(S_DIMS[::-1])
    return mesh_ref.mesh(sdf, S_ORIGIN, S_STEP, 0.0)


def test_lattice_is_one_multiply_and_one_add():
    P = mesh_ref.lattice(S_ORIGIN, S_STEP, S_DIMS).reshape(S_DIMS[2], S_DIMS[1], S_DIMS[0], 3)
    i, j, k = 7, 10, 8
    want = [F(S_ORIGIN[a]) + F(idx) * F(S_STEP[a]) for a, idx in enumerate((i, j, k))]
    assert [v.tobytes() for v in P[k, j, i]] == [F(w).tobytes() for w in want]


def test_sphere_is_a_closed_oriented_manifold_on_the_surface(sphere):
    V, T, cells, keys = sphere
    assert len(V) > 300 and len(T) > 600
    assert (np.diff(keys) > 0).all()  # the pinned vertex order
    # every directed edge once, its reverse once
    assert mesh_ref.is_closed_oriented(T)
    # Euler characteristic of a sphere: V - E + F with E = 3 F / 2
    assert len(V) - 3 * len(T) // 2 + len(T) == 2
    a, b, c = (V[T[:, m]].astype(np.float64) for m in range(3))
    vol = np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0
    assert vol > 0  # outward winding
    assert 0.9 * 4 / 3 * np.pi * R ** 3 < vol < 4 / 3 * np.pi * R ** 3  # inscribed in the convex ball
    # linear interpolation of a distance field along an edge of length <= L, L the cell's diagonal
    L = float(np.linalg.norm(np.asarray(S_STEP, np.float64)))
    err = np.abs(np.linalg.norm(V.astype(np.float64), axis=1) - R)
    print("max | |v| - r | =", err.max(), "bound", L * L / (8 * (R - L)) + 1e-6)
    assert (err <= L * L / (8 * (R - L)) + 1e-6).all()
    # each triangle's vertices lie on edges of the cell it is listed under
    assert np.array_equal(mesh_ref.triangle_cells(T, keys, S_DIMS), cells)
    assert (np.diff(cells) >= 0).all()


def test_random_lattice_reaches_every_case():
    """Every (tetrahedron, mask) pair with mask 1 .. 14 occurs on the 6 x 5 x 4 lattice: the GPU
    comparison on it covers the whole triangle table."""
    masks = mesh_ref.tet_masks(mesh_ref.random_lattice(), 0.0)
    assert masks.shape == (60, 6)
    hist = np.stack([np.bincount(masks[:, t], minlength=16) for t in range(6)])
    assert hist.tolist() == [[1, 5, 6, 4, 2, 7, 3, 2, 4, 3, 6, 4, 5, 3, 4, 1], [2, 3, 4, 3, 1, 9, 5, 3, 4, 4, 6, 2, 5, 2, 4, 3],
                             [2, 5, 5, 4, 3, 7, 2, 2, 3, 4, 7, 3, 4, 4, 5, 0], [3, 5, 1, 2, 2, 7, 6, 4, 4, 4, 7, 1, 3, 4, 5, 2],
                             [3, 1, 3, 5, 5, 6, 1, 6, 3, 3, 7, 3, 5, 3, 4, 2], [2, 3, 2, 4, 6, 4, 2, 7, 5, 1, 6, 4, 3, 5, 5, 1]]
    assert (hist[:, 1:15] >= 1).all()
    # the triangle count follows the masks: one for 1 or 3 inside corners, two for 2
    V, T, cells, keys = mesh_ref.mesh(mesh_ref.random_lattice(), mesh_ref.RANDOM_ORIGIN, mesh_ref.RANDOM_STEP, 0.0)
    pop = np.array([bin(m).count("1") for m in range(16)])
    assert len(T) == int(np.where(pop[masks] == 2, 2, (pop[masks] % 4 != 0).astype(int)).sum()) == 502
    assert len(V) == 304 and len(set(cells.tolist())) == 60


def test_triangle_rule_winding_and_edges():
    """The derived table: every triangle is on three distinct crossing edges of its tetrahedron,
    and the two triangles of a 2-2 case share the diagonal AC-BD with opposite directions."""
    for t in range(6):
        path = [tuple(v) for v in mesh_ref.tet_path(t)]
        for mask in range(1, 15):
            tris = mesh_ref.tet_triangles(t, mask)
            assert len(tris) == (2 if bin(mask).count("1") == 2 else 1)
            for tri in tris:
                assert len(set(tri)) == 3
                for base, slot in tri:
                    end = tuple(np.add(base, mesh_ref.SLOTS[slot]))
                    assert ((mask >> path.index(base)) & 1) != ((mask >> path.index(end)) & 1)
            if len(tris) == 2:
                d0 = {(tris[0][r], tris[0][(r + 1) % 3]) for r in range(3)}
                d1 = {(tris[1][(r + 1) % 3], tris[1][r]) for r in range(3)}
                assert len(d0 & d1) == 1


def test_cells_share_vertices():
    """Triangles of adjacent cells use the same vertex ids on their common face: on the random
    lattice (open at the lattice faces) no directed edge repeats, and an edge without its reverse has
    both vertices on lattice edges that lie in one boundary face of the lattice."""
    sdf = mesh_ref.random_lattice()
    nz, ny, nx = sdf.shape
    V, T, cells, keys = mesh_ref.mesh(sdf, mesh_ref.RANDOM_ORIGIN, mesh_ref.RANDOM_STEP, 0.0)
    E = mesh_ref.directed_edges(T)
    fwd = {(int(a), int(b)) for a, b in E}
    assert len(fwd) == len(E)
    base, slot = keys // 7, keys % 7
    lo = np.stack([base % nx, (base // nx) % ny, base // (nx * ny)], -1)
    hi = lo + mesh_ref.SLOTS[slot]
    # the boundary faces (axis, side) that hold a vertex's whole lattice edge
    dims = np.array([nx, ny, nz])
    faces = [{(a, 0) for a in range(3) if h[a] == 0} | {(a, 1) for a in range(3) if l[a] == dims[a] - 1}
             for l, h in zip(lo, hi)]
    open_edges = [(a, b) for a, b in fwd if (b, a) not in fwd]
    assert len(open_edges) > 50 and len(fwd) - len(open_edges) > 500
    for a, b in open_edges:
        assert faces[a] & faces[b], (a, b)


@pytest.mark.parametrize("with_normals", [False, True])
def test_obj_round_trip(tmp_path, with_normals):
    rng = np.random.default_rng(3)
    V = rng.normal(size=(40, 3)).astype(F)
    V[0] = [0.0, -0.0, 1e-45]       # zero, minus zero, the smallest subnormal
    V[1] = [3.4028235e38, -1.17549435e-38, 1 / 3]
    N = rng.normal(size=(40, 3)).astype(F) if with_normals else None
    T = rng.integers(0, 40, size=(70, 3)).astype(np.int32)
    path = tmp_path / "mesh.obj"
    nr.save_obj(path, V, T, normals=N)
    v, vn, f = [], [], []
    for line in open(path).read().splitlines():
        tag, *rest = line.split()
        if tag == "v":
            v.append([F(x) for x in rest])
        elif tag == "vn":
            vn.append([F(x) for x in rest])
        else:
            assert tag == "f"
            if with_normals:
                pairs = [x.split("//") for x in rest]
                assert all(a == b for a, b in pairs)
                f.append([int(a) - 1 for a, _ in pairs])
            else:
                f.append([int(x) - 1 for x in rest])
    assert np.array_equal(mesh_ref.bits(np.array(v, F)), mesh_ref.bits(V))
    assert np.array_equal(np.array(f, np.int32), T)
    if with_normals:
        assert np.array_equal(mesh_ref.bits(np.array(vn, F)), mesh_ref.bits(N))
    else:
        assert not vn


def test_obj_save_errors_and_exports(tmp_path):
    L = nr.lib()
    z = np.zeros(3, F)
    t = np.zeros(3, np.int32)
    assert L.nr_obj_save(str(tmp_path / "no" / "such" / "dir.obj").encode(), z.ctypes.data, 1, None, t.ctypes.data, 1) == -3
    assert L.nr_obj_save(None, z.ctypes.data, 1, None, t.ctypes.data, 1) == -1
    for name in ("nr_sample_grid", "nr_mesh_grid", "nr_extract_mesh", "nr_obj_save"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    # a NULL context is rejected without touching a device
    one = np.ones(3, F)
    d = np.full(3, 2, np.int32)
    ip = d.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    assert L.nr_sample_grid(None, nr.renderer._fptr(z), nr.renderer._fptr(one), ip, z.ctypes.data, 0, None) == -1
    assert L.nr_abi_version() == 3
