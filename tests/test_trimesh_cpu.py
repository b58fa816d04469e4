"""The triangle-mesh query without a GPU: tests/trimesh_ref.py (the numpy restatement of the contract
in include/neural_render.h) against an independent float64 implementation, nr_trimesh_normals against
the restatement's table, and nr_obj_load."""
import ctypes
import functools

import numpy as np
import pytest

import cudaneuralrender_amd as nr
from cudaneuralrender_amd import _lib
import trimesh_ref as R

MESHES = ("tetrahedron", "cube", "torus")
NE = 700  # points per mesh of the float64 comparison


# ---- an independent float64 distance: project onto the plane, then clamp to the three segments;
# the sign from the winding number (the solid angles of the triangles seen from the point)

def _seg(p, a, b):
    e = b - a
    t = np.clip(((p - a) * e).sum(-1) / (e * e).sum(-1), 0.0, 1.0)
    return np.linalg.norm(p - (a + t[..., None] * e), axis=-1)


def distance64(V, T, X):
    V, X = np.asarray(V, np.float64), np.asarray(X, np.float64)
    a, b, c = V[T[:, 0]][None], V[T[:, 1]][None], V[T[:, 2]][None]
    p = X[:, None, :]
    n = np.cross(b - a, c - a)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    h = ((p - a) * n).sum(-1)
    proj = p - h[..., None] * n
    inside = np.ones(h.shape, bool)
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(v - u, proj - u) * n).sum(-1) >= 0
    d = np.where(inside, np.abs(h), np.inf)
    for u, v in ((a, b), (b, c), (c, a)):
        d = np.minimum(d, _seg(p, u, v))
    dist = d.min(1)
    # van Oosterom and Strackee: tan(omega / 2) = det(a, b, c) / (|a||b||c| + (a.b)|c| + (a.c)|b| + (b.c)|a|)
    ra, rb, rc = a - p, b - p, c - p
    la, lb, lc = (np.linalg.norm(r, axis=-1) for r in (ra, rb, rc))
    num = (ra * np.cross(rb, rc)).sum(-1)
    den = la * lb * lc + (ra * rb).sum(-1) * lc + (ra * rc).sum(-1) * lb + (rb * rc).sum(-1) * la
    wind = (2.0 * np.arctan2(num, den)).sum(1) / (4.0 * np.pi)
    return np.where(np.abs(wind) > 0.5, -dist, dist)


@functools.lru_cache(maxsize=None)
def both(name):
    V, T = R.mesh(name)
    X = R.points(name, NE, 23, False)
    return X, R.distance(V, T, X), distance64(V, T, X)


# the largest |d32 - d64| measured over the three point sets, and the bound: 4 x that
MEASURED_MAX = 2.28e-6
BOUND = 4 * MEASURED_MAX


@pytest.mark.parametrize("name", MESHES)
def test_restatement_against_float64(name):
    """trimesh_ref (f32 chains of the header) against distance64 (float64, another method).
    Measured on the CPU: the largest | |sdf32| - |d64| | over the 3 x 700 points is 2.28e-6 (the
    tetrahedron's far point, |d| = 89.8: a third of an f32 ulp of that distance; 8.8e-8 over the points
    nearer than 5), so the bound is 4 x 2.28e-6 = 9.12e-6.  Signs agree wherever |d64| exceeds the
    bound; at most 2 % of the points may lie within it (measured: 1 of the cube's 700, none of the
    others')."""
    X, out, d64 = both(name)
    err = np.abs(np.abs(out["sdf"].astype(np.float64)) - np.abs(d64))
    print(f"{name}: max |d32 - d64| = {err.max():.3e}, within the bound: {(np.abs(d64) <= BOUND).mean():.4f}")
    assert err.max() <= BOUND
    far = np.abs(d64) > BOUND
    assert (~far).mean() <= 0.02
    assert np.array_equal(out["sdf"][far] < 0, d64[far] < 0)
    assert (d64 < 0).mean() > 0.02, "the point set has to reach the inside"
    # the closest point lies at the distance, on its triangle's feature
    V, T = R.mesh(name)
    assert np.abs(np.linalg.norm(X.astype(np.float64) - out["closest"], axis=1) - np.abs(d64)).max() <= BOUND
    assert set(np.unique(out["feature"])) == set(range(7)), "every feature kind has to be reached"
    assert ((out["tri"] >= 0) & (out["tri"] < len(T))).all()


def _ulps(a, b):
    a, b = (np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    a, b = np.where(a < 0, -(a & 0x7fffffff), a), np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


@pytest.mark.parametrize("name", MESHES)
def test_normals_against_restatement(name):
    V, T = R.mesh(name)
    ref, ref_closed = R.normals(V, T)
    table, closed = nr.trimesh_normals(V, T)
    assert table.shape == (len(T), 7, 3) and table.dtype == np.float32
    assert _ulps(table, ref).max() <= 1
    assert closed is True and ref_closed is True
    # the face entries are unit vectors; both triangles of an edge hold the same bits for it
    assert np.abs(np.linalg.norm(table[:, 0].astype(np.float64), axis=1) - 1).max() < 1e-6
    seen = {}
    for t in range(len(T)):
        for s in range(3):
            i, j = int(T[t, s]), int(T[t, (s + 1) % 3])
            seen.setdefault((min(i, j), max(i, j)), []).append(R.bits(table[t, 1 + s]).tolist())
    assert all(len(v) == 2 and v[0] == v[1] for v in seen.values())
    # vertex entries point outward: towards the side the incident faces look at
    for t in range(len(T)):
        for s in range(3):
            assert (table[t, 4 + s].astype(np.float64) * table[t, 0]).sum() > 0


def test_closed_flag():
    V, T = R.cube()
    assert nr.trimesh_normals(V, T)[1] is True
    assert nr.trimesh_normals(V, T[1:])[1] is False
    flipped = T.copy()
    flipped[5] = flipped[5][[0, 2, 1]]
    assert nr.trimesh_normals(V, flipped)[1] is False
    assert R.normals(V, T[1:])[1] is False and R.normals(V, flipped)[1] is False
    # a zero-area triangle: face entry 0, and it adds +0 to its neighbours' entries
    V2, T2 = R.degenerate_torus()
    t2, c2 = nr.trimesh_normals(V2, T2)
    t0, _ = nr.trimesh_normals(*R.torus())
    assert c2 is False and not t2[-3:, 0].any()
    assert np.array_equal(t2[:-3], t0)


def test_normals_invalid():
    L = nr.lib()
    V, T = R.cube()
    table = np.zeros((len(T), 7, 3), np.float32)
    closed = ctypes.c_int(0)
    args = lambda V_, nv, T_, nt, tab=table: (V_.ctypes.data if V_ is not None else None, nv,
                                               T_.ctypes.data if T_ is not None else None, nt,
                                               tab.ctypes.data if tab is not None else None, ctypes.byref(closed))
    bad = T.copy()
    bad[3, 1] = 8
    neg = T.copy()
    neg[0, 0] = -1
    for a in (args(None, 8, T, 12), args(V, 8, None, 12), args(V, 0, T, 12), args(V, 8, T, 0), args(V, 8, bad, 12),
              args(V, 8, neg, 12), args(V, 8, T, (1 << 24) + 1)):
        assert L.nr_trimesh_normals(*a) == -1
    assert L.nr_trimesh_normals(V.ctypes.data, 8, T.ctypes.data, 12, None, None) == -1
    assert L.nr_trimesh_normals(V.ctypes.data, 8, T.ctypes.data, 12, None, ctypes.byref(closed)) == 0 and closed.value == 1


# ---- nr_obj_load

@pytest.mark.parametrize("with_normals", [False, True])
def test_obj_round_trip(tmp_path, with_normals):
    V, T = R.torus()
    rng = np.random.default_rng(3)
    # values %.9g has to carry: denormals, large and tiny magnitudes, negative zero
    V = V.copy()
    V[:6, 0] = np.array([1e-42, -0.0, 3.4e38, -1.17549435e-38, 1 / 3, 16777217.0], np.float32)
    N = rng.normal(size=V.shape).astype(np.float32) if with_normals else None
    path = tmp_path / "m.obj"
    nr.save_obj(path, V, T, N)
    V2, T2 = nr.load_obj(path)
    assert V2.dtype == np.float32 and T2.dtype == np.int32
    assert np.array_equal(R.bits(V2), R.bits(V)) and np.array_equal(T2, T)


HAND = """# a comment
mtllib none.mtl
o thing
v 0 0 0
v 1 0 0 1.0
v 1 1 0
  v 0 1 0
vt 0.5 0.5
vn 0 0 1
f 1/1/1 2/1/1 3/1/1 4/1/1
v 0.5 0.5 1e0
f -1 -5 -4
f 1//1 -1//1 4//1
g grp
s off
f 2/1 3/1 5/1\r
f 1 2 3 4 5
"""


def test_obj_hand_written(tmp_path):
    path = tmp_path / "hand.obj"
    path.write_bytes(HAND.encode())
    V, T = nr.load_obj(path)
    assert np.array_equal(V, np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]], np.float32))
    assert T.tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1], [0, 4, 3], [1, 2, 4], [0, 1, 2], [0, 2, 3], [0, 3, 4]]
    # no trailing newline, and a file of vertices only
    path.write_bytes(b"v 1 2 3\nv 4 5 6\nv 7 8 9\nf 1 2 3")
    V, T = nr.load_obj(path)
    assert V.shape == (3, 3) and T.tolist() == [[0, 1, 2]]
    path.write_bytes(b"v 1 2 3\n")
    V, T = nr.load_obj(path)
    assert V.shape == (1, 3) and T.shape == (0, 3)


@pytest.mark.parametrize("text, code", [
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", -4),      # an index past the last vertex
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 0\n", -4),      # index 0
    ("v 0 0 0\nv 1 0 0\nf -1 -2 -3\nv 0 1 0\n", -4),   # a relative index before the first vertex
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n", -4),        # a face of two corners
    ("v 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n", -4),        # a vertex of two numbers
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 x 3\n", -4),      # a corner that is no number
])
def test_obj_format_errors(tmp_path, text, code):
    path = tmp_path / "bad.obj"
    path.write_text(text)
    with pytest.raises(nr.NRError) as e:
        nr.load_obj(path)
    assert e.value.code == code


def test_obj_io_error_and_null(tmp_path):
    with pytest.raises(nr.NRError) as e:
        nr.load_obj(tmp_path / "missing.obj")
    assert e.value.code == -3
    with pytest.raises(nr.NRError) as e:
        nr.load_obj(tmp_path)  # a directory
    assert e.value.code == -3
    L = nr.lib()
    assert L.nr_obj_load(None, None, None, None, None) == -1
    assert sorted(s for s in _lib.EXPORTS if "trimesh" in s or s == "nr_obj_load") == [
        "nr_obj_load", "nr_trimesh_create", "nr_trimesh_destroy", "nr_trimesh_distance", "nr_trimesh_info",
        "nr_trimesh_normals"]
