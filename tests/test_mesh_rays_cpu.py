"""The mesh ray query without a GPU: tests/mesh_ray_ref.py (the numpy restatement of the ray contract
in include/neural_render.h) against an independent float64 Moeller-Trumbore, the watertightness of the
contract's shear form, the walk's skip rule against brute force, and the host-only argument checks."""
import functools

import numpy as np
import pytest

import cudaneuralrender_amd as nr
from cudaneuralrender_amd import _lib
import mesh_ray_ref as M
import trimesh_ref as R

MESHES = ("tetrahedron", "cube", "torus")
F = np.float32
NE = 2000  # rays per mesh of the float64 comparison
MARGIN = 1e-4


# ---- an independent Moeller-Trumbore (another method: no shear, no edge functions) -------------------

def moller_trumbore(O, D, a, b, c, dtype):
    """(u, v, w, t) [n, m] of rays against triangles in `dtype`: the weights of b, c, a and the depth."""
    O, D, a, b, c = (np.asarray(x, dtype) for x in (O, D, a, b, c))
    with np.errstate(all="ignore"):
        e1, e2 = (b - a)[None], (c - a)[None]
        p = np.cross(D[:, None, :], e2)
        det = (e1 * p).sum(-1)
        s = O[:, None, :] - a[None]
        u = (s * p).sum(-1) / det
        q = np.cross(s, e1)
        v = (D[:, None, :] * q).sum(-1) / det
        t = (e2 * q).sum(-1) / det
        return u, v, (1 - u) - v, t


@functools.lru_cache(maxsize=None)
def both(name):
    V, T = R.mesh(name)
    rng = np.random.default_rng(31)
    O = rng.uniform(-1.5, 1.5, (NE, 3)).astype(F)
    lo, hi = V.min(0).astype(np.float64), V.max(0).astype(np.float64)
    D = (rng.uniform(lo, hi, (NE, 3)) - O).astype(F)
    a, b, c = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    return M.pairs(O, D, a, b, c, 0.0, np.inf), moller_trumbore(O, D, a, b, c, np.float64)


# the largest |t32 - t64| measured over the clear hits of the three ray sets, and the bound: 4 x that
MEASURED_MAX = 1.18e-6
BOUND = 4 * MEASURED_MAX


@pytest.mark.parametrize("name", MESHES)
def test_restatement_against_float64(name):
    """mesh_ray_ref.pairs (the f32 chains of the header) against a float64 Moeller-Trumbore on 2,000
    rays per mesh, origins uniform in +-1.5, aimed at uniform points of the mesh's bound.  Every
    (ray, triangle) pair whose f64 barycentrics and depth are inside by 1e-4 is a hit, every pair
    outside by 1e-4 a miss; the pairs in between are left out and may be at most 1 % of the f64 hits
    (measured: 4, 0 and 6 of 1,999, 3,970 and 3,583).  Measured on the CPU: the largest |t32 - t64|
    over the clear hits is 4.2e-7 (tetrahedron), 4.0e-7 (cube) and 1.18e-6 (torus), so the bound is
    4 x 1.18e-6 = 4.72e-6."""
    r, (u, v, w, t) = both(name)
    with np.errstate(all="ignore"):
        inner = np.minimum(np.minimum(u, v), np.minimum(w, t))
    clear_hit = inner > MARGIN
    clear_miss = ~(inner >= -MARGIN)  # (a NaN of a parallel ray is a miss)
    between = ~clear_hit & ~clear_miss
    err = np.abs(r["t"].astype(np.float64) - t)[clear_hit]
    print(f"{name}: f64 hits {clear_hit.sum()}, in between {between.sum()}, max |t32 - t64| = {err.max():.3e}")
    assert clear_hit.sum() > 1000
    assert r["hit"][clear_hit].all()
    assert not r["hit"][clear_miss].any()
    assert between.sum() <= 0.01 * clear_hit.sum()
    assert err.max() <= BOUND
    # the barycentrics are the weights of a, b, c in that order (a check of the order, not of the rounding:
    # a permutation is off by the triangle's size, 0.1 and more)
    with np.errstate(all="ignore"):
        b32 = np.stack([r["U"] / r["det"], r["V"] / r["det"], r["W"] / r["det"]], -1)[clear_hit]
    assert np.abs(b32 - np.stack([w, u, v], -1)[clear_hit]).max() <= 1e-3


# ---- watertight -------------------------------------------------------------------------------------

def _mt32_hits(name, moved):
    """The negative control: an f32 Moeller-Trumbore on the watertight rays; True where anything is hit."""
    V, T = R.mesh(name)
    O, D = M.watertight_rays(name, moved)
    u, v, w, t = moller_trumbore(O, D, V[T[:, 0]], V[T[:, 1]], V[T[:, 2]], F)
    assert u.dtype == F
    return ((u >= 0) & (v >= 0) & (w >= 0) & (t >= 0)).any(1)


@pytest.mark.parametrize("moved", (False, True))
@pytest.mark.parametrize("name", MESHES)
def test_watertight(name, moved):
    """From a point strictly inside a closed mesh, the rays at every vertex, every f32 edge midpoint
    (of every triangle) and every face centroid all hit: 20, 56 and 7,380 rays per origin.  An f32
    Moeller-Trumbore hits 18, 47-56 and 7,020-7,021 of them, so the test fails for a contract that is
    not watertight; it is kept as the negative control and has to leak on the torus."""
    V, T = R.mesh(name)
    assert R.normals(V, T)[1], "closed"
    O, D = M.watertight_rays(name, moved)
    assert len(O) == {"tetrahedron": 20, "cube": 56, "torus": 7380}[name]
    out, _ = M.trace(V, T, O, D)
    leaks = _mt32_hits(name, moved)
    print(f"{name}: shear form {int((out['status'] == M.HIT).sum())} / {len(O)}, f32 Moeller-Trumbore {int(leaks.sum())}")
    assert (out["status"] == M.HIT).all()
    # (a target on the silhouette may be passed by: the hit is then the surface behind it)
    assert (out["t"] > 0).all() and (out["t"] < 1.001).mean() > 0.99
    if name == "torus":
        assert leaks.sum() < len(O), "the negative control has to leak"


# ---- the walk ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hierarchy(name, leaf):
    V, T = M._mesh(name)
    nodes, order, _, _ = nr.trimesh_hierarchy(V, T, leaf)
    return nodes, order


WALKS = [("tetrahedron", 8), ("cube", 1), ("torus", 8), ("torus", 3), ("torus", 1), ("degenerate_torus", 8)]


@pytest.mark.parametrize("window", (0, 1))
@pytest.mark.parametrize("name,leaf", WALKS)
def test_walk_equals_brute_force(name, leaf, window):
    """The skip rule of the header's step 5, every ray on its own (the rule at its sharpest), gives
    brute force's outputs bit for bit on the ray sets of mesh_ray_ref.rays: origins up to |o| = 100,
    zero direction components, negative directions, origins that share coordinates with a vertex or
    lie on the surface (tmin = 0), a window that cuts first hits off, dead rays.  No counter-example
    was found with the pad as the header words it."""
    V, T = M._mesh(name)
    O, D = M.rays(name)
    nodes, order = hierarchy(name, leaf)
    tmin, tmax = M.WINDOWS[window]
    ref, counts = M.reference(name, window)
    out, leaves = M.walk(nodes, order, V, T, O, D, tmin, tmax)
    for k in M.KEYS:
        assert np.array_equal(M.bits(out[k]), M.bits(ref[k])), k
    nleaves = int((nodes.view(np.int32)[:, 7] <= 0).sum())
    dead = M.dead(O, D)
    assert dead.sum() >= 10 and (ref["status"][dead] == M.MISS).all() and (leaves[dead] == 0).all()
    hits = int((ref["status"] == M.HIT).sum())
    print(f"{name} leaf {leaf} window {window}: {hits} hits, leaves entered {leaves.sum()} of {nleaves * counts['live_rays']}")
    assert 100 < hits < counts["live_rays"]
    if name != "tetrahedron" and nleaves > 1:
        assert leaves.sum() < nleaves * counts["live_rays"] // 2, "the rule has to prune"
    if name == "degenerate_torus":
        assert counts["live_tris"] == len(T) - 3 and (ref["tri"] < len(T) - 3).all()
    if window == 1:
        full = M.reference(name, 0)[0]
        cut = (full["status"] == M.HIT) & ((ref["status"] == M.MISS) | (ref["t"] != full["t"]))
        assert cut.sum() > 50, "the window has to cut first hits off"
        t = ref["t"][ref["status"] == M.HIT]
        assert (t >= F(tmin)).all() and (t <= F(tmax)).all()


def test_walk_smooth_normals():
    V, T = R.torus()
    O, D = M.rays("torus")
    nodes, order = hierarchy("torus", 8)
    ref, _ = M.reference("torus", 0, True)
    flat, _ = M.reference("torus", 0, False)
    out, _ = M.walk(nodes, order, V, T, O, D, smooth=True)
    for k in M.KEYS:
        assert np.array_equal(M.bits(out[k]), M.bits(ref[k])), k
    hit = ref["status"] == M.HIT
    assert np.abs(np.linalg.norm(ref["normal"][hit], axis=1) - 1).max() < 1e-6
    assert (ref["normal"][hit] != flat["normal"][hit]).any(1).mean() > 0.9
    assert ((ref["normal"][hit] * flat["normal"][hit]).sum(1) > 0.5).all()


@pytest.mark.parametrize("window", (0, 1))
@pytest.mark.parametrize("name,leaf", [("cube", 1), ("torus", 8)])
def test_any_hit_status(name, leaf, window):
    """NR_MESH_RAY_ANY's status is closest hit's, with the same window."""
    V, T = M._mesh(name)
    O, D = M.rays(name)
    nodes, order = hierarchy(name, leaf)
    ref, _ = M.reference(name, window)
    out, leaves = M.walk(nodes, order, V, T, O, D, *M.WINDOWS[window], any_hit=True)
    assert np.array_equal(out["status"], ref["status"])
    closest = M.walk(nodes, order, V, T, O, D, *M.WINDOWS[window])[1]
    assert leaves.sum() <= closest.sum()


def test_colours():
    """The restated colours on known normals: a normal facing the ray is white, one facing away black;
    the matcap texel is the one the eye-space normal points at."""
    import designed_nets
    n = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 1, 0], [-1, 0, 0]], F)
    d = np.array([[0, 0, -1]] * 5, F)
    st = np.array([2, 2, 2, 0, 2], np.int32)
    assert list(M.facing(n, d, st)) == [0xffffffff, 0xff000000, 0xff000000, 0, 0xff000000]
    tex = designed_nets.coded_matcap(5, 9)
    eye = np.eye(4, dtype=F)
    rows, cols = designed_nets.decode_matcap(M.matcap(n, st, eye, tex))
    assert list(zip(rows, cols)) == [(2, 4), (2, 4), (2, 8), (0, 0), (2, 0)]
    assert M.matcap(n, st, eye, tex)[3] == 0


# ---- host-only argument checks ----------------------------------------------------------------------

def test_null_mesh():
    L = _lib.lib()
    z = np.zeros((1, 3), F)
    px = np.zeros(1, np.uint32)
    assert L.nr_mesh_trace_rays(None, z.ctypes.data, z.ctypes.data, 1, 0.0, 1.0, None, None, None, None, None, None, 0, 0, None) == -1
    assert L.nr_mesh_gbuffer(None, 1, 1, None, None, None, None, None, None, 0, 0, None) == -1
    assert L.nr_mesh_render(None, px.ctypes.data, 1, 1, 0, 0, None) == -1
    assert b"mesh is NULL" in L.nr_last_error(None)
    assert (_lib.NR_TRIMESH_BRUTE, _lib.NR_MESH_RAY_ANY, _lib.NR_MESH_RAY_SMOOTH) == (1, 2, 4)
    for sym in ("nr_mesh_trace_rays", "nr_mesh_gbuffer", "nr_mesh_render"):
        assert sym in _lib.EXPORTS
