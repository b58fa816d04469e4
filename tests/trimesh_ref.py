"""Reference for the triangle-mesh distance query (nr_trimesh_normals, nr_trimesh_distance): a helper,
not a test.

The numpy restatement of the contract in include/neural_render.h, written from that text: brute force
over all triangles with the header's chains (np.float32, one rounding per operation, an exact f32
fmaf), the winner as the minimum of (d2, triangle index), the sign from the pseudonormal table, which
is built here in float64 the way the header words it.  tests/test_trimesh_cpu.py pins this file
against an independent float64 implementation, so the GPU comparison is not vacuous.

Also the meshes and the point sets both test files use.
"""
import functools
import math

import numpy as np

F = np.float32
QNAN = np.uint32(0x7fc00000).view(F)


def fmaf(a, b, c):
    """Correctly rounded f32 a * b + c, elementwise: grad_ref.fmaf's rounding to odd in f64 (the
    product of two f32 is exact there, TwoSum gives the sum's error), with a non-finite sum passed on."""
    with np.errstate(all="ignore"):
        a, b, c = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64)
        p = a * b
        s = np.asarray(p + c)
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        fix = (e != 0) & ((np.ascontiguousarray(s).view(np.int64) & 1) == 0) & np.isfinite(s)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(F)


def dot(u, v):
    """fmaf(u.z, v.z, fmaf(u.y, v.y, u.x * v.x))"""
    return fmaf(u[..., 2], v[..., 2], fmaf(u[..., 1], v[..., 1], (u[..., 0] * v[..., 0]).astype(F)))


def vfma(e, t, b):
    return np.stack([fmaf(e[..., k], t, b[..., k]) for k in range(3)], -1)


def closest(p, a, b, c):
    """Step 1 of the header for broadcastable f32 [..., 3] arrays: (q [..., 3], feature [...])."""
    with np.errstate(all="ignore"):
        p, a, b, c = np.broadcast_arrays(*[np.asarray(x, F) for x in (p, a, b, c)])
        ab, ac, bc = b - a, c - a, c - b
        ap, bp, cp = p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        regions = [((d1 <= 0) & (d2 <= 0), 4), ((d3 >= 0) & (d4 <= d3), 5), ((vc <= 0) & (d1 >= 0) & (d3 <= 0), 1),
                   ((d6 >= 0) & (d5 <= d6), 6), ((vb <= 0) & (d2 >= 0) & (d6 <= 0), 3),
                   ((va <= 0) & (e43 >= 0) & (e56 >= 0), 2)]
        feature = np.select([r for r, _ in regions], [f for _, f in regions], 0).astype(np.int32)
        den = (va + vb) + vc
        q_face = vfma(ac, vc / den, vfma(ab, vb / den, a))
        q_ab = vfma(ab, d1 / (d1 - d3), a)
        q_ca = vfma(ac, d2 / (d2 - d6), a)
        q_bc = vfma(bc, e43 / (e43 + e56), b)
        f3 = feature[..., None]
        q = np.select([f3 == 4, f3 == 5, f3 == 6, f3 == 1, f3 == 3, f3 == 2], [a, b, c, q_ab, q_ca, q_bc], q_face)
        assert q.dtype == F
        return q, feature


def normals(V, T):
    """The pseudonormal table [nt, 7, 3] (float32, rounded once from float64) and `closed`."""
    V = np.asarray(V, F).astype(np.float64)
    T = np.asarray(T).reshape(-1, 3)
    nt = len(T)

    def cross(u, v):
        return np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])

    def length(u):
        return math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])

    fn = np.zeros((nt, 3))
    for t, (i, j, k) in enumerate(T):
        n = cross(V[j] - V[i], V[k] - V[i])
        l = length(n)
        if l > 0 and math.isfinite(l):
            fn[t] = n / l
    table = np.zeros((nt, 7, 3))
    table[:, 0] = fn
    uses = {}
    for t in range(nt):
        for s in range(3):
            i, j = int(T[t, s]), int(T[t, (s + 1) % 3])
            uses.setdefault((min(i, j), max(i, j)), []).append((t, s, i < j))
    closed = True
    for (i, j), lst in uses.items():
        acc = np.zeros(3)
        for t, s, _ in lst:  # ascending (triangle, slot): the order they were appended in
            acc = acc + fn[t]
        for t, s, _ in lst:
            table[t, 1 + s] = acc
        if len(lst) != 2 or lst[0][2] == lst[1][2] or i == j:
            closed = False
    corners = {}
    for t in range(nt):
        for s in range(3):
            corners.setdefault(int(T[t, s]), []).append((t, s))
    for v, lst in corners.items():
        acc = np.zeros(3)
        for t, s in lst:
            if not fn[t].any():
                continue
            o = V[T[t, s]]
            u, w = V[T[t, (s + 1) % 3]] - o, V[T[t, (s + 2) % 3]] - o
            ang = math.atan2(length(cross(u, w)), u[0] * w[0] + u[1] * w[1] + u[2] * w[2])
            acc = acc + ang * fn[t]
        for t, s in lst:
            table[t, 4 + s] = acc
    return table.astype(F), closed


def distance(V, T, X, table=None, chunk=256):
    """nr_trimesh_distance's outputs for points X [n, 3]: {"sdf", "closest", "tri", "feature"}, brute force."""
    V, T, X = np.asarray(V, F), np.asarray(T).reshape(-1, 3), np.ascontiguousarray(X, F).reshape(-1, 3)
    if table is None:
        table = normals(V, T)[0]
    a, b, c = V[T[:, 0]][None], V[T[:, 1]][None], V[T[:, 2]][None]
    flat = ~table[:, 0].any(1)  # zero-area triangles: d2 = NaN by definition
    n = len(X)
    out = {"sdf": np.full(n, QNAN, F), "closest": np.full((n, 3), QNAN, F), "tri": np.full(n, -1, np.int32),
           "feature": np.full(n, -1, np.int32)}
    with np.errstate(all="ignore"):
        for s in range(0, n, chunk):
            p = X[s:s + chunk]
            q, _ = closest(p[:, None, :], a, b, c)
            d = p[:, None, :] - q
            d2 = dot(d, d)
            d2[:, flat] = np.nan
            valid = ~np.isnan(d2)
            key = np.where(valid, d2, np.inf)
            win = np.argmax(valid & (key == key.min(1)[:, None]), 1)
            ok = np.isfinite(p).all(1) & valid.any(1)
            qw, fw = closest(p, a[0][win], b[0][win], c[0][win])
            dw = p - qw
            dist = np.sqrt(dot(dw, dw)).astype(F)
            sgn = dot(dw, table[win, fw])
            sdf = np.where(sgn < 0, -dist, dist).astype(F)
            sl = slice(s, s + len(p))
            out["sdf"][sl] = np.where(ok, sdf, QNAN)
            out["closest"][sl] = np.where(ok[:, None], qw, QNAN)
            out["tri"][sl] = np.where(ok, win, -1)
            out["feature"][sl] = np.where(ok, fw, -1)
    return out


KEYS = ("sdf", "closest", "tri", "feature")


def bits(a):
    """f32 values are compared on their uint32 views"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- the test meshes (outward winding: (b - a) x (c - a) points out) ----------------------------

def tetrahedron():
    V = np.array([[0.1, 0.05, -0.2], [0.9, -0.1, 0.1], [0.2, 0.8, 0.05], [0.3, 0.2, 0.7]], F)
    T = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32)
    return V, T


def cube():
    V = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)], F) * F(0.8) + F(0.05)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    T = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)
    return V.astype(F), T


@functools.lru_cache(maxsize=None)
def torus():
    """A torus (R = 0.6, r = 0.25, axis z) meshed by mesh_ref from analytic values on a 12^3 lattice."""
    import mesh_ref
    origin, step, dims = (-1.1, -1.1, -0.8), (0.2, 0.2, 1.6 / 11), (12, 12, 12)
    P = mesh_ref.lattice(origin, step, dims).astype(np.float64)
    sdf = np.sqrt((np.sqrt(P[:, 0] ** 2 + P[:, 1] ** 2) - 0.6) ** 2 + P[:, 2] ** 2) - 0.25
    V, T, _, _ = mesh_ref.mesh(sdf.astype(F).reshape(12, 12, 12), origin, step)
    V.setflags(write=False)
    T.setflags(write=False)
    return V, T


def mesh(name):
    return {"tetrahedron": tetrahedron, "cube": cube, "torus": torus}[name]()


def degenerate_torus():
    """The torus with three zero-area triangles appended: (i, i, j) and (i, j, j) on an edge (i, j) of
    the mesh, and (i, m, j) with a new vertex m that is exactly the midpoint of such an edge."""
    V, T = torus()
    V64 = V.astype(np.float64)
    for t in range(len(T)):
        i, j = int(T[t, 0]), int(T[t, 1])
        m = ((V64[i] + V64[j]) / 2)
        if (m.astype(F).astype(np.float64) == m).all() and (m != V64[i]).all():
            break
    else:
        raise AssertionError("no edge of the torus has an f32 midpoint")
    V2 = np.concatenate([V, m.astype(F)[None]])
    T2 = np.concatenate([T, np.array([[i, i, j], [i, j, j], [i, len(V), j]], np.int32)])
    return V2, T2


# ---- the point set of the GPU tests ---------------------------------------------------------------

NP = 1063  # 16 full chunks of 64 and a tail of 39


@functools.lru_cache(maxsize=None)
def points(name, n=NP, seed=11, surface=True):
    """n points around mesh `name`: every vertex (the first 256 at most), edge midpoints, face
    centroids (these three only with surface=True), points pushed +-0.05 along vertex and edge
    pseudonormals, one far point, and uniform points in the bound scaled 1.5 about its centre for
    the rest."""
    V, T = mesh(name)
    table, _ = normals(V, T)
    rng = np.random.default_rng(seed)
    A, B, C = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
    tsel = rng.permutation(len(T))[:48]
    unit = lambda v: v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-30)
    special = [V[:256], ((A[tsel] + B[tsel]) * F(0.5)), ((A[tsel] + B[tsel] + C[tsel]) / F(3))] if surface else []
    for sgn in (0.05, -0.05):
        special.append(A[tsel] + sgn * unit(table[tsel, 4].astype(np.float64)))
        special.append((A[tsel] + B[tsel]) * 0.5 + sgn * unit(table[tsel, 1].astype(np.float64)))
    special.append(np.array([[37.5, -81.25, 12.0]]))
    special = np.concatenate([np.asarray(s, np.float64) for s in special]).astype(F)
    assert len(special) <= n - 300, len(special)
    lo, hi = V.min(0).astype(np.float64), V.max(0).astype(np.float64)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 1.5
    uni = rng.uniform(mid - half, mid + half, (n - len(special), 3)).astype(F)
    X = np.ascontiguousarray(rng.permutation(np.concatenate([special, uni])))
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def reference(name, n=NP):
    """distance() of points(name), computed once and shared (read-only)."""
    V, T = mesh(name)
    out = distance(V, T, points(name, n))
    for a in out.values():
        a.setflags(write=False)
    return out
