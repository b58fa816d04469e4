"""Reference for the winding-number query (nr_mesh_hierarchy, nr_mesh_winding): a helper, not a
test.

The numpy restatement of the contract in include/neural_render.h, written from that text: np.float64,
one rounding per operation (numpy contracts nothing), the only square root the correctly rounded f32
one.  The sum depends on the tree and on its order, so winding() walks the tree the library exports
(nr.trimesh_hierarchy) -- once for all points, with boolean masks for "open" and "far" where the
kernel has lanes -- and moments() restates the far-field records from the same tree.
tests/test_winding_cpu.py pins this file against np.arctan2 and the exact double sum, so the GPU
comparison is not vacuous.

Also the open and self-intersecting meshes both test files use.
"""
import functools
import math

import numpy as np

import trimesh_ref as R

F = np.float32
D = np.float64
QNAN = R.QNAN
INV_4PI = 0.07957747154594767
TAN_PI_8 = 0.41421356237309503
COEF = [(-1.0) ** k / (2 * k + 1) for k in range(12)]


def dot(u, v):
    """(u.x v.x + u.y v.y) + u.z v.z"""
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def length(u):
    """(double)sqrtf((float)dot(u, u))"""
    with np.errstate(all="ignore"):
        return np.sqrt(np.asarray(dot(u, u)).astype(F)).astype(D)


def half_angle(num, den):
    """The header's h(num, den): atan2 from basic operations; 0 when num == 0 or the quotient is not finite."""
    num, den = np.broadcast_arrays(np.asarray(num, D), np.asarray(den, D))
    with np.errstate(all="ignore"):
        an, ad = np.abs(num), np.abs(den)
        lt = an < ad
        t = np.where(lt, an, ad) / np.where(lt, ad, an)
        big = t > TAN_PI_8
        u = np.where(big, (t - 1.0) / (t + 1.0), t)
        z = u * u
        p = np.full(z.shape, COEF[11])
        for k in range(10, -1, -1):
            p = p * z + COEF[k]
        a = np.where(big, 0.7853981633974483, 0.0) + u * p
        a = np.where(an > ad, 1.5707963267948966 - a, a)
        a = np.where(den < 0.0, 3.141592653589793 - a, a)
        a = np.where(num < 0.0, -a, a)
        return np.where((num == 0.0) | ~np.isfinite(t), 0.0, a)


def solid_angle(p, A, B, C):
    """Omega of triangles (A, B, C) seen from p; broadcastable [..., 3] arrays, promoted to float64."""
    with np.errstate(all="ignore"):
        p, A, B, C = [np.asarray(x).astype(D) for x in (p, A, B, C)]
        a, b, c = A - p, B - p, C - p
        det = ((a[..., 0] * (b[..., 1] * c[..., 2] - b[..., 2] * c[..., 1])
                + a[..., 1] * (b[..., 2] * c[..., 0] - b[..., 0] * c[..., 2]))
               + a[..., 2] * (b[..., 0] * c[..., 1] - b[..., 1] * c[..., 0]))
        la, lb, lc = length(a), length(b), length(c)
        den = (((la * lb) * lc + dot(a, b) * lc) + dot(b, c) * la) + dot(c, a) * lb
        return 2.0 * half_angle(det, den)


def expansion(p, rec):
    """(E, d2) of one node's record rec [16] (float32) at points p [n, 3]."""
    with np.errstate(all="ignore"):
        rec = np.asarray(rec, F).astype(D)
        r = rec[0:3] - np.asarray(p).astype(D)
        d2 = dot(r, r)
        d = np.sqrt(d2.astype(F)).astype(D)
        d3 = d2 * d
        sxx, syy, szz, sxy, sxz, syz = rec[8:14]
        s = np.stack([(sxx * r[..., 0] + sxy * r[..., 1]) + sxz * r[..., 2],
                      (sxy * r[..., 0] + syy * r[..., 1]) + syz * r[..., 2],
                      (sxz * r[..., 0] + syz * r[..., 1]) + szz * r[..., 2]], -1)
        q = dot(r, s)
        tr = (sxx + syy) + szz
        N = np.broadcast_to(rec[4:7], r.shape)
        return dot(N, r) / d3 + (tr / d3 - (3.0 * q) / (d3 * d2)), d2


def links(nodes):
    """words 3 and 7 of every node as int32"""
    w = np.ascontiguousarray(nodes, F).view(np.int32).reshape(-1, 8)
    return w[:, 3].copy(), w[:, 7].copy()


def ranges(nodes):
    """(first, count): every node's positions [first, first + count), leaves and inner nodes alike"""
    w3, w7 = links(nodes)
    nn = len(w3)
    first, count = np.zeros(nn, np.int64), np.zeros(nn, np.int64)
    for i in range(nn - 1, -1, -1):
        if w7[i] <= 0:
            first[i], count[i] = w3[i], -w7[i]
        else:
            first[i], count[i] = first[w3[i]], count[w3[i]] + count[w7[i]]
    return first, count


def moments(V, T, nodes, order):
    """The header's moments [nnodes, 16] (float32), in Python floats (IEEE double, one rounding per
    operation), every sum sequential in position order; also r2 [nnodes], the double R2 was rounded up from."""
    V = np.asarray(V, F).astype(D)
    T = np.asarray(T).reshape(-1, 3)
    first, count = ranges(nodes)
    tri = [[[float(x) for x in V[T[t, c]]] for c in range(3)] for t in order]
    per = []
    for a, b, c in tri:
        u = [b[k] - a[k] for k in range(3)]
        v = [c[k] - a[k] for k in range(3)]
        A = [0.5 * (u[1] * v[2] - u[2] * v[1]), 0.5 * (u[2] * v[0] - u[0] * v[2]), 0.5 * (u[0] * v[1] - u[1] * v[0])]
        area = math.sqrt((A[0] * A[0] + A[1] * A[1]) + A[2] * A[2])
        x = [((a[k] + b[k]) + c[k]) / 3.0 for k in range(3)]
        per.append((A, area, x))
    out = np.zeros((len(first), 16), F)
    r2s = np.zeros(len(first))
    for i in range(len(first)):
        k0, k1 = int(first[i]), int(first[i] + count[i])
        if k1 == k0:
            continue
        sa, sx, mx, N = 0.0, [0.0] * 3, [0.0] * 3, [0.0] * 3
        for A, area, x in per[k0:k1]:
            sa += area
            for k in range(3):
                sx[k] += area * x[k]
                mx[k] += x[k]
                N[k] += A[k]
        cen = [F(sx[k] / sa if sa > 0.0 else mx[k] / float(k1 - k0)) for k in range(3)]
        c = [float(v) for v in cen]
        M = [[0.0] * 3 for _ in range(3)]
        r2 = 0.0
        for pos in range(k0, k1):
            A, _, x = per[pos]
            d = [x[k] - c[k] for k in range(3)]
            for a in range(3):
                for b in range(3):
                    M[a][b] += A[a] * d[b]
            for corner in tri[pos]:
                e = [corner[k] - c[k] for k in range(3)]
                r2 = max(r2, (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        R2 = F(r2)
        if float(R2) < r2:
            R2 = np.nextafter(R2, F(np.inf))
        r2s[i] = r2
        out[i, 0:3] = cen
        out[i, 3] = R2
        out[i, 4:7] = [F(v) for v in N]
        out[i, 8:14] = [F(M[0][0]), F(M[1][1]), F(M[2][2]), F(0.5 * (M[0][1] + M[1][0])), F(0.5 * (M[0][2] + M[2][0])),
                        F(0.5 * (M[1][2] + M[2][1]))]
    return out, r2s


def winding(V, T, X, beta, nodes, order, moments, brute=False, count_evals=False):
    """nr_mesh_winding's `winding` for points X [n, 3] (float32 [n]): one walk of the exported tree for
    all points; `open` and `far` are masks over the points.  beta 0 = 2.0.  With count_evals also the
    number of solid angles and expansions evaluated, as stats.shade_evals counts them."""
    V, T, X = np.asarray(V, F), np.asarray(T).reshape(-1, 3), np.ascontiguousarray(X, F).reshape(-1, 3)
    order = np.asarray(order, np.int64)
    n, ntl = len(X), len(order)
    A, B, C = (V[T[order, k]] for k in range(3))  # corners by position
    live = np.isfinite(X).all(1) & (ntl > 0)
    W = np.zeros(n)
    P = X.astype(D)
    evals = 0

    def add_triangles(sel, k0, k1):
        # W[sel] += Omega of positions k0..k1-1, one after the other
        om = solid_angle(P[sel][:, None, :], A[None, k0:k1], B[None, k0:k1], C[None, k0:k1])
        acc = W[sel]
        for j in range(k1 - k0):
            acc = acc + om[:, j]
        W[sel] = acc

    if brute:
        sel = np.nonzero(live)[0]
        for k0 in range(0, ntl, 64):
            add_triangles(sel, k0, min(k0 + 64, ntl))
        evals = ntl * len(sel)
    elif live.any():
        w3, w7 = links(nodes)
        beta = F(beta) if F(beta) != 0 else F(2.0)
        bb = float(beta) * float(beta)
        resume = np.zeros(n, np.int64)
        stack = [(0, len(w3))]
        while stack:
            node, end = stack.pop()
            is_open = live & (node >= resume)
            sel = np.nonzero(is_open)[0]
            E, d2 = expansion(P[sel], moments[node])
            far = d2 > bb * float(moments[node][3])
            take, need = sel[far], sel[~far]
            W[take] = W[take] + E[far]
            resume[take] = end
            evals += len(take)
            if len(need) == 0:
                continue
            if w7[node] <= 0:
                add_triangles(need, int(w3[node]), int(w3[node] - w7[node]))
                evals += int(-w7[node]) * len(need)
            else:
                stack.append((int(w7[node]), end))       # the right child waits,
                stack.append((int(w3[node]), int(w7[node])))  # the left one is entered first
    with np.errstate(all="ignore"):
        w = np.where(live, (W * INV_4PI).astype(F), QNAN).astype(F)
    return (w, evals) if count_evals else w


def exact(V, T, X):
    """The winding number in plain float64 (np.arctan2, np.linalg.norm), over every triangle of T."""
    V, T, P = np.asarray(V, F).astype(D), np.asarray(T).reshape(-1, 3), np.asarray(X, F).astype(D)
    a, b, c = (V[T[:, k]][None] - P[:, None, :] for k in range(3))
    la, lb, lc = (np.linalg.norm(v, axis=-1) for v in (a, b, c))
    det = np.einsum("ijk,ijk->ij", a, np.cross(b, c))
    den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
    return (2.0 * np.arctan2(det, den)).sum(1) / (4.0 * np.pi)


# ---- the meshes ------------------------------------------------------------------------------------

def open_torus():
    """the torus without the triangles whose centroid has x >= 0.35: a cap cut off"""
    V, T = R.torus()
    keep = V.astype(D)[T].mean(1)[:, 0] < 0.35
    return V, np.ascontiguousarray(T[keep])


def open_cube():
    """the cube without its first face"""
    V, T = R.cube()
    return V, np.ascontiguousarray(T[2:])


def double_cube():
    """the cube twice, the copy moved by (0.3, 0.2, 0.1): it cuts through itself, w = 2 in the overlap"""
    V, T = R.cube()
    V2 = (V + np.array([0.3, 0.2, 0.1], F)).astype(F)
    return np.concatenate([V, V2]), np.concatenate([T, T + len(V)]).astype(np.int32)


# mesh name -> (builder, the trimesh_ref mesh whose points it is queried at)
MESHES = {"tetrahedron": (R.tetrahedron, "tetrahedron"), "cube": (R.cube, "cube"), "torus": (R.torus, "torus"),
          "open_torus": (open_torus, "torus"), "open_cube": (open_cube, "cube"), "double_cube": (double_cube, "cube")}
CLOSED = ("tetrahedron", "cube", "torus")


@functools.lru_cache(maxsize=None)
def mesh(name):
    V, T = MESHES[name][0]()
    V, T = np.array(V, F), np.array(T, np.int32)
    V.setflags(write=False)
    T.setflags(write=False)
    return V, T


def points(name):
    """trimesh_ref's points around the mesh's parent, none of them placed on the surface (read-only)"""
    return R.points(MESHES[name][1], surface=False)


@functools.lru_cache(maxsize=None)
def exact_reference(name):
    w = exact(*mesh(name), points(name))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def tree(name, leaf):
    """nr.trimesh_hierarchy of the mesh: (nodes, order, moments, depth), computed once (read-only)"""
    import cudaneuralrender_amd as nr
    out = nr.trimesh_hierarchy(*mesh(name), leaf=leaf)
    for a in out[:3]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, leaf, beta, brute=False):
    """winding() of points(name) through the library's tree, computed once and shared (read-only)"""
    nodes, order, moments, _ = tree(name, leaf)
    w = winding(*mesh(name), points(name), beta, nodes, order, moments, brute=brute)
    w.setflags(write=False)
    return w
