"""Reference for a device-built triangle mesh (nr_mesh_create_device): a helper, not a test.

The numpy restatement of "the contract of a device-built mesh" in include/neural_render.h, written
from that text: np.float64 from the float32 coordinates, one rounding per operation (numpy contracts
nothing), the only square root the correctly rounded f32 one, every sum sequential in the order the
text names.  build() returns what nr_mesh_download returns for such a mesh, to the bit.
tests/test_trimesh_device_cpu.py pins this file against the host build (tree shape, boxes, table
bound, signs, winding), so the GPU comparison is not vacuous.
"""
import functools
import math

import numpy as np

import sample_ref as SR
import trimesh_ref as R
import winding_ref as WR

F = np.float32
D = np.float64
DEAD_KEY = 1 << 30
SLACK_SHIFT = 18
AREA_BLOCK = 256


def cross(u, v):
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], -1)


def bound(V):
    """(lo, hi, maxabs) of the vertices: exact minima and maxima, -0 below +0"""
    b = np.ascontiguousarray(V, F).view(np.uint32).astype(np.int64)
    enc = np.where(b >> 31, 0xffffffff - b, b | 0x80000000)
    dec = lambda e: np.where(e >> 31, e ^ 0x80000000, 0xffffffff - e).astype(np.uint32).view(F)
    return dec(enc.min(0)), dec(enc.max(0)), float(np.abs(np.asarray(V, F)).max())


def slack_of(lo, hi, maxabs):
    extent = max(float(hi[a]) - float(lo[a]) for a in range(3))
    return math.ldexp(maxabs + extent, -SLACK_SHIFT)


def face_normals(V, T):
    """(fn [nt, 3] float64, live [nt]): rule 2's face entries before the rounding to f32"""
    V64 = np.asarray(V, F).astype(D)
    a, b, c = (V64[T[:, k]] for k in range(3))
    n = cross(b - a, c - a)
    live = n.any(1) & np.isfinite(n).all(1)
    with np.errstate(all="ignore"):
        s = np.abs(n).max(1)
        m = n / s[:, None]
        fn = m / WR.length(m)[:, None]
    return np.where(live[:, None], fn, 0.0), live


def table_of(V, T, fn, live):
    """(table [nt, 7, 3] float32, closed)"""
    V64 = np.asarray(V, F).astype(D)
    nt = len(T)
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
        for t, s, _ in lst:  # ascending (triangle, slot)
            acc = acc + fn[t]
        for t, s, _ in lst:
            table[t, 1 + s] = acc
        if len(lst) != 2 or lst[0][2] == lst[1][2] or i == j:
            closed = False
    # the angle at every corner: h(len(u x v), dot(u, v))
    ang = np.zeros((nt, 3))
    for s in range(3):
        o = V64[T[:, s]]
        u, w = V64[T[:, (s + 1) % 3]] - o, V64[T[:, (s + 2) % 3]] - o
        ang[:, s] = WR.half_angle(WR.length(cross(u, w)), WR.dot(u, w))
    corners = {}
    for t in range(nt):
        for s in range(3):
            corners.setdefault(int(T[t, s]), []).append((t, s))
    for v, lst in corners.items():
        acc = np.zeros(3)
        for t, s in lst:  # ascending (triangle, corner)
            if live[t]:
                acc = acc + ang[t, s] * fn[t]
        for t, s in lst:
            table[t, 4 + s] = acc
    return table.astype(F), closed


def order_of(V, T, live, lo, hi):
    Vf = np.asarray(V, F)
    a, b, c = (Vf[T[:, k]] for k in range(3))
    cen = (((a + b).astype(F) + c).astype(F) / F(3.0)).astype(F)
    keys = SR.morton_keys(cen, lo, hi).astype(np.int64)
    keys[~live] = DEAD_KEY
    return np.argsort(keys, kind="stable")[:int(live.sum())].astype(np.int32)


def shape(ntl, leaf):
    """(w3, w7, first, count, depth) of Builder::build's tree over ntl positions, in preorder"""
    w3, w7, first, count = [], [], [], []
    depth = 0
    todo = [(0, ntl, -1, 1, False)]
    while todo:
        f, n, parent, level, right = todo.pop()
        me = len(w3)
        if parent >= 0:
            (w7 if right else w3)[parent] = me
        first.append(f)
        count.append(n)
        depth = max(depth, level)
        if n <= leaf:
            w3.append(f)
            w7.append(-n)
            continue
        w3.append(0)
        w7.append(0)
        half = (n + 1) // 2
        todo.append((f + half, n - half, me, level + 1, True))
        todo.append((f, half, me, level + 1, False))
    return (np.array(w3, np.int32), np.array(w7, np.int32), np.array(first, np.int64), np.array(count, np.int64), depth)


def round_outward(x, up):
    """float64 x to float32: to nearest, then one ulp outward where that lies on the wrong side"""
    with np.errstate(all="ignore"):
        f = x.astype(F)
        if up:
            return np.where(f.astype(D) < x, np.nextafter(f, F(np.inf)), f).astype(F)
        return np.where(f.astype(D) > x, np.nextafter(f, F(-np.inf)), f).astype(F)


def area_table(area):
    """(thresholds [ntl] uint32, L) from |A_p| by rule 6"""
    ntl = len(area)
    if ntl == 0:
        return np.zeros(0, np.uint32), -1
    nblk = (ntl + AREA_BLOCK - 1) // AREA_BLOCK
    local, tot = np.zeros(ntl), np.zeros(nblk)
    for b in range(nblk):
        run = 0.0
        for p in range(b * AREA_BLOCK, min((b + 1) * AREA_BLOCK, ntl)):
            run = run + float(area[p])
            local[p] = run
        tot[b] = run
    base = np.zeros(nblk)
    run = 0.0
    for b in range(nblk):
        base[b] = run
        run = run + float(tot[b])
    if not (run > 0.0 and math.isfinite(run)):
        return np.zeros(ntl, np.uint32), -1
    C = base[np.arange(ntl) // AREA_BLOCK] + local
    thr = np.minimum(np.floor(C / run * 4294967296.0), 4294967295.0).astype(np.uint64).astype(np.uint32)
    rises = np.nonzero(thr.astype(np.int64) > np.concatenate([[0], thr[:-1]]).astype(np.int64))[0]
    return thr, int(rises[-1]) if len(rises) else -1


def build(V, T, leaf=0):
    """A device-built mesh: {"table", "closed", "order", "nodes", "moments", "thresholds", "last", "ntl",
    "depth", "lo", "hi", "slack"}; nodes [nnodes, 8] float32 with words 3 and 7 int32, as nr_mesh_hierarchy's."""
    V = np.ascontiguousarray(V, F)
    T = np.asarray(T, np.int64).reshape(-1, 3)
    leaf = int(leaf) if leaf else 8
    lo, hi, maxabs = bound(V)
    slack = slack_of(lo, hi, maxabs)
    fn, live = face_normals(V, T)
    table, closed = table_of(V, T, fn, live)
    order = order_of(V, T, live, lo, hi)
    ntl = len(order)
    w3, w7, first, count, depth = shape(ntl, leaf)
    nn = len(w3)
    # per position: corners, A, |A|, x
    P = V[T[order]] if ntl else np.zeros((0, 3, 3), F)  # [ntl, 3 corners, 3]
    P64 = P.astype(D)
    A = 0.5 * cross(P64[:, 1] - P64[:, 0], P64[:, 2] - P64[:, 0])
    area = WR.length(A) if ntl else np.zeros(0)
    x = ((P64[:, 0] + P64[:, 1]) + P64[:, 2]) / 3.0
    # raw sums (sa, sx, mx, N, P) and exact boxes, children before parents
    sa, sx, mx, N, Pm = np.zeros(nn), np.zeros((nn, 3)), np.zeros((nn, 3)), np.zeros((nn, 3)), np.zeros((nn, 3, 3))
    blo, bhi = np.full((nn, 3), np.inf, F), np.full((nn, 3), -np.inf, F)
    for i in range(nn - 1, -1, -1):
        if w7[i] <= 0:
            for p in range(int(first[i]), int(first[i] + count[i])):
                sa[i] = sa[i] + area[p]
                sx[i] = sx[i] + area[p] * x[p]
                mx[i] = mx[i] + x[p]
                N[i] = N[i] + A[p]
                Pm[i] = Pm[i] + np.outer(A[p], x[p])
            if count[i]:
                pts = P[int(first[i]):int(first[i] + count[i])].reshape(-1, 3)
                blo[i], bhi[i] = pts.min(0), pts.max(0)
        else:
            l, r = int(w3[i]), int(w7[i])
            sa[i], sx[i], mx[i], N[i], Pm[i] = sa[l] + sa[r], sx[l] + sx[r], mx[l] + mx[r], N[l] + N[r], Pm[l] + Pm[r]
            blo[i], bhi[i] = np.minimum(blo[l], blo[r]), np.maximum(bhi[l], bhi[r])
    nodes = np.zeros((nn, 8), F)
    nodes[:, 0:3] = round_outward(blo.astype(D) - slack, up=False)
    nodes[:, 4:7] = round_outward(bhi.astype(D) + slack, up=True)
    words = nodes.view(np.int32)
    words[:, 3], words[:, 7] = w3, w7
    moments = np.zeros((nn, 16), F)
    for i in range(nn):
        if count[i] == 0:
            continue
        with np.errstate(all="ignore"):
            cen = (sx[i] / sa[i] if sa[i] > 0.0 else mx[i] / float(count[i])).astype(F)
            c = cen.astype(D)
            M = Pm[i] - np.outer(N[i], c)
            e = P64[int(first[i]):int(first[i] + count[i])].reshape(-1, 3) - c
            r2 = D(WR.dot(e, e).max())
        moments[i, 0:3] = cen
        moments[i, 3] = round_outward(np.array([r2]), up=True)[0]
        moments[i, 4:7] = N[i].astype(F)
        moments[i, 8:14] = np.array([M[0, 0], M[1, 1], M[2, 2], 0.5 * (M[0, 1] + M[1, 0]), 0.5 * (M[0, 2] + M[2, 0]),
                                     0.5 * (M[1, 2] + M[2, 1])]).astype(F)
    thr, last = area_table(area)
    return {"table": table, "closed": closed, "order": order, "nodes": nodes, "moments": moments, "thresholds": thr,
            "last": last, "ntl": ntl, "depth": depth, "lo": lo, "hi": hi, "slack": slack}


# ---- the meshes of both test files ------------------------------------------------------------------

def flat_cube():
    """the cube flattened to z = 0: an axis without extent, dead side faces, coincident top and bottom"""
    V, T = R.cube()
    V = V.copy()
    V[:, 2] = 0
    return V, T


def fine_torus():
    """the torus refined once by midpoint subdivision: nt > 2048 (a second sort tile for the triangles, a
    third for the corners, more than 256 live positions)"""
    V, T = R.torus()
    V64 = V.astype(D)
    mid = {}
    verts = [v for v in V]

    def midpoint(i, j):
        key = (min(i, j), max(i, j))
        if key not in mid:
            mid[key] = len(verts)
            verts.append(((V64[i] + V64[j]) * 0.5).astype(F))
        return mid[key]

    tris = []
    for a, b, c in T.tolist():
        ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
        tris += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    return np.array(verts, F), np.array(tris, np.int32)


def one_triangle():
    return np.array([[0.1, 0.2, 0.3], [0.9, 0.1, -0.2], [0.3, 0.8, 0.4]], F), np.array([[0, 1, 2]], np.int32)


MESHES = {"one_triangle": one_triangle, "tetrahedron": R.tetrahedron, "cube": R.cube, "torus": R.torus,
          "degenerate_torus": R.degenerate_torus, "open_torus": WR.open_torus, "double_cube": WR.double_cube,
          "flat_cube": flat_cube, "fine_torus": fine_torus}


@functools.lru_cache(maxsize=None)
def mesh(name):
    V, T = MESHES[name]()
    V, T = np.array(V, F), np.array(T, np.int32)
    V.setflags(write=False)
    T.setflags(write=False)
    return V, T


@functools.lru_cache(maxsize=None)
def reference(name, leaf=0):
    """build() of mesh(name), computed once and shared (read-only arrays)"""
    out = build(*mesh(name), leaf=leaf)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
