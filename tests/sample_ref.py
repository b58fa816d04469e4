"""Reference for the fitting samples (nr_mesh_area_table, nr_mesh_sample, nr_points_order,
nr_mesh_fit_samples): a helper, not a test.

The numpy restatement of the contract in include/neural_render.h, written from that text: Philox4x32-10
on uint64 arrays, the area table in float64 over the positions of nr.trimesh_hierarchy's order, the
surface and volume points with trimesh_ref's exact f32 fmaf, the Morton and shuffle keys, and
np.argsort(kind="stable") in the sort's place.  The fused pipeline labels the points with
trimesh_ref.distance (brute force: the winner is a minimum, so the order and the hierarchy change no
bit) or winding_ref.winding through the exported tree.  tests/test_sample_cpu.py pins this file against
the Random123 known answers, the library's table and the distributions the contract promises.
"""
import functools

import numpy as np

import trimesh_ref as R
import winding_ref as WR

F = np.float32
U32 = np.uint64(0xffffffff)
INV24 = F(2.0 ** -24)
JITTER_C = np.uint32(0x379cc471).view(F)  # sqrt(1.5) / 65536


def philox(c, k):
    """Philox4x32-10: counters c [..., 4] and a key k [2] or [..., 2] (uint32 values) -> words [..., 4] uint32."""
    c, k = np.asarray(c, np.uint64), np.asarray(k, np.uint64)
    c0, c1, c2, c3 = (c[..., j] for j in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & U32
        k0 = (k0 + np.uint64(0x9E3779B9)) & U32
        k1 = (k1 + np.uint64(0xBB67AE85)) & U32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), -1).astype(np.uint32)


def words(seed, i, stream):
    """the four words of sample index i (array) in `stream` under `seed`"""
    i = np.asarray(i, np.uint64)
    c = np.stack([i & U32, i >> np.uint64(32), np.full(i.shape, stream, np.uint64), np.zeros(i.shape, np.uint64)], -1)
    seed = int(seed)
    return philox(c, np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff], np.uint64))


def area_table(V, T, order):
    """(thresholds [ntl] uint32, L) over the triangles T[order], in position order."""
    V64 = np.asarray(V, F).astype(np.float64)
    T = np.asarray(T).reshape(-1, 3)
    order = np.asarray(order, np.int64)
    if len(order) == 0:
        return np.zeros(0, np.uint32), -1
    a, b, c = (V64[T[order, k]] for k in range(3))
    u, v = b - a, c - a
    A = 0.5 * np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                        u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], -1)
    area = np.sqrt((A[:, 0] * A[:, 0] + A[:, 1] * A[:, 1]) + A[:, 2] * A[:, 2])
    C = np.zeros(len(order))
    s = 0.0
    for p in range(len(order)):  # the sequential sum
        s = s + float(area[p])
        C[p] = s
    if not s > 0.0:
        return np.zeros(len(order), np.uint32), -1
    thr = np.minimum(np.floor(C / s * 4294967296.0), 4294967295.0).astype(np.uint64).astype(np.uint32)
    rises = np.nonzero(thr.astype(np.int64) > np.concatenate([[0], thr[:-1]]).astype(np.int64))[0]
    return thr, int(rises[-1])


def jitter(seed, i, stream):
    w = words(seed, i, stream).astype(np.int64)
    S = ((w & 0xffff) + (w >> 16)).sum(-1)
    return ((S - 262140).astype(F) * JITTER_C).astype(F)


def sample(V, T, order, seed, n_surface, n_volume, sigma=0.0, lo=(-1, -1, -1), hi=(1, 1, 1)):
    """nr_mesh_sample's outputs: {"points" [n, 3], "tri" [n], "bary" [n, 3]}."""
    V, T = np.asarray(V, F), np.asarray(T).reshape(-1, 3)
    order = np.asarray(order, np.int64)
    lo, hi = np.broadcast_to(np.asarray(lo, F), (3,)), np.broadcast_to(np.asarray(hi, F), (3,))
    n = n_surface + n_volume
    idx = np.arange(n, dtype=np.uint64)
    w = words(seed, idx, 0)
    pts = np.zeros((n, 3), F)
    tri = np.full(n, -1, np.int32)
    bary = np.zeros((n, 3), F)
    if n_surface:
        thr, last = area_table(V, T, order)
        assert last >= 0, "no area to sample"
        ws = w[:n_surface]
        pos = np.minimum(np.searchsorted(thr, ws[:, 0], side="right"), last)
        t = order[pos]
        a, b, c = V[T[t, 0]], V[T[t, 1]], V[T[t, 2]]
        iu, iv = (ws[:, 1] >> np.uint32(8)).astype(np.int64), (ws[:, 2] >> np.uint32(8)).astype(np.int64)
        flip = iu + iv > (1 << 24)
        iu, iv = np.where(flip, (1 << 24) - iu, iu), np.where(flip, (1 << 24) - iv, iv)
        u, v = iu.astype(F) * INV24, iv.astype(F) * INV24
        e1, e2 = (b - a).astype(F), (c - a).astype(F)
        p = np.stack([R.fmaf(v, e2[:, k], R.fmaf(u, e1[:, k], a[:, k])) for k in range(3)], -1)
        if sigma > 0:
            p = np.stack([R.fmaf(F(sigma), jitter(seed, idx[:n_surface], 1 + k), p[:, k]) for k in range(3)], -1)
        pts[:n_surface] = p
        tri[:n_surface] = t
        bary[:n_surface] = np.stack([((1 << 24) - iu - iv).astype(F) * INV24, u, v], -1)
    if n_volume:
        wv = w[n_surface:]
        ext = (hi - lo).astype(F)
        pts[n_surface:] = np.stack([R.fmaf((wv[:, k] >> np.uint32(8)).astype(F) * INV24, ext[k], lo[k]) for k in range(3)], -1)
    return {"points": pts, "tri": tri, "bary": bary}


def spread(v):
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    return (v | (v << 2)) & 0x09249249


def morton_keys(X, lo, hi):
    X = np.asarray(X, F).reshape(-1, 3)
    lo, hi = np.broadcast_to(np.asarray(lo, F), (3,)), np.broadcast_to(np.asarray(hi, F), (3,))
    with np.errstate(all="ignore"):
        inv = (F(1023.0) / (hi - lo).astype(F)).astype(F)
        t = ((X - lo).astype(F) * inv).astype(F)
        ti = np.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0).clip(0, 1023).astype(np.int64)  # (int)t where 0 < t < 1023
        q = np.where(t >= 1023, 1023, np.where(t > 0, ti, 0)).astype(np.int64)
    return (spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)).astype(np.uint32)


def shuffle_keys(seed, n):
    return words(seed, np.arange(n, dtype=np.uint64), 4)[:, 0]


def order(keys):
    return np.argsort(keys, kind="stable").astype(np.int32)


def fit_samples(V, T, tree, seed, n_surface, n_volume, sigma, lo, hi, sign="normal", beta=0.0):
    """nr_mesh_fit_samples' (X, Y): tree = (nodes, order, moments) of nr.trimesh_hierarchy."""
    nodes, pos_order, moments = tree[:3]
    P = sample(V, T, pos_order, seed, n_surface, n_volume, sigma, lo, hi)["points"]
    Y = R.distance(V, T, P)["sdf"]
    if sign == "winding":
        w = WR.winding(V, T, P, beta, nodes, pos_order, moments)
        with np.errstate(all="ignore"):
            Y = np.where(np.isnan(Y), Y, np.where(w >= F(0.5), -np.abs(Y), np.abs(Y))).astype(F)
    first = order(morton_keys(P, lo, hi))
    Ps, Ys = P[first], Y[first]
    perm = order(shuffle_keys(seed, len(P)))
    return Ps[perm], Ys[perm]


@functools.lru_cache(maxsize=None)
def scaled_cube():
    """The cube with its +x face moved out (the x extent doubles) and z halved: the areas of the x, y and
    z faces are as 1 : 2 : 4."""
    V, T = R.cube()
    V = V.copy()
    V[:, 0] = np.where(V[:, 0] > 0.2, V[:, 0] + F(0.8), V[:, 0])  # x extent doubles: y and z faces double
    V[:, 2] = (V[:, 2] * F(0.5)).astype(F)                        # z extent halves: x and y faces halve
    V.setflags(write=False)
    return V, T
