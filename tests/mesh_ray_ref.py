"""Reference for the mesh ray queries (nr_mesh_trace_rays, nr_mesh_gbuffer, nr_mesh_render): a helper,
not a test.

The numpy restatement of the ray contract in include/neural_render.h, written from that text: brute
force over the live triangles with the header's chains (np.float32, one rounding per operation, the
exact f32 fmaf of trimesh_ref), the winner as the minimum of (t, triangle index), both kinds of normal,
and the colours of shade_color.  walk() applies the skip rule of the header's step 5 to the tree that
nr.trimesh_hierarchy returns.  tests/test_mesh_rays_cpu.py pins this file against an independent
float64 implementation, so the GPU comparison is not vacuous.

Also the ray sets both test files use.
"""
import functools

import numpy as np

import trimesh_ref as tr

F = np.float32
MISS, HIT = 0, 2
KEYS = ("status", "t", "tri", "bary", "position", "normal")
INF = F(np.inf)


# ---- steps 1 and 2: a ray against triangles ---------------------------------------------------------

def dead(O, D):
    """Step 1: a ray with a number that is not finite, or with d = (0, 0, 0)."""
    return ~(np.isfinite(O).all(1) & np.isfinite(D).all(1)) | ~D.any(1)


def shear(D):
    """(kx, ky, kz, Sx, Sy, Sz) of step 1, each [n]."""
    n = len(D)
    ar = np.arange(n)
    ad = np.abs(D)
    kz = np.zeros(n, np.int64)
    kz = np.where(ad[:, 1] > ad[ar, kz], 1, kz)
    kz = np.where(ad[:, 2] > ad[ar, kz], 2, kz)
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    neg = D[ar, kz] < 0
    kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
    with np.errstate(all="ignore"):
        dz = D[ar, kz]
        return kx, ky, kz, D[ar, kx] / dz, D[ar, ky] / dz, F(1.0) / dz


def pairs(O, D, a, b, c, tmin, tmax):
    """Step 2 for rays [n] against triangles (a, b, c) [m, 3]: dict of [n, m] arrays hit, t, U, V, W, det."""
    O, D = np.asarray(O, F), np.asarray(D, F)
    n = len(O)
    kx, ky, kz, Sx, Sy, Sz = shear(D)
    pick = lambda P, k: np.take_along_axis(P, k[:, None, None], 2)[..., 0]
    with np.errstate(all="ignore"):
        P3 = [(np.asarray(p, F)[None, :, :] - O[:, None, :]).astype(F) for p in (a, b, c)]
        z = [pick(P, kz) for P in P3]
        x = [pick(P, kx) - Sx[:, None] * zz for P, zz in zip(P3, z)]
        y = [pick(P, ky) - Sy[:, None] * zz for P, zz in zip(P3, z)]
        (Ax, Bx, Cx), (Ay, By, Cy), (Az, Bz, Cz) = x, y, [Sz[:, None] * zz for zz in z]
        U = Cx * By - Cy * Bx
        V = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        missed = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = (U + V) + W
        Tn = (U * Az + V * Bz) + W * Cz
        t = Tn / det
        hit = ~missed & (det != 0) & (F(tmin) <= t) & (t <= F(tmax))
    for v in (U, V, W, det, t):
        assert v.dtype == F
    return {"hit": hit & ~dead(O, D)[:, None], "t": t, "U": U, "V": V, "W": W, "det": det}


# ---- step 3: the outputs of a winner ----------------------------------------------------------------

def normalise(v):
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        l2 = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
        return v * (F(1.0) / np.sqrt(l2))[..., None], l2


def _unit_or(v, face):
    u, l2 = normalise(v)
    bad = ~(l2 > 0) | ~np.isfinite(l2)
    return np.where(bad[..., None], face, u).astype(F)


def finish(O, D, win, t, U, V, W, det, table, smooth):
    """The six outputs from the winner per ray (win [n], -1: none) and its t, U, V, W, det [n]."""
    n = len(O)
    hit = win >= 0
    w = np.where(hit, win, 0)
    out = {"status": np.where(hit, HIT, MISS).astype(np.int32), "t": np.where(hit, t, F(0)).astype(F),
           "tri": np.where(hit, win, -1).astype(np.int32)}
    with np.errstate(all="ignore"):
        bary = np.stack([U / det, V / det, W / det], -1).astype(F)
        pos = np.stack([tr.fmaf(D[:, k], t, O[:, k]) for k in range(3)], -1)
        face = table[w, 0]
        nrm = face
        if smooth:
            na, nb, nc = (_unit_or(table[w, 4 + k], face) for k in range(3))
            m = np.stack([tr.fmaf(nc[:, k], bary[:, 2], tr.fmaf(nb[:, k], bary[:, 1], (na[:, k] * bary[:, 0]).astype(F)))
                          for k in range(3)], -1)
            nrm = _unit_or(m, face)
    z3 = np.zeros((n, 3), F)
    out["bary"] = np.where(hit[:, None], bary, z3).astype(F)
    out["position"] = np.where(hit[:, None], pos, z3).astype(F)
    out["normal"] = np.where(hit[:, None], nrm, z3).astype(F)
    return out


def trace(V, T, O, D, tmin=0.0, tmax=np.inf, smooth=False, table=None, chunk=128):
    """nr_mesh_trace_rays' outputs for rays (O, D) by brute force, and the live-ray and live-triangle
    counts: (out, {"live_rays", "live_tris"})."""
    V, T = np.asarray(V, F), np.asarray(T).reshape(-1, 3)
    O, D = np.ascontiguousarray(O, F).reshape(-1, 3), np.ascontiguousarray(D, F).reshape(-1, 3)
    if table is None:
        table = tr.normals(V, T)[0]
    livet = np.flatnonzero(table[:, 0].any(1))
    a, b, c = V[T[livet, 0]], V[T[livet, 1]], V[T[livet, 2]]
    n = len(O)
    win = np.full(n, -1, np.int64)
    rec = {k: np.zeros(n, F) for k in ("t", "U", "V", "W", "det")}
    for s in range(0, n, chunk):
        if not len(livet):
            break
        r = pairs(O[s:s + chunk], D[s:s + chunk], a, b, c, tmin, tmax)
        key = np.where(r["hit"], r["t"], INF)
        # the minimum of (t, index): livet ascends, so the first position of the minimum
        first = np.argmax(r["hit"] & (key == key.min(1)[:, None]), 1)
        any_ = r["hit"].any(1)
        sl = slice(s, s + len(first))
        win[sl] = np.where(any_, livet[first], -1)
        ar = np.arange(len(first))
        for k in rec:
            rec[k][sl] = r[k][ar, first]
    out = finish(O, D, win, rec["t"], rec["U"], rec["V"], rec["W"], rec["det"], table, smooth)
    return out, {"live_rays": int((~dead(O, D)).sum()), "live_tris": int(len(livet))}


# ---- step 5: the walk -------------------------------------------------------------------------------

def scale_of(V):
    """S: the largest |coordinate| plus the largest axis extent of the vertices."""
    V64 = np.asarray(V, F).astype(np.float64)
    return F(np.abs(V64).max() + (V64.max(0) - V64.min(0)).max())


def wants(O, D, pad, lo, hi, tmin, lim):
    """(wants [n], tn [n]) of the header's slab rule for rays against one stored box (lo, hi)."""
    with np.errstate(all="ignore"):
        inv = F(1.0) / D
        t1 = ((lo[None] - pad[:, None]) - O) * inv
        t2 = ((hi[None] + pad[:, None]) - O) * inv
        mn, mx = np.fmin(t1, t2), np.fmax(t1, t2)
        tn = np.fmax(np.fmax(mn[:, 0], mn[:, 1]), mn[:, 2])
        tf = np.fmin(np.fmin(mx[:, 0], mx[:, 1]), mx[:, 2])
        return ~(tn > tf) & ~(tf < F(tmin)) & ~(tn > lim), tn


def walk(nodes, order, V, T, O, D, tmin=0.0, tmax=np.inf, smooth=False, table=None, any_hit=False):
    """The outputs of trace() by the walk of step 5 over the hierarchy (nodes, order), every ray by
    its own rule: a node is entered for exactly the rays that want it.  Returns (out, leaves), leaves
    [n] the number of leaves entered per ray.  With any_hit only out["status"] means anything."""
    V, T = np.asarray(V, F), np.asarray(T).reshape(-1, 3)
    O, D = np.ascontiguousarray(O, F).reshape(-1, 3), np.ascontiguousarray(D, F).reshape(-1, 3)
    if table is None:
        table = tr.normals(V, T)[0]
    nodes = np.ascontiguousarray(nodes, F).reshape(-1, 8)
    links = nodes.view(np.int32)
    order = np.asarray(order, np.int64)
    n = len(O)
    pad = (F(2.0 ** -18) * (np.abs(O).max(1) + scale_of(V))).astype(F)
    best = np.full(n, INF, F)
    besti = np.full(n, np.iinfo(np.int64).max, np.int64)
    rec = {k: np.zeros(n, F) for k in ("t", "U", "V", "W", "det")}
    leaves = np.zeros(n, np.int64)
    found = np.zeros(n, bool)

    def lim(idx):
        return np.minimum(best[idx], F(tmax))

    def visit(node, idx):
        if any_hit:
            idx = idx[~found[idx]]
        if not len(idx):
            return
        w3, w7 = int(links[node, 3]), int(links[node, 7])
        if w7 <= 0:
            leaves[idx] += 1
            pos = order[w3:w3 - w7]
            if not len(pos):
                return
            r = pairs(O[idx], D[idx], V[T[pos, 0]], V[T[pos, 1]], V[T[pos, 2]], tmin, tmax)
            for j, ti in enumerate(pos):
                h = r["hit"][:, j]
                tt = r["t"][:, j]
                better = h & ((tt < best[idx]) | ((tt == best[idx]) & (ti < besti[idx])))
                sel = idx[better]
                best[sel] = tt[better]
                besti[sel] = ti
                for k in rec:
                    rec[k][sel] = r[k][better, j]
                found[idx[h]] = True
            return
        wl, tl = wants(O[idx], D[idx], pad[idx], nodes[w3, 0:3], nodes[w3, 4:7], tmin, lim(idx))
        wr, trr = wants(O[idx], D[idx], pad[idx], nodes[w7, 0:3], nodes[w7, 4:7], tmin, lim(idx))
        left_near = 2 * int((tl <= trr).sum()) >= len(idx)
        if left_near:
            visit(w3, idx[wl])
            # the far child is tested again: best has shrunk meanwhile
            wr, _ = wants(O[idx], D[idx], pad[idx], nodes[w7, 0:3], nodes[w7, 4:7], tmin, lim(idx))
            visit(w7, idx[wr])
        else:
            visit(w7, idx[wr])
            wl, _ = wants(O[idx], D[idx], pad[idx], nodes[w3, 0:3], nodes[w3, 4:7], tmin, lim(idx))
            visit(w3, idx[wl])

    visit(0, np.flatnonzero(~dead(O, D)))
    win = np.where(besti < np.iinfo(np.int64).max, besti, -1)
    out = finish(O, D, win, rec["t"], rec["U"], rec["V"], rec["W"], rec["det"], table, smooth)
    return out, leaves


# ---- colours (shade_color) --------------------------------------------------------------------------

def facing(normal, dirs, status):
    import query_ref
    return query_ref.facing(normal, dirs, status)


def matcap(normal, status, normal_matrix, texels):
    """matCapColor per ray: the texel at trunc((normalise(nm n) / 2 + 1 / 2) (size - 1)) for a HIT, else 0."""
    nrm = np.asarray(normal, F).reshape(-1, 3)
    nm = np.asarray(normal_matrix, F).reshape(4, 4)
    tex = np.asarray(texels, np.uint32)
    mh, mw = tex.shape
    with np.errstate(all="ignore"):
        e = np.stack([((nrm[:, 0] * r[0] + nrm[:, 1] * r[1]) + nrm[:, 2] * r[2]) + F(0) * r[3] for r in nm[:3]], -1).astype(F)
        ne, _ = normalise(e)
        fu = (ne[:, 0].astype(np.float64) * 0.5 + 0.5).astype(F)
        fv = (ne[:, 1].astype(np.float64) * 0.5 + 0.5).astype(F)

        def rz(f):  # f2i_rz: a NaN gives 0
            return np.where(np.isnan(f), 0, np.trunc(np.nan_to_num(f))).astype(np.int64)

        ux = np.minimum(rz(fu * F(mw - 1)), mw - 1)
        uy = np.minimum(rz(fv * F(mh - 1)), mh - 1)
    index = uy * mw + ux
    px = np.where(index < 0, 0, tex.reshape(-1)[np.clip(index, 0, mh * mw - 1)])
    return np.where(np.asarray(status).reshape(-1) == HIT, px, 0).astype(np.uint32)


def bits(a):
    return tr.bits(a)


# ---- the ray sets -----------------------------------------------------------------------------------

NR = 1063  # 16 full chunks of 64 and a tail of 39
WINDOWS = ((0.0, np.inf), (0.8, 1.05))  # the second cuts first hits off at both ends (targets lie at t = 1)


def _mesh(name):
    return tr.degenerate_torus() if name == "degenerate_torus" else tr.mesh(name)


@functools.lru_cache(maxsize=None)
def rays(name, n=NR, seed=5):
    """n rays around mesh `name`: two chunks of neighbouring rays, then, shuffled: origins in +-1.5
    aimed at points of the bound (d = target - origin, so the target is at t = 1); origins up to |o| =
    100; axis-parallel rays and rays with
    one zero component; origins that share coordinates with a vertex; origins on the surface (face
    centroids, vertices); dead rays."""
    V, T = _mesh(name)
    rng = np.random.default_rng(seed)
    lo, hi = V.min(0).astype(np.float64), V.max(0).astype(np.float64)
    target = lambda k: rng.uniform(lo, hi, (k, 3))
    A, B, C = V[T[:, 0]].astype(np.float64), V[T[:, 1]].astype(np.float64), V[T[:, 2]].astype(np.float64)
    sets = []

    def add(o, d):
        sets.append((np.asarray(o, np.float64).astype(F), np.asarray(d, np.float64).astype(F)))

    k = 120
    o = rng.uniform(-100, 100, (k, 3))
    add(o, target(k) - o)                                   # far origins
    o = rng.uniform(-1.5, 1.5, (k, 3))
    d = target(k) - o
    d[np.arange(k), rng.integers(0, 3, k)] = 0.0
    add(o, d)                                               # one zero component
    o = rng.uniform(-1.5, 1.5, (60, 3))
    d = np.zeros((60, 3))
    d[np.arange(60), rng.integers(0, 3, 60)] = rng.choice([-1.0, 1.0, 0.37, -2.5], 60)
    o2 = target(60)
    ax = np.abs(d).argmax(1)
    o2[np.arange(60), ax] = o[np.arange(60), ax]
    add(o2, d)                                              # axis-parallel, through the bound
    vs = V[rng.integers(0, len(V), k)].astype(np.float64)
    o = vs.copy()
    o[np.arange(k), rng.integers(0, 3, k)] += rng.uniform(-1.5, 1.5, k)
    add(o, target(k) - o)                                   # two coordinates of a vertex
    add(o[:40], vs[:40] - o[:40])                           # ... aimed at it: axis-parallel through a vertex
    ts = rng.integers(0, len(T), k)
    cen = ((A[ts] + B[ts]) + C[ts]) / 3.0
    add(cen, rng.normal(size=(k, 3)))                       # on the surface
    add(V[rng.integers(0, len(V), 40)], rng.normal(size=(40, 3)))
    o = rng.uniform(-1.5, 1.5, (12, 3))
    d = rng.normal(size=(12, 3))
    o[0, 0], o[1, 2], d[2, 1], d[3, 0] = np.nan, np.inf, np.nan, -np.inf
    d[4:8] = 0.0
    d[8] = (0.0, -0.0, 0.0)
    o[9], d[10] = (np.inf, np.nan, 0.0), (np.inf, np.inf, np.inf)
    add(o, d)                                               # dead rays (11 is an ordinary one)
    have = sum(len(s[0]) for s in sets) + 128
    assert have <= n - 300, have
    o = rng.uniform(-1.5, 1.5, (n - have, 3))
    add(o, target(n - have) - o)
    O = np.concatenate([s[0] for s in sets])
    D = np.concatenate([s[1] for s in sets])
    p = rng.permutation(len(O))
    # in front of the shuffled rays two chunks of 64 neighbours each, a near and a far bundle at one spot
    # of the mesh: the rays that share a walk have to be neighbours for the walk to skip anything
    sets = []
    spot, width = (lo + hi) / 2 + (hi - lo) * (0.2, -0.15, 0.1), (hi - lo) * 0.04
    for eye in ((1.4, 1.2, 1.3), (60.0, -80.0, 45.0)):
        o = np.asarray(eye) + rng.uniform(-0.02, 0.02, (64, 3))
        add(o, rng.uniform(spot - width, spot + width, (64, 3)) - o)
    O = np.ascontiguousarray(np.concatenate([s[0] for s in sets] + [O[p]]))
    D = np.ascontiguousarray(np.concatenate([s[1] for s in sets] + [D[p]]))
    assert len(O) == n
    O.setflags(write=False)
    D.setflags(write=False)
    return O, D


@functools.lru_cache(maxsize=None)
def reference(name, window=0, smooth=False, n=NR):
    """trace() of rays(name) in WINDOWS[window], computed once and shared (read-only)."""
    V, T = _mesh(name)
    O, D = rays(name, n)
    out, counts = trace(V, T, O, D, *WINDOWS[window], smooth=smooth)
    for a in out.values():
        a.setflags(write=False)
    return out, counts


INSIDE = {"tetrahedron": (0.375, 0.2375, 0.1625), "cube": (0.05, 0.05, 0.05), "torus": (0.6, 0.0, 0.0)}
NUDGE = (0.01, -0.02, 0.015)


@functools.lru_cache(maxsize=None)
def watertight_rays(name, moved=False):
    """From a point strictly inside closed mesh `name`, rays at every vertex, every f32 edge midpoint
    and every face centroid."""
    V, T = tr.mesh(name)
    o = np.asarray(INSIDE[name], np.float64) + (np.asarray(NUDGE) if moved else 0.0)
    o = o.astype(F)
    edges = np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]])  # every edge of every triangle
    mid = ((V[edges[:, 0]] + V[edges[:, 1]]) * F(0.5)).astype(F)
    cen = (((V[T[:, 0]] + V[T[:, 1]]) + V[T[:, 2]]) / F(3)).astype(F)
    P = np.concatenate([V, mid, cen]).astype(F)
    O = np.broadcast_to(o, P.shape).copy()
    D = (P - O).astype(F)
    O.setflags(write=False)
    D.setflags(write=False)
    return O, D
