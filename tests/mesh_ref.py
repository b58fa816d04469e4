"""Reference for the volume sampling and the isosurface extraction (nr_sample_grid, nr_mesh_grid,
nr_extract_mesh): a helper, not a test.

The numpy restatement of the definitions in include/neural_render.h, written from that text: the
lattice, the inside test, the Kuhn split, the vertex numbering and interpolation (np.float32, one
rounding per operation) and the triangle rule, whose table is derived here from the midpoint rule
with float cross products.  The values come from the CPU oracle the way tests/query_ref.py takes
them (OracleNet.forward, oracle.scene_sdf).  tests/test_mesh_cpu.py pins this file's meshes
(closed, oriented, on the surface, every case reached), so the GPU comparison is not vacuous.
"""
import itertools

import numpy as np

import query_ref

F = np.float32
QNAN = np.uint32(0x7fc00000).view(F)
# the 7 edge kinds o -> o + e, in slot order (x first)
SLOTS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1]])
# the axis permutations in lexicographic order: xyz, xzy, yxz, yzx, zxy, zyx
PERMS = list(itertools.permutations(range(3)))


# the lattice both test files mesh: 6 x 5 x 4 uniform values in [-1, 1] (every cell is active, the
# surface is open at the lattice faces), on an anisotropic lattice
RANDOM_ORIGIN, RANDOM_STEP = (0.1, -0.2, 0.3), (0.5, 0.25, 0.7)


def random_lattice():
    return np.random.default_rng(5).uniform(-1, 1, (4, 5, 6)).astype(F)


def tet_path(t):
    """The 4 cell corners (x, y, z offsets) of tetrahedron t's path v0 .. v3."""
    v = [np.zeros(3, int)]
    for ax in PERMS[t]:
        e = np.zeros(3, int)
        e[ax] = 1
        v.append(v[-1] + e)
    return np.array(v)


def _slot(e):
    return int(np.flatnonzero((SLOTS == e).all(1))[0])


def tet_triangles(t, mask):
    """The triangles of tetrahedron t whose path vertex m is inside iff bit m of mask: a list of
    triangles, each three (base corner offset, slot) lattice edges, wound so that with the vertices
    at the edge midpoints (b - a) x (c - a) points from the inside corners' centroid to the outside
    corners'."""
    path = tet_path(t)
    ins = [m for m in range(4) if (mask >> m) & 1]
    outs = [m for m in range(4) if not (mask >> m) & 1]
    if not ins or not outs:
        return []
    if len(ins) == 1:
        tris = [[(ins[0], q) for q in outs]]
    elif len(outs) == 1:
        tris = [[(outs[0], q) for q in ins]]
    else:
        (A, B), (C, D) = ins, outs
        tris = [[(A, C), (A, D), (B, D)], [(A, C), (B, D), (B, C)]]
    direction = path[outs].mean(0) - path[ins].mean(0)
    res = []
    for tri in tris:
        mid = [(path[m] + path[n]) / 2.0 for m, n in tri]
        if np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), direction) < 0:
            tri = [tri[0], tri[2], tri[1]]
        edges = []
        for m, n in tri:
            lo, hi = min(m, n), max(m, n)
            edges.append((tuple(path[lo]), _slot(path[hi] - path[lo])))
        res.append(edges)
    return res


def lattice(origin, step, dims):
    """The lattice points [n, 3] in linear-index order (k ny + j) nx + i: origin + (float)idx * step,
    one f32 multiply, then one f32 add."""
    o, s = np.asarray(origin, F), np.asarray(step, F)
    ax = [(o[a] + np.arange(dims[a]).astype(F) * s[a]).astype(F) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3).astype(F)


def sample(net, origin, step, dims, scene=0, frame=0):
    """nr_sample_grid's values [nz, ny, nx]: sceneSDF(p, mlp(p)) through the oracle."""
    P = lattice(origin, step, dims)
    with np.errstate(all="ignore"):
        v = query_ref._scene(P, query_ref._mlp(net, P, frame), scene, frame)
    return v.reshape(dims[2], dims[1], dims[0])


def tet_masks(sdf, iso=0.0):
    """[cells, 6] inside masks of every cell's tetrahedra (cells in increasing cell index)."""
    inside = np.asarray(sdf, F) < F(iso)
    nz, ny, nx = inside.shape
    out = np.zeros((nz - 1, ny - 1, nx - 1, 6), int)
    for t in range(6):
        for m, (cx, cy, cz) in enumerate(tet_path(t)):
            out[..., t] |= inside[cz:nz - 1 + cz, cy:ny - 1 + cy, cx:nx - 1 + cx].astype(int) << m
    return out.reshape(-1, 6)


def mesh(sdf, origin, step, iso=0.0):
    """nr_mesh_grid's output for the lattice values sdf [nz, ny, nx]: the vertices V [nv, 3] in the
    pinned order, the triangles T [nt, 3] in increasing cell index (tetrahedron order within a
    cell), each triangle's cell index, and each vertex's key index(o) * 7 + slot."""
    sdf = np.ascontiguousarray(sdf, F)
    iso = F(iso)
    nz, ny, nx = sdf.shape
    n = nx * ny * nz
    inside = sdf < iso
    o, s = np.asarray(origin, F), np.asarray(step, F)
    coord = [(o[a] + np.arange(d).astype(F) * s[a]).astype(F) for a, d in enumerate((nx, ny, nz))]
    kk, jj, ii = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    index = (kk * ny + jj) * nx + ii
    keys, pos = [], []
    with np.errstate(all="ignore"):
        for slot, (ex, ey, ez) in enumerate(SLOTS):
            sa = (slice(0, nz - ez), slice(0, ny - ey), slice(0, nx - ex))
            sb = (slice(ez, nz), slice(ey, ny), slice(ex, nx))
            cross = inside[sa] != inside[sb]
            a, b = sdf[sa][cross], sdf[sb][cross]
            t = ((iso - a) / (b - a)).astype(F)
            comps = []
            for ax, (e, idx) in enumerate(((ex, ii), (ey, jj), (ez, kk))):
                pa = coord[ax][idx[sa][cross]]
                pb = coord[ax][idx[sa][cross] + e]
                v = (pa + ((pb - pa).astype(F) * t).astype(F)).astype(F)
                comps.append(np.where(np.isnan(v), QNAN, v))
            keys.append(index[sa][cross] * 7 + slot)
            pos.append(np.stack(comps, -1))
    keys = np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    V = np.concatenate(pos)[order].astype(F).reshape(-1, 3)
    vid = np.full(n * 7, -1, np.int64)
    vid[keys] = np.arange(len(keys))
    # triangles, tetrahedron by tetrahedron and case by case
    masks = tet_masks(sdf, iso)
    cell_index = index[:nz - 1, :ny - 1, :nx - 1].reshape(-1)
    rows = []  # (cell, tetrahedron, triangle within it, a, b, c)
    for t in range(6):
        for mask in range(1, 15):
            sel = np.flatnonzero(masks[:, t] == mask)
            if not sel.size:
                continue
            for q, tri in enumerate(tet_triangles(t, mask)):
                ids = []
                for (cx, cy, cz), slot in tri:
                    base = cell_index[sel] + (cz * ny + cy) * nx + cx
                    ids.append(vid[base * 7 + slot])
                rows.append(np.stack([cell_index[sel], np.full(sel.size, t), np.full(sel.size, q)] + ids, -1))
    if rows:
        rows = np.concatenate(rows)
        rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    else:
        rows = np.zeros((0, 6), np.int64)
    assert (rows[:, 3:] >= 0).all(), "a triangle names an edge without a vertex"
    return V, rows[:, 3:].astype(np.int32), rows[:, 0].astype(np.int64), keys


def normals(net, V, scene=0, frame=0):
    """The vertex normals of nr_extract_mesh: query_ref's tetrahedron formula at each vertex."""
    V = np.ascontiguousarray(V, F).reshape(-1, 3)
    if not len(V):
        return np.zeros((0, 3), F)
    acc = None
    with np.errstate(all="ignore"):
        for q in range(4):
            pq = (V + query_ref.TET[q] * query_ref.NORMAL_EPSILON).astype(F)
            c = query_ref.TET[q][None, :] * query_ref._scene(pq, query_ref._mlp(net, pq, frame), scene, frame)[:, None]
            acc = c if acc is None else acc + c
        return query_ref.normalize3(acc)


# ---- comparison conventions ---------------------------------------------------

def bits(a):
    """f32 values are compared on their uint32 views"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def rotated(T):
    """Every triangle rotated to start at its smallest index (the winding is kept)."""
    T = np.asarray(T).reshape(-1, 3)
    r = np.argmin(T, 1)
    return np.stack([T[np.arange(len(T)), (r + s) % 3] for s in range(3)], -1)


def cell_sets(T, cells):
    """{cell: sorted list of its rotated triangles}: pins the cell order of the list without pinning
    the order inside a cell."""
    cells = np.asarray(cells)
    assert (np.diff(cells) >= 0).all(), "triangles are not in increasing cell index"
    out = {}
    for c, tri in zip(cells.tolist(), rotated(T).tolist()):
        out.setdefault(c, []).append(tuple(tri))
    return {c: sorted(v) for c, v in out.items()}


def triangle_cells(T, keys, dims):
    """The cell of each triangle of a mesh whose vertex keys are known: the cell whose 8 corners hold
    every endpoint of the three lattice edges (the component-wise minimum of their base points)."""
    nx, ny, _ = dims
    T = np.asarray(T).reshape(-1, 3)
    base = np.asarray(keys)[T] // 7
    i, j, k = base % nx, (base // nx) % ny, base // (nx * ny)
    return (k.min(1) * ny + j.min(1)) * nx + i.min(1)


def directed_edges(T):
    T = np.asarray(T).reshape(-1, 3)
    return np.concatenate([T[:, [0, 1]], T[:, [1, 2]], T[:, [2, 0]]])


def is_closed_oriented(T):
    """Every directed edge appears once and its reverse appears once."""
    E = directed_edges(T).astype(np.int64)
    if not len(E):
        return False
    m = int(E.max()) + 1
    fwd = E[:, 0] * m + E[:, 1]
    rev = E[:, 1] * m + E[:, 0]
    return len(np.unique(fwd)) == len(fwd) and np.array_equal(np.sort(fwd), np.sort(rev))
