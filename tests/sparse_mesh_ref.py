"""Reference for the brick-sparse extraction (nr_extract_mesh_sparse): a helper, not a test.

Written from the contract in include/neural_render.h: the bricks of a lattice, their corners, the
active set decided on the corner values, and the mesh -- mesh_ref.mesh of the dense lattice
restricted to the cells of active bricks, its vertices renumbered by ascending key.  The comparison
convention for an output whose order is fixed but not specified: sort the vertices by their keys,
compare f32 values on uint32 views, map the triangles through the permutation and compare them cell
by cell.  tests/test_sparse_mesh_cpu.py pins what this file gives on the oracle lattices."""
import numpy as np

import mesh_ref

F = np.float32


def brick_counts(dims, B):
    """(nbx, nby, nbz): ceil((dim - 1) / B) bricks an axis"""
    return tuple((d - 1 + B - 1) // B for d in dims)


def default_band(step, B):
    """the brick's diagonal in double, rounded to f32 (Renderer.extract_mesh_sparse's band=None)"""
    return F(np.sqrt(sum((float(B) * float(F(s))) ** 2 for s in step)))


def corner_values(sdf, B):
    """[nbz + 1, nby + 1, nbx + 1]: the values at the lattice points min(B b, dim - 1)"""
    nz, ny, nx = sdf.shape
    ix = [np.minimum(B * np.arange(n + 1), d - 1) for n, d in zip(brick_counts((nx, ny, nz), B), (nx, ny, nz))]
    return np.asarray(sdf, F)[np.ix_(ix[2], ix[1], ix[0])]


def active_bricks(sdf, B, iso, band):
    """bool [nbz, nby, nbx]: a corner is NaN, the corners differ in insideness (s < iso), or the
    smallest |s - iso| (one f32 subtract) of the corners is <= band"""
    c = corner_values(sdf, B)
    iso, band = F(iso), F(band)
    nz, ny, nx = c.shape
    nan = np.zeros((nz - 1, ny - 1, nx - 1), bool)
    near = nan.copy()
    n_in = np.zeros(nan.shape, int)
    with np.errstate(all="ignore"):
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    s = c[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
                    d = np.abs((s - iso).astype(F))
                    nan |= np.isnan(s)
                    near |= d <= band
                    n_in += s < iso
    return nan | near | ((n_in > 0) & (n_in < 8))


def brick_of_cell(cells, dims, B):
    """the linear brick index of each linear cell index (the cell's corner 000)"""
    nx, ny, _ = dims
    nbx, nby, _ = brick_counts(dims, B)
    cells = np.asarray(cells, np.int64)
    i, j, k = cells % nx, (cells // nx) % ny, cells // (nx * ny)
    return ((k // B) * nby + j // B) * nbx + i // B


def crossing_bricks(sdf, B, iso=0.0):
    """bool [nbz, nby, nbx]: the brick holds a cell with a triangle"""
    nz, ny, nx = sdf.shape
    dims = (nx, ny, nz)
    masks = mesh_ref.tet_masks(sdf, iso)
    kk, jj, ii = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    cells = ((kk * ny + jj) * nx + ii).reshape(-1)
    hit = ((masks != 0) & (masks != 15)).any(1)
    nb = brick_counts(dims, B)
    out = np.zeros(nb[0] * nb[1] * nb[2], bool)
    out[brick_of_cell(cells[hit], dims, B)] = True
    return out.reshape(nb[::-1])


def smallest_sound_band(sdf, B, iso=0.0):
    """the smallest band at which every brick that holds a crossing cell is active"""
    c = corner_values(sdf, B)
    nz, ny, nx = c.shape
    d = np.full((nz - 1, ny - 1, nx - 1), np.inf)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                d = np.minimum(d, np.abs((c[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx] - F(iso)).astype(F)))
    need = crossing_bricks(sdf, B, iso) & ~active_bricks(sdf, B, iso, F(0.0))
    return float(d[need].max()) if need.any() else 0.0


def point_set_total(active, dims, B):
    """the sum over the active bricks of their point-set sizes"""
    ext = [np.minimum(B, d - 1 - B * np.arange(n)) + 1 for n, d in zip(brick_counts(dims, B), dims)]
    size = ext[2][:, None, None] * ext[1][None, :, None] * ext[0][None, None, :]
    return int(size[active].sum())


def holding_bricks(keys, dims, B):
    """[n, 8]: the linear indices of the bricks whose point set holds both ends of each edge
    (key = index(o) * 7 + slot), -1 where there are fewer: along an axis the edge does not run, a
    point on the face between two bricks belongs to both"""
    keys = np.asarray(keys, np.int64)
    o, e = keys // 7, mesh_ref.SLOTS[keys % 7]
    idx = np.stack([o % dims[0], (o // dims[0]) % dims[1], o // (dims[0] * dims[1])], -1)
    nb = np.array(brick_counts(dims, B))
    up = np.minimum(idx // B, nb - 1)
    below = (e == 0) & (idx % B == 0) & (idx > 0) & (idx // B < nb)
    out = np.full((len(keys), 8), -1, np.int64)
    for n in range(8):
        bits = np.array([(n >> a) & 1 for a in range(3)])
        ok = (below | (bits == 0)).all(1)
        b = up - bits
        out[ok, n] = ((b[:, 2] * nb[1] + b[:, 1]) * nb[0] + b[:, 0])[ok]
    return out


def restrict(dense, active, dims, B):
    """(V, T, cells, keys) of the dense mesh (mesh_ref.mesh's tuple) restricted to the active bricks:
    the triangles whose cell lies in one, the vertices they name, renumbered by ascending key"""
    V, T, cells, keys = dense[:4]
    keep = active.reshape(-1)[brick_of_cell(cells, dims, B)] if len(cells) else np.zeros(0, bool)
    T, cells = T[keep], cells[keep]
    used = np.zeros(len(V), bool)
    used[T.reshape(-1)] = True
    new = np.cumsum(used) - 1  # (the dense vertices are in ascending key)
    return V[used], new[T].astype(np.int32).reshape(-1, 3), cells, keys[used]


def mesh(sdf, origin, step, B, iso, band):
    """nr_extract_mesh_sparse's mesh in key order: (V, T, cells, keys, active)"""
    dims = sdf.shape[::-1]
    active = active_bricks(sdf, B, iso, band)
    return restrict(mesh_ref.mesh(sdf, origin, step, iso), active, dims, B) + (active,)


def in_key_order(out, dims):
    """The library's output (a dict with vertices, triangles, keys and maybe normals) in the
    reference's order: vertices sorted by key, triangle ids mapped through the permutation and the
    triangles sorted by cell (stable).  Returns (V, T, cells, keys, N or None)."""
    keys = np.asarray(out["keys"], np.int64)
    order = np.argsort(keys, kind="stable")
    rank = np.empty(len(keys), np.int64)
    rank[order] = np.arange(len(keys))
    T = rank[np.asarray(out["triangles"]).reshape(-1, 3)].astype(np.int32).reshape(-1, 3)
    cells = mesh_ref.triangle_cells(T, keys[order], dims) if len(T) else np.zeros(0, np.int64)
    by_cell = np.argsort(cells, kind="stable")
    N = out["normals"][order] if out.get("normals") is not None else None
    return out["vertices"][order], T[by_cell], cells[by_cell], keys[order], N


def assert_same_mesh(got, ref, what):
    """got, ref: (V, T, cells, keys, ...) in key order.  Keys equal, positions bit for bit,
    triangles cell by cell."""
    gV, gT, gc, gk = got[:4]
    rV, rT, rc, rk = ref[:4]
    assert (len(gV), len(gT)) == (len(rV), len(rT)), (what, len(gV), len(gT), len(rV), len(rT))
    assert np.array_equal(gk, rk), f"{what}: keys differ"
    assert len(np.unique(gk)) == len(gk), f"{what}: an edge has two vertices"
    bad = mesh_ref.bits(np.ascontiguousarray(gV)) != mesh_ref.bits(np.ascontiguousarray(rV))
    assert not bad.any(), f"{what}: {int(bad.sum())} vertex coordinates differ"
    a, b = mesh_ref.cell_sets(gT, gc), mesh_ref.cell_sets(rT, rc)
    assert a == b, f"{what}: the triangles of {sum(a.get(c) != b.get(c) for c in set(a) | set(b))} cells differ"
