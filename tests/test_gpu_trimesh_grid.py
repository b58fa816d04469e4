"""A triangle mesh's lattice calls on the GPU (nr_mesh_sample_grid, nr_mesh_remesh,
nr_mesh_remesh_sparse; nr_trimesh_grid.hip) against tests/trimesh_grid_ref.py, which composes the
existing numpy references.  The contract is bit-exactness: a lattice value is what the point calls
return for that point, whichever wave evaluates it, and the meshes are nr_mesh_grid's of those values --
f32 values are compared on uint32 views, triangles cell by cell."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cudaneuralrender_amd as nr
import mesh_ref
import sparse_mesh_ref as SR
import trimesh_grid_ref as G
import trimesh_ref as R
from mesh_ref import bits

pytestmark = pytest.mark.gpu
F = np.float32
IP = ctypes.POINTER(ctypes.c_int)
QNAN_BITS = 0x7fc00000
if torch.cuda.is_available():
    torch.cuda.init()

SMALL = (13, 10, 7)   # ragged against the 4 x 4 x 4 blocks on every axis: 4 x 3 x 2 blocks
GROW = (0.21, 0.17)   # the small lattices: the bound grown by these below / above
CLOSED = ("tetrahedron", "cube", "torus")


@pytest.fixture(scope="module")
def owner():
    with nr.Renderer(0) as r:
        yield r


def assert_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = bits(got) != bits(ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def assert_mesh(V, T, ref, dims, what):
    """vertices bit for bit and in order, triangles cell by cell (as tests/test_gpu_mesh.py)"""
    rV, rT, cells, keys = ref[:4]
    assert (len(V), len(T)) == (len(rV), len(rT)), (what, len(V), len(T), len(rV), len(rT))
    assert_bits(V, rV, what + " vertices")
    assert T.dtype == np.int32 and T.min(initial=0) >= 0 and T.max(initial=-1) < len(rV)
    got = mesh_ref.cell_sets(T, mesh_ref.triangle_cells(T, keys, dims))
    want = mesh_ref.cell_sets(rT, cells)
    assert got == want, f"{what}: the triangles of {sum(got.get(c) != want.get(c) for c in set(got) | set(want))} cells differ"


@functools.lru_cache(maxsize=None)
def small_lattice(name, dims=SMALL):
    return G.bound_lattice(G.mesh(name)[0], dims, *GROW)


@functools.lru_cache(maxsize=None)
def tree(name, leaf=8):
    out = nr.trimesh_hierarchy(*G.mesh(name), leaf=leaf)
    for a in out[:3]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def small_ref(name, sign, brute=False, dims=SMALL):
    """trimesh_grid_ref.values of the small lattice, computed once and shared (read-only)"""
    V, T = G.mesh(name)
    origin, step = small_lattice(name, dims)
    if sign == "winding":
        v = G.values(V, T, origin, step, dims, sign, 2.0, tree(name), brute, normal=small_ref(name, "normal", dims=dims))
    else:
        v = G.values(V, T, origin, step, dims, sign)
    v.setflags(write=False)
    return v


# ---- values ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["tetrahedron", "cube", "torus", "degenerate_torus"])
def test_values_bit_exact(owner, name):
    V, T = G.mesh(name)
    origin, step = small_lattice(name)
    n = SMALL[0] * SMALL[1] * SMALL[2]
    ref = small_ref(name, "normal")
    assert (ref < 0).any() and (ref > 0).any()
    for leaf in (1, 8, 32):
        with nr.TriMesh(owner, V, T, leaf=leaf) as m:
            out, st = m.sample_grid(origin, step, SMALL, with_stats=True)
            assert out.shape == SMALL[::-1] and out.dtype == F
            assert_bits(out, ref, f"{name} leaf {leaf}")
            assert st["ray_steps"] == n and 0 < st["shade_evals"] <= n * len(T) and st["launches"] == 2 and st["ms_total"] > 0
            if leaf != 8:
                continue
            out, st = m.sample_grid(origin, step, SMALL, brute=True, with_stats=True)
            assert_bits(out, ref, f"{name} brute")
            assert st["shade_evals"] == n * len(tree(name)[1])  # the live triangles
            # the winding sign: beta 2 through the library's tree (beta = 0 is 2.0), and every triangle
            wref = small_ref(name, "winding")
            out, st = m.sample_grid(origin, step, SMALL, sign="winding", beta=2.0, with_stats=True)
            assert_bits(out, wref, f"{name} winding")
            assert st["launches"] == 3 and st["ray_steps"] == n
            assert_bits(m.sample_grid(origin, step, SMALL, sign="winding"), wref, f"{name} winding, beta 0")
            assert_bits(m.sample_grid(origin, step, SMALL, sign="winding", brute=True), small_ref(name, "winding", True),
                        f"{name} winding brute")
            # and it is the point calls' value at the lattice's points
            P = mesh_ref.lattice(origin, step, SMALL)
            assert_bits(out.reshape(-1), m.winding(P, beta=2.0, sdf=True)["sdf"], f"{name} against nr_mesh_winding")
            assert_bits(ref.reshape(-1), m.distance(P)["sdf"], f"{name} against nr_trimesh_distance")


@pytest.mark.parametrize("dims", [(1, 1, 1), (3, 1, 2), (4, 4, 4), (5, 4, 4)])
def test_block_shapes(owner, dims):
    """one point; less than a block; exactly one block; one full block and one a lane thin"""
    V, T = G.mesh("cube")
    origin, step = (-0.31, -0.2, -0.42), (0.19, 0.23, 0.27)  # straddles the cube's faces at every size
    with nr.TriMesh(owner, V, T) as m:
        for sign in ("normal", "winding"):
            ref = G.values(V, T, origin, step, dims, sign, 2.0, tree("cube"))
            assert_bits(m.sample_grid(origin, step, dims, sign=sign), ref, f"{dims} {sign}")


def test_grid_stride_second_trip(owner):
    """more blocks than the launch has waves: 24 x 24 x 16 = 9,216 blocks against at most 8 workgroups of
    4 waves on each of 256 CUs"""
    dims = (96, 96, 64)
    V, T = G.mesh("cube")
    origin, step = G.bound_lattice(V, dims, 0.3, 0.2)
    assert (dims[0] // 4) * (dims[1] // 4) * (dims[2] // 4) > 256 * 8 * 4
    P = mesh_ref.lattice(origin, step, dims)
    with nr.TriMesh(owner, V, T) as m:
        got = m.sample_grid(origin, step, dims)
        assert_bits(got.reshape(-1), m.distance(P)["sdf"], "96 x 96 x 64")


def test_overflowing_step(owner):
    """step[0] = 3e38: column 2's coordinate overflows: the quiet NaN, kept; remesh follows nr_mesh_grid's NaN rule"""
    dims = (3, 2, 2)
    V, T = G.mesh("cube")
    origin, step = (-0.2, -0.1, -0.1), (3e38, 0.3, 0.3)
    with np.errstate(all="ignore"):
        ref = G.values(V, T, origin, step, dims)
    with nr.TriMesh(owner, V, T) as m:
        for sign in ("normal", "winding"):
            got = m.sample_grid(origin, step, dims, sign=sign)
            assert (bits(got)[:, :, 2] == QNAN_BITS).all(), got
            # column 0 is ordinary; column 1 lies 3e38 away, where the squares overflow too: the same
            # infinities, and where the arithmetic gives a NaN, a NaN (its sign and payload are the machine's)
            assert np.isfinite(got[:, :, 0]).all()
            assert_bits(np.abs(got[:, :, 0]), np.abs(ref[:, :, 0]), f"overflow {sign}")
            assert np.array_equal(np.isnan(got), np.isnan(ref))
            assert_bits(np.abs(np.nan_to_num(got, nan=0.0)), np.abs(np.nan_to_num(ref, nan=0.0)), f"overflow {sign}")
        got = m.sample_grid(origin, step, dims)
        out = m.remesh(origin, step, dims)
        gV, gT = owner.mesh_grid(got, origin, step)
        assert_bits(out["vertices"], gV, "overflow remesh")
        assert np.array_equal(out["triangles"], gT)
        with np.errstate(all="ignore"):
            ref_mesh = G.remesh(got, origin, step)
        assert_mesh(out["vertices"], out["triangles"], ref_mesh, dims, "overflow remesh")


# ---- remesh ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, sign, iso", [("cube", "normal", 0.0), ("torus", "normal", 0.05), ("tetrahedron", "winding", 0.0),
                                             ("torus", "winding", -0.03)])
def test_remesh(owner, name, sign, iso):
    V, T = G.mesh(name)
    origin, step = small_lattice(name)
    ref = G.remesh(small_ref(name, sign), origin, step, iso)
    assert len(ref[0]) > 50
    with nr.TriMesh(owner, V, T) as m:
        out, st = m.remesh(origin, step, SMALL, iso=iso, sign=sign, beta=2.0, with_stats=True)
        assert list(out) == ["vertices", "triangles", "source_tri"]
        assert_mesh(out["vertices"], out["triangles"], ref, SMALL, f"{name} {sign}")
        # nr_mesh_grid of the sampled values, in order as well
        gV, gT = owner.mesh_grid(m.sample_grid(origin, step, SMALL, sign=sign, beta=2.0), origin, step, iso=iso)
        assert_bits(out["vertices"], gV, "against nr_mesh_grid")
        assert np.array_equal(out["triangles"], gT)
        # source_tri: nr_trimesh_distance's tri at the vertices
        assert out["source_tri"].dtype == np.int32
        assert np.array_equal(out["source_tri"], m.distance(out["vertices"], tri=True)["tri"])
        assert out["source_tri"].min() >= 0 and out["source_tri"].max() < len(T)
        n = SMALL[0] * SMALL[1] * SMALL[2]
        assert (st["ray_steps"], st["rays_shaded"]) == (n, len(ref[0])) and st["shade_evals"] > 0 and st["ms_total"] > 0
        bare = m.remesh(origin, step, SMALL, iso=iso, sign=sign, beta=2.0, source_tri=False)
        assert list(bare) == ["vertices", "triangles"]
        assert bare["vertices"].tobytes() == out["vertices"].tobytes() and bare["triangles"].tobytes() == out["triangles"].tobytes()
        assert mesh_ref.is_closed_oriented(out["triangles"])


def _lat(origin, step, dims):
    o, s = np.asarray(origin, F), np.asarray(step, F)
    d = np.asarray(dims, np.int32)
    return o, s, d, (nr.renderer._fptr(o), nr.renderer._fptr(s), d.ctypes.data_as(IP))


def test_capacity_protocol(owner):
    """the counting call and short capacities behave as nr_mesh_grid's"""
    L = nr.lib()
    V0, T0 = G.mesh("cube")
    origin, step = small_lattice("cube")
    ref = G.remesh(small_ref("cube", "normal"), origin, step)
    NV, NT = len(ref[0]), len(ref[1])
    o, s, d, lat = _lat(origin, step, SMALL)
    with nr.TriMesh(owner, V0, T0) as m:
        def call(V, S, vcap, T, tcap):
            nv, nt = ctypes.c_long(-1), ctypes.c_long(-1)
            rc = L.nr_mesh_remesh(m._m, *lat, 0.0, 0, 0.0, None if V is None else V.ctypes.data,
                                     None if S is None else S.ctypes.data, vcap, None if T is None else T.ctypes.data, tcap,
                                     ctypes.byref(nv), ctypes.byref(nt), 0, None)
            return rc, nv.value, nt.value

        assert call(None, None, 0, None, 0) == (0, NV, NT)  # count only
        for vcap, tcap in ((NV - 1, NT), (NV, NT - 1)):
            V, S, T = np.full((NV, 3), -5.0, F), np.full(NV, -5, np.int32), np.full((NT, 3), -5, np.int32)
            assert call(V, S, vcap, T, tcap) == (-6, NV, NT)  # NR_E_NOMEM, the counts set
            assert b"capacities" in L.nr_last_error(owner._ctx)
            assert (V == -5.0).all() and (S == -5).all() and (T == -5).all()  # nothing written
        V, S, T = np.full((NV + 2, 3), -5.0, F), np.full(NV + 2, -5, np.int32), np.full((NT + 2, 3), -5, np.int32)
        assert call(V, S, NV, T, NT) == (0, NV, NT)  # exact capacities
        assert (V[NV:] == -5.0).all() and (S[NV:] == -5).all() and (T[NT:] == -5).all()
        assert_mesh(V[:NV], T[:NT], ref, SMALL, "exact capacities")
        assert call(V, None, NV, None, 0)[0] == -1  # vertices without triangles
        # a lattice without a crossing is an empty mesh, not an error
        out = m.remesh((2.0, 2.0, 2.0), (0.1, 0.1, 0.1), (3, 3, 3))
        assert out["vertices"].shape == (0, 3) and out["triangles"].shape == (0, 3) and out["source_tri"].shape == (0,)


@pytest.mark.parametrize("name", CLOSED)
@pytest.mark.parametrize("iso", [0.0, 0.05])
def test_vertices_lie_near_the_level(owner, name, iso):
    """A vertex lies on a lattice edge whose ends straddle the level, so some point of the edge has the
    distance iso exactly (the signed distance to a closed mesh is continuous); the vertex is within one
    edge -- at most a cell diagonal -- of it, and the distance is 1-Lipschitz: |d(v) - iso| <= the cell
    diagonal.  The bound asserted, twice that, leaves the f32 rounding of d and of the vertex far behind."""
    V, T = G.mesh(name)
    origin, step = small_lattice(name)
    diag = float(np.sqrt(sum(float(x) ** 2 for x in step)))
    with nr.TriMesh(owner, V, T) as m:
        out = m.remesh(origin, step, SMALL, iso=iso)
        assert len(out["vertices"]) > 50
        d = m.distance(out["vertices"])["sdf"]
        err = float(np.abs(d.astype(np.float64) - iso).max())
        print(f"{name} iso {iso}: max |d(v) - iso| = {err:.4g}, cell diagonal {diag:.4g}")
        assert err <= 2 * diag


# ---- remesh_sparse -----------------------------------------------------------------------------------

SIGN_OF = G.SPARSE_CASES


@functools.lru_cache(maxsize=None)
def repair_lattice(name):
    return G.bound_lattice(G.mesh(name)[0], G.REPAIR_DIMS)


def _gpu_dense(m, name, iso):
    """the GPU's own dense values and the reference's dense mesh of them"""
    origin, step = repair_lattice(name)
    sdf = m.sample_grid(origin, step, G.REPAIR_DIMS, sign=SIGN_OF[name])
    return sdf, mesh_ref.mesh(sdf, origin, step, iso)


def _assert_sparse(out, st, sdf, dense, name, B, iso, band, what):
    dims = G.REPAIR_DIMS
    active = SR.active_bricks(sdf, B, iso, band)
    ref = SR.restrict(dense, active, dims, B)
    got = SR.in_key_order(out, dims)
    SR.assert_same_mesh(got, ref, what)
    assert out["active_bricks"] == int(active.sum()), (what, out["active_bricks"], int(active.sum()))
    nb = SR.brick_counts(dims, B)
    steps = (nb[0] + 1) * (nb[1] + 1) * (nb[2] + 1) + SR.point_set_total(active, dims, B)
    assert (st["ray_steps"], st["rays_hit"], st["rays_shaded"]) == (steps, int(active.sum()), len(ref[0])), (what, st)
    assert st["shade_evals"] > 0 and st["launches"] >= 4 and st["ms_total"] > 0
    return got, active


@pytest.mark.parametrize("iso", G.SPARSE_ISOS)
@pytest.mark.parametrize("name", list(G.SPARSE_CASES))
def test_remesh_sparse(owner, name, iso):
    V, T = G.mesh(name)
    origin, step = repair_lattice(name)
    dims = G.REPAIR_DIMS
    sign = SIGN_OF[name]
    with nr.TriMesh(owner, V, T) as m:
        sdf, dense = _gpu_dense(m, name, iso)
        default = SR.default_band(step, 4)
        for band in (None, 0.0, np.inf):
            out, st = m.remesh_sparse(origin, step, dims, iso=iso, sign=sign, brick=4, band=band, with_stats=True)
            assert list(out) == ["vertices", "triangles", "active_bricks", "source_tri", "keys"]
            got, active = _assert_sparse(out, st, sdf, dense, name, 4, iso, default if band is None else F(band), f"{name} band {band}")
            if band is None:
                # the default band culls and is sound: the dense remesh, sorted by key, closed
                assert 1 <= active.sum() <= 0.75 * active.size
                full = m.remesh(origin, step, dims, iso=iso, sign=sign)
                assert_bits(got[0], full["vertices"], "sparse against dense")
                dcells = mesh_ref.triangle_cells(full["triangles"], got[3], dims)
                assert mesh_ref.cell_sets(got[1], got[2]) == mesh_ref.cell_sets(full["triangles"], dcells)
                assert mesh_ref.is_closed_oriented(out["triangles"])
                order = np.argsort(out["keys"], kind="stable")
                assert np.array_equal(out["source_tri"][order], full["source_tri"])
            if band == np.inf:
                assert active.all()
        if iso == 0.0:  # larger bricks, ragged last ones (44, 40, 36 cells): equality only
            for B in (8, 16):
                out, st = m.remesh_sparse(origin, step, dims, iso=iso, sign=sign, brick=B, with_stats=True)
                _assert_sparse(out, st, sdf, dense, name, B, iso, SR.default_band(step, B), f"{name} brick {B}")


# ---- repair ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["open_cube", "open_torus", "double_cube"])
def test_repair(owner, name):
    """an open mesh, and one that cuts through itself, come back closed with the winding sign"""
    V, T = G.mesh(name)
    origin, step = repair_lattice(name)
    with nr.TriMesh(owner, V, T) as m:
        if name != "double_cube":
            assert not m.info()["closed"]
        out = m.remesh(origin, step, G.REPAIR_DIMS, sign="winding")
        assert len(out["triangles"]) > 1000 and mesh_ref.is_closed_oriented(out["triangles"])
        with nr.TriMesh(owner, out["vertices"], out["triangles"]) as fixed:
            assert fixed.info()["closed"]
        if name == "open_cube":  # as many vertices and triangles as the closed cube's remesh
            with nr.TriMesh(owner, *G.mesh("cube")) as c:
                whole = c.remesh(origin, step, G.REPAIR_DIMS)
            assert (len(out["vertices"]), len(out["triangles"])) == (len(whole["vertices"]), len(whole["triangles"])) == (2594, 5184)
            assert not mesh_ref.is_closed_oriented(m.remesh(origin, step, G.REPAIR_DIMS)["triangles"])


# ---- errors and pointers -----------------------------------------------------------------------------

def test_errors(owner):
    L = nr.lib()
    buf = np.zeros(64, F)
    nv, nt, na = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(0)
    o, s = np.zeros(3, F), np.ones(3, F)
    fo, fs = nr.renderer._fptr(o), nr.renderer._fptr(s)
    keep = []

    def dims(*v):
        a = np.asarray(v, np.int32)
        keep.append(a)
        return a.ctypes.data_as(IP)

    d222 = dims(2, 2, 2)
    V, T = G.mesh("cube")
    with nr.TriMesh(owner, V, T) as m:
        def sample(d=d222, sign=0, beta=0.0, flags=0, out=buf.ctypes.data, origin=fo, mesh=m._m):
            return L.nr_mesh_sample_grid(mesh, origin, fs, d, sign, beta, flags, out, 0, None)

        def remesh(d=d222, sign=0, beta=0.0, pnv=ctypes.byref(nv), mesh=m._m, origin=fo):
            return L.nr_mesh_remesh(mesh, origin, fs, d, 0.0, sign, beta, None, None, 0, None, 0, pnv, ctypes.byref(nt), 0, None)

        def sparse(d=d222, sign=0, beta=0.0, brick=4, band=0.5, iso=0.0, pnv=ctypes.byref(nv), mesh=m._m, origin=fo,
                   vertices=None, source=None, keys=None, triangles=None):
            return L.nr_mesh_remesh_sparse(mesh, origin, fs, d, iso, sign, beta, brick, band, vertices, source, keys, 0,
                                              triangles, 0, pnv, ctypes.byref(nt), ctypes.byref(na), 0, None)

        def invalid(rc, word):
            assert rc == -1, (rc, word)
            msg = L.nr_last_error(owner._ctx)
            assert msg and word.encode() in msg, (word, msg)

        assert sample() == 0 and remesh() == 0 and sparse() == 0
        # the lattice: nr_sample_grid's, nr_extract_mesh's and nr_extract_mesh_sparse's errors
        for bad in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
            invalid(sample(d=dims(*bad)), "dims")
        assert sample(d=dims(1, 1, 1)) == 0
        for bad in ((1, 2, 2), (2, 1, 2), (2, 2, 1)):
            invalid(remesh(d=dims(*bad)), "dims")
            invalid(sparse(d=dims(*bad)), "dims")
        invalid(sample(d=dims(2 ** 30 + 1, 1, 1)), "2^30")
        invalid(sample(d=dims(2 ** 15, 2 ** 15, 2)), "2^30")
        invalid(remesh(d=dims(2 ** 28 + 1, 2, 2)), "2^30")
        invalid(sparse(d=dims(65537, 2, 2)), "dims")
        invalid(sample(out=None), "sdf")
        invalid(sample(origin=None), "NULL")
        invalid(sample(d=None), "NULL")
        invalid(remesh(pnv=None), "NULL")
        invalid(remesh(origin=None), "NULL")
        invalid(sparse(pnv=None), "NULL")
        invalid(sparse(origin=None), "NULL")
        invalid(sparse(brick=5), "brick")
        invalid(sparse(band=-1.0), "band")
        invalid(sparse(band=float("nan")), "band")
        invalid(sparse(iso=float("inf")), "iso")
        invalid(sparse(vertices=buf.ctypes.data), "together")
        invalid(sparse(source=buf.ctypes.data), "source_tri")
        invalid(sparse(keys=buf.ctypes.data), "keys")
        # sign, beta and flags: nr_mesh_fit_samples' and nr_mesh_winding's errors
        for f in (sample, remesh, sparse):
            invalid(f(sign=2), "sign")
            invalid(f(sign=-1), "sign")
            invalid(f(beta=-1.0), "beta")
            invalid(f(beta=float("nan")), "beta")
            invalid(f(beta=float("inf")), "beta")
        invalid(sample(flags=2), "flag")
        # a NULL mesh: recorded without a context
        for f, fn in ((sample, "nr_mesh_sample_grid"), (remesh, "nr_mesh_remesh"), (sparse, "nr_mesh_remesh_sparse")):
            assert f(mesh=None) == -1
            assert fn.encode() in L.nr_last_error(None)


def test_device_and_host_pointers(owner):
    V, T = G.mesh("torus")
    origin, step = small_lattice("torus")
    n = SMALL[0] * SMALL[1] * SMALL[2]
    dev = torch.device("cuda:0")
    with nr.TriMesh(owner, V, T) as m:
        for sign in ("normal", "winding"):
            host = m.sample_grid(origin, step, SMALL, sign=sign)
            sdf = torch.full((n + 8,), 7.0, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            st = m.sample_grid_device(sdf.data_ptr(), origin, step, SMALL, sign=sign, with_stats=True)
            assert st["ray_steps"] == n
            got = sdf.cpu().numpy()
            assert got[:n].tobytes() == host.tobytes() and (got[n:] == 7.0).all()
            # remesh
            ref = m.remesh(origin, step, SMALL, sign=sign, iso=0.02)
            NV, NT = len(ref["vertices"]), len(ref["triangles"])
            dV = torch.full((NV + 1, 3), -7.0, dtype=torch.float32, device=dev)
            dS = torch.full((NV + 1,), -7, dtype=torch.int32, device=dev)
            dT = torch.full((NT + 1, 3), -7, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            assert m.remesh_device(origin, step, SMALL, None, 0, None, 0, sign=sign, iso=0.02) == (NV, NT)
            assert m.remesh_device(origin, step, SMALL, dV.data_ptr(), NV, dT.data_ptr(), NT, sign=sign, iso=0.02,
                                   source_tri_ptr=dS.data_ptr()) == (NV, NT)
            owner.synchronize()
            assert dV.cpu().numpy()[:NV].tobytes() == ref["vertices"].tobytes() and (dV[NV:] == -7.0).all()
            assert dS.cpu().numpy()[:NV].tobytes() == ref["source_tri"].tobytes() and (dS[NV:] == -7).all()
            assert dT.cpu().numpy()[:NT].tobytes() == ref["triangles"].tobytes() and (dT[NT:] == -7).all()
            with pytest.raises(nr.NRError):
                m.remesh_device(origin, step, SMALL, dV.data_ptr(), NV - 1, dT.data_ptr(), NT, sign=sign, iso=0.02)
            # remesh_sparse (bricks of 4 on 12 x 9 x 6 cells: ragged)
            sref = m.remesh_sparse(origin, step, SMALL, sign=sign, iso=0.02, brick=4)
            NV, NT = len(sref["vertices"]), len(sref["triangles"])
            dV.fill_(-7.0); dS.fill_(-7); dT.fill_(-7)
            dK = torch.full((NV + 1,), -7, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            res = m.remesh_sparse_device(origin, step, SMALL, dV.data_ptr(), NV, dT.data_ptr(), NT, sign=sign, iso=0.02, brick=4,
                                         source_tri_ptr=dS.data_ptr(), keys_ptr=dK.data_ptr())
            owner.synchronize()
            assert res == (NV, NT, sref["active_bricks"])
            assert dV.cpu().numpy()[:NV].tobytes() == sref["vertices"].tobytes() and (dV[NV:] == -7.0).all()
            assert dS.cpu().numpy()[:NV].tobytes() == sref["source_tri"].tobytes()
            assert dK.cpu().numpy()[:NV].tobytes() == sref["keys"].tobytes() and (dK[NV:] == -7).all()
            assert dT.cpu().numpy()[:NT].tobytes() == sref["triangles"].tobytes() and (dT[NT:] == -7).all()
