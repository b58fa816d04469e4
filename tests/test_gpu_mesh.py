"""Volume sampling and isosurface extraction on the GPU (nr_sample_grid, nr_mesh_grid,
nr_extract_mesh; nr_mesh.hip) against tests/mesh_ref.py, the numpy restatement of the header's
definitions over the CPU oracle (pinned by tests/test_mesh_cpu.py).  The sampler runs the fp32 MLP,
whose contract is bit-exactness, and the extraction is a pure function of its inputs: f32 values are
compared on uint32 views, a triangle after rotating it to start at its smallest index, and triangle
lists cell by cell (the order inside a cell is not part of the interface)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cudaneuralrender_amd as nr
import mesh_ref
import oracle
from mesh_ref import bits

pytestmark = pytest.mark.gpu
F = np.float32
FRAME = 3
# the box B around plane_1: 24,679 points = 385 full 64-point chunks and a tail of 39; the inside set
# touches no lattice face, so B's meshes are closed
B_ORIGIN, B_STEP, B_DIMS = (-0.7, -0.8, -0.9), (0.05, 0.055, 0.05), (29, 23, 37)
# the reference's own vertex / triangle counts on B
B_COUNTS = {"tanh": (1876, 3744), "v1": (3564, 7092), "displace": (2000, 3996)}
# where torch bundles a HIP runtime of its own beside libnr's, torch has to open the GPU first
if torch.cuda.is_available():
    torch.cuda.init()


@functools.lru_cache(maxsize=None)
def plane_net(four):
    """plane_1's oracle network; four: with a 4th input row appended to the first kernel (as
    test_gpu_query.plane_net)."""
    dims, K, B = nr.read_keras_h5(nr.geometry_path("plane_1"))
    if four:
        K = [np.concatenate([K[0], np.random.default_rng(4).normal(0, 0.01, (1, 32)).astype(np.float32)], 0)] + K[1:]
        dims = [4] + list(dims[1:])
    return dims, K, B, oracle.OracleNet(K, B)


@functools.lru_cache(maxsize=None)
def ref_grid(scene, four=False, dims=B_DIMS):
    """mesh_ref.sample, computed once per case and shared (never modified)."""
    v = mesh_ref.sample(plane_net(four)[3], B_ORIGIN, B_STEP, dims, scene=nr.NR_SCENE[scene], frame=FRAME)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def ref_mesh(scene):
    """(V, T, cells, keys, normals) of B's reference mesh."""
    V, T, cells, keys = mesh_ref.mesh(ref_grid(scene), B_ORIGIN, B_STEP, 0.0)
    N = mesh_ref.normals(plane_net(False)[3], V, scene=nr.NR_SCENE[scene], frame=FRAME)
    for a in (V, T, cells, keys, N):
        a.setflags(write=False)
    return V, T, cells, keys, N


@pytest.fixture(scope="module")
def rend():
    dims, K, B, _ = plane_net(False)
    r = nr.Renderer(0)
    r.load_mlp(dims, K, B).set_precision("fp32").set_static(nr.NR_COLOR_FACING, 3)
    r.set_view(*nr.camera(0.0, 0.0, 2.0), FRAME)
    yield r
    r.close()


@pytest.fixture(scope="module")
def rend4():
    dims, K, B, _ = plane_net(True)
    r = nr.Renderer(0)
    r.load_mlp(dims, K, B).set_static(nr.NR_COLOR_FACING, 4)
    r.set_view(*nr.camera(0.0, 0.0, 2.0), FRAME)
    yield r
    r.close()


def assert_bits(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype)
    bad = bits(got) != bits(ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def assert_mesh(V, T, ref, dims, what):
    """Vertices bit for bit, triangles cell by cell."""
    rV, rT, cells, keys = ref[:4]
    assert (len(V), len(T)) == (len(rV), len(rT)), (what, len(V), len(T), len(rV), len(rT))
    assert_bits(V, rV, what + " vertices")
    assert T.dtype == np.int32 and T.min(initial=0) >= 0 and T.max(initial=-1) < len(rV)
    got = mesh_ref.cell_sets(T, mesh_ref.triangle_cells(T, keys, dims))
    want = mesh_ref.cell_sets(rT, cells)
    assert got == want, f"{what}: the triangles of {sum(got.get(c) != want.get(c) for c in set(got) | set(want))} cells differ"


GRID_CASES = [("tanh", False, B_DIMS), ("v1", False, B_DIMS), ("displace", False, B_DIMS), ("tanh", True, B_DIMS),
              ("v1", False, (3, 2, 2)), ("v1", False, (65, 1, 1))]


@pytest.mark.parametrize("scene,four,dims", GRID_CASES)
def test_grid_bitexact(rend, rend4, scene, four, dims):
    ref = ref_grid(scene, four, dims)
    n = dims[0] * dims[1] * dims[2]
    assert ref.shape == dims[::-1] and not np.isnan(ref).any()
    if dims == B_DIMS:  # the lattice crosses the (thin) model: both signs occur
        assert min(int((ref < 0).sum()), int((ref > 0).sum())) >= 100
    r = (rend4 if four else rend).set_scene(scene)
    got, st = r.sample_grid(B_ORIGIN, B_STEP, dims, with_stats=True)
    assert_bits(got, ref, f"{scene} host")
    assert st["ray_steps"] == n and st["launches"] == 1
    # the device path, on torch's current stream
    dev = torch.device("cuda:0")
    out = torch.full((n + 64,), -7.0, dtype=torch.float32, device=dev)
    try:
        r.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        dst = r.sample_grid_device(out.data_ptr(), B_ORIGIN, B_STEP, dims, with_stats=True)
        r.synchronize()
    finally:
        r.set_stream(None, own=True)
    host = out.cpu().numpy()
    assert_bits(host[:n].reshape(dims[::-1]), ref, f"{scene} device")
    assert (host[n:] == -7.0).all()  # nothing is written past the lattice
    assert dst["ray_steps"] == n


def test_grid_same_bits_any_grid(rend):
    ref = ref_grid("v1")
    rend.set_scene("v1")
    try:
        one = rend.set_occupancy(1).sample_grid(B_ORIGIN, B_STEP, B_DIMS)
    finally:
        rend.set_occupancy(0)
    assert_bits(one, ref, "one workgroup per CU")
    assert_bits(rend.sample_grid(B_ORIGIN, B_STEP, B_DIMS), ref, "default grid")
    try:
        rend.set_precision("bf16")  # ignored: the sampler always runs the fp32 MLP
        assert_bits(rend.sample_grid(B_ORIGIN, B_STEP, B_DIMS), ref, "bf16 selected")
    finally:
        rend.set_precision("fp32")
    # a smaller lattice with the same origin and steps holds B's first points: the same bits
    sub = rend.sample_grid(B_ORIGIN, B_STEP, (7, 5, 3))
    assert_bits(sub, np.ascontiguousarray(ref[:3, :5, :7]), "a smaller lattice of the same points")


def planted_lattice():
    r = mesh_ref.random_lattice().copy()
    r[0, 0, 0] = np.nan
    r[3, 4, 5] = np.nan
    r[1, 2, 3] = np.inf
    r[2, 2, 2] = -np.inf
    r[0, 4, 5] = -np.inf
    r[1, 1, 1] = 0.25  # exactly iso: outside
    r[2, 3, 4] = 0.25
    return r


@pytest.mark.parametrize("case,iso", [("random", 0.0), ("random", 0.25), ("planted", 0.25), ("no network", 0.0)])
def test_mesh_grid_cases(rend, case, iso):
    sdf = planted_lattice() if case == "planted" else mesh_ref.random_lattice()
    dims = sdf.shape[::-1]
    ref = mesh_ref.mesh(sdf, mesh_ref.RANDOM_ORIGIN, mesh_ref.RANDOM_STEP, iso)
    # the reference covers what the case is about: every cell is active, the surface is open
    assert len(set(ref[2].tolist())) == 60 and not mesh_ref.is_closed_oriented(ref[1])
    if case == "planted":
        assert np.isnan(ref[0]).any() and len(ref[0]) != len(mesh_ref.mesh(mesh_ref.random_lattice(), mesh_ref.RANDOM_ORIGIN,
                                                                            mesh_ref.RANDOM_STEP, iso)[0])
    if case == "no network":
        with nr.Renderer(0) as bare:
            V, T = bare.mesh_grid(sdf, mesh_ref.RANDOM_ORIGIN, mesh_ref.RANDOM_STEP, iso)
    else:
        V, T = rend.mesh_grid(sdf, mesh_ref.RANDOM_ORIGIN, mesh_ref.RANDOM_STEP, iso)
    assert_mesh(V, T, ref, dims, f"{case} iso {iso}")


def test_mesh_grid_many_blocks(rend):
    """A lattice of 14 256-point blocks with a crossing on most edges: the scanned block offsets."""
    sdf = np.random.default_rng(9).uniform(-1, 1, (9, 17, 23)).astype(F)
    ref = mesh_ref.mesh(sdf, (0, 0, 0), (0.1, 0.2, 0.3), 0.1)
    assert len(ref[0]) > 10000
    V, T = rend.mesh_grid(sdf, (0, 0, 0), (0.1, 0.2, 0.3), 0.1)
    assert_mesh(V, T, ref, sdf.shape[::-1], "many blocks")


def test_mesh_grid_scan_steps(rend):
    """291,200 points are 1,138 blocks: the scan of the block totals takes two 1,024-block steps,
    and vertices lie on both sides of the step (a gyroid fills the lattice)."""
    dims = (70, 64, 65)
    w = 0.12
    z, y, x = np.meshgrid(np.arange(dims[2]) * w, np.arange(dims[1]) * w, np.arange(dims[0]) * w, indexing="ij")
    sdf = (np.sin(x) * np.cos(y) + np.sin(y) * np.cos(z) + np.sin(z) * np.cos(x)).astype(F)
    ref = mesh_ref.mesh(sdf, (0, 0, 0), (0.1, 0.1, 0.1), 0.3)
    blocks = ref[3] // 7 // 256
    assert (blocks < 1024).sum() > 1000 and (blocks >= 1024).sum() > 1000
    V, T = rend.mesh_grid(sdf, (0, 0, 0), (0.1, 0.1, 0.1), 0.3)
    assert_mesh(V, T, ref, dims, "two scan steps")


@pytest.mark.parametrize("scene", ["tanh", "v1", "displace"])
def test_extract_mesh_plane(rend, scene):
    ref = ref_mesh(scene)
    rV, rT, cells, keys, rN = ref
    # the reference's own counts, and its mesh is a closed oriented manifold with finite normals
    assert (len(rV), len(rT)) == B_COUNTS[scene]
    assert mesh_ref.is_closed_oriented(rT) and not np.isnan(rN).any()
    out, st = rend.set_scene(scene).extract_mesh(B_ORIGIN, B_STEP, B_DIMS, with_stats=True)
    assert_mesh(out["vertices"], out["triangles"], ref, B_DIMS, scene)
    assert_bits(out["normals"], rN, scene + " normals")
    assert mesh_ref.is_closed_oriented(out["triangles"])
    assert not np.isnan(out["normals"]).any()
    n = B_DIMS[0] * B_DIMS[1] * B_DIMS[2]
    assert (st["ray_steps"], st["rays_shaded"], st["shade_evals"]) == (n, len(rV), 4 * len(rV))
    bare, bst = rend.extract_mesh(B_ORIGIN, B_STEP, B_DIMS, normals=False, with_stats=True)
    assert "normals" not in bare and bst["shade_evals"] == 0 and bst["rays_shaded"] == len(rV)
    assert_mesh(bare["vertices"], bare["triangles"], ref, B_DIMS, scene + " without normals")


def _lat(origin, step, dims):
    o, s, d = np.asarray(origin, F), np.asarray(step, F), np.asarray(dims, np.int32)
    IP = ctypes.POINTER(ctypes.c_int)
    return o, s, d, (nr.renderer._fptr(o), nr.renderer._fptr(s), d.ctypes.data_as(IP))


def test_capacity_protocol(rend):
    L = nr.lib()
    sdf = mesh_ref.random_lattice()
    ref = mesh_ref.mesh(sdf, mesh_ref.RANDOM_ORIGIN, mesh_ref.RANDOM_STEP, 0.0)
    NV, NT = len(ref[0]), len(ref[1])
    o, s, d, lat = _lat(mesh_ref.RANDOM_ORIGIN, mesh_ref.RANDOM_STEP, sdf.shape[::-1])

    def call(V, vcap, T, tcap):
        nv, nt = ctypes.c_long(-1), ctypes.c_long(-1)
        rc = L.nr_mesh_grid(rend._ctx, sdf.ctypes.data, *lat, 0.0, None if V is None else V.ctypes.data, vcap,
                            None if T is None else T.ctypes.data, tcap, ctypes.byref(nv), ctypes.byref(nt), 0)
        return rc, nv.value, nt.value

    assert call(None, 0, None, 0) == (0, NV, NT)  # count only
    for vcap, tcap in ((NV - 1, NT), (NV, NT - 1)):
        V, T = np.full((NV, 3), -5.0, F), np.full((NT, 3), -5, np.int32)
        assert call(V, vcap, T, tcap) == (-6, NV, NT)  # NR_E_NOMEM, the counts set
        assert (V == -5.0).all() and (T == -5).all()  # nothing written
    V, T = np.full((NV + 2, 3), -5.0, F), np.full((NT + 2, 3), -5, np.int32)
    assert call(V, NV, T, NT) == (0, NV, NT)  # exact capacities
    assert (V[NV:] == -5.0).all() and (T[NT:] == -5).all()
    assert_mesh(V[:NV], T[:NT], ref, sdf.shape[::-1], "exact capacities")
    assert call(V, NV, None, 0)[0] == -1  # vertices without triangles
    # nr_extract_mesh follows the same protocol
    rend.set_scene("tanh")
    _, _, _, blat = _lat(B_ORIGIN, B_STEP, B_DIMS)
    nv, nt = ctypes.c_long(-1), ctypes.c_long(-1)
    assert L.nr_extract_mesh(rend._ctx, *blat, 0.0, None, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt), 0, None) == 0
    assert (nv.value, nt.value) == B_COUNTS["tanh"]
    V, N, T = (np.full((nv.value, 3), -5.0, F), np.full((nv.value, 3), -5.0, F), np.full((nt.value, 3), -5, np.int32))
    assert L.nr_extract_mesh(rend._ctx, *blat, 0.0, V.ctypes.data, N.ctypes.data, nv.value - 1, T.ctypes.data, nt.value,
                             ctypes.byref(nv), ctypes.byref(nt), 0, None) == -6
    assert (V == -5.0).all() and (N == -5.0).all() and (T == -5).all()


def test_errors(rend):
    L = nr.lib()
    buf = np.zeros(64, F)
    nv, nt = ctypes.c_long(0), ctypes.c_long(0)
    o, s = np.zeros(3, F), np.ones(3, F)
    fo, fs = nr.renderer._fptr(o), nr.renderer._fptr(s)

    def dims(*v):
        a = np.asarray(v, np.int32)
        return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))

    def sample(r, d, out=buf.ctypes.data, origin=fo):
        return L.nr_sample_grid(r._ctx, origin, fs, d, out, 0, None)

    def mesh(r, d, sdf=buf.ctypes.data, pnv=ctypes.byref(nv)):
        return L.nr_mesh_grid(r._ctx, sdf, fo, fs, d, 0.0, None, 0, None, 0, pnv, ctypes.byref(nt), 0)

    def extract(r, d):
        return L.nr_extract_mesh(r._ctx, fo, fs, d, 0.0, None, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt), 0, None)

    _, d222 = dims(2, 2, 2)
    with nr.Renderer(0) as r:
        assert sample(r, d222) == -5 and extract(r, d222) == -5  # NR_E_STATE: no network
        rng = np.random.default_rng(0)
        r.load_mlp([3, 16, 1], [rng.normal(size=(3, 16)).astype(F), rng.normal(size=(16, 1)).astype(F)],
                   [np.zeros(16, F), np.zeros(1, F)])
        assert sample(r, d222) == -4 and extract(r, d222) == -4  # NR_E_FORMAT: not a network of the fused kernels
    keep = []
    for bad in ((0, 2, 2), (2, 0, 2), (2, 2, 0)):
        keep.append(dims(*bad))
        assert sample(rend, keep[-1][1]) == -1  # a dim of 0
    for bad in ((1, 2, 2), (2, 1, 2), (2, 2, 1)):
        keep.append(dims(*bad))
        assert mesh(rend, keep[-1][1]) == -1 and extract(rend, keep[-1][1]) == -1  # a dim of 1
    keep.append(dims(2 ** 15, 2 ** 15, 2))  # 2^31 points
    assert sample(rend, keep[-1][1]) == -1 and mesh(rend, keep[-1][1]) == -1
    keep.append(dims(2 ** 30 + 1, 1, 1))  # 2^30 + 1 points
    assert sample(rend, keep[-1][1]) == -1
    keep.append(dims(2 ** 29 + 1, 2, 1))
    assert sample(rend, keep[-1][1]) == -1
    keep.append(dims(2 ** 28 + 1, 2, 2))  # 2^30 + 4 points
    assert mesh(rend, keep[-1][1]) == -1 and extract(rend, keep[-1][1]) == -1
    # NULL arguments
    assert sample(rend, d222, out=None) == -1 and sample(rend, d222, origin=None) == -1 and sample(rend, None) == -1
    assert mesh(rend, d222, sdf=None) == -1 and mesh(rend, d222, pnv=None) == -1 and mesh(rend, None) == -1
    assert L.nr_sample_grid(None, fo, fs, d222, buf.ctypes.data, 0, None) == -1
    assert L.nr_mesh_grid(None, buf.ctypes.data, fo, fs, d222, 0.0, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt), 0) == -1
    # a lattice without a crossing is an empty mesh, not an error
    V, T = rend.mesh_grid(np.ones((2, 2, 2), F), (0, 0, 0), (1, 1, 1))
    assert V.shape == (0, 3) and T.shape == (0, 3)


def test_deterministic(rend):
    rend.set_scene("v1")
    a = rend.extract_mesh(B_ORIGIN, B_STEP, B_DIMS)
    b = rend.extract_mesh(B_ORIGIN, B_STEP, B_DIMS)
    for k in ("vertices", "normals", "triangles"):
        assert a[k].tobytes() == b[k].tobytes(), k
    # device buffers (loc applies to every pointer) hold the same bytes
    L = nr.lib()
    nv, nt = a["vertices"].shape[0], a["triangles"].shape[0]
    dev = torch.device("cuda:0")
    V = torch.full((nv + 1, 3), -7.0, dtype=torch.float32, device=dev)
    N = torch.full((nv + 1, 3), -7.0, dtype=torch.float32, device=dev)
    T = torch.full((nt + 1, 3), -7, dtype=torch.int32, device=dev)
    _, _, _, lat = _lat(B_ORIGIN, B_STEP, B_DIMS)
    cv, ct = ctypes.c_long(0), ctypes.c_long(0)
    try:
        rend.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        rc = L.nr_extract_mesh(rend._ctx, *lat, 0.0, ctypes.c_void_p(V.data_ptr()), ctypes.c_void_p(N.data_ptr()), nv,
                               ctypes.c_void_p(T.data_ptr()), nt, ctypes.byref(cv), ctypes.byref(ct), 1, None)
        rend.synchronize()
    finally:
        rend.set_stream(None, own=True)
    assert rc == 0 and (cv.value, ct.value) == (nv, nt)
    for k, t in (("vertices", V), ("normals", N), ("triangles", T)):
        h = t.cpu().numpy()
        assert h[:-1].tobytes() == a[k].tobytes(), k
        assert (h[-1] == -7).all(), k
