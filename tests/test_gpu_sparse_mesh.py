"""Brick-sparse isosurface extraction on the GPU (nr_extract_mesh_sparse; nr_sparse.hip) against
tests/sparse_mesh_ref.py: the dense reference mesh of the CPU oracle's lattice restricted to the
active bricks (pinned by tests/test_sparse_mesh_cpu.py).  The output's order is fixed but not
specified, so the vertices are sorted by their keys first; then positions and normals are compared
on uint32 views and the triangles cell by cell, as tests/test_gpu_mesh.py compares the dense mesh."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cudaneuralrender_amd as nr
import mesh_ref
import oracle
import query_ref
import sparse_mesh_ref as sref
from mesh_ref import bits

pytestmark = pytest.mark.gpu
F = np.float32
FRAME = 3
B_ORIGIN, B_STEP, B_DIMS = (-0.7, -0.8, -0.9), (0.05, 0.055, 0.05), (29, 23, 37)
F_STEP, F_DIMS = (0.025, 0.0275, 0.025), (57, 45, 73)
# (scene, step, dims, brick, band): the sound cases of tests/test_sparse_mesh_cpu.py, then scene v1 with
# band 0 (only the bricks with a corner sign change: an open mesh, vertices on faces of culled bricks)
CASES = [("tanh", B_STEP, B_DIMS, 4, 0.18), ("v1", B_STEP, B_DIMS, 4, 0.18), ("displace", B_STEP, B_DIMS, 4, 0.18),
         ("tanh", F_STEP, F_DIMS, 8, 0.18), ("tanh", F_STEP, F_DIMS, 4, 0.09), ("v1", B_STEP, B_DIMS, 4, 0.0)]
if torch.cuda.is_available():
    torch.cuda.init()


@functools.lru_cache(maxsize=None)
def plane_net(four):
    dims, K, B = nr.read_keras_h5(nr.geometry_path("plane_1"))
    if four:
        K = [np.concatenate([K[0], np.random.default_rng(4).normal(0, 0.01, (1, 32)).astype(np.float32)], 0)] + K[1:]
        dims = [4] + list(dims[1:])
    return dims, K, B, oracle.OracleNet(K, B)


@functools.lru_cache(maxsize=None)
def ref_grid(scene, step=B_STEP, dims=B_DIMS, four=False, origin=B_ORIGIN):
    """mesh_ref.sample, computed once per lattice and shared (never modified)."""
    v = mesh_ref.sample(plane_net(four)[3], origin, step, dims, scene=nr.NR_SCENE[scene], frame=FRAME)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def ref_sparse(scene, step, dims, brick, band, four=False):
    """(V, T, cells, keys, N, active) of the reference's restricted mesh."""
    V, T, cells, keys, active = sref.mesh(ref_grid(scene, step, dims, four), B_ORIGIN, step, brick, 0.0, F(band))
    N = mesh_ref.normals(plane_net(four)[3], V, scene=nr.NR_SCENE[scene], frame=FRAME)
    for a in (V, T, cells, keys, N, active):
        a.setflags(write=False)
    return V, T, cells, keys, N, active


def _renderer(four):
    dims, K, B, _ = plane_net(four)
    r = nr.Renderer(0)
    r.load_mlp(dims, K, B).set_precision("fp32").set_static(nr.NR_COLOR_FACING, 4 if four else 3)
    r.set_view(*nr.camera(0.0, 0.0, 2.0), FRAME)
    return r


@pytest.fixture(scope="module")
def rend():
    r = _renderer(False)
    yield r
    r.close()


@pytest.fixture(scope="module")
def rend4():
    r = _renderer(True)
    yield r
    r.close()


def assert_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype)
    bad = bits(got) != bits(ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def assert_against_ref(out, st, ref, dims, brick, what, normals=True):
    rV, rT, rc, rk, rN, active = ref
    got = sref.in_key_order(out, dims)
    sref.assert_same_mesh(got, ref, what)
    if normals:
        assert_bits(got[4], rN, what + " normals")
    assert out["triangles"].dtype == np.int32 and out["keys"].dtype == np.int64
    assert out["active_bricks"] == int(active.sum()), (what, out["active_bricks"], int(active.sum()))
    nb = sref.brick_counts(dims, brick)
    steps = (nb[0] + 1) * (nb[1] + 1) * (nb[2] + 1) + sref.point_set_total(active, dims, brick)
    want = (steps, int(active.sum()), len(rV), 4 * len(rV) if normals else 0)
    assert (st["ray_steps"], st["rays_hit"], st["rays_shaded"], st["shade_evals"]) == want, (what, st, want)
    assert st["launches"] >= 3 and st["ms_total"] > 0


@pytest.mark.parametrize("scene,step,dims,brick,band", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_against_reference(rend, scene, step, dims, brick, band):
    ref = ref_sparse(scene, step, dims, brick, band)
    assert len(ref[0]) > 500 and not ref[5].all()  # the case culls, and keeps a mesh
    if band > 0:  # the sound cases: the dense mesh, closed
        dense = mesh_ref.mesh(ref_grid(scene, step, dims), B_ORIGIN, step, 0.0)
        assert len(ref[0]) == len(dense[0]) and mesh_ref.is_closed_oriented(ref[1])
    else:
        assert not mesh_ref.is_closed_oriented(ref[1])
    out, st = rend.set_scene(scene).extract_mesh_sparse(B_ORIGIN, step, dims, brick=brick, band=F(band), with_stats=True)
    assert_against_ref(out, st, ref, dims, brick, f"{scene} brick {brick} band {band}")
    assert mesh_ref.is_closed_oriented(out["triangles"]) == (band > 0)
    if (scene, dims) == ("v1", B_DIMS):
        bare, bst = rend.extract_mesh_sparse(B_ORIGIN, step, dims, brick=brick, band=F(band), normals=False, with_stats=True)
        assert "normals" not in bare
        assert_against_ref(bare, bst, ref, dims, brick, "without normals", normals=False)
        assert bare["vertices"].tobytes() == out["vertices"].tobytes() and bare["keys"].tobytes() == out["keys"].tobytes()
        nokeys = rend.extract_mesh_sparse(B_ORIGIN, step, dims, brick=brick, band=F(band), keys=False)
        assert "keys" not in nokeys
        for k in ("vertices", "normals", "triangles"):
            assert nokeys[k].tobytes() == out[k].tobytes(), k


def _crossing_origin(di, dj, dk):
    """A lattice origin (B's steps) that puts a cell of the v1 reference mesh at cell (di, dj, dk)."""
    cells = mesh_ref.mesh(ref_grid("v1"), B_ORIGIN, B_STEP, 0.0)[2]
    c = int(cells[len(cells) // 2])
    idx = (c % B_DIMS[0] - di, (c // B_DIMS[0]) % B_DIMS[1] - dj, c // (B_DIMS[0] * B_DIMS[1]) - dk)
    return tuple(float(F(B_ORIGIN[a]) + F(idx[a]) * F(B_STEP[a])) for a in range(3))


# dims, brick, origin: the box at brick 4 and at brick 16 (ragged last bricks of 12, 6 and 4 cells), one
# ragged brick per axis, a 16-cell and a 1-cell brick -- the small ones placed on the surface
INF_CASES = [(B_DIMS, 4, None), (B_DIMS, 16, None), ((3, 2, 2), 4, (0, 0, 0)), ((3, 2, 2), 16, (1, 0, 0)),
             ((18, 17, 2), 16, (16, 8, 0)), ((18, 17, 2), 8, (9, 15, 0))]


@pytest.mark.parametrize("dims,brick,place", INF_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_infinite_band_is_extract_mesh(rend, dims, brick, place):
    origin = B_ORIGIN if place is None else _crossing_origin(*place)
    rend.set_scene("v1")
    dense, dst = rend.extract_mesh(origin, B_STEP, dims, with_stats=True)
    out, st = rend.extract_mesh_sparse(origin, B_STEP, dims, brick=brick, band=np.inf, with_stats=True)
    assert len(dense["vertices"]) > 0 and len(dense["triangles"]) > 0
    nb = sref.brick_counts(dims, brick)
    assert out["active_bricks"] == nb[0] * nb[1] * nb[2] == st["rays_hit"]
    V, T, cells, keys, N = sref.in_key_order(out, dims)
    assert_bits(V, dense["vertices"], "vertices")
    assert_bits(N, dense["normals"], "normals")
    # the dense mesh's vertices are in key order: its triangles' cells follow from the sparse keys
    dcells = mesh_ref.triangle_cells(dense["triangles"], keys, dims)
    assert mesh_ref.cell_sets(T, cells) == mesh_ref.cell_sets(dense["triangles"], dcells)
    full = np.ones(nb[::-1], bool)
    assert st["ray_steps"] == (nb[0] + 1) * (nb[1] + 1) * (nb[2] + 1) + sref.point_set_total(full, dims, brick)
    assert st["rays_shaded"] == dst["rays_shaded"] == len(V)


def test_default_band_is_the_brick_diagonal(rend):
    band = sref.default_band(B_STEP, 4)
    assert band.dtype == np.float32 and abs(float(band) - 4 * np.sqrt(0.05 ** 2 + 0.055 ** 2 + 0.05 ** 2)) < 1e-6
    ref = ref_sparse("tanh", B_STEP, B_DIMS, 4, float(band))
    assert int(ref[5].sum()) > int(ref_sparse("tanh", B_STEP, B_DIMS, 4, 0.18)[5].sum())
    out, st = rend.set_scene("tanh").extract_mesh_sparse(B_ORIGIN, B_STEP, B_DIMS, brick=4, with_stats=True)
    assert_against_ref(out, st, ref, B_DIMS, 4, "default band")


def test_four_inputs(rend4):
    ref = ref_sparse("tanh", B_STEP, B_DIMS, 4, 0.18, True)
    assert len(ref[0]) > 500 and not ref[5].all()
    out, st = rend4.set_scene("tanh").extract_mesh_sparse(B_ORIGIN, B_STEP, B_DIMS, brick=4, band=F(0.18), with_stats=True)
    assert_against_ref(out, st, ref, B_DIMS, 4, "4 inputs")


def _device_call(r, step, dims, brick, band, nv, nt, guard=1):
    dev = torch.device("cuda:0")
    V = torch.full((nv + guard, 3), -7.0, dtype=torch.float32, device=dev)
    N = torch.full((nv + guard, 3), -7.0, dtype=torch.float32, device=dev)
    K = torch.full((nv + guard,), -7, dtype=torch.int64, device=dev)
    T = torch.full((nt + guard, 3), -7, dtype=torch.int32, device=dev)
    try:
        r.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        res = r.extract_mesh_sparse_device(B_ORIGIN, step, dims, V.data_ptr(), nv, T.data_ptr(), nt, brick=brick, band=band,
                                           normals_ptr=N.data_ptr(), keys_ptr=K.data_ptr())
        r.synchronize()
    finally:
        r.set_stream(None, own=True)
    return res, {"vertices": V.cpu().numpy(), "normals": N.cpu().numpy(), "keys": K.cpu().numpy(), "triangles": T.cpu().numpy()}


def test_deterministic(rend):
    scene, step, dims, brick, band = CASES[4]
    rend.set_scene(scene)
    a = rend.extract_mesh_sparse(B_ORIGIN, step, dims, brick=brick, band=F(band))
    b = rend.extract_mesh_sparse(B_ORIGIN, step, dims, brick=brick, band=F(band))
    try:
        one = rend.set_occupancy(1).extract_mesh_sparse(B_ORIGIN, step, dims, brick=brick, band=F(band))
    finally:
        rend.set_occupancy(0)
    try:
        rend.set_precision("bf16")  # ignored: always the fp32 MLP
        low = rend.extract_mesh_sparse(B_ORIGIN, step, dims, brick=brick, band=F(band))
    finally:
        rend.set_precision("fp32")
    for k in ("vertices", "normals", "keys", "triangles"):
        for name, o in (("second call", b), ("one workgroup per CU", one), ("bf16 selected", low)):
            assert a[k].tobytes() == o[k].tobytes(), (k, name)
    nv, nt = len(a["vertices"]), len(a["triangles"])
    (cv, ct, ca), dev = _device_call(rend, step, dims, brick, F(band), nv, nt)
    assert (cv, ct, ca) == (nv, nt, a["active_bricks"])
    for k in ("vertices", "normals", "keys", "triangles"):
        assert dev[k][:-1].tobytes() == a[k].tobytes(), k
        assert (dev[k][-1] == -7).all(), k  # nothing past nv / nt


def _raw(r, dims=B_DIMS, brick=4, band=0.18, iso=0.0, V=None, N=None, K=None, T=None, vcap=0, tcap=0, origin=True, step=True,
         nv=True, nt=True, active=True, ctx=True):
    o, s = np.asarray(B_ORIGIN, F), np.asarray(B_STEP, F)
    d = None if dims is None else (ctypes.c_int * 3)(*dims)
    cv, ct, ca = ctypes.c_long(-1), ctypes.c_long(-1), ctypes.c_long(-1)
    ptr = [None if a is None else a.ctypes.data for a in (V, N, K, T)]
    rc = nr.lib().nr_extract_mesh_sparse(r._ctx if ctx else None, nr.renderer._fptr(o) if origin else None,
                                         nr.renderer._fptr(s) if step else None, d, iso, brick, band, ptr[0], ptr[1], ptr[2], vcap,
                                         ptr[3], tcap, ctypes.byref(cv) if nv else None, ctypes.byref(ct) if nt else None,
                                         ctypes.byref(ca) if active else None, 0, None)
    return rc, cv.value, ct.value, ca.value


def test_capacity_protocol(rend):
    ref = ref_sparse("tanh", B_STEP, B_DIMS, 4, 0.18)
    NV, NT, NA = len(ref[0]), len(ref[1]), int(ref[5].sum())
    rend.set_scene("tanh")
    assert _raw(rend) == (0, NV, NT, NA)  # count only
    assert _raw(rend, active=False)[:3] == (0, NV, NT)

    def bufs(extra=0):
        return (np.full((NV + extra, 3), -5.0, F), np.full((NV + extra, 3), -5.0, F), np.full((NV + extra,), -5, np.int64),
                np.full((NT + extra, 3), -5, np.int32))

    for vcap, tcap in ((NV - 1, NT), (NV, NT - 1), (0, 0)):
        V, N, K, T = bufs()
        assert _raw(rend, V=V, N=N, K=K, T=T, vcap=vcap, tcap=tcap) == (-6, NV, NT, NA)  # NR_E_NOMEM, the counts set
        assert (V == -5.0).all() and (N == -5.0).all() and (K == -5).all() and (T == -5).all()  # nothing written
    V, N, K, T = bufs(2)
    assert _raw(rend, V=V, N=N, K=K, T=T, vcap=NV, tcap=NT) == (0, NV, NT, NA)  # exact capacities
    assert (V[NV:] == -5.0).all() and (N[NV:] == -5.0).all() and (K[NV:] == -5).all() and (T[NT:] == -5).all()
    out = {"vertices": V[:NV], "normals": N[:NV], "keys": K[:NV], "triangles": T[:NT]}
    sref.assert_same_mesh(sref.in_key_order(out, B_DIMS), ref, "exact capacities")


def test_errors(rend):
    V, N, K, T = np.zeros((8, 3), F), np.zeros((8, 3), F), np.zeros(8, np.int64), np.zeros((8, 3), np.int32)
    INVALID, FORMAT, STATE = -1, -4, -5
    with nr.Renderer(0) as r:
        assert _raw(r)[0] == STATE  # no network
        rng = np.random.default_rng(0)
        r.load_mlp([3, 16, 1], [rng.normal(size=(3, 16)).astype(F), rng.normal(size=(16, 1)).astype(F)],
                   [np.zeros(16, F), np.zeros(1, F)])
        assert _raw(r)[0] == FORMAT  # not a network of the fused kernels
    assert _raw(rend, ctx=False)[0] == INVALID
    for kw in ({"origin": False}, {"step": False}, {"dims": None}, {"nv": False}, {"nt": False}):
        assert _raw(rend, **kw)[0] == INVALID, kw
    for bad in ((1, 23, 37), (29, 1, 37), (29, 23, 1), (0, 2, 2), (65537, 2, 2), (2, 65537, 2), (2, 2, 65537), (-3, 2, 2)):
        assert _raw(rend, dims=bad)[0] == INVALID, bad
    for bad in (0, 1, 2, 5, 12, 32, -4):
        assert _raw(rend, brick=bad)[0] == INVALID, bad
    for bad in (-1e-30, -1.0, float("nan"), -float("inf")):
        assert _raw(rend, band=bad)[0] == INVALID, bad
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert _raw(rend, iso=bad)[0] == INVALID, bad
    assert _raw(rend, V=V, vcap=8)[0] == INVALID and _raw(rend, T=T, tcap=8)[0] == INVALID  # only one of the two
    assert _raw(rend, K=K)[0] == INVALID and _raw(rend, N=N)[0] == INVALID  # keys, normals without vertices
    assert _raw(rend, dims=(65536, 65536, 65), brick=4)[0] == INVALID  # 2^32 bricks
    assert _raw(rend, dims=(65536, 65536, 21), brick=4)[0] == INVALID  # 2^30 + 2^28 bricks
    msg = nr.lib().nr_last_error(rend._ctx).decode()
    assert "bricks" in msg, msg


def test_empty_result(rend):
    """A lattice far from the model, every corner further than the band from iso: no active brick."""
    origin, dims = (3.0, 3.0, 3.0), (10, 9, 11)
    g = ref_grid("tanh", B_STEP, dims, False, origin)
    assert not sref.active_bricks(g, 4, 0.0, F(0.05)).any()
    rend.set_scene("tanh")
    out, st = rend.extract_mesh_sparse(origin, B_STEP, dims, brick=4, band=F(0.05), with_stats=True)
    assert out["vertices"].shape == (0, 3) and out["triangles"].shape == (0, 3) and out["keys"].shape == (0,)
    assert out["active_bricks"] == 0 and st["rays_hit"] == 0 and st["rays_shaded"] == 0
    assert st["ray_steps"] == 4 * 3 * 4  # the corner lattice alone
    # active bricks that hold no crossing: still an empty mesh, not an error
    out = rend.extract_mesh_sparse(origin, B_STEP, dims, brick=4, band=np.inf)
    assert out["active_bricks"] == 3 * 2 * 3 and out["vertices"].shape == (0, 3) and out["triangles"].shape == (0, 3)
    assert not (g < 0).any()


def test_indices_past_2_to_32(rend):
    """A lattice of 4,097 x 2,049 x 1,025 = 8.6 x 10^9 points over [-6, 6]^3 (2.2 x 10^6 bricks of 16)
    with the model around its middle layer, where the linear index passes 2^32: the keys are 64-bit
    on both sides of it, and a sample of the vertices is where the oracle's values at the two ends of
    their edges put them."""
    dims = (4097, 2049, 1025)
    origin = (-6.0, -6.0, -6.0)
    step = (F(12.0) / F(4096), F(12.0) / F(2048), F(12.0) / F(1024))
    rend.set_scene("tanh")
    out = rend.extract_mesh_sparse(origin, step, dims, brick=16, band=F(0.1), normals=False)
    keys, V, T = out["keys"], out["vertices"], out["triangles"]
    print("vertices", len(V), "triangles", len(T), "active bricks", out["active_bricks"])
    assert len(V) > 10000 and len(np.unique(keys)) == len(keys)
    assert keys.min() >= 0 and keys.max() < 7 * dims[0] * dims[1] * dims[2]
    assert (keys > 7 * 2 ** 32).sum() > 1000 and (keys < 7 * 2 ** 32).sum() > 1000
    assert T.min() >= 0 and T.max() < len(V) and mesh_ref.is_closed_oriented(T)
    sel = np.random.default_rng(1).choice(len(V), 4000, replace=False)
    o, e = keys[sel] // 7, mesh_ref.SLOTS[keys[sel] % 7]
    idx = np.stack([o % dims[0], (o // dims[0]) % dims[1], o // (dims[0] * dims[1])], -1)
    og, sg = np.asarray(origin, F), np.asarray(step, F)
    pa = (og + (idx.astype(F) * sg).astype(F)).astype(F)
    pb = (og + ((idx + e).astype(F) * sg).astype(F)).astype(F)
    net = plane_net(False)[3]
    with np.errstate(all="ignore"):
        sa = query_ref._scene(pa, query_ref._mlp(net, pa, FRAME), nr.NR_SCENE["tanh"], FRAME)
        sb = query_ref._scene(pb, query_ref._mlp(net, pb, FRAME), nr.NR_SCENE["tanh"], FRAME)
        assert ((sa < 0) != (sb < 0)).all()  # every one a crossing edge
        t = ((F(0.0) - sa) / (sb - sa)).astype(F)
        want = (pa + ((pb - pa).astype(F) * t[:, None]).astype(F)).astype(F)
    assert_bits(V[sel], want, "sampled vertices")
