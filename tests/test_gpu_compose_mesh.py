"""Composed scenes on a lattice on the GPU (nr_compose_sample_grid, nr_compose_extract_mesh,
nr_compose_extract_mesh_sparse; nr_compose_mesh.hip) against tests/compose_mesh_ref.py -- the composed
field of compose_ref on the lattice of mesh_ref, meshed by mesh_ref / sparse_mesh_ref (pinned by
tests/test_compose_mesh_cpu.py) -- against the by-hand route through nr_compose_sample and
nr_mesh_grid, and against the single-network calls for a lone identity part.  The contract is
bit-exactness: every comparison is on uint32 views or bytes."""
import ctypes

import numpy as np
import pytest
import torch

import compose_mesh_ref as cmref
import cudaneuralrender_amd as nr
import mesh_ref
import sparse_mesh_ref as sref
from compose_mesh_ref import (FOUR_DIMS, FOUR_ORIGIN, FOUR_STEP, LONE_DIMS, LONE_ORIGIN, LONE_STEP, RAGGED_DIMS, S3, S3_DIMS,
                              S3_ORIGIN, S3_STEP, SCENES)
from compose_ref import SUBTRACT, UNION, part, rot_xyz
from mesh_ref import bits

pytestmark = pytest.mark.gpu
F = np.float32
GEOMS = ("plane_1", "plane_2", "plane_3", "car_1")
INVALID, NOMEM = -1, -6
if torch.cuda.is_available():
    torch.cuda.init()


def _renderer(nets, g):
    dims, K, B = nets[g]
    r = nr.Renderer(0)
    r.load_mlp(dims, K, B).set_precision("fp32").set_static(nr.NR_COLOR_FACING, 3).set_scene("tanh")
    r.set_view(*nr.camera(0.0, 0.0, 2.0), 0)
    return r


@pytest.fixture(scope="module")
def rends(nets):
    out = {g: _renderer(nets, g) for g in GEOMS}
    yield out
    for r in out.values():
        r.close()


@pytest.fixture(scope="module")
def comps(rends):
    """The compositions, owned by the plane_1 renderer."""
    out = {k: nr.Composition(rends["plane_1"], [rends[g] for g in names], parts) for k, (names, parts) in SCENES.items()}
    yield out
    for c in out.values():
        c.close()


def assert_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = bits(got) != bits(ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def assert_dense(out, ref, dims, what, normals=True, owners=True):
    """Vertices, normals and part bit for bit in the pinned order, triangles cell by cell."""
    rV, rT, cells, keys, rN, rP = ref
    V, T = out["vertices"], out["triangles"]
    assert (len(V), len(T)) == (len(rV), len(rT)), (what, len(V), len(T), len(rV), len(rT))
    assert_bits(V, rV, what + " vertices")
    assert T.dtype == np.int32 and T.min(initial=0) >= 0 and T.max(initial=-1) < len(rV)
    got = mesh_ref.cell_sets(T, mesh_ref.triangle_cells(T, keys, dims))
    want = mesh_ref.cell_sets(rT, cells)
    assert got == want, f"{what}: the triangles of {sum(got.get(c) != want.get(c) for c in set(got) | set(want))} cells differ"
    assert ("normals" in out) == normals and ("part" in out) == owners
    if normals:
        assert_bits(out["normals"], rN, what + " normals")
    if owners:
        assert_bits(out["part"], rP, what + " part")


def same_bytes(a, b, keys, what):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


# ---- 1. sample_grid
@pytest.mark.parametrize("scene,origin,step,dims", [("s3", S3_ORIGIN, S3_STEP, S3_DIMS), ("four", FOUR_ORIGIN, FOUR_STEP, FOUR_DIMS),
                                                    ("s3", (-0.3, -0.1, -0.2), (1.3, 0.4, 0.35), (2, 2, 2))],
                         ids=["s3", "four", "2x2x2"])
def test_sample_grid(comps, scene, origin, step, dims):
    rv, ro, pairs = cmref.ref_grid(scene, origin, step, dims)
    n = dims[0] * dims[1] * dims[2]
    assert n % 64 != 0 and 0 < pairs
    value, owner, st = comps[scene].sample_grid(origin, step, dims, owner=True, with_stats=True)
    assert_bits(value, rv, "value")
    assert_bits(owner, ro, "owner")
    assert (st["ray_steps"], st["part_evals"]) == (n, pairs), (st, n, pairs)
    assert st["rays_hit"] == 0 and st["rays_shaded"] == 0 and st["shade_evals"] == 0 and st["launches"] == 2 and st["ms_total"] > 0
    assert st["wave_evals"] > 0 and (n < 1000 or st["wave_skips"] > 0)
    # nr_compose_sample's bits on the same points
    by_points = comps[scene].sample(mesh_ref.lattice(origin, step, dims))
    assert_bits(value.reshape(-1), by_points["value"], "value against sample")
    assert_bits(owner.reshape(-1), by_points["owner"], "owner against sample")
    # the value alone
    assert_bits(comps[scene].sample_grid(origin, step, dims), rv, "value alone")


def test_sample_grid_device_outputs_are_independent(rends, comps):
    """Either output alone on device buffers, guard words intact behind them."""
    rv, ro, _ = cmref.ref_grid("four", FOUR_ORIGIN, FOUR_STEP, FOUR_DIMS)
    n = rv.size
    dev = torch.device("cuda:0")
    owner = rends["plane_1"]
    V = torch.full((n + 3,), -7.0, dtype=torch.float32, device=dev)
    W = torch.full((n + 3,), -7, dtype=torch.int32, device=dev)
    try:
        owner.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        comps["four"].sample_grid_device(FOUR_ORIGIN, FOUR_STEP, FOUR_DIMS, value_ptr=V.data_ptr())
        comps["four"].sample_grid_device(FOUR_ORIGIN, FOUR_STEP, FOUR_DIMS, owner_ptr=W.data_ptr())
        owner.synchronize()
    finally:
        owner.set_stream(None, own=True)
    v, w = V.cpu().numpy(), W.cpu().numpy()
    assert_bits(v[:n], rv.reshape(-1), "value")
    assert_bits(w[:n], ro.reshape(-1), "owner")
    assert (v[n:] == -7.0).all() and (w[n:] == -7).all()


# ---- 2. extract_mesh
def test_extract_mesh(rends, comps):
    ref = cmref.ref_dense("s3")
    out, st = comps["s3"].extract_mesh(S3_ORIGIN, S3_STEP, S3_DIMS, part=True, with_stats=True)
    assert_dense(out, ref, S3_DIMS, "s3")
    assert mesh_ref.is_closed_oriented(out["triangles"])
    nv = len(ref[0])
    want = (183015, cmref.ref_grid("s3")[2], 0, nv, 5 * nv)
    assert (st["ray_steps"], st["part_evals"], st["rays_hit"], st["rays_shaded"], st["shade_evals"]) == want, (st, want)
    assert st["launches"] == 6 and st["ms_total"] > 0  # zero, sample, count, scan, emit, vertex pass
    # the by-hand route: the lattice points through nr_compose_sample, then nr_mesh_grid on the owner
    vals = comps["s3"].sample(mesh_ref.lattice(S3_ORIGIN, S3_STEP, S3_DIMS))["value"].reshape(S3_DIMS[::-1])
    V, T = rends["plane_1"].mesh_grid(vals, S3_ORIGIN, S3_STEP)
    same_bytes(out, {"vertices": V, "triangles": T}, ("vertices", "triangles"), "by hand")
    # every choice of outputs: the same mesh
    for normals, owners in ((True, False), (False, True), (False, False)):
        o, s = comps["s3"].extract_mesh(S3_ORIGIN, S3_STEP, S3_DIMS, normals=normals, part=owners, with_stats=True)
        keys = ("vertices", "triangles") + (("normals",) if normals else ()) + (("part",) if owners else ())
        assert set(o) == set(keys)
        same_bytes(o, out, keys, (normals, owners))
        assert s["shade_evals"] == (4 * nv if normals else 0) + (nv if owners else 0)
        assert s["launches"] == 5 + (normals or owners)


def test_extract_mesh_at_another_level(comps):
    ref = cmref.ref_dense("s3", 0.01)
    out = comps["s3"].extract_mesh(S3_ORIGIN, S3_STEP, S3_DIMS, iso=0.01, part=True)
    assert_dense(out, ref, S3_DIMS, "iso 0.01")


# ---- 3. a lone identity part is the single-network extraction
def test_lone_identity_part(rends):
    src = rends["plane_1"]
    want = src.extract_mesh(LONE_ORIGIN, LONE_STEP, LONE_DIMS)
    wsp = src.extract_mesh_sparse(LONE_ORIGIN, LONE_STEP, LONE_DIMS, brick=4, band=F(0.12))
    assert len(want["vertices"]) > 500 and 0 < wsp["active_bricks"] < 6 * 7 * 7
    with nr.Composition(src, [src], [part(0)]) as comp:
        value = comp.sample_grid(LONE_ORIGIN, LONE_STEP, LONE_DIMS)
        out = comp.extract_mesh(LONE_ORIGIN, LONE_STEP, LONE_DIMS, part=True)
        sp = comp.extract_mesh_sparse(LONE_ORIGIN, LONE_STEP, LONE_DIMS, brick=4, band=F(0.12), part=True)
    assert_bits(value, src.sample_grid(LONE_ORIGIN, LONE_STEP, LONE_DIMS), "values")
    same_bytes(out, want, ("vertices", "triangles", "normals"), "dense")
    same_bytes(sp, wsp, ("vertices", "triangles", "normals", "keys"), "sparse")
    assert sp["active_bricks"] == wsp["active_bricks"]
    assert not out["part"].any() and not sp["part"].any()


# ---- 4. extract_mesh_sparse
def assert_sparse(out, st, ref, scene, dims, brick, what, normals=True, owners=True, origin=S3_ORIGIN, step=S3_STEP):
    rV, rT, rc, rk, rN, active, rP = ref
    got = sref.in_key_order(out, dims)
    sref.assert_same_mesh(got, ref, what)
    if normals:
        assert_bits(got[4], rN, what + " normals")
    if owners:
        assert_bits(out["part"][np.argsort(out["keys"], kind="stable")], rP, what + " part")
    assert out["triangles"].dtype == np.int32 and out["keys"].dtype == np.int64
    na = int(active.sum())
    assert out["active_bricks"] == na, (what, out["active_bricks"], na)
    nb = sref.brick_counts(dims, brick)
    steps = (nb[0] + 1) * (nb[1] + 1) * (nb[2] + 1) + sref.point_set_total(active, dims, brick)
    pairs = cmref.sparse_pairs(cmref.inbound_counts(SCENES[scene][1], origin, step, dims), active, brick)
    nv = len(rV)
    want = (steps, pairs, na, nv, (4 * nv if normals else 0) + (nv if owners else 0))
    assert (st["ray_steps"], st["part_evals"], st["rays_hit"], st["rays_shaded"], st["shade_evals"]) == want, (what, st, want)
    assert st["launches"] >= 4 and st["ms_total"] > 0 and st["wave_evals"] > 0


@pytest.mark.parametrize("dims", [S3_DIMS, RAGGED_DIMS], ids=["full", "ragged"])
@pytest.mark.parametrize("brick,band", [(4, 0.15), (8, 0.15), (4, 0.0)])
def test_sparse_against_reference(comps, dims, brick, band):
    ref = cmref.ref_sparse("s3", brick, band, dims)
    assert len(ref[0]) > 300 and not ref[5].all()  # the case culls, and keeps a mesh
    out, st = comps["s3"].extract_mesh_sparse(S3_ORIGIN, S3_STEP, dims, brick=brick, band=F(band), part=True, with_stats=True)
    assert_sparse(out, st, ref, "s3", dims, brick, f"{dims} brick {brick} band {band}")
    # band 0 leaves the open mesh (vertices on faces of culled bricks); 0.15 is sound
    assert mesh_ref.is_closed_oriented(out["triangles"]) == (band > 0)
    if band > 0:
        # a sound band: extract_mesh's mesh once sorted by key
        dense = comps["s3"].extract_mesh(S3_ORIGIN, S3_STEP, dims, part=True)
        V, T, cells, keys, N = sref.in_key_order(out, dims)
        assert_bits(V, dense["vertices"], "vertices against dense")
        assert_bits(N, dense["normals"], "normals against dense")
        assert_bits(out["part"][np.argsort(out["keys"], kind="stable")], dense["part"], "part against dense")
        dcells = mesh_ref.triangle_cells(dense["triangles"], keys, dims)
        assert mesh_ref.cell_sets(T, cells) == mesh_ref.cell_sets(dense["triangles"], dcells)


def test_four_networks(comps):
    """Four packs: the 12-wave workgroup with 121 KB of staged packs, in all four kernels."""
    ref = cmref.ref_dense("four", 0.0, FOUR_ORIGIN, FOUR_STEP, FOUR_DIMS)
    assert len(ref[0]) > 300 and set(ref[5].tolist()) == {1, 2, 3}  # (the coarse lattice misses the thin part 0)
    out = comps["four"].extract_mesh(FOUR_ORIGIN, FOUR_STEP, FOUR_DIMS, part=True)
    assert_dense(out, ref, FOUR_DIMS, "four")
    rsp = cmref.ref_sparse("four", 4, 0.15, FOUR_DIMS, 0.0, FOUR_ORIGIN, FOUR_STEP)
    assert 0 < len(rsp[0]) and not rsp[5].all()
    sp, st = comps["four"].extract_mesh_sparse(FOUR_ORIGIN, FOUR_STEP, FOUR_DIMS, brick=4, band=F(0.15), part=True, with_stats=True)
    assert_sparse(sp, st, rsp, "four", FOUR_DIMS, 4, "four sparse", origin=FOUR_ORIGIN, step=FOUR_STEP)


def test_sparse_infinite_band_is_extract_mesh(comps):
    dims = RAGGED_DIMS
    dense = comps["s3"].extract_mesh(S3_ORIGIN, S3_STEP, dims, part=True)
    out, st = comps["s3"].extract_mesh_sparse(S3_ORIGIN, S3_STEP, dims, brick=8, band=np.inf, part=True, with_stats=True)
    nb = sref.brick_counts(dims, 8)
    assert out["active_bricks"] == nb[0] * nb[1] * nb[2] == st["rays_hit"]
    V, T, cells, keys, N = sref.in_key_order(out, dims)
    assert_bits(V, dense["vertices"], "vertices")
    assert_bits(N, dense["normals"], "normals")
    assert_bits(out["part"][np.argsort(out["keys"], kind="stable")], dense["part"], "part")
    dcells = mesh_ref.triangle_cells(dense["triangles"], keys, dims)
    assert mesh_ref.cell_sets(T, cells) == mesh_ref.cell_sets(dense["triangles"], dcells)
    full = np.ones(nb[::-1], bool)
    assert st["ray_steps"] == (nb[0] + 1) * (nb[1] + 1) * (nb[2] + 1) + sref.point_set_total(full, dims, 8)


def test_sparse_default_band_and_output_choices(rends, comps):
    """band=None is the brick's diagonal; normals, part and keys are independent of each other."""
    band = sref.default_band(S3_STEP, 4)
    ref = cmref.ref_sparse("s3", 4, float(band))
    out, st = comps["s3"].extract_mesh_sparse(S3_ORIGIN, S3_STEP, S3_DIMS, brick=4, part=True, with_stats=True)
    assert_sparse(out, st, ref, "s3", S3_DIMS, 4, "default band")
    for normals, owners, keys in ((False, False, True), (True, False, False), (False, True, False)):
        o, s = comps["s3"].extract_mesh_sparse(S3_ORIGIN, S3_STEP, S3_DIMS, brick=4, normals=normals, part=owners, keys=keys,
                                               with_stats=True)
        want = ("vertices", "triangles") + (("normals",) if normals else ()) + (("part",) if owners else ()) + (("keys",) if keys else ())
        assert set(o) == set(want) | {"active_bricks"}
        same_bytes(o, out, want, (normals, owners, keys))
        assert s["shade_evals"] == (4 * len(ref[0]) if normals else 0) + (len(ref[0]) if owners else 0)


# ---- 5. order independence
MESH_KEYS = ("vertices", "triangles", "normals", "part")


def test_same_bytes_on_every_call_and_occupancy(rends, comps):
    for scene, origin, step, dims in (("s3", S3_ORIGIN, S3_STEP, RAGGED_DIMS), ("four", FOUR_ORIGIN, FOUR_STEP, FOUR_DIMS)):
        def run():
            c = comps[scene]
            return (c.sample_grid(origin, step, dims, owner=True, with_stats=True),
                    c.extract_mesh(origin, step, dims, part=True, with_stats=True),
                    c.extract_mesh_sparse(origin, step, dims, brick=4, band=F(0.15), part=True, with_stats=True))

        a, b = run(), run()
        try:
            rends["plane_1"].set_occupancy(1)
            one = run()
        finally:
            rends["plane_1"].set_occupancy(0)
        assert len(a[1][0]["vertices"]) > 100 and len(a[2][0]["vertices"]) > 100
        for name, o in (("second call", b), ("one workgroup per CU", one)):
            assert a[0][0].tobytes() == o[0][0].tobytes() and a[0][1].tobytes() == o[0][1].tobytes(), (scene, name)
            same_bytes(a[1][0], o[1][0], MESH_KEYS, (scene, name, "dense"))
            same_bytes(a[2][0], o[2][0], MESH_KEYS + ("keys",), (scene, name, "sparse"))
            for i in range(3):  # the statistics that do not depend on the grouping
                for k in ("ray_steps", "part_evals", "rays_hit", "rays_shaded", "shade_evals"):
                    assert a[i][-1][k] == o[i][-1][k], (scene, name, i, k)


def test_one_pack_against_two(nets, rends):
    """The same parts over one pack (4-wave workgroups) and over two equal packs (12-wave
    workgroups): the same bytes."""
    car = rends["car_1"]
    twin = _renderer(nets, "car_1")
    parts = [part(0, UNION, None, (-0.9, 0.0, 0.0), 1.0), part(0, UNION, rot_xyz(0.3, 1.0, -0.2), (1.0, 0.2, 0.1), 0.75),
             part(0, SUBTRACT, rot_xyz(1.2, 0.4, 0.5), (-0.9, 0.0, 0.0), 0.6)]
    spread = [dict(p, net=j % 2) for j, p in enumerate(parts)]
    try:
        with nr.Composition(car, [car], parts) as one, nr.Composition(car, [car, twin], spread) as two:
            a, b = [(c.sample_grid(S3_ORIGIN, S3_STEP, RAGGED_DIMS, owner=True, with_stats=True),
                     c.extract_mesh(S3_ORIGIN, S3_STEP, RAGGED_DIMS, part=True, with_stats=True),
                     c.extract_mesh_sparse(S3_ORIGIN, S3_STEP, RAGGED_DIMS, brick=4, band=F(0.15), part=True, with_stats=True))
                    for c in (one, two)]
    finally:
        twin.close()
    assert len(a[1][0]["vertices"]) > 1000 and set(a[1][0]["part"].tolist()) == {0, 1, 2}
    assert a[0][0].tobytes() == b[0][0].tobytes() and a[0][1].tobytes() == b[0][1].tobytes()
    same_bytes(a[1][0], b[1][0], MESH_KEYS, "dense")
    same_bytes(a[2][0], b[2][0], MESH_KEYS + ("keys",), "sparse")
    for i in range(3):
        for k in ("ray_steps", "part_evals", "rays_hit", "rays_shaded", "shade_evals"):
            assert a[i][-1][k] == b[i][-1][k], (i, k)


# ---- 6. capacities and errors
def _dense_raw(comp, dims=S3_DIMS, iso=0.0, V=None, N=None, P=None, T=None, vcap=0, tcap=0, origin=True, step=True, nv=True,
               nt=True, c=True):
    o, s = np.asarray(S3_ORIGIN, F), np.asarray(S3_STEP, F)
    d = None if dims is None else (ctypes.c_int * 3)(*dims)
    cv, ct = ctypes.c_long(-1), ctypes.c_long(-1)
    ptr = [None if a is None else a.ctypes.data for a in (V, N, P, T)]
    rc = nr.lib().nr_compose_extract_mesh(comp._c if c else None, nr.renderer._fptr(o) if origin else None,
                                          nr.renderer._fptr(s) if step else None, d, iso, ptr[0], ptr[1], ptr[2], vcap, ptr[3],
                                          tcap, ctypes.byref(cv) if nv else None, ctypes.byref(ct) if nt else None, 0, None)
    return rc, cv.value, ct.value


def _sparse_raw(comp, dims=S3_DIMS, brick=4, band=0.15, iso=0.0, V=None, N=None, P=None, K=None, T=None, vcap=0, tcap=0,
                origin=True, step=True, nv=True, nt=True, active=True, c=True):
    o, s = np.asarray(S3_ORIGIN, F), np.asarray(S3_STEP, F)
    d = None if dims is None else (ctypes.c_int * 3)(*dims)
    cv, ct, ca = ctypes.c_long(-1), ctypes.c_long(-1), ctypes.c_long(-1)
    ptr = [None if a is None else a.ctypes.data for a in (V, N, P, K, T)]
    rc = nr.lib().nr_compose_extract_mesh_sparse(
        comp._c if c else None, nr.renderer._fptr(o) if origin else None, nr.renderer._fptr(s) if step else None, d, iso, brick,
        band, ptr[0], ptr[1], ptr[2], ptr[3], vcap, ptr[4], tcap, ctypes.byref(cv) if nv else None,
        ctypes.byref(ct) if nt else None, ctypes.byref(ca) if active else None, 0, None)
    return rc, cv.value, ct.value, ca.value


def test_capacity_protocol_on_the_host(comps):
    comp = comps["s3"]
    ref = cmref.ref_sparse("s3", 4, 0.15)
    NV, NT, NA = len(ref[0]), len(ref[1]), int(ref[5].sum())
    assert _dense_raw(comp) == (0, NV, NT)  # count only
    assert _sparse_raw(comp) == (0, NV, NT, NA) and _sparse_raw(comp, active=False)[:3] == (0, NV, NT)

    def bufs(extra=0):
        return (np.full((NV + extra, 3), -5.0, F), np.full((NV + extra, 3), -5.0, F), np.full((NV + extra,), -5, np.int32),
                np.full((NV + extra,), -5, np.int64), np.full((NT + extra, 3), -5, np.int32))

    for vcap, tcap in ((NV - 1, NT), (NV, NT - 1), (0, 0)):
        V, N, P, K, T = bufs()
        assert _dense_raw(comp, V=V, N=N, P=P, T=T, vcap=vcap, tcap=tcap) == (NOMEM, NV, NT)
        assert _sparse_raw(comp, V=V, N=N, P=P, K=K, T=T, vcap=vcap, tcap=tcap) == (NOMEM, NV, NT, NA)
        assert all((a == -5).all() for a in (V, N, P, K, T))  # nothing written
    V, N, P, K, T = bufs(2)
    assert _dense_raw(comp, V=V, N=N, P=P, T=T, vcap=NV, tcap=NT) == (0, NV, NT)  # exact capacities
    assert all((a[n:] == -5).all() for a, n in ((V, NV), (N, NV), (P, NV), (T, NT)))
    assert_dense({"vertices": V[:NV], "normals": N[:NV], "part": P[:NV], "triangles": T[:NT]}, cmref.ref_dense("s3"), S3_DIMS, "exact")
    V, N, P, K, T = bufs(2)
    assert _sparse_raw(comp, V=V, N=N, P=P, K=K, T=T, vcap=NV, tcap=NT) == (0, NV, NT, NA)
    assert all((a[n:] == -5).all() for a, n in ((V, NV), (N, NV), (P, NV), (K, NV), (T, NT)))
    sref.assert_same_mesh(sref.in_key_order({"vertices": V[:NV], "keys": K[:NV], "triangles": T[:NT]}, S3_DIMS), ref, "exact")


def test_capacity_protocol_on_device_buffers(rends, comps):
    """Short capacities write nothing; exact ones leave the guard words around the buffers intact."""
    comp, owner = comps["s3"], rends["plane_1"]
    host = comp.extract_mesh_sparse(S3_ORIGIN, S3_STEP, S3_DIMS, brick=4, band=F(0.15), part=True)
    dense = comp.extract_mesh(S3_ORIGIN, S3_STEP, S3_DIMS, part=True)
    nv, nt, G = len(host["vertices"]), len(host["triangles"]), 2
    dev = torch.device("cuda:0")

    def bufs():
        return {"vertices": torch.full((nv + 2 * G, 3), -7.0, dtype=torch.float32, device=dev),
                "normals": torch.full((nv + 2 * G, 3), -7.0, dtype=torch.float32, device=dev),
                "part": torch.full((nv + 2 * G,), -7, dtype=torch.int32, device=dev),
                "keys": torch.full((nv + 2 * G,), -7, dtype=torch.int64, device=dev),
                "triangles": torch.full((nt + 2 * G, 3), -7, dtype=torch.int32, device=dev)}

    def run(sparse, vcap, tcap):
        b = bufs()
        p = {k: t[G:].data_ptr() for k, t in b.items()}  # guard words on both sides
        try:
            owner.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            if sparse:
                res = comp.extract_mesh_sparse_device(S3_ORIGIN, S3_STEP, S3_DIMS, p["vertices"], vcap, p["triangles"], tcap, brick=4,
                                                      band=F(0.15), normals_ptr=p["normals"], part_ptr=p["part"], keys_ptr=p["keys"])
            else:
                res = comp.extract_mesh_device(S3_ORIGIN, S3_STEP, S3_DIMS, p["vertices"], vcap, p["triangles"], tcap,
                                               normals_ptr=p["normals"], part_ptr=p["part"])
            owner.synchronize()
        finally:
            owner.set_stream(None, own=True)
        return res, {k: t.cpu().numpy() for k, t in b.items()}

    for sparse, want in ((False, dense), (True, host)):
        with pytest.raises(nr.NRError) as e:
            run(sparse, nv - 1, nt)
        assert e.value.code == NOMEM
        res, got = run(sparse, nv, nt)
        assert res[:2] == (nv, nt) and (not sparse or res[2] == host["active_bricks"])
        for k, a in got.items():
            n = nt if k == "triangles" else nv
            if k == "keys" and not sparse:
                assert (a == -7).all()
                continue
            assert (a[:G] == -7).all() and (a[G + n:] == -7).all(), (sparse, k)
            assert a[G:G + n].tobytes() == want[k].tobytes(), (sparse, k)
    # a short call leaves the buffers untouched: checked on fresh buffers through the raw call
    b = bufs()
    cv, ct = ctypes.c_long(0), ctypes.c_long(0)
    o, s, d = nr.renderer._lattice(S3_ORIGIN, S3_STEP, S3_DIMS)
    rc = nr.lib().nr_compose_extract_mesh(comp._c, nr.renderer._fptr(o), nr.renderer._fptr(s), d, 0.0, b["vertices"].data_ptr(),
                                          b["normals"].data_ptr(), b["part"].data_ptr(), nv, b["triangles"].data_ptr(), nt - 1,
                                          ctypes.byref(cv), ctypes.byref(ct), 1, None)
    owner.synchronize()
    assert (rc, cv.value, ct.value) == (NOMEM, nv, nt)
    assert all(bool((t == -7).all()) for t in b.values())


def test_errors(rends, comps):
    comp = comps["s3"]
    L = nr.lib()
    V, N, P, K, T = np.zeros((8, 3), F), np.zeros((8, 3), F), np.zeros(8, np.int32), np.zeros(8, np.int64), np.zeros((8, 3), np.int32)
    o, s = nr.renderer._fptr(np.asarray(S3_ORIGIN, F)), nr.renderer._fptr(np.asarray(S3_STEP, F))
    d = (ctypes.c_int * 3)(4, 4, 4)
    val = np.zeros(64, F)
    # sample_grid
    assert L.nr_compose_sample_grid(None, o, s, d, val.ctypes.data, None, 0, None) == INVALID
    assert L.nr_compose_sample_grid(comp._c, o, s, d, None, None, 0, None) == INVALID
    assert L.nr_compose_sample_grid(comp._c, None, s, d, val.ctypes.data, None, 0, None) == INVALID
    assert L.nr_compose_sample_grid(comp._c, o, None, d, val.ctypes.data, None, 0, None) == INVALID
    assert L.nr_compose_sample_grid(comp._c, o, s, None, val.ctypes.data, None, 0, None) == INVALID
    for bad in ((0, 4, 4), (4, -1, 4), (1025, 1024, 1024)):
        assert L.nr_compose_sample_grid(comp._c, o, s, (ctypes.c_int * 3)(*bad), val.ctypes.data, None, 0, None) == INVALID, bad
    assert b"nr_compose_sample_grid" in L.nr_last_error(rends["plane_1"]._ctx)
    assert L.nr_compose_sample_grid(comp._c, o, s, (ctypes.c_int * 3)(64, 1, 1), val.ctypes.data, None, 0, None) == 0
    # the dense mesh
    assert _dense_raw(comp, c=False)[0] == INVALID
    for kw in ({"origin": False}, {"step": False}, {"dims": None}, {"nv": False}, {"nt": False}):
        assert _dense_raw(comp, **kw)[0] == INVALID, kw
    for bad in ((1, 23, 37), (29, 1, 37), (29, 23, 1), (0, 2, 2), (1025, 1024, 1024)):
        assert _dense_raw(comp, dims=bad)[0] == INVALID, bad
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert _dense_raw(comp, iso=bad)[0] == INVALID and _sparse_raw(comp, iso=bad)[0] == INVALID, bad
    assert _dense_raw(comp, V=V, vcap=8)[0] == INVALID and _dense_raw(comp, T=T, tcap=8)[0] == INVALID
    assert _dense_raw(comp, N=N)[0] == INVALID and _dense_raw(comp, P=P)[0] == INVALID
    # the sparse mesh
    assert _sparse_raw(comp, c=False)[0] == INVALID
    for kw in ({"origin": False}, {"step": False}, {"dims": None}, {"nv": False}, {"nt": False}):
        assert _sparse_raw(comp, **kw)[0] == INVALID, kw
    for bad in ((1, 23, 37), (29, 23, 1), (65537, 2, 2), (2, 2, 65537), (-3, 2, 2)):
        assert _sparse_raw(comp, dims=bad)[0] == INVALID, bad
    for bad in (0, 2, 5, 32, -4):
        assert _sparse_raw(comp, brick=bad)[0] == INVALID, bad
    for bad in (-1e-30, -1.0, float("nan"), -float("inf")):
        assert _sparse_raw(comp, band=bad)[0] == INVALID, bad
    assert _sparse_raw(comp, V=V, vcap=8)[0] == INVALID and _sparse_raw(comp, T=T, tcap=8)[0] == INVALID
    assert _sparse_raw(comp, K=K)[0] == INVALID and _sparse_raw(comp, N=N)[0] == INVALID and _sparse_raw(comp, P=P)[0] == INVALID
    assert _sparse_raw(comp, dims=(65536, 65536, 21), brick=4)[0] == INVALID  # 2^30 + 2^28 bricks
    msg = L.nr_last_error(rends["plane_1"]._ctx).decode()
    assert "nr_compose_extract_mesh_sparse" in msg and "bricks" in msg, msg


def test_the_owner_needs_no_network(rends):
    """The scratch is the owner's; its network, scene and precision are not consulted."""
    ref = cmref.ref_sparse("s3", 8, 0.15)
    srcs = [rends[g] for g in cmref.S3_NETS]
    with nr.Renderer(0) as bare:
        with nr.Composition(bare, srcs, S3) as comp:
            out, st = comp.extract_mesh_sparse(S3_ORIGIN, S3_STEP, S3_DIMS, brick=8, band=F(0.15), part=True, with_stats=True)
            dense = comp.extract_mesh(S3_ORIGIN, S3_STEP, S3_DIMS, part=True)
    assert_sparse(out, st, ref, "s3", S3_DIMS, 8, "bare owner")
    assert_dense(dense, cmref.ref_dense("s3"), S3_DIMS, "bare owner")


# ---- 7. nothing to mesh
def test_empty_result(comps):
    """A lattice outside every bound: no active brick, an empty mesh and no MLP evaluation."""
    origin, dims = (4.0, 4.0, 4.0), (10, 9, 11)
    cnt = cmref.inbound_counts(S3, origin, S3_STEP, dims)
    assert not cnt.any()
    out, st = comps["s3"].extract_mesh_sparse(origin, S3_STEP, dims, brick=4, band=F(0.3), part=True, with_stats=True)
    assert out["vertices"].shape == (0, 3) and out["triangles"].shape == (0, 3) and out["keys"].shape == (0,)
    assert out["normals"].shape == (0, 3) and out["part"].shape == (0,) and out["part"].dtype == np.int32
    assert out["active_bricks"] == 0 and st["rays_hit"] == 0 and st["rays_shaded"] == 0 and st["shade_evals"] == 0
    assert st["ray_steps"] == 4 * 3 * 4 and st["part_evals"] == 0  # the corner lattice alone
    assert st["wave_evals"] == 0 and st["wave_skips"] == 3
    dense, dst = comps["s3"].extract_mesh(origin, S3_STEP, dims, part=True, with_stats=True)
    assert dense["vertices"].shape == (0, 3) and dense["triangles"].shape == (0, 3) and dense["part"].shape == (0,)
    assert dst["ray_steps"] == 990 and dst["wave_evals"] == 0 and dst["part_evals"] == 0 and dst["wave_skips"] == 3 * 16
    # every brick active and still nothing to mesh: an empty mesh, not an error
    out = comps["s3"].extract_mesh_sparse(origin, S3_STEP, dims, brick=4, band=np.inf)
    assert out["active_bricks"] == 3 * 2 * 3 and out["vertices"].shape == (0, 3)


# ---- 8. new transforms
def test_after_set_parts(rends):
    moved = [dict(p) for p in S3]
    moved[1]["pos"] = np.array([0.4, -0.3, 0.2], F)
    moved[2]["op"] = UNION
    moved[2]["scale"] = F(0.5)
    srcs = [rends[g] for g in cmref.S3_NETS]
    origin, step, dims = S3_ORIGIN, (0.1, 0.11, 0.1), (42, 23, 25)
    with nr.Composition(rends["plane_1"], srcs, S3) as comp, nr.Composition(rends["plane_1"], srcs, moved) as fresh:
        base = comp.extract_mesh(origin, step, dims, part=True)
        comp.set_parts(moved)
        a, b = comp.extract_mesh(origin, step, dims, part=True), fresh.extract_mesh(origin, step, dims, part=True)
        sa = comp.extract_mesh_sparse(origin, step, dims, brick=4, band=F(0.3), part=True)
        sb = fresh.extract_mesh_sparse(origin, step, dims, brick=4, band=F(0.3), part=True)
        ga, gb = comp.sample_grid(origin, step, dims), fresh.sample_grid(origin, step, dims)
    assert len(a["vertices"]) > 300 and len(a["vertices"]) != len(base["vertices"])
    same_bytes(a, b, MESH_KEYS, "dense")
    same_bytes(sa, sb, MESH_KEYS + ("keys",), "sparse")
    assert ga.tobytes() == gb.tobytes()
    # and it is the new scene's reference
    nets = cmref.scene_nets("s3")
    value = cmref.sample(nets, moved, origin, step, dims)[0]
    V, T, cells, keys = mesh_ref.mesh(value, origin, step)
    assert_dense(a, (V, T, cells, keys, cmref.normals(nets, moved, V), cmref.owners(nets, moved, V)), dims, "moved")
