"""A triangle mesh built on the GPU (nr_mesh_create_device; nr_trimesh_build.hip) against
tests/trimesh_device_ref.py, the numpy restatement of the contract of a device-built mesh: what
nr_mesh_download returns is compared bit for bit, and every query of the device-built object
against the existing numpy walks fed the downloaded tree and table.  The meshes are chosen for what
can go wrong, not for size: a root that is a leaf, ragged halves, dead triangles, open and fourfold
edges, an axis without extent, and one mesh of more than 2048 triangles (several sort tiles for the
triangles and for the corners, more than 256 positions for the area table's blocks)."""
import functools

import numpy as np
import pytest
import torch

import cudaneuralrender_amd as nr
import mesh_ray_ref as MR
import sample_ref as SR
import trimesh_device_ref as DR
import trimesh_ref as R
import winding_ref as WR
from trimesh_ref import bits

pytestmark = pytest.mark.gpu
F = np.float32
if torch.cuda.is_available():
    torch.cuda.init()

# (mesh, leaf); the mesh whose points and rays it is queried at
CASES = [("one_triangle", 8), ("tetrahedron", 8), ("tetrahedron", 1), ("cube", 8), ("cube", 1), ("torus", 1), ("torus", 2),
         ("torus", 8), ("torus", 32), ("degenerate_torus", 8), ("open_torus", 8), ("double_cube", 2), ("flat_cube", 2),
         ("fine_torus", 8)]
QUERIED = [("one_triangle", 8), ("cube", 1), ("torus", 2), ("degenerate_torus", 8), ("double_cube", 2), ("flat_cube", 2),
           ("fine_torus", 8)]
PARENT = {"one_triangle": "tetrahedron", "tetrahedron": "tetrahedron", "cube": "cube", "torus": "torus",
          "degenerate_torus": "torus", "open_torus": "torus", "double_cube": "cube", "flat_cube": "cube", "fine_torus": "torus"}
ARRAYS = ("order", "nodes", "moments", "table", "thresholds")


@pytest.fixture(scope="module")
def owner():
    with nr.Renderer(0) as r:
        yield r


def assert_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = bits(got) != bits(ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def from_device(owner, V, T, leaf, with_stats=False):
    """the mesh built from torch tensors' pointers"""
    dV, dT = torch.from_numpy(np.array(V, F)).cuda(), torch.from_numpy(np.array(T, np.int32)).cuda()  # (copies: the meshes are read-only)
    torch.cuda.synchronize()
    return nr.TriMesh.from_device(owner, dV.data_ptr(), len(V), dT.data_ptr(), len(T), leaf=leaf, with_stats=with_stats)


@pytest.fixture(scope="module")
def built(owner):
    """device-built meshes by (name, leaf), kept for the module: alternately from_device and build="device" """
    made = {}

    def get(name, leaf):
        if (name, leaf) not in made:
            V, T = DR.mesh(name)
            if len(made) % 2 == 0:
                made[(name, leaf)] = from_device(owner, V, T, leaf, with_stats=True)
            else:
                made[(name, leaf)] = nr.TriMesh(owner, V, T, leaf=leaf, build="device")
        return made[(name, leaf)]

    yield get
    for m in made.values():
        m.close()


@functools.lru_cache(maxsize=None)
def points(name):
    return R.points(PARENT[name])


# ---- the build -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,leaf", CASES)
def test_download_is_the_contract(owner, built, name, leaf):
    V, T = DR.mesh(name)
    ref = DR.reference(name, leaf)
    m = built(name, leaf)
    got = m.download()
    for k in ARRAYS:
        assert_bits(got[k], ref[k], f"{name} leaf {leaf}: {k}")
    assert got["ntl"] == ref["ntl"] and got["area_last"] == ref["last"]
    info = m.info()
    assert info["closed"] == ref["closed"] and info["depth"] == ref["depth"] and info["nodes"] == len(ref["nodes"])
    assert (info["nv"], info["nt"]) == (len(V), len(T))
    assert_bits(info["lo"], ref["lo"], "lo")
    assert_bits(info["hi"], ref["hi"], "hi")
    if m.build_stats is not None:
        st = m.build_stats
        assert st["ray_steps"] == len(T) and st["launches"] == 36 + ref["depth"] and st["ms_total"] > 0


def test_both_constructors_and_two_builds_agree(owner):
    V, T = DR.mesh("fine_torus")
    with from_device(owner, V, T, 8) as a, nr.TriMesh(owner, V, T, leaf=8, build="device") as b, from_device(owner, V, T, 8) as c:
        da, db, dc = a.download(), b.download(), c.download()
    for k in ARRAYS:
        assert_bits(db[k], da[k], k)
        assert_bits(dc[k], da[k], k)


def test_default_build_is_the_hosts_and_its_download(owner):
    for name, leaf in (("degenerate_torus", 0), ("fine_torus", 3)):
        V, T = DR.mesh(name)
        nodes, order, moments, depth = nr.trimesh_hierarchy(V, T, leaf=leaf)
        thr, last = nr.renderer.mesh_area_table(V, T, leaf=leaf)
        with nr.TriMesh(owner, V, T, leaf=leaf) as m:
            got = m.download()
        assert_bits(got["nodes"], nodes, "nodes")
        assert_bits(got["order"], order, "order")
        assert_bits(got["moments"], moments, "moments")
        assert_bits(got["table"], nr.trimesh_normals(V, T)[0], "table")
        assert_bits(got["thresholds"], thr, "thresholds")
        assert got["ntl"] == len(order) and got["area_last"] == last


# ---- the queries of a device-built mesh ---------------------------------------------------------------

@pytest.mark.parametrize("name,leaf", QUERIED)
def test_distance_and_winding(owner, built, name, leaf):
    V, T = DR.mesh(name)
    m = built(name, leaf)
    d = m.download()
    X = points(name)
    ref = R.distance(V, T, X, table=d["table"])
    out = m.distance(X, closest=True, tri=True, feature=True)
    for k in R.KEYS:
        assert_bits(out[k], ref[k], f"{name}: {k}")
    assert_bits(m.distance(X, brute=True)["sdf"], ref["sdf"], "brute")
    w = m.winding(X, beta=2.0)["winding"]
    assert_bits(w, WR.winding(V, T, X, 2.0, d["nodes"], d["order"], d["moments"]), f"{name}: winding")
    wb = m.winding(X, brute=True)["winding"]
    assert_bits(wb, WR.winding(V, T, X, 2.0, d["nodes"], d["order"], d["moments"], brute=True), f"{name}: winding, brute")
    # against the host-built mesh: everything but the sign is a function of the triangles alone
    with nr.TriMesh(owner, V, T, leaf=leaf) as h:
        host = h.distance(X, closest=True, tri=True, feature=True)
    for k in ("closest", "tri", "feature"):
        assert_bits(out[k], host[k], f"{name}: {k} against the host build")
    assert_bits(np.abs(out["sdf"]), np.abs(host["sdf"]), "|sdf| against the host build")


@pytest.mark.parametrize("name,leaf", QUERIED)
def test_rays(owner, built, name, leaf):
    V, T = DR.mesh(name)
    m = built(name, leaf)
    d = m.download()
    O, D = MR.rays(PARENT[name])
    ref, _ = MR.walk(d["nodes"], d["order"], V, T, O, D, table=d["table"])
    out = m.trace_rays(O, D, bary=True)
    for k in MR.KEYS:
        assert_bits(out[k], ref[k], f"{name}: {k}")
    with nr.TriMesh(owner, V, T, leaf=leaf) as h:
        host = h.trace_rays(O, D, bary=True)
    for k in ("status", "t", "tri", "bary", "position"):
        assert_bits(out[k], host[k], f"{name}: {k} against the host build")


@pytest.mark.parametrize("name,leaf", QUERIED)
def test_samples_and_lattice(owner, built, monkeypatch, name, leaf):
    V, T = DR.mesh(name)
    m = built(name, leaf)
    d = m.download()
    # sample_ref.sample with the device-built mesh's own table (blocks of 256, not one running sum)
    monkeypatch.setattr(SR, "area_table", lambda V, T, order: (d["thresholds"], d["area_last"]))
    ref = SR.sample(V, T, d["order"], 7, 700, 100, sigma=0.01, lo=-1.0, hi=1.0)
    out = m.sample(700, 100, seed=7, sigma=0.01, lo=-1.0, hi=1.0)
    for k in ("points", "tri", "bary"):
        assert_bits(out[k], ref[k], f"{name}: sample {k}")
    lo, hi = V.min(0) - F(0.2), V.max(0) + F(0.15)
    dims = (13, 11, 9)
    step = ((hi - lo) / (np.array(dims, F) - 1)).astype(F)
    grid = m.sample_grid(lo, step, dims)
    idx = np.stack(np.meshgrid(np.arange(dims[2]), np.arange(dims[1]), np.arange(dims[0]), indexing="ij"), -1).reshape(-1, 3)
    P = (lo[None] + idx[:, ::-1].astype(F) * step[None]).astype(F)
    assert_bits(grid.reshape(-1), m.distance(P)["sdf"], f"{name}: the lattice against the point call")


# ---- errors and memory ----------------------------------------------------------------------------------

def test_invalid_meshes_and_recovery(owner):
    V, T = DR.mesh("torus")
    bad = []
    Tb = T.copy(); Tb[len(T) // 2, 1] = len(V); bad.append((V, Tb))
    Tb = T.copy(); Tb[-1, 2] = -1; bad.append((V, Tb))
    Vb = V.copy(); Vb[len(V) // 3, 1] = np.nan; bad.append((Vb, T))
    Vb = V.copy(); Vb[-1, 0] = np.inf; bad.append((Vb, T))
    for Vx, Tx in bad:
        for make in (lambda: from_device(owner, Vx, Tx, 8), lambda: nr.TriMesh(owner, Vx, Tx, build="device")):
            with pytest.raises(nr.NRError) as e:
                make()
            assert e.value.code == -1
        # ... and the next build on the same context is whole
        with from_device(owner, V, T, 8) as m:
            assert_bits(m.download()["nodes"], DR.reference("torus", 8)["nodes"], "nodes after a failure")


def test_create_destroy_keeps_no_memory(owner):
    """hipMemGetInfo before and after twenty builds of a mesh whose table alone is 551 KB: a leaked object
    would show as 11 MB; 1 MiB is allowed for what else moves.  The first build sizes the context's scratch."""
    V, T = DR.mesh("fine_torus")
    dV, dT = torch.from_numpy(V.copy()).cuda(), torch.from_numpy(T.copy()).cuda()
    torch.cuda.synchronize()
    nr.TriMesh.from_device(owner, dV.data_ptr(), len(V), dT.data_ptr(), len(T)).close()
    before = torch.cuda.mem_get_info()[0]
    for _ in range(20):
        nr.TriMesh.from_device(owner, dV.data_ptr(), len(V), dT.data_ptr(), len(T)).close()
    after = torch.cuda.mem_get_info()[0]
    assert before - after <= 1 << 20, (before, after)
