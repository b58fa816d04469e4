"""nr_mesh_trace_rays, nr_mesh_gbuffer and nr_mesh_render on the GPU (nr_mesh_rays.hip) against
tests/mesh_ray_ref.py, the numpy restatement of the ray contract in include/neural_render.h (pinned by
tests/test_mesh_rays_cpu.py).  The contract is bit-exactness: every comparison is on uint32 views."""
import numpy as np
import pytest
import torch

import cudaneuralrender_amd as nr
import designed_nets
import mesh_ray_ref as M
import query_ref
import trimesh_ref as R

pytestmark = pytest.mark.gpu
KEYS = M.KEYS
NR = M.NR
F = np.float32
# where torch bundles a HIP runtime of its own beside libnr's, torch has to open the GPU first
if torch.cuda.is_available():
    torch.cuda.init()

# (mesh, leaf): a single leaf and no inner node; the deepest tree, every leaf one triangle; ragged leaves
CASES = [("tetrahedron", 8), ("cube", 1), ("torus", 8), ("torus", 3)]
ALL = dict(tri=True, bary=True, position=True, normal=True)
VIEW = (-35.0, 30.0, 1.7)  # a set_camera(rx, ry, zoom) view beside the default one


@pytest.fixture(scope="module")
def owner():
    with nr.Renderer(0) as r:
        yield r


def same(out, ref, sl=slice(None), keys=KEYS):
    for k in keys:
        a, b = M.bits(out[k]), M.bits(np.asarray(ref[k])[sl])
        assert a.shape == b.shape, k
        assert np.array_equal(a, b), f"{k}: {int((a != b).sum())} of {a.size} words differ"


@pytest.mark.parametrize("name, leaf", CASES)
def test_against_restatement(owner, name, leaf):
    V, T = R.mesh(name)
    O, D = M.rays(name)
    with nr.TriMesh(owner, V, T, leaf=leaf) as m:
        for window, (tmin, tmax) in enumerate(M.WINDOWS):
            for smooth in (False, True):
                ref, counts = M.reference(name, window, smooth)
                hits = int((ref["status"] == M.HIT).sum())
                assert 100 < hits < NR
                out, st = m.trace_rays(O, D, tmin, tmax, smooth=smooth, with_stats=True, **ALL)
                same(out, ref)
                brute, bst = m.trace_rays(O, D, tmin, tmax, smooth=smooth, brute=True, with_stats=True, **ALL)
                same(brute, ref)
                for s in (st, bst):
                    assert s["ray_steps"] == NR and s["rays_hit"] == hits and s["launches"] > 0 and s["ms_total"] > 0
                    assert all(s[k] == 0 for k in ("rays_shaded", "iterations", "endgame_evals", "endgame_switches"))
                assert bst["shade_evals"] == counts["live_rays"] * counts["live_tris"]
                if name == "tetrahedron":  # one leaf: the walk is brute force
                    assert st["shade_evals"] == bst["shade_evals"]
                else:
                    assert 0 < st["shade_evals"] < bst["shade_evals"]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sizes(owner, n):
    """a lone ray, a chunk short of one lane, a full chunk, a chunk and a tail of one"""
    V, T = R.torus()
    O, D = M.rays("torus")
    ref, _ = M.reference("torus")
    with nr.TriMesh(owner, V, T, leaf=3) as m:
        same(m.trace_rays(O[:n], D[:n], **ALL), ref, slice(0, n))
        same(m.trace_rays(O[:n], D[:n], brute=True, **ALL), ref, slice(0, n))


def test_degenerate_triangles(owner):
    """three zero-area triangles appended to the torus are never hit; a mesh of nothing else gives MISS"""
    V2, T2 = R.degenerate_torus()
    O, D = M.rays("degenerate_torus")
    ref, counts = M.reference("degenerate_torus")
    assert counts["live_tris"] == len(T2) - 3
    with nr.TriMesh(owner, V2, T2, leaf=3) as m:
        for brute in (False, True):
            same(m.trace_rays(O, D, brute=brute, **ALL), ref)
    with nr.TriMesh(owner, V2, T2[-3:]) as m:
        for brute in (False, True):
            out, st = m.trace_rays(O[:65], D[:65], brute=brute, with_stats=True, **ALL)
            assert (out["status"] == M.MISS).all() and (out["tri"] == -1).all()
            assert all((M.bits(out[k]) == 0).all() for k in ("t", "bary", "position", "normal"))
            assert st["rays_hit"] == 0 and st["shade_evals"] == 0


def test_device_pointers_and_any_hit(owner):
    V, T = R.torus()
    O, D = M.rays("torus")
    ref, _ = M.reference("torus")
    dev = torch.device("cuda:0")
    o, d = torch.from_numpy(np.array(O)).to(dev), torch.from_numpy(np.array(D)).to(dev)
    bufs = {"status": torch.full((NR,), 7, dtype=torch.int32, device=dev), "t": torch.full((NR,), 7.0, device=dev),
            "tri": torch.full((NR,), 7, dtype=torch.int32, device=dev), "bary": torch.full((NR, 3), 7.0, device=dev),
            "position": torch.full((NR, 3), 7.0, device=dev), "normal": torch.full((NR, 3), 7.0, device=dev)}
    torch.cuda.synchronize()
    with nr.TriMesh(owner, V, T, leaf=3) as m:
        st = m.trace_rays_device(o.data_ptr(), d.data_ptr(), NR, with_stats=True,
                                 **{k + "_ptr": b.data_ptr() for k, b in bufs.items()})
        assert st["ray_steps"] == NR and st["rays_hit"] == int((ref["status"] == M.HIT).sum())
        same({k: b.cpu().numpy() for k, b in bufs.items()}, ref)
        # only the outputs asked for are written
        for b in bufs.values():
            b.fill_(7)
        torch.cuda.synchronize()
        m.trace_rays_device(o.data_ptr(), d.data_ptr(), 100, tri_ptr=bufs["tri"].data_ptr(), bary_ptr=bufs["bary"].data_ptr())
        owner.synchronize()
        same({k: bufs[k].cpu().numpy()[:100] for k in ("tri", "bary")}, ref, slice(0, 100), ("tri", "bary"))
        assert (bufs["tri"][100:] == 7).all() and (bufs["bary"][100:] == 7).all()
        assert all((bufs[k] == 7).all() for k in ("status", "t", "position", "normal"))
        # any hit: the status of closest hit, window by window, nothing else written
        for window, (tmin, tmax) in enumerate(M.WINDOWS):
            want = M.reference("torus", window)[0]["status"]
            for brute in (False, True):
                bufs["status"].fill_(7)
                torch.cuda.synchronize()
                st = m.trace_rays_device(o.data_ptr(), d.data_ptr(), NR, tmin, tmax, status_ptr=bufs["status"].data_ptr(),
                                         any_hit=True, brute=brute, with_stats=True)
                assert np.array_equal(bufs["status"].cpu().numpy(), want)
                assert st["rays_hit"] == int((want == M.HIT).sum())
            out, ast = m.trace_rays(O, D, tmin, tmax, any_hit=True, with_stats=True)
            assert list(out) == ["status"] and np.array_equal(out["status"], want)
            assert 0 < ast["shade_evals"] <= m.trace_rays(O, D, tmin, tmax, with_stats=True)[1]["shade_evals"]
        assert all((bufs[k] == 7).all() for k in ("t", "position", "normal"))


def test_invalid_arguments(owner):
    L = nr.lib()
    V, T = R.cube()
    z = np.zeros((4, 3), F)
    st = np.zeros(4, np.int32)
    t = np.zeros(4, F)
    px = np.zeros(16, np.uint32)
    nan, inf = float("nan"), float("inf")
    with nr.TriMesh(owner, V, T) as mesh:
        m = mesh._m

        def rays(o=z, d=z, n=4, tmin=0.0, tmax=inf, flags=0, t_=None, normal=None):
            return L.nr_mesh_trace_rays(m, None if o is None else o.ctypes.data, None if d is None else d.ctypes.data, n, tmin,
                                        tmax, st.ctypes.data, None if t_ is None else t_.ctypes.data, None, None, None,
                                        None if normal is None else normal.ctypes.data, flags, 0, None)

        for rc in (rays(o=None), rays(d=None), rays(n=0), rays(n=-1), rays(n=(1 << 30) + 1), rays(tmin=nan), rays(tmax=nan),
                   rays(tmin=1.0, tmax=0.5), rays(flags=8), rays(flags=2 | 4), rays(flags=2, t_=t), rays(flags=2, normal=z)):
            assert rc == -1
        assert "NR_MESH_RAY_ANY" in L.nr_last_error(owner._ctx).decode()
        for rc in (rays(), rays(tmin=-inf, tmax=inf), rays(tmin=0.5, tmax=0.5), rays(flags=2), rays(flags=1 | 2), rays(flags=1 | 4, t_=t)):
            assert rc == 0
        # every output NULL is allowed: the call runs and writes nothing
        assert L.nr_mesh_trace_rays(m, z.ctypes.data, z.ctypes.data, 4, 0.0, 1.0, None, None, None, None, None, None, 0, 0, None) == 0

        def gbuf(W, H, flags=0, t_=None):
            return L.nr_mesh_gbuffer(m, W, H, st.ctypes.data, None if t_ is None else t_.ctypes.data, None, None, None, None,
                                     flags, 0, None)

        for rc in (gbuf(0, 2), gbuf(2, 0), gbuf(1 << 16, (1 << 14) + 1), gbuf(2, 2, 8), gbuf(2, 2, 2, t), gbuf(2, 2, 2 | 4)):
            assert rc == -1
        assert gbuf(2, 2) == 0 and gbuf(2, 2, 2) == 0
        for rc in (L.nr_mesh_render(m, None, 4, 4, 0, 0, None), L.nr_mesh_render(m, px.ctypes.data, 0, 4, 0, 0, None),
                   L.nr_mesh_render(m, px.ctypes.data, 4, 0, 0, 0, None), L.nr_mesh_render(m, px.ctypes.data, 4, 4, 2, 0, None),
                   L.nr_mesh_render(m, px.ctypes.data, 4, 4, 8, 0, None)):
            assert rc == -1
        assert L.nr_mesh_render(m, px.ctypes.data, 4, 4, 4, 0, None) == 0
    # matcap colouring without a matcap: nr_render's state error
    with nr.Renderer(0) as r, nr.TriMesh(r, V, T) as mesh:
        r.set_static(nr.NR_COLOR_MATCAP, 3)
        with pytest.raises(nr.NRError) as e:
            mesh.render(4, 4)
        assert e.value.code == -5  # NR_E_STATE
        assert "status" in mesh.gbuffer(4, 4)


@pytest.mark.parametrize("name", ["tetrahedron", "cube", "torus"])
def test_watertight(owner, name):
    """the rays of test_mesh_rays_cpu.test_watertight: every one hits, with the hierarchy and without"""
    V, T = R.mesh(name)
    with nr.TriMesh(owner, V, T, leaf=3) as m:
        for moved in (False, True):
            O, D = M.watertight_rays(name, moved)
            for kw in ({}, {"brute": True}, {"any_hit": True}):
                assert (m.trace_rays(O, D, **kw)["status"] == M.HIT).all()


@pytest.mark.parametrize("view", [None, VIEW])
@pytest.mark.parametrize("W, H", [(8, 8), (1, 1), (37, 29)])
def test_gbuffer(W, H, view):
    """nr_mesh_gbuffer is nr_mesh_trace_rays on nr_render's pixel rays, and the restatement: one full
    tile, one pixel, ragged tiles in both axes with divisors that are no powers of two."""
    V, T = R.torus()
    with nr.Renderer(0) as r, nr.TriMesh(r, V, T) as m:
        iv = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 2], F)
        if view is not None:
            r.set_camera(*view)
            iv = nr.camera(*view)[0]
        O, D = query_ref.pixel_rays(W, H, iv)
        for smooth in (False, True):
            g, st = m.gbuffer(W, H, smooth=smooth, with_stats=True, **ALL)
            flat = {k: v.reshape((W * H,) + v.shape[2:]) for k, v in g.items()}
            same(flat, m.trace_rays(O, D, smooth=smooth, **ALL))
            ref, _ = M.trace(V, T, O, D, smooth=smooth)
            same(flat, ref)
            assert st["ray_steps"] == W * H and st["rays_hit"] == int((ref["status"] == M.HIT).sum())
        same({k: v.reshape((W * H,) + v.shape[2:]) for k, v in m.gbuffer(W, H, brute=True, **ALL).items()},
             M.trace(V, T, O, D)[0])
        if W * H > 1:
            assert 0 < (ref["status"] == M.HIT).sum() < W * H
        assert np.array_equal(m.gbuffer(W, H, any_hit=True)["status"].reshape(-1), ref["status"])


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("color", ["facing", "matcap"])
def test_render(color, smooth):
    """nr_mesh_render at 37 x 29 against the restated colours: shade_color of the G-buffer's normal and
    the pixel's ray; with a coded matcap a wrong texel shows.  Background pixels are exactly 0."""
    W, H = 37, 29
    V, T = R.torus()
    tex = designed_nets.coded_matcap(23, 41)
    with nr.Renderer(0) as r, nr.TriMesh(r, V, T, leaf=3) as m:
        r.set_camera(*VIEW)
        iv, nm = nr.camera(*VIEW)
        if color == "matcap":
            r.set_matcap(tex).set_static(nr.NR_COLOR_MATCAP, 3)
        img, st = m.render(W, H, smooth=smooth)
        dev = torch.full((H, W), 7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        m.render_device(dev.data_ptr(), W, H, smooth=smooth)
        r.synchronize()
    O, D = query_ref.pixel_rays(W, H, iv)
    ref, _ = M.trace(V, T, O, D, smooth=smooth)
    want = M.facing(ref["normal"], D, ref["status"]) if color == "facing" else M.matcap(ref["normal"], ref["status"], nm, tex)
    hit = ref["status"] == M.HIT
    assert img.shape == (H, W) and img.dtype == np.uint32
    assert np.array_equal(img.reshape(-1), want)
    assert np.array_equal(dev.cpu().numpy().view(np.uint32).reshape(-1), want)
    assert 100 < hit.sum() < W * H and (img.reshape(-1)[~hit] == 0).all() and (want[hit] != 0).all()
    assert len(np.unique(want[hit])) > 8
    assert st["ray_steps"] == W * H and st["rays_hit"] == int(hit.sum())


IOU_MEASURED = 0.3921
IOU_FLOOR = IOU_MEASURED - 0.05


def _iou(a, b):
    return float((a & b).sum()) / float((a | b).sum())


def test_against_network():
    """The mesh that extract_mesh takes from plane_1 (scene tanh, 32^3 over [-1, 1]^3) through
    TriMesh.gbuffer against the network itself through Renderer.render_gbuffer, 64 x 64, the suite's
    view of plane_1 (designed_nets.MATCAP_VIEW).  Where both hit, the median |dt| is at most one
    lattice step, 2 / 31 = 0.0645 (the mesh's vertices lie on the cell edges the surface crosses).
    Measured on the first run: network 1,367 px, mesh 536 px, median |dt| = 0.0357, silhouette IoU =
    0.3921 -- plane_1 is nowhere two steps of a 32^3 lattice thick, so the lattice loses most of the
    wings; the floor is that minus 0.05 = 0.3421.  (Seen end-on through the default camera the two
    silhouettes are 132 and 64 px and layers overlap in depth: too few pixels to say anything.)"""
    from test_gpu_trimesh import plane_mesh
    V, T, _, _, step = plane_mesh()
    W = H = 64
    with nr.Renderer(0) as r:
        r.load_h5(nr.geometry_path("plane_1")).set_precision("fp32").set_scene("tanh")
        r.set_camera(*designed_nets.MATCAP_VIEW[3])  # the suite's view of plane_1: from above and the side, frame-filling
        net = r.render_gbuffer(W, H, normals=False)
        with nr.TriMesh(r, V, T) as m:
            mesh = m.gbuffer(W, H)
            smooth = m.gbuffer(W, H, smooth=True)
    a, b = net["status"] == query_ref.HIT, mesh["status"] == M.HIT
    both = a & b
    dt = np.abs(net["t"][both] - mesh["t"][both])
    iou = _iou(a, b)
    print(f"plane_1 at 32^3, 64 x 64: network {int(a.sum())} px, mesh {int(b.sum())} px, IoU {iou:.4f}, "
          f"median |dt| {np.median(dt):.5f} (a lattice step is {step:.5f})")
    assert both.sum() > 200
    assert np.median(dt) <= step
    assert iou >= IOU_FLOOR
    # the smooth normals are unit vectors near the flat ones
    h = b.reshape(-1)
    ns, nf = smooth["normal"].reshape(-1, 3)[h], mesh["normal"].reshape(-1, 3)[h]
    assert np.abs(np.linalg.norm(ns, axis=1) - 1).max() < 1e-5 and np.median((ns * nf).sum(1)) > 0.9
