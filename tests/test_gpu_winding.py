"""nr_mesh_winding on the GPU (nr_winding.hip) against tests/winding_ref.py, the numpy restatement of the
contract in include/neural_render.h (pinned by tests/test_winding_cpu.py), walking the tree
nr_mesh_hierarchy exports.  The contract is bit-exactness: every comparison is on uint32 views."""
import ctypes

import numpy as np
import pytest
import torch

import cudaneuralrender_amd as nr
import trimesh_ref as R
import winding_ref as WR

pytestmark = pytest.mark.gpu
NP = R.NP
F = np.float32
# where torch bundles a HIP runtime of its own beside libnr's, torch has to open the GPU first
if torch.cuda.is_available():
    torch.cuda.init()

# (mesh, leaf): a single leaf; every leaf one triangle; ragged leaves; an open mesh; one that cuts itself
CASES = [("tetrahedron", 8), ("cube", 1), ("torus", 8), ("torus", 3), ("open_torus", 8), ("double_cube", 2)]


@pytest.fixture(scope="module")
def owner():
    with nr.Renderer(0) as r:
        yield r


def same(a, b):
    a, b = R.bits(a), R.bits(b)
    assert a.shape == b.shape
    assert np.array_equal(a, b), f"{int((a != b).sum())} of {a.size} words differ"


@pytest.mark.parametrize("name, leaf", CASES)
def test_against_restatement(owner, name, leaf):
    V, T = WR.mesh(name)
    X = WR.points(name)
    brute = WR.reference(name, leaf, 2.0, True)
    with nr.TriMesh(owner, V, T, leaf=leaf) as m:
        assert m.info()["nodes"] == len(WR.tree(name, leaf)[0])
        for beta in (2.0, 4.0):
            out, st = m.winding(X, beta=beta, with_stats=True)
            assert list(out) == ["winding"]
            same(out["winding"], WR.reference(name, leaf, beta))
            assert st["ray_steps"] == NP and 0 < st["shade_evals"] <= NP * len(T) and st["launches"] > 0 and st["ms_total"] > 0
            out, st = m.winding(X, beta=beta, brute=True, with_stats=True)
            same(out["winding"], brute)
            assert st["shade_evals"] == NP * len(T)
        # beta = 0 is 2.0
        same(m.winding(X)["winding"], WR.reference(name, leaf, 2.0))
    if name == "torus":
        assert not np.array_equal(R.bits(WR.reference(name, leaf, 2.0)), R.bits(brute)), "no node was ever far: nothing tested"


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sizes(owner, n):
    """a lone point, a chunk short of one lane, a full chunk, a chunk and a tail of one: each point's bits
    are those it has among all 1063"""
    V, T = WR.mesh("open_torus")
    X = WR.points("open_torus")
    with nr.TriMesh(owner, V, T, leaf=8) as m:
        same(m.winding(X[:n])["winding"], WR.reference("open_torus", 8, 2.0)[:n])
        same(m.winding(X[:n], brute=True)["winding"], WR.reference("open_torus", 8, 2.0, True)[:n])


def test_sdf_output(owner):
    """sdf: nr_trimesh_distance's magnitude, bit for bit, with the sign of w >= 0.5"""
    for name in ("torus", "open_torus"):
        V, T = WR.mesh(name)
        X = WR.points(name)
        with nr.TriMesh(owner, V, T) as m:
            d = m.distance(X)["sdf"]
            for brute in (False, True):
                out, st = m.winding(X, sdf=True, brute=brute, with_stats=True)
                w = out["winding"]
                same(w, WR.reference(name, 8, 2.0, brute))
                same(np.abs(out["sdf"]), np.abs(d))
                assert np.array_equal(np.signbit(out["sdf"]), w >= 0.5)
                assert (w >= 0.5).any() and (w < 0.5).any()
                assert st["launches"] == 3
                if brute:
                    assert st["shade_evals"] == 2 * NP * len(T)
            if name == "torus":  # closed: the two signs agree off the surface
                off = np.abs(d) > 1e-4
                assert np.array_equal(out["sdf"][off], d[off])
            else:
                assert (np.signbit(out["sdf"]) != np.signbit(d)).any(), "the open mesh should flip some pseudonormal sign"


def test_device_pointers(owner):
    V, T = WR.mesh("open_torus")
    X = WR.points("open_torus")
    ref = WR.reference("open_torus", 8, 2.0)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(np.array(X)).to(dev)
    w = torch.full((NP,), 7.0, dtype=torch.float32, device=dev)
    sdf = torch.full((NP,), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with nr.TriMesh(owner, V, T) as m:
        host = m.winding(X, sdf=True)
        st = m.winding_device(x.data_ptr(), NP, w.data_ptr(), sdf.data_ptr(), with_stats=True)
        assert st["ray_steps"] == NP
        same(w.cpu().numpy(), ref)
        same(w.cpu().numpy(), host["winding"])
        same(sdf.cpu().numpy(), host["sdf"])
        # only the outputs asked for are written, and only n of them
        w.fill_(7.0)
        sdf.fill_(7.0)
        torch.cuda.synchronize()
        assert m.winding_device(x.data_ptr(), 100, sdf_ptr=sdf.data_ptr()) is None
        owner.synchronize()
        same(sdf.cpu().numpy()[:100], host["sdf"][:100])
        assert (sdf[100:] == 7.0).all() and (w == 7.0).all()
        m.winding_device(x.data_ptr(), 100, winding_ptr=w.data_ptr(), beta=4.0)
        owner.synchronize()
        same(w.cpu().numpy()[:100], WR.reference("open_torus", 8, 4.0)[:100])
        assert (w[100:] == 7.0).all()


def test_device_call_only_enqueues(owner):
    """With NR_DEVICE and no stats the call returns without a stream sync: on a caller's stream that is
    still busy with tens of milliseconds of earlier work, the call comes back with the stream not yet
    idle (a call that synchronised would leave it idle), and its results are there after the sync."""
    V, T = WR.mesh("torus")
    X = WR.points("torus")
    dev = torch.device("cuda:0")
    x = torch.from_numpy(np.array(X)).to(dev)
    w = torch.full((NP,), 7.0, dtype=torch.float32, device=dev)
    sdf = torch.full((NP,), 7.0, dtype=torch.float32, device=dev)
    a = torch.ones((4096, 4096), dtype=torch.float32, device=dev)
    a @ a  # (the first product loads its kernel)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    with nr.TriMesh(owner, V, T) as m:
        try:
            with torch.cuda.stream(stream):
                owner.set_stream(stream.cuda_stream)
                for _ in range(24):
                    b = a @ a
                m.winding_device(x.data_ptr(), NP, w.data_ptr(), sdf.data_ptr())
                busy = not stream.query()
                owner.synchronize()
            stream.synchronize()
        finally:
            owner.set_stream(None, own=True)
        assert busy, "the stream was idle when the call returned: it waited"
        same(w.cpu().numpy(), WR.reference("torus", 8, 2.0))
        same(sdf.cpu().numpy(), m.winding(X, sdf=True)["sdf"])
    del b


def mixed_chunk():
    """64 points of the open torus' set: far ones (they take the root or its children), near ones (they
    reach leaves) and a non-finite one"""
    X = WR.points("open_torus")
    near = np.array(X[:40])
    rng = np.random.default_rng(41)
    d = rng.normal(size=(23, 3))
    far = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(4.0, 60.0, (23, 1))).astype(F)
    Y = np.concatenate([near[:20], far[:11], [[np.nan, 0.25, 0.5]], near[20:], far[11:]]).astype(F)
    assert Y.shape == (64, 3)
    return Y


def test_mixed_wave(owner):
    """one chunk whose lanes cut the tree at different heights: every point's bits are those of the same
    point asked alone, and of the chunk reversed -- a lane's sum depends on its own point only"""
    V, T = WR.mesh("open_torus")
    Y = mixed_chunk()
    nodes, order, moments, _ = WR.tree("open_torus", 8)
    ref, evals = WR.winding(V, T, Y, 2.0, nodes, order, moments, count_evals=True)
    # the chunk is mixed: some points take the root itself, some sum hundreds of triangles
    each = [WR.winding(V, T, Y[i:i + 1], 2.0, nodes, order, moments, count_evals=True)[1] for i in range(64)]
    assert each.count(1) >= 20 and max(each) > 100 and each[31] == 0 and sum(each) == evals
    with nr.TriMesh(owner, V, T) as m:
        out, st = m.winding(Y, with_stats=True)
        w = out["winding"]
        same(w, ref)
        assert R.bits(w)[31] == 0x7fc00000 and st["shade_evals"] == evals
        same(m.winding(Y[::-1])["winding"], ref[::-1])
        for i in range(64):
            same(m.winding(Y[i:i + 1])["winding"], ref[i:i + 1])


def test_non_finite_points(owner):
    V, T = WR.mesh("torus")
    X = WR.points("torus")
    Y = np.array(X[:192])
    bad = {3: (np.nan, 0, 0), 17: (0, np.inf, 0), 64: (0, 0, -np.inf), 70: (np.nan, np.nan, np.nan), 127: (np.inf, -np.inf, 1),
           130: (1e30, np.nan, 0)}
    for i, v in bad.items():
        Y[i] = v
    Y[128] = (3e38, -3e38, 3e38)  # finite
    dead = np.zeros(len(Y), bool)
    dead[list(bad)] = True
    nodes, order, moments, _ = WR.tree("torus", 3)
    with nr.TriMesh(owner, V, T, leaf=3) as m:
        for brute in (False, True):
            out = m.winding(Y, sdf=True, brute=brute)
            ref = WR.winding(V, T, Y, 2.0, nodes, order, moments, brute=brute)
            same(out["winding"], ref)
            assert (R.bits(out["winding"][dead]) == 0x7fc00000).all() and (R.bits(out["sdf"][dead]) == 0x7fc00000).all()
            keep = ~dead & (np.arange(len(Y)) != 128)
            same(out["winding"][keep], WR.reference("torus", 3, 2.0, brute)[:192][keep])
            assert np.isfinite(out["winding"][128])


def test_degenerate_triangles(owner):
    """Three zero-area triangles appended to the torus take no part: the tree is the torus' own (the added
    vertex belongs to no live triangle, so no moment moves -- tests/test_winding_cpu.py compares the
    trees), and the values are the torus' bit for bit.  A mesh of nothing else gives the quiet NaN."""
    V2, T2 = R.degenerate_torus()
    X = WR.points("torus")
    with nr.TriMesh(owner, V2, T2, leaf=3) as m:
        for brute in (False, True):
            same(m.winding(X, brute=brute)["winding"], WR.reference("torus", 3, 2.0, brute))
    with nr.TriMesh(owner, V2, T2[-3:]) as m:
        for brute in (False, True):
            out = m.winding(X[:65], sdf=True, brute=brute)
            assert (R.bits(out["winding"]) == 0x7fc00000).all() and (R.bits(out["sdf"]) == 0x7fc00000).all()


@pytest.mark.parametrize("name, leaf", [("torus", 3), ("open_torus", 8)])
def test_no_node_far_equals_brute(owner, name, leaf):
    V, T = WR.mesh(name)
    X = WR.points(name)
    with nr.TriMesh(owner, V, T, leaf=leaf) as m:
        a, st = m.winding(X, beta=1e15, with_stats=True)
        same(a["winding"], m.winding(X, brute=True)["winding"])
        same(a["winding"], WR.reference(name, leaf, 2.0, True))
        assert st["shade_evals"] == NP * len(T)


def test_stats(owner):
    V, T = WR.mesh("torus")
    X = WR.points("torus")
    nodes, order, moments, _ = WR.tree("torus", 8)
    # sorted along x, so that the 64 points of a walk are neighbours
    Xs = np.ascontiguousarray(X[np.argsort(X[:, 0], kind="stable")])
    with nr.TriMesh(owner, V, T) as m:
        _, st = m.winding(Xs, beta=2.0, with_stats=True)
        _, sb = m.winding(Xs, brute=True, with_stats=True)
    per_point = WR.winding(V, T, Xs, 2.0, nodes, order, moments, count_evals=True)[1]
    print(f"torus, beta 2: {st['shade_evals'] / NP:.1f} evaluations per point ({per_point / NP:.1f} if every point walked alone), "
          f"BRUTE {sb['shade_evals'] / NP:.0f}")
    assert sb["shade_evals"] == NP * len(T)
    assert 0 < st["shade_evals"] < NP * len(T)
    # lanes add only what their own point needs: the count is the restatement's, whatever the wave entered
    assert st["shade_evals"] == per_point
    assert all(st[k] == 0 for k in ("rays_hit", "rays_shaded", "iterations", "endgame_evals", "endgame_switches"))


def test_invalid_arguments(owner):
    L = nr.lib()
    V, T = R.cube()
    ctx = owner._ctx
    X = np.zeros((4, 3), F)
    w = np.full(4, 7.0, F)
    sdf = np.full(4, 7.0, F)

    def call(mm, X_, n, beta, w_, s_, flags):
        return L.nr_mesh_winding(mm, None if X_ is None else X_.ctypes.data, n, beta, None if w_ is None else w_.ctypes.data,
                                 None if s_ is None else s_.ctypes.data, flags, 0, None)

    with nr.TriMesh(owner, V, T) as mesh:
        m = mesh._m
        for rc in (call(None, X, 4, 0.0, w, sdf, 0), call(m, None, 4, 0.0, w, sdf, 0), call(m, X, 0, 0.0, w, sdf, 0),
                   call(m, X, -1, 0.0, w, sdf, 0), call(m, X, (1 << 30) + 1, 0.0, w, sdf, 0), call(m, X, 4, 0.0, w, sdf, 2),
                   call(m, X, 4, 0.0, w, sdf, 1 | 4), call(m, X, 4, -1.0, w, sdf, 0), call(m, X, 4, float("nan"), w, sdf, 0),
                   call(m, X, 4, float("inf"), w, sdf, 0), call(m, X, 4, 2.0, None, None, 0)):
            assert rc == -1
            assert (w == 7.0).all() and (sdf == 7.0).all()
        assert "NULL" in L.nr_last_error(ctx).decode()
        assert call(m, X, 4, -0.0, w, None, 0) == 0 and (sdf == 7.0).all() and not (w == 7.0).any()
        assert call(m, X, 4, 3.0, None, sdf, 1) == 0 and not (sdf == 7.0).any()
