"""nr_mesh_sample, nr_points_order and nr_mesh_fit_samples on the GPU (nr_sample.hip, nr_sort.hip) against
tests/sample_ref.py, the numpy restatement of the contract in include/neural_render.h (pinned by
tests/test_sample_cpu.py).  The contract is bit-exactness: every comparison is on uint32 views."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import cudaneuralrender_amd as nr
from cudaneuralrender_amd import _lib
import sample_ref as S
import trimesh_ref as R
import winding_ref as WR

pytestmark = pytest.mark.gpu
F = np.float32
# where torch bundles a HIP runtime of its own beside libnr's, torch has to open the GPU first
if torch.cuda.is_available():
    torch.cuda.init()

SEED = 0x9e3779b97f4a7c15  # the high word is not zero
LO, HI = (-1.3, -1.3, -1.3), (1.3, 1.3, 1.3)
TILE = 2048       # nr_kernels.h SORT_TILE: keys per workgroup
SCAN_STEP = 4096  # nr_kernels.h SORT_SCAN_STEP: table entries (256 per workgroup) per step of the scan
# one key; a wave short of one, full, and one over; a tile short of one, full, and one over; three tiles and a
# ragged fourth; 18 workgroups: a table of 4608 entries, two steps of the scan
SIZES = (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 17 * TILE + 5)
assert 256 * -(-SIZES[-1] // TILE) > SCAN_STEP

MESHES = {"torus": R.torus, "degenerate_torus": R.degenerate_torus, "tetrahedron": R.tetrahedron, "open_cube": WR.open_cube}


@pytest.fixture(scope="module")
def owner():
    with nr.Renderer(0) as r:
        yield r


def same(a, b):
    a, b = R.bits(a), R.bits(b)
    assert a.shape == b.shape
    assert np.array_equal(a, b), f"{int((a != b).sum())} of {a.size} words differ"


@functools.lru_cache(maxsize=None)
def mesh(name):
    V, T = MESHES[name]()
    return np.array(V, F), np.array(T, np.int32)


@functools.lru_cache(maxsize=None)
def tree(name, leaf=0):
    return nr.trimesh_hierarchy(*mesh(name), leaf=leaf)


def splits(n):
    """(n_surface, n_volume): all on the surface, all in the box, and both"""
    return [(n, 0), (0, n)] + ([(n - n // 2, n // 2)] if n > 1 else [])


# ---- nr_mesh_sample ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["torus", "degenerate_torus"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4099])
def test_sample_against_restatement(owner, name, n):
    V, T = mesh(name)
    order = tree(name)[1]
    with nr.TriMesh(owner, V, T) as m:
        for sigma in (0.0, 0.03):
            for ns, nv in splits(n):
                ref = S.sample(V, T, order, SEED, ns, nv, sigma, LO, HI)
                out, st = m.sample(ns, nv, seed=SEED, sigma=sigma, lo=LO, hi=HI, with_stats=True)
                for k in ("points", "tri", "bary"):
                    same(out[k], ref[k])
                assert st["ray_steps"] == n and st["launches"] == 1 and st["ms_total"] > 0
                if ns:
                    assert (out["tri"][:ns] >= 0).all() and (out["tri"][:ns] < len(R.torus()[1])).all()  # never a zero-area one
    # the outputs are optional
    with nr.TriMesh(owner, V, T) as m:
        out = m.sample(n, 0, seed=SEED, lo=LO, hi=HI, tri=False, bary=False)
        assert list(out) == ["points"]
        same(out["points"], S.sample(V, T, order, SEED, n, 0, 0.0, LO, HI)["points"])


def test_sample_seeds_leaves_and_box(owner):
    """a seed with a zero high word, a tetrahedron in one leaf, every triangle its own leaf, an uneven box"""
    lo, hi = (-1.0, 0.25, -3.0), (2.0, 0.5, 5.0)
    for name, leaf in (("tetrahedron", 8), ("tetrahedron", 1), ("torus", 3)):
        V, T = mesh(name)
        order = tree(name, leaf)[1]
        with nr.TriMesh(owner, V, T, leaf=leaf) as m:
            for seed in (7, SEED, 1 << 32):
                ref = S.sample(V, T, order, seed, 300, 200, 0.05, lo, hi)
                out = m.sample(300, 200, seed=seed, sigma=0.05, lo=lo, hi=hi)
                for k in ("points", "tri", "bary"):
                    same(out[k], ref[k])
    a = S.sample(V, T, order, 7, 64, 64, 0.05, lo, hi)["points"]
    assert not np.array_equal(a, S.sample(V, T, order, 1 << 32, 64, 64, 0.05, lo, hi)["points"])


def test_sample_device_pointers(owner):
    V, T = mesh("torus")
    n = 1000
    ref = S.sample(V, T, tree("torus")[1], SEED, 600, 400, 0.03, LO, HI)
    dev = torch.device("cuda:0")
    p = torch.full((n + 8, 3), 7.0, dtype=torch.float32, device=dev)
    t = torch.full((n + 8,), 7, dtype=torch.int32, device=dev)
    b = torch.full((n + 8, 3), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with nr.TriMesh(owner, V, T) as m:
        assert m.sample_device(p.data_ptr(), 600, 400, seed=SEED, sigma=0.03, lo=LO, hi=HI, tri_ptr=t.data_ptr(),
                               bary_ptr=b.data_ptr()) is None
        owner.synchronize()
        same(p.cpu().numpy()[:n], ref["points"])
        same(t.cpu().numpy()[:n], ref["tri"])
        same(b.cpu().numpy()[:n], ref["bary"])
        assert (p[n:] == 7.0).all() and (t[n:] == 7).all() and (b[n:] == 7.0).all()
        p.fill_(7.0); t.fill_(7)
        torch.cuda.synchronize()
        st = m.sample_device(p.data_ptr(), 600, 400, seed=SEED, sigma=0.03, lo=LO, hi=HI, with_stats=True)
        assert st["ray_steps"] == n
        same(p.cpu().numpy()[:n], ref["points"])
        assert (t == 7).all()


# ---- nr_points_order --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cloud(n):
    """n seeded points, most inside the box, some outside it on every side"""
    X = np.random.default_rng(100 + n).uniform(-1.5, 1.5, (n, 3)).astype(F)
    X.setflags(write=False)
    return X


def check_order(owner, X, lo=LO, hi=HI):
    keys = S.morton_keys(X, lo, hi)
    (perm, srt), st = owner.order_points(X, lo=lo, hi=hi, sorted_points=True, with_stats=True)
    same(perm, S.order(keys))
    same(srt, X[perm])
    assert st["ray_steps"] == len(X) and st["launches"] == 14 and st["ms_total"] > 0
    return perm


@pytest.mark.parametrize("n", SIZES)
def test_order_sizes(owner, n):
    X = cloud(n)
    perm = check_order(owner, X)
    # without `sorted`, and the same call twice: the same bits
    for _ in range(2):
        same(owner.order_points(X, lo=LO, hi=HI), perm)
    # shuffle mode, X NULL: 32-bit keys, the top digit included
    keys = S.shuffle_keys(SEED, n)
    assert n < 64 or keys.max() >= 1 << 30
    for _ in range(2):
        same(owner.order_points(None, n=n, mode="shuffle", seed=SEED), S.order(keys))
    # with X: sorted = X[perm]
    p, srt = owner.order_points(X, mode="shuffle", seed=SEED, sorted_points=True)
    same(p, S.order(keys))
    same(srt, X[p])
    if n > 64:
        assert not np.array_equal(owner.order_points(None, n=n, mode="shuffle", seed=SEED + 1), p)


@pytest.mark.parametrize("n", [65, TILE + 1, 3 * TILE + 17])
def test_order_is_stable(owner, n):
    """all keys equal: perm is the identity; two cells only: each cell's indices ascend"""
    X = np.tile(np.array([[0.25, -0.5, 0.75]], F), (n, 1))
    same(check_order(owner, X), np.arange(n, dtype=np.int32))
    X[::3] = (-0.6, 0.1, 0.2)
    perm = check_order(owner, X)
    k = S.morton_keys(X, LO, HI)
    assert len(np.unique(k)) == 2
    first = int((k == k.min()).sum())
    assert (np.diff(perm[:first]) > 0).all() and (np.diff(perm[first:]) > 0).all()


def test_order_sorted_reversed_and_odd_points(owner):
    n = 3 * TILE + 17
    X = cloud(n)
    asc = np.ascontiguousarray(X[S.order(S.morton_keys(X, LO, HI))])
    k = S.morton_keys(asc, LO, HI)
    assert (np.diff(k.astype(np.int64)) >= 0).all()
    same(check_order(owner, asc), np.arange(n, dtype=np.int32))  # already in order: ties keep their places
    check_order(owner, np.ascontiguousarray(asc[::-1]))
    # every point outside the box; non-finite coordinates (a NaN quantises to cell 0)
    check_order(owner, (cloud(n) * F(40.0) + F(3.0)).astype(F))
    Y = np.array(X)
    Y[5] = (np.nan, 0.0, 0.0)
    Y[64] = (np.nan, np.nan, np.nan)
    Y[TILE] = (np.inf, -np.inf, 0.5)
    Y[n - 1] = (0.1, np.nan, -0.2)
    Y[::7, 1] = np.nan
    assert S.morton_keys(Y, LO, HI)[64] == 0
    check_order(owner, Y)
    # an uneven box
    check_order(owner, X, lo=(-1.0, 0.0, -0.25), hi=(0.5, 1.5, 1.25))


def test_order_device_pointers(owner):
    n = TILE + 1
    X = cloud(n)
    ref = S.order(S.morton_keys(X, LO, HI))
    dev = torch.device("cuda:0")
    x = torch.from_numpy(np.array(X)).to(dev)
    perm = torch.full((n + 8,), -7, dtype=torch.int32, device=dev)
    srt = torch.full((n + 8, 3), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    assert owner.order_points_device(x.data_ptr(), n, perm.data_ptr(), lo=LO, hi=HI, sorted_ptr=srt.data_ptr()) is None
    owner.synchronize()
    same(perm.cpu().numpy()[:n], ref)
    same(srt.cpu().numpy()[:n], X[ref])
    assert (perm[n:] == -7).all() and (srt[n:] == 7.0).all()
    st = owner.order_points_device(None, n, perm.data_ptr(), mode="shuffle", seed=SEED, with_stats=True)
    assert st["launches"] == 13
    same(perm.cpu().numpy()[:n], S.order(S.shuffle_keys(SEED, n)))


# ---- nr_mesh_fit_samples ----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fit_reference(name, sign, ns, nv):
    X, Y = S.fit_samples(*mesh(name), tree(name), SEED, ns, nv, 0.03, LO, HI, sign)
    X.setflags(write=False)
    Y.setflags(write=False)
    return X, Y


@pytest.mark.parametrize("sign", ["normal", "winding"])
def test_fit_samples_torus(owner, sign):
    """(X, Y) = the three public calls composed by hand with numpy gathers = the restatement"""
    V, T = mesh("torus")
    ns = nv = 2048
    n = ns + nv
    with nr.TriMesh(owner, V, T) as m:
        X, Y, st = m.fit_samples(ns, nv, seed=SEED, sigma=0.03, lo=LO, hi=HI, sign=sign, with_stats=True)
        P = m.sample(ns, nv, seed=SEED, sigma=0.03, lo=LO, hi=HI, tri=False, bary=False)["points"]
        first, Ps = owner.order_points(P, lo=LO, hi=HI, sorted_points=True)
        Ys = m.distance(Ps)["sdf"] if sign == "normal" else m.winding(Ps, sdf=True)["sdf"]
        perm = owner.order_points(None, n=n, mode="shuffle", seed=SEED)
        same(X, Ps[perm])
        same(Y, Ys[perm])
        assert st["ray_steps"] == n and st["shade_evals"] > 0 and st["ms_total"] > 0
        assert st["launches"] == 5 + 26 + (sign == "winding")
    rx, ry = fit_reference("torus", sign, ns, nv)
    same(X, rx)
    same(Y, ry)
    assert (Y < 0).any() and (Y > 0).any() and np.isfinite(Y).all()
    # the surface half lies near the surface, the box half mostly does not
    assert 0.4 < (np.abs(Y) < 0.1).mean() < 0.9


def test_fit_samples_open_mesh(owner):
    """the cube without a face: the winding number signs what the pseudonormal cannot"""
    V, T = mesh("open_cube")
    ns = nv = 512
    with nr.TriMesh(owner, V, T) as m:
        Xn, Yn = m.fit_samples(ns, nv, seed=SEED, sigma=0.03, lo=LO, hi=HI, sign="normal")
        Xw, Yw = m.fit_samples(ns, nv, seed=SEED, sigma=0.03, lo=LO, hi=HI, sign="winding")
        Xb, Yb = m.fit_samples(ns, nv, seed=SEED, sigma=0.03, lo=LO, hi=HI, sign="winding", beta=4.0)
    same(Xn, Xw)
    same(np.abs(Yn), np.abs(Yw))
    assert (np.signbit(Yn) != np.signbit(Yw)).any()
    for sign, (X, Y) in (("normal", (Xn, Yn)), ("winding", (Xw, Yw))):
        rx, ry = fit_reference("open_cube", sign, ns, nv)
        same(X, rx)
        same(Y, ry)
    rx, ry = S.fit_samples(V, T, tree("open_cube"), SEED, ns, nv, 0.03, LO, HI, "winding", 4.0)
    same(Yb, ry)


def test_fit_samples_feed_a_fit(owner):
    """X and Y stay on the device and nr_fit_run takes them: the loss falls (sanity only)"""
    V, T = mesh("torus")
    n, batch = 1 << 14, 1 << 10
    dev = torch.device("cuda:0")
    x = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    y = torch.zeros(n, dtype=torch.float32, device=dev)
    loss = torch.zeros(n // batch, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rng = np.random.default_rng(31)
    dims = [3, 32, 32, 1]
    K = [rng.normal(0, 1.0 / np.sqrt(i), (i, o)).astype(F) for i, o in zip(dims[:-1], dims[1:])]
    B = [rng.normal(0, 0.1, o).astype(F) for o in dims[1:]]
    with nr.TriMesh(owner, V, T) as m, nr.Fit(owner, dims, K, B, lr=1e-3) as f:
        m.fit_samples_device(x.data_ptr(), y.data_ptr(), n // 2, n // 2, seed=SEED, sigma=0.03, lo=LO, hi=HI)
        hist = []
        for _ in range(4):  # 64 steps
            f.run_device(x.data_ptr(), y.data_ptr(), n, batch, loss.data_ptr())
            owner.synchronize()
            hist += loss.cpu().tolist()
    assert len(hist) == 64 and np.isfinite(hist).all()
    assert hist[49] < hist[0], (hist[0], hist[49])
    hx, hy = None, None
    with nr.TriMesh(owner, V, T) as m:
        hx, hy = m.fit_samples(n // 2, n // 2, seed=SEED, sigma=0.03, lo=LO, hi=HI)
    same(x.cpu().numpy(), hx)
    same(y.cpu().numpy(), hy)


def test_device_call_only_enqueues(owner):
    """With NR_DEVICE and no stats the fused call returns without a stream sync: on a caller's stream that is
    still busy with tens of milliseconds of earlier work, the call comes back with the stream not yet idle
    (a call that synchronised would leave it idle), and its results are there after the sync.  (The scratch
    was sized by an earlier call of the same size: a first call allocates.)"""
    V, T = mesh("torus")
    ns = nv = 2048
    n = ns + nv
    dev = torch.device("cuda:0")
    x = torch.full((n, 3), 7.0, dtype=torch.float32, device=dev)
    y = torch.full((n,), 7.0, dtype=torch.float32, device=dev)
    a = torch.ones((4096, 4096), dtype=torch.float32, device=dev)
    a @ a  # (the first product loads its kernel)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    with nr.TriMesh(owner, V, T) as m:
        m.fit_samples_device(x.data_ptr(), y.data_ptr(), ns, nv, seed=1, sigma=0.03, lo=LO, hi=HI)
        owner.synchronize()
        try:
            with torch.cuda.stream(stream):
                owner.set_stream(stream.cuda_stream)
                for _ in range(24):
                    b = a @ a
                m.fit_samples_device(x.data_ptr(), y.data_ptr(), ns, nv, seed=SEED, sigma=0.03, lo=LO, hi=HI)
                busy = not stream.query()
                owner.synchronize()
            stream.synchronize()
        finally:
            owner.set_stream(None, own=True)
    assert busy, "the stream was idle when the call returned: it waited"
    rx, ry = fit_reference("torus", "normal", ns, nv)
    same(x.cpu().numpy(), rx)
    same(y.cpu().numpy(), ry)
    del b


def test_invalid_arguments(owner):
    L = nr.lib()
    V, T = mesh("torus")
    ctx = owner._ctx
    buf = np.full((16, 3), 7.0, F)
    col = np.full(16, 7.0, F)
    perm = np.full(16, 7, np.int32)
    lo, hi = (ctypes.c_float * 3)(*LO), (ctypes.c_float * 3)(*HI)

    def opts(seed=1, ns=4, nv=4, sigma=0.0, lo=LO, hi=HI, sign=0, beta=0.0):
        return _lib.NRSampleOpts(seed, ns, nv, sigma, (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi), sign, beta)

    bad = [opts(ns=-1), opts(nv=-1), opts(ns=0, nv=0), opts(ns=(1 << 27), nv=1), opts(sigma=-0.5), opts(sigma=float("nan")),
           opts(sigma=float("inf")), opts(hi=(1.3, -1.3, 1.3)), opts(hi=(1.3, 0.0, 1.3), lo=(-1.3, 0.0, -1.3)),
           opts(lo=(float("nan"), -1, -1)), opts(hi=(float("inf"), 1, 1))]
    V2, T2 = mesh("degenerate_torus")
    with nr.TriMesh(owner, V, T) as mm, nr.TriMesh(owner, V2, T2[-3:]) as flat:  # flat: zero-area triangles only
        m = mm._m
        for o in bad:
            assert L.nr_mesh_sample(m, ctypes.byref(o), buf.ctypes.data, None, None, 0, None) == -1
            assert L.nr_mesh_fit_samples(m, ctypes.byref(o), buf.ctypes.data, col.ctypes.data, 0, None) == -1
        for o in (opts(sign=2), opts(sign=-1), opts(beta=-1.0), opts(beta=float("nan"))):
            assert L.nr_mesh_fit_samples(m, ctypes.byref(o), buf.ctypes.data, col.ctypes.data, 0, None) == -1
        good = opts()
        assert L.nr_mesh_sample(m, None, buf.ctypes.data, None, None, 0, None) == -1
        assert L.nr_mesh_sample(m, ctypes.byref(good), None, None, None, 0, None) == -1
        assert L.nr_mesh_fit_samples(m, ctypes.byref(good), None, col.ctypes.data, 0, None) == -1
        assert L.nr_mesh_fit_samples(m, ctypes.byref(good), buf.ctypes.data, None, 0, None) == -1
        # a mesh without area can be created and asked for box points, not for surface points
        assert L.nr_mesh_sample(flat._m, ctypes.byref(good), buf.ctypes.data, None, None, 0, None) == -5
        assert L.nr_mesh_fit_samples(flat._m, ctypes.byref(good), buf.ctypes.data, col.ctypes.data, 0, None) == -5
        assert (buf == 7.0).all() and (col == 7.0).all()
        assert L.nr_mesh_sample(flat._m, ctypes.byref(opts(ns=0)), buf.ctypes.data, None, None, 0, None) == 0
        assert not (buf[:4] == 7.0).any() and (buf[4:] == 7.0).all()
    buf[:] = 7.0

    def order(X=buf, n=16, mode=0, lo_=lo, hi_=hi, perm_=perm, srt=None, c=ctx):
        return L.nr_points_order(c, None if X is None else X.ctypes.data, n, mode, lo_, hi_, 0, None if perm_ is None else perm_.ctypes.data,
                                 None if srt is None else srt.ctypes.data, 0, None)

    flipped = (ctypes.c_float * 3)(1.3, -1.3, 1.3)
    for rc in (order(n=0), order(n=-1), order(n=(1 << 27) + 1), order(mode=2), order(mode=-1), order(X=None), order(perm_=None),
               order(lo_=None), order(hi_=None), order(hi_=flipped), order(hi_=lo), order(X=None, mode=1, srt=buf)):
        assert rc == -1
    assert (perm == 7).all() and (buf == 7.0).all()
    assert order(X=None, mode=1, lo_=None, hi_=None) == 0 and sorted(perm.tolist()) == list(range(16))
