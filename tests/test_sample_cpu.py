"""The fitting samples without a GPU: tests/sample_ref.py (the numpy restatement of the contract in
include/neural_render.h) against the Random123 known answers of Philox4x32-10, nr_mesh_area_table against
the restatement's table, and the distributions the contract promises -- area-weighted triangles, points in
their triangles, a unit-variance jitter, a uniform box, a shuffle that permutes -- on the restatement at a
fixed seed.  The GPU kernels are compared with the same restatement bit for bit (test_gpu_sample.py), so
what holds here holds for them."""
import ctypes
import functools

import numpy as np
import pytest

import cudaneuralrender_amd as nr
from cudaneuralrender_amd import _lib
import sample_ref as S
import trimesh_ref as R

F = np.float32
N = 200_000
SEED = 0x5eed5eed1234


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10"""
    kat = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for c, k, want in kat:
        assert " ".join(f"{w:08x}" for w in S.philox(c, k)) == want
    # the batched form, and the counter layout of a sample: (i low, i high, stream, 0) under (seed low, seed high)
    got = S.philox(np.array([k[0] for k in kat]), np.array([k[1] for k in kat]))
    assert [" ".join(f"{w:08x}" for w in row) for row in got] == [k[2] for k in kat]
    i = np.array([0x85a308d3243f6a88], np.uint64)
    assert np.array_equal(S.words(0x299f31d0a4093822, i, 0x13198a2e)[0], S.philox((0x243f6a88, 0x85a308d3, 0x13198a2e, 0), kat[2][1]))


MESHES = {"tetrahedron": R.tetrahedron, "cube": R.cube, "torus": R.torus, "degenerate_torus": R.degenerate_torus,
          "scaled_cube": S.scaled_cube}


@pytest.mark.parametrize("name", list(MESHES))
@pytest.mark.parametrize("leaf", [0, 1, 3])
def test_area_table(name, leaf):
    V, T = MESHES[name]()
    _, order, _, _ = nr.trimesh_hierarchy(V, T, leaf=leaf)
    thr, last = nr.mesh_area_table(V, T, leaf=leaf)
    want, want_last = S.area_table(V, T, order)
    assert thr.dtype == np.uint32 and np.array_equal(thr, want) and last == want_last
    assert len(thr) == len(order) and (np.diff(thr.astype(np.int64)) >= 0).all() and thr[-1] == 0xffffffff
    assert last == len(thr) - 1  # every live triangle of these meshes has a share
    if name == "degenerate_torus":
        # the three zero-area triangles are not in the table at all
        assert len(thr) == len(T) - 3 and not set(range(len(T) - 3, len(T))) & set(order.tolist())
        assert np.array_equal(thr, nr.mesh_area_table(*R.torus(), leaf=leaf)[0])
    # the shares are the areas
    V64 = V.astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(V64[T[order, 1]] - V64[T[order, 0]], V64[T[order, 2]] - V64[T[order, 0]]), axis=1)
    share = np.diff(np.concatenate([[0], thr.astype(np.float64)])) / 2.0 ** 32
    assert np.abs(share - area / area.sum()).max() < 2.0 ** -31


def test_area_table_without_area_and_errors():
    V, T = R.degenerate_torus()
    thr, last = nr.mesh_area_table(V, T[-3:])
    assert len(thr) == 0 and last == -1
    L = nr.lib()
    V, T = R.cube()
    tp, ntl, last = ctypes.POINTER(ctypes.c_uint32)(), ctypes.c_long(0), ctypes.c_long(0)
    good = [V.ctypes.data, 8, T.ctypes.data, 12, 0, ctypes.byref(tp), ctypes.byref(ntl), ctypes.byref(last)]
    for k in (0, 2, 5, 6, 7):
        a = list(good)
        a[k] = None
        assert L.nr_mesh_area_table(*a) == -1
    for k, v in ((1, 0), (3, 0), (3, (1 << 24) + 1), (4, -1), (4, 33), (1, 7)):  # (1, 7): an index out of range
        a = list(good)
        a[k] = v
        assert L.nr_mesh_area_table(*a) == -1
    assert L.nr_mesh_area_table(*good) == 0 and ntl.value == 12 and last.value == 11
    L.nr_free(ctypes.cast(tp, ctypes.c_void_p))


@functools.lru_cache(maxsize=None)
def drawn(sigma):
    V, T = S.scaled_cube()
    _, order, _, _ = nr.trimesh_hierarchy(V, T)
    out = S.sample(V, T, order, SEED, N, 0, sigma)
    for a in out.values():
        a.setflags(write=False)
    return out


def test_triangles_are_picked_by_area():
    V, T = S.scaled_cube()
    V64 = V.astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(V64[T[:, 1]] - V64[T[:, 0]], V64[T[:, 2]] - V64[T[:, 0]]), axis=1)
    assert np.isclose(area.max() / area.min(), 4.0)
    share = area / area.sum()
    counts = np.bincount(drawn(0.0)["tri"], minlength=len(T))
    sd = np.sqrt(N * share * (1 - share))
    print("counts", counts, "expected", N * share, "deviation in sd", (counts - N * share) / sd)
    assert counts.sum() == N and (np.abs(counts - N * share) <= 5 * sd).all()


def test_points_lie_in_their_triangles():
    V, T = S.scaled_cube()
    out = drawn(0.0)
    b = out["bary"].astype(np.float64)
    assert (out["bary"] >= 0).all() and np.abs(b.sum(1) - 1.0).max() <= 2.0 ** -23
    V64 = V.astype(np.float64)
    t = out["tri"]
    a, e1, e2 = V64[T[t, 0]], V64[T[t, 1]] - V64[T[t, 0]], V64[T[t, 2]] - V64[T[t, 0]]
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    off = np.abs(((out["points"].astype(np.float64) - a) * nrm).sum(1))
    print("largest distance from the plane", off.max())
    assert off.max() <= 1e-6
    # and at the barycentric combination of the corners
    comb = b[:, :1] * a + b[:, 1:2] * (a + e1) + b[:, 2:] * (a + e2)
    assert np.abs(comb - out["points"]).max() <= 1e-6
    # both halves of the parallelogram are used: the fold keeps the density uniform
    assert 0.3 < (b[:, 0] < 1 / 3).mean() < 0.6


def test_jitter_has_unit_variance():
    sigma = 0.03
    d = drawn(sigma)["points"].astype(np.float64) - drawn(0.0)["points"].astype(np.float64)
    assert np.array_equal(drawn(sigma)["tri"], drawn(0.0)["tri"]) and np.array_equal(drawn(sigma)["bary"], drawn(0.0)["bary"])
    print("jitter mean / sigma", d.mean(0) / sigma, "variance / sigma^2", d.var(0) / sigma ** 2, "largest |g|", np.abs(d).max() / sigma)
    assert (np.abs(d.mean(0)) < 5 * sigma / np.sqrt(N)).all()
    assert (np.abs(d.var(0) / sigma ** 2 - 1.0) < 0.02).all()
    assert np.abs(d).max() / sigma < 4.9 + 1e-3
    # the three axes draw from three streams
    c = np.corrcoef(d.T)
    assert np.abs(c[np.triu_indices(3, 1)]).max() < 5 / np.sqrt(N)
    # the deviate itself: an integer sum times one constant
    g = S.jitter(SEED, np.arange(1000, dtype=np.uint64), 2)
    assert np.array_equal(R.fmaf(F(sigma), g, drawn(0.0)["points"][:1000, 1]), drawn(sigma)["points"][:1000, 1])
    assert abs(float(S.JITTER_C) - np.sqrt(1.5) / 65536) < 1e-12


def test_volume_points_fill_the_box():
    V, T = S.scaled_cube()
    _, order, _, _ = nr.trimesh_hierarchy(V, T)
    lo, hi = np.array([-1.3, -0.5, 0.25], F), np.array([1.3, 2.0, 0.75], F)
    out = S.sample(V, T, order, SEED, 0, N, 0.03, lo, hi)
    P = out["points"]
    assert (out["tri"] == -1).all() and (out["bary"] == 0).all()
    assert (P >= lo).all() and (P <= hi).all()
    mid = (lo.astype(np.float64) + hi) / 2
    octant = ((P > mid) * np.array([1, 2, 4])).sum(1)
    counts = np.bincount(octant, minlength=8)
    sd = np.sqrt(N / 8 * 7 / 8)
    print("octants", counts, "deviation in sd", (counts - N / 8) / sd)
    assert (np.abs(counts - N / 8) <= 5 * sd).all()
    # mixed calls: the surface part and the volume part are those of their own indices
    mix = S.sample(V, T, order, SEED, 1000, 1000, 0.0, lo, hi)
    assert np.array_equal(mix["points"][:1000], drawn(0.0)["points"][:1000])
    assert np.array_equal(mix["points"][1000:], P[1000:2000])


def test_shuffle_is_a_seeded_permutation():
    n = 50_000
    p1, p2 = S.order(S.shuffle_keys(SEED, n)), S.order(S.shuffle_keys(SEED + 1, n))
    assert np.array_equal(np.sort(p1), np.arange(n)) and np.array_equal(np.sort(p2), np.arange(n))
    assert (p1 != p2).mean() > 0.99 and (p1 != np.arange(n)).mean() > 0.99
    assert np.array_equal(p1, S.order(S.shuffle_keys(SEED, n)))
    # no structure left: the correlation of position and index is noise
    assert abs(np.corrcoef(p1, np.arange(n))[0, 1]) < 5 / np.sqrt(n)


def test_morton_keys():
    """the key's corner cases: cells, the clamp, points outside the box, a NaN"""
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    X = np.array([[-1, -1, -1], [1, 1, 1], [5, -5, np.nan], [np.inf, -np.inf, 0], [-0.999, -1, -1], [-1, -0.999, -1],
                  [-1, -1, -0.999], [0.999, 1, 1]], F)
    k = S.morton_keys(X, lo, hi)
    assert k[0] == 0 and k[1] == (1 << 30) - 1
    assert k[2] == S.spread(np.int64(1023)) and k[3] == (S.spread(np.int64(1023)) | (S.spread(np.int64(511)) << 2))
    assert list(k[4:7]) == [0, 0, 0] and k[7] == (1 << 30) - 2  # 1022 along x
    X2 = np.array([[-0.99, -1, -1], [-1, -0.99, -1], [-1, -1, -0.99]], F)
    assert list(S.morton_keys(X2, lo, hi)) == [0b1000001, 0b1000001 << 1, 0b1000001 << 2]  # cell 5 = 0b101 along x, y, z
    # the same cells as tools/trimesh_bench.py's torch expression on points inside the box
    rng = np.random.default_rng(3)
    P = rng.uniform(-1, 1, (4096, 3)).astype(F)
    q = np.clip((P.astype(np.float64) + 1) / 2 * 1023, 0, 1023).astype(np.int64)
    mine = S.morton_keys(P, lo, hi)
    ref = (S.spread(q[:, 0]) | (S.spread(q[:, 1]) << 1) | (S.spread(q[:, 2]) << 2))
    assert (mine == ref).mean() > 0.99  # (they differ only where a rounding moves a point across a cell wall)


def test_exports_and_argument_errors():
    names = ["nr_mesh_area_table", "nr_mesh_sample", "nr_points_order", "nr_mesh_fit_samples"]
    L = nr.lib()
    for s in names:
        assert s in _lib.EXPORTS and hasattr(L, s) and "trimesh" not in s
    assert ctypes.sizeof(_lib.NRSampleOpts) == 64 and _lib.NRSampleOpts.lo.offset == 28 and _lib.NRSampleOpts.sign.offset == 52
    # what needs no device: a NULL mesh or context
    opts = _lib.NRSampleOpts(1, 4, 4, 0.0, (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(1, 1, 1), 0, 0.0)
    buf = np.zeros((8, 3), F)
    assert L.nr_mesh_sample(None, ctypes.byref(opts), buf.ctypes.data, None, None, 0, None) == -1
    assert L.nr_mesh_fit_samples(None, ctypes.byref(opts), buf.ctypes.data, buf.ctypes.data, 0, None) == -1
    perm = np.zeros(8, np.int32)
    lo, hi = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(1, 1, 1)
    assert L.nr_points_order(None, buf.ctypes.data, 8, 0, lo, hi, 0, perm.ctypes.data, None, 0, None) == -1
    assert b"NULL" in L.nr_last_error(None)
