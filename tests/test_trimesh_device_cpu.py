"""A device-built triangle mesh without a GPU: the two new symbols' argument checks, and
tests/trimesh_device_ref.py (the numpy restatement of the contract of a device-built mesh in
include/neural_render.h) against the host build -- the tree's shape, the boxes, the table, closed
and the dead set, the distance's bits, the signs and the winding number."""
import ctypes

import numpy as np
import pytest

import cudaneuralrender_amd as nr
import trimesh_device_ref as DR
import trimesh_ref as R
import winding_ref as WR

F = np.float32
D = np.float64
NR_E_INVALID = -1
SHAPES = [(name, leaf) for name in ("tetrahedron", "cube", "torus", "degenerate_torus") for leaf in (1, 2, 8)]


def test_symbols_and_null_arguments():
    L = nr.lib()
    assert hasattr(L, "nr_mesh_create_device") and hasattr(L, "nr_mesh_download")
    V, T = DR.mesh("tetrahedron")
    out = ctypes.c_void_p(0x1234)
    vp, tp = ctypes.c_void_p(V.ctypes.data), ctypes.c_void_p(T.ctypes.data)
    # no owner: nothing is touched, least of all a device
    assert L.nr_mesh_create_device(None, vp, 4, tp, 4, 0, ctypes.byref(out), None) == NR_E_INVALID
    assert out.value is None, "*out is cleared on failure"
    assert L.nr_mesh_download(None, None, None, None, None, None, None, None) == NR_E_INVALID
    ctx = ctypes.c_void_p()
    if L.nr_create(0, ctypes.byref(ctx)) != 0:
        return  # (no device to own a context: the NULL-owner checks above are all there is)
    try:
        for args in ((None, 4, tp, 4, 0, ctypes.byref(out)), (vp, 4, None, 4, 0, ctypes.byref(out)), (vp, 4, tp, 4, 0, None),
                     (vp, 0, tp, 4, 0, ctypes.byref(out)), (vp, 4, tp, 0, 0, ctypes.byref(out)),
                     (vp, 4, tp, (1 << 24) + 1, 0, ctypes.byref(out)), (vp, 4, tp, 4, 33, ctypes.byref(out)),
                     (vp, 4, tp, 4, -1, ctypes.byref(out))):
            assert L.nr_mesh_create_device(ctx, *args, None) == NR_E_INVALID, args[1:5]
    finally:
        L.nr_destroy(ctx)


@pytest.mark.parametrize("name,leaf", SHAPES)
def test_tree_shape_is_the_hosts(name, leaf):
    V, T = DR.mesh(name)
    ref = DR.reference(name, leaf)
    nodes, order, moments, depth = nr.trimesh_hierarchy(V, T, leaf=leaf)
    assert ref["ntl"] == len(order) and ref["depth"] == depth
    assert sorted(ref["order"].tolist()) == sorted(order.tolist()), "the live triangles"
    w, wh = ref["nodes"].view(np.int32), nodes.view(np.int32)
    assert np.array_equal(w[:, 3], wh[:, 3]) and np.array_equal(w[:, 7], wh[:, 7])
    assert depth <= int(np.ceil(np.log2(max(len(order), 1)))) + 1


@pytest.mark.parametrize("name,leaf", SHAPES + [("flat_cube", 2), ("fine_torus", 8), ("one_triangle", 8)])
def test_boxes_hold_their_triangles_grown_by_slack(name, leaf):
    V, T = DR.mesh(name)
    ref = DR.reference(name, leaf)
    first, count = WR.ranges(ref["nodes"])
    P = V[T[ref["order"]]].astype(D)
    for i in range(len(first)):
        pts = P[first[i]:first[i] + count[i]].reshape(-1, 3)
        assert (ref["nodes"][i, 0:3].astype(D) <= pts.min(0) - ref["slack"]).all(), i
        assert (ref["nodes"][i, 4:7].astype(D) >= pts.max(0) + ref["slack"]).all(), i
    # ... and no more than one f32 step beyond that
    lo = (P.reshape(-1, 3).min(0) - ref["slack"]).astype(F)
    assert (ref["nodes"][0, 0:3] >= np.nextafter(lo, F(-np.inf))).all()


def weights(V, T, table_host):
    """per entry of the table the sum of the weights of its terms: 1, the edge's uses, the vertex's angles"""
    V64 = V.astype(D)
    nt = len(T)
    live = table_host[:, 0].any(1)
    w = np.ones((nt, 7))
    uses = {}
    for t in range(nt):
        for s in range(3):
            i, j = int(T[t, s]), int(T[t, (s + 1) % 3])
            uses[(min(i, j), max(i, j))] = uses.get((min(i, j), max(i, j)), 0) + 1
    ang = {}
    for t in range(nt):
        for s in range(3):
            w[t, 1 + s] = uses[(min(int(T[t, s]), int(T[t, (s + 1) % 3])), max(int(T[t, s]), int(T[t, (s + 1) % 3])))]
            if live[t]:
                o = V64[T[t, s]]
                u, v = V64[T[t, (s + 1) % 3]] - o, V64[T[t, (s + 2) % 3]] - o
                ang[int(T[t, s])] = ang.get(int(T[t, s]), 0.0) + np.arctan2(np.linalg.norm(np.cross(u, v)), u @ v)
    for t in range(nt):
        for s in range(3):
            w[t, 4 + s] = ang.get(int(T[t, s]), 0.0)
    return w


@pytest.mark.parametrize("name", list(DR.MESHES))
def test_table_closed_and_dead_set_against_the_host(name):
    """2^-21 per unit of weight: len's two f32 roundings (<= 1.2e-7 relative), h's 1e-11 and the final f32
    rounding (6e-8), with a margin of about two."""
    V, T = DR.mesh(name)
    ref = DR.reference(name)
    table, closed = nr.trimesh_normals(V, T)
    assert ref["closed"] == closed
    assert np.array_equal(ref["table"][:, 0].any(1), table[:, 0].any(1)), "the dead set"
    err = np.abs(ref["table"].astype(D) - table.astype(D)).max(2)
    bound = 2.0 ** -21 * weights(V, T, table)
    print(f"{name}: largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("name", ["torus", "cube"])
def test_distance_and_signs_with_either_table(name):
    """Measured: no sign differs at any of the 1,063 points of either mesh, so equality is asked of all."""
    V, T = R.mesh(name)
    X = R.points(name, surface=False)
    ref = DR.reference(name)
    host = R.distance(V, T, X)
    dev = R.distance(V, T, X, table=ref["table"])
    for k in ("closest", "tri", "feature"):
        assert np.array_equal(R.bits(host[k]), R.bits(dev[k])), k
    assert np.array_equal(R.bits(np.abs(host["sdf"])), R.bits(np.abs(dev["sdf"])))
    differ = np.signbit(host["sdf"]) != np.signbit(dev["sdf"])
    print(f"{name}: {int(differ.sum())} of {len(X)} signs differ")
    assert not differ.any()


@pytest.mark.parametrize("name", ["torus", "open_torus", "cube", "open_cube"])
def test_winding_through_the_device_tree(name):
    """test_winding_cpu.py's bound for the host tree at beta = 2: 0.05 of the exact sum."""
    V, T = WR.mesh(name)
    ref = DR.build(V, T) if name == "open_cube" else DR.reference(name)
    w = WR.winding(V, T, WR.points(name), 2.0, ref["nodes"], ref["order"], ref["moments"])
    err = float(np.abs(w - WR.exact_reference(name)).max())
    print(f"{name}: max |w - w_exact| at beta 2 through the Morton tree: {err:.3g}")
    assert err <= 0.05


def test_moments_are_the_restated_sums_to_rounding():
    """The pairwise raw sums against winding_ref.moments' sequential ones on the same tree: f64 rounding only."""
    V, T = DR.mesh("torus")
    ref = DR.reference("torus")
    m, r2 = WR.moments(V, T, ref["nodes"], ref["order"])
    assert np.allclose(ref["moments"][:, 0:3], m[:, 0:3], rtol=0, atol=1e-6)
    assert np.allclose(ref["moments"][:, 4:14], m[:, 4:14], rtol=0, atol=1e-6)
    assert (ref["moments"][:, 3] >= r2.astype(F) * F(1 - 1e-5)).all() and (ref["moments"][:, 3] <= r2.astype(F) * F(1 + 1e-5)).all()


def test_area_table_against_the_sequential_sum():
    """Blocks of 256 against sample_ref's one running sum over the same order: thresholds within a few units of 2^-32."""
    import sample_ref as SR
    V, T = DR.mesh("fine_torus")
    ref = DR.reference("fine_torus")
    assert ref["ntl"] > 2048
    thr, last = SR.area_table(V, T, ref["order"])
    assert last == ref["last"] == ref["ntl"] - 1 and ref["thresholds"][-1] == 0xffffffff
    assert np.abs(thr.astype(np.int64) - ref["thresholds"].astype(np.int64)).max() <= 16
    assert (np.diff(ref["thresholds"].astype(np.int64)) >= 0).all()
