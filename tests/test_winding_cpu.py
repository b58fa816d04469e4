"""The winding-number query without a GPU: tests/winding_ref.py (the numpy restatement of the contract in
include/neural_render.h) against np.arctan2 and the exact float64 sum, and nr_mesh_hierarchy (the
tree and the far-field moments nr_trimesh_create uploads) against the restatement's sums."""
import ctypes

import numpy as np
import pytest

import cudaneuralrender_amd as nr
import trimesh_ref as R
import winding_ref as WR

F = np.float32
# (mesh, leaf): as the GPU tests; leaf 8 is the default
TREES = [("tetrahedron", 8), ("cube", 1), ("torus", 8), ("torus", 3), ("open_torus", 8), ("open_cube", 8),
         ("double_cube", 2)]


tree, walk = WR.tree, WR.reference


def test_meshes():
    assert len(WR.mesh("open_torus")[1]) == 1164 and len(R.torus()[1]) == 1640
    assert len(WR.mesh("open_cube")[1]) == 10 and len(WR.mesh("double_cube")[1]) == 24
    for name in ("open_torus", "open_cube"):
        assert not nr.trimesh_normals(*WR.mesh(name))[1], name
    # every edge of the doubled cube has its two triangles: `closed` does not see that it cuts through itself
    assert nr.trimesh_normals(*WR.mesh("double_cube"))[1]


def test_half_angle_against_arctan2():
    rng = np.random.default_rng(5)
    num, den = rng.normal(size=200000), rng.normal(size=200000)
    # every octant, both branches of the reduction, and magnitudes far apart
    num[:50000] *= 10.0 ** rng.uniform(-8, 8, 50000)
    err = np.abs(WR.half_angle(num, den) - np.arctan2(num, den)).max()
    print(f"max |h - arctan2| over {len(num)} pairs: {err:.3g}")
    assert err <= 1e-10


def test_half_angle_conventions():
    h = WR.half_angle
    inf, nan, pi = np.inf, np.nan, np.pi
    # num == 0 gives 0 whatever den is -- arctan2 would give pi for den < 0: a point in a triangle's
    # plane, or a triangle without area, contributes nothing
    assert [float(h(0.0, d)) for d in (1.0, -1.0, 0.0, -0.0, inf, -inf, nan)] == [0.0] * 7
    assert float(h(-0.0, -1.0)) == 0.0
    # den == 0: +-pi/2 exactly as the constant is written
    assert float(h(2.0, 0.0)) == 1.5707963267948966 and float(h(-2.0, 0.0)) == -1.5707963267948966
    assert float(h(2.0, -0.0)) == 1.5707963267948966
    # the four diagonals
    assert np.allclose([h(1.0, 1.0), h(1.0, -1.0), h(-1.0, -1.0), h(-1.0, 1.0)], [pi / 4, 3 * pi / 4, -3 * pi / 4, -pi / 4],
                       rtol=0, atol=1e-15)
    # one infinity: the quotient is 0; two: it is not finite, so 0; a NaN anywhere: 0
    assert float(h(inf, 1.0)) == 1.5707963267948966 and float(h(-inf, -1.0)) == -1.5707963267948966
    assert float(h(1.0, inf)) == 0.0 and float(h(1.0, -inf)) == 3.141592653589793
    assert [float(h(a, b)) for a, b in ((inf, inf), (-inf, inf), (inf, -inf), (nan, 1.0), (1.0, nan), (nan, nan))] == [0.0] * 6
    # the threshold between the two reductions is taken without reduction
    t = WR.TAN_PI_8
    assert abs(float(h(t, 1.0)) - np.arctan(t)) < 1e-11 and abs(float(h(np.nextafter(t, 1.0), 1.0)) - np.arctan(t)) < 1e-11


@pytest.mark.parametrize("name, leaf", TREES)
def test_hierarchy_is_a_preorder_tree(name, leaf):
    V, T = WR.mesh(name)
    nodes, order, moments, depth = tree(name, leaf)
    nn = len(nodes)
    assert nodes.shape == (nn, 8) and moments.shape == (nn, 16) and nodes.dtype == F and order.dtype == np.int32
    # every live triangle once (these meshes have no triangle without area)
    assert np.array_equal(np.sort(order), np.arange(len(T)))
    w3, w7 = WR.links(nodes)
    first, count = WR.ranges(nodes)
    seen, leaves, next_pos, deepest = 0, 0, 0, 0
    stack = [(0, nn, 1)]  # (node, the end of its subtree, level)
    while stack:
        i, end, level = stack.pop()
        assert i == seen, "the nodes are not in preorder"
        seen += 1
        deepest = max(deepest, level)
        if w7[i] <= 0:
            assert end == i + 1
            assert w3[i] == next_pos and 1 <= -w7[i] <= leaf, "leaves are not contiguous in preorder"
            next_pos += -w7[i]
            leaves += 1
        else:
            assert w3[i] == i + 1 and i + 1 < w7[i] < end
            assert count[i] > leaf and first[w7[i]] == first[i] + count[w3[i]]
            stack.append((int(w7[i]), end, level + 1))
            stack.append((int(w3[i]), int(w7[i]), level + 1))
        # the box holds the node's triangles
        P = V[T[order[first[i]:first[i] + count[i]]]].reshape(-1, 3)
        assert (P >= nodes[i, 0:3]).all() and (P <= nodes[i, 4:7]).all()
    assert seen == nn and next_pos == len(T) and deepest == depth and nn == 2 * leaves - 1
    assert depth <= int(np.ceil(np.log2(len(T)))) + 1


@pytest.mark.parametrize("name, leaf", TREES)
def test_moments_against_restatement(name, leaf):
    """The order of every sum is fixed (position order, sequential), so the library's records equal the
    restatement's bit for bit; R2 is rounded up."""
    V, T = WR.mesh(name)
    nodes, order, moments, _ = tree(name, leaf)
    ref, r2 = WR.moments(V, T, nodes, order)
    assert np.array_equal(R.bits(moments), R.bits(ref)), f"{int((R.bits(moments) != R.bits(ref)).sum())} words differ"
    assert (moments[:, 3].astype(np.float64) >= r2).all() and (moments[:, 3] > 0).all()
    assert (moments[:, 3] <= np.nextafter(r2.astype(F), F(np.inf))).all()
    assert not moments[:, [7, 14, 15]].any()
    # and they mean what they should: the root's N is the mesh's area vector (0 for a closed mesh)
    A = 0.5 * np.cross(V[T[:, 1]].astype(np.float64) - V[T[:, 0]], V[T[:, 2]].astype(np.float64) - V[T[:, 0]])
    assert np.allclose(moments[0, 4:7], A.sum(0), rtol=0, atol=1e-6)
    # the centre lies within the box, and every corner within R2 of it
    assert (moments[:, 0:3] >= nodes[:, 0:3]).all() and (moments[:, 0:3] <= nodes[:, 4:7]).all()


def test_hierarchy_leaves_out_degenerate_triangles():
    """three triangles without area appended: the same tree, records and order as the torus' own"""
    V2, T2 = R.degenerate_torus()
    a = nr.trimesh_hierarchy(V2, T2, leaf=3)
    b = tree("torus", 3)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(R.bits(x), R.bits(y))
    assert a[3] == b[3]
    nodes, order, moments, depth = nr.trimesh_hierarchy(V2, T2[-3:])
    assert (len(nodes), len(order), depth) == (1, 0, 1) and not moments.any()


def test_hierarchy_invalid_arguments():
    L = nr.lib()
    V, T = R.cube()
    outs = [ctypes.POINTER(ctypes.c_float)(), ctypes.c_long(0), ctypes.POINTER(ctypes.c_int)(), ctypes.c_long(0),
            ctypes.POINTER(ctypes.c_float)(), ctypes.c_int(0)]

    def call(V_, nv, T_, nt, leaf, drop=None):
        refs = [None if k == drop else ctypes.byref(o) for k, o in enumerate(outs)]
        return L.nr_mesh_hierarchy(None if V_ is None else V_.ctypes.data, nv, None if T_ is None else T_.ctypes.data, nt,
                                   leaf, *refs)

    high, nanv = T.copy(), V.copy()
    high[3, 1] = 8
    nanv[2, 2] = np.nan
    for rc in [call(None, 8, T, 12, 0), call(V, 8, None, 12, 0), call(V, 0, T, 12, 0), call(V, 8, T, 0, 0),
               call(V, 8, T, (1 << 24) + 1, 0), call(V, 8, high, 12, 0), call(nanv, 8, T, 12, 0), call(V, 8, T, 12, -1),
               call(V, 8, T, 12, 33)] + [call(V, 8, T, 12, 0, drop=k) for k in range(6)]:
        assert rc == -1
        assert not outs[0] and not outs[2] and not outs[4] and outs[1].value == 0
    assert call(V, 8, T, 12, 32) == 0 and outs[1].value == 1 and outs[3].value == 12 and outs[5].value == 1
    for k in (0, 2, 4):
        L.nr_free(ctypes.cast(outs[k], ctypes.c_void_p))


# ---- accuracy against the exact float64 sum --------------------------------------------------------

@pytest.mark.parametrize("name", ["torus", "open_torus", "cube", "open_cube"])
def test_accuracy_against_exact_sum(name):
    """Measured with these trees (leaf 8) and points, max |w - w_exact| at beta = 2 / 3 / 4 and BRUTE:
    torus 1.7e-2 / 4.0e-3 / 1.7e-3 / 6.1e-7, open_torus 1.7e-2 / 4.2e-3 / 1.5e-3 / 6.1e-7, cube 4.2e-7 and
    open_cube 4.0e-7 at all four (three nodes; the points are close to all of them).  0, 5, 0 and 22 of
    the 1,063 points lie within 0.05 of w = 0.5 and are left out of the sign comparison.  The bounds are
    loose against these figures on purpose: 0.05 is the margin of the sign test, 0.01 a fifth of it."""
    ex = WR.exact_reference(name)
    err = {b: float(np.abs(walk(name, 8, b) - ex).max()) for b in (2.0, 3.0, 4.0)}
    eb = float(np.abs(walk(name, 8, 2.0, True) - ex).max())
    clear = np.abs(ex - 0.5) > 0.05
    print(f"{name}: max |w - w_exact| beta 2 / 3 / 4: {err[2.0]:.3g} / {err[3.0]:.3g} / {err[4.0]:.3g}, BRUTE {eb:.3g}; "
          f"{int((~clear).sum())} of {len(ex)} points within 0.05 of 0.5")
    assert err[2.0] <= 0.05 and err[4.0] <= 0.01
    assert eb <= 1e-5
    assert (~clear).mean() <= 0.05
    for b in (2.0, 3.0, 4.0):
        assert np.array_equal(walk(name, 8, b)[clear] >= 0.5, ex[clear] >= 0.5), f"a sign flips at beta = {b}"


@pytest.mark.parametrize("name", WR.CLOSED)
def test_closed_meshes(name):
    """1 inside, 0 outside, and the inside test is the pseudonormal sign of the distance"""
    w = walk(name, 8, 2.0, True)
    assert np.minimum(np.abs(w), np.abs(w - 1)).max() <= 1e-5
    sdf = R.distance(*WR.mesh(name), WR.points(name))["sdf"]
    off = np.abs(sdf) > 1e-4
    assert off.sum() > 900 and (w >= 0.5).sum() > 20
    assert np.array_equal((w >= 0.5)[off], (sdf < 0)[off])


def test_double_cube():
    w = walk("double_cube", 2, 2.0, True)
    two = np.abs(w - 2) <= 1e-5
    assert two.sum() > 20
    X = WR.points("double_cube")
    V, _ = R.cube()
    lo, hi = V.min(0), V.max(0)
    sh = np.array([0.3, 0.2, 0.1], F)
    in1 = ((X > lo) & (X < hi)).all(1)
    in2 = ((X > lo + sh) & (X < hi + sh)).all(1)
    assert np.array_equal(two, in1 & in2)
    assert np.array_equal(w >= 0.5, in1 | in2)
    assert np.array_equal(walk("double_cube", 2, 2.0) >= 0.5, in1 | in2)


# ---- what the contract says about order --------------------------------------------------------------

@pytest.mark.parametrize("name, leaf", [("torus", 8), ("torus", 3), ("open_torus", 8), ("double_cube", 2), ("tetrahedron", 8)])
def test_no_node_far_equals_brute(name, leaf):
    a, b = walk(name, leaf, 1e15), walk(name, leaf, 2.0, True)
    assert np.array_equal(R.bits(a), R.bits(b))
    if name == "torus":
        assert not np.array_equal(R.bits(walk(name, leaf, 2.0)), R.bits(b))  # (and beta = 2 does take nodes)


def test_a_point_does_not_depend_on_the_others():
    nodes, order, moments, _ = tree("open_torus", 8)
    V, T = WR.mesh("open_torus")
    X = WR.points("open_torus")
    perm = np.random.default_rng(3).permutation(len(X))
    w = WR.winding(V, T, X[perm], 2.0, nodes, order, moments)
    assert np.array_equal(R.bits(w), R.bits(walk("open_torus", 8, 2.0)[perm]))
    one = WR.winding(V, T, X[17:18], 2.0, nodes, order, moments)
    assert R.bits(one)[0] == R.bits(walk("open_torus", 8, 2.0))[17]


def test_non_finite_points_and_default_beta():
    nodes, order, moments, _ = tree("torus", 8)
    V, T = WR.mesh("torus")
    X = np.array(WR.points("torus")[:70])
    X[3] = (np.nan, 0, 0)
    X[64] = (0, np.inf, 0)
    w, evals = WR.winding(V, T, X, 0.0, nodes, order, moments, count_evals=True)
    assert (R.bits(w[[3, 64]]) == 0x7fc00000).all()
    keep = np.ones(70, bool)
    keep[[3, 64]] = False
    assert np.array_equal(R.bits(w[keep]), R.bits(walk("torus", 8, 2.0)[:70][keep]))
    assert 0 < evals < 68 * len(T)
