"""CPU side of the brick-sparse extraction: tests/sparse_mesh_ref.py (the restatement the GPU tests
compare against) on the CPU oracle's lattices of plane_1.  With an infinite band it is the dense
reference; with the bands the GPU tests use no crossing cell lies outside an active brick -- a
condition asserted on the dense lattice, not a tolerance -- so the restricted meshes equal the dense
ones and are closed; with band = 0 the mesh is open at culled bricks.  The bundled geometry is thin:
no brick that holds a crossing cell shows a sign change among its corners on the tanh scene, so the
rule has to use the corner values as distances."""
import functools

import numpy as np
import pytest

import cudaneuralrender_amd as nr
import mesh_ref
import oracle
import sparse_mesh_ref as sref

F = np.float32
FRAME = 3
# the box of tests/test_gpu_mesh.py: with brick 4 it is 7 x 6 x 9 bricks, ragged in y (2 cells)
B_ORIGIN, B_STEP, B_DIMS = (-0.7, -0.8, -0.9), (0.05, 0.055, 0.05), (29, 23, 37)
# the same box at half the step
F_STEP, F_DIMS = (0.025, 0.0275, 0.025), (57, 45, 73)
# (scene, step, dims, brick, band) -> (bricks holding a crossing cell, active bricks, bricks): the
# reference's own counts
SOUND = {
    ("tanh", B_STEP, B_DIMS, 4, 0.18): (27, 170, 378),
    ("v1", B_STEP, B_DIMS, 4, 0.18): (82, 217, 378),
    ("displace", B_STEP, B_DIMS, 4, 0.18): (29, 171, 378),
    ("tanh", F_STEP, F_DIMS, 8, 0.18): (41, 170, 378),
    ("tanh", F_STEP, F_DIMS, 4, 0.09): (160, 545, 2772),
}


@functools.lru_cache(maxsize=None)
def net():
    _, K, B = nr.read_keras_h5(nr.geometry_path("plane_1"))
    return oracle.OracleNet(K, B)


@functools.lru_cache(maxsize=None)
def grid(scene, step=B_STEP, dims=B_DIMS):
    v = mesh_ref.sample(net(), B_ORIGIN, step, dims, scene=nr.NR_SCENE[scene], frame=FRAME)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def dense(scene, step=B_STEP, dims=B_DIMS):
    return mesh_ref.mesh(grid(scene, step, dims), B_ORIGIN, step, 0.0)


def test_brick_geometry():
    assert sref.brick_counts(B_DIMS, 4) == (7, 6, 9) and sref.brick_counts(B_DIMS, 16) == (2, 2, 3)
    assert sref.brick_counts((3, 2, 2), 4) == (1, 1, 1) and sref.brick_counts((18, 17, 2), 16) == (2, 1, 1)
    c = sref.corner_values(grid("tanh"), 4)
    assert c.shape == (10, 7, 8)
    # the last corner of the ragged axis is the lattice's last point
    assert c[9, 6, 7].tobytes() == grid("tanh")[36, 22, 28].tobytes() and c[1, 5, 2].tobytes() == grid("tanh")[4, 20, 8].tobytes()
    assert float(sref.default_band(B_STEP, 4)) == pytest.approx(0.3583, abs(1e-4))
    # every point of the box once per brick that holds it: 5 x 5 x 5 but 5 x 3 x 5 in the last y row
    assert sref.point_set_total(np.ones((9, 6, 7), bool), B_DIMS, 4) == 7 * 9 * (5 * 125 + 75)


@pytest.mark.parametrize("scene", ["tanh", "v1", "displace"])
def test_infinite_band_is_the_dense_reference(scene):
    d = dense(scene)
    for B in (4, 16):
        V, T, cells, keys, active = sref.mesh(grid(scene), B_ORIGIN, B_STEP, B, 0.0, np.inf)
        assert active.all()
        assert mesh_ref.bits(V).tobytes() == mesh_ref.bits(d[0]).tobytes()
        assert np.array_equal(T, d[1]) and np.array_equal(cells, d[2]) and np.array_equal(keys, d[3])


@pytest.mark.parametrize("case", list(SOUND), ids=lambda c: f"{c[0]}-{c[2][0]}-b{c[3]}-{c[4]}")
def test_sound_bands_give_the_dense_mesh(case):
    scene, step, dims, B, band = case
    g, d = grid(scene, step, dims), dense(scene, step, dims)
    cross = sref.crossing_bricks(g, B)
    active = sref.active_bricks(g, B, 0.0, F(band))
    print(case, "crossing", int(cross.sum()), "active", int(active.sum()), "of", active.size)
    assert (int(cross.sum()), int(active.sum()), active.size) == SOUND[case]
    assert not (cross & ~active).any()  # zero crossing cells outside active bricks
    least = sref.smallest_sound_band(g, B)
    print("smallest sound band", least, "of the diagonal", least / float(sref.default_band(step, B)))
    assert 2 * least < band  # the margin of the band
    assert not active.all()  # and the band culls
    V, T, cells, keys = sref.restrict(d, active, dims, B)
    assert mesh_ref.bits(V).tobytes() == mesh_ref.bits(d[0]).tobytes()
    assert np.array_equal(T, d[1]) and np.array_equal(keys, d[3])
    assert mesh_ref.is_closed_oriented(T)


def test_thin_geometry_defeats_a_sign_rule():
    """No brick of the tanh box that holds a crossing cell has corners of both signs."""
    g = grid("tanh")
    cross = sref.crossing_bricks(g, 4)
    signs = sref.active_bricks(g, 4, 0.0, F(0.0))
    assert int(cross.sum()) == 27 and not (cross & signs).any()


def test_zero_band_is_open():
    """Scene v1, band = 0: only the bricks with a corner sign change are kept, and the mesh is open
    where a kept brick meets a culled one that the surface enters."""
    g, d = grid("v1"), dense("v1")
    active = sref.active_bricks(g, 4, 0.0, F(0.0))
    assert int(active.sum()) == 48
    V, T, cells, keys = sref.restrict(d, active, B_DIMS, 4)
    assert 0 < len(T) < len(d[1]) and 0 < len(V) < len(d[0])
    assert not mesh_ref.is_closed_oriented(T)
    # vertices on faces shared with inactive bricks: a brick that holds both ends of the edge is culled
    hold = sref.holding_bricks(keys, B_DIMS, 4)
    assert ((hold >= 0).sum(1) >= 1).all() and (hold >= 0).sum(1).max() > 1
    act = active.reshape(-1)
    shared = ((hold >= 0) & ~act[np.maximum(hold, 0)]).any(1)
    assert ((hold >= 0) & act[np.maximum(hold, 0)]).any(1).all()  # and an active one holds it
    print("vertices on faces shared with inactive bricks:", int(shared.sum()), "of", len(keys))
    assert shared.any()


def test_rule_by_hand():
    one = np.full((5, 5, 5), 1.0, F)  # one brick of 4 cells, every corner 1 away from iso = 0
    assert not sref.active_bricks(one, 4, 0.0, 0.0).any()  # equal signs, d > 0 everywhere, band 0
    assert not sref.active_bricks(one, 4, 0.0, 0.5).any() and sref.active_bricks(one, 4, 0.0, 1.0).all()
    inner = one.copy()
    inner[2, 2, 2] = -1.0  # the surface is inside the brick and no corner sees it
    assert not sref.active_bricks(inner, 4, 0.0, 0.5).any()
    nan = one.copy()
    nan[4, 0, 4] = np.nan  # a NaN corner
    assert sref.active_bricks(nan, 4, 0.0, 0.0).all()
    nan[4, 0, 4], nan[2, 0, 4] = 1.0, np.nan  # a NaN that is no corner is not seen
    assert not sref.active_bricks(nan, 4, 0.0, 0.0).any()
    eq = one.copy()
    eq[0, 4, 0] = 0.25  # a corner equal to iso is outside, like the others, and has d = 0
    assert sref.active_bricks(eq, 4, 0.25, 0.0).all()
    assert not (eq < F(0.25)).any()
    sign = one.copy()
    sign[0, 0, 0] = -3.0  # a corner sign change, far from iso
    assert sref.active_bricks(sign, 4, 0.0, 0.0).all()
    assert sref.active_bricks(one, 4, 0.0, np.inf).all() and sref.active_bricks(np.full((5, 5, 5), np.inf, F), 4, 0.0, np.inf).all()


def test_library_exports_the_entry_point():
    assert "nr_extract_mesh_sparse" in nr._lib.EXPORTS
    assert hasattr(nr.lib(), "nr_extract_mesh_sparse")
