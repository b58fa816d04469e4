"""The composed-scene lattice calls without a GPU: tests/compose_mesh_ref.py (existing references
composed: compose_ref.field on mesh_ref.lattice, mesh_ref.mesh, sparse_mesh_ref.mesh) pinned on the
cases tests/test_gpu_compose_mesh.py compares the GPU against, so that comparison is not vacuous:
the S3 lattice gives a closed mesh every part owns vertices of, the bands chosen are sound (or, for
band 0, known not to be), and a lone identity part is the single-network lattice bit for bit."""
import numpy as np

import compose_mesh_ref as cmref
import compose_ref
import cudaneuralrender_amd as nr
import mesh_ref
import sparse_mesh_ref as sref
from compose_mesh_ref import RAGGED_DIMS, S3_DIMS, S3_ORIGIN, S3_STEP
from mesh_ref import bits

F = np.float32


def test_s3_lattice_values():
    value, owner, pairs = cmref.ref_grid("s3")
    assert value.shape == (49, 45, 83) and value.size == 183015
    assert pairs == 87021 and not np.isnan(value).any()
    assert set(owner.reshape(-1).tolist()) == {0, 1, 2}
    cnt = cmref.inbound_counts(cmref.S3, S3_ORIGIN, S3_STEP, S3_DIMS)
    assert int(cnt.sum()) == pairs and cnt.max() == 2 and (cnt == 0).sum() > value.size // 2  # mostly empty
    # the ragged lattice is a sub-lattice: the same points, the same values
    rv, ro, _ = cmref.ref_grid("s3", S3_ORIGIN, S3_STEP, RAGGED_DIMS)
    assert np.array_equal(bits(rv), bits(value[:47, :44, :82])) and np.array_equal(ro, owner[:47, :44, :82])


def test_s3_mesh_is_closed_and_every_part_owns_vertices():
    V, T, cells, keys, N, part = cmref.ref_dense("s3")
    assert (len(V), len(T)) == (5670, 11324)
    assert mesh_ref.is_closed_oriented(T)
    assert [int((part == j).sum()) for j in range(3)] == [1609, 3938, 123]  # the subtracted part owns some
    assert not np.isnan(N).any() and np.abs(np.linalg.norm(N.astype(np.float64), axis=1) - 1).max() < 1e-6
    # the ragged variant drops only empty cells
    rV, rT = cmref.ref_dense("s3", 0.0, S3_ORIGIN, S3_STEP, RAGGED_DIMS)[:2]
    assert (len(rV), len(rT)) == (5670, 11324) and mesh_ref.is_closed_oriented(rT)
    # another level: still a mesh, a different one
    V1, T1 = cmref.ref_dense("s3", 0.01)[:2]
    assert len(V1) > 5000 and mesh_ref.is_closed_oriented(T1) and (len(V1), len(T1)) != (len(V), len(T))


def test_s3_bands():
    value = cmref.ref_grid("s3")[0]
    dense = cmref.ref_dense("s3")
    # the smallest sound band, rounded up to four decimals (0.09532 and 0.11457)
    for B, up in ((4, 0.0954), (8, 0.1146)):
        b = sref.smallest_sound_band(value, B)
        assert up - 1e-4 < b <= up, (B, b)
    for B, nb, na in ((4, 2772, 1655), (8, 396, 293)):
        active = sref.active_bricks(value, B, 0.0, F(0.15))
        assert (active.size, int(active.sum())) == (nb, na)
        assert not (sref.crossing_bricks(value, B) & ~active).any()  # every crossing brick is among them
        V, T = cmref.ref_sparse("s3", B, 0.15)[:2]
        assert (len(V), len(T)) == (len(dense[0]), len(dense[1])) and mesh_ref.is_closed_oriented(T)
    # band 0: only the bricks with a corner sign change; crossing bricks are missed and the mesh is open
    active = sref.active_bricks(value, 4, 0.0, F(0.0))
    assert int(active.sum()) == 61 and int((sref.crossing_bricks(value, 4) & ~active).sum()) == 35
    V, T = cmref.ref_sparse("s3", 4, 0.0)[:2]
    assert 0 < len(T) < len(dense[1]) and not mesh_ref.is_closed_oriented(T)
    # the ragged lattice: last bricks of 1, 3 and 2 cells
    assert [(d - 1) % 4 for d in RAGGED_DIMS] == [1, 3, 2]
    rvalue = cmref.ref_grid("s3", S3_ORIGIN, S3_STEP, RAGGED_DIMS)[0]
    assert int(sref.active_bricks(rvalue, 4, 0.0, F(0.15)).sum()) == 1649
    rV, rT = cmref.ref_sparse("s3", 4, 0.15, RAGGED_DIMS)[:2]
    assert (len(rV), len(rT)) == (5670, 11324) and mesh_ref.is_closed_oriented(rT)


def test_four_network_lattice_reaches_every_part():
    value, owner, pairs = cmref.ref_grid("four", cmref.FOUR_ORIGIN, cmref.FOUR_STEP, cmref.FOUR_DIMS)
    assert value.size % 64 != 0 and not np.isnan(value).any()
    assert all((owner == j).sum() >= 50 for j in range(4))
    assert 300 <= pairs < value.size  # points inside a bound, and more outside every bound
    assert (value < 0).sum() >= 20


def test_lone_identity_part_is_the_single_network_lattice(nets):
    """One part {net 0, identity, pos 0, scale 1} on a lattice inside its bound: mesh_ref.sample of the
    network under scene tanh, bit for bit -- values, and so the mesh; the normals too, every
    tetrahedron sample being inside the bound."""
    o, s, d = cmref.LONE_ORIGIN, cmref.LONE_STEP, cmref.LONE_DIMS
    P = mesh_ref.lattice(o, s, d).astype(np.float64)
    assert ((np.abs(P) + 1e-4) ** 2).sum(1).max() <= 1.45
    net = cmref.onet("plane_1")
    value, owner, pairs = cmref.sample([net], [compose_ref.part(0)], o, s, d)
    want = mesh_ref.sample(net, o, s, d, scene=nr.NR_SCENE["tanh"])
    assert np.array_equal(bits(value), bits(want)) and not owner.any() and pairs == value.size
    V, T = mesh_ref.mesh(value, o, s)[:2]
    assert len(V) > 500 and len(T) > 500  # (open where the lattice's faces cut the model)
    got = cmref.normals([net], [compose_ref.part(0)], V)
    assert np.array_equal(bits(got), bits(mesh_ref.normals(net, V, scene=nr.NR_SCENE["tanh"])))
