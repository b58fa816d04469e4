"""The designed networks and lattices of tests/designed_nets.py, pinned on the CPU so that a GPU pass
of tests/test_gpu_scene_points.py means something: the networks compute what they are designed to
(in the oracle, bit for bit), every lattice meets the condition it was built for (by the f32
restatements of designed_nets), the oracle's reference forms and its C copies of the kernel forms
agree on every point set, and the oracle's scenes agree with a plain float64 restatement.

The plain restatement (designed_nets.plain_scene) against oracle.scene_sdf over the finite points of
every point set, each under all six scenes; deviation = |oracle - plain| / max(1, |oracle|), largest
measured (x86-64, glibc libm), and the bound asserted = 4 x that (the margin covers other libm builds):

    v1         1.001e-07  ->  4.004e-07
    tanh       2.979e-08  ->  1.192e-07
    subtract   7.884e-08  ->  3.154e-07
    cylinders  3.374e-07  ->  1.350e-06
    displace   8.645e-08  ->  3.458e-07
    round      6.505e-08  ->  2.602e-07

Every bound is below 1e-5: a wrong radius, offset or k is three orders of magnitude above it.  (A
point counts as finite when its oracle value is finite and |p| < 2^18: beyond that nr_sin's two-part
reduction is no longer a sine, by design on both sides.)
"""
import functools

import numpy as np
import pytest

import designed_nets as dn
import oracle
from designed_nets import F, WAVE

PLAIN_MEASURED = {"v1": 1.001e-07, "tanh": 2.979e-08, "subtract": 7.884e-08, "cylinders": 3.374e-07, "displace": 8.645e-08,
                  "round": 6.505e-08}
PLAIN_BOUND = {k: 4 * v for k, v in PLAIN_MEASURED.items()}
CASES = dn.cases()
BY_GROUP = {g: [c for c in CASES if c.group == g] for g in {c.group for c in CASES}}


def ids(group):
    return [c.id for c in BY_GROUP[group]]


def same_bits(a, b):
    """Equal bit for bit, or both NaN."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---- the instruments ----------------------------------------------------------

@pytest.mark.parametrize("nin", [3, 4])
@pytest.mark.parametrize("nh", [1, 2, 7])
def test_const_net_is_its_bias(nh, nin):
    X = np.random.default_rng(nh * 10 + nin).uniform(-2, 2, (500, nin)).astype(F)
    for c in (1.0, 0.3, 0.0, -0.05, -0.11, -5.0, 1e-30, -1e-30, 2.0 ** -127, np.inf, -np.inf):
        dims, K, B = dn.const_net(c, nh, nin)
        assert dims == [nin] + [32] * nh + [1]
        y = oracle.OracleNet(K, B).forward(X)[:, 0]
        assert (y.view(np.uint32) == F(c).view(np.uint32)).all(), c
    _, K, B = dn.const_net(np.nan, nh, nin)
    assert np.isnan(oracle.OracleNet(K, B).forward(X)).all()
    # -0: the chain's +0 plus the bias is +0
    _, K, B = dn.const_net(-0.0, nh, nin)
    assert (oracle.OracleNet(K, B).forward(X).view(np.uint32) == 0).all()


@pytest.mark.parametrize("a", [(16.0, 0.0, 0.0), (1.0, 0.0, 0.0), (2.0 ** -20, 0.0, 0.0), (0.0, 0.0, 1.0),
                               (0.0, 0.3, 0.0), (0.0, 0.0, 0.0, 1.0 / 360.0)])
@pytest.mark.parametrize("nh", [1, 2, 7])
def test_linear_net_is_one_product(a, nh):
    """One nonzero weight: the chain is the f32 product (the f64 product of two floats is exact, so
    rounding it once is fl(a p))."""
    nin = len(a)
    X = np.random.default_rng(3).uniform(-3, 3, (2000, nin)).astype(F)
    if nin == 4:
        X[:, 3] = np.arange(2000) % 360
    k = int(np.flatnonzero(a)[0])
    want = (np.float64(F(a[k])) * X[:, k].astype(np.float64)).astype(F)
    _, K, B = dn.linear_net(a, 0.0, nh, nin)
    assert same_bits(oracle.OracleNet(K, B).forward(X)[:, 0], want)
    _, K, B = dn.linear_net(a, 0.25, nh, nin)
    assert same_bits(oracle.OracleNet(K, B).forward(X)[:, 0], (want + F(0.25)).astype(F))


def test_linear_net_is_the_chain():
    """Three weights on inputs that are multiples of 2^-12: every product and partial sum is exact in
    f32, so the chain is the exact dot product."""
    a = (0.5, -2.0, 0.25)
    X = (np.random.default_rng(4).integers(-4096, 4097, (2000, 3)) / 4096.0).astype(F)
    want = (X.astype(np.float64) @ np.asarray(a)).astype(F)
    assert ((want.astype(np.float64)) == X.astype(np.float64) @ np.asarray(a)).all()
    _, K, B = dn.linear_net(a)
    assert same_bits(oracle.OracleNet(K, B).forward(X)[:, 0], want)


def test_coded_matcap():
    m = dn.coded_matcap(5, 9)
    assert m.shape == (5, 9) and m.dtype == np.uint32 and m[0, 0] == 0xff000000 and m[4, 8] == 0xff004008
    r, c = dn.decode_matcap(m)
    assert (r == np.arange(5)[:, None]).all() and (c == np.arange(9)[None, :]).all()


# ---- the lattices meet their conditions ---------------------------------------

def test_zoff_of_frame_180_is_zero():
    assert dn.sphere_zoff(180) == 0.0 and dn.sphere_zoff(0) == -0.7


@pytest.mark.parametrize("cid", ids("screen"))
def test_screen_lines_straddle(cid):
    case = next(c for c in CASES if c.id == cid)
    assert case.dims[0] * case.dims[1] * case.dims[2] == 3 * WAVE
    P = case.points()
    assert dn.q_in_domain(P, case.frame).all()  # the screened branch, not the sqrtf chain
    near, mid, far = dn.far_counts(dn.screen_far(P, case.info["c"], case.frame)[:, case.info["sphere"]])
    assert near == 0 and far == WAVE and 8 <= mid <= 56, (near, mid, far)
    assert (dn.reference(cid)[0] == F(case.info["c"])).all()


@pytest.mark.parametrize("cid", ids("inside"))
def test_inside_lattice(cid):
    case = next(c for c in CASES if c.id == cid)
    c, P = case.info["c"], case.points()
    T = float(dn.screen_T(F(c)))
    assert (T <= 0) if c <= -0.2 else (0 < T < 1e-5)  # -0.11f + 0.11f = 0: only the margin is left
    far = dn.screen_far(P, c, case.frame)
    assert dn.q_in_domain(P, case.frame).all()
    if c <= -0.2:
        assert far.all()  # every sphere is screened in every wave
    else:  # T = 4.7e-6: only the lattice point at the centre sphere's centre is nearer than that
        assert (~far).sum() == 1 and not far[:, 4].all()
    inside = np.sqrt(dn.sphere_q(P, case.frame)) < F(dn.SPHERE_R)
    assert inside.any(0).all()  # some point inside every sphere


def test_scattered_lattice():
    case = BY_GROUP["scattered"][0]
    P = case.points()
    assert len(P) == WAVE and dn.q_in_domain(P, case.frame).all()
    far = dn.screen_far(P, 0.3, case.frame)
    assert ((~far).sum(0) >= 1).all() and (far.sum(0) >= 1).all()  # every sphere: near for some lane, far for another
    assert len(set(dn.sphere_q(P, case.frame).argmin(1).tolist())) >= 6
    nsdf = dn.reference(BY_GROUP["scattered"][1].id)[0]
    assert same_bits(nsdf, (P[:, 2] + F(0.05)).astype(F))


def test_overflow_lattices():
    by = {c.info["kind"]: c for c in BY_GROUP["overflow"] if c.scene == "v1"}
    q = dn.sphere_q(by["inf"].points(), 180)
    assert q.shape == (WAVE, 9)
    assert np.isinf(q[32:]).all() and np.isfinite(q[:32]).all()  # one chunk: 32 finite lanes share it
    dom = dn.q_in_domain(by["inf"].points(), 180)
    assert dom[:32].all() and not dom[32:].any()
    q = dn.sphere_q(by["max"].points(), 180)
    assert np.isfinite(q).all() and (q[32:] > 0.29 * np.finfo(F).max).all() and dn.q_in_domain(by["max"].points(), 180).all()
    assert np.isnan(dn.sphere_q(by["nan"].points(), 180)).all()
    # "inf": the finite row is near every sphere, so no sphere is screened whatever the ballot says
    assert not dn.screen_far(by["inf"].points(), 0.3, 180).all(0).any()
    # "far", "far-neg": q = inf in the second row and every lane passes the screen for all nine spheres -- without
    # the domain ballot the wave would add +0 where the reference's union with an infinite distance is NaN
    for kind in ("far", "far-neg"):
        P, c = by[kind].points(), by[kind].info["c"]
        q = dn.sphere_q(P, 180)
        assert np.isinf(q[32:]).all() and np.isfinite(q[:32]).all()
        assert dn.screen_far(P, c, 180).all()
        nsdf, ref = dn.reference(by[kind].id)
        ref = ref.reshape(-1)
        assert (ref[:32] == F(c)).all() and np.isnan(ref[32:]).all() and (nsdf == F(c)).all()


def test_range_lines():
    ns = {c.info["a"]: np.abs(dn.reference(c.id)[0]) for c in BY_GROUP["ranges"] if c.scene == "tanh"}
    assert ns[16.0].max() > 19 and (ns[16.0] > 9.5).sum() > 100 and (ns[16.0] < 9.5).sum() > 100
    for a in (16.0, 1.0):  # both sides of expm1_pos's switch at 2 |x| = 0.5
        assert (ns[a] < 0.25).sum() > 10 and (ns[a] > 0.25).sum() > 10
    assert ns[2.0 ** -20].max() < 2e-6
    tiny = next(c for c in BY_GROUP["ranges"] if c.id == "ranges-tiny-a1")
    n = dn.reference(tiny.id)[0]
    assert n[0] == 0 and 0 < n[1] < 1e-30 and (np.diff(n) > 0).all()
    large = next(c for c in BY_GROUP["ranges"] if c.id == "ranges-large-displace")
    P = large.points()
    assert np.abs(P).max() > 2990 and np.abs(P).max() < 3100
    assert ((F(5) * P).astype(np.float64) == 5.0 * P.astype(np.float64)).all()
    q, kd = dn.sin_quadrants(P)
    assert set(q.reshape(-1).tolist()) == {0, 1, 2, 3} and np.abs(kd).max() > 9000
    for axis in range(3):
        assert len(set(q[:, axis].tolist())) >= 3, axis


@pytest.mark.parametrize("cid", ids("subtract") + ids("cylinders"))
def test_subtraction_lines_straddle(cid):
    case = next(c for c in CASES if c.id == cid)
    c, sign, target = case.info["c"], case.info["sign"], case.info["target"]
    t = dn.sub_chain_t(case.points(), c, case.scene, case.frame)
    k = F(dn.SMOOTH_K)
    radius = dn.SPHERE_R if case.scene == "subtract" else dn.CYL_R
    if radius - c + sign * dn.SMOOTH_K <= 0:
        # d1 + d2 >= c - radius > k everywhere: the division is skipped in every lane of every obstacle
        assert (t >= k).all()
        return
    beyond = (t[:, target] >= k) if sign > 0 else (t[:, target] > -k)
    lo, mid, hi = dn.far_counts(beyond)
    assert lo == 0 and hi == WAVE and 8 <= mid <= 56, (lo, mid, hi)
    assert (np.abs(t[:, target]) < k).sum() >= 8  # and lanes whose division is taken


# ---- reference form == kernel form on every point set -------------------------

@pytest.mark.parametrize("cid", dn.case_ids())
def test_kernel_forms_agree(cid):
    case = next(c for c in CASES if c.id == cid)
    P, nsdf = case.points(), dn.reference(cid)[0]
    with np.errstate(all="ignore"):
        d = (np.sqrt(dn.sphere_q(P, case.frame)) - F(dn.SPHERE_R)).astype(F)
    assert same_bits(*oracle.many_sphere_pair(P, nsdf, case.frame))
    assert same_bits(*oracle.cylinders_pair(P, nsdf))
    for i in range(9):
        assert same_bits(*oracle.smooth_union_pair(nsdf, d[:, i])), i
        assert same_bits(*oracle.smooth_sub_pair(nsdf, d[:, i])), i


# ---- the oracle's scenes against the plain float64 restatement ----------------

@functools.lru_cache(maxsize=None)
def point_sets():
    """The distinct (points, nsdf, frame) of the cases."""
    seen = {}
    for c in CASES:
        key = (c.net, c.origin, c.step, c.dims, c.frame)
        if repr(key) not in seen:
            seen[repr(key)] = (c.points(), dn.reference(c.id)[0], c.frame)
    return list(seen.values())


def plain_deviation(scene):
    worst, n = 0.0, 0
    for P, nsdf, frame in point_sets():
        with np.errstate(all="ignore"):
            ref = np.array([oracle.scene_sdf(p, s, dn.SCENE_ID[scene], frame) for p, s in zip(P, nsdf)], np.float64)
            ok = np.isfinite(ref) & np.isfinite(nsdf) & (np.abs(P) < 2.0 ** 18).all(1)
            if not ok.any():
                continue
            plain = dn.plain_scene(P[ok], nsdf[ok], scene, frame)
        dev = np.abs(ref[ok] - plain) / np.maximum(1.0, np.abs(ref[ok]))
        worst, n = max(worst, float(dev.max())), n + int(ok.sum())
    return worst, n


@pytest.mark.parametrize("scene", dn.SCENES)
def test_oracle_scenes_against_plain_float64(scene):
    worst, n = plain_deviation(scene)
    print(f"{scene}: largest deviation {worst:.3e} over {n} points")
    assert n > 20000
    assert PLAIN_BOUND[scene] < 1e-5
    assert worst <= PLAIN_BOUND[scene], (scene, worst)


# ---- the matcap view ----------------------------------------------------------

def test_every_group_has_a_device_path_case():
    assert {c.group for c in CASES} == {c.group for c in CASES if c.device}


def test_matcap_view_decides_nearly_every_texel():
    """The view of tests/test_gpu_matcap_shapes.py: for every shape the float64 prediction from the
    normals (query_ref) leaves at most 2 % of the coloured pixels undecided, names the texel the
    oracle's frame holds everywhere else, and reads more than one row / column of every axis longer than 2."""
    import cudaneuralrender_amd as nr
    import query_ref
    W, H, steps, cam = dn.MATCAP_VIEW
    _, K, B = nr.read_keras_h5(nr.geometry_path("plane_1"))
    net = oracle.OracleNet(K, B)
    iv, nm = nr.camera(*cam)
    O, D = query_ref.pixel_rays(W, H, iv)
    out, _ = query_ref.trace(net, O, D, steps, scene=dn.SCENE_ID["tanh"], frame=0)
    hit = out["status"] == query_ref.HIT
    assert hit.sum() > 1000 and not np.isnan(out["normal"][hit]).any()
    for shape in dn.MATCAP_SHAPES:
        row, col, sure = dn.predict_texels(out["normal"][hit], nm, shape)
        assert (~sure).sum() <= dn.NEAR_CAP * hit.sum(), shape
        img, _ = net.render(W, H, iv, nm, color_type=1, scene=dn.SCENE_ID["tanh"], matcap=dn.coded_matcap(*shape),
                            max_steps=steps)
        assert np.array_equal(img.reshape(-1) != 0, hit)
        grow, gcol = dn.decode_matcap(img.reshape(-1)[hit])
        assert np.array_equal(grow[sure], row[sure]) and np.array_equal(gcol[sure], col[sure]), shape
        # (an axis of size 2 reads texel 1 only where the coordinate is exactly 1)
        assert (len(set(grow.tolist())) > 1) == (shape[0] > 2) and (len(set(gcol.tolist())) > 1) == (shape[1] > 2), shape
