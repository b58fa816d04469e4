"""Composed scenes without a GPU: tests/compose_ref.py (the numpy restatement of the nr_compose_*
contract) pinned to query_ref.trace for a lone identity part, the world bound of nr_compose_bound,
the host-side validation, and the fold's handling of -0 and NaN."""
import ctypes
import functools

import numpy as np
import pytest

import compose_ref
import cudaneuralrender_amd as nr
import oracle
import query_ref
import test_gpu_query
from compose_ref import SUBTRACT, UNION, part, rot_xyz
from query_ref import HIT

F = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def s3_parts():
    """Scene S3 of tests/test_gpu_compose.py: net 0 = plane_1, net 1 = car_1."""
    return [part(0, UNION, None, (-0.9, 0.0, 0.0), 1.0),
            part(1, UNION, rot_xyz(0.3, 1.0, -0.2), (1.0, 0.2, 0.1), 0.75),
            part(1, SUBTRACT, rot_xyz(1.2, 0.4, 0.5), (-0.9, 0.0, 0.0), 0.6)]


@functools.lru_cache(maxsize=None)
def unit_rays():
    o, d = test_gpu_query.rays()
    with np.errstate(all="ignore"):
        d = (d / np.sqrt(query_ref.dot3(d, d))[:, None]).astype(F)
    return o, d


def test_lone_identity_part_is_the_single_network_tracer(nets):
    """One part {net 0, identity, pos 0, scale 1} with the bound (0, 1.2f) against query_ref.trace
    under scene tanh: the same status on every ray, and every HIT ray equal bit for bit.  (ESCAPED
    step counts differ: the composed tracer's interval is tfar - tnear.)"""
    dims, K, B = nets["plane_1"]
    net = oracle.OracleNet(K, B)
    o, d = unit_rays()
    ref, rst = query_ref.trace(net, o, d, 300, scene=nr.NR_SCENE["tanh"])
    got, gst = compose_ref.trace([net], [part(0)], (0, 0, 0), F(1.2), o, d, 300)
    counts = [int(v) for v in np.bincount(ref["status"], minlength=4)]
    assert counts == [171, 579, 250, 0], counts
    assert np.array_equal(got["status"], ref["status"])
    hit = ref["status"] == HIT
    for k in ("steps", "t", "position", "normal"):
        assert np.array_equal(bits(got[k])[hit], bits(ref[k])[hit]), k
    # no ray is left out of the comparison above: whatever is not a HIT has the non-hit outputs
    for k in ("t", "position", "normal"):
        assert not bits(got[k])[~hit].any() and not bits(ref[k])[~hit].any(), k
    assert np.array_equal(got["part"], np.where(hit, 0, -1))
    assert gst["rays_hit"] == rst["rays_hit"] and gst["rays_shaded"] == rst["rays_shaded"] == 250
    # a lone part: at most one network evaluation per ray-step (a ray that starts inside the surface
    # steps backwards, and may leave the bound behind its entry point)
    assert 0.99 * gst["ray_steps"] <= gst["part_evals"] <= gst["ray_steps"]


BOUND_CASES = {
    "one": [part(0)],
    "s3": s3_parts(),
    "four": [part(i, UNION, rot_xyz(0.1 * i, 0.2, 0.3 * i), p, s)
             for i, (p, s) in enumerate([((-1.5, 0.9, 0), 0.8), ((1.4, 1.0, 0.2), 1.0), ((-1.3, -1.0, -0.3), 0.9), ((1.5, -0.9, 0.1), 1.1)])],
    "far": [part(0, UNION, None, (1000.25, -3.5, 7.0), 0.01), part(0, UNION, None, (-999.0, 2.0, 1.0), 37.5),
            part(0, SUBTRACT, None, (0.1, 0.2, 0.3), 1e-3)],
}


@pytest.mark.parametrize("name", list(BOUND_CASES))
def test_bound_encloses_every_part(name):
    parts = BOUND_CASES[name]
    c, r = nr.compose_bound(parts, 4)
    assert c.dtype == np.float32 and r.dtype == np.float32
    pos = np.array([p["pos"] for p in parts], np.float64)
    assert np.array_equal(c, pos.mean(0).astype(F))
    reach = [np.sqrt(((pos[j] - c.astype(np.float64)) ** 2).sum()) + 1.2 * float(p["scale"]) for j, p in enumerate(parts)]
    # 1.2 * scale in double is within 2^-23 (relative) of the f32 product the rule uses, and the rule
    # scales the distance by 1 + 2^-20: the f32 radius, rounded up, is no smaller than either form
    rule = max(np.sqrt(((pos[j] - c.astype(np.float64)) ** 2).sum()) * (1 + 2.0 ** -20) + float(F(1.2) * F(p["scale"]))
               for j, p in enumerate(parts))
    assert float(r) >= rule and float(np.nextafter(r, F(0))) < rule
    for j, v in enumerate(reach):
        assert float(r) >= v * (1 - 2.0 ** -22), (j, float(r), v)
    if name == "one":
        assert bits(c).tolist() == [0, 0, 0] and bits(np.array([r]))[0] == bits(np.array([1.2], F))[0]


def test_validation_without_a_device():
    L = nr.lib()

    def rc(parts, nnets=2):
        arr = nr.make_parts(parts)
        return L.nr_compose_bound(arr, len(parts), nnets, None, None)

    ok = s3_parts()
    assert rc(ok) == 0
    assert rc(ok, 0) == -1 and rc(ok, 5) == -1           # nnets outside 1..4
    assert rc([part(0)] * 17) == -1 and rc([part(0)] * 16) == 0
    assert L.nr_compose_bound(nr.make_parts(ok), 0, 2, None, None) == -1   # nparts outside 1..16
    assert L.nr_compose_bound(None, 1, 1, None, None) == -1
    assert rc([part(2)]) == -1 and rc([part(-1)]) == -1  # net index out of range
    assert rc([part(0, SUBTRACT)]) == -1                  # part 0 must be a union
    assert rc([part(0), part(1, 2)]) == -1                # unknown op
    for s in (0.0, -1.0, np.inf, np.nan, 1e-39, 3e38):
        assert rc([part(0, scale=s)]) == -1, s
    assert rc([part(0, pos=(np.nan, 0, 0))]) == -1
    R = rot_xyz(0.3, 1.0, -0.2)
    assert rc([part(0, rot=R)]) == 0
    assert rc([part(0, rot=R * F(1.001))]) == -1          # |R R^T - I| > 1e-4
    assert rc([part(0, rot=R * F(1.00001))]) == 0
    assert rc([part(0, rot=np.diag([1, 1, -1]))]) == -1   # a reflection: det < 0
    assert rc([part(0, rot=np.zeros((3, 3)))]) == -1
    assert b"part 0" in L.nr_last_error(None)
    # NULL objects are errors, not crashes
    out = ctypes.c_void_p()
    assert L.nr_compose_create(None, None, 1, nr.make_parts(ok), 3, ctypes.byref(out)) == -1 and not out
    assert L.nr_compose_set_parts(None, nr.make_parts(ok), 3) == -1
    assert L.nr_compose_info(None, None, None, None, None) == -1
    assert L.nr_compose_sample(None, None, 0, None, None, 0, None) == -1
    assert L.nr_compose_trace_rays(None, None, None, 0, 10, None, None, None, None, None, None, 0, None) == -1
    assert L.nr_compose_gbuffer(None, 4, 4, 10, None, None, None, None, None, None, 0, None) == -1
    assert L.nr_compose_render(None, None, 4, 4, 10, None, 0, None) == -1
    assert L.nr_compose_destroy(None) == 0
    assert ctypes.sizeof(nr.NRPart) == 60 and ctypes.sizeof(nr.NRComposeStats) == 72


def test_fold_signed_zeros_and_nan():
    nan, inf = F(np.nan), F(np.inf)
    pz, nz = F(0.0), F(-0.0)

    def run(terms, ops):
        d, own = compose_ref.fold([np.array([t], F) for t in terms], ops)
        return bits(d)[0], int(own[0])

    def b(v):
        return bits(np.array([v], F))[0]

    # a NaN term is ignored, wherever it stands behind part 0
    assert run([1.0, nan, 0.5], [UNION, UNION, UNION]) == (b(0.5), 2)
    assert run([1.0, nan], [UNION, SUBTRACT]) == (b(1.0), 0)
    # a NaN d_0 stays: no comparison against it is true
    assert run([nan, -5.0, 5.0], [UNION, UNION, SUBTRACT])[1] == 0
    assert np.isnan(compose_ref.fold([np.array([nan], F), np.array([1.0], F)], [UNION, UNION])[0][0])
    # equal values keep the earlier owner, and -0 == +0: neither takes the other
    assert run([pz, nz], [UNION, UNION]) == (b(pz), 0)
    assert run([nz, pz], [UNION, UNION]) == (b(nz), 0)
    assert run([pz, pz], [UNION, SUBTRACT]) == (b(pz), 0)    # -(+0) = -0 is not > +0
    assert run([nz, nz], [UNION, SUBTRACT]) == (b(nz), 0)    # -(-0) = +0 is not > -0
    # subtraction negates: the sign of a taken zero is the negated term's
    assert run([-1.0, pz], [UNION, SUBTRACT]) == (b(nz), 1)
    assert run([-1.0, nz], [UNION, SUBTRACT]) == (b(pz), 1)
    assert run([2.0, -inf], [UNION, UNION]) == (b(-inf), 1)
    assert run([2.0, -inf], [UNION, SUBTRACT]) == (b(inf), 1)
    # owners in part order
    assert run([3.0, 2.0, -2.5, 1.0], [UNION, UNION, SUBTRACT, UNION]) == (b(1.0), 3)
    assert run([3.0, 2.0, -2.5, 4.0], [UNION, UNION, SUBTRACT, UNION]) == (b(2.5), 2)


def test_field_terms_and_thresholds(nets):
    """A point is evaluated by the network exactly where qq <= 1.45; outside, the term is
    scale * (sqrt(qq) - 1.19), which is positive and below the distance to the part's sphere of
    radius 1.2 scale -- a step on it cannot leave the ray short of the evaluated region."""
    dims, K, B = nets["plane_1"]
    net = oracle.OracleNet(K, B)
    rng = np.random.default_rng(3)
    P = rng.uniform(-1.0, 1.0, (400, 3)).astype(F)
    p = part(0, UNION, rot_xyz(0.4, -0.3, 1.1), (0.3, -0.2, 0.1), 0.5)
    d, own, pairs = compose_ref.field([net], [p], P)
    v = (P.astype(np.float64) - p["pos"].astype(np.float64))
    dist = np.sqrt((v ** 2).sum(1))
    inside = dist <= 0.5 * np.sqrt(1.45) * (1 - 1e-5)
    outside = dist >= 0.5 * np.sqrt(1.45) * (1 + 1e-5)
    assert 30 <= inside.sum() and 100 <= outside.sum()
    assert int(inside.sum()) <= pairs <= int((~outside).sum())
    # outside: the analytic term, in double within f32 rounding
    assert np.allclose(d[outside], dist[outside] - 0.5 * 1.19, rtol=0, atol=1e-5)
    assert (d[outside] > 0).all() and (d[outside] < dist[outside] - 0.5 * 1.2 + 0.5 * 0.0101).all()
    assert (np.abs(d[inside]) <= 0.5).all() and not own.any()
