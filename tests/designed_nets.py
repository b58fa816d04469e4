"""Designed networks and adversarial lattices: a helper, not a test.

A fused-shape network ([3|4, 32, ..., 32, 1]) loaded with nr_load_mlp can be made an instrument whose
output is an exactly known function of the point: all-zero weights give the last bias (const_net), a
ReLU pair gives the layer-0 chain fl(a.p) (linear_net).  nr_sample_grid then evaluates
sceneSDF(p, nsdf) on the device at points and surface values the test chooses, not at what a trained
network happens to produce: lines that cross a wave-wide threshold of nr_device.h inside one
64-point chunk, chunks in which one lane overflows, surface values that are NaN, infinite, tiny or
far outside [-1, 1].

Every lattice comes as (origin, step, dims, frame) -- the arguments of nr_sample_grid, whose kernel
deals the linear index in 64-point chunks, one per wave -- and with a numpy restatement in f32 steps
of the condition it is built for (sphere_q / screen_far, sub_chain_t): tests/test_designed_cpu.py
asserts the conditions, tests/test_gpu_scene_points.py runs the lattices on the device.
"""
import functools

import numpy as np

import mesh_ref
import oracle

F = np.float32
D = np.float64
SCENES = ("v1", "tanh", "subtract", "cylinders", "displace", "round")
SCENE_ID = {"v1": 0, "tanh": 1, "subtract": 2, "cylinders": 3, "displace": 4, "round": 5}
# the sphere grid of manySphere (volumeRender_kernel.cu:176-196): sphere i = 3 row + col
SPHERE_X = (-0.5, -0.1, 0.3)
SPHERE_Y = (0.2, -0.2, -0.6)
SPHERE_R, CYL_R, SMOOTH_K = 0.1, 0.02, 0.01
WAVE = 64


# ---- networks -----------------------------------------------------------------

def _zeros(nh, nin):
    dims = [nin] + [32] * nh + [1]
    K = [np.zeros((dims[i], dims[i + 1]), F) for i in range(nh + 1)]
    B = [np.zeros(dims[i + 1], F) for i in range(nh + 1)]
    return dims, K, B


def const_net(c, nh=2, nin=3):
    """(dims, kernels, biases) of the network whose output is c at every point: every kernel and bias
    is zero except the last bias."""
    dims, K, B = _zeros(nh, nin)
    B[-1][0] = F(c)
    return dims, K, B


def linear_net(a, c=0.0, nh=2, nin=3):
    """The network whose output is fl(fl(a.p) + c), a.p the layer-0 fmaf chain: h0 = relu(a.p),
    h1 = relu(-a.p), the identity on both through the hidden layers, last kernel +1 / -1."""
    dims, K, B = _zeros(nh, nin)
    a = np.asarray(a, F)
    assert a.shape == (nin,)
    K[0][:, 0] = a
    K[0][:, 1] = -a
    for j in range(1, nh):
        K[j][0, 0] = K[j][1, 1] = 1.0
    K[-1][0, 0], K[-1][1, 0] = 1.0, -1.0
    B[-1][0] = F(c)
    return dims, K, B


def coded_matcap(h, w):
    """texel[r, c] = 0xff000000 | r << 12 | c: a coloured pixel names the row and column it was read at."""
    r, c = np.mgrid[0:h, 0:w]
    return (np.uint32(0xff000000) | (r.astype(np.uint32) << 12) | c.astype(np.uint32)).astype(np.uint32)


def decode_matcap(px):
    px = np.asarray(px, np.uint32)
    return ((px >> 12) & 0xfff).astype(np.int64), (px & 0xfff).astype(np.int64)


# the matcap shapes of tests/test_gpu_matcap_shapes.py, its view of plane_1 (W, H, max_steps, camera) and the
# share of coloured pixels whose predicted texel may be left undecided
MATCAP_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (5, 512), (511, 64)]
MATCAP_VIEW = (96, 80, 64, (-35.0, 30.0, 1.3))
NEAR, NEAR_CAP = 1e-3, 0.02


def predict_texels(normals, nm, shape):
    """(row, col, sure) per normal: uv = trunc((normalize(nm[:3, :3] n) / 2 + 1 / 2) (size - 1)) per
    axis in float64, row from y and the height, column from x and the width; sure where both products
    are farther than NEAR from an integer (an axis of size 1 is always texel 0)."""
    n = np.asarray(normals, np.float64).reshape(-1, 3)
    M = np.asarray(nm, np.float64).reshape(4, 4)[:3, :3]
    e = n @ M.T
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    h, w = shape
    px, py = (e[:, 0] * 0.5 + 0.5) * (w - 1), (e[:, 1] * 0.5 + 0.5) * (h - 1)
    sure = np.ones(len(n), bool)
    for prod, size in ((px, w), (py, h)):
        if size > 1:
            sure &= np.abs(prod - np.rint(prod)) > NEAR
    return np.trunc(py).astype(np.int64), np.trunc(px).astype(np.int64), sure


# ---- the f32 restatements of the conditions -----------------------------------

def _f(x):
    return np.asarray(x, D).astype(F)


def sphere_zoff(frame):
    return -0.7 + (float(frame * 2) * 0.7 / 360.0)


def sphere_q(P, frame):
    """[n, 9] squared distances to the sphere centres as many_sphere forms them: f64 updates of f32
    coordinates, then f32 squares and sums (x first, then y, then z)."""
    P = np.asarray(P, F)
    with np.errstate(all="ignore"):
        x0 = _f(P[:, 0].astype(D) + 0.5)
        x1 = _f(x0.astype(D) - 0.4)
        x2 = _f(x1.astype(D) - 0.4)
        ys = _f(P[:, 1].astype(D) - 0.6)
        y0 = _f(ys.astype(D) + 0.4)
        y1 = _f(y0.astype(D) + 0.4)
        y2 = _f(y1.astype(D) + 0.4)
        zc = _f(P[:, 2].astype(D) + sphere_zoff(frame))
        xx = [x * x for x in (x0, x1, x2)]
        yy = [y * y for y in (y0, y1, y2)]
        zz = zc * zc
        return np.stack([(xx[i % 3] + yy[i // 3]) + zz for i in range(9)], -1).astype(F)


def screen_T(nsdf):
    """The screen's T = fmaf(|nsdf| + 0.2f, 2^-16, nsdf + 0.11f): the product by 2^-16 and the f64 sum
    of the two f32 terms are exact for the surface values used here, so one rounding remains."""
    n = np.asarray(nsdf, F)
    with np.errstate(all="ignore"):
        return _f((np.abs(n) + F(0.2)).astype(D) * 2.0 ** -16 + (n + F(0.11)).astype(D))


def screen_far(P, nsdf, frame):
    """[n, 9] bool: the lanes whose sphere i passes the screen q[i] >= T2 = max(T, 0)^2."""
    T = screen_T(np.broadcast_to(np.asarray(nsdf, F), (len(P),)))
    with np.errstate(all="ignore"):
        Tc = np.where(T < 0, F(0), T).astype(F)
        return sphere_q(P, frame) >= (Tc * Tc)[:, None]


def q_in_domain(P, frame):
    """[n] bool: the lane's bounds put its nine q in sqrt_rn_normal's domain [2^-96, FLT_MAX]."""
    q = sphere_q(P, frame)
    with np.errstate(all="ignore"):
        return (q.min(1) >= F(2.0 ** -96)) & (q.max(1) <= np.finfo(F).max)


def _smooth_sub(d1, d2, k):
    """sdfOpSmoothSubtraction in the reference's promotions (always the division)."""
    t = (d1 + d2).astype(F)
    h = _f(0.5 - 0.5 * t.astype(D) / D(k))
    h = np.where(h > 0, np.minimum(h, F(1)), F(0)).astype(F)
    mix = _f(d1.astype(D) * (1.0 - h.astype(D)) - (d2 * h).astype(F).astype(D))
    return t, _f(mix.astype(D) + (k * h).astype(F).astype(D) * (1.0 - h.astype(D)))


def sub_chain_t(P, nsdf, scene, frame=0):
    """[n, m] f32: d1 + d2 of every smooth subtraction of the chain (m = 9 spheres of "subtract", 300
    cylinders of "cylinders", in the chain's order), d1 the running value.  |t| < k is where the
    kernel's shortcut does not apply."""
    P = np.asarray(P, F)
    s = np.broadcast_to(np.asarray(nsdf, F), (len(P),)).astype(F)
    k = F(SMOOTH_K)
    ts = []
    with np.errstate(all="ignore"):
        if scene == "subtract":
            d = (np.sqrt(sphere_q(P, frame)) - F(SPHERE_R)).astype(F)
            for i in range(9):
                t, s = _smooth_sub(s, d[:, i], k)
                ts.append(t)
        else:
            cy = _f(P[:, 1].astype(D) - 0.5)
            for row in range(15):
                cy = _f(cy.astype(D) + 0.1)
                dy = cy - F(CYL_R)
                cx = _f(P[:, 0].astype(D) + 0.9)
                for col in range(20):
                    dx = cx - F(CYL_R)
                    t, s = _smooth_sub(s, (np.sqrt(dx * dx + dy * dy) - F(CYL_R)).astype(F), k)
                    ts.append(t)
                    cx = _f(cx.astype(D) - 0.1)
    return np.stack(ts, -1)


def far_counts(far_column):
    """Far lanes per 64-point chunk."""
    return [int(far_column[i:i + WAVE].sum()) for i in range(0, len(far_column), WAVE)]


# ---- lattices -----------------------------------------------------------------

def _line(axis, start, fixed, step, n):
    origin = [F(v) for v in fixed]
    origin[axis] = F(start)
    st = [F(0)] * 3
    st[axis] = F(step)
    dims = [1, 1, 1]
    dims[axis] = n
    return tuple(float(v) for v in origin), tuple(float(v) for v in st), tuple(dims)


def _centred(count_fn, axis, guess, fixed, step, n):
    """The n-point line along `axis` whose crossing (count_fn(points) = lanes beyond it, which sit at
    the line's far end) falls in the middle of the middle chunk: the start is moved by whole steps
    until half the line is beyond."""
    start = guess - (n // 2) * step
    for _ in range(12):
        o, s, dims = _line(axis, start, fixed, step, n)
        beyond = count_fn(mesh_ref.lattice(o, s, dims))
        if abs(beyond - n // 2) <= 4:
            break
        start -= (beyond - n // 2) * step
    return o, s, dims


def screen_line(c, sphere, step, frame):
    """192 points (three chunks) along x (frame 180: zoff = 0) or z (frame 0) through sphere
    `sphere`'s centre line, crossing sqrt(q) = T: the middle chunk straddles the screen, the first is
    all-near and the last all-far for that sphere."""
    assert frame in (0, 180)
    cx, cy, cz = SPHERE_X[sphere % 3], SPHERE_Y[sphere // 3], -sphere_zoff(frame)
    T = float(screen_T(F(c)))
    assert T > 0
    axis = 0 if frame == 180 else 2
    centre = (cx, cy, cz)
    o, s, dims = _centred(lambda P: int(screen_far(P, c, frame)[:, sphere].sum()), axis, centre[axis] + T, centre,
                          step, 3 * WAVE)
    return o, s, dims, frame


def box_lattice():
    """9 x 9 x 5 over the sphere grid (405 points: six chunks and a tail of 21)."""
    return (-0.6, -0.7, -0.1), (0.125, 0.125, 0.05), (9, 9, 5), 180


def scattered_lattice(frame=180):
    """One chunk whose 64 lanes sit at or next to different sphere centres."""
    return (-0.5, -0.2, 0.0), (0.4, 0.4, 0.4), (4, 4, 4), frame


def overflow_lattice(ystep=2e19, nan_origin=False, z=0.05):
    """One chunk of two rows: with ystep 2e19 the second row's q overflows to inf (the whole wave
    takes the sqrtf chain), with 1e19 it stays finite near FLT_MAX (the short root's upper end);
    nan_origin: every x is NaN.  With z = 0.05 the finite row is near every sphere; with z = 1 it is
    far from all nine, so only the domain ballot keeps the wave from screening them: inf >= T2 holds,
    but the union with an infinite distance is fmaf(inf, 0, s) = NaN, not s + 0."""
    return (float("nan") if nan_origin else -0.6, -0.2, z), (0.04, ystep, 0.1), (32, 2, 1), 180


def nonfinite_lattice():
    return (-0.6, -0.7, -0.1), (0.15, 0.3, 0.2), (8, 4, 2), 3


def range_line():
    """4096 points of x in [-1.2, 1.2]: with linear_net((a, 0, 0)) nsdf = fl(a x)."""
    return (-1.2, 0.1, 0.2), (2.4 / 4095, 0.0, 0.0), (4096, 1, 1), 0


def tiny_line():
    """x = i 2^-100: arguments far below any threshold of nr_tanh / nr_sin, zero included."""
    return (0.0, 0.1, 0.2), (2.0 ** -100, 0.0, 0.0), (64, 1, 1), 0


def large_lattice():
    """|p| up to 3000 on multiples of 2^-8 (5 p is exact in f32): nr_sin's reduction runs with k up
    to ~9500, and the inputs are beyond the fp32 pack's clamp bound (the add + max form)."""
    return (-3000.0, -2500.5, -2000.25), (399.90625, 713.6875, 571.09375), (16, 8, 8), 0


def sin_quadrants(P):
    """k mod 4 of nr_sin's reduction for the three arguments 5 p (f32 products)."""
    x = (F(5) * np.asarray(P, F)).astype(D)
    kd = np.floor(x * 0.63661977236758134308 + 0.5)
    return (kd - 4.0 * np.floor(kd * 0.25)).astype(int), kd


def subtract_line(c, sign, step=2.0 ** -24):
    """192 points along x through the first sphere's centre line (frame 180) across d1 + d2 = sign k,
    d1 = c: the sphere is first in the chain, so d1 is the surface value itself.  Where no such
    point exists (c - 0.1 > k: d1 + d2 >= k everywhere) the line starts at the centre instead."""
    cx, cy = SPHERE_X[0], SPHERE_Y[0]
    dist = SPHERE_R - c + sign * SMOOTH_K
    if dist <= 0:
        return _line(0, cx, (cx, cy, 0.0), step, 3 * WAVE) + (180,)
    k = F(SMOOTH_K) if sign > 0 else -F(SMOOTH_K)
    cnt = (lambda P: int((sub_chain_t(P, c, "subtract", 180)[:, 0] >= k).sum())) if sign > 0 else \
          (lambda P: int((sub_chain_t(P, c, "subtract", 180)[:, 0] > k).sum()))
    return _centred(cnt, 0, cx + dist, (cx, cy, 0.0), step, 3 * WAVE) + (180,)


def cylinder_line(c, row, col, sign, step=2.0 ** -24):
    """The same across cylinder (row, col) of the 15 x 20 grid of manyCylinderCut, towards +x."""
    cx, cy = -0.88 + 0.1 * col, 0.42 - 0.1 * row
    dist = CYL_R - c + sign * SMOOTH_K
    i = 20 * row + col
    if dist <= 0:
        return _line(0, cx, (cx, cy, 0.3), step, 3 * WAVE) + (0,)
    k = F(SMOOTH_K) if sign > 0 else -F(SMOOTH_K)
    cnt = (lambda P: int((sub_chain_t(P, c, "cylinders")[:, i] >= k).sum())) if sign > 0 else \
          (lambda P: int((sub_chain_t(P, c, "cylinders")[:, i] > k).sum()))
    return _centred(cnt, 0, cx + dist, (cx, cy, 0.3), step, 3 * WAVE) + (0,)


CYL_TARGETS = ((7, 0), (7, 19), (0, 10), (14, 10))  # first column, last column, first row, last row


# ---- the point sets of tests/test_gpu_scene_points.py -------------------------

class Case:
    """One nr_sample_grid call: a network, a scene and a lattice.  `device`: also run on the device
    path; `info`: what the lattice was built against (for the condition tests)."""

    def __init__(self, group, name, net, scene, lattice, device=False, **info):
        self.group, self.net, self.scene, self.device, self.info = group, net, scene, device, info
        self.origin, self.step, self.dims, self.frame = lattice
        self.id = f"{group}-{name}"

    def network(self):
        kind, args = self.net[0], self.net[1:]
        return (const_net if kind == "const" else linear_net)(*args)

    def points(self):
        return mesh_ref.lattice(self.origin, self.step, self.dims)


def _fmt(v):
    return "%g" % v if np.isfinite(v) else str(v)


def _fmt_c(c):
    return "m0" if (c == 0 and np.signbit(c)) else _fmt(c)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # 1: the screen's threshold
    for c in (1.0, 0.3, 0.0, -0.0, -0.05):
        for frame in (180, 0):
            for e in (24, 22):
                for sphere in (0, 4, 8):
                    out.append(Case("screen", f"c{_fmt_c(c)}-f{frame}-s{sphere}-2^-{e}", ("const", c), "v1",
                                    screen_line(c, sphere, 2.0 ** -e, frame),
                                    device=(c == 0.3 and frame == 180 and e == 24 and sphere == 4), c=c, sphere=sphere))
    # 2: T <= 0, and inside a sphere
    for c in (-0.11, -0.2, -1.0, -5.0):
        out.append(Case("inside", f"c{_fmt(c)}", ("const", c), "v1", box_lattice(), device=(c == -0.2), c=c))
    # 3: a scattered wave
    out.append(Case("scattered", "c0.3", ("const", 0.3), "v1", scattered_lattice(), device=True, c=0.3))
    out.append(Case("scattered", "z+0.05", ("linear", (0.0, 0.0, 1.0), 0.05), "v1", scattered_lattice()))
    # 4: one overflowing lane
    for name, lat in (("inf", overflow_lattice(2e19)), ("max", overflow_lattice(1e19)),
                      ("nan", overflow_lattice(2e19, nan_origin=True))):
        for scene in SCENES:
            out.append(Case("overflow", f"{name}-{scene}", ("const", 0.3), scene, lat,
                            device=(name == "inf" and scene == "v1"), kind=name))
    # the same with every finite lane beyond the screen for all nine spheres (z = 1), or T <= 0 (c = -0.2)
    for scene in SCENES:
        out.append(Case("overflow", f"far-{scene}", ("const", 0.3), scene, overflow_lattice(2e19, z=1.0), kind="far", c=0.3))
    out.append(Case("overflow", "far-neg-v1", ("const", -0.2), "v1", overflow_lattice(2e19), kind="far-neg", c=-0.2))
    # 5: non-finite and tiny surface values
    for c in (float("nan"), float("inf"), float("-inf"), 1e-30, -1e-30, 2.0 ** -127):
        for scene in SCENES:
            out.append(Case("values", f"c{_fmt(c)}-{scene}", ("const", c), scene, nonfinite_lattice(),
                            device=(np.isnan(c) and scene == "v1"), c=c))
    # 6: the argument ranges of nr_tanh and nr_sin
    for a in (16.0, 1.0, 2.0 ** -20):
        for scene in ("tanh", "round", "displace"):
            out.append(Case("ranges", f"a{_fmt(a)}-{scene}", ("linear", (a, 0.0, 0.0)), scene, range_line(),
                            device=(a == 16.0 and scene == "displace"), a=a))
    for a in (16.0, 1.0):
        out.append(Case("ranges", f"tiny-a{_fmt(a)}", ("linear", (a, 0.0, 0.0)), "displace", tiny_line(), a=a))
    out.append(Case("ranges", "large-displace", ("linear", (1.0, 0.0, 0.0)), "displace", large_lattice(), a=1.0))
    # 7: the shortcuts of the subtract and cylinders scenes
    for c in (0.3, 0.0, -0.05):
        for sign in (1, -1):
            sg = "+k" if sign > 0 else "-k"
            out.append(Case("subtract", f"c{_fmt(c)}{sg}", ("const", c), "subtract", subtract_line(c, sign),
                            device=(c == 0.0 and sign > 0), c=c, sign=sign, target=0))
            for row, col in CYL_TARGETS:
                out.append(Case("cylinders", f"c{_fmt(c)}{sg}-r{row}c{col}", ("const", c), "cylinders",
                                cylinder_line(c, row, col, sign), device=(c == 0.0 and sign > 0 and col == 19),
                                c=c, sign=sign, target=20 * row + col))
    # 8: four inputs
    for frame in (0, 45, 359):
        out.append(Case("four", f"f{frame}", ("linear", (0.0, 0.0, 0.0, 1.0 / 360.0), 0.0, 2, 4), "v1",
                        scattered_lattice(frame), device=(frame == 45)))
    assert len({c.id for c in out}) == len(out)
    return tuple(out)


def case_ids():
    return [c.id for c in cases()]


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """(nsdf [n], values [nz, ny, nx]) of a case through the oracle: OracleNet.forward, then
    oracle.scene_sdf per point.  Computed once, shared, read-only."""
    case = next(c for c in cases() if c.id == case_id)
    dims, K, B = case.network()
    P = case.points()
    X = P if dims[0] == 3 else np.concatenate([P, np.full((len(P), 1), F(case.frame), F)], 1)
    with np.errstate(all="ignore"):
        nsdf = oracle.OracleNet(K, B).forward(X)[:, 0]
        v = np.array([oracle.scene_sdf(p, s, SCENE_ID[case.scene], case.frame) for p, s in zip(P, nsdf)], F)
    v = v.reshape(case.dims[::-1])
    nsdf.setflags(write=False)
    v.setflags(write=False)
    return nsdf, v


# ---- the plain float64 restatement of the six scenes ---------------------------

def _su(d1, d2, k):
    h = np.clip(0.5 + 0.5 * (d2 - d1) / k, 0.0, 1.0)
    return d2 * (1.0 - h) + d1 * h - k * h * (1.0 - h)


def _ss(d1, d2, k):
    h = np.clip(0.5 - 0.5 * (d1 + d2) / k, 0.0, 1.0)
    return d1 * (1.0 - h) - d2 * h + k * h * (1.0 - h)


def plain_scene(P, nsdf, scene, frame):
    """sceneSDF in numpy float64 from the formulae (np.tanh, np.sin, the smooth operators, the sphere
    and cylinder grids by arithmetic): no f32 step but the sine's argument, which is the f32 product
    5 p the scene is defined on (its rounding is part of the input, not of the evaluation)."""
    P = np.asarray(P, F)
    x, y, z = (P[:, i].astype(D) for i in range(3))
    s = np.asarray(nsdf, F).astype(D)
    if scene == "tanh":
        return np.tanh(s)
    if scene == "round":
        return np.tanh(s) - 0.04
    if scene == "displace":
        a = (F(5) * P).astype(D)
        return np.tanh(s) + np.sin(a[:, 0]) * np.sin(a[:, 1]) * np.sin(a[:, 2]) * 0.05
    if scene == "cylinders":
        for row in range(15):
            for col in range(20):
                s = _ss(s, np.hypot(x - (-0.88 + 0.1 * col), y - (0.42 - 0.1 * row)) - CYL_R, SMOOTH_K)
        return s
    cz = 0.7 - 2.0 * frame * 0.7 / 360.0
    op = _su if scene == "v1" else _ss
    for row in range(3):
        for col in range(3):
            d = np.sqrt((x - SPHERE_X[col]) ** 2 + (y - SPHERE_Y[row]) ** 2 + (z - cz) ** 2) - SPHERE_R
            s = op(s, d, SMOOTH_K)
    return s
