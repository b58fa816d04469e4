"""Reference for the ray queries (nr_trace_rays / nr_render_gbuffer): a helper, not a test.

The numpy restatement of the ray semantics of include/neural_render.h, built only from what the
CPU oracle exports -- the entry from oracle.intersect_pair's reference form, the MLP from
OracleNet.forward (fp32), the step from oracle.scene_sdf per point -- with all ray arithmetic in
np.float32, one rounding per operation.  tests/test_query_cpu.py pins it against or_render's
frames bit for bit, so the oracle stays the yardstick and this file only transposes it.
"""
import numpy as np

import oracle

MISS, ESCAPED, HIT, LIMIT = 0, 1, 2, 3
F = np.float32
TET = np.array([[1, -1, -1], [-1, -1, 1], [-1, 1, -1], [1, 1, 1]], F)  # c_tet, volumeRender_kernel.cu:38-43
NORMAL_EPSILON = F(0.00001)
MARCHING_EPSILON = F(0.000001)


def dot3(a, b):
    """helper_math.h:1258 in f32: (a0 b0 + a1 b1) + a2 b2."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def normalize3(v):
    """helper_math.h:1309-1313: v * (1 / sqrt(dot(v, v)))."""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        inv = F(1.0) / np.sqrt(dot3(v, v))
        return v * inv[..., None]


def _mlp(net, P, frame):
    P = np.ascontiguousarray(P, F)
    if int(net.dims[0]) == 4:
        P = np.concatenate([P, np.full((P.shape[0], 1), F(frame), F)], 1)
    return net.forward(P)[:, 0]


def _scene(P, sdf, scene, frame):
    return np.array([oracle.scene_sdf(p, s, scene, frame) for p, s in zip(P, sdf)], F).reshape(-1)


def trace(net, origins, dirs, max_steps, scene=0, frame=0, normals=True):
    """The five outputs of nr_trace_rays and its stats for rays (origins, dirs)."""
    O = np.ascontiguousarray(origins, F).reshape(-1, 3)
    D = np.ascontiguousarray(dirs, F).reshape(-1, 3)
    n = O.shape[0]
    status = np.zeros(n, np.int32)
    steps = np.zeros(n, np.int32)
    t = np.zeros(n, F)
    position = np.zeros((n, 3), F)
    normal = np.zeros((n, 3), F)
    with np.errstate(all="ignore"):
        ref = oracle.intersect_pair(O, D)[0] if n else np.zeros((0, 3), F)
        entered = ref[:, 0] != 0
        tnear = np.where(ref[:, 1] < 0, F(0), ref[:, 1]).astype(F)
        tfar = ref[:, 2].astype(F).copy()
        P = (O + D * tnear[:, None]).astype(F)
        travel = np.zeros(n, F)
        live = entered.copy()
        for it in range(max_steps):
            idx = np.flatnonzero(live)
            if idx.size == 0:
                break
            ts = _scene(P[idx], _mlp(net, P[idx], frame), scene, frame)
            tfar[idx] = tfar[idx] - ts
            esc = tfar[idx] <= 0
            go = idx[~esc]
            tg = ts[~esc]
            P[go] = P[go] + D[go] * tg[:, None]
            travel[go] = travel[go] + tg
            conv = go[tg < MARCHING_EPSILON]
            status[idx[esc]] = ESCAPED
            status[conv] = HIT if it + 1 < max_steps else LIMIT
            done = np.concatenate([idx[esc], conv])
            steps[done] = it + 1
            live[done] = False
        rest = np.flatnonzero(live)
        status[rest] = LIMIT
        steps[rest] = max_steps
        hit = np.flatnonzero(status == HIT)
        t[hit] = tnear[hit] + travel[hit]
        position[hit] = P[hit]
        if normals and hit.size:
            acc = None
            for q in range(4):
                pq = (P[hit] + TET[q] * NORMAL_EPSILON).astype(F)
                c = TET[q][None, :] * _scene(pq, _mlp(net, pq, frame), scene, frame)[:, None]
                acc = c if acc is None else acc + c
            normal[hit] = normalize3(acc)
    out = {"status": status, "steps": steps, "t": t, "position": position}
    if normals:
        out["normal"] = normal
    stats = {"ray_steps": int(steps.sum()), "shade_evals": 4 * int(hit.size) if normals else 0,
             "rays_hit": int(entered.sum()), "rays_shaded": int(hit.size), "iterations": int(steps.max()) if n else 0}
    return out, stats


def pixel_rays(W, H, inv_view):
    """(origins, dirs) of the W x H pixel rays, index y W + x: or_render_ex's initMarcher lines."""
    M = np.asarray(inv_view, F).reshape(3, 4)
    z, one = F(0), F(1)
    o = np.array([((z * r[0] + z * r[1]) + z * r[2]) + one * r[3] for r in M], F)
    y, x = np.mgrid[0:H, 0:W]
    u = (x.astype(F) / F(W)) * F(2) - F(1)
    v = (y.astype(F) / F(H)) * F(2) - F(1)
    d = normalize3(np.stack([u, v, np.full_like(u, F(-2))], -1).astype(F).reshape(-1, 3))
    D = np.stack([dot3(d, M[0, :3]), dot3(d, M[1, :3]), dot3(d, M[2, :3])], -1).astype(F)
    return np.broadcast_to(o, D.shape).copy(), D


def facing(normal, dirs, status):
    """The facing-colour pixel of each ray: facingColor / rgbaFloatToInt for a HIT, else 0."""
    nrm = np.asarray(normal, F).reshape(-1, 3)
    D = np.asarray(dirs, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        dd = dot3(nrm, -D)
        ratio = np.where(dd > 0, dd, F(0)).astype(F)

        def chan(c):
            c = np.where(c > 0, np.minimum(c, F(1)), F(0)).astype(F)  # __saturatef (NaN -> 0)
            return (c * F(255)).astype(np.uint32)  # truncation

        r, a = chan(ratio), chan(np.ones_like(ratio))
    px = (a << 24) | (r << 16) | (r << 8) | r
    return np.where(np.asarray(status).reshape(-1) == HIT, px, 0).astype(np.uint32)
