"""Reference for nr_compose_render_lit: a helper, not a test.

The numpy restatement of the contract in include/neural_render.h (nr_render_lit's rules with the
composed field and the composed ray rule), built only from compose_ref.field / intersect / trace,
light_ref.sat / ndl_of / composite / AO_W and query_ref.pixel_rays / facing, all arithmetic in
np.float32, one rounding per operation.  tests/test_compose_light_cpu.py pins its shadow march to
compose_ref.trace and its occlusion to light_ref.ambient_occlusion.
"""
import numpy as np

import compose_ref
import query_ref
from light_ref import AO_W, composite, ndl_of, sat
from query_ref import ESCAPED, HIT, LIMIT, MARCHING_EPSILON, MISS

F = np.float32


def ambient_occlusion(nets, parts, P, N, ao_step, ao_strength, frame=0):
    """Rule 3 through the composed field, for the points P with normals N (ao_strength > 0)."""
    P, N = np.asarray(P, F).reshape(-1, 3), np.asarray(N, F).reshape(-1, 3)
    c = []
    with np.errstate(all="ignore"):
        for q in range(4):
            h = F(F(q + 1) * F(ao_step))
            a = (P + N * h).astype(F)
            s = compose_ref.field(nets, parts, a, frame)[0]
            c.append(((h - s) * AO_W[q]).astype(F))
        occ = ((c[0] + c[1]) + c[2]) + c[3]
        return sat(F(1) - F(ao_strength) * occ)


def shadow_march(nets, parts, center, radius, origins, L, shadow_steps, shadow_k, frame=0):
    """The march of the rays (origins[i], L): compose_ref.trace's loop with rule 4's running minimum
    res.  Returns (shadow, status, steps, occluder, in-bound (marching ray, part) pairs)."""
    O = np.ascontiguousarray(origins, F).reshape(-1, 3)
    n = O.shape[0]
    D = np.broadcast_to(np.asarray(L, F), O.shape).copy()
    k = F(shadow_k)
    status = np.zeros(n, np.int32)
    steps = np.zeros(n, np.int32)
    occluder = np.full(n, -1, np.int32)
    res = np.ones(n, F)
    pairs_sum = 0
    with np.errstate(all="ignore"):
        entered, tn, tf = compose_ref.intersect(O, D, center, radius)
        tnear = np.where(tn < 0, F(0), tn).astype(F)
        tfar = (tf - tnear).astype(F)
        P = (O + D * tnear[:, None]).astype(F)
        travel = np.zeros(n, F)
        live = entered.copy()
        for it in range(shadow_steps):
            idx = np.flatnonzero(live)
            if idx.size == 0:
                break
            ts, own, pairs = compose_ref.field(nets, parts, P[idx], frame)
            pairs_sum += pairs
            dist = (tnear[idx] + travel[idx]).astype(F)
            r = ((k * ts).astype(F) / dist).astype(F)
            lower = (dist > 0) & (r < res[idx])
            res[idx[lower]] = r[lower]
            tfar[idx] = tfar[idx] - ts
            esc = tfar[idx] <= 0
            go = idx[~esc]
            tg = ts[~esc]
            P[go] = P[go] + D[go] * tg[:, None]
            travel[go] = travel[go] + tg
            cv = tg < MARCHING_EPSILON
            conv = go[cv]
            status[idx[esc]] = ESCAPED
            status[conv] = HIT if it + 1 < shadow_steps else LIMIT
            if it + 1 < shadow_steps:
                occluder[conv] = own[~esc][cv]
            done = np.concatenate([idx[esc], conv])
            steps[done] = it + 1
            live[done] = False
        rest = np.flatnonzero(live)
        status[rest] = LIMIT
        steps[rest] = shadow_steps
        shadow = np.zeros(n, F)  # HIT, LIMIT
        shadow[status == MISS] = F(1)
        e = status == ESCAPED
        shadow[e] = sat(res[e]) if k > 0 else F(1)
    return shadow, status, steps, occluder, pairs_sum


def render(nets, parts, center, radius, W, H, inv_view, max_steps, L, shadow_steps, shadow_bias, shadow_k, ao_step,
           ao_strength, ambient, frame=0):
    """nr_compose_render_lit's outputs and grouping-independent stats for the facing colouring, and
    what the tests assert about the inputs: "gbuffer" (compose_ref.trace of the pixel rays), "ndl",
    "base", and the shadow rays' pixel indices, status and steps ("ray_pix", "ray_status",
    "ray_steps")."""
    O, D = query_ref.pixel_rays(W, H, inv_view)
    g, gst = compose_ref.trace(nets, parts, center, radius, O, D, max_steps, frame)
    n = W * H
    hit = np.flatnonzero(g["status"] == HIT)
    P, N = g["position"][hit], g["normal"][hit]
    ao = np.ones(n, F)
    shadow = np.ones(n, F)
    occluder = np.full(n, -1, np.int32)
    ndl = np.zeros(n, F)
    ndl[hit] = ndl_of(N, L)
    if ao_strength > 0 and hit.size:
        ao[hit] = ambient_occlusion(nets, parts, P, N, ao_step, ao_strength, frame)
    ray_pix = np.zeros(0, np.int64)
    rstatus, rsteps, pairs = np.zeros(0, np.int32), np.zeros(0, np.int32), 0
    if shadow_steps > 0:
        shadow[hit] = F(0)
        ray_pix = hit[ndl[hit] > 0]
        with np.errstate(all="ignore"):
            o = (g["position"][ray_pix] + g["normal"][ray_pix] * F(shadow_bias)).astype(F)
        shadow[ray_pix], rstatus, rsteps, occluder[ray_pix], pairs = shadow_march(nets, parts, center, radius, o, L,
                                                                                  shadow_steps, shadow_k, frame)
    base = query_ref.facing(g["normal"], D, g["status"])
    out = composite(base, ao, shadow, ndl, ambient)
    stats = {"ray_steps": gst["ray_steps"] + int(rsteps.sum()), "rays_hit": gst["rays_hit"],
             "rays_shaded": gst["rays_shaded"], "shade_evals": (8 if ao_strength > 0 else 4) * int(hit.size),
             "iterations": max(gst["iterations"], int(rsteps.max()) if rsteps.size else 0),
             "part_evals": gst["part_evals"] + pairs}
    return {"out": out.reshape(H, W), "ao": ao.reshape(H, W), "shadow": shadow.reshape(H, W),
            "part": g["part"].reshape(H, W), "occluder": occluder.reshape(H, W), "ndl": ndl.reshape(H, W),
            "gbuffer": g, "base": base.reshape(H, W), "ray_pix": ray_pix, "ray_status": rstatus, "ray_steps": rsteps,
            "stats": stats}
