"""Reference for nr_render_lit: a helper, not a test.

The numpy restatement of rules 1-5 of include/neural_render.h, built only from tests/query_ref.py
(the geometry buffer, the MLP, the scene, the ray entry) and what the CPU oracle exports, with all
arithmetic in np.float32, one rounding per operation.  tests/test_light_cpu.py pins its shadow
march against query_ref.trace and its composite against the oracle's frames.
"""
import numpy as np

import oracle
import query_ref
from query_ref import ESCAPED, F, HIT, LIMIT, MARCHING_EPSILON, MISS, dot3

AO_W = np.array([1.0, 0.5, 0.25, 0.125], F)
# rule 5's identity settings: f is exactly 1
LIGHT_OFF = dict(shadow_steps=0, shadow_bias=0.0, shadow_k=0.0, ao_step=0.0, ao_strength=0.0, ambient=1.0)


def sat(x):
    """saturatef_: NaN -> 0."""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        return np.where(x > 0, np.minimum(x, F(1)), F(0)).astype(F)


def ndl_of(normal, L):
    """Rule 2: dd = dot3(n, L), ndl = dd > 0 ? dd : 0 (NaN -> 0)."""
    with np.errstate(all="ignore"):
        dd = dot3(np.asarray(normal, F).reshape(-1, 3), np.asarray(L, F))
        return np.where(dd > 0, dd, F(0)).astype(F)


def ambient_occlusion(net, P, N, ao_step, ao_strength, scene=0, frame=0):
    """Rule 3 for the points P with normals N (ao_strength > 0)."""
    P, N = np.asarray(P, F).reshape(-1, 3), np.asarray(N, F).reshape(-1, 3)
    c = []
    with np.errstate(all="ignore"):
        for q in range(4):
            h = F(F(q + 1) * F(ao_step))
            a = (P + N * h).astype(F)
            s = query_ref._scene(a, query_ref._mlp(net, a, frame), scene, frame)
            c.append(((h - s) * AO_W[q]).astype(F))
        occ = ((c[0] + c[1]) + c[2]) + c[3]
        return sat(F(1) - F(ao_strength) * occ)


def shadow_march(net, origins, L, shadow_steps, shadow_k, scene=0, frame=0):
    """Rule 4's march of the rays (origins[i], L): query_ref.trace's loop with the running minimum
    res.  Returns (shadow, status, steps)."""
    O = np.ascontiguousarray(origins, F).reshape(-1, 3)
    n = O.shape[0]
    D = np.broadcast_to(np.asarray(L, F), O.shape).copy()
    k = F(shadow_k)
    status = np.zeros(n, np.int32)
    steps = np.zeros(n, np.int32)
    res = np.ones(n, F)
    with np.errstate(all="ignore"):
        ref = oracle.intersect_pair(O, D)[0] if n else np.zeros((0, 3), F)
        entered = ref[:, 0] != 0
        tnear = np.where(ref[:, 1] < 0, F(0), ref[:, 1]).astype(F)
        tfar = ref[:, 2].astype(F).copy()
        P = (O + D * tnear[:, None]).astype(F)
        travel = np.zeros(n, F)
        live = entered.copy()
        for it in range(shadow_steps):
            idx = np.flatnonzero(live)
            if idx.size == 0:
                break
            ts = query_ref._scene(P[idx], query_ref._mlp(net, P[idx], frame), scene, frame)
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
            conv = go[tg < MARCHING_EPSILON]
            status[idx[esc]] = ESCAPED
            status[conv] = HIT if it + 1 < shadow_steps else LIMIT
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
    return shadow, status, steps


def composite(base, ao, shadow, ndl, ambient):
    """Rule 5 on the uint32 frame `base` (flat arrays of one length)."""
    base = np.asarray(base, np.uint32).reshape(-1)
    amb = F(ambient)
    with np.errstate(all="ignore"):
        f = (ao * (amb + (F(1) - amb) * (shadow * ndl).astype(F)).astype(F)).astype(F)
        out = base & np.uint32(0xff000000)
        for sh in (0, 8, 16):
            ch = (((base >> np.uint32(sh)) & np.uint32(0xff)).astype(F) * f).astype(F)
            out = out | (np.minimum(ch, F(255)).astype(np.uint32) << np.uint32(sh))
    return out.astype(np.uint32)


def render(net, W, H, inv_view, max_steps, L, shadow_steps, shadow_bias, shadow_k, ao_step, ao_strength, ambient,
           scene=0, frame=0):
    """nr_render_lit's outputs and stats for the facing colouring, and what the tests assert about
    the inputs: "gbuffer" (query_ref.trace of the pixel rays), "ndl", and the shadow rays' pixel
    indices, status and steps ("ray_pix", "ray_status", "ray_steps")."""
    O, D = query_ref.pixel_rays(W, H, inv_view)
    g, gst = query_ref.trace(net, O, D, max_steps, scene=scene, frame=frame)
    n = W * H
    hit = np.flatnonzero(g["status"] == HIT)
    P, N = g["position"][hit], g["normal"][hit]
    ao = np.ones(n, F)
    shadow = np.ones(n, F)
    ndl = np.zeros(n, F)
    ndl[hit] = ndl_of(N, L)
    if ao_strength > 0 and hit.size:
        ao[hit] = ambient_occlusion(net, P, N, ao_step, ao_strength, scene, frame)
    ray_pix = np.zeros(0, np.int64)
    rstatus, rsteps = np.zeros(0, np.int32), np.zeros(0, np.int32)
    if shadow_steps > 0:
        shadow[hit] = F(0)
        ray_pix = hit[ndl[hit] > 0]
        with np.errstate(all="ignore"):
            o = (g["position"][ray_pix] + g["normal"][ray_pix] * F(shadow_bias)).astype(F)
        shadow[ray_pix], rstatus, rsteps = shadow_march(net, o, L, shadow_steps, shadow_k, scene, frame)
    base = query_ref.facing(g["normal"], D, g["status"])
    out = composite(base, ao, shadow, ndl, ambient)
    stats = {"ray_steps": gst["ray_steps"] + int(rsteps.sum()), "rays_hit": gst["rays_hit"],
             "rays_shaded": gst["rays_shaded"], "shade_evals": (8 if ao_strength > 0 else 4) * int(hit.size),
             "iterations": max(gst["iterations"], int(rsteps.max()) if rsteps.size else 0)}
    return {"out": out.reshape(H, W), "ao": ao.reshape(H, W), "shadow": shadow.reshape(H, W), "ndl": ndl.reshape(H, W),
            "gbuffer": g, "base": base.reshape(H, W), "ray_pix": ray_pix, "ray_status": rstatus, "ray_steps": rsteps,
            "stats": stats}
