"""Reference for composed scenes (nr_compose_*): a helper, not a test.

The numpy restatement of the contract in include/neural_render.h, built only from
OracleNet.forward (fp32), oracle.tanh_f and np.float32 arithmetic, one rounding per operation.  The
world bound is an argument (the tests take it from nr_compose_info / nr_compose_bound).
tests/test_compose_cpu.py pins it to query_ref.trace for a lone identity part.
"""
import numpy as np

import oracle
from query_ref import HIT, LIMIT, ESCAPED, MARCHING_EPSILON, NORMAL_EPSILON, TET, dot3, normalize3

F = np.float32
UNION, SUBTRACT = 0, 1
IN_BOUND = F(1.45)    # the network is evaluated where qq <= 1.45
BOUND_OFF = F(1.19)   # elsewhere the term is scale * (sqrt(qq) - 1.19)


def rot_xyz(rx, ry, rz):
    """Rz(rz) Ry(ry) Rx(rx) in double, rounded once to float32 (radians)."""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    X = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Y = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Z = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Z @ Y @ X).astype(F)


def part(net, op=UNION, rot=None, pos=(0, 0, 0), scale=1.0):
    return {"net": int(net), "op": int(op), "rot": np.eye(3, dtype=F) if rot is None else np.asarray(rot, F).reshape(3, 3),
            "pos": np.asarray(pos, F).reshape(3), "scale": F(scale)}


def _mlp(net, P, frame):
    P = np.ascontiguousarray(P, F)
    if int(net.dims[0]) == 4:
        P = np.concatenate([P, np.full((P.shape[0], 1), F(frame), F)], 1)
    return net.forward(P)[:, 0]


def _tanh(x):
    return np.array([oracle.tanh_f(v) for v in x], F).reshape(-1)


def fold(terms, ops):
    """The fold over the parts' terms [nparts][n] in part order: (value, owner).  NaN comparisons are
    false, so a NaN term is never taken (a NaN d_0 stays)."""
    with np.errstate(all="ignore"):
        d = np.array(terms[0], F, copy=True)
        owner = np.zeros(d.shape, np.int32)
        for j in range(1, len(terms)):
            dj = np.asarray(terms[j], F)
            if ops[j] == SUBTRACT:
                nd = -dj
                take = nd > d
                d = np.where(take, nd, d)
            else:
                take = dj < d
                d = np.where(take, dj, d)
            owner = np.where(take, np.int32(j), owner)
    return d.astype(F), owner.astype(np.int32)


def field(nets, parts, P, frame=0):
    """(value, owner, in-bound (point, part) pairs) of the composed field at the points P [n, 3]."""
    P = np.ascontiguousarray(P, F).reshape(-1, 3)
    terms, pairs = [], 0
    with np.errstate(all="ignore"):
        for p in parts:
            R = p["rot"].reshape(9)
            s = F(p["scale"])
            inv_s = F(1.0) / s
            v = (P - p["pos"][None, :]).astype(F)
            q = np.stack([((v[:, 0] * R[0 + k] + v[:, 1] * R[3 + k]) + v[:, 2] * R[6 + k]) * inv_s for k in range(3)], 1).astype(F)
            qq = dot3(q, q)
            inb = qq <= IN_BOUND
            dj = (s * (np.sqrt(qq) - BOUND_OFF)).astype(F)
            if inb.any():
                dj[inb] = s * _tanh(_mlp(nets[p["net"]], q[inb], frame))
            pairs += int(inb.sum())
            terms.append(dj)
    d, owner = fold(terms, [p["op"] for p in parts])
    return d, owner, pairs


def intersect(O, D, center, radius):
    """intersect_bounding's arithmetic on Q = o - c and r * r: (entered, tnear, tfar)."""
    c = np.asarray(center, F).reshape(3)
    r = F(radius)
    with np.errstate(all="ignore"):
        Q = (O - c[None, :]).astype(F)
        a = dot3(D, D)
        b = F(2.0) * dot3(Q, D)
        cc = dot3(Q, Q) - r * r
        disc = b * b - F(4.0) * a * cc
        entered = disc > 0
        sq = np.sqrt(disc)
        a2 = F(2.0) * a
        tn = (-b - sq) / a2
        tf = (-b + sq) / a2
    return entered, tn.astype(F), tf.astype(F)


def trace(nets, parts, center, radius, origins, dirs, max_steps, frame=0, normals=True):
    """The six outputs of nr_compose_trace_rays and its grouping-independent stats."""
    O = np.ascontiguousarray(origins, F).reshape(-1, 3)
    D = np.ascontiguousarray(dirs, F).reshape(-1, 3)
    n = O.shape[0]
    status = np.zeros(n, np.int32)
    steps = np.zeros(n, np.int32)
    t = np.zeros(n, F)
    position = np.zeros((n, 3), F)
    normal = np.zeros((n, 3), F)
    owner = np.full(n, -1, np.int32)
    part_evals = 0
    with np.errstate(all="ignore"):
        entered, tn, tf = intersect(O, D, center, radius)
        tnear = np.where(tn < 0, F(0), tn).astype(F)
        tfar = (tf - tnear).astype(F)
        P = (O + D * tnear[:, None]).astype(F)
        travel = np.zeros(n, F)
        live = entered.copy()
        for it in range(max_steps):
            idx = np.flatnonzero(live)
            if idx.size == 0:
                break
            ts, own, pairs = field(nets, parts, P[idx], frame)
            part_evals += pairs
            tfar[idx] = tfar[idx] - ts
            esc = tfar[idx] <= 0
            go = idx[~esc]
            tg = ts[~esc]
            P[go] = P[go] + D[go] * tg[:, None]
            travel[go] = travel[go] + tg
            cv = tg < MARCHING_EPSILON
            conv = go[cv]
            status[idx[esc]] = ESCAPED
            status[conv] = HIT if it + 1 < max_steps else LIMIT
            if it + 1 < max_steps:
                owner[conv] = own[~esc][cv]
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
                c = TET[q][None, :] * field(nets, parts, pq, frame)[0][:, None]
                acc = c if acc is None else acc + c
            normal[hit] = normalize3(acc)
    out = {"status": status, "steps": steps, "t": t, "position": position}
    if normals:
        out["normal"] = normal
    out["part"] = owner
    stats = {"ray_steps": int(steps.sum()), "shade_evals": 4 * int(hit.size) if normals else 0,
             "rays_hit": int(entered.sum()), "rays_shaded": int(hit.size), "iterations": int(steps.max()) if n else 0,
             "part_evals": int(part_evals)}
    return out, stats
