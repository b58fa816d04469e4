"""Reference for nr_project_points: a helper, not a test.

The numpy restatement of the loop in include/neural_render.h on top of grad_ref.gradient (value and
gradient bit for bit as nr_mlp_gradient), vectorised over the points that are still live, with every
operation of the step rounded to f32 on its own (np.float32 arrays: one rounding per operation, no
contraction).  tests/test_project_cpu.py pins the returned values against OracleNet.forward.
"""
import numpy as np

import grad_ref
from query_ref import dot3, normalize3

F = np.float32
CONVERGED, LIMIT, FLAT = 0, 1, 2
KEYS = ("position", "value", "normal", "distance", "iters", "status")


def project(K, B, X, iso=0.0, tol=1e-5, max_step=0.25, max_iters=32):
    """The six outputs of nr_project_points for the points X [n, 3 or 4], as a dict."""
    X = np.ascontiguousarray(X, F)
    n, cols = X.shape
    iso, tol, max_step = F(iso), F(tol), F(max_step)
    P = X[:, :3].copy()
    W = X[:, 3:]  # the 4th input, constant ([n, 0] for a 3-input network)
    value = np.zeros(n, F)
    grad = np.zeros((n, 3), F)
    iters = np.zeros(n, np.int32)
    status = np.full(n, -1, np.int32)
    neg = np.zeros(n, bool)
    live = np.arange(n)
    with np.errstate(all="ignore"):
        for it in range(max_iters + 1):
            if live.size == 0:
                break
            v, g, _ = grad_ref.gradient(K, B, np.concatenate([P[live], W[live]], 1))
            g = g[:, :3]
            r = (v - iso).astype(F)
            if it == 0:
                neg[live] = r < 0
            st = np.full(live.size, -1, np.int32)
            st[np.abs(r) <= tol] = CONVERGED
            if it == max_iters:
                st[st < 0] = LIMIT
            gg = dot3(g, g)
            st[(st < 0) & ~(gg > 0)] = FLAT
            done = st >= 0
            d = live[done]
            value[d], grad[d], iters[d], status[d] = v[done], g[done], it, st[done]
            go = ~done
            r, g, gg = r[go], g[go], gg[go]
            t = (r / gg).astype(F)
            if max_step > 0:
                m = (np.abs(r) / np.sqrt(gg)).astype(F)
                t = np.where(m > max_step, (t * (max_step / m).astype(F)).astype(F), t)
            live = live[go]
            P[live] = (P[live] - (g * t[:, None]).astype(F)).astype(F)
        assert live.size == 0
        delta = (P - X[:, :3]).astype(F)
        dist = np.sqrt(dot3(delta, delta)).astype(F)
        return {"position": P, "value": value, "normal": normalize3(grad), "distance": np.where(neg, -dist, dist).astype(F),
                "iters": iters, "status": status}


def stats(out):
    """The counters nr_project_points reports for these outputs."""
    n = out["iters"].size
    return {"ray_steps": int((out["iters"].astype(np.int64) + 1).sum()), "rays_shaded": int((out["status"] == CONVERGED).sum()),
            "iterations": int(out["iters"].max()) + 1 if n else 0}
