"""Time of a composed scene's geometry buffer (nr_compose_gbuffer) next to the single-network one
(nr_render_gbuffer) and, for a union of two objects, next to the alternative by hand: one
nr_render_gbuffer per object through that object's own camera and a min-depth composite in torch.
Scenes: S3 of tests/test_gpu_compose.py (plane_1, car_1 and a subtracted car_1) and a union of
plane_1 and car_1 side by side; the owner's view looks at the bound's centre from 2.3 radii, so the
bound fills the frame.  All outputs are device buffers; times are the library's own (HIP events
around the launches, ms_total), the composite's are torch events; median of --reps after --warmup,
the three measurements alternating in one process.
Runs on the GPU box: python3 tools/compose_bench.py > profiles/compose_bench.txt"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402

F = np.float32


def rot_xyz(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    X = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Y = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Z = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Z @ Y @ X).astype(F)


def P(x):
    return ctypes.c_void_p(x.data_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--max-steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    W = H = args.size
    n = W * H
    steps = args.max_steps
    dev = torch.device("cuda:0")
    torch.cuda.init()
    buf = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in ("status", "steps", "part")}
    buf["t"] = torch.zeros(n, dtype=torch.float32, device=dev)
    buf["pos"] = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    buf["nrm"] = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    # the by-hand composite's per-object buffers
    obj = [{"status": torch.zeros(n, dtype=torch.int32, device=dev), "t": torch.zeros(n, dtype=torch.float32, device=dev),
            "nrm": torch.zeros((n, 3), dtype=torch.float32, device=dev)} for _ in range(2)]
    torch.cuda.synchronize()

    rends = {}
    for g in ("plane_1", "car_1"):
        r = nr.Renderer(0)
        r.load_h5(nr.geometry_path(g)).set_precision("fp32").set_static(nr.NR_COLOR_FACING, 3).set_scene("tanh")
        rends[g] = r
    owner = nr.Renderer(0)
    L = owner._L
    eye3 = np.eye(3, dtype=F)
    scenes = {
        "S3 (plane_1 + car_1 - car_1)": [
            {"net": 0, "op": "union", "rot": eye3, "pos": (-0.9, 0.0, 0.0), "scale": 1.0},
            {"net": 1, "op": "union", "rot": rot_xyz(0.3, 1.0, -0.2), "pos": (1.0, 0.2, 0.1), "scale": 0.75},
            {"net": 1, "op": "subtract", "rot": rot_xyz(1.2, 0.4, 0.5), "pos": (-0.9, 0.0, 0.0), "scale": 0.6}],
        "union (plane_1 | car_1)": [
            {"net": 0, "op": "union", "rot": eye3, "pos": (-1.1, 0.0, 0.0), "scale": 1.0},
            {"net": 1, "op": "union", "rot": rot_xyz(0.0, 0.7, 0.0), "pos": (1.1, 0.1, 0.0), "scale": 1.0}],
    }
    srcs = [rends["plane_1"], rends["car_1"]]

    print(f"{W}x{H}, max_steps {steps}, fp32, scene tanh; {args.reps} repetitions after {args.warmup} warm-up, alternating; "
          f"ms = ms_total (HIP events around the launches)")
    for name, parts in scenes.items():
        comp = nr.Composition(owner, srcs, parts)
        info = comp.info()
        c, rad = info["center"], float(info["radius"])
        zoom = 2.3 * rad
        iv, nm = nr.camera(0.0, 0.0, zoom)
        iv = iv.copy()
        iv[3], iv[7], iv[11] = c[0], c[1], zoom + c[2]  # the eye: on the bound centre's z axis, looking down -z
        owner.set_view(iv, nm, 0)
        # (b) one object filling the frame the same way
        rends["plane_1"].set_view(*nr.camera(0.0, 0.0, 2.3 * 1.2), 0)
        # (c) each object's camera: the owner's rays in that object's frame, q = R^T (p - pos) / scale
        M = iv.reshape(3, 4)
        local = []
        for p in parts[:2]:
            R = np.asarray(p["rot"], np.float64).reshape(3, 3)
            V = np.zeros((3, 4))
            V[:, :3] = R.T @ M[:, :3]
            V[:, 3] = R.T @ (M[:, 3] - np.asarray(p["pos"], np.float64)) / float(p["scale"])
            local.append(V.astype(F).reshape(12))
        union_only = all(p["op"] == "union" for p in parts) and len(parts) == 2

        def run_compose(st):
            comp._chk(L.nr_compose_gbuffer(comp._c, W, H, steps, P(buf["status"]), P(buf["steps"]), P(buf["t"]), P(buf["pos"]),
                                           P(buf["nrm"]), P(buf["part"]), 1, st))

        def run_single(st):
            r = rends["plane_1"]
            r._chk(L.nr_render_gbuffer(r._ctx, W, H, steps, P(buf["status"]), P(buf["steps"]), P(buf["t"]), P(buf["pos"]),
                                       P(buf["nrm"]), 1, st))

        def run_by_hand():
            """(ms of the two geometry buffers, ms of the composite, ray-steps)"""
            ms, rs = 0.0, 0
            for k, g in enumerate(("plane_1", "car_1")):
                r = rends[g]
                r.set_view(local[k], nm, 0)
                st = nr._lib.NRStats()
                r._chk(L.nr_render_gbuffer(r._ctx, W, H, steps, P(obj[k]["status"]), None, P(obj[k]["t"]), None,
                                           P(obj[k]["nrm"]), 1, ctypes.byref(st)))
                ms += st.ms_total
                rs += st.ray_steps
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            inf = torch.full_like(obj[0]["t"], float("inf"))
            d0 = torch.where(obj[0]["status"] == nr.NR_RAY_HIT, obj[0]["t"] * float(parts[0]["scale"]), inf)
            d1 = torch.where(obj[1]["status"] == nr.NR_RAY_HIT, obj[1]["t"] * float(parts[1]["scale"]), inf)
            first = d0 <= d1
            depth = torch.where(first, d0, d1)
            nrm = torch.where(first[:, None], obj[0]["nrm"], obj[1]["nrm"])
            hit = torch.isfinite(depth)
            e1.record()
            torch.cuda.synchronize()
            run_by_hand.hits = int(hit.sum().item())
            del nrm
            return ms, e0.elapsed_time(e1), rs

        ms = {"a": [], "b": [], "c_gbuf": [], "c_comp": []}
        last = {}
        for i in range(args.warmup + args.reps):
            sa, sb = nr._lib.NRComposeStats(), nr._lib.NRStats()
            run_compose(ctypes.byref(sa))
            run_single(ctypes.byref(sb))
            if union_only:
                g_ms, c_ms, c_rs = run_by_hand()
                rends["plane_1"].set_view(*nr.camera(0.0, 0.0, 2.3 * 1.2), 0)
            if i >= args.warmup:
                ms["a"].append(sa.ms_total)
                ms["b"].append(sb.ms_total)
                if union_only:
                    ms["c_gbuf"].append(g_ms)
                    ms["c_comp"].append(c_ms)
            last = {"a": sa.as_dict(), "b": sb.as_dict(), "c_rs": c_rs if union_only else 0}
        a, b = float(np.median(ms["a"])), float(np.median(ms["b"]))
        sa, sb = last["a"], last["b"]
        print(f"== {name}: bound centre ({c[0]:.4f}, {c[1]:.4f}, {c[2]:.4f}) radius {rad:.4f}, eye at {zoom:.3f}")
        print(f"(a) nr_compose_gbuffer            median {a:7.3f} ms (min {min(ms['a']):7.3f}, max {max(ms['a']):7.3f})  "
              f"ray_steps {sa['ray_steps']}  rays_hit {sa['rays_hit']}  hits {sa['rays_shaded']}  part_evals {sa['part_evals']}  "
              f"part_evals/ray_steps {sa['part_evals'] / max(sa['ray_steps'], 1):.3f}  "
              f"wave_evals {sa['wave_evals']}  wave_skips {sa['wave_skips']}  {a * 1e6 / max(sa['ray_steps'], 1):.3f} ns/ray-step")
        print(f"(b) nr_render_gbuffer, plane_1    median {b:7.3f} ms (min {min(ms['b']):7.3f}, max {max(ms['b']):7.3f})  "
              f"ray_steps {sb['ray_steps']}  rays_hit {sb['rays_hit']}  hits {sb['rays_shaded']}  "
              f"{b * 1e6 / max(sb['ray_steps'], 1):.3f} ns/ray-step")
        print(f"    (a) / (b): time {a / b:.3f}, time per ray-step {(a / max(sa['ray_steps'], 1)) / (b / max(sb['ray_steps'], 1)):.3f}, "
              f"time per part evaluation {(a / max(sa['part_evals'], 1)) / (b / max(sb['ray_steps'], 1)):.3f}")
        if union_only:
            g, cm = float(np.median(ms["c_gbuf"])), float(np.median(ms["c_comp"]))
            print(f"(c) by hand: 2 x nr_render_gbuffer median {g:7.3f} ms + torch composite {cm:7.3f} ms = {g + cm:7.3f} ms  "
                  f"ray_steps {last['c_rs']}  composite hits {run_by_hand.hits}")
            print(f"    (a) / (c): {a / (g + cm):.3f}  (geometry buffers alone: {a / g:.3f})")
        comp.close()
    owner.close()
    for r in rends.values():
        r.close()


if __name__ == "__main__":
    main()
