"""Time of nr_compose_render_lit next to what it is built on and what it replaces, on the two scenes
of tools/compose_bench.py (S3: plane_1, car_1 and a subtracted car_1; a union of plane_1 and car_1
side by side), the owner's view looking at the bound's centre from 2.3 radii, facing colour,
render_lit's default light from --light:
  (a) nr_compose_render_lit, the frame into a device buffer;
  (b) nr_compose_render alone (the frame without light);
  (c) what a user does today for hard shadows without occlusion: gbuffer_device, the shadow rays
      built in torch (origins p + n * bias of the hits that face the light), trace_rays_device on
      them.  It does less than (a): no occlusion, no penumbra, no composite.
ms = the library's own HIP-event time (ms_total); wall = host clock around the call, which ends in a
stream synchronise; (c) is its two library calls' ms plus the torch part between torch events, and a
wall time around all of it.  Medians of --reps after --warmup, the variants alternating in one process.
Run on an MI355X: python3 tools/compose_light_bench.py > profiles/compose_light_bench.txt"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402
from compose_bench import rot_xyz  # noqa: E402

F = np.float32
DEFAULTS = dict(shadow_steps=64, shadow_bias=0.01, shadow_k=8.0, ao_step=0.02, ao_strength=2.0, ambient=0.3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--max-steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    # low and from the side the parts are lined up along, so that one casts on the next
    ap.add_argument("--light", type=float, nargs=3, default=(-0.96, 0.1, 0.26), metavar=("X", "Y", "Z"))
    args = ap.parse_args()
    W = H = args.size
    n = W * H
    steps = args.max_steps
    dev = torch.device("cuda:0")
    torch.cuda.init()
    img = torch.zeros(n, dtype=torch.int32, device=dev)
    part = torch.zeros(n, dtype=torch.int32, device=dev)
    occ = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    rstatus = torch.zeros(n, dtype=torch.int32, device=dev)
    pos = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    nrm = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    ldir = torch.tensor(args.light, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    rends = {}
    for g in ("plane_1", "car_1"):
        r = nr.Renderer(0)
        r.load_h5(nr.geometry_path(g)).set_precision("fp32").set_static(nr.NR_COLOR_FACING, 3).set_scene("tanh")
        rends[g] = r
    owner = nr.Renderer(0)
    owner.set_static(nr.NR_COLOR_FACING, 3)
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

    print(f"{W}x{H}, max_steps {steps}, fp32, facing colour, light {tuple(args.light)} with {DEFAULTS}; {args.reps} repetitions "
          f"after {args.warmup} warm-up, alternating")
    print("ms = ms_total (HIP events around the launches), wall = host clock around the synchronising call")
    for name, parts in scenes.items():
        comp = nr.Composition(owner, srcs, parts)
        info = comp.info()
        c, rad = info["center"], float(info["radius"])
        zoom = 2.3 * rad
        iv, nm = nr.camera(0.0, 0.0, zoom)
        iv = iv.copy()
        iv[3], iv[7], iv[11] = c[0], c[1], zoom + c[2]  # the eye: on the bound centre's z axis, looking down -z
        owner.set_view(iv, nm, 0)
        counts = {}

        def lit():
            return comp.render_lit_device(img.data_ptr(), W, H, args.light, max_steps=steps, with_stats=True, **DEFAULTS)

        def frame():
            st = nr._lib.NRComposeStats()
            comp._chk(comp._L.nr_compose_render(comp._c, ctypes.c_void_p(img.data_ptr()), W, H, steps, None, 1, ctypes.byref(st)))
            return st.as_dict()

        def by_hand():
            """(c): ms of the two library calls + the torch part, and the shadow rays' steps."""
            g = comp.gbuffer_device(W, H, steps, status_ptr=status.data_ptr(), position_ptr=pos.data_ptr(),
                                    normal_ptr=nrm.data_ptr(), with_stats=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ndl = (nrm[:, 0] * ldir[0] + nrm[:, 1] * ldir[1]) + nrm[:, 2] * ldir[2]
            sel = torch.nonzero((status == nr.NR_RAY_HIT) & (ndl > 0)).reshape(-1)
            o = (pos[sel] + nrm[sel] * DEFAULTS["shadow_bias"]).contiguous()
            d = ldir.expand(o.shape).contiguous()
            e1.record()
            torch.cuda.synchronize()  # (the library runs on the owner's stream)
            q = comp.trace_rays_device(o.data_ptr(), d.data_ptr(), int(sel.numel()), DEFAULTS["shadow_steps"],
                                       status_ptr=rstatus.data_ptr(), with_stats=True)
            counts.update(rays=int(sel.numel()), ray_steps=q["ray_steps"], torch_ms=e0.elapsed_time(e1))
            return {"ms_total": g["ms_total"] + q["ms_total"] + e0.elapsed_time(e1)}

        runs = {"(a) nr_compose_render_lit, frame": lit, "(b) nr_compose_render": frame,
                "(c) by hand: gbuffer + torch + trace_rays": by_hand}
        ms = {k: [] for k in runs}
        wall = {k: [] for k in runs}
        last = {}
        for i in range(args.warmup + args.reps):
            for k, fn in runs.items():  # alternating
                owner.synchronize()
                t0 = time.perf_counter()
                st = fn()  # with stats the calls return after a stream synchronise
                dt = (time.perf_counter() - t0) * 1e3
                if i >= args.warmup:
                    ms[k].append(st["ms_total"])
                    wall[k].append(dt)
                last[k] = st
        # what the light did, from one more call with the two maps
        comp.render_lit_device(None, W, H, args.light, max_steps=steps, ao_ptr=pos.data_ptr(), part_ptr=part.data_ptr(),
                               occluder_ptr=occ.data_ptr(), with_stats=True, **DEFAULTS)
        blocked = int((occ >= 0).sum().item())
        cross = int(((occ >= 0) & (occ != part)).sum().item())
        a, b, cc = runs.keys()
        med = {k: float(np.median(v)) for k, v in ms.items()}
        wmed = {k: float(np.median(v)) for k, v in wall.items()}
        sa = last[a]
        print(f"== {name}: bound centre ({c[0]:.4f}, {c[1]:.4f}, {c[2]:.4f}) radius {rad:.4f}, eye at {zoom:.3f}")
        print(f"   hit pixels {sa['rays_shaded']}  shadow rays {counts['rays']}  blocked {blocked}  of them by another part than the "
              f"pixel's (cross-part occlusions) {cross}")
        for k in runs:
            st = last[k]
            extra = (f"  ray_steps {st['ray_steps']}  part_evals {st['part_evals']}  wave_evals {st['wave_evals']}  "
                     f"wave_skips {st['wave_skips']}  launches {st['launches']}") if "ray_steps" in st else (
                     f"  shadow ray_steps {counts['ray_steps']}  torch part {counts['torch_ms']:.3f} ms")
            print(f"{k:42s} ms median {med[k]:7.3f} (min {min(ms[k]):7.3f}, max {max(ms[k]):7.3f})  wall median {wmed[k]:7.3f} "
                  f"(min {min(wall[k]):7.3f}, max {max(wall[k]):7.3f}){extra}")
        skips = sa["wave_skips"] / max(sa["wave_evals"] + sa["wave_skips"], 1)
        spread = (max(ms[b]) - min(ms[b])) / med[b]
        print(f"   (a): wave_skips share {skips:.3f} of (wave, part) pairs; shadow ray_steps {sa['ray_steps'] - last[b]['ray_steps']}")
        print(f"   (a) / (b): ms {med[a] / med[b]:.3f}, wall {wmed[a] / wmed[b]:.3f}  ((b)'s spread (max - min) / median = {spread:.3f})")
        print(f"   (c) / (a): ms {med[cc] / med[a]:.3f}, wall {wmed[cc] / wmed[a]:.3f}  ((c) does less: hard shadows only, no occlusion, "
              f"no composite)")
        comp.close()
    owner.close()
    for r in rends.values():
        r.close()


if __name__ == "__main__":
    main()
