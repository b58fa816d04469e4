"""Time of nr_render_lit next to what it is built on and what it replaces, on the bench frame
(plane_1 1024^2, 128 steps, fp32, facing colour, scene v1, default camera, render_lit's default
light from --light):
  (a) nr_render_lit, frame only and frame + ao + shadow, into device buffers;
  (b) nr_render_gbuffer alone (status, position, normal into device buffers: the call's first pass);
  (c) what a user does today for hard shadows without occlusion: the geometry buffer to the host,
      the shadow rays built in numpy, nr_trace_rays on them, the frame composited in numpy;
  (d) the lighting pass by itself, as nr_render_lit without a frame (geometry buffer + k_light_trace)
      minus (b), for shadows only, occlusion only and both.
ms = the library's own HIP-event time (nr_stats.ms_total); wall = host clock around the call, which
ends in a stream synchronise; (c) has only a wall time.  Medians of --reps after --warmup, all
variants alternating in one process.
Run on an MI355X: python3 tools/light_bench.py > profiles/light_bench.txt"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402

DEFAULTS = dict(shadow_steps=64, shadow_bias=0.01, shadow_k=8.0, ao_step=0.02, ao_strength=2.0, ambient=0.3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--max-steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--camera", type=float, nargs=3, default=(0.0, 0.0, 2.0), metavar=("RX", "RY", "ZOOM"))
    ap.add_argument("--light", type=float, nargs=3, default=(-0.5, 0.7, 0.5), metavar=("X", "Y", "Z"))
    args = ap.parse_args()
    W = H = args.size
    n = W * H
    steps = args.max_steps
    dev = torch.device("cuda:0")
    torch.cuda.init()
    img = torch.zeros(n, dtype=torch.int32, device=dev)
    fbuf = torch.zeros(8 * n, dtype=torch.float32, device=dev)  # ao, shadow | status, position, normal
    torch.cuda.synchronize()

    r = nr.Renderer(0)
    r.load_h5(nr.geometry_path("plane_1")).set_precision("fp32")
    r.set_view(*nr.camera(*args.camera), 0).set_static(nr.NR_COLOR_FACING, 3).set_scene("v1")
    L, ctx = r._L, r._ctx
    vp = ctypes.c_void_p
    out = vp(img.data_ptr())
    fp = fbuf.data_ptr()
    ao, sh = vp(fp), vp(fp + 4 * n)
    g_status, g_pos, g_nrm = vp(fp), vp(fp + 4 * n), vp(fp + 16 * n)
    ldir = np.asarray(args.light, np.float32)

    def lit(o, a, s, **kw):
        lt = r._light(args.light, **dict(DEFAULTS, **kw))

        def run(st):
            r._chk(L.nr_render_lit(ctx, o, W, H, steps, ctypes.byref(lt), a, s, 1, st))
        return run

    def gbuffer(st):
        r._chk(L.nr_render_gbuffer(ctx, W, H, steps, g_status, None, None, g_pos, g_nrm, 1, st))

    def frame(st):
        r._chk(L.nr_render(ctx, out, W, H, steps, 1, st))

    today_counts = {}

    def today(st):
        """(c): hard shadows, no occlusion, through the queries and numpy."""
        g = r.render_gbuffer(W, H, steps)
        base = r.render(W, H, steps, with_stats=False)
        nrm, pos = g["normal"].reshape(-1, 3), g["position"].reshape(-1, 3)
        hit = g["status"].reshape(-1) == nr.NR_RAY_HIT
        dd = (nrm[:, 0] * ldir[0] + nrm[:, 1] * ldir[1]) + nrm[:, 2] * ldir[2]
        ndl = np.where(dd > 0, dd, np.float32(0)).astype(np.float32)
        sel = np.flatnonzero(hit & (ndl > 0))
        o = (pos[sel] + nrm[sel] * np.float32(DEFAULTS["shadow_bias"])).astype(np.float32)
        q, qst = r.trace_rays(o, np.broadcast_to(ldir, o.shape), DEFAULTS["shadow_steps"], normals=False, with_stats=True)
        shadow = np.zeros(n, np.float32)
        shadow[sel[(q["status"] == nr.NR_RAY_ESCAPED) | (q["status"] == nr.NR_RAY_MISS)]] = 1.0
        amb = np.float32(DEFAULTS["ambient"])
        f = amb + (np.float32(1) - amb) * (shadow * ndl)
        b = base.reshape(-1)
        res = b & np.uint32(0xff000000)
        for s8 in (0, 8, 16):
            res |= np.minimum(((b >> np.uint32(s8)) & np.uint32(0xff)).astype(np.float32) * f, 255).astype(np.uint32) << np.uint32(s8)
        today_counts.update(rays=int(sel.size), ray_steps=qst["ray_steps"])
        return res

    runs = {
        "(b) nr_render_gbuffer": gbuffer,
        "    nr_render (the frame alone)": frame,
        "(a) nr_render_lit, frame": lit(out, None, None),
        "(a) nr_render_lit, frame + ao + shadow": lit(out, ao, sh),
        "    nr_render_lit, hard shadows only, frame": lit(out, None, None, shadow_k=0.0, ao_strength=0.0),
        "(d) lit without a frame: shadows only": lit(None, ao, sh, ao_strength=0.0),
        "(d) lit without a frame: occlusion only": lit(None, ao, sh, shadow_steps=0),
        "(d) lit without a frame: both": lit(None, ao, sh),
        "(c) today: gbuffer + numpy + nr_trace_rays": today,
    }
    ms = {k: [] for k in runs}
    wall = {k: [] for k in runs}
    last = {}
    for i in range(args.warmup + args.reps):
        for k, fn in runs.items():  # alternating
            st = nr._lib.NRStats()
            r.synchronize()
            t0 = time.perf_counter()
            fn(ctypes.byref(st))  # with stats the call returns after a stream synchronise
            dt = (time.perf_counter() - t0) * 1e3
            if i >= args.warmup:
                ms[k].append(st.ms_total)
                wall[k].append(dt)
            last[k] = st.as_dict()
    r.close()

    print(f"plane_1 {W}x{H}, max_steps {steps}, fp32, facing colour, scene v1, camera {tuple(args.camera)}, light "
          f"{tuple(args.light)} with {DEFAULTS}; {args.reps} repetitions after {args.warmup} warm-up, alternating")
    print("ms = nr_stats.ms_total (HIP events), wall = host clock around the synchronising call")
    med = {k: float(np.median(v)) for k, v in ms.items()}
    wmed = {k: float(np.median(v)) for k, v in wall.items()}
    for k, v in ms.items():
        st = last[k]
        if k.startswith("(c)"):
            print(f"{k:44s} wall median {wmed[k]:9.3f} (min {min(wall[k]):9.3f}, max {max(wall[k]):9.3f})  shadow rays "
                  f"{today_counts['rays']}  their ray_steps {today_counts['ray_steps']}")
            continue
        print(f"{k:44s} ms median {med[k]:7.3f} (min {min(v):7.3f}, max {max(v):7.3f})  wall median {wmed[k]:7.3f}  "
              f"ray_steps {st['ray_steps']:10d}  shade_evals {st['shade_evals']:8d}  rays_shaded {st['rays_shaded']:7d}  "
              f"iterations {st['iterations']:4d}  launches {st['launches']}")
    gb, a = "(b) nr_render_gbuffer", "(a) nr_render_lit, frame"
    spread = (max(ms[gb]) - min(ms[gb])) / med[gb]
    print(f"-- ratios of medians: (a) / (b) = {med[a] / med[gb]:.3f} (ms; (b)'s spread (max - min) / median = {spread:.3f}), "
          f"(a) / nr_render = {med[a] / med['    nr_render (the frame alone)']:.3f}")
    hard = "    nr_render_lit, hard shadows only, frame"
    c = "(c) today: gbuffer + numpy + nr_trace_rays"
    print(f"-- (c) / hard-shadow nr_render_lit, wall: {wmed[c] / wmed[hard]:.1f} x; (c) / (a), wall: {wmed[c] / wmed[a]:.1f} x")
    print("-- (d) the lighting pass = lit without a frame - (b), differences of ms medians:")
    gsteps = last[gb]["ray_steps"]
    for k in runs:
        if k.startswith("(d)"):
            d = med[k] - med[gb]
            ssteps = last[k]["ray_steps"] - gsteps
            evals = last[k]["shade_evals"] - last[gb]["shade_evals"]
            rate = f"{ssteps / d / 1e3:8.1f} Mray-steps/s" if ssteps else "       -"
            print(f"{k:44s} {d:7.3f} ms  shadow ray_steps {ssteps:9d}  occlusion evals {evals:8d}  {rate}")


if __name__ == "__main__":
    main()
