"""Time of nr_render_aa next to the brute-force frames it replaces, on the bench frame (plane_1
1024^2, 128 steps, fp32, facing colour, default camera): nr_render at 1024^2, 2048^2 and 4096^2
(what a user box-filters today for 2x2 and 4x4), nr_render_aa adaptive at S = 2 and 4 with contrast
32 and 254, and FULL at S = 2 -- all into device buffers, in one process, alternating.  ms = the
library's own HIP-event time (nr_stats.ms_total: the base frame's events plus the edge passes');
wall = host clock around the call, which ends in a stream synchronise (it adds the host's read of
the edge count and the launch overheads).  Medians of --reps after --warmup.
Run on an MI355X: python3 tools/aa_bench.py > profiles/aa_bench.txt"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--max-steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--camera", type=float, nargs=3, default=(0.0, 0.0, 2.0), metavar=("RX", "RY", "ZOOM"))
    args = ap.parse_args()
    W = H = args.size
    steps = args.max_steps
    dev = torch.device("cuda:0")
    torch.cuda.init()
    img = torch.zeros(16 * W * H, dtype=torch.int32, device=dev)  # up to the 4 W x 4 H frame
    torch.cuda.synchronize()

    r = nr.Renderer(0)
    r.load_h5(nr.geometry_path("plane_1")).set_precision("fp32")
    r.set_view(*nr.camera(*args.camera), 0).set_static(nr.NR_COLOR_FACING, 3).set_scene("v1")
    L, ctx = r._L, r._ctx
    out = ctypes.c_void_p(img.data_ptr())

    def frame(S):
        def run(st):
            r._chk(L.nr_render(ctx, out, S * W, S * H, steps, 1, st))
            return S * W * S * H
        return run

    def aa(S, mode, contrast):
        def run(st):
            edges = ctypes.c_long(0)
            r._chk(L.nr_render_aa(ctx, out, W, H, S, nr.NR_AA_MODE[mode], contrast, steps, 1, ctypes.byref(edges), st))
            return edges.value
        return run

    runs = {
        "nr_render 1x (base frame)": (1, frame(1)),
        "nr_render 2x2 brute force": (2, frame(2)),
        "nr_render 4x4 brute force": (4, frame(4)),
        "nr_render_aa S=2 adaptive c=32": (2, aa(2, "adaptive", 32)),
        "nr_render_aa S=2 adaptive c=254": (2, aa(2, "adaptive", 254)),
        "nr_render_aa S=4 adaptive c=32": (4, aa(4, "adaptive", 32)),
        "nr_render_aa S=4 adaptive c=254": (4, aa(4, "adaptive", 254)),
        "nr_render_aa S=2 full": (2, aa(2, "full", 32)),
    }
    ms = {k: [] for k in runs}
    wall = {k: [] for k in runs}
    last = {}
    for i in range(args.warmup + args.reps):
        for k, (_, fn) in runs.items():  # alternating
            st = nr._lib.NRStats()
            r.synchronize()
            t0 = time.perf_counter()
            count = fn(ctypes.byref(st))  # with stats the call returns after a stream synchronise
            dt = (time.perf_counter() - t0) * 1e3
            if i >= args.warmup:
                ms[k].append(st.ms_total)
                wall[k].append(dt)
            last[k] = (count, st.as_dict())
    r.close()

    print(f"plane_1 {W}x{H}, max_steps {steps}, fp32, facing colour, scene v1, camera {tuple(args.camera)}; "
          f"{args.reps} repetitions after {args.warmup} warm-up, alternating")
    print("ms = nr_stats.ms_total (HIP events), wall = host clock around the synchronising call; count = pixels "
          "rendered (nr_render) or edge pixels (nr_render_aa)")
    med = {k: float(np.median(v)) for k, v in ms.items()}
    for k, v in ms.items():
        count, st = last[k]
        print(f"{k:34s} ms median {med[k]:8.3f} (min {min(v):8.3f}, max {max(v):8.3f})  wall median "
              f"{float(np.median(wall[k])):8.3f}  count {count:9d}  ray_steps {st['ray_steps']:11d}  "
              f"rays_shaded {st['rays_shaded']:9d}  launches {st['launches']}")
    print("-- ratios of medians (ms): each variant against the brute-force frame of its S, and against the base frame")
    brute = {1: "nr_render 1x (base frame)", 2: "nr_render 2x2 brute force", 4: "nr_render 4x4 brute force"}
    for k, (S, _) in runs.items():
        if k.startswith("nr_render_aa"):
            b = brute[S]
            spread = (max(ms[b]) - min(ms[b])) / med[b]
            print(f"{k:34s} {med[k] / med[b]:6.3f} x the {S}x{S} frame ({med[b] / med[k]:5.2f} x faster; that frame's "
                  f"spread (max - min) / median = {spread:.3f}), {med[k] / med[brute[1]]:6.3f} x the base frame, "
                  f"wall {float(np.median(wall[k])) / float(np.median(wall[b])):6.3f} x")


if __name__ == "__main__":
    main()
