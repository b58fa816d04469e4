"""Time of the ray queries next to the frame they correspond to, on the bench frame (plane_1
1024^2, 128 steps, fp32, facing colour, default camera): nr_render_gbuffer with and without
normals against nr_render, all into device buffers, in one process, alternating; and one
2^20-ray nr_trace_rays call on device rays.  Times are the library's own (HIP events around the
launch, nr_stats.ms_total); median of --reps after --warmup.
Runs on the GPU box: python3 tools/query_bench.py > profiles/query_bench.txt"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--max-steps", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    W = H = args.size
    n = W * H
    steps = args.max_steps
    dev = torch.device("cuda:0")
    torch.cuda.init()
    img = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    nsteps = torch.zeros(n, dtype=torch.int32, device=dev)
    t = torch.zeros(n, dtype=torch.float32, device=dev)
    pos = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    nrm = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    # 2^20 rays: origins on the sphere of radius 2, aimed at points of the model's box
    rng = np.random.default_rng(1)
    o = rng.normal(size=(n, 3))
    o = 2.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    d = rng.uniform(-0.5, 0.5, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    to = torch.from_numpy(o.astype(np.float32)).to(dev)
    td = torch.from_numpy(d.astype(np.float32)).to(dev)
    torch.cuda.synchronize()

    r = nr.Renderer(0)
    r.load_h5(nr.geometry_path("plane_1")).set_precision("fp32")
    r.set_view(*nr.camera(0.0, 0.0, 2.0), 0).set_static(nr.NR_COLOR_FACING, 3).set_scene("v1")
    L, ctx = r._L, r._ctx

    def P(x):
        return ctypes.c_void_p(x.data_ptr())

    def gbuffer(normals, st):
        r._chk(L.nr_render_gbuffer(ctx, W, H, steps, P(status), P(nsteps), P(t), P(pos), P(nrm) if normals else None,
                                   1, st))

    def rays(normals, st):
        r._chk(L.nr_trace_rays(ctx, P(to), P(td), n, steps, P(status), P(nsteps), P(t), P(pos),
                               P(nrm) if normals else None, 1, st))

    runs = {
        "nr_render (frame)": lambda st: r._chk(L.nr_render(ctx, P(img), W, H, steps, 1, st)),
        "nr_render_gbuffer, normals": lambda st: gbuffer(True, st),
        "nr_render_gbuffer, no normals": lambda st: gbuffer(False, st),
        "nr_trace_rays 2^20 rays, normals": lambda st: rays(True, st),
        "nr_trace_rays 2^20 rays, no normals": lambda st: rays(False, st),
    }
    rows = {}
    for bpc in (0, 2, 3):  # workgroups per CU: the default, then nr_set_occupancy 2 and 3
        r.set_occupancy(bpc)
        ms = {k: [] for k in runs}
        last = {}
        for i in range(args.warmup + args.reps):
            for k, fn in runs.items():  # alternating
                st = nr._lib.NRStats()
                fn(ctypes.byref(st))
                if i >= args.warmup:
                    ms[k].append(st.ms_total)
                last[k] = st.as_dict()
        rows[bpc] = (ms, last)
    r.set_occupancy(0)
    # the G-buffer's hits are the frame's coloured pixels
    runs["nr_render (frame)"](None)
    gbuffer(True, None)
    r.synchronize()
    same = bool(((status == nr.NR_RAY_HIT) == (img != 0)).all().item())
    r.close()

    print(f"plane_1 {W}x{H}, max_steps {steps}, fp32, facing colour, scene v1, camera (0, 0, 2); "
          f"{args.reps} repetitions after {args.warmup} warm-up, alternating; ms = nr_stats.ms_total (HIP events)")
    print(f"G-buffer HIT mask == frame's coloured pixels: {same}")
    for bpc, (ms, last) in rows.items():
        print(f"-- workgroups per CU: {'default' if bpc == 0 else bpc}")
        for k, v in ms.items():
            med = float(np.median(v))
            st = last[k]
            print(f"{k:38s} median {med:7.3f} ms  (min {min(v):7.3f}, max {max(v):7.3f})  "
                  f"{st['ray_steps'] / med / 1e3:8.1f} Mray-steps/s  ray_steps {st['ray_steps']}  "
                  f"rays_hit {st['rays_hit']}  rays_shaded {st['rays_shaded']}  shade_evals {st['shade_evals']}")


if __name__ == "__main__":
    main()
