"""Time of nr_project_points on --n device-resident points (default 2^20, uniform in [-1, 1]^3) of
plane_1 with the default options (iso 0, tol 1e-5, max_step 0.25, max_iters 32), in one process,
alternating with
  * nr_mlp_gradient (value + grad) on the same points: k_grad's own rate of evaluations, and
  * the same projection done by hand on device tensors: one mlp_gradient_device call plus the
    element-wise Newton step in torch per iteration, every point carried for max_iters + 1 evaluations.
Every call runs on torch's current stream between two torch.cuda events; median, min and max of --reps
after --warmup.  The evaluations are the call's own count (stats.ray_steps).  One pass with the default
grid, then one per nr_set_occupancy value (workgroups per CU of the projection's grid).
Runs on the GPU box: python3 tools/project_bench.py > profiles/project_bench.txt"""
import argparse
import os
import sys

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402

ISO, TOL, MAX_STEP, MAX_ITERS = 0.0, 1e-5, 0.25, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-by-hand", action="store_true", help="skip the torch loop (A/B runs of the fused call)")
    args = ap.parse_args()
    n = args.n
    dev = torch.device("cuda:0")
    torch.cuda.init()
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    f32 = dict(dtype=torch.float32, device=dev)
    pts = (torch.rand((n, 3), generator=gen, **f32) * 2 - 1).contiguous()
    pos = torch.zeros((n, 3), **f32)
    val = torch.zeros(n, **f32)
    nrm = torch.zeros((n, 3), **f32)
    dist = torch.zeros(n, **f32)
    iters = torch.zeros(n, dtype=torch.int32, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    gval = torch.zeros(n, **f32)
    grad = torch.zeros((n, 3), **f32)
    torch.cuda.synchronize()

    r = nr.Renderer(0)
    r.load_h5(nr.geometry_path("plane_1")).set_precision("fp32")
    stream = torch.cuda.current_stream(dev)
    r.set_stream(stream.cuda_stream)

    def fused(with_stats=False):
        return r.project_points_device(pts.data_ptr(), n, ISO, TOL, MAX_STEP, MAX_ITERS, pos.data_ptr(), val.data_ptr(),
                                       nrm.data_ptr(), dist.data_ptr(), iters.data_ptr(), status.data_ptr(),
                                       with_stats=with_stats)

    def gradient():
        r.mlp_gradient_device(pts.data_ptr(), n, gval.data_ptr(), grad.data_ptr())

    hand = {}

    def by_hand():
        p = pts.clone()
        for it in range(MAX_ITERS + 1):
            r.mlp_gradient_device(p.data_ptr(), n, gval.data_ptr(), grad.data_ptr())
            if it == MAX_ITERS:
                break
            res = gval - ISO
            gg = (grad * grad).sum(1)
            t = res / gg
            m = res.abs() / gg.sqrt()
            t = torch.where(m > MAX_STEP, t * (MAX_STEP / m), t)
            go = (res.abs() > TOL) & (gg > 0)
            p = torch.where(go[:, None], p - grad * t[:, None], p)
        hand["p"] = p

    runs = {"nr_project_points": fused, "nr_mlp_gradient, value + grad": gradient}
    if not args.no_by_hand:
        runs["by hand: gradient call + torch step"] = by_hand
    rows = {}
    for bpc in (0, 1, 2, 4, 12):  # workgroups per CU: the default, then nr_set_occupancy
        r.set_occupancy(bpc)
        ms = {k: [] for k in runs}
        for i in range(args.warmup + args.reps):
            for k, fn in runs.items():  # alternating
                if bpc != 0 and fn is by_hand:
                    continue
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if i >= args.warmup:
                    ms[k].append(e0.elapsed_time(e1))
        rows[bpc] = ms
    r.set_occupancy(0)
    st = fused(with_stats=True)
    r.synchronize()
    torch.cuda.synchronize()
    evals = st["ray_steps"]
    it_np = iters.cpu().numpy()
    st_np = status.cpu().numpy()
    agree = None
    if hand:
        conv = torch.from_numpy(st_np == nr.NR_PROJ_CONVERGED).to(dev)
        diff = (hand["p"][conv] - pos[conv]).abs().max(1).values
        agree = (float(diff.median()), float(diff.quantile(0.99)), float(diff.max()))
    r.close()

    print(f"plane_1, fp32, {n} device-resident points uniform in [-1, 1]^3; iso {ISO}, tol {TOL}, max_step {MAX_STEP}, "
          f"max_iters {MAX_ITERS}; {args.reps} repetitions after {args.warmup} warm-up, alternating; ms = torch.cuda events "
          f"around the call on the shared stream")
    print(f"library: {os.path.relpath(nr.LIB_PATH, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))}")
    print(f"evaluations {evals} ({evals / n:.2f} per point; by hand {(MAX_ITERS + 1) * n}); converged {st['rays_shaded']} "
          f"({st['rays_shaded'] / n:.4f}), largest evaluation count {st['iterations']}; steps median {int(np.median(it_np))}, "
          f"p99 {int(np.percentile(it_np, 99))}; status counts {np.bincount(st_np, minlength=3).tolist()}")
    if agree is not None:
        print("by-hand positions of the converged points, |difference| to the fused call's (torch contracts and orders "
              f"its sums differently): median {agree[0]:.3e}, p99 {agree[1]:.3e}, max {agree[2]:.3e}")
    for bpc, ms in rows.items():
        print(f"-- workgroups per CU: {'default' if bpc == 0 else bpc}")
        gmed = float(np.median(ms["nr_mlp_gradient, value + grad"]))
        grate = n / gmed / 1e3
        fmed = float(np.median(ms["nr_project_points"]))
        for k, v in ms.items():
            if not v:
                continue
            med = float(np.median(v))
            line = f"{k:36s} median {med:8.3f} ms  (min {min(v):8.3f}, max {max(v):8.3f})"
            if k == "nr_project_points":
                line += f"  {evals / med / 1e3:8.1f} Mevals/s = {evals / med / 1e3 / grate:5.3f} x k_grad's rate"
            elif k.startswith("nr_mlp_gradient"):
                line += f"  {grate:8.1f} Mevals/s"
            else:
                line += f"  {(MAX_ITERS + 1) * n / med / 1e3:8.1f} Mevals/s, {med / fmed:5.2f} x the fused call's time"
            print(line)


if __name__ == "__main__":
    main()
