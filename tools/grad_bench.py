"""Time of the analytic gradient next to the forward pass on --n device-resident points (default
2^24, uniform in [-1, 1]^3) of plane_1 in fp32, in one process, alternating: nr_mlp_forward,
nr_mlp_gradient with value + grad, nr_mlp_gradient with the normal only.  Every call runs on torch's
current stream between two torch.cuda events; median, min and max of --reps after --warmup, and the
ratio of the medians to the forward's in the same pass (a finite-difference gradient costs four
forwards: the gradient call has to stay below 4x).  One pass with the default grids, then one per
nr_set_occupancy value (workgroups per CU of both kernels' grids).
Runs on the GPU box: python3 tools/grad_bench.py > profiles/grad_bench.txt"""
import argparse
import os
import sys

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    n = args.n
    dev = torch.device("cuda:0")
    torch.cuda.init()
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    pts = (torch.rand((n, 3), generator=gen, dtype=torch.float32, device=dev) * 2 - 1).contiguous()
    y = torch.zeros(n, dtype=torch.float32, device=dev)
    val = torch.zeros(n, dtype=torch.float32, device=dev)
    grad = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    nrm = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    r = nr.Renderer(0)
    r.load_h5(nr.geometry_path("plane_1")).set_precision("fp32")
    stream = torch.cuda.current_stream(dev)
    r.set_stream(stream.cuda_stream)
    runs = {
        "nr_mlp_forward": lambda: r.mlp_forward_device(pts.data_ptr(), y.data_ptr(), n),
        "nr_mlp_gradient, value + grad": lambda: r.mlp_gradient_device(pts.data_ptr(), n, val.data_ptr(), grad.data_ptr()),
        "nr_mlp_gradient, normal only": lambda: r.mlp_gradient_device(pts.data_ptr(), n, normal_ptr=nrm.data_ptr()),
    }
    rows = {}
    for bpc in (0, 2, 4, 8, 12):  # workgroups per CU: the defaults, then nr_set_occupancy
        r.set_occupancy(bpc)
        ms = {k: [] for k in runs}
        for i in range(args.warmup + args.reps):
            for k, fn in runs.items():  # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if i >= args.warmup:
                    ms[k].append(e0.elapsed_time(e1))
        rows[bpc] = ms
    r.set_occupancy(0)
    for fn in runs.values():
        fn()
    r.synchronize()
    torch.cuda.synchronize()
    same = bool(torch.equal(y.view(torch.int32), val.view(torch.int32)))
    eik = grad.double().norm(dim=1)
    r.close()

    print(f"plane_1, fp32, {n} device-resident points uniform in [-1, 1]^3; {args.reps} repetitions after "
          f"{args.warmup} warm-up, alternating; ms = torch.cuda events around the call on the shared stream")
    print(f"value bits == nr_mlp_forward bits: {same}; |grad| median {float(eik.median()):.4f}, "
          f"mean {float(eik.mean()):.4f}")
    for bpc, ms in rows.items():
        print(f"-- workgroups per CU: {'default' if bpc == 0 else bpc}")
        fwd = float(np.median(ms["nr_mlp_forward"]))
        for k, v in ms.items():
            med = float(np.median(v))
            print(f"{k:32s} median {med:8.3f} ms  (min {min(v):8.3f}, max {max(v):8.3f})  "
                  f"{n / med / 1e3:9.1f} Mpoints/s  {med / fwd:5.2f} x forward")


if __name__ == "__main__":
    main()
