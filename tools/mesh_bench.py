"""Time of the volume sampler and the mesh extraction on plane_1 (scene tanh, fp32) over a
--size^3 lattice of [-1, 1]^3 (default 256^3 = 2^24 points), in one process, alternating:
nr_sample_grid, nr_extract_mesh with and without normals (device buffers), and the route without a
sampler: nr_mlp_forward on the same points, device-resident (12 B of input per point, the raw
network output).  Every call runs on torch's current stream between two torch.cuda events; for the
calls that report it, the library's own nr_stats.ms_total (HIP events around its launches) is
printed beside it.  Median, min and max of --reps after --warmup.
Runs on the GPU box: python3 tools/mesh_bench.py > profiles/mesh_bench.txt"""
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
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    S = args.size
    n = S ** 3
    origin = np.full(3, -1.0, np.float32)
    step = np.full(3, np.float32(2.0) / np.float32(S - 1), np.float32)
    dims = (ctypes.c_int * 3)(S, S, S)
    dev = torch.device("cuda:0")
    torch.cuda.init()
    # the lattice as a point list, with the sampler's arithmetic: origin + (float)idx * step
    ax = torch.arange(S, dtype=torch.float32, device=dev) * float(step[0]) + float(origin[0])
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    pts = torch.stack([x, y, z], -1).reshape(n, 3).contiguous()
    raw = torch.zeros(n, dtype=torch.float32, device=dev)
    sdf = torch.zeros(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    r = nr.Renderer(0)
    r.load_h5(nr.geometry_path("plane_1")).set_precision("fp32").set_scene("tanh")
    r.set_view(*nr.camera(0.0, 0.0, 2.0), 0)
    stream = torch.cuda.current_stream(dev)
    r.set_stream(stream.cuda_stream)
    L, ctx = r._L, r._ctx
    fo, fs = nr.renderer._fptr(origin), nr.renderer._fptr(step)

    def P(t):
        return ctypes.c_void_p(t.data_ptr())

    nv, nt = ctypes.c_long(0), ctypes.c_long(0)
    r._chk(L.nr_extract_mesh(ctx, fo, fs, dims, 0.0, None, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt), 1, None))
    V = torch.zeros((max(nv.value, 1), 3), dtype=torch.float32, device=dev)
    N = torch.zeros((max(nv.value, 1), 3), dtype=torch.float32, device=dev)
    T = torch.zeros((max(nt.value, 1), 3), dtype=torch.int32, device=dev)

    def extract(normals, st):
        r._chk(L.nr_extract_mesh(ctx, fo, fs, dims, 0.0, P(V), P(N) if normals else None, nv.value, P(T), nt.value,
                                 ctypes.byref(nv), ctypes.byref(nt), 1, st))

    runs = {
        "nr_sample_grid": lambda st: r._chk(L.nr_sample_grid(ctx, fo, fs, dims, P(sdf), 1, st)),
        "nr_mlp_forward, device points": lambda st: r.mlp_forward_device(pts.data_ptr(), raw.data_ptr(), n),
        "nr_extract_mesh, normals": lambda st: extract(True, st),
        "nr_extract_mesh, no normals": lambda st: extract(False, st),
    }
    rows = {}
    for bpc in (0, 4, 8):  # workgroups per CU: the defaults, then nr_set_occupancy 4 and 8
        r.set_occupancy(bpc)
        ms = {k: [] for k in runs}
        lib_ms = {k: [] for k in runs}
        for i in range(args.warmup + args.reps):
            for k, fn in runs.items():  # alternating
                st = nr._lib.NRStats()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn(ctypes.byref(st))
                e1.record(stream)
                e1.synchronize()
                if i >= args.warmup:
                    ms[k].append(e0.elapsed_time(e1))
                    lib_ms[k].append(st.ms_total)
        rows[bpc] = (ms, lib_ms)
    r.set_occupancy(0)
    # the sampler's values are tanh of the network's output at the same points
    runs["nr_sample_grid"](None)
    runs["nr_mlp_forward, device points"](None)
    r.synchronize()
    torch.cuda.synchronize()
    dmax = float((sdf - torch.tanh(raw.double()).float()).abs().max().item())
    r.close()

    print(f"plane_1, scene tanh, fp32, lattice {S}^3 = {n} points over [-1, 1]^3; mesh {nv.value} vertices, "
          f"{nt.value} triangles; {args.reps} repetitions after {args.warmup} warm-up, alternating; "
          f"ms = torch.cuda events around the call on the shared stream (lib: nr_stats.ms_total)")
    print(f"max |nr_sample_grid - tanh(nr_mlp_forward)| = {dmax:.3g}")
    for bpc, (ms, lib_ms) in rows.items():
        print(f"-- workgroups per CU: {'default' if bpc == 0 else bpc}")
        for k, v in ms.items():
            med = float(np.median(v))
            lib = float(np.median(lib_ms[k]))
            print(f"{k:32s} median {med:8.3f} ms  (min {min(v):8.3f}, max {max(v):8.3f})  "
                  f"{n / med / 1e3:9.1f} Mpoints/s  lib {lib:8.3f} ms")


if __name__ == "__main__":
    main()
