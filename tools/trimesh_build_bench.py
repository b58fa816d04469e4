"""Times the creation of a nr_trimesh on the mesh nr_extract_mesh gives for plane_1 at 256^3 (scene tanh,
[-1, 1]^3) and on that mesh's remesh (nr_mesh_remesh at --remesh-size^3), the two meshes alternating in
one session:
    nr_trimesh_create from host arrays (the host build);
    the by-hand route for a mesh that is on the device: D2H of both arrays, then nr_trimesh_create;
    nr_mesh_create_device on the device arrays (the device build).
ms = wall time of the call(s) (time.perf_counter around a call that returns when the mesh is ready; the
device is idle before), median (min, max) of --reps after --warmup; the device build's own event time
(nr_stats.ms_total) beside it.

Then, with the host tree and with the device tree, the queries: the distance of a 128 x 128 x 64 lattice,
the distance of 2^20 Morton-sorted points, the winding number at beta 2 of those points, and the 1024^2
geometry buffer -- ms from torch.cuda events on the shared stream, the two trees alternating, and the
evaluations per point or ray (nr_stats.shade_evals / ray_steps).  Last the preview route: nr_extract_mesh
into device buffers -> from_device -> nr_mesh_render, per stage.
Runs on the GPU box: python3 tools/trimesh_build_bench.py   (writes profiles/trimesh_build_bench.txt)"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NR_DEVICE = 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-size", type=int, default=256, help="the lattice plane_1's mesh is extracted on")
    ap.add_argument("--remesh-size", type=int, default=256, help="the lattice that mesh is remeshed on")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trimesh_build_bench.txt"))
    args = ap.parse_args()
    S = args.mesh_size
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device("cuda:0")
    torch.cuda.init()
    stream = torch.cuda.current_stream(dev)
    L = nr.lib()

    src = nr.Renderer(0)
    src.load_h5(nr.geometry_path("plane_1")).set_precision("fp32").set_scene("tanh")
    src.set_stream(stream.cuda_stream)
    mstep = np.float32(2.0) / np.float32(S - 1)
    lattice = ((-1.0, -1.0, -1.0), (mstep, mstep, mstep), (S, S, S))
    mesh = src.extract_mesh(*lattice, normals=False)
    owner = nr.Renderer(0)
    owner.set_stream(stream.cuda_stream)
    meshes = [("plane_1 at %d^3" % S, mesh["vertices"], mesh["triangles"])]
    with nr.TriMesh(owner, mesh["vertices"], mesh["triangles"]) as m:
        info = m.info()
        lo, hi = info["lo"].astype(np.float64), info["hi"].astype(np.float64)
        R = args.remesh_size
        step = (hi - lo) / (R - 5)
        re = m.remesh(tuple(lo - 2 * step), tuple(step), (R, R, R), source_tri=False)
    meshes.append(("its remesh at %d^3" % R, re["vertices"], re["triangles"]))

    def stat(ms):
        return f"{float(np.median(ms)):9.2f} {f'({min(ms):.2f}, {max(ms):.2f})':>20s}"

    # ---- the build ----
    dbuf = [(torch.from_numpy(V).to(dev), torch.from_numpy(T).to(dev)) for _, V, T in meshes]
    wall = {(k, r): [] for k in range(len(meshes)) for r in ("host", "hand", "device", "device events")}
    launches = {}
    for i in range(args.warmup + args.reps):
        for k, (_, V, T) in enumerate(meshes):
            dV, dT = dbuf[k]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = nr.TriMesh(owner, V, T)
            t1 = time.perf_counter()
            m.close()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            m = nr.TriMesh(owner, dV.cpu().numpy(), dT.cpu().numpy())
            t3 = time.perf_counter()
            m.close()
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            m = nr.TriMesh.from_device(owner, dV.data_ptr(), len(V), dT.data_ptr(), len(T), with_stats=True)
            t5 = time.perf_counter()
            ev = m.build_stats["ms_total"]
            launches[k] = m.build_stats["launches"]
            m.close()
            if i >= args.warmup:
                for r, v in (("host", t1 - t0), ("hand", t3 - t2), ("device", t5 - t4)):
                    wall[(k, r)].append(v * 1e3)
                wall[(k, "device events")].append(ev)
    say(f"{'create':64s} {'ms':>9s} {'(min, max)':>20s}")
    for k, (label, V, T) in enumerate(meshes):
        say(f"{label}: {len(V)} vertices, {len(T)} triangles")
        say(f"{'  nr_trimesh_create, host arrays':64s} {stat(wall[(k, 'host')])}")
        say(f"{'  by hand from device arrays: D2H, nr_trimesh_create':64s} {stat(wall[(k, 'hand')])}")
        say(f"{'  nr_mesh_create_device (%d launches)' % launches[k]:64s} {stat(wall[(k, 'device')])}")
        say(f"{'    of that between its events on the stream':64s} {stat(wall[(k, 'device events')])}")
        say(f"  host build / device build: {np.median(wall[(k, 'host')]) / np.median(wall[(k, 'device')]):.1f} x")
    say()

    # ---- the queries, with either tree ----
    def timed(fns):
        ms = [[] for _ in fns]
        for i in range(args.warmup + args.reps):
            for k, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if i >= args.warmup:
                    ms[k].append(e0.elapsed_time(e1))
        return ms

    n = 1 << 20
    W = H = 1024
    iv, nm = nr.camera(0.0, 0.0, 2.0)
    owner.set_view(iv, nm, 0)
    for k, (label, V, T) in enumerate(meshes):
        dV, dT = dbuf[k]
        mh = nr.TriMesh(owner, V, T)
        md = nr.TriMesh.from_device(owner, dV.data_ptr(), len(V), dT.data_ptr(), len(T))
        ih, idv = mh.info(), md.info()
        say(f"{label}: host tree {ih['nodes']} nodes, depth {ih['depth']}; device tree {idv['nodes']} nodes, depth {idv['depth']}")
        say(f"{'query':40s} {'host tree ms':>12s} {'(min, max)':>20s} {'evals':>8s}   {'device tree ms':>14s} {'(min, max)':>20s} {'evals':>8s}")
        lo, hi = ih["lo"].astype(np.float64), ih["hi"].astype(np.float64)
        dims = (128, 128, 64)
        gstep = (hi - lo) / (np.array(dims) - 5)
        origin = tuple(float(np.float32(x)) for x in lo - 2 * gstep)
        gstep = tuple(float(np.float32(x)) for x in gstep)
        grid = torch.zeros(dims[0] * dims[1] * dims[2], dtype=torch.float32, device=dev)
        g = torch.Generator(device=dev).manual_seed(3)
        mid, half = (lo + hi) / 2, (hi - lo) / 2 * 1.2
        X = (torch.rand((n, 3), generator=g, device=dev, dtype=torch.float32) * 2 - 1) * torch.tensor(half, dtype=torch.float32, device=dev) \
            + torch.tensor(mid, dtype=torch.float32, device=dev)
        Xs, perm = torch.zeros_like(X), torch.zeros(n, dtype=torch.int32, device=dev)
        owner.order_points_device(X.data_ptr(), n, perm.data_ptr(), lo=tuple(mid - half), hi=tuple(mid + half), sorted_ptr=Xs.data_ptr())
        out = torch.zeros(n, dtype=torch.float32, device=dev)
        status, t = torch.zeros(W * H, dtype=torch.int32, device=dev), torch.zeros(W * H, dtype=torch.float32, device=dev)
        tri, normal = torch.zeros(W * H, dtype=torch.int32, device=dev), torch.zeros((W * H, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        calls = [
            ("distance, 128 x 128 x 64 lattice", lambda m, s=False: m.sample_grid_device(grid.data_ptr(), origin, gstep, dims, with_stats=s)),
            ("distance, 2^20 Morton-sorted points", lambda m, s=False: m.distance_device(Xs.data_ptr(), n, out.data_ptr(), with_stats=s)),
            ("winding, beta 2, the same points", lambda m, s=False: m.winding_device(Xs.data_ptr(), n, winding_ptr=out.data_ptr(), beta=2.0, with_stats=s)),
            ("G-buffer, 1024 x 1024", lambda m, s=False: m.gbuffer_device(W, H, status_ptr=status.data_ptr(), t_ptr=t.data_ptr(), tri_ptr=tri.data_ptr(),
                                                                          normal_ptr=normal.data_ptr(), with_stats=s)),
        ]
        for what, call in calls:
            sh, sd = call(mh, True), call(md, True)
            th, td = timed([lambda: call(mh), lambda: call(md)])
            say(f"{what:40s} {stat(th):>33s} {sh['shade_evals'] / sh['ray_steps']:8.1f}   {stat(td):>35s} {sd['shade_evals'] / sd['ray_steps']:8.1f}")
        mh.close()
        md.close()
        say()

    # ---- the preview route: network -> mesh on the device -> tree -> frame ----
    o, s, d = nr.renderer._lattice(*lattice)
    nv, nt = ctypes.c_long(0), ctypes.c_long(0)
    V0 = mesh["vertices"]
    dV = torch.zeros((len(V0), 3), dtype=torch.float32, device=dev)
    dT = torch.zeros((len(mesh["triangles"]), 3), dtype=torch.int32, device=dev)
    frame = torch.zeros(W * H, dtype=torch.int32, device=dev)
    stages = {"extract_mesh into device buffers": [], "from_device": [], "render 1024 x 1024": []}
    for i in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        src._chk(L.nr_extract_mesh(src._ctx, nr.renderer._fptr(o), nr.renderer._fptr(s), d, 0.0, ctypes.c_void_p(dV.data_ptr()), None,
                                   len(dV), ctypes.c_void_p(dT.data_ptr()), len(dT), ctypes.byref(nv), ctypes.byref(nt), NR_DEVICE, None))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        m = nr.TriMesh.from_device(owner, dV.data_ptr(), nv.value, dT.data_ptr(), nt.value)
        t2 = time.perf_counter()
        m.render_device(frame.data_ptr(), W, H)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        m.close()
        if i >= args.warmup:
            for key, v in zip(stages, (t1 - t0, t2 - t1, t3 - t2)):
                stages[key].append(v * 1e3)
    say(f"preview route, plane_1 at {S}^3 ({nv.value} vertices, {nt.value} triangles), wall ms per stage")
    for key, v in stages.items():
        say(f"{'  ' + key:64s} {stat(v)}")
    owner.close()
    src.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
