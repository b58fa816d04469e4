"""Time of a composed scene's mesh extraction: nr_compose_extract_mesh against the route by hand
(lattice points built in torch, 12 B a point -> nr_compose_sample -> nr_mesh_grid), the brick-sparse
call against the dense one, and the vertex pass (normals + part) on top.
Scenes: the two of tools/compose_bench.py -- S3 of tests/test_gpu_compose.py (plane_1, car_1 and a
subtracted car_1) and a union of plane_1 and car_1 side by side -- on a cubic lattice over the world
bound (origin = centre - radius, n points an axis): 256^3 dense, 256^3 / 512^3 / 1024^3 sparse with
bricks of 8 and the default band (the brick's diagonal).
All buffers are device buffers with capacities taken from a counting call outside the timed window.
Every time is a host clock around one emitting call (or one route) that ends in a synchronise of the
owner's stream; the routes of one lattice alternate in one process, median of --reps after --warmup.
Runs on the GPU box: python3 tools/compose_mesh_bench.py > profiles/compose_mesh_bench.txt"""
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


def scenes():
    eye3 = np.eye(3, dtype=F)
    return {
        "S3 (plane_1 + car_1 - car_1)": [
            {"net": 0, "op": "union", "rot": eye3, "pos": (-0.9, 0.0, 0.0), "scale": 1.0},
            {"net": 1, "op": "union", "rot": rot_xyz(0.3, 1.0, -0.2), "pos": (1.0, 0.2, 0.1), "scale": 0.75},
            {"net": 1, "op": "subtract", "rot": rot_xyz(1.2, 0.4, 0.5), "pos": (-0.9, 0.0, 0.0), "scale": 0.6}],
        "union (plane_1 | car_1)": [
            {"net": 0, "op": "union", "rot": eye3, "pos": (-1.1, 0.0, 0.0), "scale": 1.0},
            {"net": 1, "op": "union", "rot": rot_xyz(0.0, 0.7, 0.0), "pos": (1.1, 0.1, 0.0), "scale": 1.0}],
    }


def lattice_points(origin, step, n, dev):
    """The lattice points [n^3, 3] in linear-index order, origin + (float)idx * step in f32"""
    ax = [torch.tensor(float(origin[a]), dtype=torch.float32, device=dev) +
          torch.arange(n, dtype=torch.float32, device=dev) * torch.tensor(float(step[a]), dtype=torch.float32, device=dev)
          for a in range(3)]
    z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return torch.stack([x, y, z], -1).reshape(-1, 3).contiguous()


def timed(owner, fn):
    owner.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    owner.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def med(xs):
    return f"median {np.median(xs):9.3f} ms (min {min(xs):9.3f}, max {max(xs):9.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dense", type=int, default=256, help="points an axis of the dense lattice")
    ap.add_argument("--sparse", type=int, nargs="*", default=[256, 512, 1024], help="points an axis of the sparse lattices")
    ap.add_argument("--brick", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.init()
    rends = {}
    for g in ("plane_1", "car_1"):
        r = nr.Renderer(0)
        r.load_h5(nr.geometry_path(g)).set_precision("fp32").set_static(nr.NR_COLOR_FACING, 3).set_scene("tanh")
        rends[g] = r
    owner = nr.Renderer(0)
    owner.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    L = owner._L
    print(f"fp32, iso 0, bricks of {args.brick}, default band; {args.reps} repetitions after {args.warmup} warm-up, the routes of "
          f"a lattice alternating; ms = host clock around one emitting call (or route) ending in a stream synchronise")
    for name, parts in scenes().items():
        comp = nr.Composition(owner, [rends["plane_1"], rends["car_1"]], parts)
        info = comp.info()
        c, rad = info["center"].astype(np.float64), float(info["radius"])
        print(f"== {name}: bound centre ({c[0]:.4f}, {c[1]:.4f}, {c[2]:.4f}) radius {rad:.4f}")
        for n in sorted(set([args.dense] + list(args.sparse))):
            origin = (c - rad).astype(F)
            step = np.full(3, 2.0 * rad / (n - 1), F)
            dims = (n, n, n)
            dense = n == args.dense
            # capacities: one counting call (the sparse and the dense mesh are the same when the band is sound;
            # the larger of the two counts is taken)
            nv, nt, na, sst = comp.extract_mesh_sparse_device(origin, step, dims, None, 0, None, 0, brick=args.brick, with_stats=True)
            if dense:
                dv, dt = comp.extract_mesh_device(origin, step, dims, None, 0, None, 0)
                sound = (dv, dt) == (nv, nt)
                nv, nt = max(nv, dv), max(nt, dt)
            V = torch.zeros((nv, 3), dtype=torch.float32, device=dev)
            N = torch.zeros((nv, 3), dtype=torch.float32, device=dev)
            Pt = torch.zeros((nv,), dtype=torch.int32, device=dev)
            T = torch.zeros((nt, 3), dtype=torch.int32, device=dev)
            routes = {}
            if dense:
                vals = torch.zeros(n ** 3, dtype=torch.float32, device=dev)
                o, s, d = nr.renderer._lattice(origin, step, dims)
                cv, ct = ctypes.c_long(0), ctypes.c_long(0)

                def by_hand(points=None):
                    P = lattice_points(origin, step, n, dev) if points is None else points
                    comp._chk(L.nr_compose_sample(comp._c, ctypes.c_void_p(P.data_ptr()), n ** 3, ctypes.c_void_p(vals.data_ptr()),
                                                  None, 1, None))
                    owner._chk(L.nr_mesh_grid(owner._ctx, ctypes.c_void_p(vals.data_ptr()), nr.renderer._fptr(o), nr.renderer._fptr(s),
                                              d, 0.0, ctypes.c_void_p(V.data_ptr()), nv, ctypes.c_void_p(T.data_ptr()), nt,
                                              ctypes.byref(cv), ctypes.byref(ct), 1))

                pts = lattice_points(origin, step, n, dev)
                routes["dense  nr_compose_extract_mesh              "] = lambda: comp.extract_mesh_device(
                    origin, step, dims, V.data_ptr(), nv, T.data_ptr(), nt)
                routes["dense  by hand: torch points + sample + mesh"] = lambda: by_hand()
                routes["dense  by hand, the points already built    "] = lambda: by_hand(pts)
                routes["dense  with normals + part                  "] = lambda: comp.extract_mesh_device(
                    origin, step, dims, V.data_ptr(), nv, T.data_ptr(), nt, normals_ptr=N.data_ptr(), part_ptr=Pt.data_ptr())
            routes["sparse nr_compose_extract_mesh_sparse       "] = lambda: comp.extract_mesh_sparse_device(
                origin, step, dims, V.data_ptr(), nv, T.data_ptr(), nt, brick=args.brick)
            routes["sparse with normals + part                  "] = lambda: comp.extract_mesh_sparse_device(
                origin, step, dims, V.data_ptr(), nv, T.data_ptr(), nt, brick=args.brick, normals_ptr=N.data_ptr(),
                part_ptr=Pt.data_ptr())
            same = None
            if dense:
                # faster and different is not faster: the two routes give the same bytes
                comp.extract_mesh_device(origin, step, dims, V.data_ptr(), nv, T.data_ptr(), nt)
                owner.synchronize()
                fv, ft = V.clone(), T.clone()
                V.zero_()
                T.zero_()
                by_hand()
                owner.synchronize()
                same = bool(torch.equal(fv.view(torch.int32), V.view(torch.int32)) and torch.equal(ft, T))
                del fv, ft
            ms = {k: [] for k in routes}
            for i in range(args.warmup + args.reps):
                for k, fn in routes.items():
                    t = timed(owner, fn)
                    if i >= args.warmup:
                        ms[k].append(t)
            nb = (n - 1 + args.brick - 1) // args.brick
            print(f"-- {n}^3 = {n ** 3} points, step {float(step[0]):.6f}: {nv} vertices, {nt} triangles; {na} of {nb ** 3} bricks "
                  f"active, {sst['ray_steps']} points evaluated by the sparse samplers ({sst['ray_steps'] / n ** 3:.4f} of the "
                  f"lattice), part_evals {sst['part_evals']}" + (f"; sparse counts == dense counts: {sound}; fused bytes == by-hand bytes: {same}" if dense else ""))
            for k, v in ms.items():
                print(f"   {k} {med(v)}")
            keys = list(ms)
            if dense:
                a, b, b2, cn = (float(np.median(ms[k])) for k in keys[:4])
                sp, spn = (float(np.median(ms[k])) for k in keys[4:])
                print(f"   fused / by hand: {a / b:.3f} (points already built: {a / b2:.3f}); sparse / dense: {sp / a:.3f}; "
                      f"normals + part add {cn - a:.3f} ms dense, {spn - sp:.3f} ms sparse")
            else:
                sp, spn = (float(np.median(ms[k])) for k in keys)
                print(f"   normals + part add {spn - sp:.3f} ms")
        comp.close()
    owner.set_stream(None, own=True)
    owner.close()
    for r in rends.values():
        r.close()


if __name__ == "__main__":
    main()
