"""Times nr_trimesh_distance on the mesh nr_extract_mesh gives for plane_1 at 256^3 (scene tanh, [-1, 1]^3).

Queries: 2^20 device-resident points in three orders -- the points of a 128 x 128 x 64 lattice over the
box in linear order; uniform random points of the box; and fit_bench's distribution (half uniform in the
ball of radius 1.2, half projected onto the surface by nr_project_points and jittered by 0.03, shuffled)
-- and a Morton-sorted copy of the random and of the near-surface set (sorted in torch, outside the
timing).  Per set: ms of the call (sdf only, torch.cuda events on the shared stream, median (min, max) of
--reps after --warmup), points per second and the point-triangle evaluations per point from nr_stats.
NR_TRIMESH_BRUTE on the first 2^14 points of each set, scaled by 64 to the whole set.  The host's build
time (pseudonormals, hierarchy, upload) is a wall clock around nr_trimesh_create.
Runs on the GPU box: python3 tools/trimesh_bench.py > profiles/trimesh_bench.txt"""
import argparse
import os
import sys
import time

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402


def timed(stream, fn, warmup, reps):
    ms = []
    for i in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), min(ms), max(ms)


def morton_order(x, lo, hi):
    """argsort of the 30-bit Morton codes of points x [n, 3] in the box [lo, hi]"""
    q = ((x - lo) / (hi - lo) * 1023.0).clamp(0, 1023).to(torch.int64)

    def spread(v):
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        return (v | (v << 2)) & 0x09249249

    return torch.argsort(spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--brute-points", type=int, default=1 << 14)
    ap.add_argument("--leaf", type=int, default=0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    n, nb, S = args.points, args.brute_points, args.size
    dev = torch.device("cuda:0")
    torch.cuda.init()
    stream = torch.cuda.current_stream(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)

    src = nr.Renderer(0)
    src.load_h5(nr.geometry_path("plane_1")).set_precision("fp32").set_scene("tanh")
    step = np.float32(2.0) / np.float32(S - 1)
    mesh = src.extract_mesh((-1.0, -1.0, -1.0), (step, step, step), (S, S, S), normals=False)
    V, T = mesh["vertices"], mesh["triangles"]
    src.set_stream(stream.cuda_stream)

    owner = nr.Renderer(0)
    owner.set_stream(stream.cuda_stream)
    builds = []
    for _ in range(3):
        t0 = time.perf_counter()
        m = nr.TriMesh(owner, V, T, leaf=args.leaf)
        builds.append((time.perf_counter() - t0) * 1e3)
        info = m.info()
        m.close()
    m = nr.TriMesh(owner, V, T, leaf=args.leaf)
    print(f"plane_1, scene tanh, extract_mesh at {S}^3 over [-1, 1]^3: {info['nv']} vertices, {info['nt']} triangles, "
          f"closed {info['closed']}; hierarchy leaf {args.leaf or 8}: {info['nodes']} nodes, depth {info['depth']}; "
          f"nr_trimesh_create (host: pseudonormals, hierarchy, upload) {np.median(builds):.1f} ms "
          f"(min {min(builds):.1f}, max {max(builds):.1f}, 3 builds, wall clock)")
    print(f"{n} device-resident points per set; ms = torch.cuda events around the call on the shared stream, sdf only, median "
          f"(min, max) of {args.reps} after {args.warmup} warm-up; evaluations per point from nr_stats.shade_evals; "
          f"brute = NR_TRIMESH_BRUTE on the set's first {nb} points, its ms scaled by {n // nb}")

    # ---- the point sets
    nx = 128
    nz = n // (nx * nx)
    ax = torch.linspace(-1, 1, nx, device=dev)
    az = torch.linspace(-1, 1, max(nz, 1), device=dev)
    z, y, x = torch.meshgrid(az, ax, ax, indexing="ij")
    lattice = torch.stack([x, y, z], -1).reshape(-1, 3)[:n].float().contiguous()
    rand = (torch.rand((n, 3), generator=gen, device=dev) * 2 - 1).float().contiguous()
    d = torch.randn((n // 2, 3), generator=gen, device=dev)
    u = torch.rand((n // 2, 1), generator=gen, device=dev)
    ball = (d / d.norm(dim=1, keepdim=True) * 1.2 * u.pow(1.0 / 3.0)).float().contiguous()
    seeds = ball[torch.randperm(n // 2, generator=gen, device=dev)].contiguous()
    surf = torch.zeros_like(seeds)
    torch.cuda.synchronize()
    src.project_points_device(seeds.data_ptr(), n // 2, position_ptr=surf.data_ptr())
    src.synchronize()
    surf = surf + 0.03 * torch.randn(surf.shape, generator=gen, device=dev)
    near = torch.nan_to_num(torch.cat([ball, surf])[torch.randperm(n, generator=gen, device=dev)]).float().contiguous()
    lo, hi = -1.3, 1.3
    sets = [(f"lattice {nx} x {nx} x {nz}, linear order", lattice), ("uniform random in the box", rand),
            ("near-surface, jittered, shuffled (fit_bench)", near),
            ("uniform random, Morton-sorted", rand[morton_order(rand, lo, hi)].contiguous()),
            ("near-surface, Morton-sorted", near[morton_order(near, lo, hi)].contiguous())]
    sdf = torch.zeros(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    print(f"{'set':46s} {'ms':>9s} {'(min, max)':>20s} {'Mpoints/s':>10s} {'evals/pt':>9s} | {'brute ms (scaled)':>18s} "
          f"{'evals/pt':>9s} {'brute / tree':>12s}")
    for name, X in sets:
        st = m.distance_device(X.data_ptr(), n, sdf.data_ptr(), with_stats=True)
        med, tlo, thi = timed(stream, lambda: m.distance_device(X.data_ptr(), n, sdf.data_ptr()), args.warmup, args.reps)
        bst = m.distance_device(X.data_ptr(), nb, sdf.data_ptr(), brute=True, with_stats=True)
        bmed, _, _ = timed(stream, lambda: m.distance_device(X.data_ptr(), nb, sdf.data_ptr(), brute=True), 1, 3)
        scaled = bmed * (n / nb)
        print(f"{name:46s} {med:9.3f} {f'({tlo:.3f}, {thi:.3f})':>20s} {n / med / 1e3:10.2f} {st['shade_evals'] / n:9.1f} | "
              f"{scaled:18.1f} {bst['shade_evals'] / nb:9.1f} {scaled / med:12.1f}")
    m.close()
    owner.close()
    src.close()


if __name__ == "__main__":
    main()
