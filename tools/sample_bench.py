"""Times the fitting-sample stage (nr_mesh_sample, nr_points_order, nr_mesh_fit_samples) on the mesh
nr_extract_mesh gives for plane_1 at --size^3 (scene tanh, [-1, 1]^3).

 1. nr_mesh_fit_samples at --points samples (half on the surface at sigma 0.03, half in the box
    [-1.3, 1.3]^3), both signs, against the torch route of tools/fit_mesh.py on the same mesh: ball points,
    a Morton argsort, a closest-point query of n / 2 points, jitter, cat, a second Morton argsort, the
    signed-distance query of n points, randperm and two gathers.
 2. nr_points_order (Morton) at 2^20, 2^21 and 2^24 points against torch.argsort(stable=True) of the same
    keys computed in torch (the key computation inside both timings).
 3. nr_trimesh_distance on 2^20 shuffled samples against nr_points_order + the same query on `sorted`.
 4. k_mesh_sample alone (nr_mesh_sample, points only): Msamples/s and the bytes it moves per second
    (12 written per sample; the table and the records are read through the caches).
Every ms: torch.cuda events around the call on the shared stream, median (min, max) of --reps after
--warmup.  Runs on the GPU box: python3 tools/sample_bench.py > profiles/sample_bench.txt"""
import argparse
import os
import sys

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402
from trimesh_bench import morton_order, timed  # noqa: E402

LO, HI = -1.3, 1.3


def fmt(t):
    return f"{t[0]:9.3f} ({t[1]:.3f}, {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--points", type=int, default=1 << 21)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    n, S = args.points, args.size
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
    src.close()
    owner = nr.Renderer(0)
    owner.set_stream(stream.cuda_stream)
    m = nr.TriMesh(owner, V, T)
    info = m.info()
    print(f"plane_1, scene tanh, extract_mesh at {S}^3 over [-1, 1]^3: {info['nv']} vertices, {info['nt']} triangles, closed "
          f"{info['closed']}; ms = torch.cuda events around the call on the shared stream, median (min, max) of {args.reps} after "
          f"{args.warmup} warm-up")

    # ---- 1. the fused call against the torch route
    X = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    Y = torch.zeros(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def torch_route(sign):
        d = torch.randn((n // 2, 3), generator=gen, device=dev)
        u = torch.rand((n // 2, 1), generator=gen, device=dev)
        ball = (d / d.norm(dim=1, keepdim=True) * 1.2 * u.pow(1.0 / 3.0)).float()
        ball = ball[morton_order(ball, LO, HI)].contiguous()
        surf = torch.zeros_like(ball)
        m.distance_device(ball.data_ptr(), n // 2, closest_ptr=surf.data_ptr())
        surf = surf + 0.03 * torch.randn(surf.shape, generator=gen, device=dev)
        x = torch.cat([ball, surf])
        x = x[morton_order(x, LO, HI)].float().contiguous()
        y = torch.zeros(n, dtype=torch.float32, device=dev)
        if sign == "winding":
            m.winding_device(x.data_ptr(), n, sdf_ptr=y.data_ptr())
        else:
            m.distance_device(x.data_ptr(), n, y.data_ptr())
        perm = torch.randperm(n, generator=gen, device=dev)
        return x[perm].contiguous(), y[perm].contiguous()

    print(f"\n1. {n} fitting samples, X [n, 3] and Y [n] left on the device")
    print(f"{'sign':8s} {'nr_mesh_fit_samples ms':>34s} {'torch route (fit_mesh.py) ms':>36s} {'torch / fused':>14s} {'evals/pt':>9s}")
    for sign in ("normal", "winding"):
        st = m.fit_samples_device(X.data_ptr(), Y.data_ptr(), n // 2, n // 2, seed=5, sigma=0.03, lo=LO, hi=HI, sign=sign,
                                  with_stats=True)
        fused = timed(stream, lambda: m.fit_samples_device(X.data_ptr(), Y.data_ptr(), n // 2, n // 2, seed=5, sigma=0.03, lo=LO,
                                                           hi=HI, sign=sign), args.warmup, args.reps)
        route = timed(stream, lambda: torch_route(sign), args.warmup, args.reps)
        print(f"{sign:8s} {fmt(fused):>34s} {fmt(route):>36s} {route[0] / fused[0]:14.2f} {st['shade_evals'] / n:9.1f}")
        print(f"         fused: {st['launches']} launches, {float((Y < 0).float().mean()):.4f} of Y inside, |Y| < 0.1 at "
              f"{float((Y.abs() < 0.1).float().mean()):.3f}")

    # ---- 2. the order alone
    print("\n2. Morton order of uniform points of the box: nr_points_order (perm only) against torch.argsort(stable=True) of the "
          "same keys, key computation included in both")
    print(f"{'points':>10s} {'nr_points_order ms':>34s} {'torch ms':>34s} {'nr / torch':>11s} {'Mkeys/s':>9s}")

    def torch_order(x):
        q = ((x - LO) / (HI - LO) * 1023.0).clamp(0, 1023).to(torch.int64)

        def spread(v):
            v = (v | (v << 16)) & 0x030000FF
            v = (v | (v << 8)) & 0x0300F00F
            v = (v | (v << 4)) & 0x030C30C3
            return (v | (v << 2)) & 0x09249249

        return torch.argsort(spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2), stable=True)

    for k in (20, 21, 24):
        nk = 1 << k
        x = ((torch.rand((nk, 3), generator=gen, device=dev) * 2 - 1) * 1.3).float().contiguous()
        perm = torch.zeros(nk, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        mine = timed(stream, lambda: owner.order_points_device(x.data_ptr(), nk, perm.data_ptr(), lo=LO, hi=HI), args.warmup, args.reps)
        theirs = timed(stream, lambda: torch_order(x), args.warmup, args.reps)
        print(f"{'2^' + str(k):>10s} {fmt(mine):>34s} {fmt(theirs):>34s} {mine[0] / theirs[0]:11.2f} {nk / mine[0] / 1e3:9.1f}")
        del x, perm

    # ---- 3. what ordering buys the query
    nq = 1 << 20
    P = torch.zeros((nq, 3), dtype=torch.float32, device=dev)
    Ps = torch.zeros((nq, 3), dtype=torch.float32, device=dev)
    perm = torch.zeros(nq, dtype=torch.int32, device=dev)
    sdf = torch.zeros(nq, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    m.sample_device(P.data_ptr(), nq // 2, nq // 2, seed=5, sigma=0.03, lo=LO, hi=HI)
    owner.order_points_device(P.data_ptr(), nq, perm.data_ptr(), mode="shuffle", seed=5, sorted_ptr=Ps.data_ptr())
    owner.synchronize()
    P.copy_(Ps)  # the samples, shuffled
    torch.cuda.synchronize()
    s0 = m.distance_device(P.data_ptr(), nq, sdf.data_ptr(), with_stats=True)
    plain = timed(stream, lambda: m.distance_device(P.data_ptr(), nq, sdf.data_ptr()), args.warmup, args.reps)

    def ordered():
        owner.order_points_device(P.data_ptr(), nq, perm.data_ptr(), lo=LO, hi=HI, sorted_ptr=Ps.data_ptr())
        m.distance_device(Ps.data_ptr(), nq, sdf.data_ptr())

    both = timed(stream, ordered, args.warmup, args.reps)
    s1 = m.distance_device(Ps.data_ptr(), nq, sdf.data_ptr(), with_stats=True)
    alone = timed(stream, lambda: m.distance_device(Ps.data_ptr(), nq, sdf.data_ptr()), args.warmup, args.reps)
    print(f"\n3. nr_trimesh_distance on 2^20 samples (half surface at sigma 0.03, half box), sdf only")
    print(f"   shuffled:                                {fmt(plain)} ms, {s0['shade_evals'] / nq:.1f} evaluations per point")
    print(f"   nr_points_order (Morton, sorted) + query: {fmt(both)} ms, {s1['shade_evals'] / nq:.1f} evaluations per point "
          f"(the query alone {fmt(alone)} ms): {plain[0] / both[0]:.1f} x")

    # ---- 4. the sampler alone
    print("\n4. nr_mesh_sample, points only (k_mesh_sample, one launch)")
    for label, ns, nv, sigma in (("surface, sigma 0.03", n, 0, 0.03), ("surface, sigma 0", n, 0, 0.0), ("box", 0, n, 0.0),
                                 ("half and half, sigma 0.03", n // 2, n // 2, 0.03)):
        t = timed(stream, lambda: m.sample_device(X.data_ptr(), ns, nv, seed=5, sigma=sigma, lo=LO, hi=HI), args.warmup, args.reps)
        print(f"   {label:28s} {n} samples: {fmt(t)} ms, {n / t[0] / 1e3:9.1f} Msamples/s, {12 * n / t[0] / 1e6:7.1f} GB/s written")
    m.close()
    owner.close()


if __name__ == "__main__":
    main()
