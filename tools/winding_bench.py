"""Times nr_mesh_winding on the mesh nr_extract_mesh gives for plane_1 at 256^3 (scene tanh, [-1, 1]^3).

Queries: 2^20 device-resident points of fit_bench's distribution (half uniform in the ball of radius 1.2,
half projected onto the surface by nr_project_points and jittered by 0.03), Morton-sorted in torch outside
the timing -- trimesh_bench.py's "near-surface, Morton-sorted" set, same seed.  Per beta in 2, 3, 4: ms of
the call (winding only, torch.cuda events on the shared stream, median (min, max) of --reps after
--warmup), points per second, the evaluations per point (solid angles and node expansions) from nr_stats,
the largest |w - w_BRUTE| over every 64th point (2^14 of them, spread over the whole set), and the share
of all points whose inside test w >= 0.5 differs from the pseudonormal sign of nr_trimesh_distance.  Next
to them nr_trimesh_distance on the same points, the call with the sdf output (both launches) at beta 2, and NR_TRIMESH_BRUTE on those
2^14 points, its ms scaled by 64 to the whole set.
Runs on the GPU box: python3 tools/winding_bench.py > profiles/winding_bench.txt"""
import argparse
import os
import sys

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402
from trimesh_bench import morton_order, timed  # noqa: E402


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
    m = nr.TriMesh(owner, V, T, leaf=args.leaf)
    info = m.info()
    print(f"plane_1, scene tanh, extract_mesh at {S}^3 over [-1, 1]^3: {info['nv']} vertices, {info['nt']} triangles, "
          f"closed {info['closed']}; hierarchy leaf {args.leaf or 8}: {info['nodes']} nodes, depth {info['depth']}")
    print(f"{n} device-resident points, near-surface (fit_bench), Morton-sorted; ms = torch.cuda events around the call on "
          f"the shared stream, median (min, max) of {args.reps} after {args.warmup} warm-up; evaluations per point from "
          f"nr_stats.shade_evals; brute = NR_TRIMESH_BRUTE on every {n // nb}th point ({nb} points), its ms scaled by {n // nb}; "
          f"max |w - w_brute| over those {nb} points; sign differs = share of the {n} points with (w >= 0.5) != (sdf < 0)")

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
    X = near[morton_order(near, -1.3, 1.3)].contiguous()
    sdf = torch.zeros(n, dtype=torch.float32, device=dev)
    w = torch.zeros(n, dtype=torch.float32, device=dev)
    wb = torch.zeros(nb, dtype=torch.float32, device=dev)
    Xb = X[::n // nb][:nb].contiguous()
    torch.cuda.synchronize()

    head = f"{'call':44s} {'ms':>9s} {'(min, max)':>20s} {'Mpoints/s':>10s} {'evals/pt':>9s}"
    print(head + f" {'max |w - w_brute|':>18s} {'sign differs':>13s}")

    def row(name, fn, st, count, extra=""):
        med, tlo, thi = timed(stream, fn, args.warmup, args.reps)
        print(f"{name:44s} {med:9.3f} {f'({tlo:.3f}, {thi:.3f})':>20s} {count / med / 1e3:10.2f} {st['shade_evals'] / count:9.1f}{extra}")
        return med

    st = m.distance_device(X.data_ptr(), n, sdf.data_ptr(), with_stats=True)
    t_dist = row("nr_trimesh_distance (sdf only)", lambda: m.distance_device(X.data_ptr(), n, sdf.data_ptr()), st, n)
    inside_n = sdf < 0
    bst = m.winding_device(Xb.data_ptr(), nb, wb.data_ptr(), brute=True, with_stats=True)
    for beta in (2.0, 3.0, 4.0):
        st = m.winding_device(X.data_ptr(), n, w.data_ptr(), beta=beta, with_stats=True)
        err = float((w[::n // nb][:nb] - wb).abs().max())
        differs = float(((w >= 0.5) != inside_n).float().mean())
        row(f"nr_mesh_winding beta {beta:g} (winding only)",
            lambda: m.winding_device(X.data_ptr(), n, w.data_ptr(), beta=beta), st, n, f" {err:18.3e} {differs:13.6f}")
    s2 = torch.zeros(n, dtype=torch.float32, device=dev)
    st = m.winding_device(X.data_ptr(), n, w.data_ptr(), s2.data_ptr(), with_stats=True)
    row("nr_mesh_winding beta 2 (winding and sdf)", lambda: m.winding_device(X.data_ptr(), n, w.data_ptr(), s2.data_ptr()), st, n)
    bmed, blo, bhi = timed(stream, lambda: m.winding_device(Xb.data_ptr(), nb, wb.data_ptr(), brute=True), 1, 3)
    print(f"{'NR_TRIMESH_BRUTE (winding only), scaled':44s} {bmed * (n / nb):9.1f} "
          f"{f'({blo * (n / nb):.1f}, {bhi * (n / nb):.1f})':>20s} {nb / bmed / 1e3:10.2f} {bst['shade_evals'] / nb:9.1f}")
    print(f"w_brute over those {nb} points: min {float(wb.min()):.6f}, max {float(wb.max()):.6f}, "
          f"largest distance from 0 or 1 {float(torch.minimum(wb.abs(), (wb - 1).abs()).max()):.3e}; "
          f"nr_trimesh_distance took {t_dist:.3f} ms")
    m.close()
    owner.close()
    src.close()


if __name__ == "__main__":
    main()
