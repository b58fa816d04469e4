"""Times the ray queries of a TriMesh (nr_mesh_gbuffer, nr_mesh_render, nr_mesh_trace_rays) on the mesh
nr_extract_mesh gives for plane_1 at 256^3 (scene tanh, [-1, 1]^3) -- the mesh of trimesh_bench.py.

One view (--view rx ry zoom), --size^2 pixels.  Per row: ms between the library's own HIP events around
its launches (nr_stats.ms_total; no copies), median (min, max) of --reps calls after --warmup, rays per
second and the ray-triangle evaluations per ray from nr_stats.shade_evals.
  * nr_mesh_gbuffer (status, t, tri, position, normal) and nr_mesh_render, flat and smooth normals;
  * nr_render_gbuffer of the source network at the same view, in the same session: the yardstick;
  * the same pixel rays as device arrays through nr_mesh_trace_rays in three orders: 8 x 8 pixel tiles
    (the G-buffer's own order), row-major, and shuffled;
  * shadow rays from the G-buffer's hit points (moved 1e-3 along the normal) towards one light: closest
    hit (t only) against NR_MESH_RAY_ANY;
  * NR_TRIMESH_BRUTE on the first --brute-rays rays in tile order, scaled to the whole frame.
Runs on the GPU box: python3 tools/mesh_ray_bench.py > profiles/mesh_ray_bench.txt"""
import argparse
import os
import sys

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402


def timed(fn, warmup, reps):
    """fn() returns nr_stats as a dict: (median, min, max) of ms_total and the last stats"""
    ms = []
    for i in range(warmup + reps):
        st = fn()
        if i >= warmup:
            ms.append(st["ms_total"])
    return float(np.median(ms)), min(ms), max(ms), st


def pixel_rays(W, H, iv, dev):
    """nr_render's pixel rays in torch (f32), index y W + x"""
    M = torch.tensor(np.asarray(iv, np.float32).reshape(3, 4), device=dev)
    y, x = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    u = x.float() / float(W) * 2 - 1
    v = y.float() / float(H) * 2 - 1
    d = torch.stack([u, v, torch.full_like(u, -2.0)], -1).reshape(-1, 3)
    d = d / d.norm(dim=1, keepdim=True)
    return M[:, 3].expand(W * H, 3).contiguous(), (d @ M[:, :3].T).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-size", type=int, default=256)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--view", type=float, nargs=3, default=(-35.0, 30.0, 2.0))
    ap.add_argument("--brute-rays", type=int, default=1 << 12)
    ap.add_argument("--leaf", type=int, default=0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    W = H = args.size
    n, nb, S = W * H, args.brute_rays, args.mesh_size
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
    iv, nm = nr.camera(*args.view)
    src.set_view(iv, nm, 0)
    owner = nr.Renderer(0)
    owner.set_stream(stream.cuda_stream)
    owner.set_view(iv, nm, 0)
    m = nr.TriMesh(owner, V, T, leaf=args.leaf)
    info = m.info()
    print(f"plane_1, scene tanh, extract_mesh at {S}^3 over [-1, 1]^3: {info['nv']} vertices, {info['nt']} triangles, "
          f"closed {info['closed']}; hierarchy leaf {args.leaf or 8}: {info['nodes']} nodes, depth {info['depth']}")
    print(f"view camera({args.view[0]}, {args.view[1]}, {args.view[2]}), {W} x {H} = {n} rays; ms = nr_stats.ms_total (HIP events around "
          f"the call's launches), median (min, max) of {args.reps} after {args.warmup} warm-up; evaluations per ray from "
          f"nr_stats.shade_evals")

    def row(name, med, lo, hi, rays, evals=None):
        ev = f"{evals / rays:9.1f}" if evals is not None else f"{'-':>9s}"
        print(f"{name:64s} {med:9.3f} {f'({lo:.3f}, {hi:.3f})':>20s} {rays / med / 1e3:10.2f} {ev}")

    print(f"{'call':64s} {'ms':>9s} {'(min, max)':>20s} {'Mrays/s':>10s} {'evals/ray':>9s}")
    # ---- the frame calls, into device buffers
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    tri = torch.zeros(n, dtype=torch.int32, device=dev)
    t = torch.zeros(n, dtype=torch.float32, device=dev)
    pos = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    nrm = torch.zeros((n, 3), dtype=torch.float32, device=dev)
    img = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for smooth in (False, True):
        kind = "smooth" if smooth else "flat"
        med, lo, hi, st = timed(lambda: m.gbuffer_device(W, H, status.data_ptr(), t.data_ptr(), tri.data_ptr(), None, pos.data_ptr(),
                                                         nrm.data_ptr(), smooth=smooth, with_stats=True), args.warmup, args.reps)
        row(f"nr_mesh_gbuffer, {kind} normals (status, t, tri, position, normal)", med, lo, hi, n, st["shade_evals"])
        med, lo, hi, st = timed(lambda: m.render_device(img.data_ptr(), W, H, smooth=smooth, with_stats=True), args.warmup, args.reps)
        row(f"nr_mesh_render, {kind} normals, facing colour", med, lo, hi, n, st["shade_evals"])
    hits = int(st["rays_hit"])
    med, lo, hi, st = timed(lambda: src.render_gbuffer(W, H, 6000, with_stats=True)[1], args.warmup, args.reps)
    row(f"nr_render_gbuffer of the network (fp32, normals): the yardstick", med, lo, hi, n)
    print(f"  (the mesh is hit by {hits} of the {n} pixel rays, the network by {int(st['rays_shaded'])})")

    # ---- the same rays as arrays, in three orders
    m.gbuffer_device(W, H, status.data_ptr(), None, None, None, pos.data_ptr(), nrm.data_ptr())
    owner.synchronize()
    O, D = pixel_rays(W, H, iv, dev)
    idx = torch.arange(n, device=dev).reshape(H // 8, 8, W // 8, 8).permute(0, 2, 1, 3).reshape(-1)
    orders = [("8 x 8 pixel tiles", idx), ("row-major", torch.arange(n, device=dev)),
              ("shuffled", torch.randperm(n, generator=gen, device=dev))]
    for name, p in orders:
        o, d = O[p].contiguous(), D[p].contiguous()
        torch.cuda.synchronize()
        med, lo, hi, st = timed(lambda: m.trace_rays_device(o.data_ptr(), d.data_ptr(), n, status_ptr=status.data_ptr(),
                                                            t_ptr=t.data_ptr(), tri_ptr=tri.data_ptr(), position_ptr=pos.data_ptr(),
                                                            normal_ptr=nrm.data_ptr(), with_stats=True), args.warmup, args.reps)
        row(f"nr_mesh_trace_rays, the pixel rays, {name}", med, lo, hi, n, st["shade_evals"])
        if name == "8 x 8 pixel tiles":
            med, lo, hi, st = timed(lambda: m.trace_rays_device(o.data_ptr(), d.data_ptr(), nb, status_ptr=status.data_ptr(),
                                                                t_ptr=t.data_ptr(), brute=True, with_stats=True), 1, 3)
            scale = n / nb
            row(f"  NR_TRIMESH_BRUTE on the first {nb} of them, ms scaled by {scale:.0f}", med * scale, lo * scale, hi * scale, n,
                st["shade_evals"] * scale)

    # ---- shadow rays from the hit points towards one light
    m.gbuffer_device(W, H, status.data_ptr(), None, None, None, pos.data_ptr(), nrm.data_ptr())
    owner.synchronize()
    light = torch.tensor([0.5, 0.8, 0.6], device=dev)
    light = light / light.norm()
    hit = status == 2
    so = torch.where(hit[:, None], pos + 1e-3 * nrm, torch.zeros_like(pos))[idx].contiguous()
    sd = torch.where(hit[:, None], light.expand(n, 3), torch.zeros_like(pos))[idx].contiguous()  # (a miss casts a dead ray)
    torch.cuda.synchronize()
    med, lo, hi, st = timed(lambda: m.trace_rays_device(so.data_ptr(), sd.data_ptr(), n, status_ptr=status.data_ptr(), t_ptr=t.data_ptr(),
                                                        with_stats=True), args.warmup, args.reps)
    row(f"shadow rays of the {int(hit.sum())} hit pixels, closest hit (status, t)", med, lo, hi, n, st["shade_evals"])
    shadowed = int(st["rays_hit"])
    med, lo, hi, st = timed(lambda: m.trace_rays_device(so.data_ptr(), sd.data_ptr(), n, status_ptr=status.data_ptr(), any_hit=True,
                                                        with_stats=True), args.warmup, args.reps)
    row(f"the same rays, NR_MESH_RAY_ANY (status)", med, lo, hi, n, st["shade_evals"])
    print(f"  ({shadowed} of them are in shadow by closest hit, {int(st['rays_hit'])} by any hit; evaluations per ray over all {n} "
          f"slots, the dead ones included)")
    m.close()
    owner.close()
    src.close()


if __name__ == "__main__":
    main()
