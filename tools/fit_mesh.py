"""OBJ -> samples -> Fit -> load_into -> render, once, printing what it did.

The mesh: an OBJ file (nr.load_obj), or with no argument the mesh nr_extract_mesh gives for plane_1
(scene tanh, --size^3 lattice over [-1, 1]^3).  The samples, fit_bench's recipe with the mesh in the
network's place: --points / 2 points uniform in the ball of radius 1.2 about the mesh (its bound scaled
into the unit ball), as many on the surface -- the closest points nr_trimesh_distance returns for ball
points -- jittered by 0.03; the query runs on a Morton-sorted copy (neighbours in space share a walk) and
the pairs are shuffled afterwards for the fit.  Y = the signed distance, clamp 0.1 -- its sign the
pseudonormal's (--sign normal: nr_trimesh_distance) or the winding number's (--sign winding:
nr_mesh_winding with the sdf output), by default the first for a closed mesh and the second for any
other; --drop-x LO HI removes the triangles whose centroid has LO <= x <= HI first, to make an open mesh
of a closed one.  A [3, 32 x 4, 1]
student, batch 2^16, lr 1e-3, --epochs epochs; then load_into a renderer and a 256^2 frame, whose
silhouette is compared with the mesh's own (TriMesh.gbuffer through the same camera) and, when the
mesh came from a network, with that network's.
--volume-iou N adds a camera-free metric: the IoU of {student < 0} (Renderer.sample_grid, scene tanh) and
{mesh sdf < 0} (TriMesh.sample_grid with the fit's sign) on an N^3 lattice over the box [-1.3, 1.3]^3.
--sampler device replaces the torch recipe by one nr_mesh_fit_samples call: half the points on the surface in
proportion to triangle area at sigma 0.03, half uniform in the box [-1.3, 1.3]^3.
Runs on the GPU box: python3 tools/fit_mesh.py [mesh.obj]"""
import argparse
import os
import sys

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402
from fit_bench import CLAMP, init_net, silhouette  # noqa: E402
from trimesh_bench import morton_order  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("obj", nargs="?")
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--points", type=int, default=1 << 21)
    ap.add_argument("--epochs", type=int, default=400)
    ap.add_argument("--out", help="write the student's frame here (.png)")
    ap.add_argument("--sign", choices=("normal", "winding"), help="default: normal for a closed mesh, winding otherwise")
    ap.add_argument("--sampler", choices=("torch", "device"), default="torch",
                    help="torch: the recipe above (the recorded numbers); device: one nr_mesh_fit_samples call")
    ap.add_argument("--volume-iou", type=int, default=0, metavar="N",
                    help="also the IoU of {student < 0} and {mesh sdf < 0} on an N^3 lattice over [-1.3, 1.3]^3")
    ap.add_argument("--drop-x", type=float, nargs=2, metavar=("LO", "HI"), help="remove the triangles whose centroid has LO <= x <= HI")
    args = ap.parse_args()
    n = args.points
    dev = torch.device("cuda:0")
    torch.cuda.init()
    stream = torch.cuda.current_stream(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)

    source = None
    if args.obj:
        V, T = nr.load_obj(args.obj)
        print(f"{args.obj}: {len(V)} vertices, {len(T)} triangles")
        # into the unit ball, as the bundled networks' shapes are
        mid = (V.min(0) + V.max(0)) / 2
        V = ((V - mid) / np.float32(np.linalg.norm(V - mid, axis=1).max() * 1.05)).astype(np.float32)
    else:
        source = nr.Renderer(0)
        source.load_h5(nr.geometry_path("plane_1")).set_precision("fp32").set_scene("tanh")
        step = np.float32(2.0) / np.float32(args.size - 1)
        mesh = source.extract_mesh((-1.0, -1.0, -1.0), (step, step, step), (args.size,) * 3, normals=False)
        V, T = mesh["vertices"], mesh["triangles"]
        print(f"plane_1 through nr_extract_mesh at {args.size}^3: {len(V)} vertices, {len(T)} triangles")
    if args.drop_x:
        cx = V[T].astype(np.float64).mean(1)[:, 0]
        keep = (cx < args.drop_x[0]) | (cx > args.drop_x[1])
        print(f"--drop-x: {int((~keep).sum())} of {len(T)} triangles with {args.drop_x[0]} <= x <= {args.drop_x[1]} removed")
        T = np.ascontiguousarray(T[keep])
    owner = nr.Renderer(0)
    owner.set_stream(stream.cuda_stream)
    with nr.TriMesh(owner, V, T) as m:
        info = m.info()
        print(f"TriMesh: {info['nodes']} nodes, depth {info['depth']}, closed {info['closed']}")
        sign = args.sign or ("normal" if info["closed"] else "winding")
        if not info["closed"] and not args.sign:
            print("the mesh is not closed: the sign is taken from the winding number (w >= 0.5 is inside), as with --sign winding")
        elif not info["closed"] and sign == "normal":
            print("the mesh is not closed: the pseudonormal sign of the distance means nothing, and so does the fit")
        # the mesh itself through the camera silhouette() renders the networks with
        iv, nm = nr.camera(0.0, 0.0, 2.0)
        owner.set_view(iv, nm, 0)
        gb, gst = m.gbuffer(256, 256, tri=False, position=False, normal=False, with_stats=True)
        sm = gb["status"] == 2  # NR_RAY_HIT
        print(f"mesh at 256^2: {int(sm.sum())} px in {gst['ms_total']:.2f} ms ({gst['shade_evals'] / sm.size:.1f} ray-triangle "
              f"evaluations per pixel)")
        mesh_in = None
        if args.volume_iou >= 2:
            N = args.volume_iou
            vstep = np.float32(2.6) / np.float32(N - 1)
            lattice = ((-1.3, -1.3, -1.3), (vstep, vstep, vstep), (N, N, N))
            vals, vst = m.sample_grid(*lattice, sign=sign, with_stats=True)
            mesh_in = vals < 0
            print(f"mesh on the {N}^3 lattice over [-1.3, 1.3]^3 (sign: {sign}): {int(mesh_in.sum())} points inside, "
                  f"{vst['ms_total']:.2f} ms, {vst['shade_evals'] / vals.size:.1f} evaluations per point")
        if args.sampler == "device":
            # half on the surface in proportion to area, jittered by 0.03, half uniform in the box: drawn, ordered,
            # labelled and shuffled by the library, left on the device
            X = torch.zeros((n, 3), dtype=torch.float32, device=dev)
            Y = torch.zeros(n, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            st1 = m.fit_samples_device(X.data_ptr(), Y.data_ptr(), n // 2, n - n // 2, seed=5, sigma=0.03, lo=-1.3, hi=1.3,
                                       sign=sign, with_stats=True)
        else:
            d = torch.randn((n // 2, 3), generator=gen, device=dev)
            u = torch.rand((n // 2, 1), generator=gen, device=dev)
            ball = (d / d.norm(dim=1, keepdim=True) * 1.2 * u.pow(1.0 / 3.0)).float()
            ball = ball[morton_order(ball, -1.3, 1.3)].contiguous()
            surf = torch.zeros_like(ball)
            torch.cuda.synchronize()
            st0 = m.distance_device(ball.data_ptr(), n // 2, closest_ptr=surf.data_ptr(), with_stats=True)
            surf = surf + 0.03 * torch.randn(surf.shape, generator=gen, device=dev)
            X = torch.cat([ball, surf])
            X = X[morton_order(X, -1.3, 1.3)].float().contiguous()
            Y = torch.zeros(n, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            if sign == "winding":
                st1 = m.winding_device(X.data_ptr(), n, sdf_ptr=Y.data_ptr(), with_stats=True)
            else:
                st1 = m.distance_device(X.data_ptr(), n, Y.data_ptr(), with_stats=True)
    if args.sampler == "device":
        print(f"samples: nr_mesh_fit_samples, {n // 2} surface points (area-weighted, sigma 0.03) and {n - n // 2} in the box "
              f"[-1.3, 1.3]^3: drawn, Morton-ordered, {n} signed distances (sign: {sign}) and shuffled in {st1['ms_total']:.2f} ms "
              f"({st1['shade_evals'] / n:.1f} evaluations per point); "
              f"{float((Y < 0).float().mean()):.4f} of them inside, |Y| < clamp at {float((Y.abs() < CLAMP).float().mean()):.3f}")
    else:
        print(f"samples: {n // 2} ball points -> closest points in {st0['ms_total']:.2f} ms ({st0['shade_evals'] / (n // 2):.1f} "
              f"evaluations per point); {n} signed distances (sign: {sign}) in {st1['ms_total']:.2f} ms ({st1['shade_evals'] / n:.1f} per point); "
              f"{float((Y < 0).float().mean()):.4f} of them inside, |Y| < clamp at {float((Y.abs() < CLAMP).float().mean()):.3f}")
        perm = torch.randperm(n, generator=gen, device=dev)
        X, Y = X[perm].contiguous(), Y[perm].contiguous()

    dims, K, B = init_net(3, 20)
    batch = 1 << 16
    steps = n // batch
    losses = torch.zeros(steps, dtype=torch.float32, device=dev)
    curve = []
    torch.cuda.synchronize()
    with nr.Fit(owner, dims, K, B, lr=1e-3, clamp=CLAMP) as f:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for ep in range(args.epochs):
            f.run_device(X.data_ptr(), Y.data_ptr(), steps * batch, batch, losses.data_ptr())
            curve.append(losses.mean())
        e1.record(stream)
        e1.synchronize()
        student = nr.Renderer(0)
        f.load_into(student)
        step_count = f.weights()[3]
    curve = [float(c) for c in curve]
    floor = float(((Y.clamp(-CLAMP, CLAMP) - Y) ** 2).mean())
    print(f"fit: [3, 32 x 4, 1], batch 2^16, lr 1e-3, clamp {CLAMP}, {args.epochs} epochs = {step_count} steps in "
          f"{e0.elapsed_time(e1):.1f} ms (host loop included); loss of every tenth epoch: "
          + " ".join(f"{c:.3e}" for c in curve[::10]) + f"; last {curve[-1]:.3e}")
    print(f"loss of a student equal to the distance (Y is not clamped): {floor:.3e}")
    ss = silhouette(student)
    if args.out:
        img, _ = student.render(256, 256, 256)
        nr.save_png(args.out, img)
    iou = lambda a, b: float((a & b).sum() / max((a | b).sum(), 1))
    # against the mesh: the student's own zero set (scene tanh, as the mesh was rendered), not silhouette()'s scene
    student.set_scene("tanh")
    sz = student.render(256, 256, 256)[0] != 0
    print(f"silhouette at 256^2, scene tanh: mesh {int(sm.sum())} px, student fitted to it {int(sz.sum())} px, IoU against the mesh "
          f"{iou(sm, sz):.4f}")
    if mesh_in is not None:
        net_in = student.sample_grid(*lattice) < 0
        print(f"volume at {args.volume_iou}^3 over [-1.3, 1.3]^3, scene tanh: mesh {int(mesh_in.sum())} points inside, student "
              f"{int(net_in.sum())}, IoU {iou(mesh_in, net_in):.4f}")
    if source is not None:
        st = silhouette(source)
        print(f"silhouette at 256^2, scene v1: source network {int(st.sum())} px, student fitted to its mesh {int(ss.sum())} px, "
              f"IoU {iou(st, ss):.4f}")
        source.close()
    student.close()
    owner.close()


if __name__ == "__main__":
    main()
