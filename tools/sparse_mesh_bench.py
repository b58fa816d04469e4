"""Time of the brick-sparse extraction (nr_extract_mesh_sparse) against the dense one (nr_extract_mesh,
as it stands) on plane_1 (scene tanh, fp32) over size^3 lattices of [-1, 1]^3: 256^3, 512^3 and
1024^3 against the dense call on the same lattice, 2048^3 (past the dense call's 2^30 points) alone.
Bricks of 8 and 16 cells, the default band (the brick's diagonal) and half of it; normals and keys
on, device buffers.  One process, the calls alternating, each on torch's current stream between two
torch.cuda events; median, min and max of --reps after --warmup.  Per configuration: the active
bricks, the points evaluated (nr_stats.ray_steps) against size^3, the scratch the context holds for
the call (the header's formula) and whether the mesh, sorted by key, is the dense one (vertices and
normals bit for bit, the same set of triangles after rotating each to start at its smallest id).
Runs on the GPU box: python3 tools/sparse_mesh_bench.py > profiles/sparse_mesh_bench.txt"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402


def canonical(T):
    """the triangles rotated to start at their smallest id, as lexicographically sorted rows"""
    T = T.long()
    r = torch.argmin(T, 1)
    ar = torch.arange(len(T), device=T.device)
    T = torch.stack([T[ar, (r + s) % 3] for s in range(3)], 1)
    for col in (2, 1, 0):
        T = T[torch.sort(T[:, col], stable=True).indices]
    return T


def scratch_bytes(S, B, active):
    nb = (S - 1 + B - 1) // B
    per_brick = 4 * nb ** 3 + 4 * (nb + 1) ** 3 + 24 * ((nb ** 3 + 255) // 256)
    stride = ((B + 1) ** 3 + 63) // 64 * 64
    return per_brick + active * (4 + 8 * stride) + 24 * ((active * stride + 255) // 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512, 1024, 2048])
    ap.add_argument("--dense-max", type=int, default=1024, help="largest size the dense call runs at")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.init()
    r = nr.Renderer(0)
    r.load_h5(nr.geometry_path("plane_1")).set_precision("fp32").set_scene("tanh")
    r.set_view(*nr.camera(0.0, 0.0, 2.0), 0)
    stream = torch.cuda.current_stream(dev)
    r.set_stream(stream.cuda_stream)
    L, ctx = r._L, r._ctx

    def P(t):
        return ctypes.c_void_p(t.data_ptr())

    print(f"plane_1, scene tanh, fp32, lattices over [-1, 1]^3; normals and keys on, device buffers; {args.reps} repetitions "
          f"after {args.warmup} warm-up, alternating; ms = torch.cuda events around the call on the shared stream")
    for S in args.sizes:
        n = S ** 3
        origin = np.full(3, -1.0, np.float32)
        step = np.full(3, np.float32(2.0) / np.float32(S - 1), np.float32)
        dims = (ctypes.c_int * 3)(S, S, S)
        fo, fs = nr.renderer._fptr(origin), nr.renderer._fptr(step)
        nv, nt, na = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(0)
        runs, info, dense = {}, {}, None
        if S <= args.dense_max:
            r._chk(L.nr_extract_mesh(ctx, fo, fs, dims, 0.0, None, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt), 1, None))
            dV = torch.zeros((max(nv.value, 1), 3), dtype=torch.float32, device=dev)
            dN = torch.zeros_like(dV)
            dT = torch.zeros((max(nt.value, 1), 3), dtype=torch.int32, device=dev)
            dnv, dnt = nv.value, nt.value

            def run_dense(st, dV=dV, dN=dN, dT=dT, dnv=dnv, dnt=dnt):
                a, b = ctypes.c_long(0), ctypes.c_long(0)
                r._chk(L.nr_extract_mesh(ctx, fo, fs, dims, 0.0, P(dV), P(dN), dnv, P(dT), dnt, ctypes.byref(a), ctypes.byref(b), 1, st))

            run_dense(None)
            r.synchronize()
            dense = (dV[:dnv].view(torch.int32).clone(), dN[:dnv].view(torch.int32).clone(), canonical(dT[:dnt]))
            runs["nr_extract_mesh (dense)"] = run_dense
            info["nr_extract_mesh (dense)"] = (f"{dnv} vertices, {dnt} triangles; {n} points; scratch {8 * n + 24 * ((n + 255) // 256)} B")
        for B in (8, 16):
            diag = float(np.float32(np.sqrt(sum((float(B) * float(x)) ** 2 for x in step))))
            for frac in (1.0, 0.5):
                band = float(np.float32(diag * frac))
                r._chk(L.nr_extract_mesh_sparse(ctx, fo, fs, dims, 0.0, B, band, None, None, None, 0, None, 0, ctypes.byref(nv),
                                                ctypes.byref(nt), ctypes.byref(na), 1, None))
                snv, snt, sna = nv.value, nt.value, na.value
                V = torch.zeros((max(snv, 1), 3), dtype=torch.float32, device=dev)
                N = torch.zeros_like(V)
                K = torch.zeros((max(snv, 1),), dtype=torch.int64, device=dev)
                T = torch.zeros((max(snt, 1), 3), dtype=torch.int32, device=dev)

                def run_sparse(st, B=B, band=band, V=V, N=N, K=K, T=T, snv=snv, snt=snt):
                    a, b, c = ctypes.c_long(0), ctypes.c_long(0), ctypes.c_long(0)
                    r._chk(L.nr_extract_mesh_sparse(ctx, fo, fs, dims, 0.0, B, band, P(V), P(N), P(K), snv, P(T), snt, ctypes.byref(a),
                                                    ctypes.byref(b), ctypes.byref(c), 1, st))

                st = nr._lib.NRStats()
                run_sparse(ctypes.byref(st))
                r.synchronize()
                same = "not compared (no dense call at this size)"
                if dense is not None:
                    same = False
                    if (snv, snt) == (len(dense[0]), len(dense[2])):
                        order = torch.argsort(K[:snv])
                        rank = torch.empty_like(order)
                        rank[order] = torch.arange(snv, device=dev)
                        same = bool(torch.equal(V[:snv].view(torch.int32)[order], dense[0]) and
                                    torch.equal(N[:snv].view(torch.int32)[order], dense[1]) and
                                    torch.equal(canonical(rank[T[:snt].long()]), dense[2]))
                name = f"sparse, brick {B:2d}, band {frac:.1f} diagonal"
                runs[name] = run_sparse
                info[name] = (f"{snv} vertices, {snt} triangles; {sna} active bricks of {((S - 1 + B - 1) // B) ** 3}; "
                              f"{st.ray_steps} points evaluated = {st.ray_steps / n:.4f} n^3; scratch {scratch_bytes(S, B, sna)} B; "
                              f"equals the dense mesh: {same}")
        ms = {k: [] for k in runs}
        for i in range(args.warmup + args.reps):
            for k, fn in runs.items():  # alternating
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn(None)
                e1.record(stream)
                e1.synchronize()
                if i >= args.warmup:
                    ms[k].append(e0.elapsed_time(e1))
        print(f"-- {S}^3 = {n} points, step {float(step[0]):.6g}")
        base = float(np.median(ms["nr_extract_mesh (dense)"])) if dense is not None else None
        for k, v in ms.items():
            med = float(np.median(v))
            ratio = f"  dense / this {base / med:6.2f}" if base is not None else ""
            print(f"{k:36s} median {med:9.3f} ms  (min {min(v):9.3f}, max {max(v):9.3f}){ratio}")
            print(f"{'':36s} {info[k]}")
        del runs, dense
        torch.cuda.empty_cache()
    r.close()


if __name__ == "__main__":
    main()
