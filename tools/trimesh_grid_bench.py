"""Times a triangle mesh's lattice calls on the mesh nr_extract_mesh gives for plane_1 at 256^3 (scene
tanh, [-1, 1]^3): nr_mesh_sample_grid, nr_mesh_remesh and nr_mesh_remesh_sparse (bricks of 8,
the default band) on a --size^3 lattice over the mesh's bound grown by two cells, for both signs, next to
the by-hand route they replace -- the lattice's points built in torch (12 B a point), nr_points_order
(Morton, with the sorted copy), nr_trimesh_distance or nr_mesh_winding's sdf output on the sorted points,
the values scattered back through the permutation, nr_mesh_grid on the device.

Everything is device-resident and warm; ms = torch.cuda events around the call(s) on the shared stream,
the fused call and the by-hand route alternating inside one loop, median (min, max) of --reps after
--warmup.  The remesh calls are timed with buffers already sized (one call; it reads its counts on the
host in the middle, as nr_extract_mesh does), the by-hand route likewise.  Also: evaluations per point
(nr_stats.shade_evals / ray_steps), active bricks, whether the sparse mesh sorted by key is the dense one,
whether the remesh is closed (nr_trimesh_normals' flag), and the repair demo: the same mesh without the
triangles whose centroid has |x| <= 0.1 (as tools/winding_bench.py's companion run), remeshed with the
winding sign.
Runs on the GPU box: python3 tools/trimesh_grid_bench.py   (writes profiles/trimesh_grid_bench.txt)"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NR_DEVICE = 1


def canonical(T):
    """triangles rotated to start at their smallest index, rows sorted: the list as a set"""
    T = np.asarray(T).reshape(-1, 3)
    r = np.argmin(T, 1)
    R = np.stack([T[np.arange(len(T)), (r + s) % 3] for s in range(3)], -1)
    return R[np.lexsort((R[:, 2], R[:, 1], R[:, 0]))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh-size", type=int, default=256, help="the lattice plane_1's mesh is extracted on")
    ap.add_argument("--size", type=int, default=256, help="the lattice the mesh is sampled on")
    ap.add_argument("--brick", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trimesh_grid_bench.txt"))
    args = ap.parse_args()
    S, N = args.mesh_size, args.size
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
    mstep = np.float32(2.0) / np.float32(S - 1)
    mesh = src.extract_mesh((-1.0, -1.0, -1.0), (mstep, mstep, mstep), (S, S, S), normals=False)
    src.close()
    V, T = mesh["vertices"], mesh["triangles"]
    owner = nr.Renderer(0)
    owner.set_stream(stream.cuda_stream)

    def lattice_of(info):
        lo, hi = info["lo"].astype(np.float64), info["hi"].astype(np.float64)
        step = (hi - lo) / (N - 5)  # two cells of margin on either side
        origin = lo - 2 * step
        return tuple(float(np.float32(x)) for x in origin), tuple(float(np.float32(x)) for x in step), (N, N, N)

    def timed_pair(fused, by_hand):
        """the two routes alternating; (median, min, max) of each"""
        ms = ([], [])
        for i in range(args.warmup + args.reps):
            for k, fn in enumerate((fused, by_hand)):
                if fn is None:
                    continue
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                if i >= args.warmup:
                    ms[k].append(e0.elapsed_time(e1))
        return [(float(np.median(m)), min(m), max(m)) if m else None for m in ms]

    def fmt(t):
        return f"{t[0]:9.2f} {f'({t[1]:.2f}, {t[2]:.2f})':>20s}" if t else f"{'':9s} {'':>20s}"

    def bench(m, label, signs):
        info = m.info()
        origin, step, dims = lattice_of(info)
        n = N * N * N
        say(f"{label}: {info['nv']} vertices, {info['nt']} triangles, closed {info['closed']}; hierarchy {info['nodes']} nodes, "
            f"depth {info['depth']}")
        say(f"lattice {N}^3 = {n} points, origin {origin}, step {step}; brick {args.brick}, band = the brick's diagonal")
        say(f"{'call':58s} {'ms':>9s} {'(min, max)':>20s} {'evals/pt':>9s}  notes")
        o = np.asarray(origin, np.float32)
        s = np.asarray(step, np.float32)
        fo, fs = nr.renderer._fptr(o), nr.renderer._fptr(s)
        d = (ctypes.c_int * 3)(*dims)
        sdf = torch.zeros(n, dtype=torch.float32, device=dev)
        P = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        Ps = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        perm = torch.zeros(n, dtype=torch.int32, device=dev)
        vals = torch.zeros(n, dtype=torch.float32, device=dev)
        hand = torch.zeros(n, dtype=torch.float32, device=dev)
        ax = [torch.arange(N, device=dev, dtype=torch.float32) for _ in range(3)]
        lo = tuple(float(x) for x in o)
        hi = tuple(float(o[a] + np.float32(N - 1) * s[a]) for a in range(3))
        torch.cuda.synchronize()

        for sign in signs:
            def hand_values():
                # origin + (float)idx * step: one f32 multiply, one f32 add (two torch kernels an axis)
                x, y, z = ((ax[a] * float(s[a])) + float(o[a]) for a in range(3))
                P[:, 0] = x.repeat(N * N)
                P[:, 1] = y.repeat_interleave(N).repeat(N)
                P[:, 2] = z.repeat_interleave(N * N)
                owner.order_points_device(P.data_ptr(), n, perm.data_ptr(), lo=lo, hi=hi, sorted_ptr=Ps.data_ptr())
                if sign == "winding":
                    m.winding_device(Ps.data_ptr(), n, sdf_ptr=vals.data_ptr())
                else:
                    m.distance_device(Ps.data_ptr(), n, vals.data_ptr())
                hand[perm.long()] = vals

            st = m.sample_grid_device(sdf.data_ptr(), origin, step, dims, sign=sign, with_stats=True)
            tf, th = timed_pair(lambda: m.sample_grid_device(sdf.data_ptr(), origin, step, dims, sign=sign), hand_values)
            same = bool(torch.equal(sdf.view(torch.int32), hand.view(torch.int32)))
            say(f"{'sample_grid, sign ' + sign:58s} {fmt(tf)} {st['shade_evals'] / st['ray_steps']:9.1f}  {st['launches']} launches")
            say(f"{'  by hand: torch points, order, query, un-permute':58s} {fmt(th)} {'':9s}  same bits as sample_grid: {same}")

            nv, nt, st = m.remesh_device(origin, step, dims, None, 0, None, 0, sign=sign, with_stats=True)
            dV = torch.zeros((nv, 3), dtype=torch.float32, device=dev)
            dS = torch.zeros(nv, dtype=torch.int32, device=dev)
            dT = torch.zeros((nt, 3), dtype=torch.int32, device=dev)
            hV, hT = torch.zeros_like(dV), torch.zeros_like(dT)
            cnv, cnt = ctypes.c_long(0), ctypes.c_long(0)
            torch.cuda.synchronize()

            def hand_remesh():
                hand_values()
                owner._chk(L.nr_mesh_grid(owner._ctx, ctypes.c_void_p(hand.data_ptr()), fo, fs, d, 0.0, ctypes.c_void_p(hV.data_ptr()), nv,
                                          ctypes.c_void_p(hT.data_ptr()), nt, ctypes.byref(cnv), ctypes.byref(cnt), NR_DEVICE))

            tf, th = timed_pair(lambda: m.remesh_device(origin, step, dims, dV.data_ptr(), nv, dT.data_ptr(), nt, sign=sign), hand_remesh)
            same = bool(torch.equal(dV.view(torch.int32), hV.view(torch.int32)) and torch.equal(dT, hT))
            tfs, _ = timed_pair(lambda: m.remesh_device(origin, step, dims, dV.data_ptr(), nv, dT.data_ptr(), nt, sign=sign,
                                                        source_tri_ptr=dS.data_ptr()), None)
            st = m.remesh_device(origin, step, dims, dV.data_ptr(), nv, dT.data_ptr(), nt, sign=sign, source_tri_ptr=dS.data_ptr(),
                                 with_stats=True)[2]
            torch.cuda.synchronize()
            Vd, Td = dV.cpu().numpy(), dT.cpu().numpy()
            closed = bool(nr.trimesh_normals(Vd, Td)[1]) if nv else False
            say(f"{'remesh, sign ' + sign:58s} {fmt(tf)} {'':9s}  {nv} vertices, {nt} triangles, closed {closed}")
            say(f"{'  by hand: the values as above, then nr_mesh_grid':58s} {fmt(th)} {'':9s}  same mesh as remesh: {same}")
            say(f"{'remesh with source_tri, sign ' + sign:58s} {fmt(tfs)} {st['shade_evals'] / st['ray_steps']:9.1f}  {st['launches']} launches")

            snv, snt, sna, st = m.remesh_sparse_device(origin, step, dims, None, 0, None, 0, sign=sign, brick=args.brick, with_stats=True)
            sV = torch.zeros((snv, 3), dtype=torch.float32, device=dev)
            sK = torch.zeros(snv, dtype=torch.int64, device=dev)
            sT = torch.zeros((snt, 3), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ts, _ = timed_pair(lambda: m.remesh_sparse_device(origin, step, dims, sV.data_ptr(), snv, sT.data_ptr(), snt, sign=sign,
                                                              brick=args.brick, keys_ptr=sK.data_ptr()), None)
            torch.cuda.synchronize()
            keys = sK.cpu().numpy()
            order = np.argsort(keys, kind="stable")
            rank = np.empty(len(keys), np.int64)
            rank[order] = np.arange(len(keys))
            equal = (snv, snt) == (nv, nt) and sV.cpu().numpy()[order].tobytes() == Vd.tobytes() and \
                np.array_equal(canonical(rank[sT.cpu().numpy()]), canonical(Td))
            nb = [(N - 1 + args.brick - 1) // args.brick] * 3
            say(f"{'remesh_sparse, sign ' + sign:58s} {fmt(ts)} {st['shade_evals'] / st['ray_steps']:9.1f}  {sna} of {nb[0] * nb[1] * nb[2]} "
                f"bricks active, {st['ray_steps']} points evaluated ({st['ray_steps'] / n:.3f} of the lattice); sorted by key it is the "
                f"dense remesh: {bool(equal)}")
            del dV, dS, dT, hV, hT, sV, sK, sT
        say()

    with nr.TriMesh(owner, V, T) as m:
        bench(m, f"plane_1, scene tanh, extract_mesh at {S}^3 over [-1, 1]^3", ("normal", "winding"))
    cx = V[T].astype(np.float64).mean(1)[:, 0]
    keep = np.abs(cx) > 0.1
    with nr.TriMesh(owner, V, np.ascontiguousarray(T[keep])) as m:
        bench(m, f"repair demo: the same mesh without the {int((~keep).sum())} triangles whose centroid has |x| <= 0.1", ("winding",))
    owner.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
