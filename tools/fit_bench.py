"""Distils plane_1 (7 hidden layers) into a [3, 32 x 4, 1] network with nr_fit_run and times the fit.

Data, on the device: --points/2 points uniform in the ball of radius 1.2, as many projected onto the
surface by nr_project_points and jittered (normal, sigma 0.03), shuffled; Y = nr_mlp_forward of the
teacher; clamp = 0.1.
Timing: nr_fit_run on device pointers at batch 2^16 and 2^18 for nh = 3 and nh = 7 students, 8 steps
per call, --reps calls after --warmup, torch.cuda events on the shared stream around the call;
beside it, in the same pass, (a) the by-hand route: the same MLP, batch, clamped loss and
torch.optim.Adam in torch fp32 on the same device, and (b) nr_mlp_gradient (the input gradient) of a
network of the same depth on the same number of points, for the cost per point.
Quality: the loss of every tenth epoch of --epochs at batch 2^16, lr 1e-3 (He-normal hidden kernels, a
last kernel 0.02 times that, so that the student starts inside the clamp), next to the loss of a
perfect student (Y is not clamped, so that is not 0), and the silhouette IoU of teacher and student
at 256^2 (the student rendered after load_into).
Runs on the GPU box: python3 tools/fit_bench.py > profiles/fit_bench.txt"""
import argparse
import os
import sys

import numpy as np
import torch  # device buffers; initialised before libnr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cudaneuralrender_amd as nr  # noqa: E402

CLAMP = 0.1
STEPS_PER_CALL = 8


def init_net(nh, seed):
    rng = np.random.default_rng(seed)
    dims = [3] + [32] * (nh + 1) + [1]
    K = [rng.normal(0, np.sqrt(2.0 / i), (i, o)).astype(np.float32) for i, o in zip(dims[:-1], dims[1:])]
    # a small last kernel: the student starts inside the clamp, where the clamped loss has a gradient
    K[-1] = (K[-1] * np.float32(0.02)).astype(np.float32)
    B = [np.zeros(o, np.float32) for o in dims[1:]]
    return dims, K, B


def torch_student(dims, K, B, dev):
    layers = []
    for l, (k, b) in enumerate(zip(K, B)):
        lin = torch.nn.Linear(k.shape[0], k.shape[1])
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(k.T.copy()))
            lin.bias.copy_(torch.from_numpy(b))
        layers.append(lin)
        if l < len(K) - 1:
            layers.append(torch.nn.ReLU())
    return torch.nn.Sequential(*layers).to(dev)


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


def silhouette(r, size=256):
    iv, nm = nr.camera(0.0, 0.0, 2.0)
    r.set_view(iv, nm, 0).set_static(nr.NR_COLOR_FACING, 3).set_scene("v1")
    img, _ = r.render(size, size, 256)
    return img != 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 21)
    ap.add_argument("--epochs", type=int, default=400)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    n = args.points
    dev = torch.device("cuda:0")
    torch.cuda.init()
    stream = torch.cuda.current_stream(dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)

    teacher = nr.Renderer(0)
    teacher.load_h5(nr.geometry_path("plane_1")).set_precision("fp32")
    teacher.set_stream(stream.cuda_stream)
    # uniform in the ball of radius 1.2
    d = torch.randn((n // 2, 3), generator=gen, device=dev)
    u = torch.rand((n // 2, 1), generator=gen, device=dev)
    ball = (d / d.norm(dim=1, keepdim=True) * 1.2 * u.pow(1.0 / 3.0)).float().contiguous()
    # as many on the surface (projected from points of the ball), jittered
    seeds = ball[torch.randperm(n // 2, generator=gen, device=dev)].contiguous()
    surf = torch.zeros_like(seeds)
    status = torch.zeros(n // 2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    teacher.project_points_device(seeds.data_ptr(), n // 2, position_ptr=surf.data_ptr(), status_ptr=status.data_ptr())
    teacher.synchronize()
    conv = float((status == nr.NR_PROJ_CONVERGED).float().mean())
    surf = surf + 0.03 * torch.randn(surf.shape, generator=gen, device=dev)
    X = torch.cat([ball, surf])[torch.randperm(n, generator=gen, device=dev)].float().contiguous()
    X = torch.nan_to_num(X)
    Y = torch.zeros(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    teacher.mlp_forward_device(X.data_ptr(), Y.data_ptr(), n)
    teacher.synchronize()
    print(f"plane_1 -> student; {n} points ({n // 2} uniform in the ball of radius 1.2, {n // 2} projected onto the surface "
          f"({conv:.3f} converged) and jittered by 0.03); clamp {CLAMP}; ms = torch.cuda events around the call on the "
          f"shared stream, median (min, max) of {args.reps} after {args.warmup} warm-up; {STEPS_PER_CALL} steps per call")
    print(f"|Y| < clamp at {float((Y.abs() < CLAMP).float().mean()):.3f} of the points")

    owner = nr.Renderer(0)
    owner.set_stream(stream.cuda_stream)
    # ---- timing
    for nh in (3, 7):
        dims, K, B = init_net(nh, 17 + nh)
        probe = nr.Renderer(0)
        probe.load_mlp(dims, K, B).set_stream(stream.cuda_stream)
        for batch in (1 << 16, 1 << 18):
            m = batch * STEPS_PER_CALL
            if m > n:
                print(f"nh = {nh}, batch {batch}: needs {m} points, skipped")
                continue
            with nr.Fit(owner, dims, K, B, lr=1e-3, clamp=CLAMP) as f:
                fit_ms = timed(stream, lambda: f.run_device(X.data_ptr(), Y.data_ptr(), m, batch), args.warmup, args.reps)
            net = torch_student(dims, K, B, dev)
            opt = torch.optim.Adam(net.parameters(), lr=1e-3)

            def by_hand():
                for k in range(STEPS_PER_CALL):
                    xb, yb = X[k * batch:(k + 1) * batch], Y[k * batch:(k + 1) * batch]
                    opt.zero_grad(set_to_none=True)
                    e = net(xb)[:, 0].clamp(-CLAMP, CLAMP) - yb
                    (0.5 * (e * e).mean()).backward()
                    opt.step()

            hand_ms = timed(stream, by_hand, args.warmup, args.reps)
            val = torch.zeros(m, dtype=torch.float32, device=dev)
            g = torch.zeros((m, 3), dtype=torch.float32, device=dev)
            grad_ms = timed(stream, lambda: probe.mlp_gradient_device(X.data_ptr(), m, val.data_ptr(), g.data_ptr()),
                            args.warmup, args.reps)
            print(f"nh = {nh}, batch 2^{batch.bit_length() - 1}:")
            for name, (med, lo, hi) in (("nr_fit_run", fit_ms), ("torch fp32 + torch.optim.Adam", hand_ms),
                                        ("nr_mlp_gradient, same points", grad_ms)):
                print(f"  {name:32s} {med / STEPS_PER_CALL:8.4f} ms/step ({lo / STEPS_PER_CALL:.4f}, {hi / STEPS_PER_CALL:.4f})  "
                      f"{m / med / 1e3:9.1f} Mpoints/s  {med / fit_ms[0]:6.2f} x nr_fit_run")
        probe.close()

    # ---- quality: nh = 3
    dims, K, B = init_net(3, 20)
    batch = 1 << 16
    steps = n // batch
    losses = torch.zeros(steps, dtype=torch.float32, device=dev)
    curve = []
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
        step = f.weights()[3]
    curve = [float(c) for c in curve]
    print(f"quality: [3, 32 x 4, 1], batch 2^16, lr 1e-3, {args.epochs} epochs = {step} steps in {e0.elapsed_time(e1):.1f} ms "
          f"(host loop included)")
    floor = float(((Y.clamp(-CLAMP, CLAMP) - Y) ** 2).mean())
    print("loss of every tenth epoch (mean over its steps): " + " ".join(f"{c:.3e}" for c in curve[::10]) + f"; last {curve[-1]:.3e}")
    print(f"loss of a student equal to the teacher (Y is not clamped): {floor:.3e}")
    teacher.set_stream(None, own=True)
    st, ss = silhouette(teacher), silhouette(student)
    print(f"silhouette at 256^2: teacher {int(st.sum())} px, student {int(ss.sum())} px, IoU {float((st & ss).sum() / max((st | ss).sum(), 1)):.4f}")
    for r in (student, owner, teacher):
        r.close()


if __name__ == "__main__":
    main()
