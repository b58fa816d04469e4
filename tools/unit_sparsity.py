"""Measured unit sparsity of the batched fp32 tracer's unit form (nr_mlp16.h mlp64_fp32_units).

    python tools/unit_sparsity.py [--size 1024] [--steps 128] [--batch 8] [--out profiles/unit_skip_sparsity.txt]
Renders one nr_render_batch of --batch frames (cameras a turn apart on the default orbit) per bundled
network and reads nr_unit_skip_counts: the unit instructions the waves came to and those skipped
because the unit was +0 in every live lane of the wave.  Per wave evaluation a network has
inputs + 32 x hidden layers unit instructions; unit 0 of a hidden layer is always issued.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cudaneuralrender_amd as nr  # noqa: E402

GEOMS = ["plane_1", "plane_2", "plane_3", "car_1", "3a3d4a90a2db90b4203936772104a82d.obj"]

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "unit_skip_sparsity.txt"))
a = ap.parse_args()

lines = [f"# tools/unit_sparsity.py --size {a.size} --steps {a.steps} --batch {a.batch}: nr_unit_skip_counts of one nr_render_batch,",
         "# cameras a turn apart on the default orbit (distance 2); units = unit instructions per wave evaluation",
         f"# {'network':<40} {'units':>5} {'wave evals':>11} {'issued':>13} {'skipped':>13} {'skipped/eval':>12} {'share':>6} {'lanes/eval':>10}"]
for g in GEOMS:
    dims, K, B = nr.read_keras_h5(nr.geometry_path(g))
    units = dims[0] + 32 * (len(dims) - 3)
    with nr.Renderer(0) as r:
        r.load_h5(nr.geometry_path(g)).set_precision("fp32").set_static(nr.NR_COLOR_MATCAP, 3).set_scene("v1")
        r.set_matcap(nr.load_png(nr.matcap_path("Chrome")))
        frames = [(*nr.camera(0.0, 360.0 * k / a.batch, 2.0), 0) for k in range(a.batch)]
        _, st = r.render_batch(a.size, a.size, frames, a.steps)
        issued, skipped = r.unit_skip_counts()
    evals = issued // units
    points = st["ray_steps"] + st["shade_evals"]
    lines.append(f"{g:<42} {units:>5} {evals:>11} {issued:>13} {skipped:>13} {skipped / max(evals, 1):>12.1f} "
                 f"{skipped / max(issued, 1):>6.3f} {points / max(evals, 1):>10.1f}")
text = "\n".join(lines) + "\n"
print(text, end="")
with open(a.out, "w") as f:
    f.write(text)
