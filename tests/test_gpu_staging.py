"""The host staging of the C ABI's point and ray calls (csrc/nr_ctx.h Staging): whatever subset of the
outputs a caller asks for, and wherever its arrays live, every output holds the same bytes.  For each
entry point and n = 1, 65 and 257 (one point, one wave plus one, one 256-thread workgroup plus one):
  (a) host arrays, every output;
  (b) host arrays, the last output alone, and the first plus one from the middle, each equal to (a)'s;
  (c) device buffers (torch tensors), every output, equal to (a)'s -- where renderer.py has a _device
      wrapper for the call.
A size term that disagrees with its carve, or a download from the wrong place, shows here."""
import ctypes

import numpy as np
import pytest
import torch

import cudaneuralrender_amd as nr
import trimesh_ref
from compose_ref import SUBTRACT, UNION, part, rot_xyz
from cudaneuralrender_amd._lib import NR_DEVICE, NR_HOST, check

pytestmark = pytest.mark.gpu
if torch.cuda.is_available():
    torch.cuda.init()

F, I = np.float32, np.int32
SIZES = (1, 65, 257)
NMAX = max(SIZES)
STEPS = 96
FILL = 0xA5  # what an output holds before the call, on the host and on the device alike


@pytest.fixture(scope="module")
def scene():
    """plane_1 on one renderer, a composition of three of it, a cube; the seeded inputs."""
    rng = np.random.default_rng(2024)
    pts = rng.uniform(-1.0, 1.0, (NMAX, 3)).astype(F)
    origins = rng.normal(size=(NMAX, 3))
    origins = (2.5 * origins / np.linalg.norm(origins, axis=1, keepdims=True)).astype(F)
    dirs = (-origins + rng.uniform(-0.6, 0.6, (NMAX, 3))).astype(F)
    V, T = trimesh_ref.mesh("cube")
    parts = [part(0, UNION, None, (-0.8, 0.0, 0.0), 1.0), part(0, UNION, rot_xyz(0.3, 1.0, -0.2), (0.9, 0.2, 0.1), 0.75),
             part(0, SUBTRACT, rot_xyz(1.2, 0.4, 0.5), (-0.8, 0.0, 0.0), 0.6)]
    with nr.Renderer(0) as r:
        r.load_h5(nr.geometry_path("plane_1"))
        r.set_precision("fp32").set_static(nr.NR_COLOR_FACING, 3).set_scene("tanh").set_view(*nr.camera(0.0, 0.0, 2.0), 0)
        with nr.Composition(r, [r], parts) as cp, nr.TriMesh(r, V, T) as mesh:
            yield {"r": r, "cp": cp, "mesh": mesh, "pts": pts, "origins": origins, "dirs": dirs}


# entry point -> (inputs, outputs as (name, words per item, dtype), has a _device wrapper, the call)
def entries(s):
    L, r, cp, m = nr.lib(), s["r"], s["cp"], s["mesh"]
    opts = nr.NRProjectOpts(0.0, 1e-5, 0.25, 32)
    rays = (s["origins"], s["dirs"])
    query = [("status", 1, I), ("steps", 1, I), ("t", 1, F), ("position", 3, F), ("normal", 3, F)]
    return {
        "trace_rays": (rays, query, True,
                       lambda i, o, n, loc: L.nr_trace_rays(r._ctx, *i, n, STEPS, *o, loc, None)),
        "mlp_gradient": ((s["pts"],), [("value", 1, F), ("grad", 3, F), ("normal", 3, F)], True,
                         lambda i, o, n, loc: L.nr_mlp_gradient(r._ctx, *i, n, *o, loc, None)),
        "project_points": ((s["pts"],), [("position", 3, F), ("value", 1, F), ("normal", 3, F), ("distance", 1, F),
                                         ("iters", 1, I), ("status", 1, I)], True,
                           lambda i, o, n, loc: L.nr_project_points(r._ctx, *i, n, ctypes.byref(opts), *o, loc, None)),
        "trimesh_distance": ((s["pts"],), [("sdf", 1, F), ("closest", 3, F), ("tri", 1, I), ("feature", 1, I)], True,
                             lambda i, o, n, loc: L.nr_trimesh_distance(m._m, *i, n, *o, 0, loc, None)),
        "compose_trace_rays": (rays, query + [("part", 1, I)], True,
                               lambda i, o, n, loc: L.nr_compose_trace_rays(cp._c, *i, n, STEPS, *o, loc, None)),
        "compose_sample": ((s["pts"],), [("value", 1, F), ("owner", 1, I)], False,
                           lambda i, o, n, loc: L.nr_compose_sample(cp._c, *i, n, *o, loc, None)),
    }


ENTRY_NAMES = ("trace_rays", "mlp_gradient", "project_points", "trimesh_distance", "compose_trace_rays", "compose_sample")


def run(s, entry, n, want, device=False):
    """One call for the outputs named in `want`: {name: bytes of the result}."""
    inputs, outputs, _, call = entry
    ins = [np.ascontiguousarray(a[:n]) for a in inputs]
    outs = {k: np.full((n, w) if w > 1 else (n,), FILL * 0x01010101, np.uint32).view(t) for k, w, t in outputs if k in want}
    if device:
        ins = [torch.from_numpy(a).cuda() for a in ins]
        outs = {k: torch.from_numpy(a).cuda() for k, a in outs.items()}
        ptr = lambda a: a.data_ptr()  # noqa: E731
    else:
        ptr = lambda a: a.ctypes.data  # noqa: E731
    rc = call([ptr(a) for a in ins], [ptr(outs[k]) if k in outs else None for k, _, _ in outputs], n,
              NR_DEVICE if device else NR_HOST)
    check(rc, s["r"]._ctx)
    if device:
        s["r"].synchronize()
        outs = {k: a.cpu().numpy() for k, a in outs.items()}
    return {k: a.tobytes() for k, a in outs.items()}


def same(got, full, what):
    for k, b in got.items():
        assert len(b) == len(full[k]), (what, k)
        if b != full[k]:
            g, f = np.frombuffer(b, np.uint32), np.frombuffer(full[k], np.uint32)
            raise AssertionError(f"{what}: {k}: {int((g != f).sum())} of {g.size} words differ from the full call's")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ENTRY_NAMES)
def test_outputs_do_not_depend_on_staging(scene, name, n):
    entry = entries(scene)[name]
    names = [k for k, _, _ in entry[1]]
    full = run(scene, entry, n, names)
    assert set(full) == set(names)
    for k, w, _ in entry[1]:
        assert len(full[k]) == 4 * n * w
    # something was computed: no output is left as it was filled
    assert all(b != bytes([FILL]) * len(b) for b in full.values()), [k for k, b in full.items() if b == bytes([FILL]) * len(b)]
    same(run(scene, entry, n, names[-1:]), full, "the last output alone")
    first_and_middle = [names[0]] + ([names[len(names) // 2]] if len(names) > 2 else [])
    same(run(scene, entry, n, first_and_middle), full, f"{first_and_middle} alone")
    if entry[2]:
        same(run(scene, entry, n, names, device=True), full, "device buffers")
