"""The batched fp32 tracer's unit form (nr_mlp16.h mlp64_fp32_units) against the CPU oracle, bit for bit.

Every case goes through nr_render_batch.  The unit form (the default: unit skip on, prune mode 1)
issues one matrix instruction per hidden input unit and skips the units that are +0 in every live
lane of the wave; unit skip off, and prune modes 0 and 2, run the paths they ran before.  All four
give the oracle's frames and statistics.  Shapes: 40 x 24 with three cameras at 16 steps (ragged
8 x 8 blocks, fewer rays than one wave per workgroup) and 96 x 96 with two cameras at 64 steps.
Networks: plane_1; a designed network with thirty dead units per layer, which must skip; dense random
networks of 1, 3 and 8 hidden layers; a 4-input network with a frame number per frame; and a network
whose scaled pack is refused, which takes the fallback and skips nothing.
"""
import functools

import numpy as np
import pytest

import cudaneuralrender_amd as nr
import depth_nets
import designed_nets
import oracle

pytestmark = pytest.mark.gpu

F = np.float32
CAMS = {"mid": (-15.0, 30.0, 2.0), "far": (10.0, 200.0, 8.0), "inside": (0.0, 75.0, 1.0), "depth": depth_nets.CAMERA}
# (W, H, cameras of the batch, steps)
SHAPES = [(40, 24, ("mid", "far", "inside"), 16), (96, 96, ("mid", "depth"), 64)]
STAT_KEYS = ("ray_steps", "shade_evals", "rays_hit", "rays_shaded")
NETS = ("plane_1", "designed", "dense1", "dense3", "dense8", "four_inputs", "refused")
# (unit skip, prune mode): the unit form, its A/B arm, and the two modes that keep their paths
MODES = ((1, 1), (0, 1), (1, 0), (1, 2))


@functools.lru_cache(maxsize=None)
def _weights(name):
    if name == "designed":
        # a tilted plane through the volume: two live units per layer, thirty that never fire
        return designed_nets.linear_net((0.3, 0.8, -0.5), 0.05, nh=3)
    if name.startswith("dense"):
        dims, K, B = depth_nets.cached_net(int(name[5:]), 3)
        return list(dims), list(K), list(B)
    if name == "four_inputs":
        dims, K, B = depth_nets.cached_net(2, 4)
        return list(dims), list(K), list(B)
    dims, K, B = nr.read_keras_h5(nr.geometry_path("plane_1"))
    if name == "refused":
        K = [k.copy() for k in K]
        K[2][1, 1] = F(1e-30)  # a weight below 2^-60: no scaled pack, hence no unit pack
    return dims, K, B


def _frame_of(name, k):
    return 3 + 7 * k if name == "four_inputs" else 0


@functools.lru_cache(maxsize=None)
def _chrome():
    return nr.load_png(nr.matcap_path("Chrome"))


@functools.lru_cache(maxsize=None)
def _ref(name, W, H, cam, frame, steps):
    """The oracle's frame and statistics (once per network, view and shape; read-only)."""
    dims, K, B = _weights(name)
    iv, nm = nr.camera(*CAMS[cam])
    img, st = oracle.OracleNet(K, B).render(W, H, iv, nm, frame=frame, color_type=1, num_inputs=dims[0],
                                            scene=nr.NR_SCENE["v1"], matcap=_chrome(), max_steps=steps, nthreads=16)
    img.setflags(write=False)
    return img, st


@pytest.fixture(scope="module", params=NETS)
def rend(request):
    r = nr.Renderer(0)
    dims, K, B = _weights(request.param)
    r.load_mlp(dims, K, B).set_precision("fp32").set_static(nr.NR_COLOR_MATCAP, dims[0]).set_scene("v1")
    r.set_matcap(_chrome())
    yield request.param, r
    r.close()


def _render(r, name, unit_skip, mode, W, H, names, steps):
    r.set_unit_skip(unit_skip).set_prune(mode)
    try:
        imgs, st = r.render_batch(W, H, [(*nr.camera(*CAMS[c]), _frame_of(name, k)) for k, c in enumerate(names)], steps)
        return imgs, st, r.unit_skip_counts()
    finally:
        r.set_unit_skip(1).set_prune(1)


@pytest.mark.parametrize("W,H,names,steps", SHAPES)
def test_every_mode_matches_the_oracle(rend, W, H, names, steps):
    name, r = rend
    dims, K, B = _weights(name)
    refs = [_ref(name, W, H, c, _frame_of(name, k), steps) for k, c in enumerate(names)]
    evals = sum(x[1]["ray_steps"] + x[1]["shade_evals"] for x in refs)
    out = {}
    for us, mode in MODES:
        imgs, st, (issued, skipped) = _render(r, name, us, mode, W, H, names, steps)
        print(name, (W, H), "unit skip", us, "prune", mode, "issued", issued, "skipped", skipped, "ray_steps", st["ray_steps"])
        for k, (img, (ref, _)) in enumerate(zip(imgs, refs)):
            assert np.array_equal(img, ref), (us, mode, names[k], int((img != ref).sum()))
        for key in STAT_KEYS:
            assert st[key] == sum(x[1][key] for x in refs), (us, mode, key)
        assert st["iterations"] == max(x[1]["iterations"] for x in refs), (us, mode)
        out[us, mode] = (imgs, {k: st[k] for k in STAT_KEYS + ("iterations",)}, issued, skipped)
    for key in MODES[1:]:
        assert out[key][1] == out[1, 1][1]
        assert all(np.array_equal(a, b) for a, b in zip(out[key][0], out[1, 1][0]))
        assert out[key][2] == 0 and out[key][3] == 0, key  # the other paths count nothing
    issued, skipped = out[1, 1][2:]
    units = dims[0] + 32 * (len(dims) - 3)
    if name == "refused":
        assert nr.pack_fp32_units(dims, K, B) is None
        assert issued == 0 and skipped == 0
        return
    assert nr.pack_fp32_units(dims, K, B) is not None
    assert skipped <= issued and issued % units == 0
    if evals > 0:
        # every live point is evaluated by some wave of 64: at least evals / 64 wave evaluations
        assert issued >= units * ((evals + 63) // 64)
    if name == "designed" and evals > 0:
        assert skipped > 0
