"""Matcap shading on matcaps that are not square: rows against the height, columns against the width.

shade_color forms uvx from the width, uvy from the height and index = uvy * width + uvx, and
Renderer.set_matcap passes (shape[1], shape[0]); with the square 512 x 512 matcaps every other test
uses, swapping the two anywhere (kernels, ABI, wrapper, drivers) changes nothing.  Here the matcap is
coded (designed_nets.coded_matcap: texel[r, c] = 0xff000000 | r << 12 | c), so a coloured pixel names
the texel it was read at, in shapes with one row, one column, more rows than columns and the reverse.
Frames are compared with the oracle bit for bit, and the decoded (row, column) with a prediction that
does not go through the oracle: float64 arithmetic on the G-buffer's world normals.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import cudaneuralrender_amd as nr
import designed_nets as dn
import oracle
from query_ref import HIT

pytestmark = pytest.mark.gpu
W, H, STEPS, CAM = dn.MATCAP_VIEW
CAM2 = (20.0, 210.0, 1.4)
SHAPES = dn.MATCAP_SHAPES
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def plane():
    return nr.read_keras_h5(nr.geometry_path("plane_1"))


@functools.lru_cache(maxsize=None)
def ref_frame(shape, cam=CAM):
    _, K, B = plane()
    iv, nm = nr.camera(*cam)
    img, st = oracle.OracleNet(K, B).render(W, H, iv, nm, color_type=1, scene=nr.NR_SCENE["tanh"],
                                            matcap=dn.coded_matcap(*shape), max_steps=STEPS)
    img.setflags(write=False)
    return img, st


@pytest.fixture(scope="module")
def rend():
    r = nr.Renderer(0)
    dims, K, B = plane()
    r.load_mlp(dims, K, B).set_static(nr.NR_COLOR_MATCAP, 3).set_scene("tanh")
    yield r
    r.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_matcap_shapes_fp32(rend, shape):
    ref, rst = ref_frame(shape)
    assert (ref != 0).sum() > 1000
    mc = dn.coded_matcap(*shape)
    iv, nm = nr.camera(*CAM)
    rend.set_precision("fp32").set_matcap(mc).set_view(iv, nm, 0)
    try:
        for schedule in ("persistent", "wavefront", "layered"):
            img, st = rend.set_schedule(schedule).render(W, H, STEPS)
            assert np.array_equal(img, ref), (schedule, int((img != ref).sum()))
            assert st["ray_steps"] == rst["ray_steps"] and st["rays_shaded"] == rst["rays_shaded"], schedule
    finally:
        rend.set_schedule("persistent")
    imgs, _ = rend.render_batch(W, H, [(*nr.camera(*CAM), 0), (*nr.camera(*CAM2), 0)], STEPS)
    assert np.array_equal(imgs[0], ref) and np.array_equal(imgs[1], ref_frame(shape, CAM2)[0])
    # the independent prediction: rows against the height, columns against the width
    rend.set_view(iv, nm, 0)
    g = rend.render_gbuffer(W, H, STEPS)
    hit = (g["status"] == HIT).reshape(-1)
    assert np.array_equal(hit, (img != 0).reshape(-1))
    row, col, sure = dn.predict_texels(g["normal"].reshape(-1, 3)[hit], nm, shape)
    assert (~sure).sum() <= dn.NEAR_CAP * hit.sum(), (int((~sure).sum()), int(hit.sum()))
    grow, gcol = dn.decode_matcap(img.reshape(-1)[hit])
    assert (grow < shape[0]).all() and (gcol < shape[1]).all()
    assert np.array_equal(grow[sure], row[sure]) and np.array_equal(gcol[sure], col[sure])
    if shape[0] > 2:  # the view reads more than one row / column (of 2, the second only at exactly 1)
        assert len(set(grow.tolist())) > 1
    if shape[1] > 2:
        assert len(set(gcol.tolist())) > 1


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_matcap_shapes_16bit_schedules_agree(rend, prec):
    iv, nm = nr.camera(*CAM)
    try:
        rend.set_precision(prec).set_view(iv, nm, 0)
        for shape in SHAPES:
            rend.set_matcap(dn.coded_matcap(*shape))
            a, sa = rend.set_schedule("wavefront").render(W, H, STEPS)
            b, sb = rend.set_schedule("persistent").render(W, H, STEPS)
            assert np.array_equal(a, b), (shape, int((a != b).sum()))
            assert sa["ray_steps"] == sb["ray_steps"] and sa["rays_shaded"] == sb["rays_shaded"], shape
            row, col = dn.decode_matcap(a[a != 0])
            assert (a != 0).sum() > 1000 and (row < shape[0]).all() and (col < shape[1]).all(), shape
    finally:
        rend.set_precision("fp32").set_schedule("persistent")


def test_nan_normal_reads_texel_0(rend):
    """f2i_rz(NaN) = 0: a NaN normal reads texel [0, 0], whatever the shape (a flat field; every ray
    that enters the sphere is a hit with a zero gradient)."""
    dims, K, B = dn.const_net(0.0)
    mc = dn.coded_matcap(3, 5).copy()
    mc[0, 0] = 0xff123456  # unlike opaque black, unlike every other texel
    with nr.Renderer(0) as r:
        r.load_mlp(dims, K, B).set_precision("fp32").set_static(nr.NR_COLOR_MATCAP, 3).set_scene("tanh").set_matcap(mc)
        iv, nm = nr.camera(*CAM)
        r.set_view(iv, nm, 0)
        ref, _ = oracle.OracleNet(K, B).render(W, H, iv, nm, color_type=1, scene=nr.NR_SCENE["tanh"], matcap=mc,
                                               max_steps=STEPS)
        assert set(np.unique(ref).tolist()) - {0} == {0xff123456}
        for schedule in ("persistent", "wavefront", "layered"):
            img, _ = r.set_schedule(schedule).render(W, H, STEPS)
            assert np.array_equal(img, ref), schedule


def test_renderer_tool_with_a_5x9_matcap(tmp_path):
    """The headless driver's path: the matcap is a 5 x 9 PNG written by nr_png_save."""
    mc = dn.coded_matcap(5, 9)
    path = str(tmp_path / "coded.png")
    nr.save_png(path, mc, flip=False)
    assert np.array_equal(nr.load_png(path), mc)
    args = [os.path.join(REPO, "tools", "bin", "neuralSDFRenderer"), "-i", nr.geometry_path("plane_1"),
            "-o", str(tmp_path) + "/", "-W", str(W), "-H", str(H), "-rx", "-35", "-ry", "30", "-z", "1.3", "--single",
            "--max-steps", str(STEPS), "--scene", "tanh", "-M", path]
    p = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    png = nr.load_png(str(tmp_path / "plane_1.h5.png"))
    ref = ref_frame((5, 9))[0]
    assert np.array_equal(png, ref[::-1, ::-1])  # savePNG rotates the frame by 180 degrees
    row, col = dn.decode_matcap(png[png != 0])
    assert row.max() <= 4 and col.max() > 4  # columns that a 9 x 5 reading of the file does not have
