"""neuralSDFRenderer --light x,y,z and its companions: the saved frame is render_lit's for the same
view and light."""
import os
import subprocess

import numpy as np
import pytest

import cudaneuralrender_amd as nr

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "tools", "bin")
DEFAULTS = dict(shadow_steps=64, shadow_bias=0.01, shadow_k=8.0, ao_step=0.02, ao_strength=2.0, ambient=0.3)


@pytest.mark.parametrize("flags,light", [
    ([], {}),
    (["--shadow-steps", "32", "--shadow-k", "0", "--shadow-bias", "0.02", "--ao", "3", "--ao-step", "0.03", "--ambient", "0.5",
      "--precision", "bf16"],
     dict(shadow_steps=32, shadow_k=0.0, shadow_bias=0.02, ao_strength=3.0, ao_step=0.03, ambient=0.5))])
def test_renderer_light_png(tmp_path, flags, light):
    W, H = 64, 48
    args = [os.path.join(BIN, "neuralSDFRenderer"), "-i", nr.geometry_path("plane_1"), "-o", str(tmp_path) + "/",
            "-W", str(W), "-H", str(H), "-rx", "-35", "-ry", "30", "-z", "1.3", "--single", "--max-steps", "128",
            "-M", nr.matcap_path("Chrome"), "--light", "-0.8,0.6,0"] + flags
    p = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    png = nr.load_png(str(tmp_path / "plane_1.h5.png"))
    dims, K, B = nr.read_keras_h5(nr.geometry_path("plane_1"))
    with nr.Renderer(0) as r:
        r.load_mlp(dims, K, B).set_static(nr.NR_COLOR_MATCAP, 3).set_matcap(nr.load_png(nr.matcap_path("Chrome")))
        r.set_view(*nr.camera(-35, 30, 1.3), 0)
        plain, _ = r.render(W, H, 128)
        ref, st = r.render_lit(W, H, (-0.8, 0.6, 0.0), max_steps=128, with_stats=True, **dict(DEFAULTS, **light))
    assert (ref != 0).sum() >= 1000 and (ref != plain).sum() >= 1000  # the light shows in the frame
    assert f"lighting: {st['rays_shaded']} hit pixels, {st['ray_steps']} ray-steps" in p.stdout
    # savePNG reverses the byte stream: the saved image is the frame rotated 180 degrees
    assert np.array_equal(png, ref[::-1, ::-1])
