"""neuralSDFRenderer --aa S / --aa-full / --aa-contrast N: the saved frame is nr_render_aa's, against
tests/aa_ref.py on the CPU oracle's S W x S H frame."""
import os
import subprocess

import numpy as np
import pytest

import aa_ref
import cudaneuralrender_amd as nr
import oracle

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "tools", "bin")


@pytest.mark.parametrize("flags,S,contrast,full", [(["--aa", "2"], 2, 32, False),
                                                   (["--aa", "3", "--aa-contrast", "200"], 3, 200, False),
                                                   (["--aa", "2", "--aa-full", "--precision", "bf16"], 2, 32, True)])
def test_renderer_aa_png(tmp_path, flags, S, contrast, full):
    W, H = 64, 48
    args = [os.path.join(BIN, "neuralSDFRenderer"), "-i", nr.geometry_path("plane_1"), "-o", str(tmp_path) + "/",
            "-W", str(W), "-H", str(H), "-rx", "-20", "-ry", "30", "-z", "1.2", "--single", "--max-steps", "128",
            "-M", nr.matcap_path("Chrome")] + flags
    p = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    png = nr.load_png(str(tmp_path / "plane_1.h5.png"))
    dims, K, B = nr.read_keras_h5(nr.geometry_path("plane_1"))
    iv, nm = nr.camera(-20, 30, 1.2)
    big, _ = oracle.OracleNet(K, B).render(S * W, S * H, iv, nm, color_type=1, matcap=nr.load_png(nr.matcap_path("Chrome")),
                                           max_steps=128)
    ref, mask = aa_ref.resolve(big, S, contrast, full)
    assert mask.sum() >= 50 and (full or (~mask & (big[::S, ::S] != 0)).sum() >= 50)
    assert f"antialiasing: {S} x {S} samples on {int(mask.sum())} edge pixels" in p.stdout
    # savePNG reverses the byte stream: the saved image is the frame rotated 180 degrees
    assert np.array_equal(png, ref[::-1, ::-1])
