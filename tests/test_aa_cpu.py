"""tests/aa_ref.py (the reference of nr_render_aa) pinned on hand-built images, and the anchor of
the contract on the CPU oracle: sub-sample (0, 0) of pixel (x, y) -- pixel (S x, S y) of the
S W x S H frame -- has the ray of pixel (x, y) of the W x H frame.  No GPU."""
import numpy as np
import pytest

import aa_ref
import cudaneuralrender_amd as nr
import oracle
from conftest import REF_CAMERAS


def px(r, g=None, b=None, a=255):
    g = r if g is None else g
    b = r if b is None else b
    return (a << 24) | (b << 16) | (g << 8) | r


def frame(rows):
    return np.array(rows, np.uint32)


def mask_of(base, contrast):
    return aa_ref.resolve(frame(base), 1, contrast)[1].astype(int).tolist()


def test_strictness():
    """A difference of exactly `contrast` is not an edge, contrast + 1 is -- in any one channel."""
    assert mask_of([[px(100), px(132)]], 32) == [[0, 0]]
    assert mask_of([[px(100), px(133)]], 32) == [[1, 1]]
    assert mask_of([[px(133), px(100)]], 32) == [[1, 1]]
    for ch in range(4):
        lo = [100, 100, 100, 100]
        hi = list(lo)
        hi[ch] += 33
        assert mask_of([[px(*lo), px(*hi)]], 32) == [[1, 1]], ch
        hi[ch] -= 1
        assert mask_of([[px(*lo), px(*hi)]], 32) == [[0, 0]], ch


def test_diagonal_neighbour_counts():
    g = px(10)
    base = [[g, g, g, g],
            [g, g, g, g],
            [g, g, g, px(200)]]
    assert mask_of(base, 32) == [[0, 0, 0, 0],
                                 [0, 0, 1, 1],
                                 [0, 0, 1, 1]]
    # only diagonal contact
    assert mask_of([[px(200), g], [g, px(200)]], 32) == [[1, 1], [1, 1]]
    assert mask_of([[px(200), px(200)], [px(200), g]], 32) == [[1, 1], [1, 1]]


def test_lone_pixel_on_the_border_and_in_a_corner():
    """Neighbours outside the image do not exist: the frame border itself is not an edge."""
    c = px(255)
    border = [[0, 0, c, 0, 0],
              [0, 0, 0, 0, 0],
              [0, 0, 0, 0, 0]]
    assert mask_of(border, 32) == [[0, 1, 1, 1, 0],
                                   [0, 1, 1, 1, 0],
                                   [0, 0, 0, 0, 0]]
    corner = [[0, 0, 0],
              [0, 0, 0],
              [0, 0, c]]
    assert mask_of(corner, 32) == [[0, 0, 0],
                                   [0, 1, 1],
                                   [0, 1, 1]]
    # a fully coloured frame has no edge, up to and including its border
    assert mask_of([[c] * 4] * 3, 0) == [[0] * 4] * 3


def test_degenerate_frames():
    c = px(255)
    assert mask_of([[c]], 0) == [[0]]
    assert mask_of([[0]], 0) == [[0]]
    assert mask_of([[0, 0, c, c, 0, 0, 0]], 32) == [[0, 1, 1, 1, 1, 0, 0]]
    assert mask_of([[0], [0], [c], [c], [0], [0], [0]], 32) == [[0], [1], [1], [1], [1], [0], [0]]
    out, m = aa_ref.resolve(frame([[c, 0], [0, 0]]), 2, 32, full=True)
    assert out.shape == (1, 1) and m.tolist() == [[True]]
    out, m = aa_ref.resolve(frame([[c, 0], [0, 0]]), 2, 32)
    assert out.tolist() == [[c]] and m.tolist() == [[False]]  # no neighbour: not an edge, base unchanged


def test_round_half_up():
    """(sum + S S / 2) / (S S): at S = 2, sum 2 of 4 gives 1 and sum 1 gives 0; at S = 3 (+ 4, / 9)
    sum 5 gives 1 and sum 4 gives 0."""
    def one(vals, S):
        big = frame(np.array(vals).reshape(S, S))
        return int(aa_ref.resolve(big, S, 0, full=True)[0][0, 0])

    assert one([2, 0, 0, 0], 2) == 1
    assert one([1, 1, 0, 0], 2) == 1
    assert one([1, 0, 0, 0], 2) == 0
    assert one([5, 0, 0, 0, 0, 0, 0, 0, 0], 3) == 1
    assert one([1, 1, 1, 1, 1, 0, 0, 0, 0], 3) == 1
    assert one([4, 0, 0, 0, 0, 0, 0, 0, 0], 3) == 0
    assert one([13, 0, 0, 0, 0, 0, 0, 0, 0], 3) == 1
    assert one([14, 0, 0, 0, 0, 0, 0, 0, 0], 3) == 2
    # channels do not carry into each other: 255 everywhere stays 255
    assert one([0xffffffff] * 4, 2) == 0xffffffff
    assert one([0xffffffff] * 9, 3) == 0xffffffff


def test_alpha_is_coverage_and_colours_premultiplied():
    c = px(200, 100, 40)
    # pixel (0, 0) of a 2 x 1 frame at S = 2: three of its four samples are covered
    big = frame([[c, c, 0, 0],
                 [c, 0, 0, 0]])
    out, m = aa_ref.resolve(big, 2, 32)
    assert m.tolist() == [[True, True]]
    # (600 + 2) / 4 = 150, (300 + 2) / 4 = 75, (120 + 2) / 4 = 30, alpha (765 + 2) / 4 = 191
    assert out.tolist() == [[px(150, 75, 30, 191), 0]]
    # S = 4, one sample of sixteen: (200 + 8) / 16 = 13, (100 + 8) / 16 = 6, (40 + 8) / 16 = 3, alpha (255 + 8) / 16 = 16
    big = np.zeros((4, 8), np.uint32)
    big[0, 0] = c
    out, m = aa_ref.resolve(big, 4, 32)
    assert out.tolist() == [[px(13, 6, 3, 16), 0]]
    # the edge's other side gains the coverage of samples its own base ray missed
    big = np.zeros((4, 8), np.uint32)
    big[0, 0] = c
    big[:, 6:] = c
    out, m = aa_ref.resolve(big, 4, 32)
    assert out.tolist() == [[px(13, 6, 3, 16), px(100, 50, 20, 128)]]


def test_contrasts_0_254_255():
    base = [[px(10), px(11), px(11), 0]]
    assert mask_of(base, 0) == [[1, 1, 1, 1]]
    assert mask_of(base, 1) == [[0, 0, 1, 1]]
    assert mask_of(base, 254) == [[0, 0, 1, 1]]   # alpha 255 against the background's 0
    assert mask_of(base, 255) == [[0, 0, 0, 0]]   # finds no edge
    big = frame([[px(10), px(50), px(11), px(51), px(11), px(51), 0, 0]])
    out, m = aa_ref.resolve(big.repeat(2, 0), 2, 255)
    assert not m.any() and np.array_equal(out, big[:, ::2])


def test_full_mode():
    c = px(255)
    big = frame([[c, c, c, 0],
                 [c, c, 0, 0]])
    out, m = aa_ref.resolve(big, 2, 255, full=True)
    assert m.all()
    assert out.tolist() == [[c, px(64, 64, 64, 64)]]
    # S = 1: every pixel is "resolved" from its one sample
    out, m = aa_ref.resolve(big, 1, 32, full=True)
    assert m.all() and np.array_equal(out, big)
    # a non-edge pixel keeps its base colour in adaptive mode even when its other samples differ
    big = frame([[c, 0, c, 0],
                 [0, 0, 0, 0]])
    out, m = aa_ref.resolve(big, 2, 32)
    assert not m.any() and out.tolist() == [[c, c]]


@pytest.fixture(scope="module")
def plane(nets):
    dims, K, B = nets["plane_1"]
    return oracle.OracleNet(K, B)


@pytest.mark.parametrize("W,H,S", [(37, 29, 2), (37, 29, 3), (37, 29, 4), (64, 48, 2)])
def test_anchor_on_the_oracle(plane, W, H, S):
    """big[::S, ::S] is the W x H frame, pixel for pixel; 64 x 48 at S = 2 makes S W a power of two
    (the reciprocal form of the pixel coordinate)."""
    iv, nm = nr.camera(*REF_CAMERAS["plane_1"])
    base, _ = plane.render(W, H, iv, nm, max_steps=300)
    big, _ = plane.render(S * W, S * H, iv, nm, max_steps=300)
    assert (base != 0).sum() >= 20
    assert np.array_equal(big[::S, ::S], base)
