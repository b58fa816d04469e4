"""Reference for nr_render_aa: a helper, not a test.

Rules 1-3 of the call's contract (include/neural_render.h) restated in numpy on an S W x S H frame
of uint32 pixels -- the frame nr_render (or the CPU oracle) gives for that size.  Pinned on
hand-built images by tests/test_aa_cpu.py.
"""
import numpy as np


def channels(img):
    """Rule 1: uint32 (a << 24 | b << 16 | g << 8 | r) -> [..., 4] int64 (r, g, b, a)."""
    img = np.asarray(img, np.uint32)
    return np.stack([(img >> np.uint32(8 * c)) & np.uint32(0xff) for c in range(4)], -1).astype(np.int64)


def pack(ch):
    ch = np.asarray(ch, np.int64)
    return (ch[..., 0] | (ch[..., 1] << 8) | (ch[..., 2] << 16) | (ch[..., 3] << 24)).astype(np.uint32)


def edge_mask(base, contrast):
    """Rule 2: the pixels with a neighbour (of the 8, inside the image) that differs by more than
    `contrast` in some channel."""
    c = channels(base)
    H, W = c.shape[:2]
    mask = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            # pixels (y, x) whose neighbour (y + dy, x + dx) exists
            ys = slice(max(0, -dy), H - max(0, dy))
            xs = slice(max(0, -dx), W - max(0, dx))
            yn = slice(max(0, dy), H - max(0, -dy))
            xn = slice(max(0, dx), W - max(0, -dx))
            diff = np.abs(c[ys, xs] - c[yn, xn]).max(-1)
            mask[ys, xs] |= diff > contrast
    return mask


def resolve(big, S, contrast, full=False):
    """(frame, edge mask) of the W x H antialiased frame from the S W x S H frame `big`."""
    big = np.asarray(big, np.uint32)
    assert big.ndim == 2 and big.shape[0] % S == 0 and big.shape[1] % S == 0, (big.shape, S)
    H, W = big.shape[0] // S, big.shape[1] // S
    base = big[::S, ::S]
    mask = np.ones((H, W), bool) if full else edge_mask(base, contrast)
    # rule 3: (sum + S S / 2) / (S S) per channel over the pixel's S x S block, in integers
    sums = channels(big).reshape(H, S, W, S, 4).sum((1, 3))
    box = pack((sums + (S * S) // 2) // (S * S))
    return np.where(mask, box, base).astype(np.uint32), mask
