"""Test content with true fractional motion, for the TF sub-pel refinement
(tests/test_tfsp.py, tests/golden/make_golden_tfsp.py).

A band-limited texture is made at 8x resolution in integer arithmetic (random
cells, smoothed twice by a box filter: exact on every platform) and decimated by
8 x 8 box averages at offsets of t * k / 8 pixels, so that picture t is the
texture moved by a fraction of a pixel per picture. Two motions share a picture:
a static mask of 32-pixel cells in the upper half and of 8-pixel cells in the
lower half picks the motion of each cell, so that some 64x64, 32x32 and 16x16
blocks hold both motions and are better predicted in parts.
"""
import numpy as np

MARGIN = 40  # pixels of texture around the picture: |t * k / 8| stays below it
MOTIONS = ((3, -5), (-13, 10))  # (kx, ky) in 1/8 pixel per picture, per mask value


def _box(a: np.ndarray, n: int, axis: int) -> np.ndarray:
    """Sums over windows of n samples along axis (valid part), int64."""
    c = np.cumsum(a, axis=axis, dtype=np.int64)
    c = np.concatenate([np.zeros_like(np.take(c, [0], axis=axis)), c], axis=axis)
    hi = np.take(c, np.arange(n, c.shape[axis]), axis=axis)
    lo = np.take(c, np.arange(0, c.shape[axis] - n), axis=axis)
    return hi - lo


def texture8(w: int, h: int, seed: int) -> np.ndarray:
    """The texture at 8x resolution, int64 in [0, 255], covering the picture and MARGIN around it."""
    rng = np.random.default_rng(seed)
    W8, H8 = (w + 2 * MARGIN) * 8, (h + 2 * MARGIN) * 8
    out = np.zeros((H8, W8), np.int64)
    for cell, weight in ((48, 5), (20, 3)):  # cells of 6 and 2.5 pixels
        n = 2 * (cell // 2)
        gh, gw = (H8 + 2 * n) // cell + 2, (W8 + 2 * n) // cell + 2
        g = rng.integers(0, 256, (gh, gw), dtype=np.int64)
        layer = np.kron(g, np.ones((cell, cell), np.int64))[:H8 + 2 * n - 2, :W8 + 2 * n - 2]
        for _ in range(2):  # a tent: two box filters of n samples per axis
            layer = _box(_box(layer, n, 0), n, 1)
        out += weight * (layer // (n ** 4))
    return out // 8


def mask(w: int, h: int, seed: int) -> np.ndarray:
    """Which motion each pixel follows: 32-pixel cells in the upper half, 8-pixel cells below."""
    rng = np.random.default_rng(seed + 1)
    big = np.kron(rng.integers(0, 2, ((h + 31) // 32, (w + 31) // 32)), np.ones((32, 32), np.int64))[:h, :w]
    small = np.kron(rng.integers(0, 2, ((h + 7) // 8, (w + 7) // 8)), np.ones((8, 8), np.int64))[:h, :w]
    rows = np.arange(h)[:, None]
    return np.where(rows < h // 2, big, small).astype(bool)


def _decimate(tex: np.ndarray, w: int, h: int, ox: int, oy: int) -> np.ndarray:
    """The w x h picture whose sample (x, y) is the rounded mean of the 8 x 8 texture samples
    at (8 (x + MARGIN) + ox, 8 (y + MARGIN) + oy)."""
    y0, x0 = 8 * MARGIN + oy, 8 * MARGIN + ox
    s = _box(_box(tex[y0:y0 + 8 * h, x0:x0 + 8 * w], 8, 0), 8, 1)[::8, ::8]
    return ((s + 32) // 64).astype(np.uint8)


def fractional_frames(w: int, h: int, ts, seed: int = 7, one_motion: bool = False) -> dict:
    """{t: luma plane}: picture t is the texture moved by t * MOTIONS[m] / 8 pixels, m by the mask
    (one_motion: MOTIONS[0] everywhere, a picture that glides as a whole)."""
    tex, m = texture8(w, h, seed), mask(w, h, seed)
    out = {}
    for t in ts:
        a, b = (_decimate(tex, w, h, t * kx, t * ky) for kx, ky in MOTIONS)
        out[t] = a if one_motion else np.where(m, b, a)
    return out
