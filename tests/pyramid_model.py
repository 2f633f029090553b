"""A numpy model of the resident luma pyramid (svtme_pyramid.hip; svtme_picture_download's geometry).

Independent of the product and of the CPU oracle: the picture is padded to a multiple of 8 by edge
replication, each lower level is the 2x2 mean (a + b + c + d + 2) >> 2 of the interior of the level
above, and every level gets edge-replicated margins of PAD_FULL / PAD_QUARTER / PAD_SIXTEENTH. A
10-bit plane (uint16) is reduced to its MSB plane (>> 2) first. tests/test_pictures.py pins the
model to the reference's pyramid hashes of tests/golden/me_cases.json.

The keyword arguments of pyramid() build deliberately wrong variants (the discrimination test of
tests/test_dg.py); the defaults are the model.
"""
import numpy as np

PAD_FULL, PAD_QUARTER, PAD_SIXTEENTH = 72, 32, 16
PADS = (PAD_FULL, PAD_QUARTER, PAD_SIXTEENTH)


def align8(v: int) -> int:
    return (v + 7) & ~7


def down(p: np.ndarray, rnd: int = 2) -> np.ndarray:
    p = p.astype(np.uint32)
    return ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + rnd) >> 2).astype(np.uint8)


def pyramid(y: np.ndarray, rnd: int = 2, margin: str = "edge", pad8: str = "edge", quarter_shift: int = 0):
    """(h, w) uint8, or uint16 reduced >> 2 -> [full, quarter, sixteenth], each with its margins."""
    y = np.asarray(y)
    if y.dtype == np.uint16:
        y = (y >> 2).astype(np.uint8)
    assert y.dtype == np.uint8 and y.ndim == 2
    h, w = y.shape
    full = np.pad(y, ((0, align8(h) - h), (0, align8(w) - w)), mode=pad8)
    if quarter_shift:  # (a wrong variant) the quarter plane from the padded plane, `quarter_shift` up and left
        o = PAD_FULL - quarter_shift
        quarter = down(np.pad(full, PAD_FULL, mode=margin)[o:o + full.shape[0], o:o + full.shape[1]], rnd)
    else:
        quarter = down(full, rnd)
    levels = (full, quarter, down(quarter, rnd))
    return [np.pad(p, pad, mode=margin) for p, pad in zip(levels, PADS)]
