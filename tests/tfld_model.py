"""A model of low-delay temporal filtering (svtme_tf_filter_ld, include/svtme.h) in numpy and Python
integers: produce_temporally_filtered_pic_ld (temporal_filtering.c:3404-3816) for one window.

It stands on its own: nothing of it goes through ctypes or oracle/_ref, and it shares no code with
the fixtures' generator (tests/golden/make_golden_tfld.py), which drives the reference's own
functions. Both take the padded planes the generator's input makers give.

Per 64x64 SB, for luma and, with chroma, Cb and Cr at half size:
  1. accum = 1000 * centre, count = 1000                        (:349-421)
  2. the prediction is the co-located block of the reference    (:3693-3705, MV (0, 0))
  3. var32 of each 32x32 luma block                             (:3725-3767)
  4. w = (EXP_TAB[min(((var32 >> 2 or 6) << 2) / max(decay >> 10, 1), 112)] * 1000) >> 17 per plane;
     count += w, accum += w * pred over the block                (:818-864, :920-967)
  5. (accum + (count >> 1)) / count                              (:2607-)
"""
import math

import numpy as np

EXP_TAB = [int(math.floor(math.exp(-i / 16) * 65536)) for i in range(113)]  # expf_tab_fp16
M32 = 0xFFFFFFFF


def variance32(pred: np.ndarray, cen: np.ndarray, ss: int, bit_depth: int) -> int:
    """Step 3 for one 32x32 block: svt_aom_variance32x32_c, with ss 1 svt_aom_variance32x16_c on every
    second row and << 1 (variance.c:300-306); at 10 bit svt_aom_highbd_10_variance* (svt_psnr.c:139-177)."""
    d = pred[::1 << ss].astype(np.int64) - cen[::1 << ss].astype(np.int64)
    sse, total, n = int((d * d).sum()), int(d.sum()), 32 * (32 >> ss)
    if bit_depth == 8:
        q = abs(total * total) // n  # C division of a non-negative int64
        return (((sse & M32) - (q & M32)) & M32) << ss & M32
    sse, total = (sse + 8) >> 4, (total + 2) >> 2  # ROUND_POWER_OF_TWO; the sum's shift is arithmetic
    return (max(sse - (total * total) // n, 0) << ss) & M32


def weight(var32: int, decay: int, bit_depth: int) -> int:
    """Step 4's weight of one plane's block from the 32x32 LUMA variance and the plane's decay factor."""
    e = var32 >> (2 if bit_depth == 8 else 6)
    sd = min(((e << 2) & M32) // max(decay >> 10, 1), 7 * 16)
    return (EXP_TAB[sd] * 1000) >> 17


def filter_window(cen, refs, ctl: dict, W: int, H: int, pad=(72, 40)):
    """cen: (y, cb, cr) padded planes of the centre picture (cb, cr unused without chroma, may be None),
    refs: a list of such tuples; W x H: the 8-aligned luma size; pad: the planes' (luma, chroma) padding.
    -> {"y", "cb", "cr": the filtered planes at W x H and W/2 x H/2 (chroma only with ctl["chroma"]),
        "var32": [refs][SBs][4] u32, "weights": [refs][SBs][4][3] u32 (block, plane)}."""
    bd, ss, chroma = ctl["bit_depth"], ctl["sub_sampling_shift"], bool(ctl["chroma"])
    decay = ctl["tf_decay_factor_fp16"]
    dt = np.uint8 if bd == 8 else np.uint16
    wb, hb = (W + 63) // 64, (H + 63) // 64
    n, planes = len(refs), 3 if chroma else 1
    out = [np.zeros((hb * 64 >> (p > 0), wb * 64 >> (p > 0)), dt) for p in range(planes)]
    var32 = np.zeros((n, wb * hb, 4), np.uint32)
    weights = np.zeros((n, wb * hb, 4, 3), np.uint32)

    def block(pic, p, x, y, size):  # the size x size block at luma / chroma (x, y) of plane p, read from the padding too
        o = pad[p > 0]
        return pic[p][o + y:o + y + size, o + x:o + x + size].astype(np.int64)

    for k in range(wb * hb):
        for q in range(4):
            x, y = 64 * (k % wb) + 32 * (q & 1), 64 * (k // wb) + 32 * (q >> 1)
            c = [block(cen, p, x >> (p > 0), y >> (p > 0), 32 >> (p > 0)) for p in range(planes)]
            accum = [1000 * a for a in c]
            count = [1000] * planes
            for r, ref in enumerate(refs):
                pred = [block(ref, p, x >> (p > 0), y >> (p > 0), 32 >> (p > 0)) for p in range(planes)]
                v = variance32(pred[0], c[0], ss, bd)
                var32[r, k, q] = v
                for p in range(planes):
                    w = weight(v, decay[p], bd)
                    weights[r, k, q, p] = w
                    count[p] += w
                    accum[p] = accum[p] + w * pred[p]
            for p in range(planes):
                s = 32 >> (p > 0)
                out[p][y >> (p > 0):(y >> (p > 0)) + s, x >> (p > 0):(x >> (p > 0)) + s] = \
                    (accum[p] + (count[p] >> 1)) // count[p]
    res = {"y": out[0][:H, :W].copy(), "var32": var32, "weights": weights}
    if chroma:
        res["cb"], res["cr"] = out[1][:H // 2, :W // 2].copy(), out[2][:H // 2, :W // 2].copy()
    return res


def model_weights(tuples: np.ndarray) -> np.ndarray:
    """The weights of the fixture's table: rows of (bit_depth, tf_decay_factor_fp16, var32)."""
    return np.array([weight(int(t[2]), int(t[1]), int(t[0])) for t in tuples], np.uint32)
