"""Temporal filtering's 10-bit luma prediction and weighting in numpy and Python integers,
independent of the reference (tests/test_tff_10bit.py).

The glue is make_golden_tff's through make_golden_tffh.filter_window_hbd; the arithmetic
is ModelArithH below: the predictor from the specification's Subpel_Filters[2]
(tff_model.SPEC_SHARP) with the single-reference convolve's rounding at bit depth 10, the
10-bit variance, the weights through tff_model.weight with the three scalings the
high-bit-depth function adds, the accumulation and the normalisation. Nothing here needs
oracle/_ref.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "golden"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_golden_tff as GF  # noqa: E402
import make_golden_tffh as GH  # noqa: E402
import tff_model as M  # noqa: E402

BD = GH.BD
PIX_MAX = GH.PIX_MAX
M32 = 0xFFFFFFFF


def predict_unclipped(full, pad, b, px, py, qx, qy) -> np.ndarray:
    """svt_av1_highbd_convolve_2d_sr_c / _x_sr_c / _y_sr_c / the copy at bd 10, round_0 3, round_1 11
    (inter_prediction.c:670-777), before clip_pixel_highbd -> [b][b] i8."""
    fx, fy, x0, y0 = qx & 15, qy & 15, px + (qx >> 4), py + (qy >> 4)
    win = full[pad + y0 - 3:pad + y0 + b + 4, pad + x0 - 3:pad + x0 + b + 4].astype(np.int64)
    assert win.shape == (b + 7, b + 7), (x0, y0, b)  # inside the plane's padding
    tx, ty = M.SPEC_SHARP[fx], M.SPEC_SHARP[fy]
    if fx and fy:
        im = ((1 << (BD + 6)) + sum(tx[k] * win[:, k:k + b] for k in range(8)) + 4) >> 3
        assert im.max() < 1 << 15 and im.min() >= 0  # the reference keeps it in int16_t
        offset_bits = BD + 14 - 3
        return (((1 << offset_bits) + sum(ty[k] * im[k:k + b] for k in range(8)) + 1024) >> 11) - \
            ((1 << (offset_bits - 11)) + (1 << (offset_bits - 12)))
    if fx:
        return (((sum(tx[k] * win[3:3 + b, k:k + b] for k in range(8)) + 4) >> 3) + 8) >> 4
    if fy:
        return (sum(ty[k] * win[k:k + b, 3:3 + b] for k in range(8)) + 64) >> 7
    return win[3:3 + b, 3:3 + b]


def weight_hbd(sse: int, block_error: int, mvx: int, mvy: int, split: bool, decay: int, dist_th: int) -> int:
    """The weight of one 16x16 quarter from the raw SSE of its 10-bit samples
    (svt_av1_apply_temporal_filter_planewise_medium_hbd_partial_c, temporal_filtering.c:1211-1333): the
    8-bit function (tff_model.weight) on sse >> 4 (:800), the 16x16 error >> 4 of a split block (:1241),
    the 32x32 error >> 6 of an unsplit one (:1256; tff_model.weight takes it before its own >> 2)."""
    be = block_error >> 4 if split else (block_error >> 6) << 2
    return M.weight(sse >> ((BD - 8) * 2), be, mvx, mvy, split, decay, dist_th)[0]


def model_weights(tuples: np.ndarray) -> np.ndarray:
    out = np.zeros((len(tuples), 4), np.uint32)
    for k, t in enumerate(tuples):
        meta, ctl = GF.tuple_meta(t)
        for j in range(4):
            mv = meta["mv16"][j] if meta["split"] else meta["mv32"]
            be = meta["err16"][j] if meta["split"] else meta["err32"]
            out[k, j] = weight_hbd(int(t[6 + 4 * j]), be, mv[0], mv[1], meta["split"], ctl["tf_decay_factor_fp16"],
                                   ctl["tf_mv_dist_th"])
    return out


def normalise16(cen64, preds, weights) -> np.ndarray:
    """1000 x centre plus the weighted predictions over their count, rounded."""
    accum, count = 1000 * cen64.astype(np.int64), np.full((64, 64), 1000, np.int64)
    for p, w in zip(preds, weights):
        wp = M.weight_plane(w)
        accum += wp * p
        count += wp
    return ((accum + (count >> 1)) // count).astype(np.uint16)


class ModelArithH(GH.HbdGlue):
    """The arithmetic make_golden_tffh.filter_window_hbd takes, without the reference."""

    def predict16(self, full, pad, b, px, py, qx, qy) -> np.ndarray:
        raw = predict_unclipped(full, pad, b, px, py, qx, qy)
        self.cover["clip_low"] += int((raw < 0).sum())
        self.cover["clip_high"] += int((raw > PIX_MAX).sum())
        return np.clip(raw, 0, PIX_MAX).astype(np.uint16)

    def var32_16(self, pred, cen, ss) -> int:
        sse, total, n = GH.var_parts(pred, cen, ss)
        return (max(sse - total * total // n, 0) << ss) & M32

    def sb_weights(self, cen64, pred, meta, ctl) -> np.ndarray:
        d = pred.astype(np.int64) - cen64.astype(np.int64)
        w = np.zeros(16, np.uint32)
        for i in range(4):
            m = meta[i]
            for j in range(4):
                y, x = (i >> 1) * 32 + (j >> 1) * 16, (i & 1) * 32 + (j & 1) * 16
                sse = int((d[y:y + 16, x:x + 16] ** 2).sum())
                mv = m["mv16"][j] if m["split"] else m["mv32"]
                be = m["err16"][j] if m["split"] else m["err32"]
                w[i * 4 + j] = weight_hbd(sse, be, mv[0], mv[1], m["split"], ctl["tf_decay_factor_fp16"],
                                          ctl["tf_mv_dist_th"])
        return w

    def filter_sb16(self, cen64, preds, metas, ctl):
        weights = np.array([self.sb_weights(cen64, p, m, ctl) for p, m in zip(preds, metas)], np.uint32)
        return normalise16(cen64, preds, weights), weights


def filter_window(centre, refs, controls: dict, subpel: np.ndarray):
    """centre / refs: make_golden_tffh.host_picture -> (plane [H][W] u16 of the aligned picture,
    err32 [refs][SBs][4], weights [refs][SBs][16], coverage)."""
    cover = {k: 0 for k in GH.COUNTED_KEYS}
    plane, err32, weights = GH.filter_window_hbd(centre, list(refs), controls, subpel, ModelArithH(), cover)
    return plane, err32, weights, cover


def run_case(case: dict) -> (dict, dict):
    cover = {k: 0 for k in GH.COUNTED_KEYS}
    return GH.run_case(case, ModelArithH(), cover), cover
