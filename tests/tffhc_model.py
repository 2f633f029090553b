"""Temporal filtering's 10-bit chroma stage in numpy and Python integers, independent of the
reference (tests/test_tff_10bit_chroma.py). The glue is make_golden_tffc's through
make_golden_tffhc.filter_window_yuv_hbd; the arithmetic is ModelArithUVH below: luma's from
tests/tffh_model.py, the chroma predictor from the specification's Subpel_Filters[2] and, for the
4x4 blocks, Subpel_Filters[4] with the single-reference convolve's rounding at bit depth 10, the
chroma window error with its blend with the luma window error, both >> 4, the scaled block
errors, the per-plane decay factors, the accumulation and the normalisation. Nothing here needs
oracle/_ref.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "golden"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_golden_tffc as GC  # noqa: E402
import make_golden_tffhc as GHC  # noqa: E402
import tff_model as M  # noqa: E402
import tffc_model as MC  # noqa: E402
import tffh_model as MH  # noqa: E402

BD = MH.BD
PIX_MAX = MH.PIX_MAX
M32 = M.M32


def predict_unclipped_uv(full, pad, b, px, py, qx, qy) -> np.ndarray:
    """tffh_model.predict_unclipped for a chroma block: Subpel_Filters[4] in both directions at 4x4."""
    if b != 4:
        return MH.predict_unclipped(full, pad, b, px, py, qx, qy)
    fx, fy, x0, y0 = qx & 15, qy & 15, px + (qx >> 4), py + (qy >> 4)
    win = full[pad + y0 - 3:pad + y0 + b + 4, pad + x0 - 3:pad + x0 + b + 4].astype(np.int64)
    assert win.shape == (b + 7, b + 7), (x0, y0, b)
    tx, ty = MC.SPEC_FOUR[fx], MC.SPEC_FOUR[fy]
    if fx and fy:
        im = ((1 << (BD + 6)) + sum(tx[k] * win[:, k:k + b] for k in range(8)) + 4) >> 3
        assert im.max() < 1 << 15 and im.min() >= 0
        offset_bits = BD + 14 - 3
        return (((1 << offset_bits) + sum(ty[k] * im[k:k + b] for k in range(8)) + 1024) >> 11) - \
            ((1 << (offset_bits - 11)) + (1 << (offset_bits - 12)))
    if fx:
        return (((sum(tx[k] * win[3:3 + b, k:k + b] for k in range(8)) + 4) >> 3) + 8) >> 4
    if fy:
        return (sum(ty[k] * win[k:k + b, 3:3 + b] for k in range(8)) + 64) >> 7
    return win[3:3 + b, 3:3 + b]


def chroma_weight_hbd(sse_c: int, sse_y: int, block_error: int, mvx: int, mvy: int, split: bool, decay: int,
                      dist_th: int) -> int:
    """The weight of one 8x8 chroma quarter from the raw SSEs of 10-bit samples
    (svt_av1_apply_temporal_filter_planewise_medium_hbd_partial_c, is_chroma 1, temporal_filtering.c:1211-1333):
    both SSEs >> 4 (:800), the chroma window error (((sum << 4) / 8) << 4) / 8, the luma window error
    (((sum << 4) / 16) << 4) / 16, (chroma * 5 + luma) / 6 in 32 bits (:1299), then tff_model.weight with
    the 16x16 error >> 4 of a split block (:1241) or the 32x32 error >> 6 (:1256; tff_model.weight takes it
    before its own >> 2)."""
    sc, sy = sse_c >> ((BD - 8) * 2), sse_y >> ((BD - 8) * 2)
    win_c = ((((sc << 4) & M32) // 8 << 4) & M32) // 8
    win_y = ((((sy << 4) & M32) // 16 << 4) & M32) // 16
    win = ((win_c * 5 + win_y) & M32) // 6
    be = block_error >> 4 if split else (block_error >> 6) << 2
    return M.weight(win, be, mvx, mvy, split, decay, dist_th)[0]


def model_weights(tuples: np.ndarray) -> np.ndarray:
    out = np.zeros((len(tuples), 4), np.uint32)
    for k, t in enumerate(tuples):
        meta, ctl = GHC.tuple_meta(t)
        for j in range(4):
            mv = meta["mv16"][j] if meta["split"] else meta["mv32"]
            be = meta["err16"][j] if meta["split"] else meta["err32"]
            out[k, j] = chroma_weight_hbd(int(t[GHC.WEIGHT_COLS - 4 + j]), int(t[6 + 4 * j]), be, mv[0], mv[1],
                                          meta["split"], ctl["tf_decay_factor_cb_fp16"], ctl["tf_mv_dist_th"])
    return out


def normalise16(cen, preds, weights) -> np.ndarray:
    """1000 x centre plus the weighted predictions over their count, rounded; any square plane, u16."""
    size = cen.shape[0]
    accum, count = 1000 * cen.astype(np.int64), np.full(cen.shape, 1000, np.int64)
    for p, w in zip(preds, weights):
        wp = MC.quarter_plane(w, size)
        accum += wp * p
        count += wp
    return ((accum + (count >> 1)) // count).astype(np.uint16)


class ModelArithUVH(GHC.HbdGlueUV):
    """The arithmetic make_golden_tffhc.filter_window_yuv_hbd takes, without the reference."""
    predict16 = MH.ModelArithH.predict16
    var32_16 = MH.ModelArithH.var32_16
    sb_weights = MH.ModelArithH.sb_weights

    def predict16_uv(self, full, pad, b, px, py, qx, qy) -> np.ndarray:
        raw = predict_unclipped_uv(full, pad, b, px, py, qx, qy)
        self.cover["clip_low_uv"] += int((raw < 0).sum())
        self.cover["clip_high_uv"] += int((raw > PIX_MAX).sum())
        return np.clip(raw, 0, PIX_MAX).astype(np.uint16)

    def filter_sb_yuv16(self, cen64, cen_cb, cen_cr, preds, metas, ctl):
        yctl = GC.luma_controls(ctl)
        cen = (cen64, cen_cb, cen_cr)
        decay = (ctl["tf_decay_factor_fp16"], ctl["tf_decay_factor_cb_fp16"], ctl["tf_decay_factor_cr_fp16"])
        weights = [np.zeros((len(preds), 16), np.uint32) for _ in range(3)]
        for r, (pred, meta) in enumerate(zip(preds, metas)):
            weights[0][r] = self.sb_weights(cen64, pred[0], meta, yctl)
            dy = (pred[0].astype(np.int64) - cen64.astype(np.int64)) ** 2
            for p in (1, 2):
                dc = (pred[p].astype(np.int64) - cen[p].astype(np.int64)) ** 2
                for i in range(4):
                    m = meta[i]
                    for j in range(4):
                        y, x = (i >> 1) * 32 + (j >> 1) * 16, (i & 1) * 32 + (j & 1) * 16
                        sse_y = int(dy[y:y + 16, x:x + 16].sum())
                        sse_c = int(dc[y // 2:y // 2 + 8, x // 2:x // 2 + 8].sum())
                        mv = m["mv16"][j] if m["split"] else m["mv32"]
                        be = m["err16"][j] if m["split"] else m["err32"]
                        weights[p][r, i * 4 + j] = chroma_weight_hbd(sse_c, sse_y, be, mv[0], mv[1], m["split"],
                                                                     decay[p], ctl["tf_mv_dist_th"])
        out = [normalise16(cen[p], [pr[p] for pr in preds], weights[p]) for p in range(3)]
        return out, weights


def filter_window_yuv(centre, refs, centre_uv, ref_uvs, controls: dict, subpel: np.ndarray):
    """centre / refs: make_golden_tffh.host_picture; centre_uv / ref_uvs: (cb, cr) padded by
    make_golden_tffhc.pad_chroma16 -> (dict of make_golden_tffhc.filter_window_yuv_hbd, coverage)."""
    cover = {k: 0 for k in GHC.COUNTED_KEYS}
    res = GHC.filter_window_yuv_hbd(centre, list(refs), centre_uv, list(ref_uvs), controls, subpel, ModelArithUVH(),
                                    cover)
    return res, cover


def run_case(case: dict) -> (dict, dict):
    cover = {k: 0 for k in GHC.COUNTED_KEYS}
    return GHC.run_case(case, ModelArithUVH(), cover), cover
