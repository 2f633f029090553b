"""Temporal filtering's chroma stage in numpy and Python integers, independent of the
reference (tests/test_tff_chroma.py). It extends tests/tff_model.py: the glue is the
one the fixture generator restates (tests/golden/make_golden_tffc.py:
filter_window_yuv), with the arithmetic replaced by ModelArithUV below: the 4-tap
predictor of the 4x4 blocks from the AV1 specification's Subpel_Filters[4], the chroma
window error and its blend with the luma window error, the per-plane decay factors,
the accumulation and the normalisation. Nothing here needs oracle/_ref.

The module also holds the inputs of the random sweep and the numpy re-pad that a
resident chroma plane is compared with.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "golden"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_golden_tffc as GC  # noqa: E402
import svtme as S  # noqa: E402
import tff_model as M  # noqa: E402

# AV1 specification, Subpel_Filters[4], phases 0..8; phase 16 - p is phase p mirrored
_FOUR_HALF = [[0, 0, 0, 128, 0, 0, 0, 0], [0, 0, -4, 126, 8, -2, 0, 0], [0, 0, -8, 122, 18, -4, 0, 0],
              [0, 0, -10, 116, 28, -6, 0, 0], [0, 0, -12, 110, 38, -8, 0, 0], [0, 0, -12, 102, 48, -10, 0, 0],
              [0, 0, -14, 94, 58, -10, 0, 0], [0, 0, -12, 84, 66, -10, 0, 0], [0, 0, -12, 76, 76, -12, 0, 0]]
SPEC_FOUR = np.array(_FOUR_HALF + [_FOUR_HALF[16 - p][::-1] for p in range(9, 16)], np.int64)
assert (SPEC_FOUR.sum(axis=1) == 128).all()
M32 = M.M32


def chroma_weight(sse_c: int, sse_y: int, block_error: int, mvx: int, mvy: int, split: bool, decay: int,
                  dist_th: int) -> int:
    """The weight of one 8x8 chroma quarter: tff_model.weight with the window error replaced by
    ((((sse_c << 4) / 8) << 4) / 8 * 5 + the luma window error of the quarter) / 6 in 32 bits."""
    win_c = ((((sse_c << 4) & M32) // 8 << 4) & M32) // 8
    win = ((win_c * 5 + sse_y) & M32) // 6
    return M.weight(win, block_error, mvx, mvy, split, decay, dist_th)[0]


def quarter_plane(w16: np.ndarray, size: int) -> np.ndarray:
    """[size][size] from 16 weights (32x32 luma block * 4 + quarter): 64 luma, 32 chroma."""
    h, q = size // 2, size // 4
    out = np.zeros((size, size), np.int64)
    for k in range(16):
        i, j = k >> 2, k & 3
        out[(i >> 1) * h + (j >> 1) * q:, (i & 1) * h + (j & 1) * q:][:q, :q] = int(w16[k])
    return out


def normalise(cen, preds, weights) -> np.ndarray:
    """1000 x centre plus the weighted predictions over their count, rounded; any square plane."""
    size = cen.shape[0]
    accum, count = 1000 * cen.astype(np.int64), np.full(cen.shape, 1000, np.int64)
    for p, w in zip(preds, weights):
        wp = quarter_plane(w, size)
        accum += wp * p
        count += wp
    return ((accum + (count >> 1)) // count).astype(np.uint8)


class ModelArithUV(M.ModelArith):
    """The arithmetic make_golden_tffc.filter_window_yuv takes, without the reference."""

    def predict(self, full, pad, b, px, py, qx, qy) -> np.ndarray:
        if b != 4:
            return super().predict(full, pad, b, px, py, qx, qy)
        # a 4 x 4 block: Subpel_Filters[4] in both directions, the rounding unchanged
        fx, fy, x0, y0 = qx & 15, qy & 15, px + (qx >> 4), py + (qy >> 4)
        win = full[pad + y0 - 3:pad + y0 + b + 4, pad + x0 - 3:pad + x0 + b + 4].astype(np.int64)
        assert win.shape == (b + 7, b + 7), (x0, y0, b)
        tx, ty = SPEC_FOUR[fx], SPEC_FOUR[fy]
        if fx and fy:
            im = ((1 << 14) + sum(tx[k] * win[:, k:k + b] for k in range(8)) + 4) >> 3
            pred = (((1 << 19) + sum(ty[k] * im[k:k + b] for k in range(8)) + 1024) >> 11) - 384
        elif fx:
            pred = (((sum(tx[k] * win[3:3 + b, k:k + b] for k in range(8)) + 4) >> 3) + 8) >> 4
        elif fy:
            pred = (sum(ty[k] * win[k:k + b, 3:3 + b] for k in range(8)) + 64) >> 7
        else:
            pred = win[3:3 + b, 3:3 + b]
        return np.clip(pred, 0, 255).astype(np.uint8)

    def filter_sb_yuv(self, cen64, cen_cb, cen_cr, preds, metas, ctl):
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
                        weights[p][r, i * 4 + j] = chroma_weight(sse_c, sse_y, be, mv[0], mv[1], m["split"], decay[p],
                                                                 ctl["tf_mv_dist_th"])
        out = [normalise(cen[p], [pr[p] for pr in preds], weights[p]) for p in range(3)]
        return out, weights


def filter_window_yuv(centre_pyr, ref_pyrs, centre_uv, ref_uvs, controls: dict, subpel: np.ndarray):
    """-> (dict of make_golden_tffc.filter_window_yuv, coverage). centre_uv / ref_uvs: (cb, cr) padded by
    make_golden_tffc.pad_chroma."""
    cover = {k: 0 for k in GC.COVERAGE_KEYS}
    res = GC.filter_window_yuv(centre_pyr, list(ref_pyrs), centre_uv, list(ref_uvs), controls, subpel, ModelArithUV(),
                               cover)
    return res, cover


# ----------------------------------------------------------------------------
# the random sweep's inputs
# ----------------------------------------------------------------------------
SWEEP_SEEDS = tuple(range(12))
SWEEP_SHAPES = ((8, 8), (72, 40), (64, 64), (124, 66), (121, 67), (200, 72))
SWEEP_DECAYS = M.SWEEP_DECAYS


def sweep_case(seed: int) -> dict:
    """The case of a seed: the luma sweep's case of that seed (content, window, TF-ME, sub-pel and luma
    filter controls; n from 1 to 16, seeds 0 and 1 pinned to 1 and 16) at a shape of this sweep (even and
    odd sizes from 8x8 to 200x72), with chroma decay factors drawn apart from luma's."""
    case = M.sweep_case(seed)
    rng = np.random.default_rng(9000 + seed)
    case["w"], case["h"] = SWEEP_SHAPES[seed % len(SWEEP_SHAPES)]
    case["filter"] = dict(case["filter"],
                          tf_decay_factor_cb_fp16=int(SWEEP_DECAYS[int(rng.integers(0, len(SWEEP_DECAYS)))]),
                          tf_decay_factor_cr_fp16=int(SWEEP_DECAYS[int(rng.integers(0, len(SWEEP_DECAYS)))]))
    return case
