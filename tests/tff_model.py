"""Temporal filtering's luma prediction and weighting in numpy and Python integers,
independent of the reference (tests/test_tff.py).

The glue is the one the fixture generator restates (tests/golden/make_golden_tff.py:
sb_blocks, filter_meta, filter_window), shared, with the arithmetic replaced by
ModelArith below: the predictor from the AV1 specification's Subpel_Filters[2] and the
rounding of the single-reference convolve, the variance, the weights from the two
tables' defining formulas, the accumulation and the normalisation. Nothing here needs
oracle/_ref.

The module also holds the inputs of the random sweep.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "golden"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_golden_tff as GF  # noqa: E402
import make_golden_tfsp as G  # noqa: E402
import svtme as S  # noqa: E402
import tfsp_model  # noqa: E402

# AV1 specification, Subpel_Filters[2] (MULTITAP_SHARP), phases 0..8; phase 16 - p is phase p
# mirrored, and every phase sums to 128.
_SPEC_HALF = [[0, 0, 0, 128, 0, 0, 0, 0], [-2, 2, -6, 126, 8, -2, 2, 0], [-2, 6, -12, 124, 16, -6, 4, -2],
              [-2, 8, -18, 120, 26, -10, 6, -2], [-4, 10, -22, 116, 38, -14, 6, -2],
              [-4, 10, -22, 108, 48, -18, 8, -2], [-4, 10, -24, 100, 60, -20, 8, -2],
              [-4, 10, -24, 90, 70, -22, 10, -2], [-4, 12, -24, 80, 80, -24, 12, -4]]
SPEC_SHARP = np.array(_SPEC_HALF + [_SPEC_HALF[16 - p][::-1] for p in range(9, 16)], np.int64)
assert (SPEC_SHARP.sum(axis=1) == 128).all()

# exp(-i / 16) and sqrt(i) in 16 fractional bits, rounded down
EXP_TAB = [int(math.floor(math.exp(-i / 16) * 65536)) for i in range(113)]
SQRT_TAB = [math.isqrt(i << 32) for i in range(16)]
M32 = 0xFFFFFFFF


def sqrt_fast(x: int):
    """-> (value, log2_half or -1 on the table branch, table index)."""
    if x > 15:
        log2_half = (x.bit_length() - 1) >> 1
        base = x >> (2 * log2_half - 2)
        return SQRT_TAB[base] >> (17 - log2_half), log2_half, base
    return SQRT_TAB[x] >> 16, -1, x


def weight(sse: int, block_error: int, mvx: int, mvy: int, split: bool, decay: int, dist_th: int):
    """The weight of one 16x16 quarter -> (weight, index into the exp table, sqrt_fast's branch).
    block_error: the quarter's 16x16 error when the 32x32 block is split, else the 32x32 error.
    32-bit unsigned arithmetic wraps as in C."""
    dth = max((dist_th << 16) // 10, 1 << 16)
    be = (block_error if split else block_error >> 2) & M32
    dec = decay if split else (decay << 1) & M32
    d2 = (mvx * mvx + mvy * mvy) & M32
    dist, log2_half, base = sqrt_fast((d2 << 8) & M32)
    dfac = max(((dist << 12) & M32) // (dth >> 8), 1 << 8)
    comb = ((sse * 5 + be) & M32) // 6
    avg = ((comb >> 3) * (dfac >> 3)) & M32
    sd = min(avg // max(dec >> 10, 1), 7 * 16)
    return (EXP_TAB[sd] * 1000) >> 16, sd, (log2_half, base)


def weights_coverage(tuples: np.ndarray) -> dict:
    """How often the fixture "weights" reaches each index of the exp table, sqrt_fast's table branch,
    each log2_half of its other branch and each table entry that branch can read (4..15)."""
    exp_index, table, halves, bases = [0] * 113, [0], [0] * 12, [0] * 12
    for t in tuples:
        meta, ctl = GF.tuple_meta(t)
        for j in range(4):
            mv = meta["mv16"][j] if meta["split"] else meta["mv32"]
            be = meta["err16"][j] if meta["split"] else meta["err32"]
            _, sd, (lh, base) = weight(int(t[6 + 4 * j]), be, mv[0], mv[1], meta["split"],
                                       ctl["tf_decay_factor_fp16"], ctl["tf_mv_dist_th"])
            exp_index[sd] += 1
            if lh < 0:
                table[0] += 1
            else:
                halves[lh - 4] += 1  # x >= 256: log2_half 4..15
                bases[base - 4] += 1
    return {"exp_index": exp_index, "sqrt_table_branch": table, "sqrt_log2_half_4_15": halves,
            "sqrt_base_4_15": bases}


def model_weights(tuples: np.ndarray) -> np.ndarray:
    out = np.zeros((len(tuples), 4), np.uint32)
    for k, t in enumerate(tuples):
        meta, ctl = GF.tuple_meta(t)
        for j in range(4):
            mv = meta["mv16"][j] if meta["split"] else meta["mv32"]
            be = meta["err16"][j] if meta["split"] else meta["err32"]
            out[k, j] = weight(int(t[6 + 4 * j]), be, mv[0], mv[1], meta["split"], ctl["tf_decay_factor_fp16"],
                               ctl["tf_mv_dist_th"])[0]
    return out


class ModelArith:
    """The arithmetic make_golden_tff.filter_window takes, without the reference."""

    def predict(self, full, pad, b, px, py, qx, qy) -> np.ndarray:
        fx, fy, x0, y0 = qx & 15, qy & 15, px + (qx >> 4), py + (qy >> 4)
        win = full[pad + y0 - 3:pad + y0 + b + 4, pad + x0 - 3:pad + x0 + b + 4].astype(np.int64)
        assert win.shape == (b + 7, b + 7), (x0, y0, b)  # inside the plane's padding
        tx, ty = SPEC_SHARP[fx], SPEC_SHARP[fy]
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

    def var32(self, pred, cen, ss) -> int:
        d = pred[::1 << ss].astype(np.int64) - cen[::1 << ss].astype(np.int64)
        total, sse = int(d.sum()), int((d * d).sum())
        return (((sse - total * total // (32 * (32 >> ss))) & M32) << ss) & M32

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
                w[i * 4 + j] = weight(sse, be, mv[0], mv[1], m["split"], ctl["tf_decay_factor_fp16"],
                                      ctl["tf_mv_dist_th"])[0]
        return w

    def filter_sb(self, cen64, preds, metas, ctl):
        weights = np.array([self.sb_weights(cen64, p, m, ctl) for p, m in zip(preds, metas)], np.uint32)
        return normalise(cen64, preds, weights), weights


def weight_plane(w16: np.ndarray) -> np.ndarray:
    """[64][64] from the 16 weights of an SB (32x32 block * 4 + quarter)."""
    out = np.zeros((64, 64), np.int64)
    for k in range(16):
        i, j = k >> 2, k & 3
        y, x = (i >> 1) * 32 + (j >> 1) * 16, (i & 1) * 32 + (j & 1) * 16
        out[y:y + 16, x:x + 16] = int(w16[k])
    return out


def normalise(cen64, preds, weights) -> np.ndarray:
    """1000 x centre plus the weighted predictions over their count, rounded."""
    accum, count = 1000 * cen64.astype(np.int64), np.full((64, 64), 1000, np.int64)
    for p, w in zip(preds, weights):
        wp = weight_plane(w)
        accum += wp * p
        count += wp
    return ((accum + (count >> 1)) // count).astype(np.uint8)


def filter_window(centre_pyr, ref_pyrs, controls: dict, subpel: np.ndarray):
    """-> (plane [H][W] of the aligned picture, err32 [refs][SBs][4], weights [refs][SBs][16], coverage)."""
    cover = {k: 0 for k in GF.COVERAGE_KEYS}
    plane, err32, weights = GF.filter_window(centre_pyr, list(ref_pyrs), controls, subpel, ModelArith(), cover)
    return plane, err32, weights, cover


def window_tiles(centre_pyr, ref_pyrs, subpel: np.ndarray) -> np.ndarray:
    """[refs][SBs][64][64]: the final predictions alone."""
    W, H, pad = centre_pyr.width, centre_pyr.height, S.PAD_FULL
    wb, ar = (W + 63) // 64, ModelArith()
    out = np.zeros(subpel.shape + (64, 64), np.uint8)
    for r, ref in enumerate(ref_pyrs):
        for k in range(subpel.shape[1]):
            sb_x, sb_y = 64 * (k % wb), 64 * (k // wb)
            for b, bx, by, m in GF.sb_blocks(subpel[r, k]):
                qx, _, _ = G.clamp(int(subpel[r, k]["mv"]["x"][m]), sb_x + bx, b, W)
                qy, _, _ = G.clamp(int(subpel[r, k]["mv"]["y"][m]), sb_y + by, b, H)
                out[r, k, by:by + b, bx:bx + b] = ar.predict(ref.full, pad, b, sb_x + bx, sb_y + by, qx, qy)
    return out


def plane_from_weights(centre_pyr, tiles: np.ndarray, weights: np.ndarray) -> np.ndarray:
    """The filtered plane from given predictions [refs][SBs][64][64] and weights [refs][SBs][16]."""
    W, H, pad = centre_pyr.width, centre_pyr.height, S.PAD_FULL
    wb, hb = (W + 63) // 64, (H + 63) // 64
    plane = np.zeros((hb * 64, wb * 64), np.uint8)
    for k in range(wb * hb):
        sb_x, sb_y = 64 * (k % wb), 64 * (k // wb)
        cen64 = centre_pyr.full[pad + sb_y:pad + sb_y + 64, pad + sb_x:pad + sb_x + 64]
        plane[sb_y:sb_y + 64, sb_x:sb_x + 64] = normalise(cen64, tiles[:, k], weights[:, k])
    return plane[:H, :W].copy()


# ----------------------------------------------------------------------------
# the random sweep's inputs
# ----------------------------------------------------------------------------
SWEEP_SEEDS = tuple(range(20))
SWEEP_SHAPES = ((8, 8), (72, 40), (64, 64), (124, 66), (136, 72), (200, 72))
SWEEP_DECAYS = GF.DECAYS + (1024, 500_000, 8_000_000, 0xFFFFFFFF)
SWEEP_DIST_THS = GF.DIST_THS + (1, 10, 100, 200)


def sweep_case(seed: int) -> dict:
    """The case of a seed: the sub-pel sweep's case of that seed (shape, content, window, TF-ME and
    sub-pel controls; n from 1 to 16, seeds 0 and 1 pinned to 1 and 16) with filter controls drawn
    from the ranges svtme_tf_filter accepts."""
    case = tfsp_model.sweep_case(seed, n={0: 1, 1: S.MAX_BATCH_JOBS}.get(seed))
    rng = np.random.default_rng(5000 + seed)
    case["w"], case["h"] = SWEEP_SHAPES[seed % len(SWEEP_SHAPES)]
    case["filter"] = {"tf_decay_factor_fp16": int(SWEEP_DECAYS[int(rng.integers(0, len(SWEEP_DECAYS)))]),
                      "tf_mv_dist_th": int(SWEEP_DIST_THS[int(rng.integers(0, len(SWEEP_DIST_THS)))]),
                      "sub_sampling_shift": case["subpel"]["sub_sampling_shift"]}
    return case


def perturb_subpel(sub: np.ndarray, seed: int) -> np.ndarray:
    """A copy of sub-pel results [refs][SBs] moved off what the stage gave: a third of the (reference,
    SB)s get another branch, a third new split flags, a quarter of the MVs move by up to 12 (1/8 pel),
    one in 16 far beyond a picture edge, one error in 8 is replaced."""
    rng = np.random.default_rng(seed)
    out = sub.copy()
    for idx in np.ndindex(out.shape):
        sb = out[idx]
        if rng.integers(0, 3) == 0:
            sb["branch"] = rng.integers(0, 3)
        if rng.integers(0, 3) == 0:
            sb["split_32x32"] = rng.integers(0, 2, 4)
            sb["split_16x16"] = rng.integers(0, 2, (4, 4)) * rng.choice((1, 9), (4, 4))
        kind = rng.integers(0, 16, S.TFSP_BLOCKS)
        x, y = sb["mv"]["x"].astype(np.int64), sb["mv"]["y"].astype(np.int64)
        x = np.where(kind < 4, x + rng.integers(-12, 13, S.TFSP_BLOCKS), np.where(kind == 4, rng.choice((-9000, 9000)), x))
        y = np.where(kind < 4, y + rng.integers(-12, 13, S.TFSP_BLOCKS), np.where(kind == 5, rng.choice((-9000, 9000)), y))
        sb["mv"]["x"], sb["mv"]["y"] = np.clip(x, -32767, 32767), np.clip(y, -32767, 32767)
        e = rng.integers(0, 8, S.TFSP_BLOCKS)
        sb["error"] = np.where(e == 0, rng.integers(0, 1 << 20, S.TFSP_BLOCKS), sb["error"])
        out[idx] = sb
    return out
