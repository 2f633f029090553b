"""Temporal filtering's sub-pel refinement in numpy, independent of the reference
(tests/test_tfsp.py).

The control flow is the one the fixture generator restates
(tests/golden/make_golden_tfsp.py: Side.search_block, refine_sb), shared, with
the position evaluator replaced: numpy_distortion below interpolates with the
filter taps of the AV1 specification and the rounding of the single-reference
convolve, on the CPU oracle's planes. Nothing here needs oracle/_ref.

The module also holds the inputs of the random sweep, so that the GPU test, the
coverage test of the model alone and the model-against-reference test draw the
same cases from the same seeds.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, "golden"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_golden_tfsp as G  # noqa: E402
import svtme as S  # noqa: E402

# AV1 specification, Subpel_Filters[0] (EIGHTTAP_REGULAR), phases 0..8; phase 16 - p is phase p
# mirrored, and every phase sums to 128. The bilinear filter is 128 - 8 p, 8 p.
_SPEC_HALF = [[0, 0, 0, 128, 0, 0, 0, 0], [0, 2, -6, 126, 8, -2, 0, 0], [0, 2, -10, 122, 18, -4, 0, 0],
              [0, 2, -12, 116, 28, -8, 2, 0], [0, 2, -14, 110, 38, -10, 2, 0], [0, 2, -14, 102, 48, -12, 2, 0],
              [0, 2, -16, 94, 58, -12, 2, 0], [0, 2, -14, 84, 66, -12, 2, 0], [0, 2, -14, 76, 76, -14, 2, 0]]
SPEC_REGULAR = np.array(_SPEC_HALF + [_SPEC_HALF[16 - p][::-1] for p in range(9, 16)], np.int64)
assert (SPEC_REGULAR.sum(axis=1) == 128).all()


def q4_distortion(cen, ref, pad, b, px, py, qx, qy, bil, ss):
    """The distortion of the b x b block at (px, py) at the clamped q4 MV (qx, qy)."""
    fx, fy, x0, y0 = qx & 15, qy & 15, px + (qx >> 4), py + (qy >> 4)
    bilinear = lambda p: np.array([0, 0, 0, 128 - 8 * p, 8 * p, 0, 0, 0], np.int64)  # noqa: E731
    taps = bilinear if bil else (lambda p: SPEC_REGULAR[p])
    win = ref[pad + y0 - 3:pad + y0 + b + 4, pad + x0 - 3:pad + x0 + b + 4].astype(np.int64)
    assert win.shape == (b + 7, b + 7), (x0, y0, b)  # inside the plane's padding
    if fx and fy:
        im = ((1 << 14) + sum(taps(fx)[k] * win[:, k:k + b] for k in range(8)) + 4) >> 3
        s = (1 << 19) + sum(taps(fy)[k] * im[k:k + b] for k in range(8))
        pred = ((s + 1024) >> 11) - 384
    elif fx:
        pred = (((sum(taps(fx)[k] * win[3:3 + b, k:k + b] for k in range(8)) + 4) >> 3) + 8) >> 4
    elif fy:
        pred = (sum(taps(fy)[k] * win[k:k + b, 3:3 + b] for k in range(8)) + 64) >> 7
    else:
        pred = win[3:3 + b, 3:3 + b]
    pred = np.clip(pred, 0, 255)[::1 << ss]
    d = pred - cen[pad + py:pad + py + b:1 << ss, pad + px:pad + px + b].astype(np.int64)
    total, sse = int(d.sum()), int((d * d).sum())
    q = abs(total * total) // (b * (b >> ss))
    return ((sse - q) & 0xFFFFFFFF) << ss


def numpy_distortion(cen, ref, pad, W, H, b, px, py, mvx, mvy, bil, ss):
    """The distortion of one position by the AV1 specification's filters and the rounding of the
    single-reference convolve (round_0 3, round_1 11), independent of the reference's code."""
    qx, _, _ = G.clamp(mvx, px, b, W)
    qy, _, _ = G.clamp(mvy, py, b, H)
    return q4_distortion(cen, ref, pad, b, px, py, qx, qy, bil, ss)


def model_distortion(side, b, px, py, qx, qy, bil, centre):
    """The evaluator G.Side takes in place of the reference-backed one."""
    return q4_distortion(side.cen.full, side.ref.full, side.pad, b, px, py, qx, qy, bil,
                         side.ctl["sub_sampling_shift"])


def refine_window(centre_pyr, ref_pyrs, controls: dict, records: np.ndarray):
    """The refinement of a window -> (results [refs][SBs] of svtme.TF_SUBPEL_SB_DTYPE, coverage counts).
    centre_pyr / ref_pyrs: svtme.HostPyramid (build_host_pyramid(.., "oracle")); controls: the
    fields of svtme.TfSubpelControls; records [refs][SBs] of svtme.REF_RECORD_DTYPE."""
    cover = {k: 0 for k in G.COVERAGE_KEYS}
    out = G.refine_window(centre_pyr, list(ref_pyrs), controls, records, cover, model_distortion)
    return out, cover


# ----------------------------------------------------------------------------
# the random sweep's inputs
# ----------------------------------------------------------------------------
SWEEP_SHAPES = ((72, 40), (136, 72), (200, 72), (124, 66), (64, 64), (8, 8))
SWEEP_KINDS = ("frac", "noise", "sat")
SWEEP_EXIT_TH = (0, 1, 2, 4, 8, 64)
SWEEP_64_ONLY_TH = (0, 10, 35, 200, 255)
SWEEP_ERR_32_TH = (0, 8 * 32 * 32, 20 * 32 * 32, G.U64_MAX)
SWEEP_CENTRE = 8  # the references are among the 8 pictures before and after it (tfsp_content.MARGIN)


def sweep_case(seed: int, n: int = None) -> dict:
    """The case of a seed: shape, content, window and controls drawn uniformly from the ranges
    svtme_tf_subpel accepts (`n`: the number of references, drawn from 1..MAX_BATCH_JOBS when None)."""
    rng = np.random.default_rng(seed)
    w, h = SWEEP_SHAPES[int(rng.integers(0, len(SWEEP_SHAPES)))]
    kind = SWEEP_KINDS[int(rng.integers(0, len(SWEEP_KINDS)))]
    drawn = int(rng.integers(1, S.MAX_BATCH_JOBS + 1))
    n = drawn if n is None else n
    others = [SWEEP_CENTRE + d for d in range(-8, 9) if d]
    refs = [int(t) for t in rng.permutation(others)[:n]]
    pick = lambda values: values[int(rng.integers(0, len(values)))]  # noqa: E731
    ctl = dict(half_pel_mode=int(rng.integers(0, 4)), quarter_pel_mode=int(rng.integers(0, 4)),
               eight_pel_mode=int(rng.integers(0, 2)), use_2tap=int(rng.integers(0, 2)),
               sub_sampling_shift=int(rng.integers(0, 2)), enable_8x8_pred=int(rng.integers(0, 2)),
               use_pred_64x64_only_th=pick(SWEEP_64_ONLY_TH), subpel_early_exit_th=pick(SWEEP_EXIT_TH),
               pred_error_32x32_th=pick(SWEEP_ERR_32_TH))
    me = dict(hme_me_level=int(rng.integers(1, 3)), me_exit_th=pick((0, 16 * 16)))
    return {"id": f"seed{seed}", "seed": seed, "kind": kind, "w": w, "h": h, "centre": SWEEP_CENTRE, "refs": refs,
            "controls": dict(ctl, **me), "subpel": ctl}


def sweep_frames(case: dict) -> dict:
    return G.case_frames(case)


def sweep_records(case: dict, me_recs: np.ndarray) -> np.ndarray:
    """The sweep's records from the TF-ME job's [refs][SBs]."""
    return G.perturb_records(me_recs, 1000 + case["seed"])


def sweep_inputs(case: dict):
    """-> (pyramids {picture: HostPyramid}, the oracle's ME records [refs][SBs], the sweep's records)."""
    pyr = {t: S.build_host_pyramid(f, "oracle") for t, f in sweep_frames(case).items()}
    me = G.me_records(case, pyr, "oracle")
    return pyr, me, sweep_records(case, me)


def sweep_model(case: dict):
    """-> (ME records, the sweep's records, the model's results, its coverage) of a sweep case."""
    pyr, me, recs = sweep_inputs(case)
    out, cover = refine_window(pyr[case["centre"]], [pyr[r] for r in case["refs"]], case["subpel"], recs)
    return me, recs, out, cover
