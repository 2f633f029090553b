"""Generate the low-delay TF fixtures (tests/golden/tfld_cases.json, tfld_cases.npz).

produce_temporally_filtered_pic_ld (temporal_filtering.c:3404-3816), what
svt_av1_init_temporal_filtering runs with SVT_AV1_PRED_LOW_DELAY_B: no TF-ME, no sub-pel search,
MV (0, 0) for every 64x64 block, the zz-based filter. The expected values come from the
reference's own functions in oracle/_ref/libtfsp_ref.so (make_golden_tfsp.load_enc), driven per SB:

  * svt_aom_apply_filtering_central_c / _highbd_c;
  * svt_aom_variance32x32_c / 32x16_c, svt_aom_highbd_10_variance32x32_c / 32x16_c on each
    32x32 luma block of the co-located prediction against the centre (:3725-3767);
  * svt_av1_apply_zz_based_temporal_filter_planewise_medium_c / _hbd_c per 32x32 block
    (apply_filtering_block_plane_wise, :1411-1493), with a MeContext whose
    tf_32x32_block_error, tf_32x32_block_split_flag = 0, tf_block_row / col, tf_chroma and
    tf_decay_factor_fp16 are set at the offsets make_golden_tff.me_offsets derives from the
    reference's header;
  * svt_aom_get_final_filtered_pixels_c.

For one case (PREDICTOR_CASE) the reference's predictors (svt_inter_predictor,
svt_highbd_inter_predictor) are called at MV (0, 0) for every SB and plane and must return the
co-located block: that the prediction is a copy is then checked, not assumed. Only the loop over
the SBs and the cut of each SB out of the padded planes is restated here.

  tfld_cases.json   the case list with the controls of each case, the coverage counts
  tfld_cases.npz    per case "<id>.y" [H][W], with chroma "<id>.cb", "<id>.cr" [H/2][W/2] (u8 at 8
                    bit, u16 at 10), "<id>.var32" [refs][SBs][4] u32; the weight table
                    "weights.in" [tuples][3] i8 (bit depth, decay factor, var32) and "weights.out"
                    [tuples] u32

Container only (needs oracle/_ref). Run from the repository root:
python tests/golden/make_golden_tfld.py. The output is byte-for-byte reproducible. It fails when a
coverage count is 0 (BETWEEN_DISTINCT: below 3).
"""
import ctypes as C
import json
import os
import sys
import zlib
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "svt-av1-mirror_amd"))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_golden_tff as GF  # noqa: E402
import make_golden_tffc as GC  # noqa: E402
import make_golden_tffh as GH  # noqa: E402
import make_golden_tffhc as GHC  # noqa: E402
import make_golden_tfsp as G  # noqa: E402
import svtme as S  # noqa: E402
import tfsp_content  # noqa: E402

MODES = ((8, 0, "8"), (8, 1, "8c"), (10, 0, "10"), (10, 1, "10c"))  # bit depth, chroma, suffix of the id
MID, MID2 = 150 << 10, 600 << 10  # decay factors that put the weights of the moving content strictly between 0 and 500
# tf_decay_factor_fp16[Y, Cb, Cr] by case, in turn: 0, 1023 (>> 10 is 0), the mid values, the largest
DECAYS = ((MID, 0, 0x7FFFFFFF), (1023, MID, MID2), (0x7FFFFFFF, MID2, 1023), (MID2, 0x7FFFFFFF, MID), (0, 1023, MID2))
# base id, content, w, h, centre, references, sub_sampling_shift, modes
BASES = [
    ("ld64", "frac", 64, 64, 8, [7], 0, MODES),                # one SB
    ("ld72", "frac", 72, 40, 8, [9], 1, MODES),                # 2nd SB column: 8 luma / 4 chroma true columns
    ("ld136", "frac", 136, 72, 8, [7, 9, 6], 0, MODES),        # 3 x 2 SBs, ragged both ways
    ("ld8", "frac", 8, 8, 8, [7], 0, MODES[1::2]),             # yuv only: chroma 4 x 4
    ("ld64_same", "same", 64, 64, 8, [7], 0, MODES),           # identical pictures: variance 0, weight 500
    ("ld64_dc", "dc", 64, 64, 8, [7, 9], 0, MODES),            # reference = centre + constant: variance 0, SSE large
    ("ld64_clip", "clip", 64, 64, 8, [7, 9], 1, MODES[2:]),    # 10-bit samples at 0 and 1023
]
DC = (13, -9, 5)  # the constants of the dc content by reference, in 8-bit steps
PREDICTOR_CASE = "ld136"
PLANES = ("y", "cb", "cr")
COVERAGE_KEYS = tuple(f"{k}_{p}" for p in PLANES for k in ("w500", "between", "w0")) + \
    ("var_clamped_to_0", "quadrant_beyond", "ss1_odd_rows_unseen")
BETWEEN_DISTINCT = tuple("between_distinct_" + p for p in PLANES)  # distinct weights strictly between, over the fixture


def case_dicts():
    out = []
    for b in BASES:
        for bd, chroma, suffix in b[7]:
            k = len(out)
            out.append({"id": f"{b[0]}_{suffix}", "base": b[0], "kind": b[1], "w": b[2], "h": b[3], "centre": b[4],
                        "refs": list(b[5]),
                        "controls": {"tf_decay_factor_fp16": list(DECAYS[k % len(DECAYS)]), "sub_sampling_shift": b[6],
                                     "bit_depth": bd, "chroma": chroma}})
    return out


# ----------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------
def _content_case(case: dict) -> dict:
    """The case as the sibling generators' frame makers read it: the modes of a base share their content."""
    return dict(case, id=case["base"])


def _lsb(case: dict, t: int, plane: int, shape) -> np.ndarray:
    rng = np.random.default_rng([zlib.crc32(case["base"].encode()), t, plane])
    return rng.integers(0, 4, shape, dtype=np.uint16)


def luma_frames(case: dict) -> dict:
    """{picture number: [h][w] luma} at the case's bit depth. frac / same: make_golden_tfsp.case_frames, at 10
    bit make_golden_tffh.frames10 of them (<< 2 | two random bits); clip: make_golden_tffh's cells at 0 and
    1023; dc: the centre kept inside [32, 220] and each reference the centre + DC[i] (10 bit: + 4 DC[i]; in
    the first reference two samples of each 32x32 block one step short of it, which makes the rounded
    variance of svt_aom_highbd_10_variance32x32_c negative before its clamp)."""
    bd, cc = case["controls"]["bit_depth"], _content_case(case)
    if case["kind"] != "dc":
        out = GH.frames10(cc) if bd == 10 else GH.frames8(cc)
        return {t: out[case["centre"]].copy() for t in out} if case["kind"] == "same" else out  # the two random bits too
    c, w, h = case["centre"], case["w"], case["h"]
    cen = np.clip(tfsp_content.fractional_frames(w, h, [c])[c], 32, 220).astype(np.uint16)
    if bd == 10:
        cen = (cen << 2) | _lsb(case, c, 0, cen.shape)
    out = {c: cen}
    for i, r in enumerate(case["refs"]):
        f = (cen.astype(np.int64) + DC[i] * (4 if bd == 10 else 1))
        if bd == 10 and i == 0:
            f[1::32, 1::32] -= 1
            f[4::32, 6::32] -= 1
        out[r] = f.astype(np.uint16)
    dt = np.uint16 if bd == 10 else np.uint8
    return {t: f.astype(dt) for t, f in out.items()}


def chroma_frames(case: dict) -> dict:
    """{picture number: (cb, cr)} at the case's bit depth, ((h + 1) >> 1, (w + 1) >> 1) each:
    make_golden_tffc.chroma_frames / make_golden_tffhc.chroma_frames10; dc as the luma's, without the short samples."""
    bd, cc = case["controls"]["bit_depth"], _content_case(case)
    if case["kind"] != "dc":
        out = GHC.chroma_frames10(cc) if bd == 10 else GHC.chroma_frames8(cc)
        return {t: out[case["centre"]] for t in out} if case["kind"] == "same" else out
    c = case["centre"]
    cen = [np.clip(p, 32, 220).astype(np.uint16) for p in GC.chroma_frames(dict(cc, kind="frac"))[c]]
    if bd == 10:
        cen = [(p << 2) | _lsb(case, c, 1 + k, p.shape) for k, p in enumerate(cen)]
    dt = np.uint16 if bd == 10 else np.uint8
    out = {c: tuple(p.astype(dt) for p in cen)}
    for i, r in enumerate(case["refs"]):
        out[r] = tuple((p.astype(np.int64) + DC[i] * (4 if bd == 10 else 1)).astype(dt) for p in cen)
    return out


def case_inputs(case: dict) -> dict:
    """{picture number: (y, cb, cr)} as the resident planes hold them: replicated to the aligned size and
    padded by SVTME_PAD_FULL / SVTME_PAD_CHROMA replicated samples; cb, cr None without chroma."""
    W, H = S.align8(case["w"]), S.align8(case["h"])
    luma = luma_frames(case)
    uv = chroma_frames(case) if case["controls"]["chroma"] else {t: (None, None) for t in luma}
    return {t: (GH.pad_hbd(luma[t], W, H),) + tuple(None if p is None else GC.pad_chroma(p, W, H) for p in uv[t])
            for t in luma}


def sb_block(pic, p: int, sb_x: int, sb_y: int) -> np.ndarray:
    """The SB at luma (sb_x, sb_y) of plane p of a padded picture, the padding where it overhangs."""
    pad, s = (S.PAD_FULL, S.PAD_CHROMA)[p > 0], 64 >> (p > 0)
    x, y = sb_x >> (p > 0), sb_y >> (p > 0)
    return np.ascontiguousarray(pic[p][pad + y:pad + y + s, pad + x:pad + x + s])


# ----------------------------------------------------------------------------
# the reference's arithmetic
# ----------------------------------------------------------------------------
class RefArithLD(GHC.RefArithUVH):
    """The reference's own functions of the low-delay path (oracle/_ref/libtfsp_ref.so)."""

    def __init__(self):
        GHC.RefArithUVH.__init__(self)
        self.cover = defaultdict(int)  # the predictors' clip counts (make_golden_tffh), not used here
        lib, vp, i32 = self.lib, C.c_void_p, C.c_int
        zz = [vp, vp, i32, vp, vp, i32, C.c_uint, C.c_uint, i32, i32] + [vp] * 6
        lib.svt_av1_apply_zz_based_temporal_filter_planewise_medium_c.argtypes = zz
        lib.svt_av1_apply_zz_based_temporal_filter_planewise_medium_c.restype = None
        lib.svt_av1_apply_zz_based_temporal_filter_planewise_medium_hbd_c.argtypes = zz + [C.c_uint32]
        lib.svt_av1_apply_zz_based_temporal_filter_planewise_medium_hbd_c.restype = None

    def variance32(self, pred, cen, ss: int, bd: int) -> int:
        return self.var32_16(pred, cen, ss) if bd == 10 else GF.RefArith.var32(self, pred, cen, ss)

    def zz_weight(self, bd: int, decay: int, var32: int) -> int:
        """The weight the zz function adds to the count of a 32x32 luma block with that error."""
        self.field("tf_chroma", np.uint8)[0] = 0
        self.field("tf_decay_factor_fp16", np.uint32, 3)[:] = (decay, 0, 0)
        self.field("tf_32x32_block_split_flag", np.int32, 4)[:] = 0
        self.field("tf_32x32_block_error", np.uint64, 4)[:] = (var32, 0, 0, 0)
        self.field("tf_block_row", np.int32)[0], self.field("tf_block_col", np.int32)[0] = 0, 0
        pre = np.zeros(32 * 32, np.uint16 if bd == 10 else np.uint8)
        accum, count = np.zeros(32 * 32, np.uint32), np.zeros(32 * 32, np.uint16)
        args = (self.me.ctypes.data, pre.ctypes.data, 32, None, None, 16, 32, 32, 1, 1, accum.ctypes.data,
                count.ctypes.data, None, None, None, None)
        if bd == 10:
            self.lib.svt_av1_apply_zz_based_temporal_filter_planewise_medium_hbd_c(*args, 10)
        else:
            self.lib.svt_av1_apply_zz_based_temporal_filter_planewise_medium_c(*args)
        assert (count == count[0]).all()
        return int(count[0])

    def filter_sb(self, cen, preds, ctl: dict):
        """One SB: cen and each of preds (y [64][64], cb, cr [32][32] or None) -> (the filtered planes,
        var32 [refs][4], weights [refs][4][3])."""
        bd, ss, chroma = ctl["bit_depth"], ctl["sub_sampling_shift"], ctl["chroma"]
        hbd, dt, sizes = bd == 10, np.uint16 if bd == 10 else np.uint8, (64, 32, 32)
        fill = lambda t: [np.ascontiguousarray(a if a is not None else np.zeros((s, s), dt), dt)  # noqa: E731
                          for a, s in zip(t, sizes)]
        ptr = lambda a: (C.c_void_p * 3)(*[x.ctypes.data for x in a])  # noqa: E731
        at = lambda arr, off: arr.ctypes.data + arr.itemsize * off  # noqa: E731
        self.field("tf_chroma", np.uint8)[0] = chroma
        self.field("tf_decay_factor_fp16", np.uint32, 3)[:] = ctl["tf_decay_factor_fp16"]
        self.field("tf_32x32_block_split_flag", np.int32, 4)[:] = 0
        src = fill(cen)
        accum = [np.zeros(s * s, np.uint32) for s in sizes]
        count = [np.zeros(s * s, np.uint16) for s in sizes]
        central = self.lib.svt_aom_apply_filtering_central_highbd_c if hbd else self.lib.svt_aom_apply_filtering_central_c
        central(self.me.ctypes.data, self.desc.ctypes.data, ptr(src), ptr(accum), ptr(count), 64, 64, 1, 1)
        var32 = np.zeros((len(preds), 4), np.uint32)
        weights = np.zeros((len(preds), 4, 3), np.uint32)
        for r, pred in enumerate(preds):
            pre = fill(pred)
            before = [c.copy() for c in count]
            for i in range(4):  # (:3725-3767)
                y, x = 32 * (i >> 1), 32 * (i & 1)
                var32[r, i] = self.variance32(pre[0][y:y + 32, x:x + 32], src[0][y:y + 32, x:x + 32], ss, bd)
            self.field("tf_32x32_block_error", np.uint64, 4)[:] = var32[r]
            for row in range(2):  # (:3769-3795), apply_filtering_block_plane_wise (:1411-1493)
                for col in range(2):
                    self.field("tf_block_row", np.int32)[0], self.field("tf_block_col", np.int32)[0] = row, col
                    o, oc = row * 32 * 64 + col * 32, row * 16 * 32 + col * 16
                    args = (self.me.ctypes.data, at(pre[0], o), 64, at(pre[1], oc), at(pre[2], oc), 32, 32, 32, 1, 1,
                            at(accum[0], o), at(count[0], o), at(accum[1], oc), at(count[1], oc), at(accum[2], oc),
                            at(count[2], oc))
                    if hbd:
                        self.lib.svt_av1_apply_zz_based_temporal_filter_planewise_medium_hbd_c(*args, bd)
                    else:
                        self.lib.svt_av1_apply_zz_based_temporal_filter_planewise_medium_c(*args)
            for p, s in enumerate(sizes[:3 if chroma else 1]):
                d = (count[p] - before[p]).reshape(s, s)
                for i in range(4):
                    q = d[(i >> 1) * s // 2:, (i & 1) * s // 2:][:s // 2, :s // 2]
                    assert (q == q[0, 0]).all()
                    weights[r, i, p] = q[0, 0]
        out = [np.zeros((s, s), dt) for s in sizes]
        stride = (C.c_uint32 * 3)(64, 32, 32)
        self.lib.svt_aom_get_final_filtered_pixels_c(self.me.ctypes.data, None if hbd else ptr(out),
                                                     ptr(out) if hbd else None, ptr(accum), ptr(count), stride, 0, 0,
                                                     32, 32, hbd)
        return out, var32, weights

    def check_copy(self, pic, W: int, H: int, bd: int, chroma: int):
        """The reference's predictor at MV (0, 0) returns the co-located block of every SB and plane."""
        for sb_y in range(0, H, 64):
            for sb_x in range(0, W, 64):
                for p in range(3 if chroma else 1):
                    pad, b = (S.PAD_FULL, S.PAD_CHROMA)[p > 0], 64 >> (p > 0)
                    x, y = sb_x >> (p > 0), sb_y >> (p > 0)
                    fn = GF.RefArith.predict if bd == 8 else self.predict16 if p == 0 else self.predict16_uv
                    got = fn(pic[p], pad, b, x, y, 0, 0) if bd == 10 else fn(self, pic[p], pad, b, x, y, 0, 0)
                    assert np.array_equal(got, sb_block(pic, p, sb_x, sb_y)), (sb_x, sb_y, p)


def run_case(case: dict, arith: RefArithLD) -> dict:
    """-> {"y", "cb", "cr", "var32", "weights"} of a case; weights [refs][SBs][4][3] is not stored."""
    ctl = case["controls"]
    W, H = S.align8(case["w"]), S.align8(case["h"])
    pics = case_inputs(case)
    cen, refs = pics[case["centre"]], [pics[r] for r in case["refs"]]
    if case["base"] == PREDICTOR_CASE:
        for ref in refs:
            arith.check_copy(ref, W, H, ctl["bit_depth"], ctl["chroma"])
    wb, hb = (W + 63) // 64, (H + 63) // 64
    dt = np.uint16 if ctl["bit_depth"] == 10 else np.uint8
    planes = [np.zeros((hb * 64 >> (p > 0), wb * 64 >> (p > 0)), dt) for p in range(3)]
    var32 = np.zeros((len(refs), wb * hb, 4), np.uint32)
    weights = np.zeros((len(refs), wb * hb, 4, 3), np.uint32)
    for k in range(wb * hb):
        sb_x, sb_y = 64 * (k % wb), 64 * (k // wb)
        cut = lambda pic: [sb_block(pic, p, sb_x, sb_y) if pic[p] is not None else None for p in range(3)]  # noqa: E731
        out, var32[:, k], weights[:, k] = arith.filter_sb(cut(cen), [cut(r) for r in refs], ctl)
        for p in range(3):
            s = 64 >> (p > 0)
            planes[p][(sb_y >> (p > 0)):(sb_y >> (p > 0)) + s, (sb_x >> (p > 0)):(sb_x >> (p > 0)) + s] = out[p]
    res = {"y": planes[0][:H, :W].copy(), "var32": var32, "weights": weights}
    if ctl["chroma"]:
        res["cb"], res["cr"] = planes[1][:H // 2, :W // 2].copy(), planes[2][:H // 2, :W // 2].copy()
    return res


def coverage_of(case: dict, res: dict, variance32) -> (dict, list):
    """The coverage counts of one case from its inputs, var32 and weights [refs][SBs][4][3];
    variance32(pred, cen, ss, bit depth): the arithmetic that made var32. -> (counts, the sets of weights
    strictly between 0 and 500 by plane)."""
    ctl = case["controls"]
    bd, ss = ctl["bit_depth"], ctl["sub_sampling_shift"]
    W, H = S.align8(case["w"]), S.align8(case["h"])
    pics = case_inputs(case)
    cen = pics[case["centre"]]
    wb = (W + 63) // 64
    cover, between = {k: 0 for k in COVERAGE_KEYS}, [set(), set(), set()]
    wts = res["weights"]
    for p in range(3 if ctl["chroma"] else 1):
        w = wts[..., p]
        cover["w500_" + PLANES[p]] += int((w == 500).sum())
        cover["w0_" + PLANES[p]] += int((w == 0).sum())
        cover["between_" + PLANES[p]] += int(((w > 0) & (w < 500)).sum())
        between[p] |= {int(v) for v in w[(w > 0) & (w < 500)]}
    assert wts.max() <= 500
    for r, rn in enumerate(case["refs"]):
        for k in range(wts.shape[1]):
            c64, p64 = sb_block(cen, 0, 64 * (k % wb), 64 * (k // wb)), sb_block(pics[rn], 0, 64 * (k % wb), 64 * (k // wb))
            for i in range(4):
                y, x = 32 * (i >> 1), 32 * (i & 1)
                cover["quadrant_beyond"] += 64 * (k % wb) + x >= W or 64 * (k // wb) + y >= H
                pq, cq = p64[y:y + 32, x:x + 32], c64[y:y + 32, x:x + 32]
                if bd == 10:
                    sse, total, n = GH.var_parts(pq, cq, ss)
                    cover["var_clamped_to_0"] += sse - total * total // n < 0
                if ss:
                    cover["ss1_odd_rows_unseen"] += variance32(pq, cq, 0, bd) != int(res["var32"][r, k, i])
    return cover, between


# ----------------------------------------------------------------------------
# the weight table
# ----------------------------------------------------------------------------
def weight_tuples() -> np.ndarray:
    """[tuples][3] i8: bit depth, tf_decay_factor_fp16, var32. The first 2 x 113 reach each index of the exp
    table in turn at 8 and at 10 bit (a decay factor of 4 << 10: the index is var32 >> 2 or >> 6); the
    rest are drawn: the decay factors of the cases and their neighbours, variances up to 1 << 27."""
    rng = np.random.default_rng(91)
    rows = [[8, 4 << 10, 4 * i] for i in range(113)] + [[10, 4 << 10, 64 * i] for i in range(113)]
    decays = (0, 1, 1023, 1024, 2047, 2048, MID, MID2, 1 << 20, 0x7FFFFFFF, 0xFFFFFFFF)
    for _ in range(274):
        var = int(rng.choice((0, 3, 4, 63, 64, int(rng.integers(0, 600)), int(rng.integers(0, 1 << 14)),
                              int(rng.integers(0, 1 << 20)), int(rng.integers(0, 1 << 27)))))
        rows.append([int(rng.choice((8, 10))), int(rng.choice(decays + (int(rng.integers(0, 1 << 20)),))), var])
    return np.array(rows, np.int64)


def reference_weights(tuples: np.ndarray, arith: RefArithLD) -> np.ndarray:
    return np.array([arith.zz_weight(int(t[0]), int(t[1]), int(t[2])) for t in tuples], np.uint32)


def main():
    cases, ar = case_dicts(), RefArithLD()
    arrays, cover, per_case, between = {}, {k: 0 for k in COVERAGE_KEYS}, {}, [set(), set(), set()]
    for case in cases:
        res = run_case(case, ar)
        for name in ("y", "cb", "cr", "var32"):
            if name in res:
                arrays[f"{case['id']}.{name}"] = res[name]
        cv, bt = coverage_of(case, res, ar.variance32)
        per_case[case["id"]] = {k: v for k, v in cv.items() if v}
        for k, v in cv.items():
            cover[k] += v
        for p in range(3):
            between[p] |= bt[p]
        print(case["id"], res["y"].shape, per_case[case["id"]], [sorted(b) for b in bt])
    tuples = weight_tuples()
    arrays["weights.in"], arrays["weights.out"] = tuples, reference_weights(tuples, ar)
    for name, b in zip(BETWEEN_DISTINCT, between):
        cover[name] = len(b)
    doc = {"cases": cases, "coverage": cover, "coverage_per_case": per_case}
    with open(os.path.join(HERE, "tfld_cases.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    G.write_npz(os.path.join(HERE, "tfld_cases.npz"), arrays)
    missing = [k for k in COVERAGE_KEYS if cover[k] == 0] + [k for k in BETWEEN_DISTINCT if cover[k] < 3]
    print(cover, os.path.getsize(os.path.join(HERE, "tfld_cases.npz")))
    if missing:
        sys.exit("coverage counts too low: " + ", ".join(missing))


if __name__ == "__main__":
    main()
