"""Generate the TF sub-pel refinement fixtures (tests/golden/tfsp_cases.json, tfsp_cases.npz).

The refinement that follows the TF-ME call (temporal_filtering.c:3177-3336, up to the
first tf_64x64_inter_prediction / tf_32x32_inter_prediction) is made of static
functions of the reference, so the expected values are put together from the pieces
the reference exports:

  * the planes are the reference's own: svtref_build_pyramid (full level, pad 72);
  * the records are the reference's own ME (run_checker(..., "ref") on an ME_MCTF job
    with derive_controls_tf), hand-made records whose MVs point far outside each
    of the four picture edges ("edges"), or the ME's records perturbed from a seed
    kept with the case ("wrap", perturb_records(): MVs beside the winners, MVs and
    search centres 2100 and 4096 pixels away, whose << 3 or * 2 wraps in int16,
    TF-ME early exits, SADs that send tf_use_64x64_pred both ways);
  * the arithmetic is the reference's own: svt_inter_predictor after the reference's
    rtcd setup (its C convolves and its own filter tables) and
    svt_aom_variance{64x64,64x32,32x32,32x16,16x16,16x8,8x8,8x4}_c, reached through
    ctypes in a shared object linked from oracle/_ref/enc/libsvtenc.a (the archive
    __graft_entry__.build() makes) into oracle/_ref/libtfsp_ref.so;
  * the control flow is a RESTATEMENT in Python integers, with the reference's lines:
    the clamp (clamp()), svt_check_position / tf_subpel_search (search_block()), the
    four tf_*_sub_pel_search start MVs and the branches, tf_use_64x64_pred and
    derive_tf_32x32_block_split_flag (refine_sb()). The evaluation of one position is
    handed to it (Side's `evaluate`): the reference's arithmetic above by default;
    tests/tfsp_model.py passes one in numpy and so gets a model of the whole
    refinement that needs nothing from oracle/_ref. The coverage counts are kept by
    the shared flow, whichever evaluator runs.

  tfsp_cases.json   the case list, the control sets (with their lines in enc_handle.c)
                    and the coverage counts of the reference-side run, in total and
                    per case
  tfsp_cases.npz    per case "<id>.rec": the records [refs][SBs] (raw bytes of
                    svtme.REF_RECORD_DTYPE) and "<id>.out": the results [refs][SBs]
                    (svtme.TF_SUBPEL_SB_DTYPE)

Container only (needs oracle/_ref, built by __graft_entry__.build() where the
reference's sources are present). Run from the repository root:
python tests/golden/make_golden_tfsp.py. The output is byte-for-byte reproducible
(fixed archive time stamps, deflate at a fixed level). It fails when a coverage
count is 0.
"""
import ctypes as C
import io
import json
import os
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "svt-av1-mirror_amd"))
sys.path.insert(0, os.path.dirname(HERE))

import svtme as S  # noqa: E402
import tfsp_content  # noqa: E402

INT_MAX = 0x7FFFFFFF
U64_MAX = (1 << 64) - 1

# Control sets: the reference's own TF levels (tf_controls, Source/Lib/Globals/enc_handle.c).
CONTROL_SETS = {
    # tf_level 2, I_SLICE parameters (enc_handle.c:2736-2750): presets M2-M3
    "l2": dict(hme_me_level=1, me_exit_th=0, half_pel_mode=1, quarter_pel_mode=1, eight_pel_mode=1, use_2tap=0,
               sub_sampling_shift=0, enable_8x8_pred=1, use_pred_64x64_only_th=0, subpel_early_exit_th=0,
               pred_error_32x32_th=8 * 32 * 32),
    # tf_level 5, I_SLICE parameters (enc_handle.c:2957-2971): presets M5-M7
    "l5": dict(hme_me_level=2, me_exit_th=0, half_pel_mode=2, quarter_pel_mode=1, eight_pel_mode=0, use_2tap=1,
               sub_sampling_shift=0, enable_8x8_pred=0, use_pred_64x64_only_th=0, subpel_early_exit_th=1,
               pred_error_32x32_th=20 * 32 * 32),
    # tf_level 8, I_SLICE parameters (enc_handle.c:3131-3145): preset M8
    "l8": dict(hme_me_level=2, me_exit_th=16 * 16, half_pel_mode=2, quarter_pel_mode=1, eight_pel_mode=0,
               use_2tap=1, sub_sampling_shift=1, enable_8x8_pred=0, use_pred_64x64_only_th=35,
               subpel_early_exit_th=4, pred_error_32x32_th=U64_MAX),
    # The sets below are named by what they set. Every value is one svtme_tf_subpel accepts and the
    # reference's code handles, but the combinations are not levels of enc_handle.c.
    # no half-pel stage (the quarter-pel stage starts from the full-pel centre), quarter-pel without
    # diagonals, bilinear at 64/32 beside the regular filter at 16/8, 8x8 blocks on 4 kept rows
    "h0_q2_2tap_8x8_ss1": dict(hme_me_level=1, me_exit_th=0, half_pel_mode=0, quarter_pel_mode=2, eight_pel_mode=1,
                               use_2tap=1, sub_sampling_shift=1, enable_8x8_pred=1, use_pred_64x64_only_th=0,
                               subpel_early_exit_th=2, pred_error_32x32_th=0),
    # half-pel mode 3 and quarter-pel mode 3 (both without diagonals), a 64x64-only threshold that
    # is neither 0 nor 35, every 32x32 block refined further
    "h3_q3_th10_e0": dict(hme_me_level=1, me_exit_th=0, half_pel_mode=3, quarter_pel_mode=3, eight_pel_mode=0,
                          use_2tap=0, sub_sampling_shift=0, enable_8x8_pred=1, use_pred_64x64_only_th=10,
                          subpel_early_exit_th=8, pred_error_32x32_th=0),
    # only the eighth-pel stage after the centre; a 64x64-only threshold most SBs pass
    "h0_q0_th200": dict(hme_me_level=2, me_exit_th=0, half_pel_mode=0, quarter_pel_mode=0, eight_pel_mode=1,
                        use_2tap=0, sub_sampling_shift=1, enable_8x8_pred=0, use_pred_64x64_only_th=200,
                        subpel_early_exit_th=4, pred_error_32x32_th=8 * 32 * 32),
}
SUBPEL_FIELDS = ("half_pel_mode", "quarter_pel_mode", "eight_pel_mode", "use_2tap", "sub_sampling_shift",
                 "enable_8x8_pred", "use_pred_64x64_only_th", "subpel_early_exit_th", "pred_error_32x32_th")

TFSP_CASES = [
    # id, content, w, h, control set, centre, references, records ("me", "edges" or "wrap"), seed of "wrap"
    ("frac128_l2", "frac", 128, 128, "l2", 8, [7], "me"),
    ("frac128_l8_w3", "frac", 128, 128, "l8", 8, [7, 9, 6], "me"),
    ("frac128_l5", "frac", 128, 128, "l5", 8, [9], "me"),
    ("frac192_l2", "frac", 192, 136, "l2", 8, [9], "me"),
    ("frac192_l8", "frac", 192, 136, "l8", 8, [6], "me"),
    ("glide128_l2", "glide", 128, 128, "l2", 8, [7], "me"),
    ("same128_l8", "same", 128, 128, "l8", 8, [7], "me"),
    ("same128_l2", "same", 128, 128, "l2", 8, [7], "me"),
    ("flat128_l2", "flat", 128, 128, "l2", 8, [7], "me"),
    ("flat128_l8", "flat", 128, 128, "l8", 8, [7], "me"),
    ("edges128_l2", "frac", 128, 128, "l2", 8, [7], "edges"),
    ("edges192_l8", "frac", 192, 136, "l8", 8, [9], "edges"),
    # records "wrap": the ME records perturbed by perturb_records() from the seed given last
    ("frac72_h0q2_wrap", "frac", 72, 40, "h0_q2_2tap_8x8_ss1", 8, [7], "wrap", 11),  # 2nd SB column: 8 of 64 px
    ("frac200_h3q3_wrap", "frac", 200, 72, "h3_q3_th10_e0", 8, [9], "wrap", 12),  # partial column and row
    ("frac200_h0q0_wrap", "frac", 200, 72, "h0_q0_th200", 8, [7], "wrap", 13),
    ("noise124_h0q2_wrap", "noise", 124, 66, "h0_q2_2tap_8x8_ss1", 8, [7], "wrap", 14),  # not multiples of 8
    ("frac124_h3q3", "frac", 124, 66, "h3_q3_th10_e0", 8, [6], "me"),
    ("noise72_l8_wrap", "noise", 72, 40, "l8", 8, [9], "wrap", 15),
    ("frac72_l2_w5", "frac", 72, 40, "l2", 8, [7, 9, 6, 10, 5], "wrap", 16),  # 5 distinct references
]

# the keys before "exit_mid_stage" are those of the first 12 cases' generation
COVERAGE_KEYS = ("win_centre", "win_half", "win_quarter", "win_eighth", "branch_64_only", "branch_64_chosen",
                 "branch_32", "bypass_32", "split_32", "split_16_to_8", "early_exit", "tf_early_exit",
                 "clamp_left", "clamp_right", "clamp_top", "clamp_bottom",
                 # an early-exit skip in a stage in which an earlier candidate was evaluated
                 "exit_mid_stage",
                 # a position whose mv * 2 leaves int16; a start MV or hme_sc whose << 3 does
                 "wrap_q4", "wrap_start",
                 # a searched block with origin >= W / >= H of the aligned picture
                 "block_beyond_w", "block_beyond_h",
                 # a stage with mode 0 before a stage that evaluates a position; a diagonal the quarter-pel
                 # stage drops (and would have evaluated)
                 "stage_skipped", "diag_dropped_quarter",
                 # e64 * 14 < s32 * 16 holds and e64 >= 2^18 alone sends the SB to the 32x32 branch
                 "e64_ge_2p18",
                 # tf_use_64x64_pred with a negative deviation (C truncation, compared signed)
                 "dev_negative")


def case_dicts():
    return [{"id": c[0], "kind": c[1], "w": c[2], "h": c[3], "controls": c[4], "centre": c[5], "refs": list(c[6]),
             "records": c[7], "seed": c[8] if len(c) > 8 else None} for c in TFSP_CASES]


def subpel_controls(name: str) -> "S.TfSubpelControls":
    return S.TfSubpelControls.from_dict({f: CONTROL_SETS[name][f] for f in SUBPEL_FIELDS})


def case_frames(case: dict) -> dict:
    """{picture number: luma plane} of a case."""
    ts = sorted(set([case["centre"]] + case["refs"]))
    w, h = case["w"], case["h"]
    if case["kind"] == "frac":
        return tfsp_content.fractional_frames(w, h, ts)
    if case["kind"] == "glide":  # one fractional motion for the whole picture
        return tfsp_content.fractional_frames(w, h, ts, one_motion=True)
    if case["kind"] == "same":  # identical pictures: every centre position has variance 0
        base = tfsp_content.fractional_frames(w, h, [0])[0]
        return {t: base.copy() for t in ts}
    if case["kind"] == "flat":  # ties everywhere
        return {t: np.full((h, w), 128, np.uint8) for t in ts}
    if case["kind"] in ("noise", "sat"):  # no MV predicts anything: the largest errors
        return S.test_frames(case["kind"], w, h, ts)
    raise ValueError(case["kind"])


# ----------------------------------------------------------------------------
# the reference's arithmetic
# ----------------------------------------------------------------------------
class SubpelParams(C.Structure):  # inter_prediction.h:55-60
    _fields_ = [("xs", C.c_int32), ("ys", C.c_int32), ("subpel_x", C.c_int32), ("subpel_y", C.c_int32)]


class ConvolveParams(C.Structure):  # definitions.h:572-585
    _fields_ = [("ref", C.c_int32), ("do_average", C.c_int32), ("dst", C.c_void_p), ("dst_stride", C.c_int32),
                ("round_0", C.c_int32), ("round_1", C.c_int32), ("plane", C.c_int32), ("is_compound", C.c_int32),
                ("use_jnt_comp_avg", C.c_int32), ("fwd_offset", C.c_int32), ("bck_offset", C.c_int32),
                ("use_dist_wtd_comp_avg", C.c_int32)]


EIGHTTAP_REGULAR, BILINEAR = 0, 3  # InterpFilter, definitions.h:712-716
VARIANCE_FN = {(64, 0): "svt_aom_variance64x64_c", (64, 1): "svt_aom_variance64x32_c",
               (32, 0): "svt_aom_variance32x32_c", (32, 1): "svt_aom_variance32x16_c",
               (16, 0): "svt_aom_variance16x16_c", (16, 1): "svt_aom_variance16x8_c",
               (8, 0): "svt_aom_variance8x8_c", (8, 1): "svt_aom_variance8x4_c"}
_lib = None


def load_enc():
    """oracle/_ref/libtfsp_ref.so: the reference encoder library's objects (C only), linked whole
    from the archive build() makes; rtcd set up for the C kernels."""
    global _lib
    if _lib is not None:
        return _lib
    ref = os.path.join(ROOT, "oracle", "_ref")
    arc, so = os.path.join(ref, "enc", "libsvtenc.a"), os.path.join(ref, "libtfsp_ref.so")
    if not os.path.exists(arc) and not os.path.exists(so):
        raise RuntimeError("oracle/_ref/enc/libsvtenc.a is missing: run __graft_entry__.build() where the "
                           "reference's sources are present")
    if not os.path.exists(so) or (os.path.exists(arc) and os.path.getmtime(so) < os.path.getmtime(arc)):
        subprocess.run(["gcc", "-shared", "-o", so, "-Wl,--whole-archive", arc, "-Wl,--no-whole-archive",
                        "-lpthread", "-lm"], check=True)
    lib = C.CDLL(so)
    lib.svt_aom_setup_common_rtcd_internal.argtypes = [C.c_uint64]
    lib.svt_aom_setup_rtcd_internal.argtypes = [C.c_uint64]
    lib.svt_aom_setup_common_rtcd_internal(0)  # EbCpuFlags 0: the C kernels
    lib.svt_aom_setup_rtcd_internal(0)
    lib.svt_aom_asm_set_convolve_asm_table.argtypes = []
    lib.svt_aom_asm_set_convolve_asm_table()  # svt_aom_convolve[][][] from the rtcd pointers
    lib.svt_inter_predictor.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(SubpelParams),
                                        C.c_void_p, C.c_int32, C.c_int32, C.POINTER(ConvolveParams), C.c_uint32,
                                        C.c_int32]
    lib.svt_inter_predictor.restype = None
    for name in VARIANCE_FN.values():
        fn = getattr(lib, name)
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]
        fn.restype = C.c_uint32
    _lib = lib
    return lib


def i16(v: int) -> int:
    """The value of (int16_t)v."""
    return (int(v) + 0x8000) % 0x10000 - 0x8000


def clamp(mv: int, pu: int, b: int, dim: int):
    """One axis of clamp_mv_to_umv_border_sb (enc_inter_prediction.c:28-48, ss = 0) for a block of
    size b at pu of an aligned picture of size dim: -> (q4 MV, clamped low, clamped high).
    mb_to_*_edge as temporal_filtering.c:1858-1861 set them from mi_rows / mi_cols."""
    q4 = i16(mv * 2)  # (int16_t)(mv * (1 << (1 - ss)))
    spel = (4 + b) << 4  # (AOM_INTERP_EXTEND + bw) << SUBPEL_BITS
    lo = -(pu * 8) * 2 - spel
    hi = (dim - b - pu) * 8 * 2 + spel - 16  # spel_right = spel_left - SUBPEL_SHIFTS
    return (lo if q4 < lo else hi if q4 > hi else q4), q4 < lo, q4 > hi


def wraps_i16(v: int) -> bool:
    return i16(v) != int(v)


def reference_distortion(side: "Side", b: int, px: int, py: int, qx: int, qy: int, bil: bool, centre: bool) -> int:
    """The reference-backed position evaluator (Side's default): svt_check_position's distortion
    (temporal_filtering.c:1581-1636) at the clamped q4 MV: svt_aom_simple_luma_unipred ->
    tf_inter_predictor (enc_inter_prediction.c:3166-3221, 3347-3402), then the variance of the rows
    sub_sampling_shift keeps, << shift."""
    ss = side.ctl["sub_sampling_shift"]
    # compute_subpel_params (enc_inter_prediction.c:3154-3163)
    sp = SubpelParams(1 << 10, 1 << 10, (qx & 15) << 6, (qy & 15) << 6)
    pos_x, pos_y = px + (qx >> 4), py + (qy >> 4)
    # get_conv_params_no_round(0, 0, 0, tmp, 128, 0, 8): round_0 = 3, round_1 = 2 * FILTER_BITS - round_0
    cp = ConvolveParams(0, 0, side.tmp.ctypes.data, 128, 3, 11, 0, 0, 0, 0, 0, 0)
    f = BILINEAR if bil else EIGHTTAP_REGULAR
    shift = ss if centre else 0  # the prediction is sub-sampled only at xd == yd == 0 (:1603)
    src = side.ref.full.ctypes.data + (side.pad + pos_y) * side.stride + side.pad + pos_x
    lo = (side.pad + pos_y - 3) * side.stride + side.pad + pos_x - 3
    hi = (side.pad + pos_y + b + 4) * side.stride + side.pad + pos_x + b + 4
    assert 0 <= lo and hi <= side.ref.full.size, (pos_x, pos_y, b)
    side.lib.svt_inter_predictor(src, side.stride << shift, side.pred.ctypes.data, 64 << shift, C.byref(sp),
                                 side.sf.ctypes.data, b, b >> shift, C.byref(cp), (f << 16) | f, 0)
    sse = C.c_uint32()
    cptr = side.cen.full.ctypes.data + (side.pad + py) * side.stride + side.pad + px
    var = getattr(side.lib, VARIANCE_FN[(b, ss)])(side.pred.ctypes.data, 64 << ss, cptr, side.stride << ss,
                                                  C.byref(sse))
    return var << ss


class Side:
    """The evaluation of positions on one (centre, reference) pair of planes and the control flow
    around it. The distortion of one position comes from `evaluate(side, b, px, py, qx, qy, bil,
    centre)` (the clamped q4 MV): reference_distortion by default, which needs oracle/_ref; another
    evaluator (tests/tfsp_model.py passes one written in numpy) needs nothing from the reference.
    Everything else, the coverage counts included, is shared by the evaluators."""

    def __init__(self, cen: "S.HostPyramid", ref: "S.HostPyramid", ctl: dict, cover: dict, evaluate=None):
        self.cen, self.ref, self.ctl, self.cover = cen, ref, ctl, cover
        self.W, self.H = cen.width, cen.height
        self.stride, self.pad = cen.full.shape[1], S.PAD_FULL
        if evaluate is None:
            self.lib = load_enc()
            self.pred = np.zeros((64, 64), np.uint8)  # stride BW = 64 (temporal_filtering.c:1924)
            self.tmp = np.zeros(128 * 128, np.uint16)
            self.sf = np.zeros(256, np.uint8)  # the identity ScaleFactors: not read on the unscaled path
            evaluate = reference_distortion
        self.evaluate = evaluate
        self.positions = self.macs = 0

    def dist(self, b: int, px: int, py: int, mvx: int, mvy: int, bil: bool, centre: bool) -> int:
        """The distortion of one position: the clamp of the MV (counted), then the evaluator."""
        ss = self.ctl["sub_sampling_shift"]
        qx, cl, cr = clamp(mvx, px, b, self.W)
        qy, ct, cb = clamp(mvy, py, b, self.H)
        for key, hit in (("clamp_left", cl), ("clamp_right", cr), ("clamp_top", ct), ("clamp_bottom", cb)):
            self.cover[key] += bool(hit)
        self.cover["wrap_q4"] += wraps_i16(mvx * 2) or wraps_i16(mvy * 2)
        d = self.evaluate(self, b, px, py, qx, qy, bil, centre)
        self.positions += 1
        # multiply-adds by the non-zero taps (6 regular, 2 bilinear) over the rows kept (scripts/tf_subpel_bench.py)
        taps, fx, fy, rows = 2 if bil else 6, qx & 15, qy & 15, b >> ss
        self.macs += taps * b * ((b + 7 + rows) if fx and fy else rows if fx or fy else 0)
        return d

    def search_block(self, b: int, px: int, py: int, mvx: int, mvy: int, bil: bool):
        """tf_subpel_search (temporal_filtering.c:1669-1790) -> (best distortion, MV x, MV y)."""
        best, bx, by = INT_MAX, mvx, mvy
        th = self.ctl["subpel_early_exit_th"]
        won = "win_centre"
        self.cover["block_beyond_w"] += px >= self.W
        self.cover["block_beyond_h"] += py >= self.H
        stages = ((0, 0, "win_centre"), (self.ctl["half_pel_mode"], 4, "win_half"),
                  (self.ctl["quarter_pel_mode"], 2, "win_quarter"), (self.ctl["eight_pel_mode"], 1, "win_eighth"))
        skipped = 0  # stages with mode 0 so far: counted once a later stage evaluates a position
        for si, (mode, step, key) in enumerate(stages):
            if si and not mode:
                skipped += 1
                continue
            cx, cy = bx, by
            offsets = [(0, 0)] if si == 0 else [(i, j) for i in (-step, 0, step) for j in (-step, 0, step)
                                                 if (i, j) != (0, 0)]
            evaluated = 0  # positions of this stage
            for xd, yd in offsets:  # x offset outer, y offset inner (:1703-1704)
                m = self.ctl["half_pel_mode"] if si == 0 else mode
                diag = m >= 2 and xd != 0 and yd != 0  # svt_check_position (:1567)
                if best == 0:  # (:1571)
                    continue
                if th and best < b * b * th:  # (:1575-1578), 8-bit
                    if not diag:
                        self.cover["early_exit"] += 1
                        self.cover["exit_mid_stage"] += evaluated > 0
                    continue
                if diag:  # checked first in the reference; a skip either way
                    self.cover["diag_dropped_quarter"] += si == 2
                    continue
                self.cover["stage_skipped"] += skipped
                skipped = 0
                d = self.dist(b, px, py, i16(cx + xd), i16(cy + yd), bil, si == 0)
                evaluated += 1
                if d < best:  # strict (:1657)
                    best, bx, by, won = d, i16(cx + xd), i16(cy + yd), key
        self.cover[won] += 1
        return best, bx, by

    def start_mv(self, v: int):
        """(_MVXT, _MVYT) of a packed full-pel MV, << 3 into the int16 fields (:1980-1981)."""
        x, y = i16(v & 0xFFFF), i16(v >> 16)
        self.cover["wrap_start"] += wraps_i16(x << 3) or wraps_i16(y << 3)
        return i16(x << 3), i16(y << 3)


def block_xy(level: int, k: int):
    """Origin inside the SB of block k of a level (1: 32x32, 2: 16x16, 3: 8x8) in the reference's
    index order idx_32x32 (* 4 + idx_16x16 (* 4 + idx_8x8)): each index is (row << 1) | col of its
    quadrant (idx_32x32_to_idx_16x16 / _8x8 with subblock_xy_*, temporal_filtering.c:43-78)."""
    x = y = 0
    for j in range(level):
        pair = (k >> (2 * (level - 1 - j))) & 3
        x += (pair & 1) * (32 >> j)
        y += (pair >> 1) * (32 >> j)
    return x, y


def refine_sb(side: Side, rec, sb_x: int, sb_y: int) -> np.ndarray:
    """temporal_filtering.c:3177-3336 for one (reference, SB) -> one TF_SUBPEL_SB_DTYPE result."""
    ctl, cover = side.ctl, side.cover
    out = np.zeros((), S.TF_SUBPEL_SB_DTYPE)
    out["error"][:] = INT_MAX
    sad, mvs = rec["best_sad"], rec["best_mv"]
    th64 = 255 if rec["tf_early_exit"] else ctl["use_pred_64x64_only_th"]  # motion_estimation.c:3111
    cover["tf_early_exit"] += bool(rec["tf_early_exit"])

    def put(idx, res):
        out["error"][idx], out["mv"]["x"][idx], out["mv"]["y"][idx] = res

    def use_64x64_pred():  # tf_use_64x64_pred (:2675-2689): C division truncates toward zero
        d32 = (int(sad[1]) + int(sad[2]) + int(sad[3]) + int(sad[4])) & 0xFFFFFFFF
        a, c = max(int(sad[0]), 1), max(d32, 1)
        num = (a - c) * 100
        dev = abs(num) // c * (1 if num >= 0 else -1)
        cover["dev_negative"] += dev < 0
        return dev < th64

    # tf_64x64_sub_pel_search: from hme_sc when the threshold is ~0 (:1866-1869)
    if th64 == 255:
        hx, hy = int(rec["hme_sc_x"]) << 3, int(rec["hme_sc_y"]) << 3
        cover["wrap_start"] += wraps_i16(hx) or wraps_i16(hy)
        sx, sy = i16(hx), i16(hy)
    else:
        sx, sy = side.start_mv(int(mvs[0]))
    bil = bool(ctl["use_2tap"])
    only64 = bool(th64) and (th64 == 255 or use_64x64_pred())  # (:3177-3179)
    r64 = side.search_block(64, sb_x, sb_y, sx, sy, bil)
    put(0, r64)
    if only64:
        branch = S.TFSP_64_ONLY
        cover["branch_64_only"] += 1
    else:
        r32 = []
        for i in range(4):  # tf_32x32_sub_pel_search (:1957-2011)
            bx, by = block_xy(1, i)
            r32.append(side.search_block(32, sb_x + bx, sb_y + by, *side.start_mv(int(mvs[1 + i])), bil))
        s32 = sum(r[0] for r in r32)
        cover["e64_ge_2p18"] += r64[0] * 14 < s32 * 16 and r64[0] >= (1 << 18)
        if r64[0] * 14 < s32 * 16 and r64[0] < (1 << 18):  # (:3265-3266)
            branch = S.TFSP_64_CHOSEN
            cover["branch_64_chosen"] += 1
        else:
            branch = S.TFSP_32
            cover["branch_32"] += 1
            for i in range(4):
                put(1 + i, r32[i])
                if r32[i][0] < ctl["pred_error_32x32_th"]:  # (:3293-3296)
                    cover["bypass_32"] += 1
                    continue
                e16 = []
                for j in range(4):  # tf_16x16_sub_pel_search (:2073-2131): always the regular filter
                    bx, by = block_xy(2, i * 4 + j)
                    r = side.search_block(16, sb_x + bx, sb_y + by, *side.start_mv(int(mvs[5 + i * 4 + j])), False)
                    put(5 + i * 4 + j, r)
                    e16.append(r[0])
                e8 = []
                if ctl["enable_8x8_pred"]:  # tf_8x8_sub_pel_search (:2190-2250)
                    for j in range(16):
                        bx, by = block_xy(3, i * 16 + j)
                        r = side.search_block(8, sb_x + bx, sb_y + by, *side.start_mv(int(mvs[21 + i * 16 + j])), False)
                        put(21 + i * 16 + j, r)
                        e8.append(r[0])
                # derive_tf_32x32_block_split_flag (:236-285)
                total = 0
                for j in range(4):
                    e = e16[j]
                    if ctl["enable_8x8_pred"]:
                        s8 = sum(e8[4 * j:4 * j + 4])
                        if not e * 8 < s8 * 16:
                            out["split_16x16"][i][j] = 1
                            out["error"][5 + i * 4 + j] = s8
                            e = s8
                            cover["split_16_to_8"] += 1
                    total += e
                assert total * 16 < 1 << 31 and r32[i][0] * 14 < 1 << 31  # the reference's int arithmetic holds
                if not r32[i][0] * 14 < total * 16:
                    out["split_32x32"][i] = 1
                    cover["split_32"] += 1
    if branch != S.TFSP_32:  # convert_64x64_info_to_32x32_info (:2696-2712)
        for i in range(4):
            put(1 + i, (INT_MAX, r64[1], r64[2]))
    out["branch"] = branch
    return out


# ----------------------------------------------------------------------------
# records
# ----------------------------------------------------------------------------
def me_job(case: dict, cs: dict, ref: int, base: int = 0) -> "S.Job":
    """The TF-ME job of one reference of a case (picture numbers offset by `base`)."""
    w, h = case["w"], case["h"]
    ctrl = S.derive_controls_tf(cs["hme_me_level"], 0, 35, S.input_resolution_of(w, h))
    return S.case_job(ctrl, w, h, base + case["centre"], (base + ref,), (), 0, me_type=S.ME_MCTF,
                      tf_me_exit_th=cs["me_exit_th"])


def me_records(case: dict, pyr: dict, checker: str = "ref") -> np.ndarray:
    """[refs][SBs] slot 0 of the reference's (or the oracle's) TF-ME job of each reference."""
    cs = case["controls"] if isinstance(case["controls"], dict) else CONTROL_SETS[case["controls"]]
    out = []
    for r in case["refs"]:
        recs, _ = S.run_checker(me_job(case, cs, r), pyr[case["centre"]], {(0, 0): pyr[r]}, checker,
                                with_sb_results=False)
        out.append(recs[:, 0])
    return np.stack(out)


def perturb_records(recs: np.ndarray, seed: int) -> np.ndarray:
    """A copy of ME records [refs][SBs] moved off the ME's winners: every PU's MV by up to 2 pixels
    per axis; a sixth of the (reference, SB)s, MVs and hme_sc alike, by +-2100 pixels (<< 3 fits
    int16, * 2 after it does not) or by 4096 pixels (<< 3 wraps to the opposite sign) on one axis
    or both; a fifth with tf_early_exit set; half with random best_sad[0..4], so that
    tf_use_64x64_pred goes both ways and its deviation takes both signs."""
    rng = np.random.default_rng(seed)
    out = recs.copy()
    for idx in np.ndindex(out.shape):
        rec = out[idx]
        mv = rec["best_mv"].astype(np.int64)
        x, y = (mv & 0xFFFF) + rng.integers(-2, 3, S.PU_COUNT), (mv >> 16) + rng.integers(-2, 3, S.PU_COUNT)
        hx, hy = int(rec["hme_sc_x"]), int(rec["hme_sc_y"])
        if rng.integers(0, 6) == 0:
            far = (-2100, 2100, 4096, -4096)
            fx, fy = [(int(rng.choice(far)), 0), (0, int(rng.choice(far))),
                      (int(rng.choice(far)), int(rng.choice(far)))][int(rng.integers(0, 3))]
            x, y, hx, hy = x + fx, y + fy, hx + fx, hy + fy
        rec["best_mv"] = (((y & 0xFFFF) << 16) | (x & 0xFFFF)).astype(np.uint32)
        rec["hme_sc_x"], rec["hme_sc_y"] = i16(hx), i16(hy)
        if rng.integers(0, 5) == 0:
            rec["tf_early_exit"] = 1
        if rng.integers(0, 2):
            rec["best_sad"][0] = rng.integers(0, 20000)
            rec["best_sad"][1:5] = rng.integers(0, 5000, 4)
        out[idx] = rec
    return out


def edge_records(case: dict) -> np.ndarray:
    """Hand-made records: SB k points every block far outside edge k % 4 (left, right, top, bottom),
    some blocks a little less far, with SADs that take the 32x32 path; one SB per edge also takes
    the TF-ME early exit from a far search centre."""
    w, h = S.align8(case["w"]), S.align8(case["h"])
    sbs = S.sb_total(w, h)
    recs = np.zeros((len(case["refs"]), sbs), S.REF_RECORD_DTYPE)
    far = [(-(w + 200), 3), (w + 200, -2), (5, -(h + 200)), (-4, h + 200)]
    for r in range(recs.shape[0]):
        for k in range(sbs):
            fx, fy = far[k % 4]
            for pu in range(S.PU_COUNT):
                x, y = fx + (pu % 3) * 7 * (1 if fx < 0 else -1 if abs(fx) > 100 else 0), \
                    fy + (pu % 5) * 9 * (1 if fy < 0 else -1 if abs(fy) > 100 else 0)
                recs[r, k]["best_mv"][pu] = ((y & 0xFFFF) << 16) | (x & 0xFFFF)
            recs[r, k]["best_sad"][:] = 1000
            recs[r, k]["best_sad"][0] = 9000  # 64x64 far above the 32x32 sum: not 64x64-only by threshold
            recs[r, k]["hme_sc_x"], recs[r, k]["hme_sc_y"] = fx, fy
            recs[r, k]["searched"] = recs[r, k]["do_ref"] = 1
            recs[r, k]["tf_early_exit"] = 1 if k >= 4 and k % 4 == 0 else 0
    return recs


def generate_case(case: dict, cover: dict = None):
    """-> (records [refs][SBs], results [refs][SBs]) from the reference; `cover` accumulates the counts."""
    cover = {k: 0 for k in COVERAGE_KEYS} if cover is None else cover
    pyr = {t: S.build_host_pyramid(f, "ref") for t, f in case_frames(case).items()}
    recs = edge_records(case) if case["records"] == "edges" else me_records(case, pyr)
    if case["records"] == "wrap":
        recs = perturb_records(recs, case["seed"])
    ctl = CONTROL_SETS[case["controls"]]
    return recs, refine_window(pyr[case["centre"]], [pyr[r] for r in case["refs"]], ctl, recs, cover)


def refine_window(cen: "S.HostPyramid", refs: list, ctl: dict, recs: np.ndarray, cover: dict,
                  evaluate=None) -> np.ndarray:
    """The results [refs][SBs] of a window; `evaluate` as Side takes it."""
    wb = (cen.width + 63) // 64
    out = np.zeros(recs.shape, S.TF_SUBPEL_SB_DTYPE)
    for r, ref in enumerate(refs):
        side = Side(cen, ref, ctl, cover, evaluate)
        for k in range(recs.shape[1]):
            out[r, k] = refine_sb(side, recs[r, k], 64 * (k % wb), 64 * (k // wb))
    return out


def write_npz(path: str, arrays: dict):
    """A deflated .npz with fixed time stamps (np.savez stamps the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    cases = case_dicts()
    arrays, cover, per_case = {}, {k: 0 for k in COVERAGE_KEYS}, {}
    for case in cases:
        before = dict(cover)
        recs, out = generate_case(case, cover)
        arrays[case["id"] + ".rec"] = recs
        arrays[case["id"] + ".out"] = out
        per_case[case["id"]] = {k: cover[k] - before[k] for k in COVERAGE_KEYS if cover[k] != before[k]}
        print(case["id"], out.shape, per_case[case["id"]])
    doc = {"controls": {n: {k: (v if v != U64_MAX else "UINT64_MAX") for k, v in c.items()}
                        for n, c in CONTROL_SETS.items()},
           "cases": cases, "coverage": cover, "coverage_per_case": per_case}
    with open(os.path.join(HERE, "tfsp_cases.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    write_npz(os.path.join(HERE, "tfsp_cases.npz"), arrays)
    missing = [k for k in COVERAGE_KEYS if cover[k] == 0]
    if missing:
        sys.exit("coverage counts of 0: " + ", ".join(missing))


if __name__ == "__main__":
    main()
