"""Generate the 10-bit TF chroma fixtures (tests/golden/tffhc_cases.json, tffhc_cases.npz).

Temporal filtering with is_highbd and tf_chroma set, 4:2:0, use_zz_based_filter == 0,
use_8bit_subpel == 1: what svtme_tf_filter_yuv_10bit computes. The expected values come
from the reference's own functions in oracle/_ref/libtfsp_ref.so:

  * svt_highbd_inter_predictor with MULTITAP_SHARP and bd 10 on the 16-bit luma planes and,
    at the chroma block sizes 32, 16, 8 and 4, on the 16-bit chroma planes (the reference
    picks sub_pel_filters_4 at 4x4 itself);
  * svt_aom_highbd_10_variance32x32_c / 32x16_c (make_golden_tffh.RefArithH);
  * svt_aom_apply_filtering_central_highbd_c,
    svt_av1_apply_temporal_filter_planewise_medium_hbd_c with MeContext.tf_chroma = 1 and the
    three decay factors, and svt_aom_get_final_filtered_pixels_c with is_highbd, on the
    three planes of each SB.

The glue between them is make_golden_tffc's (filter_window_yuv, clamp_uv), shared as it
stands. It keeps predictions and planes in 8-bit arrays of its own, so the arithmetic handed
to it (HbdGlueUV, make_golden_tffh.HbdGlue with the two chroma planes) keeps the 16-bit
arrays beside them and filter_window_yuv_hbd puts the 16-bit planes together.
tests/tffhc_model.py passes the same glue an arithmetic in numpy and Python integers.

Inputs: the five cases of make_golden_tffc.CASES with their sizes, seeds, random_subpel and
controls; each luma and chroma frame is (frame8 << 2) | two seeded random bits. One clip
case is added at 64x64 whose chroma holds runs of 0 and 1023 beside mid-grey.

  tffhc_cases.json  the case list, the controls, the coverage counts
  tffhc_cases.npz   per case "<id>.y" [H][W], "<id>.cb", "<id>.cr" [H/2][W/2] u16,
                    "<id>.err32" [refs][SBs][4], "<id>.weights_uv" [refs][SBs][2][16] u32,
                    "<id>.subpel" [refs][SBs]; "weights.in" [tuples][24] i8
                    (make_golden_tff's 19 columns with the luma SSEs of 10-bit samples, the
                    chroma decay factor, the four chroma 8x8 SSEs) and "weights.out"
                    [tuples][4] u32, the chroma weights

Container only (needs oracle/_ref). Run from the repository root:
python tests/golden/make_golden_tffhc.py. The output is byte-for-byte reproducible. It fails
when a coverage count is 0.
"""
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "svt-av1-mirror_amd"))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_golden_tff as GF  # noqa: E402
import make_golden_tffc as GC  # noqa: E402
import make_golden_tffh as GH  # noqa: E402
import make_golden_tfsp as G  # noqa: E402
import svtme as S  # noqa: E402

PAD = S.PAD_CHROMA
BD = GH.BD
PIX_MAX = GH.PIX_MAX

# the case of this file: id, w, h, centre, references, seed of random_subpel, controls
CLIP_CASE = ("c64_clip", 64, 64, 8, [7, 9], 36,
             dict(tf_decay_factor_fp16=2_000_000, tf_mv_dist_th=64, sub_sampling_shift=0,
                  tf_decay_factor_cb_fp16=2_000_000, tf_decay_factor_cr_fp16=0x7FFFFFFF))

COVERAGE_KEYS = GC.COVERAGE_KEYS + ("clip_low_uv", "clip_high_uv")  # a chroma sample below 0 / above 1023 before the clip
COUNTED_KEYS = COVERAGE_KEYS + ("clip_low", "clip_high", "var_clamped_to_0")  # luma's: counted, not required


def case_dicts():
    c = CLIP_CASE
    return GC.case_dicts() + [{"id": c[0], "kind": "clip", "w": c[1], "h": c[2], "centre": c[3], "refs": list(c[4]),
                               "subpel": "random", "seed": c[5], "controls": dict(c[6])}]


def chroma_frames8(case: dict) -> dict:
    """{picture number: (cb, cr)} in 8 bits: make_golden_tffc's; in the clip case make_golden_tffh's cells
    at the chroma size, Cr a picture ahead of Cb."""
    if case["kind"] != "clip":
        return GC.chroma_frames(case)
    ts = sorted(set([case["centre"]] + case["refs"]))
    cw, ch = (case["w"] + 1) >> 1, (case["h"] + 1) >> 1
    cb, cr = GH.clip_frames(cw, ch, ts), GH.clip_frames(cw, ch, [t + 1 for t in ts])
    return {t: (cb[t], cr[t + 1]) for t in ts}


def chroma_frames10(case: dict) -> dict:
    """{picture number: (cb, cr) u16}: (frame8 << 2) | two seeded random bits; in the clip case 0 stays 0 and
    255 becomes 1023."""
    out = {}
    for t, planes in chroma_frames8(case).items():
        pair = []
        for p, f in enumerate(planes):
            rng = np.random.default_rng([zlib.crc32(case["id"].encode()), t, 1 + p])
            lsb = rng.integers(0, 4, f.shape, dtype=np.uint16)
            if case["kind"] == "clip":
                lsb = np.where(f == 0, 0, np.where(f == 255, 3, lsb)).astype(np.uint16)
            pair.append((f.astype(np.uint16) << 2) | lsb)
        out[t] = tuple(pair)
    return out


def pad_chroma16(plane: np.ndarray, W: int, H: int) -> np.ndarray:
    """What svtme_picture_attach_chroma_10bit leaves (make_golden_tffc.pad_chroma on 16-bit samples): the
    true plane replicated to W/2 x H/2 of the aligned picture, then margins of PAD replicated samples. The
    reference's packed planes hold the same inside its own 36 (svt_aom_pack_highbd_pic of the 8-bit planes,
    padded by pad_input_picture and svt_aom_generate_padding, and of the 2-bit planes, padded by
    pad_2b_compressed_input_picture and svt_aom_generate_padding_compressed_10bit, which repeat the edge
    sample's two bits)."""
    assert plane.dtype == np.uint16
    return GC.pad_chroma(plane, W, H)


class HbdGlueUV(GH.HbdGlue):
    """Runs make_golden_tffc.filter_window_yuv on 16-bit samples: make_golden_tffh.HbdGlue for luma (the
    calls with luma's padding) and the same bookkeeping for the two chroma planes, which the glue
    predicts Cb then Cr after each luma block. A subclass gives predict16, var32_16, predict16_uv and
    filter_sb_yuv16."""

    def begin(self, cover: dict):
        super().begin(cover)
        self.preds_uv, self.cur_uv, self.filled_uv, self.plane = [], None, 0, 0

    def predict(self, full, pad, b, px, py, qx, qy) -> np.ndarray:
        if pad == S.PAD_FULL:
            return super().predict(full, pad, b, px, py, qx, qy)
        assert pad == PAD
        if self.cur_uv is None:
            self.cur_uv, self.filled_uv = [np.zeros((32, 32), np.uint16), np.zeros((32, 32), np.uint16)], 0
        p = self.predict16_uv(full, pad, b, px, py, qx, qy)
        self.cur_uv[self.plane][py % 32:py % 32 + b, px % 32:px % 32 + b] = p
        self.plane ^= 1
        self.filled_uv += b * b
        if self.filled_uv == 2 * 32 * 32:  # the chroma blocks of a (reference, SB) tile its two 32x32 blocks
            self.preds_uv.append(tuple(self.cur_uv))
            self.cur_uv = None
        return (p & 0xFF).astype(np.uint8)

    def filter_sb_yuv(self, cen64, cen_cb, cen_cr, preds, metas, ctl):
        assert len(self.preds) == len(self.preds_uv) == len(preds) and self.cur is None and self.cur_uv is None
        preds16 = [(y, uv[0], uv[1]) for y, uv in zip(self.preds, self.preds_uv)]
        out, weights = self.filter_sb_yuv16(cen64, cen_cb, cen_cr, preds16, metas, ctl)
        self.outs.append(out)
        self.preds, self.preds_uv = [], []
        return [(o & 0xFF).astype(np.uint8) for o in out], weights


def filter_window_yuv_hbd(cen, refs: list, cen_uv, refs_uv: list, ctl: dict, subpel: np.ndarray, arith: HbdGlueUV,
                          cover: dict) -> dict:
    """make_golden_tffc.filter_window_yuv on 16-bit pictures (make_golden_tffh.host_picture, pad_chroma16)
    -> its dict with y [H][W], cb and cr [H/2][W/2] in u16."""
    arith.begin(cover)
    res = GC.filter_window_yuv(cen, refs, cen_uv, refs_uv, ctl, subpel, arith, cover)
    W, H = cen.width, cen.height
    wb, hb = (W + 63) // 64, (H + 63) // 64
    y, uv = np.zeros((hb * 64, wb * 64), np.uint16), np.zeros((2, hb * 32, wb * 32), np.uint16)
    for k, out in enumerate(arith.outs):
        sy, sx = 64 * (k // wb), 64 * (k % wb)
        y[sy:sy + 64, sx:sx + 64] = out[0]
        for p in range(2):
            uv[p, sy // 2:sy // 2 + 32, sx // 2:sx // 2 + 32] = out[1 + p]
    res.update(y=y[:H, :W].copy(), cb=uv[0, :H // 2, :W // 2].copy(), cr=uv[1, :H // 2, :W // 2].copy())
    return res


# ----------------------------------------------------------------------------
# the reference's arithmetic
# ----------------------------------------------------------------------------
class RefArithUVH(HbdGlueUV, GH.RefArithH):
    """The reference's own high-bit-depth arithmetic with MeContext.tf_chroma set."""

    def __init__(self):
        GH.RefArithH.__init__(self)
        self.field("tf_chroma", np.uint8)[0] = 1

    def predict16_uv(self, full, pad, b, px, py, qx, qy) -> np.ndarray:
        import tffhc_model as MHC  # the clip counts are the model's: the reference returns clipped samples only

        sp = G.SubpelParams(1 << 10, 1 << 10, (qx & 15) << 6, (qy & 15) << 6)
        pos_x, pos_y = px + (qx >> 4), py + (qy >> 4)
        stride = full.shape[1]
        assert full.dtype == np.uint16 and pad + pos_y - 3 >= 0 and pad + pos_x - 3 >= 0 \
            and pad + pos_y + b + 4 <= full.shape[0] and pad + pos_x + b + 4 <= stride, (pos_x, pos_y, b)
        cp = G.ConvolveParams(0, 0, self.tmp.ctypes.data, 128, 3, 11, 0, 0, 0, 0, 0, 0)  # get_conv_params_no_round, bd 10
        pred = np.zeros((b, b), np.uint16)
        self.lib.svt_highbd_inter_predictor(full.ctypes.data + 2 * ((pad + pos_y) * stride + pad + pos_x), stride,
                                            pred.ctypes.data, b, C.byref(sp), self.sf.ctypes.data, b, b, C.byref(cp),
                                            (GF.MULTITAP_SHARP << 16) | GF.MULTITAP_SHARP, 0, BD)
        raw = MHC.predict_unclipped_uv(full, pad, b, px, py, qx, qy)
        assert np.array_equal(np.clip(raw, 0, PIX_MAX), pred)
        self.cover["clip_low_uv"] += int((raw < 0).sum())
        self.cover["clip_high_uv"] += int((raw > PIX_MAX).sum())
        return pred

    def apply32_yuv(self, src, pre, offs, accum, count):
        """One 32x32 luma block and its two 16x16 chroma blocks through the reference's function; src / pre:
        (y stride 64, cb, cr stride 32) u16 arrays, offs: the block's (luma, chroma) sample offsets."""
        o, oc = offs
        a = lambda arr, off, size: arr.ctypes.data + size * off  # noqa: E731
        self.lib.svt_av1_apply_temporal_filter_planewise_medium_hbd_c(
            self.me.ctypes.data, a(src[0], o, 2), 64, a(pre[0], o, 2), 64, a(src[1], oc, 2), a(src[2], oc, 2), 32,
            a(pre[1], oc, 2), a(pre[2], oc, 2), 32, 32, 32, 1, 1, a(accum[0], o, 4), a(count[0], o, 2),
            a(accum[1], oc, 4), a(count[1], oc, 2), a(accum[2], oc, 4), a(count[2], oc, 2), BD)

    def filter_sb_yuv16(self, cen64, cen_cb, cen_cr, preds, metas, ctl):
        sizes = (64, 32, 32)
        src = [np.ascontiguousarray(a, np.uint16) for a in (cen64, cen_cb, cen_cr)]
        accum = [np.zeros(s * s, np.uint32) for s in sizes]
        count = [np.zeros(s * s, np.uint16) for s in sizes]
        ptr = lambda a: (C.c_void_p * 3)(*[x.ctypes.data for x in a])  # noqa: E731
        # src_stride_ch = stride_y >> ss_x = 32 (:395-396)
        self.lib.svt_aom_apply_filtering_central_highbd_c(self.me.ctypes.data, self.desc.ctypes.data, ptr(src),
                                                          ptr(accum), ptr(count), 64, 64, 1, 1)
        decay = self.field("tf_decay_factor_fp16", np.uint32, 3)
        weights = [np.zeros((len(preds), 16), np.uint32) for _ in sizes]
        for r, (pred, meta) in enumerate(zip(preds, metas)):
            pred = [np.ascontiguousarray(p, np.uint16) for p in pred]
            before = [c.copy() for c in count]
            for row in range(2):  # (:3353-3375), apply_filtering_block_plane_wise (:1411-1493)
                for col in range(2):
                    self.set_block(meta[col + 2 * row], row, col, ctl)
                    decay[1], decay[2] = ctl["tf_decay_factor_cb_fp16"], ctl["tf_decay_factor_cr_fp16"]
                    self.apply32_yuv(src, pred, (row * 32 * 64 + col * 32, row * 16 * 32 + col * 16), accum, count)
            for p, s in enumerate(sizes):
                weights[p][r] = GC.quarter_weights((count[p] - before[p]).reshape(s, s), s)
        out = [np.zeros((s, s), np.uint16) for s in sizes]
        stride = (C.c_uint32 * 3)(64, 32, 32)
        self.lib.svt_aom_get_final_filtered_pixels_c(self.me.ctypes.data, None, ptr(out), ptr(accum), ptr(count), stride,
                                                     0, 0, 32, 32, True)
        return out, weights


# ----------------------------------------------------------------------------
# the fixture "weights": chroma weight tuples through the reference's high-bit-depth filter function
# ----------------------------------------------------------------------------
WEIGHT_COLS = GF.WEIGHT_COLS + 5  # make_golden_tff's 19, the chroma decay factor, 4 x the chroma 8x8 SSE
SSE_MAX_Y = GH.SSE_MAX               # 256 x 1023^2: the luma window error at its maximum
SSE_MAX_C = 64 * PIX_MAX * PIX_MAX   # 64 x 1023^2


def weight_tuples() -> np.ndarray:
    """[tuples][24] i8. The first 113 reach each index of the exp table in turn through the chroma SSE
    alone (split, MV 0, the threshold at its floor, a chroma decay factor of 32 << 10, block error and
    luma SSE 0: the index is ((((sse >> 4) * 4 * 5) / 6) * 5 / 6) >> 3); the next 8 hold both SSEs at their
    maxima on both paths; the rest are drawn, half of them unsplit."""
    rng = np.random.default_rng(79)
    rows = []
    for t in range(113):
        comb = -(-(8 * t * 6) // 5)  # the least window error whose 5 / 6 reaches 8 t
        sse = -(-(comb * 6) // 20) << 4  # the least chroma SSE whose window error reaches it
        rows.append([1, 0, 64] + [0, 0, 0, 0] * 4 + [32 << 10] + [sse] * 4)
    for k in range(8):
        rows.append([k & 1, GF.DECAYS[k % 4], GF.DIST_THS[(k >> 1) % 4]] + [0, 0, 1 << (4 * k), SSE_MAX_Y] * 4 +
                    [GF.DECAYS[(k + 1) % 4]] + [SSE_MAX_C] * 4)
    for k in range(199):
        split = int(rng.integers(0, 2))
        decay_y = int(rng.choice(GF.DECAYS))
        decay_c = int(rng.choice(GF.DECAYS + (1024, 2047, 1 << 20, 3_000_000, 0xFFFFFFFF, int(rng.integers(0, 1 << 32)))))
        th = int(rng.choice(GF.DIST_THS + (1, 9, 10, 11, 100, 200, int(rng.integers(0, 32768)))))
        row, tail = [split, decay_y, th], []
        e32 = int(rng.choice((0, 5, 63, 64, int(rng.integers(0, 1 << 14)), int(rng.integers(0, 1 << 26)), G.INT_MAX)))
        mv32 = None
        for j in range(4):
            kind = int(rng.integers(0, 5))
            mag = (0, 3, 60, 3000, 32767)[kind]
            x, y = int(rng.integers(-mag, mag + 1)), int(rng.integers(-mag, mag + 1))
            mv32 = mv32 or (x, y)
            e16 = int(rng.choice((0, 7, 15, 16, int(rng.integers(0, 1 << 12)), int(rng.integers(0, 1 << 24)), G.INT_MAX)))
            sse_y = int(rng.choice((0, 15, 16, int(rng.integers(0, 32000)), int(rng.integers(0, 250 * PIX_MAX * PIX_MAX + 1)))))
            row += list(mv32 if not split else (x, y)) + [e16 if split else e32, sse_y]
            tail.append(int(rng.choice((0, 1, 15, 16, 17, int(rng.integers(0, 8000)),
                                        int(rng.integers(0, 58 * PIX_MAX * PIX_MAX + 1))))))
        rows.append(row + [decay_c] + tail)
    return np.array(rows, np.int64)


def sse_block8(targets) -> np.ndarray:
    """A 16x16 block of 10-bit differences whose 8x8 quarters have the SSEs asked for."""
    blk = np.zeros((16, 16), np.uint16)
    for j, t in enumerate(targets):
        vals, rem = [], int(t)
        while rem:
            v = min(PIX_MAX, int(np.sqrt(rem)))
            while v * v > rem:
                v -= 1
            vals.append(v)
            rem -= v * v
        assert len(vals) <= 64, t
        q = np.zeros(64, np.uint16)
        q[:len(vals)] = vals
        blk[(j >> 1) * 8:(j >> 1) * 8 + 8, (j & 1) * 8:(j & 1) * 8 + 8] = q.reshape(8, 8)
    return blk


def tuple_meta(t) -> (dict, dict):
    meta, ctl = GF.tuple_meta(t[:GF.WEIGHT_COLS])
    return meta, dict(ctl, tf_decay_factor_cb_fp16=int(t[GF.WEIGHT_COLS]), tf_decay_factor_cr_fp16=int(t[GF.WEIGHT_COLS]))


def reference_weights(tuples: np.ndarray) -> np.ndarray:
    """[tuples][4]: the weights svt_av1_apply_temporal_filter_planewise_medium_hbd_c adds to the count of
    Cb (and, with the same decay factor and samples, of Cr)."""
    ar = RefArithUVH()
    out = np.zeros((len(tuples), 4), np.uint32)
    src = [np.zeros((64, 64), np.uint16), np.zeros((32, 32), np.uint16), np.zeros((32, 32), np.uint16)]
    decay = ar.field("tf_decay_factor_fp16", np.uint32, 3)
    for k, t in enumerate(tuples):
        meta, ctl = tuple_meta(t)
        for x, y in [meta["mv32"]] + meta["mv16"]:
            assert x * x + y * y < 1 << 31
        assert meta["split"] or len(set(meta["err16"])) == 1
        ar.set_block(meta, 0, 0, ctl)
        decay[1] = decay[2] = ctl["tf_decay_factor_cb_fp16"]
        pre = [np.zeros((64, 64), np.uint16), np.zeros((32, 32), np.uint16), np.zeros((32, 32), np.uint16)]
        pre[0][:32, :32] = GH.sse_block16([int(t[6 + 4 * j]) for j in range(4)])
        pre[1][:16, :16] = pre[2][:16, :16] = sse_block8([int(v) for v in t[GF.WEIGHT_COLS + 1:]])
        accum = [np.zeros(s * s, np.uint32) for s in (64, 32, 32)]
        count = [np.zeros(s * s, np.uint16) for s in (64, 32, 32)]
        ar.apply32_yuv(src, pre, (0, 0), accum, count)
        cb, cr = count[1].reshape(32, 32), count[2].reshape(32, 32)
        out[k] = [cb[0, 0], cb[0, 8], cb[8, 0], cb[8, 8]]
        assert np.array_equal(cb, cr)
    return out


def case_inputs(case: dict):
    """-> (16-bit pictures {picture: host_picture}, 16-bit chroma {picture: (cb, cr) padded}, subpel)."""
    W, H = S.align8(case["w"]), S.align8(case["h"])
    pics = {t: GH.host_picture(f) for t, f in GH.frames10(case).items()}
    uv = {t: tuple(pad_chroma16(p, W, H) for p in planes) for t, planes in chroma_frames10(case).items()}
    return pics, uv, GF.random_subpel(case)


def run_case(case: dict, arith: HbdGlueUV, cover: dict) -> dict:
    pics, uv, sub = case_inputs(case)
    res = filter_window_yuv_hbd(pics[case["centre"]], [pics[r] for r in case["refs"]], uv[case["centre"]],
                                [uv[r] for r in case["refs"]], case["controls"], sub, arith, cover)
    res["subpel"] = sub
    return res


FIXTURE_KEYS = ("y", "cb", "cr", "err32", "weights_uv", "subpel")


def main():
    cases = case_dicts()
    arrays, cover, per_case = {}, {k: 0 for k in COUNTED_KEYS}, {}
    ar, luma = RefArithUVH(), GH.RefArithH()
    for case in cases:
        before = dict(cover)
        res = run_case(case, ar, cover)
        # the luma beside the chroma is the luma of the luma-only functions
        pics, _, sub = case_inputs(case)
        plane, err32, weights = GH.filter_window_hbd(pics[case["centre"]], [pics[r] for r in case["refs"]],
                                                     GC.luma_controls(case["controls"]), sub, luma,
                                                     {k: 0 for k in GH.COUNTED_KEYS})
        assert np.array_equal(plane, res["y"]) and np.array_equal(err32, res["err32"])
        assert np.array_equal(weights, res["weights"])
        for name in FIXTURE_KEYS:
            arrays[case["id"] + "." + name] = res[name]
        per_case[case["id"]] = {k: int(cover[k] - before[k]) for k in COUNTED_KEYS if cover[k] != before[k]}
        print(case["id"], res["cb"].shape, per_case[case["id"]])
    tuples = weight_tuples()
    arrays["weights.in"], arrays["weights.out"] = tuples, reference_weights(tuples)
    doc = {"cases": cases, "coverage": {k: int(cover[k]) for k in COVERAGE_KEYS}, "coverage_per_case": per_case,
           "weights_sse_max": [int(tuples[:, 6:GF.WEIGHT_COLS:4].max()), int(tuples[:, GF.WEIGHT_COLS + 1:].max())]}
    with open(os.path.join(HERE, "tffhc_cases.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    G.write_npz(os.path.join(HERE, "tffhc_cases.npz"), arrays)
    missing = [k for k in COVERAGE_KEYS if cover[k] == 0]
    if missing:
        sys.exit("coverage counts of 0: " + ", ".join(missing))


if __name__ == "__main__":
    main()
