"""Generate the TF chroma fixtures (tests/golden/tffc_cases.json, tffc_cases.npz).

Temporal filtering with tf_chroma set, 8 bit, 4:2:0, use_zz_based_filter == 0: what
svtme_tf_filter_yuv computes beside the luma of make_golden_tff.py. The expected
values are put together as there, from the pieces the reference exports
(oracle/_ref/libtfsp_ref.so):

  * svt_inter_predictor with MULTITAP_SHARP on chroma planes at the chroma block size
    (32, 16, 8 or 4 square), so the reference itself picks sub_pel_filters_4 at 4x4
    (av1_get_convolve_filter_params, inter_prediction.h:137-153);
  * svt_aom_apply_filtering_central_c, svt_av1_apply_temporal_filter_planewise_medium_c
    and svt_aom_get_final_filtered_pixels_c with MeContext.tf_chroma = 1 and the three
    decay factors, on the three planes of each SB.

The glue between them is a RESTATEMENT (filter_window_yuv): the blocks are luma's
(make_golden_tff.sb_blocks), each predicts its half-size Cb and Cr block at the luma MV
read as 1/16 chroma pel and clamped with the chroma block size (clamp_uv,
enc_inter_prediction.c:28-48 with ss 1), svt_aom_inter_prediction's chroma part
(:4248-4360). Reference-side chroma planes carry a replicated margin of 40
(svtme.PAD_CHROMA; the reference's own is 36, see include/svtme.h). The arithmetic is
handed to the glue (`arith`): RefArithUV here, tests/tffc_model.py passes one in numpy.

  tffc_cases.json  the case list with the controls of each case, the coverage counts
  tffc_cases.npz   per case "<id>.cb", "<id>.cr" [H/2][W/2] u8, "<id>.weights_uv"
                   [refs][SBs][2][16] u32 (plane, 32x32 luma block * 4 + quarter),
                   "<id>.subpel" [refs][SBs] (svtme.TF_SUBPEL_SB_DTYPE)

Container only (needs oracle/_ref). Run from the repository root:
python tests/golden/make_golden_tffc.py. The output is byte-for-byte reproducible. It
fails when a coverage count is 0.
"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "svt-av1-mirror_amd"))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_golden_tff as GF  # noqa: E402
import make_golden_tfsp as G  # noqa: E402
import svtme as S  # noqa: E402
import tfsp_content  # noqa: E402

PAD = S.PAD_CHROMA

# id, content, w, h, centre, references, seed of random_subpel, controls
CASES = [
    ("c64_rand", "frac", 64, 64, 8, [7, 9], 31,
     dict(tf_decay_factor_fp16=2_000_000, tf_mv_dist_th=64, sub_sampling_shift=0,
          tf_decay_factor_cb_fp16=2_000_000, tf_decay_factor_cr_fp16=0x7FFFFFFF)),
    ("c72_rand", "frac", 72, 40, 8, [9], 48,  # chroma 36 x 20: the second SB column holds 4 chroma samples
     dict(tf_decay_factor_fp16=1023, tf_mv_dist_th=450, sub_sampling_shift=1,
          tf_decay_factor_cb_fp16=0x7FFFFFFF, tf_decay_factor_cr_fp16=2_000_000)),
    ("c128_rand", "frac", 128, 128, 8, [7, 9, 6], 33,
     dict(tf_decay_factor_fp16=2_000_000, tf_mv_dist_th=0, sub_sampling_shift=1,
          tf_decay_factor_cb_fp16=0x7FFFFFFF, tf_decay_factor_cr_fp16=1023)),
    ("c8_rand", "frac", 8, 8, 8, [9], 34,  # chroma 4 x 4
     dict(tf_decay_factor_fp16=0x7FFFFFFF, tf_mv_dist_th=32767, sub_sampling_shift=0,
          tf_decay_factor_cb_fp16=1023, tf_decay_factor_cr_fp16=0x7FFFFFFF)),
    ("c64_same", "same", 64, 64, 8, [7, 9], 35,  # identical pictures: SSE 0 where the MV is 0
     dict(tf_decay_factor_fp16=0, tf_mv_dist_th=64, sub_sampling_shift=1,
          tf_decay_factor_cb_fp16=2_000_000, tf_decay_factor_cr_fp16=0)),
]

LUMA_KEYS = ("tf_decay_factor_fp16", "tf_mv_dist_th", "sub_sampling_shift")
COVERAGE_KEYS = ("pred_c32", "pred_c16", "pred_c8", "pred_c4",
                 "conv_copy", "conv_x", "conv_y", "conv_2d",  # chroma blocks of 8 and above
                 "conv4_copy", "conv4_x", "conv4_y", "conv4_2d",  # 4x4: the 4-tap set
                 "clamp_left", "clamp_right", "clamp_top", "clamp_bottom",
                 "clamp_chroma_alone",  # an axis the chroma clamp changes and the luma clamp does not
                 "cb_weight_0", "cb_weight_1000", "cb_weight_between",
                 "cr_weight_0", "cr_weight_1000", "cr_weight_between",
                 "quarter_cb_ne_cr", "block_beyond_w2", "block_beyond_h2")


def case_dicts():
    return [{"id": c[0], "kind": c[1], "w": c[2], "h": c[3], "centre": c[4], "refs": list(c[5]), "subpel": "random",
             "seed": c[6], "controls": dict(c[7])} for c in CASES]


def luma_controls(ctl: dict) -> dict:
    return {k: ctl[k] for k in LUMA_KEYS}


def chroma_frames(case: dict) -> dict:
    """{picture number: (cb, cr)} of a case, ((h + 1) >> 1, (w + 1) >> 1) each: content of its own,
    drawn apart from the luma's (other seeds, the chroma size)."""
    ts = sorted(set([case["centre"]] + case["refs"]))
    cw, ch = (case["w"] + 1) >> 1, (case["h"] + 1) >> 1
    if case["kind"] == "same":
        cb, cr = (tfsp_content.fractional_frames(cw, ch, [0], seed=s)[0] for s in (11, 13))
        return {t: (cb.copy(), cr.copy()) for t in ts}
    if case["kind"] == "noise":
        rng = np.random.default_rng(900 + cw * 1000 + ch)
        return {t: (rng.integers(0, 256, (ch, cw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8))
                for t in ts}
    cb, cr = (tfsp_content.fractional_frames(cw, ch, ts, seed=s) for s in (11, 13))
    return {t: (cb[t], cr[t]) for t in ts}


def pad_chroma(plane: np.ndarray, W: int, H: int) -> np.ndarray:
    """What svtme_picture_upload_chroma leaves: the true plane replicated to W/2 x H/2 of the aligned
    picture, then margins of PAD replicated samples -> [H/2 + 2 PAD][W/2 + 2 PAD]."""
    ch, cw = plane.shape
    assert cw <= W // 2 and ch <= H // 2
    return np.ascontiguousarray(np.pad(plane, ((PAD, PAD + H // 2 - ch), (PAD, PAD + W // 2 - cw)), mode="edge"))


def clamp_uv(mv: int, pu: int, b: int, dim: int):
    """One axis of clamp_mv_to_umv_border_sb (enc_inter_prediction.c:28-48) with ss = 1 for the chroma
    block of the luma block of size b at pu of an aligned picture of size dim: -> (q4 MV in 1/16 chroma
    pel, clamped low, clamped high). mb_to_*_edge are the luma block's, unscaled."""
    q4 = G.i16(mv)  # (int16_t)(mv * (1 << (1 - ss)))
    spel = (4 + b // 2) << 4  # (AOM_INTERP_EXTEND + bw) << SUBPEL_BITS, bw the chroma width
    lo = -(pu * 8) - spel
    hi = (dim - b - pu) * 8 + spel - 16
    return (lo if q4 < lo else hi if q4 > hi else q4), q4 < lo, q4 > hi


def filter_window_yuv(cen, refs: list, cen_uv, refs_uv: list, ctl: dict, subpel: np.ndarray, arith, cover: dict):
    """make_golden_tff.filter_window with the chroma stage. cen / refs: svtme.HostPyramid; cen_uv /
    refs_uv: (cb, cr) padded by pad_chroma -> dict(y [H][W], cb, cr [H/2][W/2], err32 [refs][SBs][4],
    weights [refs][SBs][16], weights_uv [refs][SBs][2][16])."""
    W, H, pad = cen.width, cen.height, S.PAD_FULL
    wb, hb = (W + 63) // 64, (H + 63) // 64
    n, ss = len(refs), ctl["sub_sampling_shift"]
    y = np.zeros((hb * 64, wb * 64), np.uint8)
    uv = np.zeros((2, hb * 32, wb * 32), np.uint8)
    err32 = np.zeros((n, wb * hb, 4), np.uint32)
    weights = np.zeros((n, wb * hb, 16), np.uint32)
    weights_uv = np.zeros((n, wb * hb, 2, 16), np.uint32)
    for k in range(wb * hb):
        sb_x, sb_y = 64 * (k % wb), 64 * (k // wb)
        cen64 = np.ascontiguousarray(cen.full[pad + sb_y:pad + sb_y + 64, pad + sb_x:pad + sb_x + 64])
        cen32 = [np.ascontiguousarray(p[PAD + sb_y // 2:PAD + sb_y // 2 + 32, PAD + sb_x // 2:PAD + sb_x // 2 + 32])
                 for p in cen_uv]
        preds, metas = [], []
        for r, ref in enumerate(refs):
            sub = subpel[r, k]
            pred = np.zeros((64, 64), np.uint8)
            pred_uv = [np.zeros((32, 32), np.uint8), np.zeros((32, 32), np.uint8)]
            for b, bx, by, m in GF.sb_blocks(sub):
                px, py = sb_x + bx, sb_y + by
                mvx, mvy = int(sub["mv"]["x"][m]), int(sub["mv"]["y"][m])
                assert mvx * mvx + mvy * mvy < 1 << 31
                qx, lx0, lx1 = G.clamp(mvx, px, b, W)
                qy, ly0, ly1 = G.clamp(mvy, py, b, H)
                pred[by:by + b, bx:bx + b] = arith.predict(ref.full, pad, b, px, py, qx, qy)
                cx, cl, cr = clamp_uv(mvx, px, b, W)
                cy, ct, cbm = clamp_uv(mvy, py, b, H)
                c = b // 2
                for key, hit in (("clamp_left", cl), ("clamp_right", cr), ("clamp_top", ct), ("clamp_bottom", cbm),
                                 ("clamp_chroma_alone", ((cl or cr) and not (lx0 or lx1)) or
                                  ((ct or cbm) and not (ly0 or ly1))),
                                 ("block_beyond_w2", px // 2 >= W // 2), ("block_beyond_h2", py // 2 >= H // 2),
                                 ("pred_c32", c == 32), ("pred_c16", c == 16), ("pred_c8", c == 8), ("pred_c4", c == 4)):
                    cover[key] += bool(hit)
                cover[("conv4_" if c == 4 else "conv_") + ("copy", "x", "y", "2d")[bool(cx & 15) + 2 * bool(cy & 15)]] += 1
                for p in range(2):
                    pred_uv[p][by // 2:by // 2 + c, bx // 2:bx // 2 + c] = arith.predict(refs_uv[r][p], PAD, c, px // 2,
                                                                                        py // 2, cx, cy)
            if sub["branch"] == S.TFSP_32:
                e32 = [int(sub["error"][1 + i]) for i in range(4)]
            else:  # (:2714-2757)
                e32 = [arith.var32(pred[yy:yy + 32, xx:xx + 32], cen64[yy:yy + 32, xx:xx + 32], ss)
                       for yy, xx in ((0, 0), (0, 32), (32, 0), (32, 32))]
            err32[r, k] = e32
            preds.append((pred, pred_uv[0], pred_uv[1]))
            metas.append(GF.filter_meta(sub, e32))
        out, w = arith.filter_sb_yuv(cen64, cen32[0], cen32[1], preds, metas, ctl)
        y[sb_y:sb_y + 64, sb_x:sb_x + 64] = out[0]
        for p in range(2):
            uv[p, sb_y // 2:sb_y // 2 + 32, sb_x // 2:sb_x // 2 + 32] = out[1 + p]
            weights_uv[:, k, p] = w[1 + p]
            name = ("cb", "cr")[p]
            cover[name + "_weight_0"] += int((w[1 + p] == 0).sum())
            cover[name + "_weight_1000"] += int((w[1 + p] == 1000).sum())
            cover[name + "_weight_between"] += int(((w[1 + p] > 0) & (w[1 + p] < 1000)).sum())
        weights[:, k] = w[0]
        cover["quarter_cb_ne_cr"] += int((w[1] != w[2]).sum())
    return {"y": y[:H, :W].copy(), "cb": uv[0, :H // 2, :W // 2].copy(), "cr": uv[1, :H // 2, :W // 2].copy(),
            "err32": err32, "weights": weights, "weights_uv": weights_uv}


def quarter_weights(delta: np.ndarray, size: int) -> np.ndarray:
    """[16] from the count a reference added to a size x size plane (64: luma, 32: chroma): constant over
    each quarter of each 32x32 luma block."""
    h, q = size // 2, size // 4
    w = np.zeros(16, np.uint32)
    for i in range(4):
        for j in range(4):
            blk = delta[(i >> 1) * h + (j >> 1) * q:, (i & 1) * h + (j & 1) * q:][:q, :q]
            assert (blk == blk[0, 0]).all()
            w[i * 4 + j] = blk[0, 0]
    return w


class RefArithUV(GF.RefArith):
    """The reference's own arithmetic with MeContext.tf_chroma set."""

    def __init__(self):
        super().__init__()
        self.field("tf_chroma", np.uint8)[0] = 1

    def filter_sb_yuv(self, cen64, cen_cb, cen_cr, preds, metas, ctl):
        sizes = (64, 32, 32)
        src = (cen64, cen_cb, cen_cr)
        accum = [np.zeros(s * s, np.uint32) for s in sizes]
        count = [np.zeros(s * s, np.uint16) for s in sizes]
        ptr = lambda a: (C.c_void_p * 3)(*[x.ctypes.data for x in a])  # noqa: E731
        # src_stride_ch = stride_y >> ss_x = 32 (:355-356)
        self.lib.svt_aom_apply_filtering_central_c(self.me.ctypes.data, self.desc.ctypes.data, ptr(src), ptr(accum),
                                                   ptr(count), 64, 64, 1, 1)
        decay = self.field("tf_decay_factor_fp16", np.uint32, 3)
        weights = [np.zeros((len(preds), 16), np.uint32) for _ in sizes]
        for r, (pred, meta) in enumerate(zip(preds, metas)):
            before = [c.copy() for c in count]
            for row in range(2):  # (:3353-3375), apply_filtering_block_plane_wise (:1411-1493)
                for col in range(2):
                    self.set_block(meta[col + 2 * row], row, col, ctl)
                    decay[1], decay[2] = ctl["tf_decay_factor_cb_fp16"], ctl["tf_decay_factor_cr_fp16"]
                    o, oc = row * 32 * 64 + col * 32, row * 16 * 32 + col * 16
                    self.lib.svt_av1_apply_temporal_filter_planewise_medium_c(
                        self.me.ctypes.data, src[0].ctypes.data + o, 64, pred[0].ctypes.data + o, 64,
                        src[1].ctypes.data + oc, src[2].ctypes.data + oc, 32, pred[1].ctypes.data + oc,
                        pred[2].ctypes.data + oc, 32, 32, 32, 1, 1, accum[0].ctypes.data + 4 * o,
                        count[0].ctypes.data + 2 * o, accum[1].ctypes.data + 4 * oc, count[1].ctypes.data + 2 * oc,
                        accum[2].ctypes.data + 4 * oc, count[2].ctypes.data + 2 * oc)
            for p, s in enumerate(sizes):
                weights[p][r] = quarter_weights((count[p] - before[p]).reshape(s, s), s)
        out = [np.zeros((s, s), np.uint8) for s in sizes]
        stride = (C.c_uint32 * 3)(64, 32, 32)
        self.lib.svt_aom_get_final_filtered_pixels_c(self.me.ctypes.data, ptr(out), None, ptr(accum), ptr(count), stride,
                                                     0, 0, 32, 32, False)
        return out, weights


def case_inputs(case: dict, checker: str = "ref"):
    """-> (pyramids {picture: HostPyramid}, chroma {picture: (cb, cr) padded}, subpel [refs][SBs])."""
    W, H = S.align8(case["w"]), S.align8(case["h"])
    pyr = {t: S.build_host_pyramid(f, checker) for t, f in G.case_frames(case).items()}
    uv = {t: tuple(pad_chroma(p, W, H) for p in planes) for t, planes in chroma_frames(case).items()}
    return pyr, uv, GF.random_subpel(case)


def run_case(case: dict, arith, cover: dict, checker: str = "ref") -> dict:
    pyr, uv, sub = case_inputs(case, checker)
    res = filter_window_yuv(pyr[case["centre"]], [pyr[r] for r in case["refs"]], uv[case["centre"]],
                            [uv[r] for r in case["refs"]], case["controls"], sub, arith, cover)
    res["subpel"] = sub
    return res


def main():
    cases = case_dicts()
    arrays, cover, per_case = {}, {k: 0 for k in COVERAGE_KEYS}, {}
    ar, luma = RefArithUV(), GF.RefArith()
    for case in cases:
        before = dict(cover)
        res = run_case(case, ar, cover)
        # the luma beside the chroma is the luma of the luma-only functions
        pyr, _, sub = case_inputs(case)
        plane, err32, weights = GF.filter_window(pyr[case["centre"]], [pyr[r] for r in case["refs"]],
                                                 luma_controls(case["controls"]), sub, luma,
                                                 {k: 0 for k in GF.COVERAGE_KEYS})
        assert np.array_equal(plane, res["y"]) and np.array_equal(err32, res["err32"])
        assert np.array_equal(weights, res["weights"])
        for name in ("cb", "cr", "weights_uv", "subpel"):
            arrays[case["id"] + "." + name] = res[name]
        per_case[case["id"]] = {k: cover[k] - before[k] for k in COVERAGE_KEYS if cover[k] != before[k]}
        print(case["id"], res["cb"].shape, per_case[case["id"]])
    doc = {"cases": cases, "coverage": cover, "coverage_per_case": per_case}
    with open(os.path.join(HERE, "tffc_cases.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    G.write_npz(os.path.join(HERE, "tffc_cases.npz"), arrays)
    missing = [k for k in COVERAGE_KEYS if cover[k] == 0]
    if missing:
        sys.exit("coverage counts of 0: " + ", ".join(missing))


if __name__ == "__main__":
    main()
