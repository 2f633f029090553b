"""Generate the 10-bit TF filter fixtures (tests/golden/tffh_cases.json, tffh_cases.npz).

What follows the sub-pel refinement in produce_temporally_filtered_pic
(temporal_filtering.c:3196-3390) for luma with is_highbd set, use_zz_based_filter == 0
and use_8bit_subpel == 1: the sub-pel results are those of the 8-bit stage on the MSB
planes, the final prediction, the 32x32 errors of the 64x64 branches, the weights, the
accumulation and the normalisation run on the packed 16-bit pictures. The expected
values come from the reference's own functions in oracle/_ref/libtfsp_ref.so
(make_golden_tfsp.load_enc):

  * svt_highbd_inter_predictor with MULTITAP_SHARP and bd 10;
  * svt_aom_highbd_10_variance32x32_c / 32x16_c (convert_64x64_info_to_32x32_info);
  * svt_aom_apply_filtering_central_highbd_c,
    svt_av1_apply_temporal_filter_planewise_medium_hbd_c and
    svt_aom_get_final_filtered_pixels_c with is_highbd.

The glue between them is make_golden_tff's (sb_blocks, the clamp, filter_meta,
filter_window), shared as it stands. filter_window keeps the predictions and the plane in
8-bit arrays of its own, so the arithmetic handed to it (HbdGlue) keeps the 16-bit
arrays beside them: it collects each (reference, SB)'s blocks into its own 64x64
prediction, answers var32 and filter_sb from those, and keeps the 16-bit result of every
SB, from which filter_window_hbd puts the plane together. tests/tffh_model.py passes the
same glue an arithmetic in numpy and Python integers.

Inputs: the 10-bit frame of a case is (frame8 << 2) | lsb with frame8 the 8-bit case's
frame and lsb two seeded random bits, so the MSB plane is the 8-bit case's picture and
its sub-pel results (tfsp_cases.npz, or make_golden_tff.random_subpel) are valid as
they stand. The "clip" cases hold runs of 0 and of 1023 next to mid-grey edges: the
sharp filter's lobes leave [0, 1023] there on both sides.

  tffh_cases.json  the case list, the controls, the coverage counts
  tffh_cases.npz   per case "<id>.plane" [H][W] u16, "<id>.err32" [refs][SBs][4] u32,
                   "<id>.weights" [refs][SBs][16] u32, for the cases with random sub-pel
                   results "<id>.subpel"; "weights.in" [tuples][19] i8 (make_golden_tff's
                   columns, SSEs up to 256 x 1023^2) and "weights.out" [tuples][4] u32

Container only (needs oracle/_ref). Run from the repository root:
python tests/golden/make_golden_tffh.py. The output is byte-for-byte reproducible. It
fails when a required coverage count is 0.
"""
import ctypes as C
import json
import os
import sys
import zlib
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "svt-av1-mirror_amd"))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import make_golden_tff as GF  # noqa: E402
import make_golden_tfsp as G  # noqa: E402
import svtme as S  # noqa: E402

BD = 10
PIX_MAX = (1 << BD) - 1

# the 8-bit fixtures' cases taken over (their controls with them); the 192x136 ones are left out
KEEP = ("frac128_l8_w3", "edges128_l2", "frac72_h0q2_wrap", "frac200_h3q3_wrap", "frac200_h0q0_wrap",
        "noise124_h0q2_wrap", "frac124_h3q3", "frac72_l2_w5", "own64_rand", "own72_rand", "own128_rand", "own64_same")
# cases of this file: id, w, h, centre, references, seed of random_subpel
CLIP_CASES = [("clip64_rand", 64, 64, 8, [7, 9], 31), ("clip72_rand", 72, 40, 8, [9], 32)]

COVERAGE_KEYS = GF.COVERAGE_KEYS + ("clip_low", "clip_high")  # a predicted sample below 0 / above 1023 before the clip
COUNTED_KEYS = COVERAGE_KEYS + ("var_clamped_to_0",)  # counted and reported, not required


def case_dicts():
    by_id = {c["id"]: c for c in GF.case_dicts()}
    out = [dict(by_id[name]) for name in KEEP]
    k0 = len(by_id)
    for k, c in enumerate(CLIP_CASES):
        out.append({"id": c[0], "kind": "clip", "w": c[1], "h": c[2], "centre": c[3], "refs": list(c[4]),
                    "subpel": "random", "seed": c[5], "controls": GF.tff_controls(k0 + k)})
    return out


def clip_frames(w: int, h: int, ts) -> dict:
    """8-bit pictures of cells 10 wide and 7 high at 0, 128, 255, 128 in turn, moving by (3, 2) a picture."""
    y, x = np.mgrid[0:h, 0:w]
    levels = np.array([0, 128, 255, 128], np.uint8)
    return {t: levels[((x + 3 * t) // 10 + (y + 2 * t) // 7) % 4] for t in ts}


def frames8(case: dict) -> dict:
    if case["kind"] == "clip":
        return clip_frames(case["w"], case["h"], sorted(set([case["centre"]] + case["refs"])))
    return G.case_frames(case)


def frames10(case: dict) -> dict:
    """{picture number: [h][w] u16}: (frame8 << 2) | two seeded random bits; in the clip cases 0 stays 0
    and 255 becomes 1023."""
    out = {}
    for t, f in frames8(case).items():
        rng = np.random.default_rng([zlib.crc32(case["id"].encode()), t])
        lsb = rng.integers(0, 4, f.shape, dtype=np.uint16)
        if case["kind"] == "clip":
            lsb = np.where(f == 0, 0, np.where(f == 255, 3, lsb)).astype(np.uint16)
        out[t] = (f.astype(np.uint16) << 2) | lsb
    return out


def pad_hbd(y: np.ndarray, W: int, H: int) -> np.ndarray:
    """The padded 16-bit plane of an aligned W x H picture from its true samples: replicated to the
    aligned size and by SVTME_PAD_FULL on every side (svt_aom_pack_highbd_pic of the padded 8-bit and
    2-bit planes: pad_2b_compressed_input_picture and svt_aom_generate_padding_compressed_10bit repeat
    the edge sample's two bits where svt_aom_generate_padding repeats its eight)."""
    h, w = y.shape
    return np.ascontiguousarray(np.pad(y, ((S.PAD_FULL, H - h + S.PAD_FULL), (S.PAD_FULL, W - w + S.PAD_FULL)), mode="edge"))


def host_picture(y: np.ndarray) -> SimpleNamespace:
    """What filter_window reads of a svtme.HostPyramid, on 16-bit samples."""
    W, H = S.align8(y.shape[1]), S.align8(y.shape[0])
    return SimpleNamespace(width=W, height=H, full=pad_hbd(np.ascontiguousarray(y, np.uint16), W, H))


def var_parts(pred, cen, ss):
    """svt_aom_highbd_10_variance32x32_c / 32x16_c restated far enough to see the clamp: (rounded sse,
    rounded sum, N) over the kept rows (svt_psnr.c:139-177)."""
    d = pred[::1 << ss].astype(np.int64) - cen[::1 << ss].astype(np.int64)
    return (int((d * d).sum()) + 8) >> 4, (int(d.sum()) + 2) >> 2, 32 * (32 >> ss)


class HbdGlue:
    """Runs make_golden_tff.filter_window on 16-bit samples. A subclass gives predict16, var32_16 and
    filter_sb16; `cover` receives the counts filter_window does not make."""
    cover = None

    def begin(self, cover: dict):
        self.cover, self.preds, self.cur, self.filled, self.nvar, self.outs = cover, [], None, 0, 0, []

    def predict(self, full, pad, b, px, py, qx, qy) -> np.ndarray:
        if self.cur is None:
            self.cur, self.filled = np.zeros((64, 64), np.uint16), 0
        p = self.predict16(full, pad, b, px, py, qx, qy)
        self.cur[py % 64:py % 64 + b, px % 64:px % 64 + b] = p
        self.filled += b * b
        if self.filled == 64 * 64:  # the blocks of a (reference, SB) tile the SB
            self.preds.append(self.cur)
            self.cur, self.nvar = None, 0
        return (p & 0xFF).astype(np.uint8)

    def var32(self, pred, cen, ss) -> int:
        y, x = ((0, 0), (0, 32), (32, 0), (32, 32))[self.nvar]  # the order filter_window asks in
        self.nvar += 1
        p = self.preds[-1][y:y + 32, x:x + 32]
        sse, total, n = var_parts(p, cen, ss)
        self.cover["var_clamped_to_0"] += sse - total * total // n < 0
        return self.var32_16(p, cen, ss)

    def filter_sb(self, cen64, preds, metas, ctl):
        assert len(self.preds) == len(preds) and self.cur is None
        out, weights = self.filter_sb16(cen64, self.preds, metas, ctl)
        self.outs.append(out)
        self.preds = []
        return (out & 0xFF).astype(np.uint8), weights


def filter_window_hbd(cen, refs: list, ctl: dict, subpel: np.ndarray, arith: HbdGlue, cover: dict):
    """make_golden_tff.filter_window on 16-bit pictures (host_picture) -> (plane [H][W] u16 of the aligned
    picture, err32 [refs][SBs][4], weights [refs][SBs][16])."""
    arith.begin(cover)
    _, err32, weights = GF.filter_window(cen, refs, ctl, subpel, arith, cover)
    W, H = cen.width, cen.height
    wb, hb = (W + 63) // 64, (H + 63) // 64
    plane = np.zeros((hb * 64, wb * 64), np.uint16)
    for k, out in enumerate(arith.outs):
        plane[64 * (k // wb):64 * (k // wb) + 64, 64 * (k % wb):64 * (k % wb) + 64] = out
    return plane[:H, :W].copy(), err32, weights


# ----------------------------------------------------------------------------
# the reference's arithmetic
# ----------------------------------------------------------------------------
def byteptr(a: np.ndarray, offset: int = 0) -> int:
    """CONVERT_TO_BYTEPTR of a 16-bit array's sample `offset`."""
    return (a.ctypes.data + 2 * offset) >> 1


class RefArithH(HbdGlue, GF.RefArith):
    """The reference's own high-bit-depth arithmetic (oracle/_ref/libtfsp_ref.so)."""

    def __init__(self):
        GF.RefArith.__init__(self)
        lib, vp, i32 = self.lib, C.c_void_p, C.c_int
        lib.svt_aom_asm_set_convolve_hbd_asm_table.argtypes = []
        lib.svt_aom_asm_set_convolve_hbd_asm_table()  # svt_aom_convolveHbd[][][] from the rtcd pointers (the C kernels)
        lib.svt_highbd_inter_predictor.argtypes = [vp, C.c_int32, vp, C.c_int32, C.POINTER(G.SubpelParams), vp, C.c_int32,
                                                   C.c_int32, C.POINTER(G.ConvolveParams), C.c_uint32, C.c_int32,
                                                   C.c_int32]
        lib.svt_highbd_inter_predictor.restype = None
        for name in ("svt_aom_highbd_10_variance32x32_c", "svt_aom_highbd_10_variance32x16_c"):
            fn = getattr(lib, name)
            fn.argtypes = [vp, i32, vp, i32, C.POINTER(C.c_uint32)]
            fn.restype = C.c_uint32
        lib.svt_aom_apply_filtering_central_highbd_c.argtypes = [vp, vp, vp, vp, vp, C.c_uint16, C.c_uint16, C.c_uint32,
                                                                 C.c_uint32]
        lib.svt_aom_apply_filtering_central_highbd_c.restype = None
        lib.svt_av1_apply_temporal_filter_planewise_medium_hbd_c.argtypes = (
            [vp, vp, i32, vp, i32, vp, vp, i32, vp, vp, i32, C.c_uint, C.c_uint, i32, i32] + [vp] * 6 + [C.c_uint32])
        lib.svt_av1_apply_temporal_filter_planewise_medium_hbd_c.restype = None

    def predict16(self, full, pad, b, px, py, qx, qy) -> np.ndarray:
        import tffh_model as MH  # the clip counts are the model's: the reference returns clipped samples only

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
        raw = MH.predict_unclipped(full, pad, b, px, py, qx, qy)
        assert np.array_equal(np.clip(raw, 0, PIX_MAX), pred)
        self.cover["clip_low"] += int((raw < 0).sum())
        self.cover["clip_high"] += int((raw > PIX_MAX).sum())
        return pred

    def var32_16(self, pred, cen, ss) -> int:
        pred, cen = np.ascontiguousarray(pred), np.ascontiguousarray(cen)
        sse = C.c_uint32()
        fn = getattr(self.lib, "svt_aom_highbd_10_variance32x16_c" if ss else "svt_aom_highbd_10_variance32x32_c")
        return (fn(byteptr(pred), 32 << ss, byteptr(cen), 32 << ss, C.byref(sse)) << ss) & 0xFFFFFFFF  # (:2748-2753)

    def apply32_hbd(self, src, src_stride, pre, pre_stride, accum, count):
        self.lib.svt_av1_apply_temporal_filter_planewise_medium_hbd_c(
            self.me.ctypes.data, src, src_stride, pre, pre_stride, None, None, 0, None, None, 0, 32, 32, 1, 1,
            accum, count, None, None, None, None, BD)

    def filter_sb16(self, cen64, preds, metas, ctl):
        accum, count = np.zeros(64 * 64, np.uint32), np.zeros(64 * 64, np.uint16)
        ptr = lambda a: (C.c_void_p * 3)(a.ctypes.data, None, None)  # noqa: E731
        cen64 = np.ascontiguousarray(cen64, np.uint16)
        self.lib.svt_aom_apply_filtering_central_highbd_c(self.me.ctypes.data, self.desc.ctypes.data, ptr(cen64),
                                                          ptr(accum), ptr(count), 64, 64, 1, 1)
        weights = np.zeros((len(preds), 16), np.uint32)
        for r, (pred, meta) in enumerate(zip(preds, metas)):
            before = count.copy()
            for row in range(2):  # (:3353-3375), apply_filtering_block_plane_wise (:1411-1493)
                for col in range(2):
                    self.set_block(meta[col + 2 * row], row, col, ctl)
                    o = row * 32 * 64 + col * 32
                    self.apply32_hbd(cen64.ctypes.data + 2 * o, 64, pred.ctypes.data + 2 * o, 64,
                                     accum.ctypes.data + 4 * o, count.ctypes.data + 2 * o)
            d = (count - before).reshape(64, 64)
            for i in range(4):
                for j in range(4):
                    q = d[(i >> 1) * 32 + (j >> 1) * 16:, (i & 1) * 32 + (j & 1) * 16:][:16, :16]
                    assert (q == q[0, 0]).all()
                    weights[r, i * 4 + j] = q[0, 0]
        out = np.zeros((64, 64), np.uint16)
        stride = (C.c_uint32 * 3)(64, 0, 0)
        self.lib.svt_aom_get_final_filtered_pixels_c(self.me.ctypes.data, None, ptr(out), ptr(accum), ptr(count), stride,
                                                     0, 0, 0, 0, True)
        return out, weights


# ----------------------------------------------------------------------------
# the fixture "weights": tuples through the reference's high-bit-depth filter function
# ----------------------------------------------------------------------------
SSE_MAX = 256 * PIX_MAX * PIX_MAX


def weight_tuples() -> np.ndarray:
    """make_golden_tff.weight_tuples' columns with the SSEs of 10-bit samples. The first 113 reach each
    index of the exp table in turn (MV 0, the threshold at its floor, a decay factor of 32 << 10, a
    block error of 0: the index is (((SSE >> 4) * 5) / 6) >> 3); the next 8 hold the largest SSE; the
    rest are drawn."""
    rng = np.random.default_rng(78)
    rows = []
    for t in range(113):
        sse = -(-(8 * t * 6) // 5) << 4
        rows.append([1, 32 << 10, 64] + [0, 0, 0, sse] * 4)
    for k in range(8):
        rows.append([k & 1, GF.DECAYS[k % 4], GF.DIST_THS[(k >> 1) % 4]] + [0, 0, 1 << (4 * k), SSE_MAX] * 4)
    for k in range(279):
        split = int(rng.integers(0, 2))
        decay = int(rng.choice(GF.DECAYS + (1024, 2047, 1 << 20, 3_000_000, 0xFFFFFFFF, int(rng.integers(0, 1 << 32)))))
        th = int(rng.choice(GF.DIST_THS + (1, 9, 10, 11, 100, 200, int(rng.integers(0, 32768)))))
        row = [split, decay, th]
        e32 = int(rng.choice((0, 5, 63, 64, int(rng.integers(0, 1 << 14)), int(rng.integers(0, 1 << 26)), G.INT_MAX)))
        mv32 = None
        for j in range(4):
            kind = int(rng.integers(0, 5))
            mag = (0, 3, 60, 3000, 32767)[kind]
            x, y = int(rng.integers(-mag, mag + 1)), int(rng.integers(-mag, mag + 1))
            if kind == 4 and rng.integers(0, 2):
                x, y = (32767 if x >= 0 else -32767), (32767 if y >= 0 else -32767)
            if k % 9 == 0:  # (x * x + y * y) << 8 wraps to 0 in 32 bits
                x, y = 4096 * int(rng.integers(1, 5)), 0
            mv32 = mv32 or (x, y)
            e16 = int(rng.choice((0, 7, 15, 16, int(rng.integers(0, 1 << 12)), int(rng.integers(0, 1 << 24)), G.INT_MAX)))
            sse = int(rng.choice((0, 1, 15, 16, int(rng.integers(0, 32000)),
                                  int(rng.integers(0, 250 * PIX_MAX * PIX_MAX + 1)))))  # (sse_block16 holds 256 squares)
            row += list(mv32 if not split else (x, y)) + [e16 if split else e32, sse]
        rows.append(row)
    return np.array(rows, np.int64)


def sse_block16(targets) -> np.ndarray:
    """A 32x32 block of 10-bit differences whose 16x16 quarters have the SSEs asked for."""
    blk = np.zeros((32, 32), np.uint16)
    for j, t in enumerate(targets):
        vals, rem = [], int(t)
        while rem:
            v = min(PIX_MAX, int(np.sqrt(rem)))
            while v * v > rem:
                v -= 1
            vals.append(v)
            rem -= v * v
        assert len(vals) <= 256, t
        q = np.zeros(256, np.uint16)
        q[:len(vals)] = vals
        blk[(j >> 1) * 16:(j >> 1) * 16 + 16, (j & 1) * 16:(j & 1) * 16 + 16] = q.reshape(16, 16)
    return blk


def reference_weights(tuples: np.ndarray) -> np.ndarray:
    """[tuples][4]: the weights svt_av1_apply_temporal_filter_planewise_medium_hbd_c adds to the count."""
    ar = RefArithH()
    out = np.zeros((len(tuples), 4), np.uint32)
    src = np.zeros((32, 32), np.uint16)
    for k, t in enumerate(tuples):
        meta, ctl = GF.tuple_meta(t)
        for x, y in [meta["mv32"]] + meta["mv16"]:
            assert x * x + y * y < 1 << 31
        assert meta["split"] or len(set(meta["err16"])) == 1
        ar.set_block(meta, 0, 0, ctl)
        pre = sse_block16([int(t[6 + 4 * j]) for j in range(4)])
        accum, count = np.zeros(32 * 32, np.uint32), np.zeros(32 * 32, np.uint16)
        ar.apply32_hbd(src.ctypes.data, 32, pre.ctypes.data, 32, accum.ctypes.data, count.ctypes.data)
        c = count.reshape(32, 32)
        out[k] = [c[0, 0], c[0, 16], c[16, 0], c[16, 16]]
    return out


def case_inputs(case: dict):
    """-> (16-bit pictures {picture: host_picture}, subpel [refs][SBs]) of a case."""
    pics = {t: host_picture(f) for t, f in frames10(case).items()}
    if case["subpel"] == "tfsp":
        sub = np.load(os.path.join(HERE, "tfsp_cases.npz"))[case["id"] + ".out"]
    else:
        sub = GF.random_subpel(case)
    return pics, sub


def run_case(case: dict, arith: HbdGlue, cover: dict) -> dict:
    pics, sub = case_inputs(case)
    plane, err32, weights = filter_window_hbd(pics[case["centre"]], [pics[r] for r in case["refs"]], case["controls"],
                                              sub, arith, cover)
    res = {"plane": plane, "err32": err32, "weights": weights}
    if case["subpel"] == "random":
        res["subpel"] = sub
    return res


def main():
    cases = case_dicts()
    arrays, cover, per_case = {}, {k: 0 for k in COUNTED_KEYS}, {}
    ar = RefArithH()
    for case in cases:
        before = dict(cover)
        for key, val in run_case(case, ar, cover).items():
            arrays[case["id"] + "." + key] = val
        per_case[case["id"]] = {k: int(cover[k] - before[k]) for k in COUNTED_KEYS if cover[k] != before[k]}
        print(case["id"], arrays[case["id"] + ".plane"].shape, per_case[case["id"]])
    tuples = weight_tuples()
    arrays["weights.in"], arrays["weights.out"] = tuples, reference_weights(tuples)
    doc = {"cases": cases, "coverage": {k: int(cover[k]) for k in COVERAGE_KEYS}, "coverage_per_case": per_case,
           "var_clamped_to_0": int(cover["var_clamped_to_0"]),
           "weights_sse_max": int(tuples[:, 6::4].max())}
    with open(os.path.join(HERE, "tffh_cases.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    G.write_npz(os.path.join(HERE, "tffh_cases.npz"), arrays)
    missing = [k for k in COVERAGE_KEYS if cover[k] == 0]
    if missing:
        sys.exit("coverage counts of 0: " + ", ".join(missing))


if __name__ == "__main__":
    main()
