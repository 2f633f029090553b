"""Time the 10-bit yuv temporal-filter calls for one window beside the 10-bit luma and the 8-bit yuv ones.

The window of scripts/tf_10bit_bench.py: 1920x1080, the centre picture and 6 references,
the controls of the TF level preset 8 uses (tests/golden/make_golden_tfsp.py
CONTROL_SETS["l8"]) with a luma decay factor of 2 000 000 and tf_mv_dist_th 64, plus chroma
decay factors of 3 000 000 (Cb) and 1 000 000 (Cr). Luma is the fractional-motion texture of
tests/tfsp_content.py as a 256x256 tile, repeated; Cb and Cr are the same texture from other
seeds as 128x128 tiles. Every 10-bit plane is its 8-bit plane << 2 with two seeded random bits
below. Each picture carries all five attachments: the MSB pyramid
(svtme_picture_upload_10bit), the 16-bit luma plane, the 16-bit chroma planes and, for the
8-bit yuv calls, the 8-bit chroma planes (the 16-bit ones >> 2).

In one process on the same resident pictures, by the host clock, the median of three runs of
`calls` calls each after a warm-up:
  1. svtme_tf_window_yuv_10bit into a fresh picture number with no host output, then
     svtme_sync (the result left resident);
  2. svtme_tf_window_10bit likewise;
  3. svtme_tf_window_yuv, the 8-bit call, likewise (it reads the MSB planes);
  4. svtme_tf_filter_yuv_10bit on the sub-pel results of the window, planes copied out;
  5. svtme_tf_filter_10bit on the same sub-pel results;
  6. svtme_tf_filter_yuv, the 8-bit call, on the same sub-pel results.
The 10-bit yuv window's outputs are compared with svtme_tf_filter_yuv_10bit's. The kernels'
own times need a kernel trace in a run of its own:
rocprofv3 --kernel-trace --stats -- python3 scripts/tf_10bit_chroma_bench.py 30 --no-write

Run on the GPU box: python3 scripts/tf_10bit_chroma_bench.py [calls] [--no-write] [--out DIR]
Writes DIR/tf_10bit_chroma_1080p.json (default profiles/tf_10bit_chroma) and prints it.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svt-av1-mirror_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import svtme as S  # noqa: E402
import make_golden_tfsp as G  # noqa: E402
import tfsp_content  # noqa: E402

W, H, TILE = 1920, 1080, 256
CW, CH = W // 2, H // 2
CENTRE, REFS = 8, (5, 6, 7, 9, 10, 11)
SET = "l8"
FILTER = {"tf_decay_factor_fp16": 2_000_000, "tf_mv_dist_th": 64}
CHROMA = {"tf_decay_factor_cb_fp16": 3_000_000, "tf_decay_factor_cr_fp16": 1_000_000}
OUT, OUT10, OUT8 = 100, 101, 102  # the result pictures' numbers


def tiled10(w, h, tile, seed, rng_base):
    """{t: [h][w] u16}: the texture of `seed` as tile x tile tiles, << 2, two seeded random bits below."""
    tiles = tfsp_content.fractional_frames(tile, tile, (CENTRE,) + REFS, seed=seed)
    reps = ((h + tile - 1) // tile, (w + tile - 1) // tile)
    out = {}
    for t, f in tiles.items():
        f8 = np.ascontiguousarray(np.tile(f, reps)[:h, :w])
        lsb = np.random.default_rng(rng_base + t).integers(0, 4, f8.shape, dtype=np.uint16)
        out[t] = (f8.astype(np.uint16) << 2) | lsb
    return out


def main():
    argv = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles", "tf_10bit_chroma")
    if "--out" in argv:
        out_dir = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    args = [a for a in argv if not a.startswith("--")]
    calls = int(args[0]) if args else 200
    import torch

    torch.cuda.set_device(0)
    gpu = S.GpuME(0)
    y = tiled10(W, H, TILE, 7, 900)
    cb, cr = tiled10(CW, CH, TILE // 2, 11, 1900), tiled10(CW, CH, TILE // 2, 13, 2900)
    for t, f in y.items():
        gpu.upload(t, f)
        gpu.attach_10bit(t, f)
        gpu.attach_chroma_10bit(t, cb[t], cr[t], W, H)
        gpu.upload_chroma(t, (cb[t] >> 2).astype(np.uint8), (cr[t] >> 2).astype(np.uint8), W, H)
    cs = G.CONTROL_SETS[SET]
    sp_ctl = G.subpel_controls(SET)
    luma = dict(FILTER, sub_sampling_shift=cs["sub_sampling_shift"])
    ctl = S.TfFilterControls.from_dict(luma)
    ctl_yuv = S.TfFilterYuvControls.from_dict(dict(luma, **CHROMA))
    me = S.derive_controls_tf(cs["hme_me_level"], 0, 35, S.input_resolution_of(W, H))
    jobs = [S.case_job(me, W, H, CENTRE, (r,), (), 0, me_type=S.ME_MCTF, tf_me_exit_th=cs["me_exit_th"]) for r in REFS]

    def window_yuv10(want):
        res = gpu.tf_window_yuv_10bit(jobs, W, H, sp_ctl, ctl_yuv, OUT, want=want)
        if not want:
            gpu.sync()
        return res

    def window10():
        gpu.tf_window_10bit(jobs, W, H, sp_ctl, ctl, OUT10, want=())
        gpu.sync()

    def window_yuv8():
        gpu.tf_window_yuv(jobs, W, H, sp_ctl, ctl_yuv, OUT8, want=())
        gpu.sync()

    def timed(fn, n):
        t0 = time.perf_counter()
        for _ in range(n):
            out = fn()
        return (time.perf_counter() - t0) * 1e3 / n, out

    def median_of_3(fn, n):
        timed(fn, 3)  # warm-up
        runs = [timed(fn, n) for _ in range(3)]
        return [round(ms, 4) for ms, _ in runs], runs[0][1]

    got = window_yuv10(("plane", "records", "subpel", "err32", "plane16", "cb", "cr"))
    sub = got["subpel"]
    wy10_runs, _ = median_of_3(lambda: window_yuv10(()), calls)
    w10_runs, _ = median_of_3(window10, calls)
    wy8_runs, _ = median_of_3(window_yuv8, calls)
    fy10_runs, (p16, c16b, c16r, e32) = median_of_3(lambda: gpu.tf_filter_yuv_10bit(CENTRE, REFS, W, H, ctl_yuv, sub), calls)
    f10_runs, _ = median_of_3(lambda: gpu.tf_filter_10bit(CENTRE, REFS, W, H, ctl, sub), calls)
    fy8_runs, _ = median_of_3(lambda: gpu.tf_filter_yuv(CENTRE, REFS, W, H, ctl_yuv, sub), calls)
    equal = {"plane16": bool(np.array_equal(got["plane16"], p16)), "cb": bool(np.array_equal(got["cb"], c16b)),
             "cr": bool(np.array_equal(got["cr"], c16r)), "err32": bool(np.array_equal(got["err32"], e32)),
             "plane": bool(np.array_equal(got["plane"], (p16 >> 2).astype(np.uint8)))}
    med = lambda runs: sorted(runs)[1]  # noqa: E731
    res = {
        "what": "svtme_tf_window_yuv_10bit and svtme_tf_filter_yuv_10bit, one 1080p window (centre + 6 references), TF "
                "level 8 controls plus chroma decay factors, beside svtme_tf_window_10bit / svtme_tf_filter_10bit and "
                "svtme_tf_window_yuv / svtme_tf_filter_yuv on the same resident pictures in the same process",
        "width": W, "height": H, "references": len(REFS), "sbs_per_reference": int(sub.shape[1]),
        "controls": ctl_yuv.as_dict(), "calls_per_run": calls,
        "tf_window_yuv_10bit_no_output_sync_ms_runs": wy10_runs, "tf_window_yuv_10bit_no_output_sync_ms": med(wy10_runs),
        "tf_window_10bit_no_output_sync_ms_runs": w10_runs, "tf_window_10bit_no_output_sync_ms": med(w10_runs),
        "tf_window_yuv_no_output_sync_ms_runs": wy8_runs, "tf_window_yuv_no_output_sync_ms": med(wy8_runs),
        "tf_filter_yuv_10bit_ms_runs": fy10_runs, "tf_filter_yuv_10bit_ms": med(fy10_runs),
        "tf_filter_10bit_ms_runs": f10_runs, "tf_filter_10bit_ms": med(f10_runs),
        "tf_filter_yuv_ms_runs": fy8_runs, "tf_filter_yuv_ms": med(fy8_runs),
        "window_equals_filter_yuv_10bit": equal,
        "samples_changed": {"y": int((got["plane16"] != y[CENTRE]).sum()), "cb": int((got["cb"] != cb[CENTRE]).sum()),
                            "cr": int((got["cr"] != cr[CENTRE]).sum())},
    }
    gpu.close()
    if "--no-write" not in sys.argv:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "tf_10bit_chroma_1080p.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
