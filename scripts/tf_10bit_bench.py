"""Time the 10-bit temporal-filter calls for one window beside the 8-bit ones.

The window of scripts/tf_window_bench.py: 1920x1080, the centre picture and 6
references, the controls of the TF level preset 8 uses
(tests/golden/make_golden_tfsp.py CONTROL_SETS["l8"]) with a luma decay factor of
2 000 000 and tf_mv_dist_th 64, the fractional-motion texture of
tests/tfsp_content.py as a 256x256 tile, repeated. The 10-bit pictures are that
texture << 2 with two seeded random bits below, uploaded with
svtme_picture_upload_10bit (the MSB plane is the 8-bit window's picture) and attached
with svtme_picture_attach_10bit.

In one process, by the host clock, the median of three runs of `calls` calls each
after a warm-up:
  1. svtme_tf_window_10bit into a fresh picture number with no host output, then
     svtme_sync (the result left resident);
  2. svtme_tf_filter_10bit on the sub-pel results of the window, plane copied out;
  3. svtme_tf_window, the 8-bit call, on the same pictures (it reads the MSB planes),
     left resident;
  4. svtme_tf_filter, the 8-bit call, on the same sub-pel results.
The 10-bit window's outputs are compared with svtme_tf_filter_10bit's. The kernels'
own times need a kernel trace in a run of its own:
rocprofv3 --kernel-trace --stats -- python3 scripts/tf_10bit_bench.py 30 --no-write

Run on the GPU box: python3 scripts/tf_10bit_bench.py [calls] [--no-write] [--out DIR]
Writes DIR/tf_10bit_1080p.json (default profiles/tf_10bit) and prints it.
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
CENTRE, REFS = 8, (5, 6, 7, 9, 10, 11)
SET = "l8"
FILTER = {"tf_decay_factor_fp16": 2_000_000, "tf_mv_dist_th": 64}
OUT, OUT8 = 100, 101  # the result pictures' numbers


def window_frames():
    tiles = tfsp_content.fractional_frames(TILE, TILE, (CENTRE,) + REFS)
    reps = ((H + TILE - 1) // TILE, (W + TILE - 1) // TILE)
    out = {}
    for t, f in tiles.items():
        f8 = np.ascontiguousarray(np.tile(f, reps)[:H, :W])
        lsb = np.random.default_rng(900 + t).integers(0, 4, f8.shape, dtype=np.uint16)
        out[t] = (f8.astype(np.uint16) << 2) | lsb
    return out


def main():
    argv = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles", "tf_10bit")
    if "--out" in argv:
        out_dir = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    args = [a for a in argv if not a.startswith("--")]
    calls = int(args[0]) if args else 300
    import torch

    torch.cuda.set_device(0)
    gpu = S.GpuME(0)
    frames = window_frames()

    def upload_all():
        for t, f in frames.items():
            gpu.upload(t, f)
            gpu.attach_10bit(t, f)

    upload_all()
    cs = G.CONTROL_SETS[SET]
    sp_ctl = G.subpel_controls(SET)
    ctl = S.TfFilterControls.from_dict(dict(FILTER, sub_sampling_shift=cs["sub_sampling_shift"]))
    me = S.derive_controls_tf(cs["hme_me_level"], 0, 35, S.input_resolution_of(W, H))
    jobs = [S.case_job(me, W, H, CENTRE, (r,), (), 0, me_type=S.ME_MCTF, tf_me_exit_th=cs["me_exit_th"]) for r in REFS]

    def window10(out_pn, want):
        res = gpu.tf_window_10bit(jobs, W, H, sp_ctl, ctl, out_pn, want=want)
        if not want:
            gpu.sync()
        return res

    def window8(out_pn):
        gpu.tf_window(jobs, W, H, sp_ctl, ctl, out_pn, want=())
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

    got = window10(OUT, ("plane", "records", "subpel", "err32", "plane16"))
    sub = got["subpel"]
    w10_runs, _ = median_of_3(lambda: window10(OUT, ()), calls)
    f10_runs, (p16, e32) = median_of_3(lambda: gpu.tf_filter_10bit(CENTRE, REFS, W, H, ctl, sub), calls)
    w8_runs, _ = median_of_3(lambda: window8(OUT8), calls)
    f8_runs, _ = median_of_3(lambda: gpu.tf_filter(CENTRE, REFS, W, H, ctl, sub), calls)
    equal = {"plane16": bool(np.array_equal(got["plane16"], p16)), "err32": bool(np.array_equal(got["err32"], e32)),
             "plane": bool(np.array_equal(got["plane"], (p16 >> 2).astype(np.uint8)))}
    med = lambda runs: sorted(runs)[1]  # noqa: E731
    res = {
        "what": "svtme_tf_window_10bit and svtme_tf_filter_10bit, one 1080p window (centre + 6 references), TF level 8 "
                "controls, beside svtme_tf_window and svtme_tf_filter on the same pictures in the same process",
        "width": W, "height": H, "references": len(REFS), "sbs_per_reference": int(sub.shape[1]),
        "controls": ctl.as_dict(), "calls_per_run": calls,
        "tf_window_10bit_no_output_sync_ms_runs": w10_runs, "tf_window_10bit_no_output_sync_ms": med(w10_runs),
        "tf_filter_10bit_ms_runs": f10_runs, "tf_filter_10bit_ms": med(f10_runs),
        "tf_window_no_output_sync_ms_runs": w8_runs, "tf_window_no_output_sync_ms": med(w8_runs),
        "tf_filter_ms_runs": f8_runs, "tf_filter_ms": med(f8_runs),
        "window_equals_filter_10bit": equal,
        "samples_changed": int((got["plane16"] != frames[CENTRE]).sum()),
    }
    gpu.close()
    if "--no-write" not in sys.argv:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "tf_10bit_1080p.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
