"""Time svtme_tf_filter for one temporal-filtering window, after the two calls that feed it.

1920x1080, the centre picture and 6 references, the controls of the TF level
preset 8 uses (tests/golden/make_golden_tfsp.py CONTROL_SETS["l8"]:
sub_sampling_shift 1) with a typical luma decay factor (2 000 000) and
tf_mv_dist_th 64. The content is the fractional-motion texture of
tests/tfsp_content.py, made as a 256x256 tile and repeated. The chain is the
library's own: the TF-ME jobs of the window, svtme_tf_subpel on their records,
svtme_tf_filter on its results; the first two are run once before the timed
calls of the third, and timed too, for the whole inner loop of a window.

Reports ms per call by the host clock around synchronous calls (the upload of
the sub-pel results, two launches, the kernels, the copy-out of the plane and of
err32, the synchronisation). The kernels' own times need a kernel trace in a run
of its own:
rocprofv3 --kernel-trace --stats -- python3 scripts/tf_filter_bench.py 30 --no-write
With --check the first reference alone (n = 1) is compared with the numpy model
of tests/tff_model.py: plane and err32.

Run on the GPU box: python3 scripts/tf_filter_bench.py [calls] [--check] [--no-write] [--out DIR]
Writes DIR/tf_filter_1080p.json (default profiles/tf_filter) and prints it.
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


def window_frames():
    tiles = tfsp_content.fractional_frames(TILE, TILE, (CENTRE,) + REFS)
    reps = ((H + TILE - 1) // TILE, (W + TILE - 1) // TILE)
    return {t: np.ascontiguousarray(np.tile(f, reps)[:H, :W]) for t, f in tiles.items()}


def main():
    argv = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles", "tf_filter")
    if "--out" in argv:
        out_dir = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    args = [a for a in argv if not a.startswith("--")]
    calls = int(args[0]) if args else 100
    import torch

    torch.cuda.set_device(0)
    gpu = S.GpuME(0)
    frames = window_frames()
    for t, f in frames.items():
        gpu.upload(t, f)
    cs = G.CONTROL_SETS[SET]
    sp_ctl = G.subpel_controls(SET)
    ctl = S.TfFilterControls.from_dict(dict(FILTER, sub_sampling_shift=cs["sub_sampling_shift"]))
    me = S.derive_controls_tf(cs["hme_me_level"], 0, 35, S.input_resolution_of(W, H))
    jobs = [S.case_job(me, W, H, CENTRE, (r,), (), 0, me_type=S.ME_MCTF, tf_me_exit_th=cs["me_exit_th"]) for r in REFS]
    Wa, Ha = S.align8(W), S.align8(H)

    def tf_me():
        return np.ascontiguousarray(np.stack([gpu.submit(j, with_sb_results=False)[0][:, 0] for j in jobs]))

    def timed(fn, n):
        t0 = time.perf_counter()
        for _ in range(n):
            out = fn()
        return (time.perf_counter() - t0) * 1e3 / n, out

    def median_of_3(fn, n):
        timed(fn, 3)  # warm-up
        runs = [timed(fn, n) for _ in range(3)]
        return [round(ms, 4) for ms, _ in runs], runs[0][1]

    me_runs, recs = median_of_3(tf_me, max(calls // 10, 3))
    sp_runs, sub = median_of_3(lambda: gpu.tf_subpel(CENTRE, REFS, W, H, sp_ctl, recs), calls)
    f_runs, (plane, err32) = median_of_3(lambda: gpu.tf_filter(CENTRE, REFS, Wa, Ha, ctl, sub), calls)
    n1_runs, (plane1, err1) = median_of_3(lambda: gpu.tf_filter(CENTRE, REFS[:1], Wa, Ha, ctl, sub[:1]), calls)
    src = frames[CENTRE]
    res = {
        "what": "svtme_tf_filter, one 1080p window (centre + 6 references) in one call, TF level 8 controls, "
                "after the window's TF-ME jobs and svtme_tf_subpel",
        "width": W, "height": H, "references": len(REFS), "sbs_per_reference": int(sub.shape[1]),
        "controls": ctl.as_dict(), "calls_per_run": calls,
        "tf_filter_ms_per_call_runs": f_runs, "tf_filter_ms_per_call": sorted(f_runs)[1],
        "tf_filter_one_reference_ms_per_call": sorted(n1_runs)[1],
        "tf_subpel_ms_per_call": sorted(sp_runs)[1],
        "tf_me_6_jobs_ms": sorted(me_runs)[1],
        "window_ms_tf_me_subpel_filter": round(sorted(me_runs)[1] + sorted(sp_runs)[1] + sorted(f_runs)[1], 4),
        "bytes_to_device_per_call": int(sub.nbytes), "bytes_to_host_per_call": int(Wa * Ha + err32.nbytes),
        "branches": {name: int((sub["branch"] == v).sum()) for name, v in
                     (("64_only", S.TFSP_64_ONLY), ("64_chosen", S.TFSP_64_CHOSEN), ("32", S.TFSP_32))},
        "pixels_changed": int((plane[:H, :W] != src).sum()),
        "mean_abs_change": round(float(np.abs(plane[:H, :W].astype(np.int32) - src).mean()), 4),
    }
    gpu.close()
    if "--check" in sys.argv:
        import tff_model as M

        pyr = {t: S.build_host_pyramid(frames[t], "oracle") for t in (CENTRE, REFS[0])}
        want, want_err, _, _ = M.filter_window(pyr[CENTRE], [pyr[REFS[0]]], ctl.as_dict(), sub[:1])
        res["one_reference_matches_model"] = bool(np.array_equal(want, plane1) and np.array_equal(want_err, err1))
    if "--no-write" not in sys.argv:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "tf_filter_1080p.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
