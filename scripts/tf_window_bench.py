"""Time svtme_tf_window for one temporal-filtering window against the three calls it chains.

The window of scripts/tf_filter_bench.py: 1920x1080, the centre picture and 6
references, the controls of the TF level preset 8 uses
(tests/golden/make_golden_tfsp.py CONTROL_SETS["l8"]) with a luma decay factor of
2 000 000 and tf_mv_dist_th 64, the fractional-motion texture of
tests/tfsp_content.py as a 256x256 tile, repeated.

In one process, by the host clock, the median of three runs of `calls` calls each
after a warm-up:
  1. the three-call chain: the window's six TF-ME jobs (six synchronous
     submissions with their records copied out, as tf_filter_bench.py times them),
     svtme_tf_subpel on those records, svtme_tf_filter on its results; each
     stage's own time is reported beside the sum;
  2. svtme_tf_window into a fresh picture number with no host output, then
     svtme_sync;
  3. svtme_tf_window with the plane copied out;
  4. the same as 2 in place (the centre's own number); the pictures are uploaded
     again afterwards.
The window's outputs are compared with the chain's (records by the fields the
reference defines, the rest byte for byte). The kernels' own times need a kernel
trace in a run of its own:
rocprofv3 --kernel-trace --stats -- python3 scripts/tf_window_bench.py 30 --no-write

Run on the GPU box: python3 scripts/tf_window_bench.py [calls] [--no-write] [--out DIR]
Writes DIR/tf_window_1080p.json (default profiles/tf_window) and prints it.
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
OUT = 100  # the result picture's number


def window_frames():
    tiles = tfsp_content.fractional_frames(TILE, TILE, (CENTRE,) + REFS)
    reps = ((H + TILE - 1) // TILE, (W + TILE - 1) // TILE)
    return {t: np.ascontiguousarray(np.tile(f, reps)[:H, :W]) for t, f in tiles.items()}


def main():
    argv = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles", "tf_window")
    if "--out" in argv:
        out_dir = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    args = [a for a in argv if not a.startswith("--")]
    calls = int(args[0]) if args else 300
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

    def chain():
        recs = tf_me()
        sub = gpu.tf_subpel(CENTRE, REFS, W, H, sp_ctl, recs)
        plane, err32 = gpu.tf_filter(CENTRE, REFS, Wa, Ha, ctl, sub)
        return {"plane": plane[:H, :W], "records": recs, "subpel": sub, "err32": err32}

    def window(out_pn, want):
        res = gpu.tf_window(jobs, W, H, sp_ctl, ctl, out_pn, want=want)
        if not want:
            gpu.sync()
        return res

    def timed(fn, n):
        t0 = time.perf_counter()
        for _ in range(n):
            out = fn()
        return (time.perf_counter() - t0) * 1e3 / n, out

    def median_of_3(fn, n):
        timed(fn, 3)  # warm-up
        runs = [timed(fn, n) for _ in range(3)]
        return [round(ms, 4) for ms, _ in runs], runs[0][1]

    me_runs, recs = median_of_3(tf_me, calls)
    sp_runs, sub = median_of_3(lambda: gpu.tf_subpel(CENTRE, REFS, W, H, sp_ctl, recs), calls)
    f_runs, _ = median_of_3(lambda: gpu.tf_filter(CENTRE, REFS, Wa, Ha, ctl, sub), calls)
    c_runs, want = median_of_3(chain, calls)
    w_runs, _ = median_of_3(lambda: window(OUT, ()), calls)
    p_runs, _ = median_of_3(lambda: window(OUT, ("plane",)), calls)
    got = window(OUT, ("plane", "records", "subpel", "err32"))
    equal = {"records": S.compare_records(want["records"].reshape(-1, 1), got["records"].reshape(-1, 1)) == [],
             "subpel": got["subpel"].tobytes() == want["subpel"].tobytes(),
             "err32": bool(np.array_equal(got["err32"], want["err32"])),
             "plane": bool(np.array_equal(got["plane"], want["plane"]))}
    # in place last: every call filters the centre again, so the pictures' content drifts (the work
    # per call does not: the grids depend on the size alone)
    i_runs, _ = median_of_3(lambda: window(CENTRE, ()), calls)
    gpu.upload(CENTRE, frames[CENTRE])
    src = frames[CENTRE]
    med = lambda runs: sorted(runs)[1]  # noqa: E731
    res = {
        "what": "svtme_tf_window, one 1080p window (centre + 6 references) in one call, TF level 8 controls, against "
                "the three calls it chains (six TF-ME submissions, svtme_tf_subpel, svtme_tf_filter) in the same process",
        "width": W, "height": H, "references": len(REFS), "sbs_per_reference": int(sub.shape[1]),
        "controls": ctl.as_dict(), "calls_per_run": calls,
        "three_calls_ms_runs": c_runs, "three_calls_ms": med(c_runs),
        "three_calls_stages_ms": {"tf_me_6_jobs": med(me_runs), "tf_subpel": med(sp_runs), "tf_filter": med(f_runs)},
        "tf_window_no_output_sync_ms_runs": w_runs, "tf_window_no_output_sync_ms": med(w_runs),
        "tf_window_plane_out_ms_runs": p_runs, "tf_window_plane_out_ms": med(p_runs),
        "tf_window_in_place_no_output_sync_ms_runs": i_runs, "tf_window_in_place_no_output_sync_ms": med(i_runs),
        "speedup_no_output": round(med(c_runs) / med(w_runs), 3),
        "speedup_plane_out": round(med(c_runs) / med(p_runs), 3),
        "window_equals_three_calls": equal,
        "host_bytes_three_calls": int(2 * recs.nbytes + 2 * sub.nbytes + Wa * Ha + want["err32"].nbytes),
        "host_bytes_window_plane_out": int(W * H),
        "pixels_changed": int((got["plane"] != src).sum()),
    }
    gpu.close()
    if "--no-write" not in sys.argv:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "tf_window_1080p.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
