"""Time the chroma stage of temporal filtering: svtme_tf_filter_yuv and svtme_tf_window_yuv
beside the luma-only calls, and the luma-only calls of this build against another build.

The window of scripts/tf_window_bench.py: 1920x1080, the centre
picture and 6 references, the controls of TF level 8 with a luma decay factor of
2 000 000 and tf_mv_dist_th 64; the chroma decay factors are 2 000 000 too, the chroma
planes a fractional-motion texture of their own (128x128 tiles, repeated).

Default mode, in one process, by the host clock, the median of three runs of `calls`
calls each after a warm-up:
  svtme_tf_filter, svtme_tf_filter_yuv (all planes copied out), svtme_tf_window and
  svtme_tf_window_yuv (no host output, then svtme_sync), svtme_tf_window_yuv with the
  three planes copied out. The yuv calls' luma is compared with the luma-only calls',
  the window's chroma with the filter's.
The kernels' own times need a kernel trace in a run of its own:
rocprofv3 --kernel-trace --stats -- python3 scripts/tf_chroma_bench.py 30 --no-write

--luma-runs   three runs of svtme_tf_filter and of svtme_tf_window with the library
              SVTME_LIB names (default: this build's), printed as JSON.
--luma-ab LIB the same for the build LIB (the parent commit's library) and for this
              build, each in a process of its own, one after the other, twice in turn;
              writes DIR/luma_ab.json with both sets of runs and the verdict: this build
              is not slower than LIB's slowest run by more than LIB's own min-max spread.

Run on the GPU box: python3 scripts/tf_chroma_bench.py [calls] [--no-write] [--out DIR]
Writes DIR/tf_chroma_1080p.json (default profiles/tf_chroma) and prints it.
"""
import json
import os
import subprocess
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
CHROMA = {"tf_decay_factor_cb_fp16": 2_000_000, "tf_decay_factor_cr_fp16": 2_000_000}
OUT = 100  # the result picture's number


def tiled(w, h, tile, seed):
    tiles = tfsp_content.fractional_frames(tile, tile, (CENTRE,) + REFS, seed=seed)
    reps = ((h + tile - 1) // tile, (w + tile - 1) // tile)
    return {t: np.ascontiguousarray(np.tile(f, reps)[:h, :w]) for t, f in tiles.items()}


def timed(fn, n):
    t0 = time.perf_counter()
    for _ in range(n):
        out = fn()
    return (time.perf_counter() - t0) * 1e3 / n, out


def three_runs(fn, n):
    timed(fn, 3)  # warm-up
    runs = [timed(fn, n) for _ in range(3)]
    return [round(ms, 4) for ms, _ in runs], runs[0][1]


def med(runs):
    return sorted(runs)[1]


class Window:
    def __init__(self, chroma: bool):
        import torch

        torch.cuda.set_device(0)
        self.gpu = S.GpuME(0)
        for t, f in tiled(W, H, TILE, 7).items():
            self.gpu.upload(t, f)
        if chroma:
            cb, cr = tiled(W // 2, H // 2, TILE // 2, 11), tiled(W // 2, H // 2, TILE // 2, 13)
            for t in cb:
                self.gpu.upload_chroma(t, cb[t], cr[t], W, H)
        cs = G.CONTROL_SETS[SET]
        self.sp_ctl = G.subpel_controls(SET)
        luma = dict(FILTER, sub_sampling_shift=cs["sub_sampling_shift"])
        self.ctl = S.TfFilterControls.from_dict(luma)
        self.yuv_ctl = S.TfFilterYuvControls.from_dict(dict(luma, **CHROMA)) if chroma else None
        me = S.derive_controls_tf(cs["hme_me_level"], 0, 35, S.input_resolution_of(W, H))
        self.jobs = [S.case_job(me, W, H, CENTRE, (r,), (), 0, me_type=S.ME_MCTF, tf_me_exit_th=cs["me_exit_th"])
                     for r in REFS]
        recs = np.ascontiguousarray(np.stack([self.gpu.submit(j, with_sb_results=False)[0][:, 0] for j in self.jobs]))
        self.sub = self.gpu.tf_subpel(CENTRE, REFS, W, H, self.sp_ctl, recs)

    def tf_filter(self):
        return self.gpu.tf_filter(CENTRE, REFS, S.align8(W), S.align8(H), self.ctl, self.sub)

    def tf_filter_yuv(self):
        return self.gpu.tf_filter_yuv(CENTRE, REFS, W, H, self.yuv_ctl, self.sub)

    def tf_window(self, want=()):
        res = self.gpu.tf_window(self.jobs, W, H, self.sp_ctl, self.ctl, OUT, want=want)
        if not want:
            self.gpu.sync()
        return res

    def tf_window_yuv(self, want=()):
        res = self.gpu.tf_window_yuv(self.jobs, W, H, self.sp_ctl, self.yuv_ctl, OUT, want=want)
        if not want:
            self.gpu.sync()
        return res


def luma_runs(calls: int) -> dict:
    win = Window(chroma=False)
    f_runs, _ = three_runs(win.tf_filter, calls)
    w_runs, _ = three_runs(win.tf_window, calls)
    win.gpu.close()
    return {"library": os.path.basename(S.product_lib_path()), "calls_per_run": calls, "tf_filter_ms_runs": f_runs,
            "tf_window_no_output_sync_ms_runs": w_runs}


def luma_ab(parent_lib: str, calls: int) -> dict:
    def child(lib):
        env = dict(os.environ, SVTME_LIB=lib)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), str(calls), "--luma-runs"], env=env, check=True,
                             capture_output=True, text=True, timeout=600).stdout
        return json.loads(out.strip().splitlines()[-1])

    this_lib = os.path.join(ROOT, "svt-av1-mirror_amd", "libsvtme.so")
    sets = {"parent": [], "this": []}
    for _ in range(2):  # parent, this, parent, this: the session's drift falls on both
        sets["parent"].append(child(parent_lib))
        sets["this"].append(child(this_lib))
    res = {"what": "svtme_tf_filter and svtme_tf_window (no host output, then svtme_sync) on the 1080p window of "
                   "scripts/tf_window_bench.py, the parent commit's library against this build's, each process "
                   "three runs, ms per call by the host clock, in one GPU session",
           "calls_per_run": calls, "sets": sets, "verdict": {}}
    for key in ("tf_filter_ms_runs", "tf_window_no_output_sync_ms_runs"):
        p = [v for s in sets["parent"] for v in s[key]]
        t = [v for s in sets["this"] for v in s[key]]
        # the condition is on three runs of each: the first process of each side; the second is shown beside it
        p3, t3 = sets["parent"][0][key], sets["this"][0][key]
        bound = max(p3) + (max(p3) - min(p3))
        res["verdict"][key] = {"parent_runs": p3, "this_runs": t3, "parent_slowest": max(p3),
                               "parent_spread": round(max(p3) - min(p3), 4), "bound": round(bound, 4),
                               "this_median": med(t3), "this_slowest": max(t3), "not_slower": max(t3) <= bound,
                               "all_parent_runs": p, "all_this_runs": t}
    return res


def main():
    argv = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles", "tf_chroma")
    if "--out" in argv:
        out_dir = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    parent_lib = None
    if "--luma-ab" in argv:
        parent_lib = os.path.abspath(argv[argv.index("--luma-ab") + 1])
        del argv[argv.index("--luma-ab"):argv.index("--luma-ab") + 2]
    args = [a for a in argv if not a.startswith("--")]
    calls = int(args[0]) if args else 300
    name = "tf_chroma_1080p.json"
    if "--luma-runs" in argv:
        print(json.dumps(luma_runs(calls)))
        return
    if parent_lib:
        res, name = luma_ab(parent_lib, calls), "luma_ab.json"
    else:
        win = Window(chroma=True)
        f_runs, (y0, e0) = three_runs(win.tf_filter, calls)
        fy_runs, (y1, cb1, cr1, e1) = three_runs(win.tf_filter_yuv, calls)
        w_runs, _ = three_runs(win.tf_window, calls)
        wy_runs, _ = three_runs(win.tf_window_yuv, calls)
        wp_runs, _ = three_runs(lambda: win.tf_window(("plane",)), calls)
        wyp_runs, got = three_runs(lambda: win.tf_window_yuv(("plane", "cb", "cr")), calls)
        equal = {"filter_yuv_luma_is_tf_filter": bool(np.array_equal(y1, y0[:H, :W]) and np.array_equal(e1, e0)),
                 "window_yuv_luma_is_filter_yuv": bool(np.array_equal(got["plane"], y1)),
                 "window_yuv_chroma_is_filter_yuv": bool(np.array_equal(got["cb"], cb1) and np.array_equal(got["cr"], cr1))}
        res = {
            "what": "the chroma stage of temporal filtering on one 1080p window (centre + 6 references, 8-bit 4:2:0), TF "
                    "level 8 controls, beside the luma-only calls in the same process; ms per call, medians of three runs",
            "width": W, "height": H, "references": len(REFS), "controls": win.yuv_ctl.as_dict(), "calls_per_run": calls,
            "tf_filter_ms_runs": f_runs, "tf_filter_ms": med(f_runs),
            "tf_filter_yuv_ms_runs": fy_runs, "tf_filter_yuv_ms": med(fy_runs),
            "tf_window_no_output_sync_ms_runs": w_runs, "tf_window_no_output_sync_ms": med(w_runs),
            "tf_window_yuv_no_output_sync_ms_runs": wy_runs, "tf_window_yuv_no_output_sync_ms": med(wy_runs),
            "tf_window_plane_out_ms_runs": wp_runs, "tf_window_plane_out_ms": med(wp_runs),
            "tf_window_yuv_planes_out_ms_runs": wyp_runs, "tf_window_yuv_planes_out_ms": med(wyp_runs),
            "chroma_cost_filter_ms": round(med(fy_runs) - med(f_runs), 4),
            "chroma_cost_window_ms": round(med(wy_runs) - med(w_runs), 4),
            "equal": equal,
            "chroma_pixels_changed": int((cb1 != tiled(W // 2, H // 2, TILE // 2, 11)[CENTRE]).sum()),
        }
        win.gpu.close()
    if "--no-write" not in sys.argv:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, name), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
