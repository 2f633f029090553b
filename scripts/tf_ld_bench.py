"""Time the low-delay temporal-filter calls (svtme_tf_window_ld, svtme_tf_filter_ld) beside the matching
svtme_tf_window* call and a device-to-device copy of the same number of bytes.

Shapes: 1920x1080 and 3840x2160, the centre picture with 1 and with 6 references, in the four modes (8 / 10
bit, luma alone / with 4:2:0 chroma). Luma is the fractional-motion texture of tests/tfsp_content.py as a
256x256 tile, repeated; Cb and Cr the same texture from other seeds as 128x128 tiles; every 10-bit plane is
its 8-bit plane << 2 with two seeded random bits below. Each picture carries all five attachments (the MSB
pyramid, the 16-bit luma plane, the 16-bit chroma planes, the 8-bit chroma planes), so the four modes and the
four existing window calls read the same resident pictures in one process. Decay factors: 150 << 10 (Y),
600 << 10 (Cb), 20 << 10 (Cr); sub_sampling_shift 1.

By the host clock, the median of three runs of `calls` calls each after a warm-up, per shape and mode:
  1. svtme_tf_window_ld into a fresh picture number with no host output, then svtme_sync (left resident);
  2. svtme_tf_window_ld with y (and cb, cr) copied out;
  3. svtme_tf_filter_ld, planes and variances copied out;
  4. for context the matching svtme_tf_window / _yuv / _10bit / _yuv_10bit call (TF level 8 controls: it
     runs the TF-ME batch and the sub-pel search the low-delay path does not have), no host output, then sync;
  5. the yardstick of the fused kernel, which moves (n + 1) plane reads and one write and does almost no
     arithmetic: hipMemcpyAsync device to device of HALF that many bytes, which reads and writes the same
     total, and of all of them; `calls` copies queued, then one synchronise.
The byte counts are computed here from the shapes (at 10 bit the kernel also writes level 0, one byte a luma
sample). The kernel's own time needs a kernel trace in a run of its own:
  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 scripts/tf_ld_bench.py 20 --trace
runs only the `calls` resident window calls of each shape and mode, in the order of SHAPES x MODES, and
  python3 scripts/tf_ld_bench.py 20 --summarise DIR/.../run_kernel_trace.csv [--copies FILE.json]
reads the median duration of k_tfld per shape and mode from it and, given the JSON of a plain run, the ratio
to the copy.

--shape WxH:n (e.g. 3840x2160:6) keeps that shape alone, for a counter run of its own:
  rocprofv3 --pmc SQ_WAVES SQ_BUSY_CYCLES ... -d DIR -o run --output-format csv -- \
      python3 scripts/tf_ld_bench.py 5 --trace --shape 3840x2160:6

Run on the GPU box: python3 scripts/tf_ld_bench.py [calls] [--no-write] [--out DIR]
Writes DIR/tf_ld.json (default profiles/tf_ld) and prints it.
"""
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svt-av1-mirror_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

TILE = 256
CENTRE, REFS = 8, (7, 6, 5, 9, 10, 11)
SIZES = ((1920, 1080), (3840, 2160))
SHAPES = [(w, h, n) for w, h in SIZES for n in (1, 6)]
MODES = ((8, 0), (8, 1), (10, 0), (10, 1))
DECAYS = [150 << 10, 600 << 10, 20 << 10]
SET = "l8"
OUT = 100


def key(w, h, n, bd, chroma):
    return f"{w}x{h}_n{n}_{bd}bit{'_yuv' if chroma else ''}"


def kernel_bytes(w, h, n, bd, chroma):
    """What k_tfld reads and writes for one window: (n + 1) reads and one write of each plane it filters, of
    the aligned size; at 10 bit level 0 too."""
    W, H = (w + 7) & ~7, (h + 7) & ~7
    plane = W * H * (2 if bd == 10 else 1) * (3 if chroma else 2) // 2
    return (n + 2) * plane + (W * H if bd == 10 else 0)


def summarise(path, calls, copies):
    rows = [r for r in csv.DictReader(open(path)) if "k_tfld" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    combos = [(w, h, n, bd, c) for w, h, n in SHAPES for bd, c in MODES]
    assert len(rows) == len(combos) * (calls + 3), (len(rows), len(combos), calls)
    out = {}
    for k, (w, h, n, bd, c) in enumerate(combos):
        grp = rows[k * (calls + 3) + 3:(k + 1) * (calls + 3)]  # after the warm-up's three
        d = sorted((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in grp)
        e = {"kernel": grp[0]["Kernel_Name"], "k_tfld_us_median": round(d[len(d) // 2], 2), "k_tfld_us_min": round(d[0], 2),
             "k_tfld_us_max": round(d[-1], 2), "bytes_moved": kernel_bytes(w, h, n, bd, c)}
        e["gb_per_s"] = round(e["bytes_moved"] / e["k_tfld_us_median"] / 1e3, 1)
        if copies:
            cp = copies["shapes"][key(w, h, n, bd, c)]
            e["copy_same_total_us"] = cp["copy_half_bytes_us"]
            e["ratio_to_copy_same_total"] = round(e["k_tfld_us_median"] / cp["copy_half_bytes_us"], 3)
            e["ratio_to_copy_of_all_bytes"] = round(e["k_tfld_us_median"] / cp["copy_all_bytes_us"], 3)
        out[key(w, h, n, bd, c)] = e
    return out


def main():
    argv = sys.argv[1:]
    out_dir = os.path.join(ROOT, "profiles", "tf_ld")
    if "--out" in argv:
        out_dir = argv[argv.index("--out") + 1]
        del argv[argv.index("--out"):argv.index("--out") + 2]
    copies = None
    if "--copies" in argv:
        copies = json.load(open(argv[argv.index("--copies") + 1]))
        del argv[argv.index("--copies"):argv.index("--copies") + 2]
    trace_csv = None
    if "--summarise" in argv:
        trace_csv = argv[argv.index("--summarise") + 1]
        del argv[argv.index("--summarise"):argv.index("--summarise") + 2]
    global SIZES, SHAPES
    if "--shape" in argv:  # WxH:n, e.g. 3840x2160:6: that shape alone (a counter run)
        size, n = argv[argv.index("--shape") + 1].split(":")
        del argv[argv.index("--shape"):argv.index("--shape") + 2]
        SIZES = (tuple(int(v) for v in size.split("x")),)
        SHAPES = [SIZES[0] + (int(n),)]
    args = [a for a in argv if not a.startswith("--")]
    calls = int(args[0]) if args else 50
    if trace_csv:
        res = {"what": "k_tfld per window from a rocprofv3 kernel trace of scripts/tf_ld_bench.py --trace",
               "calls_per_shape": calls, "shapes": summarise(trace_csv, calls, copies)}
        if "--no-write" not in sys.argv:
            os.makedirs(out_dir, exist_ok=True)
            with open(os.path.join(out_dir, "tf_ld_kernel.json"), "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        print(json.dumps(res))
        return
    trace = "--trace" in argv

    import torch

    import make_golden_tfsp as G
    import svtme as S
    import tfsp_content

    torch.cuda.set_device(0)
    gpu = S.GpuME(0)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipDeviceSynchronize.argtypes = []
    D2D = 3  # hipMemcpyDeviceToDevice

    def tiled10(w, h, tile, seed, rng_base):
        tiles = tfsp_content.fractional_frames(tile, tile, (CENTRE,) + REFS, seed=seed)
        reps = ((h + tile - 1) // tile, (w + tile - 1) // tile)
        out = {}
        for t, f in tiles.items():
            f8 = np.ascontiguousarray(np.tile(f, reps)[:h, :w])
            lsb = np.random.default_rng(rng_base + t).integers(0, 4, f8.shape, dtype=np.uint16)
            out[t] = (f8.astype(np.uint16) << 2) | lsb
        return out

    def timed(fn, n):
        t0 = time.perf_counter()
        for _ in range(n):
            out = fn()
        return (time.perf_counter() - t0) * 1e3 / n, out

    def median_of_3(fn, n):
        timed(fn, 3)  # warm-up
        runs = sorted(round(timed(fn, n)[0], 4) for _ in range(3))
        return {"ms": runs[1], "ms_runs": runs}

    def copy_us(nbytes, src, dst):
        def batch():
            for _ in range(calls):
                assert hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, D2D, None) == 0
            assert hip.hipDeviceSynchronize() == 0
        batch()
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            batch()
            runs.append((time.perf_counter() - t0) * 1e6 / calls)
        return round(sorted(runs)[1], 2)

    shapes = {}
    for w, h in SIZES:
        y = tiled10(w, h, TILE, 7, 900)
        cb, cr = tiled10(w // 2, h // 2, TILE // 2, 11, 1900), tiled10(w // 2, h // 2, TILE // 2, 13, 2900)
        for t, f in y.items():
            gpu.upload(t, f)
            gpu.attach_10bit(t, f)
            gpu.attach_chroma_10bit(t, cb[t], cr[t], w, h)
            gpu.upload_chroma(t, (cb[t] >> 2).astype(np.uint8), (cr[t] >> 2).astype(np.uint8), w, h)
        W, H = S.align8(w), S.align8(h)
        cs = G.CONTROL_SETS[SET]
        sp_ctl = G.subpel_controls(SET)
        luma = {"tf_decay_factor_fp16": 2_000_000, "tf_mv_dist_th": 64, "sub_sampling_shift": cs["sub_sampling_shift"]}
        f_ctl = S.TfFilterControls.from_dict(luma)
        f_yuv = S.TfFilterYuvControls.from_dict(dict(luma, tf_decay_factor_cb_fp16=3_000_000, tf_decay_factor_cr_fp16=1_000_000))
        me = S.derive_controls_tf(cs["hme_me_level"], 0, 35, S.input_resolution_of(w, h))
        biggest = kernel_bytes(w, h, 6, 10, 1)
        src = torch.randint(0, 255, (biggest,), dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        for n in [s[2] for s in SHAPES if s[:2] == (w, h)]:
            refs = list(REFS[:n])
            jobs = [S.case_job(me, w, h, CENTRE, (r,), (), 0, me_type=S.ME_MCTF, tf_me_exit_th=cs["me_exit_th"]) for r in refs]
            for bd, chroma in MODES:
                ctl = S.TfLdControls.from_dict({"tf_decay_factor_fp16": DECAYS, "sub_sampling_shift": 1, "bit_depth": bd,
                                                "chroma": chroma})
                planes = ("y", "cb", "cr") if chroma else ("y",)

                def resident():
                    gpu.tf_window_ld(CENTRE, refs, w, h, ctl, OUT)
                    gpu.sync()

                if trace:
                    timed(resident, 3)
                    timed(resident, calls)
                    continue
                existing = {(8, 0): lambda: gpu.tf_window(jobs, w, h, sp_ctl, f_ctl, OUT + 1, want=()),
                            (8, 1): lambda: gpu.tf_window_yuv(jobs, w, h, sp_ctl, f_yuv, OUT + 1, want=()),
                            (10, 0): lambda: gpu.tf_window_10bit(jobs, w, h, sp_ctl, f_ctl, OUT + 1, want=()),
                            (10, 1): lambda: gpu.tf_window_yuv_10bit(jobs, w, h, sp_ctl, f_yuv, OUT + 1, want=())}[(bd, chroma)]

                def existing_sync():
                    existing()
                    gpu.sync()

                nbytes = kernel_bytes(w, h, n, bd, chroma)
                e = {"bytes_moved": nbytes,
                     "tf_window_ld_resident": median_of_3(resident, calls),
                     "tf_window_ld_planes_out": median_of_3(lambda: gpu.tf_window_ld(CENTRE, refs, w, h, ctl, OUT, want=planes), calls),
                     "tf_filter_ld": median_of_3(lambda: gpu.tf_filter_ld(CENTRE, refs, W, H, ctl), calls),
                     "matching_tf_window_resident": median_of_3(existing_sync, max(calls // 5, 3)),
                     "copy_half_bytes_us": copy_us(nbytes // 2, src, dst), "copy_all_bytes_us": copy_us(nbytes, src, dst)}
                got = gpu.tf_window_ld(CENTRE, refs, w, h, ctl, OUT, want=planes + ("var32",))
                flt = gpu.tf_filter_ld(CENTRE, refs, W, H, ctl)
                e["window_equals_filter"] = bool(all(np.array_equal(got[k], flt[k][:got[k].shape[0], :got[k].shape[1]])
                                                     for k in planes) and np.array_equal(got["var32"], flt["var32"]))
                src_y = y[CENTRE] if bd == 10 else (y[CENTRE] >> 2).astype(np.uint8)
                e["luma_samples_changed"] = int((got["y"] != src_y).sum())
                shapes[key(w, h, n, bd, chroma)] = e
        del src, dst
        for t in list(y) + [OUT, OUT + 1]:
            try:
                gpu.release(t)
            except RuntimeError:
                pass
    gpu.close()
    if trace:
        return
    res = {"what": "svtme_tf_window_ld and svtme_tf_filter_ld per window, beside the matching svtme_tf_window* call on "
                   "the same resident pictures and device-to-device copies, in one process; host clock, each ending "
                   "in a synchronise", "decays": DECAYS, "sub_sampling_shift": 1, "calls_per_run": calls, "shapes": shapes}
    if "--no-write" not in sys.argv:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "tf_ld.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
