"""Time svtme_tf_subpel for one temporal-filtering window.

1920x1080, the centre picture and 6 references, the control set of the TF level
preset 8 uses (tests/golden/make_golden_tfsp.py CONTROL_SETS["l8"]). The content
is the fractional-motion texture of tests/tfsp_content.py, made as a 256x256
tile and repeated (the texture is built at 8x resolution). The records are the
GPU's own TF-ME jobs of the window (hme_me_level 2, tf_me_exit_th 256), taken
once before the timed calls.

Reports ms per call by the host clock around synchronous calls (the record
upload, the launch, the kernel, the copy-out and the synchronisation). The
kernel's own time needs a kernel trace in a run of its own:
rocprofv3 --kernel-trace --stats -- python3 scripts/tf_subpel_bench.py 30 --no-cpu
Where oracle/_ref holds the reference library (tests/golden/make_golden_tfsp.py
links it), the same window goes through the generator's reference-side path on
one core: the reference's C convolves and variance kernels under the Python
restatement of the control flow, so that time includes the restatement's own
interpreter overhead and no AVX2 kernel (the reference's AVX2 convolves are not
part of that build). The per-SB results of both sides are compared.

Run on the GPU box: python3 scripts/tf_subpel_bench.py [calls] [--no-cpu]
Writes profiles/tf_subpel/tf_subpel_1080p.json (not with --no-cpu) and prints it.
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
CPU_BUDGET_S = 120.0  # references timed on the CPU until this is used up; the rest is extrapolated
# 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz: one 32-bit multiply-add per lane and clock (not measured)
VALU_MAD_PEAK_T = 256 * 128 * 2.4e9 / 1e12


def window_frames():
    tiles = tfsp_content.fractional_frames(TILE, TILE, (CENTRE,) + REFS)
    reps = ((H + TILE - 1) // TILE, (W + TILE - 1) // TILE)
    return {t: np.ascontiguousarray(np.tile(f, reps)[:H, :W]) for t, f in tiles.items()}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    calls = int(args[0]) if args else 100
    with_cpu = "--no-cpu" not in sys.argv
    import torch

    torch.cuda.set_device(0)
    gpu = S.GpuME(0)
    frames = window_frames()
    for t, f in frames.items():
        gpu.upload(t, f)
    cs = G.CONTROL_SETS[SET]
    ctl = G.subpel_controls(SET)
    me = S.derive_controls_tf(cs["hme_me_level"], 0, 35, S.input_resolution_of(W, H))
    recs = []
    for r in REFS:
        job = S.case_job(me, W, H, CENTRE, (r,), (), 0, me_type=S.ME_MCTF, tf_me_exit_th=cs["me_exit_th"])
        recs.append(gpu.submit(job, with_sb_results=False)[0][:, 0])
    recs = np.ascontiguousarray(np.stack(recs))

    def timed(n):
        t0 = time.perf_counter()
        for _ in range(n):
            out = gpu.tf_subpel(CENTRE, REFS, W, H, ctl, recs)
        return (time.perf_counter() - t0) * 1e3 / n, out

    timed(5)  # warm-up
    runs = []
    for _ in range(3):
        ms, out = timed(calls)
        runs.append(ms)
    sbs = out.shape[1]
    branches = {name: int((out["branch"] == v).sum()) for name, v in
                (("64_only", S.TFSP_64_ONLY), ("64_chosen", S.TFSP_64_CHOSEN), ("32", S.TFSP_32))}
    res = {
        "what": "svtme_tf_subpel, one 1080p window (centre + 6 references) in one call, TF level 8 controls",
        "width": W, "height": H, "references": len(REFS), "sbs_per_reference": sbs, "controls": ctl.as_dict(),
        "calls_per_run": calls, "ms_per_call_runs": [round(v, 4) for v in runs],
        "ms_per_call": round(sorted(runs)[1], 4), "branches": branches,
        "tf_early_exit_sbs": int(recs["tf_early_exit"].sum()),
    }
    gpu.close()
    if with_cpu and os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libtfsp_ref.so")):
        pyr = {t: S.build_host_pyramid(f, "ref") for t, f in frames.items()}
        wb = (S.align8(W) + 63) // 64
        cover = {k: 0 for k in G.COVERAGE_KEYS}
        spent, timed_refs, positions, macs, same = 0.0, 0, 0, 0, True
        for k, r in enumerate(REFS):
            if spent > CPU_BUDGET_S:
                break
            side = G.Side(pyr[CENTRE], pyr[r], cs, cover)
            t0 = time.perf_counter()
            cpu = [G.refine_sb(side, recs[k, i], 64 * (i % wb), 64 * (i // wb)) for i in range(sbs)]
            spent += time.perf_counter() - t0
            timed_refs += 1
            positions += side.positions
            macs += side.macs
            same = same and np.stack(cpu).tobytes() == out[k].tobytes()
        per_ref = spent * 1e3 / timed_refs
        res["cpu_ref_one_core"] = {
            "what": "the reference's C svt_inter_predictor and variance kernels under the generator's Python "
                    "restatement of the control flow; no AVX2 convolve in that build",
            "references_timed": timed_refs, "ms_per_reference": round(per_ref, 1),
            "ms_per_window": round(per_ref * len(REFS), 1), "extrapolated": timed_refs < len(REFS),
            "positions_per_reference": positions // timed_refs, "matches_gpu": bool(same),
        }
        window_macs = macs / timed_refs * len(REFS)
        res["multiply_adds_per_window_reference_positions"] = int(window_macs)
        res["valu_mad_peak_T"] = round(VALU_MAD_PEAK_T, 1)
        res["least_kernel_us_at_valu_peak"] = round(window_macs / (VALU_MAD_PEAK_T * 1e12) * 1e6, 2)
    if with_cpu:
        os.makedirs(os.path.join(ROOT, "profiles", "tf_subpel"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "tf_subpel", "tf_subpel_1080p.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
