"""Time svtme_dg_detect for the three picture pairs of one dynamic-GOP decision.

1920x1080, search area 128x128 (the reference's rule above 480p), the three
pairs of one 32-picture mini-GOP (end/start, end/mid, mid/start,
pd_process.c:672-718) in ONE call on resident pictures, metrics only (the
encoder's binding reads nothing else). After warm-up the call is repeated
until the timed window is far above one launch + synchronisation.

Reports ms per call (host clock around synchronous calls: the launch, the
kernel, the 96-byte copy and the synchronisation), absdiff/s over the clamped
windows actually searched and that rate as a fraction of the VALU-SAD roof
bench.py uses (150.3 T absdiff/s): a call-level figure, not the kernel's share
of the roof, which needs the kernel's own time from a kernel trace
(rocprofv3 --kernel-trace --stats -- python3 scripts/dg_bench.py 50). Where
oracle/_ref/libsvtref.so is present, the reference's own sad_loop kernel is
timed on one core over the same windows of one pair (the CPU side of the
comparison; tests/golden/make_golden_dg.py holds the windows).

Run on the GPU box: python3 scripts/dg_bench.py [calls]
Writes profiles/dg/dg_1080p.json and prints it.
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "svt-av1-mirror_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import svtme as S  # noqa: E402
import make_golden_dg as G  # noqa: E402

SAD_PEAK_T = 150.3  # bench.py: v_sad_u8 roof measured on MI355X, T absdiff/s
W, H, SA = 1920, 1080, 128
PICS = (8, 24, 40)
PAIRS = ((40, 8), (40, 24), (24, 8))


def timed(gpu, arr, met, sa, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        st = gpu.lib.svtme_dg_detect(gpu.ctx, arr, len(PAIRS), sa, sa, met, None)
        if st:
            gpu._check(st, "svtme_dg_detect")
    return (time.perf_counter() - t0) * 1e3 / calls


def main():
    calls = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    import torch

    torch.cuda.set_device(0)
    gpu = S.GpuME(0)
    frames = S.test_frames("pan", W, H, PICS)
    for t, f in frames.items():
        gpu.upload(t, f)
    arr = (S.DgPair * len(PAIRS))(*[S.DgPair(c, r) for c, r in PAIRS])
    met = (S.DgMetrics * len(PAIRS))()
    timed(gpu, arr, met, SA, 20)  # warm-up
    runs = [timed(gpu, arr, met, SA, calls) for _ in range(3)]
    ms = sorted(runs)[1]
    wins = G.sb_windows(W, H, SA, SA)
    absdiffs = len(PAIRS) * sum(sw * sh for *_, sw, sh in wins) * 256
    out = {
        "what": "svtme_dg_detect, 3 pairs of one decision in one call, metrics only",
        "width": W, "height": H, "sa": [SA, SA], "pairs": len(PAIRS), "sbs_per_pair": len(wins),
        "calls_per_run": calls, "ms_per_call_runs": [round(v, 4) for v in runs], "ms_per_call": round(ms, 4),
        "absdiffs_per_call": absdiffs,
        "absdiff_per_s_T": round(absdiffs / (ms * 1e-3) / 1e12, 3),
        "call_frac_of_valu_sad_roof": round(absdiffs / (ms * 1e-3) / 1e12 / SAD_PEAK_T, 4),
        "metrics": [m.as_dict() for m in met],
    }
    if os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")):
        lib = G.load_ref_c()
        pyr = {t: S.build_host_pyramid(frames[t], "ref") for t in PAIRS[0]}
        out["cpu_ref_one_core"] = {}
        for simd, name in ((1, "avx2"), (0, "c")):  # svt_sad_loop_kernel_avx2_intrin / _c; ends on the default
            lib.svtref_set_simd(simd)
            t0 = time.perf_counter()
            sb = G.search_pair(pyr[PAIRS[0][0]], pyr[PAIRS[0][1]], SA, SA, lib)
            cpu_ms = (time.perf_counter() - t0) * 1e3
            out["cpu_ref_one_core"][name] = {
                "ms_per_pair": round(cpu_ms, 1), "ms_per_decision": round(3 * cpu_ms, 1),
                "absdiff_per_s_G": round(absdiffs / 3 / (cpu_ms * 1e-3) / 1e9, 2),
                "matches_gpu_metrics": G.metrics_of(W, H, sb) == [met[0].as_dict()[f] for f in G.METRIC_FIELDS]}
    gpu.close()
    os.makedirs(os.path.join(ROOT, "profiles", "dg"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "dg", "dg_1080p.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
