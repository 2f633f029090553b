"""Generate tests/golden/me_sweep.json from the reference itself.

Every case of tests/me_sweep.py (the draws of SWEEP_SEEDS, then DIRECTED) runs through
oracle/_ref/libsvtref.so, the reference's own open-loop ME compiled from its sources, with
the C kernels and with the AVX2 kernels; the two must agree. The controls come from the
reference's svt_aom_sig_deriv_me / svt_aom_sig_deriv_me_tf, then the case's mutations.
Stored per case: the case dict, records_checksum(records, sb_results) and the coverage counts
(me_sweep.coverage, from the reference's outputs and the case alone); and the total coverage.
No arrays.

Run from the repo root in the build container: python tests/golden/make_golden_me_sweep.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "svt-av1-mirror_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import svtme as S  # noqa: E402
import me_sweep as M  # noqa: E402


def golden_entry(case) -> dict:
    """One case through the reference (C and AVX2 kernels) -> its fixture entry."""
    ref = S.load_ref()
    frames = M.frames_of(S, case)
    ctrl = M.controls_of(S, case, reference=True)
    out = {}
    for simd in (0, 1):
        ref.svtref_set_simd(simd)
        out[simd] = M.run_cpu(S, case, "ref", frames=frames, ctrl=ctrl)
    recs, sbr = out[0]
    errs = S.compare_records(recs, out[1][0], sbr, out[1][1])
    assert not errs, (case["name"], errs[:3])
    return {"case": case, "checksum": S.records_checksum(recs, sbr), "coverage": M.coverage(S, case, ctrl, recs, sbr)}


def dumps(entries, total) -> str:
    lines = ",\n".join("  " + json.dumps(e, separators=(",", ":")) for e in entries)
    return '{"cases": [\n' + lines + '\n],\n"total": ' + json.dumps(total, separators=(",", ":")) + "}\n"


def main():
    entries = []
    total = dict.fromkeys(M.COVERAGE_KEYS, 0)
    for case in M.cases():
        e = golden_entry(case)
        for k, v in e["coverage"].items():
            total[k] += v
        entries.append(e)
        print(case["name"], e["checksum"][:16], {k: v for k, v in e["coverage"].items() if v}, flush=True)
    with open(os.path.join(HERE, "me_sweep.json"), "w") as fh:
        fh.write(dumps(entries, total))
    print("total", total)
    missing = [k for k, v in total.items() if not v]
    if missing:
        raise SystemExit(f"coverage keys at zero: {missing}")


if __name__ == "__main__":
    main()
