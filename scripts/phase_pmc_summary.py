"""Per-phase counters from scripts/gpu_phase_pmc.sh output: the average per k_hme launch of each
stop-after build, the differences between consecutive builds, and the same per SB.
usage: python3 scripts/phase_pmc_summary.py [dir] [SBs per launch] [out.json]"""
import csv
import glob
import json
import os
import sys

O = sys.argv[1] if len(sys.argv) > 1 else "gpurun_out/phase_pmc"
NSB = int(sys.argv[2]) if len(sys.argv) > 2 else 0
OUT = sys.argv[3] if len(sys.argv) > 3 else None
KS = ["1", "2", "3", "4", "5", "55", "6", "full"]
NAMES = ["start..A0", "A1 table", "A1 tiles", "D + L1 table", "L1 tiles", "final centre", "full-pel", "decode+tail"]
rows = []
for k in KS:
    f = glob.glob(os.path.join(O, f"stop{k}", "**", "*counter_collection.csv"), recursive=True)
    if not f:
        print("missing", k)
        sys.exit(1)
    acc, disp = {}, set()
    for r in csv.DictReader(open(f[0])):
        acc[r["Counter_Name"]] = acc.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
        disp.add(r["Dispatch_Id"])
    n = max(1, len(disp))
    rows.append({c: v / n for c, v in acc.items()})
cs = sorted(rows[0])
print(f"{'phase':16s}" + "".join(f"{c:>24s}" for c in cs))
prev = {c: 0.0 for c in cs}
phases = []
for name, r in zip(NAMES, rows):
    d = {c: r[c] - prev[c] for c in cs}
    phases.append({"phase": name, "per_launch": d, "per_sb": {c: d[c] / NSB for c in cs} if NSB else None})
    print(f"{name:16s}" + "".join(f"{d[c]:24.0f}" for c in cs))
    prev = r
print(f"{'total':16s}" + "".join(f"{rows[-1][c]:24.0f}" for c in cs))
if NSB:
    print(f"\nper SB ({NSB} SBs per launch)")
    for p in phases:
        print(f"{p['phase']:16s}" + "".join(f"{p['per_sb'][c]:24.1f}" for c in cs))
    print(f"{'total':16s}" + "".join(f"{rows[-1][c] / NSB:24.1f}" for c in cs))
if OUT:
    with open(OUT, "w") as fh:
        json.dump({"sbs_per_launch": NSB, "phases": phases, "total_per_launch": rows[-1],
                   "total_per_sb": {c: rows[-1][c] / NSB for c in cs} if NSB else None}, fh, indent=1)
        fh.write("\n")
