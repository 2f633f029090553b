"""Static instruction counts of one k_hme instance per barrier-delimited segment (no GPU).

Compiles csrc/svtme_stages.hip to gfx950 assembly (about 30 s), takes the text of the named
instance and splits it at every s_barrier, in text order. Per segment it prints the number of
VALU, v_qsad*, SALU, LDS, VMEM and SMEM instructions and the ten most frequent VALU opcodes.
Instructions are classified by opcode prefix only:

  qsad  v_qsad* / v_mqsad*            VALU  every other v_*
  LDS   ds_*                          VMEM  buffer_* / global_* / flat_* / scratch_*
  SMEM  s_load* / s_buffer_load*      SALU  every other s_*

The counts are static: a loop body counts once and both sides of a branch count. The segments
of the whole-pass instances (FP = true, no HME-L2 at run time) are, in text order:
  0 job copy, 1 phase 0, 2-3 the two A1 rounds, 4 D + L1 table, 5 L1 tiles, 6-7 HME-L2 (table,
  tiles; not run at p8), 8 L1 resolve + BState + final centre, 9 full-pel, 10-13 phase E.

usage: python scripts/isa_phase_count.py ['k_hme<true,true,true,false,3>'] [--asm FILE] [--json OUT]
"""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "svt-av1-mirror_amd", "csrc", "svtme_stages.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
DEFAULT = "k_hme<true,true,true,false,3>"
COLS = ("valu", "qsad", "salu", "lds", "vmem", "smem")


def compile_asm(src=SRC, extra=()):
    """gfx950 assembly of src (device code only), as text"""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                            "-o", out, os.path.abspath(src), *extra], capture_output=True, text=True, cwd=td)
        if r.returncode:
            raise SystemExit(r.stderr[-3000:])
        with open(out) as f:
            return f.read()


def mangled(inst):
    """'k_hme<true,true,true,false,3>' -> the symbol of that instance in namespace svtme"""
    m = re.fullmatch(r"\s*(\w+)\s*<(.*)>\s*", inst)
    if not m:
        raise SystemExit(f"not a template instance: {inst!r}")
    args = ""
    for a in (x.strip() for x in m.group(2).split(",")):
        if a in ("true", "false"):
            args += "Lb1E" if a == "true" else "Lb0E"
        elif re.fullmatch(r"-?\d+", a):
            args += "Li" + ("n" + a[1:] if a[0] == "-" else a) + "E"
        else:
            raise SystemExit(f"template argument {a!r}: bool or int")
    name = m.group(1)
    return f"_ZN5svtme{len(name)}{name}I{args}EEv8DevBatch"


def classify(op):
    if op.startswith("v_"):
        return "qsad" if op.startswith(("v_qsad", "v_mqsad")) else "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op.startswith("s_"):
        return "salu"
    return None


def count(asm, inst=DEFAULT):
    """{'instance', 'symbol', 'vgprs', 'scratch', 'segments': [...], 'total': {...}} or None when
    the assembly has no such instance"""
    sym = mangled(inst)
    lines = asm.splitlines()
    try:
        start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
    except StopIteration:
        return None
    segs = [{c: 0 for c in COLS}]
    tops = [collections.Counter()]
    first = [start + 1]
    info = {}
    for i in range(start + 1, len(lines)):
        l = lines[i]
        if l.startswith(".Lfunc_end"):
            # the resource comments follow the function's end
            for k in lines[i:i + 40]:
                m = re.match(r"; (NumVgprs|ScratchSize|TotalNumSgprs|Occupancy|LDSByteSize): (\d+)", k)
                if m:
                    info[m.group(1)] = int(m.group(2))
            break
        m = re.match(r"\s+([a-z][a-z0-9_]+)", l)
        if not m or not l[0].isspace():
            continue
        op = m.group(1)
        if op == "s_barrier":
            segs.append({c: 0 for c in COLS})
            tops.append(collections.Counter())
            first.append(i + 1)
            continue
        cls = classify(op)
        if cls is None:
            continue
        segs[-1][cls] += 1
        if cls == "valu":
            # the opcode without its encoding suffix (_e32, _e64, _dpp, _sdwa)
            tops[-1][re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)] += 1
    out = []
    for n, (s, t, f) in enumerate(zip(segs, tops, first)):
        out.append({"segment": n, "line": f - start, **s, "top_valu": t.most_common(10)})
    total = {c: sum(s[c] for s in segs) for c in COLS}
    return {"instance": inst, "symbol": sym, "vgprs": info.get("NumVgprs"), "scratch": info.get("ScratchSize"),
            "sgprs": info.get("TotalNumSgprs"), "occupancy": info.get("Occupancy"), "lds_bytes": info.get("LDSByteSize"),
            "segments": out, "total": total}


def render(r):
    o = [f"{r['instance']}  ({r['symbol']})",
         f"VGPRs {r['vgprs']}  SGPRs {r['sgprs']}  scratch {r['scratch']}  LDS {r['lds_bytes']}  occupancy {r['occupancy']}",
         f"{'seg':>3} {'line':>6} " + " ".join(f"{c.upper():>6}" for c in COLS) + "  top VALU opcodes"]
    for s in r["segments"]:
        top = " ".join(f"{k}:{v}" for k, v in s["top_valu"])
        o.append(f"{s['segment']:>3} {s['line']:>6} " + " ".join(f"{s[c]:>6}" for c in COLS) + "  " + top)
    o.append(f"{'all':>3} {'':>6} " + " ".join(f"{r['total'][c]:>6}" for c in COLS))
    return "\n".join(o)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("instance", nargs="?", default=DEFAULT)
    ap.add_argument("--asm", help="count this assembly file instead of compiling")
    ap.add_argument("--json", help="also write the counts to this file")
    a = ap.parse_args()
    if a.asm:
        with open(a.asm) as f:
            asm = f.read()
    else:
        asm = compile_asm()
    r = count(asm, a.instance)
    if r is None:
        raise SystemExit(f"no instance {a.instance} ({mangled(a.instance)}) in the assembly")
    print(render(r))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
