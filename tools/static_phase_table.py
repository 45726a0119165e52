#!/usr/bin/env python3
"""Static instruction classes of the solver loop of the stage-wise branch of k_solve_routed<4, true, 1024>, by phase (every
arm counted).  Compiles neo_mpc_riccati.hip for the device with the Makefile's flags and -gline-tables-only -S, follows each
instruction's inlining chain to its line in solve_search (csrc/k1_solve.h) under the kernel's stage-wise call site, and sorts
the lines into phases by the NEO_PHASE markers of the solver loop -- the phases tools/phase_timing_routed.py clocks.  No GPU.
usage: python tools/static_phase_table.py [--root DIR]      (DIR: another checkout to count, default this one)"""
import argparse
import collections
import os
import re
import subprocess
import tempfile

PHASES = ["adjoint", "cone", "direction", "restrict/early", "candidates", "accept"]
COLUMNS = ["all", "f64", "valu_other", "v_mov", "v_cndmask", "v_cmp", "ds", "s_waitcnt", "s_nop", "salu", "branch"]
KERNEL = "k_solve_routedILi4ELb1ELi1024E"


def classify(op):
    if op.startswith("ds_"):
        return "ds"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op == "s_nop":
        return "s_nop"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        if "f64" in op:
            return "f64"
        for k in ("v_mov", "v_cndmask", "v_cmp"):
            if op.startswith(k):
                return k
        return "valu_other"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    csrc = os.path.join(args.root, "neo_mpc_planner2_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^RICCATI_FLAGS := (.*)$", mk, re.M).group(1).split()
    src = open(os.path.join(csrc, "k1_solve.h")).read().split("\n")
    marks = {int(re.search(r"NEO_PHASE\((\d)\)", l).group(1)): i + 1 for i, l in enumerate(src) if re.match(r"\s*NEO_PHASE\(\d\);", l)}
    loop_top = next(i + 1 for i, l in enumerate(src) if "K1-SEARCH-LOOP-BEGIN" in l)   # (marker comments of k1_solve.h)
    loop_end = next(i + 1 for i, l in enumerate(src) if re.match(r"\s*NEO_PHASE_DUMP\(\);", l))
    site = next(i + 1 for i, l in enumerate(src) if "K1-ROUTED-STAGEWISE-SEARCH" in l)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-pass-failed"] + flags +
                       ["-gline-tables-only", "-x", "hip", "--cuda-device-only", "-S", os.path.join(csrc, "neo_mpc_riccati.hip"),
                        "-o", out], check=True, stderr=subprocess.DEVNULL)
        text = open(out).read().split("\n")
    start = next(i for i, l in enumerate(text) if l.startswith("_Z") and KERNEL in l and ":" in l)
    end = next(i for i in range(start, len(text)) if ".amdhsa_kernel" in text[i])
    table = collections.defaultdict(collections.Counter)
    line = None
    for l in text[start:end]:
        if re.match(r"\s*\.loc\s", l):
            chain = [int(x) for x in re.findall(r"k1_solve\.h:(\d+):\d+", l)]
            m = re.match(r"\s*\.loc\s+\d+\s+(\d+)\s", l)
            own = int(m.group(1))
            # (the frame under the kernel's call site is the line in solve_search; an instruction of solve_search itself has
            # only the call site behind it)
            if chain and chain[-1] == site:
                line = chain[-2] if len(chain) >= 2 else own
            else:
                line = None
            continue
        t = l.strip()
        if line is None or not t or t[0] in ".;_" or t.endswith(":"):
            continue
        kind = classify(t.split()[0])
        if kind is None or not (loop_top <= line <= loop_end):
            continue
        table["loop"][kind] += 1
        for k, name in enumerate(PHASES):
            if marks[k] <= line < marks[k + 1]:
                table[name][kind] += 1
    print("%-16s" % "phase" + "".join("%11s" % c for c in COLUMNS))
    for name in PHASES + ["loop"]:
        row = table[name]
        print("%-16s" % name + "%11d" % sum(row.values()) + "".join("%11d" % row[c] for c in COLUMNS[1:]))


if __name__ == "__main__":
    main()
