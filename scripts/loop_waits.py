#!/usr/bin/env python3
"""The memory / wait sequence of a step kernel's loop, from the compiler's
assembly, and how many LDS round trips the loop exposes.

Input: the device assembly of csrc/voxnav_env.hip with line tables,

  hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 -I include \
        -S -gline-tables-only --cuda-device-only csrc/voxnav_env.hip -o env.s
  python scripts/loop_waits.py env.s "env_kernel<8,false,true,false,2>" [more kernels]

A kernel is named as in the source (a trailing DFL argument defaults to
false) or by any substring of its mangled symbol.  The step loop is the
largest backward-branch extent of the function (label .. branch back to it).
Printed: every LDS (ds_*), vector-memory (global_* / buffer_* / flat_* /
scratch_*) and s_waitcnt instruction of that extent in order, each with the
source line chain of its .loc (innermost first), then the counts.

An LDS read is *exposed* when the next LDS instruction or lgkmcnt wait after
it is a full `lgkmcnt(0)`: the wave then sits out that read's whole round
trip.  A batch of reads issued back to back ahead of one wait counts once
(the last read of the batch); a read followed by further LDS instructions or
by a counted wait (lgkmcnt(n > 0)) does not count.  --summary prints only
the counts, grouped by the outermost inlined source line.
"""
import argparse
import re
import sys
from collections import Counter

LDS = re.compile(r"^ds_")
VMEM = re.compile(r"^(global_|buffer_|flat_|scratch_)")
BRANCH = re.compile(r"^s_c?branch\w*\s+(\.LBB\w+)")
LABEL = re.compile(r"^(\.LBB\w+):")
LOC = re.compile(r"^\.loc\s+\d+\s+(\d+)")
CHAIN = re.compile(r"([\w./-]+):(\d+):\d+")


def mangled(spec: str) -> str:
    """env_kernel<8,false,true,false,2[,true]> -> the Itanium template-argument string."""
    m = re.fullmatch(r"\s*(\w+)\s*<(.*)>\s*", spec)
    if not m:
        return spec
    args = [a.strip() for a in m.group(2).split(",")]
    if m.group(1) == "env_kernel" and len(args) == 5:
        args.append("false")
    enc = "".join(f"Lb{int(a == 'true')}E" if a in ("true", "false") else f"Li{int(a)}E" for a in args)
    return f"{len(m.group(1))}{m.group(1)}I{enc}E"


def function_lines(lines, key):
    start = [i for i, l in enumerate(lines) if l.startswith("_Z") and key in l.split(":")[0] and l.rstrip().find(":") > 0
             and not l.startswith("\t")]
    if not start:
        raise SystemExit(f"no function matches {key!r}")
    if len(start) > 1:
        raise SystemExit(f"{key!r} matches {len(start)} functions: name it exactly")
    s = start[0]
    e = next(i for i in range(s, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return s, e


def loop_extent(lines, s, e):
    label_at = {}
    best = None
    for i in range(s, e):
        t = lines[i].strip()
        m = LABEL.match(t)
        if m:
            label_at[m.group(1)] = i
            continue
        m = BRANCH.match(t)
        if m and m.group(1) in label_at:                   # backward: the label is already seen
            ext = (label_at[m.group(1)], i)
            if best is None or ext[1] - ext[0] > best[1] - best[0]:
                best = ext
    if best is None:
        raise SystemExit("no backward branch: no loop")
    return best


def sequence(lines, lo, hi):
    """(kind, text, chain) of the extent's LDS / VMEM / wait instructions; kind in 'L', 'V', 'W'."""
    seq, chain = [], "?"
    for i in range(lo, hi + 1):
        t = lines[i].strip()
        if LOC.match(t):
            c = t.split(";", 1)[1] if ";" in t else ""
            parts = [f"{f.rsplit('/', 1)[-1]}:{ln}" for f, ln in CHAIN.findall(c)]
            chain = " < ".join(parts) if parts else "line " + LOC.match(t).group(1)
            continue
        op = t.split(";")[0].strip()
        if not op or op.startswith("."):
            continue
        if LDS.match(op):
            seq.append(("L", op, chain))
        elif VMEM.match(op):
            seq.append(("V", op, chain))
        elif op.startswith("s_waitcnt"):
            seq.append(("W", op, chain))
    return seq


def static_counts(lines, lo, hi):
    """--counts: the extent's static instruction mix, and its SGPR-spill lane moves
    (v_readlane / v_writelane) by outermost source line"""
    ops, where, chain = Counter(), Counter(), "?"
    for i in range(lo, hi + 1):
        t = lines[i].strip()
        if LOC.match(t):
            c = t.split(";", 1)[1] if ";" in t else ""
            parts = [f"{f.rsplit('/', 1)[-1]}:{ln}" for f, ln in CHAIN.findall(c)]
            chain = parts[-1] if parts else "line " + LOC.match(t).group(1)
            continue
        op = t.split(";")[0].strip()
        if not op or op.startswith(".") or op.endswith(":"):
            continue
        mn = op.split()[0]
        ops[mn] += 1
        if mn in ("v_readlane_b32", "v_writelane_b32"):
            where[chain + " " + mn[2:-4]] += 1
    total = sum(ops.values())
    br = sum(n for m, n in ops.items() if re.match(r"s_c?branch", m))
    print(f"   static instructions {total}: v_readlane_b32 {ops['v_readlane_b32']}, v_writelane_b32 "
          f"{ops['v_writelane_b32']}, s_nop {ops['s_nop']}, branches {br}, s_and_saveexec_b64 "
          f"{ops['s_and_saveexec_b64']}, s_setprio {ops['s_setprio']}, s_waitcnt {ops['s_waitcnt']}, VALU (v_*) "
          f"{sum(n for m, n in ops.items() if m.startswith('v_'))}, SALU (s_*) "
          f"{sum(n for m, n in ops.items() if m.startswith('s_'))}")
    for w, c in sorted(where.items(), key=lambda kv: -kv[1]):
        print(f"     {c:3d}  {w}")


def lgkm(op):
    """the lgkmcnt of a wait, or None when it does not wait on lgkmcnt"""
    m = re.search(r"lgkmcnt\((\d+)\)", op)
    return int(m.group(1)) if m else None


def exposed(seq):
    """indices of the exposed LDS reads"""
    out = []
    for i, (k, op, _) in enumerate(seq):
        if k != "L" or not op.startswith("ds_read"):
            continue
        for k2, op2, _ in seq[i + 1:]:
            if k2 == "L":
                break
            if k2 == "W" and lgkm(op2) is not None:
                if lgkm(op2) == 0:
                    out.append(i)
                break
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("kernels", nargs="+")
    ap.add_argument("--summary", action="store_true", help="counts only")
    ap.add_argument("--counts", action="store_true", help="also the loop's static instruction mix and spill lane moves")
    a = ap.parse_args()
    lines = open(a.asm).read().splitlines()
    for spec in a.kernels:
        s, e = function_lines(lines, mangled(spec))
        lo, hi = loop_extent(lines, s, e)
        seq = sequence(lines, lo, hi)
        exp = set(exposed(seq))
        print(f"== {spec}  ({lines[s].split(':')[0]})")
        print(f"   step loop: {lines[lo].strip()} .. {lines[hi].strip().split()[0]} back, {hi - lo} asm lines")
        if not a.summary:
            # a run of one mnemonic from one source line is one line with its count
            # (the last instruction's text; an exposed read ends its run)
            i = 0
            while i < len(seq):
                k, op, chain = seq[i]
                j = i
                while (j + 1 < len(seq) and j not in exp and seq[j + 1][0] == k and seq[j + 1][2] == chain
                       and seq[j + 1][1].split()[0] == op.split()[0] and k != "W"):
                    j += 1
                mark = "*" if j in exp else " "
                n = f"x{j - i + 1}" if j > i else ""
                print(f" {mark}{k} {n:<3} {seq[j][1]} ; {chain}")
                i = j + 1
        n = Counter(k for k, _, _ in seq)
        reads = sum(1 for k, op, _ in seq if k == "L" and op.startswith("ds_read"))
        full = sum(1 for k, op, _ in seq if k == "W" and lgkm(op) == 0)
        counted = sum(1 for k, op, _ in seq if k == "W" and (lgkm(op) or 0) > 0)
        print(f"   LDS instructions {n['L']} (reads {reads}), vector-memory {n['V']}, s_waitcnt {n['W']} "
              f"(lgkmcnt(0) {full}, counted lgkmcnt {counted})")
        print(f"   exposed LDS round trips: {len(exp)}")
        if a.counts:
            static_counts(lines, lo, hi)
        by = Counter(seq[i][2].split(" < ")[-1] + "  (" + seq[i][2].split(" < ")[0] + ")" for i in exp)
        for where, c in sorted(by.items(), key=lambda kv: (int(kv[0].split(":")[1].split()[0]), kv[0])):
            print(f"     {c:3d}  {where}")
        print()
    return 0


if __name__ == "__main__":
    sys.exit(main())
