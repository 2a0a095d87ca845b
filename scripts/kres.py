#!/usr/bin/env python3
"""VGPRs / spills / LDS of the rollout-buffer env kernels (PH 8 and 16) for
one or more sets of extra hipcc flags:
    python scripts/kres.py "" "-DVN_PC_MIN_WAVES=3"
With --unit: SGPRs, VGPRs, spills, scratch, occupancy and LDS of every kernel
of another unit (--csrc: of another checkout's csrc/):
    python scripts/kres.py --unit voxnav_simple.hip ""
"""
import argparse
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "3d-navigation-reinforcement-learning_amd"))
from voxnav import _build as b  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--unit", default="voxnav_env.hip")
ap.add_argument("--csrc", type=Path, default=b.CSRC)
ap.add_argument("flags", nargs="*")
args = ap.parse_args()
env = args.unit == "voxnav_env.hip"
fields = ("VGPRs:", "VGPRs Spill", "LDS Size") if env else \
    ("SGPRs:", "VGPRs:", "SGPRs Spill", "VGPRs Spill", "ScratchSize", "Occupancy", "LDS Size")

flags = [f for f in b.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
for extra in [a.split() for a in args.flags] or [[]]:
    cmd = [b.hipcc(), *flags, *extra, "-I", str(b.INCLUDE), "-c", str(args.csrc / args.unit), "-o", "/tmp/kres.o",
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    cur, res = None, {}
    for line in r.stderr.splitlines():
        if " error" in line:
            print(line)
        if "Function Name" in line:
            name = line.split("Function Name: ")[1].split(" ")[0]
            keep = not env or ("env_kernel" in name and ("ILi8ELb0ELb1ELb0E" in name or "ILi16ELb0ELb1ELb0E" in name))
            cur = name if keep else None
        elif cur and any(f in line for f in fields):
            text = line.split("remark: ")[-1]
            res.setdefault(cur, []).append((text.split(" [")[0] if env else text.rsplit(" [-R", 1)[0]).strip())
    for k, v in res.items():
        print(extra, k.split("env_kernel")[1][:26] if env else k, v)
