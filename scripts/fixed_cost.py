#!/usr/bin/env python3
"""Per-launch fixed cost of the CubicEnv rollout-buffer kernel in the
driver's window: after a reset and W warmup steps, one launch of F steps
(HIP events on the launch stream), for several F; fits t(F) = fixed + F * step.
  python scripts/fixed_cost.py [--lib path] [--warmup 5] [--tuning pcache_cap=1,dflush=3]"""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "3d-navigation-reinforcement-learning_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from voxnav import _native  # noqa: E402
from voxnav.env import BatchedGridEnv, Rollout  # noqa: E402
from voxnav.rooms import box_room, single_room_set  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--N", type=int, default=65536)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--F", default="1,2,5,10,20,40")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--tuning", default="", help="field=V,... VnTuning fields of the env")
a = ap.parse_args()
tuning = {k: int(v) for k, v in (kv.split("=", 1) for kv in filter(None, a.tuning.split(",")))} or None
lib = _native.load_variant(REPO / a.lib) if a.lib else _native.load()
env = BatchedGridEnv(num_agents=a.N, rooms=single_room_set(box_room(32, 32, 8)), local_map_length=10,
                     autoreset=True, device="cuda:0", lib=lib, tuning=tuning)
Fs = [int(f) for f in a.F.split(",")]
Fm = max(Fs)
dev = "cuda:0"
out = Rollout(torch.empty((Fm, a.N, 80), device=dev), torch.empty((Fm, a.N), device=dev),
              torch.empty((Fm, a.N), dtype=torch.uint8, device=dev),
              torch.empty((Fm, a.N), dtype=torch.uint8, device=dev), None)
res = {}
for F in Fs:
    ts = []
    sub = Rollout(out.obs[:F], out.reward[:F], out.terminated[:F], out.truncated[:F], None)
    wsub = Rollout(out.obs[:a.warmup], out.reward[:a.warmup], out.terminated[:a.warmup],
                   out.truncated[:a.warmup], None)
    for r in range(a.reps + 1):
        env.reset(seed=42 + r)
        if a.warmup:
            env.step_random(a.warmup, policy_seed=7, t0=0, out=wsub)
        fn = env.step_random_launcher(F, 7, a.warmup, sub)
        s = torch.cuda.current_stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(s)
        fn()
        e1.record(s)
        torch.cuda.synchronize()
        if r:
            ts.append(e0.elapsed_time(e1) * 1e3)
    res[F] = float(np.median(ts))
x = np.array(Fs, dtype=float)
y = np.array([res[F] for F in Fs])
step, fixed = np.polyfit(x, y, 1)
print(json.dumps({"us": {str(k): round(v, 2) for k, v in res.items()}, "fixed_us": round(fixed, 2),
                  "per_step_us": round(step, 3), "warmup": a.warmup}))
