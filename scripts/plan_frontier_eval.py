#!/usr/bin/env python3
"""The results table of train/evaluate_grid.py for the two policies that need no training: the
frontier planner (voxnav.planner.evaluate_planner) and the uniform random policy
(vn_step_random), on the P1 / P2 / P3 evaluate room sets -- the yardstick rows a trained checkpoint
is compared with.  --episodes agents per set, agent i reset with seed + i, one
episode each (no auto-reset), L 10.  Prints the table and one JSON line.  Needs a GPU."""
import argparse
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "3d-navigation-reinforcement-learning_amd"))
import torch  # noqa: E402

from voxnav.env import BatchedGridEnv  # noqa: E402
from voxnav.evaluate import RESULTS_HEADER, results_table_row  # noqa: E402
from voxnav.planner import evaluate_planner  # noqa: E402
from voxnav.rooms import load_archive_set  # noqa: E402


def evaluate_random(rooms, n_episodes, L, seed, device, policy_seed=42, chunk=64):
    """evaluate_policy's dictionary for the Philox uniform random policy."""
    env = BatchedGridEnv(num_agents=n_episodes, rooms=rooms, local_map_length=L, autoreset=False, device=device)
    try:
        env.reset(seed=seed)
        dev = env.device
        alive = torch.ones(n_episodes, dtype=torch.bool, device=dev)
        score = torch.zeros(n_episodes, dtype=torch.float64, device=dev)
        steps = torch.zeros(n_episodes, dtype=torch.int64, device=dev)
        limit = int(env.total_free_cells.max()) + 1
        for _ in range(0, limit, chunk):
            ro = env.step_random(chunk, policy_seed=policy_seed, reward_f64=True)
            ended = (ro.terminated | ro.truncated).bool()
            for k in range(chunk):
                score += torch.where(alive, ro.reward[k], torch.zeros_like(score))
                steps += alive.to(torch.int64)
                alive &= ~ended[k]
            if not bool(alive.any()):
                break
        final = env.episode_records()[:, [7, 8, 11]].cpu().tolist()
        sc, sp = score.cpu().tolist(), steps.cpu().tolist()
        eps = [dict(score=sc[i], bumps=final[i][0], discovered_cells=final[i][1], finished=bool(final[i][2] & 1),
                    steps=sp[i]) for i in range(n_episodes)]
        n = max(1, n_episodes)
        return dict(episodes=eps, avg_score=sum(e["score"] for e in eps) / n, avg_bumps=sum(e["bumps"] for e in eps) / n,
                    finished_pct=100.0 * sum(e["finished"] for e in eps) / n,
                    avg_discovered=sum(e["discovered_cells"] for e in eps) / n, avg_steps=sum(e["steps"] for e in eps) / n)
    finally:
        env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="+", default=["P1_evaluate", "P2_evaluate", "P3_evaluate"])
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--L", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("plan_frontier_eval.py needs a GPU")
    out = {}
    print(RESULTS_HEADER)
    for name in args.sets:
        rooms = load_archive_set(name)
        kw = dict(n_episodes=args.episodes, seed=args.seed, device="cuda:0")
        for label, r in (("frontier planner", evaluate_planner(rooms, local_map_length=args.L, **kw)),
                         ("uniform random", evaluate_random(rooms, L=args.L, **kw))):
            print(results_table_row(f"{name}: {label}", r))
            out[f"{name}/{label}"] = {k: v for k, v in r.items() if k != "episodes"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
