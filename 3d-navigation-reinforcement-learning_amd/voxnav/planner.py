"""The frontier planner as a policy: the classical exploration baseline.

``BatchedGridEnv.plan_frontier`` (``vn_plan_frontier``, include/voxnav.h)
reads every agent's belief map on the device and returns the first action of
a shortest known-free path to the nearest cell the agent knows to be free and
has not visited.  This module wraps it in what the learned policies have:

* ``FrontierExplorer.act(env)``: the actions of one step;
* ``FrontierExplorer.act_dists(env)``: the same with the distance through each
  of the six first actions and the set of equally short ones
  (``vn_plan_frontier_dists``);
* ``FrontierExplorer.rollout(env, k_steps)``: plan + step for k steps into
  [K, N] tensors -- the obs acted on, the actions, rewards and flags: a
  demonstration set for a warm start;
* ``evaluate_planner(rooms, ...)``: ``evaluate_policy``'s metrics and
  dictionary (train/evaluate_grid.py:180-268) for the planner, the yardstick
  row a trained checkpoint is compared with in the results table.

There is no learned part and no host round trip per step: the plan is one
kernel launch, the step another.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional

import torch

from .env import BatchedGridEnv, FrontierDists


class PlannedRollout(NamedTuple):
    obs: torch.Tensor            # f32 [K, N, obs_dim]: the observation each action was planned for
    actions: torch.Tensor        # i32 [K, N]
    reward: torch.Tensor         # f32 [K, N]
    terminated: torch.Tensor     # bool [K, N]
    truncated: torch.Tensor      # bool [K, N]
    dist: torch.Tensor           # i32 [K, N]: steps to the planned target, -1 = fallback action
    last_obs: torch.Tensor       # f32 [N, obs_dim]: the observation after the last step


class FrontierExplorer:
    """Nearest-unvisited-cell exploration from the agents' own belief maps
    (CubicEnv variant, padded rooms of at most 64 x 64)."""

    def act(self, env: BatchedGridEnv, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
            return_dist: bool = False):
        """Actions int32 [N] for the env's current state (``plan_frontier``)."""
        return env.plan_frontier(mask=mask, out=out, return_dist=return_dist)

    def act_dists(self, env: BatchedGridEnv, mask: Optional[torch.Tensor] = None, out: Optional[FrontierDists] = None):
        """``(actions, dist, dists, best)`` for the env's current state
        (``plan_frontier_dists``): the action of ``act`` together with the
        distance through each of the six first actions and the set of the
        shortest."""
        return env.plan_frontier_dists(mask=mask, out=out)

    @torch.no_grad()
    def rollout(self, env: BatchedGridEnv, k_steps: int, obs: Optional[torch.Tensor] = None,
                seed=None) -> PlannedRollout:
        """``k_steps`` alternations of plan and ``env.step``.  ``obs`` is the
        observation of the env's current state (what ``reset`` or the last
        step returned, e.g. the previous rollout's ``last_obs``); without it
        the env is reset first (``env.reset(seed)``) and the rollout starts
        from that observation.  With autoreset an agent goes on into its next
        episode, as in a collector's rollout."""
        K, N, dev = int(k_steps), env.num_agents, env.device
        if K < 1:
            raise ValueError(f"k_steps must be >= 1 (got {k_steps})")
        if obs is None:
            obs = env.reset(seed)
        if tuple(obs.shape) != (N, env.obs_dim):
            raise ValueError(f"obs: expected {(N, env.obs_dim)}, got {tuple(obs.shape)}")
        o = torch.empty((K, N, env.obs_dim), dtype=torch.float32, device=dev)
        acts = torch.zeros((K, N), dtype=torch.int32, device=dev)
        dist = torch.empty((K, N), dtype=torch.int32, device=dev)
        rew = torch.empty((K, N), dtype=torch.float32, device=dev)
        te = torch.empty((K, N), dtype=torch.uint8, device=dev)
        tr = torch.empty((K, N), dtype=torch.uint8, device=dev)
        cur = obs.to(device=dev, dtype=torch.float32)
        for t in range(K):
            o[t].copy_(cur)
            _, d = env.plan_frontier(out=acts[t], return_dist=True)
            dist[t].copy_(d)
            cur = torch.empty((N, env.obs_dim), dtype=torch.float32, device=dev)
            env.step_into(acts[t], cur, rew[t], te[t], tr[t])
        return PlannedRollout(o, acts, rew, te.bool(), tr.bool(), dist, cur)


@torch.no_grad()
def evaluate_planner(rooms, n_episodes: int = 10, local_map_length: int = 10, seed: int = 0, device="cuda:0",
                     crash_penalty: float = -2.0, max_steps: Optional[int] = None,
                     record_actions: bool = False) -> Dict[str, object]:
    """``evaluate_policy`` with the frontier planner in the policy's place:
    ``n_episodes`` agents play one episode each side by side (agent i reset
    with ``seed + i``), and the same dictionary comes back -- ``{"episodes":
    [{score, bumps, discovered_cells, finished, steps}], "avg_score",
    "avg_bumps", "finished_pct", "avg_discovered", "avg_steps"}`` (plus
    ``"actions"`` [steps, n_episodes] when ``record_actions``), printable with
    ``results_table_row``.  The finals are the step kernel's episode records."""
    env = BatchedGridEnv(num_agents=n_episodes, rooms=rooms, local_map_length=local_map_length, autoreset=False,
                         device=device, crash_penalty=crash_penalty)
    try:
        dev = env.device
        env.reset(seed=seed)
        planner = FrontierExplorer()
        alive = torch.ones(n_episodes, dtype=torch.bool, device=dev)
        score = torch.zeros(n_episodes, dtype=torch.float64, device=dev)
        steps = torch.zeros(n_episodes, dtype=torch.int64, device=dev)
        limit = int(max_steps) if max_steps is not None else int(env.total_free_cells.max()) + 1
        acts: List[torch.Tensor] = []
        for t in range(limit):
            a = planner.act(env)
            if record_actions:
                acts.append(a)
            res = env.step(a, reward_f64=True, terminal_obs=False)
            score += torch.where(alive, res.reward, torch.zeros_like(res.reward))
            steps += alive.to(torch.int64)
            alive &= ~(res.terminated | res.truncated)
            if (t & 63) == 63 and not bool(alive.any()):
                break
        final = env.episode_records()[:, [7, 8, 11]]     # last_bumps, last_visited, last_flags
        final[:, 2] &= 1                                 # bit 0: terminated = done
        f = final.cpu().tolist()
        sc, sp = score.cpu().tolist(), steps.cpu().tolist()
        eps = [dict(score=sc[i], bumps=f[i][0], discovered_cells=f[i][1], finished=bool(f[i][2]), steps=sp[i])
               for i in range(n_episodes)]
        n = max(1, n_episodes)
        out = dict(episodes=eps,
                   avg_score=sum(e["score"] for e in eps) / n,
                   avg_bumps=sum(e["bumps"] for e in eps) / n,
                   finished_pct=100.0 * sum(e["finished"] for e in eps) / n,
                   avg_discovered=sum(e["discovered_cells"] for e in eps) / n,
                   avg_steps=sum(e["steps"] for e in eps) / n)
        if record_actions:
            out["actions"] = torch.stack(acts).cpu().numpy() if acts else None
        return out
    finally:
        env.close()
