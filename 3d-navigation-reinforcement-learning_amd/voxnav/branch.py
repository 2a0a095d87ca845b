"""Branching on top of per-agent copies: fan chosen agents out into a wider
env and evaluate action plans from them.

``fan_out`` is one ``vn_copy_agents`` launch, ``evaluate_plans`` that plus one
``vn_step_actions`` launch; neither synchronises the host.  The copies are
layout-native and carry the source's next auto-reset seed, so a branch
continues exactly as its root would under the same actions.  (The random
policy of ``step_random`` is keyed by the agent's slot: branches differ under
it.)  Not copied: episode records, and whatever a collector or learner keeps
per agent (LSTM rows, Monitor counters) -- callers index those themselves.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from .env import BatchedGridEnv


def wide_env(env: BatchedGridEnv, num_agents: int) -> BatchedGridEnv:
    """An env of ``num_agents`` agents that ``env``'s agents can be copied
    into: built from ``env``'s arguments with its ``seed_stride`` and
    launch-time tuning, and reset once so that every slot holds a valid agent."""
    ctor = dict(env._ctor, num_agents=int(num_agents), seed_stride=env.seed_stride)
    other = BatchedGridEnv(**ctor)
    if env._tuning is not None:
        other.set_tuning(**{f: getattr(env._tuning, f) for f in ("prio", "dflush", "wrec_k", "wrec_early")})
    other.reset(seed=0)
    return other


def fan_out(env: BatchedGridEnv, roots, width: int, into: Optional[BatchedGridEnv] = None) -> BatchedGridEnv:
    """An env of ``M * width`` agents whose agent ``m * width + b`` is a copy
    of ``env``'s agent ``roots[m]`` (int [M]).  ``into`` reuses a compatible
    env of that size (one returned by an earlier call); its rejection count
    of the copy is left in ``last_rejected`` (device int32 [1])."""
    r = torch.as_tensor(roots, device=env.device).to(torch.int32).reshape(-1)
    M, W = int(r.numel()), int(width)
    if M < 1 or W < 1:
        raise ValueError(f"fan_out needs at least one root and width >= 1 (got {M}, {W})")
    if into is None:
        into = wide_env(env, M * W)
    elif into.num_agents != M * W:
        raise ValueError(f"into has {into.num_agents} agents, {M} roots x width {W} need {M * W}")
    elif into is env:
        raise ValueError("into must be another env than the one the roots are in")
    into.last_rejected = into.copy_agents(env, r.repeat_interleave(W))
    into._t = env._t
    return into


def evaluate_plans(env: BatchedGridEnv, roots, plans, gamma: float = 1.0,
                   into: Optional[BatchedGridEnv] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The return of every action plan from every root: ``plans`` is int
    [B, K] (B plans of K actions), ``roots`` int [M].  Returns ``(returns
    f64 [M, B], ended_at i32 [M, B])``: the discounted sum
    ``sum_k gamma**k * r_k`` of the exact f64 rewards up to and including the
    first step that ended the root's running episode (``ended_at``: that
    step, -1 if the episode outlasts the plan); rewards after an in-launch
    auto-reset are not counted.  One fan-out and one ``step_actions`` launch;
    the sum runs on the device, left to right.  ``env`` is not stepped."""
    p = torch.as_tensor(plans, device=env.device).to(torch.int32)
    if p.dim() != 2 or p.shape[0] < 1 or p.shape[1] < 1:
        raise ValueError(f"plans: expected [B, K], got {tuple(p.shape)}")
    B, K = int(p.shape[0]), int(p.shape[1])
    M = int(torch.as_tensor(roots).numel())
    wide = fan_out(env, roots, B, into=into)
    ro = wide.step_actions(p.t().repeat(1, M), reward_f64=True)       # agent m * B + b takes plans[b]
    ended = (ro.terminated | ro.truncated).bool()                     # [K, M * B]
    before = torch.cumsum(ended.to(torch.int32), 0) - ended.to(torch.int32)   # episodes ended before step k
    ret = torch.zeros(M * B, dtype=torch.float64, device=env.device)
    disc = 1.0
    for k in range(K):
        ret = ret + torch.where(before[k] == 0, disc * ro.reward[k], torch.zeros_like(ret))
        disc = disc * float(gamma)
    first = torch.argmax(ended.to(torch.int32), 0).to(torch.int32)
    ended_at = torch.where(ended.any(0), first, torch.full_like(first, -1))
    return ret.view(M, B), ended_at.view(M, B)
