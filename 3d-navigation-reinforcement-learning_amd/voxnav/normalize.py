"""Return-based reward normalisation on the device (vn_return_moments /
vn_reward_normalize; the rule is stated in include/voxnav.h).

SB3's ``VecNormalize(norm_reward=True, norm_obs=False)``: each reward is
divided by the running standard deviation of the discounted return and
clipped to +-``clip_reward`` (``_update_reward`` / ``normalize_reward`` /
``RunningMeanStd.update_from_moments``; the reference's other trainer wraps
its env so, GARL/train/train_single.py:26).  Here it runs on the rollout
buffer's ``[T, N]`` rewards where the collector left them, with no host read:
``RolloutCollector(..., reward_norm=RewardNormalizer(...))`` normalises the
steps collected since the last flush right before each truncation bootstrap.

The batch moments are summed in a fixed order (64-agent chunks by global id,
then a binary tree over the chunks), so the statistics and the rewards do not
depend on how the agents are sharded over ranks; with a process group the
ranks' chunk triples are all-gathered between the two calls, one collective
per segment.  Observations are not normalised (the env emits scaled ones).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _native

CHUNK = 64      # agents per chunk (csrc/ret_rms.h RR_CHUNK)


class RewardNormalizer:
    """Owns the state: ``rms`` f64 [3] = (mean, var, count), initially
    (0, 1, 1e-4), and the discounted returns ``ret`` f64 [num_agents], on
    ``device``.

    ``agent_id_base`` / ``n_global``: this shard's first global agent id and
    the agents of all shards (default: this shard alone).  Every shard but
    the last must hold a multiple of 64 agents.  ``process_group``: the ranks
    whose shards make up ``n_global``, in rank order.

    ``training = False`` (SB3's ``VecNormalize.training``) scales by the
    stored variance and leaves ``ret`` and the statistics alone.
    """

    def __init__(self, num_agents: int, gamma: float, clip_reward: float = 10.0, epsilon: float = 1e-8,
                 agent_id_base: int = 0, n_global: Optional[int] = None, process_group=None, device="cuda:0"):
        self.num_agents = int(num_agents)
        self.gamma = float(gamma)
        self.clip_reward = float(clip_reward)
        self.epsilon = float(epsilon)
        self.agent_id_base = int(agent_id_base)
        self.n_global = self.num_agents if n_global is None else int(n_global)
        self.process_group = process_group
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"device must be a GPU, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.training = True
        if self.num_agents < 1:
            raise ValueError("num_agents must be >= 1")
        if not self.clip_reward > 0:
            raise ValueError("clip_reward must be positive")
        if self.agent_id_base < 0 or self.agent_id_base % CHUNK:
            raise ValueError(f"agent_id_base must be a non-negative multiple of {CHUNK} (got {self.agent_id_base}): "
                             "chunks of 64 agents are reduced by global id")
        end = self.agent_id_base + self.num_agents
        if end > self.n_global:
            raise ValueError(f"agents {self.agent_id_base} .. {end - 1} lie outside n_global = {self.n_global}")
        last = end == self.n_global
        if process_group is not None:
            import torch.distributed as dist
            self._world = dist.get_world_size(process_group)
            last = dist.get_rank(process_group) == self._world - 1
            sizes = [None] * self._world            # every rank's chunk count, once
            dist.all_gather_object(sizes, -(-self.num_agents // CHUNK), group=process_group)
            self._sizes = [int(v) for v in sizes]
            if sum(self._sizes) != -(-self.n_global // CHUNK):
                raise ValueError(f"the ranks hold {sum(self._sizes)} chunks of 64 agents, n_global = {self.n_global} "
                                 f"makes {-(-self.n_global // CHUNK)}")
        elif self.n_global != self.num_agents:
            raise ValueError("n_global beyond this shard needs the process_group that holds the other shards")
        if not last and self.num_agents % CHUNK:
            raise ValueError(f"every shard but the last must hold a multiple of {CHUNK} agents (got {self.num_agents})")
        self.lib = _native.load()
        self.c_local = -(-self.num_agents // CHUNK)
        self.c_global = -(-self.n_global // CHUNK)
        self.rms = torch.tensor([0.0, 1.0, 1e-4], dtype=torch.float64, device=self.device)
        self.ret = torch.zeros(self.num_agents, dtype=torch.float64, device=self.device)
        self._partials = None       # [steps, c_local, 3], grown on demand
        self._scales = None
        self.last_scales = None     # f64 [t1 - t0]: sqrt(var_t + epsilon) of the last segment (a view)

    # ------------------------------------------------------------------ state
    @property
    def mean(self) -> float:
        return float(self.rms[0])

    @property
    def var(self) -> float:
        return float(self.rms[1])

    @property
    def count(self) -> float:
        return float(self.rms[2])

    def state_dict(self) -> Dict[str, object]:
        return dict(rms=self.rms.cpu().clone(), ret=self.ret.cpu().clone(), num_agents=self.num_agents,
                    agent_id_base=self.agent_id_base, gamma=self.gamma, clip_reward=self.clip_reward,
                    epsilon=self.epsilon)

    def load_state_dict(self, sd: Dict[str, object]) -> None:
        rms = torch.as_tensor(sd["rms"], dtype=torch.float64).reshape(-1)
        ret = torch.as_tensor(sd["ret"], dtype=torch.float64).reshape(-1)
        if int(sd.get("num_agents", ret.numel())) != self.num_agents or ret.numel() != self.num_agents:
            raise ValueError(f"reward-normaliser state of {ret.numel()} agents, this one has {self.num_agents}")
        if rms.numel() != 3:
            raise ValueError("rms must hold (mean, var, count)")
        self.rms.copy_(rms)
        self.ret.copy_(ret)

    # ------------------------------------------------------------------ work
    def _buffers(self, steps: int):
        if self._partials is None or self._partials.shape[0] < steps:
            self._partials = torch.zeros((steps, self.c_local, 3), dtype=torch.float64, device=self.device)
            self._scales = torch.zeros(steps, dtype=torch.float64, device=self.device)
        return self._partials[:steps], self._scales[:steps]

    def _gather(self, part: torch.Tensor) -> torch.Tensor:
        """All ranks' chunk triples in rank order, [steps, c_global, 3]: one collective of
        equal-sized blocks (padded to the largest shard's chunk count; the pad is dropped)."""
        import torch.distributed as dist
        steps, c_max = part.shape[0], max(self._sizes)
        block = torch.zeros((steps, c_max, 3), dtype=torch.float64, device=self.device)
        block[:, :self.c_local] = part
        out = [torch.empty_like(block) for _ in range(self._world)]
        dist.all_gather(out, block, group=self.process_group)
        return torch.cat([o[:, :c] for o, c in zip(out, self._sizes)], dim=1).contiguous()

    @torch.no_grad()
    def normalize_segment(self, rewards: torch.Tensor, episode_starts: torch.Tensor, t0: int, t1: int,
                          stream=None) -> None:
        """Normalise ``rewards[t0:t1]`` in place.  ``rewards`` f32 [T, N];
        ``episode_starts`` f32 [T + 1, N], row t + 1 marking the agents whose
        episode ended at step t (the collector's layout); both contiguous, on
        the normaliser's device.  Stream-ordered: no host read."""
        T, N = rewards.shape
        if N != self.num_agents:
            raise ValueError(f"rewards of {N} agents, the normaliser has {self.num_agents}")
        if not 0 <= t0 < t1 <= T:
            raise ValueError(f"steps [{t0}, {t1}) outside the {T} rows of rewards")
        for name, x, rows in (("rewards", rewards, T), ("episode_starts", episode_starts, T + 1)):
            if x.dtype != torch.float32 or x.device != self.device or not x.is_contiguous() or \
                    tuple(x.shape) != (rows, N):
                raise ValueError(f"{name} must be a contiguous f32 [{rows}, {N}] tensor on {self.device}")
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        if stream is None:
            stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        steps = t1 - t0
        part, scales = self._buffers(steps)
        with torch.cuda.device(self.device):
            if not self.training:
                _native.check(self.lib.vn_reward_normalize(p(rewards), t0, t1, N, None, 0, p(self.rms), self.epsilon,
                                                           self.clip_reward, 0, p(scales), stream),
                              "vn_reward_normalize")
                self.last_scales = scales
                return
            dones = episode_starts[1:]          # row t = episode_starts[t + 1]
            _native.check(self.lib.vn_return_moments(p(rewards), p(dones), t0, t1, N, self.agent_id_base, self.gamma,
                                                     p(self.ret), p(part), stream), "vn_return_moments")
            allp = part if self.process_group is None else self._gather(part)
            _native.check(self.lib.vn_reward_normalize(p(rewards), t0, t1, N, p(allp), self.c_global, p(self.rms),
                                                       self.epsilon, self.clip_reward, 1, p(scales), stream),
                          "vn_reward_normalize")
        self.last_scales = scales
