"""BatchedGridEnv: N CubicEnv agents on one MI355X behind libvoxnav.

This replaces, for the hot path, what train/Grid_Train.py builds with
``SubprocVecEnv([make_env_fn(...) for i in range(NUM_ENVS)])``
(train/Grid_Train.py:120-126, :191-192): N independent ``GridAgent``
envs (envs/CubicEnv.py:15) with SB3 VecEnv auto-reset.  Inputs and outputs
are torch tensors resident on the GPU; nothing crosses PCIe per step.

Seeds.  ``reset(seed)`` with an int seeds agent i (global id
``agent_id_base + i``) with ``seed + gid``, the ``seed=42+i`` pattern of
Grid_Train's workers (:122-125).  After an auto-reset an agent's next
episode uses ``previous_seed + seed_stride`` (default: the global agent
count), all modulo 2**32, so every episode of every agent is reproducible
and identical for any sharding of the agents over GPUs.  (SB3 auto-resets
with ``seed=None``, i.e. OS entropy; the build pins the schedule instead.)
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Optional, Sequence, Union

import numpy as np
import torch

from . import _native
from .rooms import RoomSet, as_room_set

OBS_DIM = _native.VN_OBS_DIM
NUM_ACTIONS = 6
FINISH_PERCENTAGE = 0.84   # envs/CubicEnv.py:12
SEED_LIMIT = 2 ** 32       # np.random.seed range (envs/CubicEnv.py:80)


class StepResult(NamedTuple):
    obs: torch.Tensor            # f32 [N, obs_dim]  (post-reset obs for finished agents)
    reward: torch.Tensor         # f32 [N]  (or f64 with reward_f64=True)
    terminated: torch.Tensor     # bool [N]
    truncated: torch.Tensor      # bool [N]
    terminal_obs: Optional[torch.Tensor]  # f32 [N, obs_dim], rows valid where terminated|truncated


class Rollout(NamedTuple):
    obs: torch.Tensor            # f32 [K, N, obs_dim]
    reward: torch.Tensor         # f32 [K, N]
    terminated: torch.Tensor     # bool [K, N]
    truncated: torch.Tensor      # bool [K, N]
    actions: Optional[torch.Tensor]  # i32 [K, N]
    terminal_obs: Optional[torch.Tensor] = None  # f32 [K, N, obs_dim] (step_actions): rows valid where an episode ended


class FrontierDists(NamedTuple):
    """``BatchedGridEnv.plan_frontier_dists``: the planner's action and, per first action, its distance."""
    actions: torch.Tensor        # i32 [N]: plan_frontier's action
    dist: torch.Tensor           # i32 [N]: plan_frontier's dist (-1: the fallback)
    dists: torch.Tensor          # i32 [N, 6]: steps to the nearest target through action k; -1 unreached, -2 not passable
    best: torch.Tensor           # u8 [N]: bit k set iff dists[:, k] is the smallest positive entry


class EnvSnapshot(NamedTuple):
    """A whole-env raw snapshot (``BatchedGridEnv.snapshot``): opaque,
    layout-native bytes that only an env with the same tag can load."""
    tag: int                     # vn_snapshot_tag of the env that took it
    data: torch.Tensor           # uint8 [vn_snapshot_bytes], on the env's device
    t: int                       # the env's random-policy step counter


def _variant_code(v) -> int:
    if isinstance(v, str):
        try:
            return {"cubic": _native.VN_VARIANT_CUBIC, "simple": _native.VN_VARIANT_SIMPLE}[v.lower()]
        except KeyError:
            raise ValueError(f"variant must be 'cubic' or 'simple', got {v!r}") from None
    if int(v) not in (_native.VN_VARIANT_CUBIC, _native.VN_VARIANT_SIMPLE):
        raise ValueError(f"variant must be 0 (cubic) or 1 (simple), got {v!r}")
    return int(v)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream_ptr(device: torch.device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class BatchedGridEnv:
    """N GridAgents (envs/CubicEnv.py) stepping together on one GPU.

    Parameters mirror ``GridAgent.__init__`` (envs/CubicEnv.py:17-29):
    ``room_path`` (or an explicit ``rooms`` RoomSet), ``width/depth/height``
    for the ctor box used when no room path is given, ``local_map_length``
    and ``crash_penalty``.  ``num_agents`` is the batch, ``autoreset`` the
    VecEnv behaviour.  ``variant="simple"`` selects the goal-seeking
    envs/simpleEnv.py GridAgent (obs 6L+7) instead
    of envs/CubicEnv.py.  ``tuning`` names VnTuning fields (include/voxnav.h)
    to override for A/B timing and mode tests, e.g. ``{"pcache_cap": 0}``;
    the launch-time ones can be changed later with ``set_tuning``.
    """

    def __init__(self, num_agents: int = 1, room_path=None, rooms: Optional[RoomSet] = None,
                 local_map_length: int = 4, crash_penalty: float = -2.0, width: int = 20, depth: int = 20,
                 height: int = 12, autoreset: bool = True, device: Union[int, str, torch.device, None] = None,
                 agent_id_base: int = 0, seed_stride: Optional[int] = None,
                 finish_percentage: float = FINISH_PERCENTAGE, variant: Union[int, str] = "cubic", lib=None,
                 tuning: Optional[dict] = None):
        if not torch.cuda.is_available():
            raise _native.VoxnavError("BatchedGridEnv needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.lib = lib if lib is not None else _native.load()
        self.room_set = as_room_set(rooms, room_path, width, depth, height)
        # what clone() builds its env from (the parsed rooms stand in for room_path / width, depth, height)
        self._ctor = dict(num_agents=num_agents, rooms=self.room_set, local_map_length=local_map_length,
                          crash_penalty=crash_penalty, autoreset=autoreset, device=device, agent_id_base=agent_id_base,
                          seed_stride=seed_stride, finish_percentage=finish_percentage, variant=variant, lib=lib,
                          tuning=None if tuning is None else dict(tuning))
        self.num_agents = int(num_agents)
        self.local_map_length = int(local_map_length)
        if not 1 <= self.local_map_length <= _native.VN_MAX_L:
            raise ValueError(f"local_map_length must be in 1..{_native.VN_MAX_L}")
        self.crash_penalty = float(crash_penalty)
        self.autoreset = bool(autoreset)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if dev.type != "cuda":
            raise ValueError(f"device must be a GPU, got {dev}")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.agent_id_base = int(agent_id_base)
        self.seed_stride = int(seed_stride) if seed_stride is not None else self.num_agents
        self.variant = _variant_code(variant)
        whd, walls, fs, gl = self.room_set.pack(self.variant)
        rs = _native.VnRoomSet(len(self.room_set), whd.ctypes.data, walls.ctypes.data, fs.ctypes.data,
                               gl.ctypes.data)
        cfg = _native.VnConfig(self.local_map_length, int(self.room_set.use_room_draw), int(self.autoreset),
                               self.variant, self.crash_penalty, float(finish_percentage), self.agent_id_base,
                               self.seed_stride)
        h = C.c_void_p()
        self._tuning = None   # the VnTuning in force, once it is not the library's default
        with torch.cuda.device(self.device):
            if tuning is None:   # plain vn_create: what an older A/B build passed as lib= also has
                rc = self.lib.vn_create(C.byref(rs), self.num_agents, C.byref(cfg), self.device.index, C.byref(h))
            else:
                self._tuning = self._tuning_with(self._default_tuning(), tuning)
                rc = self.lib.vn_create_tuned(C.byref(rs), self.num_agents, C.byref(cfg), self.device.index,
                                              C.byref(self._tuning), C.byref(h))
            _native.check(rc, "vn_create")
        self._h = h
        info = _native.VnInfo()
        _native.check(self.lib.vn_get_info(self._h, C.byref(info)), "vn_get_info")
        self.info = info
        self.obs_dim = int(info.obs_dim)
        self.total_free_cells = np.asarray([r.total_free_cells_for(self.variant) for r in self.room_set.rooms],
                                           dtype=np.int64)
        self._was_reset = False
        self._t = 0   # global step counter for the random policy stream
        self.last_rejected = None   # device i32 [1]: agents the last import_state rejected

    # ------------------------------------------------------------------ utils
    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self.lib.vn_destroy(h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return _stream_ptr(self.device)

    def _default_tuning(self) -> _native.VnTuning:
        t = _native.VnTuning()
        _native.check(self.lib.vn_tuning_default(C.byref(t)), "vn_tuning_default")
        return t

    @staticmethod
    def _tuning_with(base: _native.VnTuning, fields: dict) -> _native.VnTuning:
        names = [f for f, _ in _native.VnTuning._fields_]
        t = _native.VnTuning.from_buffer_copy(base)
        for k, v in fields.items():
            if k not in names:
                raise ValueError(f"unknown tuning field {k!r} (VnTuning has {', '.join(names)})")
            setattr(t, k, int(v))
        return t

    def set_tuning(self, **fields):
        """Replace launch-time VnTuning fields (prio, dflush, wrec_k,
        wrec_early) of the live env; the library refuses a change of a
        creation-time field and leaves the env as it was."""
        cur = self._tuning if self._tuning is not None else self._default_tuning()
        t = self._tuning_with(cur, fields)
        _native.check(self.lib.vn_set_tuning(self._h, C.byref(t)), "vn_set_tuning")
        self._tuning = t

    def _seeds_tensor(self, seed) -> torch.Tensor:
        N = self.num_agents
        if seed is None:
            s = np.frombuffer(os.urandom(8 * N), dtype=np.uint64) % np.uint64(SEED_LIMIT)
            arr = s.astype(np.int64)
        elif isinstance(seed, (int, np.integer)):
            arr = int(seed) + self.agent_id_base + np.arange(N, dtype=np.int64)
        else:
            arr = np.asarray(seed.cpu() if isinstance(seed, torch.Tensor) else seed, dtype=np.int64).reshape(-1)
            if arr.size != N:
                raise ValueError(f"expected {N} seeds, got {arr.size}")
        if (arr < 0).any() or (arr >= SEED_LIMIT).any():
            raise ValueError("Seed must be between 0 and 2**32 - 1")   # np.random.seed (envs/CubicEnv.py:80)
        return torch.as_tensor(arr, dtype=torch.int64).to(self.device)

    # ------------------------------------------------------------------ API
    def reset(self, seed=None, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
        """GridAgent.reset(seed) for all agents (or those with mask[i]).

        Returns obs f32 [N, obs_dim] (rows of unmasked agents are left as in
        ``out`` / zero).
        """
        seeds = self._seeds_tensor(seed)
        if out is None:
            out = torch.zeros((self.num_agents, self.obs_dim), dtype=torch.float32, device=self.device)
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        _native.check(self.lib.vn_reset(self._h, _ptr(seeds), _ptr(m), _ptr(out), self._stream()), "vn_reset")
        self._was_reset = True
        return out

    def step(self, actions, reward_f64: bool = False, terminal_obs: bool = True) -> StepResult:
        """GridAgent.step(a) for every agent + SB3 auto-reset (envs/CubicEnv.py:110-132)."""
        if not self._was_reset:
            raise RuntimeError("call reset() before step()")
        N = self.num_agents
        a = torch.as_tensor(actions, device=self.device).to(torch.int32).reshape(N).contiguous()
        obs = torch.empty((N, self.obs_dim), dtype=torch.float32, device=self.device)
        rew = torch.empty(N, dtype=torch.float64 if reward_f64 else torch.float32, device=self.device)
        te = torch.empty(N, dtype=torch.uint8, device=self.device)
        tr = torch.empty(N, dtype=torch.uint8, device=self.device)
        tob = torch.zeros((N, self.obs_dim), dtype=torch.float32, device=self.device) if (terminal_obs and self.autoreset) else None
        _native.check(self.lib.vn_step(self._h, _ptr(a), _ptr(obs), None if reward_f64 else _ptr(rew),
                                       _ptr(rew) if reward_f64 else None, _ptr(te), _ptr(tr), _ptr(tob),
                                       self._stream()), "vn_step")
        return StepResult(obs, rew, te.bool(), tr.bool(), tob)

    def step_into(self, actions: torch.Tensor, obs: torch.Tensor, reward: torch.Tensor, terminated: torch.Tensor,
                  truncated: torch.Tensor, terminal_obs: Optional[torch.Tensor] = None,
                  reward64: Optional[torch.Tensor] = None):
        """``step`` writing into caller-owned device buffers (no allocation):
        actions i32 [N], obs f32 [N, obs_dim], reward f32 (or f64) [N],
        terminated / truncated u8 [N], terminal_obs f32 [N, obs_dim] or None;
        ``reward64`` (f64 [N], with an f32 ``reward``) also receives the exact
        f64 reward (what the Monitor sums)."""
        if not self._was_reset:
            raise RuntimeError("call reset() before step()")
        N = self.num_agents
        for name, t, dt, shape in (("actions", actions, torch.int32, (N,)), ("obs", obs, torch.float32, (N, self.obs_dim)),
                                   ("terminated", terminated, torch.uint8, (N,)),
                                   ("truncated", truncated, torch.uint8, (N,))):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"{name}: expected contiguous {dt} {shape} on {self.device}")
        if reward.dtype not in (torch.float32, torch.float64) or tuple(reward.shape) != (N,) or not reward.is_contiguous():
            raise ValueError("reward: expected contiguous f32/f64 [N]")
        f64 = reward.dtype == torch.float64
        if reward64 is not None:
            if f64 or reward64.dtype != torch.float64 or tuple(reward64.shape) != (N,) or not reward64.is_contiguous():
                raise ValueError("reward64: expected contiguous f64 [N] next to an f32 reward")
        r64 = reward if f64 else reward64
        _native.check(self.lib.vn_step(self._h, _ptr(actions), _ptr(obs), None if f64 else _ptr(reward),
                                       _ptr(r64), _ptr(terminated), _ptr(truncated),
                                       _ptr(terminal_obs), self._stream()), "vn_step")

    def step_random(self, k_steps: int, policy_seed: int = 42, t0: Optional[int] = None, record_actions: bool = False,
                    reward_f64: bool = False, out: Optional[Rollout] = None) -> Rollout:
        """k fused steps under the build's Philox uniform random policy."""
        if not self._was_reset:
            raise RuntimeError("call reset() before step_random()")
        K, N = int(k_steps), self.num_agents
        if t0 is None:
            t0 = self._t
        if out is None:
            obs = torch.empty((K, N, self.obs_dim), dtype=torch.float32, device=self.device)
            rew = torch.empty((K, N), dtype=torch.float64 if reward_f64 else torch.float32, device=self.device)
            te = torch.empty((K, N), dtype=torch.uint8, device=self.device)
            tr = torch.empty((K, N), dtype=torch.uint8, device=self.device)
            act = torch.empty((K, N), dtype=torch.int32, device=self.device) if record_actions else None
        else:
            self._check_rollout(out, K, reward_f64)
            obs, rew, te, tr, act = out[:5]
        _native.check(self.lib.vn_step_random(self._h, int(policy_seed), int(t0), K, _ptr(act), _ptr(obs),
                                              None if reward_f64 else _ptr(rew), _ptr(rew) if reward_f64 else None,
                                              _ptr(te), _ptr(tr), None, self._stream()), "vn_step_random")
        self._t = int(t0) + K
        return Rollout(obs, rew, te, tr, act)

    def step_actions(self, actions, reward_f64: bool = False, terminal_obs: bool = False,
                     out: Optional[Rollout] = None, reward64: Optional[torch.Tensor] = None) -> Rollout:
        """K fused steps of given actions (``vn_step_actions``): ``step``'s
        semantics per step, auto-reset included, ``step_random``'s [K, N, ...]
        output layout, one launch.  ``actions`` is int [K, N]; it comes back
        (as the int32 device tensor the kernel read) in ``Rollout.actions``.
        ``terminal_obs=True`` adds ``Rollout.terminal_obs`` [K, N, obs_dim],
        whose row [k, i] is written (else zero) where agent i's step k ended
        an episode.  ``reward64`` (f64 [K, N], next to an f32 reward) also
        receives the exact f64 rewards, as in ``step_into``.  The random
        policy's step counter advances by K."""
        if not self._was_reset:
            raise RuntimeError("call reset() before step_actions()")
        N = self.num_agents
        a = torch.as_tensor(actions, device=self.device).to(torch.int32)
        if a.dim() != 2 or a.shape[1] != N or a.shape[0] < 1:
            raise ValueError(f"actions: expected [K, {N}] with K >= 1, got {tuple(a.shape)}")
        a = a.contiguous()
        K = int(a.shape[0])
        if out is None:
            obs = torch.empty((K, N, self.obs_dim), dtype=torch.float32, device=self.device)
            rew = torch.empty((K, N), dtype=torch.float64 if reward_f64 else torch.float32, device=self.device)
            te = torch.empty((K, N), dtype=torch.uint8, device=self.device)
            tr = torch.empty((K, N), dtype=torch.uint8, device=self.device)
            tob = None
        else:
            self._check_rollout(out, K, reward_f64)
            obs, rew, te, tr = out[:4]
            tob = out.terminal_obs
            if tob is not None and (tob.dtype != torch.float32 or tuple(tob.shape) != (K, N, self.obs_dim)
                                    or not tob.is_contiguous() or tob.device != self.device):
                raise ValueError(f"out.terminal_obs: expected contiguous float32 {(K, N, self.obs_dim)} on {self.device}")
        if terminal_obs and tob is None:
            tob = torch.zeros((K, N, self.obs_dim), dtype=torch.float32, device=self.device)
        if reward64 is not None and (reward_f64 or reward64.dtype != torch.float64 or tuple(reward64.shape) != (K, N)
                                     or not reward64.is_contiguous() or reward64.device != self.device):
            raise ValueError(f"reward64: expected contiguous f64 {(K, N)} on {self.device} next to an f32 reward")
        _native.check(self.lib.vn_step_actions(self._h, _ptr(a), K, _ptr(obs), None if reward_f64 else _ptr(rew),
                                               _ptr(rew) if reward_f64 else _ptr(reward64), _ptr(te), _ptr(tr), _ptr(tob),
                                               self._stream()), "vn_step_actions")
        self._t += K
        return Rollout(obs, rew, te, tr, a, tob)

    def copy_agents(self, src_env: "BatchedGridEnv", src_index, seeds=None) -> torch.Tensor:
        """Agent i of this env becomes a layout-native copy of agent
        ``src_index[i]`` of ``src_env`` (-1: i keeps its state;
        ``vn_copy_agents``).  ``src_env`` may be this env, or any env on the
        same device built alike but for ``num_agents`` and ``agent_id_base``
        (same variant, rooms, config, ``seed_stride`` and creation-time
        tuning); both must have been reset.  ``seeds`` (int64 [N], optional):
        ``seeds[i] >= 0`` replaces the copied next auto-reset seed, -1 keeps
        the source's.  The episode records stay with the slots.  Returns the
        device int32 [1] count of destinations the device-side validation
        rejected and left untouched (an index or seed out of range; in place,
        a source that the same call writes); no host sync."""
        if not isinstance(src_env, BatchedGridEnv):
            raise TypeError("src_env must be a BatchedGridEnv")
        if not (self._was_reset and src_env._was_reset):
            raise RuntimeError("copy_agents() needs both envs reset (or imported / restored) before")
        if src_env.device != self.device:
            raise ValueError(f"src_env is on {src_env.device}, this env on {self.device}")
        N = self.num_agents
        idx = torch.as_tensor(src_index, device=self.device).to(torch.int32).reshape(-1).contiguous()
        if idx.numel() != N:
            raise ValueError(f"src_index: expected {N} entries, got {idx.numel()}")
        sd = None
        if seeds is not None:
            sd = torch.as_tensor(seeds, device=self.device).to(torch.int64).reshape(-1).contiguous()
            if sd.numel() != N:
                raise ValueError(f"seeds: expected {N} entries, got {sd.numel()}")
        rej = torch.zeros(1, dtype=torch.int32, device=self.device)
        _native.check(self.lib.vn_copy_agents(self._h, src_env._h, _ptr(idx), _ptr(sd), _ptr(rej), self._stream()),
                      "vn_copy_agents")
        self._was_reset = True
        return rej

    def plan_frontier(self, mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                      return_dist: bool = False):
        """The frontier planner (CubicEnv variant, padded rooms of at most
        64 x 64; ``vn_plan_frontier``): per agent the first action of a
        shortest path through cells it knows to be free to the nearest cell
        that is known free and not yet visited, from its own belief map on the
        device.  Returns actions int32 [N] (``out`` if given; rows of agents
        without ``mask[i]`` are left as they were, zero in a fresh tensor);
        with ``return_dist`` also dist int32 [N]: the number of steps to that
        cell, or -1 where none is reachable and the action is the fallback
        (the least-visited passable neighbour, 0 if there is none).  Reads the
        env only; stream-ordered, no host sync."""
        if not self._was_reset:
            raise RuntimeError("call reset() before plan_frontier()")
        N = self.num_agents
        if out is None:
            out = torch.zeros(N, dtype=torch.int32, device=self.device)
        elif out.dtype != torch.int32 or tuple(out.shape) != (N,) or not out.is_contiguous() or out.device != self.device:
            raise ValueError(f"out: expected contiguous int32 {(N,)} on {self.device}")
        m = None
        if mask is not None:
            m = torch.as_tensor(mask).to(device=self.device, dtype=torch.uint8).reshape(N).contiguous()
        dist = torch.full((N,), -1, dtype=torch.int32, device=self.device) if return_dist else None
        _native.check(self.lib.vn_plan_frontier(self._h, _ptr(m), _ptr(out), _ptr(dist), self._stream()),
                      "vn_plan_frontier")
        return (out, dist) if return_dist else out

    def plan_frontier_dists(self, mask: Optional[torch.Tensor] = None, out: Optional["FrontierDists"] = None):
        """The frontier planner's distance for each first action
        (``vn_plan_frontier_dists``; the rule is in include/voxnav.h).  Returns
        the named tuple ``(actions, dist, dists, best)``: ``actions`` / ``dist``
        int32 [N] exactly as ``plan_frontier`` gives them; ``dists`` int32
        [N, 6], per action the steps to the nearest target when the first step
        is that action, -1 where its cell is passable but reaches none, -2
        where it is not passable; ``best`` uint8 [N], bit k set where action k
        is among the shortest (0: the planner has only its fallback).  ``out``:
        a ``FrontierDists`` of contiguous tensors to write into; rows of agents
        without ``mask[i]`` are left as they were (in fresh tensors: action 0,
        dist -1, dists -2, best 0).  Reads the env only; stream-ordered."""
        if not self._was_reset:
            raise RuntimeError("call reset() before plan_frontier_dists()")
        N, dev = self.num_agents, self.device
        if out is None:
            out = FrontierDists(torch.zeros(N, dtype=torch.int32, device=dev),
                                torch.full((N,), -1, dtype=torch.int32, device=dev),
                                torch.full((N, 6), -2, dtype=torch.int32, device=dev),
                                torch.zeros(N, dtype=torch.uint8, device=dev))
        else:
            out = FrontierDists(*out)
            for name, t, dt, shape in (("actions", out.actions, torch.int32, (N,)), ("dist", out.dist, torch.int32, (N,)),
                                       ("dists", out.dists, torch.int32, (N, 6)), ("best", out.best, torch.uint8, (N,))):
                if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                    raise ValueError(f"out.{name}: expected contiguous {dt} {shape} on {dev}")
        m = None
        if mask is not None:
            m = torch.as_tensor(mask).to(device=dev, dtype=torch.uint8).reshape(N).contiguous()
        _native.check(self.lib.vn_plan_frontier_dists(self._h, _ptr(m), _ptr(out.actions), _ptr(out.dist),
                                                      _ptr(out.dists), _ptr(out.best), self._stream()),
                      "vn_plan_frontier_dists")
        return out

    def _check_rollout(self, out: Rollout, K: int, reward_f64: bool):
        """A caller-owned [K, N, ...] rollout chunk: the kernel writes all K
        steps, so a short or mistyped buffer is refused here."""
        N, dev = self.num_agents, self.device
        obs, rew, te, tr, act = out[:5]
        rdt = torch.float64 if reward_f64 else torch.float32
        for name, t, dt, shape in (("obs", obs, torch.float32, (K, N, self.obs_dim)), ("reward", rew, rdt, (K, N)),
                                   ("terminated", te, torch.uint8, (K, N)), ("truncated", tr, torch.uint8, (K, N))):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"out.{name}: expected contiguous {dt} {shape} on {dev}")
        if act is not None and (act.dtype != torch.int32 or tuple(act.shape) != (K, N) or not act.is_contiguous()
                                or act.device != dev):
            raise ValueError(f"out.actions: expected contiguous int32 {(K, N)} on {dev}")

    def step_random_launcher(self, k_steps: int, policy_seed: int, t0: int, out: Rollout, reward_f64: bool = False):
        """``step_random(k_steps, policy_seed, t0, out=out)`` prepared: the
        argument checks and conversions happen here, and the returned
        zero-argument callable is one C call on the current stream (for timed
        loops whose host overhead per launch should be the launch itself)."""
        if not self._was_reset:
            raise RuntimeError("call reset() before step_random()")
        K = int(k_steps)
        self._check_rollout(out, K, reward_f64)
        obs, rew, te, tr, act = out[:5]
        args = (self._h, int(policy_seed), int(t0), K, _ptr(act), _ptr(obs), None if reward_f64 else _ptr(rew),
                _ptr(rew) if reward_f64 else None, _ptr(te), _ptr(tr), None, self._stream())
        fn = self.lib.vn_step_random
        t_end = int(t0) + K

        def launch():
            rc = fn(*args)
            if rc:
                _native.check(rc, "vn_step_random")
            self._t = t_end          # a later step_random() without t0 continues after this launch
        launch.out = out             # args holds raw device pointers: keep the tensors alive with the callable
        return launch

    def kernel_label(self, k_steps: int = 16, explicit_actions: bool = False, fast: bool = True) -> str:
        """Name of the kernel instantiation a step call of this shape launches
        (``k_steps=0``: reset; ``fast``: the rollout-buffer call)."""
        buf = C.create_string_buffer(160)
        _native.check(self.lib.vn_kernel_label(self._h, int(k_steps), int(bool(explicit_actions)), int(bool(fast)),
                                               buf, 160), "vn_kernel_label")
        return buf.value.decode()

    def kernel_box(self, k_steps: int = 16, explicit_actions: bool = False, fast: bool = True) -> bool:
        """Whether that call launches the label's BOX instantiation, which
        computes the ray record of an exact box instead of loading it
        (``vn_kernel_box``; tuning ``prio`` bit 8 keeps such an env on the table)."""
        box = C.c_int32(0)
        _native.check(self.lib.vn_kernel_box(self._h, int(k_steps), int(bool(explicit_actions)), int(bool(fast)),
                                             C.byref(box)), "vn_kernel_box")
        return bool(box.value)

    def export_state(self) -> torch.Tensor:
        out = torch.empty((self.num_agents, _native.VN_STATE_FIELDS), dtype=torch.int64, device=self.device)
        _native.check(self.lib.vn_export_state(self._h, _ptr(out), self._stream()), "vn_export_state")
        return out

    def state(self) -> dict:
        s = self.export_state().cpu().numpy()
        return {f: s[:, i] for i, f in enumerate(_native.STATE_FIELDS)}

    def belief(self) -> torch.Tensor:
        """int8 [N, pad_w, pad_d, pad_h], the reference's internal_grid values
        (CubicEnv: counts saturate at 63; simpleEnv: -1/0/1/2); -128 outside
        the agent's room."""
        i = self.info
        out = torch.empty((self.num_agents, i.pad_w, i.pad_d, i.pad_h), dtype=torch.int8, device=self.device)
        _native.check(self.lib.vn_export_belief(self._h, _ptr(out), self._stream()), "vn_export_belief")
        return out

    def action_masks(self, obs: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 [N]: bit a set iff action a taken on observation ``obs`` [N, 80]
        would not bump (``voxnav.masking.action_masks``; CubicEnv variant only)."""
        if self.variant != _native.VN_VARIANT_CUBIC:
            raise ValueError("action masks are read off the CubicEnv observation (variant='cubic')")
        from .masking import action_masks
        return action_masks(obs, out)

    # ------------------------------------------------------- episode records
    def episode_records(self) -> torch.Tensor:
        """int64 [N, 12] (``_native.EPISODE_FIELDS``): per agent the totals
        over every episode it ended since creation or the last clear
        (``episodes``, ``finished``, ``sum_steps``, ``sum_bumps``,
        ``sum_visited``, ``sum_max_steps``) and its last ended episode
        (``last_steps``, ``last_bumps``, ``last_visited``, ``last_max_steps``,
        ``last_room``, ``last_flags``: bit 0 terminated, bit 1 truncated) --
        what envs/CubicEnv.py:212-222 prints at every episode end, written by
        the step kernels before the auto-reset.  Stream-ordered, no host sync."""
        out = torch.empty((self.num_agents, _native.VN_EPISODE_FIELDS), dtype=torch.int64, device=self.device)
        _native.check(self.lib.vn_episode_records(self._h, _ptr(out), self._stream()), "vn_episode_records")
        return out

    def episode_totals(self) -> torch.Tensor:
        """int64 [6]: the six totals of ``episode_records`` summed over all
        agents on the device (exact integer sums)."""
        out = torch.empty(6, dtype=torch.int64, device=self.device)
        _native.check(self.lib.vn_episode_totals(self._h, _ptr(out), self._stream()), "vn_episode_totals")
        return out

    def clear_episode_records(self, mask: Optional[torch.Tensor] = None) -> None:
        """Zero the episode records of the agents with ``mask[i]`` (None: all)."""
        m = None
        if mask is not None:
            m = torch.as_tensor(mask).to(device=self.device, dtype=torch.uint8).reshape(self.num_agents).contiguous()
        _native.check(self.lib.vn_episode_clear(self._h, _ptr(m), self._stream()), "vn_episode_clear")

    # ------------------------------------------------- state import, snapshots
    def import_state(self, state: torch.Tensor, belief: torch.Tensor, mask: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None, check: bool = True) -> torch.Tensor:
        """The exports' other direction (CubicEnv variant; ``vn_import_state``):
        agent i takes the attributes of ``state[i]`` (``export_state``'s 16
        int64 fields) and the map ``belief[i]`` (``belief()``'s int8
        encoding), for the agents with ``mask[i]`` (None: all), in whatever
        belief layout this env has.  Returns obs f32 [N, 80]: ``get_obs()``
        of the imported agents (rows of the others as in ``out`` / zero).
        Agents the device-side validation rejects are left untouched;
        ``check=True`` reads their count back and raises ``VoxnavError``
        naming it."""
        N, i = self.num_agents, self.info
        st = torch.as_tensor(state).to(device=self.device, dtype=torch.int64).contiguous()
        bl = torch.as_tensor(belief).to(device=self.device, dtype=torch.int8).contiguous()
        if tuple(st.shape) != (N, _native.VN_STATE_FIELDS):
            raise ValueError(f"state: expected [{N}, {_native.VN_STATE_FIELDS}], got {tuple(st.shape)}")
        if tuple(bl.shape) != (N, i.pad_w, i.pad_d, i.pad_h):
            raise ValueError(f"belief: expected {(N, i.pad_w, i.pad_d, i.pad_h)}, got {tuple(bl.shape)}")
        m = None
        if mask is not None:
            m = torch.as_tensor(mask).to(device=self.device, dtype=torch.uint8).reshape(N).contiguous()
            if not self._was_reset:
                raise ValueError("a partial import needs an env that was reset (or fully imported) before")
        if out is None:
            out = torch.zeros((N, self.obs_dim), dtype=torch.float32, device=self.device)
        elif (out.dtype != torch.float32 or tuple(out.shape) != (N, self.obs_dim) or not out.is_contiguous()
              or out.device != self.device):
            raise ValueError(f"out: expected contiguous float32 {(N, self.obs_dim)} on {self.device}")
        rej = torch.zeros(1, dtype=torch.int32, device=self.device)
        _native.check(self.lib.vn_import_state(self._h, _ptr(st), _ptr(bl), _ptr(m), _ptr(out), _ptr(rej),
                                               self._stream()), "vn_import_state")
        self.last_rejected = rej          # device i32 [1]: what check=False callers may read later
        if check:
            n = int(rej.item())
            if n:
                raise _native.VoxnavError(f"vn_import_state rejected {n} of {N} agents (left untouched)")
        if m is None:
            self._was_reset = True
        return out

    def _snapshot_tag(self) -> int:
        tag = C.c_uint64()
        _native.check(self.lib.vn_snapshot_tag(self._h, C.byref(tag)), "vn_snapshot_tag")
        return int(tag.value)

    def snapshot(self) -> EnvSnapshot:
        """A raw copy of every mutable per-agent buffer (both variants, every
        layout), taken on the current stream."""
        n = C.c_int64()
        _native.check(self.lib.vn_snapshot_bytes(self._h, C.byref(n)), "vn_snapshot_bytes")
        data = torch.empty(int(n.value), dtype=torch.uint8, device=self.device)
        _native.check(self.lib.vn_snapshot_save(self._h, _ptr(data), self._stream()), "vn_snapshot_save")
        return EnvSnapshot(self._snapshot_tag(), data, int(self._t))

    def restore(self, snap: EnvSnapshot) -> None:
        """Load a snapshot taken from this env or from one built alike (same
        variant, agents, rooms, config and creation-time tuning); any other
        raises ``VoxnavError`` and leaves this env as it was."""
        data = snap.data.to(device=self.device, dtype=torch.uint8).contiguous()
        n = C.c_int64()
        _native.check(self.lib.vn_snapshot_bytes(self._h, C.byref(n)), "vn_snapshot_bytes")
        if int(snap.tag) == self._snapshot_tag() and data.numel() != int(n.value):
            raise ValueError(f"snapshot holds {data.numel()} bytes, this env's snapshots have {int(n.value)}")
        _native.check(self.lib.vn_snapshot_load(self._h, _ptr(data), int(snap.tag), self._stream()),
                      "vn_snapshot_load")
        self._t = int(snap.t)
        self._was_reset = True

    def clone(self) -> "BatchedGridEnv":
        """A new env built from the same arguments, in this env's state."""
        other = BatchedGridEnv(**self._ctor)
        if self._tuning is not None:      # launch-time fields changed by set_tuning
            other.set_tuning(**{f: getattr(self._tuning, f) for f in ("prio", "dflush", "wrec_k", "wrec_early")})
        if self._was_reset:
            other.restore(self.snapshot())
        return other
