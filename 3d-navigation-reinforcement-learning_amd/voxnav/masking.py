"""Invalid-action masks of CubicEnv observations (Huang & Ontanon 2020; what
sb3_contrib ``MaskablePPO`` reads through ``env.action_masks()``).

A mask is one byte per agent: bit ``a`` (0 fwd, 1 right, 2 back, 3 left, 4 up,
5 down) is set iff action ``a`` taken now would not bump.  It is read off the
observation alone (``vn_action_mask``, include/voxnav.h has the formula and
why it is exact): the six neighbour cells lie inside the 4x4x4 window, and
``get_obs`` has ray-cast every one of them before it builds the window
(envs/CubicEnv.py:229-275, :322-332), so a neighbour reads known wall, known
free or -- only out of bounds -- unknown.

The collector draws from the masked head (``RolloutCollector(...,
action_masks=True)``, ``vn_policy_head_masked``) and the learner trains on the
masked loss (``PPOLearner(..., action_masks=True)``, ``vn_ppo_loss_masked``).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native

NUM_ACTIONS = 6
OBS_DIM = _native.VN_OBS_DIM


def action_masks(obs: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [N]: the masks of CubicEnv observations ``obs`` f32 [N, 80] on the
    GPU (rows may be strided), one launch on the current stream, no host sync."""
    if obs.dim() != 2 or obs.shape[1] != OBS_DIM or obs.dtype != torch.float32 or not obs.is_cuda or \
            obs.stride(1) != 1 or obs.shape[0] < 1 or obs.stride(0) < OBS_DIM:
        raise ValueError(f"action_masks: obs must be f32 [N, {OBS_DIM}] rows on the GPU (a CubicEnv observation)")
    n = obs.shape[0]
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=obs.device)
    elif out.dtype != torch.uint8 or out.shape != (n,) or not out.is_contiguous() or out.device != obs.device:
        raise ValueError("action_masks: out must be contiguous uint8 [N] on the observations' device")
    stream = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
    _native.check(_native.load().vn_action_mask(C.c_void_p(obs.data_ptr()), obs.stride(0), n,
                                                C.c_void_p(out.data_ptr()), stream), "vn_action_mask")
    return out


def mask_to_bool(mask: torch.Tensor) -> torch.Tensor:
    """bool [N, 6] of a uint8 [N] mask (``MaskablePPO``'s layout)."""
    bits = torch.arange(NUM_ACTIONS, device=mask.device, dtype=torch.int32)
    return ((mask.to(torch.int32).unsqueeze(-1) >> bits) & 1).bool()
