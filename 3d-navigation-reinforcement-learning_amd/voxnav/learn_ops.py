"""The PPO learner's matrix products on the f32 matrix cores (no library GEMM).

Autograd functions over the HIP kernels of csrc/voxnav_gemm_f32.hip for the
learner's Linear layers (SB3 ``MlpExtractor`` + ``action_net`` /
``value_net``, reached from ``RecurrentPPO.train`` / ``PPO.train`` at
train/Grid_Train.py:228) and the LSTM weight gradients:

* ``linear_tanh_pair``: one Tanh layer of BOTH branches (pi, vf) per launch,
  forward ``tanh(x W^T + b)``; backward ``dX = (dY (1 - Y^2)) W`` with the
  Tanh backward formed on the operand load, ``dW = dZ^T X`` split over the
  sample axis (per-split partials summed in order) and ``db = sum dZ`` from
  the same staged tiles;
* ``linear``: a Linear without activation (the heads), same backward;
* ``mm_tn``: ``a^T b`` over a tall sample axis (+ the column sums of a).

f32 throughout (the reference's dtype).  CUDA tensors only; the CPU path
(the CPU parity tests) uses torch's own ops.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch

from . import _native

SPLIT_ROWS = 256         # minimum rows of the sample axis per split of a weight-gradient product


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _splits(K: int, tiles: int) -> int:
    """Split count for a K-long reduction whose output has `tiles` 128x128 tiles:
    enough blocks to fill the chip (>= ~512), at least SPLIT_ROWS rows each."""
    want = max(1, -(-512 // max(1, tiles)))
    sp = max(1, min(want, 256, K // SPLIT_ROWS))
    # a multiple of 8 when it can be: the kernel then deals whole splits to one
    # XCD each (csrc/voxnav_gemm_f32.hip), so a split's operand rows are read
    # into one L2
    return sp if sp < 8 else sp // 8 * 8


def mm_tn(a: torch.Tensor, b: torch.Tensor, y: Optional[torch.Tensor] = None, colsum: bool = False,
          out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """Batched ``z^T b`` with z = a (1 - y^2) if y is given else a.
    a, y: [batch, K, M]; b: [batch, K, N] (batch stride 0 allowed via expand);
    returns ([batch, M, N], [batch, M] column sums of z or None)."""
    lib = _native.load()
    Bt, K, M = a.shape
    N = b.shape[2]
    dev = a.device
    if a.stride(2) != 1 or a.stride(1) != M or b.stride(2) != 1 or b.stride(1) != N:
        raise ValueError("mm_tn: operands must be row-contiguous [batch, K, cols]")
    if y is not None and (y.shape != a.shape or y.stride() != a.stride() or y.dtype != a.dtype or
                          y.device != a.device):
        raise ValueError("mm_tn: y must have a's shape, strides, dtype and device (the kernel reads both "
                         "with one row and batch stride)")
    tiles = -(-M // 128) * -(-N // 128) * Bt
    sp = _splits(K, tiles)
    out = torch.empty((Bt, M, N), dtype=torch.float32, device=dev) if out is None else out
    ws = torch.empty(sp * Bt * M * N, dtype=torch.float32, device=dev)
    cs = torch.empty((Bt, M), dtype=torch.float32, device=dev) if colsum else None
    ws2 = torch.empty(sp * Bt * M, dtype=torch.float32, device=dev) if colsum else None
    _native.check(lib.vn_gemm_f32_tn(_p(a), _p(y), M, a.stride(0), _p(b), N, b.stride(0), _p(out), M * N, _p(cs),
                                     M, N, K, Bt, sp, _p(ws), _p(ws2), 0, _stream(dev)), "vn_gemm_f32_tn")
    return out, cs


def _pair_stride(a: torch.Tensor, b: torch.Tensor) -> int:
    """Element offset from tensor a to tensor b (same shape, contiguous f32):
    the kernels' batch stride, so the two branches' parameters are read in
    place instead of stacked into a [2, ...] copy every minibatch."""
    d = b.data_ptr() - a.data_ptr()
    if d % 4 or a.shape != b.shape or not (a.is_contiguous() and b.is_contiguous()):
        raise ValueError("pair operands must be contiguous f32 tensors of one shape")
    return d // 4


class _LinearTanhPair(torch.autograd.Function):
    """y[br] = tanh(x[br] W[br]^T + b[br]) for br in (pi, vf): x [2, M, K]
    (batch stride 0 when both branches read the same input), W_pi, W_vf
    [N, K], b_pi, b_vf [N] (read in place: the batch stride is the distance
    between the two tensors)."""

    @staticmethod
    def forward(ctx, x, wa, wb, ba, bb, tanh: bool):
        lib = _native.load()
        _, M, K = x.shape
        N = wa.shape[0]
        dev = x.device
        y = torch.empty((2, M, N), dtype=torch.float32, device=dev)
        sw, sb = _pair_stride(wa, wb), _pair_stride(ba, bb)
        _native.check(lib.vn_gemm_f32_linear(_p(x), K, x.stride(0), _p(wa), K, sw, _p(ba), sb, _p(y), N, M * N, M, N,
                                             K, 2, 1 if tanh else 0, _stream(dev)), "vn_gemm_f32_linear")
        ctx.save_for_backward(x, wa, wb, y)
        ctx.tanh = tanh
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _native.load()
        x, wa, wb, y = ctx.saved_tensors
        _, M, K = x.shape
        N = wa.shape[0]
        dev = x.device
        st = _stream(dev)
        dy = dy.contiguous()
        yy = y if ctx.tanh else None
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((2, M, K), dtype=torch.float32, device=dev)
            # dX = dZ W: W [N][K] row-major is the k-major operand of this product
            _native.check(lib.vn_gemm_f32_dx(_p(dy), _p(yy), N, M * N, _p(wa), K, _pair_stride(wa, wb), _p(dx), K,
                                             M * K, M, K, N, 2, st), "vn_gemm_f32_dx")
            # (a shared input was expanded outside: expand's backward sums the branches)
        dw, db = mm_tn(dy, x, y=yy, colsum=True)
        return dx, dw[0], dw[1], db[0], db[1], None


def linear_tanh_pair(x: torch.Tensor, w, b, tanh: bool = True) -> torch.Tensor:
    """x [2, M, K] (or [M, K], shared by both branches); w = (W_pi, W_vf) [N, K]
    each (or one stacked [2, N, K]), b = (b_pi, b_vf) [N] (or [2, N]) -> [2, M, N]."""
    if x.dim() == 2:
        x = x.contiguous().unsqueeze(0).expand(2, *x.shape)
    elif not x.is_contiguous():
        x = x.contiguous()
    if isinstance(w, torch.Tensor):
        w = (w[0], w[1])
    if isinstance(b, torch.Tensor):
        b = (b[0], b[1])
    return _LinearTanhPair.apply(x, w[0], w[1], b[0], b[1], tanh)


class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        lib = _native.load()
        M, K = x.shape
        N = w.shape[0]
        dev = x.device
        y = torch.empty((M, N), dtype=torch.float32, device=dev)
        _native.check(lib.vn_gemm_f32_linear(_p(x), K, 0, _p(w), K, 0, _p(b), 0, _p(y), N, 0, M, N, K, 1, 0,
                                             _stream(dev)), "vn_gemm_f32_linear")
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _native.load()
        x, w = ctx.saved_tensors
        M, K = x.shape
        N = w.shape[0]
        dev = x.device
        dy = dy.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((M, K), dtype=torch.float32, device=dev)
            _native.check(lib.vn_gemm_f32_dx(_p(dy), None, N, 0, _p(w), K, 0, _p(dx), K, 0, M, K, N, 1, _stream(dev)),
                          "vn_gemm_f32_dx")
        dw, db = mm_tn(dy.unsqueeze(0), x.unsqueeze(0), colsum=True)
        return dx, dw[0], db[0]


def linear(x: torch.Tensor, module: torch.nn.Linear) -> torch.Tensor:
    """``module(x)`` for 2-D x on the matrix-core kernels (CUDA), torch otherwise."""
    if x.device.type != "cuda":
        return module(x)
    return _Linear.apply(x.contiguous(), module.weight, module.bias)


def mlp_pair(pi_net: torch.nn.Sequential, vf_net: torch.nn.Sequential, x_pi: torch.Tensor,
             x_vf: Optional[torch.Tensor] = None, x_pair: Optional[torch.Tensor] = None, stacked: bool = False):
    """Both SB3 MLP branches (Linear + Tanh layers of equal widths) layer by
    layer, the two branches of a layer in one launch.  ``x_vf is None``: both
    read ``x_pi`` (MlpPolicy's observation).  ``x_pair`` [2, M, K]: the two
    branches' inputs already stacked (the row-layout LSTM's output), used
    as is -- no stacking copy forward, no gradient accumulation backward.
    Returns (h_pi, h_vf); with ``stacked`` the [2, M, F] pair itself, or None
    when the branches do not take the paired kernels."""
    def tanh_layers(seq):   # [Linear, Tanh] * n, or None
        mods = list(seq)
        if len(mods) % 2 or not all(isinstance(a, torch.nn.Linear) and a.bias is not None and
                                    isinstance(t, torch.nn.Tanh) for a, t in zip(mods[0::2], mods[1::2])):
            return None
        return mods[0::2]
    lin_pi, lin_vf = tanh_layers(pi_net), tanh_layers(vf_net)
    if x_pair is not None:
        x_pi, x_vf = x_pair[0], x_pair[1]
    if (x_pi.device.type != "cuda" or lin_pi is None or lin_vf is None or len(lin_pi) != len(lin_vf) or
            any(a.weight.shape != b.weight.shape for a, b in zip(lin_pi, lin_vf))):
        if stacked:
            return None
        return pi_net(x_pi), vf_net(x_pi if x_vf is None else x_vf)
    h = x_pair if x_pair is not None else (x_pi if x_vf is None else torch.stack([x_pi, x_vf]))
    for a, b in zip(lin_pi, lin_vf):
        h = linear_tanh_pair(h, (a.weight, b.weight), (a.bias, b.bias), tanh=True)
    return h if stacked else (h[0], h[1])


def ppo_loss_supported(action_net: torch.nn.Linear, value_net: torch.nn.Linear, F: int) -> bool:
    """The fused loss kernel takes these heads (F = latent width)."""
    return (F % 64 == 0 and 64 <= F <= 256 and action_net.in_features == F and value_net.in_features == F and
            value_net.out_features == 1 and 1 <= action_net.out_features <= 8 and action_net.bias is not None and
            value_net.bias is not None)


def _head_loss(name: str, h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear,
               src: Optional[torch.Tensor], buffers, what: str, scalars, adv_words: int = 0,
               n_stats: int = 6):
    """What ppo_loss, bc_loss and bc_loss_set share (csrc/head_loss.h is their one kernel): the
    checks, the workspaces, the call of ``vn_<name>`` and the views of the head gradients.
    ``buffers``: the entry point's gathered buffers as (tensor or None, dtype), in its argument
    order (an entry with dtype None is a ctypes scalar among them, passed as it is: the soft
    entries' ``ldd``); ``scalars``: its arguments between the sizes and the outputs; ``adv_words``: f64
    words of vn_ppo_loss' advantage sums, passed before the partials; ``n_stats``: the entry
    point's stats words."""
    lib = _native.load()
    _, M, F = h.shape
    A = action_net.out_features
    dev = h.device
    if h.stride(2) != 1 or h.stride(1) != F:
        raise ValueError(f"{name}: latents must be row-contiguous [2, M, F]")
    for t, dt in buffers:
        if dt is not None and t is not None and (t.dtype != dt or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"{name}: buffers must be contiguous {what} on the latents' device")
    if src is not None and (src.dtype != torch.int64 or src.numel() != M or not src.is_contiguous()):
        raise ValueError(f"{name}: src must be [M] contiguous int64")
    npart, nspart = C.c_int64(), C.c_int64()
    sizes = ("vn_bc_loss_part_floats" if name.startswith("bc_") else
             "vn_ppo_bc_loss_part_floats" if name.startswith("ppo_bc_") else
             "vn_ppo_loss_masked_part_floats" if name.startswith("ppo_loss_masked") else "vn_ppo_loss_part_floats")
    _native.check(getattr(lib, sizes)(M, F, A, C.byref(npart), C.byref(nspart)), sizes)
    dh = torch.empty((2, M, F), dtype=torch.float32, device=dev)
    gh = torch.empty(A * F + A + F + 1, dtype=torch.float32, device=dev)
    dbl = torch.empty(n_stats + adv_words + nspart.value, dtype=torch.float64, device=dev)
    part = torch.empty(npart.value, dtype=torch.float32, device=dev)
    stats = dbl[:n_stats]
    wa, ba = action_net.weight.detach(), action_net.bias.detach()
    wv, bv = value_net.weight.detach(), value_net.bias.detach()
    adv_sums = (_p(dbl[n_stats:n_stats + adv_words]),) if adv_words else ()
    _native.check(getattr(lib, "vn_" + name)(_p(h[0]), _p(h[1]), F, _p(wa.contiguous()), _p(ba), _p(wv.contiguous()),
                                              _p(bv), _p(src), *[t if dt is None else _p(t) for t, dt in buffers],
                                              M, F, A, *scalars,
                                              _p(dh[0]), _p(dh[1]), _p(gh), _p(stats), *adv_sums, _p(part),
                                              _p(dbl[n_stats + adv_words:]), _stream(dev)), "vn_" + name)
    grads = (gh[:A * F].view(A, F), gh[A * F:A * F + A], gh[A * F + A:A * F + A + F].view(1, F), gh[-1:])
    return dh, grads, stats


def ppo_loss(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear, src: Optional[torch.Tensor],
             actions: torch.Tensor, advantages: torch.Tensor, old_log_prob: torch.Tensor, returns: torch.Tensor,
             clip_range: float, ent_coef: float, vf_coef: float, normalize_advantage: bool):
    """The PPO minibatch loss and its gradient (csrc/voxnav_ppo_loss.hip): the
    heads, the advantage normalisation, the clipped surrogate, value MSE and
    entropy bonus of sb3 (Recurrent)PPO.train, in three launches.

    h [2, M, F]: the (actor, critic) latents; src [M] int64 (or None): the
    samples' rows in the flat rollout buffers ``actions`` (int32),
    ``advantages``, ``old_log_prob``, ``returns``.  Returns (dh [2, M, F],
    (d action_net.weight, d action_net.bias, d value_net.weight,
    d value_net.bias), stats f64 [6]: policy loss, value loss, entropy loss,
    loss, approx kl, clip fraction).  Nothing is differentiated here: the
    caller backpropagates dh from h and assigns the head gradients."""
    return _head_loss("ppo_loss", h, action_net, value_net, src,
                      ((actions, torch.int32), (advantages, torch.float32), (old_log_prob, torch.float32),
                       (returns, torch.float32)), "int32 actions / f32 values",
                      (float(clip_range), float(ent_coef), float(vf_coef), int(bool(normalize_advantage))),
                      adv_words=128)


def ppo_loss_masked(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear,
                    src: Optional[torch.Tensor], actions: torch.Tensor, advantages: torch.Tensor,
                    old_log_prob: torch.Tensor, returns: torch.Tensor, action_masks: torch.Tensor, clip_range: float,
                    ent_coef: float, vf_coef: float, normalize_advantage: bool):
    """``ppo_loss`` with invalid-action masking (csrc/voxnav_masked_loss.hip, the
    formula in include/voxnav.h vn_ppo_loss_masked): ``action_masks`` uint8, a
    flat rollout buffer like the others, bit j set where action j was allowed;
    each sample's softmax, log-prob and entropy run over its allowed actions
    (the taken one always among them), and the logits of the others get a
    gradient of exactly 0.  Arguments, outputs and stats as ``ppo_loss``."""
    return _head_loss("ppo_loss_masked", h, action_net, value_net, src,
                      ((actions, torch.int32), (advantages, torch.float32), (old_log_prob, torch.float32),
                       (returns, torch.float32), (action_masks, torch.uint8)),
                      "int32 actions / f32 values / uint8 masks",
                      (float(clip_range), float(ent_coef), float(vf_coef), int(bool(normalize_advantage))),
                      adv_words=128)


def _check_clip_range_vf(name: str, old_values, clip_range_vf) -> float:
    if old_values is None:
        raise ValueError(f"{name}: old_values is required (the rollout's f32 values)")
    c = float(clip_range_vf)
    if not c > 0.0:                       # also NaN
        raise ValueError(f"{name}: clip_range_vf must be > 0 (inf: no clip), got {clip_range_vf!r}")
    return c


def ppo_loss_vclip(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear,
                   src: Optional[torch.Tensor], actions: torch.Tensor, advantages: torch.Tensor,
                   old_log_prob: torch.Tensor, returns: torch.Tensor, old_values: torch.Tensor, clip_range: float,
                   clip_range_vf: float, ent_coef: float, vf_coef: float, normalize_advantage: bool):
    """``ppo_loss`` with the value update clipped (csrc/voxnav_vclip_loss.hip, the
    formula in include/voxnav.h vn_ppo_loss_vclip; sb3's ``clip_range_vf``):
    ``old_values`` f32, a flat rollout buffer like ``returns`` (the values the
    rollout stored); the value loss is on ``v`` clamped to ``old_values`` +-
    ``clip_range_vf``, and a sample outside that range gets no value gradient.
    ``clip_range_vf=inf`` gives ``ppo_loss``'s bits.  Arguments, outputs and
    stats otherwise as ``ppo_loss``."""
    c = _check_clip_range_vf("ppo_loss_vclip", old_values, clip_range_vf)
    return _head_loss("ppo_loss_vclip", h, action_net, value_net, src,
                      ((actions, torch.int32), (advantages, torch.float32), (old_log_prob, torch.float32),
                       (returns, torch.float32), (old_values, torch.float32)), "int32 actions / f32 values",
                      (float(clip_range), c, float(ent_coef), float(vf_coef), int(bool(normalize_advantage))),
                      adv_words=128)


def ppo_loss_masked_vclip(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear,
                          src: Optional[torch.Tensor], actions: torch.Tensor, advantages: torch.Tensor,
                          old_log_prob: torch.Tensor, returns: torch.Tensor, action_masks: torch.Tensor,
                          old_values: torch.Tensor, clip_range: float, clip_range_vf: float, ent_coef: float,
                          vf_coef: float, normalize_advantage: bool):
    """``ppo_loss_masked`` with ``ppo_loss_vclip``'s clipped value update
    (``vn_ppo_loss_masked_vclip``)."""
    _required_masks("ppo_loss_masked_vclip", action_masks)
    c = _check_clip_range_vf("ppo_loss_masked_vclip", old_values, clip_range_vf)
    return _head_loss("ppo_loss_masked_vclip", h, action_net, value_net, src,
                      ((actions, torch.int32), (advantages, torch.float32), (old_log_prob, torch.float32),
                       (returns, torch.float32), (action_masks, torch.uint8), (old_values, torch.float32)),
                      "int32 actions / f32 values / uint8 masks",
                      (float(clip_range), c, float(ent_coef), float(vf_coef), int(bool(normalize_advantage))),
                      adv_words=128)


def kl_gate(stats: torch.Tensor, threshold: float, stop: torch.Tensor, skip: torch.Tensor,
            ran: Optional[torch.Tensor] = None, err: Optional[torch.Tensor] = None, kl_index: int = 4) -> None:
    """The learner's KL gate (csrc/voxnav_trust.hip, the rule in include/voxnav.h
    vn_kl_gate), one launch between a fused loss and ``adam_step``: ``stop``
    (int32 word, sticky, zeroed by the caller) is set when it was 0 and
    ``stats[kl_index]`` (f64) > ``threshold``; ``ran`` (uint8, optional) receives
    whether it was 0 on entry -- the minibatch counts in the logs; ``skip``
    (int32) receives ``stop`` or-ed with ``err`` (int32, optional: the row-layout
    LSTM's error word) for ``adam_step(skip=...)``.  Nothing is read back."""
    dev = stats.device
    for t, dt, what in ((stats, torch.float64, "stats"), (stop, torch.int32, "stop"), (skip, torch.int32, "skip"),
                        (ran, torch.uint8, "ran"), (err, torch.int32, "err")):
        if t is not None and (t.dtype != dt or t.device != dev or not t.is_contiguous() or t.numel() < 1):
            raise ValueError(f"kl_gate: {what} must be a contiguous {dt} tensor on the stats' device")
    if not 0 <= int(kl_index) < stats.numel():
        raise ValueError(f"kl_gate: kl_index {kl_index} outside stats [{stats.numel()}]")
    _native.check(_native.load().vn_kl_gate(_p(stats), int(kl_index), float(threshold), _p(err), _p(stop), _p(skip), _p(ran),
                                 _stream(dev)), "vn_kl_gate")


def bc_loss(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear, src: Optional[torch.Tensor],
            labels: torch.Tensor, weight: Optional[torch.Tensor], returns: torch.Tensor, ent_coef: float,
            vf_coef: float):
    """The behaviour-cloning minibatch loss and its gradient
    (csrc/voxnav_bc_loss.hip, the formula in include/voxnav.h vn_bc_loss):
    cross-entropy to the expert's ``labels`` over the samples with
    ``weight``, value MSE and entropy bonus over all of them, in two launches
    (three with weights).

    h [2, M, F]: the (actor, critic) latents; src [M] int64 (or None): the
    samples' rows in the flat rollout buffers ``labels`` (int32), ``weight``
    (uint8, or None: every sample labelled) and ``returns``.  Returns (dh
    [2, M, F], (d action_net.weight, d action_net.bias, d value_net.weight,
    d value_net.bias), stats f64 [6]: cross-entropy, value loss, entropy loss,
    loss, accuracy, labelled share).  Nothing is differentiated here: the
    caller backpropagates dh from h and assigns the head gradients."""
    return _head_loss("bc_loss", h, action_net, value_net, src,
                      ((labels, torch.int32), (weight, torch.uint8), (returns, torch.float32)),
                      "int32 labels / uint8 weights / f32 returns", (float(ent_coef), float(vf_coef)))


def bc_loss_set(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear, src: Optional[torch.Tensor],
                label_set: torch.Tensor, weight: Optional[torch.Tensor], returns: torch.Tensor, ent_coef: float,
                vf_coef: float):
    """``bc_loss`` with a set of equally good actions per sample
    (``vn_bc_loss_set``, include/voxnav.h): ``label_set`` uint8, bit j set
    where action j is optimal (the ``best`` of ``plan_frontier_dists``); the
    cross-entropy is -log of the probability of the whole set, its gradient
    p - softmax restricted to the set; a sample with an empty set is
    unlabelled.  Everything else -- arguments, outputs, stats -- as ``bc_loss``
    (accuracy: the argmax lies in the set).  Three launches."""
    return _head_loss("bc_loss_set", h, action_net, value_net, src,
                      ((label_set, torch.uint8), (weight, torch.uint8), (returns, torch.float32)),
                      "uint8 label sets / uint8 weights / f32 returns", (float(ent_coef), float(vf_coef)))


def _required_masks(name: str, action_masks) -> None:
    """The masked entry points take no absent mask buffer (NULL is refused like any required pointer)."""
    if action_masks is None:
        raise ValueError(f"{name}: action_masks is required (uint8 masks)")


def bc_loss_masked(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear,
                   src: Optional[torch.Tensor], labels: torch.Tensor, weight: Optional[torch.Tensor],
                   action_masks: torch.Tensor, returns: torch.Tensor, ent_coef: float, vf_coef: float):
    """``bc_loss`` with invalid-action masking (csrc/voxnav_masked_bc_loss.hip, the
    rule in include/voxnav.h vn_bc_loss_masked): ``action_masks`` uint8, a flat
    rollout buffer like the others, bit j set where action j was allowed; each
    sample's softmax, entropy and argmax run over its mask with the label (of a
    labelled sample) added, an empty set counting as full, and the logits of
    the other actions get a gradient of exactly 0.  Arguments, outputs and
    stats as ``bc_loss``."""
    _required_masks("bc_loss_masked", action_masks)
    return _head_loss("bc_loss_masked", h, action_net, value_net, src,
                      ((labels, torch.int32), (weight, torch.uint8), (action_masks, torch.uint8),
                       (returns, torch.float32)),
                      "int32 labels / uint8 weights / uint8 masks / f32 returns", (float(ent_coef), float(vf_coef)))


def bc_loss_set_masked(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear,
                       src: Optional[torch.Tensor], label_set: torch.Tensor, weight: Optional[torch.Tensor],
                       action_masks: torch.Tensor, returns: torch.Tensor, ent_coef: float, vf_coef: float):
    """``bc_loss_set`` with invalid-action masking (``vn_bc_loss_set_masked``):
    ``bc_loss_masked`` with the labelled sample's whole set added to its
    allowed actions."""
    _required_masks("bc_loss_set_masked", action_masks)
    return _head_loss("bc_loss_set_masked", h, action_net, value_net, src,
                      ((label_set, torch.uint8), (weight, torch.uint8), (action_masks, torch.uint8),
                       (returns, torch.float32)),
                      "uint8 label sets / uint8 weights / uint8 masks / f32 returns",
                      (float(ent_coef), float(vf_coef)))


def _ppo_bc(name, h, action_net, value_net, src, actions, advantages, old_log_prob, returns, labels, label_dtype,
            weight, clip_range, ent_coef, vf_coef, bc_coef, normalize_advantage, action_masks=None):
    masked = name.endswith("_masked")
    if masked:
        _required_masks(name, action_masks)
    return _head_loss(name, h, action_net, value_net, src,
                      ((actions, torch.int32), (advantages, torch.float32), (old_log_prob, torch.float32),
                       (returns, torch.float32), (labels, label_dtype), (weight, torch.uint8),
                       *(((action_masks, torch.uint8),) if masked else ())),
                      "int32 actions / f32 values / labels / uint8 weights" + (" / uint8 masks" if masked else ""),
                      (float(clip_range), float(ent_coef), float(vf_coef), float(bc_coef),
                       int(bool(normalize_advantage))), adv_words=128, n_stats=9)


def ppo_bc_loss(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear, src: Optional[torch.Tensor],
                actions: torch.Tensor, advantages: torch.Tensor, old_log_prob: torch.Tensor, returns: torch.Tensor,
                labels: torch.Tensor, weight: Optional[torch.Tensor], clip_range: float, ent_coef: float,
                vf_coef: float, bc_coef: float, normalize_advantage: bool):
    """Kickstarted PPO's minibatch loss and its gradient
    (csrc/voxnav_ppo_bc_loss.hip, the formula in include/voxnav.h
    vn_ppo_bc_loss): ``ppo_loss`` + ``bc_coef`` x the cross-entropy of
    ``bc_loss`` to ``labels`` (int32) over the samples with ``weight`` (uint8,
    or None), in one pass over the samples.  Arguments and outputs as
    ``ppo_loss``; stats f64 [9]: its six (the loss with the cross-entropy
    term), then cross-entropy, accuracy, labelled share."""
    return _ppo_bc("ppo_bc_loss", h, action_net, value_net, src, actions, advantages, old_log_prob, returns, labels,
                   torch.int32, weight, clip_range, ent_coef, vf_coef, bc_coef, normalize_advantage)


def ppo_bc_loss_set(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear,
                    src: Optional[torch.Tensor], actions: torch.Tensor, advantages: torch.Tensor,
                    old_log_prob: torch.Tensor, returns: torch.Tensor, label_set: torch.Tensor,
                    weight: Optional[torch.Tensor], clip_range: float, ent_coef: float, vf_coef: float, bc_coef: float,
                    normalize_advantage: bool):
    """``ppo_bc_loss`` with the set-valued cross-entropy of ``bc_loss_set``
    (``vn_ppo_bc_loss_set``): ``label_set`` uint8, a sample with an empty set is
    unlabelled, accuracy counts the argmax lying in the set."""
    return _ppo_bc("ppo_bc_loss_set", h, action_net, value_net, src, actions, advantages, old_log_prob, returns,
                   label_set, torch.uint8, weight, clip_range, ent_coef, vf_coef, bc_coef, normalize_advantage)


def ppo_bc_loss_masked(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear,
                       src: Optional[torch.Tensor], actions: torch.Tensor, advantages: torch.Tensor,
                       old_log_prob: torch.Tensor, returns: torch.Tensor, labels: torch.Tensor,
                       weight: Optional[torch.Tensor], action_masks: torch.Tensor, clip_range: float, ent_coef: float,
                       vf_coef: float, bc_coef: float, normalize_advantage: bool):
    """``ppo_bc_loss`` with invalid-action masking
    (csrc/voxnav_masked_ppo_bc_loss.hip, the rule in include/voxnav.h
    vn_ppo_bc_loss_masked): ``action_masks`` uint8 as ``ppo_loss_masked``'s;
    each sample's softmax, log-prob, entropy and argmax run over its mask with
    the taken action and the label (of a labelled sample) added, an empty set
    counting as full.  Arguments, outputs and stats as ``ppo_bc_loss``."""
    return _ppo_bc("ppo_bc_loss_masked", h, action_net, value_net, src, actions, advantages, old_log_prob, returns,
                   labels, torch.int32, weight, clip_range, ent_coef, vf_coef, bc_coef, normalize_advantage,
                   action_masks)


def ppo_bc_loss_set_masked(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear,
                           src: Optional[torch.Tensor], actions: torch.Tensor, advantages: torch.Tensor,
                           old_log_prob: torch.Tensor, returns: torch.Tensor, label_set: torch.Tensor,
                           weight: Optional[torch.Tensor], action_masks: torch.Tensor, clip_range: float,
                           ent_coef: float, vf_coef: float, bc_coef: float, normalize_advantage: bool):
    """``ppo_bc_loss_set`` with invalid-action masking
    (``vn_ppo_bc_loss_set_masked``): ``ppo_bc_loss_masked`` with the labelled
    sample's whole set added to its allowed actions."""
    return _ppo_bc("ppo_bc_loss_set_masked", h, action_net, value_net, src, actions, advantages, old_log_prob,
                   returns, label_set, torch.uint8, weight, clip_range, ent_coef, vf_coef, bc_coef,
                   normalize_advantage, action_masks)


def _check_tau(name: str, tau) -> float:
    """The soft entries refuse a temperature that is not finite and > 0 before anything is launched."""
    v = float(tau)
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"{name}: tau must be finite and > 0, got {tau!r}")
    return v


def _dists_rows(name: str, dists: torch.Tensor, A: int):
    """``dists`` [rows, ldd] int32 (any leading shape flattened by the caller) -> (tensor, ldd)."""
    if dists is None or dists.dim() != 2 or dists.shape[1] < A:
        raise ValueError(f"{name}: dists must be [rows, ldd >= A = {A}] int32 (the planner's distance through each "
                         "first action)")
    return dists, C.c_int64(int(dists.shape[1]))


def bc_loss_soft(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear, src: Optional[torch.Tensor],
                 dists: torch.Tensor, weight: Optional[torch.Tensor], returns: torch.Tensor, tau: float,
                 ent_coef: float, vf_coef: float):
    """``bc_loss_set`` with a distance-weighted target in place of the set
    (csrc/voxnav_soft_bc_loss.hip, the rule in include/voxnav.h vn_bc_loss_soft):
    ``dists`` int32 [rows, ldd >= A], the planner's distance through each first
    action (``plan_frontier_dists``: positive = path length, -1 unreached, -2 not
    passable), a flat rollout buffer like the others.  The target is
    q_k = w_k / sum w over the actions with a positive distance, w_k = 1 at the
    shortest and exp(-(d_k - d*) / tau) elsewhere; the loss is KL(q || pi), its
    gradient p - q; a sample without a positive distance is unlabelled;
    accuracy: the argmax is among the shortest.  ``tau`` finite and > 0.
    Everything else -- arguments, outputs, stats -- as ``bc_loss``.  Three
    launches."""
    tau = _check_tau("bc_loss_soft", tau)
    dists, ldd = _dists_rows("bc_loss_soft", dists, action_net.out_features)
    return _head_loss("bc_loss_soft", h, action_net, value_net, src,
                      ((dists, torch.int32), (ldd, None), (weight, torch.uint8), (returns, torch.float32)),
                      "int32 distances / uint8 weights / f32 returns", (tau, float(ent_coef), float(vf_coef)))


def bc_loss_soft_masked(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear,
                        src: Optional[torch.Tensor], dists: torch.Tensor, weight: Optional[torch.Tensor],
                        action_masks: torch.Tensor, returns: torch.Tensor, tau: float, ent_coef: float,
                        vf_coef: float):
    """``bc_loss_soft`` with invalid-action masking (``vn_bc_loss_soft_masked``):
    ``bc_loss_masked`` with every action of a labelled sample that has a
    positive distance added to its allowed actions."""
    _required_masks("bc_loss_soft_masked", action_masks)
    tau = _check_tau("bc_loss_soft_masked", tau)
    dists, ldd = _dists_rows("bc_loss_soft_masked", dists, action_net.out_features)
    return _head_loss("bc_loss_soft_masked", h, action_net, value_net, src,
                      ((dists, torch.int32), (ldd, None), (weight, torch.uint8), (action_masks, torch.uint8),
                       (returns, torch.float32)),
                      "int32 distances / uint8 weights / uint8 masks / f32 returns",
                      (tau, float(ent_coef), float(vf_coef)))


def _ppo_bc_soft(name, h, action_net, value_net, src, actions, advantages, old_log_prob, returns, dists, weight,
                 clip_range, ent_coef, vf_coef, bc_coef, tau, normalize_advantage, action_masks=None):
    masked = name.endswith("_masked")
    if masked:
        _required_masks(name, action_masks)
    tau = _check_tau(name, tau)
    dists, ldd = _dists_rows(name, dists, action_net.out_features)
    return _head_loss(name, h, action_net, value_net, src,
                      ((actions, torch.int32), (advantages, torch.float32), (old_log_prob, torch.float32),
                       (returns, torch.float32), (dists, torch.int32), (ldd, None), (weight, torch.uint8),
                       *(((action_masks, torch.uint8),) if masked else ())),
                      "int32 actions / f32 values / int32 distances / uint8 weights" +
                      (" / uint8 masks" if masked else ""),
                      (float(clip_range), float(ent_coef), float(vf_coef), float(bc_coef), tau,
                       int(bool(normalize_advantage))), adv_words=128, n_stats=9)


def ppo_bc_loss_soft(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear,
                     src: Optional[torch.Tensor], actions: torch.Tensor, advantages: torch.Tensor,
                     old_log_prob: torch.Tensor, returns: torch.Tensor, dists: torch.Tensor,
                     weight: Optional[torch.Tensor], clip_range: float, ent_coef: float, vf_coef: float,
                     bc_coef: float, tau: float, normalize_advantage: bool):
    """``ppo_bc_loss`` with the distance-weighted KL of ``bc_loss_soft`` in the
    cross-entropy's place (csrc/voxnav_soft_ppo_bc_loss.hip,
    ``vn_ppo_bc_loss_soft``): ``dists`` int32 [rows, ldd >= A]; a sample without
    a positive distance is unlabelled, accuracy counts the argmax among the
    shortest actions."""
    return _ppo_bc_soft("ppo_bc_loss_soft", h, action_net, value_net, src, actions, advantages, old_log_prob, returns,
                        dists, weight, clip_range, ent_coef, vf_coef, bc_coef, tau, normalize_advantage)


def ppo_bc_loss_soft_masked(h: torch.Tensor, action_net: torch.nn.Linear, value_net: torch.nn.Linear,
                            src: Optional[torch.Tensor], actions: torch.Tensor, advantages: torch.Tensor,
                            old_log_prob: torch.Tensor, returns: torch.Tensor, dists: torch.Tensor,
                            weight: Optional[torch.Tensor], action_masks: torch.Tensor, clip_range: float,
                            ent_coef: float, vf_coef: float, bc_coef: float, tau: float, normalize_advantage: bool):
    """``ppo_bc_loss_soft`` with invalid-action masking
    (``vn_ppo_bc_loss_soft_masked``): ``ppo_bc_loss_masked`` with every action of
    a labelled sample that has a positive distance added to its allowed
    actions."""
    return _ppo_bc_soft("ppo_bc_loss_soft_masked", h, action_net, value_net, src, actions, advantages, old_log_prob,
                        returns, dists, weight, clip_range, ent_coef, vf_coef, bc_coef, tau, normalize_advantage,
                        action_masks)


def grad_norm_scale(params, max_norm: float, work: Optional[torch.Tensor] = None):
    """The total 2-norm of the parameters' gradients and the divisor that
    clips them to ``max_norm`` (csrc/voxnav_ppo_loss.hip vn_grad_norm): two
    launches, device scalars (norm, scale) -- handed to the fused Adam step as
    its grad_scale instead of rescaling every gradient in place
    (torch.nn.utils.clip_grad_norm_'s update, folded into the step)."""
    lib = _native.load()
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:
        raise ValueError("grad_norm_scale: no gradients")
    dev = grads[0].device
    grads = [g for g in grads if g.numel()]      # an empty tensor has no address to pass and adds nothing
    if not grads:
        return torch.zeros((), dtype=torch.float32, device=dev), torch.ones((), dtype=torch.float32, device=dev)
    for g in grads:
        if g.dtype != torch.float32 or not g.is_contiguous() or g.device != dev:
            raise ValueError("grad_norm_scale: gradients must be contiguous f32 on one device")
    n = len(grads)
    ptrs = (C.c_void_p * n)(*[g.data_ptr() for g in grads])
    sizes = (C.c_int64 * n)(*[g.numel() for g in grads])
    out = torch.empty(2, dtype=torch.float32, device=dev)
    work = torch.empty(256, dtype=torch.float64, device=dev) if work is None else work
    _native.check(lib.vn_grad_norm(ptrs, sizes, n, float(max_norm), _p(out[0:1]), _p(out[1:2]), _p(work),
                                   _stream(dev)), "vn_grad_norm")
    return out[0], out[1]


def adam_step(optimizer: torch.optim.Adam, clip_scale: Optional[torch.Tensor] = None,
              skip: Optional[torch.Tensor] = None) -> None:
    """``optimizer.step()`` for a single-group ``torch.optim.Adam`` (no
    amsgrad / weight decay / maximize) on the library's kernel
    (csrc/voxnav_ppo_loss.hip vn_adam_step): one launch over every parameter,
    the gradients divided by ``clip_scale`` (``grad_norm_scale``'s divisor) on
    the way.  The optimizer's own state tensors are updated in place
    (``exp_avg``, ``exp_avg_sq``, ``step``), so ``state_dict()`` / checkpoints
    are torch's.  ``skip``: a device int32 word; when it is nonzero at run
    time the step changes nothing (the row-layout LSTM's error word: the
    gradients of a timed-out launch are never applied) -- parameters, moments
    and ``step`` stay as they were, and the next applied step is numbered from
    the device counters (the host's count below may run ahead of them after a
    skipped step; the kernel then forms the bias corrections itself)."""
    lib = _native.load()
    if len(optimizer.param_groups) != 1:
        raise ValueError("adam_step: one parameter group")
    grp = optimizer.param_groups[0]
    if grp.get("amsgrad") or grp.get("weight_decay") or grp.get("maximize"):
        raise ValueError("adam_step: plain Adam only (no amsgrad, weight decay or maximize)")
    params = [p for p in grp["params"] if p.grad is not None]
    if not params:
        return
    dev = params[0].device
    steps = []
    for p in params:
        st = optimizer.state[p]
        if not st:
            st["step"] = torch.zeros((), dtype=torch.float32, device=dev)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        if skip is not None and (st["step"].device != dev or st["step"].dtype != torch.float32):
            # a gated step: the counter must live on the device, where the kernel
            # advances it only when the step is applied
            st["step"] = st["step"].to(device=dev, dtype=torch.float32)
        steps.append(st["step"])
        for t in (p, p.grad, st["exp_avg"], st["exp_avg_sq"]):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                raise ValueError("adam_step: contiguous f32 parameters, gradients and moments on one device")
    # the step count, kept on the host (read back once after a fresh state or a
    # load_state_dict); for a gated step it is the count of attempts: the
    # launch checks it against the device counters, which count applied steps
    cache = getattr(optimizer, "_vn_adam_t", None)
    if cache is None or cache[0] is not steps[0]:
        t = int(round(float(steps[0].item())))
    else:
        t = cache[1]
    t += 1
    optimizer._vn_adam_t = (steps[0], t)
    n = len(params)
    arr = lambda ts: (C.c_void_p * n)(*[x.data_ptr() for x in ts])  # noqa: E731
    st_ptrs = [s if (s.device == dev and s.dtype == torch.float32) else None for s in steps]
    steps_arr = (C.c_void_p * n)(*[(x.data_ptr() if x is not None else None) for x in st_ptrs])
    sizes = (C.c_int64 * n)(*[p.numel() for p in params])
    b1, b2 = grp["betas"]
    _native.check(lib.vn_adam_step(arr(params), arr([p.grad for p in params]),
                                   arr([optimizer.state[p]["exp_avg"] for p in params]),
                                   arr([optimizer.state[p]["exp_avg_sq"] for p in params]), steps_arr, sizes, n,
                                   _p(clip_scale), _p(skip), float(grp["lr"]), float(b1), float(b2), float(grp["eps"]), t,
                                   _stream(dev)), "vn_adam_step")
    for s, x in zip(steps, st_ptrs):
        if x is None:                       # a CPU / other-dtype step counter (a loaded state): set on the host
            s.fill_(float(t))


def minibatch_rows(idx: torch.Tensor, T: int, N: int, obs: torch.Tensor):
    """(src, obs rows) of a feed-forward PPO minibatch in one launch
    (vn_minibatch_rows): idx [M] env-major flat ids (int64), obs [T, N, D]
    -> src [M] int64 rows of the [T, N]-major buffers, [M, D] observations."""
    lib = _native.load()
    M = idx.numel()
    D = obs.shape[-1]
    dev = idx.device
    if idx.dtype != torch.int64 or not idx.is_contiguous() or not obs.is_contiguous() or obs.dtype != torch.float32:
        raise ValueError("minibatch_rows: contiguous int64 ids and f32 observations")
    out = torch.empty((M, D), dtype=torch.float32, device=dev)
    src = torch.empty(M, dtype=torch.int64, device=dev)
    _native.check(lib.vn_minibatch_rows(_p(idx), M, T, N, _p(obs), D, _p(out), _p(src), _stream(dev)),
                  "vn_minibatch_rows")
    return src, out
