"""DAgger warm start: the frontier planner teaches the policy.

The frontier planner (``voxnav.planner``, ``vn_plan_frontier``) finishes every
evaluate episode without a bump; this module lets a policy learn from it
before (or instead of) PPO, by dataset aggregation (Ross, Gordon & Bagnell,
"A Reduction of Imitation Learning and Structured Prediction to No-Regret
Online Learning", AISTATS 2011):

* ``DaggerCollector``: a ``RolloutCollector`` whose policy runs in the loop --
  so the LSTM states, values and returns of the buffer are the policy's own --
  while the planner labels every visited state.  The executed action is the
  planner's with probability ``beta``, else the policy's sample
  (``vn_dagger_mix``, one launch per step, nothing crosses to the host).
* ``BCLearner``: a ``PPOLearner`` whose loss is the cross-entropy to the
  labels (+ the value MSE and the entropy bonus), through the fused kernel
  ``learn_ops.bc_loss`` (csrc/voxnav_bc_loss.hip) on the GPU and torch
  autograd elsewhere.  Minibatches, the LSTM re-run from the stored states,
  the all-reduce, the clip and the Adam step are the parent's.
* ``warm_start``: ``ppo.learn``'s loop over the two, with a beta schedule.
* ``KickstartLearner`` / ``kickstart``: PPO on the policy's own rollouts
  (beta = 0) with the cross-entropy to the planner's labels added under a
  coefficient that the loop lets decay to 0 (Schmitt et al., "Kickstarting
  Deep Reinforcement Learning", 2018), through the fused
  kernel ``learn_ops.ppo_bc_loss`` (csrc/voxnav_ppo_bc_loss.hip).
* ``MaskedDaggerCollector`` / ``MaskedDaggerBuffer`` and the two learners'
  ``action_masks=True``: the same with invalid-action masking (DESIGN.md
  10.9).  The collector samples from the allowed actions only, so a rollout
  never bumps at any beta; the learners' softmax runs over each sample's mask
  with the label (and, under PPO, the taken action) added -- the planner never
  labels an action the mask forbids, so the label is always in the support.

* ``labels="soft"`` / ``execute="best"``: the two consumers
  of the planner's per-action distances.  The learners' target becomes the
  distance-weighted distribution of include/voxnav.h vn_bc_loss_soft (a
  temperature ``label_tau``; the loss is KL(q || pi)), through
  ``learn_ops.bc_loss_soft`` / ``ppo_bc_loss_soft`` and their masked forms; the
  collectors execute the policy's own sample whenever it is among the shortest
  actions (``vn_dagger_mix_best``), so the rollouts stay on the paths the
  policy itself prefers.

The policy module is the one ``PPOLearner``, ``save_checkpoint`` and
``evaluate_policy`` take: a warm start followed by ``ppo.learn`` needs no
conversion.  CubicEnv variant only, rooms within the planner's 64 x 64 bound.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Union

import numpy as np
import torch
import torch.nn.functional as Fn

from . import _native, learn_ops
from .collector import MaskedRolloutBuffer, RolloutBuffer, RolloutCollector, _p
from .env import BatchedGridEnv, FrontierDists
from .planner import FrontierExplorer
from .ppo import PPOLearner, run_loop

PLANNER_MAX_PAD = 64     # vn_plan_frontier's bound on the padded width and depth


@dataclass
class DaggerBuffer(RolloutBuffer):
    """A ``RolloutBuffer`` plus the planner's labels, all [T, N] on the GPU.

    ``actions`` are the executed actions (what the env stepped with and what
    obs / rewards / returns follow from).  ``log_probs`` are the log-probs of
    the policy's own sample ``policy_actions``, not of the executed action:
    with beta > 0 this is NOT a PPO buffer (the importance ratio of
    ``PPOLearner`` would pair an action with another action's old log-prob).
    With beta = 0 the executed action is the policy's sample everywhere and
    the ``RolloutBuffer`` fields equal a plain ``RolloutCollector``'s.

    ``expert_actions`` / ``expert_dist``: the planner's action and distance
    for the state each step acted on (dist = -1: its fallback, no target in
    reach); ``label_weight``: 1 where dist != -1 (the sample is labelled);
    ``took_expert``: 1 where the planner's action was executed;
    ``policy_actions``: the policy's sample.

    A collector with ``labels="set"`` also fills ``expert_dists`` ([T, N, 6]
    int32: the planner's distance through each first action, -1 unreached, -2
    not passable) and ``expert_set`` ([T, N] uint8: bit k set where action k
    is among the shortest; 0 where dist = -1); both are None otherwise
    (``labels="soft"`` fills the same two).  A collector with
    ``execute="best"`` fills ``own_best`` ([T, N] uint8: 1 where the policy's own
    sample was among the shortest actions of a labelled state); None otherwise."""
    expert_actions: Optional[torch.Tensor] = None
    expert_dist: Optional[torch.Tensor] = None
    label_weight: Optional[torch.Tensor] = None
    took_expert: Optional[torch.Tensor] = None
    policy_actions: Optional[torch.Tensor] = None
    expert_dists: Optional[torch.Tensor] = None
    expert_set: Optional[torch.Tensor] = None
    own_best: Optional[torch.Tensor] = None


@dataclass
class MaskedDaggerBuffer(DaggerBuffer, MaskedRolloutBuffer):
    """A ``DaggerBuffer`` of a ``MaskedDaggerCollector``: ``action_masks`` uint8
    [T, N] as ``MaskedRolloutBuffer``'s.  ``actions``, ``policy_actions``, every
    labelled ``expert_actions`` and ``expert_set`` lie inside the masks.  Taken
    wherever a ``MaskedRolloutBuffer`` or a ``DaggerBuffer`` is."""


def _check_labels(labels) -> str:
    if labels not in ("action", "set", "soft"):
        raise ValueError(f"labels must be 'action', 'set' or 'soft', got {labels!r}")
    return labels


def _check_execute(execute, labels: str) -> str:
    if execute not in ("expert", "best"):
        raise ValueError(f"execute must be 'expert' or 'best', got {execute!r}")
    if execute == "best" and labels == "action":
        raise ValueError("execute='best' needs labels='set' or 'soft': with labels='action' the planner is not "
                         "asked for the set of shortest actions")
    return execute


def _check_tau(tau) -> float:
    v = float(tau)
    if not (np.isfinite(v) and v > 0.0):
        raise ValueError(f"label_tau must be finite and > 0, got {tau!r}")
    return v


def _check_beta(beta) -> float:
    b = float(beta)
    if not 0.0 <= b <= 1.0:
        raise ValueError(f"beta must be in [0, 1], got {beta!r}")
    return b


def _buffer_labels(buf, labels: str, who: str):
    """The flat labels (``expert_set``, ``expert_actions``, or the rows of ``expert_dists``) and
    label weights (or None) of a buffer for learner ``who``; raises where the buffer does not
    carry them."""
    if labels == "soft":
        lab = getattr(buf, "expert_dists", None)
        if lab is None:
            raise ValueError(f"{who}(labels='soft') needs the buffer's expert_dists (a DaggerCollector with "
                             "labels='soft' or 'set')")
        w = getattr(buf, "label_weight", None)
        return lab.reshape(-1, lab.shape[-1]), (None if w is None else w.reshape(-1))
    if labels == "set":
        lab = getattr(buf, "expert_set", None)
        if lab is None:
            raise ValueError(f"{who}(labels='set') needs the buffer's expert_set (a DaggerCollector with "
                             "labels='set')")
    else:
        lab = getattr(buf, "expert_actions", None)
        if lab is None:
            raise ValueError(f"{who} needs the buffer's expert_actions (a DaggerBuffer)")
    w = getattr(buf, "label_weight", None)
    return lab.reshape(-1), (None if w is None else w.reshape(-1))


class DaggerCollector(RolloutCollector):
    """``collect()`` fills a ``DaggerBuffer``: the policy acts in the loop, the
    planner ``expert`` labels every step, and the env executes the planner's
    action with probability ``beta`` (where the planner found a target), else
    the policy's sample.

    The draw is the sampler's Philox word under the key ``mix_seed`` with the
    counter (global agent id, global step): like the Categorical draw, it does
    not depend on how the agents are sharded over envs.

    ``labels="set"``: the planner is asked for the distance through every
    first action (one ``plan_frontier_dists`` call per step in place of
    ``plan_frontier``) and the buffer carries ``expert_dists`` and
    ``expert_set`` as well.  The executed action does not change: the
    planner's lowest-k action with probability ``beta``.  ``labels="soft"``
    is the same planner call and the same buffers (the learners read
    ``expert_dists`` in place of ``expert_set``).

    ``execute="best"`` (with ``labels="set"`` or ``"soft"``): the planner's
    action is executed only where the policy's own sample is not among the
    shortest actions (``vn_dagger_mix_best``, the same draw, one launch), and
    the buffer carries ``own_best``.  At beta = 1 the agent still walks a
    shortest path, but the policy breaks the ties, not the index rule.
    ``execute="expert"`` (the default) is ``vn_dagger_mix``."""

    _masked = False      # MaskedDaggerCollector: the parent collector's masked path

    def __init__(self, env: BatchedGridEnv, policy, *args, expert: Optional[FrontierExplorer] = None,
                 beta: float = 1.0, mix_seed: int = 4242, labels: str = "action", execute: str = "expert",
                 **kwargs):
        if env.variant != _native.VN_VARIANT_CUBIC:
            raise ValueError("DaggerCollector: the frontier planner needs the CubicEnv variant")
        if kwargs.pop("action_masks", False):
            raise ValueError("DaggerCollector takes no action_masks: masked DAgger / kickstart is "
                             "MaskedDaggerCollector")
        info = env.info
        if info.pad_w > PLANNER_MAX_PAD or info.pad_d > PLANNER_MAX_PAD:
            raise ValueError(f"DaggerCollector: the frontier planner takes padded rooms of at most {PLANNER_MAX_PAD} x "
                             f"{PLANNER_MAX_PAD} (this env: {info.pad_w} x {info.pad_d})")
        self.expert = expert if expert is not None else FrontierExplorer()
        self.beta = _check_beta(beta)
        self.mix_seed = int(mix_seed)
        self.labels = _check_labels(labels)
        self.execute = _check_execute(execute, self.labels)
        super().__init__(env, policy, *args, action_masks=self._masked, **kwargs)
        T, N, dev = self.n_steps, self.N, self.device
        self.expert_actions = torch.zeros((T, N), dtype=torch.int32, device=dev)
        self.expert_dist = torch.full((T, N), -1, dtype=torch.int32, device=dev)
        self.policy_actions = torch.zeros((T, N), dtype=torch.int32, device=dev)
        self.label_weight = torch.zeros((T, N), dtype=torch.uint8, device=dev)
        self.took_expert = torch.zeros((T, N), dtype=torch.uint8, device=dev)
        self.expert_dists = self.expert_set = self.own_best = None
        if self.labels != "action":
            self.expert_dists = torch.full((T, N, 6), -2, dtype=torch.int32, device=dev)
            self.expert_set = torch.zeros((T, N), dtype=torch.uint8, device=dev)
        if self.execute == "best":
            self.own_best = torch.zeros((T, N), dtype=torch.uint8, device=dev)

    def set_beta(self, beta: float) -> None:
        """The probability of executing the planner's action, from the next ``collect()`` on."""
        self.beta = _check_beta(beta)

    def _choose_actions(self, t: int) -> None:
        self.policy_actions[t].copy_(self.actions[t])
        if self.labels != "action":
            self.expert.act_dists(self.env, out=FrontierDists(self.expert_actions[t], self.expert_dist[t],
                                                              self.expert_dists[t], self.expert_set[t]))
        else:
            _, dist = self.expert.act(self.env, out=self.expert_actions[t], return_dist=True)
            self.expert_dist[t].copy_(dist)
        if self.execute == "best":
            _native.check(self.lib.vn_dagger_mix_best(_p(self.policy_actions[t]), _p(self.expert_actions[t]),
                                                      _p(self.expert_dist[t]), _p(self.expert_set[t]), self.N,
                                                      C.c_double(self.beta), C.c_uint64(self.mix_seed & (2 ** 64 - 1)),
                                                      C.c_uint64(self.t_global), self.env.agent_id_base,
                                                      _p(self.actions[t]), _p(self.took_expert[t]),
                                                      _p(self.label_weight[t]), _p(self.own_best[t]), self._stream()),
                          "vn_dagger_mix_best")
            return
        _native.check(self.lib.vn_dagger_mix(_p(self.policy_actions[t]), _p(self.expert_actions[t]),
                                             _p(self.expert_dist[t]), self.N, C.c_double(self.beta),
                                             C.c_uint64(self.mix_seed & (2 ** 64 - 1)), C.c_uint64(self.t_global),
                                             self.env.agent_id_base, _p(self.actions[t]), _p(self.took_expert[t]),
                                             _p(self.label_weight[t]), self._stream()), "vn_dagger_mix")

    @torch.no_grad()
    def collect(self) -> DaggerBuffer:
        """One rollout of n_steps.  The returned buffer views the collector's
        storage: it stays valid until the next ``collect()``."""
        rb = super().collect()
        cls = MaskedDaggerBuffer if self._masked else DaggerBuffer     # (rb carries action_masks when masked)
        return cls(**{k: getattr(rb, k) for k in rb.__dataclass_fields__},
                   expert_actions=self.expert_actions, expert_dist=self.expert_dist,
                   label_weight=self.label_weight, took_expert=self.took_expert,
                   policy_actions=self.policy_actions, expert_dists=self.expert_dists,
                   expert_set=self.expert_set, own_best=self.own_best)


class MaskedDaggerCollector(DaggerCollector):
    """A ``DaggerCollector`` with invalid-action masking: the
    parent ``RolloutCollector``'s masked path -- per step ``vn_action_mask`` on
    the observation into row t of the [T, N] mask buffer, the layer kernels and
    ``vn_policy_head_masked`` -- then the unchanged planner labels and
    ``vn_dagger_mix``.  The planner's action is always inside the mask (both
    read an in-bounds neighbour with belief >= 0), so no executed action bumps
    at any ``beta``.  ``collect()`` returns a ``MaskedDaggerBuffer``; ``act()``
    and ``set_beta`` are as inherited.  Takes no ``action_masks`` keyword; f32
    collectors on a CubicEnv only, rooms within the planner's bound."""

    _masked = True

    def __init__(self, env: BatchedGridEnv, policy, *args, **kwargs):
        if "action_masks" in kwargs:
            raise TypeError("MaskedDaggerCollector takes no action_masks keyword (it always masks)")
        super().__init__(env, policy, *args, **kwargs)


def _allowed(masks: torch.Tensor, A: int, always: torch.Tensor) -> torch.Tensor:
    """S [M, A] bool: the mask's bits below A with ``always`` (the label's bits of a labelled
    sample, the taken action) added; an empty row counts as full (include/voxnav.h
    vn_bc_loss_masked)."""
    ar = torch.arange(A, device=masks.device)
    S = ((masks.view(-1, 1).to(torch.int64) >> ar) & 1).bool() | always
    return S | ~S.any(-1, keepdim=True)


def _cross_entropy(logits: torch.Tensor, labels: torch.Tensor, w: torch.Tensor, sets: bool,
                   masks: Optional[torch.Tensor] = None, taken: Optional[torch.Tensor] = None,
                   tau: Optional[float] = None):
    """The torch path's cross-entropy of both learners, on the minibatch's rows.  ``labels``: the
    expert's actions, or (``sets``) their uint8 sets; ``w`` [M]: 1 where the weight labels the
    sample; ``masks`` (uint8 [M], or None): the softmax runs over S = mask | label bits of a
    labelled sample | ``taken`` (the executed actions, int64, under PPO), an empty S as full.
    -> (logits with -inf outside S, log_softmax with zeros outside S, the label's (the set's)
    log-probability [M], w with empty sets dropped, right_of(argmax) -> the argmax is the label's).
    ``tau`` (labels="soft"): ``labels`` are the planner's distance rows [M, >= A] and the target is
    the distance-weighted q of include/voxnav.h vn_bc_loss_soft; the third value is then -KL(q || pi),
    the label bits are the actions with a positive distance, and the argmax is right where its
    distance is the shortest."""
    A = logits.shape[-1]
    ar = torch.arange(A, device=logits.device)
    soft = tau is not None
    if soft:
        # in_set [M, A]: P, the actions with a positive distance; q = w / sum w, w = 1 at the
        # shortest distance and exp(-delta / tau) elsewhere in P; ln q = -delta / tau - ln sum w
        d = labels[:, :A].long()
        in_set = d > 0
        some = in_set.any(-1)
        w = w * some.to(w.dtype)
        dmin = torch.where(in_set, d, torch.full_like(d, 2 ** 62)).min(-1, keepdim=True).values
        delta = torch.where(in_set, d - dmin, torch.zeros_like(d))
        e = -delta.to(logits.dtype) / tau
        wk = torch.where(in_set, torch.where(delta == 0, torch.ones_like(e), torch.exp(e)), torch.zeros_like(e))
        sw = torch.where(some, wk.sum(-1), torch.ones_like(wk[:, 0])).view(-1, 1)
        q = wk / sw
        ln_q = torch.where(q > 0, e - torch.log(sw), torch.zeros_like(e))     # (a term whose q is 0 is 0)
        shortest = in_set & (delta == 0)
    elif sets:
        # in_set [M, A]: bit j of the sample's set; -log sum_{j in set} p_j = lse(z) - lse(z over the set)
        in_set = ((labels.long().view(-1, 1) >> ar) & 1).bool()
        some = in_set.any(-1)
        w = w * some.to(w.dtype)
    else:
        lab = labels.long()
    S = None
    if masks is not None:
        always = (in_set if sets or soft else ar.view(1, A) == lab.view(-1, 1)) & (w != 0).view(-1, 1)
        if taken is not None:
            always = always | (ar.view(1, A) == taken.view(-1, 1))
        S = _allowed(masks, A, always)
        logits = logits.masked_fill(~S, float("-inf"))
    lp_all = torch.log_softmax(logits, dim=-1)
    if S is not None:
        # a masked action's terms are zeros (exp(0) 0 in the entropy), and it gets no gradient
        lp_all = torch.where(S, lp_all, lp_all.new_zeros(()))
    if soft:
        kl = torch.where(q > 0, q * (ln_q - lp_all), torch.zeros_like(q)).sum(-1)
        return logits, lp_all, -kl, w, lambda amax: shortest.gather(1, amax.view(-1, 1)).flatten()
    if sets:
        sel = in_set if S is None else in_set & S          # (a labelled sample's set lies in S)
        masked = logits.masked_fill(~sel, float("-inf"))
        masked = torch.where(sel.any(-1, keepdim=True), masked, torch.zeros_like(masked))   # (empty: no -inf row)
        lp = torch.logsumexp(masked, dim=-1) - torch.logsumexp(logits, dim=-1)
        return logits, lp_all, lp, w, lambda amax: in_set.gather(1, amax.view(-1, 1)).flatten()
    lp = lp_all.gather(1, lab.view(-1, 1)).flatten()
    return logits, lp_all, lp, w, lambda amax: amax == lab


class _PlannerLabels:
    """What the two learners share about their labels: the label mode's buffer fields, and the
    temperature of ``labels="soft"`` with its schedule."""

    def _init_label_tau(self, label_tau) -> None:
        # a float, or a callable of the remaining progress like the parent's schedules
        # (set_progress; until its first call it holds its value at 1)
        self._label_tau_fn = label_tau if callable(label_tau) else None
        self.label_tau = _check_tau(label_tau(1.0) if callable(label_tau) else label_tau)

    def set_progress(self, progress_remaining: float) -> None:
        """``PPOLearner.set_progress`` plus a callable ``label_tau``."""
        super().set_progress(progress_remaining)
        if self._label_tau_fn is not None:
            self.label_tau = _check_tau(self._label_tau_fn(float(progress_remaining)))

    def _tau(self) -> Optional[float]:
        return self.label_tau if self.labels == "soft" else None

    def _labels(self, buf):
        who = type(self).__name__
        lab, w = _buffer_labels(buf, self.labels, who)
        if self.labels == "soft" and self.policy.action_net.out_features != lab.shape[-1]:
            raise ValueError(f"{who}(labels='soft'): the policy has {self.policy.action_net.out_features} actions, "
                             f"expert_dists has {lab.shape[-1]} columns (the planner's first actions)")
        return lab, w


class BCLearner(_PlannerLabels, PPOLearner):
    """Behaviour cloning on a ``DaggerBuffer``: per minibatch
        loss = CE(labelled samples) + ent_coef * (-mean H) + vf_coef * MSE(returns, values)
    (the formula of include/voxnav.h vn_bc_loss), with the parent's
    minibatch order, LSTM re-run, all-reduce, grad-norm clip and Adam step.
    ``clip_range`` and ``normalize_advantage`` are unused.  With a process
    group the ranks' gradients are averaged equally, although their labelled
    counts may differ.

    ``labels="set"``: the labels are the buffer's ``expert_set`` (a
    ``DaggerCollector(labels="set")``), the cross-entropy is -log of the
    probability of the whole set of equally short actions (the formula of
    vn_bc_loss_set, through ``learn_ops.bc_loss_set`` on the GPU), a sample
    with an empty set is unlabelled, and ``accuracy`` counts the argmax lying
    in the set.

    ``action_masks=True`` trains on a ``MaskedDaggerBuffer``: every sample's
    softmax, entropy and argmax run over S = its mask with the label's bits
    (of a labelled sample) added, an empty set counting as full (the rule of
    vn_bc_loss_masked), in ``learn_ops.bc_loss_masked`` / ``bc_loss_set_masked``
    where the fused loss runs, else through torch autograd of the same formula
    (``PPOLearner._heads``' masked_fill / log_softmax / where).

    ``labels="soft"``: the labels are the buffer's ``expert_dists`` (a
    ``DaggerCollector(labels="soft")`` or ``"set"``), the target is the
    distance-weighted distribution of vn_bc_loss_soft at the temperature
    ``label_tau`` (a float, or a callable of the remaining progress evaluated
    by ``set_progress`` like the parent's schedules), ``bc_loss`` is
    KL(target || policy), and ``accuracy`` counts the argmax among the shortest
    actions; through ``learn_ops.bc_loss_soft`` / ``bc_loss_soft_masked`` where
    the fused loss runs.  The policy must have the planner's 6 actions."""

    def __init__(self, policy, learning_rate: float = 3e-4, n_epochs: int = 10, batch_size: int = 64,
                 ent_coef: float = 0.0, vf_coef: float = 0.5, max_grad_norm: float = 0.5, seed: int = 0,
                 process_group=None, labels: str = "action", action_masks: bool = False, target_kl=None,
                 clip_range_vf=None, label_tau: Union[float, Callable[[float], float]] = 1.0):
        if target_kl is not None or clip_range_vf is not None:
            raise ValueError("BCLearner takes no target_kl or clip_range_vf: its loss has no importance ratio "
                             "(its fifth logged value is the accuracy) and no clipped value term")
        super().__init__(policy, learning_rate=learning_rate, n_epochs=n_epochs, batch_size=batch_size,
                         ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm, seed=seed,
                         process_group=process_group, action_masks=action_masks)
        # minibatches that went through learn_ops.bc_loss / bc_loss_set or, counted in
        # masked_fused_updates as well, their masked forms
        self.fused_updates = 0
        self.labels = _check_labels(labels)
        self._init_label_tau(label_tau)

    def update(self, buf, idx: torch.Tensor, packed: Optional[dict] = None) -> torch.Tensor:
        """One minibatch (env-major flat ids ``idx``): loss, backward,
        (all-reduce), clip, Adam.  Returns the logged values as a device
        tensor: cross-entropy, value loss, entropy loss, loss, accuracy,
        labelled share, grad norm."""
        self._check_masks(buf)
        if self.recurrent:
            (lat_pi, lat_vf, lat_pair), src = self._evaluate_recurrent(buf, packed or self._pack_begin(buf, idx))
        else:
            (lat_pi, lat_vf, lat_pair), src = self._evaluate_ff(buf, idx)
        labels, weight = self._labels(buf)
        pol = self.policy
        ex = pol.mlp_extractor
        if lat_pi.is_cuda:
            F = ex.latent_dim_pi
            if F == ex.latent_dim_vf and learn_ops.ppo_loss_supported(pol.action_net, pol.value_net, F):
                h = learn_ops.mlp_pair(ex.policy_net, ex.value_net, lat_pi, None if lat_vf is lat_pi else lat_vf,
                                       x_pair=lat_pair, stacked=True)
                if h is not None:
                    return self._update_fused_bc(buf, h, src, labels, weight)
        # torch's ops and autograd: the CPU path, and heads the fused kernel does not take
        h_pi, h_vf = learn_ops.mlp_pair(ex.policy_net, ex.value_net, lat_pi, None if lat_vf is lat_pi else lat_vf,
                                        x_pair=lat_pair)
        logits = learn_ops.linear(h_pi, pol.action_net)
        values = learn_ops.linear(h_vf, pol.value_net).flatten()
        A = logits.shape[-1]
        w = torch.ones_like(values) if weight is None else (weight[src] != 0).to(values.dtype)
        ret = buf.returns.reshape(-1)[src]
        masks = buf.action_masks.reshape(-1)[src] if self.action_masks else None
        logits, lp_all, lp, w, right_of = _cross_entropy(logits, labels[src], w, self.labels == "set", masks,
                                                         tau=self._tau())
        entropy = -(lp_all.exp() * lp_all).sum(-1)
        n = w.sum()
        den = torch.clamp(n, min=1.0)
        bc = (w * -lp).sum() / den
        value_loss = ((ret - values) ** 2).mean()
        entropy_loss = -entropy.mean()
        loss = bc + self.ent_coef * entropy_loss + self.vf_coef * value_loss
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        if self.group is not None:
            self._allreduce_grads()
        gnorm = self._clip_step()
        with torch.no_grad():
            top = logits.max(-1, keepdim=True).values
            ar = torch.arange(A, device=logits.device).expand_as(logits)
            amax = torch.where(logits == top, ar, torch.full_like(ar, A)).min(-1).values   # ties: the lowest index
            # counts are integers: their quotients in f64, as the kernel's
            acc = (w.double() * right_of(amax).double()).sum() / den.double()
            return torch.stack([bc.detach().double(), value_loss.detach().double(), entropy_loss.detach().double(),
                                loss.detach().double(), acc, n.double() / w.numel(), gnorm.detach().double()])

    def _update_fused_bc(self, buf, h: torch.Tensor, src: torch.Tensor, labels: torch.Tensor,
                         weight: Optional[torch.Tensor]) -> torch.Tensor:
        """``update`` from the MLP latents h [2, M, F] on: the heads, the loss
        and its gradient in the fused kernel (learn_ops.bc_loss / bc_loss_set),
        then ``PPOLearner._step_fused``."""
        pol = self.policy
        coefs = ((self.label_tau,) if self.labels == "soft" else ()) + (self.ent_coef, self.vf_coef)
        if self.action_masks:
            fused = {"set": learn_ops.bc_loss_set_masked, "soft": learn_ops.bc_loss_soft_masked,
                     "action": learn_ops.bc_loss_masked}[self.labels]
            dh, grads, stats = fused(h, pol.action_net, pol.value_net, src, labels, weight,
                                     buf.action_masks.reshape(-1), buf.returns.reshape(-1), *coefs)
            self.masked_fused_updates += 1
        else:
            fused = {"set": learn_ops.bc_loss_set, "soft": learn_ops.bc_loss_soft,
                     "action": learn_ops.bc_loss}[self.labels]
            dh, grads, stats = fused(h, pol.action_net, pol.value_net, src, labels, weight, buf.returns.reshape(-1),
                                     *coefs)
        self.fused_updates += 1
        return self._step_fused(h, dh, grads, stats)

    def train(self, buf, epoch_orders: Optional[Sequence] = None) -> Dict[str, float]:
        """One ``train()`` over a ``DaggerBuffer`` (n_epochs passes).  Returns
        the means over the minibatches of ``bc_loss`` (cross-entropy on the
        labelled samples), ``value_loss``, ``entropy_loss``, ``loss``,
        ``accuracy`` (labelled samples whose argmax is the label), ``labelled``
        (their share), ``grad_norm``, and ``n_minibatches``, ``n_updates``."""
        self._check_masks(buf)
        self._labels(buf)
        m, n_mb = self._run_epochs(buf, epoch_orders)
        return dict(bc_loss=m[0], value_loss=m[1], entropy_loss=m[2], loss=m[3], accuracy=m[4], labelled=m[5],
                    grad_norm=m[6], n_minibatches=n_mb, n_updates=self.n_updates)


def _own_best_rate(buf) -> Dict[str, float]:
    """``own_best_rate`` of a rollout collected with ``execute="best"``: the share of steps where
    the policy's own sample was among the shortest actions (its stochastic on-path rate)."""
    ob = getattr(buf, "own_best", None)
    return {} if ob is None else {"own_best_rate": float(ob.float().mean())}


def warm_start(collector: DaggerCollector, learner: BCLearner, total_timesteps: int,
               beta: Union[float, Callable[[int], float]] = 1.0, callback=None) -> List[Dict[str, float]]:
    """DAgger: alternate ``collector.collect()`` under ``beta`` and
    ``learner.train()`` until ``total_timesteps`` env steps were collected,
    pushing the updated weights into the collector after every update (the
    loop and the callbacks of ``ppo.learn``).

    ``beta``: the probability of executing the planner's action, a float or
    ``callable(iteration) -> float`` with iteration 0, 1, ... (DAgger lets it
    fall from 1, e.g. ``lambda i: 0.5 ** i``).

    Returns the per-iteration rows: the train dict (``BCLearner.train``),
    ``beta``, ``num_timesteps``, ``expert_share`` (the mean of
    ``took_expert``), ``own_best_rate`` (the mean of ``own_best``, with a
    collector that has ``execute="best"``), the Monitor and exploration keys ``ppo.learn`` reports
    and the evaluation's ``eval/*`` keys when one ran; with a reward
    normaliser on the collector its ``ret_rms_var`` / ``ret_rms_mean``."""
    def begin(it):
        b = float(beta(it)) if callable(beta) else float(beta)
        collector.set_beta(b)
        return {"beta": b}

    return run_loop(collector, learner, total_timesteps, callback, begin=begin,
                    extra=lambda buf: {"expert_share": float(buf.took_expert.float().mean()), **_own_best_rate(buf)})


def _check_bc_coef(c) -> float:
    v = float(c)
    if not (np.isfinite(v) and v >= 0.0):
        raise ValueError(f"bc_coef must be finite and >= 0, got {c!r}")
    return v


class KickstartLearner(_PlannerLabels, PPOLearner):
    """PPO with an auxiliary cross-entropy to the planner's labels on the
    policy's own rollouts (kickstarting): per minibatch
        loss = PPO's loss + bc_coef * CE(labelled samples)
    (the formula of include/voxnav.h vn_ppo_bc_loss), with the parent's
    minibatch order, LSTM re-run, all-reduce, grad-norm clip and Adam step.
    ``train()`` takes a ``DaggerBuffer`` collected with beta = 0: with an
    executed planner action the importance ratio would pair an action with
    another action's old log-prob (``DaggerBuffer``).  ``labels`` as
    ``BCLearner``'s.  With a process group the ranks' gradients are averaged
    equally, although their labelled counts may differ.

    ``action_masks=True`` trains on a ``MaskedDaggerBuffer`` (beta = 0): every
    sample's softmax runs over S = its mask with the taken action and the
    label's bits (of a labelled sample) added, an empty set counting as full
    (the rule of vn_ppo_bc_loss_masked), in ``learn_ops.ppo_bc_loss_masked`` /
    ``ppo_bc_loss_set_masked`` where the fused loss runs, else through torch
    autograd of the same formula.

    ``labels="soft"`` / ``label_tau`` as ``BCLearner``'s (the formula of
    vn_ppo_bc_loss_soft, through ``learn_ops.ppo_bc_loss_soft`` /
    ``ppo_bc_loss_soft_masked``)."""

    def __init__(self, policy, learning_rate: float = 3e-4, n_epochs: int = 10, batch_size: int = 64,
                 clip_range: float = 0.2, ent_coef: float = 0.01, vf_coef: float = 0.5, max_grad_norm: float = 0.5,
                 normalize_advantage: bool = True, seed: int = 0, process_group=None, bc_coef: float = 1.0,
                 labels: str = "action", action_masks: bool = False, target_kl: Optional[float] = None,
                 clip_range_vf=None, label_tau: Union[float, Callable[[float], float]] = 1.0):
        if clip_range_vf is not None:
            raise ValueError("KickstartLearner takes no clip_range_vf: no fused PPO+BC entry point clips the "
                             "value update")
        super().__init__(policy, learning_rate=learning_rate, n_epochs=n_epochs, batch_size=batch_size,
                         clip_range=clip_range, ent_coef=ent_coef, vf_coef=vf_coef, max_grad_norm=max_grad_norm,
                         normalize_advantage=normalize_advantage, seed=seed, process_group=process_group,
                         action_masks=action_masks, target_kl=target_kl)
        # minibatches that went through learn_ops.ppo_bc_loss / ppo_bc_loss_set or, counted in
        # masked_fused_updates as well, their masked forms
        self.fused_updates = 0
        self.labels = _check_labels(labels)
        self._init_label_tau(label_tau)
        self.bc_coef = _check_bc_coef(bc_coef)

    def set_bc_coef(self, bc_coef: float) -> None:
        """The cross-entropy's coefficient, from the next minibatch on."""
        self.bc_coef = _check_bc_coef(bc_coef)

    def update(self, buf, idx: torch.Tensor, packed: Optional[dict] = None) -> torch.Tensor:
        """One minibatch (env-major flat ids ``idx``).  Returns the logged
        values as a device tensor: ``PPOLearner.update``'s six (the loss with
        the cross-entropy term), cross-entropy, accuracy, labelled share, grad
        norm."""
        self._check_masks(buf)
        if self.recurrent:
            (lat_pi, lat_vf, lat_pair), src = self._evaluate_recurrent(buf, packed or self._pack_begin(buf, idx))
        else:
            (lat_pi, lat_vf, lat_pair), src = self._evaluate_ff(buf, idx)
        norm = self.normalize_advantage and (self.recurrent or src.numel() > 1)
        labels, weight = self._labels(buf)
        pol = self.policy
        ex = pol.mlp_extractor
        if lat_pi.is_cuda and self.fused_loss:
            F = ex.latent_dim_pi
            if F == ex.latent_dim_vf and learn_ops.ppo_loss_supported(pol.action_net, pol.value_net, F):
                h = learn_ops.mlp_pair(ex.policy_net, ex.value_net, lat_pi, None if lat_vf is lat_pi else lat_vf,
                                       x_pair=lat_pair, stacked=True)
                if h is not None:
                    bufs = (buf.actions.reshape(-1), buf.advantages.reshape(-1), buf.log_probs.reshape(-1),
                            buf.returns.reshape(-1), labels, weight)
                    coefs = (self.clip_range, self.ent_coef, self.vf_coef, self.bc_coef,
                             *((self.label_tau,) if self.labels == "soft" else ()), norm)
                    if self.action_masks:
                        fused = {"set": learn_ops.ppo_bc_loss_set_masked, "soft": learn_ops.ppo_bc_loss_soft_masked,
                                 "action": learn_ops.ppo_bc_loss_masked}[self.labels]
                        dh, grads, stats = fused(h, pol.action_net, pol.value_net, src, *bufs,
                                                 buf.action_masks.reshape(-1), *coefs)
                        self.masked_fused_updates += 1
                    else:
                        fused = {"set": learn_ops.ppo_bc_loss_set, "soft": learn_ops.ppo_bc_loss_soft,
                                 "action": learn_ops.ppo_bc_loss}[self.labels]
                        dh, grads, stats = fused(h, pol.action_net, pol.value_net, src, *bufs, *coefs)
                    self.fused_updates += 1
                    return self._step_fused(h, dh, grads, stats)
        # torch's ops and autograd: the CPU path, and heads the fused kernel does not take
        h_pi, h_vf = learn_ops.mlp_pair(ex.policy_net, ex.value_net, lat_pi, None if lat_vf is lat_pi else lat_vf,
                                        x_pair=lat_pair)
        logits = learn_ops.linear(h_pi, pol.action_net)
        values = learn_ops.linear(h_vf, pol.value_net).flatten()
        A = logits.shape[-1]
        taken = buf.actions.reshape(-1)[src].long()
        w = torch.ones_like(values) if weight is None else (weight[src] != 0).to(values.dtype)
        masks = buf.action_masks.reshape(-1)[src] if self.action_masks else None
        logits, lp_all, lp, w, right_of = _cross_entropy(logits, labels[src], w, self.labels == "set", masks, taken,
                                                         tau=self._tau())
        log_prob = lp_all.gather(1, taken.view(-1, 1)).flatten()
        entropy = -(lp_all.exp() * lp_all).sum(-1)
        adv = buf.advantages.reshape(-1)[src]
        if norm:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        old_lp = buf.log_probs.reshape(-1)[src]
        ret = buf.returns.reshape(-1)[src]
        ratio = torch.exp(log_prob - old_lp)
        policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - self.clip_range, 1 + self.clip_range)).mean()
        value_loss = Fn.mse_loss(ret, values)
        entropy_loss = -entropy.mean()
        n = w.sum()
        den = torch.clamp(n, min=1.0)
        bc = (w * -lp).sum() / den
        loss = policy_loss + self.ent_coef * entropy_loss + self.vf_coef * value_loss + self.bc_coef * bc
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        if self.group is not None:
            self._allreduce_grads()
        with torch.no_grad():
            log_ratio = log_prob - old_lp
            approx_kl = ((torch.exp(log_ratio) - 1) - log_ratio).mean().double()
        gnorm = self._clip_step(approx_kl)
        with torch.no_grad():
            top = logits.max(-1, keepdim=True).values
            ar = torch.arange(A, device=logits.device).expand_as(logits)
            amax = torch.where(logits == top, ar, torch.full_like(ar, A)).min(-1).values   # ties: the lowest index
            acc = (w.double() * right_of(amax).double()).sum() / den.double()
            return torch.stack([policy_loss.detach().double(), value_loss.detach().double(),
                                entropy_loss.detach().double(), loss.detach().double(), approx_kl,
                                (torch.abs(ratio - 1) > self.clip_range).double().mean(), bc.detach().double(), acc,
                                n.double() / w.numel(), gnorm.detach().double()])

    def train(self, buf, epoch_orders: Optional[Sequence] = None) -> Dict[str, float]:
        """One ``train()`` over a ``DaggerBuffer`` collected with beta = 0
        (n_epochs passes).  Returns ``PPOLearner.train``'s keys plus
        ``bc_loss``, ``accuracy`` and ``labelled`` (``BCLearner.train``)."""
        self._check_masks(buf)
        self._labels(buf)
        took = getattr(buf, "took_expert", None)
        if took is not None and bool(took.any()):       # one host read per rollout
            raise ValueError(f"{type(self).__name__} needs a rollout collected with beta = 0: where the planner's "
                             "action was executed, log_probs belong to another action (DaggerBuffer)")
        m, n_mb = self._run_epochs(buf, epoch_orders, width=10)
        return dict(policy_gradient_loss=m[0], value_loss=m[1], entropy_loss=m[2], loss=m[3], approx_kl=m[4],
                    clip_fraction=m[5], bc_loss=m[6], accuracy=m[7], labelled=m[8], grad_norm=m[9],
                    explained_variance=self._explained_variance(buf), n_minibatches=n_mb, n_updates=self.n_updates,
                    early_stop=self.early_stop, epochs_run=self.epochs_run)


def kickstart(collector: DaggerCollector, learner: KickstartLearner, total_timesteps: int,
              bc_coef: Union[float, Callable[[int], float]] = 1.0, callback=None) -> List[Dict[str, float]]:
    """Kickstarted PPO: ``ppo.learn``'s loop (its callbacks, Monitor,
    exploration and reward-normaliser keys) over a ``DaggerCollector`` at
    beta = 0 and a ``KickstartLearner``.

    ``bc_coef``: the cross-entropy's coefficient, a float or
    ``callable(iteration) -> float`` with iteration 0, 1, ... (kickstarting
    lets it decay to 0, e.g. ``lambda i: 0.5 ** i``; at 0 the update is
    ``PPOLearner``'s).

    Returns the per-iteration rows: the train dict
    (``KickstartLearner.train``), ``bc_coef``, ``num_timesteps``,
    ``own_best_rate`` (with a collector that has ``execute="best"``) and the
    keys ``ppo.learn`` reports."""
    collector.set_beta(0.0)

    def begin(it):
        c = float(bc_coef(it)) if callable(bc_coef) else float(bc_coef)
        learner.set_bc_coef(c)
        return {"bc_coef": c}

    return run_loop(collector, learner, total_timesteps, callback, begin=begin, extra=_own_best_rate)
