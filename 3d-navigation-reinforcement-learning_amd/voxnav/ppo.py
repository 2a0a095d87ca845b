"""PPO learner on the collector's device buffers.

Restates the update the reference runs through ``model.learn``
(train/Grid_Train.py:228; RecurrentPPO with the hyperparameters of
train/Grid_Train.py:84-86: lr 3e-4, batch_size 64, n_epochs 10, clip 0.2,
ent_coef 0.01, vf_coef 0.5; SB3 defaults max_grad_norm 0.5,
normalize_advantage True, Adam eps 1e-5):

* sb3_contrib ``RecurrentPPO.train`` for ``RecurrentActorCriticPolicy``:
  per epoch the env-major flattened buffer (``swap_and_flatten``) is rolled
  by a random split index and cut into minibatches of ``batch_size``
  samples; each minibatch is split into sequences at episode starts and env
  changes (``create_sequencers``), padded, and both LSTMs are re-run from
  the buffer's stored states at the sequence starts (``_process_sequence``);
  clipped surrogate + value MSE + entropy over the unpadded positions,
  advantages normalised per minibatch, grad-norm clip, Adam.
* SB3 ``PPO.train`` for ``ActorCriticPolicy``: a random permutation per
  epoch, same losses without sequences.

Everything stays on the device: minibatch rows are gathered straight from
the collector's ``[T, N]``-major buffers by index arithmetic (no flattened
copies), sequences are packed with one scatter, and both LSTMs run together
over the padded batch (``voxnav.lstm_seq.dual_lstm``: one fused
matrix-core launch per step, csrc/voxnav_learn_f32.hip, forward and
backward), which equals sb3's masked per-step loop because a sequence can only begin
with an episode start.
The one host round-trip per recurrent minibatch is the (n_seq, max_len)
pair that sizes the padded tensor (none in the row layout,
``voxnav.lstm_seq.dual_lstm_rows``).  From the MLP latents on, the heads,
the advantage normalisation, the three losses and their gradient run in the
fused loss kernel (``learn_ops.ppo_loss``, csrc/voxnav_ppo_loss.hip); the
latents' gradient is backpropagated through the MLP and LSTM kernels.

With ``process_group`` set, gradients are averaged over the ranks (one
flattened all-reduce per minibatch, RCCL over xGMI with the nccl backend)
before the clip -- data-parallel training over agent shards.

``action_masks=True`` trains on a ``MaskedRolloutBuffer`` (a collector with
``action_masks=True``; sb3_contrib ``MaskablePPO.train``): every sample's
softmax, log-prob and entropy run over its allowed actions ``S`` -- its mask
with the taken action added, an empty set counting as full -- in the fused
masked kernel (``learn_ops.ppo_loss_masked``, csrc/voxnav_masked_loss.hip)
where the fused loss runs, else through torch autograd of the same formula:
logits ``masked_fill(~S, -inf)``, ``log_softmax``, the entropy with the masked
terms zeroed (also the CPU path).

sb3's three controls over how far one ``train()`` moves the policy (DESIGN.md
10.10), all off by default:

* ``target_kl``: the passes end once a minibatch's approximate KL exceeds
  1.5 ``target_kl``; that minibatch is logged and not stepped.  On the fused
  path the comparison runs on the device between the loss and the Adam step
  (``learn_ops.kl_gate``, csrc/voxnav_trust.hip: the step's skip word), the
  remaining minibatches of that epoch run and change nothing, and the host
  reads the stop word once per epoch; elsewhere it is a host comparison and a
  ``break``.  With a process group the ranks' mean KL decides.
* ``clip_range_vf``: the value loss on ``v`` clamped to the rollout's value
  +- ``clip_range_vf`` (``learn_ops.ppo_loss_vclip`` / ``ppo_loss_masked_vclip``,
  csrc/voxnav_vclip_loss.hip; ``torch.clamp`` on the torch path).
* ``learning_rate``, ``clip_range`` and ``clip_range_vf`` may be callables of the
  remaining progress in [0, 1]; ``set_progress`` evaluates them, and ``learn``
  calls it before every ``train()``.

The minibatch order is drawn from ``numpy.random.default_rng(seed)``
(sb3 uses the global numpy generator) or passed explicitly as
``epoch_orders`` (what the parity tests do with ``oracle/ppo_oracle.py``).
"""
from __future__ import annotations

import os
from contextlib import nullcontext as _nullctx
from typing import Callable, Dict, List, Optional, Sequence, Union

import numpy as np
import torch
import torch.nn.functional as Fn

from . import _native, learn_ops, lstm_seq
from .lstm_seq import dual_lstm
from .policy import ActorCriticPolicy, RecurrentActorCriticPolicy


Schedule = Union[float, Callable[[float], float]]


def _check_clip_range_vf(c) -> float:
    v = float(c)
    if not v > 0.0:                       # also NaN
        raise ValueError(f"clip_range_vf must be > 0 (inf: no clip), got {c!r}")
    return v


class PPOLearner:
    def __init__(self, policy, learning_rate: Schedule = 3e-4, n_epochs: int = 10, batch_size: int = 64,
                 clip_range: Schedule = 0.2, ent_coef: float = 0.01, vf_coef: float = 0.5,
                 max_grad_norm: float = 0.5, normalize_advantage: bool = True, seed: int = 0, process_group=None,
                 action_masks: bool = False, target_kl: Optional[float] = None,
                 clip_range_vf: Optional[Schedule] = None):
        if not isinstance(policy, (ActorCriticPolicy, RecurrentActorCriticPolicy)):
            raise TypeError("policy must be an ActorCriticPolicy or RecurrentActorCriticPolicy")
        if batch_size < 1 or n_epochs < 1:
            raise ValueError("batch_size and n_epochs must be >= 1")
        if target_kl is not None and not (np.isfinite(float(target_kl)) and float(target_kl) > 0.0):
            raise ValueError(f"target_kl must be a positive finite number or None, got {target_kl!r}")
        self.policy = policy
        self.recurrent = bool(getattr(policy, "recurrent", False))
        # learning_rate, clip_range and clip_range_vf: floats, or callables of the remaining
        # progress (1 at the start of training, 0 at its end: sb3's schedules), evaluated by
        # set_progress; until its first call they hold their value at 1
        self._schedules = {k: v for k, v in (("lr", learning_rate), ("clip_range", clip_range),
                                             ("clip_range_vf", clip_range_vf)) if callable(v)}
        at_start = lambda v: v(1.0) if callable(v) else v  # noqa: E731
        self.lr = float(at_start(learning_rate))
        self.n_epochs = int(n_epochs)
        self.batch_size = int(batch_size)
        self.clip_range = float(at_start(clip_range))
        self.clip_range_vf = None if clip_range_vf is None else _check_clip_range_vf(at_start(clip_range_vf))
        # stop a train() once a minibatch's approximate KL exceeds 1.5 target_kl (sb3): that
        # minibatch is logged and not stepped, nothing after it is stepped or logged
        self.target_kl = None if target_kl is None else float(target_kl)
        self._kl = None              # the running train()'s gate state (_kl_begin)
        self.ent_coef = float(ent_coef)
        self.vf_coef = float(vf_coef)
        self.max_grad_norm = float(max_grad_norm)
        self.normalize_advantage = bool(normalize_advantage)
        self.action_masks = bool(action_masks)
        # minibatches that went through learn_ops.ppo_loss_masked (imitate's learners: their masked losses)
        self.masked_fused_updates = 0
        self.rng = np.random.default_rng(seed)
        self.group = process_group
        self.params = [p for p in policy.parameters() if p.requires_grad]
        # on the GPU one fused Adam kernel over all parameters (sb3's Adam, same
        # update; torch's per-tensor foreach path costs ~9 launches per step)
        fused = bool(self.params) and all(p.is_cuda for p in self.params)
        self.optimizer = torch.optim.Adam(self.params, lr=self.lr, eps=1e-5, fused=fused or None)
        self.n_updates = 0
        # heads + losses + their gradient in one fused kernel family on the GPU
        # (learn_ops.ppo_loss); VOXNAV_FUSED_LOSS=0: torch's ops and autograd (A/B knob)
        self.fused_loss = os.environ.get("VOXNAV_FUSED_LOSS", "1") != "0"
        # the Adam step on the library's kernel (learn_ops.adam_step, the optimizer's
        # own state tensors); VOXNAV_NATIVE_ADAM=0: torch's fused Adam
        self.native_adam = os.environ.get("VOXNAV_NATIVE_ADAM", "1") != "0"
        # the recurrent learner's row-layout LSTM; VOXNAV_LSTM_ROWS=0: the per-sequence packed path (A/B knob)
        self.lstm_rows = os.environ.get("VOXNAV_LSTM_ROWS", "1") != "0"
        # the row-layout LSTM keeps all its blocks resident and hands states over
        # inside the launch: with another rank's grid on the same device that
        # co-residency is not guaranteed, so such ranks take the packed path
        self._rows_off = self.recurrent and process_group is not None and _ranks_share_device(process_group,
                                                                                             self.params)

    # ------------------------------------------------------------ helpers
    def _orders(self, total: int) -> List:
        if self.recurrent:
            return [int(self.rng.integers(total)) for _ in range(self.n_epochs)]
        return [self.rng.permutation(total) for _ in range(self.n_epochs)]

    def set_progress(self, progress_remaining: float) -> None:
        """Evaluate the schedules (callable ``learning_rate`` / ``clip_range`` /
        ``clip_range_vf``) at the remaining progress in [0, 1] -- sb3's
        ``_update_current_progress_remaining`` + ``_update_learning_rate``; ``run_loop``
        calls it before every ``train()``.  Float hyper-parameters are left alone."""
        p = float(progress_remaining)
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"progress_remaining must be in [0, 1], got {progress_remaining!r}")
        for name, fn in self._schedules.items():
            v = float(fn(p))
            if name == "lr":
                self.lr = v
                self.optimizer.param_groups[0]["lr"] = v     # learn_ops.adam_step reads it per call
            elif name == "clip_range":
                self.clip_range = v
            else:
                self.clip_range_vf = _check_clip_range_vf(v)

    # ------------------------------------------------------------ target_kl
    def _kl_begin(self, dev) -> dict:
        """A fresh gate state (``train()``; ``update`` outside of it makes one on first use):
        on the GPU the device words ``stop`` (sticky) and ``skip`` of learn_ops.kl_gate and the
        minibatches' ``ran`` bytes, elsewhere the host's flag."""
        self._kl = dict(host_stop=False, rans=[], stop=None, skip=None)
        if torch.device(dev).type == "cuda":
            words = torch.zeros(2, dtype=torch.int32, device=dev)
            self._kl.update(stop=words[0:1], skip=words[1:2])
        return self._kl

    def _kl_mean(self, kl: torch.Tensor) -> torch.Tensor:
        """The minibatch's approximate KL as a [1] f64 tensor, with a process group the
        ranks' mean (one scalar all-reduce), so that every rank stops at the same minibatch."""
        kl = kl.detach().double().reshape(1)
        if self.group is None:
            return kl
        import torch.distributed as dist
        kl = kl.clone()
        dist.all_reduce(kl, op=dist.ReduceOp.SUM, group=self.group)
        return kl / dist.get_world_size(self.group)

    def _kl_gate(self, kl: torch.Tensor, err: Optional[torch.Tensor]) -> torch.Tensor:
        """The device gate between a fused loss and the Adam step: -> the step's skip word."""
        st = self._kl if self._kl is not None and self._kl["stop"] is not None else self._kl_begin(kl.device)
        ran = torch.empty(1, dtype=torch.uint8, device=kl.device)
        learn_ops.kl_gate(self._kl_mean(kl), 1.5 * self.target_kl, st["stop"], st["skip"], ran, err, kl_index=0)
        st["rans"].append(ran)
        return st["skip"]

    def _kl_host(self, kl: torch.Tensor) -> bool:
        """The same rule with a host comparison (one read of the KL): True -> no step, and
        ``update_many`` / ``train`` stop after this minibatch."""
        st = self._kl if self._kl is not None else self._kl_begin(kl.device)
        if float(self._kl_mean(kl)) > 1.5 * self.target_kl:      # strict; a NaN does not stop
            st["host_stop"] = True
            return True
        return False

    def _allreduce_grads(self):
        """Average the gradients over the group (one flattened all-reduce).
        The recurrent learner appends its row-layout error word (1.0 when an
        in-launch hand-off of this rank timed out) to the same buffer, and every
        rank takes the reduced word as its own: if any rank's gradients are
        garbage, every rank skips the Adam step and every rank raises in
        ``update_many`` (no rank applies a corrupted average, no rank runs on
        into the next collective alone)."""
        import torch.distributed as dist
        grads = [p.grad for p in self.params if p.grad is not None]
        parts = [g.reshape(-1) for g in grads]
        err = lstm_seq._rows_err(grads[0].device) if self.recurrent else None
        if err is not None:
            parts.append((err != 0).to(grads[0].dtype).view(1))
        flat = torch.cat(parts)
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=self.group)
        if err is not None:
            err.copy_((flat[-1:] != 0).to(err.dtype))
            flat = flat[:-1]
        flat /= dist.get_world_size(self.group)
        o = 0
        for g in grads:
            n = g.numel()
            g.copy_(flat[o:o + n].view_as(g))
            o += n

    def _heads(self, lat_pi, lat_vf, actions, lat_pair=None, masks=None):
        pol = self.policy
        # both MLP branches layer by layer and the heads on the f32 matrix
        # cores (voxnav/learn_ops.py; torch's own ops on the CPU)
        ex = pol.mlp_extractor
        h_pi, h_vf = learn_ops.mlp_pair(ex.policy_net, ex.value_net, lat_pi, None if lat_vf is lat_pi else lat_vf,
                                        x_pair=lat_pair)
        logits = learn_ops.linear(h_pi, pol.action_net)
        values = learn_ops.linear(h_vf, pol.value_net).flatten()
        if masks is not None:
            # the allowed set: the mask's bits, the taken action, and everything when that is empty
            A = logits.shape[-1]
            ar = torch.arange(A, device=masks.device)
            S = ((masks.view(-1, 1).to(torch.int64) >> ar) & 1).bool()
            S = S | (ar.view(1, A) == actions.view(-1, 1))
            S = S | ~S.any(-1, keepdim=True)
            logits = logits.masked_fill(~S, float("-inf"))
        logp_all = torch.log_softmax(logits, dim=-1)
        if masks is not None:
            # a masked action's terms are zeros (exp(0) 0 in the entropy), and it gets no gradient
            logp_all = torch.where(S, logp_all, logp_all.new_zeros(()))
        log_prob = logp_all.gather(1, actions.view(-1, 1)).flatten()
        entropy = -(logp_all.exp() * logp_all).sum(-1)
        return values, log_prob, entropy

    def _pack_begin(self, buf, idx: torch.Tensor, window: bool = False) -> dict:
        """The sequence structure of minibatch rows ``idx`` (env-major flat
        ids): sequences start at episode starts and env changes
        (sb3_contrib create_sequencers).  Everything but the padded size
        (n_seq, max_len) stays on the device; on CUDA the structure is
        computed on a side stream and the size copied to pinned host memory,
        so the one host read per minibatch can wait for it while the previous
        minibatch's update still runs (``update_many``).

        ``window``: the caller guarantees ``idx`` is one contiguous window of
        the rolled env-major order (``(idx[0] + i) mod T N``, what ``train``
        cuts) -- the row layout's mapping is only valid for such minibatches;
        any other index set takes the packed per-sequence path."""
        T, N = buf.actions.shape
        dev = idx.device
        side = None
        if dev.type == "cuda":
            if getattr(self, "_side", None) is None:
                self._side = torch.cuda.Stream(dev)
            side = self._side
            side.wait_stream(torch.cuda.current_stream(dev))
        n = idx.numel()
        rows = n // T if (window and dev.type == "cuda" and n % T == 0 and n // T <= N) else 0
        if rows and not self._rows_ok(buf.obs.shape[-1], rows):
            rows = 0
        with torch.cuda.stream(side) if side is not None else _nullctx():
            env = idx // T
            t = idx - env * T
            src = t * N + env                                         # row in the [T, N]-major buffers
            es = buf.episode_starts.reshape(-1)[src]
            if rows:
                # row layout (csrc/voxnav_learn_rows.hip): row r = env e0 + r over all T
                # steps; the last env of a minibatch that starts mid-rollout (steps
                # t < t0) shares row 0 with the first (steps >= t0)
                r = torch.remainder(env - env[0], N)
                r = torch.where(r == rows, torch.zeros_like(r), r)
                pos = t * rows + r
                t0 = t[0]
                st = (t == 0) | (es > 0.5) | ((r == 0) & (t == t0) & (t0 > 0))
                src_rows = torch.empty_like(src)
                src_rows[pos] = src
                grid = dict(src=src_rows,
                            env=torch.empty(n, dtype=torch.int32, device=dev).index_put_((pos,), env.to(torch.int32)),
                            start=torch.empty(n, dtype=torch.uint8, device=dev).index_put_((pos,), st.to(torch.uint8)),
                            keep=torch.empty(n, dtype=torch.float32, device=dev).index_put_((pos,), 1.0 - es))
                pk = dict(idx=idx, rows=rows, **grid)
                if side is not None:
                    ev = torch.cuda.Event()
                    ev.record(side)
                    pk["ev"] = ev
        if rows:
            if side is not None:
                main = torch.cuda.current_stream(dev)
                for v in pk.values():
                    if isinstance(v, torch.Tensor) and v.is_cuda:
                        v.record_stream(main)
            return pk
        with torch.cuda.stream(side) if side is not None else _nullctx():
            seq_start = (es > 0.5) | (t == 0)                         # episode start or env change
            seq_start[0] = True
            seq_id = torch.cumsum(seq_start.to(torch.int64), 0) - 1
            ar = torch.arange(idx.numel(), device=dev)
            # position in the sequence: distance to the last start at or before (a running max, no sync)
            pos = ar - torch.cummax(torch.where(seq_start, ar, torch.zeros_like(ar)), 0).values
            size = torch.stack([seq_id[-1] + 1, pos.max() + 1])
            pk = dict(idx=idx, env=env, t=t, src=src, es=es, seq_start=seq_start, seq_id=seq_id, pos=pos)
            if side is not None:
                host = torch.empty(2, dtype=torch.int64, pin_memory=True)
                host.copy_(size, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(side)
                pk.update(host=host, ev=ev)
            else:
                pk.update(host=size)
        if side is not None:
            main = torch.cuda.current_stream(dev)
            for v in pk.values():
                if isinstance(v, torch.Tensor) and v.is_cuda:
                    v.record_stream(main)            # made on the side stream, used on the main one
        return pk

    def _rows_ok(self, D: int, rows: int) -> bool:
        """The row-layout LSTM kernels take (D, rows) for this policy (cached host query)."""
        cache = self.__dict__.setdefault("_rows_cache", {})
        # the layout option decides the grid the library checks, so it is part of the key
        key = (D, rows, _native.get_option("rows_layout"))
        if key not in cache:
            cache[key] = self.lstm_rows and not self._rows_off and lstm_seq.rows_supported(self.policy, D, rows)
        return cache[key]

    def _evaluate_rows(self, buf, pk: dict):
        """evaluate_actions in the row layout: both LSTMs over [T, rows] in one
        persistent launch each (no host read, no padding)."""
        T, N = buf.actions.shape
        rows = pk["rows"]
        if "ev" in pk:
            torch.cuda.current_stream(pk["idx"].device).wait_event(pk["ev"])
        src = pk["src"]
        D = buf.obs.shape[-1]
        x = buf.obs.reshape(T * N, D)[src].view(T, rows, D)
        out = lstm_seq.dual_lstm_rows_pair(self.policy, x, pk["env"], pk["start"], pk["keep"], buf.lstm_h,
                                           buf.lstm_c)                       # [2, T, rows, H]: actor, critic
        H = out.shape[-1]
        lat = out.view(2, T * rows, H)
        return (lat[0], lat[1], lat), src

    def _evaluate_recurrent(self, buf, pk: dict):
        """evaluate_actions on a packed minibatch (``_pack_begin``)."""
        T, N = buf.actions.shape
        if "rows" in pk:
            return self._evaluate_rows(buf, pk)
        if "ev" in pk:
            pk["ev"].synchronize()                                # the minibatch's size only
            torch.cuda.current_stream(pk["idx"].device).wait_event(pk["ev"])
        n_seq, max_len = (int(v) for v in pk["host"].tolist())
        src, es, seq_start, seq_id, pos, t, env = (pk[k] for k in ("src", "es", "seq_start", "seq_id", "pos", "t",
                                                                   "env"))
        dev = src.device
        first = (torch.nonzero_static(seq_start, size=n_seq).flatten() if dev.type == "cuda"
                 else torch.nonzero(seq_start, as_tuple=True)[0])   # position of each sequence start
        D = buf.obs.shape[-1]
        x = torch.zeros((max_len, n_seq, D), dtype=torch.float32, device=dev)
        x[pos, seq_id] = buf.obs.reshape(T * N, D)[src]
        keep = (1.0 - es[first]).view(1, n_seq, 1)               # (1 - episode_start) at the sequence start
        tf, ef = t[first], env[first]
        h0 = buf.lstm_h[tf, :, ef].permute(1, 0, 2) * keep        # stored states [T, 2, N, H] -> [2, n_seq, H]
        c0 = buf.lstm_c[tf, :, ef].permute(1, 0, 2) * keep
        out_pi, out_vf = dual_lstm(self.policy, x, h0, c0)
        lat_pi = out_pi[pos, seq_id]
        lat_vf = out_vf[pos, seq_id]
        return (lat_pi, lat_vf, None), src

    def _evaluate_ff(self, buf, idx: torch.Tensor):
        T, N = buf.actions.shape
        if idx.is_cuda and buf.obs.shape[-1] % 4 == 0 and buf.obs.is_contiguous():
            src, obs = learn_ops.minibatch_rows(idx.contiguous(), T, N, buf.obs)   # one launch
            return (obs, obs, None), src
        env = idx // T
        src = (idx - env * T) * N + env
        obs = buf.obs.reshape(T * N, -1)[src]
        return (obs, obs, None), src

    def _check_masks(self, buf) -> None:
        """``train`` and ``update`` refuse a buffer without masks when the learner masks."""
        if self.action_masks and getattr(buf, "action_masks", None) is None:
            raise ValueError("PPOLearner(action_masks=True) needs the buffer's action_masks "
                             "(RolloutCollector(action_masks=True))")

    def update(self, buf, idx: torch.Tensor, packed: Optional[dict] = None) -> torch.Tensor:
        """One minibatch (env-major flat ids ``idx``): losses, backward,
        (all-reduce), clip, Adam.  Returns the logged values as a device
        tensor (no host sync beyond the recurrent minibatch's size)."""
        self._check_masks(buf)
        if self.recurrent:
            (lat_pi, lat_vf, lat_pair), src = self._evaluate_recurrent(buf, packed or self._pack_begin(buf, idx))
        else:
            (lat_pi, lat_vf, lat_pair), src = self._evaluate_ff(buf, idx)
        norm = self.normalize_advantage and (self.recurrent or src.numel() > 1)
        if lat_pi.is_cuda and self.fused_loss:
            pol = self.policy
            ex = pol.mlp_extractor
            F = ex.latent_dim_pi
            if F == ex.latent_dim_vf and learn_ops.ppo_loss_supported(pol.action_net, pol.value_net, F):
                h = learn_ops.mlp_pair(ex.policy_net, ex.value_net, lat_pi, None if lat_vf is lat_pi else lat_vf,
                                       x_pair=lat_pair, stacked=True)
                if h is not None:
                    return self._update_fused(buf, h, src, norm)
        masks = buf.action_masks.reshape(-1)[src] if self.action_masks else None
        values, log_prob, entropy = self._heads(lat_pi, lat_vf, buf.actions.reshape(-1)[src].long(), lat_pair, masks)
        adv = buf.advantages.reshape(-1)[src]
        if norm:
            adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        old_lp = buf.log_probs.reshape(-1)[src]
        ret = buf.returns.reshape(-1)[src]
        ratio = torch.exp(log_prob - old_lp)
        l1 = adv * ratio
        l2 = adv * torch.clamp(ratio, 1 - self.clip_range, 1 + self.clip_range)
        policy_loss = -torch.min(l1, l2).mean()
        if self.clip_range_vf is not None:
            # v clamped to old +- c (include/voxnav.h vn_ppo_loss_vclip): inside the range v
            # itself, and clamp's backward passes the gradient on the inclusive range
            old_v = buf.values.reshape(-1)[src]
            values = torch.clamp(values, old_v - self.clip_range_vf, old_v + self.clip_range_vf)
        value_loss = Fn.mse_loss(ret, values)
        entropy_loss = -entropy.mean()
        loss = policy_loss + self.ent_coef * entropy_loss + self.vf_coef * value_loss
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        if self.group is not None:
            self._allreduce_grads()
        with torch.no_grad():
            log_ratio = log_prob - old_lp
            approx_kl = ((torch.exp(log_ratio) - 1) - log_ratio).mean().double()
        gnorm = self._clip_step(approx_kl)
        with torch.no_grad():
            return torch.stack([policy_loss.detach().double(), value_loss.detach().double(),
                                entropy_loss.detach().double(), loss.detach().double(), approx_kl,
                                (torch.abs(ratio - 1) > self.clip_range).double().mean(),
                                gnorm.detach().double()])

    def _update_fused(self, buf, h: torch.Tensor, src: torch.Tensor, norm: bool) -> torch.Tensor:
        """``update`` from the MLP latents h [2, M, F] on: the heads, losses and
        their gradient in the fused loss kernel (learn_ops.ppo_loss), then
        ``_step_fused``."""
        pol = self.policy
        if self.clip_range_vf is not None:
            bufs = (buf.actions.reshape(-1), buf.advantages.reshape(-1), buf.log_probs.reshape(-1),
                    buf.returns.reshape(-1))
            coefs = (self.clip_range, self.clip_range_vf, self.ent_coef, self.vf_coef, norm)
            if self.action_masks:
                dh, grads, stats = learn_ops.ppo_loss_masked_vclip(h, pol.action_net, pol.value_net, src, *bufs,
                                                                   buf.action_masks.reshape(-1),
                                                                   buf.values.reshape(-1), *coefs)
                self.masked_fused_updates += 1
            else:
                dh, grads, stats = learn_ops.ppo_loss_vclip(h, pol.action_net, pol.value_net, src, *bufs,
                                                            buf.values.reshape(-1), *coefs)
            return self._step_fused(h, dh, grads, stats)
        if self.action_masks:
            dh, grads, stats = learn_ops.ppo_loss_masked(h, pol.action_net, pol.value_net, src,
                                                         buf.actions.reshape(-1), buf.advantages.reshape(-1),
                                                         buf.log_probs.reshape(-1), buf.returns.reshape(-1),
                                                         buf.action_masks.reshape(-1), self.clip_range,
                                                         self.ent_coef, self.vf_coef, norm)
            self.masked_fused_updates += 1
            return self._step_fused(h, dh, grads, stats)
        dh, grads, stats = learn_ops.ppo_loss(h, pol.action_net, pol.value_net, src, buf.actions.reshape(-1),
                                              buf.advantages.reshape(-1), buf.log_probs.reshape(-1),
                                              buf.returns.reshape(-1), self.clip_range, self.ent_coef, self.vf_coef,
                                              norm)
        return self._step_fused(h, dh, grads, stats)

    def _step_fused(self, h: torch.Tensor, dh: torch.Tensor, grads, stats: torch.Tensor) -> torch.Tensor:
        """The rest of an update after a fused head loss (learn_ops.ppo_loss, bc_loss,
        bc_loss_set): dh backpropagated from h, the head gradients assigned, (all-reduce),
        clip, Adam.  Returns the loss's stats with the gradient norm appended."""
        pol = self.policy
        self.optimizer.zero_grad(set_to_none=True)
        h.backward(dh)
        for prm, g in zip((pol.action_net.weight, pol.action_net.bias, pol.value_net.weight, pol.value_net.bias),
                          grads):
            if prm.requires_grad:
                prm.grad = g
        if self.group is not None:
            self._allreduce_grads()
        gnorm = self._clip_step(stats[4:5])           # approx kl (the PPO objectives' stats)
        return torch.cat([stats, gnorm.detach().double().view(1)])

    def _clip_step(self, approx_kl: Optional[torch.Tensor] = None) -> torch.Tensor:
        """clip_grad_norm_ + Adam step.  On the GPU: the norm in two launches
        (learn_ops.grad_norm_scale) and the step in one (learn_ops.adam_step),
        the clip applied by the step as its divisor of the gradients; else
        torch's clip and step.  ``approx_kl`` (the minibatch's, a one-element
        tensor) with ``target_kl`` set: no step once it exceeds 1.5 target_kl --
        decided on the device before the native Adam step (learn_ops.kl_gate,
        no host read), by a host comparison elsewhere."""
        gate = self.target_kl is not None and approx_kl is not None
        fused = self.optimizer.param_groups[0].get("fused")
        if fused and self.params[0].is_cuda:
            gnorm, scale = learn_ops.grad_norm_scale(self.params, self.max_grad_norm)
            if self.native_adam:
                # the recurrent learner's row-layout launches set a device error word
                # when an in-launch hand-off times out; the step is skipped on the
                # device while it is set (rows_check raises after the minibatches)
                skip = lstm_seq.rows_err_word(self.params[0].device) if self.recurrent else None
                if gate:
                    skip = self._kl_gate(approx_kl, skip)
                learn_ops.adam_step(self.optimizer, scale, skip=skip)
            elif gate and self._kl_host(approx_kl):
                return gnorm
            else:
                self.optimizer.grad_scale = scale
                try:
                    self.optimizer.step()
                finally:
                    self.optimizer.grad_scale = None
        else:
            gnorm = torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)
            err = lstm_seq.rows_err_word(self.params[0].device) if self.recurrent else None
            if err is not None and err.device.type == "cpu" and int(err.item()) != 0:
                return gnorm                # a rank's hand-off timed out (the reduced word): no step anywhere
            if gate and self._kl_host(approx_kl):
                return gnorm
            self.optimizer.step()
        self.n_updates += 1
        return gnorm

    def update_many(self, buf, idxs: Sequence[torch.Tensor], windows: bool = False) -> torch.Tensor:
        """``update`` over consecutive minibatches, the next minibatch's
        sequence structure computed (side stream) while this one's update is
        queued, so the host read of its size does not idle the GPU.
        ``windows``: every ``idx`` is a contiguous window of the rolled
        env-major order (``train``'s minibatches), which lets whole-rollout
        minibatches take the row-layout LSTM.  Returns the stacked logs [n, 7].

        With ``target_kl`` and the host rule the loop ends with the minibatch that
        crosses the threshold (fewer rows than ``idxs``); with the device gate every
        minibatch runs and is returned, and the ones after the stop change nothing
        (``train`` leaves them out of its means).  Called outside ``train``, the gate
        starts fresh with each call."""
        idxs = list(idxs)
        if not idxs:
            return torch.zeros((0, 7), dtype=torch.float64)
        nxt = self._pack_begin(buf, idxs[0], windows) if self.recurrent else None
        n0 = self.n_updates
        own_kl = self.target_kl is not None and self._kl is None
        logs = []
        try:
            for i, idx in enumerate(idxs):
                cur = nxt
                if self.recurrent and i + 1 < len(idxs):
                    nxt = self._pack_begin(buf, idxs[i + 1], windows)
                logs.append(self.update(buf, idx, packed=cur))
                if self._kl is not None and self._kl["host_stop"]:
                    break                           # target_kl, host rule: this minibatch is the last one logged
        finally:
            if own_kl:
                self._kl = None
        if self.recurrent:
            try:
                lstm_seq.rows_check(self.params[0].device)   # a timed-out row-layout launch raises
            except Exception:
                # the skipped Adam steps did not advance the device step counters:
                # n_updates counts the steps actually applied, and the host mirror
                # of the step count is re-read on the next step
                cache = getattr(self.optimizer, "_vn_adam_t", None)
                if cache is not None:
                    t_dev = int(round(float(cache[0].item())))
                    self.n_updates = n0 + max(0, t_dev - (cache[1] - len(idxs)))
                self.optimizer._vn_adam_t = None
                raise
        return torch.stack(logs)

    # ------------------------------------------------------------ train
    def _run_epochs(self, buf, epoch_orders: Optional[Sequence], width: int = 7):
        """``train()``'s passes over the buffer (this class's and its subclasses'): per
        epoch the rolled (recurrent) or permuted env-major order cut into minibatches of
        ``batch_size``, through ``update_many``.  ``width``: the length of ``update``'s log
        vector.  -> (the logs' means over the minibatches, the minibatch count).

        With ``target_kl`` the passes end with the epoch in which a minibatch's approximate
        KL exceeded 1.5 target_kl (``self.early_stop``, ``self.epochs_run``); the means and
        the count are over the minibatches up to and including that one.  On the device
        gate the sums and the count stay on the device (weighted by the gate's ``ran``
        bytes) and the host reads the stop word once per epoch."""
        T, N = buf.actions.shape
        total = T * N
        dev = buf.actions.device
        if self.recurrent and (buf.lstm_h is None or buf.lstm_c is None):
            raise ValueError("the recurrent learner needs the buffer's LSTM states (store_lstm_states=True)")
        orders = list(epoch_orders) if epoch_orders is not None else self._orders(total)
        acc = torch.zeros(width, dtype=torch.float64, device=dev)
        n_mb = 0
        self.policy.train()
        self.early_stop, self.epochs_run = False, 0
        if self.target_kl is not None:
            return self._run_epochs_gated(buf, orders, acc)
        for order in orders:
            logs = self.update_many(buf, self._minibatches(order, total, dev), windows=self.recurrent)
            acc += logs.sum(0)
            n_mb += logs.shape[0]
            self.epochs_run += 1
        return (acc / max(1, n_mb)).tolist(), n_mb

    def _minibatches(self, order, total: int, dev) -> List[torch.Tensor]:
        if self.recurrent:
            perm = torch.roll(torch.arange(total, device=dev), -int(order))
        else:
            perm = torch.as_tensor(np.asarray(order), dtype=torch.int64, device=dev)
        return [perm[s:s + self.batch_size] for s in range(0, total, self.batch_size)]

    def _run_epochs_gated(self, buf, orders, acc: torch.Tensor):
        """``_run_epochs`` under ``target_kl``."""
        total = buf.actions.numel()
        dev = buf.actions.device
        n0 = self.n_updates
        st = self._kl_begin(dev)
        cnt = torch.zeros((), dtype=torch.float64, device=dev)
        try:
            for order in orders:
                logs = self.update_many(buf, self._minibatches(order, total, dev), windows=self.recurrent)
                self.epochs_run += 1
                if st["rans"]:
                    # the device gate: one byte per minibatch, 0 after the stop
                    if len(st["rans"]) != logs.shape[0]:
                        raise RuntimeError("target_kl: the minibatches of an epoch took different update paths")
                    ran = torch.cat(st["rans"]).to(torch.float64)
                    st["rans"] = []
                    acc += torch.where(ran.view(-1, 1) != 0, logs, logs.new_zeros(())).sum(0)
                    cnt += ran.sum()
                    self.early_stop = int(st["stop"].item()) != 0      # the epoch's one host read
                else:
                    acc += logs.sum(0)
                    cnt += logs.shape[0]
                    self.early_stop = st["host_stop"]
                if self.early_stop:
                    break
        finally:
            self._kl = None
        out = torch.cat([acc / cnt.clamp(min=1.0), cnt.view(1)]).tolist()
        n_mb = int(round(out[-1]))
        if self.early_stop:
            # the crossing minibatch was logged and not stepped; the skipped steps did not
            # advance the device step counters: the next step re-reads them
            self.n_updates = n0 + n_mb - 1
            self.optimizer._vn_adam_t = None
        return out[:-1], n_mb

    @staticmethod
    def _explained_variance(buf) -> float:
        with torch.no_grad():
            v, r = buf.values.reshape(-1), buf.returns.reshape(-1)
            var_r = torch.var(r)
            return float("nan") if float(var_r) == 0 else float(1 - torch.var(r - v) / var_r)

    def train(self, buf, epoch_orders: Optional[Sequence] = None) -> Dict[str, float]:
        """One ``train()`` over a collector ``RolloutBuffer`` (n_epochs passes).
        Returns the means of sb3's logged quantities, ``n_minibatches`` (the
        ones logged), ``n_updates`` (the steps applied so far), ``early_stop``
        (``target_kl`` ended the passes) and ``epochs_run``."""
        self._check_masks(buf)
        m, n_mb = self._run_epochs(buf, epoch_orders)
        return dict(policy_gradient_loss=m[0], value_loss=m[1], entropy_loss=m[2], loss=m[3], approx_kl=m[4],
                    clip_fraction=m[5], grad_norm=m[6], explained_variance=self._explained_variance(buf),
                    n_minibatches=n_mb, n_updates=self.n_updates, early_stop=self.early_stop,
                    epochs_run=self.epochs_run)


def _ranks_share_device(group, params) -> bool:
    """Whether another rank of ``group`` drives the same GPU as this one (one
    all-gather of (host, device uuid) at construction; False off the GPU)."""
    if not params or not params[0].is_cuda:
        return False
    import socket
    import torch.distributed as dist
    dev = params[0].device
    me = (socket.gethostname(), str(torch.cuda.get_device_properties(dev).uuid))
    allk = [None] * dist.get_world_size(group)
    dist.all_gather_object(allk, me, group=group)
    return allk.count(me) > 1


def learn(collector, learner: PPOLearner, total_timesteps: int, callback=None) -> List[Dict[str, float]]:
    """``model.learn(total_timesteps, callback=...)`` (OnPolicyAlgorithm.learn):
    alternate ``collector.collect()`` and ``learner.train()`` until
    ``total_timesteps`` env steps (agents x steps, summed over this rank)
    were collected, pushing the updated weights into the collector after
    every update.

    ``callback``: one callback or a list.  Objects with ``on_rollout_end``
    (``voxnav.evaluate.EvalCallback``, Grid_Train.py:218-226) run after each
    rollout, before the update -- the weights the rollout was collected
    with; plain callables ``callback(iteration, num_timesteps, stats)`` run
    after the update, returning False stops early (SB3 semantics).

    Returns the per-iteration stats: the train losses, ``num_timesteps``,
    the Monitor's ``ep_rew_mean`` / ``ep_len_mean`` over the last 100
    finished episodes (SB3's ``rollout/`` logger keys, when any episode has
    finished), for a rollout in which at least one episode ended the
    reference's episode-end figures over that rollout's episodes --
    ``ep_finished_rate``, ``ep_bumps_mean``, ``ep_discovered_mean`` and
    ``ep_coverage`` (discovered cells / max_steps as a ratio of the two sums;
    ``EpisodeMonitor._harvest_exploration``) -- and the evaluation's
    ``eval/*`` keys when one ran; with a reward normaliser on the collector
    (``voxnav.normalize``) its running ``ret_rms_var`` / ``ret_rms_mean``."""
    return run_loop(collector, learner, total_timesteps, callback)


def run_loop(collector, learner, total_timesteps: int, callback=None, begin=None, extra=None):
    """The loop of ``learn`` (and of ``imitate.warm_start`` / ``imitate.kickstart``, which
    add a schedule): ``begin(iteration)`` runs before each rollout (iteration 0, 1, ...)
    and ``extra(buf)`` after each update; the dicts they return go into the iteration's
    row between the train stats and the Monitor keys."""
    if collector.policy is not learner.policy:
        raise ValueError("collector and learner must share the policy module")
    cbs = [] if callback is None else (list(callback) if isinstance(callback, (list, tuple)) else [callback])
    per_rollout = collector.n_steps * collector.N
    done, it, history = 0, 0, []
    while done < total_timesteps:
        row = dict(begin(it) or {}) if begin is not None else {}
        buf = collector.collect()
        done += per_rollout
        it += 1
        evals = {}
        for cb in cbs:
            if hasattr(cb, "on_rollout_end"):
                evals.update(cb.on_rollout_end(learner.policy, done, collector.n_steps, learner.optimizer) or {})
        # the schedules see the progress with this rollout counted (sb3's
        # _update_current_progress_remaining); a no-op with float hyper-parameters, and a
        # learner without schedules need not have the method
        set_progress = getattr(learner, "set_progress", None)
        if set_progress is not None:
            set_progress(max(0.0, 1.0 - done / total_timesteps))
        st = learner.train(buf)
        collector.sync_weights()
        st.update(row)
        st["num_timesteps"] = done
        if extra is not None:
            st.update(extra(buf) or {})
        mon = getattr(collector, "monitor", None)
        if mon is not None and mon.ep_info_buffer:
            st["ep_rew_mean"] = mon.ep_rew_mean()
            st["ep_len_mean"] = mon.ep_len_mean()
        if mon is not None and getattr(mon, "last_exploration", None):
            st.update(mon.last_exploration)   # this rollout's episodes: ep_finished_rate, ep_bumps_mean, ...
        rn = getattr(collector, "reward_norm", None)
        if rn is not None:                    # the return statistics the rollout's rewards were scaled by
            st["ret_rms_var"], st["ret_rms_mean"] = rn.var, rn.mean
        st.update(evals)
        history.append(st)
        stop = False
        for cb in cbs:
            if not hasattr(cb, "on_rollout_end") and callable(cb) and cb(it, done, st) is False:
                stop = True
        if stop:
            break
    return history
