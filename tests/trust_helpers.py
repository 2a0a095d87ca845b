"""Restatements for the trust-region tests (test_trust_cpu.py, test_trust_gloo.py,
test_trust_gpu.py): the value-clipped PPO minibatch loss in float64 autograd
(vn_ppo_loss_vclip / vn_ppo_loss_masked_vclip, on tests/ppo_loss_helpers.py's
formula and tests/mask_helpers.py's allowed sets), the rule of vn_kl_gate, and a
float64 ``train()`` with sb3's early-stop loop, value clip and per-call learning
rate, on the pieces of oracle/ppo_oracle.py.  Importing this module needs no GPU."""
import numpy as np
import torch

import mask_helpers as mh
from oracle import ppo_oracle as po
from ppo_loss_helpers import close  # noqa: F401  (the PPO grid test's comparator)


# ------------------------------------------------------------------ the loss
def clip_bounds(old, c):
    """(lo, hi) = old -+ c formed in f32 (include/voxnav.h vn_ppo_loss_vclip), as float64."""
    old = old.detach().float()
    cf = torch.tensor(c, dtype=torch.float32, device=old.device)
    return (old - cf).double(), (old + cf).double()


def vclip_loss_reference(h, wa, ba, wv, bv, act, adv, olp, ret, old, clip, clip_vf, ent_coef, vf_coef, norm,
                         mask=None):
    """ppo_loss_helpers._ppo_loss_reference (``mask`` given:
    mask_helpers.masked_ppo_loss_reference) with the value loss on
    v' = clamp(v, old - c, old + c): torch.clamp's backward passes the gradient
    on the inclusive range.  -> (dh, head gradients, stats [6], the shares of
    the samples (below, inside, above) the range)."""
    h = h.detach().double().requires_grad_(True)
    P = [t.detach().double().requires_grad_(True) for t in (wa, ba, wv, bv)]
    logits = h[0] @ P[0].T + P[1]
    values = (h[1] @ P[2].T + P[3]).flatten()
    if mask is None:
        lp_all = torch.log_softmax(logits, -1)
        ent = -(lp_all.exp() * lp_all).sum(-1)
    else:
        S = mh.allowed_sets(mask, logits.shape[-1], act)
        lp_all = torch.log_softmax(logits.masked_fill(~S, float("-inf")), -1)
        lp_all = torch.where(S, lp_all, torch.zeros_like(lp_all))
        ent = -(torch.where(S, lp_all.exp(), torch.zeros_like(lp_all)) * lp_all).sum(-1)
    lp = lp_all.gather(1, act.long().view(-1, 1)).flatten()
    adv = adv.double()
    if norm:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(lp - olp.double())
    pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    lo, hi = clip_bounds(old, clip_vf)
    vd = values.detach()
    share = tuple(float(m.double().mean()) for m in (vd < lo, (vd >= lo) & (vd <= hi), vd > hi))
    vl = torch.nn.functional.mse_loss(ret.double(), torch.clamp(values, lo, hi))
    el = -ent.mean()
    loss = pl + ent_coef * el + vf_coef * vl
    loss.backward()
    lr = lp - olp.double()
    stats = torch.stack([pl, vl, el, loss, ((torch.exp(lr) - 1) - lr).mean(),
                         ((ratio - 1).abs() > clip).double().mean()]).detach()
    return h.grad, [p.grad for p in P], stats, share


def draw_old_values(h, wv, bv, rows, sel, c, seed):
    """Old values for a buffer of ``rows`` rows whose samples ``sel`` (their rows) fall,
    a third each, below, inside and above v +- c -- v the float64 value head on
    h[1]: old = v + c (1.25 .. 2.25) puts v below the range, old = v - the same
    above it, old = v + 0.8 c u (|u| <= 1) inside.  The margins (a quarter and a
    fifth of c) are far above the f32 value head's error, so the kernel and the
    restatement sort every sample alike."""
    g = torch.Generator().manual_seed(seed)
    v = (h[1].detach().double() @ wv.detach().double().T + bv.detach().double()).flatten().cpu()
    M = v.numel()
    kind = (torch.arange(M) + int(torch.randint(0, 3, (1,), generator=g))) % 3
    far = c * (1.25 + torch.rand(M, generator=g, dtype=torch.float64))
    near = 0.8 * c * (2 * torch.rand(M, generator=g, dtype=torch.float64) - 1)
    old_sel = v + torch.where(kind == 0, far, torch.where(kind == 2, -far, near))
    old = torch.randn(rows, generator=g, dtype=torch.float64)
    old[sel.cpu()] = old_sel
    return old.float().to(h.device).contiguous()


# ------------------------------------------------------------------ the gate
def gate_rule(stop, kl, threshold, err):
    """vn_kl_gate (include/voxnav.h): -> (ran, stop after, skip).  ``err``: None for NULL."""
    ran = int(stop == 0)
    if stop == 0 and kl > threshold:          # strict; False for a NaN
        stop = 1
    return ran, stop, int(stop != 0 or (err is not None and err != 0))


# ------------------------------------------------------------------ train()
class _Flat:
    """The env-major flattened rollout of oracle/ppo_oracle.train (``swap_and_flatten``), and
    its minibatches the way sb3_contrib cuts them: sequences, padding, the stored states at
    the sequence starts."""

    def __init__(self, buf, recurrent):
        self.recurrent = recurrent
        T, N = buf["actions"].shape
        self.T, self.N, self.total = T, N, T * N
        self.a = {k: po.swap_and_flatten(np.asarray(buf[k], np.float64)) for k in
                  ("obs", "actions", "episode_starts", "values", "log_probs", "advantages", "returns")}
        if recurrent:
            self.hs = {b: po.swap_and_flatten(np.asarray(buf["lstm_h"], np.float64)[:, b]) for b in (0, 1)}
            self.cs = {b: po.swap_and_flatten(np.asarray(buf["lstm_c"], np.float64)[:, b]) for b in (0, 1)}
            env_change = np.zeros((T, N))
            env_change[0, :] = 1.0
            self.env_change = po.swap_and_flatten(env_change).reshape(-1)

    def minibatch(self, params, bi):
        """evaluate_actions on rows ``bi`` -> dict(values, log_prob, entropy, mask, old_lp, adv, ret, old_v)."""
        a = self.a
        if self.recurrent:
            st, en = po.create_sequencers(a["episode_starts"][bi].reshape(-1), self.env_change[bi])
            n_seq = len(st)
            PF = lambda x: torch.tensor(po.pad_and_flatten(st, en, x.reshape(-1)))  # noqa: E731
            obs = torch.tensor(po.pad(st, en, a["obs"][bi]).reshape(-1, a["obs"].shape[-1]))
            starts = PF(a["episode_starts"][bi])
            mask = PF(np.ones(len(bi))) > 1e-8
            lstm = tuple((torch.tensor(self.hs[b][bi][st]), torch.tensor(self.cs[b][bi][st])) for b in (0, 1))
        else:
            n_seq, starts, lstm = None, None, None
            PF = lambda x: torch.tensor(x.reshape(-1))  # noqa: E731
            obs = torch.tensor(a["obs"][bi])
            mask = torch.ones(len(bi), dtype=torch.bool)
        values, log_prob, entropy = po.evaluate_actions(params, obs, PF(a["actions"][bi]).long(), lstm, starts, n_seq)
        return dict(values=values, log_prob=log_prob, entropy=entropy, mask=mask, old_lp=PF(a["log_probs"][bi]),
                    adv=PF(a["advantages"][bi]), ret=PF(a["returns"][bi]), old_v=PF(a["values"][bi]))


def own_log_probs(weights, buf):
    """[T, N] f32: the log-probs of the buffer's actions under ``weights`` (float64, the whole
    buffer as one minibatch from the stored states) -- a buffer carrying them is one the policy
    itself collected: the first minibatch's ratio is 1 and its approximate KL 0."""
    w = {k: torch.tensor(np.asarray(v), dtype=po.F64) for k, v in weights.items()}
    fl = _Flat(buf, "lstm_actor.weight_ih_l0" in w)
    with torch.no_grad():
        m = fl.minibatch(w, np.arange(fl.total))
    return m["log_prob"][m["mask"]].numpy().reshape(fl.N, fl.T).T.astype(np.float32).copy()


def train_reference(weights, buf, epoch_orders, *, learning_rate=3e-4, batch_size=64, clip_range=0.2,
                    clip_range_vf=None, target_kl=None, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, adam=None):
    """oracle/ppo_oracle.train's loop (its sequencers, padded LSTM re-run,
    written-out clip and Adam) in float64 with what sb3's PPO.train /
    RecurrentPPO.train add for ``clip_range_vf`` (values_pred = old +
    clamp(v - old, -c, c)) and ``target_kl`` (after the losses and before the
    step: approx_kl > 1.5 target_kl ends the passes; the minibatch is logged).
    ``learning_rate`` is this call's (``adam.lr`` is set to it).
    -> (weights, the logged minibatches' stats, adam, dict(early_stop,
    epochs_run, n_steps))."""
    w = {k: torch.tensor(np.asarray(v), dtype=po.F64) for k, v in weights.items()}
    fl = _Flat(buf, "lstm_actor.weight_ih_l0" in w)
    names = list(w.keys())
    adam = adam or po.Adam(names, learning_rate)
    adam.lr = learning_rate
    stats, info = [], dict(early_stop=False, epochs_run=0, n_steps=0)
    for order in epoch_orders:
        if fl.recurrent:
            split = int(order)
            indices = np.concatenate((np.arange(fl.total)[split:], np.arange(fl.total)[:split]))
        else:
            indices = np.asarray(order)
        info["epochs_run"] += 1
        for start in range(0, fl.total, batch_size):
            params = {k: v.clone().requires_grad_(True) for k, v in w.items()}
            m = fl.minibatch(params, indices[start:start + batch_size])
            mask, adv, values, log_ratio = m["mask"], m["adv"], m["values"], m["log_prob"] - m["old_lp"]
            if fl.recurrent or len(adv) > 1:
                adv = (adv - adv[mask].mean()) / (adv[mask].std() + 1e-8)
            ratio = torch.exp(log_ratio)
            policy_loss = -torch.mean(torch.min(adv * ratio,
                                                adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range))[mask])
            if clip_range_vf is not None:
                values = m["old_v"] + torch.clamp(values - m["old_v"], -clip_range_vf, clip_range_vf)
            value_loss = torch.mean(((m["ret"] - values) ** 2)[mask])
            entropy_loss = -torch.mean(m["entropy"][mask])
            loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
            with torch.no_grad():
                approx_kl = float(torch.mean(((torch.exp(log_ratio) - 1) - log_ratio)[mask]))
                clip_frac = float(torch.mean((torch.abs(ratio - 1) > clip_range).double()[mask]))
            grads = torch.autograd.grad(loss, [params[k] for k in names], allow_unused=True)
            grads = {k: (g if g is not None else torch.zeros_like(w[k])) for k, g in zip(names, grads)}
            grads, gnorm = po.clip_grad_norm(grads, max_grad_norm)
            stats.append(dict(policy_loss=float(policy_loss.detach()), value_loss=float(value_loss.detach()),
                              entropy_loss=float(entropy_loss.detach()), loss=float(loss.detach()),
                              approx_kl=approx_kl, clip_fraction=clip_frac, grad_norm=gnorm))
            if target_kl is not None and approx_kl > 1.5 * target_kl:
                info["early_stop"] = True
                break
            adam.step(w, grads)
            info["n_steps"] += 1
        if info["early_stop"]:
            break
    return {k: v.numpy() for k, v in w.items()}, stats, adam, info


def crossing(kls, first=1):
    """(k, target_kl) for a dry run's per-minibatch approximate KLs: the minibatch k >= ``first``
    whose KL stands furthest (as a ratio) above the largest one before it, and the target_kl
    whose threshold 1.5 target_kl is the geometric mean of the two -- so a run with it stops at
    k, by a margin far above the f32 learner's error in a KL."""
    kls = [max(float(x), 0.0) for x in kls]
    best, k = 0.0, None
    for i in range(max(first, 1), len(kls)):
        before = max(max(kls[:i]), 1e-300)
        if kls[i] / before > best:
            best, k = kls[i] / before, i
    assert k is not None and best > 1.05, ("no minibatch stands clear above the ones before it", kls)
    return k, float(np.sqrt(kls[k] * max(max(kls[:k]), kls[k] / 1e4))) / 1.5


def assert_logged_means(st, rows):
    """A learner's ``train()`` dict against the means of the restatement's logged rows
    (test_ppo._run_parity's keys and bound)."""
    for key, okey in (("policy_gradient_loss", "policy_loss"), ("value_loss", "value_loss"),
                      ("entropy_loss", "entropy_loss"), ("approx_kl", "approx_kl"),
                      ("clip_fraction", "clip_fraction")):
        ref = np.mean([s[okey] for s in rows])
        assert abs(st[key] - ref) <= 1e-4 * max(1.0, abs(ref)), (key, st[key], ref)
