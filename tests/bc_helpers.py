"""Float64 restatements for the DAgger warm start (voxnav.imitate, csrc/voxnav_bc_loss.hip) -- TEST
INFRASTRUCTURE ONLY; the product paths are the HIP kernels and voxnav.imitate's torch path.

* ``bc_terms``: the behaviour-cloning loss of include/voxnav.h (vn_bc_loss) from logits and values;
* ``bc_heads64``: that loss from the latents on, with its gradients by float64 autograd;
* ``bc_train``: one ``BCLearner.train`` call, minibatches and sequences cut as oracle/ppo_oracle.py
  cuts them (its sequencers, ``evaluate_actions``, ``Adam`` and ``clip_grad_norm``);
* ``mix``: the rule of vn_dagger_mix from ``helpers.philox_uniform``.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from helpers import philox_uniform
from oracle import ppo_oracle as po

F64 = torch.float64


def bc_terms(logits, values, labels, weight, returns, ent_coef, vf_coef, mask=None):
    """-> dict of 0-d tensors: bc_loss, value_loss, entropy_loss, loss, accuracy, labelled.
    ``weight`` None: every sample labelled.  ``mask``: the unpadded positions (None: all)."""
    M = logits.shape[0]
    mask = torch.ones(M, dtype=torch.bool) if mask is None else mask
    m = mask.to(logits.dtype)
    w = m.clone() if weight is None else (torch.as_tensor(weight) != 0).to(logits.dtype) * m
    count = m.sum()
    lp_all = torch.log_softmax(logits, dim=-1)
    p = lp_all.exp()
    H = -(p * lp_all).sum(-1)
    lp = lp_all.gather(1, labels.view(-1, 1).long()).flatten()
    n = w.sum()
    den = torch.clamp(n, min=1.0)
    ce = (w * -lp).sum() / den
    el = -(m * H).sum() / count
    vl = (m * (returns - values) ** 2).sum() / count
    A = logits.shape[1]
    amax = torch.full((M,), A, dtype=torch.int64)
    top = logits.max(-1).values
    for j in reversed(range(A)):                         # ties: the lowest index wins
        amax = torch.where(logits[:, j] == top, torch.full_like(amax, j), amax)
    acc = (w * (amax == labels.long()).to(logits.dtype)).sum() / den
    return dict(bc_loss=ce, value_loss=vl, entropy_loss=el, loss=ce + ent_coef * el + vf_coef * vl,
                accuracy=acc.detach(), labelled=(n / count).detach())


def bc_heads64(hp, hv, wa, ba, wv, bv, labels, weight, returns, ent_coef, vf_coef):
    """The loss from the latents hp, hv [M, F] on, in float64, and its gradients by autograd.
    -> (dhp, dhv, (dwa, dba, dwv, dbv), stats [6]) as numpy float64."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    hp, hv, wa, ba, wv, bv = (t(a) for a in (hp, hv, wa, ba, wv, bv))
    logits = hp @ wa.T + ba
    values = hv @ wv.reshape(-1) + bv.reshape(())
    r = bc_terms(logits, values, torch.as_tensor(np.asarray(labels)), None if weight is None else np.asarray(weight),
                 torch.tensor(np.asarray(returns, np.float64)), ent_coef, vf_coef)
    g = torch.autograd.grad(r["loss"], [hp, hv, wa, ba, wv, bv], allow_unused=True)
    g = [np.zeros(tuple(x.shape)) if y is None else y.numpy() for x, y in zip((hp, hv, wa, ba, wv, bv), g)]
    stats = np.array([float(r[k].detach()) for k in ("bc_loss", "value_loss", "entropy_loss", "loss", "accuracy", "labelled")])
    return g[0], g[1], tuple(g[2:]), stats


def bc_train(weights, buf, epoch_orders, *, learning_rate=3e-4, batch_size=64, ent_coef=0.0, vf_coef=0.5,
             max_grad_norm=0.5):
    """One ``BCLearner.train`` call in float64.  ``buf``: ppo_oracle.train's arrays plus
    ``expert_actions`` [T, N] and ``label_weight`` [T, N] (or absent: all labelled).
    -> (new weights, per-minibatch stats)."""
    w = {k: torch.tensor(np.asarray(v), dtype=F64) for k, v in weights.items()}
    recurrent = "lstm_actor.weight_ih_l0" in w
    T, N = buf["actions"].shape
    total = T * N
    lw = buf.get("label_weight")
    arrays = dict(obs=buf["obs"], episode_starts=buf["episode_starts"], returns=buf["returns"],
                  labels=buf["expert_actions"], lw=np.ones((T, N)) if lw is None else lw)
    flat = {k: po.swap_and_flatten(np.asarray(v, np.float64)) for k, v in arrays.items()}
    if recurrent:
        hs = {b: po.swap_and_flatten(np.asarray(buf["lstm_h"], np.float64)[:, b]) for b in (0, 1)}
        cs = {b: po.swap_and_flatten(np.asarray(buf["lstm_c"], np.float64)[:, b]) for b in (0, 1)}
        env_change = np.zeros((T, N))
        env_change[0, :] = 1.0
        env_change = po.swap_and_flatten(env_change).reshape(-1)
    names = list(w.keys())
    adam = po.Adam(names, learning_rate)
    stats = []
    for order in epoch_orders:
        if recurrent:
            split = int(order)
            indices = np.concatenate((np.arange(total)[split:], np.arange(total)[:split]))
        else:
            indices = np.asarray(order)
        for start in range(0, total, batch_size):
            bi = indices[start:start + batch_size]
            if recurrent:
                st, en = po.create_sequencers(flat["episode_starts"][bi].reshape(-1), env_change[bi])
                n_seq = len(st)
                PF = lambda a: torch.tensor(po.pad_and_flatten(st, en, a.reshape(-1)))  # noqa: E731
                obs = torch.tensor(po.pad(st, en, flat["obs"][bi]).reshape(-1, flat["obs"].shape[-1]))
                labels, lwt, ret, starts = (PF(flat[k][bi]) for k in ("labels", "lw", "returns", "episode_starts"))
                mask = PF(np.ones(len(bi))) > 1e-8
                lstm = tuple((torch.tensor(hs[b][bi][st]), torch.tensor(cs[b][bi][st])) for b in (0, 1))
            else:
                n_seq = None
                obs = torch.tensor(flat["obs"][bi])
                labels, lwt, ret = (torch.tensor(flat[k][bi].reshape(-1)) for k in ("labels", "lw", "returns"))
                starts, lstm, mask = None, None, torch.ones(len(bi), dtype=torch.bool)
            params = {k: v.clone().requires_grad_(True) for k, v in w.items()}
            labels = labels.long()
            # the logits: evaluate_actions gives log-probs, values and entropy; the argmax needs the
            # logits themselves, which the log-softmax over all actions keeps up to a per-row shift
            rows = [po.evaluate_actions(params, obs, torch.full_like(labels, j), lstm, starts, n_seq) for j in
                    range(w["action_net.weight"].shape[0])]
            values = rows[0][0]
            lp_all = torch.stack([r[1] for r in rows], dim=1)
            r = bc_terms(lp_all, values, labels, lwt.numpy(), ret, ent_coef, vf_coef, mask=mask)
            grads = torch.autograd.grad(r["loss"], [params[k] for k in names], allow_unused=True)
            grads = {k: (g if g is not None else torch.zeros_like(w[k])) for k, g in zip(names, grads)}
            grads, gnorm = po.clip_grad_norm(grads, max_grad_norm)
            adam.step(w, grads)
            stats.append(dict({k: float(v.detach()) for k, v in r.items()}, grad_norm=gnorm, n_seq=n_seq or 0))
    return {k: v.numpy() for k, v in w.items()}, stats


def mix(policy, expert, dist, beta, mix_seed, gids, t):
    """vn_dagger_mix's rule -> (executed, took_expert, label_weight)."""
    thr = math.floor(float(beta) * 2 ** 24)
    u24 = np.rint(philox_uniform(mix_seed, gids, t) * 2 ** 24).astype(np.int64)     # exact: u = u24 / 2^24
    lab = np.asarray(dist) != -1
    took = lab & (u24 < thr)
    return np.where(took, expert, policy).astype(np.int32), took.astype(np.uint8), lab.astype(np.uint8)


# ------------------------------------------------------------------ learner parity (CPU and GPU)
def small_policy(recurrent, arch=(32, 16), lstm=16, seed=0):
    from voxnav.policy import ActorCriticPolicy, RecurrentActorCriticPolicy
    torch.manual_seed(seed)
    net = dict(pi=list(arch), vf=list(arch))
    if recurrent:
        return RecurrentActorCriticPolicy(obs_dim=80, lstm_hidden_size=lstm, net_arch=net)
    return ActorCriticPolicy(obs_dim=80, net_arch=net)


def dagger_arrays(T, N, H, recurrent, seed=1, p_start=0.15, p_unlabelled=0.2):
    """A DaggerBuffer-shaped synthetic buffer as numpy arrays ([T, N]-major): tests/test_ppo.py's
    fields plus expert_actions and label_weight (zero with probability ``p_unlabelled``)."""
    rng = np.random.default_rng(seed)
    b = dict(
        obs=rng.random((T, N, 80), dtype=np.float32),
        actions=rng.integers(0, 6, (T, N)).astype(np.int32),
        episode_starts=(rng.random((T, N)) < p_start).astype(np.float32),
        values=rng.normal(0, 1, (T, N)).astype(np.float32),
        log_probs=(np.log(1 / 6) + rng.normal(0, 0.15, (T, N))).astype(np.float32),
        advantages=rng.normal(0, 2, (T, N)).astype(np.float32),
        returns=rng.normal(0, 2, (T, N)).astype(np.float32),
        expert_actions=rng.integers(0, 6, (T, N)).astype(np.int32),
        label_weight=(rng.random((T, N)) >= p_unlabelled).astype(np.uint8),
    )
    b["episode_starts"][0, :2] = 1.0
    if recurrent:
        b["lstm_h"] = rng.normal(0, 0.3, (T, 2, N, H)).astype(np.float32)
        b["lstm_c"] = rng.normal(0, 0.3, (T, 2, N, H)).astype(np.float32)
    return b


def as_dagger_buffer(b, device):
    from voxnav.imitate import DaggerBuffer
    t = {k: torch.as_tensor(v, device=device) for k, v in b.items()}
    return DaggerBuffer(obs=t["obs"], actions=t["actions"], rewards=torch.zeros_like(t["values"]),
                        episode_starts=t["episode_starts"], values=t["values"], log_probs=t["log_probs"],
                        advantages=t["advantages"], returns=t["returns"], lstm_h=t.get("lstm_h"),
                        lstm_c=t.get("lstm_c"), expert_actions=t["expert_actions"], label_weight=t.get("label_weight"),
                        took_expert=None, policy_actions=t["actions"])


STAT_KEYS = ("bc_loss", "value_loss", "entropy_loss", "loss", "accuracy", "labelled")


def run_bc_parity(device, recurrent, T=12, N=5, batch_size=16, epochs=2, arch=(32, 16), lstm=16, p_start=0.15,
                  ent_coef=0.0, atol=2e-5, rtol=1e-4):
    """``BCLearner.train`` on ``device`` against ``bc_train``: parameters within atol + rtol |ref|
    (tests/test_ppo.py's bounds for the PPO learner against its oracle: the learner runs in f32, a
    few Adam steps of lr 3e-4 move parameters by ~1e-3), logged values within 1e-4 relative.
    -> (learner, oracle stats)."""
    from voxnav.imitate import BCLearner
    from voxnav.policy import numpy_weights
    pol = small_policy(recurrent, arch, lstm).to(device)
    w0 = numpy_weights(pol)
    b = dagger_arrays(T, N, lstm, recurrent, p_start=p_start)
    rng = np.random.default_rng(7)
    orders = ([int(rng.integers(T * N)) for _ in range(epochs)] if recurrent
              else [rng.permutation(T * N) for _ in range(epochs)])
    ln = BCLearner(pol, n_epochs=epochs, batch_size=batch_size, ent_coef=ent_coef)
    st = ln.train(as_dagger_buffer(b, device), epoch_orders=orders)
    w1, ost = bc_train(w0, b, orders, batch_size=batch_size, ent_coef=ent_coef)
    got = numpy_weights(pol)
    moved = 0.0
    for k in w1:
        np.testing.assert_allclose(got[k], w1[k], atol=atol, rtol=rtol, err_msg=k)
        moved = max(moved, float(np.abs(w1[k] - w0[k]).max()))
    assert moved > 1e-4                                 # the update did something
    n = len(ost)
    assert st["n_minibatches"] == n == epochs * -(-T * N // batch_size)
    assert st["n_updates"] == n
    for key in STAT_KEYS + ("grad_norm",):
        ref = float(np.mean([s[key] for s in ost]))
        print(f"{key}: learner {st[key]!r} restatement {ref!r}")
        assert abs(st[key] - ref) <= 1e-4 * max(1.0, abs(ref)), (key, st[key], ref)
    if recurrent and batch_size < T * N:
        assert sum(s["n_seq"] for s in ost) > n        # sequences were actually split
    assert 0.5 < np.mean([s["labelled"] for s in ost]) < 1.0
    return ln, ost
