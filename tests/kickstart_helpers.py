"""Float64 restatements for kickstarted PPO (voxnav.imitate.KickstartLearner,
csrc/voxnav_ppo_bc_loss.hip) -- TEST INFRASTRUCTURE ONLY; the product paths are the HIP kernel and
voxnav.imitate's torch path.

* ``kickstart_terms``: the loss of include/voxnav.h (vn_ppo_bc_loss / vn_ppo_bc_loss_set) from
  logits and values: sb3's PPO terms as oracle/ppo_oracle.py's ``train`` writes them, plus bc_coef
  times the cross-entropy of ``bc_helpers.bc_terms`` / ``bc_set_helpers.bc_set_terms``;
* ``kickstart_heads64``: that loss from the latents on, with its gradients by float64 autograd;
* ``kickstart_train``: one ``KickstartLearner.train`` call, minibatches and sequences cut with
  oracle/ppo_oracle.py's own functions, as ``bc_helpers.bc_train`` does;
* ``case``: heads, latents and buffers by ``test_ppo_loss_grid_gpu._case``'s recipe (old log-probs
  around the true ones, so the ratio falls on both sides of the clip range and inside it), with
  labels, weights and sets as ``bc_helpers`` / ``bc_set_helpers`` build them.
"""
from __future__ import annotations

import numpy as np
import torch

import bc_helpers as bh
import bc_set_helpers as bs
from oracle import ppo_oracle as po

F64 = torch.float64
PPO_KEYS = ("policy_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction")
STAT_KEYS = PPO_KEYS + ("bc_loss", "accuracy", "labelled")


def kickstart_terms(logits, values, actions, adv, old_lp, returns, labels, weight, clip, ent_coef, vf_coef, bc_coef,
                    norm, sets=False, mask=None):
    """-> dict of 0-d tensors under STAT_KEYS.  ``labels``: int labels, or uint8 sets with
    ``sets``; ``weight`` None: every sample labelled; ``mask``: the unpadded positions."""
    M = logits.shape[0]
    mask = torch.ones(M, dtype=torch.bool) if mask is None else mask
    lp_all = torch.log_softmax(logits, dim=-1)
    log_prob = lp_all.gather(1, actions.view(-1, 1).long()).flatten()
    entropy = -(lp_all.exp() * lp_all).sum(-1)
    if norm:
        adv = (adv - adv[mask].mean()) / (adv[mask].std() + 1e-8)
    ratio = torch.exp(log_prob - old_lp)
    l1 = adv * ratio
    l2 = adv * torch.clamp(ratio, 1 - clip, 1 + clip)
    pl = -torch.mean(torch.min(l1, l2)[mask])
    vl = torch.mean(((returns - values) ** 2)[mask])
    el = -torch.mean(entropy[mask])
    lr = (log_prob - old_lp).detach()
    kl = torch.mean(((torch.exp(lr) - 1) - lr)[mask])
    cf = torch.mean((torch.abs(ratio.detach() - 1) > clip).double()[mask])
    if sets:
        b = bs.bc_set_terms(logits, values, np.asarray(labels), weight, returns, 0.0, 0.0, mask=mask)
    else:
        b = bh.bc_terms(logits, values, torch.as_tensor(labels), weight, returns, 0.0, 0.0, mask=mask)
    ce = b["bc_loss"]
    loss = pl + ent_coef * el + vf_coef * vl + bc_coef * ce
    return dict(policy_loss=pl, value_loss=vl, entropy_loss=el, loss=loss, approx_kl=kl, clip_fraction=cf,
                bc_loss=ce, accuracy=b["accuracy"], labelled=b["labelled"])


def ppo_terms(logits, values, actions, adv, old_lp, returns, clip, ent_coef, vf_coef, norm):
    """The PPO restatement alone (tests/ppo_loss_helpers.py's formula on logits and values)."""
    lp_all = torch.log_softmax(logits, dim=-1)
    lp = lp_all.gather(1, actions.view(-1, 1).long()).flatten()
    ent = -(lp_all.exp() * lp_all).sum(-1)
    if norm:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(lp - old_lp)
    pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    vl = torch.nn.functional.mse_loss(returns, values)
    el = -ent.mean()
    return dict(policy_loss=pl, value_loss=vl, entropy_loss=el, loss=pl + ent_coef * el + vf_coef * vl)


def kickstart_heads64(hp, hv, wa, ba, wv, bv, actions, adv, old_lp, returns, labels, weight, clip, ent_coef, vf_coef,
                      bc_coef, norm, sets=False):
    """The loss from the latents hp, hv [M, F] on, in float64, and its gradients by autograd.
    -> (dh [2, M, F], (dwa, dba, dwv, dbv), stats [9]) as float64 torch tensors."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    c = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    hp, hv, wa, ba, wv, bv = (t(a) for a in (hp, hv, wa, ba, wv, bv))
    logits = hp @ wa.reshape(-1, hp.shape[1]).T + ba
    values = hv @ wv.reshape(-1) + bv.reshape(())
    r = kickstart_terms(logits, values, torch.as_tensor(np.asarray(actions)), c(adv), c(old_lp), c(returns),
                        np.asarray(labels), None if weight is None else np.asarray(weight), clip, ent_coef, vf_coef,
                        bc_coef, norm, sets=sets)
    g = torch.autograd.grad(r["loss"], [hp, hv, wa, ba, wv, bv], allow_unused=True)
    g = [torch.zeros_like(x) if y is None else y for x, y in zip((hp, hv, wa, ba, wv, bv), g)]
    stats = torch.stack([r[k].detach().double() for k in STAT_KEYS])
    return torch.stack([g[0], g[1]]), tuple(g[2:]), stats


def kickstart_train(weights, buf, epoch_orders, *, learning_rate=3e-4, batch_size=64, clip_range=0.2, ent_coef=0.01,
                    vf_coef=0.5, max_grad_norm=0.5, normalize_advantage=True, bc_coef=1.0, sets=False):
    """One ``KickstartLearner.train`` call in float64.  ``buf``: ppo_oracle.train's arrays plus
    ``expert_actions`` (or ``expert_set`` with ``sets``) and ``label_weight`` [T, N] (or absent: all
    labelled).  -> (new weights, per-minibatch stats)."""
    w = {k: torch.tensor(np.asarray(v), dtype=F64) for k, v in weights.items()}
    recurrent = "lstm_actor.weight_ih_l0" in w
    T, N = buf["actions"].shape
    total = T * N
    lw = buf.get("label_weight")
    arrays = dict(obs=buf["obs"], actions=buf["actions"], episode_starts=buf["episode_starts"],
                  log_probs=buf["log_probs"], advantages=buf["advantages"], returns=buf["returns"],
                  labels=buf["expert_set"] if sets else buf["expert_actions"], lw=np.ones((T, N)) if lw is None else lw)
    flat = {k: po.swap_and_flatten(np.asarray(v, np.float64)) for k, v in arrays.items()}
    if recurrent:
        hs = {b: po.swap_and_flatten(np.asarray(buf["lstm_h"], np.float64)[:, b]) for b in (0, 1)}
        cs = {b: po.swap_and_flatten(np.asarray(buf["lstm_c"], np.float64)[:, b]) for b in (0, 1)}
        env_change = np.zeros((T, N))
        env_change[0, :] = 1.0
        env_change = po.swap_and_flatten(env_change).reshape(-1)
    names = list(w.keys())
    adam = po.Adam(names, learning_rate)
    A = w["action_net.weight"].shape[0]
    keys = ("actions", "log_probs", "advantages", "returns", "labels", "lw")
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
                acts, olp, adv, ret, labels, lwt = (PF(flat[k][bi]) for k in keys)
                starts = PF(flat["episode_starts"][bi])
                mask = PF(np.ones(len(bi))) > 1e-8
                lstm = tuple((torch.tensor(hs[b][bi][st]), torch.tensor(cs[b][bi][st])) for b in (0, 1))
            else:
                n_seq = None
                obs = torch.tensor(flat["obs"][bi])
                acts, olp, adv, ret, labels, lwt = (torch.tensor(flat[k][bi].reshape(-1)) for k in keys)
                starts, lstm, mask = None, None, torch.ones(len(bi), dtype=torch.bool)
            params = {k: v.clone().requires_grad_(True) for k, v in w.items()}
            acts, labels = acts.long(), labels.long()
            # log-probs of every action: the logits up to a per-row shift (bc_helpers.bc_train)
            rows = [po.evaluate_actions(params, obs, torch.full_like(acts, j), lstm, starts, n_seq) for j in range(A)]
            values = rows[0][0]
            lp_all = torch.stack([r[1] for r in rows], dim=1)
            norm = normalize_advantage and (recurrent or len(bi) > 1)
            r = kickstart_terms(lp_all, values, acts, adv, olp, ret, labels.numpy() if sets else labels, lwt.numpy(),
                                clip_range, ent_coef, vf_coef, bc_coef, norm, sets=sets, mask=mask)
            grads = torch.autograd.grad(r["loss"], [params[k] for k in names], allow_unused=True)
            grads = {k: (g if g is not None else torch.zeros_like(w[k])) for k, g in zip(names, grads)}
            grads, gnorm = po.clip_grad_norm(grads, max_grad_norm)
            adam.step(w, grads)
            stats.append(dict({k: float(v.detach()) for k, v in r.items()}, grad_norm=gnorm, n_seq=n_seq or 0))
    return {k: v.numpy() for k, v in w.items()}, stats


# ------------------------------------------------------------------ kernel cases (any device)
def case(M, F, A, gather, device, seed=0, logit_span=None, weights="random", sets=False, zero_adv=False):
    """Heads, latents and rollout buffers by test_ppo_loss_grid_gpu._case's recipe, plus labels
    (int32, uniform as bc_helpers.dagger_arrays draws them, or uint8 sets by
    ``bc_set_helpers.random_sets``: 30 % empty) and weights (None; "random": ~20 % zero, as
    bc_helpers.dagger_arrays; "zero": none labelled inside the minibatch)."""
    torch.manual_seed(1000 * M + 10 * F + A + seed)
    an, vn = torch.nn.Linear(F, A).to(device), torch.nn.Linear(F, 1).to(device)
    h = torch.tanh(torch.randn((2, M, F), device=device))
    if logit_span is not None and A > 1:
        with torch.no_grad():
            z = h[0] @ an.weight.T + an.bias
            k = 2 * logit_span / (z.max(-1).values - z.min(-1).values).max()
            an.weight.mul_(k)
            an.bias.mul_(k)
    R = M + 1000 if gather else M
    src = torch.randperm(R, device=device)[:M].contiguous() if gather else None
    act = torch.randint(0, A, (R,), device=device, dtype=torch.int32)
    adv = torch.zeros(R, device=device) if zero_adv else torch.randn(R, device=device) * 3 + 0.5
    ret = torch.randn(R, device=device)
    with torch.no_grad():
        lp_true = torch.log_softmax(h[0] @ an.weight.T + an.bias, -1)
    sel = src if gather else torch.arange(M, device=device)
    olp = torch.randn(R, device=device) - 1.5
    olp[sel] = lp_true.gather(1, act[sel].long().view(-1, 1)).flatten() + 0.3 * torch.randn(M, device=device)
    rng = np.random.default_rng(1000 * M + 10 * F + A + seed)
    if sets:
        lab = torch.as_tensor(bs.random_sets(rng, (R,), A), device=device)
    else:
        lab = torch.as_tensor(rng.integers(0, A, R).astype(np.int32), device=device)
    if weights is None:
        wgt = None
    elif weights == "random":
        wgt = torch.as_tensor((rng.random(R) >= 0.2).astype(np.uint8), device=device)
    else:
        wgt = torch.ones(R, dtype=torch.uint8, device=device)     # rows outside the minibatch do not count
        wgt[sel] = 0
    c = dict(M=M, F=F, A=A, an=an, vn=vn, h=h, src=src, act=act, adv=adv, olp=olp, ret=ret, lab=lab, wgt=wgt,
             sets=sets)
    if weights != "zero":
        # a small minibatch may draw few labelled samples: label its first unlabelled rows (a
        # singleton set, weight 1) until at least half are, so that no case compares an
        # unlabelled batch only; this only lowers the share of empty sets
        un = [int(r) for r, l in zip(sel.tolist(), _labelled_rows(c).tolist()) if not l]
        for r in un[:max(0, -(-M // 2) - (M - len(un)))]:
            if sets:
                lab[r] = 1 << int(act[r])
            if wgt is not None:
                wgt[r] = 1
    return c


def _labelled_rows(c):
    g = lambda t: t if c["src"] is None else t[c["src"]]  # noqa: E731
    w = torch.ones(c["M"], dtype=torch.bool, device=c["h"].device) if c["wgt"] is None else g(c["wgt"]) != 0
    if c["sets"]:
        w = w & ((g(c["lab"]).long() & ((1 << c["A"]) - 1)) != 0)
    return w


def labelled_share(c):
    """The labelled share of the case's minibatch, from its labels and weights alone."""
    return float(_labelled_rows(c).double().mean())


def reference(c, clip, ent_coef, vf_coef, bc_coef, norm):
    """``kickstart_heads64`` on a case."""
    n = lambda t: t.detach().cpu().numpy()  # noqa: E731
    g = lambda t: None if t is None else n(t if c["src"] is None else t[c["src"]])  # noqa: E731
    an, vn = c["an"], c["vn"]
    return kickstart_heads64(n(c["h"][0]), n(c["h"][1]), n(an.weight), n(an.bias), n(vn.weight), n(vn.bias),
                             g(c["act"]), g(c["adv"]), g(c["olp"]), g(c["ret"]), g(c["lab"]), g(c["wgt"]), clip,
                             ent_coef, vf_coef, bc_coef, norm, sets=c["sets"])


# ------------------------------------------------------------------ learner parity (CPU and GPU)
def kickstart_buffer(b, device, sets):
    buf = bs.set_buffer(b, device) if sets else bh.as_dagger_buffer(b, device)
    buf.took_expert = torch.zeros(b["actions"].shape, dtype=torch.uint8, device=device)
    return buf


def run_kickstart_parity(device, recurrent, sets, T=12, N=5, batch_size=16, epochs=2, arch=(32, 16), lstm=16,
                         p_start=0.15, bc_coef=0.7, atol=2e-5, rtol=1e-4):
    """``KickstartLearner.train`` on ``device`` against ``kickstart_train``, within the bounds
    ``bc_helpers.run_bc_parity`` holds ``BCLearner`` to: parameters within atol + rtol |ref|,
    logged values within 1e-4 relative.  -> (learner, restatement stats)."""
    from voxnav.imitate import KickstartLearner
    from voxnav.policy import numpy_weights
    pol = bh.small_policy(recurrent, arch, lstm).to(device)
    w0 = numpy_weights(pol)
    b = bh.dagger_arrays(T, N, lstm, recurrent, p_start=p_start)
    if sets:
        b["expert_set"] = bs.random_sets(np.random.default_rng(11), (T, N), 6)
    rng = np.random.default_rng(7)
    orders = ([int(rng.integers(T * N)) for _ in range(epochs)] if recurrent
              else [rng.permutation(T * N) for _ in range(epochs)])
    ln = KickstartLearner(pol, n_epochs=epochs, batch_size=batch_size, bc_coef=bc_coef,
                          labels="set" if sets else "action")
    st = ln.train(kickstart_buffer(b, device, sets), epoch_orders=orders)
    w1, ost = kickstart_train(w0, b, orders, batch_size=batch_size, bc_coef=bc_coef, sets=sets)
    got = numpy_weights(pol)
    moved = 0.0
    for k in w1:
        np.testing.assert_allclose(got[k], w1[k], atol=atol, rtol=rtol, err_msg=k)
        moved = max(moved, float(np.abs(w1[k] - w0[k]).max()))
    assert moved > 1e-4                                 # the update did something
    n = len(ost)
    assert st["n_minibatches"] == n == epochs * -(-T * N // batch_size)
    assert st["n_updates"] == n
    names = dict(policy_loss="policy_gradient_loss")
    for key in STAT_KEYS + ("grad_norm",):
        ref = float(np.mean([s[key] for s in ost]))
        val = st[names.get(key, key)]
        print(f"{key}: learner {val!r} restatement {ref!r}")
        assert abs(val - ref) <= 1e-4 * max(1.0, abs(ref)), (key, val, ref)
    if recurrent and batch_size < T * N:
        assert sum(s["n_seq"] for s in ost) > n        # sequences were actually split
    assert 0.3 < np.mean([s["labelled"] for s in ost]) < 1.0
    return ln, ost
