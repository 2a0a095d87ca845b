"""Float64 restatements of the distance-weighted behaviour-cloning losses and of best-set execution
(include/voxnav.h vn_bc_loss_soft, vn_ppo_bc_loss_soft, their masked forms, vn_dagger_mix_best) --
TEST INFRASTRUCTURE ONLY; the product paths are the HIP kernels and voxnav.imitate's torch path.

* ``soft_target``: P, q, ln q and the shortest actions of the rule, from the distance rows;
* ``bc_soft_terms`` / ``kickstart_soft_terms``: ``bc_helpers.bc_terms`` / ``kickstart_helpers.kickstart_terms``
  with KL(q || pi) in the cross-entropy's place; ``masks``: over the softmax restricted to S_i
  (``masked_imitate_helpers.support`` with P_i as the label's bits);
* ``bc_soft_heads64`` / ``kickstart_soft_heads64``: those from the latents on, gradients by float64 autograd;
* ``bc_soft_train`` / ``kickstart_soft_train``: ``bc_helpers.bc_train`` / ``kickstart_helpers.kickstart_train``
  (their minibatches, sequences, Adam and clip) with the soft terms; a sample's distance row rides through
  their gathers as its row number in the label's place (and the mask byte above it);
* ``mix_best``: the rule of vn_dagger_mix_best from ``helpers.philox_uniform``;
* ``random_dists``, ``run_soft_parity``: the inputs and the learner parity check of the tests.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import bc_helpers as bh
import kickstart_helpers as kh
import masked_imitate_helpers as mi
from helpers import philox_uniform

BC_KEYS = bh.STAT_KEYS
KS_KEYS = kh.STAT_KEYS
ROW = 1 << 16            # bc_soft_train's packing: row number + ROW * mask byte


def f32(tau):
    """The temperature as the C-ABI receives it (a float): the restatement's tau."""
    return float(np.float32(tau))


def soft_target(dists, A, tau):
    """dists [M, >= A] ints -> (P bool [M, A], q f64 [M, A], ln q (0 where q is 0), shortest bool [M, A]).
    Written row by row with Python's own floats and ``math``, on purpose unlike the product's
    vectorised torch path (voxnav.imitate._cross_entropy): the two share no expression."""
    rows = np.asarray(dists).astype(np.int64)[:, :A].tolist()
    M = len(rows)
    P, short = np.zeros((M, A), bool), np.zeros((M, A), bool)
    q, ln_q = np.zeros((M, A)), np.zeros((M, A))
    tau = float(tau)
    for i, row in enumerate(rows):
        reached = [k for k, d in enumerate(row) if d > 0]
        if not reached:
            continue
        dstar = min(row[k] for k in reached)
        w = {}
        for k in reached:
            delta = row[k] - dstar
            w[k] = 1.0 if delta == 0 else math.exp(-(delta / tau))
            P[i, k] = True
            short[i, k] = delta == 0
        z = math.fsum(w.values())
        for k in reached:
            q[i, k] = w[k] / z
            if q[i, k] > 0.0:
                ln_q[i, k] = -((row[k] - dstar) / tau) - math.log(z)
    return torch.as_tensor(P), torch.as_tensor(q), torch.as_tensor(ln_q), torch.as_tensor(short)


def p_bits(dists, A):
    """int64 [M]: bit k set where d_k > 0 (k < A): the label's bits of the masked forms."""
    P = torch.as_tensor(np.asarray(dists).astype(np.int64))[:, :A] > 0
    return (P.to(torch.int64) << torch.arange(A)).sum(-1)


def _argmax_low(logits):
    M, A = logits.shape
    amax = torch.full((M,), A, dtype=torch.int64)
    top = logits.max(-1).values
    for j in reversed(range(A)):                         # ties: the lowest index wins
        amax = torch.where(logits[:, j] == top, torch.full_like(amax, j), amax)
    return amax


def _kl(logits, dists, weight, tau, m):
    """-> (kl mean over the labelled, accuracy, labelled share) of the logits as they are."""
    M, A = logits.shape
    P, q, ln_q, short = soft_target(dists, A, tau)
    w = m.clone() if weight is None else (torch.as_tensor(np.asarray(weight)).reshape(-1) != 0).to(logits.dtype) * m
    w = w * P.any(-1).to(logits.dtype)
    lp_all = torch.log_softmax(logits, dim=-1)
    kl_i = torch.where(q > 0, q * (ln_q - lp_all), torch.zeros_like(q)).sum(-1)
    n = w.sum()
    den = torch.clamp(n, min=1.0)
    acc = (w * short.gather(1, _argmax_low(logits).view(-1, 1)).flatten().to(logits.dtype)).sum() / den
    return (w * kl_i).sum() / den, acc.detach(), (n / m.sum()).detach()


def bc_soft_terms(logits, values, dists, weight, returns, tau, ent_coef, vf_coef, masks=None, mask=None):
    """``bc_helpers.bc_terms`` with the distance-weighted target -> the same dict.  ``masks`` (the
    action-mask bytes, or None): everything over S_i = mask | P_i of a labelled sample, empty as full."""
    M, A = logits.shape
    mask = torch.ones(M, dtype=torch.bool) if mask is None else mask
    m = mask.to(logits.dtype)
    if masks is not None:
        logits = mi.restrict(logits, mi.support(masks, p_bits(dists, A), weight, A, True))
    lp_all = torch.log_softmax(logits, dim=-1)
    H = -(lp_all.exp() * lp_all).sum(-1)
    kl, acc, share = _kl(logits, dists, weight, tau, m)
    count = m.sum()
    el = -(m * H).sum() / count
    vl = (m * (returns - values) ** 2).sum() / count
    return dict(bc_loss=kl, value_loss=vl, entropy_loss=el, loss=kl + ent_coef * el + vf_coef * vl, accuracy=acc,
                labelled=share)


def kickstart_soft_terms(logits, values, actions, adv, old_lp, returns, dists, weight, tau, clip, ent_coef, vf_coef,
                         bc_coef, norm, masks=None, mask=None):
    """``kickstart_helpers.kickstart_terms`` with the distance-weighted target -> the same dict.
    ``masks``: over S_i = mask | taken action | P_i of a labelled sample."""
    M, A = logits.shape
    mask = torch.ones(M, dtype=torch.bool) if mask is None else mask
    if masks is not None:
        logits = mi.restrict(logits, mi.support(masks, p_bits(dists, A), weight, A, True, actions))
    acts = torch.as_tensor(np.asarray(actions)).reshape(-1).long()
    r = kh.kickstart_terms(logits, values, acts, adv, old_lp, returns, torch.zeros(M, dtype=torch.int64), weight, clip,
                           ent_coef, vf_coef, 0.0, norm, mask=mask)       # the PPO terms alone
    kl, acc, share = _kl(logits, dists, weight, tau, mask.to(logits.dtype))
    r.update(loss=r["loss"] + bc_coef * kl, bc_loss=kl, accuracy=acc, labelled=share)
    return r


def bc_soft_heads64(hp, hv, wa, ba, wv, bv, dists, weight, returns, tau, ent_coef, vf_coef, masks=None):
    """-> (dh [2, M, F], (dwa, dba, dwv, dbv), stats [6]) float64 tensors."""
    leaves, logits, values = mi._heads(hp, hv, wa, ba, wv, bv)
    r = bc_soft_terms(logits, values, dists, weight, torch.tensor(np.asarray(returns, np.float64)), tau, ent_coef,
                      vf_coef, masks=masks)
    return mi._grads(r["loss"], leaves, torch.stack([r[k].detach().double() for k in BC_KEYS]))


def kickstart_soft_heads64(hp, hv, wa, ba, wv, bv, actions, adv, old_lp, returns, dists, weight, tau, clip, ent_coef,
                           vf_coef, bc_coef, norm, masks=None):
    """-> (dh [2, M, F], (dwa, dba, dwv, dbv), stats [9]) float64 tensors."""
    c = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    leaves, logits, values = mi._heads(hp, hv, wa, ba, wv, bv)
    r = kickstart_soft_terms(logits, values, actions, c(adv), c(old_lp), c(returns), dists, weight, tau, clip,
                             ent_coef, vf_coef, bc_coef, norm, masks=masks)
    return mi._grads(r["loss"], leaves, torch.stack([r[k].detach().double() for k in KS_KEYS]))


# ------------------------------------------------------------------ the learners' train() in float64
def _rows(buf, masked):
    T, N = np.asarray(buf["actions"]).shape
    assert T * N < ROW, "the row number must fit below the mask byte"
    rows = np.arange(T * N, dtype=np.int64).reshape(T, N)
    return rows + ROW * np.asarray(buf["action_masks"]).astype(np.int64) if masked else rows


def _unrow(lab, table, masked):
    lab = mi._int(lab)
    return table[(lab % ROW).numpy()], (lab // ROW if masked else None)


def bc_soft_train(weights, buf, epoch_orders, tau, masked=False, **kw):
    """One ``BCLearner(labels="soft").train`` call in float64: ``bc_helpers.bc_train`` with
    ``bc_soft_terms``.  ``buf``: its arrays plus ``expert_dists`` [T, N, 6] (and ``action_masks``
    uint8 [T, N] with ``masked``).  -> (new weights, per-minibatch stats)."""
    table = np.asarray(buf["expert_dists"]).reshape(-1, np.asarray(buf["expert_dists"]).shape[-1])
    b = dict(buf, expert_actions=_rows(buf, masked))
    saved = bh.bc_terms

    calls = []

    def terms(lg, v, lab, w, ret, ec, vc, mask=None):
        calls.append(1)
        d, m = _unrow(lab, table, masked)
        return bc_soft_terms(lg, v, d, w, ret, tau, ec, vc, masks=m, mask=mask)

    bh.bc_terms = terms
    try:
        out = bh.bc_train(weights, b, epoch_orders, **kw)
    finally:
        bh.bc_terms = saved
    assert len(calls) == len(out[1]) > 0, "bc_train did not go through the soft terms"
    return out


def kickstart_soft_train(weights, buf, epoch_orders, tau, masked=False, **kw):
    """One ``KickstartLearner(labels="soft").train`` call in float64:
    ``kickstart_helpers.kickstart_train`` with ``kickstart_soft_terms``."""
    table = np.asarray(buf["expert_dists"]).reshape(-1, np.asarray(buf["expert_dists"]).shape[-1])
    b = dict(buf, expert_actions=_rows(buf, masked))
    saved = kh.kickstart_terms

    calls = []

    def terms(lg, v, acts, adv, olp, ret, lab, w, clip, ec, vc, bc, norm, sets=False, mask=None):
        calls.append(1)
        d, m = _unrow(lab, table, masked)
        kh.kickstart_terms = saved          # kickstart_soft_terms calls the real one
        try:
            return kickstart_soft_terms(lg, v, acts, adv, olp, ret, d, w, tau, clip, ec, vc, bc, norm, masks=m,
                                        mask=mask)
        finally:
            kh.kickstart_terms = terms

    kh.kickstart_terms = terms
    try:
        out = kh.kickstart_train(weights, b, epoch_orders, **kw)
    finally:
        kh.kickstart_terms = saved
    assert len(calls) == len(out[1]) > 0, "kickstart_train did not go through the soft terms"
    return out


# ------------------------------------------------------------------ vn_dagger_mix_best
def mix_best(policy, expert, dist, best, beta, mix_seed, gids, t):
    """vn_dagger_mix_best's rule -> (executed, took_expert, label_weight, own_best)."""
    thr = math.floor(float(beta) * 2 ** 24)
    u24 = np.rint(philox_uniform(mix_seed, gids, t) * 2 ** 24).astype(np.int64)     # exact: u = u24 / 2^24
    policy = np.asarray(policy).astype(np.int64)
    lab = np.asarray(dist) != -1
    inr = (policy >= 0) & (policy < 8)
    own = lab & inr & (((np.asarray(best).astype(np.int64) >> np.where(inr, policy, 0)) & 1) == 1)
    took = lab & (u24 < thr) & ~own
    return (np.where(took, expert, policy).astype(np.int32), took.astype(np.uint8), lab.astype(np.uint8),
            own.astype(np.uint8))


# ------------------------------------------------------------------ inputs
PAD = 1                  # the poison of the padding columns: read as a distance it would be the shortest


def random_dists(rng, rows, A, ldd=None, p_none=0.3, p_single=0.25, p_wide=0.05):
    """int32 [rows, ldd] distance rows (ldd = A + 2 by default, the padding poisoned): ``p_none`` of
    them without a positive entry (-1, -2 and 0), ``p_single`` with exactly one, the rest with a
    shortest distance d* up to 2000 and every other action at d*, d* + 1, d* + 2, -1 or -2;
    ``p_wide`` of the rows (among the rest) have one entry at d* + 100 as well."""
    ldd = A + 2 if ldd is None else ldd
    d = np.full((rows, ldd), PAD, np.int32)
    neg = np.array([-1, -2, 0], np.int32)
    u = rng.random(rows)
    for i in range(rows):
        row = neg[rng.integers(0, 3, A)]
        if u[i] >= p_none:
            dstar = int(rng.integers(1, 2001))
            k = int(rng.integers(0, A))
            row[k] = dstar
            if u[i] >= p_none + p_single:
                for j in range(A):
                    if j != k:
                        c = int(rng.integers(0, 5))
                        row[j] = dstar + c if c < 3 else (-1 if c == 3 else -2)
                if A > 1 and rng.random() < p_wide / (1 - p_none - p_single):
                    j = (k + 1 + int(rng.integers(0, A - 1))) % A
                    row[j] = dstar + 100
        d[i, :A] = row
    return d


def soft_buffer(b, device, masked=False):
    """``bc_helpers.as_dagger_buffer`` (``masked_imitate_helpers.masked_buffer``) plus ``expert_dists``."""
    buf = mi.masked_buffer(b, device, False) if masked else bh.as_dagger_buffer(b, device)
    buf.expert_dists = torch.as_tensor(b["expert_dists"], device=device)
    buf.took_expert = torch.zeros(np.asarray(b["actions"]).shape, dtype=torch.uint8, device=device)
    return buf


def parity_arrays(T, N, lstm, recurrent, masked, p_start=0.15):
    b = bh.dagger_arrays(T, N, lstm, recurrent, p_start=p_start)
    b["expert_dists"] = random_dists(np.random.default_rng(11), T * N, 6, ldd=6).reshape(T, N, 6)
    if masked:
        b["action_masks"] = mi.random_masks(np.random.default_rng(13), (T, N))
    return b


def run_soft_parity(device, which, recurrent, masked, tau=0.7, T=12, N=5, batch_size=16, epochs=2, arch=(32, 16),
                    lstm=16, p_start=0.15, bc_coef=0.7, atol=2e-5, rtol=1e-4):
    """``BCLearner`` (``which`` = "bc") or ``KickstartLearner`` ("kickstart") with ``labels="soft"``
    on ``device`` against its float64 restatement, with ``bc_set_helpers.run_bc_set_parity``'s
    shapes and bounds: parameters within atol + rtol |ref|, logged values within 1e-4 relative.
    -> (learner, restatement stats)."""
    from voxnav.imitate import BCLearner, KickstartLearner
    from voxnav.policy import numpy_weights
    pol = bh.small_policy(recurrent, arch, lstm).to(device)
    w0 = numpy_weights(pol)
    b = parity_arrays(T, N, lstm, recurrent, masked, p_start)
    if masked:                                           # positive distances outside their masks
        assert ((p_bits(b["expert_dists"].reshape(-1, 6), 6).numpy() & ~b["action_masks"].reshape(-1) & 63) != 0).mean() > 0.2
    rng = np.random.default_rng(7)
    orders = ([int(rng.integers(T * N)) for _ in range(epochs)] if recurrent
              else [rng.permutation(T * N) for _ in range(epochs)])
    if which == "bc":
        ln = BCLearner(pol, n_epochs=epochs, batch_size=batch_size, labels="soft", label_tau=tau, action_masks=masked)
        w1, ost = bc_soft_train(w0, b, orders, f32(tau), masked=masked, batch_size=batch_size)
        keys, names = BC_KEYS, {}
    else:
        ln = KickstartLearner(pol, n_epochs=epochs, batch_size=batch_size, bc_coef=bc_coef, labels="soft",
                              label_tau=tau, action_masks=masked)
        w1, ost = kickstart_soft_train(w0, b, orders, f32(tau), masked=masked, batch_size=batch_size, bc_coef=bc_coef)
        keys, names = KS_KEYS, dict(policy_loss="policy_gradient_loss")
    st = ln.train(soft_buffer(b, device, masked), epoch_orders=orders)
    got = numpy_weights(pol)
    moved = 0.0
    for k in w1:
        np.testing.assert_allclose(got[k], w1[k], atol=atol, rtol=rtol, err_msg=k)
        moved = max(moved, float(np.abs(w1[k] - w0[k]).max()))
    assert moved > 1e-4                                 # the update did something
    n = len(ost)
    assert st["n_minibatches"] == n == epochs * -(-T * N // batch_size)
    for key in keys + ("grad_norm",):
        ref = float(np.mean([s[key] for s in ost]))
        val = st[names.get(key, key)]
        print(f"{key}: learner {val!r} restatement {ref!r}")
        assert abs(val - ref) <= 1e-4 * max(1.0, abs(ref)), (key, val, ref)
    assert 0.3 < np.mean([s["labelled"] for s in ost]) < 0.8
    return ln, ost
