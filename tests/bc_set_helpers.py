"""Float64 restatements of the set-valued behaviour-cloning loss (include/voxnav.h, vn_bc_loss_set)
-- TEST INFRASTRUCTURE ONLY; the product paths are the HIP kernel and voxnav.imitate's torch path.

* ``bc_set_terms``: the loss from logits and values, ``bc_helpers.bc_terms`` with a bit set per
  sample in place of a label; written with explicit sums over the set's members (log sum_{j in S} p_j),
  not with the masked logsumexp of the product's torch path;
* ``bc_set_heads64``: that loss from the latents on, with its gradients by float64 autograd;
* ``bc_set_train``: ``bc_helpers.bc_train`` with ``bc_set_terms`` as its loss and ``expert_set`` as
  its labels;
* ``random_sets``, ``run_bc_set_parity``: the inputs and the learner parity check of the tests.
"""
from __future__ import annotations

import numpy as np
import torch

import bc_helpers as bh


def members(sets, A):
    """bool [M, A]: bit j < A of each set (bits at or above A are ignored)."""
    s = torch.as_tensor(np.asarray(sets).astype(np.int64)).view(-1, 1)
    return ((s >> torch.arange(A)) & 1).bool()


def bc_set_terms(logits, values, sets, weight, returns, ent_coef, vf_coef, mask=None):
    """``bc_helpers.bc_terms`` for label sets -> the same dict."""
    M, A = logits.shape
    mask = torch.ones(M, dtype=torch.bool) if mask is None else mask
    m = mask.to(logits.dtype)
    S = members(sets, A)
    some = S.any(-1)
    w = m.clone() if weight is None else (torch.as_tensor(weight) != 0).to(logits.dtype) * m
    w = w * some.to(logits.dtype)
    count = m.sum()
    lp_all = torch.log_softmax(logits, dim=-1)
    p = lp_all.exp()
    H = -(p * lp_all).sum(-1)
    p_set = (p * S.to(logits.dtype)).sum(-1)
    ce_i = -torch.log(torch.where(some, p_set, torch.ones_like(p_set)))
    n = w.sum()
    den = torch.clamp(n, min=1.0)
    ce = (w * ce_i).sum() / den
    el = -(m * H).sum() / count
    vl = (m * (returns - values) ** 2).sum() / count
    amax = torch.full((M,), A, dtype=torch.int64)
    top = logits.max(-1).values
    for j in reversed(range(A)):                         # ties: the lowest index wins
        amax = torch.where(logits[:, j] == top, torch.full_like(amax, j), amax)
    acc = (w * S.gather(1, amax.view(-1, 1)).flatten().to(logits.dtype)).sum() / den
    return dict(bc_loss=ce, value_loss=vl, entropy_loss=el, loss=ce + ent_coef * el + vf_coef * vl,
                accuracy=acc.detach(), labelled=(n / count).detach())


def bc_set_heads64(hp, hv, wa, ba, wv, bv, sets, weight, returns, ent_coef, vf_coef):
    """``bc_helpers.bc_heads64`` for label sets."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    hp, hv, wa, ba, wv, bv = (t(a) for a in (hp, hv, wa, ba, wv, bv))
    logits = hp @ wa.T + ba
    values = hv @ wv.reshape(-1) + bv.reshape(())
    r = bc_set_terms(logits, values, np.asarray(sets), None if weight is None else np.asarray(weight),
                     torch.tensor(np.asarray(returns, np.float64)), ent_coef, vf_coef)
    g = torch.autograd.grad(r["loss"], [hp, hv, wa, ba, wv, bv], allow_unused=True)
    g = [np.zeros(tuple(x.shape)) if y is None else y.numpy() for x, y in zip((hp, hv, wa, ba, wv, bv), g)]
    stats = np.array([float(r[k].detach()) for k in bh.STAT_KEYS])
    return g[0], g[1], tuple(g[2:]), stats


def bc_set_train(weights, buf, epoch_orders, **kw):
    """``bc_helpers.bc_train`` (its minibatches, sequences, Adam and clip) with the set loss:
    ``buf["expert_set"]`` takes the labels' place."""
    b = dict(buf, expert_actions=np.asarray(buf["expert_set"]).astype(np.int64))
    saved = bh.bc_terms
    bh.bc_terms = lambda lg, v, lab, w, ret, ec, vc, mask=None: bc_set_terms(lg, v, lab.numpy(), w, ret, ec, vc,
                                                                            mask=mask)
    try:
        return bh.bc_train(weights, b, epoch_orders, **kw)
    finally:
        bh.bc_terms = saved


def random_sets(rng, shape, A, p_empty=0.3, p_single=0.25):
    """uint8 sets: empty with probability ``p_empty``, one member with ``p_single``, else every bit
    below A with probability 1/2; bits at or above A set at random as well (they are to be ignored)."""
    n = int(np.prod(shape))
    u = rng.random(n)
    s = rng.integers(0, 1 << A, n)
    single = 1 << rng.integers(0, A, n)
    s = np.where(u < p_empty, 0, np.where(u < p_empty + p_single, single, s))
    if A < 8:
        s = s | (rng.integers(0, 1 << (8 - A), n) << A)
    return s.astype(np.uint8).reshape(shape)


def set_buffer(b, device):
    """``bc_helpers.as_dagger_buffer`` plus ``expert_set``."""
    buf = bh.as_dagger_buffer(b, device)
    buf.expert_set = torch.as_tensor(b["expert_set"], device=device)
    return buf


def run_bc_set_parity(device, recurrent, T=12, N=5, batch_size=16, epochs=2, arch=(32, 16), lstm=16, p_start=0.15,
                      ent_coef=0.0, atol=2e-5, rtol=1e-4):
    """``bc_helpers.run_bc_parity`` for ``BCLearner(labels="set")`` against ``bc_set_train``, with its
    bounds.  Sets: 30 % empty, 25 % singletons; ~20 % of the label weights zero.
    -> (learner, restatement stats)."""
    from voxnav.imitate import BCLearner
    from voxnav.policy import numpy_weights
    pol = bh.small_policy(recurrent, arch, lstm).to(device)
    w0 = numpy_weights(pol)
    b = bh.dagger_arrays(T, N, lstm, recurrent, p_start=p_start)
    b["expert_set"] = random_sets(np.random.default_rng(11), (T, N), 6)
    rng = np.random.default_rng(7)
    orders = ([int(rng.integers(T * N)) for _ in range(epochs)] if recurrent
              else [rng.permutation(T * N) for _ in range(epochs)])
    ln = BCLearner(pol, n_epochs=epochs, batch_size=batch_size, ent_coef=ent_coef, labels="set")
    st = ln.train(set_buffer(b, device), epoch_orders=orders)
    w1, ost = bc_set_train(w0, b, orders, batch_size=batch_size, ent_coef=ent_coef)
    got = numpy_weights(pol)
    moved = 0.0
    for k in w1:
        np.testing.assert_allclose(got[k], w1[k], atol=atol, rtol=rtol, err_msg=k)
        moved = max(moved, float(np.abs(w1[k] - w0[k]).max()))
    assert moved > 1e-4                                 # the update did something
    n = len(ost)
    assert st["n_minibatches"] == n == epochs * -(-T * N // batch_size)
    for key in bh.STAT_KEYS + ("grad_norm",):
        ref = float(np.mean([s[key] for s in ost]))
        print(f"{key}: learner {st[key]!r} restatement {ref!r}")
        assert abs(st[key] - ref) <= 1e-4 * max(1.0, abs(ref)), (key, st[key], ref)
    assert 0.3 < np.mean([s["labelled"] for s in ost]) < 0.8
    return ln, ost
