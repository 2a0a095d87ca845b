"""Float64 restatements for masked DAgger and masked kickstart (voxnav.imitate with
``action_masks=True``, csrc/voxnav_masked_bc_loss.hip, csrc/voxnav_masked_ppo_bc_loss.hip) -- TEST
INFRASTRUCTURE ONLY; the product paths are the HIP kernels and voxnav.imitate's torch path.

Everything here is one of the existing restatements -- ``bc_helpers.bc_terms``,
``bc_set_helpers.bc_set_terms``, ``kickstart_helpers.kickstart_terms`` -- applied to the softmax
restricted to S_i (include/voxnav.h vn_bc_loss_masked):

* ``support``: S_i = ``mask_helpers.allowed_sets`` of the mask byte with the label's bits of a
  labelled sample (and, for the PPO+BC forms, the taken action) or-ed in, so that its "an empty set
  counts as full" applies to the union, as the header states it;
* ``restrict``: the logits with a finite, hugely negative value outside S_i.  In float64 its
  exponential is exactly 0, so log-softmax, probabilities, entropy and argmax over the restricted
  logits are those over S_i, the terms outside are 0 * finite = 0 (never 0 * inf), and through
  ``torch.where`` the masked logits get a gradient of exactly 0;
* ``masked_bc_terms`` / ``masked_kickstart_terms``: the terms; ``bc_heads64`` / ``kickstart_heads64``:
  from the latents on with autograd; ``reference``: those on a kernel case;
* ``masked_bc_train`` / ``masked_kickstart_train``: ``bc_helpers.bc_train`` /
  ``kickstart_helpers.kickstart_train`` (their minibatches, sequences, Adam and clip) with the masked
  terms; the mask byte rides through their gathers in the label's high bits.
"""
from __future__ import annotations

import numpy as np
import torch

import bc_helpers as bh
import bc_set_helpers as bs
import kickstart_helpers as kh
import mask_helpers as mh

NEG = -1e30        # exp(NEG - anything a head produces) is exactly 0 in float64
BC_KEYS = bh.STAT_KEYS
KS_KEYS = kh.STAT_KEYS


def _int(a):
    return torch.as_tensor(np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a)).to(torch.int64).reshape(-1)


def _labelled_by_weight(weight, M):
    return torch.ones(M, dtype=torch.bool) if weight is None else _int(weight) != 0


def label_bits(labels, weight, A, sets):
    """int64 [M]: L_i, the label's bits below A where the weight labels the sample (an empty set
    has no bits: such a sample is unlabelled anyway)."""
    lab = _int(labels)
    on = _labelled_by_weight(weight, lab.numel())
    full = (1 << A) - 1
    if sets:
        bits = lab & full
    else:
        bits = torch.where((lab >= 0) & (lab < A), torch.ones_like(lab) << lab.clamp(0, A - 1), torch.zeros_like(lab))
    return torch.where(on, bits, torch.zeros_like(bits))


def support(masks, labels, weight, A, sets, actions=None):
    """bool [M, A]: S_i = (mask_i & full) | L_i (| 1 << a_i with ``actions``), empty as full."""
    m = _int(masks) | label_bits(labels, weight, A, sets)
    return mh.allowed_sets(m, A, None if actions is None else _int(actions))


def restrict(logits, S):
    return torch.where(S, logits, torch.full_like(logits, NEG))


def _effective_sets(labels, weight, A):
    """The sets with those of samples without weight emptied: they are unlabelled either way, and a
    set outside S_i has probability 0 (bc_set_terms would take its logarithm)."""
    return label_bits(labels, weight, A, True).numpy()


def masked_bc_terms(logits, values, labels, masks, weight, returns, ent_coef, vf_coef, sets=False, mask=None):
    """``bc_terms`` / ``bc_set_terms`` over S_i -> the same dict."""
    A = logits.shape[1]
    zl = restrict(logits, support(masks, labels, weight, A, sets))
    if sets:
        return bs.bc_set_terms(zl, values, _effective_sets(labels, weight, A), weight, returns, ent_coef, vf_coef,
                               mask=mask)
    return bh.bc_terms(zl, values, _int(labels), weight, returns, ent_coef, vf_coef, mask=mask)


def masked_kickstart_terms(logits, values, actions, adv, old_lp, returns, labels, masks, weight, clip, ent_coef, vf_coef,
                           bc_coef, norm, sets=False, mask=None):
    """``kickstart_terms`` over S_i (the taken action added) -> the same dict."""
    A = logits.shape[1]
    zl = restrict(logits, support(masks, labels, weight, A, sets, actions))
    lab = _effective_sets(labels, weight, A) if sets else _int(labels)
    return kh.kickstart_terms(zl, values, _int(actions), adv, old_lp, returns, lab, weight, clip, ent_coef, vf_coef,
                              bc_coef, norm, sets=sets, mask=mask)


# ------------------------------------------------------------------ from the latents on
def _heads(hp, hv, wa, ba, wv, bv):
    t = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)  # noqa: E731
    leaves = [t(a) for a in (hp, hv, wa, ba, wv, bv)]
    hp, hv, wa, ba, wv, bv = leaves
    return leaves, hp @ wa.reshape(-1, hp.shape[1]).T + ba, hv @ wv.reshape(-1) + bv.reshape(())


def _grads(loss, leaves, stats):
    g = torch.autograd.grad(loss, leaves, allow_unused=True)
    g = [torch.zeros_like(x) if y is None else y for x, y in zip(leaves, g)]
    return torch.stack([g[0], g[1]]), tuple(g[2:]), stats


def bc_heads64(hp, hv, wa, ba, wv, bv, labels, masks, weight, returns, ent_coef, vf_coef, sets=False):
    """-> (dh [2, M, F], (dwa, dba, dwv, dbv), stats [6]) float64 tensors."""
    leaves, logits, values = _heads(hp, hv, wa, ba, wv, bv)
    r = masked_bc_terms(logits, values, labels, masks, weight, torch.tensor(np.asarray(returns, np.float64)),
                        ent_coef, vf_coef, sets=sets)
    return _grads(r["loss"], leaves, torch.stack([r[k].detach().double() for k in BC_KEYS]))


def kickstart_heads64(hp, hv, wa, ba, wv, bv, actions, adv, old_lp, returns, labels, masks, weight, clip, ent_coef,
                      vf_coef, bc_coef, norm, sets=False):
    """-> (dh [2, M, F], (dwa, dba, dwv, dbv), stats [9]) float64 tensors."""
    c = lambda a: torch.tensor(np.asarray(a, np.float64))  # noqa: E731
    leaves, logits, values = _heads(hp, hv, wa, ba, wv, bv)
    r = masked_kickstart_terms(logits, values, actions, c(adv), c(old_lp), c(returns), labels, masks, weight, clip,
                               ent_coef, vf_coef, bc_coef, norm, sets=sets)
    return _grads(r["loss"], leaves, torch.stack([r[k].detach().double() for k in KS_KEYS]))


def reference(c, mask, ent_coef, vf_coef, ppo=None):
    """The restatement on a kernel case of ``kickstart_helpers.case`` with the rollout's mask
    buffer.  ``ppo`` None: the BC form; else (clip, bc_coef, norm): the PPO+BC form."""
    n = lambda t: t.detach().cpu().numpy()  # noqa: E731
    g = lambda t: None if t is None else n(t if c["src"] is None else t[c["src"]])  # noqa: E731
    an, vn = c["an"], c["vn"]
    heads = (n(c["h"][0]), n(c["h"][1]), n(an.weight), n(an.bias), n(vn.weight), n(vn.bias))
    if ppo is None:
        return bc_heads64(*heads, g(c["lab"]), g(mask), g(c["wgt"]), g(c["ret"]), ent_coef, vf_coef, sets=c["sets"])
    clip, bc_coef, norm = ppo
    return kickstart_heads64(*heads, g(c["act"]), g(c["adv"]), g(c["olp"]), g(c["ret"]), g(c["lab"]), g(mask),
                             g(c["wgt"]), clip, ent_coef, vf_coef, bc_coef, norm, sets=c["sets"])


# ------------------------------------------------------------------ the learners' train() in float64
def _packed(buf, sets):
    """label + 256 mask, so that the mask follows the label through the restatements' gathers and
    paddings (a padded position gets label 0 and an empty mask; it carries no weight)."""
    lab = np.asarray(buf["expert_set"] if sets else buf["expert_actions"]).astype(np.int64)
    return lab + 256 * np.asarray(buf["action_masks"]).astype(np.int64)


def _unpack(lab):
    lab = _int(lab)
    return lab % 256, lab // 256


def masked_bc_train(weights, buf, epoch_orders, sets=False, **kw):
    """One ``BCLearner(action_masks=True).train`` call in float64: ``bc_helpers.bc_train`` with
    ``masked_bc_terms``.  ``buf``: its arrays plus ``action_masks`` uint8 [T, N] (and ``expert_set``
    with ``sets``).  -> (new weights, per-minibatch stats)."""
    b = dict(buf, expert_actions=_packed(buf, sets))
    saved = bh.bc_terms

    def terms(lg, v, lab, w, ret, ec, vc, mask=None):
        lab, m = _unpack(lab)
        bh.bc_terms = saved                 # masked_bc_terms calls the real one
        try:
            return masked_bc_terms(lg, v, lab, m, w, ret, ec, vc, sets=sets, mask=mask)
        finally:
            bh.bc_terms = terms

    bh.bc_terms = terms
    try:
        return bh.bc_train(weights, b, epoch_orders, **kw)
    finally:
        bh.bc_terms = saved


def masked_kickstart_train(weights, buf, epoch_orders, sets=False, **kw):
    """One ``KickstartLearner(action_masks=True).train`` call in float64:
    ``kickstart_helpers.kickstart_train`` with ``masked_kickstart_terms``."""
    b = dict(buf)
    b["expert_set" if sets else "expert_actions"] = _packed(buf, sets)
    saved = kh.kickstart_terms

    def terms(lg, v, acts, adv, olp, ret, lab, w, clip, ec, vc, bc, norm, sets=False, mask=None):
        lab, m = _unpack(lab)
        kh.kickstart_terms = saved          # masked_kickstart_terms calls the real one
        try:
            return masked_kickstart_terms(lg, v, acts, adv, olp, ret, lab, m, w, clip, ec, vc, bc, norm, sets=sets,
                                          mask=mask)
        finally:
            kh.kickstart_terms = terms

    kh.kickstart_terms = terms
    try:
        return kh.kickstart_train(weights, b, epoch_orders, sets=sets, **kw)
    finally:
        kh.kickstart_terms = saved


# ------------------------------------------------------------------ buffers and learner parity (CPU and GPU)
def random_masks(rng, shape, A=6, p_empty=0.05):
    """uint8 masks drawn like test_masked_loss_gpu._masks: uniform bytes (stray bits at and above A
    among them), about ``p_empty`` of them with no bit below A."""
    m = rng.integers(0, 256, shape)
    m = np.where(rng.random(shape) < p_empty, m & ~((1 << A) - 1), m)
    return m.astype(np.uint8)


def masked_buffer(b, device, sets, took_expert=True):
    """A ``MaskedDaggerBuffer`` of the arrays of ``bc_helpers.dagger_arrays`` plus ``action_masks``
    (and ``expert_set``)."""
    from voxnav.imitate import MaskedDaggerBuffer
    plain = bs.set_buffer(b, device) if sets else bh.as_dagger_buffer(b, device)
    buf = MaskedDaggerBuffer(**{k: getattr(plain, k) for k in plain.__dataclass_fields__},
                             action_masks=torch.as_tensor(b["action_masks"], device=device))
    if took_expert:
        buf.took_expert = torch.zeros(b["actions"].shape, dtype=torch.uint8, device=device)
    return buf


def parity_arrays(T, N, lstm, recurrent, sets, p_start=0.15, full=False):
    b = bh.dagger_arrays(T, N, lstm, recurrent, p_start=p_start)
    if sets:
        b["expert_set"] = bs.random_sets(np.random.default_rng(11), (T, N), 6)
    b["action_masks"] = (np.full((T, N), 0xFF, np.uint8) if full
                         else random_masks(np.random.default_rng(13), (T, N)))
    return b


def run_masked_parity(device, which, recurrent, sets, T=12, N=5, batch_size=16, epochs=2, arch=(32, 16), lstm=16,
                      p_start=0.15, bc_coef=0.7, atol=2e-5, rtol=1e-4):
    """``BCLearner`` (``which`` = "bc") or ``KickstartLearner`` ("kickstart") with
    ``action_masks=True`` on ``device`` against its float64 ``*_train`` restatement, within the
    bounds of ``bc_helpers.run_bc_parity`` / ``kickstart_helpers.run_kickstart_parity``: parameters
    within atol + rtol |ref|, logged values within 1e-4 relative.  Masks as ``random_masks``: labels
    and taken actions fall outside them.  -> (learner, restatement stats)."""
    from voxnav.imitate import BCLearner, KickstartLearner
    from voxnav.policy import numpy_weights
    pol = bh.small_policy(recurrent, arch, lstm).to(device)
    w0 = numpy_weights(pol)
    b = parity_arrays(T, N, lstm, recurrent, sets, p_start)
    lab = b["expert_set"] if sets else (1 << b["expert_actions"])
    assert ((lab & ~b["action_masks"] & 63) != 0).mean() > 0.2           # labels outside their masks
    rng = np.random.default_rng(7)
    orders = ([int(rng.integers(T * N)) for _ in range(epochs)] if recurrent
              else [rng.permutation(T * N) for _ in range(epochs)])
    form = "set" if sets else "action"
    if which == "bc":
        ln = BCLearner(pol, n_epochs=epochs, batch_size=batch_size, labels=form, action_masks=True)
        w1, ost = masked_bc_train(w0, b, orders, sets=sets, batch_size=batch_size)
        keys, names = BC_KEYS, {}
    else:
        ln = KickstartLearner(pol, n_epochs=epochs, batch_size=batch_size, bc_coef=bc_coef, labels=form,
                              action_masks=True)
        w1, ost = masked_kickstart_train(w0, b, orders, sets=sets, batch_size=batch_size, bc_coef=bc_coef)
        keys, names = KS_KEYS, dict(policy_loss="policy_gradient_loss")
    st = ln.train(masked_buffer(b, device, sets), epoch_orders=orders)
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
    assert 0.3 < np.mean([s["labelled"] for s in ost]) < 1.0
    return ln, ost
