"""The float64 restatement of the PPO minibatch loss shared by
tests/test_learn_ops.py and tests/test_ppo_loss_grid_gpu.py, and the
tolerances both use.  Importing this module needs no GPU."""
import torch


def close(got, ref, rel=2e-5, floor=1e-6):
    """|got - ref| <= rel max|ref| + floor, entrywise (test_learn_ops._close)."""
    err = (got - ref).abs().max().item()
    assert err <= rel * ref.abs().max().item() + floor, err


def _ppo_loss_reference(h, wa, ba, wv, bv, act, adv, olp, ret, clip, ent_coef, vf_coef, norm):
    """sb3's heads + losses in float64 with autograd (RecurrentPPO.train /
    PPO.train, the block after evaluate_actions)."""
    h = h.detach().double().requires_grad_(True)
    P = [t.detach().double().requires_grad_(True) for t in (wa, ba, wv, bv)]
    logits = h[0] @ P[0].T + P[1]
    values = (h[1] @ P[2].T + P[3]).flatten()
    lp_all = torch.log_softmax(logits, -1)
    lp = lp_all.gather(1, act.long().view(-1, 1)).flatten()
    ent = -(lp_all.exp() * lp_all).sum(-1)
    adv = adv.double()
    if norm:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(lp - olp.double())
    pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    vl = torch.nn.functional.mse_loss(ret.double(), values)
    el = -ent.mean()
    loss = pl + ent_coef * el + vf_coef * vl
    loss.backward()
    lr = lp - olp.double()
    stats = torch.stack([pl, vl, el, loss, ((torch.exp(lr) - 1) - lr).mean(),
                         ((ratio - 1).abs() > clip).double().mean()]).detach()
    return h.grad, [p.grad for p in P], stats
