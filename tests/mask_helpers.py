"""Restatements for the invalid-action masking tests (test_action_mask_cpu.py,
test_action_mask_gpu.py, test_masked_loss_gpu.py, test_masked_ppo_gpu.py): the
mask of a CubicEnv observation in NumPy (include/voxnav.h vn_action_mask), the
masked Categorical draw given its uniform in float64 (vn_policy_head_masked),
and the masked PPO loss with its gradients in float64 autograd
(vn_ppo_loss_masked).  Importing this module needs no GPU."""
import numpy as np
import torch

from ppo_loss_helpers import close  # noqa: F401  (the PPO grid test's comparator)

# (dx, dy) of relative direction a (rows: fwd, right, back, left) under facing f
# (columns: N, E, S, W) -- SURVEY.md App. A.1
STEP = (((0, 1), (1, 0), (0, -1), (-1, 0)),
        ((1, 0), (0, -1), (-1, 0), (0, 1)),
        ((0, -1), (-1, 0), (0, 1), (1, 0)),
        ((-1, 0), (0, 1), (1, 0), (0, -1)))
WALL = np.float32(0.0)                       # (-2 + 2) / 22
OUTSIDE = np.float32(1) / np.float32(22)     # the window's out-of-bounds code (-1 + 2) / 22


def cell(dx, dy, dz):
    return (dx + 2) * 16 + (dy + 2) * 4 + (dz + 2)


def mask_reference(obs: np.ndarray) -> np.ndarray:
    """uint8 [N] from obs f32 [N, 80], action by action as the header states it."""
    obs = np.asarray(obs, dtype=np.float32).reshape(-1, 80)
    out = np.zeros(obs.shape[0], np.uint8)
    for n, o in enumerate(obs):
        ones = np.flatnonzero(o[64:68] == np.float32(1.0))
        f = int(ones[0]) if ones.size else 0
        m = 0
        for a in range(6):
            if a < 4:
                dx, dy = STEP[a][f]
                dz = 0
            else:
                dx, dy, dz = 0, 0, (1 if a == 4 else -1)
            v = o[cell(dx, dy, dz)]
            if not (v == WALL or v == OUTSIDE):
                m |= 1 << a
        out[n] = m
    return out


def hand_row(facing: int, blocked=(), code=WALL) -> np.ndarray:
    """An observation whose window is all known-free (visit count 1) except the
    neighbours in world directions ``blocked`` (triples (dx, dy, dz)), which
    hold ``code``."""
    o = np.full(80, np.float32(3) / np.float32(22), np.float32)
    o[64:] = 0
    o[64 + facing] = 1
    for d in blocked:
        o[cell(*d)] = code
    return o


WORLD = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))


def hand_rows():
    """(obs [K, 80], expected mask [K]): each facing with nothing blocked, each
    single blocked world direction (as a wall and as out of bounds), all six
    blocked; the expectation written from the direction table, not from
    ``mask_reference``."""
    rows, exp = [], []
    for f in range(4):
        rows.append(hand_row(f))
        exp.append(63)
        for d in WORLD:
            for code in (WALL, OUTSIDE):
                rows.append(hand_row(f, [d], code))
                if d[2]:
                    a = 4 if d[2] > 0 else 5
                else:
                    a = next(k for k in range(4) if STEP[k][f] == (d[0], d[1]))
                exp.append(63 & ~(1 << a))
        rows.append(hand_row(f, WORLD))
        exp.append(0)
    return np.stack(rows), np.asarray(exp, np.uint8)


def allowed_sets(mask, A, actions=None):
    """bool [M, A]: the mask's bits below A, the taken action added (when given),
    an empty set counting as full."""
    mask = torch.as_tensor(mask)
    S = ((mask.view(-1, 1).to(torch.int64) >> torch.arange(A, device=mask.device)) & 1).bool()
    if actions is not None:
        S = S | (torch.arange(A, device=mask.device).view(1, A) == actions.view(-1, 1).long())
    return S | ~S.any(-1, keepdim=True)


def masked_draw_reference(z, mask, u, deterministic=False):
    """float64: (actions [N], log_probs [N], cdf [N, A]) of the masked draw on
    logits z [N, A] given the uniforms u [N]: the first allowed a with
    u < cdf[a], the cdf over the allowed actions in index order; the highest
    allowed index when none crosses; the argmax over the allowed actions
    (lowest index on ties) when deterministic."""
    z = z.double()
    N, A = z.shape
    S = allowed_sets(mask, A)
    zm = z.masked_fill(~S, float("-inf"))
    lp = torch.log_softmax(zm, -1)
    p = torch.where(S, lp.exp(), torch.zeros_like(lp))
    cdf = torch.cumsum(p, -1)
    idx = torch.arange(A, device=z.device).view(1, A)
    last = torch.where(S, idx, torch.full_like(idx, -1)).max(-1).values
    if deterministic:
        act = zm.argmax(-1)       # ties: checked by the caller to be absent
    else:
        cross = S & (u.double().view(-1, 1) < cdf) & (idx < last.view(-1, 1))
        first = torch.where(cross, idx, torch.full_like(idx, A)).min(-1).values
        act = torch.where(first < A, first, last)
    return act, lp.gather(1, act.view(-1, 1)).flatten(), cdf


def masked_ppo_loss_reference(h, wa, ba, wv, bv, act, adv, olp, ret, mask, clip, ent_coef, vf_coef, norm):
    """tests/ppo_loss_helpers._ppo_loss_reference with every sample's softmax
    restricted to S_i = mask_i | {a_i} (float64, autograd): logits
    masked_fill(~S, -inf), log_softmax, the entropy with the masked terms
    zeroed."""
    h = h.detach().double().requires_grad_(True)
    P = [t.detach().double().requires_grad_(True) for t in (wa, ba, wv, bv)]
    logits = h[0] @ P[0].T + P[1]
    values = (h[1] @ P[2].T + P[3]).flatten()
    S = allowed_sets(mask, logits.shape[-1], act)
    lp_all = torch.log_softmax(logits.masked_fill(~S, float("-inf")), -1)
    lp_all = torch.where(S, lp_all, torch.zeros_like(lp_all))
    lp = lp_all.gather(1, act.long().view(-1, 1)).flatten()
    ent = -(torch.where(S, lp_all.exp(), torch.zeros_like(lp_all)) * lp_all).sum(-1)
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


def golden_pairs(d):
    """(prev_obs [K, 80], actions [K], bumped [K]) of a golden CubicEnv
    trajectory: step t acts on obs[t - 1], or on the reset obs when it is the
    first step or directly follows an episode end."""
    n = len(d["actions"])
    prev = np.empty((n, 80), np.float32)
    bumped = np.zeros(n, bool)
    ri, cur, cur_b = 1, d["reset_obs"][0], int(d["reset_state"][0][7])
    for t in range(n):
        prev[t] = cur
        b = int(d["state"][t][7])
        bumped[t] = b > cur_b
        if d["terminated"][t] or d["truncated"][t]:
            cur, cur_b = d["reset_obs"][ri], int(d["reset_state"][ri][7])
            ri += 1
        else:
            cur, cur_b = d["obs"][t], b
    return prev, d["actions"].astype(np.int64), bumped


def masked_train_reference(policy, buf, orders, batch_size, lr=3e-4, clip=0.2, ent_coef=0.01, vf_coef=0.5,
                           max_grad_norm=0.5):
    """One ``PPOLearner(action_masks=True).train`` of a feed-forward policy in
    float64: a double copy of ``policy`` (returned, with the per-minibatch
    stats), SB3 PPO.train's passes over the buffer (``orders``: one
    permutation of the env-major flat ids per epoch) with the masked heads of
    ``masked_ppo_loss_reference``'s formula, clip_grad_norm_, Adam(eps=1e-5)."""
    import copy
    pol = copy.deepcopy(policy).double().cpu()
    opt = torch.optim.Adam(pol.parameters(), lr=lr, eps=1e-5)
    T, N = buf.actions.shape
    flat = lambda t: t.detach().cpu().reshape(T * N, *t.shape[2:])  # noqa: E731
    obs, act, adv_all, olp_all, ret_all, mask = (flat(getattr(buf, k)) for k in (
        "obs", "actions", "advantages", "log_probs", "returns", "action_masks"))
    logs = []
    for order in orders:
        perm = torch.as_tensor(np.asarray(order), dtype=torch.int64)
        for s in range(0, T * N, batch_size):
            idx = perm[s:s + batch_size]
            env = idx // T
            src = (idx - env * T) * N + env
            x = obs[src].double()
            logits = pol.action_net(pol.mlp_extractor.policy_net(x))
            values = pol.value_net(pol.mlp_extractor.value_net(x)).flatten()
            a = act[src].long()
            S = allowed_sets(mask[src], logits.shape[-1], a)
            lp_all = torch.log_softmax(logits.masked_fill(~S, float("-inf")), -1)
            lp_all = torch.where(S, lp_all, torch.zeros_like(lp_all))
            lp = lp_all.gather(1, a.view(-1, 1)).flatten()
            ent = -(torch.where(S, lp_all.exp(), torch.zeros_like(lp_all)) * lp_all).sum(-1)
            adv = adv_all[src].double()
            if src.numel() > 1:
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            ratio = torch.exp(lp - olp_all[src].double())
            pl = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
            vl = torch.nn.functional.mse_loss(ret_all[src].double(), values)
            el = -ent.mean()
            loss = pl + ent_coef * el + vf_coef * vl
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(pol.parameters(), max_grad_norm)
            opt.step()
            logs.append(dict(policy_gradient_loss=pl.item(), value_loss=vl.item(), entropy_loss=el.item(),
                             loss=loss.item()))
    return pol, logs
