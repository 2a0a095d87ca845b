"""The DAgger warm start off the GPU (voxnav.imitate's torch path, tests/bc_helpers.py's float64
restatements): known answers of the loss formula (include/voxnav.h, vn_bc_loss), ``BCLearner.train``
against the restatement, the mix rule of vn_dagger_mix, and a closed loop in which a policy learns
from the frontier planner's rule (tests/route_helpers.py) driving the per-agent CPU oracle.
"""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bc_helpers as bh  # noqa: E402
import route_helpers as rh  # noqa: E402
from helpers import box_text, philox_uniform  # noqa: E402


# ------------------------------------------------------------------ 1. known answers
def _zero_head_learner(M, A, weight, **kw):
    """A feed-forward BCLearner with zero heads on an M-sample buffer ([T = M, N = 1])."""
    from voxnav.imitate import BCLearner
    pol = bh.small_policy(False)
    with torch.no_grad():
        for p in list(pol.action_net.parameters()) + list(pol.value_net.parameters()):
            p.zero_()
    b = bh.dagger_arrays(M, 1, 16, False, seed=3)
    b["label_weight"] = weight
    if weight is None:
        del b["label_weight"]
    # no clipping: the gradients left in .grad are the loss's own
    ln = BCLearner(pol, n_epochs=1, batch_size=M, max_grad_norm=1e9, **kw)
    return pol, b, ln


def test_restatement_zero_logits_give_ln_A_and_uniform_minus_onehot():
    M, A = 7, 6
    rng = np.random.default_rng(0)
    labels = torch.as_tensor(rng.integers(0, A, M))
    logits = torch.zeros((M, A), dtype=torch.float64, requires_grad=True)
    r = bh.bc_terms(logits, torch.zeros(M, dtype=torch.float64), labels, None, torch.zeros(M, dtype=torch.float64),
                    0.0, 0.5)
    assert abs(float(r["bc_loss"].detach()) - math.log(A)) < 1e-12
    assert abs(float(r["entropy_loss"].detach()) + math.log(A)) < 1e-12
    dz, = torch.autograd.grad(r["loss"], [logits])
    want = (1.0 / A - torch.nn.functional.one_hot(labels, A).double()) / M
    assert float((dz - want).abs().max()) < 1e-15
    # every logit ties: the argmax is index 0
    assert float(r["accuracy"]) == float((labels == 0).double().mean()) and float(r["labelled"]) == 1.0


def test_restatement_all_zero_weights():
    M, A = 9, 4
    rng = np.random.default_rng(1)
    labels = torch.as_tensor(rng.integers(0, A, M))
    logits = torch.tensor(rng.normal(size=(M, A)), requires_grad=True)
    values = torch.tensor(rng.normal(size=M), requires_grad=True)
    ret = torch.tensor(rng.normal(size=M))
    r = bh.bc_terms(logits, values, labels, np.zeros(M, np.uint8), ret, 0.0, 0.5)
    assert float(r["bc_loss"].detach()) == 0.0 and float(r["accuracy"]) == 0.0 and float(r["labelled"]) == 0.0
    dz, dv = torch.autograd.grad(r["loss"], [logits, values])
    assert float(dz.abs().max()) == 0.0
    assert float((dv - 2 * 0.5 * (values - ret).detach() / M).abs().max()) < 1e-15      # the value term is unchanged


def test_restatement_argmax_tie_goes_to_the_lowest_index():
    logits = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, 1.0, 0.5, 1.0]], dtype=torch.float64)
    z = torch.zeros(3, dtype=torch.float64)
    for labels, want in (([1, 0, 1], 1.0), ([2, 1, 3], 0.0), ([1, 3, 3], 1 / 3)):
        r = bh.bc_terms(logits, z, torch.tensor(labels), None, z, 0.0, 0.0)
        assert abs(float(r["accuracy"]) - want) < 1e-15


@pytest.mark.parametrize("weighted", [False, True], ids=["all-labelled", "weights"])
def test_torch_path_zero_heads(weighted):
    """BCLearner's torch path with zero head weights and biases: ce = ln A, the action bias
    gradient is sum_i dz_i with dz = (w_i / n)(1/A - onehot), ties count for index 0."""
    M, A = 12, 6
    weight = (np.arange(M).reshape(M, 1) % 3 != 0).astype(np.uint8) if weighted else None
    pol, b, ln = _zero_head_learner(M, A, weight)
    st = ln.train(bh.as_dagger_buffer(b, "cpu"), epoch_orders=[np.arange(M)])
    w = np.ones(M) if weight is None else weight.reshape(-1).astype(np.float64)
    lab = b["expert_actions"].reshape(-1)
    n = w.sum()
    assert abs(st["bc_loss"] - math.log(A)) < 1e-6 and abs(st["entropy_loss"] + math.log(A)) < 1e-6
    assert abs(st["labelled"] - n / M) < 1e-12
    assert abs(st["accuracy"] - (w * (lab == 0)).sum() / n) < 1e-12
    want = ((w[:, None] / n) * (1.0 / A - np.eye(A)[lab])).sum(0)
    np.testing.assert_allclose(pol.action_net.bias.grad.numpy(), want, atol=1e-7)
    assert st["n_minibatches"] == 1 and st["n_updates"] == 1


def test_torch_path_all_zero_weights():
    M, A = 12, 6
    pol, b, ln = _zero_head_learner(M, A, np.zeros((M, 1), np.uint8))
    st = ln.train(bh.as_dagger_buffer(b, "cpu"), epoch_orders=[np.arange(M)])
    assert st["bc_loss"] == 0.0 and st["accuracy"] == 0.0 and st["labelled"] == 0.0
    assert float(pol.action_net.bias.grad.abs().max()) == 0.0 and float(pol.action_net.weight.grad.abs().max()) == 0.0
    assert float(pol.value_net.bias.grad.abs().max()) > 0.0                      # the value term is unchanged
    assert st["value_loss"] > 0.0


def test_learner_needs_labels():
    from voxnav.collector import RolloutBuffer
    from voxnav.imitate import BCLearner
    b = bh.as_dagger_buffer(bh.dagger_arrays(4, 2, 16, False), "cpu")
    plain = RolloutBuffer(**{k: getattr(b, k) for k in RolloutBuffer.__dataclass_fields__})
    with pytest.raises(ValueError, match="expert_actions"):
        BCLearner(bh.small_policy(False)).train(plain)


# ------------------------------------------------------------------ 2. the learner vs the restatement
@pytest.mark.parametrize("recurrent", [True, False], ids=["lstm", "mlp"])
def test_bc_learner_matches_restatement_cpu(recurrent):
    """tests/test_ppo.py's small shapes: T = 12, N = 5, batch 16, 2 epochs, LSTM 16 / MLP [32, 16];
    episode starts at p = 0.15, ~20 % of the label weights zero."""
    bh.run_bc_parity("cpu", recurrent)


def test_bc_learner_entropy_bonus_cpu():
    bh.run_bc_parity("cpu", False, ent_coef=0.01)


# ------------------------------------------------------------------ 3. the mix rule
@pytest.mark.parametrize("base", [0, (1 << 32) + 12345], ids=["base0", "base>2^32"])
def test_mix_rule_restatement(base):
    N, seed, t = 500, 4242, (1 << 33) + 7
    rng = np.random.default_rng(5)
    policy = rng.integers(0, 6, N).astype(np.int32)
    expert = ((policy + 1 + rng.integers(0, 5, N)) % 6).astype(np.int32)      # never the policy's action
    dist = rng.integers(1, 20, N).astype(np.int32)
    dist[rng.random(N) < 0.2] = -1
    gids = base + np.arange(N)
    u = philox_uniform(seed, gids, t)
    lab = dist != -1
    assert lab.any() and (~lab).any()
    ex, took, w = bh.mix(policy, expert, dist, 0.0, seed, gids, t)
    assert not took.any() and (ex == policy).all() and (w == lab).all()
    ex, took, w = bh.mix(policy, expert, dist, 1.0, seed, gids, t)
    assert (took == lab).all() and (ex == np.where(lab, expert, policy)).all() and (w == lab).all()
    ex, took, w = bh.mix(policy, expert, dist, 0.5, seed, gids, t)
    assert (took == (lab & (u < 0.5))).all() and (ex == np.where(took, expert, policy)).all()
    assert 0.3 < took[lab].mean() < 0.7
    # the draw depends on the key, the agent and the step
    assert (bh.mix(policy, expert, dist, 0.5, seed + 1, gids, t)[1] != took).any()
    assert (bh.mix(policy, expert, dist, 0.5, seed, gids, t + 1)[1] != took).any()
    if base:
        assert (bh.mix(policy, expert, dist, 0.5, seed, gids - (1 << 32), t)[1] != took).any()


# ------------------------------------------------------------------ 4. closed loop
def _planner_rollout(agents, obs, T, episode, gamma=0.99):
    """T steps of every agent under the planner's rule -> DaggerBuffer arrays (returns: the
    discounted reward to go inside the rollout, cut at episode ends)."""
    N = len(agents)
    b = dict(obs=np.zeros((T, N, 80), np.float32), expert_actions=np.zeros((T, N), np.int32),
             label_weight=np.zeros((T, N), np.uint8), episode_starts=np.zeros((T, N), np.float32),
             rewards=np.zeros((T, N), np.float32), dones=np.zeros((T, N), bool))
    for t in range(T):
        for i, env in enumerate(agents):
            b["obs"][t, i] = obs[i]
            a, d, _ = rh.plan(env.belief, (env.x, env.y, env.z), env.facing)
            b["expert_actions"][t, i], b["label_weight"][t, i] = a, d != -1
            o, r, te, tr = env.step(a)
            b["rewards"][t, i], b["dones"][t, i] = r, te or tr
            if te or tr:
                assert env.bump_count == 0
                episode[i] += 1
                o = env.reset(1000 * episode[i] + i)
                if t + 1 < T:
                    b["episode_starts"][t + 1, i] = 1.0
            obs[i] = o
    ret = np.zeros((T, N), np.float32)
    run = np.zeros(N)
    for t in reversed(range(T)):
        run = b["rewards"][t] + gamma * run * ~b["dones"][t]
        ret[t] = run
    z = np.zeros((T, N), np.float32)
    b.update(actions=b["expert_actions"], returns=ret, values=z, log_probs=z, advantages=z)
    return b


def test_closed_loop_policy_learns_from_the_planner_cpu():
    """Eight per-agent CPU oracles (oracle/py_cubic.py) on the 8x8x4 box, driven by the planner's
    rule; an MLP policy [64, 64] trained by BCLearner's torch path (its defaults but lr 1e-3, one
    epoch) on each 32-step rollout in turn, 10 iterations, seeds fixed.  Observed: bc_loss 1.769 in
    the first iteration, 0.946 in the last; accuracy 0.543 -> 0.703 (about the share of the
    planner's most frequent action: a feed-forward policy of this size learns little more than that
    in 2,560 samples); labelled share 1.0 in every iteration -- the restatement alone labels every
    step of this room, a target stays in reach until the episode ends.  The asserted margins are a
    third of the observed loss drop and of the accuracy gain."""
    from oracle.oracle import parse_room_text
    from oracle.py_cubic import PyCubicAgent
    from voxnav.imitate import BCLearner
    N, T, iters = 8, 32, 10
    room = parse_room_text(box_text(8, 8, 4), "box")
    agents = [PyCubicAgent([room], local_map_length=4) for _ in range(N)]
    obs = [env.reset(i) for i, env in enumerate(agents)]
    episode = [0] * N
    pol = bh.small_policy(False, arch=(64, 64), seed=2)
    ln = BCLearner(pol, learning_rate=1e-3, n_epochs=1, batch_size=64, seed=2)
    hist = []
    for _ in range(iters):
        b = _planner_rollout(agents, obs, T, episode)
        hist.append(ln.train(bh.as_dagger_buffer(b, "cpu")))
    print([(round(h["bc_loss"], 3), round(h["accuracy"], 3), h["labelled"]) for h in hist])
    assert all(h["labelled"] >= 0.9 for h in hist)
    assert sum(episode) >= 1                                     # episodes ended and restarted inside the run
    assert hist[-1]["bc_loss"] < hist[0]["bc_loss"] - 0.27
    assert hist[-1]["accuracy"] > hist[0]["accuracy"] + 0.05
