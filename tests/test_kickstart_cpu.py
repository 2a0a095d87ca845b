"""Kickstarted PPO off the GPU (voxnav.imitate.KickstartLearner's torch path, tests/kickstart_helpers.py's
float64 restatements): known answers of the loss formula (include/voxnav.h, vn_ppo_bc_loss),
``KickstartLearner.train`` against the restatement, its refusals, and ``kickstart``'s history.
"""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bc_helpers as bh  # noqa: E402
import bc_set_helpers as bs  # noqa: E402
import kickstart_helpers as kh  # noqa: E402

CLIP, ENT, VF = 0.2, 0.01, 0.5


# ------------------------------------------------------------------ 1. known answers: the restatement
def _logit_case(M, A, seed, zero_logits=False):
    rng = np.random.default_rng(seed)
    logits = torch.tensor(np.zeros((M, A)) if zero_logits else rng.normal(size=(M, A)), requires_grad=True)
    values = torch.tensor(rng.normal(size=M), requires_grad=True)
    t = lambda a: torch.tensor(a)  # noqa: E731
    return dict(logits=logits, values=values, actions=t(rng.integers(0, A, M)), adv=t(rng.normal(1, 2, M)),
                old_lp=t(np.log(1 / A) + rng.normal(0, 0.3, M)), returns=t(rng.normal(size=M)),
                labels=rng.integers(0, A, M), sets=bs.random_sets(rng, (M,), A))


def test_restatement_zero_logits_give_ln_A():
    M, A = 11, 6
    c = _logit_case(M, A, 0, zero_logits=True)
    r = kh.kickstart_terms(c["logits"], c["values"], c["actions"], c["adv"], c["old_lp"], c["returns"],
                           torch.as_tensor(c["labels"]), None, CLIP, ENT, VF, 0.7, True)
    assert abs(float(r["bc_loss"].detach()) - math.log(A)) < 1e-12
    assert abs(float(r["entropy_loss"].detach()) + math.log(A)) < 1e-12
    assert float(r["labelled"]) == 1.0
    p = kh.ppo_terms(c["logits"], c["values"], c["actions"], c["adv"], c["old_lp"], c["returns"], CLIP, ENT, VF, True)
    assert abs(float((r["loss"] - p["loss"]).detach()) - 0.7 * math.log(A)) < 1e-12


@pytest.mark.parametrize("sets", [False, True], ids=["action", "set"])
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
def test_restatement_reduces_to_ppo(norm, sets):
    """bc_coef = 0 with any labels, and any bc_coef with all-zero weights: the PPO restatement, in
    its loss and in its gradients."""
    M, A = 13, 5
    c = _logit_case(M, A, 1)
    lab = c["sets"] if sets else torch.as_tensor(c["labels"])
    p = kh.ppo_terms(c["logits"], c["values"], c["actions"], c["adv"], c["old_lp"], c["returns"], CLIP, ENT, VF, norm)
    gp = torch.autograd.grad(p["loss"], [c["logits"], c["values"]])
    for bc_coef, weight in ((0.0, None), (0.0, np.ones(M, np.uint8)), (3.0, np.zeros(M, np.uint8))):
        r = kh.kickstart_terms(c["logits"], c["values"], c["actions"], c["adv"], c["old_lp"], c["returns"], lab,
                               weight, CLIP, ENT, VF, bc_coef, norm, sets=sets)
        for k in ("policy_loss", "value_loss", "entropy_loss", "loss"):
            assert abs(float((r[k] - p[k]).detach())) < 1e-14, (k, bc_coef)
        g = torch.autograd.grad(r["loss"], [c["logits"], c["values"]])
        assert float((g[0] - gp[0]).abs().max()) < 1e-15 and float((g[1] - gp[1]).abs().max()) < 1e-15
        if weight is not None and not weight.any():
            assert float(r["bc_loss"].detach()) == 0.0 and float(r["accuracy"]) == 0.0 and float(r["labelled"]) == 0.0


@pytest.mark.parametrize("sets", [False, True], ids=["action", "set"])
def test_case_builder_labels_at_least_half(sets):
    """Every case the GPU grid builds (tests/test_kickstart_loss_gpu.py) has a labelled share of at
    least 0.5, and the sets' builder leaves at most 30 % of them empty (its p_empty) up to the
    sampling error of a large draw."""
    for M in (1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 257):
        for F, A in ((192, 5), (64, 2)):
            for gather in (False, True):
                for weights in (None, "random"):
                    c = kh.case(M, F, A, gather, "cpu", weights=weights, sets=sets)
                    assert kh.labelled_share(c) >= 0.5, (M, F, A, gather, weights)
    for A in range(1, 9):
        c = kh.case(129, 64, A, True, "cpu", weights="random", sets=sets)
        assert kh.labelled_share(c) >= 0.5, A
    if sets:
        s = bs.random_sets(np.random.default_rng(0), (100000,), 6)
        assert abs(float(((s & 63) == 0).mean()) - 0.3) < 0.01
    c = kh.case(129, 64, 6, True, "cpu", weights="zero", sets=sets)
    assert kh.labelled_share(c) == 0.0


# ------------------------------------------------------------------ 2. known answers: the torch path
def _learner(M, A, weight, sets=False, zero_heads=False, seed=3, **kw):
    """A feed-forward KickstartLearner on an M-sample buffer ([T = M, N = 1]), unclipped: the
    gradients left in .grad are the loss's own."""
    from voxnav.imitate import KickstartLearner
    pol = bh.small_policy(False)
    if zero_heads:
        with torch.no_grad():
            for p in list(pol.action_net.parameters()) + list(pol.value_net.parameters()):
                p.zero_()
    b = bh.dagger_arrays(M, 1, 16, False, seed=seed)
    b["label_weight"] = weight
    if weight is None:
        del b["label_weight"]
    if sets:
        b["expert_set"] = bs.random_sets(np.random.default_rng(seed), (M, 1), A)
    ln = KickstartLearner(pol, n_epochs=1, batch_size=M, max_grad_norm=1e9, labels="set" if sets else "action", **kw)
    return pol, b, ln


def _grads(pol):
    return [p.grad.detach().clone() for p in pol.parameters()]


def _ppo_grads(M, seed=3):
    """The plain PPOLearner's stats and gradients on the same policy and buffer."""
    from voxnav.ppo import PPOLearner
    pol = bh.small_policy(False)
    b = bh.dagger_arrays(M, 1, 16, False, seed=seed)
    ln = PPOLearner(pol, n_epochs=1, batch_size=M, max_grad_norm=1e9)
    st = ln.train(bh.as_dagger_buffer(b, "cpu"), epoch_orders=[np.arange(M)])
    return st, _grads(pol)


def test_torch_path_zero_heads_give_ln_A():
    M, A = 12, 6
    pol, b, ln = _learner(M, A, None, zero_heads=True, bc_coef=0.5)
    st = ln.train(kh.kickstart_buffer(b, "cpu", False), epoch_orders=[np.arange(M)])
    assert abs(st["bc_loss"] - math.log(A)) < 1e-6 and abs(st["entropy_loss"] + math.log(A)) < 1e-6
    assert st["labelled"] == 1.0
    lab = b["expert_actions"].reshape(-1)
    assert abs(st["accuracy"] - float((lab == 0).mean())) < 1e-12        # every logit ties: the argmax is index 0
    want = st["policy_gradient_loss"] + ln.ent_coef * st["entropy_loss"] + ln.vf_coef * st["value_loss"] + \
        0.5 * math.log(A)
    assert abs(st["loss"] - want) < 1e-6
    assert st["n_minibatches"] == 1 and st["n_updates"] == 1


@pytest.mark.parametrize("sets", [False, True], ids=["action", "set"])
def test_torch_path_reduces_to_ppo(sets):
    """bc_coef = 0, and all-zero weights under any bc_coef: PPOLearner's stats and gradients."""
    M, A = 12, 6
    pst, pg = _ppo_grads(M)
    for bc_coef, weight in ((0.0, None), (2.5, np.zeros((M, 1), np.uint8))):
        pol, b, ln = _learner(M, A, weight, sets=sets, bc_coef=bc_coef)
        st = ln.train(kh.kickstart_buffer(b, "cpu", sets), epoch_orders=[np.arange(M)])
        for k in ("policy_gradient_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction",
                  "grad_norm", "explained_variance"):
            assert abs(st[k] - pst[k]) <= 1e-6 * max(1.0, abs(pst[k])), (k, st[k], pst[k])
        for a, g in zip(_grads(pol), pg):
            assert float((a - g).abs().max()) <= 1e-7
        if weight is not None:
            assert st["bc_loss"] == 0.0 and st["accuracy"] == 0.0 and st["labelled"] == 0.0


# ------------------------------------------------------------------ 3. the learner vs the restatement
@pytest.mark.parametrize("sets", [False, True], ids=["action", "set"])
@pytest.mark.parametrize("recurrent", [True, False], ids=["lstm", "mlp"])
def test_kickstart_learner_matches_restatement_cpu(recurrent, sets):
    """tests/test_imitate_cpu.py's shapes and bounds: T = 12, N = 5, batch 16, 2 epochs, LSTM 16 /
    MLP [32, 16]; episode starts at p = 0.15, ~20 % of the label weights zero, 30 % of the sets empty."""
    kh.run_kickstart_parity("cpu", recurrent, sets)


# ------------------------------------------------------------------ 4. refusals
def test_train_refuses_a_buffer_without_labels():
    from voxnav.collector import RolloutBuffer
    from voxnav.imitate import KickstartLearner
    b = bh.as_dagger_buffer(bh.dagger_arrays(4, 2, 16, False), "cpu")
    plain = RolloutBuffer(**{k: getattr(b, k) for k in RolloutBuffer.__dataclass_fields__})
    with pytest.raises(ValueError, match="expert_actions"):
        KickstartLearner(bh.small_policy(False)).train(plain)
    with pytest.raises(ValueError, match="expert_set"):
        KickstartLearner(bh.small_policy(False), labels="set").train(b)


def test_train_refuses_an_executed_expert_action():
    from voxnav.imitate import KickstartLearner
    b = kh.kickstart_buffer(bh.dagger_arrays(4, 2, 16, False), "cpu", False)
    pol = bh.small_policy(False)
    w0 = [p.detach().clone() for p in pol.parameters()]
    ln = KickstartLearner(pol, n_epochs=1, batch_size=8)
    b.took_expert[2, 1] = 1
    with pytest.raises(ValueError, match="beta = 0"):
        ln.train(b)
    assert ln.n_updates == 0 and all(torch.equal(a, p) for a, p in zip(w0, pol.parameters()))
    b.took_expert[2, 1] = 0
    assert ln.train(b)["n_minibatches"] == 1


def test_bc_coef_is_checked():
    from voxnav.imitate import KickstartLearner
    pol = bh.small_policy(False)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bc_coef"):
            KickstartLearner(pol, bc_coef=bad)
    ln = KickstartLearner(pol)
    assert ln.bc_coef == 1.0 and ln.labels == "action"
    ln.set_bc_coef(0.25)
    assert ln.bc_coef == 0.25
    with pytest.raises(ValueError, match="bc_coef"):
        ln.set_bc_coef(-1.0)


# ------------------------------------------------------------------ 5. kickstart()'s history
class _Collector:
    """A CPU stand-in for ``DaggerCollector``: synthetic rollouts of [T, N], the attributes the
    loop reads."""

    def __init__(self, policy, T, N):
        self.policy, self.n_steps, self.N = policy, T, N
        self.beta, self.rollouts, self.synced = 1.0, 0, 0

    def set_beta(self, beta):
        self.beta = float(beta)

    def collect(self):
        assert self.beta == 0.0                                 # the loop set it before the first rollout
        self.rollouts += 1
        return kh.kickstart_buffer(bh.dagger_arrays(self.n_steps, self.N, 16, False, seed=self.rollouts), "cpu", False)

    def sync_weights(self):
        self.synced += 1


def test_kickstart_history_follows_the_schedule():
    from voxnav import KickstartLearner, kickstart
    from voxnav.imitate import KickstartLearner as KL
    assert KickstartLearner is KL
    T, N = 6, 4
    pol = bh.small_policy(False)
    col = _Collector(pol, T, N)
    ln = KickstartLearner(pol, n_epochs=1, batch_size=8, bc_coef=9.0)
    seen = []
    hist = kickstart(col, ln, total_timesteps=3 * T * N - 1, bc_coef=lambda i: 0.5 ** i,
                     callback=lambda it, done, st: seen.append((it, done, st["bc_coef"])))
    assert len(hist) == 3 and col.rollouts == 3 and col.synced == 3
    assert [h["bc_coef"] for h in hist] == [1.0, 0.5, 0.25] and ln.bc_coef == 0.25
    assert [h["num_timesteps"] for h in hist] == [T * N, 2 * T * N, 3 * T * N]
    assert seen == [(1, T * N, 1.0), (2, 2 * T * N, 0.5), (3, 3 * T * N, 0.25)]
    keys = {"policy_gradient_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction", "grad_norm",
            "explained_variance", "n_minibatches", "n_updates", "bc_loss", "accuracy", "labelled", "bc_coef",
            "num_timesteps"}
    for h in hist:
        assert keys <= set(h), keys - set(h)
        assert h["n_minibatches"] == 3
    # a constant coefficient, and a callback that stops the loop
    hist = kickstart(col, ln, total_timesteps=10 * T * N, bc_coef=0.3, callback=lambda it, done, st: it < 2)
    assert [h["bc_coef"] for h in hist] == [0.3, 0.3]
    with pytest.raises(ValueError, match="share the policy"):
        kickstart(_Collector(bh.small_policy(False), T, N), ln, total_timesteps=1)
