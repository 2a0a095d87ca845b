"""``target_kl``, ``clip_range_vf`` and the schedules off the GPU (voxnav.ppo's
torch path, voxnav.imitate's learners; tests/trust_helpers.py's float64
restatements): the learner against the float64 ``train()`` with sb3's early-stop
loop and value clip, to test_ppo.py's CPU bounds (parameters 2e-5 + 1e-4
relative, logged means 1e-4 relative); what must be bit-identical to the learner
without the keywords; the schedules through ``ppo.learn``; every refusal."""
import copy
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bc_helpers as bh  # noqa: E402
import kickstart_helpers as kh  # noqa: E402
import trust_helpers as th  # noqa: E402
from test_ppo import _as_rollout, _buffer, _policy  # noqa: E402

T, N, BATCH = 12, 5, 16
PER_EPOCH = -(-T * N // BATCH)


def _orders(recurrent, epochs, first=None):
    rng = np.random.default_rng(7)
    o = [int(rng.integers(T * N)) for _ in range(epochs)] if recurrent else [rng.permutation(T * N)
                                                                            for _ in range(epochs)]
    if first is not None:
        o[0] = first
    return o


def _assert_params(pol, want, atol=2e-5, rtol=1e-4):
    from voxnav.policy import numpy_weights
    got = numpy_weights(pol)
    for k in want:
        np.testing.assert_allclose(got[k], want[k], atol=atol, rtol=rtol, err_msg=k)


# ------------------------------------------------------------------ 1. the restatement's own rule
def test_gate_rule_table():
    assert th.gate_rule(0, 0.1, 0.2, None) == (1, 0, 0)
    assert th.gate_rule(0, 0.2, 0.2, None) == (1, 0, 0)            # strict
    assert th.gate_rule(0, 0.3, 0.2, None) == (1, 1, 1)            # logged, not stepped
    assert th.gate_rule(1, 0.0, 0.2, None) == (0, 1, 1)            # sticky: neither
    assert th.gate_rule(0, float("nan"), 0.2, 0) == (1, 0, 0)
    assert th.gate_rule(0, 0.1, 0.2, 7) == (1, 0, 1)               # the error word alone skips, and does not stop


def test_reference_value_clip_equals_the_clamp_form():
    """sb3's old + clamp(v - old, -c, c) and clamp(v, old - c, old + c) agree to rounding,
    with the gradient on the inclusive range in both."""
    g = torch.Generator().manual_seed(0)
    v = torch.randn(64, generator=g, dtype=torch.float64, requires_grad=True)
    old = torch.randn(64, generator=g, dtype=torch.float64)
    a = old + torch.clamp(v - old, -0.5, 0.5)
    b = torch.clamp(v, old - 0.5, old + 0.5)
    assert float((a - b).detach().abs().max()) < 1e-15
    ga, = torch.autograd.grad(a.sum(), v)
    gb, = torch.autograd.grad(b.sum(), v)
    assert torch.equal(ga, gb) and 0 < float(ga.sum()) < 64


# ------------------------------------------------------------------ 2. the torch path against float64
@pytest.mark.parametrize("recurrent", [True, False], ids=["lstm", "mlp"])
def test_value_clip_matches_float64_cpu(recurrent):
    from voxnav.policy import numpy_weights
    from voxnav.ppo import PPOLearner
    pol = _policy(recurrent)
    w0 = numpy_weights(pol)
    b = _buffer(T, N, 16, recurrent)
    orders = _orders(recurrent, 2)
    ln = PPOLearner(pol, n_epochs=2, batch_size=BATCH, clip_range_vf=0.5)
    st = ln.train(_as_rollout(b, "cpu"), epoch_orders=orders)
    w1, rows, _, info = th.train_reference(w0, b, orders, batch_size=BATCH, clip_range_vf=0.5)
    _assert_params(pol, w1)
    th.assert_logged_means(st, rows)
    assert st["n_minibatches"] == len(rows) == 2 * PER_EPOCH == st["n_updates"] == info["n_steps"]
    assert st["early_stop"] is False and st["epochs_run"] == 2
    # the clip took part: the unclipped value loss is another number
    _, rows0, _, _ = th.train_reference(w0, b, orders, batch_size=BATCH)
    assert abs(rows0[0]["value_loss"] - rows[0]["value_loss"]) > 1e-2 * rows0[0]["value_loss"]


@pytest.mark.parametrize("recurrent", [True, False], ids=["lstm", "mlp"])
def test_target_kl_stops_where_float64_stops_cpu(recurrent):
    """A buffer the policy itself collected (old log-probs = its own): the first
    minibatch's KL is 0 and never stops; the threshold is put between the KL of a
    later minibatch k (of the float64 run without target_kl) and every KL before it."""
    from voxnav.policy import numpy_weights
    from voxnav.ppo import PPOLearner
    pol = _policy(recurrent)
    w0 = numpy_weights(pol)
    b = _buffer(T, N, 16, recurrent)
    b["log_probs"] = th.own_log_probs(w0, b)
    epochs = 3
    orders = _orders(recurrent, epochs, first=0 if recurrent else None)
    _, dry, _, _ = th.train_reference(w0, b, orders, batch_size=BATCH)
    kls = [r["approx_kl"] for r in dry]
    assert abs(kls[0]) < 1e-12
    k, target = th.crossing(kls)
    assert k >= 1
    ln = PPOLearner(pol, n_epochs=epochs, batch_size=BATCH, target_kl=target)
    st = ln.train(_as_rollout(b, "cpu"), epoch_orders=orders)
    w1, rows, _, info = th.train_reference(w0, b, orders, batch_size=BATCH, target_kl=target)
    assert info["early_stop"] and info["n_steps"] == k and len(rows) == k + 1
    assert st["early_stop"] is True and st["epochs_run"] == info["epochs_run"] == k // PER_EPOCH + 1
    assert st["n_minibatches"] == k + 1 and st["n_updates"] == ln.n_updates == k
    _assert_params(pol, w1)
    th.assert_logged_means(st, rows)                  # the crossing minibatch is among the logged
    assert all(float(ln.optimizer.state[p]["step"]) == k for p in pol.parameters() if p.grad is not None)
    # the next train() starts afresh (the stop is not sticky across calls)
    st2 = ln.train(_as_rollout(b, "cpu"), epoch_orders=orders[:1])
    assert st2["n_minibatches"] >= 1 and ln.n_updates >= k


@pytest.mark.parametrize("recurrent", [True, False], ids=["lstm", "mlp"])
def test_target_kl_crossed_by_the_first_minibatch_changes_nothing(recurrent):
    """Old log-probs that are not the policy's: minibatch 0 of epoch 0 crosses a tiny
    threshold; it is logged, nothing is stepped."""
    from voxnav.policy import numpy_weights
    from voxnav.ppo import PPOLearner
    pol = _policy(recurrent)
    w0 = numpy_weights(pol)
    p0 = [p.detach().clone() for p in pol.parameters()]
    b = _buffer(T, N, 16, recurrent)
    orders = _orders(recurrent, 2)
    ln = PPOLearner(pol, n_epochs=2, batch_size=BATCH, target_kl=1e-9)
    st = ln.train(_as_rollout(b, "cpu"), epoch_orders=orders)
    assert st["early_stop"] is True and st["epochs_run"] == 1
    assert st["n_minibatches"] == 1 and st["n_updates"] == 0 and ln.n_updates == 0
    for p, q in zip(pol.parameters(), p0):
        assert torch.equal(p.detach(), q)
    assert len(ln.optimizer.state) == 0               # Adam's moments and step: as constructed
    _, rows, _, info = th.train_reference(w0, b, orders, batch_size=BATCH, target_kl=1e-9)
    assert len(rows) == 1 and info["n_steps"] == 0 and rows[0]["approx_kl"] > 1.5e-9
    th.assert_logged_means(st, rows)


# ------------------------------------------------------------------ 3. what must not change a bit
@pytest.mark.parametrize("recurrent", [True, False], ids=["lstm", "mlp"])
def test_huge_target_kl_and_infinite_value_clip_are_bit_identical(recurrent):
    from voxnav.ppo import PPOLearner
    b = _buffer(T, N, 16, recurrent)
    orders = _orders(recurrent, 2)
    pol0 = _policy(recurrent)
    pol1 = copy.deepcopy(pol0)
    st0 = PPOLearner(pol0, n_epochs=2, batch_size=BATCH).train(_as_rollout(b, "cpu"), epoch_orders=orders)
    ln1 = PPOLearner(pol1, n_epochs=2, batch_size=BATCH, target_kl=1e30, clip_range_vf=math.inf)
    st1 = ln1.train(_as_rollout(b, "cpu"), epoch_orders=orders)
    for p, q in zip(pol0.parameters(), pol1.parameters()):
        assert torch.equal(p, q)
    for k in st0:
        assert st0[k] == st1[k] or (math.isnan(st0[k]) and math.isnan(st1[k])), k
    assert st1["early_stop"] is False and st1["epochs_run"] == 2


# ------------------------------------------------------------------ 4. schedules
class _Collector:
    """``collect()`` hands out the same buffer (what ``ppo.run_loop`` needs of a collector)."""

    def __init__(self, policy, buf):
        self.policy, self.buf = policy, buf
        self.n_steps, self.N = buf.actions.shape
        self.rollouts = 0

    def collect(self):
        self.rollouts += 1
        return self.buf

    def sync_weights(self):
        pass


def test_schedules_through_learn():
    """Three iterations: the schedules are evaluated at 1 - done / total with the
    rollout counted (2/3, 1/3, 0); a learning rate of 0.0 leaves the parameters' bits."""
    from voxnav.ppo import PPOLearner, learn
    pol = _policy(False)
    buf = _as_rollout(_buffer(T, N, 16, False), "cpu")
    asked = []

    def lr(p):
        asked.append(p)
        return 0.0 if abs(p - 1 / 3) < 1e-9 else 1e-3 * (0.5 + p)

    ln = PPOLearner(pol, learning_rate=lr, n_epochs=1, batch_size=BATCH, clip_range=lambda p: 0.1 + 0.1 * p,
                    clip_range_vf=lambda p: 0.25 + p)
    assert ln.lr == 1.5e-3 and ln.clip_range == 0.2 and ln.clip_range_vf == 1.25      # their values at 1
    seen, snaps = [], []
    train = ln.train

    def spy(b, *a, **k):
        seen.append((ln.optimizer.param_groups[0]["lr"], ln.lr, ln.clip_range, ln.clip_range_vf))
        snaps.append([p.detach().clone() for p in pol.parameters()])
        return train(b, *a, **k)

    ln.train = spy
    hist = learn(_Collector(pol, buf), ln, total_timesteps=3 * T * N)
    snaps.append([p.detach().clone() for p in pol.parameters()])
    assert len(hist) == 3
    ps = [1 - (i + 1) / 3 for i in range(3)]
    assert [s[0] for s in seen] == [s[1] for s in seen] == [lr(p) for p in ps]
    assert [s[2] for s in seen] == [0.1 + 0.1 * p for p in ps]
    assert [s[3] for s in seen] == [0.25 + p for p in ps]
    assert asked[0] == 1.0 and all(0.0 <= p <= 1.0 for p in asked)
    moved = [any(not torch.equal(a, b) for a, b in zip(snaps[i], snaps[i + 1])) for i in range(3)]
    assert moved == [True, False, True]               # lr 0.0 in the second iteration


def test_float_hyperparameters_make_set_progress_a_no_op():
    from voxnav.ppo import PPOLearner
    ln = PPOLearner(_policy(False), learning_rate=2e-4, clip_range=0.3, clip_range_vf=0.7)
    ln.optimizer.param_groups[0]["lr"] = 5e-4         # set by hand: a float schedule leaves it
    ln.set_progress(0.25)
    assert ln.optimizer.param_groups[0]["lr"] == 5e-4 and ln.lr == 2e-4
    assert ln.clip_range == 0.3 and ln.clip_range_vf == 0.7
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="progress_remaining"):
            ln.set_progress(bad)


def test_scheduled_learning_rate_matches_float64_cpu():
    """Two train() calls at different scheduled rates, one Adam state: the float64 run
    with the same per-call rates."""
    from voxnav.policy import numpy_weights
    from voxnav.ppo import PPOLearner
    pol = _policy(False)
    w = numpy_weights(pol)
    b = _buffer(T, N, 16, False)
    orders = _orders(False, 1)
    ln = PPOLearner(pol, learning_rate=lambda p: 1e-3 * p, n_epochs=1, batch_size=BATCH)
    adam = None
    for p in (0.5, 0.0):
        ln.set_progress(p)
        ln.train(_as_rollout(b, "cpu"), epoch_orders=orders)
        w, _, adam, _ = th.train_reference(w, b, orders, batch_size=BATCH, learning_rate=1e-3 * p, adam=adam)
    _assert_params(pol, w)


# ------------------------------------------------------------------ 5. the imitation learners
def test_kickstart_learner_takes_target_kl_cpu():
    from voxnav.imitate import KickstartLearner
    M = 24
    pol = bh.small_policy(False)
    p0 = [p.detach().clone() for p in pol.parameters()]
    b = bh.dagger_arrays(M, 1, 16, False, seed=3)
    buf = kh.kickstart_buffer(b, "cpu", False)
    ln = KickstartLearner(pol, n_epochs=2, batch_size=8, bc_coef=0.5, target_kl=1e-9)
    st = ln.train(buf, epoch_orders=[np.arange(M), np.arange(M)])
    assert st["early_stop"] is True and st["epochs_run"] == 1 and st["n_minibatches"] == 1 and st["n_updates"] == 0
    assert st["approx_kl"] > 1.5e-9 and np.isfinite(st["bc_loss"])
    for p, q in zip(pol.parameters(), p0):
        assert torch.equal(p.detach(), q)
    # and a threshold nothing reaches: the learner without it, bit for bit
    pol1, pol2 = bh.small_policy(False), bh.small_policy(False)
    o = [np.arange(M)[::-1].copy(), np.arange(M)]
    s1 = KickstartLearner(pol1, n_epochs=2, batch_size=8, bc_coef=0.5).train(buf, epoch_orders=o)
    s2 = KickstartLearner(pol2, n_epochs=2, batch_size=8, bc_coef=0.5, target_kl=1e30).train(buf, epoch_orders=o)
    assert all(torch.equal(p, q) for p, q in zip(pol1.parameters(), pol2.parameters()))
    assert s1["loss"] == s2["loss"] and s2["n_minibatches"] == 6 and s2["early_stop"] is False


# ------------------------------------------------------------------ 6. refusals
def test_refusals():
    from voxnav import learn_ops
    from voxnav.imitate import BCLearner, KickstartLearner
    from voxnav.ppo import PPOLearner
    pol = _policy(False)
    for bad in (0.0, -0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="target_kl"):
            PPOLearner(pol, target_kl=bad)
        with pytest.raises(ValueError, match="target_kl"):
            KickstartLearner(pol, target_kl=bad)
    for bad in (0.0, -0.2, float("nan")):
        with pytest.raises(ValueError, match="clip_range_vf"):
            PPOLearner(pol, clip_range_vf=bad)
        with pytest.raises(ValueError, match="clip_range_vf"):
            PPOLearner(pol, clip_range_vf=lambda p, bad=bad: bad)
    ln = PPOLearner(pol, clip_range_vf=lambda p: p)           # 0 at the end of training
    with pytest.raises(ValueError, match="clip_range_vf"):
        ln.set_progress(0.0)
    assert PPOLearner(pol, clip_range_vf=float("inf")).clip_range_vf == math.inf
    with pytest.raises(ValueError, match="clip_range_vf"):
        KickstartLearner(pol, clip_range_vf=0.2)
    with pytest.raises(ValueError, match="BCLearner takes no target_kl"):
        BCLearner(pol, target_kl=0.02)
    with pytest.raises(ValueError, match="BCLearner takes no target_kl"):
        BCLearner(pol, clip_range_vf=0.2)
    # the wrappers refuse before anything is launched
    lin = torch.nn.Linear(64, 6)
    h = torch.zeros(2, 4, 64)
    z = torch.zeros(4)
    zi = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match="old_values is required"):
        learn_ops.ppo_loss_vclip(h, lin, torch.nn.Linear(64, 1), None, zi, z, z, z, None, 0.2, 0.5, 0.01, 0.5, True)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="clip_range_vf must be > 0"):
            learn_ops.ppo_loss_vclip(h, lin, torch.nn.Linear(64, 1), None, zi, z, z, z, z, 0.2, bad, 0.01, 0.5, True)
        with pytest.raises(ValueError, match="clip_range_vf must be > 0"):
            learn_ops.ppo_loss_masked_vclip(h, lin, torch.nn.Linear(64, 1), None, zi, z, z, z,
                                            torch.zeros(4, dtype=torch.uint8), z, 0.2, bad, 0.01, 0.5, True)
    with pytest.raises(ValueError, match="action_masks is required"):
        learn_ops.ppo_loss_masked_vclip(h, lin, torch.nn.Linear(64, 1), None, zi, z, z, z, None, z, 0.2, 0.5, 0.01,
                                        0.5, True)
    stats = torch.zeros(6, dtype=torch.float64)
    word = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="stats must be"):
        learn_ops.kl_gate(stats.float(), 0.03, word, word.clone())
    with pytest.raises(ValueError, match="stop must be"):
        learn_ops.kl_gate(stats, 0.03, word.long(), word)
    with pytest.raises(ValueError, match="ran must be"):
        learn_ops.kl_gate(stats, 0.03, word, word.clone(), ran=word.clone())
    with pytest.raises(ValueError, match="kl_index"):
        learn_ops.kl_gate(stats, 0.03, word, word.clone(), kl_index=6)
