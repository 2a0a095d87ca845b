"""Kickstarted PPO on the GPU: ``DaggerCollector(beta=0)`` + ``KickstartLearner`` (the fused kernel
``learn_ops.ppo_bc_loss`` / ``ppo_bc_loss_set``, csrc/voxnav_ppo_bc_loss.hip) against the restated
train call of tests/kickstart_helpers.py on the collector's own rollout, ``kickstart`` end to end,
and the refusal of a rollout in which the planner's action was executed.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bc_helpers as bh  # noqa: E402
import kickstart_helpers as kh  # noqa: E402
from helpers import product_room_set  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMS = pytest.mark.parametrize("labels", ["action", "set"])


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def np_(t):
    return t.detach().cpu().numpy()


def _collector(pol, labels, beta=0.0, N=8, T=16):
    from voxnav.env import BatchedGridEnv
    from voxnav.imitate import DaggerCollector
    env = BatchedGridEnv(num_agents=N, rooms=product_room_set("box:8x8x4"), local_map_length=4, device=DEV)
    return env, DaggerCollector(env, pol, n_steps=T, beta=beta, labels=labels)


def _arrays(buf, sets):
    names = ["obs", "actions", "episode_starts", "values", "log_probs", "advantages", "returns", "expert_actions",
             "label_weight"] + (["expert_set"] if sets else []) + (["lstm_h", "lstm_c"] if buf.lstm_h is not None else [])
    return {k: np_(getattr(buf, k)).copy() for k in names}


def _parity(recurrent, labels, batch_size, epochs, arch, lstm, bc_coef=0.7, atol=2e-5, rtol=1e-4):
    """``KickstartLearner.train`` on a rollout of the 8x8x4 box (N = 8, T = 16, beta = 0) against
    ``kickstart_train`` on the same arrays, within ``BCLearner``'s GPU bounds
    (tests/test_imitate_gpu.py: parameters atol 2e-5 + rtol 1e-4, logged values 1e-4 relative)."""
    from voxnav.imitate import KickstartLearner
    from voxnav.policy import numpy_weights
    sets = labels == "set"
    pol = bh.small_policy(recurrent, arch, lstm).to(DEV)
    env, col = _collector(pol, labels)
    buf = col.collect()
    T, N = buf.actions.shape
    assert int(buf.took_expert.sum()) == 0
    w0, b = numpy_weights(pol), _arrays(buf, sets)
    rng = np.random.default_rng(7)
    orders = ([int(rng.integers(T * N)) for _ in range(epochs)] if recurrent
              else [rng.permutation(T * N) for _ in range(epochs)])
    ln = KickstartLearner(pol, n_epochs=epochs, batch_size=batch_size, bc_coef=bc_coef, labels=labels)
    st = ln.train(buf, epoch_orders=orders)
    w1, ost = kh.kickstart_train(w0, b, orders, batch_size=batch_size, bc_coef=bc_coef, sets=sets)
    got = numpy_weights(pol)
    moved = 0.0
    for k in w1:
        np.testing.assert_allclose(got[k], w1[k], atol=atol, rtol=rtol, err_msg=k)
        moved = max(moved, float(np.abs(w1[k] - w0[k]).max()))
    assert moved > 1e-4                                 # the update did something
    n = len(ost)
    assert st["n_minibatches"] == n == epochs * -(-T * N // batch_size) and st["n_updates"] == n
    names = dict(policy_loss="policy_gradient_loss")
    for key in kh.STAT_KEYS + ("grad_norm",):
        ref = float(np.mean([s[key] for s in ost]))
        val = st[names.get(key, key)]
        print(f"{key}: learner {val!r} restatement {ref!r}")
        assert abs(val - ref) <= 1e-4 * max(1.0, abs(ref)), (key, val, ref)
    assert st["labelled"] >= 0.5
    assert ln.fused_updates == n > 0                    # every minibatch went through the fused kernel
    env.close()
    return ln, ost


@FORMS
@pytest.mark.parametrize("recurrent", [True, False], ids=["lstm", "mlp"])
def test_kickstart_learner_matches_restatement_gpu(recurrent, labels):
    """LSTM 16 / MLP [32, 64] (a latent width the fused kernel takes), batch 32, 2 epochs."""
    _parity(recurrent, labels, batch_size=32, epochs=2, arch=(32, 64), lstm=16)


@FORMS
def test_kickstart_learner_whole_rollout_takes_the_row_layout_lstm(labels):
    """One minibatch = the whole rollout (T = 16, N = 8), LSTM 256 (the width the row-layout kernels
    take), MLP [64]: the LSTMs re-run in the row layout, the loss in the fused kernel."""
    ln, ost = _parity(True, labels, batch_size=128, epochs=1, arch=(64,), lstm=256)
    assert ln.fused_updates == len(ost) == 1
    assert any(ln.__dict__.get("_rows_cache", {}).values()), "the row layout must be the path under test"


def test_train_refuses_a_rollout_with_executed_planner_actions():
    from voxnav.imitate import KickstartLearner
    pol = bh.small_policy(False, arch=(32, 64)).to(DEV)
    env, col = _collector(pol, "action", beta=0.5)
    buf = col.collect()
    assert int(buf.took_expert.sum()) > 0
    ln = KickstartLearner(pol, n_epochs=1, batch_size=32)
    with pytest.raises(ValueError, match="beta = 0"):
        ln.train(buf)
    assert ln.n_updates == 0 and ln.fused_updates == 0
    col.set_beta(0.0)
    assert ln.train(col.collect())["n_minibatches"] == 4
    env.close()


@FORMS
def test_kickstart_end_to_end(tmp_path, labels):
    """8x8x4 box, 8 agents x 16 steps, an MLP policy [64, 64]: two iterations with bc_coef = 1, 0.5
    (the collector starts at beta = 1 and the loop sets it to 0), a checkpoint round trip, then one
    plain ``ppo.learn`` iteration on the same module."""
    from voxnav.checkpoint import load_checkpoint, save_checkpoint
    from voxnav.collector import RolloutCollector
    from voxnav.env import BatchedGridEnv
    from voxnav.imitate import KickstartLearner, kickstart
    from voxnav.ppo import PPOLearner, learn
    N, T, iters = 8, 16, 2
    pol = bh.small_policy(False, arch=(64, 64), seed=2).to(DEV)
    env, col = _collector(pol, labels, beta=1.0, N=N, T=T)
    ln = KickstartLearner(pol, n_epochs=1, batch_size=64, seed=1, labels=labels)
    seen = []
    hist = kickstart(col, ln, total_timesteps=iters * N * T, bc_coef=lambda i: 0.5 ** i,
                     callback=lambda it, done, st: seen.append((it, done)))
    assert col.beta == 0.0 and len(hist) == iters and seen == [(i + 1, (i + 1) * N * T) for i in range(iters)]
    keys = {"policy_gradient_loss", "value_loss", "entropy_loss", "loss", "approx_kl", "clip_fraction", "grad_norm",
            "explained_variance", "n_minibatches", "n_updates", "bc_loss", "accuracy", "labelled", "bc_coef",
            "num_timesteps"}
    for i, h in enumerate(hist):
        assert keys <= set(h), keys - set(h)
        assert h["bc_coef"] == 0.5 ** i and h["num_timesteps"] == (i + 1) * N * T and h["n_minibatches"] == 2
        assert all(np.isfinite(h[k]) for k in keys - {"explained_variance"})
        assert 0.0 <= h["bc_loss"] <= np.log(6) + 0.5 and 0.0 <= h["accuracy"] <= 1.0 and 0.5 <= h["labelled"] <= 1.0
    print([(round(h["loss"], 3), round(h["bc_loss"], 3), round(h["accuracy"], 3)) for h in hist])
    assert ln.fused_updates == iters * 2 and ln.bc_coef == 0.5
    path = save_checkpoint(tmp_path / "kick.zip", pol, ln.optimizer, num_timesteps=hist[-1]["num_timesteps"])
    pol2, data = load_checkpoint(path, device=DEV)
    assert data["num_timesteps"] == iters * N * T
    for a, b in zip(pol.parameters(), pol2.parameters()):
        assert torch.equal(a, b)
    env.close()
    # the same module goes on under plain PPO
    env2 = BatchedGridEnv(num_agents=N, rooms=product_room_set("box:8x8x4"), local_map_length=4, device=DEV)
    w0 = torch.cat([p.detach().reshape(-1).clone() for p in pol.parameters()])
    ph = learn(RolloutCollector(env2, pol, n_steps=T), PPOLearner(pol, n_epochs=2, batch_size=64, seed=1),
               total_timesteps=N * T)
    assert len(ph) == 1 and np.isfinite(ph[0]["loss"])
    assert float((torch.cat([p.detach().reshape(-1) for p in pol.parameters()]) - w0).abs().max()) > 1e-5
    env2.close()
