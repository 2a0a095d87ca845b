"""Masked DAgger and masked kickstart end to end on the GPU, at
test_masked_ppo_gpu's shapes (64 agents x 64 steps, L = 4, the 8x8x4 box and maze_8x8_seed22, an
untrained LSTM policy): a ``MaskedDaggerCollector`` never bumps at any beta (and the same seeds on a
plain ``DaggerCollector`` do), everything it stores lies inside its masks, ``BCLearner`` and
``KickstartLearner`` with ``action_masks=True`` take the fused masked kernels and the row-layout LSTM
and match the float64 restatements of tests/masked_imitate_helpers.py, and ``warm_start`` /
``kickstart`` / ``evaluate_policy`` / checkpoints / ``ppo.learn`` run with the new classes."""
import numpy as np
import pytest
import torch

import bc_helpers as bh
import mask_helpers as mh
import masked_imitate_helpers as mi
from test_masked_ppo_gpu import DEV, N, T, _bumps, _env, _policy, _rooms

pytestmark = pytest.mark.gpu

FORMS = pytest.mark.parametrize("labels", ["action", "set"])


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _inside(masks, actions):
    return ((masks.long() >> actions.long()) & 1) == 1


# ------------------------------------------------------------------ 1. rollouts
@FORMS
@pytest.mark.parametrize("which", ["box", "maze"])
def test_masked_dagger_rollouts_never_bump(which, labels):
    from voxnav.collector import MaskedRolloutBuffer
    from voxnav.imitate import DaggerBuffer, DaggerCollector, MaskedDaggerBuffer, MaskedDaggerCollector
    pol = _policy(True)
    env = _env(which)
    narrow = 0
    try:
        col = MaskedDaggerCollector(env, pol, n_steps=T, sample_seed=5, reset_seed=11, labels=labels)
        assert not col.w.mlp_head                                   # the fused head is bypassed
        for beta in (0.0, 0.5, 1.0):
            col.set_beta(beta)
            for _ in range(2):
                buf = col.collect()
                assert isinstance(buf, MaskedDaggerBuffer) and isinstance(buf, DaggerBuffer)
                assert isinstance(buf, MaskedRolloutBuffer)
                m = buf.action_masks
                assert m.shape == (T, N) and m.dtype == torch.uint8
                lab = buf.label_weight != 0
                assert bool(_inside(m, buf.actions).all()) and bool(_inside(m, buf.policy_actions).all())
                assert bool(_inside(m, buf.expert_actions)[lab].all()) and int(lab.sum()) > T * N // 2
                if labels == "set":
                    assert int((buf.expert_set & ~m).sum()) == 0 and bool((buf.expert_set[lab] != 0).all())
                want = mh.mask_reference(buf.obs.reshape(T * N, 80).cpu().numpy())
                assert m.reshape(-1).cpu().numpy().tolist() == want.tolist()
                took = int(buf.took_expert.sum())
                assert (took == 0 if beta == 0.0 else took == int(lab.sum()) if beta == 1.0
                        else 0 < took < int(lab.sum())), (beta, took)
                narrow += int((m != 63).sum())
                assert _bumps(env) == 0, beta                       # episode totals plus the running counts
        assert narrow > 0                                           # and the masks did forbid something
    finally:
        env.close()
    # the same seeds without masks bump: the assertion above can fail
    env = _env(which)
    try:
        col = DaggerCollector(env, pol, n_steps=T, sample_seed=5, reset_seed=11, labels=labels, beta=0.0)
        for _ in range(2):
            col.collect()
        assert _bumps(env) >= 1
    finally:
        env.close()


# ------------------------------------------------------------------ 2. learners against float64
PT, PN = 16, 8        # the part of the rollout the float64 restatement re-runs (test_kickstart_gpu's size)


@pytest.fixture(scope="module")
def rollout():
    """One beta = 0 rollout of the box at the shapes above with ``labels="set"`` (it carries the
    planner's action too), and its first PT steps of the first PN agents as arrays: what both
    learners and both label forms train on.  Collected once, never written."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from voxnav.imitate import MaskedDaggerBuffer, MaskedDaggerCollector
    pol = _policy(True, seed=4)
    env = _env("box")
    try:
        buf = MaskedDaggerCollector(env, pol, n_steps=T, sample_seed=6, reset_seed=12, labels="set", beta=0.0).collect()
        cut = {}
        for k in buf.__dataclass_fields__:
            v = getattr(buf, k)
            if v is None or v.dim() < 2 or v.shape[0] != T:
                continue                                            # (last_values, dones: per agent only)
            cut[k] = (v[:PT, :, :PN] if k in ("lstm_h", "lstm_c") else v[:PT, :PN]).clone()
        part = MaskedDaggerBuffer(**cut)
        assert int(part.took_expert.sum()) == 0 and int((part.action_masks != 63).sum()) > 0
        assert float((part.label_weight != 0).float().mean()) >= 0.5
        return pol.state_dict(), part, {k: v.cpu().numpy() for k, v in cut.items()}
    finally:
        env.close()


@FORMS
@pytest.mark.parametrize("which", ["bc", "kickstart"])
def test_masked_learners_match_float64_on_the_fused_path(rollout, which, labels):
    """One minibatch = the whole part (PT x PN = 128 samples) of the reference's LSTM 256 policy:
    the LSTMs re-run in the row layout, the loss in the fused masked kernel.  Bounds as
    tests/test_imitate_gpu.py / tests/test_kickstart_gpu.py: parameters atol 2e-5 + rtol 1e-4, logged
    values 1e-4 relative."""
    from voxnav.imitate import BCLearner, KickstartLearner
    from voxnav.policy import numpy_weights
    state, part, b = rollout
    sets = labels == "set"
    pol = _policy(True, seed=4)
    pol.load_state_dict(state)
    w0 = numpy_weights(pol)
    orders = [37]
    if which == "bc":
        ln = BCLearner(pol, n_epochs=1, batch_size=PT * PN, labels=labels, action_masks=True)
        w1, ost = mi.masked_bc_train(w0, b, orders, sets=sets, batch_size=PT * PN)
        keys, names = mi.BC_KEYS, {}
    else:
        ln = KickstartLearner(pol, n_epochs=1, batch_size=PT * PN, bc_coef=0.7, labels=labels, action_masks=True)
        w1, ost = mi.masked_kickstart_train(w0, b, orders, sets=sets, batch_size=PT * PN, bc_coef=0.7)
        keys, names = mi.KS_KEYS, dict(policy_loss="policy_gradient_loss")
    st = ln.train(part, epoch_orders=orders)
    got = numpy_weights(pol)
    moved = 0.0
    for k in w1:
        np.testing.assert_allclose(got[k], w1[k], atol=2e-5, rtol=1e-4, err_msg=k)
        moved = max(moved, float(np.abs(w1[k] - w0[k]).max()))
    assert moved > 1e-4                                 # the update did something
    for key in keys + ("grad_norm",):
        ref = float(np.mean([s[key] for s in ost]))
        val = st[names.get(key, key)]
        print(f"{key}: learner {val!r} restatement {ref!r}")
        assert abs(val - ref) <= 1e-4 * max(1.0, abs(ref)), (key, val, ref)
    assert st["labelled"] >= 0.5
    assert ln.masked_fused_updates == ln.fused_updates == st["n_minibatches"] == len(ost) == 1
    assert any(ln.__dict__.get("_rows_cache", {}).values()), "the row layout must be the path under test"


# ------------------------------------------------------------------ 3. end to end
@FORMS
def test_warm_start_kickstart_evaluate_checkpoint_and_masked_ppo(tmp_path, labels):
    from voxnav import ppo
    from voxnav.checkpoint import load_checkpoint, save_checkpoint
    from voxnav.evaluate import EvalCallback, evaluate_policy
    from voxnav.imitate import BCLearner, KickstartLearner, MaskedDaggerCollector, kickstart, warm_start
    from voxnav.ppo import PPOLearner
    pol = _policy(True, seed=2)
    w0 = [p.detach().clone() for p in pol.parameters()]
    env = _env("maze")
    try:
        col = MaskedDaggerCollector(env, pol, n_steps=T, sample_seed=7, reset_seed=13, labels=labels)
        bl = BCLearner(pol, n_epochs=1, batch_size=1024, labels=labels, action_masks=True)
        cb = EvalCallback(_rooms("maze"), eval_freq=1, n_eval_episodes=4, local_map_length=4, device=DEV,
                          action_masks=True)
        hist = warm_start(col, bl, total_timesteps=2 * T * N, beta=lambda i: 1.0 - 0.5 * i, callback=cb)
        assert [h["beta"] for h in hist] == [1.0, 0.5] and bl.masked_fused_updates == bl.fused_updates == 8
        assert all(np.isfinite(h[k]) for h in hist for k in ("loss", "bc_loss", "accuracy", "grad_norm"))
        assert hist[0]["expert_share"] == pytest.approx(hist[0]["labelled"], abs=1e-6)
        kl = KickstartLearner(pol, n_epochs=1, batch_size=1024, labels=labels, action_masks=True)
        khist = kickstart(col, kl, total_timesteps=2 * T * N, bc_coef=lambda i: 0.5 ** i)
        assert col.beta == 0.0 and [h["bc_coef"] for h in khist] == [1.0, 0.5]
        assert kl.masked_fused_updates == kl.fused_updates == 8
        assert all(np.isfinite(h[k]) for h in khist for k in ("loss", "bc_loss", "approx_kl", "accuracy", "grad_norm"))
        assert any(not torch.equal(p.detach(), w) for p, w in zip(pol.parameters(), w0))
        assert _bumps(env) == 0                                     # four rollouts at beta 1, 0.5, 0, 0
        r = evaluate_policy(pol, _rooms("maze"), n_episodes=10, local_map_length=4, seed=21, device=DEV,
                            action_masks=True)
        assert r["avg_bumps"] == 0.0 and r["avg_steps"] > 0
        path = save_checkpoint(tmp_path / "masked_imitate", pol, kl.optimizer, num_timesteps=4 * T * N)
        pol2, data = load_checkpoint(path, device=DEV)
        assert data["num_timesteps"] == 4 * T * N
        for (k, a), b in zip(pol.state_dict().items(), pol2.state_dict().values()):
            assert torch.equal(a, b), k
        # a masked ppo.learn iteration on the same collector: its buffer is a MaskedRolloutBuffer too
        pl = PPOLearner(pol, n_epochs=1, batch_size=1024, action_masks=True)
        ph = ppo.learn(col, pl, total_timesteps=T * N)
        assert len(ph) == 1 and pl.masked_fused_updates == ph[0]["n_minibatches"] == 4 and np.isfinite(ph[0]["loss"])
        assert _bumps(env) == 0
        # a rollout with executed planner actions is no PPO buffer, masked or not
        col.set_beta(0.5)
        buf = col.collect()
        assert int(buf.took_expert.sum()) > 0
        n0 = kl.n_updates
        with pytest.raises(ValueError, match="beta = 0"):
            kl.train(buf)
        assert kl.n_updates == n0
    finally:
        env.close()
