"""Invalid-action masking end to end on the GPU: a masked collector never
bumps (and the same seeds without masks do), every stored action lies inside
its stored mask, ``PPOLearner(action_masks=True)`` takes the fused masked
kernel and matches the float64 restatement, ``ppo.learn`` / checkpoints /
``evaluate_policy`` / ``VoxnavVecEnv.action_masks`` work with it, and the
refusals."""
import numpy as np
import pytest
import torch

import mask_helpers as mh
from helpers import archive_texts

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, T = 64, 64


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _rooms(which):
    from voxnav import rooms as R
    if which == "box":
        return R.single_room_set(R.box_room(8, 8, 4))
    name = "P2_training/maze_8x8_seed22.txt"
    return R.single_room_set(R.parse_room(archive_texts()[name], "maze_8x8_seed22.txt"))


def _env(which, n=N):
    from voxnav.env import BatchedGridEnv
    return BatchedGridEnv(num_agents=n, rooms=_rooms(which), local_map_length=4, autoreset=True, device=DEV)


def _policy(recurrent, seed=0):
    from voxnav.policy import ActorCriticPolicy, RecurrentActorCriticPolicy
    torch.manual_seed(seed)
    return (RecurrentActorCriticPolicy() if recurrent else ActorCriticPolicy()).to(DEV)


def _bumps(env):
    """bumps of every ended episode plus those of the running ones"""
    return int(env.episode_totals()[3]) + int(env.state()["bump_count"].sum())


@pytest.mark.parametrize("which", ["box", "maze"])
def test_masked_rollouts_never_bump(which):
    from voxnav.collector import MaskedRolloutBuffer, RolloutCollector
    pol = _policy(True)
    env = _env(which)
    try:
        col = RolloutCollector(env, pol, n_steps=T, sample_seed=5, reset_seed=11, action_masks=True)
        assert not col.w.mlp_head                                   # the fused head is bypassed
        for _ in range(2):
            buf = col.collect()
            assert isinstance(buf, MaskedRolloutBuffer) and buf.action_masks.shape == (T, N)
            assert buf.action_masks.dtype == torch.uint8
            inside = (buf.action_masks.long() >> buf.actions.long()) & 1
            assert bool((inside == 1).all())
            want = mh.mask_reference(buf.obs.reshape(T * N, 80).cpu().numpy())
            assert buf.action_masks.reshape(-1).cpu().numpy().tolist() == want.tolist()
            assert bool(torch.isfinite(buf.log_probs).all()) and bool((buf.log_probs <= 0).all())
        assert int(env.episode_totals()[3]) == 0 and int(env.state()["bump_count"].sum()) == 0
        assert int((buf.action_masks != 63).sum()) > 0              # and the masks did forbid something
    finally:
        env.close()
    # the same seeds without masks bump: the assertion above can fail
    env = _env(which)
    try:
        col = RolloutCollector(env, pol, n_steps=T, sample_seed=5, reset_seed=11)
        for _ in range(2):
            col.collect()
        assert _bumps(env) >= 1
    finally:
        env.close()


def test_train_takes_the_fused_masked_kernel_and_matches_float64():
    """One train() of the reference's MLP policy on a masked rollout against
    the float64 restatement (mask_helpers.masked_train_reference), to
    test_ppo's full-size GPU bounds (5e-5 + 1e-3 relative on the parameters,
    1e-4 relative on the logged losses)."""
    from voxnav.collector import RolloutCollector
    from voxnav.ppo import PPOLearner
    pol = _policy(False, seed=1)
    env = _env("box")
    try:
        buf = RolloutCollector(env, pol, n_steps=T, sample_seed=6, reset_seed=12, action_masks=True).collect()
        rng = np.random.default_rng(3)
        orders = [rng.permutation(T * N)]
        ref, logs = mh.masked_train_reference(pol, buf, orders, 512)
        ln = PPOLearner(pol, n_epochs=1, batch_size=512, action_masks=True)
        st = ln.train(buf, epoch_orders=orders)
        assert ln.masked_fused_updates == st["n_minibatches"] == len(logs) == 8
        got = {k: v.detach().cpu().double() for k, v in pol.state_dict().items()}
        for k, v in ref.state_dict().items():
            np.testing.assert_allclose(got[k].numpy(), v.numpy(), atol=5e-5, rtol=1e-3, err_msg=k)
        for key in ("policy_gradient_loss", "value_loss", "entropy_loss", "loss"):
            want = np.mean([s[key] for s in logs])
            assert abs(st[key] - want) <= 1e-4 * max(1.0, abs(want)), (key, st[key], want)
    finally:
        env.close()


def test_learn_iteration_and_checkpoint_round_trip(tmp_path):
    from voxnav import ppo
    from voxnav.checkpoint import load_checkpoint, save_checkpoint
    from voxnav.collector import RolloutCollector
    from voxnav.ppo import PPOLearner
    pol = _policy(True, seed=2)
    w0 = [p.detach().clone() for p in pol.parameters()]
    env = _env("maze")
    try:
        col = RolloutCollector(env, pol, n_steps=T, sample_seed=7, reset_seed=13, action_masks=True)
        ln = PPOLearner(pol, n_epochs=1, batch_size=1024, action_masks=True)
        hist = ppo.learn(col, ln, total_timesteps=T * N)
        assert len(hist) == 1 and ln.masked_fused_updates == hist[0]["n_minibatches"] == 4
        assert all(np.isfinite(hist[0][k]) for k in ("loss", "entropy_loss", "approx_kl", "grad_norm"))
        assert any(not torch.equal(p.detach(), w) for p, w in zip(pol.parameters(), w0))
        assert _bumps(env) == 0
        path = save_checkpoint(tmp_path / "masked", pol, ln.optimizer, num_timesteps=T * N)
        pol2, data = load_checkpoint(path, device=DEV)
        assert data["num_timesteps"] == T * N
        for (k, a), b in zip(pol.state_dict().items(), pol2.state_dict().values()):
            assert torch.equal(a, b), k
        # the reloaded policy collects on: the next rollout still never bumps
        col2 = RolloutCollector(env, pol2, n_steps=8, sample_seed=7, reset_seed=14, action_masks=True)
        env.clear_episode_records()
        col2.collect()
        assert _bumps(env) == 0
        # a plain buffer is refused by the masked learner
        plain = RolloutCollector(env, pol, n_steps=8).collect()
        with pytest.raises(ValueError, match="action_masks"):
            ln.train(plain)
    finally:
        env.close()


def test_evaluate_policy_with_masks_reports_no_bumps():
    from voxnav.evaluate import EvalCallback, evaluate_policy
    pol = _policy(True, seed=3)
    r = evaluate_policy(pol, _rooms("maze"), n_episodes=10, local_map_length=4, seed=21, device=DEV,
                        action_masks=True)
    assert r["avg_bumps"] == 0.0 and r["avg_steps"] > 0
    r0 = evaluate_policy(pol, _rooms("maze"), n_episodes=10, local_map_length=4, seed=21, device=DEV)
    assert r0["avg_bumps"] > 0.0
    cb = EvalCallback(_rooms("maze"), eval_freq=1, n_eval_episodes=4, local_map_length=4, device=DEV,
                      action_masks=True)
    assert cb.on_rollout_end(pol, 64, 1)["eval/mean_ep_length"] > 0


def test_vec_env_and_facade_masks():
    from voxnav.gym_api import GridAgent
    from voxnav.vec_env import VoxnavVecEnv
    ve = VoxnavVecEnv(8, rooms=_rooms("maze"), local_map_length=4, seed=31, device=DEV)
    try:
        with pytest.raises(RuntimeError):
            ve.action_masks()                                       # no observation yet
        obs = ve.reset()
        rng = np.random.default_rng(0)
        for _ in range(6):
            m = ve.action_masks()
            assert m.dtype == np.bool_ and m.shape == (8, 6)
            want = (mh.mask_reference(obs)[:, None] >> np.arange(6)) & 1
            assert (m == want.astype(bool)).all()
            lst = ve.env_method("action_masks")
            assert len(lst) == 8 and all(x.shape == (6,) and (x == m[i]).all() for i, x in enumerate(lst))
            assert (ve.env_method("action_masks", indices=[5])[0] == m[5]).all()
            # a random allowed action per env never bumps
            b0 = np.asarray(ve.get_attr("bump_count"))
            acts = [int(rng.choice(np.flatnonzero(row))) for row in m]
            obs, _, done, _ = ve.step(acts)
            b1 = np.asarray(ve.get_attr("bump_count"))
            assert ((b1 == b0) | done).all()
    finally:
        ve.close()
    ga = GridAgent(rooms=_rooms("box"), local_map_length=4, device=DEV)
    try:
        with pytest.raises(RuntimeError):
            ga.action_masks()
        o, _ = ga.reset(seed=3)
        for _ in range(4):
            m = ga.action_masks()
            assert m.dtype == np.bool_ and m.shape == (6,)
            assert (m == ((int(mh.mask_reference(o)[0]) >> np.arange(6)) & 1).astype(bool)).all()
            blocked = np.flatnonzero(~m)
            a = int(blocked[0]) if blocked.size else 0
            before = ga.bump_count
            o, *_ = ga.step(a)
            assert (ga.bump_count > before) == bool(blocked.size)   # a forbidden action does bump
    finally:
        ga.close()


def test_refusals():
    from voxnav.collector import RolloutCollector
    from voxnav.env import BatchedGridEnv
    from voxnav.imitate import DaggerCollector
    from voxnav.policy import ActorCriticPolicy
    pol = _policy(False)
    env = _env("box", n=8)
    try:
        with pytest.raises(ValueError, match="f32"):
            RolloutCollector(env, pol, n_steps=4, policy_dtype="bf16", action_masks=True)
        with pytest.raises(ValueError, match="action_masks"):
            DaggerCollector(env, pol, n_steps=4, action_masks=True)
    finally:
        env.close()
    simple = BatchedGridEnv(num_agents=8, rooms=_rooms("box"), local_map_length=4, device=DEV, variant="simple")
    try:
        spol = ActorCriticPolicy(obs_dim=simple.obs_dim).to(DEV)
        with pytest.raises(ValueError, match="CubicEnv"):
            RolloutCollector(simple, spol, n_steps=4, action_masks=True)
    finally:
        simple.close()
