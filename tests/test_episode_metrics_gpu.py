"""The Python surface of the episode records: learn()'s exploration metrics,
evaluate_policy's episode figures, VoxnavVecEnv's info["exploration"] and the
GridAgent facades' last_episode -- each against a CPU-oracle replay of the
actions the run recorded (exact equality)."""
import numpy as np
import pytest

import episode_helpers as eh
from helpers import box_text

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

BOXES = [(8, 8, 4), (6, 6, 4), (7, 5, 5), (5, 5, 4)]      # tests/test_monitor_gpu.py's rooms


@pytest.fixture(scope="module")
def voxnav():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import voxnav
    voxnav.load_library()
    return voxnav


def _small_policy():
    from voxnav.policy import RecurrentActorCriticPolicy
    torch.manual_seed(4)
    return RecurrentActorCriticPolicy(lstm_hidden_size=16, net_arch=dict(pi=[32, 16], vf=[32, 16])).to("cuda:0")


def test_learn_history_reports_exploration_metrics(voxnav):
    from voxnav.collector import RolloutCollector
    from voxnav.env import BatchedGridEnv
    from voxnav.ppo import PPOLearner, learn
    N, L, T, R = 64, 4, 32, 3
    env = BatchedGridEnv(num_agents=N, rooms=eh.product_boxes(BOXES), local_map_length=L, device="cuda:0")
    pol = _small_policy()
    col = RolloutCollector(env, pol, n_steps=T, sample_seed=3, reset_seed=42)
    ln = PPOLearner(pol, n_epochs=1, batch_size=1024, seed=1)
    acts = []
    hist = learn(col, ln, total_timesteps=R * T * N,
                 callback=lambda it, done, st: acts.append(col.actions.cpu().numpy().copy()))
    assert len(hist) == R == len(acts)
    eo = eh.EpisodeOracle(eh.oracle_boxes(BOXES, N, L), 42 + np.arange(N), N)
    prev = eo.totals()
    seen = 0
    for h, a in zip(hist, acts):
        eo.run(T, actions=a)
        d = [int(v) for v in eo.totals() - prev]
        prev = eo.totals()
        keys = ("ep_finished_rate", "ep_bumps_mean", "ep_discovered_mean", "ep_coverage")
        if d[0] == 0:
            assert not any(k in h for k in keys)
            continue
        seen += 1
        assert h["ep_finished_rate"] == d[1] / d[0]
        assert h["ep_bumps_mean"] == d[3] / d[0]
        assert h["ep_discovered_mean"] == d[4] / d[0]
        assert h["ep_coverage"] == d[4] / d[5]
        assert "ep_rew_mean" in h and "ep_len_mean" in h
    assert seen >= 2, "episodes end in at least two of the three rollouts (18- to 72-step rooms)"
    assert env.episode_totals().tolist() == eo.totals().tolist()
    env.close()


def test_evaluate_policy_reads_the_records_once(voxnav, monkeypatch):
    from oracle.oracle import OracleEnv, parse_room_text
    from voxnav.env import BatchedGridEnv
    from voxnav.evaluate import evaluate_policy
    calls = {"export_state": 0}
    real = BatchedGridEnv.export_state

    def counted(self):
        calls["export_state"] += 1
        return real(self)
    monkeypatch.setattr(BatchedGridEnv, "export_state", counted)
    n, L, seed = 10, 4, 5
    out = evaluate_policy(_small_policy(), eh.product_boxes(BOXES), n_episodes=n, local_map_length=L, seed=seed,
                          record_actions=True)
    assert calls["export_state"] <= 1
    acts = out.pop("actions")
    orc = OracleEnv([parse_room_text(t, nm) for nm, t in eh.box_texts(BOXES)], n_agents=n, local_map_length=L)
    eps = []
    for i in range(n):
        orc.reset(i, seed + i)
        score, steps = 0.0, 0
        for k in range(acts.shape[0]):
            _, r, te, tr = orc.step(i, int(acts[k, i]))
            score += r
            steps += 1
            if te or tr:
                break
        else:
            raise AssertionError("every episode ends within max_steps + 1 steps")
        st = orc.state(i)
        eps.append(dict(score=score, bumps=st["bump_count"], discovered_cells=st["visited_count"],
                        finished=bool(st["done"]), steps=steps))
    want = dict(episodes=eps, avg_score=sum(e["score"] for e in eps) / n, avg_bumps=sum(e["bumps"] for e in eps) / n,
                finished_pct=100.0 * sum(e["finished"] for e in eps) / n,
                avg_discovered=sum(e["discovered_cells"] for e in eps) / n, avg_steps=sum(e["steps"] for e in eps) / n)
    assert out == want


def test_vec_env_info_exploration(voxnav):
    from voxnav.vec_env import VoxnavVecEnv
    N, L, K = 32, 4, 80
    venv = VoxnavVecEnv(N, rooms=eh.product_boxes(BOXES), local_map_length=L, seed=42, device="cuda:0")
    venv.reset()
    eo = eh.EpisodeOracle(eh.oracle_boxes(BOXES, N, L), 42 + np.arange(N), N)
    acts = np.random.default_rng(3).integers(0, 6, size=(K, N))
    ret, length, n_eps = np.zeros(N), np.zeros(N, np.int64), 0
    for k in range(K):
        _, rew, dones, infos = venv.step(acts[k])
        ends = eo.run(1, actions=acts[k:k + 1])
        assert dones.tolist() == (ends > 0).tolist()
        assert np.array_equal(rew, eo.step_rewards[0])
        ret += eo.step_rewards[0]
        length += 1
        for i in range(N):
            d = infos[i]
            if not ends[i]:
                assert "exploration" not in d and "episode" not in d
                continue
            r = eo.rec[i]
            assert d["exploration"] == {"steps": int(r[6]), "bumps": int(r[7]), "discovered_cells": int(r[8]),
                                        "max_steps": int(r[9]), "finished": bool(r[11] & 1), "room": int(r[10])}
            # the Monitor's dict is what it was
            assert set(d["episode"]) == {"r", "l", "t"}
            assert d["episode"]["r"] == round(float(ret[i]), 6) and d["episode"]["l"] == int(length[i])
            assert d["TimeLimit.truncated"] == bool(r[11] == 2)
            ret[i], length[i] = 0.0, 0
            n_eps += 1
    assert n_eps >= N
    venv.close()


@pytest.mark.parametrize("variant", ["cubic", "simple"])
def test_facade_last_episode(voxnav, variant):
    from oracle.oracle import OracleEnv, parse_room_text
    from voxnav.gym_api import GridAgent, SimpleGridAgent
    from voxnav.rooms import RoomSet, parse_room
    name, text = "box5x5x4.txt", box_text(5, 5, 4)
    rooms = RoomSet([parse_room(text, name)], use_room_draw=True, source="box")
    ag = (GridAgent if variant == "cubic" else SimpleGridAgent)(rooms=rooms, local_map_length=4, device="cuda:0")
    orc = OracleEnv([parse_room_text(text, name)], n_agents=1, local_map_length=4, variant=int(variant == "simple"))
    ag.reset(seed=7)
    orc.reset(0, 7)
    assert ag.last_episode is None
    rng = np.random.default_rng(1)
    for _ in range(200):
        a = int(rng.integers(0, 6))
        _, _, te, tr, _ = ag.step(a)
        _, _, ote, otr = orc.step(0, a)
        assert (te, tr) == (ote, otr)
        if te or tr:
            break
        assert ag.last_episode is None
    st = orc.state(0)
    assert ag.last_episode == {"steps": st["step_count"], "bumps": st["bump_count"],
                               "discovered_cells": st["visited_count"], "max_steps": st["max_steps"],
                               "finished": bool(st["done"]), "room": 0, "terminated": te, "truncated": tr}
    ag.close()
