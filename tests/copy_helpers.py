"""Shared pieces of the explicit-action and per-agent-copy GPU tests (test_step_actions_gpu.py,
test_copy_agents_gpu.py, test_branch_gpu.py): envs, oracle runs under given actions, comparisons."""
from __future__ import annotations

import numpy as np

from helpers import oracle_env, product_room_set

MODES = {"0/df1": dict(pcache_cap=0, defer=-1), "0/df0": dict(pcache_cap=0, defer=0),
         "1": dict(pcache_cap=1, defer=-1), "2": dict(pcache_cap=2, defer=-1)}

# simpleEnv: absolute direction (0:+x 1:-x 2:+y 3:-y) of the relative moves forward, right, backward, left by
# facing N, E, S, W (envs/simpleEnv.py:153-158, :224-231); actions 4 / 5 are up / down
REL_DIR = [[2, 0, 3, 1], [0, 3, 1, 2], [3, 1, 2, 0], [1, 2, 0, 3]]


def np_(t):
    return t.cpu().numpy()


def make_env(variant, src, L, n, tuning=None, **kw):
    from voxnav.env import BatchedGridEnv
    return BatchedGridEnv(num_agents=n, rooms=product_room_set(src), local_map_length=L, autoreset=True,
                          device="cuda:0", variant=variant, tuning=tuning, **kw)


def vcode(variant):
    return 1 if variant == "simple" else 0


def oracle_run(variant, src, L, seeds, acts, stride):
    """Agents reset with `seeds`, then acts [K, N] with auto-resets (next seed += stride) -> (rows, oracle env)."""
    seeds = np.asarray(seeds, dtype=np.int64)
    env = oracle_env(src, L, n_agents=len(seeds), variant=vcode(variant))
    orc = env.run_random(seeds, policy_seed=0, K=len(acts), seed_stride=stride, actions=acts, terminal_obs=True)
    return orc, env


def seek_actions(src, L, seeds, K, rng, every=2):
    """Random actions [K, N] in which every `every`-th simpleEnv agent walks to its goal (x, then y, then z) and
    is random after reaching it: goal terminations where random walks would find few."""
    N = len(seeds)
    acts = rng.integers(0, 6, size=(K, N)).astype(np.int32)
    env = oracle_env(src, L, n_agents=N, variant=1)
    for i in range(0, N, every):
        env.reset(i, int(seeds[i]))
        for k in range(K):
            s = env.state(i)
            pos, goal = (s["x"], s["y"], s["z"]), (s["last_bump"], s["near_wall"], s["was_near_wall"])   # fields 9..11
            if pos == goal:
                break
            if pos[0] != goal[0] or pos[1] != goal[1]:
                ax = 0 if pos[0] != goal[0] else 1
                d = 2 * ax + (0 if goal[ax] > pos[ax] else 1)
                a = [r[s["facing"]] for r in REL_DIR].index(d)
            else:
                a = 4 if goal[2] > pos[2] else 5
            acts[k, i] = a
            if env.step(i, a)[2]:
                break
    return acts


def assert_rows(got, orc, what="", agents=None):
    """got: dict of numpy arrays (obs, reward64, reward32, terminated, truncated, terminal_obs; any may be absent)
    [K, N, ...]; orc: OracleEnv.run_random's dict.  `agents`: (got columns, oracle columns)."""
    gi, oi = (slice(None), slice(None)) if agents is None else agents
    te, tr = orc["terminated"][:, oi], orc["truncated"][:, oi]
    if "terminated" in got:
        np.testing.assert_array_equal(got["terminated"][:, gi].astype(np.uint8), te, err_msg=f"{what}: terminated")
        np.testing.assert_array_equal(got["truncated"][:, gi].astype(np.uint8), tr, err_msg=f"{what}: truncated")
    if "reward64" in got:
        np.testing.assert_array_equal(got["reward64"][:, gi], orc["reward"][:, oi], err_msg=f"{what}: f64 reward")
    if "reward32" in got:
        np.testing.assert_array_equal(got["reward32"][:, gi], orc["reward"][:, oi].astype(np.float32),
                                      err_msg=f"{what}: f32 reward")
    if "obs" in got:
        a, b = np.ascontiguousarray(got["obs"][:, gi]), np.ascontiguousarray(orc["obs"][:, oi])
        bad = np.argwhere((a.view(np.uint32) != b.view(np.uint32)).any(-1))
        assert bad.size == 0, f"{what}: obs bytes differ at (step, agent) {bad[:5].tolist()}"
    if "terminal_obs" in got:
        done = (te | tr).astype(bool)
        a, b = got["terminal_obs"][:, gi], orc["terminal_obs"][:, oi]
        assert a[done].tobytes() == b[done].tobytes(), f"{what}: terminal obs rows"
        assert not a[~done].any(), f"{what}: a terminal obs row written where no episode ended"


def assert_exports(env, oenv, what="", agents=None):
    """The env's exported state (all 16 fields) and belief of each agent equal the oracle agent's."""
    st, bl = np_(env.export_state()), np_(env.belief()).astype(np.int64)
    pairs = [(i, i) for i in range(len(st))] if agents is None else list(zip(*agents))
    for gi, oi in pairs:
        o = oenv.state(oi)
        assert [int(v) for v in st[gi]] == list(o.values()), f"{what}: state of agent {gi}: {st[gi].tolist()} vs {o}"
        W, D, H = oenv.rooms[o["room"]].whd
        np.testing.assert_array_equal(bl[gi, :W, :D, :H], np.minimum(oenv.belief(oi), 63),
                                      err_msg=f"{what}: belief of agent {gi}")


def launch_all(env, acts, ks, fast=True):
    """acts [sum(ks), N] in launches of ks steps.  fast: f32 reward + f64 reward + flags + terminal obs (the
    rollout-buffer kernel); else the f64 reward alone with flags and terminal obs (the other instantiation)."""
    import torch
    out = {k: [] for k in (("obs", "reward32", "reward64", "terminated", "truncated", "terminal_obs") if fast else
                           ("obs", "reward64", "terminated", "truncated", "terminal_obs"))}
    at, k0 = torch.as_tensor(acts, device=env.device), 0
    for k in ks:
        if fast:
            r64 = torch.empty((k, env.num_agents), dtype=torch.float64, device=env.device)
            ro = env.step_actions(at[k0:k0 + k], terminal_obs=True, reward64=r64)
            out["reward32"].append(np_(ro.reward))
            out["reward64"].append(np_(r64))
        else:
            ro = env.step_actions(at[k0:k0 + k], reward_f64=True, terminal_obs=True)
            out["reward64"].append(np_(ro.reward))
        assert ro.actions.dtype == torch.int32 and torch.equal(ro.actions, at[k0:k0 + k].to(torch.int32))
        for name, v in (("obs", ro.obs), ("terminated", ro.terminated), ("truncated", ro.truncated),
                        ("terminal_obs", ro.terminal_obs)):
            out[name].append(np_(v))
        k0 += k
    return {k: np.concatenate(v) for k, v in out.items()}
