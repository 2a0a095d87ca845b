"""The step loop's LDS phases (csrc/voxnav_env.hip: the window words read in
sense_observe, the plane-row word, the wave's obs flush) against the oracle,
at the shapes where a restructured read or store mask can go wrong
(DESIGN 7.16).

A window word is the 4 bytes [z - 2, z + 1] of a tile column, zeros outside
the column: checked at every z of PH-8, PH-16 and PH-32 rooms.  The flush
stores only the float4s of present agents: checked with last waves of 1 and
13 agents, with the bytes behind the last agent's rows poisoned.  Both flush
orders (in-step and deferred) run in the plane-set kernel.  Everything is
bit-exact: obs bytes, rewards, flags, and the exported belief.
"""
import numpy as np
import pytest

from helpers import oracle_env, product_room_set

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def voxnav():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import voxnav
    voxnav.load_library()
    return voxnav


def make_env(voxnav, src, L, n, **kw):
    from voxnav.env import BatchedGridEnv
    return BatchedGridEnv(num_agents=n, rooms=product_room_set(src), local_map_length=L, autoreset=True,
                          device="cuda:0", **kw)


def assert_belief_matches(env, orc_env, N):
    b = env.belief().cpu().numpy().astype(np.int64)
    st = env.export_state().cpu().numpy()
    rooms = env.room_set.rooms
    for a in range(N):
        W, D, H = rooms[int(st[a, 13])].shape
        np.testing.assert_array_equal(b[a, :W, :D, :H], np.minimum(orc_env.belief(a), 63), err_msg=f"agent {a}")


# ---- window word at every z ----
def sweep_actions(H, N, seed):
    """Up over the full height (H steps: the last ones bump at the ceiling),
    a horizontal move, down over the full height, a horizontal move -- twice.
    The horizontal moves are drawn per agent, so the agents' columns differ."""
    rng = np.random.default_rng(seed)
    blocks = []
    for vertical in (4, 5, 4, 5):
        blocks.append(np.full((H, N), vertical, dtype=np.int32))
        blocks.append(rng.integers(0, 4, size=(1, N)).astype(np.int32))
    return np.concatenate(blocks)


# (room, tuning): PH 8 in plane-set mode (u32 and u64 rows) and in byte-mark mode (deferred marks auto / off)
WINDOW_CASES = [("box:6x6x8", {"pcache_cap": 2}), ("box:6x6x8", {"pcache_cap": 1}),
                ("box:6x6x8", {"pcache_cap": 0, "defer": -1}), ("box:6x6x8", {"pcache_cap": 0, "defer": 0}),
                ("box:6x6x16", None), ("box:6x6x31", None)]   # PH 32: the library's tallest room is 31


@pytest.mark.parametrize("src,tuning", WINDOW_CASES,
                         ids=[c[0] + ("" if c[1] is None else "-" + "-".join(f"{k}{v}" for k, v in c[1].items()))
                              for c in WINDOW_CASES])
def test_window_word_at_every_z(voxnav, src, tuning):
    """16 agents swept over the room's full height twice by explicit up / down
    actions: the window [z - 2, z + 1] reaches below the floor (z - 2 < 0), the
    column's last dword and past its top (z + 1 = H - 1 with the window's end
    clamped) for each column height (PH 8, 16 and 32; the PH-32 room is 31 high,
    the tallest the library accepts, so its z + 1 reaches the last dword but not
    the clamp).  Obs, f64 rewards and flags of every step
    and the exported belief at the end equal the oracle's."""
    L, N = 4, 16
    H = int(src.rsplit("x", 1)[1])
    acts = sweep_actions(H, N, seed=H)
    K = acts.shape[0]
    env = make_env(voxnav, src, L, N, **({} if tuning is None else {"tuning": tuning}))
    env.reset(seed=300)
    orc_env = oracle_env(src, L, n_agents=N)
    orc = orc_env.run_random(300 + np.arange(N), policy_seed=0, K=K, seed_stride=N, actions=acts, terminal_obs=True)
    at = torch.as_tensor(acts, device="cuda:0")
    zs = set()
    for k in range(K):
        res = env.step(at[k], reward_f64=True, terminal_obs=True)
        assert res.obs.cpu().numpy().tobytes() == orc["obs"][k].tobytes(), f"obs, step {k}"
        np.testing.assert_array_equal(res.reward.cpu().numpy(), orc["reward"][k], err_msg=f"step {k}")
        np.testing.assert_array_equal(res.terminated.cpu().numpy(), orc["terminated"][k].astype(bool))
        np.testing.assert_array_equal(res.truncated.cpu().numpy(), orc["truncated"][k].astype(bool))
        zs.update(env.export_state().cpu().numpy()[:, 2].tolist())
    assert zs >= set(range(1, H - 1)), "the sweep visits every free z"
    assert_belief_matches(env, orc_env, N)


# ---- flush masks ----
FLUSH_K = (60, 8, 1, 31)      # an unpoisoned run-in, then 40 steps across the truncation at step 72


@pytest.mark.parametrize("N", [1, 13, 16, 29, 77])
def test_flush_store_masks(voxnav, N):
    """The rollout-buffer call with a last wave of 1 (N = 1, 77), 13 (13, 29)
    and 16 agents: the flush covers the wave's 320 staged words and
    stores only the float4s of present agents (nvalid = 20 / 260 / 320), so
    each of the five stores is fully on, partly masked or fully off in some
    case.  The obs buffer is a view of a poisoned allocation with room for 16
    more rows: every byte behind agent N - 1's last row stays poison, and the
    rows, rewards and flags equal the oracle's through the auto-reset."""
    from voxnav.env import Rollout
    src, L = "box:8x8x4", 4
    env = make_env(voxnav, src, L, N)
    env.reset(seed=42)
    poison = float(np.float32(-12345.5))
    obs, rew, te, tr = [], [], [], []
    for K in FLUSH_K:
        flat = torch.full(((K * N + 16) * 80,), poison, device="cuda:0")
        out = Rollout(flat[:K * N * 80].view(K, N, 80), torch.empty((K, N), device="cuda:0"),
                      torch.empty((K, N), dtype=torch.uint8, device="cuda:0"),
                      torch.empty((K, N), dtype=torch.uint8, device="cuda:0"), None)
        env.step_random(K, policy_seed=7, out=out)
        tail = flat[K * N * 80:].cpu().numpy()
        assert (tail == np.float32(poison)).all(), f"N={N} K={K}: stores behind the last agent's rows"
        obs.append(out.obs.cpu().numpy())
        rew.append(out.reward.cpu().numpy())
        te.append(out.terminated.cpu().numpy())
        tr.append(out.truncated.cpu().numpy())
    orc = oracle_env(src, L, n_agents=N).run_random(42 + np.arange(N, dtype=np.int64), policy_seed=7,
                                                    K=sum(FLUSH_K), seed_stride=N)
    assert orc["truncated"][FLUSH_K[0]:].any() or orc["terminated"][FLUSH_K[0]:].any(), "no auto-reset in the window"
    assert np.concatenate(obs).tobytes() == orc["obs"].tobytes()
    np.testing.assert_array_equal(np.concatenate(rew), orc["reward"].astype(np.float32))
    np.testing.assert_array_equal(np.concatenate(te), orc["terminated"])
    np.testing.assert_array_equal(np.concatenate(tr), orc["truncated"])


# ---- both flush orders ----
@pytest.mark.parametrize("dflush", [0, 3])
def test_both_flush_orders(voxnav, dflush):
    """The plane-set kernel with the flush inside the step (dflush 0) and
    deferred behind the next step's loads (dflush 3), launches of 16, 1, 5
    and 30 steps: obs, f64 rewards, flags and belief equal the oracle's."""
    src, L, N, ks = "box:32x32x8", 10, 64, [16, 1, 5, 30]
    env = make_env(voxnav, src, L, N, tuning={"dflush": dflush})
    label = env.kernel_label(16)
    assert label.endswith("true>") == (dflush == 3), label
    env.reset(seed=42)
    obs, rew, te, tr = [], [], [], []
    for k in ks:
        ro = env.step_random(k, policy_seed=7, reward_f64=True)
        obs.append(ro.obs.cpu().numpy())
        rew.append(ro.reward.cpu().numpy())
        te.append(ro.terminated.cpu().numpy())
        tr.append(ro.truncated.cpu().numpy())
    orc_env = oracle_env(src, L, n_agents=N)
    orc = orc_env.run_random(42 + np.arange(N, dtype=np.int64), policy_seed=7, K=sum(ks), seed_stride=N)
    assert np.concatenate(obs).tobytes() == orc["obs"].tobytes()
    np.testing.assert_array_equal(np.concatenate(rew), orc["reward"])
    np.testing.assert_array_equal(np.concatenate(te), orc["terminated"])
    np.testing.assert_array_equal(np.concatenate(tr), orc["truncated"])
    assert_belief_matches(env, orc_env, N)
