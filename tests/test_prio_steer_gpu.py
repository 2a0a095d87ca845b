"""The step kernel's wave priorities (csrc/voxnav_env.hip: VnTuning::prio, the
base level taken from the progress table) and the step loop's every-step
stream change timing only: every priority mode gives the oracle's results, bit
for bit -- obs, rewards, flags, the exported state and the belief.

Co-residency is not reached here: these shapes do not put several waves of a
launch on one SIMD (the dispatcher spreads blocks over the CUs first), so no
wave ever finds a mate's word in its row.  The tests pin that results do not
depend on the table -- its words of earlier launches, of finished waves and of
another env of the device included; what the levels do to the timing is shown
by the measurements (profiles/prio_steer/).
"""
import numpy as np
import pytest

from helpers import oracle_env, product_room_set

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KS = (16, 1, 5, 8, 9)          # crosses the K >= 8 switch in both directions; stale table words between launches
PRIOS = (67, 71, 3, 0)         # closed loop, rotation, no base level, no priorities


@pytest.fixture(scope="module")
def voxnav():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import voxnav
    voxnav.load_library()
    return voxnav


def make_env(src, L, n, **kw):
    from voxnav.env import BatchedGridEnv
    return BatchedGridEnv(num_agents=n, rooms=product_room_set(src), local_map_length=L, autoreset=True,
                          device="cuda:0", **kw)


_ORACLE = {}


def oracle_run(src, L, N, K):
    """The oracle's K random-policy steps of (src, L, N), computed once and shared (read-only)."""
    key = (src, L, N, K)
    if key not in _ORACLE:
        env = oracle_env(src, L, n_agents=N)
        out = env.run_random(42 + np.arange(N, dtype=np.int64), policy_seed=7, K=K, seed_stride=N)
        state = np.array([[env.state(a)[f] for f in list(env.state(0))[:14]] for a in range(N)], dtype=np.int64)
        belief = [np.minimum(env.belief(a), 63) for a in range(N)]
        _ORACLE[key] = (out, state, belief)
    return _ORACLE[key]


def assert_matches_oracle(env, chunks, src, L, N):
    out, state, belief = oracle_run(src, L, N, sum(KS))
    obs, rew, te, tr = (np.concatenate(c) for c in zip(*chunks))
    assert obs.tobytes() == out["obs"].tobytes()
    np.testing.assert_array_equal(rew, out["reward"])
    np.testing.assert_array_equal(te, out["terminated"])
    np.testing.assert_array_equal(tr, out["truncated"])
    st = env.export_state().cpu().numpy()
    np.testing.assert_array_equal(st[:, :14], state)
    b = env.belief().cpu().numpy().astype(np.int64)
    rooms = env.room_set.rooms
    for a in range(N):
        W, D, H = rooms[int(st[a, 13])].shape
        np.testing.assert_array_equal(b[a, :W, :D, :H], belief[a], err_msg=f"agent {a}")


def rollout(env, k):
    ro = env.step_random(k, policy_seed=7, reward_f64=True)
    return [t.cpu().numpy() for t in (ro.obs, ro.reward, ro.terminated, ro.truncated)]


@pytest.mark.parametrize("prio", PRIOS)
def test_all_priority_modes(voxnav, prio):
    """A PH-8 plane-set env, 8 x 8 x 4 box, 40 agents (two full waves and a last
    wave of 8), launches of 16, 1, 5, 8 and 9 steps in one sequence under each
    priority mode.  (No co-residency: see the module docstring.)"""
    src, L, N = "box:8x8x4", 4, 40
    env = make_env(src, L, N, tuning={"prio": prio})
    assert env.kernel_label(16).endswith(", 2>"), env.kernel_label(16)
    env.reset(seed=42)
    assert_matches_oracle(env, [rollout(env, k) for k in KS], src, L, N)


@pytest.mark.parametrize("prio", PRIOS)
def test_two_envs_at_once(voxnav, prio):
    """The same at 32 x 32 x 8, L = 10, 1,037 agents (65 waves, the last of 13
    agents), with a second env of another size alive on the device and stepped
    between the launches: the table then holds words of foreign tags.  (No
    co-residency: see the module docstring.)"""
    src, L, N = "box:32x32x8", 10, 1037
    env = make_env(src, L, N, tuning={"prio": prio})
    other = make_env("box:8x8x4", 4, 200, tuning={"prio": prio})
    env.reset(seed=42)
    other.reset(seed=9)
    chunks = []
    for k in KS:
        chunks.append(rollout(env, k))
        other.step_random(12, policy_seed=3)
    assert_matches_oracle(env, chunks, src, L, N)
    other.close()


def test_plane_rows_to_both_ends(voxnav):
    """u32 plane rows with bit 31 in use: a box 32 wide and 32 deep, 64 agents
    turned towards the four walls (16 each), walked into them and then moved at
    random along them, in explicit-action launches of 32 and 24 steps.  The
    sensing spans then end at row bits 0 and 31 in both planes."""
    src, L, N = "box:32x32x8", 10, 64
    rng = np.random.default_rng(5)
    turn = (np.arange(N) // 16).astype(np.int32)          # fwd +y, right +x, back -y, left -x (facing north)
    acts = np.concatenate([turn[None], np.zeros((31, N), np.int32), rng.integers(0, 6, size=(24, N)).astype(np.int32)])
    env = make_env(src, L, N)
    assert env.kernel_label(16).endswith(", 2>"), env.kernel_label(16)
    env.reset(seed=300)
    orc_env = oracle_env(src, L, n_agents=N)
    orc = orc_env.run_random(300 + np.arange(N), policy_seed=0, K=acts.shape[0], seed_stride=N, actions=acts)
    at = torch.as_tensor(acts, device="cuda:0")
    first = env.step_actions(at[:32], reward_f64=True)
    st = env.export_state().cpu().numpy()
    assert (st[0:16, 1] == 30).all() and (st[16:32, 0] == 30).all() and (st[32:48, 1] == 1).all() \
        and (st[48:64, 0] == 1).all(), "every agent stands against its wall"
    second = env.step_actions(at[32:], reward_f64=True)
    for name, got in (("obs", [first.obs, second.obs]), ("reward", [first.reward, second.reward]),
                      ("terminated", [first.terminated, second.terminated]),
                      ("truncated", [first.truncated, second.truncated])):
        g = np.concatenate([t.cpu().numpy() for t in got])
        if name == "obs":
            assert g.tobytes() == orc["obs"].tobytes()
        else:
            np.testing.assert_array_equal(g, orc[name], err_msg=name)
    st = env.export_state().cpu().numpy()
    want = np.array([[orc_env.state(a)[f] for f in list(orc_env.state(0))[:14]] for a in range(N)], dtype=np.int64)
    np.testing.assert_array_equal(st[:, :14], want)
    b = env.belief().cpu().numpy().astype(np.int64)
    for a in range(N):
        np.testing.assert_array_equal(b[a, :32, :32, :8], np.minimum(orc_env.belief(a), 63), err_msg=f"agent {a}")
