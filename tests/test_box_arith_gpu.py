"""The BOX step kernels (csrc/voxnav_env.hip, env_kernel's BOX argument): for
an env whose every room vn_create has proven an exact box, the plane-set step
kernels compute each ray record from the agent's coordinates and its room's
size instead of loading it.  Everything here is compared bit for bit with the
float64 oracle: obs, rewards, flags, the exported state and the belief.

Shapes (small on purpose; the oracle of a case is computed once, with
checkpoints after 1, 24 and 128 steps, and shared read-only):
  rooms   3x3x3 (one free cell: every move bumps, every extent is 0, an
          auto-reset at every step), 5x5x4 (18 free cells: many auto-resets in
          64 steps), 8x8x4 (H < PH), 16x16x8, 32x32x8, 40x33x8 (the u64 plane
          rows of kernel mode 1)
  L       1, 4, 10: rays that end short of L and beyond it
  agents  1, 13 (a partial wave), 80 (a full wave and a partial one)
  mixes   [1], [16, 1, 7], [128] steps per launch
  calls   random policy / explicit actions, each as the rollout-buffer call
          (the FAST kernel) and with f64 rewards (the other one)
Which kernel a call takes is asserted through kernel_label and kernel_box
(vn_kernel_box: the label stops before the BOX argument).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CUTS = (1, 24, 128)                                   # oracle checkpoints = the totals of the launch mixes
MIXES = {1: [1], 24: [16, 1, 7], 128: [128]}
PRIO_TABLE = 8                                        # VnTuning::prio: a box-exact env stays on the ray table

# (room W, D, H), L, agents -- every room with two of the L values and two of the agent counts
CASES = [((3, 3, 3), 1, 1), ((3, 3, 3), 4, 13),
         ((5, 5, 4), 4, 80), ((5, 5, 4), 10, 13),
         ((8, 8, 4), 1, 80), ((8, 8, 4), 10, 13),
         ((16, 16, 8), 4, 13), ((16, 16, 8), 10, 1),
         ((32, 32, 8), 10, 80), ((32, 32, 8), 1, 13),
         ((40, 33, 8), 10, 80), ((40, 33, 8), 4, 1)]
CALLS = [("random", True), ("random", False), ("explicit", True), ("explicit", False)]   # (policy, FAST)


@pytest.fixture(scope="module")
def voxnav():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import voxnav
    voxnav.load_library()
    return voxnav


def room_text(W, D, H, pillar=None):
    """A box of one wall layer; pillar=(x, y): that interior column walled from floor to ceiling."""
    lines = [f"Size={W},{D},{H}"]
    for z in range(H):
        lines.append(f"Layer z={z}")
        for y in range(D):
            lines.append(" ".join(
                "2" if (x in (0, W - 1) or y in (0, D - 1) or z in (0, H - 1) or (x, y) == pillar) else "0"
                for x in range(W)))
    return "\n".join(lines) + "\n"


def texts_of(rooms):
    """rooms: tuple of (W, D, H) or (W, D, H, px, py) -> [(file name, text)], in the set's order."""
    return [("room%d_%s.txt" % (i, "x".join(map(str, r))), room_text(*r[:3], pillar=tuple(r[3:]) or None))
            for i, r in enumerate(rooms)]


def make_env(rooms, L, N, **kw):
    from voxnav.env import BatchedGridEnv
    from voxnav.rooms import RoomSet, parse_room
    rs = RoomSet([parse_room(t, n) for n, t in texts_of(rooms)], use_room_draw=True, source="test")
    return BatchedGridEnv(num_agents=N, rooms=rs, local_map_length=L, autoreset=True, device="cuda:0", **kw)


def actions_of(N):
    return np.random.default_rng(1000 + N).integers(0, 6, size=(CUTS[-1], N)).astype(np.int32)


_ORACLE = {}


def oracle_run(rooms, L, N, policy):
    """The oracle's 128 steps of (rooms, L, N) under the Philox policy or the explicit actions, with
    the state and belief after 1, 24 and 128 steps.  Computed once per key; read-only."""
    key = (rooms, L, N, policy)
    if key not in _ORACLE:
        from oracle.oracle import OracleEnv, parse_room_text
        env = OracleEnv([parse_room_text(t, n) for n, t in texts_of(rooms)], n_agents=N, local_map_length=L,
                        use_room_draw=True)
        seeds = 42 + np.arange(N, dtype=np.int64)
        acts = actions_of(N) if policy == "explicit" else None
        parts, marks, t = [], {}, 0
        for cut in CUTS:
            parts.append(env.run_random(seeds, policy_seed=7, K=cut - t, t0=t, seed_stride=N, initial_reset=t == 0,
                                        actions=None if acts is None else acts[t:cut]))
            t = cut
            state = np.array([[env.state(a)[f] for f in list(env.state(0))[:14]] for a in range(N)], dtype=np.int64)
            marks[cut] = (state, [np.minimum(env.belief(a), 63) for a in range(N)])
        out = {k: np.concatenate([p[k] for p in parts]) for k in ("obs", "reward", "terminated", "truncated", "actions")}
        for v in out.values():
            v.setflags(write=False)
        _ORACLE[key] = (out, marks)
    return _ORACLE[key]


def launch(env, k, t, policy, fast, N):
    """One launch of k steps from launch step t -> (obs, reward, terminated, truncated, actions or None)."""
    if policy == "random" and fast:       # the rollout-buffer call, into a caller's buffer
        from voxnav.env import Rollout
        out = Rollout(torch.empty((k, N, 80), device="cuda:0"), torch.empty((k, N), device="cuda:0"),
                      torch.empty((k, N), dtype=torch.uint8, device="cuda:0"),
                      torch.empty((k, N), dtype=torch.uint8, device="cuda:0"), None)
        ro = env.step_random(k, policy_seed=7, out=out)
    elif policy == "random":              # f64 rewards and the action record
        ro = env.step_random(k, policy_seed=7, reward_f64=True, record_actions=True)
    else:
        at = torch.as_tensor(actions_of(N)[t:t + k], device="cuda:0")
        ro = env.step_actions(at, reward_f64=not fast)
    acts = ro.actions.cpu().numpy() if (policy == "random" and not fast) else None
    return [x.cpu().numpy() for x in (ro.obs, ro.reward, ro.terminated, ro.truncated)] + [acts]


def assert_run(env, chunks, rooms, L, N, policy, fast, total):
    """The launches' outputs, then the exported state and belief, against the oracle's first `total` steps."""
    out, marks = oracle_run(rooms, L, N, policy)
    obs, rew, te, tr = (np.concatenate([c[i] for c in chunks]) for i in range(4))
    assert obs.tobytes() == out["obs"][:total].tobytes(), "obs"
    want_r = out["reward"][:total].astype(np.float32) if fast else out["reward"][:total]
    assert rew.dtype == want_r.dtype
    np.testing.assert_array_equal(rew, want_r, err_msg="reward")
    np.testing.assert_array_equal(te, out["terminated"][:total], err_msg="terminated")
    np.testing.assert_array_equal(tr, out["truncated"][:total], err_msg="truncated")
    if chunks[0][4] is not None:
        np.testing.assert_array_equal(np.concatenate([c[4] for c in chunks]), out["actions"][:total])
    state, belief = marks[total]
    st = env.export_state().cpu().numpy()
    np.testing.assert_array_equal(st[:, :14], state, err_msg="state")
    b = env.belief().cpu().numpy().astype(np.int64)
    shapes = [r[:3] for r in rooms]
    for a in range(N):
        W, D, H = shapes[int(st[a, 13])]
        np.testing.assert_array_equal(b[a, :W, :D, :H], belief[a], err_msg=f"belief of agent {a}")


def run_mix(rooms, L, N, policy, fast, total, want_box, **kw):
    env = make_env(rooms, L, N, **kw)
    try:
        env.reset(seed=42)
        chunks, t = [], 0
        for k in MIXES[total]:
            assert env.kernel_box(k, explicit_actions=policy == "explicit", fast=fast) == want_box, (k, policy, fast)
            chunks.append(launch(env, k, t, policy, fast, N))
            t += k
        assert_run(env, chunks, rooms, L, N, policy, fast, total)
    finally:
        env.close()


@pytest.mark.parametrize("policy,fast", CALLS, ids=["random-fast", "random-f64", "explicit-fast", "explicit-f64"])
@pytest.mark.parametrize("whd,L,N", CASES, ids=["%dx%dx%d-L%d-N%d" % (*c[0], c[1], c[2]) for c in CASES])
def test_boxes_match_the_oracle(voxnav, whd, L, N, policy, fast):
    """Every launch mix of one (room, L, agents, call shape), each from a fresh reset, on the BOX kernels."""
    env = make_env((whd,), L, N)
    pcm = 2 if max(whd[0], whd[1]) <= 32 else 1
    assert env.kernel_label(16, explicit_actions=policy == "explicit", fast=fast) == \
        "env_kernel<8, %s, %s, false, %d>" % ("true" if policy == "explicit" else "false", "true" if fast else "false", pcm)
    env.close()
    for total in CUTS:
        run_mix((whd,), L, N, policy, fast, total, want_box=True)


@pytest.mark.parametrize("policy,fast", [("random", True), ("explicit", False)], ids=["random-fast", "explicit-f64"])
def test_two_boxes_of_different_sizes(voxnav, policy, fast):
    """A set of two boxes with the room draw: the record comes from each agent's own room's size."""
    rooms = ((8, 8, 4), (5, 6, 3))
    for total in (24, 128):
        run_mix(rooms, 4, 80, policy, fast, total, want_box=True)
    out, marks = oracle_run(rooms, 4, 80, policy)
    assert len(set(marks[128][0][:, 13])) == 2, "both rooms drawn"


@pytest.mark.parametrize("policy,fast", [("random", True), ("explicit", False)], ids=["random-fast", "explicit-f64"])
def test_box_and_pillar_room_stay_on_the_table(voxnav, policy, fast):
    """One room of the set is no box: no call of the env takes a BOX kernel, whatever the bit says."""
    rooms = ((8, 8, 4), (8, 8, 4, 4, 3))
    env = make_env(rooms, 4, 80)
    for prio in (67, 67 | PRIO_TABLE):
        env.set_tuning(prio=prio)
        for k in (0, 1, 16, 128):
            for ext in (False, True):
                for f in (False, True):
                    assert not env.kernel_box(k, explicit_actions=ext, fast=f)
    assert env.kernel_label(16) == "env_kernel<8, false, true, false, 2>"
    env.close()
    for total in (24, 128):
        run_mix(rooms, 4, 80, policy, fast, total, want_box=False)


def test_which_calls_take_the_box_kernels(voxnav):
    """A box-exact env: BOX exactly when the bit is clear, for every step shape; never for a reset, for
    the deferred-flush instantiation, or in the byte-mark modes.  The label itself does not change."""
    env = make_env(((32, 32, 8),), 10, 64)
    for prio, want in ((67, True), (67 | PRIO_TABLE, False), (3, True), (3 | PRIO_TABLE, False)):
        env.set_tuning(prio=prio)
        for k in (1, 7, 128):
            for ext in (False, True):
                for f in (False, True):
                    assert env.kernel_box(k, explicit_actions=ext, fast=f) == want, (prio, k, ext, f)
                    assert env.kernel_label(k, explicit_actions=ext, fast=f) == \
                        "env_kernel<8, %s, %s, false, 2>" % ("true" if ext else "false", "true" if f else "false")
        assert not env.kernel_box(0)
    env.set_tuning(prio=67, dflush=3)               # the deferred flush in the plane-set kernels: stays on the table
    assert env.kernel_label(16).endswith(", 2, true>") and not env.kernel_box(16)
    assert env.kernel_box(1) and env.kernel_box(16, explicit_actions=True)   # (no deferred flush for these)
    env.close()
    env = make_env(((32, 32, 8),), 10, 64, tuning={"pcache_cap": 0})          # byte marks (kernel mode 3)
    assert env.kernel_label(1).endswith(", 3>") and not env.kernel_box(1) and not env.kernel_box(16)
    env.close()
    env = make_env(((8, 8, 12),), 4, 16)                                      # PH 16
    assert env.kernel_label(16).startswith("env_kernel<16,") and not env.kernel_box(16)
    env.close()


def test_flipping_the_bit_in_mid_episode(voxnav):
    """One env flips the bit between the launches of an episode, a second one never sets it, a third
    always: the three trajectories are the oracle's, and each other's."""
    rooms, L, N = ((32, 32, 8),), 10, 80
    ks = [16, 1, 7, 40, 64]
    runs = []
    for prios in ([67, 67 | PRIO_TABLE, 67, 67 | PRIO_TABLE, 67], [67] * 5, [67 | PRIO_TABLE] * 5):
        env = make_env(rooms, L, N)
        env.reset(seed=42)
        chunks, t = [], 0
        for k, prio in zip(ks, prios):
            env.set_tuning(prio=prio)
            assert env.kernel_box(k) == (not prio & PRIO_TABLE)
            chunks.append(launch(env, k, t, "random", True, N))
            t += k
        assert_run(env, chunks, rooms, L, N, "random", True, sum(ks))
        runs.append((np.concatenate([c[0] for c in chunks]), env.export_state().cpu().numpy(),
                     env.belief().cpu().numpy()))
        env.close()
    for other in runs[1:]:
        assert runs[0][0].tobytes() == other[0].tobytes()
        np.testing.assert_array_equal(runs[0][1], other[1])
        np.testing.assert_array_equal(runs[0][2], other[2])
