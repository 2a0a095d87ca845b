"""The device-side episode records (vn_episode_records / _totals / _clear):
every finished episode's steps, bumps, discovered cells, max_steps, room and
flags -- what envs/CubicEnv.py:212-222 prints at each episode end and
train/evaluate_grid.py:213-247 tabulates -- written by the step kernels at
the ending step, before any auto-reset.

Bar: exact integer equality with the reference goldens' state rows and with
the CPU oracle's accumulators (tests/episode_helpers.py); no tolerances.
"""
import ctypes

import numpy as np
import pytest

import episode_helpers as eh
from helpers import GOLDEN, load_golden, product_room_set

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

CUBIC_GOLDENS = ["traj_box8x8x4_file_L4_explore", "traj_box8x8x4_ctor_L4_random", "traj_maze3dtunnels_L10_explore"]
SIMPLE_GOLDENS = ["simple_box8x8x4_L4_random", "simple_kitchen2_L10_seek"]
# the belief modes of the CubicEnv kernels (VnTuning): plane sets u32 / u64, byte marks deferred / in the pass
MODES = [None, {"pcache_cap": 1}, {"pcache_cap": 0}, {"pcache_cap": 0, "defer": 0}]
MODE_IDS = ["default", "pcache1", "pcache0", "pcache0-defer0"]


@pytest.fixture(scope="module")
def voxnav():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import voxnav
    voxnav.load_library()
    return voxnav


def make_env(rooms, n, L=4, autoreset=True, **kw):
    from voxnav.env import BatchedGridEnv
    return BatchedGridEnv(num_agents=n, rooms=rooms, local_map_length=L, autoreset=autoreset, device="cuda:0", **kw)


def records(env):
    return env.episode_records().cpu().numpy()


def totals(env):
    return env.episode_totals().cpu().numpy()


# ---------------------------------------------------------------- a. reference goldens
@pytest.mark.parametrize("name", CUBIC_GOLDENS + SIMPLE_GOLDENS)
def test_records_match_reference_goldens(voxnav, name):
    """One agent, autoreset off, manual reset at every end (as
    test_golden_trajectory_on_gpu replays them): after every ending step the
    last_* fields are that step's golden state row, last_flags the golden
    flags, the totals the running sums."""
    d = load_golden(GOLDEN / f"{name}.npz")
    simple = name.startswith("simple_")
    env = make_env(product_room_set(str(d["room_source"])), 1, L=int(d["L"]), autoreset=False,
                   variant="simple" if simple else "cubic",
                   **({} if simple else {"crash_penalty": float(d["crash_penalty"])}))
    seeds = [int(s) for s in d["seeds"]]
    env.reset(seed=[seeds[0]])
    si = 1
    acts = torch.as_tensor(d["actions"], dtype=torch.int32, device="cuda:0")
    want = np.zeros(12, np.int64)
    n_term = n_trunc = 0
    for t in range(len(d["actions"])):
        env.step(acts[t:t + 1], terminal_obs=False)
        te, tr = bool(d["terminated"][t]), bool(d["truncated"][t])
        if not (te or tr):
            continue
        st = d["state"][t]           # x y z facing last_action step_count visited_count bump_count done ...
        max_steps = int(env.export_state()[0, 14])
        want[0] += 1
        want[1] += int(st[8])
        want[2:6] += (int(st[5]), int(st[7]), int(st[6]), max_steps)
        want[6:10] = (int(st[5]), int(st[7]), int(st[6]), max_steps)
        want[11] = int(te) | (int(tr) << 1)
        got = records(env)[0]
        want[10] = got[10]
        assert got.tolist() == want.tolist(), f"record after the end at step {t}"
        assert got[10] == int(env.export_state()[0, 13])
        assert totals(env).tolist() == want[:6].tolist()
        n_term += int(te)
        n_trunc += int(tr and not te)
        if si < len(seeds):
            env.reset(seed=[seeds[si]])
            si += 1
    expect = {"traj_box8x8x4_file_L4_explore": (6, 0), "traj_box8x8x4_ctor_L4_random": (0, 4),
              "traj_maze3dtunnels_L10_explore": (0, 4), "simple_box8x8x4_L4_random": (1, 5),
              "simple_kitchen2_L10_seek": (25, 0)}[name]
    assert (n_term, n_trunc) == expect
    env.close()


# ---------------------------------------------------------------- b. fused launches through auto-reset
_EXPECT = {}


def _cubic_expect(N, boxes=tuple(eh.CUBIC_BOXES), policy_seed=eh.CUBIC_POLICY_SEED):
    key = (N, boxes, policy_seed)
    if key not in _EXPECT:      # computed once, shared by the modes, never changed
        eo, snaps, first = eh.cubic_expectation(N, boxes=list(boxes), policy_seed=policy_seed)
        # the input must exercise the cases: a terminated end, a truncated end, several ends in one launch
        assert eo.n_term + eo.n_both >= 1 and eo.n_trunc + eo.n_both >= 1
        assert int((first >= 2).sum()) >= N // 2
        _EXPECT[key] = snaps
    return _EXPECT[key]


def _run_fused(env, snaps, launches, policy_seed):
    N = env.num_agents
    env.reset(seed=42)
    for K, (rec, tot) in zip(launches, snaps):
        env.step_random(K, policy_seed=policy_seed)
        got = records(env)
        bad = np.nonzero((got != rec).any(1))[0]
        assert bad.size == 0, f"after the {K}-step launch: agent {bad[0]} got {got[bad[0]].tolist()} want {rec[bad[0]].tolist()}"
        assert totals(env).tolist() == tot.tolist()
    assert env._t == sum(launches) and N == rec.shape[0]


@pytest.mark.parametrize("N", [64, 50])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_fused_launches_through_autoreset(voxnav, mode, N):
    snaps = _cubic_expect(N)
    env = make_env(eh.product_boxes(eh.CUBIC_BOXES), N, tuning=mode)
    _run_fused(env, snaps, eh.CUBIC_LAUNCHES, eh.CUBIC_POLICY_SEED)
    env.close()


def test_fused_launches_ph16(voxnav):
    """A room higher than 8: the PH-16 byte-mark kernel."""
    snaps = _cubic_expect(64, boxes=tuple(eh.PH16_BOXES), policy_seed=eh.PH16_POLICY_SEED)
    env = make_env(eh.product_boxes(eh.PH16_BOXES), 64)
    assert env.info.pad_h == 16
    _run_fused(env, snaps, eh.CUBIC_LAUNCHES, eh.PH16_POLICY_SEED)
    env.close()


# ---------------------------------------------------------------- c. simpleEnv
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_simple_fused_launches_through_autoreset(voxnav, layout):
    key = "simple"
    if key not in _EXPECT:
        eo, snaps, first = eh.simple_expectation()
        assert eo.n_term + eo.n_both >= 1 and eo.n_trunc + eo.n_both >= 1 and int((first >= 2).sum()) >= 1
        _EXPECT[key] = snaps
    env = make_env(eh.product_boxes(eh.SIMPLE_BOXES), eh.SIMPLE_N, variant="simple", tuning={"simple_layout": layout})
    want = {0: "simple_line_kernel", 1: "simple_pipe_kernel", 2: "simple_kernel"}[layout]
    assert env.kernel_label(16).startswith(want)
    _run_fused(env, _EXPECT[key], eh.SIMPLE_LAUNCHES, eh.SIMPLE_POLICY_SEED)
    env.close()


# ---------------------------------------------------------------- d. the latch
@pytest.mark.parametrize("variant", ["cubic", "simple"])
def test_no_autoreset_latch(voxnav, variant):
    N, box, ps = 32, [(4, 4, 3)], 5
    env = make_env(eh.product_boxes(box), N, autoreset=False, variant=variant)
    eo = eh.EpisodeOracle(eh.oracle_boxes(box, N, variant=int(variant == "simple")), 42 + np.arange(N), N, ps,
                          autoreset=False)
    env.reset(seed=42)
    for K in (40, 1, 1, 1, 1, 1):       # stepped on after the end: nothing more
        env.step_random(K, policy_seed=ps)
        eo.run(K)
        got = records(env)
        assert (got[:, 0] == 1).all()
        assert got.tolist() == eo.rec.tolist()
    half = np.arange(N) % 2 == 0
    env.reset(seed=1000, mask=torch.as_tensor(half))
    for i in np.nonzero(half)[0]:
        eo.reset(int(i), 1000 + int(i))
    env.step_random(40, policy_seed=ps)
    eo.run(40)
    got = records(env)
    assert got[:, 0].tolist() == np.where(half, 2, 1).tolist()
    assert got.tolist() == eo.rec.tolist()
    # a reset of agents in mid-episode abandons the episode: nothing counted
    quarter = np.arange(N) % 4 == 0
    qm = torch.as_tensor(quarter)
    env.reset(seed=2000, mask=qm)
    env.step_random(2, policy_seed=ps)          # max_steps is 4: two steps in, CubicEnv agents cannot have ended
    for i in np.nonzero(quarter)[0]:
        eo.reset(int(i), 2000 + int(i))
    eo.run(2)
    mid = [int(i) for i in np.nonzero(quarter)[0] if not eo.over[i]]
    assert mid if variant == "simple" else len(mid) == int(quarter.sum())   # (a simpleEnv goal may be 2 steps away)
    st = env.export_state().cpu().numpy()
    assert (st[mid, 5] == 2).all() and (st[mid, 8] == 0).all()
    early = np.array([bool(quarter[i]) and eo.over[i] for i in range(N)])    # (simpleEnv: ended in those 2 steps)
    env.reset(seed=3000, mask=qm)
    for i in np.nonzero(quarter)[0]:
        eo.reset(int(i), 3000 + int(i))
    assert records(env).tolist() == eo.rec.tolist()
    assert records(env)[:, 0].tolist() == (np.where(half, 2, 1) + early).tolist()     # the abandoned ones: nothing
    env.step_random(40, policy_seed=ps)
    eo.run(40)
    assert records(env).tolist() == eo.rec.tolist()
    assert records(env)[:, 0].tolist() == (np.where(half, 2, 1) + early + quarter).tolist()
    assert totals(env).tolist() == eo.totals().tolist()
    env.close()


# ---------------------------------------------------------------- e. state plumbing
def test_snapshot_clone_import_clear(voxnav):
    N, ps = 48, 9
    env = make_env(eh.product_boxes(eh.CUBIC_BOXES), N)
    env.reset(seed=42)
    env.step_random(60, policy_seed=ps)
    at_snap = records(env)
    assert at_snap[:, 0].sum() > N
    snap = env.snapshot()
    env.step_random(50, policy_seed=ps)
    later = records(env)
    assert (later[:, 0] >= at_snap[:, 0]).all() and later[:, 0].sum() > at_snap[:, 0].sum()
    env.restore(snap)
    assert records(env).tolist() == at_snap.tolist()
    other = env.clone()
    assert records(other).tolist() == at_snap.tolist()
    for K in (50, 7):
        env.step_random(K, policy_seed=ps)
        other.step_random(K, policy_seed=ps)
        assert records(other).tolist() == records(env).tolist()
    assert records(env).tolist() != at_snap.tolist()
    other.close()
    # import_state of an exported state leaves the rows untouched
    before = records(env)
    env.import_state(env.export_state(), env.belief())
    assert records(env).tolist() == before.tolist()
    # clear: exactly the masked rows
    mask = np.arange(N) % 3 == 0
    env.clear_episode_records(torch.as_tensor(mask))
    got = records(env)
    assert (got[mask] == 0).all() and got[~mask].tolist() == before[~mask].tolist()
    assert totals(env).tolist() == before[~mask][:, :6].sum(0).tolist()
    env.clear_episode_records()
    assert (records(env) == 0).all() and (totals(env) == 0).all()
    # NULL arguments are refused
    lib, h = env.lib, env._h
    buf = torch.zeros(N * 12, dtype=torch.int64, device="cuda:0")
    p = ctypes.c_void_p(buf.data_ptr())
    assert lib.vn_episode_records(None, p, None) == -1 and lib.vn_episode_records(h, None, None) == -1
    assert lib.vn_episode_totals(None, p, None) == -1 and lib.vn_episode_totals(h, None, None) == -1
    assert lib.vn_episode_clear(None, None, None) == -1
    env.close()


def test_rows_are_zero_at_create_and_simple_snapshot(voxnav):
    env = make_env(eh.product_boxes(eh.SIMPLE_BOXES), 40, variant="simple")
    assert (records(env) == 0).all() and (totals(env) == 0).all()
    env.reset(seed=42)
    env.step_random(64, policy_seed=3)
    a = records(env)
    assert a[:, 0].sum() > 0
    snap = env.snapshot()
    env.step_random(30, policy_seed=3)
    env.restore(snap)
    assert records(env).tolist() == a.tolist()
    env.close()


# ---------------------------------------------------------------- f. the reduction's edges
@pytest.mark.parametrize("N", [1, 63, 64, 65, 4099])
def test_totals_reduction_edges(voxnav, N):
    env = make_env(eh.product_boxes([(4, 4, 3)]), N)
    env.reset(seed=42)
    env.step_random(32, policy_seed=7)
    rec = env.episode_records()
    assert int(rec[:, 0].min()) >= 1
    assert env.episode_totals().tolist() == rec[:, :6].sum(0).tolist()
    env.close()
