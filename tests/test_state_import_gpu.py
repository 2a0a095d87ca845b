"""Env state import (vn_import_state) and whole-env snapshots (vn_snapshot_*) on the GPU.

Bar: an imported agent is indistinguishable from one that reached the state by stepping -- obs
bytes, exact f64 rewards, flags, exported state and belief, and the auto-reset seed schedule
continue bit for bit, in whatever belief layout the destination env has; a restored or cloned env
repeats the original's steps exactly.  Modes are tuning (pcache_cap, defer) as in MIX_MODES of
tests/test_env_gpu.py; the plane-set modes apply to 8-high rooms of at most 64 x 64.
"""
import functools

import numpy as np
import pytest

from helpers import oracle_env, product_room_set

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MODES = {"0/df1": dict(pcache_cap=0, defer=-1), "0/df0": dict(pcache_cap=0, defer=0),
         "1": dict(pcache_cap=1, defer=-1), "2": dict(pcache_cap=2, defer=-1)}


@pytest.fixture(scope="module")
def voxnav():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import voxnav
    voxnav.load_library()
    return voxnav


def make_env(src, L, n, mode=None, autoreset=True, **kw):
    from voxnav.env import BatchedGridEnv
    if mode is not None:
        kw["tuning"] = MODES[mode]
    return BatchedGridEnv(num_agents=n, rooms=product_room_set(src), local_map_length=L, autoreset=autoreset,
                          device="cuda:0", **kw)


def np_(t):
    return t.cpu().numpy()


def launches(env, ks, policy_seed, t0):
    """Random-policy launches of ks steps from t0: (obs, f64 reward, terminated, truncated), concatenated."""
    out = [[], [], [], []]
    for k in ks:
        ro = env.step_random(k, policy_seed=policy_seed, t0=t0, reward_f64=True)
        for o, v in zip(out, (ro.obs, ro.reward, ro.terminated, ro.truncated)):
            o.append(np_(v))
        t0 += k
    return tuple(np.concatenate(o) for o in out)


def assert_same_rollout(a, b, what):
    assert a[0].tobytes() == b[0].tobytes(), f"{what}: obs bytes"
    np.testing.assert_array_equal(a[1], b[1], err_msg=f"{what}: f64 reward")
    np.testing.assert_array_equal(a[2], b[2], err_msg=f"{what}: terminated")
    np.testing.assert_array_equal(a[3], b[3], err_msg=f"{what}: truncated")


def room_beliefs(env):
    """Each agent's exported belief cut to its room."""
    st, b = np_(env.export_state()), np_(env.belief()).astype(np.int64)
    out = []
    for a in range(len(st)):
        W, D, H = env.room_set.rooms[int(st[a, 13])].shape
        out.append(b[a, :W, :D, :H])
    return out


def get_obs_of(state, step_obs):
    """get_obs() of the exported agents, from the obs rows the step returned for them.  step() takes its
    observation before it updates last_action, last_bump and was_near_wall (envs/CubicEnv.py:120-124, :169-224),
    so the step's row shows the values of before the step in obs[68..70] and no export holds those; get_obs() on
    the state the step left (what an import returns) shows the exported ones: f32(last_action / 5), was_near_wall,
    last_bump (:284-286).  The other 77 floats -- the window, facing, cells_insight_down, the explored share,
    the padding -- are the step's own, byte for byte.  (For an agent the step auto-reset, and after a reset,
    the three already agree.)"""
    want = step_obs.copy()
    want[:, 68] = (state[:, 4].astype(np.float64) / 5.0).astype(np.float32)
    want[:, 69] = state[:, 11].astype(np.float32)
    want[:, 70] = state[:, 9].astype(np.float32)
    return want


# ------------------------------------------------------- 1. round trip and continuation, across layouts
CASES = [("box:8x8x4", 4, 40, 85, 75), ("box:16x16x8", 7, 50, 37, 40), ("box:32x32x8", 10, 96, 37, 40),
         ("set:P3_training", 10, 64, 300, 100), ("box:100x40x8", 10, 48, 37, 40)]
SMALL_PAIRS = [(m, m) for m in MODES] + [("2", "0/df0"), ("0/df1", "2"), ("1", "2"), ("2", "1")]
LARGE_PAIRS = [("0/df1", "0/df1"), ("0/df0", "0/df0"), ("0/df1", "0/df0"), ("0/df0", "0/df1")]
ROUND_TRIPS = [(c, p) for c in CASES for p in (LARGE_PAIRS if c[0].startswith(("set:", "box:100")) else SMALL_PAIRS)]


@functools.lru_cache(maxsize=None)
def oracle_run(case):
    """One oracle run of k1 + k2 steps (shared, read-only): rows, final beliefs (min(., 63)), episode ends."""
    src, L, N, k1, k2 = case
    env = oracle_env(src, L, n_agents=N)
    orc = env.run_random(42 + np.arange(N, dtype=np.int64), policy_seed=7, K=k1 + k2, seed_stride=N)
    ended = orc["terminated"].astype(bool) | orc["truncated"].astype(bool)
    return dict(rows=(orc["obs"], orc["reward"], orc["terminated"], orc["truncated"]), ended=ended,
                beliefs=[np.minimum(env.belief(a), 63) for a in range(N)],
                max_count=max(int(env.belief(a).max()) for a in range(N)))


@functools.lru_cache(maxsize=None)
def source_run(case, mode):
    """Env A of a case in one mode (shared, read-only): its exports after launches of k1 - 1 and 1 steps -- the
    one-step launch leaves live window records -- and its continuation through launches of 1, 5 and k2 - 6."""
    src, L, N, k1, k2 = case
    env = make_env(src, L, N, mode)
    env.reset(seed=42)
    before = launches(env, [k1 - 1, 1], 7, 0)
    state, belief = env.export_state(), env.belief()
    cont = launches(env, [1, 5, k2 - 6], 7, k1)
    out = dict(state=np_(state), belief=np_(belief), obs=before[0][k1 - 1], before=before, cont=cont,
               final_state=np_(env.export_state()), final_beliefs=room_beliefs(env))
    env.close()
    return out


@pytest.mark.parametrize("case,pair", ROUND_TRIPS,
                         ids=[f"{c[0]}-{p[0]}->{p[1]}".replace("/", "") for c, p in ROUND_TRIPS])
def test_import_round_trip_and_continuation(voxnav, case, pair):
    src, L, N, k1, k2 = case
    orc = oracle_run(case)
    # what the case is for, asserted from the oracle's own output
    if src == "box:8x8x4":      # 72 interior cells: every agent auto-resets before the import and again after it
        assert orc["ended"][:k1].any(0).all() and orc["ended"][k1:].any(0).all()
    if src == "set:P3_training":
        # an auto-reset before the import, and a visit count past the device's 63 (reached in the continuation:
        # the largest count at step 300 is 57; a count above 63 in the imported map itself is
        # test_imported_count_above_63_is_clamped)
        assert orc["ended"][:k1].any() and orc["max_count"] > 63
    a = source_run(case, pair[0])
    assert_same_rollout(a["before"], tuple(r[:k1] for r in orc["rows"]), "A before the export vs oracle")

    b = make_env(src, L, N, pair[1])
    b.reset(seed=1000)          # a used env: live window records, stood rows and planes of its own
    launches(b, [4, 1], 11, 0)
    obs = b.import_state(torch.as_tensor(a["state"]), torch.as_tensor(a["belief"]))
    np.testing.assert_array_equal(np_(b.export_state()), a["state"])       # all 16 fields
    np.testing.assert_array_equal(np_(b.belief()), a["belief"])
    assert np_(obs).tobytes() == get_obs_of(a["state"], a["obs"]).tobytes()

    cont = launches(b, [1, 5, k2 - 6], 7, k1)
    assert_same_rollout(cont, a["cont"], "B vs A")
    assert_same_rollout(cont, tuple(r[k1:] for r in orc["rows"]), "B vs oracle")
    assert_same_rollout(a["cont"], tuple(r[k1:] for r in orc["rows"]), "A vs oracle")
    for i, (got_b, got_a, want) in enumerate(zip(room_beliefs(b), a["final_beliefs"], orc["beliefs"])):
        np.testing.assert_array_equal(got_b, want, err_msg=f"B agent {i}")
        np.testing.assert_array_equal(got_a, want, err_msg=f"A agent {i}")
    np.testing.assert_array_equal(np_(b.export_state())[:, :14], a["final_state"][:, :14])
    b.close()


def test_imported_count_above_63_is_clamped(voxnav):
    """A map whose own-cell count is 100: it reads back as 63, as the device map saturates."""
    src, L, N = "box:8x8x4", 4, 16
    a = make_env(src, L, N, "2")
    a.reset(seed=42)
    st, bl = a.export_state(), a.belief()
    idx = torch.arange(N, device=bl.device)
    bl[idx, st[:, 0], st[:, 1], st[:, 2]] = 100
    for mode in MODES:
        b = make_env(src, L, N, mode)
        b.import_state(st, bl)
        got = b.belief()
        assert (got[idx, st[:, 0], st[:, 1], st[:, 2]] == 63).all(), mode
        bl63 = bl.clone()
        bl63[idx, st[:, 0], st[:, 1], st[:, 2]] = 63
        assert torch.equal(got, bl63), mode
        b.close()
    a.close()


# --------------------------------------------------------------------------------------------- 2. mask
@pytest.mark.parametrize("mode", list(MODES), ids=[m.replace("/", "") for m in MODES])
def test_masked_import_leaves_the_others_untouched(voxnav, mode):
    case = ("box:16x16x8", 7, 50, 37, 40)
    src, L, N, k1, _ = case
    a = source_run(case, "2")
    b = make_env(src, L, N, mode)
    b.reset(seed=42)
    st0, bl0 = np_(b.export_state()), np_(b.belief())
    mask = torch.arange(N) % 2 == 0
    even, odd = np_(mask), ~np_(mask)
    out = torch.full((N, 80), -7.0, dtype=torch.float32, device="cuda:0")
    got = b.import_state(torch.as_tensor(a["state"]), torch.as_tensor(a["belief"]), mask=mask, out=out)
    assert got is out
    st, bl, obs = np_(b.export_state()), np_(b.belief()), np_(out)
    np.testing.assert_array_equal(st[even], a["state"][even])
    np.testing.assert_array_equal(bl[even], a["belief"][even])
    assert obs[even].tobytes() == get_obs_of(a["state"], a["obs"])[even].tobytes()
    np.testing.assert_array_equal(st[odd], st0[odd])
    np.testing.assert_array_equal(bl[odd], bl0[odd])
    assert (obs[odd] == -7.0).all()
    cont = launches(b, [1, 5, 14], 7, k1)           # the even agents then continue like A (global step k1 onwards)
    for got_rows, want_rows in zip(cont, a["cont"]):
        np.testing.assert_array_equal(got_rows[:, even], want_rows[:20][:, even])
    b.close()


def test_partial_import_needs_a_reset_env(voxnav):
    case = ("box:16x16x8", 7, 50, 37, 40)
    a = source_run(case, "2")
    b = make_env(case[0], case[1], case[2])
    with pytest.raises(ValueError, match="partial import"):
        b.import_state(torch.as_tensor(a["state"]), torch.as_tensor(a["belief"]), mask=torch.arange(50) % 2 == 0)
    b.import_state(torch.as_tensor(a["state"]), torch.as_tensor(a["belief"]))      # a full one marks it reset
    b.step_random(1, policy_seed=7, t0=37)
    b.close()


# ------------------------------------------------------------------------------- 3. sensing on import
@pytest.mark.parametrize("mode", ["2", "0/df0"], ids=["2", "0df0"])
@pytest.mark.parametrize("src,L,N", [("box:8x8x4", 4, 40), ("box:32x32x8", 10, 96)], ids=["box8", "box32"])
def test_import_senses_like_the_first_observation(voxnav, src, L, N, mode):
    a = make_env(src, L, N, mode)
    obs = a.reset(seed=42)
    st, bl = a.export_state(), a.belief()
    blank = torch.where(bl == -128, bl, torch.full_like(bl, -1))           # everything unknown ...
    idx = torch.arange(N, device=bl.device)
    blank[idx, st[:, 0], st[:, 1], st[:, 2]] = bl[idx, st[:, 0], st[:, 1], st[:, 2]]   # ... but the agent's own cell
    bare = st.clone()
    bare[:, 10] = 0             # near_wall
    bare[:, 12] = 0             # cells_insight_down
    b = make_env(src, L, N, mode)
    got = b.import_state(bare, blank)
    assert np_(got).tobytes() == np_(obs).tobytes()
    np.testing.assert_array_equal(np_(b.export_state()), np_(st))
    np.testing.assert_array_equal(np_(b.belief()), np_(bl))
    a.close()
    b.close()


# --------------------------------------------------------------------------------------- 4. validation
def raw_parts(env, snap):
    """Per-agent rows of a CubicEnv snapshot's first parts (include/voxnav.h: each part starts on a 256-byte
    boundary): hot words, window records (16 columns of pad_h bytes), next seeds, belief blocks."""
    N, ph, ab = env.num_agents, env.info.pad_h, env.info.belief_bytes_per_agent
    blob, out, off = np_(snap.data), {}, 0
    for name, per_agent in (("hot+wrec", None), ("seed", 4), ("belief", ab)):
        n = N * (16 + 16 * ph) if per_agent is None else N * per_agent
        part = blob[off:off + n]
        if per_agent is None:
            out["hot"], out["wrec"] = part[:16 * N].reshape(N, 16), part[16 * N:].reshape(N, 16 * ph)
        else:
            out[name] = part.reshape(N, per_agent)
        off += (n + 255) & ~255
    return out


def test_rejected_agents_are_counted_and_left_untouched(voxnav):
    from voxnav._native import VoxnavError
    src, L, N = "set:P3_training", 10, 16
    a = make_env(src, L, N)
    a.reset(seed=42)
    a.step_random(20, policy_seed=7, t0=0)
    st, bl = np_(a.export_state()), np_(a.belief())
    rooms = a.room_set.rooms

    def cell(agent, wall):      # a cell of the agent's room that is (not) a wall and not the agent's own
        w = rooms[int(st[agent, 13])].walls_for(0) != 0
        for x, y, z in np.argwhere(w == wall):
            if (x, y, z) != tuple(st[agent, :3]):
                return int(x), int(y), int(z)
        raise AssertionError("no such cell")

    bad_st, bad_bl = st.copy(), bl.copy()
    bad_st[1, :3] = cell(1, True)                       # position on a wall cell
    x, y, z = cell(4, True)
    bad_bl[4, x, y, z] = 0                              # belief 0 at a wall cell
    x, y, z = cell(7, False)
    bad_bl[7, x, y, z] = -2                             # belief -2 at a free cell
    bad_st[10, 3] = 4                                   # facing 4
    bad_bl[13, st[13, 0], st[13, 1], st[13, 2]] = -1    # own cell -1
    bad = [1, 4, 7, 10, 13]
    good = [i for i in range(N) if i not in bad]

    b = make_env(src, L, N)
    b.reset(seed=1000)
    b.step_random(3, policy_seed=11, t0=0)
    st0, bl0 = np_(b.export_state()), np_(b.belief())
    snap0 = b.snapshot()
    out = torch.full((N, 80), -7.0, dtype=torch.float32, device="cuda:0")
    b.import_state(torch.as_tensor(bad_st), torch.as_tensor(bad_bl), out=out, check=False)
    assert int(b.last_rejected.item()) == 5
    st1, bl1, obs1 = np_(b.export_state()), np_(b.belief()), np_(out)
    np.testing.assert_array_equal(st1[bad], st0[bad])
    np.testing.assert_array_equal(bl1[bad], bl0[bad])
    assert (obs1[bad] == -7.0).all()
    np.testing.assert_array_equal(st1[good], st[good])
    np.testing.assert_array_equal(bl1[good], bl[good])
    assert (obs1[good] != -7.0).any(1).all()
    # bit-identical: the rejected agents' share of every raw per-agent buffer
    raw0, raw1 = raw_parts(b, snap0), raw_parts(b, b.snapshot())
    for name in raw0:
        np.testing.assert_array_equal(raw1[name][bad], raw0[name][bad], err_msg=name)
    assert (raw1["hot"][good] != raw0["hot"][good]).any(1).all()
    with pytest.raises(VoxnavError, match="rejected 5 of 16"):
        b.import_state(torch.as_tensor(bad_st), torch.as_tensor(bad_bl))
    a.close()
    b.close()


# -------------------------------------------------------------------------------------- 5. resharding
def test_import_reshards_agents(voxnav):
    case = ("box:8x8x4", 4, 40, 85, 75)
    src, L, N, k1, k2 = case
    a = source_run(case, "2")
    halves = []
    for base in (0, 20):
        b = make_env(src, L, 20, agent_id_base=base, seed_stride=40)
        b.import_state(torch.as_tensor(a["state"][base:base + 20]), torch.as_tensor(a["belief"][base:base + 20]))
        halves.append(launches(b, [1, 5, k2 - 6], 7, k1))
        b.close()
    union = tuple(np.concatenate([h[j] for h in halves], axis=1) for j in range(4))
    assert_same_rollout(union, a["cont"], "B1 + B2 vs A")
    assert (a["cont"][2] | a["cont"][3]).any(0).all()                      # every agent auto-resets in these steps


# ---------------------------------------------------------------------------------------- 6. snapshots
SNAP_ENVS = [("cubic", "box:16x16x8", 7, MODES["0/df1"]), ("cubic", "box:16x16x8", 7, MODES["0/df0"]),
             ("cubic", "box:16x16x8", 7, MODES["1"]), ("cubic", "box:16x16x8", 7, MODES["2"]),
             ("simple", "box:8x8x4", 4, {"simple_layout": 0}), ("simple", "box:8x8x4", 4, {"simple_layout": 1}),
             ("simple", "box:8x8x4", 4, {"simple_layout": 2}), ("simple", "box:40x40x8", 4, None)]


def snap_env(variant, src, L, tuning, n=48):
    from voxnav.env import BatchedGridEnv
    return BatchedGridEnv(num_agents=n, rooms=product_room_set(src), local_map_length=L, autoreset=True,
                          device="cuda:0", variant=variant, tuning=tuning)


def exports(env):
    return np_(env.export_state()), np_(env.belief())


SNAP_IDS = ["cubic-0df1", "cubic-0df0", "cubic-1", "cubic-2", "simple-lines", "simple-words", "simple-dense",
            "simple-40x40-words"]


@pytest.mark.parametrize("variant,src,L,tuning", SNAP_ENVS, ids=SNAP_IDS)
def test_snapshot_restore_and_clone(voxnav, variant, src, L, tuning):
    N = 48
    env = snap_env(variant, src, L, tuning)
    env.reset(seed=42)
    head = launches(env, [29, 1], 7, 0)                 # 30 steps; the one-step launch leaves window records
    snap = env.snapshot()
    assert snap.t == 30 and snap.data.dtype == torch.uint8 and snap.data.device.type == "cuda"
    first = launches(env, [1, 39], 7, 30)
    ex_first = exports(env)
    orc_env = oracle_env(src, L, n_agents=N, variant=1 if variant == "simple" else 0)
    seeds = 42 + np.arange(N, dtype=np.int64)
    orc = orc_env.run_random(seeds, policy_seed=7, K=70, seed_stride=N)
    rows = (orc["obs"], orc["reward"], orc["terminated"], orc["truncated"])
    assert_same_rollout(tuple(np.concatenate([h, f]) for h, f in zip(head, first)), rows, "vs oracle")
    for a in range(N):
        W, D, H = orc_env.rooms[int(ex_first[0][a, 13])].whd
        np.testing.assert_array_equal(ex_first[1][a, :W, :D, :H], np.minimum(orc_env.belief(a), 63),
                                      err_msg=f"agent {a}")
    # the clone continues like the oracle while the original is stepped differently in between ...
    twin = env.clone()
    assert twin._t == env._t == 70
    env.step_random(7, policy_seed=99, t0=500)
    more = orc_env.run_random(seeds, policy_seed=7, K=13, t0=70, seed_stride=N, initial_reset=False)
    assert_same_rollout(launches(twin, [1, 12], 7, 70),
                        (more["obs"], more["reward"], more["terminated"], more["truncated"]), "clone vs oracle")
    # ... and the original, restored, repeats its 40 steps: outputs and exports
    env.restore(snap)
    assert env._t == 30
    assert_same_rollout(launches(env, [1, 39], 7, 30), first, "after restore")
    for got, want in zip(exports(env), ex_first):
        np.testing.assert_array_equal(got, want)
    env.close()
    twin.close()


def test_snapshot_of_another_env_is_refused(voxnav):
    from voxnav._native import VoxnavError
    src, L = "box:16x16x8", 7
    a = snap_env("cubic", src, L, {"pcache_cap": 2})
    a.reset(seed=42)
    a.step_random(10, policy_seed=7, t0=0)
    snap = a.snapshot()
    for other in (snap_env("cubic", src, L, {"pcache_cap": 1}), snap_env("cubic", src, L, {"pcache_cap": 2}, n=32)):
        other.reset(seed=5)
        other.step_random(3, policy_seed=7, t0=0)
        before = exports(other)
        with pytest.raises(VoxnavError, match=r"vn_snapshot_load failed \(-1\)"):
            other.restore(snap)
        for got, want in zip(exports(other), before):
            np.testing.assert_array_equal(got, want)
        assert other._t == 3
        other.close()
    a.close()


def test_import_into_simple_env_is_refused(voxnav):
    from voxnav._native import VoxnavError
    env = snap_env("simple", "box:8x8x4", 4, None)
    env.reset(seed=42)
    st, bl = env.export_state(), env.belief()
    with pytest.raises(VoxnavError, match=r"vn_import_state failed \(-1\).*simpleEnv"):
        env.import_state(st, bl)
    env.close()
