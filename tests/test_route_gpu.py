"""The frontier planner on the GPU (vn_plan_frontier, BatchedGridEnv.plan_frontier, voxnav.planner).

Bar: for every agent, in every belief layout (kernel modes 0-3, column heights 8 / 16 / 32), the
kernel's action and distance equal the NumPy restatement of the rule (tests/route_helpers.py, itself
held to hand-derived answers in tests/test_route_cpu.py) applied to the env's own exports -- exact
integers, no tolerance, no agent left out.  The call is read-only on the env.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import route_helpers as rh
from helpers import oracle_env, product_room_set

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# (room source, L, N): bit 63 of a row and an N that is a multiple of nothing; plane-set mode 2
# (u32 plane rows); u64 plane rows, mode 1 and a width that is no multiple of 4; column height 32;
# column height 16 and rooms of different sizes in one padded layout; a small room
SHAPES = [("box:64x12x5", 1, 63), ("box:16x16x8", 2, 50), ("box:33x20x8", 2, 48), ("box:9x9x20", 1, 40),
          ("set:P2_training", 10, 48), ("box:8x8x4", 1, 40)]
DEFAULT = {}
# the non-default tunings of tests/test_env_gpu.py (MIX_MODES) where they change the layout
CASES = [(s, DEFAULT) for s in SHAPES] + [
    (SHAPES[1], {"pcache_cap": 0}), (SHAPES[1], {"pcache_cap": 1}), (SHAPES[1], {"pcache_cap": 0, "defer": 0}),
    (SHAPES[5], {"pcache_cap": 0}), (SHAPES[5], {"pcache_cap": 1}),
    (SHAPES[3], {"defer": 0}), (SHAPES[4], {"defer": 0})]


def case_id(case):
    (src, _, _), tuning = case
    return src.split(":")[1] + "".join(f"-{k[:2]}{v}" for k, v in tuning.items())


@pytest.fixture(scope="module")
def voxnav():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import voxnav
    voxnav.load_library()
    return voxnav


def make_env(shape, tuning=None, autoreset=True, **kw):
    from voxnav.env import BatchedGridEnv
    src, L, N = shape
    return BatchedGridEnv(num_agents=N, rooms=product_room_set(src), local_map_length=L, autoreset=autoreset,
                          device="cuda:0", tuning=dict(tuning) if tuning else None, **kw)


def np_(t):
    return t.cpu().numpy()


def expected(env):
    """The restatement on the env's own exports -> (actions, dist, tie)."""
    shapes = [r.shape for r in env.room_set.rooms]
    return rh.plan_batch(np_(env.export_state()), np_(env.belief()), shapes)


def assert_plan_matches(env, what):
    want_a, want_d, _ = expected(env)
    act, dist = env.plan_frontier(return_dist=True)
    np.testing.assert_array_equal(np_(dist), want_d, err_msg=f"{what}: dist")
    np.testing.assert_array_equal(np_(act), want_a, err_msg=f"{what}: actions")
    return want_a, want_d


# ------------------------------------------------------------------------------------ 0. the symbol
def test_library_exports_vn_plan_frontier(voxnav):
    from voxnav import _native
    assert "vn_plan_frontier" in _native.EXPORTED_SYMBOLS
    assert hasattr(_native.load(), "vn_plan_frontier")


# ------------------------------------------------------------------------------- 1. crafted maps
@functools.lru_cache(maxsize=None)
def crafted(shape):
    """One set of importable agents per shape (shared between the tunings, read-only)."""
    src, L, N = shape
    walls = [r.walls for r in product_room_set(src).rooms]
    mw, md, mh = (max(w.shape[k] for w in walls) for k in range(3))
    pads = (4 * ((mw + 3) // 4), 4 * ((md + 3) // 4), 8 if mh <= 8 else 16 if mh <= 16 else 32)
    return rh.crafted_agents(walls, L, N, pads, 100 + SHAPES.index(shape))


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_crafted_maps(voxnav, case):
    """Beliefs built on the host and imported: far targets, detours, ties and fallbacks, which a
    random policy's states hardly hold."""
    shape, tuning = case
    state, belief = crafted(shape)
    env = make_env(shape, tuning)
    assert (env.info.pad_w, env.info.pad_d, env.info.pad_h) == belief.shape[1:]
    env.import_state(torch.as_tensor(state), torch.as_tensor(belief))
    want_a, want_d, tie = expected(env)
    if shape[0].startswith("box:"):      # what the case is for, asserted on the expected values
        assert (want_d == -1).any() and (want_d >= 5).any() and tie.any() and (~tie).any()
    act, dist = env.plan_frontier(return_dist=True)
    np.testing.assert_array_equal(np_(dist), want_d)
    np.testing.assert_array_equal(np_(act), want_a)
    env.close()


def test_crafted_maps_hold_every_action(voxnav):
    seen = set()
    for shape in SHAPES:
        state, belief = crafted(shape)
        shapes = [r.shape for r in product_room_set(shape[0]).rooms]
        seen.update(int(a) for a in rh.plan_batch(state, belief, shapes)[0])
    assert seen == set(range(6))


# ------------------------------------------------------------------------------- 2. stepped maps
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_stepped_maps(voxnav, case):
    """The representation stepping leaves -- plane bits only in the marking ray's plane, blind
    marks, stood rows: after a reset, a 16-step and a 200-step random-policy launch."""
    shape, tuning = case
    env = make_env(shape, tuning)
    env.reset(seed=42)
    assert_plan_matches(env, "after reset")
    env.step_random(16, policy_seed=7)
    assert_plan_matches(env, "after 16 steps")
    env.step_random(200, policy_seed=7)
    assert_plan_matches(env, "after 216 steps")
    env.close()


# -------------------------------------------------------------------------------- 3. closed loop
def test_closed_loop(voxnav):
    """64 alternations of plan and one-step launch (live window records): every step's actions are
    the restatement's on that step's exports, no agent ever bumps, and after a step planned with
    dist = d >= 2 the next dist is in 1..d-1."""
    env = make_env(("box:16x16x8", 4, 50))
    env.reset(seed=11)
    prev = None
    for t in range(64):
        want_a, want_d = assert_plan_matches(env, f"step {t}")
        steps = np_(env.export_state())[:, 5]
        if prev is not None:
            # an agent that was not auto-reset by the last step
            cont = (prev >= 2) & (steps > 0)
            assert ((want_d[cont] >= 1) & (want_d[cont] <= prev[cont] - 1)).all(), t
        prev = want_d
        env.step(torch.as_tensor(want_a))
        assert (np_(env.export_state())[:, 7] == 0).all(), t
    assert int(env.episode_totals()[3]) == 0          # sum_bumps of any episode that ended
    env.close()


# ---------------------------------------------------------------------------------- 4. read-only
def snapshot_bytes(env):
    """vn_snapshot_save into a zeroed blob (the padding between its parts is not written)."""
    from voxnav import _native
    n = C.c_int64()
    _native.check(env.lib.vn_snapshot_bytes(env._h, C.byref(n)), "vn_snapshot_bytes")
    data = torch.zeros(int(n.value), dtype=torch.uint8, device=env.device)
    _native.check(env.lib.vn_snapshot_save(env._h, C.c_void_p(data.data_ptr()), env._stream()), "vn_snapshot_save")
    return data


@pytest.mark.parametrize("tuning", [DEFAULT, {"pcache_cap": 0}], ids=["default", "pc0"])
def test_planning_leaves_the_env_untouched(voxnav, tuning):
    env = make_env(("box:16x16x8", 4, 50), tuning)
    env.reset(seed=3)
    env.step_random(40, policy_seed=5)
    env.step(torch.zeros(50, dtype=torch.int32))       # a one-step launch: live window records
    twin = env.clone()                                  # never planned
    before = snapshot_bytes(env)
    env.plan_frontier(return_dist=True)
    assert torch.equal(before, snapshot_bytes(env))
    a = torch.arange(50, dtype=torch.int32) % 6
    r1, r2 = env.step(a, reward_f64=True), twin.step(a, reward_f64=True)
    assert np_(r1.obs).tobytes() == np_(r2.obs).tobytes()
    for x, y in zip(r1[1:4], r2[1:4]):
        assert torch.equal(x, y)
    o1, o2 = env.step_random(8, policy_seed=9, t0=0), twin.step_random(8, policy_seed=9, t0=0)
    assert np_(o1.obs).tobytes() == np_(o2.obs).tobytes()
    twin.close()
    env.close()


# --------------------------------------------------------------------------------------- 5. mask
def test_mask_leaves_the_other_rows(voxnav):
    from voxnav import _native
    env = make_env(("box:16x16x8", 2, 50))
    env.reset(seed=8)
    env.step_random(30, policy_seed=2)
    want_a, want_d, _ = expected(env)
    mask = torch.arange(50) % 3 != 1
    m = np_(mask)
    out = torch.full((50,), -7, dtype=torch.int32, device="cuda:0")
    got = env.plan_frontier(mask=mask, out=out)
    assert got is out
    np.testing.assert_array_equal(np_(out)[m], want_a[m])
    assert (np_(out)[~m] == -7).all()
    # dist through the C call: its rows keep the caller's sentinel as well
    acts = torch.full((50,), -7, dtype=torch.int32, device="cuda:0")
    dist = torch.full((50,), -9, dtype=torch.int32, device="cuda:0")
    mu8 = mask.to(device="cuda:0", dtype=torch.uint8).contiguous()
    rc = env.lib.vn_plan_frontier(env._h, C.c_void_p(mu8.data_ptr()), C.c_void_p(acts.data_ptr()),
                                  C.c_void_p(dist.data_ptr()), env._stream())
    _native.check(rc, "vn_plan_frontier")
    np.testing.assert_array_equal(np_(acts)[m], want_a[m])
    np.testing.assert_array_equal(np_(dist)[m], want_d[m])
    assert (np_(acts)[~m] == -7).all() and (np_(dist)[~m] == -9).all()
    # dist = NULL is allowed
    only = env.plan_frontier()
    np.testing.assert_array_equal(np_(only), want_a)
    env.close()


# ------------------------------------------------------------------------------------- 6. errors
def test_errors(voxnav):
    from voxnav import _native
    from voxnav.env import BatchedGridEnv
    lib = _native.load()
    acts = torch.full((8,), -7, dtype=torch.int32, device="cuda:0")

    simple = BatchedGridEnv(num_agents=8, rooms=product_room_set("box:8x8x4"), local_map_length=4, device="cuda:0",
                            variant="simple")
    simple.reset(seed=1)
    with pytest.raises(_native.VoxnavError, match=r"\(-1\).*simpleEnv"):
        simple.plan_frontier()
    simple.close()

    wide = BatchedGridEnv(num_agents=8, rooms=product_room_set("box:100x40x8"), local_map_length=4, device="cuda:0")
    wide.reset(seed=1)
    with pytest.raises(_native.VoxnavError, match=r"\(-1\).*64"):
        wide.plan_frontier(out=acts)
    wide.close()

    env = BatchedGridEnv(num_agents=8, rooms=product_room_set("box:8x8x4"), local_map_length=4, device="cuda:0")
    env.reset(seed=1)
    assert lib.vn_plan_frontier(env._h, None, None, None, env._stream()) == -1
    assert b"NULL" in lib.vn_last_error()
    assert lib.vn_plan_frontier(None, None, C.c_void_p(acts.data_ptr()), None, env._stream()) == -1
    assert b"NULL" in lib.vn_last_error()
    torch.cuda.synchronize()
    assert (np_(acts) == -7).all()                      # nothing was launched
    env.close()


# --------------------------------------------------------------------------- 7. evaluate_planner
@pytest.mark.parametrize("src,L", [("box:8x8x4", 4), ("box:16x16x8", 10)], ids=["8x8x4", "16x16x8"])
def test_evaluate_planner_matches_oracle_replay(voxnav, src, L):
    """The recorded actions replayed through the CPU oracle give each episode's score, steps, bumps,
    discovered cells and finished flag; every episode finishes without a bump."""
    from voxnav.evaluate import results_table_row
    from voxnav.planner import evaluate_planner
    n, seed = 8, 100
    r = evaluate_planner(product_room_set(src), n_episodes=n, local_map_length=L, seed=seed, device="cuda:0",
                         record_actions=True)
    acts = r["actions"]
    oenv = oracle_env(src, L, n_agents=n)
    for i in range(n):
        oenv.reset(i, seed + i)
        score, steps = 0.0, 0
        for t in range(acts.shape[0]):
            _, rew, te, tr = oenv.step(i, int(acts[t, i]))
            score += rew
            steps += 1
            if te or tr:
                break
        e, st = r["episodes"][i], oenv.state(i)
        assert (e["steps"], e["bumps"], e["discovered_cells"], e["finished"]) == \
            (steps, int(st["bump_count"]), int(st["visited_count"]), bool(st["done"])), i
        assert e["score"] == score, i
        assert e["finished"] and e["bumps"] == 0, i
    assert r["finished_pct"] == 100.0 and r["avg_bumps"] == 0.0
    assert "Frontier" in results_table_row("Frontier planner", r)


def test_rollout_records_what_was_acted_on(voxnav):
    from voxnav.planner import FrontierExplorer
    env, twin = make_env(("box:8x8x4", 4, 40)), make_env(("box:8x8x4", 4, 40))
    ro = FrontierExplorer().rollout(env, 12, seed=5)
    obs = twin.reset(seed=5)
    for t in range(12):
        assert np_(ro.obs[t]).tobytes() == np_(obs).tobytes(), t
        want_a, want_d, _ = expected(twin)
        np.testing.assert_array_equal(np_(ro.actions[t]), want_a)
        np.testing.assert_array_equal(np_(ro.dist[t]), want_d)
        res = twin.step(ro.actions[t])
        assert torch.equal(res.reward, ro.reward[t]) and torch.equal(res.terminated, ro.terminated[t])
        assert torch.equal(res.truncated, ro.truncated[t])
        obs = res.obs
    assert np_(ro.last_obs).tobytes() == np_(obs).tobytes()
    twin.close()
    env.close()
