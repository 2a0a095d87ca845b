"""The frontier planner's per-action distances on the GPU (vn_plan_frontier_dists,
BatchedGridEnv.plan_frontier_dists, FrontierExplorer.act_dists).

Bar: for every agent, in every belief layout (kernel modes 0-3, column heights 8 / 16 / 32), the
six distances and the best set equal the NumPy restatement of the rule (tests/route_dists_helpers.py,
itself held to the hand-derived table in tests/test_route_dists_cpu.py) applied to the env's own
exports, and actions / dist are bit-equal to a vn_plan_frontier call on the same state -- exact
integers, no tolerance, no agent left out.  The call is read-only on the env.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import route_dists_helpers as rd
import route_helpers as rh
from helpers import product_room_set

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# tests/test_route_gpu.py's shapes and tunings (bit 63 of a row; plane-set mode 2; u64 plane rows
# and a width that is no multiple of 4; column heights 32 and 16 with rooms of different sizes in one
# padded layout; a small room) and the smallest room vn_create accepts
SHAPES = [("box:64x12x5", 1, 63), ("box:16x16x8", 2, 50), ("box:33x20x8", 2, 48), ("box:9x9x20", 1, 40),
          ("set:P2_training", 10, 48), ("box:8x8x4", 1, 40), ("box:4x4x3", 1, 40)]
DEFAULT = {}
CASES = [(s, DEFAULT) for s in SHAPES] + [
    (SHAPES[1], {"pcache_cap": 0}), (SHAPES[1], {"pcache_cap": 1}), (SHAPES[1], {"pcache_cap": 0, "defer": 0}),
    (SHAPES[5], {"pcache_cap": 0}), (SHAPES[5], {"pcache_cap": 1}),
    (SHAPES[3], {"defer": 0}), (SHAPES[4], {"defer": 0}), (SHAPES[6], {"pcache_cap": 0})]
DEV = "cuda:0"


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


def make_env(shape, tuning=None, N=None, **kw):
    from voxnav.env import BatchedGridEnv
    src, L, n = shape
    return BatchedGridEnv(num_agents=N or n, rooms=product_room_set(src), local_map_length=L, device=DEV,
                          tuning=dict(tuning) if tuning else None, **kw)


def np_(t):
    return t.cpu().numpy()


def expected(env):
    """The restatement on the env's own exports -> (dists, best, flooded)."""
    shapes = [r.shape for r in env.room_set.rooms]
    return rd.plan_dists_batch(np_(env.export_state()), np_(env.belief()), shapes)


def assert_dists_match(env, what):
    want_d, want_b, flooded = expected(env)
    got = env.plan_frontier_dists()
    np.testing.assert_array_equal(np_(got.dists), want_d, err_msg=f"{what}: dists")
    np.testing.assert_array_equal(np_(got.best), want_b, err_msg=f"{what}: best")
    act, dist = env.plan_frontier(return_dist=True)
    assert torch.equal(got.actions, act) and torch.equal(got.dist, dist), what
    return got, want_d, want_b, flooded


def kinds(dists, best, flooded):
    """Which kinds of case a set of agents holds (on the restatement's values)."""
    pc = rd.popcount(best)
    low = np.where(dists > 0, dists, 1 << 30).min(1)
    return dict(singleton=(pc == 1).any(), three=(pc >= 3).any(),
                plus2=((dists > 0) & (dists == low[:, None] + 2)).any(),
                fallback=(dists.max(1) <= -1).any(),
                blocked_beside=((dists == -2).any(1) & (dists > 0).any(1)).any(),
                no_flood=(~flooded).any(), flood=flooded.any())


# ------------------------------------------------------------------------------------ 0. the symbol
def test_library_exports_vn_plan_frontier_dists(voxnav):
    from voxnav import _native
    assert "vn_plan_frontier_dists" in _native.EXPORTED_SYMBOLS
    assert hasattr(_native.load(), "vn_plan_frontier_dists")


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
    """Beliefs built on the host and imported.  Every box shape but the 4x4x3 one (two by two free
    cells) holds every kind of case; that is asserted on the restatement's values, so the test
    cannot pass on trivial inputs."""
    shape, tuning = case
    state, belief = crafted(shape)
    env = make_env(shape, tuning)
    assert (env.info.pad_w, env.info.pad_d, env.info.pad_h) == belief.shape[1:]
    env.import_state(torch.as_tensor(state), torch.as_tensor(belief))
    _, want_d, want_b, flooded = assert_dists_match(env, case_id(case))
    if shape[0].startswith("box:") and shape[0] != "box:4x4x3":
        have = kinds(want_d, want_b, flooded)
        assert all(have.values()), have
    env.close()


# ------------------------------------------------------------------------------- 2. stepped maps
@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_stepped_maps(voxnav, case):
    """The representation stepping leaves: after a reset, a 16-step and a 200-step random-policy launch."""
    shape, tuning = case
    env = make_env(shape, tuning)
    env.reset(seed=42)
    assert_dists_match(env, "after reset")
    env.step_random(16, policy_seed=7)
    assert_dists_match(env, "after 16 steps")
    env.step_random(200, policy_seed=7)
    assert_dists_match(env, "after 216 steps")
    env.close()


# -------------------------------------------------------------------------------- 3. closed loop
def test_closed_loop(voxnav):
    """32 alternations of act_dists and a one-step launch (live window records): every step's four
    outputs are the rule's on that step's exports, and the sets met have at least three sizes."""
    from voxnav.planner import FrontierExplorer
    env = make_env(("box:16x16x8", 4, 50))
    env.reset(seed=11)
    sizes = set()
    for t in range(32):
        got, _, want_b, _ = assert_dists_match(env, f"step {t}")
        again = FrontierExplorer().act_dists(env)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
        sizes.update(int(v) for v in rd.popcount(want_b))
        env.step(got.actions)
    assert len(sizes) >= 3 and max(sizes) >= 3, sizes
    env.close()


# ------------------------------------------------------------------------------------- 4. N edges
@pytest.mark.parametrize("N", [1, 63, 64, 65])
def test_agent_counts(voxnav, N):
    env = make_env(("box:8x8x4", 2, N))
    env.reset(seed=5)
    env.step_random(24, policy_seed=3)
    assert_dists_match(env, f"N={N}")
    env.close()


# ---------------------------------------------------------------------------------- 5. read-only
def test_planning_leaves_the_env_untouched(voxnav):
    env = make_env(("box:16x16x8", 4, 50))
    env.reset(seed=3)
    env.step_random(40, policy_seed=5)
    env.step(torch.zeros(50, dtype=torch.int32))       # a one-step launch: live window records
    state, belief = env.export_state().clone(), env.belief().clone()
    twin = env.clone()                                  # never planned
    env.plan_frontier_dists()
    assert torch.equal(state, env.export_state()) and torch.equal(belief, env.belief())
    a = torch.arange(50, dtype=torch.int32) % 6
    r1, r2 = env.step(a, reward_f64=True), twin.step(a, reward_f64=True)
    assert np_(r1.obs).tobytes() == np_(r2.obs).tobytes()
    for x, y in zip(r1[1:4], r2[1:4]):
        assert torch.equal(x, y)
    twin.close()
    env.close()


# --------------------------------------------------------------------------------------- 6. mask
def test_mask_leaves_the_other_rows(voxnav):
    from voxnav.env import FrontierDists
    env = make_env(("box:16x16x8", 2, 50))
    env.reset(seed=8)
    env.step_random(30, policy_seed=2)
    want_d, want_b, _ = expected(env)
    want_a, want_dist, _ = rh.plan_batch(np_(env.export_state()), np_(env.belief()), [r.shape for r in env.room_set.rooms])
    mask = torch.arange(50) % 3 != 1
    m = np_(mask)
    out = FrontierDists(torch.full((50,), -7, dtype=torch.int32, device=DEV),
                        torch.full((50,), -9, dtype=torch.int32, device=DEV),
                        torch.full((50, 6), -11, dtype=torch.int32, device=DEV),
                        torch.full((50,), 200, dtype=torch.uint8, device=DEV))
    got = env.plan_frontier_dists(mask=mask, out=out)
    assert all(a is b for a, b in zip(got, out))
    for t, want, sentinel in ((out.actions, want_a, -7), (out.dist, want_dist, -9), (out.dists, want_d, -11),
                              (out.best, want_b, 200)):
        np.testing.assert_array_equal(np_(t)[m], want[m])
        assert (np_(t)[~m] == sentinel).all()
    # actions, dist and best may be NULL
    dists = torch.full((50, 6), -11, dtype=torch.int32, device=DEV)
    assert env.lib.vn_plan_frontier_dists(env._h, None, None, None, C.c_void_p(dists.data_ptr()), None,
                                          env._stream()) == 0
    np.testing.assert_array_equal(np_(dists), want_d)
    with pytest.raises(ValueError, match="dists"):
        env.plan_frontier_dists(out=FrontierDists(out.actions, out.dist, out.dists[:, :5], out.best))
    env.close()


# ------------------------------------------------------------------------------------- 7. errors
def test_errors(voxnav):
    from voxnav import _native
    from voxnav.env import BatchedGridEnv
    lib = _native.load()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    acts = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    dist = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    dists = torch.full((8, 6), -7, dtype=torch.int32, device=DEV)
    best = torch.full((8,), 200, dtype=torch.uint8, device=DEV)

    simple = BatchedGridEnv(num_agents=8, rooms=product_room_set("box:8x8x4"), local_map_length=4, device=DEV,
                            variant="simple")
    simple.reset(seed=1)
    with pytest.raises(_native.VoxnavError, match=r"\(-1\).*simpleEnv"):
        simple.plan_frontier_dists()
    assert lib.vn_plan_frontier_dists(simple._h, None, p(acts), p(dist), p(dists), p(best), simple._stream()) == -1
    simple.close()

    wide = BatchedGridEnv(num_agents=8, rooms=product_room_set("box:100x40x8"), local_map_length=4, device=DEV)
    wide.reset(seed=1)
    with pytest.raises(_native.VoxnavError, match=r"\(-1\).*64"):
        wide.plan_frontier_dists()
    assert lib.vn_plan_frontier_dists(wide._h, None, p(acts), p(dist), p(dists), p(best), wide._stream()) == -1
    wide.close()

    env = BatchedGridEnv(num_agents=8, rooms=product_room_set("box:8x8x4"), local_map_length=4, device=DEV)
    with pytest.raises(RuntimeError, match="reset"):
        env.plan_frontier_dists()
    env.reset(seed=1)
    assert lib.vn_plan_frontier_dists(env._h, None, p(acts), p(dist), None, p(best), env._stream()) == -1
    assert b"NULL" in lib.vn_last_error()
    assert lib.vn_plan_frontier_dists(None, None, p(acts), p(dist), p(dists), p(best), env._stream()) == -1
    assert b"NULL" in lib.vn_last_error()
    torch.cuda.synchronize()
    assert (np_(acts) == -7).all() and (np_(dist) == -7).all() and (np_(dists) == -7).all() and (np_(best) == 200).all()
    env.close()
