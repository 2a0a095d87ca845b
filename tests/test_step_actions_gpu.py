"""K fused steps of caller-given actions (vn_step_actions) on the GPU.

Bar: one launch of K explicit-action steps is bit-identical to the oracle stepping the same actions
(`OracleEnv.run_random(actions=..., terminal_obs=True)`): obs bytes, f64 reward, f32 reward, flags,
terminal obs rows, and the exported state and belief it leaves.  The shapes are the smallest that
reach each way it can go wrong: K not a multiple of the 4-step reward block and a block split
across launches, every agent auto-resetting inside a launch, a one-step launch leaving window
records for the next, a partly filled wave, each CubicEnv belief mode and column height, u64 plane
words, and the three simpleEnv kernels with goal terminations inside the launch.
"""
import ctypes as C

import numpy as np
import pytest

from copy_helpers import MODES, assert_exports, assert_rows, launch_all, make_env, np_, oracle_run, seek_actions

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def voxnav():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import voxnav
    voxnav.load_library()
    return voxnav


# (id, src, L, N, tuning, launches).  box:8x8x4 has 72 free cells = max_steps: the 75-step launch auto-resets every
# agent; 1 + 5 + 17 = 23 leaves the 75-step launch starting inside a 4-step block.  The PH-16 and PH-32 rooms have
# 6 * 6 * 8 = 4 * 4 * 18 = 288 free cells: a 290-step launch is longer than max_steps.
CUBIC = [(f"8x8x4-{m}", "box:8x8x4", 4, 40, MODES[m], [1, 5, 17, 75]) for m in MODES] + [
    ("ph16", "box:8x8x10", 4, 24, None, [1, 290]), ("ph32", "box:6x6x20", 4, 24, None, [1, 290]),
    ("u64-planes", "box:100x40x8", 10, 24, None, [40])]
# N = 70: one full wave of 64 agents and 6 more
SIMPLE = [("lines", "box:8x8x4", 4, 70, {"simple_layout": 0}, [1, 45]),
          ("words", "box:8x8x4", 4, 70, {"simple_layout": 1}, [1, 45]),
          ("dense", "box:8x8x4", 4, 70, {"simple_layout": 2}, [1, 45]),
          ("40x40-words", "box:40x40x8", 4, 70, None, [1, 45])]


def actions_for(variant, src, L, seeds, K):
    rng = np.random.default_rng(1234 + K)
    if variant == "simple":
        return seek_actions(src, L, seeds, K, rng)      # every second agent walks to its goal
    return rng.integers(0, 6, size=(K, len(seeds))).astype(np.int32)


def check(variant, src, L, N, tuning, ks, fast):
    seeds = 1000 + np.arange(N, dtype=np.int64)
    acts = actions_for(variant, src, L, seeds, sum(ks))
    orc, oenv = oracle_run(variant, src, L, seeds, acts, N)
    env = make_env(variant, src, L, N, tuning)
    env.reset(seed=1000)
    got = launch_all(env, acts, ks, fast=fast)
    assert env._t == sum(ks)
    assert_rows(got, orc, "vs oracle")
    assert_exports(env, oenv, "after the launches")
    env.close()
    return orc


@pytest.mark.parametrize("name,src,L,N,tuning,ks", CUBIC, ids=[c[0] for c in CUBIC])
def test_cubic_launches_match_oracle(voxnav, name, src, L, N, tuning, ks):
    orc = check("cubic", src, L, N, tuning, ks, fast=True)
    ended = (orc["terminated"] | orc["truncated"]).astype(bool)
    if src != "box:100x40x8":
        assert ended[-ks[-1]:].any(0).all()             # every agent auto-resets inside the last launch


@pytest.mark.parametrize("name,src,L,N,tuning,ks", SIMPLE, ids=[c[0] for c in SIMPLE])
def test_simple_launches_match_oracle(voxnav, name, src, L, N, tuning, ks):
    orc = check("simple", src, L, N, tuning, ks, fast=True)
    assert orc["terminated"][1:].sum() >= 8              # goals reached inside the 45-step launch


OTHER = [CUBIC[0], CUBIC[3], CUBIC[4], SIMPLE[0], SIMPLE[1], SIMPLE[2]]


@pytest.mark.parametrize("name,src,L,N,tuning,ks", OTHER, ids=[c[0] for c in OTHER])
def test_f64_reward_only_launches_match_oracle(voxnav, name, src, L, N, tuning, ks):
    """reward_f64=True (no f32 reward) with terminal obs: the kernels' other explicit-action instantiation."""
    check("simple" if (name, src, L, N, tuning, ks) in SIMPLE else "cubic", src, L, N, tuning, ks, fast=False)


@pytest.mark.parametrize("variant,src,L,N,tuning", [("cubic", "box:8x8x4", 4, 40, MODES["2"]),
                                                    ("cubic", "box:8x8x4", 4, 40, MODES["0/df1"]),
                                                    ("simple", "box:8x8x4", 4, 70, None)],
                         ids=["cubic-2", "cubic-0df1", "simple-lines"])
def test_one_launch_equals_single_steps(voxnav, variant, src, L, N, tuning):
    """K one-step env.step calls and one step_actions(K) call: identical outputs and exports."""
    K = 90
    acts = torch.as_tensor(np.random.default_rng(9).integers(0, 6, size=(K, N)).astype(np.int32), device="cuda:0")
    a, b = make_env(variant, src, L, N, tuning), make_env(variant, src, L, N, tuning)
    a.reset(seed=77)
    b.reset(seed=77)
    ro = a.step_actions(acts, reward_f64=True, terminal_obs=True)
    singles = [b.step(acts[k], reward_f64=True, terminal_obs=True) for k in range(K)]
    assert np_(ro.obs).tobytes() == np_(torch.stack([s.obs for s in singles])).tobytes()
    np.testing.assert_array_equal(np_(ro.reward), np_(torch.stack([s.reward for s in singles])))
    te, tr = torch.stack([s.terminated for s in singles]), torch.stack([s.truncated for s in singles])
    assert torch.equal(ro.terminated.bool(), te) and torch.equal(ro.truncated.bool(), tr)
    done = np_(te | tr)
    assert done.any(0).all()
    assert np_(ro.terminal_obs)[done].tobytes() == np_(torch.stack([s.terminal_obs for s in singles]))[done].tobytes()
    np.testing.assert_array_equal(np_(a.export_state()), np_(b.export_state()))
    np.testing.assert_array_equal(np_(a.belief()), np_(b.belief()))
    a.close()
    b.close()


def test_errors(voxnav):
    from voxnav.env import _ptr
    N = 8
    env = make_env("cubic", "box:8x8x4", 4, N)
    with pytest.raises(RuntimeError):
        env.step_actions(torch.zeros((2, N), dtype=torch.int32))
    env.reset(seed=1)
    before = np_(env.export_state())
    with pytest.raises(ValueError):
        env.step_actions(torch.zeros((3, N - 1), dtype=torch.int32))
    with pytest.raises(ValueError):
        env.step_actions(torch.zeros((0, N), dtype=torch.int32))
    acts = torch.zeros((1, N), dtype=torch.int32, device="cuda:0")
    obs = torch.zeros((1, N, 80), device="cuda:0")
    null = C.c_void_p()
    for k, a, o in ((0, acts, obs), (-3, acts, obs), (1, None, obs), (1, acts, None)):
        rc = env.lib.vn_step_actions(env._h, _ptr(a), k, _ptr(o), null, null, null, null, null, env._stream())
        assert rc == -1, (k, rc)                         # VN_ERR_INVALID, nothing launched
    assert "k_steps" in env.lib.vn_last_error().decode() or "NULL" in env.lib.vn_last_error().decode()
    np.testing.assert_array_equal(np_(env.export_state()), before)
    assert env.kernel_label(k_steps=17, explicit_actions=True) == env.kernel_label(k_steps=1, explicit_actions=True)
    env.close()
