"""voxnav.branch on the GPU: fan-out of chosen agents into a wider env and the returns of action plans.

Bar: `evaluate_plans` equals the oracle -- for each root an oracle agent reset with the root's seed
replays the root's recorded actions and then takes the plan; the expected return is the float64 sum
of its rewards, left to right, up to and including the first step that ends the episode.  Bit for
bit at gamma = 1 and within rtol 1e-15 at gamma = 0.99 (the same multiplications and additions in
the same order); `ended_at` exactly.
"""
import numpy as np
import pytest

from copy_helpers import make_env, np_, oracle_run

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SRC, L, N = "box:8x8x4", 4, 24          # 72 free cells = max_steps


@pytest.fixture(scope="module")
def voxnav():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import voxnav
    voxnav.load_library()
    return voxnav


def expected(roots, seeds, hists, plans, gamma):
    """-> (returns f64 [M, B], ended_at [M, B]) from oracle agents (root m, plan b); roots of one history length
    share an oracle run."""
    M, (B, K) = len(roots), plans.shape
    ret, end = np.zeros((M, B)), np.full((M, B), -1, dtype=np.int32)
    for H in sorted({len(h) for h in hists}):
        ms = [m for m in range(M) if len(hists[m]) == H]
        acts = np.concatenate([np.repeat(np.stack([hists[m] for m in ms], 1), B, axis=1),
                               np.tile(plans.T, (1, len(ms)))]).astype(np.int32)
        orc, _ = oracle_run("cubic", SRC, L, np.repeat([seeds[m] for m in ms], B), acts, N)
        rew = orc["reward"][H:]
        ended = (orc["terminated"] | orc["truncated"]).astype(bool)[H:]
        for n, m in enumerate(ms):
            for b in range(B):
                total, disc = np.float64(0.0), 1.0
                for k in range(K):
                    total = total + disc * rew[k, n * B + b]
                    disc = disc * gamma
                    if ended[k, n * B + b]:
                        end[m, b] = k
                        break
                ret[m, b] = total
    return ret, end


def check(env, roots, seeds, hists, plans, into=None):
    from voxnav import branch
    for gamma in (1.0, 0.99):
        got_ret, got_end = branch.evaluate_plans(env, roots, plans, gamma=gamma, into=into)
        assert got_ret.dtype == torch.float64 and got_end.dtype == torch.int32
        assert tuple(got_ret.shape) == tuple(got_end.shape) == (len(roots), len(plans))
        want_ret, want_end = expected(roots, seeds, hists, plans, gamma)
        np.testing.assert_array_equal(np_(got_end), want_end)
        if gamma == 1.0:
            np.testing.assert_array_equal(np_(got_ret), want_ret)
        else:
            np.testing.assert_allclose(np_(got_ret), want_ret, rtol=1e-15, atol=0.0)
    return want_end


def test_plans_from_roots_match_oracle(voxnav):
    from voxnav import branch
    env = make_env("cubic", SRC, L, N)
    env.reset(seed=42)
    h1 = np_(env.step_random(20, policy_seed=7, record_actions=True).actions)

    # ---- case 1: all 36 two-step plans from 4 roots ----
    roots = [1, 5, 9, 20]
    pairs = np.array([(a, b) for a in range(6) for b in range(6)], dtype=np.int32)
    before = np_(env.export_state()), np_(env.belief())
    end = check(env, roots, [42 + r for r in roots], [h1[:, r] for r in roots], pairs)
    assert (end == -1).all()
    for got, want in zip((np_(env.export_state()), np_(env.belief())), before):   # the env itself is not stepped
        np.testing.assert_array_equal(got, want)

    # ---- fan_out alone, and a reused wide env ----
    wide = branch.fan_out(env, roots, 3)
    assert wide.num_agents == 12 and int(wide.last_rejected.item()) == 0
    np.testing.assert_array_equal(np_(wide.export_state()), before[0][np.repeat(roots, 3)])
    np.testing.assert_array_equal(np_(wide.belief()), before[1][np.repeat(roots, 3)])
    again = branch.fan_out(env, [2, 2, 3, 4], 3, into=wide)
    assert again is wide
    np.testing.assert_array_equal(np_(wide.export_state()), before[0][np.repeat([2, 2, 3, 4], 3)])
    with pytest.raises(ValueError):
        branch.fan_out(env, roots, 2, into=wide)

    # ---- case 2: 8 random plans of 9 steps; one root's episode ends inside the horizon ----
    # agents 12.. start a new episode here, so the two halves are 20 steps apart; 44 more steps bring the
    # first half to step 64 of 72
    late_half = np.arange(N) < 12
    env.reset(seed=300, mask=torch.as_tensor(~late_half))
    h2 = np_(env.step_random(44, policy_seed=7, record_actions=True).actions)
    steps = np_(env.export_state())[:, 5]
    late = int(np.flatnonzero(steps >= 72 - 9)[0])
    assert late_half[late] and steps[late] == 64
    roots = [late, 13, 17, 22]
    assert (steps[roots[1:]] < 72 - 9).all()
    seeds = [42 + late] + [300 + r for r in roots[1:]]
    hists = [np.concatenate([h1[:, late], h2[:, late]])] + [h2[:, r] for r in roots[1:]]
    plans = np.random.default_rng(6).integers(0, 6, size=(8, 9)).astype(np.int32)
    wide8 = branch.fan_out(env, roots, 8)
    end = check(env, roots, seeds, hists, plans, into=wide8)
    assert (end[0] == 7).all() and (end[1:] == -1).all()      # step 72 is the plan's step 7; the others run on
    for e in (env, wide, wide8):
        e.close()
