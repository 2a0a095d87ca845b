"""The float64 restatement of the reward normalisation (tests/rnorm_helpers.py) on its own: answers
worked by hand, the straightforward np.mean / np.var form of SB3's update within a derived bound,
and shard invariance.  No GPU, no library.

The hand answers use that merging (count, mean, var) with batches is pooling: after any number of
updates from the initial (1e-4, 0, 1) the statistics are those of all returns seen plus a prior of
mass c0 = 1e-4 with mean 0 and second moment 1,
    count = c0 + n,  mean = sum(x) / count,  var = (c0 + sum(x^2)) / count - mean^2,
evaluated here in exact rational arithmetic.
"""
from fractions import Fraction as Fr

import numpy as np

import rnorm_helpers as rn

C0 = Fr(1e-4)          # the f64 nearest 1e-4, exactly
EPS = Fr(1e-8)
REL = 1e-12            # the hand answers are well conditioned: a few dozen f64 roundings, ~1e-15


def pooled(xs):
    count = C0 + len(xs)
    mean = sum(xs, Fr(0)) / count
    var = (C0 + sum((x * x for x in xs), Fr(0))) / count - mean * mean
    return mean, var, count


def close(got, want, rel=REL):
    return abs(float(got) - float(want)) <= rel * abs(float(want))


def test_merge_by_hand():
    # {1, 3} with {5}: n 3, mean 3, M2 = 2 + 0 + (4^2 * 2 * 1) / 3 ... = 8 = sum (x - 3)^2
    n, mean, m2 = rn.merge((2.0, 2.0, 2.0), (1.0, 5.0, 0.0))
    assert (n, mean) == (3.0, 3.0) and close(m2, 8.0)
    # a full chunk of 0 .. 63: sum 2016, mean 31.5, M2 = 64 (64^2 - 1) / 12 = 21840, all exact in f64
    t = rn.chunk_triples(np.arange(64.0))
    assert t.tolist() == [[64.0, 31.5, 21840.0]]
    # a short chunk: absent lanes add nothing (neither to the sum nor (0 - mean)^2 to M2)
    assert rn.chunk_triples(np.array([1.0, 2.0, 6.0])).tolist() == [[3.0, 3.0, 14.0]]
    # three chunks: the third passes the first level through; root = all 130 values
    x = np.arange(130.0)
    n, mean, m2 = rn.tree(rn.chunk_triples(x))
    assert (n, mean) == (130.0, 64.5) and close(m2, ((x - 64.5) ** 2).sum())


def test_one_agent_three_steps():
    """Rewards 1, 1, 1 with gamma 0.5: returns 1, 1.5, 1.75.  After step 0 the variance is ~2e-4
    (one sample on a prior of mass 1e-4), the scale ~0.014 and the reward 1 / 0.014 clips at 10."""
    st = rn.new_state(1)
    rew = np.ones((3, 1), np.float32)
    dones = np.zeros((3, 1), np.float32)
    scales = rn.run(st, rew, dones, 0, 3, 0.5)
    xs = [Fr(1), Fr(3, 2), Fr(7, 4)]
    assert st["ret"].tolist() == [1.75]
    mean, var, count = pooled(xs)
    assert close(st["rms"][0], mean) and close(st["rms"][1], var) and close(st["rms"][2], count)
    want = []
    for t in range(3):
        var_t = pooled(xs[:t + 1])[1]
        assert close(scales[t] ** 2, var_t + EPS)
        want.append(min(10.0, 1.0 / float(var_t + EPS) ** 0.5))
    assert want[0] == 10.0 and want[1] < 10.0
    assert rew[0, 0] == np.float32(10.0)
    np.testing.assert_allclose(rew[1:, 0], want[1:], rtol=2.0 ** -23)        # one f32 rounding


def test_two_agents_with_an_episode_end():
    """Agent 0's episode ends at step 0: its return restarts from 0 at step 1, agent 1's carries."""
    st = rn.new_state(2)
    rew = np.array([[1.0, 0.5], [2.0, -1.0], [3.0, 4.0]], np.float32)
    dones = np.array([[1, 0], [0, 0], [0, 0]], np.float32)
    rn.run(st, rew, dones, 0, 3, 0.5)
    xs = [Fr(1), Fr(1, 2), Fr(2), Fr(-3, 4), Fr(4), Fr(29, 8)]       # step 2: 0.5 * 2 + 3, 0.5 * -0.75 + 4
    assert st["ret"].tolist() == [4.0, 3.625]
    mean, var, count = pooled(xs)
    assert close(st["rms"][0], mean) and close(st["rms"][1], var) and close(st["rms"][2], count)
    # step 1's rewards over step 1's scale (the var that already includes step 1)
    sc1 = float(pooled(xs[:4])[1] + EPS) ** 0.5
    np.testing.assert_allclose(rew[1], [2.0 / sc1, -1.0 / sc1], rtol=2.0 ** -23)


def test_clip_from_both_sides():
    """A settled variance of 1 (count 1e6, so one step of +-100 moves it by ~1 %): +-100 / ~1 clips
    to +-clip exactly; 1.5 is inside and only scaled."""
    for clip in (10.0, 2.5):
        st = rn.new_state(3, mean=0.0, var=1.0, count=1e6)
        rew = np.array([[100.0, -100.0, 1.5]], np.float32)
        sc = rn.run(st, rew, np.zeros((1, 3), np.float32), 0, 1, 0.99, clip=clip)
        assert rew[0, 0] == np.float32(clip) and rew[0, 1] == np.float32(-clip)
        assert 1.0 < sc[0] < 1.01 and rew[0, 2] == np.float32(1.5 / sc[0])


def test_not_training_leaves_the_state_bit_unchanged():
    st = rn.new_state(5, mean=0.25, var=4.0, count=37.0)
    st["ret"][:] = [1.0, -2.0, 3.5, 0.0, 7.0]
    before = {k: v.tobytes() for k, v in st.items()}
    rew = np.array([[1.0, -3.0, 50.0, 0.0, 2.0], [2.0, 2.0, 2.0, 2.0, -50.0]], np.float32)
    sc = rn.run(st, rew, np.ones((2, 5), np.float32), 0, 2, 0.9, training=False)
    assert {k: v.tobytes() for k, v in st.items()} == before
    s = np.sqrt(np.float64(4.0) + np.float64(1e-8))
    assert sc.tolist() == [s, s]
    assert rew.tolist() == np.array([[0.5, -1.5, 10.0, 0.0, 1.0], [1.0, 1.0, 1.0, 1.0, -10.0]], np.float32).tolist()


_random_case = rn.random_case


def test_against_the_straightforward_sb3_update():
    """np.mean / np.var and update_from_moments as SB3 writes them, on the same returns: mean and var
    within the operation-count bound of rnorm_helpers (derived there, from the data's condition
    numbers, not from this difference)."""
    for seed, T, N in ((1, 12, 193), (2, 40, 64), (3, 5, 1000), (4, 25, 7)):
        rew, dones = _random_case(seed, T, N)
        st = rn.new_state(N)
        rms0 = st["rms"].copy()
        steps = []
        work = rew.copy()
        for t in range(T):
            rn.run(st, work, dones, t, t + 1, 0.99)
            steps.append(st["rms"].copy())
        ref, rets = rn.sb3_run(rms0.copy(), rew.astype(np.float64), dones, np.float64(0.99))
        bm, bv = rn.sb3_rel_bound(rms0, rets, np.array(steps))
        rel_m = abs(st["rms"][0] - ref[0]) / abs(ref[0])
        rel_v = abs(st["rms"][1] - ref[1]) / abs(ref[1])
        print(f"T={T} N={N}: rel(mean) {rel_m:.3g} (bound {bm:.3g}), rel(var) {rel_v:.3g} (bound {bv:.3g})")
        assert st["rms"][2] == ref[2]                   # counts are small integers plus 1e-4
        assert rel_m <= bm and rel_v <= bv
        assert bm < 1e-9 and bv < 1e-9                  # the bound itself says something


def test_shard_invariance():
    """Chunk triples computed per shard (each with its own agent_id_base) and concatenated give the
    state and the rewards of the unsharded run, bit for bit."""
    for shards in ((128, 65), (64, 64, 2)):
        N, T = sum(shards), 9
        rew, dones = _random_case(10 + N, T, N, p_done=0.2)
        one, many = rn.new_state(N), rn.new_state(N)
        r1, r2 = rew.copy(), rew.copy()
        s1 = rn.run(one, r1, dones, 0, T, 0.99)
        s2 = rn.run(many, r2, dones, 0, T, 0.99, shards=shards)
        assert one["rms"].tobytes() == many["rms"].tobytes() and one["ret"].tobytes() == many["ret"].tobytes()
        assert s1.tobytes() == s2.tobytes() and r1.tobytes() == r2.tobytes()
        assert not np.array_equal(r1, rew)


def test_segments_compose():
    rew, dones = _random_case(77, 7, 130)
    a, b = rn.new_state(130), rn.new_state(130)
    ra, rb = rew.copy(), rew.copy()
    rn.run(a, ra, dones, 0, 7, 0.99)
    rn.run(b, rb, dones, 0, 3, 0.99)
    rn.run(b, rb, dones, 3, 7, 0.99)
    assert ra.tobytes() == rb.tobytes() and a["rms"].tobytes() == b["rms"].tobytes()
