"""Per-agent copies between envs (vn_copy_agents) on the GPU.

Bar: a copied agent is indistinguishable from its source.  Its exports equal the source's, and
under explicit actions (vn_step_actions) it continues bit for bit like an oracle agent that was
reset with the source's seed, replayed the source's recorded actions and then took the new ones --
obs bytes, f64 and f32 rewards, flags, terminal obs rows, final state and belief, through
auto-resets on the copied seed schedule.  Agents that are not copied, and destinations the device
validation rejects, keep every byte of their state.  Layouts: the snapshot tests' list
(test_state_import_gpu.SNAP_ENVS), 40 steps after the copy, plus two CubicEnv modes in a room small
enough that every agent auto-resets after the copy (box:8x8x4: max_steps 72, 30 of them taken
before the copy, 45 after it).
"""
import numpy as np
import pytest

from copy_helpers import MODES, assert_exports, assert_rows, launch_all, make_env, np_, oracle_run
from test_state_import_gpu import SNAP_ENVS, SNAP_IDS

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NA, NB, HIST, FRESH = 48, 20, 30, 40
COPY_ENVS = [e + (FRESH,) for e in SNAP_ENVS] + [("cubic", "box:8x8x4", 4, MODES["2"], 45),
                                                 ("cubic", "box:8x8x4", 4, MODES["0/df1"], 45)]
COPY_IDS = SNAP_IDS + ["cubic-8x8x4-2", "cubic-8x8x4-0df1"]
# -1 (kept), repeated sources, every third agent of A, its first and last agent
INDEX = np.array([-1, 3, 3, 6, -1, 9, 12, 12, -1, 15, 45, 0, -1, 21, 24, 3, -1, 27, 30, 47], dtype=np.int32)


@pytest.fixture(scope="module")
def voxnav():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import voxnav
    voxnav.load_library()
    return voxnav


def stepped(variant, src, L, tuning, n, seed, policy_seed, **kw):
    """An env after 29 + 1 recorded random steps (the one-step launch leaves window records) -> (env, actions)."""
    env = make_env(variant, src, L, n, tuning, **kw)
    env.reset(seed=seed)
    acts = [np_(env.step_random(k, policy_seed=policy_seed, record_actions=True).actions) for k in (HIST - 1, 1)]
    return env, np.concatenate(acts)


def exports(env):
    return np_(env.export_state()), np_(env.belief())


def fresh_actions(n, steps, seed=77):
    return np.random.default_rng(seed).integers(0, 6, size=(steps, n)).astype(np.int32)


def expect_after_copy(variant, src, L, index, seeds_src, hist_src, seeds_own, hist_own, acts):
    """The oracle agents of a destination env: agent i reset with its source's seed (or its own), its source's
    (own) recorded actions replayed, then `acts`; seed stride NA.  -> (rows of the last FRESH steps, oracle env)"""
    copied = index >= 0
    seeds = np.where(copied, seeds_src[np.maximum(index, 0)], seeds_own)
    hist = np.where(copied[None, :], hist_src[:, np.maximum(index, 0)], hist_own)
    orc, oenv = oracle_run(variant, src, L, seeds, np.concatenate([hist, acts]), NA)
    return {k: (v[HIST:] if isinstance(v, np.ndarray) else v) for k, v in orc.items()}, oenv


def test_cases_reach_what_they_are_for():
    """(CPU) the chosen steps take the extra box:8x8x4 cases through an auto-reset of every agent."""
    assert HIST + 45 > 72 > HIST + FRESH


@pytest.mark.parametrize("variant,src,L,tuning,steps", COPY_ENVS, ids=COPY_IDS)
def test_cross_env_copy_continues_like_the_source(voxnav, variant, src, L, tuning, steps):
    a, hist_a = stepped(variant, src, L, tuning, NA, 42, 7)
    b, hist_b = stepped(variant, src, L, tuning, NB, 1000, 11, seed_stride=NA)
    ex_a, ex_b = exports(a), exports(b)
    rej = b.copy_agents(a, INDEX)
    assert rej.dtype == torch.int32 and rej.device.type == "cuda" and int(rej.item()) == 0
    copied, kept = np.flatnonzero(INDEX >= 0), np.flatnonzero(INDEX < 0)
    for got, src_rows, own in zip(exports(b), ex_a, ex_b):
        np.testing.assert_array_equal(got[copied], src_rows[INDEX[copied]])
        np.testing.assert_array_equal(got[kept], own[kept])
    for got, want in zip(exports(a), ex_a):              # the source env is only read
        np.testing.assert_array_equal(got, want)
    acts = fresh_actions(NB, steps)
    got = launch_all(b, acts, [steps])
    orc, oenv = expect_after_copy(variant, src, L, INDEX, 42 + np.arange(NA), hist_a, 1000 + np.arange(NB), hist_b, acts)
    assert_rows(got, orc, "B after the copy")
    assert_exports(b, oenv, "B after the copy")
    ended = (orc["terminated"] | orc["truncated"]).astype(bool)
    if steps > FRESH:                                    # every agent passes an auto-reset on its (copied) seed schedule
        assert ended.any(0).all()
    elif src == "box:8x8x4":                             # simpleEnv: copied agents reach goals and go on from the copied seeds
        assert ended[:, copied].sum() >= 4
    a.close()
    b.close()


@pytest.mark.parametrize("variant,src,L,tuning,steps", COPY_ENVS, ids=COPY_IDS)
def test_in_place_fan_out(voxnav, variant, src, L, tuning, steps):
    """dst == src: agents 0..3 onto slots 4..47."""
    a, hist = stepped(variant, src, L, tuning, NA, 42, 7)
    index = np.where(np.arange(NA) < 4, -1, np.arange(NA) % 4).astype(np.int32)
    ex0 = exports(a)
    assert int(a.copy_agents(a, index).item()) == 0
    for got, before in zip(exports(a), ex0):
        np.testing.assert_array_equal(got, before[np.arange(NA) % 4])
    acts = fresh_actions(NA, steps, seed=78)
    got = launch_all(a, acts, [1, steps - 1])            # the one-step launch reads the copied window records
    seeds = 42 + np.arange(NA)
    orc, oenv = expect_after_copy(variant, src, L, index, seeds, hist, seeds, hist, acts)
    assert_rows(got, orc, "after the fan-out")
    assert_exports(a, oenv, "after the fan-out")
    a.close()


def test_same_env_permutation_is_rejected_for_every_agent(voxnav):
    for variant, tuning in (("cubic", MODES["2"]), ("simple", None)):
        a, _ = stepped(variant, "box:8x8x4", 4, tuning, NA, 42, 7)
        ex0, raw0 = exports(a), raw_rows(a, np_(a.snapshot().data))
        rej = a.copy_agents(a, (np.arange(NA) + 1) % NA)
        assert int(rej.item()) == NA
        for got, want in zip(exports(a), ex0):
            np.testing.assert_array_equal(got, want)
        assert_raw_equal(raw_rows(a, np_(a.snapshot().data)), raw0)       # every raw per-agent buffer
        # a self-index is no write: its readers are served; one with a seed override is written, so they are not
        index = np.array([0, 0, 0] + [-1] * (NA - 3), dtype=np.int32)
        assert int(a.copy_agents(a, index).item()) == 0
        np.testing.assert_array_equal(np_(a.export_state())[[1, 2]], ex0[0][[0, 0]])
        seeds = np.array([9, -1, -1] + [-1] * (NA - 3), dtype=np.int64)
        index[1] = -1
        st1 = np_(a.export_state())
        assert int(a.copy_agents(a, index, seeds).item()) == 1            # agent 2 reads agent 0, which is written
        st2 = np_(a.export_state())
        assert st2[0, 15] == 9 and (st2[0, :15] == st1[0, :15]).all()
        np.testing.assert_array_equal(st2[1:], st1[1:])
        a.close()


def test_range_and_seed_rejections_are_counted_and_left_untouched(voxnav):
    for variant, tuning in (("cubic", MODES["1"]), ("simple", {"simple_layout": 1})):
        a, _ = stepped(variant, "box:8x8x4", 4, tuning, NA, 42, 7)
        b, _ = stepped(variant, "box:8x8x4", 4, tuning, NB, 1000, 11, seed_stride=NA)
        ex_a, ex_b, snap_b = exports(a), exports(b), np_(b.snapshot().data)
        index = np.arange(NB, dtype=np.int32) * 2
        seeds = np.full(NB, -1, dtype=np.int64)
        index[2], index[5] = NA, -2                        # >= N_src, < -1
        seeds[7], seeds[11] = -2, 2 ** 32                  # < -1, >= 2^32
        seeds[3], seeds[4] = 2 ** 32 - 1, 0                # the range's ends are accepted
        bad = [2, 5, 7, 11]
        good = [i for i in range(NB) if i not in bad]
        assert int(b.copy_agents(a, index, seeds).item()) == len(bad)
        st, bl = exports(b)
        np.testing.assert_array_equal(st[bad], ex_b[0][bad])
        np.testing.assert_array_equal(bl[bad], ex_b[1][bad])
        want = ex_a[0][index[good]].copy()
        want[good.index(3), 15], want[good.index(4), 15] = 2 ** 32 - 1, 0
        np.testing.assert_array_equal(st[good], want)
        np.testing.assert_array_equal(bl[good], ex_a[1][index[good]])
        # bit-identical: the rejected agents' share of every raw buffer
        parts_before, parts_after = raw_rows(b, snap_b), raw_rows(b, np_(b.snapshot().data))
        for name in parts_before:
            np.testing.assert_array_equal(parts_after[name][bad], parts_before[name][bad], err_msg=name)
        a.close()
        b.close()


def raw_rows(env, blob):
    """Per-agent rows of a snapshot blob's parts (include/voxnav.h: each part starts on a 256-byte boundary; the
    bytes between parts are not written): hot words, window records, next seeds, belief blocks, goals, draw-ahead
    rows, episode records and, where the blob has them, stood rows and nonzero-set masks."""
    N, ab = env.num_agents, env.info.belief_bytes_per_agent
    wrec = 16 * env.info.pad_h if env.variant == 0 else 0
    out, off = {}, 0
    for name, per_agent in (("hot+wrec", 16 + wrec), ("seed", 4), ("belief", ab), ("goal", 4), ("predraw", 16),
                            ("episodes", 64), ("stood+pnz", 128 + 8)):
        if off == len(blob):
            assert name == "stood+pnz"
            break
        part = blob[off:off + N * per_agent]
        if name == "hot+wrec":
            out["hot"], out["wrec"] = part[:16 * N].reshape(N, 16), part[16 * N:].reshape(N, wrec)
        elif name == "stood+pnz":
            out["stood"], out["pnz"] = part[:128 * N].reshape(N, 128), part[128 * N:].reshape(N, 8)
        else:
            out[name] = part.reshape(N, per_agent)
        off += (N * per_agent + 255) & ~255
    assert off == len(blob)
    return out


def assert_raw_equal(got, want):
    assert got.keys() == want.keys()
    for name in want:
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)


@pytest.mark.parametrize("variant,tuning", [("cubic", MODES["2"]), ("cubic", MODES["0/df1"]), ("simple", None),
                                            ("simple", {"simple_layout": 1})],
                         ids=["cubic-2", "cubic-0df1", "simple-lines", "simple-words"])
def test_seed_override_starts_the_next_episode_from_that_seed(voxnav, variant, tuning):
    src, L = "box:8x8x4", 4
    a, _ = stepped(variant, src, L, tuning, NA, 42, 7)
    b, _ = stepped(variant, src, L, tuning, NB, 1000, 11, seed_stride=NA)
    index = np.arange(NB, dtype=np.int32) + 5
    seeds = np.where(np.arange(NB) % 2 == 0, 5000 + 17 * np.arange(NB), -1).astype(np.int64)
    if variant == "simple":
        # sources whose draw-ahead row {start, goal, seed, valid} is valid for their next seed (a row is consumed
        # by the reset that uses it and drawn again later): an override must leave the copied row unused
        raw = raw_rows(a, np_(a.snapshot().data))
        pre, nxt = raw["predraw"].view(np.uint32), raw["seed"].view(np.uint32)[:, 0]
        valid = np.flatnonzero((pre[:, 3] == 1) & (pre[:, 2] == nxt))
        assert len(valid) >= NB
        index = valid[:NB].astype(np.int32)
    next_a = np_(a.export_state())[:, 15]
    assert int(b.copy_agents(a, index, seeds).item()) == 0
    want = np.where(seeds >= 0, seeds, next_a[index])
    np.testing.assert_array_equal(np_(b.export_state())[:, 15], want)
    K = 80                                               # max_steps is 72 (cubic) / below it (simple): every episode ends
    ro = b.step_actions(np.random.default_rng(3).integers(0, 6, size=(K, NB)).astype(np.int32))
    ended = np_(ro.terminated | ro.truncated).astype(bool)
    assert ended.any(0).all()
    first = ended.argmax(0)
    fresh = make_env(variant, src, L, NB, tuning, seed_stride=NA)
    obs0 = np_(fresh.reset(seed=torch.as_tensor(want)))
    got = np_(ro.obs)[first, np.arange(NB)]
    assert got.tobytes() == obs0.tobytes()
    for e in (a, b, fresh):
        e.close()


@pytest.mark.parametrize("variant,tuning", [("cubic", MODES["2"]), ("simple", None)], ids=["cubic-2", "simple-lines"])
def test_episode_records_stay_with_the_slot(voxnav, variant, tuning):
    """The copy leaves the destination slots' records alone; the copied running episode's counters travel in the
    hot state, so the slot's next record is the one the source's slot gets for the same episode."""
    src, L = "box:8x8x4", 4
    a, _ = stepped(variant, src, L, tuning, NA, 42, 7)
    b, _ = stepped(variant, src, L, tuning, NB, 1000, 11, seed_stride=NA)
    b.step_random(70, policy_seed=11)                    # B's slots have ended episodes on record
    a.step_random(3, policy_seed=7)
    index = np.where(np.arange(NB) % 2 == 1, 2 * np.arange(NB) + 1, -1).astype(np.int32)    # distinct sources
    copied = np.flatnonzero(index >= 0)
    rec_a0, rec_b0 = np_(a.episode_records()), np_(b.episode_records())
    assert (rec_b0[:, 0] >= 1).all()
    st_a = np_(a.export_state())
    assert int(b.copy_agents(a, index).item()) == 0
    np.testing.assert_array_equal(np_(b.episode_records()), rec_b0)
    K = 45
    acts_b = np.random.default_rng(4).integers(0, 6, size=(K, NB)).astype(np.int32)
    acts_a = np.random.default_rng(5).integers(0, 6, size=(K, NA)).astype(np.int32)
    acts_a[:, index[copied]] = acts_b[:, copied]
    ro_b, ro_a = b.step_actions(acts_b), a.step_actions(acts_a)
    ended_b = np_(ro_b.terminated | ro_b.truncated).astype(bool)
    assert (np_(ro_a.terminated | ro_a.truncated).astype(bool)[:, index[copied]] == ended_b[:, copied]).all()
    assert ended_b[:, copied].any(0).all() if variant == "cubic" else ended_b[:, copied].any(0).sum() >= 4
    rec_a1, rec_b1 = np_(a.episode_records()), np_(b.episode_records())
    # the totals grow by what the source's slot recorded for the same episodes; where one ended, the last episode is
    # the same, and a slot whose copy ended none keeps its own last episode
    np.testing.assert_array_equal(rec_b1[copied, :6] - rec_b0[copied, :6], (rec_a1 - rec_a0)[index[copied], :6])
    some, none = copied[ended_b[:, copied].any(0)], copied[~ended_b[:, copied].any(0)]
    np.testing.assert_array_equal(rec_b1[some, 6:], rec_a1[index[some], 6:])
    np.testing.assert_array_equal(rec_b1[none], rec_b0[none])
    once = copied[ended_b[:, copied].sum(0) == 1]
    assert variant != "cubic" or len(once) == len(copied)
    # an episode that ended once: the copied step count plus the steps taken here
    np.testing.assert_array_equal(rec_b1[once, 6], st_a[index[once], 5] + ended_b[:, once].argmax(0) + 1)
    a.close()
    b.close()


def test_incompatible_envs_are_refused_with_nothing_written(voxnav):
    from voxnav._native import VoxnavError
    src, L = "box:16x16x8", 7
    b, _ = stepped("cubic", src, L, MODES["2"], NB, 1000, 11, seed_stride=NA)
    before, raw = exports(b), raw_rows(b, np_(b.snapshot().data))
    others = [make_env("cubic", src, 6, NA, MODES["2"]), make_env("cubic", src, L, NA, MODES["1"]),
              make_env("cubic", "box:16x12x8", L, NA, MODES["2"]), make_env("simple", src, L, NA, None),
              make_env("cubic", src, L, NA, MODES["2"], seed_stride=NA + 1)]
    for other in others:
        other.reset(seed=5)
        with pytest.raises(VoxnavError, match=r"vn_copy_agents failed \(-1\).*layout tag"):
            b.copy_agents(other, np.arange(NB, dtype=np.int32))
        other.close()
    for got, want in zip(exports(b), before):
        np.testing.assert_array_equal(got, want)
    assert_raw_equal(raw_rows(b, np_(b.snapshot().data)), raw)
    unreset = make_env("cubic", src, L, NA, MODES["2"])
    with pytest.raises(RuntimeError):
        b.copy_agents(unreset, np.arange(NB, dtype=np.int32))
    # another size and agent_id_base are what the layout tag leaves out
    c = make_env("cubic", src, L, 7, MODES["2"], seed_stride=NA, agent_id_base=100)
    c.reset(seed=1)
    assert int(c.copy_agents(b, np.arange(7, dtype=np.int32)).item()) == 0
    np.testing.assert_array_equal(np_(c.export_state()), before[0][:7])
    for e in (b, unreset, c):
        e.close()
