"""Return-based reward normalisation on the GPU: vn_return_moments / vn_reward_normalize through the
raw C-ABI against the float64 restatement (tests/rnorm_helpers.py, pinned to csrc/ret_rms.h by
tests/test_reward_norm_host.py), bit for bit -- statistics, returns, per-step scales and the
normalised f32 rewards -- then segment splitting, repeatability, guard values, two shards in one
process, the refused arguments, and voxnav.normalize.RewardNormalizer inside RolloutCollector /
DaggerCollector / ppo.learn and through the checkpoint functions.

Bit-equality rests on f64 division and square root being correctly rounded on gfx950 and on the
library being built without contraction.
"""
import ctypes as C

import numpy as np
import pytest

import bc_helpers as bh
import rnorm_helpers as rn
from helpers import product_room_set

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAND = 64
EPS = 1e-8


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from voxnav import _native
    return _native.load()


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Guarded:
    """A device array with BAND sentinel elements on either side of the payload."""

    def __init__(self, data: np.ndarray):
        data = np.ascontiguousarray(data)
        self.sent = {np.dtype(np.float32): np.float32(-12345.5), np.dtype(np.float64): np.float64(-12345.5)}[data.dtype]
        raw = np.full(data.size + 2 * BAND, self.sent, data.dtype)
        raw[BAND:BAND + data.size] = data.ravel()
        self.raw = torch.from_numpy(raw).to(DEV)
        self.t = self.raw[BAND:BAND + data.size].view(data.shape)

    def np(self):
        return self.t.cpu().numpy()

    def intact(self):
        r = self.raw.cpu().numpy()
        return bool((r[:BAND] == self.sent).all() and (r[-BAND:] == self.sent).all())


def gpu_run(lib, rewards, dones, rms, ret, t0, t1, gamma, clip=10.0, training=True, shards=None, scale_out=True):
    """Both calls per shard, the shards' triples concatenated in between; every shard normalises its
    own rewards with its own copy of the statistics (as ranks would).
    -> dict(rms [S][3], ret [N], scales [S][t1 - t0], rewards [T][N], guards intact, rcs)."""
    from voxnav import _native
    T, N = rewards.shape
    sizes = [N] if shards is None else list(shards)
    bases = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(int)
    steps = t1 - t0
    sh = []
    for b, n in zip(bases, sizes):
        c = -(-n // 64)
        sh.append(dict(n=n, base=int(b), c=c, rew=Guarded(rewards[:, b:b + n]), ret=Guarded(ret[b:b + n]),
                       dones=torch.from_numpy(np.ascontiguousarray(dones[:, b:b + n])).to(DEV),
                       part=Guarded(np.zeros((steps, c, 3))), rms=Guarded(np.asarray(rms, np.float64)),
                       scales=Guarded(np.zeros(steps))))
    if training:
        for s in sh:
            _native.check(lib.vn_return_moments(p(s["rew"].t), p(s["dones"]), t0, t1, s["n"], s["base"], float(gamma),
                                                p(s["ret"].t), p(s["part"].t), None), "vn_return_moments")
        allp = np.concatenate([s["part"].np() for s in sh], axis=1)
    cg = -(-N // 64)
    for s in sh:
        gp = Guarded(allp) if training else None
        _native.check(lib.vn_reward_normalize(p(s["rew"].t), t0, t1, s["n"], p(gp.t) if training else None,
                                              cg if training else 0, p(s["rms"].t), EPS, float(clip),
                                              int(training), p(s["scales"].t) if scale_out else None, None),
                      "vn_reward_normalize")
        s["gp"] = gp
    torch.cuda.synchronize()
    guards = all(s[k].intact() for s in sh for k in ("rew", "ret", "part", "rms", "scales")) and \
        all(s["gp"] is None or s["gp"].intact() for s in sh)
    return dict(rms=np.stack([s["rms"].np() for s in sh]), ret=np.concatenate([s["ret"].np() for s in sh]),
                scales=np.stack([s["scales"].np() for s in sh]),
                rewards=np.concatenate([s["rew"].np() for s in sh], axis=1), guards=guards,
                partials=allp if training else None)


def ref_run(rewards, dones, rms, ret, t0, t1, gamma, clip=10.0, training=True, shards=None):
    st = dict(rms=np.asarray(rms, np.float64).copy(), ret=np.asarray(ret, np.float64).copy())
    rew = rewards.copy()
    sc = rn.run(st, rew, dones, t0, t1, gamma, epsilon=EPS, clip=clip, training=training, shards=shards)
    return dict(rms=st["rms"], ret=st["ret"], scales=sc, rewards=rew)


def assert_bits(got, want, what):
    """Bit-equality of every output; on a mismatch the message names the first quantity that differs."""
    for k in ("ret", "rms", "scales", "rewards"):
        g = got[k] if k in ("ret", "rewards") else got[k][0]
        if g.tobytes() != want[k].tobytes():
            bad = np.argwhere(np.asarray(g != want[k]).reshape(g.shape))
            i = tuple(bad[0]) if len(bad) else ()
            raise AssertionError(f"{what}: {k} differs in {len(bad)} of {g.size} places, first at {i}: "
                                 f"gpu {g[i]!r} vs restatement {want[k][i]!r}")
    for k in ("rms", "scales"):        # every shard's copy of the statistics is the same
        assert all(row.tobytes() == got[k][0].tobytes() for row in got[k]), f"{what}: shards disagree on {k}"
    assert got["guards"], f"{what}: a guard value was overwritten"


def _inputs(N, T, variant, seed):
    rng = np.random.default_rng(seed)
    if variant == "default":      # the initial state, ordinary rewards
        rew = rng.uniform(-1.0, 2.0, (T, N)).astype(np.float32)
        rms, ret, clip = (0.0, 1.0, 1e-4), np.zeros(N), 10.0
    elif variant == "loaded":     # a loaded state with count = 64 and returns under way
        rew = rng.normal(0.5, 3.0, (T, N)).astype(np.float32)
        rms, ret, clip = (0.5, 2.0, 64.0), rng.normal(0.0, 3.0, N), 10.0
    else:                         # rewards of +-100 on a settled variance of 1: clipped to +-10 from both sides
        rew = (rng.choice([-100.0, 100.0], (T, N)) * rng.choice([1.0, 0.01], (T, N), p=[0.7, 0.3])).astype(np.float32)
        rew[0, 0], rew[-1, -1] = 100.0, -100.0
        if N > 2:
            rew[0, 1] = 0.5       # and one inside the clip
        rms, ret, clip = (0.0, 1.0, 1e6), np.zeros(N), 10.0
    dones = (rng.random((T, N)) < 0.15).astype(np.float32)
    dones[0, ::2] = 1.0           # episodes end on the first and on the last step of the segment
    dones[-1, ::3] = 1.0
    return rew, dones, np.array(rms), ret, clip


@pytest.mark.parametrize("N", [1, 63, 64, 65, 130, 320])
def test_raw_abi_equals_restatement(lib, N):
    """One lane, a short last chunk, chunk counts 1, 2, 3 and 5 (a non-power-of-two tree); T 1 and 7;
    gamma 0, 0.99 and 1; the initial state, a loaded one and the clip."""
    for T in (1, 7):
        for gamma in (0.0, 0.99, 1.0):
            for variant in ("default", "loaded", "clip"):
                rew, dones, rms, ret, clip = _inputs(N, T, variant, 1000 * N + 10 * T + int(gamma * 100))
                got = gpu_run(lib, rew, dones, rms, ret, 0, T, gamma, clip)
                want = ref_run(rew, dones, rms, ret, 0, T, gamma, clip)
                assert_bits(got, want, f"N={N} T={T} gamma={gamma} {variant}")
                if variant == "clip":
                    r = got["rewards"]
                    assert (np.abs(r) == 10.0).any()
                    if N > 2:
                        assert (r == 10.0).any() and (r == -10.0).any() and (np.abs(r) < 10.0).any()
    # not training: one scale from the stored var, state untouched, partials NULL
    rew, dones, rms, ret, clip = _inputs(N, 7, "loaded", 5)
    got = gpu_run(lib, rew, dones, rms, ret, 0, 7, 0.99, clip, training=False)
    assert_bits(got, ref_run(rew, dones, rms, ret, 0, 7, 0.99, clip, training=False), f"N={N} not training")
    assert got["rms"][0].tobytes() == rms.tobytes() and got["ret"].tobytes() == ret.tobytes()
    # without scale_out
    a = gpu_run(lib, rew, dones, rms, ret, 0, 7, 0.99, clip, scale_out=False)
    b = gpu_run(lib, rew, dones, rms, ret, 0, 7, 0.99, clip)
    assert a["rewards"].tobytes() == b["rewards"].tobytes() and a["rms"].tobytes() == b["rms"].tobytes()
    assert (a["scales"] == 0).all() and a["guards"]


@pytest.mark.parametrize("N,T", [(130, 70), (1, 1030), (64 * 513 + 1, 2)])
def test_tile_boundaries(lib, N, T):
    """The sizes at which the kernels start another tile: more than 64 steps in the moments scan
    (and a last load batch that is not full), more than 1024 steps in the chain, more than 512
    chunks in the tree (a second level over the tile roots, the last tile holding two chunks, one
    of them a single agent)."""
    rew, dones, rms, ret, clip = _inputs(N, T, "loaded", N + T)
    got = gpu_run(lib, rew, dones, rms, ret, 0, T, 0.99, clip)
    assert_bits(got, ref_run(rew, dones, rms, ret, 0, T, 0.99, clip), f"N={N} T={T}")


def test_segments_compose_and_repeat(lib):
    """[0, 3) then [3, 7) equals [0, 7) bitwise (rows outside a segment untouched); two calls on
    equal inputs give equal bits."""
    N, T = 130, 7
    rew, dones, rms, ret, clip = _inputs(N, T, "default", 31)
    whole = gpu_run(lib, rew, dones, rms, ret, 0, T, 0.99)
    again = gpu_run(lib, rew, dones, rms, ret, 0, T, 0.99)
    for k in ("rms", "ret", "scales", "rewards", "partials"):
        assert whole[k].tobytes() == again[k].tobytes(), k
    a = gpu_run(lib, rew, dones, rms, ret, 0, 3, 0.99)
    assert a["rewards"][3:].tobytes() == rew[3:].tobytes() and a["guards"]
    b = gpu_run(lib, a["rewards"], dones, a["rms"][0], a["ret"], 3, 7, 0.99)
    assert b["rewards"][:3].tobytes() == a["rewards"][:3].tobytes() and b["guards"]
    for k in ("rms", "ret", "rewards"):
        assert b[k].tobytes() == whole[k].tobytes(), k
    assert np.concatenate([a["scales"][0], b["scales"][0]]).tobytes() == whole["scales"][0].tobytes()


def test_two_shards_in_one_process(lib):
    """agent_id_base 0 and 128, the triples concatenated: the unsharded run, bit for bit."""
    N, T = 193, 7
    rew, dones, rms, ret, clip = _inputs(N, T, "loaded", 77)
    one = gpu_run(lib, rew, dones, rms, ret, 0, T, 0.99)
    two = gpu_run(lib, rew, dones, rms, ret, 0, T, 0.99, shards=(128, 65))
    want = ref_run(rew, dones, rms, ret, 0, T, 0.99, shards=(128, 65))
    assert_bits(two, want, "two shards")
    assert_bits(one, want, "one shard")
    assert one["partials"].tobytes() == two["partials"].tobytes()


def test_invalid_arguments_are_refused(lib):
    N, T = 65, 4
    rew = torch.zeros((T, N), device=DEV)
    dn = torch.zeros((T, N), device=DEV)
    ret = torch.zeros(N, dtype=torch.float64, device=DEV)
    part = torch.zeros((T, 2, 3), dtype=torch.float64, device=DEV)
    rms = torch.tensor([0.0, 1.0, 1e-4], dtype=torch.float64, device=DEV)

    def refused(rc, word):
        msg = lib.vn_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    mom = lambda **k: lib.vn_return_moments(*[k.get(n, d) for n, d in (  # noqa: E731
        ("rew", p(rew)), ("dn", p(dn)), ("t0", 0), ("t1", T), ("N", N), ("base", 0), ("g", 0.99), ("ret", p(ret)),
        ("part", p(part)), ("s", None))])
    refused(mom(base=32), "multiple of 64")
    refused(mom(base=-64), "multiple of 64")
    refused(mom(rew=None), "NULL")
    refused(mom(dn=None), "NULL")
    refused(mom(ret=None), "NULL")
    refused(mom(part=None), "NULL")
    refused(mom(t0=2, t1=2), "t0")
    refused(mom(t0=-1), "t0")
    refused(mom(N=0), "N must")
    nor = lambda **k: lib.vn_reward_normalize(*[k.get(n, d) for n, d in (  # noqa: E731
        ("rew", p(rew)), ("t0", 0), ("t1", T), ("N", N), ("part", p(part)), ("C", 2), ("rms", p(rms)), ("eps", EPS),
        ("clip", 10.0), ("upd", 1), ("sc", None), ("s", None))])
    refused(nor(rew=None), "NULL")
    refused(nor(rms=None), "NULL")
    refused(nor(part=None), "partials")
    refused(nor(t1=0), "t0")
    refused(nor(t0=3, t1=2), "t0")
    refused(nor(N=0), "N must")
    refused(nor(clip=0.0), "clip")
    refused(nor(clip=-1.0), "clip")
    refused(nor(clip=float("nan")), "clip")
    refused(nor(eps=-1.0), "epsilon")
    refused(nor(C=1), "C_global")          # fewer chunks than this shard's own
    refused(nor(C=262145), "C_global")
    refused(nor(t1=65536), "steps")
    torch.cuda.synchronize()
    assert float(rew.abs().sum()) == 0.0 and rms.tolist() == [0.0, 1.0, 1e-4]
    assert mom() == 0 and nor() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the collector
T_, N_, L_ = 8, 65, 4
GAMMA = 0.99


def _collector(kind, norm, flush, cls=None, **kw):
    from voxnav.collector import RolloutCollector
    from voxnav.env import BatchedGridEnv
    from voxnav.normalize import RewardNormalizer
    env = BatchedGridEnv(num_agents=N_, rooms=product_room_set("ctor:4x4x3"), local_map_length=L_, device=DEV)
    rnorm = RewardNormalizer(N_, GAMMA, device=DEV) if norm else None
    col = (cls or RolloutCollector)(env, bh.small_policy(kind == "lstm").to(DEV), n_steps=T_, gamma=GAMMA,
                                    sample_seed=1234, reset_seed=42, reward_norm=rnorm, **kw)
    if flush:
        col._flush_every = flush        # the mid-rollout flush (default min(T, 4 * 4) = 8: none)
    log = []
    orig = col._bootstrap

    def spy(count):                     # the rewards as each bootstrap found them, and the stash it used
        pre = col.rewards.clone()
        orig(count)
        M = int(count.item())
        log.append(dict(pre=pre.cpu().numpy(), flat=col._stash_flat[:M].cpu().numpy(), tv=col._tv[:M].cpu().numpy(),
                        t=col.t_global))
    col._bootstrap = spy
    return env, col, log


def _pre_bootstrap(log, t_first):
    """[T][N] rewards as they stood before any bootstrap touched them: each flush's own rows."""
    out, a = np.zeros_like(log[0]["pre"]), 0
    for e in log:
        b = e["t"] - t_first
        out[a:b] = e["pre"][a:b]
        a = b
    assert a == out.shape[0]
    return out


@pytest.mark.parametrize("kind,flush", [("mlp", None), ("lstm", None), ("mlp", 3)])
def test_collector_with_normaliser(lib, kind, flush):
    """4 x 4 x 3 walled box (max_steps 4: truncations and bootstraps inside the 8-step rollout), 65
    agents, two rollouts (the carried returns and statistics)."""
    from voxnav.gae import compute_gae
    envp, plain, plog = _collector(kind, False, flush)
    envn, normd, nlog = _collector(kind, True, flush)
    st = rn.new_state(N_)
    boots = 0
    for r in range(2):
        plog.clear(), nlog.clear()
        bp, bn = plain.collect(), normd.collect()
        torch.cuda.synchronize()
        assert len(nlog) == len(plog) == (3 if flush else 1)
        for f in ("obs", "actions", "values", "log_probs", "episode_starts", "dones", "last_values"):
            assert torch.equal(getattr(bp, f), getattr(bn, f)), f
        ep, en = plain.monitor.last_episodes, normd.monitor.last_episodes
        assert ep["agent"].tolist() == en["agent"].tolist() and ep["step"].tolist() == en["step"].tolist()
        assert torch.equal(torch.as_tensor(ep["return"]), torch.as_tensor(en["return"])) and len(ep["agent"]) > 0
        assert plain.monitor.ep_rew_mean() == normd.monitor.ep_rew_mean()
        # the raw rewards, normalised by the restatement, are what every bootstrap of the
        # normalising collector found, bit for bit
        raw = _pre_bootstrap(plog, r * T_)
        dones = np.concatenate([bp.episode_starts.cpu().numpy()[1:], bp.dones.cpu().numpy()[None]])
        want = raw.copy()
        rn.run(st, want, dones, 0, T_, GAMMA)
        assert _pre_bootstrap(nlog, r * T_).tobytes() == want.tobytes()
        assert normd.reward_norm.rms.cpu().numpy().tobytes() == st["rms"].tobytes()
        assert normd.reward_norm.ret.cpu().numpy().tobytes() == st["ret"].tobytes()
        # plus gamma * V(terminal obs) from the stash values, in normalised units
        flat = np.concatenate([e["flat"] for e in nlog])
        tv = np.concatenate([e["tv"] for e in nlog])
        # (stash rows land in the waves' completion order: a set keyed by the flat index)
        assert sorted(flat.tolist()) == sorted(np.concatenate([e["flat"] for e in plog]).tolist())
        assert len(set(flat.tolist())) == len(flat)
        boots += len(flat)
        exp = want.astype(np.float64).ravel()
        exp[flat] += GAMMA * tv.astype(np.float64)
        got = bn.rewards.cpu().numpy().ravel()
        mask = np.zeros(got.size, bool)
        mask[flat] = True
        assert np.array_equal(got[~mask], want.ravel()[~mask])
        assert (np.abs(got[mask] - exp[mask]) <= 1e-4 + 1e-5 * np.abs(exp[mask])).all()
        adv, ret = compute_gae(bn.rewards, bn.values, bn.episode_starts, bn.last_values, bn.dones, GAMMA, 0.95)
        assert torch.equal(adv, bn.advantages) and torch.equal(ret, bn.returns)
        assert not torch.equal(bn.rewards, bp.rewards)
    assert boots > 0, "the room must produce truncations inside the rollout"
    envp.close(), envn.close()


def test_collector_refuses_a_foreign_normaliser(lib):
    from voxnav.collector import RolloutCollector
    from voxnav.env import BatchedGridEnv
    from voxnav.normalize import RewardNormalizer
    env = BatchedGridEnv(num_agents=N_, rooms=product_room_set("ctor:4x4x3"), local_map_length=L_, device=DEV)
    pol = bh.small_policy(False).to(DEV)
    with pytest.raises(ValueError, match="reward_norm"):
        RolloutCollector(env, pol, n_steps=T_, reward_norm=RewardNormalizer(N_ + 1, 0.99, device=DEV))
    with pytest.raises(ValueError, match="discounts"):
        RolloutCollector(env, pol, n_steps=T_, gamma=0.99, reward_norm=RewardNormalizer(N_, 0.9, device=DEV))
    with pytest.raises(ValueError, match="multiple of 64"):
        RewardNormalizer(N_, 0.99, agent_id_base=32, n_global=200, device=DEV)
    with pytest.raises(ValueError, match="process_group"):
        RewardNormalizer(N_, 0.99, agent_id_base=0, n_global=200, device=DEV)
    env.close()


def test_dagger_collector_accepts_the_normaliser(lib):
    from voxnav.imitate import DaggerCollector
    env, col, log = _collector("mlp", True, None, cls=DaggerCollector, beta=0.5)
    buf = col.collect()
    torch.cuda.synchronize()
    rms = col.reward_norm.rms.cpu().numpy()
    assert abs(rms[2] - (1e-4 + T_ * N_)) < 1e-9 and rms[1] > 0 and np.isfinite(rms).all()
    assert float(buf.rewards.abs().max()) <= 10.0 + 1e-4 + 0.99 * float(col._tv.abs().max())
    assert buf.expert_actions.shape == (T_, N_)
    env.close()


def test_ppo_learn_reports_the_statistics(lib):
    from voxnav.ppo import PPOLearner, learn
    env, col, _ = _collector("mlp", True, None)
    hist = learn(col, PPOLearner(col.policy, n_epochs=1, batch_size=260, seed=1), total_timesteps=T_ * N_)
    assert len(hist) == 1 and np.isfinite(hist[0]["loss"])
    assert hist[0]["ret_rms_var"] == col.reward_norm.var > 0 and hist[0]["ret_rms_mean"] == col.reward_norm.mean
    env2, col2, _ = _collector("mlp", False, None)
    h2 = learn(col2, PPOLearner(col2.policy, n_epochs=1, batch_size=260, seed=1), total_timesteps=T_ * N_)
    assert "ret_rms_var" not in h2[0]
    env.close(), env2.close()


def test_checkpoint_round_trip(lib, tmp_path):
    from voxnav.checkpoint import load_reward_norm, save_reward_norm
    from voxnav.normalize import RewardNormalizer
    a = RewardNormalizer(130, 0.99, device=DEV)
    rew, dones, _, _, _ = _inputs(130, 7, "default", 3)
    starts = torch.from_numpy(np.concatenate([np.zeros((1, 130), np.float32), dones])).to(DEV)
    r = torch.from_numpy(rew).to(DEV)
    a.normalize_segment(r, starts, 0, 7)
    want = ref_run(rew, dones, (0.0, 1.0, 1e-4), np.zeros(130), 0, 7, 0.99)
    assert r.cpu().numpy().tobytes() == want["rewards"].tobytes()
    assert a.last_scales.cpu().numpy().tobytes() == want["scales"].tobytes()
    path = save_reward_norm(tmp_path / "rnorm", a)
    assert path.suffix == ".npz"
    b = RewardNormalizer(130, 0.99, device=DEV)
    load_reward_norm(path, b)
    assert torch.equal(a.rms, b.rms) and torch.equal(a.ret, b.ret)
    assert b.rms.cpu().numpy().tobytes() == want["rms"].tobytes() and (b.var, b.mean) == (a.var, a.mean)
    with pytest.raises(ValueError, match="agents"):
        load_reward_norm(path, RewardNormalizer(131, 0.99, device=DEV))
    # training = False: scaled by the stored var, nothing moves
    b.training = False
    r2 = torch.from_numpy(rew).to(DEV)
    b.normalize_segment(r2, starts, 0, 7)
    assert torch.equal(a.rms, b.rms) and torch.equal(a.ret, b.ret)
    assert r2.cpu().numpy().tobytes() == rn.normalize_rewards(rew, rn.scale(want["rms"][1])).tobytes()
    with pytest.raises(ValueError, match="contiguous"):
        b.normalize_segment(r2.double(), starts, 0, 7)
