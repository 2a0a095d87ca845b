"""The DAgger warm start on the GPU: vn_bc_loss and vn_dagger_mix (csrc/voxnav_bc_loss.hip) against
the float64 restatements of tests/bc_helpers.py, ``DaggerCollector`` against a plain collector and
the CPU oracle's replay, ``BCLearner`` against the restated train call, and ``warm_start`` end to end.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bc_helpers as bh  # noqa: E402
import route_helpers as rh  # noqa: E402
from helpers import oracle_env, product_room_set  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def np_(t):
    return t.detach().cpu().numpy()


def _close(got, ref, rel, floor, what):
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    bound = rel * (float(np.abs(ref).max()) if ref.size else 0.0) + floor
    print(f"{what}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (what, err, bound)


# ------------------------------------------------------------------ 5. vn_bc_loss
# M: the 4-sample pass (1, 3, 4, 5) and the 128-sample block edges (127, 128, 129) of the kernel,
# which lays the samples out as vn_ppo_loss does (32 per wave, 4 waves per block), and more than
# 64 count blocks' worth of blocks (4099: 33 loss blocks, 65 samples per count block)
BC_M = [1, 3, 4, 5, 127, 128, 129, 4099]
# (gather through src, weights, ent_coef, vf_coef)
BC_MODES = [(False, None, 0.01, 0.5), (True, "random", 0.0, 0.5), (True, "zero", 0.01, 0.5),
            (False, "random", 0.01, 0.0), (True, None, 0.0, 0.5), (False, "zero", 0.0, 0.5)]


def _bc_loss_against_float64(M, F, A, modes):
    from voxnav.learn_ops import bc_loss
    torch.manual_seed(1000 * M + F + A)
    an, vn = torch.nn.Linear(F, A).to(DEV), torch.nn.Linear(F, 1).to(DEV)
    h = torch.tanh(torch.randn((2, M, F), device=DEV))
    for gather, wmode, ent, vf in modes:
        R = M + 1000 if gather else M
        src = torch.randperm(R, device=DEV)[:M].contiguous() if gather else None
        lab = torch.randint(0, A, (R,), device=DEV, dtype=torch.int32)
        ret = torch.randn(R, device=DEV)
        wgt = None if wmode is None else (torch.rand(R, device=DEV) < 0.7).to(torch.uint8) if wmode == "random" \
            else torch.zeros(R, dtype=torch.uint8, device=DEV)
        if wmode == "zero" and gather:
            wgt[torch.randperm(R, device=DEV)[M:]] = 1           # rows outside the minibatch do not count
            wgt[src] = 0
        dh, grads, stats = bc_loss(h, an, vn, src, lab, wgt, ret, ent, vf)
        dh2, grads2, stats2 = bc_loss(h, an, vn, src, lab, wgt, ret, ent, vf)
        assert torch.equal(dh, dh2) and torch.equal(stats, stats2)
        assert all(torch.equal(a, b) for a, b in zip(grads, grads2))
        g = lambda t: None if t is None else np_(t if src is None else t[src])  # noqa: E731
        rp, rv, rg, rstats = bh.bc_heads64(np_(h[0]), np_(h[1]), np_(an.weight), np_(an.bias), np_(vn.weight),
                                           np_(vn.bias), g(lab), g(wgt), g(ret), ent, vf)
        what = f"M={M} F={F} A={A} gather={gather} weights={wmode} ent={ent} vf={vf}"
        _close(np_(dh).astype(np.float64), np.stack([rp, rv]), 2e-5, 1e-9, what + " dh")
        for name, a, b in zip(("dWa", "dba", "dwv", "dbv"), grads, rg):
            assert tuple(a.shape) == tuple(np.shape(b)), name
            _close(np_(a).astype(np.float64).reshape(-1), np.asarray(b).reshape(-1), 1e-4, 1e-9, f"{what} {name}")
        st = np_(stats)
        _close(st[:4], rstats[:4], 1e-5, 1e-7, what + " stats")
        assert st[4] == rstats[4] and st[5] == rstats[5], (what, st[4:], rstats[4:])
        if wmode == "zero":
            assert st[0] == 0.0 and st[4] == 0.0 and st[5] == 0.0
            if ent == 0.0:
                assert float(dh[0].abs().max()) == 0.0


@pytest.mark.parametrize("A", [1, 6, 8])
@pytest.mark.parametrize("F", [64, 256])
@pytest.mark.parametrize("M", BC_M)
def test_bc_loss_matches_float64(M, F, A):
    """Tolerances of tests/test_learn_ops.py::test_ppo_loss_matches_float64: latent gradients 2e-5,
    head gradients 1e-4, logged sums 1e-5 relative; accuracy and labelled share exact.  Two calls
    on the same inputs give the same bits."""
    _bc_loss_against_float64(M, F, A, BC_MODES)


# every instantiation of the loss kernel (Q = F / 64, AM = A rounded up to even), at one full block
# plus one sample: a second block, a partial wave and padding groups; gathered with weights (the
# counted path) and plain (labelled count = M)
GRID_MODES = {"src+weights": (True, "random", 0.01, 0.5), "plain": (False, None, 0.01, 0.5)}


@pytest.mark.parametrize("mode", list(GRID_MODES))
@pytest.mark.parametrize("A", range(1, 9))
@pytest.mark.parametrize("F", [64, 128, 192, 256])
def test_bc_loss_grid_matches_float64(F, A, mode):
    """test_bc_loss_matches_float64's checks and tolerances on all 32 (F, A) pairs at M = 129."""
    _bc_loss_against_float64(129, F, A, [GRID_MODES[mode]])


def test_bc_loss_argmax_tie_goes_to_the_lowest_index():
    """Zero head weights: every logit ties, the argmax is action 0, ce = ln A."""
    from voxnav.learn_ops import bc_loss
    M, F, A = 37, 64, 6
    an, vn = torch.nn.Linear(F, A).to(DEV), torch.nn.Linear(F, 1).to(DEV)
    with torch.no_grad():
        an.weight.zero_()
        an.bias.zero_()
    h = torch.tanh(torch.randn((2, M, F), device=DEV))
    lab = (torch.arange(M, device=DEV) % A).to(torch.int32)
    _, grads, stats = bc_loss(h, an, vn, None, lab, None, torch.zeros(M, device=DEV), 0.0, 0.5)
    st = np_(stats)
    assert abs(st[0] - np.log(A)) < 1e-6 and st[4] == float((np_(lab) == 0).sum()) / M and st[5] == 1.0
    want = (1.0 / A - np.eye(A)[np_(lab)]).sum(0) / M
    np.testing.assert_allclose(np_(grads[1]), want, atol=1e-7)


def test_bc_loss_and_mix_refuse_invalid_arguments():
    from voxnav import _native
    lib = _native.load()
    M, F, A = 8, 64, 6
    f = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
    hp, hv, wa, ba, wv, bv, ret = f(M, F), f(M, F), f(A, F), f(A), f(F), f(1), f(M)
    lab = torch.zeros(M, dtype=torch.int32, device=DEV)
    dhp, dhv, gh = f(M, F) - 7, f(M, F), f(A * F + A + F + 1)
    stats = torch.zeros(6, dtype=torch.float64, device=DEV)
    part, spart = f(4096), torch.zeros(256, dtype=torch.float64, device=DEV)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def call(ptrs=None, M=M, F=F, A=A, ldh=F):
        a = dict(hp=hp, hv=hv, wa=wa, ba=ba, wv=wv, bv=bv, lab=lab, ret=ret, dhp=dhp, dhv=dhv, gh=gh, stats=stats,
                 part=part, spart=spart)
        a.update(ptrs or {})
        return lib.vn_bc_loss(p(a["hp"]), p(a["hv"]), ldh, p(a["wa"]), p(a["ba"]), p(a["wv"]), p(a["bv"]), None,
                              p(a["lab"]), None, p(a["ret"]), M, F, A, 0.0, 0.5, p(a["dhp"]), p(a["dhv"]), p(a["gh"]),
                              p(a["stats"]), p(a["part"]), p(a["spart"]), None)

    for name in ("hp", "hv", "wa", "ba", "wv", "bv", "lab", "ret", "dhp", "dhv", "gh", "stats", "part", "spart"):
        assert call({name: None}) == -1, name
        assert b"NULL" in lib.vn_last_error()
    for kw in (dict(M=0), dict(M=-3), dict(A=0), dict(A=9), dict(F=32), dict(F=320), dict(F=100), dict(ldh=F - 1)):
        assert call(**kw) == -1, kw
    n1, n2 = C.c_int64(), C.c_int64()
    for bad in ((0, F, A), (M, 0, A), (M, F, 0)):
        assert lib.vn_bc_loss_part_floats(*bad, C.byref(n1), C.byref(n2)) == -1
    i32 = lambda: torch.zeros(M, dtype=torch.int32, device=DEV)  # noqa: E731
    u8 = lambda: torch.zeros(M, dtype=torch.uint8, device=DEV)  # noqa: E731
    pol, exp, dist, out, took, w = i32(), i32(), i32(), i32() - 7, u8(), u8()

    def mix(ptrs=None, N=M, beta=0.5):
        a = dict(pol=pol, exp=exp, dist=dist, out=out, took=took, w=w)
        a.update(ptrs or {})
        return lib.vn_dagger_mix(p(a["pol"]), p(a["exp"]), p(a["dist"]), N, beta, 1, 0, 0, p(a["out"]), p(a["took"]),
                                 p(a["w"]), None)

    for name in ("pol", "exp", "dist", "out", "took", "w"):
        assert mix({name: None}) == -1, name
    for kw in (dict(N=0), dict(N=-1), dict(beta=-0.01), dict(beta=1.0001), dict(beta=float("nan"))):
        assert mix(**kw) == -1, kw
    assert b"beta" in lib.vn_last_error()
    torch.cuda.synchronize()
    assert float(dhp.max()) == -7.0 and int(out.max()) == -7             # nothing was launched
    assert call() == 0 and mix() == 0 and mix(beta=0.0) == 0 and mix(beta=1.0) == 0


# ------------------------------------------------------------------ 6. vn_dagger_mix
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_dagger_mix_matches_restatement(N):
    from voxnav import _native
    lib = _native.load()
    rng = np.random.default_rng(N)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for beta, seed, t, base in ((0.0, 4242, 0, 0), (1.0, 4242, 5, 0), (0.37, 0x1234567890ABCDEF, (1 << 33) + 5,
                                                                      (1 << 32) + 12345)):
        policy = rng.integers(0, 6, N).astype(np.int32)
        expert = ((policy + 1 + rng.integers(0, 5, N)) % 6).astype(np.int32)
        dist = rng.integers(1, 30, N).astype(np.int32)
        dist[rng.random(N) < 0.25] = -1
        dist[0] = -1 if N > 1 else dist[0]
        want = bh.mix(policy, expert, dist, beta, seed, base + np.arange(N), t)
        pol, exp, dst = (torch.as_tensor(a, device=DEV) for a in (policy, expert, dist))
        out = torch.full((N,), -7, dtype=torch.int32, device=DEV)
        took = torch.full((N,), 9, dtype=torch.uint8, device=DEV)
        w = torch.full((N,), 9, dtype=torch.uint8, device=DEV)
        _native.check(lib.vn_dagger_mix(p(pol), p(exp), p(dst), N, beta, seed, t, base, p(out), p(took), p(w), None))
        for name, got, ref in zip(("executed", "took_expert", "label_weight"), (out, took, w), want):
            np.testing.assert_array_equal(np_(got), ref, err_msg=f"{name} beta={beta}")
        assert (np_(pol) == policy).all()
        # executed aliased onto policy
        _native.check(lib.vn_dagger_mix(p(pol), p(exp), p(dst), N, beta, seed, t, base, p(pol), p(took), p(w), None))
        np.testing.assert_array_equal(np_(pol), want[0], err_msg=f"aliased beta={beta}")
        np.testing.assert_array_equal(np_(took), want[1])


# ------------------------------------------------------------------ 7. DaggerCollector
ROOMS = {"box8x8x4": "box:8x8x4", "box4x4x3": "ctor:4x4x3"}       # the second: max_steps 4, episodes end inside T
T_, N_, L_ = 12, 20, 4
SAMPLE_SEED, RESET_SEED, MIX_SEED = 1234, 42, 4242


def _policy(kind):
    return bh.small_policy(kind == "lstm").to(DEV)


def _dagger(src, kind, beta, N=N_, base=0, pol=None):
    from voxnav.env import BatchedGridEnv
    from voxnav.imitate import DaggerCollector
    env = BatchedGridEnv(num_agents=N, rooms=product_room_set(src), local_map_length=L_, device=DEV,
                         agent_id_base=base, seed_stride=N_)
    pol = _policy(kind) if pol is None else pol
    return env, DaggerCollector(env, pol, n_steps=T_, sample_seed=SAMPLE_SEED, reset_seed=RESET_SEED, beta=beta,
                                mix_seed=MIX_SEED)


def _replay(src, buf, N=N_, base=0):
    """The executed actions replayed through the CPU oracle, one step at a time: the planner's rule
    (route_helpers.plan) on the oracle's state before every step, and the env's outputs.
    -> dict(expert, dist [T], obs [T + 1], reward, terminated, truncated, bumped [T])."""
    seeds = RESET_SEED + base + np.arange(N)
    oenv, first = oracle_env(src, L_, n_agents=N), oracle_env(src, L_, n_agents=N)
    acts = np_(buf.actions)
    exp, dist = np.zeros((T_, N), np.int32), np.zeros((T_, N), np.int32)
    obs = np.zeros((T_ + 1, N, 80), np.float32)
    rew, te, tr = np.zeros((T_, N)), np.zeros((T_, N), bool), np.zeros((T_, N), bool)
    bumped = np.zeros((T_, N), bool)
    for i in range(N):
        obs[0, i] = first.reset(i, int(seeds[i]))
    for t in range(T_):
        st = first if t == 0 else oenv
        for i in range(N):
            s = st.state(i)
            exp[t, i], dist[t, i], _ = rh.plan(st.belief(i), (s["x"], s["y"], s["z"]), s["facing"])
        rr = oenv.run_random(seeds, 0, 1, t0=t, seed_stride=N_, initial_reset=(t == 0), actions=acts[t:t + 1],
                             terminal_obs=True, gid_base=base)
        obs[t + 1], rew[t] = rr["obs"][0], rr["reward"][0]
        te[t], tr[t] = rr["terminated"][0].astype(bool), rr["truncated"][0].astype(bool)
        # obs[70] is last_bump; an episode's last step shows it in the terminal observation only
        bumped[t] = np.where(te[t] | tr[t], rr["terminal_obs"][0][:, 70], obs[t + 1][:, 70]) > 0
    return dict(expert=exp, dist=dist, obs=obs, reward=rew, terminated=te, truncated=tr, bumped=bumped)


def _assert_labels_follow_the_oracle(src, buf, col, N=N_, base=0):
    """Labels, observations, rewards and flags of a rollout against the oracle's replay, bit for bit
    (rewards: but for the bootstrap added where an episode was truncated)."""
    rp = _replay(src, buf, N, base)
    done = rp["terminated"] | rp["truncated"]
    np.testing.assert_array_equal(np_(buf.expert_dist), rp["dist"])
    np.testing.assert_array_equal(np_(buf.expert_actions), rp["expert"])
    np.testing.assert_array_equal(np_(buf.label_weight), (rp["dist"] != -1).astype(np.uint8))
    assert np_(buf.obs).tobytes() == rp["obs"][:-1].tobytes(), "obs"
    assert np_(col._obs[T_]).tobytes() == rp["obs"][-1].tobytes()
    np.testing.assert_array_equal(np_(buf.episode_starts)[1:], done[:-1].astype(np.float32))
    np.testing.assert_array_equal(np_(buf.dones), done[-1].astype(np.float32))
    plain = ~(rp["truncated"] & ~rp["terminated"])
    assert np.array_equal(np_(buf.rewards)[plain], rp["reward"].astype(np.float32)[plain]), "rewards"
    rp["done"] = done
    return rp


@pytest.mark.parametrize("room", list(ROOMS))
@pytest.mark.parametrize("kind", ["mlp", "lstm"])
def test_dagger_collector_beta0_is_the_plain_collector(kind, room):
    from voxnav.collector import RolloutBuffer, RolloutCollector
    from voxnav.env import BatchedGridEnv
    src = ROOMS[room]
    env, col = _dagger(src, kind, 0.0)
    env2 = BatchedGridEnv(num_agents=N_, rooms=product_room_set(src), local_map_length=L_, device=DEV, seed_stride=N_)
    plain = RolloutCollector(env2, _policy(kind), n_steps=T_, sample_seed=SAMPLE_SEED, reset_seed=RESET_SEED)
    for r in range(2):                                             # the second rollout: the carried state
        buf, ref = col.collect(), plain.collect()
        for name in RolloutBuffer.__dataclass_fields__:
            a, b = getattr(buf, name), getattr(ref, name)
            assert (a is None) == (b is None), name
            if a is not None:
                assert torch.equal(a, b), name
        assert torch.equal(buf.actions, buf.policy_actions) and int(buf.took_expert.sum()) == 0
        if r == 0:
            rp = _assert_labels_follow_the_oracle(src, buf, col)
            if room == "box4x4x3":
                assert rp["done"].any()                            # episodes ended and restarted inside the rollout
    env.close()
    env2.close()


@pytest.mark.parametrize("room", list(ROOMS))
@pytest.mark.parametrize("kind", ["mlp", "lstm"])
def test_dagger_collector_beta1_executes_the_planner(kind, room):
    src = ROOMS[room]
    env, col = _dagger(src, kind, 1.0)
    buf = col.collect()
    lw = np_(buf.label_weight).astype(bool)
    assert lw.mean() > 0.5
    assert (np_(buf.actions)[lw] == np_(buf.expert_actions)[lw]).all()
    assert (np_(buf.actions)[~lw] == np_(buf.policy_actions)[~lw]).all()
    np.testing.assert_array_equal(np_(buf.took_expert), np_(buf.label_weight))
    rp = _assert_labels_follow_the_oracle(src, buf, col)
    rec = np_(env.episode_records())
    led = lw.all(axis=0)                                           # agents the planner led at every step
    assert led.any()
    assert (rec[led, 3] == 0).all() and (rec[led, 7] == 0).all()   # sum_bumps, last_bumps of their episodes
    assert not rp["bumped"][:, led].any()
    st = np_(env.export_state())
    assert (st[led, 7] == 0).all()                                 # the running episode's bump count
    if room == "box4x4x3":
        assert rec[:, 0].sum() > 0 and rp["done"].any()
    env.close()


@pytest.mark.parametrize("room", list(ROOMS))
@pytest.mark.parametrize("kind", ["mlp", "lstm"])
def test_dagger_collector_beta_half_follows_the_draw(kind, room):
    src = ROOMS[room]
    env, col = _dagger(src, kind, 0.5)
    buf = col.collect()
    pa, ea, ed = np_(buf.policy_actions), np_(buf.expert_actions), np_(buf.expert_dist)
    took = np_(buf.took_expert)
    for t in range(T_):
        ex, tk, w = bh.mix(pa[t], ea[t], ed[t], 0.5, MIX_SEED, np.arange(N_), t)
        np.testing.assert_array_equal(took[t], tk, err_msg=f"step {t}")
        np.testing.assert_array_equal(np_(buf.actions)[t], ex)
        np.testing.assert_array_equal(np_(buf.label_weight)[t], w)
    assert 0 < took.sum() < np_(buf.label_weight).sum()
    _assert_labels_follow_the_oracle(src, buf, col)
    # two shards of 10 agents reproduce the unsharded run
    for base in (0, 10):
        senv, scol = _dagger(src, kind, 0.5, N=10, base=base)
        sbuf = scol.collect()
        np.testing.assert_array_equal(np_(sbuf.took_expert), took[:, base:base + 10], err_msg=f"shard {base}")
        np.testing.assert_array_equal(np_(sbuf.actions), np_(buf.actions)[:, base:base + 10])
        senv.close()
    # set_beta takes effect in the next rollout
    col.set_beta(0.0)
    assert int(col.collect().took_expert.sum()) == 0
    with pytest.raises(ValueError):
        col.set_beta(1.5)
    env.close()


def test_dagger_collector_refuses_what_the_planner_cannot_take():
    from voxnav.env import BatchedGridEnv
    from voxnav.imitate import DaggerCollector
    simple = BatchedGridEnv(num_agents=8, rooms=product_room_set("box:8x8x4"), local_map_length=4, device=DEV,
                            variant="simple")
    with pytest.raises(ValueError, match="CubicEnv"):
        DaggerCollector(simple, _policy("mlp"), n_steps=4)
    simple.close()
    wide = BatchedGridEnv(num_agents=8, rooms=product_room_set("box:100x40x8"), local_map_length=4, device=DEV)
    with pytest.raises(ValueError, match="64"):
        DaggerCollector(wide, _policy("mlp"), n_steps=4)
    wide.close()
    env = BatchedGridEnv(num_agents=8, rooms=product_room_set("box:8x8x4"), local_map_length=4, device=DEV)
    with pytest.raises(ValueError, match="beta"):
        DaggerCollector(env, _policy("mlp"), n_steps=4, beta=-0.1)
    env.close()


# ------------------------------------------------------------------ 8. BCLearner
@pytest.mark.parametrize("recurrent", [True, False], ids=["lstm", "mlp"])
def test_bc_learner_matches_restatement_gpu(recurrent):
    """tests/test_ppo.py's small shapes with a latent width of 64: every minibatch goes through the
    fused kernel.  Bounds as on the CPU (tests/test_imitate_cpu.py)."""
    ln, ost = bh.run_bc_parity(DEV, recurrent, arch=(32, 64))
    assert ln.fused_updates == len(ost) > 0


def test_bc_learner_whole_rollout_takes_the_row_layout_lstm():
    """One minibatch = the whole rollout (T = 16, N = 8), LSTM 256 (the width the row-layout
    kernels take), MLP [64]: the LSTMs re-run in the row layout, the loss in the fused kernel."""
    ln, ost = bh.run_bc_parity(DEV, True, T=16, N=8, batch_size=128, epochs=1, arch=(64,), lstm=256, p_start=0.05)
    assert ln.fused_updates == len(ost) == 1
    assert any(ln.__dict__.get("_rows_cache", {}).values()), "the row layout must be the path under test"


# ------------------------------------------------------------------ 9. warm_start
def test_warm_start_end_to_end(tmp_path):
    """8x8x4 box, 64 agents x 32 steps, an MLP policy [64, 64], five iterations of one epoch with beta
    = 1, 0.8, 0.6, 0.4, 0.2.  Observed bc_loss per iteration: 1.732, 1.586, 1.397, 1.373, 1.289 (ln 6 =
    1.792 untrained), accuracy 0.611, 0.613, 0.652, 0.492, 0.517: each rollout's loss is measured on
    that rollout's states, which move from the planner's to the policy's own as beta falls, where
    the planner's actions are more varied -- the loss still falls, the accuracy does not.  The
    asserted margin is a third of the observed drop."""
    from voxnav.checkpoint import load_checkpoint, save_checkpoint
    from voxnav.collector import RolloutCollector
    from voxnav.env import BatchedGridEnv
    from voxnav.imitate import BCLearner, DaggerCollector, warm_start
    from voxnav.ppo import PPOLearner, learn
    N, T, iters = 64, 32, 5
    rooms = product_room_set("box:8x8x4")
    pol = bh.small_policy(False, arch=(64, 64), seed=2).to(DEV)
    env = BatchedGridEnv(num_agents=N, rooms=rooms, local_map_length=4, device=DEV)
    col = DaggerCollector(env, pol, n_steps=T)
    ln = BCLearner(pol, learning_rate=1e-3, n_epochs=1, batch_size=256, seed=1)
    seen = []
    hist = warm_start(col, ln, total_timesteps=iters * N * T, beta=lambda i: 1 - 0.2 * i,
                      callback=lambda it, done, st: seen.append((it, done)))
    assert len(hist) == iters and seen == [(i + 1, (i + 1) * N * T) for i in range(iters)]
    keys = {"bc_loss", "value_loss", "entropy_loss", "loss", "accuracy", "labelled", "grad_norm", "n_minibatches",
            "n_updates", "beta", "num_timesteps", "expert_share"}
    for i, h in enumerate(hist):
        assert keys <= set(h), keys - set(h)
        assert h["beta"] == 1 - 0.2 * i and h["num_timesteps"] == (i + 1) * N * T and h["n_minibatches"] == 8
        assert all(np.isfinite(h[k]) for k in keys)
        assert 0.0 <= h["expert_share"] <= h["labelled"] + 1e-6 <= 1.0 + 1e-6
    print([(round(h["bc_loss"], 3), round(h["accuracy"], 3), round(h["expert_share"], 3)) for h in hist])
    assert abs(hist[0]["expert_share"] - hist[0]["labelled"]) < 1e-6      # beta = 1: every labelled step is the planner's
    assert hist[-1]["expert_share"] < hist[0]["expert_share"]
    assert ln.fused_updates == iters * 8
    assert hist[-1]["bc_loss"] < hist[0]["bc_loss"] - 0.15
    # the Monitor / exploration keys ppo.learn reports appear once episodes have ended
    assert any("ep_rew_mean" in h and "ep_finished_rate" in h for h in hist)
    path = save_checkpoint(tmp_path / "warm.zip", pol, ln.optimizer, num_timesteps=hist[-1]["num_timesteps"])
    pol2, data = load_checkpoint(path, device=DEV)
    assert data["num_timesteps"] == iters * N * T
    for a, b in zip(pol.parameters(), pol2.parameters()):
        assert torch.equal(a, b)
    env.close()
    # the same module goes on under PPO
    env2 = BatchedGridEnv(num_agents=N, rooms=rooms, local_map_length=4, device=DEV)
    w0 = torch.cat([p.detach().reshape(-1).clone() for p in pol.parameters()])
    ph = learn(RolloutCollector(env2, pol, n_steps=T), PPOLearner(pol, n_epochs=2, batch_size=256, seed=1),
               total_timesteps=N * T)
    assert len(ph) == 1 and np.isfinite(ph[0]["loss"])
    assert float((torch.cat([p.detach().reshape(-1) for p in pol.parameters()]) - w0).abs().max()) > 1e-5
    env2.close()
