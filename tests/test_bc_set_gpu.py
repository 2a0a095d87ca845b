"""The set-valued DAgger warm start on the GPU: vn_bc_loss_set against the float64 restatement
(tests/bc_set_helpers.py), DaggerCollector(labels="set") against the action-mode collector and the
CPU oracle's replay, BCLearner(labels="set") against the restatement, and a short warm start.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bc_helpers as bh  # noqa: E402
import bc_set_helpers as bs  # noqa: E402
import route_dists_helpers as rd  # noqa: E402
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


# ------------------------------------------------------------------ 1. vn_bc_loss_set
# tests/test_imitate_gpu.py's edges: the 4-sample pass, the 128-sample block, more than 64 count
# blocks' worth of blocks
BC_M = [1, 3, 4, 5, 127, 128, 129, 4099]
# (gather through src, weights, ent_coef, vf_coef)
BC_MODES = [(False, None, 0.01, 0.5), (True, "random", 0.0, 0.5), (True, "zero", 0.01, 0.5),
            (False, "random", 0.01, 0.0), (True, None, 0.0, 0.5), (False, "zero", 0.0, 0.5)]


def _bc_loss_set_against_float64(M, F, A, modes):
    from voxnav.learn_ops import bc_loss_set
    torch.manual_seed(1000 * M + F + A)
    rng = np.random.default_rng(1000 * M + F + A)
    an, vn = torch.nn.Linear(F, A).to(DEV), torch.nn.Linear(F, 1).to(DEV)
    h = torch.tanh(torch.randn((2, M, F), device=DEV))
    for gather, wmode, ent, vf in modes:
        R = M + 1000 if gather else M
        src = torch.randperm(R, device=DEV)[:M].contiguous() if gather else None
        sets = torch.as_tensor(bs.random_sets(rng, (R,), A), device=DEV)
        ret = torch.randn(R, device=DEV)
        wgt = None if wmode is None else (torch.rand(R, device=DEV) < 0.7).to(torch.uint8) if wmode == "random" \
            else torch.zeros(R, dtype=torch.uint8, device=DEV)
        if wmode == "zero" and gather:
            wgt[torch.randperm(R, device=DEV)[M:]] = 1           # rows outside the minibatch do not count
            wgt[src] = 0
        dh, grads, stats = bc_loss_set(h, an, vn, src, sets, wgt, ret, ent, vf)
        dh2, grads2, stats2 = bc_loss_set(h, an, vn, src, sets, wgt, ret, ent, vf)
        assert torch.equal(dh, dh2) and torch.equal(stats, stats2)
        assert all(torch.equal(a, b) for a, b in zip(grads, grads2))
        g = lambda t: None if t is None else np_(t if src is None else t[src])  # noqa: E731
        rp, rv, rg, rstats = bs.bc_set_heads64(np_(h[0]), np_(h[1]), np_(an.weight), np_(an.bias), np_(vn.weight),
                                               np_(vn.bias), g(sets), g(wgt), g(ret), ent, vf)
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
def test_bc_loss_set_matches_float64(M, F, A):
    """Tolerances of tests/test_imitate_gpu.py::test_bc_loss_matches_float64: latent gradients 2e-5,
    head gradients 1e-4, logged sums 1e-5 relative; accuracy and labelled share exact.  Two calls
    on the same inputs give the same bits.  Sets: 30 % empty, 25 % singletons, random bits at or
    above A."""
    _bc_loss_set_against_float64(M, F, A, BC_MODES)


# every instantiation of the loss kernel at one full block plus one sample
# (tests/test_imitate_gpu.py::test_bc_loss_grid_matches_float64, on label sets)
GRID_MODES = {"src+weights": (True, "random", 0.01, 0.5), "plain": (False, None, 0.01, 0.5)}


@pytest.mark.parametrize("mode", list(GRID_MODES))
@pytest.mark.parametrize("A", range(1, 9))
@pytest.mark.parametrize("F", [64, 128, 192, 256])
def test_bc_loss_set_grid_matches_float64(F, A, mode):
    """test_bc_loss_set_matches_float64's checks and tolerances on all 32 (F, A) pairs at M = 129."""
    _bc_loss_set_against_float64(129, F, A, [GRID_MODES[mode]])


def test_random_sets_hold_what_the_test_is_for():
    s = bs.random_sets(np.random.default_rng(0), (4099,), 6) & 63
    size = np.array([bin(int(v)).count("1") for v in s])
    assert 0.25 < (size == 0).mean() < 0.36 and (size == 1).mean() >= 0.2 and (size >= 3).any()


@pytest.mark.parametrize("M,F,A", [(129, 64, 6), (4099, 256, 8), (5, 64, 1)])
def test_singleton_sets_agree_with_bc_loss(M, F, A):
    """With one member per set the outputs agree with vn_bc_loss on the corresponding labels within
    the bounds both are held to against float64; accuracy and labelled share are equal."""
    from voxnav.learn_ops import bc_loss, bc_loss_set
    torch.manual_seed(M + F + A)
    an, vn = torch.nn.Linear(F, A).to(DEV), torch.nn.Linear(F, 1).to(DEV)
    h = torch.tanh(torch.randn((2, M, F), device=DEV))
    lab = torch.randint(0, A, (M,), device=DEV, dtype=torch.int32)
    sets = (1 << lab).to(torch.uint8)
    ret = torch.randn(M, device=DEV)
    for wgt in (None, (torch.rand(M, device=DEV) < 0.7).to(torch.uint8)):
        dh, grads, stats = bc_loss(h, an, vn, None, lab, wgt, ret, 0.01, 0.5)
        dh2, grads2, stats2 = bc_loss_set(h, an, vn, None, sets, wgt, ret, 0.01, 0.5)
        _close(np_(dh2).astype(np.float64), np_(dh).astype(np.float64), 2e-5, 1e-9, "dh")
        for a, b in zip(grads2, grads):
            _close(np_(a).astype(np.float64).reshape(-1), np_(b).astype(np.float64).reshape(-1), 1e-4, 1e-9, "heads")
        _close(np_(stats2)[:4], np_(stats)[:4], 1e-5, 1e-7, "stats")
        assert torch.equal(stats2[4:], stats[4:])


def test_full_sets_and_ties():
    """Zero head weights: every logit ties, the argmax is action 0, ce = ln(A / |S|); the full set
    gives a cross-entropy of exactly 0 and an action gradient of 0 up to f32 rounding."""
    from voxnav.learn_ops import bc_loss_set
    M, F, A = 37, 64, 6
    an, vn = torch.nn.Linear(F, A).to(DEV), torch.nn.Linear(F, 1).to(DEV)
    h = torch.tanh(torch.randn((2, M, F), device=DEV))
    ret = torch.zeros(M, device=DEV)
    full = torch.full((M,), 63 + 128, dtype=torch.uint8, device=DEV)
    dh, grads, stats = bc_loss_set(h, an, vn, None, full, None, ret, 0.0, 0.0)
    assert float(stats[0]) == 0.0 and float(stats[4]) == 1.0 and float(stats[5]) == 1.0
    # p - q = 0 but for f32 rounding: p and q are two exponentials of at most 1, a few ulp (2^-24) apart,
    # so |dz| <= 4 * 2^-24 / M per logit; d ba sums M of them, a latent gradient A of them times a
    # weight below 1 / sqrt(F), a weight gradient M of them times a latent below 1
    ulp = 4 * 2.0 ** -24
    assert float(grads[1].abs().max()) <= ulp and float(grads[0].abs().max()) <= ulp
    assert float(dh[0].abs().max()) <= A * ulp / M / np.sqrt(F)
    with torch.no_grad():
        an.weight.zero_()
        an.bias.zero_()
    sets = (torch.arange(M, device=DEV) % 63 + 1).to(torch.uint8)
    _, grads, stats = bc_loss_set(h, an, vn, None, sets, None, ret, 0.0, 0.5)
    s = np_(sets)
    size = np.array([bin(int(v)).count("1") for v in s])
    st = np_(stats)
    assert abs(st[0] - np.mean(np.log(A / size))) < 1e-6 and st[4] == float((s & 1).sum()) / M and st[5] == 1.0
    S = bs.members(s, A).numpy().astype(np.float64)
    np.testing.assert_allclose(np_(grads[1]), (1.0 / A - S / size[:, None]).sum(0) / M, atol=1e-7)


def test_bc_loss_set_refuses_invalid_arguments():
    from voxnav import _native
    lib = _native.load()
    M, F, A = 8, 64, 6
    f = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
    hp, hv, wa, ba, wv, bv, ret = f(M, F), f(M, F), f(A, F), f(A), f(F), f(1), f(M)
    sets = torch.ones(M, dtype=torch.uint8, device=DEV)
    dhp, dhv, gh = f(M, F) - 7, f(M, F), f(A * F + A + F + 1)
    stats = torch.zeros(6, dtype=torch.float64, device=DEV)
    part, spart = f(4096), torch.zeros(256, dtype=torch.float64, device=DEV)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731

    def call(ptrs=None, M=M, F=F, A=A, ldh=F):
        a = dict(hp=hp, hv=hv, wa=wa, ba=ba, wv=wv, bv=bv, sets=sets, ret=ret, dhp=dhp, dhv=dhv, gh=gh, stats=stats,
                 part=part, spart=spart)
        a.update(ptrs or {})
        return lib.vn_bc_loss_set(p(a["hp"]), p(a["hv"]), ldh, p(a["wa"]), p(a["ba"]), p(a["wv"]), p(a["bv"]), None,
                                  p(a["sets"]), None, p(a["ret"]), M, F, A, 0.0, 0.5, p(a["dhp"]), p(a["dhv"]),
                                  p(a["gh"]), p(a["stats"]), p(a["part"]), p(a["spart"]), None)

    for name in ("hp", "hv", "wa", "ba", "wv", "bv", "sets", "ret", "dhp", "dhv", "gh", "stats", "part", "spart"):
        assert call({name: None}) == -1, name
        assert b"NULL" in lib.vn_last_error()
    for kw in (dict(M=0), dict(M=-3), dict(A=0), dict(A=9), dict(F=32), dict(F=320), dict(F=100), dict(ldh=F - 1)):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert float(dhp.max()) == -7.0                                      # nothing was launched
    assert call() == 0


# ------------------------------------------------------------------ 2. DaggerCollector(labels="set")
ROOMS = {"box8x8x4": "box:8x8x4", "box4x4x3": "ctor:4x4x3"}       # the second: max_steps 4, episodes end inside T
T_, N_, L_ = 12, 20, 4
SAMPLE_SEED, RESET_SEED, MIX_SEED = 1234, 42, 4242


def _dagger(src, kind, beta, labels):
    from voxnav.env import BatchedGridEnv
    from voxnav.imitate import DaggerCollector
    env = BatchedGridEnv(num_agents=N_, rooms=product_room_set(src), local_map_length=L_, device=DEV, seed_stride=N_)
    pol = bh.small_policy(kind == "lstm").to(DEV)
    return env, DaggerCollector(env, pol, n_steps=T_, sample_seed=SAMPLE_SEED, reset_seed=RESET_SEED, beta=beta,
                                mix_seed=MIX_SEED, labels=labels)


def _replay_dists(src, actions):
    """The executed actions replayed through the CPU oracle, the per-action rule on the oracle's
    state before every step -> (dists [T, N, 6], best [T, N], whether an episode ended)."""
    seeds = RESET_SEED + np.arange(N_)
    oenv, first = oracle_env(src, L_, n_agents=N_), oracle_env(src, L_, n_agents=N_)
    dists, best = np.zeros((T_, N_, 6), np.int32), np.zeros((T_, N_), np.uint8)
    ended = False
    for i in range(N_):
        first.reset(i, int(seeds[i]))
    for t in range(T_):
        st = first if t == 0 else oenv
        for i in range(N_):
            s = st.state(i)
            dists[t, i], best[t, i], _ = rd.plan_dists(st.belief(i), (s["x"], s["y"], s["z"]), s["facing"])
        rr = oenv.run_random(seeds, 0, 1, t0=t, seed_stride=N_, initial_reset=(t == 0), actions=actions[t:t + 1],
                             terminal_obs=True, gid_base=0)
        ended = ended or bool(rr["terminated"][0].any() or rr["truncated"][0].any())
    return dists, best, ended


@pytest.mark.parametrize("room", list(ROOMS))
@pytest.mark.parametrize("beta", [0.0, 1.0, 0.5])
@pytest.mark.parametrize("kind", ["mlp", "lstm"])
def test_set_collector_is_the_action_collector_plus_the_sets(kind, beta, room):
    from voxnav.collector import RolloutBuffer
    src = ROOMS[room]
    env, col = _dagger(src, kind, beta, "set")
    env2, ref_col = _dagger(src, kind, beta, "action")
    for r in range(2):                                             # the second rollout: the carried state
        buf, ref = col.collect(), ref_col.collect()
        assert ref.expert_dists is None and ref.expert_set is None
        for name in list(RolloutBuffer.__dataclass_fields__) + ["expert_actions", "expert_dist", "took_expert",
                                                                "label_weight", "policy_actions"]:
            a, b = getattr(buf, name), getattr(ref, name)
            assert (a is None) == (b is None), name
            if a is not None:
                assert torch.equal(a, b), name
        assert buf.expert_dists.shape == (T_, N_, 6) and buf.expert_set.dtype == torch.uint8
        # the set is empty exactly where the sample is unlabelled, and holds the planner's action
        es, ea, lw = np_(buf.expert_set), np_(buf.expert_actions), np_(buf.label_weight)
        assert ((es != 0) == (lw != 0)).all()
        assert (((es >> ea) & 1) == 1)[lw != 0].all() and ((es & -es.astype(np.int32)) == (1 << ea))[lw != 0].all()
        if r == 0:
            dists, best, ended = _replay_dists(src, np_(buf.actions))
            np.testing.assert_array_equal(np_(buf.expert_dists), dists)
            np.testing.assert_array_equal(es, best)
            assert (rd.popcount(best) > 1).any()
            if room == "box4x4x3":
                assert ended                                       # episodes ended and restarted inside the rollout
    env.close()
    env2.close()


def test_collector_refuses_an_unknown_label_mode():
    from voxnav.env import BatchedGridEnv
    from voxnav.imitate import DaggerCollector
    env = BatchedGridEnv(num_agents=8, rooms=product_room_set("box:8x8x4"), local_map_length=4, device=DEV)
    with pytest.raises(ValueError, match="labels"):
        DaggerCollector(env, bh.small_policy(False).to(DEV), n_steps=4, labels="both")
    env.close()


# ------------------------------------------------------------------ 3. BCLearner(labels="set")
@pytest.mark.parametrize("recurrent", [True, False], ids=["lstm", "mlp"])
def test_bc_set_learner_matches_restatement_gpu(recurrent):
    """tests/test_imitate_gpu.py's shapes (a latent width of 64: every minibatch goes through the
    fused kernel) and the CPU bounds."""
    ln, ost = bs.run_bc_set_parity(DEV, recurrent, arch=(32, 64))
    assert ln.fused_updates == len(ost) > 0


def test_bc_set_learner_whole_rollout_takes_the_row_layout_lstm():
    ln, ost = bs.run_bc_set_parity(DEV, True, T=16, N=8, batch_size=128, epochs=1, arch=(64,), lstm=256, p_start=0.05)
    assert ln.fused_updates == len(ost) == 1
    assert any(ln.__dict__.get("_rows_cache", {}).values()), "the row layout must be the path under test"


# ------------------------------------------------------------------ 4. warm_start
def test_warm_start_in_set_mode_end_to_end(tmp_path):
    """8x8x4 box, 64 agents x 32 steps, an MLP policy [64, 64], three iterations of one epoch with
    beta = 1, 0.5, 0 in set mode, a checkpoint round trip, then one ppo.learn iteration on the same
    module.  The untrained policy's set cross-entropy is at most ln 6 (a singleton) and the loss
    must be finite and the accuracy a share; what the loss does over three iterations is printed,
    not asserted."""
    from voxnav.checkpoint import load_checkpoint, save_checkpoint
    from voxnav.collector import RolloutCollector
    from voxnav.env import BatchedGridEnv
    from voxnav.imitate import BCLearner, DaggerCollector, warm_start
    from voxnav.ppo import PPOLearner, learn
    N, T, iters = 64, 32, 3
    rooms = product_room_set("box:8x8x4")
    pol = bh.small_policy(False, arch=(64, 64), seed=2).to(DEV)
    env = BatchedGridEnv(num_agents=N, rooms=rooms, local_map_length=4, device=DEV)
    col = DaggerCollector(env, pol, n_steps=T, labels="set")
    ln = BCLearner(pol, learning_rate=1e-3, n_epochs=1, batch_size=256, seed=1, labels="set")
    hist = warm_start(col, ln, total_timesteps=iters * N * T, beta=lambda i: 1 - 0.5 * i)
    assert len(hist) == iters and ln.fused_updates == iters * 8
    print([(round(h["bc_loss"], 3), round(h["accuracy"], 3), round(h["labelled"], 3)) for h in hist])
    for h in hist:
        assert np.isfinite(h["loss"]) and 0.0 <= h["bc_loss"] <= np.log(6) + 0.5 and 0.0 <= h["accuracy"] <= 1.0
        assert 0.5 < h["labelled"] <= 1.0
    path = save_checkpoint(tmp_path / "warm_set.zip", pol, ln.optimizer, num_timesteps=hist[-1]["num_timesteps"])
    pol2, data = load_checkpoint(path, device=DEV)
    assert data["num_timesteps"] == iters * N * T
    for a, b in zip(pol.parameters(), pol2.parameters()):
        assert torch.equal(a, b)
    env.close()
    env2 = BatchedGridEnv(num_agents=N, rooms=rooms, local_map_length=4, device=DEV)
    w0 = torch.cat([p.detach().reshape(-1).clone() for p in pol.parameters()])
    ph = learn(RolloutCollector(env2, pol, n_steps=T), PPOLearner(pol, n_epochs=2, batch_size=256, seed=1),
               total_timesteps=N * T)
    assert len(ph) == 1 and np.isfinite(ph[0]["loss"])
    assert float((torch.cat([p.detach().reshape(-1) for p in pol.parameters()]) - w0).abs().max()) > 1e-5
    env2.close()
