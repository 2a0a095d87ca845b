"""The distance-weighted behaviour-cloning target and best-set execution off the GPU
(include/voxnav.h vn_bc_loss_soft, vn_dagger_mix_best): hand-derived answers of the float64
restatement (tests/bc_soft_helpers.py), ``BCLearner`` / ``KickstartLearner(labels="soft")``'s torch
path against it, the ``label_tau`` schedule, and every refusal on the Python side.
"""
import math
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bc_helpers as bh  # noqa: E402
import bc_soft_helpers as so  # noqa: E402

F64 = torch.float64
ROW = [3, 3, 4, 5, -1, -2]


def _q_of_row(tau=1.0):
    w = np.array([1.0, 1.0, math.exp(-1 / tau), math.exp(-2 / tau), 0.0, 0.0])
    return w / w.sum()


# ------------------------------------------------------------------ 1. the rule, by hand
def test_zero_logits_give_ln_A_minus_entropy_of_q():
    """Zero logits, A = 6, dists = [3, 3, 4, 5, -1, -2], tau = 1: q = [1, 1, 1/e, 1/e^2, 0, 0] / Z,
    kl = sum q (ln q + ln 6) = ln 6 - H(q), dz = (1/6 - q) / n; the argmax is index 0, a shortest one."""
    M, A = 5, 6
    dists = np.tile(np.array(ROW, np.int32), (M, 1))
    logits = torch.zeros((M, A), dtype=F64, requires_grad=True)
    z = torch.zeros(M, dtype=F64)
    r = so.bc_soft_terms(logits, z, dists, None, z, 1.0, 0.0, 0.5)
    q = _q_of_row()
    Hq = -(q[:4] * np.log(q[:4])).sum()
    assert abs(float(r["bc_loss"].detach()) - (math.log(6) - Hq)) < 1e-14
    dz, = torch.autograd.grad(r["loss"], [logits])
    assert float((dz - torch.as_tensor((1 / 6 - q) / M)).abs().max()) < 1e-16
    assert float(r["accuracy"]) == 1.0 and float(r["labelled"]) == 1.0
    P, qq, ln_q, short = so.soft_target(dists, A, 1.0)
    assert P[0].tolist() == [True] * 4 + [False] * 2 and short[0].tolist() == [True, True] + [False] * 4
    np.testing.assert_allclose(qq[0].numpy(), q, rtol=0, atol=1e-16)
    assert ln_q[0, 4:].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("weighted", [False, True], ids=["all", "weights"])
def test_singletons_are_the_label_cross_entropy(weighted):
    M, A = 11, 6
    rng = np.random.default_rng(3)
    labels = rng.integers(0, A, M)
    dists = np.where(np.arange(A) == labels[:, None], rng.integers(1, 2000, (M, 1)), -2).astype(np.int32)
    dists[::2] = np.where(dists[::2] == -2, -1, dists[::2])
    weight = (rng.random(M) < 0.7).astype(np.uint8) if weighted else None
    ret = torch.tensor(rng.normal(size=M))
    out = []
    for soft in (False, True):
        logits = torch.tensor(np.random.default_rng(4).normal(size=(M, A)), requires_grad=True)
        values = torch.tensor(np.random.default_rng(5).normal(size=M), requires_grad=True)
        r = (so.bc_soft_terms(logits, values, dists, weight, ret, 0.3, 0.01, 0.5) if soft
             else bh.bc_terms(logits, values, torch.as_tensor(labels), weight, ret, 0.01, 0.5))
        out.append(([float(r[k].detach()) for k in bh.STAT_KEYS], torch.autograd.grad(r["loss"], [logits, values])))
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=0, atol=1e-14)
    for x, y in zip(out[0][1], out[1][1]):
        assert float((x - y).abs().max()) < 1e-15


@pytest.mark.parametrize("tau,on", [(1e-30, "best"), (1e30, "P")])
def test_extreme_temperatures_are_uniform_targets_without_nan(tau, on):
    """tau = 1e-30: delta / tau overflows and w = 0, the target is uniform on the shortest actions;
    tau = 1e30: every w is 1, the target is uniform on the reached, passable actions."""
    M, A = 64, 6
    dists = so.random_dists(np.random.default_rng(0), M, A)
    P, q, ln_q, short = so.soft_target(dists, A, so.f32(tau))
    S = (short if on == "best" else P).double()
    want = S / torch.clamp(S.sum(-1, keepdim=True), min=1.0)
    assert float((q - want).abs().max()) < 1e-15 and bool(torch.isfinite(ln_q).all())
    logits = torch.tensor(np.random.default_rng(1).normal(size=(M, A)), requires_grad=True)
    z = torch.zeros(M, dtype=F64)
    r = so.bc_soft_terms(logits, z, dists, None, z, so.f32(tau), 0.0, 0.0)
    dz, = torch.autograd.grad(r["loss"], [logits])
    assert math.isfinite(float(r["bc_loss"].detach())) and bool(torch.isfinite(dz).all())
    n = float(P.any(-1).sum())
    lab = P.any(-1, keepdim=True).double()
    assert float((dz - lab * (torch.softmax(logits.detach(), -1) - want) / n).abs().max()) < 1e-15


def test_rows_without_a_positive_distance_are_unlabelled_with_exact_zeros():
    M, A = 9, 6
    rng = np.random.default_rng(1)
    dists = np.array([-1, -2, 0], np.int32)[rng.integers(0, 3, (M, A))]
    logits = torch.tensor(rng.normal(size=(M, A)), requires_grad=True)
    values = torch.tensor(rng.normal(size=M), requires_grad=True)
    ret = torch.tensor(rng.normal(size=M))
    r = so.bc_soft_terms(logits, values, dists, None, ret, 1.0, 0.0, 0.5)
    assert float(r["bc_loss"].detach()) == 0.0 and float(r["accuracy"]) == 0.0 and float(r["labelled"]) == 0.0
    dz, dv = torch.autograd.grad(r["loss"], [logits, values])
    assert float(dz.abs().max()) == 0.0
    assert float((dv - 2 * 0.5 * (values - ret).detach() / M).abs().max()) < 1e-15
    # one such row among labelled ones behaves as a zero weight
    d2 = so.random_dists(rng, M, A, p_none=0.0)[:, :A]
    drop = np.arange(M) % 3 == 0
    out = []
    for d, w in ((np.where(drop[:, None], -1, d2), None), (d2, (~drop).astype(np.uint8))):
        lg = torch.tensor(np.random.default_rng(4).normal(size=(M, A)), requires_grad=True)
        r = so.bc_soft_terms(lg, values.detach(), d, w, ret, 0.5, 0.0, 0.5)
        out.append(([float(r[k].detach()) for k in bh.STAT_KEYS], torch.autograd.grad(r["loss"], [lg])[0]))
    assert out[0][0] == out[1][0] and torch.equal(out[0][1], out[1][1])


def test_masked_target_keeps_its_support_and_zeroes_the_rest():
    """A mask that excludes a positive-distance action: the action stays in S_i (it has target mass);
    a masked action without a positive distance gets a gradient of exactly 0."""
    M, A = 4, 6
    dists = np.tile(np.array(ROW, np.int32), (M, 1))
    masks = np.full(M, 0b000001, np.uint8)               # only action 0 allowed: 1, 2, 3 come in through P
    logits = torch.tensor(np.random.default_rng(2).normal(size=(M, A)), requires_grad=True)
    z = torch.zeros(M, dtype=F64)
    r = so.bc_soft_terms(logits, z, dists, None, z, 1.0, 0.01, 0.0, masks=masks)
    dz, = torch.autograd.grad(r["loss"], [logits])
    assert float(dz[:, 4:].abs().max()) == 0.0 and float(dz[:, :4].abs().min()) > 0.0
    p = torch.softmax(logits.detach()[:, :4], -1)
    kl = (torch.as_tensor(_q_of_row()[:4]) * (torch.log(torch.as_tensor(_q_of_row()[:4])) - torch.log(p))).sum(-1)
    assert abs(float(r["bc_loss"].detach()) - float(kl.mean())) < 1e-14


def test_random_dists_hold_what_the_tests_are_for():
    A = 6
    d = so.random_dists(np.random.default_rng(0), 4099, A)
    assert d.shape == (4099, A + 2) and (d[:, A:] == so.PAD).all()          # ldd > A, poisoned padding
    body = d[:, :A]
    pos = (body > 0).sum(1)
    assert 0.25 < (pos == 0).mean() < 0.36 and 0.2 <= (pos == 1).mean() < 0.32
    multi = body[pos >= 2].astype(np.int64)
    dstar = np.where(multi > 0, multi, 1 << 40).min(1, keepdims=True)
    delta = np.where(multi > 0, multi - dstar, -1)
    assert dstar.max() > 1500 and dstar.min() < 100
    for v in (0, 1, 2):
        assert (delta == v).any()
    assert ((delta == 0).sum(1) >= 2).mean() > 0.2                          # ties among the shortest
    assert 0 < (delta == 100).any(1).sum() < 0.1 * 4099                      # a few rows with a spread of 100
    assert (body == -1).any() and (body == -2).any() and (body == 0).any()


# ------------------------------------------------------------------ 2. the torch path
def _zero_head_learner(M, dists, weight, cls="bc", **kw):
    from voxnav.imitate import BCLearner, KickstartLearner
    pol = bh.small_policy(False)
    with torch.no_grad():
        for p in list(pol.action_net.parameters()) + list(pol.value_net.parameters()):
            p.zero_()
    b = bh.dagger_arrays(M, 1, 16, False, seed=3)
    if weight is None:
        del b["label_weight"]
    else:
        b["label_weight"] = weight
    b["expert_dists"] = dists.reshape(M, 1, -1)
    make = BCLearner if cls == "bc" else KickstartLearner
    return pol, b, make(pol, n_epochs=1, batch_size=M, max_grad_norm=1e9, labels="soft", **kw)


@pytest.mark.parametrize("weighted", [False, True], ids=["all-labelled", "weights"])
def test_torch_path_zero_heads(weighted):
    """Zero heads and the hand-derived row: bc_loss = ln 6 - H(q), d ba = (1/6 - q) summed over the
    labelled / n; two rows without a positive distance are unlabelled."""
    M = 12
    dists = np.tile(np.array(ROW, np.int32), (M, 1))
    dists[3] = -1
    dists[7] = [-2, 0, -1, -1, -2, 0]
    weight = (np.arange(M).reshape(M, 1) % 3 != 1).astype(np.uint8) if weighted else None
    pol, b, ln = _zero_head_learner(M, dists, weight, label_tau=1.0)
    st = ln.train(so.soft_buffer(b, "cpu"), epoch_orders=[np.arange(M)])
    w = (dists > 0).any(1) * (np.ones(M) if weight is None else weight.reshape(-1))
    n = w.sum()
    q = _q_of_row()
    assert abs(st["bc_loss"] - (math.log(6) + (q[:4] * np.log(q[:4])).sum())) < 1e-6
    assert abs(st["labelled"] - n / M) < 1e-12 and st["accuracy"] == 1.0
    np.testing.assert_allclose(pol.action_net.bias.grad.numpy(), (1 / 6 - q), atol=1e-7)


@pytest.mark.parametrize("tau", [1e-30, 1e30])
def test_torch_path_extreme_temperatures_stay_finite(tau):
    M = 16
    dists = so.random_dists(np.random.default_rng(5), M, 6, ldd=6)
    pol, b, ln = _zero_head_learner(M, dists, None, label_tau=tau)
    st = ln.train(so.soft_buffer(b, "cpu"), epoch_orders=[np.arange(M)])
    assert all(math.isfinite(st[k]) for k in bh.STAT_KEYS + ("grad_norm",))
    assert bool(torch.isfinite(pol.action_net.bias.grad).all())


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("recurrent", [True, False], ids=["lstm", "mlp"])
@pytest.mark.parametrize("which", ["bc", "kickstart"])
def test_soft_learners_match_restatement_cpu(which, recurrent, masked):
    """``run_bc_set_parity``'s shapes and bounds (atol 2e-5, rtol 1e-4)."""
    so.run_soft_parity("cpu", which, recurrent, masked)


def test_label_tau_schedules_through_set_progress():
    from voxnav.imitate import BCLearner, KickstartLearner
    for make in (BCLearner, KickstartLearner):
        ln = make(bh.small_policy(False), labels="soft", label_tau=lambda p: 0.25 + 2.0 * p)
        assert ln.label_tau == 2.25                          # its value at 1 until the first call
        ln.set_progress(0.5)
        assert ln.label_tau == 1.25
        ln.set_progress(0.0)
        assert ln.label_tau == 0.25
        with pytest.raises(ValueError, match="progress_remaining"):
            ln.set_progress(1.5)
        fixed = make(bh.small_policy(False), labels="soft", label_tau=0.5, learning_rate=lambda p: 1e-3 * p)
        fixed.set_progress(0.5)
        assert fixed.label_tau == 0.5 and fixed.lr == 5e-4   # the parent's schedules still run
        bad = make(bh.small_policy(False), labels="soft", label_tau=lambda p: p)
        with pytest.raises(ValueError, match="label_tau"):
            bad.set_progress(0.0)


def test_the_schedule_reaches_the_loss():
    """Two minibatch losses under a schedule equal those of fixed temperatures."""
    M = 12
    dists = so.random_dists(np.random.default_rng(5), M, 6, ldd=6, p_none=0.0, p_single=0.0)
    got = []
    for tau in (lambda p: 0.2 + p, 1.2, 0.2):
        pol, b, ln = _zero_head_learner(M, dists, None, label_tau=tau)
        if callable(tau):
            a = ln.train(so.soft_buffer(b, "cpu"), epoch_orders=[np.arange(M)])["bc_loss"]
            pol2, b2, ln2 = _zero_head_learner(M, dists, None, label_tau=tau)
            ln2.set_progress(0.0)
            got += [a, ln2.train(so.soft_buffer(b2, "cpu"), epoch_orders=[np.arange(M)])["bc_loss"]]
        else:
            got.append(ln.train(so.soft_buffer(b, "cpu"), epoch_orders=[np.arange(M)])["bc_loss"])
    assert got[0] == got[2] and got[1] == got[3] and got[0] != got[1]


# ------------------------------------------------------------------ 3. vn_dagger_mix_best's rule
def _mix_inputs(N, seed=0):
    rng = np.random.default_rng(seed)
    expert = rng.integers(0, 6, N).astype(np.int32)
    policy = rng.integers(0, 6, N).astype(np.int32)
    dist = np.where(rng.random(N) < 0.2, -1, rng.integers(1, 50, N)).astype(np.int32)
    extra = rng.integers(0, 64, N) * (rng.random(N) < 0.6)
    best = np.where(dist == -1, 0, (1 << expert) | extra).astype(np.uint8)
    return policy, expert, dist, best


@pytest.mark.parametrize("beta", [0.0, 0.3, 1.0])
def test_mix_best_restatement(beta):
    N = 4099
    policy, expert, dist, best = _mix_inputs(N)
    gids = np.arange(N)
    ex, took, lw, own = so.mix_best(policy, expert, dist, best, beta, 4242, gids, 17)
    lab = dist != -1
    assert (lw == lab).all() and (own == (lab & (((best >> policy) & 1) == 1))).all()
    assert not (took & own).any() and not took[~lab].any()
    assert (ex[took == 1] == expert[took == 1]).all() and (ex[took == 0] == policy[took == 0]).all()
    if beta == 0.0:
        assert not took.any() and (ex == policy).all()
    if beta == 1.0:                                      # every labelled executed action is a shortest one
        assert (took == (lab & (own == 0))).all() and (((best >> ex) & 1) == 1)[lab].all()
    # singletons: vn_dagger_mix's executed actions and label weights
    single = np.where(lab, 1 << expert, 0).astype(np.uint8)
    ex1, took1, lw1, own1 = so.mix_best(policy, expert, dist, single, beta, 4242, gids, 17)
    ex0, took0, lw0 = bh.mix(policy, expert, dist, beta, 4242, gids, 17)
    assert (ex1 == ex0).all() and (lw1 == lw0).all() and (own1 == (lab & (policy == expert))).all()
    assert (took1 == (took0 & (own1 == 0))).all()
    # a policy action outside 0..7 is never its own best
    wild = policy.copy()
    wild[::5] = np.resize(np.array([-1, 8, 99, -7, 1 << 20], np.int32), wild[::5].shape)
    _, _, _, ownw = so.mix_best(wild, expert, dist, np.full(N, 255, np.uint8), beta, 4242, gids, 17)
    assert not ownw[::5].any()


# ------------------------------------------------------------------ 4. refusals on the Python side
def test_learners_refuse_what_they_cannot_train_on():
    from voxnav.imitate import BCLearner, KickstartLearner
    plain = bh.as_dagger_buffer(bh.dagger_arrays(4, 2, 16, False), "cpu")
    for make in (BCLearner, KickstartLearner):
        with pytest.raises(ValueError, match="expert_dists"):
            make(bh.small_policy(False), labels="soft").train(plain)
        with pytest.raises(ValueError, match="labels"):
            make(bh.small_policy(False), labels="softmax")
        for tau in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="label_tau"):
                make(bh.small_policy(False), labels="soft", label_tau=tau)
        # a policy with another action count than expert_dists' 6 columns
        from voxnav.policy import ActorCriticPolicy
        pol4 = ActorCriticPolicy(obs_dim=80, n_actions=4, net_arch=dict(pi=[16], vf=[16]))
        b = bh.dagger_arrays(4, 2, 16, False)
        b["expert_dists"] = np.ones((4, 2, 6), np.int32)
        with pytest.raises(ValueError, match="6 columns"):
            make(pol4, labels="soft").train(so.soft_buffer(b, "cpu"))


def test_collector_refuses_best_execution_without_sets():
    from voxnav import _native
    from voxnav.imitate import DaggerCollector, MaskedDaggerCollector
    env = types.SimpleNamespace(variant=_native.VN_VARIANT_CUBIC, info=types.SimpleNamespace(pad_w=8, pad_d=8))
    for make in (DaggerCollector, MaskedDaggerCollector):
        with pytest.raises(ValueError, match="execute='best'"):
            make(env, None, expert=object(), labels="action", execute="best")
        with pytest.raises(ValueError, match="execute"):
            make(env, None, expert=object(), labels="set", execute="policy")
        with pytest.raises(ValueError, match="labels"):
            make(env, None, expert=object(), labels="hard")


def test_learn_ops_refuse_bad_temperatures_and_distance_rows():
    from voxnav import learn_ops
    M, F, A = 4, 64, 6
    an, vn = torch.nn.Linear(F, A), torch.nn.Linear(F, 1)
    h = torch.zeros((2, M, F))
    dists = torch.ones((M, A), dtype=torch.int32)
    i32, f32_, u8 = (torch.zeros(M, dtype=t) for t in (torch.int32, torch.float32, torch.uint8))
    calls = {
        "bc_loss_soft": lambda d, tau: learn_ops.bc_loss_soft(h, an, vn, None, d, None, f32_, tau, 0.0, 0.5),
        "bc_loss_soft_masked": lambda d, tau: learn_ops.bc_loss_soft_masked(h, an, vn, None, d, None, u8, f32_, tau,
                                                                            0.0, 0.5),
        "ppo_bc_loss_soft": lambda d, tau: learn_ops.ppo_bc_loss_soft(h, an, vn, None, i32, f32_, f32_, f32_, d, None,
                                                                      0.2, 0.0, 0.5, 1.0, tau, True),
        "ppo_bc_loss_soft_masked": lambda d, tau: learn_ops.ppo_bc_loss_soft_masked(h, an, vn, None, i32, f32_, f32_,
                                                                                    f32_, d, None, u8, 0.2, 0.0, 0.5,
                                                                                    1.0, tau, True),
    }
    for name, call in calls.items():
        for tau in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="tau"):
                call(dists, tau)
        for bad in (None, dists[:, :A - 1], dists.reshape(-1)):
            with pytest.raises(ValueError, match="dists"):
                call(bad, 1.0)
    with pytest.raises(ValueError, match="action_masks"):
        learn_ops.bc_loss_soft_masked(h, an, vn, None, dists, None, None, f32_, 1.0, 0.0, 0.5)
    with pytest.raises(ValueError, match="action_masks"):
        learn_ops.ppo_bc_loss_soft_masked(h, an, vn, None, i32, f32_, f32_, f32_, dists, None, None, 0.2, 0.0, 0.5,
                                          1.0, 1.0, True)
