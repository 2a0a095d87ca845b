"""The set-valued behaviour-cloning loss off the GPU (include/voxnav.h, vn_bc_loss_set): known
answers of the float64 restatement (tests/bc_set_helpers.py), and ``BCLearner(labels="set")``'s
torch path against it.
"""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bc_helpers as bh  # noqa: E402
import bc_set_helpers as bs  # noqa: E402

F64 = torch.float64


def popcount(s):
    return np.array([bin(int(v)).count("1") for v in s])


# ------------------------------------------------------------------ 1. known answers
def test_zero_logits_give_ln_A_over_S_and_uniform_minus_uniform_on_S():
    """Zero logits: p = 1/A, so ce_i = -ln(|S_i| / A) and dz_ij = (1/n)(1/A - [j in S_i] / |S_i|);
    every logit ties, the argmax is index 0, so the accuracy is the share of sets that hold bit 0."""
    M, A = 9, 6
    sets = np.array([1, 3, 7, 15, 31, 63, 32, 40, 5], np.uint8)
    logits = torch.zeros((M, A), dtype=F64, requires_grad=True)
    z = torch.zeros(M, dtype=F64)
    r = bs.bc_set_terms(logits, z, sets, None, z, 0.0, 0.5)
    size = popcount(sets)
    assert abs(float(r["bc_loss"].detach()) - np.mean(np.log(A / size))) < 1e-12
    dz, = torch.autograd.grad(r["loss"], [logits])
    S = bs.members(sets, A).double()
    want = (1.0 / A - S / torch.as_tensor(size).view(-1, 1)) / M
    assert float((dz - want).abs().max()) < 1e-15
    assert float(r["accuracy"]) == float(np.mean(sets & 1)) and float(r["labelled"]) == 1.0


def test_full_set_gives_exactly_zero():
    M, A = 7, 6
    rng = np.random.default_rng(2)
    logits = torch.tensor(rng.normal(size=(M, A)), requires_grad=True)
    z = torch.zeros(M, dtype=F64)
    r = bs.bc_set_terms(logits, z, np.full(M, 63, np.uint8), None, z, 0.0, 0.0)
    assert abs(float(r["bc_loss"].detach())) < 1e-15 and float(r["accuracy"]) == 1.0
    dz, = torch.autograd.grad(r["loss"], [logits])
    assert float(dz.abs().max()) < 1e-16


@pytest.mark.parametrize("weighted", [False, True], ids=["all", "weights"])
def test_singletons_are_bc_terms(weighted):
    M, A = 11, 6
    rng = np.random.default_rng(3)
    labels = rng.integers(0, A, M)
    weight = (rng.random(M) < 0.7).astype(np.uint8) if weighted else None
    ret = torch.tensor(rng.normal(size=M))
    out = []
    for terms, lab in ((bh.bc_terms, torch.as_tensor(labels)), (bs.bc_set_terms, (1 << labels).astype(np.uint8))):
        logits = torch.tensor(np.random.default_rng(4).normal(size=(M, A)), requires_grad=True)
        values = torch.tensor(np.random.default_rng(5).normal(size=M), requires_grad=True)
        r = terms(logits, values, lab, weight, ret, 0.01, 0.5)
        out.append(([float(r[k].detach()) for k in bh.STAT_KEYS], torch.autograd.grad(r["loss"], [logits, values])))
    np.testing.assert_allclose(out[0][0], out[1][0], rtol=0, atol=1e-14)
    for x, y in zip(out[0][1], out[1][1]):
        assert float((x - y).abs().max()) < 1e-15


def test_empty_sets_behave_as_zero_weights():
    M, A = 9, 4
    rng = np.random.default_rng(1)
    sets = bs.random_sets(rng, (M,), A, p_empty=0.0)
    drop = np.arange(M) % 3 == 0
    ret = torch.tensor(rng.normal(size=M))
    out = []
    for s, w in ((np.where(drop, 0, sets), None), (sets, (~drop).astype(np.uint8))):
        logits = torch.tensor(np.random.default_rng(4).normal(size=(M, A)), requires_grad=True)
        values = torch.tensor(np.random.default_rng(5).normal(size=M), requires_grad=True)
        r = bs.bc_set_terms(logits, values, s.astype(np.uint8), w, ret, 0.0, 0.5)
        out.append(([float(r[k].detach()) for k in bh.STAT_KEYS], torch.autograd.grad(r["loss"], [logits, values])))
    assert out[0][0] == out[1][0]
    for x, y in zip(out[0][1], out[1][1]):
        assert torch.equal(x, y)
    # all sets empty: as all weights zero
    logits = torch.tensor(rng.normal(size=(M, A)), requires_grad=True)
    values = torch.tensor(rng.normal(size=M), requires_grad=True)
    r = bs.bc_set_terms(logits, values, np.zeros(M, np.uint8), None, ret, 0.0, 0.5)
    assert float(r["bc_loss"].detach()) == 0.0 and float(r["accuracy"]) == 0.0 and float(r["labelled"]) == 0.0
    dz, dv = torch.autograd.grad(r["loss"], [logits, values])
    assert float(dz.abs().max()) == 0.0
    assert float((dv - 2 * 0.5 * (values - ret).detach() / M).abs().max()) < 1e-15


def test_bits_at_or_above_A_are_ignored():
    M, A = 8, 6
    rng = np.random.default_rng(6)
    sets = rng.integers(0, 64, M).astype(np.uint8)
    sets[0] = 0
    high = (sets | np.array([64, 128, 192] * 3, np.uint8)[:M]).astype(np.uint8)     # sets[0]: only high bits = empty
    logits = torch.tensor(rng.normal(size=(M, A)))
    z = torch.zeros(M, dtype=F64)
    a, b = (bs.bc_set_terms(logits, z, s, None, z, 0.0, 0.0) for s in (sets, high))
    assert all(float(a[k]) == float(b[k]) for k in bh.STAT_KEYS)
    assert float(a["labelled"]) == float(np.mean(sets != 0)) < 1.0


# ------------------------------------------------------------------ 2. the torch path
def _zero_head_learner(M, sets, weight):
    from voxnav.imitate import BCLearner
    pol = bh.small_policy(False)
    with torch.no_grad():
        for p in list(pol.action_net.parameters()) + list(pol.value_net.parameters()):
            p.zero_()
    b = bh.dagger_arrays(M, 1, 16, False, seed=3)
    b["label_weight"] = weight
    if weight is None:
        del b["label_weight"]
    b["expert_set"] = sets.reshape(M, 1)
    return pol, b, BCLearner(pol, n_epochs=1, batch_size=M, max_grad_norm=1e9, labels="set")


@pytest.mark.parametrize("weighted", [False, True], ids=["all-labelled", "weights"])
def test_torch_path_zero_heads(weighted):
    """Zero heads: ce = mean over the labelled of ln(A / |S|), d ba = (1/n) sum_i (1/A - [j in S_i] / |S_i|)."""
    M, A = 12, 6
    sets = np.array([1, 3, 7, 15, 31, 63, 32, 40, 5, 0, 64 + 2, 128], np.uint8)      # two empty ones (0; only bit 7)
    weight = (np.arange(M).reshape(M, 1) % 3 != 0).astype(np.uint8) if weighted else None
    pol, b, ln = _zero_head_learner(M, sets, weight)
    st = ln.train(bs.set_buffer(b, "cpu"), epoch_orders=[np.arange(M)])
    S = bs.members(sets, A).numpy().astype(np.float64)
    size = S.sum(1)
    w = (size > 0) * (np.ones(M) if weight is None else weight.reshape(-1))
    n = w.sum()
    safe = np.maximum(size, 1)
    assert abs(st["bc_loss"] - (w * np.log(A / safe)).sum() / n) < 1e-6
    assert abs(st["labelled"] - n / M) < 1e-12
    assert abs(st["accuracy"] - (w * S[:, 0]).sum() / n) < 1e-12
    want = ((w[:, None] / n) * (1.0 / A - S / safe[:, None])).sum(0)
    np.testing.assert_allclose(pol.action_net.bias.grad.numpy(), want, atol=1e-7)


def test_torch_path_all_empty_sets():
    M = 12
    pol, b, ln = _zero_head_learner(M, np.full(M, 192, np.uint8), None)
    st = ln.train(bs.set_buffer(b, "cpu"), epoch_orders=[np.arange(M)])
    assert st["bc_loss"] == 0.0 and st["accuracy"] == 0.0 and st["labelled"] == 0.0
    assert float(pol.action_net.bias.grad.abs().max()) == 0.0 and float(pol.action_net.weight.grad.abs().max()) == 0.0
    assert float(pol.value_net.bias.grad.abs().max()) > 0.0


def test_set_learner_needs_sets_and_a_known_mode():
    from voxnav.imitate import BCLearner
    b = bh.as_dagger_buffer(bh.dagger_arrays(4, 2, 16, False), "cpu")
    with pytest.raises(ValueError, match="expert_set"):
        BCLearner(bh.small_policy(False), labels="set").train(b)
    with pytest.raises(ValueError, match="labels"):
        BCLearner(bh.small_policy(False), labels="sets")


@pytest.mark.parametrize("recurrent", [True, False], ids=["lstm", "mlp"])
def test_bc_set_learner_matches_restatement_cpu(recurrent):
    """tests/test_imitate_cpu.py's shapes and bounds for the action mode."""
    bs.run_bc_set_parity("cpu", recurrent)


def test_bc_set_learner_entropy_bonus_cpu():
    bs.run_bc_set_parity("cpu", False, ent_coef=0.01)
