"""Masked DAgger / kickstart without a GPU: the planner never labels an action the
mask forbids (on the CPU oracle), the known answers of the S_i rule, both learners' torch path with
``action_masks=True`` against the float64 restatements of tests/masked_imitate_helpers.py within
test_imitate_cpu's and test_kickstart_cpu's bounds, full masks giving the unmasked learners'
parameters bit for bit, and the refusals."""
import math
import random

import numpy as np
import pytest
import torch

import bc_helpers as bh
import kickstart_helpers as kh
import mask_helpers as mh
import masked_imitate_helpers as mi
import route_dists_helpers as rd
import route_helpers as rh
from helpers import archive_texts, box_text

FORMS = pytest.mark.parametrize("sets", [False, True], ids=["action", "set"])


# ------------------------------------------------------------------ 1. planner against mask
def _oracle_rooms():
    from oracle.oracle import parse_room_text
    t = archive_texts()
    rooms = [parse_room_text(box_text(8, 8, 4), "box")]
    for name in ("P2_training/maze_8x8_seed22.txt", "P2_training/tightcorridor.txt", "P3_training/kitchen2.txt"):
        rooms.append(parse_room_text(t[name], name.split("/")[1]))
    return rooms


def test_the_planner_never_labels_a_masked_action():
    """A half-random, half-planner driver on the CPU oracle, four rooms at L = 4 and 10 (about 7,000
    steps): the mask of the observation is the planner's passable set, and every label and every
    ``best`` bit lies inside it."""
    from oracle.py_cubic import PyCubicAgent
    steps = labelled = narrow = 0
    for room in _oracle_rooms():
        for L in (4, 10):
            env = PyCubicAgent([room], local_map_length=L)
            rng = random.Random(7)
            for ep in range(3):
                obs = env.reset(3 + ep)
                for _ in range(min(env.max_steps, 400)):
                    m = int(mh.mask_reference(obs)[0])
                    pos = (env.x, env.y, env.z)
                    action, dist, _ = rh.plan(env.belief, pos, env.facing)
                    dists, best, _ = rd.plan_dists(env.belief, pos, env.facing)
                    assert m == sum(1 << k for k in range(6) if dists[k] != -2), (steps, m, dists)
                    assert best & ~m == 0, (steps, m, best)
                    if dist != -1:
                        labelled += 1
                        assert (m >> action) & 1, (steps, m, action)
                    narrow += m != 63
                    a = action if (rng.random() < 0.5 and dist != -1) else rng.randrange(6)
                    obs, _, done, trunc = env.step(a)
                    steps += 1
                    if done or trunc:
                        break
    print(f"{steps} steps, {labelled} labelled, {narrow} with a mask other than 63")
    assert steps > 6000 and labelled > steps // 2 and narrow >= 1


# ------------------------------------------------------------------ 2. known answers
def _one_update(which, sets, logits_bias, labels, masks, weight=None, actions=None, A=6, lr=0.0):
    """The learner's torch path on a policy with zero heads' weights (logits = the action bias):
    -> the train stats of one minibatch over T x N = len(labels) x 1 samples."""
    from voxnav.imitate import BCLearner, KickstartLearner
    pol = bh.small_policy(False)
    with torch.no_grad():
        pol.action_net.weight.zero_()
        pol.action_net.bias.copy_(torch.as_tensor(logits_bias, dtype=torch.float32))
    T = len(labels)
    b = bh.dagger_arrays(T, 1, 16, False)
    b["expert_actions"] = np.asarray(labels, np.int32).reshape(T, 1)
    b["expert_set"] = np.asarray(labels, np.uint8).reshape(T, 1)
    b["label_weight"] = np.ones((T, 1), np.uint8) if weight is None else np.asarray(weight, np.uint8).reshape(T, 1)
    b["action_masks"] = np.asarray(masks, np.uint8).reshape(T, 1)
    if actions is not None:
        b["actions"] = np.asarray(actions, np.int32).reshape(T, 1)
    form = "set" if sets else "action"
    if which == "bc":
        ln = BCLearner(pol, n_epochs=1, batch_size=T, labels=form, action_masks=True, learning_rate=lr)
    else:
        ln = KickstartLearner(pol, n_epochs=1, batch_size=T, labels=form, action_masks=True, learning_rate=lr)
    return ln.train(mi.masked_buffer(b, "cpu", sets), epoch_orders=[np.arange(T)])


@pytest.mark.parametrize("which", ["bc", "kickstart"])
def test_zero_heads_give_ln_of_the_support_size(which):
    """All logits 0: the cross-entropy of a single label inside a mask of |S| actions is ln |S|, and
    so is the entropy; an empty mask with its label is the singleton (0), without one it is full."""
    masks = [0b000111, 0b111111, 0b010010, 0b000000, 0b11000001]
    labels = [1, 5, 4, 2, 0]
    sizes = [3, 6, 2, 1, 1]
    st = _one_update(which, False, [0.0] * 6, labels, masks, actions=labels)
    assert st["bc_loss"] == pytest.approx(np.mean([math.log(s) for s in sizes]), abs=1e-6)
    assert st["entropy_loss"] == pytest.approx(-np.mean([math.log(s) for s in sizes]), abs=1e-6)
    assert st["accuracy"] == pytest.approx(2 / 5)        # the argmax is S's lowest index: the two singletons
    # unlabelled, the label stays out of S: an empty mask counts as full, entropy ln 6
    st = _one_update(which, False, [0.0] * 6, [2, 2], [0, 0], weight=[0, 0], actions=[2, 2])
    want = math.log(6) if which == "bc" else 0.0         # (under PPO the taken action is the singleton S)
    assert st["entropy_loss"] == pytest.approx(-want, abs=1e-6) and st["bc_loss"] == 0.0 and st["labelled"] == 0.0


@FORMS
@pytest.mark.parametrize("which", ["bc", "kickstart"])
def test_a_single_bit_mask_equal_to_the_label_gives_exactly_zero(which, sets):
    labels = [3, 0, 5, 2]
    bits = [1 << k for k in labels]
    st = _one_update(which, sets, [0.3, -2.0, 1.5, 0.1, 4.0, -0.7], bits if sets else labels, bits, actions=labels)
    assert st["bc_loss"] == 0.0 and st["entropy_loss"] == 0.0 and st["accuracy"] == 1.0 and st["labelled"] == 1.0


def test_the_restatement_knows_the_same_answers():
    z = torch.zeros((3, 6), dtype=torch.float64)
    v = torch.zeros(3, dtype=torch.float64)
    r = mi.masked_bc_terms(z, v, np.array([1, 5, 4]), np.array([0b000111, 0xFF, 0b000010]), None, v, 0.0, 0.0)
    assert float(r["bc_loss"]) == pytest.approx((math.log(3) + math.log(6) + math.log(2)) / 3, abs=1e-12)
    r = mi.masked_bc_terms(z + torch.arange(6), v, np.array([8, 1, 32], np.uint8), np.array([8, 1, 32]), None, v, 0.0,
                           0.0, sets=True)
    assert float(r["bc_loss"]) == 0.0 and float(r["entropy_loss"]) == 0.0


# ------------------------------------------------------------------ 3. torch path against float64
@FORMS
@pytest.mark.parametrize("recurrent", [False, True], ids=["mlp", "lstm"])
def test_bc_learner_matches_float64(recurrent, sets):
    ln, _ = mi.run_masked_parity("cpu", "bc", recurrent, sets)
    assert ln.fused_updates == 0 and ln.masked_fused_updates == 0


@FORMS
@pytest.mark.parametrize("recurrent", [False, True], ids=["mlp", "lstm"])
def test_kickstart_learner_matches_float64(recurrent, sets):
    ln, _ = mi.run_masked_parity("cpu", "kickstart", recurrent, sets)
    assert ln.fused_updates == 0 and ln.masked_fused_updates == 0


# ------------------------------------------------------------------ 4. full masks
@FORMS
@pytest.mark.parametrize("recurrent", [False, True], ids=["mlp", "lstm"])
@pytest.mark.parametrize("which", ["bc", "kickstart"])
def test_full_masks_give_the_unmasked_learners_parameters(which, recurrent, sets):
    from voxnav.imitate import BCLearner, KickstartLearner
    T, N = 12, 5
    b = mi.parity_arrays(T, N, 16, recurrent, sets, full=True)
    b["action_masks"][::2] = 63                           # both spellings of "full"
    orders = [3, 40] if recurrent else [np.random.default_rng(5).permutation(T * N) for _ in range(2)]
    cls = BCLearner if which == "bc" else KickstartLearner
    out = []
    for masked in (False, True):
        pol = bh.small_policy(recurrent)
        ln = cls(pol, n_epochs=2, batch_size=16, labels="set" if sets else "action", action_masks=masked)
        buf = mi.masked_buffer(b, "cpu", sets) if masked else kh.kickstart_buffer(b, "cpu", sets)
        ln.train(buf, epoch_orders=orders)
        out.append([p.detach().clone() for p in pol.parameters()])
    assert all(torch.equal(x, y) for x, y in zip(*out))
    assert any(not torch.equal(x, y) for x, y in zip(out[0], bh.small_policy(recurrent).parameters()))


# ------------------------------------------------------------------ 5. refusals
@pytest.mark.parametrize("which", ["bc", "kickstart"])
def test_a_buffer_without_masks_is_refused(which):
    from voxnav.imitate import BCLearner, KickstartLearner, MaskedDaggerBuffer
    from voxnav.collector import MaskedRolloutBuffer
    from voxnav.imitate import DaggerBuffer
    b = mi.parity_arrays(6, 3, 16, False, False)
    pol = bh.small_policy(False)
    ln = (BCLearner if which == "bc" else KickstartLearner)(pol, n_epochs=1, batch_size=8, action_masks=True)
    plain = kh.kickstart_buffer(b, "cpu", False)
    with pytest.raises(ValueError, match="action_masks"):
        ln.train(plain)
    with pytest.raises(ValueError, match="action_masks"):      # update() called directly refuses alike
        ln.update(plain, torch.arange(8))
    buf = mi.masked_buffer(b, "cpu", False)
    assert isinstance(buf, MaskedDaggerBuffer) and isinstance(buf, DaggerBuffer) and isinstance(buf, MaskedRolloutBuffer)
    assert ln.train(buf)["n_minibatches"] == 3
    # an unmasked learner takes the masked buffer as the DaggerBuffer it is
    ln0 = (BCLearner if which == "bc" else KickstartLearner)(bh.small_policy(False), n_epochs=1, batch_size=8)
    assert ln0.train(buf)["n_minibatches"] == 3
    if which == "kickstart":
        buf.took_expert[2, 1] = 1
        with pytest.raises(ValueError, match="beta = 0"):
            ln.train(buf)


def test_dagger_collector_still_refuses_action_masks():
    """The refusal comes before the env is touched: no GPU needed."""
    from voxnav import _native
    from voxnav.imitate import DaggerCollector, MaskedDaggerCollector

    class _Env:
        variant = _native.VN_VARIANT_CUBIC

    with pytest.raises(ValueError, match="action_masks"):
        DaggerCollector(_Env(), bh.small_policy(False), n_steps=4, action_masks=True)
    with pytest.raises(TypeError, match="action_masks"):
        MaskedDaggerCollector(_Env(), bh.small_policy(False), n_steps=4, action_masks=True)
    assert issubclass(MaskedDaggerCollector, DaggerCollector)
