"""Invalid-action masking without a GPU: the mask formula (tests/mask_helpers.py
restates include/voxnav.h vn_action_mask) against the bumps the unmodified
reference recorded in every CubicEnv golden trajectory and against hand-made
rows; the torch path of ``PPOLearner(action_masks=True)`` against its float64
restatement; and the refusals that need no device."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mask_helpers as mh  # noqa: E402
from helpers import golden_trajectories, load_golden  # noqa: E402
from test_ppo import _as_rollout, _buffer, _policy  # noqa: E402


def test_mask_equals_the_reference_bumps_on_every_golden_trajectory():
    """For every step of every traj_*.npz: bit actions[t] of the mask of the
    observation the step acted on (obs[t - 1], or the reset obs after an episode
    end and at t = 0) is clear iff bump_count rose at t.  Nothing is skipped."""
    checked = bumps = 0
    files = golden_trajectories()
    assert len(files) == 15
    for path in files:
        prev, act, bumped = mh.golden_pairs(load_golden(path))
        m = mh.mask_reference(prev)
        assert not (m & 0xC0).any(), path.stem                        # bits 6 and 7 are 0
        blocked = ((m >> act) & 1) == 0
        bad = np.flatnonzero(blocked != bumped)
        assert bad.size == 0, (path.stem, bad[:5].tolist())
        checked += len(act)
        bumps += int(bumped.sum())
    assert checked >= 12_600 and bumps >= 1_000, (checked, bumps)


def test_hand_made_rows():
    rows, want = mh.hand_rows()
    assert rows.shape == (4 * 14, 80)
    assert mh.mask_reference(rows).tolist() == want.tolist()
    # facing north, a wall ahead (+y): forward is the one forbidden action
    assert int(mh.mask_reference(mh.hand_row(0, [(0, 1, 0)]))[0]) == 0b111110
    # facing east, the same wall is to the left
    assert int(mh.mask_reference(mh.hand_row(1, [(0, 1, 0)]))[0]) == 0b110111
    # a visited or unknown-but-in-bounds cell never blocks: only the two codes do
    o = mh.hand_row(2)
    o[mh.cell(0, -1, 0)] = np.float32(2) / np.float32(22)            # known free, never visited
    assert int(mh.mask_reference(o)[0]) == 63


def test_mask_to_bool_layout():
    from voxnav.masking import mask_to_bool
    b = mask_to_bool(torch.tensor([0, 63, 0b100101, 0xFF], dtype=torch.uint8))
    assert b.dtype == torch.bool and b.shape == (4, 6)
    assert b.tolist() == [[False] * 6, [True] * 6, [True, False, True, False, False, True], [True] * 6]


def _masked_buffer(T, N, full=False, seed=3):
    from voxnav.collector import MaskedRolloutBuffer
    b = _as_rollout(_buffer(T, N, 16, False), "cpu")
    g = torch.Generator().manual_seed(seed)
    m = torch.full((T, N), 63, dtype=torch.uint8) if full else \
        torch.randint(0, 64, (T, N), generator=g).to(torch.uint8)
    fields = {k: getattr(b, k) for k in b.__dataclass_fields__}
    return MaskedRolloutBuffer(action_masks=m, **fields)


def test_torch_path_matches_float64():
    """PPOLearner(action_masks=True) on the CPU (torch autograd of the masked
    formula) against the float64 restatement, to test_ppo's CPU bounds:
    parameters within 2e-5 + 1e-4 relative, logged losses within 1e-4
    relative.  Random masks: some exclude the taken action (it is added), some
    are empty (they count as full)."""
    from voxnav.ppo import PPOLearner
    T, N, bs, epochs = 12, 5, 16, 2
    pol = _policy(False)
    buf = _masked_buffer(T, N)
    taken = (buf.action_masks.long() >> buf.actions.long()) & 1
    assert int((taken == 0).sum()) > 0
    rng = np.random.default_rng(7)
    orders = [rng.permutation(T * N) for _ in range(epochs)]
    ref, logs = mh.masked_train_reference(pol, buf, orders, bs)
    w0 = {k: v.detach().clone() for k, v in pol.state_dict().items()}
    ln = PPOLearner(pol, n_epochs=epochs, batch_size=bs, action_masks=True)
    st = ln.train(buf, epoch_orders=orders)
    moved = 0.0
    for k, v in ref.state_dict().items():
        np.testing.assert_allclose(pol.state_dict()[k].numpy(), v.numpy(), atol=2e-5, rtol=1e-4, err_msg=k)
        moved = max(moved, float((v - w0[k].double()).abs().max()))
    assert moved > 1e-4
    assert st["n_minibatches"] == len(logs)
    for key in ("policy_gradient_loss", "value_loss", "entropy_loss", "loss"):
        want = np.mean([s[key] for s in logs])
        assert abs(st[key] - want) <= 1e-4 * max(1.0, abs(want)), (key, st[key], want)
    # the masks matter: the unmasked learner ends elsewhere
    pol2 = _policy(False)
    PPOLearner(pol2, n_epochs=epochs, batch_size=bs).train(buf, epoch_orders=orders)
    assert any(not torch.equal(a, b) for a, b in zip(pol.state_dict().values(), pol2.state_dict().values()))


@pytest.mark.parametrize("recurrent", [False, True], ids=["mlp", "lstm"])
def test_full_masks_equal_the_unmasked_learner(recurrent):
    from voxnav.collector import MaskedRolloutBuffer
    from voxnav.ppo import PPOLearner
    T, N = 12, 5
    b = _as_rollout(_buffer(T, N, 16, recurrent), "cpu")
    fields = {k: getattr(b, k) for k in b.__dataclass_fields__}
    mb = MaskedRolloutBuffer(action_masks=torch.full((T, N), 63, dtype=torch.uint8), **fields)
    rng = np.random.default_rng(7)
    orders = [int(rng.integers(T * N)) for _ in range(2)] if recurrent else [rng.permutation(T * N) for _ in range(2)]
    pa, pb = _policy(recurrent), _policy(recurrent)
    PPOLearner(pa, n_epochs=2, batch_size=16).train(b, epoch_orders=orders)
    PPOLearner(pb, n_epochs=2, batch_size=16, action_masks=True).train(mb, epoch_orders=orders)
    for (k, x), y in zip(pa.state_dict().items(), pb.state_dict().values()):
        assert torch.equal(x, y), k


def test_refusals():
    from voxnav.ppo import PPOLearner
    pol = _policy(False)
    plain = _as_rollout(_buffer(4, 3, 16, False), "cpu")
    with pytest.raises(ValueError, match="action_masks"):
        PPOLearner(pol, action_masks=True).train(plain)
    with pytest.raises(ValueError, match="action_masks"):      # update() called directly refuses alike
        PPOLearner(pol, action_masks=True).update(plain, torch.arange(12))
    from voxnav.masking import action_masks
    with pytest.raises(ValueError, match="obs"):
        action_masks(torch.zeros(3, 80))                       # not on the GPU
    with pytest.raises(ValueError, match="obs"):
        action_masks(torch.zeros(3, 79))
