"""``vn_action_mask`` and ``vn_policy_head_masked`` (csrc/voxnav_mask.hip) on
the GPU: the mask kernel against the NumPy restatement on every golden
observation and the hand-made rows, around its 16-agents-per-block tiling,
with a padded row stride and guard bytes; the masked draw against
``vn_policy_head`` (full masks: the same bits) and the float64 restatement of
tests/mask_helpers.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import mask_helpers as mh
from helpers import golden_trajectories, load_golden, philox_uniform

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64          # guard bytes on either side of the mask
FILL = 0xA5


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def golden_obs():
    """Every observation of the CubicEnv goldens (steps and resets), and the hand-made rows."""
    rows = []
    for p in golden_trajectories():
        d = load_golden(p)
        rows += [d["obs"], d["reset_obs"]]
    hand, want = mh.hand_rows()
    obs = np.concatenate(rows + [hand]).astype(np.float32)
    ref = mh.mask_reference(obs)
    assert ref[-len(want):].tolist() == want.tolist()
    return obs, ref


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _mask_raw(obs_dev, ldo, N):
    """vn_action_mask into a guarded byte buffer -> (rc, mask [N], guards intact)."""
    from voxnav import _native
    buf = torch.full((N + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
    rc = _native.load().vn_action_mask(_p(obs_dev), ldo, N, C.c_void_p(buf.data_ptr() + GUARD), None)
    torch.cuda.synchronize()
    ok = bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + N:] == FILL).all())
    return rc, buf[GUARD:GUARD + N].cpu().numpy(), ok


def test_mask_on_every_golden_observation(golden_obs):
    from voxnav.masking import action_masks, mask_to_bool
    obs, ref = golden_obs
    assert obs.shape[0] > 12_700
    x = torch.as_tensor(obs, device=DEV)
    got = action_masks(x)
    assert got.dtype == torch.uint8 and got.cpu().numpy().tolist() == ref.tolist()
    assert len(set(ref.tolist())) > 20                               # many different masks among them
    want_bool = ((ref[:, None] >> np.arange(6)) & 1).astype(bool)
    assert (mask_to_bool(got).cpu().numpy() == want_bool).all()
    out = torch.zeros(x.shape[0], dtype=torch.uint8, device=DEV)
    assert action_masks(x, out=out) is out and torch.equal(out, got)


@pytest.mark.parametrize("pad", [0, 3], ids=["dense", "ldo83"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_mask_tiling_edges_and_padded_rows(golden_obs, N, pad):
    obs, ref = golden_obs
    sel = np.random.default_rng(N).choice(obs.shape[0], N, replace=False)
    ldo = 80 + pad
    x = torch.full((N, ldo), float("nan"), device=DEV)               # the padding is never read into a result
    x[:, :80] = torch.as_tensor(obs[sel], device=DEV)
    rc, got, ok = _mask_raw(x, ldo, N)
    assert rc == 0 and ok
    assert got.tolist() == ref[sel].tolist()
    if pad:                                                          # the wrapper takes strided rows as they are
        from voxnav.masking import action_masks
        assert action_masks(x[:, :80]).cpu().numpy().tolist() == ref[sel].tolist()


def test_mask_refusals():
    from voxnav import _native
    lib = _native.load()
    x = torch.zeros((4, 80), device=DEV)
    m = torch.full((4,), FILL, dtype=torch.uint8, device=DEV)
    for args in ((None, 80, 4, _p(m)), (_p(x), 80, 4, None), (_p(x), 80, 0, _p(m)), (_p(x), 80, -1, _p(m)),
                 (_p(x), 79, 4, _p(m))):
        assert lib.vn_action_mask(*args, None) == -1, args
    torch.cuda.synchronize()
    assert bool((m == FILL).all())
    from voxnav.env import BatchedGridEnv
    from voxnav.rooms import box_room, single_room_set
    env = BatchedGridEnv(num_agents=4, rooms=single_room_set(box_room(8, 8, 4)), local_map_length=4, device=DEV,
                         variant="simple")
    try:
        with pytest.raises(ValueError, match="CubicEnv"):
            env.action_masks(x)
    finally:
        env.close()


# ------------------------------------------------------------------ the masked head
SEED, T_STEP, BASE = 1234, 77, 1000


def _head_case(N, P, A, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 1000 * N + P + A)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    c = dict(lp=torch.tanh(r(N, P)), lv=torch.tanh(r(N, P)), wa=r(A, P) * scale / P ** 0.5 * 4, ba=r(A) * 0.5 * scale,
             wv=r(P) / P ** 0.5, bv=r(1))
    return {k: v.to(DEV).contiguous() for k, v in c.items()}


def _head(c, N, P, A, mask, deterministic=False, masked=True):
    from voxnav import _native
    lib = _native.load()
    act = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    val = torch.full((N,), float("nan"), device=DEV)
    lp = torch.full((N,), float("nan"), device=DEV)
    pre = (_p(c["lp"]), _p(c["lv"]), N, P, _p(c["wa"]), _p(c["ba"]), A, _p(c["wv"]), _p(c["bv"]))
    post = (SEED, T_STEP, BASE, int(deterministic), _p(act), _p(val), _p(lp), None)
    rc = lib.vn_policy_head_masked(*pre, _p(mask), *post) if masked else lib.vn_policy_head(*pre, *post)
    torch.cuda.synchronize()
    assert rc == 0
    return act, val, lp


def _logits64(c):
    return c["lp"].double() @ c["wa"].double().T + c["ba"].double()


@pytest.mark.parametrize("deterministic", [False, True], ids=["sample", "argmax"])
@pytest.mark.parametrize("N,P,A", [(257, 128, 6), (33, 68, 1), (65, 256, 8)])
def test_full_masks_give_the_unmasked_head_bits(N, P, A, deterministic):
    c = _head_case(N, P, A)
    full = torch.full((N,), 0xFF, dtype=torch.uint8, device=DEV)      # bits at and above A are ignored
    a0, v0, l0 = _head(c, N, P, A, None, deterministic, masked=False)
    a1, v1, l1 = _head(c, N, P, A, full, deterministic)
    assert torch.equal(a0, a1) and torch.equal(v0, v1) and torch.equal(l0, l1)
    empty = torch.zeros(N, dtype=torch.uint8, device=DEV)            # S = 0 counts as all allowed
    a2, v2, l2 = _head(c, N, P, A, empty, deterministic)
    assert torch.equal(a0, a2) and torch.equal(v0, v2) and torch.equal(l0, l2)


def test_random_masks_against_float64():
    N, P, A = 257, 128, 6
    c = _head_case(N, P, A, seed=5)
    g = torch.Generator().manual_seed(11)
    mask = torch.randint(1, 64, (N,), generator=g).to(torch.uint8).to(DEV)
    act, val, lp = _head(c, N, P, A, mask)
    assert bool((((mask.long() >> act.long()) & 1) == 1).all())       # always an allowed action
    u = torch.as_tensor(philox_uniform(SEED, BASE + np.arange(N), T_STEP), device=DEV)
    ract, rlp, cdf = mh.masked_draw_reference(_logits64(c), mask, u)
    S = mh.allowed_sets(mask, A)
    edge = torch.where(S, (cdf - u.view(-1, 1)).abs(), torch.ones_like(cdf)).min(-1).values
    sure = edge > 1e-6
    assert int(sure.sum()) > N - 8
    assert torch.equal(act.long()[sure], ract[sure])
    # log-probs of the action the kernel took, under the restricted softmax
    zm = _logits64(c).masked_fill(~S, float("-inf"))
    want = torch.log_softmax(zm, -1).gather(1, act.long().view(-1, 1)).flatten()
    mh.close(lp.double(), want, rel=2e-5, floor=1e-6)
    v64 = c["lv"].double() @ c["wv"].double() + c["bv"].double()
    mh.close(val.double(), v64, rel=2e-5, floor=1e-6)
    # the masks change the draw: some agents' unmasked action was forbidden
    a0, v0, _ = _head(c, N, P, A, None, masked=False)
    assert int((((mask.long() >> a0.long()) & 1) == 0).sum()) > 0 and torch.equal(v0, val)


def test_deterministic_is_the_argmax_over_the_allowed_actions():
    N, P, A = 257, 128, 6
    c = _head_case(N, P, A, seed=6)
    g = torch.Generator().manual_seed(12)
    mask = torch.randint(1, 64, (N,), generator=g).to(torch.uint8).to(DEV)
    act, _, lp = _head(c, N, P, A, mask, deterministic=True)
    z = _logits64(c)
    ract, rlp, _ = mh.masked_draw_reference(z, mask, torch.zeros(N, device=DEV), deterministic=True)
    top2 = z.masked_fill(~mh.allowed_sets(mask, A), float("-inf")).topk(2, -1).values
    sure = (top2[:, 0] - top2[:, 1]) > 1e-5
    assert int(sure.sum()) > N - 8
    assert torch.equal(act.long()[sure], ract[sure])
    mh.close(lp.double()[sure], rlp[sure], rel=2e-5, floor=1e-6)
    # ties go to the lowest allowed index: equal logits everywhere
    c0 = dict(c, wa=torch.zeros_like(c["wa"]), ba=torch.zeros_like(c["ba"]))
    act, _, _ = _head(c0, N, P, A, mask, deterministic=True)
    lowest = torch.tensor([(int(m) & -int(m)).bit_length() - 1 for m in mask.cpu()], device=DEV)
    assert torch.equal(act.long(), lowest)


@pytest.mark.parametrize("deterministic", [False, True], ids=["sample", "argmax"])
def test_single_bit_masks(deterministic):
    N, P, A = 257, 128, 6
    c = _head_case(N, P, A, seed=7)
    bit = torch.arange(N) % A
    mask = (1 << bit).to(torch.uint8).to(DEV)
    act, _, lp = _head(c, N, P, A, mask, deterministic)
    assert torch.equal(act.long().cpu(), bit)
    assert bool((lp == 0.0).all())


def test_saturated_head_with_the_largest_logit_masked():
    """Logits spanning about +-60 with the largest one forbidden: it takes no
    part in the max or the log-sum-exp, so the draw and the log-prob stay
    finite and follow the restricted softmax."""
    N, P, A = 257, 128, 6
    c = _head_case(N, P, A, seed=8)
    z = _logits64(c)
    k = 120.0 / float((z.max(-1).values - z.min(-1).values).max())
    c["wa"] = (c["wa"] * k).contiguous()
    c["ba"] = (c["ba"] * k).contiguous()
    z = _logits64(c)
    top = z.argmax(-1)
    mask = (63 & ~(1 << top)).to(torch.uint8)
    act, _, lp = _head(c, N, P, A, mask)
    assert bool(torch.isfinite(lp).all()) and bool((act.long() != top).all())
    want = torch.log_softmax(z.masked_fill(~mh.allowed_sets(mask, A), float("-inf")), -1) \
        .gather(1, act.long().view(-1, 1)).flatten()
    assert bool(torch.isfinite(want).all())
    mh.close(lp.double(), want, rel=2e-5, floor=1e-5)


@pytest.mark.parametrize("A", [1, 8])
def test_action_count_edges(A):
    N, P = 65, 128
    c = _head_case(N, P, A, seed=9)
    g = torch.Generator().manual_seed(13)
    mask = torch.randint(0, 256, (N,), generator=g).to(torch.uint8).to(DEV)
    act, _, lp = _head(c, N, P, A, mask)
    S = mh.allowed_sets(mask, A)
    assert bool(S.gather(1, act.long().view(-1, 1)).all())
    want = torch.log_softmax(_logits64(c).masked_fill(~S, float("-inf")), -1).gather(1, act.long().view(-1, 1))
    mh.close(lp.double(), want.flatten(), rel=2e-5, floor=1e-6)
    if A == 1:
        assert bool((act == 0).all()) and bool((lp == 0.0).all())


def test_head_refusals():
    from voxnav import _native
    lib = _native.load()
    N, P, A = 8, 64, 6
    c = _head_case(N, P, A)
    mask = torch.full((N,), 63, dtype=torch.uint8, device=DEV)
    act = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    val = torch.zeros(N, device=DEV)
    lp = torch.zeros(N, device=DEV)

    def call(**over):
        a = dict(lp=_p(c["lp"]), lv=_p(c["lv"]), N=N, P=P, wa=_p(c["wa"]), ba=_p(c["ba"]), A=A, wv=_p(c["wv"]),
                 bv=_p(c["bv"]), mask=_p(mask), act=_p(act), val=_p(val), logp=_p(lp))
        a.update(over)
        return lib.vn_policy_head_masked(a["lp"], a["lv"], a["N"], a["P"], a["wa"], a["ba"], a["A"], a["wv"], a["bv"],
                                         a["mask"], SEED, T_STEP, BASE, 0, a["act"], a["val"], a["logp"], None)

    for over in (dict(mask=None), dict(lp=None), dict(wa=None), dict(ba=None), dict(act=None), dict(logp=None),
                 dict(wv=None), dict(val=None), dict(N=0), dict(P=6), dict(P=4100), dict(A=0), dict(A=9)):
        assert call(**over) == -1, over
    torch.cuda.synchronize()
    assert bool((act == -7).all())
    assert call() == 0 and call(lv=None, val=None) == 0               # the value head is optional
    torch.cuda.synchronize()
    assert bool((act >= 0).all())
