"""``vn_ppo_loss_masked`` (csrc/voxnav_masked_loss.hip) against the float64
autograd restatement of tests/mask_helpers.py over all 16 instantiations and
both action counts of each, around the sample tiling's edges, with and without
``src`` and the advantage normalisation -- the cases and tolerances of
tests/test_ppo_loss_grid_gpu.py -- and what masking adds: full masks give
``vn_ppo_loss``'s bits, a shared mask equals the restricted head, masked
actions get exact zeros, nothing turns NaN."""
import ctypes as C

import pytest
import torch

import gemm_helpers as gh
import mask_helpers as mh
from test_ppo_loss_grid_gpu import CLIP, DEV, ENT, VF, _case, _compare
from test_ppo_loss_grid_gpu import _wrapper as _unmasked

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _masks(c, seed=0, full=False):
    """Random masks over the buffer rows: about a sixth exclude the taken
    action (it is added back), a few are empty (they count as full), and bits
    at and above A are set at random (they are ignored)."""
    R = c["act"].numel()
    if full:
        return torch.full((R,), 0xFF, dtype=torch.uint8, device=DEV)
    g = torch.Generator().manual_seed(77 + seed + R)
    m = torch.randint(0, 256, (R,), generator=g)
    m[torch.rand(R, generator=g) < 0.05] &= ~((1 << c["A"]) - 1)
    return m.to(torch.uint8).to(DEV)


def _reference(c, mask, norm):
    g = lambda t: t if c["src"] is None else t[c["src"]]  # noqa: E731
    an, vn = c["an"], c["vn"]
    return mh.masked_ppo_loss_reference(c["h"], an.weight, an.bias, vn.weight, vn.bias, g(c["act"]), g(c["adv"]),
                                        g(c["olp"]), g(c["ret"]), g(mask), CLIP, ENT, VF, norm)


def _wrapper(c, mask, norm):
    from voxnav.learn_ops import ppo_loss_masked
    return ppo_loss_masked(c["h"], c["an"], c["vn"], c["src"], c["act"], c["adv"], c["olp"], c["ret"], mask, CLIP,
                           ENT, VF, norm)


def _refit_old_log_probs(c, mask):
    """old log-probs around the masked ones, so the ratio stays on both sides of the clip range"""
    M, A = c["M"], c["A"]
    sel = c["src"] if c["src"] is not None else torch.arange(M, device=DEV)
    with torch.no_grad():
        z = c["h"][0] @ c["an"].weight.T + c["an"].bias
        S = mh.allowed_sets(mask[sel], A, c["act"][sel])
        lp = torch.log_softmax(z.masked_fill(~S, float("-inf")), -1).gather(1, c["act"][sel].long().view(-1, 1))
        g = torch.Generator().manual_seed(M)
        c["olp"][sel] = lp.flatten() + 0.3 * torch.randn(M, generator=g).to(DEV)
    return c


def _masked_case(M, F, A, gather, seed=0, **kw):
    c = _case(M, F, A, gather, seed=seed, **kw)
    mask = _masks(c, seed)
    return _refit_old_log_probs(c, mask), mask


@pytest.mark.parametrize("A", range(1, 9))
@pytest.mark.parametrize("F", [64, 128, 192, 256])
def test_every_instantiation(F, A):
    c, mask = _masked_case(129, F, A, gather=True)
    _compare(_wrapper(c, mask, True), _reference(c, mask, True))


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("gather", [False, True], ids=["identity", "src"])
@pytest.mark.parametrize("M", [3, 31, 32, 33, 127, 128, 129, 257])
@pytest.mark.parametrize("F,A", [(192, 5), (64, 2)])
def test_sample_count_edges(F, A, M, gather, norm):
    c, mask = _masked_case(M, F, A, gather, seed=int(norm))
    _compare(_wrapper(c, mask, norm), _reference(c, mask, norm))


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("M,F,A", [(129, 192, 5), (257, 128, 6), (33, 64, 2), (65, 256, 8)])
def test_full_masks_give_the_unmasked_bits(M, F, A, norm):
    c = _case(M, F, A, gather=True)
    (d0, g0, s0), (d1, g1, s1) = _unmasked(c, norm), _wrapper(c, _masks(c, full=True), norm)
    assert torch.equal(d0, d1) and torch.equal(s0, s1)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    # and a mask that allows exactly the A actions, no stray high bits
    d2, g2, s2 = _wrapper(c, torch.full_like(_masks(c, full=True), (1 << A) - 1), norm)
    assert torch.equal(d0, d2) and torch.equal(s0, s2)


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
def test_shared_mask_equals_the_restricted_head(norm):
    """Every sample under the same mask, every taken action inside it: the loss
    of the head restricted to the allowed rows, actions remapped; the gradient
    rows and bias entries of the masked actions are exactly 0."""
    M, F, A = 257, 128, 6
    keep = [0, 2, 3, 5]
    c = _case(M, F, A, gather=True)
    remap = torch.tensor(keep, device=DEV, dtype=torch.int32)
    small = torch.randint(0, len(keep), (c["act"].numel(),), device=DEV)
    c["act"] = remap[small].contiguous()
    mask = torch.full((c["act"].numel(),), sum(1 << k for k in keep), dtype=torch.uint8, device=DEV)
    c = _refit_old_log_probs(c, mask)
    dh, grads, stats = _wrapper(c, mask, norm)
    an2 = torch.nn.Linear(F, len(keep)).to(DEV)
    with torch.no_grad():
        an2.weight.copy_(c["an"].weight[keep])
        an2.bias.copy_(c["an"].bias[keep])
    c2 = dict(c, A=len(keep), an=an2, act=small.to(torch.int32).contiguous())
    rdh, rgrads, rstats = _unmasked(c2, norm)
    mh.close(dh.double(), rdh.double(), rel=2e-5, floor=1e-9)
    mh.close(stats, rstats, rel=1e-5, floor=1e-7)
    mh.close(grads[0][keep].double(), rgrads[0].double(), rel=1e-4, floor=1e-9)
    mh.close(grads[1][keep].double(), rgrads[1].double(), rel=1e-4, floor=1e-9)
    for k in (2, 3):
        mh.close(grads[k].double(), rgrads[k].double(), rel=1e-4, floor=1e-9)
    out = [k for k in range(A) if k not in keep]
    assert bool((grads[0][out] == 0).all()) and bool((grads[1][out] == 0).all())
    assert bool((grads[0][keep] != 0).any())


def test_taken_action_outside_its_mask_is_finite():
    M, F, A = 129, 192, 5
    c = _case(M, F, A, gather=True)
    mask = ((31 & ~(1 << c["act"].long())) | 0xE0).to(torch.uint8)     # every taken action forbidden by its mask
    got = _wrapper(c, mask, True)
    assert all(bool(torch.isfinite(t).all()) for t in (got[0], got[2], *got[1]))
    _compare(got, _reference(c, mask, True))
    # only the taken action allowed: p = 1, the entropy and the policy gradient vanish
    one = torch.zeros_like(mask)
    dh, grads, stats = _wrapper(c, one, False)
    assert float(stats[2]) == 0.0 and bool((dh[0] == 0).all()) and bool((grads[0] == 0).all())


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("M,F,A", [(129, 192, 5), (257, 256, 8)])
def test_saturated_heads_with_the_largest_logit_masked(M, F, A, norm):
    c = _case(M, F, A, gather=True, logit_span=60.0)
    sel = c["src"]
    with torch.no_grad():
        z = c["h"][0] @ c["an"].weight.T + c["an"].bias
    top = z.argmax(-1)
    # the taken action is another one, and the largest logit is forbidden
    c["act"][sel] = ((top + 1 + torch.arange(M, device=DEV) % (A - 1)) % A).to(torch.int32)
    assert bool((c["act"][sel].long() != top).all())
    mask = torch.full((c["act"].numel(),), 0xFF, dtype=torch.uint8, device=DEV)
    mask[sel] = (0xFF & ~(1 << top)).to(torch.uint8)
    c = _refit_old_log_probs(c, mask)
    got = _wrapper(c, mask, norm)
    assert all(bool(torch.isfinite(t).all()) for t in (got[0], got[2], *got[1]))
    _compare(got, _reference(c, mask, norm))


def test_two_calls_are_bit_identical():
    c, mask = _masked_case(257, 128, 6, gather=True)
    (d0, g0, s0), (d1, g1, s1) = _wrapper(c, mask, True), _wrapper(c, mask, True)
    assert torch.equal(d0, d1) and torch.equal(s0, s1) and all(torch.equal(a, b) for a, b in zip(g0, g1))


# ------------------------------------------------------------------- raw ABI
def _raw(c, masks, norm, ldh=None, **over):
    """vn_ppo_loss_masked itself, every output between guard bands (the raw call
    of tests/test_ppo_loss_grid_gpu.py with the mask)."""
    from voxnav import _native
    lib = _native.load()
    M, F, A = c["M"], c["F"], c["A"]
    ldh = F if ldh is None else ldh
    PG = A * F + A + F + 1
    n1, n2 = C.c_int64(), C.c_int64()
    assert lib.vn_ppo_loss_masked_part_floats(M, F, A, C.byref(n1), C.byref(n2)) == 0
    S = lambda n: gh.Slab(DEV, 1, 1, n)  # noqa: E731
    s = dict(hp=gh.Slab(DEV, 1, M, F, ld=max(ldh, F)).put(c["h"][0]),
             hv=gh.Slab(DEV, 1, M, F, ld=max(ldh, F)).put(c["h"][1]),
             dhp=gh.Slab(DEV, 1, M, F), dhv=gh.Slab(DEV, 1, M, F), gh=S(PG), stats=S(12), adv_sums=S(256),
             part=S(n1.value), spart=S(2 * n2.value))
    an, vn = c["an"], c["vn"]
    t = dict(wa=an.weight.detach().contiguous(), ba=an.bias.detach(), wv=vn.weight.detach().contiguous(),
             bv=vn.bias.detach(), src=c["src"], act=c["act"], adv=c["adv"], olp=c["olp"], ret=c["ret"], mask=masks)
    ptr = {k: v.ptr for k, v in s.items()}
    ptr.update({k: (0 if v is None else v.data_ptr()) for k, v in t.items()})
    a = dict(M=M, F=F, A=A, ldh=ldh)
    for k, v in over.items():
        if k in a:
            a[k] = v
        else:
            ptr[k] = v
    p = lambda k: C.c_void_p(ptr[k]) if ptr[k] else None  # noqa: E731
    rc = lib.vn_ppo_loss_masked(p("hp"), p("hv"), a["ldh"], p("wa"), p("ba"), p("wv"), p("bv"), p("src"), p("act"),
                                p("adv"), p("olp"), p("ret"), p("mask"), a["M"], a["F"], a["A"], CLIP, ENT, VF,
                                int(norm), p("dhp"), p("dhv"), p("gh"), p("stats"), p("adv_sums"), p("part"),
                                p("spart"), None)
    torch.cuda.synchronize()
    return rc, s


@pytest.mark.parametrize("M,F,A", [(129, 192, 5), (33, 64, 2)])
def test_guard_bands_and_padded_latent_rows(M, F, A):
    c, mask = _masked_case(M, F, A, gather=True)
    rc, s = _raw(c, mask, True, ldh=F + 4)
    assert rc == 0
    for name, slab in s.items():
        assert slab.intact(), name
    dh = torch.stack([s["dhp"].mat(0), s["dhv"].mat(0)])
    g = s["gh"].mat(0)[0]
    grads = (g[:A * F].view(A, F), g[A * F:A * F + A], g[A * F + A:A * F + A + F].view(1, F), g[-1:])
    stats = s["stats"].mat(0)[0].contiguous().view(torch.float64)
    _compare((dh, grads, stats), _reference(c, mask, True))
    d2, g2, s2 = _wrapper(c, mask, True)
    assert torch.equal(dh, d2) and torch.equal(stats, s2) and all(torch.equal(a, b) for a, b in zip(grads, g2))


def test_refusals_leave_outputs_untouched():
    M, F, A = 8, 64, 6
    c, mask = _masked_case(M, F, A, gather=True)
    from voxnav import _native
    lib = _native.load()
    outs = ("dhp", "dhv", "gh", "stats", "adv_sums", "part", "spart")

    def refused(**over):
        rc, s = _raw(c, mask, True, **over)
        assert rc == -1, over
        for k in outs:
            assert s[k].untouched(), (over, k)

    for name in ("hp", "hv", "wa", "ba", "wv", "bv", "act", "adv", "olp", "ret", "mask", "dhp", "dhv", "gh", "stats",
                 "adv_sums", "part", "spart"):
        refused(**{name: 0})
        assert b"NULL" in lib.vn_last_error()
    for kw in (dict(M=0), dict(M=-3), dict(A=0), dict(A=9), dict(F=32), dict(F=100), dict(F=320), dict(ldh=F - 1)):
        refused(**kw)
    n1, n2 = C.c_int64(), C.c_int64()
    for bad in ((0, F, A), (M, 0, A), (M, F, 0)):
        assert lib.vn_ppo_loss_masked_part_floats(*bad, C.byref(n1), C.byref(n2)) == -1
    rc, s = _raw(c, mask, True)                # src may be NULL; the valid call goes through
    assert rc == 0 and not s["dhp"].untouched()
    assert _raw(dict(c, src=None), mask, True)[0] == 0
    from voxnav.learn_ops import ppo_loss_masked
    with pytest.raises(ValueError, match="uint8 masks"):
        ppo_loss_masked(c["h"], c["an"], c["vn"], c["src"], c["act"], c["adv"], c["olp"], c["ret"], mask.to(torch.int32),
                        CLIP, ENT, VF, True)
