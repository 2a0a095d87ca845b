"""``vn_bc_loss_masked`` / ``vn_bc_loss_set_masked`` (csrc/voxnav_masked_bc_loss.hip) and
``vn_ppo_bc_loss_masked`` / ``vn_ppo_bc_loss_set_masked`` (csrc/voxnav_masked_ppo_bc_loss.hip)
through their wrappers against the float64 restatements of tests/masked_imitate_helpers.py: all 32
(F, A) of each, the sample tiling's edges with and without src, weights and the advantage
normalisation over the bc_coef grid -- compared by ``test_ppo_loss_grid_gpu._compare`` with its
tolerances (dh rel 2e-5 / floor 1e-9, head gradients rel 1e-4 / floor 1e-9, stats rel 1e-5 / floor
1e-7), accuracy and labelled share exactly -- and what the masks add: the reductions to the unmasked
entries, to ``vn_ppo_loss_masked`` and to ``vn_bc_loss[_set]_masked`` bit for bit, a shared mask as
the restricted head with exact zeros outside it, saturated heads, determinism, the raw ABI between
guard bands, and every refusal."""
import ctypes as C

import pytest
import torch

import gemm_helpers as gh
import kickstart_helpers as kh
import mask_helpers as mh
import masked_imitate_helpers as mi
from test_ppo_loss_grid_gpu import _compare as _grid_compare

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CLIP, ENT, VF = 0.2, 0.01, 0.5
ENTRIES = pytest.mark.parametrize("ppo", [False, True], ids=["bc", "ppo_bc"])
FORMS = pytest.mark.parametrize("sets", [False, True], ids=["action", "set"])
BC_COEFS = (0.0, 0.3, 1.0, 4.0)


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------ cases
def _masks(c, seed=0, full=None):
    """Masks over the buffer rows, drawn like test_masked_loss_gpu._masks: uniform bytes (stray bits
    at and above A), about 5 % with no bit below A (they count as full unless a label or the taken
    action fills them); so some labels and taken actions lie outside their mask."""
    R = c["act"].numel()
    if full is not None:
        return torch.full((R,), full, dtype=torch.uint8, device=DEV)
    g = torch.Generator().manual_seed(77 + seed + R)
    m = torch.randint(0, 256, (R,), generator=g)
    m[torch.rand(R, generator=g) < 0.05] &= ~((1 << c["A"]) - 1)
    return m.to(torch.uint8).to(DEV)


def _sel(c):
    return c["src"] if c["src"] is not None else torch.arange(c["M"], device=DEV)


def _support(c, mask, ppo):
    """S [M, A] on the device, from the restatement's own rule."""
    sel = _sel(c)
    g = lambda t: None if t is None else t[sel]  # noqa: E731
    return mi.support(g(mask), g(c["lab"]), g(c["wgt"]), c["A"], c["sets"], g(c["act"]) if ppo else None).to(DEV)


def _refit_old_log_probs(c, mask):
    """old log-probs around the masked ones, so the ratio stays on both sides of the clip range"""
    sel, M = _sel(c), c["M"]
    with torch.no_grad():
        z = c["h"][0] @ c["an"].weight.T + c["an"].bias
        S = _support(c, mask, True)
        lp = torch.log_softmax(z.masked_fill(~S, float("-inf")), -1).gather(1, c["act"][sel].long().view(-1, 1))
        g = torch.Generator().manual_seed(M)
        c["olp"][sel] = lp.flatten() + 0.3 * torch.randn(M, generator=g).to(DEV)
    return c


def _case(M, F, A, gather, sets, seed=0, weights="random", **kw):
    c = kh.case(M, F, A, gather, DEV, seed=seed, weights=weights, sets=sets, **kw)
    mask = _masks(c, seed)
    return _refit_old_log_probs(c, mask), mask


def _outside(c, mask):
    """the shares of labelled samples whose label has a bit outside the mask, and of taken actions outside it"""
    sel, full = _sel(c), (1 << c["A"]) - 1
    w = None if c["wgt"] is None else c["wgt"][sel].cpu()
    L = mi.label_bits(c["lab"][sel], w, c["A"], c["sets"])
    m = mask[sel].cpu().long() & full
    return float(((L & ~m) != 0).double().mean()), float((((m >> c["act"][sel].cpu().long()) & 1) == 0).double().mean())


# ------------------------------------------------------------------ calls
def _masked(c, mask, ppo, norm=True, bc_coef=0.7, ent=ENT, vf=VF):
    from voxnav import learn_ops
    if ppo:
        fn = learn_ops.ppo_bc_loss_set_masked if c["sets"] else learn_ops.ppo_bc_loss_masked
        return fn(c["h"], c["an"], c["vn"], c["src"], c["act"], c["adv"], c["olp"], c["ret"], c["lab"], c["wgt"],
                  mask, CLIP, ent, vf, bc_coef, norm)
    fn = learn_ops.bc_loss_set_masked if c["sets"] else learn_ops.bc_loss_masked
    return fn(c["h"], c["an"], c["vn"], c["src"], c["lab"], c["wgt"], mask, c["ret"], ent, vf)


def _unmasked(c, ppo, norm=True, bc_coef=0.7, ent=ENT, vf=VF):
    from voxnav import learn_ops
    if ppo:
        fn = learn_ops.ppo_bc_loss_set if c["sets"] else learn_ops.ppo_bc_loss
        return fn(c["h"], c["an"], c["vn"], c["src"], c["act"], c["adv"], c["olp"], c["ret"], c["lab"], c["wgt"], CLIP,
                  ent, vf, bc_coef, norm)
    fn = learn_ops.bc_loss_set if c["sets"] else learn_ops.bc_loss
    return fn(c["h"], c["an"], c["vn"], c["src"], c["lab"], c["wgt"], c["ret"], ent, vf)


def _reference(c, mask, ppo, norm=True, bc_coef=0.7):
    return mi.reference(c, mask, ENT, VF, (CLIP, bc_coef, norm) if ppo else None)


def _compare(got, ref, ppo, what=""):
    """test_ppo_loss_grid_gpu._compare, its tolerances unchanged; accuracy and the labelled share
    (integer quotients in f64) exactly."""
    dh, grads, stats = got[0].cpu(), [g.cpu() for g in got[1]], got[2].cpu()
    print(what, "stats", stats.tolist(), "restatement", ref[2].tolist())
    assert stats.shape == ((9,) if ppo else (6,))
    _grid_compare((dh, grads, stats), ref)
    k = 7 if ppo else 4
    assert stats[k] == ref[2][k] and stats[k + 1] == ref[2][k + 1], (what, stats[k:], ref[2][k:])


def _same(a, b):
    """Equal as values (-0 equals +0): dh, the head gradients, the stats."""
    return torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1])) and torch.equal(a[2], b[2])


def _against_float64(c, mask, ppo, norm, bc_coef, what=""):
    assert kh.labelled_share(c) >= 0.5, what
    got = _masked(c, mask, ppo, norm, bc_coef)
    _compare(got, _reference(c, mask, ppo, norm, bc_coef), ppo, what)
    assert float(got[2][8 if ppo else 5]) >= 0.5


# ------------------------------------------------------------------ 1. every instantiation
@pytest.mark.parametrize("A", range(1, 9))
@pytest.mark.parametrize("F", [64, 128, 192, 256])
def test_every_instantiation(F, A):
    """Q = F / 64 in 1..4 times AM in {2, 4, 6, 8} (both A of each AM) of all four objectives, at
    M = 129: one full block and one sample in the next; through src, with weights, normalised."""
    seen = [0.0, 0.0]
    for sets in (False, True):
        c, mask = _case(129, F, A, True, sets)
        seen = [max(a, b) for a, b in zip(seen, _outside(c, mask))]
        for ppo in (False, True):
            _against_float64(c, mask, ppo, True, BC_COEFS[(F // 64 + A) % 4], f"F={F} A={A} sets={sets} ppo={ppo}")
    if A > 1:
        assert seen[0] > 0.05 and seen[1] > 0.05           # labels and taken actions outside their masks


# (gather through src, weights, normalize_advantage, bc_coef)
MODES = [(False, None, False, 0.3), (True, "random", True, 1.0), (False, "random", True, 4.0), (True, None, False, 0.0)]


@FORMS
@pytest.mark.parametrize("M", [3, 31, 32, 33, 127, 128, 129, 257])
@pytest.mark.parametrize("F,A", [(192, 5), (64, 2)])
def test_sample_count_edges(F, A, M, sets):
    """The 4-sample pass, the 32-sample wave and the 128-sample block edges; with and without src
    and weights, raw and normalised advantages (PPO+BC), every bc_coef of the grid."""
    for i, (gather, weights, norm, bc_coef) in enumerate(MODES):
        c, mask = _case(M, F, A, gather, sets, seed=i, weights=weights)
        for ppo in (False, True):
            _against_float64(c, mask, ppo, norm, bc_coef, f"M={M} F={F} A={A} mode={i} ppo={ppo}")


# ------------------------------------------------------------------ 5. reductions, bit for bit
@ENTRIES
@FORMS
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("M,F,A", [(129, 192, 5), (257, 128, 6), (33, 64, 2), (65, 256, 8)])
def test_full_masks_give_the_unmasked_bits(M, F, A, norm, sets, ppo):
    c = kh.case(M, F, A, True, DEV, weights="random", sets=sets)
    ref = _unmasked(c, ppo, norm)
    for full in (0xFF, (1 << A) - 1):                     # stray high bits, and exactly the A actions
        got = _masked(c, _masks(c, full=full), ppo, norm)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2]), full
        assert all(torch.equal(a, b) for a, b in zip(got[1], ref[1])), full


def _labels_inside(c, mask):
    """the masks with every sample's label bits (labelled or not) or-ed in"""
    full = (1 << c["A"]) - 1
    bits = (c["lab"].long() & full) if c["sets"] else (1 << c["lab"].long())
    return (mask.long() | bits).to(torch.uint8)


@FORMS
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("M,F,A", [(129, 128, 6), (257, 256, 8)])
def test_bc_coef_zero_gives_the_masked_ppo_loss(M, F, A, norm, sets):
    """bc_coef = 0 with the labels inside the masks: S_i is vn_ppo_loss_masked's, and dhp, dhv,
    grad_heads and stats[0..5] are its, as values."""
    from voxnav.learn_ops import ppo_loss_masked
    c, mask = _case(M, F, A, True, sets)
    mask = _labels_inside(c, mask)
    got = _masked(c, mask, True, norm, 0.0)
    ref = ppo_loss_masked(c["h"], c["an"], c["vn"], c["src"], c["act"], c["adv"], c["olp"], c["ret"], mask, CLIP, ENT,
                          VF, norm)
    assert _same((got[0], got[1], got[2][:6]), ref), (got[2].tolist(), ref[2].tolist())
    assert float(got[2][8]) >= 0.5 and float(got[2][6]) > 0.0      # labelled, with a cross-entropy to report


@FORMS
@pytest.mark.parametrize("weights", [None, "random"], ids=["all", "weights"])
@pytest.mark.parametrize("M,F,A", [(129, 128, 6), (257, 256, 8)])
def test_zero_advantages_give_the_masked_bc_gradients(M, F, A, weights, sets):
    """Advantages all 0, not normalised, bc_coef = 1, the taken actions inside the masks: the
    gradients are vn_bc_loss[_set]_masked's as values, and stats[6, 7, 8] its stats[0, 4, 5]."""
    c = kh.case(M, F, A, True, DEV, weights=weights, sets=sets, zero_adv=True)
    mask = (_masks(c).long() | (1 << c["act"].long())).to(torch.uint8)
    dh, grads, stats = _masked(c, mask, True, False, 1.0)
    rdh, rgrads, rstats = _masked(c, mask, False)
    assert torch.equal(dh, rdh) and all(torch.equal(a, b) for a, b in zip(grads, rgrads))
    assert torch.equal(stats[[6, 7, 8]], rstats[[0, 4, 5]]), (stats.tolist(), rstats.tolist())
    assert float(stats[0]) == 0.0                          # the policy loss of zero advantages


# ------------------------------------------------------------------ 6. a shared mask
@ENTRIES
@FORMS
def test_shared_mask_equals_the_restricted_head(sets, ppo):
    """Every sample under the same mask, every label and taken action inside it: the unmasked entry
    on the head restricted to the allowed rows, labels and actions remapped (the bounds of
    test_masked_loss_gpu's counterpart); the gradient rows and bias entries of the masked actions
    are exactly 0."""
    M, F, A = 257, 128, 6
    keep = [0, 2, 3, 5]
    K = len(keep)
    c = kh.case(M, F, A, True, DEV, weights="random", sets=sets)
    R = c["act"].numel()
    remap = torch.tensor(keep, device=DEV)
    small_act = torch.randint(0, K, (R,), device=DEV)
    c["act"] = remap[small_act].to(torch.int32).contiguous()
    if sets:
        small_lab = torch.randint(0, 1 << K, (R,), device=DEV)          # (some empty: unlabelled)
        big = sum(((small_lab >> j) & 1) << keep[j] for j in range(K))
        c["lab"] = big.to(torch.uint8).contiguous()
        small_lab = small_lab.to(torch.uint8).contiguous()
    else:
        small_lab = torch.randint(0, K, (R,), device=DEV)
        c["lab"] = remap[small_lab].to(torch.int32).contiguous()
        small_lab = small_lab.to(torch.int32).contiguous()
    mask = torch.full((R,), sum(1 << k for k in keep) | 0xC0, dtype=torch.uint8, device=DEV)
    c = _refit_old_log_probs(c, mask)
    dh, grads, stats = _masked(c, mask, ppo)
    an2 = torch.nn.Linear(F, K).to(DEV)
    with torch.no_grad():
        an2.weight.copy_(c["an"].weight[keep])
        an2.bias.copy_(c["an"].bias[keep])
    c2 = dict(c, A=K, an=an2, act=small_act.to(torch.int32).contiguous(), lab=small_lab)
    rdh, rgrads, rstats = _unmasked(c2, ppo)
    mh.close(dh.double(), rdh.double(), rel=2e-5, floor=1e-9)
    mh.close(stats, rstats, rel=1e-5, floor=1e-7)
    k = 7 if ppo else 4
    assert torch.equal(stats[k:k + 2], rstats[k:k + 2])
    mh.close(grads[0][keep].double(), rgrads[0].double(), rel=1e-4, floor=1e-9)
    mh.close(grads[1][keep].double(), rgrads[1].double(), rel=1e-4, floor=1e-9)
    for j in (2, 3):
        mh.close(grads[j].double(), rgrads[j].double(), rel=1e-4, floor=1e-9)
    out = [j for j in range(A) if j not in keep]
    assert bool((grads[0][out] == 0).all()) and bool((grads[1][out] == 0).all())
    assert bool((grads[0][keep] != 0).any())


# ------------------------------------------------------------------ 7. saturated heads
@ENTRIES
@FORMS
@pytest.mark.parametrize("M,F,A", [(129, 192, 5), (257, 256, 8)])
def test_saturated_heads_with_the_largest_logit_masked(M, F, A, sets, ppo):
    """Logits spanning about +-40, the largest one forbidden by every mask, and every labelled
    sample's label (the singleton of it) on its least likely allowed action: everything stays
    finite and within the same bounds."""
    c = kh.case(M, F, A, True, DEV, logit_span=40.0, weights="random", sets=sets)
    sel = c["src"]
    with torch.no_grad():
        z = c["h"][0] @ c["an"].weight.T + c["an"].bias
    top = z.argmax(-1)
    low = z.masked_fill(torch.arange(A, device=DEV).view(1, A) == top.view(-1, 1), float("inf")).argmin(-1)
    assert bool((low != top).all())
    c["act"][sel] = ((top + 1 + torch.arange(M, device=DEV) % (A - 1)) % A).to(torch.int32)
    c["lab"][sel] = ((torch.ones_like(low) << low) if sets else low).to(c["lab"].dtype)
    mask = torch.full((c["act"].numel(),), 0xFF, dtype=torch.uint8, device=DEV)
    mask[sel] = (0xFF & ~(1 << top)).to(torch.uint8)
    c = _refit_old_log_probs(c, mask)
    got = _masked(c, mask, ppo, True, 1.0)
    assert all(bool(torch.isfinite(t).all()) for t in (got[0], got[2], *got[1]))
    _compare(got, _reference(c, mask, ppo, True, 1.0), ppo)
    assert float(got[2][6 if ppo else 0]) > 5.0            # the far-off labels were in the sum


# ------------------------------------------------------------------ 8. relaunch
@ENTRIES
@FORMS
def test_two_calls_are_bit_identical(sets, ppo):
    c, mask = _case(257, 128, 6, True, sets)
    assert _same(_masked(c, mask, ppo), _masked(c, mask, ppo))


# ------------------------------------------------------------------ 9. raw ABI
def _raw(c, mask, ppo, norm=True, bc_coef=0.7, ldh=None, **over):
    """The entry point itself, every output between guard bands (tests/gemm_helpers.py's
    allocator); latents with row stride ldh.  -> (rc, slabs)."""
    from voxnav import _native
    lib = _native.load()
    M, F, A = c["M"], c["F"], c["A"]
    ldh = F if ldh is None else ldh
    PG = A * F + A + F + 1
    n1, n2 = C.c_int64(), C.c_int64()
    sizes = lib.vn_ppo_bc_loss_part_floats if ppo else lib.vn_bc_loss_part_floats
    assert sizes(M, F, A, C.byref(n1), C.byref(n2)) == 0
    nb = -(-M // 128)
    assert (n1.value, n2.value) == (nb * PG, nb * (7 if ppo else 4) + 64)      # the unmasked entries' sizes
    S = lambda n: gh.Slab(DEV, 1, 1, n)  # noqa: E731
    s = dict(hp=gh.Slab(DEV, 1, M, F, ld=max(ldh, F)).put(c["h"][0]),
             hv=gh.Slab(DEV, 1, M, F, ld=max(ldh, F)).put(c["h"][1]),
             dhp=gh.Slab(DEV, 1, M, F), dhv=gh.Slab(DEV, 1, M, F), gh=S(PG), stats=S(18 if ppo else 12),
             part=S(n1.value), spart=S(2 * n2.value))
    if ppo:
        s["adv_sums"] = S(256)
    an, vn = c["an"], c["vn"]
    t = dict(wa=an.weight.detach().contiguous(), ba=an.bias.detach(), wv=vn.weight.detach().contiguous(),
             bv=vn.bias.detach(), src=c["src"], act=c["act"], adv=c["adv"], olp=c["olp"], ret=c["ret"], lab=c["lab"],
             wgt=c["wgt"], msk=mask)
    ptr = {k: v.ptr for k, v in s.items()}
    ptr.update({k: (0 if v is None else v.data_ptr()) for k, v in t.items()})
    a = dict(M=M, F=F, A=A, ldh=ldh)
    for k, v in over.items():
        if k in a:
            a[k] = v
        else:
            ptr[k] = v
    p = lambda k: C.c_void_p(ptr[k]) if ptr[k] else None  # noqa: E731
    if ppo:
        fn = lib.vn_ppo_bc_loss_set_masked if c["sets"] else lib.vn_ppo_bc_loss_masked
        rc = fn(p("hp"), p("hv"), a["ldh"], p("wa"), p("ba"), p("wv"), p("bv"), p("src"), p("act"), p("adv"), p("olp"),
                p("ret"), p("lab"), p("wgt"), p("msk"), a["M"], a["F"], a["A"], CLIP, ENT, VF, bc_coef, int(norm),
                p("dhp"), p("dhv"), p("gh"), p("stats"), p("adv_sums"), p("part"), p("spart"), None)
    else:
        fn = lib.vn_bc_loss_set_masked if c["sets"] else lib.vn_bc_loss_masked
        rc = fn(p("hp"), p("hv"), a["ldh"], p("wa"), p("ba"), p("wv"), p("bv"), p("src"), p("lab"), p("wgt"),
                p("msk"), p("ret"), a["M"], a["F"], a["A"], ENT, VF, p("dhp"), p("dhv"), p("gh"), p("stats"),
                p("part"), p("spart"), None)
    torch.cuda.synchronize()
    return rc, s


@ENTRIES
@FORMS
@pytest.mark.parametrize("M,F,A", [(129, 192, 5), (33, 64, 2)])
def test_guard_bands_and_padded_latent_rows(M, F, A, sets, ppo):
    """ldh = F + 4 through the raw ABI: the latents are read with the padded stride (the padding
    holds NaN patterns), every guard band survives, and the results are the dense call's bits."""
    c, mask = _case(M, F, A, True, sets)
    rc, s = _raw(c, mask, ppo, ldh=F + 4)
    assert rc == 0
    for name, slab in s.items():
        assert slab.intact(), name
    dh = torch.stack([s["dhp"].mat(0), s["dhv"].mat(0)])
    g = s["gh"].mat(0)[0]
    grads = (g[:A * F].view(A, F), g[A * F:A * F + A], g[A * F + A:A * F + A + F].view(1, F), g[-1:])
    stats = s["stats"].mat(0)[0].contiguous().view(torch.float64)
    _compare((dh, grads, stats), _reference(c, mask, ppo), ppo)
    assert _same((dh, grads, stats), _masked(c, mask, ppo))


# ------------------------------------------------------------------ 10. refusals
@ENTRIES
@FORMS
def test_refusals_leave_outputs_untouched(sets, ppo):
    M, F, A = 8, 64, 6
    c, mask = _case(M, F, A, True, sets)
    from voxnav import _native, learn_ops
    lib = _native.load()
    outs = ("dhp", "dhv", "gh", "stats", "part", "spart") + (("adv_sums",) if ppo else ())

    def refused(bc_coef=0.7, **over):
        rc, s = _raw(c, mask, ppo, bc_coef=bc_coef, **over)
        assert rc == -1, (bc_coef, over)
        for k in outs:
            assert s[k].untouched(), (over, k)

    required = ("hp", "hv", "wa", "ba", "wv", "bv", "ret", "lab", "msk") + outs
    if ppo:
        required += ("act", "adv", "olp")
    for name in required:
        refused(**{name: 0})
        assert b"NULL" in lib.vn_last_error()
    for kw in (dict(M=0), dict(M=-3), dict(A=0), dict(A=9), dict(F=32), dict(F=100), dict(F=320), dict(ldh=F - 1)):
        refused(**kw)
    if ppo:
        for bad in (-0.5, float("nan"), float("inf"), float("-inf")):
            refused(bc_coef=bad)
            assert b"bc_coef" in lib.vn_last_error()
    # src and weight may be NULL (bc_coef may be 0); the valid calls go through
    rc, s = _raw(c, mask, ppo)
    assert rc == 0 and not s["dhp"].untouched()
    assert _raw(dict(c, src=None, wgt=None), mask, ppo, bc_coef=0.0)[0] == 0
    # the wrappers: an absent, a mistyped and a strided mask buffer
    with pytest.raises(ValueError, match="action_masks is required"):
        _masked(c, None, ppo)
    with pytest.raises(ValueError, match="uint8 masks"):
        _masked(c, mask.to(torch.int32), ppo)
    with pytest.raises(ValueError, match="uint8 masks"):
        _masked(c, torch.stack([mask, mask], 1)[:, 0], ppo)
    assert all(hasattr(learn_ops, n) for n in ("bc_loss_masked", "bc_loss_set_masked", "ppo_bc_loss_masked",
                                               "ppo_bc_loss_set_masked"))
