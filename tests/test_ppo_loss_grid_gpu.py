"""``vn_ppo_loss`` (csrc/voxnav_ppo_loss.hip) over all of its 16
instantiations (F / 64 in 1..4 times the action count rounded up to even),
around the edges of its sample tiling (4 samples per pass, 32 per wave, 128
per block), at a padded latent row stride, with saturated heads and degenerate
advantages, and its argument refusals -- against the float64 autograd
restatement of tests/ppo_loss_helpers.py, to the tolerances of
test_learn_ops.test_ppo_loss_matches_float64."""
import ctypes as C
import math

import pytest
import torch

import gemm_helpers as gh
from ppo_loss_helpers import _ppo_loss_reference, close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CLIP, ENT, VF = 0.2, 0.01, 0.5


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _case(M, F, A, gather, seed=0, logit_span=None, adv=None):
    """Heads, latents and rollout buffers as test_ppo_loss_matches_float64
    builds them: old log-probs around the true ones, so the ratio falls on
    both sides of the clip range and inside it."""
    torch.manual_seed(1000 * M + 10 * F + A + seed)
    an, vn = torch.nn.Linear(F, A).to(DEV), torch.nn.Linear(F, 1).to(DEV)
    h = torch.tanh(torch.randn((2, M, F), device=DEV))
    if logit_span is not None and A > 1:
        # the widest sample's logits run from about -logit_span to +logit_span
        with torch.no_grad():
            z = h[0] @ an.weight.T + an.bias
            k = 2 * logit_span / (z.max(-1).values - z.min(-1).values).max()
            an.weight.mul_(k)
            an.bias.mul_(k)
    R = M + 1000 if gather else M
    src = torch.randperm(R, device=DEV)[:M].contiguous() if gather else None
    act = torch.randint(0, A, (R,), device=DEV, dtype=torch.int32)
    adv = torch.randn(R, device=DEV) * 3 + 0.5 if adv is None else torch.full((R,), adv, device=DEV)
    ret = torch.randn(R, device=DEV)
    with torch.no_grad():
        lp_true = torch.log_softmax(h[0] @ an.weight.T + an.bias, -1)
    sel = src if gather else torch.arange(M, device=DEV)
    olp = torch.randn(R, device=DEV) - 1.5
    olp[sel] = lp_true.gather(1, act[sel].long().view(-1, 1)).flatten() + 0.3 * torch.randn(M, device=DEV)
    return dict(M=M, F=F, A=A, an=an, vn=vn, h=h, src=src, act=act, adv=adv, olp=olp, ret=ret)


def _reference(c, norm):
    g = lambda t: t if c["src"] is None else t[c["src"]]  # noqa: E731
    an, vn = c["an"], c["vn"]
    return _ppo_loss_reference(c["h"], an.weight, an.bias, vn.weight, vn.bias, g(c["act"]), g(c["adv"]), g(c["olp"]),
                               g(c["ret"]), CLIP, ENT, VF, norm)


def _compare(got, ref):
    (dh, grads, stats), (rdh, rgrads, rstats) = got, ref
    assert bool(torch.isfinite(dh).all()) and bool(torch.isfinite(stats).all())
    close(dh.double(), rdh, rel=2e-5, floor=1e-9)
    for a, b in zip(grads, rgrads):
        assert a.shape == b.shape and bool(torch.isfinite(a).all())
        close(a.double(), b, rel=1e-4, floor=1e-9)
    close(stats, rstats, rel=1e-5, floor=1e-7)


def _wrapper(c, norm):
    from voxnav.learn_ops import ppo_loss
    return ppo_loss(c["h"], c["an"], c["vn"], c["src"], c["act"], c["adv"], c["olp"], c["ret"], CLIP, ENT, VF, norm)


@pytest.mark.parametrize("A", range(1, 9))
@pytest.mark.parametrize("F", [64, 128, 192, 256])
def test_every_instantiation(F, A):
    """Q = F / 64 in 1..4 times AM in {2, 4, 6, 8} (both A of each AM), at
    M = 129: one full block and one sample in the next."""
    c = _case(129, F, A, gather=True)
    _compare(_wrapper(c, True), _reference(c, True))


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("gather", [False, True], ids=["identity", "src"])
@pytest.mark.parametrize("M", [3, 31, 32, 33, 127, 128, 129, 257])
@pytest.mark.parametrize("F,A", [(192, 5), (64, 2)])
def test_sample_count_edges(F, A, M, gather, norm):
    c = _case(M, F, A, gather, seed=int(norm))
    _compare(_wrapper(c, norm), _reference(c, norm))


@pytest.mark.parametrize("gather", [False, True], ids=["identity", "src"])
@pytest.mark.parametrize("F,A", [(192, 5), (64, 2)])
def test_one_sample(F, A, gather):
    """M = 1.  Without normalisation: the formula.  With it the unbiased
    standard deviation of one sample is NaN, as torch's: the policy loss, the
    loss, dhp and the action head's gradients are NaN, and everything that
    does not depend on the advantage -- value loss, entropy loss, approx kl,
    clip fraction, dhv, the value head's gradients -- is unchanged
    (include/voxnav.h, vn_ppo_loss)."""
    c = _case(1, F, A, gather)
    _compare(_wrapper(c, False), _reference(c, False))
    dh, grads, stats = _wrapper(c, True)
    rdh, rgrads, rstats = _reference(c, True)
    assert bool(torch.isnan(rdh[0]).all()) and bool(torch.isfinite(rdh[1]).all())     # the float64 formula itself
    assert bool(torch.isnan(dh[0]).all())
    assert bool(torch.isnan(grads[0]).all()) and bool(torch.isnan(grads[1]).all())
    assert torch.equal(torch.isnan(stats).cpu(), torch.tensor([True, False, False, True, False, False]))
    assert torch.equal(torch.isnan(stats), torch.isnan(rstats))
    close(dh[1].double(), rdh[1], rel=2e-5, floor=1e-9)
    for k in (2, 3):
        close(grads[k].double(), rgrads[k], rel=1e-4, floor=1e-9)
    close(stats[[1, 2, 4, 5]], rstats[[1, 2, 4, 5]], rel=1e-5, floor=1e-7)


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("M,F,A", [(129, 192, 5), (33, 64, 2), (257, 256, 8)])
def test_saturated_heads(M, F, A, norm):
    """Logits spanning +-60: the smallest f32 probabilities underflow to 0
    (p log p must stay 0, not NaN); every output finite and within the same
    tolerance of float64."""
    c = _case(M, F, A, gather=True, logit_span=60.0)
    with torch.no_grad():
        z = (c["h"][0] @ c["an"].weight.T + c["an"].bias)
    assert math.isclose(float((z.max(-1).values - z.min(-1).values).max()), 120.0, rel_tol=1e-3)
    assert float(torch.softmax(z, -1).min()) == 0.0
    _compare(_wrapper(c, norm), _reference(c, norm))


@pytest.mark.parametrize("M,F,A", [(129, 192, 5), (2, 64, 2), (257, 128, 6)])
def test_zero_variance_advantages(M, F, A):
    """Every advantage equal: the normalised advantage is 0 / (0 + 1e-8) = 0,
    and every output is finite and equal to the float64 formula."""
    c = _case(M, F, A, gather=True, adv=0.3)
    got, ref = _wrapper(c, True), _reference(c, True)
    _compare(got, ref)
    assert float(got[2][0]) == 0.0 and float(ref[2][0]) == 0.0      # the policy loss of a zero advantage


# ------------------------------------------------------------------- raw ABI
def _raw(c, norm, ldh=None, **over):
    """vn_ppo_loss itself, every output between guard bands; latents with row
    stride ldh (padding: the sentinel NaN, which must never be read into a
    result).  Returns (rc, slabs dict)."""
    from voxnav import _native
    lib = _native.load()
    M, F, A = c["M"], c["F"], c["A"]
    ldh = F if ldh is None else ldh
    PG = A * F + A + F + 1
    n1, n2 = C.c_int64(), C.c_int64()
    assert lib.vn_ppo_loss_part_floats(M, F, A, C.byref(n1), C.byref(n2)) == 0
    S = lambda n: gh.Slab(DEV, 1, 1, n)  # noqa: E731
    s = dict(hp=gh.Slab(DEV, 1, M, F, ld=max(ldh, F)).put(c["h"][0]),
             hv=gh.Slab(DEV, 1, M, F, ld=max(ldh, F)).put(c["h"][1]),
             dhp=gh.Slab(DEV, 1, M, F), dhv=gh.Slab(DEV, 1, M, F), gh=S(PG), stats=S(12), adv_sums=S(256),
             part=S(n1.value), spart=S(2 * n2.value))
    an, vn = c["an"], c["vn"]
    t = dict(wa=an.weight.detach().contiguous(), ba=an.bias.detach(), wv=vn.weight.detach().contiguous(),
             bv=vn.bias.detach(), src=c["src"], act=c["act"], adv=c["adv"], olp=c["olp"], ret=c["ret"])
    ptr = {k: v.ptr for k, v in s.items()}
    ptr.update({k: (0 if v is None else v.data_ptr()) for k, v in t.items()})
    a = dict(M=M, F=F, A=A, ldh=ldh)
    for k, v in over.items():
        if k in a:
            a[k] = v
        else:
            ptr[k] = v
    p = lambda k: C.c_void_p(ptr[k]) if ptr[k] else None  # noqa: E731
    rc = lib.vn_ppo_loss(p("hp"), p("hv"), a["ldh"], p("wa"), p("ba"), p("wv"), p("bv"), p("src"), p("act"), p("adv"),
                         p("olp"), p("ret"), a["M"], a["F"], a["A"], CLIP, ENT, VF, int(norm), p("dhp"), p("dhv"),
                         p("gh"), p("stats"), p("adv_sums"), p("part"), p("spart"), None)
    torch.cuda.synchronize()
    return rc, s


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("M,F,A", [(129, 192, 5), (33, 64, 2)])
def test_padded_latent_rows(M, F, A, norm):
    """ldh = F + 4 through the raw ABI: the latents are read with the padded
    stride (the padding holds NaN patterns), dhp / dhv are written [M][F]
    contiguous as include/voxnav.h documents, and every guard band around
    the outputs and workspaces survives."""
    c = _case(M, F, A, gather=True)
    rc, s = _raw(c, norm, ldh=F + 4)
    assert rc == 0
    for name, slab in s.items():
        assert slab.intact(), name
    dh = torch.stack([s["dhp"].mat(0), s["dhv"].mat(0)])
    g = s["gh"].mat(0)[0]
    grads = (g[:A * F].view(A, F), g[A * F:A * F + A], g[A * F + A:A * F + A + F].view(1, F), g[-1:])
    stats = s["stats"].mat(0)[0].contiguous().view(torch.float64)
    _compare((dh, grads, stats), _reference(c, norm))
    # and the same bits as the dense call
    d2, g2, s2 = _wrapper(c, norm)
    assert torch.equal(dh, d2) and torch.equal(stats, s2)
    for a, b in zip(grads, g2):
        assert torch.equal(a, b)


def test_refusals_leave_outputs_untouched():
    M, F, A = 8, 64, 6
    c = _case(M, F, A, gather=True)
    from voxnav import _native
    lib = _native.load()
    outs = ("dhp", "dhv", "gh", "stats", "adv_sums", "part", "spart")

    def refused(**over):
        rc, s = _raw(c, True, **over)
        assert rc == -1, over
        for k in outs:
            assert s[k].untouched(), (over, k)

    for name in ("hp", "hv", "wa", "ba", "wv", "bv", "act", "adv", "olp", "ret", "dhp", "dhv", "gh", "stats",
                 "adv_sums", "part", "spart"):
        refused(**{name: 0})
        assert b"NULL" in lib.vn_last_error()
    for kw in (dict(M=0), dict(M=-3), dict(A=0), dict(A=9), dict(F=32), dict(F=100), dict(F=320), dict(ldh=F - 1)):
        refused(**kw)
    n1, n2 = C.c_int64(), C.c_int64()
    for bad in ((0, F, A), (M, 0, A), (M, F, 0)):
        assert lib.vn_ppo_loss_part_floats(*bad, C.byref(n1), C.byref(n2)) == -1
    rc, s = _raw(c, True)                      # src may be NULL; the valid call goes through
    assert rc == 0 and not s["dhp"].untouched()
    c2 = dict(c, src=None)
    assert _raw(c2, True)[0] == 0
