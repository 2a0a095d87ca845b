"""``vn_ppo_bc_loss`` / ``vn_ppo_bc_loss_set`` (csrc/voxnav_ppo_bc_loss.hip) against the float64
autograd restatement of tests/kickstart_helpers.py over all 16 instantiations of each objective and
the edges of the sample tiling, to tests/test_ppo_loss_grid_gpu.py's tolerances (dh rel 2e-5 / floor
1e-9, head gradients rel 1e-4 / floor 1e-9, stats rel 1e-5 / floor 1e-7; accuracy and labelled share
exact: integer quotients in f64); their reductions to ``vn_ppo_loss`` and to ``vn_bc_loss`` /
``vn_bc_loss_set`` as values; linearity against those two; determinism; guard bands; saturated
heads; refusals."""
import ctypes as C

import pytest
import torch

import gemm_helpers as gh
import kickstart_helpers as kh
from ppo_loss_helpers import close

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CLIP, ENT, VF = 0.2, 0.01, 0.5
FORMS = pytest.mark.parametrize("sets", [False, True], ids=["action", "set"])


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _fused(c, norm, bc_coef, ent=ENT, vf=VF):
    from voxnav import learn_ops
    fn = learn_ops.ppo_bc_loss_set if c["sets"] else learn_ops.ppo_bc_loss
    return fn(c["h"], c["an"], c["vn"], c["src"], c["act"], c["adv"], c["olp"], c["ret"], c["lab"], c["wgt"], CLIP,
              ent, vf, bc_coef, norm)


def _ppo(c, norm, ent=ENT, vf=VF):
    from voxnav.learn_ops import ppo_loss
    return ppo_loss(c["h"], c["an"], c["vn"], c["src"], c["act"], c["adv"], c["olp"], c["ret"], CLIP, ent, vf, norm)


def _bc(c, ent=ENT, vf=VF):
    from voxnav import learn_ops
    fn = learn_ops.bc_loss_set if c["sets"] else learn_ops.bc_loss
    return fn(c["h"], c["an"], c["vn"], c["src"], c["lab"], c["wgt"], c["ret"], ent, vf)


def _compare(got, ref, what=""):
    (dh, grads, stats), (rdh, rgrads, rstats) = got, ref
    dh, grads, stats = dh.cpu(), [g.cpu() for g in grads], stats.cpu()
    print(what, "stats", stats.tolist(), "restatement", rstats.tolist())
    assert stats.shape == (9,) and bool(torch.isfinite(dh).all()) and bool(torch.isfinite(stats).all())
    close(dh.double(), rdh, rel=2e-5, floor=1e-9)
    for a, b in zip(grads, rgrads):
        assert a.numel() == b.numel() and bool(torch.isfinite(a).all())
        close(a.double().reshape(-1), b.reshape(-1), rel=1e-4, floor=1e-9)
    close(stats[:7], rstats[:7], rel=1e-5, floor=1e-7)
    assert stats[7] == rstats[7] and stats[8] == rstats[8], (what, stats[7:], rstats[7:])


def _same(a, b):
    """Equal as values (-0 equals +0), entry by entry."""
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _against_float64(c, norm, bc_coef, what=""):
    assert kh.labelled_share(c) >= 0.5, what
    got = _fused(c, norm, bc_coef)
    again = _fused(c, norm, bc_coef)
    assert torch.equal(got[0], again[0]) and torch.equal(got[2], again[2]) and _same(got[1], again[1]), what
    _compare(got, kh.reference(c, CLIP, ENT, VF, bc_coef, norm), what)
    assert float(got[2][8]) >= 0.5


# ------------------------------------------------------------------ 1. against float64
BC_COEFS = (0.0, 0.3, 1.0, 4.0)


@FORMS
@pytest.mark.parametrize("A", range(1, 9))
@pytest.mark.parametrize("F", [64, 128, 192, 256])
def test_every_instantiation(F, A, sets):
    """Q = F / 64 in 1..4 times AM in {2, 4, 6, 8} (both A of each AM) of both objectives, at
    M = 129: one full block and one sample in the next; through src, with weights, normalised."""
    c = kh.case(129, F, A, True, DEV, weights="random", sets=sets)
    _against_float64(c, True, BC_COEFS[(F // 64 + A) % 4], f"F={F} A={A}")


# (gather through src, weights, normalize_advantage, bc_coef)
MODES = [(False, None, False, 0.3), (True, "random", True, 1.0), (False, "random", True, 4.0), (True, None, False, 0.0)]


@FORMS
@pytest.mark.parametrize("M", [1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 257])
@pytest.mark.parametrize("F,A", [(192, 5), (64, 2)])
def test_sample_count_edges(F, A, M, sets):
    """The 4-sample pass, the 32-sample wave and the 128-sample block edges; with and without src,
    weights and advantage normalisation, every bc_coef of the grid.  (M = 1 is not normalised: the
    unbiased std of one sample is NaN, as vn_ppo_loss documents.)"""
    for i, (gather, weights, norm, bc_coef) in enumerate(MODES):
        c = kh.case(M, F, A, gather, DEV, seed=i, weights=weights, sets=sets)
        _against_float64(c, norm and M > 1, bc_coef, f"M={M} F={F} A={A} mode={i}")


# ------------------------------------------------------------------ 2. reduction to vn_ppo_loss
@FORMS
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("M", [129, 257])
@pytest.mark.parametrize("F,A", [(128, 6), (256, 8)])
def test_reduces_to_ppo_loss(F, A, M, norm, sets):
    """bc_coef = 0 with any labels, and any bc_coef with no labelled sample (all-zero weights; sets
    with no bit below A): dhp, dhv, grad_heads and stats[0:6] are vn_ppo_loss's, as values."""
    c = kh.case(M, F, A, True, DEV, weights="random", sets=sets)
    ref = _ppo(c, norm)
    zero = torch.ones_like(c["wgt"])                                  # rows outside the minibatch do not count
    zero[c["src"]] = 0
    runs = [("bc_coef=0", c, 0.0), ("bc_coef=0 unweighted", dict(c, wgt=None), 0.0),
            ("zero weights", dict(c, wgt=zero), 2.5)]
    if sets:
        empty = torch.full_like(c["lab"], (0xFF << A) & 0xFF)          # bits at or above A are ignored
        runs.append(("empty sets", dict(c, lab=empty, wgt=None), 2.5))
    for name, cc, bc_coef in runs:
        dh, grads, stats = _fused(cc, norm, bc_coef)
        assert torch.equal(dh, ref[0]), name
        assert _same(grads, ref[1]), name
        assert torch.equal(stats[:6], ref[2]), (name, stats.tolist(), ref[2].tolist())
        if bc_coef != 0.0:
            assert stats[6:].tolist() == [0.0, 0.0, 0.0], name


# ------------------------------------------------------------------ 3. reduction to vn_bc_loss(_set)
@FORMS
@pytest.mark.parametrize("weights", [None, "random"], ids=["all", "weights"])
@pytest.mark.parametrize("M", [129, 257])
@pytest.mark.parametrize("F,A", [(128, 6), (256, 8)])
def test_reduces_to_bc_loss(F, A, M, weights, sets):
    """Advantages all 0, not normalised, finite old log-probs, bc_coef = 1: the gradients are the
    BC call's as values, and stats[6, 7, 8] its stats[0, 4, 5]."""
    c = kh.case(M, F, A, True, DEV, weights=weights, sets=sets, zero_adv=True)
    dh, grads, stats = _fused(c, False, 1.0)
    rdh, rgrads, rstats = _bc(c)
    assert torch.equal(dh, rdh) and _same(grads, rgrads)
    assert torch.equal(stats[[6, 7, 8]], rstats[[0, 4, 5]]), (stats.tolist(), rstats.tolist())
    assert float(stats[0]) == 0.0                                    # the policy loss of zero advantages


# ------------------------------------------------------------------ 4. linearity
@FORMS
@pytest.mark.parametrize("bc_coef", [0.3, 4.0])
@pytest.mark.parametrize("M,F,A", [(129, 128, 6), (257, 256, 8), (33, 64, 3)])
def test_linear_in_the_two_merged_kernels(M, F, A, bc_coef, sets):
    """dh and the head gradients equal vn_ppo_loss(ent, vf) + bc_coef vn_bc_loss(ent = 0, vf = 0)
    within the sum of the two calls' tolerances against float64."""
    c = kh.case(M, F, A, True, DEV, weights="random", sets=sets)
    dh, grads, _ = _fused(c, True, bc_coef)
    pdh, pgrads, _ = _ppo(c, True)
    bdh, bgrads, _ = _bc(c, ent=0.0, vf=0.0)

    def check(got, p, b, rel):
        want = p.double() + bc_coef * b.double()
        bound = rel * float(p.abs().max()) + 1e-9 + bc_coef * (rel * float(b.abs().max()) + 1e-9)
        err = float((got.double() - want).abs().max())
        print(f"err {err:.3e} bound {bound:.3e}")
        assert err <= bound, (err, bound)

    check(dh, pdh, bdh, 2e-5)
    for g, p, b in zip(grads, pgrads, bgrads):
        check(g, p, b, 1e-4)


# ------------------------------------------------------------------ raw ABI
def _raw(c, norm, bc_coef=0.7, ldh=None, **over):
    """The entry point itself, every output between guard bands (tests/gemm_helpers.py's
    allocator); latents with row stride ldh.  -> (rc, slabs, (blocks, PG))."""
    from voxnav import _native
    lib = _native.load()
    M, F, A = c["M"], c["F"], c["A"]
    ldh = F if ldh is None else ldh
    PG = A * F + A + F + 1
    n1, n2 = C.c_int64(), C.c_int64()
    assert lib.vn_ppo_bc_loss_part_floats(M, F, A, C.byref(n1), C.byref(n2)) == 0
    nb = -(-M // 128)
    assert (n1.value, n2.value) == (nb * PG, nb * 7 + 64)            # the restated sizes
    S = lambda n: gh.Slab(DEV, 1, 1, n)  # noqa: E731
    s = dict(hp=gh.Slab(DEV, 1, M, F, ld=max(ldh, F)).put(c["h"][0]),
             hv=gh.Slab(DEV, 1, M, F, ld=max(ldh, F)).put(c["h"][1]),
             dhp=gh.Slab(DEV, 1, M, F), dhv=gh.Slab(DEV, 1, M, F), gh=S(PG), stats=S(18), adv_sums=S(256),
             part=S(n1.value), spart=S(2 * n2.value))
    an, vn = c["an"], c["vn"]
    t = dict(wa=an.weight.detach().contiguous(), ba=an.bias.detach(), wv=vn.weight.detach().contiguous(),
             bv=vn.bias.detach(), src=c["src"], act=c["act"], adv=c["adv"], olp=c["olp"], ret=c["ret"], lab=c["lab"],
             wgt=c["wgt"])
    ptr = {k: v.ptr for k, v in s.items()}
    ptr.update({k: (0 if v is None else v.data_ptr()) for k, v in t.items()})
    a = dict(M=M, F=F, A=A, ldh=ldh)
    for k, v in over.items():
        if k in a:
            a[k] = v
        else:
            ptr[k] = v
    p = lambda k: C.c_void_p(ptr[k]) if ptr[k] else None  # noqa: E731
    fn = lib.vn_ppo_bc_loss_set if c["sets"] else lib.vn_ppo_bc_loss
    rc = fn(p("hp"), p("hv"), a["ldh"], p("wa"), p("ba"), p("wv"), p("bv"), p("src"), p("act"), p("adv"), p("olp"),
            p("ret"), p("lab"), p("wgt"), a["M"], a["F"], a["A"], CLIP, ENT, VF, bc_coef, int(norm), p("dhp"),
            p("dhv"), p("gh"), p("stats"), p("adv_sums"), p("part"), p("spart"), None)
    torch.cuda.synchronize()
    return rc, s, (nb, PG)


def _written(slab, n=None):
    """No float of the slab's first n payload floats (default: all) still holds the NaN sentinel."""
    n = slab.span if n is None else n
    return bool((slab.raw[slab.off0:slab.off0 + n] != gh.SENTINEL).all().item())


# ------------------------------------------------------------------ 6. buffer hygiene (+ a padded ldh)
@FORMS
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("M,F,A", [(129, 192, 5), (33, 64, 2)])
def test_padded_rows_and_guard_bands(M, F, A, norm, sets):
    """ldh = F + 4 through the raw ABI: the latents are read with the padded stride (the padding
    holds NaN patterns), every guard band around dhp, dhv, grad_heads, stats, part, spart and
    adv_sums survives, nothing inside the documented extents is left NaN, and the results are the
    dense call's bits."""
    c = kh.case(M, F, A, True, DEV, weights="random", sets=sets)
    rc, s, (nb, PG) = _raw(c, norm, ldh=F + 4)
    assert rc == 0
    for name, slab in s.items():
        assert slab.intact(), name
    for name in ("dhp", "dhv", "gh", "stats", "part", "spart"):      # spart: the blocks' sums and the 64 counts
        assert _written(s[name]), name
    assert _written(s["adv_sums"]) == norm                           # the advantage sums: only when normalised
    dh = torch.stack([s["dhp"].mat(0), s["dhv"].mat(0)])
    g = s["gh"].mat(0)[0]
    grads = (g[:A * F].view(A, F), g[A * F:A * F + A], g[A * F + A:A * F + A + F].view(1, F), g[-1:])
    stats = s["stats"].mat(0)[0].contiguous().view(torch.float64)
    _compare((dh, grads, stats), kh.reference(c, CLIP, ENT, VF, 0.7, norm))
    d2, g2, s2 = _fused(c, norm, 0.7)
    assert torch.equal(dh, d2) and torch.equal(stats, s2) and _same(grads, g2)
    # without weights the label form counts nothing: the count words stay as they were
    rc, s, (nb, PG) = _raw(dict(c, wgt=None), norm)
    assert rc == 0 and all(slab.intact() for slab in s.values())
    assert _written(s["spart"], 2 * nb * 7)
    tail = s["spart"].raw[s["spart"].off0 + 2 * nb * 7:s["spart"].off0 + s["spart"].span]
    assert bool((tail != gh.SENTINEL).all()) == sets


# ------------------------------------------------------------------ 7. saturated heads
@FORMS
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("M,F,A", [(129, 192, 5), (33, 64, 2), (257, 256, 8)])
def test_saturated_heads(M, F, A, norm, sets):
    """Logits spanning about +-40: everything finite and within the same bounds.  Half of the
    samples are labelled with their least likely action (set form: the singleton of it, a set far
    below the top logit, cross-entropy up to ~80)."""
    c = kh.case(M, F, A, True, DEV, logit_span=40.0, weights="random", sets=sets)
    with torch.no_grad():
        z = c["h"][0] @ c["an"].weight.T + c["an"].bias
    assert 79.0 < float((z.max(-1).values - z.min(-1).values).max()) < 81.0
    rows = c["src"][:M // 2]
    low = z.argmin(-1)[:M // 2]
    c["lab"][rows] = ((torch.ones_like(low) << low) if sets else low).to(c["lab"].dtype)
    c["wgt"][rows] = 1
    got = _fused(c, norm, 1.0)
    _compare(got, kh.reference(c, CLIP, ENT, VF, 1.0, norm))
    assert float(got[2][6]) > 5.0                                    # the far-off labels were in the sum


# ------------------------------------------------------------------ 8. refusals
@FORMS
def test_refusals_leave_outputs_untouched(sets):
    M, F, A = 8, 64, 6
    c = kh.case(M, F, A, True, DEV, weights="random", sets=sets)
    from voxnav import _native
    lib = _native.load()
    outs = ("dhp", "dhv", "gh", "stats", "adv_sums", "part", "spart")

    def refused(bc_coef=0.7, **over):
        rc, s, _ = _raw(c, True, bc_coef=bc_coef, **over)
        assert rc == -1, (bc_coef, over)
        for k in outs:
            assert s[k].untouched(), (over, k)

    for name in ("hp", "hv", "wa", "ba", "wv", "bv", "act", "adv", "olp", "ret", "lab", "dhp", "dhv", "gh", "stats",
                 "adv_sums", "part", "spart"):
        refused(**{name: 0})
        assert b"NULL" in lib.vn_last_error()
    for kw in (dict(M=0), dict(M=-3), dict(A=0), dict(A=9), dict(F=32), dict(F=100), dict(F=320), dict(ldh=F - 1)):
        refused(**kw)
    for bad in (-0.5, float("nan"), float("inf"), float("-inf")):
        refused(bc_coef=bad)
        assert b"bc_coef" in lib.vn_last_error()
    n1, n2 = C.c_int64(), C.c_int64()
    for bad in ((0, F, A), (M, 0, A), (M, F, 0)):
        assert lib.vn_ppo_bc_loss_part_floats(*bad, C.byref(n1), C.byref(n2)) == -1
    for m in (1, 128, 129, 4099):
        assert lib.vn_ppo_bc_loss_part_floats(m, F, A, C.byref(n1), C.byref(n2)) == 0
        nb = -(-m // 128)
        assert (n1.value, n2.value) == (nb * (A * F + A + F + 1), nb * 7 + 64)
    # src and weight may be NULL, bc_coef may be 0; the valid calls go through
    rc, s, _ = _raw(c, True)
    assert rc == 0 and not s["dhp"].untouched()
    assert _raw(dict(c, src=None, wgt=None), True, bc_coef=0.0)[0] == 0
