"""Distance-weighted planner labels and best-set execution on the GPU:
vn_bc_loss_soft, vn_bc_loss_soft_masked, vn_ppo_bc_loss_soft and vn_ppo_bc_loss_soft_masked against the
float64 restatement (tests/bc_soft_helpers.py) at tests/test_bc_set_gpu.py's shapes and tolerances,
their identities and refusals, vn_dagger_mix_best exactly, the collectors' ``labels="soft"`` /
``execute="best"`` against the set-mode collector and the CPU oracle's replay, the learners against
the restatement, and a short warm start and kickstart.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bc_helpers as bh  # noqa: E402
import bc_soft_helpers as so  # noqa: E402
import kickstart_helpers as kh  # noqa: E402
import masked_imitate_helpers as mi  # noqa: E402
import route_dists_helpers as rd  # noqa: E402
from helpers import product_room_set  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLIP, BC_COEF = 0.2, 0.7
ENTRIES = ["bc", "bc_masked", "ppo", "ppo_masked"]
TAUS = [1e-30, 0.05, 1.0, 8.0, 1e30]


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


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. the four entries
# tests/test_bc_set_gpu.py's shapes: the 4-sample pass, the 128-sample block, more than 64 count blocks' worth
BC_M = [1, 3, 4, 5, 127, 128, 129, 4099]
# (gather through src, weights, ent_coef, vf_coef)
BC_MODES = [(False, None, 0.01, 0.5), (True, "random", 0.0, 0.5), (True, "zero", 0.01, 0.5),
            (False, "random", 0.01, 0.0), (True, None, 0.0, 0.5), (False, "zero", 0.0, 0.5)]


def _case(M, F, A, gather, weights, seed=0, **kw):
    """``kickstart_helpers.case`` (heads, latents, src, PPO buffers, returns, weights) plus distance
    rows with ldd = A + 2 and poisoned padding, and mask bytes."""
    c = kh.case(M, F, A, gather, DEV, seed=seed, weights=weights, **kw)
    rng = np.random.default_rng(7000 * M + 10 * F + A + seed)
    R = c["ret"].numel()
    c["dists"] = torch.as_tensor(so.random_dists(rng, R, A), device=DEV)
    c["mask"] = torch.as_tensor(mi.random_masks(rng, (R,), A), device=DEV)
    return c


def _fused(entry, c, tau, ent, vf, norm=False, bc_coef=BC_COEF):
    from voxnav import learn_ops as lo
    heads = (c["h"], c["an"], c["vn"], c["src"])
    ppo = (c["act"], c["adv"], c["olp"], c["ret"])
    if entry == "bc":
        return lo.bc_loss_soft(*heads, c["dists"], c["wgt"], c["ret"], tau, ent, vf)
    if entry == "bc_masked":
        return lo.bc_loss_soft_masked(*heads, c["dists"], c["wgt"], c["mask"], c["ret"], tau, ent, vf)
    if entry == "ppo":
        return lo.ppo_bc_loss_soft(*heads, *ppo, c["dists"], c["wgt"], CLIP, ent, vf, bc_coef, tau, norm)
    return lo.ppo_bc_loss_soft_masked(*heads, *ppo, c["dists"], c["wgt"], c["mask"], CLIP, ent, vf, bc_coef, tau, norm)


def _reference(entry, c, tau, ent, vf, norm=False, bc_coef=BC_COEF):
    g = lambda t: None if t is None else np_(t if c["src"] is None else t[c["src"]])  # noqa: E731
    an, vn = c["an"], c["vn"]
    heads = (np_(c["h"][0]), np_(c["h"][1]), np_(an.weight), np_(an.bias), np_(vn.weight), np_(vn.bias))
    masks = g(c["mask"]) if entry.endswith("masked") else None
    if entry.startswith("bc"):
        return so.bc_soft_heads64(*heads, g(c["dists"]), g(c["wgt"]), g(c["ret"]), so.f32(tau), ent, vf, masks=masks)
    return so.kickstart_soft_heads64(*heads, g(c["act"]), g(c["adv"]), g(c["olp"]), g(c["ret"]), g(c["dists"]),
                                     g(c["wgt"]), so.f32(tau), CLIP, ent, vf, bc_coef, norm, masks=masks)


def _compare(entry, got, ref, what):
    """tests/test_bc_set_gpu.py's tolerances: latent gradients 2e-5 relative + 1e-9, head gradients
    1e-4 + 1e-9, logged sums 1e-5 + 1e-7; accuracy and labelled share exact."""
    (dh, grads, stats), (rdh, rgrads, rstats) = got, ref
    assert bool(torch.isfinite(dh).all()) and bool(torch.isfinite(stats).all()), what
    _close(np_(dh).astype(np.float64), rdh.numpy(), 2e-5, 1e-9, what + " dh")
    for name, a, b in zip(("dWa", "dba", "dwv", "dbv"), grads, rgrads):
        assert a.numel() == b.numel() and bool(torch.isfinite(a).all()), name
        _close(np_(a).astype(np.float64).reshape(-1), b.numpy().reshape(-1), 1e-4, 1e-9, f"{what} {name}")
    st, rst = np_(stats), rstats.numpy()
    ns = 4 if entry.startswith("bc") else 7
    assert st.shape == (ns + 2,)
    _close(st[:ns], rst[:ns], 1e-5, 1e-7, what + " stats")
    assert st[ns] == rst[ns] and st[ns + 1] == rst[ns + 1], (what, st[ns:], rst[ns:])


def _against_float64(entry, M, F, A, modes, k0=0):
    for i, (gather, wmode, ent, vf) in enumerate(modes):
        tau = TAUS[(k0 + i) % len(TAUS)]
        norm = entry.startswith("ppo") and M > 1 and i % 2 == 0      # (the std of one sample is NaN, as vn_ppo_loss's)
        c = _case(M, F, A, gather, wmode, seed=i)
        got = _fused(entry, c, tau, ent, vf, norm)
        again = _fused(entry, c, tau, ent, vf, norm)
        assert torch.equal(got[0], again[0]) and torch.equal(got[2], again[2]) and _same(got[1], again[1])
        what = f"{entry} M={M} F={F} A={A} gather={gather} weights={wmode} ent={ent} vf={vf} tau={tau} norm={norm}"
        _compare(entry, got, _reference(entry, c, tau, ent, vf, norm), what)
        if wmode == "zero":
            ns = 4 if entry.startswith("bc") else 7
            st = np_(got[2])
            assert st[ns - 4 if ns == 4 else 6] == 0.0 and st[ns] == 0.0 and st[ns + 1] == 0.0
            if ent == 0.0 and entry.startswith("bc"):
                assert float(got[0][0].abs().max()) == 0.0


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("A", [1, 6, 8])
@pytest.mark.parametrize("F", [64, 256])
@pytest.mark.parametrize("M", BC_M)
def test_soft_entries_match_float64(M, F, A, entry):
    """Every temperature of {1e-30, 0.05, 1, 8, 1e30} runs in every (M, F, A) case, rotated over the
    six modes.  Two calls on the same inputs give the same bits; zero weights give exact zeros in
    the KL, the accuracy and the labelled share and, with ent_coef 0, in dhp."""
    _against_float64(entry, M, F, A, BC_MODES, k0=BC_M.index(M) + A)


GRID_MODES = {"src+weights": (True, "random", 0.01, 0.5), "plain": (False, None, 0.01, 0.5)}


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("mode", list(GRID_MODES))
@pytest.mark.parametrize("A", range(1, 9))
@pytest.mark.parametrize("F", [64, 128, 192, 256])
def test_soft_entries_grid_matches_float64(F, A, mode, entry):
    """All 32 (F, A) pairs -- every (Q, AM) instantiation, both A of each AM -- at M = 129."""
    _against_float64(entry, 129, F, A, [GRID_MODES[mode]], k0=F // 64 + A)


# ------------------------------------------------------------------ 2. identities
def _singleton_dists(lab, A, rng):
    d = np.where(np.arange(A) == np_(lab)[:, None], rng.integers(1, 2000, (lab.numel(), 1)), -2).astype(np.int32)
    d[::2] = np.where(d[::2] == -2, -1, d[::2])
    return torch.as_tensor(d, device=DEV)


@pytest.mark.parametrize("M,F,A", [(129, 64, 6), (4099, 256, 8), (5, 64, 1)])
def test_singleton_rows_agree_with_bc_loss(M, F, A):
    """One positive distance per row: the outputs agree with vn_bc_loss on the corresponding labels
    within the bounds both are held to against float64; accuracy and labelled share are equal."""
    from voxnav.learn_ops import bc_loss, bc_loss_soft
    torch.manual_seed(M + F + A)
    an, vn = torch.nn.Linear(F, A).to(DEV), torch.nn.Linear(F, 1).to(DEV)
    h = torch.tanh(torch.randn((2, M, F), device=DEV))
    lab = torch.randint(0, A, (M,), device=DEV, dtype=torch.int32)
    dists = _singleton_dists(lab, A, np.random.default_rng(M))
    ret = torch.randn(M, device=DEV)
    for tau, wgt in ((0.05, None), (8.0, (torch.rand(M, device=DEV) < 0.7).to(torch.uint8))):
        dh, grads, stats = bc_loss(h, an, vn, None, lab, wgt, ret, 0.01, 0.5)
        dh2, grads2, stats2 = bc_loss_soft(h, an, vn, None, dists, wgt, ret, tau, 0.01, 0.5)
        _close(np_(dh2).astype(np.float64), np_(dh).astype(np.float64), 2e-5, 1e-9, "dh")
        for a, b in zip(grads2, grads):
            _close(np_(a).astype(np.float64).reshape(-1), np_(b).astype(np.float64).reshape(-1), 1e-4, 1e-9, "heads")
        _close(np_(stats2)[:4], np_(stats)[:4], 1e-5, 1e-7, "stats")
        assert torch.equal(stats2[4:], stats[4:])


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("M,F,A", [(129, 128, 6), (257, 256, 8)])
def test_bc_coef_zero_is_ppo_loss(M, F, A, norm, masked):
    """bc_coef = 0: dhp, dhv, grad_heads and stats[0..5] are vn_ppo_loss's (vn_ppo_loss_masked's,
    with the positive distances inside the masks) as values."""
    from voxnav import learn_ops as lo
    c = _case(M, F, A, True, "random")
    heads = (c["h"], c["an"], c["vn"], c["src"], c["act"], c["adv"], c["olp"], c["ret"])
    if masked:
        c["mask"] = (c["mask"] | torch.as_tensor(so.p_bits(np_(c["dists"]), A).numpy().astype(np.uint8),
                                                 device=DEV)).contiguous()
        ref = lo.ppo_loss_masked(*heads, c["mask"], CLIP, 0.01, 0.5, norm)
    else:
        ref = lo.ppo_loss(*heads, CLIP, 0.01, 0.5, norm)
    dh, grads, stats = _fused("ppo_masked" if masked else "ppo", c, 0.5, 0.01, 0.5, norm, bc_coef=0.0)
    assert torch.equal(dh, ref[0]) and _same(grads, ref[1])
    assert torch.equal(stats[:6], ref[2]), (stats.tolist(), ref[2].tolist())


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("weights", [None, "random"], ids=["all", "weights"])
@pytest.mark.parametrize("M,F,A", [(129, 128, 6), (257, 256, 8)])
def test_zero_advantages_are_bc_loss_soft(M, F, A, weights, masked):
    """Advantages all 0, not normalised, bc_coef = 1 (masked: the taken actions inside the masks):
    the gradients are the BC call's as values, and stats[6, 7, 8] its stats[0, 4, 5]."""
    c = _case(M, F, A, True, weights, zero_adv=True)
    if masked:
        c["mask"] = (c["mask"] | (1 << c["act"]).to(torch.uint8)).contiguous()
    dh, grads, stats = _fused("ppo_masked" if masked else "ppo", c, 0.5, 0.01, 0.5, False, bc_coef=1.0)
    rdh, rgrads, rstats = _fused("bc_masked" if masked else "bc", c, 0.5, 0.01, 0.5)
    assert torch.equal(dh, rdh) and _same(grads, rgrads)
    assert torch.equal(stats[[6, 7, 8]], rstats[[0, 4, 5]]), (stats.tolist(), rstats.tolist())
    assert float(stats[0]) == 0.0


@pytest.mark.parametrize("entry", ["bc", "ppo"])
@pytest.mark.parametrize("M,F,A", [(129, 128, 6), (4099, 256, 8), (5, 64, 1), (33, 192, 3)])
def test_full_masks_give_the_unmasked_bits(M, F, A, entry):
    c = _case(M, F, A, True, "random")
    for full in (0xFF, (1 << A) - 1):
        c["mask"] = torch.full_like(c["mask"], full)
        for tau in (0.05, 8.0):
            a = _fused(entry, c, tau, 0.01, 0.5, True)
            b = _fused(entry + "_masked", c, tau, 0.01, 0.5, True)
            assert torch.equal(a[0], b[0]) and _same(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("entry", ["bc_masked", "ppo_masked"])
def test_a_masked_positive_distance_keeps_its_support(entry):
    """Masks that allow one action only: every action with a positive distance of a labelled sample
    (and the taken action) stays in S_i and gets a gradient; the columns outside S_i are exactly 0
    in d ba's per-sample terms -- seen through M = 1 calls, where d ba is dz itself."""
    F, A = 64, 6
    hit = 0
    for seed in range(12):
        c = _case(1, F, A, False, None, seed=seed)
        c["dists"][0, :A] = torch.tensor([3, 3, 4, 5, -1, -2], dtype=torch.int32, device=DEV).roll(seed % A)
        c["mask"][0] = 1 << (seed % A)
        dh, grads, stats = _fused(entry, c, 1.0, 0.01, 0.5)
        S = (1 << (seed % A)) | int(so.p_bits(np_(c["dists"]), A)[0])
        if entry == "ppo_masked":
            S |= 1 << int(c["act"][0])
        dba = np_(grads[1])
        for j in range(A):
            if (S >> j) & 1:
                assert dba[j] != 0.0, (seed, j)
            else:
                assert dba[j] == 0.0 and float(grads[0][j].abs().max()) == 0.0, (seed, j)
                hit += 1
        _compare(entry, (dh, grads, stats), _reference(entry, c, 1.0, 0.01, 0.5), f"{entry} seed={seed}")
    assert hit > 0


# ------------------------------------------------------------------ 3. refusals through the raw ABI
def _raw(entry, over=None, M=8, F=64, A=6, ldd=8, tau=1.0):
    """The entry point itself on sentinel-filled outputs -> (rc, outputs)."""
    from voxnav import _native
    lib = _native.load()
    f = lambda *s: torch.zeros(s, device=DEV)  # noqa: E731
    R, W = 8, 320                                        # the buffers' rows and widths, whatever is asked for
    t = dict(hp=f(R, W), hv=f(R, W), wa=f(9, W), ba=f(9), wv=f(W), bv=f(1), ret=f(R), adv=f(R), olp=f(R),
             act=torch.zeros(R, dtype=torch.int32, device=DEV), dists=torch.ones((R, 8), dtype=torch.int32, device=DEV),
             mask=torch.full((R,), 63, dtype=torch.uint8, device=DEV))
    outs = dict(dhp=f(R, W) - 7, dhv=f(R, W) - 7, gh=f(9 * W + 9 + W + 1) - 7,
                stats=torch.full((9,), -7.0, dtype=torch.float64, device=DEV),
                adv_sums=torch.full((128,), -7.0, dtype=torch.float64, device=DEV), part=f(4096) - 7,
                spart=torch.full((256,), -7.0, dtype=torch.float64, device=DEV))
    t.update(outs)
    t.update(over or {})
    p = lambda k: None if t[k] is None else C.c_void_p(t[k].data_ptr())  # noqa: E731
    head = (p("hp"), p("hv"), F, p("wa"), p("ba"), p("wv"), p("bv"), None)
    mask = (p("mask"),) if entry.endswith("masked") else ()
    tail = (p("dhp"), p("dhv"), p("gh"), p("stats"))
    if entry.startswith("bc"):
        fn = lib.vn_bc_loss_soft_masked if mask else lib.vn_bc_loss_soft
        rc = fn(*head, p("dists"), ldd, None, *mask, p("ret"), M, F, A, tau, 0.0, 0.5, *tail, p("part"), p("spart"),
                None)
    else:
        fn = lib.vn_ppo_bc_loss_soft_masked if mask else lib.vn_ppo_bc_loss_soft
        rc = fn(*head, p("act"), p("adv"), p("olp"), p("ret"), p("dists"), ldd, None, *mask, M, F, A, CLIP, 0.0, 0.5,
                1.0, tau, 1, *tail, p("adv_sums"), p("part"), p("spart"), None)
    torch.cuda.synchronize()
    return rc, outs


@pytest.mark.parametrize("entry", ENTRIES)
def test_soft_entries_refuse_invalid_arguments(entry):
    from voxnav import _native
    lib = _native.load()

    def refused(**kw):
        rc, outs = _raw(entry, **kw)
        assert rc == -1, kw
        for k, v in outs.items():
            assert float(v.max()) == -7.0 and float(v.min()) == -7.0, (kw, k)       # nothing was launched

    refused(over=dict(dists=None))
    assert b"NULL" in lib.vn_last_error()
    refused(ldd=5)
    assert b"stride" in lib.vn_last_error()
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        refused(tau=tau)
        assert b"tau" in lib.vn_last_error()
    # the namesakes' refusals
    names = ["hp", "hv", "wa", "ba", "wv", "bv", "ret", "dhp", "dhv", "gh", "stats", "part", "spart"]
    names += ["mask"] if entry.endswith("masked") else []
    names += ["act", "adv", "olp", "adv_sums"] if entry.startswith("ppo") else []
    for name in names:
        refused(over={name: None})
        assert b"NULL" in lib.vn_last_error()
    for kw in (dict(M=0), dict(M=-3), dict(A=0), dict(A=9), dict(F=32), dict(F=320), dict(F=100)):
        refused(**kw)
    rc, outs = _raw(entry)
    assert rc == 0 and float(outs["dhp"].max()) != -7.0
    assert _raw(entry, ldd=6, tau=1e-30)[0] == 0 and _raw(entry, tau=1e30)[0] == 0


# ------------------------------------------------------------------ 4. vn_dagger_mix_best
def _mix_inputs(N, seed=0):
    rng = np.random.default_rng(seed)
    expert = rng.integers(0, 6, N).astype(np.int32)
    policy = rng.integers(0, 6, N).astype(np.int32)
    policy[::11] = np.resize(np.array([-1, 8, 99, 7, 6], np.int32), policy[::11].shape)
    dist = np.where(rng.random(N) < 0.2, -1, rng.integers(1, 50, N)).astype(np.int32)
    extra = rng.integers(0, 256, N) * (rng.random(N) < 0.6)
    best = np.where(dist == -1, 0, (1 << expert) | extra).astype(np.uint8)
    return policy, expert, dist, best


def _mix_best(policy, expert, dist, best, beta, seed, t, base=0, alias=False):
    from voxnav import _native
    lib = _native.load()
    N = len(policy)
    d = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    pol, ex, di, be = d(policy), d(expert), d(dist), d(best)
    out = pol if alias else torch.full((N,), -9, dtype=torch.int32, device=DEV)
    took, lw, own = (torch.full((N,), 9, dtype=torch.uint8, device=DEV) for _ in range(3))
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    rc = lib.vn_dagger_mix_best(p(pol), p(ex), p(di), p(be), N, C.c_double(beta), C.c_uint64(seed), C.c_uint64(t),
                                base, p(out), p(took), p(lw), p(own), None)
    assert rc == 0
    return np_(out), np_(took), np_(lw), np_(own)


@pytest.mark.parametrize("beta", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 4099])
def test_dagger_mix_best_is_the_restatement(N, beta):
    policy, expert, dist, best = _mix_inputs(N, seed=N)
    t, seed, base = 12345, 4242, 1000
    want = so.mix_best(policy, expert, dist, best, beta, seed, base + np.arange(N), t)
    got = _mix_best(policy, expert, dist, best, beta, seed, t, base)
    for a, b, name in zip(got, want, ("executed", "took_expert", "label_weight", "own_best")):
        np.testing.assert_array_equal(a, b, err_msg=name)
    # executed may alias policy
    al = _mix_best(policy, expert, dist, best, beta, seed, t, base, alias=True)
    for a, b in zip(al, want):
        np.testing.assert_array_equal(a, b)
    # two agent_id_base shards are one call's bits
    k = N // 2
    if k:
        lo = _mix_best(policy[:k], expert[:k], dist[:k], best[:k], beta, seed, t, base)
        hi = _mix_best(policy[k:], expert[k:], dist[k:], best[k:], beta, seed, t, base + k)
        for a, b, c in zip(lo, hi, got):
            np.testing.assert_array_equal(np.concatenate([a, b]), c)
    lab = dist != -1
    if beta == 1.0:
        assert (((best >> got[0].clip(0, 7)) & 1) == 1)[lab].all()


@pytest.mark.parametrize("beta", [0.0, 0.3, 1.0])
def test_singleton_best_sets_give_dagger_mix(beta):
    from voxnav import _native
    lib = _native.load()
    N = 4099
    policy, expert, dist, _ = _mix_inputs(N, seed=3)
    single = np.where(dist != -1, 1 << expert, 0).astype(np.uint8)
    ex, took, lw, own = _mix_best(policy, expert, dist, single, beta, 77, 5, 64)
    d = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    pol, exq, di = d(policy), d(expert), d(dist)
    out = torch.empty(N, dtype=torch.int32, device=DEV)
    tk, w = (torch.empty(N, dtype=torch.uint8, device=DEV) for _ in range(2))
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    assert lib.vn_dagger_mix(p(pol), p(exq), p(di), N, C.c_double(beta), C.c_uint64(77), C.c_uint64(5), 64, p(out),
                             p(tk), p(w), None) == 0
    np.testing.assert_array_equal(ex, np_(out))
    np.testing.assert_array_equal(lw, np_(w))
    np.testing.assert_array_equal(took, np_(tk) & (1 - own))


def test_dagger_mix_best_refuses_invalid_arguments():
    from voxnav import _native
    lib = _native.load()
    N = 8
    i32 = lambda v: torch.full((N,), v, dtype=torch.int32, device=DEV)  # noqa: E731
    u8 = lambda v: torch.full((N,), v, dtype=torch.uint8, device=DEV)  # noqa: E731
    t = dict(policy=i32(1), expert=i32(2), dist=i32(3), best=u8(4), executed=i32(-9), took=u8(9), lw=u8(9), own=u8(9))
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())  # noqa: E731

    def call(N=N, beta=0.5, **over):
        a = dict(t, **over)
        return lib.vn_dagger_mix_best(p(a["policy"]), p(a["expert"]), p(a["dist"]), p(a["best"]), N, C.c_double(beta),
                                      C.c_uint64(1), C.c_uint64(2), 0, p(a["executed"]), p(a["took"]), p(a["lw"]),
                                      p(a["own"]), None)

    for name in t:
        assert call(**{name: None}) == -1, name
        assert b"NULL" in lib.vn_last_error()
    for kw in (dict(N=0), dict(N=-1), dict(beta=-0.1), dict(beta=1.5), dict(beta=float("nan"))):
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert int(t["executed"].max()) == -9 and int(t["own"].min()) == 9             # nothing was launched
    assert call() == 0


# ------------------------------------------------------------------ 5. the collectors
ROOMS = {"box8x8x4": "box:8x8x4", "box4x4x3": "ctor:4x4x3"}       # the second: max_steps 4, episodes end inside T
T_, N_, L_ = 12, 20, 4
SAMPLE_SEED, RESET_SEED, MIX_SEED = 1234, 42, 4242


def _dagger(src, kind, beta, labels, execute="expert", masked=False):
    from voxnav.env import BatchedGridEnv
    from voxnav.imitate import DaggerCollector, MaskedDaggerCollector
    env = BatchedGridEnv(num_agents=N_, rooms=product_room_set(src), local_map_length=L_, device=DEV, seed_stride=N_)
    pol = bh.small_policy(kind == "lstm").to(DEV)
    make = MaskedDaggerCollector if masked else DaggerCollector
    return env, make(env, pol, n_steps=T_, sample_seed=SAMPLE_SEED, reset_seed=RESET_SEED, beta=beta,
                     mix_seed=MIX_SEED, labels=labels, execute=execute)


def _fields(buf):
    return [k for k in buf.__dataclass_fields__]


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("kind", ["mlp", "lstm"])
def test_soft_collector_is_the_set_collector(kind, beta, masked):
    env, col = _dagger(ROOMS["box8x8x4"], kind, beta, "soft", masked=masked)
    env2, ref_col = _dagger(ROOMS["box8x8x4"], kind, beta, "set", masked=masked)
    for _ in range(2):
        buf, ref = col.collect(), ref_col.collect()
        assert _fields(buf) == _fields(ref) and buf.own_best is None and buf.expert_dists is not None
        for name in _fields(buf):
            a, b = getattr(buf, name), getattr(ref, name)
            assert (a is None) == (b is None), name
            if a is not None:
                assert torch.equal(a, b), name
    env.close()
    env2.close()


@pytest.mark.parametrize("room", list(ROOMS))
@pytest.mark.parametrize("beta", [0.0, 1.0, 0.5])
@pytest.mark.parametrize("labels", ["set", "soft"])
def test_best_execution_against_the_oracle_replay(labels, beta, room):
    """The executed actions replayed through the CPU oracle (tests/test_bc_set_gpu.py's replay): the
    planner's rule on the oracle's state before every step gives the buffer's dists and sets;
    executed, took_expert, label_weight and own_best are the restatement's on the stored policy
    samples; at beta 1 every labelled executed action is in expert_set; at beta 0 the rollout is
    the execute="expert" collector's."""
    from test_bc_set_gpu import _replay_dists
    src = ROOMS[room]
    env, col = _dagger(src, "lstm", beta, labels, execute="best")
    buf = col.collect()
    dists, best, ended = _replay_dists(src, np_(buf.actions))
    np.testing.assert_array_equal(np_(buf.expert_dists), dists)
    np.testing.assert_array_equal(np_(buf.expert_set), best)
    assert (rd.popcount(best) > 1).any() and (ended or room != "box4x4x3")
    pa, ea, di = np_(buf.policy_actions), np_(buf.expert_actions), np_(buf.expert_dist)
    for t in range(T_):
        ex, took, lw, own = so.mix_best(pa[t], ea[t], di[t], best[t], beta, MIX_SEED, np.arange(N_), t)
        np.testing.assert_array_equal(np_(buf.actions[t]), ex)
        np.testing.assert_array_equal(np_(buf.took_expert[t]), took)
        np.testing.assert_array_equal(np_(buf.label_weight[t]), lw)
        np.testing.assert_array_equal(np_(buf.own_best[t]), own)
    lab = np_(buf.label_weight) != 0
    assert buf.own_best.dtype == torch.uint8 and 0 < int(buf.own_best.sum()) < lab.sum()
    if beta == 1.0:
        assert (((best >> np_(buf.actions)) & 1) == 1)[lab].all()
        assert (np_(buf.took_expert) == (lab & (np_(buf.own_best) == 0))).all()
    if beta == 0.0:
        env2, ref_col = _dagger(src, "lstm", 0.0, labels)
        ref = ref_col.collect()
        for name in _fields(ref):
            a, b = getattr(buf, name), getattr(ref, name)
            if b is not None:
                assert torch.equal(a, b), name
        assert ref.own_best is None
        env2.close()
    env.close()


def test_masked_best_execution_never_bumps():
    src = ROOMS["box8x8x4"]
    env, col = _dagger(src, "lstm", 1.0, "soft", execute="best", masked=True)
    for beta in (1.0, 0.5, 0.0):
        col.set_beta(beta)
        buf = col.collect()
        inside = ((buf.action_masks.long() >> buf.actions.long()) & 1) == 1
        assert bool(inside.all()) and int((buf.expert_set & ~buf.action_masks).sum()) == 0
        assert int(env.episode_totals()[3]) + int(env.state()["bump_count"].sum()) == 0
        lab = buf.label_weight != 0
        if beta == 1.0:
            assert bool(((((buf.expert_set.long() >> buf.actions.long()) & 1) == 1) | ~lab).all())
    env.close()


def test_collector_refuses_best_execution_with_action_labels():
    from voxnav.env import BatchedGridEnv
    from voxnav.imitate import DaggerCollector
    env = BatchedGridEnv(num_agents=8, rooms=product_room_set("box:8x8x4"), local_map_length=4, device=DEV)
    with pytest.raises(ValueError, match="execute='best'"):
        DaggerCollector(env, bh.small_policy(False).to(DEV), n_steps=4, labels="action", execute="best")
    env.close()


# ------------------------------------------------------------------ 6. the learners
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("recurrent", [True, False], ids=["lstm", "mlp"])
@pytest.mark.parametrize("which", ["bc", "kickstart"])
def test_soft_learners_match_restatement_gpu(which, recurrent, masked):
    """tests/test_bc_set_gpu.py's shapes (a latent width of 64: every minibatch goes through the
    fused kernel) and the CPU bounds."""
    ln, ost = so.run_soft_parity(DEV, which, recurrent, masked, arch=(32, 64))
    assert ln.fused_updates == len(ost) > 0
    assert ln.masked_fused_updates == (len(ost) if masked else 0)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("which", ["bc", "kickstart"])
def test_soft_learners_whole_rollout_takes_the_row_layout_lstm(which, masked):
    ln, ost = so.run_soft_parity(DEV, which, True, masked, T=16, N=8, batch_size=128, epochs=1, arch=(64,), lstm=256,
                                 p_start=0.05)
    assert ln.fused_updates == len(ost) == 1
    assert any(ln.__dict__.get("_rows_cache", {}).values()), "the row layout must be the path under test"


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("which", ["bc", "kickstart"])
def test_soft_learners_fallback_head_on_the_gpu(which, masked):
    """A latent width of 16 is no width of the fused loss: torch's ops and autograd on the GPU."""
    ln, ost = so.run_soft_parity(DEV, which, False, masked)
    assert ln.fused_updates == 0 and len(ost) > 0


# ------------------------------------------------------------------ 7. warm_start and kickstart
def test_warm_start_soft_best_then_kickstart(tmp_path):
    """8x8x4 box, 64 agents x 32 steps, an MLP policy [64, 64]: three warm-start iterations with
    labels="soft", execute="best" and a label_tau schedule, a checkpoint round trip, then one
    kickstart iteration on the same collector.  The KL of an untrained policy is at most ln 6 and
    must be finite; what it does over three iterations is printed, not asserted."""
    from voxnav.checkpoint import load_checkpoint, save_checkpoint
    from voxnav.env import BatchedGridEnv
    from voxnav.imitate import BCLearner, DaggerCollector, KickstartLearner, kickstart, warm_start
    N, T, iters = 64, 32, 3
    pol = bh.small_policy(False, arch=(64, 64), seed=2).to(DEV)
    env = BatchedGridEnv(num_agents=N, rooms=product_room_set("box:8x8x4"), local_map_length=4, device=DEV)
    col = DaggerCollector(env, pol, n_steps=T, labels="soft", execute="best")
    ln = BCLearner(pol, learning_rate=1e-3, n_epochs=1, batch_size=256, seed=1, labels="soft",
                   label_tau=lambda p: 0.5 + p)
    hist = warm_start(col, ln, total_timesteps=iters * N * T, beta=lambda i: 1 - 0.5 * i)
    assert len(hist) == iters and ln.fused_updates == iters * 8 and ln.label_tau == 0.5
    print([(round(h["bc_loss"], 3), round(h["accuracy"], 3), round(h["own_best_rate"], 3), round(h["expert_share"], 3))
           for h in hist])
    for h in hist:
        assert np.isfinite(h["loss"]) and 0.0 <= h["bc_loss"] <= np.log(6) + 0.5 and 0.0 <= h["accuracy"] <= 1.0
        assert 0.5 < h["labelled"] <= 1.0 and 0.0 < h["own_best_rate"] <= h["labelled"] + 1e-6
        assert h["expert_share"] <= h["labelled"] - h["own_best_rate"] + 1e-6
    assert hist[-1]["expert_share"] == 0.0
    path = save_checkpoint(tmp_path / "warm_soft.zip", pol, ln.optimizer, num_timesteps=hist[-1]["num_timesteps"])
    pol2, data = load_checkpoint(path, device=DEV)
    assert data["num_timesteps"] == iters * N * T
    for a, b in zip(pol.parameters(), pol2.parameters()):
        assert torch.equal(a, b)
    w0 = torch.cat([p.detach().reshape(-1).clone() for p in pol.parameters()])
    kl = KickstartLearner(pol, n_epochs=2, batch_size=256, seed=1, labels="soft", label_tau=0.5)
    kh_ = kickstart(col, kl, total_timesteps=N * T, bc_coef=0.5)
    assert len(kh_) == 1 and kl.fused_updates == 16 and col.beta == 0.0
    assert all(np.isfinite(kh_[0][k]) for k in ("loss", "bc_loss", "approx_kl", "accuracy", "grad_norm"))
    assert 0.0 < kh_[0]["own_best_rate"] <= 1.0 and kh_[0]["bc_coef"] == 0.5
    assert float((torch.cat([p.detach().reshape(-1) for p in pol.parameters()]) - w0).abs().max()) > 1e-5
    env.close()
