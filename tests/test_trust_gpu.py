"""``target_kl``, ``clip_range_vf`` and the schedules on the GPU:

* ``vn_kl_gate`` (csrc/voxnav_trust.hip) through the raw ABI: its whole table
  against tests/trust_helpers.gate_rule, stickiness, guard bands, a side stream,
  refusals;
* ``vn_ppo_loss_vclip`` / ``vn_ppo_loss_masked_vclip`` (csrc/voxnav_vclip_loss.hip)
  against the float64 restatement over every instantiation and the sample
  tiling's edges, with test_ppo_loss_grid_gpu's comparison and tolerances, on old
  values that put a third of the samples below, inside and above the range; the
  exact boundary; ``c = inf`` and full masks bit for bit; the raw ABI;
* the learners on the fused path: a ``target_kl`` stop at a chosen minibatch
  equals the ungated learner driven over the minibatches before it, bit for bit;
  ``clip_range_vf`` against float64; one ``ppo.learn`` iteration with everything.
"""
import copy
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

import bc_helpers as bh
import gemm_helpers as gh
import trust_helpers as th
from helpers import product_room_set
from test_masked_loss_gpu import _masks, _refit_old_log_probs
from test_ppo_loss_grid_gpu import CLIP, DEV, ENT, VF, _case, _compare

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _lib():
    from voxnav import _native
    return _native.load()


# =================================================================== 1. vn_kl_gate
GUARD32, GUARD8 = 0x5A5A5A5A, 0xA5
THR = 0.03


def _gate(lib, stats, idx, thr, err, stop, skip, ran, stream=None):
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    return lib.vn_kl_gate(p(stats), idx, C.c_double(thr), p(err), p(stop), p(skip), p(ran), stream)


def test_gate_table_with_guard_bands():
    """stop in {0, 1} x kl {below, equal, above, NaN} x err {NULL, 0, nonzero} x ran
    {NULL, given}: 48 launches on words that each sit between guard words."""
    lib = _lib()
    kls = (math.nextafter(THR, 0.0), THR, math.nextafter(THR, 1.0), float("nan"))
    cases = [(s, kl, e, r) for s in (0, 1) for kl in kls for e in (None, 0, 3) for r in (False, True)]
    n = len(cases)
    words = torch.full((n, 3, 3), GUARD32, dtype=torch.int32, device=DEV)      # [case][stop, skip, err][guard, word, guard]
    rans = torch.full((n, 3), GUARD8, dtype=torch.uint8, device=DEV)
    stats = torch.full((n, 16), 7.0, dtype=torch.float64, device=DEV)
    for i, (s, kl, e, r) in enumerate(cases):
        words[i, 0, 1] = s
        words[i, 2, 1] = 0 if e is None else e
        stats[i, i % 16] = kl
    stats0 = stats.clone()
    torch.cuda.synchronize()
    for i, (s, kl, e, r) in enumerate(cases):
        rc = _gate(lib, stats[i], i % 16, THR, None if e is None else words[i, 2, 1:2], words[i, 0, 1:2],
                   words[i, 1, 1:2], rans[i, 1:2] if r else None)
        assert rc == 0, cases[i]
    torch.cuda.synchronize()
    w, rn = words.cpu(), rans.cpu()
    for i, (s, kl, e, r) in enumerate(cases):
        ran, stop, skip = th.gate_rule(s, kl, THR, e)
        assert (int(w[i, 0, 1]), int(w[i, 1, 1])) == (stop, skip), cases[i]
        assert int(rn[i, 1]) == (ran if r else GUARD8), cases[i]
        assert int(w[i, 2, 1]) == (0 if e is None else e)                       # err is only read
        assert bool((w[i, :, 0] == GUARD32).all()) and bool((w[i, :, 2] == GUARD32).all()), cases[i]
        assert int(rn[i, 0]) == GUARD8 and int(rn[i, 2]) == GUARD8, cases[i]
    assert torch.equal(stats.nan_to_num(nan=-1.0), stats0.nan_to_num(nan=-1.0))   # stats are only read


def test_gate_is_sticky_over_three_calls_on_a_side_stream():
    """below, above, below on one stop word: (ran, skip) = (1, 0), (1, 1), (0, 1) --
    the crossing minibatch is logged and not stepped, the one after it neither;
    launched on a side stream, ordered after that stream's writes of the KL."""
    lib = _lib()
    side = torch.cuda.Stream(DEV)
    stats = torch.zeros(6, dtype=torch.float64, device=DEV)
    w = torch.zeros(2, dtype=torch.int32, device=DEV)
    ran = torch.full((3,), GUARD8, dtype=torch.uint8, device=DEV)
    skips = torch.full((3,), GUARD32, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for i, kl in enumerate((0.5 * THR, 2 * THR, 0.5 * THR)):
            stats[4:5].fill_(kl)
            assert _gate(lib, stats, 4, THR, None, w[0:1], w[1:2], ran[i:i + 1], C.c_void_p(side.cuda_stream)) == 0
            skips[i:i + 1].copy_(w[1:2])
    side.synchronize()
    assert ran.tolist() == [1, 1, 0] and skips.tolist() == [0, 1, 1] and w.tolist() == [1, 1]
    # the wrapper, on the current stream, after the caller zeroes the word
    from voxnav.learn_ops import kl_gate
    w.zero_()
    kl_gate(stats, THR, w[0:1], w[1:2], ran[0:1])
    assert w.tolist() == [0, 0] and int(ran[0]) == 1


def test_gate_refusals_launch_nothing():
    lib = _lib()
    stats = torch.full((16,), 1.0, dtype=torch.float64, device=DEV)
    w = torch.full((3,), GUARD32, dtype=torch.int32, device=DEV)
    ran = torch.full((1,), GUARD8, dtype=torch.uint8, device=DEV)
    bad = [dict(stats=None), dict(stop=None), dict(skip=None), dict(idx=-1), dict(idx=16), dict(thr=0.0),
           dict(thr=-1.0), dict(thr=float("nan")), dict(thr=float("inf"))]
    for kw in bad:
        a = dict(stats=stats, idx=4, thr=THR, err=w[2:3], stop=w[0:1], skip=w[1:2], ran=ran)
        a.update(kw)
        assert _gate(lib, a["stats"], a["idx"], a["thr"], a["err"], a["stop"], a["skip"], a["ran"]) == -1, kw
        assert lib.vn_last_error()
    torch.cuda.synchronize()
    assert w.tolist() == [GUARD32] * 3 and int(ran[0]) == GUARD8


# =================================================================== 2. the value-clipped losses
def _vcase(M, F, A, gather, c, seed=0):
    """test_ppo_loss_grid_gpu._case plus masks (old log-probs refitted to the masked
    head for the masked entry) and old values around the float64 values."""
    cs = _case(M, F, A, gather, seed=seed)
    R = cs["act"].numel()
    sel = cs["src"] if gather else torch.arange(M, device=DEV)
    cs["old"] = th.draw_old_values(cs["h"], cs["vn"].weight, cs["vn"].bias, R, sel, c, seed=M + F + A + seed)
    cm = dict(cs)
    cm["olp"] = cs["olp"].clone()
    cm["mask"] = _masks(cm, seed)
    _refit_old_log_probs(cm, cm["mask"])
    return cs, cm


def _ref(cs, c, norm):
    g = lambda t: t if cs["src"] is None else t[cs["src"]]  # noqa: E731
    an, vn = cs["an"], cs["vn"]
    mask = g(cs["mask"]) if "mask" in cs else None
    *ref, share = th.vclip_loss_reference(cs["h"], an.weight, an.bias, vn.weight, vn.bias, g(cs["act"]), g(cs["adv"]),
                                          g(cs["olp"]), g(cs["ret"]), g(cs["old"]), CLIP, c, ENT, VF, norm, mask=mask)
    return tuple(ref), share


def _call(cs, c, norm):
    from voxnav.learn_ops import ppo_loss_masked_vclip, ppo_loss_vclip
    if "mask" in cs:
        return ppo_loss_masked_vclip(cs["h"], cs["an"], cs["vn"], cs["src"], cs["act"], cs["adv"], cs["olp"],
                                     cs["ret"], cs["mask"], cs["old"], CLIP, c, ENT, VF, norm)
    return ppo_loss_vclip(cs["h"], cs["an"], cs["vn"], cs["src"], cs["act"], cs["adv"], cs["olp"], cs["ret"],
                          cs["old"], CLIP, c, ENT, VF, norm)


def _check_both(M, F, A, gather, norm, c, seed=0):
    for cs in _vcase(M, F, A, gather, c, seed):
        ref, share = _ref(cs, c, norm)
        assert min(share) >= 0.2, share            # a fifth of the samples below, inside and above the range
        _compare(_call(cs, c, norm), ref)


@pytest.mark.parametrize("A", range(1, 9))
@pytest.mark.parametrize("F", [64, 128, 192, 256])
def test_vclip_every_instantiation(F, A):
    _check_both(129, F, A, True, True, 0.05 if A % 2 else 0.5)


@pytest.mark.parametrize("c", [0.05, 0.5])
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("gather", [False, True], ids=["identity", "src"])
@pytest.mark.parametrize("M", [3, 31, 32, 33, 127, 128, 129, 257])
@pytest.mark.parametrize("F,A", [(192, 5), (64, 2)])
def test_vclip_sample_count_edges(F, A, M, gather, norm, c):
    _check_both(M, F, A, gather, norm, c, seed=int(norm))


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_vclip_exact_boundary(masked):
    """Zero value-head weights and bias 0.5: v is exactly 0.5.  With c = 0.25, old =
    0.25 (hi = v) and old = 0.75 (lo = v) take the gradient -- the bounds are inclusive.
    Above: the next float after 0.75 has lo = 0.5 + 2^-24 > v and takes none.  Below:
    the next float before 0.25 is 0.25 - 2^-26, and hi = old + c, formed in f32, falls
    halfway between 0.5 - 2^-25 and 0.5 and rounds (to even) to 0.5 = v, so that sample
    still takes the gradient; the float before it (0.25 - 2^-25, hi = 0.5 - 2^-25 < v)
    is the first that takes none.  Where none is taken the value head's gradient is
    exactly 0 and the value loss is on the bound."""
    M, F, A, c = 5, 64, 3, 0.25
    cs, cm = _vcase(M, F, A, False, c)
    cs = cm if masked else cs
    with torch.no_grad():
        cs["vn"].weight.zero_()
        cs["vn"].bias.fill_(0.5)
    ret = cs["ret"].double()
    one = np.float32
    below1 = np.nextafter(one(0.25), one(0))
    below2 = np.nextafter(below1, one(0))
    above1 = np.nextafter(one(0.75), one(1))
    assert float(below1) == 0.25 - 2.0 ** -26 and float(below2) == 0.25 - 2.0 ** -25 and float(above1) == 0.75 + 2.0 ** -24
    for old, passes, seen in ((one(0.25), True, 0.5), (one(0.75), True, 0.5), (below1, True, 0.5),
                              (below2, False, 0.5 - 2.0 ** -25), (above1, False, 0.5 + 2.0 ** -24)):
        lo, hi = float(old - one(c)), float(old + one(c))             # formed in f32
        assert (lo <= 0.5 <= hi) == passes and min(max(0.5, lo), hi) == seen, float(old)
        old = float(old)
        cs["old"] = torch.full((M,), old, device=DEV)
        dh, grads, stats = _call(cs, c, False)
        terms = 2 * VF * (seen - ret) / M
        if passes:
            assert abs(float(grads[3]) - float(terms.sum())) <= 1e-6 * float(terms.abs().sum()), old
            assert float(grads[3]) != 0.0
        else:
            assert float(grads[3]) == 0.0 and bool((grads[2] == 0).all()), old
        assert bool((dh[1] == 0).all())                        # dv wv with wv = 0
        want_vl = float(((ret - seen) ** 2).mean())
        assert abs(float(stats[1]) - want_vl) <= 1e-6 * want_vl, (old, float(stats[1]), want_vl)


@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
@pytest.mark.parametrize("M,F,A", [(129, 192, 5), (257, 128, 6), (33, 64, 2), (65, 256, 8)])
def test_vclip_infinite_range_and_full_masks_give_the_same_bits(M, F, A, norm):
    from voxnav.learn_ops import ppo_loss, ppo_loss_masked
    cs, cm = _vcase(M, F, A, True, 0.5)

    def same(x, y):
        assert torch.equal(x[0], y[0]) and torch.equal(x[2], y[2]) and all(torch.equal(a, b) for a, b in zip(x[1], y[1]))

    # c = inf: the unclipped entries
    same(_call(cs, math.inf, norm), ppo_loss(cs["h"], cs["an"], cs["vn"], cs["src"], cs["act"], cs["adv"], cs["olp"],
                                             cs["ret"], CLIP, ENT, VF, norm))
    same(_call(cm, math.inf, norm), ppo_loss_masked(cm["h"], cm["an"], cm["vn"], cm["src"], cm["act"], cm["adv"],
                                                    cm["olp"], cm["ret"], cm["mask"], CLIP, ENT, VF, norm))
    # full masks: the unmasked clipped entry
    full = dict(cs, mask=_masks(cs, full=True))
    same(_call(full, 0.5, norm), _call(cs, 0.5, norm))
    # and the clip did something at c = 0.5
    assert not torch.equal(_call(cs, 0.5, norm)[0][1], _call(cs, math.inf, norm)[0][1])


def test_vclip_two_calls_are_bit_identical():
    for cs in _vcase(257, 128, 6, True, 0.05):
        (d0, g0, s0), (d1, g1, s1) = _call(cs, 0.05, True), _call(cs, 0.05, True)
        assert torch.equal(d0, d1) and torch.equal(s0, s1) and all(torch.equal(a, b) for a, b in zip(g0, g1))


# ------------------------------------------------------------------- raw ABI
def _raw(cs, c, norm, ldh=None, **over):
    """vn_ppo_loss_vclip / vn_ppo_loss_masked_vclip themselves (the masked one when the
    case carries a mask), every output between guard bands (the raw call of
    tests/test_ppo_loss_grid_gpu.py with the old values and clip_range_vf)."""
    lib = _lib()
    masked = "mask" in cs
    M, F, A = cs["M"], cs["F"], cs["A"]
    ldh = F if ldh is None else ldh
    PG = A * F + A + F + 1
    n1, n2 = C.c_int64(), C.c_int64()
    sizes = lib.vn_ppo_loss_masked_part_floats if masked else lib.vn_ppo_loss_part_floats
    assert sizes(M, F, A, C.byref(n1), C.byref(n2)) == 0
    S = lambda n: gh.Slab(DEV, 1, 1, n)  # noqa: E731
    s = dict(hp=gh.Slab(DEV, 1, M, F, ld=max(ldh, F)).put(cs["h"][0]),
             hv=gh.Slab(DEV, 1, M, F, ld=max(ldh, F)).put(cs["h"][1]),
             dhp=gh.Slab(DEV, 1, M, F), dhv=gh.Slab(DEV, 1, M, F), gh=S(PG), stats=S(12), adv_sums=S(256),
             part=S(n1.value), spart=S(2 * n2.value))
    an, vn = cs["an"], cs["vn"]
    t = dict(wa=an.weight.detach().contiguous(), ba=an.bias.detach(), wv=vn.weight.detach().contiguous(),
             bv=vn.bias.detach(), src=cs["src"], act=cs["act"], adv=cs["adv"], olp=cs["olp"], ret=cs["ret"],
             old=cs["old"], mask=cs.get("mask"))
    ptr = {k: v.ptr for k, v in s.items()}
    ptr.update({k: (0 if v is None else v.data_ptr()) for k, v in t.items()})
    a = dict(M=M, F=F, A=A, ldh=ldh, cvf=c)
    for k, v in over.items():
        if k in a:
            a[k] = v
        else:
            ptr[k] = v
    p = lambda k: C.c_void_p(ptr[k]) if ptr[k] else None  # noqa: E731
    bufs = [p("act"), p("adv"), p("olp"), p("ret")] + ([p("mask")] if masked else []) + [p("old")]
    fn = lib.vn_ppo_loss_masked_vclip if masked else lib.vn_ppo_loss_vclip
    rc = fn(p("hp"), p("hv"), a["ldh"], p("wa"), p("ba"), p("wv"), p("bv"), p("src"), *bufs, a["M"], a["F"], a["A"],
            CLIP, a["cvf"], ENT, VF, int(norm), p("dhp"), p("dhv"), p("gh"), p("stats"), p("adv_sums"), p("part"),
            p("spart"), None)
    torch.cuda.synchronize()
    return rc, s


@pytest.mark.parametrize("M,F,A", [(129, 192, 5), (33, 64, 2)])
def test_vclip_guard_bands_and_padded_latent_rows(M, F, A):
    for cs in _vcase(M, F, A, True, 0.5):
        rc, s = _raw(cs, 0.5, True, ldh=F + 4)
        assert rc == 0
        for name, slab in s.items():
            assert slab.intact(), name
        dh = torch.stack([s["dhp"].mat(0), s["dhv"].mat(0)])
        g = s["gh"].mat(0)[0]
        grads = (g[:A * F].view(A, F), g[A * F:A * F + A], g[A * F + A:A * F + A + F].view(1, F), g[-1:])
        stats = s["stats"].mat(0)[0].contiguous().view(torch.float64)
        _compare((dh, grads, stats), _ref(cs, 0.5, True)[0])
        d2, g2, s2 = _call(cs, 0.5, True)
        assert torch.equal(dh, d2) and torch.equal(stats, s2) and all(torch.equal(a, b) for a, b in zip(grads, g2))


def test_vclip_refusals_leave_outputs_untouched():
    M, F, A = 8, 64, 6
    lib = _lib()
    outs = ("dhp", "dhv", "gh", "stats", "adv_sums", "part", "spart")
    for cs in _vcase(M, F, A, True, 0.5):
        def refused(**over):
            rc, s = _raw(cs, 0.5, True, **over)
            assert rc == -1, over
            for k in outs:
                assert s[k].untouched(), (over, k)

        names = ["hp", "hv", "wa", "ba", "wv", "bv", "act", "adv", "olp", "ret", "old", "dhp", "dhv", "gh", "stats",
                 "adv_sums", "part", "spart"] + (["mask"] if "mask" in cs else [])
        for name in names:
            refused(**{name: 0})
            assert b"NULL" in lib.vn_last_error()
        for kw in (dict(M=0), dict(M=-3), dict(A=0), dict(A=9), dict(F=32), dict(F=100), dict(F=320),
                   dict(ldh=F - 1), dict(cvf=0.0), dict(cvf=-0.5), dict(cvf=float("nan")), dict(cvf=-math.inf)):
            refused(**kw)
        assert b"clip_range_vf" in lib.vn_last_error()
        rc, s = _raw(cs, 0.5, True)                # src may be NULL; the valid call goes through
        assert rc == 0 and not s["dhp"].untouched()
        assert _raw(dict(cs, src=None), math.inf, True)[0] == 0
    from voxnav.learn_ops import ppo_loss_vclip
    with pytest.raises(ValueError, match="f32 values"):
        ppo_loss_vclip(cs["h"], cs["an"], cs["vn"], cs["src"], cs["act"], cs["adv"], cs["olp"], cs["ret"],
                       cs["old"].double(), CLIP, 0.5, ENT, VF, True)


# =================================================================== 3. the learners
N, T, BATCH, EPOCHS = 8, 16, 32, 4
PER_EPOCH = N * T // BATCH


def _policy(recurrent, seed=0):
    """LSTM 256 (the width the row-layout kernels take) + MLP [64], or an MLP [32, 64]."""
    return (bh.small_policy(True, arch=(64,), lstm=256, seed=seed) if recurrent
            else bh.small_policy(False, arch=(32, 64), seed=seed)).to(DEV)


def _rollout(pol, masks=False):
    from voxnav.collector import RolloutCollector
    from voxnav.env import BatchedGridEnv
    env = BatchedGridEnv(num_agents=N, rooms=product_room_set("box:8x8x4"), local_map_length=4, device=DEV)
    col = RolloutCollector(env, pol, n_steps=T, sample_seed=5, reset_seed=11, action_masks=masks)
    return env, col


def _orders(recurrent):
    rng = np.random.default_rng(7)
    return ([int(rng.integers(T * N)) for _ in range(EPOCHS)] if recurrent
            else [rng.permutation(T * N) for _ in range(EPOCHS)])


def _arrays(buf):
    names = ["obs", "actions", "episode_starts", "values", "log_probs", "advantages", "returns"] + \
        (["lstm_h", "lstm_c"] if buf.lstm_h is not None else [])
    return {k: getattr(buf, k).detach().cpu().numpy().copy() for k in names}


class _Calls:
    """Counts the fused entry points a learner goes through."""

    def __init__(self, monkeypatch, *names):
        from voxnav import learn_ops
        self.n = {k: 0 for k in names}
        for k in names:
            monkeypatch.setattr(learn_ops, k, self._wrap(k, getattr(learn_ops, k)))

    def _wrap(self, k, fn):
        def f(*a, **kw):
            self.n[k] += 1
            return fn(*a, **kw)
        return f


def _assert_params(pol, want, recurrent):
    """test_ppo.py's GPU bounds: 2e-5 + 1e-4 relative for the small MLP policy, its full-size
    bound 5e-5 + 1e-3 relative for the LSTM-256 policy (f32 sums over 256 units per step)."""
    from voxnav.policy import numpy_weights
    got = numpy_weights(pol)
    atol, rtol = (5e-5, 1e-3) if recurrent else (2e-5, 1e-4)
    print("largest parameter deviation from float64:", max(float(np.abs(got[k] - want[k]).max()) for k in want))
    for key in want:
        np.testing.assert_allclose(got[key], want[key], atol=atol, rtol=rtol, err_msg=key)


def _state(ln):
    out = []
    for p in ln.policy.parameters():
        s = ln.optimizer.state[p]
        out.append((p.detach(), s["exp_avg"], s["exp_avg_sq"], s["step"]))
    return out


@pytest.mark.parametrize("recurrent", [True, False], ids=["lstm", "mlp"])
def test_target_kl_stop_equals_the_ungated_learner_over_the_first_k_minibatches(recurrent, monkeypatch):
    from voxnav.policy import numpy_weights
    from voxnav.ppo import PPOLearner
    calls = _Calls(monkeypatch, "ppo_loss", "kl_gate")
    pol0 = _policy(recurrent)
    env, col = _rollout(pol0)
    try:
        buf = col.collect()
        orders = _orders(recurrent)
        w0, b = numpy_weights(pol0), _arrays(buf)
        # the dry run: the learner without target_kl, its per-minibatch logs
        ln_d = PPOLearner(copy.deepcopy(pol0), n_epochs=EPOCHS, batch_size=BATCH)
        rows, update = [], ln_d.update

        def spy(*a, **k):
            rows.append(update(*a, **k))
            return rows[-1]

        ln_d.update = spy
        ln_d.train(buf, epoch_orders=orders)
        assert calls.n == dict(ppo_loss=EPOCHS * PER_EPOCH, kl_gate=0)            # fused, and no gate without target_kl
        rows = torch.stack(rows).cpu().numpy()
        kls = rows[:, 4].tolist()
        print("dry run approx_kl per minibatch:", kls)
        k, target = th.crossing(kls, first=PER_EPOCH)                              # a minibatch of epoch >= 1
        assert max(kls[:k]) < 1.5 * target < kls[k]
        # the gated learner
        ln_g = PPOLearner(copy.deepcopy(pol0), n_epochs=EPOCHS, batch_size=BATCH, target_kl=target)
        st = ln_g.train(buf, epoch_orders=orders)
        stop_epoch = k // PER_EPOCH
        assert calls.n["kl_gate"] == (stop_epoch + 1) * PER_EPOCH == calls.n["ppo_loss"] - EPOCHS * PER_EPOCH
        if recurrent:
            assert any(ln_g.__dict__.get("_rows_cache", {}).values()), "the row layout must be the path under test"
        assert st["early_stop"] is True and st["epochs_run"] == stop_epoch + 1
        assert st["n_minibatches"] == k + 1 and st["n_updates"] == ln_g.n_updates == k
        for j, key in enumerate(("policy_gradient_loss", "value_loss", "entropy_loss", "loss", "approx_kl",
                                 "clip_fraction", "grad_norm")):
            want = float(rows[:k + 1, j].mean())
            assert abs(st[key] - want) <= 1e-12 * max(1.0, abs(want)), (key, st[key], want)
        # the ungated learner over exactly the first k minibatches of the same orders
        ln_m = PPOLearner(copy.deepcopy(pol0), n_epochs=EPOCHS, batch_size=BATCH)
        ln_m.policy.train()
        left = k
        for order in orders:
            mbs = ln_m._minibatches(order, T * N, buf.actions.device)[:left]
            if mbs:
                ln_m.update_many(buf, mbs, windows=recurrent)
            left -= len(mbs)
        for (p, m, v, s), (p2, m2, v2, s2) in zip(_state(ln_g), _state(ln_m)):
            assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2) and torch.equal(s, s2)
            assert float(s) == k
        # float64 stops at the same minibatch, and the train() after the stop applies
        # its first step with the bias correction of step k + 1
        w1, _, adam, info = th.train_reference(w0, b, orders, batch_size=BATCH, target_kl=target)
        assert info["n_steps"] == k and info["early_stop"]
        ln_g.target_kl = 1e30                     # gated still, and nothing reaches it
        ln_g.n_epochs = 1
        st2 = ln_g.train(buf, epoch_orders=orders[-1:])
        w2, _, _, _ = th.train_reference(w1, b, orders[-1:], batch_size=BATCH, adam=adam)
        assert st2["early_stop"] is False and ln_g.n_updates == k + PER_EPOCH
        assert all(float(s) == k + PER_EPOCH for _, _, _, s in _state(ln_g))
        _assert_params(ln_g.policy, w2, recurrent)
    finally:
        env.close()


@pytest.mark.parametrize("recurrent", [True, False], ids=["lstm", "mlp"])
def test_clip_range_vf_train_matches_float64(recurrent, monkeypatch):
    """Half of the rollout's values shifted by +-0.3 (they are the policy's own, so
    nothing would be clipped) and c = 0.2 -- those samples lie outside the range, the
    others inside: train() against the float64 restatement within test_ppo.py's GPU
    bounds."""
    from voxnav.policy import numpy_weights
    from voxnav.ppo import PPOLearner
    calls = _Calls(monkeypatch, "ppo_loss_vclip", "ppo_loss")
    pol = _policy(recurrent, seed=1)
    env, col = _rollout(pol)
    try:
        buf = col.collect()
        g = torch.Generator().manual_seed(3)
        shift = 0.3 * torch.sign(torch.randn(buf.values.shape, generator=g))
        shift = (shift * (torch.rand(buf.values.shape, generator=g) < 0.5)).to(DEV)
        buf = dataclasses.replace(buf, values=(buf.values + shift).contiguous())
        orders = _orders(recurrent)[:2]
        w0, b = numpy_weights(pol), _arrays(buf)
        ln = PPOLearner(pol, n_epochs=2, batch_size=BATCH, clip_range_vf=0.2)
        st = ln.train(buf, epoch_orders=orders)
        assert calls.n == dict(ppo_loss_vclip=2 * PER_EPOCH, ppo_loss=0)
        w1, rows, _, _ = th.train_reference(w0, b, orders, batch_size=BATCH, clip_range_vf=0.2)
        _assert_params(pol, w1, recurrent)
        th.assert_logged_means(st, rows)
        # the clip took part: without it float64 ends elsewhere, by more than the bound above
        wu, rows0, _, _ = th.train_reference(w0, b, orders, batch_size=BATCH)
        assert rows0[0]["value_loss"] != rows[0]["value_loss"]
        assert max(float(np.abs(wu[k] - w1[k]).max()) for k in w1) > 2e-4
    finally:
        env.close()


@pytest.mark.parametrize("masks", [False, True], ids=["plain", "masked"])
def test_learn_iterations_with_everything(masks, monkeypatch):
    """Two ``ppo.learn`` iterations of an LSTM policy with target_kl, clip_range_vf and a
    linear learning-rate schedule, on a RolloutBuffer and on a MaskedRolloutBuffer."""
    from voxnav import ppo
    from voxnav.ppo import PPOLearner
    name = "ppo_loss_masked_vclip" if masks else "ppo_loss_vclip"
    calls = _Calls(monkeypatch, name, "kl_gate")
    pol = _policy(True, seed=2)
    w0 = [p.detach().clone() for p in pol.parameters()]
    env, col = _rollout(pol, masks=masks)
    try:
        ln = PPOLearner(pol, learning_rate=lambda p: 3e-4 * p, n_epochs=2, batch_size=BATCH, target_kl=0.02,
                        clip_range_vf=0.2, action_masks=masks)
        lrs, train = [], ln.train

        def spy(*a, **k):
            lrs.append(ln.optimizer.param_groups[0]["lr"])
            return train(*a, **k)

        ln.train = spy
        hist = ppo.learn(col, ln, total_timesteps=2 * T * N)
        assert len(hist) == 2 and lrs == [3e-4 * 0.5, 0.0]
        assert calls.n[name] == calls.n["kl_gate"] == sum(h["epochs_run"] for h in hist) * PER_EPOCH > 0
        if masks:
            assert ln.masked_fused_updates == calls.n[name]
        for h in hist:
            assert all(np.isfinite(h[key]) for key in ("loss", "value_loss", "approx_kl", "grad_norm"))
            assert 1 <= h["n_minibatches"] <= h["epochs_run"] * PER_EPOCH and isinstance(h["early_stop"], bool)
        assert any(not torch.equal(p.detach(), w) for p, w in zip(pol.parameters(), w0))
    finally:
        env.close()
