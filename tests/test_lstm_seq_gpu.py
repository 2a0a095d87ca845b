"""The learner's per-step LSTM time loops (csrc/voxnav_learn_f32.hip:
vn_lstm_seq_fwd_mfma / vn_lstm_seq_bwd_mfma, both step-kernel templates, the
weight packing and the block mapping) against float64 restatements
(tests/lstm_seq_helpers.py), through the raw ABI.

* The case table reaches every branch the entry points and kernels take
  (asserted on the CPU by tests/test_lstm_seq_helpers_cpu.py).
* Every array the ABI writes is compared -- hs, cs, the four gates, dG, dc,
  dh0 -- per LSTM and per step, against float64 with the f32 restatement of
  the reference as the yardstick of the tolerance.
* Outputs live between sentinel bands and start as NaN, inputs between NaN
  bands: an over-read reaches an output as NaN, an over-write breaks a band.
* The autograd wrapper ``lstm_seq.dual_lstm`` against float64 autograd,
  including the input gradient and the learner's own configuration (no
  gradient for h0, c0 and x).
"""
import ctypes as C
import functools

import pytest
import torch

import gemm_helpers as gh
import lstm_seq_helpers as lh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # VN_ERR_INVALID
FWD_IN = ("x", "w_ih", "w_hh", "bias", "h0", "c0")


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _lib():
    from voxnav import _native
    return _native.load()


def _p(slab):
    return None if slab is None else C.c_void_p(slab.ptr)


@functools.lru_cache(maxsize=None)
def _refs(case):
    """(inputs, float64 forward, f32 forward) of a case, computed once."""
    d = lh.make_inputs(case)
    fin = [d[k] for k in FWD_IN]
    return d, lh.lstm_ref64(*fin), lh.plain32("fwd", *fin)


class Seq:
    """One case's operands in guarded flat arrays and the two entry points."""

    def __init__(self, d):
        self.d = d
        self.n, self.D, self.H, self.L, self.B = (d[k] for k in ("n", "D", "H", "L", "B"))
        self.geo = lh.seq_geometry(self.n, self.D, self.H, self.B)
        self.inp = {k: lh.flat(DEV, d[k].numel(), d[k]) for k in ("x", "w_ih", "w_hh", "bias", "dh_out")}
        self.fwd_out = self.bwd_out = None

    # ---- forward
    def new_fwd(self, fill=True):
        n, L, B, H = self.n, self.L, self.B, self.H
        o = dict(hs=lh.flat(DEV, n * (L + 1) * B * H), cs=lh.flat(DEV, n * (L + 1) * B * H),
                 act=lh.flat(DEV, L * n * B * 4 * H), wpack=lh.flat(DEV, self.geo["fwd_floats"]))
        if fill:
            lh.view(o["hs"], n, L + 1, B, H)[:, 0] = self.d["h0"].to(DEV)
            lh.view(o["cs"], n, L + 1, B, H)[:, 0] = self.d["c0"].to(DEV)
        self.fwd_out = o
        return o

    def fwd(self, stream=None, **over):
        a = dict(x=self.inp["x"], w_ih=self.inp["w_ih"], w_hh=self.inp["w_hh"], bias=self.inp["bias"],
                 n=self.n, D=self.D, H=self.H, L=self.L, B=self.B, **self.fwd_out)
        a.update(over)
        return _lib().vn_lstm_seq_fwd_mfma(_p(a["x"]), a["D"], _p(a["w_ih"]), _p(a["w_hh"]), _p(a["bias"]),
                                           _p(a["wpack"]), _p(a["hs"]), _p(a["cs"]), _p(a["act"]), a["n"], a["L"],
                                           a["B"], a["H"], stream)

    def fwd_arrays(self):
        n, L, B, H = self.n, self.L, self.B, self.H
        o = self.fwd_out
        return (lh.view(o["hs"], n, L + 1, B, H).cpu(), lh.view(o["cs"], n, L + 1, B, H).cpu(),
                lh.view(o["act"], L, n, B, 4 * H).cpu())

    def run_fwd(self, stream=None):
        """A forward into fresh outputs, with every band and finiteness check."""
        o = self.new_fwd()
        assert self.fwd(stream) == 0
        stream_sync(stream)
        for k, s in list(o.items()) + [(k, self.inp[k]) for k in ("x", "w_ih", "w_hh", "bias")]:
            assert s.intact(), f"guard bands of {k} overwritten"
        hs, cs, act = self.fwd_arrays()
        for k, t in (("hs", hs), ("cs", cs), ("act", act), ("wpack", o["wpack"].get())):
            assert bool(torch.isfinite(t).all()), f"{k}: NaN / unwritten floats"
        assert torch.equal(lh.bits(hs[:, 0]), lh.bits(self.d["h0"])), "row 0 of hs changed"
        assert torch.equal(lh.bits(cs[:, 0]), lh.bits(self.d["c0"])), "row 0 of cs changed"
        return hs, cs, act

    # ---- backward (from the forward arrays in self.fwd_out)
    def new_bwd(self, dc_in=None):
        n, L, B, H = self.n, self.L, self.B, self.H
        self.bwd_out = dict(dG=lh.flat(DEV, n * L * B * 4 * H), dc=lh.flat(DEV, n * B * H, dc_in),
                            dh0=lh.flat(DEV, n * B * H), wpack=lh.flat(DEV, self.geo["bwd_floats"]))
        return self.bwd_out

    def bwd(self, with_dh0=True, stream=None, **over):
        a = dict(dh_out=self.inp["dh_out"], w_hh=self.inp["w_hh"], act=self.fwd_out["act"], cs=self.fwd_out["cs"],
                 n=self.n, H=self.H, L=self.L, B=self.B, **self.bwd_out)
        if not with_dh0:
            a["dh0"] = None
        a.update(over)
        return _lib().vn_lstm_seq_bwd_mfma(_p(a["dh_out"]), _p(a["w_hh"]), _p(a["wpack"]), _p(a["act"]), _p(a["cs"]),
                                           _p(a["dG"]), _p(a["dc"]), _p(a["dh0"]), a["n"], a["L"], a["B"], a["H"],
                                           stream)

    def run_bwd(self, dc_in, with_dh0, stream=None):
        n, L, B, H = self.n, self.L, self.B, self.H
        before = [lh.bits(t) for t in self.fwd_arrays()[1:]] + [lh.bits(self.inp["dh_out"].get())]
        o = self.new_bwd(dc_in)
        assert self.bwd(with_dh0, stream) == 0
        stream_sync(stream)
        for k, s in list(o.items()) + [(k, self.inp[k]) for k in ("dh_out", "w_hh")] + \
                [(k, self.fwd_out[k]) for k in ("act", "cs")]:
            assert s.intact(), f"guard bands of {k} overwritten"
        after = [lh.bits(t) for t in self.fwd_arrays()[1:]] + [lh.bits(self.inp["dh_out"].get())]
        assert all(torch.equal(a, b) for a, b in zip(before, after)), "the backward wrote cs, act or dh_out"
        dG, dc = lh.view(o["dG"], n, L, B, 4 * H).cpu(), lh.view(o["dc"], n, B, H).cpu()
        dh0 = lh.view(o["dh0"], n, B, H).cpu() if with_dh0 else None
        if not with_dh0:
            assert o["dh0"].untouched(), "dh0 written though not passed"
        for k, t in (("dG", dG), ("dc", dc), ("dh0", dh0), ("wpack", o["wpack"].get())):
            assert t is None or bool(torch.isfinite(t).all()), f"{k}: NaN / unwritten floats"
        return dG, dc, dh0


def stream_sync(stream):
    if stream is None:
        torch.cuda.synchronize()


def _check_fwd(case, got, ref, p32):
    hs, cs, act = got
    lh.assert_lstm_close(hs[:, 1:], ref[0][:, 1:], p32[0][:, 1:], f"{case} fwd: hs")
    lh.assert_lstm_close(cs[:, 1:], ref[1][:, 1:], p32[1][:, 1:], f"{case} fwd: cs")
    lh.assert_lstm_close(lh.by_lstm(act), lh.by_lstm(ref[2]), lh.by_lstm(p32[2]), f"{case} fwd: act")


def _check_bwd(case, got, ref, p32):
    lh.assert_lstm_close(got[0], ref[0], p32[0], f"{case} bwd: dG")
    lh.assert_lstm_close(lh.states(got[1]), lh.states(ref[1]), lh.states(p32[1]), f"{case} bwd: dc")
    if got[2] is not None:
        lh.assert_lstm_close(lh.states(got[2]), lh.states(ref[2]), lh.states(p32[2]), f"{case} bwd: dh0")


def _forward_backward(case, d, ref_f, p32_f, stream=None):
    """Forward twice, backward with dh0 twice and once without: every compared
    array against float64, bands, bit-stability.  Returns the kernel's arrays."""
    raw = None if stream is None else C.c_void_p(stream.cuda_stream)
    s = Seq(d)
    first = s.run_fwd(raw)
    if stream is not None:
        stream.synchronize()
    _check_fwd(case, first, ref_f, p32_f)
    again = s.run_fwd(raw)
    if stream is not None:
        stream.synchronize()
    assert all(torch.equal(lh.bits(a), lh.bits(b)) for a, b in zip(first, again)), "forward not deterministic"
    hs, cs, act = again
    bin_ = (d["dh_out"], d["dc_in"], d["w_hh"], act, cs)       # the kernel's own forward arrays
    ref_b, p32_b = lh.lstm_bwd_ref64(*bin_), lh.plain32("bwd", *bin_)
    runs = []
    for with_dh0 in (True, True, False):
        runs.append(s.run_bwd(d["dc_in"], with_dh0, raw))
        if stream is not None:
            stream.synchronize()
        _check_bwd(case, runs[-1], ref_b, p32_b)
    for k in range(3):
        assert torch.equal(lh.bits(runs[0][k]), lh.bits(runs[1][k])), "backward not deterministic"
    for k in range(2):   # dG and dc do not depend on whether dh0 is asked for
        assert torch.equal(lh.bits(runs[0][k]), lh.bits(runs[2][k])), "dG / dc differ without dh0"
    return (hs, cs, act), runs[0], ref_b


@pytest.mark.parametrize("case", list(lh.CASES))
def test_seq_loops_match_float64(case):
    d, ref_f, p32_f = _refs(case)
    _forward_backward(case, d, ref_f, p32_f)


def test_seq_loops_on_a_side_stream():
    """Case F launched on a non-default stream, synchronised by that stream only."""
    d, ref_f, p32_f = _refs("F")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(DEV)
    with torch.cuda.stream(stream):
        _forward_backward("F stream", d, ref_f, p32_f, stream)


def test_saturated_gates_stay_exact():
    """Case E with biases of +-100 on a quarter of the units: everything
    finite, gates exactly 0 / +-1 where float64 rounds to that in f32, dG
    exactly 0 where the float64 product does."""
    d = dict(lh.make_inputs("E"))
    n, H = d["n"], d["H"]
    bias = d["bias"].clone().view(n, 4, H)
    for l in range(n):
        for g in range(4):
            for u in range(0, H, 4):
                bias[l, g, u] = 100.0 if (l + g + u // 4) % 2 else -100.0
    d["bias"] = bias.view(n, 4 * H)
    d["dc_in"] = torch.randn(d["dc_in"].shape, generator=torch.Generator().manual_seed(9))
    fin = [d[k] for k in FWD_IN]
    ref_f, p32_f = lh.lstm_ref64(*fin), lh.plain32("fwd", *fin)
    (hs, cs, act), (dG, dc, dh0), ref_b = _forward_backward("E saturated", d, ref_f, p32_f)
    r32 = ref_f[2].float()
    pinned = (r32 == 0.0) | (r32.abs() == 1.0)
    assert int(pinned.sum()) >= act.numel() // 16
    assert torch.equal(act[pinned], r32[pinned])
    zero = ref_b[0].float() == 0.0
    assert int(zero.sum()) > 0 and not bool(dG[zero].any())


# ------------------------------------------------------------------ refusals
def _all_untouched(s):
    slabs = list(s.inp.values()) + list(s.fwd_out.values()) + list(s.bwd_out.values())
    torch.cuda.synchronize()
    return all(x.untouched() for x in slabs)


def test_refusals_launch_nothing():
    d = lh.make_inputs("E")
    s = Seq(d)
    s.inp = {k: lh.flat(DEV, d[k].numel()) for k in s.inp}   # nothing put: sentinel everywhere
    s.new_fwd(fill=False)
    s.new_bwd()
    bad_fwd = [dict(D=v) for v in (0, 3, 6, -4)] + [dict(H=v) for v in (0, 2, 6, -4)] + \
              [dict(L=0), dict(B=0), dict(n=0), dict(L=-1), dict(B=-1), dict(n=-1)] + \
              [{k: None} for k in ("x", "w_ih", "w_hh", "bias", "wpack", "hs", "cs", "act")]
    for over in bad_fwd:
        assert s.fwd(**over) == INVALID, over
    bad_bwd = [dict(H=v) for v in (0, 2, 6, -4)] + [dict(L=0), dict(B=0), dict(n=0)] + \
              [{k: None} for k in ("dh_out", "w_hh", "wpack", "act", "cs", "dG", "dc")]
    for over in bad_bwd:
        for with_dh0 in (True, False):
            assert s.bwd(with_dh0, **over) == INVALID, over
    assert _all_untouched(s)
    from voxnav import _native
    assert "NULL" in _native.load().vn_last_error().decode()


def test_pack_size():
    lib = _lib()
    nf, nb = C.c_int64(), C.c_int64()
    assert lib.vn_lstm_seq_pack_size(2, 80, 256, None, C.byref(nb)) == INVALID
    assert lib.vn_lstm_seq_pack_size(2, 80, 256, C.byref(nf), None) == INVALID
    for n, D, H, L, B in lh.CASES.values():
        assert lib.vn_lstm_seq_pack_size(n, D, H, C.byref(nf), C.byref(nb)) == 0
        geo = lh.seq_geometry(n, D, H, B)
        assert (nf.value, nb.value) == (geo["fwd_floats"], geo["bwd_floats"])


# ------------------------------------------------------- the autograd wrapper
def _policy(d):
    from types import SimpleNamespace
    mods = []
    for l in range(2):
        m = torch.nn.LSTM(d["D"], d["H"]).to(DEV)
        with torch.no_grad():
            m.weight_ih_l0.copy_(d["w_ih"][l])
            m.weight_hh_l0.copy_(d["w_hh"][l])
            m.bias_ih_l0.copy_(d["bias"][l])     # b_ih + b_hh = bias exactly
            m.bias_hh_l0.zero_()
        mods.append(m)
    return SimpleNamespace(lstm_actor=mods[0], lstm_critic=mods[1]), mods


def _wrapper_reference(d, dy, real=None):
    """float64 autograd through lstm_ref64 (over the real steps only when a
    [L, B] mask is given) and the entrywise bounds of every gradient: the
    comparator's bound on dG / hs carried through the weight-gradient products
    as gemm_helpers.ErrProp.tn does, on top of the products' own summation bound."""
    from voxnav.learn_ops import _splits
    n, D, H, L, B = (d[k] for k in ("n", "D", "H", "L", "B"))
    leaves = {k: d[k].double().requires_grad_() for k in FWD_IN}
    if real is None:
        hs, _, _ = lh.lstm_ref64(*leaves.values())
        loss = (hs[:, 1:] * dy.double()).sum()
    else:
        loss = 0.0
        lengths = real.sum(0).long()
        for ln in sorted(set(lengths.tolist())):
            cols = (lengths == ln).nonzero().flatten()
            hs, _, _ = lh.lstm_ref64(leaves["x"][:ln, cols], leaves["w_ih"], leaves["w_hh"], leaves["bias"],
                                     leaves["h0"][:, cols], leaves["c0"][:, cols])
            loss = loss + (hs[:, 1:] * dy.double()[:, :ln, cols]).sum()
    loss.backward()
    ref = {k: v.grad for k, v in leaves.items()}
    # the bounds, from the whole padded arrays (dG is exactly 0 on padded steps)
    fin = [d[k] for k in FWD_IN]
    zero = torch.zeros(n, B, H)
    f64, f32 = lh.lstm_ref64(*fin), lh.plain32("fwd", *fin)
    b64 = lh.lstm_bwd_ref64(dy, zero, d["w_hh"], f64[2], f64[1])
    b32 = lh.plain32("bwd", dy, zero, d["w_hh"], f32[2], f32[1])
    # hs only where it is real: a padded step's state multiplies a zero dG row
    m_hs = torch.ones(1, L + 1, B, 1, dtype=torch.float64)
    if real is not None:
        m_hs[0, 1:, :, 0] = real.double()
    e_dG, e_hs = lh.lstm_bound(b64[0], b32[0]).clone(), lh.lstm_bound(f64[0] * m_hs, f32[0] * m_hs.float()).clone()
    e_hs[:, 0] = 0.0                                        # the initial state is an input
    if real is not None:
        e_dG = e_dG * real.double().view(1, L, B, 1)        # exact zeros: 0 x finite
        assert not bool(b64[0][:, ~real.bool()].any())
    K = L * B
    Dp = -(-D // 4) * 4
    bound, e_x = {}, torch.zeros(K, D, dtype=torch.float64)
    b_dx = torch.zeros(K, D, dtype=torch.float64)
    for l in range(n):
        dz, e_dz = b64[0][l].reshape(K, 4 * H), e_dG[l].reshape(K, 4 * H)
        a_dz = dz.abs() + e_dz
        hp, e_hp = f64[0][l, :L].reshape(K, H), e_hs[l, :L].reshape(K, H)
        sp_hh = gh.tn_plan(K, _splits(K, -(-4 * H // 128) * -(-H // 128) * n))[1]
        sp_ih = gh.tn_plan(K, _splits(K, -(-4 * H // 128) * -(-Dp // 128) * n))[1]
        (_, bound["w_hh", l]), _ = gh.ErrProp.tn(dz, e_dz, a_dz, hp, e_hp, sp_hh)
        (_, bound["w_ih", l]), (_, bound["bias", l]) = gh.ErrProp.tn(dz, e_dz, a_dz, d["x"].double().reshape(K, D),
                                                                     e_x, sp_ih)
        b_dx += gh.ErrProp.dx(dz, e_dz, a_dz, d["w_ih"][l])[1]
    bound["x"] = gh.ErrProp.SLACK * (b_dx + n * gh.U * ref["x"].abs().reshape(K, D)).reshape(L, B, D)
    return ref, bound, (f64, f32, b64, b32)


def _run_wrapper(d, dy, need_inputs):
    from voxnav.lstm_seq import dual_lstm
    pol, mods = _policy(d)
    x, h0, c0 = (d[k].to(DEV).requires_grad_(need_inputs) for k in ("x", "h0", "c0"))
    oa, oc = dual_lstm(pol, x, h0, c0)
    ((oa * dy[0].to(DEV)).sum() + (oc * dy[1].to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    got = {"out": torch.stack([oa, oc]).detach().cpu()}
    for l, m in enumerate(mods):
        for k, p in (("w_ih", m.weight_ih_l0), ("w_hh", m.weight_hh_l0), ("b_ih", m.bias_ih_l0),
                     ("b_hh", m.bias_hh_l0)):
            got[k, l] = p.grad.cpu()
    for k, t in (("x", x), ("h0", h0), ("c0", c0)):
        got[k] = t.grad.cpu() if need_inputs else None
        assert need_inputs or t.grad is None
    return got


def _check_wrapper(what, d, dy, got, ref, bound, chains, need_inputs, check_out=True):
    f64, f32, b64, b32 = chains
    if check_out:
        lh.assert_lstm_close(got["out"], f64[0][:, 1:], f32[0][:, 1:], f"{what}: out")
    for l in range(2):
        assert got["w_ih", l].shape == (4 * d["H"], d["D"])
        gh.assert_within(got["w_ih", l], ref["w_ih"][l], bound["w_ih", l], f"{what}: w_ih.grad[{l}]")
        gh.assert_within(got["w_hh", l], ref["w_hh"][l], bound["w_hh", l], f"{what}: w_hh.grad[{l}]")
        for k in ("b_ih", "b_hh"):
            gh.assert_within(got[k, l], ref["bias"][l], bound["bias", l], f"{what}: {k}.grad[{l}]")
    if need_inputs:
        assert got["x"].shape == d["x"].shape
        gh.assert_within(got["x"], ref["x"], bound["x"], f"{what}: x.grad")
        lh.assert_lstm_close(lh.states(got["h0"]), lh.states(ref["h0"]), lh.states(b32[2]), f"{what}: h0.grad")
        lh.assert_lstm_close(lh.states(got["c0"]), lh.states(ref["c0"]), lh.states(b32[1]), f"{what}: c0.grad")


WRAPPER_SHAPES = {"A": lh.CASES["A"], "E": lh.CASES["E"], "D31": (2, 31, 20, 3, 37), "D1": (2, 1, 4, 2, 3)}


@pytest.mark.parametrize("name", list(WRAPPER_SHAPES))
def test_dual_lstm_wrapper_matches_float64_autograd(name):
    d = lh.make_inputs(name, WRAPPER_SHAPES[name])
    dy = d["dh_out"]
    ref, bound, chains = _wrapper_reference(d, dy)
    with_in = _run_wrapper(d, dy, True)
    _check_wrapper(f"{name} wrapper", d, dy, with_in, ref, bound, chains, True)
    # the learner's own configuration: dh0 = NULL, no dx
    without = _run_wrapper(d, dy, False)
    _check_wrapper(f"{name} wrapper, no input grads", d, dy, without, ref, bound, chains, False)
    for k in with_in:
        if without[k] is not None:
            assert torch.equal(with_in[k], without[k]), f"{k} depends on whether the inputs need gradients"


def test_dual_lstm_padded_steps_do_not_reach_the_real_ones():
    """L 6 / B 40, every column with a real length in 1..6: zero output
    gradient and x = 1e3 on the padded steps.  Every gradient equals the
    float64 reference over the real steps only; x.grad is 0 on padded steps."""
    d = lh.make_inputs("padded", (2, 12, 12, 6, 40))
    L, B = d["L"], d["B"]
    g = torch.Generator().manual_seed(77)
    lengths = torch.randint(1, L + 1, (B,), generator=g)
    lengths[0], lengths[1] = L, 1
    real = (torch.arange(L).view(L, 1) < lengths.view(1, B)).float()          # [L, B]
    d["x"] = torch.where(real.bool().unsqueeze(-1), d["x"], torch.full_like(d["x"], 1e3))
    dy = d["dh_out"] * real.view(1, L, B, 1)
    ref, bound, chains = _wrapper_reference(d, dy, real)
    got = _run_wrapper(d, dy, True)
    f64, f32, b64, b32 = chains
    # outputs: the real steps only (padded outputs are the masked losses' don't-cares)
    m = real.view(1, L, B, 1)
    lh.assert_lstm_close(got["out"] * m, f64[0][:, 1:] * m, f32[0][:, 1:] * m, "padded: out")
    _check_wrapper("padded", d, dy, got, ref, bound, chains, True, check_out=False)
    pad = ~real.bool()
    assert float(ref["x"][pad].abs().max()) == 0.0
    assert float(got["x"][pad].abs().max()) <= lh.F * lh.U * float(ref["x"].abs().max())
