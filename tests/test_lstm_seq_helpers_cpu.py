"""The yardsticks of tests/test_lstm_seq_gpu.py, checked on the CPU: the
float64 restatements (tests/lstm_seq_helpers.py) against torch's own
``nn.LSTM`` in float64 and autograd through it; the case table against the
list of kernel branches it has to reach (from ``seq_geometry``); and the
comparator against the f32 restatement with one defect at a time."""
import pytest
import torch

import lstm_seq_helpers as lh


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("case", ["D", "E", "F"])   # L 1; H 12; n_lstm 3
def test_restatements_match_torch_lstm_float64(case):
    d = lh.make_inputs(case)
    n, D, H, L, B = lh.CASES[case]
    dc_in = d["dc_in"] if d["dc_in"].any() else torch.randn(n, B, H, generator=torch.Generator().manual_seed(1))
    hs, cs, act = lh.lstm_ref64(d["x"], d["w_ih"], d["w_hh"], d["bias"], d["h0"], d["c0"])
    dG, dc_out, dh0 = lh.lstm_bwd_ref64(d["dh_out"], dc_in, d["w_hh"], act, cs)
    d_w_hh, d_w_ih, db = lh.weight_grads64(dG, hs, d["x"])
    x = d["x"].double().requires_grad_()
    dx = torch.zeros_like(x)
    for l in range(n):
        m = torch.nn.LSTM(D, H).double()
        with torch.no_grad():
            m.weight_ih_l0.copy_(d["w_ih"][l])
            m.weight_hh_l0.copy_(d["w_hh"][l])
            m.bias_ih_l0.copy_(d["bias"][l])
            m.bias_hh_l0.zero_()
        h0 = d["h0"][l:l + 1].double().requires_grad_()
        c0 = d["c0"][l:l + 1].double().requires_grad_()
        out, (hn, cn) = m(x, (h0, c0))
        assert _rel(hs[l, 1:], out.detach()) <= 1e-12
        assert _rel(cs[l, L], cn.detach()[0]) <= 1e-12
        ((out * d["dh_out"][l].double()).sum() + (cn[0] * dc_in[l].double()).sum()).backward()
        assert _rel(dh0[l], h0.grad[0]) <= 1e-12
        assert _rel(dc_out[l], c0.grad[0]) <= 1e-12
        assert _rel(d_w_hh[l], m.weight_hh_l0.grad) <= 1e-12
        assert _rel(d_w_ih[l], m.weight_ih_l0.grad) <= 1e-12
        assert _rel(db[l], m.bias_ih_l0.grad) <= 1e-12
        assert _rel(db[l], m.bias_hh_l0.grad) <= 1e-12
        dx += dG[l].reshape(L, B, 4 * H) @ d["w_ih"][l].double()
    assert _rel(dx, x.grad) <= 1e-12
    # the act / cs arrays: gates in (0, 1) / (-1, 1), c_t = f c_{t-1} + i g, h_t = o tanh c_t
    i, f, g, o = (lh.by_lstm(act)[..., s * H:(s + 1) * H] for s in range(4))
    assert _rel(cs[:, 1:], f * cs[:, :L] + i * g) <= 1e-15 and _rel(hs[:, 1:], o * torch.tanh(cs[:, 1:])) <= 1e-15
    assert torch.equal(hs[:, 0], d["h0"].double()) and torch.equal(cs[:, 0], d["c0"].double())


def test_lstm_ref64_is_differentiable_and_agrees_with_the_hand_backward():
    """float64 autograd through lstm_ref64 (what the wrapper tests compare
    against) equals lstm_bwd_ref64 and the three weight-gradient products."""
    d = lh.make_inputs("E")
    leaves = [d[k].double().requires_grad_() for k in ("x", "w_ih", "w_hh", "bias", "h0", "c0")]
    hs, cs, act = lh.lstm_ref64(*leaves)
    (hs[:, 1:] * d["dh_out"].double()).sum().backward()
    dG, dc_out, dh0 = lh.lstm_bwd_ref64(d["dh_out"], torch.zeros_like(d["dc_in"]), d["w_hh"], act.detach(),
                                        cs.detach())
    d_w_hh, d_w_ih, db = lh.weight_grads64(dG, hs.detach(), d["x"])
    for got, ref in zip((d_w_ih, d_w_hh, db, dh0, dc_out), (t.grad for t in leaves[1:])):
        assert _rel(got, ref) <= 1e-12


def test_case_table_reaches_every_branch():
    geo = {c: dict(lh.seq_geometry(n, D, H, B), n=n, D=D, H=H, L=L, B=B) for c, (n, D, H, L, B) in lh.CASES.items()}
    has = lambda pred: any(pred(g) for g in geo.values())  # noqa: E731
    assert {g["fwd_template"] for g in geo.values()} == {"42", "0"}
    assert {g["bwd_template"] for g in geo.values()} == {"128", "0"}
    assert has(lambda g: g["fwd_template"] == "42" and (g["D"], g["H"]) != (80, 256))
    assert has(lambda g: g["bwd_template"] == "0" and g["NCb"] > 32)
    for nc in (8, 16, 24):
        assert has(lambda g: g["swizzled"] and g["ncombo"] == nc), nc
    assert has(lambda g: g["swizzled"] and g["ntiles"] > 1)
    assert has(lambda g: not g["swizzled"] and g["ntiles"] > 1) and has(lambda g: not g["swizzled"] and g["UB"] > 1)
    assert {g["n"] for g in geo.values()} >= {1, 2, 3, 4}
    assert has(lambda g: g["fwd_idle_waves"] > 0) and has(lambda g: g["bwd_idle_waves"] > 0)
    assert has(lambda g: g["NCf"] < 4)
    assert {16, 17} <= {g["NCf"] for g in geo.values()}
    assert {32, 34} <= {g["NCb"] for g in geo.values()}
    assert has(lambda g: g["fwd_n_it"] > 1 and g["fwd_template"] == "0") and has(lambda g: g["bwd_n_it"] > 1)
    assert has(lambda g: g["seam_in_chunk"]) and has(lambda g: g["h_tail_from_zero"])
    assert has(lambda g: g["UB"] > 1 and g["live_units_last_block"] < lh.LQ_UNITS)
    assert has(lambda g: g["UB"] == 1 and g["live_units_last_block"] < lh.LQ_UNITS)
    assert has(lambda g: g["D"] == 4) and has(lambda g: g["H"] == 4)
    assert has(lambda g: g["B"] == 1) and has(lambda g: 1 < g["B"] < 32) and has(lambda g: g["B"] == 32)
    assert has(lambda g: g["B"] > 32 and g["B"] % 32 == 1)
    assert has(lambda g: g["L"] == 1) and has(lambda g: g["L"] > 2)
    # what the table says of single cases
    assert (geo["A"]["fwd_template"], geo["A"]["bwd_template"], geo["A"]["ncombo"], geo["A"]["ntiles"]) == \
        ("42", "128", 16, 2)
    assert (geo["B"]["fwd_template"], geo["B"]["bwd_template"], geo["B"]["NCb"], geo["B"]["ncombo"]) == \
        ("42", "0", 64, 8)
    assert (geo["C"]["fwd_template"], geo["C"]["UB"], geo["C"]["ncombo"], geo["C"]["NCb"]) == ("42", 10, 20, 160)
    assert (geo["D"]["NCf"], geo["D"]["NCb"], geo["D"]["fwd_idle_waves"], geo["D"]["bwd_idle_waves"]) == (2, 2, 2, 2)
    assert geo["E"]["seam_in_chunk"] and geo["E"]["h_tail_from_zero"]
    assert (geo["F"]["UB"], geo["F"]["live_units_last_block"], geo["F"]["ntiles"]) == (2, 4, 3)
    assert geo["G"]["NCf"] == 16 and geo["H"]["NCf"] == 17 and geo["I"]["NCb"] == 32
    assert (geo["J"]["NCb"], geo["J"]["ncombo"]) == (34, 12)
    assert (geo["K"]["ncombo"], geo["K"]["ntiles"], geo["K"]["swizzled"]) == (24, 3, True)


@pytest.mark.parametrize("ncombo,ntiles,UB", [(16, 2, 8), (8, 2, 4), (24, 3, 12), (20, 1, 10), (6, 3, 2), (1, 1, 1),
                                              (12, 1, 3)])
def test_block_mapping_is_a_bijection(ncombo, ntiles, UB):
    seen = {lh.block_of(i, ncombo, ntiles, UB) for i in range(ncombo * ntiles)}
    assert seen == {(l, ub, rt) for l in range(ncombo // UB) for ub in range(UB) for rt in range(ntiles)}


# ----------------------------------------------------- the comparator rejects
def _fwd32(d, defect=None):
    """The f32 restatement of the forward loop with one defect."""
    f32 = torch.float32
    x, w_ih, w_hh, bias = (d[k].to(f32).clone() for k in ("x", "w_ih", "w_hh", "bias"))
    n, H, L, B = d["n"], d["H"], d["L"], d["B"]
    if defect == "w_hh_last_k":
        w_hh[:, :, H - 1] = 0.0
    if defect == "bias_last_unit":
        bias[n - 1, H - 1::H] = 0.0
    hs, cs, act = [d["h0"].to(f32)], [d["c0"].to(f32)], []
    for t in range(L):
        hp = hs[-1]
        if defect == "row_from_neighbour":
            hp = hp.clone()
            hp[:, B - 1] = hp[:, B - 2]
        pre = x[t] @ w_ih.transpose(1, 2) + hp @ w_hh.transpose(1, 2) + bias.unsqueeze(1)
        if defect == "f_g_exchanged":
            pre = pre.clone()
            pre[0, :, [H, 2 * H]] = pre[0, :, [2 * H, H]]
        i, f, o = (torch.sigmoid(pre[..., s * H:(s + 1) * H]) for s in (0, 1, 3))
        g = torch.tanh(pre[..., 2 * H:3 * H])
        c = f * cs[-1] + i * g
        hs.append(o * torch.tanh(c))
        cs.append(c)
        act.append(torch.cat([i, f, g, o], dim=-1))
    return torch.stack(hs, 1), torch.stack(cs, 1), torch.stack(act, 0)


def _bwd32(d, act, cs, dc_in, defect=None):
    """The f32 restatement of the backward loop with one defect."""
    H, L = d["H"], d["L"]
    dh_out, w_hh, dc = d["dh_out"], d["w_hh"], dc_in.clone()
    dG = [None] * L
    for t in range(L - 1, -1, -1):
        rec = t < L - 1 and not (defect == "dh_rec_missing" and t == 0)
        dh = dh_out[:, t] + dG[t + 1] @ w_hh if rec else dh_out[:, t]
        if defect == "dc_not_carried" and t == 0:
            dc = torch.zeros_like(dc)
        i, f, g, o = (act[t][..., s * H:(s + 1) * H] for s in range(4))
        cp, tc = cs[:, t], torch.tanh(cs[:, t + 1])
        dcc = dc + (dh * o) * (1.0 - tc * tc)
        dG[t] = torch.cat([dcc * g * (i * (1.0 - i)), dcc * cp * (f * (1.0 - f)), dcc * i * (1.0 - g * g),
                           dh * tc * (o * (1.0 - o))], dim=-1)
        dc = dcc * f
    dh0 = dG[0] @ w_hh
    if defect == "dh_rec_missing" and L == 1:   # one step: the only recurrent product is dh0's
        dh0 = torch.zeros_like(dh0)
    return torch.stack(dG, 1), dc, dh0


def _compare_fwd(got, ref, p32):
    for k, name in enumerate(("hs", "cs")):
        lh.assert_lstm_close(got[k][:, 1:], ref[k][:, 1:], p32[k][:, 1:], name)
    lh.assert_lstm_close(lh.by_lstm(got[2]), lh.by_lstm(ref[2]), lh.by_lstm(p32[2]), "act")


def _compare_bwd(got, ref, p32):
    lh.assert_lstm_close(got[0], ref[0], p32[0], "dG")
    lh.assert_lstm_close(lh.states(got[1]), lh.states(ref[1]), lh.states(p32[1]), "dc")
    lh.assert_lstm_close(lh.states(got[2]), lh.states(ref[2]), lh.states(p32[2]), "dh0")


FWD_DEFECTS = ("w_hh_last_k", "f_g_exchanged", "row_from_neighbour", "bias_last_unit")
BWD_DEFECTS = ("dc_not_carried", "dh_rec_missing")
# case D has one row: no neighbour to take h_prev from, so that defect runs on E and F
DEFECT_CASES = [(df, c) for df in FWD_DEFECTS + BWD_DEFECTS for c in ("D", "E", "F")
                if not (df == "row_from_neighbour" and c == "D")]


def _defect_setup(case):
    d = lh.make_inputs(case)
    fin = [d[k] for k in ("x", "w_ih", "w_hh", "bias", "h0", "c0")]
    ref_f, p32_f = lh.lstm_ref64(*fin), lh.plain32("fwd", *fin)
    # the backward from f32 forward arrays (the kernel's stand-in), a non-zero dc on entry
    dc_in = torch.randn(d["dc_in"].shape, generator=torch.Generator().manual_seed(5))
    bin_ = (d["dh_out"], dc_in, d["w_hh"], p32_f[2], p32_f[1])
    return d, ref_f, p32_f, dc_in, lh.lstm_bwd_ref64(*bin_), lh.plain32("bwd", *bin_)


@pytest.mark.parametrize("case", ["D", "E", "F"])
def test_comparator_accepts_the_restatement_without_a_defect(case):
    d, ref_f, p32_f, dc_in, ref_b, p32_b = _defect_setup(case)
    _compare_fwd(_fwd32(d), ref_f, p32_f)
    _compare_bwd(_bwd32(d, p32_f[2], p32_f[1], dc_in), ref_b, p32_b)


@pytest.mark.parametrize("defect,case", DEFECT_CASES)
def test_comparator_rejects_a_defect(defect, case):
    d, ref_f, p32_f, dc_in, ref_b, p32_b = _defect_setup(case)
    with pytest.raises(AssertionError, match="beyond"):
        if defect in FWD_DEFECTS:
            _compare_fwd(_fwd32(d, defect), ref_f, p32_f)
        else:
            _compare_bwd(_bwd32(d, p32_f[2], p32_f[1], dc_in, defect), ref_b, p32_b)


def test_comparator_rejects_nan_and_a_single_wrong_entry():
    d, ref_f, p32_f, *_ = _defect_setup("E")
    for bad in (float("nan"), None):
        got = p32_f[0].clone()
        got[1, 2, 30, 11] = bad if bad is not None else got[1, 2, 30, 11] + 1e-4
        with pytest.raises(AssertionError):
            lh.assert_lstm_close(got[:, 1:], ref_f[0][:, 1:], p32_f[0][:, 1:], "hs")
