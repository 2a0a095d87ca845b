"""The yardsticks of tests/test_lstm_rows_gpu.py, checked on the CPU: the
float64 restatements of tests/lstm_rows_helpers.py against autograd and
against torch's own ``nn.LSTM`` in float64; the case table against the list of
edges it has to reach, from the shapes; every case's poisoning; and the checks
the GPU file runs, applied to the f32 restatement's own arrays in guarded CPU
buffers -- they pass as they are and fail with one defect seeded at a time."""
import functools

import pytest
import torch

import lstm_rows_helpers as lr


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def _inputs(case):
    return lr.make_inputs(case)


def _fin(d):
    return [d[k] for k in lr.FWD_IN]


@pytest.mark.parametrize("case", ["L5B97", "L3B40all"])   # interior starts at a rate; a start in every row at every step
def test_hand_backward_matches_autograd_through_the_forward(case):
    d = _inputs(case)
    L, B = d["L"], d["B"]
    w_ih, w_hh = (d[k].double().requires_grad_() for k in ("w_ih", "w_hh"))
    bias = d["bias"].double().view(2, 1, 1, lr.G4).expand(2, L, B, lr.G4).clone().requires_grad_()
    fa = dict(zip(lr.FWD_OUT, lr.rows_fwd64(d["x"], w_ih, w_hh, bias, *_fin(d)[4:])))
    (fa["hout"] * d["dh_out"].double()).sum().backward()
    dG, dw_hh, dw_ih, db = lr.rows_bwd64(*lr.bwd_args(d, {k: v.detach() for k, v in fa.items()}))
    assert _rel(dG, bias.grad) <= 1e-12
    assert _rel(dw_hh, w_hh.grad) <= 1e-12 and _rel(dw_ih, w_ih.grad) <= 1e-12
    assert _rel(db, bias.grad.sum((1, 2))) <= 1e-12
    # the per-sample bias is the plain one
    plain = lr.rows_fwd64(*_fin(d))
    assert all(torch.equal(a, b.detach()) for a, b in zip(plain, fa.values()))


def test_forward_matches_torch_lstm_float64():
    """L6B40none has no interior start: each LSTM is nn.LSTM from stored x keep."""
    d = _inputs("L6B40none")
    L = d["L"]
    assert not bool(d["eff"][1:].any())
    hout, hprev, cprev, cnew, act = lr.rows_fwd64(*_fin(d))
    h0, c0 = lr.stored_times_keep(d, "h_store")[:, 0].double(), lr.stored_times_keep(d, "c_store")[:, 0].double()
    for l in range(2):
        m = torch.nn.LSTM(lr.D, lr.H).double()
        with torch.no_grad():
            m.weight_ih_l0.copy_(d["w_ih"][l])
            m.weight_hh_l0.copy_(d["w_hh"][l])
            m.bias_ih_l0.copy_(d["bias"][l])
            m.bias_hh_l0.zero_()
            out, (hn, cn) = m(d["x"].double(), (h0[l:l + 1], c0[l:l + 1]))
        assert _rel(hout[l], out) <= 1e-12 and _rel(cnew[l, L - 1], cn[0]) <= 1e-12
    assert torch.equal(hprev[:, 0], h0) and torch.equal(cprev[:, 0], c0)
    assert torch.equal(hprev[:, 1:], hout[:, :-1]) and torch.equal(cprev[:, 1:], cnew[:, :-1])
    i, f, g, o = (act[..., s * lr.H:(s + 1) * lr.H] for s in range(4))
    assert _rel(cnew, f * cprev + i * g) <= 1e-15 and _rel(hout, o * torch.tanh(cnew)) <= 1e-15


def test_one_step_form_matches_the_loop():
    d = _inputs("L5B97")
    hout, hprev, cprev, cnew, act = lr.rows_fwd64(*_fin(d))
    a, c, h = lr.rows_step64(d["x"], hprev, cprev, d["w_ih"], d["w_hh"], d["bias"])
    assert _rel(a, act) <= 1e-14 and _rel(c, cnew) <= 1e-14 and _rel(h, hout) <= 1e-14


def test_case_table_reaches_every_edge():
    geo = {c: dict(lr.rows_geometry(L, B), L=L, B=B, p=p, start0=s0) for c, (L, B, N, p, s0) in lr.CASES.items()}
    has = lambda pred: any(pred(g) for g in geo.values())  # noqa: E731
    assert [(g["L"], g["B"]) for g in geo.values()] == [(1, 1), (2, 32), (3, 33), (4, 31), (5, 97), (4, 95), (8, 64),
                                                        (3, 40), (6, 40)]
    assert all(N >= 8 for (_, _, N, _, _) in lr.CASES.values())
    assert has(lambda g: g["L"] == 1 and g["B"] == 1 and g["handoffs"] == 0)
    assert has(lambda g: g["NT"] == 1 and g["last_tile_rows"] == 32 and g["handoffs"] == 1)
    assert has(lambda g: g["NT"] > 1 and g["last_tile_rows"] == 1)                    # a one-row tile
    assert has(lambda g: g["NT"] == 1 and 1 < g["last_tile_rows"] < 32)               # a ragged single tile
    assert has(lambda g: g["NT"] > 1 and g["NT"] % 2 == 1)                            # an odd NT
    assert has(lambda g: g["NT"] == 2 and min(g["slot_writes"]) > 2)                  # both slot parities, reused
    assert has(lambda g: g["start0"] == "zeros" and g["p"] == 0.0)                    # start[0] = 0, nothing flagged
    assert has(lambda g: g["start0"] == "zeros" and g["p"] > 0.0)
    assert has(lambda g: g["start0"] == "mixed")
    assert has(lambda g: g["p"] == 1.0)                                               # an all-start case
    assert max(g["L"] for g in geo.values()) <= 8 and max(g["B"] for g in geo.values()) <= 97
    for c, g in geo.items():
        d = _inputs(c)
        s0 = d["start"][0]
        assert {"ones": bool(s0.all()), "zeros": not bool(s0.any()),
                "mixed": bool(s0.any()) and not bool(s0.all())}[g["start0"]], c
        if g["p"] == 1.0:
            assert bool(d["start"].all())
        if g["p"] == 0.0:
            assert not bool(d["start"][1:].any())
        if 0.0 < g["p"] < 1.0 and g["L"] > 1 and g["B"] > 1:
            assert bool(d["start"][1:].any()) and not bool(d["start"][1:].all()), c


@pytest.mark.parametrize("nt", [1, 2, 3, 4])
def test_rows2_map_is_a_bijection(nt):
    seen = [lr.rows2_map(b, nt) for b in range(32 * nt)]
    assert sorted(seen) == [(ub, g) for ub in range(16) for g in range(2 * nt)]
    # block b and block b + grid / 2 (one CU) run different LSTMs of the same row tile
    for b in range(16 * nt):
        (_, g0), (_, g1) = seen[b], seen[b + 16 * nt]
        assert g0 % nt == g1 % nt and g0 // nt != g1 // nt
    if nt == 3:   # the blocks of a group do not share blockIdx mod 8
        assert len({b % 8 for b in range(32 * nt) if seen[b][1] == 0}) > 1


@pytest.mark.parametrize("case", list(lr.CASES))
def test_poisoning_is_consistent(case):
    d = _inputs(case)
    L, B, N, eff = d["L"], d["B"], d["N"], d["eff"]
    assert bool(eff[0].all()) and torch.equal(eff[1:], d["start"][1:].bool())
    assert int(d["env"].min()) >= 0 and int(d["env"].max()) < N
    tt = torch.arange(L).view(L, 1).expand(L, B)
    reads = torch.zeros(L, N, dtype=torch.bool)
    reads[tt[eff], d["env"].long()[eff]] = True
    assert torch.equal(reads, d["read"])
    for k in ("h_store", "c_store"):
        nan = torch.isnan(d[k])
        assert torch.equal(nan, (~reads).view(L, 1, N, 1).expand_as(nan)), k   # NaN exactly where no start reads
    assert torch.equal(torch.isnan(d["keep"]), ~eff)
    assert bool(((d["keep"][eff] == 0) | (d["keep"][eff] == 1)).all())
    assert not bool(reads[tt[~eff], d["env"].long()[~eff]].any())              # env of a non-start: a NaN slot
    for k in ("x", "w_ih", "w_hh", "bias", "dh_out"):
        assert bool(torch.isfinite(d[k]).all())
    for t in lr.rows_fwd64(*_fin(d)) + lr.plain32("fwd", *_fin(d)):
        assert bool(torch.isfinite(t).all())
    assert bool(torch.isfinite(lr.stored_times_keep(d, "h_store")[:, eff]).all())


# ------------------------------------------------ the checks reject a defect
def _standin(case, fwd_defect=None, bwd_defect=None):
    """The f32 restatement's arrays in guarded CPU buffers, as a finished
    16-unit forward and the backward behind it would leave them."""
    d = _inputs(case)
    b = lr.Bufs("cpu", d)
    b.put_fwd(lr.plain32("fwd", *_fin(d), **(fwd_defect or {})))
    b.put_bwd(*lr.plain32("bwd", *lr.bwd_args(d, b.fwd_arrays()), **(bwd_defect or {})))
    return b


def _all_checks(b):
    b.put_counters(16 * b.L)
    lr.check_all_fwd(b, 2, "stand-in fwd")
    b.put_counters(16 * (b.L - 1))
    lr.check_all_bwd(b, "stand-in bwd")


def _swap_outputs(b):
    for k, t in b.fwd_arrays().items():
        b.fwd[k].put(t.flip(0).reshape(1, 1, -1))


def _unwritten(b):
    lr.view(b.fwd["hout"], 2, b.L, b.B, lr.H)[1, b.L - 1, b.B - 1, lr.H - 1] = float("nan")


def _unwritten_dG(b):
    lr.interior(b.bwd["dG"]).view(2, b.L, b.B, lr.G4)[0, 0, b.B - 1, 3] = lr.SENTINEL


def _behind_last_row(b):
    s = b.fwd["cnew"]
    s.f[s.off0 + s.cols] = 0.25


def _behind_last_row_dG(b):
    s = b.bwd["dG"]
    s.f[s.off0 + s.cols] = 0.25


def _db_differs(b):
    w = lr.interior(b.bwd["db_hh"])
    w[700] = w[700] ^ 1


# name -> (forward defect, backward defect, edit of the finished buffers, what the failure says)
DEFECTS = {
    "hprev_from_two_steps_back": (dict(lag=2), None, None, r"hprev\[t\] is not hout\[t-1\]"),
    "start_does_not_cut_dh": (None, dict(cut_dh=False), None, "dG: .* beyond"),
    "start_does_not_zero_dc": (None, dict(zero_dc=False), None, "dG: .* beyond"),
    "keep_ignored": (dict(use_keep=False), None, None, "at a start is not ._store x keep"),
    "lstm_outputs_swapped": (None, None, _swap_outputs, "at a start is not|beyond"),
    "last_row_element_unwritten": (None, None, _unwritten, "hout: 1 NaN / unwritten"),
    "last_row_dG_element_unwritten": (None, None, _unwritten_dG, "dG: 1 NaN / unwritten"),
    "float_behind_last_row": (None, None, _behind_last_row, "guard bands of cnew"),
    "dG_float_behind_last_row": (None, None, _behind_last_row_dG, "guard bands of dG"),
    "db_hh_differs_from_db_ih": (None, None, _db_differs, "db_ih differs from db_hh"),
}
DEFECT_CASES = ("L8B64", "L5B97")   # interior starts, kept and dropped stored states, three or more steps


@pytest.mark.parametrize("case", DEFECT_CASES)
def test_checks_accept_the_restatement_without_a_defect(case):
    _all_checks(_standin(case))


@pytest.mark.parametrize("case", DEFECT_CASES)
@pytest.mark.parametrize("name", list(DEFECTS))
def test_checks_reject_a_defect(name, case):
    fwd_defect, bwd_defect, edit, says = DEFECTS[name]
    b = _standin(case, fwd_defect, bwd_defect)
    if edit is not None:
        edit(b)
    with pytest.raises(AssertionError, match=says):
        _all_checks(b)


def test_counter_check_rejects_a_short_count_and_a_stray_word():
    b = _standin("L5B97")
    b.put_counters(16 * b.L)
    lr.check_counters(b, 16 * b.L)
    lr.interior(b.cnt)[lr.CSTRIDE] -= 1
    with pytest.raises(AssertionError, match="counters"):
        lr.check_counters(b, 16 * b.L)
    b.put_counters(16 * b.L)
    lr.interior(b.cnt)[lr.CSTRIDE + 1] = 1
    with pytest.raises(AssertionError, match="counters"):
        lr.check_counters(b, 16 * b.L)
    b.put_counters(16 * b.L)
    b.cnt.raw[b.cnt.off0 + b.cnt.cols] = 0
    with pytest.raises(AssertionError, match="guard words"):
        lr.check_counters(b, 16 * b.L)
