"""tests/collect_mfma_helpers.py checked on the CPU: the packed layouts against
the collector's pack functions, the decodes and what the case tables reach,
the float64 restatements against torch.nn.LSTM / torch.nn.Linear, the exact
inputs' exactness, the draw allowance of the MLP head cases, and every check of
tests/test_collect_mfma_gpu.py against defects seeded into the plain-f32
restatements (each must fail a check somewhere on the case table; the
unmodified restatement passes them all)."""
import functools

import pytest
import torch

import collect_mfma_helpers as cm
from helpers import COLLECTOR_PATHS, path_policy

F64 = torch.float64


# --------------------------------------------------------------- packed layouts
def _coded(rows, cols, mod=None):
    w = (torch.arange(rows * cols, dtype=torch.float32).reshape(rows, cols) + 1.0)
    return w if mod is None else (w % mod) - mod // 2


def test_w_cat_matches_the_collector():
    from voxnav.collector import _Weights
    pol = path_policy("P7")
    H = COLLECTOR_PATHS["P7"][0]
    with torch.no_grad():
        for m, off in ((pol.lstm_actor, 0), (pol.lstm_critic, 3)):
            m.weight_ih_l0.copy_(_coded(*m.weight_ih_l0.shape, mod=251) + off)       # small integers: exact in bf16
            m.weight_hh_l0.copy_(_coded(*m.weight_hh_l0.shape, mod=241) + off)
    w = _Weights(pol, "cpu", torch.bfloat16)
    assert w.fused
    od = pol.lstm_actor.weight_ih_l0.shape[1]
    geo = cm.lf_geometry(2, 1, H, od)
    assert (w.kx, w.Kp) == (geo["kx"], geo["Kp"]) and geo["Kp"] > geo["K"]
    w_ih = torch.stack([pol.lstm_actor.weight_ih_l0, pol.lstm_critic.weight_ih_l0]).detach()
    w_hh = torch.stack([pol.lstm_actor.weight_hh_l0, pol.lstm_critic.weight_hh_l0]).detach()
    mine = cm.w_cat_bf16(w_ih, w_hh, geo["Kp"])
    assert torch.equal(mine, w.w_cat.float())
    assert float(mine[:, :, geo["K"]:].abs().sum()) == 0.0 and float(mine[:, :, :geo["K"]].abs().min()) >= 0.0


@pytest.mark.parametrize("n,H,od", [(2, 64, 31), (1, 128, 5), (2, 256, 80), (1, 64, 16)])
def test_pack_lstm_f32(n, H, od):
    from voxnav.collector import pack_lstm_f32
    w_ih = torch.stack([_coded(4 * H, od) + 1000000 * b for b in range(n)])
    w_hh = torch.stack([-_coded(4 * H, H) - 1000000 * b for b in range(n)])
    mine = cm.pack_lstm_f32_ref(w_ih, w_hh)
    assert torch.equal(mine, pack_lstm_f32(list(w_ih), list(w_hh)))
    kx = -(-od // 16) * 16
    assert mine.shape == (n, H // 64, kx + H, 4, 64)
    assert float(mine[:, :, od:kx].abs().sum()) == 0.0 and bool((mine[:, :, :od] != 0).all())
    assert torch.equal(cm.unpack_lstm_f32(mine), cm.lstm32_wcat(w_ih, w_hh))
    # one element spelled out: [b][ub][k][g][uu] = Wcat[g H + 64 ub + uu][k]
    b, ub, k, g, uu = n - 1, H // 64 - 1, kx + 3, 2, 17
    assert float(mine[b, ub, k, g, uu]) == float(w_hh[b, g * H + 64 * ub + uu, 3])


@pytest.mark.parametrize("Nout,K", [(128, 16), (384, 80)])
def test_pack_linear_f32(Nout, K):
    from voxnav.collector import pack_linear_f32
    w = _coded(Nout, K)
    mine = cm.pack_linear_f32_ref(w)
    assert torch.equal(mine, pack_linear_f32(w)) and torch.equal(cm.unpack_linear_f32(mine), w)
    assert float(mine[Nout // 128 - 1, 5, 77]) == float(w[Nout - 128 + 77, 5])


@pytest.mark.parametrize("N,K", [(128, 16), (256, 80), (128, 48), (256, 256)])
def test_pack_mlp_head_f32(N, K):
    from voxnav.collector import pack_mlp_head_f32
    w = _coded(N, K)
    mine = cm.pack_mlp_head_f32_ref(w)
    theirs = pack_mlp_head_f32(w)          # [N/32][Kp/8][2][32][4]: the same memory, the lane index split
    assert theirs.is_contiguous() and torch.equal(mine.reshape(-1), theirs.reshape(-1))
    Kp = -(-K // 16) * 16
    un = cm.unpack_mlp_head_f32(mine)
    assert un.shape == (N, Kp) and torch.equal(un[:, :K], w) and float(un[:, K:].abs().sum()) == 0.0
    assert float(mine[1, 1, 37, 2]) == float(w[32 + 5, 8 + 4 + 2])


def test_f2bf_is_round_to_nearest_even():
    g = torch.Generator().manual_seed(5)
    t = torch.cat([torch.randn(4096, generator=g), torch.randn(4096, generator=g) * 1e-3,
                   torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -9, -1.0 - 2.0 ** -8, 0.0, 0.4375])])
    want = cm.bf16_bits(t.to(torch.bfloat16))
    assert torch.equal(cm.bf16_rne_bits(t), want)                   # torch rounds to nearest even
    assert int((cm.bf16_trunc_bits(t) != want).sum()) > 1000        # truncation is told apart
    assert cm.bf16_rne_bits(torch.tensor([1.0 + 2.0 ** -8])).item() == 0x3F80      # a tie goes to the even neighbour
    assert cm.bf16_rne_bits(torch.tensor([1.0 + 3 * 2.0 ** -8])).item() == 0x3F82


# ------------------------------------------------------------ decode and coverage
def _lstm_geos():
    out = [("bf16", k, cm.lf_geometry(*v)) for k, v in cm.BF16_CASES.items()]
    out += [("f32", k, cm.ls_geometry(*v)) for k, v in {**cm.F32_CASES, **cm.F32_MULTI}.items()]
    return out


def test_decodes_are_bijections():
    for kind, case, geo in _lstm_geos():
        n_ids = geo["grid"] if kind == "bf16" else geo["n_items"]
        assert n_ids == geo["ntiles"] * geo["ncombo"]
        cm.check_decode(cm.decode, geo["ntiles"], geo["ncombo"])
        if kind == "f32":            # the persistent walk takes every item once
            for cus in (256, 304, 8, 1):
                grid = min(n_ids, cm.ls_slots(cus))
                walked = sorted(i for b in range(grid) for i in cm.ls_walk(b, grid, n_ids))
                assert walked == list(range(n_ids))
                assert grid % 8 == 0 or grid == n_ids
    for case, row in cm.LINEAR_CASES.items():
        geo = cm.ln_geometry(*row[:4])
        assert geo["grid"] == (geo["ntiles"] * geo["ncombo"], row[3])
        cm.check_decode(cm.decode, geo["ntiles"], geo["ncombo"])
    for case, (M, _, _, nb, _, _) in cm.HEAD_CASES.items():
        geo = cm.mh_geometry(M, nb)
        assert geo["grid"] == (-(-M // 32), nb) and geo["br0"] == 2 - nb
    # the two mappings differ where the swizzle applies, and the plain one fails the XCD property there
    assert [cm.decode(i, 16, 4) for i in (0, 1, 8, 32, 33)] == [(0, 0), (1, 0), (0, 1), (8, 0), (9, 0)]
    assert [cm.decode(i, 4, 4) for i in (0, 1, 5)] == [(0, 0), (0, 1), (1, 1)]
    with pytest.raises(AssertionError):
        cm.check_decode(cm.plain_decode, 16, 4)


def test_case_tables_reach_every_branch():
    bf = {k: cm.lf_geometry(*v) for k, v in cm.BF16_CASES.items()}
    assert {g["swizzled"] for g in bf.values()} == {True, False}
    assert {g["vec_x"] for g in bf.values()} == {True, False}
    assert bf["swz8"]["ntiles"] == 8 and bf["swz8"]["ncombo"] == 1
    assert bf["swz16"]["ntiles"] == 16 and bf["swz16"]["ncombo"] == 4            # local / ncombo > 0 from id 32
    assert bf["one_row"]["Kp"] - bf["one_row"]["K"] == 56 and bf["one_row"]["tail_rows"] == 1
    assert bf["one_tile"]["ntiles"] == 1 and bf["one_tile"]["tail_rows"] == cm.LF_ROWS
    assert bf["critic"]["tail_rows"] == 1 and bf["critic"]["ublocks"] == 4 and cm.BF16_CASES["critic"][0] == 1
    assert bf["scalar31"]["kx"] - 31 == 1 and cm.BF16_CASES["scalar5"][3] < 8
    assert bf["zero_chunk"]["Kp"] - bf["zero_chunk"]["K"] >= cm.LF_KC
    assert bf["zero_chunk"]["Kp"] == -(-bf["zero_chunk"]["K"] // 64) * 64 + 64
    assert {v[0] for v in cm.BF16_CASES.values()} == {1, 2} and {v[2] for v in cm.BF16_CASES.values()} == {64, 128, 256}
    ls = {k: cm.ls_geometry(*v) for k, v in {**cm.F32_CASES, **cm.F32_MULTI}.items()}
    assert {g["swizzled"] for g in ls.values()} == {True, False}
    assert {g["vec_x"] for g in ls.values()} == {True, False} and ls["straddle"]["straddle"]
    assert not any(g["straddle"] for k, g in ls.items() if k != "straddle" and k != "smallest")
    assert cm.F32_CASES["smallest"] == (1, 1, 64, 4) and ls["one_tile"]["tail_rows"] == cm.LS_ROWS
    assert ls["tail_row"]["tail_rows"] == 1 and cm.F32_CASES["scalar5"][3] < cm.PF_KC and ls["swz8"]["ntiles"] == 8
    assert (ls["multi_plain"]["ntiles"], ls["multi_plain"]["n_items"]) == (66, 528) and not ls["multi_plain"]["swizzled"]
    assert (ls["multi_swz"]["ntiles"], ls["multi_swz"]["n_items"]) == (72, 576) and ls["multi_swz"]["swizzled"]
    assert all(g["n_items"] > cm.ls_slots(256) for g in (ls["multi_plain"], ls["multi_swz"]))     # an MI355X has 256 CUs
    assert all(g["n_items"] <= cm.ls_slots(256) for k, g in ls.items() if not k.startswith("multi"))
    ln = {k: cm.ln_geometry(*v[:4]) for k, v in cm.LINEAR_CASES.items()}
    assert {g["swizzled"] for g in ln.values()} == {True, False} and ln["swz8"]["ntiles"] == 8
    assert ln["m1k16"]["nchunks"] == 1 and {v[4] for v in cm.LINEAR_CASES.values()} == {0, 4, 12}
    assert {v[3] for v in cm.LINEAR_CASES.values()} == {1, 2}
    hc = cm.HEAD_CASES.values()
    assert {len(v[2]) for v in hc} >= {1, cm.MH_MAXL} and {v[4] for v in hc} >= {1, cm.MH_MAXA}
    assert {v[0] for v in hc} >= {1, cm.MH_R, cm.MH_R + 1} and {v[1] for v in hc} >= {16, 256}
    assert {v[5] for v in hc} == {0, 4, 12} and {v[3] for v in hc} == {1, 2}
    for kind, table in (("bf16", cm.BF16_CASES), ("f32", cm.F32_CASES)):      # the drawn starts mix both values
        for case, row in table.items():
            if row[1] > 1:
                s = cm.lstm_inputs(kind, case)["start"]
                assert 0 < float(s.sum()) < row[1], (kind, case)


# ----------------------------------------------------------------- references
@pytest.mark.parametrize("kind,case", [("f32", "scalar31"), ("bf16", "scalar5"), ("f32", "tail_row")])
def test_lstm_ref_matches_nn_lstm(kind, case):
    d = cm.lstm_inputs(kind, case)
    for start in (None, d["start"]):
        ref = cm.lstm_ref(d, start)
        for b in range(d["n"]):
            m = torch.nn.LSTM(d["od"], d["H"], batch_first=True).to(F64)
            with torch.no_grad():
                m.weight_ih_l0.copy_(d["w_ih"][b])
                m.weight_hh_l0.copy_(d["w_hh"][b])
                m.bias_ih_l0.copy_(d["bias"][b])
                m.bias_hh_l0.zero_()
                h0, c0 = d["h_in"][b].to(F64), d["c0"][b].to(F64)
                if start is not None:
                    keep = (start == 0).to(F64)[:, None]
                    c0 = c0 * keep
                    if kind == "f32":
                        h0 = h0 * keep
                _, (h1, c1) = m(d["x"].to(F64)[:, None, :], (h0[None], c0[None]))
            assert torch.allclose(ref["h"][b], h1[0], rtol=0, atol=1e-14)
            assert torch.allclose(ref["c"][b], c1[0], rtol=0, atol=1e-14)


def test_linear_and_head_refs_match_nn_linear():
    d = cm.linear_inputs("tail_row")
    for act in (False, True):
        for i, y in enumerate(cm.linear_ref(d, act)):
            m = torch.nn.Linear(d["K"], d["Nout"]).to(F64)
            with torch.no_grad():
                m.weight.copy_(d["ws"][i])
                m.bias.copy_(d["bs"][i])
                z = m(d["xs"][i].to(F64))
            assert torch.allclose(y, torch.tanh(z) if act else z, rtol=0, atol=1e-14)
    d = cm.head_inputs("m33")
    ref = cm.head_ref(d)
    hs = []
    for x, ls in zip(d["xs"], d["layers"]):
        mods = []
        for w, b in ls:
            m = torch.nn.Linear(w.shape[1], w.shape[0]).to(F64)
            with torch.no_grad():
                m.weight.copy_(w)
                m.bias.copy_(b)
            mods += [m, torch.nn.Tanh()]
        with torch.no_grad():
            hs.append(torch.nn.Sequential(*mods)(x.to(F64)))
    assert torch.allclose(ref["values"], hs[1] @ d["wv"].to(F64) + d["bv"].to(F64), rtol=0, atol=1e-14)
    assert torch.allclose(ref["logits"], hs[0] @ d["wa"].to(F64).T + d["ba"].to(F64), rtol=0, atol=1e-14)
    assert torch.allclose(ref["lsm"].exp().sum(-1), torch.ones(d["M"], dtype=F64), rtol=0, atol=1e-13)


def test_exact_inputs_are_exact():
    for kind, table in (("bf16", cm.BF16_CASES), ("f32", {**cm.F32_CASES, **cm.F32_MULTI})):
        for case in table:
            d = cm.lstm_inputs(kind, case)
            cm.assert_exact_lstm(d)
            assert torch.equal(d["c0"], d["c0"].double().float())
    for case in cm.LINEAR_CASES:
        cm.assert_exact_linear(cm.linear_inputs(case))
    bad = cm.linear_inputs("m1k16")
    bad["ws"][0][0, 0] = 1.0 / 3.0
    with pytest.raises(AssertionError):
        cm.assert_exact_linear(bad)
    # on exact data the f32 sums are the float64 sums, whatever the order
    d = cm.lstm_inputs("f32", "scalar31")
    pre32 = cm.lstm_ref(d, None, torch.float32)["pre"]
    assert torch.equal(pre32.double(), cm.lstm_ref(d, None)["pre"])


# ------------------------------------------------- the restatements under every check
@functools.lru_cache(maxsize=None)
def _lstm_case(kind, case, generic=False):
    d = cm.lstm_inputs(kind, case, generic)
    return d, cm.lstm_packed(d)


def lstm_checks(kind, case, mode, defect=None, generic=False):
    """What tests/test_collect_mfma_gpu.py checks of one LSTM launch, on the
    restatement: mode 'plain', or a masked launch with the starts 'drawn',
    'all' or 'none' (NaN in the starting rows of c_in, and of h_in for f32)."""
    d, packed = _lstm_case(kind, case, generic)
    geo = d["geo"]
    start = None if mode == "plain" else cm.starts(d, mode)
    c_in, h_in = d["c0"], d["h_in"]
    if start is not None:
        c_in = cm.poisoned(c_in, start)
        if kind == "f32":
            h_in = cm.poisoned(h_in, start)
    out = cm.lstm_plain32(d, packed, h_in, c_in, start, defect)
    cm.check_decode(out["decode"], geo["ntiles"], geo["ncombo"])
    ref = cm.lstm_ref(d, start)
    cm.check_lstm(d, ref, out, f"{kind} {case} {mode}", cm.lstm_bound(d, ref, start) if generic else None)
    if start is not None:     # bitwise the plain entry on the masked state
        hm = cm.masked_state(d["h_in"], start) if kind == "f32" else d["h_in"]
        plain = cm.lstm_plain32(d, packed, hm, cm.masked_state(d["c0"], start), None)
        for k in ("c", "h"):
            assert torch.equal(cm.bits(out[k]), cm.bits(plain[k])), f"{k}: masked entry differs from plain on masked state"


def linear_checks(case, act, defect=None, generic=False):
    d = cm.linear_inputs(case, generic)
    xb = [cm.padded_rows(x, d["ldx"]) for x in d["xs"]]
    ys = cm.linear_plain32(d, xb, [cm.pack_linear_f32_ref(w) for w in d["ws"]], act, defect)
    refs = cm.linear_ref(d, act)
    cm.check_decode(cm.plain_decode if defect == "plain_decode" else cm.decode, d["geo"]["ntiles"], d["geo"]["ncombo"])
    cm.check_linear(d, refs, ys, act, f"linear {case}", cm.linear_bounds(d, refs, act) if generic else None)


@functools.lru_cache(maxsize=None)
def _head_case(case):
    d = cm.head_inputs(case)
    return d, cm.head_ref(d), [cm.pack_mlp_head_f32_ref(w) for ls in d["layers"] for w, _ in ls]


def head_checks(case, det, draw, defect=None):
    d, ref, packed = _head_case(case)
    xb = [cm.padded_rows(x, d["ldx"]) for x in d["xs"]]
    out = cm.head_plain32(d, xb, packed, det, draw, defect)
    return cm.check_head(d, ref, out, det, draw, f"head {case}")


@pytest.mark.parametrize("kind,case", [("bf16", c) for c in cm.BF16_CASES] + [("f32", c) for c in cm.F32_CASES])
def test_lstm_restatement_passes(kind, case):
    modes = ["plain", "drawn"] + (["all", "none"] if case in (cm.BF16_ALL_NONE if kind == "bf16" else cm.F32_ALL_NONE)
                                  else [])
    for mode in modes:
        lstm_checks(kind, case, mode)


@pytest.mark.parametrize("kind,case", [("bf16", cm.BF16_GENERIC), ("f32", cm.F32_GENERIC)])
def test_lstm_generic_restatement_within_the_derived_bound(kind, case):
    for mode in ("plain", "drawn"):
        lstm_checks(kind, case, mode, generic=True)
    assert max(v for k, v in cm.SHARES.items() if k in ("c", "h")) <= 1.0


def test_linear_and_head_restatements_pass():
    for case in cm.LINEAR_CASES:
        for act in (False, True):
            linear_checks(case, act)
    for act in (False, True):
        linear_checks(cm.LINEAR_GENERIC, act, generic=True)
    for case in cm.HEAD_CASES:
        head_checks(case, True, cm.DRAWS[0])


def test_draw_allowance_holds_for_the_chosen_seeds():
    """The sampled-action cap is a condition on the data: the plain-f32 chain
    differs from the float64 draw at most DRAW_CAP times per launch, and only
    within CDF_MARGIN of a boundary, for every case and draw of the GPU file."""
    s0, t0, b0 = cm.DRAWS[0]
    s1, t1, b1 = cm.DRAWS[1]
    for case, row in cm.HEAD_CASES.items():
        if row[3] == 1:
            continue
        for draw in (cm.DRAWS[0], cm.DRAWS[1], (s1, t0, b0), (s0, t1, b0), (s0, t0, b1)):
            assert head_checks(case, False, draw) <= cm.DRAW_CAP
    # each of the three moves the uniforms
    u0 = cm.draw_uniforms(300, cm.DRAWS[0])
    for draw in ((s1, t0, b0), (s0, t1, b0), (s0, t0, b1)):
        assert (cm.draw_uniforms(300, draw) != u0).mean() > 0.9


# -------------------------------------------------------------- seeded defects
def _fails_somewhere(runs):
    failed = 0
    for fn in runs:
        try:
            fn()
        except AssertionError:
            failed += 1
    return failed


@pytest.mark.parametrize("kind,defect", [(k, df) for k in ("bf16", "f32") for df in cm.LSTM_DEFECTS
                                         if not (k == "f32" and df == "truncate")])     # the f32 entry writes no bf16
def test_lstm_checks_catch_seeded_defects(kind, defect):
    table = cm.BF16_CASES if kind == "bf16" else cm.F32_CASES
    runs, must = [], []
    for case in table:
        geo = _lstm_case(kind, case)[0]["geo"]
        for mode in ("plain", "drawn"):
            runs.append(functools.partial(lstm_checks, kind, case, mode, defect))
            if defect == "gates" or defect == "truncate":
                must.append(runs[-1])                          # every launch shows these
            elif defect == "last_row" and geo["tail_rows"] < geo["rows"]:
                must.append(runs[-1])
            elif defect == "chunk" and geo["nchunks"] > 1:
                must.append(runs[-1])
            elif defect == "pad_column" and geo["kx"] > _lstm_case(kind, case)[0]["od"]:
                must.append(runs[-1])
            elif defect == "h_mask" and mode == "drawn" and table[case][1] > 1:
                must.append(runs[-1])
            elif defect == "plain_decode" and geo["swizzled"] and geo["ncombo"] > 1:
                must.append(runs[-1])
    assert must, "the case table holds no case that can show this defect"
    assert _fails_somewhere(must) == len(must), f"{defect}: a case that must show it passed"
    assert _fails_somewhere(runs) >= len(must)


@pytest.mark.parametrize("defect", ["ldx", "last_row", "plain_decode"])
def test_linear_checks_catch_seeded_defects(defect):
    must = []
    for case, (M, K, Nout, nb, pad) in cm.LINEAR_CASES.items():
        geo = cm.ln_geometry(M, K, Nout, nb)
        hit = {"ldx": pad > 0 and M > 1, "last_row": geo["tail_rows"] < geo["rows"],
               "plain_decode": geo["swizzled"] and geo["ncombo"] > 1}[defect]
        if hit:
            must += [functools.partial(linear_checks, case, act, defect) for act in (False, True)]
    assert must and _fails_somewhere(must) == len(must)


@pytest.mark.parametrize("defect", cm.HEAD_DEFECTS)
def test_head_checks_catch_seeded_defects(defect):
    must = []
    for case, (M, K0, widths, nb, A, pad) in cm.HEAD_CASES.items():
        if defect == "ldx" and not (pad > 0 and M > 1):
            continue
        if defect == "agent_id_base":
            if nb == 2 and A > 1 and M >= 32:
                must.append(functools.partial(head_checks, case, False, cm.DRAWS[0], defect))
            continue
        must += [functools.partial(head_checks, case, det, cm.DRAWS[0], defect) for det in (True, False)]
    assert must and _fails_somewhere(must) == len(must)
