"""The collector's fallback kernels alone against float64 (direct C-ABI calls).

``vn_lstm_cell`` / ``vn_lstm_cell_masked`` / ``vn_lstm_cell_bf16`` and
``vn_policy_head`` / ``vn_policy_head_bf16`` (csrc/voxnav_collect.hip) serve
every policy whose shapes the matrix-core kernels do not take (INTEGRATION.md,
"Collector paths").  The data is exact in f32 and bf16 -- gate
pre-activations, biases and latents in multiples of 1/8, head weights in
multiples of 1/16 -- so every sum is exact in any order and only the
nonlinearities round.  Bounds:

  LSTM h, c                |gpu - f64| <= 2e-6 + 2e-6 |f64|   (the project's
                           bound for exact-sum LSTM outputs; expf / tanhf here
                           are libm's)
  h_bf16                   bitwise h.to(bfloat16) (round to nearest even)
  h_store / c_store        bitwise h / c
  masked entry             bitwise the plain entry on the masked state
  head values              bitwise float32(exact sum)
  head log-probs           |gpu - f64| <= 2e-5 + 2e-5 |f64|
  deterministic action     the float64 arg-max (the data has no ties)
  sampled action           the float64 draw for the same Philox uniform, except
                           within 1e-5 of a CDF boundary, at most 2 per launch
                           (tests/test_collector_paths.py checks the seeds
                           against a numpy f32 restatement on the CPU)

Measured on an MI355X, maximum |gpu - f64| over all cases: LSTM c 3.8e-7,
h 1.7e-7 (f32 and bf16 pre-activations alike; at most 9 % of the bound);
head log-probs 5.5e-7 (3 % of the bound, at P = 4096); no sampled action
differed from the float64 draw.  The P = 4096, 8-action launch (147,456 B
of dynamic LDS a block) is accepted by the runtime.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import HEAD_CASES, HEAD_DRAWS, head_case_data, head_draws64, philox_uniform

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import voxnav
    return voxnav.load_library()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _t(a, dt=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dt).contiguous()


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _within(got, ref, atol, rtol, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    use = (err / (atol + rtol * np.abs(ref))).max()
    print(f"{what}: max err {err.max():.3g}, {use:.3f} of the bound")
    assert use <= 1.0, f"{what}: {(err > atol + rtol * np.abs(ref)).sum()} of {err.size} out of tolerance, " \
                       f"max err {err.max():.3g}"


# ------------------------------------------------------------------ LSTM cell
# (n_lstm, N, H, padding after a gx row): more than one block with a ragged
# tail, a single thread, H = 256 with N % 64 != 0, and a padded gx row; the
# last is the critic's call (n_lstm = 1, gx_row_stride = 4H)
CELL_CASES = [(2, 300, 48, 0), (1, 1, 4, 0), (2, 257, 256, 0), (1, 70, 12, 8), (1, 70, 12, 0)]
CELL_IDS = [f"B{b}-N{n}-H{h}-pad{p}" for b, n, h, p in CELL_CASES]
PAD = 1000.0          # what the padding of a gx row holds: a read of it shows at once


def _cell_data(B, N, H, pad):
    rng = np.random.default_rng(100 * N + H + pad)
    G = 4 * H
    d = dict(gx=rng.integers(-16, 17, size=(B, N, G)) / 8.0, gh=rng.integers(-16, 17, size=(B, N, G)) / 8.0,
             b_ih=rng.integers(-8, 9, size=(B, G)) / 8.0, b_hh=rng.integers(-8, 9, size=(B, G)) / 8.0,
             c0=rng.standard_normal((B, N, H)).astype(np.float32).astype(np.float64),
             start=(rng.random(N) < 0.3).astype(np.float32))
    if N == 1:
        d["start"][:] = 1.0
    assert 0 < d["start"].sum() and (N == 1 or d["start"].sum() < N)
    rows = np.full((N, B * G + pad), PAD)
    rows[:, :B * G] = d["gx"].transpose(1, 0, 2).reshape(N, B * G)       # element (b, n, j) at n*stride + b*4H + j
    d["gx_rows"] = rows
    return d


def _cell_ref(d, with_gh, masked=False):
    """(h, c) in float64: pre = gx + gh + b_ih + b_hh, torch gate order i, f, g, o."""
    B, N, G = d["gx"].shape
    H = G // 4
    keep = (d["start"] == 0)[None, :, None] if masked else np.ones((1, N, 1), bool)
    pre = d["gx"] + (np.where(keep, d["gh"], 0.0) if with_gh else 0.0) + d["b_ih"][:, None] + d["b_hh"][:, None]
    sg = lambda v: 1.0 / (1.0 + np.exp(-v))  # noqa: E731
    i, f, g, o = (pre[..., k * H:(k + 1) * H] for k in range(4))
    c1 = sg(f) * np.where(keep, d["c0"], 0.0) + sg(i) * np.tanh(g)
    return sg(o) * np.tanh(c1), c1


@pytest.mark.parametrize("B,N,H,pad", CELL_CASES, ids=CELL_IDS)
def test_lstm_cell_f32_matches_float64(lib, B, N, H, pad):
    """vn_lstm_cell and vn_lstm_cell_masked: gh NULL / given, the buffer
    copies NULL / given, the episode-start mask, the refusals."""
    d = _cell_data(B, N, H, pad)
    stride = B * 4 * H + pad
    gx, gh, bi, bh = _t(d["gx_rows"]), _t(d["gh"]), _t(d["b_ih"]), _t(d["b_hh"])
    for with_gh in (False, True):
        h_ref, c_ref = _cell_ref(d, with_gh)
        for store in (False, True):
            h, c = _nan(B, N, H), _t(d["c0"])
            hs, cs = (_nan(B, N, H), _nan(B, N, H)) if store else (None, None)
            assert lib.vn_lstm_cell(_p(gx), stride, _p(gh) if with_gh else None, _p(bi), _p(bh), _p(h), _p(c), _p(hs),
                                    _p(cs), B, N, H, None) == 0
            torch.cuda.synchronize()
            _within(c, c_ref, 2e-6, 2e-6, f"c (gh {with_gh})")
            _within(h, h_ref, 2e-6, 2e-6, f"h (gh {with_gh})")
            if store:
                assert torch.equal(hs, h) and torch.equal(cs, c)
    assert torch.equal(gx, _t(d["gx_rows"])) and torch.equal(gh, _t(d["gh"]))          # inputs not written
    # the rollout entry: c_in / gh of the unmasked state + start == the plain
    # entry on the masked state, bitwise; its inputs are not written
    start, c_in = _t(d["start"]), _t(d["c0"])
    h_m, c_m = _nan(B, N, H), _nan(B, N, H)
    assert lib.vn_lstm_cell_masked(_p(gx), stride, _p(gh), _p(bi), _p(bh), _p(c_in), _p(start), _p(h_m), _p(c_m), B, N,
                                   H, None) == 0
    keep = (d["start"] == 0)[None, :, None]
    h_p, c_p = _nan(B, N, H), _t(np.where(keep, d["c0"], 0.0))
    gh_p = _t(np.where(keep, d["gh"], 0.0))
    assert lib.vn_lstm_cell(_p(gx), stride, _p(gh_p), _p(bi), _p(bh), _p(h_p), _p(c_p), None, None, B, N, H, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(h_m, h_p) and torch.equal(c_m, c_p)
    assert torch.equal(c_in, _t(d["c0"])) and torch.equal(gh, _t(d["gh"])) and torch.equal(start, _t(d["start"]))
    h_ref, c_ref = _cell_ref(d, True, masked=True)
    _within(c_m, c_ref, 2e-6, 2e-6, "c (masked)")
    _within(h_m, h_ref, 2e-6, 2e-6, "h (masked)")
    # refusals: nothing is launched (the outputs keep their fill)
    h, c = _nan(B, N, H), _nan(B, N, H)

    def cell(st, hh, ci=None, co=None):
        if ci is None:
            return lib.vn_lstm_cell(_p(gx), st, _p(gh), _p(bi), _p(bh), _p(h), _p(c), None, None, B, N, hh, None)
        return lib.vn_lstm_cell_masked(_p(gx), st, _p(gh), _p(bi), _p(bh), _p(ci), _p(start), _p(h), _p(co), B, N, hh,
                                       None)

    assert cell(stride, 6) != 0 and cell(stride, 6, c_in, c) != 0                     # H % 4 != 0
    assert cell(B * 4 * H - 4, H) != 0 and cell(B * 4 * H - 4, H, c_in, c) != 0       # a row shorter than its gates
    assert cell(stride, H, c_in, c_in) != 0                                           # c_in == c_out
    assert lib.vn_lstm_cell_masked(_p(gx), stride, _p(gh), _p(bi), _p(bh), _p(c_in), None, _p(h), _p(c), B, N, H,
                                   None) != 0                                         # start NULL
    torch.cuda.synchronize()
    assert bool(torch.isnan(h).all()) and bool(torch.isnan(c).all()) and torch.equal(c_in, _t(d["c0"]))


@pytest.mark.parametrize("B,N,H,pad", CELL_CASES, ids=CELL_IDS)
def test_lstm_cell_bf16_matches_float64(lib, B, N, H, pad):
    """vn_lstm_cell_bf16: bf16 pre-activations that bf16 holds exactly, so
    (h, c) meet the f32 bound; h_bf16 is h rounded to nearest even."""
    d = _cell_data(B, N, H, pad)
    stride = B * 4 * H + pad
    bf = torch.bfloat16
    gx, gh, bi, bh = _t(d["gx_rows"], bf), _t(d["gh"], bf), _t(d["b_ih"]), _t(d["b_hh"])
    assert torch.equal(gx.double().cpu(), torch.as_tensor(d["gx_rows"]))              # exact in bf16
    for with_gh in (False, True):
        h_ref, c_ref = _cell_ref(d, with_gh)
        for extra in (False, True):
            h, c = _nan(B, N, H), _t(d["c0"])
            hs, cs = (_nan(B, N, H), _nan(B, N, H)) if extra else (None, None)
            h_bf = torch.full((B, N, H), float("nan"), dtype=bf, device=DEV) if extra or with_gh else None
            assert lib.vn_lstm_cell_bf16(_p(gx), stride, _p(gh) if with_gh else None, _p(bi), _p(bh), _p(h), _p(c),
                                         _p(h_bf), _p(hs), _p(cs), B, N, H, None) == 0
            torch.cuda.synchronize()
            _within(c, c_ref, 2e-6, 2e-6, f"c bf16 (gh {with_gh})")
            _within(h, h_ref, 2e-6, 2e-6, f"h bf16 (gh {with_gh})")
            if h_bf is not None:
                assert torch.equal(h_bf.view(torch.int16), h.to(bf).view(torch.int16))
            if extra:
                assert torch.equal(hs, h) and torch.equal(cs, c)
    assert torch.equal(gx, _t(d["gx_rows"], bf)) and torch.equal(gh, _t(d["gh"], bf))
    h, c = _nan(B, N, H), _nan(B, N, H)
    assert lib.vn_lstm_cell_bf16(_p(gx), stride, _p(gh), _p(bi), _p(bh), _p(h), _p(c), None, None, None, B, N, 6,
                                 None) != 0
    assert lib.vn_lstm_cell_bf16(_p(gx), B * 4 * H - 4, _p(gh), _p(bi), _p(bh), _p(h), _p(c), None, None, None, B, N, H,
                                 None) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(h).all()) and bool(torch.isnan(c).all())


# ---------------------------------------------------------------- policy head
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("N,P,A", HEAD_CASES, ids=[f"N{n}-P{p}-A{a}" for n, p, a in HEAD_CASES])
def test_policy_head_matches_float64(lib, N, P, A, dtype):
    """vn_policy_head / vn_policy_head_bf16 on exact data: ragged N over many
    blocks, one lane doing all the work (P = 4), P % 64 != 0 with all 8
    actions, and the largest P the entry point accepts with 8 actions (its
    largest LDS request, (A + 1) P floats)."""
    fn = lib.vn_policy_head if dtype == "f32" else lib.vn_policy_head_bf16
    ldt = torch.float32 if dtype == "f32" else torch.bfloat16
    d = head_case_data(N, P, A)
    lp, lv = _t(d["lat_pi"], ldt), _t(d["lat_vf"], ldt)
    wa, ba, wv, bv = _t(d["wa"]), _t(d["ba"]), _t(d["wv"]), _t(d["bv"])
    v32 = d["values"].astype(np.float32)

    def run(pi, vf, det, seed, t, base, n_actions=A, p=P):
        acts = torch.full((N,), -1, dtype=torch.int32, device=DEV)
        lps, vals = _nan(N), _nan(N)
        rc = fn(_p(lp) if pi else None, _p(lv) if vf else None, N, p, _p(wa) if pi else None, _p(ba) if pi else None,
                n_actions if pi else 0, _p(wv) if vf else None, _p(bv) if vf else None, seed, t, base, det,
                _p(acts), _p(vals), _p(lps), None)
        torch.cuda.synchronize()
        return rc, acts.cpu().numpy().astype(np.int64), lps, vals.cpu().numpy()

    def check_logp(acts, lps, what):
        assert acts.min() >= 0 and acts.max() < A
        _within(lps, d["lsm"][np.arange(N), acts], 2e-5, 2e-5, what)

    # deterministic: the arg-max of the exact logits (no ties in the data)
    rc, acts, lps, vals = run(True, True, 1, 1234, 77, 1000)
    assert rc == 0, lib.vn_last_error().decode()
    assert np.array_equal(vals, v32), "values are not the exact sums"
    assert np.array_equal(acts, d["logits"].argmax(1))
    check_logp(acts, lps, "log_probs (argmax)")
    # sampled: the draw of the float64 probabilities for the same uniform;
    # agent_id_base and t enter as collector_oracle.sample_uniform says
    draws = []
    for seed, t, base in HEAD_DRAWS:
        rc, acts, lps, vals = run(True, True, 0, seed, t, base)
        assert rc == 0 and np.array_equal(vals, v32)
        want, margin = head_draws64(d["lsm"], philox_uniform(seed, base + np.arange(N, dtype=np.uint64), t))
        diff = acts != want
        assert np.all(margin[diff] < 1e-5), f"{diff.sum()} draws differ away from a cdf boundary"
        assert diff.sum() <= 2
        check_logp(acts, lps, "log_probs (sampled)")
        draws.append(want)
    if N > 1000:
        assert (draws[0] != draws[1]).any()
        # t and agent_id_base each move the draw on their own
        seed, t, base = HEAD_DRAWS[0]
        for t2, b2 in ((t + 1, base), (t, base + 1)):
            acts2 = run(True, True, 0, seed, t2, b2)[1]
            want, margin = head_draws64(d["lsm"], philox_uniform(seed, b2 + np.arange(N, dtype=np.uint64), t2))
            assert (want != draws[0]).any() and np.all(margin[acts2 != want] < 1e-5) and (acts2 != want).sum() <= 2
    # value only: actions / log-probs untouched; pi only: values untouched
    rc, acts, lps, vals = run(False, True, 0, 0, 0, 0)
    assert rc == 0 and np.array_equal(vals, v32)
    assert (acts == -1).all() and bool(torch.isnan(lps).all())
    rc, acts, lps, vals = run(True, False, 1, 1234, 77, 1000)
    assert rc == 0 and np.isnan(vals).all()
    assert np.array_equal(acts, d["logits"].argmax(1))
    check_logp(acts, lps, "log_probs (pi only)")
    # refusals: nothing is launched
    from voxnav.collector import MAX_LATENT
    assert max(p for _, p, _ in HEAD_CASES) == MAX_LATENT
    for kw in (dict(n_actions=9), dict(p=6), dict(p=MAX_LATENT + 4)):
        rc, acts, lps, vals = run(True, True, 0, 1234, 77, 1000, **kw)
        assert rc != 0 and (acts == -1).all() and np.isnan(vals).all() and bool(torch.isnan(lps).all())
