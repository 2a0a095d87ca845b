"""Shared pieces of the collector's matrix-core kernel tests
(tests/test_collect_mfma_gpu.py, tests/test_collect_mfma_helpers_cpu.py):
vn_lstm_fused_bf16[_masked] (csrc/voxnav_collect.hip) and vn_lstm_fused_f32,
vn_linear_f32, vn_mlp_head_f32 (csrc/voxnav_policy_f32.hip) through the raw
ABI.  Here: the launch geometry of each kernel restated in Python, the packed
weight layouts written from the formulas of include/voxnav.h, inputs on which
f32 sums are exact, float64 restatements of every entry point, plain-f32
restatements that consume the packed arrays block by block (the carrier of the
CPU file's seeded defects and of the draw allowance), the derived bound for
generic inputs, and the checks both test files run -- the GPU file on the
kernels' arrays, the CPU file on the restatement's.  Importing this module
needs no GPU.

Masking (include/voxnav.h).  vn_lstm_fused_bf16_masked reads c_in as zero in
rows with start != 0 and h_in as it is (the collector zeroes h itself);
vn_lstm_fused_f32 with start reads both the h_in rows and c_in as zero.

Exact inputs.  x, h_in and the biases are multiples of 1/8 (|x|, |h| <= 1/2,
|b| <= 1 for the LSTMs), LSTM weights multiples of 1/8 (|w| <= 3/8), linear
weights multiples of 1/16 (|w| <= 3/16): every product is a multiple of 1/128
and ``assert_exact`` shows that sum |a||w| + |b| stays below 2^24 such units,
so each partial sum of any order is an exact f32 number; bf16 holds every
operand exactly too.  c0 is randn rounded to f32.

Bounds.  Exact-sum LSTM outputs: |got - f64| <= 2e-6 + 2e-6 |f64| (the
project's bound for these kernels: only the hardware exp / rcp round).  Linear:
the identity epilogue is bitwise float32(exact sum), Tanh within 1e-6 + 1e-5
|y|.  MLP head: values and log-probs within 2e-5 + 2e-5 |x|.  Generic inputs:
the pre-activation bound of gemm_helpers.bound_linear, (K + 9) u sum |a||w|,
carried through the gates with the Lipschitz constants (sigmoid 1/4, tanh 1):
  e_c = e_pre (|c_in| / 4 + |g| / 4 + |i|),  e_h = e_pre |tanh c| / 4 + |o| e_c
times 1.01 for the second-order terms, plus the exact-data bound.

f2bf (csrc/voxnav_collect.hip:45) is (u + 0x7FFF + ((u >> 16) & 1)) >> 16:
round to nearest even on finite values, which ``bf16_rne_bits`` restates.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Callable, Optional

import numpy as np
import torch

from gemm_helpers import BAND, SENTINEL, U, Slab, bound_linear
from helpers import head_draws32, head_draws64, philox_uniform
from lstm_seq_helpers import bits, flat, view

# tile constants, the kernels' documented defaults
LF_ROWS, LF_UNITS, LF_KC = 64, 64, 64              # csrc/voxnav_collect.hip:156-163
LS_ROWS, LS_UNITS, PF_KC = 128, 64, 16             # csrc/voxnav_policy_f32.hip:91, :66
LN_ROWS, LN_COLS = 128, 128                        # csrc/voxnav_policy_f32.hip:355
MH_R, MH_MAXL, MH_MAXA, MH_MAXP = 32, 4, 8, 256    # csrc/voxnav_policy_f32.hip:530

LSTM_ATOL = LSTM_RTOL = 2e-6
TANH_ATOL, TANH_RTOL = 1e-6, 1e-5
HEAD_ATOL = HEAD_RTOL = 2e-5
CDF_MARGIN, DRAW_CAP, ARGMAX_GAP = 1e-5, 2, 1e-5
SLACK = 1.01

# (n_lstm, N, H, obs_dim, extra Kp chunks)
BF16_CASES = OrderedDict([
    ("current", (2, 200, 128, 80, 0)),
    ("one_row", (1, 1, 64, 8, 0)),          # 56 zero columns from K to Kp
    ("one_tile", (2, 64, 64, 32, 0)),
    ("critic", (1, 65, 256, 80, 0)),        # a one-row second tile, four unit blocks, w_cat[1:2]
    ("swz8", (1, 509, 64, 80, 0)),          # 8 tiles, swizzled, ncombo 1
    ("swz16", (2, 1019, 128, 32, 0)),       # 16 tiles, swizzled, ncombo 4, local / ncombo > 0
    ("scalar31", (2, 130, 64, 31, 0)),      # VEC_X false, one padded column
    ("scalar5", (1, 70, 128, 5, 0)),        # VEC_X false, obs_dim < 8
    ("zero_chunk", (2, 200, 64, 80, 1)),    # a whole zero chunk beyond kx + H
])
BF16_ALL_NONE = ("one_tile", "scalar31")    # a start everywhere / nowhere
BF16_GENERIC = "current"

# (n_lstm, N, H, obs_dim)
F32_CASES = OrderedDict([
    ("smallest", (1, 1, 64, 4)),
    ("one_tile", (2, 128, 64, 16)),
    ("tail_row", (1, 129, 256, 80)),
    ("straddle", (2, 257, 128, 20)),        # VEC_X with a chunk that straddles obs_dim
    ("scalar31", (2, 130, 64, 31)),
    ("scalar5", (1, 70, 128, 5)),
    ("swz8", (2, 1021, 64, 80)),
])
F32_MULTI = OrderedDict([
    ("multi_plain", (2, 8325, 256, 80)),    # 66 tiles x 8 = 528 items
    ("multi_swz", (2, 9216, 256, 80)),      # 72 tiles, swizzled, 576 items
])
F32_ALL_NONE = ("one_tile", "scalar31")
F32_GENERIC = "straddle"

# (M, K, Nout, branches, ldx - K)
LINEAR_CASES = OrderedDict([
    ("m1k16", (1, 16, 128, 1, 0)),
    ("one_tile", (128, 80, 128, 2, 0)),
    ("tail_row", (129, 80, 256, 2, 4)),
    ("ldx12", (300, 256, 384, 1, 12)),
    ("swz8", (1021, 256, 256, 2, 0)),
])
LINEAR_GENERIC = "ldx12"
ROW_PAD = 1000.0

# (M, K0, widths, branches, A, ldx - K0)
HEAD_CASES = OrderedDict([
    ("m1", (1, 16, (128,), 2, 1, 0)),
    ("m32", (32, 80, (256, 128), 2, 8, 0)),
    ("m33", (33, 256, (256, 128, 256, 128), 2, 6, 4)),
    ("value_only", (77, 48, (128, 256), 1, 0, 0)),
    ("m300", (300, 80, (256, 256, 128), 2, 2, 12)),
])
DRAWS = [(1234, 77, 1000), (0x1234567890ABCDEF, (1 << 33) + 5, (1 << 32) + 12345)]


# ------------------------------------------------------------------- geometry
def decode(bid: int, ntiles: int, ncombo: int, swizzled: Optional[bool] = None):
    """Block (or work item) id -> (row tile, combo) as lstm_fused_bf16_kernel,
    ls_decode and linear_f32_kernel do it: with a tile count that is a multiple
    of 8 the combos of one row tile take ids of one residue mod 8 (one XCD)."""
    if swizzled is None:
        swizzled = (ntiles & 7) == 0
    if swizzled:
        xcd, local = bid & 7, bid >> 3
        return xcd + 8 * (local // ncombo), local - (local // ncombo) * ncombo
    return bid // ncombo, bid - (bid // ncombo) * ncombo


def plain_decode(bid: int, ntiles: int, ncombo: int):
    return decode(bid, ntiles, ncombo, False)


def lf_geometry(n_lstm, N, H, od, extra=0) -> dict:
    kx = (od + 7) // 8 * 8
    ntiles, ub = -(-N // LF_ROWS), H // LF_UNITS
    Kp = -(-(kx + H) // LF_KC) * LF_KC + extra * LF_KC
    return dict(rows=LF_ROWS, ntiles=ntiles, ublocks=ub, ncombo=n_lstm * ub, grid=ntiles * n_lstm * ub, kx=kx,
                K=kx + H, Kp=Kp, nchunks=Kp // LF_KC, kc=LF_KC, vec_x=od % 8 == 0, swizzled=(ntiles & 7) == 0,
                tail_rows=N - LF_ROWS * (ntiles - 1))


def ls_slots(cus: int) -> int:
    """The persistent grid of vn_lstm_fused_f32: 2 blocks per CU, rounded up to a multiple of 8."""
    return (2 * cus + 7) // 8 * 8


def ls_geometry(n_lstm, N, H, od, cus: int = 256) -> dict:
    kx = -(-od // PF_KC) * PF_KC
    ntiles, ub = -(-N // LS_ROWS), H // LS_UNITS
    n_items = ntiles * n_lstm * ub
    return dict(rows=LS_ROWS, ntiles=ntiles, ublocks=ub, ncombo=n_lstm * ub, n_items=n_items, kx=kx, K=kx + H,
                Kp=kx + H, nchunks=(kx + H) // PF_KC, kc=PF_KC, vec_x=od % 4 == 0,
                straddle=od % 4 == 0 and od % PF_KC != 0, swizzled=(ntiles & 7) == 0,
                grid=min(n_items, ls_slots(cus)), tail_rows=N - LS_ROWS * (ntiles - 1))


def ls_walk(block: int, grid: int, n_items: int):
    """The items a persistent block takes, in order."""
    return list(range(block, n_items, grid))


def ln_geometry(M, K, Nout, nb) -> dict:
    ntiles, ncb = -(-M // LN_ROWS), Nout // LN_COLS
    return dict(rows=LN_ROWS, ntiles=ntiles, ncombo=ncb, grid=(ntiles * ncb, nb), nchunks=K // PF_KC,
                swizzled=(ntiles & 7) == 0, tail_rows=M - LN_ROWS * (ntiles - 1))


def mh_geometry(M, nb) -> dict:
    """mlp_head_f32_kernel: block (x, y) is rows 32 x .. of branch br0 + y."""
    nt = -(-M // MH_R)
    return dict(rows=MH_R, ntiles=nt, grid=(nt, nb), br0=0 if nb == 2 else 1, tail_rows=M - MH_R * (nt - 1))


def check_decode(dec: Callable, ntiles: int, ncombo: int, n_ids: Optional[int] = None):
    """The decode is a bijection of the ids onto (tile, combo); when the tile
    count is a multiple of 8 every combo of tile t has an id congruent to t mod 8."""
    n = ntiles * ncombo if n_ids is None else n_ids
    seen = [dec(i, ntiles, ncombo) for i in range(n)]
    assert len(set(seen)) == n == ntiles * ncombo, "decode repeats a (tile, combo)"
    assert all(0 <= t < ntiles and 0 <= c < ncombo for t, c in seen), "decode leaves the (tile, combo) range"
    if (ntiles & 7) == 0:
        off = [i for i, (t, _) in enumerate(seen) if (i & 7) != (t & 7)]
        assert not off, f"{len(off)} ids of a swizzled grid sit on another XCD than their tile"


# --------------------------------------------------------------- packed layouts
def _bf16_exact(t: torch.Tensor) -> bool:
    return bool(torch.equal(t.float().to(torch.bfloat16).float(), t.float()))


def w_cat_bf16(w_ih, w_hh, Kp: int) -> torch.Tensor:
    """f32 [n][4H][Kp] holding vn_lstm_fused_bf16's w_cat: W_ih in columns
    [0, obs_dim), W_hh in [kx, kx + H), kx = obs_dim rounded up to 8, zeros elsewhere."""
    n, G, od = w_ih.shape
    H = w_hh.shape[2]
    kx = (od + 7) // 8 * 8
    wc = torch.zeros((n, G, Kp), dtype=torch.float32)
    for b in range(n):
        for k in range(od):
            wc[b, :, k] = w_ih[b, :, k]
        for k in range(H):
            wc[b, :, kx + k] = w_hh[b, :, k]
    return wc


def _lstm32_index(n, H, Kp):
    b, ub, k, g, uu = torch.meshgrid(torch.arange(n), torch.arange(H // LS_UNITS), torch.arange(Kp), torch.arange(4),
                                     torch.arange(LS_UNITS), indexing="ij")
    return b, g * H + LS_UNITS * ub + uu, k


def lstm32_wcat(w_ih, w_hh) -> torch.Tensor:
    """[W_ih | 0 | W_hh] f32 [n][4H][Kp], kx = obs_dim rounded up to 16, Kp = kx + H."""
    n, G, od = w_ih.shape
    H = w_hh.shape[2]
    kx = -(-od // PF_KC) * PF_KC
    wc = torch.zeros((n, G, kx + H), dtype=torch.float32)
    wc[:, :, :od] = w_ih
    wc[:, :, kx:] = w_hh
    return wc


def pack_lstm_f32_ref(w_ih, w_hh) -> torch.Tensor:
    """vn_lstm_fused_f32's w_packed [n][H/64][Kp][4][64]: element
    [b][ub][k][g][uu] = Wcat_b[g H + 64 ub + uu][k]."""
    wc = lstm32_wcat(w_ih, w_hh)
    return wc[_lstm32_index(wc.shape[0], w_hh.shape[2], wc.shape[2])].contiguous()


def unpack_lstm_f32(packed: torch.Tensor) -> torch.Tensor:
    n, ub, Kp = packed.shape[:3]
    wc = torch.zeros((n, 4 * ub * LS_UNITS, Kp), dtype=packed.dtype)
    wc[_lstm32_index(n, ub * LS_UNITS, Kp)] = packed
    return wc


def _linear_index(Nout, K):
    cb, k, j = torch.meshgrid(torch.arange(Nout // LN_COLS), torch.arange(K), torch.arange(LN_COLS), indexing="ij")
    return LN_COLS * cb + j, k


def pack_linear_f32_ref(w: torch.Tensor) -> torch.Tensor:
    """vn_linear_f32's w_packed [Nout/128][K][128]: element [cb][k][j] = W[128 cb + j][k]."""
    return w.float()[_linear_index(*w.shape)].contiguous()


def unpack_linear_f32(packed: torch.Tensor) -> torch.Tensor:
    ncb, K = packed.shape[:2]
    w = torch.zeros((ncb * LN_COLS, K), dtype=packed.dtype)
    w[_linear_index(ncb * LN_COLS, K)] = packed
    return w


def _mlp_index(N, Kp):
    cb, kg, lane, s = torch.meshgrid(torch.arange(N // 32), torch.arange(Kp // 8), torch.arange(64), torch.arange(4),
                                     indexing="ij")
    return 32 * cb + lane % 32, 8 * kg + 4 * (lane // 32) + s


def pack_mlp_head_f32_ref(w: torch.Tensor) -> torch.Tensor:
    """vn_mlp_head_f32's per-lane layout [N/32][Kp/8][64][4], Kp = K rounded up
    to 16 with zero weights past K: element [cb][kg][lane][s] =
    W[32 cb + lane % 32][8 kg + 4 (lane / 32) + s]."""
    N, K = w.shape
    Kp = -(-K // 16) * 16
    wp = torch.zeros((N, Kp), dtype=torch.float32)
    wp[:, :K] = w
    return wp[_mlp_index(N, Kp)].contiguous()


def unpack_mlp_head_f32(packed: torch.Tensor) -> torch.Tensor:
    N, Kp = packed.shape[0] * 32, packed.shape[1] * 8
    w = torch.zeros((N, Kp), dtype=packed.dtype)
    w[_mlp_index(N, Kp)] = packed
    return w


def bf16_rne_bits(t: torch.Tensor) -> torch.Tensor:
    """f2bf of csrc/voxnav_collect.hip on finite f32 values -> int32 holding the 16 bits."""
    u = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).to(torch.int32)


def bf16_trunc_bits(t: torch.Tensor) -> torch.Tensor:
    return ((t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF) >> 16).to(torch.int32)


def bf16_bits(t: torch.Tensor) -> torch.Tensor:
    """The 16 bits of a bf16 tensor as int32."""
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


# --------------------------------------------------------------------- inputs
def _ri(g, lo, hi, den, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float() / den


def lstm_inputs(kind: str, case: str, generic: bool = False) -> dict:
    """CPU f32 inputs of an LSTM case (kind 'bf16' or 'f32'), seeded per case.
    Generic: x normal, h uniform in +-1, nn.LSTM's default weights (uniform in
    +-1 / sqrt(H)); the bf16 kind rounds h and the weights to bf16, which is
    what the entry takes.  start is drawn at 0.3."""
    table = BF16_CASES if kind == "bf16" else {**F32_CASES, **F32_MULTI}
    row = table[case]
    n, N, H, od = row[:4]
    g = torch.Generator()
    g.manual_seed(41000 + 1000 * (kind == "f32") + 17 * list(table).index(case) + 500 * generic)
    if generic:
        k = 1.0 / H ** 0.5
        uni = lambda *s: (torch.rand(s, generator=g) * 2.0 - 1.0)  # noqa: E731
        x, h_in = torch.randn((N, od), generator=g), uni(n, N, H)
        w_ih, w_hh, bias = uni(n, 4 * H, od) * k, uni(n, 4 * H, H) * k, (uni(n, 4 * H) + uni(n, 4 * H)) * k
        if kind == "bf16":
            h_in, w_ih, w_hh = (t.to(torch.bfloat16).float() for t in (h_in, w_ih, w_hh))
    else:
        x, h_in = _ri(g, -4, 4, 8.0, N, od), _ri(g, -4, 4, 8.0, n, N, H)
        w_ih, w_hh = _ri(g, -3, 3, 8.0, n, 4 * H, od), _ri(g, -3, 3, 8.0, n, 4 * H, H)
        bias = _ri(g, -8, 8, 8.0, n, 4 * H)
    c0 = torch.randn((n, N, H), generator=g)
    start = (torch.rand((N,), generator=g) < 0.3).float()
    geo = lf_geometry(n, N, H, od, row[4]) if kind == "bf16" else ls_geometry(n, N, H, od)
    return dict(kind=kind, case=case, n=n, N=N, H=H, od=od, geo=geo, x=x, h_in=h_in, w_ih=w_ih, w_hh=w_hh, bias=bias,
                c0=c0, start=start, exact=not generic)


def lstm_packed(d: dict) -> torch.Tensor:
    """The case's packed weights (f32 values; the bf16 entry takes them as bf16)."""
    if d["kind"] == "bf16":
        return w_cat_bf16(d["w_ih"], d["w_hh"], d["geo"]["Kp"])
    return pack_lstm_f32_ref(d["w_ih"], d["w_hh"])


def starts(d: dict, which: str) -> torch.Tensor:
    return {"drawn": d["start"], "all": torch.ones_like(d["start"]), "none": torch.zeros_like(d["start"])}[which]


def poisoned(t: torch.Tensor, start: torch.Tensor) -> torch.Tensor:
    """[n][N][H] with NaN in the rows that start an episode."""
    return torch.where(start.view(1, -1, 1) != 0, torch.full_like(t, float("nan")), t)


def masked_state(t: torch.Tensor, start: torch.Tensor) -> torch.Tensor:
    return torch.where(start.view(1, -1, 1) != 0, torch.zeros_like(t), t)


def assert_exact(a_abs_w_sum: torch.Tensor, bias: torch.Tensor, operands, unit: float):
    """Every operand is a multiple of its unit and bf16-exact, and
    (sum |a||w| + |b|) / unit < 2^24: every partial sum is an exact f32."""
    for t, u in operands:
        assert bool(((t.double() / u) == (t.double() / u).round()).all()), f"an operand is no multiple of {u}"
        assert _bf16_exact(t), "an operand is not exact in bf16"
    worst = float(a_abs_w_sum.max()) + float(bias.abs().max())
    assert worst / unit < 2 ** 24, f"partial sums reach {worst / unit:.3g} units of {unit}"


def assert_exact_lstm(d: dict):
    x, h = d["x"].double().abs(), d["h_in"].double().abs()
    m = (torch.einsum("nk,bgk->bng", x, d["w_ih"].double().abs())
         + torch.einsum("bnk,bgk->bng", h, d["w_hh"].double().abs()))
    assert_exact(m, d["bias"], [(d["x"], 1 / 8), (d["h_in"], 1 / 8), (d["w_ih"], 1 / 8), (d["w_hh"], 1 / 8),
                                (d["bias"], 1 / 8)], 1 / 64)


def linear_inputs(case: str, generic: bool = False) -> dict:
    M, K, Nout, nb, pad = LINEAR_CASES[case]
    g = torch.Generator()
    g.manual_seed(43000 + 17 * list(LINEAR_CASES).index(case) + 500 * generic)
    if generic:
        xs = [torch.randn((M, K), generator=g) for _ in range(nb)]
        ws = [torch.randn((Nout, K), generator=g) / K ** 0.5 for _ in range(nb)]
        bs = [0.1 * torch.randn((Nout,), generator=g) for _ in range(nb)]
    else:
        xs = [_ri(g, -4, 4, 8.0, M, K) for _ in range(nb)]
        ws = [_ri(g, -3, 3, 16.0, Nout, K) for _ in range(nb)]
        bs = [_ri(g, -8, 8, 8.0, Nout) for _ in range(nb)]
    return dict(case=case, M=M, K=K, Nout=Nout, nb=nb, ldx=K + pad, xs=xs, ws=ws, bs=bs, geo=ln_geometry(M, K, Nout, nb),
                exact=not generic)


def assert_exact_linear(d: dict):
    for x, w, b in zip(d["xs"], d["ws"], d["bs"]):
        assert_exact(x.double().abs() @ w.double().abs().T, b, [(x, 1 / 8), (w, 1 / 16), (b, 1 / 8)], 1 / 128)


def padded_rows(x: torch.Tensor, ldx: int, fill: float = ROW_PAD) -> torch.Tensor:
    """[M][ldx] with x in the first columns and `fill` in the row padding."""
    out = torch.full((x.shape[0], ldx), fill, dtype=torch.float32)
    out[:, :x.shape[1]] = x
    return out


def head_inputs(case: str) -> dict:
    """Generic data (Tanh outputs cannot be exact), scaled as the existing
    vn_mlp_head_f32 test scales it."""
    M, K0, widths, nb, A, pad = HEAD_CASES[case]
    g = torch.Generator()
    g.manual_seed(47000 + 17 * list(HEAD_CASES).index(case))
    rn = lambda *s, sc=1.0: torch.randn(s, generator=g) * sc  # noqa: E731
    xs = [rn(M, K0) for _ in range(nb)]
    layers = []
    for _ in range(nb):
        ls, k = [], K0
        for w in widths:
            ls.append((rn(w, k, sc=1.0 / k ** 0.5), rn(w, sc=0.1)))
            k = w
        layers.append(ls)
    P = widths[-1]
    d = dict(case=case, M=M, K0=K0, widths=widths, nb=nb, A=A, ldx=K0 + pad, xs=xs, layers=layers, P=P,
             wv=rn(P, sc=1.0 / P ** 0.5), bv=rn(1), geo=mh_geometry(M, nb))
    if nb == 2:
        d["wa"], d["ba"] = rn(A, P, sc=3.0 / P ** 0.5), rn(A, sc=0.5)
    return d


# ----------------------------------------------------------------- references
def lstm_ref(d: dict, start: Optional[torch.Tensor], dtype=torch.float64, device=None) -> dict:
    """One step of every LSTM of a case in `dtype`: start None is the plain
    entry; with start the bf16 kind masks c_in only, the f32 kind the h_in rows
    and c_in.  The bf16 kind rounds x to bf16 first (the kernel's operand).
    -> pre [n][N][4H], i, f, g, o, c_in, c, h [n][N][H]."""
    to = lambda t: t.to(device=device, dtype=dtype)  # noqa: E731
    x = d["x"].to(torch.bfloat16).float() if d["kind"] == "bf16" else d["x"]
    h_in, c_in = d["h_in"], d["c0"]
    if start is not None:
        c_in = masked_state(c_in, start)
        if d["kind"] == "f32":
            h_in = masked_state(h_in, start)
    pre = (torch.einsum("nk,bgk->bng", to(x), to(d["w_ih"])) + torch.einsum("bnk,bgk->bng", to(h_in), to(d["w_hh"]))
           + to(d["bias"])[:, None, :])
    i, f, g, o = pre.chunk(4, dim=-1)
    i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
    c = f * to(c_in) + i * g
    return dict(pre=pre, i=i, f=f, g=g, o=o, c_in=to(c_in), c=c, h=o * torch.tanh(c))


def lstm_bound(d: dict, ref: dict, start: Optional[torch.Tensor]):
    """(e_c, e_h): the module docstring's derived bound for generic inputs, on top of the exact-data one."""
    x = d["x"].to(torch.bfloat16).float() if d["kind"] == "bf16" else d["x"]
    h_in = masked_state(d["h_in"], start) if (start is not None and d["kind"] == "f32") else d["h_in"]
    dev = ref["c"].device
    m = (torch.einsum("nk,bgk->bng", x.double().abs().to(dev), d["w_ih"].double().abs().to(dev))
         + torch.einsum("bnk,bgk->bng", h_in.double().abs().to(dev), d["w_hh"].double().abs().to(dev))
         + d["bias"].double().abs().to(dev)[:, None, :])
    e = (d["geo"]["Kp"] + 9) * U * m
    ei, ef, eg, eo = e.chunk(4, dim=-1)
    e_c = ef / 4 * ref["c_in"].abs() + ei / 4 * ref["g"].abs() + ref["i"].abs() * eg
    e_h = eo / 4 * torch.tanh(ref["c"]).abs() + ref["o"].abs() * e_c
    return (SLACK * e_c + LSTM_ATOL + LSTM_RTOL * ref["c"].abs(), SLACK * e_h + LSTM_ATOL + LSTM_RTOL * ref["h"].abs())


def linear_ref(d: dict, act: bool, device=None):
    out = []
    for x, w, b in zip(d["xs"], d["ws"], d["bs"]):
        z = x.double().to(device) @ w.double().to(device).T + b.double().to(device)
        out.append(torch.tanh(z) if act else z)
    return out


def head_ref(d: dict) -> dict:
    """float64: the MLP of each branch, the logits and log-softmax of the pi branch, the values of the vf branch."""
    hs = []
    for x, ls in zip(d["xs"], d["layers"]):
        h = x.double()
        for w, b in ls:
            h = torch.tanh(h @ w.double().T + b.double())
        hs.append(h)
    r = dict(values=hs[-1] @ d["wv"].double() + d["bv"].double())
    if d["nb"] == 2:
        r["logits"] = hs[0] @ d["wa"].double().T + d["ba"].double()
        r["lsm"] = torch.log_softmax(r["logits"], -1)
    return r


def draw_uniforms(M: int, draw) -> np.ndarray:
    seed, t, base = draw
    return philox_uniform(seed, np.uint64(base) + np.arange(M, dtype=np.uint64), t)


# ------------------------------------------------ plain-f32 restatements, by block
def _scatter(full: torch.Tensor, out: torch.Tensor, geo: dict, cols: int, dec: Callable, n_ids: int, drop_last_row: bool):
    """full, out [n_mat][rows][width]: every id's (tile, combo) block copied, combo = matrix x column block."""
    R, ncb = geo["rows"], full.shape[2] // cols
    N = full.shape[1]
    for bid in range(n_ids):
        tile, combo = dec(bid, geo["ntiles"], geo["ncombo"])
        b, cb = combo // ncb, combo % ncb
        r1 = min(N, (tile + 1) * R)
        if drop_last_row and tile == geo["ntiles"] - 1 and geo["tail_rows"] < R:
            r1 -= 1
        out[b, tile * R:r1, cb * cols:(cb + 1) * cols] = full[b, tile * R:r1, cb * cols:(cb + 1) * cols]


LSTM_DEFECTS = ("gates", "last_row", "chunk", "pad_column", "h_mask", "plain_decode", "truncate")


def lstm_plain32(d: dict, packed: torch.Tensor, h_in: torch.Tensor, c_in: torch.Tensor, start: Optional[torch.Tensor],
                 defect: Optional[str] = None) -> dict:
    """The entry restated in torch f32 from the arrays the kernel takes: the
    packed weights, x between NaN guard floats, h_in and c_in as passed
    (NaN-poisoned rows included), start.  Outputs are NaN until a block of the
    grid, decoded as the kernel decodes it, writes them.  -> c, h (f32), hb
    (the bf16 bits of h, bf16 kind), decode (the decode used)."""
    kind, geo, n, N, H, od = d["kind"], d["geo"], d["n"], d["N"], d["H"], d["od"]
    kx, Kp = geo["kx"], geo["Kp"]
    wc = packed if kind == "bf16" else unpack_lstm_f32(packed)
    x = d["x"].to(torch.bfloat16).float() if kind == "bf16" else d["x"]
    a = torch.zeros((n, N, Kp), dtype=torch.float32)
    a[:, :, :od] = x
    if defect == "pad_column" and kx > od:
        xf = torch.cat([x.reshape(-1), torch.full((kx,), float("nan"))])       # the guard band behind x
        for j in range(od, kx):
            a[:, :, j] = xf[torch.arange(N) * od + j]
    mask_h = (kind == "f32") != (defect == "h_mask")
    sel = start is not None
    h = h_in
    if sel and mask_h:
        h = torch.where(start.view(1, -1, 1) != 0, torch.zeros_like(h), h)     # by select: NaN rows do not pass
    a[:, :, kx:kx + H] = h
    if defect == "chunk":
        a[:, :, geo["kc"]:2 * geo["kc"]] = 0.0
    pre = torch.einsum("bnk,bgk->bng", a, wc) + d["bias"][:, None, :]
    gi, gf, gg, go = pre.chunk(4, dim=-1)
    if defect == "gates":
        gi, gf = gf, gi
    i, f, g, o = torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)
    cin = torch.where(start.view(1, -1, 1) != 0, torch.zeros_like(c_in), c_in) if sel else c_in
    c = f * cin + i * g
    hn = o * torch.tanh(c)
    dec = plain_decode if defect == "plain_decode" else decode
    n_ids = geo["grid"] if kind == "bf16" else geo["n_items"]
    out = dict(decode=dec)
    for k, full in (("c", c), ("h", hn)):
        out[k] = torch.full_like(full, float("nan"))
        _scatter(full, out[k], geo, LF_UNITS, dec, n_ids, defect == "last_row")
    if kind == "bf16":
        hb = torch.where(torch.isfinite(out["h"]), out["h"], torch.zeros_like(out["h"]))
        out["hb"] = bf16_trunc_bits(hb) if defect == "truncate" else bf16_rne_bits(hb)
    return out


def linear_plain32(d: dict, xbufs, packed, act: bool, defect: Optional[str] = None):
    """vn_linear_f32 in torch f32 from the padded x rows [M][ldx] and the packed weights."""
    M, K, ldx = d["M"], d["K"], d["ldx"]
    ys = []
    for xb, wp, b in zip(xbufs, packed, d["bs"]):
        flatx = xb.reshape(-1)
        ld = K if defect == "ldx" else ldx
        x = flatx[(torch.arange(M) * ld)[:, None] + torch.arange(K)[None, :]]
        z = x @ unpack_linear_f32(wp).T + b
        full = (torch.tanh(z) if act else z)[None]
        y = torch.full_like(full, float("nan"))
        _scatter(full, y, d["geo"], LN_COLS, plain_decode if defect == "plain_decode" else decode,
                 d["geo"]["grid"][0], defect == "last_row")
        ys.append(y[0])
    return ys


HEAD_DEFECTS = ("ldx", "bias", "agent_id_base", "last_row")


def head_plain32(d: dict, xbufs, packed, det: bool, draw, defect: Optional[str] = None) -> dict:
    """vn_mlp_head_f32 in torch / numpy f32: the layers from the packed
    weights, the heads, and helpers.head_draws32 for the draw."""
    M, K0 = d["M"], d["K0"]
    ld = K0 if defect == "ldx" else d["ldx"]
    nl = len(d["widths"])
    hs = []
    for bi, xb in enumerate(xbufs):
        h = xb.reshape(-1)[(torch.arange(M) * ld)[:, None] + torch.arange(K0)[None, :]]
        for l in range(nl):
            w = unpack_mlp_head_f32(packed[bi * nl + l])[:, :h.shape[1]]
            z = h @ w.T
            if not (defect == "bias" and l == nl - 1):
                z = z + d["layers"][bi][l][1]
            h = torch.tanh(z)
        hs.append(h)
    live = M - 1 if defect == "last_row" else M
    nan = float("nan")
    out = dict(values=torch.full((M,), nan))
    out["values"][:live] = (hs[-1] @ d["wv"] + d["bv"])[:live]
    if d["nb"] == 2:
        lg = (hs[0] @ d["wa"].T + d["ba"]).numpy()
        if det:
            act = lg.argmax(1)
        else:
            seed, t, base = draw
            act = head_draws32(lg, draw_uniforms(M, (seed, t, 0 if defect == "agent_id_base" else base)))
        lsm = torch.log_softmax(torch.as_tensor(lg), -1)
        out["actions"] = torch.full((M,), SENTINEL, dtype=torch.int32)
        out["actions"][:live] = torch.as_tensor(act, dtype=torch.int32)[:live]
        out["log_probs"] = torch.full((M,), nan)
        out["log_probs"][:live] = lsm[torch.arange(M), torch.as_tensor(act)][:live]
    return out


# --------------------------------------------------------------------- checks
SHARES = {}    # what -> the largest share of its bound used in this process


def assert_bounded(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str):
    """Entrywise |got - ref| <= bound; prints the maximum error and the share of the bound used."""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~torch.isfinite(got)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} NaN / unwritten, first at {bad.nonzero()[0].tolist()}"
    err = (got.double().to(ref.device) - ref).abs()
    share = float((err / bound).max())
    key = what.split(":")[-1].strip()
    SHARES[key] = max(SHARES.get(key, 0.0), share)
    print(f"MAXERR {what} {float(err.max()):.3e} share {share:.4f}")
    assert share <= 1.0, f"{what}: {int((err > bound).sum())} of {err.numel()} beyond the bound, worst share {share:.3g}"


def check_lstm(d: dict, ref: dict, out: dict, what: str, bound=None):
    """out: c and h (the f32 h: h_store, h32 or the f32 entry's h_out) and,
    where the launch passed them, c_store, h32, h_store, hb (bf16 bits of
    h_out).  Values against `ref` within the exact-data bound (or `bound` =
    (e_c, e_h)); the copies and the bf16 rounding bit for bit."""
    e_c, e_h = bound if bound is not None else (LSTM_ATOL + LSTM_RTOL * ref["c"].abs(),
                                                LSTM_ATOL + LSTM_RTOL * ref["h"].abs())
    assert_bounded(out["c"], ref["c"], e_c, f"{what}: c")
    if out.get("h") is not None:
        assert_bounded(out["h"], ref["h"], e_h, f"{what}: h")
    if out.get("c_store") is not None:
        assert torch.equal(bits(out["c_store"]), bits(out["c"])), f"{what}: c_store is not c"
    if out.get("h32") is not None and out.get("h_store") is not None:
        assert torch.equal(bits(out["h32"]), bits(out["h_store"])), f"{what}: h32 is not h_store"
    if out.get("hb") is not None and out.get("h") is not None:
        want = bf16_rne_bits(out["h"])
        diff = out["hb"].cpu() != want
        assert not bool(diff.any()), (f"{what}: h_out is not the round-to-nearest-even bf16 of the stored h at "
                                      f"{int(diff.sum())} of {diff.numel()}")


def check_linear(d: dict, refs, ys, act: bool, what: str, bounds=None):
    for i, (ref, y) in enumerate(zip(refs, ys)):
        if bounds is not None:
            assert_bounded(y, ref, bounds[i], f"{what} branch {i}: y generic")
        elif act:
            assert_bounded(y, ref, TANH_ATOL + TANH_RTOL * ref.abs(), f"{what} branch {i}: y tanh")
        else:
            assert bool(torch.isfinite(y).all()), f"{what} branch {i}: NaN / unwritten"
            assert torch.equal(y.cpu(), ref.float().cpu()), f"{what} branch {i}: identity form is not float32(exact sum)"


def linear_bounds(d: dict, refs, act: bool):
    out = []
    for x, w, b, ref in zip(d["xs"], d["ws"], d["bs"], refs):
        e = SLACK * bound_linear(x, w, b, d["K"]).to(ref.device)
        out.append(e + TANH_ATOL + TANH_RTOL * ref.abs() if act else e)
    return out


def check_head(d: dict, ref: dict, out: dict, det: bool, draw, what: str) -> int:
    """-> the number of sampled actions that differ from the float64 draw (all within CDF_MARGIN of a boundary)."""
    M = d["M"]
    assert_bounded(out["values"], ref["values"], HEAD_ATOL + HEAD_RTOL * ref["values"].abs(), f"{what}: values")
    if d["nb"] == 1:
        return 0
    act = out["actions"].long()
    assert bool(((act >= 0) & (act < d["A"])).all()), f"{what}: actions outside 0..{d['A'] - 1} (or unwritten)"
    lsm = ref["lsm"]
    n_diff = 0
    if det:
        if d["A"] > 1:
            srt = ref["logits"].sort(-1, descending=True).values
            clear = (srt[:, 0] - srt[:, 1]) > ARGMAX_GAP
            assert torch.equal(act[clear], ref["logits"].argmax(-1)[clear]), f"{what}: not the float64 arg-max"
    else:
        want, margin = head_draws64(lsm.numpy(), draw_uniforms(M, draw))
        diff = act.numpy() != want
        n_diff = int(diff.sum())
        assert bool((margin[diff] < CDF_MARGIN).all()), (f"{what}: {int((margin[diff] >= CDF_MARGIN).sum())} draws "
                                                         f"differ away from a CDF boundary")
        assert n_diff <= DRAW_CAP, f"{what}: {n_diff} draws differ from the float64 draw (cap {DRAW_CAP})"
    lp_ref = lsm.gather(1, act[:, None])[:, 0]
    assert_bounded(out["log_probs"], lp_ref, HEAD_ATOL + HEAD_RTOL * lp_ref.abs(), f"{what}: log_probs")
    return n_diff


# -------------------------------------------------------------------- buffers
def fbuf(dev, data: Optional[torch.Tensor] = None, numel: Optional[int] = None) -> Slab:
    """A guarded f32 array: `data`, or `numel` sentinel NaNs (an output)."""
    return flat(dev, data.numel(), data) if data is not None else flat(dev, numel)


def hbuf(dev, data: Optional[torch.Tensor] = None, numel: Optional[int] = None) -> Slab:
    """A guarded bf16 array (an even count): the sentinel's halves are a NaN and 0xA5A5."""
    n = data.numel() if data is not None else numel
    assert n % 2 == 0
    s = flat(dev, n // 2)
    if data is not None:
        hview(s).copy_(data.reshape(-1).to(torch.bfloat16))
    return s


def hview(s: Slab) -> torch.Tensor:
    return s.mat(0).reshape(-1).view(torch.bfloat16)


def iview(s: Slab) -> torch.Tensor:
    return s.raw[s.off0:s.off0 + s.cols]


def snapshot(slabs) -> list:
    return [s.raw.clone() for s in slabs]


def unchanged(slabs, snap) -> bool:
    return all(torch.equal(s.raw, r) for s, r in zip(slabs, snap))


__all__ = [n for n in dir() if not n.startswith("_")]
