"""Shared pieces of the per-step LSTM loop tests (tests/test_lstm_seq_gpu.py,
tests/test_lstm_seq_helpers_cpu.py): a restatement of the launch geometry of
csrc/voxnav_learn_f32.hip, float64 restatements of the forward and backward
time loops in the ABI's own layouts, the same restatements in plain f32 (the
yardstick of the tolerance), the comparator, the case table and guarded
buffers.  Importing this module needs no GPU.

Layouts (n = n_lstm LSTMs sharing x, gate order i, f, g, o):
  x [L, B, D]   w_ih [n, 4H, D]   w_hh [n, 4H, H]   bias [n, 4H] (b_ih + b_hh)
  hs, cs [n, L+1, B, H] (row 0: the initial state)    act [L, n, B, 4H]
  dh_out, [n, L, B, H]   dG [n, L, B, 4H]   dc, dh0 [n, B, H]

Tolerance.  ``assert_lstm_close`` compares per LSTM and per time step: with
u = 2^-24 and scale = max|ref64| of the slice,
  max|got - ref64| <= F max(max|p32 - ref64|, u scale),
where p32 is the f32 restatement of the reference (plain matmul, then the
gates), never the kernel.  F covers the kernel's other summation order (4
waves x 2-wide MFMA steps, an LDS reduction) and its own expf / tanhf.

Measured ratios max|got - ref64| / max(max|p32 - ref64|, u scale), the worst
slice of each compared array over the whole case table (cases A..K, the
backward from the kernel's own forward arrays, with and without dh0), on an
MI355X:
  hs 1.5204 (F)   cs 1.5026 (B)   act 2.2015 (I)
  dG 1.1800 (F)   dc 1.5052 (I)   dh0 1.4607 (K)
(torch 2.10.0+rocm7.0).  The further runs stay below them: case E with
saturated gates hs 1.5374, the wrapper's outputs 1.7814 (the padded batch),
h0.grad 1.1394, c0.grad 1.0000.  The worst is 2.2015, twice it 4.403, so
F = 8: the smallest power of two at least twice the worst ratio.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Optional

import torch

from gemm_helpers import SENTINEL, Slab

U = 2.0 ** -24
F = 8.0

LQ_ROWS, LQ_UNITS, LQ_KC = 32, 32, 8

# (n_lstm, D, H, L, B) -- what each case hits is asserted by
# tests/test_lstm_seq_helpers_cpu.py from seq_geometry
CASES = OrderedDict([
    ("A", (2, 80, 256, 3, 33)),    # production templates <42> / <128>, swizzle with ncombo 16, a one-row tile
    ("B", (2, 208, 128, 2, 40)),   # <42> with another x|h split, backward <0> with 64 chunks, ncombo 8
    ("C", (2, 16, 320, 2, 32)),    # <42> again, UB 10, plain mapping (ncombo 20), NCb 160
    ("D", (1, 4, 4, 1, 1)),        # every minimum: NCf 2 and NCb 2 (two idle waves), L 1, B 1
    ("E", (2, 12, 12, 4, 31)),     # x|h seam inside a chunk, h tail from the zero block, B < 32
    ("F", (3, 8, 36, 3, 65)),      # odd n_lstm, 4 live units in the second unit block, three row tiles
    ("G", (2, 96, 32, 2, 64)),     # forward NC exactly 16
    ("H", (2, 96, 40, 2, 32)),     # forward NC 17
    ("I", (2, 4, 64, 3, 33)),      # backward NCb 32
    ("J", (4, 20, 68, 2, 8)),      # backward NCb 34, n_lstm 4, ncombo 12
    ("K", (2, 8, 384, 2, 70)),     # swizzle with ncombo 24 and three row tiles
])


# ------------------------------------------------------------------- geometry
def seq_geometry(n_lstm: int, D: int, H: int, B: int) -> dict:
    """lq_geom / lq_block of csrc/voxnav_learn_f32.hip restated: the chunk
    counts, the kernel templates the entry points pick, the block mapping and
    the pipeline trip counts for n_lstm LSTMs of D -> H over B rows."""
    kx = D
    Hp = -(-H // LQ_KC) * LQ_KC
    Kp = -(-(kx + Hp) // LQ_KC) * LQ_KC
    NCf, NCb = Kp // LQ_KC, -(-4 * H // LQ_KC)
    UB = -(-H // LQ_UNITS)
    ncombo, ntiles = n_lstm * UB, -(-B // LQ_ROWS)
    return dict(
        kx=kx, Kp=Kp, NCf=NCf, NCb=NCb, UB=UB, ncombo=ncombo, ntiles=ntiles,
        fwd_template="42" if NCf == 42 else "0", bwd_template="128" if NCb == 128 else "0",
        swizzled=ncombo % 8 == 0,
        fwd_n_it=-(-NCf // 16), bwd_n_it=-(-NCb // 32),
        fwd_idle_waves=max(0, 4 - NCf), bwd_idle_waves=max(0, 4 - NCb),   # waves whose first chunk is past NC
        live_units_last_block=H - LQ_UNITS * (UB - 1),
        seam_in_chunk=D % 8 == 4, h_tail_from_zero=H % 8 == 4,
        fwd_floats=n_lstm * UB * NCf * 2 * LQ_UNITS * 16 + 64,
        bwd_floats=n_lstm * UB * NCb * 2 * LQ_UNITS * 4 + 64,
    )


def block_of(block_id: int, ncombo: int, ntiles: int, UB: int):
    """lq_block: (LSTM, unit block, row tile) of a block id."""
    if ncombo % 8 == 0:
        xcd, local = block_id & 7, block_id >> 3
        combo, rt = xcd + 8 * (local // ntiles), local % ntiles
    else:
        combo, rt = divmod(block_id, ntiles)
    return combo // UB, combo % UB, rt


# --------------------------------------------------------------------- inputs
def make_inputs(case: str, shape=None) -> dict:
    """f32 CPU inputs of a case: nn.LSTM's default init (uniform in +-1 /
    sqrt(H); bias = b_ih + b_hh), standard-normal x, h0, c0, dh_out, and a
    dc_in that is zero in every other case of the table, standard normal in
    the rest.  The seed is the case's own."""
    n, D, H, L, B = CASES[case] if shape is None else shape
    idx = list(CASES).index(case) if case in CASES else 97
    g = torch.Generator()
    g.manual_seed(20240 + 131 * idx)
    k = 1.0 / math.sqrt(H)
    uni = lambda *s: (torch.rand(s, generator=g) * 2.0 - 1.0) * k  # noqa: E731
    rnd = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    d = dict(n=n, D=D, H=H, L=L, B=B)
    d["w_ih"], d["w_hh"] = uni(n, 4 * H, D), uni(n, 4 * H, H)
    d["bias"] = uni(n, 4 * H) + uni(n, 4 * H)
    d["x"], d["h0"], d["c0"] = rnd(L, B, D), rnd(n, B, H), rnd(n, B, H)
    d["dh_out"] = rnd(n, L, B, H)
    dc = rnd(n, B, H)
    d["dc_in"] = torch.zeros_like(dc) if idx % 2 == 0 else dc
    return d


# ----------------------------------------------------------------- references
def _fwd(x, w_ih, w_hh, bias, h0, c0, dtype):
    x, w_ih, w_hh, bias, h0, c0 = (t.to(dtype) for t in (x, w_ih, w_hh, bias, h0, c0))
    L, H = x.shape[0], w_hh.shape[2]
    hs, cs, act = [h0], [c0], []
    for t in range(L):
        pre = x[t] @ w_ih.transpose(1, 2) + hs[-1] @ w_hh.transpose(1, 2) + bias.unsqueeze(1)   # [n, B, 4H]
        i, f, o = (torch.sigmoid(pre[..., s * H:(s + 1) * H]) for s in (0, 1, 3))
        gg = torch.tanh(pre[..., 2 * H:3 * H])
        c = f * cs[-1] + i * gg
        hs.append(o * torch.tanh(c))
        cs.append(c)
        act.append(torch.cat([i, f, gg, o], dim=-1))
    return torch.stack(hs, 1), torch.stack(cs, 1), torch.stack(act, 0)


def _bwd(dh_out, dc_in, w_hh, act, cs, dtype):
    dh_out, dc, w_hh, act, cs = (t.to(dtype) for t in (dh_out, dc_in, w_hh, act, cs))
    L, H = dh_out.shape[1], w_hh.shape[2]
    dG = [None] * L
    for t in range(L - 1, -1, -1):
        dh = dh_out[:, t] + dG[t + 1] @ w_hh if t < L - 1 else dh_out[:, t]
        i, f, g, o = (act[t][..., s * H:(s + 1) * H] for s in range(4))
        cp, tc = cs[:, t], torch.tanh(cs[:, t + 1])
        dcc = dc + (dh * o) * (1.0 - tc * tc)
        dG[t] = torch.cat([dcc * g * (i * (1.0 - i)), dcc * cp * (f * (1.0 - f)), dcc * i * (1.0 - g * g),
                           dh * tc * (o * (1.0 - o))], dim=-1)
        dc = dcc * f
    return torch.stack(dG, 1), dc, dG[0] @ w_hh


def lstm_ref64(x, w_ih, w_hh, bias, h0, c0):
    """n stacked LSTMs sharing x, step by step in float64 -> hs, cs
    [n, L+1, B, H] and act [L, n, B, 4H] (i, f, g, o after the nonlinearity):
    the arrays vn_lstm_seq_fwd_mfma writes.  Differentiable (torch autograd)."""
    return _fwd(x, w_ih, w_hh, bias, h0, c0, torch.float64)


def lstm_bwd_ref64(dh_out, dc_in, w_hh, act, cs):
    """The hand-written backward in float64 from forward arrays `act`, `cs`,
    with the formulas of lstm_bwd_step_kernel's epilogue -> dG [n, L, B, 4H],
    dc_out (dL/dc_0) and dh0 = dG_0 @ W_hh, each [n, B, H]."""
    return _bwd(dh_out, dc_in, w_hh, act, cs, torch.float64)


def plain32(which: str, *args):
    """The same restatement ('fwd' or 'bwd') in torch float32 on the CPU."""
    return {"fwd": _fwd, "bwd": _bwd}[which](*args, torch.float32)


def weight_grads64(dG, hs, x):
    """(dW_hh, dW_ih, db) of the loop: dG^T H_prev, dG^T X and sum dG, float64."""
    n, L, B, G = dG.shape
    dGf = dG.double().reshape(n, L * B, G)
    hp = hs.double()[:, :L].reshape(n, L * B, -1)
    xf = x.double().reshape(1, L * B, -1)
    return dGf.transpose(1, 2) @ hp, dGf.transpose(1, 2) @ xf, dGf.sum(1)


# ----------------------------------------------------------------- comparator
def slice_ratios(got, ref64, p32):
    """Per leading-two-axes slice ([n, T, ...]): (max|got - ref64|, the
    yardstick max(max|p32 - ref64|, u max|ref64|))."""
    n, T = ref64.shape[:2]
    r = ref64.reshape(n, T, -1)
    err = (got.double().reshape(n, T, -1) - r).abs().amax(-1)
    yard = torch.maximum((p32.double().reshape(n, T, -1) - r).abs().amax(-1), U * r.abs().amax(-1))
    return err, yard


def lstm_bound(ref64, p32, factor: Optional[float] = None):
    """The comparator's tolerance as an entrywise bound shaped like ref64."""
    n, T = ref64.shape[:2]
    _, yard = slice_ratios(ref64, ref64, p32)
    f = F if factor is None else factor
    return (f * yard).reshape(n, T, *([1] * (ref64.dim() - 2))).expand_as(ref64)


RATIOS = {}   # what -> the worst ratio seen in this process (the measurement behind F)


def assert_lstm_close(got, ref64, p32, what: str, factor: Optional[float] = None):
    """got, ref64, p32 shaped [n_lstm, steps, ...]: per LSTM and per step,
    max|got - ref64| <= F max(max|p32 - ref64|, u max|ref64|)."""
    f = F if factor is None else factor
    assert got.shape == ref64.shape == p32.shape, (what, got.shape, ref64.shape, p32.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    err, yard = slice_ratios(got, ref64, p32)
    ratio = err / yard.clamp_min(1e-300)
    worst = float(ratio.max())
    key = what.split(":")[-1].strip()
    RATIOS[key] = max(RATIOS.get(key, 0.0), worst)
    print(f"RATIO {what} {worst:.4f}")
    bad = err > f * yard
    at = divmod(int(ratio.argmax()), ratio.shape[1])
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} (LSTM, step) slices beyond {f} x the "
                                 f"f32 yardstick, worst ratio {worst:.3g} at (LSTM, step) {at}")


def by_lstm(act):
    """act [L, n, B, 4H] -> [n, L, B, 4H] (the comparator's slice order)."""
    return act.transpose(0, 1)


def states(t):
    """[n, B, H] -> [n, 1, B, H]."""
    return t.unsqueeze(1)


# -------------------------------------------------------------------- buffers
def flat(dev, numel: int, data: Optional[torch.Tensor] = None) -> Slab:
    """A flat guarded array of `numel` floats (gemm_helpers.Slab of one row):
    SENTINEL -- a NaN -- in both bands and, until `data` is put, in the
    interior too, so an output's unwritten floats and any over-read are NaN."""
    s = Slab(dev, 1, 1, numel)
    if data is not None:
        s.put(data.reshape(1, 1, numel).float())
    return s


def view(s: Slab, *shape) -> torch.Tensor:
    return s.mat(0).reshape(-1).view(*shape)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32).cpu()


__all__ = ["CASES", "F", "U", "SENTINEL", "Slab", "seq_geometry", "block_of", "make_inputs", "lstm_ref64",
           "lstm_bwd_ref64", "plain32", "weight_grads64", "assert_lstm_close", "lstm_bound", "slice_ratios", "flat",
           "view", "bits", "by_lstm", "states", "RATIOS"]
