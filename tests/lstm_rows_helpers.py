"""Shared pieces of the row-layout LSTM tests (tests/test_lstm_rows_gpu.py,
tests/test_lstm_rows_helpers_cpu.py): the inputs of csrc/voxnav_learn_rows.hip
with everything a correct kernel never reads poisoned, float64 restatements of
one step, of the forward loop with its sequence starts and of the backward in
the ABI's own layouts, the same restatements in plain f32 (the yardstick of the
tolerance), guarded buffers for every pointer argument, and the checks both
test files run -- the GPU file on the kernels' arrays, the CPU file on the
restatement's own arrays with one defect seeded at a time.  Importing this
module needs no GPU.

Layouts (vn_lstm_rows_fwd / vn_lstm_rows_bwd in include/voxnav.h; two LSTMs
sharing x, gate order i, f, g, o; D 80, H 256):
  x [L, B, 80]   w_ih [2, 1024, 80]   w_hh [2, 1024, 256]   bias [2, 1024]
  h_store, c_store [L, 2, N, 256]   env [L, B] i32   start [L, B] u8
  keep [L, B]   hout, hprev, cprev, cnew [2, L, B, 256]   act, dG [2, L, B, 1024]
  dw_hh [2, 1024, 256]   dw_ih [2, 1024, 80]   db_ih, db_hh [2, 1024]
  cnt [2 NT 64] u32 (NT = ceil(B / 32); word 64 g is group g's counter)
  part: vn_lstm_rows_part_floats(B) floats
Step 0 starts a sequence in every row whatever start[0] says; at a start the
state is the stored one at (t, env[t, row]) times keep[t, row].

Poisoning.  Every (t, env) slot of h_store / c_store that no start of the case
reads is NaN, keep is NaN at every (t, row) that is no start, and env there
points at a NaN slot of that step (in range): a kernel that consults any of
them where it must not turns an output into NaN.

Tolerance.  ``assert_lstm_close`` (tests/lstm_seq_helpers.py) per LSTM and per
step -- the weight gradients per LSTM and per gate -- with the factor F_ROWS:
  max|got - ref64| <= F_ROWS max(max|p32 - ref64|, u max|ref64|),
p32 the f32 restatement of the reference on the same inputs (torch matmul,
torch.sigmoid / tanh), never the kernel.  The forward is compared one step at
a time from the kernel's own hprev / cprev, so its bound does not grow with L;
the backward from the kernel's own forward arrays.

Measured ratios max|got - ref64| / max(max|p32 - ref64|, u scale), the worst
slice of each compared array over the whole case table and every further run
of tests/test_lstm_rows_gpu.py (both forward layouts, the backward behind the
16-unit forward), with the case that gave it, on an MI355X:
  act   4.3287 (L1B1, 32 units; 16 units 3.9632, L1B1)
  cnew  3.1187 (L6B40none, 32 units; 16 units 2.9446, L3B33 cut to 32 rows)
  hout  3.6958 (L6B40none, 32 units; 16 units 3.5988, L6B40none)
  dG    1.8395 (L1B1)   dw_hh 2.9964 (L1B1)   dw_ih 3.1912 (L1B1)   db 3.6016 (L1B1)
(torch 2.10.0+rocm7.0).  The worst is 4.3287, twice it 8.657, so F_ROWS = 16:
the smallest power of two at least twice the worst ratio.  No array exceeds 8.
The forward ratios sit above those of the per-step loops (2.2 there) because
these kernels take the gates from the hardware exp and reciprocal (__expf,
__frcp_rn: about 4e-7 absolute, 6 to 7 u on a gate near 1) where the yardstick
uses torch's sigmoid and tanh; a one-row case has the smallest yardstick (the
maximum over 1024 entries instead of 1024 B), which is why L1B1 leads.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Optional

import torch

from gemm_helpers import SENTINEL, Slab
from lstm_seq_helpers import RATIOS, U, assert_lstm_close, bits, flat, slice_ratios, view

D, H = 80, 256
G4 = 4 * H
RW, CSTRIDE = 32, 64           # rows per tile, u32 words per group counter (csrc/voxnav_learn_rows.hip)
UNIT_BLOCKS = {1: 8, 2: 16}    # blocks per (LSTM, row tile) group: rows_layout 1 (32 units), 2 (16 units)
CNT_FILL = 0x7FFFFFFF          # what the counters hold on entry
F_ROWS = 16.0

# (L, B, N, p, start[0]): p the Bernoulli rate of start[1:], start[0] all "ones", all "zeros" or "mixed"
CASES = OrderedDict([
    ("L1B1", (1, 1, 8, 0.5, "ones")),        # one step, one live row: no hand-off, the backward's t == 0 break, 0 publishes
    ("L2B32", (2, 32, 8, 0.3, "mixed")),     # one full tile, one hand-off each way
    ("L3B33", (3, 33, 8, 0.3, "ones")),      # a full tile plus a one-row tile (31 dead rows clamped to B - 1)
    ("L4B31", (4, 31, 11, 0.3, "zeros")),    # a ragged single tile
    ("L5B97", (5, 97, 11, 0.25, "mixed")),   # NT 4 (97 = 3 x 32 + 1): the largest grid, a one-row tile behind full ones
    ("L4B95", (4, 95, 8, 0.25, "mixed")),    # NT 3: rows2_map's (g + NT) % G swap with odd NT, groups across blockIdx mod 8
    ("L8B64", (8, 64, 8, 0.15, "ones")),     # NT 2, seven hand-offs, both partial-dh slots used more than twice
    ("L3B40all", (3, 40, 8, 1.0, "ones")),   # every row starts at every step: no state crosses a step
    ("L6B40none", (6, 40, 8, 0.0, "zeros")),  # no start flagged at all: only the implicit one at t = 0
])


# ------------------------------------------------------------------- geometry
def part_floats(B: int) -> int:
    """The header's formula: two partial-dh slots [2][NT][16][32][256], the
    per-row-tile [dW_hh | dW_ih] partials and the per-row-tile db partials."""
    nt = -(-B // RW)
    return 2 * 2 * nt * 16 * RW * H + nt * 2 * G4 * (H + D) + nt * 2 * G4


def rows_geometry(L: int, B: int) -> dict:
    nt = -(-B // RW)
    writes = [t & 1 for t in range(1, L)]      # the backward's step t > 0 writes partial slot t & 1
    return dict(NT=nt, groups=2 * nt, last_tile_rows=B - RW * (nt - 1), cnt_words=2 * nt * CSTRIDE,
                grid={1: 2 * 8 * nt, 2: 2 * 16 * nt}, handoffs=L - 1,
                slot_writes=(writes.count(0), writes.count(1)), part_floats=part_floats(B))


def rows2_map(block: int, nt: int):
    """rows2_map of csrc/voxnav_learn_rows.hip: block id -> (unit block, group)
    of the 16-unit kernels; group g is (LSTM g // NT, row tile g % NT)."""
    G, half = 2 * nt, 8 * 2 * nt
    second = block >= half
    b = block - half if second else block
    ub, g = b // G + (8 if second else 0), b % G
    return ub, (g + nt) % G if second else g


# --------------------------------------------------------------------- inputs
def make_inputs(case: str) -> dict:
    """f32 CPU inputs of a case, seeded per case: nn.LSTM's default init
    (uniform in +-1 / sqrt(H); bias = b_ih + b_hh), standard-normal x and
    dh_out, stored states 0.5 x normal, keep 0 or 1, start Bernoulli(p) with
    the case's own start[0], and the poisoning of the module docstring.
    d["eff"] is start with step 0 forced: the starts the kernels act on."""
    L, B, N, p, start0 = CASES[case]
    g = torch.Generator()
    g.manual_seed(30310 + 137 * list(CASES).index(case))
    k = 1.0 / math.sqrt(H)
    uni = lambda *s: (torch.rand(s, generator=g) * 2.0 - 1.0) * k  # noqa: E731
    rnd = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    d = dict(case=case, L=L, B=B, N=N)
    d["w_ih"], d["w_hh"] = uni(2, G4, D), uni(2, G4, H)
    d["bias"] = uni(2, G4) + uni(2, G4)
    d["x"], d["dh_out"] = rnd(L, B, D), rnd(2, L, B, H)
    h_store, c_store = 0.5 * rnd(L, 2, N, H), 0.5 * rnd(L, 2, N, H)
    start = (torch.rand((L, B), generator=g) < p).to(torch.uint8)
    if start0 == "mixed":
        start[0] = (torch.rand((B,), generator=g) < 0.5).to(torch.uint8)
        start[0, 0], start[0, 1] = 1, 0
    else:
        start[0] = 1 if start0 == "ones" else 0
    eff = start.bool().clone()
    eff[0] = True
    keep01 = (torch.rand((L, B), generator=g) > 0.3).float()
    env = torch.zeros((L, B), dtype=torch.int32)
    read = torch.zeros((L, N), dtype=torch.bool)
    for t in range(L):
        st = eff[t]
        n_free = B - int(st.sum())
        e = torch.randint(0, N - 1 if n_free else N, (B,), generator=g)   # slot N - 1 stays unread while a row needs one
        read[t, e[st]] = True
        if n_free:
            free = (~read[t]).nonzero().flatten()
            e[~st] = free[torch.randint(0, len(free), (n_free,), generator=g)]
        env[t] = e.to(torch.int32)
    nan = float("nan")
    d["h_store"] = h_store.masked_fill(~read.view(L, 1, N, 1), nan)
    d["c_store"] = c_store.masked_fill(~read.view(L, 1, N, 1), nan)
    d["keep"] = torch.where(eff, keep01, torch.full_like(keep01, nan))
    d["env"], d["start"], d["eff"], d["read"] = env, start, eff, read
    return d


def first_rows(d: dict, B: int) -> dict:
    """The case cut to its first B rows (the stores stay whole)."""
    o = dict(d, B=B)
    for k in ("x", "env", "start", "eff", "keep"):
        o[k] = d[k][:, :B].contiguous()
    o["dh_out"] = d["dh_out"][:, :, :B].contiguous()
    return o


def lstms_exchanged(d: dict) -> dict:
    """The case with the two LSTMs' weights, biases, stored states and output
    gradients exchanged."""
    o = dict(d)
    for k in ("w_ih", "w_hh", "bias", "dh_out"):
        o[k] = d[k].flip(0).contiguous()
    for k in ("h_store", "c_store"):
        o[k] = d[k].flip(1).contiguous()
    return o


def stored_times_keep(d: dict, which: str) -> torch.Tensor:
    """[2, L, B, H] f32: the store `which` at (t, env[t, row]) times keep[t, row]
    -- one f32 product, what a start step must take bit for bit (NaN where the
    case poisoned it: at the steps that start nothing)."""
    L, B = d["L"], d["B"]
    tt = torch.arange(L).view(L, 1).expand(L, B)
    sel = d[which][tt, :, d["env"].long()]                     # [L, B, 2, H]
    return sel.permute(2, 0, 1, 3).float() * d["keep"].view(1, L, B, 1)


# ----------------------------------------------------------------- references
def _step(x, hp, cp, w_ih, w_hh, bias, dtype):
    x, hp, cp, w_ih, w_hh, bias = (t.to(dtype) for t in (x, hp, cp, w_ih, w_hh, bias))
    one = [1] * (hp.dim() - 3)
    wt = lambda w: w.transpose(1, 2).reshape(2, *one, w.shape[2], w.shape[1])  # noqa: E731
    # (a bias per sample, shaped like the pre-activations, lets autograd return dG as its gradient)
    pre = x.unsqueeze(0) @ wt(w_ih) + hp @ wt(w_hh) + (bias.reshape(2, *one, 1, G4) if bias.dim() == 2 else bias)
    i, f, o = (torch.sigmoid(pre[..., s * H:(s + 1) * H]) for s in (0, 1, 3))
    g = torch.tanh(pre[..., 2 * H:3 * H])
    c = f * cp + i * g
    return torch.cat([i, f, g, o], dim=-1), c, o * torch.tanh(c)


def _fwd(x, w_ih, w_hh, bias, h_store, c_store, env, start, keep, dtype, use_keep=True, lag=1):
    """use_keep / lag are the CPU self-test's seeded defects (keep ignored;
    h_{t-1} taken from hout[t - lag])."""
    h_store, c_store, keep = h_store.to(dtype), c_store.to(dtype), keep.to(dtype)
    L, B = start.shape
    hout, hprev, cprev, cnew, act = [], [], [], [], []
    for t in range(L):
        kp = keep[t].view(1, B, 1) if use_keep else 1.0
        h_in, c_in = h_store[t][:, env[t].long()] * kp, c_store[t][:, env[t].long()] * kp
        if t > 0:
            st = start[t].bool().view(1, B, 1)
            h_in = torch.where(st, h_in, hout[max(t - lag, 0)])
            c_in = torch.where(st, c_in, cnew[t - 1])
        a, c, h = _step(x[t], h_in, c_in, w_ih, w_hh, bias if bias.dim() == 2 else bias[:, t], dtype)
        for lst, v in ((hout, h), (hprev, h_in), (cprev, c_in), (cnew, c), (act, a)):
            lst.append(v)
    return tuple(torch.stack(v, 1) for v in (hout, hprev, cprev, cnew, act))


def _bwd(dh_out, w_hh, act, cprev, cnew, hprev, x, start, dtype, cut_dh=True, zero_dc=True):
    """cut_dh / zero_dc are the CPU self-test's seeded defects."""
    dh_out, w_hh, act, cprev, cnew, hprev, x = (t.to(dtype) for t in (dh_out, w_hh, act, cprev, cnew, hprev, x))
    L, B = start.shape
    st = start.bool().clone()
    st[0] = True
    dG = [None] * L
    dc = torch.zeros_like(dh_out[:, 0])
    for t in range(L - 1, -1, -1):
        dh = dh_out[:, t]
        if t < L - 1:
            rec = dG[t + 1] @ w_hh
            dh = dh + (torch.where(st[t + 1].view(1, B, 1), torch.zeros_like(rec), rec) if cut_dh else rec)
        i, f, g, o = (act[:, t, :, s * H:(s + 1) * H] for s in range(4))
        tc = torch.tanh(cnew[:, t])
        dcc = dc + (dh * o) * (1.0 - tc * tc)
        dG[t] = torch.cat([dcc * g * (i * (1.0 - i)), dcc * cprev[:, t] * (f * (1.0 - f)), dcc * i * (1.0 - g * g),
                           dh * tc * (o * (1.0 - o))], dim=-1)
        dc = dcc * f
        if zero_dc:
            dc = torch.where(st[t].view(1, B, 1), torch.zeros_like(dc), dc)
    dG = torch.stack(dG, 1)
    dGf = dG.reshape(2, L * B, G4).transpose(1, 2)
    return dG, dGf @ hprev.reshape(2, L * B, H), dGf @ x.reshape(1, L * B, D), dGf.sum(2)


def rows_step64(x_t, hprev_t, cprev_t, w_ih, w_hh, bias):
    """One step (or, with a leading L axis on x and behind the LSTM axis of the
    states, L independent steps) from given inputs, float64 -> act_t
    [2, ..., B, 4H], cnew_t, h_t [2, ..., B, H]."""
    return _step(x_t, hprev_t, cprev_t, w_ih, w_hh, bias, torch.float64)


def rows_fwd64(x, w_ih, w_hh, bias, h_store, c_store, env, start, keep):
    """The whole forward loop in float64 -> hout, hprev, cprev, cnew
    [2, L, B, H], act [2, L, B, 4H].  t = 0 always starts; at a start the state
    is the stored one times keep.  Differentiable (torch autograd)."""
    return _fwd(x, w_ih, w_hh, bias, h_store, c_store, env, start, keep, torch.float64)


def rows_bwd64(dh_out, w_hh, act, cprev, cnew, hprev, x, start):
    """The backward in float64 with the formulas of cell_bwd: dh_t = dh_out_t +
    [step t + 1 of the row is no start] dG_{t+1} @ W_hh, dc zeroed behind a
    start -> dG [2, L, B, 4H], dW_hh = sum dG^T hprev, dW_ih = sum dG^T x,
    db = sum dG."""
    return _bwd(dh_out, w_hh, act, cprev, cnew, hprev, x, start, torch.float64)


def plain32(which: str, *args, **defect):
    """The same restatement ('step', 'fwd' or 'bwd') in torch float32 on the CPU."""
    return {"step": _step, "fwd": _fwd, "bwd": _bwd}[which](*args, torch.float32, **defect)


FWD_IN = ("x", "w_ih", "w_hh", "bias", "h_store", "c_store", "env", "start", "keep")
FWD_OUT = ("hout", "hprev", "cprev", "cnew", "act")
BWD_OUT = ("dG", "dw_hh", "dw_ih", "db_ih", "db_hh")


def bwd_args(d: dict, fa: dict):
    """The backward's operands from a case and forward arrays `fa`."""
    return d["dh_out"], d["w_hh"], fa["act"], fa["cprev"], fa["cnew"], fa["hprev"], d["x"], d["start"]


# -------------------------------------------------------------------- buffers
def words(dev, n: int, data: Optional[torch.Tensor] = None, fill: Optional[int] = None) -> Slab:
    """`n` guarded 32-bit words (env, the counters): SENTINEL bands both sides."""
    s = Slab(dev, 1, 1, n)
    if fill is not None:
        s.raw[s.off0:s.off0 + n] = fill
    if data is not None:
        s.raw[s.off0:s.off0 + n] = data.reshape(n).to(torch.int32)
    return s


def byte_array(dev, n: int, data: torch.Tensor) -> Slab:
    """`n` guarded bytes (start); the pad up to a whole word keeps the sentinel."""
    s = Slab(dev, 1, 1, -(-n // 4))
    s.raw.view(torch.uint8)[4 * s.off0:4 * s.off0 + n] = data.reshape(n).to(torch.uint8)
    return s


def interior(s: Slab) -> torch.Tensor:
    """The payload words of a flat slab, as int32."""
    return s.raw[s.off0:s.off0 + s.cols]


class Bufs:
    """Every pointer argument of one case in a guarded slab on `dev`: inputs
    between NaN bands, outputs NaN inside too, the counters pre-filled with
    CNT_FILL, the workspace NaN-filled."""

    def __init__(self, dev, d: dict):
        self.dev, self.d, self.L, self.B = dev, d, d["L"], d["B"]
        self.nt = -(-self.B // RW)
        n = self.L * self.B
        self.inp = {k: flat(dev, d[k].numel(), d[k]) for k in ("x", "w_ih", "w_hh", "bias", "h_store", "c_store",
                                                                "keep", "dh_out")}
        self.inp["env"] = words(dev, n, d["env"])
        self.inp["start"] = byte_array(dev, n, d["start"])
        self.new_fwd()
        self.new_bwd()
        self.new_work()

    def new_fwd(self):
        n = 2 * self.L * self.B
        self.fwd = {k: flat(self.dev, n * (G4 if k == "act" else H)) for k in FWD_OUT}

    def new_bwd(self):
        sizes = dict(dG=2 * self.L * self.B * G4, dw_hh=2 * G4 * H, dw_ih=2 * G4 * D, db_ih=2 * G4, db_hh=2 * G4)
        self.bwd = {k: flat(self.dev, sizes[k]) for k in BWD_OUT}

    def new_work(self):
        self.cnt = words(self.dev, 2 * self.nt * CSTRIDE, fill=CNT_FILL)
        self.part = flat(self.dev, part_floats(self.B))

    def put_fwd(self, arrays):
        for k, t in zip(FWD_OUT, arrays):
            self.fwd[k].put(t.reshape(1, 1, -1).float())

    def put_bwd(self, dG, dw_hh, dw_ih, db):
        for k, t in zip(BWD_OUT, (dG, dw_hh, dw_ih, db, db)):
            self.bwd[k].put(t.reshape(1, 1, -1).float())

    def put_counters(self, per_group: int):
        """What a finished launch leaves: the range zeroed, word 64 g = per_group."""
        w = interior(self.cnt)
        w[:2 * self.nt * CSTRIDE] = 0
        w[0:2 * self.nt * CSTRIDE:CSTRIDE] = per_group

    def fwd_arrays(self) -> dict:
        L, B = self.L, self.B
        return {k: view(self.fwd[k], 2, L, B, G4 if k == "act" else H).cpu() for k in FWD_OUT}

    def bwd_arrays(self) -> dict:
        shapes = dict(dG=(2, self.L, self.B, G4), dw_hh=(2, G4, H), dw_ih=(2, G4, D), db_ih=(2, G4), db_hh=(2, G4))
        return {k: view(self.bwd[k], *shapes[k]).cpu() for k in BWD_OUT}

    def slabs(self, *groups):
        """(name, slab) of the named groups: 'inp', 'fwd', 'bwd', 'work'."""
        out = []
        for grp in groups:
            out += [("cnt", self.cnt), ("part", self.part)] if grp == "work" else list(getattr(self, grp).items())
        return out


# --------------------------------------------------------------------- checks
def check_guards(b: Bufs, *groups):
    for name, s in b.slabs(*groups):
        assert s.intact(), f"guard bands of {name} overwritten"


def check_counters(b: Bufs, per_group: int, behind: Optional[torch.Tensor] = None, nt: Optional[int] = None):
    """Word 64 g of each of the 2 NT groups equals per_group, every other word
    of the zeroed range is 0, the words behind it are as they were on entry
    (`behind`: the whole interior on entry) and the bands intact."""
    nt = b.nt if nt is None else nt
    n = 2 * nt * CSTRIDE
    w = interior(b.cnt).cpu()
    exp = torch.zeros(n, dtype=torch.int32)
    exp[::CSTRIDE] = per_group
    assert torch.equal(w[:n], exp), (f"counters: groups hold {w[:n:CSTRIDE].tolist()}, expected {per_group} each; "
                                     f"{int((w[:n] != exp).sum())} words of the zeroed range differ")
    if behind is not None:
        assert torch.equal(w[n:], behind.cpu()[n:]), "counter words behind the launch's range changed"
    assert b.cnt.intact(), "guard words round the counters overwritten"


def check_fwd_exact(d: dict, a: dict):
    """Finite everywhere; a step that starts nothing consumed, bit for bit, what
    the step before published (h) and carried (c); a start step took exactly
    stored x keep."""
    for k in FWD_OUT:
        bad = ~torch.isfinite(a[k])
        assert not bool(bad.any()), f"{k}: {int(bad.sum())} NaN / unwritten floats, first at {bad.nonzero()[0].tolist()}"
    eff = d["eff"]
    carried = ~eff[1:]
    for used, made in (("hprev", "hout"), ("cprev", "cnew")):
        u, m = bits(a[used])[:, 1:][:, carried], bits(a[made])[:, :-1][:, carried]
        assert torch.equal(u, m), (f"{used}[t] is not {made}[t-1] at {int((u != m).any(-1).sum())} of "
                                   f"{u.shape[0] * u.shape[1]} (LSTM, step, row) that start nothing")
    for used, store in (("hprev", "h_store"), ("cprev", "c_store")):
        u, m = bits(a[used])[:, eff], bits(stored_times_keep(d, store))[:, eff]
        assert torch.equal(u, m), (f"{used} at a start is not {store} x keep at {int((u != m).any(-1).sum())} of "
                                   f"{u.shape[0] * u.shape[1]} (LSTM, step, row)")


def check_fwd_close(d: dict, a: dict, what: str, factor: Optional[float] = None):
    """act, cnew and hout per LSTM and per step against rows_step64 from the
    arrays' own hprev / cprev."""
    args = (d["x"], a["hprev"], a["cprev"], d["w_ih"], d["w_hh"], d["bias"])
    ref, p32 = rows_step64(*args), plain32("step", *args)
    f = F_ROWS if factor is None else factor
    for i, k in enumerate(("act", "cnew", "hout")):
        assert_lstm_close(a[k], ref[i], p32[i], f"{what}: {k}", f)


def by_gate(t: torch.Tensor) -> torch.Tensor:
    """[2, 4H, ...] -> [2, 4, ...]: a slice per LSTM and per gate block of 256 rows."""
    return t.reshape(2, 4, -1)


def check_bwd(d: dict, fa: dict, ga: dict, what: str, factor: Optional[float] = None, with_dG: bool = True):
    """dG per LSTM and step, dW_hh / dW_ih / db per LSTM and gate against
    rows_bwd64 from the forward arrays `fa`; db_ih bit-equal to db_hh; every
    element written."""
    for k in BWD_OUT:
        if k == "dG" and not with_dG:
            continue
        bad = ~torch.isfinite(ga[k])
        assert not bool(bad.any()), f"{k}: {int(bad.sum())} NaN / unwritten floats, first at {bad.nonzero()[0].tolist()}"
    assert torch.equal(bits(ga["db_ih"]), bits(ga["db_hh"])), "db_ih differs from db_hh"
    ref, p32 = rows_bwd64(*bwd_args(d, fa)), plain32("bwd", *bwd_args(d, fa))
    f = F_ROWS if factor is None else factor
    if with_dG:
        assert_lstm_close(ga["dG"], ref[0], p32[0], f"{what}: dG", f)
    for i, k, name in ((1, "dw_hh", "dw_hh"), (2, "dw_ih", "dw_ih"), (3, "db_ih", "db")):
        assert_lstm_close(by_gate(ga[k]), by_gate(ref[i]), by_gate(p32[i]), f"{what}: {name}", f)


def check_all_fwd(b: Bufs, layout: int, what: str, factor: Optional[float] = None) -> dict:
    """Every check of a finished forward into b.fwd (exact ones first)."""
    a = b.fwd_arrays()
    check_fwd_exact(b.d, a)
    check_guards(b, "inp", "fwd", "work")
    check_counters(b, UNIT_BLOCKS[layout] * b.L)
    check_fwd_close(b.d, a, what, factor)
    return a


def check_all_bwd(b: Bufs, what: str, factor: Optional[float] = None, with_dG: bool = True) -> dict:
    """Every check of a finished backward into b.bwd behind the forward in b.fwd."""
    ga = b.bwd_arrays()
    check_guards(b, "inp", "fwd", "bwd", "work")
    check_counters(b, 16 * (b.L - 1))
    if not with_dG:
        assert b.bwd["dG"].untouched(), "dG written though not passed"
    check_bwd(b.d, b.fwd_arrays(), ga, what, factor, with_dG)
    return ga


__all__ = ["CASES", "F_ROWS", "U", "SENTINEL", "Slab", "RATIOS", "D", "H", "G4", "RW", "CSTRIDE", "UNIT_BLOCKS",
           "CNT_FILL", "FWD_IN", "FWD_OUT", "BWD_OUT", "part_floats", "rows_geometry", "rows2_map", "make_inputs",
           "first_rows", "lstms_exchanged", "stored_times_keep", "rows_step64", "rows_fwd64", "rows_bwd64", "plain32",
           "bwd_args", "words", "byte_array", "interior", "Bufs", "check_guards", "check_counters", "check_fwd_exact",
           "check_fwd_close", "check_bwd", "check_all_fwd", "check_all_bwd", "by_gate", "assert_lstm_close", "bits",
           "flat", "view", "slice_ratios"]
