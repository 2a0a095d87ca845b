"""The collector's matrix-core kernels through the raw ABI against the float64
restatements of tests/collect_mfma_helpers.py: vn_lstm_fused_bf16 and
vn_lstm_fused_bf16_masked (csrc/voxnav_collect.hip), vn_lstm_fused_f32,
vn_linear_f32 and vn_mlp_head_f32 (csrc/voxnav_policy_f32.hip).

* Every pointer argument sits in a guarded slab (sentinel NaN bands both sides,
  the sentinel inside every output); every input is bit-compared after the
  launch, every guard band checked.
* The case tables of the helpers reach both block decodes of each kernel, both
  VEC_X and both MASK instantiations of each LSTM, one-row and exact tiles,
  n_lstm 1 on a weight slice, every H, a Kp beyond the minimum, padded row
  strides, every layer count and action count, and the persistent LSTM's
  multi-item walk (tests/test_collect_mfma_helpers_cpu.py asserts what each
  case reaches and proves the checks against seeded defects).
* Exact data: c and h within 2e-6 + 2e-6 |f64|; c_store bitwise c, h32 bitwise
  h_store, the bf16 h_out bitwise the round-to-nearest-even bf16 of the
  kernel's own h_store (f2bf of csrc/voxnav_collect.hip rounds that way); the
  masked entries bitwise the plain entry on the masked state, finite although
  the starting rows of c_in (and of h_in for f32) hold NaN; the linear
  identity epilogue bitwise float32(exact sum), Tanh within 1e-6 + 1e-5 |y|.
* One generic-data case per LSTM entry and for the linear kernel within the
  bound derived from the inputs (the helpers' docstring).
* MLP head: values and log-probs within 2e-5 + 2e-5 |x|, the deterministic
  action the float64 arg-max, a sampled action off the float64 draw only
  within 1e-5 of a CDF boundary and at most twice per launch; seed, t and
  agent_id_base each move the draw.
* A relaunch is bit-stable, a side stream gives the default stream's bits,
  refusals return non-zero and leave every output's sentinel.

Measured on an MI355X (torch 2.10.0+rocm7.0), maximum |gpu - f64| over the
case tables and the largest share of the bound used:
  bf16 LSTM, exact data     c 4.1e-7 (11 %), h 2.5e-7 (12 %); h_out, the copies
                            and the masked entry bit for bit as stated
  f32 LSTM, exact data      c 6.5e-7 (13 %), h 3.1e-7 (13 %), both at the
                            multi-item cases (528 and 576 items on 512 blocks)
  bf16 LSTM, generic data   c 3.6e-7 (0.3 %), h 1.8e-7 (0.4 % of the derived bound)
  f32 LSTM, generic data    c 4.1e-7 (1.4 %), h 1.8e-7 (2.2 %)
  linear, Tanh              1.7e-7 (7 %); generic data 2.8e-6 (1.7 %)
  MLP head                  values 4.9e-7 (1.6 %), log-probs 1.4e-6 (2.9 %); no
                            sampled action differed from the float64 draw
The derived bounds are worst-case summation bounds (K u sum |a||w|), which
random rounding errors do not approach.
"""
import ctypes as C
import functools
import itertools

import pytest
import torch

import collect_mfma_helpers as cm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _lib():
    from voxnav import _native
    return _native.load()


def _p(s, off_bytes=0):
    return None if s is None else C.c_void_p(s.ptr + off_bytes)


def _raw(stream):
    return None if stream is None else C.c_void_p(stream.cuda_stream)


def _sync(stream):
    (torch.cuda if stream is None else stream).synchronize()


def _ok(rc, what):
    assert rc == 0, f"{what}: {_lib().vn_last_error().decode(errors='replace')}"


def _guards(slabs, what):
    for name, s in slabs.items():
        if s is not None:
            assert s.intact(), f"{what}: guard band of {name} overwritten"


# ------------------------------------------------------------------ the LSTMs
@functools.lru_cache(maxsize=None)
def _case(kind, case, generic=False):
    d = cm.lstm_inputs(kind, case, generic)
    return d, cm.lstm_packed(d)


@functools.lru_cache(maxsize=None)
def _ref(kind, case, mode, generic=False):
    d, _ = _case(kind, case, generic)
    start = None if mode == "plain" else cm.starts(d, mode)
    big = d["N"] > 4096                     # the multi-item cases: float64 on the device
    ref = cm.lstm_ref(d, start, device=DEV if big else None)
    return ref, (cm.lstm_bound(d, ref, start) if generic else None)


def _weights(d, packed):
    """-> (slab, byte offset): n_lstm 1 takes the second LSTM's slice of a
    two-LSTM array whose first slice is NaN, as the critic's bootstrap call does."""
    mk = cm.hbuf if d["kind"] == "bf16" else cm.fbuf
    if d["n"] == 1:
        both = torch.cat([torch.full_like(packed, float("nan")), packed])
        return mk(DEV, both), packed.numel() * (2 if d["kind"] == "bf16" else 4)
    return mk(DEV, packed), 0


def run_bf16(kind_case, mode, opt=(True, True, True), stream=None, c_state=None, generic=False):
    """One launch of vn_lstm_fused_bf16 (mode 'plain'; c_state overrides the
    state it starts from) or vn_lstm_fused_bf16_masked (starts 'drawn', 'all',
    'none'; NaN in the starting rows of c_in) with every check of the buffers.
    opt: (h32, h_store, c_store) passed or NULL.  -> CPU arrays."""
    d, packed = _case("bf16", kind_case, generic)
    n, N, H, od, geo = d["n"], d["N"], d["H"], d["od"], d["geo"]
    numel = n * N * H
    what = f"bf16 {kind_case} {mode}"
    w, woff = _weights(d, packed)
    inp = dict(x=cm.fbuf(DEV, d["x"]), h_in=cm.hbuf(DEV, d["h_in"]), w=w, bias=cm.fbuf(DEV, d["bias"]))
    out = dict(h_out=cm.hbuf(DEV, numel=numel))
    masked = mode != "plain"
    if masked:
        start = cm.starts(d, mode)
        inp["start"] = cm.fbuf(DEV, start)
        inp["c_in"] = cm.fbuf(DEV, cm.poisoned(d["c0"], start))
        out["c"] = cm.fbuf(DEV, numel=numel)
        out["h_store"] = cm.fbuf(DEV, numel=numel) if opt[1] else None
    else:
        out["c"] = cm.fbuf(DEV, d["c0"] if c_state is None else c_state)
        for k, given in zip(("h32", "h_store", "c_store"), opt):
            out[k] = cm.fbuf(DEV, numel=numel) if given else None
    snap = cm.snapshot(inp.values())
    torch.cuda.synchronize()
    if masked:
        rc = _lib().vn_lstm_fused_bf16_masked(_p(inp["x"]), od, _p(inp["h_in"]), _p(w, woff), geo["Kp"], _p(inp["bias"]),
                                              _p(inp["c_in"]), _p(inp["start"]), _p(out["c"]), _p(out["h_out"]),
                                              _p(out["h_store"]), n, N, H, _raw(stream))
    else:
        rc = _lib().vn_lstm_fused_bf16(_p(inp["x"]), od, _p(inp["h_in"]), _p(w, woff), geo["Kp"], _p(inp["bias"]),
                                       _p(out["c"]), _p(out["h_out"]), _p(out["h32"]), _p(out["h_store"]),
                                       _p(out["c_store"]), n, N, H, _raw(stream))
    _ok(rc, what)
    _sync(stream)
    assert cm.unchanged(inp.values(), snap), f"{what}: an input was written"
    _guards({**inp, **out}, what)
    res = {k: cm.view(s, n, N, H).cpu() for k, s in out.items() if s is not None and k != "h_out"}
    res["hb"] = cm.bf16_bits(cm.hview(out["h_out"]).view(n, N, H).cpu())
    res["h"] = res.get("h_store", res.get("h32"))
    return res


def _same(a, b, keys, what):
    for k in keys:
        assert torch.equal(cm.bits(a[k]), cm.bits(b[k])), f"{what}: {k} differs bit for bit"


@pytest.mark.parametrize("case", list(cm.BF16_CASES))
def test_bf16_plain(case):
    d, _ = _case("bf16", case)
    out = run_bf16(case, "plain")
    cm.check_lstm(d, _ref("bf16", case, "plain")[0], out, f"bf16 {case} plain")
    _same(out, run_bf16(case, "plain"), ("c", "hb", "h32", "h_store", "c_store"), "relaunch")


@pytest.mark.parametrize("case", list(cm.BF16_CASES))
def test_bf16_masked(case):
    d, _ = _case("bf16", case)
    out = run_bf16(case, "drawn")
    cm.check_lstm(d, _ref("bf16", case, "drawn")[0], out, f"bf16 {case} masked")
    plain = run_bf16(case, "plain", c_state=cm.masked_state(d["c0"], d["start"]))
    _same(out, plain, ("c", "hb", "h_store"), "the masked entry against the plain entry on the masked state")


@pytest.mark.parametrize("case", cm.BF16_ALL_NONE)
@pytest.mark.parametrize("mode", ["all", "none"])
def test_bf16_start_everywhere_and_nowhere(case, mode):
    d, _ = _case("bf16", case)
    out = run_bf16(case, mode)
    cm.check_lstm(d, _ref("bf16", case, mode)[0], out, f"bf16 {case} start {mode}")
    plain = run_bf16(case, "plain", c_state=cm.masked_state(d["c0"], cm.starts(d, mode)))
    _same(out, plain, ("c", "hb", "h_store"), f"start {mode} against the plain entry")


@pytest.mark.parametrize("case", ["critic", "scalar31"])
def test_bf16_optional_outputs(case):
    full = run_bf16(case, "plain")
    for opt in itertools.product((False, True), repeat=3):
        if all(opt):
            continue
        got = run_bf16(case, "plain", opt=opt)
        _same(got, full, ["c", "hb"] + [k for k, g in zip(("h32", "h_store", "c_store"), opt) if g], f"outputs {opt}")
    _same(run_bf16(case, "drawn", opt=(False, False, False)), run_bf16(case, "drawn"), ("c", "hb"), "masked, h_store NULL")


def test_bf16_generic_within_the_derived_bound():
    case = cm.BF16_GENERIC
    d, _ = _case("bf16", case, True)
    for mode in ("plain", "drawn"):
        ref, bound = _ref("bf16", case, mode, True)
        cm.check_lstm(d, ref, run_bf16(case, mode, generic=True), f"bf16 generic {mode}", bound)


def test_bf16_side_stream():
    s = torch.cuda.Stream()
    for mode in ("plain", "drawn"):
        _same(run_bf16("swz16", mode, stream=s), run_bf16("swz16", mode), ("c", "hb", "h_store"), f"side stream {mode}")


def run_f32(case, mode, inplace=False, stream=None, state=None, generic=False):
    """One launch of vn_lstm_fused_f32: mode 'plain' (start NULL; state =
    (h_in, c_in) overrides the inputs) or masked with the starts 'drawn', 'all',
    'none' and NaN in the starting rows of h_in and c_in.  -> CPU arrays, or
    device arrays for the multi-item cases."""
    d, packed = _case("f32", case, generic)
    n, N, H, od, geo = d["n"], d["N"], d["H"], d["od"], d["geo"]
    numel = n * N * H
    what = f"f32 {case} {mode}{' in place' if inplace else ''}"
    w, woff = _weights(d, packed)
    h_in, c_in = (d["h_in"], d["c0"]) if state is None else state
    masked = mode != "plain"
    inp = dict(x=cm.fbuf(DEV, d["x"]), w=w, bias=cm.fbuf(DEV, d["bias"]))
    if masked:
        start = cm.starts(d, mode)
        inp["start"] = cm.fbuf(DEV, start)
        h_in, c_in = cm.poisoned(h_in, start), cm.poisoned(c_in, start)
    inp["h_in"] = cm.fbuf(DEV, h_in)
    c_slab = cm.fbuf(DEV, c_in)
    if not inplace:
        inp["c_in"] = c_slab
    out = dict(c=c_slab if inplace else cm.fbuf(DEV, numel=numel), h=cm.fbuf(DEV, numel=numel))
    snap = cm.snapshot(inp.values())
    torch.cuda.synchronize()
    rc = _lib().vn_lstm_fused_f32(_p(inp["x"]), od, _p(inp["h_in"]), _p(w, woff), geo["Kp"], _p(inp["bias"]), _p(c_slab),
                                  _p(inp.get("start")), _p(out["c"]), _p(out["h"]), n, N, H, _raw(stream))
    _ok(rc, what)
    _sync(stream)
    assert cm.unchanged(inp.values(), snap), f"{what}: an input was written"
    _guards({**inp, **out}, what)
    res = {k: cm.view(s, n, N, H) for k, s in out.items()}
    return res if N > 4096 else {k: v.cpu() for k, v in res.items()}


@pytest.mark.parametrize("case", list(cm.F32_CASES))
def test_f32_plain(case):
    d, _ = _case("f32", case)
    out = run_f32(case, "plain")
    cm.check_lstm(d, _ref("f32", case, "plain")[0], out, f"f32 {case} plain")
    _same(out, run_f32(case, "plain"), ("c", "h"), "relaunch")
    _same(out, run_f32(case, "plain", inplace=True), ("c", "h"), "c_in == c_out")


@pytest.mark.parametrize("case", list(cm.F32_CASES))
def test_f32_masked(case):
    d, _ = _case("f32", case)
    out = run_f32(case, "drawn")
    cm.check_lstm(d, _ref("f32", case, "drawn")[0], out, f"f32 {case} masked")
    _same(out, run_f32(case, "drawn", inplace=True), ("c", "h"), "masked, c_in == c_out")
    zeroed = (cm.masked_state(d["h_in"], d["start"]), cm.masked_state(d["c0"], d["start"]))
    _same(out, run_f32(case, "plain", state=zeroed), ("c", "h"), "the masked launch against start NULL on the masked state")


@pytest.mark.parametrize("case", cm.F32_ALL_NONE)
@pytest.mark.parametrize("mode", ["all", "none"])
def test_f32_start_everywhere_and_nowhere(case, mode):
    d, _ = _case("f32", case)
    out = run_f32(case, mode)
    cm.check_lstm(d, _ref("f32", case, mode)[0], out, f"f32 {case} start {mode}")
    st = cm.starts(d, mode)
    zeroed = (cm.masked_state(d["h_in"], st), cm.masked_state(d["c0"], st))
    _same(out, run_f32(case, "plain", state=zeroed), ("c", "h"), f"start {mode} against start NULL")


@pytest.mark.parametrize("case", list(cm.F32_MULTI))
@pytest.mark.parametrize("mode", ["plain", "drawn"])
def test_f32_multi_item_walk(case, mode):
    d, _ = _case("f32", case)
    slots = cm.ls_slots(torch.cuda.get_device_properties(0).multi_processor_count)
    if d["geo"]["n_items"] <= slots:
        pytest.skip(f"{d['geo']['n_items']} items fit the {slots} persistent blocks of this device: no block walks two")
    assert d["geo"]["n_items"] > slots
    out = run_f32(case, mode)
    cm.check_lstm(d, _ref("f32", case, mode)[0], out, f"f32 {case} {mode}")


def test_f32_generic_within_the_derived_bound():
    case = cm.F32_GENERIC
    d, _ = _case("f32", case, True)
    for mode in ("plain", "drawn"):
        ref, bound = _ref("f32", case, mode, True)
        cm.check_lstm(d, ref, run_f32(case, mode, generic=True), f"f32 generic {mode}", bound)


def test_f32_side_stream():
    s = torch.cuda.Stream()
    for mode in ("plain", "drawn"):
        _same(run_f32("swz8", mode, stream=s), run_f32("swz8", mode), ("c", "h"), f"side stream {mode}")


# ------------------------------------------------------------------ vn_linear_f32
def _arr(slabs, offs=None):
    offs = offs or [0] * len(slabs)
    return (C.c_void_p * len(slabs))(*[None if s is None else s.ptr + o for s, o in zip(slabs, offs)])


@functools.lru_cache(maxsize=None)
def _lin_case(case, generic=False):
    d = cm.linear_inputs(case, generic)
    refs = {act: cm.linear_ref(d, act) for act in (False, True)}
    return d, refs


def run_linear(case, act, stream=None, generic=False):
    d, _ = _lin_case(case, generic)
    M, K, Nout, nb = d["M"], d["K"], d["Nout"], d["nb"]
    what = f"linear {case} act {int(act)}"
    xs = [cm.fbuf(DEV, cm.padded_rows(x, d["ldx"])) for x in d["xs"]]
    ws = [cm.fbuf(DEV, cm.pack_linear_f32_ref(w)) for w in d["ws"]]
    bs = [cm.fbuf(DEV, b) for b in d["bs"]]
    ys = [cm.fbuf(DEV, numel=M * Nout) for _ in range(nb)]
    snap = cm.snapshot(xs + ws + bs)
    torch.cuda.synchronize()
    _ok(_lib().vn_linear_f32(nb, _arr(xs), d["ldx"], _arr(ws), _arr(bs), _arr(ys), M, K, Nout, int(act), _raw(stream)), what)
    _sync(stream)
    assert cm.unchanged(xs + ws + bs, snap), f"{what}: an input was written"
    _guards({f"{k}{i}": s for k, sl in (("x", xs), ("w", ws), ("b", bs), ("y", ys)) for i, s in enumerate(sl)}, what)
    return [cm.view(y, M, Nout).cpu() for y in ys]


@pytest.mark.parametrize("case", list(cm.LINEAR_CASES))
@pytest.mark.parametrize("act", [False, True])
def test_linear(case, act):
    d, refs = _lin_case(case)
    ys = run_linear(case, act)
    cm.check_linear(d, refs[act], ys, act, f"linear {case}")
    again = run_linear(case, act)
    assert all(torch.equal(cm.bits(a), cm.bits(b)) for a, b in zip(ys, again)), "relaunch differs"
    if d["nb"] == 2:
        assert not torch.equal(ys[0], ys[1]), "the two branches returned the same array"


def test_linear_generic_and_side_stream():
    case = cm.LINEAR_GENERIC
    d, refs = _lin_case(case, True)
    for act in (False, True):
        cm.check_linear(d, refs[act], run_linear(case, act, generic=True), act, "linear generic",
                        cm.linear_bounds(d, refs[act], act))
    s = torch.cuda.Stream()
    a, b = run_linear("swz8", True, stream=s), run_linear("swz8", True)
    assert all(torch.equal(cm.bits(u), cm.bits(v)) for u, v in zip(a, b)), "side stream differs"


# ---------------------------------------------------------------- vn_mlp_head_f32
@functools.lru_cache(maxsize=None)
def _head_case(case):
    d = cm.head_inputs(case)
    return d, cm.head_ref(d)


def _head_slabs(d):
    s = dict(xs=[cm.fbuf(DEV, cm.padded_rows(x, d["ldx"])) for x in d["xs"]],
             ws=[cm.fbuf(DEV, cm.pack_mlp_head_f32_ref(w)) for ls in d["layers"] for w, _ in ls],
             bs=[cm.fbuf(DEV, b) for ls in d["layers"] for _, b in ls],
             wv=cm.fbuf(DEV, d["wv"]), bv=cm.fbuf(DEV, d["bv"]), wa=None, ba=None)
    if d["nb"] == 2:
        s["wa"], s["ba"] = cm.fbuf(DEV, d["wa"]), cm.fbuf(DEV, d["ba"])
    return s


def _head_call(d, s, o, det, draw, stream=None, **over):
    a = dict(nb=d["nb"], x=_arr(s["xs"]), ldx=d["ldx"], K0=d["K0"], nl=len(d["widths"]), widths=d["widths"],
             w=_arr(s["ws"]), b=_arr(s["bs"]), wa=_p(s["wa"]), ba=_p(s["ba"]), A=d["A"], wv=_p(s["wv"]), bv=_p(s["bv"]),
             actions=_p(o["actions"]), log_probs=_p(o["log_probs"]), values=_p(o["values"]), M=d["M"])
    a.update(over)
    widths = (C.c_int32 * len(a["widths"]))(*a["widths"]) if a["widths"] is not None else None
    return _lib().vn_mlp_head_f32(a["nb"], a["x"], a["ldx"], a["K0"], a["nl"], widths, a["w"], a["b"], a["wa"], a["ba"],
                                  a["A"], a["wv"], a["bv"], draw[0], draw[1], draw[2], int(det), a["actions"],
                                  a["log_probs"], a["values"], a["M"], _raw(stream))


def _head_outputs(d):
    return {k: cm.fbuf(DEV, numel=d["M"]) for k in ("actions", "log_probs", "values")}


def run_head(case, det, draw, stream=None):
    d, _ = _head_case(case)
    what = f"head {case} det {int(det)}"
    s, o = _head_slabs(d), _head_outputs(d)
    ins = s["xs"] + s["ws"] + s["bs"] + [v for v in (s["wv"], s["bv"], s["wa"], s["ba"]) if v is not None]
    snap = cm.snapshot(ins)
    torch.cuda.synchronize()
    _ok(_head_call(d, s, o, det, draw, stream), what)
    _sync(stream)
    assert cm.unchanged(ins, snap), f"{what}: an input was written"
    _guards({**{f"in{i}": v for i, v in enumerate(ins)}, **o}, what)
    res = dict(values=cm.view(o["values"], d["M"]).cpu())
    if d["nb"] == 2:
        res["actions"] = cm.iview(o["actions"]).cpu().clone()
        res["log_probs"] = cm.view(o["log_probs"], d["M"]).cpu()
    else:
        assert o["actions"].untouched() and o["log_probs"].untouched(), f"{what}: a value-only launch wrote a pi output"
    return res


def _same_head(a, b, what):
    for k in a:
        assert torch.equal(cm.bits(a[k]), cm.bits(b[k])), f"{what}: {k} differs"


@pytest.mark.parametrize("case", list(cm.HEAD_CASES))
@pytest.mark.parametrize("det", [True, False])
def test_mlp_head(case, det):
    d, ref = _head_case(case)
    for draw in cm.DRAWS:
        out = run_head(case, det, draw)
        n_diff = cm.check_head(d, ref, out, det, draw, f"head {case} det {int(det)}")
        print(f"DRAWS head {case}: {n_diff} sampled actions differ from the float64 draw")
    _same_head(out, run_head(case, det, cm.DRAWS[1]), "relaunch")


def test_mlp_head_draw_keys_and_side_stream():
    """seed, t and agent_id_base each move the draw: with one of them changed
    the actions are the float64 draw of the changed uniforms, which differ."""
    case = "m300"
    d, ref = _head_case(case)
    (s0, t0, b0), (s1, t1, b1) = cm.DRAWS
    base = run_head(case, False, cm.DRAWS[0])
    for draw in ((s1, t0, b0), (s0, t1, b0), (s0, t0, b1)):
        out = run_head(case, False, draw)
        cm.check_head(d, ref, out, False, draw, f"head {case} draw {draw}")
        assert not torch.equal(out["actions"], base["actions"])
        _same_head({"values": out["values"]}, {"values": base["values"]}, "the draw moved the values")
    s = torch.cuda.Stream()
    _same_head(run_head(case, False, cm.DRAWS[0], stream=s), base, "side stream")


# ------------------------------------------------------------------- refusals
def _refused(rc, outs, what):
    assert rc != 0, f"{what}: accepted"
    torch.cuda.synchronize()
    for s in outs:
        assert s.untouched(), f"{what}: an output was written"


def test_bf16_refusals():
    d, packed = _case("bf16", "one_tile")
    n, N, H, od, Kp = d["n"], d["N"], d["H"], d["od"], d["geo"]["Kp"]
    numel = n * N * H
    a = dict(x=cm.fbuf(DEV, d["x"]), od=od, h_in=cm.hbuf(DEV, d["h_in"]), w=cm.hbuf(DEV, packed), Kp=Kp,
             bias=cm.fbuf(DEV, d["bias"]), c=cm.fbuf(DEV, numel=numel), h_out=cm.hbuf(DEV, numel=numel),
             h32=cm.fbuf(DEV, numel=numel), h_store=cm.fbuf(DEV, numel=numel), c_store=cm.fbuf(DEV, numel=numel),
             n=n, N=N, H=H, c_in=cm.fbuf(DEV, d["c0"]), start=cm.fbuf(DEV, d["start"]))
    outs = [a[k] for k in ("c", "h_out", "h32", "h_store", "c_store")]
    assert (d["geo"]["K"], Kp) == (96, 128)

    def plain(**o):
        v = dict(a, **o)
        g = lambda k: v[k] if isinstance(v[k], int) or v[k] is None else _p(v[k])  # noqa: E731
        return _lib().vn_lstm_fused_bf16(g("x"), v["od"], g("h_in"), g("w"), v["Kp"], g("bias"), g("c"), g("h_out"),
                                         g("h32"), g("h_store"), g("c_store"), v["n"], v["N"], v["H"], None)

    def masked(**o):
        v = dict(a, **o)
        g = lambda k: None if v[k] is None else _p(v[k])  # noqa: E731
        return _lib().vn_lstm_fused_bf16_masked(g("x"), v["od"], g("h_in"), g("w"), v["Kp"], g("bias"), g("c_in"),
                                                g("start"), g("c"), g("h_out"), g("h_store"), v["n"], v["N"], v["H"], None)

    for k in ("x", "h_in", "w", "bias", "c", "h_out"):
        _refused(plain(**{k: None}), outs, f"plain, {k} NULL")
        _refused(masked(**{k: None}), outs, f"masked, {k} NULL")
    _refused(masked(c_in=None), outs, "masked, c_in NULL")
    _refused(masked(start=None), outs, "masked, start NULL")
    _refused(masked(c=a["c_in"]), outs, "masked, c_in == c_out")
    _refused(plain(h_out=a["h_in"]), outs, "h_in == h_out")
    _refused(masked(h_out=a["h_in"]), outs, "masked, h_in == h_out")
    for over in (dict(H=32), dict(H=96), dict(Kp=Kp + 8), dict(Kp=64), dict(N=0), dict(n=0), dict(od=0)):
        _refused(plain(**over), outs, f"plain {over}")
        _refused(masked(**over), outs, f"masked {over}")
    assert cm.unchanged([a["c_in"]], [cm.fbuf(DEV, d["c0"]).raw])


def test_f32_refusals():
    d, packed = _case("f32", "one_tile")
    n, N, H, od, Kp = d["n"], d["N"], d["H"], d["od"], d["geo"]["Kp"]
    numel = n * N * H
    a = dict(x=cm.fbuf(DEV, d["x"]), od=od, h_in=cm.fbuf(DEV, d["h_in"]), w=cm.fbuf(DEV, packed), Kp=Kp,
             bias=cm.fbuf(DEV, d["bias"]), c_in=cm.fbuf(DEV, d["c0"]), start=cm.fbuf(DEV, d["start"]),
             c=cm.fbuf(DEV, numel=numel), h=cm.fbuf(DEV, numel=numel), n=n, N=N, H=H)
    outs = [a["c"], a["h"]]
    assert od % 4 == 0        # the launcher then checks x's alignment too

    def call(off=None, **o):
        v = dict(a, **o)
        g = lambda k: None if v[k] is None else _p(v[k], 4 if k == off else 0)  # noqa: E731
        return _lib().vn_lstm_fused_f32(g("x"), v["od"], g("h_in"), g("w"), v["Kp"], g("bias"), g("c_in"), g("start"),
                                        g("c"), g("h"), v["n"], v["N"], v["H"], None)

    for k in ("x", "h_in", "w", "bias", "c_in", "c", "h"):
        _refused(call(**{k: None}), outs, f"{k} NULL")
    _refused(call(h=a["h_in"]), outs, "h_in == h_out")
    for over in (dict(H=32), dict(H=96), dict(Kp=Kp + 16), dict(Kp=Kp - 16), dict(od=3), dict(N=0), dict(n=0)):
        _refused(call(**over), outs, f"{over}")
    for k in ("x", "h_in", "w"):
        _refused(call(off=k), outs, f"{k} off 16-byte alignment")


def test_linear_refusals():
    d, _ = _lin_case("one_tile")
    M, K, Nout = d["M"], d["K"], d["Nout"]
    xs = [cm.fbuf(DEV, cm.padded_rows(x, K + 4)) for x in d["xs"]]
    ws = [cm.fbuf(DEV, cm.pack_linear_f32_ref(w)) for w in d["ws"]]
    bs = [cm.fbuf(DEV, b) for b in d["bs"]]
    ys = [cm.fbuf(DEV, numel=M * Nout) for _ in range(2)]

    def call(nb=2, x=xs, w=ws, b=bs, y=ys, ldx=K, M=M, K=K, Nout=Nout, xo=None, wo=None, null=None):
        arrs = dict(x=_arr(x, xo), w=_arr(w, wo), b=_arr(b), y=_arr(y))
        if null:
            arrs[null] = None
        return _lib().vn_linear_f32(nb, arrs["x"], ldx, arrs["w"], arrs["b"], arrs["y"], M, K, Nout, 1, None)

    for k in ("x", "w", "b", "y"):
        _refused(call(null=k), ys, f"{k} array NULL")
    for k, v in (("x", xs), ("w", ws), ("b", bs), ("y", ys)):
        _refused(call(**{k: [v[0], None]}), ys, f"{k}[1] NULL")
    for over in (dict(K=8), dict(K=24), dict(Nout=64), dict(ldx=K - 4), dict(ldx=K + 2), dict(nb=3), dict(nb=0), dict(M=0)):
        _refused(call(**over), ys, f"{over}")
    _refused(call(xo=[0, 4], ldx=K + 4), ys, "x[1] off 16-byte alignment")
    _refused(call(wo=[4, 0]), ys, "w_packed[0] off 16-byte alignment")


def test_mlp_head_refusals():
    d, _ = _head_case("m33")
    s, o = _head_slabs(d), _head_outputs(d)
    outs = list(o.values())
    nl = len(d["widths"])
    assert nl == cm.MH_MAXL and d["ldx"] > d["K0"]
    for over in (dict(nl=0), dict(nl=5, widths=d["widths"] + (128,)), dict(widths=(256, 64, 256, 128)), dict(K0=272, ldx=272),
                 dict(K0=24), dict(A=9), dict(A=0), dict(M=0), dict(nb=3), dict(ldx=d["K0"] - 4), dict(ldx=d["K0"] + 2),
                 dict(actions=None), dict(log_probs=None), dict(actions=None, log_probs=None), dict(values=None),
                 dict(wa=None), dict(ba=None), dict(wv=None), dict(bv=None), dict(x=None), dict(w=None), dict(b=None),
                 dict(widths=None)):
        _refused(_head_call(d, s, o, False, cm.DRAWS[0], **over), outs, f"{over}")
    _refused(_head_call(d, s, o, False, cm.DRAWS[0], x=_arr(s["xs"], [0, 4])), outs, "x[1] off 16-byte alignment")
    _refused(_head_call(d, s, o, False, cm.DRAWS[0], w=_arr(s["ws"], [0] * (2 * nl - 1) + [4])), outs,
             "a weight off 16-byte alignment")
    _refused(_head_call(d, s, o, False, cm.DRAWS[0], w=_arr(s["ws"][:-1] + [None])), outs, "a weight NULL")
