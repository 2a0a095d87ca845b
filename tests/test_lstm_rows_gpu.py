"""The row-layout LSTM (csrc/voxnav_learn_rows.hip: vn_lstm_rows_fwd in both
forward layouts, vn_lstm_rows_bwd, vn_lstm_rows_part_floats) through the raw
ABI against the float64 restatements of tests/lstm_rows_helpers.py.

* Every pointer argument sits in a guarded slab: NaN bands both sides, NaN
  inside every output and the workspace, the counters pre-filled; stored
  states, keep and env are poisoned wherever a correct kernel never reads them.
* Forward, per case and forced layout: the hand-off (hprev[t] is hout[t-1],
  cprev[t] is cnew[t-1], a start took stored x keep) and the counters' final
  values exactly, then act, cnew and hout per LSTM and per step against
  float64 from the kernel's own hprev / cprev.
* Backward, per case behind the 16-unit forward: dG per LSTM and step, the
  weight and bias gradients per LSTM and gate, db_ih against db_hh, dG = NULL.
* Bit-exact invariances: a second launch, rows_prio, the automatic layout
  pick, 32 of 33 rows, the LSTMs exchanged, a side stream, a dirty workspace.
* Refusals launch nothing.
The err word is read after every launch; a hand-off that timed out fails the
test there and every later test of this file without another launch.
"""
import contextlib
import ctypes as C
import functools

import pytest
import torch

import lstm_rows_helpers as lr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INVALID = -1   # VN_ERR_INVALID
_TIMED_OUT = []


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not _lib().vn_lstm_rows_supported(lr.D, lr.H, 97):
        pytest.skip("row-layout kernels not co-resident on this device")
    if _TIMED_OUT:
        pytest.fail(f"a hand-off timed out in {_TIMED_OUT[0]}: nothing more is launched")


def _lib():
    from voxnav import _native
    return _native.load()


def _err():
    from voxnav import lstm_seq
    return lstm_seq._rows_err(torch.device(DEV))


def _last_error():
    return _lib().vn_last_error().decode(errors="replace")


def _p(slab):
    return None if slab is None else C.c_void_p(slab.ptr)


def _layout(v):
    from voxnav import _native
    return _native.option("rows_layout", v)


def _prio(v):
    from voxnav import _native
    return _native.option("rows_prio", v)


def _raw(stream):
    return None if stream is None else C.c_void_p(stream.cuda_stream)


def _fwd(b, stream=None, **over):
    a = dict(b.inp, **b.fwd, cnt=b.cnt, err=_err(), D=lr.D, H=lr.H, L=b.L, B=b.B, n_env=b.d["N"])
    a.update(over)
    err = None if a["err"] is None else C.c_void_p(a["err"].data_ptr())
    return _lib().vn_lstm_rows_fwd(_p(a["x"]), a["D"], _p(a["w_ih"]), _p(a["w_hh"]), _p(a["bias"]), _p(a["h_store"]),
                                   _p(a["c_store"]), a["n_env"], _p(a["env"]), _p(a["start"]), _p(a["keep"]),
                                   _p(a["hout"]), _p(a["hprev"]), _p(a["cprev"]), _p(a["cnew"]), _p(a["act"]),
                                   _p(a["cnt"]), err, a["L"], a["B"], a["H"], _raw(stream))


def _bwd(b, with_dG=True, stream=None, **over):
    a = dict(b.inp, **b.fwd, **b.bwd, cnt=b.cnt, part=b.part, err=_err(), H=lr.H, L=b.L, B=b.B)
    if not with_dG:
        a["dG"] = None
    a.update(over)
    err = None if a["err"] is None else C.c_void_p(a["err"].data_ptr())
    return _lib().vn_lstm_rows_bwd(_p(a["dh_out"]), _p(a["w_hh"]), _p(a["act"]), _p(a["cprev"]), _p(a["cnew"]),
                                   _p(a["hprev"]), _p(a["x"]), _p(a["start"]), _p(a["dG"]), _p(a["dw_hh"]),
                                   _p(a["dw_ih"]), _p(a["db_ih"]), _p(a["db_hh"]), _p(a["part"]), _p(a["cnt"]), err,
                                   a["L"], a["B"], a["H"], _raw(stream))


def _done(rc, what, stream=None):
    """Behind every launch: the return code, the launch finished, the err word."""
    assert rc == 0, f"{what}: {_last_error()}"
    if stream is None:
        torch.cuda.synchronize()
    else:
        stream.synchronize()
    if int(_err().item()) != 0:
        _err().zero_()
        _TIMED_OUT.append(what)
        pytest.fail(f"{what}: the err word is set -- an in-launch hand-off timed out")


def run_fwd(b, layout, what, stream=None, check=True):
    """A forward into fresh NaN outputs and a fresh workspace, with every check."""
    b.new_fwd()
    b.new_work()
    with _layout(layout):
        _done(_fwd(b, stream), what, stream)
    if check:
        lr.check_all_fwd(b, layout, what)
    return b.fwd_arrays()


def run_bwd(b, what, with_dG=True, stream=None, fresh_work=True):
    """A backward into fresh NaN outputs behind the forward in b.fwd, with every check."""
    before = {k: lr.bits(v) for k, v in b.fwd_arrays().items()}
    b.new_bwd()
    if fresh_work:
        b.new_work()
    _done(_bwd(b, with_dG, stream), what, stream)
    ga = lr.check_all_bwd(b, what, with_dG=with_dG)
    assert all(torch.equal(v, lr.bits(b.fwd_arrays()[k])) for k, v in before.items()), "the backward wrote a forward array"
    return ga


@functools.lru_cache(maxsize=None)
def _inputs(case):
    return lr.make_inputs(case)


@functools.lru_cache(maxsize=None)
def _forwarded(case):
    """The case's buffers behind a checked 16-unit forward (shared; a test that
    launches another forward into them does so on buffers of its own)."""
    b = lr.Bufs(DEV, _inputs(case))
    run_fwd(b, 2, f"{case} fwd16")
    return b


def _same(a, b, what):
    for k in a:
        if a[k] is not None and b[k] is not None:
            assert torch.equal(lr.bits(a[k]), lr.bits(b[k])), f"{what}: {k} differs"


# ------------------------------------------------------------------ a. forward
@pytest.mark.parametrize("layout", [1, 2])
@pytest.mark.parametrize("case", list(lr.CASES))
def test_forward_matches_float64_per_step(case, layout):
    if layout == 2:
        _forwarded(case)
    else:
        run_fwd(lr.Bufs(DEV, _inputs(case)), 1, f"{case} fwd32")


# ---------------------------------------------------------------- b. auto pick
@pytest.mark.parametrize("case", list(lr.CASES))
def test_auto_pick_is_the_16_unit_layout_up_to_one_block_per_cu(case):
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    d = _inputs(case)
    if 32 * -(-d["B"] // 32) > ncu:
        pytest.skip("the 16-unit grid exceeds one block per CU on this device")
    ref = _forwarded(case).fwd_arrays()
    b = lr.Bufs(DEV, d)
    b.new_fwd()
    with _layout(0):
        _done(_fwd(b), f"{case} fwd auto")
    lr.check_counters(b, 16 * b.L)
    _same(b.fwd_arrays(), ref, f"{case}: auto against layout 2")


# ----------------------------------------------------------------- c. backward
@pytest.mark.parametrize("case", list(lr.CASES))
def test_backward_matches_float64(case):
    b = _forwarded(case)
    with_dG = run_bwd(b, f"{case} bwd")
    without = run_bwd(b, f"{case} bwd, dG NULL", with_dG=False)
    _same({k: with_dG[k] for k in lr.BWD_OUT[1:]}, without, f"{case}: dG = NULL")


# -------------------------------------------------------------- d. invariances
def test_second_launch_gives_the_same_bits():
    b = lr.Bufs(DEV, _inputs("L5B97"))
    for layout in (1, 2):
        first = run_fwd(b, layout, f"fwd layout {layout}", check=False)
        _same(run_fwd(b, layout, f"fwd layout {layout} again"), first, f"forward layout {layout} relaunched")
    first = run_bwd(b, "bwd")
    _same(run_bwd(b, "bwd again"), first, "backward relaunched")


def test_rows_prio_does_not_change_a_bit():
    b = _forwarded("L8B64")
    ref_f = b.fwd_arrays()
    ref_b = run_bwd(b, "bwd prio 1")
    o = lr.Bufs(DEV, _inputs("L8B64"))
    with _prio(0):
        _same(run_fwd(o, 2, "fwd16 prio 0"), ref_f, "forward with rows_prio 0")
        _same(run_bwd(o, "bwd prio 0"), ref_b, "backward with rows_prio 0")


@pytest.mark.parametrize("layout", [1, 2])
def test_32_rows_of_33_do_not_depend_on_the_one_row_tile(layout):
    d = _inputs("L3B33")
    whole = run_fwd(lr.Bufs(DEV, d), layout, "B 33")
    part = run_fwd(lr.Bufs(DEV, lr.first_rows(d, 32)), layout, "B 32")
    _same(part, {k: v[:, :, :32] for k, v in whole.items()}, "rows 0..31 of B = 33 against B = 32")


def test_exchanged_lstms_give_exchanged_outputs():
    d = _inputs("L4B95")
    o = lr.Bufs(DEV, lr.lstms_exchanged(d))
    for layout in (1, 2):
        ref = run_fwd(lr.Bufs(DEV, d), layout, "fwd", check=False) if layout == 1 else _forwarded("L4B95").fwd_arrays()
        got = run_fwd(o, layout, f"fwd layout {layout}, LSTMs exchanged")
        _same({k: v.flip(0) for k, v in got.items()}, ref, f"forward layout {layout} with the LSTMs exchanged")
    ref_b = run_bwd(_forwarded("L4B95"), "bwd")
    got_b = run_bwd(o, "bwd, LSTMs exchanged")
    _same({k: v.flip(0) for k, v in got_b.items()}, ref_b, "backward with the LSTMs exchanged")


def test_side_stream_behind_a_stream_ordered_producer():
    """x (forward) and dh_out (backward) are overwritten with NaN and restored
    by copies on the side stream right in front of each launch; only that
    stream is synchronised."""
    d = _inputs("L5B97")
    ref_f = _forwarded("L5B97").fwd_arrays()
    ref_b = run_bwd(_forwarded("L5B97"), "bwd, default stream")
    b = lr.Bufs(DEV, d)
    x, dh = d["x"].to(DEV).reshape(-1), d["dh_out"].to(DEV).reshape(-1)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(DEV)
    with torch.cuda.stream(stream):
        for layout in (1, 2):
            b.new_fwd()
            b.new_work()
            lr.view(b.inp["x"], x.numel()).fill_(float("nan"))
            lr.view(b.inp["x"], x.numel()).copy_(x, non_blocking=True)
            with _layout(layout):
                _done(_fwd(b, stream), f"fwd layout {layout}, side stream", stream)
            lr.check_all_fwd(b, layout, f"fwd layout {layout}, side stream")
        _same(b.fwd_arrays(), ref_f, "forward on a side stream")
        b.new_bwd()
        b.new_work()
        lr.view(b.inp["dh_out"], dh.numel()).fill_(float("nan"))
        lr.view(b.inp["dh_out"], dh.numel()).copy_(dh, non_blocking=True)
        _done(_bwd(b, True, stream), "bwd, side stream", stream)
        _same(lr.check_all_bwd(b, "bwd, side stream"), ref_b, "backward on a side stream")
    torch.cuda.synchronize()


# --------------------------------------------------------- e. workspace reuse
def test_backward_on_a_dirty_workspace():
    """B = 97, then B = 31 on the same part and cnt (now holding the larger
    launch's partials and counters): equal to a run on fresh ones, and the
    counter words behind the smaller launch's range stay as they were."""
    big, small = _forwarded("L5B97"), _forwarded("L4B31")
    fresh = run_bwd(small, "B 31, fresh workspace")
    run_bwd(big, "B 97")
    entry = lr.interior(big.cnt).clone()
    own = (small.cnt, small.part, small.nt)
    try:
        small.cnt, small.part = big.cnt, big.part
        small.new_bwd()
        _done(_bwd(small), "B 31, dirty workspace")
        ga = small.bwd_arrays()
        lr.check_guards(small, "inp", "fwd", "bwd", "work")
        lr.check_counters(small, 16 * (small.L - 1), behind=entry)
        assert int(entry[2 * small.nt * lr.CSTRIDE]) == 16 * (big.L - 1)     # there was something to keep
        lr.check_bwd(small.d, small.fwd_arrays(), ga, "B 31, dirty workspace")
        _same(ga, fresh, "backward on a dirty workspace")
    finally:
        small.cnt, small.part, small.nt = own


# ----------------------------------------------------------------- f. refusals
def test_refusals_launch_nothing():
    """Each refusal stands in front of the counters' memset and the launch in
    vn_lstm_rows_fwd / vn_lstm_rows_bwd; hout at 2 GB and B past the
    co-residency bound are passed the small buffers of L2B32, which a refusal
    does not touch."""
    d = _inputs("L2B32")
    b = lr.Bufs(DEV, d)
    b.inp = {k: lr.flat(DEV, s.cols) for k, s in b.inp.items()}     # nothing put: sentinel everywhere
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    over_b = 32 * (ncu // 16) + 1
    fwd_bad = [(dict(x=None), "NULL"), (dict(act=None), "NULL"), (dict(cnt=None), "NULL"), (dict(err=None), "NULL"),
               (dict(D=79), "D 80 and H 256 only"), (dict(H=255), "D 80 and H 256 only"), (dict(L=0), "L < 1"),
               (dict(B=0), "not co-resident"), (dict(B=over_b), "not co-resident"),
               (dict(L=32768, B=32), "hout over 2 GB")]
    bwd_bad = [(dict(dh_out=None), "NULL"), (dict(dw_hh=None), "NULL"), (dict(part=None), "NULL"),
               (dict(err=None), "NULL"), (dict(H=255), "H 256 only"), (dict(L=0), "L < 1"),
               (dict(B=0), "not co-resident"), (dict(B=over_b), "not co-resident")]
    for layout in (0, 1, 2):
        with _layout(layout):
            for over, says in fwd_bad:
                assert _fwd(b, **over) == INVALID, over
                assert says in _last_error(), (over, _last_error())
            for over, says in bwd_bad:
                for with_dG in (True, False):
                    assert _bwd(b, with_dG, **over) == INVALID, over
                    assert says in _last_error(), (over, _last_error())
    torch.cuda.synchronize()
    for name, s in b.slabs("inp", "fwd", "bwd"):
        assert s.untouched(), f"{name} touched by a refused call"
    assert b.part.untouched() and b.cnt.intact()
    assert bool((lr.interior(b.cnt) == lr.CNT_FILL).all()), "counters zeroed by a refused call"
    assert int(_err().item()) == 0


def test_part_floats():
    lib = _lib()
    n = C.c_int64(-1)
    assert lib.vn_lstm_rows_part_floats(0, C.byref(n)) == INVALID and "bad argument" in _last_error()
    assert lib.vn_lstm_rows_part_floats(32, None) == INVALID and "bad argument" in _last_error()
    assert n.value == -1
    for B in (1, 32, 33, 97):
        nt = -(-B // 32)
        assert lib.vn_lstm_rows_part_floats(B, C.byref(n)) == 0
        assert n.value == 2 * 2 * nt * 16 * 32 * 256 + nt * 2 * 1024 * (256 + 80) + nt * 2 * 1024 == lr.part_floats(B)
