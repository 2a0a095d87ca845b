"""Every kernel variant behind the three learner products
(csrc/voxnav_gemm_f32.hip: vn_gemm_f32_linear / _dx / _tn) against float64
restatements (tests/gemm_helpers.py).

* Inputs on which f32 arithmetic is exact: the result must be bit-equal to the
  float64 reference cast to f32 (``torch.equal``), whatever the summation
  order, chunking, k-permutation or split count -- no tolerance.  Only the
  Tanh epilogue has one (the measured error of tanhf, gemm_helpers).
* Every case runs under the default options, ``gemm_dl = 0`` (the
  register-staged kernel only) and ``gemm_k32 = 1`` (32-deep direct-load
  chunks); the test ids name the kernel the defaults take (dl / staged), from
  a restatement of launch()'s eligibility rule.
* Outputs and workspaces live between guard bands of a sentinel pattern that
  must survive, as must the padding columns of an ``ldc > N`` output.
"""
import contextlib
import ctypes as C

import pytest
import torch

import gemm_helpers as gh

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SETTINGS = (("defaults", None), ("gemm_dl=0", ("gemm_dl", 0)), ("gemm_k32=1", ("gemm_k32", 1)))
INVALID = -1   # VN_ERR_INVALID


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@contextlib.contextmanager
def _setting(opt):
    from voxnav import _native
    if opt is None:
        assert _native.get_option("gemm_dl") == 1 and _native.get_option("gemm_k32") == 0
        yield
    else:
        with _native.option(*opt):
            yield


def _lib():
    from voxnav import _native
    return _native.load()


def _p(addr):
    return C.c_void_p(addr) if addr else None


def _gen(*seed):
    g = torch.Generator()
    g.manual_seed(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)) + 11)
    return g


def _expand(t, batch):
    return t if t.shape[0] == batch else t.expand(batch, *t.shape[1:])


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Case:
    """One product's inputs in guarded slabs; ``run()`` calls the entry point
    into fresh guarded outputs and returns them (CPU)."""
    slabs = ()

    def inputs_intact(self):
        return all(s.intact() for s in self.slabs)


class LinearCase(_Case):
    def __init__(self, gen, M, N, K, batch=1, epi=2, exact=True, lda=None, ldw=None, ldc=None, shift=0,
                 a_shared=False, w_shared=False, negative=False, odd_bias=False, density=1.0):
        self.M, self.N, self.K, self.batch, self.epi, self.ldc = M, N, K, batch, epi, ldc
        mk = gh.exact_ints if exact else gh.generic
        nA, nW = (1 if a_shared else batch), (1 if w_shared else batch)
        kw = dict(density=density) if exact else {}
        self.x, self.w = mk(gen, nA, M, K), mk(gen, nW, N, K, **kw)
        self.b = (gh.exact_bias if exact else gh.generic)(gen, nW, N) if epi else None
        lda, ldw = lda or K, ldw or K
        sgn = -1 if negative else 1
        self.A = gh.Slab(DEV, batch, M, K, ld=lda, stride=0 if a_shared else gh.round4(M * lda),
                         shift=shift).put(self.x)
        self.W = gh.Slab(DEV, batch, N, K, ld=ldw, stride=0 if w_shared else sgn * gh.round4(N * ldw),
                         shift=shift).put(self.w)
        self.B = None
        if epi:
            sb = 0 if w_shared else sgn * (gh.odd_stride(N) if odd_bias else gh.round4(N))
            self.B = gh.Slab(DEV, batch, 1, N, stride=sb).put(self.b)
        self.slabs = [s for s in (self.A, self.W, self.B) if s is not None]
        self.family = gh.kernel_family("linear", M, N, K, lda=lda, ldb=ldw, sa=self.A.stride, sb=self.W.stride,
                                       aligned=shift == 0)

    def ref(self):
        return gh.ref_linear(_expand(self.x, self.batch), _expand(self.w, self.batch),
                             None if self.b is None else _expand(self.b, self.batch), self.epi == 1)

    def bound(self):
        return gh.bound_linear(_expand(self.x, self.batch), _expand(self.w, self.batch),
                               None if self.b is None else _expand(self.b, self.batch), self.K)

    def call(self, c_ptr, ldc, sc, **over):
        a = dict(a=self.A.ptr, w=self.W.ptr, bias=self.B.ptr if self.B else 0, c=c_ptr, M=self.M, N=self.N, K=self.K,
                 batch=self.batch, act=1 if self.epi == 1 else 0)
        a.update(over)
        return _lib().vn_gemm_f32_linear(_p(a["a"]), self.A.ld, self.A.stride, _p(a["w"]), self.W.ld, self.W.stride,
                                         _p(a["bias"]), self.B.stride if self.B else 0, _p(a["c"]), ldc, sc, a["M"],
                                         a["N"], a["K"], a["batch"], a["act"], None)

    def out_slab(self):
        ldc = self.ldc or self.N
        return gh.Slab(DEV, self.batch, self.M, self.N, ld=ldc, stride=gh.round4(self.M * ldc))

    def run(self):
        Cs = self.out_slab()
        assert self.call(Cs.ptr, Cs.ld, Cs.stride) == 0
        torch.cuda.synchronize()
        assert Cs.intact(), "guard bands / padding of C overwritten"
        assert self.inputs_intact()
        return (Cs.get(),)


class DxCase(_Case):
    def __init__(self, gen, M, N, K, batch=1, with_y=True, exact=True, ldd=None, ldw=None, ldc=None, shift=0,
                 a_shared=False, w_shared=False, negative=False):
        self.M, self.N, self.K, self.batch, self.ldc = M, N, K, batch, ldc
        mk = gh.exact_ints if exact else gh.generic
        nA, nW = (1 if a_shared else batch), (1 if w_shared else batch)
        self.dy, self.w = mk(gen, nA, M, K), mk(gen, nW, K, N)
        self.y = (gh.exact_y if exact else gh.generic_y)(gen, nA, M, K) if with_y else None
        ldd, ldw = ldd or K, ldw or N
        sd = 0 if a_shared else gh.round4(M * ldd)
        self.D = gh.Slab(DEV, batch, M, K, ld=ldd, stride=sd, shift=shift).put(self.dy)
        self.Y = gh.Slab(DEV, batch, M, K, ld=ldd, stride=sd, shift=shift).put(self.y) if with_y else None
        self.W = gh.Slab(DEV, batch, K, N, ld=ldw, stride=0 if w_shared else (-1 if negative else 1) *
                         gh.round4(K * ldw), shift=shift).put(self.w)
        self.slabs = [s for s in (self.D, self.Y, self.W) if s is not None]
        self.family = gh.kernel_family("dx", M, N, K, lda=ldd, ldb=ldw, sa=sd, sb=self.W.stride, aligned=shift == 0)

    def _ops(self):
        return (_expand(self.dy, self.batch), None if self.y is None else _expand(self.y, self.batch),
                _expand(self.w, self.batch))

    def ref(self):
        return gh.ref_dx(*self._ops())

    def bound(self):
        return gh.bound_dx(*self._ops(), self.K)

    def call(self, c_ptr, ldc, sc, **over):
        a = dict(dy=self.D.ptr, w=self.W.ptr, c=c_ptr, M=self.M, N=self.N, K=self.K, batch=self.batch)
        a.update(over)
        return _lib().vn_gemm_f32_dx(_p(a["dy"]), _p(self.Y.ptr if self.Y else 0), self.D.ld, self.D.stride,
                                     _p(a["w"]), self.W.ld, self.W.stride, _p(a["c"]), ldc, sc, a["M"], a["N"],
                                     a["K"], a["batch"], None)

    out_slab = LinearCase.out_slab
    run = LinearCase.run


class TnCase(_Case):
    """C [M][N] = dZ^T X over K rows (+ column sums), `splits` as requested."""

    def __init__(self, gen, M, N, K, splits, batch=1, with_y=True, colsum=True, exact=True, ldd=None, ldb=None,
                 shift=0, a_shared=False, b_shared=False, negative=False, accumulate=False):
        self.M, self.N, self.K, self.batch, self.splits = M, N, K, batch, splits
        self.colsum, self.accumulate = colsum, accumulate
        mk = gh.exact_ints if exact else gh.generic
        nA, nB = (1 if a_shared else batch), (1 if b_shared else batch)
        self.dy, self.x = mk(gen, nA, K, M), mk(gen, nB, K, N)
        self.y = (gh.exact_y if exact else gh.generic_y)(gen, nA, K, M) if with_y else None
        self.c0 = gh.exact_ints(gen, batch, M, N) if accumulate else None
        self.s0 = gh.exact_ints(gen, batch, 1, M) if accumulate else None
        ldd, ldb = ldd or M, ldb or N
        sd = 0 if a_shared else gh.round4(K * ldd)
        self.D = gh.Slab(DEV, batch, K, M, ld=ldd, stride=sd, shift=shift).put(self.dy)
        self.Y = gh.Slab(DEV, batch, K, M, ld=ldd, stride=sd, shift=shift).put(self.y) if with_y else None
        self.X = gh.Slab(DEV, batch, K, N, ld=ldb, stride=0 if b_shared else (-1 if negative else 1) *
                         gh.round4(K * ldb), shift=shift).put(self.x)
        self.slabs = [s for s in (self.D, self.Y, self.X) if s is not None]
        self.kper, self.eff = gh.tn_plan(K, splits)
        self.family = gh.kernel_family("tn", M, N, K, kper=self.kper, lda=ldd, ldb=ldb, sa=sd, sb=self.X.stride,
                                       aligned=shift == 0)

    def _ops(self):
        return (_expand(self.dy, self.batch), None if self.y is None else _expand(self.y, self.batch),
                _expand(self.x, self.batch))

    def ref(self):
        c, s = gh.ref_tn(*self._ops())
        if self.accumulate:
            c, s = c + self.c0.double(), s + self.s0.double().squeeze(1)
        return c, s

    def bound(self):
        return gh.bound_tn(*self._ops(), self.K, self.eff)

    def out_slabs(self):
        M, N, bt = self.M, self.N, self.batch
        Cs = gh.Slab(DEV, bt, M, N, stride=M * N)
        S = gh.Slab(DEV, bt, 1, M, stride=M)
        if self.accumulate:
            Cs.put(self.c0)
            S.put(self.s0)
        return Cs, S, gh.Slab(DEV, 1, 1, self.splits * bt * M * N), gh.Slab(DEV, 1, 1, self.splits * bt * M)

    def call(self, Cs, S, work, work2, **over):
        a = dict(dy=self.D.ptr, b=self.X.ptr, c=Cs.ptr, sc=self.M * self.N, colsum=S.ptr if self.colsum else 0,
                 M=self.M, N=self.N, K=self.K, batch=self.batch, splits=self.splits, ws=work.ptr,
                 ws2=work2.ptr if self.colsum else 0)
        a.update(over)
        return _lib().vn_gemm_f32_tn(_p(a["dy"]), _p(self.Y.ptr if self.Y else 0), self.D.ld, self.D.stride,
                                     _p(a["b"]), self.X.ld, self.X.stride, _p(a["c"]), a["sc"], _p(a["colsum"]),
                                     a["M"], a["N"], a["K"], a["batch"], a["splits"], _p(a["ws"]), _p(a["ws2"]),
                                     1 if self.accumulate else 0, None)

    def run(self):
        Cs, S, ws, ws2 = self.out_slabs()
        assert self.call(Cs, S, ws, ws2) == 0
        torch.cuda.synchronize()
        for name, s in (("C", Cs), ("colsum", S), ("workspace", ws), ("workspace2", ws2)):
            assert s.intact(), f"guard bands of {name} overwritten"
        assert self.inputs_intact()
        # the entry point lowers the split count: only `eff` partials are written
        used = self.eff * self.batch * self.M
        assert bool((ws.mat(0).view(torch.int32)[0, used * self.N:] == gh.SENTINEL).all())
        if self.colsum:
            assert bool((ws2.mat(0).view(torch.int32)[0, used:] == gh.SENTINEL).all())
            return Cs.get(), S.get().squeeze(1)
        assert S.untouched() and ws2.untouched()
        return (Cs.get(),)


def _check_exact(case, what):
    """Under every option setting: bit-equal to float64 (tanh: within its
    tolerance), and the defaults and gemm_dl = 0 bit-equal to each other."""
    ref = case.ref()
    ref = ref if isinstance(ref, tuple) else (ref,)
    tanh = getattr(case, "epi", 0) == 1
    outs = {}
    for name, opt in SETTINGS:
        with _setting(opt):
            outs[name] = got = case.run()
        for g, r in zip(got, ref):
            if tanh:
                gh.assert_tanh_close(g, r, f"{what} [{name}]")
            else:
                assert torch.equal(g, r.float()), f"{what} [{name}]: not bit-equal to the float64 reference"
    if not tanh:
        for g, h in zip(outs["defaults"], outs["gemm_dl=0"]):
            assert torch.equal(_bits(g), _bits(h)), f"{what}: defaults and gemm_dl=0 differ in bits"


def _grid(ks):
    return [(M, N, ks[(i + 2 * j) % len(ks)]) for i, M in enumerate(gh.TILE_EDGES) for j, N in
            enumerate(gh.TILE_EDGES)]


def _lin_id(p):
    M, N, K = p
    return f"{M}x{N}x{K}-{gh.kernel_family('linear', M, N, K)}"


def _dx_id(p):
    M, N, K = p
    return f"{M}x{N}x{K}-{gh.kernel_family('dx', M, N, K)}"


def _tn_id(p):
    M, N, (K, sp) = p
    return f"{M}x{N}-K{K}s{sp}-{gh.kernel_family('tn', M, N, K, kper=gh.tn_plan(K, sp)[0])}"


def test_grids_cover_every_listed_value_in_both_families():
    """The shape lists of this file: every tile edge as M and as N, crossed;
    every K (and (K, splits)); both kernel families for each product."""
    for grid, kid, ks in ((_grid(gh.K_LINEAR), _lin_id, gh.K_LINEAR), (_grid(gh.K_LINEAR), _dx_id, gh.K_LINEAR),
                          (_grid(gh.TN_K_SPLITS), _tn_id, gh.TN_K_SPLITS)):
        assert {(M, N) for M, N, _ in grid} == {(M, N) for M in gh.TILE_EDGES for N in gh.TILE_EDGES}
        assert {k for _, _, k in grid} == set(ks)
        fams = {kid(p).rsplit("-", 1)[1] for p in grid}
        assert fams == {"dl", "staged"}
    assert gh.tn_plan(100, 7) == (32, 4) and 100 - 3 * 32 == 4
    assert gh.tn_plan(1056, 8) == (160, 7) and 1056 - 6 * 160 == 96
    assert gh.tn_plan(300, 300) == (32, 10) and gh.tn_plan(17, 5) == (32, 1)
    assert gh.kernel_family("linear", 8, 8, 96, gemm_k32=1) == "dl32"
    assert gh.kernel_family("linear", 8, 8, 48, gemm_k32=1) == "dl"     # K % 32 != 0: 16-deep chunks
    assert gh.kernel_family("linear", 8, 8, 96, gemm_dl=0) == "staged"


# ------------------------------------------------------------------ the grids
@pytest.mark.parametrize("shape", _grid(gh.K_LINEAR), ids=_lin_id)
def test_linear_exact(shape):
    M, N, K = shape
    for epi in (0, 2, 1):   # store, + bias, tanh(+ bias)
        # tanh: sparse weights keep the exact pre-activations where tanh is not saturated
        case = LinearCase(_gen(M, N, K, epi), M, N, K, epi=epi, density=min(1.0, 2.0 / K) if epi == 1 else 1.0)
        assert case.family == _lin_id(shape).rsplit("-", 1)[1]
        _check_exact(case, f"linear {shape} epi {epi}")


@pytest.mark.parametrize("shape", _grid(gh.K_LINEAR), ids=_dx_id)
def test_dx_exact(shape):
    M, N, K = shape
    for with_y in (False, True):
        case = DxCase(_gen(M, N, K, with_y), M, N, K, with_y=with_y)
        assert case.family == _dx_id(shape).rsplit("-", 1)[1]
        _check_exact(case, f"dx {shape} y={with_y}")


@pytest.mark.parametrize("shape", _grid(gh.TN_K_SPLITS), ids=_tn_id)
def test_tn_exact(shape):
    M, N, (K, sp) = shape
    for with_y in (False, True):
        for colsum in (False, True):
            case = TnCase(_gen(M, N, K, sp, with_y, colsum), M, N, K, sp, with_y=with_y, colsum=colsum)
            assert case.family == _tn_id(shape).rsplit("-", 1)[1]
            _check_exact(case, f"tn {shape} y={with_y} colsum={colsum}")


# ------------------------------------------- block counts (the XCD re-deal), batch
# (kind, M, N, K, batch, splits) -> nblk: 8 and 24 re-dealt, 6 and 9 not
BLOCKS = [("linear", 200, 200, 48, 2, 1, 8), ("linear", 260, 200, 17, 4, 1, 24), ("linear", 260, 200, 48, 1, 1, 6),
          ("linear", 260, 260, 17, 1, 1, 9),
          ("dx", 200, 200, 48, 2, 1, 8), ("dx", 260, 200, 17, 4, 1, 24), ("dx", 260, 200, 48, 1, 1, 6),
          ("dx", 260, 260, 17, 1, 1, 9),
          ("tn", 200, 200, 48, 2, 1, 8), ("tn", 200, 200, 96, 2, 3, 24), ("tn", 129, 64, 100, 1, 7, 8),
          ("tn", 128, 68, 96, 2, 3, 6), ("tn", 260, 31, 96, 1, 3, 9)]


@pytest.mark.parametrize("kind,M,N,K,batch,splits,blocks", BLOCKS,
                         ids=[f"{b[0]}-{b[1]}x{b[2]}x{b[3]}-b{b[4]}s{b[5]}-nblk{b[6]}" for b in BLOCKS])
def test_block_counts_exact(kind, M, N, K, batch, splits, blocks):
    g = _gen(M, N, K, batch, splits)
    if kind == "tn":
        case = TnCase(g, M, N, K, splits, batch=batch)
        assert gh.nblk(M, N, batch, case.eff) == blocks
    else:
        case = (LinearCase if kind == "linear" else DxCase)(g, M, N, K, batch=batch)
        assert gh.nblk(M, N, batch) == blocks
    _check_exact(case, f"{kind} nblk {blocks}")


LAYOUTS = ["a_shared", "b_shared", "negative", "odd_bias"]     # odd_bias: only the Linear forward takes a bias
STRIDES = [(kind, M, N, K, layout)
           for kind, M, N, K in [("linear", 132, 68, 48), ("linear", 31, 6, 17), ("dx", 132, 68, 48),
                                 ("dx", 31, 6, 17), ("tn", 132, 68, 96), ("tn", 31, 6, 100)]
           for layout in LAYOUTS if kind == "linear" or layout != "odd_bias"]


@pytest.mark.parametrize("kind,M,N,K,layout", STRIDES)
def test_batch_strides_exact(kind, M, N, K, layout):
    """Batch 2 with a stride-0 A, a stride-0 B, the second branch's weights
    (and bias) below the first's (negative strides, as _pair_stride gives for
    separately allocated parameters), a bias stride that is no multiple of 4."""
    g = _gen(M, N, K, LAYOUTS.index(layout))
    if kind == "linear":
        case = LinearCase(g, M, N, K, batch=2, a_shared=layout == "a_shared", w_shared=layout == "b_shared",
                          negative=layout == "negative", odd_bias=layout == "odd_bias")
        if layout == "negative":
            assert case.W.stride < 0 and case.B.stride < 0
        if layout == "odd_bias":
            assert case.B.stride % 4 != 0
    elif kind == "dx":
        case = DxCase(g, M, N, K, batch=2, a_shared=layout == "a_shared", w_shared=layout == "b_shared",
                      negative=layout == "negative")
    else:
        case = TnCase(g, M, N, K, 3, batch=2, a_shared=layout == "a_shared", b_shared=layout == "b_shared",
                      negative=layout == "negative")
    _check_exact(case, f"{kind} {layout}")


# ------------------------------------------------------------- raw-ABI layouts
# (vn_gemm_f32_tn writes a contiguous C: no ldc)
LAYOUT_VARIANTS = [(kind, variant, M, N, K) for M, N, K in [(132, 68, 48), (129, 31, 40)]
                   for variant in ["lda+4", "lda+1", "ldb_padded", "ldc+3", "shifted", "all"]
                   for kind in ["linear", "dx", "tn"] if not (kind == "tn" and variant == "ldc+3")]


@pytest.mark.parametrize("kind,variant,M,N,K", LAYOUT_VARIANTS)
def test_leading_dimensions_and_alignment_exact(kind, variant, M, N, K):
    """Leading dimensions larger than the row (lda = K + 4 keeps the
    direct-load kernel, K + 1 defeats it), a padded weight row, ldc = N + 3
    with guarded padding columns, and every operand pointer advanced by one
    float (the misaligned fallback): the same bits as the float64 reference."""
    g = _gen(M, N, K, len(variant))
    pad_a = {"lda+4": 4, "lda+1": 1, "all": 4}.get(variant, 0)
    pad_b = {"ldb_padded": 8, "all": 4}.get(variant, 0)
    pad_c = 3 if variant in ("ldc+3", "all") else 0
    shift = 1 if variant in ("shifted", "all") else 0
    if kind == "linear":
        case = LinearCase(g, M, N, K, batch=2, lda=K + pad_a, ldw=K + pad_b, ldc=N + pad_c, shift=shift)
        dense = gh.kernel_family("linear", M, N, K)
    elif kind == "dx":
        case = DxCase(g, M, N, K, batch=2, ldd=K + pad_a, ldw=N + pad_b, ldc=N + pad_c, shift=shift)
        dense = gh.kernel_family("dx", M, N, K)
    else:
        case = TnCase(g, M, N, K, 2, batch=2, ldd=M + pad_a, ldb=N + pad_b, shift=shift)
        dense = gh.kernel_family("tn", M, N, K, kper=case.kper)
    if variant in ("lda+1", "shifted", "all"):
        assert case.family == "staged"
    else:
        assert case.family == dense
    _check_exact(case, f"{kind} {variant}")


@pytest.mark.parametrize("M,N,K,sp", [(132, 68, 96, 3), (129, 31, 100, 7), (64, 64, 1056, 8)])
def test_tn_accumulate_exact(M, N, K, sp):
    """accumulate = 1: C and colsum pre-filled with exact values, result =
    old + product."""
    for with_y in (False, True):
        _check_exact(TnCase(_gen(M, N, K, with_y), M, N, K, sp, batch=2, with_y=with_y, accumulate=True),
                     f"tn accumulate y={with_y}")


# ------------------------------------------------ generic inputs, determinism
GENERIC = [("linear", 132, 68, 96), ("linear", 129, 31, 100), ("dx", 132, 68, 96), ("dx", 129, 31, 100),
           ("tn", 132, 68, 1056), ("tn", 129, 31, 300)]


@pytest.mark.parametrize("setting", SETTINGS, ids=[s[0] for s in SETTINGS])
@pytest.mark.parametrize("kind,M,N,K", GENERIC)
def test_generic_inputs_within_derived_bound_and_deterministic(kind, M, N, K, setting):
    """randn operands: every entry within (K + splits + 8) 2^-24 (|A| |B|)_ij of
    float64 (gemm_helpers: derived, not measured), and a second call on the
    same inputs gives the same bits."""
    g = _gen(M, N, K, 5)
    if kind == "linear":
        cases = [LinearCase(g, M, N, K, batch=2, epi=2, exact=False)]
    elif kind == "dx":
        cases = [DxCase(g, M, N, K, batch=2, with_y=wy, exact=False) for wy in (False, True)]
    else:
        cases = [TnCase(g, M, N, K, 8, batch=2, with_y=wy, exact=False) for wy in (False, True)]
    for case in cases:
        ref, bound = case.ref(), case.bound()
        ref, bound = (ref, bound) if isinstance(ref, tuple) else ((ref,), (bound,))
        with _setting(setting[1]):
            got, again = case.run(), case.run()
        for a, b, r, bd in zip(got, again, ref, bound):
            assert torch.equal(_bits(a), _bits(b)), "two calls on the same inputs differ"
            gh.assert_within(a, r, bd, f"{kind} {setting[0]}")


def test_generic_bound_has_teeth():
    """The derived bound separates a correct f32 sum from one with a dropped
    term (CPU arithmetic only): a chunked f32 sum stays inside it, the same
    sum without one k-term leaves it in most entries."""
    g = _gen(99)
    M, N, K = 64, 48, 1056
    x, w = gh.generic(g, 1, M, K), gh.generic(g, 1, N, K)
    ref, bound = gh.ref_linear(x, w, None, False), gh.bound_linear(x, w, None, K, splits=8)
    acc = torch.zeros((1, M, N))
    for k0 in range(0, K, 37):
        acc = acc + x[:, :, k0:k0 + 37] @ w[:, :, k0:k0 + 37].transpose(1, 2)
    gh.assert_within(acc, ref, bound, "chunked f32 sum")
    dropped = acc - x[:, :, 5:6] @ w[:, :, 5:6].transpose(1, 2)
    assert float(((dropped.double() - ref).abs() > bound).double().mean()) > 0.5


# -------------------------------------------------------------------- refusals
def test_refusals_leave_outputs_untouched():
    """VN_ERR_INVALID, nothing launched: NULL operands, a size below 1, the
    Tanh epilogue without a bias, colsum without workspace2, sc != M N."""
    g = _gen(1)
    M, N, K = 33, 20, 24
    lin, dx, tn = LinearCase(g, M, N, K, epi=1), DxCase(g, M, N, K), TnCase(g, M, N, K, 2)
    lib = _lib()
    outs = []
    for case in (lin, dx):
        Cs = case.out_slab()
        outs.append(Cs)
        names = ("a", "w", "c") if case is lin else ("dy", "w", "c")
        for name in names:
            assert case.call(Cs.ptr, Cs.ld, Cs.stride, **{name: 0}) == INVALID, name
            assert b"NULL" in lib.vn_last_error()
        for dim in ("M", "N", "K", "batch"):
            for bad in (0, -2):
                assert case.call(Cs.ptr, Cs.ld, Cs.stride, **{dim: bad}) == INVALID, (dim, bad)
    assert lin.call(outs[0].ptr, N, M * N, bias=0) == INVALID    # act = 1 without bias
    assert b"bias" in lib.vn_last_error()
    Cs, S, ws, ws2 = tn.out_slabs()
    outs += [Cs, S, ws, ws2]
    for name in ("dy", "b", "c", "ws"):
        assert tn.call(Cs, S, ws, ws2, **{name: 0}) == INVALID, name
        assert b"NULL" in lib.vn_last_error()
    for dim in ("M", "N", "K", "batch", "splits"):
        for bad in (0, -2):
            assert tn.call(Cs, S, ws, ws2, **{dim: bad}) == INVALID, (dim, bad)
    assert tn.call(Cs, S, ws, ws2, ws2=0) == INVALID
    assert b"workspace2" in lib.vn_last_error()
    for bad in (M * N - 1, M * N + 4, 0):
        assert tn.call(Cs, S, ws, ws2, sc=bad) == INVALID
    torch.cuda.synchronize()
    for s in outs:
        assert s.untouched()
    # and the same calls, valid, go through
    assert lin.call(outs[0].ptr, N, M * N) == 0 and dx.call(outs[1].ptr, N, M * N) == 0
    assert tn.call(Cs, S, ws, ws2) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------ autograd wrappers
def _params(shapes, order):
    """Separately allocated f32 tensors, one per branch and shape; `order`
    +1: the pi branch's tensors lie below the vf branch's, -1: above."""
    out = []
    for s in shapes:
        pair = sorted((torch.empty(s, device=DEV), torch.empty(s, device=DEV)), key=lambda t: t.data_ptr())
        out.append(pair if order > 0 else pair[::-1])
    return out


def _leaf(t):
    return t.to(DEV).requires_grad_(True)


@pytest.mark.parametrize("M,K,N", [(132, 48, 132), (5, 17, 3)])
def test_linear_wrapper_gradients_exact(M, K, N):
    """``linear`` (the heads) on exact inputs: the output and every gradient
    bit-equal to float64 autograd."""
    from voxnav.learn_ops import linear
    g = _gen(M, K, N)
    lin = torch.nn.Linear(K, N).to(DEV)
    with torch.no_grad():
        lin.weight.copy_(gh.exact_ints(g, N, K))
        lin.bias.copy_(gh.exact_bias(g, N))
    x, dy = _leaf(gh.exact_ints(g, M, K)), gh.exact_ints(g, M, N)
    for name, opt in SETTINGS:
        x.grad = lin.weight.grad = lin.bias.grad = None
        with _setting(opt):
            y = linear(x, lin)
            (y * dy.to(DEV)).sum().backward()
        x64, w64, b64 = (t.detach().cpu().double().requires_grad_(True) for t in (x, lin.weight, lin.bias))
        y64 = x64 @ w64.T + b64
        (y64 * dy.double()).sum().backward()
        for got, ref in ((y, y64), (x.grad, x64.grad), (lin.weight.grad, w64.grad), (lin.bias.grad, b64.grad)):
            assert torch.equal(got.detach().cpu(), ref.detach().float()), name


def _pair_reference(x, ws, bs, dy, tanh):
    """float64 autograd of one paired layer; x [2, M, K] leaves per branch."""
    x64 = x.detach().cpu().double().requires_grad_(True)
    w64 = [w.detach().cpu().double().requires_grad_(True) for w in ws]
    b64 = [b.detach().cpu().double().requires_grad_(True) for b in bs]
    z = torch.stack([x64[i] @ w64[i].T + b64[i] for i in range(2)])
    y = torch.tanh(z) if tanh else z
    (y * dy.double()).sum().backward()
    return y.detach(), x64.grad, [w.grad for w in w64], [b.grad for b in b64]


@pytest.mark.parametrize("order", [1, -1], ids=["pi_below_vf", "pi_above_vf"])
@pytest.mark.parametrize("M,K,N", [(132, 48, 132), (5, 17, 3)])
def test_linear_pair_wrapper_gradients_exact(M, K, N, order):
    """``linear_tanh_pair(tanh=False)`` with the two branches' parameters
    allocated separately, in both address orders (a negative batch stride in
    one of them): output and gradients bit-equal to float64 autograd."""
    from voxnav.learn_ops import linear_tanh_pair
    g = _gen(M, K, N, order + 1)
    (wa, wb), (ba, bb) = _params([(N, K), (N,)], order)
    assert (wb.data_ptr() - wa.data_ptr()) * order > 0 and (bb.data_ptr() - ba.data_ptr()) * order > 0
    for w in (wa, wb):
        w.copy_(gh.exact_ints(g, N, K))
        w.requires_grad_(True)
    for b in (ba, bb):
        b.copy_(gh.exact_bias(g, N))
        b.requires_grad_(True)
    x, dy = _leaf(gh.exact_ints(g, 2, M, K)), gh.exact_ints(g, 2, M, N)
    for name, opt in SETTINGS:
        for t in (x, wa, wb, ba, bb):
            t.grad = None
        with _setting(opt):
            y = linear_tanh_pair(x, (wa, wb), (ba, bb), tanh=False)
            (y * dy.to(DEV)).sum().backward()
        y64, dx64, dw64, db64 = _pair_reference(x, (wa, wb), (ba, bb), dy, False)
        for got, ref in ((y, y64), (x.grad, dx64), (wa.grad, dw64[0]), (wb.grad, dw64[1]), (ba.grad, db64[0]),
                         (bb.grad, db64[1])):
            assert torch.equal(got.detach().cpu(), ref.float()), name


def _mlp_with_bounds(x, e_x, layers, dy):
    """float64 forward / backward of a Tanh MLP branch with first-order error
    bounds of the f32 kernels (gemm_helpers.ErrProp); layers: [(W, b)] f32
    CPU.  Returns (h, e_h), dx with bound, [(dW, e), (db, e)] per layer."""
    P = gh.ErrProp
    acts = [(x.double(), e_x)]
    for w, b in layers:
        acts.append(P.tanh(*P.linear(*acts[-1], w, b)))
    d, e_d = dy.double(), torch.zeros_like(dy, dtype=torch.float64)
    grads = [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        (h_in, e_in), (h_out, e_out) = acts[l], acts[l + 1]
        dz, e_dz, a_dz = P.agrad(d, e_d, h_out, e_out)
        grads[l] = P.tn(dz, e_dz, a_dz, h_in, e_in)
        d, e_d = P.dx(dz, e_dz, a_dz, layers[l][0])
    return acts[-1], (d, e_d), grads


@pytest.mark.parametrize("order", [1, -1], ids=["pi_below_vf", "pi_above_vf"])
@pytest.mark.parametrize("M,K,N", [(132, 48, 132), (5, 17, 3)])
def test_tanh_pair_and_mlp_pair_gradients_against_float64(M, K, N, order):
    """``linear_tanh_pair`` (one Tanh layer) and ``mlp_pair`` (two layers,
    K -> N -> N) on generic inputs against float64 autograd's values: every
    output and gradient entry within the first-order propagated bound
    (gemm_helpers.ErrProp: the summation bound of each product plus the
    tanh tolerance, carried through the layers).  mlp_pair must also give the
    bits of its layers called one by one."""
    from voxnav.learn_ops import linear_tanh_pair, mlp_pair
    g = _gen(M, K, N, order + 7)
    shapes = [(N, K), (N,), (N, N), (N,)]
    prm = _params(shapes, order)
    nets = []
    for br in range(2):
        net = torch.nn.Sequential(torch.nn.Linear(K, N), torch.nn.Tanh(), torch.nn.Linear(N, N), torch.nn.Tanh())
        for mod, (wi, bi) in ((net[0], (0, 1)), (net[2], (2, 3))):
            prm[wi][br].copy_(torch.randn(shapes[wi], generator=g) / shapes[wi][1] ** 0.5)
            prm[bi][br].copy_(0.1 * torch.randn(shapes[bi], generator=g))
            mod.weight = torch.nn.Parameter(prm[wi][br])
            mod.bias = torch.nn.Parameter(prm[bi][br])
            assert mod.weight.data_ptr() == prm[wi][br].data_ptr()
        nets.append(net)
    pi, vf = nets
    x = _leaf(gh.generic(g, 2, M, K))
    dy = gh.generic(g, 2, M, N)
    params = [p for net in nets for p in net.parameters()]

    def clear():
        for t in [x] + params:
            t.grad = None

    for name, opt in SETTINGS:
        with _setting(opt):
            # one layer
            clear()
            y1 = linear_tanh_pair(x, (pi[0].weight, vf[0].weight), (pi[0].bias, vf[0].bias))
            (y1 * dy.to(DEV)).sum().backward()
            one = [y1.detach().cpu(), x.grad.cpu()] + [[n[0].weight.grad.cpu(), n[0].bias.grad.cpu()] for n in nets]
            # two layers, by mlp_pair and layer by layer
            clear()
            h = mlp_pair(pi, vf, None, x_pair=x, stacked=True)
            (h * dy.to(DEV)).sum().backward()
            two = [h.detach().cpu(), x.grad.cpu()] + [[p.grad.cpu() for p in n.parameters()] for n in nets]
            clear()
            h2 = linear_tanh_pair(linear_tanh_pair(x, (pi[0].weight, vf[0].weight), (pi[0].bias, vf[0].bias)),
                                  (pi[2].weight, vf[2].weight), (pi[2].bias, vf[2].bias))
            (h2 * dy.to(DEV)).sum().backward()
            chain = [h2.detach().cpu(), x.grad.cpu()] + [[p.grad.cpu() for p in n.parameters()] for n in nets]
        assert torch.equal(_bits(two[0]), _bits(chain[0])) and torch.equal(_bits(two[1]), _bits(chain[1]))
        for br in range(2):
            for a, b in zip(two[2 + br], chain[2 + br]):
                assert torch.equal(_bits(a), _bits(b))
        for br in range(2):
            net = nets[br]
            lay = [(net[0].weight.detach().cpu(), net[0].bias.detach().cpu()),
                   (net[2].weight.detach().cpu(), net[2].bias.detach().cpu())]
            xb, zero = x.detach().cpu()[br], torch.zeros((M, K), dtype=torch.float64)
            for depth, got in ((1, one), (2, two)):
                (hh, e_h), (dx, e_dx), grads = _mlp_with_bounds(xb, zero, lay[:depth], dy[br])
                what = f"{name} branch {br} depth {depth}"
                gh.assert_within(got[0][br], hh, e_h, what + " output")
                gh.assert_within(got[1][br], dx, e_dx, what + " dx")
                flat = got[2 + br]
                for l in range(depth):
                    (dw, e_dw), (db, e_db) = grads[l]
                    gh.assert_within(flat[2 * l], dw, e_dw, what + f" dW{l}")
                    gh.assert_within(flat[2 * l + 1], db, e_db, what + f" db{l}")


def test_mlp_pair_shared_input_matches_stacked():
    """``mlp_pair(pi, vf, x)`` (both branches read x, expanded with batch
    stride 0; expand's backward sums the branches' dX) against the stacked
    call on exact inputs: outputs bit-equal, dX the exact sum."""
    from voxnav.learn_ops import linear_tanh_pair
    g = _gen(21)
    M, K, N = 132, 48, 132
    w, b = gh.exact_ints(g, 2, N, K).to(DEV), gh.exact_bias(g, 2, N).to(DEV)
    x, dy = _leaf(gh.exact_ints(g, M, K)), gh.exact_ints(g, 2, M, N)
    y = linear_tanh_pair(x, w, b, tanh=False)
    (y * dy.to(DEV)).sum().backward()
    x64 = x.detach().cpu().double().requires_grad_(True)
    y64 = torch.stack([x64 @ w[i].cpu().double().T + b[i].cpu().double() for i in range(2)])
    (y64 * dy.double()).sum().backward()
    assert torch.equal(y.detach().cpu(), y64.detach().float())
    assert torch.equal(x.grad.cpu(), x64.grad.float())


@pytest.mark.parametrize("K,M,N,bt", [(1056, 132, 68, 2), (100, 31, 6, 1)])
def test_mm_tn_out_and_y_validation(K, M, N, bt):
    """``mm_tn(out=...)`` writes the given tensor (guarded) and returns it;
    a ``y`` whose shape or strides differ from ``a``'s is refused before
    anything is launched."""
    from voxnav.learn_ops import mm_tn
    g = _gen(K, M, N)
    a, b, y = gh.exact_ints(g, bt, K, M), gh.exact_ints(g, bt, K, N), gh.exact_y(g, bt, K, M)
    c64, s64 = gh.ref_tn(a, y, b)
    slab = gh.Slab(DEV, bt, M, N, stride=M * N)
    out = slab.f[slab.off0:slab.off0 + bt * M * N].view(bt, M, N)
    ad, bd, yd = a.to(DEV), b.to(DEV), y.to(DEV)
    for name, opt in SETTINGS:
        with _setting(opt):
            got, cs = mm_tn(ad, bd, y=yd, colsum=True, out=out)
        assert got is out
        assert torch.equal(out.cpu(), c64.float()) and torch.equal(cs.cpu(), s64.float()), name
        assert slab.intact()
    before = _bits(out).clone()
    wide = torch.zeros((bt, K, M + 4), device=DEV)[:, :, :M]
    bad = [yd[:, :K - 1], yd.transpose(1, 2).contiguous().transpose(1, 2), wide, yd[0]]
    if bt > 1:
        bad.append(yd[:1].expand(bt, K, M))
    for yy in bad:
        with pytest.raises(ValueError):
            mm_tn(ad, bd, y=yy, colsum=True, out=out)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), before)
