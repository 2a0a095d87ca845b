"""Shared pieces of the learner-GEMM tests (tests/test_gemm_variants_gpu.py):
float64 restatements of the three products of csrc/voxnav_gemm_f32.hip,
inputs on which f32 arithmetic is exact, the derived error bound for generic
inputs, the tanh tolerance, a restatement of launch()'s kernel choice, and a
guard-band allocator.  Importing this module needs no GPU.

The products (f32 operands, restated on CPU float64 tensors):
  linear  C = act(X W^T + b)      X [M][K], W [N][K], b [N]
  dx      C = dZ W                dZ [M][K], W [K][N]
  tn      C = dZ^T X, s = colsum  dZ [K][M], X [K][N], s [M] = sum_k dZ[k][m]
  with dZ = dy (1 - y^2) when y is given, else dy.

Exact inputs.  Operands are integers in [-4, 4], biases multiples of 1/16 in
[-1, 1], y a multiple of 1/4 in [-0.75, 0.75].  Then 1 - y^2 is a multiple of
1/16 in [7/16, 1], dZ a multiple of 1/16 of magnitude <= 4, every product a
multiple of 1/16 of magnitude <= 16, and every partial sum of up to K = 4096
products has magnitude <= 2^16: at most 2^20 units of 2^-4, below 2^24.  Every
intermediate of any summation order is therefore an exact f32 number, and a
correct kernel returns the float64 result cast to f32, bit for bit.

Generic inputs.  For an f32 dot product of K terms summed in any order, plus
`splits` partials added in order, plus the operand formation of AGRAD
(y y, 1 - y y, dy (1 - y y): three roundings, whose absolute error is at most
3 u |dy| (1 + y^2)) and the bias add, the standard bound is
  |err_ij| <= (K + splits + 8) u (|A| |B|)_ij,   u = 2^-24,
with |A| = |dy| (1 + y^2) under AGRAD (gamma_n <= n u (1 + small); the + 8
absorbs the operand roundings, the bias add and the second-order terms).

tanh.  The ROCm installation documents no ulp bound for tanhf, so it was
measured once, on its own: torch.tanh of the 2^25 + 1 f32
values -8 + i 2^-21 (i = 0 .. 2^25) on an MI355X (torch 2.10.0+rocm7.0, HIP
7.0.51831) against float64 tanh of the same values, the error in ulps of the
float64 result's f32 binade: maximum 1.3630 ulp (at x = -0.63531876).  The
tolerance of the Tanh epilogue on exact pre-activations is twice that,
TANH_TOL_ULP = 2.726 ulp.  (It was not derived from the GEMM's own output.)
"""
from __future__ import annotations

import math
from typing import Optional

import torch

U = 2.0 ** -24
TANH_MEASURED_ULP = 1.3630047049373388
TANH_TOL_ULP = max(1.0, 2.0 * TANH_MEASURED_ULP)

SENTINEL = 0x7FA5A5A5          # a NaN bit pattern no kernel here produces
BAND = 256                     # guard floats on each side (keeps the payload 16-B aligned)

TILE_EDGES = (1, 4, 6, 31, 64, 127, 128, 129, 132, 260)
K_LINEAR = (1, 3, 17, 40, 100, 16, 32, 48, 96)
TN_K_SPLITS = ((16, 1), (96, 3), (100, 7), (1056, 8), (2048, 8), (17, 5), (300, 300))
GT, GK_TN, GKD = 128, 32, 16


# ----------------------------------------------------------------- references
def dz64(dy: torch.Tensor, y: Optional[torch.Tensor]) -> torch.Tensor:
    d = dy.double()
    return d * (1.0 - y.double() ** 2) if y is not None else d


def ref_linear(x, w, b, act: bool):
    """x [bt, M, K], w [bt, N, K], b [bt, N] or None -> [bt, M, N] float64."""
    z = x.double() @ w.double().transpose(-1, -2)
    if b is not None:
        z = z + b.double().unsqueeze(-2)
    return torch.tanh(z) if act else z


def ref_dx(dy, y, w):
    """dy, y [bt, M, K], w [bt, K, N] -> [bt, M, N] float64."""
    return dz64(dy, y) @ w.double()


def ref_tn(dy, y, x):
    """dy, y [bt, K, M], x [bt, K, N] -> ([bt, M, N], [bt, M]) float64."""
    z = dz64(dy, y)
    return z.transpose(-1, -2) @ x.double(), z.sum(-2)


def abs_dz(dy, y):
    a = dy.double().abs()
    return a * (1.0 + y.double() ** 2) if y is not None else a


def bound_linear(x, w, b, K, splits=1):
    m = x.double().abs() @ w.double().abs().transpose(-1, -2)
    if b is not None:
        m = m + b.double().abs().unsqueeze(-2)
    return (K + splits + 8) * U * m


def bound_dx(dy, y, w, K, splits=1):
    return (K + splits + 8) * U * (abs_dz(dy, y) @ w.double().abs())


def bound_tn(dy, y, x, K, splits):
    a = abs_dz(dy, y)
    f = (K + splits + 8) * U
    return f * (a.transpose(-1, -2) @ x.double().abs()), f * a.sum(-2)


def ulp32(ref64: torch.Tensor) -> torch.Tensor:
    """The f32 unit in the last place at each float64 value."""
    e = torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 23)


def assert_tanh_close(got: torch.Tensor, ref64: torch.Tensor, what=""):
    err = ((got.double() - ref64).abs() / ulp32(ref64)).max().item()
    assert err <= TANH_TOL_ULP, f"{what}: tanh epilogue off by {err:.3f} ulp (tolerance {TANH_TOL_ULP:.3f})"


def assert_within(got: torch.Tensor, ref64: torch.Tensor, bound: torch.Tensor, what=""):
    err = (got.double() - ref64).abs()
    bad = err > bound
    assert not bool(bad.any()), (f"{what}: {int(bad.sum())} of {bad.numel()} entries beyond the derived bound, worst "
                                 f"ratio {float((err / bound.clamp_min(1e-300)).max()):.3g}")


# --------------------------------------------------------------------- inputs
def exact_ints(gen: torch.Generator, *shape, density: float = 1.0) -> torch.Tensor:
    t = torch.randint(-4, 5, shape, generator=gen).float()
    if density < 1.0:
        t = t * (torch.rand(shape, generator=gen) < density).float()
    return t


def exact_bias(gen, *shape):
    return torch.randint(-16, 17, shape, generator=gen).float() / 16.0


def exact_y(gen, *shape):
    return torch.randint(-3, 4, shape, generator=gen).float() / 4.0


def generic(gen, *shape):
    return torch.randn(shape, generator=gen)


def generic_y(gen, *shape):
    return 0.95 * torch.tanh(torch.randn(shape, generator=gen))


# ---------------------------------------------------- launch()'s kernel choice
def tn_plan(K: int, splits: int):
    """(K per split, split count) as vn_gemm_f32_tn lowers a requested count."""
    kper = -(-K // splits)
    kper = -(-kper // GK_TN) * GK_TN
    return kper, -(-K // kper)


def kernel_family(kind: str, M: int, N: int, K: int, kper: Optional[int] = None, lda: Optional[int] = None,
                  ldb: Optional[int] = None, sa: int = 0, sb: int = 0, aligned: bool = True, gemm_dl: int = 1,
                  gemm_k32: int = 0) -> str:
    """Which kernel launch() of csrc/voxnav_gemm_f32.hip takes: 'dl' (16-deep
    direct-load), 'dl32' (32-deep) or 'staged'.  kind: linear (A, B row-major),
    dx (B k-major), tn (both k-major).  M, N: rows / columns of C; K: the
    reduction length; lda, ldb: the operands' leading dimensions (defaults:
    dense); aligned: every operand pointer is 16-B aligned."""
    a_km, b_km = kind == "tn", kind in ("dx", "tn")
    kper = K if kper is None else kper
    lda = (M if a_km else K) if lda is None else lda
    ldb = (N if b_km else K) if ldb is None else ldb
    dl = (gemm_dl != 0 and K % GKD == 0 and kper % GKD == 0 and lda % 4 == 0 and ldb % 4 == 0 and sa % 4 == 0 and
          sb % 4 == 0 and aligned and (not a_km or M % 4 == 0) and (not b_km or N % 4 == 0))
    if dl and gemm_k32 and K % 32 == 0 and kper % 32 == 0:
        return "dl32"
    return "dl" if dl else "staged"


def nblk(M: int, N: int, batch: int, splits: int = 1) -> int:
    return -(-M // GT) * -(-N // GT) * batch * splits


# ---------------------------------------------------------------- guard bands
class Slab:
    """`batch` matrices [rows][cols] with leading dimension ld and batch
    stride `stride` floats (0: one shared matrix; negative: later batches at
    lower addresses) inside one allocation pre-filled with SENTINEL, BAND
    guard floats on either side; `shift` floats move the payload off 16-B
    alignment.  ``intact()`` says that every float outside the matrices'
    [rows][cols] -- the bands, the padding columns of ld > cols, the gaps
    between batches -- still holds the sentinel (compared as int32)."""

    def __init__(self, dev, batch: int, rows: int, cols: int, ld: Optional[int] = None, stride: Optional[int] = None,
                 shift: int = 0):
        self.batch, self.rows, self.cols = batch, rows, cols
        self.ld = cols if ld is None else ld
        assert self.ld >= cols
        self.span = rows * self.ld
        self.stride = self.span if stride is None else stride
        assert self.stride == 0 or abs(self.stride) >= self.span
        self.nmat = 1 if self.stride == 0 else batch
        self.off0 = BAND + shift + (0 if self.stride >= 0 else (batch - 1) * -self.stride)
        total = BAND + shift + self.span + (self.nmat - 1) * abs(self.stride) + BAND
        self.raw = torch.full((total,), SENTINEL, dtype=torch.int32, device=dev)
        self.f = self.raw.view(torch.float32)
        assert self.f.data_ptr() % 16 == 0

    @property
    def ptr(self) -> int:
        return self.f.data_ptr() + 4 * self.off0

    @property
    def aligned(self) -> bool:
        return self.ptr % 16 == 0

    def mat(self, b: int) -> torch.Tensor:
        o = self.off0 + b * self.stride
        return self.f[o:o + self.span].view(self.rows, self.ld)[:, :self.cols]

    def put(self, data: torch.Tensor) -> "Slab":
        """data [nmat, rows, cols] (CPU f32)."""
        data = data.reshape(self.nmat, self.rows, self.cols)
        for b in range(self.nmat):
            self.mat(b).copy_(data[b])
        return self

    def get(self) -> torch.Tensor:
        return torch.stack([self.mat(b) for b in range(self.nmat)]).cpu()

    def intact(self) -> bool:
        total = self.raw.numel()
        starts = sorted(self.off0 + b * self.stride for b in range(self.nmat))
        parts = [self.raw[:starts[0]]]
        for s, nxt in zip(starts, starts[1:] + [total]):
            if self.ld > self.cols:
                parts.append(self.raw[s:s + self.span].view(self.rows, self.ld)[:, self.cols:].reshape(-1))
            parts.append(self.raw[s + self.span:nxt])
        return bool((torch.cat(parts) == SENTINEL).all().item())

    def untouched(self) -> bool:
        return bool((self.raw == SENTINEL).all().item())


def odd_stride(n: int) -> int:
    """The smallest stride >= n that is not a multiple of 4."""
    return n if n % 4 else n + 1


def round4(n: int) -> int:
    return -(-n // 4) * 4


def splits_recomputed(K: int, sp: int) -> int:
    return math.ceil(K / (math.ceil(math.ceil(K / sp) / 32) * 32))


# ------------------------------------------- error bounds through several layers
class ErrProp:
    """First-order error propagation through the learner's f32 kernels.  Every
    function takes float64 values together with an entrywise bound on the
    distance of the kernels' f32 values from them, and returns its float64
    result with such a bound: the summation bound of the product itself
    (above) plus the operands' bounds carried through the product's absolute
    values.  tanh: |tanh'| <= 1 and the measured tanhf tolerance; dZ = dy (1 -
    y^2): |d dZ / dy| <= 1, |d dZ / d y| = 2 |y| |dy|.  Terms of second order
    (a product of two bounds, below 1e-5 of the first-order ones at these
    sizes) are covered by SLACK."""
    SLACK = 1.01

    @staticmethod
    def linear(h, e_h, w, b):
        K, w64, b64 = h.shape[-1], w.double(), b.double()
        e = (K + 9) * U * (h.abs() @ w64.abs().T + b64.abs()) + e_h @ w64.abs().T
        return h @ w64.T + b64, ErrProp.SLACK * e

    @staticmethod
    def tanh(z, e_z):
        y = torch.tanh(z)
        return y, ErrProp.SLACK * (e_z + TANH_TOL_ULP * ulp32(y))

    @staticmethod
    def agrad(dy, e_dy, y, e_y):
        """-> dZ, its bound, and |dy| (1 + y^2) for the summation bounds."""
        a = dy.abs() * (1.0 + y * y)
        e = e_dy * (1.0 + y * y) + dy.abs() * 2.0 * y.abs() * e_y + 3.0 * U * a
        return dy * (1.0 - y * y), ErrProp.SLACK * e, a + e

    @staticmethod
    def dx(dz, e_dz, a_dz, w):
        """dZ [M][N] W [N][K]."""
        w64 = w.double()
        e = (dz.shape[-1] + 9) * U * (a_dz @ w64.abs()) + e_dz @ w64.abs()
        return dz @ w64, ErrProp.SLACK * e

    @staticmethod
    def tn(dz, e_dz, a_dz, x, e_x, splits=1):
        """(dZ^T X with bound, column sums of dZ with bound); dZ [M][N], X [M][K]."""
        f = (dz.shape[0] + splits + 8) * U
        e_w = f * (a_dz.T @ x.abs()) + e_dz.T @ x.abs() + a_dz.T @ e_x
        e_b = f * a_dz.sum(0) + e_dz.sum(0)
        return (dz.T @ x, ErrProp.SLACK * e_w), (dz.sum(0), ErrProp.SLACK * e_b)
