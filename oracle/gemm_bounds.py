"""The dinox_gemm argument contract on raw buffers: float64 reference, a-priori elementwise bounds, guarded buffers (CPU, no GPU).

include/dinox.h promises ONE contract for dinox_gemm -- leading dimensions that may exceed the width, batch strides where 0 means a
shared operand, alpha, ACCUM, colsum under ACCUM, a side tensor and a residual indexed per batch item as b * M * ld -- and ten device
kernels serve it.  This module states what every output ELEMENT must be (reference), how far fp32 arithmetic in ANY summation order
can land from that (bound), and lays the operands out so that a kernel which reads padding poisons its result and a kernel which
writes outside its window is caught (build, canary check).

Operands are bf16 (throughput mode); A is [M][K] / B is [N][K] ("NT", trans = 0) or A is [K][M] / B is [K][N] ("TN", trans = 1).

reference, following epilogue_store of csrc/gemm_common.h (float64 on the bf16 values; S = sum_k A B, T = sum_k |A| |B|):
    v = alpha S + bias[n]
    GELU:   aux[b M ldaux + m ldaux + n] = v  (gelu'(v) under AUXGRAD);  v = gelu(v)
    DGELU:  v *= gelu'(aux)                   (v *= aux under AUXGRAD)
    RESIDUAL: v += residual[b M ldr + m ldr + n];   ACCUM: v += C;   C[b strideC + m ldc + n] = v
    colsum[m] = sum_k A(m, k)  (+ colsum under ACCUM; never scaled by alpha)

bound (u = 2^-24; products of two bf16 values are exact in fp32, so only the additions round):
    accumulation     gamma_K |alpha| T,  gamma_K = K u / (1 - K u): any order of the K additions, split-K partial sums included
    combining        (ceil(K / 256) + EPI_OPS) u (|alpha| T + |bias| + |C_in|): the alpha product, the bias add, and the partial
                     sums of a split-K product meeting in C (atomics or the two-stage reduction; no split has fewer than 256 k)
    GELU             L_GELU e + 0.5 |v| ERF_AS_ERR + EPI_OPS u (|v| + |gelu v|)           (e = the error of v so far)
    GELU'            L_DGELU e + 0.5 ERF_AS_ERR + EXP_ERR(v) |v| pdf(v) + EPI_OPS u        (side tensor under AUXGRAD; factor of DGELU)
    x factor g       |g| e + |v| e_g + 2 u |v g|
    + residual, + C  2 u (|v| + |r|) each
    bf16 output      + half a bf16 ulp of |ref| + e: f32_to_bf16 of csrc/common.h is a plain cast, which hipcc lowers to
                     v_cvt_pk_bf16_f32, round to nearest even.  bf16 keeps 8 significant bits, so half an ulp of x is
                     2^(floor(log2 |x|) - 8): 2^-9 relative at the top of a binade, 2^-8 at its bottom (a flat 2^-9 |x| is NOT a
                     bound: correctly rounded values miss it by up to x 2).  fp32 outputs carry no further rounding.
    colsum           gamma_K sum_k |a| + (ceil(K / 256) + EPI_OPS) u (sum_k |a| + |colsum_in|)
L_GELU = max |gelu'| = 1.12897 and L_DGELU = max |gelu''| = 0.79788 are taken in float64 on a grid of 2^20 + 1 points of [-12, 12]
(lipschitz_constants()).

ERF_AS_ERR, the fast erf of csrc/common.h (erf_as, Abramowitz-Stegun 7.1.26: 1 rcp + 1 exp + 5 fma): measure_erf_as() evaluates the
SAME formula in NumPy float32 on 2^20 + 1 points of [-12, 12] against float64 erf, and adds what one ulp of the hardware reciprocal
(t: |d poly / dt| t e 2^-23) and the hardware exponential (e = __expf(-z^2) = exp2(-z^2 log2 e): (z^2 + 2) 2^-23 relative, one ulp of
v_exp_f32 plus the rounding of its argument) can move the result.  Measured: 5.34e-7 for the float32 formula alone, at z = -0.074
(the approximation itself is 1.39e-7 in float64, the published 1.5e-7; the rest is float32 cancellation in 1 - poly e, where the
polynomial's coefficients of +-1.4 leave a few ulp of 1.4), 1.13e-6 with the two hardware terms (tests/test_gemm_contract_cpu.py
re-measures both).  ERF_AS_ERR = 1.2e-6 -- eight times the "1.5e-7" that the comment in common.h quotes, still 2^-11 of a bf16
half-ulp.  Beyond |z| = 12 the exponential underflows and the formula returns exactly +-1.
The generic kernels call erff / __expf instead (a few ulp): inside the same constant.

fp32 operands (Spec.in_ = "f32": csrc/gemm_f32.hip, the parity-mode product) and the mixed layouts (Spec.trans_b != Spec.trans).  The
products of two fp32 values are no longer exact, but the exact-fp32 MFMA rounds a product once, TOGETHER with the sum it joins
(acc = fma(a, b, acc)): K roundings per output, each relative to a partial sum that T bounds, which is what gamma_K |alpha| T already
states.  No constant changes.  emulate() follows the kernel for these operands: one fma32() chain per output in ascending k (fma32 is
an exact float32 fused multiply-add: the product is exact in float64, the float64 sum is corrected to round-to-odd by the TwoSum
error term, and a round-to-odd float64 rounds to float32 as the exact value would -- 53 >= 24 + 2 bits).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace
from typing import Dict, Optional

import numpy as np

BIAS, GELU, DGELU, RESIDUAL, ACCUM, AUXGRAD = 1, 2, 4, 8, 16, 32       # DINOX_EPI_* of include/dinox.h

U32 = 2.0 ** -24                        # unit roundoff of fp32
EPI_OPS = 4                             # "a few u" per epilogue stage
ERF_AS_ERR = 1.2e-6                     # see the module docstring and measure_erf_as()
L_GELU = 1.12897                        # max |gelu'|  (lipschitz_constants())
L_DGELU = 0.79789                       # max |gelu''|

GUARD = 1024                            # elements of guard at both ends of every allocation
NAN_BF16 = np.uint16(0x7FC0)
CANARY_BF16 = np.uint16(0x7A5C)         # a bit pattern no test value has (bf16 3.6e35; the fp32 word below is 2.9e35)
CANARY_F32 = np.uint32(0x7A5C3CA5)


# ------------------------------------------------------------------------------------------ bf16 as uint16 bits
def bf16_round(x: np.ndarray) -> np.ndarray:
    """float -> bf16 bits, round to nearest even (finite values)."""
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def half_ulp_bf16(x: np.ndarray) -> np.ndarray:
    """Half a bf16 ulp at magnitude x (8 significant bits; the smallest normal binade below 2^-126)."""
    ex = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126)))
    return np.exp2(ex - 8.0)


def bf16_trunc(x: np.ndarray) -> np.ndarray:
    return (np.asarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_to_f64(b: np.ndarray) -> np.ndarray:
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------ an exact float32 fused multiply-add
def fma32(a, b, c) -> np.ndarray:
    """fl32(a b + c) with ONE rounding, elementwise, for finite float32 operands whose result is a normal float32.  The product of
    two float32 values is exact in float64 (48 bits).  s = fl64(p + c) and the TwoSum error term e give p + c = s + e exactly; where
    e != 0 the sum is moved to the neighbour with an odd last bit (round to odd), and a float64 rounded to odd rounds to float32
    exactly as the unrounded value does: the sticky bit survives, so no tie is invented and none is lost."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    p = a * b
    s = np.asarray(p + c)
    t = s - p
    e = (p - (s - t)) + (c - t)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    s = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def fma32_double_rounded(a, b, c) -> np.ndarray:
    """What fma32 must NOT be: the float64 sum rounded to float32 (two roundings)."""
    a, b, c = (np.asarray(x, dtype=np.float32).astype(np.float64) for x in (a, b, c))
    return (a * b + c).astype(np.float32)


# ------------------------------------------------------------------------------------------ GELU in float64, and the constants
_erf64 = np.vectorize(math.erf, otypes=[np.float64])


def gelu64(x):
    return 0.5 * x * (1.0 + _erf64(x * math.sqrt(0.5)))


def pdf64(x):
    return np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def dgelu64(x):
    return 0.5 * (1.0 + _erf64(x * math.sqrt(0.5))) + x * pdf64(x)


def lipschitz_constants(points: int = (1 << 20) + 1):
    x = np.linspace(-12.0, 12.0, points)
    return float(np.abs(dgelu64(x)).max()), float(np.abs(pdf64(x) * (2.0 - x * x)).max())


_AS = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)


def erf_as_f32(z: np.ndarray):
    """erf_as of csrc/common.h in NumPy float32, operation for operation; returns (erf, t, e, poly)."""
    f = np.float32
    z = np.asarray(z, dtype=f)
    a = np.abs(z)
    t = f(1.0) / (f(1.0) + f(0.3275911) * a)
    e = np.exp(-a * a).astype(f)
    poly = t * (f(_AS[0]) + t * (f(_AS[1]) + t * (f(_AS[2]) + t * (f(_AS[3]) + t * f(_AS[4])))))
    return np.copysign(f(1.0) - poly * e, z), t, e, poly


def measure_erf_as(points: int = (1 << 20) + 1):
    """(error of the float32 formula alone, error with one ulp each of the hardware rcp and exp) over [-12, 12]."""
    z = np.linspace(-12.0, 12.0, points).astype(np.float32)
    got, t, e, poly = erf_as_f32(z)
    plain = np.abs(got.astype(np.float64) - _erf64(z.astype(np.float64)))
    t, e, poly, a = t.astype(np.float64), e.astype(np.float64), poly.astype(np.float64), np.abs(z.astype(np.float64))
    dpoly = _AS[0] + 2 * _AS[1] * t + 3 * _AS[2] * t ** 2 + 4 * _AS[3] * t ** 3 + 5 * _AS[4] * t ** 4
    hw = np.abs(dpoly) * t * e * 2.0 ** -23 + poly * e * (a * a + 2.0) * 2.0 ** -23
    return float(plain.max()), float((plain + hw).max())


def _gelu_eval_err(v):
    return 0.5 * np.abs(v) * ERF_AS_ERR + EPI_OPS * U32 * (np.abs(v) + np.abs(gelu64(v)))


def _dgelu_eval_err(v):
    return 0.5 * ERF_AS_ERR + (v * v + 2.0) * 2.0 ** -23 * np.abs(v) * pdf64(v) + EPI_OPS * U32


# ------------------------------------------------------------------------------------------ the argument set
@dataclass(frozen=True)
class Spec:
    """dinox_gemm_args without the pointers.  pad* = leading dimension minus width; gap* = elements between batch items beyond one
    item's extent (negative: the items' extents overlap, as in the split-K form where item c starts K elements further along every
    row of one wide matrix -- no ELEMENT belongs to two items); off* = byte offset of the operand's first element from a 16-byte
    boundary."""
    M: int
    N: int
    K: int
    trans: int = 0                      # 0: NT, 1: TN (transA; transB too unless trans_b is given)
    out: str = "bf16"                   # "bf16" | "f32": C and the side tensor
    epi: int = 0
    alpha: float = 1.0
    batch: int = 1
    aux: bool = False                   # side tensor present (GELU: written; DGELU: read)
    colsum: bool = False
    pad_a: int = 0
    pad_b: int = 0
    pad_c: int = 0
    pad_r: int = 0
    pad_x: int = 0
    share_a: bool = False
    share_b: bool = False
    gap_a: int = 0
    gap_b: int = 0
    gap_c: int = 0
    off_a: int = 0
    off_b: int = 0
    off_c: int = 0
    seed: int = 0
    in_: str = "bf16"                   # "bf16" | "f32": A and B
    trans_b: Optional[int] = None       # transB; None: equal to trans

    @property
    def tb(self) -> int:
        return self.trans if self.trans_b is None else self.trans_b

    # shapes as stored
    @property
    def a_shape(self):
        return (self.K, self.M) if self.trans else (self.M, self.K)

    @property
    def b_shape(self):
        return (self.K, self.N) if self.tb else (self.N, self.K)

    @property
    def lda(self):
        return self.a_shape[1] + self.pad_a

    @property
    def ldb(self):
        return self.b_shape[1] + self.pad_b

    @property
    def ldc(self):
        return self.N + self.pad_c

    @property
    def ldr(self):
        return self.N + self.pad_r

    @property
    def ldaux(self):
        return self.N + self.pad_x

    @property
    def stride_a(self):
        return 0 if self.share_a else self.a_shape[0] * self.lda + self.gap_a

    @property
    def stride_b(self):
        return 0 if self.share_b else self.b_shape[0] * self.ldb + self.gap_b

    @property
    def stride_c(self):
        return self.M * self.ldc + self.gap_c

    def but(self, **kw) -> "Spec":
        return replace(self, **kw)


@dataclass
class Buf:
    """One allocation: `data` (uint16 bf16 bits or float32), the operand's first element at `origin`, the element index of every live
    (b, row, col) in `idx`; everything outside idx is padding (NaN for inputs, canary words for outputs)."""
    data: np.ndarray
    origin: int
    idx: np.ndarray
    output: bool

    def live(self) -> np.ndarray:
        v = self.data[self.idx]
        return bf16_to_f64(v) if self.data.dtype == np.uint16 else v.astype(np.float64)

    def words(self) -> np.ndarray:
        return self.data.view(np.uint16 if self.data.dtype == np.uint16 else np.uint32)

    def copy(self) -> "Buf":
        return Buf(self.data.copy(), self.origin, self.idx, self.output)


def _layout(nb: int, rows: int, cols: int, ld: int, stride: int, off_elems: int):
    origin = GUARD + off_elems
    b = np.arange(nb if stride else 1).reshape(-1, 1, 1)
    idx = origin + b * stride + np.arange(rows).reshape(1, -1, 1) * ld + np.arange(cols).reshape(1, 1, -1)
    if not stride and nb > 1:
        idx = np.broadcast_to(idx, (nb, rows, cols))
    return origin, idx, int(idx.max()) + 1 + GUARD + 8


def _make(values: np.ndarray, bf16: bool, nb, rows, cols, ld, stride, off_bytes, output: bool, fill_live: bool = True) -> Buf:
    esz = 2 if bf16 else 4
    assert off_bytes % esz == 0
    origin, idx, total = _layout(nb, rows, cols, ld, stride, off_bytes // esz)
    if bf16:
        data = np.full(total, CANARY_BF16 if output else NAN_BF16, dtype=np.uint16)
    else:
        data = np.full(total, CANARY_F32, dtype=np.uint32).view(np.float32) if output else np.full(total, np.nan, dtype=np.float32)
    if fill_live:
        own = idx if stride or nb == 1 else idx[:1]
        vals = values[: own.shape[0]]
        data[own] = bf16_round(vals) if bf16 else vals.astype(np.float32)
    return Buf(data, origin, idx, output)


def build(s: Spec) -> Dict[str, Buf]:
    """Every operand of `s` in a guarded allocation of its own.  Values: A, B ~ randn scaled so that the pre-activation has a standard
    deviation of about 1.5 (the GELU's curved range), bias ~ 0.5 randn, residual, C (under ACCUM) and the GELU' input ~ randn."""
    rng = np.random.default_rng(1000 + s.seed)
    sc = math.sqrt(1.5 / math.sqrt(s.K) / max(abs(s.alpha), 0.25))
    ar, ac = s.a_shape
    br, bc = s.b_shape
    out16 = s.out == "bf16"
    in16 = s.in_ == "bf16"
    bufs = {
        "A": _make(rng.standard_normal((s.batch, ar, ac)) * sc, in16, s.batch, ar, ac, s.lda, s.stride_a, s.off_a, False),
        "B": _make(rng.standard_normal((s.batch, br, bc)) * sc, in16, s.batch, br, bc, s.ldb, s.stride_b, s.off_b, False),
        "C": _make(rng.standard_normal((s.batch, s.M, s.N)), out16, s.batch, s.M, s.N, s.ldc, s.stride_c, s.off_c, True,
                   fill_live=bool(s.epi & ACCUM)),
    }
    if s.epi & BIAS:
        bufs["bias"] = _make(rng.standard_normal((1, 1, s.N)) * 0.5, False, 1, 1, s.N, s.N, 0, 0, False)
    if s.epi & RESIDUAL:
        bufs["residual"] = _make(rng.standard_normal((s.batch, s.M, s.N)), False, s.batch, s.M, s.N, s.ldr, s.M * s.ldr, 0, False)
    if s.aux:
        reads = bool(s.epi & DGELU)
        bufs["aux"] = _make(rng.standard_normal((s.batch, s.M, s.N)) * 1.5, out16, s.batch, s.M, s.N, s.ldaux, s.M * s.ldaux, 0,
                            not reads, fill_live=reads)
    if s.colsum:
        bufs["colsum"] = _make(rng.standard_normal((1, 1, s.M)), False, 1, 1, s.M, s.M, 0, 0, True, fill_live=bool(s.epi & ACCUM))
    return bufs


OUTPUTS = ("C", "aux", "colsum")


def is_output(s: Spec, name: str) -> bool:
    return name == "C" or name == "colsum" or (name == "aux" and bool(s.epi & GELU))


# ------------------------------------------------------------------------------------------ reference and bound
def _operands(s: Spec, bufs):
    A, B = bufs["A"].live(), bufs["B"].live()          # [batch][rows][cols] as stored
    if s.trans:
        A = A.transpose(0, 2, 1)
    if s.tb:
        B = B.transpose(0, 2, 1)
    return A, B                                        # [batch][M][K], [batch][N][K]


def reference(s: Spec, bufs: Dict[str, Buf], with_bound: bool = True):
    """{'C': [batch][M][N], 'aux': ..., 'colsum': [M]} in float64, and the same keys + '_bound' when asked."""
    A, B = _operands(s, bufs)
    S = np.einsum("bmk,bnk->bmn", A, B)
    T = np.einsum("bmk,bnk->bmn", np.abs(A), np.abs(B))
    K = s.K
    gam = K * U32 / (1.0 - K * U32)
    comb = (math.ceil(K / 256) + EPI_OPS) * U32
    al = abs(s.alpha)
    bias = bufs["bias"].live() if s.epi & BIAS else np.zeros((1, 1, s.N))
    c_in = bufs["C"].live() if s.epi & ACCUM else np.zeros_like(S)
    v = s.alpha * S + bias
    e = gam * al * T + comb * (al * T + np.abs(bias) + np.abs(c_in))
    out = {}
    out16 = s.out == "bf16"

    def rounded(ref, err):
        return err + half_ulp_bf16(np.abs(ref) + err) if out16 else err

    if s.epi & GELU:
        if s.aux:
            if s.epi & AUXGRAD:
                out["aux"], xe = dgelu64(v), L_DGELU * e + _dgelu_eval_err(v)
            else:
                out["aux"], xe = v, e
            out["aux_bound"] = rounded(out["aux"], xe)
        e = L_GELU * e + _gelu_eval_err(v)
        v = gelu64(v)
    if s.epi & DGELU:
        x = bufs["aux"].live()
        g, ge = (x, np.zeros_like(x)) if s.epi & AUXGRAD else (dgelu64(x), _dgelu_eval_err(x))
        e = np.abs(g) * e + np.abs(v) * ge + 2 * U32 * np.abs(v * g)
        v = v * g
    if s.epi & RESIDUAL:
        r = bufs["residual"].live()
        e = e + 2 * U32 * (np.abs(v) + np.abs(r))
        v = v + r
    if s.epi & ACCUM:
        e = e + 2 * U32 * (np.abs(v) + np.abs(c_in))
        v = v + c_in
    out["C"], out["C_bound"] = v, rounded(v, e)
    if s.colsum:
        A0 = A[0]
        cs_in = bufs["colsum"].live().reshape(-1) if s.epi & ACCUM else np.zeros(s.M)
        sa = np.abs(A0).sum(1)
        out["colsum"] = A0.sum(1) + cs_in
        out["colsum_bound"] = gam * sa + comb * (sa + np.abs(cs_in)) + 2 * U32 * np.abs(out["colsum"])
    if not with_bound:
        out = {k: x for k, x in out.items() if not k.endswith("_bound")}
    return out


# ------------------------------------------------------------------------------------------ judging a result
def check(s: Spec, before: Dict[str, Buf], after: Dict[str, np.ndarray], ref: Optional[dict] = None) -> dict:
    """`before`: the buffers as built; `after`: name -> the raw array after the launch, for every output (C, the written side tensor,
    colsum).  Every live element is compared (none is exempt) and every padding word.  Returns, per output, ratio_<name> = the
    largest |got - ref| / bound, where_<name> = its (b, m, n); nan = number of non-finite live elements; canary = number of padding
    words that changed, canary_at = the first few (name, element index); ok = ratio <= 1 everywhere, no NaN, no canary touched."""
    ref = ref or reference(s, before)
    r = {"nan": 0, "canary": 0, "canary_at": [], "compared": 0, "exempt": 0}
    for name in OUTPUTS:
        if name not in before or not is_output(s, name):
            continue
        b0 = before[name]
        got_buf = Buf(np.asarray(after[name]), b0.origin, b0.idx, True)
        assert got_buf.data.dtype == b0.data.dtype and got_buf.data.shape == b0.data.shape, name
        got = got_buf.live().reshape(ref[name].shape)
        bad = ~np.isfinite(got)
        r["nan"] += int(bad.sum())
        ratio = np.where(bad, np.inf, np.abs(np.where(bad, 0.0, got) - ref[name]) / ref[name + "_bound"])
        r["compared"] += ratio.size
        at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        r["ratio_" + name], r["where_" + name] = float(ratio[at]), tuple(int(i) for i in at)
        pad = np.ones(b0.data.shape, dtype=bool)
        pad[b0.idx.reshape(-1)] = False
        changed = np.nonzero(pad & (got_buf.words() != b0.words()))[0]
        r["canary"] += int(changed.size)
        r["canary_at"] += [(name, int(i) - b0.origin) for i in changed[:4]]
    r["ratio"] = max(v for k, v in r.items() if k.startswith("ratio_"))
    r["ok"] = r["ratio"] <= 1.0 and r["nan"] == 0 and r["canary"] == 0
    return r


# ------------------------------------------------------------------------------------------ the documented arithmetic on the CPU
def _gelu_both_f32(x):
    """gelu_fast_both of csrc/common.h in float32."""
    f = np.float32
    er, _, _, _ = erf_as_f32(x * f(0.70710678118654752))
    e = np.exp(f(-0.5) * x * x).astype(f)
    h = f(0.5) * (f(1.0) + er)
    return x * h, h + x * e * f(0.39894228040143268)


def _gather(buf: Buf, rel: np.ndarray) -> np.ndarray:
    """float64 values at element offsets `rel` from the operand's first element, as a kernel with a wrong index would read them: NaN
    padding where it lands on padding, NaN too outside the allocation (the emulation does not fault)."""
    idx = buf.origin + rel
    ok = (idx >= 0) & (idx < buf.data.size)
    v = buf.data[np.where(ok, idx, 0)]
    v = bf16_to_f64(v) if buf.data.dtype == np.uint16 else v.astype(np.float64)
    return np.where(ok, v, np.nan)


def emulate(s: Spec, bufs: Dict[str, Buf], order: str = "seq", mutant: Optional[str] = None) -> Dict[str, np.ndarray]:
    """The kernels' documented arithmetic on the CPU: float32 accumulation of the exact bf16 products (order "seq": k ascending;
    "blk32": blocks of 32 summed on their own, then added in order), float32 epilogue with the fast erf, bf16 rounding.  With fp32
    operands every step is acc = fma32(a, b, acc): order "seq" is then the chain that csrc/gemm_f32.hip documents.  Works on the
    raw buffers and returns the output arrays as a launch would leave them.  `mutant` plants one defect (MUTANTS)."""
    f = np.float32
    A, B = _operands(s, bufs)
    if mutant == "trans_b_follows_a" and s.tb != s.trans:
        n, k = np.arange(s.N).reshape(1, -1, 1), np.arange(s.K).reshape(1, 1, -1)
        B = _gather(bufs["B"], np.arange(s.batch).reshape(-1, 1, 1) * s.stride_b + (n + k * s.ldb if s.trans else n * s.ldb + k))
    if mutant == "batch_stride_as_extent" and s.batch > 1 and not s.share_a:
        m, k = np.arange(s.M).reshape(1, -1, 1), np.arange(s.K).reshape(1, 1, -1)
        A = _gather(bufs["A"], np.arange(s.batch).reshape(-1, 1, 1) * (s.a_shape[0] * s.lda) + (m + k * s.lda if s.trans else m * s.lda + k))
    A, B = A.astype(f), B.astype(f)
    if mutant == "batch1_uses_b0" and s.batch > 1:
        B = B.copy()
        B[1] = B[0]
    ks = list(range(s.K))
    if mutant == "drop_last_8k":
        ks = ks[:-8]
    if mutant == "odd_k_dropped" and s.K % 2:
        ks = ks[:-1]
    if mutant == "stale_last_slab" and s.K > 16:                  # the last 16-slab is never fetched: the one before it is multiplied twice
        last = (s.K - 1) // 16 * 16
        ks = ks[:last] + ks[last - 16:last]
    fused = s.in_ == "f32"                                        # fp32 operands: the product is rounded once, with the sum
    acc = np.zeros((s.batch, s.M, s.N), dtype=f)
    part = np.zeros_like(acc)
    cs = np.zeros(s.M, dtype=f)
    for i, k in enumerate(ks):
        a, b = A[:, :, k, None], B[:, None, :, k]
        if order == "seq":
            acc = fma32(a, b, acc) if fused else acc + a * b
        else:
            part = fma32(a, b, part) if fused else part + a * b
            if i % 32 == 31 or i == len(ks) - 1:
                acc += part
                part[...] = 0
        cs += A[0, :, k]
    if mutant == "edge_row_map" and s.M % 32:                     # accumulator j of half h holds row (j & 3) + 8 (j >> 2) + 4 h of a 32-row
        row0 = s.M - s.M % 32                                     # block; the defect stores it at (j >> 2) + 8 (j & 3) + 4 h
        moved = acc.copy()
        for l in range(32):
            to = row0 + (l >> 3) + 8 * (l & 3) + (l & 4)
            if to < s.M:
                moved[:, to] = acc[:, row0 + l] if row0 + l < s.M else 0
        acc = moved
    alpha = f(1.0) if mutant == "alpha_ignored" else f(s.alpha)
    v = acc * alpha
    if s.epi & BIAS:
        bias = bufs["bias"].live().astype(f).reshape(-1)
        if mutant == "bias_shift_last_strip":
            bias = bias.copy()
            bias[s.N - 8:] = np.roll(bias, -1)[s.N - 8:]
        v = v + bias
    out = {k: bufs[k].data.copy() for k in OUTPUTS if k in bufs and is_output(s, k)}
    out16 = s.out == "bf16"
    cvt = (bf16_trunc if mutant == "bf16_truncated" else bf16_round) if out16 else (lambda x: x.astype(f))
    if s.epi & GELU:
        y, d = _gelu_both_f32(v)
        if s.aux:
            xb = bufs["aux"]
            idx = xb.idx
            if mutant == "ldaux_taken_as_n":
                idx = xb.origin + (np.arange(s.batch).reshape(-1, 1, 1) * s.M + np.arange(s.M).reshape(1, -1, 1)) * s.N + np.arange(s.N)
            out["aux"][idx] = cvt(d if s.epi & AUXGRAD else v)
        v = y
    if s.epi & DGELU:
        x = bufs["aux"].live().astype(f)
        v = v * (x if s.epi & AUXGRAD else _gelu_both_f32(x)[1])
    if s.epi & RESIDUAL:
        rb = bufs["residual"]
        idx = rb.idx
        if mutant == "ldr_taken_as_n":
            idx = rb.origin + (np.arange(s.batch).reshape(-1, 1, 1) * s.M + np.arange(s.M).reshape(1, -1, 1)) * s.N + np.arange(s.N)
        v = v + rb.data[idx]
    if s.epi & ACCUM and mutant != "accum_overwrites":
        v = v + bufs["C"].live().astype(f)
    out["C"][bufs["C"].idx] = cvt(v)
    if s.colsum:
        out["colsum"][bufs["colsum"].idx.reshape(-1)] = cs + (bufs["colsum"].live().astype(f).reshape(-1) if s.epi & ACCUM else f(0))
    if mutant == "canary_word":
        w = out["C"].view(np.uint16 if out16 else np.uint32)
        w[bufs["C"].origin + s.N if s.ldc > s.N else bufs["C"].origin - 1] ^= 1
    return out


MUTANTS = ("drop_last_8k", "alpha_ignored", "bias_shift_last_strip", "accum_overwrites", "ldr_taken_as_n", "ldaux_taken_as_n",
           "batch1_uses_b0", "bf16_truncated", "canary_word")
# defects of the kind csrc/gemm_f32.hip could have (tests/test_gemm_f32_contract_cpu.py): the last k of an odd K (a K-step of two that
# does not guard its second half), the prefetch guard of the 128-tile kernel off by one slab, B read with A's layout flag, a
# permuted accumulator-to-row map inside the last partial 32-row block, and the batch stride taken as rows x ld (what breaks the
# split-K argument form, whose items overlap)
F32_MUTANTS = ("odd_k_dropped", "stale_last_slab", "trans_b_follows_a", "edge_row_map", "batch_stride_as_extent")
MUTANTS_ALL = MUTANTS + F32_MUTANTS


# ------------------------------------------------------------------------------------------ the cases of the contract tests
# kernel -> (how to force it, [(M, N, K)]): the smallest shapes with a full tile, a ragged edge in M and N and an 8-column last strip.
NT_SHAPES = {
    "gemm_bf16_nt_pp": [(256 + 17, 256 + 8, 192)],
    "gemm_bf16_nt_pp128": [(256 + 17, 128 + 8, 192)],
    "gemm_bf16_nt_pp384": [(208 + 1, 384, 128), (208 + 1, 384, 256)],
    "gemm_bf16_nt_areg": [(128 + 5, 128 + 8, 384)],
    "gemm_bf16_nt_glds": [(128 + 5, 136, 128), (128 + 5, 136, 576)],        # K <= 512: the 3-stage BK = 32 ring; longer: 2-stage BK = 64
    "gemm_bf16_nt": [(77, 24, 40)],
}
F32_SHAPES = {"gemm_f32": [(77, 24, 44)]}                                   # K % 8 != 0: outside every bf16 MFMA kernel
TN_SHAPES = {
    "gemm_bf16_tn_dma": [(136, 72, 200), (136, 72, 1000)],                  # one split, several
    "gemm_bf16_tn_big": [(64, 72, 8192 + 40)],
}
NT_ALL = {**NT_SHAPES, **F32_SHAPES}
KERNELS = list(NT_ALL) + list(TN_SHAPES)
# environment that forces each kernel (DINOX_* knobs of csrc/knobs.h; monkeypatch.setenv in the tests)
FORCE = {
    "gemm_bf16_nt_pp": {"DINOX_NT_PP": "3", "DINOX_NT_PP384": "0"},
    "gemm_bf16_nt_pp128": {"DINOX_NT_PP": "2", "DINOX_NT_PP384": "0"},
    "gemm_bf16_nt_pp384": {"DINOX_NT_PP": "1", "DINOX_NT_PP384": "1"},
    "gemm_bf16_nt_areg": {"DINOX_NT_PP": "0", "DINOX_NT_AREG_MAXK": "576"},
    "gemm_bf16_nt_glds": {"DINOX_NT_PP": "0", "DINOX_NT_AREG_MAXK": "0"},
    "gemm_bf16_nt": {"DINOX_NT_PP": "0"},
    "gemm_bf16_tn_dma": {},
    "gemm_bf16_tn_big": {},
    "gemm_f32": {"DINOX_NT_PP": "0"},
}
# leading dimensions larger than the width by DIFFERENT amounts that keep every kernel's alignment rule (lda, ldb % 8; ldc, ldaux
# rows of 16 bytes in either output type; ldr % 4)
PADS = dict(pad_a=8, pad_b=24, pad_c=16, pad_r=4, pad_x=40)
NT_EPILOGUES = {
    "plain": dict(),
    "bias": dict(epi=BIAS),
    "gelu_aux": dict(epi=BIAS | GELU, aux=True),
    "gelu_auxgrad": dict(epi=BIAS | GELU | AUXGRAD, aux=True),
    "dgelu": dict(epi=DGELU, aux=True),
    "dgelu_auxgrad": dict(epi=DGELU | AUXGRAD, aux=True),
    "residual": dict(epi=BIAS | RESIDUAL),
}


def strided_cases(kernel: str):
    """Variant 1: every leading dimension padded, both output types, every epilogue the kernel family takes."""
    if kernel in NT_ALL:
        for (M, N, K) in NT_ALL[kernel]:
            for out in ("bf16", "f32"):
                for name, kw in NT_EPILOGUES.items():
                    yield f"{M}x{N}x{K}-{out}-{name}", Spec(M, N, K, out=out, seed=len(name) + K, **PADS, **kw)
    else:
        for (M, N, K) in TN_SHAPES[kernel]:
            yield f"{M}x{N}x{K}-f32-plain", Spec(M, N, K, trans=1, out="f32", seed=K, pad_a=8, pad_b=24)
            yield f"{M}x{N}x{K}-f32-colsum", Spec(M, N, K, trans=1, out="f32", seed=K + 1, pad_a=16, pad_b=8, colsum=True)
            yield f"{M}x{N}x{K}-f32-ldc", Spec(M, N, K, trans=1, out="f32", seed=K + 2, pad_a=8, pad_b=24, pad_c=16)
            yield f"{M}x{N}x{K}-bf16-bias-ldc", Spec(M, N, K, trans=1, out="bf16", seed=K + 3, epi=BIAS, pad_a=8, pad_b=24, pad_c=16)


def batched_cases(kernel: str):
    """Variant 2: batch = 3 with own B, shared B, shared A, and a gap in strideC; side tensor and residual included."""
    shapes = NT_ALL.get(kernel) or TN_SHAPES[kernel]
    M, N, K = shapes[0]
    t = 0 if kernel in NT_ALL else 1
    base = Spec(M, N, K, trans=t, batch=3, out="f32", seed=7, pad_a=8, pad_b=24, pad_c=16)
    yield "own_b", base.but(gap_a=8, gap_b=16)
    yield "shared_b", base.but(share_b=True, gap_a=8)
    yield "shared_a", base.but(share_a=True, gap_b=16)
    yield "stride_c_gap", base.but(gap_c=48, gap_a=8)
    if not t:
        yield "residual", base.but(epi=BIAS | RESIDUAL, pad_r=4, gap_c=16)
        yield "gelu_aux", base.but(out="bf16", epi=BIAS | GELU, aux=True, pad_x=40, gap_c=16)
        yield "dgelu", base.but(out="bf16", epi=DGELU, aux=True, pad_x=40, share_b=True)


def alpha_cases(kernel: str):
    """Variant 3: alpha in {0.375, -1.5} with bias and with ACCUM."""
    shapes = NT_ALL.get(kernel) or TN_SHAPES[kernel]
    M, N, K = shapes[-1]
    t = 0 if kernel in NT_ALL else 1
    for alpha in (0.375, -1.5):
        if not t:
            yield f"alpha{alpha}-bias", Spec(M, N, K, out="bf16", epi=BIAS, alpha=alpha, seed=11, **PADS)
        else:
            yield f"alpha{alpha}-plain", Spec(M, N, K, trans=1, out="f32", alpha=alpha, seed=11, pad_a=8, pad_b=24)
        yield f"alpha{alpha}-accum", Spec(M, N, K, trans=t, out="f32", epi=ACCUM | (0 if t else BIAS), alpha=alpha, seed=12, pad_a=8, pad_b=24,
                                          pad_c=0 if t else 16)


def accum_cases():
    """Variant 4: ACCUM wherever a kernel takes it (name -> (expected kernel, spec, workspace?))."""
    yield "nt", ("gemm_bf16_nt", Spec(77, 24, 40, out="f32", epi=ACCUM | BIAS, seed=21, **PADS), False)
    yield "nt_batch", ("gemm_bf16_nt", Spec(77, 24, 40, out="f32", epi=ACCUM, batch=3, gap_c=8, seed=22, **PADS), False)
    for ws in (False, True):
        tag = "ws" if ws else "atomics"
        yield f"tn_dma_{tag}", ("gemm_bf16_tn_dma", Spec(136, 72, 1000, trans=1, out="f32", epi=ACCUM, seed=23, pad_a=8, pad_b=24), ws)
        yield f"tn_dma_colsum_{tag}", ("gemm_bf16_tn_dma", Spec(136, 72, 1000, trans=1, out="f32", epi=ACCUM, colsum=True, seed=24, pad_a=16, pad_b=8), ws)
    yield "tn_dma_ldc_long_k", ("gemm_bf16_tn_dma", Spec(136, 72, 1000, trans=1, out="f32", epi=ACCUM, seed=25, pad_a=8, pad_b=24, pad_c=16), True)
    yield "tn_dma_ldc_long_k_overwrite", ("gemm_bf16_tn_dma", Spec(136, 72, 1000, trans=1, out="f32", seed=26, pad_a=8, pad_b=24, pad_c=16, colsum=True), False)
    yield "tn_big", ("gemm_bf16_tn_big", Spec(64, 72, 8192 + 40, trans=1, out="f32", epi=ACCUM, seed=27, pad_a=8, pad_b=24), True)
    yield "tn_big_colsum", ("gemm_bf16_tn_big", Spec(64, 72, 8192 + 40, trans=1, out="f32", epi=ACCUM, colsum=True, seed=28, pad_a=16, pad_b=8), True)
    yield "f32_nt", ("gemm_f32", Spec(77, 24, 44, out="f32", epi=ACCUM | BIAS, alpha=0.375, seed=29, pad_a=4, pad_b=12, pad_c=8), False)
    yield "f32_tn_colsum", ("gemm_f32", Spec(76, 20, 44, trans=1, out="f32", epi=ACCUM, colsum=True, seed=30, pad_a=4, pad_b=12, pad_c=8), False)


def misaligned_cases():
    """Variant 5: operands and C at an 8-byte (not 16-byte) offset, ldr odd: whatever kernel is named must stay inside the bound."""
    yield "nt_a_off8", Spec(133, 136, 384, out="bf16", epi=BIAS, off_a=8, seed=31, **PADS)
    yield "nt_b_off8", Spec(133, 136, 128, out="f32", epi=BIAS | RESIDUAL, off_b=8, seed=32, **PADS)
    yield "nt_c_off8", Spec(133, 136, 384, out="bf16", epi=BIAS | GELU | AUXGRAD, aux=True, off_c=8, seed=33, **PADS)
    yield "nt_c_off8_f32", Spec(273, 264, 192, out="f32", epi=BIAS | RESIDUAL, off_c=8, seed=34, **PADS)
    yield "nt_ldr_odd", Spec(133, 136, 384, out="f32", epi=BIAS | RESIDUAL, seed=35, **{**PADS, "pad_r": 5})
    yield "nt_ldr_odd_pp", Spec(273, 264, 192, out="f32", epi=RESIDUAL, seed=36, **{**PADS, "pad_r": 3})
    yield "tn_a_off8", Spec(136, 72, 200, trans=1, out="f32", off_a=8, seed=37, pad_a=8, pad_b=24)
    yield "tn_c_off8", Spec(136, 72, 1000, trans=1, out="f32", off_c=8, colsum=True, seed=38, pad_a=8, pad_b=24)
    yield "nt_all_off8", Spec(77, 24, 40, out="bf16", epi=BIAS | DGELU, aux=True, off_a=8, off_b=8, off_c=8, seed=39, **PADS)


def cpu_families():
    """One representative of every case family the GPU tests run, at shapes the CPU emulation finishes in well under a second each."""
    yield "strided-bias", Spec(77, 24, 40, out="bf16", epi=BIAS, **PADS)
    yield "strided-gelu-aux", Spec(45, 24, 64, out="bf16", epi=BIAS | GELU, aux=True, seed=1, **PADS)
    yield "strided-gelu-auxgrad-f32", Spec(45, 24, 64, out="f32", epi=BIAS | GELU | AUXGRAD, aux=True, seed=2, **PADS)
    yield "strided-dgelu", Spec(45, 24, 64, out="bf16", epi=DGELU, aux=True, seed=3, **PADS)
    yield "strided-dgelu-auxgrad-f32", Spec(45, 24, 64, out="f32", epi=DGELU | AUXGRAD, aux=True, seed=4, **PADS)
    yield "strided-residual", Spec(45, 24, 64, out="f32", epi=BIAS | RESIDUAL, seed=5, **PADS)
    yield "batched-own-b", Spec(37, 24, 48, batch=3, out="f32", gap_a=8, gap_b=16, gap_c=48, seed=6, **PADS)
    yield "batched-shared-b-residual", Spec(37, 24, 48, batch=3, out="f32", epi=BIAS | RESIDUAL, share_b=True, seed=7, **PADS)
    yield "batched-shared-a-gelu", Spec(37, 24, 48, batch=3, out="bf16", epi=BIAS | GELU, aux=True, share_a=True, seed=8, **PADS)
    yield "alpha-bias", Spec(45, 24, 64, out="bf16", epi=BIAS, alpha=0.375, seed=9, **PADS)
    yield "alpha-accum", Spec(45, 24, 64, out="f32", epi=BIAS | ACCUM, alpha=-1.5, seed=10, **PADS)
    yield "tn-accum-colsum", Spec(40, 24, 1000, trans=1, out="f32", epi=ACCUM, colsum=True, seed=11, pad_a=16, pad_b=8)
    yield "tn-long-k", Spec(16, 24, 8192 + 40, trans=1, out="f32", seed=12, pad_a=8, pad_b=24)
    yield "misaligned", Spec(45, 24, 40, out="bf16", epi=BIAS | DGELU, aux=True, off_a=8, off_b=8, off_c=8, seed=13, **{**PADS, "pad_r": 5})


# ------------------------------------------------------------------------------------------ the exact-fp32 kernels (csrc/gemm_f32.hip)
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))                          # (transA, transB); (0, 1) is the P V product of fp32 attention
# gemm_f32 has no alignment rule: odd paddings, all different
F32_PADS = dict(pad_a=3, pad_b=7, pad_c=5, pad_r=1, pad_x=9)
F32_EPILOGUES = {
    "plain": dict(),
    "bias": dict(epi=BIAS),
    "gelu_aux": dict(epi=BIAS | GELU, aux=True),
    "gelu_auxgrad": dict(epi=BIAS | GELU | AUXGRAD, aux=True),
    "dgelu": dict(epi=DGELU, aux=True),
    "dgelu_auxgrad": dict(epi=DGELU | AUXGRAD, aux=True),
    "residual": dict(epi=RESIDUAL),
    "accum_bias": dict(epi=ACCUM | BIAS, alpha=-1.5),               # fp32 C only
}


def uses_big_tiles(s: Spec) -> bool:
    """launch_gemm_f32's predicate: 128 x 128 tiles (gemm_f32_big) when both extents reach 128 and there is a tile per CU."""
    return s.M >= 128 and s.N >= 128 and -(-s.M // 128) * -(-s.N // 128) * s.batch >= 256


def _lay(ta: int, tb: int) -> dict:
    return dict(trans=ta, trans_b=tb)


def f32_layout_cases():
    """All four layouts x both operand types x both output types at (77, 24, 44) and (65, 130, 17) -- one full tile plus one row,
    three column tiles, K one past a slab -- every leading dimension padded, the epilogues cycling so that each meets at least two
    layouts and both output types (tests/test_gemm_f32_contract_cpu.py counts them)."""
    names = list(F32_EPILOGUES)
    for si, (M, N, K) in enumerate(((77, 24, 44), (65, 130, 17))):
        for li, (ta, tb) in enumerate(LAYOUTS):
            for ii, in_ in enumerate(("f32", "bf16")):
                n = li * 2 + ii
                for out in ("f32", "bf16"):
                    name = names[(n + 3 * si) % 8] if out == "f32" else names[(n + 3 * si) % 7]
                    yield (f"{M}x{N}x{K}-{ta}{tb}-{in_}-{out}-{name}",
                           Spec(M, N, K, out=out, in_=in_, seed=40 + 8 * si + n, **_lay(ta, tb), **F32_PADS, **F32_EPILOGUES[name]))


def f32_k_edge_cases():
    """K around the K-step of two and the 16-slab, on a tile ragged in M and N; and the degenerate extents."""
    for K in (1, 2, 3, 15, 16, 17, 31, 32, 33):
        for ta, tb in ((0, 0), (1, 0)):
            yield f"33x40x{K}-{ta}{tb}", Spec(33, 40, K, out="f32", in_="f32", seed=60 + K, pad_a=3, pad_b=7, pad_c=5, **_lay(ta, tb))
    for K in (1, 17):
        for i, (M, N) in enumerate(((1, 1), (1, 70), (70, 1))):
            ta, tb = LAYOUTS[(i + K) % 4]
            yield f"{M}x{N}x{K}-{ta}{tb}", Spec(M, N, K, out="f32", in_="f32", seed=70 + K + i, pad_a=3, pad_b=7, pad_c=5, **_lay(ta, tb))


def f32_big_cases():
    """(name, on the 128-tile kernel?, spec).  Each case is written for one side of launch_gemm_f32's dispatch line and
    uses_big_tiles() is asserted for it wherever it is used."""
    base = Spec(129, 130, 37, batch=64, out="f32", pad_a=3, pad_b=7, pad_c=5)
    variants = {
        "own_b": dict(gap_a=2, gap_b=6),
        "shared_b": dict(share_b=True, out="bf16", epi=BIAS | GELU, aux=True, pad_x=9),
        "gap_c": dict(gap_c=11, epi=RESIDUAL, pad_r=1),
    }
    for li, (ta, tb) in enumerate(LAYOUTS):
        for ii, in_ in enumerate(("f32", "bf16")):
            for vi, (name, kw) in enumerate(variants.items()):
                yield f"129x130x37b64-{ta}{tb}-{in_}-{name}", True, base.but(in_=in_, seed=80 + 6 * li + 3 * ii + vi, **_lay(ta, tb), **kw)
    for ta, tb in ((0, 0), (0, 1)):
        big = Spec(1930, 2050, 19, out="f32", in_="f32", pad_a=3, pad_b=7, pad_c=5, **_lay(ta, tb))
        yield f"1930x2050x19-{ta}{tb}-bias_residual", True, big.but(epi=BIAS | RESIDUAL, pad_r=1, seed=110 + tb)
        yield f"1930x2050x19-{ta}{tb}-accum", True, big.but(epi=ACCUM, seed=112 + tb)
    yield "128x128x16b256-00", True, Spec(128, 128, 16, batch=256, out="f32", in_="f32", seed=114)
    yield "128x128x16b256-11", True, Spec(128, 128, 16, batch=256, out="f32", in_="f32", seed=115, **_lay(1, 1))
    yield "129x130x37b63-00-neighbour", False, base.but(batch=63, in_="f32", seed=116, gap_a=2, gap_b=6)
    yield "129x130x37b63-01-neighbour", False, base.but(batch=63, in_="bf16", seed=117, gap_a=2, gap_b=6, **_lay(0, 1))


def splitk_spec(M: int, N: int, kc: int, splits: int, **kw) -> Spec:
    """ops.gemm_nt_f32_splitk's argument form: A [M][K_total] and B [N][K_total] contiguous, lda = ldb = K_total, item c = columns
    c kc .. (c + 1) kc of every row (strideA = strideB = kc), batch = splits."""
    kt = kc * splits
    return Spec(M, N, kc, batch=splits, out="f32", in_="f32", pad_a=kt - kc, pad_b=kt - kc, gap_a=kc - M * kt, gap_b=kc - N * kt, **kw)


def splitk_reference(A: np.ndarray, B: np.ndarray, splits: int, c_in: Optional[np.ndarray] = None):
    """(float64 A B^T (+ c_in), bound) of a product whose reduction is cut into `splits` equal chunks (A [M][K], B [N][K] float64,
    as ops.gemm_nt_f32_splitk and the split branch of ops.gemm run it): each chunk is an fma chain of kc = K / splits steps,
    gamma_kc T_c; the parts, each at most (1 + gamma_kc) T_c in magnitude, meet in dinox_colsum over `splits` rows, at most
    ceil(splits / 16) + 6 additions deep (tests/_colsum_emul.py), the last of them the addition to C.  One chunk: the chain, and two
    roundings for alpha and ACCUM."""
    K = A.shape[1]
    assert K % splits == 0
    kc = K // splits
    T = np.abs(A) @ np.abs(B).T
    c = np.zeros_like(T) if c_in is None else np.asarray(c_in, dtype=np.float64)
    gk = kc * U32 / (1.0 - kc * U32)
    d = math.ceil(splits / 16) + 6 if splits > 1 else 2
    gd = d * U32 / (1.0 - d * U32)
    return A @ B.T + c, gk * T + gd * ((1.0 + gk) * T + np.abs(c))


def f32_overlapped_stride_cases():
    yield "40x24-4x33", False, splitk_spec(40, 24, 33, 4, seed=120)
    yield "129x130-64x18", True, splitk_spec(129, 130, 18, 64, seed=121)


def f32_colsum_cases():
    """dinox_gemm with colsum on fp32 operands (A stored [K][M]: dinox_colsum over it), with and without ACCUM."""
    for ta, tb in ((1, 1), (1, 0)):
        for acc in (0, ACCUM):
            yield (f"76x20x44-{ta}{tb}-{'accum' if acc else 'overwrite'}",
                   Spec(76, 20, 44, out="f32", in_="f32", epi=acc, colsum=True, seed=130 + 2 * tb + (acc > 0), pad_a=3, pad_b=7, pad_c=5,
                        **_lay(ta, tb)))


def f32_cpu_families():
    """One representative of every gemm_f32 case family, at shapes the fma chain of the emulation finishes quickly."""
    lay = dict(f32_layout_cases())
    for n in ("77x24x44-00-f32-f32-plain", "77x24x44-00-bf16-bf16-bias", "77x24x44-01-f32-f32-gelu_aux", "77x24x44-10-f32-f32-dgelu",
              "77x24x44-11-f32-bf16-residual", "65x130x17-00-f32-bf16-gelu_auxgrad", "65x130x17-01-f32-f32-dgelu_auxgrad",
              "65x130x17-01-bf16-f32-residual", "65x130x17-10-f32-f32-accum_bias", "65x130x17-11-bf16-f32-gelu_aux"):
        yield "layout-" + n, lay[n]
    edge = dict(f32_k_edge_cases())
    for n in ("33x40x1-00", "33x40x3-10", "33x40x17-00", "33x40x33-10", "1x1x17-01", "70x1x1-11"):
        yield "kedge-" + n, edge[n]
    yield "big-own-b", Spec(129, 130, 37, batch=3, out="f32", in_="f32", pad_a=3, pad_b=7, pad_c=5, gap_a=2, gap_b=6, seed=140, **_lay(0, 1))
    yield "big-shared-b", Spec(129, 130, 37, batch=3, out="bf16", in_="bf16", epi=BIAS | GELU, aux=True, share_b=True, seed=141, **F32_PADS)
    yield "overlapped", splitk_spec(40, 24, 33, 4, seed=120)
    for n, s in f32_colsum_cases():
        yield "colsum-" + n, s
