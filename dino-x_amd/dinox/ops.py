"""Host-side wrappers of the C ABI: tensor -> pointer plumbing and autograd glue.

Every function here enqueues hand-written HIP kernels from libdinox_hip.so on torch's current
stream.  PyTorch is used for device memory (its caching allocator owns every buffer), streams and
the autograd graph only.  Tensors must live on a CUDA(HIP) device: CPU tensors raise -- the product
has no CPU fallback (the CPU restatement lives in oracle/ and is test infrastructure).

Numeric modes (see include/dinox.h): fp32 "parity" mode and bf16 "throughput" mode.  The mode is
taken from an explicit override (``compute_dtype(...)`` context manager) or, like the reference's
``--amp`` path (scripts/phase5_big_run.py:1716-1717), from the ambient ``torch.autocast`` state.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import operator
import os
import weakref
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import BF16, EPI_ACCUM, EPI_AUXGRAD, EPI_BIAS, EPI_DGELU, EPI_GELU, EPI_RESIDUAL, F32, BlockBwdArgs, BlockFwdArgs, BlockPlan, GemmArgs, check, lib

Tensor = torch.Tensor
_OVERRIDE: list = []


# ------------------------------------------------------------------------------------------
# mode / plumbing helpers
# ------------------------------------------------------------------------------------------
@contextlib.contextmanager
def compute_dtype(dtype: torch.dtype):
    """Force the numeric mode (torch.float32 or torch.bfloat16) regardless of autocast state."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("compute dtype must be torch.float32 or torch.bfloat16")
    _OVERRIDE.append(dtype)
    try:
        yield
    finally:
        _OVERRIDE.pop()


def current_dtype() -> torch.dtype:
    if _OVERRIDE:
        return _OVERRIDE[-1]
    if torch.is_autocast_enabled("cuda"):
        dt = torch.get_autocast_dtype("cuda")
        if dt != torch.bfloat16:
            raise RuntimeError(f"the HIP path supports bfloat16 autocast only (got {dt}); use --amp-dtype bfloat16")
        return torch.bfloat16
    return torch.float32


def _code(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return F32
    if dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {dtype}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _need_cuda(*ts: Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "dinox: tensors must be on a CUDA/HIP device -- the MI355X kernel library is the only compute "
                "path (no CPU fallback). Move the model and inputs to 'cuda'.")


def _c(t: Tensor) -> Tensor:
    return t if t.is_contiguous() else t.contiguous()


class GemmTimer:
    """Timing of dinox_gemm launches with HIP events recorded on the launch stream, INSIDE the library (dinox_gemm_timer_start / _stop:
    the launches that dinox_block_forward / _backward issue from C are seen too; bench.py runs one over its timed region to price the
    dominant kernel against its roofline).  Keyed by the kernel the dispatcher picks.  Every launch is COUNTED (launches, algorithmic
    flops and bytes); one launch in `every` is TIMED -- an event pair per launch costs the timed region 2.3 % at bs 256 (40.94 vs 40.00 ms:
    two marker packets around each of ~300 launches per step keep the next kernel from starting under the previous one's tail), which a
    1-in-16 sample brings to nothing measurable (40.02 ms).  The pick is a fixed multiplicative hash of the launch counter, so every
    position of the step is reached over a few steps; a family's time is the sum over its shapes of (mean timed duration of the shape)
    x (its launches).  One timer per process; not under graph capture."""

    def __init__(self, every: int = 16) -> None:
        self.every = max(1, int(every))
        self.text = ""

    def start(self) -> None:
        check(lib.dinox_gemm_timer_start(self.every), "dinox_gemm_timer_start")

    def stop(self) -> None:
        """Synchronises the recorded events and collects the per-shape records."""
        buf = C.create_string_buffer(1 << 20)
        n = lib.dinox_gemm_timer_stop(buf, len(buf))
        if n < 0:
            raise RuntimeError("dinox_gemm_timer_stop: record buffer too small")
        self.text += buf.value.decode()

    def __enter__(self):
        self.start()
        return self

    def __exit__(self, *exc):
        self.stop()
        return False

    @staticmethod
    def algorithmic_bytes(M, N, K, batch, epilogue, in_dtype, out_dtype, has_aux, shared_b) -> float:
        """HBM bytes one launch has to move if every operand and result crosses the memory interface exactly once:
        A (M x K) and B (N x K, once if shared by the batch) in the input dtype, C (M x N) in the output dtype, plus the
        epilogue's extra tensors -- the fp32 residual read, the GELU' side tensor written (GELU) or read (DGELU), C read back
        under ACCUM."""
        isz = 2 if in_dtype == BF16 else 4
        osz = 2 if out_dtype == BF16 else 4
        mn = float(M) * N * batch
        b = float(M) * K * batch * isz + float(N) * K * isz * (1 if shared_b else batch) + mn * osz
        if epilogue & EPI_RESIDUAL:
            b += mn * 4
        if has_aux and (epilogue & (EPI_GELU | EPI_DGELU)):
            b += mn * osz
        if epilogue & EPI_ACCUM:
            b += mn * 4
        return b

    def summary(self) -> dict:
        """{kernel: {"launches", "timed", "flops", "bytes", "ms"}} -- after stop().  "ms" is the family's time over ALL its launches,
        estimated from the timed ones (see the class docstring)."""
        out: dict = {}
        untimed = []
        for line in self.text.splitlines():
            f = line.split()
            if len(f) != 13:
                continue
            name = f[0]
            M, N, K, batch, epi, idt, odt, aux, shb, launches, timed = (int(v) for v in f[1:12])
            ms = float(f[12])
            fl = 2.0 * M * N * K * batch * launches
            by = self.algorithmic_bytes(M, N, K, batch, epi, idt, odt, aux, shb) * launches
            d = out.setdefault(name, {"launches": 0, "timed": 0, "flops": 0.0, "bytes": 0.0, "ms": 0.0, "_tb": 0.0, "_tms": 0.0})
            d["launches"] += launches
            d["flops"] += fl
            d["bytes"] += by
            if timed:
                d["timed"] += timed
                d["ms"] += ms / timed * launches
                d["_tb"] += by / launches * timed
                d["_tms"] += ms
            else:
                untimed.append((name, by))
        for name, by in untimed:          # a shape the sample never reached: the family's measured time per algorithmic byte
            d = out[name]
            if d["_tb"] > 0:
                d["ms"] += by * d["_tms"] / d["_tb"]
        for name in [k for k, d in out.items() if d["timed"] == 0]:
            del out[name]
        for d in out.values():
            del d["_tb"], d["_tms"]
        self.text = ""
        return out


TRACE_KERNELS: Optional[list] = None      # tests set this to a list to learn which GEMM kernel each call used


# ------------------------------------------------------------------------------------------
# raw ops (no autograd)
# ------------------------------------------------------------------------------------------
def gemm(A: Tensor, B: Tensor, *, transA=False, transB=False, out: Optional[Tensor] = None,
         out_dtype: Optional[torch.dtype] = None, bias: Optional[Tensor] = None, gelu=False, aux: Optional[Tensor] = None,
         dgelu=False, residual: Optional[Tensor] = None, accumulate=False, alpha: float = 1.0,
         colsum_out: Optional[Tensor] = None, auxgrad=False) -> Tensor:
    """C = epilogue(alpha * op(A) op(B)^T); A: [M,K] (or [K,M] if transA), B: [N,K] (or [K,N] if transB).
    3-D operands are batched over dim 0 (B may be 2-D = shared)."""
    _need_cuda(A, B)
    assert A.dtype == B.dtype, (A.dtype, B.dtype)
    A, B = _c(A), _c(B)
    batched = A.dim() == 3
    if batched:
        batch = A.shape[0]
        a2, b2 = A.shape[1:], (B.shape[1:] if B.dim() == 3 else B.shape)
    else:
        batch, a2, b2 = 1, A.shape, B.shape
    M, K = (a2[1], a2[0]) if transA else (a2[0], a2[1])
    N, Kb = (b2[1], b2[0]) if transB else (b2[0], b2[1])
    assert K == Kb, f"inner dims differ: {tuple(A.shape)} vs {tuple(B.shape)} (transA={transA}, transB={transB})"
    odt = out_dtype or (out.dtype if out is not None else A.dtype)
    if out is None:
        out = torch.empty((batch, M, N) if batched else (M, N), dtype=odt, device=A.device)
    else:
        assert out.is_contiguous() and out.dtype == odt and out.numel() == batch * M * N
    epi = 0
    if bias is not None:
        epi |= EPI_BIAS
        assert bias.dtype == torch.float32 and bias.numel() == N
    if gelu:
        epi |= EPI_GELU
    if dgelu:
        epi |= EPI_DGELU
        assert aux is not None
    if aux is not None:
        assert aux.dtype == odt and aux.is_contiguous() and aux.numel() == batch * M * N
    if residual is not None:
        epi |= EPI_RESIDUAL
        assert residual.dtype == torch.float32 and residual.is_contiguous() and residual.numel() == batch * M * N
    if accumulate:
        epi |= EPI_ACCUM
    if auxgrad:
        epi |= EPI_AUXGRAD
    if colsum_out is not None:
        assert transA and not batched and colsum_out.dtype == torch.float32 and colsum_out.numel() == M and colsum_out.is_contiguous()
    g = GemmArgs(
        A=_p(A), B=_p(B), C=_p(out), M=M, N=N, K=K, lda=a2[1], ldb=b2[1], ldc=N, batch=batch,
        strideA=a2[0] * a2[1] if batched else 0, strideB=(b2[0] * b2[1] if (batched and B.dim() == 3) else 0),
        strideC=M * N, transA=int(transA), transB=int(transB), in_dtype=_code(A.dtype), out_dtype=_code(odt),
        epilogue=epi, alpha=alpha, bias=_p(bias), residual=_p(residual), ldr=N, aux=_p(aux), ldaux=N, colsum=_p(colsum_out), ws=None)
    if (transA and transB and not batched and odt == torch.float32 and K >= 4096 and not (epi & ~EPI_ACCUM)
            and ((M + 127) // 128) * ((N + 127) // 128) < 256 and lib.dinox_gemm_kernel_name(C.byref(g)).decode().startswith("gemm_f32")):
        # dW products that land on the general exact-fp32 kernel -- the whole fp32 mode, and bf16 operands whose shape the MFMA bf16 kernels
        # do not take (patch 14: 3 x 14 x 14 = 588 columns) -- are a few dozen tiles with the whole token axis as reduction: 36-60 workgroups
        # on 256 CUs, 3-12 ms per launch.  Cut the reduction into chunks that run as ONE batched launch and meet in the fixed-order column sum.
        tiles = ((M + 127) // 128) * ((N + 127) // 128)
        splits = max(1, min(K // 1024, 1024 // tiles))
        while splits > 1 and K % splits:
            splits -= 1
        if splits > 1:
            kc = K // splits
            part = torch.empty((splits, M, N), dtype=torch.float32, device=A.device)
            g2 = GemmArgs(A=_p(A), B=_p(B), C=_p(part), M=M, N=N, K=kc, lda=a2[1], ldb=b2[1], ldc=N, batch=splits, strideA=kc * a2[1],
                          strideB=kc * b2[1], strideC=M * N, transA=1, transB=1, in_dtype=_code(A.dtype), out_dtype=F32, epilogue=0, alpha=alpha,
                          bias=None, residual=None, ldr=N, aux=None, ldaux=N, colsum=None, ws=None)
            if TRACE_KERNELS is not None:
                TRACE_KERNELS.append(lib.dinox_gemm_kernel_name(C.byref(g2)).decode())
            check(lib.dinox_gemm(C.byref(g2), _stream()), "dinox_gemm")
            colsum(part.view(splits, M * N), out=out.view(-1), accumulate=accumulate)
            if colsum_out is not None:                       # A is stored [K][M]: its column sums are the bias gradient
                check(lib.dinox_colsum(_p(A), _p(colsum_out), K, M, a2[1], _code(A.dtype), int(accumulate), _stream()), "dinox_colsum")
            return out
    if transA and transB and not batched and A.dtype == torch.bfloat16 and not _TN_ATOMICS:
        need = lib.dinox_gemm_ws_bytes(C.byref(g))       # split-K dW product: deterministic two-stage reduction through a workspace
        if need:
            g.ws = _p(_tn_workspace(need, A.device))
    if TRACE_KERNELS is not None:
        TRACE_KERNELS.append(lib.dinox_gemm_kernel_name(C.byref(g)).decode())
    check(lib.dinox_gemm(C.byref(g), _stream()), "dinox_gemm")
    return out


_TN_ATOMICS = bool(os.environ.get("DINOX_TN_ATOMICS"))      # A/B: split-K dW products through fp32 atomics (round-1 behaviour, not reproducible)
_TN_WS: dict = {}


def _tn_workspace(nbytes: int, device) -> Tensor:
    """One growable scratch buffer per (device, stream): consecutive split-K products of a stream reuse it in stream order."""
    key = (device, _stream())
    ws = _TN_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _TN_WS[key] = torch.empty(max(nbytes, 40 << 20), dtype=torch.uint8, device=device)
    return ws


def gemm_nt_f32_splitk(A: Tensor, B: Tensor, splits: int = 0) -> Tensor:
    """A [M,K] . B [N,K]^T in exact fp32 with the reduction cut into K-chunks that run as ONE batched launch (operand strides: chunk c
    starts K/splits elements further along every row) and meet in a fixed-order column sum.  For few-tile, long-K products: the KoLeo
    inner products are 512 x 512 x 8192 = 16 tiles, i.e. 16 workgroups on 256 CUs and 784 us as a plain product."""
    _need_cuda(A, B)
    assert A.dtype == torch.float32 and B.dtype == torch.float32 and A.is_contiguous() and B.is_contiguous() and A.dim() == 2 and B.dim() == 2
    M, K = A.shape
    N = B.shape[0]
    assert B.shape[1] == K
    if splits <= 0:
        tiles = ((M + 127) // 128) * ((N + 127) // 128)
        splits = max(1, min(K // 256, 256 // max(tiles, 1)))
    while splits > 1 and K % splits:
        splits -= 1
    if splits == 1:
        return gemm(A, B, out_dtype=torch.float32)
    kc = K // splits
    part = torch.empty((splits, M, N), dtype=torch.float32, device=A.device)
    g = GemmArgs(A=_p(A), B=_p(B), C=_p(part), M=M, N=N, K=kc, lda=K, ldb=K, ldc=N, batch=splits, strideA=kc, strideB=kc, strideC=M * N,
                 transA=0, transB=0, in_dtype=F32, out_dtype=F32, epilogue=0, alpha=1.0, bias=None, residual=None, ldr=N, aux=None, ldaux=N,
                 colsum=None, ws=None)
    if TRACE_KERNELS is not None:
        TRACE_KERNELS.append(lib.dinox_gemm_kernel_name(C.byref(g)).decode())
    check(lib.dinox_gemm(C.byref(g), _stream()), "dinox_gemm")
    return colsum(part.view(splits, M * N)).view(M, N)


def colsum(x: Tensor, out: Optional[Tensor] = None, accumulate=False) -> Tensor:
    x2 = _c(x).reshape(-1, x.shape[-1])
    if out is None:
        out = torch.empty(x2.shape[1], dtype=torch.float32, device=x.device)
    check(lib.dinox_colsum(_p(x2), _p(out), x2.shape[0], x2.shape[1], x2.shape[1], _code(x.dtype), int(accumulate), _stream()), "dinox_colsum")
    return out


def cast_bf16(x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    x = _c(x)
    if out is None:
        out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    else:
        assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.numel() == x.numel()
    check(lib.dinox_cast_bf16(_p(x), _p(out), x.numel(), _stream()), "dinox_cast_bf16")
    return out


def cast_transpose_bf16(w: Tensor) -> Tensor:
    w = _c(w)
    R, Cc = w.shape
    out = torch.empty((Cc, R), dtype=torch.bfloat16, device=w.device)
    check(lib.dinox_cast_transpose_bf16(_p(w), _p(out), R, Cc, _stream()), "dinox_cast_transpose_bf16")
    return out


def to_mode(x: Tensor, dt: torch.dtype) -> Tensor:
    """Bring an activation to the GEMM operand dtype of the current mode."""
    if x.dtype == dt:
        return _c(x)
    if dt == torch.bfloat16 and x.dtype == torch.float32:
        return cast_bf16(x)
    if dt == torch.float32 and x.dtype == torch.bfloat16:
        return x.float()
    raise TypeError(f"cannot bring {x.dtype} to {dt}")


class ArenaShadow:
    """bf16 image of a whole flat fp32 parameter arena, refreshed by ONE cast launch after an optimiser step, plus transposed
    images (one launch for all of them) of the matrices a backward pass has asked for.  Replaces ~150 per-weight cast launches
    per ViT-S step.  A parameter whose version moved since the refresh (load_state_dict, a manual copy_) is not served."""

    def __init__(self, flat: Tensor, params, offsets) -> None:
        self.flat, self.params, self.offsets = flat, list(params), list(offsets)
        self.index = {p.data_ptr(): i for i, p in enumerate(self.params) if p.numel()}
        self.plain: Optional[Tensor] = None
        self.trans: Optional[Tensor] = None
        self.versions: list = []
        self.wanted: dict = {}          # parameter index -> (R, C) of matrices needed transposed
        self.table: Optional[Tensor] = None
        self.table_for: tuple = ()
        self.tiles = 0
        self.served_t: set = set()

    def refresh(self) -> None:
        # (ONE persistent image, rewritten in place: the operand views handed out earlier stay valid, and a step captured into a
        # hipGraph reads at replay n + 1 what replay n wrote)
        self.plain = cast_bf16(self.flat, out=self.plain)
        self.versions = [p._version for p in self.params]
        self.served_t = set()
        if self.wanted:
            key = tuple(sorted(self.wanted))
            if key != self.table_for:
                rows, tiles = [], 0
                for i in key:
                    R, Cc = self.wanted[i]
                    rows.append([self.offsets[i], R, Cc, tiles])
                    tiles += ((R + 31) // 32) * ((Cc + 31) // 32)
                self.table = torch.tensor(rows, dtype=torch.int64, device=self.flat.device)
                self.table_for, self.tiles = key, tiles
            if self.trans is None:
                self.trans = torch.empty(self.flat.numel(), dtype=torch.bfloat16, device=self.flat.device)
            check(lib.dinox_cast_transpose_bf16_multi(_p(self.flat), _p(self.trans), _p(self.table), len(self.table_for), self.tiles,
                                                      _stream()), "dinox_cast_transpose_bf16_multi")
            self.served_t = set(self.table_for)

    def get(self, w: Tensor, transposed: bool) -> Optional[Tensor]:
        i = self.index.get(w.data_ptr())
        if i is None or self.params[i].shape != w.shape:
            return None
        R = w.shape[0]
        Cc = w.numel() // R
        if transposed:
            self.wanted.setdefault(i, (R, Cc))
        if self.plain is None or self.versions[i] != w._version:
            return None
        off = self.offsets[i]
        if not transposed:
            return self.plain[off:off + R * Cc].view(R, Cc)
        if i not in self.served_t:
            return None
        return self.trans[off:off + R * Cc].view(Cc, R)


class _WeightCache:
    """bf16 (and transposed bf16) copies of fp32 master weights.  Arena shadows registered by the training engine serve whole
    models from one cast launch; anything else is cast per weight and cached so the student forward, its backward and repeated
    teacher forwards of one step share one cast.

    An entry is valid only for the very tensor OBJECT it was made from (held by weak reference and compared with ``is``) at
    the version it had then: a freed model whose successor lands on the same addresses at version 0 (two ``load_model`` calls
    in a row) can therefore never be served the old model's weights.  Writers that go around torch's version counter (the
    ``dinox_adamw_ema`` kernel, any C-ABI caller writing through raw pointers) must call ``invalidate_weights()``."""

    def __init__(self) -> None:
        self.d: dict = {}
        self.extra: dict = {}          # other per-step images of a weight (the zero-padded patch-embedding operand), same lifetime
        self.shadows: list = []

    def clear(self) -> None:
        self.d.clear()
        self.extra.clear()

    def get(self, w: Tensor, transposed: bool) -> Tensor:
        for sh in self.shadows:
            hit = sh.get(w, transposed)
            if hit is not None:
                return hit
        key = (id(w), transposed)
        hit = self.d.get(key)
        if hit is not None and hit[0]() is w and hit[1] == (w.data_ptr(), w._version, tuple(w.shape)):
            return hit[2]
        if len(self.d) > 4096:
            self.d.clear()
        w2 = w.detach().reshape(w.shape[0], -1)
        val = cast_transpose_bf16(w2) if transposed else cast_bf16(w2)
        d = self.d
        self.d[key] = (weakref.ref(w, lambda _r, key=key, d=d: d.pop(key, None)), (w.data_ptr(), w._version, tuple(w.shape)), val)
        return val


weight_cache = _WeightCache()


def invalidate_weights(params=None) -> None:
    """Drop every cached bf16 weight image -- or, with ``params``, only the images of those tensors.  For callers that modify master
    weights through raw device pointers (the C ABI's ``dinox_adamw_ema``, a custom optimiser): torch's version counter does not see
    such writes."""
    if params is None:
        weight_cache.clear()
        return
    for p in params:
        weight_cache.d.pop((id(p), False), None)
        weight_cache.d.pop((id(p), True), None)


def weight_operand(w: Tensor, dt: torch.dtype, transposed=False) -> Tensor:
    """W as [N,K] (or W^T as [K,N] when transposed) in the GEMM operand dtype."""
    w2 = w.detach().reshape(w.shape[0], -1)
    if dt == torch.float32:
        return w2 if not transposed else w2  # fp32 kernels take either layout through the trans flags
    return weight_cache.get(w, transposed)


def dx_operand(w: Tensor, dt: torch.dtype):
    """W as the B operand of dX = dY . W  (dY [M,N], W [N,K]): returns (B, transB).  The fp32 kernels read W itself through the
    trans flag, the bf16 kernels take the cached W^T image."""
    if dt == torch.float32:
        return w.detach(), True
    return weight_operand(w, dt, transposed=True), False


def dx_product(dy: Tensor, w: Tensor, dt: torch.dtype, **epilogue_kw) -> Tensor:
    """dX = dY . W in compute mode dt; dgelu / aux / auxgrad / out_dtype go to gemm."""
    b, transB = dx_operand(w, dt)
    return gemm(dy, b, transB=transB, **epilogue_kw)


def layernorm_fwd(x: Tensor, w: Tensor, b: Tensor, out_dtype: torch.dtype, eps: float = 1e-5):
    _need_cuda(x, w, b)
    assert x.dtype == torch.float32
    x = _c(x)
    D = x.shape[-1]
    rows = x.numel() // D
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(lib.dinox_layernorm_fwd(_p(x), _p(w), _p(b), _p(y), _p(mean), _p(rstd), rows, D, eps, _code(out_dtype), _stream()), "dinox_layernorm_fwd")
    return y, mean, rstd


def linear_residual_ln(a: Tensor, w: Tensor, bias: Optional[Tensor], residual: Optional[Tensor], gamma: Tensor, beta: Tensor, eps: float,
                       y_dtype: torch.dtype):
    """x = residual + a W^T + bias (fp32) and y = LayerNorm(x) (y_dtype) with its row statistics, one launch.
    a [M,K] bf16, w [N,K] bf16.  Returns (x, y, mean, rstd)."""
    _need_cuda(a, w)
    assert a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and a.is_contiguous() and w.is_contiguous()
    M, K = a.shape
    N = w.shape[0]
    assert w.shape[1] == K and (residual is None or (residual.dtype == torch.float32 and residual.is_contiguous() and residual.numel() == M * N))
    dev = a.device
    x = torch.empty((M, N), dtype=torch.float32, device=dev)
    y = torch.empty((M, N), dtype=y_dtype, device=dev)
    mean = torch.empty(M, dtype=torch.float32, device=dev)
    rstd = torch.empty(M, dtype=torch.float32, device=dev)
    if TRACE_KERNELS is not None:
        TRACE_KERNELS.append("gemm_bf16_rowln")
    check(lib.dinox_linear_residual_ln(_p(a), _p(w), _p(bias), _p(residual), _p(x), _p(_c(gamma)), _p(_c(beta)), eps, _p(y), _code(y_dtype),
                                       _p(mean), _p(rstd), M, N, K, _stream()), "dinox_linear_residual_ln")
    return x, y, mean, rstd


def layernorm_bwd(dy: Tensor, x: Tensor, w: Tensor, mean: Tensor, rstd: Tensor, dx: Optional[Tensor] = None,
                  dx_add: Optional[Tensor] = None, want_lowp=False, b: Optional[Tensor] = None):
    """dx = (dx_add or 0) + LN'(dy); returns (dx, dw, db, bf16 copy of dx or None).  dx may alias dx_add.
    With the bias parameter ``b`` given and both affine parameters registered in the gradient sink, dw/db are added
    straight into the gradient arena and returned as None."""
    dy, x = _c(dy), _c(x)
    D = x.shape[-1]
    rows = x.numel() // D
    if dx is None:
        dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if dx_add is not None:
        assert dx_add.is_contiguous() and dx_add.dtype == torch.float32 and dx_add.numel() == x.numel()
    sw, sb = (grad_sink.lookup(w), grad_sink.lookup(b)) if b is not None else (None, None)
    sunk = sw is not None and sb is not None
    dw = sw[1].grad if sunk else torch.empty(D, dtype=torch.float32, device=x.device)
    db = sb[1].grad if sunk else torch.empty(D, dtype=torch.float32, device=x.device)
    lowp = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if want_lowp else None
    ws = torch.empty(lib.dinox_layernorm_bwd_ws_bytes(rows, D), dtype=torch.uint8, device=x.device)
    check(lib.dinox_layernorm_bwd(_p(dy), _p(x), _p(w), _p(mean), _p(rstd), _p(dx), _p(dx_add), _p(lowp), _p(dw), _p(db), _p(ws),
                                  rows, D, _code(dy.dtype), int(sunk), _stream()), "dinox_layernorm_bwd")
    if sunk:
        grad_sink.ready(sw)
        grad_sink.ready(sb)
        return dx, None, None, lowp
    return dx, dw, db, lowp


def linear_ln_bwd(a: Tensor, w_t: Tensor, x: Tensor, w: Tensor, mean: Tensor, rstd: Tensor, dx: Optional[Tensor] = None,
                  dx_add: Optional[Tensor] = None, want_lowp=False, b: Optional[Tensor] = None):
    """dy = a w_t^T (bf16), then layernorm_bwd(dy, x, w, mean, rstd, ...) in the same launch: returns (dx, dw, db, bf16 copy of dx or None)
    exactly as layernorm_bwd does.  a [M,K] bf16, w_t [D,K] bf16 (the W^T operand of the Linear in front of the LayerNorm)."""
    a, x = _c(a), _c(x)
    M, K = a.shape
    D = x.shape[-1]
    assert w_t.shape == (D, K) and w_t.is_contiguous() and x.numel() == M * D
    if dx is None:
        dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if dx_add is not None:
        assert dx_add.is_contiguous() and dx_add.dtype == torch.float32 and dx_add.numel() == x.numel()
    sw, sb = (grad_sink.lookup(w), grad_sink.lookup(b)) if b is not None else (None, None)
    sunk = sw is not None and sb is not None
    dw = sw[1].grad if sunk else torch.empty(D, dtype=torch.float32, device=x.device)
    db = sb[1].grad if sunk else torch.empty(D, dtype=torch.float32, device=x.device)
    lowp = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device) if want_lowp else None
    ws = torch.empty(lib.dinox_layernorm_bwd_ws_bytes(M, D), dtype=torch.uint8, device=x.device)
    if TRACE_KERNELS is not None:
        TRACE_KERNELS.append("gemm_bf16_nt_pp384(ln_bwd)")
    check(lib.dinox_linear_ln_bwd(_p(a), _p(w_t), _p(x), _p(w), _p(mean), _p(rstd), _p(dx), _p(dx_add), _p(lowp), _p(dw), _p(db), _p(ws),
                                  M, D, K, int(sunk), _stream()), "dinox_linear_ln_bwd")
    if sunk:
        grad_sink.ready(sw)
        grad_sink.ready(sb)
        return dx, None, None, lowp
    return dx, dw, db, lowp


_ATTN_F32_REF = bool(os.environ.get("DINOX_ATTN_F32_REF"))      # fp32 attention by the per-lane reference kernels whatever the size (A/B, tests)


def _gemm_f32_raw(a: int, b: int, c: int, M: int, N: int, K: int, lda: int, ldb: int, ldc: int, batch: int, sa: int, sb: int, sc: int,
                  ta: bool, tb: bool, alpha: float = 1.0) -> None:
    """One batched exact-fp32 product on raw addresses and element strides (operands are slices of packed tensors: no copies)."""
    g = GemmArgs(A=a, B=b, C=c, M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, batch=batch, strideA=sa, strideB=sb, strideC=sc,
                 transA=int(ta), transB=int(tb), in_dtype=F32, out_dtype=F32, epilogue=0, alpha=alpha, bias=None, residual=None, ldr=N,
                 aux=None, ldaux=N, colsum=None, ws=None)
    check(lib.dinox_gemm(C.byref(g), _stream()), "dinox_gemm")


def _use_f32_products(qkv: Tensor, N: int, d: int) -> bool:
    # full-size fp32 attention: batched exact-fp32 products + softmax rows (the per-lane reference kernels take 4.3 / 32 ms per layer
    # forward / backward at bs 64; this form 0.7 / 1.7 ms).  Small problems keep the reference kernels (fewer launches).
    return qkv.dtype == torch.float32 and not _ATTN_F32_REF and N >= 32 and qkv.shape[0] * N >= 4096


def _bf16_attention_needs_products(qkv: Tensor, N: int, d: int, fwd: bool) -> bool:
    """bf16 mode, a head size the MFMA attention kernels do not take (not a multiple of 8, or above 128), big enough to matter.  Since round 3
    every other shape runs on the device kernels: head size 64 up to 288 / 544 tokens on the whole-strip kernels (csrc/attention_bf16.hip),
    longer sequences and head sizes up to 128 -- ViT-g: 88 -- on the tiled ones (csrc/attention_flash.hip)."""
    if qkv.dtype != torch.bfloat16 or _ATTN_F32_REF or N < 32 or qkv.shape[0] * N < 4096:
        return False
    return d % 8 != 0 or d > 128


_PRODUCTS_BUDGET = 256 << 20      # bytes of fp32 scores per buffer of the product form (S, and dP in the backward)


def _product_chunks(B: int, N: int):
    """Batch ranges of the fp32 product form such that a [b, N, N] fp32 score buffer stays within _PRODUCTS_BUDGET (at bs 256
    and 785 tokens the un-chunked buffers were 1.26 GB each)."""
    per = max(1, _PRODUCTS_BUDGET // (4 * N * N))
    return [(b0, min(B, b0 + per)) for b0 in range(0, B, per)]


def _attention_fwd_f32_products(qkv: Tensor, heads: int, o: Tensor, lse: Tensor) -> None:
    """softmax(Q K^T / sqrt(d)) V per head as S = scale Q K^T (NT), softmax rows, O = P V -- operands addressed inside the packed qkv
    [B, N, 3, heads, d] and o [B, N, heads, d] by leading dimensions and batch strides; the batch is walked in chunks that keep the
    score buffer within _PRODUCTS_BUDGET."""
    B, N, C3 = qkv.shape
    Cc = C3 // 3
    d = Cc // heads
    scale = 1.0 / math.sqrt(d)
    chunks = _product_chunks(B, N)
    S = torch.empty((chunks[0][1] - chunks[0][0], N, N), dtype=torch.float32, device=qkv.device)
    E = 4
    for b0, b1 in chunks:
        nb = b1 - b0
        q0, o0 = qkv.data_ptr() + E * b0 * N * C3, o.data_ptr() + E * b0 * N * Cc
        for h in range(heads):
            qh, kh, vh = q0 + E * h * d, q0 + E * (Cc + h * d), q0 + E * (2 * Cc + h * d)
            _gemm_f32_raw(qh, kh, _p(S), N, N, d, C3, C3, N, nb, N * C3, N * C3, N * N, False, False, scale)          # S[b] = scale Q K^T
            check(lib.dinox_softmax_rows(_p(S), lse.data_ptr() + E * (b0 * heads + h) * N, nb * N, N, N, heads * N, _stream()), "dinox_softmax_rows")
            _gemm_f32_raw(_p(S), vh, o0 + E * h * d, N, d, N, N, C3, Cc, nb, N * N, N * C3, N * Cc, False, True)      # O[b] = P V


def _attention_bwd_f32_products(do: Tensor, qkv: Tensor, o: Tensor, lse: Tensor, heads: int, dqkv: Tensor) -> None:
    """Backward of the same: P = exp(S - lse) recomputed per head, dP = dO V^T, dS = P o (dP - rowsum(P o dP)) * scale, then
    dV = P^T dO, dQ = dS K, dK = dS^T Q written straight into the packed dqkv (batch chunks as in the forward)."""
    B, N, C3 = qkv.shape
    Cc = C3 // 3
    d = Cc // heads
    scale = 1.0 / math.sqrt(d)
    dev = qkv.device
    chunks = _product_chunks(B, N)
    nb0 = chunks[0][1] - chunks[0][0]
    S = torch.empty((nb0, N, N), dtype=torch.float32, device=dev)
    dP = torch.empty((nb0, N, N), dtype=torch.float32, device=dev)
    E = 4
    for b0, b1 in chunks:
        nb = b1 - b0
        q0, g0, do0 = qkv.data_ptr() + E * b0 * N * C3, dqkv.data_ptr() + E * b0 * N * C3, do.data_ptr() + E * b0 * N * Cc
        for h in range(heads):
            qh, kh, vh = q0 + E * h * d, q0 + E * (Cc + h * d), q0 + E * (2 * Cc + h * d)
            dqh, dkh, dvh = g0 + E * h * d, g0 + E * (Cc + h * d), g0 + E * (2 * Cc + h * d)
            doh = do0 + E * h * d
            _gemm_f32_raw(qh, kh, _p(S), N, N, d, C3, C3, N, nb, N * C3, N * C3, N * N, False, False, scale)          # S = scale Q K^T
            _gemm_f32_raw(doh, vh, _p(dP), N, N, d, Cc, C3, N, nb, N * Cc, N * C3, N * N, False, False)               # dP = dO V^T
            check(lib.dinox_softmax_bwd_rows(_p(S), _p(dP), lse.data_ptr() + E * (b0 * heads + h) * N, scale, nb * N, N, N, heads * N, _stream()),
                  "dinox_softmax_bwd_rows")                                                                              # S <- P, dP <- dS
            _gemm_f32_raw(_p(S), doh, dvh, N, d, N, N, Cc, C3, nb, N * N, N * Cc, N * C3, True, True)                  # dV = P^T dO
            _gemm_f32_raw(_p(dP), kh, dqh, N, d, N, N, C3, C3, nb, N * N, N * C3, N * C3, False, True)                 # dQ = dS K
            _gemm_f32_raw(_p(dP), qh, dkh, N, d, N, N, C3, C3, nb, N * N, N * C3, N * C3, True, True)                  # dK = dS^T Q


def attention_fwd(qkv: Tensor, heads: int):
    _need_cuda(qkv)
    qkv = _c(qkv)
    B, N, C3 = qkv.shape
    Cc = C3 // 3
    d = Cc // heads
    o = torch.empty((B, N, Cc), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, heads, N), dtype=torch.float32, device=qkv.device)
    if _use_f32_products(qkv, N, d):
        _attention_fwd_f32_products(qkv, heads, o, lse)
        return o, lse
    if _bf16_attention_needs_products(qkv, N, d, fwd=True):
        # head sizes / sequence lengths the MFMA attention kernels do not take (ViT-g: 88 per head; > 288 tokens): the exact-fp32 product
        # form on a float copy instead of the per-lane reference kernels (which are two orders of magnitude slower at these sizes)
        q32 = qkv.float()
        o32 = torch.empty((B, N, Cc), dtype=torch.float32, device=qkv.device)
        _attention_fwd_f32_products(q32, heads, o32, lse)
        return o32.to(qkv.dtype), lse
    check(lib.dinox_attention_fwd(_p(qkv), _p(o), _p(lse), B, N, heads, d, _code(qkv.dtype), _stream()), "dinox_attention_fwd")
    return o, lse


def qkv_attention_ok(B: int, N: int, heads: int, D: int, C: int) -> bool:
    """Is (B images of N tokens, width D in, heads x 64 out) inside the fused qkv-projection + attention kernel?"""
    return C % heads == 0 and bool(lib.dinox_qkv_attention_ok(B, N, heads, C // heads, D))


def qkv_attention(x: Tensor, w: Tensor, bias: Optional[Tensor], heads: int, want_qkv: bool = False, want_lse: bool = False):
    """o = attention(x w^T + bias) in ONE launch (dinox_qkv_attention_fwd): x [B,N,D] bf16, w [3C,D] bf16, bias [3C] fp32 or None
    -> o [B,N,C] bf16; with want_qkv / want_lse also the packed qkv rows [B,N,3C] / the log-sum-exp [B,heads,N] (else None).
    Replaces Attention.qkv + the attention core (zoo/arch.py:46-52) for passes that keep nothing for a backward."""
    _need_cuda(x, w)
    x, w = _c(x), _c(w)
    B, N, D = x.shape
    C = w.shape[0] // 3
    assert x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and w.shape == (3 * C, D) and C % heads == 0
    o = torch.empty((B, N, C), dtype=torch.bfloat16, device=x.device)
    qkv = torch.empty((B, N, 3 * C), dtype=torch.bfloat16, device=x.device) if want_qkv else None
    lse = torch.empty((B, heads, N), dtype=torch.float32, device=x.device) if want_lse else None
    if TRACE_KERNELS is not None:
        TRACE_KERNELS.append("attn_qkv_fused_fwd")
    check(lib.dinox_qkv_attention_fwd(_p(x), _p(w), _p(None if bias is None else _c(bias)), _p(o), _p(qkv), _p(lse), B, N, heads, C // heads, D,
                                      _stream()), "dinox_qkv_attention_fwd")
    return o, qkv, lse


def attention_bwd(do: Tensor, qkv: Tensor, o: Tensor, lse: Tensor, heads: int) -> Tensor:
    do = to_mode(do, qkv.dtype)
    B, N, C3 = qkv.shape
    d = C3 // 3 // heads
    dqkv = torch.empty_like(qkv)
    if _use_f32_products(qkv, N, d):
        _attention_bwd_f32_products(_c(do), _c(qkv), o, lse, heads, dqkv)
        return dqkv
    if _bf16_attention_needs_products(qkv, N, d, fwd=False):
        d32 = torch.empty(qkv.shape, dtype=torch.float32, device=qkv.device)
        _attention_bwd_f32_products(_c(do).float(), _c(qkv).float(), o, lse, heads, d32)
        return d32.to(qkv.dtype)
    ws = torch.empty(lib.dinox_attention_bwd_ws_bytes(B, N, heads), dtype=torch.uint8, device=qkv.device)
    check(lib.dinox_attention_bwd(_p(do), _p(qkv), _p(o), _p(lse), _p(dqkv), _p(ws), B, N, heads, d, _code(qkv.dtype), _stream()),
          "dinox_attention_bwd")
    return dqkv


# ------------------------------------------------------------------------------------------
# autograd functions
# ------------------------------------------------------------------------------------------
class LayerNormFn(torch.autograd.Function):
    """nn.LayerNorm over the fp32 residual stream (reference zoo/arch.py:89,91,187)."""

    @staticmethod
    def forward(ctx, x, w, b, out_dtype, eps):
        y, mean, rstd = layernorm_fwd(x, w, b, out_dtype, eps)
        ctx.save_for_backward(x, w, mean, rstd, b)
        ctx.mode_bf16 = current_dtype() == torch.bfloat16
        if ctx.needs_input_grad[1]:
            grad_sink.use(w, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, mean, rstd, b = ctx.saved_tensors
        dx, dw, db, lowp = layernorm_bwd(dy, x, w, mean, rstd, want_lowp=ctx.mode_bf16, b=b if ctx.needs_input_grad[1] else None)
        if lowp is not None:
            lowp_cache.put(dx, lowp)
        return dx, dw, db, None, None


class LayerNormPrecomputedFn(torch.autograd.Function):
    """The model's final LayerNorm when its forward was already produced by the last block's fused fc2 epilogue
    (linear_residual_ln): hands the precomputed output to autograd; backward is the ordinary LayerNorm backward."""

    @staticmethod
    def forward(ctx, x, w, b, y, mean, rstd):
        ctx.save_for_backward(x, w, mean, rstd, b)
        ctx.mode_bf16 = current_dtype() == torch.bfloat16
        if ctx.needs_input_grad[1]:
            grad_sink.use(w, b)
        return y.view_as(y)

    @staticmethod
    def backward(ctx, dy):
        x, w, mean, rstd, b = ctx.saved_tensors
        dx, dw, db, lowp = layernorm_bwd(dy, x.reshape(-1, x.shape[-1]), w, mean, rstd, want_lowp=ctx.mode_bf16,
                                         b=b if ctx.needs_input_grad[1] else None)
        dx = dx.view(x.shape)
        if lowp is not None:
            lowp_cache.put(dx, lowp.view(x.shape))
        return dx, dw, db, None, None, None


class _LowpCache:
    """bf16 copies of residual-stream gradients, handed from the kernel that produced the fp32 gradient
    (LayerNorm backward writes both) to the next backward node, which needs the bf16 form as a GEMM operand."""

    def __init__(self) -> None:
        self.key = None
        self.val = None

    def put(self, t: Tensor, lowp: Tensor) -> None:
        self.key, self.val = (t.data_ptr(), t._version, tuple(t.shape)), lowp

    def take(self, t: Tensor) -> Optional[Tensor]:
        if self.key == (t.data_ptr(), t._version, tuple(t.shape)):
            v, self.key, self.val = self.val, None, None
            return v
        return None


lowp_cache = _LowpCache()


def grad_operand(g: Tensor, dt: torch.dtype) -> Tensor:
    """A residual-stream gradient as a GEMM operand of the current mode (cached bf16 copy if one was emitted)."""
    if dt == torch.float32:
        return _c(g) if g.dtype == torch.float32 else g.float()
    if g.dtype == torch.bfloat16:
        return _c(g)
    hit = lowp_cache.take(g)
    return hit if hit is not None else cast_bf16(g)


class _GradSink:
    """Gradient arena registered by the training engine.  A weight gradient whose parameter is registered is accumulated by the
    dW product itself straight into the parameter's slice of the flat arena (the split-K atomics / ACCUM epilogue land there, the
    bias gradient rides along) and autograd gets ``None``: no zero-fill of a temporary, no temporary, no ``grad += dW`` pass per
    parameter (rocprof: ~150 fills and ~150 adds per ViT-S step).  ``on_ready(i)`` replaces the post-accumulate-grad hook that
    autograd no longer fires for such a parameter (dp.GradBucketer counts gradients with it); it fires when as many products
    have landed as forward passes used the parameter (``use``), so a module applied twice is still exchanged once, complete."""

    def __init__(self) -> None:
        self.slots: dict = {}
        self.uses: dict = {}
        self.on_ready = None
        self.owner = None
        self.recomputing = 0        # > 0 while torch.utils.checkpoint re-runs a forward to rebuild saved tensors

    def register(self, owner, params, on_ready=None) -> None:
        self.slots = {p.data_ptr(): (i, p) for i, p in enumerate(params) if p.requires_grad and p.numel()}
        self.uses, self.on_ready, self.owner = {}, on_ready, owner

    def clear(self) -> None:
        self.slots, self.uses, self.on_ready, self.owner = {}, {}, None, None

    def lookup(self, w: Optional[Tensor]):
        if w is None or not self.slots:
            return None
        slot = self.slots.get(w.data_ptr())
        if slot is None:
            return None
        g = slot[1].grad
        if g is None or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != w.shape:
            return None
        return slot

    def use(self, *ws) -> None:
        """Forward passes that will back-propagate into these parameters announce themselves (DP only)."""
        if self.on_ready is None or self.recomputing:      # a recomputed forward adds no backward product of its own
            return
        for w in ws:
            slot = self.lookup(w)
            if slot is not None:
                self.uses[slot[0]] = self.uses.get(slot[0], 0) + 1

    def ready(self, slot) -> None:
        if self.on_ready is None:
            return
        left = self.uses.get(slot[0], 1) - 1
        self.uses[slot[0]] = max(left, 0)
        if left <= 0:
            self.on_ready(slot[0])


grad_sink = _GradSink()


@contextlib.contextmanager
def _recompute_scope():
    grad_sink.recomputing += 1
    try:
        yield
    finally:
        grad_sink.recomputing -= 1


def checkpoint_contexts():
    """``context_fn`` for ``torch.utils.checkpoint.checkpoint(use_reentrant=False)``: (original forward, recomputation).
    The recomputation runs every forward of the block a second time only to rebuild its saved tensors; marking it keeps the
    gradient sink's use counts equal to the number of backward products, so data-parallel buckets still fire DURING backward."""
    return contextlib.nullcontext(), _recompute_scope()


def small_grad(param: Optional[Tensor], g: Optional[Tensor]) -> Optional[Tensor]:
    """A small parameter gradient (tokens, position embedding, scale-embedding MLP) produced by a kernel as a tensor of its own:
    with the parameter registered in the gradient sink it is added into the arena by dinox_axpy and autograd gets None (instead of
    one framework add kernel per parameter: nine per ViT-S step)."""
    if g is None or param is None:
        return g
    slot = grad_sink.lookup(param)
    if slot is None or g.dtype != torch.float32 or not g.is_contiguous():
        return g
    axpy_(slot[1].grad.view(-1), g.view(-1), 1.0)
    grad_sink.ready(slot)
    return None


class _DwStream:
    """The weight-gradient products have no consumer inside backward (their results are read by the optimiser, or by a gradient
    bucket's all-reduce): with DINOX_DW_STREAM=1 they are enqueued on a second HIP stream, so that a dW product (matrix pipe) can
    share the chip with the memory-bound kernels of the dX chain (LayerNorm backward, attention backward) instead of standing in
    line between them.  `join()` makes the current stream wait for everything enqueued there (engine: before the optimiser;
    dp.GradBucketer: before a bucket is exchanged)."""

    def __init__(self) -> None:
        self.enabled = bool(os.environ.get("DINOX_DW_STREAM"))
        self.streams: dict = {}
        self.dirty = False

    def side(self, device):
        st = self.streams.get(device)
        if st is None:
            st = self.streams[device] = torch.cuda.Stream(device=device)
        return st

    def run(self, fn, *tensors) -> None:
        main = torch.cuda.current_stream()
        side = self.side(tensors[0].device)
        side.wait_stream(main)                     # operands (and the zeroed arena) are products of the main stream
        with torch.cuda.stream(side):
            fn()
        for t in tensors:                          # their memory must outlive the side stream's use of it
            t.record_stream(side)
        self.dirty = True

    def join(self) -> None:
        if self.dirty:
            main = torch.cuda.current_stream()
            for st in self.streams.values():
                main.wait_stream(st)
            self.dirty = False


dw_stream = _DwStream()


def weight_grad(dy: Tensor, x: Tensor, w: Tensor, bias: Optional[Tensor], want_db: bool):
    """dW = dy^T x  ([N,M].[M,K]) and, if wanted, db = column sums of dy, from one product.
    Returns (dw, db) for autograd -- or (None, None) after accumulating both into the engine's gradient arena."""
    sw = grad_sink.lookup(w)
    sb = grad_sink.lookup(bias) if want_db else None
    if sw is not None and (not want_db or sb is not None):
        def product():
            gemm(dy, x, transA=True, transB=True, out=sw[1].grad.view(w.shape[0], -1), accumulate=True,
                 colsum_out=sb[1].grad if want_db else None)
        if dw_stream.enabled and dy.is_cuda:
            dw_stream.run(product, dy, x)
        else:
            product()
        grad_sink.ready(sw)
        if want_db:
            grad_sink.ready(sb)
        return None, None
    db = torch.empty(w.shape[0], dtype=torch.float32, device=dy.device) if want_db else None
    dw = gemm(dy, x, transA=True, transB=True, out_dtype=torch.float32, colsum_out=db)
    return dw.reshape(w.shape), db


def block_plan(V: int, N: int, D: int, H: int, heads: int, dt: torch.dtype, train: bool, next_dtype: Optional[torch.dtype] = None) -> BlockPlan:
    """Which launches of one transformer block (V views of N tokens, width D, hidden width H; compute mode dt; next_dtype = dtype of the
    LayerNorm that follows the block, None without one) run fused: .qkv_fused, .fuse_proj_ln, .fuse_fc2_ln, .fuse_ln_bwd.  The library
    decides (dinox_block_plan, csrc/block.hip: the measured rules and their DINOX_* switches, read at every call); both sequencers of
    BlockFn and both of its passes act on this one answer."""
    plan = BlockPlan()
    check(lib.dinox_block_plan(V, N, D, H, heads, _code(dt), int(train), -1 if next_dtype is None else _code(next_dtype), C.byref(plan)),
          "dinox_block_plan")
    return plan


_BLOCK_NATIVE = os.environ.get("DINOX_BLOCK_NATIVE", "1") != "0"      # "0": the block node issues its launches one by one from Python (A/B, tests)


def _block_native_ok(dt: torch.dtype, x0: Tensor, wqkv: Tensor) -> bool:
    """May this block run as ONE call into the library (dinox_block_forward / _backward, csrc/block.hip)?  bf16 throughput mode only (the
    fp32 parity mode composes full-size attention from several launches on the host), nobody listening to individual launches, and the
    weight-gradient side stream off (its products are enqueued from Python)."""
    return _BLOCK_NATIVE and dt == torch.bfloat16 and x0.is_cuda and TRACE_KERNELS is None and not dw_stream.enabled


def _block_forward_native(ctx, x0, n1w, n1b, wqkv, bqkv, wproj, bproj, n2w, n2b, w1, b1, w2, b2, heads, eps, pre_ln, next_ln, train, plan):
    """BlockFn.forward through dinox_block_forward: the same kernels in the same order, one foreign call."""
    dt = torch.bfloat16
    V, N, D = x0.shape
    M, H = V * N, w1.shape[0]
    dev = x0.device
    bf = lambda *shape: torch.empty(shape, dtype=torch.bfloat16, device=dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    if pre_ln is None:
        xn1, mean1, rstd1 = bf(V, N, D), f32(M), f32(M)
    else:
        xn1, mean1, rstd1 = pre_ln
    if plan.qkv_fused:      # no backward: projection + attention in one launch, no qkv tensor
        qkv, o, lse = None, bf(V, N, D), None
    else:
        qkv, o, lse = bf(M, 3 * D), bf(V, N, D), f32(V, heads, N)
    x1, xn2, mean2, rstd2 = f32(M, D), bf(M, D), f32(M), f32(M)
    act = bf(M, H)
    pre = bf(M, H) if train else None
    x2 = f32(V, N, D)
    nxt = None
    wops = [weight_operand(w_, dt) for w_ in (wqkv, wproj, w1, w2)]          # (held until the call is enqueued: a per-call cast would otherwise be freed)
    a = BlockFwdArgs(V=V, N=N, D=D, H=H, heads=heads, train=int(train), fuse_proj_ln=plan.fuse_proj_ln, fuse_fc2_ln=plan.fuse_fc2_ln, eps=eps,
                     x0=_p(x0), qkv=_p(qkv), o=_p(o), lse=_p(lse), x1=_p(x1), xn2=_p(xn2), mean2=_p(mean2), rstd2=_p(rstd2), act=_p(act), pre=_p(pre),
                     x2=_p(x2), n1w=_p(n1w), n1b=_p(n1b), n2w=_p(n2w), n2b=_p(n2b), wqkv=_p(wops[0]), wproj=_p(wops[1]), w1=_p(wops[2]), w2=_p(wops[3]),
                     bqkv=_p(bqkv), bproj=_p(bproj), b1=_p(b1), b2=_p(b2))
    if pre_ln is None:
        a.xn1, a.mean1, a.rstd1 = _p(xn1), _p(mean1), _p(rstd1)
    else:
        a.xn1_in, a.mean1_in, a.rstd1_in = _p(xn1), _p(mean1), _p(rstd1)
    if next_ln is not None:
        ydt = next_ln[3] or dt
        yn, mn, rn = torch.empty((V, N, D), dtype=ydt, device=dev), f32(M), f32(M)
        a.next_g, a.next_b, a.next_eps, a.next_dtype = _p(next_ln[0]), _p(next_ln[1]), next_ln[2], _code(ydt)
        a.yn, a.meann, a.rstdn = _p(yn), _p(mn), _p(rn)
        nxt = (yn, mn, rn)
    check(lib.dinox_block_forward(C.byref(a), _stream()), "dinox_block_forward")
    if train:
        ctx.save_for_backward(x0, x1, xn1, xn2, qkv, o, lse, pre, act, mean1, rstd1, mean2, rstd2, n1w, n2w, wqkv, wproj, w1, w2,
                              bqkv, bproj, b1, b2, n1b, n2b)
        ctx.dt, ctx.heads, ctx.shape, ctx.native, ctx.fuse_ln_bwd = dt, heads, (V, N, D), True, plan.fuse_ln_bwd
        grad_sink.use(wqkv, bqkv, wproj, bproj, w1, b1, w2, b2, n1w, n1b, n2w, n2b)
    if next_ln is None:
        return x2
    ctx.mark_non_differentiable(*nxt)
    return (x2,) + nxt


_BLOCK_TN_WS: dict = {}


def _block_tn_ws_bytes(M: int, D: int, H: int) -> int:
    """Workspace the four dW products of a block need for their deterministic split-K reduction (the largest of them), asked of the
    library once per shape (dinox_gemm_ws_bytes looks at shapes and pointer alignment only)."""
    key = (M, D, H)
    hit = _BLOCK_TN_WS.get(key)
    if hit is None:
        hit = 0
        for n_out, n_in in ((D, H), (H, D), (D, D), (3 * D, D)):
            g = GemmArgs(A=0x1000, B=0x1000, C=0x1000, M=n_out, N=n_in, K=M, lda=n_out, ldb=n_in, ldc=n_in, batch=1, strideA=0, strideB=0, strideC=n_out * n_in,
                         transA=1, transB=1, in_dtype=BF16, out_dtype=F32, epilogue=EPI_ACCUM, alpha=1.0, bias=None, residual=None, ldr=n_in, aux=None,
                         ldaux=n_in, colsum=0x1000, ws=0x1000)
            hit = max(hit, int(lib.dinox_gemm_ws_bytes(C.byref(g))))
        _BLOCK_TN_WS[key] = hit
    return hit


def _block_backward_native(ctx, g: Tensor, saved):
    """BlockFn.backward through dinox_block_backward -- when every parameter gradient of the block goes straight into the gradient arena
    (the training engine's registration); otherwise None and the composed path takes over.  `saved` = ctx.saved_tensors, unpacked by the
    caller (under torch.utils.checkpoint they may be unpacked only once)."""
    (x0, x1, xn1, xn2, qkv, o, lse, pre, act, mean1, rstd1, mean2, rstd2, n1w, n2w, wqkv, wproj, w1, w2, bqkv, bproj, b1, b2,
     n1b, n2b) = saved
    slots = [grad_sink.lookup(t) for t in (wqkv, bqkv, wproj, bproj, w1, b1, w2, b2, n1w, n1b, n2w, n2b)]
    have = [t is not None for t in (wqkv, bqkv, wproj, bproj, w1, b1, w2, b2, n1w, n1b, n2w, n2b)]
    if any(h and s is None for h, s in zip(have, slots)) or not all(have[i] for i in (0, 2, 4, 6, 8, 9, 10, 11)):
        return None
    dt, heads = torch.bfloat16, ctx.heads
    V, N, D = ctx.shape
    M, H = V * N, w1.shape[0]
    dev = g.device
    bf = lambda *shape: torch.empty(shape, dtype=torch.bfloat16, device=dev)
    g_lp = lowp_cache.take(g)
    g1 = torch.empty((V, N, D), dtype=torch.float32, device=dev)
    g0_lp = bf(V, N, D)
    gp = lambda sl: None if sl is None else sl[1].grad.data_ptr()
    tn_ws = _tn_workspace(max(_block_tn_ws_bytes(M, D, H), 1), dev)
    # scratch of the call: every tensor is HELD until the call has been enqueued (a temporary freed inside the argument list would hand
    # its memory to the next allocation of the same list: dpre, dxn2, ... would alias)
    scratch = dict(dpre=bf(M, H), dxn2=bf(M, D), d_o=bf(M, D), dqkv=bf(M, 3 * D), dxn1=bf(M, D), g1_lowp=bf(M, D),
                   g_lowp_buf=None if g_lp is not None else bf(M, D),
                   attn_ws=torch.empty(lib.dinox_attention_bwd_ws_bytes(V, N, heads), dtype=torch.uint8, device=dev),
                   ln_ws=torch.empty(lib.dinox_layernorm_bwd_ws_bytes(M, D), dtype=torch.uint8, device=dev))
    wts = [weight_operand(w_, dt, transposed=True) for w_ in (wqkv, wproj, w1, w2)]
    a = BlockBwdArgs(V=V, N=N, D=D, H=H, heads=heads, fuse_ln_bwd=ctx.fuse_ln_bwd, g=_p(g), g_lowp=_p(g_lp), g_lowp_buf=_p(scratch["g_lowp_buf"]),
                     x0=_p(x0), x1=_p(x1), xn1=_p(xn1), xn2=_p(xn2), qkv=_p(qkv), o=_p(o), lse=_p(lse), pre=_p(pre), act=_p(act), mean1=_p(mean1),
                     rstd1=_p(rstd1), mean2=_p(mean2), rstd2=_p(rstd2), n1w=_p(n1w), n2w=_p(n2w),
                     wqkv_t=_p(wts[0]), wproj_t=_p(wts[1]), w1_t=_p(wts[2]), w2_t=_p(wts[3]),
                     dwqkv=gp(slots[0]), dbqkv=gp(slots[1]), dwproj=gp(slots[2]), dbproj=gp(slots[3]), dw1=gp(slots[4]), db1=gp(slots[5]),
                     dw2=gp(slots[6]), db2=gp(slots[7]), dn1w=gp(slots[8]), dn1b=gp(slots[9]), dn2w=gp(slots[10]), dn2b=gp(slots[11]),
                     dpre=_p(scratch["dpre"]), dxn2=_p(scratch["dxn2"]), d_o=_p(scratch["d_o"]), dqkv=_p(scratch["dqkv"]), dxn1=_p(scratch["dxn1"]),
                     g1=_p(g1), g1_lowp=_p(scratch["g1_lowp"]), g0_lowp=_p(g0_lp), attn_ws=_p(scratch["attn_ws"]), ln_ws=_p(scratch["ln_ws"]),
                     tn_ws=_p(tn_ws), tn_ws_bytes=tn_ws.numel())
    check(lib.dinox_block_backward(C.byref(a), _stream()), "dinox_block_backward")
    for sl in slots:
        if sl is not None:
            grad_sink.ready(sl)
    lowp_cache.put(g1, g0_lp)
    return (g1,) + (None,) * 16


_outer_grad_mode = [True]


def block_fn(*args):
    """BlockFn.apply that also tells the node whether the caller runs with gradients enabled (a no-grad pass saves nothing: no GELU' side
    tensor, and where block_plan says qkv_fused no packed qkv tensor either)."""
    prev = _outer_grad_mode[0]
    _outer_grad_mode[0] = torch.is_grad_enabled()
    try:
        return BlockFn.apply(*args)
    finally:
        _outer_grad_mode[0] = prev


class BlockFn(torch.autograd.Function):
    """One pre-norm transformer block as a single autograd node (reference zoo/arch.py:94-97 with
    Attention :43-54 and Mlp :75-76 inlined):  x1 = x0 + proj(attn(norm1(x0)));  x2 = x1 + fc2(gelu(fc1(norm2(x1)))).

    13 kernel launches forward, 15 backward, no torch elementwise kernels: residual adds live in GEMM
    epilogues, the skip-connection gradient add and the bf16 cast of the residual gradient live in the
    LayerNorm backward kernel, bias gradients ride along the dW products."""

    @staticmethod
    def forward(ctx, x0, n1w, n1b, wqkv, bqkv, wproj, bproj, n2w, n2b, w1, b1, w2, b2, heads, eps, pre_ln=None, next_ln=None):
        """``pre_ln`` = (norm1(x0), mean, rstd) when the producer of x0 already normalised it (the previous block's fc2 epilogue);
        ``next_ln`` = (gamma, beta, eps, out_dtype) of the LayerNorm that FOLLOWS this block (the next block's norm1, or the model's
        final norm): then the block also returns (LN(x2), mean, rstd) -- in bf16 mode at width 384 straight from the fc2 product's
        epilogue (linear_residual_ln), as the proj product's epilogue produces norm2(x1); otherwise from LayerNorm launches.
        Returns x2, or (x2, y_next, mean_next, rstd_next) with ``next_ln``."""
        _need_cuda(x0, wqkv)
        ctx.set_materialize_grads(False)      # the non-differentiable outputs (LN of the next block) would otherwise arrive as zero-FILLED tensors
        dt = current_dtype()
        x0 = _c(x0 if x0.dtype == torch.float32 else x0.float())
        V, N, D = x0.shape
        M = V * N
        # needs_input_grad says which inputs COULD take a gradient; under torch.no_grad() (encode(), an evaluation loop over a model whose
        # parameters still require grad) nothing will ever ask for one: block_fn() notes the caller's grad mode (inside forward it is always off)
        train = any(ctx.needs_input_grad) and _outer_grad_mode[0]
        plan = block_plan(V, N, D, w1.shape[0], heads, dt, train, None if next_ln is None else next_ln[3] or dt)
        if _block_native_ok(dt, x0, wqkv):
            return _block_forward_native(ctx, x0, n1w, n1b, wqkv, bqkv, wproj, bproj, n2w, n2b, w1, b1, w2, b2, heads, eps, pre_ln, next_ln, train, plan)
        ctx.native = False
        if pre_ln is None:
            xn1, mean1, rstd1 = layernorm_fwd(x0, n1w, n1b, dt, eps)
        else:
            xn1, mean1, rstd1 = pre_ln
        if plan.qkv_fused:
            o, qkv, lse = qkv_attention(xn1.view(V, N, D), weight_operand(wqkv, dt), bqkv, heads)      # one launch, no qkv tensor
        else:
            qkv = gemm(xn1.view(M, D), weight_operand(wqkv, dt), bias=bqkv, out_dtype=dt)
            o, lse = attention_fwd(qkv.view(V, N, 3 * D), heads)
        if plan.fuse_proj_ln:
            x1, xn2, mean2, rstd2 = linear_residual_ln(o.view(M, D), weight_operand(wproj, dt), bproj, x0.view(M, D), n2w, n2b, eps, dt)
        else:
            x1 = gemm(o.view(M, D), weight_operand(wproj, dt), bias=bproj, residual=x0.view(M, D), out_dtype=torch.float32)
            xn2, mean2, rstd2 = layernorm_fwd(x1, n2w, n2b, dt, eps)
        nxt = None
        # (A fused fc1 -> GELU -> fc2 kernel for passes that save nothing -- hidden activation on chip, -632 MB per block -- was built in
        #  round 1 and removed in round 2: 509 us against 197 + 197 us for the two products at the hot-path shape)
        if True:
            H = w1.shape[0]
            pre = torch.empty((M, H), dtype=dt, device=x0.device) if train else None
            act = gemm(xn2, weight_operand(w1, dt), bias=b1, gelu=True, aux=pre, auxgrad=True, out_dtype=dt)   # pre := gelu'(fc1 out)
            if plan.fuse_fc2_ln:
                x2, yn, mn, rn = linear_residual_ln(act, weight_operand(w2, dt), b2, x1, next_ln[0], next_ln[1], next_ln[2], next_ln[3] or dt)
                nxt = (yn.view(V, N, D), mn, rn)
            else:
                x2 = gemm(act, weight_operand(w2, dt), bias=b2, residual=x1, out_dtype=torch.float32)
            if train:
                ctx.save_for_backward(x0, x1, xn1, xn2, qkv, o, lse, pre, act, mean1, rstd1, mean2, rstd2, n1w, n2w, wqkv, wproj, w1, w2,
                                      bqkv, bproj, b1, b2, n1b, n2b)
                ctx.dt, ctx.heads, ctx.shape, ctx.fuse_ln_bwd = dt, heads, (V, N, D), plan.fuse_ln_bwd
                grad_sink.use(wqkv, bqkv, wproj, bproj, w1, b1, w2, b2, n1w, n1b, n2w, n2b)
        x2 = x2.view(V, N, D)
        if next_ln is None:
            return x2
        if nxt is None:
            yn, mn, rn = layernorm_fwd(x2, next_ln[0], next_ln[1], next_ln[3] or dt, next_ln[2])
            nxt = (yn, mn, rn)
        ctx.mark_non_differentiable(*nxt)
        return (x2,) + nxt

    @staticmethod
    def backward(ctx, g, *_unused):
        (x0, x1, xn1, xn2, qkv, o, lse, pre, act, mean1, rstd1, mean2, rstd2, n1w, n2w, wqkv, wproj, w1, w2, bqkv, bproj, b1, b2,
         n1b, n2b) = ctx.saved_tensors
        dt, heads = ctx.dt, ctx.heads
        V, N, D = ctx.shape
        M = V * N
        dev = g.device
        g = _c(g if g.dtype == torch.float32 else g.float())
        bf = dt == torch.bfloat16
        if ctx.native:
            native = _block_backward_native(ctx, g, (x0, x1, xn1, xn2, qkv, o, lse, pre, act, mean1, rstd1, mean2, rstd2, n1w, n2w, wqkv, wproj, w1, w2,
                                                     bqkv, bproj, b1, b2, n1b, n2b))
            if native is not None:
                return native

        g_op = grad_operand(g, dt).view(M, D)
        # ---- MLP: x2 = x1 + fc2(gelu(fc1(xn2)))
        dpre = dx_product(g_op, w2, dt, dgelu=True, aux=pre, auxgrad=True, out_dtype=dt)
        dw2, db2 = weight_grad(g_op, act, w2, b2, b2 is not None)
        fuse_ln = ctx.fuse_ln_bwd
        if fuse_ln:
            w1t, _ = dx_operand(w1, dt)
        else:
            dxn2 = dx_product(dpre, w1, dt, out_dtype=dt)
        dw1, db1 = weight_grad(dpre, xn2.view(M, D), w1, b1, b1 is not None)
        if fuse_ln:     # g1 = g + LN2'(dpre W1): product and LayerNorm backward in one launch
            g1, dn2w, dn2b, g1_lp = linear_ln_bwd(dpre, w1t, x1, n2w, mean2, rstd2, dx_add=g.view(M, D), want_lowp=True, b=n2b)
        else:
            g1, dn2w, dn2b, g1_lp = layernorm_bwd(dxn2, x1, n2w, mean2, rstd2, dx_add=g.view(M, D), want_lowp=bf, b=n2b)   # g1 = g + LN2'(.)
        del dpre
        g1_op = g1_lp if bf else g1
        # ---- attention: x1 = x0 + proj(attn(qkv(xn1)))
        do = dx_product(g1_op, wproj, dt, out_dtype=dt)
        dwp, dbp = weight_grad(g1_op, o.view(M, D), wproj, bproj, bproj is not None)
        dqkv = attention_bwd(do.view(V, N, D), qkv.view(V, N, 3 * D), o, lse, heads).view(M, 3 * D)
        if fuse_ln:
            wqkvt, _ = dx_operand(wqkv, dt)
        else:
            dxn1 = dx_product(dqkv, wqkv, dt, out_dtype=dt)
        dwq, dbq = weight_grad(dqkv, xn1.view(M, D), wqkv, bqkv, bqkv is not None)
        if not bf:
            dw_stream.join()        # fp32 mode: the proj dW product reads g1 itself (bf16 mode: its own low-precision copy)
        if fuse_ln:
            g0, dn1w, dn1b, g0_lp = linear_ln_bwd(dqkv, wqkvt, x0, n1w, mean1, rstd1, dx=g1, dx_add=g1, want_lowp=True, b=n1b)   # in place on our own g1
        else:
            g0, dn1w, dn1b, g0_lp = layernorm_bwd(dxn1, x0, n1w, mean1, rstd1, dx=g1, dx_add=g1, want_lowp=bf, b=n1b)      # in place on our own g1
        g0 = g0.view(V, N, D)
        if g0_lp is not None:
            lowp_cache.put(g0, g0_lp.view(V, N, D))
        return g0, dn1w, dn1b, dwq, dbq, dwp, dbp, dn2w, dn2b, dw1, db1, dw2, db2, None, None, None, None


class LinearFn(torch.autograd.Function):
    """y = x W^T + b (+ residual), nn.Linear semantics (reference zoo/arch.py:40-41,46,53)."""

    @staticmethod
    def forward(ctx, x, w, b, residual, out_dtype):
        _need_cuda(x, w)
        dt = current_dtype()
        xm = to_mode(x, dt)
        K = xm.shape[-1]
        x2 = xm.reshape(-1, K)
        odt = torch.float32 if residual is not None else (out_dtype or dt)
        y = gemm(x2, weight_operand(w, dt), bias=b, residual=None if residual is None else _c(residual).reshape(-1, w.shape[0]),
                 out_dtype=odt)
        ctx.save_for_backward(x2, w, b)
        if ctx.needs_input_grad[1]:
            grad_sink.use(w, b if ctx.needs_input_grad[2] else None)
        ctx.dt, ctx.has_bias, ctx.has_res, ctx.xshape, ctx.xdtype = dt, b is not None, residual is not None, x.shape, x.dtype
        return y.reshape(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w, b = ctx.saved_tensors
        dt = ctx.dt
        dy2 = to_mode(dy.reshape(-1, w.shape[0]), dt)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = dx_product(dy2, w, dt, out_dtype=dt if dt == torch.bfloat16 else ctx.xdtype)       # dy [M,N] . W [N,K]
            if dx.dtype != ctx.xdtype:
                dx = dx.to(ctx.xdtype)
            dx = dx.reshape(ctx.xshape)
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            dw, db = weight_grad(dy2, x2, w, b, want_db)                                            # dy^T [N,M] . x [M,K] (+ db)
        elif want_db:
            db = colsum(dy2)
        dres = dy if ctx.has_res else None
        return dx, dw, db, dres, None


# ------------------------------------------------------------------------------------------
# LoRA: the low-rank side of a wrapped linear layer (csrc/lora.hip)
# ------------------------------------------------------------------------------------------
def _lora_small(t: Tensor, what: str) -> Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32 (the adapter matrices are never rounded), got {t.dtype}")
    return _c(t.detach())


def lora_down(x: Tensor, small: Tensor, layout: int = 0) -> Tensor:
    """u [M,r] fp32 = x [M,K] . S: layout 0 takes S = A stored [r,K] (u = xl A^T), layout 1 takes S = B stored [K,r] (v = dy B)."""
    _need_cuda(x, small)
    x, small = _c(x), _lora_small(small, "lora_down: the small matrix")
    M, K = x.shape
    r = small.shape[1] if layout else small.shape[0]
    assert small.shape == ((K, r) if layout else (r, K)), (tuple(x.shape), tuple(small.shape), layout)
    u = torch.empty((M, r), dtype=torch.float32, device=x.device)
    check(lib.dinox_lora_down(_p(x), _p(small), _p(u), M, K, r, int(layout), _code(x.dtype), _stream()), "dinox_lora_down")
    return u


def lora_up(u: Tensor, small: Tensor, s: float, res: Optional[Tensor] = None, layout: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """t [M,N] fp32 = s u [M,r] . S (+ res): layout 0 takes S = B stored [N,r], layout 1 takes S = A stored [r,N]."""
    _need_cuda(u, small)
    u, small = _lora_small(u, "lora_up: u"), _lora_small(small, "lora_up: the small matrix")
    M, r = u.shape
    N = small.shape[1] if layout else small.shape[0]
    assert small.shape == ((r, N) if layout else (N, r)), (tuple(u.shape), tuple(small.shape), layout)
    if res is not None:
        assert res.dtype == torch.float32 and res.is_contiguous() and res.numel() == M * N
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=u.device)
    else:
        assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == M * N
    check(lib.dinox_lora_up(_p(u), _p(small), _p(res), _p(out), float(s), M, N, r, int(layout), _stream()), "dinox_lora_up")
    return out


def lora_grad(xl: Tensor, dy: Tensor, A: Tensor, B: Tensor, s: float):
    """(dA [r,K], dB [N,r]) = (s v^T xl, s dy^T u) with u = xl A^T and v = dy B formed on chip: xl and dy are read once."""
    _need_cuda(xl, dy, A, B)
    assert xl.dtype == dy.dtype and xl.dim() == 2 and dy.dim() == 2 and xl.shape[0] == dy.shape[0]
    xl, dy, A, B = _c(xl), _c(dy), _lora_small(A, "lora_grad: A"), _lora_small(B, "lora_grad: B")
    M, K = xl.shape
    N, r = B.shape
    assert A.shape == (r, K) and dy.shape[1] == N
    need = lib.dinox_lora_grad_ws_bytes(M, K, N, r)
    if need <= 0:
        raise ValueError(f"lora_grad: M={M} K={K} N={N} r={r} outside the kernel's range (1 <= r <= 64)")
    ws = torch.empty(need // 4, dtype=torch.float32, device=xl.device)
    dA, dB = torch.empty_like(A), torch.empty_like(B)
    check(lib.dinox_lora_grad(_p(xl), _p(dy), _p(A), _p(B), float(s), _p(dA), _p(dB), _p(ws), M, K, N, r, _code(xl.dtype), _stream()),
          "dinox_lora_grad")
    return dA, dB


def lora_dropout(x: Tensor, p: float, seed: int, offset: int, out: Optional[Tensor] = None) -> Tensor:
    """x keep / (1 - p) with keep recomputed from (seed, offset, flat element index): no mask is stored (include/dinox.h has the hash)."""
    _need_cuda(x)
    x = _c(x)
    if out is None:
        out = torch.empty_like(x)
    else:
        assert out.dtype == x.dtype and out.is_contiguous() and out.numel() == x.numel()
    check(lib.dinox_lora_dropout(_p(x), _p(out), x.numel(), float(p), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), _code(x.dtype),
                                 _stream()), "dinox_lora_dropout")
    return out


def lora_merge(w: Tensor, A: Tensor, B: Tensor, s: float, sign: int = 1, out: Optional[Tensor] = None) -> Tensor:
    """W + sign s B A in fp32 (sign -1 takes a merged adapter out again); out may be w itself."""
    _need_cuda(w, A, B)
    assert w.dtype == torch.float32 and w.is_contiguous() and w.dim() == 2
    A, B = _lora_small(A, "lora_merge: A"), _lora_small(B, "lora_merge: B")
    N, K = w.shape
    r = A.shape[0]
    assert A.shape == (r, K) and B.shape == (N, r)
    if out is None:
        out = torch.empty_like(w)
    else:
        assert out.dtype == torch.float32 and out.is_contiguous() and out.shape == w.shape
    check(lib.dinox_lora_merge(_p(w), _p(A), _p(B), _p(out), float(s), int(sign), N, K, r, _stream()), "dinox_lora_merge")
    return out


class LoraLinearFn(torch.autograd.Function):
    """y = x W^T + b + s (xl A^T) B^T (+ residual); xl = dropout(x) when p > 0, else x.  The base product is LinearFn's dinox_gemm call;
    the low-rank term (plus the residual) reaches it as its fp32 RESIDUAL input, so it meets the base product in fp32 and the sum is
    rounded once -- it is never folded into a bf16 image of W.  A, B, u and v are fp32 in both modes.  With A None: LinearFn.
    Saved for backward: xl only if A or B needs a gradient, x2 only if the base weight does (so a frozen base with dropout keeps one
    activation, not two), and the dropout integers; u is not saved -- dinox_lora_grad forms u and v of a row chunk on chip."""

    @staticmethod
    def forward(ctx, x, w, b, A, B, s, p, seed, offset, residual, out_dtype):
        _need_cuda(x, w, A, B)
        dt = current_dtype()
        xm = to_mode(x, dt)
        K, N = xm.shape[-1], w.shape[0]
        x2 = xm.reshape(-1, K)
        drop = p > 0.0
        xl = lora_dropout(x2, p, seed, offset) if drop else x2
        res2 = None if residual is None else _c(residual).reshape(-1, N)
        t = lora_up(lora_down(xl, A, 0), B, s, res=res2, layout=0)
        odt = torch.float32 if residual is not None else (out_dtype or dt)
        y = gemm(x2, weight_operand(w, dt), bias=b, residual=t, out_dtype=odt)
        ctx.save_for_backward(x2 if ctx.needs_input_grad[1] else None, xl if (ctx.needs_input_grad[3] or ctx.needs_input_grad[4]) else None,
                              w, b, A, B)
        if ctx.needs_input_grad[1]:
            grad_sink.use(w, b if ctx.needs_input_grad[2] else None)
        ctx.dt, ctx.has_bias, ctx.has_res, ctx.xshape, ctx.xdtype = dt, b is not None, residual is not None, x.shape, x.dtype
        ctx.s, ctx.drop = float(s), ((float(p), int(seed), int(offset)) if drop else None)
        return y.reshape(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, xl, w, b, A, B = ctx.saved_tensors
        dt, s = ctx.dt, ctx.s
        dy2 = to_mode(dy.reshape(-1, w.shape[0]), dt)
        dx = dw = db = dA = dB = None
        if ctx.needs_input_grad[0]:
            t = lora_up(lora_down(dy2, B, 1), A, s, layout=1)                                    # s (dy B) A, fp32 [M,K]
            if ctx.drop is not None:
                lora_dropout(t, *ctx.drop, out=t)                                               # the forward's mask, recomputed
            dx = dx_product(dy2, w, dt, residual=t, out_dtype=dt if dt == torch.bfloat16 else ctx.xdtype)
            if dx.dtype != ctx.xdtype:
                dx = dx.to(ctx.xdtype)
            dx = dx.reshape(ctx.xshape)
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1]:
            dw, db = weight_grad(dy2, x2, w, b, want_db)
        elif want_db:
            db = colsum(dy2)
        if ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            dA, dB = lora_grad(xl, dy2, A, B, s)
        dres = dy if ctx.has_res else None
        return dx, dw, db, dA, dB, None, None, None, None, dres, None


def lora_linear(x: Tensor, w: Tensor, b: Optional[Tensor], A: Optional[Tensor], B: Optional[Tensor], s: float, p: float, seed_offset,
                residual: Optional[Tensor] = None, out_dtype: Optional[torch.dtype] = None) -> Tensor:
    """A LoRA-wrapped linear layer.  ``p`` is the dropout probability that applies to THIS call (0 in eval mode); ``seed_offset`` is the
    (seed, offset) pair the dropout mask is recomputed from.  ``A is None`` is the plain layer, bit for bit ``LinearFn``."""
    if A is None:
        return LinearFn.apply(x, w, b, residual, out_dtype)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"lora_linear: dropout probability {p} outside [0, 1)")
    seed, offset = seed_offset if seed_offset is not None else (0, 0)
    return LoraLinearFn.apply(x, w, b, A, B, float(s), float(p), int(seed), int(offset), residual, out_dtype)


def mlp_forward(x2: Tensor, w1: Tensor, b1: Optional[Tensor], w2: Tensor, b2: Optional[Tensor], residual: Optional[Tensor],
                out_dtype: Optional[torch.dtype], dt: torch.dtype, train: bool):
    """fc2(GELU_erf(fc1(x2))) (+ residual) on rows x2 [M,K] that are already operands of mode dt, without autograd: two products, GELU
    (and, with ``train``, GELU' for the backward as a side tensor) in the first one's epilogue.  Returns (y [M,N], saved for mlp_backward)."""
    M = x2.shape[0]
    pre = torch.empty((M, w1.shape[0]), dtype=dt, device=x2.device) if train else None
    act = gemm(x2, weight_operand(w1, dt), bias=b1, gelu=True, aux=pre, auxgrad=True, out_dtype=dt)
    odt = torch.float32 if residual is not None else (out_dtype or dt)
    y = gemm(act, weight_operand(w2, dt), bias=b2, residual=None if residual is None else _c(residual).reshape(M, w2.shape[0]),
             out_dtype=odt)
    if train:
        grad_sink.use(w1, b1, w2, b2)
    return y, (x2, pre, act)


def mlp_backward(saved, dy2: Tensor, w1: Tensor, b1: Optional[Tensor], w2: Tensor, b2: Optional[Tensor], dt: torch.dtype, want_dx: bool):
    """dy2 [M,N] (mode dt) -> (dx [M,K] in dt or None, dw1, db1, dw2, db2); a parameter gradient that went straight into the
    gradient arena comes back as None (weight_grad)."""
    x2, pre, act = saved
    dpre = dx_product(dy2, w2, dt, dgelu=True, aux=pre, auxgrad=True, out_dtype=dt)
    dw2, db2 = weight_grad(dy2, act, w2, b2, b2 is not None)
    dx = dx_product(dpre, w1, dt, out_dtype=dt) if want_dx else None
    dw1, db1 = weight_grad(dpre, x2, w1, b1, b1 is not None)
    return dx, dw1, db1, dw2, db2


class MlpFn(torch.autograd.Function):
    """mlp_forward / mlp_backward as an autograd node (reference zoo/arch.py:71-76; also the DINO head, zoo/arch.py:252-256)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, residual, out_dtype):
        _need_cuda(x, w1, w2)
        dt = current_dtype()
        xm = to_mode(x, dt)
        y, saved = mlp_forward(xm.reshape(-1, xm.shape[-1]), w1, b1, w2, b2, residual, out_dtype, dt, any(ctx.needs_input_grad[:5]))
        ctx.save_for_backward(*saved, w1, b1, w2, b2)
        ctx.dt, ctx.has_res, ctx.xshape, ctx.xdtype = dt, residual is not None, x.shape, x.dtype
        return y.reshape(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, pre, act, w1, b1, w2, b2 = ctx.saved_tensors
        dx, dw1, db1, dw2, db2 = mlp_backward((x2, pre, act), to_mode(dy.reshape(-1, w2.shape[0]), ctx.dt), w1, b1, w2, b2, ctx.dt,
                                              ctx.needs_input_grad[0])
        if dx is not None:
            dx = (dx if dx.dtype == ctx.xdtype else dx.to(ctx.xdtype)).reshape(ctx.xshape)
        return dx, dw1, db1, dw2, db2, (dy if ctx.has_res else None), None


class AttentionCoreFn(torch.autograd.Function):
    """softmax(Q K^T / sqrt(d)) V on the packed qkv tensor (reference zoo/arch.py:45-52)."""

    @staticmethod
    def forward(ctx, qkv, heads):
        o, lse = attention_fwd(qkv, heads)
        ctx.save_for_backward(qkv, o, lse)
        ctx.heads = heads
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        return attention_bwd(do, qkv, o, lse, ctx.heads), None


ATTENTION_ROWS_MAX_Q = 8
ATTENTION_ROWS_MAX_D = 256


def attention_rows(qkv: Tensor, heads: int, query_idx, want_lse: bool = False):
    """Softmax rows of a few query tokens over all keys, per head (dinox_attention_rows): the probabilities the attention cores never keep.
    qkv: packed [B, N, 3 heads d] (or [B, N, 3, heads, d]) fp32 or bf16 on the device, as attention_fwd takes it; query_idx: 1..8 token
    indices in [0, N) (a sequence of ints or an integer tensor; repeats allowed).  -> probs [B, heads, Q, N] fp32, and with want_lse
    also lse [B, heads, Q] fp32.  No gradient is defined: the result is detached.  Arguments are checked on the host: ValueError."""
    if not isinstance(qkv, Tensor) or not qkv.is_cuda:
        raise ValueError("attention_rows: qkv must be a tensor on a CUDA/HIP device (the MI355X kernel library is the only compute path)")
    if qkv.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"attention_rows: qkv must be float32 or bfloat16, got {qkv.dtype}")
    if qkv.dim() == 5:
        if qkv.shape[2] != 3 or qkv.shape[3] != heads:
            raise ValueError(f"attention_rows: a 5-D qkv must be [B, N, 3, heads={heads}, d], got {tuple(qkv.shape)}")
        qkv = qkv.reshape(qkv.shape[0], qkv.shape[1], -1)
    if qkv.dim() != 3:
        raise ValueError(f"attention_rows: qkv must be [B, N, 3 heads d], got {tuple(qkv.shape)}")
    B, N, C3 = qkv.shape
    if not isinstance(heads, int) or heads < 1 or C3 % (3 * heads) or B < 1 or N < 1 or C3 < 1:
        raise ValueError(f"attention_rows: qkv {tuple(qkv.shape)} is not [B >= 1, N >= 1, 3 x heads={heads} x d]")
    d = C3 // (3 * heads)
    if d > ATTENTION_ROWS_MAX_D:
        raise ValueError(f"attention_rows: head size {d} above {ATTENTION_ROWS_MAX_D}")
    if isinstance(query_idx, Tensor):
        if query_idx.dim() != 1 or query_idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"attention_rows: query_idx must be a 1-D int32 / int64 tensor, got {query_idx.dtype} {tuple(query_idx.shape)}")
        idx = query_idx.tolist()
    else:
        idx = list(query_idx)
        if not all(isinstance(i, int) and not isinstance(i, bool) for i in idx):
            raise ValueError(f"attention_rows: query_idx must hold integers, got {idx}")
    Q = len(idx)
    if not 1 <= Q <= ATTENTION_ROWS_MAX_Q:
        raise ValueError(f"attention_rows: 1 to {ATTENTION_ROWS_MAX_Q} query rows, got {Q}")
    if any(i < 0 or i >= N for i in idx):
        raise ValueError(f"attention_rows: query_idx {idx} outside [0, {N})")
    if not lib.dinox_attention_rows_ok(B, N, heads, d, Q):
        raise ValueError(f"attention_rows: B={B} N={N} heads={heads} d={d} Q={Q} outside the kernel")
    qkv = _c(qkv.detach())
    qi = torch.tensor(idx, dtype=torch.int32, device=qkv.device)
    probs = torch.empty((B, heads, Q, N), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, heads, Q), dtype=torch.float32, device=qkv.device) if want_lse else None
    if TRACE_KERNELS is not None:
        TRACE_KERNELS.append("attention_rows")
    check(lib.dinox_attention_rows(_p(qkv), _p(qi), _p(probs), _p(lse), B, N, heads, d, Q, _code(qkv.dtype), _stream()), "dinox_attention_rows")
    return (probs, lse) if want_lse else probs


ATTENTION_ROLLOUT_MAX_N = 4096


def attention_rollout_step(qkv: Tensor, heads: int, w: Tensor, residual: float = 0.5) -> Tensor:
    """One step of the rollout chain over one block (dinox_attention_rollout_step):
        out[b, j] = residual w[b, j] + (1 - residual) / heads * sum_h sum_i w[b, i] softmax_j(q_i . k_j / sqrt(d))
    qkv: packed [B, N, 3 heads d] (or [B, N, 3, heads, d]) fp32 or bf16 on the device, as attention_fwd takes it; w: [B, N] on the same
    device (taken as fp32); residual in [0, 1].  -> [B, N] fp32, a new tensor.  No N x N matrix is formed; the workspace is B heads N
    floats.  No gradient is defined: the result is detached.  Arguments are checked on the host: ValueError."""
    if not isinstance(qkv, Tensor) or not qkv.is_cuda:
        raise ValueError("attention_rollout_step: qkv must be a tensor on a CUDA/HIP device (the MI355X kernel library is the only compute path)")
    if qkv.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"attention_rollout_step: qkv must be float32 or bfloat16, got {qkv.dtype}")
    if qkv.dim() == 5:
        if qkv.shape[2] != 3 or qkv.shape[3] != heads:
            raise ValueError(f"attention_rollout_step: a 5-D qkv must be [B, N, 3, heads={heads}, d], got {tuple(qkv.shape)}")
        qkv = qkv.reshape(qkv.shape[0], qkv.shape[1], -1)
    if qkv.dim() != 3:
        raise ValueError(f"attention_rollout_step: qkv must be [B, N, 3 heads d], got {tuple(qkv.shape)}")
    B, N, C3 = qkv.shape
    if not isinstance(heads, int) or isinstance(heads, bool) or heads < 1 or C3 % (3 * heads) or B < 1 or N < 1 or C3 < 1:
        raise ValueError(f"attention_rollout_step: qkv {tuple(qkv.shape)} is not [B >= 1, N >= 1, 3 x heads={heads} x d]")
    d = C3 // (3 * heads)
    if d > ATTENTION_ROWS_MAX_D or N > ATTENTION_ROLLOUT_MAX_N:
        raise ValueError(f"attention_rollout_step: head size {d} above {ATTENTION_ROWS_MAX_D} or {N} tokens above {ATTENTION_ROLLOUT_MAX_N}")
    if not isinstance(w, Tensor) or w.device != qkv.device:
        raise ValueError("attention_rollout_step: w must be a tensor on the device of qkv")
    if w.dim() != 2 or tuple(w.shape) != (B, N) or not w.dtype.is_floating_point:
        raise ValueError(f"attention_rollout_step: w must be a float tensor [B={B}, N={N}], got {w.dtype} {tuple(w.shape)}")
    if isinstance(residual, bool) or not isinstance(residual, (int, float)) or not 0.0 <= float(residual) <= 1.0:
        raise ValueError(f"attention_rollout_step: residual must be a number in [0, 1], got {residual!r}")
    if not lib.dinox_attention_rollout_step_ok(B, N, heads, d):
        raise ValueError(f"attention_rollout_step: B={B} N={N} heads={heads} d={d} outside the kernel")
    qkv = _c(qkv.detach())
    w = _c(w.detach().float())
    out = torch.empty((B, N), dtype=torch.float32, device=qkv.device)
    ws = torch.empty((lib.dinox_attention_rollout_step_ws_bytes(B, N, heads) // 4,), dtype=torch.float32, device=qkv.device)
    if TRACE_KERNELS is not None:
        TRACE_KERNELS.append("attention_rollout_step")
    check(lib.dinox_attention_rollout_step(_p(qkv), _p(w), _p(out), _p(ws), B, N, heads, d, float(residual), _code(qkv.dtype), _stream()),
          "dinox_attention_rollout_step")
    return out


class _UnfoldShare:
    """The student and the teacher of one training step see the same batch (scripts/phase5_big_run.py:1741-1743) and can share
    its unfolded form.  Sharing is OPT-IN and scoped: only inside ``with unfold_share():`` (TrainEngine.step) is an unfolded
    batch kept, the entry holds the input tensor itself (so its memory cannot be recycled under the entry) and is matched by
    object identity + version; leaving the scope drops it.  A plain ``PatchViT.forward`` (encode(), eval loops) never looks here."""

    def __init__(self) -> None:
        self.depth = 0
        self.entries: list = []

    def find(self, x: Tensor, patch: int, dt: torch.dtype) -> Optional[Tensor]:
        for (t, ver, p, d, u) in self.entries:
            if t is x and ver == x._version and p == patch and d == dt:
                return u
        return None

    def put(self, x: Tensor, patch: int, dt: torch.dtype, u: Tensor) -> None:
        self.entries = [e for e in self.entries if e[0] is not x][-3:] + [(x, x._version, patch, dt, u)]


_unfold_share = _UnfoldShare()


@contextlib.contextmanager
def unfold_share():
    _unfold_share.depth += 1
    try:
        yield
    finally:
        _unfold_share.depth -= 1
        if _unfold_share.depth == 0:
            _unfold_share.entries = []


def patch_cols(patch: int, dt: torch.dtype) -> int:
    """Columns of the unfolded patch matrix: 3 p^2, rounded up to a multiple of 64 in the bf16 mode when 3 p^2 is no multiple of 8 (patch
    14: 588 -> 640) -- the MFMA bf16 products take no other shape; the tail columns are zeros on both operands."""
    k = 3 * patch * patch
    return k if (dt != torch.bfloat16 or k % 8 == 0) else (k + 63) // 64 * 64


def padded_patch_weight(pw: Tensor, dt: torch.dtype, cols: int) -> Tensor:
    """The patch-embedding weight [D, 3 p^2] as a [D, cols] operand with zero tail columns (built once per optimiser step)."""
    key = (id(pw), "padK", cols)
    hit = weight_cache.extra.get(key)
    if hit is not None and hit[0]() is pw and hit[2] == (pw.data_ptr(), pw._version):
        return hit[1]
    w2 = pw.detach().reshape(pw.shape[0], -1)
    out = torch.zeros((w2.shape[0], cols), dtype=dt, device=pw.device)
    out[:, :w2.shape[1]].copy_(w2)
    weight_cache.extra[key] = (weakref.ref(pw), out, (pw.data_ptr(), pw._version))
    return out


class PatchOperand:
    """A batch of views that is ALREADY the patch-embed operand: ``u`` = [V*P, patch_cols(patch, dtype)], made by
    ``views.make_views(..., patch=p, operand_dtype=dt)`` (dinox_slice_views_patches writes it straight from the u16 stacks).  Stands in
    for the (V,3,S,S) fp32 image batch wherever the training path takes one -- PatchViT.forward, TrainEngine.step -- and answers
    the few questions they ask of it (shape, device); ``patch_unfold`` hands out ``u`` itself."""

    def __init__(self, u: Tensor, V: int, size: int, patch: int) -> None:
        g = size // patch
        assert size % patch == 0 and u.dim() == 2 and u.shape[0] == V * g * g and u.shape[1] >= 3 * patch * patch, (tuple(u.shape), V, size, patch)
        self.u, self.patch, self.size = u, patch, size
        self.shape = torch.Size((V, 3, size, size))

    device = property(lambda self: self.u.device)
    dtype = property(lambda self: self.u.dtype)
    is_cuda = property(lambda self: self.u.is_cuda)

    def dim(self) -> int:
        return 4

    def clone(self) -> "PatchOperand":
        return PatchOperand(self.u.clone(), self.shape[0], self.size, self.patch)

    def copy_(self, other: "PatchOperand", non_blocking: bool = False) -> "PatchOperand":
        if not isinstance(other, PatchOperand) or other.patch != self.patch:
            raise TypeError("a patch-operand batch can only be overwritten by another one of the same patch size")
        self.u.copy_(other.u, non_blocking=non_blocking)
        return self

    def record_stream(self, stream) -> None:
        self.u.record_stream(stream)


def patch_unfold(x, patch: int, dt: torch.dtype) -> Tensor:
    """[V,3,H,W] fp32 -> [V*P, patch_cols(patch, dt)] in dt (shared between student and teacher inside ``unfold_share()`` only).
    A ``PatchOperand`` is that matrix already."""
    if isinstance(x, PatchOperand):
        if x.patch != patch or x.u.dtype != dt or x.u.shape[1] != patch_cols(patch, dt):
            raise ValueError(f"the batch was unfolded for patch {x.patch} in {x.u.dtype} ({x.u.shape[1]} columns); this model takes "
                             f"patch {patch} in {dt} ({patch_cols(patch, dt)} columns)")
        _need_cuda(x.u)
        return x.u
    _need_cuda(x)
    sharing = _unfold_share.depth > 0
    if sharing:
        hit = _unfold_share.find(x, patch, dt)
        if hit is not None:
            return hit
    x0 = x
    x = _c(x)
    if x.dtype != torch.float32:
        x = x.float()
    V, Cn, H, W = x.shape
    assert Cn == 3, "2.5D slice stacks have 3 channels"
    cols = patch_cols(patch, dt)
    u = torch.empty((V * (H // patch) * (W // patch), cols), dtype=dt, device=x.device)
    if cols == 3 * patch * patch:
        check(lib.dinox_patch_unfold(_p(x), _p(u), V, H, W, patch, _code(dt), _stream()), "dinox_patch_unfold")
    else:
        check(lib.dinox_patch_unfold_ld(_p(x), _p(u), V, H, W, patch, cols, _code(dt), _stream()), "dinox_patch_unfold_ld")
    if sharing:
        _unfold_share.put(x0, patch, dt, u)
    return u


class TokensFn(torch.autograd.Function):
    """patch-embed conv (as GEMM) + [CLS|patches] + pos (+scale) + registers (reference zoo/arch.py:216-229)."""

    @staticmethod
    def forward(ctx, x, pw, pb, cls, pos, regs, scale, patch):
        dt = current_dtype()
        u = patch_unfold(x, patch, dt)
        V = x.shape[0]
        D = pw.shape[0]
        P = u.shape[0] // V
        R = 0 if regs is None else regs.shape[1]
        K0 = 3 * patch * patch
        wop = weight_operand(pw, dt) if u.shape[1] == K0 else padded_patch_weight(pw, dt, u.shape[1])
        patches = gemm(u, wop, bias=pb, out_dtype=dt)
        tokens = torch.empty((V, 1 + P + R, D), dtype=torch.float32, device=x.device)
        sc = None if scale is None else _c(scale).reshape(V, D)
        check(lib.dinox_tokens_fwd(_p(patches), _p(_c(cls)), _p(_c(pos)), _p(None if regs is None else _c(regs)), _p(sc), _p(tokens),
                                   V, P, R, D, _code(dt), _stream()), "dinox_tokens_fwd")
        ctx.save_for_backward(u, pw, pb)
        ctx.small = (cls, pos if isinstance(pos, torch.nn.Parameter) else None, regs)       # (an interpolated pos is not a leaf)
        grad_sink.use(pw, pb, cls, ctx.small[1], regs)
        ctx.dims, ctx.dt, ctx.has_scale = (V, P, R, D), dt, scale is not None
        return tokens

    @staticmethod
    def backward(ctx, dtok):
        u, pw, pb = ctx.saved_tensors
        V, P, R, D = ctx.dims
        dt = ctx.dt
        dtok = _c(dtok)
        dev = dtok.device
        dpatches = torch.empty((V * P, D), dtype=dt, device=dev)
        dcls = torch.empty((1, 1, D), dtype=torch.float32, device=dev)
        dpos = torch.empty((1, 1 + P, D), dtype=torch.float32, device=dev)
        dregs = torch.empty((1, R, D), dtype=torch.float32, device=dev) if R else None
        dscale = torch.empty((V, 1, D), dtype=torch.float32, device=dev) if ctx.has_scale else None
        check(lib.dinox_tokens_bwd(_p(dtok), _p(dpatches), _p(dcls), _p(dpos), _p(dregs), _p(dscale), V, P, R, D, _code(dt), _stream()),
              "dinox_tokens_bwd")
        K0 = pw[0].numel()
        if u.shape[1] == K0:
            dw, db = weight_grad(dpatches, u, pw, pb, pb is not None)
        else:
            # padded operand (patch 14): the product gives [D, cols]; its first 3 p^2 columns are the gradient.  One strided add per step
            # into the arena (the only place of a step where a framework kernel does arithmetic, and only at such patch sizes).
            dbt = torch.empty(D, dtype=torch.float32, device=dev) if pb is not None else None
            dwp = gemm(dpatches, u, transA=True, transB=True, out_dtype=torch.float32, colsum_out=dbt)
            sw, sb = grad_sink.lookup(pw), (grad_sink.lookup(pb) if pb is not None else None)
            if sw is not None and (pb is None or sb is not None):
                sw[1].grad.view(D, K0).add_(dwp[:, :K0])
                grad_sink.ready(sw)
                if pb is not None:
                    axpy_(sb[1].grad.view(-1), dbt, 1.0)
                    grad_sink.ready(sb)
                dw = db = None
            else:
                dw, db = dwp[:, :K0].reshape(pw.shape).contiguous(), dbt
        cls, pos, regs = ctx.small
        return None, dw, db, small_grad(cls, dcls), small_grad(pos, dpos), small_grad(regs, dregs), dscale, None


class ScaleEmbedFn(torch.autograd.Function):
    """ScaleEmbedding MLP (reference zoo/arch.py:119-140), fp32, fused per row."""

    @staticmethod
    def forward(ctx, spacing, w0, b0, w2, b2, lnw, lnb, eps):
        _need_cuda(spacing, w0)
        sp = _c(spacing.float())
        V, h, D = sp.shape[0], w0.shape[0], w2.shape[0]
        dev = sp.device
        out = torch.empty((V, 1, D), dtype=torch.float32, device=dev)
        hpre = torch.empty((V, h), dtype=torch.float32, device=dev)
        e = torch.empty((V, D), dtype=torch.float32, device=dev)
        mean = torch.empty(V, dtype=torch.float32, device=dev)
        rstd = torch.empty(V, dtype=torch.float32, device=dev)
        check(lib.dinox_scale_embed_fwd(_p(sp), _p(_c(w0)), _p(b0), _p(_c(w2)), _p(b2), _p(lnw), _p(lnb), _p(out), _p(hpre), _p(e),
                                        _p(mean), _p(rstd), V, h, D, eps, _stream()), "dinox_scale_embed_fwd")
        ctx.save_for_backward(sp, w0, w2, lnw, hpre, e, mean, rstd)
        ctx.small = (w0, b0, w2, b2, lnw, lnb)
        grad_sink.use(*ctx.small)
        return out

    @staticmethod
    def backward(ctx, dout):
        sp, w0, w2, lnw, hpre, e, mean, rstd = ctx.saved_tensors
        V, h, D = sp.shape[0], w0.shape[0], w2.shape[0]
        dev = sp.device
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        dw0, db0, dw2, db2, dlnw, dlnb = f(h, 3), f(h), f(D, h), f(D), f(D), f(D)
        dsp = f(V, 3) if ctx.needs_input_grad[0] else None
        ws = torch.empty(lib.dinox_scale_embed_bwd_ws_bytes(V, h, D), dtype=torch.uint8, device=dev)
        check(lib.dinox_scale_embed_bwd(_p(_c(dout)), _p(sp), _p(_c(w0)), _p(_c(w2)), _p(lnw), _p(hpre), _p(e), _p(mean), _p(rstd),
                                        _p(dw0), _p(db0), _p(dw2), _p(db2), _p(dlnw), _p(dlnb), _p(dsp), _p(ws), V, h, D, _stream()),
              "dinox_scale_embed_bwd")
        pw0, pb0, pw2, pb2, plnw, plnb = ctx.small
        return (dsp, small_grad(pw0, dw0), small_grad(pb0, db0), small_grad(pw2, dw2), small_grad(pb2, db2), small_grad(plnw, dlnw),
                small_grad(plnb, dlnb), None)


def _ds_buffer(ds_out: Optional[Tensor], like: Tensor) -> Tensor:
    """The gradient buffer of a cross-entropy: a fresh one, or the caller's rows of a larger buffer (the engine's head backward takes the
    rows of every term in one operand)."""
    if ds_out is None:
        return torch.empty_like(like)
    assert ds_out.dtype == torch.float32 and ds_out.is_contiguous() and ds_out.shape == like.shape and ds_out.device == like.device
    return ds_out


def dino_ce(s: Tensor, t: Tensor, center: Tensor, student_temp: float, teacher_temp: float, want_grad: bool, grad_scale: float = 1.0,
            ds_out: Optional[Tensor] = None):
    """Returns (loss[1], ds or None).  s, t: [2B, K]."""
    _need_cuda(s, t, center)
    s, t = _c(s.float()), _c(t.float())
    rows, K = s.shape
    loss = torch.empty(1, dtype=torch.float32, device=s.device)
    row_loss = torch.empty(rows, dtype=torch.float32, device=s.device)
    ds = _ds_buffer(ds_out, s) if want_grad else None
    check(lib.dinox_dino_ce(_p(s), _p(t), _p(_c(center).reshape(-1)), student_temp, teacher_temp, grad_scale, _p(loss), _p(ds), _p(row_loss),
                            rows, K, _stream()), "dinox_dino_ce")
    return loss, ds


def dino_ce_multi(s: Tensor, t: Tensor, center: Tensor, student_temp: float, teacher_temp: float, n_global: int, grad_scale: float = 1.0,
                  ds_out: Optional[Tensor] = None):
    """Multi-crop DINO CE (see DinoCEMultiFn): returns (loss[1], ds) with ds already multiplied by grad_scale."""
    _need_cuda(s, t, center)
    sf, tf = _c(s.float()), _c(t.float())
    K = sf.shape[1]
    B = tf.shape[0] // n_global
    n_views = sf.shape[0] // B
    assert tf.shape[0] == n_global * B and sf.shape[0] == n_views * B and tf.shape[1] == K, (tuple(s.shape), tuple(t.shape), n_global)
    loss = torch.empty(1, dtype=torch.float32, device=sf.device)
    ds = _ds_buffer(ds_out, sf)
    ws = torch.empty((n_views + 2 * n_global) * B, dtype=torch.float32, device=sf.device)
    check(lib.dinox_dino_ce_multi(_p(sf), _p(tf), _p(_c(center).reshape(-1)), student_temp, teacher_temp, grad_scale, _p(loss), _p(ds), _p(ws),
                                  B, n_global, n_views, K, _stream()), "dinox_dino_ce_multi")
    return loss, ds


class DinoCEFn(torch.autograd.Function):
    """DINO centring/sharpening cross-entropy (reference scripts/phase5_big_run.py:692-717)."""

    @staticmethod
    def forward(ctx, s, t, center, student_temp, teacher_temp):
        loss, ds = dino_ce(s, t, center, student_temp, teacher_temp, ctx.needs_input_grad[0])
        ctx.save_for_backward(ds)
        ctx.sdtype = s.dtype
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (ds,) = ctx.saved_tensors
        return (ds * g).to(ctx.sdtype), None, None, None, None


class DinoCEMultiFn(torch.autograd.Function):
    """Multi-crop DINO cross-entropy (extension; the reference has 2 global views only): student rows view-major
    [(G+L) views][B], globals first; teacher rows [G][B]; mean over every (teacher view, other student view) pair.
    G = 2, L = 0 equals DinoCEFn."""

    @staticmethod
    def forward(ctx, s, t, center, student_temp, teacher_temp, n_global):
        _need_cuda(s, t, center)
        sf, tf = _c(s.float()), _c(t.float())
        K = sf.shape[1]
        B = tf.shape[0] // n_global
        n_views = sf.shape[0] // B
        assert tf.shape[0] == n_global * B and sf.shape[0] == n_views * B and tf.shape[1] == K, (tuple(s.shape), tuple(t.shape), n_global)
        loss = torch.empty(1, dtype=torch.float32, device=sf.device)
        ds = torch.empty_like(sf) if ctx.needs_input_grad[0] else None
        ws = torch.empty((n_views + 2 * n_global) * B, dtype=torch.float32, device=sf.device)
        check(lib.dinox_dino_ce_multi(_p(sf), _p(tf), _p(_c(center).reshape(-1)), student_temp, teacher_temp, 1.0, _p(loss), _p(ds), _p(ws),
                                      B, n_global, n_views, K, _stream()), "dinox_dino_ce_multi")
        ctx.save_for_backward(ds)
        ctx.sdtype = s.dtype
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (ds,) = ctx.saved_tensors
        return (ds * g).to(ctx.sdtype), None, None, None, None, None


_POS_W: dict = {}


def _bicubic_matrix_1d(n_in: int, n_out: int):
    """[n_out][n_in] weights of torch's non-antialiased bicubic resize (align_corners=False, Keys cubic A = -0.75, border
    replication): what F.interpolate(mode="bicubic") applies along one axis."""
    A = -0.75
    rows = [[0.0] * n_in for _ in range(n_out)]
    scale = n_in / n_out
    for i in range(n_out):
        x = (i + 0.5) * scale - 0.5
        ix = math.floor(x)
        t = x - ix
        w = (((A * (t + 1) - 5 * A) * (t + 1) + 8 * A) * (t + 1) - 4 * A,
             ((A + 2) * t - (A + 3)) * t * t + 1,
             ((A + 2) * (1 - t) - (A + 3)) * (1 - t) * (1 - t) + 1,
             ((A * (2 - t) - 5 * A) * (2 - t) + 8 * A) * (2 - t) - 4 * A)
        for k in range(4):
            rows[i][min(max(ix - 1 + k, 0), n_in - 1)] += w[k]
    return rows


class PosInterpFn(torch.autograd.Function):
    """Position embedding of a crop whose patch grid differs from the model's (multi-crop extension; the reference adds
    ``pos_embed`` as is and cannot take another input size): the CLS entry is kept, the g x g patch grid is resized to
    g_out x g_out by bicubic interpolation, written as ONE fp32 product with the constant [g_out^2, g^2] weight matrix
    (kron of the two 1-D bicubic matrices); backward is the transposed product."""

    @staticmethod
    def forward(ctx, pos, g_out):
        _need_cuda(pos)
        P_in, D = pos.shape[1] - 1, pos.shape[2]
        g_in = int(round(math.sqrt(P_in)))
        assert g_in * g_in == P_in, "position grid must be square"
        key = (g_in, g_out, pos.device)
        W = _POS_W.get(key)
        if W is None:
            m = torch.tensor(_bicubic_matrix_1d(g_in, g_out), dtype=torch.float64)
            W = _POS_W[key] = torch.kron(m, m).float().to(pos.device).contiguous()
        out = torch.empty((1, 1 + g_out * g_out, D), dtype=torch.float32, device=pos.device)
        pf = _c(pos.detach().float())
        out[0, :1].copy_(pf[0, :1])
        gemm(W, pf[0, 1:], transB=True, out=out[0, 1:])
        ctx.W = W
        # A second path into pos_embed: it is counted like the direct one (TokensFn) and its gradient goes the same way -- into the
        # gradient arena, announced to the bucketer once per use.  (Round 2 returned dpos to autograd here: under data parallelism with
        # local crops the arena slice was then all-reduced when the GLOBAL pass had landed, before AccumulateGrad added this part.)
        ctx.pos = pos if isinstance(pos, torch.nn.Parameter) else None
        grad_sink.use(ctx.pos)
        return out

    @staticmethod
    def backward(ctx, g):
        W = ctx.W
        g = _c(g.float())
        dpos = torch.empty((1, 1 + W.shape[1], g.shape[2]), dtype=torch.float32, device=g.device)
        dpos[0, :1].copy_(g[0, :1])
        gemm(W, g[0, 1:], transA=True, transB=True, out=dpos[0, 1:])
        return small_grad(ctx.pos, dpos), None


def interp_pos(pos: Tensor, g_out: int) -> Tensor:
    return PosInterpFn.apply(pos, g_out)


def take_rows(src: Tensor, row: int, dt: torch.dtype, out: Optional[Tensor] = None, out_row0: int = 0, out_rows: int = 0) -> Tensor:
    """src [V,N,D] fp32 -> out[out_row0 + v] = src[v, row] in dt (``feats[:, 0]`` without a strided copy + cast)."""
    _need_cuda(src)
    assert src.dtype == torch.float32 and src.is_contiguous() and src.dim() == 3
    V, N, D = src.shape
    if out is None:
        out = torch.empty((out_rows or V, D), dtype=dt, device=src.device)
    check(lib.dinox_take_rows(src.data_ptr() + 4 * row * D, _p(out), V, N * D, D, out_row0, _code(dt), _stream()), "dinox_take_rows")
    return out


def put_rows_(dst: Tensor, row: int, src: Tensor, src_row0: int = 0, accumulate: bool = False) -> None:
    """dst[v, row] (+)= src[src_row0 + v]  (dst [V,N,D] fp32; src [*,D] fp32 or bf16)."""
    assert dst.dtype == torch.float32 and dst.is_contiguous() and dst.dim() == 3 and src.is_contiguous()
    V, N, D = dst.shape
    check(lib.dinox_put_rows(_p(src), dst.data_ptr() + 4 * row * D, V, N * D, D, src_row0, _code(src.dtype), int(accumulate), _stream()),
          "dinox_put_rows")


def axpy_(y: Tensor, x: Tensor, alpha: float) -> None:
    assert y.dtype == torch.float32 and x.dtype == torch.float32 and y.is_contiguous() and x.is_contiguous() and y.numel() == x.numel()
    check(lib.dinox_axpy(_p(y), _p(x), alpha, y.numel(), _stream()), "dinox_axpy")


def lincomb3(a: Tensor, b: Optional[Tensor], c: Optional[Tensor], wb: float, wc: float) -> Tensor:
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    check(lib.dinox_lincomb3(_p(a), _p(b), _p(c), wb, wc, _p(out), _stream()), "dinox_lincomb3")
    return out


def zero_(t: Tensor) -> None:
    assert t.is_contiguous()
    check(lib.dinox_zero(_p(t), t.numel() * t.element_size(), _stream()), "dinox_zero")


def colmean(t: Tensor) -> Tensor:
    t = _c(t.float())
    out = torch.empty(t.shape[1], dtype=torch.float32, device=t.device)
    check(lib.dinox_colmean(_p(t), _p(out), t.shape[0], t.shape[1], _stream()), "dinox_colmean")
    return out


def center_ema_(center: Tensor, batch_mean: Tensor, momentum: float) -> None:
    assert center.is_contiguous() and center.dtype == torch.float32
    check(lib.dinox_center_ema(_p(center), _p(batch_mean), momentum, center.numel(), _stream()), "dinox_center_ema")


def _sk_operand(t: Tensor) -> Tensor:
    _need_cuda(t)
    t = _c(t.float())
    assert t.dim() == 2, tuple(t.shape)
    return t


def _sk_ws(R: int, K: int, device) -> Tensor:
    return torch.empty(max(1, lib.dinox_sk_ws_floats(R, K)), dtype=torch.float32, device=device)


def sk_col_lse(t: Tensor, a: Optional[Tensor] = None, inv_temp: float = 1.0, out_scale: float = 1.0) -> Tensor:
    """out[k] = out_scale * log sum_i exp(t[i,k] * inv_temp + a[i])  (t [R,K] fp32; a [R] or None = zeros): the column pass of
    Sinkhorn-Knopp in the log domain (include/dinox.h)."""
    t = _sk_operand(t)
    R, K = t.shape
    if a is not None:
        assert a.dtype == torch.float32 and a.is_contiguous() and a.numel() == R, (tuple(a.shape), R)
    out = torch.empty(K, dtype=torch.float32, device=t.device)
    check(lib.dinox_sk_col_lse(_p(t), _p(a), inv_temp, out_scale, _p(out), _p(_sk_ws(R, K, t.device)), R, K, _stream()), "dinox_sk_col_lse")
    return out


def sk_row_lse(t: Tensor, b: Optional[Tensor] = None, inv_temp: float = 1.0, out_scale: float = 1.0) -> Tensor:
    """out[i] = out_scale * log sum_k exp(t[i,k] * inv_temp + b[k])  (b [K] or None = zeros): the row pass."""
    t = _sk_operand(t)
    R, K = t.shape
    if b is not None:
        assert b.dtype == torch.float32 and b.is_contiguous() and b.numel() == K, (tuple(b.shape), K)
    out = torch.empty(R, dtype=torch.float32, device=t.device)
    check(lib.dinox_sk_row_lse(_p(t), _p(b), inv_temp, out_scale, _p(out), R, K, _stream()), "dinox_sk_row_lse")
    return out


def sk_center(t: Tensor, teacher_temp: float, n_iters: int = 3, group=None) -> Tensor:
    """The centre c [K] of the teacher logits t [R,K] for which softmax((t - c) / teacher_temp), row by row, are the Sinkhorn-Knopp
    targets of DINOv2/v3 after ``n_iters`` iterations -- what dino_ce / dino_ce_multi take in place of the EMA centre.

    Without an exchanging ``group``: one call of dinox_sk_center (2 n_iters - 1 passes over t).  With one, Sinkhorn-Knopp runs over the
    GLOBAL batch, as in DINOv2: every column pass is the local sk_col_lse, an all-gather of its K results into [world][K] and
    sk_col_lse on that matrix; the row passes are local.  n_iters all-gathers of K floats, no framework kernel."""
    import torch.distributed as dist
    from .dp import exchanging
    t = _sk_operand(t)
    R, K = t.shape
    if n_iters < 1:
        raise ValueError(f"sk_center: n_iters must be >= 1, got {n_iters}")
    if not exchanging(group):
        out = torch.empty(K, dtype=torch.float32, device=t.device)
        check(lib.dinox_sk_center(_p(t), teacher_temp, n_iters, _p(out), _p(_sk_ws(R, K, t.device)), R, K, _stream()), "dinox_sk_center")
        return out
    world = dist.get_world_size(group)
    inv = C.c_float(1.0 / C.c_float(teacher_temp).value).value     # 1.0f / tau, as the library forms it (a double quotient rounds to the same float)
    gathered = torch.empty((world, K), dtype=torch.float32, device=t.device)
    a = None
    for n in range(1, n_iters + 1):
        dist.all_gather_into_tensor(gathered, sk_col_lse(t, a, inv), group=group)
        if n == n_iters:
            return sk_col_lse(gathered, None, 1.0, teacher_temp)                   # c = -tau b = tau lse
        a = sk_row_lse(t, sk_col_lse(gathered, None, 1.0, -1.0), inv, -1.0)


def sk_center_idle(K: int, n_iters: int, group, device) -> None:
    """A rank WITHOUT rows in a data-parallel ``sk_center`` over the global batch (the iBOT patch rows of a step on which this rank masked
    nothing): it joins the n_iters all-gathers of the column passes with log 0 = -inf in every column, which adds nothing to the other
    ranks' sums, and computes no centre.  (The -inf vector is one framework fill: this path runs only on a step on which a rank
    masked nothing, and sk_center's own passes stay free of framework kernels.)"""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    gathered = torch.empty((world, K), dtype=torch.float32, device=device)
    nothing = torch.full((K,), float("-inf"), dtype=torch.float32, device=device)
    for _ in range(n_iters):
        dist.all_gather_into_tensor(gathered, nothing, group=group)


def gram_loss_fwd(sf: Tensor, tf: Tensor, dt: torch.dtype):
    """Returns (loss[1], saved) with saved = (diff [V,T,T] fp32, shat, snorm) for backward."""
    _need_cuda(sf, tf)
    sf, tf = _c(sf.float()), _c(tf.float())
    V, N, D = sf.shape
    T = N - 1
    dev = sf.device
    cat = torch.empty((V, T, 2 * D), dtype=dt, device=dev)
    catneg = torch.empty((V, T, 2 * D), dtype=dt, device=dev)
    shat = torch.empty((V, T, D), dtype=dt, device=dev)
    snorm = torch.empty((V, T), dtype=torch.float32, device=dev)
    check(lib.dinox_gram_normalize(_p(sf), _p(tf), _p(cat), _p(catneg), _p(shat), _p(snorm), V, N, D, _code(dt), _stream()), "dinox_gram_normalize")
    diff = gemm(cat, catneg, out_dtype=torch.float32)          # [V,T,T] = Gs - Gt in one batched NT GEMM (K = 2D)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    ws = torch.empty(1024, dtype=torch.float32, device=dev)
    check(lib.dinox_sqsum(_p(diff), diff.numel(), 1.0 / float(V * T * T), _p(loss), _p(ws), _stream()), "dinox_sqsum")
    return loss, (diff, shat, snorm)


def gram_loss_bwd(saved, sf_shape, scale: float, dfeats: Optional[Tensor] = None, accumulate=False) -> Tensor:
    diff, shat, snorm = saved
    V, N, D = sf_shape
    T = N - 1
    dt = shat.dtype
    d_in = diff if dt == torch.float32 else cast_bf16(diff)
    # dXh = (4*scale/(V T^2)) * diff . Xh ; diff is symmetric, so it is also the [K=u][M=t] operand of a TN product
    dxh = gemm(d_in, shat, transA=True, transB=True, out_dtype=torch.float32, alpha=4.0 * scale / float(V * T * T))
    if dfeats is None:
        dfeats = torch.zeros((V, N, D), dtype=torch.float32, device=diff.device)
    check(lib.dinox_gram_normalize_bwd(_p(dxh), _p(shat), _p(snorm), None, _p(dfeats), V, N, D, _code(dt), int(accumulate), _stream()),
          "dinox_gram_normalize_bwd")
    return dfeats


class GramLossFn(torch.autograd.Function):
    """Gram-anchoring loss (reference scripts/phase5_big_run.py:723-739)."""

    @staticmethod
    def forward(ctx, sf, tf):
        dt = current_dtype()
        loss, saved = gram_loss_fwd(sf, tf, dt)
        ctx.save_for_backward(*saved)
        ctx.shape = tuple(sf.shape)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        d = gram_loss_bwd(ctx.saved_tensors, ctx.shape, 1.0)
        return d * g, None


def koleo_begin(x: Tensor, group=None):
    """First half of koleo_fwd: normalise the rows and -- under data parallelism -- START the all-gather of the unit rows (V x out_dim fp32 per
    rank, 134 MB at 8 x 512 x 8192) without waiting for it, so that the caller can run independent work (the Gram loss) under the transfer."""
    import torch.distributed as dist
    _need_cuda(x)
    x = _c(x.float())
    V, D = x.shape
    dev = x.device
    from .dp import exchanging
    gather = exchanging(group)
    world = dist.get_world_size(group) if gather else 1
    rank = dist.get_rank(group) if gather else 0
    f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
    xh, norm, sq = f(V, D), f(V), f(V)
    check(lib.dinox_koleo_normalize(_p(x), _p(xh), _p(norm), _p(sq), V, D, 1e-12, _stream()), "dinox_koleo_normalize")
    works = []
    if gather:
        xh_all, sq_all = f(world * V, D), f(world * V)
        works.append(dist.all_gather_into_tensor(xh_all, xh, group=group, async_op=True))
        works.append(dist.all_gather_into_tensor(sq_all, sq, group=group, async_op=True))
    else:
        xh_all, sq_all = xh, sq
    return (xh, xh_all, sq_all, norm, works, group, gather, world, rank, V, D)


def koleo_end(state, eps: float = 1e-8):
    """Second half: wait for the gathered rows, nearest neighbours over the global batch, the loss.  Returns (loss[1], saved)."""
    import torch.distributed as dist
    xh, xh_all, sq_all, norm, works, group, gather, world, rank, V, D = state
    for w in works:
        w.wait()
    dev = xh.device
    f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=dev)
    Vg, row0 = world * V, rank * V
    G = gemm_nt_f32_splitk(xh, xh_all)                                  # [V, Vg] inner products, exact-fp32 MFMA, reduction split over the chip
    idx = torch.empty(V, dtype=torch.int32, device=dev)
    dmin = f(V)
    check(lib.dinox_koleo_nn(_p(G), Vg, _p(sq_all), _p(xh_all), row0, V, Vg, D, _p(idx), _p(dmin), _stream()), "dinox_koleo_nn")
    if gather:
        idx_all = torch.empty(Vg, dtype=torch.int32, device=dev)
        d_all = f(Vg)
        dist.all_gather_into_tensor(idx_all, idx, group=group)
        dist.all_gather_into_tensor(d_all, dmin, group=group)
    else:
        idx_all, d_all = idx, dmin
    loss = f(1)
    check(lib.dinox_koleo_loss(_p(dmin), V, eps, _p(loss), _stream()), "dinox_koleo_loss")
    return loss, (xh_all, idx_all, d_all, norm, (row0, V, Vg, D), eps)


def koleo_fwd(x: Tensor, eps: float = 1e-8, group=None):
    """KoLeo regulariser on the student head output (reference scripts/phase5_big_run.py:742-773, applied at :1764-1766):
    -mean_i log(min_{j != i} ||x^_i - x^_j|| + eps) with x^ = F.normalize(x).  fp32 in both modes, like cdist under autocast.
    Returns (loss[1], saved) -- no autograd, no framework kernel; koleo_bwd(saved, gscale) gives d(gscale * loss)/dx.

    Data parallel (``group`` with more than one rank): the neighbour of a row is searched over the GLOBAL batch, as the
    single-process reference would at that batch size.  Two all-gathers (unit rows; then index + distance per row) and no
    gradient collective: a row's gradient needs its own pair and the pairs that chose it, all of which are gathered data.
    The value returned is this rank's mean over its own rows, so the mean over ranks is the global loss.
    (koleo_begin / koleo_end are the two halves, for callers that have work to run under the first all-gather.)"""
    return koleo_end(koleo_begin(x, group), eps)


def koleo_bwd(saved, gscale: float = 1.0) -> Tensor:
    """dx [V, D] = d(gscale * koleo loss) / dx (the upstream factor is a host scalar here: loss weight / accumulation steps)."""
    xh_all, idx_all, d_all, norm, (row0, V, Vg, D), eps = saved
    dx = torch.empty((V, D), dtype=torch.float32, device=xh_all.device)
    check(lib.dinox_koleo_bwd(_p(xh_all), _p(idx_all), _p(d_all), _p(norm), row0, V, Vg, D, gscale / V, eps, 1e-12, _p(dx), _stream()),
          "dinox_koleo_bwd")
    return dx


class KoLeoFn(torch.autograd.Function):
    """koleo_fwd / koleo_bwd as an autograd node (the engine's fallback path and callers outside the engine)."""

    @staticmethod
    def forward(ctx, x, eps, group):
        loss, saved = koleo_fwd(x, eps, group)
        ctx.saved = saved
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        # the upstream gradient is a device scalar: run with gscale = 1 and scale the result (one small elementwise multiply, no host sync)
        return koleo_bwd(ctx.saved, 1.0) * g, None, None


def koleo_loss(x: Tensor, eps: float = 1e-8, group=None) -> Tensor:
    return KoLeoFn.apply(x, eps, group)


def ntxent_fwd(z: Tensor, temperature: float = 0.1, group=None, force_rect: bool = False):
    """NT-Xent / SimCLR loss on the student head output (reference scripts/phase5_big_run.py:776-813): z [2B, D] = [z1; z2],
    z^ = F.normalize(z), s = z^ z^T / temperature without the diagonal, cross-entropy of row i against row (i + B) mod 2B, mean over
    the 2B rows.  fp32 in both modes (the reference's --amp autocasts the similarity matmul to bf16; this stays more accurate).
    Returns (loss[1], saved) -- no autograd, no framework kernel; ntxent_bwd(saved, gscale) gives d(gscale * loss)/dz.

    Data parallel (``group`` a process group -- not None -- with more than one rank, dp.exchanging): the negatives of a row are the rows of the GLOBAL batch, as the
    single-process reference has them at that batch size.  z holds this rank's Ml = 2 Bl rows [z1_local; z2_local]; the unit rows
    are all-gathered into Z^_all [Mg = world * Ml, D] (rank r's block at row0 = r * Ml), S = Z^_local Z^_all^T is [Ml, Mg], and for
    local row i the excluded column is row0 + i and the positive is row0 + (i + Bl) mod Ml (dinox_ntxent_rows_rect).  Three
    all-gathers: Ml * D floats (unit rows), Ml floats (lse, for the backward's transposed term) and 1 float (the rank's sum of row
    losses).  The loss returned is the GLOBAL mean L = (1 / Mg) sum over all rows: the ``world`` partial sums added in rank order,
    then divided by Mg (a handful of one-element adds) -- the same bits on every rank.  Without an exchanging group the square kernels run, bit for bit as ever;
    ``force_rect`` sends a single rank through the rectangular kernels (world = 1, row0 = 0).

    Gradient convention: a rank's rows enter L through their own row terms AND as columns of every other rank's rows.  The W of
    dinox_ntxent_coeff_rect holds both (the second through the gathered lse, S_ij standing in for S_ji) at scale 1 / (Ml tau), so
    what ntxent_bwd returns is Mg / Ml = world times dL/dz_local -- the factor the engine needs: GradBucketer SUMS the ranks'
    parameter gradients and AdamW applies 1 / world, so the averaged gradient is the single-process gradient of the global batch."""
    _need_cuda(z)
    if z.dim() != 2 or z.shape[0] < 2 or z.shape[0] % 2:
        raise ValueError(f"ntxent: z must be [2B, D] = [z1; z2] with B >= 1, got {tuple(z.shape)}")
    if not temperature > 0.0:
        raise ValueError(f"ntxent: temperature must be positive, got {temperature}")
    from .dp import exchanging
    gather = group is not None and exchanging(group)                    # group=None: never a collective, whatever is initialised
    z = _c(z.float())
    M, D = z.shape
    f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=z.device)
    zh, norm, sq = f(M, D), f(M), f(M)
    check(lib.dinox_koleo_normalize(_p(z), _p(zh), _p(norm), _p(sq), M, D, 1e-12, _stream()), "dinox_koleo_normalize")
    inv_tau = 1.0 / temperature
    if not (gather or force_rect):
        S = gemm_nt_f32_splitk(zh, zh)                                  # [M, M] inner products, exact-fp32 MFMA
        lse, row_loss, loss = f(M), f(M), f(1)
        check(lib.dinox_ntxent_rows(_p(S), M, M, inv_tau, _p(lse), _p(row_loss), _p(loss), _stream()), "dinox_ntxent_rows")
        return loss, (S, zh, norm, lse, inv_tau)
    import torch.distributed as dist
    world = dist.get_world_size(group) if gather else 1
    rank = dist.get_rank(group) if gather else 0
    Mg, row0, Bl = world * M, rank * M, M // 2
    if gather:
        zh_all = f(Mg, D)
        dist.all_gather_into_tensor(zh_all, zh, group=group)
    else:
        zh_all = zh
    S = gemm_nt_f32_splitk(zh, zh_all)                                  # [Ml, Mg]: local rows x global columns
    lse, row_loss, part = f(M), f(M), f(1)
    check(lib.dinox_ntxent_rows_rect(_p(S), Mg, M, Mg, row0, Bl, inv_tau, _p(lse), _p(row_loss), _p(part), _stream()), "dinox_ntxent_rows_rect")
    if gather:
        lse_all, parts = f(Mg), f(world)
        dist.all_gather_into_tensor(lse_all, lse, group=group)
        dist.all_gather_into_tensor(parts, part, group=group)
    else:
        lse_all, parts = lse, part
    loss = parts[0:1].clone()
    for r in range(1, world):                                           # rank order: every rank adds the same floats the same way
        loss += parts[r:r + 1]
    loss /= float(Mg)
    return loss, (S, zh, norm, lse, inv_tau, (zh_all, lse_all, row0))


def ntxent_bwd(saved, gscale: float = 1.0) -> Tensor:
    """dz [2B, D] = d(gscale * NT-Xent loss) / dz (the upstream factor is a host scalar here: 1 / accumulation steps).  After a
    data-parallel ntxent_fwd: world * d(gscale * global loss) / dz_local (see there), from gathered data alone -- no collective."""
    S, zh, norm, lse, inv_tau, *rect = saved
    M, D = zh.shape
    W = torch.empty_like(S)
    if rect:
        zh_all, lse_all, row0 = rect[0]
        Mg = zh_all.shape[0]
        check(lib.dinox_ntxent_coeff_rect(_p(S), Mg, _p(lse), _p(lse_all), M, Mg, row0, M // 2, inv_tau, gscale, _p(W), Mg, _stream()),
              "dinox_ntxent_coeff_rect")
        dzh = gemm(W, zh_all, transB=True, out_dtype=torch.float32)     # dZ^_local = W Z^_all  (W [Ml, Mg])
    else:
        check(lib.dinox_ntxent_coeff(_p(S), M, _p(lse), M, inv_tau, gscale, _p(W), M, _stream()), "dinox_ntxent_coeff")
        dzh = gemm(W, zh, transB=True, out_dtype=torch.float32)         # dZ^ = W Z^  (W [M,M] symmetric, zero diagonal)
    dz = torch.empty_like(zh)
    check(lib.dinox_normalize_bwd(_p(dzh), _p(zh), _p(norm), _p(dz), M, D, 1e-12, _stream()), "dinox_normalize_bwd")
    return dz


class NTXentFn(torch.autograd.Function):
    """ntxent_fwd / ntxent_bwd as an autograd node (the engine's fallback path and callers outside the engine)."""

    @staticmethod
    def forward(ctx, z, temperature, group=None, force_rect=False):
        loss, saved = ntxent_fwd(z, temperature, group, force_rect)
        ctx.saved = saved
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        # the upstream gradient is a device scalar: run with gscale = 1 and scale the result (one small elementwise multiply, no host sync)
        return ntxent_bwd(ctx.saved, 1.0) * g, None, None, None


def simclr_loss(z1: Tensor, z2: Tensor, temperature: float = 0.1, group=None, force_rect: bool = False) -> Tensor:
    """SimCLRLoss(temperature)(z1, z2) of the reference: z1, z2 [B, D] are the head outputs of the two views.  ``group``: the negatives
    span the global batch and the value is the global mean loss (ntxent_fwd); its gradient is then world times the global loss's."""
    _need_cuda(z1, z2)
    if z1.shape != z2.shape or z1.dim() != 2:
        raise ValueError(f"simclr_loss: z1 and z2 must both be [B, D], got {tuple(z1.shape)} and {tuple(z2.shape)}")
    return NTXentFn.apply(torch.cat([z1, z2], 0), temperature, group, force_rect)


# ------------------------------------------------------------------------------------------
# MAE masked-token glue (csrc/mae.hip; reference scripts/phase5_big_run.py:816-1023)
# ------------------------------------------------------------------------------------------
def mae_len_keep(L: int, mask_ratio: float) -> int:
    """``int(L * (1 - mask_ratio))`` as the reference's random_masking computes it (:976)."""
    return int(L * (1 - mask_ratio))


def _mae_ids(ids: Tensor, V: int, n: int, what: str) -> Tensor:
    _need_cuda(ids)
    if ids.dtype != torch.int32 or tuple(ids.shape) != (V, n):
        raise ValueError(f"mae: {what} must be int32 [{V}, {n}], got {ids.dtype} {tuple(ids.shape)}")
    return _c(ids)


def mae_mask_ids(noise: Tensor, len_keep: int):
    """noise [V, L] fp32 -> (ids_restore [V, L] int32, ids_keep [V, len_keep] int32): ``argsort(argsort(noise))`` and the first
    ``len_keep`` columns of ``argsort(noise)`` of the reference's random_masking (:981-985), ties resolved as a stable sort."""
    _need_cuda(noise)
    if noise.dim() != 2:
        raise ValueError(f"mae_mask_ids: noise must be [V, L], got {tuple(noise.shape)}")
    noise = _c(noise.float())
    V, L = noise.shape
    ids_restore = torch.empty((V, L), dtype=torch.int32, device=noise.device)
    ids_keep = torch.empty((V, max(int(len_keep), 0)), dtype=torch.int32, device=noise.device)
    check(lib.dinox_mae_mask_ids(_p(noise), _p(ids_restore), _p(ids_keep), V, L, int(len_keep), _stream()), "dinox_mae_mask_ids")
    return ids_restore, ids_keep


def mae_gather_unfold(x: Tensor, ids_keep: Tensor, patch: int, dt: torch.dtype) -> Tensor:
    """[V,3,H,W] fp32 -> the patch-embed operand of the kept patches only: [V*Lk, patch_cols(patch, dt)] in dt, the rows
    v*L + ids_keep[v, r] of ``patch_unfold`` bit for bit."""
    if isinstance(x, PatchOperand):
        raise ValueError("mae: the batch must be the fp32 image batch (the loss reads its pixels), not a PatchOperand")
    _need_cuda(x)
    x = _c(x)
    if x.dtype != torch.float32:
        x = x.float()
    V, Cn, H, W = x.shape
    assert Cn == 3, "2.5D slice stacks have 3 channels"
    ids_keep = _mae_ids(ids_keep, V, ids_keep.shape[-1], "ids_keep")
    Lk = ids_keep.shape[1]
    cols = patch_cols(patch, dt)
    u = torch.empty((V * Lk, cols), dtype=dt, device=x.device)
    check(lib.dinox_mae_gather_unfold(_p(x), _p(ids_keep), _p(u), V, H, W, patch, Lk, cols, _code(dt), _stream()), "dinox_mae_gather_unfold")
    return u


class MaeTokensFn(torch.autograd.Function):
    """Encoder input of the MAE pass: the patch-embedding product on the KEPT patches only (M = V*Lk rows instead of V*L), then
    [cls + pos[0] | patches[r] + pos[1 + ids_keep[r]]] (reference MaeModel.forward :998-1013).  Same conventions as TokensFn."""

    @staticmethod
    def forward(ctx, x, pw, pb, cls, pos, ids_restore, ids_keep, patch):
        dt = current_dtype()
        _need_cuda(x, pw, cls, pos)
        V = x.shape[0]
        D = pw.shape[0]
        L = pos.shape[1] - 1
        ids_restore = _mae_ids(ids_restore, V, L, "ids_restore")
        u = mae_gather_unfold(x, ids_keep, patch, dt)
        Lk = u.shape[0] // V
        K0 = 3 * patch * patch
        wop = weight_operand(pw, dt) if u.shape[1] == K0 else padded_patch_weight(pw, dt, u.shape[1])
        patches = gemm(u, wop, bias=pb, out_dtype=dt)
        tokens = torch.empty((V, 1 + Lk, D), dtype=torch.float32, device=x.device)
        check(lib.dinox_mae_tokens_fwd(_p(patches), _p(_c(cls)), _p(_c(pos)), _p(_c(ids_keep)), _p(tokens), V, L, Lk, D, _code(dt), _stream()),
              "dinox_mae_tokens_fwd")
        ctx.save_for_backward(u, pw, pb, ids_restore)
        ctx.small = (cls, pos)
        grad_sink.use(pw, pb, cls, pos)
        ctx.dims, ctx.dt = (V, L, Lk, D), dt
        return tokens

    @staticmethod
    def backward(ctx, dtok):
        u, pw, pb, ids_restore = ctx.saved_tensors
        V, L, Lk, D = ctx.dims
        dt = ctx.dt
        dtok = _c(dtok)
        dev = dtok.device
        dpatches = torch.empty((V * Lk, D), dtype=dt, device=dev)
        dcls = torch.empty((1, 1, D), dtype=torch.float32, device=dev)
        dpos = torch.empty((1, 1 + L, D), dtype=torch.float32, device=dev)
        check(lib.dinox_mae_tokens_bwd(_p(dtok), _p(ids_restore), _p(dpatches), _p(dcls), _p(dpos), V, L, Lk, D, _code(dt), _stream()),
              "dinox_mae_tokens_bwd")
        K0 = pw[0].numel()
        if u.shape[1] == K0:
            dw, db = weight_grad(dpatches, u, pw, pb, pb is not None)
        else:
            # padded operand (3 p^2 % 8 != 0 in bf16): as TokensFn.backward -- the first 3 p^2 columns of the product are the gradient
            dbt = torch.empty(D, dtype=torch.float32, device=dev) if pb is not None else None
            dwp = gemm(dpatches, u, transA=True, transB=True, out_dtype=torch.float32, colsum_out=dbt)
            sw, sb = grad_sink.lookup(pw), (grad_sink.lookup(pb) if pb is not None else None)
            if sw is not None and (pb is None or sb is not None):
                sw[1].grad.view(D, K0).add_(dwp[:, :K0])
                grad_sink.ready(sw)
                if pb is not None:
                    axpy_(sb[1].grad.view(-1), dbt, 1.0)
                    grad_sink.ready(sb)
                dw = db = None
            else:
                dw, db = dwp[:, :K0].reshape(pw.shape).contiguous(), dbt
        cls, pos = ctx.small
        return None, dw, db, small_grad(cls, dcls), small_grad(pos, dpos), None, None, None


class MaeUnshuffleFn(torch.autograd.Function):
    """Decoder input (reference MaeDecoder.forward :864-870): e [V, 1+Lk, Dd] (the decoder_embed output, fp32 or bf16) -> fp32
    [V, 1+L, Dd] with the kept rows back at their patch positions, mask_token elsewhere, plus the fixed decoder_pos_embed (which gets
    no gradient)."""

    @staticmethod
    def forward(ctx, e, mask_token, dec_pos, ids_restore, ids_keep):
        _need_cuda(e, mask_token, dec_pos)
        if e.dtype not in (torch.float32, torch.bfloat16):
            e = e.float()
        e = _c(e)
        V, Ne, Dd = e.shape
        L, Lk = dec_pos.shape[1] - 1, Ne - 1
        ids_restore = _mae_ids(ids_restore, V, L, "ids_restore")
        ids_keep = _mae_ids(ids_keep, V, Lk, "ids_keep")
        xd = torch.empty((V, 1 + L, Dd), dtype=torch.float32, device=e.device)
        check(lib.dinox_mae_unshuffle_fwd(_p(e), _p(_c(mask_token)), _p(_c(dec_pos)), _p(ids_restore), _p(xd), V, L, Lk, Dd, _code(e.dtype),
                                          _stream()), "dinox_mae_unshuffle_fwd")
        ctx.save_for_backward(ids_restore, ids_keep)
        ctx.mask_token = mask_token
        grad_sink.use(mask_token)
        ctx.dims, ctx.edt = (V, L, Lk, Dd), e.dtype
        return xd

    @staticmethod
    def backward(ctx, g):
        ids_restore, ids_keep = ctx.saved_tensors
        V, L, Lk, Dd = ctx.dims
        g = _c(g)
        dev = g.device
        de = torch.empty((V, 1 + Lk, Dd), dtype=ctx.edt, device=dev)
        dmask = torch.empty((1, 1, Dd), dtype=torch.float32, device=dev)
        ws = torch.empty((V, Dd), dtype=torch.float32, device=dev)
        check(lib.dinox_mae_unshuffle_bwd(_p(g), _p(ids_keep), _p(ids_restore), _p(de), _p(dmask), _p(ws), V, L, Lk, Dd, _code(ctx.edt),
                                          _stream()), "dinox_mae_unshuffle_bwd")
        return de, small_grad(ctx.mask_token, dmask), None, None, None


def mae_loss_fwd(pred: Tensor, x: Tensor, ids_restore: Tensor, len_keep: int, patch: int, lead: int = 0):
    """Reconstruction loss of the reference's forward_loss (:955-969) without a patchified copy of the batch: pred
    [V, lead + L, 3 p^2] (fp32 or bf16; lead = 1 when the decoder's CLS row is still in front), x [V,3,H,W] fp32, ids_restore [V, L].
    Returns (loss[1] fp32 on the device, saved); mae_loss_bwd(saved, gscale) gives d(gscale * loss)/dpred."""
    _need_cuda(pred, x, ids_restore)
    if isinstance(x, PatchOperand):
        raise ValueError("mae: the batch must be the fp32 image batch (the loss reads its pixels), not a PatchOperand")
    if pred.dtype not in (torch.float32, torch.bfloat16):
        pred = pred.float()
    pred, x = _c(pred), _c(x.float())
    V, Cn, H, W = x.shape
    L = (H // patch) * (W // patch) if patch > 0 else 0
    if Cn != 3 or pred.dim() != 3 or tuple(pred.shape) != (V, lead + L, 3 * patch * patch):
        raise ValueError(f"mae_loss: pred {tuple(pred.shape)} is not [V, {lead} + L, 3 p^2] = [{V}, {lead + L}, {3 * patch * patch}] "
                         f"for images {tuple(x.shape)} and patch {patch}")
    ids_restore = _mae_ids(ids_restore, V, L, "ids_restore")
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = torch.empty(V * L, dtype=torch.float32, device=x.device)
    check(lib.dinox_mae_loss_fwd(_p(pred), _p(x), _p(ids_restore), _p(loss), _p(ws), V, H, W, patch, int(len_keep), lead, _code(pred.dtype),
                                 _stream()), "dinox_mae_loss_fwd")
    return loss, (pred, x, ids_restore, int(len_keep), patch, lead)


def mae_loss_bwd(saved, gscale: float = 1.0, out_dtype: Optional[torch.dtype] = None) -> Tensor:
    """dpred (the layout of pred; ``out_dtype`` defaults to pred's dtype) = d(gscale * loss)/dpred: exactly 0 on kept patches and on the
    lead rows.  The upstream factor is a host scalar (1 / accumulation steps)."""
    pred, x, ids_restore, len_keep, patch, lead = saved
    V, _, H, W = x.shape
    dpred = torch.empty(pred.shape, dtype=out_dtype or pred.dtype, device=pred.device)
    check(lib.dinox_mae_loss_bwd(_p(pred), _p(x), _p(ids_restore), _p(dpred), float(gscale), V, H, W, patch, len_keep, lead,
                                 _code(pred.dtype), _code(dpred.dtype), _stream()), "dinox_mae_loss_bwd")
    return dpred


class MaeLossFn(torch.autograd.Function):
    """mae_loss_fwd / mae_loss_bwd as an autograd node (callers outside the engine)."""

    @staticmethod
    def forward(ctx, pred, x, ids_restore, len_keep, patch, lead):
        loss, saved = mae_loss_fwd(pred, x, ids_restore, len_keep, patch, lead)
        ctx.saved, ctx.pdt = saved, pred.dtype
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        # the upstream gradient is a device scalar: run with gscale = 1 and scale the result (no host sync)
        d = mae_loss_bwd(ctx.saved, 1.0) * g
        return (d if d.dtype == ctx.pdt else d.to(ctx.pdt)), None, None, None, None, None


# ---------------------------------------------------------------- iBOT masked-patch objective (csrc/ibot.hip)
IBOT_MASK_CHUNK = 64      # csrc/ibot.hip: masked rows per partial sum of dinox_ibot_put_mask_bwd


def _row_index(idx: Tensor, what: str) -> Tensor:
    _need_cuda(idx)
    if idx.dtype != torch.int32 or idx.dim() != 1:
        raise TypeError(f"{what} must be a 1-D int32 tensor on the device, got {idx.dtype} {tuple(idx.shape)}")
    return _c(idx)


def gather_rows(src: Tensor, row: Tensor, dt: torch.dtype, out: Optional[Tensor] = None, out_row0: int = 0, out_rows: int = 0) -> Tensor:
    """out[out_row0 + m] = src.view(-1, D)[row[m]] in dt (src fp32 [..., D]; row int32 [M] on the device): ``take_rows`` by index.  An entry
    outside the rows of src is skipped."""
    _need_cuda(src)
    assert src.dtype == torch.float32 and src.is_contiguous() and src.dim() >= 2
    row = _row_index(row, "row")
    D, M = src.shape[-1], row.numel()
    if out is None:
        out = torch.empty((out_rows or M, D), dtype=dt, device=src.device)
    assert out.is_contiguous() and out.dtype == dt and out.shape[-1] == D and out_row0 >= 0 and out_row0 + M <= out.numel() // D
    check(lib.dinox_gather_rows(_p(src), _p(row), _p(out), M, src.numel() // D, D, out_row0, _code(dt), _stream()), "dinox_gather_rows")
    return out


def scatter_add_rows_(dst: Tensor, row: Tensor, src: Tensor, src_row0: int = 0) -> None:
    """dst.view(-1, D)[row[m]] += src[src_row0 + m]  (dst fp32 [..., D]; src [*, D] fp32 or bf16; the rows must be distinct)."""
    assert dst.dtype == torch.float32 and dst.is_contiguous() and src.is_contiguous() and dst.shape[-1] == src.shape[-1]
    row = _row_index(row, "row")
    D, M = dst.shape[-1], row.numel()
    assert src_row0 >= 0 and src_row0 + M <= src.numel() // D
    check(lib.dinox_scatter_add_rows(_p(src), _p(row), _p(dst), M, dst.numel() // D, D, src_row0, _code(src.dtype), _stream()),
          "dinox_scatter_add_rows")


def ibot_put_mask_(patches: Tensor, mask_token: Tensor, idx: Tensor) -> None:
    """patches[idx[m]] = mask_token (rounded to the dtype of patches [rows, D]), in place."""
    assert patches.is_contiguous() and patches.dim() == 2 and mask_token.dtype == torch.float32 and mask_token.numel() == patches.shape[1]
    idx = _row_index(idx, "idx")
    check(lib.dinox_ibot_put_mask(_p(patches), _p(_c(mask_token)), _p(idx), idx.numel(), patches.shape[0], patches.shape[1],
                                  _code(patches.dtype), _stream()), "dinox_ibot_put_mask")


def ibot_put_mask_bwd_(dpatches: Tensor, idx: Tensor) -> Tensor:
    """-> dmask_token [1, 1, D] fp32 = sum_m dpatches[idx[m]] (fixed order); those rows of dpatches [rows, D] are then set to 0."""
    assert dpatches.is_contiguous() and dpatches.dim() == 2
    idx = _row_index(idx, "idx")
    M, D = idx.numel(), dpatches.shape[1]
    dmask = torch.empty((1, 1, D), dtype=torch.float32, device=dpatches.device)
    ws = torch.empty(((M + IBOT_MASK_CHUNK - 1) // IBOT_MASK_CHUNK, D), dtype=torch.float32, device=dpatches.device)
    check(lib.dinox_ibot_put_mask_bwd(_p(dpatches), _p(idx), _p(dmask), _p(ws), M, dpatches.shape[0], D, _code(dpatches.dtype), _stream()),
          "dinox_ibot_put_mask_bwd")
    return dmask


def ibot_ce(s: Tensor, t: Tensor, center: Tensor, w: Tensor, student_temp: float, teacher_temp: float, scale: float = 1.0,
            want_grad: bool = True, grad_scale: float = 1.0, ds_out: Optional[Tensor] = None):
    """The masked-patch cross-entropy: s, t [M, K] fp32 (rows of a larger contiguous matrix are fine), center [K], w [M] fp32.
    Returns (loss[1] = scale * sum_m w[m] row_loss[m], ds or None, row_loss [M]); ds = grad_scale * scale * w[m] * d row_loss[m] / d s[m]."""
    _need_cuda(s, t, center, w)
    assert s.dtype == torch.float32 and t.dtype == torch.float32 and s.is_contiguous() and t.is_contiguous() and s.shape == t.shape and s.dim() == 2
    M, K = s.shape
    assert w.dtype == torch.float32 and w.is_contiguous() and w.numel() == M and center.numel() == K, (tuple(w.shape), tuple(center.shape), M, K)
    loss = torch.empty(1, dtype=torch.float32, device=s.device)
    row_loss = torch.empty(M, dtype=torch.float32, device=s.device)
    ds = _ds_buffer(ds_out, s) if want_grad else None
    check(lib.dinox_ibot_ce(_p(s), _p(t), _p(_c(center.float()).reshape(-1)), _p(w), student_temp, teacher_temp, scale, grad_scale, _p(loss),
                            _p(ds), _p(row_loss), M, K, _stream()), "dinox_ibot_ce")
    return loss, ds, row_loss


def ibot_center_ema_(center: Tensor, sum_count: Tensor, momentum: float) -> None:
    """center [K] moves towards sum_count[:K] / sum_count[K] (column sums and number of the masked teacher rows); untouched at a count of 0."""
    assert center.is_contiguous() and center.dtype == torch.float32 and sum_count.dtype == torch.float32 and sum_count.is_contiguous()
    assert sum_count.numel() == center.numel() + 1
    check(lib.dinox_ibot_center_ema(_p(center), _p(sum_count), momentum, center.numel(), _stream()), "dinox_ibot_center_ema")


class MaskedTokensFn(torch.autograd.Function):
    """TokensFn with the embedding of the patches ``idx`` (int32 [M], flat positions v P + i, distinct) replaced by ``mask_token``
    [1, 1, D] after the patch-embedding product and before pos_embed / the scale embedding are added: unfold, patch product,
    dinox_ibot_put_mask, dinox_tokens_fwd.  Backward: dinox_tokens_bwd, dinox_ibot_put_mask_bwd (the mask token's gradient; the masked rows
    send nothing into the patch product), then the dW / db products of TokensFn."""

    @staticmethod
    def forward(ctx, x, pw, pb, cls, pos, regs, scale, patch, idx, mask_token):
        dt = current_dtype()
        u = patch_unfold(x, patch, dt)
        idx = _row_index(idx, "idx")
        V = x.shape[0]
        D = pw.shape[0]
        P = u.shape[0] // V
        R = 0 if regs is None else regs.shape[1]
        K0 = 3 * patch * patch
        wop = weight_operand(pw, dt) if u.shape[1] == K0 else padded_patch_weight(pw, dt, u.shape[1])
        patches = gemm(u, wop, bias=pb, out_dtype=dt)
        ibot_put_mask_(patches, mask_token.detach().reshape(-1), idx)
        tokens = torch.empty((V, 1 + P + R, D), dtype=torch.float32, device=x.device)
        sc = None if scale is None else _c(scale).reshape(V, D)
        check(lib.dinox_tokens_fwd(_p(patches), _p(_c(cls)), _p(_c(pos)), _p(None if regs is None else _c(regs)), _p(sc), _p(tokens),
                                   V, P, R, D, _code(dt), _stream()), "dinox_tokens_fwd")
        ctx.save_for_backward(u, pw, pb, idx)
        ctx.small = (cls, pos if isinstance(pos, torch.nn.Parameter) else None, regs, mask_token)
        grad_sink.use(pw, pb, cls, ctx.small[1], regs, mask_token)
        ctx.dims, ctx.dt, ctx.has_scale = (V, P, R, D), dt, scale is not None
        return tokens

    @staticmethod
    def backward(ctx, dtok):
        u, pw, pb, idx = ctx.saved_tensors
        V, P, R, D = ctx.dims
        dt = ctx.dt
        dtok = _c(dtok)
        dev = dtok.device
        dpatches = torch.empty((V * P, D), dtype=dt, device=dev)
        dcls = torch.empty((1, 1, D), dtype=torch.float32, device=dev)
        dpos = torch.empty((1, 1 + P, D), dtype=torch.float32, device=dev)
        dregs = torch.empty((1, R, D), dtype=torch.float32, device=dev) if R else None
        dscale = torch.empty((V, 1, D), dtype=torch.float32, device=dev) if ctx.has_scale else None
        check(lib.dinox_tokens_bwd(_p(dtok), _p(dpatches), _p(dcls), _p(dpos), _p(dregs), _p(dscale), V, P, R, D, _code(dt), _stream()),
              "dinox_tokens_bwd")
        dmask = ibot_put_mask_bwd_(dpatches, idx)
        dw, db = _patch_weight_grad(dpatches, u, pw, pb, D, dev)
        cls, pos, regs, mask_token = ctx.small
        return (None, dw, db, small_grad(cls, dcls), small_grad(pos, dpos), small_grad(regs, dregs), dscale, None, None,
                small_grad(mask_token, dmask))


class AnnounceFn(torch.autograd.Function):
    """Identity on ``x`` that tells the gradient sink, at this point of backward, that ``param`` has its (zero) gradient: the place of
    ``mask_token`` in a token assembly that masks nothing.  Under data parallelism the ranks exchange a gradient bucket when its last
    parameter is announced, and all ranks must do so in one order: a rank that masked nothing on a step (and every rank's local crops)
    announces mask_token here, just ahead of the token assembly's own backward, where MaskedTokensFn announces it on the ranks that
    did mask -- no other bucket completes in between.  No kernel is launched."""

    @staticmethod
    def forward(ctx, x, param):
        ctx.param = param
        grad_sink.use(param)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        slot = grad_sink.lookup(ctx.param)
        if slot is not None:
            grad_sink.ready(slot)
        return g, None


def _patch_weight_grad(dpatches: Tensor, u: Tensor, pw: Tensor, pb: Optional[Tensor], D: int, dev):
    """The dW / db products of the patch embedding with the arithmetic of TokensFn.backward (whose text stays as it is)."""
    K0 = pw[0].numel()
    if u.shape[1] == K0:
        return weight_grad(dpatches, u, pw, pb, pb is not None)
    dbt = torch.empty(D, dtype=torch.float32, device=dev) if pb is not None else None
    dwp = gemm(dpatches, u, transA=True, transB=True, out_dtype=torch.float32, colsum_out=dbt)
    sw, sb = grad_sink.lookup(pw), (grad_sink.lookup(pb) if pb is not None else None)
    if sw is not None and (pb is None or sb is not None):
        sw[1].grad.view(D, K0).add_(dwp[:, :K0])
        grad_sink.ready(sw)
        if pb is not None:
            axpy_(sb[1].grad.view(-1), dbt, 1.0)
            grad_sink.ready(sb)
        return None, None
    return dwp[:, :K0].reshape(pw.shape).contiguous(), dbt


def adamw_hyper(lr: float, beta1: float, beta2: float, step_t: int) -> list:
    """The three per-step scalars of the optimiser pass -- [lr, 1/(1-beta1^t), 1/sqrt(1-beta2^t)] -- for dinox_adamw_ema_dev."""
    # with the betas as the fp32 values the C entry receives (dinox_adamw_ema raises (double)(float)beta to the step): the replayed
    # launch then gets bit-for-bit the corrections of the eager one (0.999 as a double and as a float differ by 6e-6 in the second)
    beta1, beta2 = C.c_float(beta1).value, C.c_float(beta2).value
    return [lr, 1.0 / (1.0 - beta1 ** step_t), 1.0 / math.sqrt(1.0 - beta2 ** step_t)]


def adamw_ema_(p: Tensor, g: Tensor, m: Tensor, v: Tensor, teacher: Optional[Tensor], *, lr: float, weight_decay: float,
               beta1: float, beta2: float, eps: float, step_t: int, ema: float, grad_scale: float = 1.0,
               hyper: Optional[Tensor] = None) -> Tensor:
    """Fused grad-norm + AdamW + EMA over flat fp32 arenas; returns gnorm_sq[1] (device).  With ``hyper`` (device float[3], see
    adamw_hyper) lr and the bias corrections are read from device memory: the launch is replayable from a captured hipGraph."""
    _need_cuda(p, g, m, v)
    for t in (p, g, m, v) + ((teacher,) if teacher is not None else ()):
        assert t.is_contiguous() and t.dtype == torch.float32 and t.numel() == p.numel()
    out = torch.empty(1, dtype=torch.float32, device=p.device)
    ws = torch.empty(4096, dtype=torch.float32, device=p.device)
    if hyper is not None:
        assert hyper.is_cuda and hyper.dtype == torch.float32 and hyper.numel() == 3
        check(lib.dinox_adamw_ema_dev(_p(p), _p(g), _p(m), _p(v), _p(teacher), p.numel(), _p(hyper), weight_decay, beta1, beta2, eps, ema,
                                      grad_scale, _p(out), _p(ws), _stream()), "dinox_adamw_ema_dev")
        return out
    check(lib.dinox_adamw_ema(_p(p), _p(g), _p(m), _p(v), _p(teacher), p.numel(), lr, weight_decay, beta1, beta2, eps, step_t, ema,
                              grad_scale, _p(out), _p(ws), _stream()), "dinox_adamw_ema")
    return out


def sumsq(x: Tensor) -> Tensor:
    x = _c(x)
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = torch.empty(4096, dtype=torch.float32, device=x.device)
    check(lib.dinox_sumsq(_p(x), x.numel(), _p(out), _p(ws), _stream()), "dinox_sumsq")
    return out


class GeluFn(torch.autograd.Function):
    """Stand-alone exact-erf GELU (fp32 math) for module paths that cannot use the fused epilogue."""

    @staticmethod
    def forward(ctx, x):
        _need_cuda(x)
        xf = _c(x.float())
        y = torch.empty_like(xf)
        check(lib.dinox_gelu_fwd(_p(xf), _p(y), xf.numel(), _stream()), "dinox_gelu_fwd")
        ctx.save_for_backward(xf)
        ctx.xdtype = x.dtype
        return y.to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        (xf,) = ctx.saved_tensors
        dyf = _c(dy.float())
        dx = torch.empty_like(xf)
        check(lib.dinox_gelu_bwd(_p(dyf), _p(xf), _p(dx), xf.numel(), _stream()), "dinox_gelu_bwd")
        return dx.to(ctx.xdtype)


# ------------------------------------------------------------------------------------------
# view retrieval (csrc/retrieval.hip)
# ------------------------------------------------------------------------------------------
def normalize_rows(x: Tensor):
    """F.normalize(x, dim=-1) of fp32 rows [V, D] (x / max(||x||, 1e-12)) on dinox_koleo_normalize; returns (unit rows, norms [V])."""
    _need_cuda(x)
    x = _c(x.float())
    V, D = x.shape
    f = lambda *sh: torch.empty(sh, dtype=torch.float32, device=x.device)
    xh, norm, sq = f(V, D), f(V), f(V)
    check(lib.dinox_koleo_normalize(_p(x), _p(xh), _p(norm), _p(sq), V, D, 1e-12, _stream()), "dinox_koleo_normalize")
    return xh, norm


def retrieval_rank(q: Tensor, k: Tensor, target: Optional[Tensor] = None):
    """For each fp32 query row of q [Nq, D] against the fp32 key rows of k [Nk, D]: (rank, best_idx, best_val, pos_val), each [Nq] --
    rank[i] is the place of key target[i] (default: i) in a stable descending sort of the scores q_i . k_j, best_* the row maximum and
    its first index, pos_val the positive's score.  The scores exist only in the accumulators of the exact-fp32 MFMA: no Nq x Nk
    tensor is allocated.  The rows are used as given (normalise them first: normalize_rows); target indices are checked against
    [0, Nk) here (the kernel itself clamps them).  Rows of NaNs compare false with everything: see include/dinox.h."""
    _need_cuda(q, k, target)
    if q.dtype != torch.float32 or k.dtype != torch.float32 or q.dim() != 2 or k.dim() != 2 or q.shape[1] != k.shape[1]:
        raise ValueError(f"retrieval_rank: fp32 [Nq, D] and [Nk, D] rows expected, got {q.dtype}{tuple(q.shape)} and {k.dtype}{tuple(k.shape)}")
    if q.stride(1) != 1 or q.stride(0) < q.shape[1]:
        q = q.contiguous()
    if k.stride(1) != 1 or k.stride(0) < k.shape[1]:
        k = k.contiguous()
    (Nq, D), Nk = q.shape, k.shape[0]
    if min(Nq, Nk, D) < 1:
        raise ValueError(f"retrieval_rank: empty operand (Nq={Nq}, Nk={Nk}, D={D})")
    if target is None:
        if Nq != Nk:
            raise ValueError(f"retrieval_rank: without target, query i is matched to key i and Nq must equal Nk ({Nq}, {Nk})")
    else:
        if target.shape != (Nq,):
            raise ValueError(f"retrieval_rank: target must have shape ({Nq},), got {tuple(target.shape)}")
        if target.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"retrieval_rank: target must be int32 or int64 indices, got {target.dtype}")
        lo, hi = int(target.min()), int(target.max())          # one host sync on an evaluation path: the kernel clamps, it cannot refuse
        if lo < 0 or hi >= Nk:
            raise ValueError(f"retrieval_rank: target indices must lie in [0, {Nk}), got [{lo}, {hi}]")
        target = _c(target.to(torch.int32))
    dev = q.device
    rank = torch.empty(Nq, dtype=torch.int32, device=dev)
    best_idx = torch.empty(Nq, dtype=torch.int32, device=dev)
    best_val = torch.empty(Nq, dtype=torch.float32, device=dev)
    pos_val = torch.empty(Nq, dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib.dinox_retrieval_ws_bytes(Nq, Nk, D)), dtype=torch.uint8, device=dev)
    check(lib.dinox_retrieval_rank(_p(q), q.stride(0), _p(k), k.stride(0), _p(target), Nq, Nk, D, _p(rank), _p(best_idx), _p(best_val),
                                   _p(pos_val), _p(ws), _stream()), "dinox_retrieval_rank")
    return rank, best_idx, best_val, pos_val


def _rr_rows(name: str, q: Tensor, k: Tensor):
    """The row checks of retrieval_rank for a sibling entry: fp32 [Nq, D] / [Nk, D], row-major views with a leading dimension kept."""
    if q.dtype != torch.float32 or k.dtype != torch.float32 or q.dim() != 2 or k.dim() != 2 or q.shape[1] != k.shape[1]:
        raise ValueError(f"{name}: fp32 [Nq, D] and [Nk, D] rows expected, got {q.dtype}{tuple(q.shape)} and {k.dtype}{tuple(k.shape)}")
    if q.stride(1) != 1 or q.stride(0) < q.shape[1]:
        q = q.contiguous()
    if k.stride(1) != 1 or k.stride(0) < k.shape[1]:
        k = k.contiguous()
    if min(q.shape[0], k.shape[0], q.shape[1]) < 1:
        raise ValueError(f"{name}: empty operand (Nq={q.shape[0]}, Nk={k.shape[0]}, D={q.shape[1]})")
    return q, k


def _rr_index(name: str, what: str, t: Tensor, Nq: int) -> Tensor:
    if t.shape != (Nq,):
        raise ValueError(f"{name}: {what} must have shape ({Nq},), got {tuple(t.shape)}")
    if t.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name}: {what} must be int32 or int64 indices, got {t.dtype}")
    return t


def retrieval_rank_windowed(q: Tensor, k: Tensor, key_lo: Tensor, key_hi: Tensor, target: Optional[Tensor] = None):
    """retrieval_rank with a key window per query: (rank, best_idx, best_val, pos_val), each [Nq], where query i competes only with the keys
    key_lo[i] <= j < key_hi[i] -- rank[i] is the place of key target[i] (default: i) among them, best_* the window's maximum and its first
    (global) index, pos_val the positive's score.  The scores are bitwise those of retrieval_rank; a strip of queries sweeps only the key
    tiles its windows touch, so rows sorted by group cost sum n_g^2 scores (csrc/retrieval.hip).  Window bounds outside [0, Nk] are clamped by
    the kernel and are no error; an empty window gives rank 0, best_idx 0x7fffffff, best_val -inf; a target outside its window is allowed.
    target indices are checked against [0, Nk) here.  See include/dinox.h."""
    _need_cuda(q, k, key_lo, key_hi, target)
    name = "retrieval_rank_windowed"
    q, k = _rr_rows(name, q, k)
    (Nq, D), Nk = q.shape, k.shape[0]
    key_lo, key_hi = _rr_index(name, "key_lo", key_lo, Nq), _rr_index(name, "key_hi", key_hi, Nq)
    # int64 bounds beyond int32 are clamped here the way the kernel clamps the rest
    key_lo, key_hi = _c(key_lo.clamp(0, Nk).to(torch.int32)), _c(key_hi.clamp(0, Nk).to(torch.int32))
    if target is None:
        if Nq != Nk:
            raise ValueError(f"{name}: without target, query i is matched to key i and Nq must equal Nk ({Nq}, {Nk})")
    else:
        target = _rr_index(name, "target", target, Nq)
        lo, hi = int(target.min()), int(target.max())
        if lo < 0 or hi >= Nk:
            raise ValueError(f"{name}: target indices must lie in [0, {Nk}), got [{lo}, {hi}]")
        target = _c(target.to(torch.int32))
    dev = q.device
    rank = torch.empty(Nq, dtype=torch.int32, device=dev)
    best_idx = torch.empty(Nq, dtype=torch.int32, device=dev)
    best_val = torch.empty(Nq, dtype=torch.float32, device=dev)
    pos_val = torch.empty(Nq, dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib.dinox_retrieval_rank_windowed_ws_bytes(Nq, Nk, D)), dtype=torch.uint8, device=dev)
    check(lib.dinox_retrieval_rank_windowed(_p(q), q.stride(0), _p(k), k.stride(0), _p(target), _p(key_lo), _p(key_hi), Nq, Nk, D, _p(rank),
                                            _p(best_idx), _p(best_val), _p(pos_val), _p(ws), _stream()), "dinox_retrieval_rank_windowed")
    return rank, best_idx, best_val, pos_val


def row_dots(a: Tensor, b: Tensor) -> Tensor:
    """out[i] = a_i . b_i of fp32 rows a, b [N, D], fp32 [N]: bitwise ``retrieval_rank(a, b)[3]`` (the positive's score of query a_i against
    key b_i) from that entry's first launch alone -- no workspace, no sweep.  Row-major views with a leading dimension are accepted."""
    _need_cuda(a, b)
    a, b = _rr_rows("row_dots", a, b)
    if a.shape != b.shape:
        raise ValueError(f"row_dots: rows are paired and the shapes must be equal, got {tuple(a.shape)} and {tuple(b.shape)}")
    N, D = a.shape
    out = torch.empty(N, dtype=torch.float32, device=a.device)
    check(lib.dinox_row_dots(_p(a), a.stride(0), _p(b), b.stride(0), N, D, _p(out), _stream()), "dinox_row_dots")
    return out


KNN_MAX_K = 32


def knn_topk(q: Tensor, k: Tensor, K: int, exclude=None):
    """(idx int32 [Nq, K], val fp32 [Nq, K]): for each fp32 query row of q [Nq, D], the K keys of k [Nk, D] with the highest scores q_i . k_j,
    ordered by (score descending, index ascending); key ``exclude[i]`` is left out of row i (``exclude="self"`` = arange(Nq), needs
    Nq == Nk: the self-exclusion of a set searched against itself; -1 or any index outside [0, Nk) leaves nothing out).  With fewer than K
    eligible keys the remaining slots hold index -1 and value -inf.  1 <= K <= 32.  The scores are the ones ``retrieval_rank`` sees (same
    sweep, csrc/knn.hip): column 0 is bitwise its best_idx / best_val.  No Nq x Nk tensor is allocated; the workspace is 8 K bytes per query
    and key split.  Rows are used as given (normalise them first: normalize_rows); rows that meet NaN scores: see include/dinox.h.
    Arguments are checked before the device is: a wrong call raises ValueError anywhere."""
    if not (isinstance(q, Tensor) and isinstance(k, Tensor)) or q.dtype != torch.float32 or k.dtype != torch.float32 or q.dim() != 2 \
            or k.dim() != 2 or q.shape[1] != k.shape[1]:
        raise ValueError("knn_topk: fp32 [Nq, D] and [Nk, D] rows expected, got "
                         + " and ".join(f"{t.dtype}{tuple(t.shape)}" if isinstance(t, Tensor) else type(t).__name__ for t in (q, k)))
    (Nq, D), Nk = q.shape, k.shape[0]
    if min(Nq, Nk, D) < 1:
        raise ValueError(f"knn_topk: empty operand (Nq={Nq}, Nk={Nk}, D={D})")
    if q.device != k.device:
        raise ValueError(f"knn_topk: queries on {q.device}, keys on {k.device}")
    K_given = K
    try:
        K = None if isinstance(K, bool) else operator.index(K)                 # Python and NumPy integers; not bool, not float
    except TypeError:
        K = None
    if K is None or not 1 <= K <= KNN_MAX_K:
        raise ValueError(f"knn_topk: K must be an integer in [1, {KNN_MAX_K}], got {K_given!r} (q {tuple(q.shape)}, k {tuple(k.shape)})")
    if isinstance(exclude, str):
        if exclude != "self":
            raise ValueError(f"knn_topk: exclude must be None, 'self' or an index tensor of shape ({Nq},), got {exclude!r}")
        if Nq != Nk:
            raise ValueError(f"knn_topk: exclude='self' leaves key i out of row i and needs Nq == Nk ({Nq}, {Nk})")
        exclude = torch.arange(Nq, dtype=torch.int32, device=q.device)
    elif exclude is not None:
        if not isinstance(exclude, Tensor) or exclude.shape != (Nq,):
            raise ValueError(f"knn_topk: exclude must have shape ({Nq},), got {tuple(getattr(exclude, 'shape', ()))}")
        if exclude.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"knn_topk: exclude must be int32 or int64 indices, got {exclude.dtype}")
        if exclude.device != q.device:
            raise ValueError(f"knn_topk: queries on {q.device}, exclude on {exclude.device}")
    _need_cuda(q, k, exclude)
    if exclude is not None and exclude.dtype != torch.int32:
        exclude = torch.where((exclude >= 0) & (exclude < Nk), exclude, torch.full_like(exclude, -1)).to(torch.int32)   # (no wrap-around into range)
    if exclude is not None:
        exclude = _c(exclude)
    if q.stride(1) != 1 or q.stride(0) < D:
        q = q.contiguous()
    if k.stride(1) != 1 or k.stride(0) < D:
        k = k.contiguous()
    dev = q.device
    idx = torch.empty((Nq, K), dtype=torch.int32, device=dev)
    val = torch.empty((Nq, K), dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib.dinox_knn_ws_bytes(Nq, Nk, D, K)), dtype=torch.uint8, device=dev)
    check(lib.dinox_knn_topk(_p(q), q.stride(0), _p(k), k.stride(0), _p(exclude), Nq, Nk, D, K, _p(idx), _p(val), _p(ws), _stream()),
          "dinox_knn_topk")
    return idx, val


LABELPROP_MIN_C, LABELPROP_MAX_C = 2, 64


def _lp_int(name: str, what: str, v, lo: int, hi: Optional[int] = None) -> int:
    try:
        n = None if isinstance(v, bool) else operator.index(v)                 # Python and NumPy integers; not bool, not float
    except TypeError:
        n = None
    if n is None or n < lo or (hi is not None and n > hi):
        rng = f"in [{lo}, {hi}]" if hi is not None else f">= {lo}"
        raise ValueError(f"{name}: {what} must be an integer {rng}, got {v!r}")
    return n


def label_propagate(q: Tensor, k: Tensor, seg: Tensor, g: int, K: int = 5, radius: int = 12, temperature: float = 0.1):
    """One step of dense label propagation (csrc/labelprop.hip; definitions in include/dinox.h): for each of the N = g g fp32 patch rows of
    q [N, D], the K best-matching rows of k [F N, D] -- the patches of F context slots, key j = f N + y' g + x' -- among those within
    ``radius`` patches in y and in x (radius < 0 or >= g - 1: the whole grid), then the softmax-weighted vote
    out[p] = sum_i w_i seg[j_i] / sum_i w_i with w_i = exp((s_i - s_1) / temperature) over their soft labels seg [F N, C].  Returns
    (out fp32 [N, C], idx int32 [N, K], val fp32 [N, K]); idx / val are ordered by (score descending, index ascending) and are bitwise
    ``knn_topk(q, k, K)`` for a whole-grid radius; slots past the candidates hold (-1, -inf), and a row without candidates votes zero.
    out is not renormalised over the classes.  Rows are used as given (normalise them first: normalize_rows).  Row-major views with a
    leading dimension are accepted for q and k.  Arguments are checked before the device is: a wrong call raises ValueError anywhere."""
    name = "label_propagate"
    if not all(isinstance(t, Tensor) for t in (q, k, seg)) or any(t.dtype != torch.float32 or t.dim() != 2 for t in (q, k, seg)) \
            or q.shape[1] != k.shape[1] or k.shape[0] != seg.shape[0]:
        raise ValueError(f"{name}: fp32 q [N, D], k [F N, D] and seg [F N, C] expected, got {_describe(q, k, seg)}")
    g = _lp_int(name, "g", g, 1)
    K = _lp_int(name, "K", K, 1, KNN_MAX_K)
    radius = _lp_int(name, "radius", radius, -(1 << 31), (1 << 31) - 1)
    (N, D), Nk, C = q.shape, k.shape[0], seg.shape[1]
    if N != g * g:
        raise ValueError(f"{name}: q has {N} rows, the grid g = {g} has g g = {g * g} patches")
    if D < 1:
        raise ValueError(f"{name}: empty feature rows (D = {D})")
    if Nk < N or Nk % N != 0:
        raise ValueError(f"{name}: k has {Nk} rows, which is not F >= 1 times the N = {N} patches of a slice")
    if not LABELPROP_MIN_C <= C <= LABELPROP_MAX_C:
        raise ValueError(f"{name}: seg has C = {C} classes, outside [{LABELPROP_MIN_C}, {LABELPROP_MAX_C}]")
    if Nk > 0x7fffffff - 128:
        raise ValueError(f"{name}: F N = {Nk} keys exceed 2^31 - 129")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature) or temperature <= 0:
        raise ValueError(f"{name}: temperature must be a finite number > 0, got {temperature!r}")
    inv_t = float(torch.tensor(1.0 / float(temperature), dtype=torch.float32))
    if not (math.isfinite(inv_t) and inv_t > 0):
        raise ValueError(f"{name}: 1 / temperature = {inv_t} is not a finite positive fp32 number (temperature {temperature!r})")
    if not (q.device == k.device == seg.device):
        raise ValueError(f"{name}: q on {q.device}, k on {k.device}, seg on {seg.device}")
    _need_cuda(q, k, seg)
    if q.stride(1) != 1 or q.stride(0) < D:
        q = q.contiguous()
    if k.stride(1) != 1 or k.stride(0) < D:
        k = k.contiguous()
    seg = _c(seg)
    F, dev = Nk // N, q.device
    out = torch.empty((N, C), dtype=torch.float32, device=dev)
    idx = torch.empty((N, K), dtype=torch.int32, device=dev)
    val = torch.empty((N, K), dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib.dinox_labelprop_ws_bytes(g, F, D, C, K)), dtype=torch.uint8, device=dev)
    check(lib.dinox_labelprop(_p(q), q.stride(0), _p(k), k.stride(0), _p(seg), g, F, D, C, K, radius, inv_t, _p(out), _p(idx), _p(val),
                              _p(ws), _stream()), "dinox_labelprop")
    return out, idx, val


# ------------------------------------------------------------------------------------------
# probes (csrc/gram.hip, csrc/probe.hip)
# ------------------------------------------------------------------------------------------
GRAM_MAX_D = 1024
PROBE_MAX_C = 32


def _describe(*ts) -> str:
    return " and ".join(f"{t.dtype}{tuple(t.shape)}" if isinstance(t, Tensor) else type(t).__name__ for t in ts)


def _rows_operand(x: Tensor, D: int) -> Tensor:
    return x if x.stride(1) == 1 and x.stride(0) >= D else x.contiguous()


def gram(x: Tensor, shift: Optional[Tensor] = None):
    """(gram float64 [D, D], colsum float64 [D]) of the fp32 rows x [N, D]: with z_i = x_i - shift (one fp32 subtraction per element;
    ``shift`` fp32 [D] or None), gram = sum_i z_i z_i^T and colsum = sum_i z_i.  Exact-fp32 MFMA products over a deterministic split of
    the rows, the splits summed in double (csrc/gram.hip): |error of gram[a, b]| <= N 2^-24 sum_i |z_ia z_ib|, bit-reproducible and
    symmetric to the bit.  1 <= D <= 1024.  Append a target column to x to get X^T y and y^T y from the same pass.
    Arguments are checked before the device is: a wrong call raises ValueError anywhere."""
    if not isinstance(x, Tensor) or x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError(f"gram: fp32 [N, D] rows expected, got {_describe(x)}")
    N, D = x.shape
    if N < 1 or not 1 <= D <= GRAM_MAX_D:
        raise ValueError(f"gram: needs N >= 1 and 1 <= D <= {GRAM_MAX_D}, got N={N}, D={D}")
    if shift is not None:
        if not isinstance(shift, Tensor) or shift.dtype != torch.float32 or shift.shape != (D,):
            raise ValueError(f"gram: shift must be fp32 of shape ({D},), got {_describe(shift)}")
        if shift.device != x.device:
            raise ValueError(f"gram: rows on {x.device}, shift on {shift.device}")
    _need_cuda(x, shift)
    x = _rows_operand(x, D)
    if shift is not None:
        shift = _c(shift)
    dev = x.device
    g = torch.empty((D, D), dtype=torch.float64, device=dev)
    cs = torch.empty(D, dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.dinox_gram_ws_bytes(N, D)), dtype=torch.uint8, device=dev)
    check(lib.dinox_gram_f32(_p(x), x.stride(0), N, D, _p(shift), _p(g), _p(cs), _p(ws), _stream()), "dinox_gram_f32")
    return g, cs


def softmax_probe(x: Tensor, label: Tensor, theta: Tensor, *, want_grad: bool = True, want_prob: bool = False):
    """One evaluation of a softmax (multinomial logistic) probe on the fp32 rows x [N, D] with int labels [N] and fp32 parameters
    theta [C, D + 1] (last column = intercept): returns (loss, grad, prob) with loss = sum_i (logsumexp(z_i) - z_i,label_i) as a float64
    0-d tensor, grad = sum_i (p_i - onehot_i) [x_i, 1]^T float64 [C, D + 1] (both None without ``want_grad``) and prob = softmax(z) fp32
    [N, C] (None without ``want_prob``).  ``want_grad=False, want_prob=True`` is the predict form; the probabilities are bitwise the same
    in both forms.  A row whose label is outside [0, C) contributes nothing to loss and grad.  2 <= C <= 32, 1 <= D <= 1024.  One pass
    over x on the exact-fp32 MFMA, deterministic reduction in double (csrc/probe.hip).
    Arguments are checked before the device is: a wrong call raises ValueError anywhere."""
    if not isinstance(x, Tensor) or x.dtype != torch.float32 or x.dim() != 2:
        raise ValueError(f"softmax_probe: fp32 [N, D] rows expected, got {_describe(x)}")
    N, D = x.shape
    if N < 1 or not 1 <= D <= GRAM_MAX_D:
        raise ValueError(f"softmax_probe: needs N >= 1 and 1 <= D <= {GRAM_MAX_D}, got N={N}, D={D}")
    if not isinstance(theta, Tensor) or theta.dtype != torch.float32 or theta.dim() != 2 or theta.shape[1] != D + 1:
        raise ValueError(f"softmax_probe: theta must be fp32 [C, {D + 1}] (last column = intercept), got {_describe(theta)}")
    C = theta.shape[0]
    if not 2 <= C <= PROBE_MAX_C:
        raise ValueError(f"softmax_probe: C must lie in [2, {PROBE_MAX_C}], got {C}")
    if not isinstance(label, Tensor) or label.shape != (N,) or label.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"softmax_probe: label must be int32 or int64 of shape ({N},), got {_describe(label)}")
    if not (want_grad or want_prob):
        raise ValueError("softmax_probe: nothing asked for (want_grad=False, want_prob=False)")
    if label.device != x.device or theta.device != x.device:
        raise ValueError(f"softmax_probe: rows on {x.device}, label on {label.device}, theta on {theta.device}")
    _need_cuda(x, label, theta)
    if label.dtype != torch.int32:
        label = torch.where((label >= 0) & (label < C), label, torch.full_like(label, -1)).to(torch.int32)     # (no wrap-around into range)
    x, label, theta = _rows_operand(x, D), _c(label), _c(theta)
    dev = x.device
    loss = torch.empty((), dtype=torch.float64, device=dev) if want_grad else None
    grad = torch.empty((C, D + 1), dtype=torch.float64, device=dev) if want_grad else None
    prob = torch.empty((N, C), dtype=torch.float32, device=dev) if want_prob else None
    ws = torch.empty(int(lib.dinox_softmax_probe_ws_bytes(N, D, C)) // 8 + 1, dtype=torch.float64, device=dev)
    check(lib.dinox_softmax_probe(_p(x), x.stride(0), _p(label), N, D, C, _p(theta), _p(loss), _p(grad), _p(prob), _p(ws), _stream()),
          "dinox_softmax_probe")
    return loss, grad, prob


# ------------------------------------------------------------------------------------------
# dense segmentation on patch logits (csrc/segloss.hip)
# ------------------------------------------------------------------------------------------
SEG_MAX_CLASSES = 64
SEG_MAX_UPSAMPLE = 32
SEG_IGNORE = 255


def _seg_geometry(name: str, z: Tensor, u: int):
    """(B, g, C) of patch logits z [B, g^2, C] for an integer upsampling factor u; ValueError for anything the kernels do not take."""
    if not isinstance(z, Tensor) or z.dim() != 3 or not z.is_floating_point():
        raise ValueError(f"{name}: patch logits must be a floating-point [B, P, C] tensor, got {_describe(z)}")
    B, P, C = z.shape
    g = math.isqrt(P)
    if B < 1 or P < 1 or g * g != P:
        raise ValueError(f"{name}: P = {P} patches are not a square grid (z is {tuple(z.shape)})")
    if isinstance(u, bool) or not isinstance(u, int) or not 1 <= u <= SEG_MAX_UPSAMPLE:
        raise ValueError(f"{name}: the upsampling factor must be an integer in [1, {SEG_MAX_UPSAMPLE}], got {u!r}")
    if not 2 <= C <= SEG_MAX_CLASSES:
        raise ValueError(f"{name}: C must lie in [2, {SEG_MAX_CLASSES}], got {C}")
    return B, g, C


def _seg_labels(name: str, y, B: int, g: int, z: Tensor) -> int:
    """The upsampling factor u of a uint8 label map [B, S, S] with S = g u."""
    if not isinstance(y, Tensor) or y.dtype != torch.uint8 or y.dim() != 3 or y.shape[0] != B or y.shape[1] != y.shape[2]:
        raise ValueError(f"{name}: labels must be uint8 [{B}, S, S] (255 = ignore), got {_describe(y)}")
    S = y.shape[1]
    if S < g or S % g or S // g > SEG_MAX_UPSAMPLE:
        raise ValueError(f"{name}: label side {S} is not {g} patches times an integer factor in [1, {SEG_MAX_UPSAMPLE}]")
    if y.device != z.device:
        raise ValueError(f"{name}: logits on {z.device}, labels on {y.device}")
    return S // g


def _seg_refuse_bad_labels(name: str, bad: int, C: int) -> None:
    if bad:
        raise ValueError(f"{name}: {bad} label(s) are >= C = {C} and not {SEG_IGNORE} (ignore)")


def seg_loss_fwd(z: Tensor, y: Tensor, w_ce: float = 1.0, w_dice: float = 1.0, c0: int = 0):
    """Cross-entropy + soft Dice of the patch logits z [B, g^2, C] against the uint8 label map y [B, S, S] (S = g u, 255 = ignore) at full
    resolution, the logits upsampled bilinearly (align_corners=False) inside the kernel (include/dinox.h has the definitions).  Returns
    (loss[3] = (L, CE, Dice) fp32 on the device, stats [3, C] = (I, P, Y), saved); seg_loss_bwd(saved, gscale) gives d(gscale L)/dz.
    A label >= C other than 255 raises ValueError (one device read of two integers)."""
    B, g, C = _seg_geometry("seg_loss", z, 1)
    u = _seg_labels("seg_loss", y, B, g, z)
    if c0 not in (0, 1):
        raise ValueError(f"seg_loss: c0 must be 0 or 1, got {c0!r}")
    _need_cuda(z, y)
    z, y = _c(z.float()), _c(y)
    dev = z.device
    loss = torch.empty(3, dtype=torch.float32, device=dev)
    stats = torch.empty((3, C), dtype=torch.float32, device=dev)
    nv = torch.empty(2, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.dinox_seg_loss_ws_bytes(B, g, u, C)) // 4, dtype=torch.float32, device=dev)
    check(lib.dinox_seg_loss_fwd(_p(z), _p(y), _p(loss), _p(stats), _p(nv), _p(ws), B, g, u, C, int(c0), float(w_ce), float(w_dice), _stream()),
          "dinox_seg_loss_fwd")
    _seg_refuse_bad_labels("seg_loss", int(nv[1]), C)
    return loss, stats, (z, y, stats, nv, ws, (B, g, u, C, int(c0), float(w_ce), float(w_dice)))


def seg_loss_bwd(saved, gscale: float = 1.0) -> Tensor:
    """dz [B, g^2, C] fp32 = d(gscale L)/dz: each patch gathers the pixels it was interpolated into, in a fixed order."""
    z, y, stats, nv, ws, (B, g, u, C, c0, w_ce, w_dice) = saved
    dz = torch.empty_like(z)
    check(lib.dinox_seg_loss_bwd(_p(z), _p(y), _p(stats), _p(nv), _p(dz), _p(ws), B, g, u, C, c0, w_ce, w_dice, float(gscale), _stream()),
          "dinox_seg_loss_bwd")
    return dz


class SegLossFn(torch.autograd.Function):
    """(z, y, w_ce, w_dice, c0) -> (L, CE, Dice) as 0-d tensors; the backward takes the upstream gradient of L only (CE and Dice are
    reported values).  z of any floating dtype is cast to fp32."""

    @staticmethod
    def forward(ctx, z, y, w_ce=1.0, w_dice=1.0, c0=0):
        loss, _, saved = seg_loss_fwd(z, y, w_ce, w_dice, c0)
        ctx.saved, ctx.zdt = saved, z.dtype
        total, ce, dice = (loss[i].clone() for i in range(3))
        ctx.mark_non_differentiable(ce, dice)
        return total, ce, dice

    @staticmethod
    def backward(ctx, g, *_reported):
        # the upstream gradient is a device scalar: run with gscale = 1 and scale the small [B, P, C] result (no host sync)
        d = seg_loss_bwd(ctx.saved, 1.0) * g
        return (d if d.dtype == ctx.zdt else d.to(ctx.zdt)), None, None, None, None


def seg_predict(z: Tensor, u: int, labels: Optional[Tensor] = None):
    """Label map of the patch logits z [B, g^2, C] at S = g u: pred uint8 [B, S, S] = argmax of the bilinearly upsampled logits (lowest
    index on an exact tie).  With ``labels`` (uint8 [B, S, S], 255 = ignore) returns (pred, counts): counts int64 [3, C] = true positives,
    predicted pixels and labelled pixels per class over the valid pixels (dinox.segment turns them into Dice / IoU / accuracy)."""
    B, g, C = _seg_geometry("seg_predict", z, u)
    if labels is not None and _seg_labels("seg_predict", labels, B, g, z) != u:
        raise ValueError(f"seg_predict: labels {tuple(labels.shape)} do not have side g u = {g * u}")
    _need_cuda(z, labels)
    z = _c(z.float())
    dev = z.device
    pred = torch.empty((B, g * u, g * u), dtype=torch.uint8, device=dev)
    counts = None
    if labels is not None:
        labels = _c(labels)
        counts = torch.empty(3 * C + 1, dtype=torch.int64, device=dev)
    check(lib.dinox_seg_predict(_p(z), _p(labels), _p(pred), _p(counts), B, g, u, C, _stream()), "dinox_seg_predict")
    if counts is None:
        return pred
    _seg_refuse_bad_labels("seg_predict", int(counts[3 * C]), C)
    return pred, counts[:3 * C].view(3, C)


# ------------------------------------------------------------------------------------------
# calibration of the upsampled softmax: confidence, entropy, reliability histogram, NLL / Brier / Newton sums (csrc/segcalib.hip)
# ------------------------------------------------------------------------------------------
SEG_CALIB_MAX_BINS = 64


class SegCalib(NamedTuple):
    """What ``seg_calib`` returns.  ``pred`` uint8, ``conf`` and ``entropy`` fp32 [B, S, S] (None where not asked for); with labels
    ``hist`` int64 [NB, 3] = per bin (count, correct, Q: the confidences in 2^-24 fixed point), ``tail`` int64 [3] = (valid pixels, labels
    >= C other than 255 -- always 0 here, such labels raise --, valid pixels whose confidence is not finite) and ``sums`` fp32 [5] = (NLL,
    Brier, G = dNLL/ds, H = d2NLL/ds2, entropy) totals over the valid pixels with finite confidence; None without labels."""
    pred: Optional[Tensor]
    conf: Optional[Tensor]
    entropy: Optional[Tensor]
    hist: Optional[Tensor]
    tail: Optional[Tensor]
    sums: Optional[Tensor]


def seg_calib(z: Tensor, u: int, labels: Optional[Tensor] = None, *, inv_temperature: float = 1.0, bins: int = 15, want_pred: bool = True,
              want_conf: bool = False, want_entropy: bool = False) -> SegCalib:
    """One launch over the patch logits z [B, g^2, C] at S = g u (include/dinox.h has the definitions): the arg-max map of ``seg_predict``
    (bit for bit, whatever the temperature), the confidence p[pred] and the normalised entropy of softmax(inv_temperature * l), and with
    ``labels`` (uint8 [B, S, S], 255 = ignore) the reliability histogram over ``bins`` equal-width confidence bins and the five sums.
    Nothing of full resolution is allocated but the maps asked for.  A label >= C other than 255 raises the ValueError of ``seg_predict``
    (one device read)."""
    B, g, C = _seg_geometry("seg_calib", z, u)
    if labels is not None and _seg_labels("seg_calib", labels, B, g, z) != u:
        raise ValueError(f"seg_calib: labels {tuple(labels.shape)} do not have side g u = {g * u}")
    if isinstance(bins, bool) or not isinstance(bins, int) or not 1 <= bins <= SEG_CALIB_MAX_BINS:
        raise ValueError(f"seg_calib: bins must be an integer in [1, {SEG_CALIB_MAX_BINS}], got {bins!r}")
    s = float(inv_temperature)
    if not (s > 0 and math.isfinite(s) and math.isfinite(float(np.float32(s))) and float(np.float32(s)) > 0):
        raise ValueError(f"seg_calib: inv_temperature must be finite and > 0 (in fp32), got {inv_temperature!r}")
    if labels is None and not (want_pred or want_conf or want_entropy):
        raise ValueError("seg_calib: nothing to compute (no labels and no map asked for)")
    _need_cuda(z, labels)
    z = _c(z.float())
    dev = z.device
    S = g * u
    pred = torch.empty((B, S, S), dtype=torch.uint8, device=dev) if want_pred else None
    conf = torch.empty((B, S, S), dtype=torch.float32, device=dev) if want_conf else None
    ent = torch.empty((B, S, S), dtype=torch.float32, device=dev) if want_entropy else None
    hist = sums = ws = None
    if labels is not None:
        labels = _c(labels)
        hist = torch.empty(3 * bins + 3, dtype=torch.int64, device=dev)
        sums = torch.empty(5, dtype=torch.float32, device=dev)
        ws = torch.empty(int(lib.dinox_seg_calib_ws_bytes(B, g, u, C, bins)) // 4, dtype=torch.float32, device=dev)
    check(lib.dinox_seg_calib(_p(z), _p(labels), s, _p(pred), _p(conf), _p(ent), _p(hist), _p(sums), _p(ws), B, g, u, C, bins, _stream()),
          "dinox_seg_calib")
    if hist is None:
        return SegCalib(pred, conf, ent, None, None, None)
    tail = hist[3 * bins:]
    _seg_refuse_bad_labels("seg_calib", int(tail[1]), C)
    return SegCalib(pred, conf, ent, hist[:3 * bins].view(bins, 3), tail, sums)


# ------------------------------------------------------------------------------------------
# edge-aware refinement of the upsampled softmax: mean-field iterations of a local CRF on a guide image (csrc/segrefine.hip)
# ------------------------------------------------------------------------------------------
SEG_REFINE_MAX_ITERS = 32
SEG_REFINE_MAX_RADIUS = 3
SEG_REFINE_MAX_DILATION = 8


def seg_refine_table(radius: int, dilation: int, sigma_xy: float) -> np.ndarray:
    """The spatial weights g_(dy,dx) = exp(-(dy^2 + dx^2) d^2 / (2 sigma_xy^2)) of the (2r+1)^2 window, row-major, computed in float64
    and rounded to fp32 (the centre entry is never read)."""
    o = np.arange(-radius, radius + 1, dtype=np.float64)
    return np.exp(-(o[:, None] ** 2 + o[None, :] ** 2) * float(dilation) ** 2 / (2.0 * float(sigma_xy) ** 2)).astype(np.float32).reshape(-1)


def _seg_refine_number(what: str, v, lo_open: bool) -> float:
    """v as a float that is finite in fp32 and > 0 (lo_open) or >= 0."""
    ok = isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and math.isfinite(float(np.float32(v)))
    if not ok or (float(np.float32(v)) <= 0 if lo_open else v < 0):
        raise ValueError(f"seg_refine: {what} must be finite and {'> 0 (in fp32)' if lo_open else '>= 0'}, got {v!r}")
    return float(v)


def seg_refine(z: Tensor, guide: Tensor, u: int, labels: Optional[Tensor] = None, *, iters: int = 5, radius: int = 2, dilation: int = 2,
               sigma_xy: float = 3.0, sigma_i: float = 0.5, mix: float = 0.8, weight: float = 4.0, inv_temperature: float = 1.0,
               want_conf: bool = False):
    """Edge-aware refinement of the label map of the patch logits z [B, g^2, C] at S = g u (include/dinox.h has the definition): ``iters``
    mean-field iterations of a local CRF whose unary term is ``inv_temperature`` times the upsampled logits and whose messages come from
    the (2 radius + 1)^2 window at ``dilation``, weighted by exp(-dist^2 / (2 sigma_xy^2)) in pixels and by (1 - mix) + mix
    exp(-(I_p - I_j)^2 / (2 sigma_i^2)) on the fp32 ``guide`` [B, S, S]; ``weight`` scales the message.  Returns (pred uint8 [B, S, S],
    conf fp32 [B, S, S] or None, counts int64 [3, C] or None): the arg-max after the last iteration, its probability (``want_conf``) and,
    with ``labels`` (uint8 [B, S, S], 255 = ignore), ``seg_predict``'s counts of the refined map.  ``iters = 0`` gives ``seg_predict``'s
    map and counts and ``seg_calib``'s confidence bit for bit.  The workspace (two fp32 planes [B, C, S, S]) lives for the call only."""
    B, g, C = _seg_geometry("seg_refine", z, u)
    S = g * u
    if labels is not None and _seg_labels("seg_refine", labels, B, g, z) != u:
        raise ValueError(f"seg_refine: labels {tuple(labels.shape)} do not have side g u = {S}")
    if not isinstance(guide, Tensor) or guide.dtype != torch.float32 or tuple(guide.shape) != (B, S, S):
        raise ValueError(f"seg_refine: the guide must be fp32 [{B}, {S}, {S}], got {_describe(guide)}")
    if guide.device != z.device:
        raise ValueError(f"seg_refine: logits on {z.device}, guide on {guide.device}")
    for name, v, top in (("iters", iters, SEG_REFINE_MAX_ITERS), ("radius", radius, SEG_REFINE_MAX_RADIUS), ("dilation", dilation, SEG_REFINE_MAX_DILATION)):
        lo = 0 if name == "iters" else 1
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= top:
            raise ValueError(f"seg_refine: {name} must be an integer in [{lo}, {top}], got {v!r}")
    if radius * dilation >= S:
        raise ValueError(f"seg_refine: radius * dilation = {radius * dilation} reaches across the image side {S}: no neighbour is left")
    if 2 * dilation > S:
        raise ValueError(f"seg_refine: dilation = {dilation} leaves the pixels in the middle of an image of side {S} no neighbour "
                         f"(2 * dilation <= side)")
    sigma_xy = _seg_refine_number("sigma_xy", sigma_xy, True)
    sigma_i = _seg_refine_number("sigma_i", sigma_i, True)
    weight = _seg_refine_number("weight", weight, False)
    s = _seg_refine_number("inv_temperature", inv_temperature, True)
    if isinstance(mix, bool) or not isinstance(mix, (int, float)) or not 0.0 <= mix <= 1.0:
        raise ValueError(f"seg_refine: mix must lie in [0, 1], got {mix!r}")
    gtab = seg_refine_table(radius, dilation, sigma_xy)
    if not (gtab[2 * radius * (radius + 1) + 1] > 0):                         # the neighbour at (0, +1): the largest entry off the centre
        raise ValueError(f"seg_refine: sigma_xy = {sigma_xy!r} is so small against dilation = {dilation} that every spatial weight is 0 in fp32")
    inv2 = 1.0 / (2.0 * sigma_i * sigma_i)
    if not inv2 <= float(np.finfo(np.float32).max):
        raise ValueError(f"seg_refine: sigma_i = {sigma_i!r}: 1 / (2 sigma_i^2) is not finite in fp32")
    _need_cuda(z, guide, labels)
    z, guide = _c(z.float()), _c(guide)
    dev = z.device
    pred = torch.empty((B, S, S), dtype=torch.uint8, device=dev)
    conf = torch.empty((B, S, S), dtype=torch.float32, device=dev) if want_conf else None
    counts = None
    if labels is not None:
        labels = _c(labels)
        counts = torch.empty(3 * C + 1, dtype=torch.int64, device=dev)
    nbytes = int(lib.dinox_seg_refine_ws_bytes(B, g, u, C))
    if nbytes <= 0:
        raise ValueError(f"seg_refine: B = {B}, S = {S}, C = {C} is beyond the sizes the kernel takes")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev) if iters > 0 else None
    check(lib.dinox_seg_refine(_p(z), _p(guide), _p(labels), _p(pred), _p(conf), _p(counts), _p(ws), B, g, u, C, iters, radius, dilation,
                               gtab.ctypes.data, inv2, float(mix), weight, s, _stream()), "dinox_seg_refine")
    if counts is None:
        return pred, conf, None
    _seg_refuse_bad_labels("seg_refine", int(counts[3 * C]), C)
    return pred, conf, counts[:3 * C].view(3, C)


# ------------------------------------------------------------------------------------------
# sliding-window prediction: the blend of overlapping tiles' patch logits (csrc/segblend.hip)
# ------------------------------------------------------------------------------------------
SEG_BLEND_MAX_FLIPS = 4


def _host_table(name: str, what: str, v, dtype) -> np.ndarray:
    """A 1-D host copy of a small table given as a sequence, an ndarray or a tensor (a device tensor costs one read)."""
    a = v.detach().cpu().numpy() if isinstance(v, Tensor) else np.asarray(v)
    if a.ndim != 1 or a.size < 1 or a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) if dtype == np.int32
                                                                 else np.issubdtype(a.dtype, np.floating)):
        raise ValueError(f"{name}: {what} must be a 1-D, non-empty {'integer' if dtype == np.int32 else 'floating-point'} table, got "
                         f"{a.dtype} {a.shape}")
    if dtype == np.int32 and (np.abs(a.astype(np.int64)) >= 1 << 31).any():
        raise ValueError(f"{name}: {what} holds a value outside int32")
    return np.ascontiguousarray(a, dtype=dtype)


def _seg_blend_origins(name: str, what: str, o: np.ndarray, L: int, t: int) -> None:
    """Tile origins along one axis of length L: strictly ascending, from 0 to L - t, no step above t (so every pixel is covered)."""
    if int(o[0]) != 0 or int(o[-1]) != L - t:
        raise ValueError(f"{name}: {what} must start at 0 and end at {L} - {t} = {L - t} to cover the image, got {o[0]} .. {o[-1]}")
    d = np.diff(o.astype(np.int64))
    if (d <= 0).any():
        raise ValueError(f"{name}: {what} must be strictly ascending")
    if (d > t).any():
        raise ValueError(f"{name}: {what} leave a gap: consecutive origins {int(d.max())} apart with tiles of side {t}")


def seg_blend_predict(z: Tensor, ys, xs, flips, win, H: int, W: int, t: int, labels: Optional[Tensor] = None, want_conf: bool = False):
    """Label map of B images of size H x W from the patch logits of their overlapping tiles, z [B, F, ny, nx, g^2, C]: tile (iy, ix) is
    the t x t crop at (ys[iy], xs[ix]), variant f saw it mirrored along x (``flips[f] & 1``) and / or y (``& 2``).  Every pixel blends
    the bilinearly upsampled logits (align_corners=False, any t) of the tiles that cover it with weights ``win[ly] win[lx]`` -- ``win``
    fp32 [t], e.g. ``dinox.tiled.blend_window`` -- and takes the arg-max (lowest index on a tie); include/dinox.h has the definitions.
    ``ys``, ``xs``, ``flips`` and ``win`` are small host tables (sequences, ndarrays or tensors); they are checked here -- ascending
    origins from 0 to L - t without a gap, flip codes in [0, 4), weights finite and > 0 -- because the kernel trusts them.
    Returns pred uint8 [B, H, W]; with ``labels`` (uint8 [B, H, W], 255 = ignore) (pred, counts int64 [3, C]) as ``seg_predict``; with
    ``want_conf`` the fp32 [B, H, W] confidence 1 / sum_c exp(L_c - L_max) is appended."""
    name = "seg_blend_predict"
    if not isinstance(z, Tensor) or z.dim() != 6 or not z.is_floating_point():
        raise ValueError(f"{name}: tile logits must be a floating-point [B, F, ny, nx, P, C] tensor, got {_describe(z)}")
    B, F, ny, nx, P, C = z.shape
    g = math.isqrt(P)
    if min(B, ny, nx) < 1:
        raise ValueError(f"{name}: T = B F ny nx must be >= 1 (z is {tuple(z.shape)})")
    if not 1 <= F <= SEG_BLEND_MAX_FLIPS:
        raise ValueError(f"{name}: F = {F} flip variants, must lie in [1, {SEG_BLEND_MAX_FLIPS}]")
    if P < 1 or g * g != P:
        raise ValueError(f"{name}: P = {P} patches are not a square grid (z is {tuple(z.shape)})")
    if not 2 <= C <= SEG_MAX_CLASSES:
        raise ValueError(f"{name}: C must lie in [2, {SEG_MAX_CLASSES}], got {C}")
    for what, v in (("H", H), ("W", W), ("t", t)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= 1 << 20:
            raise ValueError(f"{name}: {what} must be an integer in [1, 2^20], got {v!r}")
    H, W, t = int(H), int(W), int(t)
    if t > min(H, W):
        raise ValueError(f"{name}: tile side t = {t} exceeds min(H, W) = {min(H, W)}")
    if t * g > 1 << 28 or g > 4096:
        raise ValueError(f"{name}: g = {g}, t = {t}: g <= 4096 and t g <= 2^28")
    ys_h, xs_h = _host_table(name, "ys", ys, np.int32), _host_table(name, "xs", xs, np.int32)
    fl_h, win_h = _host_table(name, "flips", flips, np.int32), _host_table(name, "win", win, np.float32)
    if ys_h.size != ny or xs_h.size != nx or fl_h.size != F:
        raise ValueError(f"{name}: ys, xs, flips have {ys_h.size}, {xs_h.size}, {fl_h.size} entries; z {tuple(z.shape)} wants {ny}, {nx}, {F}")
    _seg_blend_origins(name, "ys", ys_h, H, t)
    _seg_blend_origins(name, "xs", xs_h, W, t)
    if ((fl_h < 0) | (fl_h > 3)).any():
        raise ValueError(f"{name}: flip codes must lie in [0, 4) (bit 0: mirrored along x, bit 1: along y), got {fl_h.tolist()}")
    if win_h.size != t or not bool((np.isfinite(win_h) & (win_h > 0)).all()):
        raise ValueError(f"{name}: win must hold t = {t} finite weights > 0 (got {win_h.size}, min {float(np.min(win_h))!r})")
    if labels is not None:
        if not isinstance(labels, Tensor) or labels.dtype != torch.uint8 or tuple(labels.shape) != (B, H, W):
            raise ValueError(f"{name}: labels must be uint8 [{B}, {H}, {W}] (255 = ignore), got {_describe(labels)}")
        if labels.device != z.device:
            raise ValueError(f"{name}: logits on {z.device}, labels on {labels.device}")
    _need_cuda(z, labels)
    z = _c(z.float())
    dev = z.device
    tab = torch.from_numpy(np.concatenate([ys_h, xs_h, fl_h])).to(dev)
    wn = torch.from_numpy(win_h).to(dev)
    pred = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    conf = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_conf else None
    counts = None
    if labels is not None:
        labels = _c(labels)
        counts = torch.empty(3 * C + 1, dtype=torch.int64, device=dev)
    check(lib.dinox_seg_blend_predict(_p(z), tab.data_ptr(), tab.data_ptr() + 4 * ny, tab.data_ptr() + 4 * (ny + nx), _p(wn), _p(labels), _p(pred),
                                      _p(conf), _p(counts), B, F, ny, nx, g, t, C, H, W, _stream()), "dinox_seg_blend_predict")
    out = [pred]
    if counts is not None:
        _seg_refuse_bad_labels(name, int(counts[3 * C]), C)
        out.append(counts[:3 * C].view(3, C))
    if want_conf:
        out.append(conf)
    return out[0] if len(out) == 1 else tuple(out)


# ------------------------------------------------------------------------------------------
# patch sampling for training at native resolution (csrc/segpatch.hip)
# ------------------------------------------------------------------------------------------
SEG_PATCH_MAX_SIDE = 1 << 14        # S
SEG_PATCH_MAX_PLANE = 1 << 20       # H, W of a source plane
SEG_PATCH_MAX_RUNS = 1 << 31        # B S ceil(S / 64): the grid


def _host_matrix(name: str, what: str, v, cols: int, dtype) -> np.ndarray:
    """A [B, cols] host copy of a job table given as a nested sequence, an ndarray or a tensor (a device tensor costs one read)."""
    a = v.detach().cpu().numpy() if isinstance(v, Tensor) else np.asarray(v)
    integer = dtype == np.int64
    if a.ndim != 2 or a.shape[1] != cols or a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) if integer
                                                                         else np.issubdtype(a.dtype, np.number)):
        raise ValueError(f"{name}: {what} must be a [B, {cols}] {'integer' if integer else 'numeric'} table, got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a, dtype=dtype)


def seg_patch_sample(img_pool: Tensor, msk_pool: Tensor, jobs, par, S: int, mean, std, pad: float = 0.0, *, out=None):
    """B training patches in one launch: (x fp32 [B, 3, S, S], m uint8 [B, S, S]) sampled from the device-resident pools ``img_pool``
    (fp32, 1-D, planes already windowed to [0, 1]) and ``msk_pool`` (uint8, 1-D) under each job's inverse affine map -- the image
    bilinear with ``pad`` outside the plane, then gain * v^gamma and (v - mean_c) / std_c; the label nearest with 255 (ignore) outside;
    include/dinox.h has the definitions.  ``jobs`` int64 [B, 4] = (image offset, mask offset, H, W) and ``par`` fp32 [B, 8] =
    (a00, a01, a02, a10, a11, a12, gamma, gain) are host tables (nested sequences, ndarrays or tensors).  They are checked here, before
    the library is touched, because the kernel trusts ``jobs``: every plane inside its pool, 1 <= H, W <= 2^20, ``par`` finite,
    gamma > 0, 1 <= S <= 2^14, B S ceil(S / 64) <= 2^31.  ``out = (x, m)``: contiguous tensors of those shapes to write into instead of fresh ones -- views into larger buffers included,
    which is how the tests put guard elements around both outputs and reach the label store path of an unaligned ``m``."""
    name = "seg_patch_sample"
    if not isinstance(img_pool, Tensor) or img_pool.dtype != torch.float32 or img_pool.dim() != 1 or not img_pool.is_contiguous():
        raise ValueError(f"{name}: img_pool must be a contiguous 1-D float32 tensor, got {_describe(img_pool)}")
    if not isinstance(msk_pool, Tensor) or msk_pool.dtype != torch.uint8 or msk_pool.dim() != 1 or not msk_pool.is_contiguous():
        raise ValueError(f"{name}: msk_pool must be a contiguous 1-D uint8 tensor, got {_describe(msk_pool)}")
    if img_pool.device != msk_pool.device:
        raise ValueError(f"{name}: img_pool on {img_pool.device}, msk_pool on {msk_pool.device}")
    if isinstance(S, bool) or not isinstance(S, (int, np.integer)) or not 1 <= S <= SEG_PATCH_MAX_SIDE:
        raise ValueError(f"{name}: S must be an integer in [1, 2^14], got {S!r}")
    S = int(S)
    jb, pr = _host_matrix(name, "jobs", jobs, 4, np.int64), _host_matrix(name, "par", par, 8, np.float32)
    B = jb.shape[0]
    if pr.shape[0] != B:
        raise ValueError(f"{name}: {B} jobs but {pr.shape[0]} rows of par")
    if B < 1 or B > 1 << 20 or B * S * (-(-S // 64)) > SEG_PATCH_MAX_RUNS:
        raise ValueError(f"{name}: B = {B} patches of side {S}: 1 <= B <= 2^20 and B S ceil(S / 64) <= 2^31 (what one grid takes)")
    hw = jb[:, 2:]
    if ((hw < 1) | (hw > SEG_PATCH_MAX_PLANE)).any():
        k = int(np.argmax(((hw < 1) | (hw > SEG_PATCH_MAX_PLANE)).any(1)))
        raise ValueError(f"{name}: job {k}: plane of H x W = {int(hw[k, 0])} x {int(hw[k, 1])}; both must lie in [1, 2^20]")
    area = hw[:, 0] * hw[:, 1]
    for col, pool, what in ((0, img_pool, "img_pool"), (1, msk_pool, "msk_pool")):
        bad = (jb[:, col] < 0) | (jb[:, col] > pool.numel() - area)
        if bad.any():
            k = int(np.argmax(bad))
            raise ValueError(f"{name}: job {k}: plane [{int(jb[k, col])}, {int(jb[k, col] + area[k])}) leaves {what} of {pool.numel()} elements")
    if not np.isfinite(pr).all():
        raise ValueError(f"{name}: par holds a non-finite value (job {int(np.argmax(~np.isfinite(pr).all(1)))})")
    if (pr[:, 6] <= 0).any():
        k = int(np.argmax(pr[:, 6] <= 0))
        raise ValueError(f"{name}: job {k}: gamma = {float(pr[k, 6])!r} must be > 0")
    mean_h, std_h = np.asarray(mean, dtype=np.float32).reshape(-1), np.asarray(std, dtype=np.float32).reshape(-1)
    if mean_h.size != 3 or std_h.size != 3 or not (np.isfinite(mean_h).all() and np.isfinite(std_h).all() and (std_h > 0).all()):
        raise ValueError(f"{name}: mean and std must be 3 finite values each, std > 0, got {mean_h.tolist()} and {std_h.tolist()}")
    if not math.isfinite(float(pad)):
        raise ValueError(f"{name}: pad = {pad!r} is not finite")
    dev = img_pool.device
    if out is not None:
        x, m = out
        if not (isinstance(x, Tensor) and x.dtype == torch.float32 and tuple(x.shape) == (B, 3, S, S) and x.is_contiguous() and x.device == dev
                and isinstance(m, Tensor) and m.dtype == torch.uint8 and tuple(m.shape) == (B, S, S) and m.is_contiguous() and m.device == dev):
            raise ValueError(f"{name}: out must be contiguous (float32 [{B}, 3, {S}, {S}], uint8 [{B}, {S}, {S}]) on {dev}, got {_describe(*out)}")
    _need_cuda(img_pool, msk_pool)
    if out is None:
        x = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
        m = torch.empty((B, S, S), dtype=torch.uint8, device=dev)
    jd, pd = torch.from_numpy(jb).to(dev), torch.from_numpy(pr).to(dev)
    check(lib.dinox_seg_patch_sample(_p(img_pool), _p(msk_pool), _p(jd), _p(pd), _p(x), _p(m), B, S, mean_h.ctypes.data, std_h.ctypes.data,
                                     float(pad), _stream()), "dinox_seg_patch_sample")
    return x, m


# ------------------------------------------------------------------------------------------
# surface distances between two label maps (csrc/surfdist.hip)
# ------------------------------------------------------------------------------------------
SURFACE_MAX_SIDE = 1024
SURFACE_MAX_TOLERANCES = 8
SURFACE_WS_CAP = 256 << 20      # bytes of workspace per call: a longer batch is evaluated in pieces (a single image may exceed it)


def _surface_maps(pred, labels):
    """(B, H, W) of two uint8 label maps [B, H, W] on one device; ValueError for anything the kernel does not take."""
    for what, t in (("pred", pred), ("labels", labels)):
        if not isinstance(t, Tensor) or t.dtype != torch.uint8 or t.dim() != 3:
            raise ValueError(f"surface_stats: {what} must be uint8 [B, H, W], got {_describe(t)}")
    if pred.shape != labels.shape:
        raise ValueError(f"surface_stats: pred {tuple(pred.shape)} and labels {tuple(labels.shape)} differ in shape")
    if pred.device != labels.device:
        raise ValueError(f"surface_stats: pred on {pred.device}, labels on {labels.device}")
    B, H, W = pred.shape
    if B < 1 or not (1 <= H <= SURFACE_MAX_SIDE and 1 <= W <= SURFACE_MAX_SIDE):
        raise ValueError(f"surface_stats: maps must be [B >= 1, H, W] with 1 <= H, W <= {SURFACE_MAX_SIDE}, got {tuple(pred.shape)}")
    return B, H, W


def _surface_spacing(spacing, B: int, device) -> Tensor:
    """spacing [B, 2] = (s_y, s_x) in mm per pixel -> fp32 on ``device``; every entry finite and > 0."""
    sp = torch.as_tensor(spacing)
    if sp.dim() != 2 or tuple(sp.shape) != (B, 2) or sp.is_complex() or sp.dtype == torch.bool:
        raise ValueError(f"surface_stats: spacing must be [{B}, 2] = (s_y, s_x) in mm per pixel, got {_describe(sp)}")
    sp = sp.to(device=device, dtype=torch.float32)
    if not bool((torch.isfinite(sp) & (sp > 0)).all()):
        raise ValueError("surface_stats: every spacing must be finite and > 0")
    return _c(sp)


def _surface_params(fn: str, num_classes, tolerances, q):
    """(C, tolerances as floats) of surface_stats / surface_stats_3d; ValueError for anything the kernels do not take."""
    C = num_classes
    if isinstance(C, bool) or not isinstance(C, int) or not 2 <= C <= SEG_MAX_CLASSES:
        raise ValueError(f"{fn}: num_classes must be an integer in [2, {SEG_MAX_CLASSES}], got {C!r}")
    try:
        tol = [float(t) for t in tolerances]
    except TypeError as e:
        raise ValueError(f"{fn}: tolerances must be a sequence of numbers, got {tolerances!r}") from e
    if not 1 <= len(tol) <= SURFACE_MAX_TOLERANCES or not all(math.isfinite(t) and t >= 0 for t in tol):
        raise ValueError(f"{fn}: 1 to {SURFACE_MAX_TOLERANCES} tolerances in mm, finite and >= 0, got {tolerances!r}")
    if (not isinstance(q, (tuple, list)) or len(q) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in q)
            or not 0 < q[0] <= q[1] or q[1] >= 1 << 31):
        raise ValueError(f"{fn}: q must be two integers (q_num, q_den) with 0 < q_num <= q_den, got {q!r}")
    return C, tol


def surface_stats(pred: Tensor, labels: Tensor, spacing, num_classes: int, tolerances=(1.0,), q=(95, 100)):
    """Directed surface-distance statistics of two uint8 label maps [B, H, W] (labels: 255 = ignore) in mm, spacing [B, 2] = (s_y, s_x)
    per image (include/dinox.h has the definitions).  Returns (counts int64 [B, C, 2, 1 + T] = (n, within tolerance t), values fp32
    [B, C, 2, 3] = (sum, max, q[0]/q[1] nearest-rank quantile)), both on the device; direction 0 runs from the border of ``pred`` to the
    border of ``labels``, direction 1 the other way.  dinox.segment.surface_metrics forms HD95 / ASSD / NSD from them.  The batch is cut
    so that one call's workspace stays under SURFACE_WS_CAP; the results do not depend on the cut.  A label >= C other than 255 in
    ``labels``, or any value >= C in ``pred``, raises ValueError (one device read of two integers)."""
    B, H, W = _surface_maps(pred, labels)
    C, tol = _surface_params("surface_stats", num_classes, tolerances, q)
    _need_cuda(pred, labels)
    dev = pred.device
    sp = _surface_spacing(spacing, B, dev)
    pred, labels = _c(pred), _c(labels)
    T = len(tol)
    tol_host = (_lib.f32 * T)(*tol)                         # a host array: the entry reads it during the call
    counts = torch.empty((B, C, 2, 1 + T), dtype=torch.int64, device=dev)
    values = torch.empty((B, C, 2, 3), dtype=torch.float32, device=dev)
    per_image = int(lib.dinox_surface_ws_bytes(1, H, W, C))
    step = max(1, min(B, SURFACE_WS_CAP // per_image))
    while step > 1 and not lib.dinox_surface_ws_bytes(step, H, W, C):      # the launch grids bound the images per call as well
        step //= 2
    ws = torch.empty(per_image * step // 4, dtype=torch.float32, device=dev)
    bad = torch.zeros((-(-B // step), 2), dtype=torch.int64, device=dev)
    for i, b0 in enumerate(range(0, B, step)):
        n = min(step, B - b0)
        check(lib.dinox_surface_stats(_p(pred[b0:]), _p(labels[b0:]), _p(sp[b0:]), tol_host, _p(counts[b0:]), _p(values[b0:]), _p(bad[i]), _p(ws),
                                      n, H, W, C, T, int(q[0]), int(q[1]), _stream()), "dinox_surface_stats")
    nbad = bad.sum(0).tolist()
    if nbad[0] or nbad[1]:
        raise ValueError(f"surface_stats: {nbad[0]} value(s) of pred are >= C = {C}, {nbad[1]} label(s) are >= C and not {SEG_IGNORE} (ignore)")
    return counts, values


# ------------------------------------------------------------------------------------------
# boundary loss: signed distance maps (csrc/distmap.hip) and the boundary term of the segmentation loss (csrc/segloss.hip)
# ------------------------------------------------------------------------------------------
def signed_distance_map(labels: Tensor, spacing, num_classes: int) -> Tensor:
    """Signed Euclidean distance maps phi fp32 [B, C, H, W] of a uint8 label map [B, H, W] (255 = ignore), spacing [B, 2] = (s_y, s_x) per
    image (include/dinox.h has the definitions): +distance to the class outside it, -distance to the other valid pixels inside it, 0 at
    ignored pixels and where the class is absent from the image or covers all of it.  The batch is cut so that one call's workspace stays
    under SURFACE_WS_CAP; the result does not depend on the cut.  A label >= C other than 255 raises ValueError (one device read)."""
    if not isinstance(labels, Tensor) or labels.dtype != torch.uint8 or labels.dim() != 3:
        raise ValueError(f"signed_distance_map: labels must be uint8 [B, H, W], got {_describe(labels)}")
    B, H, W = labels.shape
    if B < 1 or not (1 <= H <= SURFACE_MAX_SIDE and 1 <= W <= SURFACE_MAX_SIDE):
        raise ValueError(f"signed_distance_map: maps must be [B >= 1, H, W] with 1 <= H, W <= {SURFACE_MAX_SIDE}, got {tuple(labels.shape)}")
    C = num_classes
    if isinstance(C, bool) or not isinstance(C, int) or not 2 <= C <= SEG_MAX_CLASSES:
        raise ValueError(f"signed_distance_map: num_classes must be an integer in [2, {SEG_MAX_CLASSES}], got {C!r}")
    _need_cuda(labels)
    dev = labels.device
    try:
        sp = _surface_spacing(spacing, B, dev)
    except ValueError as e:
        raise ValueError(str(e).replace("surface_stats", "signed_distance_map")) from None
    labels = _c(labels)
    phi = torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
    per_image = int(lib.dinox_signed_distance_ws_bytes(1, H, W, C))
    step = max(1, min(B, SURFACE_WS_CAP // per_image))
    while step > 1 and not lib.dinox_signed_distance_ws_bytes(step, H, W, C):      # the launch grids bound the images per call as well
        step //= 2
    ws = torch.empty(per_image * step // 4, dtype=torch.float32, device=dev)
    bad = torch.zeros(-(-B // step), dtype=torch.int64, device=dev)
    for i, b0 in enumerate(range(0, B, step)):
        n = min(step, B - b0)
        check(lib.dinox_signed_distance(_p(labels[b0:]), _p(sp[b0:]), _p(phi[b0:]), _p(bad[i:]), _p(ws), n, H, W, C, _stream()),
              "dinox_signed_distance")
    _seg_refuse_bad_labels("signed_distance_map", int(bad.sum()), C)
    return phi


def seg_loss_bd_fwd(z: Tensor, y: Tensor, phi: Tensor, w_ce: float = 1.0, w_dice: float = 1.0, w_bd: float = 1.0, c0: int = 0):
    """seg_loss_fwd with the boundary term: phi fp32 [B, C, S, S] from signed_distance_map(y, ...).  Returns (loss[4] = (L, CE, Dice, BD),
    L = w_ce CE + w_dice Dice + w_bd BD, stats [3, C], saved); seg_loss_bd_bwd(saved, gscale) gives d(gscale L)/dz.  phi is data: it
    gets no gradient."""
    B, g, C = _seg_geometry("seg_loss_bd", z, 1)
    u = _seg_labels("seg_loss_bd", y, B, g, z)
    S = g * u
    if not isinstance(phi, Tensor) or phi.dtype != torch.float32 or tuple(phi.shape) != (B, C, S, S):
        raise ValueError(f"seg_loss_bd: phi must be fp32 [{B}, {C}, {S}, {S}] (ops.signed_distance_map of the labels), got {_describe(phi)}")
    if phi.device != z.device:
        raise ValueError(f"seg_loss_bd: logits on {z.device}, phi on {phi.device}")
    if c0 not in (0, 1):
        raise ValueError(f"seg_loss_bd: c0 must be 0 or 1, got {c0!r}")
    _need_cuda(z, y, phi)
    z, y, phi = _c(z.float()), _c(y), _c(phi)
    dev = z.device
    loss = torch.empty(4, dtype=torch.float32, device=dev)
    stats = torch.empty((3, C), dtype=torch.float32, device=dev)
    nv = torch.empty(2, dtype=torch.int64, device=dev)
    ws = torch.empty(int(lib.dinox_seg_loss_bd_ws_bytes(B, g, u, C)) // 4, dtype=torch.float32, device=dev)
    check(lib.dinox_seg_loss_bd_fwd(_p(z), _p(y), _p(phi), _p(loss), _p(stats), _p(nv), _p(ws), B, g, u, C, int(c0), float(w_ce), float(w_dice),
                                    float(w_bd), _stream()), "dinox_seg_loss_bd_fwd")
    _seg_refuse_bad_labels("seg_loss_bd", int(nv[1]), C)
    return loss, stats, (z, y, phi, stats, nv, ws, (B, g, u, C, int(c0), float(w_ce), float(w_dice), float(w_bd)))


def seg_loss_bd_bwd(saved, gscale: float = 1.0) -> Tensor:
    """dz [B, g^2, C] fp32 = d(gscale L)/dz of seg_loss_bd_fwd, the boundary term in the same pixel pass as the other two."""
    z, y, phi, stats, nv, ws, (B, g, u, C, c0, w_ce, w_dice, w_bd) = saved
    dz = torch.empty_like(z)
    check(lib.dinox_seg_loss_bd_bwd(_p(z), _p(y), _p(phi), _p(stats), _p(nv), _p(dz), _p(ws), B, g, u, C, c0, w_ce, w_dice, w_bd, float(gscale),
                                    _stream()), "dinox_seg_loss_bd_bwd")
    return dz


class SegBoundaryLossFn(torch.autograd.Function):
    """(z, y, phi, w_ce, w_dice, w_bd, c0) -> (L, CE, Dice, BD) as 0-d tensors; the backward takes the upstream gradient of L only (the
    other three are reported values) and gives one to z only.  z of any floating dtype is cast to fp32."""

    @staticmethod
    def forward(ctx, z, y, phi, w_ce=1.0, w_dice=1.0, w_bd=1.0, c0=0):
        loss, _, saved = seg_loss_bd_fwd(z, y, phi, w_ce, w_dice, w_bd, c0)
        ctx.saved, ctx.zdt = saved, z.dtype
        total, ce, dice, bd = (loss[i].clone() for i in range(4))
        ctx.mark_non_differentiable(ce, dice, bd)
        return total, ce, dice, bd

    @staticmethod
    def backward(ctx, g, *_reported):
        d = seg_loss_bd_bwd(ctx.saved, 1.0) * g             # (a device scalar: no host sync, as in SegLossFn)
        return (d if d.dtype == ctx.zdt else d.to(ctx.zdt)), None, None, None, None, None, None


def surface_stats_3d(pred: Tensor, labels: Tensor, spacing, num_classes: int, tolerances=(1.0,), q=(95, 100)):
    """Directed surface-distance statistics of two uint8 label volumes [Z, H, W] (labels: 255 = ignore) in mm with the voxel
    spacing = (s_z, s_y, s_x) (include/dinox.h has the definitions: the border is taken with the six face neighbours, so a one-slice volume
    is all border and does not reproduce ``surface_stats`` of that slice).  Returns (counts int64 [C, 2, 1 + T] = (n, within tolerance t),
    values fp32 [C, 2, 3] = (sum, max, q[0]/q[1] nearest-rank quantile)), both on the device; direction 0 runs from the border of ``pred``
    to the border of ``labels``, direction 1 the other way.  dinox.segment.surface_metrics_3d forms HD95 / ASSD / NSD from them.  The
    workspace is 12 bytes per voxel whatever C is (the classes are walked one at a time).  A label >= C other than 255 in ``labels``, or
    any value >= C in ``pred``, raises ValueError (one device read of two integers)."""
    for what, t in (("pred", pred), ("labels", labels)):
        if not isinstance(t, Tensor) or t.dtype != torch.uint8 or t.dim() != 3:
            raise ValueError(f"surface_stats_3d: {what} must be uint8 [Z, H, W], got {_describe(t)}")
    if pred.shape != labels.shape:
        raise ValueError(f"surface_stats_3d: pred {tuple(pred.shape)} and labels {tuple(labels.shape)} differ in shape")
    if pred.device != labels.device:
        raise ValueError(f"surface_stats_3d: pred on {pred.device}, labels on {labels.device}")
    Z, H, W = pred.shape
    if not all(1 <= n <= SURFACE_MAX_SIDE for n in (Z, H, W)):
        raise ValueError(f"surface_stats_3d: volumes must be [Z, H, W] with 1 <= Z, H, W <= {SURFACE_MAX_SIDE}, got {tuple(pred.shape)}")
    # (so Z H W <= 2^30: every count fits an unsigned 32-bit integer)
    C, tol = _surface_params("surface_stats_3d", num_classes, tolerances, q)
    try:
        sp = [float(v) for v in (spacing.tolist() if isinstance(spacing, Tensor) else spacing)]
    except (TypeError, ValueError) as e:
        raise ValueError(f"surface_stats_3d: spacing must be three numbers (s_z, s_y, s_x) in mm per voxel, got {spacing!r}") from e
    if len(sp) != 3:
        raise ValueError(f"surface_stats_3d: spacing must be three numbers (s_z, s_y, s_x) in mm per voxel, got {spacing!r}")
    sp_host = (_lib.f32 * 3)(*sp)                           # host arrays: the entry reads them during the call
    if not all(math.isfinite(v) and v > 0 for v in sp_host):
        raise ValueError(f"surface_stats_3d: every spacing must be finite and > 0 (in fp32), got {spacing!r}")
    _need_cuda(pred, labels)
    dev = pred.device
    pred, labels = _c(pred), _c(labels)
    T = len(tol)
    tol_host = (_lib.f32 * T)(*tol)
    counts = torch.empty((C, 2, 1 + T), dtype=torch.int64, device=dev)
    values = torch.empty((C, 2, 3), dtype=torch.float32, device=dev)
    ws = torch.empty(int(lib.dinox_surface3d_ws_bytes(Z, H, W, C)) // 4, dtype=torch.float32, device=dev)
    bad = torch.zeros(2, dtype=torch.int64, device=dev)
    check(lib.dinox_surface3d_stats(_p(pred), _p(labels), sp_host, tol_host, _p(counts), _p(values), _p(bad), _p(ws), Z, H, W, C, T, int(q[0]), int(q[1]),
                                    _stream()), "dinox_surface3d_stats")
    nbad = bad.tolist()
    if nbad[0] or nbad[1]:
        raise ValueError(f"surface_stats_3d: {nbad[0]} value(s) of pred are >= C = {C}, {nbad[1]} label(s) are >= C and not {SEG_IGNORE} (ignore)")
    return counts, values


# ------------------------------------------------------------------------------------------
# connected components of a label map: labelling, clean-up, lesion-wise counts (csrc/cclabel.hip)
# ------------------------------------------------------------------------------------------
CC_MAX_SIDE = 1024
CC_WS_CAP = 256 << 20           # bytes of workspace per call: a longer batch is labelled in pieces (images are independent)
CC3D_MAX_VOXELS = 1 << 30       # one volume is labelled whole: every voxel index and every area fits int32


def _cc_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _cc_maps(fn: str, named, num_classes, connectivity, volume: bool = False):
    """(B, H, W) of uint8 maps [B, H, W] of one shape on one device (``named``: (name, tensor or None) pairs; None is skipped);
    ValueError for anything the kernels do not take.  ``volume``: (Z, H, W) of one volume [Z, H, W] and its connectivities."""
    lead, conns, said = ("Z", (6, 18, 26), "6, 18 or 26") if volume else ("B", (4, 8), "4 or 8")
    first = None
    for what, t in named:
        if t is None:
            continue
        if not isinstance(t, Tensor) or t.dtype != torch.uint8 or t.dim() != 3:
            raise ValueError(f"{fn}: {what} must be uint8 [{lead}, H, W], got {_describe(t)}")
        if first is None:
            first = (what, t)
        elif t.shape != first[1].shape:
            raise ValueError(f"{fn}: {first[0]} {tuple(first[1].shape)} and {what} {tuple(t.shape)} differ in shape")
        elif t.device != first[1].device:
            raise ValueError(f"{fn}: {first[0]} on {first[1].device}, {what} on {t.device}")
    B, H, W = first[1].shape
    if B < 1 or not (1 <= H <= CC_MAX_SIDE and 1 <= W <= CC_MAX_SIDE):
        raise ValueError(f"{fn}: maps must be [{lead} >= 1, H, W] with 1 <= H, W <= {CC_MAX_SIDE}, got {tuple(first[1].shape)}")
    if volume and B * H * W > CC3D_MAX_VOXELS:
        raise ValueError(f"{fn}: a volume holds at most 2^30 voxels, got {tuple(first[1].shape)}")
    if not _cc_int(num_classes) or not 2 <= num_classes <= SEG_MAX_CLASSES:
        raise ValueError(f"{fn}: num_classes must be an integer in [2, {SEG_MAX_CLASSES}], got {num_classes!r}")
    if not _cc_int(connectivity) or connectivity not in conns:
        raise ValueError(f"{fn}: connectivity must be {said}, got {connectivity!r}")
    return B, H, W


def _cc_min_px(fn: str, min_px, B: int):
    """None, one integer or B integers (a sequence or an integer tensor), each in [0, 2^31) -> None or an int32 tensor [B] on the host."""
    if min_px is None:
        return None
    if _cc_int(min_px):
        min_px = [min_px] * B
    t = min_px if isinstance(min_px, Tensor) else None
    if t is None:
        try:
            vals = list(min_px)
        except TypeError as e:
            raise ValueError(f"{fn}: min_px must be None, an integer or {B} integers, got {min_px!r}") from e
        if not all(_cc_int(v) for v in vals):
            raise ValueError(f"{fn}: min_px must be None, an integer or {B} integers, got {min_px!r}")
        if len(vals) != B or not all(0 <= v < 1 << 31 for v in vals):
            raise ValueError(f"{fn}: min_px must hold {B} value(s) in [0, 2^31), got {min_px!r}")
        return torch.tensor(vals, dtype=torch.int32)
    if t.dtype not in (torch.int32, torch.int64) or tuple(t.shape) != (B,):
        raise ValueError(f"{fn}: min_px must be None, an integer or {B} integers, got {_describe(t)}")
    if not bool(((t >= 0) & (t < 1 << 31)).all()):
        raise ValueError(f"{fn}: min_px must hold {B} value(s) in [0, 2^31)")
    return t.to(torch.int32)


def _cc_step(B: int, H: int, W: int, C: int) -> int:
    """Images per call: the workspace under CC_WS_CAP (one image may exceed it) and the sizes inside what the entries take."""
    step = max(1, min(B, CC_WS_CAP // int(lib.dinox_cc_ws_bytes(1, H, W, C))))
    while step > 1 and not lib.dinox_cc_ws_bytes(step, H, W, C):
        step //= 2
    return step


def _cc_ws(step: int, H: int, W: int, C: int, dev) -> Tensor:
    return torch.empty(int(lib.dinox_cc_ws_bytes(step, H, W, C)) // 8, dtype=torch.int64, device=dev)


def _cc_label_into(labels, mask, C, conn, ws, step):
    """(comp, area, ncomp, bad [chunks]) of contiguous device maps, nothing read back."""
    B, H, W = labels.shape
    dev = labels.device
    comp = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    area = torch.empty((B, H, W), dtype=torch.int32, device=dev)
    ncomp = torch.empty((B, C), dtype=torch.int64, device=dev)
    bad = torch.zeros(-(-B // step), dtype=torch.int64, device=dev)
    for i, b0 in enumerate(range(0, B, step)):
        check(lib.dinox_cc_label(_p(labels[b0:]), None if mask is None else _p(mask[b0:]), _p(comp[b0:]), _p(area[b0:]), _p(ncomp[b0:]), _p(bad[i:]),
                                 _p(ws), min(step, B - b0), H, W, C, conn, _stream()), "dinox_cc_label")
    return comp, area, ncomp, bad


def _cc_refuse(fn: str, what: str, bad: int, C: int) -> None:
    if bad:
        raise ValueError(f"{fn}: {bad} value(s) of {what} are >= C = {C} and not {SEG_IGNORE}")


def cc_label(labels: Tensor, num_classes: int, connectivity: int = 8, mask: Optional[Tensor] = None):
    """Connected components of a uint8 label map [B, H, W], every class in one pass (include/dinox.h has the definitions).  Returns
    (comp int32 [B, H, W]: the index y W + x of the component's first pixel in raster order, -1 where the pixel is in none; area int32
    [B, H, W]: the pixel count at that root pixel, 0 elsewhere; ncomp int64 [B, C]), all on the device.  A pixel with ``mask == 255`` or
    a label of 255 is in no component; any other label >= C raises ValueError (one device read).  ``connectivity`` 4 joins pixels that
    share an edge, 8 also those that share a corner.  The batch is cut so that one call's workspace stays under CC_WS_CAP; the results
    do not depend on the cut."""
    B, H, W = _cc_maps("cc_label", (("labels", labels), ("mask", mask)), num_classes, connectivity)
    _need_cuda(labels, mask)
    labels, mask = _c(labels), None if mask is None else _c(mask)
    step = _cc_step(B, H, W, num_classes)
    comp, area, ncomp, bad = _cc_label_into(labels, mask, num_classes, connectivity, _cc_ws(step, H, W, num_classes, labels.device), step)
    _cc_refuse("cc_label", "labels", int(bad.sum()), num_classes)
    return comp, area, ncomp


def cc_filter(labels: Tensor, num_classes: int, *, min_px=None, keep_largest: bool = False, first_class: int = 1, connectivity: int = 8,
              mask: Optional[Tensor] = None, targets: Optional[Tensor] = None):
    """Clean-up of a uint8 label map [B, H, W]: ``out`` equals ``labels`` where the pixel's component is kept and is 0 elsewhere.  Classes
    below ``first_class`` are always kept; a component of another class is kept iff its area >= min_px[b] (None: 1; one integer or B of
    them) and, with ``keep_largest``, it is the largest of its (image, class) -- equal areas: the one whose first pixel comes first.
    With ``targets`` (uint8, 255 = ignore) returns (out, counts int64 [3, C]) with ops.seg_predict's counts of ``out`` against them.
    Labels internally (``connectivity``, ``mask``: see cc_label); bad values raise ValueError after one device read."""
    B, H, W = _cc_maps("cc_filter", (("labels", labels), ("mask", mask), ("targets", targets)), num_classes, connectivity)
    C = num_classes
    if not _cc_int(first_class) or not 0 <= first_class <= C:
        raise ValueError(f"cc_filter: first_class must be an integer in [0, {C}], got {first_class!r}")
    if not isinstance(keep_largest, (bool, int)):
        raise ValueError(f"cc_filter: keep_largest must be a bool, got {keep_largest!r}")
    mp = _cc_min_px("cc_filter", min_px, B)
    _need_cuda(labels, mask, targets)
    dev = labels.device
    labels, mask, targets = _c(labels), None if mask is None else _c(mask), None if targets is None else _c(targets)
    mp = None if mp is None else mp.to(dev)
    step = _cc_step(B, H, W, C)
    ws = _cc_ws(step, H, W, C, dev)
    comp, area, _, bad = _cc_label_into(labels, mask, C, connectivity, ws, step)
    out = torch.empty_like(labels)
    counts = None if targets is None else torch.empty((-(-B // step), 3 * C + 1), dtype=torch.int64, device=dev)
    for i, b0 in enumerate(range(0, B, step)):
        check(lib.dinox_cc_filter(_p(labels[b0:]), _p(comp[b0:]), _p(area[b0:]), None if mp is None else _p(mp[b0:]),
                                  None if targets is None else _p(targets[b0:]), _p(out[b0:]), None if counts is None else _p(counts[i]), _p(ws),
                                  min(step, B - b0), H, W, C, first_class, int(bool(keep_largest)), _stream()), "dinox_cc_filter")
    if counts is None:
        _cc_refuse("cc_filter", "labels", int(bad.sum()), C)
        return out
    counts = counts.sum(0)
    nbad = torch.stack([bad.sum(), counts[3 * C]]).tolist()
    _cc_refuse("cc_filter", "labels", nbad[0], C)
    _seg_refuse_bad_labels("cc_filter", nbad[1], C)
    return out, counts[:3 * C].view(3, C)


def lesion_counts(pred: Tensor, labels: Tensor, num_classes: int, *, connectivity: int = 8, overlap=(0, 1), min_px=None) -> Tensor:
    """Lesion-wise detection counts of a prediction against a ground truth, both uint8 [B, H, W] (labels: 255 = ignore):
    int64 [B, C, 4] = (n_gt, n_gt_hit, n_pred, n_pred_hit) on the device.  The components of ``pred`` are taken over the pixels
    ``labels`` does not ignore.  A component is hit iff the pixels of it where pred == labels number >= 1 and >= overlap[0] / overlap[1]
    of its area (integers, 0 <= num <= den < 2^20; (0, 1): any overlap).  Components under min_px[b] pixels are no lesions on their side.
    dinox.segment.lesion_metrics turns the counts into sensitivity, precision, F1 and false positives per image."""
    B, H, W = _cc_maps("lesion_counts", (("pred", pred), ("labels", labels)), num_classes, connectivity)
    C = num_classes
    if (not isinstance(overlap, (tuple, list)) or len(overlap) != 2 or not all(_cc_int(v) for v in overlap)
            or not (0 <= overlap[0] <= overlap[1] and 0 < overlap[1] < 1 << 20)):
        raise ValueError(f"lesion_counts: overlap must be two integers (num, den) with 0 <= num <= den and 0 < den < 2^20, got {overlap!r}")
    mp = _cc_min_px("lesion_counts", min_px, B)
    _need_cuda(pred, labels)
    dev = pred.device
    pred, labels = _c(pred), _c(labels)
    mp = None if mp is None else mp.to(dev)
    step = _cc_step(B, H, W, C)
    ws = _cc_ws(step, H, W, C, dev)
    pc, pa, _, pbad = _cc_label_into(pred, labels, C, connectivity, ws, step)
    gc, ga, _, gbad = _cc_label_into(labels, None, C, connectivity, ws, step)
    counts = torch.empty((B, C, 4), dtype=torch.int64, device=dev)
    for b0 in range(0, B, step):
        check(lib.dinox_cc_match(_p(pred[b0:]), _p(pc[b0:]), _p(pa[b0:]), _p(labels[b0:]), _p(gc[b0:]), _p(ga[b0:]), None if mp is None else _p(mp[b0:]),
                                 _p(counts[b0:]), _p(ws), min(step, B - b0), H, W, C, int(overlap[0]), int(overlap[1]), _stream()), "dinox_cc_match")
    nbad = torch.stack([pbad.sum(), gbad.sum()]).tolist()
    _cc_refuse("lesion_counts", "pred", nbad[0], C)
    _cc_refuse("lesion_counts", "labels", nbad[1], C)
    return counts


# ------------------------------------------------------------------------------------------
# connected components of one label volume (csrc/cclabel3d.hip on the stages of csrc/cclabel.hip)
# ------------------------------------------------------------------------------------------
def _cc3d_min_vox(fn: str, min_vox) -> int:
    if min_vox is None:
        return 1
    if not _cc_int(min_vox) or not 0 <= min_vox < 1 << 31:
        raise ValueError(f"{fn}: min_vox must be None or an integer in [0, 2^31), got {min_vox!r}")
    return min_vox


def _cc3d_ws(Z: int, H: int, W: int, C: int, dev) -> Tensor:
    return torch.empty(int(lib.dinox_cc3d_ws_bytes(Z, H, W, C)) // 8, dtype=torch.int64, device=dev)


def _cc3d_label_into(volume, mask, C, conn, ws):
    """(comp, area, ncomp, bad [1]) of a contiguous device volume, nothing read back."""
    Z, H, W = volume.shape
    dev = volume.device
    comp = torch.empty((Z, H, W), dtype=torch.int32, device=dev)
    area = torch.empty((Z, H, W), dtype=torch.int32, device=dev)
    ncomp = torch.empty(C, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int64, device=dev)
    check(lib.dinox_cc3d_label(_p(volume), None if mask is None else _p(mask), _p(comp), _p(area), _p(ncomp), _p(bad), _p(ws), Z, H, W, C, conn,
                               _stream()), "dinox_cc3d_label")
    return comp, area, ncomp, bad


def cc_label_3d(volume: Tensor, num_classes: int, connectivity: int = 26, mask: Optional[Tensor] = None):
    """Connected components of ONE uint8 label volume [Z, H, W], every class in one pass (include/dinox.h has the definitions).  Returns
    (comp int32 [Z, H, W]: the index (z H + y) W + x of the component's first voxel in raster order, -1 where the voxel is in none; area
    int32 [Z, H, W]: the voxel count at that root, 0 elsewhere; ncomp int64 [C]), all on the device.  A voxel with ``mask == 255`` or a
    label of 255 is in no component; any other label >= C raises ValueError (one device read).  ``connectivity`` 6 joins voxels that share
    a face, 18 also those that share an edge, 26 also those that share a corner.  At most 2^30 voxels, 1 <= H, W <= 1024."""
    Z, H, W = _cc_maps("cc_label_3d", (("volume", volume), ("mask", mask)), num_classes, connectivity, volume=True)
    _need_cuda(volume, mask)
    volume, mask = _c(volume), None if mask is None else _c(mask)
    comp, area, ncomp, bad = _cc3d_label_into(volume, mask, num_classes, connectivity, _cc3d_ws(Z, H, W, num_classes, volume.device))
    _cc_refuse("cc_label_3d", "volume", int(bad.sum()), num_classes)
    return comp, area, ncomp


def cc_filter_3d(volume: Tensor, num_classes: int, *, min_vox=None, keep_largest: bool = False, first_class: int = 1, connectivity: int = 26,
                 mask: Optional[Tensor] = None, targets: Optional[Tensor] = None):
    """Clean-up of one uint8 label volume [Z, H, W]: ``out`` equals ``volume`` where the voxel's component is kept and is 0 elsewhere.
    Classes below ``first_class`` are always kept; a component of another class is kept iff its voxel count >= min_vox (None: 1) and,
    with ``keep_largest``, it is the largest of its class in the whole volume -- equal counts: the one whose first voxel comes first.
    With ``targets`` (uint8, 255 = ignore) returns (out, counts int64 [3, C]) with ops.seg_predict's counts of ``out`` against them.
    Labels internally (``connectivity``, ``mask``: see cc_label_3d); bad values raise ValueError after one device read."""
    Z, H, W = _cc_maps("cc_filter_3d", (("volume", volume), ("mask", mask), ("targets", targets)), num_classes, connectivity, volume=True)
    C = num_classes
    if not _cc_int(first_class) or not 0 <= first_class <= C:
        raise ValueError(f"cc_filter_3d: first_class must be an integer in [0, {C}], got {first_class!r}")
    if not isinstance(keep_largest, (bool, int)):
        raise ValueError(f"cc_filter_3d: keep_largest must be a bool, got {keep_largest!r}")
    mv = _cc3d_min_vox("cc_filter_3d", min_vox)
    _need_cuda(volume, mask, targets)
    dev = volume.device
    volume, mask, targets = _c(volume), None if mask is None else _c(mask), None if targets is None else _c(targets)
    ws = _cc3d_ws(Z, H, W, C, dev)
    comp, area, _, bad = _cc3d_label_into(volume, mask, C, connectivity, ws)
    out = torch.empty_like(volume)
    counts = None if targets is None else torch.empty(3 * C + 1, dtype=torch.int64, device=dev)
    check(lib.dinox_cc3d_filter(_p(volume), _p(comp), _p(area), mv, None if targets is None else _p(targets), _p(out),
                                None if counts is None else _p(counts), _p(ws), Z, H, W, C, first_class, int(bool(keep_largest)), _stream()),
          "dinox_cc3d_filter")
    if counts is None:
        _cc_refuse("cc_filter_3d", "volume", int(bad.sum()), C)
        return out
    nbad = torch.stack([bad.sum(), counts[3 * C]]).tolist()
    _cc_refuse("cc_filter_3d", "volume", nbad[0], C)
    _seg_refuse_bad_labels("cc_filter_3d", nbad[1], C)
    return out, counts[:3 * C].view(3, C)


def lesion_counts_3d(pred: Tensor, labels: Tensor, num_classes: int, *, connectivity: int = 26, overlap=(0, 1), min_vox=None) -> Tensor:
    """Lesion-wise detection counts of one predicted volume against its ground truth, both uint8 [Z, H, W] (labels: 255 = ignore):
    int64 [C, 4] = (n_gt, n_gt_hit, n_pred, n_pred_hit) on the device, a lesion being a 3-D component.  The components of ``pred`` are taken
    over the voxels ``labels`` does not ignore.  The hit rule and ``overlap`` are lesion_counts'; components under ``min_vox`` voxels are
    no lesions on their side.  dinox.segment.CaseAccumulator sums the counts over cases."""
    Z, H, W = _cc_maps("lesion_counts_3d", (("pred", pred), ("labels", labels)), num_classes, connectivity, volume=True)
    C = num_classes
    if (not isinstance(overlap, (tuple, list)) or len(overlap) != 2 or not all(_cc_int(v) for v in overlap)
            or not (0 <= overlap[0] <= overlap[1] and 0 < overlap[1] < 1 << 20)):
        raise ValueError(f"lesion_counts_3d: overlap must be two integers (num, den) with 0 <= num <= den and 0 < den < 2^20, got {overlap!r}")
    mv = _cc3d_min_vox("lesion_counts_3d", min_vox)
    _need_cuda(pred, labels)
    dev = pred.device
    pred, labels = _c(pred), _c(labels)
    ws = _cc3d_ws(Z, H, W, C, dev)
    pc, pa, _, pbad = _cc3d_label_into(pred, labels, C, connectivity, ws)
    gc, ga, _, gbad = _cc3d_label_into(labels, None, C, connectivity, ws)
    counts = torch.empty((C, 4), dtype=torch.int64, device=dev)
    check(lib.dinox_cc3d_match(_p(pred), _p(pc), _p(pa), _p(labels), _p(gc), _p(ga), mv, _p(counts), _p(ws), Z, H, W, C, int(overlap[0]),
                               int(overlap[1]), _stream()), "dinox_cc3d_match")
    nbad = torch.stack([pbad.sum(), gbad.sum()]).tolist()
    _cc_refuse("lesion_counts_3d", "pred", nbad[0], C)
    _cc_refuse("lesion_counts_3d", "labels", nbad[1], C)
    return counts
