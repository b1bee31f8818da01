"""Raw caller of dinox_gemm for the contract tests: builds dinox._lib.GemmArgs straight from the guarded buffers of
oracle/gemm_bounds.py (as ops._gemm_f32_raw does for the fp32 products), so that every field of the argument struct can be set.
ops.gemm is not involved.  args() / kernel_name() / ws_bytes() are host-only (fake pointer values are fine); run() needs a GPU."""
import ctypes as C

import numpy as np

from dinox import _lib
from dinox._lib import BF16, F32, GemmArgs
from oracle import gemm_bounds as GB

VECTOR_STORE = ("gemm_bf16_nt_glds", "gemm_bf16_nt_areg", "gemm_bf16_nt_pp", "gemm_bf16_nt_pp128", "gemm_bf16_nt_pp384")
PP = ("gemm_bf16_nt_pp", "gemm_bf16_nt_pp128", "gemm_bf16_nt_pp384")
FAKE = {"A": 0x100000, "B": 0x200000, "C": 0x300000, "bias": 0x400000, "residual": 0x500000, "aux": 0x600000, "colsum": 0x700000,
        "ws": 0x800000}


def args(s: GB.Spec, ptr: dict, ws: int = 0) -> GemmArgs:
    """ptr: name -> address of the operand's FIRST element (the spec's byte offsets already applied)."""
    return GemmArgs(A=ptr["A"], B=ptr["B"], C=ptr["C"], M=s.M, N=s.N, K=s.K, lda=s.lda, ldb=s.ldb, ldc=s.ldc, batch=s.batch,
                    strideA=s.stride_a, strideB=s.stride_b, strideC=s.stride_c, transA=s.trans, transB=s.tb,
                    in_dtype=BF16 if s.in_ == "bf16" else F32,
                    out_dtype=BF16 if s.out == "bf16" else F32, epilogue=s.epi, alpha=s.alpha,
                    bias=ptr["bias"] if s.epi & GB.BIAS else None, residual=ptr["residual"] if s.epi & GB.RESIDUAL else None, ldr=s.ldr,
                    aux=ptr["aux"] if s.aux else None, ldaux=s.ldaux, colsum=ptr["colsum"] if s.colsum else None, ws=ws or None)


def fake_ptrs(s: GB.Spec) -> dict:
    p = dict(FAKE)
    p["A"] += s.off_a
    p["B"] += s.off_b
    p["C"] += s.off_c
    return p


def kernel_name(s: GB.Spec, ptr: dict = None, ws: int = 0) -> str:
    g = args(s, ptr or fake_ptrs(s), ws)
    return _lib.lib.dinox_gemm_kernel_name(C.byref(g)).decode()


def ws_bytes(s: GB.Spec, ptr: dict = None) -> int:
    g = args(s, ptr or fake_ptrs(s), 0)
    return int(_lib.lib.dinox_gemm_ws_bytes(C.byref(g)))


def admits(kernel: str, s: GB.Spec, ws: bool) -> bool:
    """The envelope each kernel DOCUMENTS (include/dinox.h, the _ok predicates' comments), restricted to what the contract cases vary:
    may `kernel`, forced by its knobs at one of its own shapes, take these arguments?"""
    e = s.epi
    esz = 2 if s.out == "bf16" else 4
    aligned = not (s.off_a % 16 or s.off_b % 16 or s.lda % 8 or s.ldb % 8 or s.stride_a % 8 or s.stride_b % 8)
    if kernel == "gemm_f32":
        return True
    if not aligned:
        return False
    if kernel in VECTOR_STORE:
        if s.trans or e & GB.ACCUM or s.off_c % 16 or (s.ldc * esz) % 16 or (s.stride_c * esz) % 16:
            return False
        if e & GB.RESIDUAL and s.ldr % 4:
            return False
        if e & (GB.GELU | GB.DGELU) and s.aux and (s.ldaux * esz) % 16:
            return False
        if kernel != "gemm_bf16_nt_glds" and s.batch != 1:
            return False
        if kernel != "gemm_bf16_nt_glds" and e & GB.RESIDUAL and e & (GB.GELU | GB.DGELU):
            return False
        if kernel in PP and s.aux and not e & GB.AUXGRAD:
            return False
        if kernel == "gemm_bf16_nt_pp384" and (e & (GB.GELU | GB.DGELU) or (e & GB.RESIDUAL and s.out != "f32")):
            return False
        return True
    if kernel == "gemm_bf16_nt":
        return not s.trans
    if kernel == "gemm_bf16_tn_big":
        return bool(s.trans) and ws and s.batch == 1 and s.pad_c == 0 and s.out == "f32" and not e & ~GB.ACCUM
    if kernel == "gemm_bf16_tn_dma":
        return bool(s.trans)
    raise KeyError(kernel)


def _torch_of(a: np.ndarray):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def _upload(bufs: dict):
    dev = {k: _torch_of(b.data).to("cuda") for k, b in bufs.items()}
    ptr = {k: dev[k].data_ptr() + bufs[k].origin * bufs[k].data.itemsize for k in bufs}
    for k in ("bias", "residual", "aux", "colsum"):
        ptr.setdefault(k, 0)
    return dev, ptr


def _download(s: GB.Spec, bufs: dict, dev: dict) -> dict:
    after = {}
    for k in GB.OUTPUTS:
        if k in bufs and GB.is_output(s, k):
            a = dev[k].cpu().numpy()
            after[k] = a.view(np.uint16) if bufs[k].data.dtype == np.uint16 else a
    return after


def pieces(s: GB.Spec, by: str):
    """The product of `s` cut into launches of their own: by = "item", one per batch item; by = "strip", one per 128 columns of N
    (batch = 1).  Yields (spec of the piece -- shape and batch only, for the tile-form predicate --, batch item, first column)."""
    if by == "item":
        for b in range(s.batch):
            yield s.but(batch=1), b, 0
    else:
        assert by == "strip" and s.batch == 1
        for n0 in range(0, s.N, 128):
            yield s.but(N=min(128, s.N - n0)), 0, n0


def run_pieces(s: GB.Spec, bufs: dict, by: str):
    """The same product as run(s, bufs), from the same buffers, as the launches of pieces(): every pointer is moved to the piece's
    first element and nothing else changes (leading dimensions stay).  Returns {output name: raw array after all launches}."""
    import torch
    assert not s.colsum
    dev, ptr = _upload(bufs)
    ein, eout = (2 if s.in_ == "bf16" else 4), (2 if s.out == "bf16" else 4)
    for sp, b, n0 in pieces(s, by):
        p = dict(ptr)
        p["A"] += b * s.stride_a * ein
        p["B"] += (b * s.stride_b + n0 * (1 if s.tb else s.ldb)) * ein
        p["C"] += (b * s.stride_c + n0) * eout
        p["bias"] += n0 * 4
        p["residual"] += (b * s.M * s.ldr + n0) * 4
        p["aux"] += (b * s.M * s.ldaux + n0) * eout
        g = args(s, p, 0)
        g.N, g.batch = sp.N, 1
        _lib.check(_lib.lib.dinox_gemm(C.byref(g), None), "dinox_gemm")
    torch.cuda.synchronize()
    return _download(s, bufs, dev)


def run(s: GB.Spec, bufs: dict, use_ws: bool = False):
    """One launch on cuda:0 from the buffers as built (they are not modified).  Returns (kernel name, {output name: raw array after
    the launch}, workspace bytes used).  The workspace, when asked for and when dinox_gemm_ws_bytes grants one, is filled with NaN."""
    import torch
    dev, ptr = _upload(bufs)
    g = args(s, ptr, 0)
    need = int(_lib.lib.dinox_gemm_ws_bytes(C.byref(g))) if use_ws else 0
    ws = None
    if need:
        ws = torch.full(((need + 3) // 4 + 64,), float("nan"), dtype=torch.float32, device="cuda")
        g.ws = ws.data_ptr()
    name = _lib.lib.dinox_gemm_kernel_name(C.byref(g)).decode()
    _lib.check(_lib.lib.dinox_gemm(C.byref(g), None), "dinox_gemm")
    torch.cuda.synchronize()
    return name, _download(s, bufs, dev), need
