"""csrc/gemm_f32.hip and dinox_colsum held to elementwise float64 bounds and to the two claims their comments make.

gemm_f32 is what the fp32 parity mode multiplies with, what every bf16 product the MFMA kernels refuse falls back to, and what the
KoLeo, NT-Xent and fp32 attention inner products run on; its header calls it the on-GPU reference of the bf16 kernels.  Here, through
tests/_gemm_raw.py on the guarded buffers of oracle/gemm_bounds.py:

* every (transA, transB) x operand type x output type, every epilogue, padded leading dimensions; K around the K-step of two and the
  16-slab; both tile forms, each case on the side of launch_gemm_f32's line it was written for (GB.uses_big_tiles mirrors the
  predicate; the library names both forms "gemm_f32"); the split-K argument form whose batch items overlap; colsum through dinox_gemm.
  Per case: every element inside its bound, no NaN (input padding is NaN), no canary word changed, a second launch bit-identical.
* claim (a), "bit-identical to the kernel above": each 128-tile product again as launches that the predicate sends to the 64-tile
  kernel (one per batch item, or one per 128-column strip) -- equal bytes.
* claim (b), "a k-ordered fmaf chain per output": equal bits to acc = fma32(a_k, b_k, acc), k ascending, on the CPU.
* colsum_kernel against tests/_colsum_emul.py bit for bit, and against float64 within gamma_{ceil(M/16) + 6} sum |x|.
* the two Python split-reduction paths (ops.gemm with transA and transB at K >= 4096, ops.gemm_nt_f32_splitk).

Every case prints `GEMM-F32-CONTRACT <form> <case>: ratio=...`; the gemm_f32 rows of DESIGN.md ("GEMM argument contract") are the
maxima of those lines.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _colsum_emul as CS
import _gemm_raw as R
from oracle import gemm_bounds as GB

pytestmark = pytest.mark.gpu

_REF = {}
_RUN = {}


@pytest.fixture(scope="module", autouse=True)
def device():
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in ("DINOX_NT_PP", "DINOX_NT_PP384", "DINOX_NT_AREG_MAXK", "DINOX_FC1_AREG"):
        monkeypatch.delenv(k, raising=False)


def _built(s):
    """Buffers and float64 reference of a spec, computed once per module and left unchanged."""
    if s not in _REF:
        bufs = GB.build(s)
        _REF[s] = (bufs, GB.reference(s, bufs))
    return _REF[s]


def _first_launch(s):
    if s not in _RUN:
        _RUN[s] = R.run(s, _built(s)[0])
    return _RUN[s]


def _form(s):
    return "128-tile" if GB.uses_big_tiles(s) else "64-tile"


def _judge(s, family, case, big=False):
    assert GB.uses_big_tiles(s) == big, f"{case}: written for the {'128' if big else '64'}-tile kernel, the predicate says otherwise"
    bufs, ref = _built(s)
    name, after, ws = _first_launch(s)
    r = GB.check(s, bufs, after, ref)
    print(f"GEMM-F32-CONTRACT {_form(s)} {family} {case}: in={s.in_} out={s.out} K={s.K} ratio={r['ratio']:.3g} " +
          " ".join(f"{k}={v:.3g}" for k, v in r.items() if k.startswith("ratio_")) + f" nan={r['nan']} canary={r['canary']}")
    assert name == "gemm_f32" and ws == 0, (case, name)
    assert r["compared"] == sum(bufs[k].idx.size for k in after) and r["exempt"] == 0
    assert r["nan"] == 0, (case, r)
    assert r["canary"] == 0, (case, r["canary_at"])
    assert r["ratio"] <= 1.0, (case, {k: v for k, v in r.items() if k.startswith(("ratio", "where"))})
    _, again, _ = R.run(s, bufs)
    for k in after:
        assert np.array_equal(after[k].view(np.uint8), again[k].view(np.uint8)), f"{case}: {k} differs on a second launch"
    return r


@pytest.mark.parametrize("case,s", [pytest.param(n, s, id=n) for n, s in GB.f32_layout_cases()])
def test_layouts_types_epilogues(case, s):
    _judge(s, "layout", case)


@pytest.mark.parametrize("case,s", [pytest.param(n, s, id=n) for n, s in GB.f32_k_edge_cases()])
def test_k_edges(case, s):
    _judge(s, "kedge", case)


@pytest.mark.parametrize("case,big,s", [pytest.param(n, b, s, id=n) for n, b, s in GB.f32_big_cases()])
def test_both_sides_of_the_tile_dispatch(case, big, s):
    _judge(s, "big", case, big)


@pytest.mark.parametrize("case,big,s", [pytest.param(n, b, s, id=n) for n, b, s in GB.f32_overlapped_stride_cases()])
def test_overlapped_batch_strides(case, big, s):
    _judge(s, "overlapped", case, big)


@pytest.mark.parametrize("case,s", [pytest.param(n, s, id=n) for n, s in GB.f32_colsum_cases()])
def test_colsum_through_gemm(case, s):
    _judge(s, "colsum", case)
    bufs, _ = _built(s)
    A = bufs["A"].live()[0].astype(np.float32)                                       # stored [K][M]: its column sums
    cs_in = bufs["colsum"].live().reshape(-1).astype(np.float32) if s.epi & GB.ACCUM else None
    got = _first_launch(s)[1]["colsum"][bufs["colsum"].idx.reshape(-1)]
    assert np.array_equal(got.view(np.uint32), CS.colsum32(A, cs_in).view(np.uint32)), case


# ------------------------------------------------------------------------------------------ claim (a): one arithmetic, two tilings
@pytest.mark.parametrize("case,s", [pytest.param(n, s, id=n) for n, b, s in list(GB.f32_big_cases()) + list(GB.f32_overlapped_stride_cases()) if b])
def test_big_tiles_are_bit_identical_to_small_tiles(case, s):
    """'results are bit-identical to the kernel above' (csrc/gemm_f32.hip): the 128-tile launch against the same product as launches
    the predicate keeps on the 64-tile kernel -- one per batch item (4 tiles), or one per 128-column strip (16 tiles)."""
    by = "item" if s.batch > 1 else "strip"
    assert GB.uses_big_tiles(s) and all(not GB.uses_big_tiles(sp) for sp, _, _ in R.pieces(s, by))
    bufs, _ = _built(s)
    _, whole, _ = _first_launch(s)
    parts = R.run_pieces(s, bufs, by)
    for k in whole:
        same = np.array_equal(whole[k].view(np.uint8), parts[k].view(np.uint8))
        if not same:
            live = bufs[k].idx.reshape(-1)
            n = int((whole[k][live] != parts[k][live]).sum())
            raise AssertionError(f"{case}: {k} of the 128-tile launch differs from the 64-tile launches in {n} of {live.size} elements")


# ------------------------------------------------------------------------------------------ claim (b): the fma chain
def _chain(A, B):
    """acc = fma32(a_k, b_k, acc), k ascending: A [M][K], B [N][K] float32 -> [M][N]."""
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=np.float32)
    for k in range(A.shape[1]):
        acc = GB.fma32(A[:, k, None], B[None, :, k], acc)
    return acc


_CHAIN = [(f"33x40x{K}", GB.Spec(33, 40, K, out="f32", in_="f32", seed=150 + K, pad_a=3, pad_b=7, pad_c=5)) for K in (1, 2, 3, 17, 33)] + \
         [("129x130x37b64", next(s for n, _, s in GB.f32_big_cases() if n == "129x130x37b64-00-f32-own_b"))]


@pytest.mark.parametrize("case,s", [pytest.param(n, s, id=n) for n, s in _CHAIN])
def test_result_is_a_k_ordered_fma_chain(case, s):
    """'bit-for-bit a k-ordered fmaf chain per output': epi = 0, alpha = 1, fp32 in and out (alpha = 1 and the absent bias leave the
    accumulator as it is)."""
    assert s.epi == 0 and s.alpha == 1.0 and s.in_ == "f32" and s.out == "f32" and s.trans == 0 and s.tb == 0
    bufs, _ = _built(s)
    _, after, _ = _first_launch(s)
    A, B = GB._operands(s, bufs)
    want = _chain(A[0].astype(np.float32), B[0].astype(np.float32))
    got = after["C"][bufs["C"].idx[0]]
    diff = got.view(np.uint32) != want.view(np.uint32)
    print(f"GEMM-F32-CONTRACT {_form(s)} chain {case}: {int(diff.sum())} of {diff.size} elements differ from the fma chain")
    assert not diff.any(), (case, int(diff.sum()), np.argwhere(diff)[:4].tolist())


# ------------------------------------------------------------------------------------------ the column-sum kernel on its own
@pytest.mark.parametrize("case,M,N,ldx,bf16,accumulate", [pytest.param(*c, id=c[0]) for c in CS.cases()])
def test_colsum_kernel_bits_and_bound(case, M, N, ldx, bf16, accumulate):
    import torch
    import dinox._lib as L
    raw, live, out, out_in = CS.build(M, N, ldx, bf16, accumulate)
    want = CS.colsum32(live, out_in)
    ref, bound = CS.reference(live, out_in)
    x = R._torch_of(raw).to("cuda")
    results = []
    for _ in range(2):
        o = torch.from_numpy(out.copy()).to("cuda")
        L.check(L.lib.dinox_colsum(x.data_ptr() + CS.GUARD * raw.itemsize, o.data_ptr() + CS.GUARD * 4, M, N, ldx, L.BF16 if bf16 else L.F32,
                                   int(accumulate), None), "dinox_colsum")
        torch.cuda.synchronize()
        results.append(o.cpu().numpy())
    got = results[0]
    words = got.view(np.uint32)
    assert (words[:CS.GUARD] == CS.CANARY_F32).all() and (words[CS.GUARD + N:] == CS.CANARY_F32).all(), case
    v = got[CS.GUARD:CS.GUARD + N]
    assert np.isfinite(v).all(), case
    ratio = float((np.abs(v.astype(np.float64) - ref) / bound).max())
    nbits = int((v.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"GEMM-F32-CONTRACT colsum {case}: ratio={ratio:.3g} bit-differences={nbits}")
    assert ratio <= 1.0, (case, ratio)
    assert nbits == 0, f"{case}: {nbits} of {N} columns differ from the emulated order"
    assert np.array_equal(results[0].view(np.uint8), results[1].view(np.uint8)), case


# ------------------------------------------------------------------------------------------ the Python split-reduction paths
class _Spy:
    """ops.lib with dinox_gemm's arguments recorded."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def dinox_gemm(self, ref, stream):
        g = ref._obj
        self.calls.append(dict(batch=g.batch, K=g.K, lda=g.lda, strideA=g.strideA, strideB=g.strideB, M=g.M, N=g.N))
        return self._real.dinox_gemm(ref, stream)


def _ops_splits(M, N, K):
    """The split count ops.gemm's fp32 transA/transB branch documents: min(K / 1024, 1024 / tiles), walked down to a divisor of K."""
    tiles = -(-M // 128) * -(-N // 128)
    n = max(1, min(K // 1024, 1024 // tiles))
    while n > 1 and K % n:
        n -= 1
    return n


@pytest.fixture(scope="module")
def tt_operands():
    """(A [K][M], B [K][N], C_in, colsum_in) float32 per (M, N, K), drawn once."""
    out = {}
    for M, N in ((5, 3), (130, 72)):
        for K in (4096, 4100, 4099):
            rng = np.random.default_rng(M * 7 + K)
            out[M, N, K] = tuple(rng.standard_normal(sh).astype(np.float32) for sh in ((K, M), (K, N), (M, N), (M,)))
    return out


@pytest.mark.parametrize("accumulate,with_colsum", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("K", [4096, 4100, 4099])
@pytest.mark.parametrize("M,N", [(5, 3), (130, 72)])
def test_ops_gemm_split_reduction(monkeypatch, tt_operands, M, N, K, accumulate, with_colsum):
    import torch
    import dinox.ops as ops
    A, B, c_in, cs_in = tt_operands[M, N, K]
    splits = _ops_splits(M, N, K)
    assert (splits > 1) == (K != 4099) and K % splits == 0
    spy = _Spy(ops.lib)
    monkeypatch.setattr(ops, "lib", spy)
    monkeypatch.setattr(ops, "TRACE_KERNELS", [])
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    results = []
    for _ in range(2):
        out = torch.from_numpy(c_in.copy()).cuda() if accumulate else torch.full((M, N), float("nan"), device="cuda")
        cs = (torch.from_numpy(cs_in.copy()).cuda() if accumulate else torch.full((M,), float("nan"), device="cuda")) if with_colsum else None
        ops.gemm(dA, dB, transA=True, transB=True, out=out, accumulate=accumulate, colsum_out=cs)
        torch.cuda.synchronize()
        results.append((out.cpu().numpy(), None if cs is None else cs.cpu().numpy()))
    assert ops.TRACE_KERNELS == ["gemm_f32", "gemm_f32"]
    for call in spy.calls:                                                          # one launch per call: batched exactly when split
        assert (call["batch"], call["K"]) == (splits, K // splits), call
        if splits > 1:
            assert call["strideA"] == (K // splits) * M and call["strideB"] == (K // splits) * N and call["lda"] == M
    assert len(spy.calls) == 2
    got, got_cs = results[0]
    ref, bound = GB.splitk_reference(A.T.astype(np.float64), B.T.astype(np.float64), splits, c_in if accumulate else None)
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"GEMM-F32-CONTRACT ops.gemm-tt {M}x{N}x{K} splits={splits} acc={int(accumulate)} colsum={int(with_colsum)}: ratio={ratio:.3g}")
    assert np.isfinite(got).all() and ratio <= 1.0, ratio
    assert np.array_equal(results[0][0].view(np.uint8), results[1][0].view(np.uint8))
    if with_colsum:
        want = CS.colsum32(A, cs_in if accumulate else None)
        assert np.array_equal(got_cs.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(results[1][1].view(np.uint32), want.view(np.uint32))


@pytest.fixture(scope="module")
def nt_operands():
    out = {}
    for M, N, K in ((40, 24, 1024), (129, 130, 1152)):
        rng = np.random.default_rng(M + K)
        out[M, N, K] = (rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32))
    return out


@pytest.mark.parametrize("M,N,K,asked,splits", [(40, 24, 1024, 0, 4), (40, 24, 1024, 3, 2), (40, 24, 1024, 5, 4),
                                                (129, 130, 1152, 0, 4), (129, 130, 1152, 3, 3)])
def test_ops_gemm_nt_f32_splitk(monkeypatch, nt_operands, M, N, K, asked, splits):
    """Auto splits = min(K / 256, 256 / tiles) walked down to a divisor (1024: 4; 1152 with 4 tiles: 4); a request that does not
    divide K walks down too (3 -> 2 and 5 -> 4 at K = 1024)."""
    import torch
    import dinox.ops as ops
    A, B = nt_operands[M, N, K]
    spy = _Spy(ops.lib)
    monkeypatch.setattr(ops, "lib", spy)
    monkeypatch.setattr(ops, "TRACE_KERNELS", [])
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    got = [ops.gemm_nt_f32_splitk(dA, dB, asked).cpu().numpy() for _ in range(2)]
    assert ops.TRACE_KERNELS == ["gemm_f32", "gemm_f32"]
    assert [(c["batch"], c["K"], c["lda"], c["strideA"], c["strideB"]) for c in spy.calls] == [(splits, K // splits, K, K // splits, K // splits)] * 2
    ref, bound = GB.splitk_reference(A.astype(np.float64), B.astype(np.float64), splits)
    ratio = float((np.abs(got[0] - ref) / bound).max())
    print(f"GEMM-F32-CONTRACT ops.splitk {M}x{N}x{K} asked={asked} splits={splits}: ratio={ratio:.3g}")
    assert np.isfinite(got[0]).all() and ratio <= 1.0, ratio
    assert np.array_equal(got[0].view(np.uint8), got[1].view(np.uint8))
