"""Every bf16 GEMM kernel against the full dinox_gemm argument contract, element by element (oracle/gemm_bounds.py).

Each kernel is forced by its knobs (csrc/knobs.h) at the smallest shape that still has a full tile, a ragged edge in M and N and an
8-column last strip, and the traced kernel name is asserted, so no case passes on a fallback.  Where a kernel's predicate does not
admit an argument (tests/_gemm_raw.py, admits()), the dispatcher must name another kernel and the result must still be inside the
bound.  Per case: every element of C, of the written side tensor and of colsum within the bound, no NaN (input padding is NaN: a
kernel that uses it poisons its result), every canary word of the output padding intact bit for bit, and -- everything except the
fp32-atomics path of the split-K TN kernel -- a second launch bit-identical to the first.

gemm_bf16_tn, the non-DMA form of the TN kernel, is reachable only with an operand of 2 GB or more (K * ld * 2 >= 2^31): left out.

Every case prints `GEMM-CONTRACT <kernel named> <variant> <case>: ratio=...`, the largest |got - ref| / bound over all its outputs;
the table in DESIGN.md ("GEMM argument contract") is the per-kernel maximum of those lines.
"""
import numpy as np
import pytest

import _gemm_raw as R
from oracle import gemm_bounds as GB

pytestmark = pytest.mark.gpu

KERNELS = GB.KERNELS
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def device():
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()


def _force(monkeypatch, kernel):
    for k in ("DINOX_NT_PP", "DINOX_NT_PP384", "DINOX_NT_AREG_MAXK", "DINOX_FC1_AREG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in GB.FORCE[kernel].items():
        monkeypatch.setenv(k, v)


def _built(s):
    """Buffers and float64 reference of a spec, computed once per module and left unchanged."""
    if s not in _REF:
        bufs = GB.build(s)
        _REF[s] = (bufs, GB.reference(s, bufs))
    return _REF[s]


def _judge(s, variant, case, expect=None, refuse=None, use_ws=False):
    bufs, ref = _built(s)
    name, after, ws = R.run(s, bufs, use_ws)
    r = GB.check(s, bufs, after, ref)
    print(f"GEMM-CONTRACT {name} {variant} {case}: out={s.out} K={s.K} ratio={r['ratio']:.3g} " +
          " ".join(f"{k}={v:.3g}" for k, v in r.items() if k.startswith("ratio_")) + f" nan={r['nan']} canary={r['canary']} ws={ws}")
    if expect is not None:
        assert name == expect, f"{variant} {case}: dispatched to {name}, the case is for {expect}"
    if refuse is not None:
        assert name != refuse, f"{variant} {case}: {refuse} does not admit these arguments and was named"
    assert r["compared"] == sum(bufs[k].idx.size for k in after) and r["exempt"] == 0
    assert r["nan"] == 0, (name, case, r)
    assert r["canary"] == 0, (name, case, r["canary_at"])
    assert r["ratio"] <= 1.0, (name, case, {k: v for k, v in r.items() if k.startswith(("ratio", "where"))})
    atomics = bool(s.trans) and name.startswith("gemm_bf16_tn") and ws == 0 and s.K > 256 and s.out == "f32" and not (s.epi & ~GB.ACCUM)
    if not atomics:
        name2, again, _ = R.run(s, bufs, use_ws)
        assert name2 == name
        for k in after:
            assert np.array_equal(after[k].view(np.uint8), again[k].view(np.uint8)), f"{name} {case}: {k} differs on a second launch"
    return name, r


def _by_envelope(kernel, s, ws):
    return dict(expect=kernel) if R.admits(kernel, s, ws) else dict(refuse=kernel)


def _cases(gen):
    return [pytest.param(k, n, s, id=f"{k[5:]}-{n}") for k in KERNELS for n, s in gen(k)]


@pytest.mark.parametrize("kernel,case,s", _cases(GB.strided_cases))
def test_strided_operands(monkeypatch, kernel, case, s):
    """All of lda / ldb / ldc / ldr / ldaux larger than the width by different amounts; bf16 and fp32 outputs; every epilogue."""
    _force(monkeypatch, kernel)
    ws = kernel == "gemm_bf16_tn_big"
    _judge(s, "strided", case, use_ws=ws, **_by_envelope(kernel, s, ws))


@pytest.mark.parametrize("kernel,case,s", _cases(GB.batched_cases))
def test_batch_of_three(monkeypatch, kernel, case, s):
    """batch = 3: own B, shared B (strideB = 0), shared A, strideC with a gap; side tensor and residual indexed as b * M * ld."""
    _force(monkeypatch, kernel)
    ws = kernel == "gemm_bf16_tn_big"
    _judge(s, "batched", case, use_ws=ws, **_by_envelope(kernel, s, ws))


@pytest.mark.parametrize("kernel,case,s", _cases(GB.alpha_cases))
def test_alpha(monkeypatch, kernel, case, s):
    """alpha in {0.375, -1.5} with bias and with ACCUM."""
    _force(monkeypatch, kernel)
    ws = kernel == "gemm_bf16_tn_big"
    _judge(s, "alpha", case, use_ws=ws, **_by_envelope(kernel, s, ws))


@pytest.mark.parametrize("case,expect,s,ws", [pytest.param(n, k, s, w, id=n) for n, (k, s, w) in GB.accum_cases()])
def test_accum(monkeypatch, case, expect, s, ws):
    """ACCUM on every kernel that takes it: the generic NT kernel, the TN kernels through atomics and through the deterministic
    workspace, gemm_f32 on bf16 operands; colsum under ACCUM; ldc != N with a long K (no workspace is granted, and without ACCUM
    the launcher falls back to one split because it cannot zero a strided C)."""
    _force(monkeypatch, expect)
    name, r = _judge(s, "accum", case, expect=expect, use_ws=ws)
    if "ldc" in case:
        assert R.ws_bytes(s) == 0


@pytest.mark.parametrize("case,s", [pytest.param(n, s, id=n) for n, s in GB.misaligned_cases()])
def test_misaligned_operands(monkeypatch, case, s):
    """Operands and C at an 8-byte (not 16-byte) offset, ldr odd: inside the bound on whatever kernel is named -- and that kernel is
    never one that moves the misaligned operand by 16-byte vectors."""
    _force(monkeypatch, "gemm_f32")
    monkeypatch.delenv("DINOX_NT_PP", raising=False)
    monkeypatch.setenv("DINOX_NT_PP", "1")
    name, r = _judge(s, "misaligned", case)
    if s.off_a or s.off_b:
        assert name == "gemm_f32"
    if s.off_c or s.ldr % 4:
        assert name not in R.VECTOR_STORE
