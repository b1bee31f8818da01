"""oracle/gemm_bounds.py judged on the CPU, and the host-only half of the dinox_gemm contract.

1. The bound is neither vacuous nor too tight: the kernels' documented arithmetic (float32 accumulation of the exact bf16 products in
   two summation orders, float32 epilogue with the fast erf, bf16 rounding), emulated in NumPy, lies inside the bound on EVERY
   element of every case family the GPU tests run -- and each planted defect (GB.MUTANTS) is flagged on at least one element or
   canary word.  No element is exempt from the comparison: check() reports how many it compared and that must be all of them.
2. The dispatcher (dinox_gemm_kernel_name / dinox_gemm_ws_bytes on fake pointer values, nothing is dereferenced) never names a
   kernel whose predicate excludes the argument.
"""
import numpy as np
import pytest

import _gemm_raw as R
from oracle import gemm_bounds as GB

FAMILIES = dict(GB.cpu_families())


@pytest.fixture(scope="module")
def built():
    """name -> (spec, buffers, reference), computed once and left unchanged."""
    out = {}
    for name, s in FAMILIES.items():
        bufs = GB.build(s)
        out[name] = (s, bufs, GB.reference(s, bufs))
    return out


def _n_outputs(s, bufs):
    return sum(bufs[k].idx.size for k in GB.OUTPUTS if k in bufs and GB.is_output(s, k))


def test_constants_are_what_the_docstring_says():
    plain, hw = GB.measure_erf_as()
    print(f"erf_as: float32 formula alone {plain:.3e}, with one ulp of rcp and exp {hw:.3e}; ERF_AS_ERR = {GB.ERF_AS_ERR:.3e}")
    assert 1.0e-7 < plain < hw <= GB.ERF_AS_ERR < 1.25 * hw          # the constant covers the measurement and is not padded
    lg, ld = GB.lipschitz_constants()
    assert lg <= GB.L_GELU < lg * 1.0001 and ld <= GB.L_DGELU < ld * 1.0001
    import torch
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * np.float32(3.0)
    want = torch.from_numpy(x).to(torch.bfloat16)
    assert (GB.bf16_round(x).view(np.int16) == want.view(torch.int16).numpy()).all()
    assert (GB.bf16_to_f64(GB.bf16_round(x)) == want.double().numpy()).all()
    assert GB.bf16_round(np.array([1.00390625, 1.01171875], dtype=np.float32)).tolist() == [0x3F80, 0x3F82]     # ties to even


@pytest.mark.parametrize("order", ["seq", "blk32"])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_documented_arithmetic_is_inside_the_bound(built, name, order):
    s, bufs, ref = built[name]
    r = GB.check(s, bufs, GB.emulate(s, bufs, order), ref)
    print(f"GEMM-CONTRACT-CPU {name} {order}: " + " ".join(f"{k}={v:.3g}" for k, v in r.items() if k.startswith("ratio")))
    assert r["compared"] == _n_outputs(s, bufs) and r["exempt"] == 0
    assert r["ok"], r
    # (worst-case accumulation, gamma_K, grows with K where the rounding errors of real data grow with sqrt K: at K = 8232 the emulation
    #  uses 1e-4 of the bound and eight dropped k-terms still show, see the mutants; at short K the bound must be within 200 x)
    if s.K <= 64:
        assert r["ratio"] > 5e-3, f"the bound is vacuous on {name}: the emulated arithmetic uses {r['ratio']:.2e} of it"


# which family shows which planted defect (every mutant is tried on every family it applies to; it must be flagged on these)
MUTANT_FAMILIES = {
    "drop_last_8k": ["strided-bias", "tn-accum-colsum", "tn-long-k"],
    "alpha_ignored": ["alpha-bias", "alpha-accum"],
    "bias_shift_last_strip": ["strided-bias", "strided-gelu-aux", "alpha-accum"],
    "accum_overwrites": ["alpha-accum", "tn-accum-colsum"],
    "ldr_taken_as_n": ["strided-residual", "batched-shared-b-residual"],
    "ldaux_taken_as_n": ["strided-gelu-aux", "strided-gelu-auxgrad-f32", "batched-shared-a-gelu"],
    "batch1_uses_b0": ["batched-own-b"],
    "bf16_truncated": ["strided-bias", "strided-gelu-aux", "strided-dgelu"],
    "canary_word": ["strided-bias", "strided-residual", "tn-long-k"],
}


@pytest.mark.parametrize("mutant,name", [(m, f) for m in GB.MUTANTS for f in MUTANT_FAMILIES[m]])
def test_every_mutant_is_flagged(built, mutant, name):
    s, bufs, ref = built[name]
    r = GB.check(s, bufs, GB.emulate(s, bufs, "blk32", mutant), ref)
    print(f"GEMM-CONTRACT-CPU mutant {mutant} on {name}: ratio={r['ratio']:.3g} nan={r['nan']} canary={r['canary']}")
    assert not r["ok"], f"{mutant} on {name} passes: {r}"
    if mutant == "canary_word":
        assert r["canary"] == 1 and r["ratio"] <= 1.0
    if mutant == "ldaux_taken_as_n":
        assert r["canary"] > 0                        # the misplaced rows land in the padding columns
    if mutant == "bias_shift_last_strip":
        assert r["where_C"][2] >= s.N - 8             # flagged inside the last strip, nowhere else


def test_input_padding_is_poison_and_output_padding_is_canary():
    s = FAMILIES["batched-shared-b-residual"]
    bufs = GB.build(s)
    for k, b in bufs.items():
        pad = np.ones(b.data.shape, dtype=bool)
        pad[b.idx.reshape(-1)] = False
        assert pad[:GB.GUARD].all() and pad[-GB.GUARD:].all() and pad.sum() > 2 * GB.GUARD
        if GB.is_output(s, k):
            assert (b.words()[pad] == (GB.CANARY_BF16 if b.data.dtype == np.uint16 else GB.CANARY_F32)).all()
        else:
            vals = GB.bf16_to_f64(b.data[pad]) if b.data.dtype == np.uint16 else b.data[pad]
            assert np.isnan(vals).all() and np.isfinite(b.live()).all()
    assert bufs["B"].idx.shape[0] == 3 and (bufs["B"].idx[0] == bufs["B"].idx[2]).all()          # shared operand: stride 0
    # a kernel that reads one padding column poisons its result
    s2 = s.but(K=s.K + 1, pad_a=GB.PADS["pad_a"] - 1, pad_b=GB.PADS["pad_b"] - 1)               # same layout, one column too many
    got = GB.reference(s2, {**bufs, "A": GB.Buf(bufs["A"].data, bufs["A"].origin, GB.build(s2)["A"].idx, False),
                            "B": GB.Buf(bufs["B"].data, bufs["B"].origin, GB.build(s2)["B"].idx, False)}, with_bound=False)
    assert np.isnan(got["C"]).all()


# ------------------------------------------------------------------------------------------ dispatcher, host only
def _setenv(monkeypatch, kernel):
    for k in ("DINOX_NT_PP", "DINOX_NT_PP384", "DINOX_NT_AREG_MAXK", "DINOX_FC1_AREG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in GB.FORCE[kernel].items():
        monkeypatch.setenv(k, v)


FORCED_NT = {k: v[-1] for k, v in GB.NT_SHAPES.items()}


@pytest.mark.parametrize("kernel", list(FORCED_NT))
def test_forced_kernel_is_named_and_refuses_what_its_predicate_excludes(monkeypatch, kernel):
    _setenv(monkeypatch, kernel)
    M, N, K = FORCED_NT[kernel]
    base = GB.Spec(M, N, K, out="bf16", **GB.PADS)
    assert R.kernel_name(base) == kernel
    assert R.kernel_name(base.but(out="f32", epi=GB.BIAS | GB.RESIDUAL)) == kernel
    no_batch = ("gemm_bf16_nt_areg",) + R.PP
    no_accum = ("gemm_bf16_nt_glds", "gemm_bf16_nt_areg") + R.PP
    # batch = 2
    got = R.kernel_name(base.but(batch=2))
    assert (got not in no_batch) and (got == kernel) == (kernel not in no_batch), got
    # ACCUM
    got = R.kernel_name(base.but(out="f32", epi=GB.ACCUM))
    assert got not in no_accum and (got == kernel) == (kernel not in no_accum), got
    # C or the side tensor off 16-byte alignment; rows of C / the side tensor / the residual that break the vector accesses; lda
    fake = R.fake_ptrs(base)
    aux = base.but(epi=GB.GELU | GB.AUXGRAD, aux=True)
    refused = {
        "C + 8": R.kernel_name(base.but(off_c=8)),
        "aux + 8": R.kernel_name(aux, {**fake, "aux": fake["aux"] + 8}),
        "ldc * esz % 16": R.kernel_name(base.but(pad_c=4)),
        "ldaux * esz % 16": R.kernel_name(aux.but(pad_x=4)),
        "ldr % 4": R.kernel_name(base.but(out="f32", epi=GB.RESIDUAL, pad_r=5)),
        "residual + 8": R.kernel_name(base.but(out="f32", epi=GB.RESIDUAL), {**fake, "residual": fake["residual"] + 8}),
    }
    for why, got in refused.items():
        assert got not in R.VECTOR_STORE, (why, got)
    for why, sp in {"lda % 8": base.but(pad_a=4), "ldb % 8": base.but(pad_b=4), "A + 8": base.but(off_a=8), "B + 8": base.but(off_b=8)}.items():
        assert R.kernel_name(sp) == "gemm_f32", why
    # the side tensor without AUXGRAD never reaches a ping-pong kernel, in either direction
    for sp in (base.but(epi=GB.BIAS | GB.GELU, aux=True), base.but(epi=GB.DGELU, aux=True)):
        assert R.kernel_name(sp) not in R.PP
        assert (R.kernel_name(sp) == kernel) == R.admits(kernel, sp, False)
    if kernel in R.PP and kernel != "gemm_bf16_nt_pp384":
        assert R.kernel_name(aux) == kernel and R.kernel_name(base.but(epi=GB.DGELU | GB.AUXGRAD, aux=True)) == kernel


def test_every_contract_case_goes_where_the_documented_envelope_says(monkeypatch):
    """admits() -- the envelope as documented -- against the dispatcher, for every case the GPU tests will launch."""
    n = 0
    for kernel in GB.KERNELS:
        _setenv(monkeypatch, kernel)
        ws = kernel == "gemm_bf16_tn_big"
        for gen in (GB.strided_cases, GB.batched_cases, GB.alpha_cases):
            for name, s in gen(kernel):
                got = R.kernel_name(s, ws=R.FAKE["ws"] if ws else 0)
                assert (got == kernel) == R.admits(kernel, s, ws), (kernel, name, got)
                n += 1
    assert n > 180


def test_tn_workspace_exactly_when_the_deterministic_reduction_applies(monkeypatch):
    _setenv(monkeypatch, "gemm_bf16_tn_dma")
    for (M, N, K) in [(136, 72, 1000), (64, 72, 8192 + 40), (1536, 384, 102912)]:
        s = GB.Spec(M, N, K, trans=1, out="f32", pad_a=8, pad_b=24)
        assert R.ws_bytes(s) > 0 and R.ws_bytes(s.but(epi=GB.ACCUM)) > 0 and R.ws_bytes(s.but(colsum=True)) > R.ws_bytes(s)
        assert R.ws_bytes(s.but(pad_c=16)) == 0                                  # ldc != N
        assert R.ws_bytes(s.but(batch=2)) == 0                                   # batch > 1
        assert R.ws_bytes(s.but(out="bf16")) == 0 and R.ws_bytes(s.but(epi=GB.BIAS)) == 0
        # and the big-tile kernel, which exists only through the workspace, is never named without it or outside that envelope
        for sp, ws in [(s, 0), (s.but(pad_c=16), 1), (s.but(batch=2), 1), (s.but(epi=GB.BIAS), 1), (s.but(out="bf16"), 1)]:
            assert R.kernel_name(sp, ws=R.FAKE["ws"] * ws) != "gemm_bf16_tn_big"
    assert R.ws_bytes(GB.Spec(136, 72, 200, trans=1, out="f32")) == 0            # one split: nothing to reduce
    assert R.kernel_name(GB.Spec(64, 72, 8192 + 40, trans=1, out="f32", pad_a=8), ws=R.FAKE["ws"]) == "gemm_bf16_tn_big"
    assert R.ws_bytes(GB.Spec(133, 136, 384)) == 0                               # NT products need none
