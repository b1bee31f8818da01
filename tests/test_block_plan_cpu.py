"""CPU checks of dinox_block_plan (csrc/block.hip): the one place that decides which launches of a transformer block run fused.  It is
host logic -- nothing is launched or dereferenced -- so the rules and their DINOX_* switches are pinned here without a GPU, as
tests/test_abi.py pins the GEMM dispatcher through dinox_gemm_kernel_name."""
import pytest
import torch

KNOBS = ("DINOX_ROWLN", "DINOX_ROWLN_PP", "DINOX_ROWLN_FC2", "DINOX_LNBWD_PP", "DINOX_QKV_FUSED")

# (V, N, D, H), heads = D / 64
SHAPES = (
    (512, 201, 384, 1536),      # hot path, M = 102 912
    (128, 201, 384, 1536),      # M = 25 728: below the full-row rule (40 000), above the LayerNorm-backward rule (8192)
    (4, 201, 384, 1536),        # M = 804: below both
    (256, 201, 1024, 4096),     # no width-384 kernel, D > 512
    (512, 261, 384, 1536),      # outside the qkv-fused envelope (193..224 tokens)
)
BF, F32 = torch.bfloat16, torch.float32
# columns of a row below: (train, dtype of the LayerNorm after the block)
CASES = ((0, None), (0, BF), (0, F32), (1, None), (1, BF), (1, F32))

# Expected plans in bf16 mode, one string per case: qkv_fused, fuse_proj_ln, fuse_fc2_ln, fuse_ln_bwd.  Produced at the commit BEFORE
# dinox_block_plan existed, from the predicates of dinox/ops.py it replaces: for each environment a fresh process (they read the
# environment at import) evaluated, over SHAPES x CASES, the four expressions BlockFn used -- no-grad and the qkv-fused width rule and
# ops.qkv_attention_ok(V, N, heads, D, D); the product + LayerNorm rule on (M, D, D); on (M, D, H) with the next LayerNorm's dtype; the
# dX + LayerNorm-backward rule on (M, D, H) and on (M, D, 3 D) -- and the output was pasted here.  (fp32 mode gave 0000 everywhere.)
PARENT = {
    None: (
        ("1101", "1111", "1101", "0101", "0111", "0101"),
        ("1101", "1101", "1101", "0101", "0101", "0101"),
        ("1100", "1100", "1100", "0100", "0100", "0100"),
        ("0000", "0000", "0000", "0000", "0000", "0000"),
        ("0101", "0111", "0101", "0101", "0111", "0101"),
    ),
    ("DINOX_ROWLN", "0"): (
        ("1001", "1001", "1001", "0001", "0001", "0001"),
        ("1001", "1001", "1001", "0001", "0001", "0001"),
        ("1000", "1000", "1000", "0000", "0000", "0000"),
        ("0000", "0000", "0000", "0000", "0000", "0000"),
        ("0001", "0001", "0001", "0001", "0001", "0001"),
    ),
    ("DINOX_ROWLN", "1"): (
        ("1101", "1111", "1111", "0101", "0111", "0111"),
        ("1101", "1111", "1111", "0101", "0111", "0111"),
        ("1100", "1110", "1110", "0100", "0110", "0110"),
        ("0000", "0000", "0000", "0000", "0000", "0000"),
        ("0101", "0111", "0111", "0101", "0111", "0111"),
    ),
    ("DINOX_ROWLN_PP", "0"): (
        ("1101", "1101", "1101", "0101", "0101", "0101"),
        ("1101", "1101", "1101", "0101", "0101", "0101"),
        ("1100", "1100", "1100", "0100", "0100", "0100"),
        ("0000", "0000", "0000", "0000", "0000", "0000"),
        ("0101", "0101", "0101", "0101", "0101", "0101"),
    ),
    ("DINOX_ROWLN_FC2", "0"): (
        ("1101", "1101", "1101", "0101", "0101", "0101"),
        ("1101", "1101", "1101", "0101", "0101", "0101"),
        ("1100", "1100", "1100", "0100", "0100", "0100"),
        ("0000", "0000", "0000", "0000", "0000", "0000"),
        ("0101", "0101", "0101", "0101", "0101", "0101"),
    ),
    ("DINOX_LNBWD_PP", "0"): (
        ("1100", "1110", "1100", "0100", "0110", "0100"),
        ("1100", "1100", "1100", "0100", "0100", "0100"),
        ("1100", "1100", "1100", "0100", "0100", "0100"),
        ("0000", "0000", "0000", "0000", "0000", "0000"),
        ("0100", "0110", "0100", "0100", "0110", "0100"),
    ),
    ("DINOX_LNBWD_PP", "1"): (
        ("1101", "1111", "1101", "0101", "0111", "0101"),
        ("1101", "1101", "1101", "0101", "0101", "0101"),
        ("1101", "1101", "1101", "0101", "0101", "0101"),
        ("0000", "0000", "0000", "0000", "0000", "0000"),
        ("0101", "0111", "0101", "0101", "0111", "0101"),
    ),
    ("DINOX_QKV_FUSED", "0"): (
        ("0101", "0111", "0101", "0101", "0111", "0101"),
        ("0101", "0101", "0101", "0101", "0101", "0101"),
        ("0100", "0100", "0100", "0100", "0100", "0100"),
        ("0000", "0000", "0000", "0000", "0000", "0000"),
        ("0101", "0111", "0101", "0101", "0111", "0101"),
    ),
    ("DINOX_QKV_FUSED", "1"): (
        ("1101", "1111", "1101", "0101", "0111", "0101"),
        ("1101", "1101", "1101", "0101", "0101", "0101"),
        ("1100", "1100", "1100", "0100", "0100", "0100"),
        ("1000", "1000", "1000", "0000", "0000", "0000"),
        ("0101", "0111", "0101", "0101", "0111", "0101"),
    ),
}
# DINOX_ROWLN_PP=1 from the same run.  Its fuse_fc2_ln column is NOT the expectation: the Python copy of the rule had no "=1" case, the
# library's launch choice (dinox_linear_residual_ln) has, and the library's form is the rule (test_rowln_pp_1_follows_the_launch_choice).
PARENT_ROWLN_PP_1 = (
    ("1101", "1111", "1101", "0101", "0111", "0101"),
    ("1101", "1101", "1101", "0101", "0101", "0101"),
    ("1100", "1100", "1100", "0100", "0100", "0100"),
    ("0000", "0000", "0000", "0000", "0000", "0000"),
    ("0101", "0111", "0101", "0101", "0111", "0101"),
)


@pytest.fixture(autouse=True)
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def plan(shape, dt, train, nxt):
    from dinox import ops
    V, N, D, H = shape
    p = ops.block_plan(V, N, D, H, D // 64, dt, train, nxt)
    return f"{p.qkv_fused}{p.fuse_proj_ln}{p.fuse_fc2_ln}{p.fuse_ln_bwd}"


@pytest.mark.parametrize("env", list(PARENT), ids=lambda e: "unset" if e is None else "=".join(e))
def test_plan_equals_the_rules_it_replaced(env, monkeypatch):
    """Every shape x train x next-LayerNorm dtype x compute mode, per environment: the plan is what the Python rules gave.  With nothing set
    this is also the check that the library's full-row predicate (gemm_bf16_nt_pp384_ln_ok) and the Python copy it replaces (K >= 128)
    agree over these shapes."""
    if env is not None:
        monkeypatch.setenv(*env)
    for shape, row in zip(SHAPES, PARENT[env]):
        for (train, nxt), want in zip(CASES, row):
            assert plan(shape, BF, train, nxt) == want, (env, shape, train, nxt)
            assert plan(shape, F32, train, nxt) == "0000", (env, shape, train, nxt)


def test_rowln_pp_1_follows_the_launch_choice(monkeypatch):
    """DINOX_ROWLN_PP=1 ("every shape in the full-row kernel's envelope"): dinox_linear_residual_ln launches the full-row kernel for bf16 y
    at M = 25 728 too, so fc2 + LayerNorm is fused there; fp32 y stays on the 128 x 384 kernel, where fc2 is not worth fusing.  The
    other three flags do not depend on the knob."""
    monkeypatch.setenv("DINOX_ROWLN_PP", "1")
    for shape, row in zip(SHAPES, PARENT_ROWLN_PP_1):
        for (train, nxt), want in zip(CASES, row):
            got = plan(shape, BF, train, nxt)
            assert got[:2] + got[3] == want[:2] + want[3], (shape, train, nxt)
            assert plan(shape, F32, train, nxt) == "0000"
    for train in (0, 1):
        assert plan(SHAPES[1], BF, train, BF)[2] == "1"
        assert plan(SHAPES[1], BF, train, F32)[2] == "0"
        assert plan(SHAPES[0], BF, train, BF)[2] == "1" and plan(SHAPES[0], BF, train, F32)[2] == "0" and plan(SHAPES[1], BF, train, None)[2] == "0"


def test_knobs_are_read_at_every_call(monkeypatch):
    """One process flips each switch between two calls and the plan follows (before dinox_block_plan the Python side read four of the
    five at import)."""
    hot, mid, small, wide = SHAPES[:4]
    assert plan(hot, BF, 1, BF) == "0111"
    monkeypatch.setenv("DINOX_ROWLN", "0")
    assert plan(hot, BF, 1, BF) == "0001"
    monkeypatch.setenv("DINOX_ROWLN", "1")
    assert plan(small, BF, 1, F32) == "0110"
    monkeypatch.delenv("DINOX_ROWLN")
    assert plan(small, BF, 1, F32) == "0100"

    monkeypatch.setenv("DINOX_ROWLN_PP", "0")
    assert plan(hot, BF, 1, BF) == "0101"
    monkeypatch.setenv("DINOX_ROWLN_PP", "1")
    assert plan(mid, BF, 1, BF) == "0111"
    monkeypatch.delenv("DINOX_ROWLN_PP")
    assert plan(mid, BF, 1, BF) == "0101" and plan(hot, BF, 1, BF) == "0111"

    monkeypatch.setenv("DINOX_ROWLN_FC2", "0")
    assert plan(hot, BF, 1, BF) == "0101"
    monkeypatch.delenv("DINOX_ROWLN_FC2")
    assert plan(hot, BF, 1, BF) == "0111"

    assert plan(small, BF, 1, None) == "0100"
    monkeypatch.setenv("DINOX_LNBWD_PP", "1")
    assert plan(small, BF, 1, None) == "0101"
    monkeypatch.setenv("DINOX_LNBWD_PP", "0")
    assert plan(hot, BF, 1, None) == "0100"
    monkeypatch.delenv("DINOX_LNBWD_PP")
    assert plan(hot, BF, 1, None) == "0101"

    assert plan(wide, BF, 0, None) == "0000" and plan(hot, BF, 0, None) == "1101"
    monkeypatch.setenv("DINOX_QKV_FUSED", "1")
    assert plan(wide, BF, 0, None) == "1000" and plan(wide, BF, 1, None) == "0000"
    monkeypatch.setenv("DINOX_QKV_FUSED", "0")
    assert plan(hot, BF, 0, None) == "0101"


def test_bad_arguments_are_errors():
    from dinox import _lib
    p = _lib.BlockPlan()
    assert _lib.lib.dinox_block_plan(4, 201, 384, 1536, 6, _lib.BF16, 0, -1, None) == -1 and "null" in _lib.last_error()
    assert _lib.lib.dinox_block_plan(0, 201, 384, 1536, 6, _lib.BF16, 0, -1, p) == -1
    assert _lib.lib.dinox_block_plan(4, 201, 384, 1536, 6, 7, 0, -1, p) == -1
    assert _lib.lib.dinox_block_plan(4, 201, 384, 1536, 5, _lib.BF16, 0, -1, p) == 0 and p.qkv_fused == 0      # D % heads != 0: no fused kernel
