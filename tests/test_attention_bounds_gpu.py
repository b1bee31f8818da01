"""The attention kernels against the ELEMENTWISE float64 bounds of oracle/attention_bounds.py, on inputs whose softmax is not the
diffuse one of randn data (a row maximum that rises to the last key tile, or never moves; scores near +80; a dominant key in the
ragged last tile; near-one-hot rows), at the smallest shape that reaches each kernel path.  dQ, dK and dV are judged separately, and
the backward against float64 GIVEN the kernel's own o and lse.  A failure names (image, head, token, column): which tile, which
operand, padded row or not.  Every case prints its measured err / bound ("Attention bounds", is filled from these lines).
"""
import pytest
import torch

from oracle import attention_bounds as AB

pytestmark = pytest.mark.gpu

DEV = "cuda"

# (B, N, heads, d) -> the path it is the smallest shape of
BF16_PATHS = {
    (3, 19, 2, 64): "persistent forward, 1 tile",
    (2, 33, 2, 64): "2 tiles, one valid key in the last",
    (2, 130, 2, 64): "two-pass persistent, 3 to 6 tiles",
    (2, 201, 6, 64): "hot path: one-pass 7 tiles, fused backward",
    (2, 224, 2, 64): "no padding",
    (1, 261, 2, 64): "non-persistent forward, two-kernel backward",
    (1, 289, 2, 64): "first length on the tiled forward, whole-strip backward",
    (1, 545, 1, 64): "first length on the tiled backward",
    (1, 609, 2, 88): "96-column images, 9 chunks + 33 rows",
    (1, 333, 1, 128): "128-column images",
    (2, 290, 2, 40): "zero-padded head columns",
    (2, 70, 2, 8): "narrowest head the tiled kernels take",
    (2, 37, 2, 20): "per-lane reference kernels in bf16",
}
FP32_PATHS = {
    (2, 37, 2, 20): "fp32 per-lane reference kernels, odd head",
    (2, 201, 2, 64): "fp32 per-lane reference kernels",
    (8, 530, 1, 64): "fp32 product form with softmax rows",
}
_ID = lambda s: "x".join(map(str, s))


@pytest.fixture(scope="module")
def ops():
    from dinox import ops as O
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()
    return O


def _report(tag, shape, case, r):
    print(f"BOUNDS-GPU {tag} {_ID(shape)} {case}: " + " ".join(f"{k}={v:.3g}" for k, v in sorted(r.items())))


def _core_case(ops, shape, case, dt):
    """Forward and backward of one family at one shape against the bounds; every output is asserted (in lastkey / onehot the dQ and
    dK bounds are the fp32 noise term alone: still a bound, if a loose one)."""
    B, N, h, d = shape
    fp32 = dt == torch.float32
    qkv = AB.make_qkv(case, B, N, h, d, seed=N + d, dtype=dt)
    do = AB.make_do(B, N, h, d, seed=N + d, dtype=dt)
    fb = AB.forward_bounds(qkv, h, fp32)
    Q, DO = qkv.to(DEV), do.to(DEV)
    o, lse = ops.attention_fwd(Q, h)
    dqkv = ops.attention_bwd(DO, Q, o, lse, h)
    torch.cuda.synchronize()
    o, lse, dqkv = o.cpu(), lse.cpu(), dqkv.cpu()
    what = f"{'fp32' if fp32 else 'bf16'} {shape} {case}"
    bb = AB.backward_bounds(do, qkv, o, lse, h, fp32)
    # measure everything first, then assert: one line per case whatever fails
    dq, dk, dv = AB.split_dqkv(dqkv, h)
    r = {"o": AB.ratio(AB.heads_first(o, h), fb["o"], fb["o_bound"])[0], "lse": AB.ratio(lse, fb["lse"], fb["lse_bound"])[0],
         "lse_err": float((lse.double() - fb["lse"]).abs().max()),
         "dq": AB.ratio(dq, bb["dq"], bb["dq_bound"])[0], "dk": AB.ratio(dk, bb["dk"], bb["dk_bound"])[0],
         "dv": AB.ratio(dv, bb["dv"], bb["dv_bound"])[0]}
    _report("fp32" if fp32 else "bf16", shape, case, r)
    AB.check_forward(o, lse, fb, h, what)
    AB.check_backward(dqkv, bb, h, what)


@pytest.mark.parametrize("case", AB.FAMILIES)
@pytest.mark.parametrize("shape", list(BF16_PATHS), ids=_ID)
def test_bf16_attention_within_elementwise_bounds(ops, shape, case):
    _core_case(ops, shape, case, torch.bfloat16)


@pytest.mark.parametrize("case", AB.FAMILIES)
@pytest.mark.parametrize("shape", list(FP32_PATHS), ids=_ID)
def test_fp32_attention_within_elementwise_bounds(ops, shape, case):
    _core_case(ops, shape, case, torch.float32)


@pytest.mark.parametrize("case", AB.FAMILIES)
@pytest.mark.parametrize("B,N", [(2, 201), (2, 193)])
def test_fused_qkv_attention_within_elementwise_bounds(ops, B, N, case):
    """dinox_qkv_attention_fwd on x, w whose product has the family's softmax (AB.make_xw): o and lse against float64 on the bf16 qkv
    rows the kernel hands over (what its attention phase saw); the handed-over rows themselves against x w^T to a bf16 rounding."""
    h, d, D = 2, 64, 128
    assert ops.qkv_attention_ok(B, N, h, D, h * d)
    x, w = AB.make_xw(case, B, N, h, d, D, seed=N)
    o, qkv, lse = ops.qkv_attention(x.to(DEV), w.to(DEV), None, h, want_qkv=True, want_lse=True)
    torch.cuda.synchronize()
    o, qkv, lse = o.cpu(), qkv.cpu(), lse.cpu()
    qkv64 = x.double() @ w.double().t()
    perr = (qkv.double() - qkv64).abs()
    assert bool((perr <= AB.U_BF16 * qkv64.abs() + 2.0 ** -12 * (x.double().abs() @ w.double().abs().t())).all()), f"qkv hand-over: max err {float(perr.max()):.3g}"
    fb = AB.forward_bounds(qkv, h)
    r = {"o": AB.ratio(AB.heads_first(o, h), fb["o"], fb["o_bound"])[0], "lse": AB.ratio(lse, fb["lse"], fb["lse_bound"])[0],
         "lse_err": float((lse.double() - fb["lse"]).abs().max())}
    _report("fused", (B, N, h, d), case, r)
    AB.check_forward(o, lse, fb, h, f"fused qkv+attention {(B, N, h, D)} {case}")


@pytest.mark.parametrize("B,N,heads,D", [(2, 201, 6, 384), (2, 193, 2, 96)])
def test_fused_qkv_attention_equals_the_forward_on_its_own_rows(ops, B, N, heads, D):
    """The attention phase of dinox_qkv_attention_fwd is, by its own comment, exactly the persistent forward's one-pass block: the two
    are separate copies of that text, and this pins them together.  dinox_attention_fwd on the qkv rows the fused kernel handed over
    gives the same o and lse bit for bit (7 key tiles, padded last tile: 201 and 193 tokens)."""
    C = heads * 64
    assert ops.qkv_attention_ok(B, N, heads, D, C)
    g = torch.Generator().manual_seed(N + D)
    x = (torch.randn(B, N, D, generator=g) * 0.7).bfloat16().to(DEV)
    w = (torch.randn(3 * C, D, generator=g) * (1.5 / D ** 0.5)).bfloat16().to(DEV)
    o, qkv, lse = ops.qkv_attention(x, w, None, heads, want_qkv=True, want_lse=True)
    o2, lse2 = ops.attention_fwd(qkv, heads)
    torch.cuda.synchronize()
    assert torch.equal(o, o2), f"o: {int((o != o2).sum())} of {o.numel()} elements differ"
    assert torch.equal(lse, lse2), f"lse: {int((lse != lse2).sum())} of {lse.numel()} elements differ"


# ------------------------------------------------------------------------------------------ padding
GUARD = 4096          # elements on either side of every output (a multiple of 8: the 16-byte alignment of the kernels holds)


def _guarded(n, dtype, fill):
    big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return big, big[GUARD:GUARD + n]


def _guards_intact(big, n, fill, what):
    ref = torch.full((GUARD,), fill, dtype=big.dtype, device=DEV)
    assert torch.equal(big[:GUARD], ref), f"{what}: written before its first element"
    bad = (big[GUARD + n:] != ref).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} elements written past the last token, the first {int(bad[0])} elements past the end"


# every bf16 path; fp32 takes the same per-lane kernels at every small shape, so: its three shapes and the one-tile one
PAD_CASES = [(s, "bf16") for s in BF16_PATHS] + [(s, "fp32") for s in FP32_PATHS] + [((3, 19, 2, 64), "fp32")]


@pytest.mark.parametrize("shape,mode", PAD_CASES, ids=lambda v: _ID(v) if isinstance(v, tuple) else v)
def test_attention_writes_nothing_past_the_last_token(ops, shape, mode):
    """The kernels work on 32-row tiles and 64-row chunks; o, lse and dqkv end at the last token.  Outputs sit inside over-allocated
    buffers of guard values: the guards survive, the payload is fully written (no guard value left in it) and equals the plain call."""
    B, N, h, d = shape
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    C = h * d
    qkv = AB.make_qkv("randn", B, N, h, d, seed=N, dtype=dt).to(DEV)
    do = AB.make_do(B, N, h, d, seed=N, dtype=dt).to(DEV)
    FILL = -12288.0                                            # exact in bf16, far outside every output's range
    o_big, o = _guarded(B * N * C, dt, FILL)
    l_big, lse = _guarded(B * h * N, torch.float32, FILL)
    g_big, dqkv = _guarded(B * N * 3 * C, dt, FILL)
    o, lse, dqkv = o.view(B, N, C), lse.view(B, h, N), dqkv.view(B, N, 3 * C)
    o_ref, lse_ref = ops.attention_fwd(qkv, h)
    dqkv_ref = ops.attention_bwd(do, qkv, o_ref, lse_ref, h)
    if ops._use_f32_products(qkv, N, d):
        ops._attention_fwd_f32_products(qkv, h, o, lse)
        ops._attention_bwd_f32_products(do, qkv, o, lse, h, dqkv)
    else:
        ws = torch.empty(ops.lib.dinox_attention_bwd_ws_bytes(B, N, h), dtype=torch.uint8, device=DEV)
        code, st = ops._code(dt), ops._stream()
        ops.check(ops.lib.dinox_attention_fwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), B, N, h, d, code, st), "dinox_attention_fwd")
        ops.check(ops.lib.dinox_attention_bwd(do.data_ptr(), qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), ws.data_ptr(), B, N, h, d,
                                              code, st), "dinox_attention_bwd")
    torch.cuda.synchronize()
    for big, view, ref, name in ((o_big, o, o_ref, "o"), (l_big, lse, lse_ref, "lse"), (g_big, dqkv, dqkv_ref, "dqkv")):
        _guards_intact(big, view.numel(), FILL, f"{mode} {shape} {name}")
        assert not bool((view == FILL).any()), f"{mode} {shape} {name}: elements left unwritten"
        assert torch.equal(view, ref), f"{mode} {shape} {name}: differs from the plain call"


@pytest.mark.parametrize("B,N", [(2, 201), (2, 193)])
def test_fused_qkv_attention_writes_nothing_past_the_last_token(ops, B, N):
    h, d, D = 2, 64, 128
    C = h * d
    x, w = AB.make_xw("randn", B, N, h, d, D, seed=N)
    x, w = x.to(DEV), w.to(DEV)
    FILL = -12288.0
    o_big, o = _guarded(B * N * C, torch.bfloat16, FILL)
    q_big, qkv = _guarded(B * N * 3 * C, torch.bfloat16, FILL)
    l_big, lse = _guarded(B * h * N, torch.float32, FILL)
    o_ref, qkv_ref, lse_ref = ops.qkv_attention(x, w, None, h, want_qkv=True, want_lse=True)
    ops.check(ops.lib.dinox_qkv_attention_fwd(x.data_ptr(), w.data_ptr(), None, o.data_ptr(), qkv.data_ptr(), lse.data_ptr(), B, N, h, d, D,
                                              ops._stream()), "dinox_qkv_attention_fwd")
    torch.cuda.synchronize()
    for big, view, ref, name in ((o_big, o, o_ref, "o"), (q_big, qkv, qkv_ref, "qkv"), (l_big, lse, lse_ref, "lse")):
        _guards_intact(big, view.numel(), FILL, f"fused {(B, N)} {name}")
        assert not bool((view == FILL).any()), f"fused {(B, N)} {name}: elements left unwritten"
        assert torch.equal(view, ref.reshape(-1)), f"fused {(B, N)} {name}: differs from the plain call"
