"""The host half of the workspace contract.

1. tests/_guarded_alloc.py tested on itself: plain-torch stand-in "kernels" on CPU tensors, the unmutated one and one mutant per kind of
   bug the GPU module (tests/test_workspace_contract_gpu.py) is there to see.  Each mutant must be caught by the check named for it, the
   unmutated stand-in must pass all of them, and the cached-workspace mutant shows why the caches are dropped before a guarded call.
2. Every dinox_*_ws_bytes query (host arithmetic): 0 exactly when the documented envelope refuses the shape, positive inside it, a
   multiple of the element size the ops wrapper divides by, never smaller for a larger batch / row / class count, and every section
   offset of the layouts documented beside the query a multiple of that section's element size.
"""
import itertools

import pytest
import torch

import _guarded_alloc as G

ROWS, COLS = 8, 5
_WS_CACHE: dict = {}


# ------------------------------------------------------------------------------------------ the stand-in kernel and its mutants
def standin(x, mutant=None, reduce="sum", cached=False):
    """out[i] = 2 x[i] + r, r = the sum (or fmaxf-style maximum) over ROWS partial row sums that go through a workspace: the shape of the
    two-stage reductions of csrc/.  Allocates as the ops wrappers do, with torch.empty."""
    n = x.numel()
    out = torch.empty(n, dtype=torch.float32)
    if cached:                                                        # as ops._tn_workspace: one buffer, kept between calls
        ws = _WS_CACHE.get("ws")
        if ws is None:
            ws = _WS_CACHE["ws"] = torch.empty(ROWS, dtype=torch.float32)
    else:
        ws = torch.empty(ROWS, dtype=torch.float32)
    filled = ROWS // 2 if mutant in ("half_sum", "half_max") else ROWS
    ws[:filled] = x.reshape(ROWS, COLS).sum(1)[:filled]
    if reduce == "max":
        r = ws[~torch.isnan(ws)].max()                                # fmaxf: a NaN operand is dropped
    else:
        r = ws.sum()
    out[:] = 2 * x.reshape(-1) + r
    if mutant == "past":
        torch.as_strided(out, (n + 1,), (1,))[n] = 1.0                # one element past the output
    if mutant == "before":
        torch.as_strided(out, (1,), (1,), out.storage_offset() - 1)[0] = 1.0
    if mutant == "ws_past":
        torch.as_strided(ws, (ROWS + 1,), (1,), ws.storage_offset())[ROWS] = 1.0
    return out


def make_x():
    x = torch.arange(ROWS * COLS, dtype=torch.float32).reshape(ROWS, COLS) * 0.25 - 1.0
    return x.flip(0).contiguous()                                     # the largest row sums come first: in the half a half_* mutant fills


def failed_checks(x, **kw):
    """The checks of the GPU module on the stand-in: -> the set of those that fail, {"canary", "bits", "poison"} at most."""
    want = standin(x, reduce=kw.get("reduce", "sum"))                 # the unmutated stand-in, unguarded: its result reads no unwritten byte
    bad, outs = set(), {}
    for poison in G.POISONS:
        with G.guarded(poison, drop=False, check=False) as g:
            outs[poison] = standin(x, **kw)
        if g.damaged():
            bad.add("canary")
        if not torch.equal(G.as_bytes(outs[poison]), G.as_bytes(want)):
            bad.add(f"bits 0x{poison:02X}")
    if bool((G.poisoned_elements(outs[0xFF], 0xFF) & G.poisoned_elements(outs[0x7F], 0x7F)).any()):
        bad.add("poison")
    return bad


def test_the_unmutated_standin_passes_every_check():
    x = make_x()
    assert failed_checks(x) == set() and failed_checks(x, reduce="max") == set()
    assert torch.equal(standin(x), 2 * x.reshape(-1) + x.sum())


def test_a_store_one_element_past_the_output_damages_the_rear_canary():
    x = make_x()
    assert failed_checks(x, mutant="past") == {"canary"}
    with pytest.raises(AssertionError, match=r"allocation #0 \(160 bytes, from test_workspace_contract_cpu.py:\d+ in standin\) first at live\+160"):
        with G.guarded(0xFF, drop=False):
            standin(x, mutant="past")


def test_a_store_one_element_before_the_output_damages_the_front_canary():
    x = make_x()
    assert failed_checks(x, mutant="before") == {"canary"}
    with G.guarded(0x7F, drop=False, check=False) as g:
        standin(x, mutant="before")
    (a, at), = g.damaged()
    assert (a.index, a.nbytes, at) == (0, 160, -4)
    with pytest.raises(AssertionError, match=r"first at live-4"):
        g.check()


def test_a_sum_over_a_half_filled_workspace_moves_with_either_poison():
    assert failed_checks(make_x(), mutant="half_sum") == {"bits 0xFF", "bits 0x7F"}


def test_a_maximum_over_a_half_filled_workspace_shows_under_0x7f_only():
    """fmaxf drops the NaN of 0xFF and the written half holds the true maximum: that run is bit-identical to the reference, and the bug is
    seen only because 3.39e38 wins the maximum under 0x7F.  This is why every case runs under both poisons."""
    assert failed_checks(make_x(), mutant="half_max", reduce="max") == {"bits 0x7F"}


def test_a_cached_workspace_bypasses_the_guard_until_the_cache_is_dropped():
    x = make_x()
    _WS_CACHE.clear()
    _WS_CACHE["ws"] = torch.empty(ROWS + 8, dtype=torch.float32)[:ROWS]           # allocated before the guard, with slack behind it
    with G.guarded(0xFF, drop=False, check=False) as g:
        standin(x, mutant="ws_past", cached=True)
    assert len(g) == 1 and not g.damaged()                            # the output alone was guarded: the overrun went unseen
    _WS_CACHE.clear()                                                 # what drop_caches() does for dinox.ops
    with G.guarded(0xFF, drop=False, check=False) as g:
        standin(x, mutant="ws_past", cached=True)
    (a, at), = g.damaged()
    assert len(g) == 2 and (a.index, a.nbytes, at) == (1, 4 * ROWS, 4 * ROWS)
    _WS_CACHE.clear()


def test_the_helper_restores_torch_empty_and_changes_nothing_at_import():
    real = torch.empty
    with pytest.raises(RuntimeError, match="inside"):
        with G.guarded(0xFF, drop=False):
            assert torch.empty is not real
            raise RuntimeError("inside")
    assert torch.empty is real
    with G.guarded(0x7F, drop=False) as g:
        shapes = [torch.empty(3, 5), torch.empty((2, 3), dtype=torch.bfloat16), torch.empty(7, dtype=torch.uint8), torch.empty((), dtype=torch.float64),
                  torch.empty(0, dtype=torch.int64), torch.empty(torch.Size([4]), dtype=torch.int32, device="cpu")]
    assert [tuple(t.shape) for t in shapes] == [(3, 5), (2, 3), (7,), (), (0,), (4,)] and len(g) == 6
    assert all(t.data_ptr() % 256 == 0 and t.is_contiguous() for t in shapes)
    assert shapes[0][0, 0].item() == pytest.approx(3.39615e38, rel=1e-5) and shapes[5].tolist() == [0x7F7F7F7F] * 4
    assert float(shapes[1][0, 0]) > 1e38 and torch.isfinite(shapes[1]).all()
    with G.guarded(0xFF, drop=False) as g:
        t, i = torch.empty(4), torch.empty(4, dtype=torch.int16)
    assert torch.isnan(t).all() and i.tolist() == [-1] * 4


def test_dropped_caches_make_the_cached_paths_allocate_again(monkeypatch):
    """ops._tn_workspace (the split-K dW products of ops.gemm and of the native block backward, ops.py `tn_ws = _tn_workspace(...)`) and
    ops._block_tn_ws_bytes (sizes per shape) are the caches a workspace can come from; allocations are counted."""
    from dinox import ops
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    cpu = torch.device("cpu")
    G.drop_caches()
    with G.guarded(0xFF, check=False) as g:
        a = ops._tn_workspace(1000, cpu)
        assert len(g) == 1
        assert ops._tn_workspace(900, cpu) is a and len(g) == 1       # the cache answers: no allocation
    with G.guarded(0x7F, check=False) as g:                           # guarded() drops the caches on entry
        b = ops._tn_workspace(1000, cpu)
        assert len(g) == 1 and b is not a and int(b[0]) == 0x7F
        G.drop_caches()
        assert ops._tn_workspace(1000, cpu) is not b and len(g) == 2
    need = ops._block_tn_ws_bytes(394, 384, 1536)
    assert need > 0 and (394, 384, 1536) in ops._BLOCK_TN_WS
    G.drop_caches()
    assert not ops._BLOCK_TN_WS and not ops._TN_WS


# ------------------------------------------------------------------------------------------ size queries
def lib():
    from dinox import _lib
    return _lib.lib


def ceil_div(a, b):
    return -(-a // b)


def seg_ok(B, g, u, C):
    return 1 <= B <= 1 << 20 and 1 <= g <= 4096 and 1 <= u <= 32 and 2 <= C <= 64 and B * g * g <= 1 << 32


SEG_ARGS = [(B, g, u, C) for B in (0, 1, 2, 3, 7, 1 << 20, (1 << 20) + 1) for g in (0, 1, 2, 3, 14, 4096, 4097) for u in (0, 1, 3, 16, 32, 33)
            for C in (1, 2, 3, 5, 33, 64, 65)]


def check_query(fn, args_list, ok, divisor, grow):
    """0 exactly outside the envelope `ok`; positive multiples of `divisor` inside; monotone in the argument positions `grow`."""
    seen = 0
    for a in args_list:
        n = int(fn(*a))
        assert (n > 0) == bool(ok(*a)) and n >= 0, (fn.__name__, a, n)
        if n:
            seen += 1
            assert n % divisor == 0, (fn.__name__, a, n, divisor)
            for pos in grow:
                b = list(a)
                b[pos] += 1
                if ok(*b):
                    assert int(fn(*b)) >= n, (fn.__name__, a, b)
    assert 0 < seen < len(args_list), fn.__name__                     # the sweep has shapes on both sides of the envelope


def test_seg_loss_queries_and_their_layouts():
    L = lib()
    for fn, lead in ((L.dinox_seg_loss_ws_bytes, 1), (L.dinox_seg_loss_bd_ws_bytes, 2)):
        check_query(fn, SEG_ARGS, seg_ok, 4, (0, 1, 3))               # ops.seg_loss_fwd / seg_loss_bd_fwd allocate bytes // 4 floats
        for B, g, u, C in SEG_ARGS:
            if not seg_ok(B, g, u, C):
                continue
            parts, ncell = ceil_div(B * g * g, 8), B * g * g
            wsi = parts * (lead + 2 * C) * 4                          # wsf float [parts][lead + 2 C] | wsi uint32 [parts][C + 2]
            assert wsi % 4 == 0 and wsi + parts * (C + 2) * 4 <= fn(B, g, u, C) and ncell * 4 * C * 4 <= fn(B, g, u, C)
    # the boundary-sized workspace also holds the plain kernels (w_bd = 0 runs them in it)
    assert all(L.dinox_seg_loss_bd_ws_bytes(*a) >= L.dinox_seg_loss_ws_bytes(*a) for a in SEG_ARGS)


def test_other_segmentation_queries():
    L = lib()
    calib = [a + (nb,) for a in SEG_ARGS[::5] for nb in (0, 1, 10, 15, 64, 65)]
    check_query(L.dinox_seg_calib_ws_bytes, calib, lambda B, g, u, C, NB: seg_ok(B, g, u, C) and 1 <= NB <= 64, 4, (0, 1))

    def refine_ok(B, g, u, C):
        S = g * u
        return seg_ok(B, g, u, C) and B * ceil_div(S, 32) * ceil_div(S, 8) <= 0x7FFFFFFF and B * C * S * S <= 1 << 40
    check_query(L.dinox_seg_refine_ws_bytes, SEG_ARGS, refine_ok, 4, (0, 1, 2, 3))


def test_connected_component_queries():
    L = lib()
    sides = (0, 1, 2, 37, 129, 1024, 1025)

    def cc_ok(limit):
        return lambda B, H, W, C: 1 <= H <= 1024 and 1 <= W <= 1024 and 2 <= C <= 64 and B >= 1 and B * H * W <= limit
    args = [(B, H, W, C) for B in (0, 1, 2, 3, 1023, 1024, 2047, 2048) for H in sides for W in sides for C in (1, 2, 3, 64, 65)]
    check_query(L.dinox_cc_ws_bytes, args, cc_ok((1 << 31) - 1), 8, (0, 1, 2, 3))            # ops._cc_ws: bytes // 8 int64
    check_query(L.dinox_cc3d_ws_bytes, args, cc_ok(1 << 30), 8, (0, 1, 2, 3))                # ops._cc3d_ws: bytes // 8 int64
    assert L.dinox_cc_ws_bytes(2047, 1024, 1024, 3) > 0 and L.dinox_cc_ws_bytes(2048, 1024, 1024, 3) == 0
    assert L.dinox_cc3d_ws_bytes(1024, 1024, 1024, 3) > 0 and L.dinox_cc3d_ws_bytes(1025, 1024, 1024, 3) == 0


def test_distance_queries_and_the_3d_layout():
    L = lib()
    sides = (0, 1, 3, 257, 1024, 1025)
    args = [(B, H, W, C) for B in (0, 1, 2, 3, 1 << 20, (1 << 20) + 1) for H in sides for W in sides for C in (1, 2, 3, 5, 64, 65)]
    base = lambda B, H, W, C: 1 <= B <= 1 << 20 and 1 <= H <= 1024 and 1 <= W <= 1024 and 2 <= C <= 64
    check_query(L.dinox_surface_ws_bytes, args, lambda B, H, W, C: base(B, H, W, C) and B * C * 2 * H <= 1 << 30, 4, (0, 1, 2, 3))
    check_query(L.dinox_signed_distance_ws_bytes, args, lambda B, H, W, C: base(B, H, W, C) and B * C * H <= 1 << 30, 2, (0, 1, 2, 3))
    vols = [(Z, H, W, C) for Z in sides for H in sides for W in sides for C in (1, 2, 5, 64, 65)]
    ok3 = lambda Z, H, W, C: all(1 <= s <= 1024 for s in (Z, H, W)) and 2 <= C <= 64
    check_query(L.dinox_surface3d_ws_bytes, vols, ok3, 4, (0, 1, 2))                         # ops.surface_stats_3d: bytes // 4 floats
    for Z, H, W, C in vols:
        if ok3(Z, H, W, C):                                           # zd uint16 [2][Z][H][W] | g fp32 [2][Z][H][W] | partial fp32 [2][Z] | state uint32
            n = Z * H * W
            g_at, partial_at, state_at = 4 * n, 12 * n, 12 * n + 8 * Z
            assert g_at % 4 == 0 and partial_at % 4 == 0 and state_at % 4 == 0 and state_at < L.dinox_surface3d_ws_bytes(Z, H, W, C)
    # the 2-D surface layout: axis distances uint16 [B C 2][H][W], then the distance planes fp32
    assert all((B * C * 2 * H * W * 2) % 4 == 0 for B, H, W, C in args)


def test_transformer_queries():
    L = lib()
    pos = lambda *a: all(v >= 1 for v in a)
    small = (-1, 0, 1, 2, 3, 33, 209)
    check_query(L.dinox_layernorm_bwd_ws_bytes, [(r, d) for r in small + (1 << 20,) for d in (0, 1, 4, 130, 384, 2052)], pos, 4, (0, 1))
    check_query(L.dinox_attention_bwd_ws_bytes, list(itertools.product(small, (0, 1, 33, 201, 545), (0, 1, 2, 6))), pos, 4, (0, 1, 2))
    # attention_rollout_step: 1 <= N <= 4096 (the launcher's _ok predicate; d is no argument of the query)
    roll_ok = lambda B, N, heads: pos(B, N, heads) and N <= 4096 and L.dinox_attention_rollout_step_ok(B, N, heads, 8) == 1
    check_query(L.dinox_attention_rollout_step_ws_bytes, list(itertools.product(small, (0, 1, 63, 4096, 4097), (0, 1, 3))), roll_ok, 4, (0, 1, 2))
    assert L.dinox_attention_rollout_step_ok(1, 4096, 1, 8) == 1 and L.dinox_attention_rollout_step_ok(1, 4097, 1, 8) == 0
    # scale_embed_bwd: de [V][D] | dhpre [V][h] | gelu(hpre) [V][h], all fp32; refused when (D + h + 16) floats pass 64 KiB
    se_ok = lambda V, h, D: pos(V, h, D) and (D + h + 16) * 4 <= 64 * 1024
    se = list(itertools.product((0, 1, 5, 8), (0, 1, 12, 300, 8000), (0, 1, 50, 384, 8368, 8369)))
    check_query(L.dinox_scale_embed_bwd_ws_bytes, se, se_ok, 4, (0, 1, 2))
    for V, h, D in se:
        if se_ok(V, h, D):
            assert (V * D * 4) % 4 == 0 and (V * (D + h) * 4) % 4 == 0 and V * (D + 2 * h) * 4 == L.dinox_scale_embed_bwd_ws_bytes(V, h, D)
    lora_ok = lambda M, K, N, r: 1 <= M <= 0x7FFFFFFF and 1 <= K <= 1 << 20 and 1 <= N <= 1 << 20 and 1 <= r <= 64
    lora = list(itertools.product((0, 1, 5, 128, 129, 130, 0x7FFFFFFF, 1 << 31), (0, 1, 8, 36, 1 << 20, (1 << 20) + 1), (0, 1, 8, 1152), (0, 1, 16, 64, 65)))
    check_query(L.dinox_lora_grad_ws_bytes, lora, lora_ok, 4, (0, 1, 2, 3))
    check_query(L.dinox_sk_ws_floats, list(itertools.product((-1, 0, 1, 31, 32, 33, 100), (0, 1, 7, 256))), pos, 1, (0, 1))


def test_search_and_probe_queries():
    L = lib()
    pos = lambda *a: all(v >= 1 for v in a)
    big = (1 << 31) - 129
    ns = (0, 1, 3, 5, 65, 300, 4099)
    rr_ok = lambda Nq, Nk, D: pos(Nq, Nk, D) and Nq <= big and Nk <= big       # the launchers refuse Nq, Nk > 2^31 - 129
    rr = list(itertools.product(ns + (big, big + 1), ns + (big, big + 1), (0, 1, 7, 16)))
    check_query(L.dinox_retrieval_ws_bytes, rr, rr_ok, 4, (0, 1))
    check_query(L.dinox_retrieval_rank_windowed_ws_bytes, rr, rr_ok, 4, (0, 1))
    knn_ok = lambda Nq, Nk, D, K: pos(Nq, Nk, D) and 1 <= K <= 32 and Nq <= big and Nk <= big
    check_query(L.dinox_knn_ws_bytes, list(itertools.product(ns + (big, big + 1), ns + (big + 1,), (0, 7), (0, 1, 10, 32, 33))), knn_ok, 8, (0, 1, 3))
    lp_ok = lambda g, F, D, C, K: pos(g, F, D) and 2 <= C <= 64 and 1 <= K <= 32 and F * g * g <= big
    lp = list(itertools.product((0, 1, 3, 16, 46340), (0, 1, 2, 5), (0, 16), (1, 2, 3, 64, 65), (0, 1, 5, 32, 33)))
    check_query(L.dinox_labelprop_ws_bytes, lp, lp_ok, 8, (0, 1, 4))         # patches g^2, context slots F, K; C and D do not enter
    check_query(L.dinox_gram_ws_bytes, list(itertools.product((0, 1, 33, 257, 4099), (0, 1, 7, 129, 1024, 1025))), lambda N, D: N >= 1 and 1 <= D <= 1024,
                4, (0, 1))
    pb_ok = lambda N, D, C: N >= 1 and 1 <= D <= 1024 and 2 <= C <= 32
    pb = list(itertools.product((0, 1, 32, 33, 67, 20000), (0, 1, 7, 65, 1024, 1025), (1, 2, 3, 10, 32, 33)))
    # ops.softmax_probe allocates bytes // 8 + 1 doubles, which covers a size that is 4 mod 8; the fp32 gradients start behind the doubles
    check_query(L.dinox_softmax_probe_ws_bytes, pb, pb_ok, 4, (0, 1, 2))
    for N, D, C in pb:
        if pb_ok(N, D, C):
            groups = min(ceil_div(N, 32), 512)
            n = L.dinox_softmax_probe_ws_bytes(N, D, C)
            assert n == groups * (8 + C * (D + 1) * 4) and (8 * groups) % 8 == 0 and (n // 8 + 1) * 8 >= n
