"""The LayerNorm kernel family on the device, element by element against oracle/ln_bounds.py: every instance of csrc/layernorm.hip
(NV = 1, 2, 4, 8 and their masked-lane edges, the width-384 half-wave kernels, the generic kernels with a short row, a ragged three-trip
row and a multiple of four past the fast path), their grid-stride loops, accumulate = 1 of ln_bwd_reduce, the two product + LayerNorm
kernels behind dinox_linear_residual_ln and the product + LayerNorm-backward epilogue behind dinox_linear_ln_bwd, on the hostile
input families of the oracle.  Per case: mean, rstd, y, dx, the bf16 copy, dgamma and dbeta within their bounds, EVERY element
compared, no NaN, and a second launch bit-identical (no LayerNorm path uses atomics).

Every case prints `LN-BOUNDS <kernel/path> <family> <shape>: ratio=...`, the largest |got - ref| / bound; the table in DESIGN.md
("LayerNorm bounds") is the per-path maximum of those lines.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import ln_bounds as LB

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WIDTHS = [4, 64, 256, 260, 384, 512, 516, 1024, 1028, 2048, 2052, 50, 130]
ROWS = [1, 5, 33]
_CACHE = {}


@pytest.fixture(scope="module")
def ops():
    import dinox._lib as L
    from dinox import ops as O
    assert L.lib.dinox_device_ok() == 1, L.last_error()
    return O


def instance(dim):
    """The kernel instance the dispatch at the bottom of csrc/layernorm.hip picks for a width (16-byte aligned operands)."""
    if dim == 384:
        return "ln_384"
    if dim % 4 == 0 and dim <= 2048:
        nv = math.ceil(dim // 4 / 64)
        return "ln_nv%d" % (1 if nv <= 1 else 2 if nv <= 2 else 4 if nv <= 4 else 8)
    return "ln_generic"


def test_every_instance_has_a_width():
    got = {}
    for d in WIDTHS:
        got.setdefault(instance(d), []).append(d)
    assert got == {"ln_nv1": [4, 64, 256], "ln_nv2": [260, 512], "ln_384": [384], "ln_nv4": [516, 1024], "ln_nv8": [1028, 2048],
                   "ln_generic": [2052, 50, 130]}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.float().cpu().numpy()


def same(a, b):
    return all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(a, b) if p is not None)


def report(path, family, shape, r, extra=""):
    parts = " ".join(f"{k[6:]}={v:.3g}" for k, v in r.items() if k.startswith("ratio_"))
    print(f"LN-BOUNDS {path} {family} {shape}: ratio={r['ratio']:.3g} {parts} nan={r['nan']} compared={r['compared']}{extra}")
    assert r["nan"] == 0, (path, family, shape, r)
    assert r["compared"] == r["expected"], (path, family, shape, r)
    assert r["ratio"] <= 1.0, (path, family, shape, r)


def inputs(family, rows, dim):
    key = (family, rows, dim)
    if key not in _CACHE:
        _CACHE[key] = (LB.make_x(family, rows, dim), *LB.make_params(dim))
    return _CACHE[key]


def run_forward(ops, path, family, rows, dim, eps, odt):
    x, gamma, beta = inputs(family, rows, dim)
    X, G, B = dev(x), dev(gamma), dev(beta)
    out = ops.layernorm_fwd(X, G, B, odt, eps)
    assert same(out, ops.layernorm_fwd(X, G, B, odt, eps)), f"{path} {family}: a second launch differs"
    ref = LB.forward_ref(x, gamma, beta, eps, odt == torch.bfloat16)
    y, mean, rstd = out
    report(path, family, f"{rows}x{dim} eps={eps} {str(odt)[6:]}", LB.check_all({"mean": host(mean), "rstd": host(rstd), "y": host(y)}, ref))
    return mean, rstd


def run_backward(ops, path, xfam, dyfam, rows, dim, eps, dy_bf16, forms=("plain", "add", "alias")):
    x, gamma, beta = inputs(xfam, rows, dim)
    dy = LB.make_dy(dyfam, x, gamma, eps, bf16=dy_bf16)
    add = np.random.default_rng([17, rows, dim]).standard_normal((rows, dim)).astype(np.float32)
    X, G, B, A = dev(x), dev(gamma), dev(beta), dev(add)
    DY = dev(dy).bfloat16() if dy_bf16 else dev(dy)
    _, mean, rstd = ops.layernorm_fwd(X, G, B, torch.float32, eps)
    chain = LB.standalone_chain(rows, dim)
    tag = f"{rows}x{dim} dy={'bf16' if dy_bf16 else 'f32'}"
    kept = None
    for form in forms:
        def launch():
            if form == "plain":
                return ops.layernorm_bwd(DY, X, G, mean, rstd, want_lowp=True)
            buf = A.clone()
            return ops.layernorm_bwd(DY, X, G, mean, rstd, dx=buf if form == "alias" else None, dx_add=buf, want_lowp=True)
        out = launch()
        assert same(out, launch()), f"{path} {xfam}+{dyfam} {form}: a second launch differs"
        if form == "alias":
            assert kept is not None and same(out, kept), f"{path} {xfam}+{dyfam}: dx aliasing dx_add differs from the out-of-place run"
            continue
        kept = out if form == "add" else kept
        ref = LB.backward_ref(dy, x, gamma, host(mean), host(rstd), dx_add=None if form == "plain" else add, chain=chain)
        dx, dw, db, lowp = out
        report(path, f"{xfam}+{dyfam}", f"{tag} {form}", LB.check_all({"dx": host(dx), "lowp": host(lowp), "dgamma": host(dw), "dbeta": host(db)}, ref))


# ------------------------------------------------------------------------------------------ stand-alone kernels
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dim", WIDTHS)
def test_forward(ops, dim, rows):
    """Every x family, both output dtypes, eps 1e-5 and 1e-6: mean, rstd and y inside their bounds."""
    for family in LB.X_FAMILIES:
        for eps in (1e-5, 1e-6):
            for odt in (torch.float32, torch.bfloat16):
                run_forward(ops, f"fwd/{instance(dim)}", family, rows, dim, eps, odt)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dim", WIDTHS)
def test_backward(ops, dim, rows):
    """The four dy families on randn and offset rows, both dy dtypes; dx out of place, with dx_add, and aliasing dx_add (bit-equal)."""
    for xfam in ("randn", "offset"):
        for dyfam in LB.DY_FAMILIES:
            for dy_bf16 in (False, True):
                run_backward(ops, f"bwd/{instance(dim)}", xfam, dyfam, rows, dim, 1e-6 if dy_bf16 else 1e-5, dy_bf16)


@pytest.mark.parametrize("family", ["steps", "const", "tiny", "spike_first", "spike_last"])
def test_backward_hostile_rows(ops, family):
    """The backward on the remaining x families (xh of a constant row is 0 x rstd = 1 / sqrt(eps); of a spike row one element is sqrt(D))."""
    for dim in (64, 384, 516, 130):
        run_backward(ops, f"bwd/{instance(dim)}", family, "randn", 5, dim, 1e-5, False, forms=("plain", "add"))


@pytest.mark.parametrize("rows,dim", [(16384 + 5, 64), (33001, 384)])
def test_forward_grid_stride(ops, rows, dim):
    """More rows than the capped grid has waves: a wave (half wave) walks on to a second row."""
    run_forward(ops, f"fwd/{instance(dim)}/stride", "randn", rows, dim, 1e-5, torch.float32)
    run_forward(ops, f"fwd/{instance(dim)}/stride", "randn", rows, dim, 1e-5, torch.bfloat16)


@pytest.mark.parametrize("rows,dim", [(4096 + 3, 64), (4096 + 3, 512), (33001, 384)])
def test_backward_grid_stride(ops, rows, dim):
    """More rows than LN_MAX_PARTS blocks have waves: the column sums aw / ab carry across a wave's rows."""
    for dyfam in ("randn", "lastrow"):
        run_backward(ops, f"bwd/{instance(dim)}/stride", "randn", dyfam, rows, dim, 1e-5, False, forms=("plain", "add", "alias"))
    run_backward(ops, f"bwd/{instance(dim)}/stride", "randn", "randn", rows, dim, 1e-5, True, forms=("plain",))


@pytest.mark.parametrize("rows,dim", [(33, 64), (230, 384), (33, 130), (4096 + 3, 512)])
def test_accumulate_through_the_c_abi(ops, rows, dim):
    """accumulate = 1 of ln_bwd_reduce: dw / db pre-filled; the result is the pre-fill plus the non-accumulating result to one fp32
    rounding, and inside the bound of the sum."""
    import dinox._lib as L
    x, gamma, beta = inputs("randn", rows, dim)
    dy = LB.make_dy("randn", x, gamma, 1e-5)
    pre = (np.random.default_rng([19, rows, dim]).standard_normal((2, dim)) * 10).astype(np.float32)
    X, G, B, DY = dev(x), dev(gamma), dev(beta), dev(dy)
    _, mean, rstd = ops.layernorm_fwd(X, G, B, torch.float32, 1e-5)

    def launch(accumulate):
        dx = torch.empty_like(X)
        dw, db = dev(pre[0]).clone(), dev(pre[1]).clone()
        ws = torch.empty(L.lib.dinox_layernorm_bwd_ws_bytes(rows, dim), dtype=torch.uint8, device=DEV)
        rc = L.lib.dinox_layernorm_bwd(ops._p(DY), ops._p(X), ops._p(G), ops._p(mean), ops._p(rstd), ops._p(dx), None, None, ops._p(dw), ops._p(db),
                                       ops._p(ws), rows, dim, L.F32, accumulate, ops._stream())
        assert rc == 0, L.last_error()
        torch.cuda.synchronize()
        return dx, dw, db
    dx0, dw0, db0 = launch(0)
    dx1, dw1, db1 = launch(1)
    assert same((dx1, dw1, db1), launch(1)) and torch.equal(dx0, dx1)
    for got, base, p in ((dw1, dw0, pre[0]), (db1, db0, pre[1])):
        want = p.astype(np.float64) + host(base).astype(np.float64)
        assert np.all(np.abs(host(got) - want) <= LB.U32 * np.abs(want) * (1 + 1e-6)), "accumulate: not pre-fill + result to one rounding"
    ref = LB.backward_ref(dy, x, gamma, host(mean), host(rstd), chain=LB.standalone_chain(rows, dim), acc_w=pre[0], acc_b=pre[1])
    report(f"bwd/{instance(dim)}/accumulate", "randn+randn", f"{rows}x{dim}", LB.check_all({"dx": host(dx1), "dgamma": host(dw1), "dbeta": host(db1)}, ref))


def test_width_8196(ops):
    """Past the generic backward's LDS row: the forward is inside the bound, the backward refuses with a message and writes nothing."""
    import dinox._lib as L
    rows, dim = 3, 8196
    mean, rstd = run_forward(ops, "fwd/ln_generic", "randn", rows, dim, 1e-5, torch.float32)
    run_forward(ops, "fwd/ln_generic", "offset", rows, dim, 1e-5, torch.bfloat16)
    x, gamma, beta = inputs("randn", rows, dim)
    X, G, DY = dev(x), dev(gamma), dev(LB.make_dy("randn", x, gamma, 1e-5))
    dx = torch.full_like(X, 7.0)
    lowp = torch.full_like(X, 7.0).bfloat16()
    dw, db = torch.full((dim,), 7.0, device=DEV), torch.full((dim,), 7.0, device=DEV)
    ws = torch.zeros(max(int(L.lib.dinox_layernorm_bwd_ws_bytes(rows, dim)), 16), dtype=torch.uint8, device=DEV)
    rc = L.lib.dinox_layernorm_bwd(ops._p(DY), ops._p(X), ops._p(G), ops._p(mean), ops._p(rstd), ops._p(dx), None, ops._p(lowp), ops._p(dw), ops._p(db),
                                   ops._p(ws), rows, dim, L.F32, 0, ops._stream())
    torch.cuda.synchronize()
    assert rc == L.EUNSUPPORTED and "8196" in L.last_error()
    assert bool((dx == 7.0).all()) and bool((lowp.float() == 7.0).all()) and bool((dw == 7.0).all()) and bool((db == 7.0).all()) and int(ws.sum()) == 0


# ------------------------------------------------------------------------------------------ product + LayerNorm
def full_row_kernel(M, y_f32):
    """Does dinox_linear_residual_ln run on the full-row 208 x 384 kernel under the knobs now set?  Read off dinox_block_plan: for a long
    reduction (K = 1152 > 576) fc2 + LayerNorm is fused exactly when linear_residual_ln_full_row says so (csrc/block.hip)."""
    import dinox._lib as L
    plan = L.BlockPlan()
    assert L.lib.dinox_block_plan(M, 1, 384, 1152, 6, L.BF16, 1, L.F32 if y_f32 else L.BF16, C.byref(plan)) == 0
    return bool(plan.fuse_fc2_ln)


def product_case(M, K, family, bias, residual):
    """bf16 a, w and the fp32 residual that carries the x family; a w^T is small noise on it (none on const and tiny rows, which it would
    turn into something else); without a residual the product is the row."""
    rng = np.random.default_rng([23, M, K, LB._key(family)])
    quiet = family in ("const", "tiny")
    a = LB.to_bf16_values(np.zeros((M, K)) if quiet and residual else rng.standard_normal((M, K)) * 0.5)
    w = LB.to_bf16_values(rng.standard_normal((384, K)) * ((0.02 if residual else 2.0) / math.sqrt(K)))
    b = None if not bias else (np.zeros(384, dtype=np.float32) if quiet else (0.1 * rng.standard_normal(384)).astype(np.float32))
    r = LB.make_x(family, M, 384, seed=K) if residual else None
    return a, w, b, r


@pytest.mark.parametrize("M", [1, 77, 198, 209, 623])
@pytest.mark.parametrize("pp,K,ydt", [("0", 32, torch.bfloat16), ("0", 384, torch.bfloat16), ("0", 32, torch.float32), ("0", 384, torch.float32),
                                      ("0", 1152, torch.bfloat16), ("1", 128, torch.bfloat16), ("1", 384, torch.bfloat16)])
def test_linear_residual_ln(ops, monkeypatch, pp, K, ydt, M):
    """x_out with the GEMM bound; y, mean, rstd with the LayerNorm bound given the kernel's own x_out.  pp = DINOX_ROWLN_PP: 0 = the
    128 x 384 kernel (two-slot ring; four-slot at K = 1152), 1 = the full-row kernel's LayerNorm epilogue (bf16 y, K >= 128)."""
    import dinox._lib as L
    monkeypatch.delenv("DINOX_ROWLN", raising=False)
    monkeypatch.delenv("DINOX_ROWLN_FC2", raising=False)
    monkeypatch.setenv("DINOX_ROWLN_PP", pp)
    assert L.lib.dinox_linear_residual_ln_ok(M, 384, K) == 1 and L.lib.dinox_linear_residual_ln_ok(M, 384, 16) == 0      # 32: the smallest K
    full = full_row_kernel(M, ydt == torch.float32) and K >= 128
    assert full == (pp == "1"), "the case is for the other kernel"
    path = "linear_residual_ln/" + ("pp384_ln" if full else "rowln")
    gamma, beta = LB.make_params(384, seed=K)
    cases = [(f, True, True) for f in LB.X_FAMILIES] + [("randn", True, False), ("randn", False, True)]
    for family, bias, residual in cases:
        a, w, b, r = product_case(M, K, family, bias, residual)
        args = (dev(a).bfloat16(), dev(w).bfloat16(), dev(b), dev(r), dev(gamma), dev(beta), 1e-5, ydt)
        ops.TRACE_KERNELS = []
        try:
            out = ops.linear_residual_ln(*args)
            trace = list(ops.TRACE_KERNELS)
        finally:
            ops.TRACE_KERNELS = None
        assert trace == ["gemm_bf16_rowln"]
        assert same(out, ops.linear_residual_ln(*args)), f"{path} {family}: a second launch differs"
        x_out, y, mean, rstd = out
        pr = LB.product_ref(a, w, b, r)
        fr = LB.forward_ref(host(x_out), gamma, beta, 1e-5, ydt == torch.bfloat16, serial=12 if full else 48, combine=not full)
        ref = {"x": pr["x"], "x_bound": pr["x_bound"], **fr}
        tag = family + ("" if bias else "/nobias") + ("" if residual else "/noresidual")
        report(path, tag, f"M={M} K={K} {str(ydt)[6:]}", LB.check_all({"x": host(x_out), "mean": host(mean), "rstd": host(rstd), "y": host(y)}, ref))


# ------------------------------------------------------------------------------------------ product + LayerNorm backward
def lnbwd_operands(M, K, mode):
    key = ("lnbwd", M, K, mode)
    if key not in _CACHE:
        rng = np.random.default_rng([29, M, K])
        a = rng.standard_normal((M, K)) * 0.5
        if mode == "lastrow":
            a[:-1] = 0.0
        a, w = LB.to_bf16_values(a), LB.to_bf16_values(rng.standard_normal((384, K)) * (2.0 / math.sqrt(K)))
        _CACHE[key] = (a, w, *LB.rounded_dy(a, w))
    return _CACHE[key]


@pytest.mark.parametrize("add", [None, "other", "alias"])
@pytest.mark.parametrize("M,K", [(90, 128), (90, 1152), (1873, 128), (1873, 1152)])
def test_linear_ln_bwd(ops, M, K, add):
    """dy = bf16(a w^T) inside the launch: an element within the accumulation bound of a rounding tie carries one bf16 ulp through the
    backward formulas into the bound (nothing is exempt; the share is printed).  dy randn-like, and living in the last row only."""
    import dinox._lib as L
    assert L.lib.dinox_linear_ln_bwd_ok(M, 384, K) == 1
    tiles = math.ceil(M / 208)
    chain = LB.row_chain(13, tiles, waves=16)
    base = np.random.default_rng([31, M]).standard_normal((M, 384)).astype(np.float32)
    for family in ("randn", "offset", "steps"):
        for mode in ("randn", "lastrow"):
            a, w, dy_ref, ulp, share = lnbwd_operands(M, K, mode)
            x, gamma, beta = inputs(family, M, 384)
            X, G = dev(x), dev(gamma)
            _, mean, rstd = ops.layernorm_fwd(X, G, dev(beta), torch.float32, 1e-5)
            A, W = dev(a).bfloat16(), dev(w).bfloat16()

            def launch():
                buf = None if add is None else dev(base)
                ops.TRACE_KERNELS = []
                try:
                    out = ops.linear_ln_bwd(A, W, X, G, mean, rstd, dx=buf if add == "alias" else None, dx_add=buf, want_lowp=True)
                    assert ops.TRACE_KERNELS == ["gemm_bf16_nt_pp384(ln_bwd)"]
                finally:
                    ops.TRACE_KERNELS = None
                return out
            out = launch()
            assert same(out, launch()), f"linear_ln_bwd {family}+{mode}: a second launch differs"
            ref = LB.backward_ref(dy_ref, x, gamma, host(mean), host(rstd), dx_add=None if add is None else base, chain=chain, dy_ulp=ulp)
            dx, dw, db, lowp = out
            report("linear_ln_bwd/pp384_lnbwd", f"{family}+{mode}", f"M={M} K={K} add={add}",
                   LB.check_all({"dx": host(dx), "lowp": host(lowp), "dgamma": host(dw), "dbeta": host(db)}, ref), extra=f" tie_share={share:.3g}")
