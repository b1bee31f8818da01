"""Workspace contract of the ops wrappers: every scratch buffer and every output they allocate with torch.empty is run with 4096
guard bytes on either side and a poisoned live region (tests/_guarded_alloc.py).

Per entry point and shape, three runs of the wrapper: unguarded, under guarded(0xFF) and under guarded(0x7F).  Asserted:
  (a) every canary byte of every allocation is intact (an undersized workspace or a store past an output lands in a guard);
  (b) every output of the guarded runs equals the unguarded run bit for bit, compared as bytes so that NaN equals NaN (a kernel that
      reads scratch it never wrote moves with the poison; 0x7F is there for max-reductions, which drop the NaN of 0xFF);
  (c) no output element holds the poison in both guarded runs (0xFF.. in one and 0x7F.. in the other: never written; a value that is
      legitimately -1 or NaN shows in one run only and is bit-equal in the other, so it is not flagged).  This stands in for a mask of
      the positions the oracle says are written: every output here is written whole, so the mask would be all ones;
  (d) the unguarded run passes the family's float64 judge, so the reference of (b) is itself checked.
The wrapper must reach the patched torch.empty at least once under the guard (cached workspaces are dropped on entry).

Shapes are the smallest of each family's own test module at which the path still has sections of different type and a ragged count.
Every family prints its largest error / bound ratio once at the end.
"""
import contextlib
import math

import numpy as np
import pytest
import torch

import _guarded_alloc as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RATIOS: dict = {}
SEG_SHAPES = ((1, 4, 1, 2), (2, 3, 1, 5), (3, 16, 3, 33), (2, 2, 1, 64))          # (g, u, B, C)
SEG_SHAPES_2 = ((2, 3, 1, 5), (3, 16, 3, 33))


@pytest.fixture(scope="module", autouse=True)
def device():
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()


# ------------------------------------------------------------------------------------------ the driver
def _flatten(out, prefix="out"):
    """Every tensor of a wrapper's result (tensor, tuple, NamedTuple, dict, nested) as {name: tensor}."""
    if out is None:
        return {}
    if torch.is_tensor(out):
        return {prefix: out}
    if isinstance(out, dict):
        items = out.items()
    elif hasattr(out, "_asdict"):
        items = out._asdict().items()
    elif isinstance(out, (tuple, list)):
        items = enumerate(out)
    else:
        return {}
    flat = {}
    for k, v in items:
        flat.update(_flatten(v, f"{prefix}.{k}"))
    return flat


@contextlib.contextmanager
def _ratios(family, module):
    """Collect what a family module's own judge records (its RATIOS dict) under `family` here, leaving the module's dict as it was."""
    saved, module.RATIOS = module.RATIOS, {}
    try:
        yield
    finally:
        if module.RATIOS:
            RATIOS[family] = max(RATIOS.get(family, 0.0), max(module.RATIOS.values()))
        module.RATIOS = saved


def _record(family, ratio):
    RATIOS[family] = max(RATIOS.get(family, 0.0), float(ratio))


def contract(name, run, judge=None, bit_exact=True):
    """run() -> the wrapper's outputs; judge(outputs) asserts the float64 bound (d).  bit_exact=False: the path is not reproducible (fp32
    atomics); each of its runs is judged instead of compared."""
    base = _flatten(run())
    torch.cuda.synchronize()
    assert base, f"{name}: no output tensor"
    if judge is not None:
        judge(base)
    got = {}
    for poison in G.POISONS:
        with G.guarded(poison) as g:                                   # (a): the canaries are checked when the block ends
            out = run()
        assert len(g) > 0, f"{name}: the wrapper never reached torch.empty under the guard"
        got[poison] = _flatten(out)
        assert got[poison].keys() == base.keys(), name
        if not bit_exact:
            judge(got[poison])
            continue
        for k, ref in base.items():                                    # (b)
            a, b = G.as_bytes(got[poison][k]), G.as_bytes(ref)
            assert a.shape == b.shape, (name, k)
            if not torch.equal(a, b):
                at = int((a != b).nonzero()[0]) // ref.element_size()
                raise AssertionError(f"{name}: output {k} moves with the poison 0x{poison:02X}: first at element {at} of {ref.numel()} "
                                     f"({int((a != b).sum())} bytes differ)")
    for k in base:                                                     # (c)
        never = G.poisoned_elements(got[G.POISON_NAN][k], G.POISON_NAN) & G.poisoned_elements(got[G.POISON_BIG][k], G.POISON_BIG)
        assert not bool(never.any()), f"{name}: output {k} holds the poison in {int(never.sum())} element(s): never written"
    print(f"WS-CONTRACT {name}: {len(g)} guarded allocations, {sum(a.nbytes for a in g.allocations)} bytes, canaries intact, "
          f"{len(base)} outputs bit-identical under both poisons")


def _bound_judge(family, name, got, ref, bound):
    got = got.detach().double().cpu().numpy().reshape(ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    _record(family, ratio)
    assert (err <= bound).all(), f"{name}: error / bound = {ratio:.3g}"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------ segmentation loss
def _seg_inputs(g, u, B, C):
    import test_segloss_gpu as TS
    rng = np.random.default_rng([77, g, u, B, C])
    z = TS.make_logits(rng, "normal", B, g * g, C)
    y = TS.make_labels(rng, "quarter ignored", B, g * u, C)
    return z, y, TS.on_device(z, 0), _dev(y)


@pytest.mark.parametrize("g,u,B,C", SEG_SHAPES)
def test_seg_loss(g, u, B, C):
    import _segloss_oracle as SO
    from dinox import ops
    z, y, zt, yt = _seg_inputs(g, u, B, C)

    def run():
        loss, stats, saved = ops.seg_loss_fwd(zt, yt, 0.7, 1.3, 1)
        return dict(loss=loss, stats=stats, nv=saved[3], dz=ops.seg_loss_bwd(saved, 1.0))

    def judge(o):
        px = SO.Pixels(z, y, g, u)
        fwd = SO.forward(z, y, g, u, 0.7, 1.3, 1, px)
        ref_dz, e_dz = SO.backward(z, y, g, u, 0.7, 1.3, 1, 1.0, px, fwd)
        assert o["out.nv"].cpu().tolist() == [fwd["nv"], 0]
        _bound_judge("seg_loss", "loss", o["out.loss"], fwd["loss"], fwd["e_loss"])
        _bound_judge("seg_loss", "stats", o["out.stats"], fwd["stats"], fwd["e_stats"])
        _bound_judge("seg_loss", "dz", o["out.dz"], ref_dz, e_dz)
    contract(f"seg_loss_fwd/bwd g={g} u={u} B={B} C={C}", run, judge)


@pytest.mark.parametrize("g,u,B,C,w_bd", [s + (0.5,) for s in SEG_SHAPES] + [(2, 3, 1, 5, 0.0)])
def test_seg_loss_bd(g, u, B, C, w_bd):
    """w_bd = 0 puts the plain kernels into the boundary-sized workspace."""
    import _bdloss_oracle as BO
    import _segloss_oracle as SO
    import test_bdloss_gpu as TB
    from dinox import ops
    z, y, zt, yt = _seg_inputs(g, u, B, C)
    spacing = np.random.default_rng([78, g, u]).uniform(0.5, 2.0, (B, 2)).astype(np.float32)
    phi = TB.device_phi(y, spacing, C)
    ph = phi.cpu().numpy()

    def run():
        loss, stats, saved = ops.seg_loss_bd_fwd(zt, yt, phi, 0.7, 1.3, w_bd, 1)
        return dict(loss=loss, stats=stats, nv=saved[4], dz=ops.seg_loss_bd_bwd(saved, 1.0))

    def judge(o):
        px = SO.Pixels(z, y, g, u)
        fwd = BO.forward(z, y, ph, g, u, 0.7, 1.3, w_bd, 1, px)
        ref_dz, e_dz = BO.backward(z, y, ph, g, u, 0.7, 1.3, w_bd, 1, 1.0, px, fwd)
        assert o["out.nv"].cpu().tolist() == [fwd["nv"], 0]
        _bound_judge("seg_loss_bd", "loss", o["out.loss"], fwd["loss"], fwd["e_loss"])
        _bound_judge("seg_loss_bd", "stats", o["out.stats"], fwd["stats"], fwd["e_stats"])
        _bound_judge("seg_loss_bd", "dz", o["out.dz"], ref_dz, e_dz)
    contract(f"seg_loss_bd_fwd/bwd g={g} u={u} B={B} C={C} w_bd={w_bd}", run, judge)


# ------------------------------------------------------------------------------------------ other segmentation
@pytest.mark.parametrize("g,u,B,C", SEG_SHAPES_2)
def test_seg_predict(g, u, B, C):
    import _segloss_oracle as SO
    from dinox import ops
    z, y, zt, yt = _seg_inputs(g, u, B, C)

    def judge(o):
        ref, margin, e_l = SO.predict(z, g, u)
        decided = margin > e_l
        pred = o["out.0"].cpu().numpy()
        assert (pred[decided] == ref[decided]).all() and np.array_equal(o["out.1"].cpu().numpy(), SO.counts(pred, y, C))
    contract(f"seg_predict g={g} u={u} B={B} C={C}", lambda: ops.seg_predict(zt, u, yt), judge)


@pytest.mark.parametrize("g,u,B,C", SEG_SHAPES_2)
def test_seg_calib(g, u, B, C):
    """bins = 10 and s = 0.37: settings of tests/test_segcalib_gpu.py (NBS, SS)."""
    import _segcalib_oracle as CO
    import test_segcalib_gpu as TC
    from dinox import ops
    z, y, zt, yt = _seg_inputs(g, u, B, C)

    def judge(o):
        cal = CO.Calib(z, y, g, u)
        ref = cal.at(0.37)
        with _ratios("seg_calib", TC):
            TC.judge("conf", o["out.conf"].cpu().numpy(), ref["conf"], ref["e_conf"], cal.decided)
            TC.judge("entropy", o["out.entropy"].cpu().numpy(), ref["entropy"], ref["e_entropy"])
            sums = o["out.sums"].cpu().numpy()
            for k, name in enumerate(CO.NAMES):
                TC.judge(f"sum {name}", sums[k:k + 1], ref["sums"][k:k + 1], ref["e_sums"][k:k + 1])
        hist, tail = CO.histogram(o["out.pred"].cpu().numpy(), o["out.conf"].cpu().numpy(), y, C, 10)
        assert np.array_equal(o["out.hist"].cpu().numpy(), hist) and np.array_equal(o["out.tail"].cpu().numpy(), tail)
    contract(f"seg_calib g={g} u={u} B={B} C={C}",
             lambda: ops.seg_calib(zt, u, yt, inv_temperature=0.37, bins=10, want_conf=True, want_entropy=True), judge)


@pytest.mark.parametrize("g,u,B,C", SEG_SHAPES_2)
def test_seg_refine(g, u, B, C):
    """The first "normal" case of tests/test_segrefine_cpu.py that iterates and is not refused at this image side."""
    import _segloss_oracle as SO
    import _segrefine_oracle as RO
    import test_segloss_gpu as TS
    import test_segrefine_cpu as RC
    import test_segrefine_gpu as TR
    from dinox import ops
    i = next(i for i in range(4) if RC.case_params(i)["T"] >= 1 and not RC.refused(RC.case_params(i), g * u))
    p = RC.case_params(i)
    z, guide = RC.normal_case(g, u, B, C, i)
    y = TS.make_labels(np.random.default_rng([79, g, u, B, C]), "quarter ignored", B, g * u, C)
    zt, gt, yt = TS.on_device(z, 0), TS.on_device(guide, 0), _dev(y)

    def judge(o):
        pred, conf = o["out.0"].cpu().numpy(), o["out.1"].cpu().numpy()
        assert np.array_equal(o["out.2"].cpu().numpy(), SO.counts(pred, y, C))
        with _ratios("seg_refine", TR):
            TR.against_oracle("conf", z, guide, g, u, p, pred, conf)
    contract(f"seg_refine g={g} u={u} B={B} C={C} case {i}", lambda: ops.seg_refine(zt, gt, u, yt, want_conf=True, **TR.op_kwargs(p)), judge)


# ------------------------------------------------------------------------------------------ connected components
@pytest.mark.parametrize("conn", (4, 8))
@pytest.mark.parametrize("H,W", ((1, 37), (33, 65), (63, 129)))
def test_cc(H, W, conn):
    import _cc_oracle as CO
    import test_cclabel_gpu as TCC
    from dinox import ops
    rng = np.random.default_rng([80, H, W, conn])
    m, y = TCC.random_map(rng, 2, H, W, 3), TCC.random_map(rng, 2, H, W, 3, p255=0.1)
    mt, yt = _dev(m), _dev(y)

    def run():
        return dict(label=ops.cc_label(mt, 3, conn), filter=ops.cc_filter(mt, 3, connectivity=conn, min_px=[3, 6], keep_largest=True, targets=yt),
                    match=ops.lesion_counts(mt, yt, 3, connectivity=conn, overlap=(1, 2)))

    def judge(o):
        TCC.agree([o[f"out.label.{i}"] for i in range(3)], CO.label_flood(m, 3, conn), f"({H}, {W}) conn {conn}")
        want = CO.cc_filter(m, 3, connectivity=conn, min_px=[3, 6], keep_largest=True)
        assert np.array_equal(o["out.filter.0"].cpu().numpy(), want)
        assert o["out.filter.1"].cpu().tolist() == CO.overlap_counts(want, y, 3)[0].tolist()
        assert o["out.match"].cpu().tolist() == CO.lesion_counts(m, y, 3, connectivity=conn, overlap=(1, 2)).tolist()
        _record("cc (exact)", 0.0)
    contract(f"cc_label/filter/match {H}x{W} conn {conn}", run, judge)


@pytest.mark.parametrize("conn", (6, 26))
@pytest.mark.parametrize("name", ("small", "partial", "corner"))
def test_cc3d(name, conn):
    import _cc3d_oracle as O
    import test_cclabel3d_gpu as T3
    from dinox import ops
    v = T3._volume(name)
    gt = O.noise(v.shape, seed=8)
    vt, gtt = _dev(v), _dev(gt)

    def run():
        return dict(label=ops.cc_label_3d(vt, 3, conn), filter=ops.cc_filter_3d(vt, 3, min_vox=2, keep_largest=True, connectivity=conn, targets=gtt),
                    match=ops.lesion_counts_3d(vt, gtt, 3, connectivity=conn, overlap=(1, 2)))

    def judge(o):
        T3._equal([o[f"out.label.{i}"] for i in range(3)], T3._want(name, conn, False), (name, conn))
        want = O.cc_filter(v, 3, min_vox=2, keep_largest=True, connectivity=conn)
        assert np.array_equal(o["out.filter.0"].cpu().numpy(), want)
        assert np.array_equal(o["out.filter.1"].cpu().numpy(), O.overlap_counts(want, gt, 3)[0])
        assert np.array_equal(o["out.match"].cpu().numpy(), O.lesion_counts(v, gt, 3, conn, (1, 2)))
        _record("cc3d (exact)", 0.0)
    contract(f"cc3d_label/filter/match {name} conn {conn}", run, judge)


# ------------------------------------------------------------------------------------------ distance maps and surface distances
@pytest.mark.parametrize("B,H,W", ((1, 3, 257), (2, 37, 70), (1, 1, 1)))
def test_signed_distance(B, H, W):
    import _bdloss_oracle as BO
    import test_bdloss_gpu as TB
    from dinox import ops
    rng = np.random.default_rng([81, B, H, W])
    y = TB.make_map("blobs", rng, B, H, W, 3)
    spacing = rng.uniform(0.4, 2.5, (B, 2)).astype(np.float32)
    yt, st = _dev(y), torch.from_numpy(spacing)

    def judge(o):
        with _ratios("signed_distance", TB):
            TB.judge_phi(f"({B}, {H}, {W})", o["out"], BO.signed_distance(y, spacing, 3))
    contract(f"signed_distance B={B} {H}x{W} C=3", lambda: ops.signed_distance_map(yt, st, 3), judge)


@pytest.mark.parametrize("H,W", ((33, 17), (40, 130)))
def test_surface_stats(H, W):
    import test_surface_gpu as TSF
    from dinox import ops
    pred, gt, D = TSF.case(H, W, 5)
    pt, gtt, sp = _dev(pred), _dev(gt), torch.from_numpy(TSF.SPACINGS).to(DEV)
    tol, paired = TSF.TOLERANCES[0]

    def judge(o):
        with _ratios("surface_stats", TSF):
            TSF.judge(f"({H}, {W})", o["out.0"], o["out.1"], D.stats(tol, (95, 100)), paired)
    contract(f"surface_stats {H}x{W} C=5", lambda: ops.surface_stats(pt, gtt, sp, 5, tolerances=tol, q=(95, 100)), judge)


@pytest.mark.parametrize("Z,H,W", ((1, 1, 1), (2, 3, 5)))
def test_surface3d_stats(Z, H, W):
    """(1, 1, 1) is the smallest case of tests/test_surface3d_gpu.py; (2, 3, 5), the next one, has an odd Z H W (the fp32 partials start
    at 12 Z H W bytes) and more than one slice."""
    import test_surface3d_gpu as T3
    from dinox import ops
    pred, gt, oracles = T3.case(Z, H, W, 5)
    pt, gtt = _dev(pred), _dev(gt)
    (sp, tol), D = T3.PAIRS[0], oracles[0]

    def judge(o):
        with _ratios("surface3d_stats", T3):
            T3.judge(f"({Z}, {H}, {W})", o["out.0"], o["out.1"], D.stats(tol, (95, 100)))
    contract(f"surface3d_stats {Z}x{H}x{W} C=5", lambda: ops.surface_stats_3d(pt, gtt, sp, 5, tolerances=tol, q=(95, 100)), judge)


# ------------------------------------------------------------------------------------------ LayerNorm
def _ln_report(family, r):
    assert r["nan"] == 0 and r["compared"] == r["expected"], r
    _record(family, r["ratio"])
    assert r["ratio"] <= 1.0, r


@pytest.mark.parametrize("dim", (384, 130, 260, 1028, 2052))
def test_layernorm_bwd(dim):
    import test_ln_bounds_gpu as TL
    from dinox import ops
    from oracle import ln_bounds as LB
    rows = 33
    x, gamma, beta = TL.inputs("randn", rows, dim)
    dy = LB.make_dy("randn", x, gamma, 1e-5)
    X, Gm, DY = TL.dev(x), TL.dev(gamma), TL.dev(dy)
    _, mean, rstd = ops.layernorm_fwd(X, Gm, TL.dev(beta), torch.float32, 1e-5)

    def judge(o):
        ref = LB.backward_ref(dy, x, gamma, TL.host(mean), TL.host(rstd), dx_add=None, chain=LB.standalone_chain(rows, dim))
        _ln_report("layernorm_bwd", LB.check_all({"dx": TL.host(o["out.0"]), "lowp": TL.host(o["out.3"]), "dgamma": TL.host(o["out.1"]),
                                                  "dbeta": TL.host(o["out.2"])}, ref))
    contract(f"layernorm_bwd {rows}x{dim}", lambda: ops.layernorm_bwd(DY, X, Gm, mean, rstd, want_lowp=True), judge)


def test_linear_residual_ln():
    import test_ln_bounds_gpu as TL
    from dinox import ops
    from oracle import ln_bounds as LB
    M, K, ydt = 209, 384, torch.bfloat16
    gamma, beta = LB.make_params(384, seed=K)
    a, w, b, r = TL.product_case(M, K, "randn", True, True)
    args = (TL.dev(a).bfloat16(), TL.dev(w).bfloat16(), TL.dev(b), TL.dev(r), TL.dev(gamma), TL.dev(beta), 1e-5, ydt)
    full = TL.full_row_kernel(M, False) and K >= 128

    def judge(o):
        pr = LB.product_ref(a, w, b, r)
        fr = LB.forward_ref(TL.host(o["out.0"]), gamma, beta, 1e-5, True, serial=12 if full else 48, combine=not full)
        ref = {"x": pr["x"], "x_bound": pr["x_bound"], **fr}
        _ln_report("linear_residual_ln", LB.check_all({"x": TL.host(o["out.0"]), "mean": TL.host(o["out.2"]), "rstd": TL.host(o["out.3"]),
                                                       "y": TL.host(o["out.1"])}, ref))
    contract(f"linear_residual_ln M={M} K={K}", lambda: ops.linear_residual_ln(*args), judge)


def test_linear_ln_bwd_with_dx_add_aliased():
    import dinox._lib as L
    import test_ln_bounds_gpu as TL
    from dinox import ops
    from oracle import ln_bounds as LB
    M, K = 209, 384
    assert L.lib.dinox_linear_ln_bwd_ok(M, 384, K) == 1
    chain = LB.row_chain(13, math.ceil(M / 208), waves=16)
    base = np.random.default_rng([31, M]).standard_normal((M, 384)).astype(np.float32)
    a, w, dy_ref, ulp, share = TL.lnbwd_operands(M, K, "randn")
    x, gamma, beta = TL.inputs("randn", M, 384)
    X, Gm = TL.dev(x), TL.dev(gamma)
    _, mean, rstd = ops.layernorm_fwd(X, Gm, TL.dev(beta), torch.float32, 1e-5)
    A, W = TL.dev(a).bfloat16(), TL.dev(w).bfloat16()

    def run():
        buf = TL.dev(base)
        return ops.linear_ln_bwd(A, W, X, Gm, mean, rstd, dx=buf, dx_add=buf, want_lowp=True)

    def judge(o):
        ref = LB.backward_ref(dy_ref, x, gamma, TL.host(mean), TL.host(rstd), dx_add=base, chain=chain, dy_ulp=ulp)
        _ln_report("linear_ln_bwd", LB.check_all({"dx": TL.host(o["out.0"]), "lowp": TL.host(o["out.3"]), "dgamma": TL.host(o["out.1"]),
                                                  "dbeta": TL.host(o["out.2"])}, ref))
    contract(f"linear_ln_bwd M={M} K={K} dx_add aliased", run, judge)


# ------------------------------------------------------------------------------------------ attention
ATTN = [((2, 33, 2, 64), torch.bfloat16), ((2, 201, 6, 64), torch.bfloat16), ((1, 261, 2, 64), torch.bfloat16), ((1, 545, 1, 64), torch.bfloat16),
        ((2, 37, 2, 20), torch.bfloat16), ((2, 37, 2, 20), torch.float32)]


@pytest.mark.parametrize("shape,dt", ATTN, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)[6:])
def test_attention_bwd(shape, dt):
    from dinox import ops
    from oracle import attention_bounds as AB
    B, N, h, d = shape
    fp32 = dt == torch.float32
    case = AB.FAMILIES[0]
    qkv = AB.make_qkv(case, B, N, h, d, seed=N + d, dtype=dt)
    do = AB.make_do(B, N, h, d, seed=N + d, dtype=dt)
    Q, DO = qkv.to(DEV), do.to(DEV)

    def run():
        o, lse = ops.attention_fwd(Q, h)
        return dict(o=o, lse=lse, dqkv=ops.attention_bwd(DO, Q, o, lse, h))

    def judge(out):
        o, lse, dqkv = out["out.o"].cpu(), out["out.lse"].cpu(), out["out.dqkv"].cpu()
        fb = AB.forward_bounds(qkv, h, fp32)
        bb = AB.backward_bounds(do, qkv, o, lse, h, fp32)
        dq, dk, dv = AB.split_dqkv(dqkv, h)
        for got, key in ((dq, "dq"), (dk, "dk"), (dv, "dv")):
            _record("attention_bwd", AB.ratio(got, bb[key], bb[key + "_bound"])[0])
        AB.check_forward(o, lse, fb, h, f"{shape} {case}")
        AB.check_backward(dqkv, bb, h, f"{shape} {case}")
    contract(f"attention_fwd/bwd {shape} {str(dt)[6:]}", run, judge)


# ------------------------------------------------------------------------------------------ split-K TN product through the workspace
@pytest.mark.parametrize("M,N,K,colsum", ((136, 72, 1000, False), (64, 72, 8232, True)))
def test_tn_gemm_with_workspace(M, N, K, colsum):
    """dW = dY^T X through ops.gemm: the wrapper asks dinox_gemm_ws_bytes and takes the workspace from ops._tn_workspace, whose cache the
    guard drops.  Bound: bf16 products are exact in fp32; K fp32 additions in any order: |err| <= gamma_K sum_k |a_k b_k|, gamma_K =
    K u / (1 - K u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); colsum the same with |a_k|."""
    from dinox import ops
    rng = np.random.default_rng([82, M, N, K])
    a = torch.from_numpy(rng.standard_normal((K, M)).astype(np.float32)).bfloat16()
    b = torch.from_numpy(rng.standard_normal((K, N)).astype(np.float32)).bfloat16()
    A, Bm = a.to(DEV), b.to(DEV)
    u = 2.0 ** -24
    gam = K * u / (1 - K * u)

    def run():
        cs = torch.empty(M, dtype=torch.float32, device=DEV) if colsum else None
        c = ops.gemm(A, Bm, transA=True, transB=True, out_dtype=torch.float32, colsum_out=cs)
        return dict(c=c, colsum=cs)

    def judge(o):
        a64, b64 = a.double().numpy(), b.double().numpy()
        _bound_judge("tn_gemm", "C", o["out.c"], a64.T @ b64, gam * (np.abs(a64).T @ np.abs(b64)))
        if colsum:
            _bound_judge("tn_gemm", "colsum", o["out.colsum"], a64.sum(0), gam * np.abs(a64).sum(0))
    ops.TRACE_KERNELS = []
    try:
        run()
        assert any(k.startswith("gemm_bf16_tn") for k in ops.TRACE_KERNELS), ops.TRACE_KERNELS
    finally:
        ops.TRACE_KERNELS = None
    contract(f"dinox_gemm TN {M}x{N}x{K} colsum={colsum}", run, judge)


# ------------------------------------------------------------------------------------------ LoRA
@pytest.mark.parametrize("M,K,N,r", ((5, 8, 8, 16), (130, 36, 1152, 1)))
def test_lora_grad(M, K, N, r):
    import _lora_oracle as LO
    import test_lora_gpu as TLo
    from dinox import ops
    rng = np.random.default_rng([3, M, K, N, r])
    xl, xl64 = TLo.operand(rng, (M, K), "bf16")
    dy, dy64 = TLo.operand(rng, (M, N), "bf16")
    A, A64 = TLo.f32(rng, (r, K), 0.1)
    Bm, B64 = TLo.f32(rng, (N, r), 0.1)

    def judge(o):
        rA, eA, rB, eB = LO.grad(xl64, dy64, A64, B64, 2.0)
        _bound_judge("lora_grad", "dA", o["out.0"], rA, eA)
        _bound_judge("lora_grad", "dB", o["out.1"], rB, eB)
    contract(f"lora_grad M={M} K={K} N={N} r={r}", lambda: ops.lora_grad(xl, dy, A, Bm, 2.0), judge)


# ------------------------------------------------------------------------------------------ search, probes
def _int_rows(rng, n, D):
    return rng.integers(-3, 4, (n, D)).astype(np.float32)               # integer rows: every score is exact in fp32


@pytest.mark.parametrize("Nq,Nk,D", ((5, 3, 16), (300, 65, 7)))
def test_search(Nq, Nk, D):
    """retrieval_rank, retrieval_rank_windowed over the whole key range, knn_topk (K = 10 where 10 <= Nk, else Nk).  Integer rows: the
    scores are exact, so the float64 judge is equality with the stable descending order."""
    from dinox import ops
    rng = np.random.default_rng([83, Nq, Nk, D])
    q, k = _int_rows(rng, Nq, D), _int_rows(rng, Nk, D)
    target = rng.integers(0, Nk, Nq).astype(np.int32)
    K = 10 if Nk >= 10 else Nk
    qt, kt, tt = _dev(q), _dev(k), _dev(target)
    lo, hi = torch.zeros(Nq, dtype=torch.int32, device=DEV), torch.full((Nq,), Nk, dtype=torch.int32, device=DEV)

    def run():
        return dict(rank=ops.retrieval_rank(qt, kt, tt), windowed=ops.retrieval_rank_windowed(qt, kt, lo, hi, tt), knn=ops.knn_topk(qt, kt, K))

    def judge(o):
        S = q.astype(np.float64) @ k.astype(np.float64).T
        pos = S[np.arange(Nq), target]
        rank = (S > pos[:, None]).sum(1) + ((S == pos[:, None]) & (np.arange(Nk)[None] < target[:, None])).sum(1)
        order = np.lexsort((np.broadcast_to(np.arange(Nk), S.shape), -S), axis=1)[:, :K]
        for fam in ("rank", "windowed"):                                  # (rank, best_idx, best_val, pos_val), in that order
            got = [o[f"out.{fam}.{i}"].cpu().numpy() for i in range(4)]
            assert [g.dtype for g in got] == [np.int32, np.int32, np.float32, np.float32], fam
            assert np.array_equal(got[0], rank), f"{fam}: rank"
            assert np.array_equal(got[1], order[:, 0]), f"{fam}: best_idx"
            assert np.array_equal(got[2].astype(np.float64), S.max(1)), f"{fam}: best_val"
            assert np.array_equal(got[3].astype(np.float64), pos), f"{fam}: pos_val"
        idx, val = o["out.knn.0"].cpu().numpy(), o["out.knn.1"].cpu().numpy()      # (idx, val)
        assert idx.dtype == np.int32 and np.array_equal(idx, order), "knn_topk: indices"
        assert val.dtype == np.float32 and np.array_equal(val.astype(np.float64), np.take_along_axis(S, order, 1)), "knn_topk: values"
        _record("search (exact)", 0.0)
    contract(f"retrieval_rank/windowed/knn_topk Nq={Nq} Nk={Nk} D={D} K={K}", run, judge)


def test_gram_and_softmax_probe():
    """(33, 7) and (67, 7, 3): the smallest odd shapes of tests/test_probes_gpu.py.  Integer rows make the Gram sums exact; the probe's
    outputs are held to that module's float64 reference and bounds."""
    import test_probes_gpu as TP
    from dinox import ops
    rng = np.random.default_rng([84])
    x = _int_rows(rng, 33, 7)
    xt = _dev(x)

    def judge_gram(o):                                                    # (gram [D][D], colsum [D]), double
        x64 = x.astype(np.float64)
        gm, cs = o["out.0"].cpu().numpy(), o["out.1"].cpu().numpy()
        assert gm.dtype == np.float64 and gm.shape == (7, 7) and np.array_equal(gm, x64.T @ x64), "gram"
        assert cs.dtype == np.float64 and cs.shape == (7,) and np.array_equal(cs, x64.sum(0)), "colsum"
        _record("gram (exact)", 0.0)
    contract("gram N=33 D=7", lambda: ops.gram(xt), judge_gram)
    px, label, theta = TP.probe_case(67, 7, 3, 8.0)
    X, Lb, Th = TP.dev(px), TP.dev(label), TP.dev(theta)

    def judge_probe(o):
        """(loss, grad, prob) of the very run that serves as the bit-equality reference, against the float64 reference and the bounds
        of tests/test_probes_gpu.py (check_probe): t bounds a logit's fp32 error; 4 t + 1e-6 a probability, N (2 t + 1e-6) the loss,
        (4 t + 1e-6) sum_i |x_id| a gradient column."""
        p64, loss64, grad64, t, colabs = TP.probe_reference(px, label, theta)
        N = px.shape[0]
        _bound_judge("softmax_probe", "prob", o["out.2"], p64, np.full_like(p64, 4 * t + 1e-6))
        _bound_judge("softmax_probe", "loss", o["out.0"], np.asarray(loss64, dtype=np.float64), np.asarray(N * (2 * t + 1e-6)))
        _bound_judge("softmax_probe", "grad", o["out.1"], grad64, (4 * t + 1e-6) * np.broadcast_to(colabs[None, :], grad64.shape))
    contract("softmax_probe N=67 D=7 C=3", lambda: ops.softmax_probe(X, Lb, Th, want_grad=True, want_prob=True), judge_probe)


def test_attention_rollout_step():
    """(2, 63, 2, 16): the smallest shape of tests/test_attention_rollout_gpu.py with more than one image, head and row chunk."""
    import _attention_rollout_oracle as RL
    from dinox import ops
    from oracle import attention_bounds as AB
    B, N, h, d = 2, 63, 2, 16
    qkv = AB.make_qkv(AB.FAMILIES[0], B, N, h, d, seed=5, dtype=torch.float32)
    w = torch.rand(B, N, generator=torch.Generator().manual_seed(6))
    Q, Wt = qkv.to(DEV), w.to(DEV)

    def judge(o):
        ref = RL.step_oracle(qkv, h, w, 0.5)
        _record("attention_rollout_step", RL.check(o["out"], ref["out"], ref["bound"], f"{(B, N, h, d)}"))
    contract(f"attention_rollout_step {(B, N, h, d)}", lambda: ops.attention_rollout_step(Q, h, Wt, 0.5), judge)


# ------------------------------------------------------------------------------------------ label propagation
def test_labelprop():
    """(g, F, D, C) = (5, 8, 7, 3): the smallest odd-C case of tests/test_labelprop_gpu.py (less than a tile, a non-vector D), K = 5,
    radius 1; integer operands, so selection and scores are exact and the vote is held to the oracle's derived bound."""
    import _labelprop_oracle as O
    import test_labelprop_gpu as TLP
    from dinox import ops
    shape, K, radius = (5, 8, 7, 3), 5, 1
    g = shape[0]
    q, k, seg = O.exact_case(*shape)
    qt, kt, st = _dev(q), _dev(k), _dev(seg)

    def judge(o):
        out, idx, val = (o[f"out.{i}"].cpu().numpy() for i in range(3))
        widx, wval = TLP.selected("exact", shape, radius)
        assert np.array_equal(idx, widx[:, :K]) and np.array_equal(val, wval[:, :K].astype(np.float32))
        want, bound = O.vote(idx, val, seg, TLP.INV_T), O.vote_bound(idx, val, TLP.INV_T)
        err = np.abs(out.astype(np.float64) - want).max(1)
        _record("labelprop", float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
    contract(f"labelprop {shape} K={K} radius={radius}", lambda: ops.label_propagate(qt, kt, st, g, K=K, radius=radius, temperature=TLP.T), judge)


# ------------------------------------------------------------------------------------------ scale embedding
def test_scale_embed_bwd():
    """V = 5, h = 12, D = 50 through ops.ScaleEmbedFn: the backward carves de [V][D] | dhpre [V][h] | hact [V][h] out of one workspace.
    Tolerances: those of test_scale_embed in tests/test_small_kernels_gpu.py (1e-4 of the largest output forward, 5e-4 backward)."""
    import _small_kernels_oracle as SO
    from dinox import ops
    V, h, D = 5, 12, 50
    i = SO.se_inputs(V, h, D, seed=V + h)
    names = ("sp", "w0", "b0", "w2", "b2", "lnw", "lnb")
    dout = _dev(i["dout"]).view(V, 1, D)

    def run():
        leaves = [_dev(i[n]).requires_grad_(True) for n in names]
        out = ops.ScaleEmbedFn.apply(*leaves, 1e-5)
        out.backward(dout)
        return dict(out=out.detach(), **{n: t.grad for n, t in zip(names, leaves)})

    def judge(o):
        full = SO.scale_embed_fwd(*(i[n] for n in names), eps=1e-5)
        fb = SO.scale_embed_bwd(i["dout"], i["sp"], i["w0"], i["w2"], i["lnw"], full["hpre"], full["e"], full["mean"], full["rstd"])
        refs = {"out": full["out"], "sp": fb["dspacing"], "w0": fb["dw0"], "b0": fb["db0"], "w2": fb["dw2"], "b2": fb["db2"], "lnw": fb["dlnw"],
                "lnb": fb["dlnb"]}
        for n, ref in refs.items():
            ref = np.asarray(ref, dtype=np.float64)
            _bound_judge("scale_embed", n, o[f"out.{n}"], ref, np.full(ref.shape, (1e-4 if n == "out" else 5e-4) * np.abs(ref).max() + 1e-5))
    contract(f"scale_embed_fwd/bwd V={V} h={h} D={D}", run, judge)


# ------------------------------------------------------------------------------------------ native block calls
def _block_reference(blk, x, dy, heads):
    """The block in float64 torch (pre-norm, exact-erf GELU) on the fp32 parameters: y, dx and the parameter gradients."""
    import torch.nn.functional as F
    sd = {n: p.detach().double().cpu().requires_grad_(True) for n, p in blk.named_parameters()}
    xi = x.double().cpu().requires_grad_(True)
    V, N, D = xi.shape
    xn = F.layer_norm(xi, (D,), sd["norm1.weight"], sd["norm1.bias"], blk.norm1.eps)
    qkv = (xn @ sd["attn.qkv.weight"].t() + sd["attn.qkv.bias"]).reshape(V, N, 3, heads, D // heads)
    q, k, v = (t.transpose(1, 2) for t in qkv.unbind(2))
    o = (torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D // heads), -1) @ v).transpose(1, 2).reshape(V, N, D)
    x1 = xi + o @ sd["attn.proj.weight"].t() + sd["attn.proj.bias"]
    xn2 = F.layer_norm(x1, (D,), sd["norm2.weight"], sd["norm2.bias"], blk.norm2.eps)
    y = x1 + F.gelu(xn2 @ sd["mlp.fc1.weight"].t() + sd["mlp.fc1.bias"]) @ sd["mlp.fc2.weight"].t() + sd["mlp.fc2.bias"]
    y.backward(dy.double().cpu())
    return y.detach(), xi.grad, {n: t.grad for n, t in sd.items()}


def test_block_forward_and_backward():
    """The shape of test_block_fused_node_matches_composed_ops (3 x 37 x 128, 2 heads, hidden 512) in bf16 mode, with every parameter
    registered in the gradient sink so that BOTH native calls run: dinox_block_forward and dinox_block_backward, the one place where the
    split-K, attention and LayerNorm workspaces are used together (tn_ws from ops._tn_workspace, attn_ws, ln_ws and the bf16 scratch).
    Judge: relative L2 distance to the float64 block under 2e-2, the bf16 tolerance of that test."""
    import zoo.arch as arch
    from dinox import ops
    torch.manual_seed(4)
    blk = arch.TransformerBlock(128, 2).to(DEV)
    with torch.no_grad():
        for p_ in blk.parameters():
            if p_.ndim == 1:
                p_.add_(0.05 * torch.randn_like(p_))
    assert blk._fusable()
    x, dy = torch.randn(3, 37, 128, device=DEV), torch.randn(3, 37, 128, device=DEV)
    params = list(blk.parameters())
    for p_ in params:
        p_.grad = torch.zeros_like(p_)
    seen = []
    real_fwd, real_bwd = ops._block_forward_native, ops._block_backward_native

    def spy_fwd(*a, **kw):
        seen.append("fwd")
        return real_fwd(*a, **kw)

    def spy_bwd(*a, **kw):
        out = real_bwd(*a, **kw)
        seen.append("bwd" if out is not None else "bwd-composed")
        return out

    def run():
        for p_ in params:
            p_.grad.zero_()
        xi = x.clone().requires_grad_(True)
        with ops.compute_dtype(torch.bfloat16):
            y = blk(xi)
            y.backward(dy)
        return dict(y=y.detach(), dx=xi.grad, **{n: p_.grad.clone() for n, p_ in blk.named_parameters()})

    def judge(o):
        y, dx, grads = _block_reference(blk, x, dy, 2)
        for n, ref in [("y", y), ("dx", dx)] + list(grads.items()):
            rel = float((o[f"out.{n}"].double().cpu() - ref).norm() / ref.norm().clamp_min(1e-30))
            _record("block (rel L2 / 2e-2)", rel / 2e-2)
            assert rel < 2e-2, (n, rel)
    ops.grad_sink.register(blk, params)
    ops._block_forward_native, ops._block_backward_native = spy_fwd, spy_bwd
    try:
        contract("block_forward/backward 3x37x128 heads=2 bf16", run, judge)
    finally:
        ops._block_forward_native, ops._block_backward_native = real_fwd, real_bwd
        ops.grad_sink.clear()
        ops.invalidate_weights()
    assert seen == ["fwd", "bwd"] * 3, seen                            # both native calls, in all three runs


# ------------------------------------------------------------------------------------------ sliding-window blend, patch sampler
@pytest.mark.parametrize("cid", ("3-5", "0-64"))
def test_seg_blend_predict(cid):
    """seg_blend_predict takes tiles, not (g, u, B, C): the nearest cases of tests/_segblend_cases.py are 3-5 (9 x 23, t = 7, g = 4,
    C = 5: small, odd, ragged) and 0-64 (37 x 53, t = 16, two overlaps, the widest class count)."""
    import _segblend_cases as K
    import _segblend_oracle as O
    import test_segblend_gpu as TSB
    from dinox import ops
    s, ys, xs, win, z, want = K.case(cid)
    lab = TSB._labels((s["B"], s["H"], s["W"]), s["C"], s["seed"] + 7)
    zt, lt = TSB._dev(z), TSB._dev(lab)

    def judge(o):
        pred, conf = o["out.0"].cpu().numpy(), o["out.2"].cpu().numpy()
        share, worst = want.check(pred, conf)
        _record("seg_blend_predict", worst)
        assert np.array_equal(o["out.1"].cpu().numpy(), O.confusion_counts(pred, lab, s["C"]))
    contract(f"seg_blend_predict case {cid}", lambda: ops.seg_blend_predict(zt, ys, xs, s["flips"], win, s["H"], s["W"], s["t"], labels=lt, want_conf=True),
             judge)


@pytest.mark.parametrize("i", (0, 1))
def test_seg_patch_sample(i):
    """seg_patch_sample takes a pool and jobs, not (g, u, B, C): launches 0 and 1 of tests/_segpatch_cases.py (S = 16 with B = 1 and
    B = 3, odd pool offsets) are the smallest of its own test."""
    import _segpatch_cases as K
    import _segpatch_oracle as O
    from dinox import ops
    c = K.launch(i)
    _, img, msk, _, _ = K.pool()
    pi, pm = _dev(img.copy()), _dev(msk.copy())

    def judge(o):
        x, m = o["out.0"].cpu().numpy(), o["out.1"].cpu().numpy()
        _, m32 = O.emulate32(K.pool()[0], c["plane_of"], c["par"], c["S"], K.MEAN, K.STD, c["pad"])
        ratio, share = c["want"].check(x, m, m32)
        _record("seg_patch_sample", ratio)
    contract(f"seg_patch_sample launch {i} S={c['S']} B={c['B']}", lambda: ops.seg_patch_sample(pi, pm, c["jobs"], c["par"], c["S"], K.MEAN, K.STD, c["pad"]),
             judge)


def test_zz_report_error_to_bound_ratios():
    """Not a check of its own: prints the largest error / bound ratio every family above saw (each was asserted <= 1 there)."""
    for k in sorted(RATIOS):
        print(f"workspace-contract error/bound  {k:28s} {RATIOS[k]:.4f}")
