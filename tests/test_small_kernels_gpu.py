"""The small kernels of a training step -- csrc/tokens.hip, scale_embed.hip, loss.hip, optim.hip, glue.hip -- called directly (the C
ABI or the thin ops wrappers, never through a GEMM) on every dispatch path of their launchers: scalar and vector kernels (by size
and by alignment), unrolled trips and their tails, second column blocks, grid caps, null optional arguments.

Copies, casts and single additions are compared bit for bit.  Everything else is held, element by element, to
    |got - ref| <= (n_ops + 2) 2^-24 S + tiny
against the float64 statements of tests/_small_kernels_oracle.py (S: the sum of the absolute terms of the element, n_ops: the rounded
operations on the longest path to it; the counts are written at the bound builders there), plus the project's existing tolerance
where expf / logf / erff enter.  tests/test_small_kernels_cpu.py proves those statements and shows that a NumPy float32 evaluation
of the same inputs stays inside the same bounds.  Every output buffer starts as NaN, so an element nobody wrote fails.

Each check prints ``ratio <kernel> <largest error / bound>`` (visible with ``pytest -s``)."""
import numpy as np
import pytest
import torch

import _small_kernels_oracle as SO

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
U = SO.U


@pytest.fixture(scope="module")
def dx():
    from dinox import ops
    import dinox._lib as L
    assert L.lib.dinox_device_ok() == 1, L.last_error()
    return ops, L


def nan(*shape, dtype=F32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def dev(a, dtype=F32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(device=DEV, dtype=dtype)


def off1(t):
    """The same values in storage that starts one element past an aligned address: the launchers' alignment tests then fail."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def P(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def code(dt):
    return 0 if dt == F32 else 1


def host(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def exact(got, want, what):
    want = torch.as_tensor(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert torch.equal(got.cpu(), want), f"{what}: {int((got.cpu() != want).sum())} of {want.numel()} elements differ"


def within(name, got, ref, bound, what=""):
    got = host(got) if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref, bound = np.broadcast_to(np.asarray(ref, np.float64), got.shape), np.broadcast_to(np.asarray(bound, np.float64), got.shape)
    assert np.isfinite(got).all(), f"{name} {what}: {int((~np.isfinite(got)).sum())} elements not finite (unwritten or overflowed)"
    ratio = float((np.abs(got - ref) / bound).max()) if got.size else 0.0
    print(f"ratio {name} {ratio:.4f}")
    assert ratio <= 1.0, f"{name} {what}: error at {ratio:.3f} of the bound (worst element {int(np.argmax(np.abs(got - ref) / bound))})"


def rng(*key):
    return np.random.default_rng(sum((i + 1) * int(k) for i, k in enumerate(key)))


def randn(r, *shape):
    return r.standard_normal(shape).astype(np.float32)


# ========================================================================================== bit-exact: copies, casts, single additions
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V,H,W,p,offset", [(3, 32, 48, 4, False), (3, 32, 48, 8, False), (3, 32, 48, 16, False), (2, 28, 42, 14, False),
                                            (3, 32, 48, 16, True)])
def test_patch_unfold(dx, V, H, W, p, offset, dt):
    """patch 4 and 14: scalar kernel; 8 and 16: eight elements per thread; 16 from a view one float off alignment: scalar again.
    The image is not square, so g (= W / p) and gh (= H / p) cannot stand in for each other."""
    _, L = dx
    x = randn(rng(V, H, W, p), V, 3, H, W)
    xd = off1(dev(x)) if offset else dev(x)
    u = nan(V * (H // p) * (W // p), 3 * p * p, dtype=dt)
    L.check(L.lib.dinox_patch_unfold(P(xd), P(u), V, H, W, p, code(dt), stream()), "dinox_patch_unfold")
    exact(u, torch.from_numpy(SO.unfold(x, p)).to(dt), "unfold")


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_patch_unfold_ld(dx, dt):
    _, L = dx
    V, H, W, p, ld = 2, 28, 42, 14, 640
    x = randn(rng(5), V, 3, H, W)
    xd, u = dev(x), nan(V * 2 * 3, ld, dtype=dt)
    L.check(L.lib.dinox_patch_unfold_ld(P(xd), P(u), V, H, W, p, ld, code(dt), stream()), "dinox_patch_unfold_ld")
    want = torch.from_numpy(SO.unfold_ld(x, p, ld)).to(dt)
    assert (want[:, 588:] == 0).all() and want[:, :588].abs().min() > 0
    exact(u, want, "unfold_ld")


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("D,offset", [(4, False), (256, False), (260, False), (384, False), (6, False), (50, False), (64, True)])
def test_tokens_fwd_and_patch_gradient(dx, D, offset, dt):
    """D % 4 == 0 and aligned: four features per thread (D = 260, 384: a second column block in the backward); D = 6, 50 and the
    offset view: scalar kernels.  Forward against fp32 (patches + pos) + scale, one rounded addition each, in the kernel's order;
    dpatches is a copy or a cast of rows 1..P."""
    _, L = dx
    V = 3
    for P_ in (1, 4, 9):
        for R in (0, 4):
            for has_scale in (False, True):
                r = rng(D, P_, R, has_scale)
                N = 1 + P_ + R
                patches = dev(randn(r, V, P_, D)).to(dt)
                cls, pos = dev(randn(r, D)), dev(randn(r, 1 + P_, D))
                regs = dev(randn(r, R, D)) if R else None
                scale = dev(randn(r, V, D)) if has_scale else None
                tok = nan(V, N, D)
                tokv = off1(tok) if offset else tok
                L.check(L.lib.dinox_tokens_fwd(P(patches), P(cls), P(pos), P(regs), P(scale), P(tokv), V, P_, R, D, code(dt), stream()),
                        "dinox_tokens_fwd")
                body = torch.cat([cls.cpu().expand(V, 1, D), patches.cpu().float()], 1) + pos.cpu()
                if has_scale:
                    body = body + scale.cpu()[:, None]
                want = torch.cat([body, regs.cpu().expand(V, R, D)], 1) if R else body
                exact(tokv, want, f"tokens P={P_} R={R} scale={has_scale}")
                dtok = dev(randn(r, V, N, D))
                dtokv = off1(dtok) if offset else dtok
                dpatches, dcls, dpos = nan(V, P_, D, dtype=dt), nan(D), nan(1 + P_, D)
                dregs = nan(R, D) if R else None
                L.check(L.lib.dinox_tokens_bwd(P(dtokv), P(dpatches), P(dcls), P(dpos), P(dregs), None, V, P_, R, D, code(dt), stream()),
                        "dinox_tokens_bwd")
                exact(dpatches, dtok[:, 1:1 + P_].cpu().to(dt), f"dpatches P={P_} R={R}")


@pytest.mark.parametrize("D", [4, 256, 260, 6])
@pytest.mark.parametrize("V", [1, 3, 4, 5, 13, 16, 17, 33])
def test_tokens_bwd_batch_sums(dx, V, D):
    """The V loop of the vector kernel runs 16 deep over four slices (V = 13: slice 0 takes one unrolled trip, 16, 17, 33: more
    slices do, each with another tail); D = 260: the second column block holds one float4; D = 6: the scalar kernel."""
    _, L = dx
    P_ = 4
    for R in (0, 4):
        for want_scale in (False, True):
            dtok = randn(rng(V, D, R), V, 1 + P_ + R, D)
            o = SO.tokens_bwd(dtok, P_, R)
            b = SO.bound_tokens_bwd(o, V, P_)
            dpatches, dcls, dpos = nan(V, P_, D), nan(D), nan(1 + P_, D)
            dregs = nan(R, D) if R else None
            dscale = nan(V, D) if want_scale else None
            dtokd = dev(dtok)
            L.check(L.lib.dinox_tokens_bwd(P(dtokd), P(dpatches), P(dcls), P(dpos), P(dregs), P(dscale), V, P_, R, D, 0, stream()),
                    "dinox_tokens_bwd")
            exact(dpatches, torch.from_numpy(dtok[:, 1:1 + P_]), "dpatches")
            within("tokens_bwd.dcls", dcls, o["dcls"][0], b["dcls"])
            within("tokens_bwd.dpos", dpos, o["dpos"][0], b["dpos"])
            if R:
                within("tokens_bwd.dregs", dregs, o["dregs"][0], b["dregs"])
            if want_scale:
                within("tokens_bwd.dscale", dscale, o["dscale"][0], b["dscale"])


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_take_rows(dx, dt):
    """Row 2 of every [5, D] image (source stride N D) into rows dst_row0.. of a larger buffer, whose other rows stay untouched."""
    ops, _ = dx
    for D in (4, 64, 384):
        for V in (1, 7):
            for row0 in (0, 3):
                src = dev(randn(rng(D, V, row0), V, 5, D))
                out = nan(V + 5, D, dtype=dt)
                ops.take_rows(src, 2, dt, out=out, out_row0=row0)
                exact(out[row0:row0 + V], src[:, 2].cpu().to(dt), f"take_rows D={D} V={V} row0={row0}")
                rest = torch.cat([out[:row0], out[row0 + V:]])
                assert torch.isnan(rest).all(), "take_rows wrote outside its rows"


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_put_rows(dx, dt):
    """dst[v, row] = src[src_row0 + v] (any D: a scalar kernel), then the accumulating form: one rounded addition per element,
    bound (1 + 2) u (|src| + |dst|)."""
    ops, _ = dx
    for D in (6, 64):
        V, N, row, row0 = 5, 4, 1, 2
        src = dev(randn(rng(D, 1), V + row0 + 1, D)).to(dt)
        dst = nan(V, N, D)
        ops.put_rows_(dst, row, src, src_row0=row0)
        exact(dst[:, row], src[row0:row0 + V].float().cpu(), f"put_rows D={D}")
        assert torch.isnan(dst[:, :row]).all() and torch.isnan(dst[:, row + 1:]).all(), "put_rows wrote outside its row"
        base = randn(rng(D, 2), V, N, D)
        dst = dev(base)
        ops.put_rows_(dst, row, src, src_row0=row0, accumulate=True)
        x, d = host(src[row0:row0 + V]), base[:, row].astype(np.float64)
        within("put_rows.accumulate", dst[:, row], x + d, (1 + 2) * U * (np.abs(x) + np.abs(d)) + SO.TINY)
        keep = torch.ones(N, dtype=torch.bool)
        keep[row] = False
        exact(dst[:, keep], torch.from_numpy(base)[:, keep], "put_rows: the other rows")


@pytest.mark.parametrize("n", [1, 255, 1025])
def test_cast_bf16(dx, n):
    _, L = dx
    x = dev(randn(rng(n), n))
    out = nan(n + 3, dtype=BF16)
    L.check(L.lib.dinox_cast_bf16(P(x), P(out), n, stream()), "dinox_cast_bf16")
    exact(out[:n], x.cpu().bfloat16(), "cast_bf16")
    assert torch.isnan(out[n:]).all()


@pytest.mark.parametrize("R,C", [(1, 1), (31, 33), (32, 32), (33, 65), (384, 100)])
def test_cast_transpose_bf16(dx, R, C):
    _, L = dx
    x = dev(randn(rng(R, C), R, C))
    out = nan(C, R, dtype=BF16)
    L.check(L.lib.dinox_cast_transpose_bf16(P(x), P(out), R, C, stream()), "dinox_cast_transpose_bf16")
    exact(out, x.cpu().t().contiguous().bfloat16(), "cast_transpose")


def test_cast_transpose_bf16_multi(dx):
    """table[i] = {element offset in both arenas, R, C, first tile} (int64 x 4, as documented at cast_transpose_multi_kernel); a
    32 x 32 tile per workgroup, so a matrix takes ceil(C / 32) ceil(R / 32) of them.  The gaps between the matrices stay untouched."""
    _, L = dx
    mats, table, off, tile = [(5, 7), (33, 65), (32, 32)], [], 0, 0
    for R, C in mats:
        table.append([off, R, C, tile])
        off = (off + R * C + 7) // 8 * 8 + 8
        tile += -(-C // 32) * -(-R // 32)
    assert tile == 1 + 6 + 1
    src = dev(randn(rng(9), off))
    out = nan(off, dtype=BF16)
    tab = torch.tensor(table, dtype=torch.int64, device=DEV)
    L.check(L.lib.dinox_cast_transpose_bf16_multi(P(src), P(out), P(tab), len(mats), tile, stream()), "dinox_cast_transpose_bf16_multi")
    written = torch.zeros(off, dtype=torch.bool)
    for o, R, C, _ in table:
        exact(out[o:o + R * C].view(C, R), src[o:o + R * C].view(R, C).cpu().t().contiguous().bfloat16(), f"multi transpose {R}x{C}")
        written[o:o + R * C] = True
    assert torch.isnan(out.cpu()[~written]).all()


# ========================================================================================== fp64-bounded
@pytest.mark.parametrize("h,D", [(16, 64), (100, 384), (300, 600)])
@pytest.mark.parametrize("V", [1, 7, 8, 9, 17])
def test_scale_embed(dx, V, h, D):
    """V = 8, 9, 17: the 8-row unrolled trip of the parameter sums, with and without a tail; h = 300, D = 384 / 600: the strided
    loops of the row kernels (more than 256 hidden units / features).  Stage by stage on the kernel's own intermediates (the
    forward returns hpre, e, mean, rstd; the backward's de, dhpre and gelu(hpre) are read from its workspace), then end to end
    at the tolerances of test_scale_embedding_golden."""
    _, L = dx
    lib = L.lib
    i = SO.se_inputs(V, h, D, seed=V + h)
    d = {k: dev(v) for k, v in i.items()}
    names = ("sp", "w0", "b0", "w2", "b2", "lnw", "lnb")
    f = {"out": nan(V, D), "hpre": nan(V, h), "e": nan(V, D), "mean": nan(V), "rstd": nan(V)}
    L.check(lib.dinox_scale_embed_fwd(*(P(d[k]) for k in names), P(f["out"]), P(f["hpre"]), P(f["e"]), P(f["mean"]), P(f["rstd"]),
                                      V, h, D, 1e-5, stream()), "dinox_scale_embed_fwd")
    got = {k: v.cpu().numpy() for k, v in f.items()}
    for k, (ref, bound) in SO.bound_se_fwd(*(i[k] for k in names), 1e-5, got).items():
        within(f"scale_embed_fwd.{k}", got[k], ref, bound)
    full = SO.scale_embed_fwd(*(i[k] for k in names), eps=1e-5)
    assert np.abs(full["out"]).max() > 0.5
    assert np.abs(got["out"] - full["out"]).max() <= 1e-4 * np.abs(full["out"]).max() + 1e-5

    assert lib.dinox_scale_embed_bwd_ws_bytes(V, h, D) == 4 * V * (D + 2 * h)
    for want_dsp in (True, False):
        ws = nan(V * (D + 2 * h))
        g = {"dw0": nan(h, 3), "db0": nan(h), "dw2": nan(D, h), "db2": nan(D), "dlnw": nan(D), "dlnb": nan(D)}
        dsp = nan(V, 3) if want_dsp else None
        L.check(lib.dinox_scale_embed_bwd(P(d["dout"]), P(d["sp"]), P(d["w0"]), P(d["w2"]), P(d["lnw"]), P(f["hpre"]), P(f["e"]), P(f["mean"]),
                                          P(f["rstd"]), P(g["dw0"]), P(g["db0"]), P(g["dw2"]), P(g["db2"]), P(g["dlnw"]), P(g["dlnb"]), P(dsp),
                                          P(ws), V, h, D, stream()), "dinox_scale_embed_bwd")
        gb = {k: v.cpu().numpy() for k, v in g.items()}
        w = ws.cpu().numpy()
        gb.update(de=w[:V * D].reshape(V, D), dhpre=w[V * D:V * (D + h)].reshape(V, h), hact=w[V * (D + h):].reshape(V, h))
        if want_dsp:
            gb["dspacing"] = dsp.cpu().numpy()
        for k, (ref, bound) in SO.bound_se_bwd(i["dout"], i["sp"], i["w0"], i["w2"], i["lnw"], got, gb).items():
            if k in gb:
                within(f"scale_embed_bwd.{k}", gb[k], ref, bound)
        fb = SO.scale_embed_bwd(i["dout"], i["sp"], i["w0"], i["w2"], i["lnw"], full["hpre"], full["e"], full["mean"], full["rstd"])
        for k, ref in fb.items():
            if k in gb:
                assert np.abs(gb[k] - ref).max() <= 5e-4 * np.abs(ref).max() + 1e-5, k


def _check_dino(name, o, row, ds, loss):
    b = SO.bound_dino(o)
    within(name + ".row_loss", row, o["row"], b["row"] + SO.CE_LOSS_RTOL * np.abs(o["row"]))
    within(name + ".ds", ds, o["ds"], b["ds"] + SO.CE_DS_RTOL * np.abs(o["ds"]).max(1, keepdims=True))
    within(name + ".loss", loss, [o["loss"]], b["loss"] + SO.CE_LOSS_RTOL * abs(o["loss"]))


@pytest.mark.parametrize("regime", ["normal", "underflow", "onehot"])
@pytest.mark.parametrize("K", [1, 7, 255, 256, 257, 1000, 65536])
@pytest.mark.parametrize("rows", [2, 6])
def test_dino_ce(dx, rows, K, regime):
    """K < 256: idle threads in every block reduction; K % 256 != 0: a ragged last trip; 65536: 256 trips.  See SO.dino_inputs for
    the three logit regimes; everything must stay finite.  grad_scale = 0.7."""
    _, L = dx
    s, t, c = SO.dino_inputs(regime, rows, rows, K, seed=K + rows)
    o = SO.dino_ce(s, t, c, 0.1, 0.04, grad_scale=0.7)
    loss, ds, row = nan(1), nan(rows, K), nan(rows)
    sd, td, cd = dev(s), dev(t), dev(c)                                 # (named: a temporary's memory is reused by the next one)
    L.check(L.lib.dinox_dino_ce(P(sd), P(td), P(cd), 0.1, 0.04, 0.7, P(loss), P(ds), P(row), rows, K, stream()), "dinox_dino_ce")
    _check_dino("dino_ce", o, row, ds, loss)
    loss2, row2 = nan(1), nan(rows)                                     # without the gradient: the same losses, bit for bit
    L.check(L.lib.dinox_dino_ce(P(sd), P(td), P(cd), 0.1, 0.04, 0.7, P(loss2), None, P(row2), rows, K, stream()), "dinox_dino_ce")
    exact(row2, row.cpu(), "row losses without ds")
    exact(loss2, loss.cpu(), "loss without ds")


@pytest.mark.parametrize("K", [7, 257, 1000])
@pytest.mark.parametrize("G,views,B", [(2, 2, 1), (2, 5, 3), (3, 3, 2), (1, 2, 5)])
def test_dino_ce_multi(dx, G, views, B, K):
    _, L = dx
    s, t, c = SO.dino_inputs("normal", views * B, G * B, K, seed=K + G)
    o = SO.dino_ce_multi(s, t, c, 0.1, 0.04, G, grad_scale=1.3)
    loss, ds, ws = nan(1), nan(views * B, K), nan((views + 2 * G) * B)
    sd, td, cd = dev(s), dev(t), dev(c)
    L.check(L.lib.dinox_dino_ce_multi(P(sd), P(td), P(cd), 0.1, 0.04, 1.3, P(loss), P(ds), P(ws), B, G, views, K, stream()),
            "dinox_dino_ce_multi")
    _check_dino("dino_ce_multi", o, ws[:views * B], ds, loss)


@pytest.mark.parametrize("K,offset", [(4, False), (252, False), (256, False), (260, False), (7, False), (256, True)])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 13, 16, 17, 33])
def test_colmean(dx, rows, K, offset):
    """K % 4 == 0 and aligned: four slices of the rows, 16 deep (rows = 13: one unrolled trip in slice 0; 16, 17, 33: more); K = 260:
    a second workgroup with one float4; K = 7 and the offset view: the scalar kernel.  rows adds on a path at most, then the
    division: (rows + 1 + 2) u S."""
    _, L = dx
    t = randn(rng(rows, K), rows, K)
    td = off1(dev(t)) if offset else dev(t)
    out = nan(K)
    L.check(L.lib.dinox_colmean(P(td), P(out), rows, K, stream()), "dinox_colmean")
    ref, a = SO.colmean(t)
    within("colmean", out, ref, (rows + 1 + 2) * U * a + SO.TINY)


def test_center_ema(dx):
    ops, _ = dx
    r = rng(257)
    c, m = 50 * randn(r, 257), randn(r, 257)
    cd = dev(c)
    ops.center_ema_(cd, dev(m), 0.9)
    ref, a = SO.center_ema(c, m, 0.9)
    within("center_ema", cd, ref, (4 + 2) * U * a + SO.TINY)              # 1 - mom, two products, the sum


def _bf16_ulp(r):
    r = np.abs(np.asarray(r, np.float64))
    return np.where(r > 0, 2.0 ** (np.floor(np.log2(np.maximum(r, 1e-300))) - 7), SO.TINY)


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V,N,D", [(1, 2, 32), (3, 6, 65), (2, 5, 384)])
def test_gram_normalize(dx, V, N, D, dt):
    """(1, 2, 32): one token; (3, 6, 65): 15 rows, not a multiple of the four a workgroup takes, D not a multiple of the wave;
    one row exactly zero and one of norm 1e-13, both at the clamp: snorm = 1e-12, the backward is g * 1e12 on non-zero data.
    bf16 outputs: the float64 value rounded once, one bf16 ulp."""
    _, L = dx
    T = N - 1
    sf, tf = SO.gram_inputs(V, N, D, seed=D)
    o = SO.gram_normalize(sf, tf)
    b = SO.bound_gram_normalize(o, D)
    cat, catneg, shat, snorm = nan(V, T, 2 * D, dtype=dt), nan(V, T, 2 * D, dtype=dt), nan(V, T, D, dtype=dt), nan(V, T)
    sfd, tfd = dev(sf), dev(tf)
    L.check(L.lib.dinox_gram_normalize(P(sfd), P(tfd), P(cat), P(catneg), P(shat), P(snorm), V, N, D, code(dt), stream()),
            "dinox_gram_normalize")
    within("gram_normalize.snorm", snorm, o["snorm"], b["snorm"])
    special = V * T > 1                                                  # (a single row stays an ordinary one)
    if special:
        assert float(snorm[0, 0]) == float(np.float32(1e-12)) == float(snorm[V - 1, T - 1]) and (shat[0, 0] == 0).all()
    for k, got in (("cat", cat), ("catneg", catneg), ("shat", shat)):
        if dt == F32:
            within("gram_normalize." + k, got, o[k], b[k])
        else:
            r1 = host(torch.from_numpy(o[k]).to(BF16))
            within("gram_normalize_bf16." + k, got, r1, _bf16_ulp(r1))

    r = rng(V, N, D, 3)
    dxh = randn(r, V, T, D)
    sh_in, sn_in = torch.from_numpy(o["shat"]).to(dt), o["snorm"].astype(np.float32)
    base = randn(r, V, N, D)
    dxhd, shd, snd = dev(dxh), sh_in.to(DEV), dev(sn_in)
    for accumulate in (False, True):
        dfeats = dev(base) if accumulate else nan(V, N, D)
        L.check(L.lib.dinox_gram_normalize_bwd(P(dxhd), P(shd), P(snd), None, P(dfeats), V, N, D, code(dt),
                                               int(accumulate), stream()), "dinox_gram_normalize_bwd")
        ref, bound = SO.bound_gram_normalize_bwd(dxh, host(sh_in), sn_in, dst=base[:, 1:] if accumulate else None)
        within(f"gram_normalize_bwd{'.accumulate' if accumulate else ''}", dfeats[:, 1:], ref, bound)
        assert not special or np.abs(ref[0, 0]).max() > 1e11             # the clamped row carries g * 1e12
        if accumulate:
            exact(dfeats[:, 0], torch.from_numpy(base)[:, 0], "CLS rows")
        else:
            assert torch.isnan(dfeats[:, 0]).all(), "the CLS rows are not this kernel's to write"


HP = dict(lr=2e-3, weight_decay=0.04, beta1=0.9, beta2=0.999, eps=1e-8, step_t=3, ema=0.996, grad_scale=0.37)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 10007, 2048 * 256 * 4 + 1203])
def test_adamw_ema(dx, n):
    """Arenas of exactly n elements (n % 4 = 1, 2, 3: the tail of the first workgroup; the last n: past the cap of 2048 workgroups,
    so every thread strides, with a tail of 3), each followed by NaN guards that must survive.  With and without a teacher; the
    device-side hyper-parameters of ops.adamw_hyper must reproduce the host-scalar launch bit for bit; the squared gradient
    norm and ops.sumsq against float64."""
    ops, _ = dx
    r = rng(n)
    p, g, tch = randn(r, n), randn(r, n), randn(r, n)
    m, v = 0.1 * randn(r, n), 0.01 * np.abs(randn(r, n))
    hp = (HP["step_t"], HP["lr"], HP["weight_decay"], HP["beta1"], HP["beta2"], HP["eps"], HP["ema"])

    def arena(a):
        buf = nan(n + 8)
        buf[:n] = torch.from_numpy(a)
        return buf

    def run(teacher, hyper=None):
        bufs = [arena(a) for a in (p, g, m, v)] + ([arena(tch)] if teacher else [])
        P_, G_, M_, V_ = (b[:n] for b in bufs[:4])
        T_ = bufs[4][:n] if teacher else None
        out = ops.adamw_ema_(P_, G_, M_, V_, T_, hyper=hyper, **HP)
        for b in bufs:
            assert torch.isnan(b[n:]).all(), "adamw_ema wrote past the end of an arena"
        exact(G_, torch.from_numpy(g), "the gradient arena is read-only")
        return P_, M_, V_, T_, out

    blocks = min(2048, -(-n // 1024))
    for teacher in (True, False):
        ref = SO.adamw_ema(p, g, m, v, tch if teacher else None, *hp, grad_scale=HP["grad_scale"])
        b = SO.bound_adamw(p, g, m, v, tch if teacher else None, *hp, HP["grad_scale"], ref)
        got = run(teacher)
        tag = "adamw_ema" if teacher else "adamw_ema_no_teacher"
        within(tag + ".p", got[0], ref[0], b["p"]); within(tag + ".m", got[1], ref[1], b["m"]); within(tag + ".v", got[2], ref[2], b["v"])
        if teacher:
            within(tag + ".teacher", got[3], ref[3], b["teacher"])
        within(tag + ".gnorm_sq", got[4], [ref[4]], SO.bound_sumsq(n, blocks, 3 + 5, ref[4]) + SO.TINY)   # gr (twice), the square; a thread's last 4-wide trip and the tail
        hyper = torch.tensor(ops.adamw_hyper(HP["lr"], HP["beta1"], HP["beta2"], HP["step_t"]), dtype=F32, device=DEV)
        again = run(teacher, hyper=hyper)
        for a, c, what in zip(got, again, ("p", "m", "v", "teacher", "gnorm_sq")):
            if a is not None:
                exact(c, a.cpu(), f"hyper launch {what}")
    total = float((g.astype(np.float64) ** 2).sum())
    within("sumsq", ops.sumsq(dev(g)), [total], SO.bound_sumsq(n, min(2048, -(-n // 2048)), 1, total) + SO.TINY)


@pytest.mark.parametrize("n", [1, 257, 4096 * 256 + 5])
def test_axpy(dx, n):
    """The last n is past the cap of 4096 workgroups: the first threads stride.  2u (|y| + |alpha x|): the product and the sum, or one FMA."""
    ops, _ = dx
    r = rng(n)
    y, x = randn(r, n), randn(r, n)
    buf = nan(n + 8)
    buf[:n] = torch.from_numpy(y)
    ops.axpy_(buf[:n], dev(x), -0.3)
    ref, a = SO.axpy(y, x, -0.3)
    within("axpy", buf[:n], ref, 2 * U * a + SO.TINY)
    assert torch.isnan(buf[n:]).all()


def test_lincomb3(dx):
    ops, _ = dx
    a, b, c = dev([1.7]), dev([-2.9]), dev([0.013])
    for bb, cc in ((b, c), (None, c), (b, None), (None, None)):
        ref, s = SO.lincomb3(float(a), None if bb is None else float(bb), None if cc is None else float(cc), 0.3, 7.1)
        within("lincomb3", ops.lincomb3(a, bb, cc, 0.3, 7.1), [ref], (4 + 2) * U * s + SO.TINY)   # two products, two sums


def test_gelu_fn(dx):
    """A grid over [-10, 10], +-0, +-30 and a subnormal: (|x| + 1) 2^-22 for the cancellation in 1 + erf, plus the project's 1e-5."""
    ops, _ = dx
    x = np.concatenate([np.linspace(-10, 10, 2001), [0.0, -0.0, 30.0, -30.0, 1e-40]]).astype(np.float32)
    dy = randn(rng(4), x.size)
    xd = dev(x).requires_grad_(True)
    y = ops.GeluFn.apply(xd)
    y.backward(dev(dy))
    x64 = x.astype(np.float64)
    within("gelu_fwd", y, SO.gelu(x64), SO.gelu_tol(x64, SO.gelu(x64)))
    gg = SO.gelu_grad(x64)
    within("gelu_bwd", xd.grad, dy * gg, np.abs(dy) * SO.gelu_tol(x64, gg) + 2 * U * np.abs(dy * gg) + SO.TINY)
