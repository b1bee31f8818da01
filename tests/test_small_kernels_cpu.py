"""The small kernels of a training step (tokens, scale embedding, losses, optimiser, glue), host side: the float64 statements of
tests/_small_kernels_oracle.py against float64 autograd on the plain PyTorch statement of each forward and against the fixtures
recorded from the reference; the same formulas evaluated in NumPy float32 against the bounds the GPU tests hold the kernels to (if an
honest fp32 evaluation left a bound, the input would be wrong, not the bound); and the argument checks of the C entry points, which
return before any launch.  No kernel is launched."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

import _small_kernels_oracle as SO

F32 = np.float32


def T(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def same(got, want, tol=1e-10):
    got, want = np.asarray(got, np.float64), np.asarray(want.detach() if torch.is_tensor(want) else want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max()), np.abs(got - want).max()


def inside(got, ref, bound, what):
    ratio = np.abs(np.asarray(got, np.float64) - ref) / bound
    assert np.isfinite(np.asarray(got, np.float64)).all() and ratio.max() <= 1.0, f"{what}: fp32 evaluation at {ratio.max():.3f} of the bound"
    return float(ratio.max())


# ------------------------------------------------------------------------------------------ float64 autograd
def test_unfold_is_the_strided_convolution_input():
    """F.unfold with kernel = stride = patch lists the same columns (c, py, px) for patch (gy, gx), also on a non-square image."""
    x = np.random.default_rng(0).standard_normal((3, 3, 8, 12))
    want = F.unfold(T(x), kernel_size=4, stride=4).transpose(1, 2).reshape(3 * 2 * 3, 48)
    same(SO.unfold(x, 4), want, 0.0)
    u = SO.unfold_ld(x, 4, 64)
    assert u.shape == (18, 64) and (u[:, :48] == SO.unfold(x, 4)).all() and (u[:, 48:] == 0).all()
    assert SO.unfold(x, 4)[1 * 6 + 1 * 3 + 2, 2 * 16 + 3 * 4 + 1] == x[1, 2, 4 + 3, 8 + 1]


@pytest.mark.parametrize("R,has_scale", [(0, False), (4, True)])
def test_tokens_backward_is_autograd_of_cat_and_add(R, has_scale):
    r = np.random.default_rng(1)
    V, P, D = 5, 4, 6
    patches, cls, pos = T(r.standard_normal((V, P, D)), True), T(r.standard_normal(D), True), T(r.standard_normal((1 + P, D)), True)
    regs = T(r.standard_normal((R, D)), True) if R else None
    scale = T(r.standard_normal((V, D)), True) if has_scale else None
    tok = torch.cat([cls.expand(V, 1, D), patches], 1) + pos
    if has_scale:
        tok = tok + scale[:, None]
    if R:
        tok = torch.cat([tok, regs.expand(V, R, D)], 1)
    same(SO.tokens_fwd(patches.detach(), cls.detach(), pos.detach(), None if regs is None else regs.detach(),
                       None if scale is None else scale.detach()), tok)
    dtok = r.standard_normal(tuple(tok.shape))
    tok.backward(T(dtok))
    o = SO.tokens_bwd(dtok, P, R)
    same(o["dpatches"][0], patches.grad); same(o["dcls"][0], cls.grad); same(o["dpos"][0], pos.grad)
    if R:
        same(o["dregs"][0], regs.grad)
    if has_scale:
        same(o["dscale"][0], scale.grad)
    assert (o["dpos"][1] >= np.abs(o["dpos"][0])).all() and o["dscale"][1].shape == (V, D)


def test_scale_embed_backward_is_autograd_of_linear_gelu_linear_layernorm():
    i = SO.se_inputs(7, 16, 24, seed=2)
    names = ("sp", "w0", "b0", "w2", "b2", "lnw", "lnb")
    sp, w0, b0, w2, b2, lnw, lnb = (T(i[k], True) for k in names)
    e = F.linear(F.gelu(F.linear(sp, w0, b0)), w2, b2)
    y = F.layer_norm(e, (24,), lnw, lnb, 1e-5)
    f = SO.scale_embed_fwd(*(i[k] for k in names), eps=1e-5)
    same(f["out"], y); same(f["e"], e)
    y.backward(T(i["dout"]))
    b = SO.scale_embed_bwd(i["dout"], i["sp"], i["w0"], i["w2"], i["lnw"], f["hpre"], f["e"], f["mean"], f["rstd"])
    for k, want in (("dw0", w0), ("db0", b0), ("dw2", w2), ("db2", b2), ("dlnw", lnw), ("dlnb", lnb), ("dspacing", sp)):
        same(b[k], want.grad)


def _dino_torch(s, t, c, ts, tt, pairs, coef):
    ls = F.log_softmax(s / ts, dim=1)
    tp = F.softmax((t - c) / tt, dim=1)
    return coef * sum(-(tp[q].sum(0) * ls[i]).sum() for i, q in enumerate(pairs))


@pytest.mark.parametrize("regime", ["normal", "underflow", "onehot"])
def test_dino_ce_backward_is_autograd_of_softmax_cross_entropy(regime):
    s, t, c = SO.dino_inputs(regime, 6, 6, 37, seed=3)
    o = SO.dino_ce(s, t, c, SO.f32(0.1), SO.f32(0.04), grad_scale=0.7)
    st = T(s, True)
    loss = _dino_torch(st, T(t), T(c), SO.f32(0.1), SO.f32(0.04), [[(i + 3) % 6] for i in range(6)], 1.0 / 6)
    loss.backward()
    same(o["loss"], loss); same(o["ds"], SO.f32(0.7) * st.grad)
    assert np.isfinite(o["ds"]).all() and np.isfinite(o["row"]).all()


@pytest.mark.parametrize("G,views,B", [(2, 2, 1), (2, 5, 3), (3, 3, 2), (1, 2, 5)])
def test_dino_ce_multi_backward_is_autograd(G, views, B):
    s, t, c = SO.dino_inputs("normal", views * B, G * B, 19, seed=4)
    o = SO.dino_ce_multi(s, t, c, SO.f32(0.1), SO.f32(0.04), G, grad_scale=1.3)
    st = T(s, True)
    pairs = [[q * B + b for q in range(G) if q != v] for v in range(views) for b in range(B)]
    loss = _dino_torch(st, T(t), T(c), SO.f32(0.1), SO.f32(0.04), pairs, 1.0 / (B * G * (views - 1)))
    loss.backward()
    same(o["loss"], loss); same(o["ds"], SO.f32(1.3) * st.grad)
    if (G, views) == (2, 2):                                             # two global views: the two-view loss
        two = SO.dino_ce(s, t, c, SO.f32(0.1), SO.f32(0.04), grad_scale=1.3)
        same(two["loss"], o["loss"], 1e-14); same(two["ds"], o["ds"], 1e-14)


def test_gram_normalize_backward_is_autograd_of_normalize_with_its_clamp():
    sf, tf = SO.gram_inputs(3, 6, 9, seed=5)
    o = SO.gram_normalize(sf, tf)
    x = T(sf, True)
    xh = F.normalize(x[:, 1:], dim=-1)
    same(o["shat"], xh); same(o["cat"][..., 9:], F.normalize(T(tf)[:, 1:], dim=-1)); same(o["catneg"][..., 9:], -o["cat"][..., 9:], 0.0)
    assert o["snorm"][0, 0] == SO.NORM_CLAMP and o["snorm"][2, 4] == SO.NORM_CLAMP and (o["shat"][0, 0] == 0).all()
    assert abs(np.linalg.norm(o["shat"][2, 4]) - 0.1) < 1e-6            # 1e-13 / 1e-12: the clamp divides, it does not normalise
    dxh = np.random.default_rng(6).standard_normal((3, 5, 9))
    (xh * T(dxh)).sum().backward()
    d, _, _ = SO.gram_normalize_bwd(dxh, o["shat"], o["snorm"])
    want = x.grad[:, 1:].numpy()
    assert np.abs(d - want).max() <= 1e-10 * np.abs(want).max() and (x.grad[:, 0] == 0).all()
    assert np.allclose(d[0, 0], dxh[0, 0] * 1e12, rtol=1e-8) and np.abs(d[0, 0]).min() > 0


def test_gelu_grad_is_autograd_of_gelu():
    x = np.concatenate([np.linspace(-10, 10, 401), [0.0, -0.0, 30.0, -30.0, 1e-40]])
    xt = T(x, True)
    y = F.gelu(xt)
    y.sum().backward()
    same(SO.gelu(x), y, 1e-14); same(SO.gelu_grad(x), xt.grad, 1e-13)


def test_adamw_step_is_torch_adamw_and_colmean_center_are_their_formulas():
    r = np.random.default_rng(7)
    n = 23
    p, g, m, v, tch = r.standard_normal(n), r.standard_normal(n), 0.1 * r.standard_normal(n), 0.01 * np.abs(r.standard_normal(n)), r.standard_normal(n)
    hp = dict(lr=SO.f32(2e-3), wd=SO.f32(0.04), b1=SO.f32(0.9), b2=SO.f32(0.999), eps=SO.f32(1e-8))
    w = T(p, True)
    opt = torch.optim.AdamW([w], lr=hp["lr"], betas=(hp["b1"], hp["b2"]), eps=hp["eps"], weight_decay=hp["wd"])
    w.grad = T(0.5 * g)
    opt.state[w] = {"step": torch.tensor(2.0), "exp_avg": T(m), "exp_avg_sq": T(v)}
    opt.step()
    pn, mn, vn, tn, gsq = SO.adamw_ema(p, g, m, v, tch, 3, 2e-3, 0.04, 0.9, 0.999, 1e-8, 0.996, grad_scale=0.5)
    same(pn, w, 1e-12); same(mn, opt.state[w]["exp_avg"], 1e-14); same(vn, opt.state[w]["exp_avg_sq"], 1e-14)
    same(tn, SO.f32(0.996) * tch + (1 - SO.f32(0.996)) * pn, 1e-15)
    assert abs(gsq - float((0.25 * g * g).sum())) <= 1e-12 * gsq
    assert SO.adamw_ema(p, g, m, v, None, 3, 2e-3, 0.04, 0.9, 0.999, 1e-8, 0.996)[3] is None
    t = r.standard_normal((5, 7))
    same(SO.colmean(t)[0], T(t).mean(0), 1e-15)
    same(SO.center_ema(t[0], t[1], 0.9)[0], SO.f32(0.9) * t[0] + (1 - SO.f32(0.9)) * t[1], 1e-15)
    assert SO.lincomb3(2.0, None, 3.0, 9.0, 0.5) == (3.5, 3.5) and SO.lincomb3(2.0, -1.0, None, 0.5, 9.0) == (1.5, 2.5)


# ------------------------------------------------------------------------------------------ fixtures recorded from the reference
def test_dino_oracle_matches_the_reference_fixture():
    """Tolerances of test_dino_loss_golden (the fixture is the reference's own fp32 arithmetic)."""
    g = load_golden("dino_loss.npz")
    ts, tt = float(g["student_temp"]), float(g["teacher_temp"])
    o = SO.dino_ce(g["s"], g["t"], g["center0"], ts, tt)
    assert abs(o["loss"] - float(g["loss1"])) <= 1e-5 * float(g["loss1"])
    assert np.abs(o["ds"] - g["ds1"]).max() <= 1e-4 * np.abs(g["ds1"]).max() + 1e-8
    c1, _ = SO.center_ema(g["center0"].reshape(-1), SO.colmean(g["t"])[0], float(g["momentum"]))
    assert np.abs(c1 - g["center1"].reshape(-1)).max() <= 1e-5 * np.abs(g["center1"]).max() + 1e-7
    o2 = SO.dino_ce(g["s"], g["t2"], c1, ts, tt)
    assert abs(o2["loss"] - float(g["loss2"])) <= 1e-5 * float(g["loss2"])


def test_gram_oracle_matches_the_reference_fixture():
    g = load_golden("gram_loss.npz")
    sf, tf = g["sf"], g["tf"]
    V, N, D = sf.shape
    T_ = N - 1
    o = SO.gram_normalize(sf, tf)
    gs = o["shat"] @ o["shat"].transpose(0, 2, 1)
    assert np.abs(gs - g["gram_s"]).max() <= 1e-6
    diff = o["cat"] @ o["catneg"].transpose(0, 2, 1)                      # Gs - Gt in one product, as the step forms it
    loss = (diff ** 2).mean()
    assert abs(loss - float(g["loss"])) <= 1e-5 * float(g["loss"])
    d, _, _ = SO.gram_normalize_bwd((4.0 / (V * T_ * T_)) * (diff @ o["shat"]), o["shat"], o["snorm"])
    want = g["dsf"].astype(np.float64)
    assert (want[:, 0] == 0).all()
    zero = np.argwhere(o["snorm"] <= SO.NORM_CLAMP)
    assert len(zero) == 1                                                # the fixture's zero-norm token: 1e12-scaled round-off there
    v0, t0 = zero[0]
    d[v0, t0] = 0; want[v0, 1 + t0] = 0
    assert np.abs(d - want[:, 1:]).max() <= 2e-4 * np.abs(want).max() + 1e-8


def test_scale_embed_oracle_matches_the_reference_fixture():
    g = load_golden("ops_scale_embed.npz")
    w = {k[2:]: v for k, v in g.items() if k.startswith("w/")}
    f = SO.scale_embed_fwd(g["spacing"], w["mlp.0.weight"], w["mlp.0.bias"], w["mlp.2.weight"], w["mlp.2.bias"], w["mlp.3.weight"], w["mlp.3.bias"])
    assert np.abs(f["out"] - g["y"][:, 0]).max() <= 1e-4 * np.abs(g["y"]).max() + 1e-5
    b = SO.scale_embed_bwd(g["dy"][:, 0], g["spacing"], w["mlp.0.weight"], w["mlp.2.weight"], w["mlp.3.weight"], f["hpre"], f["e"], f["mean"], f["rstd"])
    for k, name in (("dw0", "mlp.0.weight"), ("db0", "mlp.0.bias"), ("dw2", "mlp.2.weight"), ("db2", "mlp.2.bias"), ("dlnw", "mlp.3.weight"),
                    ("dlnb", "mlp.3.bias")):
        assert np.abs(b[k] - g["g/" + name]).max() <= 5e-4 * np.abs(g["g/" + name]).max() + 1e-5, k
    assert np.abs(b["dspacing"] - g["dspacing"]).max() <= 5e-4 * np.abs(g["dspacing"]).max() + 1e-5


# ------------------------------------------------------------------------------------------ an fp32 evaluation stays inside the bounds
@pytest.mark.parametrize("regime", ["normal", "underflow", "onehot"])
@pytest.mark.parametrize("rows,K", [(2, 1), (6, 7), (2, 255), (6, 257), (2, 1000), (6, 65536)])
def test_fp32_dino_ce_stays_inside_its_bound(regime, rows, K):
    s, t, c = SO.dino_inputs(regime, rows, rows, K, seed=K + rows)
    o = SO.dino_ce(s, t, c, SO.f32(0.1), SO.f32(0.04), grad_scale=0.7)
    b = SO.bound_dino(o)
    lo = SO.dino_ce(s, t, c, 0.1, 0.04, grad_scale=0.7, dt=F32)
    inside(lo["row"], o["row"], b["row"] + SO.CE_LOSS_RTOL * np.abs(o["row"]), "row loss")
    inside(lo["ds"], o["ds"], b["ds"] + SO.CE_DS_RTOL * np.abs(o["ds"]).max(1, keepdims=True), "ds")
    inside(lo["loss"], o["loss"], b["loss"] + SO.CE_LOSS_RTOL * abs(o["loss"]), "loss")
    if regime == "underflow" and K >= 255:
        assert (np.exp((o["zs"] - o["ms"]).astype(F32)) == 0).mean() > 0.5          # most student exponentials do underflow
    if regime == "onehot":
        assert (o["tp"].max(1) > 1 - 1e-6).all() and np.abs(c).min() == 50


@pytest.mark.parametrize("G,views,B,K", [(2, 2, 1, 7), (2, 5, 3, 257), (3, 3, 2, 1000), (1, 2, 5, 257)])
def test_fp32_dino_ce_multi_stays_inside_its_bound(G, views, B, K):
    s, t, c = SO.dino_inputs("normal", views * B, G * B, K, seed=K + G)
    o = SO.dino_ce_multi(s, t, c, SO.f32(0.1), SO.f32(0.04), G, grad_scale=1.3)
    b = SO.bound_dino(o)
    lo = SO.dino_ce_multi(s, t, c, 0.1, 0.04, G, grad_scale=1.3, dt=F32)
    inside(lo["row"], o["row"], b["row"] + SO.CE_LOSS_RTOL * np.abs(o["row"]), "row loss")
    inside(lo["ds"], o["ds"], b["ds"] + SO.CE_DS_RTOL * np.abs(o["ds"]).max(1, keepdims=True), "ds")


@pytest.mark.parametrize("V,h,D", [(1, 16, 64), (9, 100, 384), (17, 300, 600)])
def test_fp32_scale_embed_stays_inside_its_bounds(V, h, D):
    i = SO.se_inputs(V, h, D, seed=V)
    args = [i[k] for k in ("sp", "w0", "b0", "w2", "b2", "lnw", "lnb")]
    lo = SO.scale_embed_fwd(*args, eps=1e-5, dt=F32)
    assert lo["out"].dtype == F32
    for k, (ref, bound) in SO.bound_se_fwd(*args, 1e-5, lo).items():
        inside(lo[k], ref, bound, k)
    assert np.abs(lo["out"]).max() > 0.5                                 # weights away from init: the output is not ~0
    de, _ = SO.se_bwd_de(i["dout"], i["lnw"], lo["e"], lo["mean"], lo["rstd"], dt=F32)
    dh, _, _ = SO.se_bwd_dh(de, i["w2"], lo["hpre"], dt=F32)
    got = {"de": de, "dhpre": dh, "hact": SO.gelu(lo["hpre"])}
    got.update({k: v[0] for k, v in SO.se_bwd_params(i["dout"], i["sp"], got["hact"], lo["e"], lo["mean"], lo["rstd"], de, dh, dt=F32).items()})
    got["dspacing"] = SO.se_bwd_dsp(dh, i["w0"], dt=F32)[0]
    for k, (ref, bound) in SO.bound_se_bwd(i["dout"], i["sp"], i["w0"], i["w2"], i["lnw"], lo, got).items():
        inside(got[k], ref, bound, k)


def test_fp32_reductions_and_elementwise_steps_stay_inside_their_bounds():
    r = np.random.default_rng(11)
    dtok = r.standard_normal((33, 1 + 4 + 4, 260)).astype(F32)
    o, lo = SO.tokens_bwd(dtok, 4, 4), SO.tokens_bwd(dtok, 4, 4, dt=F32)
    for k, bound in SO.bound_tokens_bwd(o, 33, 4).items():
        inside(lo[k][0], o[k][0], bound, k)
    t = r.standard_normal((33, 260)).astype(F32)
    inside(SO.colmean(t, dt=F32)[0], SO.colmean(t)[0], (33 + 1 + 2) * SO.U * SO.colmean(t)[1], "colmean")
    ce = SO.center_ema(t[0], t[1], SO.f32(0.9))
    inside(SO.center_ema(t[0], t[1], 0.9, dt=F32)[0], ce[0], (4 + 2) * SO.U * ce[1], "center_ema")
    for V, N, D in ((1, 2, 32), (3, 6, 65), (2, 5, 384)):
        sf, tf = SO.gram_inputs(V, N, D, seed=D)
        o, lo = SO.gram_normalize(sf, tf), SO.gram_normalize(sf, tf, dt=F32)
        for k, bound in SO.bound_gram_normalize(o, D).items():
            inside(lo[k], o[k], bound, k)
        dxh = r.standard_normal((V, N - 1, D)).astype(F32)
        sh, sn = o["shat"].astype(F32), o["snorm"].astype(F32)
        ref, bound = SO.bound_gram_normalize_bwd(dxh, sh, sn)
        inside(SO.gram_normalize_bwd(dxh, sh, sn, dt=F32)[0], ref, bound, "gram bwd")
        assert V * (N - 1) == 1 or (sn[0, 0] == F32(1e-12) and np.abs(ref[0, 0]).max() > 1e11)          # a clamped row with non-zero data
    n = 10007
    p, g, m, v, tch = (a.astype(F32) for a in (r.standard_normal(n), r.standard_normal(n), 0.1 * r.standard_normal(n),
                                               0.01 * np.abs(r.standard_normal(n)), r.standard_normal(n)))
    hp = (3, 2e-3, 0.04, 0.9, 0.999, 1e-8, 0.996)
    ref = SO.adamw_ema(p, g, m, v, tch, *hp, grad_scale=0.5)
    b = SO.bound_adamw(p, g, m, v, tch, *hp, 0.5, ref)
    lr, wd, b1, b2, eps, ema = (F32(a) for a in hp[1:])
    gr = g * F32(0.5)
    mn = b1 * m + (F32(1) - b1) * gr
    vn = b2 * v + (F32(1) - b2) * gr * gr
    ibc1, isb = F32(1.0 / (1.0 - float(b1) ** 3)), F32(1.0 / np.sqrt(1.0 - float(b2) ** 3))
    pn = p * (F32(1) - lr * wd) - lr * ibc1 * (mn / (np.sqrt(vn) * isb + eps))
    tn = ema * tch + (F32(1) - ema) * pn
    for k, got, want in (("p", pn, ref[0]), ("m", mn, ref[1]), ("v", vn, ref[2]), ("teacher", tn, ref[3])):
        assert got.dtype == F32
        inside(got, want, b[k], "adamw " + k)


# ------------------------------------------------------------------------------------------ argument contracts of the C entry points
def test_abi_rejects_bad_arguments_without_a_launch():
    """The checks run on the host, ahead of the launch: the pointers below are never dereferenced."""
    from dinox import _lib
    lib = _lib.lib
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    p = p + (-p) % 16                                                    # a 16-byte aligned address inside the buffer
    EINVAL, EALIGN = -1, -3
    err = _lib.last_error

    assert lib.dinox_patch_unfold(None, p, 1, 8, 8, 4, 0, None) == EINVAL and "null" in err()
    assert lib.dinox_patch_unfold(p, p, 1, 8, 9, 4, 0, None) == EINVAL and "W=9" in err()
    assert lib.dinox_patch_unfold(p, p, 1, 8, 8, 4, 2, None) == EINVAL and "dtype" in err()
    assert lib.dinox_patch_unfold_ld(p, p, 1, 8, 8, 4, 47, 0, None) == EINVAL and "ld=47" in err()

    assert lib.dinox_tokens_fwd(p, p, None, None, None, p, 2, 4, 0, 8, 0, None) == EINVAL and "null" in err()
    assert lib.dinox_tokens_fwd(p, p, p, None, None, p, 2, 4, 4, 8, 0, None) == EINVAL and "R=4" in err()          # R > 0, no registers
    assert lib.dinox_tokens_fwd(p, p, p, None, None, p, 2, 4, 0, 8, 5, None) == EINVAL and "dtype" in err()
    assert lib.dinox_tokens_bwd(p, None, p, p, None, None, 2, 4, 0, 8, 0, None) == EINVAL and "null" in err()
    assert lib.dinox_tokens_bwd(p, p, p, p, None, None, 2, 4, 4, 8, 0, None) == EINVAL and "R=4" in err()

    a12 = [p] * 12
    assert lib.dinox_scale_embed_fwd(*([None] + a12[1:]), 2, 16, 64, 1e-5, None) == EINVAL and "null" in err()
    assert lib.dinox_scale_embed_fwd(*a12, 2, 8193, 64, 1e-5, None) == EINVAL and "h=8193" in err()
    a17 = [p] * 17
    assert lib.dinox_scale_embed_bwd(*(a17[:16] + [None]), 2, 16, 64, None) == EINVAL and "null" in err()          # no workspace
    assert lib.dinox_scale_embed_bwd(*a17, 2, 8192, 8192, None) == EINVAL and "D=8192" in err()                    # (D + h + 16) floats > 64 KiB of LDS
    assert lib.dinox_scale_embed_bwd(*a17, 2, 8184, 8185, None) == EINVAL and "D=8185" in err()                    # one float over the limit
    assert lib.dinox_scale_embed_bwd_ws_bytes(3, 16, 64) == 3 * (64 + 32) * 4 and lib.dinox_scale_embed_bwd_ws_bytes(0, 16, 64) == 0

    assert lib.dinox_dino_ce(p, p, p, 0.1, 0.04, 1.0, p, p, None, 4, 8, None) == EINVAL and "null" in err()
    assert lib.dinox_dino_ce(p, p, p, 0.1, 0.04, 1.0, p, p, p, 3, 8, None) == EINVAL and "rows=3" in err()
    assert lib.dinox_dino_ce(p, p, p, 0.0, 0.04, 1.0, p, p, p, 4, 8, None) == EINVAL and "temperatures" in err()
    assert lib.dinox_dino_ce(p, p, p, 0.1, -0.04, 1.0, p, p, p, 4, 8, None) == EINVAL and "temperatures" in err()
    assert lib.dinox_dino_ce_multi(p, p, p, 0.1, 0.04, 1.0, p, p, p, 2, 3, 2, 8, None) == EINVAL and "global=3" in err()     # views < globals
    assert lib.dinox_dino_ce_multi(p, p, p, 0.1, 0.0, 1.0, p, p, p, 2, 2, 2, 8, None) == EINVAL and "temperatures" in err()
    assert lib.dinox_colmean(p, None, 4, 8, None) == EINVAL and lib.dinox_colmean(p, p, 0, 8, None) == EINVAL and "colmean" in err()
    assert lib.dinox_center_ema(p, p, 0.9, 0, None) == EINVAL and "center_ema" in err()
    assert lib.dinox_gram_normalize(p, p, p, p, p, None, 2, 5, 8, 0, None) == EINVAL and "null" in err()
    assert lib.dinox_gram_normalize(p, p, p, p, p, p, 2, 1, 8, 0, None) == EINVAL and "N=1" in err()                # no patch tokens
    assert lib.dinox_gram_normalize_bwd(p, p, p, None, p, 2, 5, 8, 3, 0, None) == EINVAL and "dtype" in err()

    assert lib.dinox_take_rows(None, p, 2, 40, 8, 0, 0, None) == EINVAL and "take_rows" in err()
    assert lib.dinox_take_rows(p, p, 2, 30, 6, 0, 0, None) == EINVAL and "D=6" in err()                             # D % 4 != 0
    assert lib.dinox_take_rows(p, p, 2, 42, 8, 0, 0, None) == EINVAL and "stride=42" in err()
    assert lib.dinox_take_rows(p + 4, p, 2, 40, 8, 0, 0, None) == EALIGN and "aligned" in err()
    assert lib.dinox_take_rows(p, p + 8, 2, 40, 8, 0, 1, None) == EALIGN and "aligned" in err()
    assert lib.dinox_take_rows(p, p, 2, 40, 8, 0, 7, None) == EINVAL and "dtype" in err()
    assert lib.dinox_put_rows(p, None, 2, 40, 8, 0, 0, 0, None) == EINVAL and "put_rows" in err()
    assert lib.dinox_put_rows(p, p, 2, 40, 8, -1, 0, 0, None) == EINVAL and lib.dinox_put_rows(p, p, 2, 40, 8, 0, 9, 0, None) == EINVAL and "dtype" in err()
    assert lib.dinox_axpy(p, None, 1.0, 8, None) == EINVAL and lib.dinox_axpy(p, p, 1.0, 0, None) == EINVAL and "axpy" in err()
    assert lib.dinox_lincomb3(None, p, p, 1.0, 1.0, p, None) == EINVAL and "lincomb3" in err()

    adam = lambda *ptrs, n=8, step=1: lib.dinox_adamw_ema(*ptrs, n, 1e-3, 0.04, 0.9, 0.999, 1e-8, step, 0.99, 1.0, p, p, None)
    assert adam(p, p, p, p, p, step=0) == EINVAL and "step_t=0" in err()
    assert adam(p, p, p, p + 4, p) == EALIGN and "aligned" in err()
    assert adam(p, p, p, p, p + 8) == EALIGN and "aligned" in err()                                                  # the teacher arena too
    assert adam(p, None, p, p, None) == EINVAL and "null" in err()
    assert adam(p, p, p, p, None, n=0) == EINVAL and "n=0" in err()
    assert lib.dinox_adamw_ema_dev(p, p, p, p, p, 8, None, 0.04, 0.9, 0.999, 1e-8, 0.99, 1.0, p, p, None) == EINVAL and "hyper" in err()
    assert lib.dinox_sumsq(p, 0, p, p, None) == EINVAL and lib.dinox_cast_bf16(p, None, 8, None) == EINVAL
    assert lib.dinox_cast_transpose_bf16(p, p, 0, 4, None) == EINVAL and "cast_transpose" in err()
    assert lib.dinox_cast_transpose_bf16_multi(p, p, p, 0, 4, None) == EINVAL and "n_mats=0" in err()
    assert lib.dinox_gelu_fwd(p, p, 0, None) == EINVAL and lib.dinox_gelu_bwd(p, None, p, 8, None) == EINVAL and "gelu_bwd" in err()
