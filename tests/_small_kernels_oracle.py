"""Plain NumPy float64 statements of the small kernels of a training step -- csrc/tokens.hip, scale_embed.hip, loss.hip, optim.hip and
glue.hip -- written from the formulas in include/dinox.h and the comments at the kernels; no project code is called (oracle/kernels_np
states the AdamW step already and is reused).  Every reduction also returns the sum of the absolute values of its terms per output
element, from which the second half of this file builds the elementwise fp32 error bounds of tests/test_small_kernels_gpu.py.
tests/test_small_kernels_cpu.py proves the statements against float64 autograd and the recorded fixtures, and evaluates the same
formulas in NumPy float32 (``dt=np.float32``) to show that an honest fp32 evaluation of the test inputs stays inside those bounds."""
import math

import numpy as np
from scipy.special import erf

from oracle import kernels_np as KNP

F64 = np.float64
U = 2.0 ** -24                    # unit roundoff of fp32
TINY = 1e-37                      # room for a result that rounds into the fp32 subnormal range
GELU_RTOL = 1e-5                  # the project's tolerance for erff / __expf in GELU (test_gemm_f32_epilogues_and_batch)
CE_LOSS_RTOL, CE_DS_RTOL = 1e-5, 1e-4   # ... and for expf / logf in the DINO cross-entropy (test_dino_loss_golden)


def _sum(x, axis):
    """(sum, sum of absolute terms) along axis."""
    return x.sum(axis), np.abs(x).sum(axis)


def f32(x):
    """The fp32 value of a host scalar the C ABI takes as float, as a Python float."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------ tokens.hip
def unfold(x, p):
    """[V,3,H,W] -> [V * gh * g, 3 p^2]: row (v, gy, gx), column c p^2 + py p + px holds x[v, c, gy p + py, gx p + px].  Index
    arithmetic on purpose (no reshape / transpose): H and W each appear once.  unfold_ld pads the rows with zeros to ld columns."""
    x = np.asarray(x)
    V, _, H, W = x.shape
    gh, g = H // p, W // p
    row, k = np.arange(gh * g), np.arange(3 * p * p)
    gy, gx = row // g, row % g
    c, py, px = k // (p * p), (k // p) % p, k % p
    return x[:, c[None, :], gy[:, None] * p + py[None, :], gx[:, None] * p + px[None, :]].reshape(V * gh * g, 3 * p * p)


def unfold_ld(x, p, ld):
    u = unfold(x, p)
    return np.concatenate([u, np.zeros((u.shape[0], ld - u.shape[1]), u.dtype)], axis=1)


def tokens_fwd(patches, cls, pos, regs, scale, dt=F64):
    """patches [V,P,D], cls [D], pos [1+P,D], regs [R,D] or None, scale [V,D] or None -> tokens [V, 1+P+R, D]."""
    patches, cls, pos = np.asarray(patches, dt), np.asarray(cls, dt), np.asarray(pos, dt)
    V, P, D = patches.shape
    tok = np.concatenate([np.broadcast_to(cls, (V, 1, D)), patches], axis=1) + pos[None]
    if scale is not None:
        tok = tok + np.asarray(scale, dt)[:, None, :]
    if regs is not None:
        regs = np.asarray(regs, dt)
        tok = np.concatenate([tok, np.broadcast_to(regs, (V,) + regs.shape)], axis=1)
    return tok


def tokens_bwd(dtok, P, R, dt=F64):
    """dtok [V, 1+P+R, D] -> dict of (value, abs sum): dpatches [V,P,D] (a copy), dcls [D], dpos [1+P,D], dregs [R,D], dscale [V,D]."""
    dtok = np.asarray(dtok, dt)
    body = dtok[:, :1 + P]
    dpos = _sum(body, 0)
    return {"dpatches": (body[:, 1:], np.abs(body[:, 1:])), "dpos": dpos, "dcls": (dpos[0][0], dpos[1][0]),
            "dregs": _sum(dtok[:, 1 + P:], 0), "dscale": _sum(body, 1)}


# ------------------------------------------------------------------------------------------ GELU (exact erf)
def gelu(x):
    return 0.5 * x * (1.0 + erf(x * math.sqrt(0.5)))


def gelu_grad(x):
    return 0.5 * (1.0 + erf(x * math.sqrt(0.5))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_tol(x, ref):
    """|x| + 1 units of 2^-22 for the cancellation in 1 + erf (and x exp(-x^2/2) of the derivative), plus the project's 1e-5."""
    return (np.abs(x) + 1.0) * 2.0 ** -22 + GELU_RTOL * np.abs(ref)


# ------------------------------------------------------------------------------------------ scale_embed.hip
# Linear(3,h) -> GELU -> Linear(h,D) -> LayerNorm(D), one row per image.  Stated in stages, so that a test can hand each stage the
# intermediate the kernel itself produced (hpre, e, mean, rstd are outputs of the forward and inputs of the backward).
def se_hidden(sp, w0, b0, dt=F64):
    sp, w0, b0 = np.asarray(sp, dt), np.asarray(w0, dt), np.asarray(b0, dt)
    terms = sp[:, None, :] * w0[None]                                   # [V,h,3]
    return b0 + terms.sum(2), np.abs(b0) + np.abs(terms).sum(2)


def se_project(hpre, w2, b2, dt=F64):
    """-> e [V,D], its abs sum, and sum_j |w2[d,j]| tol_j for an error tol_j of the activation a_j."""
    hpre, w2, b2 = np.asarray(hpre, dt), np.asarray(w2, dt), np.asarray(b2, dt)
    a = gelu(hpre)
    return b2 + a @ w2.T, np.abs(b2) + np.abs(a) @ np.abs(w2).T, gelu_tol(hpre, a) @ np.abs(w2).T


def se_norm(e, lnw, lnb, eps, mean=None, rstd=None, dt=F64):
    e, lnw, lnb = np.asarray(e, dt), np.asarray(lnw, dt), np.asarray(lnb, dt)
    mu = e.mean(1) if mean is None else np.asarray(mean, dt)
    c = e - mu[:, None]
    rs = 1.0 / np.sqrt((c * c).mean(1) + dt(f32(eps))) if rstd is None else np.asarray(rstd, dt)
    xh = c * rs[:, None]
    return xh * lnw + lnb, np.abs(xh * lnw) + np.abs(lnb), mu, rs


def scale_embed_fwd(sp, w0, b0, w2, b2, lnw, lnb, eps=1e-5, dt=F64):
    hpre, _ = se_hidden(sp, w0, b0, dt)
    e, _, _ = se_project(hpre, w2, b2, dt)
    out, _, mean, rstd = se_norm(e, lnw, lnb, eps, dt=dt)
    return {"out": out, "hpre": hpre, "e": e, "mean": mean, "rstd": rstd}


def se_bwd_de(dout, lnw, e, mean, rstd, dt=F64):
    """LayerNorm backward of a row: de = rstd (g - mean(g) - xh mean(g xh)), g = dout lnw.  Also returns what the bound needs."""
    dout, lnw, e, mean, rstd = (np.asarray(a, dt) for a in (dout, lnw, e, mean, rstd))
    g = dout * lnw
    xh = (e - mean[:, None]) * rstd[:, None]
    m1, a1 = g.mean(1), np.abs(g).mean(1)
    m2, a2 = (g * xh).mean(1), np.abs(g * xh).mean(1)
    de = rstd[:, None] * (g - m1[:, None] - xh * m2[:, None])
    return de, {"g": g, "xh": xh, "m1": m1, "a1": a1, "m2": m2, "a2": a2, "rstd": rstd}


def se_bwd_dh(de, w2, hpre, dt=F64):
    de, w2, hpre = np.asarray(de, dt), np.asarray(w2, dt), np.asarray(hpre, dt)
    s, sa = de @ w2, np.abs(de) @ np.abs(w2)                             # [V,h]
    return s * gelu_grad(hpre), s, sa


def se_bwd_dsp(dhpre, w0, dt=F64):
    dhpre, w0 = np.asarray(dhpre, dt), np.asarray(w0, dt)
    return dhpre @ w0, np.abs(dhpre) @ np.abs(w0)


def se_bwd_params(dout, sp, hact, e, mean, rstd, de, dhpre, dt=F64):
    """Six parameter gradients, each a sum over the V rows: name -> (value, abs sum)."""
    dout, sp, hact, e, mean, rstd, de, dhpre = (np.asarray(a, dt) for a in (dout, sp, hact, e, mean, rstd, de, dhpre))
    xh = (e - mean[:, None]) * rstd[:, None]
    return {"dw2": _sum(de[:, :, None] * hact[:, None, :], 0), "db2": _sum(de, 0),
            "dw0": _sum(dhpre[:, :, None] * sp[:, None, :], 0), "db0": _sum(dhpre, 0),
            "dlnw": _sum(dout * xh, 0), "dlnb": _sum(dout, 0)}


def scale_embed_bwd(dout, sp, w0, w2, lnw, hpre, e, mean, rstd, dt=F64):
    de, _ = se_bwd_de(dout, lnw, e, mean, rstd, dt)
    dhpre, _, _ = se_bwd_dh(de, w2, hpre, dt)
    out = {k: v[0] for k, v in se_bwd_params(dout, sp, gelu(np.asarray(hpre, dt)), e, mean, rstd, de, dhpre, dt).items()}
    out["dspacing"] = se_bwd_dsp(dhpre, w0, dt)[0]
    return out


# ------------------------------------------------------------------------------------------ loss.hip
def _softmax_parts(z):
    m = z.max(1, keepdims=True)
    ex = np.exp(z - m)
    sm = ex.sum(1, keepdims=True)
    return m, ex, sm


def _dino(s, t, center, ts, tt, pairs, coef, nq, grad_scale, dt):
    """Shared tail of the two cross-entropies: pairs[i] lists the teacher rows student row i is scored against."""
    s, t, center = np.asarray(s, dt), np.asarray(t, dt), np.asarray(center, dt).reshape(1, -1)
    ts, tt, grad_scale = dt(f32(ts)), dt(f32(tt)), f32(grad_scale)     # the C ABI takes these as float
    zt = (t - center) / tt
    mt, et, st = _softmax_parts(zt)
    tp = et / st                                                         # softmax((t - c) / tt), per teacher row
    zs = s / ts
    ms, es, ss = _softmax_parts(zs)
    lse = np.log(ss)
    ls = zs - ms - lse                                                   # log_softmax(s / ts)
    p = es / ss
    tpi = np.stack([tp[q].sum(0) for q in pairs])                        # [rows, K]
    row, row_abs = -(tpi * ls).sum(1), (tpi * (np.abs(zs - ms) + np.abs(lse))).sum(1)
    nq = np.asarray(nq, dt)[:, None]
    ds = dt(grad_scale) * dt(coef) * (nq * p - tpi) / ts
    return {"loss": dt(coef) * row.sum(), "row": row, "row_abs": row_abs, "ds": ds, "zt": zt, "mt": mt, "et": et, "st": st, "tp": tp,
            "zs": zs, "ms": ms, "es": es, "ss": ss, "lse": lse, "ls": ls, "p": p, "tpi": tpi, "pairs": pairs, "nq": nq,
            "c": abs(float(grad_scale) * float(coef) / float(ts)), "coef": float(coef)}


def dino_ce(s, t, center, ts, tt, grad_scale=1.0, dt=F64):
    """s, t [2B,K] = [view 1; view 2]: student row i against teacher row (i + B) mod 2B.  row[i] = -sum_k p_t[k] log_softmax(s_i / ts)[k],
    loss = mean(row), ds = grad_scale d loss / d s."""
    rows = np.asarray(s).shape[0]
    pairs = [[(i + rows // 2) % rows] for i in range(rows)]
    return _dino(s, t, center, ts, tt, pairs, 1.0 / rows, [1] * rows, grad_scale, dt)


def dino_ce_multi(s, t, center, ts, tt, n_global, grad_scale=1.0, dt=F64):
    """Student rows [views][B] (the first n_global views are the teacher's), teacher rows [n_global][B]: row (v, b) is scored against
    every teacher view q != v of sample b; loss = sum(row) / (B n_global (views - 1))."""
    G = n_global
    B = np.asarray(t).shape[0] // G
    views = np.asarray(s).shape[0] // B
    pairs = [[q * B + b for q in range(G) if q != v] for v in range(views) for b in range(B)]
    return _dino(s, t, center, ts, tt, pairs, 1.0 / (B * G * (views - 1)), [len(q) for q in pairs], grad_scale, dt)


def colmean(t, dt=F64):
    t = np.asarray(t, dt)
    return t.sum(0) / dt(t.shape[0]), np.abs(t).sum(0) / t.shape[0]


def center_ema(center, batch_mean, momentum, dt=F64):
    c, m, mom = np.asarray(center, dt), np.asarray(batch_mean, dt), dt(f32(momentum))
    return c * mom + m * (dt(1) - mom), np.abs(c * mom) + np.abs(m * (dt(1) - mom))


NORM_CLAMP = 1e-12               # (the kernel's 1e-12f and 1e12f are 4e-9 away from these: a fraction of one fp32 rounding)


def gram_normalize(sf, tf, dt=F64):
    """sf, tf [V,N,D] -> rows (v, token >= 1): shat = s / max(|s|, 1e-12), cat = [shat | that], catneg = [shat | -that], snorm."""
    xs, xt = np.asarray(sf, dt)[:, 1:], np.asarray(tf, dt)[:, 1:]
    ns = np.maximum(np.sqrt((xs * xs).sum(-1, keepdims=True)), dt(NORM_CLAMP))
    nt = np.maximum(np.sqrt((xt * xt).sum(-1, keepdims=True)), dt(NORM_CLAMP))
    a, b = xs / ns, xt / nt
    return {"shat": a, "cat": np.concatenate([a, b], -1), "catneg": np.concatenate([a, -b], -1), "snorm": ns[..., 0]}


def gram_normalize_bwd(dxh, shat, snorm, dt=F64):
    """Rows [V,T,D]: d = (g - shat (shat . g)) / norm; a row at the clamp (norm <= 1e-12) is x * 1e12 in the forward, so d = g * 1e12.
    -> (d, proj, abs sum of proj)."""
    g, sh, nrm = np.asarray(dxh, dt), np.asarray(shat, dt), np.asarray(snorm, dt)[..., None]
    proj, proj_abs = (sh * g).sum(-1, keepdims=True), np.abs(sh * g).sum(-1, keepdims=True)
    with np.errstate(over="ignore"):
        d = np.where(nrm > dt(NORM_CLAMP), (g - sh * proj) / nrm, g * dt(1e12))
    return d, proj, proj_abs


# ------------------------------------------------------------------------------------------ optim.hip, glue.hip
def adamw_ema(p, g, m, v, teacher, step_t, lr, wd, b1, b2, eps, ema, grad_scale=1.0):
    """oracle/kernels_np.adamw_ema on the fp32 values of the host scalars (the C entry takes floats: 1 - 0.999f is 1.3e-5 away from
    0.001).  teacher None: no EMA.  -> (p, m, v, teacher or None, sum (grad_scale g)^2)."""
    lr, wd, b1, b2, eps, ema, gs = (f32(a) for a in (lr, wd, b1, b2, eps, ema, grad_scale))
    p, g, m, v = (np.asarray(a, F64) for a in (p, g, m, v))
    tch = np.zeros_like(p) if teacher is None else np.asarray(teacher, F64)
    pn, mn, vn, tn, gsq = KNP.adamw_ema(p, gs * g, m, v, tch, step_t, lr, wd, b1, b2, eps, ema)
    return pn, mn, vn, (None if teacher is None else tn), gsq


def axpy(y, x, alpha):
    y, ax = np.asarray(y, F64), f32(alpha) * np.asarray(x, F64)
    return y + ax, np.abs(y) + np.abs(ax)


def lincomb3(a, b, c, wb, wc):
    terms = [float(a)] + ([f32(wb) * float(b)] if b is not None else []) + ([f32(wc) * float(c)] if c is not None else [])
    return sum(terms), sum(abs(x) for x in terms)


# ------------------------------------------------------------------------------------------ seeded inputs shared by the two test files
def dino_inputs(regime, srows, trows, K, seed):
    """fp32 (s, t, center).  normal: logits of a few units.  underflow: student logits spread over +-80, so that at student temperature
    0.1 most entries sit hundreds below the row maximum and their expf is 0.  onehot: a centre of magnitude 50 and teacher rows that
    stand 20 above it in one column (500 at teacher temperature 0.04): a softmax that is one-hot but for ~e^-500."""
    r = np.random.default_rng(seed)
    s, t, c = 2 * r.standard_normal((srows, K)), 2 * r.standard_normal((trows, K)), 0.5 * r.standard_normal(K)
    if regime == "underflow":
        s = r.uniform(-80, 80, (srows, K))
    elif regime == "onehot":
        c = 50 * np.sign(r.standard_normal(K))
        t = c + 0.1 * r.standard_normal((trows, K))
        t[np.arange(trows), r.integers(0, K, trows)] += 20
    else:
        assert regime == "normal"
    return s.astype(np.float32), t.astype(np.float32), c.astype(np.float32)


def se_inputs(V, h, D, seed):
    """fp32 spacing, the six parameters away from their init (so the output is not ~0) and an upstream gradient."""
    r = np.random.default_rng(seed)
    f = lambda *shape, s=1.0: (s * r.standard_normal(shape)).astype(np.float32)
    return {"sp": (r.uniform(0.4, 2.4, (V, 3))).astype(np.float32), "w0": f(h, 3), "b0": f(h, s=0.5), "w2": f(D, h, s=h ** -0.5), "b2": f(D, s=0.5),
            "lnw": (1 + f(D, s=0.3)), "lnb": f(D, s=0.3), "dout": f(V, D)}


def gram_inputs(V, N, D, seed):
    """fp32 (sf, tf).  With more than one token row: the first exactly zero, the last of norm 1e-13 (below the clamp; its squares,
    ~1e-26 / D, are normal in fp32)."""
    r = np.random.default_rng(seed)
    sf, tf = r.standard_normal((V, N, D)), r.standard_normal((V, N, D))
    if V * (N - 1) > 1:
        sf[0, 1] = 0.0
        row = r.standard_normal(D)
        sf[V - 1, N - 1] = 1e-13 * row / np.linalg.norm(row)
    return sf.astype(np.float32), tf.astype(np.float32)


# ========================================================================================== fp32 error bounds
# Every bound has the form  (n_ops + 2) u S  (+ terms carried over from an input that is itself rounded):  S the sum of the absolute
# terms of the element, n_ops the rounded operations on the longest path to it (the standard summation bound; +2 is head-room for FMA
# contraction and constants rounded on the host).
def block_adds(n):
    """Adds on the longest path of a 256-thread strided sum of n terms: the thread's own trips, 6 wave steps, 4 wave partials."""
    return -(-n // 256) + 10


def bound_tokens_bwd(o, V, P):
    """dcls / dpos / dregs: V terms in any order is at most V adds on a path (scalar kernel: V - 1 in a row; vector kernel: V/4 per
    slice, then 2 to join the slices).  dscale: P + 1 terms in a row."""
    b = {k: (V + 2) * U * o[k][1] + TINY for k in ("dcls", "dpos", "dregs")}
    b["dscale"] = (P + 1 + 2) * U * o["dscale"][1] + TINY
    return b


def bound_se_fwd(sp, w0, b0, w2, b2, lnw, lnb, eps, got):
    """Stage by stage on the kernel's own intermediates ``got`` (hpre, e, mean, rstd as fp32 arrays): -> name -> (ref, bound)."""
    h, D = w0.shape[0], w2.shape[0]
    nD = block_adds(D)
    hp, hp_abs = se_hidden(sp, w0, b0)
    out = {"hpre": (hp, (6 + 2) * U * hp_abs + TINY)}                     # 3 products + 3 adds
    e, e_abs, e_in = se_project(got["hpre"], w2, b2)
    out["e"] = (e, (h + 1 + 2) * U * e_abs + e_in + TINY)                # h adds in a row + the product; + |w2| . (GELU tolerance)
    ge = np.asarray(got["e"], F64)
    mu = ge.mean(1)
    bmu = (nD + 1 + 2) * U * np.abs(ge).mean(1) + TINY                   # block sum + the division
    out["mean"] = (mu, bmu)
    c = ge - mu[:, None]
    var = (c * c).mean(1)
    rs = 1.0 / np.sqrt(var + f32(eps))
    # c (1) squared (2: both factors) summed (nD) / D (1) + eps (1): relative (nD + 5 + 2) u on a sum of positive terms; the kernel's
    # own mean shifts the sum by D dmu^2 only (sum c = 0); sqrt halves a relative error; v_rsq_f32 is good to 1 ulp <= 2u, + 2.
    out["rstd"] = (rs, rs * (0.5 * ((nD + 7) * U + bmu ** 2 / np.maximum(var, 1e-300)) + 4 * U))
    y, y_abs, _, _ = se_norm(got["e"], lnw, lnb, eps, mean=got["mean"], rstd=got["rstd"])
    out["out"] = (y, (4 + 2) * U * y_abs + TINY)                          # e - mu, * rs, * lnw, + lnb
    return out


def bound_se_bwd(dout, sp, w0, w2, lnw, fwd, got):
    """fwd: the forward's hpre, e, mean, rstd (fp32, as the kernel read them); got: the kernel's workspace de, dhpre, hact.
    -> name -> (ref, bound) for de, dhpre, hact, dspacing and the six parameter gradients."""
    V, h, D = np.asarray(sp).shape[0], w0.shape[0], w2.shape[0]
    nD = block_adds(D)
    de, q = se_bwd_de(dout, lnw, fwd["e"], fwd["mean"], fwd["rstd"])
    bm1 = (nD + 2 + 2) * U * q["a1"]                                     # g (1), block sum, / D (1)
    bm2 = (nD + 5 + 2) * U * q["a2"]                                     # g (1), xh (2), product (1), block sum, / D (1)
    rs, xh = q["rstd"][:, None], np.abs(q["xh"])
    s_de = np.abs(q["g"]) + np.abs(q["m1"])[:, None] + xh * np.abs(q["m2"])[:, None]
    out = {"de": (de, rs * ((6 + 2) * U * s_de + bm1[:, None] + xh * bm2[:, None]) + TINY)}   # g (1) xh (2) xh m2 (1) two subtractions, * rs
    hp = np.asarray(fwd["hpre"], F64)
    dh, s, s_abs = se_bwd_dh(got["de"], w2, hp)
    gg = gelu_grad(hp)
    out["dhpre"] = (dh, np.abs(gg) * (D + 1 + 2) * U * s_abs + np.abs(s) * gelu_tol(hp, gg) + 2 * U * np.abs(dh) + TINY)
    out["hact"] = (gelu(hp), gelu_tol(hp, gelu(hp)))
    dsp, dsp_abs = se_bwd_dsp(got["dhpre"], w0)
    out["dspacing"] = (dsp, (h + 1 + 2) * U * dsp_abs + TINY)
    extra = {"dw2": 1, "db2": 0, "dw0": 1, "db0": 0, "dlnw": 3, "dlnb": 0}          # rounded operations inside one term
    for k, (val, a) in se_bwd_params(dout, sp, got["hact"], fwd["e"], fwd["mean"], fwd["rstd"], got["de"], got["dhpre"]).items():
        out[k] = (val, (V + extra[k] + 2) * U * a + TINY)                # at most V adds on a path of the 8-way partial sums
    return out


def bound_dino(o):
    """Bounds of row losses, ds and the loss of a _dino result, fp32 rounding carried through; the caller adds the project's
    tolerance for expf / logf (CE_LOSS_RTOL |row|, CE_DS_RTOL max_k |ds[row]|)."""
    K = o["zs"].shape[1]
    ns = block_adds(K)
    # argument of every exp: z - m, z = x (1/T): 1/T rounded, the product, the teacher's t - c, the subtraction: <= 4 operations
    da_s = (4 + 2) * U * (np.abs(o["zs"]) + np.abs(o["ms"]))
    da_t = (4 + 2) * U * (np.abs(o["zt"]) + np.abs(o["mt"]))
    # a sum of exps (all positive): the weighted mean of the argument errors, then the block sum
    rel_ss = (o["es"] * da_s).sum(1, keepdims=True) / o["ss"] + (ns + 2) * U
    rel_st = (o["et"] * da_t).sum(1, keepdims=True) / o["st"] + (ns + 2) * U
    dtp = o["tp"] * (da_t + rel_st + 2 * U)                              # exp(arg) * (1 / st)
    dp = o["p"] * (da_s + rel_ss + 2 * U)
    dls = da_s + rel_ss + U * np.abs(o["lse"]) + U * np.abs(o["ls"])     # log has condition 1 / |log| in relative terms: absolute rel_ss
    dtpi = np.stack([dtp[q].sum(0) for q in o["pairs"]]) + o["nq"] * U * o["tpi"]
    row = (dtpi * np.abs(o["ls"]) + o["tpi"] * dls).sum(1) + (ns + 1 + 2) * U * o["row_abs"] + TINY
    # nq p - tp, then * gscale * (1/ts) (/ rows): 4 operations on |nq p| + |tp|
    ds = o["c"] * (o["nq"] * dp + dtpi + (4 + 2) * U * (o["nq"] * o["p"] + o["tpi"])) + TINY
    n = len(o["row"])
    loss = o["coef"] * (row.sum() + (block_adds(n) + 1 + 2) * U * np.abs(o["row"]).sum()) + TINY
    return {"row": row, "ds": ds, "loss": loss}


def bound_gram_normalize(o, D):
    """Relative: sum of squares (x^2: 1, wave sum: ceil(D/64) + 6) -> sqrt halves it, + sqrt (1), 1/n (1), x * (1)."""
    nq = -(-D // 64) + 6
    rel = (0.5 * (nq + 1 + 2) + 3) * U
    return {k: rel * np.abs(o[k]) + TINY for k in ("shat", "cat", "catneg")} | {"snorm": (0.5 * (nq + 1 + 2) + 1) * U * o["snorm"]}


def bound_gram_normalize_bwd(dxh, shat, snorm, dst=None):
    """proj: D/64 strided products, 6 wave steps; then g - shat proj (2), * (1/norm) (2); the clamped rows are one product; accumulate
    adds one more rounded sum."""
    D = np.asarray(dxh).shape[-1]
    g, sh, nrm = np.asarray(dxh, F64), np.asarray(shat, F64), np.asarray(snorm, F64)[..., None]
    d, proj, proj_abs = gram_normalize_bwd(dxh, shat, snorm)
    bproj = (-(-D // 64) + 6 + 1 + 2) * U * proj_abs
    b = np.where(nrm > NORM_CLAMP, (np.abs(sh) * bproj + (4 + 2) * U * (np.abs(g) + np.abs(sh * proj))) / nrm, (1 + 2) * U * np.abs(d))
    if dst is not None:
        b = b + (1 + 2) * U * (np.abs(d) + np.abs(np.asarray(dst, F64)))
        d = d + np.asarray(dst, F64)
    return d, b + TINY


def bound_adamw(p, g, m, v, teacher, step_t, lr, wd, b1, b2, eps, ema, grad_scale, ref):
    """Elementwise bounds of one fused step; ref = adamw_ema(...) of the same arguments.  1 - b1, 1 - b2 and 1 - ema are exact in fp32
    (b in [0.5, 1]).  Longest paths:
      m  = b1 m + (1-b1) gr, gr = g gscale                      4 operations on |b1 m| + |(1-b1) gr|
      v  = b2 v + (1-b2) gr gr   (gr enters twice)              6 operations, all terms positive
      p  = p (1 - lr wd) - lr ibc1 (m / (sqrt(v) isb + eps))     through the denominator: v (6, halved by the sqrt but counted whole),
           sqrt, isb rounded, the product, + eps, the division, lr ibc1 (2: ibc1 rounded), the product, the subtraction: 15; the
           numerator's own error enters as dm / denominator.
      teacher = ema T + (1-ema) p                               3 operations on its two terms, + (1-ema) dp."""
    lr, wd, b1, b2, eps, ema, gs = (f32(a) for a in (lr, wd, b1, b2, eps, ema, grad_scale))
    p, g, m, v = (np.asarray(a, F64) for a in (p, g, m, v))
    pn, mn, vn, tn, _ = ref
    gr = gs * g
    bm = (4 + 2) * U * (np.abs(b1 * m) + np.abs((1 - b1) * gr)) + TINY
    bv = (6 + 2) * U * vn + TINY
    denom = np.sqrt(vn) / math.sqrt(1 - b2 ** step_t) + eps
    k = lr / (1 - b1 ** step_t)
    bp = (15 + 2) * U * (np.abs(p * (1 - lr * wd)) + k * np.abs(mn) / denom) + k * bm / denom + TINY
    out = {"p": bp, "m": bm, "v": bv}
    if teacher is not None:
        out["teacher"] = (1 - ema) * bp + (3 + 2) * U * (np.abs(ema * np.asarray(teacher, F64)) + np.abs((1 - ema) * pn)) + TINY
    return out


def bound_sumsq(n, blocks, per_term, total):
    """Relative bound of a grid-stride sum of n squares over ``blocks`` workgroups of 256 and a second pass over the partials:
    per_term operations inside a term, the thread's trips, the block sum, the partials' block sum."""
    trips = -(-n // (blocks * 256))
    return (per_term + trips + 10 + block_adds(blocks) + 2) * U * total
