"""Float64 NumPy statement of the dense segmentation loss of include/dinox.h (csrc/segloss.hip) -- forward, backward, prediction, counts --
written from the formulas, calling no project code, with a-priori elementwise fp32 bounds.

Bounds, in the manner of tests/_lora_oracle.py (u = 2^-24, gam(n) = n u / (1 - n u)): a sum of n fp32 terms lands within gam(n) sum |terms|
of the exact sum whatever its order, n being the number of pixels that feed it; an input that carries an error passes it on through the
first derivative, taken on the worst side of the interval where a quotient is involved; every further fp32 operation adds u times the
magnitude it produces.  expf / logf are taken at 2 ulp.  Interpolation weights: the kernel forms w1 = r * fl(1 / 2u) (2 roundings) and
w0 = 1 - w1 (one more), so each of the two weights of an axis is off by at most 3 u absolutely and a tap's weight w_y w_x by 6 u (+ 1 u for
the product); the four products and three additions of the interpolation add 4 u relative.
"""
from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24
TINY = 2.0 ** -126                        # below this fp32 results are subnormal or zero: an absolute floor on exp()
IGNORE = 255
EPS = 1.0


def gam(n) -> float:
    return n * U32 / (1.0 - n * U32)


# ------------------------------------------------------------------------------------------ geometry
def taps(g: int, u: int):
    """Along one axis of S = g u pixels: (i0, i1, w1) -- first tap, second tap, weight of the second (align_corners=False)."""
    x = np.arange(g * u, dtype=np.float64)
    s = np.maximum((x + 0.5) / u - 0.5, 0.0)
    i0 = np.floor(s).astype(np.int64)
    i1 = np.minimum(i0 + 1, g - 1)
    return i0, i1, s - i0


def _grid(z, g):
    B, P, C = z.shape
    assert P == g * g
    return z.reshape(B, g, g, C)


def upsample(z: np.ndarray, g: int, u: int) -> np.ndarray:
    """l [B, S, S, C] from z [B, g^2, C]."""
    zg = _grid(np.asarray(z, dtype=np.float64), g)
    i0, i1, w = taps(g, u)
    rows = zg[:, i0] * (1.0 - w)[None, :, None, None] + zg[:, i1] * w[None, :, None, None]              # [B, S, g, C]
    return rows[:, :, i0] * (1.0 - w)[None, None, :, None] + rows[:, :, i1] * w[None, None, :, None]     # [B, S, S, C]


def upsample_abs(z: np.ndarray, g: int, u: int) -> np.ndarray:
    """Sum of |z| over the four tap positions of every pixel (weights left out): what an absolute weight error multiplies."""
    a = _grid(np.abs(np.asarray(z, dtype=np.float64)), g)
    i0, i1, _ = taps(g, u)
    rows = a[:, i0] + a[:, i1]
    return rows[:, :, i0] + rows[:, :, i1]


def adjoint(G: np.ndarray, g: int, u: int, unit_weights: bool = False) -> np.ndarray:
    """[B, g^2, C]: sum_p W(p, j) G_p, the transpose of upsample(); unit_weights puts 1 for every tap weight."""
    S = g * u
    i0, i1, w = taps(g, u)
    w0, w1 = (np.ones(S), np.ones(S)) if unit_weights else (1.0 - w, w)
    Wm = np.zeros((S, g))                                   # Wm[x, j] = weight of patch column j at pixel column x
    np.add.at(Wm, (np.arange(S), i0), w0)
    np.add.at(Wm, (np.arange(S), i1), w1)
    cols = np.einsum("byxc,xj->byjc", G, Wm, optimize=True)
    return np.einsum("byjc,yi->bijc", cols, Wm, optimize=True).reshape(G.shape[0], g * g, G.shape[3])


def footprint(g: int, u: int) -> np.ndarray:
    """[g^2]: the number of pixels a patch is a tap of."""
    i0, i1, _ = taps(g, u)
    n = np.array([np.count_nonzero((i0 == j) | (i1 == j)) for j in range(g)])
    return (n[:, None] * n[None, :]).reshape(-1)


# ------------------------------------------------------------------------------------------ per-pixel quantities, each with its bound
class Pixels:
    """l, p = softmax(l), the cross-entropy term t = lse(l) - l_y and their bounds for a batch (valid: y != 255)."""

    def __init__(self, z, y, g, u):
        z = np.asarray(z, dtype=np.float64)
        self.y = np.asarray(y)
        self.C = z.shape[2]
        assert not ((self.y >= self.C) & (self.y != IGNORE)).any(), "labels >= C other than 255 are an argument error"
        self.valid = self.y != IGNORE
        self.onehot = (self.y[..., None] == np.arange(self.C)) & self.valid[..., None]
        self.l = upsample(z, g, u)
        self.e_l = 11 * U32 * upsample_abs(z, g, u)                                # 7 u absolute on each tap's weight, 4 u relative
        C = self.C
        E = self.e_l.max(-1)                                                      # [B, S, S]
        m = self.l.max(-1)
        d = self.l - m[..., None]
        D = np.abs(d).max(-1)
        e_d = 2 * E + U32 * D                                                     # both operands' errors, one subtraction
        ex = np.exp(d)
        s = ex.sum(-1)
        self.p = ex / s[..., None]
        rho_e = np.expm1(e_d) + 2 * U32                                           # relative error of one exp(l - m)
        rho_s = rho_e + gam(C)                                                    # ... of their sum
        self.rho_p = rho_e + rho_s + 3 * U32                                      # 1 / sum and the product (+ slack for second order)
        self.e_p = self.rho_p[..., None] * self.p + TINY
        ly = np.where(self.onehot, self.l, 0.0).sum(-1)
        self.t = np.where(self.valid, np.log(s) + m - ly, 0.0)
        e_log = rho_s / (1.0 - rho_s) + 2 * U32 * np.log(s)                       # the sum's error through log, logf's own
        self.e_t = np.where(self.valid, e_log + 2 * E + U32 * (np.abs(np.log(s) + m) + np.abs(self.t)), 0.0)


def _quotient_bound(num, e_num, den, e_den):
    """|(num +- e_num) / (den +- e_den) - num / den| on the worst side (num, den > 0, e_den < den) plus the division's rounding."""
    q = num / den
    hi = (num + e_num) / (den - e_den)
    lo = (num - e_num) / (den + e_den)
    return np.maximum(hi - q, q - lo) + U32 * hi


def forward(z, y, g, u, w_ce=1.0, w_dice=1.0, c0=0, px: Pixels | None = None):
    """-> dict: loss[3] = (L, CE, Dice), stats[3, C] = (I, P, Y), nv, and e_loss, e_stats."""
    px = px or Pixels(z, y, g, u)
    C = px.C
    nv = int(px.valid.sum())
    v = px.valid[..., None]
    Yc = px.onehot.sum((0, 1, 2)).astype(np.float64)
    Pc = np.where(v, px.p, 0.0).sum((0, 1, 2))
    Ic = np.where(px.onehot, px.p, 0.0).sum((0, 1, 2))
    e_P = np.where(v, px.e_p, 0.0).sum((0, 1, 2)) + gam(nv + 8) * Pc
    e_I = np.where(px.onehot, px.e_p, 0.0).sum((0, 1, 2)) + gam(Yc + 8) * Ic
    e_Y = np.where(Yc >= 2 ** 24, U32 * Yc, 0.0)
    stats, e_stats = np.stack([Ic, Pc, Yc]), np.stack([e_I, e_P, e_Y])
    if nv == 0:
        return dict(loss=np.zeros(3), e_loss=np.zeros(3), stats=stats, e_stats=e_stats, nv=0)
    ce = px.t.sum() / nv
    e_ce = (px.e_t.sum() + gam(nv + 8) * np.abs(px.t).sum()) / nv + 2 * U32 * abs(ce)
    num, den = 2 * Ic + EPS, Pc + Yc + EPS
    e_num, e_den = 2 * e_I + U32 * num, e_P + e_Y + 2 * U32 * den
    Dc = num / den
    e_D = _quotient_bound(num, e_num, den, e_den)
    n = C - c0
    dice = 1.0 - Dc[c0:].sum() / n
    e_dice = (e_D[c0:].sum() + gam(n + 2) * Dc[c0:].sum()) / n + 2 * U32
    L = w_ce * ce + w_dice * dice
    e_L = abs(w_ce) * e_ce + abs(w_dice) * e_dice + 3 * U32 * (abs(w_ce * ce) + abs(w_dice * dice)) + U32 * abs(L)
    return dict(loss=np.array([L, ce, dice]), e_loss=np.array([e_L, e_ce, e_dice]), stats=stats, e_stats=e_stats, nv=nv)


def backward(z, y, g, u, w_ce=1.0, w_dice=1.0, c0=0, grad_scale=1.0, px: Pixels | None = None, fwd: dict | None = None):
    """-> (dz [B, g^2, C], e_dz): the device takes the statistics of its own forward, so their bounds enter."""
    px = px or Pixels(z, y, g, u)
    fwd = fwd or forward(z, y, g, u, w_ce, w_dice, c0, px)
    C, nv = px.C, fwd["nv"]
    if nv == 0:
        zero = np.zeros((px.l.shape[0], g * g, C))
        return zero, zero
    (Ic, Pc, Yc), (e_I, e_P, e_Y) = fwd["stats"], fwd["e_stats"]
    k = 1.0 / (C - c0)
    num, den = 2 * Ic + EPS, Pc + Yc + EPS
    e_num, e_den = 2 * e_I + U32 * num, e_P + e_Y + 2 * U32 * den
    rel_den = e_den / (den - e_den)
    live = (np.arange(C) >= c0).astype(np.float64)
    al = -w_dice * k * 2.0 / den * live                                           # w_dice a_pc = be_c + [y_p = c] al_c
    be = w_dice * k * num / den ** 2 * live
    e_al = np.abs(al) * (rel_den + 5 * U32)
    e_be = np.abs(be) * (e_num / num + 2 * rel_den + rel_den ** 2 + 7 * U32)
    oh = px.onehot.astype(np.float64)
    a = be + oh * al
    e_a = e_be + oh * e_al + U32 * np.abs(a)
    dot = (px.p * a).sum(-1, keepdims=True)
    e_dot = (px.e_p * np.abs(a) + px.p * e_a).sum(-1, keepdims=True) + gam(C + 1) * (px.p * np.abs(a)).sum(-1, keepdims=True)
    kce = w_ce / nv
    t1 = kce * (px.p - oh)
    e1 = abs(kce) * (px.e_p + U32 * np.abs(px.p - oh)) + 4 * U32 * np.abs(t1)
    ad = a - dot
    e_ad = e_a + e_dot + U32 * np.abs(ad)
    t2 = px.p * ad
    e2 = px.e_p * (np.abs(ad) + e_ad) + px.p * e_ad + U32 * np.abs(t2)
    v = px.valid[..., None]
    G = np.where(v, t1 + t2, 0.0)
    e_G = np.where(v, e1 + e2 + U32 * np.abs(G), 0.0)
    dz = grad_scale * adjoint(G, g, u)
    n = footprint(g, u)[None, :, None]
    e_dz = abs(grad_scale) * (adjoint(e_G, g, u) + 8 * U32 * adjoint(np.abs(G) + e_G, g, u, unit_weights=True)
                              + gam(n + 8) * adjoint(np.abs(G) + e_G, g, u)) + 2 * U32 * np.abs(dz)
    return dz, e_dz


def predict(z, g, u):
    """-> (pred uint8 [B, S, S], margin, e_l): the float64 arg-max (lowest index on a tie), its top-2 margin and the bound on one l_p[c]
    (the largest over the pixel's classes); the tests hold the kernel to the float64 arg-max wherever margin > e_l."""
    px_l = upsample(z, g, u)
    e_l = (11 * U32 * upsample_abs(z, g, u)).max(-1)
    pred = px_l.argmax(-1).astype(np.uint8)
    top2 = np.sort(px_l, -1)[..., -2:]
    return pred, top2[..., 1] - top2[..., 0], e_l


def counts(pred, y, C):
    """int64 [3, C]: true positives, predicted pixels, labelled pixels per class over the valid pixels."""
    pred, y = np.asarray(pred), np.asarray(y)
    valid = y != IGNORE
    out = np.zeros((3, C), dtype=np.int64)
    for c in range(C):
        out[0, c] = np.count_nonzero(valid & (pred == c) & (y == c))
        out[1, c] = np.count_nonzero(valid & (pred == c))
        out[2, c] = np.count_nonzero(valid & (y == c))
    return out
