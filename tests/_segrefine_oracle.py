"""Float64 NumPy statement of the edge-aware refinement of include/dinox.h (csrc/segrefine.hip), computed literally from the definition
(padded arrays and shifted slices, not the kernel's tiles), with an a-priori bound per pixel on the fp32 kernel's error in the pre-softmax
values V = U + w m and in the probabilities Q.  Geometry, ``upsample`` and the interpolation bound e_l are tests/_segloss_oracle.py's;
the softmax rounding chain is tests/_segcalib_oracle.py's.  u = 2^-24, gam(n) = n u / (1 - n u).

The recursion, per pixel p and class c (E = the largest bound over the pixel's classes):

    U = s l                one multiply:                         e_U = s e_l (1 + u) + u |U|
    weights                the guide is exact fp32.  t = (I_p - I_j)^2 k with k = fl(1 / (2 sigma_I^2)) carries at most 6 u relative (the
                           subtraction, the square, k, the product), expf 4 u, and t e^-t <= 1 / e: exp(-t) is off by less than 7 u
                           absolutely; 1 - lambda, lambda exp and their sum add 3 u (a <= 1): |da| <= 10 u.  g is rounded once and
                           multiplied once: the kernel's weight of neighbour j is g_j (a_j + da)(1 + 2 u), off by at most g_j EW, EW = 13 u.
    m = sum_j g_j a_j Q_j / sum_j g_j   (n <= 48 neighbours, fused multiply-adds, one division).  With G = sum_j g_j:
                           e_m = (EW sum_j g_j Q_j / G + sum_j g_j (a_j + EW) e_Q_j / G)(1 + rr) + rr m,   rr = 2 gam(50) + 4 u
                           -- a sub-convex combination (a <= 1): the neighbours' errors are averaged, never amplified
                           (|dm| <= max_j |dQ_j| + rounding), and the roundings of the numerator, the normaliser and the division are
                           relative to a sum of non-negative terms.
    V = U + w m            a product and a sum (or one fma):     e_V = (e_U + w e_m + u |w m| + u |V|)(1 + 2 u)
    Q = softmax(V)         perturbing every V_k by at most E' = E_V + u max_k |V_k - max V| (the subtraction of the maximum) moves
                           Q_c by at most Q_c (1 - Q_c) expm1(2 E'): the worst case is +E' on c and -E' on every other class, where
                           Q'_c - Q_c = Q_c (1 - Q_c)(1 - e^(-2E')) / (Q_c + (1 - Q_c) e^(-2E')) and the denominator is >= e^(-2E').
                           The roundings of the evaluation (expf 4 u, the sum of C terms, 1 / sum, the product) are relative:
                           rho = 8 u + (4 u + gam(C)) / (1 - 4 u - gam(C)).
                           e_Q = Q (1 - Q) expm1(2 E') + rho Q + TINY
    Q^0 = softmax(U) is the same step with e_V = e_U; iteration t takes e_Q of iteration t - 1.

A pixel is DECIDED when the top-two gap of the final V exceeds twice the pixel's E_V (at T = 0 the arg-max is taken on the unscaled l:
the gap of l against twice e_l); the kernel must give the float64 arg-max there, and conf within e_Q[pred].
"""
from __future__ import annotations

import numpy as np

import _segloss_oracle as SO
from _segloss_oracle import TINY, U32, gam

EW = 13 * U32
RR = 2 * gam(50) + 4 * U32


def table(r: int, d: int, sigma_xy: float) -> np.ndarray:
    """g_(dy,dx) in float64, [2r+1, 2r+1]."""
    o = np.arange(-r, r + 1, dtype=np.float64)
    return np.exp(-(o[:, None] ** 2 + o[None, :] ** 2) * float(d) ** 2 / (2.0 * float(sigma_xy) ** 2))


def _softmax(V, e_V, C):
    """-> (Q, e_Q) over the last axis by the step of the docstring."""
    E = e_V.max(-1)
    mx = V.max(-1, keepdims=True)
    dd = V - mx
    Ep = E + U32 * np.abs(dd).max(-1)
    ex = np.exp(dd)
    sm = ex.sum(-1, keepdims=True)
    Q = ex / sm
    one_minus = (sm - ex) / sm
    rho = 8 * U32 + (4 * U32 + gam(C)) / (1.0 - 4 * U32 - gam(C))
    return Q, Q * one_minus * np.expm1(2 * Ep)[..., None] + rho * Q + TINY


def _shift(A, r, d, dy, dx, S):
    """A [B, S + 2rd, S + 2rd, ...] padded -> the [B, S, S, ...] view at neighbour (dy, dx)."""
    H = r * d
    return A[:, H + dy * d:H + dy * d + S, H + dx * d:H + dx * d + S]


def refine(z, guide, g, u, *, s=1.0, T=5, r=2, d=2, sigma_xy=3.0, sigma_i=0.5, lam=0.8, w=4.0):
    """-> dict(pred uint8 [B, S, S], conf, e_conf, V [B, S, S, C], e_V (the pixel's E_V), gap, decided, Q, e_Q).  The scalars are
    taken at the fp32 values the kernel is handed (s, lambda, w); sigma_xy and sigma_i stay exact, their roundings are in the bounds."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return _refine(z, guide, g, u, float(np.float32(s)), int(T), int(r), int(d), float(sigma_xy), float(sigma_i), float(np.float32(lam)),
                       float(np.float32(w)))


def _refine(z, guide, g, u, s, T, r, d, sigma_xy, sigma_i, lam, w):
    z = np.asarray(z, dtype=np.float64)
    I = np.asarray(guide, dtype=np.float64)
    B, S, C = z.shape[0], g * u, z.shape[2]
    assert I.shape == (B, S, S) and r * d < S and 2 * d <= S          # (2 d > S: the pixels in the middle have no neighbour; refused)
    l = SO.upsample(z, g, u)
    e_l = 11 * U32 * SO.upsample_abs(z, g, u)
    U = s * l
    e_U = s * e_l * (1 + U32) + U32 * np.abs(U)
    if T == 0:                                            # the arg-max of the unscaled logits, the softmax of U
        Q, e_Q = _softmax(U, e_U, C)
        V, e_V = l, e_l
    else:
        Q, e_Q = _softmax(U, e_U, C)
        H = r * d
        gt = table(r, d, sigma_xy)
        pad2 = ((0, 0), (H, H), (H, H))
        inside = np.pad(np.ones((B, S, S)), pad2)
        Ip = np.pad(I, pad2)
        offs = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if (dy, dx) != (0, 0)]
        # per neighbour: the weight g a (0 outside the image) and the normaliser
        A, AE, G = {}, {}, np.zeros((B, S, S))
        for dy, dx in offs:
            ins = _shift(inside, r, d, dy, dx, S)
            a = (1.0 - lam) + lam * np.exp(-(I - _shift(Ip, r, d, dy, dx, S)) ** 2 / (2.0 * sigma_i ** 2))
            gj = gt[dy + r, dx + r]
            A[dy, dx] = np.where(ins > 0, gj * a, 0.0)[..., None]
            AE[dy, dx] = np.where(ins > 0, gj * (a + EW), 0.0)[..., None]
            G += ins * gj
        pad3 = pad2 + ((0, 0),)
        for _ in range(T):
            Qp, eQp = np.pad(Q, pad3), np.pad(e_Q, pad3)          # zeros outside: with the zero weights there, neither sum sees them
            num, plain, err = np.zeros_like(Q), np.zeros_like(Q), np.zeros_like(Q)
            for dy, dx in offs:
                Qj = _shift(Qp, r, d, dy, dx, S)
                num += A[dy, dx] * Qj
                plain += gt[dy + r, dx + r] * Qj
                err += AE[dy, dx] * _shift(eQp, r, d, dy, dx, S)
            m = num / G[..., None]
            e_m = (EW * plain + err) / G[..., None] * (1 + RR) + RR * np.abs(m)
            V = U + w * m
            e_V = (e_U + w * e_m + U32 * np.abs(w * m) + U32 * np.abs(V)) * (1 + 2 * U32)
            Q, e_Q = _softmax(V, e_V, C)
    E = e_V.max(-1)
    Vs = np.where(np.isnan(V), -np.inf, V)
    pred = Vs.argmax(-1).astype(np.uint8)
    top2 = np.sort(Vs, -1)[..., -2:]
    gap = top2[..., 1] - top2[..., 0]
    finite = np.isfinite(V).all(-1) & np.isfinite(E) & np.isfinite(Q).all(-1)
    decided = finite & (gap > 2 * E)
    idx = pred[..., None].astype(np.int64)
    return dict(pred=pred, conf=np.take_along_axis(Q, idx, -1)[..., 0], e_conf=np.take_along_axis(e_Q, idx, -1)[..., 0], V=V, e_V=E, gap=gap,
                decided=decided, finite=finite, Q=Q, e_Q=e_Q)


def dice(pred, truth, c=1) -> float:
    a, b = np.asarray(pred) == c, np.asarray(truth) == c
    return 2.0 * (a & b).sum() / max(a.sum() + b.sum(), 1)


def disc_case(n=64, gp=8, seed=0):
    """The synthetic case of the feature's motivation: a noisy disc on an n x n image, patch logits from each patch's foreground fraction.
    -> (z fp32 [1, gp^2, 2], guide fp32 [1, n, n], truth uint8 [n, n], u)."""
    u = n // gp
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n]
    truth = ((yy - 0.47 * n) ** 2 + (xx - 0.53 * n) ** 2 <= (0.3 * n) ** 2).astype(np.uint8)
    guide = (truth + 0.1 * rng.standard_normal((n, n))).astype(np.float32)
    frac = truth.reshape(gp, u, gp, u).mean((1, 3)).reshape(-1)
    f = np.clip(frac, 0.02, 0.98)
    z = np.stack([np.zeros_like(f), np.log(f / (1 - f))], -1).astype(np.float32)[None]
    return z, guide[None], truth, u
