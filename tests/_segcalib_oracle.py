"""Float64 NumPy statement of the segmentation calibration quantities of include/dinox.h (csrc/segcalib.hip) -- per pixel the confidence,
the normalised entropy, the NLL, Brier, mu - l_y and centred-variance terms at an inverse temperature s, and their five totals -- with
a-priori fp32 bounds in the manner of tests/_segloss_oracle.py, whose geometry, ``Pixels`` (for l and e_l), ``gam`` and ``predict`` it
reuses.  u = 2^-24.  The chain the bounds follow, per pixel (E = the largest e_l over the pixel's classes):

    t_c = s l_c            one multiply:                       e_t   = s e_l (1 + u) + u |t_c|,   E_t = max_c e_t
    d_c = t_c - max t      both operands, one subtraction:      e_d   = (2 E_t + u max|d|)(1 + u)
    exp(d_c)               expf at 2 ulp = 4 u:                 rho_e = expm1(e_d) + 4 u          (relative; absolute floor TINY)
    sum                    C terms:                             rho_s = rho_e + gam(C)
    p_c = exp * (1 / sum)  a division, a product, slack:        rho_p = rho_e + rho_s / (1 - rho_s) + 3 u;  e_p = rho_p p_c + TINY
    lse = log(sum) + max   logf at 2 ulp, the max, one add:     e_lse = rho_s / (1 - rho_s) + 4 u |log sum| + E_t + u |lse|
    a sum of C products x_c y_c:  sum (e_x |y| + |x| e_y + e_x e_y) + gam(C + 1) sum |x y|   (a rounding per product, gam(C) for the sum)

A class whose computed probability is 0 is left out of the kernel's p-weighted sums; its exact term is at most e_p |.|, which the product
bound above already holds.  The totals add n per-pixel terms: gam(n + 8) sum (|x| + e_x) whatever the order.  Fused multiply-adds only
drop roundings.  The entropy is multiplied by fl(1 / fl(log fl(C))) formed on the host (5 u relative with the product's rounding, 7 u
taken); clamping to [0, 1] moves a value no further from an exact value that lies inside.
"""
from __future__ import annotations

import numpy as np

import _segloss_oracle as SO
from _segloss_oracle import TINY, U32, gam

IGNORE = SO.IGNORE
NAMES = ("nll", "brier", "g", "h", "entropy")


def _dot_bound(x, e_x, y, e_y, C):
    """Bound on a C-term sum of products over the last axis."""
    return (e_x * np.abs(y) + np.abs(x) * e_y + e_x * e_y).sum(-1) + gam(C + 1) * np.abs(x * y).sum(-1)


class Calib:
    """Everything at one (z, y, g, u): ``at(s)`` gives the per-pixel quantities, their bounds and the totals at inverse temperature s;
    ``newton(s)`` only the float64 totals (NLL, G, H) that temperature fitting walks on.  y = None: no labels (maps only)."""

    def __init__(self, z, y, g, u):
        z = np.asarray(z, dtype=np.float64)
        B, S = z.shape[0], g * u
        self.C = z.shape[2]
        self.y = np.full((B, S, S), IGNORE, dtype=np.uint8) if y is None else np.asarray(y)
        px = SO.Pixels(z, self.y, g, u)
        self.l, self.e_l, self.valid, self.onehot = px.l, px.e_l, px.valid, px.onehot
        self.pred, self.margin, E = SO.predict(z, g, u)
        self.decided = self.margin > E
        self.nv = int(self.valid.sum())
        self.ly = np.where(self.onehot, self.l, 0.0).sum(-1)
        self.e_ly = np.where(self.onehot, self.e_l, 0.0).sum(-1)

    def newton(self, s: float):
        t = s * self.l
        m = t.max(-1, keepdims=True)
        ex = np.exp(t - m)
        sm = ex.sum(-1, keepdims=True)
        p = ex / sm
        lse = (np.log(sm) + m)[..., 0]
        mu = (p * self.l).sum(-1)
        var = (p * (self.l - mu[..., None]) ** 2).sum(-1)
        v = self.valid
        return float((lse - s * self.ly)[v].sum()), float((mu - self.ly)[v].sum()), float(var[v].sum())

    def at(self, s: float) -> dict:
        s = float(np.float32(s))                                                  # what the kernel is handed
        C, l, e_l = self.C, self.l, self.e_l
        t = s * l
        e_t = s * e_l * (1 + U32) + U32 * np.abs(t)
        E_t = e_t.max(-1)
        m = t.max(-1)
        d = t - m[..., None]
        e_d = (2 * E_t + U32 * np.abs(d).max(-1)) * (1 + U32)
        ex = np.exp(d)
        sm = ex.sum(-1)
        p = ex / sm[..., None]
        rho_e = np.expm1(e_d) + 4 * U32
        rho_s = rho_e + gam(C)
        rho_p = rho_e + rho_s / (1.0 - rho_s) + 3 * U32
        e_p = rho_p[..., None] * p + TINY
        lse = np.log(sm) + m
        e_lse = rho_s / (1.0 - rho_s) + 4 * U32 * np.abs(np.log(sm)) + E_t + U32 * np.abs(lse)
        # confidence: p at the arg-max of the unscaled logits
        conf = np.take_along_axis(p, self.pred[..., None].astype(np.int64), -1)[..., 0]
        e_conf = np.take_along_axis(e_p, self.pred[..., None].astype(np.int64), -1)[..., 0]
        # entropy / log C
        pt = (p * t).sum(-1)
        e_pt = _dot_bound(p, e_p, t, e_t, C)
        raw = lse - pt
        ent = np.clip(raw / np.log(C), 0.0, 1.0)
        e_ent = (e_lse + e_pt + U32 * np.abs(raw)) / np.log(C) * (1 + 7 * U32) + 7 * U32 * np.abs(raw) / np.log(C)
        # the label terms
        v = self.valid
        ty = s * self.ly
        e_ty = s * self.e_ly * (1 + U32) + U32 * np.abs(ty)
        nll = np.where(v, lse - ty, 0.0)
        e_nll = np.where(v, e_lse + e_ty + U32 * np.abs(nll), 0.0)
        dd = p - self.onehot
        e_dd = e_p + U32 * np.abs(dd)
        brier = np.where(v, (dd * dd).sum(-1), 0.0)
        e_brier = np.where(v, (2 * np.abs(dd) * e_dd + e_dd ** 2).sum(-1) + gam(C + 1) * (dd * dd).sum(-1), 0.0)
        mu = (p * l).sum(-1)
        e_mu = _dot_bound(p, e_p, l, e_l, C)
        gp = np.where(v, mu - self.ly, 0.0)
        e_gp = np.where(v, e_mu + self.e_ly + U32 * np.abs(gp), 0.0)
        dl = l - mu[..., None]
        e_dl = e_l + e_mu[..., None] + U32 * np.abs(dl)
        sq = dl * dl
        e_sq = 2 * np.abs(dl) * e_dl + e_dl ** 2 + U32 * sq
        var = np.where(v, (p * sq).sum(-1), 0.0)
        e_var = np.where(v, _dot_bound(p, e_p, sq, e_sq, C) + U32 * (p * sq).sum(-1), 0.0)
        ent_v, e_ent_v = np.where(v, ent, 0.0), np.where(v, e_ent, 0.0)
        per = dict(nll=(nll, e_nll), brier=(brier, e_brier), g=(gp, e_gp), h=(var, e_var), entropy=(ent_v, e_ent_v))
        n = self.nv
        sums = np.array([per[k][0].sum() for k in NAMES])
        e_sums = np.array([per[k][1].sum() + gam(n + 8) * (np.abs(per[k][0]) + per[k][1]).sum() for k in NAMES])
        return dict(s=s, p=p, conf=conf, e_conf=e_conf, entropy=ent, e_entropy=e_ent, per=per, sums=sums, e_sums=e_sums, nv=n)


def root_of_g(cal, lo: float = 1e-3, hi: float = 1e3, tol: float = 1e-12) -> float:
    """s* with G(s*) = 0 over the batches ``cal`` (a list of Calib), by float64 bisection on log s (G is increasing in s)."""
    G = lambda s: sum(c.newton(s)[1] for c in cal)
    a, b = np.log(lo), np.log(hi)
    assert G(np.exp(a)) < 0 < G(np.exp(b)), "the root of G is not inside the bracket"
    while b - a > tol:
        mid = 0.5 * (a + b)
        if G(np.exp(mid)) > 0:
            b = mid
        else:
            a = mid
    return float(np.exp(0.5 * (a + b)))


# ------------------------------------------------------------------------------------------ the histogram, from maps (exact integers)
def histogram(pred, conf, y, C: int, NB: int):
    """(hist int64 [NB, 3], tail int64 [3]) from a prediction map, an fp32 confidence map and labels, by the formulas of include/dinox.h
    in NumPy fp32: k = min((int)(conf * (float)NB), NB - 1), q = (int64)rint(conf * 2^24)."""
    pred, y = np.asarray(pred), np.asarray(y)
    conf = np.asarray(conf, dtype=np.float32)
    valid = (y != IGNORE) & (y < C)
    fin = np.isfinite(conf)
    use = valid & fin
    c = conf[use]
    k = np.minimum((c * np.float32(NB)).astype(np.int64), NB - 1)
    q = np.rint(c * np.float32(16777216.0)).astype(np.int64)
    hit = (pred[use] == y[use]).astype(np.int64)
    hist = np.zeros((NB, 3), dtype=np.int64)
    np.add.at(hist[:, 0], k, 1)
    np.add.at(hist[:, 1], k, hit)
    np.add.at(hist[:, 2], k, q)
    tail = np.array([valid.sum(), ((y != IGNORE) & (y >= C)).sum(), (valid & ~fin).sum()], dtype=np.int64)
    return hist, tail
