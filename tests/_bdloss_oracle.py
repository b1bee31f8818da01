"""Float64 NumPy statement of the boundary loss of include/dinox.h (csrc/distmap.hip and the boundary term of csrc/segloss.hip), written
from the definitions, calling no project code.

Signed distance map: brute force over all pixel pairs.  The spacing is taken as the fp32 values the kernel sees; everything after that is
float64, so the result is the exact distance up to 2^-52.  The kernel's bound is 3 u relative (u = 2^-24): fl(s k)^2, fl(s m)^2 are each
within (1 + u)^3 of exact, their rounded sum within (1 + u)^4, the correctly rounded root of that within (1 + u)^2 (1 + u) -- 3 u to first
order, the second-order terms far below the 2^-52 of this oracle's own arithmetic relative to u.

Boundary term: the per-pixel quantities and their bounds come from tests/_segloss_oracle.py (Pixels: p and e_p); what is added here
follows the same rules (gam(n) sum |terms| for a sum of n fp32 terms in any order, first-derivative propagation, u per further operation).
The magnitudes the boundary sum accumulates are |phi| p.  phi is an INPUT of the loss kernels (fp32, handed to this oracle as the very
values the kernel reads), so it carries no error of its own here.
"""
from __future__ import annotations

import numpy as np

import _segloss_oracle as SO

U32 = SO.U32
IGNORE = SO.IGNORE
DIST_REL = 3 * U32                        # the derived bound of the distance kernels, relative


# ------------------------------------------------------------------------------------------ signed distance map
def signed_distance(y, spacing, C: int) -> np.ndarray:
    """phi float64 [B, C, H, W] of labels y uint8 [B, H, W] (255 = ignore), spacing [B, 2] = (s_y, s_x)."""
    y = np.asarray(y)
    B, H, W = y.shape
    sp = np.asarray(spacing, dtype=np.float32).astype(np.float64).reshape(B, 2)
    assert not ((y >= C) & (y != IGNORE)).any(), "labels >= C other than 255 are an argument error"
    yy, xx = np.divmod(np.arange(H * W), W)
    phi = np.zeros((B, C, H * W))
    for b in range(B):
        lab = y[b].reshape(-1).astype(np.int64)
        valid = lab != IGNORE
        for i0 in range(0, H * W, 512):                       # a block of query pixels against every pixel
            q = slice(i0, min(i0 + 512, H * W))
            d = np.sqrt((sp[b, 0] * (yy[q, None] - yy[None, :])) ** 2 + (sp[b, 1] * (xx[q, None] - xx[None, :])) ** 2)
            for c in range(C):
                G, R = lab == c, valid & (lab != c)
                if not G.any() or not R.any():
                    continue                                # the set some pixel needs is empty: the whole plane is 0
                to_g = d[:, G].min(1)
                to_r = d[:, R].min(1)
                phi[b, c, q] = np.where(R[q], to_g, np.where(G[q], -to_r, 0.0))
    return phi.reshape(B, C, H, W)


def scipy_signed_distance(y, spacing, C: int, ndi) -> np.ndarray:
    """The scipy.ndimage expression of the header, for maps without ignored pixels whose classes are each present and not all-covering."""
    y = np.asarray(y)
    sp = np.asarray(spacing, dtype=np.float32).astype(np.float64)
    out = np.zeros((y.shape[0], C) + y.shape[1:])
    for b in range(y.shape[0]):
        for c in range(C):
            G = y[b] == c
            if G.all() or not G.any():
                continue
            out[b, c] = ndi.distance_transform_edt(~G, sampling=sp[b]) * ~G - ndi.distance_transform_edt(G, sampling=sp[b]) * G
    return out


# ------------------------------------------------------------------------------------------ loss: forward
def forward(z, y, phi, g, u, w_ce=1.0, w_dice=1.0, w_bd=1.0, c0=0, px: SO.Pixels | None = None):
    """-> dict as _segloss_oracle.forward, loss[4] = (L, CE, Dice, BD) and e_loss[4]."""
    px = px or SO.Pixels(z, y, g, u)
    base = SO.forward(z, y, g, u, w_ce, w_dice, c0, px)
    C, nv = px.C, base["nv"]
    if nv == 0:
        return dict(base, loss=np.zeros(4), e_loss=np.zeros(4))
    ph = np.moveaxis(np.asarray(phi, dtype=np.float64), 1, -1)                     # [B, S, S, C]
    live = (np.arange(C) >= c0) & px.valid[..., None]
    n = C - c0
    mag = np.where(live, px.p * np.abs(ph), 0.0).sum()                            # what the sum accumulates
    s = np.where(live, px.p * ph, 0.0).sum()
    e_s = np.where(live, px.e_p * np.abs(ph), 0.0).sum() + SO.gam(nv * n + 8) * mag
    bd = s / (nv * n)
    e_bd = e_s / (nv * n) + 3 * U32 * abs(bd)                                     # (float) Nv, its product with C - c0, the division
    L0, ce, dice = base["loss"]
    e_L0, e_ce, e_dice = base["e_loss"]
    L = L0 + w_bd * bd
    e_L = e_L0 + abs(w_bd) * e_bd + U32 * (abs(w_bd * bd) + abs(L))
    return dict(base, loss=np.array([L, ce, dice, bd]), e_loss=np.array([e_L, e_ce, e_dice, e_bd]))


# ------------------------------------------------------------------------------------------ loss: backward
def backward(z, y, phi, g, u, w_ce=1.0, w_dice=1.0, w_bd=1.0, c0=0, grad_scale=1.0, px: SO.Pixels | None = None, fwd: dict | None = None):
    """-> (dz [B, g^2, C], e_dz).  _segloss_oracle.backward with the boundary term p (t - sum p t), t = kbd phi, kbd = w_bd / (Nv (C - c0)),
    added to G: the same steps and bounds as the Dice term's p (a - sum p a)."""
    px = px or SO.Pixels(z, y, g, u)
    fwd = fwd or forward(z, y, phi, g, u, w_ce, w_dice, w_bd, c0, px)
    C, nv = px.C, fwd["nv"]
    if nv == 0:
        zero = np.zeros((px.l.shape[0], g * g, C))
        return zero, zero
    (Ic, Pc, Yc), (e_I, e_P, e_Y) = fwd["stats"], fwd["e_stats"]
    k = 1.0 / (C - c0)
    num, den = 2 * Ic + SO.EPS, Pc + Yc + SO.EPS
    e_num, e_den = 2 * e_I + U32 * num, e_P + e_Y + 2 * U32 * den
    rel_den = e_den / (den - e_den)
    live = (np.arange(C) >= c0).astype(np.float64)
    al = -w_dice * k * 2.0 / den * live
    be = w_dice * k * num / den ** 2 * live
    e_al = np.abs(al) * (rel_den + 5 * U32)
    e_be = np.abs(be) * (e_num / num + 2 * rel_den + rel_den ** 2 + 7 * U32)
    oh = px.onehot.astype(np.float64)
    a = be + oh * al
    e_a = e_be + oh * e_al + U32 * np.abs(a)
    dot = (px.p * a).sum(-1, keepdims=True)
    e_dot = (px.e_p * np.abs(a) + px.p * e_a).sum(-1, keepdims=True) + SO.gam(C + 1) * (px.p * np.abs(a)).sum(-1, keepdims=True)
    kce = w_ce / nv
    t1 = kce * (px.p - oh)
    e1 = abs(kce) * (px.e_p + U32 * np.abs(px.p - oh)) + 4 * U32 * np.abs(t1)
    ad = a - dot
    e_ad = e_a + e_dot + U32 * np.abs(ad)
    t2 = px.p * ad
    e2 = px.e_p * (np.abs(ad) + e_ad) + px.p * e_ad + U32 * np.abs(t2)
    # the boundary term, of the same shape with t = kbd phi in the place of a
    kbd = w_bd / (nv * (C - c0))
    t = kbd * np.moveaxis(np.asarray(phi, dtype=np.float64), 1, -1) * live        # [B, S, S, C]
    e_t = 4 * U32 * np.abs(t)                                                     # kbd: three roundings; its product with phi
    dotb = (px.p * t).sum(-1, keepdims=True)
    e_dotb = (px.e_p * np.abs(t) + px.p * e_t).sum(-1, keepdims=True) + SO.gam(C + 1) * (px.p * np.abs(t)).sum(-1, keepdims=True)
    adb = t - dotb
    e_adb = e_t + e_dotb + U32 * np.abs(adb)
    t3 = px.p * adb
    e3 = px.e_p * (np.abs(adb) + e_adb) + px.p * e_adb + U32 * np.abs(t3)
    v = px.valid[..., None]
    G = np.where(v, t1 + t2 + t3, 0.0)
    e_G = np.where(v, e1 + e2 + e3 + U32 * (np.abs(t1 + t2) + np.abs(G)), 0.0)
    dz = grad_scale * SO.adjoint(G, g, u)
    n = SO.footprint(g, u)[None, :, None]
    e_dz = abs(grad_scale) * (SO.adjoint(e_G, g, u) + 8 * U32 * SO.adjoint(np.abs(G) + e_G, g, u, unit_weights=True)
                              + SO.gam(n + 8) * SO.adjoint(np.abs(G) + e_G, g, u)) + 2 * U32 * np.abs(dz)
    return dz, e_dz
