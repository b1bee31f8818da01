"""Float64 NumPy statement of the sliding-window blend of include/dinox.h (csrc/segblend.hip), written from the formulas and calling no
project code, with a-priori fp32 bounds; beside it an fp32 emulation of the kernel's arithmetic (for the CPU self-tests and for measuring
how many pixels the margin rule exempts) that can carry planted defects.

The statement walks the TILES and adds each tile's upsampled, window-weighted logits into whole-image float64 accumulators -- the scatter
the kernel avoids -- so it shares neither the kernel's traversal (a gather per pixel) nor its covering-range search.

Bounds (u = 2^-24, gam(n) = n u / (1 - n u), as tests/_segloss_oracle.py).  A pixel is covered by n = F * (covering tiles) visits j; visit
j contributes w_j l_j with w_j = win[ly] win[lx] and l_j the 4-tap interpolation of the tile's patch logits.  Write A_j for the sum of |z|
over the visit's four taps (weights left out), M = sum_j w_j A_j, D = sum_j w_j, L = (sum_j w_j l_j) / D.
  * interpolation: each axis weight is r * fl(1 / 2t) (two roundings) or one minus that (one more): off by at most 3 u absolutely, a tap's
    weight w_y w_x by 6 u (+ u for the product); the four products and three additions add 4 u relative: |l^_j - l_j| <= 11 u A_j, the bound
    tests/_segloss_oracle.py derives for the same four taps;
  * the window weight w_j is one fp32 product of exact inputs (u relative) and w_j l_j one more product (u): with |l_j| <= A_j the term
    w_j l_j is off by at most (11 + 2) u w_j A_j, taken as 14 u for the second-order terms;
  * the numerator is a sum of n such terms, each itself a sum over four taps: an accumulation of length 4 n in the worst association,
    gam(4 n) sum_j w_j A_j; a fused multiply-add only removes roundings;
  * the denominator: n positive terms, each u off, summed: gam(n + 1) relative;
  * one division: u relative.
Together, with |L| <= M / D:   e_L = (14 u + gam(4 n) + gam(n + 1) + u) / (1 - gam(n + 1)) * M / D.
conf = 1 / sum_c exp(L_c - L_b), b the device's own arg-max (the value does not depend on which class is subtracted): the exponent's
argument is off by e_d = 2 E + u (R + 2 E), E = max_c e_L, R = max_c L_c - min_c L_c (both operands' errors, one subtraction of a
difference no larger than R + 2 E); expf is taken at 2 ulp as the other oracles take it; the C-term sum adds gam(C), the reciprocal u:
  rho = expm1(e_d) + 2 u + gam(C) + u,   e_conf = rho / (1 - rho) * conf + C 2^-126   (the floor: exponentials that underflow).
pred is compared where the float64 top-2 margin exceeds 2 E; elsewhere either of the classes within 2 E of the maximum may win.
"""
from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24
TINY = 2.0 ** -126
IGNORE = 255
DEFECTS = ("dropped_mirror", "no_half_pixel", "conf_without_division", "second_tap_unclamped", "last_tile_skipped")


def gam(n):
    return n * U32 / (1.0 - n * U32)


def axis_taps(t: int, g: int, mirror: bool):
    """Per tile-local coordinate l = 0 .. t - 1: (lm, k0, k1, w1) -- the mirrored coordinate, the two taps, the weight of the second."""
    l = np.arange(t, dtype=np.int64)
    lm = t - 1 - l if mirror else l
    s = np.maximum((lm + 0.5) * g / t - 0.5, 0.0)
    k0 = np.floor(s).astype(np.int64)
    k1 = np.minimum(k0 + 1, g - 1)
    return lm, k0, k1, s - k0


class Blend:
    """L [B, H, W, C], its bound e_L, conf and e_conf [B, H, W], the float64 arg-max and the top-2 margin, for
    z [B, F, ny, nx, g^2, C], origins ys / xs, flip codes, the fp32 window and tiles of side t on an H x W image."""

    def __init__(self, z, ys, xs, flips, win, H, W, t):
        z = np.asarray(z, dtype=np.float64)
        B, F, ny, nx, P, C = z.shape
        g = int(round(P ** 0.5))
        assert g * g == P and len(ys) == ny and len(xs) == nx and len(flips) == F and len(win) == t
        w64 = np.asarray(win, dtype=np.float32).astype(np.float64)
        N = np.zeros((B, H, W, C))
        M = np.zeros((B, H, W, C))
        D = np.zeros((H, W))
        n = np.zeros((H, W), dtype=np.int64)
        for f, code in enumerate(flips):
            lmy, ky0, ky1, wy = axis_taps(t, g, bool(code & 2))
            lmx, kx0, kx1, wx = axis_taps(t, g, bool(code & 1))
            Wt = np.outer(w64[lmy], w64[lmx])                                       # [t, t]
            for iy, y0 in enumerate(ys):
                for ix, x0 in enumerate(xs):
                    zt = z[:, f, iy, ix].reshape(B, g, g, C)
                    rows = zt[:, ky0] * (1.0 - wy)[None, :, None, None] + zt[:, ky1] * wy[None, :, None, None]
                    full = rows[:, :, kx0] * (1.0 - wx)[None, None, :, None] + rows[:, :, kx1] * wx[None, None, :, None]
                    a = np.abs(zt)
                    ar = a[:, ky0] + a[:, ky1]
                    A = ar[:, :, kx0] + ar[:, :, kx1]
                    sl = (slice(None), slice(y0, y0 + t), slice(x0, x0 + t))
                    N[sl] += Wt[None, :, :, None] * full
                    M[sl] += Wt[None, :, :, None] * A
                    D[y0:y0 + t, x0:x0 + t] += Wt
                    n[y0:y0 + t, x0:x0 + t] += 1
        assert (n >= 1).all(), "the tiles do not cover the image"
        self.C, self.n = C, n
        self.L = N / D[None, :, :, None]
        k = (14 * U32 + gam(4 * n) + gam(n + 1) + U32) / (1.0 - gam(n + 1))         # [H, W]
        self.e_L = k[None, :, :, None] * M / D[None, :, :, None]
        self.E = self.e_L.max(-1)
        top = np.sort(self.L, axis=-1)
        self.margin = top[..., -1] - top[..., -2]
        self.pred = self.L.argmax(-1)                                               # (the first maximum: the lowest index)
        self.decided = self.margin > 2 * self.E
        R = top[..., -1] - top[..., 0]
        with np.errstate(over="ignore"):
            self.conf = 1.0 / np.exp(self.L - top[..., -1:]).sum(-1)
            e_d = 2 * self.E + U32 * (R + 2 * self.E)
            rho = np.expm1(e_d) + 2 * U32 + gam(C) + U32
        self.e_conf = np.where(rho < 1.0, rho / np.where(rho < 1.0, 1.0 - rho, 1.0), np.inf) * self.conf + C * TINY

    def check(self, pred, conf=None, cap: float = 1e-3):
        """Asserts the comparison the tests make; returns (share of pixels the margin rule exempts, largest conf error / bound)."""
        pred = np.asarray(pred)
        assert pred.shape == self.pred.shape and pred.dtype == np.uint8
        assert (pred < self.C).all()
        wrong = self.decided & (pred != self.pred)
        assert not wrong.any(), f"{int(wrong.sum())} decided pixel(s) differ from the float64 arg-max, first at {tuple(np.argwhere(wrong)[0])}"
        # an undecided pixel may take any class within 2 E of the maximum, nothing else
        got = np.take_along_axis(self.L, pred[..., None].astype(np.int64), -1)[..., 0]
        far = ~self.decided & (self.L.max(-1) - got > 2 * self.E)
        assert not far.any(), f"{int(far.sum())} undecided pixel(s) took a class further than 2 E from the maximum"
        share = 1.0 - float(self.decided.mean())
        assert share <= cap, f"the margin rule exempts {share:.2e} of the pixels (cap {cap:.0e})"
        worst = 0.0
        if conf is not None:
            conf = np.asarray(conf, dtype=np.float64)
            assert conf.shape == self.conf.shape
            err = np.abs(conf - self.conf)
            bad = ~(err <= self.e_conf)
            assert not bad.any(), (f"conf outside its bound at {int(bad.sum())} pixel(s), first {tuple(np.argwhere(bad)[0])}: "
                                   f"error {err[bad].max():.3e} vs bound {self.e_conf[bad].min():.3e}")
            worst = float((err / self.e_conf).max())
        return share, worst


def confusion_counts(pred, labels, C):
    """int64 [3, C]: true positives, predicted and labelled pixels per class over the pixels whose label is not 255."""
    pred, labels = np.asarray(pred), np.asarray(labels)
    v = labels != IGNORE
    out = np.zeros((3, C), dtype=np.int64)
    for c in range(C):
        out[0, c] = np.count_nonzero(v & (pred == c) & (labels == c))
        out[1, c] = np.count_nonzero(v & (pred == c))
        out[2, c] = np.count_nonzero(v & (labels == c))
    return out


# ------------------------------------------------------------------------------------------ fp32 emulation of the kernel's arithmetic
def _taps32(t, g, mirror, defect):
    f32 = np.float32
    l = np.arange(t, dtype=np.int64)
    lm = t - 1 - l if (mirror and defect != "dropped_mirror") else l
    num = (2 * lm + 1) * g - t if defect != "no_half_pixel" else 2 * lm * g       # the defect: s = l g / t, no half-pixel shift
    k0 = np.where(num > 0, num // (2 * t), 0)
    inv2t = f32(1.0) / f32(2 * t)
    if defect == "second_tap_unclamped":
        k1 = (k0 + 1) % g                                                           # (reads the neighbouring row instead of faulting)
        w1 = np.where(num > 0, (num - 2 * t * k0).astype(f32) * inv2t, f32(0))
    else:
        k1 = np.minimum(k0 + 1, g - 1)
        w1 = np.where((k0 + 1 < g) & (num > 0), (num - 2 * t * k0).astype(f32) * inv2t, f32(0))
    return lm, k0, k1, w1.astype(f32)


def emulate(z, ys, xs, flips, win, H, W, t, defect=None):
    """(pred uint8 [B, H, W], conf fp32 [B, H, W]) in fp32 NumPy, the sums in the kernel's order (variant, tile row, tile column), every
    product and sum rounded (no fused multiply-add).  ``defect``: one of DEFECTS, planted."""
    assert defect is None or defect in DEFECTS
    f32 = np.float32
    z = np.asarray(z, dtype=f32)
    B, F, ny, nx, P, C = z.shape
    g = int(round(P ** 0.5))
    win = np.asarray(win, dtype=f32)
    N = np.zeros((B, H, W, C), dtype=f32)
    D = np.zeros((H, W), dtype=f32)
    for f, code in enumerate(flips):
        lmy, ky0, ky1, wy1 = _taps32(t, g, bool(code & 2), defect)
        lmx, kx0, kx1, wx1 = _taps32(t, g, bool(code & 1), defect)
        wy0, wx0 = f32(1) - wy1, f32(1) - wx1
        Wt = (win[lmy][:, None] * win[lmx][None, :]).astype(f32)
        for iy, y0 in enumerate(ys):
            for ix, x0 in enumerate(xs):
                zt = z[:, f, iy, ix].reshape(B, g, g, C)
                top, bot = zt[:, ky0], zt[:, ky1]                                   # [B, t, g, C]
                a0 = top[:, :, kx0] * wx0[None, None, :, None] + top[:, :, kx1] * wx1[None, None, :, None]
                a1 = bot[:, :, kx0] * wx0[None, None, :, None] + bot[:, :, kx1] * wx1[None, None, :, None]
                lj = a0 * wy0[None, :, None, None] + a1 * wy1[None, :, None, None]
                mask = np.ones((t, t), dtype=bool)
                if defect == "last_tile_skipped" and ix == nx - 1:
                    mask[:] = False                                                 # the covering range stops one tile column short
                sl = (slice(None), slice(y0, y0 + t), slice(x0, x0 + t))
                N[sl] = np.where(mask[None, :, :, None], N[sl] + Wt[None, :, :, None] * lj, N[sl])
                D[y0:y0 + t, x0:x0 + t] = np.where(mask, D[y0:y0 + t, x0:x0 + t] + Wt, D[y0:y0 + t, x0:x0 + t])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        L = (N / D[None, :, :, None]).astype(f32)
        pred = np.zeros((B, H, W), dtype=np.int64)
        bv = L[..., 0].copy()
        for c in range(1, C):
            better = L[..., c] > bv
            pred = np.where(better, c, pred)
            bv = np.where(better, L[..., c], bv)
        src = N if defect == "conf_without_division" else L
        bs = np.take_along_axis(src, pred[..., None], -1)
        s = np.zeros((B, H, W), dtype=f32)
        for c in range(C):
            s = s + np.exp((src[..., c:c + 1] - bs)[..., 0].astype(f32)).astype(f32)
        conf = (f32(1) / s).astype(f32)
    return pred.astype(np.uint8), conf


# ------------------------------------------------------------------------------------------ inputs
def make_logits(kind: str, shape, seed: int) -> np.ndarray:
    """fp32 tile logits [B, F, ny, nx, P, C]: "randn", "randn30" (times 30) or "offset" (randn, class 1 moved up by 1e4)."""
    z = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    if kind == "randn30":
        z = (z * np.float32(30)).astype(np.float32)
    elif kind == "offset":
        z[..., 1] += np.float32(1e4)
    else:
        assert kind == "randn"
    return z


def mirrored_variants(z0: np.ndarray, flips) -> np.ndarray:
    """[B, F, ny, nx, P, C] from variant 0's logits [B, ny, nx, P, C]: variant f is what a model that commutes with mirroring would
    give on the mirrored tile -- the patch grid flipped along x (bit 0) and / or y (bit 1)."""
    B, ny, nx, P, C = z0.shape
    g = int(round(P ** 0.5))
    zg = z0.reshape(B, ny, nx, g, g, C)
    out = []
    for code in flips:
        v = zg
        if code & 1:
            v = v[:, :, :, :, ::-1]
        if code & 2:
            v = v[:, :, :, ::-1]
        out.append(v.reshape(B, ny, nx, P, C))
    return np.ascontiguousarray(np.stack(out, 1))
