"""Float64 NumPy statement of the patch sampler of include/dinox.h (csrc/segpatch.hip), written from the definitions and calling no project
code, an fp32 emulation of the kernel's arithmetic, and the error bounds the tests hold the kernel to.

``sample64`` walks the SOURCE PLANES (the kernel walks output runs): for each plane, every job that reads it, index arithmetic in float64.

Bounds, u = 2^-24, gamma_k = k u / (1 - k u).  Starred values are exact (float64 stands in for them: its own error is 2^-29 of u).
  Coordinates.  The chain is t = fl(a01 dy + a02), s = fl(a00 dx + t), both fmas, and for the image c = fl(s - 0.5): three roundings.
      |s - s*| <= delta_s = u (|t*| + |s*|) (1 + 2^-20),    |c - c*| <= delta_c = delta_s + u |c*| (1 + 2^-20).
  Label.  floor(s) = floor(s*) unless an integer lies within delta_s of s* (the plane's edges 0, W, H are integers): outside that band
      the kernel's label is the oracle's; everywhere it is the fp32 emulation's.
  Image.  f(c_x, c_y), the bilinear interpolant of the plane continued by ``pad``, is continuous and piecewise bilinear; along each axis
      its slope is at most R, the spread (max - min) of the 4 x 4 taps around the exact cell, which holds every cell a point less
      than one pixel away can reach:  |f(c) - f(c*)| <= (delta_cx + delta_cy) R, and never more than the spread G of the whole
      continued plane (delta >= 1/2: G).  The interpolation itself: w1 = c - floor(c) is exact, w0 = fl(1 - w1) one rounding, then per term
      a product, a sum, a product and a sum: each of the four terms passes at most 6 roundings and the weights sum to 1, so
      the interpolation adds gamma_7 M, M = max |tap| over the same 4 x 4 taps.   e_v = coordinate term + gamma_7 M.
  Gamma and gain.  gamma == 1: v' = fl(gain v): e' = |gain| e_v + u |gain v*|.  Otherwise p = powf(max(v, 0), gamma): the power is
      monotone, so the input error moves it by at most e_in = max((v* + e_v)^gamma - p*, p* - max(v* - e_v, 0)^gamma) (float64), powf
      itself by POW_ULP u (p* + e_in), and the product by u: e' = |gain| (e_in + POW_ULP u (p* + e_in)) (1 + u) + u |gain| (p* + e_in).
  Normalisation.  x = fl(fl(v' - mean) / std):  e_x = (e' + 2 u (|v'* - mean| + e')) / std (1 + 2^-20).
POW_ULP is not derivable from this code base and the ROCm documentation installed beside the compiler carries no accuracy table for the
device math functions, so it is MEASURED (tests/test_segpatch_gpu.py::test_pow_error_is_within_twice_the_record) and gated at twice the
recorded value.
"""
import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
POW_ULP_RECORDED = 2.18          # largest |gain powf(v, gamma) - exact| / (u exact) seen on the MI355X over the pow cases
POW_ULP = 2.0 * POW_ULP_RECORDED

DEFECTS = ("label_half", "split_matrix", "pad0", "transpose", "no_half")


def gamma_k(k):
    return k * U / (1 - k * U)


def _centred(S, dtype):
    d = np.arange(S, dtype=dtype) + dtype(0.5) - dtype(S) / dtype(2)
    return d[None, :], d[:, None]                       # dx [1, S], dy [S, 1]


class Result:
    """What ``sample64`` returns for a launch: x [B, 3, S, S] and m [B, S, S] exact, ex the bound on |x_kernel - x|, band [B, S, S] True where
    the label is not decided by the oracle alone, and vprime / evprime, the value before normalisation and its bound."""

    def check(self, x, m, m_emulated=None, cap=0.01):
        """AssertionError unless kernel outputs x, m are what the contract allows.  Returns (largest error / bound, band share)."""
        x, m = np.asarray(x), np.asarray(m)
        assert x.shape == self.x.shape and m.shape == self.m.shape and x.dtype == np.float32 and m.dtype == np.uint8
        assert np.isfinite(x).all(), "non-finite image value"
        err = np.abs(x.astype(np.float64) - self.x)
        ratio = float((err / np.maximum(self.ex, 1e-300)).max())
        assert (err <= self.ex).all(), f"image error {ratio:.3f} x the bound at {np.unravel_index(np.argmax(err - self.ex), err.shape)}"
        if m_emulated is not None:
            assert np.array_equal(m, m_emulated), f"{int((m != m_emulated).sum())} labels differ from the fp32 emulation"
        share = float(self.band.reshape(len(self.band), -1).mean(1).max())
        assert share <= cap, f"{share:.4f} of a job's pixels lie in the undecided band (cap {cap})"
        free = ~self.band
        assert np.array_equal(m[free], self.m[free]), f"{int((m[free] != self.m[free]).sum())} decided labels differ from the oracle"
        return ratio, share


def sample64(planes, plane_of, par, S, mean, std, pad, pow_ulp=POW_ULP):
    """planes: list of (image float32 [H, W], mask uint8 [H, W]); plane_of [B]: the plane each job reads; par float32 [B, 8]."""
    par = np.asarray(par, dtype=np.float32).astype(np.float64)
    mean, std, pad = np.float32(mean).astype(np.float64), np.float32(std).astype(np.float64), float(np.float32(pad))
    B = len(plane_of)
    r = Result()
    r.x, r.ex = np.empty((B, 3, S, S)), np.empty((B, 3, S, S))
    r.m, r.band = np.empty((B, S, S), np.uint8), np.empty((B, S, S), bool)
    r.vprime, r.evprime = np.empty((B, S, S)), np.empty((B, S, S))
    dx, dy = _centred(S, np.float64)
    for k, (img, msk) in enumerate(planes):                                       # the walk over SOURCE planes
        H, W = img.shape
        im = img.astype(np.float64)
        G = max(im.max(), pad) - min(im.min(), pad)
        for b in np.flatnonzero(np.asarray(plane_of) == k):
            a00, a01, a02, a10, a11, a12, gam, gain = par[b]
            tx, ty = a01 * dy + a02, a11 * dy + a12
            sx, sy = a00 * dx + tx, a10 * dx + ty
            dsx, dsy = U * (np.abs(tx) + np.abs(sx)) * SLACK + 2.0 ** -149, U * (np.abs(ty) + np.abs(sy)) * SLACK + 2.0 ** -149
            # label
            inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
            ix, iy = np.clip(np.floor(sx), 0, W - 1).astype(np.int64), np.clip(np.floor(sy), 0, H - 1).astype(np.int64)
            r.m[b] = np.where(inside, msk[iy, ix], 255)
            r.band[b] = (np.abs(sx - np.rint(sx)) <= dsx) | (np.abs(sy - np.rint(sy)) <= dsy)
            # image
            cx, cy = sx - 0.5, sy - 0.5
            dcx, dcy = dsx + U * np.abs(cx) * SLACK, dsy + U * np.abs(cy) * SLACK
            fx, fy = np.floor(np.clip(cx, -3, W + 2)), np.floor(np.clip(cy, -3, H + 2))
            wx, wy = np.clip(cx, -3, W + 2) - fx, np.clip(cy, -3, H + 2) - fy
            x0, y0 = fx.astype(np.int64), fy.astype(np.int64)

            def tap(yy, xx):
                ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                return np.where(ok, im[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], pad)

            v = (1 - wy) * ((1 - wx) * tap(y0, x0) + wx * tap(y0, x0 + 1)) + wy * ((1 - wx) * tap(y0 + 1, x0) + wx * tap(y0 + 1, x0 + 1))
            nb = np.stack([tap(y0 + j, x0 + i) for j in (-1, 0, 1, 2) for i in (-1, 0, 1, 2)])
            R, M = nb.max(0) - nb.min(0), np.abs(nb).max(0)
            move = np.where((dcx < 0.5) & (dcy < 0.5), np.minimum((dcx + dcy) * R, G), G)
            ev = move + gamma_k(7) * M
            if gam == 1.0:
                vp = gain * v
                evp = abs(gain) * ev + U * np.abs(vp)
            else:
                p = np.maximum(v, 0) ** gam
                e_in = np.maximum((np.maximum(v, 0) + ev) ** gam - p, p - np.maximum(v - ev, 0) ** gam)
                vp = gain * p
                evp = abs(gain) * (e_in + pow_ulp * U * (p + e_in)) * (1 + U) + U * abs(gain) * (p + e_in)
            r.vprime[b], r.evprime[b] = vp, evp
            for c in range(3):
                r.x[b, c] = (vp - mean[c]) / std[c]
                r.ex[b, c] = (evp + 2 * U * (np.abs(vp - mean[c]) + evp)) / std[c] * SLACK
    return r


# ------------------------------------------------------------------------------------------ the kernel's arithmetic in NumPy float32
def fma32(a, b, c):
    """fl32(a b + c) for float32 operands: the product is exact in float64, the sum is rounded to float64 and then to float32."""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def coords32(p, S, defect=None):
    """(sx, sy) float32 [S, S] of one job's parameters p float32 [8], in the contract's order of operations."""
    f = np.float32
    dx, dy = _centred(S, np.float32)
    if defect == "no_half":
        dx, dy = dx - f(0.5), dy - f(0.5)
    a00, a01, a02, a10, a11, a12 = (f(v) for v in p[:6])
    if defect == "transpose":
        a01, a10 = a10, a01
    dxx, dyy = np.broadcast_to(dx, (S, S)), np.broadcast_to(dy, (S, S))
    return fma32(a00, dxx, fma32(a01, dyy, a02)), fma32(a10, dxx, fma32(a11, dyy, a12))


def emulate32(planes, plane_of, par, S, mean, std, pad, defect=None):
    """(x float32 [B, 3, S, S], m uint8 [B, S, S]) as the kernel computes them, operation by operation in float32 (the power through
    float64, rounded once).  ``defect``: one of DEFECTS planted on purpose (the tests show that each is caught)."""
    assert defect is None or defect in DEFECTS
    f = np.float32
    par = np.asarray(par, dtype=np.float32)
    mean, std, pad = np.asarray(mean, f), np.asarray(std, f), f(pad)
    B = len(plane_of)
    x, m = np.empty((B, 3, S, S), f), np.empty((B, S, S), np.uint8)
    for b in range(B):
        img, msk = planes[plane_of[b]]
        H, W = img.shape
        sx, sy = coords32(par[b], S, defect if defect in ("transpose", "no_half") else None)
        lx, ly = sx, sy
        if defect == "label_half":
            lx, ly = sx - f(0.5), sy - f(0.5)
        if defect == "split_matrix":                                              # the label under the matrix without its rotation part
            q = par[b].copy()
            q[1] = q[3] = 0
            lx, ly = coords32(q, S)
        with np.errstate(invalid="ignore"):
            inside = (lx >= 0) & (lx < f(W)) & (ly >= 0) & (ly < f(H))
        ix, iy = np.where(inside, np.floor(lx), 0).astype(np.int64), np.where(inside, np.floor(ly), 0).astype(np.int64)
        m[b] = np.where(inside, msk[iy, ix], 0 if defect == "pad0" else 255)
        u, v = sx - f(0.5), sy - f(0.5)
        with np.errstate(invalid="ignore"):
            near = (u > -1) & (u < f(W)) & (v > -1) & (v < f(H))
        us, vs = np.where(near, u, f(0)), np.where(near, v, f(0))
        fu, fv = np.floor(us), np.floor(vs)
        x0, y0 = fu.astype(np.int64), fv.astype(np.int64)
        wx1, wy1 = us - fu, vs - fv
        wx0, wy0 = f(1) - wx1, f(1) - wy1

        def tap(yy, xx):
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            return np.where(ok, img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], pad).astype(f)

        val = wy0 * (wx0 * tap(y0, x0) + wx1 * tap(y0, x0 + 1)) + wy1 * (wx0 * tap(y0 + 1, x0) + wx1 * tap(y0 + 1, x0 + 1))
        val = np.where(near, val, pad).astype(f)
        gam, gain = par[b, 6], par[b, 7]
        if gam != f(1):
            val = (np.maximum(val, f(0)).astype(np.float64) ** float(gam)).astype(f)
        val = gain * val
        for c in range(3):
            x[b, c] = (val - mean[c]) / std[c]
    return x, m
