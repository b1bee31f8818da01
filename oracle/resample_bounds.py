"""The two resampling kernels, csrc/views.hip and csrc/encode_prep.hip, element by element: float64 statements that keep the tap rule
where the parity target has it, a-priori rounding bounds, the host-side table sizing restated, and the deterministic cases of
tests/test_resample_bounds_{cpu,gpu}.py (TEST INFRASTRUCTURE; NumPy only, no torch, no device).

Statements
    views    taps and weights: oracle.slice_views.aa_bicubic_weights (torch's fp32 rule, held to torch's kernel by
             tests/test_slice_views.py::test_restatement_matches_torch_kernel); the windowed source: the fp32 formula of
             oracle.slice_views.hu_window01; the two passes, the flip and (a - mean) / std accumulated in float64.
    encode   taps and weights: PIL's rule in double (pil_bilinear_weights, held to the recorded PIL outputs by
             tests/test_encode_device_cpu.py::test_filter_rule_reproduces_golden); element -> fp32 -> HU -> clip -> window in the fp32
             formula of the reference; both passes and the normalisation in float64.

Bounds.  u = 2^-24, gam(n) = n u / (1 - n u).  Per output element, every term with its operation count:
    window (views)    t = u16 - 32768 is exact; h = t * 0.1f (1), d = h - wmin (1, or both in one fma), e = d / wden (1, correctly rounded):
                      both the statement and the device lie within ERR = u (|h| + 2 |d|) / wden of the exact e, and clip is monotone:
                      dX = max(clip(e + ERR) - x, x - clip(e - ERR)), x the statement's fp32 value.  0 where the window saturates.
    window (encode)   the same operations in the same order on both sides, no product feeds a sum: only the division is given room, 1 op:
                      dX = u |x| (0 for windowed_float, where the source is taken as it is).
    weight (views)    argument a = ((j - c) + .5) inv with c = scale (i + .5): c rounded (1, or fused into the subtraction), the
                      subtraction (1), + .5 (1), times inv (1):  da = inv u (|c| + |j - c| + |j - c + .5|) + u |a|.  The first share,
                      dlt = inv u |c|, is one common shift of all arguments of the index (the device has the statement's c or the
                      exact one): its first order enters a pass as |sum_k D_k x_k| dlt with D the signed derivative of the normalised
                      weights, its second order (5 da^2 + 20 dlt^2) and the other shares per tap.  The Keys cubic in
                      Horner form, with or without fused multiply-adds, bounded from the magnitudes of its intermediates:
                      |x| < 1: m = 1.5 x, s = m - 2.5, p = s x, q = p x, r = q + 1:  u (|m| x^2 + |s| x^2 + |p| x + |q| + |r|)      (5 ops)
                      |x| < 2: t1 = x - 5, t2 = t1 x, t3 = t2 + 8, t4 = t3 x, t5 = t4 - 4, r = -t5 / 2 (exact):
                               u (|t1| x^2 + |t2| x + |t3| x + |t4| + |t5|) / 2                                                       (5 ops)
                      e = (|W'(a)| + 5 da) da + horner(|a| + da)   (|W''| <= 5; W is C1, so the branch taken near 1 and 2 is covered);
                      device against statement: 2 e per raw weight.
    weight (encode)   the device computes PIL's double weight as the statement does and rounds it once: u |w| + 16 * 2^-53.
    renormalisation   tot = sum of n raw weights in any order: dtot = sum 2 e + 2 gam(n) sum |w|;  w^ = w / tot (1 each side):
                      dw^ = 2 e / T + |w| dtot / (|tot| T) + 2 u |w^|,  T = |tot| - dtot.
    pass              sum_k w^_k x_k, n products and n additions in index order, fused or not: gam(n + 1) sum |w^| |x|, plus
                      sum dw^ |x| + sum |w^| dx.
    strip             the horizontal result is stored as fp32: it is the fp32 accumulator itself, no further rounding; one u |strip| is
                      kept as room for a compiler that keeps a wider intermediate.
    final             (a - mean) (1), / std (1): (B_a + u |a - mean|) / std + u |r|.
    knife-edge        the device may fuse scale * (i + .5) into the subtraction that follows, so centre -+ support + .5 can fall on
                      the other side of an integer than in the statement and the device carries one edge tap more or fewer.  For
                      every output index whose expression lies within its own rounding error (3 roundings: u (|c| + |c -+ sup| +
                      |c -+ sup + .5|); encode: the same with 2^-53) of an integer m that moves the range, tap m - 1 is in doubt: with
                      g = (|W(a_{m-1})| + e) / (|tot| - |W| - e) the bound of that tap grows by g and the bound of every other tap of the
                      index by |w^| g (the change of the renormalisation).  Computed for every index, never assumed zero.
Never looser than today: an element whose derived bound exceeds GATE = 1e-5 on the normalised tensor is held at 1e-5 (``capped``).
"""
from __future__ import annotations

import numpy as np

from oracle import slice_views as SV

U = 2.0 ** -24
U64 = 2.0 ** -53
GATE = 1e-5
F32, F64 = np.float32, np.float64
T = 16                                   # output tile side of both kernels
LDS_LIMIT = 150 * 1024
MEAN, STD = SV.MEAN.astype(F64), SV.STD.astype(F64)
FMT = {"hu_float": 0, "hu16_png": 1, "windowed_float": 2}
DT_CODE = {"float32": 0, "uint16": 2, "int16": 3}
CANARY = np.array([0x7A5C3CA5], dtype=np.uint32).view(F32)[0]           # 2.9e35, a value no case produces
SIZING_S = (1, 7, 8, 16, 17, 24, 28, 32, 40, 96, 224)
SIZING_N = range(1, 2400)


def gam(n):
    n = np.asarray(n, F64)
    return n * U / (1.0 - n * U)


# ------------------------------------------------------------------------------------------ table sizing, restated
def tables(kind: str, S: int, max_side: int):
    """(F, MAXT, LDS bytes) as the host code of the two kernels sizes them (kind 'views' | 'encode')."""
    s = max_side / S
    sup = (2.0 if kind == "views" else 1.0) * max(s, 1.0)
    Fp, M = int(T * s + 2.0 * sup) + 4, int(2.0 * sup) + 3
    return Fp, M, (Fp * Fp + Fp * T + 2 * T * M) * 4


def largest_side(kind: str, S: int) -> int:
    """The largest crop / plane side whose tables fit under the 150 KiB limit."""
    n = S
    while tables(kind, S, n + 1)[2] <= LDS_LIMIT:
        n += 1
    return n


def views_tap_ranges(n: int, S: int):
    """(xmin[S], xn[S]) of torch's fp32 rule, vectorised (the ranges of aa_bicubic_weights)."""
    scale = F32(n) / F32(S)
    sup = F32(2.0) * scale if scale >= 1 else F32(2.0)
    c = scale * (np.arange(S, dtype=F32) + F32(0.5))
    x0 = np.maximum((c - sup + F32(0.5)).astype(np.int64), 0)
    x1 = np.minimum((c + sup + F32(0.5)).astype(np.int64), n)
    return x0, x1 - x0


def encode_tap_ranges(n: int, S: int):
    """(xmin[S], xn[S]) of PIL's rule in double, vectorised (the ranges of pil_bilinear_weights)."""
    scale = n / S
    fs = max(scale, 1.0)
    c = (np.arange(S, dtype=F64) + 0.5) * scale
    x0 = np.maximum((c - fs + 0.5).astype(np.int64), 0)
    x1 = np.minimum((c + fs + 0.5).astype(np.int64), n)
    return x0, x1 - x0


def tile_footprints(x0, xn):
    """Per 16-wide tile of output indices: max(x0 + xn) - min(x0)."""
    return np.array([(x0[a:a + T] + xn[a:a + T]).max() - x0[a:a + T].min() for a in range(0, len(x0), T)])


def sizing_margins(kind: str, n: int, S: int):
    """(F - largest footprint, MAXT - largest tap count, smallest tap count) of an n -> S axis with tables sized for n."""
    Fp, M, _ = tables(kind, S, n)
    x0, xn = (views_tap_ranges if kind == "views" else encode_tap_ranges)(n, S)
    return Fp - int(tile_footprints(x0, xn).max()), M - int(xn.max()), int(xn.min())


# ------------------------------------------------------------------------------------------ the tap rules, dense
def pil_bilinear_weights(n: int, S: int):
    """PIL's bilinear coefficients along one axis (the rule of csrc/encode_prep.hip): [(first tap, weights in double)] per output index."""
    scale = n / S
    fs = max(scale, 1.0)
    support = fs
    out = []
    for i in range(S):
        centre = (i + 0.5) * scale
        x0 = max(int(centre - support + 0.5), 0)
        x1 = min(int(centre + support + 0.5), n)
        w = np.array([max(0.0, 1.0 - abs((x - centre + 0.5) / fs)) for x in range(x0, x1)], dtype=np.float64)
        out.append((x0, w / w.sum()))
    return out


def _keys(a):
    """The Keys cubic (a = -0.5), its derivative's magnitude and the Horner rounding bound at |a| (float64, elementwise)."""
    x = np.abs(np.asarray(a, F64))
    near, far = x < 1, (x >= 1) & (x < 2)
    W = np.where(near, (1.5 * x - 2.5) * x * x + 1, np.where(far, (((x - 5) * x + 8) * x - 4) * -0.5, 0.0))
    dW = np.where(near, np.abs(4.5 * x * x - 5 * x), np.where(far, np.abs(-1.5 * x * x + 5 * x - 4), 0.0))
    m, s = 1.5 * x, np.abs(1.5 * x - 2.5)
    p = s * x
    hn = U * (m * x * x + s * x * x + p * x + p * x + np.abs(1 - p * x))
    t1 = np.abs(x - 5)
    t2 = t1 * x
    t3 = np.abs(8 - t2)
    t4 = t3 * x
    hf = 0.5 * U * (t1 * x * x + t2 * x + t3 * x + t4 + np.abs(t4 - 4) + 1e-30)
    return W, dW, np.where(x < 2.5, np.maximum(hn * (x < 1.5), hf), 0.0)


def _knife(expr, err, n: int):
    """Indices of the taps in doubt: expr (float64, exact) within err of an integer m that moves the range -> tap m - 1, else -1."""
    m = np.rint(expr)
    hit = np.abs(expr - m) <= err
    hit &= (m >= 1) & (m <= n)
    return np.where(hit, m - 1, -1).astype(np.int64)


def _axis_finish(Wn, raw, e, sup, tot, doubt, doubt_mag, unit):
    """Dense bound dW [S, n] on the device's normalised weights against the statement's Wn, from the raw weights' errors e."""
    S_, n = Wn.shape
    cnt = sup.sum(1)
    dtot = (2 * e * sup).sum(1) + 2 * gam(cnt) * np.abs(raw * sup).sum(1)
    Tt = np.abs(tot) - dtot
    assert (Tt > 0).all()
    dW = (2 * e / Tt[:, None] + np.abs(raw) * (dtot / (np.abs(tot) * Tt))[:, None] + 2 * unit * np.abs(Wn)) * sup
    knife = np.zeros(S_, bool)
    for side in range(2):
        for i in np.nonzero(doubt[side] >= 0)[0]:
            j, mag = doubt[side][i], doubt_mag[side][i]
            g = mag / (Tt[i] - mag)
            assert g >= 0
            dW[i] += np.abs(Wn[i]) * g
            dW[i, j] += g
            knife[i] = True
    return dW, knife


def views_axis(n: int, S: int):
    """One axis of the antialiased bicubic, n -> S: dict(W [S, n] the statement's normalised weights, dW their bound, sup the statement's
    tap ranges (bool), taps [S], knife [S] indices with a tap in doubt)."""
    tab = SV.aa_bicubic_weights(n, S)
    scale = F32(n) / F32(S)
    sup32 = F32(2.0) * scale if scale >= 1 else F32(2.0)
    inv32 = F32(1.0) / scale if scale >= 1 else F32(1.0)
    sc, sp, inv = float(scale), float(sup32), float(inv32)
    Wn, raw, sup = np.zeros((S, n)), np.zeros((S, n)), np.zeros((S, n), bool)
    for i, (x0, k, w) in enumerate(tab):
        assert k > 0
        Wn[i, x0:x0 + k], sup[i, x0:x0 + k] = w.astype(F64), True
        c32 = scale * F32(i + 0.5)
        raw[i, x0:x0 + k] = SV._cubic((np.arange(k, dtype=F32) + F32(x0) - c32 + F32(0.5)) * inv32).astype(F64)
    c = sc * (np.arange(S) + 0.5)
    j = np.arange(n, dtype=F64)
    jc = j[None, :] - c[:, None]
    a = (jc + 0.5) * inv
    # the rounding of c is ONE shift of every argument of the index (the device has the statement's c or, fused, the exact one): it enters
    # through the signed derivative D of the normalised weights, |sum_k D_k x_k| dlt, not through sum |W'| |x|
    dlt = inv * U * np.abs(c) * (1 + 1e-6)
    da_ind = inv * U * (np.abs(jc) + np.abs(jc + 0.5)) + U * np.abs(a)
    da = da_ind + dlt[:, None]
    W, dW1, _ = _keys(a)
    _, _, horner = _keys(np.abs(a) + da)
    e_full = (dW1 + 5 * da) * da + horner
    e = dW1 * da_ind + 5 * da * da + horner + 20 * dlt[:, None] ** 2      # without the first-order share of the shift; 20 dlt^2: its second order through the division
    x = np.abs(a)
    dWs = np.sign(a) * np.where(x < 1, 4.5 * x * x - 5 * x, np.where(x < 2, -1.5 * x * x + 5 * x - 4, 0.0)) * sup
    t64 = (W * sup).sum(1)[:, None]
    D = (dWs * t64 - W * sup * dWs.sum(1)[:, None]) / (t64 * t64)
    tot = (raw * sup).sum(1)
    doubt, mags = [], []
    for side, sgn in ((0, -1.0), (1, 1.0)):
        expr = c + sgn * sp + 0.5
        err = U * (np.abs(c) + np.abs(c + sgn * sp) + np.abs(expr)) * 1.01
        d = _knife(expr, err, n)
        doubt.append(d)
        rows = np.arange(S)
        mags.append(np.where(d >= 0, np.abs(W[rows, np.maximum(d, 0)]) + e_full[rows, np.maximum(d, 0)], 0.0))
    dW, knife = _axis_finish(Wn, raw, e, sup, tot, doubt, mags, U)
    return dict(W=Wn, dW=dW, sup=sup, taps=sup.sum(1), knife=knife, doubt=np.stack(doubt), D=D, dlt=dlt)


def encode_axis(n: int, S: int):
    """One axis of PIL's bilinear, n -> S, in the same form as views_axis."""
    tab = pil_bilinear_weights(n, S)
    scale = n / S
    fs = max(scale, 1.0)
    Wn, raw, sup = np.zeros((S, n)), np.zeros((S, n)), np.zeros((S, n), bool)
    c = (np.arange(S) + 0.5) * scale
    j = np.arange(n, dtype=F64)
    a = (j[None, :] - c[:, None] + 0.5) / fs
    Wall = np.maximum(0.0, 1.0 - np.abs(a))
    for i, (x0, w) in enumerate(tab):
        assert len(w) > 0
        Wn[i, x0:x0 + len(w)], sup[i, x0:x0 + len(w)] = w, True
    raw = Wall * sup
    tot = raw.sum(1)
    e64 = 8 * U64 * (np.abs(c)[:, None] / fs + 2.0 + 0 * a)                     # a raw double weight: (j - c + .5) / fs and 1 - |.|
    doubt, mags = [], []
    rows = np.arange(S)
    for side, sgn in ((0, -1.0), (1, 1.0)):
        expr = c + sgn * fs + 0.5
        err = 2 * U64 * (np.abs(c) + np.abs(c + sgn * fs) + np.abs(expr))
        d = _knife(expr, err, n)
        doubt.append(d)
        mags.append(np.where(d >= 0, Wall[rows, np.maximum(d, 0)] + e64[rows, np.maximum(d, 0)], 0.0))
    dW, knife = _axis_finish(Wn, raw, e64 * 0.5, sup, tot, doubt, mags, U64)
    dW += (U * np.abs(Wn) + 16 * U64) * sup                             # the one rounding of the double weight to fp32
    return dict(W=Wn, dW=dW, sup=sup, taps=sup.sum(1), knife=knife, doubt=np.stack(doubt), D=np.zeros_like(Wn), dlt=np.zeros(S))


_AXES = {}


def axis(kind: str, n: int, S: int):
    key = (kind, n, S)
    if key not in _AXES:
        _AXES[key] = (views_axis if kind == "views" else encode_axis)(n, S)
    return _AXES[key]


def two_passes(X, dX, ax, ay):
    """The separable resize of X [h, w] (float64; NaN allowed) through the dense axes: (a [S, S], its bound, the NaN mask, the strip's
    relative share).  Horizontal first."""
    nan = np.isnan(X)
    X0 = np.where(nan, 0.0, X)
    aX = np.abs(X0)
    strip = X0 @ ax["W"].T
    astrip = aX @ np.abs(ax["W"]).T
    Bs = aX @ ax["dW"].T + dX @ np.abs(ax["W"]).T + gam(ax["taps"] + 1)[None, :] * astrip + U * np.abs(strip)
    Bs += (np.abs(X0 @ ax["D"].T) + dX @ np.abs(ax["D"]).T) * ax["dlt"][None, :]
    nan_s = (nan.astype(F64) @ ax["sup"].T.astype(F64)) > 0
    a = ay["W"] @ strip
    Ba = ay["dW"] @ np.abs(strip) + np.abs(ay["W"]) @ Bs + gam(ay["taps"] + 1)[:, None] * (np.abs(ay["W"]) @ np.abs(strip))
    Ba += (np.abs(ay["D"] @ strip) + np.abs(ay["D"]) @ Bs) * ay["dlt"][:, None]
    nan_a = (ay["sup"].astype(F64) @ nan_s.astype(F64)) > 0
    return a, Ba, nan_a


def normalise(a, Ba, c: int):
    r = (a - MEAN[c]) / STD[c]
    return r, (Ba + U * np.abs(a - MEAN[c])) / STD[c] * (1 + 2 * U) + U * np.abs(r)


def cap(bound):
    """-> (the bound held at GATE, where that happened)."""
    capped = bound > GATE
    return np.where(capped, GATE, bound), capped


# ------------------------------------------------------------------------------------------ views: statement and bound
def view_tables(views):
    """view_i [V, 8] int64 and view_f [V, 2] fp32 as dinox.views.make_views builds them."""
    vi = np.array([[v["off"], v["H"], v["W"], v["top"], v["left"], v["h"], v["w"], int(v["flip"])] for v in views], dtype=np.int64)
    vf = np.array([[F32(v["level"] - v["width"] / 2.0), F32(max(v["width"], 1.0))] for v in views], dtype=F32)
    return vi, vf


def views_window(u16, level: float, width: float):
    """(x, dx): the statement's fp32 window of a u16 array (as float64) and the window term of the bound."""
    x = SV.hu_window01(u16, level, width).astype(F64)
    wmin, wden = float(F32(level - width / 2.0)), float(F32(max(width, 1.0)))
    h = (u16.astype(F64) - 32768.0) * float(F32(0.1))
    d = h - wmin
    e = d / wden
    err = U * (np.abs(h) + 2 * np.abs(d)) / wden * (1 + 8 * U)
    dx = np.maximum(np.clip(e + err, 0, 1) - x, x - np.clip(e - err, 0, 1))
    assert (dx >= 0).all()
    return x, dx


def views_statement(case):
    """-> dict(ref [V, 3, S, S] float64, bound (held at GATE), capped (bool), raw_bound (before the cap), knife [V, S, S] bool)."""
    S_ = case["S"]
    V = len(case["views"])
    ref, bound, knife = np.zeros((V, 3, S_, S_)), np.zeros((V, 3, S_, S_)), np.zeros((V, S_, S_), bool)
    for v, p in enumerate(case["views"]):
        H, W = p["H"], p["W"]
        stack = case["raw"][p["off"]:p["off"] + 3 * H * W].reshape(3, H, W)
        ax, ay = axis("views", p["w"], S_), axis("views", p["h"], S_)
        knife[v] = ay["knife"][:, None] | ax["knife"][None, :]
        for c in range(3):
            x, dx = views_window(stack[c, p["top"]:p["top"] + p["h"], p["left"]:p["left"] + p["w"]], p["level"], p["width"])
            a, Ba, _ = two_passes(x, dx, ax, ay)
            r, Br = normalise(a, Ba, c)
            if p["flip"]:
                r, Br = r[:, ::-1], Br[:, ::-1]
            ref[v, c], bound[v, c] = r, Br
        if p["flip"]:
            knife[v] = knife[v][:, ::-1]
    held, capped = cap(bound)
    return dict(ref=ref, bound=held, capped=capped, raw_bound=bound, knife=knife)


def unfold(img, p: int, ld: int):
    """[V, 3, S, S] -> the patch-embed operand [V g g, ld], columns c p^2 + py p + px, padded columns 0 (independent NumPy unfold)."""
    V, C, S_, _ = img.shape
    g = S_ // p
    u = np.zeros((V * g * g, ld), dtype=img.dtype)
    u[:, :C * p * p] = img.reshape(V, C, g, p, g, p).transpose(0, 2, 4, 1, 3, 5).reshape(V * g * g, C * p * p)
    return u


def bf16_round(a):
    """fp32 -> the round-to-nearest-even bf16 value, as fp32."""
    b = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    return r.view(F32).reshape(np.shape(a))


# ------------------------------------------------------------------------------------------ encode: statement and bound
def encode_window(plane, fmt: str, lo: float, hi: float):
    """Element -> fp32 -> HU -> clip -> window in the reference's fp32 formula (lo, hi: the doubles level -+ width / 2): (x, dx)."""
    a = plane.astype(F32)
    if fmt == "hu16_png":
        a = (a - F32(32768.0)) * F32(0.1)
    if fmt == "windowed_float":
        return a.astype(F64), np.zeros(a.shape)
    with np.errstate(invalid="ignore"):
        a = (np.clip(a, F32(lo), F32(hi)) - F32(lo)) / F32(hi - lo)
    x = a.astype(F64)
    return x, U * np.abs(np.where(np.isnan(x), 0.0, x))


def job_plane(src, job):
    off, H, W, rs, ps = (int(v) for v in job[:5])
    idx = off + np.arange(H)[:, None] * rs + np.arange(W)[None, :] * ps
    return src[idx]


def encode_statement(case):
    """-> dict(ref [n_images * 3, S, S] float64 (NaN: poisoned, skipped or holding a NaN tap), bound, capped, written (bool per
    destination), knife).  Jobs with nd outside 1..3 poison every slot that names a destination; destinations outside [0, 3 n_images)
    are skipped; a destination no job names keeps what the caller put there (``written`` False)."""
    S_, n_img = case["S"], case["n_images"]
    ref = np.full((3 * n_img, S_, S_), np.nan)
    bound, knife = np.zeros((3 * n_img, S_, S_)), np.zeros((3 * n_img, S_, S_), bool)
    written, poisoned = np.zeros(3 * n_img, bool), np.zeros(3 * n_img, bool)
    lo, hi = case["level"] - case["width"] / 2, case["level"] + case["width"] / 2
    for job in case["jobs"]:
        nd = int(job[5])
        bad = nd < 1 or nd > 3
        dests = [int(d) for d in job[6:6 + (3 if bad else nd)] if 0 <= int(d) < 3 * n_img]
        if bad:
            for d in dests:
                written[d], poisoned[d], ref[d] = True, True, np.nan
            continue
        x, dx = encode_window(job_plane(case["src"], job), case["fmt"], lo, hi)
        ax, ay = axis("encode", int(job[2]), S_), axis("encode", int(job[1]), S_)
        a, Ba, nan_a = two_passes(x, dx, ax, ay)
        for d in dests:
            r, Br = normalise(a, Ba, d % 3)
            ref[d], bound[d], written[d], poisoned[d] = np.where(nan_a, np.nan, r), Br, True, False
            knife[d] = ay["knife"][:, None] | ax["knife"][None, :]
    held, capped = cap(bound)
    return dict(ref=ref.reshape(n_img, 3, S_, S_), bound=held.reshape(n_img, 3, S_, S_), capped=capped.reshape(n_img, 3, S_, S_),
                raw_bound=bound.reshape(n_img, 3, S_, S_), written=written, poisoned=poisoned, knife=knife.reshape(n_img, 3, S_, S_))


def judge(got, st, prefill=None):
    """The largest error / bound of one launch against a statement; asserts that NaN sits exactly where the statement has it (and,
    with ``prefill``, that an unwritten destination keeps the caller's bits).  No element is excluded."""
    got = np.asarray(got)
    ref, bound = st["ref"], st["bound"]
    assert got.shape == ref.shape, (got.shape, ref.shape)
    want_nan = np.isnan(ref)
    if "written" in st:
        w = np.repeat(st["written"], ref.shape[-1] * ref.shape[-2]).reshape(ref.shape)
        if prefill is not None:
            assert np.array_equal(got[~w].view(np.uint32), np.full((~w).sum(), prefill, F32).view(np.uint32)), "an unnamed destination was written"
        want_nan = want_nan & w
        live = w & ~want_nan
        assert np.isnan(got[want_nan]).all(), "an element that must be NaN is not"
    else:
        live = ~want_nan
    assert not np.isnan(got[live]).any(), f"{int(np.isnan(got[live]).sum())} NaN elements where the statement is finite"
    err = np.abs(got.astype(F64)[live] - ref[live])
    b = bound[live]
    assert (err[b == 0] == 0).all(), "an element that must be exact is not"
    return float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0


def flagged(got, st, prefill=None) -> bool:
    """True if judge would fail: some element outside its bound, a NaN out of place, an unwritten element."""
    try:
        return not judge(got, st, prefill) <= 1.0
    except AssertionError:
        return True


# ------------------------------------------------------------------------------------------ cases
VIEW_S = (16, 17, 40)
_rng_cache = {}


def _noise(shape, seed):
    return np.random.default_rng(seed).integers(-1000, 1001, size=shape)


def make_stack(H, W, top, left, h, w, high: bool, seed: int, inside=None):
    """(3, H, W) u16: inside the crop box an asymmetric ramp plus noise in [34000, 40000] (high) or [25000, 31000]; everything outside
    the box is the opposite extreme, 0 or 65535."""
    st = np.full((3, H, W), 0 if high else 65535, dtype=np.int64)
    if inside is None:
        y, x = np.arange(h)[:, None] / max(h - 1, 1), np.arange(w)[None, :] / max(w - 1, 1)
        base = (34000 if high else 25000) + 1000
        inside = np.stack([base + 2500 * y + 1500 * x * x + 300 * c + _noise((h, w), seed * 3 + c) for c in range(3)], 0)
        inside = np.clip(inside, base - 1000, base + 5000)
    st[:, top:top + h, left:left + w] = inside
    return st.astype(np.uint16)


def window_for(high: bool):
    """(level, width) that maps the inside range of make_stack to about [0.1, 0.9] and the outside to the opposite extreme."""
    wmin = 50.0 if high else -850.0
    return wmin + 375.0, 750.0


class ViewsBuilder:
    """Packs the stacks of a launch into one flat u16 buffer at different, non-zero offsets (odd gaps between them)."""

    def __init__(self, S, name, family):
        self.case = dict(kind="views", name=name, family=family, S=S, views=[], max_crop=1)
        self.parts, self.pos, self.k = [], 0, 0

    def add(self, H, W, top, left, h, w, flips=(False, True), level=None, width=None, inside=None, high=None):
        assert 0 <= top and top + h <= H and 0 <= left and left + w <= W and H <= 160 and W <= 176
        for flip in flips:
            hi_ = (self.k % 2 == 0) if high is None else high
            lv, wd = window_for(hi_)
            gap = 7 + 2 * self.k
            self.parts.append(np.full(gap, 0 if hi_ else 65535, np.uint16))
            self.pos += gap
            self.parts.append(make_stack(H, W, top, left, h, w, hi_, 100 + self.k, inside).reshape(-1))
            self.case["views"].append(dict(off=self.pos, H=H, W=W, top=top, left=left, h=h, w=w, flip=flip,
                                           level=lv if level is None else level, width=wd if width is None else width))
            self.pos += 3 * H * W
            self.case["max_crop"] = max(self.case["max_crop"], h, w)
            self.k += 1
        return self

    def done(self, **extra):
        self.case["raw"] = np.concatenate(self.parts + [np.zeros(5, np.uint16)])
        self.case.update(extra)
        return self.case


def knife_sides(S):
    """Crop extents at which centre -+ support + .5 is an integer for several output indices (S = 16: only the exact scales 1 and 3;
    S = 17: odd extents, at i = 6 and 10, in fp32 inexact; S = 40: multiples of 8, at every fifth index, in fp32 inexact)."""
    return {16: (16, 48), 17: (19, 35, 53), 40: (24, 56, 88, 120)}[S]


def _views_case(family, S):
    b = ViewsBuilder(S, f"{family}-{S}", family)
    if family == "full":
        b.add(37, 53, 0, 0, 37, 53).add(64, 48, 0, 0, 64, 48)
    elif family == "corners":
        for top, left in ((0, 0), (0, 32), (28, 0), (28, 32), (13, 17)):
            b.add(48, 56, top, left, 20, 24)
    elif family == "slivers":
        b.add(33, 47, 5, 7, 1, 1).add(33, 47, 9, 0, 1, 47).add(33, 47, 0, 11, 33, 1).add(33, 47, 31, 45, 2, 2)
    elif family == "aspect":
        h, w = 4 * S, S // 2
        b.add(h, w + 17, 0, 13, h, w).add(w + 11, h + 9, 7, 9, w, h)
    elif family == "scales":
        ks = (1, 2, 3, 1.5, 2.5) if S % 2 == 0 else (1, 2, 3)
        for k in ks:
            n = int(k * S)
            b.add(n + 5, n + 9, 3, 5, n, n, flips=(False,)).add(S + 3 + 5, n + 9, 3, 5, S + 3, n, flips=(True,))
            b.add(n + 5, S - 3 + 9, 3, 5, n, S - 3, flips=(False,))
    elif family == "knife":
        sides = knife_sides(S)
        for i, n in enumerate(sides):
            m = sides[(i + 1) % len(sides)]
            b.add(m + 5, n + 9, 2, 4, m, n)
    elif family == "window":
        H, W, top, left, h, w = 40, 44, 3, 5, 30, 33
        steps = 32768 + 30 + _noise((3, h, w), 7) % 7 - 3                   # 2.7 .. 3.3 HU in steps of 0.1
        b.add(H, W, top, left, h, w, level=3.0, width=0.5, inside=steps, high=False)          # wden = max(0.5, 1) = 1
        b.add(H, W, top, left, h, w, level=5500.0, width=1000.0)           # saturates every pixel to 0
        b.add(H, W, top, left, h, w, level=-4500.0, width=1000.0)          # ... and to 1
        ext = 32768 + 20 * _noise((3, h, w), 9)
        ext[:, ::3, ::4], ext[:, 1::5, 2::3] = 0, 65535
        b.add(H, W, top, left, h, w, level=-0.05, width=6553.5, inside=ext)                    # stored 0 and 65535 inside the crop
    elif family == "mixed":
        big = (100, 90) if S < 40 else (160, 176)
        b.add(9, 11, 3, 4, 2, 2).add(big[0], big[1], 0, 0, big[0], big[1]).add(9, 11, 5, 2, 2, 2, flips=(True,))
    elif family == "lds64":                                                # > 64 KiB of dynamic LDS: the launch goes through reserve_lds
        b.add(107, 113, 4, 6, 100, 93)
    elif family == "ldsmax":                                               # the largest crop under the 150 KiB limit
        n = largest_side("views", S)
        assert n <= 160
        b.add(160, 176, 160 - n, 9, n, n - 5, flips=(True,)).add(20, n + 3, 2, 1, 11, n, flips=(False,))
    else:
        raise KeyError(family)
    return b.done()


VIEW_FAMILIES = ("full", "corners", "slivers", "aspect", "scales", "knife", "window", "mixed")
VIEW_LDS = (("lds64", 16), ("ldsmax", 16))
VIEW_CASES = tuple(f"{f}-{S}" for f in VIEW_FAMILIES for S in VIEW_S) + tuple(f"{f}-{S}" for f, S in VIEW_LDS)
PATCH_CASES = ((40, 8, "corners-40"), (16, 16, "slivers-16"), (28, 14, "patch-28"))      # (S, p, the views case whose draws it takes)

_CASES, _STATEMENTS = {}, {}


def views_case(name):
    if name not in _CASES:
        family, S = name.rsplit("-", 1)
        if family == "patch":                                              # S = 28, p = 14: tiles straddle patches
            b = ViewsBuilder(int(S), name, family)
            b.add(48, 56, 28, 32, 20, 24).add(70, 61, 3, 5, 63, 50).add(33, 47, 9, 0, 1, 47, flips=(True,))
            _CASES[name] = b.done()
        elif family == "under":                                            # understated max_crop (C ABI only): 100 stated as 80
            b = ViewsBuilder(int(S), name, family)
            b.add(105, 109, 3, 5, 100, 100).add(50, 60, 3, 5, 44, 47, flips=(False,))
            _CASES[name] = b.done(max_crop=80)
        else:
            _CASES[name] = _views_case(family, int(S))
    return _CASES[name]


def statement(case):
    """The float64 statement of a case, computed once and shared (never modified by a caller)."""
    key = (case["kind"], case["name"])
    if key not in _STATEMENTS:
        _STATEMENTS[key] = (views_statement if case["kind"] == "views" else encode_statement)(case)
    return _STATEMENTS[key]


ENC_S = (16, 17, 40)
ENC_DTYPES = ("float32", "uint16", "int16")
ENC_FORMATS = ("hu_float", "hu16_png", "windowed_float")
ENC_N_IMAGES = 5


def _values(shape, dtype, fmt, seed):
    """Source values for a (dtype, format) pair: inside and on both sides of the window 40 / 400 (hu16: of its stored image);
    u16 above 32767, i16 with negatives; windowed_float in [0, 1] for fp32 and raw integers for the integer types."""
    rng = np.random.default_rng(seed)
    if dtype == "float32":
        if fmt == "windowed_float":
            return rng.random(shape, dtype=F32)
        if fmt == "hu16_png":
            return (32768 + rng.integers(-3000, 4000, size=shape)).astype(F32)
        return (rng.standard_normal(shape) * 200 + 40).astype(F32)
    if fmt == "windowed_float":                                            # integer sources taken as they are: 0 and 1
        return rng.integers(0, 2, size=shape).astype(dtype)
    if dtype == "uint16":
        if fmt == "hu16_png":
            return (32768 + rng.integers(-3000, 4000, size=shape)).astype(np.uint16)
        return np.where(rng.random(shape) < 0.5, rng.integers(0, 400, size=shape), rng.integers(32768, 65536, size=shape)).astype(np.uint16)
    if fmt == "hu16_png":                                                  # an int16 image of stored values: -340 .. -260 HU below the offset
        return rng.integers(-2000, 8000, size=shape).astype(np.int16)
    return rng.integers(-300, 400, size=shape).astype(np.int16)


class EncodeBuilder:
    def __init__(self, S, name, family, dtype, fmt, n_images=ENC_N_IMAGES, level=40.0, width=400.0):
        self.case = dict(kind="encode", name=name, family=family, S=S, dtype=dtype, fmt=fmt, n_images=n_images, level=level, width=width,
                         max_side=1)
        self.parts, self.pos, self.jobs = [], 0, []

    def block(self, shape):
        """A block of source values at a fresh, non-zero offset; -> (offset, array)."""
        gap = 5 + 2 * len(self.parts)
        k = len(self.parts)
        self.parts.append(_values((gap,), self.case["dtype"], self.case["fmt"], 900 + k))
        self.pos += gap
        a = _values(shape, self.case["dtype"], self.case["fmt"], 500 + k + 31 * self.case["S"])
        self.parts.append(a.reshape(-1))
        off, self.pos = self.pos, self.pos + a.size
        return off, a

    def job(self, off, H, W, rs, ps, dests, nd=None):
        assert H <= 160 and W <= 176 or H <= 176 and W <= 160
        d = list(dests) + [-1] * (3 - len(dests))
        self.jobs.append([off, H, W, rs, ps, len(dests) if nd is None else nd] + d[:3])
        self.case["max_side"] = max(self.case["max_side"], H, W)
        return self

    def plane(self, H, W, dests, nd=None):
        off, _ = self.block((H, W))
        return self.job(off, H, W, W, 1, dests, nd)

    def done(self, **extra):
        self.case["src"] = np.concatenate(self.parts + [_values((7,), self.case["dtype"], self.case["fmt"], 3)])
        self.case["jobs"] = np.array(self.jobs, dtype=np.int64)
        self.case.update(extra)
        return self.case


def _encode_case(family, S, dtype, fmt):
    name = f"{family}-{S}-{dtype}-{fmt}"
    lw = dict(level=-3000.0, width=800.0) if (dtype, fmt) == ("int16", "hu16_png") else {}      # the window over that image
    b = EncodeBuilder(S, name, family, dtype, fmt, **lw)
    if family == "planes":
        # 15 destinations, every one named once, in another order than the planes
        b.plane(1, 1, [4]).plane(1, 23, [7, 2]).plane(19, 1, [11, 0, 9]).plane(29, 45, [1])
        big = min(5 * S + 7, 160)                                          # >= 5x down (S = 16, 17; 4x at S = 40: no source above 160 x 176)
        b.plane(big, S - 5, [6, 8, 10])
        off, _ = b.block((40, 66))                                         # a strided view [::2, ::3]
        b.job(off, 20, 22, 2 * 66, 3, [3])
        off, _ = b.block((21, 26, 3))                                      # interleaved (H, W, 3)
        for c, d in enumerate((14, 12, 13)):
            b.job(off + c, 21, 26, 3 * 26, 3, [d])
        b.plane(S, S, [5])                                                 # identity
    elif family == "skipped":
        b.plane(23, 31, [-5, 1]).plane(18, 27, [2, 3 * ENC_N_IMAGES, 0]).plane(9, 12, [2 ** 40, 7, -1], nd=3)
    elif family == "badnd":
        b.plane(23, 31, [0, 1], nd=0).plane(18, 27, [2, 3, 4], nd=4).plane(9, 12, [5]).plane(9, 12, [9, -1, 10], nd=-1)
    elif family == "nan":
        off, a = b.block((33, 41))
        a[13, 17] = np.nan
        a[0, 40] = np.nan
        b.parts[-1] = a.reshape(-1)
        b.job(off, 33, 41, 41, 1, [0, 4, 8])
    elif family == "lds64":
        b.plane(24, 110, [0]).plane(110, 20, [1, 2])
    elif family == "ldsmax":
        n = largest_side("encode", S)
        assert n <= 176
        b.plane(21, n, [2, 0]).plane(5, 7, [1])
    else:
        raise KeyError(family)
    return b.done()


ENC_CASES = tuple(f"planes-{S}-{d}-{f}" for S in ENC_S for d in ENC_DTYPES for f in ENC_FORMATS) + \
    ("skipped-17-int16-hu_float", "badnd-17-uint16-hu16_png", "nan-17-float32-windowed_float", "nan-40-float32-hu_float",
     "lds64-16-float32-hu_float", "ldsmax-16-uint16-hu16_png")


def encode_case(name):
    if name not in _CASES:
        family, S, dtype, fmt = name.split("-")
        if family == "under":                                              # understated max_side (C ABI only): 100 stated as 80
            b = EncodeBuilder(int(S), name, family, dtype, fmt, n_images=1)
            b.plane(100, 100, [0, 1]).plane(30, 44, [2])
            _CASES[name] = b.done(max_side=80)
        else:
            _CASES[name] = _encode_case(family, int(S), dtype, fmt)
    return _CASES[name]


def tile_facts(kind, case_axes_x, case_axes_y, S, Fp, M):
    """Per tile (ty, tx) of an S x S output: (must be NaN, must not be NaN) from the statement's tap ranges -- a tile whose footprint
    exceeds F, or whose tap count exceeds MAXT, by 2 or more is refused; one that stays 2 under both is computed (a tap in doubt
    moves either by at most 1 a side)."""
    nt = (S + T - 1) // T
    must, mustnt = np.zeros((nt, nt), bool), np.zeros((nt, nt), bool)

    def facts(ax, t):
        sup = ax["sup"][t * T:(t + 1) * T]
        cols = np.nonzero(sup.any(0))[0]
        return cols.max() + 1 - cols.min(), sup.sum(1).max()
    for ty in range(nt):
        for tx in range(nt):
            (fw, nx), (fh, ny) = facts(case_axes_x, tx), facts(case_axes_y, ty)
            must[ty, tx] = max(fw, fh) >= Fp + 2 or max(nx, ny) >= M + 2
            mustnt[ty, tx] = max(fw, fh) <= Fp - 2 and max(nx, ny) <= M - 2
    return must, mustnt


def judge_understated(got, st, must, mustnt, prefill_nan=True):
    """A launch whose tables were sized for less than it holds: every element NaN or within its bound, NaN in whole tiles, the tiles
    that must be refused are NaN, those that fit with room are not.  got, st: one [S, S] plane.  -> error / bound over the computed tiles."""
    S = got.shape[-1]
    ratio = 0.0
    for ty in range(must.shape[0]):
        for tx in range(must.shape[1]):
            sl = (slice(ty * T, min(ty * T + T, S)), slice(tx * T, min(tx * T + T, S)))
            g = got[sl]
            n = np.isnan(g)
            assert n.all() or not n.any(), f"tile {(ty, tx)}: NaN in part of a tile"
            assert not (must[ty, tx] and not n.all()), f"tile {(ty, tx)} exceeds the tables and was computed"
            assert not (mustnt[ty, tx] and n.any()), f"tile {(ty, tx)} fits the tables and was refused"
            if not n.any():
                err, b = np.abs(g.astype(F64) - st["ref"][sl]), st["bound"][sl]
                assert (err <= b).all(), f"tile {(ty, tx)}: error / bound {float((err / b).max()):.3f}"
                ratio = max(ratio, float((err / np.maximum(b, 1e-300)).max()))
    return ratio
