"""An fp32 NumPy emulation of csrc/views.hip and csrc/encode_prep.hip in their documented order -- tile by tile: tap table, footprint,
staging, horizontal strip, vertical pass, put, the three output layouts -- with one-line defects that can be planted by name
(tests/test_resample_bounds_cpu.py shows which case flags each).  No fused multiply-adds: the bounds of oracle/resample_bounds.py must
hold for this order too."""
import numpy as np

from oracle import resample_bounds as RB

F32 = np.float32
T = 16
NAN = F32(np.nan)
MEAN = np.array([0.485, 0.456, 0.406], dtype=F32)
STD = np.array([0.229, 0.224, 0.225], dtype=F32)

DEFECTS = ("flip_off_by_one", "flip_vertical_too", "taps_clipped_to_image", "sx_sy_swapped", "support_from_other_axis", "no_renormalisation",
           "top_left_swapped", "plane_stride_from_crop", "wden_is_width", "strip_without_fy0", "patch_py_px_swapped",
           "enc_strides_swapped", "enc_channel0_normalisation", "enc_int16_as_uint16", "partial_tile_at_full_origin")


def cubic(x):
    a = F32(-0.5)
    x = np.abs(x).astype(F32)
    near = ((a + F32(2)) * x - (a + F32(3))) * x * x + F32(1)
    far = (((x - F32(5)) * x + F32(8)) * x - F32(4)) * a
    return np.where(x < 1, near, np.where(x < 2, far, F32(0))).astype(F32)


def view_tables(views, defect=None):
    """The per-view tables as dinox.views.make_views builds them."""
    vi, vf = RB.view_tables(views)
    if defect == "wden_is_width":
        vf[:, 1] = [F32(v["width"]) for v in views]
    return vi, vf


def _tile_loop(S):
    nt = (S + T - 1) // T
    return [(ty, tx) for ty in range(nt) for tx in range(nt)]


def _footprint(S, o0, mn, n):
    live = [q for q in range(T) if o0 + q < S]
    bad = any(n[q] < 0 for q in live)
    f0 = min(mn[q] for q in live)
    f1 = max([0] + [mn[q] + n[q] for q in live])
    return bad, f0, f1 - f0


def _pass(src_rows, S, o0, mn, n, w, f0):
    """sum_k w[q][k] * src[:, mn_q - f0 + k] for the 16 columns of a tile, fp32, k in order -> [rows, 16]."""
    out = np.zeros((src_rows.shape[0], T), dtype=F32)
    for q in range(T):
        if o0 + q < S:
            a = np.zeros(src_rows.shape[0], dtype=F32)
            for k in range(n[q]):
                a = a + w[q][k] * src_rows[:, mn[q] - f0 + k]
            out[:, q] = a
    return out


def _origin(o0, S, defect):
    return S - T if defect == "partial_tile_at_full_origin" and o0 + T > S and S >= T else o0


def views_emul(case, layout=0, p=1, ld=0, defect=None, max_crop=None):
    """-> the image batch [V, 3, S, S] (layout 0) or the patch operand [V g g, ld] (1: bf16 values, 2: fp32), NaN where nothing is written
    (padded operand columns: 0, as the memset of the entry point leaves them)."""
    S, raw = case["S"], case["raw"]
    vi, vf = view_tables(case["views"], defect)
    Fp, M, _ = RB.tables("views", S, case["max_crop"] if max_crop is None else max_crop)
    V, g = len(vi), S // p
    if layout == 0:
        out = np.full((V, 3, S, S), NAN, dtype=F32)
    else:
        out = np.full((V * g * g, ld), NAN, dtype=F32)
        out[:, 3 * p * p:] = 0

    def put(v, c, oy, ox, val):
        if layout == 0:
            out[v, c, oy, ox] = val
        else:
            gy, gx = oy // p, ox // p
            py, px = (oy - gy * p, ox - gx * p) if defect != "patch_py_px_swapped" else (ox - gx * p, oy - gy * p)
            out[v * g * g + gy * g + gx, (c * p + py) * p + px] = RB.bf16_round(val) if layout == 1 else val

    for v in range(V):
        off, H, W, top, left, ch, cw, flip = (int(x) for x in vi[v])
        if defect == "top_left_swapped":
            top, left = left, top
        wmin, wden = vf[v]
        sx, sy = F32(cw) / F32(S), F32(ch) / F32(S)
        if defect == "sx_sy_swapped":
            sx, sy = sy, sx
        supx, supy = (F32(2) * sx if sx >= 1 else F32(2)), (F32(2) * sy if sy >= 1 else F32(2))
        invx, invy = (F32(1) / sx if sx >= 1 else F32(1)), (F32(1) / sy if sy >= 1 else F32(1))
        if defect == "support_from_other_axis":
            supx = supy
        for c in range(3):
            plane0 = off + c * (ch * cw if defect == "plane_stride_from_crop" else H * W)
            for ty, tx in _tile_loop(S):
                ox0, oy0 = tx * T, ty * T
                mn, n, w = [[0] * T, [0] * T], [[0] * T, [0] * T], [[None] * T, [None] * T]
                for axis in range(2):
                    for q in range(T):
                        o = (ox0 if axis == 0 else oy0) + q
                        if o >= S:
                            continue
                        fl = flip and (axis == 0 or defect == "flip_vertical_too")
                        i = (S - o if defect == "flip_off_by_one" else S - 1 - o) if fl else o
                        sc, sup, size, inv = (sx, supx, cw, invx) if axis == 0 else (sy, supy, ch, invy)
                        lo_clip, hi_clip = 0, size
                        if defect == "taps_clipped_to_image":
                            lo_clip, hi_clip = (-left, W - left) if axis == 0 else (-top, H - top)
                        center = sc * F32(i + 0.5)
                        xmin = max(int(center - sup + F32(0.5)), lo_clip)
                        xn = min(int(center + sup + F32(0.5)), hi_clip) - xmin
                        if xn > M:
                            xn = -1
                        wk = cubic((np.arange(max(xn, 0), dtype=F32) + F32(xmin) - center + F32(0.5)) * inv)
                        tot = F32(0)
                        for k in range(max(xn, 0)):
                            tot = tot + wk[k]
                        with np.errstate(all="ignore"):
                            w[axis][q] = wk if defect == "no_renormalisation" else (wk / tot).astype(F32)
                        mn[axis][q], n[axis][q] = xmin, xn
                badx, fx0, fw = _footprint(S, ox0, mn[0], n[0])
                bady, fy0, fh = _footprint(S, oy0, mn[1], n[1])
                wx0, wy0 = _origin(ox0, S, defect), _origin(oy0, S, defect)
                if badx or bady or fw > Fp or fh > Fp:
                    for qy in range(T):
                        for qx in range(T):
                            if oy0 + qy < S and ox0 + qx < S:
                                put(v, c, wy0 + qy, wx0 + qx, NAN)
                    continue
                ry, rx = np.arange(fh)[:, None], np.arange(fw)[None, :]
                idx = plane0 + (top + fy0 + ry) * W + (left + fx0 + rx)
                u = raw[np.clip(idx, 0, raw.size - 1)].astype(F32)          # (a defect may index past the buffer: the emulation stays inside)
                hu = (u - F32(32768.0)) * F32(0.1)
                src = np.minimum(np.maximum((hu - wmin) / wden, F32(0)), F32(1)).astype(F32)
                strip = np.full((fh + max(mn[1]) + M + 2, T), NAN, dtype=F32)  # LDS rows past the footprint hold no data of this tile
                strip[:fh] = _pass(src, S, ox0, mn[0], n[0], w[0], fx0)
                res = _pass(strip.T, S, oy0, mn[1], n[1], w[1], 0 if defect == "strip_without_fy0" else fy0)
                for qy in range(T):
                    for qx in range(T):
                        if oy0 + qy < S and ox0 + qx < S:
                            put(v, c, wy0 + qy, wx0 + qx, (res[qx, qy] - MEAN[c]) / STD[c])
    return out


def encode_emul(case, defect=None, max_side=None, prefill=NAN):
    """-> [n_images, 3, S, S]; ``prefill`` where no job writes."""
    S, n_img, fmt = case["S"], case["n_images"], case["fmt"]
    src = case["src"]
    if defect == "enc_int16_as_uint16" and src.dtype == np.int16:
        src = src.view(np.uint16)
    Fp, M, _ = RB.tables("encode", S, case["max_side"] if max_side is None else max_side)
    lo64, hi64 = case["level"] - case["width"] / 2, case["level"] + case["width"] / 2
    lo, hi, den = F32(lo64), F32(hi64), F32(hi64 - lo64)
    out = np.full((3 * n_img, S, S), prefill, dtype=F32)
    for job in case["jobs"]:
        off, H, W, rs, ps, nd = (int(x) for x in job[:6])
        if defect == "enc_strides_swapped":
            rs, ps = ps, rs
        for ty, tx in _tile_loop(S):
            ox0, oy0 = tx * T, ty * T
            mn, n, w = [[0] * T, [0] * T], [[0] * T, [0] * T], [[None] * T, [None] * T]
            for axis in range(2):
                for q in range(T):
                    o, size = (ox0 if axis == 0 else oy0) + q, (W if axis == 0 else H)
                    if o >= S:
                        continue
                    scale = size / S
                    fs = scale if scale > 1.0 else 1.0
                    center = (o + 0.5) * scale
                    xmin = max(int(center - fs + 0.5), 0)
                    xn = min(int(center + fs + 0.5), size) - xmin
                    if xn > M or xn <= 0:
                        xn = -1
                    wk = [max(0.0, 1.0 - abs(((k + xmin) - center + 0.5) / fs)) for k in range(max(xn, 0))]
                    tot = 0.0
                    for x in wk:
                        tot += x
                    w[axis][q] = [F32(x / tot) for x in wk]
                    mn[axis][q], n[axis][q] = xmin, xn
            badx, fx0, fw = _footprint(S, ox0, mn[0], n[0])
            bady, fy0, fh = _footprint(S, oy0, mn[1], n[1])
            bad = nd < 1 or nd > 3 or badx or bady or fw > Fp or fh > Fp
            res = None
            if not bad:
                ry, rx = np.arange(fh)[:, None], np.arange(fw)[None, :]
                idx = off + (fy0 + ry) * rs + (fx0 + rx) * ps
                x = src[np.clip(idx, 0, src.size - 1)].astype(F32)
                if fmt == "hu16_png":
                    x = (x - F32(32768.0)) * F32(0.1)
                if fmt != "windowed_float":
                    with np.errstate(invalid="ignore"):
                        x = np.where(x < lo, lo, np.where(x > hi, hi, x)).astype(F32)
                    x = ((x - lo) / den).astype(F32)
                strip = _pass(x, S, ox0, mn[0], n[0], w[0], fx0)
                res = _pass(strip.T, S, oy0, mn[1], n[1], w[1], fy0)
            wx0, wy0 = _origin(ox0, S, defect), _origin(oy0, S, defect)
            for d in range(3 if bad else nd):
                dst = int(job[6 + d])
                if dst < 0 or dst >= 3 * n_img:
                    continue
                c = 0 if defect == "enc_channel0_normalisation" else dst % 3
                for qy in range(T):
                    for qx in range(T):
                        if oy0 + qy < S and ox0 + qx < S:
                            out[dst, wy0 + qy, wx0 + qx] = NAN if bad else (res[qx, qy] - MEAN[c]) / STD[c]
    return out.reshape(n_img, 3, S, S)
