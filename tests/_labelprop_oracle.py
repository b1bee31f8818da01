"""float64 NumPy restatement of dense label propagation (csrc/labelprop.hip, dinox/propagate.py): the window mask, the selection by
``np.lexsort((index, -score))``, the vote, ``patch_soft_labels`` and the schedule -- and the derived bound of the vote.

The bound of ``out``  (seg in [0, 1]; on the kernel's OWN returned (idx, val), so the selection is not part of it)
----------------------------------------------------------------------------------------------------------------
Let s_1 >= ... >= s_n be the returned fp32 scores of the n filled slots of a row, t = inv_temperature (the fp32 value the kernel gets),
a_i = (s_i - s_1) t <= 0, w_i = exp(a_i), W = sum w_i, R = sum_i w_i seg_i / W the exact vote, u = 2^-24.

1. Argument.  The kernel forms (s_i - s_1) t in double (error 2^-52 |a_i|, dropped against u) and rounds it to fp32 once:
   a^_i = a_i (1 + d), |d| <= u, so exp(a^_i) = w_i exp(a_i d) and |exp(a_i d) - 1| <= expm1(|a_i| u).  For unit rows |s_i - s_1| <= 2
   and |a_i| <= 2 t.
2. Exponential.  The kernel calls expf, documented (HIP math API, single precision) to at most 1 ulp: a relative error of at most
   2^-23, and an absolute floor of 2^-126 where the result falls below the normal range.  So the weight it holds is
   w^_i = w_i + D_i,   |D_i| <= w_i (exp(|a_i| u) (1 + 2^-23) - 1) + 2^-126  =: e_i,   and e_1 = 0: a_1 = 0 exactly and expf(0) = 1.
3. The vote with the weights w^_i, exactly: R^ = sum w^_i seg_i / W^.  Since sum_i w_i (seg_i - R) = 0,
   R^ - R = sum_i D_i (seg_i - R) / W^,  |seg_i - R| <= 1,  W^ >= w^_1 = 1:      |R^ - R| <= sum_{i >= 2} e_i.
   (x exp(-x) <= 1 / e: a far neighbour's large |a_i| costs nothing, its weight is gone.)
4. Sums and division.  The numerator is one fp32 fma chain over i ascending: a term sees at most n roundings.  The denominator is a
   compensated fp32 sum over i ascending (the rounding error of every addition, exact by TwoSum, is added back once): one rounding and a
   second-order term of at most n^2 u^2.  One division.  All terms are >= 0, so the computed value is R^ (1 + theta) with
   |theta| <= gamma_{n+2} + n^2 u^2,  gamma_m = m u / (1 - m u), and R^ <= 1.
Together:   |out - R| <= sum_{i >= 2} e_i + gamma_{n+2} + n^2 u^2                                        (vote_bound, per row)
and for unit rows, uniformly:   (K - 1) (expm1(2 t u) (1 + 2^-23) + 2^-23 + 2^-126) + gamma_{K+2} + K^2 u^2     (vote_bound_unit).
Nothing in either expression is fitted to the kernel's output.
"""
import math

import numpy as np

U = 2.0 ** -24
EXP_REL = 2.0 ** -23          # expf: 1 ulp
EXP_FLOOR = 2.0 ** -126


def effective_radius(g, radius):
    return g if (radius < 0 or radius >= g - 1) else radius


def window_mask(g, F, radius):
    """bool [N, F N]: key j = f N + y' g + x' is a candidate of patch p = y g + x."""
    R = effective_radius(g, radius)
    y, x = np.divmod(np.arange(g * g), g)
    near = (np.abs(y[:, None] - y[None, :]) <= R) & (np.abs(x[:, None] - x[None, :]) <= R)
    return np.tile(near, (1, F))


def scores64(q, k):
    return np.asarray(q, np.float64) @ np.asarray(k, np.float64).T


def select(S, mask, K):
    """(idx int32 [N, K], val float64 [N, K]): the first K candidates in the order (score descending, index ascending); NaN scores never
    enter; empty slots are (-1, -inf)."""
    N, Nk = S.shape
    idx = np.full((N, K), -1, np.int32)
    val = np.full((N, K), -np.inf)
    ar = np.arange(Nk)
    for p in range(N):
        ok = mask[p] & ~np.isnan(S[p])
        cand = ar[ok]
        order = cand[np.lexsort((cand, -S[p, cand]))][:K]
        idx[p, :len(order)] = order
        val[p, :len(order)] = S[p, order]
    return idx, val


def vote(idx, val, seg, inv_t):
    """float64 [N, C]: the vote over the filled slots of (idx, val); a row with none is zero."""
    seg = np.asarray(seg, np.float64)
    idx = np.asarray(idx)
    val = np.asarray(val, np.float64)
    out = np.zeros((idx.shape[0], seg.shape[1]))
    for p in range(idx.shape[0]):
        n = int((idx[p] >= 0).sum())
        if n == 0:
            continue
        w = np.exp((val[p, :n] - val[p, 0]) * float(inv_t))
        out[p] = (w[:, None] * seg[idx[p, :n]]).sum(0) / w.sum()
    return out


def propagate_step(q, k, seg, g, K, radius, inv_t):
    """(out, idx, val) in float64 from the operands alone."""
    F = k.shape[0] // (g * g)
    idx, val = select(scores64(q, k), window_mask(g, F, radius), K)
    return vote(idx, val, seg, inv_t), idx, val


def gamma(m):
    return m * U / (1.0 - m * U)


def vote_bound(idx, val, inv_t):
    """float64 [N]: the bound of |out - vote(idx, val, seg, inv_t)| per row for seg in [0, 1] (module docstring)."""
    idx = np.asarray(idx)
    val = np.asarray(val, np.float64)
    filled = idx >= 0
    n = filled.sum(1)
    with np.errstate(invalid="ignore"):
        a = np.where(filled, np.abs(val - val[:, :1]) * float(inv_t), 0.0)
    w = np.where(filled, np.exp(-a), 0.0)
    e = np.where(filled, w * (np.exp(a * U) * (1.0 + EXP_REL) - 1.0) + EXP_FLOOR, 0.0)
    e[:, 0] = 0.0
    return e.sum(1) + gamma(n + 2) + (n * U) ** 2


def vote_bound_unit(inv_t, K):
    """The uniform bound for unit rows (|a_i| <= 2 inv_t, w_i <= 1)."""
    return (K - 1) * (math.expm1(2.0 * float(inv_t) * U) * (1.0 + EXP_REL) + EXP_REL + EXP_FLOOR) + gamma(K + 2) + (K * U) ** 2


def patch_soft_labels(label_map, C, patch):
    """float64 [N, C]: per patch the share of its non-ignored (!= 255) pixels in each class; an all-ignored patch is a zero row."""
    lab = np.asarray(label_map)
    S = lab.shape[0]
    g = S // patch
    if ((lab != 255) & (lab >= C)).any():
        raise ValueError("class index out of range")
    out = np.zeros((g * g, C))
    for y in range(g):
        for x in range(g):
            cell = lab[y * patch:(y + 1) * patch, x * patch:(x + 1) * patch].ravel()
            cell = cell[cell != 255]
            if len(cell):
                out[y * g + x] = np.bincount(cell, minlength=C)[:C] / len(cell)
    return out


def context_schedule(Z, seeds, n_context):
    """(source, steps): written independently of dinox.propagate -- by distance from the seed instead of by walking."""
    seeds = sorted(set(seeds))
    source = {}
    for z in range(Z):
        if z in seeds:
            continue
        best = None
        for s in seeds:                                                          # ascending: a tie keeps the lower seed
            if best is None or abs(z - s) < abs(z - best):
                best = s
        source[z] = best
    steps = []
    for s in seeds:
        for sign in (1, -1):
            mine = sorted((z for z, src in source.items() if src == s and (z - s) * sign > 0), key=lambda z: abs(z - s))
            for n, z in enumerate(mine):
                steps.append((z, [s] + mine[max(0, n - n_context):n]))
    return source, steps


def bilinear_upsample(p, g, u):
    """float64 [S, S, C] of patch values p [g g, C] at S = g u: the half-pixel-centre bilinear map with clamped borders that
    ops.seg_predict applies (source coordinate (i + 0.5) / u - 0.5, clamped to [0, g - 1])."""
    p = np.asarray(p, np.float64).reshape(g, g, -1)
    c = np.clip((np.arange(g * u) + 0.5) / u - 0.5, 0.0, g - 1.0)
    i0 = np.minimum(np.floor(c).astype(int), g - 1)
    i1 = np.minimum(i0 + 1, g - 1)
    f = c - i0
    rows = p[i0] * (1 - f)[:, None, None] + p[i1] * f[:, None, None]
    return rows[:, i0] * (1 - f)[None, :, None] + rows[:, i1] * f[None, :, None]


# ------------------------------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
SHAPES = [(14, 1, 384, 2), (14, 3, 32, 5), (5, 8, 7, 3), (28, 8, 384, 4), (1, 1, 1, 2), (9, 2, 88, 64)]     # (g, F, D, C)
KS = (1, 5, 32)


def radii(g):
    return (0, 1, 3, 12, -1, g + 5)


def soft_rows(rng, n, C):
    """fp32 [n, C] in [0, 1], rows summing to about 1, some rows all zero."""
    s = rng.dirichlet(np.ones(C), n).astype(np.float32)
    s[rng.random(n) < 0.1] = 0.0
    return s


def exact_case(g, F, D, C, seed=0):
    """Integer-valued fp32 rows in {-3..3}: every score is an exact integer in fp32 and in float64, and ties are everywhere."""
    rng = np.random.default_rng([seed, g, F, D, C])
    N = g * g
    return (rng.integers(-3, 4, (N, D)).astype(np.float32), rng.integers(-3, 4, (F * N, D)).astype(np.float32), soft_rows(rng, F * N, C))


def float_case(g, F, D, C, seed=0):
    """Unit fp32 rows that vary smoothly over the grid (low random Fourier features of (y, x)) plus noise per frame and patch."""
    rng = np.random.default_rng([seed + 1000, g, F, D, C])
    N = g * g
    y, x = np.divmod(np.arange(N), g)
    pos = np.stack([y, x], 1) / max(g, 1)
    field = np.cos(pos @ rng.normal(0.0, 3.0, (2, D)) + rng.uniform(0, 2 * np.pi, D))

    def rows(n_frames):
        r = np.tile(field, (n_frames, 1)) + 1.0 * rng.standard_normal((n_frames * N, D))
        return (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(np.float32)

    return rows(1), rows(F), soft_rows(rng, F * N, C)


def sharp_rows(S, mask, K, tau):
    """bool [N]: the K-th and the (K+1)-th candidate score are more than 2 tau apart (rows with at most K candidates are sharp)."""
    Sm = np.where(mask, S, -np.inf)
    top = -np.sort(-Sm, axis=1)[:, :K + 1]
    if top.shape[1] <= K:
        return np.ones(S.shape[0], bool)
    with np.errstate(invalid="ignore"):
        return ~(top[:, K - 1] - top[:, K] <= 2 * tau)


E2E = dict(Z=9, g=14, D=48, C=3, patch=4, seed_z=4, n_context=3, topk=5, radius=4, temperature=0.1)


def e2e_case(planes="drift"):
    """(feats fp32 [Z, N, D], label maps uint8 [Z, S, S]): two discs that drift slowly along z; the features are a random-weight map
    (one tanh layer) of every patch's class shares and grid position plus a little noise.  planes="same": every slice is the same plane of
    three vertical bands."""
    p = E2E
    Z, g, D, C, u = p["Z"], p["g"], p["D"], p["C"], p["patch"]
    S = g * u
    rng = np.random.default_rng(77)
    yy, xx = np.mgrid[0:S, 0:S] + 0.5
    labs = np.zeros((Z, S, S), np.uint8)
    for z in range(Z):
        if planes == "same":                                                     # patch-aligned bands: straight borders, which the bilinear
            labs[z][:, 5 * u:9 * u] = 1                                          # upsampling of whole-patch labels returns pixel for pixel
            labs[z][:, 9 * u:] = 2                                               # (a pixel's own patch weighs >= 0.625; corners would not)
            continue
        labs[z][(yy - 0.32 * S - 0.6 * z) ** 2 + (xx - 0.30 * S) ** 2 <= (0.17 * S) ** 2] = 1
        labs[z][(yy - 0.68 * S) ** 2 + (xx - 0.66 * S + 0.6 * z) ** 2 <= (0.15 * S) ** 2] = 2
    W = rng.normal(0.0, 1.0, (C + 2, D))
    W[:C] *= 3.0
    y, x = np.divmod(np.arange(g * g), g)
    pos = np.stack([y, x], 1) / g
    noise = rng.standard_normal((Z, g * g, D))
    feats = np.stack([np.tanh(np.concatenate([patch_soft_labels(labs[z], C, u), pos], 1) @ W) + 0.02 * noise[0 if planes == "same" else z]
                      for z in range(Z)])
    return feats.astype(np.float32), labs


def unit64(rows32):
    """float64 unit rows of fp32 rows (what the oracle multiplies; the kernel multiplies the fp32-normalised rows)."""
    r = np.asarray(rows32, np.float64)
    return r / np.maximum(np.linalg.norm(r, axis=-1, keepdims=True), 1e-12)
