"""NumPy float32 emulation of csrc/koleo.hip and of normalize_bwd_kernel (csrc/ntxent.hip) in the kernels' own summation shape: 256
threads, a thread's strided terms, the xor exchange of wave_sum, the four wave cells added in order; the ballot compaction of
koleo_bwd chunk by chunk.  Every product and sum is rounded on its own (no fma), which is the upper end of what the build may do.
`defect` plants one fault; the kernels themselves are never touched."""
import numpy as np

from oracle import koleo_bounds as KB

F32 = np.float32
T = KB.THREADS
LANES = np.arange(T)
DEFECTS = ("tie_highest", "self_is_i", "expanded_dist", "drop_ragged_chunk", "lane63_lost", "offsets_restart", "own_pair_at_zero",
           "eps_squared", "project_clamped", "sq_clamped_one", "tail_dropped")


def strided(terms):
    """[rows, n] fp32 terms -> [rows, 256]: thread t adds terms t, t + 256, ... in order."""
    terms = np.asarray(terms, dtype=F32)
    rows, n = terms.shape
    k = -(-n // T)
    pad = np.zeros((rows, k * T), dtype=F32)
    pad[:, :n] = terms
    pad = pad.reshape(rows, k, T)
    a = np.zeros((rows, T), dtype=F32)
    for q in range(k):
        a = a + pad[:, q]
    return a


def block_sum(part):
    v = np.asarray(part, dtype=F32)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, LANES ^ o]
    t = np.zeros(v.shape[0], dtype=F32)
    for w in range(T // 64):
        t = t + v[:, 64 * w]
    return t


def normalize(x, eps=KB.NORM_EPS, defect=None):
    x = np.asarray(x, dtype=F32)
    a = block_sum(strided(x * x))
    n = np.sqrt(a)
    inv = F32(1.0) / np.maximum(n, F32(eps))
    sq = a * inv * inv
    if defect == "sq_clamped_one":
        sq = np.where(n < F32(eps), F32(1.0), sq)
    return x * inv[:, None], n, sq


def nn(G, sq_all, xh_all, row0, defect=None):
    G, sq_all, xh_all = (np.asarray(a, dtype=F32) for a in (G, sq_all, xh_all))
    V_l, V_g = G.shape
    rows = np.arange(V_l)
    own = row0 + rows
    v = ((sq_all[own, None] + sq_all[None, :]) - F32(2.0) * G).astype(F32)
    v[rows, rows if defect == "self_is_i" else own] = np.inf
    wave = (np.arange(V_g) % T) // 64
    best, bj = np.full(V_l, np.inf, dtype=F32), np.full(V_l, 0x7fffffff, dtype=np.int64)
    for w in range(T // 64):
        cols = np.nonzero(wave == w)[0]
        if cols.size == 0:
            wv, wj = np.full(V_l, np.inf, dtype=F32), np.full(V_l, 0x7fffffff, dtype=np.int64)
        else:
            k = np.argmin(v[:, cols], axis=1)                            # lowest j of the wave's minimum: strict < and the exchange
            wv, wj = v[rows, cols[k]], np.where(np.isinf(v[rows, cols[k]]), 0x7fffffff, cols[k])
        tie = (wj > bj) if defect == "tie_highest" else (wj < bj)
        take = (wv < best) | ((wv == best) & tie) if w else np.ones(V_l, dtype=bool)
        best, bj = np.where(take, wv, best), np.where(take, wj, bj)
    found = bj < V_g
    j = np.where(found, bj, 0)
    t = xh_all[own] - xh_all[j]
    d = np.sqrt(block_sum(strided(t * t)))
    if defect == "expanded_dist":
        d = np.sqrt(np.maximum(best, F32(0.0)))
    return np.where(found, bj, -1).astype(np.int32), np.where(found, d, KB.NO_NEIGHBOUR).astype(F32)


def loss(dist, eps=KB.KOLEO_EPS):
    d = np.asarray(dist, dtype=F32)
    a = block_sum(strided(np.log(d + F32(eps))[None, :]))[0]
    return F32(-a / F32(d.size))


def neighbour_list(idx_all, rg, defect=None):
    """The rows that chose rg, as the chunks of the ballot compaction leave them in LDS."""
    V_g = len(idx_all)
    lst = np.full(V_g + 1, -1, dtype=np.int64)
    s_n = 0
    for base in range(0, V_g, T):
        if defect == "drop_ragged_chunk" and base + T > V_g:
            break
        i = base + LANES
        hit = (i < V_g) & (idx_all[np.minimum(i, V_g - 1)] == rg)
        if defect == "lane63_lost":
            hit &= (LANES & 63) != 63
        start = 0 if defect == "offsets_restart" else s_n
        pos = start + np.cumsum(hit) - hit                               # wave counts in order, then the lanes below inside a wave
        lst[pos[hit]] = i[hit]
        s_n = start + int(hit.sum())
    return lst[:s_n]


def bwd(xh_all, idx_all, dist_all, norm_loc, row0, gscale, eps=KB.KOLEO_EPS, norm_eps=KB.NORM_EPS, defect=None):
    x, d = np.asarray(xh_all, dtype=F32), np.asarray(dist_all, dtype=F32)
    idx, nl = np.asarray(idx_all), np.asarray(norm_loc, dtype=F32)
    gs, eps, neps = F32(gscale), F32(eps), F32(norm_eps)
    V_l, D = nl.size, x.shape[1]
    g = np.zeros((V_l, D), dtype=F32)

    def coef(di):
        with np.errstate(divide="ignore", invalid="ignore"):
            return gs / ((di + eps) * ((di + eps) if defect == "eps_squared" else di))

    with np.errstate(invalid="ignore"):
        for r in range(V_l):
            rg = row0 + r
            xv = x[rg]
            if idx[rg] >= 0 and (d[rg] > 0 or defect == "own_pair_at_zero"):
                g[r] = g[r] + (-coef(d[rg])) * (xv - x[idx[rg]])
            for i in neighbour_list(idx, rg, defect):
                if d[i] > 0:
                    g[r] = g[r] + coef(d[i]) * (x[i] - xv)
    xr = x[row0:row0 + V_l]
    dot = block_sum(strided(g * xr))[:, None]
    cl = (nl < neps)[:, None]
    if defect == "project_clamped":
        cl = np.zeros_like(cl)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.where(cl, g * (F32(1.0) / neps), (g - xr * dot) * (F32(1.0) / nl)[:, None]).astype(F32)


def normalize_bwd(dxh, xh, norm, eps=KB.NORM_EPS, vec=None, defect=None):
    g, u, n = (np.asarray(a, dtype=F32) for a in (dxh, xh, norm))
    V, D = g.shape
    vec = D % 4 == 0 if vec is None else vec
    d4 = D // 4 if vec or defect == "tail_dropped" else 0
    p = g * u
    part = np.zeros((V, T), dtype=F32)
    if d4:
        q = p[:, :4 * d4].reshape(V, d4, 4)
        part = strided(((q[:, :, 0] + q[:, :, 1]) + q[:, :, 2]) + q[:, :, 3])
    if defect != "tail_dropped" and 4 * d4 < D:
        part = part + strided(p[:, 4 * d4:])                             # the tail's first term lands on the thread's float4 sum
    dot = block_sum(part)[:, None]
    cl = (n < F32(eps))[:, None]
    inv = (F32(1.0) / np.where(cl[:, 0], F32(eps), n))[:, None]
    return ((g - u * np.where(cl, F32(0.0), dot)) * inv).astype(F32)


def end_to_end(x, gscale=1.0, defect=None):
    """normalize -> G (float64 product rounded once) -> nn -> loss -> bwd on one process's rows."""
    xh, norm, sq = normalize(x, defect=defect)
    G = KB.gram32(xh, xh)
    idx, dist = nn(G, sq, xh, 0, defect=defect)
    return {"xh": xh, "norm": norm, "sq": sq, "G": G, "idx": idx, "dist": dist, "loss": loss(dist),
            "dx": bwd(xh, idx, dist, norm, 0, F32(gscale / len(x)), defect=defect)}
