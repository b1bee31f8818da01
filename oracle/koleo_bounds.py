"""The KoLeo kernels and the row normalisation, element by element: float64 references, a-priori rounding bounds, hostile rows (CPU).

Kernels (csrc/koleo.hip; normalize_bwd_kernel of csrc/ntxent.hip).  Every one is a workgroup of 256 threads per row (koleo_loss: one
workgroup in all); a row sum is a thread's strided terms, the 6 exchange steps of wave_sum and the 4 waves' cells added in order:
    normalize      a = sum x^2,  norm = sqrt(a),  inv = 1 / max(norm, eps),  xh = x inv,  sq = a inv inv
    nn             v_j = (sq_i + sq_j) - 2 G_ij,  j* = the lowest j != row0 + i that attains min v,  dist = sqrt(sum (xh_i - xh_j*)^2)
                   (no such j: idx = -1, dist = 1e9f)
    loss           -(sum log(dist + eps)) / V
    bwd            c_i = -gscale / ((d_i + eps) d_i);   g = c_rg (xh_r - xh_j) [unless j < 0 or d_rg = 0]
                   + sum over the i with idx_i = rg, ascending, d_i > 0, of  c_i (xh_r - xh_i);
                   dx = (g - xh_r (xh_r . g)) / norm_r,   or g / norm_eps where norm_r < norm_eps
    normalize_bwd  dx = (dxh - xh (xh . dxh)) / norm,  or dxh / eps where norm < eps; the dot product four columns at a time when
                   D % 4 == 0 and the three pointers are 16-byte aligned, one at a time otherwise
Every kernel is judged GIVEN the fp32 arrays it was handed: the reference evaluates the same formulas on those values in float64, so
no error is counted twice (nn: given G and sq; bwd: given idx, dist and norm; the backward of the normalisation: given xh and norm).

What the build does (read from the gfx950 assembly of koleo.hip and ntxent.hip at -O3, no fast-math flag):
  * 1.0f / x is the correctly rounded division (v_div_scale / v_rcp / v_fma ... / v_div_fmas / v_div_fixup), one rounding;
  * sqrtf is correctly rounded (v_sqrt_f32 followed by the two v_fma residual tests that move the result one ulp down or up);
  * logf is v_log_f32 and a fix-up, NOT a correctly rounded operation, so the loss carries the project's logf tolerance;
  * a * b + c IS contracted to v_fma / v_fmac (hipcc's default -ffp-contract=fast).  A contraction removes a rounding, so every bound
    below, which counts the product and the sum as two operations, holds with and without it;
  * the selection value is the SAME fp32 number either way: 2 G is exact, so (sq_i + sq_j) - 2 G rounded once (fma) and
    (sq_i + sq_j) - fl(2 G) are both fl(fl(sq_i + sq_j) - 2 G).  That is why idx can be required exactly (nn_index; the CPU test
    proves the identity on every family).

Bounds, per output element (u = 2^-24, gamma(n) = n u / (1 - n u); every constant is an operation count, written at its builder):
    depth(n) = ceil(n / 256) - 1 + 9   a thread's own additions (its first is 0 + term, exact), the 6 exchange steps of wave_sum and
                   the 3 rounded additions of the four wave cells (the first is 0 + cell, exact)
    normalize      rel(a) = gamma(depth(D) + 1) (the square);  norm: sqrt halves it, + u;  inv: + u;  xh: + u;
                   sq = a_c inv_c inv_c stands on the COMPUTED a: sqrt, division (each squared) and two products: gamma(6) about 1.
                   clamp (norm < eps): inv = fl(1 / eps) (u), xh = x / eps within gamma(2), sq = a / eps^2 within rel(a) + gamma(4);
                   an all-zero row: xh and sq are 0 exactly.  A row whose norm lies within its own bound of eps is refused as an input.
    nn, index      exact (above).  Selection contract, selection_slack(): |v_j - d2_j| <= e_sel(j) = 2 u (|sq_i| + |sq_j| + 2 |G_ij|)
                   (the add and the subtract) + what the handed sq and G themselves differ from |xh|^2 and xh_i . xh_j, so the float64
                   squared distance of the picked row exceeds the true minimum by at most e_sel(picked) + e_sel(nearest) <= 2 e_sel.
    nn, distance   RELATIVE: each difference u, its square 2 u + u, the sum gamma(depth(D)): rel(a) = gamma(depth(D) + 3); the root
                   halves it, + u.  Nothing in it depends on the size of d: it holds at d = 1e-4 as at d = 1.
    loss           [gamma(depth(V) + 1) sum |l_i| + sum (u + LOG_RTOL |l_i|)] / V + u |loss|: d + eps (u in the argument is u in the
                   logarithm), logf (the project's CE_LOSS_RTOL of tests/_small_kernels_oracle.py, passed in), the sum, the division
    bwd            e_g = gamma(5 + n_in + 1) sum |c_i| |xh_i - xh_r|: c (3: the add, the product, the division), the difference, the
                   product, then at most n_in + 1 additions in a row;  e_dot = sum |xh_r| e_g + gamma(depth(D) + 1) sum |g xh_r|;
                   dx: (e_g + |xh_r| e_dot + gamma(4) (|g| + |xh_r dot|)) / norm  (1 / norm, the product, the difference, the product);
                   clamped: (e_g + gamma(2) |g|) / norm_eps
    normalize_bwd  e_dot = gamma(dot_depth + 1) sum |dxh xh|, dot_depth = 4 ceil(D / 1024) - 1 + 9 (float4: three additions inside a
                   trip and one onto the thread's sum, the first of those exact) or depth(D) (scalar);  dx: (|xh| e_dot + gamma(4) (|dxh| + |xh dot|)) / norm;
                   clamped: gamma(2) |dxh| / eps
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np

U32 = 2.0 ** -24
F32, F64 = np.float32, np.float64
THREADS = 256
NORM_EPS = F32(1e-12)                   # the clamp of the normalisation (ops passes 1e-12)
KOLEO_EPS = F32(1e-8)                   # eps inside the logarithm
NO_NEIGHBOUR = F32(1e9)                 # dist where idx = -1
MAX_LIST_ROWS = 15359                   # (V_g + 1) ints of LDS <= 60 KiB
BLOCK_SUM_OPS = 9                       # block_sum: 6 exchange steps + the 4 wave cells added in order, the first of them onto 0
SQ_OPS = 6                              # sqrt and division (each enters squared) + two products
SEL_OPS = 2                             # the add and the subtract (or fma) of the selection value
DIST_TERM_OPS = 3                       # the difference (enters squared: 2) and the square
COEF_OPS = 3                            # d + eps, the product with d, the division
BWD_TERM_OPS = COEF_OPS + 2             # ... the difference of the rows, the product
OUT_OPS = 4                             # 1 / norm, xh dot, the difference, the product
FAMILIES = ("randn", "offset", "pairs", "dup", "zero", "zero2", "tiny", "cluster")
E2E_FAMILIES = FAMILIES + ("offset2",)  # end to end also the mild form of offset: the one whose neighbours the reference decides
SHARE_EXEMPT = ("cluster", "offset")    # families in which a pick may differ from the float64 nearest row (the contract still holds)
WIDTHS = (1, 3, 64, 255, 256, 257, 1000)
WIDE = 8192                             # run once, at 6 rows
NN_SIZES = (1, 2, 63, 64, 65, 256, 257, 700)
RECT = ((100, 700, 0), (100, 700, 300), (100, 700, 600), (1, 257, 256))   # (V_l, V_g, row0)
LOSS_SIZES = (1, 255, 256, 257, 700)
E2E = ((300, 257), (700, 64))
PAIR_D = (1e-4, 1e-3, 3e-2)


def gamma(n: float) -> float:
    return n * U32 / (1.0 - n * U32)


def depth(n: int) -> int:
    return math.ceil(n / THREADS) - 1 + BLOCK_SUM_OPS


def comp(*rels):
    """The relative error of a product of factors with these relative errors."""
    p = 1.0
    for r in rels:
        p = p * (1.0 + r)
    return p - 1.0


# ------------------------------------------------------------------------------------------ inputs
def _key(name: str) -> int:
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def _unit_perp(r, a):
    """A random direction per row of a, orthogonal to it, of the row's own length."""
    n = r.standard_normal(a.shape)
    n -= a * ((n * a).sum(1, keepdims=True) / np.maximum((a * a).sum(1, keepdims=True), 1e-300))
    return n * (np.linalg.norm(a, axis=1, keepdims=True) / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300))


def make_rows(family: str, rows: int, dim: int, seed: int = 0, offset: float = 1e3) -> np.ndarray:
    """fp32 rows [rows, dim].  offset: `offset` x one common vector + randn, all rows nearly parallel (offset2: 2 x, cos = 0.8).  pairs: rows 3k + 1 (k = 0..)
    are copies of rows 3k moved by an angle of PAIR_D[k % 3] (needs dim >= 2).  dup: rows 1, 2 copy row 0, row rows-1 copies row 5.
    zero / zero2: row 2 (and row rows-2) all zero.  tiny: row 1 has norm 1e-13 (below the clamp), row 3 norm 1e-11.  cluster: rows
    0..4 within 1e-3 (angle) of each other."""
    r = np.random.default_rng([23, _key(family), rows, dim, seed])
    x = r.standard_normal((rows, dim))
    if family == "randn":
        pass
    elif family in ("offset", "offset2"):
        x = (offset if family == "offset" else 2.0) * r.standard_normal((1, dim)) + x
    elif family == "pairs":
        for k in range(min(6, (rows - 1) // 3)):
            a = x[3 * k:3 * k + 1]
            x[3 * k + 1] = (a + PAIR_D[k % 3] * _unit_perp(r, a))[0] if dim > 1 else a[0]
    elif family == "dup":
        x[1 % rows] = x[0]
        x[2 % rows] = x[0]
        x[rows - 1] = x[5 % rows]
    elif family in ("zero", "zero2"):
        x[2 % rows] = 0.0
        if family == "zero2":
            x[rows - 2] = 0.0
    elif family == "tiny":
        x[1 % rows] *= 1e-13 / np.linalg.norm(x[1 % rows])
        x[3 % rows] *= 1e-11 / np.linalg.norm(x[3 % rows])
    elif family == "cluster":
        for k in range(1, min(5, rows)):
            x[k] = (x[0:1] + 0.5e-3 * _unit_perp(r, x[0:1]))[0] if dim > 1 else x[0]
    else:
        raise ValueError(family)
    return np.ascontiguousarray(x, dtype=F32)


# End to end the selection is judged on the library's own G, whose a-priori error (any summation order over D terms) is about D u.
# In `offset` (1e3 x the common vector) all rows lie within that error of each other: which of them is picked is NOT decided by the
# float64 reference, the selection contract alone judges the pick (SHARE_EXEMPT), as in cluster.  In every other family the seed is
# the first at which the float64 nearest row of every row with a direction beats the rest by more than 2 e_sel, so that a differing
# pick is a broken contract and not a coin toss.  E2E_SEEDS caches first_decisive_seed() (`python -m oracle.koleo_bounds` prints the
# table); tests/test_koleo_bounds_cpu.py checks every entry on the emulated rows.
E2E_SEEDS = {(300, 257): {"randn": 1, "pairs": 9, "offset2": 19}, (700, 64): {"pairs": 6, "offset2": 3}}            # every other entry: 0


def e2e_seed(family: str, rows: int, dim: int) -> int:
    return E2E_SEEDS.get((rows, dim), {}).get(family, 0)


def decisive_margin(family: str, rows: int, dim: int, seed: int) -> float:
    """The smallest `clear` (selection_contract) over the rows with a direction, on float64-normalised rows rounded to fp32 and the
    library's a-priori G error.  cluster: over the rows outside the cluster."""
    x = make_rows(family, rows, dim, seed).astype(F64)
    n = np.sqrt((x * x).sum(1, keepdims=True))
    xh = (x / np.maximum(n, float(NORM_EPS))).astype(F32)
    G, sq = gram32(xh, xh), sq32(xh)
    e_sq, e_g = handed_errors(xh, xh, dim + max(1, dim // 256))
    clear = selection_contract(nn_index(G, sq, 0), G, sq, xh, 0, e_sq, e_g)["clear"]
    keep = (xh != 0).any(1)
    if family == "cluster":
        keep[:5] = False
    return float(clear[keep].min())


def first_decisive_seed(family: str, rows: int, dim: int, need: float = 1.5, tries: int = 64) -> int:
    for seed in range(tries):
        if decisive_margin(family, rows, dim, seed) > need:
            return seed
    raise ValueError(f"no decisive seed for {family} {rows} x {dim}")


def gram32(xh_loc: np.ndarray, xh_all: np.ndarray) -> np.ndarray:
    """The inner products in float64, rounded once to fp32: a G that carries no GEMM."""
    return (xh_loc.astype(F64) @ xh_all.astype(F64).T).astype(F32)


def sq32(xh: np.ndarray) -> np.ndarray:
    return (xh.astype(F64) ** 2).sum(1).astype(F32)


def unit_rows(rows: int, dim: int, seed: int = 0) -> np.ndarray:
    x = np.random.default_rng([29, rows, dim, seed]).standard_normal((rows, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)


TIE_MODES = ("three_waves", "second_trip", "last", "around_self")


def tie_case(mode: str, V_l: int, V_g: int, row0: int, seed: int = 0):
    """A hand-made G with exact ties (sq = 1 everywhere).  Every entry is a multiple of 2^-10 in [-0.5, 0.5], so v = 2 - 2 G is exact;
    the diagonal holds 1 (v = 0, the smallest value of all, and excluded); the minimum over the rest, G = 0.75, is planted at columns
    {70, 130, 257} (three_waves: waves 1, 2 and 0 of the search), {257, 300} (second_trip: both found on a thread's second visit),
    V_g - 1 (last) or self - 1 and self + 1 (around_self).  Returns G [V_l, V_g], sq [V_g] and the required idx [V_l]."""
    r = np.random.default_rng([31, _key(mode), V_l, V_g, row0, seed])
    G = (r.integers(-512, 513, size=(V_l, V_g)) / 1024.0).astype(F32)
    own = row0 + np.arange(V_l)
    want = np.empty(V_l, dtype=np.int32)
    for i, s in enumerate(own):
        cols = {"three_waves": (70, 130, 257), "second_trip": (257, 300), "last": (V_g - 1,), "around_self": (s - 1, s + 1)}[mode]
        cols = [c for c in cols if 0 <= c < V_g and c != s] or [V_g - 2]          # the last row itself: its other neighbour
        G[i, cols] = 0.75
        G[i, s] = 1.0
        want[i] = min(cols)
    return G, np.ones(V_g, dtype=F32), want


BWD_CASES = ("hub300", "hub700", "lanes", "nohits", "neg", "dzero", "clamped", "row0")


def bwd_case(name: str, D: int = 24, seed: int = 0) -> dict:
    """Hand-made idx_all / dist_all for koleo_bwd (gscale = 0.37 / V_l throughout, never 1).  hub: every row chooses row 0, so
    n_in = V_g - 1 with a ragged last chunk.  lanes: row 5 is chosen exactly by the rows at lanes 0 and 63 of every wave of every chunk.
    nohits: nobody chooses a local row.  neg: a third of the rows have idx = -1 (dist 1e9).  dzero: d = 0 on own pairs and on rows that
    chose a local row.  clamped: norm_loc below norm_eps, and 0.  row0: 100 local rows at 300 of 700."""
    V_g = {"hub300": 300, "nohits": 300}.get(name, 700)
    V_l, row0 = {"nohits": (4, 0), "row0": (100, 300), "lanes": (16, 0)}.get(name, (V_g, 0))
    r = np.random.default_rng([37, _key(name), D, seed])
    xh = unit_rows(V_g, D, seed + 1)
    idx = (np.arange(V_g) + r.integers(1, V_g, size=V_g)) % V_g
    if name.startswith("hub"):
        idx[:] = 0
        idx[0] = 1
    elif name == "lanes":
        idx[:] = np.where(np.arange(V_g) == 9, 10, 9)
        lane = np.arange(V_g) & 63
        idx[((lane == 0) | (lane == 63)) & (np.arange(V_g) != 5)] = 5
    elif name == "nohits":
        idx[:] = 100 + (np.arange(V_g) % 50)
        idx[100:150] += 50
    elif name == "neg":
        idx[r.random(V_g) < 1.0 / 3.0] = -1
    x64 = xh.astype(F64)
    dist = np.where(idx < 0, float(NO_NEIGHBOUR), np.sqrt(((x64 - x64[np.maximum(idx, 0)]) ** 2).sum(1))).astype(F32)
    if name == "dzero":
        idx[:40] = 3                                                     # row 3 is chosen by 39 rows, half of them at d = 0
        idx[3] = 4
        dist[0:40:2] = 0.0
        dist[3] = 0.0
        dist[r.random(V_g) < 0.2] = 0.0
    norm = r.uniform(0.5, 20.0, size=V_l).astype(F32)
    if name == "clamped":
        norm[1], norm[2], norm[V_l - 1] = 1e-13, 0.0, 9.9e-13
    return {"xh_all": xh, "idx_all": idx.astype(np.int32), "dist_all": dist, "norm_loc": norm, "row0": row0, "V_l": V_l, "V_g": V_g,
            "D": D, "gscale": float(F32(0.37 / V_l))}


NBWD_WIDTHS = (1, 6, 257, 4, 1024, 1028)


def nbwd_case(D: int, rows: int = 5, seed: int = 0):
    """dxh, xh, norm for normalize_bwd: row 0 plain, row 1 has dxh parallel to xh (dx about 0), row 2 a clamped norm, row 3 norm 0."""
    r = np.random.default_rng([41, D, rows, seed])
    xh = unit_rows(rows, D, seed + 2)
    dxh = r.standard_normal((rows, D)).astype(F32)
    dxh[1] = F32(3.0) * xh[1]
    norm = r.uniform(0.5, 20.0, size=rows).astype(F32)
    norm[2], norm[3] = 1e-13, 0.0
    return dxh, xh, norm


# ------------------------------------------------------------------------------------------ normalize
def normalize_ref(x: np.ndarray, eps=NORM_EPS) -> Dict[str, np.ndarray]:
    """norm, sq [V] and xh [V, D] in float64 on the fp32 x, with `<name>_bound`."""
    x = np.asarray(x, dtype=F64)
    eps = float(F32(eps))
    D = x.shape[1]
    ra = gamma(depth(D) + 1)
    a = (x * x).sum(1)
    n = np.sqrt(a)
    rel_n = comp(math.sqrt(1.0 + ra) - 1.0, U32)
    if (np.abs(n - eps) <= rel_n * n).any():
        raise ValueError("a row's norm lies within its own rounding of eps: the clamp is not decided by the input")
    cl = n < eps
    rel_inv = comp(rel_n / (1.0 - rel_n), U32)
    inv = 1.0 / np.maximum(n, eps)
    xh = x * inv[:, None]
    rel_xh = np.where(cl, gamma(2), comp(rel_inv, U32))
    sq = a * inv * inv
    e_sq = np.where(cl, comp(ra, gamma(4)) * sq, gamma(SQ_OPS) * sq)
    return {"norm": n, "norm_bound": rel_n * n, "xh": xh, "xh_bound": rel_xh[:, None] * np.abs(xh), "sq": sq, "sq_bound": e_sq,
            "clamped": cl}


# ------------------------------------------------------------------------------------------ nn
def selection_values(G, sq_all, row0: int) -> np.ndarray:
    """v [V_l, V_g] in fp32 as the kernel rounds it: fl(fl(sq_i + sq_j) - 2 G_ij); the excluded diagonal is +inf."""
    G, sq_all = np.asarray(G, dtype=F32), np.asarray(sq_all, dtype=F32)
    V_l = G.shape[0]
    s = sq_all[row0:row0 + V_l, None] + sq_all[None, :]
    v = (s - F32(2.0) * G).astype(F32)
    v[np.arange(V_l), row0 + np.arange(V_l)] = np.inf
    return v


def nn_index(G, sq_all, row0: int) -> np.ndarray:
    """The required idx [V_l] (int32): the first index of the fp32 minimum over j != row0 + i, -1 where there is no such j."""
    v = selection_values(G, sq_all, row0)
    if v.shape[1] == 1:
        return np.full(v.shape[0], -1, dtype=np.int32)
    return np.argmin(v, axis=1).astype(np.int32)


def selection_slack(sq_i, sq_j, g_ij, e_sq_i=0.0, e_sq_j=0.0, e_g=0.0):
    """e_sel: how far the fp32 selection value of (i, j) may lie from the float64 squared distance of the two rows.  e_sq / e_g: how far
    the handed sq and G may themselves lie from |xh|^2 and xh_i . xh_j."""
    return gamma(SEL_OPS) * (np.abs(sq_i) + np.abs(sq_j) + 2.0 * np.abs(g_ij)) + e_sq_i + e_sq_j + 2.0 * e_g


def d2_matrix(xh_all: np.ndarray, row0: int, V_l: int) -> np.ndarray:
    """Float64 squared distances [V_l, V_g] on the rows themselves (differences first); the diagonal is +inf."""
    x = np.asarray(xh_all, dtype=F64)
    out = np.empty((V_l, x.shape[0]))
    for i in range(V_l):
        t = x - x[row0 + i]
        out[i] = (t * t).sum(1)
        out[i, row0 + i] = np.inf
    return out


def selection_contract(idx, G, sq_all, xh_all, row0: int, e_sq=None, e_g=None) -> dict:
    """Judge picked indices against the float64 nearest rows.  excess = d2(picked) - min d2, allowed = e_sel(picked) + e_sel(nearest).
    Returns the worst excess / allowed, the share of rows with excess > 0, the largest excess, and per row the smallest margin by which
    the float64 nearest beats every other row, in units of the allowed slack (`clear` > 1: the reference alone decides the pick)."""
    G, sq = np.asarray(G, dtype=F64), np.asarray(sq_all, dtype=F64)
    idx = np.asarray(idx)
    V_l, V_g = G.shape
    rows = np.arange(V_l)
    d2 = d2_matrix(xh_all, row0, V_l)
    esq = np.zeros(V_g) if e_sq is None else np.broadcast_to(np.asarray(e_sq, dtype=F64), (V_g,))
    eg = np.zeros((V_l, V_g)) if e_g is None else np.broadcast_to(np.asarray(e_g, dtype=F64), (V_l, V_g))
    slack = selection_slack(sq[row0:row0 + V_l, None], sq[None, :], G, esq[row0:row0 + V_l, None], esq[None, :], eg)
    near = np.argmin(d2, axis=1)
    excess = d2[rows, idx] - d2[rows, near]
    allowed = slack[rows, idx] + slack[rows, near]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(excess <= 0.0, 0.0, excess / allowed)
        margin = (d2 - d2[rows, near][:, None]) / (slack + slack[rows, near][:, None])
    margin[rows, near] = np.inf
    margin[d2 == d2[rows, near][:, None]] = np.inf                       # an exact twin of the nearest row is as near
    return {"ratio": float(ratio.max()), "share": float((excess > 0.0).mean()), "excess": float(excess.max()),
            "clear": margin.min(axis=1), "near": near, "d2": d2}


def nn_dist_ref(xh_all, idx, row0: int):
    """dist [V_l] in float64 on the fp32 rows of the given idx, and its bound (relative; idx = -1: exactly 1e9f, bound 0)."""
    x = np.asarray(xh_all, dtype=F64)
    idx = np.asarray(idx)
    V_l, D = len(idx), x.shape[1]
    j = np.where(idx < 0, 0, idx)
    t = x[row0:row0 + V_l] - x[j]
    d = np.sqrt((t * t).sum(1))
    rel = comp(math.sqrt(1.0 + gamma(depth(D) + DIST_TERM_OPS)) - 1.0, U32)
    return np.where(idx < 0, float(NO_NEIGHBOUR), d), np.where(idx < 0, 0.0, rel * d)


def handed_errors(xh_loc, xh_all, gemm_terms: int):
    """(e_sq [V_g], e_g [V_l, V_g]) for selection_contract: how far the sq of koleo_normalize lies from the float64 |xh|^2 of the fp32
    rows it wrote (a_c against a: gamma(depth(D) + 1); the two products of sq and the squared product of xh: 4), and how far a G summed
    in ANY order over gemm_terms rounded operations lies from the float64 product (gemm_terms = 1: gram32)."""
    xl, xa = np.abs(np.asarray(xh_loc, dtype=F64)), np.abs(np.asarray(xh_all, dtype=F64))
    return gamma(depth(xa.shape[1]) + 5) * (xa * xa).sum(1), gamma(gemm_terms) * (xl @ xa.T)


# ------------------------------------------------------------------------------------------ loss
def loss_ref(dist, eps=KOLEO_EPS, log_rtol: float = 1e-5):
    """-mean log(dist + eps) in float64 on the fp32 dist, and its bound.  log_rtol: the project's logf tolerance (CE_LOSS_RTOL)."""
    d = np.asarray(dist, dtype=F64)
    V = d.size
    l = np.log(d + float(F32(eps)))
    loss = -l.sum() / V
    e = (gamma(depth(V) + 1) * np.abs(l).sum() + (gamma(1) + log_rtol * np.abs(l)).sum()) / V + U32 * abs(loss)
    return loss, e


# ------------------------------------------------------------------------------------------ bwd
def bwd_ref(xh_all, idx_all, dist_all, norm_loc, row0: int, gscale: float, eps=KOLEO_EPS, norm_eps=NORM_EPS) -> Dict[str, np.ndarray]:
    """dx [V_l, D] in float64 on the handed arrays, its bound, and n_in [V_l]: how many rows chose each local row."""
    x = np.asarray(xh_all, dtype=F64)
    idx = np.asarray(idx_all).astype(np.int64)
    d = np.asarray(dist_all, dtype=F64)
    nl = np.asarray(norm_loc, dtype=F64)
    gs, eps, neps = float(F32(gscale)), float(F32(eps)), float(F32(norm_eps))
    V_g, D = x.shape
    V_l = nl.size
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(d > 0.0, -gs / ((d + eps) * d), 0.0)
    g, ga = np.zeros((V_l, D)), np.zeros((V_l, D))
    own = np.arange(row0, row0 + V_l)
    has = (idx[own] >= 0) & (d[own] > 0.0)
    t = np.where(has, c[own], 0.0)[:, None] * (x[own] - x[np.where(has, idx[own], 0)])
    g += t
    ga += np.abs(t)
    chose = np.nonzero((idx >= row0) & (idx < row0 + V_l))[0]
    n_in = np.bincount(idx[chose] - row0, minlength=V_l)
    live = chose[d[chose] > 0.0]
    t = c[live][:, None] * (x[idx[live]] - x[live])
    np.add.at(g, idx[live] - row0, t)
    np.add.at(ga, idx[live] - row0, np.abs(t))
    xr = x[own]
    e_g = np.array([gamma(BWD_TERM_OPS + n + 1) for n in n_in])[:, None] * ga
    dot = (g * xr).sum(1, keepdims=True)
    e_dot = (np.abs(xr) * e_g).sum(1, keepdims=True) + gamma(depth(D) + 1) * np.abs(g * xr).sum(1, keepdims=True)
    cl = (nl < neps)[:, None]
    n = np.where(cl, neps, nl.reshape(-1, 1))
    dx = np.where(cl, g, g - xr * dot) / n
    e = np.where(cl, e_g + gamma(2) * np.abs(g), e_g + np.abs(xr) * e_dot + gamma(OUT_OPS) * (np.abs(g) + np.abs(xr * dot))) / n
    return {"dx": dx, "dx_bound": e, "n_in": n_in}


# ------------------------------------------------------------------------------------------ normalize_bwd
def normalize_bwd_ref(dxh, xh, norm, eps=NORM_EPS, vec: Optional[bool] = None):
    """dx [V, D] in float64 and its bound.  vec: the float4 kernel (None: what D % 4 == 0 selects for aligned pointers)."""
    g, u = np.asarray(dxh, dtype=F64), np.asarray(xh, dtype=F64)
    D = g.shape[1]
    vec = D % 4 == 0 if vec is None else vec
    assert not vec or D % 4 == 0
    dd = 4 * math.ceil(D / (4 * THREADS)) - 1 + BLOCK_SUM_OPS if vec else depth(D)
    eps = float(F32(eps))
    nrm = np.asarray(norm, dtype=F64).reshape(-1, 1)
    cl = nrm < eps
    dot = (g * u).sum(1, keepdims=True)
    e_dot = gamma(dd + 1) * np.abs(g * u).sum(1, keepdims=True)
    n = np.where(cl, eps, nrm)
    dx = np.where(cl, g, g - u * dot) / n
    e = np.where(cl, gamma(2) * np.abs(g), np.abs(u) * e_dot + gamma(OUT_OPS) * (np.abs(g) + np.abs(u * dot))) / n
    return dx, e


# ------------------------------------------------------------------------------------------ judging a result
def check(got, ref, bound) -> dict:
    """The largest |got - ref| / bound over EVERY element (a non-finite element counts as infinite; an element with bound 0 must
    equal its reference), where it is, and the number of non-finite elements."""
    ref = np.asarray(ref, dtype=F64)
    got = np.asarray(got, dtype=F64).reshape(ref.shape)
    bound = np.broadcast_to(np.asarray(bound, dtype=F64), ref.shape)
    bad = ~np.isfinite(got)
    err = np.abs(np.where(bad, 0.0, got) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bad, np.inf, np.where(err == 0.0, 0.0, err / bound))
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
    return {"ratio": float(ratio[at]) if ratio.size else 0.0, "where": tuple(int(i) for i in at), "nan": int(bad.sum())}


if __name__ == "__main__":
    print({shape: {f: first_decisive_seed(f, *shape) for f in E2E_FAMILIES if f not in SHARE_EXEMPT} for shape in E2E})
