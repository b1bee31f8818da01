"""The NT-Xent kernels of csrc/ntxent.hip, element by element: float64 statements, a-priori rounding bounds, hostile similarity
matrices, and an fp32 NumPy emulation in the kernels' own order with planted defects (CPU; no torch, no device).

Kernels.  S is an ARBITRARY fp32 matrix here (not necessarily symmetric, not necessarily a product of unit rows), x = S inv_tau:
    rows        lse_i = logsumexp_{j != d(i)} x_ij,   row_loss_i = lse_i - x_{i p(i)};   one workgroup of 256 threads per row:
                the maximum, a thread's strided sum of exp(x - mx), block_sum, one logf
    sum         (sum_i row_loss_i) / divisor: one thread, M additions in index order (through LDS, 1024 rows per pass)
    coeff       W_ij = scale (exp(x_ij - lse_i) + exp(x_ji - lse_j) - [j = p(i)] - [i = p(j)]),  W_ii = 0,  scale = gscale inv_tau / M;
                32 x 32 tiles, S_ji read through the LDS image of the mirror tile
    rows_rect   the same row pass over [Ml, Mg]: d(i) = row0 + i, p(i) = row0 + (i + Bl) mod Ml
    coeff_rect  W_ij = scale (exp(x_ij - lse_local_i) + exp(x_ij - lse_all_j) - 2 [j = p(i)]),  W_{i, row0 + i} = 0,  scale = gscale inv_tau / Ml
The square forms are d(i) = i, p(i) = (i + M/2) mod M.  The statements are those of tests/_ntxent_oracle.py and
tests/_ntxent_dp_oracle.py (rows_rect and coeff_rect are called from there, not restated); only the square coeff on an asymmetric S
is new.  Every kernel is judged GIVEN the fp32 arrays it was handed: coeff takes the lse the device produced, sum the device's
row_loss, so no kernel's error is charged to the next.

Bounds: (n_ops + 2) u (sum of the absolute terms of the element) + TINY, u = 2^-24, as in tests/_small_kernels_oracle.py (+2 is the
head-room for fma contraction and for scalars rounded on the host; TINY = 1e-37 is room for a result that lands among the fp32
subnormals, e.g. exp(-100) at tau = 0.01).  Operation counts:
    argument of an exp   x - m: the product S inv_tau (1), the subtraction (1):        ARG_OPS = 2   on |x| + |m|
    expf, logf           EXP_LOG_RTOL = 1e-5 relative: the project's CE_LOSS_RTOL of tests/_small_kernels_oracle.py (the allowance the
                         DINO cross-entropy, Sinkhorn and KoLeo bounds already give expf / logf; tests/test_ntxent_bounds_cpu.py
                         asserts that the two constants are the same number).  Nothing here is measured on a device.
    lse                  the positive sum: the softmax-weighted mean of the argument errors + EXP_LOG_RTOL, then depth(n) = ceil(n / 256)
                         - 1 + 9 additions on the longest path (a thread's own, its first onto 0; the 6 exchange steps of wave_sum; the
                         4 wave cells added in order, the first onto 0): relative in the sum = absolute in its logarithm;
                         logf: EXP_LOG_RTOL |log a|;  mx + log a: LSE_OPS = 1 on |mx| + |log a|
    row_loss             + the product and the subtraction: ROW_OPS = 2 on |lse| + |x_ip|
    loss                 n additions in a row and the division: SUM_OPS(n) = n + 1 on sum |row_loss| / divisor
    W                    each exponential: P ((ARG_OPS + 2) u (|x| + |lse|) + EXP_LOG_RTOL);  then P1 + P2 (1), minus the indicators (1),
                         times scale (1), scale itself gscale inv_tau / M rounded twice on the host (2): W_OPS = 5 on P1 + P2 + indicators
    dz, end to end       see e2e_ref
"""
from __future__ import annotations

import math
import os
import sys
from typing import Optional

import numpy as np

from oracle.koleo_bounds import check, gamma, normalize_bwd_ref, normalize_ref  # noqa: F401  (check is re-exported)

try:
    import _ntxent_dp_oracle as DPO
    import _ntxent_oracle as NX
except ImportError:                                                      # imported outside pytest: the two statements live beside the tests
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import _ntxent_dp_oracle as DPO
    import _ntxent_oracle as NX

U = 2.0 ** -24
TINY = 1e-37
F32, F64 = np.float32, np.float64
EXP_LOG_RTOL = 1e-5                     # == tests/_small_kernels_oracle.CE_LOSS_RTOL
THREADS, TILE, SUM_CHUNK = 256, 32, 1024
ARG_OPS, LSE_OPS, ROW_OPS, W_OPS = 2, 1, 2, 5
GEMM_EPI_OPS = 4                        # EPI_OPS of oracle/gemm_bounds.py
CANARY = np.array([0x7A5C3CA5], dtype=np.uint32).view(F32)[0]           # 2.9e35, a value no case produces

FAMILIES = ("randn", "asym", "duplicates", "collapsed", "onehot", "antipodal", "zero_rows")
E2E_FAMILIES = ("randn", "duplicates", "onehot", "antipodal", "zero_rows")
SQUARE_M = (2, 6, 34, 66, 256, 258, 1026)
TAUS = (0.5, 0.1, 0.07, 0.01)
GSCALES = (1.0, 0.25)
RECT = ((2, 1), (2, 3), (6, 2), (34, 2), (66, 4), (258, 2))            # (Ml, world), every row0 of each
SHARD = ((2, 3), (6, 2), (66, 4))
E2E_M, E2E_D, E2E_TAUS = (6, 66, 258), (5, 32, 384), (0.1, 0.01)
LDS_PAD, LDW_PAD = 5, 3
MUTANTS = ("diag_included", "last_col_dropped", "second_stride_dropped", "pos_wrap_off_by_one", "mirror_not_transposed",
           "lse_i_for_lse_j", "pair_counted_once", "scale_without_M", "rect_row0_ignored", "rect_pair_1_not_2",
           "sum_second_pass_dropped", "mirror_oob_not_zeroed_then_used")


VARIANTS = FAMILIES + ("randn@1e30",)   # per shape one input whose excluded entries hold 1e30, not NaN: it would win the maximum if read


def variant(v: str):
    """'family' or 'family@fill' -> (family, what the excluded entries hold)."""
    family, _, fill = v.partition("@")
    return family, (float(fill) if fill else np.nan)


def judge_rows(lse, row_loss, out, S, inv_tau: float, Mg: int, row0: int, divisor: float, ref: Optional[dict] = None) -> dict:
    """Ratios error / bound of one rows launch: lse and row_loss against float64 on S; `loss` is the sum kernel GIVEN the row_loss it
    read; `loss_e2e` is the same output against the float64 row losses (their bounds, then the chain)."""
    ref = rows_ref(S, inv_tau, Mg, row0) if ref is None else ref
    c = {k: check(v, ref[k], ref[k + "_bound"]) for k, v in (("lse", lse), ("row_loss", row_loss))}
    s, b = sum_ref(row_loss, divisor)
    c["loss"] = check(out, s, b)
    s64, b64 = sum_ref(ref["row_loss"].astype(F64), divisor)
    c["loss_e2e"] = check(out, s64, b64 + ref["row_loss_bound"].sum() / divisor)
    return {k: (v["ratio"] if v["nan"] == 0 else math.inf) for k, v in c.items()}


def judge_w(flat, rows: int, cols: int, ldw: int, ref: dict, gscale: float = 1.0) -> float:
    """Ratio of one coeff launch: every element of W (ref at gscale 1 scales exactly), inf if a canary changed or an element is not
    finite."""
    W, clean = split_w(flat, rows, cols, ldw)
    g = f32(gscale)
    c = check(W, g * ref["W"], np.where(ref["W_bound"] > 0.0, abs(g) * (ref["W_bound"] - TINY) + TINY, 0.0))
    return c["ratio"] if clean and c["nan"] == 0 else math.inf


def f32(x) -> float:
    """The fp32 value of a host scalar that the C ABI takes as float."""
    return float(F32(x))


def depth(n: int) -> int:
    return math.ceil(n / THREADS) - 1 + 9


def positives(Ml: int, row0: int = 0) -> np.ndarray:
    i = np.arange(Ml)
    return row0 + (i + Ml // 2) % Ml


# ------------------------------------------------------------------------------------------ inputs
def _key(name: str) -> int:
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def sample_rows(Ml: int, world: int):
    """Global row indices (z1 row, z2 row) of every sample, ranks holding [z1_r; z2_r] blocks of Ml rows."""
    Bl = Ml // 2
    s = np.arange(world * Bl)
    r, b = s // Bl, s % Bl
    return r * Ml + b, r * Ml + Bl + b


def make_z(family: str, Ml: int, world: int = 1, D: int = 32, seed: int = 0) -> np.ndarray:
    """Unit rows [world Ml, D] in float64 (zero_rows: two rows all zero), laid out in rank blocks [z1_r; z2_r].
    duplicates: samples 2k and 2k + 1 are the same sample (an odd last one copies sample 0), so every row has an exact copy that is
    not its positive (one sample in all: nothing to copy, the family is randn).  collapsed: one direction.  onehot: sample s has
    z1 = z2 = the basis vector s mod D.  antipodal: z2 = -z1.  zero_rows: rows 1 and Mg - 2 are zero."""
    Mg, Bg = Ml * world, Ml * world // 2
    r = np.random.default_rng([43, _key(family), Ml, world, D, seed])
    a, b = r.standard_normal((Bg, D)), r.standard_normal((Bg, D))
    if family == "duplicates":
        base = np.arange(Bg) - np.arange(Bg) % 2
        if Bg % 2:
            base[-1] = 0
        a, b = a[base], b[base]
    elif family == "collapsed":
        a = b = np.broadcast_to(a[:1], (Bg, D)).copy()
    elif family == "onehot":
        a = b = np.eye(D)[np.arange(Bg) % D]
    elif family == "antipodal":
        b = -a
    elif family not in ("randn", "zero_rows"):
        raise ValueError(family)
    z = np.empty((Mg, D))
    i1, i2 = sample_rows(Ml, world)
    z[i1], z[i2] = a, b
    z /= np.linalg.norm(z, axis=1, keepdims=True)
    if family == "zero_rows":
        z[[1 % Mg, Mg - 2]] = 0.0
    return z


def make_S(family: str, Ml: int, world: int = 1, seed: int = 0) -> np.ndarray:
    """The global fp32 S [Mg, Mg] of a family, built in float64 and rounded once; rank r's rectangular S is rows r Ml .. (r + 1) Ml.
    asym: independent entries in [-1, 1].  onehot: every sample its own axis (D = Mg / 2).  collapsed: exactly 1 everywhere."""
    Mg = Ml * world
    if family == "asym":
        return np.random.default_rng([47, Ml, world, seed]).uniform(-1.0, 1.0, (Mg, Mg)).astype(F32)
    if family == "collapsed":
        return np.ones((Mg, Mg), dtype=F32)
    z = make_z(family, Ml, world, D=Mg // 2 if family == "onehot" else 32, seed=seed)
    return (z @ z.T).astype(F32)


def poison(S: np.ndarray, row0: int = 0, ld: Optional[int] = None, excluded=np.nan) -> np.ndarray:
    """S [Ml, Mg] -> [Ml, ld] with `excluded` (NaN, or 1e30) on every excluded entry (i, row0 + i) and NaN on the columns [Mg, ld)."""
    Ml, Mg = S.shape
    out = np.full((Ml, Mg if ld is None else ld), np.nan, dtype=F32)
    out[:, :Mg] = S
    out[np.arange(Ml), row0 + np.arange(Ml)] = excluded
    return out


# ------------------------------------------------------------------------------------------ statements and bounds
def _x(S, Mg: int, inv_tau: float) -> np.ndarray:
    return np.asarray(S, dtype=F64)[:, :Mg] * f32(inv_tau)


def rows_ref(S, inv_tau: float, Mg: Optional[int] = None, row0: int = 0) -> dict:
    """S [Ml, >= Mg] (excluded entries and padding may hold anything) -> lse, row_loss [Ml] in float64 with `<name>_bound`."""
    S = np.asarray(S)
    Ml = S.shape[0]
    Mg = S.shape[1] if Mg is None else Mg
    x = _x(S, Mg, inv_tau)
    with np.errstate(all="ignore"):
        lse, row_loss = DPO.rows_rect(x, row0, Ml // 2)
    i = np.arange(Ml)
    off = np.ones((Ml, Mg), dtype=bool)
    off[i, row0 + i] = False
    xm = np.where(off, x, -np.inf)
    mx = xm.max(1, keepdims=True)
    e = np.exp(xm - mx)
    s = e.sum(1)
    da = (ARG_OPS + 2) * U * np.where(off, np.abs(x) + np.abs(mx), 0.0)
    rel = (e * da).sum(1) / s + EXP_LOG_RTOL + (depth(Mg) + 2) * U
    logs = np.abs(np.log(s))
    b_lse = rel + EXP_LOG_RTOL * logs + (LSE_OPS + 2) * U * (np.abs(mx[:, 0]) + logs) + TINY
    xp = x[i, positives(Ml, row0)]
    b_row = b_lse + (ROW_OPS + 2) * U * (np.abs(lse) + np.abs(xp)) + TINY
    return {"lse": lse, "lse_bound": b_lse, "row_loss": row_loss, "row_loss_bound": b_row}


def sum_ref(row_loss, divisor: float):
    """(sum row_loss) / divisor on the handed fp32 row_loss, and its bound: the serial chain of n additions and the division."""
    r = np.asarray(row_loss, dtype=F64)
    return r.sum() / divisor, (r.size + 1 + 2) * U * np.abs(r).sum() / divisor + TINY


def _w(x1, l1, x2, l2, ind, scale, zero):
    with np.errstate(all="ignore"):
        P1, P2 = np.exp(x1 - l1), np.exp(x2 - l2)
        dP = P1 * ((ARG_OPS + 2) * U * (np.abs(x1) + np.abs(l1)) + EXP_LOG_RTOL) + P2 * ((ARG_OPS + 2) * U * (np.abs(x2) + np.abs(l2)) + EXP_LOG_RTOL)
        W = scale * (P1 + P2 - ind)
        b = abs(scale) * (dP + (W_OPS + 2) * U * (P1 + P2 + ind)) + TINY
    return np.where(zero, 0.0, W), np.where(zero, 0.0, b), np.where(zero, 0.0, P1), np.where(zero, 0.0, P2)


def coeff_ref(S, lse, inv_tau: float, gscale: float = 1.0, M: Optional[int] = None) -> dict:
    """The square W [M, M] in float64 on the handed S and lse, with W_bound (the diagonal: 0, bound 0) and the two P terms."""
    M = len(lse) if M is None else M
    x = _x(np.asarray(S)[:M], M, inv_tau)
    l = np.asarray(lse, dtype=F64)
    pos = positives(M)
    T = np.zeros((M, M))
    T[np.arange(M), pos] = 1.0
    W, b, P1, P2 = _w(x, l[:, None], x.T, l[None, :], T + T.T, f32(gscale) * f32(inv_tau) / M, np.eye(M, dtype=bool))
    return {"W": W, "W_bound": b, "P1": P1, "P2": P2}


def coeff_rect_ref(S, lse_local, lse_all, row0: int, inv_tau: float, gscale: float = 1.0) -> dict:
    """The rectangular W [Ml, Mg] (the kernel's own statement: S_ij in both exponentials, 2 [j = p(i)])."""
    Ml, Mg = len(lse_local), len(lse_all)
    x = _x(np.asarray(S)[:Ml], Mg, inv_tau)
    ll, la = np.asarray(lse_local, dtype=F64), np.asarray(lse_all, dtype=F64)
    i = np.arange(Ml)
    ind = np.zeros((Ml, Mg))
    ind[i, positives(Ml, row0)] = 2.0
    zero = np.zeros((Ml, Mg), dtype=bool)
    zero[i, row0 + i] = True
    W, b, P1, P2 = _w(x, ll[:, None], x, la[None, :], ind, f32(gscale) * f32(inv_tau) / Ml, zero)
    xs = np.where(zero, 0.0, x)                                          # what the shared statement is given where nothing may be read
    with np.errstate(all="ignore"):
        same = DPO.coeff_rect(xs, ll, la, row0, Ml // 2, 1.0 / f32(inv_tau), f32(gscale))
    assert np.allclose(same, W, rtol=1e-12, atol=1e-300), "coeff_rect_ref left the statement of tests/_ntxent_dp_oracle.py"
    return {"W": W, "W_bound": b, "P1": P1, "P2": P2}


def gemm_rel(K: int) -> float:
    """The accumulation and combining terms of oracle/gemm_bounds.py for an fp32 product over K, relative to sum |a| |b|."""
    return gamma(K) + (math.ceil(K / 256) + GEMM_EPI_OPS) * U


def e2e_ref(z, inv_tau: float, rect: bool = False) -> dict:
    """ops.ntxent_fwd / ntxent_bwd on fp32 rows z [M, D] against _ntxent_oracle.ntxent at the temperature 1 / fl32(inv_tau) the kernels
    are handed (and the clamp fl32(1e-12)): loss and dz in float64 with bounds carried a priori through the chain (A = |zh|, all in float64 on z):
        zh, norm      koleo_bounds.normalize_ref: e_zh, e_n
        S             e_S = gemm_rel(D) A A^T + e_zh A^T + A e_zh^T;  e_x = inv_tau e_S
        lse           rows_ref's bound + max_j e_x_ij (a log-sum-exp is 1-Lipschitz in the sup norm)
        loss          mean(e_lse_i + e_x_ip + (ROW_OPS + 2) u (|lse| + |x_ip|)) + (M + 2 + 2) u mean |row_loss|  (the chain, the division,
                      and under rect the host's division by Mg)
        W             coeff's own bound + scale (dP_ij + dP_ji), dP_ij = P_ij expm1(e_x_ij + e_lse_i).  The rectangular form reads
                      S_ij where P_ji is meant: |S_ij - S_ji| inv_tau P <= 2 e_x_ij P_ji, both within the GEMM bound: added under rect
        dzh = W zh    e_g = e_W A + |W| e_zh + gemm_rel(M) |W| A
        dz            koleo_bounds.normalize_bwd_ref's bound + the formula's first-order response to e_g, e_zh and e_n:
                      (e_g + e_zh |dot| + |zh| sum (|zh| e_g + |g| e_zh)) / n + |dz| e_n / n;   clamped rows: e_g / eps"""
    z = np.asarray(z, dtype=F32)
    M, D = z.shape
    it = f32(inv_tau)
    eps = f32(NX.EPS)                                                    # the clamp as the kernels are handed it
    loss, dz = NX.ntxent(z, 1.0 / it, eps)
    nr = normalize_ref(z)
    zh, n = NX.normalize(z, eps)
    A, e_zh, e_n = np.abs(zh), nr["xh_bound"], nr["norm_bound"]
    e_x = it * (gemm_rel(D) * (A @ A.T) + e_zh @ A.T + A @ e_zh.T)
    S = zh @ zh.T
    r = rows_ref(S, it)
    off = ~np.eye(M, dtype=bool)
    e_lse = r["lse_bound"] + np.where(off, e_x, 0.0).max(1)
    i, pos = np.arange(M), positives(M)
    xp = S[i, pos] * it
    e_row = e_lse + e_x[i, pos] + (ROW_OPS + 2) * U * (np.abs(r["lse"]) + np.abs(xp))
    loss_bound = e_row.mean() + (M + 2 + 2) * U * np.abs(r["row_loss"]).mean() + TINY
    c = coeff_ref(S, r["lse"], it, 1.0)
    scale = it / M
    dP = c["P1"] * np.expm1(e_x + e_lse[:, None])
    e_W = c["W_bound"] + scale * (dP + dP.T) + (scale * 2.0 * e_x * c["P2"] if rect else 0.0)
    W = c["W"]
    g = W @ zh
    e_g = e_W @ A + np.abs(W) @ e_zh + gemm_rel(M) * (np.abs(W) @ A)
    ref, b = normalize_bwd_ref(g, zh, n, vec=D % 4 == 0)
    dot = (g * zh).sum(1, keepdims=True)
    e_dot = (A * e_g + np.abs(g) * e_zh).sum(1, keepdims=True)
    cl = (n < eps)[:, None]
    nn = np.where(cl, 1.0, n[:, None])
    carried = np.where(cl, e_g / eps, (e_g + e_zh * np.abs(dot) + A * e_dot) / nn + np.abs(ref) * (e_n[:, None] / nn))
    assert np.allclose(ref, dz, rtol=1e-9, atol=1e-300)
    return {"loss": loss, "loss_bound": loss_bound, "dz": dz, "dz_bound": b + carried + TINY}


# ------------------------------------------------------------------------------------------ the kernels' order in NumPy float32
def _block_sum(lanes: np.ndarray) -> np.ndarray:
    """block_sum of csrc/common.h on [rows, 256] fp32: the xor butterfly inside each wave of 64, then the four cells onto 0 in order."""
    v = lanes.reshape(-1, THREADS // 64, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    t = np.zeros(v.shape[0], dtype=F32)
    for w in range(THREADS // 64):
        t = t + v[:, w, 0]
    return t


def _pos(i, Ml: int, row0: int, mutant: Optional[str]):
    p = positives(Ml, row0)[i]
    if mutant == "pos_wrap_off_by_one":
        p = np.where(i == Ml // 2, row0 + (1 % Ml), p)                   # the first wrapped row lands one row off
    return p


def emulate_rows(S, lds: int, Ml: int, Mg: int, row0: int, inv_tau: float, divisor: float, mutant: Optional[str] = None):
    """ntxent_rows(_rect)_kernel + ntxent_sum_kernel on the padded S [Ml, lds] -> (lse, row_loss, out) in fp32."""
    S = np.asarray(S, dtype=F32).reshape(Ml, lds)
    with np.errstate(all="ignore"):
        x = S[:, :Mg] * F32(inv_tau)
        i, j = np.arange(Ml), np.arange(Mg)
        dg = i if mutant == "rect_row0_ignored" else row0 + i
        keep = j[None, :] != dg[:, None]
        if mutant == "diag_included":
            keep[:] = True
        if mutant == "last_col_dropped":
            keep[:, Mg - 1] = False
        if mutant == "second_stride_dropped":
            keep[:, THREADS:] = False
        mx = np.fmax.reduce(np.where(keep, x, -np.inf), axis=1, initial=-np.inf).astype(F32)       # fmaxf passes over a NaN
        e = np.where(keep, np.exp(x - mx[:, None]), F32(0)).astype(F32)
        trips = math.ceil(Mg / THREADS)
        e = np.concatenate([e, np.zeros((Ml, trips * THREADS - Mg), dtype=F32)], axis=1)
        lanes = np.zeros((Ml, THREADS), dtype=F32)
        for k in range(trips):
            lanes = lanes + e[:, k * THREADS:(k + 1) * THREADS]
        lse = (mx + np.log(_block_sum(lanes))).astype(F32)
        row_loss = (lse - x[i, _pos(i, Ml, row0, mutant)]).astype(F32)
        a = F32(0)
        for base in range(0, Ml, SUM_CHUNK):
            if base and mutant == "sum_second_pass_dropped":
                break
            for t in range(base, min(base + SUM_CHUNK, Ml)):
                a = F32(a + row_loss[t])
        return lse, row_loss, F32(a / F32(divisor))


def emulate_coeff(S, lds: int, lse, M: int, inv_tau: float, gscale: float, ldw: int, mutant: Optional[str] = None) -> np.ndarray:
    """ntxent_coeff_kernel -> the flat W buffer as a launch leaves it: M ldw floats and a tail of TILE ldw more, CANARY where nothing
    was written.  The mirror term is what the LDS tile holds: S[j0 + r][i0 + c], zero outside the matrix."""
    Sf = np.concatenate([np.asarray(S, dtype=F32).reshape(-1), np.full(1, np.nan, dtype=F32)])
    lse = np.asarray(lse, dtype=F32)
    it, half = F32(inv_tau), M // 2
    scale = F32(F32(gscale) * it) if mutant == "scale_without_M" else F32(F32(F32(gscale) * it) / F32(M))
    tiles = math.ceil(M / TILE)
    cols = tiles * TILE if mutant == "mirror_oob_not_zeroed_then_used" else M
    i, j = np.arange(M)[:, None], np.arange(cols)[None, :]

    def load(r, c, zero_outside):
        v = Sf[np.minimum(r * lds + c, Sf.size - 1)]
        return np.where((r < M) & (c < M), v, F32(0)) if zero_outside else v

    with np.errstate(all="ignore"):
        own = load(i, j, False)
        if mutant == "mirror_not_transposed":
            i0, j0 = i - i % TILE, j - j % TILE
            mir = load(j0 + i % TILE, i0 + j % TILE, True)               # mir[r][tx] where mir[tx][r] is meant
        else:
            mir = load(j, i, mutant != "mirror_oob_not_zeroed_then_used")
        lj = lse[np.minimum(j, M - 1)]
        w = np.exp(own * it - lse[:M, None]) + np.exp(mir * it - (lse[:M, None] if mutant == "lse_i_for_lse_j" else lj))
        pi, pj = _pos(i, M, 0, mutant), _pos(np.minimum(j, M - 1), M, 0, mutant)
        ind = (j == pi).astype(F32) + (F32(0) if mutant == "pair_counted_once" else (i == pj).astype(F32))
        w = ((w - ind) * scale).astype(F32)
        if mutant != "diag_included":
            w = np.where(i == j, F32(0), w)
    out = np.full((M + TILE) * ldw, CANARY, dtype=F32)
    for b0 in range(0, M, TILE):                                         # a row of tiles at a time: the ragged tile's stray columns land
        rows = np.arange(b0, min(b0 + TILE, M))                          # on the next rows after their own tiles wrote them
        out[(rows[:, None] * ldw + np.arange(M)[None, :]).reshape(-1)] = w[rows, :M].reshape(-1)
        if cols > M:
            out[(rows[:, None] * ldw + np.arange(M, cols)[None, :]).reshape(-1)] = w[rows, M:].reshape(-1)
    return out


def emulate_coeff_rect(S, lds: int, lse_local, lse_all, Ml: int, Mg: int, row0: int, inv_tau: float, gscale: float, ldw: int,
                       mutant: Optional[str] = None) -> np.ndarray:
    """ntxent_coeff_rect_kernel -> the flat W buffer [Ml ldw], CANARY where nothing was written."""
    S = np.asarray(S, dtype=F32).reshape(Ml, lds)
    it = F32(inv_tau)
    scale = F32(F32(F32(gscale) * it) / F32(Ml))
    i, j = np.arange(Ml)[:, None], np.arange(Mg)[None, :]
    with np.errstate(all="ignore"):
        s = S[:, :Mg] * it
        w = np.exp(s - np.asarray(lse_local, dtype=F32)[:, None]) + np.exp(s - np.asarray(lse_all, dtype=F32)[None, :])
        w = w - np.where(j == _pos(i, Ml, row0, mutant), F32(1 if mutant == "rect_pair_1_not_2" else 2), F32(0))
        w = np.where(j == (i if mutant == "rect_row0_ignored" else row0 + i), F32(0), (w * scale).astype(F32))
    out = np.full((Ml, ldw), CANARY, dtype=F32)
    out[:, :Mg] = w
    return out.reshape(-1)


def split_w(flat, rows: int, cols: int, ldw: int):
    """A flat W buffer -> (the [rows, cols] payload, True if every padding column and every element past the last row is CANARY)."""
    flat = np.asarray(flat, dtype=F32)
    body = flat[:rows * ldw].reshape(rows, ldw)
    can = np.array([CANARY]).view(np.uint32)[0]
    clean = bool((body[:, cols:].view(np.uint32) == can).all() and (flat[rows * ldw:].view(np.uint32) == can).all())
    return body[:, :cols], clean


def lse_all_for(S_glob, Ml: int, inv_tau: float) -> np.ndarray:
    """A gathered lse [Mg] for the kernel-level rectangular cases: the float64 lse of every rank's block, moved by 0.25 sin(j) so that
    no entry equals the local lse the kernel is handed beside it."""
    Mg = S_glob.shape[0]
    parts = [rows_ref(poison(S_glob[r0:r0 + Ml], r0), inv_tau, Mg, r0)["lse"] for r0 in range(0, Mg, Ml)]
    return (np.concatenate(parts) + 0.25 * np.sin(np.arange(Mg))).astype(F32)


def shard_maps(Ml: int, world: int):
    """g [world, Ml]: the row of the global batch [z1 of all ranks; z2 of all ranks] that local row i of rank r is."""
    Bl, Bg = Ml // 2, Ml * world // 2
    i = np.arange(Ml)
    return np.stack([np.where(i < Bl, r * Bl + i, Bg + r * Bl + (i - Bl)) for r in range(world)])
