"""Float64 restatement of the LoRA products of include/dinox.h (csrc/lora.hip), the dropout hash, and a-priori elementwise bounds.

Matrices are in their mathematical orientation here (A [r,K], B [N,r]); the storage layouts are the device's business.
Bounds, in the manner of oracle/gemm_bounds.py (u = 2^-24): a chain or tree of n fp32 fma / add steps over terms a_i b_i lands within
gamma_n sum |a_i b_i| of the exact sum, gamma_n = n u / (1 - n u), whatever the order; an input that itself carries an error e adds
sum e |b|; every further fp32 multiply or add adds u times the magnitudes it touches; a bf16 store adds half a bf16 ulp.
"""
from __future__ import annotations

import math

import numpy as np

from oracle.gemm_bounds import U32, half_ulp_bf16

CHUNK = 128                                   # csrc/lora.hip LORA_GRAD_CHUNK
M32 = 0xFFFFFFFF


def gam(n: int) -> float:
    return n * U32 / (1.0 - n * U32)


# ------------------------------------------------------------------------------------------ dropout hash (uint32 arithmetic)
def mix(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x21F0AAAD)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x735A2D97)) & M32
    x ^= x >> np.uint64(15)
    return x


def dropout_key(seed: int, offset: int) -> int:
    seed, offset = seed & (2 ** 64 - 1), offset & (2 ** 64 - 1)
    ks = int(mix((seed & M32) ^ int(mix(((seed >> 32) + 0x9E3779B9) & M32))))
    return int(mix((offset & M32) ^ int(mix(((offset >> 32) + ks) & M32))))


def keep_mask(n: int, p: float, seed: int, offset: int, start: int = 0) -> np.ndarray:
    """keep(i) for i in [start, start + n): bool."""
    p32 = float(np.float32(p))
    thr = int(math.ceil(p32 * 16777216.0))
    i = np.arange(start, start + n, dtype=np.uint64)
    key = np.uint64(dropout_key(seed, offset))
    h = mix((i & np.uint64(M32)) ^ mix(((i >> np.uint64(32)) + key) & np.uint64(M32)))
    return (h >> np.uint64(8)) >= np.uint64(thr)


def dropout(x: np.ndarray, p: float, seed: int, offset: int, bf16_out: bool):
    """-> (xl, e_xl): x keep / (1 - p) over the flat index, and the error of the device's fp32 scale (1 / (1 - p) and the product:
    4 u) plus the bf16 store."""
    if p == 0.0:
        return x, np.zeros_like(x)
    p32 = float(np.float32(p))
    keep = keep_mask(x.size, p, seed, offset).reshape(x.shape)
    xl = np.where(keep, x / (1.0 - p32), 0.0)
    e = 4 * U32 * np.abs(xl)
    if bf16_out:
        e = e + np.where(keep, half_ulp_bf16(np.abs(xl) + e), 0.0)
    return xl, e


# ------------------------------------------------------------------------------------------ the products, each with its bound
def down(x, S, e_x=None):
    """u = x S^T (x [M,K], S [r,K]) -> (u, e_u)."""
    K = x.shape[1]
    u = x @ S.T
    e = gam(K + 8) * (np.abs(x) @ np.abs(S).T)
    if e_x is not None:
        e = e + e_x @ np.abs(S).T
    return u, e


def up(u, S, s, res=None, e_u=None):
    """t = s u S^T (+ res) (u [M,r], S [N,r]) -> (t, e_t)."""
    r = u.shape[1]
    e_u = np.zeros_like(u) if e_u is None else e_u
    v = s * (u @ S.T)
    T = (np.abs(u) + e_u) @ np.abs(S).T
    e = abs(s) * (e_u @ np.abs(S).T + gam(r + 2) * T) + 2 * U32 * np.abs(v)
    if res is not None:
        e = e + 2 * U32 * (np.abs(v) + np.abs(res))
        v = v + res
    return v, e


def grad(xl, dy, A, B, s, e_xl=None):
    """-> (dA, e_dA, dB, e_dB): dA = s v^T xl, dB = s dy^T u with u = xl A^T, v = dy B."""
    M = xl.shape[0]
    n = min(M, CHUNK) + (M + CHUNK - 1) // CHUNK + 2
    e_xl = np.zeros_like(xl) if e_xl is None else e_xl
    u, e_u = down(xl, A, e_xl)
    v, e_v = down(dy, B.T)
    dA = s * (v.T @ xl)
    e_dA = abs(s) * (e_v.T @ np.abs(xl) + (np.abs(v) + e_v).T @ e_xl + gam(n) * ((np.abs(v) + e_v).T @ (np.abs(xl) + e_xl))) + 2 * U32 * np.abs(dA)
    dB = s * (dy.T @ u)
    e_dB = abs(s) * (np.abs(dy).T @ e_u + gam(n) * (np.abs(dy).T @ (np.abs(u) + e_u))) + 2 * U32 * np.abs(dB)
    return dA, e_dA, dB, e_dB


def merge(W, A, B, s, sign):
    return up(B, A.T, sign * s, res=W)


def base_product(x, W, b, K_ops=None):
    """x W^T + b with the accumulation and combining terms of oracle/gemm_bounds.reference -> (v, e)."""
    K = x.shape[1]
    S = x @ W.T
    T = np.abs(x) @ np.abs(W).T
    bias = np.zeros((1, W.shape[0])) if b is None else b[None, :]
    comb = (math.ceil(K / 256) + 4) * U32
    return S + bias, gam(K) * T + comb * (T + np.abs(bias))


def rounded(ref, err, bf16_out: bool):
    return err + half_ulp_bf16(np.abs(ref) + err) if bf16_out else err


def lora_linear(x, W, b, A, B, s, residual=None, p=0.0, seed=0, offset=0, bf16_ops=False, bf16_out=False):
    """Forward of one wrapped layer on the operand VALUES (x and W already rounded to the mode's dtype) -> (y, e_y, xl, e_xl)."""
    xl, e_xl = dropout(x, p, seed, offset, bf16_ops)
    u, e_u = down(xl, A, e_xl)
    t, e_t = up(u, B, s, res=residual, e_u=e_u)
    v, e_v = base_product(x, W, b)
    y = v + t
    e = e_v + e_t + 2 * U32 * (np.abs(v) + np.abs(t))
    return y, rounded(y, e, bf16_out), xl, e_xl


def lora_linear_bwd(x, xl, e_xl, dy, W, A, B, s, p=0.0, seed=0, offset=0, bf16_out=False):
    """-> {"dx": (ref, bound), "dA": ..., "dB": ...} for dy in the mode's operand dtype."""
    v, e_v = down(dy, B.T)
    t, e_t = up(v, A.T, s, e_u=e_v)
    if p > 0.0:
        t, e_d = dropout(t, p, seed, offset, False)
        keep = keep_mask(t.size, p, seed, offset).reshape(t.shape)
        e_t = np.where(keep, e_t / (1.0 - float(np.float32(p))), 0.0) + e_d
    g, e_g = base_product(dy, W.T, None)
    dx = g + t
    e_dx = rounded(dx, e_g + e_t + 2 * U32 * (np.abs(g) + np.abs(t)), bf16_out)
    dA, e_dA, dB, e_dB = grad(xl, dy, A, B, s, e_xl)
    return {"dx": (dx, e_dx), "dA": (dA, e_dA), "dB": (dB, e_dB)}


# ------------------------------------------------------------------------------------------ fp32 emulation in the kernels' order
# What csrc/lora.hip states about its arithmetic, evaluated in NumPy float32 so that the bounds above can be judged without a device
# (tests/test_lora_paths_cpu.py): the emulation must lie inside them, a planted defect (MUTANTS) must not.
TILE = 128                                    # LT_COLS


def _fma(a, b, c):
    """fl32(a b + c), elementwise with broadcasting.  The product of two fp32 values is exact in float64; the sum is rounded to 53 bits
    and then to 24, which differs from the instruction's single rounding only where the 53-bit sum lands on a 24-bit tie -- an fp32
    rounding either way, so the a-priori bounds cover both."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def mfma_order(n: int):
    """The order in which one accumulator of v_mfma_f32_32x32x2_f32 meets the contraction index in dot_tile and outer_tile: per step g of
    8, instruction i = 0 .. 3 takes k = 8 g + i from the lanes h = 0 and k = 8 g + 4 + i from h = 1 (`kq = 8 * g + 4 * h`, then `a[i]`, in
    dot_tile; `m = 8 * g + 4 * h + i` in outer_tile), the h = 0 operand first."""
    return [k for g in range(-(-n // 8)) for i in range(4) for h in range(2) for k in (8 * g + 4 * h + i,) if k < n]


def emulate_down(x, S, mutant=None):
    """u = x S^T as chunk_dot forms it: one accumulator per (row, j), the tiles of 128 columns in ascending c0 (the `for (c0 ...)` loop of
    chunk_dot), inside a tile mfma_order; columns past C are zeros in Xs and in b and add nothing.  Rows are independent, so the 128-row
    chunks of lora_down_kernel do not show in the values."""
    x, S = np.asarray(x, np.float32), np.asarray(S, np.float32)
    (M, K), r = x.shape, S.shape[0]
    k_end = K - K % TILE if mutant == "ragged_tile_dropped" else K
    acc = np.zeros((M, r), np.float32)
    for k in mfma_order(K):                          # (128 is a multiple of 8: the order over the whole row is the order tile by tile)
        if k < k_end:
            acc = _fma(x[:, k:k + 1], S[None, :, k], acc)
    if mutant == "rank_ge32_dropped":
        acc[:, 32:] = 0.0
    return acc


def emulate_up(u, S, s, res=None, mutant=None):
    """t = s u S^T (+ res) as lora_up_kernel forms it: per element one fma chain in ascending j (both j loops: the r4 loop takes j, j + 1,
    j + 2, j + 3 in that order), then `s * acc` rounded, then `+ res` rounded.  The mutant "clamped_row_past_M" returns M + 1 rows: the
    copy of row M - 1 that `urow` clamps to, stored where the `m0 + m >= M` break should have stopped it."""
    u, S = np.asarray(u, np.float32), np.asarray(S, np.float32)
    (M, r), N = u.shape, S.shape[0]
    acc = np.zeros((M, N), np.float32)
    for j in range(r - r % 4 if mutant == "up_remainder_dropped" else r):
        acc = _fma(u[:, j:j + 1], S[None, :, j], acc)
    t = acc if mutant == "s_ignored" else np.float32(s) * acc
    if res is not None and mutant != "res_ignored":
        t = t + np.asarray(res, np.float32)
    if mutant == "clamped_row_past_M" and M % 4:
        t = np.concatenate([t, t[-1:]], axis=0)
    return t


def emulate_merge(W, A, B, s, sign, mutant=None):
    """dinox_lora_merge is lora_up with B as the rows, A as the small matrix, (float)sign * s and W as res."""
    return emulate_up(B, np.asarray(A).T, float(sign) * float(np.float32(s)), res=W, mutant=mutant)


def emulate_grad(xl, dy, A, B, s, mutant=None):
    """dA, dB as lora_grad_partial_kernel + lora_grad_reduce_kernel form them.  Per 128-row chunk: u and v by chunk_dot over all 128 rows
    (rows past the chunk's end are zeros), then per output element one chain over the chunk's rows in mfma_order (outer_tile), unscaled,
    into ws; the reduce kernel adds the chunks' partials in ascending chunk order (`for (c = 0; c < nchunks; ++c) acc += ...`) and
    multiplies by s once."""
    xl, dy, A, B = (np.asarray(a, np.float32) for a in (xl, dy, A, B))
    (M, K), N, r = xl.shape, dy.shape[1], A.shape[0]
    sub = mutant if mutant in ("ragged_tile_dropped", "rank_ge32_dropped") else None
    parts = []
    for row0 in range(0, M, CHUNK):
        rows = min(CHUNK, M - row0)
        X, D = np.zeros((CHUNK, K), np.float32), np.zeros((CHUNK, N), np.float32)
        X[:rows], D[:rows] = xl[row0:row0 + rows], dy[row0:row0 + rows]
        live = rows
        if mutant == "rows_past_chunk_from_next" and rows < CHUNK:       # the rows that follow in memory; past the last row the operand wraps
            idx = (row0 + np.arange(rows, CHUNK)) % M
            X[rows:], D[rows:] = xl[idx], dy[idx]
            live = CHUNK
        u, v = emulate_down(X, A, sub), emulate_down(D, B.T, sub)
        pA, pB = np.zeros((r, K), np.float32), np.zeros((N, r), np.float32)
        for m in mfma_order(CHUNK):
            if m < live:                                                   # a zero row adds nothing
                pA = _fma(v[m][:, None], X[m][None, :], pA)
                pB = _fma(D[m][:, None], u[m][None, :], pB)
        if mutant == "ragged_tile_dropped":                                # pass 2 as well: the columns of a ragged last tile are never stored
            pA[:, K - K % TILE:] = 0.0
            pB[N - N % TILE:, :] = 0.0
        if mutant == "s_per_chunk_and_end":
            pA, pB = np.float32(s) * pA, np.float32(s) * pB
        parts.append((pA, pB))
    if mutant == "last_chunk_left_out":
        parts = parts[:-1]
    accA, accB = np.zeros((r, K), np.float32), np.zeros((N, r), np.float32)
    for pA, pB in parts:
        accA, accB = accA + pA, accB + pB
    if mutant == "s_ignored":
        return accA, accB
    return np.float32(s) * accA, np.float32(s) * accB


# planted defect -> the entries whose emulation it changes
MUTANTS = {
    "ragged_tile_dropped": ("down", "grad"),           # the columns of a last tile that is not full are left out
    "up_remainder_dropped": ("up", "merge"),           # the r % 4 terms after the last whole group of four
    "rank_ge32_dropped": ("down", "grad"),             # the second 32-wide rank block
    "rows_past_chunk_from_next": ("grad",),            # rows past the chunk's end read from memory instead of being zero
    "last_chunk_left_out": ("grad",),                  # the reduction stops one chunk early
    "s_ignored": ("up", "grad", "merge"),
    "s_per_chunk_and_end": ("grad",),                  # s applied to every partial and again to the sum
    "res_ignored": ("up", "merge"),
    "clamped_row_past_M": ("up",),                     # a canary hit, not a value error
}


def reference(c, o):
    """{output name: (float64 reference, elementwise bound)} of one case of tests/_lora_paths_cases.py on the operands ``o``: the products and
    bounds above, unchanged."""
    d = {k: np.asarray(v, np.float64) for k, v in o.items()}
    e = c["entry"]
    if e == "down":
        return {"u": down(d["x"], d["S"])}
    if e == "up":
        return {"t": up(d["u"], d["S"], c["s"], None if c["res"] == "none" else d["res"])}
    if e == "grad":
        dA, eA, dB, eB = grad(d["xl"], d["dy"], d["A"], d["B"], c["s"])
        return {"dA": (dA, eA), "dB": (dB, eB)}
    return {"out": merge(d["W"], d["A"], d["B"], c["s"], c["sign"])}


def emulate(c, o, mutant=None):
    e = c["entry"]
    if e == "down":
        return {"u": emulate_down(o["x"], o["S"], mutant)}
    if e == "up":
        return {"t": emulate_up(o["u"], o["S"], c["s"], None if c["res"] == "none" else o["res"], mutant)}
    if e == "grad":
        dA, dB = emulate_grad(o["xl"], o["dy"], o["A"], o["B"], c["s"], mutant)
        return {"dA": dA, "dB": dB}
    return {"out": emulate_merge(o["W"], o["A"], o["B"], c["s"], c["sign"], mutant)}


def chain_length(c, name):
    """The longest fma chain behind one element of output ``name`` (the condition for short chains of tests/test_gemm_contract_cpu.py)."""
    rows = min(c["M"], CHUNK)
    return {"u": c["K"], "t": c["r"], "out": c["r"], "dA": max(c["N"], rows), "dB": max(c["K"], rows)}[name]


GUARD = 512                                   # canary words after every emulated output


def check(got, ref, bound):
    """One output against its reference inside a guarded buffer: ``got`` is copied flat into ref.size + GUARD words of the fp32 canary, so
    an output with more elements than it should have lands in the guard.  -> dict(compared, ratio, nan, canary, unwritten)."""
    from oracle.gemm_bounds import CANARY_F32
    canary = np.array([CANARY_F32], np.uint32).view(np.float32)[0]
    buf = np.full(ref.size + GUARD, canary, np.float32)
    flat = np.asarray(got, np.float32).reshape(-1)
    assert flat.size <= buf.size
    buf[:flat.size] = flat
    body = buf[:ref.size].astype(np.float64).reshape(ref.shape)
    bits = buf.view(np.uint32)
    err = np.abs(body - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / bound)                         # a zero bound admits a zero error and nothing else
    nan = int(np.isnan(body).sum())
    return dict(compared=int(err.size), ratio=float(np.nanmax(q)) if q.size else 0.0, nan=nan,
                canary=int((bits[ref.size:] != CANARY_F32).sum()), unwritten=int((bits[:ref.size] == CANARY_F32).sum()))
