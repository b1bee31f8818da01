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
