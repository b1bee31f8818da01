"""float64 oracle and a-priori elementwise bound for dinox_attention_rollout_step and the rollout chain (CPU, no GPU).

Step, on the ROUNDED inputs (bf16 or fp32 values taken exactly), with the full N x N softmax matrices P^h in float64:
    ref_j = r w_j + (1 - r) / heads * sum_h sum_i w_i P^h_ij

Bound, built only from the constants of oracle/attention_bounds.py, in the manner of tests/_attention_rows_oracle.py:
    rel_ih  = 2 eps_ih + LSE_SCORE A_ih + LSE_FLOOR + 2^-22      that file's per-row relative factor of one fp32 probability
                                                                 (A_ih = sc max_j sum_c |q_ic k_jc|, eps_ih = (d + 2) 2^-24 A_ih)
    |out_j - ref_j| <= (1 - r) / heads * sum_h sum_i |w_i| P^h_ij (rel_ih + (N + heads + 4) 2^-23)  +  r |w_j| 2^-23  +  2^-120
Derivation.  The kernel forms p_ij = expf(s - max) / sum in fp32 exactly as dinox_attention_rows does, so |p - P| <= rel_ih P (that
file's derivation; a p flushed to zero where float64 still holds a number below 2^-126 is the 2^-120 at the end, for weights of
ordinary size).  The column sum is one thread's chain acc = fma(w_i, p_ij, acc) over i = 0 .. N - 1: N roundings, each at most 2^-24
of a partial sum that never exceeds sum_i |w_i| p_ij in magnitude.  The fold adds the heads in order (heads - 1 roundings of
partial sums bounded by the sum of the magnitudes), multiplies by coef = (1 - r) / heads (two roundings in coef) inside one fma with
r w_j (one rounding for the product r w_j, one for the fma's result, which is at most r |w_j| plus the attention term in
magnitude).  To first order the attention term therefore carries (N + heads + 3) 2^-24 and r w_j carries 2 2^-24 = 2^-23; the bound
states (N + heads + 4) 2^-23, twice the first-order count, which covers the products of these factors with each other and with rel_ih
for every N the kernel takes ((1 + 2^-24)^4100 - 1 < 4100 2^-23).  Nothing is fitted to what a device returns.

Chain.  w_L = e_query, w_{l-1} = step_l(w_l): the row `query` of Ahat_L ... Ahat_1, Ahat_l = r I + (1 - r) mean_h P_l^h, which
rollout_oracle forms the long way (explicit N x N products).  With rho = the largest rel_ih + (N + heads + 4) 2^-23 over every block,
image, head and row, a step is within rho S(|w|) + 2^-120 of the exact step S(w) (r |w_j| 2^-23 <= rho r |w_j|), and S is linear and
monotone on non-negative vectors, so if |got_l - ref_l| <= c ref_l then |got_{l-1} - ref_{l-1}| <= (rho (1 + c) + c) ref_{l-1}:
    |got - ref| <= ((1 + rho)^L - 1) ref + L N 2^-120          after L steps, elementwise (chain_bound)
(the last term: a 2^-120 per element, carried through at most L steps whose columns sum to at most N).
"""
from __future__ import annotations

import math
from typing import Dict, Sequence

import torch

from oracle import attention_bounds as AB

TINY = 2.0 ** -120
ROUND = 2.0 ** -22
U32 = 2.0 ** -23


def softmax_matrices(qkv: torch.Tensor, heads: int):
    """Packed qkv [B, N, 3 heads d] -> float64 P [B, heads, N, N] and the per-row relative factor rel [B, heads, N]."""
    q, k, _ = AB.split_qkv(qkv, heads)                                    # [B, heads, N, d] float64
    d = q.shape[-1]
    s = q @ k.transpose(-1, -2) / math.sqrt(d)
    P = torch.exp(s - torch.logsumexp(s, -1, keepdim=True))
    A = (q.abs() @ k.abs().transpose(-1, -2)).amax(-1) / math.sqrt(d)     # [B, heads, N]
    eps = (d + 2) * 2.0 ** -24 * A
    return P, 2 * eps + AB.LSE_SCORE * A + AB.LSE_FLOOR + ROUND


def step_oracle(qkv: torch.Tensor, heads: int, w: torch.Tensor, residual: float) -> Dict[str, torch.Tensor]:
    """-> float64 "out" [B, N], its elementwise "bound" [B, N], and "rho": the largest relative factor of the bound's attention term."""
    P, rel = softmax_matrices(qkv, heads)
    N = P.shape[-1]
    wd = w.detach().double().cpu()
    assert wd.shape == (P.shape[0], N), (wd.shape, P.shape)
    r = float(residual)
    fac = rel + (N + heads + 4) * U32                                     # [B, heads, N]
    att = torch.einsum("bi,bhij->bj", wd, P) / heads
    out = r * wd + (1.0 - r) * att
    bound = (1.0 - r) / heads * torch.einsum("bi,bhi,bhij->bj", wd.abs(), fac, P) + r * wd.abs() * U32 + TINY
    return {"out": out, "bound": bound, "rho": float(fac.max())}


def head_mean_hat(qkv: torch.Tensor, heads: int, residual: float) -> torch.Tensor:
    """Ahat = r I + (1 - r) mean_h P^h, float64 [B, N, N]."""
    P, _ = softmax_matrices(qkv, heads)
    N = P.shape[-1]
    return float(residual) * torch.eye(N, dtype=torch.float64) + (1.0 - float(residual)) * P.mean(1)


def rollout_oracle(list_of_qkv: Sequence[torch.Tensor], heads: int, query: int, residual: float) -> torch.Tensor:
    """The long way round: the explicit product Ahat_L ... Ahat_1 of the blocks' matrices (list_of_qkv[0] is the first block) in
    float64, of which row `query` is returned, [B, N]."""
    R = None
    for qkv in list_of_qkv:
        Ahat = head_mean_hat(qkv, heads, residual)
        R = Ahat if R is None else Ahat @ R
    return R[:, query, :]


def chain_oracle(list_of_qkv: Sequence[torch.Tensor], heads: int, query: int, residual: float) -> Dict[str, torch.Tensor]:
    """What the code computes, in float64: w = e_query, then one step per block from the last one down.  -> "out" [B, N], "rho" (the
    largest per-step factor) and "bound" = chain_bound of it."""
    B, N = list_of_qkv[0].shape[0], list_of_qkv[0].shape[1]
    w = torch.zeros(B, N, dtype=torch.float64)
    w[:, query] = 1.0
    rho = 0.0
    for qkv in reversed(list(list_of_qkv)):
        st = step_oracle(qkv, heads, w, residual)
        w, rho = st["out"], max(rho, st["rho"])
    return {"out": w, "rho": rho, "bound": chain_bound(w, rho, len(list_of_qkv))}


def chain_bound(ref: torch.Tensor, rho: float, L: int) -> torch.Tensor:
    return ((1.0 + rho) ** L - 1.0) * ref.abs() + L * ref.shape[-1] * TINY


def check(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str) -> float:
    """Every element inside its bound, nothing left out; returns the largest err / bound."""
    return AB.check(got, ref, bound, what)[0]
