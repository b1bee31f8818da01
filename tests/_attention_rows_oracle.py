"""float64 oracle and a-priori elementwise bound for dinox_attention_rows (CPU, no GPU).

probs[b][h][r][j] = softmax_j(q_{i_r} . k_j / sqrt(d)) on the ROUNDED inputs (bf16 or fp32 values taken exactly), in float64.

Bound, built only from the constants of oracle/attention_bounds.py.  With A_i = sc max_j sum_c |q_ic k_jc| (sc = 1 / sqrt(d)):
    eps_i = (d + 2) 2^-24 A_i                 absolute error of an fp32 score: d fma roundings, the rounding of sc and of the product
    |p - p_ref| <= (2 eps_i + LSE_SCORE A_i + LSE_FLOOR + 2^-22) p_ref + 2^-120
the factor 2 eps_i covers the score and the row maximum it is subtracted from, LSE_SCORE A_i + LSE_FLOOR is the error of the
normaliser (lse_bound of that module: p = exp(s - lse)), 2^-22 the roundings of expf, of the sum's last bits and of the division,
and 2^-120 an fp32 result flushed to zero where float64 still holds a tiny number.
    |lse - ref| <= lse_bound(A, N)            as that module defines it (asserts that it stays below 1 / (2N))
    |sum_j p - 1| <= N 2^-23 + rel_i          rel_i = the relative factor above; N 2^-23: every p is within half an ulp(1) of a value
                                              whose exact sum the relative term bounds
"""
from __future__ import annotations

import math
from typing import Dict, Sequence

import torch

from oracle import attention_bounds as AB

TINY = 2.0 ** -120
ROUND = 2.0 ** -22


def rows_oracle(qkv: torch.Tensor, heads: int, query_idx: Sequence[int]) -> Dict[str, torch.Tensor]:
    """qkv packed [B, N, 3 heads d] (any float dtype, values taken exactly) -> float64 probs [B, heads, Q, N], lse [B, heads, Q], and
    their bounds p_bound (same shape as probs), lse_bound, rel [B, heads, Q] and the sum bound sum_bound [B, heads, Q]."""
    q, k, _ = AB.split_qkv(qkv, heads)                                    # [B, heads, N, d] float64
    N, d = q.shape[-2], q.shape[-1]
    idx = torch.as_tensor(list(query_idx), dtype=torch.long)
    qs = q[:, :, idx]                                                     # [B, heads, Q, d]
    s = qs @ k.transpose(-1, -2) / math.sqrt(d)                           # [B, heads, Q, N]
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    A = (qs.abs() @ k.abs().transpose(-1, -2)).amax(-1) / math.sqrt(d)    # [B, heads, Q]
    eps = (d + 2) * 2.0 ** -24 * A
    rel = 2 * eps + AB.LSE_SCORE * A + AB.LSE_FLOOR + ROUND
    return {"probs": p, "lse": lse, "A": A, "rel": rel, "p_bound": rel[..., None] * p + TINY, "lse_bound": AB.lse_bound(A, N),
            "sum_bound": N * 2.0 ** -23 + rel}


def full_softmax_rows(qkv: torch.Tensor, heads: int, query_idx: Sequence[int]) -> torch.Tensor:
    """The same rows the long way: torch.softmax of the FULL float64 N x N score matrix, then the query rows."""
    q, k, _ = AB.split_qkv(qkv, heads)
    s = q @ k.transpose(-1, -2) / math.sqrt(q.shape[-1])
    return torch.softmax(s, -1)[:, :, torch.as_tensor(list(query_idx), dtype=torch.long)]


def check_rows(probs: torch.Tensor, lse, ref: Dict[str, torch.Tensor], what: str) -> Dict[str, float]:
    """Every element of probs (and lse, when given) inside its bound, and every row sum inside the sum bound; nothing is left out.
    Returns the measured err / bound ratios."""
    out = {"p": AB.check(probs, ref["probs"], ref["p_bound"], what + " probs")[0]}
    sums = probs.detach().double().cpu().sum(-1)
    out["sum"] = AB.check(sums, torch.ones_like(sums), ref["sum_bound"], what + " row sum")[0]
    if lse is not None:
        out["lse"] = AB.check(lse, ref["lse"], ref["lse_bound"], what + " lse")[0]
    return out
