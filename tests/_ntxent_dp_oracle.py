"""float64 NumPy restatement of the SHARDED NT-Xent formulas (data-parallel SimCLR) -- test infrastructure, not a compute path.

``world`` ranks; rank r holds Ml = 2 Bl rows z_r = [z1_r; z2_r].  What each rank computes (csrc/ntxent.hip, the rectangular kernels;
ops.ntxent_fwd(group=) / ntxent_bwd):

    zh_r    = z_r / max(||z_r||, eps)                          per row
    zh_all  = [zh_0; ...; zh_{world-1}]                        all-gather, Mg = world Ml rows, rank r's block at row0 = r Ml
    s       = zh_r zh_all^T / tau                              [Ml, Mg]
    lse_i   = logsumexp_{j != row0 + i} s_ij                   the excluded column is the row's global index
    loss_i  = lse_i - s_{i, p(i)},   p(i) = row0 + (i + Bl) mod Ml
    L       = (sum over every rank's rows of loss_i) / Mg      the global mean
    lse_all = [lse of rank 0; ...]                             all-gather
    W_ij    = (exp(s_ij - lse_i) + exp(s_ij - lse_all[j]) - 2 [j = p(i)]) / (Ml tau),   W_{i, row0 + i} = 0
    dzh_r   = W zh_all
    dz_r    = (dzh - zh (zh . dzh)) / ||z||   (dzh / eps where ||z|| < eps)

dz_r is ``world`` times dL/dz_r (the gradient convention of the engine: the ranks' parameter gradients are summed and AdamW applies
1 / world).  tests/test_simclr_dp_cpu.py holds it against _ntxent_oracle.ntxent on the permuted global batch [z1 of all ranks; z2 of all
ranks].
"""
from __future__ import annotations

import numpy as np

from _ntxent_oracle import EPS, normalize


def rows_rect(s: np.ndarray, row0: int, Bl: int):
    """s [Ml, Mg] (already divided by tau) -> (lse [Ml], row_loss [Ml])."""
    Ml, Mg = s.shape
    i = np.arange(Ml)
    off = np.ones((Ml, Mg), dtype=bool)
    off[i, row0 + i] = False
    sm = np.where(off, s, -np.inf)
    mx = sm.max(1)
    lse = mx + np.log(np.where(off, np.exp(sm - mx[:, None]), 0.0).sum(1))
    pos = row0 + (i + Bl) % Ml
    return lse, lse - s[i, pos]


def coeff_rect(s: np.ndarray, lse_local: np.ndarray, lse_all: np.ndarray, row0: int, Bl: int, temperature: float, gscale: float = 1.0):
    """W [Ml, Mg] of the module docstring."""
    Ml, Mg = s.shape
    i = np.arange(Ml)
    W = np.exp(s - lse_local[:, None]) + np.exp(s - lse_all[None, :])
    W[i, row0 + (i + Bl) % Ml] -= 2.0
    W *= gscale / (Ml * temperature)
    W[i, row0 + i] = 0.0
    return W


def normalize_bwd(dzh: np.ndarray, zh: np.ndarray, n: np.ndarray, eps: float = EPS):
    clamped = n < eps
    dot = np.where(clamped, 0.0, (dzh * zh).sum(1))
    return (dzh - dot[:, None] * zh) / np.where(clamped, eps, n)[:, None]


def ntxent_sharded(shards, temperature: float = 0.1, eps: float = EPS):
    """shards: one [2 Bl, D] array [z1_r; z2_r] per rank -> (global mean loss, [dz_r per rank], [lse_r per rank]) in float64."""
    shards = [np.asarray(z, dtype=np.float64) for z in shards]
    Ml = shards[0].shape[0]
    if Ml < 2 or Ml % 2 or any(z.shape != shards[0].shape for z in shards):
        raise ValueError("every rank holds the same even number of rows")
    Bl, Mg = Ml // 2, len(shards) * Ml
    unit = [normalize(z, eps) for z in shards]
    zh_all = np.concatenate([zh for zh, _ in unit], 0)
    s = [zh @ zh_all.T / temperature for zh, _ in unit]
    fwd = [rows_rect(s[r], r * Ml, Bl) for r in range(len(shards))]
    total = 0.0
    for _, row_loss in fwd:                       # rank order, as the gathered partial sums are added
        total += row_loss.sum()
    lse_all = np.concatenate([lse for lse, _ in fwd])
    dz = []
    for r, (zh, n) in enumerate(unit):
        W = coeff_rect(s[r], fwd[r][0], lse_all, r * Ml, Bl, temperature)
        dz.append(normalize_bwd(W @ zh_all, zh, n, eps))
    return total / Mg, dz, [lse for lse, _ in fwd]


def split(z1: np.ndarray, z2: np.ndarray, world: int):
    """The global views z1, z2 [B, D] -> one [z1_r; z2_r] per rank (contiguous sample shards, dp.shard_range)."""
    B = z1.shape[0]
    assert B % world == 0
    Bl = B // world
    return [np.concatenate([z1[r * Bl:(r + 1) * Bl], z2[r * Bl:(r + 1) * Bl]], 0) for r in range(world)]


def unsplit(parts):
    """Per-rank [a1_r; a2_r] -> the global [a1 of all ranks; a2 of all ranks] (the inverse of ``split`` on row-shaped results)."""
    Bl = parts[0].shape[0] // 2
    return np.concatenate([p[:Bl] for p in parts] + [p[Bl:] for p in parts], 0)
