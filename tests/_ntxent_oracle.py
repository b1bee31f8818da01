"""float64 NumPy restatement of the NT-Xent (SimCLR) loss and of its gradient -- test infrastructure, not a compute path.

Restates SimCLRLoss(temperature)(z1, z2) of the reference (scripts/phase5_big_run.py:776-813) on z = [z1; z2] (M = 2B rows):

    zh = z / max(||z||, eps)                                 F.normalize, eps = 1e-12
    s  = zh zh^T / tau, the diagonal excluded
    loss = mean_i ( logsumexp_{j != i} s_ij - s_{i p(i)} ),  p(i) = (i + B) mod 2B

and the closed-form gradient the kernels implement:

    W_ij  = (P_ij + P_ji - [j = p(i)] - [i = p(j)]) / (M tau),  P_ij = exp(s_ij - lse_i),  W_ii = 0
    dzh   = W zh
    dz    = (dzh - zh (zh . dzh)) / ||z||      where ||z|| >= eps
    dz    = dzh / eps                          where ||z|| <  eps  (torch's clamp_min passes no gradient to the norm there)

tests/golden/simclr_loss.npz holds what the reference's SimCLRLoss + autograd give for the same inputs; tests/test_simclr_cpu.py
compares the two.
"""
from __future__ import annotations

import numpy as np

EPS = 1e-12


def normalize(z: np.ndarray, eps: float = EPS):
    z = np.asarray(z, dtype=np.float64)
    n = np.sqrt((z * z).sum(1))
    return z / np.maximum(n, eps)[:, None], n


def ntxent(z: np.ndarray, temperature: float = 0.1, eps: float = EPS):
    """z [2B, D] -> (loss, dz [2B, D]) in float64."""
    z = np.asarray(z, dtype=np.float64)
    M = z.shape[0]
    if z.ndim != 2 or M < 2 or M % 2:
        raise ValueError(f"z must be [2B, D], got {z.shape}")
    B = M // 2
    zh, n = normalize(z, eps)
    s = zh @ zh.T / temperature
    off = ~np.eye(M, dtype=bool)
    sm = np.where(off, s, -np.inf)
    mx = sm.max(1)
    e = np.where(off, np.exp(sm - mx[:, None]), 0.0)
    lse = mx + np.log(e.sum(1))
    pos = (np.arange(M) + B) % M
    loss = float((lse - s[np.arange(M), pos]).mean())
    P = np.where(off, np.exp(sm - lse[:, None]), 0.0)
    T = np.zeros((M, M))
    T[np.arange(M), pos] = 1.0
    W = (P + P.T - T - T.T) / (M * temperature)
    dzh = W @ zh
    dot = (dzh * zh).sum(1)
    clamped = n < eps
    den = np.where(clamped, eps, n)
    dz = (dzh - np.where(clamped, 0.0, dot)[:, None] * zh) / den[:, None]
    return loss, dz


def simclr(z1: np.ndarray, z2: np.ndarray, temperature: float = 0.1):
    """(loss, dz1, dz2) of SimCLRLoss(temperature)(z1, z2)."""
    B = np.asarray(z1).shape[0]
    loss, dz = ntxent(np.concatenate([np.asarray(z1, np.float64), np.asarray(z2, np.float64)], 0), temperature)
    return loss, dz[:B], dz[B:]
