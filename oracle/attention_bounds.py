"""Adversarial softmax inputs and a-priori elementwise rounding bounds for the attention core (CPU, float64, no GPU).

The attention kernels (csrc/attention_bf16.hip, attention_flash.hip, attention_ref.hip, the fp32 product form of dinox/ops.py) document
one arithmetic: fp32 scores from exact bf16 products; P rounded to bf16 before P.V and P^T.dO; dS rounded to bf16 before dS.K and
dS^T.Q; fp32 accumulation; outputs rounded to bf16.  This module states, per output ELEMENT, how far that arithmetic can land from
float64 on the same rounded inputs, and supplies input families whose softmax is not the diffuse one of randn data: a row maximum
that keeps rising (or never moves), scores near +80, a dominant key in the ragged last tile, near-one-hot rows.

Layout: every per-head tensor here is [B, heads, N, d] (lse: [B, heads, N]), so an index reads (image, head, token, column).

Bound (U = unit roundoff: 2^-8 for bf16 -- 8 significant bits; fp32 mode replaces U by gamma = (N + d + 8) 2^-24):
    A_i   = sc max_j sum_c |q_ic k_jc|                    eps_i = (d + 2) 2^-24 A_i      (relative error of p from the fp32 score)
    |o   - ref| <= (2U + 2 eps_i + 2^-12) (P |V|)         one U for P, one for the output, 2^-12 for fp32 accumulation
    |lse - ref| <= 2^-19 A_i + LSE_FLOOR                  must stay below 1 / (2N): one dropped or doubled key of a uniform row shows
backward, against float64 GIVEN the kernel's own o and lse (delta = rowsum(dO o o_kernel): forward error is not counted twice):
    E          = U |dS| + 2^-18 P o (|dO| |V|^T + rowsum|dO o o|) + 2 eps_i |dS|
    |dV - ref| <= sum_i (2U + 2 eps_i + 2^-12) P_ij |dO_i|
    |dQ - ref| <= sc (E |K|) + U |dQ_ref|
    |dK - ref| <= sc (E^T |Q|) + U |dK_ref|
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import torch

U_BF16 = 2.0 ** -8                     # bf16 keeps 8 significant bits
ACC = 2.0 ** -12                       # fp32 accumulation up to a few thousand keys
NOISE = 2.0 ** -18                     # fp32 noise of dP - delta relative to the magnitudes that cancel in it
LSE_SCORE = 2.0 ** -19                 # lse error per unit of score magnitude (fp32 max in the log2 domain, + log)
# Absolute floor of the lse bound: the exp2 / __logf approximations.  Twice the largest lse error measured on an MI355X over every
# kernel path and input family of tests/test_attention_bounds_gpu.py (2.15e-5: the fp32 product form on the offset family; DESIGN.md
# section 2, "Attention bounds").  lse_bound() holds the total below 1 / (2N).  (The floor was 1e-4 before anybody had measured.)
LSE_FLOOR = 4.3e-5

FAMILIES = ("randn", "ramp", "fall", "offset", "lastkey", "onehot")
# dS ~ 0 in lastkey / onehot: their dQ / dK bounds are the fp32 noise term alone (still bounds, and asserted, but loose against dQ_ref):
# those two families are there for o, lse and dV; ramp, fall and offset are the ones that try dQ and dK.


def gamma_f32(N: int, d: int) -> float:
    return (N + d + 8) * 2.0 ** -24


def _unit(g: torch.Generator, B: int, heads: int, d: int) -> torch.Tensor:
    u = torch.randn(B, heads, 1, d, generator=g, dtype=torch.float64)
    return u / u.norm(dim=-1, keepdim=True)


def make_qkv(case: str, B: int, N: int, heads: int, d: int, seed: int, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """Packed [B, N, 3 heads d] (= [B, N, 3, heads, d]) of one input family, rounded to the compute dtype."""
    assert case in FAMILIES, case
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sd = math.sqrt(d)
    q, k, v = rn(B, heads, N, d), rn(B, heads, N, d), rn(B, heads, N, d)
    u = _unit(g, B, heads, d)
    j = torch.arange(N, dtype=torch.float64).view(1, 1, N, 1)
    if case in ("ramp", "fall"):
        t = j if case == "ramp" else N - 1 - j
        k = 0.3 * k + (40.0 * t / N) * u
        q = 0.3 * q + sd * u
    elif case == "offset":
        k = 0.3 * k + 8.0 * u
        q = 0.3 * q + (70.0 * sd / 8.0) * u
    elif case == "lastkey":
        k = 0.3 * k
        k[:, :, N - 1] += 25.0 * u[:, :, 0]
        q = 0.3 * q + sd * u
    elif case == "onehot":
        e = k / k.norm(dim=-1, keepdim=True)
        k = e
        q = 30.0 * sd * e[:, :, (7 * torch.arange(N) + 3) % N]
    packed = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * heads * d)       # [3,B,h,N,d] -> [B,N,3,h,d]
    return packed.to(dtype)


def make_do(B: int, N: int, heads: int, d: int, seed: int, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """dO [B, N, heads d]: randn in every family."""
    g = torch.Generator().manual_seed(seed + 7919)
    return torch.randn(B, N, heads * d, generator=g, dtype=torch.float64).to(dtype)


def make_xw(case: str, B: int, N: int, heads: int, d: int, D: int, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """x [B, N, D], w [3 heads d, D] in bf16 whose product x w^T has the character of the family (for the fused projection + attention
    kernel).  w carries the family's directions in its last columns, x their per-token coefficients; the other columns mix D - 2 noise
    inputs into every output.  onehot: x is one-hot in D (token i -> column i mod D), the columns of w are the unit keys and the
    matching queries, so a row's mass sits on the one or two keys j = (7 (i mod D) + 3) mod D (mod D)."""
    assert case in FAMILIES, case
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    C = heads * d
    sd = math.sqrt(d)
    if case == "onehot":
        e = rn(heads, D, d)
        e = e / e.norm(dim=-1, keepdim=True)
        wq = 30.0 * sd * e[:, (7 * torch.arange(D) + 3) % D]                                       # [heads, D, d]
        w = torch.cat([wq.permute(0, 2, 1).reshape(C, D), e.permute(0, 2, 1).reshape(C, D), rn(C, D)], 0)
        x = torch.zeros(B, N, D, dtype=torch.float64)
        x[:, torch.arange(N), torch.arange(N) % D] = 1.0
        return x.bfloat16(), w.bfloat16()
    nz = D - 2
    amp = 1.0 if case == "randn" else 0.3
    w = torch.zeros(3 * C, D, dtype=torch.float64)
    w[:, :nz] = rn(3 * C, nz) / math.sqrt(nz)
    w[:2 * C, :nz] *= amp                                                                            # v stays N(0, 1)
    x = torch.zeros(B, N, D, dtype=torch.float64)
    x[:, :, :nz] = rn(B, N, nz)
    if case != "randn":
        u = _unit(g, 1, heads, d).reshape(C)
        w[:C, nz] = u                                                                                # q += x[., nz] u
        w[C:2 * C, nz + 1] = u                                                                       # k += x[., nz + 1] u
        j = torch.arange(N, dtype=torch.float64)
        x[:, :, nz] = 70.0 * sd / 8.0 if case == "offset" else sd
        x[:, :, nz + 1] = {"ramp": 40.0 * j / N, "fall": 40.0 * (N - 1 - j) / N, "offset": torch.full((N,), 8.0, dtype=torch.float64),
                           "lastkey": 25.0 * (j == N - 1)}[case]
    return x.bfloat16(), w.bfloat16()


def heads_first(t: torch.Tensor, heads: int) -> torch.Tensor:
    """[B, N, heads d] -> float64 [B, heads, N, d]."""
    B, N, C = t.shape
    return t.detach().double().cpu().reshape(B, N, heads, C // heads).permute(0, 2, 1, 3)


def split_qkv(qkv: torch.Tensor, heads: int):
    """Packed [B, N, 3 heads d] -> float64 q, k, v, each [B, heads, N, d]."""
    B, N, C3 = qkv.shape
    x = qkv.detach().double().cpu().reshape(B, N, 3, heads, C3 // 3 // heads).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def _unit_roundoff(fp32: bool, N: int, d: int) -> float:
    return gamma_f32(N, d) if fp32 else U_BF16


def _eps(q: torch.Tensor, k: torch.Tensor):
    d = q.shape[-1]
    A = (q.abs() @ k.abs().transpose(-1, -2)).amax(-1) / math.sqrt(d)                               # [B, heads, N]
    return A, (d + 2) * 2.0 ** -24 * A


def lse_bound(A: torch.Tensor, N: int) -> torch.Tensor:
    b = LSE_SCORE * A + LSE_FLOOR
    assert float(b.max()) <= 1.0 / (2 * N), f"lse bound {float(b.max()):.3e} above 1 / (2 N) = {1.0 / (2 * N):.3e}: a dropped key of a uniform row would pass"
    return b


def forward_bounds(qkv: torch.Tensor, heads: int, fp32: bool = False) -> Dict[str, torch.Tensor]:
    """float64 o [B, heads, N, d] and lse [B, heads, N] of the rounded inputs, with their elementwise bounds o_bound / lse_bound."""
    q, k, v = split_qkv(qkv, heads)
    N, d = q.shape[-2], q.shape[-1]
    U = _unit_roundoff(fp32, N, d)
    s = q @ k.transpose(-1, -2) / math.sqrt(d)
    lse = torch.logsumexp(s, -1)
    P = torch.exp(s - lse[..., None])
    A, eps = _eps(q, k)
    return {"o": P @ v, "lse": lse, "o_bound": (2 * U + 2 * eps + ACC)[..., None] * (P @ v.abs()), "lse_bound": lse_bound(A, N)}


def backward_bounds(do: torch.Tensor, qkv: torch.Tensor, o_kernel: torch.Tensor, lse_kernel: torch.Tensor, heads: int,
                    fp32: bool = False) -> Dict[str, torch.Tensor]:
    """float64 dq, dk, dv [B, heads, N, d] GIVEN the kernel's own o [B, N, heads d] and lse [B, heads, N], with dq_bound, dk_bound, dv_bound."""
    q, k, v = split_qkv(qkv, heads)
    N, d = q.shape[-2], q.shape[-1]
    sc = 1.0 / math.sqrt(d)
    U = _unit_roundoff(fp32, N, d)
    dO, o = heads_first(do, heads), heads_first(o_kernel, heads)
    lse = lse_kernel.detach().double().cpu()
    P = torch.exp(q @ k.transpose(-1, -2) * sc - lse[..., None])
    delta = (dO * o).sum(-1, keepdim=True)
    dS = P * (dO @ v.transpose(-1, -2) - delta)
    _, eps = _eps(q, k)
    eps = eps[..., None]
    E = U * dS.abs() + NOISE * P * (dO.abs() @ v.abs().transpose(-1, -2) + (dO * o).abs().sum(-1, keepdim=True)) + 2 * eps * dS.abs()
    dq, dk, dv = sc * (dS @ k), sc * (dS.transpose(-1, -2) @ q), P.transpose(-1, -2) @ dO
    return {"dq": dq, "dk": dk, "dv": dv,
            "dv_bound": ((2 * U + 2 * eps + ACC) * P).transpose(-1, -2) @ dO.abs(),
            "dq_bound": sc * (E @ k.abs()) + U * dq.abs(),
            "dk_bound": sc * (E.transpose(-1, -2) @ q.abs()) + U * dk.abs()}


def split_dqkv(dqkv: torch.Tensor, heads: int):
    return split_qkv(dqkv, heads)


def ratio(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor):
    """max(|got - ref| / bound) and where: (image, head, token, column) -- (image, head, token) for lse."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    err = (got - ref).abs()
    r = err / bound.clamp_min(1e-300)
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))                        # a NaN / inf output is over any bound
    r = torch.where((err == 0) & (bound == 0), torch.zeros_like(r), r)
    flat = int(r.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), r.shape))
    return float(r.reshape(-1)[flat]), idx


def check(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, what: str):
    """Assert |got - ref| <= bound elementwise; returns (max err / bound, its index)."""
    r, idx = ratio(got, ref, bound)
    assert r <= 1.0, (f"{what}: err / bound = {r:.3g} at (image, head, token, column) = {idx}: got {float(got.detach().double().cpu()[idx]):.6g}, "
                      f"fp64 {float(ref[idx]):.6g}, bound {float(bound[idx]):.3g}")
    return r, idx


def check_forward(o: torch.Tensor, lse: torch.Tensor, fb: Dict[str, torch.Tensor], heads: int, what: str) -> Dict[str, float]:
    """o [B, N, heads d] and lse [B, heads, N] of a kernel against forward_bounds(); returns the measured ratios and the lse error."""
    out = {"lse_err": float((lse.detach().double().cpu() - fb["lse"]).abs().max())}
    out["o"] = check(heads_first(o, heads), fb["o"], fb["o_bound"], what + " o")[0]
    out["lse"] = check(lse, fb["lse"], fb["lse_bound"], what + " lse")[0]
    return out


def check_backward(dqkv: torch.Tensor, bb: Dict[str, torch.Tensor], heads: int, what: str) -> Dict[str, float]:
    """Packed dqkv of a kernel against backward_bounds(): dQ, dK and dV each on its own."""
    dq, dk, dv = split_dqkv(dqkv, heads)
    return {"dq": check(dq, bb["dq"], bb["dq_bound"], what + " dQ")[0], "dk": check(dk, bb["dk"], bb["dk_bound"], what + " dK")[0],
            "dv": check(dv, bb["dv"], bb["dv_bound"], what + " dV")[0]}
