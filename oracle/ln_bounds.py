"""The LayerNorm kernel family, element by element: float64 reference, a-priori rounding bounds, hostile rows (CPU, no GPU).

Kernels (csrc/layernorm.hip; the LayerNorm epilogues of csrc/gemm_bf16_rowln.hip and csrc/gemm_bf16_pp384.hip):
    forward    mean = sum x / D,  var = sum (x - mean)^2 / D  (two passes over registers),  rstd = rsqrt(var + eps),
               y = (x - mean) rstd gamma + beta   (fp32 or bf16)
    backward   xh = (x - mean) rstd,  g = dy gamma,  m1 = sum g / D,  m2 = sum g xh / D,
               dx = rstd (g - m1 - xh m2) (+ dx_add)   (fp32, and its bf16 copy),   dgamma = sum_r dy xh,  dbeta = sum_r dy
The backward is judged GIVEN the mean / rstd it was handed (the reference evaluates the same formulas on those fp32 values in float64),
so the forward's error is not counted twice.

Input families.  x: randn | offset (1e3 c_r + randn: |mean| >> std) | steps (0.1 randn + a level per quarter of the row: the only rows
on which the between-quarter term of the 128 x 384 kernel's combine and the half-wave exchange of the width-384 kernels carry the
variance) | const (variance 0, rstd = 1 / sqrt(eps)) | tiny (1e-4 randn: variance << eps) | spike_first / spike_last (1e4 in column 0 /
D - 1).  dy: randn | aligned (xh gamma + 0.01 randn: m2 dominates, dx is a small difference of large terms) | flat (1 / gamma: g is
constant, dx ~ 0) | lastrow (zero except the last row: a dropped partial sum shows).  gamma = 1 + 0.2 randn, beta = 0.3 randn.

Bounds, per output element (u = 2^-24; every constant is an operation count of the kernels, none comes from a run):
    depth(D, serial) = serial + 10, serial = ceil(D / 64) unless a kernel says otherwise: the longest chain of additions an addend of a
                     row sum passes through -- the lane's own terms (generic kernels: ceil(D / 64) scalars; float4 kernels:
                     ceil(D / 256) float4 + the 2 levels of (x + y) + (z + w), fewer; half-wave kernels: 3 + 2; the 128 x 384 kernel:
                     12 + 2 for the sum but 48 for its M2, so it passes serial = 48; its 3 adds of the four-quarter combine count
                     among the 6 exchange steps it does not have), 6 exchange steps, and 1 / D with its product (2) + 2 spare
    mean             e_mu = depth u mean_j |x_j|                            (the 128 x 384 kernel: the largest quarter's mean |x|)
    var              (depth + 3) u (var + e_mu^2) + e_mu^2: two passes are exact to first order in the mean's error,
                     sum (x - mu')^2 = sum (x - mu)^2 + D (mu' - mu)^2; + 3: the subtraction, the square, the product with 1 / D.
                     Four-quarter combine only (Chan): each quarter's M2 is taken about ITS computed mean and moved by 96 d_w^2, which
                     leaves the cross term 2 d_w (mu_w' - mu_w): + 2 e_mu sqrt(var)
    rstd             rstd_ref (1 / sqrt(1 - e_var / (var + eps)) - 1 + 4 u): + eps, rsqrtf (1 ulp = 2 u), 1 spare
    y                |gamma| rstd (e_mu + u |x - mu|) + |gamma xh| relerr(rstd) + 4 u (|gamma xh| + |beta|): the subtraction, two
                     products, the add;  bf16: + half a bf16 ulp of (|y_ref| + that), round to nearest even (oracle/gemm_bounds.py)
    dx               rstd u [4 |g| + (depth + 4)(mean |g| + |xh| mean |g xh|) + 6 |xh m2| + 2 |m1|] + 2 u |dx_ref| + u |dx_add|:
                     g and xh carry 1 and 2 roundings, a term of sum g xh 4, the row sums depth, the three-term difference and the product
                     with rstd 3, the final add 1;  bf16 copy: + half a bf16 ulp
    dgamma, dbeta    (chain + 3) u sum_r |dy xh|,  chain u sum_r |dy|:  chain = rows per wave + 4 waves + parts / 64 + 64 (a lane's
                     register sum over the rows its wave visits, the block's waves through LDS, ln_bwd_reduce's 64 groups and their
                     sum); + 3: xh and the product.  accumulate: + u |what dw / db held|
Fused kernels: x_out carries the GEMM bound of oracle/gemm_bounds.py (accumulation in any order, bias, residual); y, mean, rstd are
judged given the kernel's own x_out.  dinox_linear_ln_bwd rounds its product to bf16 before the LayerNorm backward: an element whose
float64 product lies within the accumulation bound of a rounding tie may round either way, and for THOSE elements one bf16 ulp of dy
is carried through the backward formulas into the bounds (dx: rstd (|gamma| t + mean |gamma| t + |xh| mean |gamma xh| t); dgamma:
sum_r t |xh|; dbeta: sum_r t).  Nothing is exempt; tie_share reports how many there were.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np

from oracle import gemm_bounds as GB

U32 = GB.U32
X_FAMILIES = ("randn", "offset", "steps", "const", "tiny", "spike_first", "spike_last")
DY_FAMILIES = ("randn", "aligned", "flat", "lastrow")
LEVELS = (-3.0, 1.0, 2.0, 8.0)
RSQ_OPS = 4
OUT_OPS = 4


def depth(dim: int, serial: Optional[int] = None) -> int:
    return (serial if serial is not None else math.ceil(dim / 64)) + 10


def row_chain(rows_per_wave: int, parts: int, waves: int = 4) -> int:
    return rows_per_wave + waves + math.ceil(parts / 64) + 64


def ln_parts(rows: int) -> int:
    """ln_parts of csrc/layernorm.hip: blocks of four waves, at most 1024."""
    return min(math.ceil(rows / 4), 1024)


def standalone_chain(rows: int, dim: int) -> int:
    """The dgamma / dbeta chain of dinox_layernorm_bwd: the width-384 kernels walk 8 half-wave rows per block and meet their twin half
    by one more add; the generic kernel adds a block's rows (4 per sweep) into one LDS cell."""
    parts = ln_parts(rows)
    if dim == 384:
        nblk = min(math.ceil(rows / 16), parts, 768)
        return row_chain(math.ceil(rows / (8 * nblk)) + 1, nblk)
    per_wave = math.ceil(rows / (4 * parts))
    fast = dim % 4 == 0 and dim <= 2048
    return row_chain(per_wave if fast else 4 * per_wave, parts)


# ------------------------------------------------------------------------------------------ inputs
def _key(name: str) -> int:
    return sum((i + 1) * ord(c) for i, c in enumerate(name))


def make_params(dim: int, seed: int = 0):
    r = np.random.default_rng([7, dim, seed])
    return (1 + 0.2 * r.standard_normal(dim)).astype(np.float32), (0.3 * r.standard_normal(dim)).astype(np.float32)


def make_x(family: str, rows: int, dim: int, seed: int = 0) -> np.ndarray:
    r = np.random.default_rng([11, _key(family), rows, dim, seed])
    z = r.standard_normal((rows, dim))
    c = r.standard_normal((rows, 1))
    if family == "randn":
        x = z
    elif family == "offset":
        x = 1e3 * c + z
    elif family == "steps":
        lv = np.empty(dim)
        for q, part in enumerate(np.array_split(np.arange(dim), 4)):
            lv[part] = LEVELS[q]
        x = 0.1 * z + lv
    elif family == "const":
        x = np.broadcast_to(c, (rows, dim))
    elif family == "tiny":
        x = 1e-4 * z
    elif family == "spike_first":
        x = z.copy()
        x[:, 0] = 1e4
    elif family == "spike_last":
        x = z.copy()
        x[:, -1] = 1e4
    else:
        raise ValueError(family)
    return np.ascontiguousarray(x, dtype=np.float32)


def to_bf16_values(a: np.ndarray) -> np.ndarray:
    """Round to bf16 (nearest even) and return the values as float32."""
    return GB.bf16_to_f64(GB.bf16_round(a)).astype(np.float32)


def make_dy(family: str, x: np.ndarray, gamma: np.ndarray, eps: float, seed: int = 0, bf16: bool = False) -> np.ndarray:
    rows, dim = x.shape
    r = np.random.default_rng([13, _key(family), rows, dim, seed])
    z = r.standard_normal((rows, dim))
    g64 = gamma.astype(np.float64)
    if family == "randn":
        dy = z
    elif family == "aligned":
        x64 = x.astype(np.float64)
        mu = x64.mean(1, keepdims=True)
        xh = (x64 - mu) / np.sqrt(((x64 - mu) ** 2).mean(1, keepdims=True) + eps)
        dy = xh * g64 + 0.01 * z
    elif family == "flat":
        dy = np.broadcast_to(1.0 / g64, (rows, dim))
    elif family == "lastrow":
        dy = np.zeros((rows, dim))
        dy[-1] = z[-1]
    else:
        raise ValueError(family)
    dy = np.ascontiguousarray(dy, dtype=np.float32)
    return to_bf16_values(dy) if bf16 else dy


# ------------------------------------------------------------------------------------------ reference and bounds
def _lowp(ref: np.ndarray, err: np.ndarray) -> np.ndarray:
    return err + GB.half_ulp_bf16(np.abs(ref) + err)


def forward_ref(x, gamma, beta, eps: float, out_bf16: bool = False, serial: Optional[int] = None, combine: bool = False) -> Dict[str, np.ndarray]:
    """mean, rstd [rows] and y [rows, D] in float64 with their bounds (`<name>_bound`).  combine: the four-quarter (Chan) form."""
    x, g, b = (np.asarray(a, dtype=np.float64) for a in (x, gamma, beta))
    D = x.shape[1]
    dep = depth(D, serial)
    mu = x.mean(1, keepdims=True)
    var = ((x - mu) ** 2).mean(1, keepdims=True)
    if combine:
        ax = np.abs(x).reshape(x.shape[0], 4, D // 4).mean(2).max(1, keepdims=True)
    else:
        ax = np.abs(x).mean(1, keepdims=True)
    e_mu = dep * U32 * ax
    e_var = (dep + 3) * U32 * (var + e_mu ** 2) + e_mu ** 2 + (2 * e_mu * np.sqrt(var) if combine else 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    t = np.minimum(e_var / (var + eps), 0.5)
    rel = 1.0 / np.sqrt(1.0 - t) - 1.0 + RSQ_OPS * U32
    xh = (x - mu) * rstd
    y = xh * g + b
    e_y = np.abs(g) * rstd * (e_mu + U32 * np.abs(x - mu)) + np.abs(g * xh) * rel + OUT_OPS * U32 * (np.abs(g * xh) + np.abs(b))
    return {"mean": mu[:, 0], "mean_bound": e_mu[:, 0],"rstd": rstd[:, 0], "rstd_bound": (rstd * rel)[:, 0],
            "y": y, "y_bound": _lowp(y, e_y) if out_bf16 else e_y}


def backward_ref(dy, x, gamma, mean, rstd, dx_add=None, chain: int = 0, serial: Optional[int] = None, acc_w=None, acc_b=None,
                 dy_ulp=None) -> Dict[str, np.ndarray]:
    """dx [rows, D], its bf16 copy `lowp`, dgamma, dbeta [D] in float64 given the fp32 mean / rstd the kernel was handed, with their
    bounds.  chain: the row chain of the launch (row_chain / standalone_chain).  acc_w / acc_b: what dgamma / dbeta held under
    accumulate.  dy_ulp [rows, D]: for the fused product, one bf16 ulp where dy may round either way, else 0."""
    dy, x, gam = (np.asarray(a, dtype=np.float64) for a in (dy, x, gamma))
    mu = np.asarray(mean, dtype=np.float64).reshape(-1, 1)
    rs = np.asarray(rstd, dtype=np.float64).reshape(-1, 1)
    D = x.shape[1]
    dep = depth(D, serial)
    xh = (x - mu) * rs
    g = dy * gam
    m1 = g.mean(1, keepdims=True)
    m2 = (g * xh).mean(1, keepdims=True)
    add = np.zeros_like(x) if dx_add is None else np.asarray(dx_add, dtype=np.float64)
    dx = rs * (g - m1 - xh * m2) + add
    ag, axh = np.abs(g), np.abs(xh)
    e = rs * U32 * (4 * ag + (dep + 4) * (ag.mean(1, keepdims=True) + axh * (ag * axh).mean(1, keepdims=True)) + 6 * np.abs(xh * m2) + 2 * np.abs(m1))
    e = e + 2 * U32 * np.abs(dx) + U32 * np.abs(add)
    dw, db = (dy * xh).sum(0), dy.sum(0)
    e_w = (chain + 3) * U32 * np.abs(dy * xh).sum(0) + U32 * np.abs(dw)
    e_b = chain * U32 * np.abs(dy).sum(0) + U32 * np.abs(db)
    if dy_ulp is not None:
        t = np.asarray(dy_ulp, dtype=np.float64)
        tg = t * np.abs(gam)
        e = e + rs * (tg + tg.mean(1, keepdims=True) + axh * (tg * axh).mean(1, keepdims=True))
        e_w = e_w + (t * axh).sum(0)
        e_b = e_b + t.sum(0)
    if acc_w is not None:
        aw, ab = np.asarray(acc_w, dtype=np.float64), np.asarray(acc_b, dtype=np.float64)
        dw, db = dw + aw, db + ab
        e_w, e_b = e_w + U32 * (np.abs(aw) + np.abs(dw)), e_b + U32 * (np.abs(ab) + np.abs(db))
    return {"dx": dx, "dx_bound": e, "lowp": dx, "lowp_bound": _lowp(dx, e), "dgamma": dw, "dgamma_bound": e_w, "dbeta": db, "dbeta_bound": e_b}


def product_ref(a, w, bias=None, residual=None) -> Dict[str, np.ndarray]:
    """x = a w^T (+ bias) (+ residual) in float64 on the bf16 operand values, with the bound of oracle/gemm_bounds.py (reference(): accumulation
    gamma_K T, combining, the residual add) for an fp32 output; `acc_bound` is the product's own part (what the bf16 rounding of
    dinox_linear_ln_bwd's internal dy sees)."""
    a, w = np.asarray(a, dtype=np.float64), np.asarray(w, dtype=np.float64)
    K = a.shape[1]
    S, T = a @ w.T, np.abs(a) @ np.abs(w).T
    gam = K * U32 / (1.0 - K * U32)
    comb = (math.ceil(K / 256) + GB.EPI_OPS) * U32
    bz = np.zeros((1, S.shape[1])) if bias is None else np.asarray(bias, dtype=np.float64).reshape(1, -1)
    v = S + bz
    e = gam * T + comb * (T + np.abs(bz))
    acc = e.copy()
    if residual is not None:
        r = np.asarray(residual, dtype=np.float64)
        e = e + 2 * U32 * (np.abs(v) + np.abs(r))
        v = v + r
    return {"x": v, "x_bound": e, "acc_bound": acc}


def rounded_dy(a, w):
    """The internal dy of dinox_linear_ln_bwd: bf16(a w^T) as float64 values, and one bf16 ulp on the elements that may round either way
    (the float64 product within the accumulation bound of a tie), 0 elsewhere; the share of those elements."""
    p = product_ref(a, w)
    S, e = p["x"], p["acc_bound"]
    mid = GB.bf16_to_f64(GB.bf16_round(S))
    lo, hi = GB.bf16_to_f64(GB.bf16_round(S - e)), GB.bf16_to_f64(GB.bf16_round(S + e))
    tie = lo != hi
    ulp = np.where(tie, np.maximum(np.abs(hi - mid), np.abs(mid - lo)), 0.0)
    return mid, ulp, float(tie.mean())


# ------------------------------------------------------------------------------------------ judging a result
def check(got, ref: np.ndarray, bound: np.ndarray) -> dict:
    """The largest |got - ref| / bound over EVERY element (none exempt; a non-finite element counts as infinite), its index, the number
    compared and the number of non-finite elements.  An element with bound 0 must equal its reference."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    bad = ~np.isfinite(got)
    err = np.abs(np.where(bad, 0.0, got) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bad, np.inf, np.where(err == 0.0, 0.0, err / bound))
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.size else ()
    return {"ratio": float(ratio[at]) if ratio.size else 0.0, "where": tuple(int(i) for i in at), "compared": int(ratio.size), "nan": int(bad.sum())}


def check_all(got: Dict[str, np.ndarray], ref: Dict[str, np.ndarray]) -> dict:
    """check() over every output named in `got`; ratio_<name>, where_<name>, the overall ratio, compared, nan, and expected = the
    number of reference elements of those outputs (compared must equal it)."""
    r = {"compared": 0, "nan": 0, "expected": 0}
    for name, g in got.items():
        c = check(g, ref[name], ref[name + "_bound"])
        r["ratio_" + name], r["where_" + name] = c["ratio"], c["where"]
        r["compared"] += c["compared"]
        r["nan"] += c["nan"]
        r["expected"] += int(ref[name].size)
    r["ratio"] = max(v for k, v in r.items() if k.startswith("ratio_"))
    r["ok"] = r["ratio"] <= 1.0 and r["nan"] == 0 and r["compared"] == r["expected"]
    return r
