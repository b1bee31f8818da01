"""colsum_kernel of csrc/gemm.hip (dinox_colsum) in NumPy float32, addition for addition, and its float64 bound.

The kernel only adds, so no compiler may contract anything: the device result must equal colsum32() bit for bit.  Order, per column:
thread group g of 16 takes rows g, g + 16, ...; while r + 48 < M four rows go into four sums (s0 += x[r], s1 += x[r + 16],
s2 += x[r + 32], s3 += x[r + 48]; r += 64), the remaining rows r, r + 16, ... into s0; the group's sum is (s0 + s1) + (s2 + s3); the
16 groups meet as the balanced tree the kernel writes out; last (accumulate ? out : 0) + v.

Bound against float64, independent of the emulation: an input passes through at most ceil(M / 16) additions inside its group sum
(ceil(ceil(M / 16) / 4) in its own s, up to 3 tail rows, 2 to join the four), 4 in the tree and 1 into out: gamma_{ceil(M/16) + 6}
(sum |x| + |out_in|), with u = 2^-24.
"""
import math

import numpy as np

U32 = 2.0 ** -24
GUARD = 64
CANARY_F32 = np.uint32(0x7A5C3CA5)
NAN_BF16 = np.uint16(0x7FC0)

MS = (1, 15, 16, 17, 48, 49, 63, 64, 65, 113, 1003)
NS = (1, 63, 64, 65, 130)


def bf16_round(x):
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def bf16_to_f32(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def colsum32(x: np.ndarray, out_in=None, variant: str = "kernel") -> np.ndarray:
    """x float32 [M][N] (the live values) -> float32 [N] in the kernel's order.  variant "flat_join": the group's sum taken as
    ((s0 + s1) + s2) + s3 -- a defect the bit comparison must see and the float64 bound must not."""
    x = np.asarray(x, dtype=np.float32)
    M, N = x.shape
    red = np.zeros((16, N), dtype=np.float32)
    for g in range(16):
        s = [np.zeros(N, dtype=np.float32) for _ in range(4)]
        r = g
        while r + 48 < M:
            for q in range(4):
                s[q] = s[q] + x[r + 16 * q]
            r += 64
        while r < M:
            s[0] = s[0] + x[r]
            r += 16
        red[g] = ((s[0] + s[1]) + s[2]) + s[3] if variant == "flat_join" else (s[0] + s[1]) + (s[2] + s[3])
    t = red
    v = (((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]))) + \
        (((t[8] + t[9]) + (t[10] + t[11])) + ((t[12] + t[13]) + (t[14] + t[15])))
    base = np.zeros(N, dtype=np.float32) if out_in is None else np.asarray(out_in, dtype=np.float32)
    return (base + v).astype(np.float32)


def ascending32(x: np.ndarray, out_in=None) -> np.ndarray:
    """The plain float32 sum over rows in ascending order: what the kernel's order must differ from for the bit test to mean anything."""
    acc = np.zeros(x.shape[1], dtype=np.float32)
    for r in range(x.shape[0]):
        acc = acc + x[r].astype(np.float32)
    return acc if out_in is None else (np.asarray(out_in, np.float32) + acc).astype(np.float32)


def reference(x: np.ndarray, out_in=None):
    """(float64 column sums, bound)."""
    M = x.shape[0]
    x64 = x.astype(np.float64)
    o = np.zeros(x.shape[1]) if out_in is None else np.asarray(out_in, dtype=np.float64)
    depth = math.ceil(M / 16) + 6
    gam = depth * U32 / (1.0 - depth * U32)
    return x64.sum(0) + o, gam * (np.abs(x64).sum(0) + np.abs(o))


def cases():
    """At most 60 (name, M, N, ldx, bf16?, accumulate) in which every M meets both dtypes and every N, both ldx forms and both
    accumulate values occur: M x dtype = 22 cases, the other axes walk through their values at coprime strides; the rest adds every
    N with the two largest M at the remaining (ldx, accumulate) combinations."""
    out = []
    i = 0
    for M in MS:
        for bf in (0, 1):
            N = NS[i % 5]
            out.append((M, N, N + 3 * ((i // 2 + bf) % 2), bf, (i // 3 + i) % 2))
            i += 1
    for j, N in enumerate(NS):
        for M in (113, 1003):
            out.append((M, N, N + 3 * (j % 2), (j + (M > 113)) % 2, (j + 1) % 2))
            out.append((M, N, N + 3 * ((j + 1) % 2), (j + 1 + (M > 113)) % 2, j % 2))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return [(f"{M}x{N}-ld{ld}-{'bf16' if bf else 'f32'}-{'acc' if ac else 'ovw'}", M, N, ld, bool(bf), bool(ac)) for M, N, ld, bf, ac in uniq]


def build(M: int, N: int, ldx: int, bf16: bool, accumulate: bool, seed: int = 0):
    """(x raw [GUARD + M ldx + GUARD] with NaN padding, live float32 [M][N], out raw float32 [GUARD + N + GUARD] between canaries
    (live part ~ randn under accumulate), out_in or None).  Mixed magnitudes, randn x 10^uniform(-3, 3): the order of the additions
    shows in the last bits."""
    rng = np.random.default_rng(7000 + 131 * M + 7 * N + ldx + 2 * bf16 + accumulate + seed)
    vals = (rng.standard_normal((M, N)) * 10.0 ** rng.uniform(-3, 3, (M, N))).astype(np.float32)
    if bf16:
        bits = bf16_round(vals)
        live = bf16_to_f32(bits)
        raw = np.full(2 * GUARD + M * ldx, NAN_BF16, dtype=np.uint16)
        src = bits
    else:
        live = vals
        raw = np.full(2 * GUARD + M * ldx, np.nan, dtype=np.float32)
        src = vals
    idx = GUARD + np.arange(M).reshape(-1, 1) * ldx + np.arange(N)
    raw[idx] = src
    out = np.full(2 * GUARD + N, CANARY_F32, dtype=np.uint32).view(np.float32)
    out_in = None
    if accumulate:
        out_in = (rng.standard_normal(N) * 100.0).astype(np.float32)
        out[GUARD:GUARD + N] = out_in
    return raw, live, out, out_in
