"""Float64 NumPy statement of the 3-D surface distances of include/dinox.h (csrc/surfdist3d.hip) -- 6-neighbour borders, directed distances
with the voxel (s_z, s_y, s_x), the per-direction statistics and the metrics formed from them -- written from the definitions, calling no
project code, with a-priori elementwise fp32 bounds.

Distances come from brute force over the border voxel lists (np.argwhere, broadcast, min), a block of query voxels at a time.  A query
voxel that is itself a border voxel of the other side has distance 0 by definition and is not searched.

Bounds (u = 2^-24, gam(n) = n u / (1 - n u)).  The kernel forms a distance as sqrt(fl(a + fl(b + c))) with a = fl(fl(s_x k)^2),
b = fl(fl(s_y m)^2), c = fl(fl(s_z n)^2) from the fp32 spacings and integer offsets, every operation rounded once (no contraction, a
correctly rounded square root).  A product and its square carry (1 + u)^3 (one rounding, doubled by squaring, and the square's own), the
inner sum one more factor on b and c, the outer sum one more on everything: the radicand is within (1 + u)^5 of exact, its root within
2.5 u, the root's own rounding adds u -- 3.5 u.  This oracle allows one half-u step above that per distance: REL = 4 u.  The minimum over
candidates in two stages (over y', then over x') moves by no more than the candidates do, and so do the order statistics: max and quantile
inherit REL.  The sum of n such distances, in any order, lands within (REL + gam(n)(1 + REL)) of the exact sum of the (non-negative)
distances.  Counts are integers and have no bound: they must be equal, which needs every exact distance clear of every tolerance --
``Distances.min_gap`` reports the smallest relative gap for the test to assert on its inputs.
The spacings are taken as the fp32 values the kernel is given (they are data, not results).
"""
from __future__ import annotations

import numpy as np

U32 = 2.0 ** -24
REL = 4 * U32
IGNORE = 255


def gam(n) -> float:
    return n * U32 / (1.0 - n * U32)


def border(X: np.ndarray) -> np.ndarray:
    """The voxels of the boolean set X [Z, H, W] with at least one of their six face neighbours outside X (outside the volume = outside X)."""
    P = np.pad(X, 1, constant_values=False)
    inner = (P[:-2, 1:-1, 1:-1] & P[2:, 1:-1, 1:-1] & P[1:-1, :-2, 1:-1] & P[1:-1, 2:, 1:-1] & P[1:-1, 1:-1, :-2] & P[1:-1, 1:-1, 2:])
    return X & ~inner


def sets(pred: np.ndarray, gt: np.ndarray, c: int):
    """(A, G) of one volume: A = {gt != 255 and pred = c}, G = {gt = c}."""
    return (gt != IGNORE) & (pred == c), gt == c


def directed(BQ: np.ndarray, BY: np.ndarray, spacing, pairs: int = 1 << 22) -> np.ndarray:
    """d(p, BY) for every voxel p of the boolean border BQ against the boolean border BY, in np.argwhere's order of BQ; inf where BY is
    empty."""
    Q, Y = np.argwhere(BQ), np.argwhere(BY)
    if len(Y) == 0:
        return np.full(len(Q), np.inf)
    out = np.zeros(len(Q), dtype=np.float64)
    far = np.flatnonzero(~BY[tuple(Q.T)])                       # the others are border voxels of the other side themselves: 0
    ym = Y.astype(np.float64) * np.asarray(spacing, dtype=np.float64)
    block = max(1, pairs // len(Y))
    for i in range(0, len(far), block):
        q = Q[far[i:i + block]].astype(np.float64) * np.asarray(spacing, dtype=np.float64)
        d2 = (q[:, None, 0] - ym[None, :, 0]) ** 2
        d2 += (q[:, None, 1] - ym[None, :, 1]) ** 2
        d2 += (q[:, None, 2] - ym[None, :, 2]) ** 2
        out[far[i:i + block]] = np.sqrt(d2.min(1))
    return out


class Distances:
    """Every directed distance of a volume, sorted, once: d[c][dir] float64 [n]; dir 0 from the border of pred to the border of gt."""

    def __init__(self, pred: np.ndarray, gt: np.ndarray, spacing, C: int) -> None:
        assert pred.shape == gt.shape and pred.dtype == gt.dtype == np.uint8 and pred.ndim == 3
        self.shape, self.C = pred.shape, C
        self.spacing = np.asarray(spacing, dtype=np.float32).astype(np.float64).reshape(3)
        self.d = []
        for c in range(C):
            A, G = sets(pred, gt, c)
            bA, bG = border(A), border(G)
            self.d.append((np.sort(directed(bA, bG, self.spacing)), np.sort(directed(bG, bA, self.spacing))))

    def min_gap(self, tolerances) -> float:
        """The smallest |d - tol| / tol over the finite distances and the tolerances (inf if there are none)."""
        out = np.inf
        for c in range(self.C):
            for d in self.d[c]:
                d = d[np.isfinite(d)]
                for t in tolerances:
                    if d.size and t > 0:
                        out = min(out, float(np.abs(d - t).min() / t))
        return out

    def stats(self, tolerances, q=(95, 100)):
        """counts int64 [C, 2, 1 + T], values float64 [C, 2, 3] = (sum, max, k-th smallest), bound: the fp32 bound of each value."""
        T = len(tolerances)
        counts = np.zeros((self.C, 2, 1 + T), dtype=np.int64)
        values = np.zeros((self.C, 2, 3))
        bound = np.zeros((self.C, 2, 3))
        for c in range(self.C):
            for k, d in enumerate(self.d[c]):
                n = len(d)
                counts[c, k, 0] = n
                if n == 0 or not np.isfinite(d[0]):              # no query border, or nothing on the other side: zeros
                    continue
                rank = (n * int(q[0]) + int(q[1]) - 1) // int(q[1])              # ceil in integers
                counts[c, k, 1:] = [(d <= np.float64(np.float32(t))).sum() for t in tolerances]
                values[c, k] = (d.sum(), d[-1], d[rank - 1])
                bound[c, k] = ((REL + gam(n) * (1 + REL)) * d.sum(), REL * d[-1], REL * d[rank - 1])
        return counts, values, bound


def metrics(counts: np.ndarray, values: np.ndarray, spacing, shape):
    """Per class of one volume from the per-direction outputs: dict of hd95 (the quantile asked for), hd, assd [1, C] and nsd [1, C, T],
    float64.  Both borders empty: NaN.  One empty: the distance metrics take the volume diagonal in mm, NSD 0."""
    counts, values = np.asarray(counts, dtype=np.float64), np.asarray(values, dtype=np.float64)
    sp = np.asarray(spacing, dtype=np.float64).reshape(3)
    diag = np.sqrt(((sp * np.asarray(shape, dtype=np.float64)) ** 2).sum())
    nA, nG = counts[:, 0, 0], counts[:, 1, 0]
    absent, one = (nA == 0) & (nG == 0), (nA == 0) ^ (nG == 0)
    den = np.maximum(nA + nG, 1)

    def pick(x):
        return np.where(absent, np.nan, np.where(one, diag, x))[None]

    nsd = (counts[:, 0, 1:] + counts[:, 1, 1:]) / den[:, None]
    nsd = np.where(one[:, None], 0.0, nsd)
    return {"hd95": pick(np.maximum(values[:, 0, 2], values[:, 1, 2])), "hd": pick(np.maximum(values[:, 0, 1], values[:, 1, 1])),
            "assd": pick((values[:, 0, 0] + values[:, 1, 0]) / den), "nsd": np.where(absent[:, None], np.nan, nsd)[None]}
