"""Float64 NumPy statement of the surface distances of include/dinox.h (csrc/surfdist.hip) -- borders, directed distances, the per-direction
statistics and the metrics formed from them -- written from the definitions, calling no project code, with a-priori elementwise fp32 bounds.

Distances come from brute force over the border pixel lists (np.argwhere, broadcast, min), a block of query pixels at a time.

Bounds (u = 2^-24, gam(n) = n u / (1 - n u)).  The kernel forms a distance as sqrt(fl(fl(fl(s_x k)^2) + fl(fl(s_y m)^2))) from the fp32
spacings and integer offsets, every operation rounded once (no contraction, a correctly rounded square root): each square carries
(1 + u)^3, the sum one more factor, so the radicand is within 4 u and its root within 2 u, the root's own rounding adds u -- 3 u, inside the
4 u this oracle allows per distance (REL).  The minimum over candidates moves by no more than the candidates do, and so do the order
statistics: max and quantile inherit REL.  The sum of n such distances, in any order, lands within (REL + gam(n)(1 + REL)) of the exact
sum of the (non-negative) distances.  Counts are integers and have no bound: they must be equal, which needs every exact distance clear
of every tolerance -- ``Distances.min_gap`` reports the smallest relative gap per image for the test to assert on its inputs.
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
    """The pixels of the boolean set X [H, W] with at least one of their four edge neighbours outside X (outside the image = outside X)."""
    P = np.pad(X, 1, constant_values=False)
    inner = P[:-2, 1:-1] & P[2:, 1:-1] & P[1:-1, :-2] & P[1:-1, 2:]
    return X & ~inner


def sets(pred: np.ndarray, gt: np.ndarray, c: int):
    """(A, G) of one image: A = {gt != 255 and pred = c}, G = {gt = c}."""
    return (gt != IGNORE) & (pred == c), gt == c


def directed(Q: np.ndarray, Y: np.ndarray, sy: float, sx: float, block: int = 512) -> np.ndarray:
    """d(p, Y) for every p of the pixel list Q [n, 2] = (y, x) against the list Y [m, 2]; inf where Y is empty."""
    if len(Y) == 0:
        return np.full(len(Q), np.inf)
    out = np.empty(len(Q), dtype=np.float64)
    yy, yx = Y[:, 0].astype(np.float64) * sy, Y[:, 1].astype(np.float64) * sx
    for i in range(0, len(Q), block):
        q = Q[i:i + block].astype(np.float64)
        d2 = (q[:, :1] * sy - yy[None]) ** 2 + (q[:, 1:] * sx - yx[None]) ** 2
        out[i:i + block] = np.sqrt(d2.min(1))
    return out


class Distances:
    """Every directed distance of a batch, sorted, once: d[b][c][dir] float64 [n]; dir 0 from the border of pred to the border of gt."""

    def __init__(self, pred: np.ndarray, gt: np.ndarray, spacing: np.ndarray, C: int) -> None:
        assert pred.shape == gt.shape and pred.dtype == gt.dtype == np.uint8 and pred.ndim == 3
        self.B, self.H, self.W = pred.shape
        self.C = C
        self.spacing = np.asarray(spacing, dtype=np.float32).astype(np.float64).reshape(self.B, 2)
        self.d = []
        for b in range(self.B):
            sy, sx = self.spacing[b]
            per = []
            for c in range(C):
                A, G = sets(pred[b], gt[b], c)
                qa, qg = np.argwhere(border(A)), np.argwhere(border(G))
                per.append((np.sort(directed(qa, qg, sy, sx)), np.sort(directed(qg, qa, sy, sx))))
            self.d.append(per)

    def min_gap(self, tolerances) -> np.ndarray:
        """[B]: the smallest |d - tol| / tol over the finite distances of an image and the tolerances (inf if there are none)."""
        out = np.full(self.B, np.inf)
        for b in range(self.B):
            for c in range(self.C):
                for d in self.d[b][c]:
                    d = d[np.isfinite(d)]
                    for t in tolerances:
                        if d.size and t > 0:
                            out[b] = min(out[b], float(np.abs(d - t).min() / t))
        return out

    def stats(self, tolerances, q=(95, 100)):
        """counts int64 [B, C, 2, 1 + T], values float64 [B, C, 2, 3] = (sum, max, k-th smallest), e_values: the fp32 bound of each."""
        T = len(tolerances)
        counts = np.zeros((self.B, self.C, 2, 1 + T), dtype=np.int64)
        values = np.zeros((self.B, self.C, 2, 3))
        bound = np.zeros((self.B, self.C, 2, 3))
        for b in range(self.B):
            for c in range(self.C):
                for k, d in enumerate(self.d[b][c]):
                    n = len(d)
                    counts[b, c, k, 0] = n
                    if n == 0 or not np.isfinite(d[0]):      # no query border, or nothing on the other side: zeros
                        continue
                    rank = (n * int(q[0]) + int(q[1]) - 1) // int(q[1])          # ceil in integers
                    counts[b, c, k, 1:] = [(d <= np.float64(np.float32(t))).sum() for t in tolerances]
                    values[b, c, k] = (d.sum(), d[-1], d[rank - 1])
                    bound[b, c, k] = ((REL + gam(n) * (1 + REL)) * d.sum(), REL * d[-1], REL * d[rank - 1])
        return counts, values, bound


def metrics(counts: np.ndarray, values: np.ndarray, spacing: np.ndarray, shape):
    """Per image and class from the per-direction outputs: dict of hd95 (the quantile asked for), hd, assd [B, C] and nsd [B, C, T],
    float64.  Both borders empty: NaN.  One empty: the distance metrics take the image diagonal in mm, NSD 0."""
    counts, values = np.asarray(counts, dtype=np.float64), np.asarray(values, dtype=np.float64)
    sp = np.asarray(spacing, dtype=np.float64).reshape(-1, 2)
    H, W = shape
    diag = np.sqrt((sp[:, 0] * H) ** 2 + (sp[:, 1] * W) ** 2)[:, None]
    nA, nG = counts[:, :, 0, 0], counts[:, :, 1, 0]
    absent, one = (nA == 0) & (nG == 0), (nA == 0) ^ (nG == 0)
    den = np.maximum(nA + nG, 1)

    def pick(x):
        x = np.where(one, diag, x)
        return np.where(absent, np.nan, x)

    nsd = (counts[:, :, 0, 1:] + counts[:, :, 1, 1:]) / den[..., None]
    nsd = np.where(one[..., None], 0.0, nsd)
    return {"hd95": pick(np.maximum(values[:, :, 0, 2], values[:, :, 1, 2])), "hd": pick(np.maximum(values[:, :, 0, 1], values[:, :, 1, 1])),
            "assd": pick((values[:, :, 0, 0] + values[:, :, 1, 0]) / den), "nsd": np.where(absent[..., None], np.nan, nsd)}
