"""Patch-based segmentation training at native resolution: the host side of csrc/segpatch.hip (nnU-Net's patch sampling).

    pool = PatchPool(images, masks, spacings, device="cuda")                       # the training set crosses to the device once
    d = draw_patch_jobs(pool, 16, gen, S=224, t=224, fg_prob=0.33, rotate_deg=15, scale_range=(0.7, 1.4))
    x, m = ops.seg_patch_sample(pool.img, pool.msk, d["jobs"], d["par"], 224, MEAN, STD)

A job is an inverse affine map from the S x S output grid into one source plane (include/dinox.h): ``patch_matrix`` builds it from a
centre, a tile side t, a scale, an angle and two mirrors; ``draw_patch_jobs`` draws B of them on the host from one ``torch.Generator``
with foreground-oversampled centres.  Everything here but the kernel launch runs without a GPU.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_LOCATIONS = 4096                 # pixel locations kept per sample and class (nnU-Net's class_locations)
IGNORE = 255
DRAW_COLUMNS = ("sample", "foreground", "class_or_row", "location_or_column", "angle", "scale", "mirror_x", "mirror_y", "gamma_on", "gamma",
                "gain_on", "gain")


class PatchPool:
    """The training images and masks on the device once -- ``img`` fp32 [sum H W] (planes already windowed to [0, 1]) and ``msk`` uint8
    [sum H W], plane i at element ``offsets[i]`` of both -- and on the host the tables ``offsets`` int64 [n], ``sizes`` int64 [n, 2] =
    (H, W), ``spacings`` float64 [n, 3] = (sx, sy, sz) in mm and ``locations``: per sample a dict class -> at most 4096 flat pixel
    indices of that class (ascending), drawn once with ``seed`` from ``np.flatnonzero``; 255 (ignore) is no class.  A pool above
    ``max_gib`` GiB is refused before anything is allocated."""

    def __init__(self, images: Sequence, masks: Sequence, spacings: Optional[Sequence] = None, device="cuda", max_gib: float = 16.0,
                 seed: int = 0) -> None:
        n = len(images)
        if n < 1 or len(masks) != n or (spacings is not None and len(spacings) != n):
            raise ValueError(f"PatchPool: {n} images, {len(masks)} masks, {None if spacings is None else len(spacings)} spacings")
        sizes = []
        for i, (a, b) in enumerate(zip(images, masks)):
            if a.ndim != 2 or tuple(a.shape) != tuple(b.shape) or min(a.shape) < 1:
                raise ValueError(f"PatchPool: sample {i}: image {tuple(a.shape)} and mask {tuple(b.shape)} must be equal (H, W) planes")
            sizes.append((int(a.shape[0]), int(a.shape[1])))
        self.sizes = np.asarray(sizes, dtype=np.int64)
        area = self.sizes[:, 0] * self.sizes[:, 1]
        total = int(area.sum())
        gib = 5 * total / 2 ** 30                               # 4 bytes of image and 1 of mask per pixel
        if not gib <= max_gib:
            raise ValueError(f"PatchPool: {n} planes of {total} pixels need {gib:.2f} GiB on the device, above max_gib = {max_gib:g}; "
                             "train on a subset or raise the limit")
        self.offsets = np.concatenate([[0], np.cumsum(area)[:-1]]).astype(np.int64)
        self.spacings = np.ones((n, 3)) if spacings is None else np.asarray(spacings, dtype=np.float64).reshape(n, 3)
        if not (np.isfinite(self.spacings).all() and (self.spacings > 0).all()):
            raise ValueError("PatchPool: spacings must be finite and > 0")
        img = torch.empty(total, dtype=torch.float32)
        msk = torch.empty(total, dtype=torch.uint8)
        rng = np.random.default_rng(seed)
        self.locations: List[Dict[int, np.ndarray]] = []
        for i, (a, b) in enumerate(zip(images, masks)):
            o, k = int(self.offsets[i]), int(area[i])
            mk = torch.as_tensor(b)
            if mk.dtype != torch.uint8:
                raise ValueError(f"PatchPool: sample {i}: the mask must be uint8 class indices (255 = ignore), got {mk.dtype}")
            img[o:o + k] = torch.as_tensor(a, dtype=torch.float32).reshape(-1)
            msk[o:o + k] = mk.reshape(-1)
            flat = mk.reshape(-1).numpy()
            loc = {}
            for c in np.unique(flat):
                if c == IGNORE:
                    continue
                idx = np.flatnonzero(flat == c)
                if idx.size > MAX_LOCATIONS:
                    idx = np.sort(rng.choice(idx, MAX_LOCATIONS, replace=False))
                loc[int(c)] = idx.astype(np.int64)
            self.locations.append(loc)
        self.device = torch.device(device)
        self.img, self.msk = img.to(self.device), msk.to(self.device)

    def __len__(self) -> int:
        return self.sizes.shape[0]

    def foreground_classes(self, i: int) -> List[int]:
        """The classes a foreground-centred job of sample i chooses from: those present, background (0) left out if any other is."""
        cs = sorted(self.locations[i])
        return [c for c in cs if c != 0] or cs


def patch_matrix(center_yx: Tuple[float, float], t: int, S: int, scale: float = 1.0, angle_rad: float = 0.0, mirror_x: bool = False,
                 mirror_y: bool = False) -> np.ndarray:
    """The fp32 2 x 3 matrix [[a00, a01, a02], [a10, a11, a12]] of a job: (sx, sy)^T = A (dx, dy)^T + (a02, a12)^T with
    A = (scale t / S) R(angle) diag(mirror_x ? -1 : 1, mirror_y ? -1 : 1), R = [[cos, -sin], [sin, cos]].  One output pixel is
    scale t / S source pixels (scale > 1: a larger field of view, structures appear smaller).  ``center_yx`` = (cy, cx) is a source
    PIXEL: its centre (cx + 0.5, cy + 0.5) is the image of the centre of output pixel (S // 2, S // 2), whose centred coordinates are
    d0 = S // 2 + 0.5 - S / 2 on both axes.  Computed in float64, rounded once."""
    if not (S >= 1 and t >= 1 and scale > 0 and math.isfinite(scale) and math.isfinite(angle_rad)):
        raise ValueError(f"patch_matrix: S = {S!r}, t = {t!r}, scale = {scale!r}, angle = {angle_rad!r}")
    k = float(scale) * t / S
    c, s = math.cos(angle_rad), math.sin(angle_rad)
    mx, my = (-1.0 if mirror_x else 1.0), (-1.0 if mirror_y else 1.0)
    a00, a01, a10, a11 = k * c * mx, -k * s * my, k * s * mx, k * c * my
    d0 = S // 2 + 0.5 - S / 2
    cy, cx = center_yx
    return np.array([[a00, a01, cx + 0.5 - (a00 + a01) * d0], [a10, a11, cy + 0.5 - (a10 + a11) * d0]], dtype=np.float32)


def _check_range(name: str, r, lo_min: float = 0.0) -> Tuple[float, float]:
    lo, hi = (float(v) for v in r)
    if not (math.isfinite(lo) and math.isfinite(hi) and lo_min < lo <= hi):
        raise ValueError(f"draw_patch_jobs: {name} = ({lo}, {hi}) must be finite with {lo_min:g} < lo <= hi")
    return lo, hi


def draw_patch_jobs(pool: PatchPool, batch_size: int, gen: torch.Generator, *, S: int, t: int, fg_prob: float = 0.33, rotate_deg: float = 15.0,
                    scale_range=(0.7, 1.4), gamma_range=(0.7, 1.5), gamma_prob: float = 0.3, gain_range=(0.75, 1.25), gain_prob: float = 0.15,
                    mirror: bool = True) -> dict:
    """``batch_size`` jobs for ``ops.seg_patch_sample``, drawn on the host.  ``S``, the side of the output grid, is a keyword of its
    own beside the tile side ``t`` because the matrix maps the S x S grid onto t source pixels (``patch_matrix`` needs both).  Two
    spacings come back, not one: the label grid's, and the one the model is told -- they differ by the factor t / S (see below).  ONE call ``torch.rand((B, 12), float64, generator=gen)``
    supplies every draw; row b, columns in the order of ``DRAW_COLUMNS``:
      0 sample = floor(r n);  1 foreground-centred if r < fg_prob;  2, 3 the centre -- foreground: class = classes[floor(r2 k)] of the
      sample's ``foreground_classes`` and location = locations[class][floor(r3 len)]; otherwise (or if the sample has no labelled pixel)
      the uniform pixel (floor(r2 H), floor(r3 W));  4 angle = (2 r - 1) rotate_deg;  5 scale = lo + r (hi - lo);  6, 7 mirror along
      x / y if r < 0.5 (and ``mirror``);  8, 9 gamma = lo + r9 (hi - lo) if r8 < gamma_prob else 1;  10, 11 gain alike, else 1.
    Returns {"jobs" int64 [B, 4], "par" fp32 [B, 8], "grid_spacing" fp32 [B, 2], "model_spacing" fp32 [B, 3], "sample" int64 [B],
    "center" int64 [B, 2] = (cy, cx), "fg_class" int64 [B] (-1: a uniform centre)} as host arrays.
    ``grid_spacing`` = (s_y, s_x) in mm per OUTPUT pixel: the sample's (sy, sx) times the lengths of the matrix columns (a11, a01) and
    (a00, a10) -- what --boundary-units mm measures in.  ``model_spacing`` = (sx, sy, sz) as a scale-aware model is told: tiled
    inference (dinox.tiled) tells the model the series' own spacing for a tile of ANY side t, so a job tells it the sample's spacing
    times the augmentation's zoom alone, (sx |col 0| S / t, sy |col 1| S / t, sz); at scale 1 that is the series' own."""
    B, n = int(batch_size), len(pool)
    if B < 1 or S < 1 or t < 1:
        raise ValueError(f"draw_patch_jobs: batch_size = {batch_size!r}, S = {S!r}, t = {t!r} must be >= 1")
    for what, p in (("fg_prob", fg_prob), ("gamma_prob", gamma_prob), ("gain_prob", gain_prob)):
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"draw_patch_jobs: {what} = {p!r} must lie in [0, 1]")
    if not (math.isfinite(rotate_deg) and 0 <= rotate_deg <= 180):
        raise ValueError(f"draw_patch_jobs: rotate_deg = {rotate_deg!r} must lie in [0, 180]")
    s_lo, s_hi = _check_range("scale_range", scale_range)
    g_lo, g_hi = _check_range("gamma_range", gamma_range)
    n_lo, n_hi = _check_range("gain_range", gain_range)
    r = torch.rand((B, len(DRAW_COLUMNS)), dtype=torch.float64, generator=gen).numpy()
    jobs, par = np.empty((B, 4), np.int64), np.empty((B, 8), np.float32)
    grid, model = np.empty((B, 2), np.float32), np.empty((B, 3), np.float32)
    sample, center, fg_class = np.empty(B, np.int64), np.empty((B, 2), np.int64), np.full(B, -1, np.int64)
    for b in range(B):
        i = min(int(r[b, 0] * n), n - 1)
        H, W = (int(v) for v in pool.sizes[i])
        classes = pool.foreground_classes(i)
        if r[b, 1] < fg_prob and classes:
            c = classes[min(int(r[b, 2] * len(classes)), len(classes) - 1)]
            loc = pool.locations[i][c]
            cy, cx = divmod(int(loc[min(int(r[b, 3] * loc.size), loc.size - 1)]), W)
            fg_class[b] = c
        else:
            cy, cx = min(int(r[b, 2] * H), H - 1), min(int(r[b, 3] * W), W - 1)
        angle = math.radians((2.0 * r[b, 4] - 1.0) * rotate_deg)
        scale = s_lo + r[b, 5] * (s_hi - s_lo)
        A = patch_matrix((cy, cx), t, S, scale, angle, mirror and r[b, 6] < 0.5, mirror and r[b, 7] < 0.5)
        gamma = g_lo + r[b, 9] * (g_hi - g_lo) if r[b, 8] < gamma_prob else 1.0
        gain = n_lo + r[b, 11] * (n_hi - n_lo) if r[b, 10] < gain_prob else 1.0
        jobs[b] = (pool.offsets[i], pool.offsets[i], H, W)
        par[b, :6], par[b, 6], par[b, 7] = A.reshape(-1), gamma, gain
        sx, sy, sz = pool.spacings[i]
        col0, col1 = math.hypot(float(A[0, 0]), float(A[1, 0])), math.hypot(float(A[0, 1]), float(A[1, 1]))
        grid[b] = (sy * col1, sx * col0)
        model[b] = (sx * col0 * S / t, sy * col1 * S / t, sz)
        sample[b], center[b] = i, (cy, cx)
    return {"jobs": jobs, "par": par, "grid_spacing": grid, "model_spacing": model, "sample": sample, "center": center, "fg_class": fg_class}
