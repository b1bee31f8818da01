"""The seeded launches of tests/test_segpatch_gpu.py, built here so that tests/test_segpatch_cpu.py can run the oracle and the fp32 emulation
over the very same cases without a GPU.  Everything is NumPy; inputs are shared between tests and must not be written to.

Pool: planes of 1 x 1, 5 x 97, 64 x 64 and 33 x 130 with guard elements (NaN in the image pool, 0xAB in the mask pool) before, between and
after them; the guard runs are sized so that every plane's offset is odd in both pools and differs between them (image 3, 9, 501, 4599;
mask 1, 11, 499, 4601): no alignment can be relied on, and a swap of the two offsets of a job reads the wrong elements on every plane.
A launch is (S, B, first kind): job i is of kind (first + i) mod 21 on plane i mod 4.  S = 16, 28, 70: a run shorter than, no multiple of
and longer than a wave; B = 1, 3, 17.  The three B = 17 launches start at kinds 0, 7 and 14, so each S sees every kind.
"""
import functools
import math

import numpy as np

import _segpatch_oracle as O

SHAPES = ((1, 1), (5, 97), (64, 64), (33, 130))
GUARDS_IMG, GUARDS_MSK = (3, 5, 7, 2, 9), (1, 9, 3, 6, 11)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CLASSES = 4
KINDS = ("identity", "shift", "mirror_x", "mirror_y", "turn1", "turn2", "turn3", "affine0", "affine1", "affine2", "affine3", "affine4",
         "far", "zero", "over_left", "over_right", "over_top", "over_bottom", "gamma0", "gamma1", "gamma_identity")
LAUNCHES = tuple((S, B, first) for S in (16, 28, 70) for B, first in ((1, 7 + S % 5), (3, 16), (17, {16: 0, 28: 7, 70: 14}[S])))


@functools.lru_cache(maxsize=None)
def pool():
    """(planes, img_pool float32, msk_pool uint8, offsets_img, offsets_msk): the planes are views of nothing -- copies, read-only."""
    rng = np.random.default_rng(20240)
    planes, img_parts, msk_parts, oi, om = [], [], [], [], []
    ni = nm = 0
    for k, (H, W) in enumerate(SHAPES):
        img = rng.random((H, W), dtype=np.float32)
        msk = rng.integers(0, CLASSES, size=(H, W)).astype(np.uint8)
        msk[rng.random((H, W)) < 0.05] = 255
        img.setflags(write=False)
        msk.setflags(write=False)
        planes.append((img, msk))
        img_parts += [np.full(GUARDS_IMG[k], np.nan, np.float32), img.reshape(-1)]
        msk_parts += [np.full(GUARDS_MSK[k], 0xAB, np.uint8), msk.reshape(-1)]
        ni, nm = ni + GUARDS_IMG[k], nm + GUARDS_MSK[k]
        oi.append(ni)
        om.append(nm)
        ni, nm = ni + H * W, nm + H * W
    img_parts.append(np.full(GUARDS_IMG[-1], np.nan, np.float32))
    msk_parts.append(np.full(GUARDS_MSK[-1], 0xAB, np.uint8))
    return planes, np.concatenate(img_parts), np.concatenate(msk_parts), oi, om


def _rot(k, angle, mx=1.0, my=1.0):
    c, s = math.cos(angle), math.sin(angle)
    return k * c * mx, -k * s * my, k * s * mx, k * c * my


def job_par(kind, H, W, S, rng):
    """float32 [8] of one job.  The exact kinds keep every coordinate on a half-integer, far from the integers where a label flips."""
    h = S / 2
    g, gain = 1.0, 1.0
    if kind in ("identity", "gamma_identity"):
        a = (1, 0, h, 0, 1, h)
        if kind == "gamma_identity":
            g, gain = 1.5, 0.8
    elif kind == "shift":
        a = (1, 0, h + 3, 0, 1, h - 2)
    elif kind == "mirror_x":
        a = (-1, 0, h, 0, 1, h)
    elif kind == "mirror_y":
        a = (1, 0, h, 0, -1, h)
    elif kind.startswith("turn"):
        q = int(kind[-1])
        c, s = (0, -1, 0)[q - 1], (1, 0, -1)[q - 1]
        a = (c, -s, h, s, c, h)
    elif kind.startswith("affine") or kind.startswith("gamma"):
        k, ang = math.exp(rng.uniform(math.log(0.5), math.log(2.0))), rng.uniform(-math.pi, math.pi)
        a00, a01, a10, a11 = _rot(k, ang, rng.choice([-1.0, 1.0]), rng.choice([-1.0, 1.0]))
        a = (a00, a01, rng.uniform(0, W), a10, a11, rng.uniform(0, H))
        if kind.startswith("gamma"):
            g, gain = rng.uniform(0.7, 1.5), rng.uniform(0.75, 1.25)
    elif kind == "far":
        a = (1, 0, 1e5 + h, 0, 1, -3e5 + h)
    elif kind == "zero":
        a = (0, 0, 0.37 * W, 0, 0, 0.61 * H)
    else:                                                   # a tile hanging over one edge, slightly scaled and turned
        cx, cy = {"over_left": (0.0, H / 2), "over_right": (float(W), H / 2), "over_top": (W / 2, 0.0), "over_bottom": (W / 2, float(H))}[kind]
        a00, a01, a10, a11 = _rot(min(1.1, 1.1 * min(H, W) / S * 2), 0.1)
        a = (a00, a01, cx + 0.013, a10, a11, cy + 0.021)
    return np.array([*a, g, gain], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def launch(i):
    """-> dict(S, B, plane_of, jobs int64 [B, 4], par float32 [B, 8], pad, kinds, want: the float64 oracle's Result)."""
    S, B, first = LAUNCHES[i]
    planes, _, _, oi, om = pool()
    rng = np.random.default_rng(700 + i)
    kinds = [KINDS[(first + j) % len(KINDS)] for j in range(B)]
    plane_of = [(j + i) % len(SHAPES) for j in range(B)]
    par = np.stack([job_par(kinds[j], *SHAPES[plane_of[j]], S, rng) for j in range(B)])
    jobs = np.array([[oi[p], om[p], *SHAPES[p]] for p in plane_of], dtype=np.int64)
    pad = (0.0, 0.25, -0.5)[i % 3]
    want = O.sample64(planes, plane_of, par, S, MEAN, STD, pad)
    return dict(S=S, B=B, plane_of=plane_of, jobs=jobs, par=par, pad=pad, kinds=kinds, want=want)


def pow_launch():
    """Integer shifts of the 64 x 64 plane (every v is a plane value, exact), mean 0 and std 1 (x is v' itself): what powf and the
    product with gain leave is read off x directly."""
    planes, _, _, oi, om = pool()
    S = 28
    g = np.array([0.7, 1.5, 2.2, 0.45], dtype=np.float32)
    gain = np.array([1.0, 0.8, 1.25, 1.0], dtype=np.float32)
    par = np.stack([np.array([1, 0, S / 2 + 3 * j, 0, 1, S / 2 + 5 * j, g[j], gain[j]], dtype=np.float32) for j in range(4)])
    jobs = np.array([[oi[2], om[2], 64, 64]] * 4, dtype=np.int64)
    return dict(S=S, B=4, plane_of=[2] * 4, jobs=jobs, par=par, pad=0.0)
