"""Host side of the iBOT masked-patch objective (an extension; iBOT, Zhou et al. 2022 / DINOv2): which patches of which global
views the student sees as ``mask_token``.

Masks are drawn on the host from a ``numpy.random.Generator`` of the generator's own, so the draws of the views, of the model
initialisation and of torch's generators do not move when the objective is switched on.  Per global view:

* with probability ``mask_prob`` the view is masked, otherwise it contributes nothing;
* a masked view gets a ratio r ~ U(ratio_min, ratio_max) and a target n = max(1, round(r P)) of its P = g x g patches;
* rectangles are placed as in BEiT / iBOT block masking: area a ~ U(4, remaining budget), aspect log-uniform in [0.3, 1 / 0.3], height
  round(sqrt(a * aspect)), width round(sqrt(a / aspect)), a uniform position; a rectangle is accepted when it fits the grid and adds between
  1 and the remaining budget of new patches; 10 attempts per rectangle, and placement ends with the first rectangle that found no place
  (or when fewer than 4 patches are left to spend);
* single patches drawn without replacement top the count up to exactly n.

``PatchMask`` holds what the kernels take: ``idx`` (int32, flat positions v * P + i, distinct, ascending), ``w`` (fp32, 1 / n_v of the
row's view: every masked view weighs the same in the loss) and ``tok`` (int32, the row v * N + 1 + i of the [V, N, D] token matrix,
N = 1 + P + registers).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

MIN_BLOCK = 4                    # patches of the smallest rectangle
ASPECT = (0.3, 1.0 / 0.3)        # log-uniform aspect range
ATTEMPTS = 10                    # per rectangle
SEED_STREAM = 0x1B07             # spawn key: the masks' stream of --train-seed, apart from every other use of the seed


@dataclass
class PatchMask:
    """idx, w, tok as described in the module docstring; host NumPy arrays from the generator, device tensors after ``to``."""
    idx: object
    w: object
    tok: object
    n_views: int
    patches: int

    @property
    def count(self) -> int:
        return int(self.idx.shape[0])

    def to(self, device) -> "PatchMask":
        """Device copies staged through page-locked memory (asynchronous, like the view parameters); an empty mask stays on the host."""
        if self.count == 0 or isinstance(self.idx, torch.Tensor):
            return self
        dev = torch.device(device)

        def up(a):
            t = torch.from_numpy(np.ascontiguousarray(a))
            return t.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" else t.to(dev)
        return PatchMask(up(self.idx), up(self.w), up(self.tok), self.n_views, self.patches)

    def triple(self) -> Tuple[object, object, object]:
        return self.idx, self.w, self.tok


def block_mask(rng: np.random.Generator, grid: int, n: int) -> np.ndarray:
    """A boolean [grid, grid] mask with exactly ``n`` patches set (1 <= n <= grid^2)."""
    P = grid * grid
    if not 1 <= n <= P:
        raise ValueError(f"cannot mask {n} of {P} patches")
    mask = np.zeros((grid, grid), dtype=bool)
    count = 0
    lo, hi = math.log(ASPECT[0]), math.log(ASPECT[1])
    while n - count >= MIN_BLOCK:
        budget = n - count
        placed = 0
        for _ in range(ATTEMPTS):
            area = rng.uniform(MIN_BLOCK, budget)
            aspect = math.exp(rng.uniform(lo, hi))
            h, w = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
            if not (1 <= h <= grid and 1 <= w <= grid):
                continue
            top, left = int(rng.integers(0, grid - h + 1)), int(rng.integers(0, grid - w + 1))
            new = h * w - int(mask[top:top + h, left:left + w].sum())
            if 0 < new <= budget:
                mask[top:top + h, left:left + w] = True
                placed = new
                break
        if placed == 0:
            break
        count += placed
    if count < n:
        free = np.flatnonzero(~mask.reshape(-1))
        mask.reshape(-1)[rng.choice(free, size=n - count, replace=False)] = True
    return mask


class MaskGenerator:
    """``draw(V)`` gives the PatchMask of one step's V global views; a function of (seed, number of draws so far) alone."""

    def __init__(self, seed: int, grid: int, registers: int = 0, mask_prob: float = 0.5, ratio: Tuple[float, float] = (0.1, 0.5)) -> None:
        lo, hi = float(ratio[0]), float(ratio[1])
        if not 0.0 <= mask_prob <= 1.0:
            raise ValueError(f"mask_prob must lie in [0, 1], got {mask_prob}")
        if not 0.0 < lo <= hi <= 1.0:
            raise ValueError(f"mask ratio must satisfy 0 < MIN <= MAX <= 1, got {lo} {hi}")
        if grid < 1:
            raise ValueError(f"grid must be >= 1, got {grid}")
        self.grid, self.registers, self.mask_prob, self.ratio = int(grid), int(registers), float(mask_prob), (lo, hi)
        self.rng = np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(seed), spawn_key=(SEED_STREAM,))))

    def draw(self, n_views: int) -> PatchMask:
        P = self.grid * self.grid
        N = 1 + P + self.registers
        idx, w = [], []
        for v in range(n_views):
            if not self.rng.random() < self.mask_prob:
                continue
            r = self.rng.uniform(*self.ratio)
            n = min(P, max(1, int(round(r * P))))
            cells = np.flatnonzero(block_mask(self.rng, self.grid, n).reshape(-1))
            idx.append(v * P + cells)
            w.append(np.full(n, 1.0 / n, dtype=np.float32))
        return make_mask(np.concatenate(idx) if idx else np.zeros(0, np.int64), n_views, P, self.registers,
                         np.concatenate(w) if w else None)

    def state(self) -> dict:
        return self.rng.bit_generator.state

    def set_state(self, state: dict) -> None:
        self.rng.bit_generator.state = state


def make_mask(flat_idx, n_views: int, patches: int, registers: int = 0, w: Optional[np.ndarray] = None) -> PatchMask:
    """A PatchMask from flat patch positions v * P + i (any order; must be distinct and in range): sorted, with w = 1 / n_v and the
    token rows."""
    idx = np.sort(np.asarray(flat_idx, dtype=np.int64).reshape(-1))
    if idx.size and (idx[0] < 0 or idx[-1] >= n_views * patches or np.any(np.diff(idx) == 0)):
        raise ValueError("masked patch positions must be distinct and inside [0, V * P)")
    v, i = idx // patches, idx % patches
    if w is None:
        per_view = np.bincount(v, minlength=n_views)
        w = (1.0 / per_view[v]).astype(np.float32) if idx.size else np.zeros(0, np.float32)
    tok = v * (1 + patches + registers) + 1 + i
    return PatchMask(idx.astype(np.int32), np.asarray(w, dtype=np.float32), tok.astype(np.int32), int(n_views), int(patches))
