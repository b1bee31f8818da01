"""Training monitor: what a checkpoint (or the student in the middle of a run) looks at, and whether its embeddings collapse.

Counterpart of the reference's monitoring (``make_attention_heatmap`` of scripts/phase5_big_run.py:85-113, called every
``--monitor-every`` steps at :1893-1906, and the statistics of scripts/phase5_monitor.py:245-252).  The reference can draw only a
patch-token-norm proxy, because its fused SDPA returns no probabilities; here ``PatchViT.last_attention`` reads the CLS softmax rows of
the last block from the packed qkv rows (``csrc/attention_rows.hip``), so the monitor writes the proxy AND the attention itself, and on
request the attention rollout of CLS through every block (``PatchViT.attention_rollout``, ``csrc/attention_rollout.hip``).

``run_monitor`` is one no-grad forward (two with ``rollout=True``, plus the rollout chain): it draws no random number, writes no
parameter, centre or optimiser state and issues no collective, so a training run with and without it is bit-identical.  Under a
captured training step (``TrainEngine(use_graph=True)``, ``--hip-graph``) nothing of it is part of the graph: the caller runs it after
a step, eagerly, between two replays, on buffers of its own, and the cached weight images are dropped around it (see ``run_monitor``).
"""
from __future__ import annotations

import json
import math
import os
from typing import Optional

import numpy as np
import torch

from . import ops

__all__ = ["patch_norm_heatmap", "embedding_stats", "attention_entropy", "first_images", "run_monitor"]


def patch_norm_heatmap(feats: torch.Tensor, n_patches: int) -> torch.Tensor:
    """The reference's heatmap (make_attention_heatmap): L2 norm of the patch tokens 1 .. P of feats [B, T, D] (CLS and registers
    skipped), (x - min) / (max - min + 1e-8) per image, as [B, g, g] fp32 on the device of ``feats``."""
    g = int(round(math.sqrt(n_patches)))
    if feats.dim() != 3 or g * g != n_patches or feats.shape[1] < 1 + n_patches:
        raise ValueError(f"feats {tuple(feats.shape)} is not [B, T >= 1 + {n_patches}, D] with a square number of patches")
    norms = torch.norm(feats[:, 1:1 + n_patches, :].float(), dim=-1)
    lo, hi = norms.amin(1, keepdim=True), norms.amax(1, keepdim=True)
    return ((norms - lo) / (hi - lo + 1e-8)).reshape(feats.shape[0], g, g)


def embedding_stats(cls: torch.Tensor) -> dict:
    """Collapse statistics of CLS embeddings [B, D] (scripts/phase5_monitor.py:245-247): ``embedding_std_mean`` is the unbiased
    standard deviation over the batch, averaged over the features (NaN for a single row, as torch gives it); ``embedding_norm_mean``
    the mean L2 norm."""
    if cls.dim() != 2 or cls.shape[0] < 1:
        raise ValueError(f"cls must be [B >= 1, D], got {tuple(cls.shape)}")
    E = cls.float()
    return {"embedding_std_mean": float(E.std(dim=0).mean()), "embedding_norm_mean": float(E.norm(dim=-1).mean())}


def attention_entropy(probs: torch.Tensor) -> torch.Tensor:
    """Entropy in nats of every row of probs [..., T] (0 log 0 = 0): log T for a uniform row, 0 for a one-hot one."""
    p = probs.float()
    return -(torch.where(p > 0, p * torch.log(p.clamp_min(1e-45)), torch.zeros_like(p))).sum(-1)


def first_images(batch, n: int):
    """-> (the first min(n, B) images of a training batch in the form the model takes, channel 1 -- the middle slice -- of image 0 as
    an [S, S] tensor).  ``batch`` is the [B, 3, S, S] image tensor or, under --gpu-views, the unfolded ``ops.PatchOperand`` (rows
    (image, gy, gx), columns (channel, py, px)), of which the leading rows are taken without a copy."""
    n = min(int(n), batch.shape[0])
    if isinstance(batch, ops.PatchOperand):
        p, S = batch.patch, batch.size
        g = S // p
        sub = ops.PatchOperand(batch.u[:n * g * g], n, S, p)
        plane = batch.u[:g * g, :3 * p * p].float().reshape(g, g, 3, p, p)[:, :, 1].permute(0, 2, 1, 3).reshape(S, S)
        return sub, plane
    return batch[:n], batch[0, 1].float()


def _save_png(arr: np.ndarray, path: str, size: Optional[int] = None) -> None:
    try:
        from PIL import Image
    except Exception:
        return
    lo, hi = float(arr.min()), float(arr.max())
    img = Image.fromarray((np.clip((arr - lo) / (hi - lo + 1e-8), 0.0, 1.0) * 255.0).astype(np.uint8))
    if size is not None and img.size != (size, size):
        img = img.resize((size, size), resample=Image.NEAREST)
    img.save(path)


def run_monitor(backbone, batch, spacing, out_dir, step: int, input_plane: Optional[torch.Tensor] = None, extra: Optional[dict] = None,
                rollout: bool = False) -> dict:
    """One no-grad ``backbone.last_attention`` on ``batch`` ([B, 3, S, S] or a PatchOperand; ``spacing`` [B, 3] or None), then
    ``out_dir/step_{step:08d}/`` receives
        heatmap.npy    [g, g]         patch-norm heatmap of image 0 (the reference's picture)
        attention.npy  [heads, g, g]  CLS attention of the last block over the patches of image 0
        input.npy      [S, S]         channel 1 (the middle slice) of image 0
        stats.json     step, embedding_std_mean, embedding_norm_mean (over the B CLS embeddings), attention_entropy (per head, mean over
                       the batch, nats), attention_entropy_max = log T, attention_patch_mass (per head), batch
    and the same three pictures as PNG where PIL imports.  With ``rollout=True`` a second no-grad forward
    (``backbone.attention_rollout``, CLS, residual 0.5, every block) adds
        rollout.npy    [g, g]         attention rollout of CLS over the patches of image 0 (and rollout.png)
    and the stats keys rollout_patch_mass (share of the rollout row that ends on patches, mean over the batch) and rollout_entropy
    (entropy of the row over all T tokens, mean over the batch, nats); with ``rollout=False`` files and keys are exactly the ones above.
    Returns the stats dict plus "dir".  The model's mode is left as it is."""
    B = batch.shape[0]
    if B < 1:
        raise ValueError("run_monitor needs at least one image")
    if input_plane is None:
        _, input_plane = first_images(batch, 1)
    # Per-weight operand images (ops.weight_cache: keyed by a parameter's version) are dropped before and after: a hipGraph replay moves
    # the weights without moving their version, so an image cached by an earlier monitor call would be stale here, and one cached here
    # would be picked up -- and frozen into the graph -- by a capture that follows.  After an eager step the cache is empty anyway.
    ops.weight_cache.clear()
    try:
        feats, probs = backbone.last_attention(batch, spacing, query_tokens=(0,))
        roll = backbone.attention_rollout(batch, spacing)[1] if rollout else None
    finally:
        ops.weight_cache.clear()
    S, P = batch.shape[-1], (batch.shape[-1] // backbone.patch) ** 2
    from zoo.arch import cls_attention_grid, rollout_grid
    heat = patch_norm_heatmap(feats[:1], P)[0]
    grid = cls_attention_grid(probs, P)                                   # [B, heads, g, g]
    stats = {"step": int(step), **embedding_stats(feats[:, 0]),
             "attention_entropy": [float(v) for v in attention_entropy(probs[:, :, 0]).mean(0)],
             "attention_entropy_max": math.log(probs.shape[-1]),
             "attention_patch_mass": [float(v) for v in grid.sum((-1, -2)).mean(0)],
             "batch": int(B)}
    if roll is not None:
        rgrid = rollout_grid(roll, P)                                     # [B, g, g]
        stats["rollout_patch_mass"] = float(rgrid.sum((-1, -2)).mean())
        stats["rollout_entropy"] = float(attention_entropy(roll).mean())
    if extra:
        stats.update(extra)
    d = os.path.join(str(out_dir), f"step_{int(step):08d}")
    os.makedirs(d, exist_ok=True)
    arrays = {"heatmap": heat.cpu().numpy(), "attention": grid[0].cpu().numpy(), "input": input_plane.detach().float().cpu().numpy()}
    if roll is not None:
        arrays["rollout"] = rgrid[0].cpu().numpy()
    for name, a in arrays.items():
        np.save(os.path.join(d, name + ".npy"), a)
    with open(os.path.join(d, "stats.json"), "w") as f:
        json.dump(stats, f, indent=2)
        f.write("\n")
    _save_png(arrays["heatmap"], os.path.join(d, "heatmap.png"), S)
    _save_png(arrays["input"], os.path.join(d, "input.png"))
    _save_png(arrays["attention"].mean(0), os.path.join(d, "attention.png"), S)
    if roll is not None:
        _save_png(arrays["rollout"], os.path.join(d, "rollout.png"), S)
    return dict(stats, dir=d)
