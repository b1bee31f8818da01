"""Dense label propagation through a volume (Caron et al. 2021, the video-segmentation protocol of DINO, with the z axis of a series as
the sequence): one annotated slice is carried through the series by the affinity of the backbone's patch features alone -- one-shot
volume segmentation, and a head-free score of a checkpoint's dense features.  The per-slice step is ``ops.label_propagate``
(csrc/labelprop.hip); this module holds the bookkeeping around it: the soft labels of a seed, the order of the walk, the ring of
context slices.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import torch

from . import ops


def patch_soft_labels(label_map: torch.Tensor, num_classes: int, patch: int) -> torch.Tensor:
    """fp32 [N, C] of a uint8 label map [S, S] (255 = ignore), N = (S / patch)^2: per patch the share of its non-ignored pixels in each
    class (counts are exact integers, one fp32 division each); an all-ignored patch gives a zero row.  A class index >= C other than 255
    raises ValueError (one device read when the map is on the device).  Computed where the map lives."""
    if not isinstance(label_map, torch.Tensor) or label_map.dtype != torch.uint8 or label_map.dim() != 2 or label_map.shape[0] != label_map.shape[1]:
        raise ValueError(f"patch_soft_labels: label_map must be uint8 [S, S], got {getattr(label_map, 'dtype', type(label_map).__name__)} "
                         f"{tuple(getattr(label_map, 'shape', ()))}")
    C, S = num_classes, label_map.shape[0]
    if isinstance(C, bool) or not isinstance(C, int) or not ops.LABELPROP_MIN_C <= C <= ops.LABELPROP_MAX_C:
        raise ValueError(f"patch_soft_labels: num_classes must be an integer in [{ops.LABELPROP_MIN_C}, {ops.LABELPROP_MAX_C}], got {C!r}")
    if isinstance(patch, bool) or not isinstance(patch, int) or patch < 1 or S < patch or S % patch:
        raise ValueError(f"patch_soft_labels: the side {S} of the label map is not a multiple of patch = {patch!r}")
    lab = label_map.long()
    valid = lab != 255
    bad = valid & (lab >= C)
    if bool(bad.any()):
        raise ValueError(f"patch_soft_labels: label {int(lab[bad].max())} is neither a class in [0, {C}) nor 255 (ignore)")
    g = S // patch
    onehot = torch.zeros((S, S, C), dtype=torch.float32, device=lab.device)
    onehot.scatter_(2, torch.where(valid, lab, torch.zeros_like(lab)).unsqueeze(2), valid.float().unsqueeze(2))
    counts = onehot.view(g, patch, g, patch, C).sum((1, 3)).view(g * g, C)      # integers up to patch^2: exact in fp32
    total = counts.sum(1, keepdim=True)
    return torch.where(total > 0, counts / total.clamp(min=1.0), torch.zeros_like(counts))


def context_schedule(Z: int, seeds, n_context: int) -> Tuple[Dict[int, int], List[Tuple[int, List[int]]]]:
    """The order of the walk, a pure function: (source, steps).  ``source[z]`` is the seed that slice z is propagated from, for every
    non-seed slice: the nearest seed, the lower z on a tie.  ``steps`` lists (target z, context) in processing order -- per seed in
    ascending order, first upwards from it, then downwards -- where context is the seed followed by the up to ``n_context`` most recently
    propagated slices of that walk, nearest last."""
    if isinstance(Z, bool) or not isinstance(Z, int) or Z < 1:
        raise ValueError(f"context_schedule: Z must be an integer >= 1, got {Z!r}")
    if isinstance(n_context, bool) or not isinstance(n_context, int) or n_context < 0:
        raise ValueError(f"context_schedule: n_context must be an integer >= 0, got {n_context!r}")
    seeds = sorted(set(seeds))
    if not seeds or any(isinstance(s, bool) or not isinstance(s, int) or not 0 <= s < Z for s in seeds):
        raise ValueError(f"context_schedule: seeds must be one or more slice indices in [0, {Z}), got {seeds!r}")
    source = {z: min(seeds, key=lambda s: (abs(z - s), s)) for z in range(Z) if z not in seeds}
    steps = []
    for s in seeds:
        for direction in (1, -1):
            done: List[int] = []
            z = s + direction
            while source.get(z) == s:
                steps.append((z, [s] + done[max(0, len(done) - n_context):]))
                done.append(z)
                z += direction
    return source, steps


def propagate_labels(feats: torch.Tensor, seeds: Dict[int, torch.Tensor], num_classes: int, *, patch: int, n_context: int = 7, topk: int = 5,
                     radius: int = 12, temperature: float = 0.1, return_trace: bool = False):
    """Carry the label maps of the seed slices through a volume.  ``feats`` [Z, N, D]: the patch tokens of every slice (any floating
    dtype, on the device; rows are normalised here with ``ops.normalize_rows``); ``seeds``: z -> uint8 label map [S, S] with S = g patch,
    255 = ignore.  Every other slice is reached by walking outwards from its nearest seed (``context_schedule``); its soft labels are
    ``ops.label_propagate`` of its patches against the seed and the ``n_context`` slices before it.  The defaults (5 neighbours, 7 context
    slices, a window of 12 patches, temperature 0.1) are those of the DINO protocol.

    Returns (soft fp32 [Z, N, C], hard uint8 [Z, S, S]), both on the device: hard = ``ops.seg_predict`` of the soft labels (bilinear
    upsampling of the patch probabilities, then argmax); seed slices return their own label map.  With ``return_trace`` a third value: per
    step a dict with "z", "seed", "slots" (the slice held by each context slot, in key order) and the kernel's "idx", "val", "out".

    The context lives in one ring on the device, features [1 + n_context, N, D] and soft labels [1 + n_context, N, C]: slot 0 is the seed,
    a new slice overwrites the oldest of the others, and while the ring fills the call sees its filled prefix -- no per-slice allocation of
    context, and the soft labels never leave the device."""
    if not isinstance(feats, torch.Tensor) or feats.dim() != 3 or not feats.is_floating_point():
        raise ValueError(f"propagate_labels: feats must be a floating-point [Z, N, D] tensor, got {type(feats).__name__} "
                         f"{tuple(getattr(feats, 'shape', ()))}")
    Z, N, D = feats.shape
    g = math.isqrt(N)
    if min(Z, N, D) < 1 or g * g != N:
        raise ValueError(f"propagate_labels: N = {N} patches are not a square grid (feats is {tuple(feats.shape)})")
    if not isinstance(seeds, dict) or not seeds:
        raise ValueError("propagate_labels: seeds must be a non-empty dict z -> uint8 label map [S, S]")
    C, S = num_classes, g * patch
    source, steps = context_schedule(Z, list(seeds), n_context)
    dev = feats.device
    seed_soft = {}
    for z, lab in seeds.items():
        if not isinstance(lab, torch.Tensor) or tuple(lab.shape) != (S, S):
            raise ValueError(f"propagate_labels: the label map of seed {z} must be uint8 [{S}, {S}] (g = {g}, patch = {patch}), got "
                             f"{tuple(getattr(lab, 'shape', ()))}")
        seed_soft[z] = patch_soft_labels(lab.to(dev), C, patch)
    ops._need_cuda(feats)
    unit = ops.normalize_rows(feats.reshape(Z * N, D))[0].view(Z, N, D)
    soft = torch.zeros((Z, N, C), dtype=torch.float32, device=dev)
    for z, s in seed_soft.items():
        soft[z] = s
    ring_f = torch.empty((1 + n_context, N, D), dtype=torch.float32, device=dev)
    ring_s = torch.empty((1 + n_context, N, C), dtype=torch.float32, device=dev)
    trace = []
    slots: List[int] = []
    pushed = 0
    for z, context in steps:
        if len(context) == 1:                                                   # a walk starts: the ring holds its seed alone
            slots, pushed = [context[0]], 0
            ring_f[0].copy_(unit[context[0]])
            ring_s[0].copy_(soft[context[0]])
        assert sorted(slots) == sorted(context), (z, slots, context)
        F = len(slots)
        out, idx, val = ops.label_propagate(unit[z], ring_f[:F].view(F * N, D), ring_s[:F].view(F * N, C), g, K=topk, radius=radius,
                                            temperature=temperature)
        soft[z] = out
        if return_trace:
            trace.append({"z": z, "seed": source[z], "slots": list(slots), "idx": idx, "val": val, "out": out})
        if n_context:
            at = 1 + pushed % n_context                                         # the next free slot, then the oldest
            ring_f[at].copy_(unit[z])
            ring_s[at].copy_(out)
            if at < len(slots):
                slots[at] = z
            else:
                slots.append(z)
            pushed += 1
    hard = ops.seg_predict(soft, patch)
    for z, lab in seeds.items():
        hard[z] = lab.to(dev)
    return (soft, hard, trace) if return_trace else (soft, hard)
