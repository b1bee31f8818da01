"""Label-free view-retrieval evaluation (the protocol of the reference's scripts/phase5_view_retrieval_eval.py) on the engine.

Two augmented views of each of N held-out samples are embedded with the student backbone (CLS row, L2-normalised);
with Q = view-1 rows and K = view-2 rows the score asks how often key i is the nearest (top-1) or among the k nearest
(top-k) keys of query i.  The reference builds S = Q K^T on the host and runs argmax / argpartition over its rows.  Here Q
and K stay on the device and ``ops.retrieval_rank`` (csrc/retrieval.hip) returns, per query, the rank of its positive key
straight from the MFMA accumulators; top-1 is ``rank == 0``, top-k is ``rank < k``.  No N x N array exists.

``metrics_from_ranks`` is a pure host function (NumPy); everything else needs a HIP device.
"""
from __future__ import annotations

from typing import Any, Iterator, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops


def _backbone(student: Any):
    return getattr(student, "backbone", student)


@torch.no_grad()
def _cls_rows(backbone, x: torch.Tensor, spacing: Optional[torch.Tensor]) -> torch.Tensor:
    """Raw CLS rows, fp32 [B, D] (under no_grad the backbone runs the fused inference path)."""
    return backbone(x, spacing=spacing)[:, 0].float().contiguous()


def embed_cls(backbone, x: torch.Tensor, spacing: Optional[torch.Tensor] = None) -> torch.Tensor:
    """L2-normalised CLS embedding of the backbone, fp32 [B, D], computed and normalised on the device
    (``F.normalize(backbone(x, spacing)[:, 0].float(), dim=-1)`` of the reference)."""
    return ops.normalize_rows(_cls_rows(backbone, x, spacing))[0]


def metrics_from_ranks(rank, topk: int = 5, ratio: float = 10.0) -> dict:
    """The reference's metric block from per-query ranks (rank[i] = number of keys placed before the positive of query i):
    ``top1`` = mean(rank == 0), ``topk_acc`` = mean(rank < min(topk, n)), ``random_baseline`` = 1 / n,
    ``ratio_vs_random`` = top1 / baseline, ``passed`` = top1 >= ratio * baseline."""
    r = np.asarray(rank).reshape(-1)
    n = int(r.shape[0])
    if n <= 0:
        raise ValueError("metrics_from_ranks: no queries")
    if topk <= 0:
        raise ValueError("topk must be > 0")
    top1 = float(np.mean(r == 0))
    chance = 1.0 / float(n)
    return {
        "top1": top1,
        "topk_acc": float(np.mean(r < min(int(topk), n))),
        "random_baseline": chance,
        "ratio_vs_random": top1 / chance,
        "passed": bool(top1 >= float(ratio) * chance),
    }


def _view_pairs(dataset, idxs: Sequence[int], batch_size: int) -> Iterator[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]:
    """Batches of (view 1, view 2, spacing) host tensors; items are drawn in the order of ``idxs`` (the draws of the two views come
    from the global RNGs, so the order is part of the protocol)."""
    for lo in range(0, len(idxs), batch_size):
        items = [dataset[i] for i in idxs[lo:lo + batch_size]]
        yield (torch.stack([views[0] for views, _ in items]), torch.stack([views[1] for views, _ in items]),
               torch.stack([spacing for _, spacing in items]))


def embed_views(student, dataset, idxs: Sequence[int], batch_size: int = 64, scale_aware: bool = False, *,
                amp_dtype: Optional[torch.dtype] = None):
    """(Q, K, stats): unit CLS rows of view 1 and view 2 of ``dataset[i]``, i in ``idxs``, fp32 [N, D] on the student's device, and the
    two collapse indicators of the un-normalised view-1 rows -- ``embedding_std_mean`` (per-dimension unbiased standard deviation over
    the samples, averaged over the dimensions) and ``embedding_norm_mean`` -- from running sums, so nothing but Q and K grows with N."""
    bb = _backbone(student)
    anchor = next(bb.parameters())
    ops._need_cuda(anchor)
    n = len(idxs)
    if n <= 0:
        raise ValueError("embed_views: no samples")
    Q = K = None
    s1 = s2 = None                      # float64 sums of x and x^2 per dimension
    norm_sum = 0.0
    was_training = bb.training
    bb.eval()
    try:
        with ops.compute_dtype(amp_dtype or torch.float32):
            at = 0
            for x1, x2, sp in _view_pairs(dataset, idxs, batch_size):
                sp = sp.to(anchor.device, non_blocking=True) if scale_aware else None
                raw = _cls_rows(bb, x1.to(anchor.device, non_blocking=True), sp)
                q, norms = ops.normalize_rows(raw)
                k = embed_cls(bb, x2.to(anchor.device, non_blocking=True), sp)
                if Q is None:
                    Q, K = q.new_empty(n, q.shape[1]), q.new_empty(n, q.shape[1])
                    s1, s2 = raw.new_zeros(q.shape[1], dtype=torch.float64), raw.new_zeros(q.shape[1], dtype=torch.float64)
                Q[at:at + len(q)], K[at:at + len(q)] = q, k
                at += len(q)
                r64 = raw.double()
                s1 += r64.sum(0)
                s2 += (r64 * r64).sum(0)
                norm_sum += float(norms.double().sum())
    finally:
        bb.train(was_training)
    var = ((s2 - s1 * s1 / n) / (n - 1)).clamp_min(0.0) if n > 1 else torch.zeros_like(s1)
    return Q, K, {"embedding_std_mean": float(var.sqrt().mean()), "embedding_norm_mean": norm_sum / n}


def view_retrieval(student, dataset, idxs: Sequence[int], batch_size: int = 64, scale_aware: bool = False, topk: int = 5,
                   ratio: float = 10.0, *, amp_dtype: Optional[torch.dtype] = None) -> dict:
    """embed_views -> ops.retrieval_rank -> metrics_from_ranks: the reference's metrics (``top1``, ``topk_acc``, ``random_baseline``,
    ``ratio_vs_random``, ``passed``) plus ``embedding_std_mean`` / ``embedding_norm_mean``.  ``amp_dtype=torch.bfloat16`` runs the
    backbone in the bf16 mode training uses; the similarity is fp32 either way.

    Raises FloatingPointError when an embedding is not finite: every comparison with a NaN score is false, so a diverged
    checkpoint would otherwise rank every positive first and pass the gate."""
    Q, K, stats = embed_views(student, dataset, idxs, batch_size, scale_aware, amp_dtype=amp_dtype)
    rank, _, _, pos_val = ops.retrieval_rank(Q, K)
    if not bool(torch.isfinite(pos_val).all()) or not bool(torch.isfinite(K).all()):
        raise FloatingPointError("view_retrieval: non-finite embeddings (diverged checkpoint?); no score can be given")
    return {**metrics_from_ranks(rank.cpu().numpy(), topk, ratio), **stats}


# ------------------------------------------------------------------------------------------ deterministic evaluation inputs
EVAL_WINDOW = (40.0, 400.0)             # the reference's fixed soft-tissue window (level, width): scripts/evaluate_panorgan.py:105-106


def eval_view(H: int, W: int):
    """The one deterministic view of an (H, W) slice stack: fixed window level 40 / width 400, the centred square crop of side
    min(H, W), no flip -- the reference's ``EvalDataset`` (scripts/evaluate_panorgan.py:91-168: Resize(img_size, bicubic) of the shorter
    side, CenterCrop(img_size), normalise) restated on the device view kernel: resizing the shorter side to S and cutting the centre
    S x S is cutting the centred min(H, W) square and resizing it to S x S (up to the rounding of the longer side).  Resize parity
    with torchvision is NOT pinned: torchvision is not a dependency; the view kernel is pinned to torch's bicubic antialias kernel
    (DESIGN.md section 8f-2)."""
    from .views import ViewParams
    side = min(H, W)
    return ViewParams(EVAL_WINDOW[0], EVAL_WINDOW[1], (H - side) // 2, (W - side) // 2, side, side, False)


def embed_eval_slices(student, dataset, idxs: Sequence[int], img_size: int, batch_size: int = 64, scale_aware: bool = False, *,
                      amp_dtype: Optional[torch.dtype] = None):
    """(E, spacing): the unit CLS row of the deterministic view (``eval_view``) of ``dataset[i]``, i in ``idxs``, fp32 [N, D] on the
    student's device, and the (N, 3) spacings on the host.  Items follow the raw-stack protocol of the training script's datasets
    (``raw_views = True``): ``(u16 stack (3, H, W) or its three slices, <ignored view draws>, spacing (3,))``.  The stacks go through
    ``dinox.views.make_views`` (one kernel: window, crop, bicubic resize, normalise); every slice is embedded once."""
    from .views import collate_stacks, make_views
    bb = _backbone(student)
    anchor = next(bb.parameters())
    ops._need_cuda(anchor)
    n = len(idxs)
    if n <= 0:
        raise ValueError("embed_eval_slices: no samples")
    E, spacings, at = None, [], 0
    was_training = bb.training
    bb.eval()
    try:
        with ops.compute_dtype(amp_dtype or torch.float32):
            for lo in range(0, n, batch_size):
                items = []
                for i in idxs[lo:lo + batch_size]:
                    stack, _, sp = dataset[i]
                    H, W = (stack.shape[1], stack.shape[2]) if isinstance(stack, np.ndarray) else stack[0].shape
                    items.append((stack, [eval_view(H, W)], sp))
                batch = collate_stacks(items).to(anchor.device)
                e = embed_cls(bb, make_views(batch, img_size), batch.spacing if scale_aware else None)
                if E is None:
                    E = e.new_empty(n, e.shape[1])
                E[at:at + len(e)] = e
                at += len(e)
                spacings.append(batch.spacing.cpu())
    finally:
        bb.train(was_training)
    return E, torch.cat(spacings, 0)
