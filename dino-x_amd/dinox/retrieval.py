"""Label-free view-retrieval evaluation (the protocol of the reference's scripts/phase5_view_retrieval_eval.py) on the engine.

Two augmented views of each of N held-out samples are embedded with the student backbone (CLS row, L2-normalised);
with Q = view-1 rows and K = view-2 rows the score asks how often key i is the nearest (top-1) or among the k nearest
(top-k) keys of query i.  The reference builds S = Q K^T on the host and runs argmax / argpartition over its rows.  Here Q
and K stay on the device and ``ops.retrieval_rank`` (csrc/retrieval.hip) returns, per query, the rank of its positive key
straight from the MFMA accumulators; top-1 is ``rank == 0``, top-k is ``rank < k``.  No N x N array exists.

The pan-organ evaluation (scripts/evaluate_panorgan.py) adds the two metrics that need backbone passes of their own: metric 1, the
same protocol per dataset (``view_retrieval_per_dataset``: one embedding pass over the picks of all datasets, one
``ops.retrieval_rank_windowed`` call with each query's window set to its dataset's rows), and metric 3, the spacing counterfactual
(``spacing_counterfactual``: the same pixels embedded with the real, the doubled and the halved spacing, cosine distances from
``ops.row_dots``).

``metrics_from_ranks``, ``per_dataset_picks``, ``per_dataset_metrics_from_ranks`` and ``counterfactual_summary`` are pure host functions
(NumPy); everything else needs a HIP device.
"""
from __future__ import annotations

import random
from typing import Any, Dict, Iterator, List, Optional, Sequence, Tuple

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


def _eval_batches(dataset, idxs: Sequence[int], batch_size: int, device):
    """Device batches (``StackBatch``) of the deterministic view of ``dataset[i]``, i in ``idxs``, in that order: raw-stack items, one
    ``eval_view`` each."""
    from .views import collate_stacks
    for lo in range(0, len(idxs), batch_size):
        items = []
        for i in idxs[lo:lo + batch_size]:
            stack, _, sp = dataset[i]
            H, W = (stack.shape[1], stack.shape[2]) if isinstance(stack, np.ndarray) else stack[0].shape
            items.append((stack, [eval_view(H, W)], sp))
        yield collate_stacks(items).to(device)


def embed_eval_slices(student, dataset, idxs: Sequence[int], img_size: int, batch_size: int = 64, scale_aware: bool = False, *,
                      amp_dtype: Optional[torch.dtype] = None):
    """(E, spacing): the unit CLS row of the deterministic view (``eval_view``) of ``dataset[i]``, i in ``idxs``, fp32 [N, D] on the
    student's device, and the (N, 3) spacings on the host.  Items follow the raw-stack protocol of the training script's datasets
    (``raw_views = True``): ``(u16 stack (3, H, W) or its three slices, <ignored view draws>, spacing (3,))``.  The stacks go through
    ``dinox.views.make_views`` (one kernel: window, crop, bicubic resize, normalise); every slice is embedded once."""
    from .views import make_views
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
            for batch in _eval_batches(dataset, idxs, batch_size, anchor.device):
                e = embed_cls(bb, make_views(batch, img_size), batch.spacing if scale_aware else None)
                if E is None:
                    E = e.new_empty(n, e.shape[1])
                E[at:at + len(e)] = e
                at += len(e)
                spacings.append(batch.spacing.cpu())
    finally:
        bb.train(was_training)
    return E, torch.cat(spacings, 0)


# ------------------------------------------------------------------------------------------ metric 1: per-dataset view retrieval
def per_dataset_picks(labels: Sequence[Optional[str]], n_per_dataset: int = 512, seed: int = 42) -> Tuple[List[str], List[List[int]]]:
    """(names, picks): the reference's sampling (scripts/evaluate_panorgan.py, metric_view_retrieval_per_dataset).  Rows are grouped by
    ``label or "unknown"``; datasets in sorted name order; per dataset a FRESH ``random.Random(seed)`` samples min(n_per_dataset, size)
    positions of the dataset's rows (index order).  ``picks[g]`` holds the row indices of dataset ``names[g]`` in pick order."""
    if n_per_dataset <= 0:
        raise ValueError("n_per_dataset must be > 0")
    groups: Dict[str, List[int]] = {}
    for i, label in enumerate(labels):
        groups.setdefault(label or "unknown", []).append(i)
    names = sorted(groups)
    picks = []
    for name in names:
        rows = groups[name]
        picks.append([rows[j] for j in random.Random(seed).sample(range(len(rows)), k=min(int(n_per_dataset), len(rows)))])
    return names, picks


def per_dataset_metrics_from_ranks(rank, group_sizes: Sequence[int], names: Sequence[str], topk: int = 5) -> dict:
    """{name: {"n", "top1", f"top{topk}", "random_baseline", "ratio_vs_random"}}, names sorted: the reference's per-dataset block from the
    ranks of the concatenated queries (group g owns the next ``group_sizes[g]`` entries of ``rank``; each rank counts keys of the query's
    own group only).  ``top1`` = mean(rank == 0), top-k = mean(rank < min(topk, n)), baseline 1 / n.  There is no ``passed`` key."""
    r = np.asarray(rank).reshape(-1)
    sizes = [int(n) for n in group_sizes]
    if len(sizes) != len(names) or len(set(names)) != len(names):
        raise ValueError("per_dataset_metrics_from_ranks: one distinct name per group expected")
    if any(n <= 0 for n in sizes) or sum(sizes) != r.shape[0]:
        raise ValueError(f"per_dataset_metrics_from_ranks: group sizes {sizes} do not partition {r.shape[0]} ranks")
    if topk <= 0:
        raise ValueError("topk must be > 0")
    starts = np.concatenate([[0], np.cumsum(sizes)])
    out = {}
    for g in sorted(range(len(names)), key=lambda g: names[g]):
        n, rg = sizes[g], r[starts[g]:starts[g + 1]]
        top1 = float(np.mean(rg == 0))
        chance = 1.0 / n
        out[str(names[g])] = {"n": n, "top1": top1, f"top{topk}": float(np.mean(rg < min(int(topk), n))), "random_baseline": chance,
                              "ratio_vs_random": top1 / chance}
    return out


def per_dataset_retrieval_from_embeddings(Q: torch.Tensor, K: torch.Tensor, group_sizes: Sequence[int], names: Sequence[str],
                                          topk: int = 5) -> dict:
    """The per-dataset block from unit rows Q, K [N, D] on the device whose rows are sorted by group: ONE ``ops.retrieval_rank_windowed``
    call, query i against the keys of its own group's row range, then ``per_dataset_metrics_from_ranks``.  Raises FloatingPointError on
    non-finite embeddings, as ``view_retrieval`` does."""
    sizes = torch.as_tensor([int(n) for n in group_sizes], dtype=torch.int64)
    if Q.shape[0] != int(sizes.sum()) or K.shape[0] != Q.shape[0]:
        raise ValueError(f"per_dataset_retrieval_from_embeddings: group sizes {sizes.tolist()} do not partition {Q.shape[0]} rows")
    hi = torch.cumsum(sizes, 0)
    key_lo = torch.repeat_interleave(hi - sizes, sizes).to(Q.device)
    key_hi = torch.repeat_interleave(hi, sizes).to(Q.device)
    rank, _, _, pos_val = ops.retrieval_rank_windowed(Q, K, key_lo, key_hi)
    if not bool(torch.isfinite(pos_val).all()) or not bool(torch.isfinite(K).all()):
        raise FloatingPointError("view_retrieval_per_dataset: non-finite embeddings (diverged checkpoint?); no score can be given")
    return per_dataset_metrics_from_ranks(rank.cpu().numpy(), sizes.tolist(), names, topk)


def view_retrieval_per_dataset(student, dataset, labels: Sequence[Optional[str]], n_per_dataset: int = 512, seed: int = 42, topk: int = 5,
                               batch_size: int = 64, scale_aware: bool = False, *, amp_dtype: Optional[torch.dtype] = None) -> dict:
    """Metric 1 of the pan-organ evaluation: view retrieval per dataset.  ``per_dataset_picks`` (the reference's sampling), then the two
    random views of every pick drawn dataset by dataset, item by item (the reference's order of the global RNG draws), ONE embedding
    pass over the concatenated picks and ONE windowed rank call: no N x N array, no per-dataset kernel loop.  ``dataset[i]`` yields
    ``([view 1, view 2], spacing)`` as for ``view_retrieval``; ``labels[i]`` is the dataset of row i."""
    if len(labels) != len(dataset):
        raise ValueError(f"view_retrieval_per_dataset: {len(labels)} labels for {len(dataset)} rows")
    names, picks = per_dataset_picks(labels, n_per_dataset, seed)
    Q, K, _ = embed_views(student, dataset, [i for p in picks for i in p], batch_size, scale_aware, amp_dtype=amp_dtype)
    return per_dataset_retrieval_from_embeddings(Q, K, [len(p) for p in picks], names, topk)


# ------------------------------------------------------------------------------------------ metric 3: spacing counterfactual
COUNTERFACTUAL_SKIPPED = {"skipped": True, "reason": "baseline model has no scale embedding"}
_COUNTERFACTUAL_NOTE = ("Baseline: distances ~0 (model ignores spacing metadata). "
                        "Scale-aware: distances > 0 (model encodes physical scale).")


def counterfactual_summary(d_real_2x, d_real_half, d_half_2x) -> dict:
    """The reference's result dict of metric 3 from the three per-sample cosine-distance lists (float64 mean / std / median)."""
    blocks = {}
    for key, d in (("cosine_distance_real_vs_2x", d_real_2x), ("cosine_distance_real_vs_half", d_real_half),
                   ("cosine_distance_half_vs_2x", d_half_2x)):
        d = np.asarray(d, dtype=np.float64).reshape(-1)
        if d.shape[0] <= 0:
            raise ValueError("counterfactual_summary: no samples")
        blocks[key] = {"mean": float(np.mean(d)), "std": float(np.std(d)), "median": float(np.median(d))}
    n = {int(np.asarray(d).size) for d in (d_real_2x, d_real_half, d_half_2x)}
    if len(n) != 1:
        raise ValueError("counterfactual_summary: the three lists must have one length")
    return {"n": n.pop(), **blocks, "interpretation": _COUNTERFACTUAL_NOTE}


SPACING_VARIANTS = (1.0, 2.0, 0.5)      # real, 2x, half


def embed_spacing_variants(student, dataset, idxs: Sequence[int], img_size: int, batch_size: int = 64, *,
                           amp_dtype: Optional[torch.dtype] = None):
    """(e_real, e_2x, e_half): unit CLS rows, fp32 [N, D] on the device, of the deterministic view of ``dataset[i]``, i in ``idxs``
    (raw-stack items, as ``embed_eval_slices``), the SAME pixels embedded with spacing, 2 * spacing and 0.5 * spacing."""
    from .views import make_views
    bb = _backbone(student)
    anchor = next(bb.parameters())
    ops._need_cuda(anchor)
    n = len(idxs)
    if n <= 0:
        raise ValueError("embed_spacing_variants: no samples")
    E, at = None, 0
    was_training = bb.training
    bb.eval()
    try:
        with ops.compute_dtype(amp_dtype or torch.float32):
            for batch in _eval_batches(dataset, idxs, batch_size, anchor.device):
                x = make_views(batch, img_size)
                for v, mult in enumerate(SPACING_VARIANTS):
                    e = embed_cls(bb, x, batch.spacing * mult)
                    if E is None:
                        E = e.new_empty(len(SPACING_VARIANTS), n, e.shape[1])
                    E[v, at:at + len(e)] = e
                at += len(e)
    finally:
        bb.train(was_training)
    return E[0], E[1], E[2]


def counterfactual_distances(e_real: torch.Tensor, e_2x: torch.Tensor, e_half: torch.Tensor):
    """(real vs 2x, real vs half, half vs 2x) cosine distances 1 - a . b of unit rows, three fp32 [N] NumPy arrays, the products from
    ``ops.row_dots``.  Raises FloatingPointError when one is not finite."""
    out = []
    for a, b in ((e_real, e_2x), (e_real, e_half), (e_half, e_2x)):
        d = 1.0 - ops.row_dots(a, b)
        if not bool(torch.isfinite(d).all()):
            raise FloatingPointError("spacing_counterfactual: non-finite embeddings (diverged checkpoint?); no distance can be given")
        out.append(d.cpu().numpy())
    return tuple(out)


def spacing_counterfactual(student, dataset, img_size: int, n: int = 256, seed: int = 42, batch_size: int = 64, *,
                           amp_dtype: Optional[torch.dtype] = None) -> dict:
    """Metric 3 of the pan-organ evaluation: how far the embedding moves when only the spacing input changes.  Rows
    ``random.Random(seed).sample(range(len(dataset)), k=min(n, len(dataset)))``, their deterministic view, three backbone passes per
    batch (``embed_spacing_variants``), ``counterfactual_summary`` of the distances.  A backbone without the scale embedding ignores the
    spacing: the reference's ``{"skipped": True, ...}`` dict is returned and nothing runs."""
    if not getattr(_backbone(student), "scale_aware", False):
        return dict(COUNTERFACTUAL_SKIPPED)
    if n <= 0:
        raise ValueError("n must be > 0")
    idxs = random.Random(seed).sample(range(len(dataset)), k=min(int(n), len(dataset)))
    return counterfactual_summary(*counterfactual_distances(*embed_spacing_variants(student, dataset, idxs, img_size, batch_size,
                                                                                    amp_dtype=amp_dtype)))
