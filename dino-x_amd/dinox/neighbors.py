"""Nearest-neighbour evaluation of embeddings on ``ops.knn_topk`` (csrc/knn.hip): the embeddings stay on the device, the K nearest keys
of every row come out of the exact-fp32 MFMA sweep, and only the [N, k] indices (and scores) reach the host.  No N x N array exists.

``domain_clustering``  the reference's pan-organ metric 4 (scripts/evaluate_panorgan.py:507-562, ``metric_domain_clustering``): how often
                       the k = 10 neighbours of a slice come from the slice's own dataset, with per-dataset enrichment over prevalence.
                       Same output keys and definitions, restated on per-row counts; the reference's N x N host block is the kernel call.
``knn_probe``          the weighted k-NN classifier of the DINO paper (Caron et al. 2021, section 4.1 / appendix: k = 20, each neighbour
                       votes for its class with weight exp(similarity / 0.07)).  The reference has no counterpart; it is specified against
                       the paper, as multi-crop is.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from . import ops

_NOTE = "High enrichment = strong domain clustering. Not necessarily good or bad."


def _names(labels: Sequence) -> list:
    return ["unknown" if (d is None or d == "") else d for d in labels]


def _check_rows(what: str, emb, n_labels: Optional[int]) -> int:
    shape = tuple(getattr(emb, "shape", ()))
    if len(shape) != 2 or shape[0] < 1:
        raise ValueError(f"{what}: [N, D] embeddings expected, got shape {shape}")
    if n_labels is not None and n_labels != shape[0]:
        raise ValueError(f"{what}: {shape[0]} embeddings but {n_labels} labels")
    return shape[0]


def domain_clustering(embeddings, labels: Sequence, k: int = 10) -> dict:
    """``embeddings``: device fp32 [N, D] (unit rows); ``labels``: the dataset name of every row (None -> "unknown").  Returns a dict
    with the reference's keys: ``k``, ``overall_same_dataset_rate`` (mean over the rows of the share of a row's k neighbours that carry
    the row's own label), ``expected_random_rate`` (sum of squared prevalences), ``enrichment_vs_random`` (their ratio),
    ``per_dataset`` {name: ``same_dataset_rate`` (the same mean over the rows of that dataset), ``expected_random`` (its prevalence),
    ``enrichment``, ``n``}, ``note``.  A row's neighbours are the first k of the OTHER rows by (score descending, index ascending);
    the reference's argpartition picks arbitrarily among equal scores at the k-th place."""
    n = _check_rows("domain_clustering", embeddings, len(labels))
    if not 1 <= k < n:
        raise ValueError(f"domain_clustering: k = {k} needs 1 <= k < N = {n}")
    names, row_class = np.unique(np.array(_names(labels), dtype=object), return_inverse=True)      # sorted distinct names, id per row
    row_class = row_class.reshape(-1)
    size = np.bincount(row_class, minlength=len(names))
    share = size / float(n)

    nbr = ops.knn_topk(embeddings, embeddings, k, exclude="self")[0].cpu().numpy()
    if (nbr < 0).any():
        raise FloatingPointError("domain_clustering: rows without k neighbours (non-finite embeddings?)")
    hits = (row_class[nbr] == row_class[:, None]).sum(axis=1)                  # exact counts, 0..k per row
    rate_of_row = hits / float(k)

    def ratio(rate: float, chance: float) -> float:
        return rate / chance if chance > 0 else float("inf")

    table = {}
    for c, name in enumerate(names):
        rate, chance = float(rate_of_row[row_class == c].mean()), float(share[c])
        table[str(name)] = {"same_dataset_rate": rate, "expected_random": chance, "enrichment": ratio(rate, chance), "n": int(size[c])}
    overall, chance = float(rate_of_row.mean()), float(np.sum(share * share))
    return {"k": k, "overall_same_dataset_rate": overall, "expected_random_rate": chance, "enrichment_vs_random": ratio(overall, chance),
            "per_dataset": table, "note": _NOTE}


def knn_probe(train_emb, train_labels: Sequence, test_emb=None, k: int = 20, temperature: float = 0.07, *,
              test_labels: Optional[Sequence] = None, return_predictions: bool = False) -> dict:
    """Weighted k-NN vote: the score of class c for a test row is the sum of exp(s / temperature) over those of its k nearest train rows
    that carry class c (s = the neighbour's similarity, accumulated in float64 on the host in neighbour order); the prediction is the
    class with the highest score, the lowest class id (position in ``classes`` = sorted distinct train labels) on equal scores.
    ``test_emb=None``: leave-one-out on the train set (row i is left out of its own neighbours) and ``test_labels`` is not read;
    otherwise ``test_labels`` gives the truth of the test rows.  Fewer than k eligible train rows: the missing neighbours do not vote.
    Returns ``accuracy``, ``per_class_accuracy`` {class: accuracy over the test rows of that class}, ``k``, ``temperature``,
    ``n_train``, ``n_test``, ``classes`` (and ``predictions``, the predicted label per test row, with ``return_predictions``)."""
    train_names = _names(train_labels)
    n_train = _check_rows("knn_probe", train_emb, len(train_names))
    if not temperature > 0:
        raise ValueError(f"knn_probe: temperature must be > 0, got {temperature}")
    if test_emb is None:
        query, truth_names, exclude = train_emb, train_names, "self"
    else:
        if test_labels is None:
            raise ValueError("knn_probe: test_emb needs test_labels")
        truth_names, query, exclude = _names(test_labels), test_emb, None
    n_test = _check_rows("knn_probe", query, len(truth_names))
    classes = sorted(set(train_names))
    cid = {c: i for i, c in enumerate(classes)}
    train_id = np.array([cid[c] for c in train_names])

    idx, val = ops.knn_topk(query, train_emb, k, exclude=exclude)
    idx, val = idx.cpu().numpy().astype(np.int64), val.cpu().numpy().astype(np.float64)
    if np.isnan(val).any():
        raise FloatingPointError("knn_probe: non-finite similarities")
    there = idx >= 0
    weight = np.where(there, np.exp(np.where(there, val, 0.0) / float(temperature)), 0.0)
    votes = np.zeros((n_test, len(classes)), dtype=np.float64)
    rows = np.arange(n_test)
    for p in range(idx.shape[1]):                         # neighbour order: a fixed summation order
        votes[rows, train_id[np.where(there[:, p], idx[:, p], 0)]] += weight[:, p]
    pred = np.argmax(votes, axis=1)                       # first maximum = lowest class id
    pred_names = [classes[i] for i in pred]
    hit = np.array([p == t for p, t in zip(pred_names, truth_names)])
    per_class = {c: float(np.mean(hit[[i for i, t in enumerate(truth_names) if t == c]])) for c in sorted(set(truth_names))}
    out = {"accuracy": float(np.mean(hit)), "per_class_accuracy": per_class, "k": int(k), "temperature": float(temperature),
           "n_train": int(n_train), "n_test": int(n_test), "classes": classes}
    if return_predictions:
        out["predictions"] = pred_names
    return out
