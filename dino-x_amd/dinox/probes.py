"""Linear probes and embedding statistics of the pan-organ evaluation on ``ops.softmax_probe`` (csrc/probe.hip) and ``ops.gram``
(csrc/gram.hip): the embedding matrix stays on the device, every pass over it is one kernel call, and what reaches the host is a
[C, D + 1] gradient, a [D + 1, D + 1] Gram matrix or the [n_test, C] probabilities.  The host side is float64 NumPy; there is no
scikit-learn or SciPy import.

``logistic_probe``   the reference's metric 2 (scripts/evaluate_panorgan.py:313-416, ``metric_dataset_discrimination_probe``): multinomial
                     logistic regression over the dataset labels with a series-level split and a series bootstrap.
``spacing_ridge``    metric 5 (:569-637, ``metric_spacing_prediction``): ridge regression of log(spacing_x).
``embedding_stats``  metric 6 (:644-697, ``metric_embedding_stats``): centroids, spread, first principal axis against spacing.

Same keys and definitions as the reference; what differs is said in each docstring.
"""
from __future__ import annotations

import random
from collections import defaultdict
from typing import Sequence

import numpy as np
import torch

from . import ops

_PROBE_NOTE = "dataset discrimination (not organ — confounded by scanner/protocol)"
_RIDGE_NOTE = "Partly circular for scale-aware models. Use as plumbing check."
LBFGS_HISTORY, LBFGS_MAX_EVALS, LBFGS_GTOL = 10, 2000, 1e-7


def _names(labels: Sequence) -> list:
    return ["unknown" if (d is None or d == "") else d for d in labels]


def _check(what: str, emb, *per_row) -> int:
    shape = tuple(getattr(emb, "shape", ()))
    if len(shape) != 2 or shape[0] < 1:
        raise ValueError(f"{what}: [N, D] embeddings expected, got shape {shape}")
    for name, v in per_row:
        if len(v) != shape[0]:
            raise ValueError(f"{what}: {shape[0]} embeddings but {len(v)} {name}")
    return shape[0]


def _spacing_x(spacings, n: int, what: str) -> np.ndarray:
    s = spacings.detach().cpu().numpy() if isinstance(spacings, torch.Tensor) else np.asarray(spacings)
    s = s.astype(np.float64)
    if s.ndim == 2:
        s = s[:, 0]
    if s.shape != (n,):
        raise ValueError(f"{what}: spacings must be [N] or [N, k] with N = {n}, got shape {tuple(np.shape(spacings))}")
    return s


# ------------------------------------------------------------------------------------------ series split
class SeriesSplit:
    """train_idx / test_idx: row numbers (ascending); train_series / test_series: sorted names; rows_of: series -> its row numbers in row
    order; dataset_of: series -> dataset."""

    def __init__(self, train_idx, test_idx, train_series, test_series, rows_of, dataset_of):
        self.train_idx, self.test_idx, self.train_series, self.test_series = train_idx, test_idx, train_series, test_series
        self.rows_of, self.dataset_of = rows_of, dataset_of


def series_split(labels: Sequence, series: Sequence, seed: int) -> SeriesSplit:
    """The reference's stratified 80/20 split at series level (its lines 329-356 and 587-612): the dataset of a series is the dataset of
    its LAST row; per dataset in sorted order the sorted series are shuffled by one ``random.Random(seed)`` and the first
    ``max(1, int(0.8 n))`` go to train, but at least one series stays for test when the dataset has two or more (a one-series dataset is
    all train).  The reference lists the rows of a split by iterating a Python set of series names, an order that changes with the
    interpreter's string-hash seed and on which none of its results depend; here the rows of a split are in ascending row order."""
    if len(labels) != len(series):
        raise ValueError(f"series_split: {len(labels)} labels but {len(series)} series")
    dataset_of, rows_of = {}, defaultdict(list)
    for i, (d, s) in enumerate(zip(_names(labels), series)):
        dataset_of[s] = d
        rows_of[s].append(i)
    by_dataset = defaultdict(list)
    for s, d in dataset_of.items():
        by_dataset[d].append(s)
    rng = random.Random(seed)
    train, test = [], []
    for d in sorted(by_dataset):
        names = sorted(by_dataset[d])
        rng.shuffle(names)
        n_train = max(1, int(0.8 * len(names)))
        if n_train == len(names):
            n_train = max(1, len(names) - 1)
        train += names[:n_train]
        test += names[n_train:]
    rows = lambda group: np.array(sorted(i for s in group for i in rows_of[s]), dtype=np.int64)
    return SeriesSplit(rows(train), rows(test), sorted(train), sorted(test), dict(rows_of), dataset_of)


def _take(E: torch.Tensor, idx: np.ndarray) -> torch.Tensor:
    return E.index_select(0, torch.from_numpy(idx).to(E.device))


# ------------------------------------------------------------------------------------------ L-BFGS
def lbfgs_minimize(fun, x0: np.ndarray, n_scale: float, *, history: int = LBFGS_HISTORY, max_evals: int = LBFGS_MAX_EVALS,
                   gtol: float = LBFGS_GTOL):
    """Minimise ``fun(x) -> (f, g)`` (float64) from x0 by L-BFGS: two-loop recursion over the last ``history`` pairs, a bracketing line
    search for the Armijo (1e-4) and weak Wolfe (0.9) conditions.  Stops when max |g| / n_scale <= gtol, after ``max_evals`` evaluations,
    or when a line search finds no lower value (``fun`` evaluates in fp32 on the device: below that resolution no step can be told from
    noise).  Returns (x, f, g, evaluations, reason)."""
    x = np.array(x0, dtype=np.float64)
    f, g = fun(x)
    evals, S, Y = 1, [], []
    reason = "max_evals"
    while evals < max_evals:
        if np.max(np.abs(g)) / n_scale <= gtol:
            reason = "gtol"
            break
        q = g.copy()
        alphas = []
        for s, y in zip(reversed(S), reversed(Y)):
            a = (s @ q) / (y @ s)
            alphas.append(a)
            q -= a * y
        if S:
            q *= (S[-1] @ Y[-1]) / (Y[-1] @ Y[-1])
        for (s, y), a in zip(zip(S, Y), reversed(alphas)):
            q += (a - (y @ q) / (y @ s)) * s
        d = -q
        gd = g @ d
        if not gd < 0:                                        # not a descent direction (noise in the pairs): steepest descent
            S, Y, d = [], [], -g
            gd = g @ d
        t = 1.0 if S else min(1.0, 1.0 / max(np.sqrt(g @ g), 1e-300))
        lo, hi, best = 0.0, np.inf, None
        for _ in range(30):
            if evals >= max_evals:
                break
            ft, gt = fun(x + t * d)
            evals += 1
            if np.isfinite(ft) and ft < f and (best is None or ft < best[1]):
                best = (t, ft, gt)
            if not np.isfinite(ft) or ft > f + 1e-4 * t * gd:
                hi = t
            elif gt @ d < 0.9 * gd:
                lo = t
            else:
                break
            t = 2.0 * t if np.isinf(hi) else 0.5 * (lo + hi)
        if best is None:
            reason = "resolution" if evals < max_evals else "max_evals"
            break
        t, ft, gt = best
        s, y = t * d, gt - g
        x, f, g = x + s, ft, gt
        if s @ y > 1e-10 * (y @ y) ** 0.5 * (s @ s) ** 0.5:
            S.append(s)
            Y.append(y)
            if len(S) > history:
                S.pop(0)
                Y.pop(0)
    else:
        if np.max(np.abs(g)) / n_scale <= gtol:
            reason = "gtol"
    return x, f, g, evals, reason


def fit_softmax(X: torch.Tensor, y: torch.Tensor, n_classes: int, *, l2: float = 1.0):
    """theta float64 [C, D + 1] minimising sum_i CE_i + 0.5 l2 ||W||^2 (the intercept column is not penalised): scikit-learn's
    LogisticRegression objective at C = 1 / l2.  Every evaluation is one ``ops.softmax_probe`` call on X at the fp32 rounding of theta,
    and the penalty is taken at the same rounded point, so value and gradient belong to one function.  Returns (theta, info)."""
    n, D = X.shape

    def fun(v):
        th32 = v.reshape(n_classes, D + 1).astype(np.float32)
        loss, grad, _ = ops.softmax_probe(X, y, torch.from_numpy(th32).to(X.device), want_grad=True)
        th = th32.astype(np.float64)
        g = grad.cpu().numpy().astype(np.float64)
        g[:, :D] += l2 * th[:, :D]
        return (float(loss) + 0.5 * l2 * float(np.sum(th[:, :D] ** 2))) / n, g.reshape(-1) / n

    v, f, g, evals, reason = lbfgs_minimize(fun, np.zeros(n_classes * (D + 1)), 1.0)
    info = {"evaluations": evals, "stopped_by": reason, "objective": f * n, "max_abs_grad_per_row": float(np.max(np.abs(g)))}
    return v.reshape(n_classes, D + 1), info


# ------------------------------------------------------------------------------------------ host metrics
def rank_auc(score: np.ndarray, positive: np.ndarray) -> float:
    """P(score of a positive > score of a negative) + P(equal) / 2 from average ranks (the area under the ROC curve)."""
    positive = np.asarray(positive, dtype=bool)
    n_pos, n_neg = int(positive.sum()), int((~positive).sum())
    if n_pos == 0 or n_neg == 0:
        return float("nan")
    vals, inv, counts = np.unique(score, return_inverse=True, return_counts=True)
    ends = np.cumsum(counts).astype(np.float64)
    avg_rank = ends - (counts - 1) / 2.0                      # 1-based average rank of each distinct value
    ranks = avg_rank[inv.reshape(-1)]
    return float((ranks[positive].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * float(n_neg)))


def probe_auc(prob: np.ndarray, y: np.ndarray) -> float:
    """Binary AUC of column 1 for two classes, else the macro average of the one-vs-rest AUCs (over the classes that have both
    positives and negatives among the rows)."""
    C = prob.shape[1]
    if C == 2:
        return rank_auc(prob[:, 1], y == 1)
    aucs = [rank_auc(prob[:, c], y == c) for c in range(C)]
    aucs = [a for a in aucs if a == a]
    return float(np.mean(aucs)) if aucs else float("nan")


def logistic_probe(E: torch.Tensor, labels: Sequence, series: Sequence, seed: int = 42, *, return_details: bool = False) -> dict:
    """Metric 2: ``E`` device fp32 [N, D]; ``labels`` the dataset and ``series`` the series of every row.  Keys as the reference:
    ``labels``, ``train_series``, ``test_series``, ``train_slices``, ``test_slices``, ``accuracy``, ``accuracy_ci95`` (2.5 / 97.5
    percentiles of 200 series-level bootstrap draws by ``random.Random(seed + 1)``), ``auc``, ``note``; or its ``{"error": ...}`` dicts.
    The fit is ``fit_softmax`` (L-BFGS to max |grad| / n <= 1e-7 where the reference stops scikit-learn's at its default tolerance);
    ``return_details`` adds ``fit`` (evaluations, stop reason) and ``probabilities`` ([n_test, C] float64 array, test rows ascending)."""
    _check("logistic_probe", E, ("labels", labels), ("series", series))
    sp = series_split(labels, series, seed)
    if len(sp.train_idx) == 0 or len(sp.test_idx) == 0:
        return {"error": "insufficient series for train/test split"}
    all_labels = sorted(set(sp.dataset_of.values()))
    cid = {name: i for i, name in enumerate(all_labels)}
    row_class = np.empty(len(labels), dtype=np.int64)
    for s, rows in sp.rows_of.items():
        row_class[rows] = cid[sp.dataset_of[s]]
    y_train, y_test = row_class[sp.train_idx], row_class[sp.test_idx]
    if len(set(y_train.tolist())) < 2 or len(set(y_test.tolist())) < 2:
        return {"error": "need at least 2 datasets in both train and test splits"}
    if len(all_labels) > ops.PROBE_MAX_C:
        raise ValueError(f"logistic_probe: {len(all_labels)} datasets, the probe kernel takes at most {ops.PROBE_MAX_C}")

    dev = E.device
    theta, info = fit_softmax(_take(E, sp.train_idx), torch.from_numpy(y_train).to(dev), len(all_labels))
    _, _, prob = ops.softmax_probe(_take(E, sp.test_idx), torch.from_numpy(y_test).to(dev), torch.from_numpy(theta.astype(np.float32)).to(dev),
                                   want_grad=False, want_prob=True)
    prob = prob.cpu().numpy().astype(np.float64)
    if not np.isfinite(prob).all():
        raise FloatingPointError("logistic_probe: non-finite probabilities (non-finite embeddings?)")
    right = np.zeros(len(labels), dtype=bool)
    right[sp.test_idx] = np.argmax(prob, axis=1) == y_test
    acc = float(np.mean(right[sp.test_idx]))
    auc = probe_auc(prob, y_test)

    boot, rng = [], random.Random(seed + 1)
    for _ in range(200):
        draw = [sp.test_series[rng.randint(0, len(sp.test_series) - 1)] for _ in range(len(sp.test_series))]
        rows = [i for s in draw for i in sp.rows_of[s]]
        if rows:
            boot.append(float(np.mean(right[rows])))
    lo = float(np.percentile(boot, 2.5)) if boot else acc
    hi = float(np.percentile(boot, 97.5)) if boot else acc
    out = {"labels": all_labels, "train_series": len(sp.train_series), "test_series": len(sp.test_series),
           "train_slices": int(len(sp.train_idx)), "test_slices": int(len(sp.test_idx)), "accuracy": acc, "accuracy_ci95": [lo, hi],
           "auc": auc, "note": _PROBE_NOTE}
    if return_details:
        out["fit"], out["probabilities"] = info, prob
    return out


# ------------------------------------------------------------------------------------------ second moments
def _centred_moments(A: torch.Tensor):
    """(n, mean float64 [k], centred Gram float64 [k, k]) of the columns of the device fp32 rows A [n, k] from two ``ops.gram`` passes: the
    first gives the means, the second runs on the rows shifted by the fp32 rounding m of the means, which takes the cancellation out of
    the fp32 products; the remainder delta = colsum / n of that pass is removed exactly: sum (z - delta)(z - delta)^T = G - n delta delta^T."""
    n = A.shape[0]
    _, colsum = ops.gram(A)
    m32 = (colsum.cpu().numpy() / n).astype(np.float32)
    G, rest = ops.gram(A, torch.from_numpy(m32).to(A.device))
    G, delta = G.cpu().numpy(), rest.cpu().numpy() / n
    return n, m32.astype(np.float64) + delta, G - n * np.outer(delta, delta)


def _with_column(E: torch.Tensor, col: np.ndarray) -> torch.Tensor:
    return torch.cat([E, torch.from_numpy(col.astype(np.float32)).to(E.device)[:, None]], dim=1)


def spacing_ridge(E: torch.Tensor, spacings, labels: Sequence, series: Sequence, seed: int = 42) -> dict:
    """Metric 5: ridge regression (penalty 1, unpenalised intercept) from the embeddings to y = log(spacing_x + 1e-6) on the train rows
    of ``series_split``, scored on its test rows.  The normal equations (Xc^T Xc + I) w = Xc^T yc come from the centred Gram of
    [E_train | y] (two ``ops.gram`` passes) and are solved by Cholesky in float64; the test rows are predicted by a float64 host
    product.  Keys as the reference: ``target``, ``train_slices``, ``test_slices``, ``r2``, ``mae_log_spacing``, ``note``."""
    n = _check("spacing_ridge", E, ("labels", labels), ("series", series))
    if E.shape[1] + 1 > ops.GRAM_MAX_D:
        raise ValueError(f"spacing_ridge: D = {E.shape[1]}, the Gram kernel takes D + 1 <= {ops.GRAM_MAX_D} columns")
    y = np.log(_spacing_x(spacings, n, "spacing_ridge") + 1e-6)
    sp = series_split(labels, series, seed)
    if len(sp.train_idx) == 0 or len(sp.test_idx) == 0:
        return {"error": "insufficient series for split"}
    D = E.shape[1]
    _, mean, G = _centred_moments(_with_column(_take(E, sp.train_idx), y[sp.train_idx]))
    L = np.linalg.cholesky(G[:D, :D] + np.eye(D))
    w = np.linalg.solve(L.T, np.linalg.solve(L, G[:D, D]))
    b = mean[D] - mean[:D] @ w
    y_test = y[sp.test_idx]
    y_pred = _take(E, sp.test_idx).cpu().numpy().astype(np.float64) @ w + b
    ss_res, ss_tot = float(np.sum((y_test - y_pred) ** 2)), float(np.sum((y_test - y_test.mean()) ** 2))
    r2 = 1.0 - ss_res / ss_tot if ss_tot > 0 else (1.0 if ss_res == 0 else 0.0)      # (scikit-learn's r2_score convention for a constant target)
    return {"target": "log(spacing_x)", "train_slices": int(len(sp.train_idx)), "test_slices": int(len(sp.test_idx)), "r2": float(r2),
            "mae_log_spacing": float(np.mean(np.abs(y_test - y_pred))), "note": _RIDGE_NOTE}


def embedding_stats(E: torch.Tensor, spacings, labels: Sequence) -> dict:
    """Metric 6, per dataset (sorted names; the rows are sorted by dataset once, as a device gather, and every dataset is a block of rows
    of [E | spacing_x] handed to ``ops.gram`` twice): ``n``, ``embedding_std`` (mean over the columns of the population standard
    deviation), ``intra_cosine_to_centroid`` (mean cosine of the rows to the unit centroid = centroid . mean), and
    ``pca1_spacing_correlation`` = v^T c_xs / sqrt(lambda_1 var_s) with (lambda_1, v) the top eigenpair (``np.linalg.eigh``) of the
    centred Gram of the embeddings, c_xs their cross moments with spacing_x; NaN unless n > 2.  The sign of a principal axis is arbitrary
    -- in the reference it is whatever LAPACK's SVD returns -- so it is fixed here: the eigenvector's largest-magnitude component is
    positive.  ``cross_dataset_centroid_cosine``: the cosines of the unit centroids, keys ``<a>_vs_<b>`` for a < b."""
    n = _check("embedding_stats", E, ("labels", labels))
    if E.shape[1] + 1 > ops.GRAM_MAX_D:
        raise ValueError(f"embedding_stats: D = {E.shape[1]}, the Gram kernel takes D + 1 <= {ops.GRAM_MAX_D} columns")
    s = _spacing_x(spacings, n, "embedding_stats")
    names, row_class = np.unique(np.array(_names(labels), dtype=object), return_inverse=True)
    row_class = row_class.reshape(-1)
    order = np.argsort(row_class, kind="stable")
    A = _with_column(_take(E, order), s[order])
    D = E.shape[1]
    sizes = np.bincount(row_class, minlength=len(names))
    per, centroids, at = {}, {}, 0
    with np.errstate(invalid="ignore", divide="ignore"):
        for name, size in zip(names, sizes):
            m, mean, G = _centred_moments(A[at:at + size])
            at += size
            centroid = mean[:D] / (np.linalg.norm(mean[:D]) + 1e-8)
            centroids[str(name)] = centroid
            corr = float("nan")
            if m > 2:
                lam, V = np.linalg.eigh(G[:D, :D])
                v = V[:, -1]
                v = v if v[np.argmax(np.abs(v))] > 0 else -v
                corr = float((v @ G[:D, D]) / np.sqrt(lam[-1] * G[D, D]))
            per[str(name)] = {"n": int(m), "embedding_std": float(np.mean(np.sqrt(np.maximum(np.diag(G)[:D], 0.0) / m))),
                              "intra_cosine_to_centroid": float(centroid @ mean[:D]), "pca1_spacing_correlation": corr}
    keys = sorted(centroids)
    cross = {f"{a}_vs_{b}": float(centroids[a] @ centroids[b]) for i, a in enumerate(keys) for b in keys[i + 1:]}
    return {"per_dataset": per, "cross_dataset_centroid_cosine": cross}
