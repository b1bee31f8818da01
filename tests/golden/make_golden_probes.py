#!/usr/bin/env python3
"""Generate panorgan_probes.npz FROM THE REAL REFERENCE (run where the reference checkout and scikit-learn exist; neither travels to the
GPU box):

    python tests/golden/make_golden_probes.py

It imports ``metric_dataset_discrimination_probe``, ``metric_spacing_prediction`` and ``metric_embedding_stats`` from the reference's
``scripts/evaluate_panorgan.py`` (with empty ``torchvision`` / ``PIL`` stub modules where those are not installed, as
make_golden_knn.py does) and records

  rows, labels, label_names, series, spacings   the draw: 3 datasets of 20 / 14 / 8 series x 24 slices (N = 1008), D = 64, unit fp32
                    rows of 0.8 g0 + centre[label] + 2.5 noise + 2 log(spacing_x) u (g0, centres, u, noise standard normal; u a unit
                    vector), one log-uniform spacing_x in [0.45, 1.0] per series, spacings = (x, x, 2.5)
  reference_probe, reference_ridge, reference_stats   the reference's three result dicts, as JSON text
  train_idx, test_idx   the rows the reference handed to its classifier (captured at the fit / predict_proba calls), ascending
  prob_tight, auc_tight   the same scikit-learn class refitted on the float64 train rows with tol = 1e-10, max_iter = 100 000 -- the
                    reference library at its optimum -- and its probabilities on the test rows (test_idx order), its AUC
  prob_default_distance   max |default fit - tight fit| over the test probabilities
  auc_slack         share of one-vs-rest (positive, negative) pairs whose prob_tight values differ by less than 2e-3, mean over classes:
                    how far an AUC can move when every probability moves by up to 1e-3

The seed is redrawn until: accuracy in [0.85, 0.98] (a wrong fit must be able to move it), default and tight fit predict the same
classes, and the two largest prob_tight of every test row are at least 0.02 apart (so a fit within 1e-3 of the optimum predicts the
same classes and accuracy and its bootstrap interval are exact).
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import types

import numpy as np

REF = os.environ.get("DINOX_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))

SERIES_PER, SLICES, D = (20, 14, 8), 24, 64
NAMES = ("abdomen_ct", "chest_ct", "head_ct")
SEED_FIT = 42


def reference_module():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "scripts"))
    for name in ("torchvision", "torchvision.transforms", "PIL", "PIL.Image"):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["PIL"], "Image"):
        sys.modules["PIL"].Image = sys.modules["PIL.Image"]
    import evaluate_panorgan as E                    # (the reference)
    return E


class Row:
    def __init__(self, dataset, series_dir):
        self.dataset, self.series_dir = dataset, series_dir


def draw(seed: int):
    g = np.random.default_rng(seed)
    g0, centre, u = g.standard_normal(D), g.standard_normal((len(NAMES), D)), g.standard_normal(D)
    u /= np.linalg.norm(u)
    labels, series, sx = [], [], []
    for d, n_series in enumerate(SERIES_PER):
        for k in range(n_series):
            s = float(np.exp(g.uniform(np.log(0.45), np.log(1.0))))
            labels += [d] * SLICES
            series += [f"{NAMES[d]}/series_{k:03d}"] * SLICES
            sx += [s] * SLICES
    labels, sx = np.array(labels), np.array(sx)
    x = 0.8 * g0 + centre[labels] + 2.5 * g.standard_normal((labels.size, D)) + 2.0 * np.log(sx)[:, None] * u
    rows = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    spacings = np.stack([sx, sx, np.full_like(sx, 2.5)], 1).astype(np.float32)
    return rows, labels, series, spacings


def main() -> None:
    E = reference_module()
    import sklearn.linear_model as lm
    from sklearn.metrics import roc_auc_score
    seen = {}

    class Recording(lm.LogisticRegression):
        def fit(self, X, y, *a, **k):
            seen["train"], seen["clf"] = np.array(X), self
            return super().fit(X, y, *a, **k)

        def predict_proba(self, X):
            seen["test"] = np.array(X)
            return super().predict_proba(X)

    for seed in range(64):
        rows, labels, series, spacings = draw(seed)
        objs = [Row(NAMES[d], s) for d, s in zip(labels, series)]
        real = lm.LogisticRegression
        lm.LogisticRegression = Recording
        try:
            probe = E.metric_dataset_discrimination_probe(rows.copy(), objs, seed=SEED_FIT)
        finally:
            lm.LogisticRegression = real
        key = {r.tobytes(): i for i, r in enumerate(rows)}
        assert len(key) == len(rows)
        train_idx = np.sort([key[r.tobytes()] for r in seen["train"]])
        in_order = np.array([key[r.tobytes()] for r in seen["test"]])
        test_idx = np.sort(in_order)
        prob_default = np.empty((len(test_idx), len(NAMES)))
        prob_default[np.searchsorted(test_idx, in_order)] = seen["clf"].predict_proba(seen["test"])
        tight = real(max_iter=100000, tol=1e-10, random_state=SEED_FIT, solver="lbfgs").fit(rows[train_idx].astype(np.float64), labels[train_idx])
        prob_tight = tight.predict_proba(rows[test_idx].astype(np.float64))
        top2 = -np.sort(-prob_tight, axis=1)[:, :2]
        ok = (0.85 <= probe["accuracy"] <= 0.98 and np.array_equal(prob_default.argmax(1), prob_tight.argmax(1))
              and float((top2[:, 0] - top2[:, 1]).min()) >= 0.02)
        print(f"seed {seed}: accuracy {probe['accuracy']:.4f}, smallest top-2 gap {float((top2[:, 0] - top2[:, 1]).min()):.4f}, "
              f"default vs tight {np.abs(prob_default - prob_tight).max():.2e} -> {'ok' if ok else 'redraw'}")
        if ok:
            break
    else:
        raise SystemExit("no seed qualifies")
    y_test = labels[test_idx]
    auc_tight = float(roc_auc_score(y_test, prob_tight, multi_class="ovr", average="macro"))
    slack = []
    for c in range(len(NAMES)):
        pos, neg = prob_tight[y_test == c, c], prob_tight[y_test != c, c]
        slack.append(float((np.abs(pos[:, None] - neg[None, :]) < 2e-3).mean()))
    ridge = E.metric_spacing_prediction(rows.copy(), spacings.copy(), objs, seed=SEED_FIT)
    stats = E.metric_embedding_stats(rows.copy(), spacings.copy(), objs)
    print(f"auc {probe['auc']:.6f} (tight {auc_tight:.6f}), auc_slack {np.mean(slack):.2e}, r2 {ridge['r2']:.6f}, "
          f"train/test {len(train_idx)}/{len(test_idx)}")
    out = os.path.join(HERE, "panorgan_probes.npz")
    np.savez_compressed(out, rows=rows, labels=labels.astype(np.int32), label_names=np.array(NAMES), series=np.array(series), spacings=spacings,
                        seed=np.int64(seed), fit_seed=np.int64(SEED_FIT), reference_probe=np.array(json.dumps(probe)),
                        reference_ridge=np.array(json.dumps(ridge)), reference_stats=np.array(json.dumps(stats)),
                        train_idx=train_idx.astype(np.int64), test_idx=test_idx.astype(np.int64), prob_tight=prob_tight,
                        auc_tight=np.float64(auc_tight), prob_default_distance=np.float64(np.abs(prob_default - prob_tight).max()),
                        auc_slack=np.float64(np.mean(slack)))
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
