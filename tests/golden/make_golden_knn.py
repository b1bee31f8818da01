#!/usr/bin/env python3
"""Generate domain_clustering.npz FROM THE REAL REFERENCE (run where the reference checkout exists; it never travels to the GPU box):

    python tests/golden/make_golden_knn.py

It imports ``metric_domain_clustering`` from the reference's ``scripts/evaluate_panorgan.py`` (with empty ``torchvision`` / ``PIL`` stub
modules where those are not installed: the script only needs them for its image pipeline) and records

  rows              N = 1536 unit fp32 rows, D = 64: unit(centre[label] + A * noise), standard normal centres and noise,
                    4 clusters of 640 / 512 / 256 / 128 rows STORED CLASS BY CLASS (the unfriendly order for a threshold filter)
  labels            cluster of every row (index into label_names)
  label_names       the dataset names handed to the reference
  seed, noise_scale the draw
  reference_result  the reference's dict, as JSON text

A = 2.6 (about 0.84; 2.4 gives 0.88, 2.8 gives 0.80): at 1.6 the overall same-dataset rate is 0.98-0.99, too close to 1 for a wrong
neighbour set to move it; the generator requires
a rate in [0.75, 0.92], clearly between the random rate (0.319 for these sizes) and 1.

One right answer under any fp32 implementation: "10th and 11th neighbour further apart than the fp32 error" cannot be met over 1536 rows
(the smallest such gap is about 1e-6, against tau = 2 D 2^-24 = 7.6e-6).  What is required instead: for every row, all keys whose float64
score lies within tau of the row's 10th score carry the SAME label.  Then every admissible neighbour set has the same same-dataset
count, and NumPy's arbitrary choice inside argpartition cannot matter either.  The seed is redrawn until that holds.
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

N_PER, D, K, A = (640, 512, 256, 128), 64, 10, 2.6
NAMES = ("abdomen_ct", "chest_ct", "head_ct", "pelvis_ct")


def reference_metric():
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
    return E.metric_domain_clustering


def draw(seed: int):
    g = np.random.default_rng(seed)
    labels = np.repeat(np.arange(len(N_PER)), N_PER)
    centre = g.standard_normal((len(N_PER), D))
    x = centre[labels] + A * g.standard_normal((labels.size, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), labels


def one_right_answer(rows: np.ndarray, labels: np.ndarray) -> bool:
    tau = 2.0 * D * 2.0 ** -24
    S = rows.astype(np.float64) @ rows.astype(np.float64).T
    np.fill_diagonal(S, -np.inf)
    s_k = -np.sort(-S, axis=1)[:, K - 1]
    near = np.abs(S - s_k[:, None]) <= tau
    return all(len(set(labels[near[i]])) == 1 for i in range(rows.shape[0]))


class Row:
    def __init__(self, dataset):
        self.dataset = dataset


def main() -> None:
    metric = reference_metric()
    for seed in range(1000):
        rows, labels = draw(seed)
        if one_right_answer(rows, labels):
            break
    else:
        raise SystemExit("no seed gives a fixture with one right answer")
    result = metric(rows.copy(), [Row(NAMES[i]) for i in labels], k=K)
    rate = result["overall_same_dataset_rate"]
    print(f"seed {seed}: overall same-dataset rate {rate:.4f}, random {result['expected_random_rate']:.4f}")
    assert 0.75 <= rate <= 0.92, rate
    out = os.path.join(HERE, "domain_clustering.npz")
    np.savez_compressed(out, rows=rows, labels=labels.astype(np.int32), label_names=np.array(NAMES), seed=np.int64(seed),
                        noise_scale=np.float64(A), reference_result=np.array(json.dumps(result)))
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
