#!/usr/bin/env python3
"""Generate panorgan_views.npz FROM THE REAL REFERENCE (run where the reference checkout exists; it does not travel to the GPU box):

    python tests/golden/make_golden_views.py

It imports the reference's ``scripts/evaluate_panorgan.py`` (with empty ``torchvision`` / ``PIL`` stub modules where those are not
installed, as make_golden_probes.py does), replaces its ``PngDataset`` / ``EvalDataset`` with in-memory datasets that return fixed
tensors per row, and calls ``metric_view_retrieval_per_dataset`` and ``metric_spacing_counterfactual`` on a tiny fixed ``student`` whose
``backbone(x, spacing)`` is the reference's own ``PatchViT`` (28 px, patch 14, width 64, depth 2, scale-aware) with seeded weights on the
CPU; the zero-initialised output layer of its scale embedding is redrawn (normal, std 0.2) so that the spacing reaches the embedding,
and the weight matrices of its blocks are scaled by 3 so that the embeddings spread (scores of a row then cover about [-0.2, 1]).
Recorded:

  datasets, series  per row (N = 300: 150 / 40 / 110 rows of three datasets, interleaved; one dataset below n_per_dataset = 96)
  names             the datasets in the reference's (sorted) order
  picks_<g>         per dataset, the positions the reference drew (into that dataset's rows in index order), in pick order -- captured at
                    the dataset's __getitem__
  Q_<g>, K_<g>      per dataset, the unit CLS rows the reference computed for view 1 / view 2 of the picks (captured at its
                    embed_backbone_cls), fp32 [n_g, 64]
  d_real_2x, d_real_half, d_half_2x   the three per-sample distance lists of the counterfactual (captured at the reference's np.mean
                    calls), float64 [64]
  reference_retrieval, reference_counterfactual   the two result dicts, as JSON text
  n_per_dataset, n_counterfactual, seed, topk, draw_seed

The draw seed (images, view noise, weights) is redrawn until, in float64, no query's positive score is within 2 D 2^-23 of another
key's score of its dataset -- every rank then has exactly one admissible value under any fp32 summation order, so top1 / top5 are exact --
and top-1 is neither 0 nor 1 in the two larger datasets.
"""
from __future__ import annotations

import importlib
import json
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("DINOX_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))

NAMES = ("abdomen_ct", "chest_ct", "head_ct")
SIZES = (150, 40, 110)
IMG, PATCH, D, DEPTH, HEADS = 28, 14, 64, 2, 2
N_PER_DATASET, N_COUNTERFACTUAL, SEED, TOPK = 96, 64, 42, 5
LATENT, VIEW_NOISE, BLOCK_GAIN = 12, 0.5, 3.0


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
    if not hasattr(sys.modules["torchvision"], "transforms"):
        sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    import evaluate_panorgan as E                    # (the reference)
    return E


class Row:
    def __init__(self, dataset, series_dir, spacing, views, image):
        self.dataset, self.series_dir = dataset, series_dir
        self.spacing_x, self.spacing_y, self.spacing_z = (float(v) for v in spacing)
        self.views, self.image = views, image


def draw(seed: int):
    """Images with a low-dimensional cause: image = 4 sum_k z_k P_k / sqrt(12) over 12 fixed random patterns P_k, z standard normal per
    row; a view is the image of z + 0.5 noise.  (Pure noise images leave the CLS rows of a random ViT nearly collinear: every score within
    0.02 of the others, and no draw meets the gap condition.)"""
    g = torch.Generator().manual_seed(seed)
    order = np.random.default_rng(seed).permutation(np.repeat(np.arange(len(NAMES)), SIZES))      # interleaved datasets
    P = torch.randn(LATENT, 3, IMG, IMG, generator=g)
    image = lambda z: 4.0 * torch.einsum("k,kchw->chw", z, P) / LATENT ** 0.5
    rows = []
    for i, d in enumerate(order):
        z = torch.randn(LATENT, generator=g)
        views = [image(z + VIEW_NOISE * torch.randn(LATENT, generator=g)) for _ in range(2)]
        sx = float(torch.rand(1, generator=g)) * 1.2 + 0.4
        rows.append(Row(NAMES[d], f"{NAMES[d]}/series_{i // 8:03d}", (sx, sx, 2.5), views, image(z)))
    return rows


class Student:
    def __init__(self, E, seed: int):
        torch.manual_seed(seed)
        self.backbone = E.PatchViT(img_size=IMG, patch=PATCH, dim=D, depth=DEPTH, heads=HEADS, scale_aware=True).eval()
        with torch.no_grad():
            torch.nn.init.normal_(self.backbone.scale_embed.mlp[2].weight, std=0.2)
            for name, p in self.backbone.named_parameters():
                if name.startswith("blocks.") and p.dim() == 2:
                    p.mul_(BLOCK_GAIN)


def main() -> None:
    E = reference_module()
    log = {"picks": [], "embeds": [], "means": []}

    class FixedViews:                                  # stands in for the reference's PngDataset
        def __init__(self, rows, **kw):
            self.rows = rows
            log["picks"].append([])

        def __getitem__(self, i):
            log["picks"][-1].append(int(i))
            r = self.rows[i]
            return r.views, torch.tensor([r.spacing_x, r.spacing_y, r.spacing_z])

    class FixedImages:                                 # stands in for the reference's EvalDataset
        def __init__(self, rows, img_size=IMG):
            self.rows = rows

        def __getitem__(self, i):
            r = self.rows[i]
            return r.image, torch.tensor([r.spacing_x, r.spacing_y, r.spacing_z], dtype=torch.float32)

    class RecordingNumpy:                              # the reference's ``np``: records what it averages
        def __getattr__(self, name):
            return getattr(np, name)

        def mean(self, x, *a, **k):
            log["means"].append(np.array(x, dtype=np.float64))
            return np.mean(x, *a, **k)

    real_embed = E.embed_backbone_cls

    def recording_embed(student, x, spacing=None):
        e = real_embed(student, x, spacing=spacing)
        log["embeds"].append(e.cpu().numpy().copy())
        return e

    E.PngDataset, E.EvalDataset, E.embed_backbone_cls = FixedViews, FixedImages, recording_embed
    dev = torch.device("cpu")
    tau = 2.0 * D * 2.0 ** -23
    for seed in range(256):
        for v in log.values():
            v.clear()
        rows, student = draw(seed), Student(E, seed)
        res = E.metric_view_retrieval_per_dataset(student, rows, IMG, {}, dev, scale_aware=True, n_per_dataset=N_PER_DATASET, seed=SEED,
                                                  topk=TOPK)
        names = list(res)
        assert names == sorted(NAMES) and len(log["picks"]) == len(names)
        Q, K, at, gap = [], [], 0, np.inf
        for g, name in enumerate(names):
            calls = 2 * -(-res[name]["n"] // 64)
            chunk = log["embeds"][at:at + calls]
            at += calls
            Q.append(np.concatenate(chunk[0::2]))
            K.append(np.concatenate(chunk[1::2]))
            assert Q[g].shape == (res[name]["n"], D) and len(log["picks"][g]) == res[name]["n"]
            S = Q[g].astype(np.float64) @ K[g].astype(np.float64).T
            off = np.abs(S - np.diagonal(S)[:, None])
            np.fill_diagonal(off, np.inf)
            gap = min(gap, float(off.min()))
        assert at == len(log["embeds"])
        top1 = [res[n]["top1"] for n in names]
        ok = gap > tau and all(0.0 < t < 1.0 for t, n in zip(top1, names) if res[n]["n"] >= 64)
        print(f"seed {seed}: n {[res[n]['n'] for n in names]}, top1 {top1}, smallest score gap {gap:.3e} (need > {tau:.3e}) -> "
              f"{'ok' if ok else 'redraw'}")
        if ok:
            break
    else:
        raise SystemExit("no seed qualifies")

    real_np, E.np = E.np, RecordingNumpy()
    try:
        cf = E.metric_spacing_counterfactual(student, rows, IMG, dev, n=N_COUNTERFACTUAL, seed=SEED)
    finally:
        E.np = real_np
    d_real_2x, d_real_half, d_half_2x = log["means"]
    assert all(d.shape == (N_COUNTERFACTUAL,) for d in log["means"]) and cf["n"] == N_COUNTERFACTUAL
    print(f"counterfactual means: {cf['cosine_distance_real_vs_2x']['mean']:.4e} {cf['cosine_distance_real_vs_half']['mean']:.4e} "
          f"{cf['cosine_distance_half_vs_2x']['mean']:.4e}")
    out = os.path.join(HERE, "panorgan_views.npz")
    per = {}
    for g in range(len(names)):
        per[f"picks_{g}"] = np.array(log["picks"][g], dtype=np.int64)
        per[f"Q_{g}"], per[f"K_{g}"] = Q[g].astype(np.float32), K[g].astype(np.float32)
    np.savez_compressed(out, datasets=np.array([r.dataset for r in rows]), series=np.array([r.series_dir for r in rows]),
                        names=np.array(names), d_real_2x=d_real_2x, d_real_half=d_real_half, d_half_2x=d_half_2x,
                        reference_retrieval=np.array(json.dumps(res)), reference_counterfactual=np.array(json.dumps(cf)),
                        n_per_dataset=np.int64(N_PER_DATASET), n_counterfactual=np.int64(N_COUNTERFACTUAL), seed=np.int64(SEED),
                        topk=np.int64(TOPK), draw_seed=np.int64(seed), **per)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
