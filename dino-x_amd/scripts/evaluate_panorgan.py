#!/usr/bin/env python3
"""Pan-organ evaluation on the MI355X engine: the nearest-neighbour metrics of the reference script of the same name.

Protocol (the reference's): every slice of the eval split (``val.series_dir`` of the split manifest) is embedded ONCE with the student
backbone from a deterministic view (fixed window level 40 / width 400, centred crop, no flip; ``dinox.retrieval.eval_view``), CLS row,
L2-normalised; the metrics are computed from those embeddings and the ``dataset`` column of the index.

What is here:

* ``metrics.domain_clustering`` -- the reference's metric 4 (``metric_domain_clustering``): how often the 10 nearest neighbours of a
  slice come from the slice's own dataset, with per-dataset enrichment over prevalence.  Same keys, same arithmetic, same three stdout
  lines.  The reference builds S = E E^T on the host (17 GB at 65 536 slices) and runs argpartition over its rows; here the embeddings
  stay on the device and ``dinox.ops.knn_topk`` (csrc/knn.hip) returns the neighbours from an exact-fp32 MFMA sweep.
* ``metrics.knn_probe`` -- extension: the weighted k-NN classifier of the DINO paper (k = 20, weights exp(s / 0.07)), leave-one-out
  over the dataset labels (``dinox.neighbors.knn_probe``).

What is kept from the reference is its interface: the flags that apply and their defaults, the seeding order, the result envelope
(``kind``, ``version``, ``created_at``, ``checkpoint``, ``step``, ``scale_aware``, ``seed``, ``val_slices``, ``datasets``, ``model``,
``metrics``, ``seconds``), the output file (``panorgan_eval_step<step>.json`` next to the checkpoint unless ``--out``), ``ok=true`` as
the last line and exit status 0.

With ``--probes`` three more of the reference's metrics are written, all linear algebra on the embedding matrix the script already holds on
the device (``dinox.probes``; csrc/probe.hip, csrc/gram.hip):

* ``metrics.dataset_discrimination_probe`` -- metric 2: multinomial logistic regression over the dataset labels, series-level split,
  series bootstrap; every evaluation of the fit is one kernel pass over the train rows.
* ``metrics.spacing_prediction`` -- metric 5: ridge regression of log(spacing_x) from the Gram matrix of [E | y].
* ``metrics.embedding_stats`` -- metric 6: centroids, spread, first principal axis against spacing, cross-dataset centroid cosines.

Same keys and the reference's stdout lines.  The probes are opt-in and their two flags (``--probes``, and ``--skip-probes``, the explicit
form of the default, which wins when both are given) are added by ``build_parser(probe_flags=True)``, the parser ``main`` uses: the
result file of a run without them, and the flag surface ``build_parser()`` returns, are what the nearest-neighbour tests pin.

With ``--view-metrics`` the reference's remaining two metrics are written, the ones that need backbone passes of their own
(``dinox.retrieval``; csrc/retrieval.hip):

* ``metrics.view_retrieval_per_dataset`` -- metric 1: per dataset, ``--n-retrieval`` (512) slices, two random views each, how often view
  2 of a slice is the nearest of its dataset's keys to view 1.  The reference's sampling and RNG position (right after seeding, before the
  deterministic embedding pass); one embedding pass over all datasets' picks and one windowed rank call instead of an S = Q K^T per
  dataset.  ``--skip-view-retrieval`` leaves it out (no key, the reference's SKIPPED line).
* ``metrics.spacing_counterfactual`` -- metric 3: ``--n-counterfactual`` (256) slices, the same pixels embedded with the real, the doubled
  and the halved spacing; mean / std / median of the three cosine distances.  Without ``--scale-aware`` the reference's
  ``{"skipped": true, ...}`` dict.

Same keys and the reference's stdout lines; both keys come after the existing ones in ``metrics``.  The four flags are added by
``build_parser(view_flags=True)``; a run without ``--view-metrics`` writes what it wrote before.

Extensions: ``--synthetic N`` (N seeded synthetic HU stacks, seed = ``--seed``, instead of a PNG index; the dataset of sample i is
``synthetic_label(i)``), ``--amp-dtype bf16`` (bf16 backbone; the similarity is fp32 either way), ``--dump-embeddings FILE`` (the
embeddings and labels the metrics were computed from, as .npz: ``embeddings`` fp32 [N, D], ``labels``).  ``--device cpu`` exits with
the training script's message: there is no CPU compute path.
"""
from __future__ import annotations

import argparse
import json
import random
import sys
import time
from datetime import datetime, timezone
from pathlib import Path

import numpy as np
import torch

_SCRIPTS = Path(__file__).resolve().parent
for _p in (str(_SCRIPTS), str(_SCRIPTS.parent)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

# (flag, argparse keywords): the reference's surface that applies, then the extensions
_FLAGS = (
    ("--checkpoint", dict(type=Path, required=True)),
    ("--index-csv", dict(type=Path, default=Path("data/processed/combined-mvp/index.csv"))),
    ("--split-manifest", dict(type=Path, default=None, help="val.series_dir lists the eval series (required unless --synthetic)")),
    ("--scale-aware", dict(action="store_true", help="model with the scale embedding (must match the checkpoint)")),
    ("--out", dict(type=Path, default=None, help="default: panorgan_eval_step<step>.json next to the checkpoint")),
    ("--batch-size", dict(type=int, default=64)),
    ("--seed", dict(type=int, default=42)),
    ("--device", dict(type=str, default=None, help="cuda (cpu exits: no CPU compute path)")),
    ("--synthetic", dict(type=int, default=0, metavar="N", help="extension: N seeded synthetic HU stacks instead of a PNG index")),
    ("--amp-dtype", dict(type=str, default="fp32", choices=("fp32", "bf16"), help="extension: backbone precision (the similarity stays fp32)")),
    ("--dump-embeddings", dict(type=Path, default=None, metavar="FILE", help="extension: write the embeddings and labels as .npz")),
)

# the probe block (metrics 2, 5, 6): build_parser(probe_flags=True)
_PROBE_FLAGS = (
    ("--probes", dict(action="store_true", help="extension: also run the logistic probe, the spacing ridge and the embedding statistics")),
    ("--skip-probes", dict(action="store_true", help="extension: do not run them (the default; wins over --probes)")),
)

# the view block (metrics 1, 3): build_parser(view_flags=True)
_VIEW_FLAGS = (
    ("--view-metrics", dict(action="store_true", help="extension: also run per-dataset view retrieval and the spacing counterfactual")),
    ("--n-retrieval", dict(type=int, default=512, help="samples per dataset for view retrieval")),
    ("--n-counterfactual", dict(type=int, default=256, help="samples for the spacing counterfactual")),
    ("--skip-view-retrieval", dict(action="store_true", help="skip view retrieval")),
)

_MODEL_KEYS = ("name", "patch", "dim", "depth", "heads")
_SYNTHETIC_DATASETS = ("synthetic_a", "synthetic_b", "synthetic_c")
DOMAIN_K, PROBE_K, PROBE_T = 10, 20, 0.07


def synthetic_label(i: int) -> str:
    """Dataset of synthetic sample i: i mod 7 in {0..3} / {4, 5} / {6} -- three interleaved classes of about 4/7, 2/7 and 1/7 of the rows."""
    r = i % 7
    return _SYNTHETIC_DATASETS[0 if r < 4 else (1 if r < 6 else 2)]


def build_parser(probe_flags: bool = False, view_flags: bool = False) -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Pan-organ evaluation: domain clustering, k-NN probe, linear probes and embedding statistics")
    for flag, kw in _FLAGS + (_PROBE_FLAGS if probe_flags else ()) + (_VIEW_FLAGS if view_flags else ()):
        ap.add_argument(flag, **kw)
    return ap


def probe_series(rows, synthetic: bool) -> list:
    """The series handed to the probes: the row's series_dir; in --synthetic mode ``series_dir:dataset``, because synthetic_label deals
    the samples of one synthetic series to several datasets and a series of the split has one dataset."""
    return [f"{r.series_dir}:{r.dataset}" if synthetic else str(r.series_dir) for r in rows]


def run_probes(E, spacings, labels, series, seed: int, metrics: dict) -> None:
    """Metrics 2, 5 and 6 into ``metrics``, with the reference's stdout lines (steps 3 to 5 of 5)."""
    from dinox import probes
    print("\n[3/5] Dataset discrimination linear probe...")
    probe = probes.logistic_probe(E, labels, series, seed=seed)
    metrics["dataset_discrimination_probe"] = probe
    if "accuracy" in probe:
        print(f"  Accuracy: {probe['accuracy']:.3f} (CI: {probe['accuracy_ci95']})")
        print(f"  AUC: {probe['auc']:.3f}")
    else:
        print(f"  ⚠️  {probe.get('error', 'unknown error')}")
    print("\n[4/5] Spacing prediction sanity check...")
    ridge = probes.spacing_ridge(E, spacings, labels, series, seed=seed)
    metrics["spacing_prediction"] = ridge
    if "r2" in ridge:
        print(f"  R²: {ridge['r2']:.3f}")
        print(f"  MAE(log spacing): {ridge['mae_log_spacing']:.4f}")
    else:
        print(f"  ⚠️  {ridge.get('error', 'unknown error')}")
    print("\n[5/5] Embedding statistics...")
    stats = probes.embedding_stats(E, spacings, labels)
    metrics["embedding_stats"] = stats
    for name, d in stats["per_dataset"].items():
        print(f"  {name}: std={d['embedding_std']:.4f} intra_cos={d['intra_cosine_to_centroid']:.3f} "
              f"pca1_sp_corr={d['pca1_spacing_correlation']:.3f}")
    for pair, cos in stats["cross_dataset_centroid_cosine"].items():
        print(f"  Cross: {pair} = {cos:.3f}")


def run_view_retrieval(student, ds, labels, args, amp_dtype, metrics: dict) -> None:
    """Metric 1 into ``metrics`` with the reference's stdout lines.  ``ds`` is in its random-view mode for the call."""
    from dinox import retrieval
    if args.skip_view_retrieval:
        print("\n[views 1/2] Per-dataset view retrieval... SKIPPED (--skip-view-retrieval)")
        return
    print("\n[views 1/2] Per-dataset view retrieval...")
    raw, ds.raw_views = ds.raw_views, False                 # items = ([view 1, view 2], spacing)
    try:
        res = retrieval.view_retrieval_per_dataset(student, ds, labels, n_per_dataset=args.n_retrieval, seed=args.seed,
                                                   batch_size=args.batch_size, scale_aware=args.scale_aware, amp_dtype=amp_dtype)
    finally:
        ds.raw_views = raw
    metrics["view_retrieval_per_dataset"] = res
    for name, d in res.items():
        print(f"  {name}: top1={d['top1']:.4f} ratio={d['ratio_vs_random']:.1f}×")


def run_counterfactual(student, ds, size: int, args, amp_dtype, metrics: dict) -> None:
    """Metric 3 into ``metrics`` with the reference's stdout lines."""
    from dinox import retrieval
    print("\n[views 2/2] Spacing counterfactual test...")
    if not args.scale_aware:
        print("  Skipped (baseline model has no scale embedding)")
        metrics["spacing_counterfactual"] = dict(retrieval.COUNTERFACTUAL_SKIPPED)
        return
    cf = retrieval.spacing_counterfactual(student, ds, size, n=args.n_counterfactual, seed=args.seed, batch_size=args.batch_size,
                                          amp_dtype=amp_dtype)
    metrics["spacing_counterfactual"] = cf
    print(f"  real→2x: dist={cf['cosine_distance_real_vs_2x']['mean']:.4f}")
    print(f"  real→½x: dist={cf['cosine_distance_real_vs_half']['mean']:.4f}")


def _check_args(args) -> None:
    need = [("Checkpoint", args.checkpoint)]
    if not args.synthetic:
        if args.split_manifest is None:
            raise SystemExit("--split-manifest is required (or use --synthetic N)")
        need += [("index_csv", args.index_csv), ("split_manifest", args.split_manifest)]
    for what, path in need:
        if not path.exists():
            raise FileNotFoundError(f"{what} not found: {path}")
    if args.synthetic < 0:
        raise SystemExit("--synthetic must be >= 0")
    if args.batch_size <= 0:
        raise SystemExit("--batch-size must be > 0")
    if args.n_retrieval <= 0 or args.n_counterfactual <= 0:
        raise SystemExit("--n-retrieval and --n-counterfactual must be > 0")


def main(argv=None) -> int:
    args = build_parser(probe_flags=True, view_flags=True).parse_args(argv)
    _check_args(args)
    for seed_fn in (random.seed, np.random.seed, torch.manual_seed):        # the reference's order
        seed_fn(args.seed)
    want = torch.device(args.device or "cuda")
    if want.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit("this engine computes on MI355X only: no CUDA/HIP device available or --device cpu requested")

    import phase5_big_run as train
    import phase5_view_retrieval_eval as vr                # checkpoint loading and the eval split are that script's
    from dinox import neighbors, retrieval

    student, step, mc, size, cfg = vr._student_from(args.checkpoint, args.scale_aware, want, train)
    ds = vr._eval_dataset(args, train, size, cfg)
    ds.raw_views = True                                    # items = (u16 stack, view draws, spacing); the draws are not used
    if args.synthetic:
        for i, r in enumerate(ds.rows):
            r.dataset = synthetic_label(i)
    n = len(ds)
    if n <= DOMAIN_K:
        raise SystemExit(f"{n} eval slices: the domain-clustering metric needs more than k = {DOMAIN_K}")
    labels = [r.dataset if r.dataset else "unknown" for r in ds.rows]
    named, counts = np.unique([r.dataset for r in ds.rows if r.dataset], return_counts=True)
    datasets_found = [str(d) for d in named]
    print(f"Val set: {n} slices across {len(datasets_found)} datasets")
    for d, c in zip(datasets_found, counts):
        print(f"  {d}: {int(c)} slices")

    started = time.time()
    results = {
        "kind": "panorgan_evaluation", "version": 1, "created_at": datetime.now(timezone.utc).isoformat(), "checkpoint": str(args.checkpoint),
        "step": step, "scale_aware": bool(args.scale_aware), "seed": args.seed, "val_slices": n, "datasets": datasets_found,
        "model": {f: getattr(mc, f) for f in _MODEL_KEYS}, "metrics": {},
    }

    amp_dtype = torch.bfloat16 if args.amp_dtype == "bf16" else None
    view_metrics, t_views = {}, None
    if args.view_metrics:                                  # metric 1 first: the reference's position in the global RNG streams
        t0 = time.time()
        try:
            run_view_retrieval(student, ds, labels, args, amp_dtype, view_metrics)
        except FloatingPointError as e:
            raise SystemExit(f"ok=false\n{e}")
        torch.cuda.synchronize()
        t_views = [time.time() - t0, 0.0]

    print("\n[embed] Embedding all val slices (deterministic)...")
    t0 = time.time()
    E, spacings = retrieval.embed_eval_slices(student, ds, list(range(n)), size, batch_size=args.batch_size, scale_aware=args.scale_aware,
                                       amp_dtype=amp_dtype)
    if not bool(torch.isfinite(E).all()):
        raise SystemExit("ok=false\nnon-finite embeddings (diverged checkpoint?); no neighbours can be given")
    torch.cuda.synchronize()
    t_embed = time.time() - t0
    print(f"  Embedded {E.shape[0]} slices → ({E.shape[1]}D) in {t_embed:.2f}s")
    if args.dump_embeddings is not None:
        args.dump_embeddings.parent.mkdir(parents=True, exist_ok=True)
        with open(args.dump_embeddings, "wb") as f:
            np.savez(f, embeddings=E.cpu().numpy(), labels=np.array(labels))

    t0 = time.time()
    print("\n[1/2] Domain clustering analysis...")
    clustering = neighbors.domain_clustering(E, labels, k=DOMAIN_K)
    results["metrics"]["domain_clustering"] = clustering
    print(f"  Same-dataset NN rate: {clustering['overall_same_dataset_rate']:.3f}")
    print(f"  Expected random: {clustering['expected_random_rate']:.3f}")
    print(f"  Enrichment: {clustering['enrichment_vs_random']:.1f}×")

    print("\n[2/2] Weighted k-NN probe over the dataset labels (leave-one-out)...")
    probe = neighbors.knn_probe(E, labels, k=min(PROBE_K, n - 1), temperature=PROBE_T)
    results["metrics"]["knn_probe"] = probe
    print(f"  Accuracy: {probe['accuracy']:.3f}")
    t_neigh = time.time() - t0

    t_probes = None
    if args.probes and not args.skip_probes:
        t0 = time.time()
        run_probes(E, spacings, labels, probe_series(ds.rows, bool(args.synthetic)), args.seed, results["metrics"])
        t_probes = time.time() - t0

    if args.view_metrics:
        t0 = time.time()
        try:
            run_counterfactual(student, ds, size, args, amp_dtype, view_metrics)
        except FloatingPointError as e:
            raise SystemExit(f"ok=false\n{e}")
        torch.cuda.synchronize()
        t_views[1] = time.time() - t0
        results["metrics"].update(view_metrics)            # after the existing keys, metric 1 before metric 3

    results["seconds"] = time.time() - started
    out = args.out or args.checkpoint.parent / f"panorgan_eval_step{step}.json"
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(results, indent=2) + "\n")
    print(f"\n{'─' * 60}")
    print(f"Evaluation complete in {results['seconds']:.1f}s (embedding {t_embed:.2f}s, neighbours {t_neigh:.3f}s"
          + (f", probes {t_probes:.3f}s" if t_probes is not None else "")
          + (f", view retrieval {t_views[0]:.2f}s, counterfactual {t_views[1]:.2f}s)" if t_views is not None else ")"))
    print(f"Results: {out}")
    print("ok=true")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
