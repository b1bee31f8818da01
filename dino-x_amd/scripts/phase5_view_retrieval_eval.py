#!/usr/bin/env python3
"""Phase 5: label-free view-retrieval evaluation on the MI355X engine -- drop-in for the reference script of the same name.

Protocol (the reference's): sample N rows of the eval split (``val.series_dir`` of the split manifest), draw two views of each
with the training script's PngDataset, embed both with the student backbone (CLS row, L2-normalised), and ask how often view 2
of sample i is the nearest (top-1) / among the k nearest (top-k) keys of view 1 of sample i.  ``passed`` is
``top1 >= ratio / N``.

What is kept from the reference is its interface: flags and defaults, seeding order (``random`` / ``numpy`` / ``torch`` seeded
with ``--seed``, then ``random.Random(seed).sample`` picks the rows), output file (``view_retrieval_step<step>_N<n>.json`` next to the
checkpoint unless ``--out``), JSON keys and their order, four stdout lines (``ok=``, ``passed=``, the metric line,
``metrics_json=``) and exit status (0 passed, 2 not passed).  What differs:

* the similarity matrix is never built: the embeddings stay on the device and ``dinox.ops.retrieval_rank`` returns the rank of
  every query's positive key from an exact-fp32 MFMA sweep (``dinox/retrieval.py``, ``csrc/retrieval.hip``); top-1 is
  ``rank == 0``, top-k is ``rank < k``, which is what argmax / argpartition give on a tie-free matrix;
* the JSON carries two more keys, ``embedding_std_mean`` and ``embedding_norm_mean`` of the un-normalised view-1 CLS rows (the
  collapse indicators of the reference's ``phase5_monitor.py``);
* ``--synthetic N`` (extension): rows come from the training script's ``SyntheticSliceDataset`` (N seeded HU stacks, seed =
  ``--seed``), so the script runs with no PNG tree; ``--index-csv`` / ``--split-manifest`` are then not read;
* ``--amp`` (extension): the backbone runs in bf16, as training does; the similarity is fp32 in both modes;
* ``--device cpu`` exits with the training script's message: there is no CPU compute path;
* non-finite embeddings (a diverged checkpoint) end the run with a message and exit status 1 instead of a score.

Checkpoints written by the reference and by this engine both load (restricted unpickler of ``zoo.hub.read_checkpoint``,
old-format keys migrated).
"""
from __future__ import annotations

import argparse
import json
import math
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

# (flag, argparse keywords): the reference's surface, then the two extensions
_FLAGS = (
    ("--checkpoint", dict(type=Path, required=True)),
    ("--index-csv", dict(type=Path, default=Path("data/processed/_index/index.csv"))),
    ("--split-manifest", dict(type=Path, default=None, help="val.series_dir lists the eval series (required unless --synthetic)")),
    ("--n", dict(type=int, default=4096, help="samples in the eval set")),
    ("--seed", dict(type=int, default=0)),
    ("--batch-size", dict(type=int, default=64)),
    ("--device", dict(type=str, default=None, help="cuda (cpu exits: no CPU compute path)")),
    ("--out", dict(type=Path, default=None, help="default: view_retrieval_step<step>_N<n>.json next to the checkpoint")),
    ("--topk", dict(type=int, default=5)),
    ("--ratio", dict(type=float, default=10.0, help="gate: top1 >= ratio / N")),
    ("--scale-aware", dict(action="store_true", help="model with the scale embedding (must match the checkpoint)")),
    ("--synthetic", dict(type=int, default=0, metavar="N", help="extension: N seeded synthetic HU stacks instead of a PNG index")),
    ("--amp", dict(action="store_true", help="extension: bf16 backbone (the similarity stays fp32)")),
)

# key order of the reference's metrics file; the two embedding statistics follow
_JSON_KEYS = ("kind", "version", "created_at", "checkpoint", "step", "index_csv", "split_manifest", "img_size", "n", "seed", "batch_size",
              "topk", "top1", "topk_acc", "random_baseline", "ratio_vs_random", "pass_ratio", "passed", "seconds", "model",
              "embedding_std_mean", "embedding_norm_mean")
_MODEL_KEYS = ("name", "patch", "dim", "depth", "heads", "mlp_ratio", "out_dim")
_WINDOW_DEFAULTS = {"rw_level_min": -400.0, "rw_level_max": 400.0, "rw_width_min": 800.0, "rw_width_max": 2000.0}


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Phase 5 label-free view-retrieval eval")
    for flag, kw in _FLAGS:
        ap.add_argument(flag, **kw)
    return ap


def _check_args(args) -> None:
    need = [("Checkpoint", args.checkpoint)]
    if not args.synthetic:
        if args.split_manifest is None:
            raise SystemExit("--split-manifest is required (or use --synthetic N)")
        need += [("index_csv", args.index_csv), ("split_manifest", args.split_manifest)]
    for what, path in need:
        if not path.exists():
            raise FileNotFoundError(f"{what} not found: {path}")
    for flag, bad in (("--n", args.n <= 0), ("--topk", args.topk <= 0)):
        if bad:
            raise SystemExit(f"{flag} must be > 0")
    if args.synthetic < 0:
        raise SystemExit("--synthetic must be >= 0")


def _student_from(ckpt: Path, scale_aware: bool, device, train):
    """(student in eval mode on device, step, model config, image size, training config dict) of a training checkpoint."""
    from zoo.hub import read_checkpoint
    blob = read_checkpoint(ckpt, "cpu")
    cfg = blob.get("config", {})
    mc = cfg.get("model", {})
    if not isinstance(mc, train.ModelConfig):
        mc = train.ModelConfig(**mc)
    size = int(cfg.get("img_size", 224))
    weights = blob["student"]
    if train.needs_migration(weights):
        weights = train.migrate_state_dict(weights)
    net = train.DinoStudentTeacher(
        train.PatchViT(img_size=size, scale_aware=scale_aware, use_grad_checkpoint=False,
                       **{f: getattr(mc, f) for f in ("patch", "dim", "depth", "heads", "mlp_ratio")}),
        out_dim=mc.out_dim)
    net.load_state_dict(weights, strict=True)          # a --scale-aware that does not match the checkpoint is an error, as in the reference
    return net.to(device).eval(), int(blob.get("step", 0) or 0), mc, size, cfg


def _eval_dataset(args, train, size: int, cfg: dict):
    window = {k: float(cfg.get(k, v)) for k, v in _WINDOW_DEFAULTS.items()}
    if args.synthetic:
        return train.SyntheticSliceDataset(args.synthetic, seed=args.seed, img_size=size, **window)
    held_out = json.loads(args.split_manifest.read_text()).get("val", {}).get("series_dir", [])
    if not isinstance(held_out, list) or not held_out:
        raise SystemExit(f"Invalid split manifest (missing val.series_dir): {args.split_manifest}")
    held_out = {str(s) for s in held_out}
    # every val row goes into the dataset, so that the (z-1, z, z+1) context of a sampled slice is what training saw
    rows = [r for r in train._load_index_rows(args.index_csv) if str(r.series_dir) in held_out]
    if not rows:
        raise SystemExit("No rows remain after filtering to val.series_dir")
    return train.PngDataset(rows, img_size=size, **window)


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    _check_args(args)
    for seed_fn in (random.seed, np.random.seed, torch.manual_seed):        # the reference's order
        seed_fn(args.seed)
    want = torch.device(args.device or "cuda")
    if want.type != "cuda" or not torch.cuda.is_available():
        raise SystemExit("this engine computes on MI355X only: no CUDA/HIP device available or --device cpu requested")

    import phase5_big_run as train
    from dinox import retrieval

    student, step, mc, size, cfg = _student_from(args.checkpoint, args.scale_aware, want, train)
    ds = _eval_dataset(args, train, size, cfg)
    if len(ds) < args.n:
        print(f"⚠️  Requested --n={args.n} but only {len(ds)} val rows available; capping n.")
        args.n = len(ds)
    picked = random.Random(args.seed).sample(range(len(ds)), k=args.n)

    started = time.time()
    try:
        res = retrieval.view_retrieval(student, ds, picked, batch_size=args.batch_size, scale_aware=args.scale_aware, topk=args.topk,
                                       ratio=args.ratio, amp_dtype=torch.bfloat16 if args.amp else None)
    except FloatingPointError as e:
        raise SystemExit(f"ok=false\n{e}")
    facts = dict(res, kind="phase5_view_retrieval", version=1, created_at=datetime.now(timezone.utc).isoformat(),
                 checkpoint=str(args.checkpoint), step=step, index_csv=str(args.index_csv), split_manifest=str(args.split_manifest),
                 img_size=size, n=args.n, seed=args.seed, batch_size=args.batch_size, topk=int(args.topk), pass_ratio=float(args.ratio),
                 seconds=time.time() - started,
                 model=dict({f: getattr(mc, f) for f in _MODEL_KEYS}, ln_out_dim=math.log(float(mc.out_dim))))
    dest = args.out or args.checkpoint.parent / f"view_retrieval_step{step}_N{args.n}.json"
    dest.parent.mkdir(parents=True, exist_ok=True)
    dest.write_text(json.dumps({k: facts[k] for k in _JSON_KEYS}, indent=2) + "\n")

    print("ok=true",
          f"passed={str(facts['passed']).lower()}",
          f"top1={facts['top1']:.6f} top{args.topk}={facts['topk_acc']:.6f} baseline={facts['random_baseline']:.6f} "
          f"ratio={facts['ratio_vs_random']:.2f} seconds={facts['seconds']:.1f}",
          f"metrics_json={dest}", sep="\n")
    return 0 if facts["passed"] else 2


if __name__ == "__main__":
    raise SystemExit(main())
