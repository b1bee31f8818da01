#!/usr/bin/env python3
"""Phase-5 training monitor for a checkpoint (safe to run beside a training job) -- port of the reference script of the same name.

Loads the student backbone of a training checkpoint (``zoo.hub``), picks one fixed sample (``--fixed-png``, else a draw from
``--sample-seed``) plus ``--batch-size`` sampled slices, windows them at a FIXED level / width (default -600 / 1500, the reference's
lung window) exactly as the reference's ``_load_fixed_sample_tensor`` does -- (z-1, z, z+1) stack, window to [0, 1], 8-bit bilinear
resize where the slice is not already ``img_size`` -- and runs ``dinox.monitor.run_monitor`` on them.  Under
``--out-dir/<timestamp>_step<step>/step_<step>/`` it writes the reference's pictures (``heatmap`` = patch-token-norm proxy, ``input``)
and ``stats.json`` with the reference's keys (``step``, ``embedding_std_mean``, ``embedding_norm_mean``, ``sample``), and what the
reference cannot produce: ``attention`` = the CLS softmax rows of the last block per head, with the per-head entropies in
``stats.json``.  Arrays are ``.npy``; PNG copies are written where PIL imports.

Extensions: ``--rollout`` (also ``rollout`` = the attention rollout of CLS through every block, heads averaged, residual 0.5:
``PatchViT.attention_rollout``), ``--synthetic N`` (seeded HU stacks of the training script instead of ``--index-csv``), ``--scale-aware`` (must match
the checkpoint), ``--amp`` (bf16 backbone).  Without a HIP device the script exits with a message: there is no CPU compute path.
"""
from __future__ import annotations

import argparse
import json
import random
import sys
from datetime import datetime
from pathlib import Path

import numpy as np
import torch

_SCRIPTS = Path(__file__).resolve().parent
for _p in (str(_SCRIPTS), str(_SCRIPTS.parent)):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Phase 5 Monitor: Checkpoints & Heatmaps (MI355X engine)")
    ap.add_argument("--checkpoint", type=Path, required=True, help="Path to .pth checkpoint")
    ap.add_argument("--index-csv", type=Path, default=Path("data/processed/_index/index.csv"))
    ap.add_argument("--batch-size", type=int, default=32, help="Batch size for embedding stats")
    ap.add_argument("--fixed-png", type=Path, help="Specific PNG to visualize")
    ap.add_argument("--sample-seed", type=int, default=42, help="Seed for random sample selection")
    ap.add_argument("--level", type=float, default=-600.0)
    ap.add_argument("--width", type=float, default=1500.0)
    ap.add_argument("--out-dir", type=Path, default=Path("data/monitor/phase5"))
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="extension: N seeded synthetic HU stacks instead of --index-csv")
    ap.add_argument("--scale-aware", action="store_true", help="model with the scale embedding (must match the checkpoint)")
    ap.add_argument("--amp", action="store_true", help="extension: bf16 backbone")
    ap.add_argument("--rollout", action="store_true",
                    help="extension: also write the attention rollout of CLS through every block (rollout.npy / rollout.png, "
                         "rollout_patch_mass and rollout_entropy in stats.json)")
    return ap


def check_args(args) -> None:
    """Host-side argument errors, before any device or checkpoint is touched."""
    if not args.checkpoint.exists():
        raise FileNotFoundError(f"Checkpoint not found: {args.checkpoint}")
    if args.synthetic < 0:
        raise SystemExit("--synthetic must be >= 0")
    if args.batch_size <= 0:
        raise SystemExit("--batch-size must be > 0")
    if args.width <= 0:
        raise SystemExit("--width must be > 0")
    if not args.synthetic and not args.index_csv.exists():
        raise FileNotFoundError(f"index_csv not found: {args.index_csv} (or use --synthetic N)")
    if args.synthetic and args.fixed_png is not None:
        raise SystemExit("--fixed-png names a row of --index-csv: not with --synthetic")


def load_sample(ds, row, img_size: int, level: float, width: float, train) -> torch.Tensor:
    """(3, img_size, img_size) in [0, 1]: the reference's _load_fixed_sample_tensor on the dataset's (z-1, z, z+1) stack."""
    out = []
    for u16 in ds._stack(row):
        w = train.hu_window01(np.asarray(u16), level, width)
        if w.shape != (img_size, img_size):
            from PIL import Image
            im = Image.fromarray((w * 255).astype(np.uint8)).resize((img_size, img_size), Image.BILINEAR)
            w = np.array(im, dtype=np.float32) / 255.0
        out.append(w.astype(np.float32))
    return torch.from_numpy(np.stack(out, 0)).contiguous()


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    check_args(args)
    if not torch.cuda.is_available():
        raise SystemExit("this engine computes on MI355X only: no CUDA/HIP device available")
    device = torch.device("cuda")

    import phase5_big_run as train
    from dinox import ops
    from dinox.monitor import run_monitor
    from zoo import hub

    print(f"Loading checkpoint: {args.checkpoint}")
    payload = hub.read_checkpoint(args.checkpoint, "cpu")
    step = int(payload.get("step", 0) or 0) if isinstance(payload, dict) else 0
    del payload
    backbone = hub.load_from_training_checkpoint(args.checkpoint, device=device, config_override={"scale_aware": bool(args.scale_aware)})
    size = backbone.img_size
    print(f"Model: patch={backbone.patch} dim={backbone.dim} depth={len(backbone.blocks)} img_size={size}")

    if args.synthetic:
        ds = train.SyntheticSliceDataset(args.synthetic, seed=args.sample_seed, img_size=size)
    else:
        ds = train.PngDataset(train._load_index_rows(args.index_csv), img_size=size)
    rows = ds.rows
    print(f"Loaded {len(rows)} rows from index")
    if not rows:
        raise SystemExit("the index holds no rows")
    if args.fixed_png:
        target = next((r for r in rows if Path(r.png_path) == args.fixed_png), None)
        if target is None:
            raise ValueError(f"PNG not found in index: {args.fixed_png}")
    else:
        target = random.Random(args.sample_seed).choice(rows)
    print(f"Visualizing sample: {target.png_path}")
    picked = [target] + random.Random(args.sample_seed).sample(rows, min(args.batch_size, len(rows)))       # the reference's two draws
    x = torch.stack([load_sample(ds, r, size, args.level, args.width, train) for r in picked], 0).to(device)
    spacing = None
    if backbone.scale_aware:
        spacing = torch.tensor([[r.spacing_x, r.spacing_y, r.spacing_z] for r in picked], dtype=torch.float32, device=device)

    run_out = args.out_dir / f"{datetime.now().strftime('%Y%m%d_%H%M%S')}_step{step}"
    with ops.compute_dtype(torch.bfloat16 if args.amp else torch.float32):
        stats = run_monitor(backbone, x, spacing, run_out, step, extra={"sample": str(target.png_path)}, rollout=args.rollout)
    print(f"Saved heatmap, attention and input to: {stats['dir']}")
    print(f"Stats: std={stats['embedding_std_mean']:.4f}, norm={stats['embedding_norm_mean']:.4f}, "
          f"attention_entropy={[round(v, 3) for v in stats['attention_entropy']]} (max {stats['attention_entropy_max']:.3f})")
    if args.rollout:
        print(f"Rollout: patch_mass={stats['rollout_patch_mass']:.4f}, entropy={stats['rollout_entropy']:.3f} (max {stats['attention_entropy_max']:.3f})")
    print(f"monitor_dir={stats['dir']}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
