#!/usr/bin/env python3
"""Embed every slice of a CT series: ``(Z, H, W)`` .npy in, ``(Z', D)`` CLS embeddings out.

    python dino-x_amd/scripts/encode_volume.py --checkpoint runs/<run>/checkpoint_00005000.pth --volume series.npy \\
        --spacing 0.7 0.7 2.0 --amp --out emb.npy

The model comes from ``zoo.hub.load_model`` (a training checkpoint, a hub directory or a hub id); the work is
``zoo.encode.encode_volume``: the volume crosses to the device once, one HIP kernel windows, resizes and normalises every plane once
for the 2.5D stacks (z-1, z, z+1) it shows in, and the slices are forwarded in chunks of ``--batch-size``.  ``--amp`` runs the forward
under bf16 autocast (the throughput mode; the default fp32 is the parity mode).  Prints ``slices=... seconds=... slices_per_s=...``.
"""
from __future__ import annotations

import argparse
import contextlib
import sys
import time
from pathlib import Path

import numpy as np
import torch

_SCRIPTS = Path(__file__).resolve().parent
for _p in (str(_SCRIPTS), str(_SCRIPTS.parent)):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Per-slice embeddings of a (Z, H, W) volume")
    ap.add_argument("--checkpoint", required=True, help="training checkpoint (.pth), hub directory or hub id")
    ap.add_argument("--volume", required=True, help=".npy file holding a (Z, H, W) array")
    ap.add_argument("--spacing", type=float, nargs=3, required=True, metavar=("SX", "SY", "SZ"), help="mm per pixel in x, y and slice spacing")
    ap.add_argument("--input-format", default="hu_float", choices=("hu_float", "hu16_png", "windowed_float"))
    ap.add_argument("--hu-level", type=float, default=40.0)
    ap.add_argument("--hu-width", type=float, default=400.0)
    ap.add_argument("--context", default="neighbours", choices=("neighbours", "replicate"))
    ap.add_argument("--z-stride", type=int, default=1)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--amp", action="store_true", help="forward under torch.autocast(bfloat16)")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--out", required=True, help="output .npy: (Z', D) fp32")
    return ap


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    from zoo.encode import encode_volume
    from zoo.hub import load_model
    model = load_model(args.checkpoint, device=args.device)
    volume = np.load(args.volume, allow_pickle=False)
    amp = torch.autocast("cuda", dtype=torch.bfloat16) if args.amp else contextlib.nullcontext()
    t0 = time.perf_counter()
    with amp:
        feats = encode_volume(model, volume, tuple(args.spacing), input_format=args.input_format, hu_level=args.hu_level,
                              hu_width=args.hu_width, context=args.context, z_stride=args.z_stride, batch_size=args.batch_size)
    emb = feats[:, 0, :].float().cpu().numpy()              # (the copy waits for the device)
    dt = time.perf_counter() - t0
    np.save(args.out, emb)
    print(f"slices={emb.shape[0]} seconds={dt:.3f} slices_per_s={emb.shape[0] / dt:.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
