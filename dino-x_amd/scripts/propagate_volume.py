#!/usr/bin/env python3
"""Carry the labels of one annotated slice through a CT series by patch-feature affinity alone (dense label propagation, Caron et al.
2021, along z): one-shot volume segmentation without a trained head, and a head-free score of a checkpoint's dense features.

    python dino-x_amd/scripts/propagate_volume.py --checkpoint C --volume series.npy --spacing 0.8 0.8 2.5 --seed-slice 40 \\
        --seed-labels seeds.npy --num-classes 3 --out labels.npy
    python dino-x_amd/scripts/propagate_volume.py --checkpoint C --volume series.npy --spacing 0.8 0.8 2.5 --labels gt.npy \\
        --num-classes 3 --out labels.npy --report case.json

The patch tokens come from ``zoo.encode.encode_volume(..., return_all_tokens=True)`` (CLS and registers dropped); the walk is
``dinox.propagate.propagate_labels`` on ``ops.label_propagate`` (csrc/labelprop.hip).  ``--seed-labels`` is uint8 with 255 = ignore, (Z, H, W)
of which only the seed slices are read, or (H, W) for a single seed; labels are brought to the model's grid by
``dinox.segment.resample_labels_nearest``.  Without ``--seed-slice`` and with ``--labels``: evaluation mode, the seed is the slice of the
ground truth with the most foreground voxels and its labels are the seed's.  ``--synthetic Z`` needs no data: a seeded series of bright
ellipses, one per class, that drift and shrink slowly along z, with its own ground truth.  ``--keep-largest`` / ``--min-component-mm3`` clean
the result through ``dinox.segment.postprocess_volume``.  ``--report`` (needs ground truth) holds per-class and mean Dice / IoU over the
non-seed slices, the same per distance |z - seed|, the parameters and the seconds taken.  The last line printed is ``ok=true``.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

_SCRIPTS = Path(__file__).resolve().parent
for _p in (str(_SCRIPTS), str(_SCRIPTS.parent)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

REPORT_KEYS = ("checkpoint", "volume", "slices", "grid", "num_classes", "seeds", "params", "per_class", "mean", "by_distance", "seconds")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="One-shot volume segmentation by dense label propagation along z",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--checkpoint", required=True, help="training checkpoint (.pth), hub directory or hub id")
    ap.add_argument("--volume", type=Path, default=None, help=".npy file holding a (Z, H, W) series")
    ap.add_argument("--spacing", type=float, nargs=3, default=None, metavar=("SX", "SY", "SZ"), help="mm per pixel in x, y and the slice spacing")
    ap.add_argument("--seed-slice", type=int, action="append", default=None, metavar="Z", help="an annotated slice; repeatable")
    ap.add_argument("--seed-labels", type=Path, default=None, help=".npy uint8 (Z, H, W), only the seed slices are read, or (H, W) for one seed")
    ap.add_argument("--num-classes", type=int, required=True, help="classes including the background 0")
    ap.add_argument("--topk", type=int, default=5, help="neighbours per patch")
    ap.add_argument("--context-frames", type=int, default=7, help="propagated slices kept as context beside the seed")
    ap.add_argument("--radius", type=int, default=12, help="half-width of the search window in patches (negative: the whole grid)")
    ap.add_argument("--temperature", type=float, default=0.1, help="softmax temperature of the vote")
    ap.add_argument("--amp", action="store_true", help="encode under torch.autocast(bfloat16)")
    ap.add_argument("--batch-size", type=int, default=64, help="slices per forward")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--keep-largest", action="store_true", help="keep only the largest 3-D component of every class >= 1")
    ap.add_argument("--min-component-mm3", type=float, default=0.0, metavar="V", help="remove the 3-D components of the classes >= 1 under V mm^3")
    ap.add_argument("--connectivity", type=int, choices=(6, 18, 26), default=26, help="neighbourhood of a 3-D connected component")
    ap.add_argument("--out", type=Path, required=True, help="output .npy: uint8 (Z, S, S) on the model's grid")
    ap.add_argument("--labels", type=Path, default=None, help=".npy ground truth, uint8 (Z, H, W) or (Z, S, S), 255 = ignore")
    ap.add_argument("--report", type=Path, default=None, help="JSON of the scores (needs --labels or --synthetic)")
    ap.add_argument("--synthetic", type=int, default=0, metavar="Z", help="a synthetic series of Z slices with its own ground truth")
    ap.add_argument("--dump-trace", type=Path, default=None, help=".npz of every step: target, seed, context slots, neighbours and scores")
    return ap


def check_args(ap: argparse.ArgumentParser, args: argparse.Namespace) -> None:
    """The argument errors that need no file and no device."""
    from dinox import ops
    if args.synthetic < 0 or (args.synthetic == 0) == (args.volume is None):
        ap.error("exactly one of --volume and --synthetic Z (Z >= 1) is needed")
    if args.synthetic and (args.labels is not None or args.seed_labels is not None):
        ap.error("--synthetic brings its own ground truth: --labels / --seed-labels do not apply")
    if args.volume is not None and args.spacing is None:
        ap.error("--volume needs --spacing")
    if args.spacing is not None and any(not 0.0 < s < float("inf") for s in args.spacing):
        ap.error(f"--spacing: three finite values > 0, got {args.spacing}")
    if not ops.LABELPROP_MIN_C <= args.num_classes <= ops.LABELPROP_MAX_C:
        ap.error(f"--num-classes: an integer in [{ops.LABELPROP_MIN_C}, {ops.LABELPROP_MAX_C}], got {args.num_classes}")
    if not 1 <= args.topk <= ops.KNN_MAX_K:
        ap.error(f"--topk: an integer in [1, {ops.KNN_MAX_K}], got {args.topk}")
    if args.context_frames < 0:
        ap.error(f"--context-frames: an integer >= 0, got {args.context_frames}")
    if not 0.0 < args.temperature < float("inf"):
        ap.error(f"--temperature: a finite value > 0, got {args.temperature}")
    if not 0.0 <= args.min_component_mm3 < float("inf"):
        ap.error(f"--min-component-mm3: a finite volume >= 0, got {args.min_component_mm3}")
    if args.batch_size < 1:
        ap.error(f"--batch-size: an integer >= 1, got {args.batch_size}")
    if not args.synthetic:
        if args.seed_slice is None and args.labels is None:
            ap.error("--seed-slice with --seed-labels (one-shot segmentation) or --labels (evaluation) is needed")
        if args.seed_slice is not None and args.seed_labels is None and args.labels is None:
            ap.error("--seed-slice needs --seed-labels (or --labels, whose seed slices are then used)")
        if args.seed_slice is None and args.seed_labels is not None:
            ap.error("--seed-labels needs --seed-slice")
    if args.report is not None and args.labels is None and not args.synthetic:
        ap.error("--report needs --labels or --synthetic")


def synthetic_case(Z: int, side: int, num_classes: int, seed: int = 0):
    """(volume float32 (Z, side, side) in HU, labels uint8 (Z, side, side)): on a dim noisy background one bright ellipse per class
    1 .. C - 1, each with its own brightness, drifting and shrinking slowly along z.  A function of its arguments alone."""
    rng = np.random.default_rng(seed)
    n = num_classes - 1
    ang = 2.0 * np.pi * (np.arange(n) + rng.uniform(0.0, 1.0)) / max(n, 1)
    cy0 = side * (0.5 + 0.24 * np.sin(ang))
    cx0 = side * (0.5 + 0.24 * np.cos(ang))
    ry0 = side * rng.uniform(0.10, 0.14, n)
    rx0 = side * rng.uniform(0.10, 0.14, n)
    drift = rng.uniform(-0.004, 0.004, (n, 2)) * side
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float64) + 0.5
    vol = (-120.0 + 15.0 * rng.standard_normal((Z, side, side))).astype(np.float32)
    lab = np.zeros((Z, side, side), dtype=np.uint8)
    for z in range(Z):
        shrink = 1.0 - 0.015 * z
        for c in range(n):
            inside = ((yy - cy0[c] - drift[c, 0] * z) / (ry0[c] * shrink)) ** 2 + ((xx - cx0[c] - drift[c, 1] * z) / (rx0[c] * shrink)) ** 2 <= 1.0
            lab[z][inside] = c + 1
            vol[z][inside] += 200.0 + 240.0 * (c + 1) / num_classes
    return vol, lab


def pick_seed(gt: np.ndarray) -> int:
    """Evaluation mode: the slice with the most foreground voxels (the lowest z on a tie)."""
    fg = ((gt != 0) & (gt != 255)).reshape(gt.shape[0], -1).sum(1)
    return int(np.argmax(fg))


def _floats(t) -> list:
    return [None if not np.isfinite(v) else float(v) for v in np.asarray(t, dtype=np.float64)]


def _mean_present(values) -> float | None:
    v = np.asarray(values, dtype=np.float64)
    v = v[np.isfinite(v)]
    return float(v.mean()) if len(v) else None


def score(pred: torch.Tensor, soft: torch.Tensor, gt: torch.Tensor, sel, patch: int, C: int, cleaned: bool) -> dict:
    """Per-class and mean (over the foreground classes present) Dice / IoU of the slices ``sel``: the counts of ``ops.seg_predict`` on the
    soft labels -- after a clean-up the same counts of the cleaned volume (``ops.cc_filter_3d`` with every class kept) -- through
    ``segment.CaseAccumulator``."""
    from dinox import ops, segment as SG
    sel = torch.as_tensor(sel, dtype=torch.long, device=pred.device)
    if cleaned:
        _, cnt = ops.cc_filter_3d(pred[sel].contiguous(), C, first_class=C, targets=gt[sel].contiguous())
    else:
        _, cnt = ops.seg_predict(soft[sel].contiguous(), patch, labels=gt[sel].contiguous())
    acc = SG.CaseAccumulator(C)
    acc.update(cnt, torch.zeros((C, 4), dtype=torch.int64))
    dice = acc.result()["dice"]
    present = (cnt[1] + cnt[2]).cpu() > 0
    iou = torch.where(present, SG.iou_per_class(cnt).cpu().double(), torch.full((C,), float("nan"), dtype=torch.float64))
    return {"slices": int(len(sel)), "dice": _floats(dice), "iou": _floats(iou), "mean_dice": _mean_present(dice[1:]), "mean_iou": _mean_present(iou[1:])}


def run(args: argparse.Namespace):
    ap = build_parser()
    check_args(ap, args)
    device = torch.device(args.device)
    if device.type != "cuda":
        raise SystemExit(f"this engine computes on MI355X only: --device {args.device} requested (no CPU compute path)")
    for f in (args.volume, args.labels, args.seed_labels):
        if f is not None and not Path(f).is_file():
            ap.error(f"{f}: no such file")
    if not torch.cuda.is_available():
        raise SystemExit("this engine computes on MI355X only: no CUDA/HIP device available")
    from dinox import propagate as PR, segment as SG
    from zoo.encode import encode_volume
    from zoo.hub import load_model
    model = load_model(args.checkpoint, device=device)
    S, patch, C = model.img_size, model.patch, args.num_classes
    g = S // patch

    gt = None
    if args.synthetic:
        vol, gt = synthetic_case(args.synthetic, S, C)
        spacing = tuple(args.spacing) if args.spacing else (1.0, 1.0, 1.0)
    else:
        vol = np.load(args.volume, allow_pickle=False)
        if vol.ndim != 3:
            ap.error(f"--volume {args.volume}: a (Z, H, W) array expected, got {vol.shape}")
        spacing = tuple(args.spacing)
    Z = vol.shape[0]

    def to_grid(arr, what):
        if arr.dtype != np.uint8 or arr.ndim != 3 or arr.shape[0] != Z:
            ap.error(f"{what}: uint8 ({Z}, H, W) expected, got {arr.dtype} {arr.shape}")
        return arr if arr.shape == (Z, S, S) else SG.resample_labels_nearest(arr, S)

    if args.labels is not None:
        gt = np.load(args.labels, allow_pickle=False)
    if gt is not None:
        gt = to_grid(gt, "--labels")
    seeds = sorted(set(args.seed_slice)) if args.seed_slice is not None else [pick_seed(gt)]
    if any(not 0 <= z < Z for z in seeds):
        ap.error(f"--seed-slice: indices in [0, {Z}), got {seeds}")
    if args.seed_labels is not None:
        sl = np.load(args.seed_labels, allow_pickle=False)
        if sl.ndim == 2:
            if len(seeds) != 1:
                ap.error(f"--seed-labels {args.seed_labels}: an (H, W) map serves one seed, got {len(seeds)} seeds")
            full = np.full((Z,) + sl.shape, 255, dtype=np.uint8)
            full[seeds[0]] = sl
            sl = full
        seed_grid = to_grid(sl, "--seed-labels")
    else:
        seed_grid = gt
    seed_maps = {z: torch.from_numpy(np.ascontiguousarray(seed_grid[z])).to(device) for z in seeds}

    t0 = time.perf_counter()
    amp = torch.autocast("cuda", dtype=torch.bfloat16) if args.amp else contextlib.nullcontext()
    with amp:
        feats = encode_volume(model, vol, spacing, batch_size=args.batch_size, return_all_tokens=True, device=device)
    tokens = feats[:, 1:1 + g * g].float().contiguous()                         # [CLS, patches, registers]: the patches
    res = PR.propagate_labels(tokens, seed_maps, C, patch=patch, n_context=args.context_frames, topk=args.topk, radius=args.radius,
                              temperature=args.temperature, return_trace=args.dump_trace is not None)
    soft, hard = res[0], res[1]
    cleaned = args.keep_largest or args.min_component_mm3 > 0
    if cleaned:
        voxel = (spacing[2], spacing[1] * vol.shape[1] / S, spacing[0] * vol.shape[2] / S)
        hard = SG.postprocess_volume(hard, C, voxel, keep_largest=args.keep_largest, min_volume_mm3=args.min_component_mm3,
                                     connectivity=args.connectivity)
    labels = hard.cpu().numpy()                                                 # (the copy waits for the device)
    seconds = time.perf_counter() - t0
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    np.save(args.out, labels)
    print(f"slices={Z} grid={g} seeds={seeds} seconds={seconds:.3f} -> {args.out}")

    if args.dump_trace is not None:
        F = 1 + args.context_frames
        tr = res[2]
        slots = np.full((len(tr), F), -1, dtype=np.int32)
        for i, t in enumerate(tr):
            slots[i, :len(t["slots"])] = t["slots"]
        shape = (0, g * g, args.topk)
        Path(args.dump_trace).parent.mkdir(parents=True, exist_ok=True)
        np.savez(args.dump_trace, z=np.array([t["z"] for t in tr], dtype=np.int32), seed=np.array([t["seed"] for t in tr], dtype=np.int32), slots=slots,
                 idx=np.stack([t["idx"].cpu().numpy() for t in tr]) if tr else np.zeros(shape, np.int32),
                 val=np.stack([t["val"].cpu().numpy() for t in tr]) if tr else np.zeros(shape, np.float32))

    report = None
    if gt is not None:
        source, _ = PR.context_schedule(Z, seeds, args.context_frames)
        gt_d = torch.from_numpy(gt).to(device)
        rest = sorted(source)
        params = {"topk": args.topk, "context_frames": args.context_frames, "radius": args.radius, "temperature": args.temperature,
                  "amp": bool(args.amp), "keep_largest": bool(args.keep_largest), "min_component_mm3": float(args.min_component_mm3),
                  "connectivity": args.connectivity}
        report = {"checkpoint": str(args.checkpoint), "volume": f"synthetic:{Z}" if args.synthetic else str(args.volume), "slices": Z, "grid": g,
                  "num_classes": C, "seeds": seeds, "params": params, "per_class": None, "mean": None, "by_distance": {}, "seconds": seconds}
        if rest:
            sc = score(hard, soft, gt_d, rest, patch, C, cleaned)
            report["per_class"] = {"dice": sc["dice"], "iou": sc["iou"]}
            report["mean"] = {"dice": sc["mean_dice"], "iou": sc["mean_iou"]}
            for d in sorted({abs(z - s) for z, s in source.items()}):
                report["by_distance"][str(d)] = score(hard, soft, gt_d, [z for z in rest if abs(z - source[z]) == d], patch, C, cleaned)
            print(f"non-seed slices={len(rest)} mean_dice={report['mean']['dice']} mean_iou={report['mean']['iou']}")
        assert tuple(report) == REPORT_KEYS
        if args.report is not None:
            Path(args.report).parent.mkdir(parents=True, exist_ok=True)
            Path(args.report).write_text(json.dumps(report, indent=2))
    print("ok=true")
    return report


def main(argv=None):
    return run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
