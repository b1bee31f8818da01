#!/usr/bin/env python3
"""Segment whole CT series with a fine-tuned segmenter, clean the result by 3-D connected components and score it per case.

    python scripts/segment_volume.py --backbone runs/x/hub-export/ --segmenter seg/x/ --volume series.npy --spacing 0.8 0.8 2.5 --out labels.npy
    python scripts/segment_volume.py --backbone B --segmenter S --volume a.npy --labels a_gt.npy --volume b.npy --labels b_gt.npy \\
        --spacing 0.8 0.8 2.5 --keep-largest --min-component-mm3 50 --out labels.npy --report cases.json

``--volume`` is a .npy file holding a (Z, H, W) series; the label volume written to ``--out`` is uint8 (Z, S, S) on the model's grid
(dinox.segment.segment_volume: one trip to the device, chunks of ``--batch-size`` slices).  With several ``--volume`` the outputs are
``--out`` with ``_0``, ``_1``, ... before the suffix.  ``--keep-largest`` / ``--min-component-mm3 V`` clean every class >= 1 by 3-D components
(csrc/cclabel3d.hip; ``--connectivity`` 6, 18 or 26; the voxel is that of the label grid, see segment_volume).

``--labels`` (one per ``--volume``, in order) holds the ground truth, uint8 with 255 = ignore: (Z, S, S) is taken as is, (Z, H, W) of the
series is resampled to the grid by dinox.segment.resample_labels_nearest.  ``--report`` then gets, per class, the mean over cases of the
per-case Dice and the lesion-wise sensitivity, precision, F1 and false positives per case (dinox.segment.CaseAccumulator); a lesion is a
3-D component of at least ``--min-component-mm3``, hit when at least ``--lesion-overlap`` of it (to 1/1000; 0: any voxel) is matched.

``--tolerance-mm T`` (repeatable, needs ``--labels``) adds the volumetric boundary metrics of every case: the cleaned prediction (what
``--out`` holds) against the ground truth through ops.surface_stats_3d (csrc/surfdist3d.hip), with the voxel (s_z, s_y, s_x) of the label
grid, so the slice spacing enters every distance.  The report then also holds, per class, the mean over cases of HD95 and ASSD in mm and
of the surface Dice (NSD) at every tolerance, with the number of cases behind them; ``--surface-quantile NUM DEN`` replaces the 95/100 of
HD95 (nearest rank).  A class in only one of the two volumes of a case scores the volume diagonal and NSD 0 there.

``--tiled`` predicts by sliding window at the series' own resolution instead (dinox.segment.segment_volume_tiled, csrc/segblend.hip):
tiles of side ``--tile N`` (default: the model's input size, clamped to the plane) overlapping by ``--overlap F``, their logits blended
under ``--blend-window`` (gaussian or constant), with ``--tta-flips`` averaged over the four mirror variants.  ``--out`` then holds
uint8 (Z, H, W), ``--labels`` must be (Z, H, W) and is compared as it is (nothing is resampled), and ``--min-component-mm3`` and
``--tolerance-mm`` use the scanner's voxel (SZ, SY, SX).  The report records the tile geometry and the grid of the scores; a metric whose
kernel declines the native size is reported with the kernel's message instead of a value.

``--refine`` refines every slice's label map before the clean-up (dinox.segment.segment_volume(refine=...), csrc/segrefine.hip): mean-field
iterations of a local CRF guided by the slice's own normalised plane, at the stored temperature.  ``--refine-iters``, ``--refine-radius``,
``--refine-dilation``, ``--refine-sigma-xy``, ``--refine-sigma-i``, ``--refine-mix`` and ``--refine-weight`` replace single parameters
(default: what the segmenter stores, else RefineConfig's defaults, untuned on real data).  ``--confidence-out`` then holds the refined
confidence.  Not with ``--tiled`` (the blend kernel never materialises the blended logits) and not with ``--entropy-out``.
"""
from __future__ import annotations

import argparse
import json
import logging
import sys
from pathlib import Path

import numpy as np
import torch

_HERE = Path(__file__).resolve().parent
for _p in (_HERE.parent, _HERE):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import finetune_lora as fl  # noqa: E402
from evaluate_segmentation import _floats, _mean_present, add_refine_flags, check_refine_flags, refine_config  # noqa: E402,F401
from dinox import ops, segment as SG  # noqa: E402

log = logging.getLogger("segment_volume")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Label volumes of whole series, 3-D clean-up and per-case scores",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    base = {a.dest: a for a in fl.build_parser()._actions}
    ap._add_action(base["backbone"])
    ap.add_argument("--segmenter", required=True, type=Path, metavar="DIR", help="output directory of finetune_segmentation.py")
    ap._add_action(base["device"])
    ap.add_argument("--volume", required=True, type=Path, action="append", help=".npy file holding a (Z, H, W) series; repeatable")
    ap.add_argument("--spacing", type=float, nargs=3, required=True, metavar=("SX", "SY", "SZ"),
                    help="mm per source pixel in x and y and the slice spacing, for every --volume")
    ap.add_argument("--out", required=True, type=Path, help="output .npy: uint8 (Z, S, S); with --tiled (Z, H, W)")
    for dest in ("input_format", "window_level", "window_width"):
        ap._add_action(base[dest])
    ap.add_argument("--context", default="neighbours", choices=("neighbours", "replicate"), help="the 2.5D stack of a slice")
    ap.add_argument("--batch-size", type=int, default=64, help="slices per forward")
    ap._add_action(base["no_amp"])
    ap.add_argument("--keep-largest", action="store_true", help="keep only the largest 3-D component of every class >= 1")
    ap.add_argument("--min-component-mm3", type=float, default=0.0, metavar="V",
                    help="remove the 3-D components of the classes >= 1 under V mm^3; with --labels also the smallest component that counts as a lesion")
    ap.add_argument("--connectivity", type=int, choices=(6, 18, 26), default=26, help="neighbourhood of a 3-D connected component")
    ap.add_argument("--labels", type=Path, action="append", default=None, help=".npy ground truth of the --volume in the same position; repeatable")
    ap.add_argument("--lesion-overlap", type=float, default=0.0, metavar="F",
                    help="a lesion is hit when at least this fraction of it is matched (taken to 1/1000; 0: any overlap)")
    ap.add_argument("--report", type=Path, default=None, help="JSON of the per-case scores (needs --labels)")
    ap.add_argument("--tolerance-mm", type=float, action="append", default=None, metavar="T",
                    help="also score HD95, ASSD and the surface Dice at this tolerance in 3-D, per case; repeatable (needs --labels)")
    ap.add_argument("--surface-quantile", type=int, nargs=2, default=[95, 100], metavar=("NUM", "DEN"),
                    help="the nearest-rank quantile reported as hd95_mm")
    ap.add_argument("--tiled", action="store_true", help="sliding-window prediction on the series' own (Z, H, W) grid")
    ap.add_argument("--tile", type=int, default=argparse.SUPPRESS, metavar="N",
                    help="tile side in source pixels (needs --tiled; default: the model's input size, clamped to the plane)")
    ap.add_argument("--overlap", type=float, default=argparse.SUPPRESS, metavar="F", help="overlap of neighbouring tiles, 0 <= F < 1 (needs --tiled; default: 0.5)")
    ap.add_argument("--blend-window", choices=("gaussian", "constant"), default=argparse.SUPPRESS,
                    help="weights of a tile's pixels in the blend (needs --tiled; default: gaussian)")
    ap.add_argument("--tta-flips", action="store_true", help="average the four mirror variants of every tile (needs --tiled)")
    ap.add_argument("--confidence-out", type=Path, default=None, metavar="NPY",
                    help="also write the fp32 confidence volume (the winning class's softmax probability at the segmenter's stored "
                         "temperature), on the grid of --out.  With --tiled it is the blend kernel's max-softmax; a stored temperature "
                         "T != 1 then divides the tile logits by T before the blend, and the labels are that launch's: they may differ "
                         "from a run without this flag at exact fp32 near-ties (with T = 1 nothing changes)")
    ap.add_argument("--entropy-out", type=Path, default=None, metavar="NPY",
                    help="also write the fp32 volume of the softmax entropy / log C at the stored temperature (not with --tiled: the blend "
                         "kernel has no entropy output)")
    add_refine_flags(ap)
    return ap


TILED_DEFAULTS = {"tile": None, "overlap": 0.5, "blend_window": "gaussian"}


def check_args(ap: argparse.ArgumentParser, args: argparse.Namespace) -> None:
    """The argument errors that need no file and no device; fills in the defaults of the --tiled options."""
    given = [f"--{k.replace('_', '-')}" for k in TILED_DEFAULTS if hasattr(args, k)] + (["--tta-flips"] if args.tta_flips else [])
    if given and not args.tiled:
        ap.error(f"{', '.join(given)}: only with --tiled")
    if args.entropy_out is not None and args.tiled:
        ap.error("--entropy-out: not with --tiled (the blend kernel has no entropy output)")
    if args.refine and args.tiled:
        ap.error("--refine: not with --tiled (the sliding-window path never materialises the blended logits the refinement starts from)")
    if args.refine and args.entropy_out is not None:
        ap.error("--entropy-out: not with --refine (the refinement kernel has no entropy output)")
    check_refine_flags(ap, args)
    for k, v in TILED_DEFAULTS.items():
        if not hasattr(args, k):
            setattr(args, k, v)
    if args.tile is not None and args.tile < 1:
        ap.error(f"--tile: an integer >= 1, got {args.tile}")
    if not 0.0 <= args.overlap < 1.0:
        ap.error(f"--overlap: a fraction in [0, 1), got {args.overlap}")
    if not 0.0 <= args.min_component_mm3 < float("inf"):
        ap.error(f"--min-component-mm3: a finite volume >= 0, got {args.min_component_mm3}")
    if not 0.0 <= args.lesion_overlap <= 1.0:
        ap.error(f"--lesion-overlap: a fraction in [0, 1], got {args.lesion_overlap}")
    if args.labels is not None and len(args.labels) != len(args.volume):
        ap.error(f"--labels: one per --volume, got {len(args.labels)} for {len(args.volume)} volume(s)")
    if args.report is not None and args.labels is None:
        ap.error("--report needs --labels")
    if args.tolerance_mm is not None:
        if args.labels is None:
            ap.error("--tolerance-mm needs --labels")
        if len(args.tolerance_mm) > ops.SURFACE_MAX_TOLERANCES or any(not 0.0 <= t < float("inf") for t in args.tolerance_mm):
            ap.error(f"--tolerance-mm: 1 to {ops.SURFACE_MAX_TOLERANCES} finite values >= 0, got {args.tolerance_mm}")
    if not 0 < args.surface_quantile[0] <= args.surface_quantile[1]:
        ap.error(f"--surface-quantile: two integers with 0 < NUM <= DEN, got {args.surface_quantile}")
    if args.batch_size < 1:
        ap.error(f"--batch-size: an integer >= 1, got {args.batch_size}")
    if any(not 0.0 < s < float("inf") for s in args.spacing):
        ap.error(f"--spacing: three finite values > 0, got {args.spacing}")


def grid_labels(ap: argparse.ArgumentParser, path: Path, vol_shape, S: int) -> np.ndarray:
    """The ground truth of one case on the (Z, S, S) grid."""
    gt = np.load(path)
    Z = vol_shape[0]
    if gt.dtype != np.uint8 or gt.ndim != 3:
        ap.error(f"--labels {path}: uint8 (Z, H, W) or (Z, S, S) expected, got {gt.dtype} {gt.shape}")
    if gt.shape == (Z, S, S):
        return gt
    if gt.shape == tuple(vol_shape):
        return SG.resample_labels_nearest(gt, S)
    ap.error(f"--labels {path}: shape {gt.shape} is neither the series' {tuple(vol_shape)} nor the label grid's {(Z, S, S)}")


def native_labels(ap: argparse.ArgumentParser, path: Path, vol_shape) -> np.ndarray:
    """The ground truth of one case under --tiled: on the series' own grid, taken as it is."""
    gt = np.load(path)
    if gt.dtype != np.uint8 or gt.shape != tuple(vol_shape):
        ap.error(f"--labels {path}: with --tiled uint8 {tuple(vol_shape)} (the series' own grid) is expected, got {gt.dtype} {gt.shape}")
    return gt


def case_report(res: dict, args: argparse.Namespace, overlap) -> dict:
    """The report of CaseAccumulator.result(); the means run over the foreground classes (>= 1) that have a value."""
    les = res["lesions"]
    scores = ("sensitivity", "precision", "f1")
    per_class = {"dice": _floats(res["dice"]), "dice_cases": res["cases"].tolist(), "fp_per_case": _floats(les["fp_per_image"])}
    per_class.update({k: _floats(les[k]) for k in scores})
    per_class.update({k: les[k].tolist() for k in SG.LESION_COUNTS})
    mean = {"dice": _mean_present(res["dice"][1:]), "fp_per_case": _mean_present(les["fp_per_image"][1:])}
    mean.update({k: _mean_present(les[k][1:]) for k in scores})
    return {"cases": les["images"], "connectivity": args.connectivity, "overlap": f"{overlap[0]}/{overlap[1]}",
            "min_volume_mm3": float(args.min_component_mm3), "keep_largest": bool(args.keep_largest), "per_class": per_class, "mean": mean}


def add_surface_report(report: dict, res: dict, args: argparse.Namespace) -> None:
    """The volumetric boundary metrics of SurfaceAccumulator.result() (one case = one image) into the report."""
    tol = list(args.tolerance_mm)
    report["tolerances_mm"] = tol
    report["quantile"] = f"{args.surface_quantile[0]}/{args.surface_quantile[1]} (nearest rank)"
    report["spacing"] = "distances in mm with the label grid's voxel (s_z, s_y, s_x) = (SZ, SY H / S, SX W / S) of every case"
    report["per_class"].update({"hd95_mm": _floats(res["hd95"]), "assd_mm": _floats(res["assd"]),
                                "nsd": {f"{t:g}": _floats(res["nsd"][:, i]) for i, t in enumerate(tol)}, "surface_cases": res["images"].tolist()})
    report["mean"].update({"hd95_mm": _mean_present(res["hd95"][1:]), "assd_mm": _mean_present(res["assd"][1:]),
                           "nsd": {f"{t:g}": _mean_present(res["nsd"][1:, i]) for i, t in enumerate(tol)}})


def score_tiled_case(ap, args, i: int, vol_shape, pred: np.ndarray, C: int, overlap, acc, surf, declined: dict, device) -> None:
    """One case under --tiled: prediction and ground truth on the series' own grid, the real voxel.  A metric kernel that declines the
    native size leaves its message in ``declined`` for the report; nothing is resampled to make it fit."""
    sx, sy, sz = args.spacing
    gt = torch.from_numpy(native_labels(ap, args.labels[i], vol_shape)).to(device)
    p = torch.from_numpy(pred).to(device)
    voxel = (sz, sy, sx)
    try:
        mv = SG.min_component_vox(args.min_component_mm3, voxel)
        _, cnt = ops.cc_filter_3d(p, C, first_class=C, connectivity=args.connectivity, targets=gt)      # first_class = C: keeps all, counts only
        acc.update(cnt, ops.lesion_counts_3d(p, gt, C, connectivity=args.connectivity, overlap=overlap, min_vox=mv))
    except (ValueError, RuntimeError) as e:
        declined.setdefault("dice_and_lesions", {})[str(i)] = str(e)
    if surf is not None:
        try:
            sc, sv = ops.surface_stats_3d(p, gt, voxel, C, tolerances=args.tolerance_mm, q=tuple(args.surface_quantile))
            surf.update(SG.surface_metrics_3d(sc, sv, voxel, tuple(p.shape)))
        except (ValueError, RuntimeError) as e:
            declined.setdefault("surface", {})[str(i)] = str(e)


def run(args: argparse.Namespace):
    ap = build_parser()
    check_args(ap, args)
    device = torch.device(args.device)
    if device.type != "cuda":
        raise SystemExit(f"this engine computes on MI355X only: --device {args.device} requested (no CPU compute path)")
    for f in list(args.volume) + list(args.labels or []):
        if not Path(f).is_file():
            ap.error(f"{f}: no such file")
    if not torch.cuda.is_available():
        raise SystemExit("this engine computes on MI355X only: no CUDA/HIP device available")
    refine = None
    if args.refine:                                 # the stored parameters with the flags in place; a bad value is an argument error
        cfg_file = Path(args.segmenter) / SG.CONFIG_FILE
        refine = refine_config(args, json.loads(cfg_file.read_text()).get("refine") if cfg_file.is_file() else None, ap)
    model = SG.load_segmenter(args.backbone, args.segmenter, device)
    C, S = model.head.num_classes, model.img_size
    overlap = (round(1000 * args.lesion_overlap), 1000)
    acc = SG.CaseAccumulator(C) if args.labels else None
    surf = SG.SurfaceAccumulator(C, len(args.tolerance_mm)) if args.tolerance_mm else None
    sx, sy, sz = args.spacing
    want_conf, want_ent = args.confidence_out is not None, args.entropy_out is not None
    declined, grids = {}, []                        # --tiled: metric -> {case: the kernel's message}; the tile grid of every case
    for i, vpath in enumerate(args.volume):
        vol = np.load(vpath)
        if vol.ndim != 3:
            ap.error(f"--volume {vpath}: a (Z, H, W) array expected, got {vol.shape}")
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=not args.no_amp):
            if args.tiled:
                plan = SG.tile_plan(model, vol.shape[1], vol.shape[2], args.tile, args.overlap, args.blend_window, args.tta_flips)
                grids.append({"shape": list(vol.shape), "tile": plan["tile"], "ys": plan["ys"], "xs": plan["xs"]})
                pred = SG.segment_volume_tiled(model, vol, (sx, sy, sz), tile=args.tile, overlap=args.overlap, window=args.blend_window,
                                               tta_flips=args.tta_flips, input_format=args.input_format, hu_level=args.window_level,
                                               hu_width=args.window_width, context=args.context, batch_size=args.batch_size, device=device,
                                               keep_largest=args.keep_largest, min_volume_mm3=args.min_component_mm3,
                                               connectivity=args.connectivity, return_confidence=want_conf)
            else:
                pred = SG.segment_volume(model, vol, (sx, sy, sz), input_format=args.input_format, hu_level=args.window_level,
                                         hu_width=args.window_width, context=args.context, batch_size=args.batch_size, device=device,
                                         keep_largest=args.keep_largest, min_volume_mm3=args.min_component_mm3,
                                         connectivity=args.connectivity, return_confidence=want_conf, return_entropy=want_ent,
                                         refine=refine)
        if want_conf or want_ent:                   # (labels, conf[, entropy])
            pred, maps = pred[0], dict(zip([p for p, w in ((args.confidence_out, want_conf), (args.entropy_out, want_ent)) if w], pred[1:]))
            for mpath, arr in maps.items():
                mout = mpath if len(args.volume) == 1 else mpath.with_name(f"{mpath.stem}_{i}{mpath.suffix}")
                Path(mout).parent.mkdir(parents=True, exist_ok=True)
                np.save(mout, arr)
        out = args.out if len(args.volume) == 1 else args.out.with_name(f"{args.out.stem}_{i}{args.out.suffix}")
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        np.save(out, pred)
        log.info("%s: %s -> %s", vpath, tuple(vol.shape), out)
        if acc is None:
            continue
        if args.tiled:
            score_tiled_case(ap, args, i, vol.shape, pred, C, overlap, acc, surf, declined, device)
            continue
        gt = torch.from_numpy(grid_labels(ap, args.labels[i], vol.shape, S)).to(device)
        p = torch.from_numpy(pred).to(device)
        voxel = (sz, sy * vol.shape[1] / S, sx * vol.shape[2] / S)
        mv = SG.min_component_vox(args.min_component_mm3, voxel)
        _, cnt = ops.cc_filter_3d(p, C, first_class=C, connectivity=args.connectivity, targets=gt)      # first_class = C: keeps all, counts only
        acc.update(cnt, ops.lesion_counts_3d(p, gt, C, connectivity=args.connectivity, overlap=overlap, min_vox=mv))
        if surf is not None:
            sc, sv = ops.surface_stats_3d(p, gt, voxel, C, tolerances=args.tolerance_mm, q=tuple(args.surface_quantile))
            surf.update(SG.surface_metrics_3d(sc, sv, voxel, tuple(p.shape)))
    if acc is None:
        return None
    report = case_report(acc.result(), args, overlap)
    if surf is not None:
        add_surface_report(report, surf.result(), args)
    if args.tiled:
        report["tiled"] = {"tile": grids[0]["tile"] if len({g["tile"] for g in grids}) == 1 else [g["tile"] for g in grids],
                           "overlap": args.overlap, "window": args.blend_window, "flips": [0, 1, 2, 3] if args.tta_flips else [0],
                           "tile_grid": grids, "score_grid": "native: the (Z, H, W) grid of every series, voxel (s_z, s_y, s_x) = (SZ, SY, SX) mm",
                           "declined": declined}
        if surf is not None:
            report["spacing"] = "distances in mm with the series' own voxel (s_z, s_y, s_x) = (SZ, SY, SX)"
    report["segmenter"], report["backbone"] = str(args.segmenter), str(args.backbone)
    if args.report is not None:
        Path(args.report).parent.mkdir(parents=True, exist_ok=True)
        Path(args.report).write_text(json.dumps(report, indent=2))
    log.info("%d case(s): mean Dice %s, sensitivity %s, false positives per case %s", report["cases"], report["mean"]["dice"],
             report["mean"]["sensitivity"], report["mean"]["fp_per_case"])
    return report


def main(argv=None):
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)s] %(message)s", datefmt="%H:%M:%S")
    return run(args)


if __name__ == "__main__":
    main()
