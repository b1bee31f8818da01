#!/usr/bin/env python3
"""Evaluate a fine-tuned segmenter: overlap scores and boundary metrics in millimetres, all of it on the device.

    python scripts/evaluate_segmentation.py --backbone runs/x/hub-export/ --segmenter seg/x/ --val-csv val.csv --out seg_eval.json
    python scripts/evaluate_segmentation.py --backbone runs/x/hub-export/ --segmenter /tmp/s --synthetic 48 --out /tmp/s/seg_eval.json

``--segmenter`` is the directory scripts/finetune_segmentation.py wrote (dinox.segment.load_segmenter puts it back together); the CSV has
that script's columns: image_path,mask_path[,spacing_x,spacing_y,spacing_z].  Per class and as means over the present classes the JSON
holds Dice and IoU (ops.seg_predict's counts over the whole set) and HD95, ASSD and the surface Dice (NSD) at every ``--tolerance-mm``
(ops.surface_stats, csrc/surfdist.hip; dinox.segment.surface_metrics), each with the number of images behind it.

Spacing.  The boundary metrics are measured on the grid the model predicts on: the centre crop resizes an h x w slice to nh x nw before
cropping, so a pixel of the label map is (spacing_y h / nh, spacing_x w / nw) mm, not the CSV's value; ``--synthetic`` maps are never
resized and keep their own spacings.  The backbone still sees the CSV's spacing, as in training.
Per image a class absent from both maps is left out; one present in exactly one of them scores the image diagonal (HD95, ASSD) and 0 (NSD).

Components (csrc/cclabel.hip; all opt-in, without these flags the report is what it was).  ``--keep-largest`` / ``--min-component-mm2 A``
clean the predicted map first (dinox.segment.postprocess's rule, the area on the evaluated grid's spacing); every score of the report is
then taken on the cleaned map and a "postprocess" object records the settings.  ``--lesion-metrics`` adds a "lesion" object: per class and
as means over the foreground classes that have a value, lesion-wise sensitivity, precision, F1 and false positives per image, with the
summed counts; a lesion is a connected component (``--connectivity``) of at least ``--min-component-mm2``, hit when at least
``--lesion-overlap`` of it (to 1/1000; 0: any pixel) is matched by the other map.

``--refine`` (csrc/segrefine.hip, dinox.segment.RefineConfig; opt-in) refines the arg-max by mean-field iterations of a local CRF guided
by the slice the backbone sees (channel 1 of its normalised input), at the stored temperature and before any clean-up.  Every score of
the report is then taken on the refined map, and a "refine" object holds the parameters and the Dice and surface scores of the unrefined
map next to the refined ones, so one run shows the effect (both sides of the pair are taken before ``--keep-largest`` /
``--min-component-mm2``, so that it isolates the refinement; the report's own scores include the clean-up).  ``--refine-iters``, ``--refine-radius``, ``--refine-dilation``,
``--refine-sigma-xy``, ``--refine-sigma-i``, ``--refine-mix`` and ``--refine-weight`` replace single parameters (default: what the segmenter
stores, else RefineConfig's defaults, which are untuned on real data); ``--write-refine`` stores the parameters used in the segmenter's
finetune_config.json, as ``--write-temperature`` does for the temperature.
"""
from __future__ import annotations

import argparse
import json
import logging
import sys
from pathlib import Path

import torch

_HERE = Path(__file__).resolve().parent
for _p in (_HERE.parent, _HERE):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import finetune_lora as fl  # noqa: E402
import finetune_segmentation as fs  # noqa: E402
from dinox import ops, segment as SG  # noqa: E402

log = logging.getLogger("evaluate_segmentation")

SPACING_CONVENTION = ("mm per pixel of the evaluated label map as (s_y, s_x): the CSV's (spacing_y h / nh, spacing_x w / nw) for an h x w "
                      "slice resized to nh x nw before the centre crop; --synthetic maps keep their own (spacing_y, spacing_x)")


def resize_factors(h: int, w: int, size: int):
    """(h / nh, w / nw) of finetune_segmentation._center_pair: the shorter side goes to ``size``, neither side below it."""
    k = size / min(h, w)
    return h / max(size, round(h * k)), w / max(size, round(w * k))


class EvalImages(fs.MaskedImages):
    """MaskedImages (centre crop) that also returns the spacing of the evaluated grid, (s_y, s_x) in mm per label-map pixel."""

    def __getitem__(self, i: int):
        row = self.rows[i]
        px, m = self.pixels(row), self.read_mask(row)
        x, m = fs.paired_transform(px[None].expand(3, -1, -1), m, self.img_size, self.gen, False)
        fy, fx = resize_factors(px.shape[-2], px.shape[-1], self.img_size)
        return x, torch.tensor(row.spacing, dtype=torch.float32), m, torch.tensor([row.spacing[1] * fy, row.spacing[0] * fx], dtype=torch.float32)


class EvalSynthetic(fs.SyntheticMasks):
    """SyntheticMasks with the (s_y, s_x) of its own spacings: the maps are generated at the evaluated size."""

    def __getitem__(self, i: int):
        x, sp, m = super().__getitem__(i)
        return x, sp, m, torch.stack([sp[1], sp[0]])


REFINE_FIELDS = (("iters", int), ("radius", int), ("dilation", int), ("sigma_xy", float), ("sigma_i", float), ("mix", float), ("weight", float))


def add_refine_flags(ap: argparse.ArgumentParser) -> None:
    """--refine and one flag per field of dinox.segment.RefineConfig (shared with scripts/segment_volume.py)."""
    ap.add_argument("--refine", action="store_true",
                    help="refine the label map by mean-field iterations of a local CRF guided by the image (csrc/segrefine.hip), before any clean-up")
    for name, kind in REFINE_FIELDS:
        ap.add_argument(f"--refine-{name.replace('_', '-')}", type=kind, default=argparse.SUPPRESS, metavar="V",
                        help=f"RefineConfig.{name} (needs --refine; default: the segmenter's stored value, else {getattr(SG.RefineConfig(), name)})")


def check_refine_flags(ap: argparse.ArgumentParser, args: argparse.Namespace) -> None:
    given = {name: getattr(args, f"refine_{name}") for name, _ in REFINE_FIELDS if hasattr(args, f"refine_{name}")}
    if given and not args.refine:
        ap.error(f"{', '.join('--refine-' + k.replace('_', '-') for k in given)}: only with --refine")
    try:
        SG.RefineConfig(**given)
    except ValueError as e:
        ap.error(str(e))


def refine_config(args: argparse.Namespace, stored, ap: argparse.ArgumentParser = None):
    """None without --refine; else the stored parameters (a RefineConfig, a dict as finetune_config.json holds it, or None for the
    defaults) with the given --refine-* flags in place.  A value that RefineConfig refuses is an argument error where ``ap`` is given."""
    if not args.refine:
        return None
    try:
        base = SG.RefineConfig.from_dict(stored).to_dict() if isinstance(stored, dict) else (stored or SG.RefineConfig()).to_dict()
        base.update({name: getattr(args, f"refine_{name}") for name, _ in REFINE_FIELDS if hasattr(args, f"refine_{name}")})
        return SG.RefineConfig(**base)
    except ValueError as e:
        if ap is None:
            raise
        ap.error(f"--refine: {e}")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Dice / IoU and HD95 / ASSD / surface Dice in mm of a fine-tuned segmenter",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    base = {a.dest: a for a in fl.build_parser()._actions}
    ap._add_action(base["backbone"])
    ap.add_argument("--segmenter", required=True, type=Path, metavar="DIR", help="output directory of finetune_segmentation.py")
    ap._add_action(base["device"])
    ap.add_argument("--val-csv", type=Path, default=None, help="required unless --synthetic")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="the validation quarter of finetune_segmentation.py --synthetic N")
    for dest in ("data_root", "input_format", "window_level", "window_width", "batch_size", "num_workers", "no_amp"):
        ap._add_action(base[dest])
    ap.add_argument("--seed", type=int, default=0, help="seed of the --synthetic set (the fine-tuning run's --seed)")
    ap.add_argument("--tolerance-mm", type=float, action="append", default=None, metavar="MM",
                    help="surface Dice tolerance in mm; repeatable (default: 1.0 and 2.0)")
    ap.add_argument("--out", type=Path, default=Path("seg_eval.json"))
    ap.add_argument("--lesion-metrics", action="store_true",
                    help="add lesion-wise sensitivity, precision, F1 and false positives per image (connected components, csrc/cclabel.hip)")
    ap.add_argument("--lesion-overlap", type=float, default=0.0, metavar="F",
                    help="a lesion is hit when at least this fraction of it is matched (taken to 1/1000; 0: any overlap)")
    ap.add_argument("--connectivity", type=int, choices=(4, 8), default=8, help="neighbourhood of a connected component")
    ap.add_argument("--keep-largest", action="store_true", help="score the map with only the largest component of every class >= 1 kept")
    ap.add_argument("--min-component-mm2", type=float, default=0.0, metavar="A",
                    help="score the map with the components of the classes >= 1 under A mm^2 removed; with --lesion-metrics also the "
                         "smallest ground-truth component that counts as a lesion")
    ap.add_argument("--calibration", action="store_true",
                    help="add a \"calibration\" object: reliability bins, ECE, MCE, NLL, Brier score and mean entropy of the upsampled softmax "
                         "(csrc/segcalib.hip).  It describes the RAW arg-max: --keep-largest and --min-component-mm2 do not affect it")
    ap.add_argument("--calibration-bins", type=int, default=15, metavar="NB", help="equal-width confidence bins of the reliability diagram")
    ap.add_argument("--temperature", type=float, default=None, metavar="T",
                    help="softmax temperature of the calibration scores (default: the one stored with the segmenter, else 1)")
    ap.add_argument("--fit-temperature", action="store_true",
                    help="fit the temperature that minimises the NLL of this set (its patch logits and labels are kept on the device) and "
                         "report the calibration before and after; implies --calibration")
    ap.add_argument("--write-temperature", action="store_true",
                    help="with --fit-temperature: store the fitted temperature in the segmenter's finetune_config.json")
    ap.add_argument("--calibration-cache-gib", type=float, default=4.0, metavar="G",
                    help="--fit-temperature is refused when the cached logits and labels would exceed this many GiB of device memory")
    add_refine_flags(ap)
    ap.add_argument("--write-refine", action="store_true",
                    help="with --refine: store the parameters used in the segmenter's finetune_config.json")
    return ap


def check_args(ap: argparse.ArgumentParser, args: argparse.Namespace) -> None:
    """What can be refused from the arguments alone (ap.error: exit status 2)."""
    if args.write_temperature and not args.fit_temperature:
        ap.error("--write-temperature needs --fit-temperature")
    if not 1 <= args.calibration_bins <= ops.SEG_CALIB_MAX_BINS:
        ap.error(f"--calibration-bins: an integer in [1, {ops.SEG_CALIB_MAX_BINS}], got {args.calibration_bins}")
    if args.temperature is not None and not 0.0 < args.temperature < float("inf"):
        ap.error(f"--temperature: a finite value > 0, got {args.temperature}")
    if not 0.0 < args.calibration_cache_gib < float("inf"):
        ap.error(f"--calibration-cache-gib: a finite value > 0, got {args.calibration_cache_gib}")
    if args.write_refine and not args.refine:
        ap.error("--write-refine needs --refine")
    check_refine_flags(ap, args)


def calibration_object(rep: dict, temperature: float, bins: int) -> dict:
    """The "calibration" object of the report: calibration_report's fields, the temperature used and the bin count."""
    return dict(rep, temperature=temperature, num_bins=bins)


def _floats(t: torch.Tensor):
    """Nested lists with None for NaN (JSON has no NaN)."""
    return [_floats(v) for v in t] if t.dim() else (None if bool(torch.isnan(t)) else float(t))


def _mean_present(t: torch.Tensor):
    keep = ~torch.isnan(t)
    return float(t[keep].mean()) if bool(keep.any()) else None


def lesion_report(res: dict, connectivity: int, overlap, min_area_mm2: float) -> dict:
    """The "lesion" object of the report from LesionAccumulator.result(); the means run over the foreground classes (>= 1) that have a
    value (a class with no ground-truth lesion has no sensitivity, one never predicted no precision)."""
    scores = ("sensitivity", "precision", "f1", "fp_per_image")
    per_class = {k: _floats(res[k]) for k in scores}
    per_class.update({k: res[k].tolist() for k in SG.LESION_COUNTS})
    mean = {k: _mean_present(res[k][1:]) for k in scores}
    mean["classes"] = int((~torch.isnan(res["f1"][1:])).sum())
    return {"connectivity": connectivity, "overlap": f"{overlap[0]}/{overlap[1]}", "min_area_mm2": min_area_mm2, "images": res["images"],
            "per_class": per_class, "mean": mean}


@torch.no_grad()
def evaluate(model: SG.SegModel, loader, device, amp: bool, tolerances, num_classes: int, *, lesion=None, post=None, calibration=None,
             cache=None, refine=None) -> dict:
    """One pass: the [3, C] overlap counts of the whole set and the per-class surface means.  -> the report dict (no file is written).
    ``post``: None or {"keep_largest", "min_area_mm2", "connectivity"} -- every score is then taken on the cleaned map (ops.cc_filter; the
    area on the evaluated grid's spacing).  ``lesion``: None or {"connectivity", "overlap": (num, den), "min_area_mm2"} -- adds "lesion".
    ``calibration``: None or {"bins", "temperature"} -- adds "calibration", from one ops.seg_calib launch per batch beside the prediction
    (always of the raw arg-max, whatever ``post`` says).  ``cache``: a list that receives every batch's (patch logits, labels).
    ``refine``: None or a RefineConfig -- the map is ops.seg_refine's (guide: channel 1 of x, at 1 / model.temperature) before ``post``;
    adds "refine" with the Dice and surface scores of the unrefined arg-max beside the refined ones, both before any clean-up."""
    cal = SG.CalibrationAccumulator(calibration["bins"]) if calibration else None
    acc = SG.SurfaceAccumulator(num_classes, len(tolerances))
    les = SG.LesionAccumulator(num_classes) if lesion else None
    counts, n = None, 0
    raw_acc, raw_counts = (SG.SurfaceAccumulator(num_classes, len(tolerances)), None) if refine else (None, None)
    ref_acc, ref_counts = (SG.SurfaceAccumulator(num_classes, len(tolerances)), None) if refine and post else (None, None)
    for x, sp, m, grid_sp in loader:
        x, m = x.to(device), m.to(device)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            logits = model(x, spacing=sp.to(device) if model.scale_aware else None)
        pred, cnt = ops.seg_predict(logits, model.patch, m)
        if refine:
            raw_counts = cnt.clone() if raw_counts is None else raw_counts + cnt
            sc, sv = ops.surface_stats(pred, m, grid_sp, num_classes, tolerances=tolerances)
            raw_acc.update(SG.surface_metrics(sc, sv, grid_sp, tuple(m.shape[-2:])))
            pred, _, cnt = ops.seg_refine(logits, x[:, 1].float().contiguous(), model.patch, m, inv_temperature=1.0 / model.temperature,
                                          **refine.to_dict())
            if post:                                # the refined map before the clean-up, for the "refine" block
                ref_counts = cnt.clone() if ref_counts is None else ref_counts + cnt
                sc, sv = ops.surface_stats(pred, m, grid_sp, num_classes, tolerances=tolerances)
                ref_acc.update(SG.surface_metrics(sc, sv, grid_sp, tuple(m.shape[-2:])))
        if cal:
            cal.update(ops.seg_calib(logits, model.patch, m, inv_temperature=1.0 / calibration["temperature"], bins=calibration["bins"],
                                     want_pred=False))
        if cache is not None:
            cache.append((logits.float(), m))
        if post:
            pred, cnt = ops.cc_filter(pred, num_classes, min_px=SG.min_component_px(post["min_area_mm2"], grid_sp, pred.shape[0]),
                                      keep_largest=post["keep_largest"], connectivity=post["connectivity"], targets=m)
        counts = cnt.clone() if counts is None else counts + cnt
        if lesion:
            les.update(ops.lesion_counts(pred, m, num_classes, connectivity=lesion["connectivity"], overlap=lesion["overlap"],
                                         min_px=SG.min_component_px(lesion["min_area_mm2"], grid_sp, pred.shape[0])))
        sc, sv = ops.surface_stats(pred, m, grid_sp, num_classes, tolerances=tolerances)
        acc.update(SG.surface_metrics(sc, sv, grid_sp, tuple(m.shape[-2:])))
        n += x.shape[0]
    counts = counts.cpu()
    res = acc.result()
    dice, iou = SG.dice_per_class(counts), SG.iou_per_class(counts)
    per_class = {"dice": _floats(dice), "iou": _floats(iou), "hd95_mm": _floats(res["hd95"]), "assd_mm": _floats(res["assd"]),
                 "nsd": {f"{t:g}": _floats(res["nsd"][:, i]) for i, t in enumerate(tolerances)}, "surface_images": res["images"].tolist(),
                 "overlap_images": n}
    mean = {"dice": SG.mean_dice(counts), "iou": SG.miou(counts), "hd95_mm": _mean_present(res["hd95"]), "assd_mm": _mean_present(res["assd"]),
            "nsd": {f"{t:g}": _mean_present(res["nsd"][:, i]) for i, t in enumerate(tolerances)},
            "classes": int((res["images"] > 0).sum())}
    report = {"images": n, "num_classes": num_classes, "tolerances_mm": list(tolerances), "quantile": "95/100 (nearest rank)",
              "spacing": SPACING_CONVENTION, "pixel_accuracy": SG.pixel_accuracy(counts), "per_class": per_class, "mean": mean}
    if refine:
        raw = raw_acc.result()

        def side(cn, rs):
            return {"dice": _floats(SG.dice_per_class(cn)), "mean_dice": SG.mean_dice(cn), "hd95_mm": _mean_present(rs["hd95"]),
                    "assd_mm": _mean_present(rs["assd"]), "nsd": {f"{t:g}": _mean_present(rs["nsd"][:, i]) for i, t in enumerate(tolerances)}}

        # both sides WITHOUT clean-up, so the pair isolates the refinement; with ``post`` the report's own scores are of the refined map
        # after the clean-up and "refined" is not a copy of them
        report["refine"] = {"parameters": refine.to_dict(), "temperature": float(model.temperature), "unrefined": side(raw_counts.cpu(), raw),
                            "refined": side(ref_counts.cpu(), ref_acc.result()) if post else side(counts, res),
                            "clean_up": "none: \"refined\" equals the report's own scores" if not post else
                                        "\"unrefined\" and \"refined\" are both taken before the clean-up; the report's own scores after it"}
    if post:
        report["postprocess"] = dict(post)
    if cal:
        report["calibration"] = calibration_object(cal.result(), calibration["temperature"], calibration["bins"])
    if lesion:
        report["lesion"] = lesion_report(les.result(), lesion["connectivity"], lesion["overlap"], lesion["min_area_mm2"])
    return report


def run(args: argparse.Namespace) -> dict:
    ap = build_parser()
    check_args(ap, args)
    device = torch.device(args.device)
    if device.type != "cuda":
        raise SystemExit(f"this engine computes on MI355X only: --device {args.device} requested (no CPU compute path)")
    if not args.synthetic and args.val_csv is None:
        ap.error("--val-csv is required unless --synthetic N is given")
    if args.val_csv is not None and not args.synthetic and not Path(args.val_csv).is_file():
        ap.error(f"--val-csv {args.val_csv}: no such file")
    tolerances = tuple(args.tolerance_mm) if args.tolerance_mm else (1.0, 2.0)
    if len(tolerances) > ops.SURFACE_MAX_TOLERANCES or any(not t >= 0 or t == float("inf") for t in tolerances):
        ap.error(f"--tolerance-mm: 1 to {ops.SURFACE_MAX_TOLERANCES} finite values >= 0, got {list(tolerances)}")
    if not 0.0 <= args.lesion_overlap <= 1.0:
        ap.error(f"--lesion-overlap: a fraction in [0, 1], got {args.lesion_overlap}")
    if not 0.0 <= args.min_component_mm2 < float("inf"):
        ap.error(f"--min-component-mm2: a finite area >= 0, got {args.min_component_mm2}")
    post = None
    if args.keep_largest or args.min_component_mm2 > 0:
        post = {"keep_largest": bool(args.keep_largest), "min_area_mm2": float(args.min_component_mm2), "connectivity": args.connectivity}
    lesion = None
    if args.lesion_metrics:
        lesion = {"connectivity": args.connectivity, "overlap": (round(1000 * args.lesion_overlap), 1000),
                  "min_area_mm2": float(args.min_component_mm2)}
    cfg_file = Path(args.segmenter) / SG.CONFIG_FILE
    if not cfg_file.is_file():
        ap.error(f"--segmenter {args.segmenter}: no {SG.CONFIG_FILE} (not an output directory of finetune_segmentation.py)")
    cfg = json.loads(cfg_file.read_text())
    if cfg.get("task") != "segmentation":
        ap.error(f"--segmenter {args.segmenter}: task {cfg.get('task')!r} is not 'segmentation'")
    if not torch.cuda.is_available():
        raise SystemExit("this engine computes on MI355X only: no CUDA/HIP device available")
    refine = refine_config(args, cfg.get("refine"), ap)      # a bad stored "refine" is refused here, before the model is loaded
    model = SG.load_segmenter(args.backbone, args.segmenter, device)
    C, img = cfg["num_classes"], model.img_size
    if args.synthetic:
        n_val = max(args.synthetic // 4, 1)
        ds = EvalSynthetic(n_val, img, C, args.seed, first=args.synthetic - n_val, augment=False)
        workers = 0
    else:
        rows = fs.read_csv(args.val_csv)
        if not rows[0].has_spacing:
            log.warning("the CSV has no spacing_x/y/z columns: 1 mm per source pixel is assumed, so the mm figures are in source pixels")
        ds = EvalImages(rows, img, input_format=args.input_format, window_level=args.window_level, window_width=args.window_width,
                        augment=False, data_root=args.data_root)
        workers = args.num_workers
    loader = torch.utils.data.DataLoader(ds, batch_size=args.batch_size, shuffle=False, num_workers=workers)
    calibration = cache = None
    if args.calibration or args.fit_temperature:
        calibration = {"bins": args.calibration_bins, "temperature": float(args.temperature if args.temperature is not None else model.temperature)}
    if args.fit_temperature:
        need = len(ds) * ((img // model.patch) ** 2 * C * 4 + img * img)
        if need > args.calibration_cache_gib * 2 ** 30:
            raise SystemExit(f"--fit-temperature: the patch logits and labels of {len(ds)} images take {need / 2 ** 30:.2f} GiB of device memory, "
                             f"above --calibration-cache-gib {args.calibration_cache_gib:g}; raise it or fit on a subset")
        cache = []
    report = evaluate(model, loader, device, not args.no_amp, tolerances, C, lesion=lesion, post=post, calibration=calibration, cache=cache,
                      refine=refine)
    if refine and args.write_refine:
        cfg["refine"] = refine.to_dict()
        cfg_file.write_text(json.dumps(cfg, indent=2))
    if args.fit_temperature:
        fit = SG.fit_temperature(cache, model.patch)
        after = SG.CalibrationAccumulator(args.calibration_bins)
        for z, m in cache:
            after.update(ops.seg_calib(z, model.patch, m, inv_temperature=1.0 / fit["temperature"], bins=args.calibration_bins, want_pred=False))
        report["temperature_fit"] = fit
        report["calibration_fitted"] = calibration_object(after.result(), fit["temperature"], args.calibration_bins)
        log.info("fitted temperature %.4f: NLL %s -> %s, ECE %s -> %s", fit["temperature"], fit["nll_before"], fit["nll_after"],
                 report["calibration"]["ece"], report["calibration_fitted"]["ece"])
        if args.write_temperature:
            cfg["temperature"] = fit["temperature"]
            cfg_file.write_text(json.dumps(cfg, indent=2))
    report["segmenter"], report["backbone"] = str(args.segmenter), str(args.backbone)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(report, indent=2))
    log.info("%d images: mean Dice %.4f, HD95 %s mm, ASSD %s mm -> %s", report["images"], report["mean"]["dice"], report["mean"]["hd95_mm"],
             report["mean"]["assd_mm"], args.out)
    return report


def main(argv=None) -> dict:
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)s] %(message)s", datefmt="%H:%M:%S")
    return run(args)


if __name__ == "__main__":
    main()
