#!/usr/bin/env python3
"""Dense segmentation fine-tuning of a DINO-X backbone on the HIP engine: a linear head on the patch tokens, cross-entropy + soft Dice.

    python scripts/finetune_segmentation.py --backbone runs/x/hub-export/ --train-csv train.csv --val-csv val.csv \\
        --num-classes 3 --rank 0 --epochs 50 --output seg/x/                       # --rank 0: frozen backbone, linear probe
    python scripts/finetune_segmentation.py --backbone runs/x/hub-export/ --synthetic 48 --num-classes 3 --epochs 3 --output /tmp/s

CSV columns: image_path,mask_path[,spacing_x,spacing_y,spacing_z].  The mask is an 8-bit single-channel PNG of class indices, 255 = ignore.
Image and mask get the same random-resized crop window and the same flip (image bicubic, mask nearest); validation takes the centre crop
of both.  The loss and the validation metrics run at full resolution inside csrc/segloss.hip (ops.SegLossFn, ops.seg_predict): the
[B, P, C] patch logits are the only logits in memory.  Optimiser, schedule, pixel reading and the adapter come from finetune_lora.py.
--boundary-weight W adds Kervadec's boundary loss (the softmax probabilities weighted by the signed distance to each class's region,
ops.signed_distance_map + ops.SegBoundaryLossFn) with --boundary-ramp-epochs and --boundary-units px|mm; 0, the default, is the run
without it.
--patch-train trains on patches at native resolution instead (dinox.patches, csrc/segpatch.hip): the training set lives on the device,
every batch is drawn as affine jobs (foreground-oversampled centres, rotation, scaling, mirrors, gamma, gain) and sampled by one kernel
launch -- no DataLoader, no host transform -- which is what scripts/segment_volume.py --tiled shows the model afterwards.  --patch-val
tiled validates each image on its own grid through the sliding-window path.
Written to --output whenever the early-stopping metric improves: the adapter files (rank > 0), seg_head.pth, finetune_config.json and,
with --unfreeze-blocks, unfrozen_blocks.pth; dinox.segment.load_segmenter puts them back together.
"""
from __future__ import annotations

import argparse
import csv
import json
import logging
import math
import random
import sys
import time
from dataclasses import asdict, dataclass
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

_HERE = Path(__file__).resolve().parent
for _p in (_HERE.parent, _HERE):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import finetune_lora as fl  # noqa: E402
from dinox import ops, patches as PT, segment as SG, tiled as TL  # noqa: E402
from zoo.hub import load_model  # noqa: E402
from zoo.peft import apply_lora, save_adapter  # noqa: E402

log = logging.getLogger("finetune_segmentation")

IGNORE = ops.SEG_IGNORE


# ------------------------------------------------------------------------------------------ records, paired transforms
@dataclass
class MaskedRow(fl.LabeledRow):
    mask_path: Path = Path()


def read_csv(path: Path) -> List[MaskedRow]:
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        cols = rd.fieldnames or []
        lacking = {"image_path", "mask_path"} - set(cols)
        if lacking:
            raise ValueError(f"{path}: column(s) {sorted(lacking)} missing (found {cols})")
        sp = all(c in cols for c in ("spacing_x", "spacing_y", "spacing_z"))
        rows = []
        for n, rec in enumerate(rd, 2):
            try:
                spacing = tuple(float(rec[c]) for c in ("spacing_x", "spacing_y", "spacing_z")) if sp else (1.0, 1.0, 1.0)
                rows.append(MaskedRow(Path(rec["image_path"]), 0.0, spacing, sp, Path(rec["mask_path"])))
            except (TypeError, ValueError) as e:
                raise ValueError(f"{path}, line {n}: {e}") from e
    return rows


def _resize_mask(m: torch.Tensor, h: int, w: int) -> torch.Tensor:
    if m.shape[-2:] == (h, w):
        return m
    return F.interpolate(m[None, None].float(), size=(h, w), mode="nearest")[0, 0].to(torch.uint8)


def _crop_window(h: int, w: int, gen: torch.Generator, scale=(0.7, 1.0), ratio=(3 / 4, 4 / 3)) -> Optional[Tuple[int, int, int, int]]:
    """(top, left, height, width) drawn as finetune_lora.random_resized_crop draws it; None after ten misses."""
    for _ in range(10):
        area = h * w * float(torch.empty(1).uniform_(scale[0], scale[1], generator=gen))
        asp = math.exp(float(torch.empty(1).uniform_(math.log(ratio[0]), math.log(ratio[1]), generator=gen)))
        cw, ch = int(round(math.sqrt(area * asp))), int(round(math.sqrt(area / asp)))
        if 0 < cw <= w and 0 < ch <= h:
            return int(torch.randint(0, h - ch + 1, (1,), generator=gen)), int(torch.randint(0, w - cw + 1, (1,), generator=gen)), ch, cw
    return None


def _center_pair(x: torch.Tensor, m: torch.Tensor, size: int):
    h, w = x.shape[-2:]
    k = size / min(h, w)
    nh, nw = max(size, round(h * k)), max(size, round(w * k))
    x, m = fl._resize(x, nh, nw), _resize_mask(m, nh, nw)
    t, l = (nh - size) // 2, (nw - size) // 2
    return x[:, t:t + size, l:l + size], m[t:t + size, l:l + size]


def _center_factors(h: int, w: int, size: int) -> Tuple[float, float]:
    """(h / nh, w / nw) of _center_pair: source pixels per pixel of the centre crop (evaluate_segmentation.py's convention)."""
    k = size / min(h, w)
    return h / max(size, round(h * k)), w / max(size, round(w * k))


def paired_transform_grid(x: torch.Tensor, m: torch.Tensor, size: int, gen: torch.Generator, augment: bool):
    """paired_transform (below) and the grid it lands on: (image, mask, (f_y, f_x)), f = source pixels per output pixel along each axis --
    ch / size and cw / size for a crop window ch x cw, the centre crop's resize factors otherwise.  The same draws in the same order."""
    if x.shape[-2:] != m.shape[-2:]:
        raise ValueError(f"image {tuple(x.shape[-2:])} and mask {tuple(m.shape[-2:])} differ in size")
    h, w = x.shape[-2:]
    if augment:
        win = _crop_window(h, w, gen)
        if win is None:
            x, m, f = *_center_pair(x, m, size), _center_factors(h, w, size)
        else:
            t, l, ch, cw = win
            x, m = fl._resize(x[:, t:t + ch, l:l + cw], size, size), _resize_mask(m[t:t + ch, l:l + cw], size, size)
            f = (ch / size, cw / size)
        if float(torch.rand(1, generator=gen)) < 0.5:
            x, m = x.flip(-1), m.flip(-1)
    else:
        x, m, f = *_center_pair(x, m, size), _center_factors(h, w, size)
    return fl.normalize(x).contiguous(), m.contiguous(), f


def paired_transform(x: torch.Tensor, m: torch.Tensor, size: int, gen: torch.Generator, augment: bool):
    """image [3, H, W] in [0, 1] and mask uint8 [H, W] -> (normalised image [3, size, size], mask uint8 [size, size]).  ``augment``: one
    random-resized crop window and one horizontal flip for both; otherwise the centre crop of both.  The image is resized bicubic, the
    mask nearest, so the mask holds only values of the source mask."""
    return paired_transform_grid(x, m, size, gen, augment)[:2]


class MaskedImages(fl.LabeledImages):
    """(image [3, S, S], spacing [3], mask uint8 [S, S]) per row; the pixel reading is finetune_lora's."""

    def read_mask(self, row: MaskedRow) -> torch.Tensor:
        from PIL import Image
        p = row.mask_path if row.mask_path.is_absolute() or self.root is None else self.root / row.mask_path
        a = np.asarray(Image.open(p))
        if a.ndim != 2 or a.dtype != np.uint8:
            raise ValueError(f"{p}: the mask must be an 8-bit single-channel image of class indices (got {a.dtype}, shape {a.shape})")
        return torch.from_numpy(a.copy())

    def __getitem__(self, i: int):
        row = self.rows[i]
        x, m = paired_transform(self.pixels(row)[None].expand(3, -1, -1), self.read_mask(row), self.img_size, self.gen, self.augment)
        return x, torch.tensor(row.spacing, dtype=torch.float32), m


class SyntheticMasks(fl.LabeledImages):
    """``n`` seeded images whose labels can be read off the pixels: noise around 0.2 (class 0) and C - 1 rectangles of rising brightness
    (classes 1 .. C - 1, later ones on top); the four left-most columns are marked 255 (ignore)."""

    def __init__(self, n: int, img_size: int, num_classes: int, seed: int, first: int = 0, augment: bool = False) -> None:
        super().__init__([], img_size, "float01", augment=augment, seed=seed + 1 + first)
        g = torch.Generator().manual_seed(seed * 7919 + 17)
        total, S = first + n, img_size
        img = 0.2 + 0.1 * (torch.rand((total, S, S), generator=g) - 0.5)
        noise = torch.rand((total, S, S), generator=g)
        mask = torch.zeros((total, S, S), dtype=torch.uint8)
        for c in range(1, num_classes):
            h = torch.randint(S // 4, S // 2 + 1, (total, 2), generator=g)
            t = (torch.rand((total, 2), generator=g) * (S - h)).long()
            for i in range(total):
                ys, xs = slice(int(t[i, 0]), int(t[i, 0] + h[i, 0])), slice(int(t[i, 1]), int(t[i, 1] + h[i, 1]))
                img[i, ys, xs] = 0.2 + 0.7 * c / (num_classes - 1) + 0.1 * (noise[i, ys, xs] - 0.5)
                mask[i, ys, xs] = c
        mask[:, :, :4] = IGNORE
        self.images, self.masks = img.clamp(0, 1)[first:, None], mask[first:]
        self.spacings = 0.5 + torch.rand((total, 3), generator=g)[first:]

    def __len__(self) -> int:
        return self.images.shape[0]

    def __getitem__(self, i: int):
        x, m = paired_transform(self.images[i].expand(3, -1, -1), self.masks[i], self.img_size, self.gen, self.augment)
        return x, self.spacings[i], m


class GridMaskedImages(MaskedImages):
    """MaskedImages that also returns the spacing of the grid the sample landed on, (s_y, s_x) in mm per label-map pixel (--boundary-units
    mm): the CSV's (spacing_y f_y, spacing_x f_x) with paired_transform_grid's factors."""

    def __getitem__(self, i: int):
        row = self.rows[i]
        x, m, (fy, fx) = paired_transform_grid(self.pixels(row)[None].expand(3, -1, -1), self.read_mask(row), self.img_size, self.gen,
                                               self.augment)
        return (x, torch.tensor(row.spacing, dtype=torch.float32), m,
                torch.tensor([row.spacing[1] * fy, row.spacing[0] * fx], dtype=torch.float32))


class GridSyntheticMasks(SyntheticMasks):
    """SyntheticMasks with the (s_y, s_x) of its own spacings as the grid spacing: the maps keep their own, cropped or not."""

    def __getitem__(self, i: int):
        x, sp, m = super().__getitem__(i)
        return x, sp, m, torch.stack([sp[1], sp[0]])


# ------------------------------------------------------------------------------------------ epochs, saving
@dataclass
class SegConfig(fl.FinetuneConfig):
    ce_weight: float = 1.0
    dice_weight: float = 1.0
    dice_c0: int = 0
    ignore_index: int = IGNORE
    best_dice_per_class: Optional[List[float]] = None
    boundary_weight: float = 0.0
    boundary_ramp_epochs: int = 0
    boundary_units: str = "px"
    patch_train: bool = False                                # the patch settings: off, and then every other one is at its "unset" value
    patch_size: int = 0
    patch_fg_prob: float = 0.0
    patch_rotate_deg: float = 0.0
    patch_scale: Optional[List[float]] = None
    patches_per_epoch: int = 0
    patch_val: str = "center"


def boundary_weight(w: float, ramp_epochs: int, epoch: int) -> float:
    """The training weight of the boundary term in 0-based ``epoch``: w min(1, (epoch + 1) / ramp_epochs); ramp_epochs = 0: constant."""
    return w if ramp_epochs <= 0 else w * min(1.0, (epoch + 1) / ramp_epochs)


def _batches_grid(loader, device, scale_aware):
    """_batches with the spacing of each sample's label grid [B, 2] = (s_y, s_x): the loader's fourth element, or 1 (pixels) without one."""
    for batch in loader:
        x, sp, m = batch[:3]
        grid = batch[3].to(device) if len(batch) > 3 else torch.ones((x.shape[0], 2), dtype=torch.float32, device=device)
        yield x.to(device), (sp.to(device) if scale_aware else None), m.to(device), grid


def _batches(loader, device, scale_aware):
    for x, sp, m in loader:
        yield x.to(device), (sp.to(device) if scale_aware else None), m.to(device)


def train_epoch(model, loader, opt: fl.ArenaAdamW, sched, device, scale_aware, amp, w_ce, w_dice, c0, w_bd: float = 0.0) -> float:
    """w_bd > 0: the boundary term joins the loss, phi computed on the device once per batch from the batch's masks."""
    model.train()
    tot, n = 0.0, 0
    if w_bd > 0:
        for x, sp, m, grid in _batches_grid(loader, device, scale_aware):
            opt.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
                logits = model(x, spacing=sp)
            phi = ops.signed_distance_map(m, grid, logits.shape[-1])
            loss = ops.SegBoundaryLossFn.apply(logits, m, phi, w_ce, w_dice, w_bd, c0)[0]
            loss.backward()
            opt.step(sched(opt.t))
            tot, n = tot + float(loss.detach()), n + 1
        return tot / max(n, 1)
    for x, sp, m in _batches(loader, device, scale_aware):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            logits = model(x, spacing=sp)
        loss, _, _ = ops.SegLossFn.apply(logits, m, w_ce, w_dice, c0)
        loss.backward()
        opt.step(sched(opt.t))
        tot, n = tot + float(loss.detach()), n + 1
    return tot / max(n, 1)


@torch.no_grad()
def validate(model, loader, device, scale_aware, amp, w_ce, w_dice, c0, w_bd: float = 0.0):
    """-> (mean loss, metrics, counts int64 [3, C] on the host, label maps uint8 [n, S, S] on the host).  w_bd > 0: the loss carries the
    boundary term at that weight."""
    model.eval()
    tot, n, counts, preds = 0.0, 0, None, []
    for x, sp, m, grid in (_batches_grid(loader, device, scale_aware) if w_bd > 0 else ((*b, None) for b in _batches(loader, device, scale_aware))):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            logits = model(x, spacing=sp)
        if w_bd > 0:
            phi = ops.signed_distance_map(m, grid, logits.shape[-1])
            tot, n = tot + float(ops.seg_loss_bd_fwd(logits, m, phi, w_ce, w_dice, w_bd, c0)[0][0]), n + 1
        else:
            tot, n = tot + float(ops.seg_loss_fwd(logits, m, w_ce, w_dice, c0)[0][0]), n + 1
        pred, cnt = ops.seg_predict(logits, model.patch, m)
        counts = cnt.clone() if counts is None else counts + cnt
        preds.append(pred.cpu())
    counts = counts.cpu()
    metrics = {"loss": tot / max(n, 1), "mean_dice": SG.mean_dice(counts, skip_background=bool(c0)), "miou": SG.miou(counts),
               "pixel_accuracy": SG.pixel_accuracy(counts)}
    return metrics["loss"], metrics, counts, torch.cat(preds)


# nnU-Net's intensity augmentation: gamma on 30 % of the patches, a multiplicative brightness on 15 %
PATCH_GAMMA = dict(gamma_range=(0.7, 1.5), gamma_prob=0.3, gain_range=(0.75, 1.25), gain_prob=0.15)


def dataset_planes(ds) -> List[Tuple[np.ndarray, np.ndarray, Tuple[float, float, float]]]:
    """(image fp32 (H, W) in [0, 1], mask uint8 (H, W), (sx, sy, sz)) of every sample of a MaskedImages / SyntheticMasks, untransformed."""
    if hasattr(ds, "images"):
        return [(ds.images[i, 0].numpy(), ds.masks[i].numpy(), tuple(float(v) for v in ds.spacings[i])) for i in range(len(ds))]
    return [(ds.pixels(r).numpy(), ds.read_mask(r).numpy(), tuple(float(v) for v in r.spacing)) for r in ds.rows]


def train_epoch_patches(model, pool: PT.PatchPool, gen: torch.Generator, steps: int, batch_size: int, draw: dict, opt: fl.ArenaAdamW, sched,
                        device, scale_aware, amp, w_ce, w_dice, c0, w_bd: float = 0.0, mm: bool = False) -> float:
    """train_epoch on ``steps`` batches of patches: jobs drawn on the host (dinox.patches.draw_patch_jobs, ``draw`` its keywords), both
    tensors of a batch from one ops.seg_patch_sample launch.  ``mm``: the boundary term measures on the jobs' own grid spacing."""
    model.train()
    tot, S = 0.0, draw["S"]
    for _ in range(steps):
        d = PT.draw_patch_jobs(pool, batch_size, gen, **draw)
        x, m = ops.seg_patch_sample(pool.img, pool.msk, d["jobs"], d["par"], S, fl.MEAN, fl.STD)
        sp = torch.from_numpy(d["model_spacing"]).to(device) if scale_aware else None
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            logits = model(x, spacing=sp)
        if w_bd > 0:
            grid = torch.from_numpy(d["grid_spacing"]).to(device) if mm else torch.ones((batch_size, 2), dtype=torch.float32, device=device)
            phi = ops.signed_distance_map(m, grid, logits.shape[-1])
            loss = ops.SegBoundaryLossFn.apply(logits, m, phi, w_ce, w_dice, w_bd, c0)[0]
        else:
            loss = ops.SegLossFn.apply(logits, m, w_ce, w_dice, c0)[0]
        loss.backward()
        opt.step(sched(opt.t))
        tot += float(loss.detach())
    return tot / max(steps, 1)


@torch.no_grad()
def validate_tiled(model, planes, tile: int, batch_size: int, device, amp, c0):
    """Every validation image on its own grid (dinox.tiled: overlap 0.5, Gaussian window, tile side ``tile``), grouped by size and spacing
    since a blend launch takes one size.  -> (1 - mean Dice, metrics, counts int64 [3, C] on the host, the label maps as a list of uint8
    (H, W) arrays).  No soft loss exists on this path: "loss" is 1 - mean Dice of the label maps, from the blend kernel's counts."""
    model.eval()
    groups = {}
    for k, (im, _, sp) in enumerate(planes):
        groups.setdefault((im.shape, sp), []).append(k)
    counts, preds = None, [None] * len(planes)
    for (_, sp), ks in groups.items():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            out, cnt = TL.tiled_label_counts(model, np.stack([planes[k][0] for k in ks]), np.stack([planes[k][1] for k in ks]), sp, tile=tile,
                                             overlap=0.5, window="gaussian", batch_size=batch_size, device=device)
        counts = cnt.clone() if counts is None else counts + cnt
        for k, o in zip(ks, out):
            preds[k] = o
    counts = counts.cpu()
    dice = SG.mean_dice(counts, skip_background=bool(c0))
    metrics = {"loss": 1.0 - dice, "mean_dice": dice, "miou": SG.miou(counts), "pixel_accuracy": SG.pixel_accuracy(counts)}
    return metrics["loss"], metrics, counts, preds


def save_segmenter(model: SG.SegModel, vit: nn.Module, output_dir: Path, config: SegConfig) -> None:
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    if config.rank > 0:
        save_adapter(model.backbone, output_dir)
    torch.save({k: v.detach().cpu().clone() for k, v in model.head.state_dict().items()}, output_dir / SG.HEAD_FILE)
    if config.unfreeze_blocks > 0:
        state = {}
        for i in fl.unfrozen_block_range(len(vit.blocks), config.unfreeze_blocks):
            for name, p in vit.blocks[i].named_parameters():
                if ".lora_" not in name:
                    state[f"blocks.{i}.{name}"] = p.detach().cpu().clone()
        torch.save(state, output_dir / SG.BLOCKS_FILE)
    (output_dir / SG.CONFIG_FILE).write_text(json.dumps(asdict(config), indent=2, default=str))


# ------------------------------------------------------------------------------------------ command line
def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Segmentation fine-tuning of a DINO-X backbone (linear head on the patch tokens)",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    base = {a.dest: a for a in fl.build_parser()._actions}
    for dest in ("backbone", "device", "train_csv", "val_csv", "synthetic", "data_root", "input_format", "window_level", "window_width",
                 "num_classes", "rank", "alpha", "lora_dropout", "epochs", "batch_size", "lr", "weight_decay", "warmup_epochs", "patience"):
        ap._add_action(base[dest])                           # the very flags of finetune_lora.py: names, types, defaults, help
    ap.add_argument("--es-metric", default="loss", choices=["loss", "mean_dice"], help="'loss' (lower is better) or 'mean_dice' (higher is better)")
    for dest in ("num_workers", "no_amp", "seed", "unfreeze_blocks", "backbone_lr", "output"):
        ap._add_action(base[dest])
    ap.add_argument("--ce-weight", type=float, default=1.0, help="weight of the cross-entropy term")
    ap.add_argument("--dice-weight", type=float, default=1.0, help="weight of the soft Dice term")
    ap.add_argument("--dice-skip-background", action="store_true", help="leave class 0 out of the Dice term (c0 = 1)")
    ap.add_argument("--ignore-index", type=int, default=IGNORE, help="label value left out of loss and metrics; only 255 is supported")
    return ap


def build_boundary_parser() -> argparse.ArgumentParser:
    """The options of the boundary loss.  They are a parser of their own (build_parser() keeps its flag set); parse_cli reads them out of
    the command line first."""
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    ap.add_argument("--boundary-weight", type=float, default=0.0, metavar="W",
                    help="weight of the boundary term (signed distance to each class's region times its softmax probability); 0: off")
    ap.add_argument("--boundary-ramp-epochs", type=int, default=0, metavar="E",
                    help="the training weight in epoch e (from 0) is W min(1, (e + 1) / E); 0: constant.  Validation always uses W")
    ap.add_argument("--boundary-units", choices=["px", "mm"], default="px",
                    help="distances in label-map pixels, or in mm on the spacing of the augmented grid (synthetic maps keep their own)")
    return ap


def build_patch_parser() -> argparse.ArgumentParser:
    """The options of patch training.  A parser of their own, as the boundary options are; parse_cli reads them out of the command line."""
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    ap.add_argument("--patch-train", action="store_true", help="train on patches at native resolution, sampled on the device")
    ap.add_argument("--patch-size", type=int, default=None, metavar="T", help="side of a patch in source pixels at scale 1 (default: the model's S)")
    ap.add_argument("--patch-fg-prob", type=float, default=0.33, help="share of patches centred on a pixel of a class present in the sample")
    ap.add_argument("--patch-rotate-deg", type=float, default=15.0, help="rotation drawn uniformly in [-D, D] degrees")
    ap.add_argument("--patch-scale", type=float, nargs=2, default=[0.7, 1.4], metavar=("LO", "HI"),
                    help="source pixels per output pixel, relative to T / S, drawn uniformly in [LO, HI]")
    ap.add_argument("--patches-per-epoch", type=int, default=None, metavar="N", help="patches per epoch (default: the number of training samples)")
    ap.add_argument("--patch-pool-gib", type=float, default=16.0, help="refuse a training set that needs more device memory than this")
    ap.add_argument("--patch-val", choices=["center", "tiled"], default="center",
                    help="validation: the centre crop at S x S, or every image on its own grid by sliding window (tile side T, overlap 0.5)")
    return ap


def build_calibration_parser() -> argparse.ArgumentParser:
    """The option of temperature fitting.  A parser of its own, as the boundary options are; parse_cli reads it out of the command line."""
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    ap.add_argument("--fit-temperature", action="store_true",
                    help="after training, reload the best checkpoint, fit the softmax temperature that minimises the NLL of the validation set "
                         "(dinox.segment.fit_temperature) and store it as \"temperature\" in finetune_config.json")
    return ap


def parse_cli(argv=None) -> argparse.Namespace:
    """The boundary options (build_boundary_parser), the patch options (build_patch_parser) and the calibration option
    (build_calibration_parser) first, everything else through build_parser; one namespace."""
    bd, rest = build_boundary_parser().parse_known_args(argv)
    pt, rest = build_patch_parser().parse_known_args(rest)
    cb, rest = build_calibration_parser().parse_known_args(rest)
    ap = build_parser()
    ap.epilog = ("Boundary loss: " + " ".join(build_boundary_parser().format_help().split()[1:]) + "  Patch training: "
                 + " ".join(build_patch_parser().format_help().split()[1:]) + "  Calibration: "
                 + " ".join(build_calibration_parser().format_help().split()[1:]))
    args = ap.parse_args(rest)
    for k, v in (*vars(bd).items(), *vars(pt).items(), *vars(cb).items()):
        setattr(args, k, v)
    return args


@torch.no_grad()
def fit_and_store_temperature(backbone_path, output_dir: Path, loader, device, scale_aware: bool, amp: bool) -> dict:
    """Reloads the best checkpoint from ``output_dir``, caches the validation set's patch logits and labels on the device, fits the
    temperature and adds "temperature" to the written finetune_config.json (every other byte of it stays).  -> fit_temperature's dict."""
    model = SG.load_segmenter(backbone_path, output_dir, device)
    cache = []
    for x, sp, m in _batches(loader, device, scale_aware):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            cache.append((model(x, spacing=sp).float(), m))
    fit = SG.fit_temperature(cache, model.patch)
    cfg_file = Path(output_dir) / SG.CONFIG_FILE
    cfg = json.loads(cfg_file.read_text())
    cfg["temperature"] = fit["temperature"]
    cfg_file.write_text(json.dumps(cfg, indent=2))
    log.info("temperature %.4f (%d passes%s): validation NLL %s -> %s", fit["temperature"], fit["iterations"],
             "" if fit["converged"] else ", not converged", fit["nll_before"], fit["nll_after"])
    return fit


def warn_mm_without_spacing(rows: List[MaskedRow], units: str) -> bool:
    """--boundary-units mm on a CSV without spacing columns: warn and take 1 mm per source pixel, as evaluate_segmentation.py does."""
    if units == "mm" and rows and not rows[0].has_spacing:
        log.warning("--boundary-units mm, but the CSV has no spacing_x/y/z columns: 1 mm per source pixel is assumed, so the boundary "
                    "term measures in source pixels")
        return True
    return False


def run(args: argparse.Namespace) -> dict:
    """One run -> {"config": SegConfig, "val_pred": the best epoch's validation label maps uint8 [n, S, S] (host; under --patch-val tiled
    a list of (H, W) arrays, each image's own grid), "val_dataset": the validation set}.  A namespace without the boundary attributes (build_parser() alone) runs without the boundary term."""
    ap = build_parser()
    w_bd, ramp = float(getattr(args, "boundary_weight", 0.0)), int(getattr(args, "boundary_ramp_epochs", 0))
    units = getattr(args, "boundary_units", "px")
    if not (w_bd >= 0 and math.isfinite(w_bd)):
        ap.error(f"--boundary-weight {w_bd}: the weight must be finite and >= 0 (0: no boundary term)")
    if ramp < 0:
        ap.error(f"--boundary-ramp-epochs {ramp}: the number of ramp epochs must be >= 0 (0: constant weight)")
    if units not in ("px", "mm"):
        ap.error(f"--boundary-units {units!r}: px or mm")
    mm = w_bd > 0 and units == "mm"                          # only then does a sample carry its grid spacing
    pdef = build_patch_parser().parse_args([])               # a namespace without the patch attributes runs without patch training
    patch = {k: getattr(args, k, v) for k, v in vars(pdef).items()}
    if patch["patch_size"] is not None and patch["patch_size"] < 1:
        ap.error(f"--patch-size {patch['patch_size']}: the patch side must be >= 1")
    if not 0.0 <= patch["patch_fg_prob"] <= 1.0:
        ap.error(f"--patch-fg-prob {patch['patch_fg_prob']}: a probability in [0, 1]")
    if not 0.0 <= patch["patch_rotate_deg"] <= 180.0:
        ap.error(f"--patch-rotate-deg {patch['patch_rotate_deg']}: degrees in [0, 180]")
    lo, hi = patch["patch_scale"]
    if not (math.isfinite(lo) and math.isfinite(hi) and 0 < lo <= hi):
        ap.error(f"--patch-scale {lo} {hi}: finite, 0 < LO <= HI")
    if patch["patches_per_epoch"] is not None and patch["patches_per_epoch"] < args.batch_size:
        ap.error(f"--patches-per-epoch {patch['patches_per_epoch']} does not fill one batch of {args.batch_size}")
    if not patch["patch_pool_gib"] > 0:
        ap.error(f"--patch-pool-gib {patch['patch_pool_gib']}: must be > 0")
    if patch["patch_val"] not in ("center", "tiled"):
        ap.error(f"--patch-val {patch['patch_val']!r}: center or tiled")
    if patch["patch_val"] == "tiled" and not patch["patch_train"]:
        ap.error("--patch-val tiled belongs to --patch-train")
    fit_t = bool(getattr(args, "fit_temperature", False))
    if fit_t and patch["patch_val"] == "tiled":
        ap.error("--fit-temperature fits on the S x S validation crops: not with --patch-val tiled")
    if args.ignore_index != IGNORE:
        ap.error(f"--ignore-index {args.ignore_index}: only {IGNORE} is supported (the kernels compare labels with that value)")
    if not 2 <= args.num_classes <= ops.SEG_MAX_CLASSES:
        ap.error(f"--num-classes {args.num_classes}: the segmentation kernels take 2 to {ops.SEG_MAX_CLASSES} classes")
    if not args.synthetic and (args.train_csv is None or args.val_csv is None):
        ap.error("--train-csv and --val-csv are required unless --synthetic N is given")
    device = torch.device(args.device)
    amp = not args.no_amp and device.type == "cuda"
    if args.seed is not None:
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
    seed = args.seed if args.seed is not None else 0
    c0 = 1 if args.dice_skip_background else 0

    backbone = load_model(args.backbone, device=str(device))
    scale_aware, dim, img = backbone.scale_aware, backbone.dim, backbone.img_size
    if backbone.patch > ops.SEG_MAX_UPSAMPLE:
        ap.error(f"patch size {backbone.patch}: the segmentation kernels upsample by at most {ops.SEG_MAX_UPSAMPLE}")
    if args.synthetic:
        n_val = max(args.synthetic // 4, 1)
        n_train = args.synthetic - n_val
        synth = GridSyntheticMasks if mm else SyntheticMasks
        train_ds = synth(n_train, img, args.num_classes, seed, first=0, augment=True)
        val_ds = synth(n_val, img, args.num_classes, seed, first=n_train, augment=False)
        workers = 0
    else:
        rows_t, rows_v = read_csv(args.train_csv), read_csv(args.val_csv)
        if scale_aware and not rows_t[0].has_spacing:
            log.warning("scale-aware backbone, but the CSV has no spacing_x/y/z columns: 1 mm is assumed everywhere")
        kw = dict(input_format=args.input_format, window_level=args.window_level, window_width=args.window_width, data_root=args.data_root)
        if w_bd > 0:
            warn_mm_without_spacing(rows_t, units)
        masked = GridMaskedImages if mm else MaskedImages
        train_ds = masked(rows_t, img, augment=True, seed=seed + 1, **kw)
        val_ds = masked(rows_v, img, augment=False, **kw)
        workers = args.num_workers
    gen = torch.Generator().manual_seed(seed)
    if patch["patch_train"]:                                 # no loader: the datasets only hand their untransformed planes to the pool
        train_loader = None
        per_epoch = (patch["patches_per_epoch"] or len(train_ds)) // args.batch_size
    else:
        train_loader = torch.utils.data.DataLoader(train_ds, batch_size=args.batch_size, shuffle=True, drop_last=True, num_workers=workers,
                                                   generator=gen)
        per_epoch = len(train_loader)
    val_loader = (torch.utils.data.DataLoader(val_ds, batch_size=args.batch_size, shuffle=False, num_workers=workers)
                  if patch["patch_val"] == "center" else None)
    if per_epoch == 0:
        ap.error(f"{len(train_ds)} training samples do not fill one batch of {args.batch_size}")

    if args.rank > 0:
        backbone = apply_lora(backbone, rank=args.rank, alpha=args.alpha, dropout=args.lora_dropout)
        vit = backbone.base_model.model
    else:                                                    # linear probe: no adapter, nothing of the backbone trains
        vit = backbone
        for p in vit.parameters():
            p.requires_grad = False
    base_params: List[nn.Parameter] = []
    for i in fl.unfrozen_block_range(len(vit.blocks), args.unfreeze_blocks):
        for p in vit.blocks[i].parameters():
            if not p.requires_grad:
                p.requires_grad = True
                base_params.append(p)
    frozen = args.rank == 0 and not base_params
    model = SG.SegModel(backbone, SG.SegHead(dim, args.num_classes), frozen_backbone=frozen).to(device)
    base_ids = {id(p) for p in base_params}
    fast = [p for p in backbone.parameters() if p.requires_grad and id(p) not in base_ids] + list(model.head.parameters())
    log.info("%d adapter + %d unfrozen + %d head parameters train%s", sum(p.numel() for p in fast) - sum(p.numel() for p in model.head.parameters()),
             sum(p.numel() for p in base_params), sum(p.numel() for p in model.head.parameters()), " (backbone under no_grad)" if frozen else "")
    opt = fl.ArenaAdamW([(fast, args.lr), (base_params, args.backbone_lr)], args.weight_decay)
    if patch["patch_train"]:
        tile = patch["patch_size"] or img
        train_planes = dataset_planes(train_ds)
        try:
            pool = PT.PatchPool([p[0] for p in train_planes], [p[1] for p in train_planes], [p[2] for p in train_planes], device=device,
                                max_gib=patch["patch_pool_gib"], seed=seed)
        except ValueError as e:
            ap.error(str(e))
        draw = dict(S=img, t=tile, fg_prob=patch["patch_fg_prob"], rotate_deg=patch["patch_rotate_deg"], scale_range=(lo, hi), **PATCH_GAMMA)
        patch_gen = torch.Generator().manual_seed(seed + 2)
        val_planes = dataset_planes(val_ds) if patch["patch_val"] == "tiled" else None
    steps, warm = args.epochs * per_epoch, args.warmup_epochs * per_epoch

    cfg = SegConfig(backbone=str(args.backbone), task="segmentation", num_classes=args.num_classes, rank=args.rank, alpha=args.alpha, lr=args.lr,
                    epochs=args.epochs, batch_size=args.batch_size, input_format=args.input_format, scale_aware=scale_aware,
                    train_samples=len(train_ds), val_samples=len(val_ds), seed=args.seed, unfreeze_blocks=args.unfreeze_blocks,
                    backbone_lr=args.backbone_lr if args.unfreeze_blocks > 0 else None, ce_weight=args.ce_weight, dice_weight=args.dice_weight,
                    dice_c0=c0, ignore_index=args.ignore_index, boundary_weight=w_bd, boundary_ramp_epochs=ramp, boundary_units=units)
    if patch["patch_train"]:
        cfg.patch_train, cfg.patch_size, cfg.patch_fg_prob, cfg.patch_rotate_deg = True, tile, patch["patch_fg_prob"], patch["patch_rotate_deg"]
        cfg.patch_scale, cfg.patches_per_epoch, cfg.patch_val = [lo, hi], per_epoch * args.batch_size, patch["patch_val"]
    higher = args.es_metric != "loss"
    best, stale, t0, best_pred = (-math.inf if higher else math.inf), 0, time.time(), None
    for epoch in range(1, args.epochs + 1):
        bd = (boundary_weight(w_bd, ramp, epoch - 1), w_bd) if w_bd > 0 else None     # (this epoch's training weight, validation's)
        if patch["patch_train"]:
            tr = train_epoch_patches(model, pool, patch_gen, per_epoch, args.batch_size, draw, opt, lambda s: fl.lr_factor(s, warm, steps), device,
                                     scale_aware, amp, args.ce_weight, args.dice_weight, c0, bd[0] if bd else 0.0, mm)
        else:
            tr = train_epoch(model, train_loader, opt, lambda s: fl.lr_factor(s, warm, steps), device, scale_aware, amp, args.ce_weight,
                             args.dice_weight, c0, *(bd[:1] if bd else ()))
        if patch["patch_val"] == "tiled":
            vl, metrics, counts, preds = validate_tiled(model, val_planes, tile, args.batch_size, device, amp, c0)
        else:
            vl, metrics, counts, preds = validate(model, val_loader, device, scale_aware, amp, args.ce_weight, args.dice_weight, c0,
                                                  *(bd[1:] if bd else ()))
        cfg.train_loss_history.append(tr)
        log.info("epoch %d/%d  train %.4f  %s", epoch, args.epochs, tr, "  ".join(f"{k} {v:.4f}" for k, v in metrics.items()))
        cur = metrics[args.es_metric] if higher else vl
        if (cur > best) if higher else (cur < best):
            best, stale, best_pred = cur, 0, preds
            cfg.best_epoch, cfg.best_val_loss, cfg.best_val_metrics = epoch, vl, metrics
            cfg.best_dice_per_class = SG.dice_per_class(counts).tolist()
            save_segmenter(model, vit, args.output, cfg)
        else:
            stale += 1
            if stale >= args.patience:
                log.info("no improvement for %d epochs: stopping at epoch %d", stale, epoch)
                break
    log.info("done in %.1f s: best epoch %d, val loss %.4f", time.time() - t0, cfg.best_epoch, cfg.best_val_loss)
    if fit_t and best_pred is not None:             # (no checkpoint was written if no epoch ever improved, e.g. a NaN loss)
        fit = fit_and_store_temperature(args.backbone, Path(args.output), val_loader, device, scale_aware, amp)
        return {"config": cfg, "val_pred": best_pred, "val_dataset": val_ds, "temperature_fit": fit}
    return {"config": cfg, "val_pred": best_pred, "val_dataset": val_ds}


def main(argv=None) -> SegConfig:
    args = parse_cli(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)s] %(message)s", datefmt="%H:%M:%S")
    return run(args)["config"]


if __name__ == "__main__":
    main()
