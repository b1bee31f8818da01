#!/usr/bin/env python3
"""Supervised LoRA fine-tuning of a DINO-X backbone on the HIP engine (the reference's scripts/finetune_lora.py flag surface).

    python scripts/finetune_lora.py --backbone runs/x/hub-export/ --train-csv train.csv --val-csv val.csv \\
        --task classification --num-classes 2 --rank 8 --epochs 50 --output adapters/x/
    python scripts/finetune_lora.py --backbone runs/x/hub-export/ --synthetic 64 --epochs 3 --output /tmp/a     # no data needed

CSV columns: image_path,label[,spacing_x,spacing_y,spacing_z].  One image per row, replicated to three channels.
The backbone runs through zoo.peft (csrc/lora.hip beside the base GEMMs), the head is the engine's Linear, the optimiser is the fused
dinox_adamw pass over one flat arena per learning-rate group; the loss on the [B, C] logits is framework code.  Written to --output
whenever the early-stopping metric improves: the adapter (adapter_config.json, adapter_model.safetensors), head.pth,
finetune_config.json and, with --unfreeze-blocks, unfrozen_blocks.pth.
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
from dataclasses import asdict, dataclass, field
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

_PKG = Path(__file__).resolve().parent.parent
if str(_PKG) not in sys.path:
    sys.path.insert(0, str(_PKG))

from dinox import ops  # noqa: E402
from zoo.arch import Linear  # noqa: E402
from zoo.hub import load_model  # noqa: E402
from zoo.peft import apply_lora, count_parameters, save_adapter  # noqa: E402

log = logging.getLogger("finetune_lora")

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ------------------------------------------------------------------------------------------ records
@dataclass
class LabeledRow:
    image_path: Path
    label: float
    spacing: Tuple[float, float, float] = (1.0, 1.0, 1.0)
    has_spacing: bool = False


@dataclass
class FinetuneConfig:
    """What finetune_config.json records beside the adapter."""
    backbone: str
    task: str
    num_classes: int
    rank: int
    alpha: float
    lr: float
    epochs: int
    batch_size: int
    input_format: str
    scale_aware: bool
    best_epoch: int = 0
    best_val_loss: float = float("inf")
    best_val_metrics: Dict[str, float] = field(default_factory=dict)
    train_samples: int = 0
    val_samples: int = 0
    seed: Optional[int] = None
    unfreeze_blocks: int = 0
    backbone_lr: Optional[float] = None
    train_loss_history: List[float] = field(default_factory=list)


def read_csv(path: Path) -> List[LabeledRow]:
    with open(path, newline="") as f:
        rd = csv.DictReader(f)
        cols = rd.fieldnames or []
        lacking = {"image_path", "label"} - set(cols)
        if lacking:
            raise ValueError(f"{path}: column(s) {sorted(lacking)} missing (found {cols})")
        sp = all(c in cols for c in ("spacing_x", "spacing_y", "spacing_z"))
        rows = []
        for n, rec in enumerate(rd, 2):
            try:
                spacing = tuple(float(rec[c]) for c in ("spacing_x", "spacing_y", "spacing_z")) if sp else (1.0, 1.0, 1.0)
                rows.append(LabeledRow(Path(rec["image_path"]), float(rec["label"]), spacing, sp))
            except (TypeError, ValueError) as e:
                raise ValueError(f"{path}, line {n}: {e}") from e
    return rows


# ------------------------------------------------------------------------------------------ image transforms as tensor code
def _resize(x: torch.Tensor, h: int, w: int) -> torch.Tensor:
    if x.shape[-2:] == (h, w):
        return x
    return F.interpolate(x[None], size=(h, w), mode="bicubic", align_corners=False, antialias=True)[0]


def resize_center_crop(x: torch.Tensor, size: int) -> torch.Tensor:
    """Shorter side to ``size`` (bicubic), then the central size x size window."""
    h, w = x.shape[-2:]
    k = size / min(h, w)
    x = _resize(x, max(size, round(h * k)), max(size, round(w * k)))
    h, w = x.shape[-2:]
    t, l = (h - size) // 2, (w - size) // 2
    return x[:, t:t + size, l:l + size]


def random_resized_crop(x: torch.Tensor, size: int, gen: torch.Generator, scale=(0.7, 1.0), ratio=(3 / 4, 4 / 3)) -> torch.Tensor:
    """A window of ``scale`` of the area and log-uniform aspect ``ratio`` (ten tries, then the centre crop), resized to size x size."""
    h, w = x.shape[-2:]
    for _ in range(10):
        area = h * w * float(torch.empty(1).uniform_(scale[0], scale[1], generator=gen))
        asp = math.exp(float(torch.empty(1).uniform_(math.log(ratio[0]), math.log(ratio[1]), generator=gen)))
        cw, ch = int(round(math.sqrt(area * asp))), int(round(math.sqrt(area / asp)))
        if 0 < cw <= w and 0 < ch <= h:
            t = int(torch.randint(0, h - ch + 1, (1,), generator=gen))
            l = int(torch.randint(0, w - cw + 1, (1,), generator=gen))
            return _resize(x[:, t:t + ch, l:l + cw], size, size)
    return resize_center_crop(x, size)


def normalize(x: torch.Tensor) -> torch.Tensor:
    return (x - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)


class LabeledImages(torch.utils.data.Dataset):
    """(image [3, S, S], spacing [3], label) per row; ``augment`` adds the random-resized crop and the horizontal flip."""

    def __init__(self, rows: List[LabeledRow], img_size: int, input_format: str = "hu16_png", window_level: float = 40.0,
                 window_width: float = 400.0, augment: bool = False, data_root: Optional[Path] = None, seed: int = 0) -> None:
        if input_format not in ("hu16_png", "float01"):
            raise ValueError(f"unknown input format {input_format!r}")
        self.rows, self.img_size, self.fmt, self.augment, self.root = rows, img_size, input_format, augment, data_root
        self.level, self.width = window_level, window_width
        self.gen = torch.Generator().manual_seed(seed)

    def __len__(self) -> int:
        return len(self.rows)

    def pixels(self, row: LabeledRow) -> torch.Tensor:
        """One channel in [0, 1], [H, W]."""
        from PIL import Image
        p = row.image_path if row.image_path.is_absolute() or self.root is None else self.root / row.image_path
        a = np.asarray(Image.open(p), dtype=np.float32)
        if a.ndim == 3:
            a = a[..., 0]
        if self.fmt == "hu16_png":                    # stored value = 10 HU + 32768; window to [0, 1]
            a = ((a - 32768.0) * 0.1 - (self.level - self.width / 2.0)) / max(self.width, 1.0)
        elif a.max() > 1.0:
            a = a / 255.0
        return torch.from_numpy(np.clip(a, 0.0, 1.0))

    def transform(self, x: torch.Tensor) -> torch.Tensor:
        if self.augment:
            x = random_resized_crop(x, self.img_size, self.gen)
            if float(torch.rand(1, generator=self.gen)) < 0.5:
                x = x.flip(-1)
        else:
            x = resize_center_crop(x, self.img_size)
        return normalize(x).contiguous()

    def __getitem__(self, i: int):
        row = self.rows[i]
        x = self.pixels(row)[None].expand(3, -1, -1)
        return self.transform(x), torch.tensor(row.spacing, dtype=torch.float32), row.label


class SyntheticStacks(LabeledImages):
    """``n`` seeded stacks whose label can be read off the pixels: noise in [0, 1] plus a label-dependent brightness step between the upper
    and the lower half (unchanged by the horizontal flip).  Classification: label i mod C; regression: uniform in [-1, 1]."""

    def __init__(self, n: int, img_size: int, task: str, num_classes: int, seed: int, first: int = 0, augment: bool = False) -> None:
        super().__init__([], img_size, "float01", augment=augment, seed=seed + 1 + first)
        g = torch.Generator().manual_seed(seed * 7919 + 13)
        total = first + n
        noise = torch.rand((total, 1, img_size, img_size), generator=g)
        labels = (torch.arange(total) % max(num_classes, 1)).float() if task == "classification" else torch.rand(total, generator=g) * 2 - 1
        level = labels / max(num_classes - 1, 1) * 2 - 1 if task == "classification" else labels
        half = torch.ones(img_size)
        half[img_size // 2:] = -1.0
        img = (0.5 + 0.25 * (noise - 0.5) + 0.25 * level.view(-1, 1, 1, 1) * half.view(1, 1, -1, 1)).clamp(0, 1)
        self.images, self.labels = img[first:], labels[first:]
        self.spacings = 0.5 + torch.rand((total, 3), generator=g)[first:]

    def __len__(self) -> int:
        return self.images.shape[0]

    def __getitem__(self, i: int):
        return self.transform(self.images[i].expand(3, -1, -1)), self.spacings[i], float(self.labels[i])


# ------------------------------------------------------------------------------------------ model, metrics
class FinetuneModel(nn.Module):
    """LoRA-wrapped backbone and a linear head on its CLS feature; the head is stored apart from the adapter (head.pth)."""

    def __init__(self, backbone: nn.Module, dim: int, num_classes: int, task: str = "classification") -> None:
        super().__init__()
        self.backbone, self.task = backbone, task
        self.head = Linear(dim, 1 if task == "regression" else num_classes)

    def forward(self, x: torch.Tensor, spacing: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self.head(self.backbone(x, spacing=spacing)[:, 0], out_dtype=torch.float32)


def auroc(scores: torch.Tensor, targets: torch.Tensor) -> float:
    """Mann-Whitney form: (sum of the positives' ranks - n+ (n+ + 1) / 2) / (n+ n-), tied scores sharing their mean rank; 0.5 when one
    class is absent."""
    s = scores.double().numpy()
    pos = targets.numpy() == 1
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    if n_pos == 0 or n_neg == 0:
        return 0.5
    order = np.argsort(s, kind="stable")
    ss = s[order]
    start = np.r_[0, np.flatnonzero(ss[1:] != ss[:-1]) + 1]           # first position of each run of equal scores
    stop = np.r_[start[1:], len(ss)]
    mean_rank = (start + 1 + stop) / 2.0                              # ranks start+1 .. stop
    ranks = np.empty(len(s))
    ranks[order] = np.repeat(mean_rank, stop - start)
    return float((ranks[pos].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


def compute_metrics(preds: torch.Tensor, targets: torch.Tensor, task: str, num_classes: int) -> Dict[str, float]:
    """classification: accuracy, macro_f1 over the classes present in ``targets`` (C > 1), auroc (C == 2, softmax score of class 1);
    regression: mse, rmse, r2 (0 for a constant target)."""
    preds, targets = preds.detach().float().cpu(), targets.detach().cpu()
    out: Dict[str, float] = {}
    if task == "classification":
        targets = targets.long()
        hard = preds.argmax(-1)
        out["accuracy"] = float((hard == targets).float().mean()) if len(targets) else 0.0
        if num_classes == 2:
            out["auroc"] = auroc(torch.softmax(preds, -1)[:, 1], targets)
        if num_classes > 1:
            f1 = []
            for c in range(num_classes):
                if not (targets == c).any():
                    continue
                tp = float(((hard == c) & (targets == c)).sum())
                fp = float(((hard == c) & (targets != c)).sum())
                fn = float(((hard != c) & (targets == c)).sum())
                prec, rec = tp / (tp + fp + 1e-8), tp / (tp + fn + 1e-8)
                f1.append(2 * prec * rec / (prec + rec + 1e-8))
            out["macro_f1"] = float(np.mean(f1)) if f1 else 0.0
    elif task == "regression":
        y, t = preds.reshape(-1).double(), targets.double()
        res = float(((y - t) ** 2).sum())
        tot = float(((t - t.mean()) ** 2).sum())
        out["mse"] = res / max(len(t), 1)
        out["rmse"] = math.sqrt(out["mse"])
        out["r2"] = 1.0 - res / tot if tot > 1e-8 else 0.0
    else:
        raise ValueError(f"unknown task {task!r}")
    return out


def task_loss(logits: torch.Tensor, labels: torch.Tensor, task: str) -> torch.Tensor:
    if task == "classification":
        return F.cross_entropy(logits.float(), labels.long())
    return F.mse_loss(logits.float().squeeze(-1), labels.float())


# ------------------------------------------------------------------------------------------ optimiser: fused AdamW over flat arenas
class ArenaAdamW:
    """One flat fp32 arena (parameters, gradients, both moments) per learning-rate group, stepped by ONE dinox_adamw_ema launch each
    (no teacher: no EMA).  Parameters and their .grad are re-pointed at slices of the arenas, 8-element aligned."""

    def __init__(self, groups: List[Tuple[List[nn.Parameter], float]], weight_decay: float, betas=(0.9, 0.999), eps: float = 1e-8) -> None:
        self.wd, self.betas, self.eps, self.t = weight_decay, betas, eps, 0
        self.groups = []
        for params, lr in groups:
            params = [p for p in params if p.requires_grad]
            if not params:
                continue
            offs, total = [], 0
            for p in params:
                offs.append(total)
                total += (p.numel() + 7) // 8 * 8
            dev = params[0].device
            flat, grad = torch.zeros(total, device=dev), torch.zeros(total, device=dev)
            for p, o in zip(params, offs):
                flat[o:o + p.numel()].copy_(p.data.reshape(-1))
                p.data = flat[o:o + p.numel()].view(p.shape)
                p.grad = grad[o:o + p.numel()].view(p.shape)
            self.groups.append(dict(params=params, lr=lr, p=flat, g=grad, m=torch.zeros_like(flat), v=torch.zeros_like(flat)))

    def zero_grad(self) -> None:
        for g in self.groups:
            ops.zero_(g["g"])

    def step(self, lr_factor: float) -> None:
        self.t += 1
        for g in self.groups:
            ops.adamw_ema_(g["p"], g["g"], g["m"], g["v"], None, lr=g["lr"] * lr_factor, weight_decay=self.wd, beta1=self.betas[0],
                           beta2=self.betas[1], eps=self.eps, step_t=self.t, ema=0.0)
        for g in self.groups:              # the kernel wrote these master weights behind torch's version counters; the frozen
            ops.invalidate_weights(g["params"])   # backbone's cached bf16 images stay


def lr_factor(step: int, warmup: int, total: int) -> float:
    """Linear warm-up over ``warmup`` steps (step / warmup, as the reference's LambdaLR: the very first step has factor 0), then a half
    cosine to zero."""
    if step < warmup:
        return step / max(warmup, 1)
    return 0.5 * (1.0 + math.cos(math.pi * (step - warmup) / max(total - warmup, 1)))


# ------------------------------------------------------------------------------------------ epochs, saving
def _batches(loader, device, scale_aware):
    for x, sp, y in loader:
        yield x.to(device), (sp.to(device) if scale_aware else None), torch.as_tensor(y).to(device)


def train_epoch(model, loader, opt: ArenaAdamW, sched, device, task, scale_aware, amp) -> float:
    model.train()
    tot, n = 0.0, 0
    for x, sp, y in _batches(loader, device, scale_aware):
        opt.zero_grad()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            loss = task_loss(model(x, spacing=sp), y, task)
        loss.backward()
        opt.step(sched(opt.t))
        tot, n = tot + float(loss.detach()), n + 1
    return tot / max(n, 1)


@torch.no_grad()
def validate(model, loader, device, task, num_classes, scale_aware, amp):
    """-> (mean loss, metrics, logits [n, C] on the host)."""
    model.eval()
    tot, n, logits, labels = 0.0, 0, [], []
    for x, sp, y in _batches(loader, device, scale_aware):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            out = model(x, spacing=sp)
        tot, n = tot + float(task_loss(out, y, task)), n + 1
        logits.append(out.float().cpu())
        labels.append(y.cpu())
    logits, labels = torch.cat(logits), torch.cat(labels)
    metrics = compute_metrics(logits, labels, task, num_classes)
    metrics["loss"] = tot / max(n, 1)
    return metrics["loss"], metrics, logits


def unfrozen_block_range(n_blocks: int, unfreeze: int) -> range:
    return range(n_blocks - min(max(unfreeze, 0), n_blocks), n_blocks)


def save_finetune(model: FinetuneModel, output_dir: Path, config: FinetuneConfig) -> None:
    """Adapter files, head.pth, finetune_config.json; with unfrozen blocks also unfrozen_blocks.pth ("blocks.<i>.<parameter>" -> tensor,
    adapter matrices left out: they are in the adapter file)."""
    output_dir = Path(output_dir)
    output_dir.mkdir(parents=True, exist_ok=True)
    save_adapter(model.backbone, output_dir)
    torch.save({k: v.detach().cpu().clone() for k, v in model.head.state_dict().items()}, output_dir / "head.pth")
    if config.unfreeze_blocks > 0:
        vit = model.backbone.base_model.model
        state = {}
        for i in unfrozen_block_range(len(vit.blocks), config.unfreeze_blocks):
            for name, p in vit.blocks[i].named_parameters():
                if ".lora_" not in name:
                    state[f"blocks.{i}.{name}"] = p.detach().cpu().clone()
        torch.save(state, output_dir / "unfrozen_blocks.pth")
    (output_dir / "finetune_config.json").write_text(json.dumps(asdict(config), indent=2, default=str))


# ------------------------------------------------------------------------------------------ command line
def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="LoRA fine-tuning of a DINO-X backbone", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--backbone", required=True, help="hub directory, training checkpoint (.pth) or HuggingFace id")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--train-csv", type=Path, default=None, help="required unless --synthetic")
    ap.add_argument("--val-csv", type=Path, default=None, help="required unless --synthetic")
    ap.add_argument("--synthetic", type=int, default=0, metavar="N", help="N seeded labelled stacks instead of the CSV files (3/4 train, 1/4 val)")
    ap.add_argument("--data-root", type=Path, default=None, help="prefix of relative image paths")
    ap.add_argument("--input-format", default="hu16_png", choices=["hu16_png", "float01"])
    ap.add_argument("--window-level", type=float, default=40.0, help="HU window centre (hu16_png)")
    ap.add_argument("--window-width", type=float, default=400.0, help="HU window width (hu16_png)")
    ap.add_argument("--task", default="classification", choices=["classification", "regression"])
    ap.add_argument("--num-classes", type=int, default=2)
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--alpha", type=float, default=16.0)
    ap.add_argument("--lora-dropout", type=float, default=0.05)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--weight-decay", type=float, default=0.01)
    ap.add_argument("--warmup-epochs", type=int, default=3)
    ap.add_argument("--patience", type=int, default=10, help="epochs without improvement before stopping")
    ap.add_argument("--es-metric", default="loss", help="'loss' (lower is better) or a metric name such as 'auroc' (higher is better)")
    ap.add_argument("--num-workers", type=int, default=4)
    ap.add_argument("--no-amp", action="store_true", help="fp32 mode instead of bf16 autocast")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--unfreeze-blocks", type=int, default=0, help="also train the last N transformer blocks' own weights")
    ap.add_argument("--backbone-lr", type=float, default=1e-5, help="learning rate of the unfrozen blocks")
    ap.add_argument("--output", required=True, type=Path)
    return ap


def run(args: argparse.Namespace) -> dict:
    """One fine-tuning run -> {"config": FinetuneConfig, "val_logits": the best epoch's validation logits [n, C] (host, fp32),
    "val_dataset": the validation set}."""
    ap = build_parser()
    if not args.synthetic and (args.train_csv is None or args.val_csv is None):
        ap.error("--train-csv and --val-csv are required unless --synthetic N is given")
    device = torch.device(args.device)
    amp = not args.no_amp and device.type == "cuda"
    if args.seed is not None:
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
    seed = args.seed if args.seed is not None else 0

    backbone = load_model(args.backbone, device=str(device))
    scale_aware, dim, img = backbone.scale_aware, backbone.dim, backbone.img_size
    if args.synthetic:
        n_val = max(args.synthetic // 4, 1)
        n_train = args.synthetic - n_val
        train_ds = SyntheticStacks(n_train, img, args.task, args.num_classes, seed, first=0, augment=True)
        val_ds = SyntheticStacks(n_val, img, args.task, args.num_classes, seed, first=n_train, augment=False)
        workers = 0
    else:
        rows_t, rows_v = read_csv(args.train_csv), read_csv(args.val_csv)
        if args.task == "classification":
            top = max(int(r.label) for r in rows_t + rows_v)
            if top >= args.num_classes:
                ap.error(f"label {top} does not fit --num-classes {args.num_classes}")
        if scale_aware and not rows_t[0].has_spacing:
            log.warning("scale-aware backbone, but the CSV has no spacing_x/y/z columns: 1 mm is assumed everywhere")
        kw = dict(input_format=args.input_format, window_level=args.window_level, window_width=args.window_width, data_root=args.data_root)
        train_ds = LabeledImages(rows_t, img, augment=True, seed=seed + 1, **kw)
        val_ds = LabeledImages(rows_v, img, augment=False, **kw)
        workers = args.num_workers
    gen = torch.Generator().manual_seed(seed)
    train_loader = torch.utils.data.DataLoader(train_ds, batch_size=args.batch_size, shuffle=True, drop_last=True, num_workers=workers,
                                               generator=gen)
    val_loader = torch.utils.data.DataLoader(val_ds, batch_size=args.batch_size, shuffle=False, num_workers=workers)
    if len(train_loader) == 0:
        ap.error(f"{len(train_ds)} training samples do not fill one batch of {args.batch_size}")

    backbone = apply_lora(backbone, rank=args.rank, alpha=args.alpha, dropout=args.lora_dropout)
    vit = backbone.base_model.model
    base_params: List[nn.Parameter] = []
    for i in unfrozen_block_range(len(vit.blocks), args.unfreeze_blocks):
        for p in vit.blocks[i].parameters():
            if not p.requires_grad:
                p.requires_grad = True
                base_params.append(p)
    model = FinetuneModel(backbone, dim, args.num_classes, args.task).to(device)
    base_ids = {id(p) for p in base_params}
    fast = [p for p in backbone.parameters() if p.requires_grad and id(p) not in base_ids] + list(model.head.parameters())
    counts = count_parameters(backbone)
    log.info("backbone %d parameters, %d adapter + %d unfrozen trainable; head %d", counts["total"],
             counts["trainable"] - sum(p.numel() for p in base_params), sum(p.numel() for p in base_params),
             sum(p.numel() for p in model.head.parameters()))
    opt = ArenaAdamW([(fast, args.lr), (base_params, args.backbone_lr)], args.weight_decay)
    steps, warm = args.epochs * len(train_loader), args.warmup_epochs * len(train_loader)

    cfg = FinetuneConfig(backbone=str(args.backbone), task=args.task, num_classes=args.num_classes, rank=args.rank, alpha=args.alpha,
                         lr=args.lr, epochs=args.epochs, batch_size=args.batch_size, input_format=args.input_format, scale_aware=scale_aware,
                         train_samples=len(train_ds), val_samples=len(val_ds), seed=args.seed, unfreeze_blocks=args.unfreeze_blocks,
                         backbone_lr=args.backbone_lr if args.unfreeze_blocks > 0 else None)
    higher = args.es_metric != "loss"
    best, stale, t0, best_logits = (-math.inf if higher else math.inf), 0, time.time(), None
    for epoch in range(1, args.epochs + 1):
        tr = train_epoch(model, train_loader, opt, lambda s: lr_factor(s, warm, steps), device, args.task, scale_aware, amp)
        vl, metrics, logits = validate(model, val_loader, device, args.task, args.num_classes, scale_aware, amp)
        cfg.train_loss_history.append(tr)
        log.info("epoch %d/%d  train %.4f  %s", epoch, args.epochs, tr, "  ".join(f"{k} {v:.4f}" for k, v in metrics.items()))
        if higher and args.es_metric not in metrics:
            log.warning("metric %r is not computed for this task: early stopping follows the loss", args.es_metric)
            higher, best = False, math.inf
        cur = metrics[args.es_metric] if higher else vl
        if (cur > best) if higher else (cur < best):
            best, stale, best_logits = cur, 0, logits
            cfg.best_epoch, cfg.best_val_loss, cfg.best_val_metrics = epoch, vl, metrics
            save_finetune(model, args.output, cfg)
        else:
            stale += 1
            if stale >= args.patience:
                log.info("no improvement for %d epochs: stopping at epoch %d", stale, epoch)
                break
    log.info("done in %.1f s: best epoch %d, val loss %.4f", time.time() - t0, cfg.best_epoch, cfg.best_val_loss)
    return {"config": cfg, "val_logits": best_logits, "val_dataset": val_ds}


def main(argv=None) -> FinetuneConfig:
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)s] %(message)s", datefmt="%H:%M:%S")
    return run(args)["config"]


if __name__ == "__main__":
    main()
