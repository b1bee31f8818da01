"""Dense segmentation on the patch tokens: a linear head per patch, the full-resolution loss and prediction in csrc/segloss.hip.

    model = SegModel(backbone, SegHead(backbone.dim, num_classes))
    total, ce, dice = ops.SegLossFn.apply(model(x, spacing), labels_u8, 1.0, 1.0, 0)       # training
    label_map = segment(model, hu_slice, pixel_spacing, slice_thickness)                    # inference, uint8 (S, S)

The head's [B, P, C] logits are all that exists in memory; the upsampling to S = g * patch happens inside the loss / predict kernels.
``load_segmenter`` puts back what scripts/finetune_segmentation.py wrote.  The metric helpers take the int64 counts [3, C] of
``ops.seg_predict`` (true positives, predicted pixels, labelled pixels per class, over the valid pixels).
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Literal, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from dinox import ops
from zoo.arch import Linear

HEAD_FILE = "seg_head.pth"
CONFIG_FILE = "finetune_config.json"
BLOCKS_FILE = "unfrozen_blocks.pth"


class SegHead(nn.Module):
    """The engine's Linear on every patch token -> fp32 logits [B, P, C].  ``tokens`` is PatchViT.forward's [B, 1 + P + registers, dim]:
    CLS (token 0) and the registers (after the patches) are dropped."""

    def __init__(self, dim: int, num_classes: int) -> None:
        super().__init__()
        if not 2 <= num_classes <= ops.SEG_MAX_CLASSES:
            raise ValueError(f"SegHead: num_classes must lie in [2, {ops.SEG_MAX_CLASSES}], got {num_classes}")
        self.dim, self.num_classes = dim, num_classes
        self.proj = Linear(dim, num_classes)

    def forward(self, tokens: torch.Tensor, n_patches: int) -> torch.Tensor:
        return self.proj(tokens[:, 1:1 + n_patches].contiguous(), out_dtype=torch.float32)


class SegModel(nn.Module):
    """Backbone (a PatchViT, plain or LoRA-wrapped) and a SegHead; ``forward`` returns the [B, P, C] fp32 patch logits.
    ``frozen_backbone``: the backbone runs under no_grad in eval mode (the linear probe: only the head trains)."""

    def __init__(self, backbone: nn.Module, head: SegHead, frozen_backbone: bool = False) -> None:
        super().__init__()
        self.backbone, self.head, self.frozen_backbone = backbone, head, frozen_backbone

    @property
    def img_size(self) -> int:
        return self.backbone.img_size

    @property
    def patch(self) -> int:
        return self.backbone.patch

    @property
    def scale_aware(self) -> bool:
        return self.backbone.scale_aware

    def train(self, mode: bool = True):
        super().train(mode)
        if self.frozen_backbone:
            self.backbone.eval()
        return self

    def forward(self, x: torch.Tensor, spacing: Optional[torch.Tensor] = None) -> torch.Tensor:
        P = (self.img_size // self.patch) ** 2
        if self.frozen_backbone:
            with torch.no_grad():
                tokens = self.backbone(x, spacing=spacing)
        else:
            tokens = self.backbone(x, spacing=spacing)
        return self.head(tokens, P)


def segment(model: SegModel, image: np.ndarray, pixel_spacing: Tuple[float, float] = (1.0, 1.0), slice_thickness: float = 1.0, *,
            input_format: Literal["hu_float", "hu16_png", "windowed_float"] = "hu_float", hu_level: float = 40.0, hu_width: float = 400.0,
            device: Union[str, torch.device, None] = None, preprocess: Literal["host", "device", "auto"] = "host") -> np.ndarray:
    """Label map of one image: uint8 (S, S) with S = model.img_size, the arg-max of the upsampled patch logits.  Preprocessing, argument
    checking and the spacing convention are those of ``zoo.encode`` (its ``_batch``), so a stored head sees what ``encode()`` sees.
    Honours an ambient ``torch.autocast`` as ``encode`` does."""
    from zoo.encode import _batch
    if device is None:
        device = next(model.parameters()).device
    x = _batch([image], model.img_size, input_format, hu_level, hu_width, device, preprocess)
    spacing = None
    if model.scale_aware:
        spacing = torch.tensor([[pixel_spacing[0], pixel_spacing[1], slice_thickness]], dtype=torch.float32, device=device)
    with torch.no_grad():
        logits = model(x, spacing=spacing)
    return ops.seg_predict(logits, model.patch)[0].cpu().numpy()


# ------------------------------------------------------------------------------------------ metrics from the int64 counts [3, C]
def _rows(counts):
    c = torch.as_tensor(counts).double().cpu()
    if c.dim() != 2 or c.shape[0] != 3:
        raise ValueError(f"counts must be [3, C] (true positives, predicted, labelled), got {tuple(c.shape)}")
    return c[0], c[1], c[2]


def dice_per_class(counts) -> torch.Tensor:
    """2 TP / (predicted + labelled) per class, float64 [C]; 0 where a class is in neither map."""
    tp, pc, yc = _rows(counts)
    den = pc + yc
    return torch.where(den > 0, 2 * tp / den.clamp(min=1), torch.zeros_like(den))


def iou_per_class(counts) -> torch.Tensor:
    """TP / (predicted + labelled - TP) per class, float64 [C]; 0 where a class is in neither map."""
    tp, pc, yc = _rows(counts)
    den = pc + yc - tp
    return torch.where(den > 0, tp / den.clamp(min=1), torch.zeros_like(den))


def _mean_present(values: torch.Tensor, counts, skip_background: bool, empty: float) -> float:
    """Mean over the classes that occur in the prediction or the labels; a batch in which the kept classes are all absent scores
    ``empty`` -- 1 if other pixels were valid (nothing to find, nothing claimed), 0 if nothing was valid at all."""
    _, pc, yc = _rows(counts)
    keep = (pc + yc) > 0
    if skip_background:
        keep[0] = False
    return float(values[keep].mean()) if keep.any() else empty


def mean_dice(counts, skip_background: bool = False) -> float:
    return _mean_present(dice_per_class(counts), counts, skip_background, 1.0 if float(_rows(counts)[2].sum()) > 0 else 0.0)


def miou(counts, skip_background: bool = False) -> float:
    return _mean_present(iou_per_class(counts), counts, skip_background, 1.0 if float(_rows(counts)[2].sum()) > 0 else 0.0)


def pixel_accuracy(counts) -> float:
    tp, _, yc = _rows(counts)
    return float(tp.sum() / yc.sum()) if float(yc.sum()) > 0 else 0.0


# ------------------------------------------------------------------------------------------ what finetune_segmentation.py wrote
def load_segmenter(backbone_path, output_dir, device: Union[str, torch.device] = "cuda") -> SegModel:
    """Backbone from ``backbone_path`` (whatever ``zoo.hub.load_model`` takes), then from ``output_dir``: the unfrozen blocks' weights if
    any, the adapter if rank > 0, and the head.  The result is in eval mode with nothing trainable."""
    from zoo.hub import load_model
    from zoo.peft import load_adapter
    out = Path(output_dir)
    cfg = json.loads((out / CONFIG_FILE).read_text())
    if cfg.get("task") != "segmentation":
        raise ValueError(f"{out / CONFIG_FILE}: task {cfg.get('task')!r} is not 'segmentation'")
    backbone = load_model(str(backbone_path), device=str(device))
    if cfg["rank"] > 0:
        backbone = load_adapter(backbone, out)
    if (out / BLOCKS_FILE).exists():
        vit = backbone.base_model.model if cfg["rank"] > 0 else backbone
        own = dict(vit.named_parameters())
        with torch.no_grad():
            for k, v in torch.load(out / BLOCKS_FILE, map_location="cpu", weights_only=True).items():
                own[k].copy_(v.to(own[k].device))
        ops.invalidate_weights()
    head = SegHead(backbone.dim, cfg["num_classes"])
    head.load_state_dict(torch.load(out / HEAD_FILE, map_location="cpu", weights_only=True))
    model = SegModel(backbone, head, frozen_backbone=cfg["rank"] == 0 and cfg.get("unfreeze_blocks", 0) == 0).to(device)
    for p in model.parameters():
        p.requires_grad = False
    return model.eval()
