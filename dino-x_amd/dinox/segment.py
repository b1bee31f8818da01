"""Dense segmentation on the patch tokens: a linear head per patch, the full-resolution loss and prediction in csrc/segloss.hip.

    model = SegModel(backbone, SegHead(backbone.dim, num_classes))
    total, ce, dice = ops.SegLossFn.apply(model(x, spacing), labels_u8, 1.0, 1.0, 0)       # training
    label_map = segment(model, hu_slice, pixel_spacing, slice_thickness)                    # inference, uint8 (S, S)

The head's [B, P, C] logits are all that exists in memory; the upsampling to S = g * patch happens inside the loss / predict kernels.
``load_segmenter`` puts back what scripts/finetune_segmentation.py wrote.  The metric helpers take the int64 counts [3, C] of
``ops.seg_predict`` (true positives, predicted pixels, labelled pixels per class, over the valid pixels); ``surface_metrics`` and
``SurfaceAccumulator`` turn ``ops.surface_stats`` (csrc/surfdist.hip) into HD95 / ASSD / surface Dice in mm, ``surface_metrics_3d`` does
the same for one volume from ``ops.surface_stats_3d`` (csrc/surfdist3d.hip); ``postprocess`` cleans a
label map by connected components and ``lesion_metrics`` / ``LesionAccumulator`` turn ``ops.lesion_counts`` (csrc/cclabel.hip) into
lesion-wise sensitivity, precision, F1 and false positives per image.  For a whole series: ``segment_volume`` (one trip to the device,
the chunk loop of ``zoo.encode.encode_volume``), ``postprocess_volume`` and ``ops.lesion_counts_3d`` on 3-D components
(csrc/cclabel3d.hip), ``resample_labels_nearest`` for the ground truth and ``CaseAccumulator`` for per-case scores.  All of the above
label the model's S x S grid; ``segment_tiled`` / ``segment_volume_tiled`` (dinox/tiled.py, csrc/segblend.hip) label the image's own
grid by sliding window.  How far the probabilities can be trusted: ``ops.seg_calib`` (csrc/segcalib.hip) gives confidence and entropy
maps (``segment(..., return_confidence=True)``), ``calibration_report`` / ``CalibrationAccumulator`` turn its integer histogram into
ECE, NLL and Brier score, and ``fit_temperature`` fits ``SegModel.temperature``.  Contours that follow the image below the patch scale:
``segment(..., refine=RefineConfig())`` / ``segment_volume(..., refine=...)`` run ``ops.seg_refine`` (csrc/segrefine.hip), a few mean-field
iterations of a local CRF guided by the slice's own normalised plane, on the calibrated probabilities and before any clean-up.  The
defaults of ``RefineConfig`` are untuned on real data.
"""
from __future__ import annotations

import dataclasses
import json
import math
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


@dataclasses.dataclass(frozen=True)
class RefineConfig:
    """The seven parameters of ``ops.seg_refine`` (include/dinox.h has the definition): mean-field iterations, window radius and
    dilation, the spatial sigma in pixels of the label grid, the appearance sigma in units of the guide (the backbone's normalised input),
    the share of the appearance term in a pairwise weight and the weight of the message against the logits.  The defaults are those of
    the op; none has been tuned on real data."""
    iters: int = 5
    radius: int = 2
    dilation: int = 2
    sigma_xy: float = 3.0
    sigma_i: float = 0.5
    mix: float = 0.8
    weight: float = 4.0

    def __post_init__(self) -> None:
        for name, lo, hi in (("iters", 0, ops.SEG_REFINE_MAX_ITERS), ("radius", 1, ops.SEG_REFINE_MAX_RADIUS), ("dilation", 1, ops.SEG_REFINE_MAX_DILATION)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
                raise ValueError(f"RefineConfig: {name} must be an integer in [{lo}, {hi}], got {v!r}")
        for name, ok, say in (("sigma_xy", lambda v: 0 < v < math.inf, "finite and > 0"), ("sigma_i", lambda v: 0 < v < math.inf, "finite and > 0"),
                              ("mix", lambda v: 0 <= v <= 1, "in [0, 1]"), ("weight", lambda v: 0 <= v < math.inf, "finite and >= 0")):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not ok(v):
                raise ValueError(f"RefineConfig: {name} must be {say}, got {v!r}")
            object.__setattr__(self, name, float(v))

    def to_dict(self) -> dict:
        return dataclasses.asdict(self)

    @classmethod
    def from_dict(cls, d: dict) -> "RefineConfig":
        unknown = sorted(set(d) - {f.name for f in dataclasses.fields(cls)})
        if unknown:
            raise ValueError(f"RefineConfig: unknown field(s) {unknown}")
        return cls(**d)


def _check_refine(who: str, refine, return_entropy: bool) -> None:
    if refine is None:
        return
    if not isinstance(refine, RefineConfig):
        raise ValueError(f"{who}: refine must be None or a RefineConfig, got {type(refine).__name__}")
    if return_entropy:
        raise ValueError(f"{who}: return_entropy is not available with refine (the refinement kernel has no entropy output)")


def _refine_chunk(model, logits: torch.Tensor, x: torch.Tensor, refine: RefineConfig, want_conf: bool):
    """(pred, conf or None) of ``ops.seg_refine`` on a batch's patch logits; the guide is channel 1 of the normalised input x [n, 3, S, S]."""
    pred, conf, _ = ops.seg_refine(logits, x[:, 1].float().contiguous(), model.patch, inv_temperature=1.0 / _temperature(model),
                                   want_conf=want_conf, **refine.to_dict())
    return pred, conf


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
        # softmax temperature of the confidence / entropy maps (fit_temperature); never applied in forward: the logits stay as they are
        self.temperature = 1.0
        # the stored RefineConfig of finetune_config.json, or None; never applied implicitly: pass it as segment(..., refine=model.refine)
        self.refine = None

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
            device: Union[str, torch.device, None] = None, preprocess: Literal["host", "device", "auto"] = "host",
            keep_largest: bool = False, min_area_mm2: float = 0.0, connectivity: int = 8, return_confidence: bool = False,
            return_entropy: bool = False, refine: Optional[RefineConfig] = None):
    """Label map of one image: uint8 (S, S) with S = model.img_size, the arg-max of the upsampled patch logits.  Preprocessing, argument
    checking and the spacing convention are those of ``zoo.encode`` (its ``_batch``), so a stored head sees what ``encode()`` sees.
    Honours an ambient ``torch.autocast`` as ``encode`` does.

    ``keep_largest`` / ``min_area_mm2`` > 0 clean the map with ``postprocess`` before it leaves the device (with the defaults nothing
    changes).  The area is measured on the model's grid: ``pixel_spacing`` is (mm per source pixel along x, along y), as for ``encode``,
    and the h x w image is resized to S x S, so a pixel of the label map is (s_y, s_x) = (pixel_spacing[1] h / S, pixel_spacing[0] w / S) mm.

    ``return_confidence`` / ``return_entropy``: the return becomes ``(labels, conf[, entropy])`` with fp32 (S, S) maps of the winning
    class's softmax probability and of the entropy / log C, both at ``model.temperature`` and of the raw arg-max (clean-up touches the
    labels only).  One ``ops.seg_calib`` launch then gives labels and maps; the labels are the same bits either way.

    ``refine``: a ``RefineConfig`` -- the labels are ``ops.seg_refine``'s (csrc/segrefine.hip) at ``inv_temperature = 1 /
    model.temperature``, taken BEFORE the clean-up.  The guide is channel 1 of the normalised stack ``zoo.encode._batch`` hands the
    backbone: the centre plane of a 3-plane input, the image itself otherwise (the three channels of a 2-D image differ only by the
    ImageNet constants), so ``sigma_i`` is in units of that channel, (windowed value - 0.456) / 0.224.  ``return_confidence`` then returns
    the refined confidence; ``return_entropy`` is refused.  With ``refine=None`` nothing changes."""
    _check_refine("segment", refine, return_entropy)
    from zoo.encode import _batch
    if device is None:
        device = next(model.parameters()).device
    x = _batch([image], model.img_size, input_format, hu_level, hu_width, device, preprocess)
    spacing = None
    if model.scale_aware:
        spacing = torch.tensor([[pixel_spacing[0], pixel_spacing[1], slice_thickness]], dtype=torch.float32, device=device)
    with torch.no_grad():
        logits = model(x, spacing=spacing)
    maps = ()
    if refine is not None:
        pred, conf = _refine_chunk(model, logits, x, refine, return_confidence)
        maps = (conf,) if return_confidence else ()
    elif return_confidence or return_entropy:
        res = ops.seg_calib(logits, model.patch, inv_temperature=1.0 / _temperature(model), want_conf=return_confidence,
                            want_entropy=return_entropy)
        pred, maps = res.pred, tuple(m for m in (res.conf, res.entropy) if m is not None)
    else:
        pred = ops.seg_predict(logits, model.patch)
    if keep_largest or min_area_mm2 > 0:
        arr = np.asarray(image)
        h, w = arr.shape[1:] if arr.ndim == 3 and arr.shape[2] != 3 else arr.shape[:2]
        S = model.img_size
        pred = postprocess(pred, model.head.num_classes, [[pixel_spacing[1] * h / S, pixel_spacing[0] * w / S]], keep_largest=keep_largest,
                           min_area_mm2=min_area_mm2, connectivity=connectivity)
    if maps:
        return (pred[0].cpu().numpy(),) + tuple(m[0].cpu().numpy() for m in maps)
    return pred[0].cpu().numpy()


def _temperature(model) -> float:
    """model.temperature as a finite float > 0 (1.0 for a model that carries none)."""
    t = float(getattr(model, "temperature", 1.0))
    if not (t > 0 and math.isfinite(t)):
        raise ValueError(f"the segmenter's temperature must be finite and > 0, got {t!r}")
    return t


def segment_volume(model: SegModel, volume: np.ndarray, spacing: Tuple[float, float, float] = (1.0, 1.0, 1.0), *,
                   input_format: Literal["hu_float", "hu16_png", "windowed_float"] = "hu_float", hu_level: float = 40.0, hu_width: float = 400.0,
                   context: Literal["neighbours", "replicate"] = "neighbours", batch_size: int = 64,
                   device: Union[str, torch.device, None] = None, keep_largest: bool = False, min_volume_mm3: float = 0.0,
                   connectivity: int = 26, return_confidence: bool = False, return_entropy: bool = False,
                   refine: Optional[RefineConfig] = None):
    """Label volume of a ``(Z, H, W)`` series: uint8 (Z, S, S) with S = model.img_size.  The volume crosses to the device once and is
    preprocessed and forwarded in chunks of ``batch_size`` slices exactly as ``zoo.encode.encode_volume`` does it (``context``: the 2.5D
    stack of a slice); every chunk's patch logits go through ``ops.seg_predict`` into one device buffer, which is copied back once.
    ``spacing = (sx, sy, sz)`` in mm holds for the whole series.  Honours an ambient ``torch.autocast`` as ``segment`` does.

    ``keep_largest`` / ``min_volume_mm3`` > 0 clean the volume with ``postprocess_volume`` (3-D components, ``connectivity`` 6, 18 or 26)
    before it leaves the device.  The voxel of the label grid follows ``segment``'s convention: the h x w planes are resized to S x S, so
    it measures (s_z, s_y, s_x) = (spacing[2], spacing[1] h / S, spacing[0] w / S) mm.

    ``return_confidence`` / ``return_entropy``: as for ``segment`` -- the return becomes ``(labels, conf[, entropy])`` with fp32 (Z, S, S)
    maps at ``model.temperature``, from one ``ops.seg_calib`` launch per chunk in place of ``ops.seg_predict`` (the same label bits).

    ``refine``: as for ``segment`` -- every chunk goes through ``ops.seg_refine`` before ``postprocess_volume``, each slice guided by its own
    plane: channel 1 of the chunk's 2.5D stacks, which is plane z in both contexts (``dinox.preprocess.stack_planes``).  Slices do not
    exchange messages, so the result does not depend on ``batch_size``, and the workspace is that of one chunk."""
    _check_refine("segment_volume", refine, return_entropy)
    from zoo.encode import forward_volume_chunks
    min_component_vox(min_volume_mm3)               # refuses a negative or non-finite volume before any work is done
    if connectivity not in (6, 18, 26):
        raise ValueError(f"segment_volume: connectivity must be 6, 18 or 26, got {connectivity!r}")
    want_maps = return_confidence or return_entropy
    inv_t = 1.0 / _temperature(model) if want_maps else 1.0
    S, out, conf, ent = model.img_size, None, None, None
    for ch, logits, x in forward_volume_chunks(model, volume, spacing, input_format=input_format, hu_level=hu_level, hu_width=hu_width,
                                               context=context, z_stride=1, batch_size=batch_size, device=device, with_input=True):
        if out is None:
            Z = np.asarray(volume).shape[0]
            out = torch.empty((Z, S, S), dtype=torch.uint8, device=logits.device)
            conf = torch.empty((Z, S, S), dtype=torch.float32, device=logits.device) if return_confidence else None
            ent = torch.empty((Z, S, S), dtype=torch.float32, device=logits.device) if return_entropy else None
        sl = slice(ch[0], ch[0] + len(ch))
        if refine is not None:
            out[sl], c = _refine_chunk(model, logits, x, refine, return_confidence)
            if conf is not None:
                conf[sl] = c
        elif want_maps:
            res = ops.seg_calib(logits, model.patch, inv_temperature=inv_t, want_conf=return_confidence, want_entropy=return_entropy)
            out[sl] = res.pred
            if conf is not None:
                conf[sl] = res.conf
            if ent is not None:
                ent[sl] = res.entropy
        else:
            out[sl] = ops.seg_predict(logits, model.patch)
    if keep_largest or min_volume_mm3 > 0:
        _, h, w = np.asarray(volume).shape
        out = postprocess_volume(out, model.head.num_classes, (spacing[2], spacing[1] * h / S, spacing[0] * w / S), keep_largest=keep_largest,
                                 min_volume_mm3=min_volume_mm3, connectivity=connectivity)
    if want_maps:
        return (out.cpu().numpy(),) + tuple(m.cpu().numpy() for m in (conf, ent) if m is not None)
    return out.cpu().numpy()


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


# ------------------------------------------------------------------------------------------ boundary metrics from ops.surface_stats
def _surface_metrics(c: torch.Tensor, v: torch.Tensor, diag: torch.Tensor) -> dict:
    """The metrics of float64 host counts [B, C, 2, 1 + T] and values [B, C, 2, 3]; ``diag`` [B] is what a one-sided class scores."""
    diag = diag[:, None].expand(-1, c.shape[1])
    nA, nG = c[:, :, 0, 0], c[:, :, 1, 0]
    absent, one = (nA == 0) & (nG == 0), (nA == 0) != (nG == 0)
    den = (nA + nG).clamp(min=1)
    nan = torch.full_like(den, float("nan"))

    def pick(x):
        return torch.where(absent, nan, torch.where(one, diag, x))

    nsd = (c[:, :, 0, 1:] + c[:, :, 1, 1:]) / den[..., None]
    nsd = torch.where(absent[..., None], nan[..., None], torch.where(one[..., None], torch.zeros_like(nsd), nsd))
    return {"hd95": pick(torch.maximum(v[:, :, 0, 2], v[:, :, 1, 2])), "hd": pick(torch.maximum(v[:, :, 0, 1], v[:, :, 1, 1])),
            "assd": pick((v[:, :, 0, 0] + v[:, :, 1, 0]) / den), "nsd": nsd}


def surface_metrics(counts, values, spacing, shape) -> dict:
    """HD95, HD, ASSD and NSD per image and class from ``ops.surface_stats``'s outputs: counts [B, C, 2, 1 + T], values [B, C, 2, 3],
    spacing [B, 2] = (s_y, s_x) in mm per pixel, shape = (H, W) of the label maps.  Returns float64 tensors on the host:
    {"hd95", "hd", "assd": [B, C], "nsd": [B, C, T]} ("hd95" is whatever quantile surface_stats was asked for; 95/100 by default).
    A class with neither border in an image is absent there: NaN.  A class with exactly one (missed or hallucinated) takes the image
    diagonal sqrt((s_y H)^2 + (s_x W)^2) for the distance metrics and 0 for NSD."""
    c, v = torch.as_tensor(counts).double().cpu(), torch.as_tensor(values).double().cpu()
    if c.dim() != 4 or c.shape[2] != 2 or c.shape[3] < 2 or v.shape != c.shape[:3] + (3,):
        raise ValueError(f"surface_metrics: counts must be [B, C, 2, 1 + T] and values [B, C, 2, 3], got {tuple(c.shape)} and {tuple(v.shape)}")
    sp = torch.as_tensor(spacing).double().cpu()
    if sp.shape != (c.shape[0], 2):
        raise ValueError(f"surface_metrics: spacing must be [{c.shape[0]}, 2] = (s_y, s_x), got {tuple(sp.shape)}")
    H, W = shape
    return _surface_metrics(c, v, torch.sqrt((sp[:, 0] * H) ** 2 + (sp[:, 1] * W) ** 2))


def surface_metrics_3d(counts, values, spacing, shape) -> dict:
    """HD95, HD, ASSD and NSD per class of ONE volume from ``ops.surface_stats_3d``'s outputs: counts [C, 2, 1 + T], values [C, 2, 3],
    spacing = (s_z, s_y, s_x) in mm per voxel, shape = (Z, H, W) of the label volumes.  Returns float64 tensors on the host in the layout
    ``SurfaceAccumulator.update`` takes, the volume as one "image": {"hd95", "hd", "assd": [1, C], "nsd": [1, C, T]}.  The rules are
    ``surface_metrics``': a class absent from both volumes is NaN; a class in exactly one takes the VOLUME diagonal
    sqrt((s_z Z)^2 + (s_y H)^2 + (s_x W)^2) for the distance metrics and 0 for NSD."""
    c, v = torch.as_tensor(counts).double().cpu(), torch.as_tensor(values).double().cpu()
    if c.dim() != 3 or c.shape[1] != 2 or c.shape[2] < 2 or v.shape != c.shape[:2] + (3,):
        raise ValueError(f"surface_metrics_3d: counts must be [C, 2, 1 + T] and values [C, 2, 3], got {tuple(c.shape)} and {tuple(v.shape)}")
    sp = torch.as_tensor(spacing, dtype=torch.float64).cpu()     # (a tuple of Python floats stays float64)
    if sp.shape != (3,) or len(tuple(shape)) != 3:
        raise ValueError(f"surface_metrics_3d: spacing must be (s_z, s_y, s_x) and shape (Z, H, W), got {tuple(sp.shape)} and {shape!r}")
    ext = sp * torch.tensor([float(n) for n in shape], dtype=torch.float64)
    return _surface_metrics(c[None], v[None], torch.sqrt((ext ** 2).sum())[None])


class SurfaceAccumulator:
    """Per-class dataset means of ``surface_metrics``' per-image figures over a stream of batches.  A class's score is the mean over the
    images in which it is not absent; ``result()`` reports that number of images beside it (a class absent everywhere scores NaN over 0)."""

    def __init__(self, num_classes: int, num_tolerances: int) -> None:
        self.C, self.T = num_classes, num_tolerances
        self.images = torch.zeros(num_classes, dtype=torch.int64)
        self.sums = {"hd95": torch.zeros(num_classes, dtype=torch.float64), "hd": torch.zeros(num_classes, dtype=torch.float64),
                     "assd": torch.zeros(num_classes, dtype=torch.float64), "nsd": torch.zeros((num_classes, num_tolerances), dtype=torch.float64)}

    def update(self, metrics: dict) -> None:
        hd = metrics["hd95"]
        if hd.dim() != 2 or hd.shape[1] != self.C or metrics["nsd"].shape != hd.shape + (self.T,):
            raise ValueError(f"SurfaceAccumulator: expected [B, {self.C}] metrics with {self.T} tolerance(s), got {tuple(hd.shape)} and "
                             f"{tuple(metrics['nsd'].shape)}")
        present = ~torch.isnan(hd)
        self.images += present.sum(0)
        for k, s in self.sums.items():
            s += torch.nan_to_num(metrics[k].double(), nan=0.0).sum(0)

    def result(self) -> dict:
        """{"hd95", "hd", "assd": [C], "nsd": [C, T], "images": int64 [C]}: float64 means, NaN where a class was in no image."""
        n = self.images.double()
        out = {k: torch.where((n > 0).reshape([-1] + [1] * (s.dim() - 1)), s / n.clamp(min=1).reshape([-1] + [1] * (s.dim() - 1)),
                              torch.full_like(s, float("nan"))) for k, s in self.sums.items()}
        out["images"] = self.images.clone()
        return out


# ------------------------------------------------------------------------------------------ components: clean-up and lesion-wise metrics
def min_component_px(min_area_mm2: float, spacing, B: int) -> list:
    """min_px[b] = ceil(min_area_mm2 / (s_y s_x)) per image, in float64 on the host: the smallest pixel count whose area reaches
    ``min_area_mm2``.  ``spacing``: [B, 2] = (s_y, s_x) in mm per pixel of the label map (one pair serves every image; None: 1 mm)."""
    a = float(min_area_mm2)
    if not (a >= 0 and math.isfinite(a)):
        raise ValueError(f"min_area_mm2 must be finite and >= 0, got {min_area_mm2!r}")
    sp = torch.ones((B, 2), dtype=torch.float64) if spacing is None else torch.as_tensor(spacing).double().cpu()
    if sp.shape == (2,):
        sp = sp[None].expand(B, 2)
    if sp.shape != (B, 2) or not bool((torch.isfinite(sp) & (sp > 0)).all()):
        raise ValueError(f"spacing must be [{B}, 2] = (s_y, s_x) in mm per pixel, finite and > 0, got {spacing!r}")
    px = [math.ceil(a / (float(s[0]) * float(s[1]))) for s in sp]
    if max(px) >= 1 << 31:
        raise ValueError(f"min_area_mm2 = {a} is {max(px)} pixels at this spacing: no map is that large")
    return px


def postprocess(label_map: torch.Tensor, num_classes: int, spacing=None, *, keep_largest: bool = False, min_area_mm2: float = 0.0,
                connectivity: int = 8) -> torch.Tensor:
    """The usual clean-up of uint8 label maps [B, H, W] on the device (``ops.cc_filter``, csrc/cclabel.hip): per image and class >= 1 drop
    the connected components under ``min_area_mm2`` and, with ``keep_largest``, every component but the largest (equal areas: the one
    whose first pixel comes first in raster order); dropped pixels become background (0), the background itself is left alone.
    ``spacing`` is the (s_y, s_x) mm per pixel of the label map's grid that ``surface_metrics`` takes, [B, 2] (one pair serves all
    images, None means 1 mm): a component is kept iff its pixel count >= min_px[b] = ceil(min_area_mm2 / (s_y s_x)), computed in
    float64 on the host, i.e. iff its area in mm^2 reaches ``min_area_mm2`` (0 removes nothing)."""
    if not isinstance(label_map, torch.Tensor) or label_map.dim() != 3:
        raise ValueError(f"postprocess: label_map must be uint8 [B, H, W], got {type(label_map).__name__}")
    return ops.cc_filter(label_map, num_classes, min_px=min_component_px(min_area_mm2, spacing, label_map.shape[0]), keep_largest=keep_largest,
                         connectivity=connectivity)


def min_component_vox(min_volume_mm3: float, voxel_mm=None) -> int:
    """ceil(min_volume_mm3 / (s_z s_y s_x)) in float64 on the host: the smallest voxel count whose volume reaches ``min_volume_mm3``.
    ``voxel_mm``: (s_z, s_y, s_x) in mm per voxel of the label volume (None: 1 mm)."""
    v = float(min_volume_mm3)
    if not (v >= 0 and math.isfinite(v)):
        raise ValueError(f"min_volume_mm3 must be finite and >= 0, got {min_volume_mm3!r}")
    sp = torch.ones(3, dtype=torch.float64) if voxel_mm is None else torch.as_tensor(voxel_mm).double().cpu()
    if sp.shape != (3,) or not bool((torch.isfinite(sp) & (sp > 0)).all()):
        raise ValueError(f"voxel_mm must be (s_z, s_y, s_x) in mm per voxel, finite and > 0, got {voxel_mm!r}")
    vox = math.ceil(v / (float(sp[0]) * float(sp[1]) * float(sp[2])))
    if vox >= 1 << 31:
        raise ValueError(f"min_volume_mm3 = {v} is {vox} voxels at this spacing: no volume is that large")
    return vox


def postprocess_volume(label_volume: torch.Tensor, num_classes: int, voxel_mm=None, *, keep_largest: bool = False, min_volume_mm3: float = 0.0,
                       connectivity: int = 26) -> torch.Tensor:
    """``postprocess`` for one uint8 label volume [Z, H, W] on the device (``ops.cc_filter_3d``, csrc/cclabel3d.hip): per class >= 1 drop
    the 3-D connected components under ``min_volume_mm3`` and, with ``keep_largest``, every component but the largest of the whole volume
    (equal counts: the one whose first voxel comes first); dropped voxels become background (0).  ``voxel_mm`` is the (s_z, s_y, s_x) mm
    per voxel of the label grid (None: 1 mm): a component is kept iff its voxel count >= ``min_component_vox(min_volume_mm3, voxel_mm)``."""
    if not isinstance(label_volume, torch.Tensor) or label_volume.dim() != 3:
        raise ValueError(f"postprocess_volume: label_volume must be uint8 [Z, H, W], got {type(label_volume).__name__}")
    return ops.cc_filter_3d(label_volume, num_classes, min_vox=min_component_vox(min_volume_mm3, voxel_mm), keep_largest=keep_largest,
                            connectivity=connectivity)


def resample_labels_nearest(labels_zhw, S: int) -> np.ndarray:
    """Ground truth (Z, H, W) on the model's S x S grid, slice by slice: output pixel (i, j) takes source pixel
    (min(floor((i + 0.5) H / S), H - 1), min(floor((j + 0.5) W / S), W - 1)).  No value is ever mixed, so 255 (ignore) is preserved."""
    lab = np.asarray(labels_zhw)
    if lab.ndim != 3 or lab.dtype != np.uint8 or min(lab.shape) < 1:
        raise ValueError(f"resample_labels_nearest: labels must be uint8 (Z, H, W), got {lab.dtype} {lab.shape}")
    if int(S) != S or S < 1:
        raise ValueError(f"resample_labels_nearest: S must be an integer >= 1, got {S!r}")
    _, H, W = lab.shape
    iy = np.minimum(((2 * np.arange(S, dtype=np.int64) + 1) * H) // (2 * int(S)), H - 1)     # floor((i + 0.5) H / S) in integers
    ix = np.minimum(((2 * np.arange(S, dtype=np.int64) + 1) * W) // (2 * int(S)), W - 1)
    return np.ascontiguousarray(lab[:, iy[:, None], ix[None, :]])


LESION_COUNTS = ("n_gt", "n_gt_hit", "n_pred", "n_pred_hit")


def lesion_metrics(counts, images: Optional[int] = None) -> dict:
    """Lesion-wise detection scores from ``ops.lesion_counts``' int64 [B, C, 4] = (n_gt, n_gt_hit, n_pred, n_pred_hit): summed over the
    images, then per class sensitivity n_gt_hit / n_gt, precision n_pred_hit / n_pred, F1 2 P R / (P + R) and false positives per image
    (n_pred - n_pred_hit) / images, float64 [C] on the host, NaN where the denominator is 0; beside them the four summed counts (int64
    [C]) and "images".  Counts already summed, [C, 4], need ``images``."""
    c = torch.as_tensor(counts).cpu()
    if c.dim() == 3 and c.shape[2] == 4 and images is None:
        images = c.shape[0]
    if c.dim() == 3 and c.shape[2] == 4:
        c = c.sum(0)
    if c.dim() != 2 or c.shape[1] != 4 or images is None or c.dtype.is_floating_point:
        raise ValueError(f"lesion_metrics: counts must be integers [B, C, 4], or [C, 4] with images given, got {tuple(c.shape)} {c.dtype}")
    c = c.to(torch.int64)
    n_gt, gt_hit, n_pred, pred_hit = (c[:, i].double() for i in range(4))
    nan = torch.full_like(n_gt, float("nan"))
    sens = torch.where(n_gt > 0, gt_hit / n_gt.clamp(min=1), nan)
    prec = torch.where(n_pred > 0, pred_hit / n_pred.clamp(min=1), nan)
    den = prec + sens
    f1 = torch.where(den > 0, 2 * prec * sens / torch.where(den > 0, den, torch.ones_like(den)), nan)
    fp = (n_pred - pred_hit) / images if images > 0 else nan
    out = {"sensitivity": sens, "precision": prec, "f1": f1, "fp_per_image": fp, "images": int(images)}
    out.update({k: c[:, i].clone() for i, k in enumerate(LESION_COUNTS)})
    return out


class LesionAccumulator:
    """Sums ``ops.lesion_counts`` over a stream of batches; ``result()`` is ``lesion_metrics`` of the whole set."""

    def __init__(self, num_classes: int) -> None:
        self.C, self.images = num_classes, 0
        self.counts = torch.zeros((num_classes, 4), dtype=torch.int64)

    def update(self, counts) -> None:
        c = torch.as_tensor(counts).cpu()
        if c.dim() != 3 or tuple(c.shape[1:]) != (self.C, 4) or c.dtype.is_floating_point:
            raise ValueError(f"LesionAccumulator: expected integer counts [B, {self.C}, 4], got {tuple(c.shape)} {c.dtype}")
        self.counts += c.to(torch.int64).sum(0)
        self.images += c.shape[0]

    def result(self) -> dict:
        return lesion_metrics(self.counts, images=self.images)


class CaseAccumulator:
    """Scores over cases (volumes).  Per case: the overlap counts [3, C] of ``ops.cc_filter_3d(..., targets=)`` / ``ops.seg_predict`` summed
    over the case, and the lesion counts [C, 4] of ``ops.lesion_counts_3d``.  ``result()``: "dice" = per class the mean of the per-case
    Dice over the cases where the class occurs in the prediction or the labels (NaN where in none), "cases" = that number of cases per
    class (int64 [C]), and "lesions" = ``lesion_metrics`` of the summed lesion counts with images = the number of cases, so its
    "fp_per_image" is false positives per case."""

    def __init__(self, num_classes: int) -> None:
        self.C, self.n = num_classes, 0
        self.dice_sum = torch.zeros(num_classes, dtype=torch.float64)
        self.cases = torch.zeros(num_classes, dtype=torch.int64)
        self.lesions = torch.zeros((num_classes, 4), dtype=torch.int64)

    def update(self, counts, lesion_counts) -> None:
        c, l = torch.as_tensor(counts).cpu(), torch.as_tensor(lesion_counts).cpu()
        if tuple(c.shape) != (3, self.C) or tuple(l.shape) != (self.C, 4) or c.dtype.is_floating_point or l.dtype.is_floating_point:
            raise ValueError(f"CaseAccumulator: expected integer counts [3, {self.C}] and lesion counts [{self.C}, 4], got {tuple(c.shape)} {c.dtype} "
                             f"and {tuple(l.shape)} {l.dtype}")
        present = (c[1] + c[2]) > 0
        self.dice_sum += torch.where(present, dice_per_class(c), torch.zeros(self.C, dtype=torch.float64))
        self.cases += present.to(torch.int64)
        self.lesions += l.to(torch.int64)
        self.n += 1

    def result(self) -> dict:
        n = self.cases.double()
        dice = torch.where(n > 0, self.dice_sum / n.clamp(min=1), torch.full_like(n, float("nan")))
        return {"dice": dice, "cases": self.cases.clone(), "lesions": lesion_metrics(self.lesions, images=self.n)}


# ------------------------------------------------------------------------------------------ calibration (ops.seg_calib, csrc/segcalib.hip)
Q_ONE = 1 << 24                                     # the histogram's confidences are integers in units of 2^-24


def calibration_report(hist, tail, sums) -> dict:
    """Scores from ``ops.seg_calib``'s integers and sums (CPU or device tensors, arrays or lists; no GPU needed): ``hist`` [NB, 3] = per
    bin (count, correct, Q), ``tail`` [3] = (valid pixels, bad labels, non-finite), ``sums`` [5] = (NLL, Brier, G, H, entropy) totals.
    Every quotient is one float64 division of exact integers (the sums: of float64 values), so e.g. a table whose bins have
    correct 2^24 = Q scores ece == 0 exactly.

    {"bins": [{"count", "accuracy" = correct / count, "mean_confidence" = Q / (2^24 count)} or None for an empty bin],
     "ece" = sum_k (count_k / N) |acc_k - conf_k|, "mce" = the largest gap over the non-empty bins, "nll", "brier", "mean_entropy" (sums / N),
     "accuracy", "mean_confidence", "pixels" = N = valid - non-finite, "nonfinite"}; with N = 0 every score is None."""
    rows = [[int(v) for v in r] for r in (hist.tolist() if hasattr(hist, "tolist") else hist)]
    nv, _, nonfinite = (int(v) for v in (tail.tolist() if hasattr(tail, "tolist") else tail))
    sm = [float(v) for v in (sums.tolist() if hasattr(sums, "tolist") else sums)]
    if any(len(r) != 3 for r in rows) or len(sm) != 5:
        raise ValueError("calibration_report: hist must be [NB, 3] and sums [5]")
    N = nv - nonfinite
    if N != sum(r[0] for r in rows):
        raise ValueError(f"calibration_report: the bins hold {sum(r[0] for r in rows)} pixels, the tail says {nv} - {nonfinite}")
    bins = [None if n == 0 else {"count": n, "accuracy": k / n, "mean_confidence": q / (Q_ONE * n)} for n, k, q in rows]
    out = {"bins": bins, "pixels": N, "nonfinite": nonfinite}
    if N == 0:
        out.update(dict.fromkeys(("ece", "mce", "nll", "brier", "mean_entropy", "accuracy", "mean_confidence")))
        return out
    gaps = [abs(k * Q_ONE - q) for n, k, q in rows]                              # |acc_k - conf_k| count_k 2^24, an integer
    out.update(ece=sum(gaps) / (Q_ONE * N), mce=max(gp / (Q_ONE * n) for gp, (n, _, _) in zip(gaps, rows) if n),
               nll=sm[0] / N, brier=sm[1] / N, mean_entropy=sm[4] / N, accuracy=sum(r[1] for r in rows) / N,
               mean_confidence=sum(r[2] for r in rows) / (Q_ONE * N))
    return out


class CalibrationAccumulator:
    """Dataset totals of ``ops.seg_calib`` results over a stream of batches: the histogram in int64, the sums in float64."""

    def __init__(self, bins: int = 15) -> None:
        self.bins = bins
        self.hist = torch.zeros((bins, 3), dtype=torch.int64)
        self.tail = torch.zeros(3, dtype=torch.int64)
        self.sums = torch.zeros(5, dtype=torch.float64)

    def update(self, result) -> None:
        if result.hist is None or tuple(result.hist.shape) != (self.bins, 3):
            raise ValueError(f"CalibrationAccumulator: expected a seg_calib result with labels and {self.bins} bins")
        self.hist += result.hist.cpu()
        self.tail += result.tail.cpu()
        self.sums += result.sums.double().cpu()

    def result(self) -> dict:
        return calibration_report(self.hist, self.tail, self.sums)


def fit_temperature(batches, u: int, *, lo: float = 0.05, hi: float = 20.0, tol: float = 1e-4, max_iter: int = 30, calib=None) -> dict:
    """The temperature T in [lo, hi] that minimises the total NLL of softmax(l / T) over ``batches``, a list of (z, labels) pairs of device
    tensors (patch logits [B, g^2, C] and uint8 labels [B, S, S] of a validation set), by safeguarded Newton on theta = log s, s = 1 / T.

    One pass = one ``ops.seg_calib`` launch per batch (``want_pred=False``: nothing of full resolution is written) and one read of its
    five sums; G = dNLL/ds and H = d2NLL/ds2 are added over the batches in float64.  d/dtheta = s G and d2/dtheta2 = s G + s^2 H, so the
    step is -(s G) / (s G + s^2 H); the sign of G keeps a bracket (NLL is convex in s) and its midpoint replaces a step that leaves the
    bracket or has a denominator <= 0.  Stops once |step| < tol (the step is still taken).

    -> {"temperature", "iterations", "nll_before" (mean NLL at T = 1), "nll_after", "converged"}; without a valid pixel
    {"temperature": 1.0, "converged": False, ...}.  ``calib``: what to call instead of ``ops.seg_calib`` (tests)."""
    calib = calib or ops.seg_calib
    if not (0 < lo < hi and math.isfinite(hi)):
        raise ValueError(f"fit_temperature: need 0 < lo < hi < inf, got {lo!r}, {hi!r}")
    if not (tol > 0 and max_iter >= 1):
        raise ValueError(f"fit_temperature: need tol > 0 and max_iter >= 1, got {tol!r}, {max_iter!r}")
    batches = list(batches)

    def totals(s: float, want_n: bool = False):
        t, n = np.zeros(5), 0
        for z, y in batches:
            r = calib(z, u, y, inv_temperature=s, want_pred=False)
            t += r.sums.double().cpu().numpy()
            if want_n:
                tl = r.tail.cpu()
                n += int(tl[0]) - int(tl[2])
        return t, n

    first, N = totals(1.0, True)
    if N == 0:
        return {"temperature": 1.0, "iterations": 0, "nll_before": None, "nll_after": None, "converged": False}
    a, b = -math.log(hi), math.log(1.0 / lo)        # the bracket of theta = log s
    theta, t, converged, it = min(max(0.0, a), b), first, False, 0
    if theta != 0.0:
        t, _ = totals(math.exp(theta))
    while it < max_iter:
        it += 1
        s = math.exp(theta)
        grad, den = s * t[2], s * t[2] + s * s * t[3]
        if grad > 0:
            b = theta
        else:
            a = theta
        new = theta - grad / den if den > 0 else None
        if new is None or not a < new < b:
            new = 0.5 * (a + b)
        step, theta = new - theta, new
        t, _ = totals(math.exp(theta))
        if abs(step) < tol:
            converged = True
            break
    return {"temperature": math.exp(-theta), "iterations": it, "nll_before": float(first[0]) / N, "nll_after": float(t[0]) / N,
            "converged": converged}


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
    if "temperature" in cfg:                        # --fit-temperature's result: used by the confidence / entropy maps only
        model.temperature = float(cfg["temperature"])
        _temperature(model)
    if "refine" in cfg:                             # stored, never applied implicitly
        model.refine = RefineConfig.from_dict(cfg["refine"])
    return model.eval()


# ------------------------------------------------------------------------------------------ sliding-window inference at native resolution
from dinox.tiled import blend_window, segment_tiled, segment_volume_tiled, tile_plan, tile_starts  # noqa: E402,F401
