"""Sliding-window segmentation at native resolution: overlapping tiles, a window-weighted blend of their logits, optional mirror
averaging (nnU-Net's ``predict_sliding_window``, MONAI's ``sliding_window_inference``).

    labels = segment_volume_tiled(model, hu_volume, (sx, sy, sz), overlap=0.5, tta_flips=True)      # uint8 (Z, H, W): the scanner's grid
    label_map = segment_tiled(model, hu_slice, (sx, sy), sz)                                        # uint8 (H, W)

A tile is a crop job of the preprocessing kernel (``preprocess.volume_tile_jobs``), so tiles of any side are resized to the model's
S x S as every image is; their [g^2, C] patch logits are all that is kept, and ``ops.seg_blend_predict`` (csrc/segblend.hip) turns
them into the label map: every pixel gathers the tiles that cover it, nothing is upsampled into memory and nothing is scattered.
``tile_starts`` and ``blend_window`` are the host side of the definitions in include/dinox.h; everything here but the launches runs
without a GPU.
"""
from __future__ import annotations

import math
from typing import List, Literal, Optional, Tuple, Union

import numpy as np
import torch

from dinox import ops

WINDOWS = ("gaussian", "constant")
FLIP_CODES = (0, 1, 2, 3)                           # bit 0: mirrored along x, bit 1: along y
_F32_MIN_NORMAL = float(np.finfo(np.float32).tiny)


def tile_starts(L: int, t: int, overlap: float = 0.5) -> List[int]:
    """Origins of the tiles of side t along an axis of length L >= t: step = max(1, round(t (1 - overlap))), n = ceil((L - t) / step) + 1
    tiles spread evenly from 0 to L - t (the integer nearest to i (L - t) / (n - 1), halves up), as nnU-Net does it.  Consecutive
    origins are at most ``step`` <= t apart, so every pixel is covered."""
    if isinstance(L, bool) or isinstance(t, bool) or int(L) != L or int(t) != t or not 1 <= t <= L:
        raise ValueError(f"tile_starts: integers with 1 <= t <= L expected, got L = {L!r}, t = {t!r}")
    if not 0.0 <= overlap < 1.0:
        raise ValueError(f"tile_starts: overlap must lie in [0, 1), got {overlap!r}")
    L, t = int(L), int(t)
    if L == t:
        return [0]
    step = max(1, int(round(t * (1.0 - overlap))))
    n = -(-(L - t) // step) + 1
    return [(2 * i * (L - t) + (n - 1)) // (2 * (n - 1)) for i in range(n)]


def blend_window(t: int, kind: str = "gaussian", sigma_scale: float = 0.125) -> np.ndarray:
    """The 1-D blend window, fp32 [t]; tile pixel (ly, lx) weighs win[ly] win[lx].  "constant": ones.  "gaussian":
    exp(-d^2 / (2 sigma^2)) with d measured from the centre (t - 1) / 2 and sigma = sigma_scale t, computed in float64 and rounded
    once.  A window whose smallest weight product win[0]^2 is not a normal fp32 number (a pixel could end up with no weight at all) is
    refused."""
    if isinstance(t, bool) or int(t) != t or t < 1:
        raise ValueError(f"blend_window: t must be an integer >= 1, got {t!r}")
    if kind not in WINDOWS:
        raise ValueError(f"Unknown window: '{kind}'. Supported: 'gaussian', 'constant'")
    if kind == "constant":
        return np.ones(int(t), dtype=np.float32)
    if not (sigma_scale > 0 and math.isfinite(sigma_scale)):
        raise ValueError(f"blend_window: sigma_scale must be finite and > 0, got {sigma_scale!r}")
    d = np.arange(int(t), dtype=np.float64) - (int(t) - 1) / 2.0
    w = np.exp(-(d * d) / (2.0 * (float(sigma_scale) * int(t)) ** 2)).astype(np.float32)
    if float(w.min()) == 0.0 or float(w.min()) ** 2 < _F32_MIN_NORMAL:
        raise ValueError(f"blend_window: sigma_scale = {sigma_scale} leaves a weight of {float(w.min())!r} at the edge of a tile of {t}: "
                         "its products are zero in fp32")
    return w


def tile_plan(model, H: int, W: int, tile: Optional[int], overlap: float, window: str, tta_flips: bool, sigma_scale: float = 0.125) -> dict:
    """What a tiled call does on an H x W plane: {"tile", "ys", "xs", "win", "flips"}.  ``tile`` None: min(model.img_size, H, W); a given
    side is clamped to min(H, W)."""
    if tile is not None and (isinstance(tile, bool) or int(tile) != tile or tile < 1):
        raise ValueError(f"tile must be an integer >= 1 or None, got {tile!r}")
    if min(H, W) < 1:
        raise ValueError(f"Unsupported plane shape: {(H, W)}")
    t = min(model.img_size if tile is None else int(tile), H, W)
    return {"tile": t, "ys": tile_starts(H, t, overlap), "xs": tile_starts(W, t, overlap), "win": blend_window(t, window, sigma_scale),
            "flips": list(FLIP_CODES) if tta_flips else [0]}


def _flipped(x: torch.Tensor, code: int) -> torch.Tensor:
    dims = [d for d, bit in ((-1, 1), (-2, 2)) if code & bit]
    return x.flip(dims) if dims else x


def _tiled_labels(model, vol: np.ndarray, spacing, plan: dict, input_format: str, hu_level: float, hu_width: float, context: str,
                  batch_size: int, device, labels: Optional[torch.Tensor] = None, want_conf: bool = False, inv_temperature: float = 1.0):
    """uint8 [Z, H, W] on the device: the tiles of every slice in the order (z, iy, ix), ``batch_size`` at a time through the
    preprocessing kernel and the model (every mirror variant a device-side flip of the same preprocessed batch); their logits wait
    in a buffer of a few slices, and each time whole slices are complete one ``ops.seg_blend_predict`` launch labels them.
    ``labels`` (uint8 [Z, H, W] on the device, 255 = ignore): returns (label volume, counts int64 [3, C]), the blend launches' own
    counts added up.  ``want_conf`` (without ``labels``): returns (label volume, fp32 [Z, H, W] confidence of the blend kernel, the
    max-softmax of the blended logits); ``inv_temperature`` != 1 scales the tile logits by it before each blend launch -- the blend is
    linear in them, so this is the blended logit over T -- and the labels are then that launch's (they can differ from an unscaled run's
    at exact fp32 near-ties).  With 1 nothing is scaled."""
    from dinox import preprocess as P
    if want_conf and labels is not None:
        raise ValueError("_tiled_labels: want_conf goes without labels")
    Z, H, W = vol.shape
    S, g = model.img_size, model.img_size // model.patch
    C = model.head.num_classes
    t, ys, xs, flips = plan["tile"], plan["ys"], plan["xs"], plan["flips"]
    ny, nx, F = len(ys), len(xs), len(flips)
    n_t = ny * nx
    items = [(z, y0, x0) for z in range(Z) for y0 in ys for x0 in xs]
    bounds = list(range(0, len(items), batch_size)) + [len(items)]
    tables = [P.volume_tile_jobs(Z, H, W, items[a:b], t, context) for a, b in zip(bounds[:-1], bounds[1:])]
    for tb, a, b in zip(tables, bounds[:-1], bounds[1:]):
        P.check_jobs(tb, Z * H * W, b - a)
    src_dtype = P.source_dtype(vol)
    host = np.ascontiguousarray(vol, dtype=np.dtype(src_dtype))
    src = torch.from_numpy(host.view(np.int16) if src_dtype == "uint16" else host).reshape(-1).to(device)
    jobs = torch.from_numpy(np.concatenate(tables, 0)).pin_memory().to(device, non_blocking=True)
    xbuf = torch.empty((min(batch_size, len(items)), 3, S, S), dtype=torch.float32, device=device)
    sp = torch.tensor([list(spacing)], dtype=torch.float32, device=device) if model.scale_aware else None
    G = -(-batch_size // n_t) + 1                    # slices a batch can touch, a partial one on either side included
    zbuf = torch.empty((G, F, n_t, g * g, C), dtype=torch.float32, device=device)
    out = torch.empty((Z, H, W), dtype=torch.uint8, device=device)
    done, at = 0, 0                                 # slices labelled so far (= the slice in zbuf[0]); rows of `jobs` consumed
    counts = None if labels is None else torch.zeros((3, C), dtype=torch.int64, device=device)
    conf = None
    for tb, a, b in zip(tables, bounds[:-1], bounds[1:]):
        n = b - a
        x = P.device_preprocess(src, jobs[at:at + len(tb)], n, S, input_format, hu_level, hu_width, out=xbuf[:n], src_dtype=src_dtype,
                                max_side=t)
        at += len(tb)
        for f, code in enumerate(flips):
            with torch.no_grad():
                logits = model(_flipped(x, code).contiguous() if code else x, spacing=None if sp is None else sp.expand(n, 3).contiguous())
            k = a
            while k < b:                            # the batch's tiles, slice by slice
                zi, j = divmod(k, n_t)
                m = min(b - k, n_t - j)
                zbuf[zi - done, f, j:j + m] = logits[k - a:k - a + m]
                k += m
        full = b // n_t - done                      # whole slices now complete
        if full > 0:
            zfull = zbuf[:full].view(full, F, ny, nx, g * g, C)
            if want_conf:
                if conf is None:
                    conf = torch.empty((Z, H, W), dtype=torch.float32, device=device)
                out[done:done + full], conf[done:done + full] = ops.seg_blend_predict(
                    zfull if inv_temperature == 1.0 else zfull * inv_temperature, ys, xs, flips, plan["win"], H, W, t, want_conf=True)
            elif labels is None:
                out[done:done + full] = ops.seg_blend_predict(zfull, ys, xs, flips, plan["win"], H, W, t)
            else:
                out[done:done + full], cnt = ops.seg_blend_predict(zfull, ys, xs, flips, plan["win"], H, W, t, labels=labels[done:done + full])
                counts += cnt
            if b % n_t:                             # the slice under way moves to the front
                zbuf[0, :, :b % n_t] = zbuf[full, :, :b % n_t].clone()
            done += full
    assert done == Z
    if want_conf:
        return out, conf
    return out if labels is None else (out, counts)


def tiled_label_counts(model, planes: np.ndarray, labels: np.ndarray, spacing: Tuple[float, float, float] = (1.0, 1.0, 1.0), *,
                       tile: Optional[int] = None, overlap: float = 0.5, window: str = "gaussian", batch_size: int = 64,
                       device: Union[str, torch.device, None] = None):
    """Tiled validation of images of ONE size: ``planes`` fp32 (n, H, W), already windowed to [0, 1] ("windowed_float"), each labelled on
    its own grid as ``segment_tiled`` labels it, against ``labels`` uint8 (n, H, W) (255 = ignore).  Returns (label maps uint8 (n, H, W)
    on the host, counts int64 [3, C] on the device: the blend kernel's true positives, predicted and labelled pixels per class)."""
    vol, lab = np.asarray(planes, dtype=np.float32), np.asarray(labels)
    if vol.ndim != 3 or lab.shape != vol.shape or lab.dtype != np.uint8:
        raise ValueError(f"tiled_label_counts: planes {vol.shape} and uint8 labels {lab.dtype} {lab.shape} must be equal (n, H, W) stacks")
    device = _check_common(model, vol, "windowed_float", "replicate", batch_size, device)
    plan = tile_plan(model, vol.shape[1], vol.shape[2], tile, overlap, window, False)
    out, counts = _tiled_labels(model, vol, spacing, plan, "windowed_float", 0.0, 1.0, "replicate", int(batch_size), device,
                                labels=torch.from_numpy(lab).to(device))
    return out.cpu().numpy(), counts


def _check_common(model, vol: np.ndarray, input_format: str, context: str, batch_size: int, device):
    from dinox import preprocess as P
    if vol.ndim != 3 or min(vol.shape) < 1:
        raise ValueError(f"Unsupported volume shape: {vol.shape}. Expected (Z, H, W).")
    if input_format not in P.FORMATS:
        raise ValueError(f"Unknown input_format: '{input_format}'. Supported: 'hu_float', 'hu16_png', 'windowed_float'")
    if context not in P.CONTEXTS:
        raise ValueError(f"Unknown context: '{context}'. Supported: 'neighbours', 'replicate'")
    if isinstance(batch_size, bool) or int(batch_size) != batch_size or batch_size < 1:
        raise ValueError(f"batch_size must be an integer >= 1, got {batch_size}")
    if device is None:
        device = next(model.parameters()).device
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"dinox: tiled segmentation needs a CUDA/HIP device, not '{device}' -- the kernel library is the only compute path.")
    return device


def segment_volume_tiled(model, volume: np.ndarray, spacing: Tuple[float, float, float] = (1.0, 1.0, 1.0), *, tile: Optional[int] = None,
                         overlap: float = 0.5, window: Literal["gaussian", "constant"] = "gaussian", tta_flips: bool = False,
                         sigma_scale: float = 0.125, input_format: Literal["hu_float", "hu16_png", "windowed_float"] = "hu_float",
                         hu_level: float = 40.0, hu_width: float = 400.0, context: Literal["neighbours", "replicate"] = "neighbours",
                         batch_size: int = 64, device: Union[str, torch.device, None] = None, keep_largest: bool = False,
                         min_volume_mm3: float = 0.0, connectivity: int = 26, return_confidence: bool = False):
    """Label volume of a ``(Z, H, W)`` series on ITS OWN grid: uint8 (Z, H, W).  Every slice is cut into tiles of side t (``tile``; None:
    min(model.img_size, H, W); clamped to min(H, W)) at ``tile_starts`` along both axes, each tile's 2.5D stack (``context``) goes
    through the preprocessing kernel -- which resizes a tile of side t != S to S x S as it does any image -- and the model,
    ``batch_size`` tiles at a time; ``tta_flips`` adds the three mirrored variants.  The tile logits are blended under ``window``
    (``blend_window``) and arg-maxed by ``ops.seg_blend_predict``.  The volume crosses to the device once and only the label volume comes
    back.  ``spacing = (sx, sy, sz)`` in mm is the series' own and is what a scale-aware model is told, as ``segment`` does.  Honours an
    ambient ``torch.autocast``.

    ``keep_largest`` / ``min_volume_mm3`` > 0 clean the volume with ``postprocess_volume``; nothing was resized, so the voxel is the
    scanner's: (s_z, s_y, s_x) = (spacing[2], spacing[1], spacing[0]).

    ``return_confidence``: returns (labels, fp32 (Z, H, W) max-softmax of the blended logits at ``model.temperature``).  With a stored
    temperature T != 1 the tile logits are divided by T before the blend launch and the labels are that launch's: they can differ from a
    run without the flag at exact fp32 near-ties.  With T = 1 the labels are the same bits."""
    from dinox.segment import _temperature, min_component_vox, postprocess_volume
    min_component_vox(min_volume_mm3)
    if connectivity not in (6, 18, 26):
        raise ValueError(f"segment_volume_tiled: connectivity must be 6, 18 or 26, got {connectivity!r}")
    vol = np.asarray(volume)
    device = _check_common(model, vol, input_format, context, batch_size, device)
    plan = tile_plan(model, vol.shape[1], vol.shape[2], tile, overlap, window, tta_flips, sigma_scale)
    conf = None
    if return_confidence:
        out, conf = _tiled_labels(model, vol, spacing, plan, input_format, hu_level, hu_width, context, int(batch_size), device, want_conf=True,
                                  inv_temperature=1.0 / _temperature(model))
    else:
        out = _tiled_labels(model, vol, spacing, plan, input_format, hu_level, hu_width, context, int(batch_size), device)
    if keep_largest or min_volume_mm3 > 0:
        out = postprocess_volume(out, model.head.num_classes, (spacing[2], spacing[1], spacing[0]), keep_largest=keep_largest,
                                 min_volume_mm3=min_volume_mm3, connectivity=connectivity)
    return (out.cpu().numpy(), conf.cpu().numpy()) if return_confidence else out.cpu().numpy()


def segment_tiled(model, image: np.ndarray, pixel_spacing: Tuple[float, float] = (1.0, 1.0), slice_thickness: float = 1.0, *,
                  tile: Optional[int] = None, overlap: float = 0.5, window: Literal["gaussian", "constant"] = "gaussian",
                  tta_flips: bool = False, sigma_scale: float = 0.125,
                  input_format: Literal["hu_float", "hu16_png", "windowed_float"] = "hu_float", hu_level: float = 40.0, hu_width: float = 400.0,
                  batch_size: int = 64, device: Union[str, torch.device, None] = None, keep_largest: bool = False, min_area_mm2: float = 0.0,
                  connectivity: int = 8) -> np.ndarray:
    """Label map of one (H, W) image on its own grid: uint8 (H, W); ``segment_volume_tiled`` of the one-slice series with
    ``context="replicate"`` (the plane in all three channels, as ``segment`` shows a single-channel image).  ``keep_largest`` /
    ``min_area_mm2`` clean the map with ``postprocess`` at the real pixel (s_y, s_x) = (pixel_spacing[1], pixel_spacing[0])."""
    from dinox.segment import min_component_px, postprocess
    arr = np.asarray(image)
    if arr.ndim != 2:
        raise ValueError(f"segment_tiled: a single-channel (H, W) image expected, got {arr.shape}")
    min_component_px(min_area_mm2, None, 1)
    device = _check_common(model, arr[None], input_format, "replicate", batch_size, device)
    plan = tile_plan(model, arr.shape[0], arr.shape[1], tile, overlap, window, tta_flips, sigma_scale)
    out = _tiled_labels(model, arr[None], (pixel_spacing[0], pixel_spacing[1], slice_thickness), plan, input_format, hu_level, hu_width,
                        "replicate", int(batch_size), device)
    if keep_largest or min_area_mm2 > 0:
        out = postprocess(out, model.head.num_classes, [[pixel_spacing[1], pixel_spacing[0]]], keep_largest=keep_largest,
                          min_area_mm2=min_area_mm2, connectivity=connectivity)
    return out[0].cpu().numpy()
