"""``zoo.encode`` surface: raw HU array + physical spacing -> features, forward on the HIP engine.

Host-side preprocessing follows the reference (zoo/encode.py:34-72,129-169): convert to HU
(``hu16_png``: (u16 - 32768) * 0.1), window to [0,1] (level 40 / width 400 by default), replicate or
split into 3 channels, PIL bilinear resize to ``model.img_size``, ImageNet normalise, spacing tensor
only for scale-aware models.  ``encode`` returns ``(1, 1, D)`` (CLS) or all tokens ``(1, N, D)``;
``ValueError`` for an unknown ``input_format``, an unsupported shape or mismatched list lengths.

``preprocess="device"`` runs the same preprocessing as ONE HIP kernel on the raw arrays (``dinox.preprocess``,
``csrc/encode_prep.hip``); ``"auto"`` tries that and falls back to the host code where the kernel declines or the model
sits on the CPU; the default ``"host"`` is the code above, unchanged.  ``encode_volume`` takes a whole ``(Z, H, W)``
series: the volume goes to the device once and every plane is resized once for the up to three 2.5D stacks it shows in.
"""
from __future__ import annotations

from typing import List, Literal, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from zoo.arch import PatchViT, cls_attention_grid, rollout_grid

_MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32).reshape(3, 1, 1)
_STD = np.array([0.229, 0.224, 0.225], dtype=np.float32).reshape(3, 1, 1)
_FORMATS = ("hu_float", "hu16_png", "windowed_float")


def _to_hu(arr: np.ndarray, input_format: str) -> np.ndarray:
    if input_format not in _FORMATS:
        raise ValueError(f"Unknown input_format: '{input_format}'. Supported: 'hu_float', 'hu16_png', 'windowed_float'")
    a = arr.astype(np.float32)
    return (a - 32768.0) * 0.1 if input_format == "hu16_png" else a


def _hu_window(arr: np.ndarray, level: float = 40.0, width: float = 400.0) -> np.ndarray:
    lo, hi = level - width / 2, level + width / 2
    return (np.clip(arr, lo, hi) - lo) / (hi - lo)


def _resize(arr: np.ndarray, size: int) -> np.ndarray:
    from PIL import Image
    return np.array(Image.fromarray(arr).resize((size, size), Image.BILINEAR))


def _channels(arr: np.ndarray) -> List[np.ndarray]:
    if arr.ndim == 2:
        return [arr, arr, arr]
    if arr.ndim == 3 and arr.shape[2] == 3:
        return [arr[:, :, i] for i in range(3)]
    if arr.ndim == 3 and arr.shape[0] == 3:
        return [arr[i] for i in range(3)]
    raise ValueError(f"Unsupported image shape: {arr.shape}. Expected (H, W), (H, W, 3), or (3, H, W).")


def preprocess(image: np.ndarray, img_size: int, input_format: str, hu_level: float, hu_width: float) -> torch.Tensor:
    """-> (3, img_size, img_size) fp32, ImageNet-normalised."""
    arr = _to_hu(image, input_format)
    if input_format != "windowed_float":
        arr = _hu_window(arr, level=hu_level, width=hu_width)
    stack = np.stack([_resize(np.ascontiguousarray(c, dtype=np.float32), img_size) for c in _channels(arr)], axis=0)
    return torch.from_numpy(((stack.astype(np.float32) - _MEAN) / _STD).astype(np.float32))


_PREPROCESS = ("host", "device", "auto")


def _batch(images: Sequence[np.ndarray], img_size: int, input_format: str, hu_level: float, hu_width: float, device,
           mode: str) -> torch.Tensor:
    """(B, 3, img_size, img_size) fp32 on ``device`` by the host code, the kernel, or the kernel where it can ("auto")."""
    if mode not in _PREPROCESS:
        raise ValueError(f"Unknown preprocess: '{mode}'. Supported: 'host', 'device', 'auto'")
    if mode == "auto" and torch.device(device).type != "cuda":
        mode = "host"
    if mode != "host":
        from dinox import preprocess as P
        if input_format not in _FORMATS:
            raise ValueError(f"Unknown input_format: '{input_format}'. Supported: 'hu_float', 'hu16_png', 'windowed_float'")
        try:
            return P.pack_and_preprocess(images, img_size, input_format, hu_level, hu_width, device)
        except P.PreprocessUnsupported:
            if mode == "device":
                raise
    return torch.stack([preprocess(im, img_size, input_format, hu_level, hu_width) for im in images], 0).to(device)


def encode(model: PatchViT, image: np.ndarray, pixel_spacing: Tuple[float, float] = (1.0, 1.0), slice_thickness: float = 1.0, *,
           input_format: Literal["hu_float", "hu16_png", "windowed_float"] = "hu_float", hu_level: float = 40.0,
           hu_width: float = 400.0, return_all_tokens: bool = False,
           device: Union[str, torch.device, None] = None,
           preprocess: Literal["host", "device", "auto"] = "host") -> torch.Tensor:
    if device is None:
        device = next(model.parameters()).device
    x = _batch([image], model.img_size, input_format, hu_level, hu_width, device, preprocess)
    spacing = None
    if model.scale_aware:
        spacing = torch.tensor([[pixel_spacing[0], pixel_spacing[1], slice_thickness]], dtype=torch.float32, device=device)
    with torch.no_grad():
        feats = model(x, spacing=spacing)
    return feats if return_all_tokens else feats[:, 0:1, :]


def attention_map(model: PatchViT, image: np.ndarray, pixel_spacing: Optional[Tuple[float, float]] = None,
                  slice_thickness: Optional[float] = None, *,
                  input_format: Literal["hu_float", "hu16_png", "windowed_float"] = "hu_float", hu_level: float = 40.0,
                  hu_width: float = 400.0, layer: int = -1, device: Union[str, torch.device, None] = None,
                  preprocess: Literal["host", "device", "auto"] = "host") -> torch.Tensor:
    """CLS attention of block ``layer`` (default: the last) over the patches of one image: ``(heads, g, g)`` fp32 on the CPU, g =
    img_size / patch.  Same preprocessing, argument checking and spacing convention as ``encode`` (spacing None = 1.0 mm; it is used
    by scale-aware models only).  Each head's map sums to 1 minus the mass that head puts on CLS and the registers.  The softmax rows
    come from ``PatchViT.last_attention`` (``csrc/attention_rows.hip``): the probabilities themselves, not a token-norm proxy."""
    if device is None:
        device = next(model.parameters()).device
    x = _batch([image], model.img_size, input_format, hu_level, hu_width, device, preprocess)
    spacing = None
    if model.scale_aware:
        sx, sy = (1.0, 1.0) if pixel_spacing is None else pixel_spacing
        spacing = torch.tensor([[sx, sy, 1.0 if slice_thickness is None else slice_thickness]], dtype=torch.float32, device=device)
    _, probs = model.last_attention(x, spacing, query_tokens=(0,), layer=layer)
    return cls_attention_grid(probs, (model.img_size // model.patch) ** 2)[0].float().cpu()


def attention_rollout(model: PatchViT, image: np.ndarray, pixel_spacing: Optional[Tuple[float, float]] = None,
                      slice_thickness: Optional[float] = None, *, residual: float = 0.5, start_layer: int = 0,
                      input_format: Literal["hu_float", "hu16_png", "windowed_float"] = "hu_float", hu_level: float = 40.0,
                      hu_width: float = 400.0, device: Union[str, torch.device, None] = None,
                      preprocess: Literal["host", "device", "auto"] = "host") -> np.ndarray:
    """Attention rollout of the CLS token over the patches of one image: a ``(g, g)`` float32 numpy map, g = img_size / patch -- where
    in the image the CLS embedding comes from, through the attention and skip connections of every block from ``start_layer`` up
    (``PatchViT.attention_rollout``; heads averaged, ``residual`` the weight of the skip connection).  Same preprocessing, argument
    checking and spacing convention as ``attention_map``.  The map sums to 1 minus the mass that ends on CLS and the registers."""
    if device is None:
        device = next(model.parameters()).device
    x = _batch([image], model.img_size, input_format, hu_level, hu_width, device, preprocess)
    spacing = None
    if model.scale_aware:
        sx, sy = (1.0, 1.0) if pixel_spacing is None else pixel_spacing
        spacing = torch.tensor([[sx, sy, 1.0 if slice_thickness is None else slice_thickness]], dtype=torch.float32, device=device)
    _, roll = model.attention_rollout(x, spacing, query_token=0, residual=residual, start_layer=start_layer)
    return rollout_grid(roll, (model.img_size // model.patch) ** 2)[0].float().cpu().numpy()


def encode_batch(model: PatchViT, images: Sequence[np.ndarray], spacings: Sequence[Tuple[float, float, float]], *,
                 input_format: Literal["hu_float", "hu16_png", "windowed_float"] = "hu_float", hu_level: float = 40.0,
                 hu_width: float = 400.0, return_all_tokens: bool = False,
                 device: Union[str, torch.device, None] = None,
                 preprocess: Literal["host", "device", "auto"] = "host") -> torch.Tensor:
    """Same preprocessing per image as ``encode`` but ONE batched forward through the HIP engine."""
    if len(images) != len(spacings):
        raise ValueError(f"images ({len(images)}) and spacings ({len(spacings)}) must have same length")
    if device is None:
        device = next(model.parameters()).device
    x = _batch(images, model.img_size, input_format, hu_level, hu_width, device, preprocess)
    spacing = None
    if model.scale_aware:
        spacing = torch.tensor([list(s) for s in spacings], dtype=torch.float32, device=device)
    with torch.no_grad():
        feats = model(x, spacing=spacing)
    return feats if return_all_tokens else feats[:, 0:1, :]


def forward_volume_chunks(model, volume: np.ndarray, spacing: Tuple[float, float, float], *, input_format: str, hu_level: float, hu_width: float,
                          context: str, z_stride: int, batch_size: int, device: Union[str, torch.device, None], with_input: bool = False):
    """The chunk loop of a ``(Z, H, W)`` series, shared by ``encode_volume`` and ``dinox.segment.segment_volume``: checks the arguments,
    moves the volume to the device once, then yields ``(slices, model(x, spacing=...))`` per chunk of ``batch_size`` of the slices
    0, z_stride, ... -- ``x`` the chunk's 2.5D stacks, preprocessed by the kernel into one reused input buffer (each plane resized once
    for all the stacks of the chunk it shows in).  ``model`` is anything with ``img_size``, ``scale_aware`` and that call (a PatchViT, a
    SegModel).  The forward runs under no_grad in the caller's autocast state.  The checks run at the first ``next()``.
    ``with_input``: yields ``(slices, features, x)`` -- ``x`` [n, 3, S, S] fp32 is a view of the reused buffer (channel 1 = the slice's own
    plane in both contexts, see ``dinox.preprocess.stack_planes``), valid until the next ``next()``."""
    from dinox import preprocess as P
    vol = np.asarray(volume)
    if vol.ndim != 3:
        raise ValueError(f"Unsupported volume shape: {vol.shape}. Expected (Z, H, W).")
    if input_format not in _FORMATS:
        raise ValueError(f"Unknown input_format: '{input_format}'. Supported: 'hu_float', 'hu16_png', 'windowed_float'")
    if context not in P.CONTEXTS:
        raise ValueError(f"Unknown context: '{context}'. Supported: 'neighbours', 'replicate'")
    if int(z_stride) != z_stride or z_stride < 1:
        raise ValueError(f"z_stride must be an integer >= 1, got {z_stride}")
    if int(batch_size) != batch_size or batch_size < 1:
        raise ValueError(f"batch_size must be an integer >= 1, got {batch_size}")
    if min(vol.shape) < 1:
        raise ValueError(f"Unsupported volume shape: {vol.shape}. Expected (Z, H, W).")
    if device is None:
        device = next(model.parameters()).device
    device = torch.device(device)
    Z, H, W = vol.shape
    S = model.img_size
    src_dtype = P.source_dtype(vol)
    host = np.ascontiguousarray(vol, dtype=np.dtype(src_dtype))
    src = torch.from_numpy(host.view(np.int16) if src_dtype == "uint16" else host).reshape(-1).to(device)
    zs = list(range(0, Z, int(z_stride)))
    chunks = [zs[at:at + int(batch_size)] for at in range(0, len(zs), int(batch_size))]
    # every chunk's job table in one page-locked upload
    tables = [P.volume_jobs(Z, H, W, ch, context) for ch in chunks]
    for tb, ch in zip(tables, chunks):
        P.check_jobs(tb, Z * H * W, len(ch))
    jobs = torch.from_numpy(np.concatenate(tables, 0)).pin_memory().to(device, non_blocking=True) if device.type == "cuda" else None
    buf = torch.empty((len(chunks[0]), 3, S, S), dtype=torch.float32, device=device)
    sp = torch.tensor([list(spacing)], dtype=torch.float32, device=device) if model.scale_aware else None
    at = 0
    for tb, ch in zip(tables, chunks):
        n = len(ch)
        x = P.device_preprocess(src, tb if jobs is None else jobs[at:at + len(tb)], n, S, input_format, hu_level, hu_width, out=buf[:n],
                                src_dtype=src_dtype, max_side=max(H, W))
        at += len(tb)
        with torch.no_grad():
            f = model(x, spacing=None if sp is None else sp.expand(n, 3).contiguous())
        yield (ch, f, x) if with_input else (ch, f)


def encode_volume(model: PatchViT, volume: np.ndarray, spacing: Tuple[float, float, float], *,
                  input_format: Literal["hu_float", "hu16_png", "windowed_float"] = "hu_float", hu_level: float = 40.0,
                  hu_width: float = 400.0, context: Literal["neighbours", "replicate"] = "neighbours", z_stride: int = 1,
                  batch_size: int = 64, return_all_tokens: bool = False,
                  device: Union[str, torch.device, None] = None) -> torch.Tensor:
    """Features of the slices 0, z_stride, 2 z_stride, ... of a ``(Z, H, W)`` series: ``(Z', 1, D)`` (CLS) or ``(Z', N, D)``.

    Slice z is encoded as the 2.5D stack the model was trained on -- planes z-1, z, z+1, clamped at the ends of the series
    (``context="neighbours"``) -- or as plane z three times (``"replicate"``, what ``encode`` makes of an (H, W) image).
    ``spacing = (sx, sy, sz)`` holds for the whole series.  The volume crosses to the device once; chunks of ``batch_size``
    slices are preprocessed by the kernel (each plane resized once for all the stacks of the chunk it shows in) into one reused
    input buffer and forwarded (``forward_volume_chunks``).  Honours an ambient ``torch.autocast`` exactly as ``encode`` does."""
    chunks = forward_volume_chunks(model, volume, spacing, input_format=input_format, hu_level=hu_level, hu_width=hu_width, context=context,
                                   z_stride=z_stride, batch_size=batch_size, device=device)
    return torch.cat([f if return_all_tokens else f[:, 0:1, :] for _, f in chunks], 0)
